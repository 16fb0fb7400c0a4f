"""Development benchmark of the population view (rf_env_configure_view_grouped, rf_rollout_advantages_grouped).

View step: DeviceVectorDiscreteSteps on small frames (so that the view's two kernels are visible next to the render),
n = 4096, W = 4, frame_stack = 5, stepped through step_tensors() without a view (twice: their difference is the noise),
with the ungrouped view, with G = 512 (m = 8: env_view_moments_packed_kernel) and with G = 2 (m = 2048:
env_view_moments_kernel<true>), in one process, in alternating windows.  What a view costs per step is its median
microseconds per step minus the median without a view.  The ungrouped kernels are instruction for instruction the
parent commit's (profiles/population_view.md), so "ungrouped" is the parent's view at the same n.

GAE: rf_rollout_advantages against rf_rollout_advantages_grouped (G = 512) on synthetic 4096 x 32 tensors, alternating
windows of back-to-back launches timed with events.

Medians and the windows' spread; one JSON line.
usage (GPU box):  python tools/bench_population_view.py [n_envs] [frame] [spp] [--windows 8] [--steps 20] [--launches 200]
                  [--ungrouped-only]
--ungrouped-only: what a checkout without groups= can run."""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd import _native  # noqa: E402
from reinfocus_amd.environments import harness  # noqa: E402


def option(argv, name, default):
    if name in argv:
        at = argv.index(name)
        value = int(argv[at + 1])
        del argv[at:at + 2]
        return value
    return default


def summary(samples):
    return {name: {"median": float(np.median(s)), "spread": float((max(s) - min(s)) / np.median(s))}
            for name, s in samples.items()}


def view_steps(n, frame, spp, windows, steps, ungrouped_only):
    kw = dict(max_episode_steps=20, num_envs=n, frame_height=frame, samples_per_pixel=spp, seed=0, device=0,
              device_initializer=True)
    views = {"off": None, "off_again": None, "ungrouped": harness.LearnerView(frame_stack=5)}
    if not ungrouped_only:
        for name, groups in (("packed", n // 8), ("block", 2)):
            gammas = np.linspace(0.9, 1.0, groups)
            views[name] = harness.LearnerView(frame_stack=5, gamma=gammas, groups=groups)
    envs = {name: harness.DeviceVectorDiscreteSteps(learner_view=view, **kw) for name, view in views.items()}
    rng = np.random.default_rng(0)
    for env in envs.values():  # reset, and the steps before a replayed graph exists
        env.reset_tensors()
        for _ in range(3):
            env.step_tensors(torch.from_numpy(rng.integers(0, 13, n)).cuda())
    micros = {name: [] for name in envs}
    for _ in range(windows):
        for name, env in envs.items():
            actions = [torch.from_numpy(rng.integers(0, 13, n)).cuda() for _ in range(steps)]
            torch.cuda.synchronize()
            start = time.perf_counter()
            for a in actions:
                env.step_tensors(a)
            torch.cuda.synchronize()  # (nothing was waited for: the window ends when the device has finished it)
            micros[name].append(1e6 * (time.perf_counter() - start) / steps)
    out = {"us_per_step": summary(micros), "branch": envs["off"]._ctx.env_last_step_branch()}
    off = out["us_per_step"]["off"]["median"]
    out["noise_us"] = abs(off - out["us_per_step"]["off_again"]["median"])
    out["view_us_per_step"] = {name: out["us_per_step"][name]["median"] - off for name in envs
                               if not name.startswith("off")}
    for env in envs.values():
        env.close()
    return out


def gae(n, steps, windows, launches, ungrouped_only):
    from reinfocus_amd.environments import rollout

    ctx = _native.Context(0)
    rng = np.random.default_rng(1)
    rewards = torch.from_numpy(rng.standard_normal((steps, n))).cuda()
    values, final_values = (torch.from_numpy(rng.standard_normal((steps, n)).astype(np.float32)).cuda() for _ in range(2))
    truncated = torch.from_numpy((rng.random((steps, n)) < 0.1).astype(np.uint8)).cuda()
    last = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    advantages, returns = (torch.zeros((steps, n), dtype=torch.float32, device="cuda") for _ in range(2))
    groups = n // 8
    table = torch.from_numpy(rollout.discount_table(np.linspace(0.9, 1.0, groups), np.linspace(0.8, 1.0, groups))).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    common = (rewards.data_ptr(), values.data_ptr(), truncated.data_ptr(), final_values.data_ptr(), last.data_ptr())
    outputs = (advantages.data_ptr(), returns.data_ptr(), stream)
    forms = {"ungrouped": lambda: ctx.rollout_advantages(steps, n, *common, 0.99, 0.95, *outputs)}
    if not ungrouped_only:
        forms["grouped"] = lambda: ctx.rollout_advantages_grouped(steps, n, groups, *common, table.data_ptr(), *outputs)
    micros = {name: [] for name in forms}
    for call in forms.values():
        call()
    torch.cuda.synchronize()
    for _ in range(windows):
        for name, call in forms.items():
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            for _ in range(launches):
                call()
            end.record()
            torch.cuda.synchronize()
            micros[name].append(1e3 * begin.elapsed_time(end) / launches)
    ctx.close()
    return {"shape": [n, steps], "launches": launches, "us_per_launch": summary(micros)}


def main():
    argv = list(sys.argv[1:])
    windows, steps = option(argv, "--windows", 8), option(argv, "--steps", 20)
    launches = option(argv, "--launches", 200)
    ungrouped_only = "--ungrouped-only" in argv
    argv = [a for a in argv if a != "--ungrouped-only"]
    n = int(argv[0]) if len(argv) > 0 else 4096
    frame = int(argv[1]) if len(argv) > 1 else 16
    spp = int(argv[2]) if len(argv) > 2 else 1
    torch.zeros(1, device="cuda")
    out = {"envs": n, "frame": frame, "spp": spp, "windows": windows, "steps": steps,
           "view": view_steps(n, frame, spp, windows, steps, ungrouped_only),
           "gae": gae(n, 32, windows, launches, ungrouped_only)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
