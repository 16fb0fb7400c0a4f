"""Development benchmark of the learner view (rf_env_configure_view): DeviceVectorDiscreteSteps stepped without a view
(twice: their difference is the noise) and with LearnerView(frame_stack=5), in one process, through step() and through
step_tensors().  Medians of alternating windows of env-steps/s and the windows' spread; one JSON line.
usage (GPU box):  python tools/bench_learner_view.py [n_envs] [frame] [spp] [--windows 6] [--steps 10] [--off-only]
--off-only: the two environments without a view alone (what a checkout without the keyword can run).
The shapes of profiles/learner_view.md: 4096 256 16, 8 300 100 and 1 64 1."""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness  # noqa: E402


def option(argv, name, default):
    if name in argv:
        at = argv.index(name)
        value = int(argv[at + 1])
        del argv[at:at + 2]
        return value
    return default


def windows_of(envs, n, steps, windows, tensors, rng):
    rates = {name: [] for name in envs}
    for _ in range(windows):
        for name, env in envs.items():
            actions = [rng.integers(0, 13, n) for _ in range(steps)]
            if tensors:
                actions = [torch.from_numpy(a).cuda() for a in actions]
                torch.cuda.synchronize()
            start = time.perf_counter()
            for a in actions:
                (env.step_tensors if tensors else env.step)(a)
            if tensors:  # (nothing was waited for: the window ends when the device has finished it)
                torch.cuda.synchronize()
            rates[name].append(n * steps / (time.perf_counter() - start))
    return rates


def main():
    argv = list(sys.argv[1:])
    windows, steps = option(argv, "--windows", 6), option(argv, "--steps", 10)
    off_only = "--off-only" in argv
    argv = [a for a in argv if a != "--off-only"]
    n = int(argv[0]) if len(argv) > 0 else 4096
    frame = int(argv[1]) if len(argv) > 1 else 256
    spp = int(argv[2]) if len(argv) > 2 else 16
    torch.zeros(1, device="cuda")
    kw = dict(max_episode_steps=20, num_envs=n, frame_height=frame, samples_per_pixel=spp, seed=0, device=0,
              device_initializer=True)
    envs = {"off": harness.DeviceVectorDiscreteSteps(**kw), "off_again": harness.DeviceVectorDiscreteSteps(**kw)}
    if not off_only:
        envs["on"] = harness.DeviceVectorDiscreteSteps(learner_view=harness.LearnerView(frame_stack=5), **kw)
    rng = np.random.default_rng(0)
    out = {"envs": n, "frame": frame, "spp": spp, "windows": windows, "steps": steps}
    for form, tensors in (("step", False), ("step_tensors", True)):
        for env in envs.values():  # reset, and the steps before a replayed graph exists
            env.reset()
            for _ in range(3):
                if tensors:
                    env.step_tensors(torch.from_numpy(rng.integers(0, 13, n)).cuda())
                else:
                    env.step(rng.integers(0, 13, n))
        rates = windows_of(envs, n, steps, windows, tensors, rng)
        medians = {name: float(np.median(r)) for name, r in rates.items()}
        result = {"median_env_steps_per_s": medians,
                  "spread": {name: float((max(r) - min(r)) / np.median(r)) for name, r in rates.items()},
                  "median_us_per_step": {name: 1e6 * n / m for name, m in medians.items()},
                  "noise": abs(medians["off"] - medians["off_again"]) / medians["off"],
                  "branch": envs["off"]._ctx.env_last_step_branch()}
        if not off_only:
            result["on_vs_off"] = medians["on"] / medians["off"] - 1.0
        out[form] = result
    print(json.dumps(out))
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    main()
