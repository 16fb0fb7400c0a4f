"""Development benchmark of the rollout's end (rf_rollout_advantages, DeviceRollout.finish): GAE advantages and returns
by rollout_gae_kernel -- one launch -- against the obvious torch form of the same definition, a Python loop over T with
about eight small launches per step, on the same device tensors in the same process.  Alternating windows, medians, the
windows' spread; the two forms are also compared bit for bit.  Then the share of a whole rollout (T environment steps
through DeviceRollout.step and one finish) that each form takes.  One JSON line.
usage (GPU box):  python tools/bench_rollout.py [--windows 7] [--calls 20] [--no-rollouts]
Shapes (profiles/rollout.md): 128 steps x 8 environments (the reference's PPO configurations) and 32 x 4096; whole
rollouts at 8 x 300 x 300 px x 100 samples and at the headline shape 4096 x 256 x 256 px x 16 samples."""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd import _native  # noqa: E402
from reinfocus_amd.environments import harness  # noqa: E402

GAMMA, GAE_LAMBDA = 0.99, 0.95


def option(argv, name, default):
    if name in argv:
        at = argv.index(name)
        value = int(argv[at + 1])
        del argv[at:at + 2]
        return value
    return default


def torch_gae(rewards, values, truncated, final_values, last_values, advantages, returns):
    """include/reinfocus_hip.h "rollout", in eager torch: float32 throughout, one step of the chain per iteration."""
    g, gl = float(np.float32(GAMMA)), float(np.float32(GAMMA * GAE_LAMBDA))
    steps = rewards.shape[0]
    r = rewards.to(torch.float32)
    if final_values is not None:
        r = torch.where(truncated != 0, r + g * final_values, r)
    nnt = 1.0 - truncated.to(torch.float32)
    last = torch.zeros_like(last_values)
    for t in range(steps - 1, -1, -1):
        next_v = last_values if t == steps - 1 else values[t + 1]
        delta = (r[t] + (g * next_v) * nnt[t]) - values[t]
        last = delta + (gl * nnt[t]) * last
        advantages[t] = last
    torch.add(advantages, values, out=returns)


def finish_times(ctx, steps, n, windows, calls):
    rng = np.random.default_rng(steps + n)
    rewards = torch.from_numpy(rng.standard_normal((steps, n))).cuda()
    values = torch.from_numpy(rng.standard_normal((steps, n)).astype(np.float32)).cuda()
    truncated = torch.from_numpy((rng.random((steps, n)) < 0.1).astype(np.uint8)).cuda()
    final_values = torch.from_numpy(rng.standard_normal((steps, n)).astype(np.float32)).cuda()
    final_values[truncated == 0] = float("nan")
    last_values = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
    outputs = {name: (torch.empty_like(values), torch.empty_like(values)) for name in ("kernel", "torch_loop")}
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        advantages, returns = outputs["kernel"]
        ctx.rollout_advantages(steps, n, rewards.data_ptr(), values.data_ptr(), truncated.data_ptr(),
                               final_values.data_ptr(), last_values.data_ptr(), GAMMA, GAE_LAMBDA, advantages.data_ptr(),
                               returns.data_ptr(), stream)

    def torch_loop():
        torch_gae(rewards, values, truncated, final_values, last_values, *outputs["torch_loop"])

    forms = {"kernel": kernel, "torch_loop": torch_loop}
    for form in forms.values():  # warm-up
        form()
    torch.cuda.synchronize()
    equal = all(np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
                for a, b in zip(outputs["kernel"], outputs["torch_loop"]))
    times = {name: [] for name in forms}
    for _ in range(windows):
        for name, form in forms.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(calls):
                form()
            torch.cuda.synchronize()  # (nothing was waited for: the window ends when the device has finished it)
            times[name].append(1e6 * (time.perf_counter() - start) / calls)
    medians = {name: float(np.median(t)) for name, t in times.items()}
    return {"steps": steps, "envs": n, "median_us": medians, "bit_equal": bool(equal),
            "spread": {name: float((max(t) - min(t)) / np.median(t)) for name, t in times.items()},
            "windows_us": {name: [round(x, 2) for x in t] for name, t in times.items()},
            "torch_loop_over_kernel": medians["torch_loop"] / medians["kernel"]}


def rollout_share(steps, n, frame, spp, windows, finish_us):
    """Seconds of `steps` environment steps through DeviceRollout.step (a policy of two elementwise launches), without
    the finish; and the share finish() would add in either form (its times from finish_times)."""
    env = harness.DeviceVectorDiscreteSteps(max_episode_steps=20, num_envs=n, frame_height=frame, samples_per_pixel=spp,
                                            seed=0, device=0, device_initializer=True, episode_records=True,
                                            learner_view=harness.LearnerView(frame_stack=5))
    buffer = harness.DeviceRollout(env, steps, GAMMA, GAE_LAMBDA)
    rng = np.random.default_rng(0)
    actions = [torch.from_numpy(rng.integers(0, 13, n)).cuda() for _ in range(steps)]
    obs = env.reset_tensors()[0]
    seconds = []
    for window in range(windows + 1):  # (the first one warms up: the replayed graph exists from the second step on)
        torch.cuda.synchronize()
        start = time.perf_counter()
        buffer.start(obs if window == 0 else None)
        for t in range(steps):
            values = obs[:, 0] * 0.5
            obs, _, _, _, info = buffer.step(actions[t], values, -values)
            buffer.bootstrap(info["final_observation"][:, 0] * 0.5)
        torch.cuda.synchronize()
        if window:
            seconds.append(time.perf_counter() - start)
        buffer.finish(obs[:, 0] * 0.5)
    torch.cuda.synchronize()
    env.close()
    collect = float(np.median(seconds))
    return {"steps": steps, "envs": n, "frame": frame, "spp": spp, "median_collect_ms": 1e3 * collect,
            "us_per_env_step_call": 1e6 * collect / steps,
            "finish_share": {name: us * 1e-6 / (collect + us * 1e-6) for name, us in finish_us.items()}}


def main():
    argv = list(sys.argv[1:])
    windows, calls = option(argv, "--windows", 7), option(argv, "--calls", 20)
    torch.zeros(1, device="cuda")
    ctx = _native.Context(0)
    out = {"windows": windows, "calls": calls, "finish": [finish_times(ctx, 128, 8, windows, calls),
                                                          finish_times(ctx, 32, 4096, windows, calls)]}
    ctx.close()
    if "--no-rollouts" not in argv:
        out["rollout"] = [rollout_share(128, 8, 300, 100, 3, out["finish"][0]["median_us"]),
                          rollout_share(32, 4096, 256, 16, 3, out["finish"][1]["median_us"])]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
