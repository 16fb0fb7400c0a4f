"""Development benchmark of episode records (rf_env_configure_records): DeviceVectorDiscreteSteps stepped without records
(twice: their difference is the noise) and with them, in one process.  Medians of alternating windows of env-steps/s; one
JSON line.
usage (GPU box):  python tools/bench_episode_records.py [n_envs] [frame] [spp] [--windows 6] [--steps 10] [--off-only]
--off-only: the two environments without records alone (what a checkout without the keyword can run)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness  # noqa: E402


def option(argv, name, default):
    if name in argv:
        at = argv.index(name)
        value = int(argv[at + 1])
        del argv[at:at + 2]
        return value
    return default


def main():
    argv = list(sys.argv[1:])
    windows, steps = option(argv, "--windows", 6), option(argv, "--steps", 10)
    off_only = "--off-only" in argv
    argv = [a for a in argv if a != "--off-only"]
    n = int(argv[0]) if len(argv) > 0 else 4096
    frame = int(argv[1]) if len(argv) > 1 else 256
    spp = int(argv[2]) if len(argv) > 2 else 16
    kw = dict(max_episode_steps=20, num_envs=n, frame_height=frame, samples_per_pixel=spp, seed=0, device=0)
    envs = {"off": harness.DeviceVectorDiscreteSteps(**kw), "off_again": harness.DeviceVectorDiscreteSteps(**kw)}
    if not off_only:
        envs["on"] = harness.DeviceVectorDiscreteSteps(episode_records=True, **kw)
    rng = np.random.default_rng(0)
    for env in envs.values():  # reset, and the steps before a replayed graph exists
        env.reset()
        for _ in range(3):
            env.step(rng.integers(0, 13, n))
    rates = {name: [] for name in envs}
    for _ in range(windows):
        for name, env in envs.items():
            actions = [rng.integers(0, 13, n) for _ in range(steps)]
            start = time.perf_counter()
            for a in actions:
                env.step(a)
            rates[name].append(n * steps / (time.perf_counter() - start))
    medians = {name: float(np.median(r)) for name, r in rates.items()}
    out = {"envs": n, "frame": frame, "spp": spp, "windows": windows, "steps": steps,
           "median_env_steps_per_s": medians, "windows_env_steps_per_s": rates,
           "noise": abs(medians["off"] - medians["off_again"]) / medians["off"],
           "branch": envs["off"]._ctx.env_last_step_branch()}
    if not off_only:
        out["on_vs_off"] = medians["on"] / medians["off"] - 1.0
    print(json.dumps(out))
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    main()
