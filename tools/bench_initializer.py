"""Development benchmark of the device initializer (rf_env_configure_initializer): harness.DeviceVectorDiscreteSteps with
random actions, device_initializer=False (the host draws a pool of candidate reset states every step, uploads it and
draws the used rows again) against device_initializer=True (the device draws them), in one process.  Rounds of
alternating windows of env-steps/s; per round the median of each path's windows, then the median of the rounds.  The
spread is the host-pool path's own: (max - min) / median of its windows within a round (the largest of the rounds) and of
its round medians.  The device path is accepted when its median is not lower than the host-pool path's by more than the
larger of the two.  Also: the host time a step of the host-pool path spends in propose() and initialize(), measured in
windows of their own (the pool's upload is 8 B/env of the step's one copy in and cannot be told apart on the host).
One JSON line per shape.
usage (GPU box):  python tools/bench_initializer.py [--rounds 3] [--windows 6] [--steps 10] [n_envs frame spp]
without a shape: 4096 x 256 x 16, 8 x 300 x 100 and 32768 x 16 x 1 in turn."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness  # noqa: E402

SHAPES = [(4096, 256, 16), (8, 300, 100), (32768, 16, 1)]


def option(argv, name, default):
    if name in argv:
        at = argv.index(name)
        value = int(argv[at + 1])
        del argv[at:at + 2]
        return value
    return default


class Timed:
    """An initializer whose propose / initialize calls are timed."""

    def __init__(self, initializer):
        self._initializer = initializer
        self.seconds = 0.0

    def propose(self, num_envs):
        start = time.perf_counter()
        rows = self._initializer.propose(num_envs)
        self.seconds += time.perf_counter() - start
        return rows

    def initialize(self, num_envs):
        start = time.perf_counter()
        rows = self._initializer.initialize(num_envs)
        self.seconds += time.perf_counter() - start
        return rows


def window(env, rng, n, steps):
    actions = [rng.integers(0, 13, n) for _ in range(steps)]
    start = time.perf_counter()
    for a in actions:
        env.step(a)
    return n * steps / (time.perf_counter() - start)


def spread(values):
    return (max(values) - min(values)) / float(np.median(values))


def bench(n, frame, spp, rounds, windows, steps):
    kw = dict(num_envs=n, frame_height=frame, samples_per_pixel=spp, seed=0, device=0)
    envs = {"host_pool": harness.DeviceVectorDiscreteSteps(**kw),
            "device": harness.DeviceVectorDiscreteSteps(device_initializer=True, **kw)}
    rng = np.random.default_rng(0)
    for env in envs.values():  # reset, and the steps before a replayed graph exists
        env.reset()
        for _ in range(3):
            env.step(rng.integers(0, 13, n))
    rates = {name: [[] for _ in range(rounds)] for name in envs}
    for r in range(rounds):
        for _ in range(windows):
            for name, env in envs.items():
                rates[name][r].append(window(env, rng, n, steps))
    round_medians = {name: [float(np.median(w)) for w in per_round] for name, per_round in rates.items()}
    medians = {name: float(np.median(m)) for name, m in round_medians.items()}
    within = max(spread(w) for w in rates["host_pool"])
    between = spread(round_medians["host_pool"])
    # the host-pool path's propose + initialize, in windows of their own (the wrapper is not in the compared windows)
    host = envs["host_pool"]
    host._initializer = timed = Timed(host._initializer)
    start = time.perf_counter()
    for _ in range(windows):
        window(host, rng, n, steps)
    host_step_us = (time.perf_counter() - start) / (windows * steps) * 1e6
    host_draw_us = timed.seconds / (windows * steps) * 1e6
    host._initializer = timed._initializer
    change = medians["device"] / medians["host_pool"] - 1.0
    out = {"envs": n, "frame": frame, "spp": spp, "rounds": rounds, "windows": windows, "steps": steps,
           "branch": {name: env._ctx.env_last_step_branch() for name, env in envs.items()},
           "median_env_steps_per_s": medians, "round_medians_env_steps_per_s": round_medians,
           "windows_env_steps_per_s": rates, "device_vs_host_pool": change,
           "host_pool_spread_within_round": within, "host_pool_spread_between_rounds": between,
           "accepted": bool(change >= -max(within, between)),
           "host_pool_step_us": host_step_us, "host_pool_propose_initialize_us_per_step": host_draw_us,
           "pool_upload_bytes_per_step": 8 * n, "step_upload_bytes": {"host_pool": 12 * n, "device": 4 * n}}
    print(json.dumps(out), flush=True)
    for env in envs.values():
        env.close()
    return out


def main():
    argv = list(sys.argv[1:])
    rounds, windows, steps = option(argv, "--rounds", 3), option(argv, "--windows", 6), option(argv, "--steps", 10)
    shapes = [tuple(int(a) for a in argv[:3])] if len(argv) >= 3 else SHAPES
    results = [bench(n, frame, spp, rounds, windows, steps) for n, frame, spp in shapes]
    sys.exit(0 if all(r["accepted"] for r in results) else 1)


if __name__ == "__main__":
    main()
