"""Development benchmark of the observer program (rf_env_configure_observed): the composition that restates
DiscreteSteps, stepped as harness.DeviceVectorEnvironment with the built-in observer (twice: their difference is the
noise), with the default observer restated as a tree (harness.default_observer) and with a 12-column tree (a normalised
delta of a delta over target, focus plane and focus value), in one process.  Medians of alternating windows of env-steps/s;
one JSON line.
usage (GPU box):  python tools/bench_observer.py [n_envs] [frame] [spp] [--windows 6] [--steps 10] [--built-in-only]
--built-in-only: the two built-in environments alone (what a checkout without observer programs can run)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import episode_ender as ee  # noqa: E402
from reinfocus_amd.environments import episode_rewarder as er  # noqa: E402
from reinfocus_amd.environments import harness  # noqa: E402
from reinfocus_amd.environments import state_initializer as si  # noqa: E402
from reinfocus_amd.environments import state_transformer as st  # noqa: E402

ENDS = (5.0, 10.0)
MOVES = 5.0 / 2.0 ** np.arange(6)


def strategies(n, observation_index=1):
    return dict(ender=ee.TimeLimitEnder(n, 20) | ee.DivergingEnder(n, (0, 1), 0.125, 3),
                initializer=si.RangedInitializer([[ENDS], [ENDS]], seed=0),
                rewarder=er.DeltaRewarder(1, 0.5) + er.ObservationRewarder(observation_index)
                + er.OnTargetRewarder((0, 1), 0.25),
                transformer=st.DiscreteMoveTransformer(n, 1, ENDS, np.concatenate([-MOVES, [0], MOVES[::-1]])), num_envs=n)


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
    built_in_only = "--built-in-only" in argv
    argv = [a for a in argv if a != "--built-in-only"]
    n = int(argv[0]) if len(argv) > 0 else 4096
    frame = int(argv[1]) if len(argv) > 1 else 256
    spp = int(argv[2]) if len(argv) > 2 else 16
    kw = dict(frame_height=frame, samples_per_pixel=spp, device=0)
    envs = {"built_in": harness.DeviceVectorEnvironment(**strategies(n), **kw),
            "built_in_again": harness.DeviceVectorEnvironment(**strategies(n), **kw)}
    if not built_in_only:
        from reinfocus_amd.environments import state_observer as so
        from reinfocus_amd.graphics import render

        described = render.FastRenderer(samples_per_pixel=spp, device=0)
        envs["default_tree"] = harness.DeviceVectorEnvironment(
            **strategies(n), observer=harness.default_observer(n, ENDS, 5.0, described, frame))
        leaves = [so.IndexedElementObserver(n, 0, *ENDS), so.IndexedElementObserver(n, 1, *ENDS),
                  so.FocusObserver(n, 0, 1, ENDS, described, frame)]
        envs["twelve_columns"] = harness.DeviceVectorEnvironment(
            **strategies(n, 2), observer=so.NormalizedObserver(so.DeltaObserver(so.DeltaObserver(leaves, True), True)),
            focus_observation_index=2)
    rng = np.random.default_rng(0)
    for env in envs.values():  # reset, and the steps before a replayed graph exists
        env.reset(seed=0)
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
           "noise": abs(medians["built_in"] - medians["built_in_again"]) / medians["built_in"]}
    if not built_in_only:
        out["default_tree_vs_built_in"] = medians["default_tree"] / medians["built_in"] - 1.0
        out["width"] = {"default_tree": 4, "twelve_columns": 12}
    print(json.dumps(out))
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    main()
