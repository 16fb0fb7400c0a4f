"""Development benchmark of the population (include/reinfocus_hip.h, "population"): G independent PPO learners over one
environment of 8 G lanes at ppo_tuned.yml's DiscreteSteps-v0 shape -- m = 8 environments per learner, T = 32, minibatches
of 64, [256, 256] ReLU, frame_stack 5 -- for G = 1, 16, 64, 512:
  (a) act() and one minibatch update through DevicePopulationPolicy / DevicePopulationLearner: 1 and 3 launches;
  (b) the same work as a Python loop over G DevicePolicy / DeviceLearner objects on slices of the same tensors, with the
      same parameters: G and 3 G launches -- the only form there is without the population, and the baseline;
  (c) at G = 1 the two are the grouped path against the ungrouped one, to be read against the windows' own spread.
Alternating windows in one process, each a run of calls ended by one synchronisation; medians and the windows' spread.
Then one end-to-end iteration, DeviceRollout.collect() of 32 steps + train() of --epochs epochs, at 8 G environments of
the headline frame shape (300 x 300 px, 100 samples), through the population.
One JSON line; --markdown FILE also rewrites the measured section of that file (profiles/population.md), between its two
marker lines.
usage (GPU box):  python tools/bench_population.py [--windows 5] [--epochs 4] [--groups 1,16,64,512] [--no-e2e]
                                                   [--markdown profiles/population.md]"""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(HERE)
ARGV = list(sys.argv[1:])
from reinfocus_amd.environments import harness  # noqa: E402

PER_GROUP, STEPS, BATCH, STACK, ACTIONS = 8, 32, 64, 5, 13
NET = dict(pi=(256, 256), vf=(256, 256), activation="relu")
HYPER = dict(learning_rate=3.338099093100241e-05, clip_range=0.2, ent_coef=0.0018133869709102076,
             vf_coef=0.4969606569643988, max_grad_norm=0.3)
BEGIN, END = "<!-- bench_population: begin -->", "<!-- bench_population: end -->"


def option(name, default, kind=int):
    return kind(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def random_state(spec, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for name, _, shape, is_weight in spec.entries:
        value = rng.standard_normal(shape[::-1]) / np.sqrt(shape[0]) if is_weight else 0.1 * rng.standard_normal(shape)
        out[name] = torch.from_numpy(value.astype(np.float32)).cuda()
    return out


def windows_of(forms, windows, calls):
    """Microseconds per call: `windows` alternating windows per form, each `calls` calls and one synchronisation."""
    for form in forms.values():  # warm-up
        form()
    times = {name: [] for name in forms}
    for _ in range(windows):
        for name, form in forms.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(calls):
                form()
            torch.cuda.synchronize()  # (nothing was waited for: the window ends when the device has finished it)
            times[name].append(1e6 * (time.perf_counter() - start) / calls)
    return {name: {"median_us": float(np.median(t)), "spread": float((max(t) - min(t)) / np.median(t)),
                   "windows_us": [round(x, 2) for x in t]} for name, t in times.items()}


def stage_times(groups, windows):
    """(a) against (b) at one G, on the same parameters, observations, rows and indices."""
    lanes = groups * PER_GROUP
    env = harness.DeviceVectorDiscreteSteps(num_envs=lanes, frame_height=16, samples_per_pixel=1, seed=0, device=0,
                                            device_initializer=True, learner_view=harness.LearnerView(frame_stack=STACK))
    try:
        width = int(env.single_observation_space.shape[0])
        spec = harness.MlpPolicySpec(width, ACTIONS, **NET)
        many = harness.DevicePopulationPolicy(env, spec, groups, list(range(groups)))
        singles = [harness.DevicePolicy(env, spec, g) for g in range(groups)]
        states = [random_state(spec, 10 + g % 8) for g in range(min(groups, 8))]
        for g, single in enumerate(singles):
            single.load_state_dict(states[g % 8])
            many.load_state_dict(states[g % 8], group=g)
        rng = np.random.default_rng(groups)
        normal = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()  # noqa: E731
        obs = normal(lanes, width)
        pieces = [obs[g * PER_GROUP:(g + 1) * PER_GROUP] for g in range(groups)]
        rows = PER_GROUP * STEPS
        flat = {"observations": normal(groups * rows, width),
                "actions": torch.from_numpy(rng.integers(0, ACTIONS, groups * rows)).cuda(),
                "log_probs": -2.5 + 0.1 * normal(groups * rows), "advantages": normal(groups * rows),
                "returns": normal(groups * rows)}
        flats = [{key: value[g * rows:(g + 1) * rows] for key, value in flat.items()} for g in range(groups)]
        index = torch.from_numpy(np.stack([rng.permutation(rows)[:BATCH] for _ in range(groups)]).astype(np.int64)).cuda()
        learner = harness.DevicePopulationLearner(many, **HYPER)
        learners = [harness.DeviceLearner(single, **HYPER) for single in singles]

        def act_loop():
            for single, piece in zip(singles, pieces):
                single.act(piece)

        def update_loop():
            for g, one in enumerate(learners):
                one.update(flats[g], index[g])

        calls = max(3, 400 // groups)
        out = {"groups": groups, "parameters": spec.size,
               "act": windows_of({"grouped": lambda: many.act(obs), "loop": act_loop}, windows, calls),
               "update": windows_of({"grouped": lambda: learner.update(flat, index), "loop": update_loop}, windows,
                                    max(3, calls // 4))}
        torch.cuda.synchronize()
        out["flags"] = float(learner.update(flat, index)[:, 7].max().cpu())
        return out
    finally:
        env.close()


def iteration_time(groups, epochs, repeats):
    """collect() + train() through the population at 8 G environments of the headline frame shape; seconds."""
    lanes = groups * PER_GROUP
    env = harness.DeviceVectorDiscreteSteps(num_envs=lanes, frame_height=300, samples_per_pixel=100, seed=0, device=0,
                                            device_initializer=True, episode_records=True,
                                            learner_view=harness.LearnerView(frame_stack=STACK))
    try:
        spec = harness.MlpPolicySpec(int(env.single_observation_space.shape[0]), ACTIONS, **NET)
        policy = harness.DevicePopulationPolicy(env, spec, groups, list(range(groups)))
        policy.load_state_dict(random_state(spec, 3))
        learner = harness.DevicePopulationLearner(policy, **HYPER)
        rollout = harness.DeviceRollout(env, STEPS, 0.9, 0.99)
        rollout.start(env.reset_tensors()[0])
        collects, trains = [], []
        for repeat in range(repeats + 1):  # (the first one warms up)
            if repeat:
                rollout.start()
            torch.cuda.synchronize()
            start = time.perf_counter()
            rollout.collect(policy)
            torch.cuda.synchronize()
            middle = time.perf_counter()
            stats = learner.train(rollout, epochs, BATCH)
            torch.cuda.synchronize()
            end = time.perf_counter()
            if repeat:
                collects.append(middle - start)
                trains.append(end - middle)
        assert env.device_fault() is None
        return {"groups": groups, "envs": lanes, "epochs": epochs, "updates": int(stats.shape[0]),
                "collect_s": float(np.median(collects)), "train_s": float(np.median(trains)),
                "env_steps_per_s": float(lanes * STEPS / (np.median(collects) + np.median(trains))),
                "flags": float(stats[:, :, 7].max().cpu())}
    finally:
        env.close()


def markdown(stages, iterations):
    lines = [BEGIN, "", "| G | call | grouped (us) | spread | loop over G objects (us) | spread | loop / grouped |",
             "|---|---|---|---|---|---|---|"]
    for r in stages:
        for call in ("act", "update"):
            a, b = r[call]["grouped"], r[call]["loop"]
            lines.append(f"| {r['groups']} | {call} | {a['median_us']:.1f} | {100 * a['spread']:.0f} % | {b['median_us']:.1f} | "
                         f"{100 * b['spread']:.0f} % | {b['median_us'] / a['median_us']:.2f} |")
    if iterations:
        lines += ["", "| G | environments | collect of 32 steps (s) | train (s) | updates | env-steps/s |", "|---|---|---|---|---|---|"]
        for r in iterations:
            lines.append(f"| {r['groups']} | {r['envs']} | {r['collect_s']:.3f} | {r['train_s']:.4f} | {r['updates']} | "
                         f"{r['env_steps_per_s']:.0f} |")
    return "\n".join(lines + ["", END])


def main():
    windows, epochs = option("--windows", 5), option("--epochs", 4)
    groups = [int(g) for g in option("--groups", "1,16,64,512", str).split(",")]
    torch.zeros(1, device="cuda")
    stages = [stage_times(g, windows) for g in groups]
    iterations = [] if "--no-e2e" in ARGV else [iteration_time(g, epochs, 2) for g in groups]
    print(json.dumps({"windows": windows, "stages": stages, "iterations": iterations}))
    if "--markdown" in ARGV:
        path = ARGV[ARGV.index("--markdown") + 1]
        text = open(path).read()
        start, end = text.index(BEGIN), text.index(END) + len(END)
        open(path, "w").write(text[:start] + markdown(stages, iterations) + text[end:])


if __name__ == "__main__":
    main()
