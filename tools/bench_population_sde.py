"""Development benchmark of the population of gSDE learners (include/reinfocus_hip.h, "population sde"): G independent
learners over one ContinuousJumps environment of 8 G lanes at ppo_tuned.yml's ContinuousJumps-v0 shape -- m = 8 environments
per learner, T = 128, minibatches of 512, [64, 64] ReLU, frame_stack 5 -- for G = 1, 16, 64, 512:
  (a) reset_noise(), act() and one minibatch update through DeviceSdePopulationPolicy / DevicePopulationLearner: 1, 1 and
      3 launches;
  (b) the same work as a Python loop over G DeviceSdePolicy / DeviceLearner objects on slices of the same tensors, with
      the same parameters: G, G and 3 G launches -- the only form there is without the population, and the baseline;
  (c) at G = 1 the two are the grouped path against the ungrouped one, to be read against the windows' own spread.
Alternating windows in one process, each a run of calls ended by one synchronisation; medians and the windows' spread.
One JSON line; --markdown FILE also rewrites the measured section of that file (profiles/population_sde.md), between its
two marker lines.
usage (GPU box):  python tools/bench_population_sde.py [--windows 5] [--groups 1,16,64,512]
                                                       [--markdown profiles/population_sde.md]"""
import json
import os
import sys

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(HERE)
ARGV = list(sys.argv[1:])
from reinfocus_amd.environments import harness  # noqa: E402
from tools.bench_population import option, random_state, windows_of  # noqa: E402

PER_GROUP, STEPS, BATCH, STACK = 8, 128, 512, 5
NET = dict(pi=(64, 64), vf=(64, 64), activation="relu", log_std_init=-0.8696787910863373)
HYPER = dict(learning_rate=0.0004305249051633182, clip_range=0.2, ent_coef=3.039717996777601e-08,
             vf_coef=0.9269765257976839, max_grad_norm=0.8)
BEGIN, END = "<!-- bench_population_sde: begin -->", "<!-- bench_population_sde: end -->"
CALLS = ("reset_noise", "act", "update")


def stage_times(groups, windows):
    """(a) against (b) at one G, on the same parameters, observations, rows and indices."""
    lanes = groups * PER_GROUP
    env = harness.DeviceVectorContinuousJumps(num_envs=lanes, frame_height=16, samples_per_pixel=1, seed=0, device=0,
                                              device_initializer=True, learner_view=harness.LearnerView(frame_stack=STACK))
    try:
        width = int(env.single_observation_space.shape[0])
        spec = harness.SdePolicySpec(width, **NET)
        many = harness.DeviceSdePopulationPolicy(env, spec, groups, list(range(groups)))
        singles = [harness.DeviceSdePolicy(env, spec, g) for g in range(groups)]
        states = [random_state(spec, 10 + g) for g in range(min(groups, 8))]
        for state in states:
            state["log_std"].fill_(NET["log_std_init"])
        for g, single in enumerate(singles):
            single.load_state_dict(states[g % 8])
            many.load_state_dict(states[g % 8], group=g)
        rng = np.random.default_rng(groups)
        normal = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()  # noqa: E731
        obs = normal(lanes, width)
        pieces = [obs[g * PER_GROUP:(g + 1) * PER_GROUP] for g in range(groups)]
        rows = PER_GROUP * STEPS
        flat = {"observations": normal(groups * rows, width), "actions": 0.5 * normal(groups * rows),
                "log_probs": -1.0 + 0.1 * normal(groups * rows), "advantages": normal(groups * rows),
                "returns": normal(groups * rows)}
        flats = [{key: value[g * rows:(g + 1) * rows] for key, value in flat.items()} for g in range(groups)]
        index = torch.from_numpy(np.stack([rng.permutation(rows)[:BATCH] for _ in range(groups)]).astype(np.int64)).cuda()
        learner = harness.DevicePopulationLearner(many, **HYPER)
        learners = [harness.DeviceLearner(single, **HYPER) for single in singles]

        def reset_loop():
            for single in singles:
                single.reset_noise(PER_GROUP)

        def act_loop():
            for single, piece in zip(singles, pieces):
                single.act(piece)

        def update_loop():
            for g, one in enumerate(learners):
                one.update(flats[g], index[g])

        calls = max(3, 400 // groups)
        out = {"groups": groups, "parameters": spec.size,
               "reset_noise": windows_of({"grouped": many.reset_noise, "loop": reset_loop}, windows, calls),
               "act": windows_of({"grouped": lambda: many.act(obs), "loop": act_loop}, windows, calls),
               "update": windows_of({"grouped": lambda: learner.update(flat, index), "loop": update_loop}, windows,
                                    max(3, calls // 4))}
        torch.cuda.synchronize()
        out["flags"] = float(learner.update(flat, index)[:, 7].max().cpu())
        return out
    finally:
        env.close()


def markdown(stages):
    lines = [BEGIN, "", "| G | call | grouped (us) | spread | loop over G objects (us) | spread | loop / grouped |",
             "|---|---|---|---|---|---|---|"]
    for r in stages:
        for call in CALLS:
            a, b = r[call]["grouped"], r[call]["loop"]
            lines.append(f"| {r['groups']} | {call} | {a['median_us']:.1f} | {100 * a['spread']:.0f} % | {b['median_us']:.1f} | "
                         f"{100 * b['spread']:.0f} % | {b['median_us'] / a['median_us']:.2f} |")
    lines += ["", "Flags of a last update, the largest over the groups: "
              + ", ".join(f"G = {r['groups']}: {r['flags']:.0f}" for r in stages) + "."]
    return "\n".join(lines + ["", END])


def main():
    windows = option("--windows", 5)
    groups = [int(g) for g in option("--groups", "1,16,64,512", str).split(",")]
    torch.zeros(1, device="cuda")
    stages = [stage_times(g, windows) for g in groups]
    print(json.dumps({"windows": windows, "stages": stages}))
    if "--markdown" in ARGV:
        path = ARGV[ARGV.index("--markdown") + 1]
        text = open(path).read()
        start, end = text.index(BEGIN), text.index(END) + len(END)
        open(path, "w").write(text[:start] + markdown(stages) + text[end:])


if __name__ == "__main__":
    main()
