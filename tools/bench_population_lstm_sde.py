"""Development benchmark of the population of recurrent gSDE learners (include/reinfocus_hip.h, "population lstm sde"): G
independent learners over one ContinuousJumps environment of 8 G lanes at the shape of the reference's
examples/ppo_lstm_untuned.yml per learner -- m = 8, T = 128, B = 128, H = 256, [64, 64] tanh -- for G = 1, 16, 64, 512:
  (a) reset_noise(), act() and train() of one epoch (8 updates, each timed as 1 / 8 of it) through
      DevicePopulationLstmSdePolicy / DevicePopulationLearner: 1 launch each and 6 launches per update;
  (b) the same work as a Python loop over G DeviceLstmSdePolicy / DeviceLstmLearner objects on contiguous copies of the
      groups' slices (made outside the timed windows), with the same parameters: G launches each and 6 G per update -- the
      only form there is without the population, and the baseline;
  (c) at G = 1 the two are the grouped path against the ungrouped one, to be read against the windows' own spread.
Alternating windows in one process, each a run of calls ended by one synchronisation; medians and the windows' spread.
One JSON line; --markdown FILE also rewrites the measured section of that file (profiles/population_lstm_sde.md), between
its two marker lines.
usage (GPU box):  python tools/bench_population_lstm_sde.py [--windows 5] [--groups 1,16,64,512]
                                                            [--markdown profiles/population_lstm_sde.md]"""
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
from tools.bench_population_lstm import Finished  # noqa: E402

PER_GROUP, STEPS, BATCH = 8, 128, 128
NET = dict(lstm_hidden=256, pi=(64, 64), vf=(64, 64), activation="tanh")
HYPER = dict(learning_rate=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)
BEGIN, END = "<!-- bench_population_lstm_sde: begin -->", "<!-- bench_population_lstm_sde: end -->"
CALLS = ("reset_noise", "act", "update")


def stage_times(groups, windows):
    """(a) against (b) at one G, on the same parameters, observations, rows, starts and states."""
    lanes = groups * PER_GROUP
    kw = dict(frame_height=16, samples_per_pixel=1, seed=0, device=0, device_initializer=True)
    env = harness.DeviceVectorContinuousJumps(num_envs=lanes, **kw)
    small = harness.DeviceVectorContinuousJumps(num_envs=PER_GROUP, **kw)  # (what the stand-alone objects are built over)
    try:
        width, hidden = int(env.single_observation_space.shape[0]), NET["lstm_hidden"]
        spec = harness.LstmSdePolicySpec(width, **NET)
        many = harness.DevicePopulationLstmSdePolicy(env, spec, groups, list(range(groups)))
        singles = [harness.DeviceLstmSdePolicy(small, spec, g) for g in range(groups)]
        rng = np.random.default_rng(groups)
        states = [random_state(spec, 10 + g) for g in range(min(groups, 8))]
        for state in states:  # (a log_std per parameter set, in the range the search draws log_std_init from)
            state["log_std"] = torch.from_numpy(rng.uniform(-1.5, 0.0, (spec.latent, 1)).astype(np.float32)).cuda()
        for g, single in enumerate(singles):
            single.load_state_dict(states[g % 8])
            many.load_state_dict(states[g % 8], group=g)
        normal = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()  # noqa: E731
        obs = normal(lanes, width)
        starts = torch.from_numpy((rng.random(lanes) < 0.05).astype(np.uint8)).cuda()
        pieces = [(obs[g * PER_GROUP:(g + 1) * PER_GROUP], starts[g * PER_GROUP:(g + 1) * PER_GROUP]) for g in range(groups)]
        rows = PER_GROUP * STEPS
        parts = {"observations": normal(groups * rows, width), "actions": 0.5 * normal(groups * rows),
                 "log_probs": -1.0 + 0.1 * normal(groups * rows), "advantages": normal(groups * rows),
                 "returns": normal(groups * rows),
                 "episode_starts": torch.from_numpy((rng.random((STEPS + 1, lanes)) < 0.03).astype(np.uint8)).cuda(),
                 "lstm_states": 0.5 * normal(STEPS + 1, 2, 2, lanes, hidden)}
        rollout = Finished(env, parts, STEPS, lanes)
        rollouts = []
        for g in range(groups):  # contiguous copies of the slices, outside the timed windows
            piece = {key: parts[key][g * rows:(g + 1) * rows].contiguous()
                     for key in ("observations", "actions", "log_probs", "advantages", "returns")}
            piece["episode_starts"] = parts["episode_starts"][:, g * PER_GROUP:(g + 1) * PER_GROUP].contiguous()
            piece["lstm_states"] = parts["lstm_states"][:, :, :, g * PER_GROUP:(g + 1) * PER_GROUP, :].contiguous()
            rollouts.append(Finished(small, piece, STEPS, PER_GROUP))
        learner = harness.DevicePopulationLearner(many, **HYPER)
        learners = [harness.DeviceLstmLearner(single, **HYPER) for single in singles]
        splits = [[int(s) for s in rng.integers(rows, size=groups)]]
        updates = -(-rows // BATCH)
        many.reset_noise()
        for single in singles:
            single.reset_noise()

        def noise_loop():
            for single in singles:
                single.reset_noise()

        def act_loop():
            for single, (piece, flags) in zip(singles, pieces):
                single.act(piece, flags)

        def train_loop():
            for g, one in enumerate(learners):
                one.train(rollouts[g], 1, BATCH, splits=[splits[0][g]])

        calls = max(3, 400 // groups)
        trains = max(1, 32 // groups)
        out = {"groups": groups, "parameters": spec.size, "updates_per_train": updates,
               "reset_noise": windows_of({"grouped": many.reset_noise, "loop": noise_loop}, windows, calls),
               "act": windows_of({"grouped": lambda: many.act(obs, starts), "loop": act_loop}, windows, calls),
               "train": windows_of({"grouped": lambda: learner.train(rollout, 1, BATCH, splits), "loop": train_loop},
                                   windows, trains)}
        out["update"] = {form: {"median_us": t["median_us"] / updates, "spread": t["spread"]}
                         for form, t in out["train"].items()}
        torch.cuda.synchronize()
        out["flags"] = float(learner.train(rollout, 1, BATCH, splits)[:, :, 7].max().cpu())
        return out
    finally:
        env.close()
        small.close()


def markdown(stages):
    lines = [BEGIN, "", "| G | call | grouped (us) | spread | loop over G objects (us) | spread | loop / grouped |",
             "|---|---|---|---|---|---|---|"]
    for r in stages:
        for call in CALLS:
            a, b = r[call]["grouped"], r[call]["loop"]
            lines.append(f"| {r['groups']} | {call} | {a['median_us']:.1f} | {100 * a['spread']:.0f} % | "
                         f"{b['median_us']:.1f} | {100 * b['spread']:.0f} % | {b['median_us'] / a['median_us']:.2f} |")
    lines += ["", "`update` is one of the 8 updates of a `train()` of one epoch (the call's time / 8).  Flags of a last "
              "train(), the largest over updates and groups: "
              + ", ".join(f"G = {r['groups']}: {r['flags']:.0f}" for r in stages) + "."]
    return "\n".join(lines + ["", END])


def main():
    windows = option("--windows", 5)
    groups = [int(g) for g in option("--groups", "1,16,64,512", str).split(",")]
    torch.zeros(1, device="cuda")
    stages = []
    for g in groups:
        stages.append(stage_times(g, windows))
        print(f"G = {g}: measured", file=sys.stderr, flush=True)  # (the largest stage takes minutes)
    print(json.dumps({"windows": windows, "stages": stages}))
    if "--markdown" in ARGV:
        path = ARGV[ARGV.index("--markdown") + 1]
        text = open(path).read()
        start, end = text.index(BEGIN), text.index(END) + len(END)
        open(path, "w").write(text[:start] + markdown(stages) + text[end:])


if __name__ == "__main__":
    main()
