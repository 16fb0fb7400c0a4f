"""Development benchmark of the evaluation (include/reinfocus_hip.h, "evaluation"): one DeviceEvaluation.run() at the
reference's shape -- m = 8 lanes and E = 5 episodes per group (n_envs: 8, --n-eval-envs 8, n_eval_episodes 5), episodes of
at most 20 steps, so max_steps = ceil(5 / 8) * 20 = 20 -- for G = 1, 16, 64, 512 groups of a DevicePopulationPolicy at
ppo_tuned.yml's network (pi = vf = [256, 256]) over DiscreteSteps with the configuration's learner view (normalize: true,
frame_stack: 5; one set of moments per group):
  (a) evaluation.run(20): statistics, reset, 20 x (act, step_tensors, rf_eval_accumulate), rf_eval_finish, two
      rf_eval_keep_rows -- and one synchronisation at the end of the window;
  (b) the only form the library allowed before: the same loop with set_view_statistics(view_statistics()) through the host,
      step() on host arrays, a host read of info["episode_return"] / ["episode_length"] per step into the numpy twin's
      tables, and the twin's finish.
The frames are 16 x 16 pixels with one sample unless --frame-height / --samples say otherwise: the render is the same work
in both forms, and at the reference's 300 x 300 x 100 it would hide everything else.  Alternating windows in one process,
medians and the windows' spread.  No ratio is promised: both sides are recorded.  One JSON line; --markdown FILE also
rewrites the measured section of that file (profiles/evaluation.md), between its two marker lines.
usage (GPU box):  python tools/bench_evaluation.py [--windows 5] [--groups 1,16,64,512] [--markdown profiles/evaluation.md]"""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(HERE)
ARGV = list(sys.argv[1:])
from reinfocus_amd.environments import evaluation  # noqa: E402
from reinfocus_amd.environments import harness  # noqa: E402

PER_GROUP, EPISODES, EPISODE_STEPS, STACK = 8, 5, 20, 5
MAX_STEPS = -(-EPISODES // PER_GROUP) * EPISODE_STEPS
BEGIN, END = "<!-- bench_evaluation: begin -->", "<!-- bench_evaluation: end -->"


def option(name, default, kind=int):
    return kind(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def windows_of(forms, windows):
    """Milliseconds per call: `windows` alternating windows per form, each `calls` calls of it and one synchronisation."""
    for form, _ in forms.values():  # warm-up
        form()
    times = {name: [] for name in forms}
    for _ in range(windows):
        for name, (form, calls) in forms.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(calls):
                form()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - start) / calls)
    return {name: {"median_ms": float(np.median(t)), "spread": float((max(t) - min(t)) / np.median(t)),
                   "windows_ms": [round(x, 3) for x in t]} for name, t in times.items()}


def stage_times(groups, windows, frame_height, samples):
    n = groups * PER_GROUP

    def env(training, seed):
        return harness.DeviceVectorDiscreteSteps(
            max_episode_steps=EPISODE_STEPS, num_envs=n, frame_height=frame_height, samples_per_pixel=samples, seed=seed,
            device=0, device_initializer=True, episode_records=True,
            learner_view=harness.LearnerView(frame_stack=STACK, groups=groups, training=training))

    train_env, eval_env = env(True, 0), env(False, 1)
    try:
        spec = harness.MlpPolicySpec(int(train_env.single_observation_space.shape[0]), int(train_env.single_action_space.n),
                                     pi=(256, 256), vf=(256, 256))
        policy = harness.DevicePopulationPolicy(train_env, spec, groups, list(range(groups)))
        policy.init_parameters(list(range(100, 100 + groups)), False)
        train_env.reset_tensors()
        measured = harness.DeviceEvaluation(eval_env, policy, n_eval_episodes=EPISODES, train_env=train_env)
        best_mean, best_serial = np.full(groups, -np.inf), np.zeros(groups, dtype=np.int64)
        actions = torch.zeros(n, dtype=torch.int64, device="cuda")
        rows = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(2)]

        def host_form():
            eval_env.set_view_statistics(train_env.view_statistics())
            obs, _ = eval_env.reset()
            counts, returns, lengths = evaluation.tables(n, PER_GROUP, EPISODES)
            for _ in range(MAX_STEPS):
                policy.act(torch.from_numpy(obs).cuda(), None, True, out=(actions, rows[0], rows[1], None))
                obs, _, _, _, info = eval_env.step(actions.cpu().numpy())
                evaluation.accumulate_numpy(counts, returns, lengths, info["episode_return"], info["episode_length"],
                                            PER_GROUP, EPISODES)
            return evaluation.finish_numpy(counts, returns, lengths, groups, PER_GROUP, EPISODES, 1, best_mean, best_serial)

        out = {"groups": groups, "lanes": n, "max_steps": MAX_STEPS}
        out.update(windows_of({"device": (lambda: measured.run(MAX_STEPS), 3), "host": (host_form, 2)}, windows))
        out["complete"] = int((measured.results()[:, evaluation.FLAGS] == 0).sum())
        return out
    finally:
        train_env.close()
        eval_env.close()


def markdown(stages):
    lines = [BEGIN, "", "| G | lanes | run() on the device (ms) | spread | host loop (ms) | spread | host / device |",
             "|---|---|---|---|---|---|---|"]
    for r in stages:
        a, b = r["device"], r["host"]
        lines.append(f"| {r['groups']} | {r['lanes']} | {a['median_ms']:.2f} | {100 * a['spread']:.0f} % | "
                     f"{b['median_ms']:.2f} | {100 * b['spread']:.0f} % | {b['median_ms'] / a['median_ms']:.1f} |")
    return "\n".join(lines + ["", END])


def main():
    windows = option("--windows", 5)
    groups = [int(g) for g in option("--groups", "1,16,64,512", str).split(",")]
    frame_height, samples = option("--frame-height", 16), option("--samples", 1)
    torch.zeros(1, device="cuda")
    stages = []
    for g in groups:
        stages.append(stage_times(g, windows, frame_height, samples))
        print(f"G = {g}: measured", file=sys.stderr, flush=True)
    print(json.dumps({"windows": windows, "frame_height": frame_height, "samples_per_pixel": samples, "stages": stages}))
    if "--markdown" in ARGV:
        path = ARGV[ARGV.index("--markdown") + 1]
        text = open(path).read()
        start, end = text.index(BEGIN), text.index(END) + len(END)
        open(path, "w").write(text[:start] + markdown(stages) + text[end:])


if __name__ == "__main__":
    main()
