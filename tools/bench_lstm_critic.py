"""Development benchmark of the recurrent policies' two critic modes (include/reinfocus_hip.h, "lstm critic"): act() and one
minibatch update with the LSTM critic (enable_critic_lstm=True: rf_lstm_forward / rf_lstm_ppo_update and their sde
siblings) and with the feed-forward critic (enable_critic_lstm=False: the rf_lstm_critic_* entry points), under both heads,
on the same parameters (where the modes share them), observations and sequences, at the two recurrent shapes:
ppo_lstm_tuned.yml's -- 8 environments, H = 16, T = 8, minibatches of 8 rows -- and sb3-contrib's defaults -- 8
environments, H = 256, T = 128, minibatches of 128.  Alternating windows in one process, each a run of calls ended by one
synchronisation; medians and the windows' spread.  One JSON line; --markdown FILE also rewrites the measured section of
that file (profiles/lstm_critic.md), between its two marker lines.
usage (GPU box):  python tools/bench_lstm_critic.py [--windows 7] [--markdown profiles/lstm_critic.md]
                  python tools/bench_lstm_critic.py --only-lstm [--root OTHER_CHECKOUT]
--only-lstm times the LSTM critic alone, through the classes' own path; with --root the package of another checkout (one from
before this mode existed, with its library built) is imported in place of this one: the same script, seeds and sequences
then time the parent commit, in a process of its own."""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGV = list(sys.argv[1:])
if "--root" in ARGV:
    sys.path.insert(0, os.path.abspath(ARGV[ARGV.index("--root") + 1]))
sys.path.append(HERE)
from reinfocus_amd.environments import harness, lstm_learner  # noqa: E402

ENVS, ACTIONS = 8, 13
NETS = {"tuned": dict(lstm_hidden=16, pi=(64, 64), vf=(64, 64), activation="relu"),
        "default": dict(lstm_hidden=256, pi=(64, 64), vf=(64, 64), activation="tanh")}
SHAPES = {"tuned": dict(steps=8, batch=8, calls=400,
                        hyper=dict(learning_rate=0.0010897458332287295, clip_range=0.3, ent_coef=0.018408120577291045,
                                   vf_coef=0.3281607546040628, max_grad_norm=0.3)),
          "default": dict(steps=128, batch=128, calls=40,
                          hyper=dict(learning_rate=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5))}
BEGIN, END = "<!-- bench_lstm_critic: begin -->", "<!-- bench_lstm_critic: end -->"


def option(name, default):
    return int(ARGV[ARGV.index(name) + 1]) if name in ARGV else default


def random_state(spec, seed):
    """Normal weights of scale 1 / sqrt(fan_in), biases of scale 0.1; every name is drawn from a generator of its own, so the
    two critic modes share every parameter they both have."""
    out = {}
    for name, _, shape, is_weight in spec.entries:
        rng = np.random.default_rng([seed] + list(name.encode()))
        value = rng.standard_normal(shape[::-1]) / np.sqrt(shape[0]) if is_weight else 0.1 * rng.standard_normal(shape)
        out[name] = torch.from_numpy(value.astype(np.float32)).cuda()
    if "log_std" in out:
        out["log_std"] = torch.full_like(out["log_std"], -0.5)
    return out


class Slabs:
    """What an update asks of a finished recurrent rollout, over random tensors: an episode start at one step in twenty."""

    def __init__(self, env, steps, width, hidden, gaussian, seed):
        rng = np.random.default_rng(seed)
        rows = steps * ENVS
        self.env, self.device, self.n_steps, self.num_envs = env, torch.device("cuda", 0), steps, ENVS
        normal = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()  # noqa: E731
        actions = 0.5 * normal(rows) if gaussian else torch.from_numpy(rng.integers(0, ACTIONS, rows)).cuda()
        self._flat = {"observations": normal(rows, width), "actions": actions, "values": normal(rows),
                      "log_probs": -2.5 + 0.1 * normal(rows), "advantages": normal(rows), "returns": normal(rows)}
        self.episode_starts = torch.from_numpy((rng.random((steps + 1, ENVS)) < 0.05).astype(np.uint8)).cuda()
        self.lstm_states = 0.5 * normal(steps + 1, 2, 2, ENVS, hidden)

    def flat(self):
        return self._flat


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


def make_pair(env, head, net, mode):
    extra = {} if mode == "lstm" else dict(enable_critic_lstm=False)  # (a checkout from before the mode has no keyword)
    width = int(env.single_observation_space.shape[0])
    if head == "sde":
        spec = harness.LstmSdePolicySpec(width, log_std_init=-0.5, **NETS[net], **extra)
        policy = harness.DeviceLstmSdePolicy(env, spec, 0)
    else:
        spec = harness.LstmPolicySpec(width, ACTIONS, **NETS[net], **extra)
        policy = harness.DeviceLstmPolicy(env, spec, 0)
    policy.load_state_dict(random_state(spec, 1))
    if head == "sde":
        policy.reset_noise()
    return spec, policy, harness.DeviceLstmLearner(policy, **SHAPES[net]["hyper"])


def measure(envs, head, net, modes, windows):
    env = envs[head]
    shape = SHAPES[net]
    pairs = {mode: make_pair(env, head, net, mode) for mode in modes}
    spec = pairs[modes[0]][0]
    slabs = Slabs(env, shape["steps"], spec.obs_width, spec.lstm_hidden, head == "sde", shape["steps"])
    parts = lstm_learner.parts_of(slabs)
    rows = shape["steps"] * ENVS
    first = rows // 3
    obs = slabs.flat()["observations"][:ENVS].contiguous()
    starts = torch.zeros(ENVS, dtype=torch.uint8, device="cuda")
    out = {"head": head, "net": net, "lstm_hidden": spec.lstm_hidden, "steps": shape["steps"], "batch": shape["batch"],
           "parameters": {mode: pairs[mode][0].size for mode in modes},
           "sequences_in_the_timed_minibatch": int(sum(row[3] for row in lstm_learner.sequence_rows(
               slabs.episode_starts.cpu().numpy(), shape["steps"], ENVS, first, shape["batch"])))}
    out["act"] = windows_of({mode: (lambda policy=pairs[mode][1]: policy.act(obs, starts)) for mode in modes}, windows,
                            shape["calls"])
    last = {}

    def update_of(mode):
        learner = pairs[mode][2]

        def update():
            last[mode] = learner.update(parts, first, shape["batch"])
        return update

    out["update"] = windows_of({mode: update_of(mode) for mode in modes}, windows, max(shape["calls"] // 4, 5))
    out["update_flags"] = {mode: float(last[mode].cpu().numpy()[7]) for mode in modes}
    out["workspace_bytes"] = {mode: 4 * pairs[mode][2]._workspace.numel() for mode in modes}
    return out


def markdown(results):
    lines = [BEGIN, "", "| head | shape | call | LSTM critic (us) | spread | feed-forward critic (us) | spread | ratio |",
             "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for call in ("act", "update"):
            a, b = r[call]["lstm"], r[call]["linear"]
            lines.append(f"| {r['head']} | {r['net']} (H = {r['lstm_hidden']}, T = {r['steps']}, B = {r['batch']}) | {call} | "
                         f"{a['median_us']:.1f} | {100 * a['spread']:.0f} % | {b['median_us']:.1f} | {100 * b['spread']:.0f} % | "
                         f"{b['median_us'] / a['median_us']:.2f} |")
    lines += ["", "Parameters and workspace bytes at the timed batch (LSTM critic / feed-forward critic):", ""]
    for r in results:
        lines.append(f"- {r['head']}, {r['net']}: {r['parameters']['lstm']} / {r['parameters']['linear']} floats; "
                     f"{r['workspace_bytes']['lstm']} / {r['workspace_bytes']['linear']} bytes; "
                     f"{r['sequences_in_the_timed_minibatch']} sequences in the timed minibatch; "
                     f"flags {r['update_flags']['lstm']:.0f} / {r['update_flags']['linear']:.0f}")
    return "\n".join(lines + ["", END])


def main():
    windows = option("--windows", 7)
    modes = ["lstm"] if "--only-lstm" in ARGV else ["lstm", "linear"]
    torch.zeros(1, device="cuda")
    kw = dict(num_envs=ENVS, frame_height=16, samples_per_pixel=1, seed=0, device=0, device_initializer=True)
    envs = {"categorical": harness.DeviceVectorDiscreteSteps(**kw), "sde": harness.DeviceVectorContinuousJumps(**kw)}
    results = [measure(envs, head, net, modes, windows) for head in envs for net in SHAPES]
    for env in envs.values():
        env.close()
    print(json.dumps({"windows": windows, "modes": modes, "results": results}))
    if "--markdown" in ARGV:
        path = ARGV[ARGV.index("--markdown") + 1]
        text = open(path).read()
        start, end = text.index(BEGIN), text.index(END) + len(END)
        open(path, "w").write(text[:start] + markdown(results) + text[end:])


if __name__ == "__main__":
    main()
