"""Development benchmark of the recurrent sde policy (rf_lstm_sde_forward, rf_lstm_sde_update: DeviceLstmSdePolicy.act,
DeviceLstmLearner.update / train over it) at ppo_lstm_untuned.yml's shape for ContinuousJumps-v0 -- 8 environments, H = 256,
[64, 64] tanh, sb3-contrib's default n_steps = 128 and minibatches of 128 rows, 10 epochs -- against the same arithmetic in
eager torch on the same device tensors in the same process: nn.LSTM x 2 with their states masked by (1 - start), the MLPs,
Normal(mu, sqrt((h * h) @ exp(log_std) ** 2 + 1e-6)) with the exploration matrix applied as sb3 does, and for the update
tools/bench_lstm_learner.py's way through a minibatch that holds episode starts, stable-baselines3's loss, backward,
clip_grad_norm_ and torch.optim.Adam(eps=1e-5).  Next to them the Categorical kernels (DeviceLstmPolicy.act,
rf_lstm_ppo_update) at equal H, B and MLPs: the heads differ by O(B L) work against O(B H^2).  Alternating windows, each
ended by one synchronisation; medians and the windows' spread.  One JSON line.
usage (GPU box):  python tools/bench_lstm_sde.py [--windows 5] [--calls 200] [--no-iteration]"""
import json
import os
import sys
import types

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness, lstm_learner  # noqa: E402
from tools import bench_policy  # noqa: E402
from tools.bench_learner import summary, windows_of  # noqa: E402
from tools.bench_lstm import ACTIONS, NETS, TorchLstm  # noqa: E402
from tools.bench_lstm_learner import SHAPES  # noqa: E402
from tools.bench_policy import option, random_state  # noqa: E402

ENVS, NET = 8, "untuned"
SHAPE = SHAPES[NET]
LOG_STD_INIT = -0.5


class _OneAction:  # (what TorchLstm reads of a spec: a pi head of one output)
    def __init__(self, spec):
        self.obs_width, self.lstm_hidden, self.pi, self.vf = spec.obs_width, spec.lstm_hidden, spec.pi, spec.vf
        self.activation, self.n_actions = spec.activation, 1


class TorchLstmSde(TorchLstm):
    """The eager-torch form of one forward of sb3-contrib's MlpLstmPolicy with use_sde."""

    def __init__(self, spec, state, n):
        super().__init__(_OneAction(spec), state, n)
        self.log_std = torch.nn.Parameter(state["log_std"].clone())
        self.hidden_pi, self.head_pi = self.nets.pi[:-1], self.nets.pi[-1]
        self.reset_noise(n)

    @torch.no_grad()
    def reset_noise(self, n):
        std = torch.exp(self.log_std)  # [L, 1]
        self.theta = torch.distributions.Normal(torch.zeros_like(std), std).rsample((n,))[:, :, 0]  # [n, L]

    def distribution(self, latent):
        variance = torch.mm(latent.detach() ** 2, torch.exp(self.log_std) ** 2)
        return torch.distributions.Normal(self.head_pi(latent), torch.sqrt(variance + 1e-6))

    @torch.no_grad()
    def act(self, obs, starts, final_obs=None):
        keep = (1.0 - starts.float()).view(1, -1, 1)
        final_values = None
        if final_obs is not None:
            final_values = self.nets.vf(self.lstm["lstm_critic"](final_obs[None], self.vf_state)[0][0])[:, 0]
        latent_pi, self.pi_state = self.lstm["lstm_actor"](obs[None], (self.pi_state[0] * keep, self.pi_state[1] * keep))
        latent_vf, self.vf_state = self.lstm["lstm_critic"](obs[None], (self.vf_state[0] * keep, self.vf_state[1] * keep))
        latent = self.hidden_pi(latent_pi[0])
        distribution = self.distribution(latent)
        actions = distribution.mean + (latent * self.theta).sum(dim=1, keepdim=True)
        return (actions[:, 0], self.nets.vf(latent_vf[0])[:, 0], distribution.log_prob(actions)[:, 0], final_values,
                torch.clamp(actions[:, 0], -1.0, 1.0))


def gaussian_update(theirs, parts, starts_host, first, count):
    """tools/bench_lstm_learner.py's TorchLstmLearner.update with the Gaussian head: the same sequence walk, then the loss
    of the state-dependent Normal on the latent the pi MLP returned."""
    eager, hyper = theirs.eager, theirs.hyper
    steps, envs = parts["n_steps"], parts["num_envs"]
    rows = (first + np.arange(count)) % (steps * envs)
    e, t = rows // steps, rows % steps
    flagged = starts_host[t, e] != 0
    is_start = flagged | (t == 0)
    is_start[0] = True
    begins = np.flatnonzero(is_start)
    lengths = np.diff(np.append(begins, count))
    order = np.argsort(-lengths, kind="stable")  # (the sequences still running at a timestep are a prefix)
    begins, lengths = begins[order], lengths[order]
    running = [int((lengths > s).sum()) for s in range(int(lengths.max()))]
    position = np.concatenate([begins[:k] + s for s, k in enumerate(running)])
    to_device = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rows_d, position_d, back = to_device(rows), to_device(position), to_device(np.argsort(position))
    at_t, at_e, zero = to_device(t[begins]), to_device(e[begins]), to_device(flagged[begins])
    obs = parts["observations"][rows_d]
    heads = []
    for net, (lstm, mlp) in enumerate(theirs.nets):
        stored = parts["lstm_states"]
        h = torch.where(zero[:, None], 0.0, stored[at_t, net, 0, at_e])[None]
        c = torch.where(zero[:, None], 0.0, stored[at_t, net, 1, at_e])[None]
        pieces, offset = [], 0
        for k in running:
            y, (h, c) = lstm(obs[position_d[offset:offset + k]][None], (h[:, :k].contiguous(), c[:, :k].contiguous()))
            pieces.append(y[0])
            offset += k
        heads.append(mlp(torch.cat(pieces)[back]))
    actions, old = parts["actions"][rows_d], parts["log_probs"][rows_d]
    advantages, returns = parts["advantages"][rows_d], parts["returns"][rows_d]
    if count > 1:
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    clip = hyper["clip_range"]
    distribution = eager.distribution(heads[0])
    ratio = torch.exp(distribution.log_prob(actions[:, None])[:, 0] - old)
    policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    value_loss = torch.nn.functional.mse_loss(returns, heads[1].flatten())
    loss = policy_loss + hyper["ent_coef"] * -distribution.entropy().mean() + hyper["vf_coef"] * value_loss
    theirs.optimizer.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(theirs.parameters, hyper["max_grad_norm"])
    theirs.optimizer.step()


def gaussian_train(theirs, rollout, n_epochs, batch_size, generator):
    parts = lstm_learner.parts_of(rollout)
    starts_host = parts["episode_starts"].cpu().numpy()  # (sb3-contrib's buffer lives on the host)
    total = parts["n_steps"] * parts["num_envs"]
    for _ in range(n_epochs):
        split = int(generator.integers(total))
        for i in range(-(-total // batch_size)):
            gaussian_update(theirs, parts, starts_host, (split + i * batch_size) % total, min(batch_size, total - i * batch_size))


class Slabs:
    """What train() asks of a finished recurrent rollout, over random tensors: an episode start at one step in twenty.
    gaussian: float32 raw actions (normal values) in place of int64 ones; everything else -- the episode starts, and so
    the sequences of every minibatch, first of all -- is the same for one seed."""

    def __init__(self, env, steps, envs, width, hidden, seed, gaussian):
        rng = np.random.default_rng(seed)
        rows = steps * envs
        self.env, self.device, self.n_steps, self.num_envs = env, torch.device("cuda", 0), steps, envs
        normal = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()  # noqa: E731
        self.episode_starts = torch.from_numpy((rng.random((steps + 1, envs)) < 0.05).astype(np.uint8)).cuda()
        self.lstm_states = 0.5 * normal(steps + 1, 2, 2, envs, hidden)
        actions = 0.5 * normal(rows) if gaussian else torch.from_numpy(rng.integers(0, ACTIONS, rows)).cuda()
        self._flat = {"observations": normal(rows, width), "actions": actions, "values": normal(rows),
                      "log_probs": (-1.0 if gaussian else -2.5) + 0.1 * normal(rows), "advantages": normal(rows),
                      "returns": normal(rows)}

    def flat(self):
        return self._flat


def sde_pair(env):
    spec = harness.LstmSdePolicySpec(int(env.single_observation_space.shape[0]), log_std_init=LOG_STD_INIT, **NETS[NET])
    state = random_state(spec, 1)
    state["log_std"] = torch.full((spec.latent, 1), LOG_STD_INIT, device="cuda")
    policy = harness.DeviceLstmSdePolicy(env, spec, 0)
    policy.load_state_dict(state)
    eager = TorchLstmSde(spec, state, env.num_envs)
    theirs = types.SimpleNamespace(eager=eager, hyper=SHAPE["hyper"])
    theirs.nets = ((eager.lstm["lstm_actor"], eager.hidden_pi), (eager.lstm["lstm_critic"], eager.nets.vf))
    theirs.parameters = [p for lstm, mlp in theirs.nets for p in list(lstm.parameters()) + list(mlp.parameters())] \
        + list(eager.head_pi.parameters()) + [eager.log_std]
    theirs.optimizer = torch.optim.Adam(theirs.parameters, lr=SHAPE["hyper"]["learning_rate"], eps=1e-5)
    return spec, policy, harness.DeviceLstmLearner(policy, **SHAPE["hyper"]), eager, theirs


def categorical_pair(env):
    spec = harness.LstmPolicySpec(int(env.single_observation_space.shape[0]), ACTIONS, **NETS[NET])
    policy = harness.DeviceLstmPolicy(env, spec, 0)
    policy.load_state_dict(random_state(spec, 1))
    return spec, policy, harness.DeviceLstmLearner(policy, **SHAPE["hyper"])


def act_times(jumps, steps_env, windows, calls):
    spec, policy, _, eager, _ = sde_pair(jumps)
    other_spec, categorical, _ = categorical_pair(steps_env)
    assert other_spec.obs_width == spec.obs_width  # (both tasks observe the same four numbers)
    rng = np.random.default_rng(ENVS)
    obs = torch.from_numpy(rng.standard_normal((ENVS, spec.obs_width)).astype(np.float32)).cuda()
    final_obs = torch.from_numpy(rng.standard_normal((ENVS, spec.obs_width)).astype(np.float32)).cuda()
    final_obs[::2] = float("nan")
    starts = torch.zeros(ENVS, dtype=torch.uint8, device="cuda")
    starts[3] = 1
    policy.reset_noise()
    # the two forms compute the same network: values agree to float32 rounding (not bit for bit: torch's order is its own)
    agree = float((policy.values(obs, starts) - eager.values(obs, starts)).abs().max())
    out = bench_policy.windows_of({"kernel": lambda: policy.act(obs, starts, final_obs),
                                   "torch": lambda: eager.act(obs, starts, final_obs),
                                   "categorical_kernel": lambda: categorical.act(obs, starts, final_obs),
                                   "noise_reset_kernel": policy.reset_noise,
                                   "noise_reset_torch": lambda: eager.reset_noise(ENVS)}, windows, calls)
    out.update(net=NET, envs=ENVS, largest_value_difference=agree,
               torch_over_kernel=out["median_us"]["torch"] / out["median_us"]["kernel"],
               gaussian_over_categorical=out["median_us"]["kernel"] / out["median_us"]["categorical_kernel"])
    return out


def stage_times(jumps, steps_env, windows):
    steps, batch, epochs = SHAPE["steps"], SHAPE["batch"], SHAPE["epochs"]
    spec, policy, learner, eager, theirs = sde_pair(jumps)
    other_spec, _, categorical = categorical_pair(steps_env)
    slabs = Slabs(jumps, steps, ENVS, spec.obs_width, spec.lstm_hidden, steps, True)
    other = Slabs(steps_env, steps, ENVS, other_spec.obs_width, spec.lstm_hidden, steps, False)
    assert torch.equal(slabs.episode_starts, other.episode_starts)  # (the same sequences in both heads' minibatches)
    parts, other_parts = lstm_learner.parts_of(slabs), lstm_learner.parts_of(other)
    starts_host = slabs.episode_starts.cpu().numpy()
    rows = steps * ENVS
    first = rows // 3
    sequences = int(sum(row[3] for row in lstm_learner.sequence_rows(starts_host, steps, ENVS, first, batch)))
    out = {"net": NET, "rows": rows, "batch": batch, "epochs": epochs, "lstm_hidden": spec.lstm_hidden,
           "sequences_in_the_timed_minibatch": sequences}
    last = {}

    def one_by_kernel():
        last["stats"] = learner.update(parts, first, batch)

    def one_categorical():
        last["categorical"] = categorical.update(other_parts, first, batch)

    out["update"] = summary(windows_of({"kernel": one_by_kernel,
                                        "torch": lambda: gaussian_update(theirs, parts, starts_host, first, batch),
                                        "categorical_kernel": one_categorical}, windows), 1)
    out["update"]["unit"] = "us per update"
    out["update"]["flags"] = [float(last["stats"].cpu().numpy()[7]), float(last["categorical"].cpu().numpy()[7])]
    medians = out["update"]["median_us"]
    out["update"]["gaussian_over_categorical"] = medians["kernel"] / medians["categorical_kernel"]
    updates = epochs * -(-rows // batch)
    seeds = {name: np.random.default_rng(5) for name in ("kernel", "torch", "categorical")}

    def by_kernel():
        last["stats"] = learner.train(slabs, epochs, batch, generator=seeds["kernel"])

    out["train"] = summary(windows_of({"kernel": by_kernel,
                                       "torch": lambda: gaussian_train(theirs, slabs, epochs, batch, seeds["torch"]),
                                       "categorical_kernel": lambda: categorical.train(other, epochs, batch,
                                                                                       generator=seeds["categorical"])},
                                      windows), 1)
    stats = last["stats"].cpu().numpy()
    out["train"].update(unit="us per train()", updates_per_train=updates, skipped_updates=int((stats[:, 7] != 0).sum()),
                        last_loss=float(stats[-1, 6]))
    return out


def iteration_times(windows):
    """Microseconds per iteration: DeviceRollout.collect(DeviceLstmSdePolicy, sde_sample_freq=-1) over ContinuousJumps at
    8 x 300 x 300 px x 100 samples (records and the learner view on; the same in both forms), then train() by the device
    learner or by the torch form."""
    steps, batch, epochs = SHAPE["steps"], SHAPE["batch"], SHAPE["epochs"]
    env = harness.DeviceVectorContinuousJumps(max_episode_steps=20, num_envs=ENVS, frame_height=300, samples_per_pixel=100,
                                              seed=0, device=0, device_initializer=True, episode_records=True,
                                              learner_view=harness.LearnerView(frame_stack=1))
    spec, policy, learner, eager, theirs = sde_pair(env)
    buffer = harness.DeviceRollout(env, steps, SHAPE["gamma"], SHAPE["gae_lambda"])
    buffer.start(env.reset_tensors()[0])
    buffer.collect(policy)
    seeds = {"kernel": np.random.default_rng(5), "torch": np.random.default_rng(5)}

    def collect_only():
        buffer.start()
        buffer.collect(policy)

    def by_kernel():
        collect_only()
        learner.train(buffer, epochs, batch, generator=seeds["kernel"])

    def by_torch():
        collect_only()
        gaussian_train(theirs, buffer, epochs, batch, seeds["torch"])

    times = windows_of({"kernel": by_kernel, "torch": by_torch, "collect": collect_only}, windows)
    fault = env.device_fault()
    env.close()
    medians = {form: float(np.median(t)) for form, t in times.items()}
    return {"net": NET, "steps": steps, "envs": ENVS, "frame": 300, "spp": 100, "updates": epochs * -(-steps * ENVS // batch),
            "us_per_iteration": medians, "windows_us": {form: [round(x) for x in t] for form, t in times.items()},
            "spread": {form: float((max(t) - min(t)) / np.median(t)) for form, t in times.items()}, "device_fault": fault}


def main():
    argv = list(sys.argv[1:])
    windows, calls = option(argv, "--windows", 5), option(argv, "--calls", 200)
    torch.zeros(1, device="cuda")
    small = dict(num_envs=ENVS, frame_height=16, samples_per_pixel=1, seed=0, device=0, device_initializer=True)
    jumps, steps_env = harness.DeviceVectorContinuousJumps(**small), harness.DeviceVectorDiscreteSteps(**small)
    out = {"windows": windows, "calls": calls, "act": act_times(jumps, steps_env, windows, calls),
           "stages": stage_times(jumps, steps_env, windows)}
    jumps.close()
    steps_env.close()
    if "--no-iteration" not in argv:
        out["iteration"] = iteration_times(windows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
