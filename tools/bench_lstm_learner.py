"""Development benchmark of the recurrent PPO update (rf_lstm_ppo_update: DeviceLstmLearner.update / train over a
DeviceLstmPolicy) at ppo_lstm_tuned.yml's shape -- 8 environments x 8 steps, minibatches of 8 rows, 5 epochs, H = 16, [64, 64]
ReLU -- and at sb3-contrib's defaults, which ppo_lstm_untuned.yml runs -- 8 x 128 steps, minibatches of 128, 10 epochs,
H = 256, [64, 64] tanh -- against the same arithmetic in eager torch on the same device tensors in the same process:
sb3-contrib's way through a minibatch that holds episode starts (the sequences padded side by side, nn.LSTM x 2 stepped
one timestep at a time over the sequences still running, from the stored states, zeroed at a start), the MLPs,
stable-baselines3's loss, backward, clip_grad_norm_ and torch.optim.Adam(eps=1e-5).  The torch form reads the episode
starts on the host, as sb3-contrib's numpy buffer does.  Alternating windows, each ended by one synchronisation; medians
and the windows' spread.  One JSON line.
usage (GPU box):  python tools/bench_lstm_learner.py [--windows 5] [--no-iteration]
Measured per shape: one update, one train() of the configuration's epochs, one full iteration (DeviceRollout.collect with
the device policy at 8 x 300 x 300 px x 100 samples -- the same in both forms -- then train() by either form)."""
import json
import os
import sys

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness, lstm_learner  # noqa: E402
from tools.bench_learner import summary, windows_of  # noqa: E402
from tools.bench_lstm import ACTIONS, NETS, TorchLstm  # noqa: E402
from tools.bench_policy import option, random_state  # noqa: E402

ENVS = 8
SHAPES = {"tuned": dict(steps=8, batch=8, epochs=5, gamma=0.98, gae_lambda=0.98,
                        hyper=dict(learning_rate=0.0010897458332287295, clip_range=0.3, ent_coef=0.018408120577291045,
                                   vf_coef=0.3281607546040628, max_grad_norm=0.3)),
          "untuned": dict(steps=128, batch=128, epochs=10, gamma=0.99, gae_lambda=0.95,
                          hyper=dict(learning_rate=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5))}


class TorchLstmLearner:
    """RecurrentPPO.train()'s body in eager torch, without its per-minibatch logging."""

    def __init__(self, eager, hyper):
        self.eager, self.hyper = eager, hyper
        self.nets = ((eager.lstm["lstm_actor"], eager.nets.pi), (eager.lstm["lstm_critic"], eager.nets.vf))
        self.parameters = [p for lstm, mlp in self.nets for p in list(lstm.parameters()) + list(mlp.parameters())]
        self.optimizer = torch.optim.Adam(self.parameters, lr=hyper["learning_rate"], eps=1e-5)

    def update(self, parts, starts_host, first, count):
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
        for net, (lstm, mlp) in enumerate(self.nets):
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
        clip = self.hyper["clip_range"]
        distribution = torch.distributions.Categorical(logits=heads[0])
        ratio = torch.exp(distribution.log_prob(actions) - old)
        policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
        value_loss = torch.nn.functional.mse_loss(returns, heads[1].flatten())
        loss = policy_loss + self.hyper["ent_coef"] * -distribution.entropy().mean() + self.hyper["vf_coef"] * value_loss
        self.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.parameters, self.hyper["max_grad_norm"])
        self.optimizer.step()

    def train(self, rollout, n_epochs, batch_size, generator):
        parts = lstm_learner.parts_of(rollout)
        starts_host = parts["episode_starts"].cpu().numpy()  # (sb3-contrib's buffer lives on the host)
        total = parts["n_steps"] * parts["num_envs"]
        for _ in range(n_epochs):
            split = int(generator.integers(total))
            for i in range(-(-total // batch_size)):
                self.update(parts, starts_host, (split + i * batch_size) % total, min(batch_size, total - i * batch_size))


class Slabs:
    """What train() asks of a finished recurrent rollout, over random tensors: an episode start at one step in twenty."""

    def __init__(self, env, steps, envs, width, hidden, seed):
        rng = np.random.default_rng(seed)
        rows = steps * envs
        self.env, self.device, self.n_steps, self.num_envs = env, torch.device("cuda", 0), steps, envs
        normal = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()  # noqa: E731
        self._flat = {"observations": normal(rows, width), "actions": torch.from_numpy(rng.integers(0, ACTIONS, rows)).cuda(),
                      "values": normal(rows), "log_probs": -2.5 + 0.1 * normal(rows), "advantages": normal(rows),
                      "returns": normal(rows)}
        self.episode_starts = torch.from_numpy((rng.random((steps + 1, envs)) < 0.05).astype(np.uint8)).cuda()
        self.lstm_states = 0.5 * normal(steps + 1, 2, 2, envs, hidden)

    def flat(self):
        return self._flat


def pair(env, name):
    spec = harness.LstmPolicySpec(int(env.single_observation_space.shape[0]), ACTIONS, **NETS[name])
    state = random_state(spec, 1)
    policy = harness.DeviceLstmPolicy(env, spec, 0)
    policy.load_state_dict(state)
    hyper = SHAPES[name]["hyper"]
    return spec, policy, harness.DeviceLstmLearner(policy, **hyper), TorchLstmLearner(TorchLstm(spec, state, env.num_envs),
                                                                                      hyper)


def stage_times(env, name, windows):
    shape = SHAPES[name]
    steps, batch, epochs = shape["steps"], shape["batch"], shape["epochs"]
    spec, policy, learner, theirs = pair(env, name)
    slabs = Slabs(env, steps, ENVS, spec.obs_width, spec.lstm_hidden, steps)
    parts = lstm_learner.parts_of(slabs)
    starts_host = slabs.episode_starts.cpu().numpy()
    rows = steps * ENVS
    first = rows // 3
    sequences = int(sum(row[3] for row in lstm_learner.sequence_rows(starts_host, steps, ENVS, first, batch)))
    out = {"net": name, "rows": rows, "batch": batch, "epochs": epochs, "lstm_hidden": spec.lstm_hidden,
           "sequences_in_the_timed_minibatch": sequences}
    last = {}

    def one_by_kernel():
        last["stats"] = learner.update(parts, first, batch)

    out["update"] = summary(windows_of({"kernel": one_by_kernel,
                                        "torch": lambda: theirs.update(parts, starts_host, first, batch)}, windows), 1)
    out["update"]["unit"] = "us per update"
    out["update"]["flags"] = float(last["stats"].cpu().numpy()[7])
    updates = epochs * -(-rows // batch)
    seeds = {"kernel": np.random.default_rng(5), "torch": np.random.default_rng(5)}

    def by_kernel():
        last["stats"] = learner.train(slabs, epochs, batch, generator=seeds["kernel"])

    out["train"] = summary(windows_of({"kernel": by_kernel,
                                       "torch": lambda: theirs.train(slabs, epochs, batch, seeds["torch"])}, windows), 1)
    stats = last["stats"].cpu().numpy()
    out["train"].update(unit="us per train()", updates_per_train=updates, skipped_updates=int((stats[:, 7] != 0).sum()),
                        last_loss=float(stats[-1, 6]))
    return out


def iteration_times(name, windows):
    """Microseconds per iteration: DeviceRollout.collect(DeviceLstmPolicy) at 8 x 300 x 300 x 100 (records and the learner
    view on; the same in both forms), then train() by the device learner or by the torch form."""
    shape = SHAPES[name]
    steps, batch, epochs = shape["steps"], shape["batch"], shape["epochs"]
    env = harness.DeviceVectorDiscreteSteps(max_episode_steps=20, num_envs=ENVS, frame_height=300, samples_per_pixel=100,
                                            seed=0, device=0, device_initializer=True, episode_records=True,
                                            learner_view=harness.LearnerView(frame_stack=1))
    spec, policy, learner, theirs = pair(env, name)
    buffer = harness.DeviceRollout(env, steps, shape["gamma"], shape["gae_lambda"])
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
        theirs.train(buffer, epochs, batch, seeds["torch"])

    times = windows_of({"kernel": by_kernel, "torch": by_torch, "collect": collect_only}, windows)
    fault = env.device_fault()
    env.close()
    medians = {form: float(np.median(t)) for form, t in times.items()}
    return {"net": name, "steps": steps, "envs": ENVS, "frame": 300, "spp": 100, "updates": epochs * -(-steps * ENVS // batch),
            "us_per_iteration": medians, "windows_us": {form: [round(x) for x in t] for form, t in times.items()},
            "spread": {form: float((max(t) - min(t)) / np.median(t)) for form, t in times.items()}, "device_fault": fault}


def main():
    argv = list(sys.argv[1:])
    windows = option(argv, "--windows", 5)
    torch.zeros(1, device="cuda")
    env = harness.DeviceVectorDiscreteSteps(num_envs=ENVS, frame_height=16, samples_per_pixel=1, seed=0, device=0,
                                            device_initializer=True)
    out = {"windows": windows, "stages": [stage_times(env, name, windows) for name in SHAPES]}
    env.close()
    if "--no-iteration" not in argv:
        out["iteration"] = [iteration_times(name, windows) for name in SHAPES]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
