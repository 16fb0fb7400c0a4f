"""Development benchmark of the learner stage (rf_ppo_update, DeviceLearner.train): the PPO minibatch updates of a rollout
as three launches each against stable-baselines3's train() restated in eager torch -- two nn.Sequential nets,
Categorical, the clipped surrogate / value / entropy loss, backward, clip_grad_norm_, torch.optim.Adam(eps=1e-5) -- on the
same device tensors in the same process.  Alternating windows, each ended by one synchronisation; medians and the
windows' spread.  Then a whole iteration (collect + train) with either learner.  One JSON line.
usage (GPU box):  python tools/bench_learner.py [--windows 7] [--no-iteration]
The torch form leaves out what SB3 logs per minibatch (approx_kl, clip_fraction: each a host read), so it waits for the
host as little as the kernel form does.  Shapes (profiles/learner.md): (a) ppo_tuned.yml's N = 256, B = 64, 20 epochs,
[256, 256] ReLU; (b) N = 16384, B = 64, 1 epoch, [64, 64] tanh; (c) N = 4096, B = 512, 1 epoch, [64, 64] tanh; all with
D = 20, A = 13.  The iteration: 8 environments x 300 x 300 px x 100 samples, 32 steps, then shape (a)'s updates."""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness  # noqa: E402
from tools.bench_policy import ACTIONS, GAE_LAMBDA, GAMMA, STACK, TorchPolicy, option, random_state  # noqa: E402

SHAPES = (("a", 256, 64, 20, (256, 256), "relu"), ("b", 16384, 64, 1, (64, 64), "tanh"), ("c", 4096, 512, 1, (64, 64), "tanh"))
HYPER = dict(learning_rate=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)


class TorchLearner:
    """PPO.train() of stable-baselines3 in eager torch, without its per-minibatch logging."""

    def __init__(self, eager):
        self.eager = eager
        self.parameters = list(eager.pi.parameters()) + list(eager.vf.parameters())
        self.optimizer = torch.optim.Adam(self.parameters, lr=HYPER["learning_rate"], eps=1e-5)

    def train(self, flat, n_epochs, batch_size):
        total = flat["actions"].shape[0]
        clip = HYPER["clip_range"]
        for _ in range(n_epochs):
            order = torch.randperm(total, device="cuda")
            for first in range(0, total, batch_size):
                index = order[first:first + batch_size]
                obs, actions = flat["observations"][index], flat["actions"][index]
                advantages, returns, old = flat["advantages"][index], flat["returns"][index], flat["log_probs"][index]
                if len(advantages) > 1:
                    advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
                distribution = torch.distributions.Categorical(logits=self.eager.pi(obs))
                ratio = torch.exp(distribution.log_prob(actions) - old)
                policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
                value_loss = torch.nn.functional.mse_loss(returns, self.eager.vf(obs).flatten())
                loss = policy_loss + HYPER["ent_coef"] * -distribution.entropy().mean() + HYPER["vf_coef"] * value_loss
                self.optimizer.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(self.parameters, HYPER["max_grad_norm"])
                self.optimizer.step()

    def state_dict(self, spec):
        """The parameters under stable-baselines3's names: what DevicePolicy.load_state_dict takes after the update."""
        out = {}
        for model, extractor, head_name, widths in ((self.eager.pi, "policy_net", "action_net", spec.pi),
                                                    (self.eager.vf, "value_net", "value_net", spec.vf)):
            keys = [f"mlp_extractor.{extractor}.{2 * i}" for i in range(len(widths))] + [head_name]
            for j, key in enumerate(keys):
                out[key + ".weight"], out[key + ".bias"] = model[2 * j].weight, model[2 * j].bias
        return out


class Slabs:
    """What train() asks of a finished rollout, over random tensors."""

    def __init__(self, env, rows, width, seed):
        rng = np.random.default_rng(seed)
        self.env, self.device = env, torch.device("cuda", 0)
        normal = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()  # noqa: E731
        self._flat = {"observations": normal(rows, width), "actions": torch.from_numpy(rng.integers(0, ACTIONS, rows)).cuda(),
                      "values": normal(rows), "log_probs": -2.5 + 0.1 * normal(rows), "advantages": normal(rows),
                      "returns": normal(rows)}

    def flat(self):
        return self._flat


def windows_of(forms, windows):
    for form in forms.values():  # warm-up
        form()
    times = {name: [] for name in forms}
    for _ in range(windows):
        for name, form in forms.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            form()
            torch.cuda.synchronize()  # (nothing was waited for: the window ends when the device has finished it)
            times[name].append(1e6 * (time.perf_counter() - start))
    return times


def summary(times, per):
    medians = {name: float(np.median(t)) / per for name, t in times.items()}
    return {"median_us": medians, "spread": {name: float((max(t) - min(t)) / np.median(t)) for name, t in times.items()},
            "windows_us": {name: [round(x / per, 2) for x in t] for name, t in times.items()},
            "torch_over_kernel": medians["torch"] / medians["kernel"]}


def pair(env, widths, activation):
    spec = harness.MlpPolicySpec(4 * STACK, ACTIONS, pi=widths, vf=widths, activation=activation)
    state = random_state(spec, 1)
    policy, eager = harness.DevicePolicy(env, spec, 0), TorchPolicy(spec, state)
    policy.load_state_dict(state)
    return spec, policy, harness.DeviceLearner(policy, **HYPER), eager, TorchLearner(eager)


def train_times(env, name, rows, batch, epochs, widths, activation, windows):
    spec, policy, learner, eager, theirs = pair(env, widths, activation)
    slabs = Slabs(env, rows, spec.obs_width, rows)
    updates = epochs * -(-rows // batch)
    last = {}

    def by_kernel():
        last["stats"] = learner.train(slabs, epochs, batch)

    out = summary(windows_of({"kernel": by_kernel, "torch": lambda: theirs.train(slabs.flat(), epochs, batch)}, windows),
                  updates)
    stats = last["stats"].cpu().numpy()
    out.update(shape=name, rows=rows, batch=batch, epochs=epochs, net=list(widths), activation=activation,
               updates_per_train=updates, unit="us per update", skipped_updates=int((stats[:, 7] != 0).sum()),
               last_loss=float(stats[-1, 6]))
    return out


def iteration_times(windows):
    """Microseconds per iteration: DeviceRollout.collect(DevicePolicy) of 32 steps at 8 x 300 x 300 x 100, then shape
    (a)'s 80 updates -- by DeviceLearner.train, in place; or by the torch learner followed by load_state_dict."""
    steps, n = 32, 8
    name, rows, batch, epochs, widths, activation = SHAPES[0]
    env = harness.DeviceVectorDiscreteSteps(max_episode_steps=20, num_envs=n, frame_height=300, samples_per_pixel=100,
                                            seed=0, device=0, device_initializer=True, episode_records=True,
                                            learner_view=harness.LearnerView(frame_stack=STACK))
    spec, policy, learner, eager, theirs = pair(env, widths, activation)
    buffer = harness.DeviceRollout(env, steps, GAMMA, GAE_LAMBDA)
    buffer.start(env.reset_tensors()[0])
    buffer.collect(policy)
    parts = {}

    def collect_only():
        buffer.start()
        buffer.collect(policy)

    def by_kernel():
        collect_only()
        learner.train(buffer, epochs, batch)

    def by_torch():
        collect_only()
        theirs.train(buffer.flat(), epochs, batch)
        policy.load_state_dict(theirs.state_dict(spec))

    times = windows_of({"kernel": by_kernel, "torch": by_torch, "collect": collect_only}, windows)
    fault = env.device_fault()
    env.close()
    medians = {name: float(np.median(t)) for name, t in times.items()}
    parts.update(steps=steps, envs=n, frame=300, spp=100, net=list(widths), updates=epochs * (steps * n // batch),
                 us_per_iteration=medians, windows_us={name: [round(x) for x in t] for name, t in times.items()},
                 spread={name: float((max(t) - min(t)) / np.median(t)) for name, t in times.items()}, device_fault=fault)
    return parts


def main():
    argv = list(sys.argv[1:])
    windows = option(argv, "--windows", 7)
    torch.zeros(1, device="cuda")
    env = harness.DeviceVectorDiscreteSteps(num_envs=1, frame_height=16, samples_per_pixel=1, seed=0, device=0,
                                            device_initializer=True)
    out = {"windows": windows, "train": [train_times(env, *shape, windows) for shape in SHAPES]}
    env.close()
    if "--no-iteration" not in argv:
        out["iteration"] = iteration_times(windows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
