"""Development benchmark of the sde policy (rf_sde_noise_reset, rf_sde_forward, rf_sde_update: DeviceSdePolicy and
DeviceLearner over it) at ppo_tuned.yml's ContinuousJumps-v0 shape -- 8 environments x 128 steps = 1024 rows, minibatches
of 512, 10 epochs, [64, 64] ReLU, frame_stack 5, sde_sample_freq 8 -- against the same restated in eager torch:
stable-baselines3's StateDependentNoiseDistribution (full_std, learn_features=False) with torch.distributions.Normal,
its loss, backward, clip_grad_norm_ and torch.optim.Adam(eps=1e-5), on the same device tensors in the same process.
Alternating windows, each ended by one synchronisation; medians and the windows' spread.  One JSON line.
usage (GPU box):  python tools/bench_sde.py [--windows 7] [--no-iteration]
Measured: time per act() (and per reset_noise()), time per update, time for a whole iteration (collect of 128 steps at
8 x 300 x 300 px x 100 samples, then the 20 updates).  The torch form leaves out what SB3 logs per minibatch."""
import json
import os
import sys

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness  # noqa: E402
from tools.bench_learner import summary, windows_of  # noqa: E402
from tools.bench_policy import STACK, TorchPolicy, option, random_state  # noqa: E402
from tools.bench_policy import windows_of as call_windows_of  # noqa: E402

ENVS, STEPS, BATCH, EPOCHS, WIDTHS, ACTIVATION, FREQ = 8, 128, 512, 10, (64, 64), "relu", 8
GAMMA, GAE_LAMBDA, LOG_STD_INIT = 0.95, 0.9, -0.8696787910863373
HYPER = dict(learning_rate=0.0004305249051633182, clip_range=0.2, ent_coef=3.039717996777601e-08,
             vf_coef=0.9269765257976839, max_grad_norm=0.8)


class TorchSde:
    """The eager-torch form of the sde actor-critic and of PPO.train() over it."""

    def __init__(self, spec, state):
        nets = {key: value for key, value in state.items() if key != "log_std"}
        self.nets = TorchPolicy(spec, nets)
        self.pi, self.vf = self.nets.pi, self.nets.vf
        self.log_std = torch.nn.Parameter(state["log_std"].clone())
        self.parameters = list(self.pi.parameters()) + list(self.vf.parameters()) + [self.log_std]
        self.optimizer = torch.optim.Adam(self.parameters, lr=HYPER["learning_rate"], eps=1e-5)
        self.theta = None

    @torch.no_grad()
    def reset_noise(self, n):
        std = torch.exp(self.log_std)[:, 0]
        self.theta = torch.distributions.Normal(torch.zeros_like(std), std).rsample((n,))

    def distribution(self, obs):
        latent = self.pi[:-1](obs)
        variance = torch.mm(latent.detach() ** 2, torch.exp(self.log_std) ** 2)[:, 0]
        return latent, torch.distributions.Normal(self.pi[-1](latent)[:, 0], torch.sqrt(variance + 1e-6))

    @torch.no_grad()
    def act(self, obs, final_obs=None):
        latent, distribution = self.distribution(obs)
        actions = distribution.mean + (latent * self.theta).sum(dim=1)
        return (actions, self.vf(obs)[:, 0], distribution.log_prob(actions),
                None if final_obs is None else self.vf(final_obs)[:, 0], torch.clamp(actions, -1.0, 1.0))

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
                _, distribution = self.distribution(obs)
                ratio = torch.exp(distribution.log_prob(actions) - old)
                policy_loss = -torch.min(advantages * ratio, advantages * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
                value_loss = torch.nn.functional.mse_loss(returns, self.vf(obs).flatten())
                loss = policy_loss + HYPER["ent_coef"] * -distribution.entropy().mean() + HYPER["vf_coef"] * value_loss
                self.optimizer.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(self.parameters, HYPER["max_grad_norm"])
                self.optimizer.step()


class Slabs:
    """What train() asks of a finished rollout, over random tensors."""

    def __init__(self, env, rows, width, seed):
        rng = np.random.default_rng(seed)
        self.env, self.device = env, torch.device("cuda", 0)
        normal = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()  # noqa: E731
        self._flat = {"observations": normal(rows, width), "actions": normal(rows), "values": normal(rows),
                      "log_probs": -1.5 + 0.1 * normal(rows), "advantages": normal(rows), "returns": normal(rows)}

    def flat(self):
        return self._flat


def pair(env):
    spec = harness.SdePolicySpec(int(env.single_observation_space.shape[0]), pi=WIDTHS, vf=WIDTHS, activation=ACTIVATION,
                                 log_std_init=LOG_STD_INIT)
    state = random_state(spec, 1)
    state["log_std"] = torch.full_like(state["log_std"], LOG_STD_INIT)
    policy = harness.DeviceSdePolicy(env, spec, 0)
    policy.load_state_dict(state)
    return spec, policy, harness.DeviceLearner(policy, **HYPER), TorchSde(spec, state)


def stage_times(env, windows):
    spec, policy, learner, eager = pair(env)
    rows = ENVS * STEPS
    obs = torch.from_numpy(np.random.default_rng(2).standard_normal((ENVS, spec.obs_width)).astype(np.float32)).cuda()
    policy.reset_noise(ENVS)
    eager.reset_noise(ENVS)
    out = {"act": call_windows_of({"kernel": lambda: policy.act(obs, obs), "torch": lambda: eager.act(obs, obs)}, windows,
                                  200),
           "reset_noise": call_windows_of({"kernel": lambda: policy.reset_noise(ENVS), "torch": lambda: eager.reset_noise(ENVS)},
                                          windows, 200)}
    slabs = Slabs(env, rows, spec.obs_width, rows)
    updates = EPOCHS * -(-rows // BATCH)
    last = {}

    def by_kernel():
        last["stats"] = learner.train(slabs, EPOCHS, BATCH)

    out["update"] = summary(windows_of({"kernel": by_kernel, "torch": lambda: eager.train(slabs.flat(), EPOCHS, BATCH)},
                                       windows), updates)
    stats = last["stats"].cpu().numpy()
    out["update"].update(rows=rows, batch=BATCH, epochs=EPOCHS, updates_per_train=updates, unit="us per update",
                         skipped_updates=int((stats[:, 7] != 0).sum()), last_loss=float(stats[-1, 6]))
    for key in ("act", "reset_noise"):
        out[key]["torch_over_kernel"] = out[key]["median_us"]["torch"] / out[key]["median_us"]["kernel"]
        out[key]["unit"] = "us per call"
    return out


def iteration_times(windows):
    """Microseconds per iteration: collect of 128 steps at 8 x 300 x 300 x 100 with sde_sample_freq 8, then the 20
    updates -- by the device policy and learner; or with the torch forms in their place (the environment's step and the
    GAE kernel are the same in both)."""
    env = harness.DeviceVectorContinuousJumps(max_episode_steps=20, num_envs=ENVS, frame_height=300, samples_per_pixel=100,
                                              seed=0, device=0, device_initializer=True, episode_records=True,
                                              learner_view=harness.LearnerView(frame_stack=STACK))
    spec, policy, learner, eager = pair(env)
    buffer = harness.DeviceRollout(env, STEPS, GAMMA, GAE_LAMBDA)
    buffer.start(env.reset_tensors()[0])
    buffer.collect(policy, sde_sample_freq=FREQ)

    def collect_only():
        buffer.start()
        buffer.collect(policy, sde_sample_freq=FREQ)

    def by_kernel():
        collect_only()
        learner.train(buffer, EPOCHS, BATCH)

    def by_torch():
        buffer.start()
        eager.reset_noise(ENVS)
        final_obs = None
        for t in range(STEPS):
            if t % FREQ == 0:
                eager.reset_noise(ENVS)
            actions, values, log_probs, final_values, clamped = eager.act(buffer.observations[t], final_obs)
            if final_obs is not None:
                buffer.bootstrap(final_values)
            final_obs = buffer.step(actions, values, log_probs, clamped)[4]["final_observation"]
        buffer.bootstrap(eager.vf(final_obs)[:, 0].detach())
        buffer.finish(eager.vf(buffer.observations[STEPS])[:, 0].detach())
        eager.train(buffer.flat(), EPOCHS, BATCH)

    times = windows_of({"kernel": by_kernel, "torch": by_torch, "collect": collect_only}, windows)
    fault = env.device_fault()
    env.close()
    medians = {name: float(np.median(t)) for name, t in times.items()}
    return dict(steps=STEPS, envs=ENVS, frame=300, spp=100, net=list(WIDTHS), updates=EPOCHS * (STEPS * ENVS // BATCH),
                us_per_iteration=medians, windows_us={name: [round(x) for x in t] for name, t in times.items()},
                spread={name: float((max(t) - min(t)) / np.median(t)) for name, t in times.items()}, device_fault=fault)


def main():
    argv = list(sys.argv[1:])
    windows = option(argv, "--windows", 7)
    torch.zeros(1, device="cuda")
    env = harness.DeviceVectorContinuousJumps(num_envs=ENVS, frame_height=16, samples_per_pixel=1, seed=0, device=0,
                                              device_initializer=True, learner_view=harness.LearnerView(frame_stack=STACK))
    out = {"windows": windows, "obs_width": int(env.single_observation_space.shape[0])}
    out.update(stage_times(env, windows))
    env.close()
    if "--no-iteration" not in argv:
        out["iteration"] = iteration_times(windows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
