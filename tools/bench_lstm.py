"""Development benchmark of the lstm policy (rf_lstm_forward: DeviceLstmPolicy.act, DeviceRollout.collect over it): the
recurrent actor-critic forward with its state and sampling as one launch of lstm_forward_kernel against the eager-torch
restatement of sb3-contrib's RecurrentActorCriticPolicy -- nn.LSTM x 2, the masking of their states by (1 - start), two
nn.Sequential MLPs, Categorical.sample and log_prob, the value of the final observation from the unmasked critic state --
on the same device tensors in the same process, at n = 8 for the networks of ppo_lstm_tuned.yml (H = 16, [64, 64] ReLU)
and ppo_lstm_untuned.yml (H = 256, [64, 64] tanh); DevicePolicy.act with the same MLP next to them for scale.  Alternating
windows, each ended by one synchronisation; medians and the windows' spread.  Then an iteration of collect with n_steps =
8 at 8 x 300 x 300 px x 100 samples with either policy.  One JSON line.
usage (GPU box):  python tools/bench_lstm.py [--windows 7] [--calls 200] [--no-iteration]"""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness  # noqa: E402
from tools.bench_policy import TorchPolicy, option, random_state, windows_of  # noqa: E402

ENVS, STEPS, ACTIONS, GAMMA, GAE_LAMBDA = 8, 8, 13, 0.99, 0.95
NETS = {"tuned": dict(lstm_hidden=16, pi=(64, 64), vf=(64, 64), activation="relu"),
        "untuned": dict(lstm_hidden=256, pi=(64, 64), vf=(64, 64), activation="tanh")}


class _Mlp:  # (what TorchPolicy reads of a spec: the MLPs' input is the LSTM's output)
    def __init__(self, spec):
        self.obs_width, self.pi, self.vf = spec.lstm_hidden, spec.pi, spec.vf
        self.activation, self.n_actions = spec.activation, spec.n_actions


class TorchLstm:
    """The eager-torch form: what sb3-contrib launches for one forward of its MlpLstmPolicy."""

    def __init__(self, spec, state, n):
        self.nets = TorchPolicy(_Mlp(spec), state)
        self.lstm = {}
        for name in ("lstm_actor", "lstm_critic"):
            lstm = torch.nn.LSTM(spec.obs_width, spec.lstm_hidden, num_layers=1).cuda()
            lstm.load_state_dict({part: state[f"{name}.{part}"] for part in
                                  ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
            self.lstm[name] = lstm
        zeros = lambda: torch.zeros(1, n, spec.lstm_hidden, device="cuda")  # noqa: E731
        self.pi_state, self.vf_state = (zeros(), zeros()), (zeros(), zeros())

    @torch.no_grad()
    def act(self, obs, starts, final_obs=None):
        keep = (1.0 - starts.float()).view(1, -1, 1)
        final_values = None
        if final_obs is not None:  # (predict_values(terminal_obs, lstm_states.vf) from the state as it is)
            final_values = self.nets.vf(self.lstm["lstm_critic"](final_obs[None], self.vf_state)[0][0])[:, 0]
        latent_pi, self.pi_state = self.lstm["lstm_actor"](obs[None], (self.pi_state[0] * keep, self.pi_state[1] * keep))
        latent_vf, self.vf_state = self.lstm["lstm_critic"](obs[None], (self.vf_state[0] * keep, self.vf_state[1] * keep))
        distribution = torch.distributions.Categorical(logits=self.nets.pi(latent_pi[0]))
        actions = distribution.sample()
        return actions, self.nets.vf(latent_vf[0])[:, 0], distribution.log_prob(actions), final_values

    @torch.no_grad()
    def values(self, obs, starts, final_obs=None):
        keep = (1.0 - starts.float()).view(1, -1, 1)
        values = self.nets.vf(self.lstm["lstm_critic"](obs[None], (self.vf_state[0] * keep, self.vf_state[1] * keep))[0][0])[:, 0]
        if final_obs is None:
            return values
        return values, self.nets.vf(self.lstm["lstm_critic"](final_obs[None], self.vf_state)[0][0])[:, 0]


def pair(env, name):
    spec = harness.LstmPolicySpec(int(env.single_observation_space.shape[0]), ACTIONS, **NETS[name])
    state = random_state(spec, 1)
    device = harness.DeviceLstmPolicy(env, spec, 0)
    device.load_state_dict(state)
    return spec, state, device, TorchLstm(spec, state, env.num_envs)


def act_times(env, name, windows, calls):
    spec, state, device, eager = pair(env, name)
    rng = np.random.default_rng(ENVS)
    obs = torch.from_numpy(rng.standard_normal((ENVS, spec.obs_width)).astype(np.float32)).cuda()
    final_obs = torch.from_numpy(rng.standard_normal((ENVS, spec.obs_width)).astype(np.float32)).cuda()
    final_obs[::2] = float("nan")
    starts = torch.zeros(ENVS, dtype=torch.uint8, device="cuda")
    starts[3] = 1
    # the two forms compute the same network: values agree to float32 rounding (not bit for bit: torch's order is its own)
    agree = float((device.values(obs, starts) - eager.values(obs, starts)).abs().max())
    mlp = harness.MlpPolicySpec(spec.obs_width, ACTIONS, pi=spec.pi, vf=spec.vf, activation=spec.activation)
    feedforward = harness.DevicePolicy(env, mlp, 0)
    feedforward.load_state_dict(random_state(mlp, 1))
    out = windows_of({"kernel": lambda: device.act(obs, starts, final_obs), "torch": lambda: eager.act(obs, starts, final_obs),
                      "feedforward_kernel": lambda: feedforward.act(obs, final_obs)}, windows, calls)
    out.update(net=name, envs=ENVS, **{k: (list(v) if isinstance(v, tuple) else v) for k, v in NETS[name].items()},
               largest_value_difference=agree, torch_over_kernel=out["median_us"]["torch"] / out["median_us"]["kernel"])
    return out


def iteration_times(name, windows):
    """Microseconds per iteration of collect (n_steps = 8 at 8 x 300 x 300 x 100, records and the learner view on):
    DeviceRollout.collect(DeviceLstmPolicy) against the explicit loop with the eager-torch policy."""
    env = harness.DeviceVectorDiscreteSteps(max_episode_steps=20, num_envs=ENVS, frame_height=300, samples_per_pixel=100,
                                            seed=0, device=0, device_initializer=True, episode_records=True,
                                            learner_view=harness.LearnerView(frame_stack=1))
    spec, state, device, eager = pair(env, name)
    buffer = harness.DeviceRollout(env, STEPS, GAMMA, GAE_LAMBDA)
    carried = {"starts": torch.ones(ENVS, dtype=torch.uint8, device="cuda")}

    def by_kernel():
        buffer.collect(device)

    def by_torch():
        obs, final_obs, starts = buffer.observations[0], None, carried["starts"]
        for _ in range(STEPS):
            actions, values, log_probs, final_values = eager.act(obs, starts, final_obs)
            if final_obs is not None:
                buffer.bootstrap(final_values)
            obs, _, _, starts, info = buffer.step(actions, values, log_probs)
            final_obs = info["final_observation"]
        last_values, final_values = eager.values(obs, starts, final_obs)
        buffer.bootstrap(final_values)
        buffer.finish(last_values)
        carried["starts"] = starts.clone()

    forms = {"kernel": by_kernel, "torch": by_torch}
    times = {form: [] for form in forms}
    first = env.reset_tensors()[0]
    for window in range(windows + 1):  # (the first one warms up: the replayed graph exists from the second step on)
        for form, run in forms.items():
            buffer.start(first if window == 0 and form == "kernel" else None)
            torch.cuda.synchronize()
            start = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if window:
                times[form].append(1e6 * (time.perf_counter() - start))
    fault = env.device_fault()
    env.close()
    medians = {form: float(np.median(t)) for form, t in times.items()}
    return {"net": name, "steps": STEPS, "envs": ENVS, "frame": 300, "spp": 100, "us_per_iteration": medians,
            "windows_us": {form: [round(x) for x in t] for form, t in times.items()},
            "spread": {form: float((max(t) - min(t)) / np.median(t)) for form, t in times.items()}, "device_fault": fault}


def main():
    argv = list(sys.argv[1:])
    windows, calls = option(argv, "--windows", 7), option(argv, "--calls", 200)
    torch.zeros(1, device="cuda")
    env = harness.DeviceVectorDiscreteSteps(num_envs=ENVS, frame_height=16, samples_per_pixel=1, seed=0, device=0,
                                            device_initializer=True)
    out = {"windows": windows, "calls": calls, "act": [act_times(env, name, windows, calls) for name in NETS]}
    env.close()
    if "--no-iteration" not in argv:
        out["iteration"] = [iteration_times(name, windows) for name in NETS]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
