"""Development benchmark of the policy stage (rf_policy_forward, DevicePolicy.act, DeviceRollout.collect): the whole
actor-critic forward with sampling as one launch of policy_forward_kernel against the eager-torch form it replaces --
two nn.Sequential nets, Categorical.sample and log_prob, as stable-baselines3's MlpPolicy runs them -- on the same
device tensors in the same process.  Alternating windows, medians, the windows' spread.  Then the per-step time of a
whole rollout with either policy.  One JSON line.
usage (GPU box):  python tools/bench_policy.py [--windows 7] [--calls 50] [--no-rollouts]
Shapes (profiles/policy.md): n = 1, 8 and 4096 observations of width 20 through [64, 64] tanh and [256, 256] ReLU;
rollouts of 128 steps at 1 x 64 x 64 px x 1 sample and at 8 x 300 x 300 px x 100 samples."""
import json
import os
import sys
import time

import numpy as np
import torch  # (before the library is loaded: one HIP runtime per process, reinfocus_amd/torch_interop.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness  # noqa: E402

GAMMA, GAE_LAMBDA, STACK, ACTIONS = 0.99, 0.95, 5, 13
NETS = (((64, 64), "tanh"), ((256, 256), "relu"))


def option(argv, name, default):
    if name in argv:
        at = argv.index(name)
        value = int(argv[at + 1])
        del argv[at:at + 2]
        return value
    return default


def random_state(spec, seed):
    rng = np.random.default_rng(seed)
    return {name: torch.from_numpy(((rng.standard_normal(shape[::-1]) / np.sqrt(shape[0])) if is_weight
                                    else 0.1 * rng.standard_normal(shape)).astype(np.float32)).cuda()
            for name, _, shape, is_weight in spec.entries}


class TorchPolicy:
    """The eager-torch form: what stable-baselines3 launches for one forward of its MlpPolicy."""

    def __init__(self, spec, state):
        def net(widths, extractor, head_name, outputs):
            act = torch.nn.Tanh if spec.activation == "tanh" else torch.nn.ReLU
            layers, fan_in = [], spec.obs_width
            for width in widths:
                layers += [torch.nn.Linear(fan_in, width), act()]
                fan_in = width
            model = torch.nn.Sequential(*layers, torch.nn.Linear(fan_in, outputs)).cuda()
            keys = [f"mlp_extractor.{extractor}.{2 * i}" for i in range(len(widths))] + [head_name]
            model.load_state_dict({f"{2 * j}.{part}": state[f"{key}.{part}"] for j, key in enumerate(keys)
                                   for part in ("weight", "bias")})
            return model

        self.pi = net(spec.pi, "policy_net", "action_net", spec.n_actions)
        self.vf = net(spec.vf, "value_net", "value_net", 1)

    @torch.no_grad()
    def act(self, obs, final_obs=None):
        distribution = torch.distributions.Categorical(logits=self.pi(obs))
        actions = distribution.sample()
        return (actions, self.vf(obs)[:, 0], distribution.log_prob(actions),
                None if final_obs is None else self.vf(final_obs)[:, 0])

    @torch.no_grad()
    def values(self, obs, final_obs=None):
        return self.vf(obs)[:, 0] if final_obs is None else (self.vf(obs)[:, 0], self.vf(final_obs)[:, 0])


def windows_of(forms, windows, calls):
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
    medians = {name: float(np.median(t)) for name, t in times.items()}
    return {"median_us": medians, "spread": {name: float((max(t) - min(t)) / np.median(t)) for name, t in times.items()},
            "windows_us": {name: [round(x, 2) for x in t] for name, t in times.items()}}


def act_times(env, widths, activation, n, windows, calls):
    spec = harness.MlpPolicySpec(4 * STACK, ACTIONS, pi=widths, vf=widths, activation=activation)
    state = random_state(spec, 1)
    device, eager = harness.DevicePolicy(env, spec, 0), TorchPolicy(spec, state)
    device.load_state_dict(state)
    rng = np.random.default_rng(n)
    obs = torch.from_numpy(rng.standard_normal((n, spec.obs_width)).astype(np.float32)).cuda()
    final_obs = torch.from_numpy(rng.standard_normal((n, spec.obs_width)).astype(np.float32)).cuda()
    final_obs[::2] = float("nan")
    # the two forms compute the same network: values agree to float32 rounding (not bit for bit: torch's order is its own)
    agree = float((device.values(obs) - eager.values(obs)).abs().max())
    out = windows_of({"kernel": lambda: device.act(obs, final_obs), "torch": lambda: eager.act(obs, final_obs)},
                     windows, calls)
    out.update(net=list(widths), activation=activation, envs=n, largest_value_difference=agree,
               torch_over_kernel=out["median_us"]["torch"] / out["median_us"]["kernel"])
    return out


def collect_times(steps, n, frame, spp, widths, activation, windows):
    """Microseconds per step of whole rollouts: DeviceRollout.collect(DevicePolicy) against the explicit loop with the
    eager-torch policy (act, step with its three row copies, bootstrap), records and the learner view on."""
    env = harness.DeviceVectorDiscreteSteps(max_episode_steps=20, num_envs=n, frame_height=frame, samples_per_pixel=spp,
                                            seed=0, device=0, device_initializer=True, episode_records=True,
                                            learner_view=harness.LearnerView(frame_stack=STACK))
    spec = harness.MlpPolicySpec(4 * STACK, ACTIONS, pi=widths, vf=widths, activation=activation)
    state = random_state(spec, 1)
    device, eager = harness.DevicePolicy(env, spec, 0), TorchPolicy(spec, state)
    device.load_state_dict(state)
    buffer = harness.DeviceRollout(env, steps, GAMMA, GAE_LAMBDA)

    def by_kernel():
        buffer.collect(device)

    def by_torch():
        obs, final_obs = buffer.observations[0], None
        for _ in range(steps):
            actions, values, log_probs, final_values = eager.act(obs, final_obs)
            if final_obs is not None:
                buffer.bootstrap(final_values)
            obs, _, _, _, info = buffer.step(actions, values, log_probs)
            final_obs = info["final_observation"]
        last_values, final_values = eager.values(obs, final_obs)
        buffer.bootstrap(final_values)
        buffer.finish(last_values)

    forms = {"kernel": by_kernel, "torch": by_torch}
    times = {name: [] for name in forms}
    first = env.reset_tensors()[0]
    for window in range(windows + 1):  # (the first one warms up: the replayed graph exists from the second step on)
        for name, form in forms.items():
            buffer.start(first if window == 0 and name == "kernel" else None)
            torch.cuda.synchronize()
            start = time.perf_counter()
            form()
            torch.cuda.synchronize()
            if window:
                times[name].append(1e6 * (time.perf_counter() - start) / steps)
    fault = env.device_fault()
    env.close()
    medians = {name: float(np.median(t)) for name, t in times.items()}
    return {"steps": steps, "envs": n, "frame": frame, "spp": spp, "net": list(widths), "activation": activation,
            "us_per_step": medians, "windows_us_per_step": {name: [round(x, 1) for x in t] for name, t in times.items()},
            "saved_us_per_step": medians["torch"] - medians["kernel"], "device_fault": fault}


def main():
    argv = list(sys.argv[1:])
    windows, calls = option(argv, "--windows", 7), option(argv, "--calls", 50)
    torch.zeros(1, device="cuda")
    env = harness.DeviceVectorDiscreteSteps(num_envs=1, frame_height=16, samples_per_pixel=1, seed=0, device=0,
                                            device_initializer=True)
    out = {"windows": windows, "calls": calls,
           "act": [act_times(env, widths, activation, n, windows, calls) for widths, activation in NETS
                   for n in (1, 8, 4096)]}
    env.close()
    if "--no-rollouts" not in argv:
        out["collect"] = [collect_times(128, 1, 64, 1, *NETS[0], windows), collect_times(128, 8, 300, 100, *NETS[1], windows)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
