"""The recurrent PPO actor-critic with the state-dependent-exploration Gaussian head: sb3-contrib's MlpLstmPolicy with
use_sde=True (RecurrentActorCriticPolicy: one LSTM layer per net, lstm_actor and lstm_critic, then the MLPs; the pi head
is StateDependentNoiseDistribution with full_std=True, use_expln=False, squash_output=False, learn_features=False,
epsilon=1e-6) for the one-dimensional Box(-1, 1, (1,)), as the reference's examples/ppo_lstm_untuned.yml trains
ContinuousJumps-v0.  The noise features are the activations of the last pi MLP layer, after the LSTM.

One definition of the arithmetic (include/reinfocus_hip.h, "lstm sde policy"): lstm_sde_numpy below composes the cell of
environments/lstm.py with the head of environments/sde.py and is the oracle; lstm_forward_kernel<true> (csrc/rf_lstm.h)
computes the same bits in one launch, sde_noise_kernel (csrc/rf_sde.h) the exploration matrix.  The update is
environments/lstm_learner.py's, which takes the head from the spec's kind.

    LstmSdePolicySpec    LstmPolicySpec's network with a pi head of one output (the mean) and log_std [L] packed last
    LstmSdePolicy        the numpy twin: reset_noise / act / values over numpy arrays, the state float32 [2, 2, n, H]
    DeviceLstmSdePolicy  the same over torch tensors on a device-resident environment's GPU: one launch per call

enable_critic_lstm=False is the spec's, as LstmPolicySpec's ("lstm critic": the head touches only the pi net).  Still out
of scope, and refused or absent: more than one action dimension, n_lstm_layers > 1, shared_lstm=True, lstm_hidden > 256,
learn_features=True, use_expln, squash_output.

torch is imported lazily, by DeviceLstmSdePolicy only (reinfocus_amd/torch_interop.py says why import order matters).
"""

import numpy as np

from reinfocus_amd.environments import lstm as lstm_module
from reinfocus_amd.environments import policy as policy_module
from reinfocus_amd.environments import sde as sde_module
from reinfocus_amd.environments.lstm import lstm_layer, next_state, recurrent_entries, vf_latents
from reinfocus_amd.environments.policy import _NAN, DETERMINISTIC, MAX_WIDTH, activation, canonical, f32, linear
from reinfocus_amd.environments.sde import env_actions_of, log_prob_of, noise_numpy, sigma_of, std2_of


class LstmSdePolicySpec(lstm_module.LstmPolicySpec):
    """LstmPolicySpec with the Gaussian head: per net (pi first) the LSTM and what SdePolicySpec packs for that net with
    input width H (a pi head of one output), then SB3's log_std [L, 1] (L = the last pi width) last of everything."""

    kind = "lstm_sde"  # (what Rollout.collect and the learners dispatch on)

    def __init__(self, obs_width, lstm_hidden=256, pi=(64, 64), vf=(64, 64), activation="tanh", log_std_init=0.0,
                 enable_critic_lstm=True):
        self.enable_critic_lstm = bool(enable_critic_lstm)
        self.lstm_hidden = int(lstm_hidden)
        if not 1 <= self.lstm_hidden <= MAX_WIDTH:
            raise ValueError(f"lstm_hidden {lstm_hidden} is not in 1 .. {MAX_WIDTH}")
        if not 1 <= int(obs_width) <= MAX_WIDTH:
            raise ValueError(f"obs_width {obs_width} is not in 1 .. {MAX_WIDTH}")
        mlp = sde_module.SdePolicySpec(self.lstm_hidden, pi=pi, vf=vf, activation=activation)  # (its checks)
        self.obs_width, self.n_actions = int(obs_width), 1
        self.pi, self.vf, self.activation = mlp.pi, mlp.vf, mlp.activation
        self.log_std_init = float(log_std_init)
        split = 2 * (len(self.pi) + 1)  # (the entries of the pi MLP and head)
        # (state_dict name, packed offset, packed shape, is a weight)
        self.entries, at = recurrent_entries(self.obs_width, self.lstm_hidden, mlp.entries[:split], mlp.entries[split:-1],
                                             self.enable_critic_lstm)
        self.log_std_at, self.latent = at, self.pi[-1]
        self.entries.append(("log_std", at, (1, self.latent), True))  # (SB3's [L, 1] is this, transposed)
        self.size = at + self.latent

    def _net_entries(self):
        return len(self.entries) - 1  # (log_std is no net's)

    def initial(self):
        params = np.zeros(self.size, dtype=f32)
        params[self.log_std_at:] = f32(self.log_std_init)
        return params


def _refuse_discrete(action_space):
    try:
        sde_module._refuse_discrete(action_space)
    except ValueError as error:
        raise ValueError(f"{error} (LstmPolicy / DeviceLstmPolicy are the recurrent policies of Discrete spaces)") from None


def _mlp(spec, layers, x):
    for weight_t, bias in layers:
        x = activation(linear(x, weight_t, bias), spec.activation)
    return x


def lstm_sde_numpy(spec, params, obs, episode_starts, state, final_obs=None, theta=None, deterministic=False,
                   values_only=False):
    """The definition, literally.  obs float32 [n, D], episode_starts uint8 [n] (non-zero: a start), state float32
    [2, 2, n, H], final_obs float32 [n, D] or None, theta float32 [n, L] (a sampled call).  Returns a dict: "actions"
    (raw), "env_actions" (clamped), "log_probs", "mean", "sigma" float32 [n] (None with values_only), "values",
    "final_values" (or None), and "state": the next state float32 [2, 2, n, H] -- None with values_only."""
    obs = np.asarray(obs, dtype=f32).reshape(-1, spec.obs_width)
    n = obs.shape[0]
    params = np.asarray(params, dtype=f32).reshape(spec.size)
    state = np.asarray(state, dtype=f32).reshape(spec.state_shape(n))
    starts = np.asarray(episode_starts).reshape(n) != 0
    masked = np.where(starts[None, None, :, None], f32(0.0), state)  # a select: no NaN or inf of a dead state survives
    nets = spec.nets(params)
    out = dict.fromkeys(("actions", "env_actions", "log_probs", "mean", "sigma", "values", "final_values", "state"))
    if final_obs is not None:
        final_obs = np.asarray(final_obs, dtype=f32).reshape(obs.shape)
    h_vf, c_vf, h_final = vf_latents(spec, nets, obs, masked, state, final_obs)  # (final_obs: from the unmasked state)
    out["values"] = canonical(linear(_mlp(spec, nets[1][1], h_vf), *nets[1][2])[:, 0])
    if final_obs is not None:
        lead = final_obs[:, 0]
        out["final_values"] = np.where(lead != lead, _NAN,
                                       canonical(linear(_mlp(spec, nets[1][1], h_final), *nets[1][2])[:, 0]))
    if values_only:
        return out
    h_pi, c_pi = lstm_layer(obs, masked[0, 0], masked[0, 1], *nets[0][0])
    h = _mlp(spec, nets[0][1], h_pi)
    mu = linear(h, *nets[0][2])[:, 0]
    sigma = sigma_of(h, std2_of(params[spec.log_std_at:]))
    a = mu
    if not deterministic:
        if theta is None:
            raise ValueError("a sampled call needs theta: reset_noise() first")
        theta = np.asarray(theta, dtype=f32).reshape(n, spec.latent)
        with np.errstate(all="ignore"):
            a = mu + sde_module._rowdot(h, theta)
    out["actions"], out["env_actions"] = canonical(a), env_actions_of(a)
    out["log_probs"], out["mean"], out["sigma"] = log_prob_of(a, mu, sigma), canonical(mu), canonical(sigma)
    out["state"] = next_state(spec, h_pi, c_pi, h_vf, c_vf)
    return out


class LstmSdePolicy(lstm_module.LstmPolicy):
    """The numpy twin of DeviceLstmSdePolicy, and its oracle.  Parameters start at zero with log_std at log_std_init; the
    state starts at zero.  reset_noise() consumes n * L draws of the generator, act() none."""

    def __init__(self, spec, seed=None, num_envs=1):
        if getattr(spec, "kind", None) != "lstm_sde":
            raise TypeError(f"LstmSdePolicy needs an LstmSdePolicySpec, not {type(spec).__name__}")
        self.spec = spec
        self.num_envs = int(num_envs)  # (how many rows reset_noise() draws)
        self.params = spec.initial()
        self._state = np.zeros(spec.state_shape(self.num_envs), dtype=f32)
        self._theta = None
        self._seed(seed)

    def reset_noise(self, num_envs=None):
        """A new theta [num_envs, L] from the current log_std: num_envs * L draws."""
        if num_envs is not None:
            self.num_envs = int(num_envs)
        self._own_state(self.num_envs)  # (a state of that many rows: zeros if the number changed)
        u = self._generator.random(self.num_envs * self.spec.latent)
        self._theta = noise_numpy(self.params[self.spec.log_std_at:], u)

    def noise(self):
        return None if self._theta is None else self._theta.copy()

    def set_noise(self, theta):
        self._theta = None if theta is None else np.array(theta, dtype=f32).reshape(-1, self.spec.latent)

    def act(self, obs, episode_starts, final_obs=None, deterministic=False, states=None):
        """(actions float32 [n] (raw), values, log_probs, final_values or None, env_actions float32 [n] (clamped)); the
        state advances as LstmPolicy.act's does."""
        obs = np.asarray(obs, dtype=f32).reshape(-1, self.spec.obs_width)
        n = obs.shape[0]
        if not deterministic and (self._theta is None or self._theta.shape[0] != n):
            raise ValueError(f"a sampled act() of {n} environments needs reset_noise() for that many first")
        source, target = (self._own_state(n),) * 2 if states is None else states
        got = lstm_sde_numpy(self.spec, self.params, obs, episode_starts, source, final_obs, self._theta, deterministic)
        target[...] = got["state"]
        return got["actions"], got["values"], got["log_probs"], got["final_values"], got["env_actions"]

    def values(self, obs, episode_starts, final_obs=None):
        """V(obs) from the own state masked by episode_starts; with final_obs (V(obs), V(final_obs)).  The state stays."""
        obs = np.asarray(obs, dtype=f32).reshape(-1, self.spec.obs_width)
        got = lstm_sde_numpy(self.spec, self.params, obs, episode_starts, self._own_state(obs.shape[0]), final_obs,
                             values_only=True)
        return got["values"] if final_obs is None else (got["values"], got["final_values"])


class DeviceLstmSdePolicy(lstm_module.DeviceLstmPolicy):
    """The recurrent sde policy of a device-resident environment with the Box(-1, 1, (1,)) action space
    (DeviceVectorContinuousJumps, or a DeviceVectorEnvironment with that space), over torch tensors on its GPU; used as
    LstmSdePolicy is and bit for bit equal to it.  reset_noise() is one launch of sde_noise_kernel
    (rf_lstm_sde_noise_reset) into a [n, L] tensor the policy owns, every act() / values() one launch of
    lstm_forward_kernel<true> (rf_lstm_sde_forward), all on torch's current stream: nothing waits for the host."""

    def __init__(self, env, spec, seed=None):
        self._device_env(env)
        _refuse_discrete(env.single_action_space)
        if getattr(spec, "kind", None) != "lstm_sde":
            raise TypeError(f"DeviceLstmSdePolicy needs an LstmSdePolicySpec, not {type(spec).__name__}")
        self._attach(env, spec, seed)
        self.num_envs = int(env.num_envs)
        self._linear = not spec.enable_critic_lstm  # (the sibling entry points over rf_lstm_critic_desc: "lstm critic")
        size = self._ctx.lstm_critic_params_size(spec.critic_desc(), sde=True) if self._linear \
            else self._ctx.lstm_sde_params_size(spec.desc())
        if size != spec.size:
            raise RuntimeError("rf_lstm_sde_params_size / rf_lstm_critic_sde_params_size disagrees with the packed parameters")
        self.params.copy_(self._torch.from_numpy(spec.initial()))
        self._state = self._torch.zeros(spec.state_shape(self.num_envs), dtype=self._torch.float32, device=self.device)
        self._theta = None

    def reset_noise(self, num_envs=None):
        """A new theta [n, L] from the current log_std: one launch, and n * L draws of the host generator.  n is the
        environment's num_envs (the state has that many rows); any other num_envs is refused."""
        torch = self._torch
        if num_envs is not None and int(num_envs) != self.num_envs:
            raise ValueError(f"reset_noise({num_envs}): the policy's state has {self.num_envs} environments")
        self._interop.check_one_runtime()
        if self._theta is None:
            self._theta = torch.zeros((self.num_envs, self.spec.latent), dtype=torch.float32, device=self.device)
        reset = self._ctx.lstm_critic_sde_noise_reset if self._linear else self._ctx.lstm_sde_noise_reset
        reset(self.spec.critic_desc() if self._linear else self.spec.desc(), self.params.data_ptr(), self.num_envs,
              policy_module.generator_words(self._bit_generator), self._theta.data_ptr(), self._io._stream())
        self._bit_generator.advance(self.num_envs * self.spec.latent)  # (after the call was taken)

    def noise(self):
        return None if self._theta is None else self._theta.clone()

    def set_noise(self, theta):
        torch = self._torch
        if theta is None:
            self._theta = None
            return
        if not isinstance(theta, torch.Tensor) or theta.dtype != torch.float32 \
                or tuple(theta.shape) != (self.num_envs, self.spec.latent):
            raise ValueError(f"theta must be a torch.float32 tensor ({self.num_envs}, {self.spec.latent}) on {self.device}")
        self._io._on_device(theta, "theta")
        self._theta = theta.contiguous().clone()

    def _forward(self, obs, episode_starts, final_obs, state_in, state_out, theta, flags, actions, env_actions, log_probs,
                 values, final_values):
        self._interop.check_one_runtime()
        pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        forward = self._ctx.lstm_critic_sde_forward if self._linear else self._ctx.lstm_sde_forward
        forward(self.spec.critic_desc() if self._linear else self.spec.desc(), self.params.data_ptr(), obs.shape[0],
                obs.data_ptr(), episode_starts.data_ptr(), pointer(final_obs), state_in.data_ptr(), pointer(state_out),
                pointer(theta), flags, pointer(actions), pointer(env_actions), pointer(log_probs), pointer(values),
                pointer(final_values), None, None, self._io._stream())

    def act(self, obs, episode_starts, final_obs=None, deterministic=False, out=None, states=None):
        """(actions float32 [n] (raw), values, log_probs, final_values or None, env_actions float32 [n] (clamped)) of obs
        float32 [n, D], episode_starts uint8 or bool [n] (and final_obs as obs); out=(actions, values, log_probs,
        final_values or None, env_actions) writes into the caller's rows.  The state advances as DeviceLstmPolicy.act's
        does (states=(in, out) goes from one tensor to another).  One launch; no draw is consumed."""
        torch = self._torch
        obs, episode_starts = self._inputs(obs, episode_starts, final_obs)
        n = self.num_envs
        if not deterministic and self._theta is None:
            raise ValueError(f"a sampled act() of {n} environments needs reset_noise() first")
        if states is None:
            state_in = state_out = self._state
        else:
            state_in, state_out = states
            state_in, state_out = self._checked_state(state_in, "states[0]"), self._checked_state(state_out, "states[1]")
        given = (None,) * 5 if out is None else tuple(out)
        if len(given) != 5:
            raise TypeError("out must be (actions, values, log_probs, final_values or None, env_actions)")
        actions = self._out("raw_actions", given[0], n, torch.float32)
        values = self._out("values", given[1], n, torch.float32)
        log_probs = self._out("log_probs", given[2], n, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[3], n, torch.float32)
        env_actions = self._out("env_actions", given[4], n, torch.float32)
        self._forward(obs, episode_starts, final_obs, state_in, state_out, None if deterministic else self._theta,
                      DETERMINISTIC if deterministic else 0, actions, env_actions, log_probs, values, final_values)
        return actions, values, log_probs, final_values, env_actions

    def values(self, obs, episode_starts, final_obs=None, out=None):
        """V(obs) from the own state masked by episode_starts; with final_obs (V(obs), V(final_obs)).  out=(values,
        final_values or None).  One launch, no draw; the state stays."""
        torch = self._torch
        obs, episode_starts = self._inputs(obs, episode_starts, final_obs)
        n = self.num_envs
        given = (None, None) if out is None else tuple(out)
        if len(given) != 2:
            raise TypeError("out must be (values, final_values or None)")
        values = self._out("last_values", given[0], n, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[1], n, torch.float32)
        self._forward(obs, episode_starts, final_obs, self._state, None, None, 0, None, None, None, values, final_values)
        return values if final_obs is None else (values, final_values)
