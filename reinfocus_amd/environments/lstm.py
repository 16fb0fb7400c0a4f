"""The recurrent PPO actor-critic for the vector environments: sb3-contrib's MlpLstmPolicy (RecurrentActorCriticPolicy at
its defaults: one LSTM layer per net, lstm_actor and lstm_critic, then the MLPs and the Categorical head of
environments/policy.py) as the reference's recurrent configurations (examples/ppo_lstm_*.yml) use it for DiscreteSteps-v0
-- the forward with its state: an observation, the episode starts and the LSTM states in, the next action, its
log-probability, V(obs), V(final_observation) and the next states out.

One definition of the arithmetic (include/reinfocus_hip.h, "lstm policy"; the scalar functions are
csrc/rf_policy_math.h): lstm_numpy below is its numpy float32 restatement and the oracle; lstm_forward_kernel
(csrc/rf_lstm.h) computes the same bits in one launch.  Deliberate differences from sb3-contrib: the float32
order and the project's own exp32 / tanh32 / sigmoid32, and an episode start SELECTS a zero state where sb3-contrib
multiplies the state by (1 - start).

    LstmPolicySpec   the shape of the network and the packing of its parameters, from and to sb3-contrib's names
    LstmPolicy       the numpy twin: act / values over numpy arrays, the state float32 [2 nets][2: h, c][n][H]
    DeviceLstmPolicy the same over torch tensors on a device-resident environment's GPU: one launch per call

The update (back-propagation through time) is environments/lstm_learner.py; the Gaussian (sde) head on top of the LSTM
(Box action spaces) is environments/lstm_sde.py.  enable_critic_lstm=False (sb3-contrib's keyword, which rl_zoo3's sampler
draws in half of its trials) is the spec's: the vf net is then critic = nn.Linear(D, H) in front of its MLP, with no state
and no episode-start mask ("lstm critic"), and every class here works from the spec.  Out of scope, and refused or absent:
n_lstm_layers > 1, shared_lstm=True, lstm_hidden > 256.

torch is imported lazily, by DeviceLstmPolicy only (reinfocus_amd/torch_interop.py says why import order matters).
"""

import numpy as np

from reinfocus_amd.environments import policy as policy_module
from reinfocus_amd.environments import spaces
from reinfocus_amd.environments.policy import (DETERMINISTIC, MAX_WIDTH, _NAN, _bits, activation, canonical, exp32, f32,
                                               head, linear, tanh32)

LSTM_PARTS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
CRITIC_LSTM, CRITIC_LINEAR = 0, 1  # RF_LSTM_CRITIC_LSTM, RF_LSTM_CRITIC_LINEAR


def recurrent_entries(obs_width, hidden, pi_entries, vf_entries, enable_critic_lstm):
    """(entries, size) of both nets: per net (pi first) the LSTM -- or, for the vf net of enable_critic_lstm=False,
    critic.weight^T [D][H] and critic.bias [H] -- then the net's own MLP entries, moved to where they are packed."""
    entries, at = [], 0
    lstm_shapes = ((obs_width, 4 * hidden), (hidden, 4 * hidden), (4 * hidden,), (4 * hidden,))
    for lstm, own in (("lstm_actor", pi_entries), ("lstm_critic", vf_entries)):
        if lstm == "lstm_critic" and not enable_critic_lstm:
            first = (("critic.weight", (obs_width, hidden)), ("critic.bias", (hidden,)))
        else:
            first = tuple((f"{lstm}.{part}", shape) for part, shape in zip(LSTM_PARTS, lstm_shapes))
        for name, shape in first:
            entries.append((name, at, shape, len(shape) == 2))
            at += int(np.prod(shape))
        for name, _, shape, is_weight in own:
            entries.append((name, at, shape, is_weight))
            at += int(np.prod(shape))
    return entries, at


def sigmoid32(x):
    """rf_policy_math.h sigmoid32: t = exp32(-|x|); x >= 0 ? 1 / (1 + t) : t / (1 + t); NaN is NaN."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(all="ignore"):
        a = (_bits(x) & np.uint32(0x7FFFFFFF)).view(f32).reshape(x.shape)
        t = exp32(-a)
        out = np.where(x >= f32(0.0), f32(1.0) / (f32(1.0) + t), t / (f32(1.0) + t))
    assert out.dtype == f32
    return np.where(x != x, _NAN, out)


def cell(a, c):
    """(h', c') of the gate sums a float32 [..., 4] (torch's order i, f, g, o) and the cell state c float32 [...]:
    c' = f * c + i * g (two multiplies, then one add), h' = o * tanh32(c')."""
    a, c = np.asarray(a, dtype=f32), np.asarray(c, dtype=f32)
    with np.errstate(all="ignore"):
        i, f, g, o = sigmoid32(a[..., 0]), sigmoid32(a[..., 1]), tanh32(a[..., 2]), sigmoid32(a[..., 3])
        fc = f * c
        ig = i * g
        c1 = fc + ig
        h1 = o * tanh32(c1)
    assert h1.dtype == f32 and c1.dtype == f32
    return h1, c1


def lstm_layer(x, h, c, w_ih_t, w_hh_t, b_ih, b_hh):
    """One step of torch.nn.LSTM's cell over rows: x [n, D], h and c [n, H], w_ih_t [D, 4H], w_hh_t [H, 4H] (both
    transposed), biases [4H].  a = b_ih; a = a + b_hh; then x_k * W_ih, then h_k * W_hh, each a multiply and an add."""
    hidden = h.shape[1]
    with np.errstate(all="ignore"):
        a = linear(h, w_hh_t, linear(x, w_ih_t, b_ih + b_hh))  # (linear starts from its "bias": the running sums)
    return cell(a.reshape(-1, 4, hidden).transpose(0, 2, 1), c)


class LstmPolicySpec(policy_module.MlpPolicySpec):
    """The shape of the recurrent network and the packing rule of its parameters.  Packed: one float32 vector, every
    matrix transposed ([in][out]), per net (pi first): W_ih^T [D][4H], W_hh^T [H][4H], b_ih, b_hh, then the net's MLP and
    head as MlpPolicySpec packs them with input width H.  enable_critic_lstm=False ("lstm critic"): the vf net packs
    critic.weight^T [D][H] and critic.bias [H] in place of its LSTM."""

    kind = "lstm"  # (what Rollout.collect dispatches on)

    def __init__(self, obs_width, n_actions, lstm_hidden=256, pi=(64, 64), vf=(64, 64), activation="tanh",
                 enable_critic_lstm=True):
        self.enable_critic_lstm = bool(enable_critic_lstm)
        self.lstm_hidden = int(lstm_hidden)
        if not 1 <= self.lstm_hidden <= MAX_WIDTH:
            raise ValueError(f"lstm_hidden {lstm_hidden} is not in 1 .. {MAX_WIDTH}")
        if not 1 <= int(obs_width) <= MAX_WIDTH:
            raise ValueError(f"obs_width {obs_width} is not in 1 .. {MAX_WIDTH}")
        mlp = policy_module.MlpPolicySpec(self.lstm_hidden, n_actions, pi=pi, vf=vf, activation=activation)  # (its checks)
        self.obs_width, self.n_actions = int(obs_width), mlp.n_actions
        self.pi, self.vf, self.activation = mlp.pi, mlp.vf, mlp.activation
        split = 2 * (len(self.pi) + 1)  # (the entries of the pi MLP and head)
        # (state_dict name, packed offset, packed shape, is a weight)
        self.entries, self.size = recurrent_entries(self.obs_width, self.lstm_hidden, mlp.entries[:split], mlp.entries[split:],
                                                    self.enable_critic_lstm)

    def desc(self):
        """The fields of rf_lstm_policy_desc, in order: rf_policy_desc's nine, then lstm_hidden."""
        return super().desc() + (self.lstm_hidden,)

    def critic_desc(self):
        """The fields of rf_lstm_critic_desc, in order: desc()'s ten, then critic."""
        return self.desc() + (CRITIC_LSTM if self.enable_critic_lstm else CRITIC_LINEAR,)

    def checked(self, state_dict, shape_of):
        """MlpPolicySpec.checked; a state_dict of the other critic mode is refused by name."""
        other = "critic." if self.enable_critic_lstm else "lstm_critic."
        wrong = [name for name in state_dict if name.startswith(other)]
        if wrong:
            raise KeyError(f"{wrong} belong to enable_critic_lstm={not self.enable_critic_lstm}; this spec has "
                           f"enable_critic_lstm={self.enable_critic_lstm}")
        return super().checked(state_dict, shape_of)

    def state_shape(self, num_envs):
        return (2, 2, int(num_envs), self.lstm_hidden)

    def nets(self, params):
        """((pi lstm, pi layers, pi head), (vf ...)): lstm = (w_ih_t, w_hh_t, b_ih, b_hh) -- for the vf net of
        enable_critic_lstm=False (weight_t [D, H], bias [H]) of `critic` --; each layer (weight_t, bias)."""
        params = np.asarray(params, dtype=f32).reshape(self.size)
        views = [params[at:at + int(np.prod(shape))].reshape(shape) for _, at, shape, _ in self.entries[:self._net_entries()]]
        out, first = [], 0
        for net, widths in enumerate((self.pi, self.vf)):
            parts = 4 if net == 0 or self.enable_critic_lstm else 2
            lstm = tuple(views[first:first + parts])
            after = first + parts
            layers = list(zip(views[after:after + 2 + 2 * len(widths):2], views[after + 1:after + 2 + 2 * len(widths):2]))
            out.append((lstm, layers[:-1], layers[-1]))
            first = after + 2 + 2 * len(widths)
        return tuple(out)

    def _net_entries(self):
        return len(self.entries)


def _refuse_box(action_space):
    if not isinstance(action_space, spaces.Discrete):
        raise ValueError(f"the lstm policy has a Categorical head over a Discrete action space, not {action_space!r}: the "
                         "Gaussian (sde) head on top of the LSTM (ppo_lstm_untuned.yml's ContinuousJumps entry) is out of "
                         "scope for this class: LstmSdePolicy / DeviceLstmSdePolicy (environments/lstm_sde.py) have it")


def _mlp(spec, layers, last, x):
    for weight_t, bias in layers:
        x = activation(linear(x, weight_t, bias), spec.activation)
    return linear(x, *last)


def vf_latents(spec, nets, obs, masked, state, final_obs):
    """What the vf MLP reads: (latent of obs, c' of the vf cell or None, latent of final_obs or None).  With the LSTM critic
    h' of the cell from the masked state (final_obs: from the state as it is); with enable_critic_lstm=False ("lstm
    critic" C2 - C4) critic(obs) and critic(final_obs): no activation, no state, no episode starts."""
    if not spec.enable_critic_lstm:
        return linear(obs, *nets[1][0]), None, None if final_obs is None else linear(final_obs, *nets[1][0])
    h_vf, c_vf = lstm_layer(obs, masked[1, 0], masked[1, 1], *nets[1][0])
    h_final = None if final_obs is None else lstm_layer(final_obs, state[1, 0], state[1, 1], *nets[1][0])[0]
    return h_vf, c_vf, h_final


def next_state(spec, h_pi, c_pi, h_vf, c_vf):
    """The state a forward stores; with enable_critic_lstm=False both halves are the pi net's (sb3-contrib's
    lstm_states_vf = lstm_states_pi)."""
    if not spec.enable_critic_lstm:
        h_vf, c_vf = h_pi, c_pi
    return canonical(np.stack([np.stack([h_pi, c_pi]), np.stack([h_vf, c_vf])]))


def lstm_numpy(spec, params, obs, episode_starts, state, final_obs=None, u=None, deterministic=False, values_only=False):
    """The definition, literally.  obs float32 [n, D], episode_starts uint8 [n] (non-zero: a start), state float32
    [2, 2, n, H], final_obs float32 [n, D] or None, u float64 [n] (the draws of a sampled call).  Returns a dict: "logits"
    float32 [n, A], "actions" int64 [n], "log_probs" float32 [n] (None with values_only), "values", "final_values" (or
    None), and "state": the next state, float32 [2, 2, n, H] -- None with values_only (the vf net only, nothing stored)."""
    obs = np.asarray(obs, dtype=f32).reshape(-1, spec.obs_width)
    n = obs.shape[0]
    state = np.asarray(state, dtype=f32).reshape(spec.state_shape(n))
    starts = np.asarray(episode_starts).reshape(n) != 0
    masked = np.where(starts[None, None, :, None], f32(0.0), state)  # a select: no NaN or inf of a dead state survives
    nets = spec.nets(params)
    out = {"values": None, "final_values": None, "logits": None, "actions": None, "log_probs": None, "state": None}
    if final_obs is not None:
        final_obs = np.asarray(final_obs, dtype=f32).reshape(obs.shape)
    h_vf, c_vf, h_final = vf_latents(spec, nets, obs, masked, state, final_obs)  # (final_obs: from the unmasked state)
    out["values"] = canonical(_mlp(spec, nets[1][1], nets[1][2], h_vf)[:, 0])
    if final_obs is not None:
        lead = final_obs[:, 0]
        out["final_values"] = np.where(lead != lead, _NAN, canonical(_mlp(spec, nets[1][1], nets[1][2], h_final)[:, 0]))
    if values_only:
        return out
    h_pi, c_pi = lstm_layer(obs, masked[0, 0], masked[0, 1], *nets[0][0])
    logits = _mlp(spec, nets[0][1], nets[0][2], h_pi)
    if not deterministic and u is None:
        raise ValueError("a sampled call needs its draws u")
    out["actions"], out["log_probs"] = head(logits, None if deterministic else u)
    out["logits"] = canonical(logits)
    out["state"] = next_state(spec, h_pi, c_pi, h_vf, c_vf)
    return out


class LstmPolicy(policy_module._Draws):
    """The numpy twin of DeviceLstmPolicy, and its oracle.  Parameters and state start at zero."""

    def __init__(self, spec, seed=None, num_envs=None):
        if getattr(spec, "kind", None) != "lstm":
            raise TypeError(f"LstmPolicy needs an LstmPolicySpec, not {type(spec).__name__}")
        self.spec = spec
        self.params = np.zeros(spec.size, dtype=f32)
        self._state = None if num_envs is None else np.zeros(spec.state_shape(num_envs), dtype=f32)
        self._seed(seed)

    init_parameters = policy_module.Policy.init_parameters

    def load_state_dict(self, state_dict):
        self.params = self.spec.pack(state_dict)

    def state_dict(self):
        return self.spec.unpack(self.params)

    def _own_state(self, n):
        if self._state is None or self._state.shape[2] != n:
            self._state = np.zeros(self.spec.state_shape(n), dtype=f32)
        return self._state

    def lstm_state(self):
        """A copy of the state float32 [2, 2, n, H] (None before the first call of a policy built without num_envs)."""
        return None if self._state is None else self._state.copy()

    def set_lstm_state(self, state):
        state = np.array(state, dtype=f32)
        if state.ndim != 4 or state.shape[:2] != (2, 2) or state.shape[3] != self.spec.lstm_hidden:
            raise ValueError(f"a state has shape (2, 2, n, {self.spec.lstm_hidden}), not {state.shape}")
        self._state = state

    def reset_state(self):
        if self._state is not None:
            self._state[...] = 0.0

    def act(self, obs, episode_starts, final_obs=None, deterministic=False, states=None):
        """(actions int64 [n], values, log_probs, final_values or None); the policy's own state advances in place, or --
        with states=(in, out), two float32 [2, 2, n, H] arrays -- `out` is written from `in` and the own state stays."""
        obs = np.asarray(obs, dtype=f32).reshape(-1, self.spec.obs_width)
        n = obs.shape[0]
        source, target = (self._own_state(n),) * 2 if states is None else states
        u = None if deterministic else self._generator.random(n)
        got = lstm_numpy(self.spec, self.params, obs, episode_starts, source, final_obs, u, deterministic)
        target[...] = got["state"]
        return got["actions"], got["values"], got["log_probs"], got["final_values"]

    def values(self, obs, episode_starts, final_obs=None):
        """V(obs) from the own state masked by episode_starts; with final_obs (V(obs), V(final_obs)).  The state stays."""
        obs = np.asarray(obs, dtype=f32).reshape(-1, self.spec.obs_width)
        got = lstm_numpy(self.spec, self.params, obs, episode_starts, self._own_state(obs.shape[0]), final_obs,
                         values_only=True)
        return got["values"] if final_obs is None else (got["values"], got["final_values"])


class DeviceLstmPolicy(policy_module.DevicePolicy):
    """The recurrent policy of a device-resident environment with a Discrete action space, over torch tensors on its GPU;
    used as LstmPolicy is and bit for bit equal to it.  Every act() / values() is ONE launch of lstm_forward_kernel
    (rf_lstm_forward) on torch's current stream; the state is one float32 [2, 2, n, H] tensor the policy owns and act()
    updates in place.  load_state_dict / state_dict are DevicePolicy's, under sb3-contrib's names: transposes and copies
    on the stream.  Nothing waits for the host."""

    def __init__(self, env, spec, seed=None):
        self._device_env(env)
        _refuse_box(env.single_action_space)
        if getattr(spec, "kind", None) != "lstm":
            raise TypeError(f"DeviceLstmPolicy needs an LstmPolicySpec, not {type(spec).__name__}")
        if env.single_action_space.n != spec.n_actions:
            raise ValueError(f"the spec has {spec.n_actions} actions, the environment {env.single_action_space.n}")
        self._attach(env, spec, seed)
        self.num_envs = int(env.num_envs)
        if not spec.enable_critic_lstm and self._ctx.lstm_critic_params_size(spec.critic_desc()) != spec.size:
            raise RuntimeError("rf_lstm_critic_params_size disagrees with the packed parameters")
        self._state = self._torch.zeros(spec.state_shape(self.num_envs), dtype=self._torch.float32, device=self.device)

    def _checked_state(self, state, what):
        torch = self._torch
        if not isinstance(state, torch.Tensor):
            raise TypeError(f"{what} must be a torch.Tensor on {self.device}, not {type(state).__name__}")
        self._io._on_device(state, what)
        want = self.spec.state_shape(self.num_envs)
        if state.dtype != torch.float32 or tuple(state.shape) != want or not state.is_contiguous():
            raise ValueError(f"{what} is {state.dtype} {tuple(state.shape)}, not contiguous torch.float32 {want}")
        return state

    def lstm_state(self):
        """A copy of the state, float32 [2, 2, n, H] on the device."""
        return self._state.clone()

    def set_lstm_state(self, state):
        """Copies `state` (a device tensor) into the policy's own, on the current stream."""
        self._state.copy_(self._checked_state(state, "state"))

    def reset_state(self):
        self._state.zero_()

    def _starts(self, episode_starts, n):
        torch = self._torch
        if not isinstance(episode_starts, torch.Tensor):
            raise TypeError(f"episode_starts must be a torch.Tensor on {self.device}, not {type(episode_starts).__name__}")
        self._io._on_device(episode_starts, "episode_starts")
        # (one byte per environment either way: step_tensors() returns `truncated` as torch.bool)
        if episode_starts.dtype not in (torch.uint8, torch.bool) or tuple(episode_starts.shape) != (n,) \
                or not episode_starts.is_contiguous():
            raise ValueError(f"episode_starts is {episode_starts.dtype} {tuple(episode_starts.shape)}, not contiguous "
                             f"torch.uint8 or torch.bool ({n},)")
        return episode_starts

    def _inputs(self, obs, episode_starts, final_obs):
        obs = self._rows(obs, "obs")
        if obs.shape[0] != self.num_envs:
            raise ValueError(f"obs has {obs.shape[0]} rows, the policy's state {self.num_envs} environments")
        if final_obs is not None and self._rows(final_obs, "final_obs").shape != obs.shape:
            raise ValueError(f"final_obs has shape {tuple(final_obs.shape)}, obs {tuple(obs.shape)}")
        return obs, self._starts(episode_starts, self.num_envs)

    def _forward(self, obs, episode_starts, final_obs, state_in, state_out, gen, flags, actions, log_probs, values,
                 final_values):
        self._interop.check_one_runtime()
        pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        # (enable_critic_lstm=False: the sibling entry point over rf_lstm_critic_desc, lstm_forward_kernel<false, true>)
        linear = not self.spec.enable_critic_lstm
        forward = self._ctx.lstm_critic_forward if linear else self._ctx.lstm_forward
        forward(self.spec.critic_desc() if linear else self.spec.desc(), self.params.data_ptr(), obs.shape[0], obs.data_ptr(),
                episode_starts.data_ptr(), pointer(final_obs), state_in.data_ptr(), pointer(state_out), gen, flags,
                pointer(actions), pointer(log_probs), pointer(values), pointer(final_values), None, self._io._stream())

    def act(self, obs, episode_starts, final_obs=None, deterministic=False, out=None, states=None):
        """(actions int64 [n], values, log_probs, final_values or None) of obs float32 [n, D], episode_starts uint8 or
        bool [n] (and final_obs as obs); out=(actions, values, log_probs, final_values or None) writes into the caller's rows.  The
        policy's own state advances in place; with states=(in, out), two device tensors float32 [2, 2, n, H], the call
        goes from `in` to `out` instead (the same tensor, or two that do not overlap) and the own state stays.  One
        launch; a sampled call advances the host generator by n."""
        torch = self._torch
        obs, episode_starts = self._inputs(obs, episode_starts, final_obs)
        n = self.num_envs
        if states is None:
            state_in = state_out = self._state
        else:
            state_in, state_out = states
            state_in, state_out = self._checked_state(state_in, "states[0]"), self._checked_state(state_out, "states[1]")
        given = (None,) * 4 if out is None else tuple(out)
        if len(given) != 4:
            raise TypeError("out must be (actions, values, log_probs, final_values or None)")
        actions = self._out("actions", given[0], n, torch.int64)
        values = self._out("values", given[1], n, torch.float32)
        log_probs = self._out("log_probs", given[2], n, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[3], n, torch.float32)
        gen = None if deterministic else policy_module.generator_words(self._bit_generator)
        self._forward(obs, episode_starts, final_obs, state_in, state_out, gen, DETERMINISTIC if deterministic else 0,
                      actions, log_probs, values, final_values)
        if not deterministic:
            self._bit_generator.advance(n)  # (after the call was taken: a refused call consumes nothing)
        return actions, values, log_probs, final_values

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
        self._forward(obs, episode_starts, final_obs, self._state, None, None, 0, None, None, values, final_values)
        return values if final_obs is None else (values, final_values)
