"""PPO's state-dependent-exploration actor-critic for ContinuousJumps-v0: stable-baselines3's
ActorCriticPolicy(use_sde=True) -- StateDependentNoiseDistribution with full_std=True, use_expln=False,
squash_output=False, learn_features=False, epsilon=1e-6 -- for the one-dimensional Box(-1, 1, (1,)), as the reference's
PPO configurations (examples/ppo_*.yml: use_sde, sde_sample_freq, log_std_init, net_arch=dict(pi=..., vf=...)) train it.

One definition of the arithmetic (include/reinfocus_hip.h, "sde policy"; the scalar functions are
csrc/rf_policy_math.h): sde_numpy and noise_numpy below are its numpy float32 restatement and the oracle;
sde_forward_kernel and sde_noise_kernel (csrc/rf_sde.h) compute the same bits in one launch each.  The update is
environments/learner.py's, which dispatches on the spec's kind.

    SdePolicySpec    the network of MlpPolicySpec with a pi head of one output (the mean) and log_std [L] packed last
    SdePolicy        the numpy twin: reset_noise / act / values over numpy arrays
    DeviceSdePolicy  the same methods over torch tensors on a device-resident environment's GPU

The exploration matrix theta [n, L] (one row per environment, even when n = 1) changes only in reset_noise(), which
consumes n * L draws of the host generator; act() consumes none.

torch is imported lazily, by DeviceSdePolicy only (reinfocus_amd/torch_interop.py says why import order matters).
"""

import numpy as np

from reinfocus_amd.environments import policy as policy_module
from reinfocus_amd.environments import spaces
from reinfocus_amd.environments.policy import _NAN, _net, activation, canonical, exp32, f32, linear, log32

EPSILON = f32(1e-6)
HALF_LOG_2PI, ENTROPY0 = f32(0.9189385332046727), f32(1.4189385332046727)
P_MIN, P_CENTRAL = f32(2.0 ** -54), f32(0.075)
LN2_HI64, LN2_LO64 = 6.93147180369123816490e-01, 1.90821492927058770002e-10
_LOG64 = tuple(2.0 / d for d in range(25, 1, -2))
# M. J. Wichura's AS 241 PPND16, leading coefficient first (the constant 1 of every denominator included)
_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4, 1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4, 5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0, 3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1, 6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2, 2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4, 1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def expw32(x):
    """rf_policy_math.h expw32: exp32(x) for x <= 0, else 1 / exp32(-x) (+inf for x > 87 and for NaN)."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(all="ignore"):
        down = x <= f32(0.0)
        out = np.where(down, exp32(np.where(down, x, f32(0.0))), f32(1.0) / exp32(np.where(down, f32(0.0), -x)))
    assert out.dtype == f32
    return out


def _horner(coefficients, x):
    """c + x * acc from the leading coefficient, in x's dtype (float64 for normal32)."""
    acc = np.full(x.shape, coefficients[0], dtype=x.dtype)
    for c in coefficients[1:]:
        acc = x.dtype.type(c) + x * acc
    return acc


def log64(s):
    """rf_policy_math.h log64: ln of positive normal float64, every operation a numpy float64 operation."""
    s = np.ascontiguousarray(s, dtype=np.float64)
    u = s.view(np.uint64)
    with np.errstate(all="ignore"):
        e = (u >> np.uint64(52)).astype(np.int64) - 1023
        m = ((u & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
        big = m > 1.4142135623730951
        m = np.where(big, m * 0.5, m)
        e = np.where(big, e + 1, e)
        f = m - 1.0
        q = f / (2.0 + f)
        z = q * q
        lnm = 2.0 * q + q * (z * _horner(_LOG64, z))
        ef = e.astype(np.float64)
        out = ef * LN2_HI64 + (lnm + ef * LN2_LO64)
    assert out.dtype == np.float64
    return out.reshape(s.shape)


def normal32_of_p(p, upper):
    """normal32 from the float32 argument p on (p = float32(u) or float32(1 - u), raised to 2^-54): float64 inside."""
    p = np.asarray(p, dtype=f32)
    wide = p.astype(np.float64)
    with np.errstate(all="ignore"):
        central = p >= P_CENTRAL
        q = np.where(upper, 0.5 - wide, wide - 0.5)
        r = 0.180625 - q * q
        middle = (q * _horner(_A, r)) / _horner(_B, r)
        r = np.sqrt(-log64(np.where(central, 0.01, wide)))
        near, far = r - 1.6, r - 5.0
        tail = np.where(r <= 5.0, _horner(_C, near) / _horner(_D, near), _horner(_E, far) / _horner(_F, far))
        out = np.where(central, middle, np.where(upper, tail, -tail)).astype(f32)
    return out


def normal32(u):
    """rf_policy_math.h normal32: the inverse normal CDF of draws u (float64, j * 2^-53), float32."""
    u = np.asarray(u, dtype=np.float64)
    upper = u >= 0.5
    p = np.where(upper, 1.0 - u, u).astype(f32)
    return normal32_of_p(np.where(p < P_MIN, P_MIN, p), upper)


def std2_of(log_std):
    std = expw32(log_std)
    return std * std


def noise_numpy(log_std, u):
    """theta [n, L] of the draws u float64 [n * L] (draw e * L + k for environment e, unit k)."""
    log_std = np.asarray(log_std, dtype=f32)
    with np.errstate(all="ignore"):
        return canonical(normal32(u).reshape(-1, log_std.size) * expw32(log_std)[None, :])


def sigma_of(h, std2):
    var = np.zeros(h.shape[0], dtype=f32)
    with np.errstate(all="ignore"):
        for k in range(h.shape[1]):
            var = var + (h[:, k] * h[:, k]) * std2[k]
        out = np.sqrt(var + EPSILON)
    assert out.dtype == f32
    return out


def log_prob_of(a, mu, sigma):
    with np.errstate(all="ignore"):
        fine = np.isfinite(sigma)
        t = a - mu
        q = (t * t) / (f32(2.0) * (sigma * sigma))
        out = ((-q) - log32(np.where(fine, sigma, f32(1.0)))) - HALF_LOG_2PI
    return np.where(fine, canonical(out), _NAN)


def entropy_of(sigma):
    with np.errstate(all="ignore"):
        fine = np.isfinite(sigma)
        return np.where(fine, ENTROPY0 + log32(np.where(fine, sigma, f32(1.0))), _NAN)


def env_actions_of(a):
    with np.errstate(all="ignore"):
        return canonical(np.where(a < f32(-1.0), f32(-1.0), np.where(a > f32(1.0), f32(1.0), a)))


class SdePolicySpec(policy_module.MlpPolicySpec):
    """MlpPolicySpec with the Gaussian head: the pi head has one output (action_net: the mean), and SB3's log_std [L, 1]
    (L = the last pi width) is packed after everything MlpPolicySpec packs, whose offsets do not move."""

    kind = "sde"
    MIN_ACTIONS = 1

    def __init__(self, obs_width, pi=(64, 64), vf=(64, 64), activation="tanh", log_std_init=0.0):
        super().__init__(obs_width, 1, pi, vf, activation)
        self.log_std_init = float(log_std_init)
        self.log_std_at, self.latent = self.size, self.pi[-1]
        self.entries.append(("log_std", self.size, (1, self.latent), True))  # (SB3's [L, 1] is this, transposed)
        self.size += self.latent

    def initial(self):
        params = np.zeros(self.size, dtype=f32)
        params[self.log_std_at:] = f32(self.log_std_init)
        return params


def sde_numpy(spec, params, obs, final_obs=None, theta=None, deterministic=False, values_only=False):
    """The definition, literally.  obs float32 [n, D], final_obs alike or None, theta float32 [n, L] (a sampled call).
    Returns a dict: "actions" (raw), "env_actions" (clamped), "log_probs", "mean", "sigma" float32 [n] (None with
    values_only), "values" float32 [n], "final_values" float32 [n] or None."""
    obs = np.asarray(obs, dtype=f32).reshape(-1, spec.obs_width)
    params = np.asarray(params, dtype=f32).reshape(spec.size)
    pi, vf = spec.nets(params)
    out = dict.fromkeys(("actions", "env_actions", "log_probs", "mean", "sigma", "final_values"))
    out["values"] = canonical(_net(spec, vf, obs)[:, 0])
    if final_obs is not None:
        final_obs = np.asarray(final_obs, dtype=f32).reshape(obs.shape)
        lead = final_obs[:, 0]
        out["final_values"] = np.where(lead != lead, _NAN, canonical(_net(spec, vf, final_obs)[:, 0]))
    if values_only:
        return out
    h = obs
    for weight_t, bias in pi[0]:
        h = activation(linear(h, weight_t, bias), spec.activation)
    mu = linear(h, *pi[1])[:, 0]
    sigma = sigma_of(h, std2_of(params[spec.log_std_at:]))
    a = mu
    if not deterministic:
        if theta is None:
            raise ValueError("a sampled call needs theta: reset_noise() first")
        theta = np.asarray(theta, dtype=f32).reshape(obs.shape[0], spec.latent)
        with np.errstate(all="ignore"):
            a = mu + _rowdot(h, theta)
    out["actions"], out["env_actions"] = canonical(a), env_actions_of(a)
    out["log_probs"], out["mean"], out["sigma"] = log_prob_of(a, mu, sigma), canonical(mu), canonical(sigma)
    return out


def _rowdot(h, theta):
    """sum over k in index order, from +0, of h[:, k] * theta[:, k]."""
    y = np.zeros(h.shape[0], dtype=f32)
    with np.errstate(all="ignore"):
        for k in range(h.shape[1]):
            y = y + h[:, k] * theta[:, k]
    assert y.dtype == f32
    return y


def _refuse_discrete(action_space):
    if not (isinstance(action_space, spaces.Box) and tuple(action_space.shape) == (1,)):
        raise ValueError(f"the sde policy has a Gaussian head over a Box action space of one dimension, not "
                         f"{action_space!r}: Discrete action spaces have Policy / DevicePolicy, wider boxes are refused")


class SdePolicy(policy_module._Draws):
    """The numpy twin of DeviceSdePolicy, and its oracle.  Parameters start at zero with log_std at log_std_init."""

    def __init__(self, spec, seed=None, num_envs=1):
        if getattr(spec, "kind", None) != "sde":
            raise TypeError(f"SdePolicy needs an SdePolicySpec, not {type(spec).__name__}")
        self.spec = spec
        self.num_envs = int(num_envs)  # (how many rows reset_noise() draws; DeviceSdePolicy takes its environment's)
        self.params = spec.initial()
        self._theta = None
        self._seed(seed)

    init_parameters = policy_module.Policy.init_parameters

    def load_state_dict(self, state_dict):
        self.params = self.spec.pack(state_dict)

    def state_dict(self):
        return self.spec.unpack(self.params)

    def reset_noise(self, num_envs=None):
        """A new theta [num_envs, L] from the current log_std: num_envs * L draws."""
        if num_envs is not None:
            self.num_envs = int(num_envs)
        u = self._generator.random(self.num_envs * self.spec.latent)
        self._theta = noise_numpy(self.params[self.spec.log_std_at:], u)

    def noise(self):
        return None if self._theta is None else self._theta.copy()

    def set_noise(self, theta):
        self._theta = None if theta is None else np.array(theta, dtype=f32).reshape(-1, self.spec.latent)

    def act(self, obs, final_obs=None, deterministic=False):
        """(actions float32 [n] (raw), values, log_probs, final_values or None, env_actions float32 [n] (clamped))."""
        obs = np.asarray(obs, dtype=f32).reshape(-1, self.spec.obs_width)
        if not deterministic and (self._theta is None or self._theta.shape[0] != obs.shape[0]):
            raise ValueError(f"a sampled act() of {obs.shape[0]} environments needs reset_noise() for that many first")
        got = sde_numpy(self.spec, self.params, obs, final_obs, self._theta, deterministic)
        return got["actions"], got["values"], got["log_probs"], got["final_values"], got["env_actions"]

    def values(self, obs, final_obs=None):
        got = sde_numpy(self.spec, self.params, obs, final_obs, values_only=True)
        return got["values"] if final_obs is None else (got["values"], got["final_values"])


class DeviceSdePolicy(policy_module.DevicePolicy):
    """The sde policy of a device-resident environment with the Box(-1, 1, (1,)) action space
    (DeviceVectorContinuousJumps, or a DeviceVectorEnvironment with that space), over torch tensors on its GPU; used as
    SdePolicy is and bit for bit equal to it.  reset_noise() is one launch of sde_noise_kernel (rf_sde_noise_reset) into a
    [n, L] tensor the policy owns, every act() / values() one launch of sde_forward_kernel (rf_sde_forward), all on
    torch's current stream: nothing waits for the host."""

    def __init__(self, env, spec, seed=None):
        self._device_env(env)
        _refuse_discrete(env.single_action_space)
        if getattr(spec, "kind", None) != "sde":
            raise TypeError(f"DeviceSdePolicy needs an SdePolicySpec, not {type(spec).__name__}")
        self._attach(env, spec, seed)
        self.num_envs = int(env.num_envs)
        self.params.copy_(self._torch.from_numpy(spec.initial()))
        self._theta = None

    def reset_noise(self, num_envs=None):
        """A new theta [num_envs, L] (the environment's num_envs unless given) from the current log_std: one launch, and
        num_envs * L draws of the host generator."""
        torch = self._torch
        num_envs = self.num_envs if num_envs is None else int(num_envs)
        self._interop.check_one_runtime()
        if self._theta is None or self._theta.shape[0] != num_envs:
            self._theta = torch.zeros((num_envs, self.spec.latent), dtype=torch.float32, device=self.device)
        self._ctx.sde_noise_reset(self.spec.desc(), self.params.data_ptr(), num_envs,
                                  policy_module.generator_words(self._bit_generator), self._theta.data_ptr(),
                                  self._io._stream())
        self._bit_generator.advance(num_envs * self.spec.latent)  # (after the call was taken)

    def noise(self):
        return None if self._theta is None else self._theta.clone()

    def set_noise(self, theta):
        torch = self._torch
        if theta is None:
            self._theta = None
            return
        if not isinstance(theta, torch.Tensor) or theta.dtype != torch.float32 or theta.dim() != 2 \
                or theta.shape[1] != self.spec.latent:
            raise ValueError(f"theta must be a torch.float32 tensor (n, {self.spec.latent}) on {self.device}")
        self._io._on_device(theta, "theta")
        self._theta = theta.contiguous().clone()

    def _forward(self, obs, final_obs, theta, flags, actions, env_actions, log_probs, values, final_values):
        self._interop.check_one_runtime()
        pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        self._ctx.sde_forward(self.spec.desc(), self.params.data_ptr(), obs.shape[0], obs.data_ptr(), pointer(final_obs),
                              pointer(theta), flags, pointer(actions), pointer(env_actions), pointer(log_probs),
                              pointer(values), pointer(final_values), None, None, self._io._stream())

    def act(self, obs, final_obs=None, deterministic=False, out=None):
        """(actions float32 [n] (raw), values, log_probs, final_values or None, env_actions float32 [n] (clamped)) of obs
        float32 [n, D]; out=(actions, values, log_probs, final_values or None, env_actions) writes into the caller's rows.
        One launch; no draw is consumed."""
        torch = self._torch
        obs = self._rows(obs, "obs")
        n = obs.shape[0]
        if final_obs is not None and self._rows(final_obs, "final_obs").shape != obs.shape:
            raise ValueError(f"final_obs has shape {tuple(final_obs.shape)}, obs {tuple(obs.shape)}")
        if not deterministic and (self._theta is None or self._theta.shape[0] != n):
            raise ValueError(f"a sampled act() of {n} environments needs reset_noise() for that many first")
        given = (None,) * 5 if out is None else tuple(out)
        if len(given) != 5:
            raise TypeError("out must be (actions, values, log_probs, final_values or None, env_actions)")
        actions = self._out("raw_actions", given[0], n, torch.float32)
        values = self._out("values", given[1], n, torch.float32)
        log_probs = self._out("log_probs", given[2], n, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[3], n, torch.float32)
        env_actions = self._out("env_actions", given[4], n, torch.float32)
        self._forward(obs, final_obs, None if deterministic else self._theta,
                      policy_module.DETERMINISTIC if deterministic else 0, actions, env_actions, log_probs, values,
                      final_values)
        return actions, values, log_probs, final_values, env_actions

    def values(self, obs, final_obs=None, out=None):
        """V(obs); with final_obs (V(obs), V(final_obs)).  out=(values, final_values or None).  One launch, no draw."""
        torch = self._torch
        obs = self._rows(obs, "obs")
        n = obs.shape[0]
        if final_obs is not None and self._rows(final_obs, "final_obs").shape != obs.shape:
            raise ValueError(f"final_obs has shape {tuple(final_obs.shape)}, obs {tuple(obs.shape)}")
        given = (None, None) if out is None else tuple(out)
        if len(given) != 2:
            raise TypeError("out must be (values, final_values or None)")
        values = self._out("last_values", given[0], n, torch.float32)
        final_values = None if final_obs is None else self._out("final_values", given[1], n, torch.float32)
        self._forward(obs, final_obs, None, 0, None, None, None, values, final_values)
        return values if final_obs is None else (values, final_values)
