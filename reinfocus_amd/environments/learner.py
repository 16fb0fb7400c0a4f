"""PPO's minibatch update for the actor-critic of environments/policy.py: stable-baselines3's PPO.train() -- the clipped
surrogate loss, the value loss and the entropy bonus, their gradient, clip_grad_norm_ and one Adam step per minibatch --
the stage of training after a rollout's flat().

One definition of the arithmetic (include/reinfocus_hip.h, "ppo update"; the scalar functions are csrc/rf_ppo.h):
ppo_update_numpy below is its numpy restatement and the oracle; rf_ppo_update computes the same bits in three launches
(ppo_backward_kernel, ppo_gradient_kernel, ppo_adam_kernel) and updates the parameters in place.

    Hyper          the hyper-parameters of one update, in rf_ppo_desc's order
    Learner        the numpy twin over a policy.Policy and a rollout.Rollout
    DeviceLearner  the same methods over a policy.DevicePolicy and a rollout.DeviceRollout: every update is enqueued on
                   torch's current stream, the stats are rows of one device tensor, nothing waits for the host

The optimizer state is one packed float32 vector, as on the device: 8 floats of header (step int64, bc1 and bc2 float64
-- the running 1 - beta^step --, a zero word), then m [P] and v [P].  All zero is a fresh optimizer.

Both heads: the Categorical one of policy.py (ppo_gradient_numpy, rf_ppo_update) and the Gaussian one of sde.py
(sde_gradient_numpy, rf_sde_update: "sde policy" in the header); every function and class here dispatches on the spec's
kind, and a spec of P + L parameters gives an optimizer state of that many.

torch is imported lazily, by DeviceLearner only (reinfocus_amd/torch_interop.py says why import order matters).
"""

import collections

import numpy as np

from reinfocus_amd.environments import policy as policy_module
from reinfocus_amd.environments.policy import _NAN, activation, canonical, exp32, f32, linear, log32, softmax_parts

MAX_BATCH = 1024  # RF_PPO_MAX_BATCH
INVALID, NONFINITE = 1, 2  # RF_PPO_INVALID, RF_PPO_NONFINITE
STATE_HEADER = 8  # floats before m
STATS = ("pg_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "grad_norm", "loss", "flags")
BATCH_KEYS = ("observations", "actions", "log_probs", "advantages", "returns")  # what an update reads of flat()

Hyper = collections.namedtuple("Hyper", ("learning_rate", "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "beta1",
                                         "beta2", "adam_eps", "normalize_advantage"))
f64 = np.float64


def checked_hyper(hyper):
    """hyper as a Hyper of Python floats and a 0 / 1; ValueError for what rf_ppo_update refuses."""
    hyper = Hyper(*hyper)
    values = [float(v) for v in hyper[:8]]
    if not all(np.isfinite(v) and v >= 0.0 for v in values):
        raise ValueError(f"a hyper-parameter is negative or not finite: {hyper}")
    if not (values[5] < 1.0 and values[6] < 1.0):
        raise ValueError(f"betas {values[5]}, {values[6]} are not in [0, 1)")
    return Hyper(*values, 1 if hyper.normalize_advantage else 0)


def fresh_state(spec):
    return np.zeros(STATE_HEADER + 2 * spec.size, dtype=f32)


def state_parts(spec, state):
    """(step int, bc1, bc2 float64, m, v float32 views) of a packed optimizer state."""
    state = np.asarray(state, dtype=f32).reshape(STATE_HEADER + 2 * spec.size)
    head = state[:STATE_HEADER]
    return (int(head.view(np.int64)[0]), head.view(f64)[1], head.view(f64)[2], state[STATE_HEADER:STATE_HEADER + spec.size],
            state[STATE_HEADER + spec.size:])


def pack_state(spec, step, bc1, bc2, m, v):
    state = fresh_state(spec)
    state[:STATE_HEADER].view(np.int64)[0] = step
    state[:STATE_HEADER].view(f64)[1:3] = (bc1, bc2)
    state[STATE_HEADER:STATE_HEADER + spec.size] = m
    state[STATE_HEADER + spec.size:] = v
    return state


def _forward(spec, net, x):
    """([input, h0, (h1)], head output) of one net."""
    layers, last = net
    acts = [x]
    for weight_t, bias in layers:
        acts.append(activation(linear(acts[-1], weight_t, bias), spec.activation))
    return acts, linear(acts[-1], *last)


def _back(spec, weight_t, delta_out, h):
    """delta_in [B, K] of delta_out [B, O] through weight_t [K, O] and the activation whose output is h [B, K]."""
    acc = np.zeros(h.shape, dtype=f32)
    for o in range(weight_t.shape[1]):
        acc = acc + weight_t[:, o][None, :] * delta_out[:, o:o + 1]
    prime = f32(1.0) - h * h if spec.activation == "tanh" else np.where(h > f32(0.0), f32(1.0), f32(0.0))
    out = prime * acc
    assert out.dtype == f32
    return out


def _net_gradient(spec, net, acts, delta_head):
    """The packed gradient pieces of one net, in packing order: dW0, db0, (dW1, db1,) dW_head, db_head."""
    layers, last = net
    matrices = [weight_t for weight_t, _ in layers] + [last[0]]
    deltas = [None] * len(layers) + [delta_head]
    for layer in range(len(layers) - 1, -1, -1):
        deltas[layer] = _back(spec, matrices[layer + 1], deltas[layer + 1], acts[layer + 1])
    pieces = []
    for x, delta in zip(acts, deltas):
        weight = np.zeros((x.shape[1], delta.shape[1]), dtype=f32)
        bias = np.zeros(delta.shape[1], dtype=f32)
        for b in range(x.shape[0]):
            weight = weight + x[b][:, None] * delta[b][None, :]
            bias = bias + delta[b]
        pieces += [weight.reshape(-1), bias]
    return pieces


def _surrogate(d, adv, c):
    """Definition steps 4 and 5 from d on: (pg, kl, clipped, g)."""
    down = d <= f32(0.0)
    ratio = np.where(down, exp32(np.where(down, d, f32(0.0))), f32(1.0) / exp32(np.where(down, f32(0.0), -d)))
    lo, hi = f32(1.0) - c, f32(1.0) + c
    cl = np.where(ratio < lo, lo, np.where(ratio > hi, hi, ratio))
    surr1, surr2 = adv * ratio, adv * cl
    pg = -np.where(surr2 < surr1, surr2, surr1)
    r1 = ratio - f32(1.0)
    kl = r1 - d
    clipped = np.where(np.where(r1 < f32(0.0), -r1, r1) > c, f32(1.0), f32(0.0))
    g = np.where(((ratio >= lo) & (ratio <= hi)) | (surr1 < surr2), surr1, f32(0.0))
    return pg, kl, clipped, g


def _normalised(adv, hyper, count):
    """Definition step 2."""
    from reinfocus_amd.environments.harness import treesum

    if not (hyper.normalize_advantage and count > 1):
        return adv
    wide = adv.astype(f64)
    mean = treesum(wide) / f64(count)
    var = treesum((wide - mean) * (wide - mean)) / f64(count - 1)
    return ((wide - mean) / (np.sqrt(var) + f64(1e-8))).astype(f32)


def sde_gradient_numpy(spec, params, batch, index, hyper):
    """ppo_gradient_numpy for the Gaussian head ("sde policy" steps 1', 3', 5', 6', 7'): the packed gradient has P + L
    entries, log_std's last; batch["actions"] are the raw float32 actions."""
    from reinfocus_amd.environments import sde

    hyper = checked_hyper(hyper)
    obs = np.asarray(batch["observations"], dtype=f32).reshape(-1, spec.obs_width)
    rows_total = obs.shape[0]
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    count = index.size
    if not 1 <= count <= MAX_BATCH:
        raise ValueError(f"a minibatch of {count} samples is not in 1 .. {MAX_BATCH}")
    rows = np.clip(index, 0, rows_total - 1)
    if np.asarray(batch["actions"]).dtype.kind in "iub":  # (as DeviceLearner refuses it: no silent cast of indices)
        raise ValueError("the update has a Gaussian head over float32 raw actions, not an int64 action slab: Discrete "
                         "action spaces have Policy")
    a = np.asarray(batch["actions"], dtype=f32).reshape(rows_total)[rows]
    invalid = bool((rows != index).any() or (a != a).any())
    adv = np.asarray(batch["advantages"], dtype=f32).reshape(rows_total)[rows]
    old = np.asarray(batch["log_probs"], dtype=f32).reshape(rows_total)[rows]
    ret = np.asarray(batch["returns"], dtype=f32).reshape(rows_total)[rows]
    x = obs[rows]
    params = np.asarray(params, dtype=f32).reshape(spec.size)
    with np.errstate(all="ignore"):
        adv = _normalised(adv, hyper, count)
        pi, vf = spec.nets(params)
        pi_acts, mean = _forward(spec, pi, x)
        vf_acts, value = _forward(spec, vf, x)
        mu, v, h = mean[:, 0], value[:, 0], pi_acts[-1]
        std2 = sde.std2_of(params[spec.log_std_at:])
        sigma = sde.sigma_of(h, std2)
        logp = sde.log_prob_of(a, mu, sigma)
        entropy = sde.entropy_of(sigma)
        c, ec, vc = f32(hyper.clip_range), f32(hyper.ent_coef), f32(hyper.vf_coef)
        pg, kl, clipped, g = _surrogate(logp - old, adv, c)
        t = ret - v
        vl = t * t
        count_f = f32(count)
        ng, t, v2 = -g, a - mu, sigma * sigma
        fine = np.isfinite(sigma) & np.isfinite(logp)
        dmu = np.where(fine, (ng * (t / v2)) / count_f, _NAN)
        dsig = np.where(fine, (((ng * ((t * t) / (v2 * sigma) - f32(1.0) / sigma)) - ec / sigma) / count_f) / sigma, _NAN)
        dv = ((vc * f32(2.0)) * (v - ret)) / count_f
        dlog_std = np.zeros(spec.latent, dtype=f32)
        for b in range(count):
            dlog_std = dlog_std + ((h[b] * h[b]) * std2) * dsig[b]
        pieces = _net_gradient(spec, pi, pi_acts, dmu[:, None]) + _net_gradient(spec, vf, vf_acts, dv[:, None]) + [dlog_std]
    grad = np.concatenate(pieces)
    terms = np.stack([pg, vl, entropy, kl, clipped]).astype(f32)
    assert grad.dtype == f32 and grad.size == spec.size and terms.dtype == f32
    return grad, terms, invalid


def gradient_numpy(spec, params, batch, index, hyper):
    """The head's definition steps 1 to 7."""
    return (sde_gradient_numpy if spec.kind == "sde" else ppo_gradient_numpy)(spec, params, batch, index, hyper)


def ppo_gradient_numpy(spec, params, batch, index, hyper):
    """Definition steps 1 to 7: (packed gradient float32 [P], the five loss terms float32 [5, B], invalid bool)."""
    hyper = checked_hyper(hyper)
    obs = np.asarray(batch["observations"], dtype=f32).reshape(-1, spec.obs_width)
    rows_total = obs.shape[0]
    index = np.asarray(index, dtype=np.int64).reshape(-1)
    count = index.size
    if not 1 <= count <= MAX_BATCH:
        raise ValueError(f"a minibatch of {count} samples is not in 1 .. {MAX_BATCH}")
    rows = np.clip(index, 0, rows_total - 1)
    raw_actions = np.asarray(batch["actions"], dtype=np.int64).reshape(rows_total)[rows]
    a = np.clip(raw_actions, 0, spec.n_actions - 1)
    invalid = bool((rows != index).any() or (a != raw_actions).any())
    adv = np.asarray(batch["advantages"], dtype=f32).reshape(rows_total)[rows]
    old = np.asarray(batch["log_probs"], dtype=f32).reshape(rows_total)[rows]
    ret = np.asarray(batch["returns"], dtype=f32).reshape(rows_total)[rows]
    x = obs[rows]
    with np.errstate(all="ignore"):
        adv = _normalised(adv, hyper, count)
        pi, vf = spec.nets(params)
        pi_acts, logits = _forward(spec, pi, x)
        vf_acts, value = _forward(spec, vf, x)
        v = value[:, 0]
        _, z, _, s, degenerate = softmax_parts(logits)
        e = exp32(z)
        lse = np.where(degenerate, _NAN, log32(np.where(degenerate, f32(1.0), s)))
        logp = z - lse[:, None]
        p = e / s[:, None]
        acc = np.zeros(count, dtype=f32)
        for i in range(spec.n_actions):
            acc = acc + np.where(e[:, i] == f32(0.0), f32(0.0), p[:, i] * logp[:, i])
        entropy = -acc
        every = np.arange(count)
        c, ec, vc = f32(hyper.clip_range), f32(hyper.ent_coef), f32(hyper.vf_coef)
        pg, kl, clipped, g = _surrogate(logp[every, a] - old, adv, c)
        t = ret - v
        vl = t * t
        count_f = f32(count)
        onehot = np.zeros((count, spec.n_actions), dtype=f32)
        onehot[every, a] = f32(1.0)
        pull = (-g)[:, None] * (onehot - p)
        ent = np.where(e == f32(0.0), f32(0.0), (ec * p) * (logp + entropy[:, None]))
        dlogit = (pull + ent) / count_f
        dv = ((vc * f32(2.0)) * (v - ret)) / count_f
        pieces = _net_gradient(spec, pi, pi_acts, dlogit) + _net_gradient(spec, vf, vf_acts, dv[:, None])
    grad = np.concatenate(pieces)
    terms = np.stack([pg, vl, entropy, kl, clipped])
    assert grad.dtype == f32 and grad.size == spec.size and terms.dtype == f32
    return grad, terms, invalid


def ppo_update_numpy(spec, params, state, batch, index, hyper):
    """The definition, literally.  params float32 [P] and state (the packed optimizer state) are not modified; batch: a
    dict with flat()'s keys (observations, actions, log_probs, advantages, returns; N rows each); index int64 [B]; hyper:
    a Hyper.  Returns (new params, new state, stats float32 [8])."""
    from reinfocus_amd.environments.harness import treesum

    hyper = checked_hyper(hyper)
    params = np.asarray(params, dtype=f32).reshape(spec.size)
    grad, terms, invalid = gradient_numpy(spec, params, batch, index, hyper)
    count = terms.shape[1]
    step, bc1, bc2, m, v = state_parts(spec, state)
    with np.errstate(all="ignore"):
        wide = grad.astype(f64)
        norm = np.sqrt(treesum(wide * wide))
        flags = INVALID if invalid else (0 if np.isfinite(norm) else NONFINITE)
        stats = np.zeros(8, dtype=f32)
        for i in range(5):
            stats[i] = canonical(f32(treesum(terms[i]) / f64(count)))
        stats[5] = canonical(f32(norm))
        stats[6] = canonical((stats[0] + f32(hyper.ent_coef) * (-stats[2])) + f32(hyper.vf_coef) * stats[1])
        stats[7] = f32(flags)
        if flags:
            return params.copy(), np.array(state, dtype=f32, copy=True).reshape(-1), stats
        q = f64(hyper.max_grad_norm) / (norm + f64(1e-6))
        coef = f32(q if q < 1.0 else 1.0)
        b1, ob1 = f32(hyper.beta1), f32(f64(1.0) - f64(hyper.beta1))
        b2, ob2 = f32(hyper.beta2), f32(f64(1.0) - f64(hyper.beta2))
        bc1 = f64(1.0) - f64(hyper.beta1) * (f64(1.0) - bc1)
        bc2 = f64(1.0) - f64(hyper.beta2) * (f64(1.0) - bc2)
        g = grad * coef
        m = b1 * m + ob1 * g
        v = b2 * v + ob2 * (g * g)
        denom = np.sqrt(v) / f32(np.sqrt(bc2)) + f32(hyper.adam_eps)
        new = params - f32(f64(hyper.learning_rate) / bc1) * (m / denom)
    assert new.dtype == f32 and m.dtype == f32 and v.dtype == f32
    return new, pack_state(spec, step + 1, bc1, bc2, m, v), stats


class _Hyper:
    """The hyper-parameters as plain attributes, which may be changed between calls (a schedule costs nothing: they
    travel by value with every update)."""

    def _configure(self, learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, normalize_advantage, betas, adam_eps):
        self.learning_rate, self.clip_range, self.ent_coef, self.vf_coef = learning_rate, clip_range, ent_coef, vf_coef
        self.max_grad_norm, self.normalize_advantage, self.betas, self.adam_eps = (max_grad_norm, normalize_advantage,
                                                                                   tuple(betas), adam_eps)
        self.hyper()

    def hyper(self):
        return checked_hyper((self.learning_rate, self.clip_range, self.ent_coef, self.vf_coef, self.max_grad_norm,
                              self.betas[0], self.betas[1], self.adam_eps, self.normalize_advantage))

    @staticmethod
    def _batches(total, n_epochs, batch_size):
        n_epochs, batch_size = int(n_epochs), int(batch_size)
        if n_epochs < 1 or not 1 <= batch_size <= MAX_BATCH:
            raise ValueError(f"n_epochs {n_epochs} must be at least 1 and batch_size {batch_size} in 1 .. {MAX_BATCH}")
        return n_epochs, batch_size, -(-total // batch_size)

    def _refuse_rollout(self, rollout):
        if self.spec.kind == "sde":
            from reinfocus_amd.environments import sde

            sde._refuse_discrete(rollout.env.single_action_space)
        else:
            policy_module._refuse_box(rollout.env.single_action_space)


class Learner(_Hyper):
    """The numpy twin of DeviceLearner, and its oracle: updates policy.params (a policy.Policy's) in place."""

    def __init__(self, policy, learning_rate=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 normalize_advantage=True, betas=(0.9, 0.999), adam_eps=1e-5):
        from reinfocus_amd.environments import sde

        if not isinstance(policy, (policy_module.Policy, sde.SdePolicy)):
            raise TypeError(f"Learner needs a Policy or an SdePolicy, not {type(policy).__name__} (a DevicePolicy has "
                            "DeviceLearner)")
        self.policy, self.spec = policy, policy.spec
        self._configure(learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, normalize_advantage, betas, adam_eps)
        self.state = fresh_state(self.spec)

    def update(self, flat, index):
        """One minibatch update from rows `index` of flat() (a dict of arrays); returns the stats float32 [8]."""
        params, self.state, stats = ppo_update_numpy(self.spec, self.policy.params, self.state, flat, index, self.hyper())
        self.policy.params[:] = params
        return stats

    def train(self, rollout, n_epochs, batch_size, permutations=None, generator=None):
        """n_epochs passes over a finished rollout in minibatches of batch_size (the last one may be shorter): stats
        float32 [n_epochs * ceil(N / batch_size), 8].  Per epoch one permutation: row e of permutations (int64
        [n_epochs, N]) if given, else generator.permutation(N) (generator: a numpy.random.Generator)."""
        self._refuse_rollout(rollout)
        flat = rollout.flat()
        total = flat["actions"].shape[0]
        n_epochs, batch_size, per_epoch = self._batches(total, n_epochs, batch_size)
        if permutations is not None:
            permutations = np.asarray(permutations, dtype=np.int64).reshape(n_epochs, total)
        elif generator is None:
            generator = np.random.default_rng()
        stats = np.zeros((n_epochs * per_epoch, 8), dtype=f32)
        for epoch in range(n_epochs):
            order = permutations[epoch] if permutations is not None else generator.permutation(total).astype(np.int64)
            for i in range(per_epoch):
                stats[epoch * per_epoch + i] = self.update(flat, order[i * batch_size:(i + 1) * batch_size])
        return stats

    def state_dict(self):
        """The optimizer: step, the running bias corrections bc1 / bc2 (1 - beta^step) and copies of m and v."""
        step, bc1, bc2, m, v = state_parts(self.spec, self.state)
        return {"step": step, "bc1": float(bc1), "bc2": float(bc2), "m": m.copy(), "v": v.copy()}

    def load_state_dict(self, state):
        self.state = pack_state(self.spec, int(state["step"]), float(state["bc1"]), float(state["bc2"]),
                                np.asarray(state["m"], dtype=f32).reshape(self.spec.size),
                                np.asarray(state["v"], dtype=f32).reshape(self.spec.size))


class DeviceLearner(_Hyper):
    """The learner of a policy.DevicePolicy, over torch tensors on its GPU; used as Learner is and bit for bit equal to
    it.  update() is rf_ppo_update: three launches on torch's current stream, which change policy.params in place -- the
    next collect() on the same stream sees them, no load_state_dict is needed.  train() enqueues every update of every
    epoch back to back; the index of each is a view of the epoch's permutation and the stats are rows of one device
    tensor.  No method synchronises the host (state_dict() reads the step and does)."""

    def __init__(self, policy, learning_rate=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5,
                 normalize_advantage=True, betas=(0.9, 0.999), adam_eps=1e-5):
        if not isinstance(policy, policy_module.DevicePolicy):  # (DeviceSdePolicy is one)
            raise TypeError(f"DeviceLearner needs a DevicePolicy or a DeviceSdePolicy, not {type(policy).__name__} (a "
                            "Policy has Learner)")
        self.policy, self.spec = policy, policy.spec
        self._sde = self.spec.kind == "sde"
        self._configure(learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, normalize_advantage, betas, adam_eps)
        self._torch, self._interop, self._io, self._ctx = policy._torch, policy._interop, policy._io, policy._ctx
        self.device = policy.device
        torch = self._torch
        state_size = self._ctx.sde_state_size if self._sde else self._ctx.ppo_state_size
        if state_size(self.spec.desc()) != 4 * (STATE_HEADER + 2 * self.spec.size):
            raise RuntimeError("rf_ppo_state_size / rf_sde_state_size disagrees with the packed optimizer state")
        self.state = torch.zeros(STATE_HEADER + 2 * self.spec.size, dtype=torch.float32, device=self.device)
        self._workspace, self._workspace_batch = None, 0
        self._stats = None

    def _checked(self, flat, index):
        torch = self._torch
        wanted = {"observations": torch.float32, "actions": torch.float32 if self._sde else torch.int64,
                  "log_probs": torch.float32, "advantages": torch.float32, "returns": torch.float32}
        if self._sde and isinstance(flat.get("actions"), torch.Tensor) and flat["actions"].dtype == torch.int64:
            raise ValueError("the update has a Gaussian head over float32 raw actions, not an int64 action slab: Discrete "
                             "action spaces have DevicePolicy")
        if not self._sde and isinstance(flat.get("actions"), torch.Tensor) and flat["actions"].dtype == torch.float32:
            raise ValueError("the update has a Categorical head over int64 actions, not a float32 action slab: continuous "
                             "action spaces (the reference trains ContinuousJumps with gSDE) are out of scope")
        total = None
        for key, dtype in wanted.items():
            tensor = flat[key]
            if not isinstance(tensor, torch.Tensor):
                raise TypeError(f"{key} must be a torch.Tensor on {self.device}, not {type(tensor).__name__}")
            self._io._on_device(tensor, key)
            shape = (tensor.shape[0], self.spec.obs_width) if key == "observations" else (tensor.shape[0],)
            if tensor.dtype != dtype or tuple(tensor.shape) != shape or not tensor.is_contiguous():
                raise ValueError(f"{key} is {tensor.dtype} {tuple(tensor.shape)}, not contiguous {dtype} {shape}")
            if total is not None and tensor.shape[0] != total:
                raise ValueError(f"{key} has {tensor.shape[0]} rows, the others {total}")
            total = tensor.shape[0]
        if not isinstance(index, torch.Tensor):
            raise TypeError(f"index must be a torch.Tensor on {self.device}, not {type(index).__name__}")
        self._io._on_device(index, "index")
        if index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous() or not 1 <= index.numel() <= MAX_BATCH:
            raise ValueError(f"index is {index.dtype} {tuple(index.shape)}, not contiguous torch.int64 (1 .. {MAX_BATCH},)")
        return total

    def _room(self, batch):
        if batch > self._workspace_batch:
            size = (self._ctx.sde_workspace_size if self._sde else self._ctx.ppo_workspace_size)(self.spec.desc(), batch)
            if size == 0:
                raise RuntimeError(f"rf_ppo_workspace_size refuses a minibatch of {batch}")
            self._workspace = self._torch.zeros(size // 4, dtype=self._torch.float32, device=self.device)
            self._workspace_batch = batch

    def _enqueue(self, flat, total, index, stats, hyper):
        update = self._ctx.sde_update if self._sde else self._ctx.ppo_update
        update(self.spec.desc(), hyper, self.policy.params.data_ptr(), self.state.data_ptr(), self._workspace.data_ptr(),
               total, flat["observations"].data_ptr(), flat["actions"].data_ptr(), flat["log_probs"].data_ptr(),
               flat["advantages"].data_ptr(), flat["returns"].data_ptr(), index.numel(), index.data_ptr(),
               stats.data_ptr(), self._io._stream())

    def update(self, flat, index):
        """One minibatch update from rows `index` (int64 device tensor) of flat() (a dict of device tensors); returns
        the stats, a float32 [8] tensor the learner owns and the next update() overwrites."""
        total = self._checked(flat, index)
        self._interop.check_one_runtime()
        self._room(index.numel())
        if self._stats is None:
            self._stats = self._torch.zeros(8, dtype=self._torch.float32, device=self.device)
        self._enqueue(flat, total, index, self._stats, self.hyper())
        return self._stats

    def train(self, rollout, n_epochs, batch_size, permutations=None, generator=None):
        """As Learner.train, over a finished DeviceRollout of the policy's GPU: permutations is an int64 device tensor
        [n_epochs, N], else one torch.randperm(N) on the device per epoch (generator: a torch.Generator of that device).
        Every update is enqueued back to back; returns the stats as one device tensor [n_epochs * ceil(N / batch_size), 8]
        that is complete when the stream reaches this point.  Nothing waits for the host."""
        torch = self._torch
        self._refuse_rollout(rollout)
        if getattr(rollout, "device", None) != self.device:
            raise ValueError(f"the rollout lives on {getattr(rollout, 'device', 'the host')}, the policy on {self.device}")
        flat = rollout.flat()
        total = flat["actions"].shape[0]
        n_epochs, batch_size, per_epoch = self._batches(total, n_epochs, batch_size)
        if permutations is not None:
            if not isinstance(permutations, torch.Tensor) or permutations.dtype != torch.int64 \
                    or tuple(permutations.shape) != (n_epochs, total) or not permutations.is_contiguous():
                raise ValueError(f"permutations must be a contiguous torch.int64 tensor ({n_epochs}, {total})")
            self._io._on_device(permutations, "permutations")
        self._checked(flat, (permutations[0] if permutations is not None
                             else torch.zeros(1, dtype=torch.int64, device=self.device))[:min(batch_size, total)])
        self._interop.check_one_runtime()
        self._room(min(batch_size, total))
        hyper = self.hyper()
        stats = torch.zeros((n_epochs * per_epoch, 8), dtype=torch.float32, device=self.device)
        for epoch in range(n_epochs):
            order = permutations[epoch] if permutations is not None else torch.randperm(total, device=self.device,
                                                                                        generator=generator)
            for i in range(per_epoch):
                self._enqueue(flat, total, order[i * batch_size:(i + 1) * batch_size], stats[epoch * per_epoch + i], hyper)
        return stats

    def state_dict(self):
        """The optimizer: step, bc1, bc2 (read from the device: this synchronises) and clones of m and v."""
        head = self.state[:STATE_HEADER].cpu().numpy()
        size = self.spec.size
        return {"step": int(head.view(np.int64)[0]), "bc1": float(head.view(f64)[1]), "bc2": float(head.view(f64)[2]),
                "m": self.state[STATE_HEADER:STATE_HEADER + size].clone(), "v": self.state[STATE_HEADER + size:].clone()}

    def load_state_dict(self, state):
        torch = self._torch
        size = self.spec.size
        for key in ("m", "v"):
            tensor = state[key]
            if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.float32 or tensor.numel() != size:
                raise ValueError(f"{key} must be a torch.float32 tensor of {size} elements on {self.device}")
            self._io._on_device(tensor, key)
        head = pack_state(self.spec, int(state["step"]), float(state["bc1"]), float(state["bc2"]), 0.0, 0.0)[:STATE_HEADER]
        self.state[:STATE_HEADER].copy_(torch.from_numpy(head.copy()))
        self.state[STATE_HEADER:STATE_HEADER + size].copy_(state["m"].reshape(size))
        self.state[STATE_HEADER + size:].copy_(state["v"].reshape(size))
