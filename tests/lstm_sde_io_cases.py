"""TEST INFRASTRUCTURE: what tests/test_lstm_sde_logic.py and tests/test_gpu_lstm_sde.py share -- the networks, the sizes,
hostile inputs, the chains of steps, the minibatch layouts, the numpy twins' results (computed once and shared), the
drivers of the end-to-end runs -- and the child process of the GPU file.

As tests/lstm_learner_io_cases.py: everything that needs torch and the library together runs in one fresh process that
imports torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.lstm_sde_io_cases <results.jsonl>
"""

import ctypes
import functools
import os
import sys

import numpy as np

from tests import learner_io_cases as learner_cases
from tests import lstm_io_cases as lstm_cases
from tests import lstm_learner_io_cases as lstm_learner_cases
from tests import policy_io_cases as policy_cases
from tests import rollout_io_cases as rollout_cases
from tests import sde_io_cases as sde_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = policy_cases.TILE
# (obs_width, lstm_hidden, pi, vf, activation): the least network; ppo_lstm_tuned.yml's MLPs on a small LSTM; sb3-contrib's
# default (ppo_lstm_untuned.yml's); widths that are no multiple of a wave, one and two layers mixed; every limit
NETWORKS = ((1, 1, (1,), (1,), "relu"),
            (4, 16, (64, 64), (64, 64), "relu"),
            (4, 256, (64, 64), (64, 64), "tanh"),
            (7, 65, (65,), (3, 200), "tanh"),
            (256, 256, (256, 256), (256,), "relu"))
SMALL, UNTUNED, LIMITS = 1, 2, 4
SIZES = (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
STEPS = lstm_cases.STEPS  # steps of a chain
OFFSETS, MODES, SEED, SENTINEL = policy_cases.OFFSETS, policy_cases.MODES, policy_cases.SEED, policy_cases.SENTINEL
PI_OUTPUTS = ("actions", "env_actions", "log_probs", "mean", "sigma")
OUTPUTS = sde_cases.FORWARD_OUTPUTS  # (rf_lstm_sde_forward's order)
UPDATES, SHIFTS = learner_cases.UPDATES, learner_cases.SHIFTS
LAYOUTS = lstm_learner_cases.LAYOUTS
ROWS = lstm_learner_cases.ROWS
starts_of = lstm_learner_cases.starts_of
bits, generator_at, hostile_rows = policy_cases.bits, policy_cases.generator_at, policy_cases.hostile_rows
hyper_of = learner_cases.hyper_of
same_runs = rollout_cases.same_runs


def sizes_of(index):
    return (1, TILE + 1) if index == LIMITS else SIZES


LIMIT_LAYOUTS = lstm_learner_cases.LIMIT_LAYOUTS


def layouts_of(index):
    return [name for name, layout in LAYOUTS.items() if name not in LIMIT_LAYOUTS and (index != LIMITS or layout[4] <= 2)]


def limit_layouts_of(index):
    """lstm_learner_io_cases.LIMIT_LAYOUTS under the Gaussian head: tuned, depth and untuned on the H = 16 network (8-row
    sequences; 1, 8, 9, 16 and 17 rows; more than 64 rows at B = 128); the 17-row sequence on the network with every limit."""
    if index == SMALL:
        return [name for name in LIMIT_LAYOUTS if name.split("/")[0] in ("tuned", "depth", "untuned") and name != "depth/0/17"]
    return ["depth/0/17"] if index == LIMITS else []


def spec_of(network, log_std_init=0.0):
    from reinfocus_amd.environments import lstm_sde

    width, hidden, pi, vf, activation = network
    return lstm_sde.LstmSdePolicySpec(width, lstm_hidden=hidden, pi=pi, vf=vf, activation=activation,
                                      log_std_init=log_std_init)


def state_dict(spec, seed, hostile=False):
    """tests/lstm_io_cases.py's weights (normal, scale 1 / sqrt(fan_in); biases of scale 0.1) with log_std uniform in
    [-1.5, 0.5]; hostile: as tests/sde_io_cases.py, its first rows are -100 (a standard deviation of 0), 0 and +3 (raw
    actions far past +-1) -- a single row is +3."""
    out = lstm_cases.state_dict(sde_cases._Entries(spec), seed)
    rng = np.random.default_rng(seed + 5000)
    log_std = rng.uniform(-1.5, 0.5, (spec.latent, 1)).astype(np.float32)
    if hostile:
        special = np.array([-100.0, 0.0, 3.0], dtype=np.float32)[-min(3, spec.latent):]
        log_std[:special.size, 0] = special
    out["log_std"] = log_std
    return out


# ---- the forward ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_inputs(index, n):
    """(spec, params, obs [STEPS, n, D], final_obs alike, starts uint8 [STEPS, n], state [2, 2, n, H]): the hostile rows,
    start bytes (0, 1, 2, 255) and states of tests/lstm_io_cases.py."""
    network = NETWORKS[index]
    spec = spec_of(network)
    params = spec.pack(state_dict(spec, 100 + index, hostile=True))
    obs = np.stack([hostile_rows(network[0], n, 1000 * index + n + 31 * s, False) for s in range(STEPS)])
    final_obs = np.stack([hostile_rows(network[0], n, 7 + n + 17 * s, True) for s in range(STEPS)])
    return (spec, params, obs, final_obs, lstm_cases.hostile_starts(n, STEPS, 50 * index + n),
            lstm_cases.hostile_state(spec, n, 9 * index + n))


@functools.lru_cache(maxsize=None)
def wanted_theta(index, n, offset):
    from reinfocus_amd.environments import sde

    spec, params = chain_inputs(index, n)[:2]
    return sde.noise_numpy(params[spec.log_std_at:], generator_at(offset)[1].random(n * spec.latent))


@functools.lru_cache(maxsize=None)
def wanted_chain(index, n, mode, offset):
    """The twin's STEPS results from chain_inputs (each the dict of lstm_sde_numpy), each step from the state of the one
    before, all with the theta of one reset `offset` draws in.  Computed once, shared, never changed."""
    from reinfocus_amd.environments import lstm_sde

    spec, params, obs, final_obs, starts, state = chain_inputs(index, n)
    theta = wanted_theta(index, n, offset) if mode == "sampled" else None
    steps = []
    for s in range(STEPS):
        steps.append(lstm_sde.lstm_sde_numpy(spec, params, obs[s], starts[s], state, final_obs[s], theta,
                                             mode == "deterministic"))
        state = steps[-1]["state"]
    return steps


# ---- the update ----------------------------------------------------------------------------------------------------------
def own_head(spec, params, batch, starts, states, n_steps, num_envs):
    """(mu, sigma, h) of every row of flat()'s order, by the twin's own forward over the whole rollout as one minibatch."""
    from reinfocus_amd.environments import lstm_learner, policy, sde

    total = n_steps * num_envs
    rows = lstm_learner.sequence_rows(starts, n_steps, num_envs, 0, total)
    lstm, layers, last = spec.nets(params)[0]
    with np.errstate(all="ignore"):
        h = lstm_learner._cell_rows(batch["observations"], rows, (states[:, 0, 0], states[:, 0, 1]), lstm)[4]
        for weight_t, bias in layers:
            h = policy.activation(policy.linear(h, weight_t, bias), spec.activation)
        mu = policy.linear(h, *last)[:, 0]
    return mu, sde.sigma_of(h, sde.std2_of(params[spec.log_std_at:])), h


@functools.lru_cache(maxsize=None)
def update_inputs(index, n_steps, num_envs, kind):
    """(spec, packed parameters, batch dict of N rows, episode_starts, lstm_states).  The stored actions are the twin's
    own sampled raw actions (log_std rows of -100, 0 and +3: some lie far past +-1), the stored log-probabilities its own
    shifted by SHIFTS in turn; the stored states are normal values of scale 1/2."""
    from reinfocus_amd.environments import sde

    network = NETWORKS[index]
    spec = spec_of(network)
    params = spec.pack(state_dict(spec, 300 + index, hostile=spec.latent > 1))
    total = n_steps * num_envs
    rng = np.random.default_rng(1000 * index + total)
    starts = starts_of(kind, n_steps, num_envs)
    states = (0.5 * rng.standard_normal((n_steps + 1,) + spec.state_shape(num_envs))).astype(np.float32)
    batch = {"observations": learner_cases.finite_rows(network[0], total, 77 * index + total),
             "advantages": rng.standard_normal(total).astype(np.float32),
             "returns": rng.standard_normal(total).astype(np.float32)}
    mu, sigma, h = own_head(spec, params, batch, starts, states, n_steps, num_envs)
    theta = sde.noise_numpy(params[spec.log_std_at:], rng.random(total * spec.latent))
    with np.errstate(all="ignore"):
        batch["actions"] = sde_module_canonical(mu + sde._rowdot(h, theta))
    shifts = np.array(SHIFTS, dtype=np.float32)[np.arange(total) % len(SHIFTS)]
    batch["log_probs"] = (sde.log_prob_of(batch["actions"], mu, sigma) - shifts).astype(np.float32)
    assert np.isfinite(batch["actions"]).all() and np.isfinite(batch["log_probs"]).all()
    return spec, params, batch, starts, states


def sde_module_canonical(a):
    from reinfocus_amd.environments import policy

    return policy.canonical(a)


def layout_inputs(index, name):
    n_steps, num_envs, kind, first, count = LAYOUTS[name]
    return update_inputs(index, n_steps, num_envs, kind) + (n_steps, num_envs, first, count)


@functools.lru_cache(maxsize=None)
def twin_updates(index, name):
    """[(params, state, stats, gradient)] after each of UPDATES consecutive updates by the numpy twin on the layout's
    minibatch: the reference, computed once."""
    from reinfocus_amd.environments import learner, lstm_learner

    spec, params, batch, starts, states, n_steps, num_envs, first, count = layout_inputs(index, name)
    state = learner.fresh_state(spec)
    seen = []
    for update in range(UPDATES):
        grad = lstm_learner.lstm_gradient_numpy(spec, params, batch, starts, states, n_steps, num_envs, first, count,
                                                hyper_of(update))[0]
        params, state, stats = lstm_learner.lstm_update_numpy(spec, params, state, batch, starts, states, n_steps, num_envs,
                                                              first, count, hyper_of(update))
        seen.append((params, state, stats, grad))
    return seen


def hostcheck():
    from tests import helpers

    lib = ctypes.CDLL(helpers.built("tests/lstmsdecheck", "liblstmsdecheck.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for name in ("lsc_params_size", "lsc_log_std", "lsc_state_size", "lsc_workspace_size", "lsc_grad_offset"):
        getattr(lib, name).restype = ctypes.c_ulonglong
    lib.lsc_params_size.argtypes = lib.lsc_state_size.argtypes = [vp]
    lib.lsc_log_std.argtypes = [vp, vp]
    lib.lsc_workspace_size.argtypes = lib.lsc_grad_offset.argtypes = [vp, i32]
    lib.lsc_noise.argtypes = [vp, vp, i32, vp, vp]
    lib.lsc_forward.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.lsc_update.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    return lib


def _lstm_desc(spec):
    from reinfocus_amd import _native

    return _native.LstmPolicyDesc(*spec.desc())


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
T = rollout_cases.T
GAMMA, GAE_LAMBDA = rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA
E2E_SIZES, E2E_ITERATIONS, E2E_EPOCHS, E2E_BATCH, E2E_FREQ = (1, 9), 2, 2, 4, 3
# with LearnerView + episode records on the small network, and with neither on the untuned configuration's
E2E_KINDS = {"view": dict(view=True, records=True, network=SMALL), "plain": dict(view=False, records=False, network=UNTUNED)}
LEARNER_KW = dict(learning_rate=1e-2, ent_coef=0.01)
e2e_splits = lstm_learner_cases.e2e_splits


def make_env(kind, n, device_form):
    from reinfocus_amd.environments import harness

    what = E2E_KINDS[kind]
    extra = dict(episode_records=what["records"], learner_view=harness.LearnerView(frame_stack=1) if what["view"] else None)
    if device_form:
        return harness.DeviceVectorContinuousJumps(num_envs=n, device_initializer=True, **rollout_cases.ENV_KW, **extra)
    return harness.VectorContinuousJumps(num_envs=n, **rollout_cases.ENV_KW, **extra)


def e2e_spec(kind, env):
    network = NETWORKS[E2E_KINDS[kind]["network"]]
    return spec_of((int(env.single_observation_space.shape[0]),) + network[1:], log_std_init=-0.5)


def e2e_state(spec):
    state = state_dict(spec, 3)
    state["log_std"][:] = np.float32(spec.log_std_init)
    return state


def train_runs(rollout, policy, learner, reset, unwrap):
    """E2E_ITERATIONS iterations of collect(sde_sample_freq=E2E_FREQ) + train: per iteration every slab of the rollout (the
    recurrent ones included), theta, the parameters, the optimizer state and the stats, unwrapped."""
    obs = reset()
    seen = []
    for iteration in range(E2E_ITERATIONS):
        rollout.start(obs if iteration == 0 else None)
        rollout.collect(policy, sde_sample_freq=E2E_FREQ)
        record = lstm_cases.slabs_of(rollout, policy, unwrap)
        record["theta"] = unwrap(policy.noise())
        record["stats"] = unwrap(learner.train(rollout, E2E_EPOCHS, E2E_BATCH,
                                               splits=e2e_splits(iteration, T * rollout.num_envs)))
        record["params"], record["state"] = unwrap(policy.params), unwrap(learner.state)
        seen.append(record)
    return seen


@functools.lru_cache(maxsize=None)
def twin_train_runs(kind, n):
    """(runs, the twin policy's generator state afterwards)."""
    from reinfocus_amd.environments import harness

    env = make_env(kind, n, False)
    try:
        spec = e2e_spec(kind, env)
        policy = harness.LstmSdePolicy(spec, SEED, num_envs=n)
        policy.load_state_dict(e2e_state(spec))
        learner = harness.LstmLearner(policy, **LEARNER_KW)
        rollout = harness.Rollout(env, T, GAMMA, GAE_LAMBDA)
        return train_runs(rollout, policy, learner, lambda: env.reset()[0], np.array), policy.rng_state()
    finally:
        env.close()


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
_guarded, _guards_kept = learner_cases._guarded, learner_cases._guards_kept
_guarded_state, _state_guards_kept = lstm_cases._guarded_state, lstm_cases._guards_kept
_sentinels = sde_cases._sentinels


def _unwrap(tensor):
    return tensor.cpu().numpy()


def _untouched(whole):
    return bool((whole.cpu().numpy().view(np.uint32) == SENTINEL).all())


def _call(torch, ctx, spec, params, n, obs, starts, final_obs, state_in, state_out, theta, flags, out, changed=()):
    """rf_lstm_sde_forward; out: {name: tensor or None} for OUTPUTS; changed: arguments by name, in place of the tensors'."""
    pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = dict(desc=spec.desc(), params=params.data_ptr(), n=n, obs=obs.data_ptr(), starts=starts.data_ptr(),
             final_obs=pointer(final_obs), state_in=state_in.data_ptr(), state_out=pointer(state_out), theta=pointer(theta),
             flags=flags)
    a.update({name: pointer(out.get(name)) for name in OUTPUTS})
    a.update(changed)
    ctx.lstm_sde_forward(a["desc"], a["params"], a["n"], a["obs"], a["starts"], a["final_obs"], a["state_in"], a["state_out"],
                         a["theta"], a["flags"], *(a[name] for name in OUTPUTS), torch.cuda.current_stream().cuda_stream)


def noise_case(torch, ctx, index, n):
    """rf_lstm_sde_noise_reset against the twin as bytes at both draw offsets, theta between guards."""
    from reinfocus_amd.environments import policy

    spec, params_h = chain_inputs(index, n)[:2]
    assert ctx.lstm_sde_params_size(spec.desc()) == spec.size
    params = torch.from_numpy(params_h).cuda()
    for offset in OFFSETS:
        whole, theta = _sentinels(torch, n * spec.latent)
        ctx.lstm_sde_noise_reset(spec.desc(), params.data_ptr(), n, policy.generator_words(generator_at(offset)[0]),
                                 theta.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert bits(_unwrap(theta).reshape(n, spec.latent)) == bits(wanted_theta(index, n, offset)), f"offset {offset}"
        assert _guards_kept(whole)


def kernel_case(torch, ctx, index, n):
    """rf_lstm_sde_forward against lstm_sde_numpy as bytes over a chain of STEPS steps: sampled at both draw offsets and
    deterministic, each with the state in place and from one tensor into another; then every subset of outputs that
    changes which blocks run: pi only, vf only (with V(final_obs)), values only, the state only."""
    from reinfocus_amd.environments import lstm_sde, policy

    spec, params_h, obs_h, final_h, starts_h, state_h = chain_inputs(index, n)
    params, obs, final_obs, starts = (torch.from_numpy(a).cuda() for a in (params_h, obs_h, final_h, starts_h))
    for mode, offset in MODES:
        want = wanted_chain(index, n, mode, offset)
        theta = torch.from_numpy(wanted_theta(index, n, offset)).cuda() if mode == "sampled" else None
        for in_place in (True, False):
            buffers = [_guarded_state(torch, spec, n, state_h), _guarded_state(torch, spec, n)]
            for s in range(STEPS):
                source = buffers[0] if in_place else buffers[s % 2]
                target = buffers[0] if in_place else buffers[(s + 1) % 2]
                outs = {name: _sentinels(torch, n) for name in OUTPUTS}
                _call(torch, ctx, spec, params, n, obs[s], starts[s], final_obs[s], source[1], target[1], theta,
                      0 if mode == "sampled" else policy.DETERMINISTIC, {name: outs[name][1] for name in OUTPUTS})
                torch.cuda.synchronize()
                where = f"{mode} at {offset}, {'in place' if in_place else 'apart'}, step {s}"
                for name in OUTPUTS:
                    assert bits(_unwrap(outs[name][1])) == bits(want[s][name]), f"{where}: {name} differ"
                    assert _guards_kept(outs[name][0]), f"{where}: a guard of {name}"
                assert bits(_unwrap(target[1])) == bits(want[s]["state"]), f"{where}: the state differs"
                assert _state_guards_kept(target[0]) and _state_guards_kept(source[0]), f"{where}: a guard row of the state"
                if not in_place and s > 0:  # (the source keeps what the step before wrote)
                    assert bits(_unwrap(source[1])) == bits(want[s - 1]["state"]), f"{where}: the source changed"
    sampled = wanted_chain(index, n, "sampled", 0)[0]
    theta = torch.from_numpy(wanted_theta(index, n, 0)).cuda()
    subsets = {"pi only": (PI_OUTPUTS, True, False), "vf only": (("values", "final_values"), True, False),
               "values only": (("values",), False, False), "state only": ((), False, True)}
    for what, (names, with_final, with_state) in subsets.items():
        whole_state, state = _guarded_state(torch, spec, n, state_h)
        whole_target, target = _guarded_state(torch, spec, n)
        outs = {name: _sentinels(torch, n) for name in OUTPUTS}
        _call(torch, ctx, spec, params, n, obs[0], starts[0], final_obs[0] if with_final else None, state,
              target if with_state else None, theta, 0, {name: outs[name][1] for name in names})
        torch.cuda.synchronize()
        for name in OUTPUTS:
            if name in names:
                assert bits(_unwrap(outs[name][1])) == bits(sampled[name]), f"{what}: {name} differ"
                assert _guards_kept(outs[name][0]), f"{what}: a guard of {name}"
            else:
                assert _untouched(outs[name][0]), f"{what}: {name} was written"
        assert bits(_unwrap(state)) == bits(state_h) and _state_guards_kept(whole_state), f"{what}: the source state changed"
        if with_state:
            assert bits(_unwrap(target)) == bits(sampled["state"]) and _state_guards_kept(whole_target), what
        else:
            assert _untouched(whole_target), f"{what}: a state was written"
    want = lstm_sde.lstm_sde_numpy(spec, params_h, obs_h[0], starts_h[0], state_h, final_h[0], values_only=True)
    assert bits(want["values"]) == bits(sampled["values"]) and bits(want["final_values"]) == bits(sampled["final_values"])


class _Device(lstm_learner_cases._Device):
    """One update's device arrays, for rf_lstm_sde_update."""

    def __init__(self, torch, ctx, lib, spec, params, state, batch, starts, states, n_steps, num_envs, max_batch=None):
        self.torch, self.ctx, self.lib, self.spec = torch, ctx, lib, spec
        self.n_steps, self.num_envs = n_steps, num_envs
        self.whole = {}
        self.whole["params"], self.params = _guarded(torch, params)
        self.whole["state"], self.state = _guarded(torch, state)
        self.whole["stats"], self.stats = _sentinels(torch, 8)
        total = max_batch or n_steps * num_envs  # (the workspace's max_batch: N, or a limit layout's B)
        floats = ctx.lstm_sde_workspace_size(spec.desc(), total) // 4
        assert floats > 0 and ctx.lstm_sde_state_size(spec.desc()) == 4 * state.size == 32 + 8 * spec.size
        assert ctx.lstm_sde_workspace_size(spec.desc(), 1) <= 4 * floats
        assert 4 * floats == lib.lsc_workspace_size(ctypes.byref(_lstm_desc(spec)), total)
        self.whole["workspace"], self.workspace = _guarded(torch, np.zeros(floats, dtype=np.float32))
        self.batch = {key: torch.from_numpy(value).cuda() for key, value in batch.items()}
        self.starts, self.states = torch.from_numpy(starts).cuda(), torch.from_numpy(states).cuda()

    def call(self, first, count, hyper, **changed):
        a = dict(desc=self.spec.desc(), hyper=tuple(hyper), params=self.params.data_ptr(), state=self.state.data_ptr(),
                 workspace=self.workspace.data_ptr(), n_steps=self.n_steps, num_envs=self.num_envs,
                 obs=self.batch["observations"].data_ptr(), actions=self.batch["actions"].data_ptr(),
                 log_probs=self.batch["log_probs"].data_ptr(), advantages=self.batch["advantages"].data_ptr(),
                 returns=self.batch["returns"].data_ptr(), starts=self.starts.data_ptr(), states=self.states.data_ptr(),
                 first=first, batch=count, stats=self.stats.data_ptr(),
                 stream=self.torch.cuda.current_stream().cuda_stream)
        a.update(changed)  # (arguments given by their names above, in place of the tensors')
        self.ctx.lstm_sde_update(a["desc"], a["hyper"], a["params"], a["state"], a["workspace"], a["n_steps"], a["num_envs"],
                                 a["obs"], a["actions"], a["log_probs"], a["advantages"], a["returns"], a["starts"],
                                 a["states"], a["first"], a["batch"], a["stats"], a["stream"])

    def gradient(self, count):
        """The packed gradient (log_std's last) the last update of `count` rows left in the workspace."""
        at = int(self.lib.lsc_grad_offset(ctypes.byref(_lstm_desc(self.spec)), count))
        return self.workspace[at:at + self.spec.size].cpu().numpy()


_same_update = lstm_learner_cases._same_update


def update_case(torch, ctx, lib, index, name):
    """rf_lstm_sde_update against lstm_update_numpy as bytes over UPDATES consecutive updates, the gradient included; a
    limit layout's workspace is sized for its B, not for N."""
    from reinfocus_amd.environments import learner

    spec, params, batch, starts, states, n_steps, num_envs, first, count = layout_inputs(index, name)
    want = twin_updates(index, name)
    device = _Device(torch, ctx, lib, spec, params, learner.fresh_state(spec), batch, starts, states, n_steps, num_envs,
                     count if name in LIMIT_LAYOUTS else None)
    for update in range(UPDATES):
        device.call(first, count, hyper_of(update))
        _same_update(device.outputs() + (device.gradient(count),), want[update], f"update {update}")
    assert device.guards_kept(), "a guard was written"
    assert all(stats[7] == 0 for _, _, stats, _ in want)


def skip_case(torch, ctx, lib):
    """A NaN stored action (RF_PPO_INVALID) and a log_std of 90 (sigma infinite: RF_PPO_NONFINITE) leave parameters and
    optimizer state as they were, with the twin's stats; the update after them is taken."""
    from reinfocus_amd.environments import learner, lstm_learner

    index, name = SMALL, f"mixed/3/{TILE + 1}"
    spec, params, batch, starts, states, n_steps, num_envs, first, count = layout_inputs(index, name)
    want = twin_updates(index, name)
    device = _Device(torch, ctx, lib, spec, params, learner.fresh_state(spec), batch, starts, states, n_steps, num_envs)
    device.call(first, count, hyper_of(0))
    _same_update(device.outputs(), want[0][:3], "the first update")
    nan_action = dict(batch, actions=batch["actions"].copy())
    nan_action["actions"][(first + 1) % ROWS] = np.nan
    wide = want[0][0].copy()
    wide[spec.log_std_at:] = np.float32(90.0)
    for what, start, changed, flag in (("NaN action", want[0][0], nan_action, learner.INVALID),
                                       ("log_std of 90", wide, batch, learner.NONFINITE)):
        device.params.copy_(torch.from_numpy(start))
        device.batch = {key: torch.from_numpy(value).cuda() for key, value in changed.items()}
        device.call(first, count, hyper_of(1))
        twin = lstm_learner.lstm_update_numpy(spec, start, want[0][1], changed, starts, states, n_steps, num_envs, first,
                                              count, hyper_of(1))
        assert twin[2][7] == flag and bits(twin[0]) == bits(start) and bits(twin[1]) == bits(want[0][1]), what
        _same_update(device.outputs(), twin, what)
    device.params.copy_(torch.from_numpy(want[0][0]))
    device.batch = {key: torch.from_numpy(value).cuda() for key, value in batch.items()}
    device.call(first, count, hyper_of(1))
    _same_update(device.outputs(), want[1][:3], "the update after the skipped ones")
    assert device.guards_kept()


def forward_refusal_case(torch, ctx):
    """Each refusal of rf_lstm_sde_forward and rf_lstm_sde_noise_reset leaves the outputs and the states as they were."""
    from reinfocus_amd.environments import policy

    index, n = SMALL, TILE + 1
    spec, params_h, obs_h, final_h, starts_h, state_h = chain_inputs(index, n)
    params, obs, final_obs, starts = (torch.from_numpy(a).cuda() for a in (params_h, obs_h[0], final_h[0], starts_h[0]))
    theta = torch.from_numpy(wanted_theta(index, n, 0)).cuda()
    outs = {name: _sentinels(torch, n) for name in OUTPUTS}
    out = {name: outs[name][1] for name in OUTPUTS}
    whole_in, state_in = _guarded_state(torch, spec, n, state_h)
    whole_out, state_out = _guarded_state(torch, spec, n)

    def refused(match, **changed):
        try:
            _call(torch, ctx, spec, params, n, obs, starts, final_obs, state_in, state_out, theta,
                  changed.pop("flags", 0), out, changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        torch.cuda.synchronize()
        assert all(_untouched(whole) for whole, _ in outs.values()), f"an output was written ({match})"
        assert _untouched(whole_out) and bits(_unwrap(state_in)) == bits(state_h), f"a state was written ({match})"

    host = np.zeros((n + 2, max(spec.obs_width, 4 * spec.lstm_hidden, spec.latent)), dtype=np.float32)
    refused("d_obs is not device memory", obs=host.ctypes.data)
    refused("d_values is not device memory", values=host.ctypes.data)
    refused("d_params is not device memory", params=params_h.ctypes.data)
    refused("d_episode_starts is not device memory", starts=starts_h.ctypes.data)
    refused("d_state_in is not device memory", state_in=state_h.ctypes.data)
    refused("d_theta is not device memory", theta=host.ctypes.data)
    refused("at least 1", n=0)
    refused("not aligned", obs=obs.data_ptr() + 2)
    refused("not aligned", actions=out["actions"].data_ptr() + 2)
    refused("not aligned", state_out=state_out.data_ptr() + 2)
    refused("d_values overlaps d_obs", values=obs.data_ptr())
    refused("d_values overlaps d_log_probs", values=out["log_probs"].data_ptr())
    refused("d_mean overlaps d_params", mean=params.data_ptr())
    refused("d_sigma overlaps d_theta", sigma=theta.data_ptr())
    refused("d_values overlaps d_state_in", values=state_in.data_ptr())
    refused("d_state_out overlaps d_values", values=state_out.data_ptr())
    refused("d_state_out overlaps d_state_in without being it", state_out=state_in.data_ptr() + 4 * spec.lstm_hidden)
    refused("d_state_out overlaps d_state_in without being it", state_out=state_in.data_ptr() - 4)
    block = torch.zeros(32 * 1024 * 1024, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    # (were the length check to miss it, the aliased output of the same call is refused next: nothing can run past the end)
    alias = out["log_probs"].data_ptr()
    refused("fewer than", obs=end - 4 * (n * spec.obs_width - 1), values=alias)
    refused("fewer than", params=end - 4 * (spec.size - 1), values=alias)
    refused("fewer than", theta=end - 4 * (n * spec.latent - 1), values=alias)
    refused("fewer than", state_in=end - 4 * (state_h.size - 1), values=alias)
    refused("d_state_out has fewer than", state_out=end - 4 * (state_h.size - 1))
    refused("fewer than", starts=end - (n - 1), values=alias)
    desc = list(spec.desc())
    for field, value in ((0, 0), (0, 257), (1, 0), (1, 2), (1, 13), (2, 2), (3, 0), (3, 3), (4, 257), (5, 0), (6, 3), (7, 0),
                         (9, 0), (9, 257), (9, -1)):
        refused("outside the limits", desc=tuple(desc[:field] + [value] + desc[field + 1:]))
    refused("unknown flags", flags=2)
    refused("needs d_theta", theta=None)  # (a pi output is sampled)
    refused("needs d_final_obs", final_obs=None)
    refused("NULL argument", starts=None)
    refused("NULL argument", state_in=None)
    refused("no output is asked for", state_out=None, **{name: None for name in OUTPUTS})
    stream = torch.cuda.current_stream().cuda_stream
    gen = policy.generator_words(generator_at(0)[0])
    whole_theta, fresh = _sentinels(torch, n * spec.latent)
    for match, changed in (("outside the limits", dict(desc=tuple(desc[:1] + [2] + desc[2:]))), ("at least 1", dict(n=0)),
                           ("NULL argument", dict(theta=None)), ("d_theta is not device memory", dict(theta=host.ctypes.data)),
                           ("d_theta overlaps d_params", dict(theta=params.data_ptr())),
                           ("fewer than", dict(theta=end - 4 * (n * spec.latent - 1)))):
        a = dict(desc=spec.desc(), params=params.data_ptr(), n=n, theta=fresh.data_ptr())
        a.update(changed)
        try:
            ctx.lstm_sde_noise_reset(a["desc"], a["params"], a["n"], gen, a["theta"], stream)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"noise reset not refused ({match})")
        torch.cuda.synchronize()
        assert _untouched(whole_theta), f"theta was written ({match})"
    # a deterministic call needs no theta, nor does a call without a pi output; the unchanged call is taken
    _call(torch, ctx, spec, params, n, obs, starts, None, state_in, None, None, 0, dict(values=out["values"]))
    torch.cuda.synchronize()
    want = wanted_chain(index, n, "sampled", 0)[0]
    assert bits(_unwrap(out["values"])) == bits(want["values"])
    _call(torch, ctx, spec, params, n, obs, starts, final_obs, state_in, state_out, theta, 0, out)
    torch.cuda.synchronize()
    for name in OUTPUTS:
        assert bits(_unwrap(out[name])) == bits(want[name]), name
        assert _guards_kept(outs[name][0]), name
    assert bits(_unwrap(state_out)) == bits(want["state"]) and _state_guards_kept(whole_out)


def update_refusal_case(torch, ctx, lib):
    """Each refusal of rf_lstm_sde_update leaves parameters, state and stats as they were: nothing was enqueued."""
    from reinfocus_amd.environments import learner

    index, name = SMALL, f"mixed/3/{TILE + 1}"
    spec, params, batch, starts, states, n_steps, num_envs, first, count = layout_inputs(index, name)
    want = twin_updates(index, name)
    device = _Device(torch, ctx, lib, spec, params, learner.fresh_state(spec), batch, starts, states, n_steps, num_envs)
    before = device.outputs()
    assert (before[2].view(np.uint32) == SENTINEL).all()

    def refused(match, **changed):
        hyper = changed.pop("hyper", hyper_of(0))
        try:
            device.call(changed.pop("first", first), count, hyper, **changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        got = device.outputs()
        assert all(bits(x) == bits(y) for x, y in zip(got, before)), f"an output was written ({match})"

    desc = list(spec.desc())
    for field, value in ((0, 0), (0, 257), (1, 0), (1, 2), (1, 13), (2, 2), (3, 0), (3, 3), (4, 257), (6, 3), (7, 0), (9, 0),
                         (9, 257), (9, -1)):
        refused("outside the limits", desc=tuple(desc[:field] + [value] + desc[field + 1:]))
    refused("at least 1", n_steps=0)
    refused("at least 1", num_envs=0)
    refused("B = ", batch=0)
    refused("B = ", batch=ROWS + 1)
    refused("B = ", batch=1025)
    refused("first = ", first=-1)
    refused("first = ", first=ROWS)
    for field in range(8):
        refused("hyper-parameter", hyper=hyper_of(0)._replace(**{learner.Hyper._fields[field]: -1.0}))
        refused("hyper-parameter", hyper=hyper_of(0)._replace(**{learner.Hyper._fields[field]: float("nan")}))
    refused("hyper-parameter", hyper=hyper_of(0)._replace(learning_rate=float("inf")))
    refused("hyper-parameter", hyper=hyper_of(0)._replace(beta1=1.0))
    refused("hyper-parameter", hyper=hyper_of(0)._replace(beta2=1.5))
    host = np.zeros(4 * spec.size + 64, dtype=np.float32)
    for key in ("params", "state", "workspace", "obs", "actions", "log_probs", "advantages", "returns", "starts", "states",
                "stats"):
        refused("NULL argument", **{key: None})
        refused("is not device memory", **{key: host.ctypes.data})
    refused("not aligned", obs=device.batch["observations"].data_ptr() + 2)
    refused("not aligned", actions=device.batch["actions"].data_ptr() + 2)
    refused("not aligned", states=device.states.data_ptr() + 2)
    refused("not aligned", state=device.state.data_ptr() + 4)
    refused("not aligned", workspace=device.workspace.data_ptr() + 4)
    block = torch.zeros(32 * 1024 * 1024, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    refused("fewer than", obs=end - 4 * (ROWS * spec.obs_width - 1))
    refused("fewer than", actions=end - 4 * (ROWS - 1))
    refused("fewer than", params=end - 4 * (spec.size - 1))  # (P + L floats: one short of log_std's last)
    refused("fewer than", state=end - 8 * spec.size)  # (a state that is too small)
    refused("fewer than", workspace=end - 1024)  # (a workspace that is too small)
    refused("fewer than", stats=end - 16)
    refused("d_episode_starts has fewer than", starts=end - ((n_steps + 1) * num_envs - 1))  # (the slabs have T + 1 rows)
    refused("d_lstm_states has fewer than", states=end - 4 * (states.size - 1))
    refused("d_lstm_states has fewer than", states=end - 4 * n_steps * 4 * num_envs * spec.lstm_hidden)  # (T rows only)
    refused("d_params overlaps d_observations", params=device.batch["observations"].data_ptr())
    refused("d_stats overlaps d_returns", stats=device.batch["returns"].data_ptr())
    refused("d_workspace overlaps d_lstm_states", workspace=device.states.data_ptr())
    refused("d_state overlaps d_params", state=device.params.data_ptr())
    refused("d_workspace overlaps d_state", workspace=device.state.data_ptr())
    refused("d_stats overlaps d_workspace", stats=device.workspace.data_ptr())
    device.call(first, count, hyper_of(0))  # ... and the same arguments unchanged are taken
    _same_update(device.outputs() + (device.gradient(count),), want[0], "the unchanged call")
    assert device.guards_kept()
    lstm_learner_cases._capturing_stream_is_refused(torch, device, first, count)


def _device_pair(torch, harness, env, kind):
    spec = e2e_spec(kind, env)
    policy = harness.DeviceLstmSdePolicy(env, spec, SEED)
    policy.load_state_dict({k: torch.from_numpy(v).cuda() for k, v in e2e_state(spec).items()})
    return policy, harness.DeviceLstmLearner(policy, **LEARNER_KW)


def end_to_end_case(torch, kind, n):
    from reinfocus_amd.environments import harness

    want, rng_state = twin_train_runs(kind, n)
    env = make_env(kind, n, True)
    try:
        policy, learner = _device_pair(torch, harness, env, kind)
        assert bits(_unwrap(policy.params)) == bits(policy.spec.pack(e2e_state(policy.spec)))
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        got = train_runs(rollout, policy, learner, lambda: env.reset_tensors()[0], _unwrap)
        same_runs(got, want)
        assert env.device_fault() is None
        assert policy.rng_state() == rng_state
        assert bits(want[0]["params"]) != bits(want[1]["params"]) and (want[1]["stats"][:, 7] == 0).all()
        assert want[0]["stats"].shape == (E2E_EPOCHS * -(-T * n // E2E_BATCH), 8)
        assert bits(want[0]["params"][policy.spec.log_std_at:]) != bits(want[1]["params"][policy.spec.log_std_at:])
        for run in got:
            assert bits(run["episode_starts"][1:]) == bits(run["truncated"])
            assert run["actions"].dtype == np.float32 and bits(run["lstm_states"][T]) == bits(run["policy_state"])
        if n > 1:  # (episode starts fall inside minibatches)
            assert want[1]["episode_starts"][1:T].any()
    finally:
        env.close()


def no_sync_case(torch):
    """Two iterations of collect + train enqueued back to back, nothing read in between; one synchronisation at the end."""
    from reinfocus_amd.environments import harness

    kind, n = "view", 9
    want = twin_train_runs(kind, n)[0]
    env = make_env(kind, n, True)
    try:
        policy, learner = _device_pair(torch, harness, env, kind)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        obs = env.reset_tensors()[0]
        torch.cuda.synchronize()
        kept = []
        for iteration in range(E2E_ITERATIONS):
            rollout.start(obs if iteration == 0 else None)
            rollout.collect(policy, sde_sample_freq=E2E_FREQ)
            stats = learner.train(rollout, E2E_EPOCHS, E2E_BATCH, splits=e2e_splits(iteration, T * n))
            kept.append((stats, policy.params.clone(), rollout.lstm_states.clone(), rollout.actions.clone(), policy.noise()))
        torch.cuda.synchronize()  # the only one
        for iteration, (stats, params, states, actions, theta) in enumerate(kept):
            assert bits(_unwrap(stats)) == bits(want[iteration]["stats"]), iteration
            assert bits(_unwrap(params)) == bits(want[iteration]["params"]), iteration
            assert bits(_unwrap(states)) == bits(want[iteration]["lstm_states"]), iteration
            assert bits(_unwrap(actions)) == bits(want[iteration]["actions"]), iteration
            assert bits(_unwrap(theta)) == bits(want[iteration]["theta"]), iteration
        assert bits(_unwrap(learner.state)) == bits(want[-1]["state"])
        assert env.device_fault() is None
    finally:
        env.close()


def resume_case(torch):
    """state_dict / load_state_dict of the policy (log_std included) and the optimizer resume bit for bit over P + L."""
    from reinfocus_amd.environments import harness

    kind, n = "view", 9
    env = make_env(kind, n, True)
    try:
        policy, learner = _device_pair(torch, harness, env, kind)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        rollout.start(env.reset_tensors()[0])
        rollout.collect(policy, sde_sample_freq=E2E_FREQ)
        splits = e2e_splits(0, T * n)
        learner.train(rollout, E2E_EPOCHS, E2E_BATCH, splits=splits)
        kept, kept_params = learner.state_dict(), policy.state_dict()
        assert kept["step"] == E2E_EPOCHS * -(-T * n // E2E_BATCH)
        assert kept["m"].numel() == policy.spec.size and tuple(kept_params["log_std"].shape) == (policy.spec.latent, 1)
        assert _unwrap(kept["m"])[policy.spec.log_std_at:].any()  # (log_std has moments: it is trained)
        straight = _unwrap(learner.train(rollout, E2E_EPOCHS, E2E_BATCH, splits=splits))
        want = _unwrap(policy.params), _unwrap(learner.state)
        policy.load_state_dict(kept_params)
        fresh = harness.DeviceLstmLearner(policy, **LEARNER_KW)
        fresh.load_state_dict(kept)
        resumed = _unwrap(fresh.train(rollout, E2E_EPOCHS, E2E_BATCH, splits=splits))
        assert bits(resumed) == bits(straight)
        assert bits(_unwrap(policy.params)) == bits(want[0]) and bits(_unwrap(fresh.state)) == bits(want[1])
    finally:
        env.close()


def surface_case(torch):
    """The refusals of the Python surface; reset_noise advances the generator by n * L; act() without out=, deterministic,
    and from one state tensor into another; the rng state round-trips."""
    from reinfocus_amd.environments import harness

    n = 5
    steps = harness.DeviceVectorDiscreteSteps(num_envs=2, device_initializer=True, **rollout_cases.ENV_KW)
    env = make_env("view", n, True)
    try:
        spec = e2e_spec("view", env)
        for build, error, match in ((lambda: harness.DeviceLstmSdePolicy(steps, spec, 0), ValueError, "Gaussian head"),
                                    (lambda: harness.DeviceLstmPolicy(env, lstm_cases.e2e_spec("view"), 0), ValueError,
                                     "out of scope"),
                                    (lambda: harness.DeviceLstmSdePolicy(env, lstm_cases.e2e_spec("view"), 0), TypeError,
                                     "LstmSdePolicySpec")):
            try:
                build()
            except error as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"taken ({match})")
        policy, learner = _device_pair(torch, harness, env, "view")
        twin = harness.LstmSdePolicy(spec, SEED, num_envs=n)
        twin.load_state_dict(e2e_state(spec))
        obs_h = hostile_rows(spec.obs_width, n, 5, False)
        starts_h = np.array([0, 1, 0, 255, 0], dtype=np.uint8)
        obs, starts = torch.from_numpy(obs_h).cuda(), torch.from_numpy(starts_h).cuda()
        try:
            policy.act(obs, starts)
        except ValueError as caught:
            assert "reset_noise" in str(caught)
        else:
            raise AssertionError("a sampled act() before reset_noise() was taken")
        before = np.random.PCG64DXSM(SEED)
        policy.reset_noise()
        twin.reset_noise()
        before.advance(n * spec.latent)
        assert policy.rng_state() == twin.rng_state() == before.state  # (the generator is advanced by n * L)
        assert bits(_unwrap(policy.noise())) == bits(twin.noise())
        start_state = lstm_cases.hostile_state(spec, n, 1)
        start_state[:, :, 0, :] = 0.5
        policy.set_lstm_state(torch.from_numpy(start_state).cuda())
        twin.set_lstm_state(start_state)
        for deterministic in (True, False):
            got = policy.act(obs, starts, deterministic=deterministic)
            want = twin.act(obs_h, starts_h, deterministic=deterministic)
            assert got[3] is None and want[3] is None
            for x, y in zip(got[:3] + got[4:], want[:3] + want[4:]):
                assert bits(_unwrap(x)) == bits(y)
            assert bits(_unwrap(policy.lstm_state())) == bits(twin.lstm_state())
        assert policy.rng_state() == before.state  # (act() consumes no draw)
        kept = policy.lstm_state()
        assert bits(_unwrap(policy.values(obs, starts))) == bits(twin.values(obs_h, starts_h))
        assert bits(_unwrap(policy.lstm_state())) == bits(_unwrap(kept))  # (values() never advances the state)
        apart = (policy.lstm_state(), torch.zeros_like(kept))
        policy.act(obs, starts, states=apart)
        twin_apart = (twin.lstm_state(), np.zeros_like(twin.lstm_state()))
        twin.act(obs_h, starts_h, states=twin_apart)
        assert bits(_unwrap(apart[1])) == bits(twin_apart[1]) and bits(_unwrap(policy.lstm_state())) == bits(_unwrap(kept))
        policy.set_rng_state(twin.rng_state())
        try:
            policy.reset_noise(n + 1)
        except ValueError:
            pass
        else:
            raise AssertionError("a reset_noise() of another size was taken")
        # the rollout's and the learner's refusals
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        rollout.start(env.reset_tensors()[0])
        for bad in (0, -2, 1.5):
            try:
                rollout.collect(policy, sde_sample_freq=bad)
            except ValueError as caught:
                assert "sde_sample_freq" in str(caught)
            else:
                raise AssertionError(f"sde_sample_freq {bad} was taken")
        other = harness.DeviceRollout(steps, T, GAMMA, GAE_LAMBDA)
        other.start(steps.reset_tensors()[0])
        for call, match in ((lambda: other.collect(policy), "Gaussian head"),
                            (lambda: learner.train(other, 1, E2E_BATCH), "Gaussian head")):
            try:
                call()
            except ValueError as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"taken ({match})")
        categorical = harness.DeviceLstmPolicy(steps, lstm_cases.e2e_spec("plain"), 0)
        try:
            harness.DeviceLstmLearner(categorical).train(rollout, 1, E2E_BATCH)
        except ValueError as caught:
            assert "out of scope" in str(caught)
        else:
            raise AssertionError("a Categorical learner took a ContinuousJumps rollout")
        rollout.collect(policy, sde_sample_freq=E2E_FREQ)
        try:
            learner.update(dict(harness_parts(rollout), actions=torch.zeros(T * n, dtype=torch.int64, device="cuda")), 0, 4)
        except ValueError as caught:
            assert "int64 action slab" in str(caught)
        else:
            raise AssertionError("an int64 action slab was taken")
        stats = learner.train(rollout, 1, 8, generator=np.random.default_rng(3))
        assert stats.shape == (-(-T * n // 8), 8) and (_unwrap(stats)[:, 7] == 0).all()
    finally:
        env.close()
        steps.close()


def harness_parts(rollout):
    from reinfocus_amd.environments import lstm_learner

    return lstm_learner.parts_of(rollout)


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    ctx = _native.Context(0)
    lib = hostcheck()
    for index in range(len(NETWORKS)):
        for n in sizes_of(index):
            with record.case(f"noise/{index}/{n}"):
                noise_case(torch, ctx, index, n)
            with record.case(f"kernel/{index}/{n}"):
                kernel_case(torch, ctx, index, n)
    with record.case("forward-refusals"):
        forward_refusal_case(torch, ctx)
    for index in range(len(NETWORKS)):
        for name in layouts_of(index) + limit_layouts_of(index):
            with record.case(f"update/{index}/{name}"):
                update_case(torch, ctx, lib, index, name)
    with record.case("skip"):
        skip_case(torch, ctx, lib)
    with record.case("update-refusals"):
        update_refusal_case(torch, ctx, lib)
    ctx.close()
    for kind in E2E_KINDS:
        for n in E2E_SIZES:
            with record.case(f"end-to-end/{kind}/{n}"):
                end_to_end_case(torch, kind, n)
    with record.case("no-sync"):
        no_sync_case(torch)
    with record.case("resume"):
        resume_case(torch)
    with record.case("surface"):
        surface_case(torch)
    with record.case("finished"):
        pass


# ---- torch on the CPU: nn.LSTM followed by the Gaussian written out from its definition ------------------------------------
SEQUENCE_STEPS, SEQUENCE_ROWS = lstm_cases.SEQUENCE_STEPS, lstm_cases.SEQUENCE_ROWS


def sequence_inputs(index):
    """(spec, state_dict, obs float32 [16, 32, D] of normal rows, starts uint8 [16, 32] with three episode starts inside
    the sequence, theta float32 [32, L])."""
    from reinfocus_amd.environments import sde

    spec = spec_of(NETWORKS[index])
    obs = np.random.default_rng(index).standard_normal((SEQUENCE_STEPS, SEQUENCE_ROWS, spec.obs_width)).astype(np.float32)
    starts = np.zeros((SEQUENCE_STEPS, SEQUENCE_ROWS), dtype=np.uint8)
    starts[4], starts[9], starts[12, ::2] = 1, 1, 1
    state = state_dict(spec, 50 + index)
    theta = sde.noise_numpy(state["log_std"][:, 0], np.random.default_rng(70 + index).random(SEQUENCE_ROWS * spec.latent))
    return spec, state, obs, starts, theta


def _torch_nets(torch, tensors, dtype, width, hidden, activation):
    """[(lstm, hidden layers with their activations, head)] for pi and vf, and {state_dict key: module}."""
    modules = {}

    def net(lstm_name, extractor, head_name):
        lstm = torch.nn.LSTM(width, hidden, num_layers=1).to(dtype)
        lstm.load_state_dict({part: tensors[f"{lstm_name}.{part}"] for part in
                              ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
        modules[lstm_name] = lstm
        layers = []
        keys = [f"mlp_extractor.{extractor}.{i}" for i in (0, 2) if f"mlp_extractor.{extractor}.{i}.weight" in tensors]
        for key in keys + [head_name]:
            weight = tensors[key + ".weight"]
            linear = torch.nn.Linear(weight.shape[1], weight.shape[0]).to(dtype)
            with torch.no_grad():
                linear.weight.copy_(weight)
                linear.bias.copy_(tensors[key + ".bias"])
            modules[key] = linear
            layers += [linear, activation()]
        return lstm, torch.nn.Sequential(*layers[:-2]), layers[-2]

    return [net("lstm_actor", "policy_net", "action_net"), net("lstm_critic", "value_net", "value_net")], modules


def _torch_gaussian(torch, latent, mean, log_std):
    """StateDependentNoiseDistribution at its defaults for one action: Normal(mu, sqrt((h * h) @ exp(log_std) ** 2 + 1e-6)),
    h detached inside the variance (learn_features=False)."""
    std = torch.exp(log_std)
    variance = torch.mm(latent.detach() ** 2, std ** 2)
    return torch.distributions.Normal(mean, torch.sqrt(variance + 1e-6))


def torch_sequence(path_in, path_out):
    """The sequence of sequence_inputs from a zero state, the state masked by (1 - start) as sb3-contrib does -- in
    float32 and in float64 from the same state_dict.  In a process of its own: torch brings a HIP runtime of its own."""
    import torch

    data = np.load(path_in)
    activation = torch.nn.Tanh if str(data["activation"]) == "tanh" else torch.nn.ReLU
    names = [str(name) for name in data["names"]]
    results = {}
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        tensors = {name: torch.from_numpy(data[name]).to(dtype) for name in names}
        obs, theta = torch.from_numpy(data["obs"]).to(dtype), torch.from_numpy(data["theta"]).to(dtype)
        keep = 1.0 - torch.from_numpy(data["starts"]).to(dtype)
        hidden = tensors["lstm_actor.weight_hh_l0"].shape[1]
        nets, _ = _torch_nets(torch, tensors, dtype, obs.shape[2], hidden, activation)
        seen = {key: [] for key in ("mean", "sigma", "actions", "log_probs", "values")}
        final = []
        with torch.no_grad():
            for which, (lstm, mlp, head) in enumerate(nets):
                h = torch.zeros(1, obs.shape[1], hidden, dtype=dtype)
                c = torch.zeros_like(h)
                for t in range(obs.shape[0]):
                    mask = keep[t].view(1, -1, 1)
                    out, (h, c) = lstm(obs[t:t + 1], (h * mask, c * mask))
                    latent = mlp(out[0])
                    if which == 1:
                        seen["values"].append(head(latent)[:, 0])
                        continue
                    distribution = _torch_gaussian(torch, latent, head(latent), tensors["log_std"])
                    action = distribution.mean[:, 0] + (latent * theta).sum(dim=1)
                    seen["mean"].append(distribution.mean[:, 0])
                    seen["sigma"].append(distribution.scale[:, 0])
                    seen["actions"].append(action)
                    seen["log_probs"].append(distribution.log_prob(action[:, None])[:, 0])
                final.append(torch.stack([h[0], c[0]]))
        for key, rows in seen.items():
            results[key + tag] = torch.stack(rows).numpy()
        results["state" + tag] = torch.stack(final).numpy()
    np.savez(path_out, **results)


def torch_learner(path_in, path_out):
    """From a state_dict, a rollout and one minibatch: the packed gradient before clipping (log_std's last) and the packed
    parameters after 1 and after `updates` updates on that minibatch, in float64 and in float32.  torch.nn.LSTM cells
    stepped per row with the sequence rule and the select of the definition, the stored states constants; the Gaussian of
    _torch_gaussian; stable-baselines3's loss, autograd, clip_grad_norm_ and Adam(eps=1e-5).  In a process of its own."""
    import torch

    data = np.load(path_in)
    names = [str(name) for name in data["names"]]
    activation = torch.nn.Tanh if str(data["activation"]) == "tanh" else torch.nn.ReLU
    clip_range, ent_coef, vf_coef, max_grad_norm, learning_rate = (float(data[k]) for k in (
        "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "learning_rate"))
    updates = int(data["updates"])
    row, env, step, is_start, zero = (data[k] for k in ("row", "env", "step", "is_start", "zero"))
    out = {}
    for label, dtype in (("64", torch.float64), ("32", torch.float32)):
        tensors = {name: torch.from_numpy(data[name]).to(dtype) for name in names}
        stored = torch.from_numpy(data["lstm_states"]).to(dtype)  # (no gradient: a constant)
        obs = torch.from_numpy(data["obs"]).to(dtype)[torch.from_numpy(row)]
        hidden = stored.shape[-1]
        nets, modules = _torch_nets(torch, tensors, dtype, obs.shape[1], hidden, activation)
        log_std = torch.nn.Parameter(tensors["log_std"].clone())

        def forward(which):
            lstm, mlp, head = nets[which]
            outs = []
            h = c = None
            for b in range(len(row)):
                if is_start[b]:
                    if zero[b]:
                        h = torch.zeros(1, 1, hidden, dtype=dtype)
                        c = torch.zeros(1, 1, hidden, dtype=dtype)
                    else:
                        h = stored[step[b], which, 0, env[b]].view(1, 1, hidden)
                        c = stored[step[b], which, 1, env[b]].view(1, 1, hidden)
                y, (h, c) = lstm(obs[b].view(1, 1, -1), (h, c))
                outs.append(y.view(hidden))
            latent = mlp(torch.stack(outs))
            return latent, head(latent)

        def packed(grad):
            parts = []
            for name in names:
                if name == "log_std":
                    tensor = log_std.grad if grad else log_std.detach()
                    parts.append(tensor.t().reshape(-1))
                    continue
                key, part = name.rsplit(".", 1)
                tensor = getattr(modules[key], part)
                tensor = tensor.grad if grad else tensor.detach()
                parts.append((tensor.t() if part.startswith("weight") else tensor).reshape(-1))
            return torch.cat(parts).numpy().copy()

        index = torch.from_numpy(row)
        actions, old, advantages, returns = (torch.from_numpy(data[k]).to(dtype)[index] for k in
                                             ("actions", "old_log_probs", "advantages", "returns"))
        parameters = [p for lstm, mlp, head in nets for p in
                      list(lstm.parameters()) + list(mlp.parameters()) + list(head.parameters())] + [log_std]
        optimizer = torch.optim.Adam(parameters, lr=learning_rate, eps=1e-5)
        for update in range(updates):
            adv = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
            latent, mean = forward(0)
            distribution = _torch_gaussian(torch, latent, mean, log_std)
            log_prob = distribution.log_prob(actions[:, None])[:, 0]
            ratio = torch.exp(log_prob - old)
            policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
            value_loss = torch.nn.functional.mse_loss(returns, forward(1)[1].flatten())
            loss = policy_loss + ent_coef * -distribution.entropy().mean() + vf_coef * value_loss
            optimizer.zero_grad()
            loss.backward()
            if update == 0:
                out["grad" + label] = packed(True)
                out["clip_fraction" + label] = (torch.abs(ratio - 1) > clip_range).to(torch.float64).mean().numpy()
            torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)
            optimizer.step()
            if update == 0:
                out["first" + label] = packed(False)
        out["last" + label] = packed(False)
    np.savez(path_out, **out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "--torch-sequence":
        torch_sequence(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "--torch-lstm-sde-learner":
        torch_learner(sys.argv[2], sys.argv[3])
    else:
        run_cases(sys.argv[1])
