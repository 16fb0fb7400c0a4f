"""TEST INFRASTRUCTURE: what tests/test_lstm_critic_logic.py and tests/test_gpu_lstm_critic.py share -- the recurrent
policies with a feed-forward critic (enable_critic_lstm=False; include/reinfocus_hip.h, "lstm critic") under both heads:
the specs, hostile inputs whose vf half of every state is NaN, the twins' results (computed once and shared), the host build
tests/lstmcriticcheck -- and the child process of the GPU file.

The inputs are the siblings' (tests/lstm_io_cases.py, lstm_learner_io_cases.py, lstm_sde_io_cases.py): their builders take a
spec, so the CPU tests below call them with a spec of this mode.  The child process runs the siblings' OWN device cases
(chains of forwards between guard rows, chained updates on every sequence layout, every refusal, the end-to-end runs, the
back-to-back variants, resume) in this mode: in that process, and only there, the siblings' spec_of builds specs with
enable_critic_lstm=False, their stored states get a NaN vf half, and the context and host library they are handed are
proxies that route every rf_lstm_* call to its rf_lstm_critic_* sibling with critic = RF_LSTM_CRITIC_LINEAR.  Every case is
recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.lstm_critic_io_cases <results.jsonl>
    python -m tests.lstm_critic_io_cases --torch-critic-learner <in.npz> <out.npz>   (torch on the CPU: autograd, Adam)
"""

import ctypes
import functools
import os
import sys

import numpy as np

from tests import learner_io_cases as learner_cases
from tests import lstm_io_cases as lstm_cases
from tests import lstm_learner_io_cases as lstm_learner_cases
from tests import lstm_sde_io_cases as lstm_sde_cases
from tests import policy_io_cases as policy_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = ("categorical", "sde")
NETWORKS = lstm_cases.NETWORKS  # (obs_width, lstm_hidden, pi, vf, n_actions, activation); the sde head has one action
# on the GPU: ppo_lstm_tuned.yml's; widths that are no multiple of a wave, one and two layers mixed; every limit at once
TUNED, ODD, LIMITS = 1, 3, 4
GPU_NETWORKS = (TUNED, ODD, LIMITS)
SIZES = lstm_cases.SIZES  # 1, a tile, one past it, three tiles and a ragged fourth
STEPS = 2  # steps of a CPU chain: the second one starts from a state whose halves are equal
LAYOUTS = lstm_learner_cases.LAYOUTS
UPDATES = learner_cases.UPDATES
hyper_of = learner_cases.hyper_of
bits = lstm_cases.bits
LINEAR = 1  # RF_LSTM_CRITIC_LINEAR


def layouts_of(index):
    return lstm_learner_cases.layouts_of(index)


def limit_layouts_of(index):
    """lstm_learner_io_cases.LIMIT_LAYOUTS for the linear critic, whose forward grid has B + ceil(B / 8) blocks: tuned and
    depth (9 tiles at B = 65 and 68) on both networks below the limits, wave (128 tiles at B = 1024, 65 at 513) on
    ppo_lstm_tuned.yml's alone; the 17-row sequence on the network with every limit."""
    kinds = {TUNED: ("tuned", "depth", "wave"), ODD: ("tuned", "depth")}.get(index, ())
    if index == LIMITS:
        return ["depth/0/17"]
    return [name for name in lstm_learner_cases.LIMIT_LAYOUTS if name.split("/")[0] in kinds and name != "depth/0/17"]


def spec_of(head, network, enable_critic_lstm=False, log_std_init=0.0):
    from reinfocus_amd.environments import lstm, lstm_sde

    width, hidden, pi, vf, actions, activation = network
    if head == "sde":
        return lstm_sde.LstmSdePolicySpec(width, lstm_hidden=hidden, pi=pi, vf=vf, activation=activation,
                                          log_std_init=log_std_init, enable_critic_lstm=enable_critic_lstm)
    return lstm.LstmPolicySpec(width, actions, lstm_hidden=hidden, pi=pi, vf=vf, activation=activation,
                               enable_critic_lstm=enable_critic_lstm)


def state_dict(head, spec, seed, hostile=False):
    """The siblings' state_dicts (they follow spec.entries, so critic.weight / critic.bias are drawn as any layer is)."""
    if head == "sde":
        return lstm_sde_cases.state_dict(spec, seed, hostile)
    return lstm_cases.state_dict(spec, seed, hostile)


def nan_vf_half(state):
    """A copy whose vf half (index 1 of the nets axis, the third from the end being [2 nets][2][n][H]) is NaN throughout."""
    state = np.array(state, dtype=np.float32, copy=True)
    state[..., 1, :, :, :] = np.nan
    return state


# ---- the forward -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_inputs(head, index, n):
    """(spec, params, obs [STEPS, n, D], final_obs alike (NaN-led rows among them), starts uint8 [STEPS, n] (bytes 0, 1, 2,
    255), state [2, 2, n, H]): the siblings' hostile inputs, the vf half of the state NaN throughout."""
    network = NETWORKS[index]
    spec = spec_of(head, network)
    params = spec.pack(state_dict(head, spec, 100 + index, hostile=True))
    obs = np.stack([policy_cases.hostile_rows(network[0], n, 1000 * index + n + 31 * s, False) for s in range(STEPS)])
    final_obs = np.stack([policy_cases.hostile_rows(network[0], n, 7 + n + 17 * s, True) for s in range(STEPS)])
    state = nan_vf_half(lstm_cases.hostile_state(spec, n, 9 * index + n))
    return spec, params, obs, final_obs, lstm_cases.hostile_starts(n, max(STEPS, 4), 50 * index + n)[:STEPS], state


def chain_noise(head, index, n, mode):
    """What a sampled call draws from: (u float64 [STEPS, n], None) or (None, theta float32 [n, L]); (None, None) else."""
    from reinfocus_amd.environments import sde

    if mode != "sampled":
        return None, None
    spec, params = chain_inputs(head, index, n)[:2]
    generator = policy_cases.generator_at(0)[1]
    if head == "sde":
        return None, sde.noise_numpy(params[spec.log_std_at:], generator.random(n * spec.latent))
    return generator.random((STEPS, n)), None


def twin_forward(head, spec, params, obs, starts, state, final_obs, u, theta, deterministic, values_only=False):
    from reinfocus_amd.environments import lstm, lstm_sde

    if head == "sde":
        return lstm_sde.lstm_sde_numpy(spec, params, obs, starts, state, final_obs, theta, deterministic, values_only)
    return lstm.lstm_numpy(spec, params, obs, starts, state, final_obs, u, deterministic, values_only)


@functools.lru_cache(maxsize=None)
def wanted_chain(head, index, n, mode):
    """The twin's STEPS results from chain_inputs, each step from the state of the one before.  Computed once, shared."""
    spec, params, obs, final_obs, starts, state = chain_inputs(head, index, n)
    u, theta = chain_noise(head, index, n, mode)
    steps = []
    for s in range(STEPS):
        steps.append(twin_forward(head, spec, params, obs[s], starts[s], state, final_obs[s], None if u is None else u[s],
                                  theta, mode == "deterministic"))
        state = steps[-1]["state"]
    return steps


# ---- the update ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def update_inputs(head, index, n_steps, num_envs, kind):
    """(spec, packed parameters, batch dict of N rows, episode_starts, lstm_states): the siblings' construction (hostile
    parameters, the stored log-probabilities the twin's own shifted in turn, states of scale 1/2) with the vf half of
    lstm_states NaN throughout."""
    from reinfocus_amd.environments import policy, sde

    network = NETWORKS[index]
    spec = spec_of(head, network)
    hostile = spec.latent > 1 if head == "sde" else True
    params = spec.pack(state_dict(head, spec, 300 + index, hostile=hostile))
    total = n_steps * num_envs
    rng = np.random.default_rng(1000 * index + total)
    starts = lstm_learner_cases.starts_of(kind, n_steps, num_envs)
    states = nan_vf_half(0.5 * rng.standard_normal((n_steps + 1,) + spec.state_shape(num_envs)))
    batch = {"observations": learner_cases.finite_rows(network[0], total, 77 * index + total)}
    if head == "categorical":
        batch["actions"] = rng.integers(0, spec.n_actions, total).astype(np.int64)
    batch["advantages"] = rng.standard_normal(total).astype(np.float32)
    batch["returns"] = rng.standard_normal(total).astype(np.float32)
    shifts = np.array(learner_cases.SHIFTS, dtype=np.float32)[np.arange(total) % len(learner_cases.SHIFTS)]
    if head == "sde":
        mu, sigma, h = lstm_sde_cases.own_head(spec, params, batch, starts, states, n_steps, num_envs)
        theta = sde.noise_numpy(params[spec.log_std_at:], rng.random(total * spec.latent))
        with np.errstate(all="ignore"):
            batch["actions"] = policy.canonical(mu + sde._rowdot(h, theta))
        own = sde.log_prob_of(batch["actions"], mu, sigma)
    else:
        own = lstm_learner_cases.own_log_probs(spec, params, batch, starts, states, n_steps, num_envs)
    batch["log_probs"] = (own - shifts).astype(np.float32)
    assert np.isfinite(batch["log_probs"]).all() and np.isnan(states[:, 1]).all()
    return spec, params, batch, starts, states


def layout_inputs(head, index, name):
    n_steps, num_envs, kind, first, count = LAYOUTS[name]
    return update_inputs(head, index, n_steps, num_envs, kind) + (n_steps, num_envs, first, count)


def twin_update(spec, params, state, batch, starts, states, n_steps, num_envs, first, count, hyper):
    """(params, state, stats, the gradient before clipping) of one update by the numpy twin."""
    from reinfocus_amd.environments import lstm_learner

    grad = lstm_learner.lstm_gradient_numpy(spec, params, batch, starts, states, n_steps, num_envs, first, count, hyper)[0]
    return lstm_learner.lstm_update_numpy(spec, params, state, batch, starts, states, n_steps, num_envs, first, count,
                                          hyper) + (grad,)


@functools.lru_cache(maxsize=None)
def twin_updates(head, index, name):
    """[(params, state, stats, gradient)] after each of UPDATES consecutive updates with changing hyper-parameters."""
    from reinfocus_amd.environments import learner

    spec, params, batch, starts, states, n_steps, num_envs, first, count = layout_inputs(head, index, name)
    state = learner.fresh_state(spec)
    seen = []
    for update in range(UPDATES):
        seen.append(twin_update(spec, params, state, batch, starts, states, n_steps, num_envs, first, count, hyper_of(update)))
        params, state = seen[-1][0], seen[-1][1]
    return seen


# ---- the host build ------------------------------------------------------------------------------------------------------------
def hostcheck():
    from tests import helpers

    lib = ctypes.CDLL(helpers.built("tests/lstmcriticcheck", "liblstmcriticcheck.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for name in ("lcc_params_size", "lcc_critic_at", "lcc_state_size", "lcc_workspace_size", "lcc_grad_offset"):
        getattr(lib, name).restype = ctypes.c_ulonglong
    lib.lcc_params_size.argtypes = lib.lcc_state_size.argtypes = [vp, i32]
    lib.lcc_critic_at.argtypes = [vp, i32, vp]
    lib.lcc_workspace_size.argtypes = lib.lcc_grad_offset.argtypes = [vp, i32, i32]
    lib.lcc_forward.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.lcc_update.argtypes = [vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    return lib


def critic_desc(spec, critic=None):
    from reinfocus_amd import _native

    desc = spec.critic_desc()
    return _native.LstmCriticDesc(*(desc if critic is None else desc[:10] + (critic,)))


def host_forward(lib, head, spec, params, obs, starts, state, final_obs, gen, theta, deterministic, values_only=False):
    """lcc_forward on copies: the dict of the twins (the keys of the head), "state" None with values_only."""
    from reinfocus_amd.environments import policy

    n = obs.shape[0]
    sde = head == "sde"
    f32 = lambda *shape: np.zeros(shape, dtype=np.float32)  # noqa: E731
    out = {"values": f32(n), "final_values": None if final_obs is None else f32(n)}
    pi = {} if values_only else {"actions": f32(n) if sde else np.zeros(n, dtype=np.int64), "log_probs": f32(n),
                                 "logits": f32(n) if sde else f32(n, spec.n_actions)}
    if sde and not values_only:
        pi.update(env_actions=f32(n), sigma=f32(n))
    state_out = None if values_only else f32(*spec.state_shape(n))
    pointer = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    arrays = [np.ascontiguousarray(a) for a in (params, obs, starts)] + [np.ascontiguousarray(state, dtype=np.float32)]
    final = None if final_obs is None else np.ascontiguousarray(final_obs)
    words = None if gen is None else (ctypes.c_ulonglong * 4)(*gen)
    theta = None if theta is None else np.ascontiguousarray(theta)
    rc = lib.lcc_forward(ctypes.byref(critic_desc(spec)), int(sde), arrays[0].ctypes.data, n, arrays[1].ctypes.data,
                         arrays[2].ctypes.data, pointer(final), arrays[3].ctypes.data, pointer(state_out), words,
                         policy.DETERMINISTIC if deterministic else 0, pointer(theta), pointer(pi.get("actions")),
                         pointer(pi.get("env_actions")), pointer(pi.get("log_probs")), out["values"].ctypes.data,
                         pointer(out["final_values"]), pointer(pi.get("logits")), pointer(pi.get("sigma")))
    assert rc == 0
    out.update(pi)
    if sde and not values_only:
        out["mean"] = out.pop("logits")
    out["state"] = state_out
    return out


def host_update(lib, head, spec, params, state, batch, starts, states, n_steps, num_envs, first, count, hyper):
    """lcc_update on copies: (params, state, stats, the packed gradient before clipping)."""
    from reinfocus_amd import _native
    from reinfocus_amd.environments import learner

    params, state = params.copy(), state.copy()
    stats, grad = np.zeros(8, dtype=np.float32), np.zeros(spec.size, dtype=np.float32)
    arrays = [np.ascontiguousarray(batch[key]) for key in learner.BATCH_KEYS]
    starts, states = np.ascontiguousarray(starts, dtype=np.uint8), np.ascontiguousarray(states, dtype=np.float32)
    rc = lib.lcc_update(ctypes.byref(critic_desc(spec)), int(head == "sde"), ctypes.byref(_native.PpoDesc(*hyper)),
                        params.ctypes.data, state.ctypes.data, n_steps, num_envs, *(a.ctypes.data for a in arrays),
                        starts.ctypes.data, states.ctypes.data, first, count, stats.ctypes.data, grad.ctypes.data)
    assert rc == 0
    return params, state, stats, grad


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------------
class CriticContext:
    """A _native.Context as the siblings' device cases use it, every recurrent call routed to its rf_lstm_critic_ sibling
    with critic = RF_LSTM_CRITIC_LINEAR (the desc the cases hand in is rf_lstm_policy_desc's ten integers)."""

    def __init__(self, ctx):
        self._ctx = ctx

    def lstm_params_size(self, desc):
        return self._ctx.lstm_critic_params_size(tuple(desc) + (LINEAR,))

    def lstm_sde_params_size(self, desc):
        return self._ctx.lstm_critic_params_size(tuple(desc) + (LINEAR,), sde=True)

    def lstm_state_size(self, desc, num_envs):
        return self._ctx.lstm_state_size(desc, num_envs)  # (the state keeps its shape: no sibling)

    def lstm_ppo_state_size(self, desc):
        return self._ctx.lstm_critic_state_size(tuple(desc) + (LINEAR,))

    def lstm_sde_state_size(self, desc):
        return self._ctx.lstm_critic_state_size(tuple(desc) + (LINEAR,), sde=True)

    def lstm_ppo_workspace_size(self, desc, max_batch):
        return self._ctx.lstm_critic_workspace_size(tuple(desc) + (LINEAR,), max_batch)

    def lstm_sde_workspace_size(self, desc, max_batch):
        return self._ctx.lstm_critic_workspace_size(tuple(desc) + (LINEAR,), max_batch, sde=True)

    def lstm_forward(self, desc, *args):
        self._ctx.lstm_critic_forward(tuple(desc) + (LINEAR,), *args)

    def lstm_sde_forward(self, desc, *args):
        self._ctx.lstm_critic_sde_forward(tuple(desc) + (LINEAR,), *args)

    def lstm_sde_noise_reset(self, desc, *args):
        self._ctx.lstm_critic_sde_noise_reset(tuple(desc) + (LINEAR,), *args)

    def lstm_ppo_update(self, desc, *args):
        self._ctx.lstm_critic_ppo_update(tuple(desc) + (LINEAR,), *args)

    def lstm_sde_update(self, desc, *args):
        self._ctx.lstm_critic_sde_update(tuple(desc) + (LINEAR,), *args)


class CriticLib:
    """tests/lstmcriticcheck under the names the siblings' device cases ask their host builds for (the workspace layout)."""

    def __init__(self, lib):
        self._lib = lib

    def _desc(self, reference):
        from reinfocus_amd import _native

        lstm = reference._obj  # (a byref of an rf_lstm_policy_desc)
        policy = lstm.policy
        return _native.LstmCriticDesc(policy.obs_width, policy.n_actions, policy.activation, policy.pi_layers,
                                      *policy.pi_width, policy.vf_layers, *policy.vf_width, lstm.lstm_hidden, LINEAR)

    def lpc_grad_offset(self, reference, count):
        return self._lib.lcc_grad_offset(ctypes.byref(self._desc(reference)), 0, count)

    def lsc_grad_offset(self, reference, count):
        return self._lib.lcc_grad_offset(ctypes.byref(self._desc(reference)), 1, count)

    def lsc_workspace_size(self, reference, count):
        return self._lib.lcc_workspace_size(ctypes.byref(self._desc(reference)), 1, count)


def _in_this_mode():
    """The siblings' case modules build their specs with enable_critic_lstm=False and hand the update a NaN vf half, in
    this (child) process only; nothing of theirs has been computed yet."""
    def categorical(network):
        return spec_of("categorical", network)

    def gaussian(network, log_std_init=0.0):
        width, hidden, pi, vf, activation = network
        return spec_of("sde", (width, hidden, pi, vf, 1, activation), log_std_init=log_std_init)

    lstm_cases.spec_of = lstm_learner_cases.spec_of = categorical
    lstm_sde_cases.spec_of = gaussian
    hostile_state = lstm_cases.hostile_state
    lstm_cases.hostile_state = lambda spec, n, seed: nan_vf_half(hostile_state(spec, n, seed))
    for module in (lstm_learner_cases, lstm_sde_cases):
        def poisoned(index, n_steps, num_envs, kind, original=module.update_inputs):
            spec, params, batch, starts, states = original(index, n_steps, num_envs, kind)
            assert not spec.enable_critic_lstm
            return spec, params, batch, starts, nan_vf_half(states)

        module.update_inputs = functools.lru_cache(maxsize=None)(poisoned)


def critic_value_case(torch, ctx):
    """Every entry point refuses critic = 2 and critic = -1 with all bytes unchanged, sizes are 0; with
    RF_LSTM_CRITIC_LSTM the siblings ARE the rf_lstm_ entry points: the same bytes from the same call."""
    from reinfocus_amd.environments import learner

    stream = torch.cuda.current_stream().cuda_stream
    for head in HEADS:
        sde = head == "sde"
        n = lstm_cases.TILE + 1
        spec, params_h, obs_h, final_h, starts_h, state_h = chain_inputs(head, TUNED, n)
        desc = spec.critic_desc()
        params, obs, starts, state = (torch.from_numpy(a).cuda() for a in (params_h, obs_h[0], starts_h[0], state_h))
        values = torch.full((n,), 7.0, device="cuda")
        target = torch.full_like(state, 7.0)
        name = f"mixed/3/{lstm_cases.TILE + 1}"
        _, uparams_h, batch, ustarts, ustates, n_steps, num_envs, first, count = layout_inputs(head, TUNED, name)
        device = {key: torch.from_numpy(value).cuda() for key, value in batch.items()}
        uparams, slab, slab_starts = (torch.from_numpy(a).cuda() for a in (uparams_h, ustates, ustarts))
        optimizer = torch.from_numpy(learner.fresh_state(spec)).cuda()
        workspace = torch.zeros(ctx.lstm_critic_workspace_size(desc, count, sde=sde) // 4, device="cuda")
        stats = torch.full((8,), 7.0, device="cuda")
        for critic in (2, -1):
            bad = desc[:10] + (critic,)
            assert ctx.lstm_critic_params_size(bad, sde=sde) == 0 and ctx.lstm_critic_state_size(bad, sde=sde) == 0
            assert ctx.lstm_critic_workspace_size(bad, count, sde=sde) == 0
            calls = [lambda: (ctx.lstm_critic_sde_forward if sde else ctx.lstm_critic_forward)(
                         bad, params.data_ptr(), n, obs.data_ptr(), starts.data_ptr(), None, state.data_ptr(),
                         target.data_ptr(), None, 1, *((None,) * 3 if sde else (None, None)), values.data_ptr(), None,
                         *((None, None) if sde else (None,)), stream),
                     lambda: (ctx.lstm_critic_sde_update if sde else ctx.lstm_critic_ppo_update)(
                         bad, tuple(hyper_of(0)), uparams.data_ptr(), optimizer.data_ptr(), workspace.data_ptr(), n_steps,
                         num_envs, device["observations"].data_ptr(), device["actions"].data_ptr(),
                         device["log_probs"].data_ptr(), device["advantages"].data_ptr(), device["returns"].data_ptr(),
                         slab_starts.data_ptr(), slab.data_ptr(), first, count, stats.data_ptr(), stream)]
            if sde:
                theta = torch.full((n, spec.latent), 7.0, device="cuda")
                calls.append(lambda: ctx.lstm_critic_sde_noise_reset(bad, params.data_ptr(), n, (1, 2, 3, 5), theta.data_ptr(),
                                                                     stream))
            for call in calls:
                try:
                    call()
                except AssertionError as caught:  # (RF_ERR_INVALID)
                    assert "outside the limits" in str(caught), str(caught)
                else:
                    raise AssertionError(f"critic = {critic} was taken")
            torch.cuda.synchronize()
            assert (values == 7.0).all() and (target == 7.0).all() and (stats == 7.0).all()
            assert bits(uparams.cpu().numpy()) == bits(uparams_h) and not optimizer.any() and not workspace.any()
            assert not sde or (theta == 7.0).all()
        # ... and unchanged, in this mode, the calls are taken: the twin's bytes
        want = wanted_chain(head, TUNED, n, "deterministic")[0]
        (ctx.lstm_critic_sde_forward if sde else ctx.lstm_critic_forward)(
            desc, params.data_ptr(), n, obs.data_ptr(), starts.data_ptr(), None, state.data_ptr(), target.data_ptr(), None, 1,
            *((None,) * 3 if sde else (None, None)), values.data_ptr(), None, *((None, None) if sde else (None,)), stream)
        torch.cuda.synchronize()
        assert bits(values.cpu().numpy()) == bits(want["values"]) and bits(target.cpu().numpy()) == bits(want["state"])
        assert bits(target[0].cpu().numpy()) == bits(target[1].cpu().numpy()), "the halves of the stored state differ"
        # the LSTM mode through the sibling equals the rf_lstm_ entry point itself (a spec of that mode, the same inputs)
        both = spec_of(head, NETWORKS[TUNED], enable_critic_lstm=True)
        weights = torch.from_numpy(both.pack(state_dict(head, both, 100 + TUNED, hostile=True))).cuda()
        clean = torch.from_numpy(lstm_cases.hostile_state(both, n, 9 * TUNED + n)).cuda()
        got = []
        for forward, lstm_desc in (((ctx.lstm_sde_forward if sde else ctx.lstm_forward), both.desc()),
                                   ((ctx.lstm_critic_sde_forward if sde else ctx.lstm_critic_forward), both.critic_desc())):
            values.fill_(7.0), target.fill_(7.0)
            forward(lstm_desc, weights.data_ptr(), n, obs.data_ptr(), starts.data_ptr(), None, clean.data_ptr(),
                    target.data_ptr(), None, 1, *((None,) * 3 if sde else (None, None)), values.data_ptr(), None,
                    *((None, None) if sde else (None,)), stream)
            torch.cuda.synchronize()
            got.append((bits(values.cpu().numpy()), bits(target.cpu().numpy())))
        assert got[0] == got[1] and both.critic_desc()[10] == 0


def value_path_case(torch, ctx):
    """The value path ignores state and starts on the device: with the state all NaN and every start byte 0, values and
    final_values of a values-only call are finite and byte-equal to those with a zero state and every start byte 1, with and
    without final_obs, and equal the twin's."""
    stream = torch.cuda.current_stream().cuda_stream
    for head in HEADS:
        sde = head == "sde"
        for index in GPU_NETWORKS:
            n = lstm_cases.TILE + 1
            spec, params_h, obs_h, _, _, _ = chain_inputs(head, index, n)
            finite = np.nan_to_num(obs_h, nan=0.25, posinf=3.0, neginf=-3.0)
            params, obs, final_obs = (torch.from_numpy(a).cuda() for a in (params_h, finite[0], finite[1]))
            forward = ctx.lstm_critic_sde_forward if sde else ctx.lstm_critic_forward
            seen = []
            for fill, byte in ((float("nan"), 0), (0.0, 1)):
                state = torch.full(spec.state_shape(n), fill, device="cuda")
                starts = torch.full((n,), byte, dtype=torch.uint8, device="cuda")
                for with_final in (True, False):
                    values, final_values = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
                    forward(spec.critic_desc(), params.data_ptr(), n, obs.data_ptr(), starts.data_ptr(),
                            final_obs.data_ptr() if with_final else None, state.data_ptr(), None, None, 0,
                            *((None,) * 3 if sde else (None, None)), values.data_ptr(),
                            final_values.data_ptr() if with_final else None, *((None, None) if sde else (None,)), stream)
                    torch.cuda.synchronize()
                    seen.append((bits(values.cpu().numpy()), bits(final_values.cpu().numpy())))
                    assert torch.isfinite(values).all() and torch.isfinite(final_values).all()
            assert seen[0] == seen[2] and seen[1] == seen[3] and seen[0][0] == seen[1][0]
            want = twin_forward(head, spec, params_h, finite[0], np.ones(n, np.uint8), np.zeros(spec.state_shape(n), np.float32),
                                finite[1], None, None, True, values_only=True)
            assert seen[0] == (bits(want["values"]), bits(want["final_values"]))


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    _in_this_mode()
    record = cases.Recorder(path)
    real = _native.Context(0)
    ctx, lib = CriticContext(real), CriticLib(hostcheck())
    for index in GPU_NETWORKS:
        for n in SIZES:
            with record.case(f"forward/categorical/{index}/{n}"):
                lstm_cases.kernel_case(torch, ctx, index, n)
            with record.case(f"forward/sde/{index}/{n}"):
                lstm_sde_cases.noise_case(torch, ctx, index, n)
                lstm_sde_cases.kernel_case(torch, ctx, index, n)
    with record.case("value-path"):
        value_path_case(torch, real)
    for index in GPU_NETWORKS:
        for name in layouts_of(index) + limit_layouts_of(index):
            with record.case(f"update/categorical/{index}/{name}"):
                lstm_learner_cases.kernel_case(torch, ctx, lib, index, name)
            with record.case(f"update/sde/{index}/{name}"):
                lstm_sde_cases.update_case(torch, ctx, lib, index, name)
    with record.case("refusals/categorical/forward"):
        lstm_cases.refusal_case(torch, ctx)
    with record.case("refusals/categorical/update"):
        lstm_learner_cases.refusal_case(torch, ctx, lib)
    with record.case("refusals/sde/forward"):
        lstm_sde_cases.forward_refusal_case(torch, ctx)
    with record.case("refusals/sde/update"):
        lstm_sde_cases.update_refusal_case(torch, ctx, lib)
    with record.case("refusals/critic"):
        critic_value_case(torch, real)
    real.close()
    for head, module in (("categorical", lstm_learner_cases), ("sde", lstm_sde_cases)):
        for n in lstm_learner_cases.E2E_SIZES:
            with record.case(f"end-to-end/{head}/{n}"):
                module.end_to_end_case(torch, "view", n)
        with record.case(f"no-sync/{head}"):
            module.no_sync_case(torch)
        with record.case(f"resume/{head}"):
            module.resume_case(torch)
    with record.case("finished"):
        pass


# ---- torch on the CPU: the actor's LSTM stepped per row, nn.Linear for `critic`, autograd, clip_grad_norm_ and Adam ------------
def torch_critic_learner(path_in, path_out):
    """From a state_dict of this mode, a rollout and one minibatch: the forward's logits (the mean with the Gaussian head)
    and values, the packed gradient before clipping, the same with the `critic` layer left out of the graph (its output
    detached: float64 only), and the packed parameters after 1 and after `updates` updates, in float64 and in float32.
    torch.nn.LSTM cells stepped per row for the actor, with the sequence rule and the select of the definition; the stored
    states are constants; the value path is critic -> MLP -> value_net on the observations alone.  In a process of its own."""
    import torch

    data = np.load(path_in)
    names = [str(name) for name in data["names"]]
    gaussian = "log_std" in names
    activation = torch.nn.Tanh if str(data["activation"]) == "tanh" else torch.nn.ReLU
    clip_range, ent_coef, vf_coef, max_grad_norm, learning_rate = (float(data[k]) for k in (
        "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "learning_rate"))
    updates = int(data["updates"])
    row, env, step, is_start, zero = (data[k] for k in ("row", "env", "step", "is_start", "zero"))
    out = {}
    for label, dtype in (("64", torch.float64), ("32", torch.float32)):
        tensors = {name: torch.from_numpy(data[name]).to(dtype) for name in names}
        stored = torch.from_numpy(data["lstm_states"]).to(dtype)  # (no gradient: a constant; only the pi half is read)
        obs = torch.from_numpy(data["obs"]).to(dtype)[torch.from_numpy(row)]
        hidden = stored.shape[-1]
        modules = {}

        def linear_of(key):
            weight = tensors[key + ".weight"]
            layer = torch.nn.Linear(weight.shape[1], weight.shape[0]).to(dtype)
            with torch.no_grad():
                layer.weight.copy_(weight)
                layer.bias.copy_(tensors[key + ".bias"])
            modules[key] = layer
            return layer

        def mlp_of(extractor, head_name):
            layers = []
            keys = [f"mlp_extractor.{extractor}.{i}" for i in (0, 2) if f"mlp_extractor.{extractor}.{i}.weight" in tensors]
            for key in keys:
                layers += [linear_of(key), activation()]
            return torch.nn.Sequential(*layers), linear_of(head_name)

        lstm = torch.nn.LSTM(obs.shape[1], hidden, num_layers=1).to(dtype)
        lstm.load_state_dict({part: tensors[f"lstm_actor.{part}"] for part in
                              ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
        modules["lstm_actor"] = lstm
        pi_mlp, pi_head = mlp_of("policy_net", "action_net")
        critic = linear_of("critic")
        vf_mlp, vf_head = mlp_of("value_net", "value_net")
        log_std = None
        if gaussian:
            log_std = torch.nn.Parameter(tensors["log_std"].clone())  # [L, 1]

        def actor():
            outs = []
            h = c = None
            for b in range(len(row)):
                if is_start[b]:
                    if zero[b]:
                        h = torch.zeros(1, 1, hidden, dtype=dtype)
                        c = torch.zeros(1, 1, hidden, dtype=dtype)
                    else:
                        h = stored[step[b], 0, 0, env[b]].view(1, 1, hidden)
                        c = stored[step[b], 0, 1, env[b]].view(1, 1, hidden)
                y, (h, c) = lstm(obs[b].view(1, 1, -1), (h, c))
                outs.append(y.view(hidden))
            latent = pi_mlp(torch.stack(outs))
            return latent, pi_head(latent)

        def values_of(without_critic):
            latent = critic(obs)
            return vf_head(vf_mlp(latent.detach() if without_critic else latent)).flatten()

        def packed(grad):
            parts = []
            for name in names:
                if name == "log_std":
                    tensor = log_std.grad if grad else log_std.detach()
                    parts.append(tensor.reshape(-1))  # ([L, 1]: its transpose has the same order)
                    continue
                key, part = name.rsplit(".", 1)
                tensor = getattr(modules[key], part)
                tensor = tensor.grad if grad else tensor.detach()
                if tensor is None:  # (a layer left out of the graph)
                    tensor = torch.zeros_like(getattr(modules[key], part))
                parts.append((tensor.t() if part.startswith("weight") else tensor).reshape(-1))
            return torch.cat(parts).numpy().copy()

        index = torch.from_numpy(row)
        actions = torch.from_numpy(data["actions"])[index]
        old, advantages, returns = (torch.from_numpy(data[k]).to(dtype)[index] for k in
                                    ("old_log_probs", "advantages", "returns"))
        parameters = [p for module in modules.values() for p in module.parameters()] + ([log_std] if gaussian else [])
        optimizer = torch.optim.Adam(parameters, lr=learning_rate, eps=1e-5)

        def loss_of(without_critic):
            adv = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
            latent, head = actor()
            if gaussian:  # (stable-baselines3's StateDependentNoiseDistribution: full_std, learn_features=False, epsilon 1e-6)
                variance = torch.mm(latent.detach() ** 2, torch.exp(log_std) ** 2)
                distribution = torch.distributions.Normal(head, torch.sqrt(variance + 1e-6))
                log_prob = distribution.log_prob(actions.to(dtype).view(-1, 1)).sum(dim=1)
                entropy = distribution.entropy().sum(dim=1)
            else:
                distribution = torch.distributions.Categorical(logits=head)
                log_prob = distribution.log_prob(actions)
                entropy = distribution.entropy()
            ratio = torch.exp(log_prob - old)
            policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
            value_loss = torch.nn.functional.mse_loss(returns, values_of(without_critic))
            return policy_loss + ent_coef * -entropy.mean() + vf_coef * value_loss, ratio, head

        if label == "64":
            optimizer.zero_grad()
            loss_of(True)[0].backward()
            out["grad_without64"] = packed(True)
        for update in range(updates):
            loss, ratio, head = loss_of(False)
            optimizer.zero_grad()
            loss.backward()
            if update == 0:
                out["grad" + label] = packed(True)
                out["head" + label] = head.detach().numpy().copy()
                out["values" + label] = values_of(False).detach().numpy().copy()
                out["clip_fraction" + label] = (torch.abs(ratio - 1) > clip_range).to(torch.float64).mean().numpy()
            torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)
            optimizer.step()
            if update == 0:
                out["first" + label] = packed(False)
        out["last" + label] = packed(False)
    np.savez(path_out, **out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "--torch-critic-learner":
        torch_critic_learner(sys.argv[2], sys.argv[3])
    else:
        run_cases(sys.argv[1])
