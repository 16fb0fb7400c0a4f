"""CPU tests of the recurrent sde policy's definition (include/reinfocus_hip.h, "lstm sde policy" and "lstm sde update"):
the numpy twins (lstm_sde.lstm_sde_numpy, lstm_learner.lstm_update_numpy with an LstmSdePolicySpec) against the host
build of the kernels' own headers (tests/lstmsdecheck) as bytes, on the networks, sizes and layouts of the GPU tests;
against torch in float64 (nn.LSTM followed by the Gaussian written out from its definition, autograd, clip_grad_norm_,
Adam) on the CPU; hostile rows; the Python surface and its refusals; the binding; the stand-alone host program.

The float64 comparisons print both distances; the factor is 4, what tests/test_lstm_logic.py and tests/test_sde_logic.py
hold for the forward and tests/test_lstm_learner_logic.py and tests/test_sde_logic.py for gradients."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, learner, lstm, lstm_learner, lstm_sde, policy, sde
from tests import helpers
from tests import lstm_io_cases as lstm_cases
from tests import lstm_sde_io_cases as cases
from tests import rollout_io_cases as rollout_cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FACTOR = 4.0  # (the siblings' factor for the same quantities)
bits = cases.bits
NETWORK_IDS = ["-".join(str(v) for v in network) for network in cases.NETWORKS]


@pytest.fixture(scope="module")
def hostcheck():
    return cases.hostcheck()


def desc_of(spec):
    return ctypes.byref(_native.LstmPolicyDesc(*spec.desc()))


def host_noise(lib, spec, params, n, bit_generator):
    theta = np.zeros((n, spec.latent), dtype=F32)
    words = (ctypes.c_ulonglong * 4)(*policy.generator_words(bit_generator))
    assert lib.lsc_noise(desc_of(spec), params.ctypes.data, n, words, theta.ctypes.data) == 0
    return theta


def host_forward(lib, spec, params, obs, starts, final_obs, state, theta, names=cases.OUTPUTS, with_state=True):
    """lsc_forward on copies: ({name: float32 [n]}, the next state or None)."""
    n = obs.shape[0]
    out = {name: np.zeros(n, dtype=F32) for name in names}
    state_in = np.ascontiguousarray(state, dtype=F32)
    state_out = np.zeros_like(state_in) if with_state else None
    pointer = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    arrays = [np.ascontiguousarray(obs), np.ascontiguousarray(starts, dtype=np.uint8),
              None if final_obs is None else np.ascontiguousarray(final_obs), state_in, state_out,
              None if theta is None else np.ascontiguousarray(theta)]
    rc = lib.lsc_forward(desc_of(spec), params.ctypes.data, n, *(pointer(a) for a in arrays),
                         *(pointer(out.get(name)) for name in cases.OUTPUTS))
    assert rc == 0
    return out, state_out


def host_update(lib, spec, params, state, batch, starts, states, n_steps, num_envs, first, count, hyper):
    """lsc_update on copies: (params, state, stats, the packed gradient before clipping)."""
    params, state = params.copy(), state.copy()
    stats, grad = np.zeros(8, dtype=F32), np.zeros(spec.size, dtype=F32)
    arrays = [np.ascontiguousarray(batch[key]) for key in learner.BATCH_KEYS]
    assert arrays[1].dtype == F32
    starts, states = np.ascontiguousarray(starts, dtype=np.uint8), np.ascontiguousarray(states, dtype=F32)
    rc = lib.lsc_update(desc_of(spec), ctypes.byref(_native.PpoDesc(*hyper)), params.ctypes.data, state.ctypes.data, n_steps,
                        num_envs, *(a.ctypes.data for a in arrays), starts.ctypes.data, states.ctypes.data, first, count,
                        stats.ctypes.data, grad.ctypes.data)
    assert rc == 0
    return params, state, stats, grad


def same(got, want, what):
    for name, x, y in zip(("params", "state", "stats", "gradient"), got, want):
        assert bits(x) == bits(y), f"{what}: {name} differ"


# ---- 1: the twins against the host build ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=NETWORK_IDS)
def test_layout_of_the_header_is_the_spec_s(index, hostcheck):
    """P + L floats, log_std last of everything; the optimizer state is 32 + 8 (P + L) bytes."""
    spec = cases.spec_of(cases.NETWORKS[index])
    categorical = lstm.LstmPolicySpec(spec.obs_width, 2, spec.lstm_hidden, spec.pi, spec.vf, spec.activation)
    latent = ctypes.c_int(0)
    assert hostcheck.lsc_params_size(desc_of(spec)) == spec.size == categorical.size - spec.pi[-1] - 1 + spec.latent
    assert hostcheck.lsc_log_std(desc_of(spec), ctypes.byref(latent)) == spec.log_std_at == spec.size - spec.latent
    assert latent.value == spec.latent == spec.pi[-1]
    assert hostcheck.lsc_state_size(desc_of(spec)) == 32 + 8 * spec.size
    assert spec.keys()[-1] == "log_std" and spec.keys()[0] == "lstm_actor.weight_ih_l0"
    for actions in (0, 2, 13):  # (any n_actions other than 1 is refused)
        wrong = _native.LstmPolicyDesc(*(spec.desc()[:1] + (actions,) + spec.desc()[2:]))
        assert hostcheck.lsc_params_size(ctypes.byref(wrong)) == 0
    state = cases.state_dict(spec, index, hostile=True)
    packed = spec.pack(state)
    back = spec.unpack(packed)
    assert all(bits(back[name]) == bits(state[name]) for name in state) and back["log_std"].shape == (spec.latent, 1)
    assert bits(packed[spec.log_std_at:]) == bits(state["log_std"][:, 0])


@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=NETWORK_IDS)
def test_forward_of_the_header_equals_the_twin(index, hostcheck):
    """The chains of the GPU tests (5 steps, hostile rows and states, start bytes 0, 1, 2 and 255), sampled at both draw
    offsets and deterministic: theta, every output and the state as bytes; then the subsets of outputs."""
    for n in cases.sizes_of(index):
        spec, params, obs, final_obs, starts, state = cases.chain_inputs(index, n)
        for mode, offset in cases.MODES:
            want = cases.wanted_chain(index, n, mode, offset)
            theta = None
            if mode == "sampled":
                theta = host_noise(hostcheck, spec, params, n, cases.generator_at(offset)[0])
                assert bits(theta) == bits(cases.wanted_theta(index, n, offset)), f"n {n}: theta at {offset}"
            current = state
            for s in range(cases.STEPS):
                got, current = host_forward(hostcheck, spec, params, obs[s], starts[s], final_obs[s], current, theta)
                for name in cases.OUTPUTS:
                    assert bits(got[name]) == bits(want[s][name]), f"n {n}, {mode} at {offset}, step {s}: {name}"
                assert bits(current) == bits(want[s]["state"]), f"n {n}, {mode} at {offset}, step {s}: the state"
        sampled, theta = cases.wanted_chain(index, n, "sampled", 0)[0], cases.wanted_theta(index, n, 0)
        got, _ = host_forward(hostcheck, spec, params, obs[0], starts[0], None, state, theta, cases.PI_OUTPUTS, False)
        assert all(bits(got[name]) == bits(sampled[name]) for name in cases.PI_OUTPUTS)
        got, _ = host_forward(hostcheck, spec, params, obs[0], starts[0], final_obs[0], state, None, ("values", "final_values"),
                              False)
        assert bits(got["values"]) == bits(sampled["values"]) and bits(got["final_values"]) == bits(sampled["final_values"])
        _, next_state = host_forward(hostcheck, spec, params, obs[0], starts[0], None, state, None, ())
        assert bits(next_state) == bits(sampled["state"])


@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=NETWORK_IDS)
def test_update_of_the_header_equals_the_twin(index, hostcheck):
    """Three chained updates with changing hyper-parameters on every sequence layout of the GPU tests: parameters (log_std
    included), optimizer state, stats and the gradient as bytes."""
    for name in cases.layouts_of(index):
        spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(index, name)
        want = cases.twin_updates(index, name)
        state = learner.fresh_state(spec)
        assert hostcheck.lsc_state_size(desc_of(spec)) == 4 * state.size
        for update in range(cases.UPDATES):
            got = host_update(hostcheck, spec, params, state, batch, starts, states, n_steps, num_envs, first, count,
                              cases.hyper_of(update))
            same(got, want[update], f"{name}, update {update}")
            params, state = got[0], got[1]
        assert learner.state_parts(spec, state)[0] == cases.UPDATES and np.isfinite(want[-1][2]).all()


LIMIT_CASES = [(index, name) for index in range(len(cases.NETWORKS)) for name in cases.limit_layouts_of(index)]


@pytest.mark.parametrize("index,name", LIMIT_CASES, ids=[f"{NETWORK_IDS[index]}-{name}" for index, name in LIMIT_CASES])
def test_update_of_the_header_equals_the_twin_at_the_limits(index, name, hostcheck):
    """The same on the limit layouts of tests/lstm_learner_io_cases.py (whose CPU test asserts their sequence lengths):
    sequences of exactly 8 rows, of 1, 8, 9, 16 and 17, and of more than 64 rows at B = 128, on the H = 16 network; one
    17-row sequence on the network with every limit."""
    spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(index, name)
    want = cases.twin_updates(index, name)
    state = learner.fresh_state(spec)
    for update in range(cases.UPDATES):
        got = host_update(hostcheck, spec, params, state, batch, starts, states, n_steps, num_envs, first, count,
                          cases.hyper_of(update))
        same(got, want[update], f"{name}, update {update}")
        params, state = got[0], got[1]
    assert learner.state_parts(spec, state)[0] == cases.UPDATES and np.isfinite(want[-1][2]).all()
    assert all(stats[7] == 0 for _, _, stats, _ in want)
    assert (np.abs(batch["actions"]) > 1).any()  # (raw actions past +-1 are still among the stored ones)


def test_inputs_hold_what_they_promise():
    """Raw actions past +-1 among the stored ones; a log_std row of -100, 0 and +3; ratios on both sides of the clip
    range; log_std has a gradient; a norm that clips and one that does not."""
    spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(2, "mixed/0/15")
    assert (np.abs(batch["actions"]) > 1).any() and (np.abs(batch["actions"]) < 1).any()
    assert list(params[spec.log_std_at:spec.log_std_at + 3]) == [-100.0, 0.0, 3.0]
    grad, terms, invalid = lstm_learner.lstm_gradient_numpy(spec, params, batch, starts, states, n_steps, num_envs, first,
                                                            count, cases.hyper_of(0))
    assert not invalid and 0 < terms[4].mean() < 1
    assert grad[spec.log_std_at] == 0 and np.abs(grad[spec.log_std_at + 1:]).min() > 0  # (std2 == 0 at -100)
    norms = [stats[5] for _, _, stats, _ in cases.twin_updates(2, "mixed/0/15")]
    schedule = cases.learner_cases.SCHEDULE
    assert norms[1] < schedule[1][0] and norms[2] > schedule[2][0]


# ---- 2: the twins against torch in float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [cases.SMALL, cases.UNTUNED], ids=["small", "untuned"])
def test_forward_is_no_further_from_float64_than_four_times_torch(index, tmp_path):
    """A 16-step sequence of normal rows with three episode starts inside it, from one state_dict and one theta: the
    twin, torch (nn.LSTM, nn.Sequential and Normal(mu, sqrt((h * h) @ exp(log_std) ** 2 + 1e-6))) in float32, and the same
    in float64.  Per kind the largest distance from the float64 run: the twin's may be at most 4 x torch float32's own.
    Both are printed; torch runs in a process of its own."""
    spec, state, obs, starts, theta = cases.sequence_inputs(index)
    np.savez(tmp_path / "in.npz", names=np.array(spec.keys()), obs=obs, starts=starts, theta=theta,
             activation=spec.activation, **state)
    subprocess.run([sys.executable, "-m", "tests.lstm_sde_io_cases", "--torch-sequence", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=300)
    theirs = np.load(tmp_path / "out.npz")
    params = spec.pack(state)
    current = np.zeros(spec.state_shape(obs.shape[1]), dtype=F32)
    kinds = ("mean", "sigma", "actions", "log_probs", "values")
    ours = {kind: [] for kind in kinds}
    for t in range(obs.shape[0]):
        got = lstm_sde.lstm_sde_numpy(spec, params, obs[t], starts[t], current, theta=theta)
        for kind in kinds:
            ours[kind].append(got[kind])
        current = got["state"]
    ours = {kind: np.stack(rows) for kind, rows in ours.items()}
    ours["state"] = current
    for kind in kinds + ("state",):
        exact = theirs[kind + "64"]
        assert theirs[kind + "32"].dtype == F32 and exact.dtype == np.float64 and exact.shape == ours[kind].shape
        twin = np.abs(ours[kind].astype(np.float64) - exact).max()
        torch = np.abs(theirs[kind + "32"].astype(np.float64) - exact).max()
        print(f"{cases.NETWORKS[index]}: {kind}: twin {twin:.3e}, torch {torch:.3e}, ratio {twin / torch:.2f}")
        assert twin <= FACTOR * torch, (kind, twin, torch)


AUTOGRAD_STEPS, AUTOGRAD_ENVS, AUTOGRAD_FIRST = 8, 4, 5


def autograd_inputs(index):
    """tests/test_lstm_learner_logic.py's rollout (8 steps of 4 environments as ONE minibatch of 32 rows rotated by 5;
    environment 1 runs all 8 rows from a stored non-zero state) with the twin's own sampled raw actions; the stored
    log-probabilities are its own plus normal noise of scale 0.15."""
    spec = cases.spec_of(cases.NETWORKS[index])
    state = cases.state_dict(spec, 60 + index)
    params = spec.pack(state)
    n_steps, num_envs = AUTOGRAD_STEPS, AUTOGRAD_ENVS
    total = n_steps * num_envs
    rng = np.random.default_rng(index)
    starts = np.zeros((n_steps + 1, num_envs), dtype=np.uint8)
    starts[0, 0], starts[3, 0], starts[5, 2], starts[0, 3], starts[6, 3] = 1, 1, 1, 1, 1
    states = (0.5 * rng.standard_normal((n_steps + 1,) + spec.state_shape(num_envs))).astype(F32)
    batch = {"observations": rng.standard_normal((total, spec.obs_width)).astype(F32),
             "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32)}
    mu, sigma, h = cases.own_head(spec, params, batch, starts, states, n_steps, num_envs)
    theta = sde.noise_numpy(params[spec.log_std_at:], rng.random(total * spec.latent))
    batch["actions"] = policy.canonical(mu + sde._rowdot(h, theta))
    batch["log_probs"] = (sde.log_prob_of(batch["actions"], mu, sigma) + 0.15 * rng.standard_normal(total)).astype(F32)
    return spec, state, params, batch, starts, states


@pytest.mark.parametrize("index", [cases.SMALL, 3], ids=["small", "odd-widths"])
def test_gradient_and_updates_are_no_further_from_float64_than_four_times_torch(index, tmp_path, hostcheck):
    """The twin's gradient before clipping (log_std's entries included), its parameters after the first update of a fresh
    optimizer and after 10 updates on one minibatch, each against the same from torch in float64 (nn.LSTM cells stepped
    per row with the definition's sequence rule and select, the Gaussian written out, stable-baselines3's loss, autograd,
    clip_grad_norm_, Adam(eps=1e-5)): the largest distance may be at most 4 x that of torch's own float32 run on the same
    inputs.  Both distances are printed, log_std's own too."""
    spec, state, params, batch, starts, states = autograd_inputs(index)
    n_steps, num_envs, first, count = AUTOGRAD_STEPS, AUTOGRAD_ENVS, AUTOGRAD_FIRST, AUTOGRAD_STEPS * AUTOGRAD_ENVS
    rows = lstm_learner.sequence_rows(starts, n_steps, num_envs, first, count)
    hyper = learner.Hyper(3e-4, 0.2, 0.01, 0.5, 0.5, 0.9, 0.999, 1e-5, 1)
    updates = 10
    np.savez(tmp_path / "in.npz", names=np.array(spec.keys()), activation=spec.activation, obs=batch["observations"],
             actions=batch["actions"], old_log_probs=batch["log_probs"], advantages=batch["advantages"],
             returns=batch["returns"], lstm_states=states, row=np.array([row[0] for row in rows], dtype=np.int64),
             env=np.array([row[1] for row in rows], dtype=np.int64), step=np.array([row[2] for row in rows], dtype=np.int64),
             is_start=np.array([row[3] for row in rows]), zero=np.array([row[4] for row in rows]),
             clip_range=hyper.clip_range, ent_coef=hyper.ent_coef, vf_coef=hyper.vf_coef,
             max_grad_norm=hyper.max_grad_norm, learning_rate=hyper.learning_rate, updates=updates, **state)
    subprocess.run([sys.executable, "-m", "tests.lstm_sde_io_cases", "--torch-lstm-sde-learner", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=600)
    theirs = np.load(tmp_path / "out.npz")
    grad, terms, invalid = lstm_learner.lstm_gradient_numpy(spec, params, batch, starts, states, n_steps, num_envs, first,
                                                            count, hyper)
    share = terms[4].mean()
    print(f"{cases.NETWORKS[index]}: share of ratios outside the clip range {share:.3f}")
    assert not invalid and 0.05 <= share <= 0.5 and abs(share - float(theirs["clip_fraction64"])) <= 2 / count
    ours = {"grad": grad}
    optimizer = learner.fresh_state(spec)
    for update in range(updates):
        params, optimizer, stats = lstm_learner.lstm_update_numpy(spec, params, optimizer, batch, starts, states, n_steps,
                                                                  num_envs, first, count, hyper)
        assert stats[7] == 0
        if update == 0:
            ours["first"] = params
    ours["last"] = params
    assert bits(host_update(hostcheck, spec, spec.pack(state), learner.fresh_state(spec), batch, starts, states, n_steps,
                            num_envs, first, count, hyper)[3]) == bits(grad)
    for kind in ("grad", "first", "last"):
        exact = theirs[kind + "64"]
        assert theirs[kind + "32"].dtype == F32 and exact.dtype == np.float64 and exact.shape == (spec.size,)
        for what, cells in (("all", slice(None)), ("log_std", slice(spec.log_std_at, None))):
            twin = np.abs(ours[kind].astype(np.float64) - exact)[cells].max()
            torch = np.abs(theirs[kind + "32"].astype(np.float64) - exact)[cells].max()
            print(f"{cases.NETWORKS[index]}: {kind} ({what}): twin {twin:.3e}, torch {torch:.3e}, ratio {twin / torch:.2f}")
            if what == "all":
                assert twin <= FACTOR * torch, (kind, twin, torch)
    assert np.abs(theirs["grad64"][spec.log_std_at:]).max() > 1e-4  # (log_std has a gradient, through sigma)


# ---- 3: hostile rows -----------------------------------------------------------------------------------------------------------
def small_update(log_std=None, nan_row=None):
    index, name = cases.SMALL, f"mixed/3/{cases.TILE + 1}"
    spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(index, name)
    params = params.copy()
    if log_std is not None:
        params[spec.log_std_at:] = F32(log_std)
    if nan_row is not None:
        batch = dict(batch, actions=batch["actions"].copy())
        batch["actions"][nan_row] = np.nan
    return spec, params, batch, starts, states, n_steps, num_envs, first, count


def test_infinite_sigma_ends_in_nonfinite_and_keeps_every_byte(hostcheck):
    """log_std so large that std = 1 / exp32(-90) is +inf: sigma is inf in every row, the update ends in
    RF_PPO_NONFINITE, and parameters and optimizer state keep their bytes -- in the twin and in the host build."""
    spec, params, batch, starts, states, n_steps, num_envs, first, count = small_update(log_std=90.0)
    assert np.isinf(sde.sigma_of(np.ones((1, spec.latent), dtype=F32), sde.std2_of(params[spec.log_std_at:]))).all()
    state = cases.twin_updates(cases.SMALL, f"mixed/3/{cases.TILE + 1}")[0][1]  # (an optimizer that has moved)
    args = (spec, params, state, batch, starts, states, n_steps, num_envs, first, count, cases.hyper_of(1))
    twin = lstm_learner.lstm_update_numpy(*args)
    assert twin[2][7] == learner.NONFINITE and bits(twin[0]) == bits(params) and bits(twin[1]) == bits(state)
    got = host_update(hostcheck, *args)
    same(got[:3], twin, "log_std of 90")


def test_zero_standard_deviation_gives_the_epsilon_sigma_and_finite_gradients(hostcheck):
    """log_std = -100: std2 == 0, sigma == sqrt32(1e-6f) in every row, and every gradient is finite (log_std's are 0)."""
    spec, params, batch, starts, states, n_steps, num_envs, first, count = small_update(log_std=-100.0)
    assert not sde.std2_of(params[spec.log_std_at:]).any()
    mu, sigma, h = cases.own_head(spec, params, batch, starts, states, n_steps, num_envs)
    assert bits(sigma) == bits(np.full(sigma.shape, np.sqrt(F32(1e-6)), dtype=F32))
    # stored log-probabilities of this very policy, so that the ratios are not all clipped away
    batch = dict(batch, actions=(mu + F32(1e-3) * np.arange(mu.size, dtype=F32) / F32(mu.size)).astype(F32))
    batch["log_probs"] = (sde.log_prob_of(batch["actions"], mu, sigma) - F32(0.05)).astype(F32)
    args = (spec, params, learner.fresh_state(spec), batch, starts, states, n_steps, num_envs, first, count,
            cases.hyper_of(0))
    grad = lstm_learner.lstm_gradient_numpy(spec, params, batch, starts, states, n_steps, num_envs, first, count,
                                            cases.hyper_of(0))[0]
    assert np.isfinite(grad).all() and not grad[spec.log_std_at:].any() and grad[:spec.log_std_at].any()
    twin = lstm_learner.lstm_update_numpy(*args)
    assert twin[2][7] == 0 and np.isfinite(twin[0]).all()
    same(host_update(hostcheck, *args), twin + (grad,), "log_std of -100")


def test_nan_action_ends_in_invalid_and_the_update_without_it_is_taken(hostcheck):
    spec, params, batch, starts, states, n_steps, num_envs, first, count = small_update()
    bad_row = (first + 2) % (n_steps * num_envs)
    poisoned = dict(batch, actions=batch["actions"].copy())
    poisoned["actions"][bad_row] = np.nan
    state = learner.fresh_state(spec)
    args = (starts, states, n_steps, num_envs, first, count, cases.hyper_of(0))
    twin = lstm_learner.lstm_update_numpy(spec, params, state, poisoned, *args)
    assert twin[2][7] == learner.INVALID and bits(twin[0]) == bits(params) and bits(twin[1]) == bits(state)
    same(host_update(hostcheck, spec, params, state, poisoned, *args)[:3], twin, "a NaN action")
    # a NaN action in a row outside the minibatch is not read: the same update is taken
    outside = dict(batch, actions=batch["actions"].copy())
    outside["actions"][(first + count) % (n_steps * num_envs)] = np.nan
    taken = lstm_learner.lstm_update_numpy(spec, params, state, outside, *args)
    want = cases.twin_updates(cases.SMALL, f"mixed/3/{cases.TILE + 1}")[0]
    same(taken, want[:3], "a NaN action outside the minibatch")
    same(host_update(hostcheck, spec, params, state, outside, *args), want, "a NaN action outside the minibatch (host)")


def test_nan_theta_is_stored_canonical(hostcheck):
    """A standard deviation of +inf times the draw whose normal32 is +0 (u = 0.5) is 0 * inf: stored as 0x7fc00000."""
    spec = cases.spec_of(cases.NETWORKS[0])
    params = spec.initial()
    params[spec.log_std_at:] = F32(90.0)
    theta = sde.noise_numpy(params[spec.log_std_at:], np.array([0.5]))
    assert theta.view(np.uint32).tolist() == [[0x7FC00000]]
    # the host build on a generator whose draw is not 0.5 gives +-inf; the product itself is checked by value
    assert np.isinf(host_noise(hostcheck, spec, params, 3, cases.generator_at(0)[0])).all()
    assert sde.noise_numpy(np.array([-100.0], dtype=F32), np.array([0.25])).view(np.uint32).tolist() == [[0x80000000]]


def test_nan_in_a_dead_state_does_not_survive_an_episode_start(hostcheck):
    index, n = cases.SMALL, cases.TILE + 1
    spec, params, obs, final_obs, starts, state = cases.chain_inputs(index, n)
    assert np.isnan(state[:, :, 0]).all() and starts[0, 0] != 0  # (environment 0: NaN throughout, and it starts)
    clean = state.copy()
    clean[:, :, 0] = 0.0
    theta = cases.wanted_theta(index, n, 0)
    finite_obs = np.where(np.isfinite(obs[0]), obs[0], F32(0.25))
    got = lstm_sde.lstm_sde_numpy(spec, params, finite_obs, starts[0], state, None, theta)
    want = lstm_sde.lstm_sde_numpy(spec, params, finite_obs, starts[0], clean, None, theta)
    for name in cases.PI_OUTPUTS + ("values",):
        assert bits(got[name][0]) == bits(want[name][0]) and np.isfinite(got[name][0]), name
    assert bits(got["state"][:, :, 0]) == bits(want["state"][:, :, 0]) and np.isfinite(got["state"][:, :, 0]).all()
    host, host_state = host_forward(hostcheck, spec, params, finite_obs, starts[0], None, state, theta,
                                    cases.PI_OUTPUTS + ("values",))
    assert all(bits(host[name]) == bits(got[name]) for name in host) and bits(host_state) == bits(got["state"])
    # and in the update: a NaN stored state behind a start byte never enters
    spec, params, batch, starts, states, n_steps, num_envs, first, count = small_update()
    poisoned = states.copy()
    for t, e in zip(*np.nonzero(starts[:n_steps])):
        poisoned[t, :, :, e] = np.nan
    args = (n_steps, num_envs, first, count, cases.hyper_of(0))
    same(lstm_learner.lstm_update_numpy(spec, params, learner.fresh_state(spec), batch, starts, poisoned, *args),
         cases.twin_updates(cases.SMALL, f"mixed/3/{cases.TILE + 1}")[0][:3], "NaN states behind start bytes")


def test_raw_actions_outside_the_box_are_kept_raw_and_clamped_for_the_step(no_gpu):  # noqa: F811
    env = harness.VectorContinuousJumps(num_envs=3, **rollout_cases.ENV_KW)
    try:
        spec = cases.e2e_spec("plain", env)
        spec = cases.spec_of((spec.obs_width, 16, (8,), (8,), "tanh"), log_std_init=1.5)  # (a wide Gaussian)
        twin = harness.LstmSdePolicy(spec, 5, num_envs=3)
        twin.load_state_dict(dict(cases.state_dict(spec, 3), log_std=np.full((spec.latent, 1), 1.5, dtype=F32)))
        rollout = harness.Rollout(env, 6)
        rollout.start(env.reset()[0])
        stepped = []
        step = env.step
        env.step = lambda actions: (stepped.append(np.array(actions)), step(actions))[1]
        rollout.collect(twin, sde_sample_freq=2)
        raw = rollout.actions
        assert raw.dtype == F32 and (np.abs(raw) > 1).any(), "no raw action left the box"
        assert bits(np.stack(stepped).reshape(raw.shape)) == bits(sde.env_actions_of(raw))
        assert rollout.lstm_states.shape == (7, 2, 2, 3, 16) and bits(rollout.episode_starts[1:]) == bits(rollout.truncated)
        assert (rollout.episode_starts[0] == 1).all() and bits(twin.lstm_state()) == bits(rollout.lstm_states[6])
    finally:
        env.close()


# ---- 4: the surface ------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_surface(no_gpu):  # noqa: F811
    jumps = harness.VectorContinuousJumps(num_envs=2, **rollout_cases.ENV_KW)
    steps = harness.VectorDiscreteSteps(num_envs=2, **rollout_cases.ENV_KW)
    try:
        spec = cases.e2e_spec("plain", jumps)
        twin = harness.LstmSdePolicy(spec, 0, num_envs=2)
        categorical = harness.LstmPolicy(lstm_cases.e2e_spec("plain"), 0, num_envs=2)
        # what still stands: the Categorical recurrent policy on a Box space, and its learner over such a rollout
        with pytest.raises(ValueError, match="out of scope") as caught:
            lstm._refuse_box(jumps.single_action_space)
        assert "sde" in str(caught.value)
        buffer = harness.Rollout(jumps, 2)
        buffer.start(jumps.reset()[0])
        with pytest.raises(ValueError, match="out of scope"):
            buffer.collect(categorical)
        with pytest.raises(ValueError, match="out of scope"):
            harness.LstmLearner(categorical).train(harness.Rollout(jumps, 2), 1, 4)
        # the new policy on a Discrete task, and the sde_sample_freq rules
        with pytest.raises(ValueError, match="sde_sample_freq"):
            buffer.collect(twin, sde_sample_freq=0)
        with pytest.raises(ValueError, match="sde_sample_freq"):
            buffer.collect(twin, sde_sample_freq=2.5)
        other = harness.Rollout(steps, 2)
        other.start(steps.reset()[0])
        with pytest.raises(ValueError, match="Gaussian head"):
            other.collect(twin)
        with pytest.raises(ValueError, match="sde_sample_freq"):
            other.collect(categorical, sde_sample_freq=4)
        with pytest.raises(ValueError, match="Gaussian head"):
            harness.LstmLearner(twin).train(harness.Rollout(steps, 2), 1, 4)
        with pytest.raises(ValueError, match="reset_noise"):
            twin.act(np.zeros((2, spec.obs_width), dtype=F32), np.zeros(2, dtype=np.uint8))
        whole = {"observations": np.zeros((4, spec.obs_width), dtype=F32), "actions": np.zeros(4, dtype=np.int64),
                 "log_probs": np.zeros(4, dtype=F32), "advantages": np.zeros(4, dtype=F32), "returns": np.zeros(4, dtype=F32),
                 "episode_starts": np.zeros((3, 2), dtype=np.uint8),
                 "lstm_states": np.zeros((3, 2, 2, 2, spec.lstm_hidden), dtype=F32), "n_steps": 2, "num_envs": 2}
        with pytest.raises(ValueError, match="int64 action slab"):  # (no silent cast of indices to raw actions)
            harness.LstmLearner(twin).update(whole, 0, 4)
        with pytest.raises(TypeError, match="device-resident"):
            harness.DeviceLstmSdePolicy(jumps, spec, 0)
        with pytest.raises(TypeError, match="DeviceLstmPolicy"):
            harness.DeviceLstmLearner(twin)
        with pytest.raises(TypeError, match="LstmSdePolicySpec"):
            harness.LstmSdePolicy(lstm_cases.e2e_spec("plain"), 0)
        with pytest.raises(TypeError, match="LstmPolicySpec"):
            harness.LstmPolicy(spec, 0)
        with pytest.raises(TypeError, match="Policy or an SdePolicy"):
            harness.Learner(twin)
    finally:
        jumps.close()
        steps.close()
    with pytest.raises(TypeError):
        lstm_sde.LstmSdePolicySpec(4, 2, 16)  # (no n_actions argument: the third positional is pi)
    assert lstm_sde.LstmSdePolicySpec(4).desc()[1] == 1 and lstm_sde.LstmSdePolicySpec(4).desc()[-1] == 256
    for action_space in (harness.spaces.Box(-1.0, 1.0, (2,), np.float32), harness.spaces.Discrete(3)):
        with pytest.raises(ValueError, match="Gaussian head"):
            lstm_sde._refuse_discrete(action_space)
    for wrong in (dict(lstm_hidden=0), dict(lstm_hidden=257), dict(pi=(64, 64, 64)), dict(activation="gelu")):
        with pytest.raises(ValueError):
            lstm_sde.LstmSdePolicySpec(4, **wrong)


def test_generator_moves_by_n_times_L_per_reset_and_by_nothing_per_act():
    spec = cases.spec_of(cases.NETWORKS[cases.SMALL])
    twin = harness.LstmSdePolicy(spec, 7, num_envs=3)
    twin.load_state_dict(cases.state_dict(spec, 1))
    reference = np.random.PCG64DXSM(7)
    twin.reset_noise()
    reference.advance(3 * spec.latent)
    assert twin.rng_state() == reference.state and twin.noise().shape == (3, spec.latent)
    obs = np.random.default_rng(0).standard_normal((3, spec.obs_width)).astype(F32)
    twin.act(obs, np.ones(3, dtype=np.uint8))
    twin.values(obs, np.zeros(3, dtype=np.uint8))
    assert twin.rng_state() == reference.state
    kept = twin.rng_state()
    twin.reset_noise()
    twin.set_rng_state(kept)
    theta = twin.noise()
    twin.reset_noise()
    assert bits(twin.noise()) == bits(theta)  # (rng_state / set_rng_state round-trip)
    twin.reset_state()
    first = twin.act(obs, np.zeros(3, dtype=np.uint8))
    moved =twin.act(obs, np.zeros(3, dtype=np.uint8))
    twin.reset_state()
    again = twin.act(obs, np.zeros(3, dtype=np.uint8))
    assert all(bits(x) == bits(y) for x, y in zip(first[:3] + first[4:], again[:3] + again[4:]))
    assert bits(moved[0]) != bits(first[0])  # (the state matters)


def test_collect_and_train_by_the_twins_runs_and_resumes(no_gpu):  # noqa: F811
    """Two iterations of collect + train by the numpy twins at the GPU tests' end-to-end shape; the learner's state_dict
    resumes bit for bit over P + L."""
    want, _ = cases.twin_train_runs("view", 9)
    assert (want[1]["stats"][:, 7] == 0).all() and bits(want[0]["params"]) != bits(want[1]["params"])
    assert want[1]["episode_starts"][1:cases.T].any() and want[0]["lstm_states"].shape[0] == cases.T + 1
    env = cases.make_env("view", 3, False)
    try:
        spec = cases.e2e_spec("view", env)
        twin = harness.LstmSdePolicy(spec, cases.SEED, num_envs=3)
        twin.load_state_dict(cases.e2e_state(spec))
        trainer = harness.LstmLearner(twin, **cases.LEARNER_KW)
        rollout = harness.Rollout(env, cases.T, cases.GAMMA, cases.GAE_LAMBDA)
        rollout.start(env.reset()[0])
        rollout.collect(twin, sde_sample_freq=cases.E2E_FREQ)
        trainer.train(rollout, 1, 8, splits=[3])
        kept, kept_params = trainer.state_dict(), twin.state_dict()
        assert kept["m"].size == spec.size and kept["m"][spec.log_std_at:].any()
        straight = trainer.train(rollout, 1, 8, splits=[5])
        after = twin.params.copy(), trainer.state.copy()
        twin.load_state_dict(kept_params)
        fresh = harness.LstmLearner(twin, **cases.LEARNER_KW)
        fresh.load_state_dict(kept)
        assert bits(fresh.train(rollout, 1, 8, splits=[5])) == bits(straight)
        assert bits(twin.params) == bits(after[0]) and bits(fresh.state) == bits(after[1])
    finally:
        env.close()


def test_import_of_harness_stays_free_of_torch():
    code = "import sys; from reinfocus_amd.environments import harness; harness.LstmSdePolicy; harness.DeviceLstmSdePolicy; " \
           "assert 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, timeout=120)


def test_binding_matches_the_header():
    """Every rf_lstm_sde_ entry point of the header is bound with as many arguments as it declares, and is in SYMBOLS."""
    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    seen = []
    for kind, name, arguments in re.findall(r"\b(int|unsigned long long)\s+(rf_lstm_sde_\w+)\s*\((.*?)\)\s*;", text, flags=re.S):
        bound = re.search(rf"lib\.{name}\.argtypes = \[(.*?)\]", source).group(1).split(",")
        assert len(bound) == len(arguments.split(",")), name
        assert (re.search(rf"lib\.{name}\.restype = ctypes\.c_ulonglong", source) is not None) == (kind != "int"), name
        assert name in _native.SYMBOLS
        assert re.search(rf"self\._lib\.{name}\(", source), name
        seen.append(name)
    assert seen == ["rf_lstm_sde_params_size", "rf_lstm_sde_noise_reset", "rf_lstm_sde_forward", "rf_lstm_sde_state_size",
                    "rf_lstm_sde_workspace_size", "rf_lstm_sde_update"]
    assert "Out of scope: the Gaussian" not in text and "lstm sde policy" in text and "lstm sde update" in text


def test_stand_alone_host_program_runs():
    """tests/lstmsdecheck/lstmsdecheck: the same source with its own main -- one noise reset, forwards and one update on a
    tiny network outside any interpreter (the form a host sanitizer build of this arithmetic takes) -- ends with status 0
    and prints finite figures."""
    helpers.built("tests/lstmsdecheck", "liblstmsdecheck.so")  # (the Makefile rule that builds both)
    done = subprocess.run([os.path.join(ROOT, "tests", "lstmsdecheck", "lstmsdecheck")], capture_output=True, text=True,
                          timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    lines = done.stdout.strip().splitlines()
    assert len(lines) == 3 and lines[2].startswith("stats:") and "nan" not in done.stdout and "inf" not in done.stdout
