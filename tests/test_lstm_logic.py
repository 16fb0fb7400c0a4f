"""CPU tests of the recurrent PPO actor-critic (environments/lstm.py): lstm_numpy -- the oracle the kernel is held to in
tests/test_gpu_lstm.py -- against the very text the kernel inlines, compiled for the host (tests/lstmcheck:
csrc/rf_policy_math.h, csrc/rf_lstm.h's cell and layout and a plain loop over them), as bytes; the accuracy of sigmoid32
against float64 and of the whole recurrent network next to torch's own float32 nn.LSTM; the packing; Rollout.collect
against the explicit loop; the binding.  The GPU's render and focus measure are replaced by a function of the state
(tests/test_composed_env_logic.py::no_gpu)."""

import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, lstm, policy
from tests import helpers
from tests import lstm_io_cases as cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits
# sigmoid32's largest absolute error against float64 on sigmoid_grid(), as measured (profiles/lstm.md)
SIGMOID_MEASURED = 8.784e-8


@pytest.fixture(scope="module")
def lstmcheck():
    lib = ctypes.CDLL(helpers.built("tests/lstmcheck", "liblstmcheck.so"))
    vp = ctypes.c_void_p
    lib.lc_sigmoid.argtypes = [vp, vp, ctypes.c_longlong]
    lib.lc_cell.argtypes = [vp, vp, vp, vp, ctypes.c_longlong]
    lib.lc_params_size.restype = ctypes.c_ulonglong
    lib.lc_params_size.argtypes = [vp]
    lib.lc_state_size.restype = ctypes.c_ulonglong
    lib.lc_state_size.argtypes = [vp, ctypes.c_int]
    lib.lc_forward.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp]
    return lib


def sigmoid_grid():
    """A dense grid over [-100, 100], +-0, +-inf, NaN, subnormals, and every 64th float32 of |x| in [86.5, 87.5], where
    exp32 cuts off."""
    lo, hi = int(F32(86.5).view(np.uint32)), int(F32(87.5).view(np.uint32))
    cut = np.arange(lo, hi + 1, 64, dtype=np.uint64).astype(np.uint32).view(F32)
    special = F32([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 87.0, -87.0, 3e38, -3e38])
    return np.concatenate([special, np.linspace(-100.0, 100.0, 400001).astype(F32), cut, -cut,
                           (np.random.default_rng(0).standard_normal(20000) * 1e-3).astype(F32)])


# ---- 1: the host build of the header equals the twin ---------------------------------------------------------------------
def test_sigmoid32_of_the_header_equals_the_twin(lstmcheck):
    x = sigmoid_grid()
    got = np.empty_like(x)
    lstmcheck.lc_sigmoid(x.ctypes.data, got.ctypes.data, x.size)
    want = lstm.sigmoid32(x)
    assert bits(policy.canonical(got)) == bits(want)
    assert bits(want[:5]) == bits(np.array([0.5, 0.5, 1.0, 0.0, policy._NAN], dtype=F32))
    live = want[~np.isnan(x)]
    assert live.min() == 0.0 and live.max() == 1.0
    assert bits(lstm.sigmoid32(F32([-87.0001, -1000.0]))) == bits(np.zeros(2, dtype=F32))  # +0 past the cut-off


def test_sigmoid32_against_float64():
    x = sigmoid_grid()
    x = x[np.isfinite(x)]
    exact = np.array([1.0 / (1.0 + math.exp(-v)) if v >= 0 else math.exp(v) / (1.0 + math.exp(v)) for v in x.astype(np.float64)])
    error = np.abs(lstm.sigmoid32(x).astype(np.float64) - exact).max()
    print("sigmoid32: largest absolute error %.3e" % error)
    assert error <= 2.0 * SIGMOID_MEASURED


def test_cell_of_the_header_equals_the_twin(lstmcheck):
    grid = sigmoid_grid()
    rng = np.random.default_rng(3)
    count = 200000
    a = rng.choice(grid, (count, 4)).astype(F32)
    a[::2] = (rng.standard_normal((count // 2, 4)) * 3.0).astype(F32)
    c = rng.choice(np.concatenate([grid, F32(rng.standard_normal(1000))]), count).astype(F32)
    h1, c1 = np.empty(count, dtype=F32), np.empty(count, dtype=F32)
    lstmcheck.lc_cell(a.ctypes.data, c.ctypes.data, h1.ctypes.data, c1.ctypes.data, count)
    want_h, want_c = lstm.cell(a, c)
    assert bits(policy.canonical(h1)) == bits(policy.canonical(want_h))
    assert bits(policy.canonical(c1)) == bits(policy.canonical(want_c))
    assert np.isnan(want_c).any() and np.isfinite(want_h).sum() > count // 2


def host_forward(lib, spec, params, obs, starts, final_obs, state_in, state_out, gen, deterministic):
    n = obs.shape[0]
    out = dict(actions=np.zeros(n, dtype=np.int64), log_probs=np.zeros(n, dtype=F32), values=np.zeros(n, dtype=F32),
               final_values=np.zeros(n, dtype=F32), logits=np.zeros((n, spec.n_actions), dtype=F32))
    desc = _native.LstmPolicyDesc(*spec.desc())
    assert lib.lc_params_size(ctypes.byref(desc)) == spec.size == params.size
    assert lib.lc_state_size(ctypes.byref(desc), n) == state_in.size
    words = None if gen is None else (ctypes.c_ulonglong * 4)(*gen)
    obs, starts, final_obs = np.ascontiguousarray(obs), np.ascontiguousarray(starts), np.ascontiguousarray(final_obs)
    assert lib.lc_forward(ctypes.byref(desc), params.ctypes.data, n, obs.ctypes.data, starts.ctypes.data,
                          final_obs.ctypes.data, state_in.ctypes.data, state_out.ctypes.data, words,
                          policy.DETERMINISTIC if deterministic else 0, *(out[k].ctypes.data for k in cases.OUTPUTS)) == 0
    return out


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)))
def test_forward_of_the_header_equals_the_twin(index, n, lstmcheck):
    """The chains of tests/test_gpu_lstm.py -- hostile observations and states, start bytes 0, 1, 2 and 255, a NaN state
    under a set start byte, NaN-led final_obs rows --, sampled at draw offsets 0 and 2^32 + 5 and deterministic, the state
    in place and from one buffer into another: every output and the state of every step as bytes."""
    spec, params, obs, final_obs, starts, state = cases.chain_inputs(index, n)
    for mode, offset in cases.MODES:
        want = cases.wanted_chain(index, n, mode, offset)
        for in_place in (True, False):
            buffers = [state.copy(), np.full_like(state, 7.0)]
            bit_generator = cases.generator_at(offset)[0]
            for s in range(cases.STEPS):
                source = buffers[0] if in_place else buffers[s % 2]
                target = buffers[0] if in_place else buffers[(s + 1) % 2]
                gen = policy.generator_words(bit_generator) if mode == "sampled" else None
                got = host_forward(lstmcheck, spec, params, obs[s], starts[s], final_obs[s], source, target, gen,
                                   mode == "deterministic")
                bit_generator.advance(n if mode == "sampled" else 0)
                for name in cases.OUTPUTS:
                    assert bits(got[name]) == bits(want[s][name]), (mode, offset, in_place, s, name)
                assert bits(target) == bits(want[s]["state"]), (mode, offset, in_place, s)


def test_hostile_chain_holds_what_it_promises():
    index, n = cases.DEFAULT, 29
    spec, params, obs, final_obs, starts, state = cases.chain_inputs(index, n)
    for special in (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001):  # +-0, +-inf, the least subnormal
        assert (obs.view(np.uint32) == special).any() and (state.view(np.uint32) == special).any(), hex(special)
    assert np.isnan(obs).any() and np.isnan(state[:, :, 0]).all() and starts[0, 0] != 0
    assert set(np.unique(starts)) == {0, 1, 2, 255}
    want = cases.wanted_chain(index, n, "sampled", 0)
    # environment 0: a NaN state under a set start byte comes out exactly as from a zero state
    zero = state.copy()
    zero[:, :, 0] = 0.0
    u = cases.generator_at(0)[1].random(n)
    again = lstm.lstm_numpy(spec, params, obs[0], starts[0], zero, final_obs[0], u)
    for name in ("actions", "log_probs", "values", "logits"):
        assert bits(again[name][0]) == bits(want[0][name][0]), name
    assert bits(again["state"][:, :, 0]) == bits(want[0]["state"][:, :, 0]) and np.isfinite(want[0]["state"][:, :, 0]).all()
    # ... while V(final_obs) starts from the state as it is: NaN for environment 0
    assert np.isnan(want[0]["final_values"][0])
    # environment 4: its NaN is not cleared (no start in step 0) and lives on in the pi state
    assert starts[0, 4] == 0 and np.isnan(want[0]["state"][0, :, 4]).all()
    assert (want[0]["state"].view(np.uint32)[np.isnan(want[0]["state"])] == policy.NAN_BITS).all()
    last = want[-1]
    live = np.isfinite(last["state"]).all(axis=(0, 1, 3))
    assert live.sum() >= 10 and not live.all()
    assert np.isfinite(last["values"][live]).all() and np.isfinite(last["log_probs"][live]).all()
    led = np.isnan(final_obs[-1][:, 0])
    assert (last["final_values"][led].view(np.uint32) == policy.NAN_BITS).all() and 0 < led.sum() < n
    assert np.isfinite(last["final_values"]).sum() >= 5
    # the start byte is a flag: 1, 2 and 255 act alike
    base = lstm.lstm_numpy(spec, params, obs[1], starts[1], want[0]["state"], final_obs[1], None, True)
    assert len(set(starts[1][starts[1] != 0])) > 1
    for byte in (1, 2, 255):
        other = starts[1].copy()
        other[other != 0] = byte
        same = lstm.lstm_numpy(spec, params, obs[1], other, want[0]["state"], final_obs[1], None, True)
        assert bits(same["state"]) == bits(base["state"]) and bits(same["values"]) == bits(base["values"])


# ---- 2: accuracy next to torch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [cases.TUNED, cases.DEFAULT], ids=["tuned", "default"])
def test_recurrent_network_is_no_further_from_float64_than_four_times_torch(index, tmp_path):
    """A 16-step sequence of normal rows with three episode starts inside it, from one state_dict: the twin, torch.nn.LSTM
    + nn.Sequential in float32, and the same in float64.  Per kind (logits, values, the final state) the largest distance
    from the float64 run: the twin's may be at most 4 x torch float32's own (the margin of tests/test_learner_logic.py).
    Both are measured here (profiles/lstm.md records a run); torch runs in a process of its own."""
    spec, state, obs, starts = cases.sequence_inputs(index)
    np.savez(tmp_path / "in.npz", obs=obs, starts=starts, activation=spec.activation, **state)
    subprocess.run([sys.executable, "-m", "tests.lstm_io_cases", "--torch-sequence", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=300)
    theirs = np.load(tmp_path / "out.npz")
    params = spec.pack(state)
    rows = obs.shape[1]
    current = np.zeros(spec.state_shape(rows), dtype=F32)
    logits, values = [], []
    for t in range(obs.shape[0]):
        got = lstm.lstm_numpy(spec, params, obs[t], starts[t], current, deterministic=True)
        logits.append(got["logits"])
        values.append(got["values"])
        current = got["state"]
    ours = {"logits": np.stack(logits), "values": np.stack(values), "state": current}
    for kind in ("logits", "values", "state"):
        exact = theirs[kind + "64"]
        assert theirs[kind + "32"].dtype == F32 and exact.dtype == np.float64 and exact.shape == ours[kind].shape
        twin = np.abs(ours[kind].astype(np.float64) - exact).max()
        torch = np.abs(theirs[kind + "32"].astype(np.float64) - exact).max()
        print(f"{cases.NETWORKS[index]}: {kind}: twin {twin:.3e}, torch {torch:.3e}, ratio {twin / torch:.2f}")
        assert twin <= 4.0 * torch, (kind, twin, torch)


# ---- 3: the packing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)))
def test_packing_round_trip_names_and_shapes(index):
    spec = cases.spec_of(cases.NETWORKS[index])
    width, hidden = spec.obs_width, spec.lstm_hidden
    state = cases.state_dict(spec, index)
    for lstm_name in ("lstm_actor", "lstm_critic"):
        assert state[lstm_name + ".weight_ih_l0"].shape == (4 * hidden, width)
        assert state[lstm_name + ".weight_hh_l0"].shape == (4 * hidden, hidden)
        assert state[lstm_name + ".bias_ih_l0"].shape == state[lstm_name + ".bias_hh_l0"].shape == (4 * hidden,)
    assert state["mlp_extractor.policy_net.0.weight"].shape == (spec.pi[0], hidden)
    assert state["mlp_extractor.value_net.0.weight"].shape == (spec.vf[0], hidden)
    assert state["action_net.weight"].shape == (spec.n_actions, spec.pi[-1]) and state["value_net.weight"].shape == (1, spec.vf[-1])
    params = spec.pack(state)
    assert params.dtype == F32 and params.shape == (spec.size,) == (sum(v.size for v in state.values()),)
    back = spec.unpack(params)
    assert list(back) == spec.keys() and sorted(back) == sorted(state)
    for name in state:
        assert bits(back[name]) == bits(state[name]), name
    with pytest.raises(KeyError, match="missing"):
        spec.pack({k: v for k, v in state.items() if k != "lstm_critic.bias_hh_l0"})
    with pytest.raises(KeyError, match="unknown"):
        spec.pack(dict(state, **{"lstm_actor.weight_ih_l1": np.zeros(1)}))
    with pytest.raises(ValueError, match="shape"):
        spec.pack(dict(state, **{"lstm_actor.weight_ih_l0": state["lstm_actor.weight_ih_l0"].T}))


def test_packed_layout_of_an_odd_width_network_element_by_element():
    """(7, 65, (65,), (3, 200), 64): pi = W_ih^T [7][260], W_hh^T [65][260], b_ih, b_hh, W0^T [65][65], b0, Wa^T [65][64],
    ba; then vf alike.  Element [k][q * H + j] of a packed LSTM matrix is torch's weight[q * H + j][k]."""
    spec = cases.spec_of(cases.NETWORKS[3])
    state = cases.state_dict(spec, 3)
    params = spec.pack(state)
    at = 0
    order = ["lstm_actor." + p for p in lstm.LSTM_PARTS] + ["mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
                                                          "action_net.weight", "action_net.bias"]
    order += ["lstm_critic." + p for p in lstm.LSTM_PARTS] + ["mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
                                                           "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
                                                           "value_net.weight", "value_net.bias"]
    assert order == spec.keys()
    for name in order:
        value = state[name]
        if value.ndim == 2:
            outs, ins = value.shape
            for k in range(ins):
                for j in range(outs):
                    assert params[at + k * outs + j] == value[j, k], (name, k, j)
        else:
            assert bits(params[at:at + value.size]) == bits(value), name
        at += value.size
    assert at == spec.size == 4 * 65 * (7 + 65 + 2) * 2 + (65 * 65 + 65 + 65 * 64 + 64) + (65 * 3 + 3 + 3 * 200 + 200 + 200 + 1)
    desc = _native.LstmPolicyDesc(*spec.desc())
    assert desc.lstm_hidden == 65 and desc.policy.obs_width == 7 and list(desc.policy.vf_width) == [3, 200]


def test_specs_outside_the_limits_are_refused():
    for kw in (dict(obs_width=0), dict(obs_width=257), dict(n_actions=1), dict(n_actions=65), dict(pi=()), dict(pi=(8, 8, 8)),
               dict(vf=(257,)), dict(vf=(0,)), dict(activation="gelu"), dict(lstm_hidden=0), dict(lstm_hidden=257)):
        with pytest.raises(ValueError):
            lstm.LstmPolicySpec(**dict(dict(obs_width=4, n_actions=13), **kw))
    spec = lstm.LstmPolicySpec(4, 13)
    assert (spec.lstm_hidden, spec.pi, spec.vf, spec.activation) == (256, (64, 64), (64, 64), "tanh")


# ---- 4: the twin's surface and the rollout ---------------------------------------------------------------------------------------
def test_twin_state_and_generator_accounting():
    spec = cases.spec_of(cases.NETWORKS[cases.TUNED])
    twin = harness.LstmPolicy(spec, 7, num_envs=9)
    twin.load_state_dict(cases.state_dict(spec, 1))
    obs = cases.hostile_rows(4, 9, 0, False)
    obs[2, -1] = 0.25  # (no NaN row: the states stay finite)
    obs[np.isinf(obs)] = 1.0
    starts = np.zeros(9, dtype=np.uint8)
    start = twin.rng_state()
    assert not twin.lstm_state().any()
    twin.values(obs, starts)
    twin.values(obs, starts, cases.hostile_rows(4, 9, 1, True))
    assert twin.rng_state() == start and not twin.lstm_state().any()  # no draw, no advance
    twin.act(obs, starts, deterministic=True)
    first = twin.lstm_state()
    assert twin.rng_state() == start and first.any() and np.isfinite(first).all()
    twin.act(obs, starts)
    assert twin.rng_state() != start and bits(twin.lstm_state()) != bits(first)
    # states=(in, out) leaves the own state alone
    own = twin.lstm_state()
    apart = (first.copy(), np.zeros_like(first))
    twin.act(obs, starts, deterministic=True, states=apart)
    assert bits(twin.lstm_state()) == bits(own) and bits(apart[0]) == bits(first) and apart[1].any()
    # a start in every environment equals a reset state
    twin.set_lstm_state(first)
    a = twin.act(obs, np.full(9, 255, dtype=np.uint8), deterministic=True)
    twin.reset_state()
    assert not twin.lstm_state().any()
    b = twin.act(obs, starts, deterministic=True)
    for x, y in zip(a[:3], b[:3]):
        assert bits(x) == bits(y)
    with pytest.raises(ValueError, match="shape"):
        twin.set_lstm_state(np.zeros((2, 2, 9, 15)))
    with pytest.raises(TypeError, match="LstmPolicySpec"):
        harness.LstmPolicy(policy.MlpPolicySpec(4, 13))


@pytest.mark.parametrize("kind", sorted(cases.E2E_KINDS))
def test_twin_collect_equals_the_explicit_loop(kind, no_gpu):  # noqa: F811
    """VectorDiscreteSteps with records and the learner view (the tuned network), and with neither (the default one):
    every slab, advantages, returns, flat() and the policy's state of two consecutive rollouts as bytes; the two
    recurrent slabs hold what they promise; environments end inside the rollouts."""
    n = 5
    (got, _), (want, _) = cases.twin_runs(kind, n), cases.twin_runs(kind, n, explicit=True)
    cases.same_runs(cases.without_recurrent(got), want)
    assert np.concatenate([run["truncated"] for run in got]).any()
    for r, run in enumerate(got):
        assert run["episode_starts"].dtype == np.uint8 and run["episode_starts"].shape == (cases.T + 1, n)
        assert run["lstm_states"].dtype == F32
        assert run["lstm_states"].shape == (cases.T + 1, 2, 2, n, cases.e2e_spec(kind).lstm_hidden)
        assert bits(run["episode_starts"][1:]) == bits(run["truncated"])
        assert (run["episode_starts"][0] == 1).all() if r == 0 else \
            bits(run["episode_starts"][0]) == bits(got[0]["truncated"][cases.T - 1])
        assert bits(run["lstm_states"][cases.T]) == bits(run["policy_state"])
        assert bits(run["lstm_states"][0]) == bits(got[0]["policy_state"] if r else np.zeros_like(run["policy_state"]))
        assert np.isfinite(run["lstm_states"]).all() and run["lstm_states"][1:].any()
    if cases.E2E_KINDS[kind]["records"]:
        for run in got:
            assert bits(np.isnan(run["final_values"])) == bits(run["truncated"] == 0)
    assert not np.isnan(got[1]["advantages"]).any()


def test_feedforward_rollout_never_allocates_the_recurrent_slabs(no_gpu):  # noqa: F811
    from tests import policy_io_cases

    env = policy_io_cases.make_env("plain", 3, False)
    spec = policy_io_cases.e2e_spec("plain")
    buffer = harness.Rollout(env, 2)
    assert buffer.episode_starts is None and buffer.lstm_states is None
    buffer.start(env.reset()[0])
    buffer.collect(harness.Policy(spec, 0))
    assert buffer.episode_starts is None and buffer.lstm_states is None
    env.close()


def test_collect_and_policy_refusals(no_gpu):  # noqa: F811
    from tests import rollout_io_cases

    jumps = harness.VectorContinuousJumps(num_envs=2, **rollout_io_cases.ENV_KW)
    buffer = harness.Rollout(jumps, 2)
    buffer.start(jumps.reset()[0])
    with pytest.raises(ValueError, match="out of scope"):
        buffer.collect(harness.LstmPolicy(cases.e2e_spec("view"), 0))
    with pytest.raises(TypeError, match="device-resident"):
        harness.DeviceLstmPolicy(jumps, cases.e2e_spec("view"), 0)
    jumps.close()


def test_import_stays_free_of_torch():
    code = ("import sys; from reinfocus_amd.environments import harness; harness.LstmPolicy; harness.DeviceLstmPolicy; "
            "harness.LstmPolicySpec; harness.lstm_numpy; assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


# ---- 5: the binding and the constants -------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    struct = re.search(r"typedef struct rf_lstm_policy_desc \{(.*?)\} rf_lstm_policy_desc;", text, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    assert [part.split() for part in struct.split(";") if part.strip()] == [["rf_policy_desc", "policy"], ["int", "lstm_hidden"]]
    assert [name for name, _ in _native.LstmPolicyDesc._fields_] == ["policy", "lstm_hidden"]
    assert ctypes.sizeof(_native.LstmPolicyDesc) == ctypes.sizeof(_native.PolicyDesc) + 4
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"\bint\s+rf_lstm_forward\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    wanted = [ctypes.c_void_p if ("*" in p or "[" in p) else ctypes.c_int for p in declaration.split(",")]
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    names = re.search(r"lib\.rf_lstm_forward\.argtypes = \[(.*?)\]", source).group(1).split(",")
    assert [{"vp": ctypes.c_void_p, "i32": ctypes.c_int}[name.strip()] for name in names] == wanted and len(wanted) == 17
    for name in ("rf_lstm_params_size", "rf_lstm_state_size", "rf_lstm_forward"):
        assert name in _native.SYMBOLS


def test_kernel_reuses_the_policy_kernels_pieces_unchanged():
    text = open(os.path.join(ROOT, "reinfocus_amd", "csrc", "rf_lstm.h")).read()
    for piece in ("policy_hidden_tile(", "policy_dot(", "policy_head(", "kPolicyTile"):
        assert piece in text, piece
    assert cases.SIZES == (1, cases.TILE, cases.TILE + 1, 3 * cases.TILE + 5)
