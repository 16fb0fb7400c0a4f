"""CPU tests of the PPO actor-critic (environments/policy.py): policy_numpy -- the oracle the kernel is held to in
tests/test_gpu_policy.py -- against the very text the kernel inlines, compiled for the host (tests/policycheck:
csrc/rf_policy_math.h and a plain loop over its functions), as bytes; the accuracy of the definition against float64
numpy and next to torch's own float32 forward; the sampling frequencies; the generator accounting; Rollout.collect
against the explicit loop; the binding.  The GPU's render and focus measure are replaced by a function of the state
(tests/test_composed_env_logic.py::no_gpu)."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, policy
from tests import helpers
from tests import policy_io_cases as cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits


@pytest.fixture(scope="module")
def policycheck():
    lib = ctypes.CDLL(helpers.built("tests/policycheck", "libpolicycheck.so"))
    vp = ctypes.c_void_p
    lib.pc_map.argtypes = [ctypes.c_int, vp, vp, ctypes.c_longlong]
    lib.pc_select.argtypes = [vp, ctypes.c_int, ctypes.c_double]
    lib.pc_draws.argtypes = [vp, ctypes.c_int, vp]
    lib.pc_params_size.restype = ctypes.c_ulonglong
    lib.pc_params_size.argtypes = [vp]
    lib.pc_forward.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp]
    return lib


def host_map(lib, which, x):
    x = np.ascontiguousarray(x, dtype=F32)
    y = np.empty_like(x)
    lib.pc_map(which, x.ctypes.data, y.ctypes.data, x.size)
    return y


def floats_between(low, high, stride):
    """Every stride-th float32 from -0.0 down to `low` (both negative or zero), by bit pattern."""
    first, last = int(F32(high).view(np.uint32)), int(F32(low).view(np.uint32))
    return np.arange(first, last + 1, stride, dtype=np.uint64).astype(np.uint32).view(F32)


# ---- 1: the host build of the header equals the twin ---------------------------------------------------------------------
def test_exp32_of_the_header_equals_the_twin(policycheck):
    x = np.concatenate([floats_between(-88.0, -0.0, 1000), F32([-88.0, -87.0, 0.0, -0.0, -np.inf, np.nan, -1e-40])])
    assert x.size >= 10 ** 6 and (x == F32(-88.0)).any() and (x.view(np.uint32) == 0x80000000).any()
    got, want = host_map(policycheck, 0, x), policy.exp32(x)
    assert bits(got) == bits(want)
    assert bits(policy.exp32(F32([0.0, -0.0]))) == bits(F32([1.0, 1.0]))  # exactly 1
    below = policy.exp32(F32([-87.00001, -88.0, -1000.0, -np.inf, np.nan]))
    assert bits(below) == bits(np.zeros(5, dtype=F32))  # +0, never a subnormal
    live = want[x >= F32(-87.0)]
    assert live.min() >= np.finfo(F32).tiny and live.max() == F32(1.0)


def test_log32_of_the_header_equals_the_twin(policycheck):
    s = np.concatenate([np.linspace(1.0, 64.0, 100001).astype(F32), np.arange(1, 65, dtype=F32),
                        np.nextafter(F32(2.0) ** np.arange(0, 7), F32(0.0)).astype(F32)[1:]])
    assert s.size >= 10 ** 5
    assert bits(host_map(policycheck, 1, s)) == bits(policy.log32(s))
    assert policy.log32(F32([1.0]))[0] == 0.0


def test_tanh32_of_the_header_equals_the_twin(policycheck):
    x = np.concatenate([F32([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 3e38, -3e38]),
                        np.linspace(-50.0, 50.0, 20001).astype(F32),
                        (np.random.default_rng(0).standard_normal(20000) * 1e-3).astype(F32)])
    got, want = policy.canonical(host_map(policycheck, 2, x)), policy.tanh32(x)
    assert bits(got) == bits(want)
    assert bits(want[:5]) == bits(np.array([0.0, -0.0, 1.0, -1.0, policy._NAN], dtype=F32))
    assert (np.abs(want[5:]) <= 1.0).all()


def test_relu_turns_nan_and_negative_zero_into_zero():
    got = policy.activation(F32([np.nan, -0.0, -1.0, 2.0, np.inf, -np.inf, 1e-40]), "relu")
    assert bits(got) == bits(F32([0.0, 0.0, 0.0, 2.0, np.inf, 0.0, 1e-40]))


def host_forward(lib, spec, params, obs, final_obs, gen, deterministic):
    n = obs.shape[0]
    out = dict(actions=np.zeros(n, dtype=np.int64), log_probs=np.zeros(n, dtype=F32), values=np.zeros(n, dtype=F32),
               final_values=np.zeros(n, dtype=F32), logits=np.zeros((n, spec.n_actions), dtype=F32))
    desc = _native.PolicyDesc(*spec.desc())
    assert lib.pc_params_size(ctypes.byref(desc)) == spec.size == params.size
    words = None if gen is None else (ctypes.c_ulonglong * 4)(*gen)
    obs, final_obs = np.ascontiguousarray(obs), np.ascontiguousarray(final_obs)
    assert lib.pc_forward(ctypes.byref(desc), params.ctypes.data, n, obs.ctypes.data, final_obs.ctypes.data, words,
                          policy.DETERMINISTIC if deterministic else 0, *(out[k].ctypes.data for k in cases.OUTPUTS)) == 0
    return out


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)))
def test_forward_of_the_header_equals_the_twin(index, n, policycheck):
    """The inputs of tests/test_gpu_policy.py -- +-0, +-inf, subnormals, NaN rows, logits that tie exactly and one 200
    below, NaN-led final_obs rows among live ones --, sampled at draw offsets 0 and 2^32 + 5 and deterministic:
    actions, log_probs, values, final_values and logits as bytes."""
    spec, params, obs, final_obs = cases.forward_inputs(index, n)
    for mode, offset in cases.MODES:
        want = cases.wanted_forward(spec, params, obs, final_obs, mode, offset)
        gen = policy.generator_words(cases.generator_at(offset)[0]) if mode == "sampled" else None
        got = host_forward(policycheck, spec, params, obs, final_obs, gen, mode == "deterministic")
        for name in cases.OUTPUTS:
            assert bits(got[name]) == bits(want[name]), (mode, offset, name)


def test_hostile_inputs_hold_what_they_promise():
    spec, params, obs, final_obs = cases.forward_inputs(1, 29)
    raw = obs.view(np.uint32)
    for special in (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001):  # +-0, +-inf, the least subnormal
        assert (raw == special).any(), hex(special)
    assert np.isnan(obs).any() and np.isnan(final_obs[1::3]).all()
    assert np.isnan(final_obs[0, 0]) and not np.isnan(final_obs[0, 1:]).any()
    want = cases.wanted_forward(spec, params, obs, final_obs, "sampled", 0)
    led = np.isnan(final_obs[:, 0])
    live = np.isfinite(final_obs).all(axis=1)
    assert live.sum() >= 5 and np.isfinite(want["final_values"][live]).all()
    assert (want["final_values"][led].view(np.uint32) == policy.NAN_BITS).all() and 0 < led.sum() < 29
    finite = np.isfinite(want["logits"]).all(axis=1)
    assert finite.sum() >= 10 and not finite.all()
    logits = want["logits"][finite]
    assert (logits[:, 0] == logits[:, 1]).all()  # exact ties
    assert (logits[:, :-1].max(axis=1) - logits[:, -1] > 150).all()  # 200 apart: e_i == 0
    assert (want["actions"][finite] != 12).all() and np.isfinite(want["log_probs"][finite]).all()
    # degenerate rows: log_prob is the one NaN, the action the first maximum
    degenerate = ~finite
    assert (want["log_probs"][degenerate].view(np.uint32) == policy.NAN_BITS).all()
    assert (want["logits"].view(np.uint32)[np.isnan(want["logits"])] == policy.NAN_BITS).all()


def test_the_outcome_for_nan_and_infinite_logits():
    nan, inf = F32(np.nan), F32(np.inf)
    logits = np.array([[0.0, nan, 1.0], [nan, 5.0, 1.0], [0.0, inf, 1.0], [-inf, -inf, -inf], [-inf, 0.0, -inf],
                       [0.0, -inf, 0.0]], dtype=F32)
    u = np.array([0.999, 0.5, 0.5, 0.5, 0.999, 0.75])
    actions, log_probs = policy.head(logits, u)
    # a NaN beside a finite maximum is never sampled; a NaN l_0 stays the maximum; a +inf or all -inf row is degenerate
    assert actions.tolist() == [2, 0, 1, 0, 1, 2]
    assert np.isnan(log_probs[[1, 2, 3]]).all() and (log_probs[[1, 2, 3]].view(np.uint32) == policy.NAN_BITS).all()
    assert log_probs[4] == 0.0 and log_probs[5] == -policy.log32(F32([2.0]))[0]
    assert policy.head(logits)[0].tolist() == [2, 0, 1, 0, 1, 0]  # deterministic: the first maximum


def test_selection_rule_on_hand_made_sums(policycheck):
    """Ties (a c_i that repeats: an e_i of 0 is never chosen), u next to a boundary on either side, u = 0 and the
    largest u, and a sum the float64 product rounds up to: none is above, the last index is taken."""
    rows = [([0.25, 0.25, 0.5, 1.0], [0.0, 0.25 - 2.0 ** -54, 0.25, 0.25 + 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53]),
            ([1.0, 1.0, 1.0], [0.0, 0.5, 1.0 - 2.0 ** -53]),
            ([0.0, 0.0, 1.0, 1.0], [0.0, 0.999]),
            ([1.0, 2.0, 3.0], [1.0 / 3.0, np.nextafter(1.0 / 3.0, 0.0), 2.0 / 3.0, np.nextafter(2.0 / 3.0, 1.0)]),
            ([3.0, 3.0], [1.0])]  # (u = 1 is never drawn: nothing is above, the last index)
    expected = [[0, 0, 2, 2, 3, 3], [0, 0, 0], [2, 2], [1, 0, 2, 2], [1]]
    for (c, us), want in zip(rows, expected):
        c = np.array(c, dtype=F32)
        twin = [int(policy.select(c[None, :], np.array([u]))[0]) for u in us]
        host = [policycheck.pc_select(c.ctypes.data, len(c), float(u)) for u in us]
        assert twin == host == want, (c, us, twin, host)


@pytest.mark.parametrize("offset", [0, 1, 2 ** 32 + 5])
def test_draws_of_the_lanes_are_numpys(offset, policycheck):
    lanes = 65
    bit_generator, generator = cases.generator_at(offset)
    words = (ctypes.c_ulonglong * 4)(*policy.generator_words(bit_generator))
    got = np.zeros(lanes)
    policycheck.pc_draws(words, lanes, got.ctypes.data)
    assert bits(got) == bits(generator.random(lanes))
    if offset == 1:  # (advance() itself: draw number offset + e of the generator)
        assert bits(got) == bits(np.random.Generator(np.random.PCG64DXSM(cases.SEED)).random(1 + lanes)[1:])


# ---- 2: the accuracy of the definition -----------------------------------------------------------------------------------
def test_exp32_and_log32_against_float64():
    x = np.concatenate([floats_between(-87.0, -0.0, 997), F32([-87.0, 0.0])])
    relative = np.abs(policy.exp32(x).astype(np.float64) / np.exp(x.astype(np.float64)) - 1.0)
    print("exp32: largest relative error 2^%.2f" % np.log2(relative.max()))
    assert relative.max() <= 2.0 ** -21
    s = np.concatenate([np.linspace(1.0, 64.0, 400001).astype(F32), np.arange(1, 65, dtype=F32)])
    exact = np.log(s.astype(np.float64))
    error = np.abs(policy.log32(s).astype(np.float64) - exact) / np.maximum(1.0, exact)
    print("log32: largest error over max(1, log s) 2^%.2f" % np.log2(error.max()))
    assert error.max() <= 2.0 ** -21


@pytest.mark.parametrize("count", [2, 13, 64])
def test_log_probs_against_float64_log_softmax(count):
    """From the same float32 logits, |z| <= 30: within 2^-17 max(1, |log p|) -- 64 summands, the two functions and two
    subtractions."""
    rng = np.random.default_rng(count)
    logits = (rng.uniform(-15.0, 15.0, (4096, count)) * rng.uniform(0.0, 1.0, (4096, 1))).astype(F32)
    logits[:64] = logits[:64].round()  # (ties)
    logits[64:128, 0] = logits[64:128, 1:].min(axis=1) + F32(30.0)  # (the whole range: the others' e_i are tiny)
    assert (logits.max(axis=1) - logits.min(axis=1)).max() <= 30.0 + 1e-3
    wide = logits.astype(np.float64)
    shifted = wide - wide.max(axis=1, keepdims=True)
    exact = shifted - np.log(np.exp(shifted).sum(axis=1, keepdims=True))
    error = np.abs(policy.log_softmax(logits).astype(np.float64) - exact) / np.maximum(1.0, np.abs(exact))
    print("log_prob: largest error over max(1, |log p|) 2^%.2f" % np.log2(error.max()))
    assert error.max() <= 2.0 ** -17


@pytest.mark.parametrize("width", [1, 20, 256])
def test_one_linear_layer_against_float64(width):
    rng = np.random.default_rng(width)
    x = (rng.standard_normal((64, width)) * 10.0 ** rng.uniform(-2, 2, (64, width))).astype(F32)
    weight_t = rng.standard_normal((width, 33)).astype(F32)
    bias = rng.standard_normal(33).astype(F32)
    got = policy.linear(x, weight_t, bias).astype(np.float64)
    exact = bias.astype(np.float64) + x.astype(np.float64) @ weight_t.astype(np.float64)
    size = np.abs(bias.astype(np.float64)) + np.abs(x.astype(np.float64)) @ np.abs(weight_t.astype(np.float64))
    assert (np.abs(got - exact) <= (width + 2) * 2.0 ** -24 * size).all()


def float64_forward(spec, state, obs):
    def net(extractor, head_name, widths):
        x = obs.astype(np.float64)
        for i in range(len(widths)):
            x = x @ state[f"mlp_extractor.{extractor}.{2 * i}.weight"].astype(np.float64).T \
                + state[f"mlp_extractor.{extractor}.{2 * i}.bias"]
            x = np.tanh(x) if spec.activation == "tanh" else np.maximum(x, 0.0)
        return x @ state[head_name + ".weight"].astype(np.float64).T + state[head_name + ".bias"]

    logits = net("policy_net", "action_net", spec.pi)
    shifted = logits - logits.max(axis=1, keepdims=True)
    return shifted - np.log(np.exp(shifted).sum(axis=1, keepdims=True)), net("value_net", "value_net", spec.vf)[:, 0]


@pytest.mark.parametrize("index", [1, 2])
def test_whole_network_is_no_further_from_float64_than_four_times_torch(index, tmp_path):
    """Per output kind (the log-probabilities of every action, the values), the largest distance from a float64
    forward: the twin's may be at most 4 x that of torch's CPU float32 forward of the same state_dict on the same
    inputs.  Both are measured here (profiles/policy.md records a run); torch runs in a process of its own."""
    spec = cases.spec_of(cases.NETWORKS[index])
    state = cases.state_dict(spec, 50 + index)
    obs = np.random.default_rng(index).standard_normal((2048, spec.obs_width)).astype(F32)
    np.savez(tmp_path / "in.npz", obs=obs, activation=spec.activation, **state)
    subprocess.run([sys.executable, "-m", "tests.policy_io_cases", "--torch-forward", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=300)
    theirs = np.load(tmp_path / "out.npz")
    params = spec.pack(state)
    pi, vf = spec.nets(params)
    ours = {"log_probs": policy.log_softmax(policy._net(spec, pi, obs)),
            "values": policy.policy_numpy(spec, params, obs, values_only=True)["values"]}
    exact = dict(zip(("log_probs", "values"), float64_forward(spec, state, obs)))
    for kind in ("log_probs", "values"):
        twin = np.abs(ours[kind].astype(np.float64) - exact[kind]).max()
        torch = np.abs(theirs[kind].astype(np.float64) - exact[kind]).max()
        print(f"{cases.NETWORKS[index]}: {kind}: twin {twin:.3e}, torch {torch:.3e}, ratio {twin / torch:.2f}")
        assert theirs[kind].dtype == F32 and twin <= 4.0 * torch, (kind, twin, torch)


# ---- 3: sampling ---------------------------------------------------------------------------------------------------------
def test_sampling_frequencies():
    """Fixed logits over 2^16 rows, seed 0: every action's frequency within 6 sqrt(p (1 - p) / N) of the float64 softmax
    probability (deterministic: the draws are numpy's)."""
    rows, count = 2 ** 16, 13
    logits = F32(np.sin(np.arange(count) * 1.7) * 2.5)
    u = np.random.Generator(np.random.PCG64DXSM(0)).random(rows)
    actions, log_probs = policy.head(np.tile(logits, (rows, 1)), u)
    wide = np.exp(logits.astype(np.float64) - logits.max())
    p = wide / wide.sum()
    frequency = np.bincount(actions, minlength=count) / rows
    print("largest deviation in sigmas: %.2f" % (np.abs(frequency - p) / np.sqrt(p * (1 - p) / rows)).max())
    assert (np.abs(frequency - p) <= 6.0 * np.sqrt(p * (1.0 - p) / rows)).all()
    assert np.allclose(log_probs, np.log(p)[actions], atol=1e-5)


# ---- 4: the generator -----------------------------------------------------------------------------------------------------
def test_generator_accounting():
    spec = cases.spec_of(cases.NETWORKS[1])
    twin = harness.Policy(spec, 7)
    twin.load_state_dict(cases.state_dict(spec, 1))
    obs = cases.hostile_rows(20, 9, 0, False)
    start = twin.rng_state()
    twin.act(obs, deterministic=True)
    twin.values(obs)
    twin.values(obs, cases.hostile_rows(20, 9, 1, True))
    assert twin.rng_state() == start  # no draw
    first, second = twin.act(obs), twin.act(obs)
    u = np.random.Generator(np.random.PCG64DXSM(7)).random(18)
    for got, draws in ((first, u[:9]), (second, u[9:])):
        want = policy.policy_numpy(spec, twin.params, obs, None, draws)
        assert bits(got[0]) == bits(want["actions"]) and bits(got[2]) == bits(want["log_probs"])
        assert bits(got[1]) == bits(want["values"]) and got[3] is None
    after = twin.rng_state()
    twin.set_rng_state(start)
    assert twin.rng_state() == start
    again = twin.act(obs)
    assert bits(again[0]) == bits(first[0]) and bits(again[2]) == bits(first[2])
    other = harness.Policy(spec, 99)
    other.set_rng_state(after)  # (a state travels between policies)
    other.load_state_dict(twin.state_dict())
    assert bits(other.params) == bits(twin.params)
    twin.set_rng_state(after)
    assert bits(other.act(obs)[0]) == bits(twin.act(obs)[0])
    # the words the device gets are the generator's: advancing by n on the host is drawing n
    bit_generator = np.random.PCG64DXSM(7)
    bit_generator.advance(18)
    restored = np.random.PCG64DXSM(0)
    restored.state = after
    assert policy.generator_words(bit_generator) == policy.generator_words(restored)


# ---- 5: the packing and the buffers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)))
def test_packing_round_trip_and_layout(index):
    spec = cases.spec_of(cases.NETWORKS[index])
    state = cases.state_dict(spec, index)
    params = spec.pack(state)
    assert params.dtype == F32 and params.shape == (spec.size,)
    back = spec.unpack(params)
    assert sorted(back) == sorted(state) == sorted(spec.keys())
    for name in state:
        assert bits(back[name]) == bits(state[name]), name
    # transposed: element [k][j] of the packed first layer is weight[j][k]
    weight = state["mlp_extractor.policy_net.0.weight"]
    assert bits(params[:weight.size].reshape(weight.shape[::-1])) == bits(np.ascontiguousarray(weight.T))
    with pytest.raises(KeyError, match="missing"):
        spec.pack({k: v for k, v in state.items() if k != "value_net.bias"})
    with pytest.raises(KeyError, match="unknown"):
        spec.pack(dict(state, log_std=np.zeros(1)))
    with pytest.raises(ValueError, match="shape"):
        spec.pack(dict(state, **{"action_net.weight": state["action_net.weight"].T}))


def test_specs_outside_the_limits_are_refused():
    for kw in (dict(obs_width=0), dict(obs_width=257), dict(n_actions=1), dict(n_actions=65), dict(pi=()), dict(pi=(8, 8, 8)),
               dict(vf=(257,)), dict(vf=(0,)), dict(activation="gelu")):
        with pytest.raises(ValueError):
            policy.MlpPolicySpec(**dict(dict(obs_width=4, n_actions=13), **kw))


@pytest.mark.parametrize("kind", sorted(cases.E2E_KINDS))
def test_twin_collect_equals_the_explicit_loop(kind, no_gpu):  # noqa: F811
    """VectorDiscreteSteps with records and the learner view, and with neither: every slab, advantages, returns and
    flat() of two consecutive rollouts as bytes; environments end inside them."""
    n = 5
    got, want = cases.twin_runs(kind, n), cases.twin_runs(kind, n, explicit=True)
    cases.same_runs(got, want)
    assert np.concatenate([run["truncated"] for run in got]).any()
    assert len({run["actions"].tobytes() for run in got}) == 2 and len(np.unique(got[0]["actions"])) > 1
    if cases.E2E_KINDS[kind]["records"]:
        for run in got:
            assert bits(np.isnan(run["final_values"])) == bits(run["truncated"] == 0)
    assert not np.isnan(got[1]["advantages"]).any()


def test_collect_refusals(no_gpu):  # noqa: F811
    from tests import rollout_io_cases

    env = cases.make_env("plain", 3, False)
    spec = cases.e2e_spec("plain")
    buffer = harness.Rollout(env, 2)
    twin = harness.Policy(spec, 0)
    with pytest.raises(ValueError, match="start"):
        buffer.collect(twin)
    obs, _ = env.reset()
    buffer.start(obs)
    buffer.step(np.zeros(3, dtype=np.int64), np.zeros(3, dtype=F32), np.zeros(3, dtype=F32))
    with pytest.raises(ValueError, match="whole rollout"):
        buffer.collect(twin)
    env.close()
    jumps = harness.VectorContinuousJumps(num_envs=2, **rollout_io_cases.ENV_KW)
    buffer = harness.Rollout(jumps, 2)
    buffer.start(jumps.reset()[0])
    with pytest.raises(ValueError, match="out of scope"):
        buffer.collect(twin)
    with pytest.raises(TypeError, match="device-resident"):
        harness.DevicePolicy(jumps, spec, 0)
    jumps.close()


def test_import_stays_free_of_torch():
    code = ("import sys; from reinfocus_amd.environments import harness; harness.Policy; harness.DevicePolicy; "
            "assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


# ---- 6: the binding and the constants -------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    struct = re.search(r"typedef struct rf_policy_desc \{(.*?)\} rf_policy_desc;", text, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = [(m.group(1), int(m.group(2) or 1)) for m in re.finditer(r"int (\w+)(?:\[(\d+)\])?;", struct)]
    assert fields == [(name, getattr(kind, "_length_", 1)) for name, kind in _native.PolicyDesc._fields_]
    assert ctypes.sizeof(_native.PolicyDesc) == 4 * sum(count for _, count in fields)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"\bint\s+rf_policy_forward\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    wanted = [ctypes.c_void_p if ("*" in p or "[" in p) else ctypes.c_int for p in declaration.split(",")]
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    names = re.search(r"lib\.rf_policy_forward\.argtypes = \[(.*?)\]", source).group(1).split(",")
    assert [{"vp": ctypes.c_void_p, "i32": ctypes.c_int}[name.strip()] for name in names] == wanted and len(wanted) == 14
    for name, value in (("RF_POLICY_MAX_WIDTH", policy.MAX_WIDTH), ("RF_POLICY_MAX_ACTIONS", policy.MAX_ACTIONS),
                        ("RF_POLICY_RELU", policy.ACTIVATIONS["relu"]), ("RF_POLICY_TANH", policy.ACTIVATIONS["tanh"]),
                        ("RF_POLICY_DETERMINISTIC", policy.DETERMINISTIC)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value


def test_tile_of_the_gpu_shapes_is_the_kernels():
    text = open(os.path.join(ROOT, "reinfocus_amd", "csrc", "rf_policy.h")).read()
    assert int(re.search(r"constexpr int kPolicyTile = (\d+);", text).group(1)) == cases.TILE
    assert cases.SIZES == (1, cases.TILE, cases.TILE + 1, 3 * cases.TILE + 5)
