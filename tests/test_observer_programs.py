"""Observer strategy objects on the CPU: the public classes of environments/state_observer.py, the host twin
harness.VectorEnvironment(observer=...) and the observer program compiler (strategy_program.compile_observer).

* The classes reproduce the reference's own observer test numbers (tests/golden/reference_strategy_cases.json, each case
  with its file:line in the reference's tests), around stand-in leaf observers as the reference's tests use.
* The classes, run under the installed numpy, reproduce tests/golden/observer_program_cases.json bit for bit: the
  observations and the DeltaObservers' old values after every call of seeded random trees (tests/observer_programs.py),
  recorded under numpy 1.26 (tests/golden/make_observer_program_cases.py).
* VectorEnvironment(observer=default_observer(...)) equals VectorEnvironment(observer=None) step for step.
* The compiler's programs column by column, every refusal, and the ObservationRewarder index bound.
* The library exports the new entry points.
The device path runs against the twin in tests/test_gpu_observed_env.py."""

import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import episode_ender as ee
from reinfocus_amd.environments import episode_rewarder as er
from reinfocus_amd.environments import harness
from reinfocus_amd.environments import state_observer as so
from reinfocus_amd.environments import state_transformer as st
from reinfocus_amd.environments import strategy_program as sp
from tests import observer_programs as op
from tests.test_composed_env_logic import ENDS, continuous_jumps, discrete_steps
from tests.test_composed_programs import _numpy_126_python
from tests.test_continuous_vector_logic import FakeFocusObserver, FakeRenderer, _actions

HERE = os.path.dirname(os.path.abspath(__file__))
SCRIPT = os.path.join(HERE, "golden", "make_observer_program_cases.py")
FIXTURE = os.path.join(HERE, "golden", "observer_program_cases.json")
DATA = json.load(open(FIXTURE))
CASES = DATA["cases"]
REFERENCE = json.load(open(os.path.join(HERE, "golden", "reference_strategy_cases.json")))["cases"]


# ---- the reference's known answers ------------------------------------------------------------------------------------


class ValueLeaf(so.BaseObserver):
    """The reference tests' stand-in leaf: observes sign * (element 0 of the state) within [low, high]."""

    def __init__(self, num_envs, sign=1.0, low=-100.0, high=100.0):
        super().__init__(num_envs, low, high)
        self._sign = sign

    def observe(self, states, indices=None):
        if indices is None:
            indices = np.full(self.observation_space.shape[0], True)
        return (self._sign * states[:, 0]).reshape((indices.sum(), 1))


def _reference(name):
    found = [c for c in REFERENCE if c["name"] == name]
    assert len(found) == 1, name
    return found[0]


def _mask(call):
    return np.array(call["mask"]) if "mask" in call else None


def _states(values):
    states = np.zeros((len(values), 2), dtype=np.float32)
    states[:, 0] = values
    return states


def test_delta_observer_spaces():
    for call in _reference("delta_observer_spaces")["ops"]:
        leaves = [ValueLeaf(3, 1.0, low, high) for low, high in zip(call["lows"], call["highs"])]
        change = call["max_change"]
        if change is not None:
            change = np.array([np.nan if m is None else m for m in change], dtype=np.float32)
        space = so.DeltaObserver(leaves, call["include_original"], change).single_observation_space
        assert space.dtype == np.float32 and space.shape == (len(call["low"]),)
        assert np.array_equal(space.low, np.array(call["low"], dtype=np.float32))
        assert np.array_equal(space.high, np.array(call["high"], dtype=np.float32))
    # a number bounds every change; a single observer need not be in a list
    space = so.DeltaObserver(ValueLeaf(3, 1.0, 2.0, 5.0), True, 0.5).single_observation_space
    assert np.array_equal(space.low, np.float32([2.0, -0.5])) and np.array_equal(space.high, np.float32([5.0, 0.5]))
    assert so.DeltaObserver(ValueLeaf(3)).observation_space.shape == (3, 1)


@pytest.mark.parametrize("name", ["delta_observer_observation", "delta_observer_partial_observation",
                                  "delta_observer_observation_with_original", "delta_observer_observation_with_reset",
                                  "delta_observer_multidimensional"])
def test_delta_observer(name):
    case = _reference(name)
    n = case["params"]["num_envs"]
    original = any("originals" in call for call in case["ops"])
    two = any("negated_deltas" in call for call in case["ops"])
    leaves = [ValueLeaf(n), ValueLeaf(n, -1.0)] if two else [ValueLeaf(n)]
    observer = so.DeltaObserver(leaves if two else leaves[0], include_original=original)
    for call in case["ops"]:
        got = (observer.reset if call["op"] == "reset" else observer.observe)(_states(call["values"]), _mask(call))
        want = [call["deltas"]] + ([call.get("negated_deltas", [-d for d in call["deltas"]])] if two else [])
        if original:
            want = [call["originals"]] + want
        assert got.dtype == np.float32
        assert np.array_equal(got, np.array(want, dtype=np.float32).T)


def test_indexed_element_observer():
    case = _reference("indexed_element_observer")
    n = case["params"]["num_envs"]
    for call in case["ops"]:
        observer = so.IndexedElementObserver(n, call["index"], 0.0, 10.0)
        assert observer.single_observation_space.shape == (1,) and observer.observation_space.shape == (n, 1)
        got = observer.observe(np.array(call["states"], dtype=np.float32), _mask(call))
        assert np.array_equal(got, np.array(call["values"], dtype=np.float32).reshape(-1, 1))


def test_normalized_observer():
    case = _reference("normalized_observer_observation")
    lows, highs = case["params"]["lows"], case["params"]["highs"]
    observer = so.NormalizedObserver([ValueLeaf(5, 1.0, low, high) for low, high in zip(lows, highs)])
    space = observer.single_observation_space
    assert np.array_equal(space.low, -np.ones(2, dtype=np.float32)) and np.array_equal(space.high, np.ones(2, dtype=np.float32))
    for call in case["ops"]:
        got = (observer.reset if call["op"] == "reset" else observer.observe)(_states(call["values"]), _mask(call))
        assert got.dtype == np.float32
        np.testing.assert_allclose(got, call["normalized"], rtol=1e-6)


def test_wrapped_observers_share_their_number_of_environments():
    with pytest.raises(AssertionError, match="same number of environments"):
        so.NormalizedObserver([ValueLeaf(3), ValueLeaf(4)])
    with pytest.raises(NotImplementedError):
        so.WrapperObserver([ValueLeaf(3)], -1.0, 1.0).observe(_states([0, 1, 2]))


# ---- numpy 1.26 ---------------------------------------------------------------------------------------------------------


def _unbits(text, dtype=np.float32):
    size = np.dtype(dtype).itemsize
    words = [int(text[i:i + 2 * size], 16) for i in range(0, len(text), 2 * size)]
    return np.array(words, dtype=f"u{size}").view(dtype)


def recorded_calls(case):
    """The calls of a fixture case in the form observer_programs.run takes."""
    calls = []
    for call in case["calls"]:
        mask = None if call["mask"] is None else np.array([c == "1" for c in call["mask"]])
        calls.append({"op": call["op"], "mask": mask, "states": _unbits(call["states"]).reshape(-1, 2),
                      "focus": _unbits(call["focus"], np.float64)})
    return calls


@pytest.mark.parametrize("case", [pytest.param(c, id=f"width{c['width']}") for c in CASES])
def test_observer_classes_reproduce_numpy_126(case):
    n = DATA["num_envs"]
    results = list(op.run(case["spec"], recorded_calls(case)))
    assert len(results) == len(case["calls"])
    for t, ((observations, old), want) in enumerate(zip(results, case["calls"])):
        k = n if want["mask"] is None else want["mask"].count("1")
        assert observations.dtype == np.float32 and observations.shape == (k, case["width"]), t
        assert np.array_equal(observations.view(np.uint32), _unbits(want["observations"], np.uint32).reshape(k, -1)), t
        assert old.dtype == np.float32 and old.shape == (case["old_rows"], n), t
        assert np.array_equal(old.view(np.uint32).ravel(), _unbits(want["old"], np.uint32)), t


def test_recorded_inputs_are_the_generated_ones():
    for case in CASES:
        for got, want in zip(recorded_calls(case), op.inputs(case["spec"])):
            assert got["op"] == want["op"] and np.array_equal(got["mask"], want["mask"])
            assert np.array_equal(got["states"], want["states"]) and np.array_equal(got["focus"], want["focus"])


def test_fixture_holds_the_generated_trees_and_they_cover_the_program():
    assert DATA["numpy"].startswith("1.26") and DATA["num_envs"] == op.NUM_ENVS
    specs = [c["spec"] for c in CASES]
    assert specs == json.loads(json.dumps([op.program(seed) for seed in op.SEEDS]))
    assert os.path.getsize(FIXTURE) < 200_000
    trees = [s["tree"] for s in specs]
    assert [op.width(t) for t in trees] == list(range(1, 17)) == [c["width"] for c in CASES]
    nodes = [node for t in trees for node in op.nodes(t)]
    assert {node["class"] for node in nodes} == {"FocusObserver", "IndexedElementObserver", "DeltaObserver",
                                                 "NormalizedObserver"}
    deltas = [node for node in nodes if node["class"] == "DeltaObserver"]
    assert {node["include_original"] for node in deltas} == {True, False}
    assert {None if node["max_change"] is None else node["max_change"][0] for node in deltas} == {None, "scalar", "array"}
    assert any("nan" in node["max_change"][1] for node in deltas if node["max_change"] and node["max_change"][0] == "array")
    assert sum(op.delta_of_delta(t) for t in trees) >= 4
    assert all(sum(node["class"] == "FocusObserver" for node in op.nodes(t)) == 1 for t in trees)
    assert max(len(op.nodes(t)) for t in trees) == op.MAX_NODES and max(op.old_rows(t) for t in trees) == op.MAX_OLD
    assert {node["index"] for node in nodes if node["class"] == "IndexedElementObserver"} == {0, 1}
    # some observations clip at either end, some old values are still NaN after the first reset of a partial mask
    values = np.concatenate([_unbits(call["observations"]) for c in CASES for call in c["calls"]])
    assert (values == 1.0).any() and (values == -1.0).any() and ((values > -1) & (values < 1) & (values != 0)).any()


def test_fixture_is_what_the_script_writes(tmp_path):
    python = _numpy_126_python()
    if python is None:
        pytest.skip("no interpreter with numpy 1.26 (set NUMPY126_PYTHON)")
    out = tmp_path / "cases.json"
    subprocess.run([python, SCRIPT, str(out)], check=True, timeout=600)
    with open(FIXTURE, "rb") as f:
        assert out.read_bytes() == f.read()


@pytest.mark.parametrize("case", [pytest.param(c, id=f"width{c['width']}") for c in CASES])
def test_compiler_accepts_every_tree(case):
    n = DATA["num_envs"]
    program = sp.compile_observer(op.build(case["spec"]["tree"], n, op.StandInFocus(n)), n)
    assert program.width == case["width"] and program.n_old == case["old_rows"]
    assert program.n_nodes == len(op.nodes(case["spec"]["tree"]))


# ---- the host twin --------------------------------------------------------------------------------------------------------


class DescribingRenderer(FakeRenderer):
    """FakeRenderer that says what the host twin asks a FocusObserver's renderer."""

    class _Ctx:
        device = 0

    def __init__(self, samples_per_pixel=100, **kwargs):
        super().__init__(**kwargs)
        self._samples_per_pixel = samples_per_pixel
        self._ctx = self._Ctx()


class DescribingFocusObserver(FakeFocusObserver):
    """FakeFocusObserver that keeps its renderer and frame height, as the real one does."""

    def __init__(self, num_envs, target_index, focus_plane_index, ends, renderer, frame_height=300):
        super().__init__(num_envs, target_index, focus_plane_index, ends, renderer, frame_height)
        self.observation_space = so.spaces.batch_space(self.single_observation_space, num_envs)
        self._target_index, self._focus_plane_index = target_index, focus_plane_index
        self._renderer, self._frame_height = renderer, frame_height


@pytest.fixture()
def no_gpu(monkeypatch):
    monkeypatch.setattr(harness.render, "FastRenderer", DescribingRenderer)
    monkeypatch.setattr(harness.state_observer, "FocusObserver", DescribingFocusObserver)


@pytest.mark.parametrize("composition", [discrete_steps, continuous_jumps])
def test_default_observer_restates_the_built_in_one(composition, no_gpu):
    n = 37
    built_in = harness.VectorEnvironment(**composition(n, 9, seed=5))
    renderer = DescribingRenderer()
    restated = harness.VectorEnvironment(**composition(n, 9, seed=5),
                                         observer=harness.default_observer(n, ENDS, 5.0, renderer))
    assert restated._renderer is renderer
    for name in ("single_observation_space", "observation_space"):
        a, b = getattr(built_in, name), getattr(restated, name)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.low, b.low) and np.array_equal(a.high, b.high)
    want, got = built_in.reset()[0], restated.reset()[0]
    assert got.dtype == want.dtype and np.array_equal(got, want)
    rng = np.random.default_rng(3)
    resets = 0
    for _ in range(60):
        actions = rng.integers(0, 13, n) if composition is discrete_steps else _actions(rng, built_in._state)
        want, got = built_in.step(actions), restated.step(actions)
        for x, y in zip(got[:4], want[:4]):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
        assert np.array_equal(built_in._state, restated._state)
        assert np.array_equal(restated.observer_state(), built_in._observer._old.T, equal_nan=True)
        resets += int(want[3].sum())
    assert resets > n
    with pytest.raises(AssertionError, match="not given an observer"):
        built_in.observer_state()


def test_host_twin_takes_the_focus_observers_renderer_or_refuses(no_gpu):
    n = 4
    make = lambda **kw: harness.default_observer(n, ENDS, 5.0, DescribingRenderer(samples_per_pixel=7), **kw)  # noqa: E731
    env = harness.VectorEnvironment(**discrete_steps(n), observer=make(frame_height=40), frame_height=40,
                                    samples_per_pixel=7, device=0)
    assert env._focus_observer._frame_height == 40
    for bad in (dict(frame_height=41), dict(samples_per_pixel=8), dict(device=1)):
        with pytest.raises(AssertionError, match="FocusObserver"):
            harness.VectorEnvironment(**discrete_steps(n), observer=make(frame_height=40), **bad)
    with pytest.raises(AssertionError, match="num_envs"):
        harness.VectorEnvironment(**discrete_steps(n + 1), observer=make())
    for bad in (4, -1, 1.0):
        with pytest.raises(AssertionError, match="focus_observation_index"):
            harness.VectorEnvironment(**discrete_steps(n), observer=make(), focus_observation_index=bad)
    with pytest.raises(AssertionError, match="focus_observation_index"):
        harness.VectorEnvironment(**discrete_steps(n), focus_observation_index=4)
    wide = harness.VectorEnvironment(**discrete_steps(n), observer=make(), focus_observation_index=3)
    assert wide._visualizer._columns["value"] == 3


# ---- the compiler -----------------------------------------------------------------------------------------------------------


def _node(program, k):
    node = program.nodes[k]
    return (node.kind, node.index, node.first, node.width, node.include_original, node.old_first)


def _leaves(n):
    return so.IndexedElementObserver(n, 0, 5.0, 10.0), so.IndexedElementObserver(n, 1, 4.0, 12.0), op.StandInFocus(n)


def test_program_of_the_default_tree():
    n = 3
    _, position, focus = _leaves(n)
    delta = so.DeltaObserver([position, focus], True, np.array([5.0, np.nan], dtype=np.float32))
    root = so.NormalizedObserver(delta)
    program = sp.compile_observer(root, n)
    assert (program.n_nodes, program.width, program.n_old) == (4, 4, 2)
    assert _node(program, 0) == (so.INDEXED_ELEMENT, 1, 0, 1, 0, 0)
    assert _node(program, 1) == (so.FOCUS, 0, 1, 1, 0, 0)
    assert _node(program, 2) == (so.DELTA, 0, 0, 2, 1, 0)
    assert _node(program, 3) == (so.NORMALIZED, 0, 0, 4, 0, 0)
    mid, scale = harness.delta_bounds([4.0, 0.0], [12.0, 1000.0], [5.0, np.nan], True)
    mid, scale = harness.normaliser_from_bounds(mid, scale)
    assert list(program.nodes[3].mid[:4]) == list(mid) == [8.0, 500.0, 0.0, 0.0]
    assert list(program.nodes[3].scale[:4]) == list(scale) == [4.0, 500.0, 5.0, 1000.0]


def test_program_of_a_tree_without_deltas():
    n = 3
    target, position, focus = _leaves(n)
    program = sp.compile_observer(so.NormalizedObserver([target, position, focus]), n)
    assert (program.n_nodes, program.width, program.n_old) == (4, 3, 0)
    assert [_node(program, k)[:4] for k in range(4)] == [(so.INDEXED_ELEMENT, 0, 0, 1), (so.INDEXED_ELEMENT, 1, 1, 1),
                                                         (so.FOCUS, 0, 2, 1), (so.NORMALIZED, 0, 0, 3)]
    assert list(program.nodes[3].mid[:3]) == [7.5, 8.0, 500.0] and list(program.nodes[3].scale[:3]) == [2.5, 4.0, 500.0]


def test_program_of_a_delta_of_a_delta_next_to_a_leaf():
    n = 3
    target, position, focus = _leaves(n)
    inner = so.DeltaObserver([position, focus], True)  # columns 1-4, old rows 0-1
    outer = so.DeltaObserver(inner, False, 2.0)  # in place on columns 1-4, old rows 2-5
    root = so.NormalizedObserver([target, outer])
    program = sp.compile_observer(root, n)
    assert (program.n_nodes, program.width, program.n_old) == (6, 5, 6)
    assert [_node(program, k) for k in range(6)] == [
        (so.INDEXED_ELEMENT, 0, 0, 1, 0, 0), (so.INDEXED_ELEMENT, 1, 1, 1, 0, 0), (so.FOCUS, 0, 2, 1, 0, 0),
        (so.DELTA, 0, 1, 2, 1, 0), (so.DELTA, 0, 1, 4, 0, 2), (so.NORMALIZED, 0, 0, 5, 0, 0)]
    assert list(program.nodes[5].mid[:5]) == [7.5, 0.0, 0.0, 0.0, 0.0]
    assert list(program.nodes[5].scale[:5]) == [2.5, 2.0, 2.0, 2.0, 2.0]
    # the host twin's old values in the same order
    states = np.array([[6.0, 7.0], [8.0, 9.0], [5.0, 5.5]], dtype=np.float32)
    focus.next = [10.0, 20.0, 30.0]
    root.reset(states)
    old = sp.host_observer_state(root, n)
    assert old.shape == (6, n) and old.dtype == np.float32
    assert np.array_equal(old, np.float32([[7, 9, 5.5], [10, 20, 30], [7, 9, 5.5], [10, 20, 30], [0, 0, 0], [0, 0, 0]]))


class UnknownObserver(so.BaseObserver):
    def observe(self, states, indices=None):
        return states[:, :1]


def _wide(n, leaves):
    return [so.IndexedElementObserver(n, 0, 5.0, 10.0) for _ in range(leaves)]


@pytest.mark.parametrize("make,match", [
    (lambda n: so.NormalizedObserver(_leaves(n)[:2]), "0 FocusObservers"),
    (lambda n: so.NormalizedObserver([op.StandInFocus(n), so.DeltaObserver(op.StandInFocus(n))]), "2 FocusObservers"),
    (lambda n: op.StandInFocus(n), "alone"),
    (lambda n: so.NormalizedObserver(UnknownObserver(n, 0.0, 1.0)), "0 FocusObservers"),
    (lambda n: so.NormalizedObserver([UnknownObserver(n, 0.0, 1.0), op.StandInFocus(n)]), "unsupported observer"),
    (lambda n: so.WrapperObserver([op.StandInFocus(n)], 0.0, 1.0), "unsupported observer"),
    (lambda n: so.NormalizedObserver([so.IndexedElementObserver(n, 2, 0.0, 1.0), op.StandInFocus(n)]), "state index"),
    (lambda n: so.NormalizedObserver([so.IndexedElementObserver(n, -1, 0.0, 1.0), op.StandInFocus(n)]), "state index"),
    (lambda n: so.NormalizedObserver(_leaves(n + 1)), "num_envs"),
    (lambda n: so.NormalizedObserver([so.IndexedElementObserver(n, 0, 0.0, np.inf), op.StandInFocus(n)]), "not finite"),
    (lambda n: so.NormalizedObserver([so.IndexedElementObserver(n, 0, -np.inf, 1.0), op.StandInFocus(n)]), "not finite"),
    (lambda n: so.NormalizedObserver([so.IndexedElementObserver(n, 0, 3.0, 3.0), op.StandInFocus(n)]), "scale"),
    (lambda n: so.NormalizedObserver(so.DeltaObserver(op.StandInFocus(n), False, 0.0)), "scale"),
    (lambda n: so.NormalizedObserver(_wide(n, 16) + [op.StandInFocus(n)]), "at most 16"),  # 18 nodes
    (lambda n: so.DeltaObserver(_wide(n, 8) + [op.StandInFocus(n)], True), "at most 16"),  # 18 columns
    (lambda n: so.DeltaObserver(so.DeltaObserver(so.DeltaObserver(_wide(n, 3) + [op.StandInFocus(n)], True), False), False),
     "old-value"),  # 4 + 8 + 8 old-value rows in 8 columns
])
def test_compiler_refuses(make, match):
    n = 4
    sp.compile_observer(so.NormalizedObserver(_leaves(n)), n)  # (a supported tree compiles)
    with pytest.raises(AssertionError, match=match):
        sp.compile_observer(make(n), n)


def test_compiler_refuses_other_focus_indices_and_an_object_used_twice():
    n = 4
    swapped = op.StandInFocus(n)
    swapped._target_index, swapped._focus_plane_index = 1, 0
    with pytest.raises(AssertionError, match=r"not \(0, 1\)"):
        sp.compile_observer(so.NormalizedObserver(swapped), n)
    leaf, focus = so.IndexedElementObserver(n, 0, 5.0, 10.0), op.StandInFocus(n)
    with pytest.raises(AssertionError, match="once"):
        sp.compile_observer(so.NormalizedObserver([leaf, leaf, focus]), n)
    delta = so.DeltaObserver(focus)
    with pytest.raises(AssertionError, match="once"):
        sp.compile_observer(so.NormalizedObserver([delta, delta]), n)


def test_observation_rewarder_index_follows_the_width():
    n = 4
    objects = dict(transformer=st.ContinuousJumpTransformer(n, 1, ENDS), ender=ee.EndlessEnder(n), num_envs=n)
    three = lambda: so.NormalizedObserver(_leaves(n))  # noqa: E731
    eight = lambda: so.DeltaObserver(so.DeltaObserver(_leaves(n)[1:], True), True)  # noqa: E731
    program, observer_program = sp.compile_program(rewarder=er.ObservationRewarder(2), observer=three(), **objects)
    assert program.rewarders[0].index0 == 2 and observer_program.width == 3
    with pytest.raises(AssertionError, match="observation index 3 outside 0-2"):
        sp.compile_program(rewarder=er.ObservationRewarder(3), observer=three(), **objects)
    program, observer_program = sp.compile_program(rewarder=er.ObservationRewarder(7), observer=eight(), **objects)
    assert program.rewarders[0].index0 == 7 and observer_program.width == 8
    with pytest.raises(AssertionError, match="observation index 8 outside 0-7"):
        sp.compile_program(rewarder=er.ObservationRewarder(8), observer=eight(), **objects)
    # the built-in observer's bound stays
    assert isinstance(sp.compile_program(rewarder=er.ObservationRewarder(3), **objects), _native.EnvProgram)
    with pytest.raises(AssertionError, match="observation index 4 outside 0-3"):
        sp.compile_program(rewarder=er.ObservationRewarder(4), **objects)
    with pytest.raises(AssertionError, match="num_envs"):
        sp.compile_program(rewarder=er.ObservationRewarder(0), observer=so.NormalizedObserver(_leaves(n + 1)), **objects)


def test_device_environment_refuses_sharding_with_an_observer():
    n = 4
    with pytest.raises(ValueError, match="devices"):
        harness.DeviceVectorEnvironment(**discrete_steps(n), observer=so.NormalizedObserver(_leaves(n)), devices=[0, 1])


# ---- the library --------------------------------------------------------------------------------------------------------------


def test_library_exports_the_observer_entry_points():
    assert os.path.exists(_native.LIB_PATH), "build with __graft_entry__.build() first"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("rf_env_configure_observed", "rf_env_get_observer_state"):
        assert name in _native.SYMBOLS and hasattr(lib, name), name
    text = open(os.path.join(os.path.dirname(HERE), "include", "reinfocus_hip.h")).read()
    assert f"#define RF_ENV_MAX_OBS_NODES {_native.MAX_OBS_NODES}\n" in text
    assert f"#define RF_ENV_MAX_OBS_COLUMNS {_native.MAX_OBS_COLUMNS}\n" in text
    # the ctypes structs are the header's: six ints, then mid and scale per column; three ints, then the nodes
    assert ctypes.sizeof(_native.EnvObserverNode) == 6 * 4 + 2 * 4 * _native.MAX_OBS_COLUMNS
    assert ctypes.sizeof(_native.EnvObserverProgram) == 3 * 4 + _native.MAX_OBS_NODES * ctypes.sizeof(_native.EnvObserverNode)
    assert (so.INDEXED_ELEMENT, so.FOCUS, so.DELTA, so.NORMALIZED) == (
        _native.OBS_INDEXED, _native.OBS_FOCUS, _native.OBS_DELTA, _native.OBS_NORMALIZED) == (0, 1, 2, 3)
