"""Composed environments on the CPU: the public strategy classes (environments/episode_ender.py, episode_rewarder.py,
state_transformer.py, state_initializer.py), the host twin harness.VectorEnvironment and the device program compiler
(environments/strategy_program.py).

* The classes reproduce the reference's own test numbers (tests/golden/composed_strategy_cases.json, each case with its
  file:line in the reference's tests/environments/).
* VectorEnvironment over the compositions that restate DiscreteSteps and ContinuousJumps equals
  harness.VectorDiscreteSteps / harness.VectorContinuousJumps step for step (those twins are pinned to numpy 1.26 by
  tests of their own), with the focus measure replaced by a function of the state (no GPU).
* Every reward term and operation has its numpy dtype; the compiler's postfix lists and every refusal.
The device path runs against the twin in tests/test_gpu_composed_env.py."""

import importlib.util
import json
import os

import numpy as np
import pytest
from numpy import testing

from reinfocus_amd.environments import episode_ender as ee
from reinfocus_amd.environments import episode_rewarder as er
from reinfocus_amd.environments import harness
from reinfocus_amd.environments import state_initializer as si
from reinfocus_amd.environments import state_transformer as st
from reinfocus_amd.environments import strategy_program as sp
from tests.test_continuous_vector_logic import FakeFocusObserver, FakeRenderer, _actions

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "composed_strategy_cases.json")))["cases"]
ENDS = (5.0, 10.0)
RADIUS = 0.25
MOVES = 5.0 / 2.0 ** np.arange(6)
ACTION_SET = np.concatenate([-MOVES, [0], MOVES[::-1]])


# ---- the reference's known answers ----------------------------------------------------------------------------------


def test_fixture_is_what_the_script_writes(tmp_path):
    spec = importlib.util.spec_from_file_location("mk", os.path.join(HERE, "golden", "make_composed_strategy_cases.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    assert json.loads(json.dumps({"cases": mk.CASES})) == {"cases": CASES}
    assert all(":" in c["source"] for c in CASES)
    assert {c["component"] for c in CASES} == {"ender", "rewarder", "transformer"}


class FixedEnder(ee.BaseEnder):
    """The reference tests' stand-in ender: fixed flags and status strings."""

    def __init__(self, terminated=None, truncated=None, status=None):
        self._t, self._u, self._s = terminated, truncated, status

    def is_terminated(self):
        return np.array(self._t)

    def is_truncated(self):
        return np.array(self._u)

    def status(self, index):
        return self._s[index]


class FixedRewarder(er.BaseRewarder):
    def __init__(self, values):
        self._values = np.array(values)

    def reward(self, states, observations):
        return self._values


def _build(spec, num_envs, module, fixed):
    if "fixed" in spec:
        return fixed(**spec["fixed"]) if isinstance(spec["fixed"], dict) else fixed(spec["fixed"])
    if "op" in spec:
        left, right = (_build(spec[k], num_envs, module, fixed) for k in ("left", "right"))
        return {"&": lambda: left & right, "|": lambda: left | right, "+": lambda: left + right,
                "*": lambda: left * right}[spec["op"]]()
    args = [tuple(a) if isinstance(a, list) and spec["class"] != "DiscreteJumpTransformer" else a for a in spec["args"]]
    cls = getattr(module, spec["class"])
    return cls(*args) if module is er else cls(num_envs, *args)


def _cases(component):
    return [pytest.param(c, id=c["name"]) for c in CASES if c["component"] == component]


@pytest.mark.parametrize("case", _cases("ender"))
def test_ender_known_answers(case):
    testee = _build(case["ender"], case["num_envs"], ee, FixedEnder)
    for op in case["ops"]:
        if op["op"] == "reset":
            testee.reset(np.array(op["states"]), np.array(op["mask"]) if "mask" in op else None)
        elif op["op"] == "step":
            testee.step(np.array(op["states"]))
        else:
            if "truncated" in op:
                testing.assert_array_equal(testee.is_truncated(), op["truncated"])
            if "terminated" in op:
                testing.assert_array_equal(testee.is_terminated(), op["terminated"])
            if "status" in op:
                assert [testee.status(i) for i in range(case["num_envs"])] == op["status"]


@pytest.mark.parametrize("case", _cases("rewarder"))
def test_rewarder_known_answers(case):
    testee = _build(case["rewarder"], None, er, FixedRewarder)
    for op in case["ops"]:
        states = np.array(op["states"])
        if op["op"] == "reset":
            testee.reset(states, np.array([]), np.array(op["mask"]) if "mask" in op else None)
        else:
            testing.assert_allclose(testee.reward(states, np.array([])), op["expected"])


@pytest.mark.parametrize("case", _cases("transformer"))
def test_transformer_known_answers(case):
    testee = _build(case["transformer"], case["num_envs"], st, None)
    states = np.array(case["states"])
    testing.assert_allclose(testee.transform(states, np.array(case["actions"])), case["expected"])
    assert np.array_equal(states, np.array(case["states"]))  # (a new array: the old states are left alone)


# ---- result dtypes --------------------------------------------------------------------------------------------------


def test_every_reward_term_has_its_dtype():
    states = np.array([[7.0, 7.1], [7.0, 9.0]], dtype=np.float32)
    observations = np.full((2, 4), 0.5, dtype=np.float32)
    terms = {er.DeltaRewarder(1, 0.5): np.float32, er.DistanceRewarder((0, 1), 2.0): np.float32,
             er.ObservationRewarder(1): np.float32, er.OnTargetRewarder((0, 1), 0.25): np.float64,
             er.StoppedRewarder(1, 0.125): np.float64}
    for term, dtype in terms.items():
        term.reset(states, observations)
        assert term.dtype == dtype
        assert term.reward(states, observations).dtype == dtype, type(term).__name__
    f32a, f32b, f64 = er.ObservationRewarder(0), er.DistanceRewarder((0, 1), 2.0), er.StoppedRewarder(1, 0.1)
    f64.reset(states, observations)
    for op, want in [(f32a + f32b, np.float32), (f32a * f32b, np.float32), (f32a + f64, np.float64),
                     (f64 * f32b, np.float64)]:
        assert op.dtype == want and op.reward(states, observations).dtype == want
    # integer on / off: numpy evaluates the term in int64
    assert er.OnTargetRewarder((0, 1), 0.25, 0, 2).dtype == np.int64


# ---- the twin against the two tasks' twins ----------------------------------------------------------------------------


@pytest.fixture()
def no_gpu(monkeypatch):
    monkeypatch.setattr(harness.render, "FastRenderer", FakeRenderer)
    monkeypatch.setattr(harness.state_observer, "FocusObserver", FakeFocusObserver)


def discrete_steps(n, max_steps=9, seed=None, **kw):
    """VectorDiscreteSteps (custom_environments.py:114-241) as a composition."""
    return dict(ender=ee.TimeLimitEnder(n, max_steps) | ee.DivergingEnder(n, (0, 1), RADIUS / 2, 3),
                initializer=si.RangedInitializer([[ENDS], [ENDS]], seed=seed),
                rewarder=er.DeltaRewarder(1, RADIUS * 2) + er.ObservationRewarder(1) + er.OnTargetRewarder((0, 1), RADIUS),
                transformer=st.DiscreteMoveTransformer(n, 1, ENDS, ACTION_SET), num_envs=n, **kw)


def continuous_jumps(n, max_steps=9, seed=None, **kw):
    """VectorContinuousJumps (custom_environments.py:244-339 with num_envs, TimeLimit | Diverging) as a composition."""
    return dict(ender=ee.TimeLimitEnder(n, max_steps) | ee.DivergingEnder(n, (0, 1), RADIUS / 2, 3),
                initializer=si.RangedInitializer([[ENDS], [ENDS]], seed=seed),
                rewarder=er.ObservationRewarder(1) + er.StoppedRewarder(1, harness.JUMP_STOP)
                * er.OnTargetRewarder((0, 1), RADIUS),
                transformer=st.ContinuousJumpTransformer(n, 1, ENDS, harness.JUMP_STOP), num_envs=n, **kw)


def _same(got, want):
    for x, y in zip(got[:4], want[:4]):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize("task", ["discrete", "continuous"])
def test_restating_compositions_equal_the_task_twins(task, no_gpu):
    n = 37
    if task == "discrete":
        twin = harness.VectorDiscreteSteps(max_episode_steps=9, num_envs=n, seed=5)
        composed = harness.VectorEnvironment(**discrete_steps(n, 9, seed=5))
    else:
        twin = harness.VectorContinuousJumps(max_episode_steps=9, num_envs=n, seed=5)
        composed = harness.VectorEnvironment(**continuous_jumps(n, 9, seed=5))
    assert np.array_equal(twin.reset()[0], composed.reset()[0])
    rng = np.random.default_rng(3)
    resets = 0
    for _ in range(60):
        actions = rng.integers(0, 13, n) if task == "discrete" else _actions(rng, twin._state)
        want = twin.step(actions)
        got = composed.step(actions)
        _same(got, want)
        assert got[1].dtype == np.float64
        assert np.array_equal(twin._state, composed._state)
        assert twin._initializer._generator.bit_generator.state == composed._initializer._generator.bit_generator.state
        for i in range(n):
            assert twin._ender.status(i) == composed.status(i)
        resets += int(want[3].sum())
    assert resets > n
    # reset(seed=...) reseeds the initializer as the twins' reset does
    assert np.array_equal(twin.reset(seed=8)[0], composed.reset(seed=8)[0])


def test_distance_rewarder_alone_is_returned_as_float64(no_gpu):
    n = 6
    env = harness.VectorEnvironment(ee.EndlessEnder(n), si.RangedInitializer([[ENDS], [ENDS]], seed=1),
                                    er.DistanceRewarder((0, 1), 5.0), st.DiscreteJumpTransformer(n, 1, ENDS, [5.0, 7.5]),
                                    n)
    env.reset()
    rewards = env.step(np.zeros(n, dtype=np.int64))[1]
    assert rewards.dtype == np.float64
    distance = np.abs(env._state[:, 0] - env._state[:, 1])
    assert np.array_equal(rewards, ((1 - distance / 5.0) * 1.0 + -1.0).astype(np.float64))


def test_host_twin_refuses_bad_actions(no_gpu):
    n = 4
    discrete = harness.VectorEnvironment(**discrete_steps(n, seed=1))
    jump = harness.VectorEnvironment(**continuous_jumps(n, seed=1))
    move = harness.VectorEnvironment(ee.EndlessEnder(n), si.RangedInitializer([[ENDS], [ENDS]], seed=1),
                                     er.ObservationRewarder(1), st.ContinuousMoveTransformer(n, 1, ENDS, 1.0), n)
    for env in (discrete, jump, move):
        env.reset()
    before = [env._state.copy() for env in (discrete, jump, move)]
    for bad in ([0, 1, 2, 13], [-1, 0, 0, 0], [0.0, 1.0, 2.0, 3.0], [0, 1, 2]):
        with pytest.raises(AssertionError):
            discrete.step(np.array(bad))
    for bad in (np.nan, np.inf, 1.5):
        with pytest.raises(AssertionError):
            jump.step(np.array([0, 0, 0, bad], dtype=np.float32))
    for bad in (np.nan, -np.inf):
        with pytest.raises(AssertionError):
            move.step(np.array([0, 0, 0, bad], dtype=np.float32))
    assert all(np.array_equal(b, env._state) for b, env in zip(before, (discrete, jump, move)))
    move.step(np.array([3.0, -7.0, 0.5, 0.0], dtype=np.float32))  # (finite values outside [-1, 1] are clipped)


# ---- initializer ----------------------------------------------------------------------------------------------------


def test_one_range_per_element_draws_what_the_task_initializer_draws():
    ours, theirs = si.RangedInitializer([[ENDS], [ENDS]], seed=4), harness._Initializer(ENDS, 4)
    for k in (5, 1, 17):
        assert np.array_equal(ours.propose(9), theirs.propose(9))
        assert np.array_equal(ours.initialize(k), theirs.initialize(k))


def test_several_ranges_per_element_are_seeded_and_keep_propose_then_consume():
    ranges = [[(0.0, 1.0), (10.0, 11.0)], [(5.0, 6.0)]]
    a, b = si.RangedInitializer(ranges, seed=2), si.RangedInitializer(ranges, seed=2)
    proposed = a.propose(50)
    assert np.array_equal(proposed, a.propose(50))  # (nothing consumed)
    assert np.array_equal(a.initialize(7), proposed[:7])  # the first k rows of any draw are a draw of k rows
    assert np.array_equal(a.initialize(50), b.initialize(57)[7:])
    rows = si.RangedInitializer(ranges, seed=3).initialize(400)
    first = rows[:, 0]
    assert rows.dtype == np.float32 and np.all((first < 1) | (first >= 10)) and np.any(first < 1) and np.any(first >= 10)
    assert np.all((rows[:, 1] >= 5) & (rows[:, 1] <= 6))


# ---- program compilation ------------------------------------------------------------------------------------------------


def test_postfix_order_of_nested_compositions():
    n = 3
    a, b, c = ee.TimeLimitEnder(n, 3), ee.DivergingEnder(n, (0, 1), 0.1), ee.EndlessEnder(n)
    leaves, ops = sp.ender_postfix((a | b) & c)
    assert leaves == [a, b, c] and ops == [0, 1, ee.OR, 2, ee.AND]
    leaves, ops = sp.ender_postfix(a | (b & c))
    assert leaves == [a, b, c] and ops == [0, 1, 2, ee.AND, ee.OR]
    x, y, z = er.ObservationRewarder(1), er.StoppedRewarder(1, 0.1), er.DistanceRewarder((0, 1), 1.0)
    leaves, ops = sp.rewarder_postfix((x + y) * z)
    assert leaves == [x, y, z] and ops == [0, 1, er.ADD, 2, er.MUL]
    program = sp.compile_program(st.ContinuousJumpTransformer(n, 1, ENDS), (a | b) & c, (x + y) * z, n)
    assert list(program.ender_ops[:5]) == [0, 1, -1, 2, -2] and program.n_enders == 3
    assert list(program.reward_ops[:5]) == [0, 1, -1, 2, -2]
    # float32, float64, their sum float64, float32, the product float64
    assert list(program.reward_f64[:5]) == [0, 1, 1, 0, 1]
    assert [program.rewarders[i].kind for i in range(3)] == [er.OBSERVATION, er.STOPPED, er.DISTANCE]


def _valid(n=4):
    return dict(transformer=st.DiscreteMoveTransformer(n, 1, ENDS, ACTION_SET),
                ender=ee.TimeLimitEnder(n, 5) | ee.StoppedEnder(n, 1, 0.1, 31),
                rewarder=er.ObservationRewarder(1) + er.OnTargetRewarder((0, 1), 0.25), num_envs=n)


@pytest.mark.parametrize("change,match", [
    (dict(num_envs=5), "num_envs"),
    (dict(transformer=st.ContinuousJumpTransformer(3, 1, ENDS)), "num_envs"),
    (dict(ender=ee.EndlessEnder(3) | ee.EndlessEnder(4)), "num_envs"),
    (dict(ender=ee.OnTargetEnder(4, (0, 2), 0.1)), "state index"),
    (dict(ender=ee.DivergingEnder(4, (-1, 1), 0.1)), "state index"),
    (dict(transformer=st.ContinuousMoveTransformer(4, 2, ENDS, 1.0)), "state index"),
    (dict(rewarder=er.DeltaRewarder(2, 0.5)), "state index"),
    (dict(rewarder=er.ObservationRewarder(4)), "observation index"),
    (dict(ender=ee.StoppedEnder(4, 1, 0.1, 32)), "outside"),
    (dict(ender=ee.OnTargetEnder(4, (0, 1), np.inf)), "not finite"),
    (dict(rewarder=er.DistanceRewarder((0, 1), np.nan)), "not finite"),
    (dict(transformer=st.ContinuousMoveTransformer(4, 1, ENDS, np.inf)), "not finite"),
    (dict(transformer=st.DiscreteJumpTransformer(4, 1, ENDS, np.arange(33.0))), "actions"),
    (dict(rewarder=er.OnTargetRewarder((0, 1), 0.25, 0, 2)), "not floating point"),
    (dict(rewarder=er.StoppedRewarder(1, 0.1, 2)), "not floating point"),
    (dict(ender=ee.EndlessEnder(4) | ee.EndlessEnder(4) | ee.EndlessEnder(4) | ee.EndlessEnder(4)
          | ee.EndlessEnder(4) | ee.EndlessEnder(4) | ee.EndlessEnder(4) | ee.EndlessEnder(4) | ee.EndlessEnder(4)),
     "at most 8"),
    (dict(rewarder=er.ObservationRewarder(0) + er.ObservationRewarder(0) + er.ObservationRewarder(0)
          + er.ObservationRewarder(0) + er.ObservationRewarder(0) + er.ObservationRewarder(0)
          + er.ObservationRewarder(0) + er.ObservationRewarder(0) + er.ObservationRewarder(0)), "at most 8"),
])
def test_compiler_refuses(change, match):
    sp.compile_program(**_valid())  # (the unchanged composition compiles)
    with pytest.raises(AssertionError, match=match):
        sp.compile_program(**{**_valid(), **change})


def test_compiler_refuses_a_leaf_used_twice():
    leaf = ee.EndlessEnder(4)
    with pytest.raises(AssertionError, match="once"):
        sp.compile_program(**{**_valid(), "ender": leaf | leaf})


def test_device_environment_refuses_sharding():
    with pytest.raises(ValueError, match="devices"):
        harness.DeviceVectorEnvironment(initializer=si.RangedInitializer([[ENDS], [ENDS]]), **_valid(), devices=[0, 1])
