"""The vector ContinuousJumps on the CPU: its host twin (harness.VectorContinuousJumps), the sharded form's host logic
and the registration factory.

* The twin's strategies reproduce the reference's own test numbers (tests/golden/continuous_strategy_cases.json,
  each case with its file:line in the reference's tests/environments/).
* The twin, with the focus measure replaced by a function of the state (no GPU), equals a plain restatement of
  VectorEnvironment.step (vector_environment.py:104-164) over these strategies (custom_environments.py:244-339 with
  num_envs in place of 1, TimeLimitEnder | DivergingEnder as :185-190) through many auto-resets.
* Actions that are NaN, infinite, outside [-1, 1] or of the wrong length are refused before any state changes.
* ShardedVectorContinuousJumps over numpy stand-ins of the shards' contexts hands every shard its slice of the float
  actions and the initializer's rows in global index order.
The device path runs against the twin in tests/test_gpu_continuous_env.py."""

import importlib
import json
import os

import numpy as np
import pytest
from numpy import testing

from reinfocus_amd.environments import harness
from reinfocus_amd.environments import spaces
from tests.test_sharded_env_logic import FakeContext

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "continuous_strategy_cases.json")))["cases"]
ENDS = (5.0, 10.0)


def _cases(component):
    return [pytest.param(c, id=c["name"]) for c in CASES if c["component"] == component]


def test_fixture_cites_the_reference():
    assert {c["component"] for c in CASES} == {"continuous_jump_transformer", "stopped_rewarder", "rewarder_times"}
    assert all(":" in c["source"] for c in CASES)


@pytest.mark.parametrize("case", _cases("continuous_jump_transformer"))
def test_jump_transformer(case):
    p = case["params"]
    testee = harness._JumpTransformer(p["move_index"], tuple(p["limits"]), p["stop_threshold"])
    states = np.array(case["states"])
    got = testee.transform(states, np.array(case["actions"]))
    testing.assert_allclose(got, case["expected"])
    assert np.array_equal(states, np.array(case["states"]))  # a new array: the old states are left alone


@pytest.mark.parametrize("case", _cases("stopped_rewarder"))
def test_stopped_rewarder(case):
    testee = harness._StoppedRewarder(**case["params"])
    for op in case["ops"]:
        states = np.array(op["states"])
        if op["op"] == "reset":
            indices = np.array(op["indices"]) if "indices" in op else None
            testee.reset(states, np.array([]), indices)
        else:
            testing.assert_allclose(testee.reward(states, np.array([])), op["expected"])


@pytest.mark.parametrize("case", _cases("rewarder_times"))
def test_rewarder_combines_stopped_times_on_target(case):
    """episode_rewarder_test.py:57-69 (`*` of two rewarders) on the twin's rewarder: with the focus value column at 0,
    the reward is the product of its stopped and on-target terms."""
    testee = harness._JumpRewarder(harness.JUMP_STOP, 0.25)
    testee._stopped.reward = lambda states, observations: np.array(case["left"], dtype=np.float64)
    testee._on_target = lambda states, observations: np.array(case["right"], dtype=np.float64)
    observations = np.zeros((2, 4), dtype=np.float32)
    testing.assert_allclose(testee.reward(np.zeros((2, 2), dtype=np.float32), observations), case["expected"])


def test_jump_rewarder_terms():
    """ObservationRewarder(1) + StoppedRewarder(1, 0.125) * OnTargetRewarder((0, 1), 0.25), float64."""
    testee = harness._JumpRewarder(harness.JUMP_STOP, 0.25)
    testee.reset(np.array([[7.0, 7.0], [7.0, 7.0], [7.0, 7.0], [7.0, 9.0]], dtype=np.float32), None)
    states = np.array([[7.0, 7.1], [7.0, 7.3], [6.0, 7.0], [7.0, 9.0]], dtype=np.float32)
    observations = np.array([[0, 0.5, 0, 0]] * 4, dtype=np.float32)
    rewards = testee.reward(states, observations)
    assert rewards.dtype == np.float64
    # stopped and on target | moved 0.3 | stopped, 1 away | stopped, 2 away
    assert list(rewards) == [1.5, 0.5, 0.5, 0.5]


class FakeRenderer:
    def __init__(self, **kwargs):
        self.closed = False

    def close(self):
        self.closed = True


class FakeFocusObserver:
    """FocusObserver with the render + focus measure replaced by a float64 function of (target, focus plane)."""

    def __init__(self, num_envs, target_index, focus_plane_index, ends, renderer, frame_height=300):
        self.single_observation_space = spaces.Box(0.0, 1000.0, dtype=np.float32)

    def observe(self, states, indices=None):
        states = np.asarray(states, dtype=np.float32)
        return (1000.0 / (1.0 + np.abs(states[:, 0] - states[:, 1]).astype(np.float64) ** 2)).reshape(-1, 1)

    def reset(self, states, indices=None):
        return self.observe(states, indices)


@pytest.fixture()
def no_gpu(monkeypatch):
    monkeypatch.setattr(harness.render, "FastRenderer", FakeRenderer)
    monkeypatch.setattr(harness.state_observer, "FocusObserver", FakeFocusObserver)


class Restated:
    """VectorEnvironment.step (vector_environment.py:104-164) over the vector ContinuousJumps' strategies, each
    restated in plain numpy from the reference's source: RangedInitializer (seedable), ContinuousJumpTransformer,
    TimeLimitEnder | DivergingEnder, NormalizedObserver(DeltaObserver([IndexedElementObserver, FocusObserver]...)),
    ObservationRewarder + StoppedRewarder * OnTargetRewarder."""

    def __init__(self, num_envs, max_steps, seed, focus):
        self.n = num_envs
        self.max_steps = max_steps
        self.initializer = harness._Initializer(ENDS, seed)
        self.focus = focus
        low = focus.single_observation_space.low[0]
        high = focus.single_observation_space.high[0]
        self.mid, self.scale = harness.normaliser_constants(ENDS, 5.0, low, high)
        self.state = None

    # RangedInitializer (state_initializer.py:30-71)
    def reset(self):
        self.state = self.initializer.initialize(self.n)
        self._ender_reset(self.state, np.full(self.n, True))
        self.old_wrapped = np.full((self.n, 2), np.nan, dtype=np.float32)
        observations = self._observer_reset(self.state, np.full(self.n, True))
        self.old_focus = self.state[:, 1]  # StoppedRewarder.reset without indices keeps the column
        return observations

    # TimeLimitEnder | DivergingEnder (episode_ender.py:137-170, :602-628; threshold 0.125, early_end_steps 3)
    def _ender_reset(self, states, indices):
        if indices.all():
            self.steps = np.zeros(self.n, dtype=np.int32)
            self.diverging = np.zeros(self.n, dtype=np.int32)
            self.last_diff = np.zeros(self.n, dtype=np.float32)
        self.steps[indices] = 0
        self.diverging[indices] = 0
        self.last_diff[indices] = abs(states[:, 0] - states[:, 1])

    def _ender_step(self, states):
        self.steps += 1
        diff = abs(states[:, 0] - states[:, 1])
        self.diverging[diff > self.last_diff + 0.125] += 1
        self.last_diff = diff

    def _truncated(self):
        return (self.steps >= self.max_steps) | (self.diverging >= 3)

    # NormalizedObserver(DeltaObserver([IndexedElementObserver(1), FocusObserver], True, [5.0, nan]))
    def _wrapped(self, states, indices):
        return np.hstack([states[:, 1].reshape(-1, 1), self.focus.observe(states, indices)], dtype=np.float32)

    def _normalize(self, observations):
        return np.clip((observations - self.mid) / self.scale, -1, 1, dtype=np.float32)

    def _observer_reset(self, states, indices):
        wrapped = self._wrapped(states, indices)
        self.old_wrapped[indices] = wrapped
        return self._normalize(np.hstack([wrapped, np.zeros(wrapped.shape, dtype=np.float32)], dtype=np.float32))

    def _observe(self, states):
        wrapped = self._wrapped(states, np.full(self.n, True))
        observations = np.hstack([wrapped, wrapped - self.old_wrapped], dtype=np.float32)
        self.old_wrapped = wrapped
        return self._normalize(observations)

    def step(self, actions):
        # ContinuousJumpTransformer(n, 1, (5.0, 10.0), 0.125) (state_transformer.py:95-118)
        new_states = self.state.copy()
        a = (np.asarray(actions, dtype=np.float32).flatten() + 1) / 2.0
        jumps = a * (ENDS[1] - ENDS[0]) + ENDS[0]
        moved = abs(new_states[:, 1] - jumps) > 0.125
        new_states[moved, 1] = jumps[moved]
        self.state = new_states
        self._ender_step(self.state)
        observations = self._observe(self.state)
        # ObservationRewarder(1) + StoppedRewarder(1, 0.125) * OnTargetRewarder((0, 1), 0.25)
        stopped = (abs(self.state[:, 1] - self.old_focus) < 0.125) * 1.0
        self.old_focus = self.state[:, 1]
        on_target = (abs(self.state[:, 0] - self.state[:, 1]) < 0.25) * 1.0 + 0.0
        rewards = observations[:, 1] + stopped * on_target
        terminated = np.full(self.n, False)
        truncated = self._truncated()
        done = terminated | truncated
        if done.any():
            new_state = self.initializer.initialize(done.sum())
            self.state[done] = new_state
            self._ender_reset(new_state, done)
            new_observations = self._observer_reset(new_state, done)
            observations[done] = new_observations
            self.old_focus[done] = new_state[:, 1]
        return observations, rewards, terminated, truncated


def _actions(rng, state):
    """A mix that exercises every branch: free jumps, the extremes, jumps shorter than the stop threshold, jumps onto
    the target."""
    n = len(state)
    free = rng.uniform(-1, 1, n).astype(np.float32)
    near = ((state[:, 1] + rng.uniform(-0.2, 0.2, n) - 5.0) / 5.0 * 2.0 - 1.0).astype(np.float32)
    onto = ((state[:, 0] + rng.uniform(-0.05, 0.05, n) - 5.0) / 5.0 * 2.0 - 1.0).astype(np.float32)
    pick = rng.integers(0, 5, n)
    actions = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [free, near, onto, np.float32(1.0)],
                        np.float32(-1.0))
    return np.clip(actions, -1, 1).astype(np.float32)


@pytest.mark.parametrize("n,max_steps,seed", [(1, 20, 0), (7, 5, 1), (64, 9, 2), (200, 20, 3)])
def test_twin_equals_restated_vector_environment(no_gpu, n, max_steps, seed):
    twin = harness.VectorContinuousJumps(max_steps, n, seed=seed)
    restated = Restated(n, max_steps, seed, FakeFocusObserver(n, 0, 1, ENDS, None))
    o_t, info = twin.reset()
    o_r = restated.reset()
    assert info == {} and o_t.dtype == np.float32 and np.array_equal(o_t, o_r)
    rng = np.random.default_rng(seed + 100)
    resets = stops = 0
    for step in range(60):
        actions = _actions(rng, twin._state)
        if step % 2:
            actions = actions.reshape(n, 1)  # (the batched action space's shape)
        before = twin._state.copy()
        got = twin.step(actions)
        want = restated.step(actions)
        assert got[1].dtype == np.float64 and want[1].dtype == np.float64
        for x, y in zip(got[:4], want):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert got[4] == {}
        assert np.array_equal(twin._state, restated.state)
        assert twin._initializer._generator.bit_generator.state == restated.initializer._generator.bit_generator.state
        resets += int(got[3].sum())
        stops += int(np.sum(~got[3] & (twin._state[:, 1] == before[:, 1])))
    assert resets > 0 and stops > 0
    assert np.all((twin._state >= 5) & (twin._state <= 10))


def test_twin_spaces_and_ender(no_gpu):
    env = harness.VectorContinuousJumps(max_episode_steps=7, num_envs=5)
    assert env.single_action_space.shape == (1,) and env.single_action_space.dtype == np.float32
    assert env.single_action_space.low[0] == -1 and env.single_action_space.high[0] == 1
    assert env.action_space.shape == (5, 1)
    assert env.observation_space.shape == (5, 4)
    # TimeLimitEnder(n, 7) | DivergingEnder(n, (0, 1), 0.125, early_end_steps=3), as the vector DiscreteSteps'
    assert (env._ender._max_steps, env._ender._threshold, env._ender._early_end_steps) == (7, 0.125, 3)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1.0001, -1.5, 3.0])
def test_twin_refuses_bad_actions_without_changing_state(no_gpu, bad):
    env = harness.VectorContinuousJumps(max_episode_steps=4, num_envs=6, seed=5)
    env.reset()
    env.step(np.zeros(6, dtype=np.float32))
    state, steps = env._state.copy(), env._ender._steps.copy()
    old_wrapped, old_focus = env._observer._old.copy(), env._rewarder._stopped._old_states.copy()
    generator = env._initializer._generator.bit_generator.state
    actions = np.full(6, 0.5, dtype=np.float32)
    actions[3] = bad
    with pytest.raises(AssertionError):
        env.step(actions)
    for wrong in (np.zeros(5, dtype=np.float32), np.zeros((6, 2), dtype=np.float32), np.float32(0.0)):
        with pytest.raises(AssertionError):
            env.step(wrong)
    assert np.array_equal(env._state, state) and np.array_equal(env._ender._steps, steps)
    assert np.array_equal(env._observer._old, old_wrapped, equal_nan=True)
    assert np.array_equal(env._rewarder._stopped._old_states, old_focus)
    assert env._initializer._generator.bit_generator.state == generator
    env.step(np.array([-1, 1, 0, -1, 1, 0], dtype=np.float64))  # the extremes are actions; float64 is cast to float32


def test_jump_actions():
    assert harness.jump_actions([0.5, -1.0], 2).dtype == np.float32
    assert harness.jump_actions(np.ones((3, 1)), 3).shape == (3,)
    with pytest.raises(AssertionError):
        harness.jump_actions(np.ones((1, 3)), 3)


class FakeJumpContext(FakeContext):
    """FakeContext with the float-action calls of a context configured for ContinuousJumps; the int32 ones refuse,
    as the library does."""

    def __init__(self, n, first_env):
        super().__init__(n, first_env)
        self.seen = []

    def _record(self, actions):
        assert actions.dtype == np.float32 and actions.shape == (self.n,)
        self.seen.append(actions.copy())

    def env_step_plan_jumps(self, actions):
        self._record(actions)
        return FakeContext.env_step_begin(self, actions)[2]

    def env_step_begin_jumps(self, actions):
        self._record(actions)
        return FakeContext.env_step_begin(self, actions)

    def env_step_plan(self, actions):
        raise AssertionError("int32 actions on a ContinuousJumps context")

    def env_step_begin(self, actions):
        raise AssertionError("int32 actions on a ContinuousJumps context")


@pytest.fixture()
def fake_jump_shards(monkeypatch):
    from reinfocus_amd import _native

    made = []

    class FakeShard:
        ENDS, TARGET_RADIUS = harness._DeviceShard.ENDS, 0.25

        def __init__(self, num_envs, max_episode_steps, frame_height, samples_per_pixel, device, first_state_index,
                     jumps=False):
            assert jumps, "a ContinuousJumps shard is configured for its task"
            self.first_env = first_state_index // (frame_height * frame_height)
            self.num_envs, self.device = num_envs, device
            self.ctx = FakeJumpContext(num_envs, self.first_env)
            made.append(self)

    monkeypatch.setattr(harness, "_DeviceShard", FakeShard)
    monkeypatch.setattr(_native, "device_count", lambda: 4)
    monkeypatch.setattr(_native, "device_info", lambda d: {"device": d, "pci_bus_id": f"0000:{d:02x}:00.0",
                                                           "numa_node": -1})
    monkeypatch.setattr(_native, "pin_to_numa_node", lambda node, whole_process=False, sysfs=None: None)
    return made


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("n,devices", [(11, [0, 1, 2]), (8, [0, 1, 2, 3])])
def test_sharded_jumps_hand_out_float_actions_and_rows_in_global_order(fake_jump_shards, n, devices, exact):
    kw = dict(num_envs=n, frame_height=16, samples_per_pixel=1, seed=4, exact=exact)
    many = harness.ShardedVectorContinuousJumps(devices=devices, **kw)
    mine = sorted(fake_jump_shards, key=lambda s: s.first_env)
    one = harness.ShardedVectorContinuousJumps(devices=[0], **kw)
    assert many.single_action_space.shape == (1,) and many.action_space.shape == (n, 1)
    assert np.array_equal(one.reset()[0], many.reset()[0])
    rng = np.random.default_rng(0)
    total = 0
    for step in range(12):
        actions = rng.uniform(-1, 1, (n, 1) if step % 2 else n).astype(np.float32)
        a, b = one.step(actions), many.step(actions)
        for x, y in zip(a[:4], b[:4]):
            assert x.shape == y.shape and np.array_equal(x, y)
        assert np.array_equal(one._state, many._state)
        flat = actions.reshape(n)
        for shard in mine:
            assert np.array_equal(shard.ctx.seen[-1], flat[shard.first_env:shard.first_env + shard.num_envs])
        total += int(b[3].sum())
    assert total > n
    assert one._initializer._generator.bit_generator.state == many._initializer._generator.bit_generator.state
    # one bad action anywhere: refused before any shard begins its step
    bad = np.zeros(n, dtype=np.float32)
    bad[-1] = np.nan
    with pytest.raises(AssertionError):
        many.step(bad)
    assert all(len(shard.ctx.seen) == 12 and shard.ctx.pending is None for shard in mine)
    many.close()
    one.close()


def test_vector_continuous_jumps_factory(fake_jump_shards, monkeypatch):
    from reinfocus_amd import registration

    built = []
    for name in ("VectorContinuousJumps", "DeviceVectorContinuousJumps"):
        monkeypatch.setattr(harness, name, lambda *args, _name=name, **kwargs: built.append((_name, args, kwargs)))
    registration.vector_continuous_jumps(num_envs=3, seed=2)
    registration.vector_continuous_jumps(7, 3, "rgb_array", glue="host", frame_height=16)
    assert built == [("DeviceVectorContinuousJumps", (20, 3, None), {"seed": 2}),
                     ("VectorContinuousJumps", (7, 3, "rgb_array"), {"frame_height": 16})]
    env = registration.vector_continuous_jumps(num_envs=6, devices=[0, 1], frame_height=8, samples_per_pixel=1)
    assert type(env) is harness.ShardedVectorContinuousJumps and env.num_envs == 6 and env.devices == [0, 1]
    env.close()
    with pytest.raises(AssertionError):
        registration.vector_continuous_jumps(num_envs=2, glue="host", devices=[0])
    with pytest.raises(AssertionError):
        registration.vector_continuous_jumps(num_envs=2, glue="numpy")
    # usable as a gymnasium vector_entry_point string ("module:attribute")
    module, _, attribute = "reinfocus_amd.registration:vector_continuous_jumps".partition(":")
    assert getattr(importlib.import_module(module), attribute) is registration.vector_continuous_jumps


def test_registrations_still_mirror_the_reference():
    from reinfocus_amd import registration

    assert set(registration.ENTRY_POINTS) == {"DiscreteSteps-v0", "ContinuousJumps-v0"}
    assert "vector_entry_point" not in registration.ENTRY_POINTS["ContinuousJumps-v0"]
    assert registration.ENTRY_POINTS["DiscreteSteps-v0"]["vector_entry_point"] == (
        "reinfocus_amd.registration:vector_discrete_steps")
    with pytest.raises(KeyError):
        registration.make_vec("ContinuousJumps-v0", 2)
