"""CPU tests of episode records (episode_records=True): the numpy twins -- the oracle the device is held to in
tests/test_gpu_episode_records.py -- against an independent restatement of the step and against their own outputs, the
seeds of the GPU tests, the stable-baselines3 shim with and without records, and what is refused.  The GPU's render and
focus measure are replaced by a function of the state (tests/test_composed_env_logic.py::no_gpu); which environments
end depends on their states alone."""

import numpy as np
import pytest

from reinfocus_amd.environments import harness, snapshot, spaces, vector_shim
from tests import test_gpu_snapshot as gpu
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture
from tests.test_gpu_device_initializer import KW, _objects

STEPS = 12
KEYS = ("final_observation", "episode_return", "episode_length")


def same_bits(a, b):
    """Equal dtype, shape and values, NaN equal to NaN."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _compositions(n):
    return {"limit": lambda: _objects(n, "multi", gpu.SEED), "stopped + delta": lambda: gpu.stopped_objects(n)}


# ---- 1: the twin against an independent restatement -------------------------------------------------------------------
@pytest.mark.parametrize("composition", ["limit", "stopped + delta"])
@pytest.mark.parametrize("n", [1, 65])
def test_twin_equals_a_restatement_of_the_step(n, composition, no_gpu):  # noqa: F811
    """A loop written here calls a second, equal set of strategy objects in the order of vector_environment.py:124-148,
    keeps the observations from before the overwrite and sums the rewards in float64: all three arrays equal the
    twin's bit for bit after every one of 12 steps."""
    make = _compositions(n)[composition]
    twin = harness.VectorEnvironment(**make(), episode_records=True, **KW)
    other = harness.VectorEnvironment(**make(), **KW)  # (only its observer is used below: it holds the fake renderer)
    parts = make()
    ender, initializer, rewarder, transformer = (parts[k] for k in ("ender", "initializer", "rewarder", "transformer"))
    observer = other._observer

    first, info = twin.reset()
    assert info == {}
    state = initializer.initialize(n)
    ender.reset(state)
    observations = observer.reset(state, None)
    rewarder.reset(state, observations)
    assert np.array_equal(first, observations)
    returns, lengths = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int32)

    seen = 0
    for action in gpu.index_actions(n, steps=STEPS):
        got = twin.step(action)
        state = transformer.transform(state, action)
        ender.step(state)
        observations = observer.observe(state)
        rewards = np.asarray(rewarder.reward(state, observations), dtype=np.float64)
        done = ender.is_terminated() | ender.is_truncated()
        want = {"final_observation": np.full((n, 4), np.nan, dtype=np.float32),
                "episode_return": np.full(n, np.nan, dtype=np.float64), "episode_length": np.zeros(n, dtype=np.int32)}
        for e in range(n):
            returns[e] = returns[e] + rewards[e]
            lengths[e] += 1
            if done[e]:
                want["final_observation"][e] = observations[e]  # (before the overwrite below)
                want["episode_return"][e], want["episode_length"][e] = returns[e], lengths[e]
                returns[e], lengths[e] = 0.0, 0
        if done.any():
            new_state = initializer.initialize(done.sum())
            state[done] = new_state
            ender.reset(new_state, done)
            new_observations = observer.reset(new_state, done)
            observations[done] = new_observations
            rewarder.reset(new_state, new_observations, done)
        assert np.array_equal(got[0], observations) and np.array_equal(got[1], rewards) and np.array_equal(got[3], done)
        assert sorted(got[4]) == sorted(KEYS)
        for key in KEYS:
            assert same_bits(got[4][key], want[key]), key
        assert all(same_bits(x, y) for x, y in zip(twin.episode_accumulators(), (returns, lengths)))
        seen += int(done.sum())
    assert seen > 0


# ---- 2: outputs alone -----------------------------------------------------------------------------------------------
def _twin_classes(n):
    kw = dict(num_envs=n, episode_records=True, **gpu.TASK_KW)
    rng = np.random.default_rng(gpu.ACTION_SEED)
    from tests.test_continuous_vector_logic import _actions

    return {"VectorDiscreteSteps": (lambda: harness.VectorDiscreteSteps(**kw), lambda state: rng.integers(0, 13, n)),
            "VectorContinuousJumps": (lambda: harness.VectorContinuousJumps(**kw), lambda state: _actions(rng, state)),
            "VectorEnvironment": (lambda: harness.VectorEnvironment(**gpu.stopped_objects(n), episode_records=True, **KW),
                                  lambda state: rng.integers(0, 13, n))}


@pytest.mark.parametrize("name", ["VectorDiscreteSteps", "VectorContinuousJumps", "VectorEnvironment"])
def test_records_follow_from_the_steps_own_outputs(name, no_gpu):  # noqa: F811
    """episode_return at an ending is the left-to-right float64 sum of the rewards step() returned for that environment
    since its previous ending or the reset, episode_length their count; the other rows are NaN / NaN / 0."""
    n = 65
    make, action = _twin_classes(n)[name]
    env = make()
    _, info = env.reset()
    assert info == {}
    since = [[] for _ in range(n)]
    endings = 0
    for _ in range(2 * STEPS):
        _, rewards, terminated, truncated, info = env.step(action(env._state))
        assert rewards.dtype == np.float64 and not terminated.any()
        final, returns, lengths = (info[key] for key in KEYS)
        assert final.dtype == np.float32 and final.shape == (n, 4) and returns.dtype == np.float64
        assert lengths.dtype == np.int32
        for e in range(n):
            since[e].append(rewards[e])
            if truncated[e]:
                total = np.float64(0.0)
                for r in since[e]:
                    total = total + r
                assert returns[e] == total and lengths[e] == len(since[e]) and not np.isnan(final[e]).any()
                since[e] = []
                endings += 1
            else:
                assert np.isnan(returns[e]) and lengths[e] == 0 and np.isnan(final[e]).all()
    assert endings > n  # (environments ended more than once)
    # a full reset zeroes the accumulators
    env.reset()
    returns, lengths = env.episode_accumulators()
    assert not returns.any() and not lengths.any() and returns.dtype == np.float64 and lengths.dtype == np.int32


def test_records_are_fresh_arrays_and_off_by_default(no_gpu):  # noqa: F811
    n = 5
    env = harness.VectorEnvironment(**_objects(n, "multi", gpu.SEED), episode_records=True, **KW)
    env.reset()
    a = env.step(np.zeros(n, dtype=np.int64))[4]
    b = env.step(np.zeros(n, dtype=np.int64))[4]
    assert all(a[key] is not b[key] and not np.shares_memory(a[key], b[key]) for key in KEYS)
    plain = harness.VectorEnvironment(**_objects(n, "multi", gpu.SEED), **KW)
    plain.reset()
    assert plain.step(np.zeros(n, dtype=np.int64))[4] == {}
    with pytest.raises(ValueError, match="episode_records"):
        plain.episode_accumulators()


# ---- 3: the seeds of the GPU tests -------------------------------------------------------------------------------------
def _ended_per_step(host, actions):
    ended = []
    for action in actions:
        action = action(host._state) if callable(action) else action
        ended.append(host.step(action)[3].copy())
    return ended


@pytest.mark.parametrize("n", [65, 1100])
def test_seeds_of_the_gpu_tests_give_partial_resets(n, no_gpu):  # noqa: F811
    """tests/test_gpu_episode_records.py, every schedule: some step ends 0 < k < n environments and some environment ends
    twice within the 12 steps."""
    host = harness.VectorEnvironment(**_objects(n, "multi", gpu.SEED), episode_records=True, **KW)
    host.reset()
    ended = _ended_per_step(host, gpu.index_actions(n, steps=STEPS))
    assert any(0 < int(flags.sum()) < n for flags in ended), [int(f.sum()) for f in ended]
    assert (np.sum(ended, axis=0) >= 2).any()


@pytest.mark.parametrize("kind", gpu.KINDS)
def test_seeds_of_every_kind_of_context(kind, no_gpu):  # noqa: F811
    from tests.test_snapshot_logic import _host_only

    n = 65
    if kind == "two delta observers":  # (the tree needs a real FocusObserver; which environments end does not)
        host = harness.VectorEnvironment(**gpu.observed_strategies(n, 4), **KW)
        make_actions = lambda rng: (lambda state: rng.integers(0, 13, n))  # noqa: E731
    else:
        host, _, _, make_actions = _host_only(kind, n)
    host.reset()
    ended = _ended_per_step(host, [make_actions(np.random.default_rng(gpu.ACTION_SEED))] * STEPS)
    assert any(0 < int(flags.sum()) < n for flags in ended) and (np.sum(ended, axis=0) >= 2).any()


def test_seeds_of_the_snapshot_tests_leave_an_episode_open(no_gpu):  # noqa: F811
    """The rewind and resume tests snapshot after HALF steps: some environment is mid-episode there, and the steps
    after it end a part of the environments."""
    n = 65
    host = harness.VectorEnvironment(**_objects(n, "multi", gpu.SEED), episode_records=True, **KW)
    host.reset()
    actions = gpu.index_actions(n)
    _ended_per_step(host, actions[:gpu.HALF])
    assert host.episode_accumulators()[1].any()
    after = _ended_per_step(host, actions[gpu.HALF:])
    assert any(0 < int(flags.sum()) < n for flags in after)


# ---- 4: the stable-baselines3 shim -------------------------------------------------------------------------------------
class _Scripted(harness.VectorDiscreteSteps):
    """A VectorDiscreteSteps that never touches the GPU: canned step results, with or without records."""

    def __init__(self, num_envs, records):  # pylint: disable=super-init-not-called
        self.num_envs = num_envs
        self.single_observation_space = spaces.Box(-np.ones(4, dtype=np.float32), np.ones(4, dtype=np.float32),
                                                   dtype=np.float32)
        self.single_action_space = spaces.Discrete(13)
        self.render_mode = None
        self.records = records

    def step(self, actions):
        n = self.num_envs
        obs = np.arange(n * 4, dtype=np.float32).reshape(n, 4)
        terminated, truncated = np.array([False, False, True][:n]), np.array([False, True, False][:n])
        info = {"steps": np.arange(n), "label": "not an array"}
        if self.records:
            done = terminated | truncated
            info["final_observation"] = np.where(done[:, None], obs + 100, np.nan).astype(np.float32)
            info["episode_return"] = np.where(done, np.array([1.5, 2.5, 3.5])[:n], np.nan)
            info["episode_length"] = np.where(done, np.array([4, 5, 6])[:n], 0).astype(np.int32)
        return obs, np.linspace(-1, 1, n), terminated, truncated, info


def test_shim_reports_the_final_observation_and_the_episode_with_records():
    testee = vector_shim.SB3Wrapper(_Scripted(3, True), None)
    testee.step_async(np.array([1, 2, 3]))
    obs, _, dones, infos = testee.step_wait()
    assert list(dones) == [False, True, True]
    assert [sorted(i) for i in infos] == [["steps"], ["episode", "steps", "terminal_observation"],
                                          ["episode", "steps", "terminal_observation"]]
    for i in (1, 2):
        assert np.array_equal(infos[i]["terminal_observation"], obs[i] + 100)  # (not the next episode's first row)
        assert infos[i]["episode"] == {"r": [1.5, 2.5, 3.5][i], "l": [4, 5, 6][i]}
        assert type(infos[i]["episode"]["r"]) is float and type(infos[i]["episode"]["l"]) is int
    assert "terminal_observation" in vector_shim.SB3Wrapper.step_wait.__doc__


def test_shim_is_unchanged_without_records():
    testee = vector_shim.SB3Wrapper(_Scripted(3, False), None)
    testee.step_async(np.array([1, 2, 3]))
    obs, _, _, infos = testee.step_wait()
    assert [sorted(i) for i in infos] == [["steps"], ["steps", "terminal_observation"], ["steps", "terminal_observation"]]
    assert [i["steps"] for i in infos] == [0, 1, 2]
    assert np.array_equal(infos[2]["terminal_observation"], obs[2])


# ---- 5: refusals ---------------------------------------------------------------------------------------------------------
def test_sharded_and_single_environments_refuse_records():
    """Before anything touches a GPU."""
    for cls in (harness.ShardedVectorDiscreteSteps, harness.ShardedVectorContinuousJumps):
        with pytest.raises(ValueError, match="sharded"):
            cls(num_envs=4, devices=[0, 0], frame_height=8, samples_per_pixel=1, episode_records=True)
    with pytest.raises(ValueError, match="sharded"):
        harness.DeviceVectorEnvironment(**_objects(4, "multi", 1), devices=[0, 0], episode_records=True, **KW)
    for cls in (harness.DiscreteSteps, harness.ContinuousJumps):
        with pytest.raises(ValueError, match="single-environment"):
            cls(frame_height=8, samples_per_pixel=1, episode_records=True)


class _NoContext:
    def env_restore(self, blob):
        raise AssertionError("the library was called")


@pytest.mark.parametrize("mine,theirs", [(True, False), (False, True)])
def test_restore_across_differing_records_is_refused_before_the_library(mine, theirs):
    env = object.__new__(harness.DeviceVectorDiscreteSteps)
    env.render_mode, env.num_envs, env._device_initializer, env._episode_records = None, 65, True, mine
    env._shard = type("Shard", (), {"frame_height": 16, "samples_per_pixel": 2})()
    env._ctx = _NoContext()
    other = snapshot.EnvSnapshot(np.zeros(512, dtype=np.uint8), "DeviceVectorDiscreteSteps", 65, 16, 2, None, theirs)
    assert f"episode_records={theirs}" in other.describe()
    with pytest.raises(ValueError, match="episode_records"):
        env.restore(other)


def test_a_snapshot_file_keeps_the_flag_and_an_old_file_has_none(tmp_path):
    import json

    blob = np.arange(300, dtype=np.uint8)
    for flag in (True, False):
        path = tmp_path / f"{flag}.npz"
        snapshot.EnvSnapshot(blob, "DeviceVectorEnvironment", 65, 16, 2, None, flag).save(path)
        back = snapshot.EnvSnapshot.load(path)
        assert back.episode_records is flag and np.array_equal(back.blob, blob)
        with np.load(path) as data:
            assert ("episode_records" in json.loads(str(data["meta"]))) == flag  # (off: the file of before the flag)
