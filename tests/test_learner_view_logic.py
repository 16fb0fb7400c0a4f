"""CPU tests of the learner view (learner_view=harness.LearnerView(...): VecNormalize followed by VecFrameStack): the
numpy twin harness._LearnerView -- the oracle the device is held to in tests/test_gpu_learner_view.py -- against a literal
second restatement of the definition (include/reinfocus_hip.h, "learner view") written here with per-environment Python
loops and a recursive treesum; treesum itself; the three host twins with the keyword; what is refused; and that the
seeds of the GPU tests end a part of the environments and some environment twice.  The GPU's render and focus measure are
replaced by a function of the state (tests/test_composed_env_logic.py::no_gpu)."""

import numpy as np
import pytest

from reinfocus_amd import registration
from reinfocus_amd.environments import harness
from tests import test_gpu_snapshot as gpu
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture
from tests.test_gpu_device_initializer import KW, _objects

STEPS = 12
F64 = np.float64


def bits(a):
    a = np.asarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def same_bits(a, b):
    """Equal dtype, shape and bytes: zero signs and NaNs count."""
    return bits(a) == bits(b)


# ---- the restatement ----------------------------------------------------------------------------------------------------
def recursive_treesum(x):
    values = [F64(v) for v in x]
    size = 1
    while size < len(values):
        size *= 2
    values += [F64(0.0)] * (size - len(values))

    def tree(lo, hi):
        if hi - lo == 1:
            return values[lo]
        mid = (lo + hi) // 2
        return tree(lo, mid) + tree(mid, hi)

    return tree(0, size) + F64(0.0)


class Restated:
    """The definition, literally: scalars of numpy.float64 / numpy.float32, one environment and one column at a time."""

    def __init__(self, n, width, k, norm_obs=True, norm_reward=True, gamma=0.99, epsilon=1e-8, clip_obs=10.0,
                 clip_reward=10.0, training=True):
        self.n, self.W, self.k, self.V = n, width, k, k * width
        self.norm_obs, self.norm_reward, self.training = norm_obs, norm_reward, training
        self.gamma, self.epsilon, self.clip_obs, self.clip_reward = F64(gamma), F64(epsilon), F64(clip_obs), F64(clip_reward)
        self.stack = [[np.float32(0.0)] * self.V for _ in range(n)]
        self.returns = [F64(0.0)] * n
        self.mean, self.var, self.count = [F64(0.0)] * (width + 1), [F64(1.0)] * (width + 1), [F64(1e-4)] * (width + 1)

    def update(self, slot, x):
        N = F64(self.n)
        bm = recursive_treesum(x) / N
        bv = recursive_treesum([(F64(v) - bm) * (F64(v) - bm) for v in x]) / N
        delta = bm - self.mean[slot]
        tot = self.count[slot] + N
        mean = self.mean[slot] + (delta * N) / tot
        m2 = (self.var[slot] * self.count[slot] + bv * N) + (((delta * delta) * self.count[slot]) * N) / tot
        self.mean[slot], self.var[slot], self.count[slot] = mean, m2 / tot, tot

    def normalise(self, row):
        if not self.norm_obs:
            return [np.float32(v) for v in row]
        out = []
        for c in range(self.W):
            z = (F64(row[c]) - self.mean[c]) / np.sqrt(self.var[c] + self.epsilon)
            z = -self.clip_obs if z < -self.clip_obs else (self.clip_obs if z > self.clip_obs else z)
            out.append(np.float32(z))
        return out

    def reset(self, obs):
        self.returns = [F64(0.0)] * self.n
        if self.training and self.norm_obs:
            for c in range(self.W):
                self.update(c, [obs[e][c] for e in range(self.n)])
        for e in range(self.n):
            self.stack[e] = [np.float32(0.0)] * (self.V - self.W) + self.normalise(obs[e])
        return np.array(self.stack, dtype=np.float32).reshape(self.n, self.V)

    def step(self, obs, reward, done, final_obs=None):
        n, W, V = self.n, self.W, self.V
        if self.training and self.norm_obs:                                                   # 1
            for c in range(W):
                self.update(c, [obs[e][c] for e in range(n)])
        newest = [self.normalise(obs[e]) for e in range(n)]                                   # 2
        if self.training:                                                                     # 3
            self.returns = [self.returns[e] * self.gamma + F64(reward[e]) for e in range(n)]
            self.update(W, self.returns)
        view_reward = []                                                                      # 4
        for e in range(n):
            r = F64(reward[e])
            if self.norm_reward:
                r = r / np.sqrt(self.var[W] + self.epsilon)
                r = -self.clip_reward if r < -self.clip_reward else (self.clip_reward if r > self.clip_reward else r)
            view_reward.append(r)
        view_final = None if final_obs is None else np.full((n, V), np.nan, dtype=np.float32)
        for e in range(n):
            self.stack[e] = self.stack[e][W:] + self.stack[e][V - W:]                         # 5 (the last W: rewritten in 8)
            if done[e]:
                if final_obs is not None:                                                     # 6
                    view_final[e] = self.stack[e][:V - W] + self.normalise(final_obs[e])
                self.stack[e] = [np.float32(0.0)] * V                                         # 7
                self.returns[e] = F64(0.0)
            self.stack[e] = self.stack[e][:V - W] + newest[e]                                 # 8
        return (np.array(self.stack, dtype=np.float32).reshape(n, V), np.array(view_reward, dtype=np.float64), view_final)


def _script(n, width, seed):
    """Random raw results of a reset and twelve steps: environments 0 mod 3 never end, 1 mod 3 end once, 2 mod 3 end
    twice (n == 1: the one environment ends twice)."""
    rng = np.random.default_rng(seed)
    reset_obs = rng.uniform(-1, 1, (n, width)).astype(np.float32)
    steps = []
    for t in range(STEPS):
        obs = (rng.standard_normal((n, width)) * rng.choice([0.01, 1.0, 30.0])).astype(np.float32)
        obs[rng.random((n, width)) < 0.05] = -0.0
        reward = rng.standard_normal(n) * 3.0
        kind = np.arange(n) % 3 if n > 1 else np.array([2])
        done = ((kind == 1) & (t == 4)) | ((kind == 2) & ((t == 3) | (t == 8)))
        final = np.where(done[:, None], rng.standard_normal((n, width)), np.nan).astype(np.float32)
        steps.append((obs, reward, done, final))
    return reset_obs, steps


# ---- 1: the twin against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, 8])
@pytest.mark.parametrize("width", [4, 16])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1100])
def test_twin_equals_the_restatement(n, width, k):
    config = harness.LearnerView(frame_stack=k)
    twin, want = harness._LearnerView(config, n, width), Restated(n, width, k)
    reset_obs, steps = _script(n, width, 100 * n + 10 * width + k)
    assert same_bits(twin.reset(reset_obs), want.reset(reset_obs))
    ended = np.zeros(n, dtype=int)
    for t, (obs, reward, done, final) in enumerate(steps):
        if t == 6:  # a reset in between: the stack and the returns start over, the moments go on
            before = twin.statistics()
            assert same_bits(twin.reset(reset_obs), want.reset(reset_obs))
            after = twin.statistics()
            assert (after["count"][:width] == before["count"][:width] + n).all()  # (updated, never reset)
            assert all(same_bits(after[key][width], before[key][width]) for key in after)  # (the returns': untouched)
            assert not twin.returns.any() and not twin.stack[:, :(k - 1) * width].any()
        got_step, want_step = twin.step(obs, reward, done, final), want.step(obs, reward, done, final)
        for name, a, b in zip(("observation", "reward", "view_final"), got_step, want_step):
            assert same_bits(a, b), (t, name)
        view_obs, view_reward, view_final = got_step
        assert view_obs.dtype == np.float32 and view_obs.shape == (n, k * width) and view_reward.dtype == np.float64
        assert same_bits(twin.stack, np.array(want.stack, dtype=np.float32).reshape(n, k * width))
        assert same_bits(twin.returns, np.array(want.returns))
        for key, values in twin.statistics().items():
            assert same_bits(values, np.array(getattr(want, key))), (t, key)
        # an environment that ended: only the newest frame is left, its returns are zero, and view_final is the k - 1
        # older frames (what the stack held, moved left) and the normalised final row
        assert not view_obs[done, :(k - 1) * width].any() and not twin.returns[done].any()
        assert np.isnan(view_final[~done]).all() and not np.isnan(view_final[done]).any()
        assert same_bits(view_final[done, (k - 1) * width:], twin._normalise(final[done]))
        assert np.abs(view_obs).max() <= 10.0 and np.abs(view_reward).max() <= 10.0
        ended += done
    assert set(ended) == ({0, 1, 2} if n >= 3 else {2} if n == 1 else {0, 1})


@pytest.mark.parametrize("norm_obs,norm_reward", [(False, True), (True, False), (False, False)])
def test_either_normalisation_off(norm_obs, norm_reward):
    n, width, k = 65, 4, 5
    kw = dict(norm_obs=norm_obs, norm_reward=norm_reward, gamma=0.9, epsilon=1e-6, clip_obs=1.5, clip_reward=0.75)
    twin = harness._LearnerView(harness.LearnerView(frame_stack=k, **kw), n, width)
    want = Restated(n, width, k, **kw)
    reset_obs, steps = _script(n, width, 5)
    assert same_bits(twin.reset(reset_obs), want.reset(reset_obs))
    for obs, reward, done, final in steps:
        got_step, want_step = twin.step(obs, reward, done, final), want.step(obs, reward, done, final)
        assert all(same_bits(a, b) for a, b in zip(got_step, want_step))
        if not norm_obs:
            assert same_bits(got_step[0][:, -width:], obs)
            assert same_bits(twin.statistics()["count"][:width], np.full(width, 1e-4))
        if not norm_reward:
            assert same_bits(got_step[1], reward)
        else:
            assert np.abs(got_step[1]).max() <= 0.75


def test_training_off_freezes_the_moments_and_the_returns():
    n, width, k = 65, 4, 2
    twin, want = harness._LearnerView(harness.LearnerView(frame_stack=k), n, width), Restated(n, width, k)
    reset_obs, steps = _script(n, width, 9)
    twin.reset(reset_obs), want.reset(reset_obs)
    for t, (obs, reward, done, final) in enumerate(steps):
        if t == 6:
            twin.training = want.training = False
            frozen, returns = twin.statistics(), twin.returns.copy()
        got_step, want_step = twin.step(obs, reward, done, final), want.step(obs, reward, done, final)
        assert all(same_bits(a, b) for a, b in zip(got_step, want_step))
        if t >= 6:
            assert all(same_bits(twin.statistics()[key], frozen[key]) for key in frozen)
            returns[done] = 0.0  # (an ending still zeroes them)
            assert same_bits(twin.returns, returns)
    twin.reset(reset_obs)
    assert all(same_bits(twin.statistics()[key], frozen[key]) for key in frozen)


# ---- 2: treesum ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1024, 1025, 1100, 2500])
def test_treesum_is_the_recursive_tree_and_ignores_zero_padding(n):
    rng = np.random.default_rng(n)
    differs = 0
    for trial in range(4):
        x = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
        if trial == 3:
            x = -np.abs(x) * 0.0  # (all -0.0)
        got = harness.treesum(x)
        assert type(got) is np.float64 and same_bits(got, recursive_treesum(x))
        for extra in (1, n, 4096):
            assert same_bits(got, harness.treesum(np.concatenate([x, np.zeros(extra)])))
        sequential = F64(0.0)
        for v in x:
            sequential = sequential + v
        differs += not same_bits(got, sequential)
    assert n < 64 or differs  # (the order is a real part of the contract)
    assert same_bits(harness.treesum(x.astype(np.float32)), recursive_treesum(x.astype(np.float32)))


def test_treesum_of_minus_zero_is_plus_zero():
    assert same_bits(harness.treesum([-0.0]), F64(0.0)) and not np.signbit(harness.treesum([-0.0, -0.0, -0.0]))


# ---- 3: the twins with the keyword -----------------------------------------------------------------------------------------
def _twin_classes(n, **extra):
    from tests.test_continuous_vector_logic import _actions

    kw = dict(num_envs=n, **gpu.TASK_KW)
    return {"VectorDiscreteSteps": (lambda **o: harness.VectorDiscreteSteps(**kw, **o), lambda rng, s: rng.integers(0, 13, n)),
            "VectorContinuousJumps": (lambda **o: harness.VectorContinuousJumps(**kw, **o), lambda rng, s: _actions(rng, s)),
            "VectorEnvironment": (lambda **o: harness.VectorEnvironment(**gpu.stopped_objects(n), **KW, **o),
                                  lambda rng, s: rng.integers(0, 13, n))}


@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("name", ["VectorDiscreteSteps", "VectorContinuousJumps", "VectorEnvironment"])
def test_twins_with_a_view(name, records, no_gpu):  # noqa: F811
    n, k = 65, 5
    make, action = _twin_classes(n)[name]
    plain = make(episode_records=records)
    viewed = make(episode_records=records, learner_view=harness.LearnerView(frame_stack=k))
    check = harness._LearnerView(harness.LearnerView(frame_stack=k), n, 4)
    assert plain.single_observation_space.shape == (4,) and viewed.single_observation_space.shape == (4 * k,)
    assert viewed.observation_space.shape == (n, 4 * k) and viewed.single_observation_space.dtype == np.float32
    assert (viewed.single_observation_space.low == -10).all() and (viewed.single_observation_space.high == 10).all()
    raw, info = plain.reset()
    obs, view_info = viewed.reset()
    assert info == {} and sorted(view_info) == ["raw_observation"] and same_bits(view_info["raw_observation"], raw)
    assert same_bits(obs, check.reset(raw)) and obs.dtype == np.float32 and obs.shape == (n, 4 * k)
    rngs = [np.random.default_rng(gpu.ACTION_SEED) for _ in range(2)]
    ended = 0
    for _ in range(STEPS):
        want = plain.step(action(rngs[0], plain._state))
        got = viewed.step(action(rngs[1], viewed._state))
        keys = ["raw_observation", "raw_reward"]
        if records:
            keys += ["final_observation", "raw_final_observation", "episode_return", "episode_length"]
        assert sorted(got[4]) == sorted(keys)
        # the raw results are those of the environment without a view
        assert same_bits(got[4]["raw_observation"], want[0]) and same_bits(got[4]["raw_reward"], np.asarray(want[1], F64))
        assert same_bits(got[2], want[2]) and same_bits(got[3], want[3])
        if records:
            assert same_bits(got[4]["raw_final_observation"], want[4]["final_observation"])
            assert same_bits(got[4]["episode_return"], want[4]["episode_return"])  # (raw, as a Monitor below reports)
            assert same_bits(got[4]["episode_length"], want[4]["episode_length"])
        view = check.step(want[0], want[1], want[2] | want[3], want[4]["final_observation"] if records else None)
        assert same_bits(got[0], view[0]) and same_bits(got[1], view[1]) and got[1].dtype == np.float64
        if records:
            assert same_bits(got[4]["final_observation"], view[2]) and view[2].shape == (n, 4 * k)
        assert all(same_bits(a, b) for a, b in zip(viewed.view_state(), (check.stack, check.returns)))
        assert all(same_bits(viewed.view_statistics()[key], check.statistics()[key]) for key in ("mean", "var", "count"))
        ended += int(want[3].sum())
    assert ended > 0
    statistics = viewed.view_statistics()
    viewed.set_view_training(False)
    viewed.step(action(rngs[1], viewed._state))
    assert all(same_bits(viewed.view_statistics()[key], statistics[key]) for key in statistics)
    statistics["mean"] = statistics["mean"] + 1.0
    viewed.set_view_statistics(statistics)
    assert same_bits(viewed.view_statistics()["mean"], statistics["mean"])
    with pytest.raises(ValueError, match="learner_view"):
        plain.view_statistics()
    plain.close(), viewed.close()


def test_spaces_without_norm_obs_repeat_the_raw_bounds(no_gpu):  # noqa: F811
    env = harness.VectorDiscreteSteps(num_envs=3, learner_view=harness.LearnerView(frame_stack=2, norm_obs=False),
                                      **gpu.TASK_KW)
    assert (env.single_observation_space.low == -1).all() and (env.single_observation_space.high == 1).all()
    assert env.single_observation_space.shape == (8,)
    env.close()


# ---- 4: what is refused -------------------------------------------------------------------------------------------------------
def test_refusals():
    """Before anything touches a GPU."""
    view = harness.LearnerView(frame_stack=5)
    for cls in (harness.ShardedVectorDiscreteSteps, harness.ShardedVectorContinuousJumps):
        with pytest.raises(ValueError, match="sharded"):
            cls(num_envs=4, devices=[0, 0], frame_height=8, samples_per_pixel=1, learner_view=view)
    for cls in (harness.DiscreteSteps, harness.ContinuousJumps):
        with pytest.raises(ValueError, match="single-environment"):
            cls(frame_height=8, samples_per_pixel=1, learner_view=view)
    for entry in (registration.vector_discrete_steps, registration.vector_continuous_jumps):
        with pytest.raises(ValueError, match="glue"):
            entry(num_envs=4, glue="host", frame_height=8, samples_per_pixel=1, learner_view=view)
    for bad in (dict(frame_stack=0), dict(frame_stack=9), dict(epsilon=0.0), dict(epsilon=np.nan), dict(clip_obs=-1.0),
                dict(clip_obs=np.inf), dict(clip_reward=0.0), dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=np.nan)):
        with pytest.raises(ValueError):
            harness.LearnerView(**bad)
    defaults = harness.LearnerView()
    assert (defaults.frame_stack, defaults.norm_obs, defaults.norm_reward, defaults.training) == (1, True, True, True)
    assert (defaults.gamma, defaults.epsilon, defaults.clip_obs, defaults.clip_reward) == (0.99, 1e-8, 10.0, 10.0)


def test_a_view_must_be_a_learner_view(no_gpu):  # noqa: F811
    with pytest.raises(TypeError, match="LearnerView"):
        harness.VectorDiscreteSteps(num_envs=3, learner_view=True, **gpu.TASK_KW)


# ---- 5: the seeds of the GPU tests ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 65, 1100, 2500])
def test_seeds_of_the_gpu_tests_give_partial_ends(n, no_gpu):  # noqa: F811
    """tests/test_gpu_learner_view.py, every schedule: some step ends 0 < k < n environments and some environment ends
    twice within the 12 steps; view_final then holds rows, and they are clipped values."""
    host = harness.VectorEnvironment(**_objects(n, "multi", gpu.SEED), episode_records=True,
                                     learner_view=harness.LearnerView(frame_stack=5), **KW)
    host.reset()
    ended = []
    for action in gpu.index_actions(n, steps=STEPS):
        result = host.step(action)
        ended.append(result[3].copy())
        assert not np.isnan(result[4]["final_observation"][result[3]]).any()
    assert gpu.some_partial([int(flags.sum()) for flags in ended], n), [int(f.sum()) for f in ended]
    assert (np.sum(ended, axis=0) >= 2).any()
    host.close()
