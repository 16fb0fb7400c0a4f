"""GPU tests of the device-resident vector ContinuousJumps (rf_env_configure_jumps, rf_env_step*_jumps): against its
numpy-glue twin (harness.VectorContinuousJumps) bit for bit on every schedule of the step, against the single
harness.ContinuousJumps, next to a DiscreteSteps context in the same process, sharded, visualised, and at the
benchmark's shape."""

import numpy as np
import pytest

from tests.test_continuous_vector_logic import _actions
from tests.test_gpu_environment import BRANCH_NAME, FIRST_STEP_BRANCH, STEP_BRANCHES

pytestmark = pytest.mark.gpu


def _same_step(got, want):
    for x, y in zip(got[:4], want[:4]):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize("branch", list(STEP_BRANCHES))
@pytest.mark.parametrize("n,height,spp,steps", [(64, 32, 4, 45), (300, 16, 2, 30), (24, 132, 1, 40)])
def test_device_step_equals_host_twin(n, height, spp, steps, branch, monkeypatch, kernel_choice):
    """Observations, float64 rewards, flags, states and initializer consumption after every step, through auto-resets,
    on every schedule of rf_env_step_jumps."""
    from reinfocus_amd.environments import harness

    kw = dict(max_episode_steps=9, num_envs=n, frame_height=height, samples_per_pixel=spp, seed=13, device=0)
    host = harness.VectorContinuousJumps(**kw)
    for name, value in STEP_BRANCHES[branch].items():
        monkeypatch.setenv(name, value)
    dev = harness.DeviceVectorContinuousJumps(**kw)
    for name in STEP_BRANCHES[branch]:
        monkeypatch.delenv(name)
    o_h, _ = host.reset()
    o_d, _ = dev.reset()
    assert o_d.dtype == np.float32 and np.array_equal(o_h, o_d)
    assert np.array_equal(host._state, dev._state)
    rng = np.random.default_rng(6)
    resets = stops = 0
    for step in range(steps):
        actions = _actions(rng, host._state)
        before = host._state.copy()
        want = host.step(actions)
        got = dev.step(actions.reshape(n, 1) if step % 2 else actions)
        _same_step(got, want)
        assert got[1].dtype == np.float64
        assert np.array_equal(host._state, dev._state)
        assert host._initializer._generator.bit_generator.state == dev._initializer._generator.bit_generator.state
        name = BRANCH_NAME.get(branch, branch)
        assert dev._ctx.env_last_step_branch() == (FIRST_STEP_BRANCH.get(name, name) if step == 0 else name)
        resets += int(want[3].sum())
        stops += int(np.sum(~want[3] & (host._state[:, 1] == before[:, 1])))
    assert resets > 0 and stops > 0
    host.close()
    dev.close()


def test_one_environment_equals_the_single_continuous_jumps(kernel_choice):
    """num_envs=1 with a time limit that never comes: step by step the single environment (DivergingEnder only, no
    auto-reset) until its first end."""
    from reinfocus_amd.environments import harness

    kw = dict(frame_height=48, samples_per_pixel=4, seed=3, device=0)
    single = harness.ContinuousJumps(**kw)
    dev = harness.DeviceVectorContinuousJumps(max_episode_steps=10 ** 6, num_envs=1, **kw)
    o_s, _ = single.reset()
    o_d, _ = dev.reset()
    assert np.array_equal(o_s, o_d[0])
    rng = np.random.default_rng(1)
    for step in range(200):
        action = _actions(rng, single._state)[0]
        obs, reward, terminated, truncated, _ = single.step(action)
        got = dev.step(np.array([action]))
        assert got[1][0] == reward and type(reward) is np.float64
        assert got[2][0] == terminated and got[3][0] == truncated
        if truncated:  # (the vector environment has reset itself already: its observation is the new episode's)
            assert np.all(got[0][0, 2:] == 0)
            break
        assert np.array_equal(obs, got[0][0])
        assert np.array_equal(single._state, dev._state)
    assert truncated and step > 2
    single.close()
    dev.close()


def test_discrete_and_continuous_contexts_side_by_side(kernel_choice):
    """A DiscreteSteps and a ContinuousJumps context stepped alternately in one process each equal their twin; the
    int32 calls on the continuous context, the float32 calls on the discrete one and bad float actions are refused
    and change nothing."""
    from reinfocus_amd.environments import harness

    n = 40
    kw = dict(max_episode_steps=6, num_envs=n, frame_height=24, samples_per_pixel=3, device=0)
    d_host, d_dev = harness.VectorDiscreteSteps(seed=1, **kw), harness.DeviceVectorDiscreteSteps(seed=1, **kw)
    c_host, c_dev = harness.VectorContinuousJumps(seed=2, **kw), harness.DeviceVectorContinuousJumps(seed=2, **kw)
    assert np.array_equal(d_host.reset()[0], d_dev.reset()[0])
    assert np.array_equal(c_host.reset()[0], c_dev.reset()[0])
    rng = np.random.default_rng(9)
    pool = np.full((n, 2), 7.5, dtype=np.float32)
    for step in range(16):
        _same_step(d_dev.step(a := rng.integers(0, 13, n)), d_host.step(a))
        _same_step(c_dev.step(a := _actions(rng, c_host._state)), c_host.step(a))
        if step % 4 == 1:
            before = [c_dev._state, *c_dev._ctx.env_counters(), d_dev._state, *d_dev._ctx.env_counters()]
            ints, floats = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
            for call in (lambda: c_dev._ctx.env_step(ints, pool), lambda: c_dev._ctx.env_step_begin(ints),
                         lambda: c_dev._ctx.env_step_plan(ints), lambda: d_dev._ctx.env_step_jumps(floats, pool),
                         lambda: d_dev._ctx.env_step_begin_jumps(floats), lambda: d_dev._ctx.env_step_plan_jumps(floats)):
                with pytest.raises(AssertionError):
                    call()
            for bad in (np.nan, np.inf, -np.inf, 1.5, -1.0000001):
                floats[n // 2] = bad
                for call in (lambda: c_dev._ctx.env_step_jumps(floats, pool),
                             lambda: c_dev._ctx.env_step_begin_jumps(floats),
                             lambda: c_dev._ctx.env_step_plan_jumps(floats)):
                    with pytest.raises(AssertionError, match="outside"):
                        call()
                with pytest.raises(AssertionError):
                    c_dev.step(floats)
            after = [c_dev._state, *c_dev._ctx.env_counters(), d_dev._state, *d_dev._ctx.env_counters()]
            assert all(np.array_equal(x, y) for x, y in zip(before, after))
        assert np.array_equal(d_host._state, d_dev._state) and np.array_equal(c_host._state, c_dev._state)
    for env in (d_host, d_dev, c_host, c_dev):
        env.close()


def _onto_target(state):
    """Jumps onto the target: nobody diverges."""
    return ((state[:, 0] - 5.0) / 5.0 * 2.0 - 1.0).astype(np.float32)


@pytest.mark.parametrize("n,shards", [(12, 2), (7, 3)])
def test_sharded_environment_equals_one_device(n, shards, kernel_choice):
    """ShardedVectorContinuousJumps (rf_env_step_plan_jumps + rf_env_step_run) with several contexts on device 0
    against one DeviceVectorContinuousJumps: identical while renders are full ones, and the initializer's states go
    to the ended environments in global index order."""
    from reinfocus_amd.environments import harness

    kw = dict(max_episode_steps=6, num_envs=n, frame_height=24, samples_per_pixel=3, seed=21)
    one = harness.DeviceVectorContinuousJumps(device=0, **kw)
    many = harness.ShardedVectorContinuousJumps(devices=[0] * shards, **kw)
    assert np.array_equal(one.reset()[0], many.reset()[0])
    for _ in range(5):
        actions = _onto_target(one._state)
        a, b = one.step(actions), many.step(actions)
        _same_step(a, b)
        assert not b[3].any() and np.array_equal(one._state, many._state)
    actions = _onto_target(one._state)
    a, b = one.step(actions), many.step(actions)
    assert a[3].all() and b[3].all() and np.array_equal(a[1], b[1])
    assert np.array_equal(one._state, many._state)
    assert one._initializer._generator.bit_generator.state == many._initializer._generator.bit_generator.state
    rng = np.random.default_rng(3)
    for _ in range(6):  # different sample paths from here on (partial renders per shard): the invariants hold
        obs, rewards, terminated, truncated, _ = many.step(_actions(rng, many._state))
        assert obs.shape == (n, 4) and np.all(np.abs(obs) <= 1) and rewards.dtype == np.float64
        assert np.all(obs[truncated, 2:] == 0)
    one.close()
    many.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_exact_mode_equals_one_device_through_auto_resets(shards, kernel_choice):
    """exact=True (rf_env_step_begin_jumps, rf_env_render_states, rf_env_step_end_given): bit for bit one device
    through many auto-resets, RNG states included."""
    from reinfocus_amd.environments import harness

    n = 13
    kw = dict(max_episode_steps=5, num_envs=n, frame_height=24, samples_per_pixel=3, seed=31)
    one = harness.DeviceVectorContinuousJumps(device=0, **kw)
    many = harness.ShardedVectorContinuousJumps(devices=[0] * shards, exact=True, **kw)
    assert np.array_equal(one.reset()[0], many.reset()[0])
    rng = np.random.default_rng(77)
    sizes = set()
    for _ in range(28):
        actions = _actions(rng, one._state)
        a, b = one.step(actions), many.step(actions)
        _same_step(a, b)
        assert np.array_equal(one._state, many._state)
        sizes.add(int(b[3].sum()))
    assert len(sizes) >= 3
    assert one._initializer._generator.bit_generator.state == many._initializer._generator.bit_generator.state
    states = np.concatenate(many._each(lambda shard: shard.ctx.get_states()))
    assert np.array_equal(states, one._ctx.get_states())
    many.close()
    one.close()


def test_device_visualiser_equals_host_glue(kernel_choice):
    """render_mode="rgb_array": the same 600 px frames from render() (full sets and the one-row set of a lone
    auto-reset), the same results afterwards, the same visualiser bookkeeping as the numpy-glue twin."""
    from reinfocus_amd.environments import harness

    kw = dict(max_episode_steps=5, num_envs=4, render_mode="rgb_array", frame_height=32, samples_per_pixel=2, seed=9,
              device=0)
    host = harness.VectorContinuousJumps(**kw)
    dev = harness.DeviceVectorContinuousJumps(**kw)
    start = [[7.5, 7.5]] * 4
    assert np.array_equal(host.reset(state=start)[0], dev.reset(state=start)[0])
    rows_seen = set()
    # environment 0 jumps away from its target by 0.5 more every step (ends alone after 3 diverging steps); the others
    # stay put (a jump to where the plane is) and end at the time limit
    away = [0.2, 0.4, 0.6, 0.8, 1.0, -1.0, -0.6, -0.2]
    for step in range(8):
        a, b = host.render(), dev.render()
        assert a.shape == b.shape and a.shape[0] % 600 == 0
        assert np.array_equal(a[:, :600], b[:, :600])
        assert np.array_equal(host.render_frames(), dev.render_frames())
        rows_seen.add(a.shape[0] // 600)
        actions = np.array([away[step], 0.0, 0.0, 0.0], dtype=np.float32)
        _same_step(dev.step(actions), host.step(actions))
        assert np.array_equal(host._state, dev._state)
        for i in range(4):
            assert host._ender.status(i) == dev._shard.status(i)
        assert np.array_equal(host._visualizer._current_moves, dev._visualizer._current_moves)
        assert np.array_equal(host._visualizer._targets, dev._visualizer._targets)
    assert {1, 4} <= rows_seen
    host.close()
    dev.close()


def test_headline_shape_spot_check():
    """4096 environments of 256 x 256 pixels at 16 samples (bench.py's shape), a few steps with auto-resets."""
    from reinfocus_amd.environments import harness

    n = 4096
    kw = dict(max_episode_steps=2, num_envs=n, frame_height=256, samples_per_pixel=16, seed=4, device=0)
    host = harness.VectorContinuousJumps(**kw)
    dev = harness.DeviceVectorContinuousJumps(**kw)
    assert np.array_equal(host.reset()[0], dev.reset()[0])
    rng = np.random.default_rng(0)
    for _ in range(4):
        actions = _actions(rng, host._state)
        want = host.step(actions)
        _same_step(dev.step(actions), want)
        assert np.array_equal(host._state, dev._state)
    assert want[3].all()  # (the time limit ended every environment in the last step)
    host.close()
    dev.close()
