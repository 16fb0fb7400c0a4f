"""GPU tests of the device initializer (rf_env_configure_initializer, device_initializer=True): the reset states drawn on
the device against the host twin's numpy initializer bit for bit -- on every schedule of the step, at one lane, past one
wave and past the 1024-lane loop of the reset kernel, with one and with several ranges per element, when every
environment ends every step and when none ever does, through graph replays, reseeding and pinned starts --, the task
environments with and without it, and everything the library refuses on such a context."""

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import episode_ender as ee
from reinfocus_amd.environments import episode_rewarder as er
from reinfocus_amd.environments import state_initializer as si
from reinfocus_amd.environments import state_transformer as st
from reinfocus_amd.environments import strategy_program as sp
from tests.test_composed_env_logic import ACTION_SET, ENDS
from tests.test_continuous_vector_logic import _actions
from tests.test_gpu_environment import BRANCH_NAME, FIRST_STEP_BRANCH, STEP_BRANCHES

pytestmark = pytest.mark.gpu

RANGES = {"single": [[ENDS], [ENDS]], "multi": [[ENDS], [(5.0, 6.0), (9.0, 10.0)]]}  # 2 / 4 draws a row
DRAWS = {"single": 2, "multi": 4}
KW = dict(frame_height=16, samples_per_pixel=2, device=0)


def _objects(n, ranges, seed, ender="limit"):
    """Fresh strategy objects (each environment owns its own).  limit: TimeLimitEnder(3) | DivergingEnder -- most steps
    reset some environments, some reset many, a few none."""
    ender = {"limit": lambda: ee.TimeLimitEnder(n, 3) | ee.DivergingEnder(n, (0, 1), 0.125, 1),
             "every": lambda: ee.TimeLimitEnder(n, 1), "never": lambda: ee.EndlessEnder(n)}[ender]()
    return dict(ender=ender, rewarder=er.ObservationRewarder(1) + er.OnTargetRewarder((0, 1), 0.25),
                transformer=st.DiscreteMoveTransformer(n, 1, ENDS, ACTION_SET),
                initializer=si.RangedInitializer(RANGES[ranges], seed=seed), num_envs=n)


def _pair(n, ranges, seed, branch="fused-graph", monkeypatch=None, ender="limit", **kw):
    from reinfocus_amd.environments import harness

    kw = {**KW, **kw}
    host = harness.VectorEnvironment(**_objects(n, ranges, seed, ender), **kw)
    for key, value in STEP_BRANCHES[branch].items():
        monkeypatch.setenv(key, value)
    dev = harness.DeviceVectorEnvironment(**_objects(n, ranges, seed, ender), device_initializer=True, **kw)
    for key in STEP_BRANCHES[branch]:
        monkeypatch.delenv(key)
    return host, dev


def _twin_generator(host):
    return sp.initializer_state(host._initializer)


def _same(host, dev, got=None, want=None):
    """Everything the two environments hold, and a step's results."""
    if got is not None:
        for x, y in zip(got[:4], want[:4]):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
    assert np.array_equal(host._state, dev._state)
    for x, y in zip(dev.strategy_state(), host.strategy_state()):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    assert dev.initializer_state() == _twin_generator(host)


def _run(host, dev, steps, seed=6):
    """reset(), then `steps` steps compared after each; the number of environments that ended in each step."""
    n = host.num_envs
    o_h, _ = host.reset()
    o_d, _ = dev.reset()
    assert o_d.dtype == np.float32 and np.array_equal(o_h, o_d)
    _same(host, dev)
    rng = np.random.default_rng(seed)
    ended = []
    for _ in range(steps):
        actions = rng.integers(0, 13, n)
        want = host.step(actions)
        _same(host, dev, dev.step(actions), want)
        ended.append(int(want[3].sum()))
    return ended


@pytest.mark.parametrize("branch", list(STEP_BRANCHES))
@pytest.mark.parametrize("n", [1, 65, 1100])
@pytest.mark.parametrize("ranges", ["single", "multi"])
def test_device_initializer_equals_host_twin(ranges, n, branch, monkeypatch):
    """Observations, rewards, flags, states, strategy state and the generator's state after reset() and after every one
    of 12 steps, on every schedule of the step.  The host twin's initializer object is the reference: the device
    environment's own object is never advanced."""
    host, dev = _pair(n, ranges, 13, branch, monkeypatch, samples_per_pixel=1 + n % 2)
    before = sp.initializer_state(dev._initializer)
    name_b = BRANCH_NAME.get(branch, branch)
    n_h = host.num_envs
    o_h, _ = host.reset()
    o_d, _ = dev.reset()
    assert np.array_equal(o_h, o_d)
    _same(host, dev)
    rng = np.random.default_rng(6)
    ended = []
    for step in range(12):
        actions = rng.integers(0, 13, n_h)
        want = host.step(actions)
        _same(host, dev, dev.step(actions), want)
        assert dev._ctx.env_last_step_branch() == (FIRST_STEP_BRANCH.get(name_b, name_b) if step == 0 else name_b)
        ended.append(int(want[3].sum()))
    assert sum(ended) > 0
    if n > 1:  # (some steps reset only a part of the environments: the rows are handed out by rank)
        assert any(0 < k < n for k in ended)
    assert sp.initializer_state(dev._initializer) == before  # (the object only describes the environment)
    host.close()
    dev.close()


@pytest.mark.parametrize("ranges", ["single", "multi"])
@pytest.mark.parametrize("ender,per_step", [("every", 1), ("never", 0)])
def test_every_environment_ends_every_step_and_none_ever(ender, per_step, ranges, monkeypatch):
    """The generator advances by n * d a step when every environment ends every step and by nothing when none ever
    does; both stay equal to the twin."""
    n = 65
    host, dev = _pair(n, ranges, 21, ender=ender, monkeypatch=monkeypatch)
    host.reset()
    dev.reset()
    state, inc = dev.initializer_state()
    bit_generator = np.random.PCG64DXSM(0)
    rng = np.random.default_rng(2)
    for _ in range(5):
        actions = rng.integers(0, 13, n)
        want = host.step(actions)
        _same(host, dev, dev.step(actions), want)
        assert int(want[3].sum()) == per_step * n
        bit_generator.state = {"bit_generator": "PCG64DXSM", "state": {"state": state, "inc": inc}, "has_uint32": 0,
                               "uinteger": 0}
        bit_generator.advance(per_step * n * DRAWS[ranges])
        state = bit_generator.state["state"]["state"]
        assert dev.initializer_state() == (state, inc)
    host.close()
    dev.close()


@pytest.mark.parametrize("task", ["DeviceVectorDiscreteSteps", "DeviceVectorContinuousJumps"])
def test_task_environments_with_and_without_the_device_initializer(task):
    """The same class with device_initializer=True and False and equal seeds over 20 steps at 64 x 16 x 16 x 2."""
    from reinfocus_amd.environments import harness

    n = 64
    kw = dict(max_episode_steps=5, num_envs=n, seed=31, **KW)
    plain = getattr(harness, task)(**kw)
    drawn = getattr(harness, task)(device_initializer=True, **kw)
    assert np.array_equal(plain.reset()[0], drawn.reset()[0])
    assert np.array_equal(plain._state, drawn._state) and plain.initializer_state() == drawn.initializer_state()
    rng = np.random.default_rng(4)
    ended = 0
    for _ in range(20):
        actions = rng.integers(0, 13, n) if task == "DeviceVectorDiscreteSteps" else _actions(rng, plain._state)
        want = plain.step(actions)
        got = drawn.step(actions)
        for x, y in zip(got[:4], want[:4]):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert np.array_equal(plain._state, drawn._state) and plain.initializer_state() == drawn.initializer_state()
        ended += int(want[3].sum())
    assert ended > n
    plain.close()
    drawn.close()


def test_graph_replay_sees_the_generator_move(monkeypatch):
    """30 steps on the fused-graph branch, the generator read after each: a replay that captured a stale state, or an
    advance that is not ordered before the next draw, shows here."""
    host, dev = _pair(300, "multi", 5, monkeypatch=monkeypatch)
    ended = _run(host, dev, 30)
    assert dev._ctx.env_last_step_branch() == "fused-graph" and sum(1 for k in ended if k > 0) > 15
    host.close()
    dev.close()


def test_reseeding_and_pinned_starts(monkeypatch):
    from reinfocus_amd.environments import harness

    n = 65
    host, dev = _pair(n, "multi", 3, monkeypatch=monkeypatch)
    _run(host, dev, 4)
    # reset(seed=...) mid-run: as the twin's, and the states and the generator of a fresh environment of that seed
    o_h, _ = host.reset(seed=77)
    o_d, _ = dev.reset(seed=77)
    assert np.array_equal(o_h, o_d)
    _same(host, dev)
    fresh = harness.DeviceVectorEnvironment(**_objects(n, "multi", 77), device_initializer=True, **KW)
    fresh.reset()
    assert np.array_equal(fresh._state, dev._state) and fresh.initializer_state() == dev.initializer_state()
    fresh.close()
    rng = np.random.default_rng(8)
    for _ in range(4):
        actions = rng.integers(0, 13, n)
        want = host.step(actions)
        _same(host, dev, dev.step(actions), want)
    # reset(state=...) installs the states and leaves the generator where it was
    before = dev.initializer_state()
    start = np.linspace(5.0, 10.0, 2 * n, dtype=np.float32).reshape(n, 2)
    o_h, _ = host.reset(state=start)
    o_d, _ = dev.reset(state=start)
    assert np.array_equal(o_h, o_d) and np.array_equal(dev._state, start) and dev.initializer_state() == before
    for _ in range(4):
        actions = rng.integers(0, 13, n)
        want = host.step(actions)
        _same(host, dev, dev.step(actions), want)
    host.close()
    dev.close()


def _malformed_programs(good):
    """(what is wrong, program) for every refusal of rf_env_configure_initializer's list."""
    def changed(change):
        program = _native.EnvInitializerProgram.from_buffer_copy(good)
        change(program)
        return program

    def setter(field, j, c, value):
        def change(program):
            getattr(program, field)[j][c] = value
        return change

    def count(j, value):
        def change(program):
            program.counts[j] = value
        return change

    def even(program):
        program.inc[0] &= ~1

    return [("no ranges", changed(count(0, 0))), ("nine ranges", changed(count(1, 9))),
            ("a negative count", changed(count(1, -1))),
            ("a NaN low", changed(setter("low", 1, 1, float("nan")))),
            ("an infinite low", changed(setter("low", 0, 0, float("-inf")))),
            ("a NaN span", changed(setter("span", 0, 0, float("nan")))),
            ("an infinite span", changed(setter("span", 1, 0, float("inf")))),
            ("a low outside float32", changed(setter("low", 0, 0, -3.4e38))),
            ("a high outside float32", changed(setter("span", 1, 1, 3.4e38))),
            ("an even increment", changed(even))]


def test_refusals_change_nothing(monkeypatch):
    """A pool, the two-phase and sharded halves and every malformed program are refused on a context with a device
    initializer, which goes on as if nothing had been asked; a context without the call still needs its pool."""
    from reinfocus_amd.environments import harness

    n = 12
    host, dev = _pair(n, "multi", 9, monkeypatch=monkeypatch)
    _run(host, dev, 3)
    ctx = dev._ctx
    actions = np.zeros(n, dtype=np.int32)
    pool = np.full((n, 2), 7.5, dtype=np.float32)

    def snapshot():
        return [dev._state, *dev.strategy_state()], dev.initializer_state()

    before = snapshot()
    calls = [lambda: ctx.env_step(actions, pool), lambda: ctx.env_step_plan(actions), lambda: ctx.env_step_begin(actions),
             lambda: ctx.env_step_end(pool[:1]), lambda: ctx.env_step_run(pool[:1]),
             lambda: ctx.env_step_end_given(pool[:1], np.zeros(1)), lambda: ctx.env_render_states(pool[:2]),
             lambda: ctx.env_step_jumps(actions.astype(np.float32))]  # (the other dtype's entry point, as before)
    good = sp.compile_initializer(si.RangedInitializer(RANGES["multi"], seed=1))
    programs = _malformed_programs(good)
    calls += [lambda p=p: ctx.env_configure_initializer(p) for _, p in programs]
    calls.append(lambda: ctx.env_set_initializer_state(5, 8))  # (an even increment)
    for call in calls:
        with pytest.raises(AssertionError):
            call()
    after = snapshot()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before[0], after[0])) and before[1] == after[1]
    rng = np.random.default_rng(12)
    for _ in range(4):  # ... and the environment goes on equal to its twin
        a = rng.integers(0, 13, n)
        want = host.step(a)
        _same(host, dev, dev.step(a), want)
    host.close()
    dev.close()

    # no environment configured: refused; a context without the call needs its pool and its states, and has no generator
    bare = _native.Context(0)
    with pytest.raises(AssertionError):
        bare.env_configure_initializer(good)
    bare.close()
    plain = harness.DeviceVectorEnvironment(**_objects(n, "multi", 9), **KW)
    plain.reset()
    for call in (lambda: plain._ctx.env_step(actions, None), lambda: plain._ctx.env_reset(None),
                 plain._ctx.env_initializer_state, lambda: plain._ctx.env_set_initializer_state(5, 7)):
        with pytest.raises(AssertionError):
            call()
    for _, program in programs:  # (refused before anything is configured, too)
        with pytest.raises(AssertionError):
            plain._ctx.env_configure_initializer(program)
    twin = harness.VectorEnvironment(**_objects(n, "multi", 9), **KW)
    twin.reset()
    a = rng.integers(0, 13, n)
    want = twin.step(a)
    for x, y in zip(plain.step(a)[:4], want[:4]):
        assert np.array_equal(x, y)
    twin.close()
    plain.close()


def test_unsupported_initializers_are_refused_by_the_environment():
    from reinfocus_amd.environments import harness

    with pytest.raises(AssertionError):
        harness.DeviceVectorEnvironment(**{**_objects(4, "single", 1), "initializer": harness._Initializer(ENDS, 1)},
                                        device_initializer=True, **KW)
    with pytest.raises(ValueError, match="device_initializer"):
        harness.ShardedVectorDiscreteSteps(num_envs=4, devices=[0, 0], device_initializer=True, frame_height=16,
                                           samples_per_pixel=2)


def test_visualiser_works_from_the_device_states(monkeypatch):
    """render_mode="rgb_array" with a device initializer: the visualiser takes the drawn states from the device and shows
    the same 600 px frames as the numpy-glue twin."""
    n = 4
    host, dev = _pair(n, "multi", 9, monkeypatch=monkeypatch, render_mode="rgb_array")
    assert np.array_equal(host.reset()[0], dev.reset()[0])
    rng = np.random.default_rng(2)
    for _ in range(5):
        a, b = host.render(), dev.render()
        assert a.shape == b.shape and np.array_equal(a[:, :600], b[:, :600])
        actions = rng.integers(0, 13, n)
        want = host.step(actions)
        _same(host, dev, dev.step(actions), want)
    host.close()
    dev.close()
