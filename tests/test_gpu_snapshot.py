"""GPU tests of environment snapshots (rf_env_snapshot* / rf_env_restore*, env.snapshot() / restore() and the resident
slots): an environment set back to a snapshot, or a fresh one of equal arguments that restores it, goes on bit for bit as
the uninterrupted run did -- results, states, strategy and observer state, the initializer's generator and every pixel's
RNG state after every step --, on every schedule of the step, for every kind of context, through files and through the
slots in device memory; everything the library refuses leaves the environment as it was.

The uninterrupted run is itself held to the host twin step by step.  Shapes are those of
tests/test_gpu_device_initializer.py: 16 x 16 pixels, 1-2 samples, 1 / 65 / 1100 environments (one lane, past one wave,
past the reset kernel's 1024-lane loop), TimeLimitEnder(3) | DivergingEnder so that most steps reset some environments.
Every rewind and resume asserts that some step before and some step after the snapshot ended 0 < k < n environments: a
restore that forgot the compacted scene set or the ranks would show.  tests/test_snapshot_logic.py checks on the CPU that
the seeds used here give such steps."""

import numpy as np
import pytest

from reinfocus_amd.environments import episode_ender as ee
from reinfocus_amd.environments import episode_rewarder as er
from reinfocus_amd.environments import state_initializer as si
from reinfocus_amd.environments import state_transformer as st
from reinfocus_amd.environments import strategy_program as sp
from reinfocus_amd.environments.snapshot import EnvSnapshot
from tests.test_composed_env_logic import ACTION_SET, ENDS
from tests.test_continuous_vector_logic import _actions
from tests.test_gpu_device_initializer import KW, RANGES, _objects
from tests.test_gpu_environment import BRANCH_NAME, STEP_BRANCHES

pytestmark = pytest.mark.gpu

SEED, ACTION_SEED, OTHER_ACTION_SEED = 13, 6, 44  # (tests/test_snapshot_logic.py: they give partial resets where needed)
HALF = 6  # steps before the snapshot, and after it
TASK_KW = dict(max_episode_steps=5, seed=31, **KW)  # (the tasks' DivergingEnder needs 3 steps: a limit of 3 would end all at once)


def index_actions(n, seed=ACTION_SEED, steps=2 * HALF):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 13, n) for _ in range(steps)]


def some_partial(ended, n):
    """Some step ended a part of the environments (n == 1: one ended)."""
    return any(0 < k < n for k in ended) if n > 1 else any(k == 1 for k in ended)


# ---- what is compared ---------------------------------------------------------------------------------------------------
def _probe(dev):
    """Everything of a device environment that a test can see, fetched from the device."""
    h = dev._shard.frame_height
    seen = {"state": dev._state, "rng": dev._ctx.get_states(0, dev.num_envs * h * h), "generator": dev.initializer_state(),
            "scene_len": dev._ctx.env_scene_len()}
    if hasattr(dev, "strategy_state"):
        seen["strategy"] = dev.strategy_state()
    if getattr(dev, "_observed", False):
        seen["observer"] = dev.observer_state()
    if not dev._device_initializer:  # (the rows the host generator would hand the next step)
        seen["pool"] = dev._initializer.propose(dev.num_envs)
    return seen


def _equal(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b


def _held_to_twin(host, dev, got=None, want=None):
    if got is not None:
        assert _equal(tuple(got[:4]), tuple(want[:4]))
    assert np.array_equal(host._state, dev._state)
    assert dev.initializer_state() == sp.initializer_state(host._initializer)
    if hasattr(dev, "strategy_state"):
        assert _equal(dev.strategy_state(), host.strategy_state())
    if getattr(dev, "_observed", False):
        assert _equal(dev.observer_state(), host.observer_state())


def _first_pass(host, dev, actions):
    """`actions` (arrays, or callables of the current state) stepped on both, the device held to the twin after each:
    (the actions taken, what the device returned and showed after each step, how many environments ended)."""
    taken, records, ended = [], [], []
    for action in actions:
        action = action(host._state) if callable(action) else action
        want = host.step(action)
        got = dev.step(action)
        _held_to_twin(host, dev, got, want)
        taken.append(action)
        records.append((tuple(got[:4]), _probe(dev)))
        ended.append(int(want[3].sum()))
    return taken, records, ended


def _replay(dev, actions, records):
    for step, (action, record) in enumerate(zip(actions, records)):
        got = dev.step(action)
        assert _equal((tuple(got[:4]), _probe(dev)), record), f"step {step} after the restore differs"


def _start(host, dev):
    o_h, _ = host.reset()
    o_d, _ = dev.reset()
    assert np.array_equal(o_h, o_d)
    _held_to_twin(host, dev)


# ---- the environments ---------------------------------------------------------------------------------------------------
def _composed(n, branch="fused-graph", monkeypatch=None, ranges="multi", seed=SEED, device_initializer=True, ender="limit",
              host=True, **kw):
    """(host twin or None, device environment) of tests/test_gpu_device_initializer.py's composition."""
    from reinfocus_amd.environments import harness

    kw = {**KW, **kw}
    twin = harness.VectorEnvironment(**_objects(n, ranges, seed, ender), **kw) if host else None
    for key, value in STEP_BRANCHES[branch].items():
        monkeypatch.setenv(key, value)
    dev = harness.DeviceVectorEnvironment(**_objects(n, ranges, seed, ender), device_initializer=device_initializer, **kw)
    for key in STEP_BRANCHES[branch]:
        monkeypatch.delenv(key)
    return twin, dev


def stopped_objects(n, seed=SEED):
    """A StoppedEnder (histories on the device) and a DeltaRewarder (an old value per environment)."""
    return dict(ender=ee.TimeLimitEnder(n, 3) | ee.DivergingEnder(n, (0, 1), 0.125, 1) | ee.StoppedEnder(n, 1, 0.3, 2),
                rewarder=er.DeltaRewarder(1, 0.5) + er.ObservationRewarder(1),
                transformer=st.DiscreteMoveTransformer(n, 1, ENDS, ACTION_SET),
                initializer=si.RangedInitializer(RANGES["multi"], seed=seed), num_envs=n)


def observed_strategies(n, width, seed=SEED):
    """tests/test_gpu_observed_env.py's composition under this file's ender."""
    from tests.test_gpu_observed_env import _strategies

    return {**_strategies(n, width, seed), "ender": ee.TimeLimitEnder(n, 3) | ee.DivergingEnder(n, (0, 1), 0.125, 1)}


KINDS = ["discrete steps, host initializer", "discrete steps, device initializer", "continuous jumps", "stopped + delta",
         "two delta observers"]


def _kind(kind, n, host=True):
    """(host twin or None, device environment, what to close afterwards, the kind's actions)."""
    from reinfocus_amd.environments import harness
    from tests import test_gpu_observed_env as observed

    index = lambda rng: (lambda state: rng.integers(0, 13, n))  # noqa: E731
    kw = dict(num_envs=n, **TASK_KW)
    if kind.startswith("discrete steps"):
        device = kind.endswith("device initializer")
        twin = harness.VectorDiscreteSteps(**kw) if host else None
        return twin, harness.DeviceVectorDiscreteSteps(device_initializer=device, **kw), [], index
    if kind == "continuous jumps":
        twin = harness.VectorContinuousJumps(**kw) if host else None
        return twin, harness.DeviceVectorContinuousJumps(**kw), [], lambda rng: (lambda state: _actions(rng, state))
    if kind == "stopped + delta":
        twin = harness.VectorEnvironment(**stopped_objects(n), **KW) if host else None
        return twin, harness.DeviceVectorEnvironment(**stopped_objects(n), **KW), [], index
    assert kind == "two delta observers"
    height, spp = KW["frame_height"], KW["samples_per_pixel"]
    renderers = [observed._renderer(spp) for _ in range(2 if host else 1)]
    trees = [observed._tree("delta of delta", n, renderer, height) for renderer in renderers]
    width = trees[0].single_observation_space.shape[0]
    twin = harness.VectorEnvironment(**observed_strategies(n, width), observer=trees[1]) if host else None
    dev = harness.DeviceVectorEnvironment(**observed_strategies(n, width), observer=trees[0])
    return twin, dev, renderers[:1], index  # (the twin closes its own renderer)


def _close(*things):
    for thing in things:
        if thing is not None:
            thing.close()


# ---- 1: rewind ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch", list(STEP_BRANCHES))
@pytest.mark.parametrize("n", [1, 65, 1100])
def test_rewind_on_every_schedule(n, branch, monkeypatch):
    """reset(), 6 steps, snapshot(), 6 more steps, restore(), the same 6 actions again: everything equals the first
    pass after every step, and the first step after the restore is a replayed graph where the schedule has one."""
    host, dev = _composed(n, branch, monkeypatch, samples_per_pixel=1 + n % 2)
    _start(host, dev)
    actions = index_actions(n)
    _, _, before = _first_pass(host, dev, actions[:HALF])
    snap = dev.snapshot()
    assert snap.host_generator is None and snap.num_envs == n and snap.env_class == "DeviceVectorEnvironment"
    at_snapshot = _probe(dev)
    _, records, after = _first_pass(host, dev, actions[HALF:])
    assert some_partial(before, n) and some_partial(after, n), (before, after)
    assert not _equal(_probe(dev), at_snapshot)
    for _ in range(2):  # (a snapshot is not used up)
        assert dev.restore(snap) is None
        assert _equal(_probe(dev), at_snapshot)
        dev.step(actions[HALF])
        name = BRANCH_NAME.get(branch, branch)
        assert dev._ctx.env_last_step_branch() == name  # (not the first step's branch: the graph was kept)
        dev.restore(snap)
        _replay(dev, actions[HALF:], records)
    _close(host, dev)


# ---- 2: resume ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 1100])
def test_resume_in_a_fresh_context_through_a_file(n, tmp_path, monkeypatch):
    """The snapshot saved, loaded and restored into an environment built from equal arguments that was never reset:
    the same actions give the uninterrupted run, other actions what a twin gives that took them from step 7 on."""
    spp = dict(samples_per_pixel=1 + n % 2)
    host, dev = _composed(n, monkeypatch=monkeypatch, **spp)
    _start(host, dev)
    actions = index_actions(n)
    _, _, before = _first_pass(host, dev, actions[:HALF])
    path = tmp_path / "environment.snapshot"
    dev.snapshot().save(path)
    _, records, after = _first_pass(host, dev, actions[HALF:])
    assert some_partial(before, n) and some_partial(after, n), (before, after)
    _close(host, dev)

    _, fresh = _composed(n, monkeypatch=monkeypatch, host=False, **spp)
    fresh.restore(EnvSnapshot.load(path))
    _replay(fresh, actions[HALF:], records)
    fresh.close()

    other = index_actions(n, OTHER_ACTION_SEED, HALF)
    assert not all(np.array_equal(a, b) for a, b in zip(other, actions[HALF:]))
    host, branched = _composed(n, monkeypatch=monkeypatch, **spp)
    host.reset()
    for action in actions[:HALF]:
        host.step(action)
    branched.restore(EnvSnapshot.load(path))
    _held_to_twin(host, branched)
    _, _, after = _first_pass(host, branched, other)
    assert some_partial(after, n), after
    _close(host, branched)


# ---- 3: every kind of context -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_rewind_and_resume_for_every_kind_of_context(kind, tmp_path):
    """Both tasks, with the reset states drawn on the host (the host generator travels in the snapshot: the pool rows
    proposed after a restore are the uninterrupted run's) and on the device; a composed environment with a StoppedEnder's
    histories and a DeltaRewarder's old values; an observer tree with two DeltaObservers' old values."""
    n = 65
    host, dev, described, make_actions = _kind(kind, n)
    _start(host, dev)
    action = make_actions(np.random.default_rng(ACTION_SEED))
    _, _, before = _first_pass(host, dev, [action] * HALF)
    snap = dev.snapshot()
    assert (snap.host_generator is None) == dev._device_initializer
    at_snapshot = _probe(dev)
    actions, records, after = _first_pass(host, dev, [action] * HALF)
    assert some_partial(before, n) and some_partial(after, n), (before, after)
    if kind == "stopped + delta":  # (the histories and the old values hold something, and moved on)
        counters, floats, histories, old = records[-1][1]["strategy"]
        assert histories.shape == (3, n) and not np.isnan(histories[-1]).any() and old.shape == (2, n)
        assert not _equal(records[-1][1]["strategy"], at_snapshot["strategy"])
    if kind == "two delta observers":
        assert records[-1][1]["observer"].shape == (9, n) and not _equal(records[-1][1]["observer"], at_snapshot["observer"])
    dev.restore(snap)
    assert _equal(_probe(dev), at_snapshot)
    _replay(dev, actions, records)
    snap.save(tmp_path / "kind.npz")
    _close(host, dev, *described)

    _, fresh, described, _ = _kind(kind, n, host=False)
    fresh.restore(EnvSnapshot.load(tmp_path / "kind.npz"))
    assert _equal(_probe(fresh), at_snapshot)
    _replay(fresh, actions, records)
    _close(fresh, *described)


# ---- 4: resident slots --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_initializer", [True, False])
def test_resident_slots(device_initializer, monkeypatch):
    """Slots 0 and 1 filled at steps 3 and 6 of a run of 10: restoring either, in either order, any number of times, gives
    that point's continuation; the host snapshot taken right after a restore is the one taken when the slot was filled,
    byte for byte; a dropped slot is empty.  With the reset states drawn on the host, that generator is kept per slot."""
    n = 65
    host, dev = _composed(n, monkeypatch=monkeypatch, device_initializer=device_initializer)
    _start(host, dev)
    actions = index_actions(n, steps=10)
    _, first, ended_a = _first_pass(host, dev, actions[:3])
    dev.snapshot_resident(0)
    blob_0 = dev.snapshot()
    _, second, ended_b = _first_pass(host, dev, actions[3:6])
    dev.snapshot_resident(1)
    blob_1 = dev.snapshot()
    _, third, ended_c = _first_pass(host, dev, actions[6:])
    assert some_partial(ended_a, n) and some_partial(ended_b, n) and some_partial(ended_c, n), (ended_a, ended_b, ended_c)
    records = first + second + third
    points = {0: (3, blob_0), 1: (6, blob_1)}
    for slot in (0, 1, 1, 0, 0, 1):
        at, blob = points[slot]
        dev.restore_resident(slot)
        again = dev.snapshot()
        assert np.array_equal(again.blob, blob.blob) and again.host_generator == blob.host_generator
        _replay(dev, actions[at:], records[at:])
    dev.drop_snapshot(0)
    for call in (lambda: dev.restore_resident(0), lambda: dev.drop_snapshot(0)):
        before = _probe(dev)
        with pytest.raises(AssertionError, match="empty"):
            call()
        assert _equal(_probe(dev), before)
    dev.restore_resident(1)  # (the other slot is untouched)
    _replay(dev, actions[6:], records[6:])
    dev.snapshot_resident(0)  # ... and a dropped slot can be filled again
    dev.restore_resident(1)
    dev.restore_resident(0)
    assert _equal(_probe(dev), records[-1][1])
    _close(host, dev)


# ---- 5: refusals --------------------------------------------------------------------------------------------------------
def _flipped(blob, byte):
    bad = blob.copy()
    bad[byte] ^= 0xFF
    return bad


def test_refusals_change_nothing(monkeypatch):
    from reinfocus_amd.environments import harness

    n = 12
    host, dev = _composed(n, monkeypatch=monkeypatch)
    _start(host, dev)
    actions = index_actions(n, steps=10)
    _first_pass(host, dev, actions[:3])
    ctx = dev._ctx
    good = dev.snapshot()
    dev.snapshot_resident(1)
    _first_pass(host, dev, actions[3:6])  # (a restore that went through would be seen)

    def blob_of(**changes):
        """A snapshot's blob of an environment that differs from `dev` in one thing."""
        arguments = dict(n=n, ranges="multi", ender="limit")
        arguments.update({k: changes.pop(k) for k in list(changes) if k in arguments})
        _, other = _composed(arguments.pop("n"), monkeypatch=monkeypatch, host=False, **arguments, **changes)
        other.reset()
        snap = other.snapshot()
        other.close()
        return snap

    wrong = {"n": blob_of(n=n + 1), "frame height": blob_of(frame_height=32), "spp": blob_of(samples_per_pixel=3),
             "program": blob_of(ender="every"), "initializer": blob_of(ranges="single")}
    assert wrong["spp"].blob.size == wrong["program"].blob.size == wrong["initializer"].blob.size == good.blob.size
    refused = [(lambda: ctx.env_restore(good.blob[:-1]), "bytes"),
               (lambda: ctx.env_restore(np.concatenate([good.blob, good.blob[:256]])), "bytes"),
               (lambda: ctx.env_restore(_flipped(good.blob, 0)), "magic"),
               (lambda: ctx.env_restore(_flipped(good.blob, 8)), "version"),
               (lambda: ctx.env_restore(wrong["n"].blob), "bytes"),
               (lambda: ctx.env_restore(wrong["frame height"].blob), "bytes"),
               (lambda: ctx.env_restore(wrong["spp"].blob), "spp"),
               (lambda: ctx.env_restore(wrong["program"].blob), "rf_env_program"),
               (lambda: ctx.env_restore(wrong["initializer"].blob), "initializer"),
               (lambda: dev.restore_resident(0), "empty"), (lambda: dev.drop_snapshot(3), "empty")]
    for slot in (4, -1):
        refused += [(lambda s=slot: dev.snapshot_resident(s), "slot"), (lambda s=slot: dev.restore_resident(s), "slot"),
                    (lambda s=slot: dev.drop_snapshot(s), "slot")]
    before = _probe(dev)
    for call, match in refused:
        with pytest.raises(AssertionError, match=match):
            call()
        assert _equal(_probe(dev), before), match
    for name in ("n", "frame height", "spp"):  # (the environment says so itself where it can tell)
        with pytest.raises(ValueError, match="the snapshot is of"):
            dev.restore(wrong[name])
    for name in ("program", "initializer"):
        with pytest.raises(AssertionError):
            dev.restore(wrong[name])
    assert _equal(_probe(dev), before)
    _first_pass(host, dev, actions[6:])  # ... and the environment goes on equal to its twin
    _close(host, dev)

    # before the first reset() there is nothing to snapshot
    _, fresh = _composed(n, monkeypatch=monkeypatch, host=False)
    for call in (fresh.snapshot, fresh.snapshot_resident):
        with pytest.raises(AssertionError, match="rf_env_reset first"):
            call()
    fresh.close()

    # an open two-phase or planned step; an aborted step.  (The halves need a context that takes its pool from the host.)
    host, plain = _composed(n, monkeypatch=monkeypatch, device_initializer=False)
    _start(host, plain)
    _first_pass(host, plain, actions[:3])
    ctx = plain._ctx
    good = plain.snapshot()
    at_snapshot = _probe(plain)
    plain.snapshot_resident(0)
    calls = [ctx.env_snapshot, lambda: ctx.env_restore(good.blob), lambda: ctx.env_snapshot_resident(1),
             lambda: ctx.env_restore_resident(0)]
    for begin in (lambda: ctx.env_step_begin(actions[3].astype(np.int32)), lambda: ctx.env_step_plan(actions[3].astype(np.int32))):
        begin()
        before = _probe(plain)
        for call in calls:
            with pytest.raises(AssertionError, match="step is open"):
                call()
        assert _equal(_probe(plain), before)
        ctx.env_step_abort()
        for call in (ctx.env_snapshot, lambda: ctx.env_snapshot_resident(1)):
            with pytest.raises(AssertionError, match="aborted"):
                call()
        assert _equal(_probe(plain), before)
        plain.restore(good)  # a restore is what makes the environment usable again, as a reset would
        assert _equal(_probe(plain), at_snapshot)
    _first_pass(host, plain, actions[3:6])
    _close(host, plain)

    # environments with a visualiser, and sharded ones
    shown = harness.DeviceVectorDiscreteSteps(num_envs=2, render_mode="rgb_array", **TASK_KW)
    shown.reset()
    for call in (shown.snapshot, lambda: shown.restore(good), shown.snapshot_resident, shown.restore_resident):
        with pytest.raises(ValueError, match="render_mode"):
            call()
    shown.close()
    sharded = harness.ShardedVectorDiscreteSteps(num_envs=4, devices=[0, 0], frame_height=16, samples_per_pixel=2)
    sharded.reset()
    for call in (sharded.snapshot, lambda: sharded.restore(good), sharded.snapshot_resident, sharded.restore_resident,
                 sharded.drop_snapshot):
        with pytest.raises(ValueError, match="no snapshots"):
            call()
    sharded.close()


# ---- 6: rf_env_render after a restore -----------------------------------------------------------------------------------
def test_render_after_a_restore_draws_the_snapshot_points_scene_set(monkeypatch):
    """ctx.env_render(32, 2) after a restore -- in place, and into a fresh context -- against the same call at the
    snapshot point of an uninterrupted twin run, where the scene set is the full one (nobody ended in the last step) and
    where it is the compacted one.  (32 px frames of all n environments need more RNG states than 16 px steps do: every
    context here is seeded for them before its reset, as _DeviceShard.render would.)"""
    n = 65

    def made(ender):
        _, env = _composed(n, monkeypatch=monkeypatch, host=False, ender=ender)
        env._ctx.seed(n * 32 * 32, 0, 0)
        return env

    actions = index_actions(n, steps=10)
    for ender, partial in (("never", False), ("limit", True)):
        twin, env = made(ender), made(ender)
        twin.reset()
        env.reset()
        point = 0
        for action in actions[:8]:
            ended = int(twin.step(action)[3].sum())
            env.step(action)
            point += 1
            if point >= 3 and (0 < ended < n) == partial:
                break
        length = ended if partial else n
        assert (0 < ended < n) == partial and twin._ctx.env_scene_len() == length
        want = twin._ctx.env_render(32, 2)
        assert want.shape == (length, 32, 32, 3) and want.std() > 0
        snap = env.snapshot()
        for action in actions[point:point + 2]:  # (other scene sets, other RNG states)
            env.step(action)
        env.restore(snap)
        assert env._ctx.env_scene_len() == length and np.array_equal(env._ctx.env_render(32, 2), want)
        fresh = made(ender)
        fresh.restore(snap)
        assert fresh._ctx.env_scene_len() == length and np.array_equal(fresh._ctx.env_render(32, 2), want)
        _close(twin, env, fresh)
