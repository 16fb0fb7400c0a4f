"""GPU tests of episode records (rf_env_configure_records, episode_records=True): the final observation of every episode
that ended -- the row the same-step auto-reset overwrites --, its return and its length, kept on the device by the step's
own kernels, against the numpy twin bit for bit (NaN equal to NaN) on every schedule of the step and for every kind of
context; records off leaves everything as it was; device io; snapshots carry the accumulators; what the library refuses.

Shapes are those of tests/test_gpu_snapshot.py: 16 x 16 pixels, 1-2 samples, 1 / 65 / 1100 environments (one lane, past
one wave, past the reset kernel's 1024-lane loop), TimeLimitEnder(3) | DivergingEnder so that most steps end a part of
the environments.  tests/test_episode_records_logic.py checks on the CPU that the seeds used here give such steps and
environments that end twice."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import state_observer as so
from reinfocus_amd.environments.snapshot import EnvSnapshot
from tests import helpers
from tests import observer_programs as op
from tests import test_gpu_snapshot as gpu
from tests.test_composed_env_logic import ENDS
from tests.test_gpu_device_initializer import KW
from tests.test_gpu_environment import BRANCH_NAME, FIRST_STEP_BRANCH, STEP_BRANCHES
from tests.test_gpu_snapshot import _close, _composed, _equal

pytestmark = pytest.mark.gpu

STEPS = 12
KEYS = ("final_observation", "episode_return", "episode_length")
RECORDS_WORD = 52  # byte offset of rf_env_snapshot_header::episode_records (include/reinfocus_hip.h)


def _same_records(dev, host, got, want):
    assert sorted(got[4]) == sorted(KEYS) and _equal(got[4], want[4]), "the step's info differs"
    n, width = want[0].shape
    assert got[4]["final_observation"].dtype == np.float32 and got[4]["final_observation"].shape == (n, width)
    assert got[4]["episode_return"].dtype == np.float64 and got[4]["episode_length"].dtype == np.int32
    assert _equal(dev.episode_accumulators(), host.episode_accumulators()), "the accumulators differ"


def _start(host, dev):
    o_h, i_h = host.reset()
    o_d, i_d = dev.reset()
    assert np.array_equal(o_h, o_d) and i_h == {} and i_d == {}
    assert _equal(dev.episode_accumulators(), host.episode_accumulators())


def _stepped(host, dev, actions, branch=None):
    """`actions` on both, the device held to the twin after each step: how many environments ended per step, per
    environment."""
    name = BRANCH_NAME.get(branch, branch)
    ended = []
    for step, action in enumerate(actions):
        action = action(host._state) if callable(action) else action
        want = host.step(action)
        got = dev.step(action)
        assert _equal(tuple(got[:4]), tuple(want[:4]))
        _same_records(dev, host, got, want)
        if branch is not None:
            assert dev._ctx.env_last_step_branch() == (FIRST_STEP_BRANCH.get(name, name) if step == 0 else name)
        ended.append(want[3].copy())
    return ended


def _partial_seen(ended, n):
    counts = [int(flags.sum()) for flags in ended]
    assert gpu.some_partial(counts, n), counts
    assert (np.sum(ended, axis=0) >= 2).any(), "no environment ended twice"


# ---- 1: the device against the twin on every schedule ---------------------------------------------------------------
@pytest.mark.parametrize("branch", list(STEP_BRANCHES))
@pytest.mark.parametrize("n", [1, 65, 1100])
def test_records_equal_the_twin_on_every_schedule(n, branch, monkeypatch):
    host, dev = _composed(n, branch, monkeypatch, samples_per_pixel=1 + n % 2, episode_records=True)
    _start(host, dev)
    _partial_seen(_stepped(host, dev, gpu.index_actions(n, steps=STEPS), branch), n)
    _close(host, dev)


# ---- 2: every kind of context ----------------------------------------------------------------------------------------
def _kind(kind, n):
    """tests/test_gpu_snapshot.py::_kind with episode_records=True on both: (twin, device, what to close, actions)."""
    from reinfocus_amd.environments import harness
    from tests import test_gpu_observed_env as observed
    from tests.test_continuous_vector_logic import _actions

    index = lambda rng: (lambda state: rng.integers(0, 13, n))  # noqa: E731
    kw = dict(num_envs=n, episode_records=True, **gpu.TASK_KW)
    records = dict(episode_records=True)
    if kind.startswith("discrete steps"):
        device = kind.endswith("device initializer")
        return harness.VectorDiscreteSteps(**kw), harness.DeviceVectorDiscreteSteps(device_initializer=device, **kw), [], index
    if kind == "continuous jumps":
        return (harness.VectorContinuousJumps(**kw), harness.DeviceVectorContinuousJumps(**kw), [],
                lambda rng: (lambda state: _actions(rng, state)))
    if kind == "stopped + delta":
        return (harness.VectorEnvironment(**gpu.stopped_objects(n), **records, **KW),
                harness.DeviceVectorEnvironment(**gpu.stopped_objects(n), **records, **KW), [], index)
    height, spp = KW["frame_height"], KW["samples_per_pixel"]
    renderers = [observed._renderer(spp) for _ in range(2)]
    if kind == "two delta observers":  # 12 columns
        trees = [observed._tree("delta of delta", n, renderer, height) for renderer in renderers]
    else:
        assert kind == "the widest tree"
        spec = max(observed.TREES, key=lambda s: op.width(s["tree"]))  # (16 columns: RF_ENV_MAX_OBS_COLUMNS)
        trees = [op.build(spec["tree"], n, so.FocusObserver(n, 0, 1, ENDS, renderer, height)) for renderer in renderers]
    width = trees[0].single_observation_space.shape[0]
    assert width > 4
    twin = harness.VectorEnvironment(**gpu.observed_strategies(n, width), observer=trees[1], **records)
    dev = harness.DeviceVectorEnvironment(**gpu.observed_strategies(n, width), observer=trees[0], **records)
    return twin, dev, renderers[:1], index


@pytest.mark.parametrize("kind", gpu.KINDS + ["the widest tree"])
def test_records_of_every_kind_of_context(kind):
    n = 65
    host, dev, extra, make_actions = _kind(kind, n)
    _start(host, dev)
    action = make_actions(np.random.default_rng(gpu.ACTION_SEED))
    ended = _stepped(host, dev, [action] * STEPS)
    assert gpu.some_partial([int(flags.sum()) for flags in ended], n)
    width = host.single_observation_space.shape[0]
    assert dev.step(action(host._state))[4]["final_observation"].shape == (n, width)
    _close(host, dev, *extra)


# ---- 3: off means unchanged ------------------------------------------------------------------------------------------
def _aligned(nbytes):
    return (nbytes + 255) & ~255


def test_records_off_is_the_environment_of_before(monkeypatch):
    n, h = 65, KW["frame_height"]
    _, off = _composed(n, monkeypatch=monkeypatch, host=False)
    _, on = _composed(n, monkeypatch=monkeypatch, host=False, episode_records=True)
    assert np.array_equal(off.reset()[0], on.reset()[0])
    for action in gpu.index_actions(n, steps=8):
        a, b = off.step(action), on.step(action)
        assert _equal(tuple(a[:4]), tuple(b[:4]))
        assert a[4] == {} and sorted(b[4]) == sorted(KEYS)
        assert np.array_equal(off._state, on._state) and _equal(off.strategy_state(), on.strategy_state())
        assert np.array_equal(off._ctx.get_states(0, n * h * h), on._ctx.get_states(0, n * h * h))
        assert off.initializer_state() == on.initializer_state()
        assert off._ctx.env_last_step_branch() == on._ctx.env_last_step_branch()
    with pytest.raises(ValueError, match="episode_records"):
        off.episode_accumulators()
    blob_off, blob_on = off.snapshot().blob, on.snapshot().blob
    # the layout of before: the header's word is 0 and the blob is shorter by exactly the two arrays
    assert blob_off.size == off._ctx.env_snapshot_size() == blob_on.size - _aligned(n * 8) - _aligned(n * 4)
    assert blob_off[RECORDS_WORD:RECORDS_WORD + 4].view(np.int32)[0] == 0
    assert blob_on[RECORDS_WORD:RECORDS_WORD + 4].view(np.int32)[0] == 1
    # ... and up to the two arrays, which precede the RNG states, the blobs hold the same bytes but for that word and size
    rng_bytes = _aligned(n * h * h * 16)
    a, b = blob_off[256:blob_off.size - rng_bytes], blob_on[256:blob_off.size - rng_bytes]
    assert np.array_equal(a, b) and np.array_equal(blob_off[-rng_bytes:], blob_on[-rng_bytes:])
    _close(off, on)


# ---- 4: device io (one child process that imports torch first: tests/episode_records_io_cases.py) --------------------
@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("episode_records_io") / "cases.jsonl")
    done = subprocess.run([sys.executable, "-m", "tests.episode_records_io_cases", path], cwd=helpers.ROOT,
                          capture_output=True, text=True, timeout=300)
    records = {}
    if os.path.exists(path):
        for line in open(path):
            record = json.loads(line)
            records[record["id"]] = record
    return records, f"exit status {done.returncode}\n{done.stderr[-3000:]}"


def _passed(recorded, name):
    records, ending = recorded
    assert name in records, f"the child process ended before case {name}: {ending}"
    assert records[name]["ok"], records[name]["message"]


@pytest.mark.parametrize("kind", ["composed-i64", "composed-i32", "jumps-f32"])
def test_step_tensors_returns_the_records_of_the_host_form(kind, recorded):
    """device_initializer=True: the info tensors of step_tensors equal what step() gives on a twin context, with the two
    forms mixed step by step on the device context, and the environment owns one set of them."""
    _passed(recorded, f"mixed/{kind}")


def test_out_keeps_its_meaning(recorded):
    _passed(recorded, "out")


def test_six_steps_enqueued_back_to_back(recorded):
    _passed(recorded, "queue")


def test_record_pointers_are_vouched_for_like_the_others(recorded):
    _passed(recorded, "refusals")
    _passed(recorded, "finished")


# ---- 5: snapshots ------------------------------------------------------------------------------------------------------
def _first_pass(host, dev, actions):
    records = []
    ended = []
    for action in actions:
        want = host.step(action)
        got = dev.step(action)
        assert _equal(tuple(got[:4]), tuple(want[:4]))
        _same_records(dev, host, got, want)
        records.append((tuple(got[:4]), got[4], dev.episode_accumulators()))
        ended.append(want[3].copy())
    return records, ended


def _replay(dev, actions, records):
    for step, (action, record) in enumerate(zip(actions, records)):
        got = dev.step(action)
        assert _equal((tuple(got[:4]), got[4], dev.episode_accumulators()), record), f"step {step} after the restore differs"


def _reports_pre_snapshot_rewards(records, ended, lengths_at_snapshot):
    """Some environment that was mid-episode at the snapshot ends afterwards with a length that counts those steps."""
    open_then = lengths_at_snapshot > 0
    assert open_then.any(), "the snapshot was not taken mid-episode"
    seen = np.zeros(len(open_then), dtype=bool)
    for step, (flags, (_, info, _)) in enumerate(zip(ended, records)):
        first = flags & ~seen & open_then
        assert (info["episode_length"][first] == lengths_at_snapshot[first] + step + 1).all()
        seen |= flags
    assert (seen & open_then).any()


@pytest.mark.parametrize("how", ["rewind", "file", "slot"])
def test_snapshots_carry_the_accumulators(how, monkeypatch, tmp_path):
    n = 65
    host, dev = _composed(n, monkeypatch=monkeypatch, episode_records=True)
    _start(host, dev)
    actions = gpu.index_actions(n)
    _, before = _first_pass(host, dev, actions[:gpu.HALF])
    at_snapshot = dev.episode_accumulators()
    if how == "slot":
        dev.snapshot_resident(1)
    else:
        snap = dev.snapshot()
        assert snap.episode_records and "episode_records=True" in snap.describe()
    records, after = _first_pass(host, dev, actions[gpu.HALF:])
    assert gpu.some_partial([int(f.sum()) for f in before], n) and gpu.some_partial([int(f.sum()) for f in after], n)
    _reports_pre_snapshot_rewards(records, after, at_snapshot[1])
    assert not _equal(dev.episode_accumulators(), at_snapshot)
    target, fresh = dev, None
    if how == "slot":
        dev.restore_resident(1)
    elif how == "rewind":
        dev.restore(snap)
    else:  # a fresh environment of equal arguments, never reset, restores what a file held
        path = tmp_path / "records.snapshot"
        snap.save(path)
        _, fresh = _composed(n, monkeypatch=monkeypatch, host=False, episode_records=True)
        loaded = EnvSnapshot.load(path)
        assert loaded.episode_records
        fresh.restore(loaded)
        target = fresh
    assert _equal(target.episode_accumulators(), at_snapshot)
    _replay(target, actions[gpu.HALF:], records)
    if how == "slot":
        dev.drop_snapshot(1)
    _close(host, dev, fresh)


def test_a_blob_of_the_other_setting_is_refused_and_nothing_changes(monkeypatch):
    n = 65
    _, off = _composed(n, monkeypatch=monkeypatch, host=False)
    _, on = _composed(n, monkeypatch=monkeypatch, host=False, episode_records=True)
    for env in (off, on):
        env.reset()
        for action in gpu.index_actions(n, steps=2):
            env.step(action)
    snaps = {env: env.snapshot() for env in (off, on)}
    for env, other in ((off, on), (on, off)):
        seen = gpu._probe(env)
        with pytest.raises(ValueError, match="episode_records"):
            env.restore(snaps[other])
        with pytest.raises(AssertionError, match="episode records"):  # (the library's own refusal names the setting)
            env._ctx.env_restore(snaps[other].blob)
        assert _equal(gpu._probe(env), seen) and np.array_equal(env.snapshot().blob, snaps[env].blob)
    _close(off, on)


# ---- 6: what the library refuses --------------------------------------------------------------------------------------
def test_abi_refusals_change_nothing(monkeypatch):
    n = 65
    _, off = _composed(n, monkeypatch=monkeypatch, host=False)
    _, on = _composed(n, monkeypatch=monkeypatch, host=False, episode_records=True)
    # rf_env_get_records: without records, and before the first step after a reset
    with pytest.raises(AssertionError, match="keeps no episode records"):
        off._ctx.env_records()
    with pytest.raises(AssertionError, match="keeps no episode records"):
        off._ctx.env_record_accumulators()
    on.reset()
    with pytest.raises(AssertionError, match="no step since the last reset"):
        on._ctx.env_records()
    off.reset()
    actions = gpu.index_actions(n, steps=3)
    for env in (off, on):
        env.step(actions[0])
    assert sorted(on.step(actions[1])[4]) == sorted(KEYS)
    on.reset()
    with pytest.raises(AssertionError, match="no step since the last reset"):
        on._ctx.env_records()
    on.step(actions[0])
    on.step(actions[1])
    # rf_env_configure_records after a step: refused either way
    for env, setting in ((off, True), (on, False), (on, True)):
        seen = gpu._probe(env)
        with pytest.raises(AssertionError, match="has stepped"):
            env._ctx.env_configure_records(setting)
        assert _equal(gpu._probe(env), seen)
    assert off.step(actions[2])[4] == {} and sorted(on.step(actions[2])[4]) == sorted(KEYS)  # (both still step)
    # a NULL context, and the exports
    lib = _native.load()
    assert lib.rf_env_configure_records(None, 1) == _native.RF_ERR_INVALID
    assert lib.rf_env_get_records(None, None, None, None) == _native.RF_ERR_INVALID
    assert lib.rf_abi_version() == 1
    _close(off, on)


def test_single_and_sharded_environments_refuse_records():
    from reinfocus_amd.environments import harness

    with pytest.raises(ValueError, match="sharded"):
        harness.ShardedVectorDiscreteSteps(num_envs=4, devices=[0, 0], frame_height=16, samples_per_pixel=2,
                                           episode_records=True)
    with pytest.raises(ValueError, match="single-environment"):
        harness.DiscreteSteps(frame_height=16, samples_per_pixel=2, episode_records=True)


def test_records_with_the_visualiser(monkeypatch):
    """render_mode="rgb_array" with records is allowed for step(): the records equal those of an environment without
    a visualiser up to the first 600 px render (which re-seeds the RNG states)."""
    from reinfocus_amd.environments import harness

    n = 3
    kw = dict(num_envs=n, episode_records=True, **gpu.TASK_KW)
    plain, drawn = harness.DeviceVectorDiscreteSteps(**kw), harness.DeviceVectorDiscreteSteps(render_mode="rgb_array", **kw)
    plain.reset()
    drawn.reset()
    rng = np.random.default_rng(2)
    for _ in range(6):
        action = rng.integers(0, 13, n)
        a, b = plain.step(action), drawn.step(action)
        assert _equal(tuple(a[:4]), tuple(b[:4])) and _equal(a[4], b[4])
    _close(plain, drawn)
