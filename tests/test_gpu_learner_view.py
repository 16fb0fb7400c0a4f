"""GPU tests of the learner view (rf_env_configure_view, learner_view=harness.LearnerView(...)): VecNormalize followed by
VecFrameStack, computed by env_view_moments_kernel and env_view_apply_kernel (csrc/rf_env_view.h) after every step and
reset, against the numpy twin bit for bit -- float32 and float64 arrays are compared as bytes, so zero signs and NaNs
count -- on every schedule of the step, for every kind of context, for several view configurations; device io; snapshots
carry the view's state; what the library refuses.

Shapes are those of tests/test_gpu_episode_records.py: 16 x 16 pixels, 1-2 samples, TimeLimitEnder(3) | DivergingEnder,
12 steps; 1 / 3 / 65 / 1100 / 2500 environments cover the tree's padding, one wave, past a wave, two leaves per thread,
and four leaves per thread with threads that own padding only.  tests/test_learner_view_logic.py checks on the CPU that
the seeds used here end a part of the environments and some environment twice, and holds the twin to the definition."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness
from reinfocus_amd.environments import state_observer as so
from reinfocus_amd.environments.snapshot import EnvSnapshot
from tests import helpers
from tests import observer_programs as op
from tests import test_gpu_snapshot as gpu
from tests.test_composed_env_logic import ENDS
from tests.test_gpu_device_initializer import KW
from tests.test_gpu_environment import BRANCH_NAME, FIRST_STEP_BRANCH, STEP_BRANCHES
from tests.test_gpu_snapshot import _close, _composed

pytestmark = pytest.mark.gpu

STEPS = 12
STACK = 5
VIEW_HASH_WORD, VIEW_TRAINING_WORD = 104, 112  # byte offsets in rf_env_snapshot_header (include/reinfocus_hip.h)


def _view(**kw):
    return harness.LearnerView(**{"frame_stack": STACK, **kw})


def _bits(a):
    a = np.asarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b):
    """Arrays as bytes, through dicts and tuples; anything else by ==."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and _bits(a) == _bits(b)
    return a == b


def _seen(env):
    """The view's state and statistics, from the device or the twin."""
    return env.view_state(), env.view_statistics()


def _same_step(dev, host, got, want, records=True):
    keys = ["raw_observation", "raw_reward"]
    if records:
        keys += ["final_observation", "raw_final_observation", "episode_return", "episode_length"]
    assert sorted(got[4]) == sorted(keys) == sorted(want[4])
    names = ["view observation", "view reward", "terminated", "truncated"] + sorted(keys)
    pairs = list(zip(got[:4], want[:4])) + [(got[4][key], want[4][key]) for key in sorted(keys)]
    for name, (x, y) in zip(names, pairs):
        assert _bits(x) == _bits(y), f"{name} differs"
    (stack, returns), statistics = _seen(dev)
    (want_stack, want_returns), want_statistics = _seen(host)
    assert _bits(stack) == _bits(want_stack), "the stack differs"
    assert _bits(returns) == _bits(want_returns), "the returns differ"
    for key in ("mean", "var", "count"):
        assert _bits(statistics[key]) == _bits(want_statistics[key]), f"the statistics' {key} differs"
    assert _bits(got[0]) == _bits(stack)  # (the view observation is the stack)


def _start(host, dev):
    (o_h, i_h), (o_d, i_d) = host.reset(), dev.reset()
    assert sorted(i_d) == ["raw_observation"] and _same(o_d, o_h) and _same(i_d, i_h)
    assert _same(_seen(dev), _seen(host))


def _stepped(host, dev, actions, branch=None, records=True, at=None):
    """`actions` on both, the device held to the twin after each step; at: {step: what to do to both before it}."""
    name = BRANCH_NAME.get(branch, branch)
    ended = []
    for step, action in enumerate(actions):
        if at and step in at:
            at[step](host), at[step](dev)
        action = action(host._state) if callable(action) else action
        want = host.step(action)
        got = dev.step(action)
        _same_step(dev, host, got, want, records)
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
def test_view_equals_the_twin_on_every_schedule(n, branch, monkeypatch):
    host, dev = _composed(n, branch, monkeypatch, samples_per_pixel=1 + n % 2, episode_records=True, learner_view=_view())
    assert dev.single_observation_space.shape == (4 * STACK,) and dev.observation_space.shape == (n, 4 * STACK)
    assert (dev.single_observation_space.high == 10).all()
    _start(host, dev)
    _partial_seen(_stepped(host, dev, gpu.index_actions(n, steps=STEPS), branch), n)
    _close(host, dev)


@pytest.mark.parametrize("n", [3, 2500])
def test_view_equals_the_twin_at_other_sizes(n, monkeypatch):
    host, dev = _composed(n, "fused", monkeypatch, samples_per_pixel=1, episode_records=True, learner_view=_view())
    _start(host, dev)
    _partial_seen(_stepped(host, dev, gpu.index_actions(n, steps=STEPS), "fused"), n)
    _close(host, dev)


# ---- 2: every kind of context ----------------------------------------------------------------------------------------
def _kind(kind, n):
    """tests/test_gpu_episode_records.py::_kind with records and a view on both: (twin, device, what to close, actions)."""
    from tests import test_gpu_observed_env as observed
    from tests.test_continuous_vector_logic import _actions

    index = lambda rng: (lambda state: rng.integers(0, 13, n))  # noqa: E731
    extra = lambda: dict(episode_records=True, learner_view=_view())  # noqa: E731
    kw = dict(num_envs=n, **gpu.TASK_KW)
    if kind.startswith("discrete steps"):
        device = kind.endswith("device initializer")
        return (harness.VectorDiscreteSteps(**kw, **extra()),
                harness.DeviceVectorDiscreteSteps(device_initializer=device, **kw, **extra()), [], index)
    if kind == "continuous jumps":
        return (harness.VectorContinuousJumps(**kw, **extra()), harness.DeviceVectorContinuousJumps(**kw, **extra()), [],
                lambda rng: (lambda state: _actions(rng, state)))
    if kind == "stopped + delta":
        return (harness.VectorEnvironment(**gpu.stopped_objects(n), **extra(), **KW),
                harness.DeviceVectorEnvironment(**gpu.stopped_objects(n), **extra(), **KW), [], index)
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
    twin = harness.VectorEnvironment(**gpu.observed_strategies(n, width), observer=trees[1], **extra())
    dev = harness.DeviceVectorEnvironment(**gpu.observed_strategies(n, width), observer=trees[0], **extra())
    return twin, dev, renderers[:1], index


@pytest.mark.parametrize("kind", gpu.KINDS + ["the widest tree"])
def test_view_of_every_kind_of_context(kind):
    n = 65
    host, dev, extra, make_actions = _kind(kind, n)
    width = host._view._width
    assert dev.single_observation_space.shape == (width * STACK,) == host.single_observation_space.shape
    _start(host, dev)
    action = make_actions(np.random.default_rng(gpu.ACTION_SEED))
    ended = _stepped(host, dev, [action] * STEPS)
    assert gpu.some_partial([int(flags.sum()) for flags in ended], n)
    assert dev.step(action(host._state))[4]["final_observation"].shape == (n, width * STACK)
    _close(host, dev, *extra)


# ---- 3: the view's configurations ------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [dict(frame_stack=1), dict(frame_stack=8), dict(norm_obs=False), dict(norm_reward=False),
                                    dict(gamma=0.9, epsilon=1e-6, clip_obs=0.5, clip_reward=0.25),
                                    dict(training=False)],
                         ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
@pytest.mark.parametrize("records", [True, False])
def test_view_configurations(config, records, monkeypatch):
    n = 65
    host, dev = _composed(n, monkeypatch=monkeypatch, episode_records=records, learner_view=_view(**config))
    _start(host, dev)
    ended = _stepped(host, dev, gpu.index_actions(n, steps=STEPS), records=records)
    assert gpu.some_partial([int(flags.sum()) for flags in ended], n)
    if config.get("training") is False:
        assert _same(dev.view_statistics()["count"], np.full(5, 1e-4)) and not dev.view_state()[1].any()
    _close(host, dev)


def test_training_off_after_six_steps_and_statistics_round_trip(monkeypatch):
    n = 65
    host, dev = _composed(n, monkeypatch=monkeypatch, episode_records=True, learner_view=_view())
    _start(host, dev)

    kept = {}

    def frozen(env):
        env.set_view_training(False)
        kept[id(env)] = env.view_statistics(), env.view_state()[1]

    def loaded(env):  # what VecNormalize.load does: statistics from elsewhere, then evaluation
        statistics, returns = kept[id(env)]
        assert _same(env.view_statistics(), statistics)  # (two steps without training moved no moment ...)
        assert _same(env.view_state()[1], np.where(ended_since[0], 0.0, returns))  # (... and no return: endings zero them)
        statistics = {"mean": statistics["mean"] * 0.5, "var": statistics["var"] + 0.25, "count": statistics["count"] * 2.0}
        env.set_view_statistics(statistics)
        assert _same(env.view_statistics(), statistics)

    ended_since = [np.zeros(n, dtype=bool)]
    actions = gpu.index_actions(n, steps=STEPS)
    ended = _stepped(host, dev, actions[:6])
    frozen(host), frozen(dev)
    ended += _stepped(host, dev, actions[6:8])
    ended_since[0] = ended[6] | ended[7]
    loaded(host), loaded(dev)
    ended += _stepped(host, dev, actions[8:], at={2: lambda env: env.set_view_training(True)})
    assert gpu.some_partial([int(flags.sum()) for flags in ended], n)
    before = dev.view_statistics()
    host.reset(), dev.reset()  # a reset never resets the moments
    assert _same(_seen(dev), _seen(host)) and (dev.view_statistics()["count"][:4] == before["count"][:4] + n).all()
    _close(host, dev)


def test_view_off_is_the_environment_of_before(monkeypatch):
    n, h = 65, KW["frame_height"]
    _, off = _composed(n, monkeypatch=monkeypatch, host=False, episode_records=True)
    _, on = _composed(n, monkeypatch=monkeypatch, host=False, episode_records=True, learner_view=_view())
    assert np.array_equal(off.reset()[0], on.reset()[1]["raw_observation"])
    for action in gpu.index_actions(n, steps=8):
        a, b = off.step(action), on.step(action)
        assert _same(a[0], b[4]["raw_observation"]) and _same(a[1], b[4]["raw_reward"]) and _same(a[3], b[3])
        assert _same(a[4]["final_observation"], b[4]["raw_final_observation"])
        assert _same(a[4]["episode_return"], b[4]["episode_return"])
        assert np.array_equal(off._state, on._state) and _same(off.strategy_state(), on.strategy_state())
        assert np.array_equal(off._ctx.get_states(0, n * h * h), on._ctx.get_states(0, n * h * h))
        assert off.initializer_state() == on.initializer_state()
        assert off._ctx.env_last_step_branch() == on._ctx.env_last_step_branch()
    with pytest.raises(ValueError, match="learner_view"):
        off.view_statistics()
    blob_off, blob_on = off.snapshot().blob, on.snapshot().blob
    aligned = lambda nbytes: (nbytes + 255) & ~255  # noqa: E731
    extra = aligned(n * 4 * STACK * 4) + aligned(n * 8) + aligned(3 * 17 * 8)
    assert blob_off.size == off._ctx.env_snapshot_size() == blob_on.size - extra
    assert not blob_off[VIEW_HASH_WORD:256].any()  # (the words of a blob without a view are what they were: zero)
    assert blob_on[VIEW_HASH_WORD:VIEW_HASH_WORD + 8].any()
    assert blob_on[VIEW_TRAINING_WORD:VIEW_TRAINING_WORD + 4].view(np.int32)[0] == 1
    rng_bytes = aligned(n * h * h * 16)
    a, b = blob_off[256:blob_off.size - rng_bytes], blob_on[256:blob_off.size - rng_bytes]
    assert np.array_equal(a, b) and np.array_equal(blob_off[-rng_bytes:], blob_on[-rng_bytes:])
    _close(off, on)


# ---- 4: device io (one child process that imports torch first: tests/learner_view_io_cases.py) -----------------------
@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("learner_view_io") / "cases.jsonl")
    done = subprocess.run([sys.executable, "-m", "tests.learner_view_io_cases", path], cwd=helpers.ROOT,
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
def test_step_tensors_returns_the_view_of_the_host_form(kind, recorded):
    """step_tensors equals step() on a twin context bit for bit, with the two forms mixed step by step on the device
    context -- with records (i64, f32) and without (i32) --, and the environment owns one set of tensors."""
    _passed(recorded, f"mixed/{kind}")


def test_out_means_the_view(recorded):
    _passed(recorded, "out")


def test_six_steps_enqueued_back_to_back(recorded):
    _passed(recorded, "queue")


def test_view_pointers_are_vouched_for_like_the_others(recorded):
    _passed(recorded, "refusals")
    _passed(recorded, "finished")


# ---- 5: snapshots ------------------------------------------------------------------------------------------------------
def _first_pass(host, dev, actions):
    records, ended = [], []
    for action in actions:
        want = host.step(action)
        got = dev.step(action)
        _same_step(dev, host, got, want)
        records.append((tuple(got[:4]), got[4], _seen(dev)))
        ended.append(want[3].copy())
    return records, ended


def _replay(dev, actions, records):
    for step, (action, record) in enumerate(zip(actions, records)):
        got = dev.step(action)
        assert _same((tuple(got[:4]), got[4], _seen(dev)), record), f"step {step} after the restore differs"


@pytest.mark.parametrize("how", ["rewind", "file", "slot"])
def test_snapshots_carry_the_view(how, monkeypatch, tmp_path):
    n = 65
    host, dev = _composed(n, monkeypatch=monkeypatch, episode_records=True, learner_view=_view())
    _start(host, dev)
    actions = gpu.index_actions(n)
    _, before = _first_pass(host, dev, actions[:gpu.HALF])
    host.set_view_training(False), dev.set_view_training(False)  # (content: the restore brings it back)
    _first_pass(host, dev, actions[:1])
    host.set_view_training(True), dev.set_view_training(True)
    at_snapshot = _seen(dev)
    if how == "slot":
        dev.snapshot_resident(1)
    else:
        snap = dev.snapshot()
    records, after = _first_pass(host, dev, actions[gpu.HALF:])
    assert gpu.some_partial([int(f.sum()) for f in before], n) and gpu.some_partial([int(f.sum()) for f in after], n)
    assert not _same(_seen(dev), at_snapshot)
    dev.set_view_training(False)  # (the snapshot was taken while training: the restore says so again)
    target, fresh = dev, None
    if how == "slot":
        dev.restore_resident(1)
    elif how == "rewind":
        dev.restore(snap)
    else:  # a fresh environment of equal arguments, never reset, restores what a file held
        path = tmp_path / "view.snapshot"
        snap.save(path)
        _, fresh = _composed(n, monkeypatch=monkeypatch, host=False, episode_records=True,
                             learner_view=_view(training=False))
        fresh.restore(EnvSnapshot.load(path))
        target = fresh
    assert _same(_seen(target), at_snapshot)
    _replay(target, actions[gpu.HALF:], records)
    if how == "slot":
        dev.drop_snapshot(1)
    _close(host, dev, fresh)


def test_a_blob_of_another_view_is_refused_and_nothing_changes(monkeypatch):
    n = 65
    views = {"none": None, "five": _view(), "two": _view(frame_stack=2), "clip": _view(clip_obs=5.0),
             "plain rewards": _view(norm_reward=False)}
    envs = {name: _composed(n, monkeypatch=monkeypatch, host=False, episode_records=True, learner_view=view)[1]
            for name, view in views.items()}
    for env in envs.values():
        env.reset()
        for action in gpu.index_actions(n, steps=2):
            env.step(action)
    snaps = {name: env.snapshot() for name, env in envs.items()}
    for name, env in envs.items():
        for other in envs:
            if other == name:
                continue
            seen = gpu._probe(env), (None if name == "none" else _seen(env))
            with pytest.raises(AssertionError, match="learner view"):  # (the library's refusal names the setting)
                env.restore(snaps[other])
            assert _same((gpu._probe(env), (None if name == "none" else _seen(env))), seen)
            assert np.array_equal(env.snapshot().blob, snaps[name].blob)
    # `training` is content, not fingerprint: such a blob is taken, and the flag comes with it
    envs["five"].set_view_training(False)
    envs["five"].restore(snaps["five"])
    moved = envs["five"].view_statistics()["count"].copy()
    envs["five"].step(gpu.index_actions(n, steps=1)[0])
    assert (envs["five"].view_statistics()["count"] == moved + n).all()
    _close(*envs.values())


# ---- 6: what the library refuses --------------------------------------------------------------------------------------
def test_abi_refusals_change_nothing(monkeypatch):
    n = 65
    _, off = _composed(n, monkeypatch=monkeypatch, host=False)
    _, on = _composed(n, monkeypatch=monkeypatch, host=False, learner_view=_view())  # (no records)
    _, host_init = _composed(n, monkeypatch=monkeypatch, host=False, device_initializer=False, learner_view=_view())
    lib = _native.load()
    with pytest.raises(AssertionError, match="no learner view"):
        off._ctx.env_view()
    with pytest.raises(AssertionError, match="no learner view"):
        off._ctx.env_view_statistics()
    with pytest.raises(AssertionError, match="no learner view"):
        off._ctx.env_view_set_training(False)
    off._ctx._env_view_stack = STACK
    with pytest.raises(AssertionError, match="no learner view"):
        off._ctx.env_view_state()
    with pytest.raises(AssertionError, match="rf_env_reset first"):
        on._ctx.env_view(rewards=False)
    # a bad configuration: refused, and the context keeps the view it has
    good = dict(frame_stack=STACK, norm_obs=1, norm_reward=1, training=1, gamma=0.99, epsilon=1e-8, clip_obs=10.0,
                clip_reward=10.0)
    for bad, match in ((dict(frame_stack=0), "frame_stack"), (dict(frame_stack=9), "frame_stack"),
                       (dict(epsilon=0.0), "epsilon"), (dict(epsilon=float("nan")), "epsilon"),
                       (dict(clip_obs=float("inf")), "clip_obs"), (dict(clip_reward=-1.0), "clip_reward"),
                       (dict(gamma=1.5), "gamma"), (dict(gamma=float("nan")), "gamma")):
        config = _native.EnvViewConfig(**{**good, **bad})
        assert lib.rf_env_configure_view(on._ctx._h, config) == _native.RF_ERR_INVALID
        assert match in lib.rf_last_error().decode()
    on.reset(), off.reset(), host_init.reset()
    with pytest.raises(AssertionError, match="no step since the last reset"):
        on._ctx.env_view()
    with pytest.raises(AssertionError, match="needs episode records"):
        on._ctx.env_view(final=True)
    actions = gpu.index_actions(n, steps=3)
    for env in (off, on, host_init):
        env.step(actions[0])
    # rf_env_configure_view after a step: refused either way
    for env, config in ((off, _native.EnvViewConfig(**good)), (on, None), (on, _native.EnvViewConfig(**good))):
        seen = gpu._probe(env)
        with pytest.raises(AssertionError, match="has stepped"):
            env._ctx.env_configure_view(config)
        assert _same(gpu._probe(env), seen)
    # the two-phase and planned forms: refused while a view is configured, nothing changes
    seen, view = gpu._probe(host_init), _seen(host_init)
    ctx = host_init._ctx
    pool = np.zeros((n, 2), dtype=np.float32)
    for call in (lambda: ctx.env_step_begin(actions[1]), lambda: ctx.env_step_plan(actions[1]),
                 lambda: ctx.env_step_end(pool), lambda: ctx.env_step_run(pool),
                 lambda: ctx.env_render_states(np.full((2, 2), 7.0, dtype=np.float32))):
        with pytest.raises(AssertionError, match="learner view"):
            call()
    assert _same((gpu._probe(host_init), _seen(host_init)), (seen, view))
    assert sorted(on.step(actions[2])[4]) == ["raw_observation", "raw_reward"] and off.step(actions[2])[4] == {}
    host_init.step(actions[2])  # (all three still step)
    # a NULL context, and the exports
    assert lib.rf_env_configure_view(None, None) == _native.RF_ERR_INVALID
    assert lib.rf_env_get_view(None, None, None, None) == _native.RF_ERR_INVALID
    assert lib.rf_env_view_set_training(None, 1) == _native.RF_ERR_INVALID
    assert lib.rf_abi_version() == 1
    _close(off, on, host_init)


def test_records_after_the_view_turn_it_off(monkeypatch):
    """rf_env_configure_records, like every rf_env_configure*, turns the view off: records are asked for first."""
    _, dev = _composed(3, monkeypatch=monkeypatch, host=False, learner_view=_view())
    dev._ctx.env_configure_records(True)
    with pytest.raises(AssertionError, match="no learner view"):
        dev._ctx.env_view_statistics()
    _close(dev)


def test_single_and_sharded_environments_refuse_a_view():
    with pytest.raises(ValueError, match="sharded"):
        harness.ShardedVectorDiscreteSteps(num_envs=4, devices=[0, 0], frame_height=16, samples_per_pixel=2,
                                           learner_view=_view())
    with pytest.raises(ValueError, match="single-environment"):
        harness.DiscreteSteps(frame_height=16, samples_per_pixel=2, learner_view=_view())
