"""GPU tests of composed environments with an observer tree (rf_env_configure_observed):
harness.DeviceVectorEnvironment(observer=...) against its numpy-glue twin harness.VectorEnvironment(observer=...) bit for
bit on every schedule of the step -- observations float32[n, W], float64 rewards, flags, states, per-leaf strategy state,
the DeltaObservers' old values (NaN equal), initializer consumption and the schedule taken -- for four hand-written
trees and for the seeded random trees of tests/golden/observer_program_cases.json (widths 1 to 16) at environment counts
that are not multiples of 64; the restated default tree against the built-in observer and DiscreteSteps at the
benchmark's shape; contexts with and without an observer program side by side; what the library refuses; the
visualiser with focus_observation_index."""

import ctypes
import json
import os

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import episode_ender as ee
from reinfocus_amd.environments import episode_rewarder as er
from reinfocus_amd.environments import state_initializer as si
from reinfocus_amd.environments import state_observer as so
from reinfocus_amd.environments import state_transformer as st
from reinfocus_amd.environments import strategy_program as sp
from tests import observer_programs as op
from tests.test_composed_env_logic import ACTION_SET, ENDS, discrete_steps
from tests.test_gpu_environment import BRANCH_NAME, FIRST_STEP_BRANCH, STEP_BRANCHES

pytestmark = pytest.mark.gpu

TREES = [c["spec"] for c in json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                                        "observer_program_cases.json")))["cases"]]


def _renderer(spp):
    from reinfocus_amd.graphics import render

    return render.FastRenderer(samples_per_pixel=spp, device=0)


def _tree(name, n, renderer, height):
    """Fresh observer objects of tree `name` around a FocusObserver on `renderer`."""
    from reinfocus_amd.environments import harness

    if name == "default":
        return harness.default_observer(n, ENDS, 5.0, renderer, height)
    focus = so.FocusObserver(n, 0, 1, ENDS, renderer, height)
    target, position = so.IndexedElementObserver(n, 0, *ENDS), so.IndexedElementObserver(n, 1, *ENDS)
    if name == "no delta":
        return so.NormalizedObserver([target, position, focus])
    if name == "raw delta":
        return so.DeltaObserver([position, focus], include_original=False)
    assert name == "delta of delta"  # 3 -> 6 -> 12 columns, 3 + 6 old-value rows
    return so.NormalizedObserver(so.DeltaObserver(so.DeltaObserver([target, position, focus], True), True, 2.5))


def _strategies(n, width, seed, max_steps=6):
    """A composition whose rewarder reads the last observation column (and column 5 of a tree that has one)."""
    rewarder = er.DeltaRewarder(1, 0.5) + er.ObservationRewarder(width - 1) * er.OnTargetRewarder((0, 1), 0.25, 0.5, 2.0)
    if width > 5:
        rewarder = rewarder + er.ObservationRewarder(5)
    return dict(ender=ee.TimeLimitEnder(n, max_steps) | ee.DivergingEnder(n, (0, 1), 0.125, 2),
                initializer=si.RangedInitializer([[ENDS], [ENDS]], seed=seed), rewarder=rewarder,
                transformer=st.DiscreteMoveTransformer(n, 1, ENDS, ACTION_SET), num_envs=n)


def _same_step(got, want):
    for x, y in zip(got[:4], want[:4]):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


def _same_state(host, dev):
    assert np.array_equal(host._state, dev._state)
    for x, y in zip(dev.strategy_state(), host.strategy_state()):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    x, y = dev.observer_state(), host.observer_state()
    assert x.dtype == y.dtype == np.float32 and x.shape == y.shape and np.array_equal(x, y, equal_nan=True)


def _pair(make_tree, n, height, spp, branch, monkeypatch, seed=13):
    """(host twin, device environment, the device tree's renderer) of the same composition around fresh trees."""
    from reinfocus_amd.environments import harness

    host_tree = make_tree(_renderer(spp))
    width = host_tree.single_observation_space.shape[0]
    plotted = dict(focus_observation_index=min(1, width - 1))  # (a tree of one column has no column 1)
    host = harness.VectorEnvironment(**_strategies(n, width, seed), observer=host_tree, **plotted)
    described = _renderer(spp)
    for key, value in STEP_BRANCHES[branch].items():
        monkeypatch.setenv(key, value)
    dev = harness.DeviceVectorEnvironment(**_strategies(n, width, seed), observer=make_tree(described), **plotted)
    for key in STEP_BRANCHES[branch]:
        monkeypatch.delenv(key)
    assert dev._shard.frame_height == height and dev._shard.samples_per_pixel == spp
    for name in ("single_observation_space", "observation_space"):
        a, b = getattr(host, name), getattr(dev, name)
        assert a.shape == b.shape and np.array_equal(a.low, b.low) and np.array_equal(a.high, b.high)
    return host, dev, described, width


def _against_twin(make_tree, n, height, spp, steps, branch, monkeypatch):
    """The device environment against its host twin after the reset and every step; the environments that ended."""
    host, dev, described, width = _pair(make_tree, n, height, spp, branch, monkeypatch)
    o_h, _ = host.reset()
    o_d, _ = dev.reset()
    assert o_d.dtype == np.float32 and o_d.shape == (n, width) and np.array_equal(o_h, o_d)
    _same_state(host, dev)
    rng = np.random.default_rng(6)
    name_b = BRANCH_NAME.get(branch, branch)
    resets = 0
    for step in range(steps):
        actions = rng.integers(0, 13, n)
        want = host.step(actions)
        got = dev.step(actions)
        _same_step(got, want)
        assert got[0].dtype == np.float32 and got[0].shape == (n, width) and got[1].dtype == np.float64
        _same_state(host, dev)
        assert host._initializer._generator.bit_generator.state == dev._initializer._generator.bit_generator.state
        assert dev._ctx.env_last_step_branch() == (FIRST_STEP_BRANCH.get(name_b, name_b) if step == 0 else name_b)
        resets += int(want[3].sum())
    host.close()
    dev.close()
    described.close()
    return resets


@pytest.mark.parametrize("branch", list(STEP_BRANCHES))
@pytest.mark.parametrize("n,height,spp,steps", [(64, 32, 4, 20), (300, 24, 2, 16)])
@pytest.mark.parametrize("name", ["default", "no delta", "raw delta", "delta of delta"])
def test_device_step_equals_host_twin(name, n, height, spp, steps, branch, monkeypatch):
    resets = _against_twin(lambda renderer: _tree(name, n, renderer, height), n, height, spp, steps, branch, monkeypatch)
    assert resets > 0


@pytest.mark.parametrize("branch", list(STEP_BRANCHES))
def test_random_trees_equal_the_host_twin(branch, monkeypatch):
    """Every tree of the numpy-1.26 fixture on every schedule, at 1, 63, 65 and 130 environments in turn."""
    resets = 0
    for i, spec in enumerate(TREES):
        n = (1, 63, 65, 130)[i % 4]

        def make_tree(renderer, n=n, spec=spec):
            return op.build(spec["tree"], n, so.FocusObserver(n, 0, 1, ENDS, renderer, 16))

        resets += _against_twin(make_tree, n, 16, 1, 9, branch, monkeypatch)
    assert resets > 0


def test_restated_default_tree_equals_the_built_in_observer_at_the_headline_shape():
    """4096 environments of 256 x 256 pixels at 16 samples (bench.py's shape), a few steps with auto-resets: the
    default tree against DeviceVectorEnvironment(observer=None) and DeviceVectorDiscreteSteps."""
    from reinfocus_amd.environments import harness

    n = 4096
    kw = dict(frame_height=256, samples_per_pixel=16, device=0)
    task_env = harness.DeviceVectorDiscreteSteps(max_episode_steps=2, num_envs=n, seed=4, **kw)
    built_in = harness.DeviceVectorEnvironment(**discrete_steps(n, 2, seed=4), **kw)
    described = _renderer(16)
    observed = harness.DeviceVectorEnvironment(**discrete_steps(n, 2, seed=4),
                                               observer=harness.default_observer(n, ENDS, 5.0, described, 256))
    want = task_env.reset()[0]
    assert np.array_equal(want, built_in.reset()[0]) and np.array_equal(want, observed.reset()[0])
    rng = np.random.default_rng(0)
    for _ in range(4):
        actions = rng.integers(0, 13, n)
        want = task_env.step(actions)
        _same_step(built_in.step(actions), want)
        _same_step(observed.step(actions), want)
        assert np.array_equal(task_env._state, observed._state)
        assert observed._ctx.env_last_step_branch() == built_in._ctx.env_last_step_branch()
    assert want[3].all()  # (the time limit ended every environment in the last step)
    for env in (task_env, built_in, observed, described):
        env.close()


def test_contexts_with_and_without_an_observer_program_side_by_side(monkeypatch):
    """A DiscreteSteps context, a composed one with the built-in observer and one with a 12-column tree, stepped
    alternately in one process, each equal their twin."""
    from reinfocus_amd.environments import harness

    n = 40
    kw = dict(frame_height=24, samples_per_pixel=3, device=0)
    d_host = harness.VectorDiscreteSteps(max_episode_steps=6, num_envs=n, seed=1, **kw)
    d_dev = harness.DeviceVectorDiscreteSteps(max_episode_steps=6, num_envs=n, seed=1, **kw)
    c_host = harness.VectorEnvironment(**discrete_steps(n, 5, seed=2), **kw)
    c_dev = harness.DeviceVectorEnvironment(**discrete_steps(n, 5, seed=2), **kw)
    o_host, o_dev, described, width = _pair(lambda renderer: _tree("delta of delta", n, renderer, 24), n, 24, 3,
                                            "fused-graph", monkeypatch)
    assert width == 12 and o_dev._ctx._env_obs_width == 12 and c_dev._ctx._env_obs_width == 4
    for host, dev in ((d_host, d_dev), (c_host, c_dev), (o_host, o_dev)):
        assert np.array_equal(host.reset()[0], dev.reset()[0])
    rng = np.random.default_rng(9)
    for _ in range(14):
        for host, dev in ((d_host, d_dev), (o_host, o_dev), (c_host, c_dev)):
            actions = rng.integers(0, 13, n)
            _same_step(dev.step(actions), host.step(actions))
            assert np.array_equal(host._state, dev._state)
        _same_state(o_host, o_dev)
    with pytest.raises(AssertionError, match="rf_env_configure_observed first"):
        c_dev._ctx.env_observer_state()
    with pytest.raises(AssertionError, match="not given an observer"):
        c_dev.observer_state()
    for env in (d_host, d_dev, c_host, c_dev, o_host, o_dev, described):
        env.close()


def _changed(program, **changes):
    """A copy of an observer program with fields set: n_nodes=..., or node3=dict(first=...)."""
    bad = type(program).from_buffer_copy(program)
    for key, value in changes.items():
        if key.startswith("node"):
            for field, v in value.items():
                if field in ("mid", "scale"):
                    getattr(bad.nodes[int(key[4:])], field)[v[0]] = v[1]
                else:
                    setattr(bad.nodes[int(key[4:])], field, v)
        else:
            setattr(bad, key, value)
    return bad


def test_library_refuses_malformed_observer_programs_and_changes_nothing(monkeypatch):
    n = 12
    host, dev, described, width = _pair(lambda renderer: _tree("default", n, renderer, 16), n, 16, 2, "fused", monkeypatch)
    assert np.array_equal(host.reset()[0], dev.reset()[0])
    rng = np.random.default_rng(1)
    for _ in range(3):
        actions = rng.integers(0, 13, n)
        _same_step(dev.step(actions), host.step(actions))
    program, good = sp.compile_program(**{k: v for k, v in _strategies(n, width, 0).items() if k != "initializer"},
                                       observer=_tree("default", n, described, 16))
    # nodes of the default tree: Indexed(1) at column 0, Focus at 1, Delta(0-1, with originals), Normalized(0-3)
    bad_programs = [
        _changed(good, n_nodes=0), _changed(good, n_nodes=17), _changed(good, node2=dict(kind=4)),
        _changed(good, node0=dict(index=2)), _changed(good, node1=dict(first=2)), _changed(good, node0=dict(width=2)),
        _changed(good, node2=dict(first=1, width=1)), _changed(good, node3=dict(width=3)),
        _changed(good, node3=dict(first=1, width=3)), _changed(good, node2=dict(old_first=1)),
        _changed(good, node0=dict(kind=_native.OBS_FOCUS)), _changed(good, node1=dict(kind=_native.OBS_INDEXED)),
        _changed(good, width=5), _changed(good, width=2), _changed(good, n_old=3),
        _changed(good, node3=dict(scale=(2, 0.0))), _changed(good, node3=dict(scale=(0, np.inf))),
        _changed(good, node3=dict(mid=(3, np.nan))),
    ]
    wide = _native.EnvObserverProgram()  # nine leaves, then a DELTA with originals: 18 columns
    wide.n_nodes, wide.width, wide.n_old = 10, 18, 9
    for k in range(9):
        wide.nodes[k].kind = _native.OBS_FOCUS if k == 0 else _native.OBS_INDEXED
        wide.nodes[k].first, wide.nodes[k].width = k, 1
    wide.nodes[9].kind, wide.nodes[9].first, wide.nodes[9].width, wide.nodes[9].include_original = _native.OBS_DELTA, 0, 9, 1
    bad_programs.append(wide)
    cfg = _native.EnvConfig()
    cfg.n = n
    lib = _native.load()
    for bad in bad_programs:  # (the library itself, past the binding's own check of the width)
        rc = lib.rf_env_configure_observed(dev._ctx._h, ctypes.byref(cfg), ctypes.byref(program), ctypes.byref(bad))
        assert rc == _native.RF_ERR_INVALID and lib.rf_last_error().decode().startswith("rf_env_configure_observed: ")
    with pytest.raises(AssertionError, match="18 observation columns"):
        dev._ctx.env_configure_observed(cfg, program, wide)
    with pytest.raises(AssertionError, match="rf_env_configure_observed: node 3"):
        dev._ctx.env_configure_observed(cfg, program, bad_programs[-2])
    beyond = type(program).from_buffer_copy(program)
    index = next(i for i in range(beyond.n_rewarders) if beyond.rewarders[i].kind == er.OBSERVATION)
    beyond.rewarders[index].index0 = width
    with pytest.raises(AssertionError, match=f"observation index {width} outside 0-{width - 1}"):
        dev._ctx.env_configure_observed(cfg, beyond, good)
    assert dev._ctx._env_obs_width == width
    for _ in range(8):  # (the context is as it was: it goes on equal to its twin, through auto-resets)
        actions = rng.integers(0, 13, n)
        _same_step(dev.step(actions), host.step(actions))
        _same_state(host, dev)
    for env in (host, dev, described):
        env.close()


def test_device_visualiser_plots_the_named_column():
    """render_mode="rgb_array" with the focus value in column 2: the same 600 px frames and status strings as the
    numpy-glue twin, and the plotted history is that column's."""
    from reinfocus_amd.environments import harness

    n = 4
    kw = dict(render_mode="rgb_array", focus_observation_index=2)
    described = _renderer(2)
    host = harness.VectorEnvironment(**_strategies(n, 3, 9), observer=_tree("no delta", n, _renderer(2), 32), **kw)
    dev = harness.DeviceVectorEnvironment(**_strategies(n, 3, 9), observer=_tree("no delta", n, described, 32), **kw)
    start = [[7.5, 7.5]] * n
    assert np.array_equal(host.reset(state=start)[0], dev.reset(state=start)[0])
    rng = np.random.default_rng(2)
    for _ in range(8):
        a, b = host.render(), dev.render()
        assert a.shape == b.shape and a.shape[0] % 600 == 0
        assert np.array_equal(a[:, :600], b[:, :600])
        actions = rng.integers(0, 13, n)
        want = host.step(actions)
        _same_step(dev.step(actions), want)
        assert [host.status(i) for i in range(n)] == [dev.status(i) for i in range(n)]
        assert host._visualizer._columns["value"] == dev._visualizer._columns["value"] == 2
        assert np.array_equal(host._visualizer._focus_histories.data, dev._visualizer._focus_histories.data, equal_nan=True)
        newest = host._visualizer._focus_histories.data[:, -1]
        assert np.array_equal(newest, want[0][:, 2])
    host.close()
    dev.close()
    described.close()
