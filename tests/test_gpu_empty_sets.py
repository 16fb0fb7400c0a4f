"""GPU parity where whole pixel sets and whole waves of render_kernel_coop2 have nothing to do.

A thread of the cooperative kernel owns three pixels (sets); the sample loop may skip, per wave, work that no lane of the
wave can use (rf_coop2.h: a wave without stragglers does not rank and park, ...).  These cases put such waves and sets
where the usual square test frames have few: tile rows that the frame's height cuts after 1 .. 5 rows (whole sets below
the frame), a width that leaves whole waves beside it, scenes in which no wave ever hits the target or every wave does,
and the environment step's two-pass form at a ragged height.  Frames AND final RNG states equal the oracle's, and every
case checks through render_kernel_name that the cooperative kernel rendered it (the session forces it at every size:
tests/conftest.py)."""

import re

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from reinfocus_amd import _native

    assert _native.device_count() >= 1, "no GPU visible: the HIP path cannot run"
    return _native


@pytest.fixture()
def ctx(native):
    c = native.Context(0)
    yield c
    c.close()


def _tile_of(kernel):
    """(tile width, set height, wave width) of the 'render_kernel_coop2<POW2, LENS, WX, WW[, true]>' that rendered: WX
    waves of WW x 64 / WW pixels side by side, 4 / WX down; a thread's three sets lie one set height apart."""
    m = re.match(r"render_kernel_coop2<(?:true|false), \d, (\d), (\d+)(?:, true)?>$", kernel)
    assert m, f"not the cooperative kernel: {kernel}"
    wx, ww = int(m.group(1)), int(m.group(2))
    return wx * ww, (4 // wx) * (64 // ww), ww


def _render_and_compare(ctx, oracle, scene, n, h, w, spp, passes=2):
    dyn, rect, origin, u, v, lens = scene
    st = oracle.seed_states(n * h * w, 0)
    ctx.seed(n * h * w, 0, 0)
    ctx.set_scene(dyn, rect, origin, u, v, lens)
    frames = []
    for _ in range(passes):  # (the second pass continues the streams the first one left)
        want = oracle.render(dyn, rect, h, w, spp, st, n_threads=8)  # (advances `st` in place)
        got = ctx.render(n, h, w, spp, to_host=True)
        assert np.array_equal(got, want)
        assert np.array_equal(ctx.get_states(0, n * h * w), st)
        frames.append(want)
    return frames, ctx.render_kernel_name()


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5])
def test_last_tile_row_cut_by_the_frame(ctx, oracle, rows):
    """256-pixel wide frames of 120 + rows rows: tiles of 128 x 6, the last tile row holds `rows` rows -- one set cut in
    the middle of its waves (odd counts), one or two sets wholly below the frame."""
    n, h, w, spp = 2, 120 + rows, 256, 3
    scene = helpers.pack_scene(*helpers.random_scene(np.random.default_rng(70 + rows), n))
    _, kernel = _render_and_compare(ctx, oracle, scene, n, h, w, spp)
    _, set_h, _ = _tile_of(kernel)
    assert h % (3 * set_h) == rows, (kernel, "the layout this case was written for has tiles of 6 rows")


def test_the_headline_height_leaves_a_dead_set(ctx, oracle):
    """256 x 256 (the power-of-two instance of the benchmark): 42 tile rows and 4 rows, set 2 of the last tile row dead."""
    n, h, w, spp = 2, 256, 256, 4
    scene = helpers.pack_scene(*helpers.random_scene(np.random.default_rng(256), n))
    _, kernel = _render_and_compare(ctx, oracle, scene, n, h, w, spp)
    assert kernel.startswith("render_kernel_coop2<true,"), kernel
    assert h % (3 * _tile_of(kernel)[1]) == 4, kernel


def test_whole_waves_beside_the_frame(ctx, oracle):
    """72 columns: the second tile column holds 8 of them, three of its four waves (side by side) are dead in every set;
    30 rows cut the last tile row as well."""
    n, h, w, spp = 3, 30, 72, 4
    scene = helpers.pack_scene(*helpers.random_scene(np.random.default_rng(72), n))
    _, kernel = _render_and_compare(ctx, oracle, scene, n, h, w, spp)
    tile_w, _, wave_w = _tile_of(kernel)
    assert 0 < w % tile_w <= tile_w - wave_w, (kernel, "no wave of the last tile column lies wholly beside the frame")


@pytest.mark.parametrize("h,w", [(64, 64), (61, 256)])
def test_no_pixel_hits_out_of_range(ctx, oracle, h, w):
    """rectangle.py:130: targets nearer than 0.001 and farther than 1e6 are missed by every ray (`tmiss`): no wave ever
    has a hit lane or a straggler of the sphere loop."""
    targets = np.array([0.0005, 2.0e6, 0.0002], dtype=np.float32)
    focus = np.array([10.0, 1.0, 5.0], dtype=np.float32)  # (t = target / focus distance)
    frames, kernel = _render_and_compare(ctx, oracle, helpers.pack_scene(targets, focus), len(targets), h, w, 4)
    _tile_of(kernel)
    assert all((f[..., 2] > 0).all() for f in frames), "a pixel without sky blue: something was hit"


@pytest.mark.parametrize("h,w", [(64, 64), (61, 256)])
def test_no_pixel_hits_a_target_out_of_view(ctx, oracle, h, w):
    """A target that is in range but subtends 1e-9 degrees: the hit test runs for every sample and fails for every one
    (the scene format centres every target, so `too small to be seen` is its only target out of view)."""
    n = 3
    targets, focus = helpers.random_scene(np.random.default_rng(9), n)
    frames, kernel = _render_and_compare(ctx, oracle, helpers.pack_scene(targets, focus, r_size=1e-9), n, h, w, 4)
    _tile_of(kernel)
    assert all((f[..., 2] > 0).all() for f in frames), "a pixel without sky blue: something was hit"


@pytest.mark.parametrize("h,w", [(64, 64), (61, 256)])
def test_target_fills_the_frame(ctx, oracle, h, w):
    """A target of 150 degrees: every sample of every pixel hits, every wave has stragglers, every block's list
    overflows (blue comes from missed samples only: there is none)."""
    n = 2
    targets, focus = helpers.random_scene(np.random.default_rng(15), n)
    frames, kernel = _render_and_compare(ctx, oracle, helpers.pack_scene(targets, focus, r_size=150), n, h, w, 4)
    _tile_of(kernel)
    assert all((f[..., 2] == 0).all() for f in frames), "a pixel with sky blue: a sample missed"


def test_two_pass_step_at_a_ragged_height(native, oracle, ctx):
    """The environment step renders the step's frames and the auto-reset's frames in ONE launch whose blocks make two
    passes (render_kernel_coop2<.., true>).  66 rows: tiles of 64 x 12, the last tile row holds 6 rows -- a set of four
    live rows, one cut after two, one dead -- and the second tile column 2 of 64 columns.  The plain render at this size
    equals the oracle (frames, RNG states); the device-resident environment, stepped through auto-resets, equals the
    host harness around that plain render observation by observation, and ends with the same RNG states."""
    from reinfocus_amd.environments import harness

    n, height, spp = 24, 66, 2
    scene = helpers.pack_scene(*helpers.random_scene(np.random.default_rng(66), n))
    _, kernel = _render_and_compare(ctx, oracle, scene, n, height, height, spp)
    _, set_h, _ = _tile_of(kernel)
    assert height % (3 * set_h) in range(1, 2 * set_h + 1), (kernel, "no set of the last tile row is dead")

    kw = dict(num_envs=n, frame_height=height, samples_per_pixel=spp, seed=11, device=0)
    host = harness.VectorDiscreteSteps(**kw)
    dev = harness.DeviceVectorDiscreteSteps(**kw)
    try:
        o_h, _ = host.reset()
        o_d, _ = dev.reset()
        assert np.array_equal(o_h, o_d)
        rng = np.random.default_rng(5)
        resets = 0
        for _ in range(40):
            actions = rng.integers(0, 13, n)
            oh, rh, th, ch, _info = host.step(actions)
            od, rd, td, cd, _info = dev.step(actions)
            assert np.array_equal(oh, od) and np.array_equal(rh, rd)
            assert np.array_equal(th, td) and np.array_equal(ch, cd)
            resets += int((th | ch).sum())
        assert resets > 0, "no auto-reset: the second pass never ran"
        name = dev._ctx.render_kernel_name()
        assert name.startswith("render_kernel_coop2<") and name.endswith(", true>"), name
        assert _tile_of(name)[1] == set_h, name
        count = n * height * height
        assert np.array_equal(dev._ctx.get_states(0, count), host._renderer._ctx.get_states(0, count))
    finally:
        host.close()
        dev.close()
