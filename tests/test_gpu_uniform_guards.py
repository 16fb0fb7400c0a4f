"""The three per-lane tests of the render loop that are decided per block or per wave where that is possible:
  * unit_dir_y's length-range test, replaced by the per-environment flag PixelEnv::dir_fast (rf_math.h);
  * disc_tails_wave's `slot < end of the wave's slots`, decided by the wave's straggler count (rf_coop2.h);
  * park()'s `slot < end of the list` of coop_finish2m's one-atomic-per-wave form, decided by the wave's range of slots.
Frames and final RNG states must equal the oracle's whichever side of each decision a block or wave is on: with scene
constants on both sides of every threshold of the flag, and -- for the two slot tests, whose per-lane form the product
capacities practically never reach -- on tests/gpucheck's build with a 32-entry list and 8 disc slots per wave, for scenes
of which the oracle alone says that they hold fitting and overflowing waves side by side."""
import functools
import re

import numpy as np
import pytest

from tests import helpers
from tests.test_gpu_parity import _render_in_child, ctx, native  # noqa: F401  (fixtures; the child that loads another build)

pytestmark = pytest.mark.gpu

F = np.float32


# --- the range flag ------------------------------------------------------------------------------------------------


def _flag_scenes():
    """Three groups of four environments: the default scene with raw camera constants replaced so that they sit on both
    sides of every threshold of dir_fast -- |llz| at 2^-49 and 2^48, the x and the y bound at 2^48 -- and non-finite ones."""
    up = np.nextafter(F(2.0 ** 48), F(np.inf))
    groups = {}
    base = helpers.pack_scene(np.array([7.0, 8.0, 6.5, 9.0], dtype=F), np.array([7.0, 6.0, 9.0, 9.0], dtype=F))

    def scene(edits, miss_by_t=()):
        dyn = np.array(base[0], dtype=F, copy=True)
        rect = np.array(base[1], dtype=F, copy=True)
        for e, (row, col, value) in enumerate(edits):
            if row is not None:
                dyn[e, row, col] = value
        for e in miss_by_t:
            rect[e, 1] = -rect[e, 1]  # the target behind the camera: t < 0.001, every ray misses (rectangle.py:130)
        return (dyn, rect) + tuple(base[2:])

    # lower_left.z: flag at -2^-49 and -2^48, none at -2^-50 and -2^49
    groups["z"] = scene([(0, 2, F(-2.0 ** -49)), (0, 2, F(-2.0 ** -50)), (0, 2, F(-2.0 ** 48)), (0, 2, F(-2.0 ** 49))])
    # horizontal.x / vertical.y: |ll| + extent + r <= 2^48 holds with the extent one ulp below 2^48 - |ll| ... and fails at
    # 2^48 + ulp (ll stays the default scene's few units, the lens radius 0.05: both vanish in the float sum)
    groups["xy"] = scene([(1, 0, F(2.0 ** 48)), (1, 0, up), (2, 1, F(2.0 ** 48)), (2, 1, up)])
    # non-finite constants (flag off: the guarded form has to give what it always gave), next to an untouched environment.
    # The NaN environment's rays all miss by their t range: a NaN that reaches a HIT's checker coordinates is coloured
    # differently by the kernels and by the oracle -- in the parent of this change too; nothing that the flag touches.
    groups["nonfinite"] = scene([(0, 0, F(np.nan)), (0, 0, F(np.inf)), (2, 1, F(-np.inf)), (None, None, None)], miss_by_t=(0,))
    return groups


@pytest.mark.parametrize("group", ["z", "xy", "nonfinite"])
def test_range_flag_on_both_sides_of_every_threshold(ctx, oracle, group):
    dyn, rect, origin, u, v, lens = _flag_scenes()[group]
    n, h, w, spp = 4, 128, 128, 3
    st = oracle.seed_states(n * h * w, 0)
    want = oracle.render(dyn, rect, h, w, spp, st, n_threads=8)
    ctx.seed(n * h * w, 0, 0)
    ctx.set_scene(dyn, rect, origin, u, v, lens)
    got = ctx.render(n, h, w, spp, to_host=True)
    for e in range(n):
        assert np.array_equal(got[e], want[e]), (group, e, dyn[e].tolist())
    assert np.array_equal(ctx.get_states(0, n * h * w), st)


# --- the slot tests: product capacities ----------------------------------------------------------------------------

DEFAULT = (np.array([8.0], dtype=F), np.array([8.0], dtype=F))
# a target of about 10 x 10 pixels in the middle of a 64 x 64 frame: ~107 hits per sample, 0.476 of them sphere stragglers
SMALL = dict(targets=np.array([9.0], dtype=F), focus=np.array([9.0], dtype=F), r_size=5.0)


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "256":
        return helpers.pack_scene(*DEFAULT), 256, 256, 4
    if name == "64":
        return helpers.pack_scene(SMALL["targets"], SMALL["focus"], r_size=SMALL["r_size"]), 64, 64, 4
    assert name == "8x64"
    return helpers.pack_scene(SMALL["targets"], SMALL["focus"], r_size=SMALL["r_size"]), 64, 8, 4


@functools.lru_cache(maxsize=None)
def _want(name):
    """(frames, final states) of the oracle: computed once, shared, never written to."""
    from oracle import oracle as orc

    orc.build()
    d, h, w, spp = _case(name)
    st = orc.seed_states(h * w, 0)
    frames = orc.render(d[0], d[1], h, w, spp, st, n_threads=8)
    frames.setflags(write=False)
    st.setflags(write=False)
    return frames, st


@pytest.mark.parametrize("name", ["256", "64"])
def test_product_library_parks_by_wave(ctx, oracle, name):
    """256 x 256 with the default scene: the tiles inside the target park more than 200 stragglers per sample (0.476 of
    768 hit pixels), waves take their slots with one atomic and every range ends within the 256-entry list or beyond it;
    64 x 64: partial tiles, waves with nothing to park."""
    d, h, w, spp = _case(name)
    want, st = _want(name)
    ctx.seed(h * w, 0, 0)
    ctx.set_scene(*d)
    assert np.array_equal(ctx.render(1, h, w, spp, to_host=True), want)
    assert np.array_equal(ctx.get_states(0, h * w), st)


# --- the slot tests: the overflow build ----------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _straggler_flags(name):
    """Per sample and pixel, from the oracle's own functions alone: was the first disc attempt rejected, was the ray a
    hit, was the first sphere attempt of a hit rejected.  (The draws of a sample are: two for the jitter, two per disc
    attempt, three per sphere attempt of a hit -- the oracle's sequence is the kernels'.)  The states the walk ends with
    are the oracle renderer's final states, which checks the walk."""
    from oracle import oracle as orc

    orc.build()
    d, h, w, spp = _case(name)
    dyn, rect = np.asarray(d[0], dtype=F).reshape(9), np.asarray(d[1], dtype=F).reshape(2)
    cs = orc.cam_static(d[2], d[3], d[4], d[5])
    states = orc.seed_states(h * w, 0)
    disc = np.zeros((spp, h, w), dtype=bool)
    hit = np.zeros((spp, h, w), dtype=bool)
    sphere = np.zeros((spp, h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            st = states[y * w + x]
            for k in range(spp):
                s = F((x + float(orc.uniform_float(st))) / w)
                t = F((y + float(orc.uniform_float(st))) / h)
                probe = st.copy()
                orc.next_u64(probe), orc.next_u64(probe)
                o, direction = orc.get_ray(dyn, cs, s, t, st)
                disc[k, y, x] = not np.array_equal(probe, st)  # more than one attempt's draws were taken
                is_hit, _ = orc.fast_hit(rect, o, direction, 0.001, 1000000.0)
                hit[k, y, x] = is_hit
                if is_hit:
                    probe = st.copy()
                    orc.next_u64(probe), orc.next_u64(probe), orc.next_u64(probe)
                    orc.random_in_unit_sphere(st)
                    sphere[k, y, x] = not np.array_equal(probe, st)
    assert np.array_equal(states, _want(name)[1]), "the walk took other draws than the oracle's renderer"
    return disc, hit, sphere


def _per_wave(flags, wx, ww):
    """Sums of `flags` [spp, h, w] over the pixels of every wave of render_kernel_coop2<.., WX, WW>: [spp, blocks, 4].  A
    block's tile is WX waves of WW x 64 / WW pixels side by side, 4 / WX down, three sets below each other."""
    spp, h, w = flags.shape
    wave_h = 64 // ww
    tile_w, tile_h = wx * ww, (4 // wx) * wave_h
    all_h = 3 * tile_h
    tiles_x, tiles_y = -(-w // tile_w), -(-h // all_h)
    out = np.zeros((spp, tiles_x * tiles_y, 4), dtype=np.int64)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            for wave in range(4):
                col0 = tx * tile_w + (wave % wx) * ww
                for j in range(3):
                    row0 = ty * all_h + j * tile_h + (wave // wx) * wave_h
                    out[:, ty * tiles_x + tx, wave] += flags[:, row0:row0 + wave_h, col0:col0 + ww].sum(axis=(1, 2))
    return out


CAP32_LIST, CAP32_DISC_SLOTS, ADAPT_ON = 32, 8, 32  # tests/gpucheck/Makefile: RF_COOP_CAP, RF_DISC_WAVE_SLOTS; rf_coop2.h kAdaptOn


@pytest.mark.parametrize("name", ["256", "64", "8x64"])
def test_overflow_build_decides_per_wave_and_per_lane(kernel_choice, oracle, tmp_path, name):
    """tests/gpucheck's build with a 32-entry list and 8 disc slots per wave: the scalar decisions come out both ways, and
    where they say "does not fit" the per-lane tests run -- in almost every sample."""
    so = helpers.built("tests/gpucheck", "libreinfocus_cap32.so")
    d, h, w, spp = _case(name)
    want, st = _want(name)
    frames, final, kernel = _render_in_child(tmp_path, d, 1, h, spp, {"REINFOCUS_HIP_LIB": so}, w=w, want_kernel=True)
    assert np.array_equal(frames, want), kernel
    assert np.array_equal(final, st), kernel
    m = re.match(r"render_kernel_coop2<true, \d, (\d+), (\d+)", kernel)
    if name == "256" or not m:  # (the counts below are of the cooperative kernel's waves; 256 x 256 is too many pixels to walk)
        return
    disc, hit, sphere = _straggler_flags(name)
    wx, ww = int(m.group(1)), int(m.group(2))
    disc_w, sphere_w = _per_wave(disc, wx, ww), _per_wave(sphere, wx, ww)
    if name == "8x64":
        # disc_tails_wave: a wave's stragglers fit iff there are at most 8 of them.  Eight columns are 48 live pixels per
        # wave of 32 x 2 pixels x 3 sets, 0.2146 of which reject their first disc attempt: 10.3 on average.
        live = disc_w[disc_w > 0]
        fitting, overflowing = int((live <= CAP32_DISC_SLOTS).sum()), int((live > CAP32_DISC_SLOTS).sum())
        print("disc stragglers per wave-sample: fitting", fitting, "overflowing", overflowing, "max", int(live.max()))
        assert fitting >= 5 and overflowing >= 5, (fitting, overflowing)
        return
    # coop_finish2m: the waves of a block take ranges of the 32-entry list in the order of their atomics.  A block-sample
    # whose waves have at most 32 stragglers each but more than 32 together holds both: the wave that comes first fits
    # whichever it is, and the wave whose range crosses the list's end does not.  (No block-sample may have more than
    # 32 + kAdaptOn stragglers, or the block would make two in-wave attempts in the next sample and these counts -- of
    # the first attempt -- would not be the kernel's.)
    per_block = sphere_w.sum(axis=2)
    assert per_block.max() <= CAP32_LIST + ADAPT_ON, per_block.max()
    mixed = (per_block > CAP32_LIST) & (sphere_w.max(axis=2) <= CAP32_LIST)
    only_fitting = (per_block > 0) & (per_block <= CAP32_LIST)
    print("sphere stragglers per block-sample: mixed", int(mixed.sum()), "all fitting", int(only_fitting.sum()),
          "max per block", int(per_block.max()), "max per wave", int(sphere_w.max()), "hits", int(hit.sum()))
    assert mixed.sum() >= 2 and only_fitting.sum() >= 2, (int(mixed.sum()), int(only_fitting.sum()))
    # disc tails at 64 x 64: 128 or 192 live pixels per wave, practically every wave overflows its 8 slots
    assert (disc_w[disc_w > 0] > CAP32_DISC_SLOTS).mean() > 0.95
