"""The focus kernels (reinfocus_amd/csrc/rf_focus.h) against an exact integer reference on hostile frames.

tests/focus_reference.py computes the chain gray -> median -> Laplacian -> sums in numpy integers from the OpenCV
definitions and the variance as the correctly rounded quotient of Python ints; tests/test_focus_reference.py holds it
against scipy, the C oracle and fractions.Fraction.  Its frame zoo -- ties in every median window, saturated rows and
columns, Laplacians on the clamp's edges, content at the frame's border only, blocks across every lane, wave, band and tile
boundary, one channel at a time -- goes up as the environments of one launch, shuffled, a constant frame in the middle.

The device takes its variance from exact integer sums (rf_math.h variance_from_sums): numerator N S2 - S1^2 and N^2 in
integers, then float64.  Where both are below 2^53 the conversions are exact and the division is the only rounding, so
the result must EQUAL the reference: every comparison here is == on float64 except the large frames of
test_two_limb_variance, whose bound is derived there.  No frame may leave the exact comparison silently: _check asserts
the condition for every frame it is handed.

The library reports which render kernel ran (rf_render_kernel_name) but offers nothing of the kind for the focus kernels;
which of them a case runs follows from the width rule in launch_focus (rf_abi_render.hip): focus_kernel_roll for widths
that are multiples of 4 and >= 8, with halo lanes iff 64 % (w / 4) != 0, else the byte-per-thread focus_kernel;
REINFOCUS_FOCUS_KERNEL=byte forces the latter, =quad takes focus_kernel_quad for multiples of 4 up to 936."""

import ctypes
import functools
import os
import re

import numpy as np
import pytest

from tests import focus_reference as fr
from tests import helpers
from tests.test_gpu_parity import FOCUS_SHAPES

pytestmark = pytest.mark.gpu

GRAY_MODES = [15, 14]


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


@functools.lru_cache(maxsize=None)
def _zoo(h, w):
    names, frames = fr.zoo_batch(h, w, fr.ZOO_SEED)
    frames.setflags(write=False)
    return names, frames


@functools.lru_cache(maxsize=None)
def _zoo_sums(h, w, mode):
    return fr.sums(_zoo(h, w)[1], mode)


def _check(got, names, sums, h, w, what):
    """Device variances equal the reference's, frame by frame; every frame must qualify for the exact comparison."""
    assert len(got) == len(names) == len(sums)
    bad = []
    for name, value, (s1, s2) in zip(names, got, sums):
        assert fr.is_exact_case(h * w, s1, s2), (what, h, w, name, "not below 2^53: == does not apply")
        want = fr.variance(h * w, s1, s2)
        if not value == want:
            bad.append((name, float(value), want))
    assert not bad, (what, h, w, bad)
    assert got[names.index(fr.CONSTANT)] == 0.0


def _check_zoo(c, h, w, mode, what):
    names, frames = _zoo(h, w)
    c.upload_frames(frames)
    _check(c.focus(len(names), h, w, mode), names, _zoo_sums(h, w, mode), h, w, what)


# --- a. every shape -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("gray_mode", GRAY_MODES)
@pytest.mark.parametrize("h,w", fr.exact_shapes(FOCUS_SHAPES))
def test_focus_equals_the_integer_reference(ctx, h, w, gray_mode):
    _check_zoo(ctx, h, w, gray_mode, "library's choice")


def test_the_new_shapes_are_what_their_names_say():
    s = fr.NEW_SHAPES
    roll = lambda h, w: w % 4 == 0 and w >= 8
    halo = lambda h, w: roll(h, w) and 64 % (w // 4) != 0
    for g in (2, 4, 8, 16, 32, 64):
        h, w = s[f"no_halo_{g}_lanes_per_row"]
        assert roll(h, w) and not halo(h, w) and w // 4 == g and all(h % band for band in (8, 16, 32, 64))
    assert sorted(w // 4 for (h, w) in s.values() if halo(h, w) and h == 37) == [62, 63, 65, 124]
    h, w = s["three_lanes_per_row_21_rows_of_bands_in_a_wave"]
    assert halo(h, w) and 62 // (w // 4) >= 20 and h // 8 >= 21
    assert {(h, w) for h in (1, 2, 3, 4, 5) for w in (8, 256)} <= set(s.values())
    assert {(h, w) for h in (15, 16, 17, 33) for w in (511, 513, 1025, 6, 7)} <= set(s.values())
    assert not any(roll(h, w) for h, w in s.values() if w in (511, 513, 1025, 6, 7))


# --- b. every band height, and the other two kernels ------------------------------------------------------------------


@pytest.mark.parametrize("band", range(1, 65))
def test_every_band_height(native, monkeypatch, band):
    """focus_kernel_roll walks band + 4 steps in trips of three: (band + 4) % 3 decides how many steps run past the band,
    bands below 4 are shorter than the pipeline, and how a wave's lanes fall onto bands and rows changes with every value."""
    monkeypatch.setenv("REINFOCUS_FOCUS_BAND", str(band))
    c = native.Context(0)
    try:
        for h, w in fr.BAND_SHAPES:
            _check_zoo(c, h, w, 15, f"band {band}")
    finally:
        c.close()


@pytest.mark.parametrize("kernel", ["byte", "quad"])
def test_the_other_kernels(native, monkeypatch, kernel):
    monkeypatch.setenv("REINFOCUS_FOCUS_KERNEL", kernel)
    takes = (lambda h, w: True) if kernel == "byte" else (lambda h, w: w % 4 == 0 and 4 <= w <= 936)
    c = native.Context(0)
    try:
        shapes = [s for s in fr.exact_shapes(FOCUS_SHAPES) + fr.BAND_SHAPES if takes(*s)]
        assert len(shapes) > 20
        for h, w in shapes:
            for mode in GRAY_MODES:
                _check_zoo(c, h, w, mode, kernel)
    finally:
        c.close()


# --- c. rf_step and the Python surface ----------------------------------------------------------------------------------


@pytest.mark.parametrize("n,h,w", fr.STEP_SHAPES)
def test_step_scores_the_frames_it_rendered(ctx, n, h, w):
    """rf_step's values are the variances of the frames that rf_step left in the frame buffer, exactly (whether those
    frames are the right ones is the render tests' business)."""
    scene = helpers.pack_scene(*helpers.random_scene(np.random.default_rng(h + w), n))
    ctx.seed(n * h * w, 0, 0)
    ctx.set_scene(*scene)
    for mode in GRAY_MODES:
        got = ctx.step(n, h, w, 2, mode)
        frames = ctx.get_frames((n, h, w))
        assert frames.any() and len({f.tobytes() for f in frames}) == n
        _check_values(got, frames, mode, h, w, "rf_step")


def _check_values(got, frames, mode, h, w, what):
    sums = fr.sums(frames, mode)
    assert all(fr.is_exact_case(h * w, s1, s2) for s1, s2 in sums), (what, h, w)
    want = [fr.variance(h * w, s1, s2) for s1, s2 in sums]
    assert list(got) == want, (what, h, w, list(got), want)


def test_vision_scores_device_and_host_frames_alike(native):
    from reinfocus_amd import vision
    from reinfocus_amd.graphics import render

    r = render.FastRenderer(samples_per_pixel=2, device=0)
    try:
        r.update_targets([10, 9, 8, 7, 6])
        r.update_focus_planes([40, 20, 10, 5, 1])
        handle = r.render(96)
        on_device = vision.focus_values(handle)
        host = np.asarray(handle)
        assert host.shape == (5, 96, 96, 3)
        from_host = vision.focus_values(host)
        assert all(isinstance(v, float) for v in on_device + from_host)
        assert on_device == from_host
        _check_values(on_device, host, vision.GRAY_MODE, 96, 96, "vision.focus_values")
        zoo_names, zoo = _zoo(33, 36)
        _check(vision.focus_values(zoo), zoo_names, _zoo_sums(33, 36, vision.GRAY_MODE), 33, 36, "vision.focus_values")
        assert vision.focus_value(zoo[0]) == vision.focus_values(zoo)[0]
    finally:
        r.close()
        vision.release()


# --- d. the ranges nobody had run on the device --------------------------------------------------------------------------


@pytest.mark.parametrize("h,w", fr.LARGE_SHAPES)
def test_two_limb_variance(ctx, h, w):
    """Frames of 1.3e8 pixels whose numerator N S2 - S1^2 is >= 2^64 (asserted), through focus_kernel_roll at band 64
    (w = 11500) and through the byte-per-thread kernel (w = 11501).  variance_from_sums then rounds more than once:

        hi = (double)(num >> 64)          exact: num < 2^16 N^2 < 2^70, so hi < 2^6
        lo = (double)(uint64)num          rounds iff lo has more than 53 significant bits
        hi * 2^64                         exact (a power of two)
        ... + lo                          rounds iff the sum of the two doubles needs more than 53 bits
        dn * dn                           rounds iff N^2 is not a float64 (N itself is: N < 2^53)
        ... / ...                         rounds

    The test evaluates the three conditions on the reference's integers and allows one ulp (of the reference value) for
    each rounding the operands do incur, k in all: at most 4, and 3 where N^2 = h^2 w^2 happens to be a float64.
    Derivation: a rounding is off by at most 2^-53 relative, which is at most one ulp of the quotient; the k - 1 roundings
    before the division therefore move the quotient it rounds by at most k - 1 ulp from the exact one (to first order:
    the second-order terms are 2^-53 of that), and two correctly rounded values of numbers k - 1 ulp apart -- the device's
    and the reference's -- are at most k ulp apart."""
    frames = np.stack(list(fr.adversarial_frames(h, w, fr.ZOO_SEED, names=fr.LARGE_NAMES).values()))
    n = h * w
    ctx.upload_frames(frames)
    got = ctx.focus(len(frames), h, w, 15)
    for name, value, (s1, s2) in zip(fr.LARGE_NAMES, got, fr.sums(frames, 15)):
        num = fr.numerator(n, s1, s2)
        assert num >= 2 ** 64, (name, "the frame no longer reaches the two-limb branch")
        hi, lo = num >> 64, num & (2 ** 64 - 1)
        lo_rounded = int(float(lo))
        roundings = (float(lo) != lo) + (int(float(hi * 2 ** 64 + lo_rounded)) != hi * 2 ** 64 + lo_rounded) \
            + (int(float(n * n)) != n * n) + 1
        assert 1 <= roundings <= 4
        want = fr.variance(n, s1, s2)
        apart = fr.ulps_apart(value, want)
        print(f"{name} {h}x{w}: numerator 2^{np.log2(float(num)):.3f}, {roundings} roundings, {apart} ulp apart")
        assert apart <= roundings, (name, float(value), want, apart, roundings)


def _free_device_memory():
    """hipMemGetInfo of the HIP runtime the library has loaded (the library has no entry point for it)."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert ctypes.CDLL(path).hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_frames_beyond_4_gib(ctx):
    """focus_row computes frame * row in 64 bits: 5470 rendered frames of 512 x 512 are 4.30e9 bytes, the last eight
    frames lie wholly beyond byte 2^32.  Rendered, not uploaded (1 sample per pixel); the first and the last four frames
    come back and are scored by the reference."""
    n, h, w = 5470, 512, 512
    per = h * w * 3
    assert (n - 4) * per >= 2 ** 32 and 4 * per < 2 ** 32
    need = n * per + n * h * w * 16 + (1 << 30)  # frames, one RNG state of 16 bytes per pixel, and room for the rest
    free = _free_device_memory()
    if free < need:
        pytest.skip(f"the device reports {free} bytes free, the frame buffer beyond 4 GiB and its RNG states need {need}")
    scene = helpers.pack_scene(*helpers.random_scene(np.random.default_rng(4), n))
    ctx.seed(n * h * w, 0, 0)
    ctx.set_scene(*scene)
    ctx.render(n, h, w, 1)
    got = ctx.focus(n, h, w, 15)
    assert got.shape == (n,) and np.all(np.isfinite(got))
    for first in (0, n - 4):
        frames = ctx.get_frames((n, h, w), first_env=first, n_envs=4)
        assert len({f.tobytes() for f in frames}) == 4
        _check_values(got[first:first + 4], frames, 15, h, w, f"frames {first} ... {first + 3}")


def test_saturated_rows_at_the_tallest_band(native, monkeypatch):
    """rows_1px at 256 x 256 and band 64: every second row of the chain is 255 throughout, the most a band can hold next
    to an all-white result (which no frame has: a saturated pixel needs darker neighbours).  Sixty-four lanes are one row
    of one band there, so a wave's sums are a band's.

    The comment on kRollBandMax states the bound "a lane's sum of squares stays below 2^32 / 64" (the wave's sum, which
    is what the kernel keeps in 32 bits after its reduction, then stays below 2^32).  Asserted from the reference: a
    wave's sum of squares exceeds half of that figure, 2^32 / 64 / 2.  In figures: 532 684 800 per wave (12.4 % of
    2^32), 8 323 200 per lane (12.4 % of 2^32 / 64).  Half of the 32 bits themselves is out of reach of ANY frame at
    kRollBandMax = 64: an all-255 band gives 64 * 4 * 255^2 = 16 646 400 per lane, 24.8 % -- the bound has a factor 4
    in hand, and this frame stands at exactly half of what arithmetic allows, which the test asserts as well."""
    h = w = 256
    band, groups = 64, w // 4
    text = open(os.path.join(helpers.ROOT, "reinfocus_amd", "csrc", "rf_focus.h")).read()
    m = re.search(r"constexpr int kRollBandMax = (\d+); // rows per band: a lane's sum of squares stays below 2\^32 / 64", text)
    assert m and int(m.group(1)) == band
    stated = 2 ** 32 // 64
    frame = fr.adversarial_frames(h, w, fr.ZOO_SEED, names=("rows_1px",))["rows_1px"]
    squares = fr.laplacian_of_frame(frame).astype(np.int64) ** 2
    assert 64 % groups == 0  # no halo lanes: wave k holds lanes 64 k ... 64 k + 63 of the (band, column group) order
    lanes = squares.reshape(h // band, band, groups, 4).sum(axis=(1, 3)).reshape(-1)  # [band * groups + group]
    waves = lanes.reshape(-1, 64).sum(axis=1)
    assert waves.max() < 2 ** 32 and lanes.max() < stated
    assert waves.max() > stated // 2
    assert waves.max() == 64 * lanes.max() == 64 * (band // 2) * 4 * 255 ** 2  # half of an all-white band, exactly

    monkeypatch.setenv("REINFOCUS_FOCUS_BAND", str(band))
    c = native.Context(0)
    try:
        names, frames = _zoo(h, w)
        assert np.array_equal(frames[names.index("rows_1px")], frame)
        for mode in GRAY_MODES:
            _check_zoo(c, h, w, mode, "band 64")
    finally:
        c.close()
