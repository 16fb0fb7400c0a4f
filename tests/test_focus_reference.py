"""The integer reference of the focus measure and its frame zoo (tests/focus_reference.py), checked where no GPU is needed:
against scipy stage by stage, against the C oracle on every frame the GPU tests launch, against fractions.Fraction for the
one division -- and the conditions tests/test_gpu_focus_exact.py relies on (which frames compare with ==, which frame
reaches the two-limb variance, what the zoo's frames are there for) evaluated on the frames themselves."""

import random
import re
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

from tests import focus_reference as fr
from tests.test_gpu_parity import FOCUS_SHAPES

STAGE_SHAPES = [(33, 35), (17, 100), (1, 9), (9, 1), (2, 2)]
LAPLACE = np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]])


@pytest.mark.parametrize("h,w", STAGE_SHAPES)
def test_stages_match_scipy(h, w):
    names, frames = fr.zoo_batch(h, w, fr.ZOO_SEED)
    for name, frame in zip(names, frames):
        for mode in (15, 14):
            g = fr.gray(frame, mode)
            assert g.shape == (h, w) and g.dtype == np.uint8
            med = fr.median3(g)
            assert np.array_equal(med, ndimage.median_filter(g, size=3, mode="nearest")), name  # BORDER_REPLICATE
            want = np.clip(ndimage.correlate(med.astype(np.int32), LAPLACE, mode="mirror"), 0, 255)  # BORDER_REFLECT_101
            lap = fr.laplacian_u8(med)
            assert np.array_equal(lap, want), name
            assert np.array_equal(fr.laplacian_of_frame(frame, mode), lap), name
            (s1, s2), = fr.sums(frame[None], mode)
            assert (s1, s2) == (int(want.sum()), int((want.astype(np.int64) ** 2).sum())), name


def test_gray_known_values():
    px = np.array([[[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [0, 0, 0]]], dtype=np.uint8)
    assert fr.gray(px, 15).tolist() == [[255, 76, 150, 29, 0]]
    assert fr.gray(px, 14).tolist() == [[255, 76, 150, 29, 0]]
    for v in (0, 1, 127, 128, 254, 255):  # (both sets of coefficients sum to one: equal channels keep their value)
        assert fr.gray(np.full((1, 1, 3), v, dtype=np.uint8), 15)[0, 0] == v
        assert fr.gray(np.full((1, 1, 3), v, dtype=np.uint8), 14)[0, 0] == v


def test_sums_do_not_depend_on_the_slices():
    for h, w in ((37, 20), (5, 8), (2, 9), (1, 12), (64, 5)):
        _, frames = fr.zoo_batch(h, w, fr.ZOO_SEED)
        whole = fr.sums(frames, 15, strip=h)
        for strip in (1, 2, 3, 7, 16):
            assert fr.sums(frames, 15, strip=strip) == whole, (h, w, strip)


@pytest.mark.parametrize("h,w", fr.exact_shapes(FOCUS_SHAPES))
def test_reference_matches_the_oracle(oracle, h, w):
    """Every frame of every shape of the exactness test, both gray modes.  The oracle sums in float64 (numpy's pairwise
    var()), so its own accuracy sets the bound: the one the oracle comparisons of tests/test_gpu_parity.py already use,
    1e-12 relative and 1e-12 absolute.  All of these shapes take the oracle milliseconds."""
    names, frames = fr.zoo_batch(h, w, fr.ZOO_SEED)
    for mode in (15, 14):
        want = oracle.focus_values(frames, mode)
        got = fr.variances(frames, mode)
        for name, g, o in zip(names, got, want):
            assert abs(g - o) <= 1e-12 + 1e-12 * abs(o), (name, mode, g, o)
        assert got[names.index(fr.CONSTANT)] == 0.0


def test_variance_is_the_correctly_rounded_quotient():
    rng = random.Random(5)
    cases = [(1, 0, 0), (1, 255, 65025), (2, 255, 65025), (4, 510, 130050), (3, 1, 1), (7, 3, 3)]
    for n in (1, 2, 9, 4096, 360000, 36_000_000, 132_250_000, 2 ** 31 - 1):
        cases += [(n, n * 255, n * 65025), (n, 0, 0), (n, (n // 2) * 255, (n // 2) * 65025), (n, 255, 65025), (n, 1, 1)]
        for _ in range(200):
            values = [rng.choice((0, 1, 254, 255, rng.randrange(256))) for _ in range(min(n, 64))]
            k = n // len(values)  # (n - k * len(values) further pixels of value 0)
            cases.append((n, k * sum(values), k * sum(v * v for v in values)))
    for n, s1, s2 in cases:
        exact = Fraction(n * s2 - s1 * s1, n * n)
        assert exact >= 0
        got = fr.variance(n, s1, s2)
        assert got == float(exact), (n, s1, s2)  # float(Fraction) rounds correctly as well, by another route
        if exact:  # and the rounding error is at most half a unit in the last place
            assert abs(Fraction(got) - exact) <= Fraction(float(np.spacing(got))) / 2
    assert fr.variance(4, 510, 130050) == 16256.25


def test_every_frame_of_the_exact_shapes_compares_with_equality():
    """tests/test_gpu_focus_exact.py compares with == wherever N S2 - S1^2 < 2^53 and N^2 < 2^53: that has to be every
    frame of every shape except the large ones.  (The largest, 600 x 600, has N^2 = 1.3e11 and, at the largest variance
    8-bit values have, 127.5^2, a numerator of 2.1e15 < 9.0e15.)"""
    for h, w in fr.exact_shapes(FOCUS_SHAPES) + fr.BAND_SHAPES + [s[1:] for s in fr.STEP_SHAPES] + [(256, 256)]:
        assert (h * w) ** 2 * 65025 < 4 * 2 ** 53, (h, w)  # (holds whatever the frames are)
        names, frames = fr.zoo_batch(h, w, fr.ZOO_SEED)
        for mode in (15, 14):
            for name, (s1, s2) in zip(names, fr.sums(frames, mode)):
                assert fr.is_exact_case(h * w, s1, s2), (h, w, name, mode)


@pytest.mark.parametrize("h,w", fr.LARGE_SHAPES)
def test_the_large_frames_reach_the_two_limb_variance(h, w):
    """(Half a minute each: 1.3e8 pixels twice.)"""
    frames = fr.adversarial_frames(h, w, fr.ZOO_SEED, names=fr.LARGE_NAMES)
    assert sorted(frames) == sorted(fr.LARGE_NAMES)
    for name, frame in frames.items():
        (s1, s2), = fr.sums(frame[None], 15)
        assert fr.numerator(h * w, s1, s2) >= 2 ** 64, (name, fr.numerator(h * w, s1, s2) / 2.0 ** 64)
        assert not fr.is_exact_case(h * w, s1, s2)
        assert s2 < 2 ** 64 and h * w * s2 < 2 ** 128


# --- the zoo is what it says ---------------------------------------------------------------------------------------------


def test_zoo_is_deterministic_and_shuffled():
    names, frames = fr.zoo_batch(33, 36, fr.ZOO_SEED)
    again_names, again = fr.zoo_batch(33, 36, fr.ZOO_SEED)
    assert names == again_names and np.array_equal(frames, again)
    assert sorted(names) == sorted(list(fr.GENERATORS) + [fr.CONSTANT]) and len(names) == 15
    assert names.index(fr.CONSTANT) == 7 and np.all(frames[7] == 77)
    assert names[:7] + names[8:] != list(fr.GENERATORS)
    other_names, other = fr.zoo_batch(33, 36, fr.ZOO_SEED + 1)
    assert not np.array_equal(frames[names.index("noise")], other[other_names.index("noise")])
    only = fr.adversarial_frames(33, 36, fr.ZOO_SEED, names=("two_level",))
    assert list(only) == ["two_level"] and np.array_equal(only["two_level"], frames[names.index("two_level")])
    assert len({f.tobytes() for f in frames}) == len(frames)


def test_rows_1px_saturates_whole_rows():
    h, w = 256, 256
    lap = fr.laplacian_of_frame(fr.adversarial_frames(h, w, fr.ZOO_SEED, names=("rows_1px",))["rows_1px"])
    full = [y for y in range(h) if np.all(lap[y] == 255)]
    assert full == list(range(1, h - 2, 2))  # every other row, 127 of them
    assert all(np.all(lap[y] == 0) for y in range(h) if y not in full)
    cols = fr.laplacian_of_frame(fr.adversarial_frames(h, w, fr.ZOO_SEED, names=("cols_1px",))["cols_1px"])
    assert np.array_equal(cols, lap.T)


def test_low_entropy_ties_in_the_median_windows():
    for mode in (15, 14):
        g = fr.gray(fr.adversarial_frames(64, 64, fr.ZOO_SEED, names=("low_entropy",))["low_entropy"], mode)
        p = np.pad(g, 1, mode="edge")
        windows = np.sort(np.stack([p[dy:dy + 64, dx:dx + 64] for dy in range(3) for dx in range(3)]), axis=0)
        tied = np.any(windows[1:] == windows[:-1], axis=0)
        assert tied.mean() >= 0.99
        assert np.mean(windows[3] == windows[4]) > 0.5  # ... and most of them at the median itself
        assert len(np.unique(g)) >= 3


def test_two_level_and_extremes_hold_what_they_claim():
    f = fr.adversarial_frames(64, 64, fr.ZOO_SEED)
    two = f["two_level"]
    assert set(np.unique(two)) == {0, 255} and np.array_equal(two[..., 0], two[..., 1]) and np.array_equal(two[..., 0], two[..., 2])
    raw = fr._laplacian_i32(fr.median3(fr.gray(two)))
    assert raw.min() <= -765 and raw.max() >= 765 and set(np.unique(fr.median3(fr.gray(two)))) == {0, 255}
    assert set(np.unique(f["extremes"])) == {0, 1, 127, 128, 254, 255}
    quads = f["extremes"].reshape(-1, 12)  # a lane's four pixels: every value at every byte position
    assert all(len(np.unique(quads[:, k])) == 6 for k in range(12))
    for k, name in enumerate(("per_channel_r", "per_channel_g", "per_channel_b")):
        assert f[name][..., k].any() and not np.delete(f[name], k, axis=2).any()


def test_clamp_edge_sits_on_both_clamps():
    frame = fr.adversarial_frames(64, 64, fr.ZOO_SEED, names=("clamp_edge",))["clamp_edge"]
    raw = fr._laplacian_i32(fr.median3(fr.gray(frame)))
    for value in (-1, 0, 1, 254, 255, 256):
        assert np.count_nonzero(raw == value) >= 3, value


def test_border_only_is_zero_inside():
    frame = fr.adversarial_frames(40, 44, fr.ZOO_SEED, names=("border_only",))["border_only"]
    assert not frame[2:-2, 2:-2].any() and frame[:2].any() and frame[-2:].any() and frame[:, :2].any() and frame[:, -2:].any()
    assert fr.laplacian_of_frame(frame)[5:-5, 5:-5].max() == 0 and fr.laplacian_of_frame(frame).any()


@pytest.mark.parametrize("h,w", [(130, 1030), (67, 36), (40, 2048), (9, 8), (600, 600)])
def test_impulses_straddle_the_boundaries_they_claim(h, w):
    plane = fr.adversarial_frames(h, w, fr.ZOO_SEED, names=("impulses",))["impulses"][..., 0]
    assert set(np.unique(plane)) == {0, 255}
    xs, ys = fr.impulse_boundaries(h, w)
    assert xs == list(range(4, w, 4)) and ys == list(range(8, h, 8))
    for m in (248, 256, 512):
        assert all(x in xs for x in range(m, w, m))
    for x in xs:
        assert np.any((plane[:, x - 1] == 255) & (plane[:, x] == 255)), x
    for y in ys:
        assert np.any((plane[y - 1] == 255) & (plane[y] == 255)), y
        for x in xs:
            if x % 248 == 0 or x % 256 == 0:
                assert plane[y - 1:y + 1, x - 1:x + 1].all(), (y, x)
    for cy in (0, h - 1):
        for cx in (0, w // 2, w - 1):
            assert plane[cy, cx] == 255
    assert plane[h // 2, 0] == 255 and plane[h // 2, w - 1] == 255
    if h >= 8:  # the blocks survive the median: the chain sees them
        assert fr.laplacian_of_frame(fr._rgb(plane)).any()


def test_the_roll_kernel_bound_the_gpu_test_quotes_is_the_one_in_the_source():
    import os

    from tests import helpers

    text = open(os.path.join(helpers.ROOT, "reinfocus_amd", "csrc", "rf_focus.h")).read()
    assert re.search(r"constexpr int kRollBandMax = 64; // rows per band: a lane's sum of squares stays below 2\^32 / 64", text)
