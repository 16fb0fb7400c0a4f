"""PixelEnv::dir_fast (rf_math.h dir_fast_env): the per-environment flag with which sample_axis_shade normalises its
directions through len_inv_rn_fast WITHOUT unit_dir_y's per-lane range test.  The flag may only be set when every squared
length the environment can produce lies in [2^-100, 2^100) -- checked here on the host, with the header compiled as
tests/hostsim compiles it, around every threshold of the rule -- and it has to be set for every camera the product makes
(or the headline path would silently take the guarded form)."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import helpers

F = np.float32
LO, HI = F(2.0 ** -49), F(2.0 ** 48)


@pytest.fixture(scope="module")
def lib():
    so = ctypes.CDLL(helpers.built("tests/dirfast", "libdirfast.so"))
    so.df_lens_bound.restype = ctypes.c_float
    so.df_lens_bound.argtypes = [ctypes.c_double]
    so.df_flags.restype = None
    so.df_flags.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_long, ctypes.c_void_p]
    so.df_flag_without_lens.restype = ctypes.c_int
    so.df_flag_without_lens.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    so.df_check_miss.restype = ctypes.c_long
    so.df_check_miss.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_long, ctypes.c_long,
                                 ctypes.c_uint64, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_long)]
    so.df_hit_in_range.restype = ctypes.c_int
    so.df_hit_in_range.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_float)]
    return so


def flags(lib, cam, rect, lens):
    cam, rect = np.ascontiguousarray(cam, dtype=F), np.ascontiguousarray(rect, dtype=F)
    out = np.zeros(len(cam), dtype=np.uint8)
    lib.df_flags(cam.ctypes.data, rect.ctypes.data, float(lens), len(cam), out.ctypes.data)
    return out.astype(bool)


def rule(cam, lens_r):
    """The flag as the issue states it, in numpy float32: |llz| in [2^-49, 2^48], |llx| + |hx| + r <= 2^48 and
    |lly| + |vy| + r <= 2^48, every comparison true."""
    with np.errstate(all="ignore"):
        az = np.abs(cam[:, 2])
        bx = (np.abs(cam[:, 0]) + np.abs(cam[:, 3])) + F(lens_r)
        by = (np.abs(cam[:, 1]) + np.abs(cam[:, 7])) + F(lens_r)
        return (az >= LO) & (az <= HI) & (bx <= HI) & (by <= HI)


def threshold_environments():
    """Camera constants around every threshold: llz at +-2^-50, +-2^-49, +-2^48, +-2^49, zero, infinite, NaN and ordinary;
    the x and the y bound at 2^48 and one ulp either side of it (in one term and split over two), zero, infinite, NaN."""
    up, down = np.nextafter(HI, F(np.inf)), np.nextafter(HI, F(0))
    half = F(2.0 ** 47)
    llz = [F(s * v) for v in (2.0 ** -50, 2.0 ** -49, 2.0 ** 48, 2.0 ** 49, 1.0, 10.0) for s in (1, -1)]
    llz += [F(0), F(-0.0), F(np.inf), F(-np.inf), F(np.nan), np.nextafter(LO, F(0)), np.nextafter(LO, F(1))]
    # (ll, extent) pairs of one axis
    axis = [(F(0), down), (F(0), HI), (F(0), up), (-down, F(0)), (-HI, F(0)), (-up, F(0)),
            (-half, half), (-half, np.nextafter(half, F(np.inf))), (-half, np.nextafter(half, F(0))), (half, -half),
            (F(0), F(0)), (F(-2.5), F(5.0)), (F(np.inf), F(1)), (F(1), F(-np.inf)), (F(np.nan), F(1)), (F(1), F(np.nan)),
            (F(2.0 ** 49), F(2.0 ** 49)), (F(-1e-30), F(2e-30))]
    cams = []
    for z, (llx, hx), (lly, vy) in itertools.product(llz, axis, axis):
        cams.append([llx, lly, z, hx, 0, 0, 0, vy, 0])
    cam = np.array(cams, dtype=F)
    rect = np.tile(np.array([-8.0, 1.0], dtype=F), (len(cam), 1))
    return cam, rect


LENSES = [0.05, 0.0, 0.6243510725689605, 2.0 ** 24, 2.0 ** 47, 2.0 ** 48, float("inf"), float("nan")]


def test_flag_is_the_stated_rule_and_implies_the_range(lib):
    cam, rect = threshold_environments()
    total_true = total_checked = 0
    for lens in LENSES:
        r = lib.df_lens_bound(lens)
        assert not (r < abs(lens)), (lens, r)  # r >= |lens radius| (or both NaN)
        got = flags(lib, cam, rect, lens)
        assert np.array_equal(got, rule(cam, r)), lens
        # both sides of every threshold occur
        total_true += int(got.sum())
        first, checked = ctypes.c_long(-1), ctypes.c_long(0)
        # 16 corners + random samples for every flagged environment and both lens_offset forms: > 10^6 in all (below)
        bad = lib.df_check_miss(cam.ctypes.data, rect.ctypes.data, float(lens), len(cam), 250, 9, ctypes.byref(first),
                                ctypes.byref(checked))
        assert bad == 0, (lens, bad, first.value, cam[first.value])
        total_checked += checked.value
    assert total_true > 1000 and total_checked >= 10 ** 6, (total_true, total_checked)
    # the thresholds themselves, spelled out (lens radius 0): at the bound yes, one ulp beyond no
    z = F(-10.0)
    up = np.nextafter(HI, F(np.inf))
    named = np.array([[0, 0, -LO, 1, 0, 0, 0, 1, 0], [0, 0, -np.nextafter(LO, F(0)), 1, 0, 0, 0, 1, 0],
                      [0, 0, HI, 1, 0, 0, 0, 1, 0], [0, 0, up, 1, 0, 0, 0, 1, 0],
                      [0, 0, z, HI, 0, 0, 0, 1, 0], [0, 0, z, up, 0, 0, 0, 1, 0],
                      [0, 0, z, 1, 0, 0, 0, HI, 0], [0, 0, z, 1, 0, 0, 0, up, 0],
                      [0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, np.nan, 1, 0, 0, 0, 1, 0], [np.inf, 0, z, 1, 0, 0, 0, 1, 0],
                      [0, np.nan, z, 1, 0, 0, 0, 1, 0]], dtype=F)
    want = [True, False, True, False, True, False, True, False, False, False, False, False]
    assert flags(lib, named, rect[:len(named)], 0.0).tolist() == want
    # a non-finite lens radius clears it everywhere; so does not naming the lens at all (the host twin's call)
    assert not flags(lib, cam, rect, float("inf")).any() and not flags(lib, cam, rect, float("nan")).any()
    ordinary = np.array([[-2.5, -2.5, -10, 5, 0, 0, 0, 5, 0]], dtype=F)
    assert flags(lib, ordinary, rect[:1], 0.05).all()
    assert lib.df_flag_without_lens(ordinary.ctypes.data, rect.ctypes.data) == 0


def test_a_million_random_miss_samples_of_flagged_environments(lib):
    """10^6 random (s, t, disc point) samples of environments that sit on the inner side of the thresholds."""
    rng = np.random.default_rng(48)
    n = 50
    mag = lambda lo, hi: F(2.0) ** rng.uniform(lo, hi, n).astype(F) * rng.choice([F(-1), F(1)], n)
    cam = np.zeros((n, 9), dtype=F)
    cam[:, 0], cam[:, 3] = mag(-60, 46.9), mag(-60, 46.9)
    cam[:, 1], cam[:, 7] = mag(-60, 46.9), mag(-60, 46.9)
    cam[:, 2] = mag(-49, 48)
    cam[:5, 2] = [LO, -LO, HI, -HI, LO]  # the z thresholds with large and with tiny x, y
    cam[4, [0, 1, 3, 7]] = F(1e-40)      # (subnormal: their squares vanish)
    rect = np.tile(np.array([-8.0, 1.0], dtype=F), (n, 1))
    assert flags(lib, cam, rect, 0.05).all()
    first, checked = ctypes.c_long(-1), ctypes.c_long(0)
    bad = lib.df_check_miss(cam.ctypes.data, rect.ctypes.data, 0.05, n, 10_000, 1, ctypes.byref(first), ctypes.byref(checked))
    assert checked.value >= 10 ** 6
    assert bad == 0, (bad, first.value, cam[first.value])


def test_hit_lanes_are_in_range_whatever_the_environment(lib):
    """Hit lanes shade (q0, q1, 1 + q2) of an accepted sphere draw (|q| < 1, multiples of 2^-24): the extremes."""
    e = 2.0 ** -24
    sq = ctypes.c_float()
    for q in [(0.0, 0.0, -1.0 + e), (1.0 - e, 0.0, 0.0), (-(1.0 - e), 0.0, 0.0), (0.0, 1.0 - e, 0.0), (0.0, -(1.0 - e), 0.0),
              (0.0, 0.0, 1.0 - e), (0.0, 0.0, 0.0), (e, -e, -1.0 + 2 * e)]:
        assert lib.df_hit_in_range(*[float(F(c)) for c in q], ctypes.byref(sq)) == 1, (q, sq.value)
        assert 2.0 ** -48 <= sq.value < 6.0, (q, sq.value)


def test_every_product_camera_gets_the_flag(lib):
    """FastCameras (aperture 0.1) at every focus distance in [0.1, 1000]: the product path must not fall to the guarded
    form."""
    from reinfocus_amd.graphics import camera

    focus = np.concatenate([np.geomspace(0.1, 1000.0, 20001), np.linspace(0.1, 1000.0, 20001), [0.1, 5.0, 10.0, 1000.0]])
    cams = camera.FastCameras()
    cams.update(focus.astype(F))
    dyn, origin, u, v, lens = cams.device_data()
    cam = np.ascontiguousarray(np.asarray(dyn, dtype=F).reshape(len(focus), 9))
    assert float(lens) == 0.05
    rect = np.tile(np.array([-8.0, 10.0], dtype=F), (len(cam), 1))
    assert flags(lib, cam, rect, float(lens)).all()
