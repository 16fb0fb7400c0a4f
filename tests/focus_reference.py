"""An integer reference of the focus measure and a zoo of hostile frames (test infrastructure, no fixtures).

The measure is cv2.cvtColor(RGB2GRAY) -> cv2.medianBlur(3) -> cv2.Laplacian(CV_8U) -> ndarray.var().  Everything here is
written from the OpenCV definitions of those four steps in plain numpy integers -- a true sort for the median, np.pad for
the borders, Python ints for the sums and one Python int / int for the variance -- and shares no code and no structure
with the kernels (reinfocus_amd/csrc/rf_focus.h) or the C oracle (oracle/rf_oracle.c), so that it can be held against both.
"""

import numpy as np

# cvtColor(COLOR_RGB2GRAY) on 8-bit images: fixed point, (R cr + G cg + B cb + half) >> shift.  15 bits since OpenCV 4,
# 14 bits before.
GRAY_COEFFICIENTS = {15: (9798, 19235, 3735, 15), 14: (4899, 9617, 1868, 14)}

STRIP_ROWS = 256  # rows per slice of sums(): nine shifted copies of a slice are sorted at once


def gray(frames, mode=15):
    """uint8[..., 3] -> uint8[...]."""
    cr, cg, cb, shift = GRAY_COEFFICIENTS[mode]
    f = np.asarray(frames).astype(np.int64)
    out = (f[..., 0] * cr + f[..., 1] * cg + f[..., 2] * cb + (1 << (shift - 1))) >> shift
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255
    return out.astype(np.uint8)


def median3(g):
    """medianBlur(ksize=3) of uint8[h, w]: BORDER_REPLICATE, the fifth of the nine sorted values of each window."""
    g = np.asarray(g)
    h, w = g.shape
    p = np.pad(g, 1, mode="edge")
    windows = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.sort(windows, axis=0)[4]


def _reflect101_pad(a, axis):
    """One more element on either side of `axis`, BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba); an axis of one element
    has nothing to reflect about: OpenCV takes the element itself."""
    width = [(0, 0), (0, 0)]
    width[axis] = (1, 1)
    return np.pad(a, width, mode="edge" if a.shape[axis] == 1 else "reflect")


def _laplacian_i32(med):
    m = np.asarray(med).astype(np.int32)
    h, w = m.shape
    v = _reflect101_pad(m, 0)
    x = _reflect101_pad(m, 1)
    return v[0:h] + v[2:h + 2] + x[:, 0:w] + x[:, 2:w + 2] - 4 * m


def laplacian_u8(med):
    """Laplacian(ddepth=CV_8U, ksize=1) of uint8[h, w]: up + down + left + right - 4 centre, BORDER_REFLECT_101, saturated."""
    return np.clip(_laplacian_i32(med), 0, 255).astype(np.uint8)


def laplacian_rows(frame, mode, r0, r1):
    """Rows [r0, r1) of the chain's result for one frame uint8[h, w, 3], computed from the rows they depend on only:
    median rows r0 - 1 ... r1 (those inside the frame), hence gray rows r0 - 2 ... r1 + 1.  A border of the slice that is not
    a border of the frame gets the wrong padding, and exactly those rows are cut away again."""
    h = frame.shape[0]
    m0, m1 = max(r0 - 1, 0), min(r1 + 1, h)
    g0, g1 = max(m0 - 1, 0), min(m1 + 1, h)
    med = median3(gray(frame[g0:g1], mode))[m0 - g0:m1 - g0]
    assert h == 1 or m1 - m0 >= 2  # (a single median row is reflected onto itself only where the frame has one row)
    return laplacian_u8(med)[r0 - m0:r1 - m0]


def laplacian_of_frame(frame, mode=15, strip=STRIP_ROWS):
    h = frame.shape[0]
    return np.concatenate([laplacian_rows(frame, mode, r0, min(r0 + strip, h)) for r0 in range(0, h, strip)])


def sums(frames, mode=15, strip=STRIP_ROWS):
    """[(S1, S2)] as Python ints, one pair per frame of uint8[n, h, w, 3]: the sum and the sum of squares of the chain."""
    out = []
    for frame in np.asarray(frames):
        h = frame.shape[0]
        s1 = s2 = 0
        for r0 in range(0, h, strip):
            lap = laplacian_rows(frame, mode, r0, min(r0 + strip, h)).astype(np.int64)
            s1 += int(lap.sum())
            s2 += int((lap * lap).sum())
        out.append((s1, s2))
    return out


def numerator(n, s1, s2):
    """N S2 - S1^2 as a Python int: N^2 times the population variance."""
    return int(n) * int(s2) - int(s1) * int(s1)


def variance(n, s1, s2):
    """The float64 nearest to the exact rational (N S2 - S1^2) / N^2: Python's int / int is correctly rounded."""
    return numerator(n, s1, s2) / (int(n) * int(n))


def is_exact_case(n, s1, s2):
    """True when numerator and denominator are both below 2^53: each is then a float64 without rounding, and a float64
    division of the two is the one correctly rounded operation that variance() is too."""
    return numerator(n, s1, s2) < 2 ** 53 and int(n) * int(n) < 2 ** 53


def variances(frames, mode=15):
    frames = np.asarray(frames)
    n = frames.shape[1] * frames.shape[2]
    return np.array([variance(n, s1, s2) for s1, s2 in sums(frames, mode)], dtype=np.float64)


def ulps_apart(got, want):
    """|got - want| in units of the spacing of float64 at `want`."""
    return abs(float(got) - float(want)) / float(np.spacing(abs(float(want)) if want else 1.0))


# --- the shapes (h, w) the exact tests add to tests/test_gpu_parity.py FOCUS_SHAPES, named for what they reach ------------
# focus_kernel_roll (widths that are multiples of 4, >= 8) gives a lane four columns: w / 4 lanes per band of rows, lanes of
# successive bands packed into waves of 64, or of 62 counted lanes between two halo lanes when 64 % (w / 4) != 0.
NEW_SHAPES = {}
for _groups in (2, 4, 8, 16, 32, 64):  # no halo lanes; 77 rows: ten bands of 8, the last one of 5 rows
    NEW_SHAPES[f"no_halo_{_groups}_lanes_per_row"] = (77, 4 * _groups)
for _groups, _what in ((62, "a_wave_ends_on_the_frame_edge"), (63, "a_wave_ends_one_lane_before_the_edge"),
                       (65, "a_wave_ends_one_lane_after_the_edge"), (124, "two_waves_per_row")):
    NEW_SHAPES[f"halo_{_groups}_lanes_{_what}"] = (37, 4 * _groups)
NEW_SHAPES["three_lanes_per_row_21_rows_of_bands_in_a_wave"] = (200, 12)
for _h in (1, 2, 3, 4, 5):  # shorter than the four rows between a load and its Laplacian
    NEW_SHAPES[f"short_{_h}_rows_narrow"] = (_h, 8)
    NEW_SHAPES[f"short_{_h}_rows_one_wave_per_row"] = (_h, 256)
for _w in (511, 513, 1025, 6, 7):  # focus_kernel: a byte per thread, bands of 16 rows, tiles of 512 columns
    for _h in (15, 16, 17, 33):
        NEW_SHAPES[f"byte_kernel_{_h}x{_w}"] = (_h, _w)
del _groups, _what, _h, _w

BAND_SHAPES = [(70, 8), (67, 36), (130, 248), (129, 256), (200, 12)]  # run at every band height 1 ... 64
STEP_SHAPES = [(6, 128, 128), (3, 100, 100), (2, 33, 35), (2, 61, 256)]  # (n, h, w) of rf_step

# Frames whose N S2 - S1^2 reaches 2^64 (the two-limb branch of variance_from_sums).  The variance of `two_level` is about
# 14 290 and that of `noise` about 1 081 at any size, so N^2 * 1081 >= 2^64 needs N >= 1.31e8 pixels: 11 500 rows.  One
# width for focus_kernel_roll, one that is not a multiple of 4 for the byte kernel.
LARGE_NAMES = ("noise", "two_level")
LARGE_SHAPES = [(11500, 11500), (11500, 11501)]

ZOO_SEED = 20240


def exact_shapes(focus_shapes):
    """Every (h, w) of the exactness test: those of FOCUS_SHAPES ((n, h, w) triples) and the new ones, without repeats."""
    return sorted({(h, w) for _, h, w in focus_shapes} | set(NEW_SHAPES.values()))


# --- the zoo ---------------------------------------------------------------------------------------------------------

CONSTANT = "constant_77"


def _rgb(plane):
    return np.repeat(np.asarray(plane, dtype=np.uint8)[:, :, None], 3, axis=2)


def _noise(h, w, rng):
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _low_entropy(h, w, rng):
    return rng.integers(0, 3, size=(h, w, 3), dtype=np.uint8)


def _two_level(h, w, rng):
    return _rgb(rng.integers(0, 2, size=(h, w)) * 255)


def _extremes(h, w, rng):
    return rng.choice(np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8), size=(h, w, 3))


def _rows_1px(h, w, rng):
    yy, _ = np.mgrid[0:h, 0:w]
    return _rgb((yy % 2) * 255)


def _cols_1px(h, w, rng):
    _, xx = np.mgrid[0:h, 0:w]
    return _rgb((xx % 2) * 255)


def _checker_1px(h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    return _rgb(((yy + xx) % 2) * 255)


def _checker_2px(h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    return _rgb(((yy // 2 + xx // 2) % 2) * 255)


def _clamp_edge(h, w, rng):
    """Upper half: the bowl (x - cx)^2 + (y - cy)^2 scaled to span 0 ... 254 over the frame -- its Laplacian, four times
    the scale, is far below 255 -- plus noise of 0 / 1: Laplacians on either side of 0.  A Laplacian of 255 needs a
    curvature that 8-bit gray cannot keep up over more than two pixels, so the lower half holds three-pixel column stripes
    (which the median keeps) of 0 and 254 with the same noise: the pixels below a step see 254 and a little more or less."""
    yy, xx = np.mgrid[0:h, 0:w]
    r2 = (xx - w // 2) ** 2 + (yy - h // 2) ** 2
    bowl = (r2 * 254) // max(int(r2.max()), 1)
    stripes = ((xx // 3) % 2) * 254
    plane = np.where(yy < (h + 1) // 2, bowl, stripes) + rng.integers(0, 2, size=(h, w))
    return _rgb(plane)


def _border_only(h, w, rng):
    f = np.zeros((h, w, 3), dtype=np.uint8)
    r = _noise(h, w, rng)
    for edge in (np.s_[:2], np.s_[-2:]):
        f[edge] = r[edge]
        f[:, edge] = r[:, edge]
    return f


def impulse_boundaries(h, w):
    """What _impulses claims: the x for which a block of 255 lies on columns x - 1 and x, and the y likewise for rows."""
    xs = [x for x in range(4, w, 4)]
    ys = [y for y in range(8, h, 8)]
    return xs, ys


def _impulses(h, w, rng):
    """3 x 3 blocks of 255 on black (the median erases a single pixel): the four corners, the middle of each edge, one
    centred on every multiple of 4 in x (hence of 248, 256 and 512: the lane, wave and tile edges) and on every multiple of
    8 in y (hence of 16, 32 and 64: the band edges) -- walking down / across the frame so that most stand alone -- and one
    on every crossing of a multiple of 248, 256 or 512 in x with a multiple of 8 in y."""
    plane = np.zeros((h, w), dtype=np.uint8)

    def block(cy, cx):
        plane[max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = 255

    for cy in (0, h // 2, h - 1):
        for cx in (0, w // 2, w - 1):
            if (cy, cx) != (h // 2, w // 2):
                block(cy, cx)
    xs, ys = impulse_boundaries(h, w)
    for k, x in enumerate(xs):
        block((5 * k + 2) % h, x)
    for k, y in enumerate(ys):
        block(y, (7 * k + 3) % w)
    for x in xs:
        if x % 248 == 0 or x % 256 == 0:
            for y in ys:
                block(y, x)
    return _rgb(plane)


def _per_channel(channel):
    def make(h, w, rng):
        f = np.zeros((h, w, 3), dtype=np.uint8)
        f[..., channel] = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        return f
    return make


def _constant(h, w, rng):
    return np.full((h, w, 3), 77, dtype=np.uint8)


GENERATORS = {
    "noise": _noise,
    "low_entropy": _low_entropy,
    "two_level": _two_level,
    "extremes": _extremes,
    "rows_1px": _rows_1px,
    "cols_1px": _cols_1px,
    "checker_1px": _checker_1px,
    "checker_2px": _checker_2px,
    "clamp_edge": _clamp_edge,
    "border_only": _border_only,
    "impulses": _impulses,
    "per_channel_r": _per_channel(0),
    "per_channel_g": _per_channel(1),
    "per_channel_b": _per_channel(2),
}


def adversarial_frames(h, w, seed, names=None):
    """{name: uint8[h, w, 3]}; a frame depends on (h, w, seed, name) only, not on which others are asked for."""
    out = {}
    for index, (name, make) in enumerate(GENERATORS.items()):
        if names is None or name in names:
            frame = make(h, w, np.random.default_rng([seed, h, w, index]))
            assert frame.shape == (h, w, 3) and frame.dtype == np.uint8
            out[name] = np.ascontiguousarray(frame)
    return out


def zoo_batch(h, w, seed):
    """(names, uint8[n, h, w, 3]): the zoo of one shape as the environments of one launch, in a seeded shuffled order with
    the constant frame in the middle."""
    frames = adversarial_frames(h, w, seed)
    names = list(frames)
    order = np.random.default_rng([seed, h, w, 1000]).permutation(len(names))
    names = [names[i] for i in order]
    names.insert(len(names) // 2, CONSTANT)
    frames[CONSTANT] = _constant(h, w, None)
    return names, np.stack([frames[name] for name in names])
