"""CPU tests of the one-argument functions of csrc/rf_policy_math.h -- expw32 (exp32), log32, tanh32, sigmoid32, the two
halves of normal32 (and with them log64 on every argument its caller gives it) -- and of float32 sqrtf and 1.0f / x, over
EVERY float32 of their domains (tests/mathcheck/mathcheck.h has the sweeps and the digest of a chunk of 2^22 patterns):

  - the host build of the header (tests/mathcheck/libmathcheck_host.so) gives the digests of
    tests/golden/scalar_digests.npy on all 1024 chunks of all 8 sweeps, so the fixture cannot outlive a change of the header
    (tests/golden/make_scalar_digests.py wrote it after the numpy twins had restated every chunk);
  - the numpy twins equal the host build as bits, result by result, on a fixed list of chunks per sweep (the ends of the
    domains, +-0, -87, +-inf and the NaNs, 1.0, the joins of normal32, four seeded random chunks), and their restated
    digests equal the fixture there;
  - the errors against glibc's float64 functions over the full domains stay within bounds that are derived, not fitted
    (profiles/scalar_math.md records the measured ones).
tests/test_gpu_scalar_math.py holds the device to the same fixture."""

import concurrent.futures
import os

import numpy as np
import pytest

from reinfocus_amd.environments import sde
from tests import helpers
from tests import scalar_math as sm

# exp32 and log32: the project's bounds (tests/test_policy_logic.py), log32's now over every positive normal.
# tanh32 = (1 - t) / (1 + t), t = exp32(-2|x|) within 2^-21 of exp absolutely (t <= 1); |d/dt (1 - t) / (1 + t)| <= 2 makes
#   that 2^-20; the float32 roundings of 1 - t, 1 + t (values <= 2: 2^-24 each, passed on with a factor <= 1) and of the
#   quotient (<= 1: 2^-25) add less than 3 * 2^-24: below 2^-19.
# sigmoid32 = 1 / (1 + t) or t / (1 + t), t = exp32(-|x|): the derivative in t is <= 1, so 2^-21, and the roundings of 1 + t
#   and of the quotient add less than 2 * 2^-24: below 2^-20.
ERROR_BOUNDS = {0: 2.0 ** -21, 1: 2.0 ** -21, 2: 2.0 ** -19, 3: 2.0 ** -20}


@pytest.fixture(scope="module")
def host():
    return sm.Library(helpers.built("tests/mathcheck", "libmathcheck_host.so"))


@pytest.fixture(scope="module")
def fixture():
    digests = np.load(sm.FIXTURE)
    assert digests.dtype == np.uint64 and digests.shape == (sm.SWEEPS, sm.CHUNKS)
    return digests


def test_domains_are_what_the_header_of_the_checker_says():
    assert sm.bits_of(2.0 ** -54) == sm.FIRST[6] and sm.bits_of(2.0 ** -29) == sm.FIRST[7] and sm.bits_of(0.5) == sm.LAST[6]
    assert sm.bits_of(np.finfo(np.float32).tiny) == sm.FIRST[1] and sm.bits_of(np.finfo(np.float32).max) == sm.LAST[1]
    assert sm.P_R5 >= sm.f32(2.0 ** -54)
    p = sm.patterns_of(7, sm.FIRST[7] >> sm.CHUNK_SHIFT)[:4096].view(np.float32).astype(np.float64)
    assert np.array_equal(1.0 - (1.0 - p), p)  # the subtraction of sweep 7 is exact from its first pattern on
    for which in range(sm.SWEEPS):
        assert int(sm.expected_visits(which).sum()) == sm.LAST[which] - sm.FIRST[which] + 1


@pytest.mark.parametrize("which", range(sm.SWEEPS))
def test_host_build_gives_the_fixture_on_every_chunk(host, fixture, which):
    rc, digests, visited = host.digests(which)
    assert rc == 0
    assert np.array_equal(visited, sm.expected_visits(which))
    differ = np.flatnonzero(digests != fixture[which])
    assert differ.size == 0, "%s: %d chunks differ from tests/golden/scalar_digests.npy, the first %d" % (
        sm.NAMES[which], differ.size, differ[0])
    assert np.array_equal(digests != 0, sm.expected_visits(which) > 0)  # nothing outside the domain contributes


def _twin_chunk(host, which, chunk):
    patterns = sm.patterns_of(which, chunk)
    rc, got = host.map(which, patterns)
    want = sm.twin(which, patterns)
    return chunk, patterns, rc, got, want, sm.digest(patterns, want)


@pytest.mark.parametrize("which", range(sm.SWEEPS))
def test_twins_equal_the_host_build_as_bits(host, fixture, which):
    chunks = sm.fixed_chunks(which)
    assert len(chunks) == len(set(chunks)) >= 7 and all(k in sm.domain_chunks(which) for k in chunks)
    # (the chunks side by side: numpy and the library call release the interpreter lock)
    with concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        results = list(pool.map(lambda chunk: _twin_chunk(host, which, chunk), chunks))
    for chunk, patterns, rc, got, want, restated in results:
        assert rc == 0
        differ = np.flatnonzero(got != want)
        assert differ.size == 0, "%s, chunk %d: %d results differ, the first at x = bits 0x%08x: host 0x%08x, twin 0x%08x" % (
            sm.NAMES[which], chunk, differ.size, patterns[differ[0]], got[differ[0]], want[differ[0]])
        assert restated == int(fixture[which, chunk]), (sm.NAMES[which], chunk)


def test_fixed_chunks_hold_the_edges_they_are_named_for():
    """The chunk lists are derived from values; this says which patterns they are meant to contain."""
    full = sm.fixed_chunks(0)
    for bits in (0x00000000, 0x80000000, 0x7F800000, 0x7FC00000, 0x7FFFFFFF, 0xFF800000, 0xFFFFFFFF, 0x00800000, 0x7F7FFFFF,
                 0x3F800000, sm.bits_of(-87.0)):
        assert bits >> sm.CHUNK_SHIFT in full, hex(bits)
    for which in (2, 3, 4, 5):
        for bits in (0x00000000, 0x80000000, 0x7F800000, 0x7FFFFFFF, 0xFF800000, 0xFFFFFFFF, 0x00800000, 0x7F7FFFFF, 0x3F800000):
            assert bits >> sm.CHUNK_SHIFT in sm.fixed_chunks(which), (which, hex(bits))
    for bits in (0x00800000, 0x7F7FFFFF, 0x3F800000):
        assert bits >> sm.CHUNK_SHIFT in sm.fixed_chunks(1), hex(bits)
    # the joins of normal32: p = 0.075f, and the p at which r = sqrt(-log64(p)) passes 5 -- both sides lie in the chunk
    # (exp(-25) < 2^-29: sweep 7, whose 1 - p has to be exact, ends before the second join)
    assert sm.chunk_of(0.075) in sm.fixed_chunks(6) and sm.chunk_of(sm.P_R5) in sm.fixed_chunks(6)
    assert sm.chunk_of(0.075) in sm.fixed_chunks(7) and sm.P_R5 < sm.f32(2.0 ** -29)
    p = sm.patterns_of(6, sm.chunk_of(0.075)).view(np.float32)
    assert p[0] < sde.P_CENTRAL <= p[-1]
    p = sm.patterns_of(6, sm.chunk_of(sm.P_R5)).view(np.float32).astype(np.float64)
    r = np.sqrt(-sde.log64(p))
    assert r[0] > 5.0 >= r[-1]


@pytest.mark.parametrize("which", range(4))
def test_errors_against_float64_over_the_full_domain(host, which):
    rc, worst = host.errors(which)
    assert rc == 0
    assert np.all(np.isfinite(worst))
    chunk = int(np.argmax(worst))
    print("%s: largest error 2^%.2f in chunk %d" % (sm.NAMES[which], np.log2(worst[chunk]), chunk))
    assert worst[chunk] <= ERROR_BOUNDS[which], (sm.NAMES[which], chunk, float(worst[chunk]))
    assert worst[chunk] >= 2.0 ** -25  # the sweep did compare something: no float32 function is exact to half an ulp of 1
