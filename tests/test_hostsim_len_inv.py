"""The host branch of len_inv_rn_fast (rf_math.h) is the plain operators: len = sqrtf(sq), inv = 1.0f / len.  True by
construction -- pinned down so that the host and device branches (the device one is checked exhaustively on the GPU,
tests/test_gpu_len_inv.py) cannot drift apart unnoticed."""
import ctypes

import numpy as np

from tests import helpers

LO_BITS, END_BITS = 0x0D800000, 0x71800000  # in_fast_range: [2^-100, 2^100)


def test_host_branch_is_sqrt_and_division():
    lib = ctypes.CDLL(helpers.built("tests/lencheck", "liblencheck_host.so"))  # the header built as tests/hostsim builds it
    lib.lc_host_len_inv.restype = ctypes.c_int
    lib.lc_host_len_inv.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    rng = np.random.default_rng(8)
    bits = np.concatenate([
        rng.integers(LO_BITS, END_BITS, 4096, dtype=np.uint32),             # log-uniform over the whole range
        np.float32(rng.uniform(0.25, 4.0, 2048)).view(np.uint32),           # where shading directions live
        np.array([LO_BITS, LO_BITS + 1, END_BITS - 2, END_BITS - 1, 0x3F800000, 0x3F7FFFFF, 0x3F800001, 0x407FFFFF],
                 dtype=np.uint32)])                                         # the range ends, 1 -+ 1 ulp, 4 - 1 ulp
    sq = np.ascontiguousarray(bits.view(np.float32))
    length, inv = np.empty_like(sq), np.empty_like(sq)
    assert lib.lc_host_len_inv(sq.ctypes.data, length.ctypes.data, inv.ctypes.data, len(sq)) == 0
    want_len = np.sqrt(sq.astype(np.float64)).astype(np.float32)  # f64 sqrt rounded to f32 == the f32 sqrt (53 >= 2*24+2)
    want_inv = np.float32(1.0) / want_len
    assert want_len.dtype == np.float32 and want_inv.dtype == np.float32
    assert np.array_equal(length.view(np.uint32), want_len.view(np.uint32))
    assert np.array_equal(inv.view(np.uint32), want_inv.view(np.uint32))
    # outside the range the function is not to be called: the export says so instead of computing something
    outside = np.array([0.0, 2.0 ** -101, 2.0 ** 100], dtype=np.float32)
    assert lib.lc_host_len_inv(outside.ctypes.data, length.ctypes.data, inv.ctypes.data, 3) == -1
