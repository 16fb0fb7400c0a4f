"""len_inv_rn_fast (rf_math.h): the pair len = RN(sqrt(sq)), inv = RN(1 / len) that every render kernel normalises its
shading directions with comes from one v_rsq_f32 and fmas.  It depends on sq alone, so equality with the IEEE
operators is checked for EVERY float the fast path accepts, on the device the kernels run on (tests/lencheck)."""
import json
import subprocess
import sys

import pytest

from tests import helpers

CHILD = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
out = (ctypes.c_ulonglong * 3)()
rc = lib.lc_check_len_inv(out)
print(json.dumps({"rc": rc, "bad": out[0], "first": out[1], "visited": out[2]}))
"""


@pytest.mark.gpu
def test_len_and_reciprocal_from_one_rsq_are_ieee_exact():
    """One launch over the 0x64000000 bit patterns of [2^-100, 2^100) (about a second), in a child process so that
    the launch has a time limit of its own: no x may give a len other than sqrtf(x) or an inv other than 1.0f / len."""
    path = helpers.built("tests/lencheck", "liblencheck.so")
    out = subprocess.run([sys.executable, "-c", CHILD, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["rc"] == 0, got
    assert got["visited"] == 0x71800000 - 0x0D800000
    assert got["bad"] == 0, "%d mismatches, the first at x = bits 0x%08x" % (got["bad"], got["first"] & 0xFFFFFFFF)
