"""The one-argument functions of csrc/rf_policy_math.h -- expw32 (exp32), log32, tanh32, sigmoid32, normal32 (and log64) --
and float32 sqrtf and 1.0f / x as flags.mk compiles them, ON THE DEVICE for EVERY float32 of their domains
(tests/mathcheck): each sweep's digests, one per chunk of 2^22 bit patterns, must equal tests/golden/scalar_digests.npy,
which the host build of the header and the numpy twins agree on chunk by chunk (tests/test_scalar_math_logic.py,
tests/golden/make_scalar_digests.py).  Every "equals the twin as bytes" of the kernel tests rests on this.

One test per sweep, one launch each, in a child process with a time limit of its own; the tests run one after another,
so one process has the GPU open at a time.  profiles/scalar_math.md records the times."""
import json
import subprocess
import sys

import pytest

from tests import helpers
from tests import scalar_math as sm

CHILD = """
import json, sys, time
started = time.time()
sys.path.insert(0, sys.argv[3])
import numpy as np
from tests import scalar_math as sm
which = int(sys.argv[2])
lib = sm.Library(sys.argv[1])
want = np.load(sm.FIXTURE)[which]
before = time.time()
rc, got, visited = lib.digests(which)
out = {"rc": rc, "digest_seconds": round(time.time() - before, 3)}
if rc == 0:  # (after a failed call nothing more is launched)
    differ = np.flatnonzero(got != want)
    out["visited_as_expected"] = bool(np.array_equal(visited, sm.expected_visits(which)))
    out["visited"] = int(visited.sum())
    out["differ"] = int(differ.size)
    if differ.size:
        chunk = int(differ[0])
        out["chunk"] = chunk
        patterns = sm.patterns_of(which, chunk)
        if patterns.size:
            rc, device = lib.map(which, patterns)
            out["map_rc"] = rc
            if rc == 0:
                twin = sm.twin(which, patterns)
                bad = np.flatnonzero(device != twin)
                out["results_differ"] = int(bad.size)
                if bad.size:
                    out["first"] = ["0x%08x" % int(a[bad[0]]) for a in (patterns, device, twin)]
out["child_seconds"] = round(time.time() - started, 3)
print(json.dumps(out))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(sm.SWEEPS))
def test_device_gives_the_fixture_on_every_float32(which):
    path = helpers.built("tests/mathcheck", "libmathcheck.so")
    out = subprocess.run([sys.executable, "-c", CHILD, path, str(which), helpers.ROOT], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = json.loads(out.stdout.strip().splitlines()[-1])
    print(sm.NAMES[which], got)
    assert got["rc"] == 0, (got, out.stderr[-2000:])
    assert got["visited_as_expected"] and got["visited"] == sm.LAST[which] - sm.FIRST[which] + 1, got
    assert got["differ"] == 0, "%s: %d chunks differ from the fixture, the first chunk %d; there %s results differ from the " \
        "twin, the first at x = bits %s: device %s, twin %s (mc_map returned %s)" % (
            (sm.NAMES[which], got["differ"], got["chunk"], got.get("results_differ")) + tuple(got.get("first", ["?"] * 3))
            + (got.get("map_rc"),))
