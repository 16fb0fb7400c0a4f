"""Writes tests/golden/scalar_digests.npy: uint64 [8][1024], the digest of every chunk of every sweep of tests/mathcheck
(mathcheck.h: expw32, log32, tanh32, sigmoid32, sqrtf, 1.0f / x and the two halves of normal32 over every float32 of their
domains).  Run once on a CPU, after building tests/mathcheck/libmathcheck_host.so:

    python tests/golden/make_scalar_digests.py [output path]

The file is written only when
  1. the host build of csrc/rf_policy_math.h gave the digests,
  2. the numpy twins (policy.exp32 / log32 / tanh32, sde.expw32 / normal32, lstm.sigmoid32, numpy.sqrt, float32(1) / x),
     restated chunk by chunk over EVERY chunk of every sweep, gave the same ones (processes, at most 16), and
  3. the range facts the header states hold over the whole domain:
       exp32      +0 or a normal number of [exp32(-87), 1], never a subnormal
       tanh32     within [-1, 1]; tanh32(-x) is tanh32(x) with the sign bit flipped
       sigmoid32  within [0, 1]
       normal32   does not decrease in p over all of sweep 6; sweep 7 is its exact negation where both are defined
                  (p = 1/2 aside: both sweeps make the same call there, normal32(1/2) = +0).
It also prints what profiles/scalar_math.md records: the wall time and the largest error of exp32, log32, tanh32 and
sigmoid32 against the float64 functions (mc_errors) with the argument it lies at.
"""

import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from reinfocus_amd.environments import policy  # noqa: E402
from tests import helpers  # noqa: E402
from tests import scalar_math as sm  # noqa: E402

f32 = np.float32
SIGN = np.uint32(0x80000000)


def _values(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(f32)


def _plain(which, chunk):
    """Sweeps 0, 1, 3, 4, 5: the twin's digest of one chunk and the range facts of exp32 and sigmoid32."""
    patterns = sm.patterns_of(which, chunk)
    bits = sm.twin(which, patterns)
    x, y = _values(patterns), _values(bits)
    broken = []
    if which == 0:
        low = x <= f32(0.0)  # the half that is exp32
        floor = policy.exp32(f32(-87.0))
        ok = (bits == 0) | ((y >= floor) & (y <= f32(1.0)) & (y >= np.finfo(f32).tiny))
        if not np.all(ok[low]):
            broken.append("exp32 leaves {0} + [exp32(-87), 1] at bits 0x%08x" % patterns[low][~ok[low]][0])
    if which == 3:
        live = x == x
        ok = (y >= f32(0.0)) & (y <= f32(1.0))
        if not np.all(ok[live]):
            broken.append("sigmoid32 leaves [0, 1] at bits 0x%08x" % patterns[live][~ok[live]][0])
    return {"digests": {(which, chunk): sm.digest(patterns, bits)}, "broken": broken}


def _tanh(chunk):
    """Sweep 2: chunk (x >= 0) and its mirror chunk + 512 (the same magnitudes, negative) together."""
    patterns, mirror = sm.patterns_of(2, chunk), sm.patterns_of(2, chunk + 512)
    bits, mirror_bits = sm.twin(2, patterns), sm.twin(2, mirror)
    x, y, my = _values(patterns), _values(bits), _values(mirror_bits)
    live = x == x
    broken = []
    if not (np.all(np.abs(y[live]) <= f32(1.0)) and np.all(np.abs(my[live]) <= f32(1.0))):
        broken.append("tanh32 leaves [-1, 1] in chunk %d or its mirror" % chunk)
    odd = mirror_bits == (bits ^ SIGN)
    if not np.all(odd[live]):
        broken.append("tanh32(-x) is not -tanh32(x) at bits 0x%08x" % patterns[live][~odd[live]][0])
    return {"digests": {(2, chunk): sm.digest(patterns, bits), (2, chunk + 512): sm.digest(mirror, mirror_bits)},
            "broken": broken}


def _normal(chunk):
    """Sweeps 6 and 7 on one chunk of p: order inside the chunk, its two end values, and the negation."""
    patterns = sm.patterns_of(6, chunk)
    bits = sm.twin(6, patterns)
    y = _values(bits)
    broken = []
    if not np.all(y[1:] >= y[:-1]):
        broken.append("normal32 decreases in p after bits 0x%08x" % patterns[:-1][~(y[1:] >= y[:-1])][0])
    out = {"digests": {(6, chunk): sm.digest(patterns, bits)}, "broken": broken, "ends": (chunk, float(y[0]), float(y[-1]))}
    upper = sm.patterns_of(7, chunk)
    if upper.size:
        upper_bits = sm.twin(7, upper)
        out["digests"][(7, chunk)] = sm.digest(upper, upper_bits)
        lower_bits = bits[patterns.size - upper.size:]  # (both domains end at 1/2: the common patterns are the last ones)
        assert np.array_equal(patterns[patterns.size - upper.size:], upper)
        same = (upper_bits == (lower_bits ^ SIGN)) | (upper == np.uint32(0x3F000000))
        if not np.all(same):
            broken.append("normal32(1 - p) is not -normal32(p) at bits 0x%08x" % upper[~same][0])
        if upper[-1] == 0x3F000000 and not (upper_bits[-1] == 0 and lower_bits[-1] == 0):
            broken.append("normal32(1/2) is not +0")
    return out


def _task(task):
    kind, which, chunk = task
    return _plain(which, chunk) if kind == "plain" else _tanh(chunk) if kind == "tanh" else _normal(chunk)


def _reference(which, x):
    """The float64 function and the error metric of mc_errors, restated with numpy to find where a maximum lies."""
    wide = x.astype(np.float64)
    with np.errstate(all="ignore"):
        if which == 0:
            want = np.exp(wide)
            return np.where((x >= f32(-87.0)) & (x <= f32(0.0)), np.abs(policy.exp32(np.where(x <= 0, x, f32(0.0))) - want) / want, 0.0)
        if which == 1:
            want = np.log(wide)
            return np.abs(policy.log32(x) - want) / np.maximum(1.0, np.abs(want))
        if which == 2:
            return np.where(x == x, np.abs(policy.tanh32(x) - np.tanh(wide)), 0.0)
        return np.where(x == x, np.abs(sm.lstm.sigmoid32(x) - 1.0 / (1.0 + np.exp(-wide))), 0.0)


def main():
    started = time.time()
    path = sys.argv[1] if len(sys.argv) > 1 else sm.FIXTURE
    host = sm.Library(helpers.built("tests/mathcheck", "libmathcheck_host.so"))

    # 1. the host build
    digests = np.zeros((sm.SWEEPS, sm.CHUNKS), dtype=np.uint64)
    for which in range(sm.SWEEPS):
        rc, digests[which], visited = host.digests(which)
        assert rc == 0, (which, rc)
        assert np.array_equal(visited, sm.expected_visits(which)), which
    host_seconds = time.time() - started

    # 2. the twins, every chunk of every sweep; 3. the range facts
    tasks = [("normal", 6, k) for k in sm.domain_chunks(6)] + [("tanh", 2, k) for k in range(512)]
    tasks += [("plain", which, k) for which in (0, 3, 1, 4, 5) for k in sm.domain_chunks(which)]
    twin = np.zeros_like(digests)
    seen = np.zeros(digests.shape, dtype=bool)
    broken, ends = [], {}
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        for result in pool.imap_unordered(_task, tasks, chunksize=4):
            for (which, chunk), value in result["digests"].items():
                twin[which, chunk] = value
                seen[which, chunk] = True
            broken += result["broken"]
            if "ends" in result:
                ends[result["ends"][0]] = result["ends"][1:]
    for which in range(sm.SWEEPS):
        assert np.array_equal(seen[which], sm.expected_visits(which) > 0), which
    order = sorted(ends)
    for before, after in zip(order, order[1:]):
        if not ends[after][0] >= ends[before][1]:
            broken.append("normal32 decreases in p between chunks %d and %d" % (before, after))
    differ = np.argwhere(twin != digests)
    if len(differ) or broken:
        print("NOT WRITTEN: %d chunks differ between the host build and the twins, the first (sweep, chunk) %s; %s"
              % (len(differ), differ[:8].tolist(), broken[:8]))
        return 1

    # the errors against the float64 functions and where they lie
    errors = {}
    for which in range(4):
        rc, worst = host.errors(which)
        assert rc == 0, (which, rc)
        chunk = int(np.argmax(worst))
        patterns = sm.patterns_of(which, chunk)
        again = _reference(which, patterns.view(f32))
        at = int(np.argmax(again))
        errors[sm.NAMES[which] if which else "exp32"] = {
            "error": float(worst[chunk]), "log2": float(np.log2(worst[chunk])), "chunk": chunk,
            "x_bits": "0x%08x" % patterns[at], "x": float(patterns.view(f32)[at]), "numpy_error_there": float(again[at])}

    np.save(path, digests)
    print(json.dumps({"written": path, "host_digest_seconds": round(host_seconds, 1),
                      "wall_seconds": round(time.time() - started, 1), "processes": min(16, os.cpu_count() or 1),
                      "errors": errors}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
