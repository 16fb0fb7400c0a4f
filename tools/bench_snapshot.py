"""Development benchmark of environment snapshots (rf_env_snapshot* / rf_env_restore*): wall time of env.snapshot(),
env.restore(), env.snapshot_resident() + synchronise and env.restore_resident() + synchronise of a
harness.DeviceVectorDiscreteSteps(device_initializer=True), the median of `--repeats` each, next to the same process's
milliseconds per step (the median of `--windows` windows of `--steps` steps with random actions) and, for the resident
forms, next to hipMemcpyDtoD of the same byte count between two plain device buffers in the same run (the HIP runtime the
library itself is linked against, reached through ctypes for this one comparison).  One JSON line per shape.
usage (GPU box):  python tools/bench_snapshot.py [--repeats 5] [--windows 5] [--steps 10] [n_envs frame spp]
without a shape: 4096 x 256 x 16 (bench.py's)."""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reinfocus_amd.environments import harness  # noqa: E402


def option(argv, name, default):
    if name in argv:
        at = argv.index(name)
        value = int(argv[at + 1])
        del argv[at:at + 2]
        return value
    return default


def timed_ms(call, repeats):
    times = []
    for _ in range(repeats):
        start = time.perf_counter()
        call()
        times.append((time.perf_counter() - start) * 1e3)
    return times


def device_copy_ms(size, repeats):
    """hipMemcpyDtoD of `size` bytes between two fresh device buffers, synchronised: milliseconds per repeat."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpyDtoD.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    a, b = ctypes.c_void_p(), ctypes.c_void_p()

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: HIP error {rc}")

    check(hip.hipMalloc(ctypes.byref(a), size), "hipMalloc")
    check(hip.hipMalloc(ctypes.byref(b), size), "hipMalloc")
    check(hip.hipMemset(a, 1, size), "hipMemset")
    check(hip.hipMemset(b, 2, size), "hipMemset")
    check(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")

    def copy():
        check(hip.hipMemcpyDtoD(b, a, size), "hipMemcpyDtoD")
        check(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")

    copy()  # (first touch)
    times = timed_ms(copy, repeats)
    check(hip.hipFree(a), "hipFree")
    check(hip.hipFree(b), "hipFree")
    return times


def bench(n, frame, spp, repeats, windows, steps):
    env = harness.DeviceVectorDiscreteSteps(num_envs=n, frame_height=frame, samples_per_pixel=spp, seed=0, device=0,
                                            device_initializer=True)
    rng = np.random.default_rng(0)
    env.reset()
    for _ in range(3):  # (the steps before a replayed graph exists)
        env.step(rng.integers(0, 13, n))

    def window():
        for _ in range(steps):
            env.step(rng.integers(0, 13, n))

    step_ms = [t / steps for t in timed_ms(window, windows)]
    ctx = env._ctx
    size = ctx.env_snapshot_size()
    kept = []

    def snapshot():
        kept[:] = [env.snapshot()]

    def resident(call):
        def run():
            call(0)
            ctx.synchronize()
        return run

    times = {"snapshot": timed_ms(snapshot, repeats), "restore": timed_ms(lambda: env.restore(kept[0]), repeats)}
    resident(env.snapshot_resident)()  # (the slot's allocation is not a copy)
    times["snapshot_resident"] = timed_ms(resident(env.snapshot_resident), repeats)
    times["restore_resident"] = timed_ms(resident(env.restore_resident), repeats)
    env.drop_snapshot(0)
    times["hipMemcpyDtoD_same_bytes"] = device_copy_ms(size, repeats)
    after_ms = [t / steps for t in timed_ms(window, windows)]
    medians = {name: float(np.median(values)) for name, values in times.items()}
    out = {"envs": n, "frame": frame, "spp": spp, "repeats": repeats, "snapshot_bytes": size,
           "branch": ctx.env_last_step_branch(), "ms_per_step_median": float(np.median(step_ms)),
           "ms_per_step_windows": step_ms, "ms_per_step_after_median": float(np.median(after_ms)),
           "median_ms": medians, "all_ms": times,
           "gb_per_s": {name: size / value / 1e6 for name, value in medians.items()},
           "resident_vs_hipMemcpyDtoD": {name: medians[name] / medians["hipMemcpyDtoD_same_bytes"]
                                         for name in ("snapshot_resident", "restore_resident")}}
    print(json.dumps(out), flush=True)
    env.close()
    return out


def main():
    argv = list(sys.argv[1:])
    repeats, windows, steps = option(argv, "--repeats", 5), option(argv, "--windows", 5), option(argv, "--steps", 10)
    n, frame, spp = (int(a) for a in argv[:3]) if len(argv) >= 3 else (4096, 256, 16)
    bench(n, frame, spp, repeats, windows, steps)


if __name__ == "__main__":
    main()
