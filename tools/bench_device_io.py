"""Host-form step() against step_tensors() of one DeviceVectorDiscreteSteps environment (device_initializer=True), in
one process: medians of six alternating windows of ten steps each, per shape.  Actions come from a device-side
torch.randint; the host form gets them as numpy (the download is part of what it costs a torch user), the device form
as they are.  A host-form window synchronises in every step by construction; a device-form window ends in ONE
torch.cuda.synchronize().  Record only: nothing here is a gate.

    python tools/bench_device_io.py [--out profiles/device_io.md] [--shapes 4096x256x16,8x300x100,1x64x1]
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402 -- before the library is loaded: one HIP runtime per process (reinfocus_amd/torch_interop.py)

WINDOWS, STEPS = 6, 10


def measure(n, frame, spp):
    from reinfocus_amd.environments import harness

    env = harness.DeviceVectorDiscreteSteps(num_envs=n, frame_height=frame, samples_per_pixel=spp, seed=1, device=0,
                                            device_initializer=True)
    env.reset_tensors()
    actions = [torch.randint(0, 13, (n,), device="cuda", dtype=torch.int64) for _ in range(STEPS)]
    for a in actions[:3]:  # both forms past their first, uncaptured steps
        env.step(a.cpu().numpy())
        env.step_tensors(a)
    torch.cuda.synchronize()
    host, device = [], []
    for _ in range(WINDOWS):
        start = time.perf_counter()
        for a in actions:
            env.step(a.cpu().numpy())
        host.append((time.perf_counter() - start) / STEPS)
        start = time.perf_counter()
        for a in actions:
            env.step_tensors(a)
        torch.cuda.synchronize()
        device.append((time.perf_counter() - start) / STEPS)
    fault = env.device_fault()
    branch = env._ctx.env_last_step_branch()
    env.close()
    assert fault is None, fault
    return statistics.median(host) * 1e3, statistics.median(device) * 1e3, branch


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None)
    parser.add_argument("--shapes", default="4096x256x16,8x300x100,1x64x1")
    args = parser.parse_args()
    torch.zeros(1, device="cuda")
    lines = ["# Device io: `step()` against `step_tensors()`", "",
             f"`tools/bench_device_io.py` on {torch.cuda.get_device_name(0)}: one `DeviceVectorDiscreteSteps` "
             f"(`device_initializer=True`) per shape, medians of {WINDOWS} alternating windows of {STEPS} steps, wall "
             "time per step.  The host form downloads the actions torch made on the device and synchronises in every "
             "step; the device form's window ends in one `torch.cuda.synchronize()`.", "",
             "| envs x frame x spp | `step()` ms | `step_tensors()` ms | ratio | schedule |", "|---|---|---|---|---|"]
    for shape in args.shapes.split(","):
        n, frame, spp = (int(v) for v in shape.split("x"))
        host_ms, device_ms, branch = measure(n, frame, spp)
        lines.append(f"| {n} x {frame}^2 x {spp} | {host_ms:.3f} | {device_ms:.3f} | {host_ms / device_ms:.2f} | {branch} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as out:
            out.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
