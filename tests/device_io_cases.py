"""TEST INFRASTRUCTURE: the child process of tests/test_gpu_device_io.py.

One process can hold one HIP runtime (reinfocus_amd/torch_interop.py), and the pytest process has loaded the library --
with the ROCm installation's runtime -- long before a test could import torch.  So everything that needs torch and the
library together runs here, in a fresh process that imports torch first: every case of the device-io tests, each
recorded as one JSON line {"id", "ok", "message"} in the file given on the command line; the pytest side starts this
once, and its tests look their cases up.  A failed comparison is recorded and the run goes on; anything else (a HIP
error above all) ends the run at once, and the cases that never ran fail on the pytest side for that reason.

    python -m tests.device_io_cases cases <results.jsonl>
    python -m tests.device_io_cases order <torch-first | library-first> <results.json>
"""

import contextlib
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(frame_height=16, device=0)
N_SIZES = (1, 65, 1100)  # one lane, past a wave, past the reset kernel's 1024-lane loop
CLASSES = {"steps-i32": "int32", "steps-i64": "int64", "jumps-f32": "float32", "composed-i32": "int32",
           "composed-i64": "int64", "observed12-i64": "int64"}
ORDER_N, ORDER_STEPS, ORDER_SEED = 65, 3, 17


def _imports(order):
    if order == "torch-first":
        import torch

        torch.zeros(1, device="cuda")
        import reinfocus_amd  # noqa: F401
    else:
        import reinfocus_amd  # noqa: F401
        import torch

        torch.zeros(1, device="cuda")
    return torch


def make_env(kind, n, seed=13, branch=None, spp=None, **extra):
    """A device environment of `kind` with a device initializer, created under the knobs of step schedule `branch`."""
    from reinfocus_amd.environments import harness
    from tests.test_gpu_environment import STEP_BRANCHES

    knobs = STEP_BRANCHES[branch] if branch else {}
    spp = 1 + n % 2 if spp is None else spp
    os.environ.update(knobs)
    try:
        family = kind.split("-")[0]
        if family in ("steps", "jumps"):
            cls = harness.DeviceVectorDiscreteSteps if family == "steps" else harness.DeviceVectorContinuousJumps
            return cls(max_episode_steps=3, num_envs=n, seed=seed, samples_per_pixel=spp, device_initializer=True,
                       **{**KW, **extra})
        from tests.test_gpu_device_initializer import _objects

        if family == "composed":  # TimeLimitEnder(3) | DivergingEnder
            return harness.DeviceVectorEnvironment(**_objects(n, "multi", seed), samples_per_pixel=spp,
                                                   device_initializer=True, **{**KW, **extra})
        from reinfocus_amd.graphics import render
        from tests.test_gpu_observed_env import _tree

        renderer = render.FastRenderer(samples_per_pixel=spp, device=0)
        observer = _tree("delta of delta", n, renderer, KW["frame_height"])  # 12 columns
        objects = _objects(n, "multi", seed)
        return harness.DeviceVectorEnvironment(**objects, observer=observer, device_initializer=True, **extra)
    finally:
        for key in knobs:
            del os.environ[key]


def host_actions(kind, rng, n):
    """One step's actions as numpy, in the dtype the case hands to step_tensors."""
    dtype = CLASSES[kind]
    if dtype == "float32":
        return rng.uniform(-1, 1, n).astype(np.float32)
    return rng.integers(0, 13, n).astype(dtype)


def everything(env):
    """What the issue compares after every step besides the step's results."""
    parts = [env._state]
    if hasattr(env, "strategy_state"):
        parts += list(env.strategy_state())
    if getattr(env, "_observed", False):
        parts.append(env.observer_state())
    return parts, env.initializer_state()


def same_step(got, want, torch):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float64 and got[2].dtype == torch.bool
    assert got[3].dtype == torch.bool and got[4] == {}
    assert not bool(got[2].any())
    for index, (x, y) in enumerate(zip(got[:4], want[:4])):
        x = x.cpu().numpy()
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f"result {index} differs"


def same_everything(a, b):
    (parts_a, gen_a), (parts_b, gen_b) = everything(a), everything(b)
    assert gen_a == gen_b, "the initializers' generators differ"
    for index, (x, y) in enumerate(zip(parts_a, parts_b)):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True), f"state {index} differs"


class Recorder:
    def __init__(self, path):
        self._out = open(path, "w")

    @contextlib.contextmanager
    def case(self, name):
        record = {"id": name, "ok": True, "message": ""}
        fatal = None
        try:
            yield
        except AssertionError:
            record.update(ok=False, message=traceback.format_exc()[-1500:])
        except BaseException as error:  # noqa: BLE001 -- (a HIP error: nothing more runs on the GPU in this process)
            record.update(ok=False, message="FATAL " + traceback.format_exc()[-1500:])
            fatal = error
        self._out.write(json.dumps(record) + "\n")
        self._out.flush()
        if fatal is not None:
            sys.exit(3)


# ---- 1: equality with the host form -------------------------------------------------------------------------------
def equality_case(torch, kind, n, branch):
    from tests.test_gpu_environment import BRANCH_NAME, FIRST_STEP_BRANCH

    host = make_env(kind, n, branch=branch)
    dev = make_env(kind, n, branch=branch)
    try:
        o_h, _ = host.reset()
        o_d, info = dev.reset_tensors()
        assert info == {} and o_d.dtype == torch.float32 and np.array_equal(o_h, o_d.cpu().numpy())
        same_everything(host, dev)
        rng = np.random.default_rng(6)
        name = BRANCH_NAME.get(branch, branch)
        name = {"count-sized": "one-sync"}.get(name, name)  # (a device step never takes the count-sized schedule)
        ended = []
        for step in range(12):
            actions = host_actions(kind, rng, n)
            want = host.step(actions)
            shaped = actions.reshape(n, 1) if step % 3 == 2 else actions  # ([n, 1] as well as [n])
            got = dev.step_tensors(torch.from_numpy(shaped).cuda())
            same_step(got, want, torch)
            same_everything(host, dev)
            assert dev._ctx.env_last_step_branch() == (FIRST_STEP_BRANCH.get(name, name) if step == 0 else name)
            assert dev.last_reset_count() == int(want[3].sum())
            ended.append(int(want[3].sum()))
        assert sum(ended) > 0, ended
        assert dev.device_fault() is None
    finally:
        host.close()
        dev.close()


# ---- 2: no baked pointers -----------------------------------------------------------------------------------------
def pointers_case(torch):
    n = 65
    host, dev = make_env("steps-i64", n), make_env("steps-i64", n)
    host.reset()
    first = dev.reset_tensors()[0]
    device = first.device
    slots = [torch.empty(n, dtype=torch.int64, device=device) for _ in range(2)]
    outs = [(torch.empty((n, 4), dtype=torch.float32, device=device), torch.empty(n, dtype=torch.float64, device=device),
             torch.empty(n, dtype=dtype, device=device)) for dtype in (torch.bool, torch.uint8)]
    rng = np.random.default_rng(2)
    for step in range(8):
        actions = host_actions("steps-i64", rng, n)
        want = host.step(actions)
        slots[step % 2].copy_(torch.from_numpy(actions))
        got = dev.step_tensors(slots[step % 2], out=outs[step % 2])
        same_step(got, want, torch)
        assert got[0].data_ptr() == outs[step % 2][0].data_ptr() and got[3].data_ptr() == outs[step % 2][2].data_ptr()
        if step:
            assert dev._ctx.env_last_step_branch() == "fused-graph"
    owned = None
    for step in range(4):  # the environment's own outputs: one set, overwritten in place
        actions = host_actions("steps-i64", rng, n)
        want = host.step(actions)
        got = dev.step_tensors(torch.from_numpy(actions).cuda())
        same_step(got, want, torch)
        pointers = [t.data_ptr() for t in got[:4]]
        assert owned is None or owned == pointers
        owned = pointers
    assert owned[0] == first.data_ptr()
    same_everything(host, dev)
    host.close()
    dev.close()


# ---- 3: stream ordering -------------------------------------------------------------------------------------------
def stream_case(torch):
    n = 65
    host, dev = make_env("steps-i32", n), make_env("steps-i32", n)
    host.reset()
    dev.reset_tensors()
    rng = np.random.default_rng(4)
    stream = torch.cuda.Stream()
    ballast = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device="cuda")  # a 256 MB fill in front of the actions
    wanted, kept = [], []
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for step in range(8):
            actions = host_actions("steps-i32", rng, n)
            wanted.append((actions, None))
            staged = torch.from_numpy(actions).pin_memory()
            ballast.fill_(float(step))
            on_device = staged.to("cuda", non_blocking=True) + 0  # produced on `stream`, after the fill
            got = dev.step_tensors(on_device)
            kept.append([t.clone() for t in got[:4]])  # consumed on `stream`, no host synchronisation
    torch.cuda.synchronize()
    for (actions, _), got in zip(wanted, kept):
        same_step(got + [{}], host.step(actions), torch)
    same_everything(host, dev)
    host.close()
    dev.close()


# ---- 4: mixing ----------------------------------------------------------------------------------------------------
def mixing_case(torch):
    n = 65
    host, dev = make_env("composed-i64", n), make_env("composed-i64", n)
    host.reset()
    dev.reset_tensors()
    rng = np.random.default_rng(8)

    def both(form):
        actions = host_actions("composed-i64", rng, n)
        want = host.step(actions)
        if form == "tensors":
            same_step(dev.step_tensors(torch.from_numpy(actions).cuda()), want, torch)
        else:
            got = dev.step(actions)
            assert all(np.array_equal(x, y) for x, y in zip(got[:4], want[:4]))
        same_everything(host, dev)
        return actions, want

    for form in ("tensors", "host", "tensors"):
        both(form)
    assert np.array_equal(host.render_frames(), dev.render_frames())  # (the deferred scene length)
    # (the 600 px render drew from the RNG states of both alike; go on from there)
    snap = dev.snapshot()
    host_snap = host.snapshot()
    assert np.array_equal(snap.blob, host_snap.blob)
    replay = [both("tensors") for _ in range(3)]
    after = everything(dev)
    dev.restore(snap)
    host.restore(host_snap)
    for actions, want in replay:
        same_step(dev.step_tensors(torch.from_numpy(actions).cuda()), want, torch)
    again = everything(dev)
    assert after[1] == again[1] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(after[0], again[0]))
    for actions, _ in replay:  # (the host twin replays too, so that the frames below are of the same step)
        host.step(actions)
    assert np.array_equal(host.render_frames(), dev.render_frames())
    host.close()
    dev.close()


# ---- 5: faults ----------------------------------------------------------------------------------------------------
def fault_case(torch, kind, bad):
    """bad: {env: value} put into the actions of step 2 (of 0, 1, 2); the lowest environment is the one reported."""
    n = 65
    dev = make_env(kind, n)
    dev.reset_tensors()
    rng = np.random.default_rng(1)
    dtype = {"int32": torch.int32, "int64": torch.int64, "float32": torch.float32}[CLASSES[kind]]
    for step in range(3):
        actions = torch.from_numpy(host_actions(kind, rng, n)).cuda()
        if step == 2:
            for env, value in bad.items():
                actions[env] = torch.tensor(value, dtype=dtype)
        dev.step_tensors(actions)
    good = torch.from_numpy(host_actions(kind, rng, n)).cuda()
    for _ in range(2):  # nobody has asked yet: further steps return without error
        out = dev.step_tensors(good)
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())
    assert dev.device_fault() == (2, min(bad)), dev.device_fault()
    assert dev.device_fault() == (2, min(bad))  # sticky
    for call in (lambda: dev.step(good.cpu().numpy()), lambda: dev.step_tensors(good), dev.snapshot):
        try:
            call()
        except AssertionError as error:
            assert "step 2" in str(error) and f"environment {min(bad)}" in str(error), str(error)
        else:
            raise AssertionError("a call was not refused after the fault was seen")
    dev.reset_tensors()
    assert dev.device_fault() is None
    dev.step_tensors(good)
    dev.step(good.cpu().numpy())
    assert dev.device_fault() is None
    dev.snapshot()
    dev.close()


def host_sees_fault_case(torch):
    """A host-form step after a device step with an invalid action resolves, and is refused itself."""
    n = 65
    dev = make_env("steps-i32", n)
    dev.reset()
    bad = torch.zeros(n, dtype=torch.int32, device="cuda")
    bad[7] = 13
    dev.step_tensors(bad)
    try:
        dev.step(np.zeros(n, dtype=np.int32))
    except AssertionError as error:
        assert "step 0" in str(error) and "environment 7" in str(error)
    else:
        raise AssertionError("the host-form step ran")
    dev.reset()
    dev.step(np.zeros(n, dtype=np.int32))
    assert dev.device_fault() is None
    dev.close()


# ---- 6: refusals --------------------------------------------------------------------------------------------------
def refusal_case(torch):
    from reinfocus_amd.environments import harness

    n = 12
    kw = dict(max_episode_steps=3, num_envs=n, seed=3, samples_per_pixel=2, **KW)
    actions = torch.zeros(n, dtype=torch.int32, device="cuda")

    def refused(call, error, match):
        try:
            call()
        except error as caught:
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")

    plain = harness.DeviceVectorDiscreteSteps(**kw)
    plain.reset()
    refused(lambda: plain.step_tensors(actions), ValueError, "device_initializer=False")
    refused(plain.reset_tensors, ValueError, "device_initializer=False")
    out = torch.empty((n, 4), device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"), \
        torch.empty(n, dtype=torch.uint8, device="cuda")
    refused(lambda: plain._ctx.env_step_device(actions.data_ptr(), 0, out[0].data_ptr(), out[1].data_ptr(),
                                               out[2].data_ptr(), None, 0), AssertionError, "no device initializer")
    plain.step(np.zeros(n, dtype=np.int32))
    plain.close()
    drawn = harness.DeviceVectorDiscreteSteps(render_mode="rgb_array", device_initializer=True, **kw)
    drawn.reset()
    refused(lambda: drawn.step_tensors(actions), ValueError, "render_mode")
    drawn.step(np.zeros(n, dtype=np.int32))
    drawn.close()
    sharded = harness.ShardedVectorDiscreteSteps(devices=[0, 0], **{k: v for k, v in kw.items() if k != "device"})
    sharded.reset()
    refused(lambda: sharded.step_tensors(actions), ValueError, "one GPU")
    sharded.step(np.zeros(n, dtype=np.int32))
    sharded.close()
    dev = harness.DeviceVectorDiscreteSteps(device_initializer=True, **kw)
    twin = harness.DeviceVectorDiscreteSteps(device_initializer=True, **kw)
    dev.reset_tensors()
    twin.reset()
    before = everything(dev)
    refused(lambda: dev.step_tensors(actions.cpu()), ValueError, "live on cpu")
    refused(lambda: dev.step_tensors(actions.float()), TypeError, "the task takes")
    refused(lambda: dev.step_tensors(actions, out=(out[0].cpu(), out[1], out[2])), ValueError, "live on cpu")
    # the library's own refusals, past Python: host memory, the other action kind
    host_array = np.zeros(n, dtype=np.int32)
    refused(lambda: dev._ctx.env_step_device(host_array.ctypes.data, 0, out[0].data_ptr(), out[1].data_ptr(),
                                             out[2].data_ptr(), None, 0), AssertionError, "not device memory")
    refused(lambda: dev._ctx.env_step_device(actions.data_ptr(), 0, host_array.ctypes.data, out[1].data_ptr(),
                                             out[2].data_ptr(), None, 0), AssertionError, "not device memory")
    refused(lambda: dev._ctx.env_step_device(actions.data_ptr(), 2, out[0].data_ptr(), out[1].data_ptr(),
                                             out[2].data_ptr(), None, 0), AssertionError, "RF_ACTION_I32")
    short = torch.empty(n - 1, dtype=torch.int32, device="cuda")
    refused(lambda: dev.step_tensors(short), ValueError, "shape")
    after = everything(dev)
    assert before[1] == after[1] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before[0], after[0]))
    want = twin.step(np.zeros(n, dtype=np.int32))
    same_step(dev.step_tensors(actions), want, torch)  # ... and the environment still steps
    dev.close()
    twin.close()


def run_cases(path):
    torch = _imports("torch-first")
    from reinfocus_amd import torch_interop
    from tests.test_gpu_environment import STEP_BRANCHES

    record = Recorder(path)
    with record.case("one-runtime"):
        assert len(torch_interop.hip_runtimes()) == 1, torch_interop.hip_runtimes()
    for kind in CLASSES:
        for n in ((65,) if kind.startswith("observed") else N_SIZES):
            for branch in STEP_BRANCHES:
                with record.case(f"equal/{kind}/{n}/{branch}"):
                    equality_case(torch, kind, n, branch)
    with record.case("pointers"):
        pointers_case(torch)
    with record.case("stream"):
        stream_case(torch)
    with record.case("mixing"):
        mixing_case(torch)
    with record.case("fault/int32"):
        fault_case(torch, "steps-i32", {64: 13, 3: -1})
    with record.case("fault/int64"):
        fault_case(torch, "composed-i64", {40: 2 ** 32 + 1, 9: 2 ** 32 + 1})
    with record.case("fault/nan"):
        fault_case(torch, "jumps-f32", {20: float("nan"), 30: 1.5})
    with record.case("fault/1.5"):
        fault_case(torch, "jumps-f32", {33: 1.5})
    with record.case("fault/host-sees-it"):
        host_sees_fault_case(torch)
    with record.case("refusals"):
        refusal_case(torch)
    with record.case("finished"):
        pass


def run_order(order, path):
    torch = _imports(order)
    from reinfocus_amd import torch_interop

    dev = make_env("steps-i64", ORDER_N, seed=ORDER_SEED)
    rng = np.random.default_rng(ORDER_SEED)
    observations = [dev.reset_tensors()[0].cpu().numpy().tolist()]
    for _ in range(ORDER_STEPS):
        actions = host_actions("steps-i64", rng, ORDER_N)
        observations.append(dev.step_tensors(torch.from_numpy(actions).cuda())[0].cpu().numpy().tolist())
    dev.close()
    json.dump({"order": order, "runtimes": torch_interop.hip_runtimes(), "observations": observations}, open(path, "w"))
    print(json.dumps(observations[-1][:2]))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "cases":
        run_cases(sys.argv[2])
    else:
        run_order(sys.argv[2], sys.argv[3])
