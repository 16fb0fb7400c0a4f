"""CPU tests of the boundary of a device step: the action rules of rf_env_io.h, compiled for the host (tests/iocheck),
against a numpy statement of the table in include/reinfocus_hip.h ("device io") on every edge of every dtype; the
arguments step_tensors refuses before the library is called; and the package staying torch-free."""

import ctypes
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from tests import helpers

I32, I64, F32 = _native.ACTION_I32, _native.ACTION_I64, _native.ACTION_F32
RULE_INDEX, RULE_JUMP, RULE_FINITE = range(3)  # rf::kActionRule*
NO_FAULT = 2 ** 64 - 1


@pytest.fixture(scope="module")
def iocheck():
    lib = ctypes.CDLL(helpers.built("tests/iocheck", "libiocheck.so"))
    lib.io_gather.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                              ctypes.c_void_p, ctypes.c_void_p]
    lib.io_gather.restype = ctypes.c_uint64
    return lib


def _gather(lib, actions, dtype, rule, n_actions, step=0):
    stored = np.full(len(actions), 0x5A5A5A5A, dtype=np.int32)
    valid = np.full(len(actions), 7, dtype=np.uint8)
    fault = lib.io_gather(actions.ctypes.data, dtype, rule, n_actions, len(actions), step, stored.ctypes.data,
                          valid.ctypes.data)
    return stored, valid.astype(bool), fault


def _want_fault(valid, step):
    bad = np.flatnonzero(~valid)
    return NO_FAULT if len(bad) == 0 else (step << 32) | int(bad[0])


# -- the table, stated in numpy ------------------------------------------------------------------------------------
def _index_rule(actions, n_actions):
    wide = actions.astype(object)  # (Python integers: no 64-bit wrap in the statement itself)
    valid = np.array([0 <= a < n_actions for a in wide])
    stored = np.array([a if ok else min(max(a, 0), n_actions - 1) for a, ok in zip(wide, valid)], dtype=np.int64)
    return stored.astype(np.int32), valid


def _jump_rule(actions):
    with np.errstate(invalid="ignore"):
        valid = (actions >= -1) & (actions <= 1)
        stored = np.where(np.isnan(actions), np.float32(0), np.clip(actions, np.float32(-1), np.float32(1)))
    return np.where(valid, actions, stored).astype(np.float32), valid


def _finite_rule(actions):
    valid = np.isfinite(actions)
    return np.where(valid, actions, np.float32(0)).astype(np.float32), valid


@pytest.mark.parametrize("n_actions", [1, 13, 32])
def test_int32_edges(n_actions, iocheck):
    info = np.iinfo(np.int32)
    actions = np.array([-1, 0, n_actions - 1, n_actions, info.min, info.max, 1, n_actions // 2, -2, n_actions + 1],
                       dtype=np.int32)
    stored, valid, fault = _gather(iocheck, actions, I32, RULE_INDEX, n_actions, step=5)
    want, want_valid = _index_rule(actions, n_actions)
    assert np.array_equal(valid, want_valid) and np.array_equal(stored, want)
    assert list(valid[:6]) == [False, True, True, False, False, False]
    assert stored[0] == 0 and stored[3] == n_actions - 1 and stored[4] == 0 and stored[5] == n_actions - 1
    assert fault == _want_fault(valid, 5) == (5 << 32)


@pytest.mark.parametrize("n_actions", [1, 13, 32])
def test_int64_is_judged_on_all_64_bits(n_actions, iocheck):
    info = np.iinfo(np.int64)
    actions = np.array([0, n_actions - 1, 2 ** 32, 2 ** 32 + 1, -2 ** 32, info.min, info.max, -1, n_actions,
                        2 ** 32 + n_actions - 1, 2 ** 63 - 2 ** 32], dtype=np.int64)
    stored, valid, fault = _gather(iocheck, actions, I64, RULE_INDEX, n_actions, step=2 ** 32 - 1)
    want, want_valid = _index_rule(actions, n_actions)
    assert np.array_equal(valid, want_valid) and np.array_equal(stored, want)
    assert list(valid) == [True, True] + [False] * 9  # (2^32 + 1 is invalid, not 1)
    assert stored[3] == n_actions - 1 and stored[4] == 0 and stored[5] == 0
    assert fault == _want_fault(valid, 2 ** 32 - 1) == ((2 ** 32 - 1) << 32) | 2
    # the same values that fit, as int32: the two dtypes agree
    fits = (actions >= -2 ** 31) & (actions < 2 ** 31)  # (not abs: INT64_MIN has none)
    stored32, valid32, _ = _gather(iocheck, actions[fits].astype(np.int32), I32, RULE_INDEX, n_actions)
    assert np.array_equal(stored32, stored[fits]) and np.array_equal(valid32, valid[fits])


def _float_edges():
    one = np.float32(1)
    tiny = np.float32(1e-45)  # the smallest subnormal
    return np.array([1, -1, np.nextafter(one, np.float32(np.inf)), np.nextafter(-one, np.float32(-np.inf)),
                     np.nextafter(one, np.float32(0)), np.nextafter(-one, np.float32(0)), 0.0, -0.0, np.inf, -np.inf,
                     np.nan, -np.nan, tiny, -tiny, np.float32(1.1754942e-38), 1.5, -1.5, 0.25, 3.4028235e38,
                     -3.4028235e38], dtype=np.float32)


def test_jump_edges(iocheck):
    actions = _float_edges()
    stored, valid, fault = _gather(iocheck, actions, F32, RULE_JUMP, 0, step=1)
    want, want_valid = _jump_rule(actions)
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(stored, want.view(np.int32))  # bit for bit: -0.0 stays -0.0, subnormals stay
    got = stored.view(np.float32)
    assert list(valid[:12]) == [True, True, False, False, True, True, True, True, False, False, False, False]
    assert got[2] == 1 and got[3] == -1 and got[8] == 1 and got[9] == -1 and got[10] == 0 and got[11] == 0
    assert not np.isnan(got).any() and np.all(np.abs(got) <= 1)
    assert fault == _want_fault(valid, 1) == (1 << 32) | 2


def test_finite_edges(iocheck):
    actions = _float_edges()
    stored, valid, fault = _gather(iocheck, actions, F32, RULE_FINITE, 0)
    want, want_valid = _finite_rule(actions)
    assert np.array_equal(valid, want_valid) and np.array_equal(stored, want.view(np.int32))
    assert int((~valid).sum()) == 4 and np.all(stored[~valid] == 0)  # +-inf, +-NaN -> +0.0
    assert fault == _want_fault(valid, 0) == 8


def test_random_actions_and_no_fault(iocheck):
    rng = np.random.default_rng(3)
    ints = rng.integers(-40, 60, 4000)
    for dtype, code in ((np.int32, I32), (np.int64, I64)):
        stored, valid, fault = _gather(iocheck, ints.astype(dtype), code, RULE_INDEX, 13, step=9)
        want, want_valid = _index_rule(ints.astype(dtype), 13)
        assert np.array_equal(stored, want) and np.array_equal(valid, want_valid) and fault == _want_fault(valid, 9)
    floats = rng.uniform(-2, 2, 4000).astype(np.float32)
    stored, valid, fault = _gather(iocheck, floats, F32, RULE_JUMP, 0, step=9)
    want, want_valid = _jump_rule(floats)
    assert np.array_equal(stored, want.view(np.int32)) and np.array_equal(valid, want_valid)
    assert fault == _want_fault(valid, 9)
    good = rng.integers(0, 13, 500).astype(np.int32)
    assert _gather(iocheck, good, I32, RULE_INDEX, 13, step=4)[2] == NO_FAULT


# -- step_tensors' refusals that need no GPU ------------------------------------------------------------------------
class _NoLibrary:
    """In place of the context: any call of the library is the failure."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name})")


def _io(n=6, float_actions=False, monkeypatch=None):
    from reinfocus_amd import torch_interop

    if monkeypatch is not None:  # (and nothing may get as far as asking about the runtime either)
        def called():
            raise AssertionError("the call went past the argument checks")
        monkeypatch.setattr(torch_interop, "check_one_runtime", called)
    return torch_interop.TensorIO(_NoLibrary(), n, 4, float_actions, 0)


def test_step_tensors_refuses_bad_arguments_before_the_library(monkeypatch):
    import torch

    n = 6
    io = _io(n, monkeypatch=monkeypatch)
    with pytest.raises(ValueError, match="live on cpu"):  # everything right but the device
        io.step(torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError, match="live on cpu"):
        io.step(torch.zeros((n, 1), dtype=torch.int64))
    for dtype in (torch.float32, torch.float64, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(TypeError, match="the task takes"):
            io.step(torch.zeros(n, dtype=dtype))
    for shape in ((n + 1,), (n - 1,), (n, 2), (1, n), (), (n, 1, 1)):
        with pytest.raises(ValueError, match="shape"):
            io.step(torch.zeros(shape, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        io.step(torch.zeros(2 * n, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="contiguous"):
        io.step(torch.zeros((n, 2), dtype=torch.int64)[:, :1])
    for other in (np.zeros(n, dtype=np.int32), [0] * n, None):
        with pytest.raises(TypeError, match="torch.Tensor"):
            io.step(other)
    floats = _io(n, float_actions=True, monkeypatch=monkeypatch)
    for dtype in (torch.float64, torch.float16, torch.int32, torch.int64):  # (float64: the caller casts)
        with pytest.raises(TypeError, match="the task takes"):
            floats.step(torch.zeros(n, dtype=dtype))
    with pytest.raises(ValueError, match="live on cpu"):
        floats.step(torch.zeros((n, 1), dtype=torch.float32))
    with pytest.raises(ValueError, match="live on meta"):  # (another device than the environment's)
        io.step(torch.zeros(n, dtype=torch.int32, device="meta"))


def test_sharded_classes_say_why_they_have_no_tensor_methods():
    from reinfocus_amd.environments import harness

    for cls in (harness.ShardedVectorDiscreteSteps, harness.ShardedVectorContinuousJumps):
        for name in ("reset_tensors", "step_tensors", "device_fault", "last_reset_count"):
            with pytest.raises(ValueError, match="one GPU"):
                getattr(cls, name)(object.__new__(cls))


def test_importing_the_package_does_not_import_torch():
    """In a fresh interpreter (this one may hold torch already): the package, its binding and the environments."""
    code = ("import sys; import reinfocus_amd; from reinfocus_amd import _native; "
            "from reinfocus_amd.environments import harness; import reinfocus_amd.torch_interop; "
            "assert 'torch' not in sys.modules, 'torch was imported'; print('ok')")
    done = subprocess.run([sys.executable, "-c", code], cwd=helpers.ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]


def test_one_runtime_check_counts_mappings(monkeypatch):
    from reinfocus_amd import torch_interop

    monkeypatch.setattr(torch_interop, "_one_runtime_checked", False)
    monkeypatch.setattr(torch_interop, "hip_runtimes", lambda: ["/a/libamdhip64.so", "/b/libamdhip64.so.7"])
    with pytest.raises(RuntimeError, match="2 HIP runtimes"):
        torch_interop.check_one_runtime()
    monkeypatch.setattr(torch_interop, "hip_runtimes", lambda: ["/a/libamdhip64.so"])
    torch_interop.check_one_runtime()
    assert isinstance(torch_interop.hip_runtimes(), list)
