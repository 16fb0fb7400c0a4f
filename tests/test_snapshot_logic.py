"""CPU tests of environment snapshots: the file form of an EnvSnapshot (one .npz: the blob and JSON metadata, no pickle),
what load() refuses, the six exports in header, binding and library, and -- with the GPU's render and focus measure
replaced by a function of the state -- that the seeds of tests/test_gpu_snapshot.py give what those tests assert before
they compare anything: steps that end a part of the environments before and after every snapshot.  (Which environments
end depends on their states alone, so the host twin with a fake focus value ends the same ones.)"""

import json
import os
import zipfile

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness
from reinfocus_amd.environments import snapshot
from tests import test_gpu_snapshot as gpu
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture
from tests.test_gpu_device_initializer import KW, _objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["rf_env_snapshot_size", "rf_env_snapshot", "rf_env_restore", "rf_env_snapshot_resident",
           "rf_env_restore_resident", "rf_env_snapshot_drop"]
GENERATOR = {"bit_generator": "PCG64DXSM", "state": {"state": (1 << 127) + 12345, "inc": (1 << 126) + 7}, "has_uint32": 0,
             "uinteger": 0}


def _synthetic(generator=GENERATOR):
    blob = np.random.default_rng(3).integers(0, 256, 5000, dtype=np.uint8)
    return snapshot.EnvSnapshot(blob, "DeviceVectorDiscreteSteps", 65, 16, 2, generator)


@pytest.mark.parametrize("generator", [GENERATOR, None])
def test_save_and_load_round_trip_exactly(generator, tmp_path):
    snap = _synthetic(generator)
    path = tmp_path / "run.snapshot"  # (the name is kept as given: no suffix is added)
    snap.save(path)
    assert os.listdir(tmp_path) == ["run.snapshot"]
    back = snapshot.EnvSnapshot.load(path)
    assert back.blob.dtype == np.uint8 and np.array_equal(back.blob, snap.blob)
    assert (back.env_class, back.num_envs, back.frame_height, back.samples_per_pixel) == \
        ("DeviceVectorDiscreteSteps", 65, 16, 2)
    assert back.host_generator == generator and back.describe() == snap.describe()
    if generator is not None:  # numpy takes the state as it came back
        bit_generator = np.random.PCG64DXSM(0)
        bit_generator.state = back.host_generator
        assert bit_generator.state == generator


def test_the_file_is_arrays_and_json_without_pickle(tmp_path):
    path = tmp_path / "run.npz"
    _synthetic().save(path)
    with zipfile.ZipFile(path) as archive:
        assert sorted(archive.namelist()) == ["blob.npy", "meta.npy"]
    with np.load(path, allow_pickle=False) as data:  # (an object array would need pickle)
        meta = json.loads(str(data["meta"]))
    assert meta["host_generator"]["state"] == hex(GENERATOR["state"]["state"]) and meta["num_envs"] == 65


def test_load_refuses_what_is_not_a_snapshot(tmp_path):
    snap = _synthetic()
    meta = np.array(json.dumps(snap._meta()))
    files = {"no blob": dict(meta=meta), "no metadata": dict(blob=snap.blob),
             "a foreign key": dict(blob=snap.blob, meta=meta, extra=np.zeros(3)),
             "a blob of floats": dict(blob=snap.blob.astype(np.float32), meta=meta),
             "a blob of two dimensions": dict(blob=snap.blob.reshape(50, 100), meta=meta),
             "metadata that is not JSON": dict(blob=snap.blob, meta=np.array("{")),
             "metadata that is not text": dict(blob=snap.blob, meta=np.zeros(4)),
             "metadata with a foreign entry": dict(blob=snap.blob, meta=np.array(json.dumps({**snap._meta(), "x": 1}))),
             "metadata without the shape": dict(blob=snap.blob, meta=np.array(json.dumps({"format": 1}))),
             "another file format": dict(blob=snap.blob, meta=np.array(json.dumps({**snap._meta(), "format": 2}))),
             "a malformed generator": dict(blob=snap.blob,
                                           meta=np.array(json.dumps({**snap._meta(), "host_generator": {"state": "zz"}})))}
    for what, arrays in files.items():
        path = tmp_path / "bad.npz"
        with open(path, "wb") as file:
            np.savez(file, **arrays)
        with pytest.raises(ValueError, match="bad.npz"):
            snapshot.EnvSnapshot.load(path)
    with open(tmp_path / "pickled.npz", "wb") as file:  # an object array is never unpickled
        np.savez(file, blob=snap.blob, meta=np.array({"format": 1}, dtype=object))
    with pytest.raises(ValueError):
        snapshot.EnvSnapshot.load(tmp_path / "pickled.npz")


def test_a_snapshot_takes_only_a_flat_uint8_blob():
    with pytest.raises(AssertionError):
        snapshot.EnvSnapshot(np.zeros(8, dtype=np.float32), "X", 1, 16, 1)
    with pytest.raises(AssertionError):
        snapshot.EnvSnapshot(np.zeros((2, 4), dtype=np.uint8), "X", 1, 16, 1)


def test_the_six_exports_are_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    lib = _native.load()
    for name in EXPORTS:
        assert f"int {name}(rf_ctx *" in header and name in _native.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert "#define RF_ENV_SNAPSHOT_SLOTS 4" in header
    for method in ("env_snapshot", "env_restore", "env_snapshot_resident", "env_restore_resident", "env_snapshot_drop"):
        assert callable(getattr(_native.Context, method))


def test_environments_have_the_methods_and_the_numpy_twins_do_not():
    methods = ("snapshot", "restore", "snapshot_resident", "restore_resident", "drop_snapshot")
    for cls in (harness.DeviceVectorDiscreteSteps, harness.DeviceVectorContinuousJumps, harness.DeviceVectorEnvironment,
                harness.ShardedVectorDiscreteSteps, harness.ShardedVectorContinuousJumps):
        assert all(callable(getattr(cls, m)) for m in methods), cls
    for cls in (harness.VectorDiscreteSteps, harness.VectorContinuousJumps, harness.VectorEnvironment):
        assert not any(hasattr(cls, m) for m in methods), cls


# ---- the GPU tests' seeds ---------------------------------------------------------------------------------------------
def _ended(host, actions):
    """How many environments ended in each step of the twin."""
    ended = []
    for action in actions:
        action = action(host._state) if callable(action) else action
        ended.append(int(host.step(action)[3].sum()))
    return ended


def _twin(n, ender="limit"):
    host = harness.VectorEnvironment(**_objects(n, "multi", gpu.SEED, ender), **KW)
    host.reset()
    return host


@pytest.mark.parametrize("n", [1, 65, 1100])
def test_seeds_of_the_rewind_and_resume_tests(n, no_gpu):  # noqa: F811
    half = gpu.HALF
    ended = _ended(_twin(n), gpu.index_actions(n))
    assert gpu.some_partial(ended[:half], n) and gpu.some_partial(ended[half:], n), ended
    host = _twin(n)
    _ended(host, gpu.index_actions(n)[:half])
    other = _ended(host, gpu.index_actions(n, gpu.OTHER_ACTION_SEED, half))
    assert gpu.some_partial(other, n), other


@pytest.mark.parametrize("kind", gpu.KINDS)
def test_seeds_of_every_kind_of_context(kind, no_gpu):  # noqa: F811
    n = 65
    if kind == "two delta observers":  # (the tree needs a real FocusObserver; which environments end does not)
        host = harness.VectorEnvironment(**gpu.observed_strategies(n, 4), **KW)  # (rewards do not decide who ends)
        make_actions = lambda rng: (lambda state: rng.integers(0, 13, n))  # noqa: E731
    else:
        host, _, _, make_actions = _host_only(kind, n)
    host.reset()
    action = make_actions(np.random.default_rng(gpu.ACTION_SEED))
    ended = _ended(host, [action] * (2 * gpu.HALF))
    assert gpu.some_partial(ended[:gpu.HALF], n) and gpu.some_partial(ended[gpu.HALF:], n), ended


def _host_only(kind, n):
    """The host twin of gpu._kind without its device environment (which needs a GPU)."""
    from tests.test_continuous_vector_logic import _actions

    index = lambda rng: (lambda state: rng.integers(0, 13, n))  # noqa: E731
    kw = dict(num_envs=n, **gpu.TASK_KW)
    if kind.startswith("discrete steps"):
        return harness.VectorDiscreteSteps(**kw), None, [], index
    if kind == "continuous jumps":
        return harness.VectorContinuousJumps(**kw), None, [], lambda rng: (lambda state: _actions(rng, state))
    assert kind == "stopped + delta"
    return harness.VectorEnvironment(**gpu.stopped_objects(n), **KW), None, [], index


def test_seeds_of_the_slot_and_render_tests(no_gpu):  # noqa: F811
    n = 65
    ended = _ended(_twin(n), gpu.index_actions(n, steps=10))
    assert all(gpu.some_partial(part, n) for part in (ended[:3], ended[3:6], ended[6:])), ended
    assert any(0 < k < n for k in ended[2:8]), ended  # (the render test's compacted point: steps 3 to 8)
    assert _ended(_twin(n, "never"), gpu.index_actions(n, steps=4)) == [0, 0, 0, 0]
