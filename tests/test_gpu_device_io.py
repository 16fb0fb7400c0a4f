"""GPU tests of device io (rf_env_step_device, step_tensors): a device-resident environment stepped from torch tensors
on its own GPU, without a host synchronisation, against the same environment stepped through the host form.

One process holds one HIP runtime, and this process loaded the library long before it could import torch
(reinfocus_amd/torch_interop.py), so the cases run in ONE fresh child process that imports torch first
(tests/device_io_cases.py): started once per session, every case recorded, each test below looks its case up.

Development run on an MI355X: all 107 tests pass, the child process takes 5 s."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import device_io_cases as cases
from tests import helpers
from tests.test_gpu_environment import STEP_BRANCHES

pytestmark = pytest.mark.gpu


def _child(arguments, timeout):
    """A fresh process (never an exec of this one), ended by its own time limit."""
    return subprocess.run([sys.executable, "-m", "tests.device_io_cases", *arguments], cwd=helpers.ROOT,
                          capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("device_io") / "cases.jsonl")
    done = _child(["cases", path], 600)
    records = {}
    if os.path.exists(path):
        for line in open(path):
            record = json.loads(line)
            records[record["id"]] = record
    return records, f"exit status {done.returncode}\n{done.stderr[-3000:]}"


def _passed(recorded, name):
    records, ending = recorded
    assert name in records, f"the child process ended before case {name}: {ending}"
    assert records[name]["ok"], records[name]["message"]


def test_child_ran_every_case_on_one_runtime(recorded):
    _passed(recorded, "one-runtime")
    _passed(recorded, "finished")


@pytest.mark.parametrize("branch", list(STEP_BRANCHES))
@pytest.mark.parametrize("n", cases.N_SIZES)
@pytest.mark.parametrize("kind", [k for k in cases.CLASSES if not k.startswith("observed")])
def test_device_steps_equal_the_host_form(kind, n, branch, recorded):
    """Two equal environments (device_initializer=True, one seed), one stepped with step(actions.cpu().numpy()), one
    with step_tensors(actions): observations, rewards, flags, states, strategy state and the generator bit for bit
    after reset and after each of 12 steps of TimeLimitEnder(3) | DivergingEnder, on every step schedule -- under the
    count-sized settings the device form reports one-sync --, for the three classes, int32 and int64 indices."""
    _passed(recorded, f"equal/{kind}/{n}/{branch}")


@pytest.mark.parametrize("branch", list(STEP_BRANCHES))
def test_device_steps_equal_the_host_form_with_a_12_column_observer(branch, recorded):
    _passed(recorded, f"equal/observed12-i64/65/{branch}")


def test_no_pointer_is_baked_into_the_replayed_graph(recorded):
    """Two action tensors and two out= sets alternate under the fused-graph schedule for 8 steps; the environment's
    own outputs are overwritten in place."""
    _passed(recorded, "pointers")


def test_steps_are_ordered_against_the_callers_stream(recorded):
    """Actions produced on a non-default stream behind a 256 MB fill, results cloned on that stream, one
    synchronisation at the very end: all 8 steps equal the host form."""
    _passed(recorded, "stream")


def test_host_and_device_steps_mix(recorded):
    """step_tensors, step, step_tensors, render_frames, snapshot, three step_tensors, restore, the same three: the
    replay and the 600 px frames equal the host form's."""
    _passed(recorded, "mixing")


@pytest.mark.parametrize("case", ["int32", "int64", "nan", "1.5", "host-sees-it"])
def test_invalid_actions_are_recorded_and_sticky(case, recorded):
    """n = 65, invalid actions in step 2: device_fault() names step 2 and the lowest environment; two further steps run
    before anybody asks; afterwards step, step_tensors and snapshot raise until reset_tensors()."""
    _passed(recorded, f"fault/{case}")


def test_refusals_come_before_anything_runs(recorded):
    _passed(recorded, "refusals")


def test_both_import_orders_share_one_runtime_and_equal_the_host_form(tmp_path):
    """Two fresh processes: torch first (with a tensor on the GPU) and then the package, and the reverse.  Each runs a
    reset and three step_tensors steps; their observations equal each other and the host form's, computed here."""
    from reinfocus_amd.environments import harness

    n = cases.ORDER_N
    host = harness.DeviceVectorDiscreteSteps(max_episode_steps=3, num_envs=n, seed=cases.ORDER_SEED, device_initializer=True,
                                             samples_per_pixel=1 + n % 2, **cases.KW)
    rng = np.random.default_rng(cases.ORDER_SEED)
    want = [host.reset()[0]]
    for _ in range(cases.ORDER_STEPS):
        want.append(host.step(cases.host_actions("steps-i64", rng, n))[0])
    host.close()
    for order in ("torch-first", "library-first"):
        path = str(tmp_path / f"{order}.json")
        done = _child(["order", order, path], 300)
        assert done.returncode == 0, f"{order}: exit status {done.returncode}\n{done.stderr[-3000:]}"
        got = json.load(open(path))
        assert len(got["runtimes"]) == 1, got["runtimes"]
        assert len(got["observations"]) == len(want)
        for x, y in zip(got["observations"], want):
            assert np.array_equal(np.array(x, dtype=np.float32), y), order
