"""GPU tests of the PPO rollout buffer (harness.DeviceRollout, rf_rollout_advantages, rollout_gae_kernel of
csrc/rf_rollout.h) against the numpy twin (harness.Rollout, rollout.gae_numpy) bit for bit: float32 and float64 arrays
are compared as bytes, so zero signs and NaNs count.

As tests/test_gpu_device_io.py: the cases need torch and the library in one process, so they run in ONE fresh child
process that imports torch first (tests/rollout_io_cases.py), started once per session; each test below looks its case
up.  tests/test_rollout_logic.py holds the twin to the definition on the CPU and checks that the seeds used here end
environments inside a rollout and on its last step.

Development run on an MI355X: all 21 tests pass, the child process takes 4 s."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import rollout_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("rollout") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.rollout_io_cases", path], cwd=helpers.ROOT, capture_output=True,
                          text=True, timeout=600)
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


def test_child_ran_every_case(recorded):
    _passed(recorded, "finished")


@pytest.mark.parametrize("form", ["bootstrap", "plain"])
@pytest.mark.parametrize("steps,n", cases.KERNEL_SHAPES, ids=lambda v: str(v))
def test_kernel_equals_gae_numpy(steps, n, form, recorded):
    """rf_rollout_advantages on synthetic device tensors -- +-0, +-inf and subnormals among the values, rewards float32
    cannot hold, final_values NaN wherever truncated is 0; truncated all 0, all 1 and random -- with (bootstrap) and
    without (plain) final_values: advantages and returns as bytes.  (1, 1): only the last_values path; (5, 64) and
    (33, 65): a full tile and one environment past it, and one step past a chunk; (128, 8): the reference's shape, four
    chunks; (chunk + 1, 1100): a chunk boundary and 18 tiles, the last one ragged.  The output slabs lie between two
    guard rows that must keep their sentinel."""
    _passed(recorded, f"kernel/{steps}x{n}/{form}")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """A host pointer (input and output), T = 0, n = 0, an output over values (whole and in part) and over the other
    output, a misaligned pointer, an array that ends past its allocation, and through DeviceRollout.finish last_values
    of another shape (too short, two columns, on the host): the outputs keep their sentinel every time, and the
    unchanged call is taken afterwards."""
    _passed(recorded, "refusals")


@pytest.mark.parametrize("n", cases.E2E_SIZES)
def test_device_rollouts_equal_the_twins(n, recorded):
    """DeviceVectorDiscreteSteps (16 x 16 px, 1 sample, device initializer, episode records, LearnerView(frame_stack=5))
    next to VectorDiscreteSteps: two consecutive rollouts of 7 steps by a fixed action schedule and a "policy" that is
    exact in float32 (values = obs[:, 0] * 0.5, log_probs = -values, V(final) alike); every slab, advantages, returns
    and flat() as bytes after each; device_fault() is None."""
    _passed(recorded, f"end-to-end/steps/{n}")


def test_device_rollouts_of_continuous_jumps_without_a_view(recorded):
    _passed(recorded, "end-to-end/jumps/65")


def test_device_rollouts_without_records_and_bootstrap(recorded):
    _passed(recorded, "end-to-end/no-records/65")


def test_nothing_waits_for_the_host(recorded):
    """A rollout, finish(), start() and the first step of the next rollout enqueued back to back, nothing read in
    between (results are cloned on torch's stream); one synchronisation at the end, and everything equals the twin's."""
    _passed(recorded, "no-sync")


def test_minibatches_and_the_refusals_of_the_class(recorded):
    """minibatches(4) of 21 rows: six batches from one torch.randperm, every index once; bootstrap without records, an
    eighth step; a host initializer, a render_mode and a sharded environment are refused as step_tensors refuses them."""
    _passed(recorded, "surface")
