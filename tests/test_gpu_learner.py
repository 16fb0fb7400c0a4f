"""GPU tests of the PPO minibatch update (harness.DeviceLearner, rf_ppo_update, the three kernels of csrc/rf_ppo.h)
against the numpy twin (harness.Learner, learner.ppo_update_numpy) bit for bit: parameters, optimizer state and stats are
compared as bytes.

As tests/test_gpu_policy.py: the cases need torch and the library in one process, so they run in ONE fresh child process
that imports torch first (tests/learner_io_cases.py), started once per session; each test below looks its case up.
tests/test_learner_logic.py holds the twin to the host build of the kernels' own header on the CPU, on the same inputs.
The refusal of a capturing caller stream is not tested, as for the rollout.

Development run on an MI355X: all 52 tests pass, the child process takes 4.4 s (3.2 s before the cases at the batch limits:
512, 513, 1000 and 1024 rows)."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import learner_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("learner") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.learner_io_cases", path], cwd=helpers.ROOT, capture_output=True,
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


@pytest.mark.parametrize("count", cases.BATCHES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))
def test_update_equals_ppo_update_numpy(index, count, recorded):
    """rf_ppo_update over three consecutive updates of a fresh optimizer -- observations with +-0 and subnormals, logits
    that tie exactly and lie 200 apart, stored log-probabilities shifted so that ratios fall inside the clip range, past
    both bounds and at d > 0, an index with a repeat, a max_grad_norm that clips and one that does not: parameters, m, v,
    the header and the stats as bytes after each, every output between guards that keep their sentinel."""
    _passed(recorded, f"kernel/{index}/{count}")


@pytest.mark.parametrize("index,count", cases.LIMIT_CASES,
                         ids=lambda v: "-".join(str(x) for x in cases.NETWORKS[v]) if v < len(cases.NETWORKS) else str(v))
def test_update_equals_ppo_update_numpy_at_the_batch_limits(index, count, recorded):
    """The same at 512 rows (the last minibatch whose block reductions over s_red[kPpoMaxBatch] take one trip), 513 (the
    first past it: a second trip and a last tile of one row), 1000 (no power of two, no multiple of the tile) and 1024
    (RF_PPO_MAX_BATCH), on the least network and on stable-baselines3's default, and at 513 on the network with every
    limit at once.  The workspace has exactly rf_ppo_workspace_size(B) bytes between its guards."""
    _passed(recorded, f"kernel/{index}/{count}")


def test_skipped_updates_change_nothing_on_the_device(recorded):
    """An index past the end and a negative one, an action past the end and a negative one, infinite returns: parameters
    and state keep their bytes, the stats carry the flag, and the next valid update is taken."""
    _passed(recorded, "skips")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """A desc outside the limits, N = 0, B = 0 and 1025, a workspace sized for 512 rows offered for 513, every hyper-parameter negative and NaN, an infinite one, betas of
    1 and above, every pointer NULL and a host pointer, misaligned pointers, arrays, state and workspace that end past
    their allocation, outputs over inputs and over each other: parameters, state and stats keep their bytes every time,
    and the unchanged call is taken afterwards."""
    _passed(recorded, "refusals")


@pytest.mark.parametrize("kind", sorted(cases.E2E_KINDS))
def test_collect_and_train_equal_the_twins(kind, recorded):
    """Two iterations of DeviceRollout.collect(DevicePolicy) + DeviceLearner.train(2 epochs, minibatches of 16 and 12,
    given permutations) over DeviceVectorDiscreteSteps (16 x 16 px, 1 sample, 4 environments, 7 steps, device
    initializer) next to the numpy twins: parameters, optimizer state, stats and every slab of both rollouts as bytes --
    the second collect used the updated parameters; device_fault() is None."""
    _passed(recorded, f"end-to-end/{kind}")


def test_nothing_waits_for_the_host(recorded):
    """Two train() calls enqueued back to back, nothing read in between, one synchronisation at the end."""
    _passed(recorded, "no-sync")


def test_optimizer_resumes_bit_for_bit(recorded):
    _passed(recorded, "resume")


def test_surface_and_its_refusals(recorded):
    """A numpy Policy, an unfinished rollout, a ContinuousJumps rollout (the policy's message), n_epochs and batch_size
    outside their ranges and a negative learning rate are refused; update() by itself equals the twin."""
    _passed(recorded, "surface")
