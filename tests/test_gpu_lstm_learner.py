"""GPU tests of the recurrent PPO minibatch update (harness.DeviceLstmLearner, rf_lstm_ppo_update, the kernels of
csrc/rf_lstm_ppo.h) against the numpy twin (harness.LstmLearner, lstm_learner.lstm_update_numpy) bit for bit: every array is
compared as bytes, so zero signs and NaNs count.

As tests/test_gpu_lstm.py: the cases need torch and the library in one process, so they run in ONE fresh child process
that imports torch first (tests/lstm_learner_io_cases.py), started once per session and ended by its own time limit; each
test below looks its case up.  tests/test_lstm_learner_logic.py holds the twin to the host build of the kernels' own
header and to torch's autograd on the CPU, on the same inputs.

Development run on an MI355X: all 133 tests pass, the child process takes 20 s (9.6 s before the limit layouts; of the 10 s
they add, 8 are the numpy twin's on the two T = 128, H = 256 cases, which the child computes on the CPU)."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import lstm_learner_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lstm_learner") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.lstm_learner_io_cases", path], cwd=helpers.ROOT,
                          capture_output=True, text=True, timeout=600)
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


@pytest.mark.parametrize("index,name", [(index, name) for index in range(len(cases.NETWORKS))
                                        for name in cases.layouts_of(index)],
                         ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in cases.NETWORKS[v]))
def test_kernels_equal_lstm_update_numpy(index, name, recorded):
    """rf_lstm_ppo_update over three chained updates with changing hyper-parameters: parameters, optimizer state, stats
    and the gradient read from the workspace as bytes, every output between guard floats that must keep their sentinel.
    Layouts on T = 5, n = 3: B = 1, 2, 7, a tile, one past it and N, each with first in 0, 3, 7, N - 1 (ragged tiles, the
    wrap, environment boundaries, start bytes 1, 2 and 255, sequences of one row and of four rows from a stored
    state); every row a start; one sequence of 9 rows (longer than a tile) that spans the minibatch.  The network with
    every limit at once runs at B = 1 and 2."""
    _passed(recorded, f"kernel/{index}/{name}")


@pytest.mark.parametrize("index,name", [(index, name) for index in range(len(cases.NETWORKS))
                                        for name in cases.limit_layouts_of(index)],
                         ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in cases.NETWORKS[v]))
def test_kernels_equal_lstm_update_numpy_at_the_limits(index, name, recorded):
    """The same on tests/lstm_learner_io_cases.py's LIMIT_LAYOUTS, the workspace sized for B exactly.
    tuned (T = 8, n = 8, ppo_lstm_tuned.yml's): every sequence has the 8 rows both walks prefetch, at B = 8 (first 0, and
    first 3: a 5-row tail and a 3-row head) and B = 64 = N (8 tiles, 8 sequences).  depth (T = 17, n = 4): sequences of 1,
    8, 9, 16 and 17 rows at B = 65 and at B = 68 = N from row 5, which wraps.  untuned (T = 128, n = 8, B = 128,
    ppo_lstm_untuned.yml's): drawn starts, a sequence longer than 64 rows and one of one row, a whole environment from
    its stored state and rows 100 .. 227 across an environment boundary -- on ppo_lstm_tuned.yml's network and on
    sb3-contrib's default (H = 256).  wave (T = 16, n = 64): 1024 one-row sequences at B = 1024 = RF_PPO_MAX_BATCH (the
    widest forward and BPTT grids, 128 MLP tiles, the second trip of the loss reductions) and 33 sequences at B = 513.
    The network with every limit at once runs one sequence of 17 rows."""
    _passed(recorded, f"kernel/{index}/{name}")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """Every refusal of rf_ppo_update's test (every field of the desc outside its limits, hyper-parameters, NULL, host
    and misaligned pointers, arrays that end past their allocation, overlaps), and: lstm_hidden outside its limits,
    n_steps or num_envs of 0, first and B outside their limits (B > N too), host pointers for the two slabs, slabs that
    end past their allocation (one with T rows in place of T + 1), a capturing stream.  Parameters, state and stats keep
    their bytes every time, and the unchanged call is taken afterwards."""
    _passed(recorded, "refusals")


@pytest.mark.parametrize("n", cases.E2E_SIZES)
@pytest.mark.parametrize("kind", sorted(cases.E2E_KINDS))
def test_device_collect_and_train_equal_the_twins(kind, n, recorded):
    """DeviceRollout.collect(DeviceLstmPolicy) then DeviceLstmLearner.train over DeviceVectorDiscreteSteps (16 x 16 px, 1
    sample, episodes of at most 5 steps, so episode starts fall inside minibatches) next to the numpy twins -- with
    episode records and LearnerView(frame_stack=1) (ppo_lstm_tuned.yml's network) and with neither (the default network,
    H = 256): two iterations of T = 7 steps, minibatches of 4 rows, 2 epochs from given split indices; the stats, the
    parameters, the optimizer state and every slab of both rollouts as bytes; device_fault() is None."""
    _passed(recorded, f"end-to-end/{kind}/{n}")


def test_nothing_waits_for_the_host(recorded):
    """Two iterations of collect + train enqueued back to back, nothing read in between (results are cloned on torch's
    stream); one synchronisation at the end, and everything equals the twin's."""
    _passed(recorded, "no-sync")


def test_state_dict_resumes_bit_for_bit(recorded):
    _passed(recorded, "resume")


def test_surface_and_its_refusals(recorded):
    """A rollout collected without a recurrent policy, a Box action space, a slab on the host, first / count / splits
    outside their limits are refused with a message; update() by itself equals the twin; train() without splits draws
    them on the host."""
    _passed(recorded, "surface")
