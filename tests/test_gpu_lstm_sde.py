"""GPU tests of the recurrent sde policy and its update (harness.DeviceLstmSdePolicy, harness.DeviceLstmLearner over it:
rf_lstm_sde_noise_reset, rf_lstm_sde_forward, rf_lstm_sde_update; lstm_forward_kernel<true> of csrc/rf_lstm.h,
lstm_ppo_mlp_kernel<true> and lstm_ppo_gradient_kernel<true> of csrc/rf_lstm_ppo.h) against the numpy twins
(harness.LstmSdePolicy, lstm_sde.lstm_sde_numpy, lstm_learner.lstm_update_numpy) bit for bit: every array is compared as
bytes, so zero signs and NaNs count, and every output lies between guard floats that must keep their sentinel.

As tests/test_gpu_lstm_learner.py: the cases need torch and the library in one process, so they run in ONE fresh child
process that imports torch first (tests/lstm_sde_io_cases.py), started once per session and ended by its own time limit;
each test below looks its case up.  tests/test_lstm_sde_logic.py holds the twins to the host build of the kernels' own
headers and to torch's autograd on the CPU.

Development run on an MI355X: all 175 tests pass, the child process takes 13.4 s (11.3 s before the limit layouts)."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import lstm_sde_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lstm_sde") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.lstm_sde_io_cases", path], cwd=helpers.ROOT,
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


_SHAPES = [(index, n) for index in range(len(cases.NETWORKS)) for n in cases.sizes_of(index)]


@pytest.mark.parametrize("index,n", _SHAPES, ids=[f"{'-'.join(str(x) for x in cases.NETWORKS[i])}-n{n}" for i, n in _SHAPES])
def test_noise_reset_equals_the_twin(index, n, recorded):
    """rf_lstm_sde_noise_reset with the generator 0 and 2^32 + 5 draws in: theta [n, L] from this layout's log_std (rows
    of -100, 0 and +3 among them) as bytes."""
    _passed(recorded, f"noise/{index}/{n}")


@pytest.mark.parametrize("index,n", _SHAPES, ids=[f"{'-'.join(str(x) for x in cases.NETWORKS[i])}-n{n}" for i, n in _SHAPES])
def test_forward_equals_lstm_sde_numpy(index, n, recorded):
    """rf_lstm_sde_forward over a chain of 5 steps on hostile device tensors (+-0, +-inf, subnormals and NaN among the
    observations and the states, start bytes 0, 1, 2 and 255): sampled at both draw offsets and deterministic, the state
    in place and from one tensor into another; then pi only, vf only, values only and the state only.  n = 1, a tile less
    one, a tile, one past it and three tiles and five; the network with every limit at once runs at 1 and a tile and
    one."""
    _passed(recorded, f"kernel/{index}/{n}")


def test_forward_refusals_come_before_anything_is_enqueued(recorded):
    """rf_lstm_forward's and rf_sde_forward's refusals, n_actions other than 1, a missing d_theta when a pi output is
    sampled; rf_lstm_sde_noise_reset's.  Outputs and states keep their bytes, and the unchanged call is taken."""
    _passed(recorded, "forward-refusals")


_LAYOUTS = [(index, name) for index in range(len(cases.NETWORKS)) for name in cases.layouts_of(index)]


@pytest.mark.parametrize("index,name", _LAYOUTS,
                         ids=[f"{'-'.join(str(x) for x in cases.NETWORKS[i])}-{name}" for i, name in _LAYOUTS])
def test_update_equals_lstm_update_numpy(index, name, recorded):
    """rf_lstm_sde_update over three chained updates with changing hyper-parameters: parameters (log_std included),
    optimizer state, stats and the gradient read from the workspace as bytes.  The layouts of
    tests/lstm_learner_io_cases.py on T = 5, n = 3: B = 1, 2, 7, a tile, one past it and N, each with first in 0, 3, 7,
    N - 1; every row a start; one sequence of 9 rows.  The network with every limit at once runs at B = 1 and 2."""
    _passed(recorded, f"update/{index}/{name}")


_LIMIT_LAYOUTS = [(index, name) for index in range(len(cases.NETWORKS)) for name in cases.limit_layouts_of(index)]


@pytest.mark.parametrize("index,name", _LIMIT_LAYOUTS,
                         ids=[f"{'-'.join(str(x) for x in cases.NETWORKS[i])}-{name}" for i, name in _LIMIT_LAYOUTS])
def test_update_equals_lstm_update_numpy_at_the_limits(index, name, recorded):
    """The same on tests/lstm_learner_io_cases.py's LIMIT_LAYOUTS, the workspace sized for B exactly, on the H = 16
    network: tuned (T = 8, n = 8: every sequence has the 8 rows both walks prefetch; B = 8 at first 0 and 3, B = 64 = N),
    depth (T = 17, n = 4: sequences of 1, 8, 9, 16 and 17 rows; B = 65, and B = 68 = N from row 5) and untuned (T = 128,
    n = 8, B = 128: a sequence longer than 64 rows, a whole environment from its stored state, an environment boundary).
    The network with every limit at once runs one sequence of 17 rows."""
    _passed(recorded, f"update/{index}/{name}")


def test_skipped_updates_change_nothing(recorded):
    _passed(recorded, "skip")


def test_update_refusals_come_before_anything_is_enqueued(recorded):
    """rf_lstm_ppo_update's refusals with float32 actions, n_actions other than 1, and a capturing stream.  Parameters,
    state and stats keep their bytes every time, and the unchanged call is taken afterwards."""
    _passed(recorded, "update-refusals")


@pytest.mark.parametrize("n", cases.E2E_SIZES)
@pytest.mark.parametrize("kind", sorted(cases.E2E_KINDS))
def test_device_collect_and_train_equal_the_twins(kind, n, recorded):
    """DeviceRollout.collect(DeviceLstmSdePolicy, sde_sample_freq=3) then DeviceLstmLearner.train over
    DeviceVectorContinuousJumps (16 x 16 px, 1 sample, episodes of at most 5 steps) next to the numpy twins -- with
    LearnerView and episode records, and with neither (the untuned configuration's network, H = 256): two iterations of
    T = 7 steps, minibatches of 4 rows, 2 epochs from given split indices; every slab, theta, the stats, the parameters
    and the optimizer state as bytes; the generators agree; device_fault() is None."""
    _passed(recorded, f"end-to-end/{kind}/{n}")


def test_nothing_waits_for_the_host(recorded):
    """Two iterations of collect + train enqueued back to back, nothing read in between (results are cloned on torch's
    stream); one synchronisation at the end, and everything equals the twin's."""
    _passed(recorded, "no-sync")


def test_state_dict_resumes_bit_for_bit(recorded):
    _passed(recorded, "resume")


def test_surface_and_its_refusals(recorded):
    """The refusals that still stand and the new ones; reset_noise advances the generator by n * L and act() by nothing;
    act() without out=, deterministic, and from one state into another; sde_sample_freq rules."""
    _passed(recorded, "surface")
