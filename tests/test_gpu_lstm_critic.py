"""GPU tests of the recurrent policies with a feed-forward critic (enable_critic_lstm=False; include/reinfocus_hip.h, "lstm
critic": lstm_forward_kernel<., true> of csrc/rf_lstm.h, lstm_ppo_forward_kernel<true> and lstm_ppo_gradient_kernel<., true>
of csrc/rf_lstm_ppo.h, the rf_lstm_critic_* entry points, and DeviceLstmPolicy / DeviceLstmSdePolicy / DeviceLstmLearner over
a spec of this mode) against the numpy twins bit for bit: every array is compared as bytes, between guard floats, so zero
signs and NaNs count.

As the siblings: the cases need torch and the library in one process, so they run in ONE fresh child process that imports
torch first (tests/lstm_critic_io_cases.py), started once per module; each test below looks its case up.  That process runs
the siblings' own device cases in this mode (their specs built with enable_critic_lstm=False, the vf half of every stored
state NaN, every rf_lstm_* call routed to its rf_lstm_critic_* sibling), and three cases of its own.
tests/test_lstm_critic_logic.py holds the twins to the host build of the kernels' own headers on the CPU.

Development run on an MI355X: all 185 tests pass, the child process takes 14.4 s (7.9 s before the limit layouts)."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import lstm_critic_io_cases as cases

pytestmark = pytest.mark.gpu
NETWORK_IDS = ["-".join(str(v) for v in cases.NETWORKS[i]) for i in cases.GPU_NETWORKS]
UPDATE_CASES = [(index, name) for index in cases.GPU_NETWORKS for name in cases.layouts_of(index)]


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lstm_critic") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.lstm_critic_io_cases", path], cwd=helpers.ROOT, capture_output=True,
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


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("index", cases.GPU_NETWORKS, ids=NETWORK_IDS)
@pytest.mark.parametrize("head", cases.HEADS)
def test_forward_equals_the_twin(head, index, n, recorded):
    """rf_lstm_critic_forward / rf_lstm_critic_sde_forward (and rf_lstm_critic_sde_noise_reset) over a chain of 5 steps on
    hostile device tensors -- +-0, +-inf, subnormals and NaN among the observations and the pi state, start bytes 0, 1, 2
    and 255 mixed, NaN-led final_obs rows among live ones, the vf half of the initial state NaN throughout -- sampled and
    deterministic, each with the state in place and from one buffer into another: every output and the state of every step
    as bytes, each between guards that must keep their sentinel; then the calls that change which blocks run: values only
    (with and without final_obs; the state bytes stay), the pi outputs only, the state only.  Networks: ppo_lstm_tuned.yml's
    (D = 4, H = 16), an odd one (D = 7, H = 65, pi (65,), vf (3, 200), 64 actions or one) and every limit at once
    (D = H = 256).  n: one environment, a full tile, one past it, three tiles and a ragged fourth."""
    _passed(recorded, f"forward/{head}/{index}/{n}")


def test_value_path_ignores_state_and_starts_on_the_device(recorded):
    """Both heads, the three networks: a state that is NaN throughout with every start byte 0 gives the finite values and
    final_values of a zero state with every start byte 1, byte for byte, and the twin's."""
    _passed(recorded, "value-path")


@pytest.mark.parametrize("index,name", UPDATE_CASES, ids=[f"{cases.NETWORKS[i][1]}-{name}" for i, name in UPDATE_CASES])
@pytest.mark.parametrize("head", cases.HEADS)
def test_update_equals_the_twin(head, index, name, recorded):
    """rf_lstm_critic_ppo_update / rf_lstm_critic_sde_update: three chained updates with changing hyper-parameters on every
    layout of lstm_learner_io_cases.LAYOUTS (T = 5, n = 3; B = 1, 2, 7, 8, 9, 15; first = 0, 3, 7, 14; every row a start; one
    9-row sequence; the network with every limit at B <= 2), the vf half of lstm_states NaN throughout: parameters,
    optimizer state, stats and the gradient left in the workspace as bytes; the guards around every output keep their
    sentinel."""
    _passed(recorded, f"update/{head}/{index}/{name}")


LIMIT_CASES = [(index, name) for index in cases.GPU_NETWORKS for name in cases.limit_layouts_of(index)]


@pytest.mark.parametrize("index,name", LIMIT_CASES, ids=[f"{cases.NETWORKS[i][1]}-{name}" for i, name in LIMIT_CASES])
@pytest.mark.parametrize("head", cases.HEADS)
def test_update_equals_the_twin_at_the_limits(head, index, name, recorded):
    """The same on lstm_learner_io_cases.LIMIT_LAYOUTS, the workspace sized for B exactly: tuned (8-row sequences; B = 8 and
    64) and depth (sequences of 1, 8, 9, 16 and 17 rows; B = 65 and 68, so the critic's forward grid of B + ceil(B / 8)
    blocks has 9 tiles) on both networks below the limits; wave (T = 16, n = 64: B = 1024 of one-row sequences, 128 tiles
    and the second trip of the loss reductions, and B = 513 in 33 sequences) on ppo_lstm_tuned.yml's; one 17-row sequence
    on the network with every limit."""
    _passed(recorded, f"update/{head}/{index}/{name}")


@pytest.mark.parametrize("what", ["categorical/forward", "categorical/update", "sde/forward", "sde/update", "critic"])
def test_refusals_come_before_anything_is_enqueued(what, recorded):
    """Everything the rf_lstm_ siblings refuse (host pointers, sizes, misaligned pointers, overlaps, arrays that end past
    their allocation, every field of the desc outside its limits, flags, hyper-parameters, NULL arguments, a capturing
    stream) through the rf_lstm_critic_ entry points, and (critic) a critic value of 2 or -1 at every entry point -- sizes
    are then 0 --: all bytes stay unchanged every time, and the unchanged call is taken afterwards.  With
    RF_LSTM_CRITIC_LSTM a sibling gives the bytes of the rf_lstm_ entry point itself."""
    _passed(recorded, f"refusals/{what}")


@pytest.mark.parametrize("n", cases.lstm_learner_cases.E2E_SIZES)
@pytest.mark.parametrize("head", cases.HEADS)
def test_collect_and_train_equal_the_twins(head, n, recorded):
    """DeviceVectorDiscreteSteps with DeviceLstmPolicy, DeviceVectorContinuousJumps with DeviceLstmSdePolicy (16 x 16 px, 1
    sample, episodes of at most 5 steps, episode records and LearnerView), specs with enable_critic_lstm=False: two
    iterations of collect() (T = 7) + train() (minibatches of 4 rows, 2 epochs from given splits) next to the numpy twins:
    stats, parameters, optimizer state and every rollout slab (episode_starts and lstm_states included) as bytes;
    device_fault() is None."""
    _passed(recorded, f"end-to-end/{head}/{n}")


@pytest.mark.parametrize("head", cases.HEADS)
def test_nothing_waits_for_the_host(head, recorded):
    """The same work enqueued back to back, nothing read in between; one synchronisation at the end."""
    _passed(recorded, f"no-sync/{head}")


@pytest.mark.parametrize("head", cases.HEADS)
def test_state_dicts_resume_bit_for_bit(head, recorded):
    """state_dict() / load_state_dict() of the policy (under critic.weight / critic.bias) and of the learner's optimizer
    resume in a fresh learner bit for bit."""
    _passed(recorded, f"resume/{head}")
