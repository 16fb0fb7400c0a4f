"""GPU tests of the recurrent PPO actor-critic (harness.DeviceLstmPolicy, rf_lstm_forward, lstm_forward_kernel of
csrc/rf_lstm.h) against the numpy twin (harness.LstmPolicy, lstm.lstm_numpy) bit for bit: every array is compared as
bytes, so zero signs and NaNs count.

As tests/test_gpu_policy.py: the cases need torch and the library in one process, so they run in ONE fresh child process
that imports torch first (tests/lstm_io_cases.py), started once per session; each test below looks its case up.
tests/test_lstm_logic.py holds the twin to the host build of the kernel's own header on the CPU, on the same inputs.

Development run on an MI355X: all 31 tests pass, the child process takes 4.8 s."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import lstm_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lstm") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.lstm_io_cases", path], cwd=helpers.ROOT, capture_output=True,
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
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))
def test_kernel_equals_lstm_numpy(index, n, recorded):
    """rf_lstm_forward over a chain of 5 steps on hostile device tensors -- +-0, +-inf, subnormals and NaN among the
    observations and the initial state, start bytes 0, 1, 2 and 255 mixed, an environment whose state is NaN and whose
    start byte is set, NaN-led final_obs rows among live ones -- sampled at draw offsets 0 and 2^32 + 5 and
    deterministic, each with the state in place and from one buffer into another: actions, log_probs, values,
    final_values, logits and the state of every step as bytes, each between guard rows that must keep their sentinel;
    then a values-only call, which must leave the state bytes untouched, and a call that advances the state only.
    n: one environment, a full tile, one past it, three tiles and a ragged fourth."""
    _passed(recorded, f"kernel/{index}/{n}")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """Every refusal of rf_policy_forward's test (host pointers, n = 0, misaligned pointers, overlaps, arrays that end
    past their allocation, every field of the desc outside its limits, flags, gen, final_obs, log_probs without actions),
    and: lstm_hidden outside its limits, a state_out that partly overlaps state_in, states that end past their
    allocation, episode_starts and state_in as host pointers, a call that asks for nothing.  The outputs and both states
    keep their bytes every time, and the unchanged call is taken afterwards."""
    _passed(recorded, "refusals")


@pytest.mark.parametrize("n", cases.E2E_SIZES)
@pytest.mark.parametrize("kind", sorted(cases.E2E_KINDS))
def test_device_collect_equals_the_twins(kind, n, recorded):
    """DeviceRollout.collect(DeviceLstmPolicy) over DeviceVectorDiscreteSteps (16 x 16 px, 1 sample, device initializer,
    episodes of at most 5 steps) next to Rollout.collect(LstmPolicy) over VectorDiscreteSteps -- with episode records
    and LearnerView(frame_stack=1) (ppo_lstm_tuned.yml's network), and with neither (the default network): two
    consecutive rollouts of 7 steps; every slab, episode_starts and lstm_states included, advantages, returns, flat() and
    the policy's state as bytes after each; the generators end in the same state; device_fault() is None."""
    _passed(recorded, f"end-to-end/{kind}/{n}")


def test_collect_equals_the_explicit_loop_on_the_device(recorded):
    _passed(recorded, "explicit")


def test_nothing_waits_for_the_host(recorded):
    """Two collects enqueued back to back, nothing read in between (the first one's results are cloned on torch's
    stream); one synchronisation at the end, and everything equals the twin's."""
    _passed(recorded, "no-sync")


def test_load_state_dict_between_two_collects(recorded):
    """New parameters (device tensors under sb3-contrib's names: transposes and copies on the stream) change the second
    rollout exactly as the twin's load_state_dict does; state_dict() gives them back."""
    _passed(recorded, "reload")


def test_feedforward_rollout_never_allocates_the_recurrent_slabs(recorded):
    """A DeviceRollout that collects with DevicePolicy in the same process equals its twin as before and has neither
    episode_starts nor lstm_states."""
    _passed(recorded, "feedforward")


def test_box_action_space_is_refused_and_the_surface(recorded):
    """DeviceVectorContinuousJumps is refused with a message that names the scope; act() without out=, deterministic and
    sampled; values() never advances the state; states=(in, out) leaves the own state alone; lstm_state / set_lstm_state
    / reset_state; inputs of another width, dtype, device or row count are refused and consume no draw."""
    _passed(recorded, "surface")
