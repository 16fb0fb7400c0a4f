"""GPU tests of the PPO actor-critic (harness.DevicePolicy, rf_policy_forward, policy_forward_kernel of
csrc/rf_policy.h) against the numpy twin (harness.Policy, policy.policy_numpy) bit for bit: every float32 array is
compared as bytes, so zero signs and NaNs count.

As tests/test_gpu_rollout.py: the cases need torch and the library in one process, so they run in ONE fresh child process
that imports torch first (tests/policy_io_cases.py), started once per session; each test below looks its case up.
tests/test_policy_logic.py holds the twin to the host build of the kernel's own header on the CPU, on the same inputs.

Development run on an MI355X: all 30 tests pass, the child process takes 3.5 s."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import policy_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("policy") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.policy_io_cases", path], cwd=helpers.ROOT, capture_output=True,
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
def test_kernel_equals_policy_numpy(index, n, recorded):
    """rf_policy_forward on hostile device tensors -- +-0, +-inf, subnormals and NaN among the observations, NaN-led
    final_obs rows among live ones, parameters whose logits tie exactly and lie 200 apart -- sampled at draw offsets 0
    and 2^32 + 5 and deterministic: actions, log_probs, values, final_values and logits as bytes, each output between two
    guard rows that must keep their sentinel; then a values-only call.  n: one environment, a full tile, one past it,
    three tiles and a ragged fourth."""
    _passed(recorded, f"kernel/{index}/{n}")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """A host pointer (input, output, parameters), n = 0, misaligned pointers, an output over an input, over another
    output and over the parameters, an array and parameters that end past their allocation, every field of the desc
    outside its limits, unknown flags, a sampled call without gen, final_values without final_obs, log_probs without
    actions: the outputs keep their sentinel every time, and the unchanged call is taken afterwards."""
    _passed(recorded, "refusals")


@pytest.mark.parametrize("n", cases.E2E_SIZES)
@pytest.mark.parametrize("kind", sorted(cases.E2E_KINDS))
def test_device_collect_equals_the_twins(kind, n, recorded):
    """DeviceRollout.collect(DevicePolicy) over DeviceVectorDiscreteSteps (16 x 16 px, 1 sample, device initializer) next
    to Rollout.collect(Policy) over VectorDiscreteSteps -- with episode records and LearnerView(frame_stack=5) ([64, 64]
    tanh), and with neither ([256, 256] ReLU): two consecutive rollouts of 7 steps; every slab, advantages, returns and
    flat() as bytes after each; the generators end in the same state; device_fault() is None."""
    _passed(recorded, f"end-to-end/{kind}/{n}")


def test_collect_equals_the_explicit_loop_on_the_device(recorded):
    _passed(recorded, "explicit")


def test_nothing_waits_for_the_host(recorded):
    """Two collects enqueued back to back, nothing read in between (the first one's results are cloned on torch's
    stream); one synchronisation at the end, and everything equals the twin's."""
    _passed(recorded, "no-sync")


def test_load_state_dict_between_two_collects(recorded):
    """New parameters (device tensors: transposes and copies on the stream) change the second rollout exactly as the
    twin's load_state_dict does; state_dict() gives them back."""
    _passed(recorded, "reload")


def test_box_action_space_is_refused_and_the_surface(recorded):
    """DeviceVectorContinuousJumps is refused with a message that says continuous action spaces are out of scope;
    act() without out=, deterministic and sampled, values(); rows of another width, dtype or device are refused and
    consume no draw."""
    _passed(recorded, "surface")
