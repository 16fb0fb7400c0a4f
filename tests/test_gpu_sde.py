"""GPU tests of the sde policy (harness.DeviceSdePolicy, rf_sde_noise_reset, rf_sde_forward, rf_sde_update: the kernels of
csrc/rf_sde.h and the Gaussian head of csrc/rf_ppo.h) against the numpy twin (harness.SdePolicy, sde.sde_numpy,
learner.sde_gradient_numpy) bit for bit: theta, every forward output, parameters, optimizer state, stats and every slab
of the rollouts are compared as bytes.

As tests/test_gpu_learner.py: the cases need torch and the library in one process, so they run in ONE fresh child process
that imports torch first (tests/sde_io_cases.py), started once per session; each test below looks its case up.
tests/test_sde_logic.py holds the twin to the host build of the kernels' own headers on the CPU, on the same inputs.
The refusal of a capturing caller stream is not tested, as for the learner.

Development run on an MI355X: all 52 tests pass, the child process takes 4.4 s (3.3 s before the updates of 513, 1000 and
1024 rows)."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import sde_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("sde") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.sde_io_cases", path], cwd=helpers.ROOT, capture_output=True,
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
def test_reset_and_forward_equal_the_twin(index, n, recorded):
    """rf_sde_noise_reset with the generator 0 and 2^32 + 5 draws in, then rf_sde_forward sampled, deterministic (no
    theta, no draw) and values-only -- log_std rows at -100, 0 and +3, observations with +-0, subnormals, infinities and a
    row that is NaN throughout, a theta that pushes raw actions far past +-1 (raw against clamped), final observations
    with NaN-led rows: theta, actions, env_actions, log_probs, values, final_values, mean and sigma as bytes, every output
    between guards that keep their sentinel."""
    _passed(recorded, f"forward/{index}/{n}")


@pytest.mark.parametrize("count", cases.BATCHES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))
def test_update_equals_the_twin(index, count, recorded):
    """rf_sde_update over three consecutive updates of a fresh optimizer -- stored log-probabilities shifted so that
    ratios fall inside the clip range and past both bounds, an index with a repeat, a max_grad_norm that clips and one
    that does not, a log_std row at -100: parameters (log_std included), m, v, the header and the stats as bytes after
    each, every output between guards."""
    _passed(recorded, f"update/{index}/{count}")


@pytest.mark.parametrize("index,count", cases.LIMIT_CASES,
                         ids=lambda v: "-".join(str(x) for x in cases.NETWORKS[v]) if v < len(cases.NETWORKS) else str(v))
def test_update_equals_the_twin_at_the_batch_limits(index, count, recorded):
    """The same at 513 rows (the first size at which the block reductions over s_red[kPpoMaxBatch] take a second trip,
    with a last tile of one row), 1000 (no multiple of the tile) and 1024 (RF_PPO_MAX_BATCH), on the single-unit latent
    and on SB3's default in both activations, and at 513 on the widest network.  The workspace has exactly
    rf_sde_workspace_size(B) bytes between its guards."""
    _passed(recorded, f"update/{index}/{count}")


def test_skipped_updates_change_nothing_on_the_device(recorded):
    """An index past the end and a negative one, a NaN action, infinite returns, a sigma made infinite by log_std = 90:
    parameters and state keep their bytes, the stats carry the flag, and the next valid update is taken."""
    _passed(recorded, "skips")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """The three new entry points: a desc outside the limits (n_actions other than 1 among them), n, N and B outside their
    ranges, a workspace sized for 512 rows offered for 513, bad hyper-parameters, unknown flags, a sampled call without theta, every pointer NULL and a host pointer,
    misaligned pointers, arrays that end past their allocation, outputs over inputs and over each other: every output
    keeps its bytes, and the unchanged update is taken afterwards."""
    _passed(recorded, "refusals")


@pytest.mark.parametrize("kind", sorted(cases.E2E_KINDS))
def test_collect_and_train_equal_the_twins(kind, recorded):
    """Two iterations of DeviceRollout.collect(DeviceSdePolicy, sde_sample_freq=3) + DeviceLearner.train(2 epochs,
    minibatches of 16 and 12, given permutations) over DeviceVectorContinuousJumps (16 x 16 px, 1 sample, 4 environments,
    7 steps, device initializer), with and without learner_view / episode_records, next to the numpy twins: every slab
    (the raw actions among them, some past +-1), theta, the parameters, the optimizer state and the stats as bytes; the
    generator moved by n * L per reset; device_fault() is None."""
    _passed(recorded, f"end-to-end/{kind}/{cases.E2E_FREQ}")


def test_collect_and_train_with_one_noise_per_rollout(recorded):
    """The same with sde_sample_freq=-1: one reset per collect()."""
    _passed(recorded, "end-to-end/records/-1")


def test_nothing_waits_for_the_host(recorded):
    """collect() + train() + collect() enqueued back to back, nothing read in between, one synchronisation at the end."""
    _passed(recorded, "no-sync")


def test_training_resumes_bit_for_bit(recorded):
    """state_dict + rng_state + noise() + the optimizer's state_dict into a fresh policy and learner: the next iteration
    equals the uninterrupted one."""
    _passed(recorded, "resume")


def test_surface_and_its_refusals(recorded):
    """An sde policy on a Discrete environment, a Categorical one on the Box environment (its old message), a numpy
    twin, another spec, a sampled act() before reset_noise(), an sde learner given an int64 action slab or a Discrete
    rollout are refused; act() without out= equals the twin and a deterministic call consumes no draw."""
    _passed(recorded, "surface")
