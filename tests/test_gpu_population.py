"""GPU tests of the population (harness.DevicePopulationPolicy / DevicePopulationLearner, rf_policy_forward_grouped,
rf_ppo_update_grouped; the grouped instantiations of the kernels of csrc/rf_policy.h and csrc/rf_ppo.h) against the numpy
twins (harness.PopulationPolicy / PopulationLearner) bit for bit, and on some cases against stand-alone DevicePolicy /
DeviceLearner objects and rf_policy_forward launches on the same device: every array is compared as bytes.

As tests/test_gpu_policy.py: the cases need torch and the library in one process, so they run in ONE fresh child process
that imports torch first (tests/population_io_cases.py), started once per session; each test below looks its case up.
tests/test_population_logic.py holds the twins to G independent existing twins on the CPU, on the same inputs.

Development run on an MI355X: all 38 tests pass, the child process takes 4.4 s (4.4 s on the same machine before the five
cases at B = 512 .. 1024, whose twins take 0.1 to 0.2 s each; 2.5 s before the cases at 64, 65, 512 and 65535 groups)."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import population_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("population") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.population_io_cases", path], cwd=helpers.ROOT, capture_output=True,
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


@pytest.mark.parametrize("per_group", cases.PER_GROUP)
@pytest.mark.parametrize("groups", cases.GROUPS)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))
def test_grouped_forward_equals_the_twin_population(index, groups, per_group, recorded):
    """rf_policy_forward_grouped on hostile device tensors, every group with parameters of its own: sampled with 0 and
    2^32 + 5 draws taken before, deterministic, and values only; final_obs with NaN rows among live ones; every output a
    slice of a larger slab whose guard rows keep their sentinel.  m: group borders inside what would be one ungrouped
    tile, exactly one tile, a ragged second tile.  With G = 5 also G stand-alone rf_policy_forward launches give the same
    bytes, and every group's values differ from what group 0's parameters give on its rows."""
    _passed(recorded, f"forward/{index}/{groups}/{per_group}")


@pytest.mark.parametrize("batch", [shape[0] for shape in cases.UPDATE_SHAPES])
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))
def test_grouped_update_equals_the_twin_population(index, batch, recorded):
    """rf_ppo_update_grouped, three groups whose hyper-parameters all differ, over two epochs of chained updates with
    m T = 12 (B = 5, 8) or 44 (B = 13), so the last minibatch of an epoch is short; P = 59 and P = 1324 (past kPpoLeaves
    and kPpoAdamSlice): parameters, optimizer states and stats as bytes after every update.  The group with
    learning_rate 0 keeps its parameters byte for byte while its Adam moments move as the twin's."""
    _passed(recorded, f"update/{index}/{batch}")


@pytest.mark.parametrize("index,groups,per_group", cases.WIDE_FORWARD)
def test_grouped_forward_at_many_groups(index, groups, per_group, recorded):
    """The same at 64 and 65 groups of m = 8 (the reference's n_envs: exactly one tile per group) on both networks, and at
    512 groups of 8 and of 1: group indices far past 4, every group with parameters and a generator of its own, sampled
    at both draw counts and deterministic, every output of every group against PopulationPolicy's as bytes, the guard
    rows kept; G stand-alone launches give the same bytes."""
    _passed(recorded, f"forward/{index}/{groups}/{per_group}")


def test_grouped_update_at_64_groups_on_the_tuned_shape(recorded):
    """rf_ppo_update_grouped at G = 64 on ppo_tuned.yml's first shape (m = 8, T = 32, B = 64; P = 1324) against
    PopulationLearner over two epochs of four chained updates, hyper-parameters that differ between neighbouring groups:
    parameters, optimizer states and stats of all 64 groups as bytes after every update (groups 0, 30, 31, 32 and 63
    named first).  Group 1 has learning_rate 0.  One row of group 31 holds a NaN observation: in the one update of each
    epoch that takes it the group carries RF_PPO_NONFINITE and keeps its bytes.  Parameters and states lie between guard
    rows, the workspace of exactly rf_ppo_grouped_workspace_size's bytes between guard floats."""
    _passed(recorded, "update/wide")


@pytest.mark.parametrize("index,groups,batch", cases.LARGE_CASES)
def test_grouped_update_at_large_minibatches(index, groups, batch, recorded):
    """rf_ppo_update_grouped on ppo_tuned.yml's ContinuousJumps shape, m = 8, T = 128 (N = 1024 rows per group), at the
    sizes the ungrouped update is held to: B = 512 (the last single trip of the s_red reductions), 513 (the second trip,
    a ragged last tile), 1000 (no multiple of the tile) and 1024 (RF_PPO_MAX_BATCH) at G = 3 on the network whose widths
    are no multiple of a wave (P = 1324), and B = 513 at G = 2 on stable-baselines3's default network (P = 11918).
    index is [G][B], every group's row its own: a permutation at B = N, drawn with repeats below.  Two consecutive
    updates against PopulationLearner, every group's parameters, optimizer state and stats as bytes; parameters and
    states between guard rows, the workspace of exactly rf_ppo_grouped_workspace_size's bytes between guard floats.  No
    group is skipped and the group with learning_rate 0 alone keeps its parameters (tests/test_population_logic.py shows
    the same without a GPU).  At B = 513, G = 3 also three stand-alone rf_ppo_update launches on contiguous copies of the
    groups' slices give the same bytes."""
    _passed(recorded, f"update/large/{index}/{groups}/{batch}")


def test_forward_and_update_at_the_group_limit(recorded):
    """G = RF_POPULATION_MAX_GROUPS = 65535 groups of one row (m = T = B = 1) on the least network: a deterministic forward
    with values and final values, and one grouped update of fresh optimizers.  Group g has parameter set g % 7,
    observation block g % 5 and hyper-parameter set g % 3, so neighbours differ in all three and a wrong stride or
    offset of parameters, states, workspace, stats or rows shows at every g; every output byte of every group is compared
    with the twin functions' result for its combination (105 of them, pairwise distinct:
    tests/test_population_logic.py).  Then G = 65536: both entry points and both size functions refuse, and nothing
    is written."""
    _passed(recorded, "limit")


def test_a_skipped_group_leaves_the_others_alone(recorded):
    """One group's index reaches into the next group's rows, another's minibatch holds a NaN observation: exactly those
    carry RF_PPO_INVALID / RF_PPO_NONFINITE and keep parameters and optimizer state; the other two equal the twin."""
    _passed(recorded, "isolation")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """Host pointers (arrays, the generator table, the hyper-parameters), G or m outside the limits, B > m T, misaligned
    and overlapping arrays, a desc outside the limits: every output keeps its bytes, and the unchanged call is taken."""
    _passed(recorded, "kernel-refusals")


def test_one_group_is_the_ungrouped_path(recorded):
    """G = 1 next to DevicePolicy / DeviceLearner with the same seed: act() sampled and deterministic, values(), three
    chained updates, rng_state(), parameters and optimizer state, bit for bit."""
    _passed(recorded, "one-group")


def test_collect_and_train_equal_the_twins(recorded):
    """DeviceVectorDiscreteSteps at 6 envs x 16 x 16 px x 1 sample with device_initializer and episode_records, G = 3: two
    iterations of DeviceRollout.collect + train(n_epochs=2, batch_size=4) equal VectorDiscreteSteps with Rollout +
    PopulationPolicy + PopulationLearner: every slab, flat(), stats, parameters, optimizer states, generator states.
    Then a second learner resumed from state_dict() repeats a train() bit for bit, and a train() that draws its own
    permutations on the device flags nothing."""
    _passed(recorded, "end-to-end")


def test_the_classes_refuse_with_a_message(recorded):
    """n not divisible by the groups, too few and too many seeds, a Box action space, G m != the rows of obs, wrong dtypes
    and types, overlapping out=, a rollout that lives on the host, batch_size > m T, index of the wrong shape or dtype:
    tensors compared unchanged afterwards, no draw consumed."""
    _passed(recorded, "surface")


def test_a_sharded_environment_is_refused(recorded):
    _passed(recorded, "sharded")
