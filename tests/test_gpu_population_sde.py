"""GPU tests of the population of gSDE learners (harness.DeviceSdePopulationPolicy / DevicePopulationLearner over it,
rf_sde_noise_reset_grouped, rf_sde_forward_grouped, rf_sde_update_grouped; the grouped instantiations of the kernels of
csrc/rf_sde.h and of ppo_backward_kernel<true, .>) against the numpy twins (harness.SdePopulationPolicy /
PopulationLearner) bit for bit, and on some cases against stand-alone rf_sde_noise_reset / rf_sde_forward launches and
DeviceSdePolicy / DeviceLearner objects on the same device: every array is compared as bytes.

As tests/test_gpu_population.py: the cases need torch and the library in one process, so they run in ONE fresh child
process that imports torch first (tests/population_sde_io_cases.py), started once per session and never replaced; each
test below looks its case up.  tests/test_population_sde_logic.py holds the twins to G independent existing twins on the
CPU, on the same inputs.

Development run on an MI355X: all 59 tests pass, the child process takes 4.1 s (3.3 s on the same machine before the five
cases at B = 512 .. 1024; the twin of the two 256-256 groups takes most of the difference)."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import population_sde_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("population_sde") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.population_sde_io_cases", path], cwd=helpers.ROOT,
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


_network = pytest.mark.parametrize("index", range(len(cases.NETWORKS)),
                                   ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))


@pytest.mark.parametrize("per_group", cases.PER_GROUP)
@pytest.mark.parametrize("groups", cases.GROUPS)
@_network
def test_grouped_noise_equals_the_twin_population(index, groups, per_group, recorded):
    """rf_sde_noise_reset_grouped: every group with its own log_std, 0 draws taken before in the even groups and
    2^32 + 5 in the odd ones; theta a slice of a larger slab whose guard rows keep the sentinel.  m L from 15 (well under
    one block) to 704 (ragged over three).  Where G >= 3 one group has log_std 100 -- theta +-inf or the canonical NaN,
    exactly as the twin -- next to finite neighbours.  Then with the first, a middle and the last group deselected:
    their rows keep the sentinel bytes, the others equal the twin.  At G = 5 also G stand-alone rf_sde_noise_reset
    launches with advanced generators give the same bytes."""
    _passed(recorded, f"noise/{index}/{groups}/{per_group}")


@pytest.mark.parametrize("per_group", cases.PER_GROUP)
@pytest.mark.parametrize("groups", cases.GROUPS)
@_network
def test_grouped_forward_equals_the_twin_population(index, groups, per_group, recorded):
    """rf_sde_forward_grouped on hostile device tensors, every group with parameters and theta of its own: sampled,
    deterministic and values only, all seven outputs; final_obs with NaN rows among live ones; every output a slice of a
    larger slab whose guard rows keep their sentinel.  Every group's mean differs from what group 0's parameters give on
    its rows.  At G = 5 also G stand-alone rf_sde_forward launches give the same bytes."""
    _passed(recorded, f"forward/{index}/{groups}/{per_group}")


@pytest.mark.parametrize("batch", [shape[0] for shape in cases.UPDATE_SHAPES])
@_network
def test_grouped_update_equals_the_twin_population(index, batch, recorded):
    """rf_sde_update_grouped, three groups whose hyper-parameters and log_std all differ, over two epochs of chained
    updates with m T = 12 (B = 5, 8) or 44 (B = 13), so the last minibatch of an epoch is short; P + L = 52 and 2023 (past
    kPpoLeaves and kPpoAdamSlice): parameters, optimizer states and stats as bytes after every update, between guard
    rows.  The group with learning_rate 0 keeps its parameters byte for byte while its Adam moments move."""
    _passed(recorded, f"update/{index}/{batch}")


@pytest.mark.parametrize("index,groups,per_group", cases.WIDE)
def test_grouped_noise_and_forward_at_many_groups(index, groups, per_group, recorded):
    """The same at 64 and 65 groups of m = 8 on both networks: group indices far past 4."""
    _passed(recorded, f"noise/{index}/{groups}/{per_group}")
    _passed(recorded, f"forward/{index}/{groups}/{per_group}")


def test_grouped_update_at_64_groups_on_the_tuned_shape(recorded):
    """One rf_sde_update_grouped at G = 64, m = 8, T = 32, B = 64 (P + L = 2023) against PopulationLearner,
    hyper-parameters that differ between neighbouring groups: all 64 groups as bytes; the workspace has exactly
    rf_sde_grouped_workspace_size's bytes between guard floats."""
    _passed(recorded, "update/wide")


@pytest.mark.parametrize("index,groups,batch", cases.LARGE_CASES)
def test_grouped_update_at_large_minibatches(index, groups, batch, recorded):
    """rf_sde_update_grouped (ppo_backward_kernel<true, true>) on ppo_tuned.yml's ContinuousJumps shape, m = 8, T = 128
    (N = 1024 rows per group): B = 512, 513 (the second trip of the s_red reductions, a ragged last tile), 1000 and 1024
    (RF_PPO_MAX_BATCH) at G = 3 on the network whose vf widths are no multiple of a wave (L = 64), and B = 513 at G = 2 on
    the widest network of tests/sde_io_cases.py (256-256 both nets).  index is [G][B], every group's row its own: a
    permutation at B = N, drawn with repeats below.  Two consecutive updates against PopulationLearner, every group's
    parameters (log_std included), optimizer state and stats as bytes, between guard rows; the workspace has exactly
    rf_sde_grouped_workspace_size's bytes between guard floats.  No group is skipped, and the group with learning_rate 0
    alone keeps its parameters.  At B = 1000, G = 3 also three stand-alone rf_sde_update launches on contiguous copies of
    the groups' slices give the same bytes."""
    _passed(recorded, f"update/large/{index}/{groups}/{batch}")


def test_noise_forward_and_update_at_the_group_limit(recorded):
    """G = RF_POPULATION_MAX_GROUPS = 65535 groups of one row (m = T = B = 1) on the least network: one reset of every
    group's noise (generator g % 11 with g draws taken before), a deterministic forward, one grouped update of fresh
    optimizers.  Group g has parameter set g % 7, observation block g % 5 and hyper-parameter set g % 3; every output byte
    of every group is compared with the twin functions' result for its combination.  Then G = 65536: all five entry
    points refuse, and nothing is written."""
    _passed(recorded, "limit")


def test_a_skipped_group_leaves_the_others_alone(recorded):
    """One group's minibatch holds a NaN raw action, another's a NaN observation: exactly those carry RF_PPO_INVALID /
    RF_PPO_NONFINITE and keep parameters and optimizer state; the other two equal the twin."""
    _passed(recorded, "isolation")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """Host pointers (arrays, d_gens, d_consumed, d_select, d_hyper), G or m outside the limits, B > m T, misaligned and
    overlapping arrays, n_actions != 1: every output keeps its bytes, and the unchanged call is then taken."""
    _passed(recorded, "kernel-refusals")


def test_one_group_is_the_ungrouped_path(recorded):
    """G = 1 next to DeviceSdePolicy / DeviceLearner with the same seed: noise, act() sampled and deterministic, values(),
    three chained updates, rng_state(), parameters and optimizer state, bit for bit."""
    _passed(recorded, "one-group")


def test_collect_and_train_equal_the_twins(recorded):
    """DeviceVectorContinuousJumps at 6 envs x 16 x 16 px x 1 sample with device_initializer, episode_records and a
    learner view of 3 groups, DeviceRollout(groups=3) with discounts per group, sde_sample_freq=[-1, 1, 3] and a
    log_std_init per group: two iterations of collect + train(n_epochs=2, batch_size=4) equal VectorContinuousJumps with
    Rollout + SdePopulationPolicy + PopulationLearner: every slab, flat(), theta, stats, parameters, optimizer states,
    generator states (1, 1 + T and 1 + ceil(T / 3) resets per rollout).  Then a second policy and learner resumed from
    the state dicts repeat a train() and a masked reset_noise() bit for bit."""
    _passed(recorded, "end-to-end")


def test_the_classes_refuse_with_a_message(recorded):
    """n not divisible by the groups, too few seeds, log_std_init of the wrong length, a Discrete space, a Categorical
    spec, a sampled act() before every group has noise, a mask of the wrong length or kind, sde_sample_freq of the wrong
    length or value, a rollout whose groups differ from the policy's, train() over the other kind of rollout."""
    _passed(recorded, "surface")
