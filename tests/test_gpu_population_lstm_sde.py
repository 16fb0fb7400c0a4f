"""GPU tests of the population of recurrent gSDE learners (harness.DevicePopulationLstmSdePolicy / DevicePopulationLearner
over it, rf_lstm_sde_noise_reset_grouped, rf_lstm_sde_forward_grouped, rf_lstm_sde_update_grouped; the grouped
instantiations of the kernels of csrc/rf_lstm.h and csrc/rf_lstm_ppo.h with the Gaussian head) against the numpy twins
(harness.LstmSdePopulationPolicy / PopulationLearner) bit for bit, and against stand-alone rf_lstm_critic_sde_noise_reset /
rf_lstm_critic_sde_forward / rf_lstm_critic_sde_update launches and DeviceLstmSdePolicy / DeviceLstmLearner objects on the
same device: every array is compared as bytes, every output is sentinel-filled between guard floats first.

As tests/test_gpu_population_lstm.py: the cases need torch and the library in one process, so they run in ONE fresh child
process that imports torch first (tests/population_lstm_sde_io_cases.py), started once per session and never replaced; each
test below looks its case up.  tests/test_population_lstm_sde_logic.py holds the twins to G independent existing twins on
the CPU, on the same inputs."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import lstm_sde_io_cases as lsde_cases
from tests import population_lstm_sde_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("population_lstm_sde") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.population_lstm_sde_io_cases", path], cwd=helpers.ROOT,
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


_network = pytest.mark.parametrize("index", cases.NETS, ids=lambda i: "-".join(str(v) for v in lsde_cases.NETWORKS[i]))
_critic = pytest.mark.parametrize("critic", [cases.critic_name(c) for c in cases.CRITICS])


@_network
@_critic
def test_grouped_noise_reset_equals_the_twin_population(critic, index, recorded):
    """rf_lstm_sde_noise_reset_grouped at G = 3, m = 3 with generators that had given (0, 2^32 + 5, 7) draws and every group
    its own log_std, for the masks None, (1, 0, 1) and (0, 0, 0): the selected groups' rows of theta are the twin's, the
    unselected rows keep their sentinel bytes, the guard floats stay; G stand-alone rf_lstm_critic_sde_noise_reset launches
    from generators advanced on the host give the same rows."""
    _passed(recorded, f"noise/{critic}/{index}")


@pytest.mark.parametrize("per_group", cases.PER_GROUP)
@pytest.mark.parametrize("groups", cases.GROUPS)
@_network
@_critic
def test_grouped_forward_equals_the_twin_population(critic, index, groups, per_group, recorded):
    """rf_lstm_sde_forward_grouped on hostile device tensors, every group with parameters, log_std and theta of its own and
    a state around its own non-zero level, mixed start bytes: sampled and deterministic (theta NULL), the state in place and
    from `in` to `out`; all seven outputs and the whole output state as bytes; then each pi output asked for by itself and
    the two values by themselves (nothing else is written, the state stays); every output between guard floats.  m = 3 puts
    a group border inside what would be one ungrouped tile, m = 8 is exactly one tile, m = 11 a ragged second one.  Then G
    stand-alone rf_lstm_critic_sde_forward launches on contiguous copies give the same bytes."""
    _passed(recorded, f"forward/{critic}/{index}/{groups}/{per_group}")


@_network
@_critic
def test_the_state_keeps_its_plane_stride(critic, index, recorded):
    """G = 3, m = 3, a distinct non-zero state per group: the grouped launch equals the twin, and the twin over the same bytes
    read as [G][2][2][m][H] gives another next state (and, past the least network, another mean) -- a kernel that added g
    times a size to the state pointer could not pass."""
    _passed(recorded, f"stride/{critic}/{index}")


@pytest.mark.parametrize("batch", cases.UPDATE["batches"])
@_network
@_critic
def test_grouped_update_equals_the_twin_population(critic, index, batch, recorded):
    """rf_lstm_sde_update_grouped, three groups of (T, m) = (4, 3) whose hyper-parameters, parameters, log_std and sequence
    structures all differ, firsts (0, 7, 11), B = 5 and 12 = N, two consecutive updates over float32 raw actions:
    parameters, optimizer states and stats [G][8] as bytes between guard floats, the workspace of exactly
    rf_lstm_sde_grouped_workspace_size's bytes between guards.  Then G stand-alone rf_lstm_critic_sde_update launches on
    contiguous slice copies give the same bytes."""
    _passed(recorded, f"update/{critic}/{index}/{batch}")


@_critic
def test_a_skipped_group_leaves_the_others_alone(critic, recorded):
    """A NaN raw action in group 1's minibatch: group 1 carries RF_PPO_INVALID in its stats[7] and keeps parameters and
    optimizer state byte for byte, groups 0 and 2 equal the undisturbed run.  The same with firsts[1] = N."""
    _passed(recorded, f"isolation/{critic}")


@_critic
def test_grouped_update_on_long_sequences(critic, recorded):
    """T = 17, m = 4, G = 3 at B = 65 on the H = 16 network: sequences of 1, 8, 9, 16 and 17 rows, the groups' columns
    rolled and their first rows (0, 5, 30), so they wrap at different rows; against the twin group by group."""
    _passed(recorded, f"depth/{critic}")


def test_update_at_the_widest_cell(recorded):
    """H = 256 (ppo_lstm_untuned.yml's network), G = 2, m = 2, T = 3, B = 6 = m T, both critic kinds: every thread of a
    block owns a unit."""
    _passed(recorded, "limit")


def test_grouped_update_at_64_groups(recorded):
    """One rf_lstm_sde_update_grouped at G = 64, m = 8, T = 8, B = 8, H = 16, every group its own first row and
    hyper-parameters that differ between neighbours, against PopulationLearner: all 64 groups as bytes."""
    _passed(recorded, "update/wide")


@_critic
def test_noise_forward_and_update_at_the_group_limit(critic, recorded):
    """G = RF_POPULATION_MAX_GROUPS = 65535 groups of one environment on the least network, m = T = B = 1: a masked noise
    reset (generator g % 11 after (0, 2^32 + 5, 7)[g % 3] draws, the groups with g % 5 = 2 left out), the forward sampled
    and deterministic with the state in place, one update of fresh optimizers.  Group g has parameter set g % 7 with its own
    log_std, input block g % 5 and hyper-parameter set and theta level g % 3; every output byte of every group is compared
    with the twin functions' result for its combination.  Where g % 11 = 5, firsts[g] = 1 = N: those 5958 groups carry
    RF_PPO_INVALID and keep parameters and optimizer state."""
    _passed(recorded, f"group-limit/{critic}")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """Host and NULL pointers, G, m or T outside the limits, B > m T, a critic kind that does not exist, misaligned and
    overlapping arrays, a sampled call without d_theta, a state_out that overlaps state_in without being it, a capturing
    caller stream: every sentinel-filled output keeps its bytes, the unchanged call is then taken, and the size functions
    return 0 where the Categorical population's do."""
    _passed(recorded, "kernel-refusals")


@_critic
def test_one_group_is_the_ungrouped_path(critic, recorded):
    """G = 1 next to DeviceLstmSdePolicy / DeviceLstmLearner with the same seed: reset_noise(), act() sampled and
    deterministic, the state, values(), three chained updates, rng_state(), parameters and optimizer state, bit for bit."""
    _passed(recorded, f"one-group/{critic}")


@_critic
def test_collect_and_train_equal_the_twins(critic, recorded):
    """DeviceVectorContinuousJumps at 9 envs x 16 x 16 px x 1 sample with device_initializer and episode_records, G = 3,
    m = 3, T = 4, log_std_init (-1, -0.5, 0.25): two iterations of collect(sde_sample_freq=(-1, 2, 1)) + train(n_epochs=2,
    batch_size=5, splits) equal VectorContinuousJumps with Rollout + LstmSdePopulationPolicy + PopulationLearner: every slab
    (raw actions among them), flat(), episode_starts, lstm_states, theta, stats, parameters, optimizer states, generator
    states and the final lstm_state().  Then a second policy and learner resumed from both state_dict()s repeat a train()
    bit for bit."""
    _passed(recorded, f"end-to-end/{critic}")


def test_the_classes_refuse_with_a_message(recorded):
    """n not divisible by the groups, a wrong number of seeds, log_std_init, sde_sample_freq or a mask of the wrong length,
    a Discrete space, specs of the three other kinds, a sampled act() before every group has noise, rows, starts and states of
    the wrong shape, batch_size > m T, splits and firsts of the wrong shape or range, a rollout with another groups=, one
    collected without a recurrent policy, one on the host -- no draw consumed by any of them; a sharded environment."""
    _passed(recorded, "surface")
    _passed(recorded, "sharded")
