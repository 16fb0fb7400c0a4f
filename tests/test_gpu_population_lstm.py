"""GPU tests of the population of recurrent PPO learners (harness.DevicePopulationLstmPolicy / DevicePopulationLearner
over it, rf_lstm_forward_grouped, rf_lstm_ppo_update_grouped; the grouped instantiations of the kernels of csrc/rf_lstm.h
and csrc/rf_lstm_ppo.h) against the numpy twins (harness.LstmPopulationPolicy / PopulationLearner) bit for bit, and against
stand-alone rf_lstm_forward / rf_lstm_ppo_update launches (their rf_lstm_critic_ siblings with the feed-forward critic) and
DeviceLstmPolicy / DeviceLstmLearner objects on the same device: every array is compared as bytes.

As tests/test_gpu_population.py: the cases need torch and the library in one process, so they run in ONE fresh child
process that imports torch first (tests/population_lstm_io_cases.py), started once per session and never replaced; each
test below looks its case up.  tests/test_population_lstm_logic.py holds the twins to G independent existing twins on the
CPU, on the same inputs.

Development run on an MI355X: all 82 tests pass, the child process takes 15.2 s (7.4 s on the same machine before the
cases on the limit layouts and at 65535 groups; the difference is the numpy twins of the 13 layout cases)."""

import json
import os
import subprocess
import sys

import pytest

from tests import helpers
from tests import population_lstm_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("population_lstm") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.population_lstm_io_cases", path], cwd=helpers.ROOT,
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


_network = pytest.mark.parametrize("index", cases.NETS, ids=lambda i: "-".join(str(v) for v in cases.lstm_cases.NETWORKS[i]))
_critic = pytest.mark.parametrize("critic", [cases.critic_name(c) for c in cases.CRITICS])


@pytest.mark.parametrize("per_group", cases.PER_GROUP)
@pytest.mark.parametrize("groups", cases.GROUPS)
@_network
@_critic
def test_grouped_forward_equals_the_twin_population(critic, index, groups, per_group, recorded):
    """rf_lstm_forward_grouped on hostile device tensors, every group with parameters of its own and a state around its own
    non-zero level, mixed start bytes: sampled with 0 and with 2^32 + 5 draws taken before, deterministic, the state in
    place and from `in` to `out`, values only (the state stays); all four outputs and the whole output state -- the vf
    half with the linear critic included -- as bytes; final_obs with NaN rows among live ones; every output a slice of a
    larger slab and the states between guard floats.  Then G stand-alone rf_lstm_forward (rf_lstm_critic_forward) launches
    on contiguous copies of the groups' rows and state columns give the same bytes."""
    _passed(recorded, f"forward/{critic}/{index}/{groups}/{per_group}")


@_network
@_critic
def test_the_state_keeps_its_plane_stride(critic, index, recorded):
    """G = 3, m = 3, a distinct non-zero state per group: the grouped launch equals the twin, and the twin over the same bytes
    read as [G][2][2][m][H] gives another next state and other log-probabilities -- a kernel that added g times a size to
    the state pointer could not pass."""
    _passed(recorded, f"stride/{critic}/{index}")


@pytest.mark.parametrize("batch", cases.UPDATE["batches"])
@_network
@_critic
def test_grouped_update_equals_the_twin_population(critic, index, batch, recorded):
    """rf_lstm_ppo_update_grouped, three groups of (T, m) = (4, 3) whose hyper-parameters, parameters and sequence
    structures all differ, firsts (0, 7, 11) -- one group does not wrap, two wrap at different rows --, B = 5 and 12 = N, two
    consecutive updates: parameters, optimizer states and stats [G][8] as bytes between guard floats, the workspace of
    exactly rf_lstm_ppo_grouped_workspace_size's bytes between guards.  Then G stand-alone rf_lstm_ppo_update
    (rf_lstm_critic_ppo_update) launches on contiguous slice copies give the same bytes."""
    _passed(recorded, f"update/{critic}/{index}/{batch}")


def test_update_at_the_widest_cell(recorded):
    """H = 256 (sb3-contrib's default network), G = 2, m = 2, T = 3, B = 6 = m T, both critic kinds, against the twin."""
    _passed(recorded, "limit")


_LAYOUTS = [(name, cases.critic_name(critic_lstm)) for name, case in cases.LAYOUT_CASES.items()
            for critic_lstm in case["critics"]]


@pytest.mark.parametrize("name,critic", _LAYOUTS)
def test_grouped_update_on_the_limit_layouts(name, critic, recorded):
    """rf_lstm_ppo_update_grouped on the layouts the ungrouped update is held to (tests/lstm_learner_io_cases.py's
    LIMIT_LAYOUTS), every group with its own parameters, hyper-parameters, first row and -- its columns rolled -- sequence
    structure, against PopulationLearner group by group: parameters, optimizer states and stats as bytes between guard
    floats, the workspace of exactly rf_lstm_ppo_grouped_workspace_size(B)'s bytes between guards.
    depth: T = 17, m = 4, sequences of 1, 8, 9, 16 and 17 rows (past the 8 rows whose weights both walks load before
    the first is used: the steady state of that prefetch and its tails), through the group's lane window of stride G m.
    G = 3 on ppo_lstm_tuned.yml's network at B = 65 with firsts (0, 5, 30) and at B = 68 = N with firsts (5, 0, 67), two
    groups wrapping at different rows; both also as three stand-alone rf_lstm_ppo_update (rf_lstm_critic_ppo_update)
    launches on contiguous slice copies.  G = 2 on sb3-contrib's default network (H = 256: every thread of a block owns a
    unit, parameters at g P) at B = 65.  Two consecutive updates each.
    untuned: ppo_lstm_untuned.yml's T = 128, m = 8, B = 128 with drawn starts, firsts (0, 100, 1000): group 1 crosses an
    environment boundary, group 2 wraps, every group holds a sequence of more than 64 rows and one of one row; G = 3 on
    the tuned network (two updates) and G = 2 on the default network with the LSTM critic, the real shape (one update).
    wave: T = 16, m = 64, N = 1024, G = 2 on the tuned network, one update: every row a start at B = 1024 from rows
    (7, 0) -- 1024 one-row sequences per group, 128 MLP tiles, the second trip of the reductions --, and no flagged start
    at B = 513 from rows (0, 9).
    tests/test_population_lstm_logic.py shows without a GPU that the layouts hold these sequences and that no update of the
    twin is skipped or leaves a group with a learning rate where it was."""
    _passed(recorded, f"layout/{name}/{critic}")


@_critic
def test_forward_and_update_at_the_group_limit(critic, recorded):
    """G = RF_POPULATION_MAX_GROUPS = 65535 groups of one environment on the least network.  rf_lstm_forward_grouped at
    m = 1, sampled (generator g % 11, 2^32 + 5 draws taken before) and deterministic, the state in place;
    rf_lstm_ppo_update_grouped at m = T = B = 1 of fresh optimizers.  Group g has parameter set g % 7, input block g % 5
    with its state on a level of its own and hyper-parameter set g % 3, so neighbours differ in all of them and a wrong
    stride of parameters, states, workspace, stats, rows or state planes shows at every g; every output byte of every
    group -- the next state included -- is compared with the twin functions' result for its combination.  Where
    g % 11 = 5, firsts[g] = 1 = N: those 5958 groups carry RF_PPO_INVALID and keep parameters and optimizer state byte
    for byte, their neighbours equal the twin.  (65536 groups are refused: test_refusals_come_before_anything_is_enqueued.)"""
    _passed(recorded, f"group-limit/{critic}")


@_critic
def test_a_skipped_group_leaves_the_others_alone(critic, recorded):
    """A NaN advantage in group 1's minibatch: group 1 carries RF_PPO_NONFINITE and keeps parameters and optimizer state byte
    for byte, groups 0 and 2 equal a run without the NaN.  The same with firsts[1] = N, out of range: RF_PPO_INVALID."""
    _passed(recorded, f"isolation/{critic}")


@pytest.mark.parametrize("groups,per_group", cases.WIDE_FORWARD)
def test_grouped_forward_at_many_groups(groups, per_group, recorded):
    """512 groups of one environment and 65 groups of eight on ppo_lstm_tuned.yml's network: group indices far past 4."""
    _passed(recorded, f"forward/wide/{groups}/{per_group}")


def test_grouped_update_at_64_groups_on_the_tuned_shape(recorded):
    """One rf_lstm_ppo_update_grouped at G = 64, m = 8, T = 8, B = 8, H = 16, every group its own first row and
    hyper-parameters that differ between neighbours, against PopulationLearner: all 64 groups as bytes."""
    _passed(recorded, "update/wide")


def test_refusals_come_before_anything_is_enqueued(recorded):
    """Host and NULL pointers (arrays, d_gens, d_firsts, d_hyper), G, m or T outside the limits, B > m T, a critic kind that
    does not exist, misaligned and overlapping arrays, a state_out that overlaps state_in without being it, a capturing
    caller stream: every sentinel-filled output keeps its bytes, and the unchanged call is then taken."""
    _passed(recorded, "kernel-refusals")


@_critic
def test_one_group_is_the_ungrouped_path(critic, recorded):
    """G = 1 next to DeviceLstmPolicy / DeviceLstmLearner with the same seed: act() sampled and deterministic, the state,
    values(), three chained updates, rng_state(), parameters and optimizer state, bit for bit."""
    _passed(recorded, f"one-group/{critic}")


@_critic
def test_collect_and_train_equal_the_twins(critic, recorded):
    """DeviceVectorDiscreteSteps at 9 envs x 16 x 16 px x 1 sample with device_initializer and episode_records, G = 3,
    m = 3, T = 4: two iterations of collect + train(n_epochs=2, batch_size=5, splits) equal VectorDiscreteSteps with
    Rollout + LstmPopulationPolicy + PopulationLearner: every slab, flat(), episode_starts, lstm_states, stats, parameters,
    optimizer states, generator states and the final lstm_state().  Then a second policy and learner resumed from both
    state_dict()s repeat a train() bit for bit."""
    _passed(recorded, f"end-to-end/{critic}")


def test_the_classes_refuse_with_a_message(recorded):
    """n not divisible by the groups, a wrong number of seeds, a Box space and an LstmSdePolicySpec (the next step), an
    MlpPolicySpec, rows, starts and states of the wrong shape, batch_size > m T, splits and firsts of the wrong shape or
    range, a rollout with another groups=, one collected without a recurrent policy, one on the host; a sharded
    environment."""
    _passed(recorded, "surface")
    _passed(recorded, "sharded")
