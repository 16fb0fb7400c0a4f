"""GPU tests of the population view (include/reinfocus_hip.h, "population view"): a learner view with running moments
and a gamma per group of lanes (rf_env_configure_view_grouped: env_view_moments_packed_kernel for groups of at most 64
lanes, env_view_moments_kernel<true> beyond, env_view_apply_kernel<true>), GAE with discounts per group
(rf_rollout_advantages_grouped: rollout_gae_kernel<true>), snapshots of a grouped view, what the library refuses, and a
population trained end to end over a grouped view through a grouped DeviceRollout.  Everything is compared as bytes
against the numpy twins.

One child process that imports torch first runs every case (tests/grouped_view_io_cases.py); frames have 16 x 16 pixels
and 1-2 samples.  tests/test_grouped_view_logic.py checks on the CPU that the cases' seeds give the episode ends they
rely on.

End to end: the least network of tests/population_io_cases.NETWORKS has 3 observation columns and 3 actions, the
environment 4 and 13; the case takes that network's hidden layers and activation at the environment's widths."""

import json
import os
import subprocess
import sys

import pytest

from tests import grouped_view_io_cases as cases
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("grouped_view_io") / "cases.jsonl")
    done = subprocess.run([sys.executable, "-m", "tests.grouped_view_io_cases", path], cwd=helpers.ROOT,
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


@pytest.mark.parametrize("case", cases.VIEW_CASES, ids=cases.case_id)
def test_grouped_view_equals_private_views_per_group(case, recorded):
    """12 steps mixing step() and step_tensors(), per-group gammas that include 0.0 and 1.0, distinct per-group
    statistics set before the first step: observation, reward, final_observation, view_state() and view_statistics()
    equal, as bytes, G private _LearnerView objects fed the raw step slice by slice."""
    _passed(recorded, cases.case_id(case))


def test_one_group_is_the_ungrouped_context(recorded):
    _passed(recorded, "one group")


@pytest.mark.parametrize("steps", cases.GAE_STEPS)
def test_grouped_gae_equals_the_twin(steps, recorded):
    """(n, G) of GAE_SHAPES, with and without final_values (NaN where not truncated), per-group gamma and lambda that
    include 0 and 1; G = 1 is byte-equal to rf_rollout_advantages."""
    _passed(recorded, f"gae/{steps}")


def test_refusals_come_before_anything_is_enqueued(recorded):
    _passed(recorded, "refusals")


def test_snapshots_carry_a_grouped_view_and_refuse_another(recorded):
    _passed(recorded, "snapshots")


def test_population_over_a_grouped_view_end_to_end(recorded):
    _passed(recorded, "end to end")
    _passed(recorded, "finished")
