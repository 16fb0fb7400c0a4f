"""GPU tests of the parameter initialisation (rf_params_init: param_fill_kernel and param_orthogonal_kernel of
csrc/rf_param_init.h; init_parameters of the eight device policy classes) against the numpy twin
(environments/param_init.py) bit for bit: every array is compared as bytes, every output is sentinel-filled between guard
floats first.

As tests/test_gpu_population_lstm_sde.py: the cases need torch and the library in one process, so they run in ONE fresh
child process that imports torch first (tests/param_init_io_cases.py), started once per session and never replaced; each
test below looks its case up.  tests/test_param_init_logic.py holds the twin to the host build of the same header."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers
from tests import param_init_io_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("param_init") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.param_init_io_cases", path], cwd=helpers.ROOT, capture_output=True,
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


def test_one_seed_has_a_high_state_word():
    from reinfocus_amd.environments.policy import generator_words

    assert any(generator_words(np.random.PCG64DXSM(seed))[1] >> 32 for seed in cases.SEEDS)


@pytest.mark.parametrize("ortho_init", cases.SCHEMES)
@pytest.mark.parametrize("name", sorted(cases.KERNEL_SPECS))
def test_params_init_equals_the_twin(name, ortho_init, recorded):
    """rf_params_init at G = 3 (seeds 3, 2^70 + 5, 11; every group its own log_std_init where the head has one) for the
    masks None, (1, 0, 1) and (0, 0, 0): the selected groups are the twin's bytes, unselected groups and the guard floats
    keep their sentinel bytes.  mlp: D = 5, pi = (7,), vf = (3, 2), A = 3 (out > in, out < in, 1 x K, odd sizes); mlp-64:
    D = 25, pi = vf = (64, 64), A = 7; mlp-256: D = 256, pi = (256,), vf = (256, 1), A = 64 (t = s = 256, the full block, and
    an in = 1 head input); the recurrent heads at H = 16 and H = 256 with D = 25, both critic kinds, with and without the
    Gaussian head."""
    _passed(recorded, f"kernel/{name}/{int(ortho_init)}")


def test_positions_outside_every_segment_keep_their_bytes(recorded):
    _passed(recorded, "outside")


def test_params_init_refusals(recorded):
    """More than 32 segments, overlapping and out-of-range segments, an unknown scheme, a non-finite or non-positive scale,
    CONSTANT without constants, orthogonal segments without a workspace, G and stride outside their limits, a NULL generator
    table, a workspace that overlaps the parameters: refused with a message, nothing written."""
    _passed(recorded, "kernel-refusals")


@pytest.mark.parametrize("kind", cases.POPULATION_KINDS)
def test_device_classes_equal_their_twins(kind, recorded):
    """Device*Policy.init_parameters equals its twin for both schemes; the device population equals the twin population for
    the three masks, G stand-alone device objects, and at G = 1 the ungrouped class; rng_state() is unchanged."""
    _passed(recorded, f"classes/{kind}")


def test_device_class_refusals(recorded):
    _passed(recorded, "surface")


def test_training_from_the_device_init_equals_the_twin(recorded):
    """DevicePolicy: after init_parameters one act() and one update() equal the twin started from the same init."""
    _passed(recorded, "train/mlp")


def test_training_a_recurrent_population_from_the_device_init_equals_the_twin(recorded):
    """DevicePopulationLstmPolicy at G = 2, m = 2, H = 4: the same, through DevicePopulationLearner."""
    _passed(recorded, "train/population")
