"""GPU tests of the evaluation (rf_eval_accumulate, rf_eval_finish, rf_eval_keep_rows, rf_env_view_get / set_statistics_device;
csrc/rf_eval.h; harness.DeviceEvaluation) against the numpy twin (environments/evaluation.py) bit for bit: every array is
compared as bytes, every output is filled with a known byte between guard bytes first.

As tests/test_gpu_param_init.py: the cases need torch and the library in one process, so they run in ONE fresh child
process that imports torch first (tests/evaluation_io_cases.py), started once per session and never replaced; each test
below looks its case up.  tests/test_evaluation_logic.py holds the twin to the host build of the same header."""

import json
import os
import subprocess
import sys

import pytest

from tests import evaluation_io_cases as cases
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("evaluation") / "cases.jsonl")
    # a fresh process (never an exec of this one), ended by its own time limit
    done = subprocess.run([sys.executable, "-m", "tests.evaluation_io_cases", path], cwd=helpers.ROOT, capture_output=True,
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


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_accumulate_and_finish_equal_the_twin(shape, recorded):
    """rf_eval_accumulate / rf_eval_finish over nine evaluations in a row (lanes that end every step, a tie, an
    improvement, lanes that end at random, a group that never ends, NaN / +-inf / +-0.0 returns): counts, tables, rows,
    best_mean, best_serial and improved are the twin's bytes after every one, and no guard byte is written.  G in {1, 3},
    m in {3, 8, 11}, E in {2, 5, 20}; E = 300 at m = 3 (K = 100, two leaves per thread), E = 257 and E = 1."""
    _passed(recorded, "kernel/" + cases.shape_id(shape))


@pytest.mark.parametrize("words", cases.KEEP_WORDS)
def test_keep_rows_copies_the_selected_rows_only(words, recorded):
    """rf_eval_keep_rows at G = 3 for the masks (1, 0, 1), (0, 0, 0) and all ones; rows of 1, 3, 4, 1023 and 1028 words (the
    dword tail, the 16-byte body, a second block), packed and 5 words apart, into a destination that shares the source's
    alignment and into one a word off it: unselected rows, gaps and guards keep their bytes."""
    _passed(recorded, f"keep/{words}")


def test_kernel_refusals(recorded):
    """E outside 1 .. 65 536, n != G m, NULL / host / misaligned / short / overlapping arrays, a serial of 2^53, words
    outside 1 .. stride, a capturing stream: refused with a message, nothing written."""
    _passed(recorded, "kernel-refusals")


@pytest.mark.parametrize("grouped", (False, True))
def test_statistics_round_trip_on_the_device(grouped, recorded):
    """view_statistics_tensor() equals view_statistics() as bytes, set_view_statistics_tensor() sets exactly them in another
    environment; a wrong dtype, device, shape or type is refused."""
    _passed(recorded, f"statistics/{int(grouped)}")


@pytest.mark.parametrize("kind", cases.E2E_KINDS)
def test_device_evaluation_equals_the_twin(kind, recorded):
    """One Categorical, one sde, one lstm and one lstm-sde population at G = 3, m = 3, E = 5, with grouped learner views:
    DeviceEvaluation.run equals Evaluation.run as bytes (rows, tables, best_*), a second run after groups 0 and 2 were
    re-initialised keeps the better group-wise, load_best((0, 1, 1)) restores only the selected groups, state_dict()
    resumes, and rng_state(), noise() and lstm_state() are byte for byte what they were."""
    _passed(recorded, f"e2e/{kind}")


@pytest.mark.parametrize("kind", cases.E2E_KINDS)
def test_training_after_an_evaluation_is_training_without_it(kind, recorded):
    _passed(recorded, f"training/{kind}")


def test_ungrouped_policy_is_one_group(recorded):
    _passed(recorded, "single")


def test_device_evaluation_refusals(recorded):
    """No episode records, another device, another n, groups, width or action space, a host-drawn initializer, a sharded or
    a twin environment, a twin policy, n_eval_episodes outside its limits, max_steps < 1, deterministic=False: each refused
    by its message before anything is enqueued."""
    _passed(recorded, "surface")
