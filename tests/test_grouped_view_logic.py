"""CPU tests of the population view (include/reinfocus_hip.h, "population view"): harness.LearnerView(groups=G, gamma=[...])
on the numpy twins, held by hand to G private _LearnerView objects fed slice by slice; groups=1 against groups=None;
rollout.gae_numpy_grouped against gae_numpy per column slice; what is refused; the ctypes binding against the header;
and, for every case of tests/test_gpu_grouped_view.py, that its seed gives the episode ends the case relies on."""

import ctypes
import os
import re

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, policy, rollout
from tests import grouped_view_io_cases as cases
from tests import rollout_io_cases
from tests import test_gpu_snapshot as gpu
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = cases.ROOT
bits = cases.bits


def _twin(case):
    view = cases.make_view(case)
    if case["kind"].startswith("composed"):
        return cases.make_twin_env(case, episode_records=case["records"], learner_view=view)
    return harness.VectorDiscreteSteps(num_envs=case["n"], episode_records=case["records"], learner_view=view, **gpu.TASK_KW)


def _driven(case):
    env = _twin(case)
    try:
        return cases.drive_view(case, env, env.reset, lambda index, actions: env.step(actions),
                                lambda e: e.set_view_training(False))
    finally:
        env.close()


# ---- 1: the twins, by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [
    dict(kind="composed-i64", n=65, groups=13, records=True, config={}, freeze=False),
    dict(kind="composed-i32", n=64, groups=8, records=False, config={}, freeze=True),
    dict(kind="steps-i64", n=12, groups=3, records=True, config=dict(norm_reward=False), freeze=False),
    dict(kind="steps-i64", n=6, groups=6, records=False, config=dict(norm_obs=False), freeze=False)], ids=cases.case_id)
def test_grouped_twins_equal_private_views_fed_slice_by_slice(case, no_gpu):  # noqa: F811
    """VectorEnvironment and VectorDiscreteSteps: every byte of observation, reward, final_observation, view_state() and
    view_statistics() after every step."""
    done = _driven(case)
    assert done.any()


def test_one_group_is_the_ungrouped_view(no_gpu):  # noqa: F811
    n = 65
    case = dict(kind="composed-i64", n=n, groups=1, records=True, config={}, freeze=False)
    plain = cases.make_twin_env(case, episode_records=True, learner_view=harness.LearnerView(frame_stack=5, gamma=0.9))
    one = cases.make_twin_env(case, episode_records=True,
                              learner_view=harness.LearnerView(frame_stack=5, gamma=[0.9], groups=1))
    a, b = plain.reset(), one.reset()
    assert bits(a[0]) == bits(b[0])
    rng = np.random.default_rng(6)
    for _ in range(cases.STEPS):
        actions = rng.integers(0, 13, n)
        x, y = plain.step(actions), one.step(actions)
        assert sorted(x[4]) == sorted(y[4])
        assert all(bits(p) == bits(q) for p, q in zip(x[:4], y[:4]))
        assert all(bits(x[4][key]) == bits(y[4][key]) for key in x[4])
        assert all(bits(p) == bits(q) for p, q in zip(plain.view_state(), one.view_state()))
        s, t = plain.view_statistics(), one.view_statistics()
        assert all(t[key].shape == (1, 5) and bits(s[key]) == bits(t[key][0]) for key in s)  # only the shape differs
        assert all(bits(one.view_statistics(group=0)[key]) == bits(s[key]) for key in s)
    plain.close(), one.close()


def test_statistics_of_one_group(no_gpu):  # noqa: F811
    case = dict(kind="steps-i64", n=12, groups=3, records=False, config={}, freeze=False)
    env = _twin(case)
    statistics = cases.statistics_of(3)
    env.set_view_statistics(statistics)
    row = {key: value[1] + 1.0 for key, value in statistics.items()}
    env.set_view_statistics(row, group=1)
    got = env.view_statistics()
    assert all(bits(got[key][1]) == bits(row[key]) and bits(got[key][0]) == bits(statistics[key][0]) for key in row)
    assert all(bits(env.view_statistics(group=1)[key]) == bits(row[key]) and row[key].shape == (5,) for key in row)
    for bad in (-1, 3, 0.5):
        with pytest.raises(ValueError, match="group"):
            env.view_statistics(group=bad)
    env.close()
    plain = harness.VectorDiscreteSteps(num_envs=4, learner_view=harness.LearnerView(), **gpu.TASK_KW)
    with pytest.raises(ValueError, match="groups="):
        plain.view_statistics(group=0)
    plain.close()


# ---- 2: GAE ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bootstrap", [True, False])
@pytest.mark.parametrize("n, groups", cases.GAE_SHAPES)
@pytest.mark.parametrize("steps", cases.GAE_STEPS)
def test_grouped_gae_is_gae_per_group(steps, n, groups, bootstrap):
    rewards, values, truncated, final_values, last_values = cases.gae_inputs(steps, n, 7)
    final_values = final_values if bootstrap else None
    gammas, lambdas = cases.gammas_of(groups), cases.lambdas_of(groups)
    got = rollout.gae_numpy_grouped(rewards, values, truncated, final_values, last_values, gammas, lambdas)
    m = n // groups
    for g in range(groups):
        lanes = slice(g * m, (g + 1) * m)
        want = rollout.gae_numpy(rewards[:, lanes], values[:, lanes], truncated[:, lanes],
                                 None if final_values is None else final_values[:, lanes], last_values[lanes], gammas[g],
                                 lambdas[g])
        assert bits(got[0][:, lanes]) == bits(want[0]) and bits(got[1][:, lanes]) == bits(want[1])
    if groups == 1:
        want = rollout.gae_numpy(rewards, values, truncated, final_values, last_values, gammas[0], lambdas[0])
        assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])


def test_discount_table_takes_the_product_in_float64():
    table = rollout.discount_table((rollout_io_cases.GAMMA, 1.0, 0.0), (rollout_io_cases.GAE_LAMBDA, 0.5, 1.0))
    assert table.dtype == np.float32 and table.shape == (3, 2)
    gamma, gae_lambda = rollout_io_cases.GAMMA, rollout_io_cases.GAE_LAMBDA
    assert table[0, 0] == np.float32(gamma) and table[0, 1] == np.float32(gamma * gae_lambda)
    assert table[0, 1] != np.float32(gamma) * np.float32(gae_lambda)  # (a wrong gl would show)
    assert table[1].tolist() == [1.0, 0.5] and table[2].tolist() == [0.0, 0.0]


def test_grouped_rollout_on_a_twin(no_gpu):  # noqa: F811
    """Rollout(groups=G): finish() is gae_numpy_grouped with the attributes as they are at the time."""
    env = harness.VectorDiscreteSteps(num_envs=6, episode_records=True, **gpu.TASK_KW)
    buffer = harness.Rollout(env, 3, (0.9, 0.5, 1.0), 0.95, groups=3)
    obs, _ = env.reset()
    buffer.start(obs)
    for t in range(3):
        values = obs[:, 0] * np.float32(0.5)
        obs, _, _, _, info = buffer.step(rollout_io_cases.index_schedule(t, 6), values, -values)
        buffer.bootstrap(info["final_observation"][:, 0] * np.float32(0.5))
    last = obs[:, 0] * np.float32(0.5)
    got = buffer.finish(last)
    want = rollout.gae_numpy_grouped(buffer.rewards, buffer.values, buffer.truncated, buffer.final_values, last,
                                     (0.9, 0.5, 1.0), (0.95,) * 3)
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    buffer.gamma, buffer.gae_lambda = 0.8, (0.0, 1.0, 0.5)  # plain attributes, read by the next finish()
    got = buffer.finish(last)
    want = rollout.gae_numpy_grouped(buffer.rewards, buffer.values, buffer.truncated, buffer.final_values, last,
                                     (0.8,) * 3, (0.0, 1.0, 0.5))
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    env.close()


# ---- 3: what is refused ----------------------------------------------------------------------------------------------------
def test_refusals(no_gpu):  # noqa: F811
    with pytest.raises(ValueError, match="needs groups="):
        harness.LearnerView(gamma=[0.9, 0.8])
    for bad in (dict(groups=0), dict(groups=65536), dict(groups=1.5), dict(groups=2, gamma=[0.9]),
                dict(groups=2, gamma=[0.9, 1.5]), dict(groups=2, gamma=[0.9, np.nan]), dict(groups=2, gamma=-0.1)):
        with pytest.raises(ValueError):
            harness.LearnerView(**bad)
    view = harness.LearnerView(frame_stack=2, gamma=[0.9, 0.8, 0.7], groups=3)
    for make in (lambda: harness.VectorDiscreteSteps(num_envs=4, learner_view=view, **gpu.TASK_KW),
                 lambda: harness.VectorEnvironment(**gpu.stopped_objects(7), learner_view=view, frame_height=16,
                                                   samples_per_pixel=1, device=0)):
        with pytest.raises(ValueError, match="do not divide"):
            make()
    for cls in (harness.ShardedVectorDiscreteSteps, harness.ShardedVectorContinuousJumps):
        with pytest.raises(ValueError, match="sharded"):
            cls(num_envs=6, devices=[0, 0], frame_height=8, samples_per_pixel=1, learner_view=view)
    for cls in (harness.DiscreteSteps, harness.ContinuousJumps):
        with pytest.raises(ValueError, match="single-environment"):
            cls(frame_height=8, samples_per_pixel=1, learner_view=view)
    # the rollout
    env = harness.VectorDiscreteSteps(num_envs=6, learner_view=view, **gpu.TASK_KW)
    with pytest.raises(ValueError, match="groups="):
        harness.Rollout(env, 4, (0.9, 0.8, 0.7), 0.95)
    with pytest.raises(ValueError, match="groups="):
        harness.Rollout(env, 4, 0.9, (0.95, 0.9, 0.8))
    with pytest.raises(ValueError, match="learner view has groups=3"):
        harness.Rollout(env, 4, 0.9, 0.95, groups=2)
    with pytest.raises(ValueError, match="do not divide"):
        harness.Rollout(env, 4, 0.9, 0.95, groups=4)
    with pytest.raises(ValueError, match="one per group"):
        harness.Rollout(env, 4, (0.9, 0.8), 0.95, groups=3)
    grouped = harness.Rollout(env, 2, (0.9, 0.8, 0.7), 0.95, groups=3)
    ungrouped = harness.Rollout(env, 2, 0.9, 0.95)
    spec = policy.MlpPolicySpec(8, 13, pi=(5,), vf=(4,), activation="tanh")
    other = harness.PopulationPolicy(spec, 2, [1, 2])
    obs, _ = env.reset()
    grouped.start(obs)
    with pytest.raises(ValueError, match="population policy of 2 groups"):
        grouped.collect(other)
    grouped.collect(harness.PopulationPolicy(spec, 3, [1, 2, 3]))
    ungrouped.start(env.reset()[0])
    ungrouped.collect(other)  # an ungrouped rollout with a population policy keeps working
    grouped.gamma = (0.9, 0.8)
    with pytest.raises(ValueError, match="one per group"):
        grouped.finish(np.zeros(6, dtype=np.float32))
    env.close()


def test_describe():
    assert harness.LearnerView(frame_stack=5).describe() == (
        "LearnerView(frame_stack=5, norm_obs=True, norm_reward=True, gamma=0.99, epsilon=1e-08, clip_obs=10.0, "
        "clip_reward=10.0)")
    text = harness.LearnerView(frame_stack=5, gamma=[0.5, 1.0], groups=2).describe()
    assert "groups=2" in text and "gamma=(0.5, 1.0)" in text
    assert harness.LearnerView(gamma=0.5, groups=2).gammas == (0.5, 0.5)
    assert harness.LearnerView().groups is None


# ---- 4: the binding --------------------------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read(), flags=re.S)
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    kinds = {"vp": ctypes.c_void_p, "i32": ctypes.c_int, "ctypes.POINTER(EnvViewConfig)": ctypes.c_void_p}
    for entry, count in (("rf_env_configure_view_grouped", 4), ("rf_env_view_get_statistics_grouped", 4),
                         ("rf_env_view_set_statistics_grouped", 4), ("rf_rollout_advantages_grouped", 13)):
        declaration = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % entry, text, flags=re.S).group(1)
        wanted = [ctypes.c_void_p if "*" in p else ctypes.c_int for p in declaration.split(",")]
        names = re.search(r"lib\.%s\.argtypes = \[(.*?)\]" % entry, source, flags=re.S).group(1).split(",")
        assert [kinds[name.strip()] for name in names] == wanted and len(wanted) == count, entry
        assert entry in _native.SYMBOLS
    assert int(re.search(r"#define RF_POPULATION_MAX_GROUPS (\d+)", text).group(1)) == harness.MAX_VIEW_GROUPS
    header = re.search(r"typedef struct rf_env_snapshot_header \{(.*?)\} rf_env_snapshot_header;", text, flags=re.S).group(1)
    assert re.search(r"int32_t view_training;\s*int32_t view_groups;\s*uint8_t zero\[136\];", header)  # 256 bytes still


# ---- 5: what the GPU cases rely on -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.VIEW_CASES, ids=cases.case_id)
def test_seeds_of_the_gpu_cases_give_the_ends_they_rely_on(case, no_gpu):  # noqa: F811
    """For every (kind, n, G, seed) of tests/test_gpu_grouped_view.py, with the numpy twins: some step has a group where
    none end, some step one where all end, and -- where a group has more than one lane -- some step one where some but
    not all end.  (With m = 1 a group is one lane: it ends or it does not.)  The twin is held to the oracle on the way."""
    done = _driven(case)
    cases.ends_promises(done, case["groups"])


def test_the_gpu_shapes_cover_both_forms():
    shapes = {(case["n"], case["groups"]) for case in cases.VIEW_CASES}
    assert shapes == set(cases.VIEW_SHAPES)
    pm = lambda m: 1 << (m - 1).bit_length()  # noqa: E731
    sizes = sorted(pm(n // groups) for n, groups in cases.VIEW_SHAPES)
    assert sizes == [1, 8, 8, 32, 64, 128, 2048]  # the packed form up to a wave, the block form with one and two leaves
    records = {case["records"] for case in cases.VIEW_CASES if not case["config"] and not case["freeze"]}
    assert records == {True, False}
    assert all(0.0 in cases.gammas_of(g) and 1.0 in cases.gammas_of(g) for _, g in cases.VIEW_SHAPES)
    assert all(len(set(cases.gammas_of(g)[:7])) == min(g, 7) for _, g in cases.VIEW_SHAPES)
