"""CPU tests of the evaluation (include/reinfocus_hip.h, "evaluation"; environments/evaluation.py): the targets against
stable-baselines3's formula, the numpy twin against the host build of csrc/rf_eval.h (tests/evalcheck) as bytes on
synthetic record streams, the tree's mean and standard deviation against math.fsum, Evaluation.run over twin environments
against a literal restatement of SB3's evaluate_policy loop, and the refusals.  tests/test_gpu_evaluation.py holds the
kernels to the same twin on the device.  The GPU's render and focus measure are replaced by a function of the state
(tests/test_composed_env_logic.py::no_gpu)."""

import math

import numpy as np
import pytest

from reinfocus_amd.environments import evaluation, harness
from tests import evaluation_io_cases as cases
from tests import test_composed_env_logic as composed
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

bits = cases.bits
GRID = [(m, E) for m in (3, 8, 11) for E in (1, 2, 5, 20, 300)]


@pytest.fixture(scope="module")
def host():
    return cases.hostcheck()


# ---- 1: targets, slots and positions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,E", GRID)
def test_targets_are_sb3s_and_sum_to_the_episodes(m, E, host):
    want = np.array([(E + i) // m for i in range(m)], dtype="int")  # evaluate_policy's episode_count_targets, verbatim
    got = evaluation.targets(m, E)
    assert got.dtype == np.int32 and (got == want).all() and got.sum() == E
    assert [host.evc_target(m, E, i) for i in range(m)] == list(want)
    assert evaluation.slots(m, E) == host.evc_slots(m, E) == want.max() == -(-E // m)
    assert [host.evc_first(m, E, i) for i in range(m)] == [int(want[:i].sum()) for i in range(m)]
    # every position is one (lane, slot) below the lane's target, lane-major and slot-minor
    pairs = [(i, k) for i in range(m) for k in range(want[i])]
    at = np.zeros(2, dtype=np.int32)
    for p, pair in enumerate(pairs):
        host.evc_locate(m, E, p, cases._p(at))
        assert tuple(at) == pair


def test_fewer_episodes_than_lanes_leave_lanes_without_a_target():
    assert list(evaluation.targets(3, 2)) == [0, 1, 1] and list(evaluation.targets(8, 5)) == [0, 0, 0, 1, 1, 1, 1, 1]
    counts, returns, lengths = evaluation.tables(3, 3, 2)
    for step in range(3):
        evaluation.accumulate_numpy(counts, returns, lengths, np.full(3, 1.0 + step), np.full(3, 4, dtype=np.int32), 3, 2)
    assert list(counts) == [0, 1, 1] and returns.shape == (3, 1) and list(returns[:, 0]) == [0.0, 1.0, 1.0]


def test_leaves_per_thread(host):
    assert [host.evc_leaves(E) for E in (1, 5, 256, 257, 300, 512, 513, 65536)] == [1, 1, 1, 2, 2, 2, 4, 256]


# ---- 2: the twin is the host build, as bytes -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_twin_equals_the_host_build(shape, host):
    """Nine evaluations in a row over the same best_*: lanes that end every step, a tie, an improvement, lanes that end at
    random, a group that never ends, NaN / +-inf / +-0.0 returns (a NaN mean from inf - inf included)."""
    wrong = cases.first_difference(cases.scenario(cases.host_backend(host), shape), cases.twin_scenario(shape))
    assert wrong is None, wrong


def _rows(shape):
    return [np.frombuffer(seen["results"][2], dtype=np.float64).reshape(shape[0], 8) for seen in cases.twin_scenario(shape)], \
        [np.frombuffer(seen["improved"][2], dtype=np.uint8) for seen in cases.twin_scenario(shape)]


def test_the_scenarios_reach_what_they_are_for():
    shape = (3, 8, 5)
    rows, improved = _rows(shape)
    kinds = {kind: index for index, kind in enumerate(cases.KINDS)}
    assert improved[kinds["all"]].all() and not improved[kinds["tie"]].any() and improved[kinds["higher"]].all()
    assert bits(rows[kinds["all"]][:, :5]) == bits(rows[kinds["tie"]][:, :5])
    never = rows[kinds["never"]]
    assert never[2, 6] == evaluation.INCOMPLETE and np.isnan(never[2, :5]).all() and never[2, 5] == 0
    assert (never[:2, 6] == 0).all() and (never[:2, 5] == 5).all()
    special = np.concatenate([rows[kinds[f"special{r}"]] for r in range(4)])
    nan_bits = np.float64(np.nan).tobytes()
    assert any(row[0].tobytes() == nan_bits and row[2].tobytes() == nan_bits for row in special)  # a NaN return
    assert any(row[2] == -np.inf and row[3] == np.inf and row[0].tobytes() == nan_bits for row in special)  # inf - inf
    assert any(row[0] == np.inf and row[1].tobytes() == nan_bits for row in special)
    zeros = [row for row in special if row[0] == 0 and row[3] == 0]
    assert zeros and all(np.signbit(row[2]) and not np.signbit(row[3]) for row in zeros)  # -0.0 below +0.0
    assert not improved[kinds["special0"]][0]  # (a NaN mean never improves)
    some = rows[kinds["some"]]
    assert set(some[:, 6]) <= {0.0, 1.0} and (some[:, 7] == kinds["some"] + 1).all()


# ---- 3: the tree against math.fsum -------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", (5, 20, 257, 300))
@pytest.mark.parametrize("spread", ("unit", "cancelling"))
def test_mean_and_std_are_within_the_pairwise_bound(E, spread):
    """A pairwise sum of E terms has a relative error of at most ceil(log2 E) u on the sum of the magnitudes (u = 2^-53),
    and the division adds one rounding: |mean - fsum(x) / E| <= (ceil(log2 E) + 1) u sum|x| / E.  The standard deviation is
    held to the same bound on its leaves, the squared differences as the twin rounds them: v = treesum(d d) / E is within
    b = (ceil(log2 E) + 1) u sum(d d) / E of V = fsum(d d) / E, so sqrt(v) is within b / (2 sqrt(V - b)) of sqrt(V) (the
    mean value theorem on the square root) plus the one rounding of the root itself."""
    m = 3
    rng = np.random.default_rng([E, len(spread)])
    x = rng.standard_normal(E)
    if spread == "cancelling":
        x = 1e6 * np.where(np.arange(E) % 2 == 0, 1.0, -1.0) + x
    counts, returns, lengths = evaluation.tables(m, m, E)
    want = evaluation.targets(m, E)
    counts[:] = want
    at = 0
    for i in range(m):
        returns[i, :want[i]] = x[at:at + want[i]]
        lengths[i, :want[i]] = 3
        at += want[i]
    rows, _ = evaluation.finish_numpy(counts, returns, lengths, 1, m, E, 1, np.full(1, -np.inf), np.zeros(1, dtype=np.int64))
    u, depth = 2.0 ** -53, math.ceil(math.log2(E)) + 1
    exact = math.fsum(x) / E
    assert abs(rows[0, 0] - exact) <= depth * u * math.fsum(np.abs(x)) / E
    squares = (x - rows[0, 0]) * (x - rows[0, 0])
    V = math.fsum(squares) / E
    b = depth * u * math.fsum(squares) / E
    assert abs(rows[0, 1] - math.sqrt(V)) <= b / (2.0 * math.sqrt(V - b)) + u * rows[0, 1]
    assert rows[0, 2] == x.min() and rows[0, 3] == x.max() and rows[0, 4] == 3.0 and rows[0, 5] == E


# ---- 4: Evaluation.run against SB3's evaluate_policy, literally -----------------------------------------------------------
def _sb3_loop(env, policy, groups, m, episodes, recurrent):
    """stable_baselines3.common.evaluation.evaluate_policy's loop, restated over this package's twins, with one set of
    episode_count_targets per group (G evaluate_policy calls side by side): per group the lists episode_rewards and
    episode_lengths in SB3's order in time.  Rewards are the raw ones (what Monitor records under VecNormalize)."""
    n = groups * m
    episode_rewards, episode_lengths = [[] for _ in range(groups)], [[] for _ in range(groups)]
    episode_counts = np.zeros(n, dtype="int")
    episode_count_targets = np.tile(np.array([(episodes + i) // m for i in range(m)], dtype="int"), groups)
    current_rewards, current_lengths = np.zeros(n), np.zeros(n, dtype="int")
    observations, _ = env.reset()
    states = np.zeros(policy.spec.state_shape(n), dtype=np.float32) if recurrent else None
    episode_starts = np.ones((n,), dtype=bool)
    while (episode_counts < episode_count_targets).any():
        if recurrent:
            actions = policy.act(observations, episode_starts.astype(np.uint8), None, True, states=(states, states))[0]
        else:
            actions = policy.act(observations, None, True)[0]
        observations, rewards, terminated, truncated, infos = env.step(actions)
        dones = terminated | truncated
        current_rewards += infos.get("raw_reward", rewards)
        current_lengths += 1
        for i in range(n):
            if episode_counts[i] < episode_count_targets[i]:
                episode_starts[i] = dones[i]
                if dones[i]:
                    episode_rewards[i // m].append(current_rewards[i])
                    episode_lengths[i // m].append(current_lengths[i])
                    episode_counts[i] += 1
                    current_rewards[i] = 0
                    current_lengths[i] = 0
            else:  # (SB3 leaves a finished lane's episode_start alone; its actions are never read again)
                episode_starts[i] = dones[i]
    return episode_rewards, episode_lengths


@pytest.mark.parametrize("kind", ("mlp", "lstm"))
def test_run_equals_the_sb3_loop(kind, no_gpu):  # noqa: F811
    G, m, E = 2, 3, 5
    n = G * m
    make = lambda: harness.VectorEnvironment(  # noqa: E731
        **composed.discrete_steps(n, 5, seed=7), episode_records=True, frame_height=16,
        learner_view=harness.LearnerView(frame_stack=2, groups=G, training=False))
    env, other = make(), make()
    try:
        spec = cases.e2e_spec(kind, env)
        if kind == "mlp":
            policy = harness.PopulationPolicy(spec, G, [1, 2])
        else:
            policy = harness.LstmPopulationPolicy(spec, G, [1, 2], num_envs=n)
        policy.init_parameters([5, 6], False)
        want_rewards, want_lengths = _sb3_loop(other, policy, G, m, E, kind == "lstm")
        measured = harness.Evaluation(env, policy, n_eval_episodes=E)
        rows = measured.run(40)
        assert (rows[:, 6] == 0).all() and (rows[:, 5] == E).all()
        u, depth = 2.0 ** -53, math.ceil(math.log2(E)) + 1
        for g in range(G):
            returns, lengths = evaluation.kept_values(measured.counts, measured.returns, measured.lengths, m, E, g)
            assert sorted(zip(returns.tolist(), lengths.tolist())) == sorted(zip(want_rewards[g], want_lengths[g]))
            assert len(set(want_lengths[g])) > 1 or len(set(want_rewards[g])) > 1
            assert abs(rows[g, 0] - math.fsum(want_rewards[g]) / E) <= depth * u * math.fsum(np.abs(want_rewards[g])) / E
            assert rows[g, 4] == np.mean(want_lengths[g])  # (integers: exact in any order)
    finally:
        env.close()
        other.close()


# ---- 5: the classes over the twins --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.E2E_KINDS)
def test_two_runs_keep_the_better_group_wise(kind, no_gpu):  # noqa: F811
    """Evaluation over the four population twins at G = 3, m = 3, E = 5: the statistics are synced from the training
    environment, the better mean is kept per group with its parameters and statistics, load_best restores the selected
    groups only, and the policy's generators, noise and LSTM state are untouched."""
    cases.e2e_promises(cases.e2e_script(kind, False, lambda a: a, np.array))


def test_refusals(no_gpu):  # noqa: F811
    n = 6
    env = lambda **kw: harness.VectorEnvironment(**composed.discrete_steps(n, 5, seed=7), frame_height=16, **kw)  # noqa: E731
    made = [env(episode_records=True), env(), env(episode_records=True, learner_view=harness.LearnerView(groups=3))]
    good, plain, viewed = made
    try:
        spec = cases.e2e_spec("mlp", good)
        policy = harness.PopulationPolicy(spec, 2, [1, 2])
        with pytest.raises(ValueError, match="episode records"):
            harness.Evaluation(plain, policy)
        with pytest.raises(ValueError, match="groups=3"):
            harness.Evaluation(viewed, policy)
        with pytest.raises(ValueError, match="not divisible"):
            harness.Evaluation(good, harness.PopulationPolicy(spec, 4, [1, 2, 3, 4]))
        with pytest.raises(ValueError, match="width"):
            harness.Evaluation(good, harness.PopulationPolicy(harness.MlpPolicySpec(spec.obs_width + 1, 3), 2, [1, 2]))
        with pytest.raises(ValueError, match="actions"):
            harness.Evaluation(good, harness.PopulationPolicy(harness.MlpPolicySpec(spec.obs_width, 2), 2, [1, 2]))
        with pytest.raises(ValueError, match="action space"):
            harness.Evaluation(good, harness.SdePopulationPolicy(harness.SdePolicySpec(spec.obs_width), 2, [1, 2]))
        with pytest.raises(TypeError, match="policy classes"):
            harness.Evaluation(good, object())
        for episodes, words in ((0, "at least 1"), (65537, "RF_EVAL_MAX_EPISODES"), (1.5, "not an integer")):
            with pytest.raises(ValueError, match=words):
                harness.Evaluation(good, policy, n_eval_episodes=episodes)
        measured = harness.Evaluation(good, policy)
        with pytest.raises(ValueError, match="at least 1"):
            measured.run(0)
        with pytest.raises(ValueError, match="deterministic=False"):
            measured.run(3, deterministic=False)
        assert measured.serial == 0
        rows = measured.run(1)  # (no lane can be done after one step: flagged, not waited for)
        assert (rows[:, 6] == evaluation.INCOMPLETE).all() and np.isnan(rows[:, :5]).all() and not measured.improved.any()
        assert (measured.best_mean == -np.inf).all() and measured.serial == 1
    finally:
        for one in made:
            one.close()


def test_the_bindings_name_the_entry_points():
    from reinfocus_amd import _native

    header = open(cases.ROOT + "/include/reinfocus_hip.h").read()
    for name in ("rf_eval_accumulate", "rf_eval_finish", "rf_eval_keep_rows", "rf_env_view_get_statistics_device",
                 "rf_env_view_set_statistics_device"):
        assert name in _native.SYMBOLS and f"int {name}(rf_ctx *ctx" in header
    assert f"#define RF_EVAL_MAX_EPISODES {evaluation.MAX_EPISODES}" in header
    assert f"#define RF_EVAL_INCOMPLETE {evaluation.INCOMPLETE}" in header
