"""CPU tests of the population (include/reinfocus_hip.h, "population"; environments/population.py): the numpy twins
PopulationPolicy / PopulationLearner against G independent existing twins (policy.Policy, learner.Learner) with the same
seeds, hyper-parameters and permutations, bit for bit; the size rules of the grouped entry points and the layout of the
hyper-parameter record, through the host build of the kernels' own header (tests/popcheck); every refusal; the binding.
At 64, 65 and 512 groups, too (the forward), at 64 groups on ppo_tuned.yml's first shape (the update), and the 105
combinations that stand for the 65535 groups of the limit case are pairwise distinct.  The large minibatches (B = 512,
513, 1000, 1024 on m = 8, T = 128) hold what their docstrings promise, and no update in them is skipped."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, learner, policy, population
from tests import helpers
from tests import population_io_cases as cases
from tests import rollout_io_cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture
from tests.test_sharded_env_logic import fake_shards  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits


class _Finished:
    """What train() needs of a finished rollout: flat() and the environment's action space."""

    class env:
        single_action_space = harness.spaces.Discrete(3)

    def __init__(self, flat):
        self._flat = flat

    def flat(self):
        return self._flat


def _members(index, groups, base=100):
    """G stand-alone twins with the population's seeds and parameters."""
    spec = cases.spec_of(index)
    members = [harness.Policy(spec, seed) for seed in cases.seeds_of(groups)]
    for member, state in zip(members, cases.group_states(spec, groups, base)):
        member.load_state_dict(state)
    return members


# ---- 1: the policy twin is G policies over slices ----------------------------------------------------------------------
@pytest.mark.parametrize("per_group", cases.PER_GROUP)
@pytest.mark.parametrize("groups", cases.GROUPS)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)))
def test_population_policy_equals_independent_policies(index, groups, per_group):
    """act() sampled, deterministic, sampled again, then values(), each against G policy.Policy over the groups' rows:
    every output and every generator state after every call."""
    _, twin = cases.twin_policy(index, groups)
    members = _members(index, groups)
    obs, final_obs = cases.forward_inputs(index, groups, per_group)
    pieces = [slice(g * per_group, (g + 1) * per_group) for g in range(groups)]
    for deterministic, with_final in ((False, True), (True, False), (False, False)):
        got = twin.act(obs, final_obs if with_final else None, deterministic)
        want = [member.act(obs[rows], final_obs[rows] if with_final else None, deterministic)
                for member, rows in zip(members, pieces)]
        for i in range(4):
            if want[0][i] is None:
                assert got[i] is None
            else:
                assert bits(got[i]) == bits(np.concatenate([part[i] for part in want])), (deterministic, i)
        assert twin.rng_state() == [member.rng_state() for member in members]
    values, final_values = twin.values(obs, final_obs)
    want = [member.values(obs[rows], final_obs[rows]) for member, rows in zip(members, pieces)]
    assert bits(values) == bits(np.concatenate([part[0] for part in want]))
    assert bits(final_values) == bits(np.concatenate([part[1] for part in want]))
    assert bits(twin.values(obs)) == bits(values)
    assert twin.rng_state() == [member.rng_state() for member in members]
    if groups > 1:  # (the groups' parameters differ, and so do their outputs on the same rows)
        same_rows = np.tile(obs[:per_group], (groups, 1))
        spread = twin.values(same_rows).reshape(groups, per_group)
        assert all(bits(spread[g]) != bits(spread[0]) for g in range(1, groups))


@pytest.mark.parametrize("index,groups,per_group", cases.WIDE_FORWARD)
def test_wide_population_policy_equals_independent_policies(index, groups, per_group):
    """The same at 64, 65 and 512 groups (cases.WIDE_FORWARD): what the GPU test compares rf_policy_forward_grouped with
    at group indices past 4 is G stand-alone policies, each with parameters and a generator of its own."""
    test_population_policy_equals_independent_policies(index, groups, per_group)
    spec, twin = cases.twin_policy(index, groups)
    assert len({bits(row) for row in twin.params}) == groups and len(set(cases.seeds_of(groups))) == groups
    final_values = cases.wanted_forward(index, groups, per_group, 0, True)[0][3]
    assert np.isnan(final_values).any() and not np.isnan(final_values).all()


def test_rng_state_round_trip_and_state_dicts():
    spec, twin = cases.twin_policy(0, 5)
    obs, _ = cases.forward_inputs(0, 5, 3)
    kept = twin.rng_state()
    first = twin.act(obs)
    twin.set_rng_state(kept)
    again = twin.act(obs)
    assert bits(first[0]) == bits(again[0]) and bits(first[2]) == bits(again[2])
    state = twin.state_dict(group=3)
    assert bits(spec.pack(state)) == bits(twin.params[3]) and bits(twin.params[3]) != bits(twin.params[0])
    twin.load_state_dict(state)  # (every group)
    assert all(bits(twin.params[g]) == bits(twin.params[3]) for g in range(5))
    assert all(member.params.base is twin.params for member in twin.policies)  # (the members still see the one array)
    with pytest.raises(IndexError):
        twin.state_dict(group=5)


# ---- 2: the learner twin is G learners over slices ----------------------------------------------------------------------
@pytest.mark.parametrize("batch,per_group", cases.UPDATE_SHAPES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)))
def test_population_learner_equals_independent_learners(index, batch, per_group):
    """Chained updates over two epochs (the last minibatch of each is short), hyper-parameters that differ per group,
    against G learner.Learner over the groups' rows; learning_rate 0 keeps a group's parameters and moves its moments."""
    groups = cases.UPDATE_GROUPS
    got = cases.twin_updates(index, batch, per_group)
    spec, twin, flat = cases.update_batch(index, groups, per_group)
    before = twin.params.copy()
    hypers = harness.PopulationLearner(twin, **cases.group_hypers(groups)).hypers()
    rows = per_group * cases.T
    members = []
    for g, member in enumerate(_members(index, groups, base=300)):
        h = hypers[g]
        members.append(harness.Learner(member, learning_rate=h.learning_rate, clip_range=h.clip_range, ent_coef=h.ent_coef,
                                       vf_coef=h.vf_coef, max_grad_norm=h.max_grad_norm,
                                       normalize_advantage=bool(h.normalize_advantage), betas=(h.beta1, h.beta2),
                                       adam_eps=h.adam_eps))
    order = cases.minibatches(cases.update_permutations(groups, rows, 7 + batch), batch)
    assert len(order) >= 3 and order[-1].shape[1] < batch
    for update, index_rows in enumerate(order):
        for g, member in enumerate(members):
            piece = {key: flat[key][g * rows:(g + 1) * rows] for key in learner.BATCH_KEYS}
            stats = member.update(piece, index_rows[g])
            assert bits(got[update][2][g]) == bits(stats), f"update {update}, group {g}: stats differ"
            assert bits(got[update][0][g]) == bits(member.policy.params), f"update {update}, group {g}: params differ"
            assert bits(got[update][1][g]) == bits(member.state), f"update {update}, group {g}: state differs"
    params, states, stats = got[-1]
    assert (stats[:, 7] == 0).all() and len({bits(row) for row in stats[:, :7]}) == groups
    assert bits(params[1]) == bits(before[1]) and bits(params[0]) != bits(before[0]) and bits(params[2]) != bits(before[2])
    assert np.abs(states[1][learner.STATE_HEADER:]).max() > 0


def test_wide_population_learner_equals_independent_learners():
    """cases.WIDE_UPDATE -- 64 groups on ppo_tuned.yml's first shape (m = 8, T = 32, B = 64), two epochs of four chained
    updates, hyper-parameters that differ between neighbours (cases.wide_hypers) -- against learner.Learner per group, for
    groups 0, 1, 30 .. 32 and 63; group 31 is flagged RF_PPO_NONFINITE in the one update of each epoch that holds its NaN
    row and keeps its bytes there, group 1 has learning_rate 0."""
    w = cases.WIDE_UPDATE
    want = cases.wide_twin_updates()
    spec, twin, flat, hypers, order = cases.wide_update_inputs()
    cases.wide_update_promises(want, twin.params)
    rows = w["per_group"] * w["steps"]
    hyper_list = harness.PopulationLearner(twin, **hypers).hypers()
    for g, (one, other) in enumerate(zip(hyper_list, hyper_list[1:])):
        assert all(x != y for x, y in zip(one, other)), f"groups {g} and {g + 1} share a hyper-parameter"
    assert [h.learning_rate == 0 for h in hyper_list] == [g == 1 for g in range(w["groups"])]
    members = _members(w["index"], w["groups"], base=300)
    for g in (0, 1, 30, 31, 32, 63):
        h = hyper_list[g]
        member = harness.Learner(members[g], learning_rate=h.learning_rate, clip_range=h.clip_range, ent_coef=h.ent_coef,
                                 vf_coef=h.vf_coef, max_grad_norm=h.max_grad_norm,
                                 normalize_advantage=bool(h.normalize_advantage), betas=(h.beta1, h.beta2), adam_eps=h.adam_eps)
        piece = {key: flat[key][g * rows:(g + 1) * rows] for key in learner.BATCH_KEYS}
        for update, index_rows in enumerate(order):
            stats = member.update(piece, index_rows[g])
            assert bits(want[update][2][g]) == bits(stats), f"update {update}, group {g}: stats differ"
            assert bits(want[update][0][g]) == bits(member.policy.params), f"update {update}, group {g}: params differ"
            assert bits(want[update][1][g]) == bits(member.state), f"update {update}, group {g}: state differs"


def _alone(member, h):
    return harness.Learner(member, learning_rate=h.learning_rate, clip_range=h.clip_range, ent_coef=h.ent_coef,
                           vf_coef=h.vf_coef, max_grad_norm=h.max_grad_norm, normalize_advantage=bool(h.normalize_advantage),
                           betas=(h.beta1, h.beta2), adam_eps=h.adam_eps)


def large_case_holds(module, members, index, groups, batch, sizes=None):
    """What a case of LARGE_CASES (this population's or the gSDE one's) promises, and that its twin population is G
    stand-alone learners over contiguous copies of the groups' slices.  sizes: the host build's (grouped state size,
    grouped workspace size, ungrouped state size, ungrouped workspace size), where there is one."""
    large = module.LARGE
    rows = large["per_group"] * large["steps"]
    assert (rows, large["updates"]) == (1024, 2) and batch <= rows
    spec, twin, flat, keywords, order = module.large_inputs(index, groups, batch)
    before = twin.params.copy()
    want = module.large_twin_updates(index, groups, batch)
    module.large_update_promises(want, before, keywords)
    assert len({bits(row) for row in before}) == groups, "two groups share their parameters"
    hypers = harness.PopulationLearner(twin, **keywords).hypers()
    for g, (one, other) in enumerate(zip(hypers, hypers[1:])):
        assert all(x != y for x, y in zip(one, other)), f"groups {g} and {g + 1} share a hyper-parameter"
    assert len(order) == 2 and bits(order[0]) != bits(order[1])
    for index_rows in order:
        assert index_rows.shape == (groups, batch) and index_rows.dtype == np.int64
        assert index_rows.min() >= 0 and index_rows.max() < rows
        assert len({bits(row) for row in index_rows}) == groups, "two groups share their index row"
        for row in index_rows:  # (a permutation of the group's rows at B = N, drawn with repeats below)
            assert (len(np.unique(row)) == batch) == (batch == rows)
    alone = [_alone(member, h) for member, h in zip(members, hypers)]
    for update, index_rows in enumerate(order):
        for g, member in enumerate(alone):
            piece = {key: np.ascontiguousarray(flat[key][g * rows:(g + 1) * rows]) for key in learner.BATCH_KEYS}
            stats = member.update(piece, index_rows[g].copy())
            assert bits(want[update][2][g]) == bits(stats), f"update {update}, group {g}: stats differ"
            assert bits(want[update][0][g]) == bits(member.policy.params), f"update {update}, group {g}: params differ"
            assert bits(want[update][1][g]) == bits(member.state), f"update {update}, group {g}: state differs"
    if sizes is None:
        return
    grouped_state, grouped_workspace, one_state, one_workspace = sizes
    desc = ctypes.byref(_native.PolicyDesc(*spec.desc()))
    assert grouped_state(desc, groups, large["per_group"]) == groups * one_state(desc) > 0
    assert grouped_workspace(desc, groups, large["per_group"], large["steps"], batch) == groups * one_workspace(desc, batch) > 0


@pytest.mark.parametrize("index,groups,batch", cases.LARGE_CASES)
def test_large_minibatches_hold_what_they_promise(index, groups, batch, popcheck, ppocheck):
    """cases.LARGE_CASES -- m = 8, T = 128, B = 512, 513, 1000 and 1024 at G = 3 on the network whose widths are no
    multiple of a wave, 513 at G = 2 on stable-baselines3's default -- without a GPU: the index is [G][B] with a row of
    its own per group (a permutation at B = N, repeats below), parameters differ per group and every hyper-parameter
    between neighbours, the twin population equals G learner.Learner over contiguous slice copies byte for byte over
    both updates, no group is skipped, every group with a learning rate ends with other parameters, and the header's
    workspace size is G times the ungrouped one."""
    assert cases.LARGE_ALONE in cases.LARGE_CASES
    large_case_holds(cases, _members(index, groups, base=300), index, groups, batch,
                     (popcheck.pop_state_size, popcheck.pop_workspace_size, ppocheck.ppc_state_size,
                      ppocheck.ppc_workspace_size))


def test_the_105_combinations_of_the_group_limit_are_distinct(popcheck, ppocheck):
    """cases.limit_results: the 35 (parameter set, observation block) pairs give 35 different values, log-probabilities
    and final values; the 105 combinations give 105 different updated parameters, optimizer states and stats, all taken.
    limit_arrays hands group g combination g % 105, so neighbouring groups differ in parameters, observations and
    hyper-parameters.  The size functions of the header take 65535 groups of that shape and refuse 65536."""
    forwards, updates = cases.limit_results()
    for i, name in enumerate(cases.ORDER):
        assert name == "actions" or len({bits(forward[i]) for forward in forwards}) == 35, name
    assert np.isfinite(np.concatenate([np.concatenate(forward[1:]) for forward in forwards])).all()
    for i, name in enumerate(("params", "state", "stats")):
        assert len({bits(update[i]) for update in updates}) == 105, name
    assert all(update[2][7] == 0 for update in updates)
    params, blocks, hypers = cases.limit_parts()
    assert all(bits(update[0]) != bits(params[c % 7]) for c, update in enumerate(updates))
    inputs, wanted_forward, wanted_update = cases.limit_arrays()
    assert inputs["params"].shape == (65535, 10) and wanted_update[1].shape == (65535, learner.STATE_HEADER + 20)
    for key in ("params", "observations", "hyper"):
        rows = inputs[key].reshape(65535, -1)
        assert all(rows[g].tobytes() != rows[g + 1].tobytes() for g in range(0, 65534, 257)), key
    assert bits(wanted_update[0][65534]) == bits(updates[65534 % 105][0]) and 65534 % 105 == 14
    assert bits(wanted_forward[1][247:248]) == bits(forwards[37][1]) and 247 % 105 == 37
    desc = ctypes.byref(_native.PolicyDesc(*cases.limit_spec().desc()))
    assert popcheck.pop_state_size(desc, 65535, 1) == 65535 * ppocheck.ppc_state_size(desc) > 0
    assert popcheck.pop_workspace_size(desc, 65535, 1, 1, 1) == 65535 * ppocheck.ppc_workspace_size(desc, 1) > 0
    assert popcheck.pop_state_size(desc, 65536, 1) == 0 and popcheck.pop_workspace_size(desc, 65536, 1, 1, 1) == 0


def test_population_train_equals_independent_trains():
    """train() with given permutations and with a generator, against learner.Learner.train per group; state_dict()
    resumes every group bit for bit."""
    index, groups, per_group = 0, 3, 3
    rows = per_group * cases.T
    spec, twin, flat = cases.update_batch(index, groups, per_group)
    kw = dict(learning_rate=[1e-2, 3e-3, 0.0], ent_coef=[0.0, 0.01, 0.02])
    many = harness.PopulationLearner(twin, **kw)
    permutations = cases.update_permutations(groups, rows, 21)
    got = many.train(_Finished(flat), cases.EPOCHS, 5, permutations=permutations)
    assert got.shape == (cases.EPOCHS * 3, groups, 8)
    members = _members(index, groups, base=300)
    for g, member in enumerate(members):
        piece = {key: flat[key][g * rows:(g + 1) * rows] for key in flat}
        one = harness.Learner(member, learning_rate=kw["learning_rate"][g], ent_coef=kw["ent_coef"][g])
        want = one.train(_Finished(piece), cases.EPOCHS, 5, permutations=permutations[:, g])
        assert bits(got[:, g]) == bits(want) and bits(twin.params[g]) == bits(member.params)
        assert bits(many.learners[g].state) == bits(one.state)
    # a generator: per epoch one permutation per group, in group order
    kept, kept_params = many.state_dict(), twin.params.copy()
    assert kept["step"] == [6, 6, 6] and kept["m"].shape == (groups, spec.size)
    straight = many.train(_Finished(flat), 1, 5, generator=np.random.default_rng(4))
    rng = np.random.default_rng(4)
    drawn = np.stack([rng.permutation(rows) for _ in range(groups)])[None]
    after = twin.params.copy(), cases.twin_states(many)
    twin.params[:] = kept_params
    second = harness.PopulationLearner(twin, **kw)
    second.load_state_dict(kept)
    assert bits(second.train(_Finished(flat), 1, 5, permutations=drawn)) == bits(straight)
    assert bits(twin.params) == bits(after[0]) and bits(cases.twin_states(second)) == bits(after[1])


def test_isolation_of_the_twin():
    """The inputs of the GPU isolation test do what they promise: exactly groups 1 and 2 are flagged and skipped."""
    spec, twin, flat, order = cases.isolation_inputs()
    before = twin.params.copy()
    stats = harness.PopulationLearner(twin, learning_rate=1e-2).update(flat, order)
    assert list(stats[:, 7]) == [0, learner.INVALID, learner.NONFINITE, 0]
    assert bits(twin.params[1]) == bits(before[1]) and bits(twin.params[2]) == bits(before[2])
    assert bits(twin.params[0]) != bits(before[0]) and bits(twin.params[3]) != bits(before[3])


def test_collect_takes_a_population_policy(no_gpu):  # noqa: F811
    """Rollout.collect(PopulationPolicy) equals the explicit loop over G policies on the groups' environments."""
    spec = cases.e2e_spec()
    runs = []
    for grouped in (True, False):
        env = harness.VectorDiscreteSteps(num_envs=6, episode_records=True, **rollout_io_cases.ENV_KW)
        try:
            rollout = harness.Rollout(env, 3)
            rollout.start(env.reset()[0])
            actor = harness.PopulationPolicy(spec, 3, [5, 6, 7])
            for g, state in enumerate(cases.group_states(spec, 3, 500)):
                actor.load_state_dict(state, group=g)
            if grouped:
                rollout.collect(actor)
            else:
                final_obs = None
                for t in range(3):
                    parts = [member.act(rollout.observations[t][2 * g:2 * g + 2],
                                        None if final_obs is None else final_obs[2 * g:2 * g + 2])
                             for g, member in enumerate(actor.policies)]
                    actions, values, log_probs = (np.concatenate([part[i] for part in parts]) for i in range(3))
                    if final_obs is not None:
                        rollout.bootstrap(np.concatenate([part[3] for part in parts]))
                    final_obs = rollout.step(actions, values, log_probs)[4]["final_observation"]
                parts = [member.values(rollout.observations[3][2 * g:2 * g + 2], final_obs[2 * g:2 * g + 2])
                         for g, member in enumerate(actor.policies)]
                rollout.bootstrap(np.concatenate([part[1] for part in parts]))
                rollout.finish(np.concatenate([part[0] for part in parts]))
            runs.append({key: value.copy() for key, value in rollout.flat().items()})
        finally:
            env.close()
    for key in runs[0]:
        assert bits(runs[0][key]) == bits(runs[1][key]), key


# ---- 3: the size rules and the record, through the header ----------------------------------------------------------------
@pytest.fixture(scope="module")
def popcheck():
    lib = ctypes.CDLL(helpers.built("tests/popcheck", "libpopcheck.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.pop_state_size.restype = lib.pop_workspace_size.restype = ctypes.c_ulonglong
    lib.pop_state_size.argtypes = [vp, i32, i32]
    lib.pop_workspace_size.argtypes = [vp, i32, i32, i32, i32]
    lib.pop_hyper_layout.argtypes = [vp]
    lib.pop_hyper.argtypes = [vp, vp]
    return lib


@pytest.fixture(scope="module")
def ppocheck():
    lib = ctypes.CDLL(helpers.built("tests/ppocheck", "libppocheck.so"))
    lib.ppc_state_size.restype = lib.ppc_workspace_size.restype = ctypes.c_ulonglong
    lib.ppc_state_size.argtypes = [ctypes.c_void_p]
    lib.ppc_workspace_size.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return lib


@pytest.mark.parametrize("index", range(len(cases.NETWORKS)))
def test_sizes_are_g_times_the_ungrouped_sizes(index, popcheck, ppocheck):
    spec = cases.spec_of(index)
    desc = ctypes.byref(_native.PolicyDesc(*spec.desc()))
    one_state = ppocheck.ppc_state_size(desc)
    assert one_state == 32 + 8 * spec.size  # (the header's words)
    for groups, per_group, steps, batch in ((1, 1, 1, 1), (1, 8, 32, 64), (5, 3, 4, 12), (512, 8, 32, 64), (65535, 1, 2, 2)):
        assert popcheck.pop_state_size(desc, groups, per_group) == groups * one_state
        assert popcheck.pop_workspace_size(desc, groups, per_group, steps, batch) \
            == groups * ppocheck.ppc_workspace_size(desc, batch) > 0
    assert popcheck.pop_state_size(desc, 0, 8) == 0 and popcheck.pop_state_size(desc, 4, 0) == 0
    assert popcheck.pop_state_size(desc, 65536, 1) == 0 and popcheck.pop_state_size(desc, -1, 8) == 0
    for refused in ((0, 8, 4, 8), (4, 0, 4, 8), (4, 8, 0, 8), (4, 3, 4, 13), (4, 8, 4, 0), (4, 1024, 4, 1025),
                    (65536, 8, 4, 8), (2, 2 ** 15, 2 ** 15, 8)):
        assert popcheck.pop_workspace_size(desc, *refused) == 0, refused
    assert popcheck.pop_workspace_size(desc, 4, 3, 4, 12) > 0  # (B == m T is the most)
    bad = list(spec.desc())
    bad[0] = 0
    assert popcheck.pop_state_size(ctypes.byref(_native.PolicyDesc(*bad)), 4, 8) == 0


def test_hyper_record_is_the_kernels_struct(popcheck):
    layout = (ctypes.c_int * 10)()
    popcheck.pop_hyper_layout(layout)
    record = population.HYPER_RECORD
    assert [record.fields[name][1] for name in record.names] == list(layout[:9]) and record.itemsize == layout[9] == 56
    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    struct = re.search(r"typedef struct rf_ppo_hyper \{(.*?)\} rf_ppo_hyper;", text, flags=re.S).group(1)
    names = [name.strip() for _, group in re.findall(r"(double|float|int) ([\w, ]+);", re.sub(r"/\*.*?\*/", "", struct))
             for name in group.split(",")]
    assert names == list(record.names)
    twin = harness.PopulationPolicy(cases.spec_of(0), 3, [1, 2, 3])
    hypers = harness.PopulationLearner(twin, **cases.group_hypers(3)).hypers()
    packed = population.hyper_records(hypers)
    for g, hyper in enumerate(hypers):
        out = np.zeros(1, dtype=record)
        assert popcheck.pop_hyper(ctypes.byref(_native.PpoDesc(*hyper)), out.ctypes.data) == 0
        assert out.tobytes() == packed[g:g + 1].tobytes()
    assert len({packed[g:g + 1].tobytes() for g in range(3)}) == 3


def test_binding_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read(), flags=re.S)
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    kinds = {"vp": ctypes.c_void_p, "i32": ctypes.c_int, "ctypes.c_ulonglong": ctypes.c_ulonglong}
    for entry, count in (("rf_policy_forward_grouped", 16), ("rf_ppo_grouped_state_size", 4),
                         ("rf_ppo_grouped_workspace_size", 6), ("rf_ppo_update_grouped", 18)):
        declaration = re.search(r"\b%s\s*\((.*?)\)\s*;" % entry, text, flags=re.S).group(1)
        wanted = [ctypes.c_void_p if "*" in p else (ctypes.c_ulonglong if "unsigned long long" in p else ctypes.c_int)
                  for p in declaration.split(",")]
        names = re.search(r"lib\.%s\.argtypes = \[(.*?)\]" % entry, source, flags=re.S).group(1).split(",")
        assert [kinds[name.strip()] for name in names] == wanted and len(wanted) == count
        assert entry in _native.SYMBOLS
    assert int(re.search(r"#define RF_POPULATION_MAX_GROUPS (\d+)", text).group(1)) == population.MAX_GROUPS


# ---- 4: refusals --------------------------------------------------------------------------------------------------------
def test_refusals(no_gpu):  # noqa: F811
    spec = cases.spec_of(0)
    with pytest.raises(ValueError, match="one seed per group"):
        harness.PopulationPolicy(spec, 3, [1, 2])
    with pytest.raises(ValueError, match="one seed per group"):
        harness.PopulationPolicy(spec, 3, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="one seed per group"):
        harness.PopulationPolicy(spec, 3, 5)
    with pytest.raises(ValueError, match="groups"):
        harness.PopulationPolicy(spec, 0, [])
    with pytest.raises(ValueError, match="out of scope"):
        harness.PopulationPolicy(harness.SdePolicySpec(3, pi=(5,), vf=(4,)), 2, [1, 2])
    twin = harness.PopulationPolicy(spec, 3, [1, 2, 3])
    before = twin.rng_state()
    with pytest.raises(ValueError, match="not divisible"):
        twin.act(np.zeros((7, 3), dtype=F32))
    with pytest.raises(ValueError, match="not divisible"):
        twin.values(np.zeros((2, 3), dtype=F32))
    assert twin.rng_state() == before
    with pytest.raises(ValueError, match="generator states"):
        twin.set_rng_state(before[:2])
    with pytest.raises(TypeError, match="PopulationPolicy"):
        harness.PopulationLearner(harness.Policy(spec, 0))
    with pytest.raises(TypeError, match="DevicePopulationPolicy"):
        harness.DevicePopulationLearner(twin)
    with pytest.raises(TypeError, match="Policy"):
        harness.Learner(twin)
    with pytest.raises(ValueError, match="entries"):
        harness.PopulationLearner(twin, learning_rate=[1e-3, 1e-3])
    with pytest.raises(ValueError, match="betas"):
        harness.PopulationLearner(twin, betas=[(0.9, 0.999)] * 2)
    with pytest.raises(ValueError, match="betas"):
        harness.PopulationLearner(twin, betas=[(0.9, 0.999), (0.9, 1.0), (0.9, 0.999)])
    with pytest.raises(ValueError, match="hyper-parameter"):
        harness.PopulationLearner(twin, ent_coef=[0.0, float("nan"), 0.0])
    many = harness.PopulationLearner(twin)
    _, _, flat = cases.update_batch(0, 3, 3)
    with pytest.raises(ValueError, match="more than the 12 rows"):
        many.train(_Finished(flat), 1, 13)
    with pytest.raises(ValueError, match="more than the 12 rows"):
        many.update(flat, np.zeros((3, 13), dtype=np.int64))
    with pytest.raises(ValueError, match="index has shape"):
        many.update(flat, np.zeros((2, 5), dtype=np.int64))
    with pytest.raises(ValueError):
        many.train(_Finished(flat), 0, 4)
    box = _Finished(flat)
    box.env = type("env", (), {"single_action_space": harness.spaces.Box(-1.0, 1.0, (1,))})
    with pytest.raises(ValueError, match="out of scope"):
        many.train(box, 1, 4)
    # the device classes refuse what is no device-resident environment before anything of the GPU is touched
    host = harness.VectorDiscreteSteps(num_envs=6, **rollout_io_cases.ENV_KW)
    try:
        with pytest.raises(TypeError, match="device-resident"):
            harness.DevicePopulationPolicy(host, cases.e2e_spec(), 3, [1, 2, 3])
    finally:
        host.close()


def test_sharded_environments_are_refused(fake_shards):  # noqa: F811
    env = harness.ShardedVectorDiscreteSteps(num_envs=6, devices=[0, 1], frame_height=16, samples_per_pixel=1, seed=1)
    try:
        with pytest.raises(ValueError, match="tensor lives on one GPU"):
            harness.DevicePopulationPolicy(env, cases.e2e_spec(), 3, [1, 2, 3])
    finally:
        env.close()


def test_import_stays_free_of_torch():
    code = ("import sys; from reinfocus_amd.environments import harness; harness.PopulationPolicy; "
            "harness.DevicePopulationLearner; assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
