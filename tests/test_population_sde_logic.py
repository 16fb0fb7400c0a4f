"""CPU tests of the population of gSDE learners (include/reinfocus_hip.h, "population sde"): the numpy twins
harness.SdePopulationPolicy / PopulationLearner over it are literally G of the existing twins (sde.SdePolicy,
learner.Learner) over slices, Rollout.collect resets each group's noise by its own sde_sample_freq, and the surface
refuses what it cannot express.  The arithmetic of one group is held to the host build of the kernels' functions by
tests/test_sde_logic.py (tests/sdecheck); nothing here needs a GPU.  tests/test_gpu_population_sde.py holds the device
classes and the grouped entry points to these twins as bytes."""

import os
import re

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, learner, policy, sde
from tests import population_sde_io_cases as cases
from tests import rollout_io_cases as rollout_cases
from tests import sde_io_cases as sde_cases
from tests import test_population_logic as population_logic
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits


def _members(index, groups, base=100):
    """G stand-alone SdePolicy twins with the population's seeds and state dicts."""
    spec = cases.spec_of(index)
    members = []
    for g, seed in enumerate(cases.seeds_of(groups)):
        member = harness.SdePolicy(spec, seed)
        member.load_state_dict(sde_cases.state_dict(spec, base + 17 * g))
        members.append(member)
    return spec, members


def _same_on_slices(population, members, per_group, obs, final_obs):
    groups = len(members)
    for deterministic in (False, True):
        got = population.act(obs, final_obs, deterministic)
        assert len(got) == 5
        for g, member in enumerate(members):
            rows = slice(g * per_group, (g + 1) * per_group)
            want = member.act(obs[rows], final_obs[rows], deterministic)
            for i in range(5):
                assert bits(got[i][rows]) == bits(want[i]), (deterministic, g, i)
    values, finals = population.values(obs, final_obs)
    noise = population.noise()
    for g, member in enumerate(members):
        rows = slice(g * per_group, (g + 1) * per_group)
        want = member.values(obs[rows], final_obs[rows])
        assert bits(values[rows]) == bits(want[0]) and bits(finals[rows]) == bits(want[1])
        assert bits(noise[rows]) == bits(member.noise())
    assert population.rng_state() == [member.rng_state() for member in members]
    assert bits(population.values(obs)) == bits(values) and groups == population.groups


@pytest.mark.parametrize("per_group", cases.PER_GROUP)
@pytest.mark.parametrize("groups", cases.GROUPS)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)))
def test_population_policy_equals_independent_policies(index, groups, per_group):
    """act (sampled and deterministic), values, noise and rng_state on slices, after sequences of reset_noise(groups=mask)
    in which the groups reset different numbers of times; an unselected group keeps its theta and its generator."""
    spec, population = cases.twin_policy(index, groups)
    _, members = _members(index, groups)
    for g, member in enumerate(members):
        assert bits(population.params[g]) == bits(member.params)
        assert np.shares_memory(population.policies[g].params, population.params[g])
    obs, final_obs = cases.forward_inputs(index, groups, per_group)
    n = groups * per_group
    assert population.noise() is None
    with pytest.raises(ValueError, match="reset_noise"):
        population.act(obs)
    population.reset_noise(num_envs=n)
    for member in members:
        member.reset_noise(per_group)
    _same_on_slices(population, members, per_group, obs, final_obs)
    rng = np.random.default_rng(groups + per_group)
    resets = np.ones(groups, dtype=int)
    for mask in [np.arange(groups) % 2 == 0, np.arange(groups) == groups - 1, rng.random(groups) < 0.5,
                 np.zeros(groups, dtype=bool), list(np.arange(groups) % 3 != 1)]:
        before, states = population.noise(), population.rng_state()
        population.reset_noise(groups=mask)
        for g, member in enumerate(members):
            rows = slice(g * per_group, (g + 1) * per_group)
            if mask[g]:
                member.reset_noise(per_group)
                resets[g] += 1
                assert bits(population.noise()[rows]) != bits(before[rows])
            else:
                assert bits(population.noise()[rows]) == bits(before[rows]) and population.rng_state()[g] == states[g]
        _same_on_slices(population, members, per_group, obs, final_obs)
    for g, seed in enumerate(cases.seeds_of(groups)):
        moved = np.random.PCG64DXSM(seed).advance(int(resets[g]) * per_group * spec.latent)
        assert population.rng_state()[g] == moved.state
    assert groups == 1 or len(set(resets)) > 1


def test_log_std_init_and_state_round_trip():
    spec = cases.spec_of(0)
    assert bits(harness.SdePopulationPolicy(spec, 2, [1, 2]).params[1]) == bits(spec.initial())
    population = harness.SdePopulationPolicy(spec, 3, [1, 2, 3], log_std_init=[-4.0, 0.5, 1.0])
    for g, value in enumerate((-4.0, 0.5, 1.0)):
        assert (population.params[g, spec.log_std_at:] == F32(value)).all() and (population.params[g, :spec.log_std_at] == 0).all()
    assert (harness.SdePopulationPolicy(spec, 2, [1, 2], log_std_init=-2.0).params[:, spec.log_std_at:] == F32(-2.0)).all()
    state = sde_cases.state_dict(spec, 9)
    population.load_state_dict(state, group=1)
    assert bits(population.params[1]) == bits(spec.pack(state)) and (population.params[0, :spec.log_std_at] == 0).all()
    for name, value in population.state_dict(group=1).items():
        assert bits(value) == bits(state[name]), name
    population.reset_noise(num_envs=6)
    kept = population.rng_state(), population.noise()
    other = harness.SdePopulationPolicy(spec, 3, [7, 8, 9])
    for g in range(3):
        other.load_state_dict(population.state_dict(group=g), group=g)
    other.set_rng_state(kept[0])
    other.set_noise(kept[1])
    obs = cases.forward_inputs(0, 3, 2)[0]
    assert bits(other.act(obs)[0]) == bits(population.act(obs)[0])
    other.reset_noise(groups=[False, True, True], num_envs=6)
    population.reset_noise(groups=[False, True, True])
    assert bits(other.noise()) == bits(population.noise()) and other.rng_state() == population.rng_state()


@pytest.mark.parametrize("batch,per_group", cases.UPDATE_SHAPES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)))
def test_population_learner_equals_independent_learners(index, batch, per_group):
    """Per-group hyper-parameters and log_std all different: parameters, optimizer states and stats as bytes over two
    epochs of chained updates against G stand-alone Learner objects over SdePolicy members."""
    want = cases.twin_updates(index, batch, per_group)
    spec, twin, flat = cases.update_batch(index, cases.UPDATE_GROUPS, per_group)
    log_stds = [bits(twin.params[g, spec.log_std_at:]) for g in range(cases.UPDATE_GROUPS)]
    assert len(set(log_stds)) == cases.UPDATE_GROUPS
    _, members = _members(index, cases.UPDATE_GROUPS, base=300)
    hypers = harness.PopulationLearner(twin, **cases.group_hypers(cases.UPDATE_GROUPS)).hypers()
    assert len({tuple(h) for h in hypers}) == cases.UPDATE_GROUPS
    alone = []
    for member, hyper in zip(members, hypers):
        alone.append(harness.Learner(member, hyper.learning_rate, hyper.clip_range, hyper.ent_coef, hyper.vf_coef,
                                     hyper.max_grad_norm, bool(hyper.normalize_advantage), (hyper.beta1, hyper.beta2),
                                     hyper.adam_eps))
    rows = per_group * cases.T
    order = cases.minibatches(cases.update_permutations(cases.UPDATE_GROUPS, rows, 7 + batch), batch)
    for update, index_rows in enumerate(order):
        for g, member in enumerate(alone):
            piece = {key: flat[key][g * rows:(g + 1) * rows] for key in learner.BATCH_KEYS}
            stats = member.update(piece, index_rows[g])
            assert bits(stats) == bits(want[update][2][g]), (update, g)
            assert bits(member.policy.params) == bits(want[update][0][g]), (update, g)
            assert bits(member.state) == bits(want[update][1][g]), (update, g)
    assert bits(want[-1][0][0, spec.log_std_at:]) != log_stds[0]  # (log_std is trained)


@pytest.mark.parametrize("index,groups,batch", cases.LARGE_CASES)
def test_large_minibatches_hold_what_they_promise(index, groups, batch):
    """cases.LARGE_CASES -- m = 8, T = 128, B = 512, 513, 1000 and 1024 at G = 3 on NETWORKS[1], 513 at G = 2 on the widest
    network of tests/sde_io_cases.py -- without a GPU, by tests/test_population_logic.py's checks: the index is [G][B] with
    a row of its own per group (a permutation at B = N, repeats below), parameters (log_std included) differ per group
    and every hyper-parameter between neighbours, the twin population equals G learner.Learner over SdePolicy members on
    contiguous slice copies byte for byte over both updates, no group is skipped, and every group with a learning rate
    ends with other parameters."""
    assert cases.LARGE_ALONE in cases.LARGE_CASES
    spec, members = _members(index, groups, base=300)
    assert len({bits(member.params[spec.log_std_at:]) for member in members}) == groups
    population_logic.large_case_holds(cases, members, index, groups, batch)


def test_learner_state_dict_resumes_bit_for_bit():
    spec, twin, flat = cases.update_batch(0, cases.UPDATE_GROUPS, 3)
    order = cases.minibatches(cases.update_permutations(cases.UPDATE_GROUPS, 3 * cases.T, 4), 5)
    first = harness.PopulationLearner(twin, **cases.group_hypers(cases.UPDATE_GROUPS))
    first.update(flat, order[0])
    kept, kept_params = first.state_dict(), twin.params.copy()
    straight = first.update(flat, order[1])
    after = twin.params.copy()
    resumed = harness.SdePopulationPolicy(spec, cases.UPDATE_GROUPS, [0] * cases.UPDATE_GROUPS)
    for g in range(cases.UPDATE_GROUPS):
        resumed.load_state_dict(spec.unpack(kept_params[g]), group=g)
    second = harness.PopulationLearner(resumed, **cases.group_hypers(cases.UPDATE_GROUPS))
    second.load_state_dict(kept)
    assert bits(second.update(flat, order[1])) == bits(straight) and bits(resumed.params) == bits(after)
    assert bits(cases.twin_states(second)) == bits(cases.twin_states(first))


def test_collect_resets_each_group_by_its_own_frequency(no_gpu):  # noqa: F811
    """Rollout.collect(sde_sample_freq=[-1, 1, 3]) on a 3-group environment equals the explicit loop of
    reset_noise(groups=...) / act / step / finish; the groups' generators have given 1, 1 + T and 1 + ceil(T / 3) resets of
    m L draws; a call with no group due is not made."""
    freqs, groups, m = [-1, 1, 3], 3, 2
    steps = rollout_cases.T
    runs = {}
    calls = []
    for how in ("collect", "explicit"):
        env = harness.VectorContinuousJumps(num_envs=groups * m, **rollout_cases.ENV_KW)
        try:
            spec = sde_cases.e2e_spec(env)
            twin = harness.SdePopulationPolicy(spec, groups, cases.seeds_of(groups), log_std_init=[-0.5, 0.0, 0.5])
            for g in range(groups):
                state = sde_cases.state_dict(spec, 40 + g)
                state["log_std"][:] = twin.params[g, spec.log_std_at]
                twin.load_state_dict(state, group=g)
            buffer = harness.Rollout(env, steps, [0.99, 0.9, 0.95], [0.92, 0.95, 0.8], groups=groups)
            buffer.start(env.reset(seed=rollout_cases.ENV_KW["seed"])[0])
            if how == "collect":
                inner = twin.reset_noise
                twin.reset_noise = lambda groups=None, num_envs=None: (calls.append(groups), inner(groups, num_envs))[1]
                buffer.collect(twin, sde_sample_freq=freqs)
            else:
                twin.reset_noise(num_envs=groups * m)
                for t in range(steps):
                    twin.reset_noise(groups=[False, True, t % 3 == 0])
                    actions, values, log_probs, _, clamped = twin.act(buffer.observations[t])
                    assert bits(clamped) == bits(np.clip(actions, -1, 1))
                    buffer.step(actions, values, log_probs, clamped)
                buffer.finish(twin.values(buffer.observations[steps]))
            runs[how] = sde_cases.policy_cases.slabs_of(buffer, np.array), twin.rng_state(), twin.noise()
        finally:
            env.close()
    sde_cases.same_runs([runs["collect"][0]], [runs["explicit"][0]])
    assert runs["collect"][1] == runs["explicit"][1] and bits(runs["collect"][2]) == bits(runs["explicit"][2])
    assert np.abs(runs["collect"][0]["actions"]).max() > 1.0  # (the slab keeps the raw action)
    assert calls[0] is None and len(calls) == 1 + steps and all(list(mask)[:2] == [False, True] for mask in calls[1:])
    for g, resets in enumerate((1, 1 + steps, 1 + -(-steps // 3))):
        moved = np.random.PCG64DXSM(cases.seeds_of(groups)[g]).advance(resets * m * spec.latent)
        assert runs["collect"][1][g] == moved.state, g


def test_collect_makes_no_call_when_no_group_is_due(no_gpu):  # noqa: F811
    env = harness.VectorContinuousJumps(num_envs=4, **rollout_cases.ENV_KW)
    try:
        spec = sde_cases.e2e_spec(env)
        twin = harness.SdePopulationPolicy(spec, 2, [1, 2])
        calls = []
        inner = twin.reset_noise
        twin.reset_noise = lambda groups=None, num_envs=None: (calls.append(groups), inner(groups, num_envs))[1]
        buffer = harness.Rollout(env, 5)
        buffer.start(env.reset(seed=1)[0])
        buffer.collect(twin, sde_sample_freq=[-1, 4])
        assert calls == [None, [False, True], [False, True]]  # (before the loop; t = 0 and t = 4)
        buffer.start()
        buffer.collect(twin, sde_sample_freq=2)  # (a scalar is every group's)
        assert calls[3:] == [None, [True, True], [True, True], [True, True]]
    finally:
        env.close()


def test_the_end_to_end_twin_runs_hold_what_they_promise(no_gpu):  # noqa: F811
    """What tests/test_gpu_population_sde.py compares the device with: two iterations of collect + train on a 3-group
    VectorContinuousJumps with a normaliser and discounts per group: every group's log_std starts at its log_std_init and
    moves, raw actions pass the clamp, episodes end, and the draw counts are those of [-1, 1, 3]."""
    runs, rng_states, states, spec = cases.e2e_twin_runs()
    groups = cases.E2E["groups"]
    for g, draws in enumerate(cases.e2e_draws(spec)):
        assert rng_states[g] == np.random.PCG64DXSM(cases.seeds_of(groups)[g]).advance(draws).state
    assert (runs[1]["stats"][:, :, 7] == 0).all() and np.concatenate([run["truncated"] for run in runs]).any()
    log_std = runs[-1]["params"][:, spec.log_std_at:]
    assert (log_std[0] != F32(cases.E2E["log_std_init"][0])).any() and (log_std[2] == F32(cases.E2E["log_std_init"][2])).all()
    assert np.abs(runs[0]["actions"]).max() > 1.0


def test_refusals(no_gpu):  # noqa: F811
    spec = cases.spec_of(0)
    make = harness.SdePopulationPolicy
    with pytest.raises(ValueError, match="one seed per group"):
        make(spec, 3, [1, 2])
    with pytest.raises(ValueError, match="one seed per group"):
        make(spec, 3, 7)
    with pytest.raises(ValueError, match="log_std_init has 2 entries"):
        make(spec, 3, [1, 2, 3], log_std_init=[0.0, 1.0])
    with pytest.raises(ValueError, match="not in 1"):
        make(spec, 0, [])
    categorical = policy.MlpPolicySpec(3, 4)
    with pytest.raises(ValueError, match="Gaussian head of SdePolicySpec"):
        make(categorical, 2, [1, 2])
    with pytest.raises(ValueError, match="out of scope"):  # (the Categorical population keeps refusing an sde spec)
        harness.PopulationPolicy(spec, 2, [1, 2])
    population = make(spec, 3, [1, 2, 3])
    for mask in ([True, False], [True] * 4, [1, 2, 0], "yes", 1):
        with pytest.raises(ValueError, match="boolean sequence"):
            population.reset_noise(groups=mask, num_envs=6)
    with pytest.raises(ValueError, match="not divisible"):
        population.reset_noise(num_envs=7)
    assert population.rng_state() == [np.random.PCG64DXSM(seed).state for seed in (1, 2, 3)]
    with pytest.raises(TypeError, match="PopulationPolicy"):
        harness.PopulationLearner(harness.SdePolicy(spec, 0))
    with pytest.raises(TypeError, match="DevicePopulationPolicy"):
        harness.DevicePopulationLearner(population)
    jumps = harness.VectorContinuousJumps(num_envs=6, **rollout_cases.ENV_KW)
    steps = harness.VectorDiscreteSteps(num_envs=6, **rollout_cases.ENV_KW)
    try:
        with pytest.raises(TypeError, match="device-resident"):
            harness.DeviceSdePopulationPolicy(jumps, spec, 3, [1, 2, 3])
        e2e = sde_cases.e2e_spec(jumps)
        twin = make(e2e, 3, [1, 2, 3])
        buffer = harness.Rollout(steps, 2)
        buffer.start(steps.reset()[0])
        with pytest.raises(ValueError, match="Gaussian head"):  # (a Discrete space)
            buffer.collect(twin)
        with pytest.raises(ValueError, match="Gaussian head"):
            harness.PopulationLearner(twin).train(buffer, 1, 2)
        buffer = harness.Rollout(jumps, 2, groups=3)
        buffer.start(jumps.reset()[0])
        for freqs in ([1, 2], [1, 2, 3, 4]):
            with pytest.raises(ValueError, match=f"sde_sample_freq has {len(freqs)} entries"):
                buffer.collect(twin, sde_sample_freq=freqs)
        for freqs in ([1, 0, 2], [1, -2, 2], [1, 2.5, 2], 0):
            with pytest.raises(ValueError, match="not -1 or a positive integer"):
                buffer.collect(twin, sde_sample_freq=freqs)
        two = harness.Rollout(jumps, 2, groups=2)
        two.start(jumps.reset()[0])
        with pytest.raises(ValueError, match="population policy of 3 groups"):
            two.collect(twin)
        assert twin.rng_state() == [np.random.PCG64DXSM(seed).state for seed in (1, 2, 3)]  # (no refusal drew)
        buffer.collect(twin, sde_sample_freq=[-1, 1, 2])
        categorical_population = harness.PopulationPolicy(policy.MlpPolicySpec(e2e.obs_width, 13), 3, [1, 2, 3])
        with pytest.raises(ValueError, match="out of scope"):  # (a Categorical population with a Box rollout, as before)
            harness.PopulationLearner(categorical_population).train(buffer, 1, 2)
        with pytest.raises(ValueError, match="more than the 4 rows"):
            harness.PopulationLearner(twin).train(buffer, 1, 5)
        assert harness.PopulationLearner(twin).train(buffer, 1, 4, generator=np.random.default_rng(0)).shape == (1, 3, 8)
        # a plain SdePolicy is collected as before
        plain = harness.SdePolicy(e2e, 0)
        single = harness.Rollout(jumps, 2)
        single.start(jumps.reset()[0])
        with pytest.raises(TypeError):  # (one value per group belongs to a population)
            single.collect(plain, sde_sample_freq=[1, 2, 3])
        single.collect(plain, sde_sample_freq=1)
    finally:
        jumps.close()
        steps.close()


def test_sizes_follow_the_sde_layout():
    """rf_sde_grouped_state_size / _workspace_size are G times the ungrouped sde sizes: csrc/rf_ppo.h's size rules for the
    host (tests/popcheck builds them for the Categorical layout; here the source is read)."""
    text = open(os.path.join(ROOT, "reinfocus_amd", "csrc", "rf_ppo.h")).read()
    assert "static_assert(!(kSde && kGrouped)" not in text
    for name in ("population_state_bytes", "population_workspace_bytes"):
        body = text[text.index("unsigned long long " + name):]
        assert "sde ? sde_layout(d, L) : policy_layout(d, L)" in body[:body.index("\n}\n")], name


def test_binding_matches_the_header():
    """Every grouped rf_sde_ entry point of the header is bound with as many arguments as it declares, and has a Context
    method."""
    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    seen = []
    for name, arguments in re.findall(r"\b(?:int|unsigned long long)\s+(rf_sde_\w*grouped\w*)\s*\((.*?)\)\s*;", text, flags=re.S):
        bound = re.search(rf"lib\.{name}\.argtypes = \[(.*?)\]", source, flags=re.S).group(1).split(",")
        assert len(bound) == len(arguments.split(",")), name
        assert name in _native.SYMBOLS and hasattr(_native.Context, name[3:]), name
        seen.append(name)
    assert sorted(seen) == ["rf_sde_forward_grouped", "rf_sde_grouped_state_size", "rf_sde_grouped_workspace_size",
                            "rf_sde_noise_reset_grouped", "rf_sde_update_grouped"]


def test_import_stays_free_of_torch():
    import subprocess
    import sys

    code = ("import sys; from reinfocus_amd.environments import harness; "
            "harness.SdePopulationPolicy; harness.DeviceSdePopulationPolicy; assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
