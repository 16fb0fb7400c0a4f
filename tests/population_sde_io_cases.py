"""TEST INFRASTRUCTURE: what tests/test_population_sde_logic.py and tests/test_gpu_population_sde.py share -- networks,
inputs, the numpy twins' results of a population of gSDE learners (include/reinfocus_hip.h, "population sde") -- and the
child process of the GPU file.

As tests/population_io_cases.py: everything that needs torch and the library together runs in one fresh process that
imports torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.population_sde_io_cases <results.jsonl>
"""

import functools
import os
import sys

import numpy as np

from tests import policy_io_cases as policy_cases
from tests import population_io_cases as pop_cases
from tests import rollout_io_cases as rollout_cases
from tests import sde_io_cases as sde_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = policy_cases.bits
SENTINEL = policy_cases.SENTINEL
# (obs_width, pi, vf, activation): L = 5, P + L = 52 < 256; L = 64, P + L = 2023 (more than one block of
# ppo_gradient_kernel's 256 leaves and of ppo_adam_kernel's 1024-parameter slices).  m L is 15 at the least (well under
# one block of 256) and 704 at the most (ragged over three).
NETWORKS = ((3, (5,), (4,), "tanh"), (20, (64,), (17, 9), "relu"))
GROUPS = (1, 3, 5)
PER_GROUP = pop_cases.PER_GROUP  # 3, 8, 11
CONSUMED = pop_cases.CONSUMED    # 0 and 2^32 + 5: which one a group has had depends on its index
T = pop_cases.T
UPDATE_GROUPS = pop_cases.UPDATE_GROUPS
UPDATE_SHAPES = pop_cases.UPDATE_SHAPES  # (B, m): m T = 12 (B = 5, 8) and 44 (B = 13)
EPOCHS = pop_cases.EPOCHS
WIDE = ((0, 64, 8), (1, 64, 8), (0, 65, 8), (1, 65, 8))  # (network, G, m) of noise and forward
WIDE_UPDATE = dict(index=1, groups=64, per_group=8, steps=32, batch=64)
# large minibatches, as population_io_cases.LARGE_CASES (m = 8, T = 128, N = 1024 rows per group): 512, 513, 1000 and 1024
# at G = 3 on NETWORKS[1], and 513 at G = 2 on the widest network of sde_io_cases (LARGE_NETWORKS, index 2; P + L = 138 k)
LARGE = pop_cases.LARGE
LARGE_NETWORKS = (sde_cases.NETWORKS[3],)
LARGE_CASES = tuple((1, 3, batch) for batch in (512, 513, 1000, 1024)) + ((2, 2, 513),)  # (network, G, B)
LARGE_ALONE = (1, 3, 1000)
ALONE_ENTRIES = ("sde_update", "sde_workspace_size")
LIMIT_GROUPS, LIMIT_PERIODS, LIMIT_GENERATORS = 65535, (7, 5, 3), 11
LIMIT_NETWORK = (1, (1,), (1,), "relu")
E2E = dict(envs=6, groups=3, steps=rollout_cases.T, epochs=2, batch=4, iterations=2, freqs=[-1, 1, 3],
           log_std_init=[-0.5, -1.25, 0.25], gammas=[0.99, 0.9, 0.95], gae_lambdas=[0.92, 0.95, 0.8])
FORWARD_OUTPUTS = sde_cases.FORWARD_OUTPUTS
HOT = 100.0  # a log_std whose standard deviation is +inf: theta is +-inf, or the canonical NaN where the normal is 0

seeds_of = pop_cases.seeds_of
advanced_states = pop_cases.advanced_states
group_hypers, wide_hypers = pop_cases.group_hypers, pop_cases.wide_hypers
minibatches, update_permutations, twin_states = pop_cases.minibatches, pop_cases.update_permutations, pop_cases.twin_states


def spec_of(index):
    return sde_cases.spec_of((NETWORKS + LARGE_NETWORKS)[index])


def twin_policy(index, groups, base=100, hot=None):
    """(spec, SdePopulationPolicy): every group with weights and a log_std of its own; group `hot` has log_std HOT."""
    from reinfocus_amd.environments import harness

    spec = spec_of(index)
    twin = harness.SdePopulationPolicy(spec, groups, seeds_of(groups))
    for g in range(groups):
        twin.load_state_dict(sde_cases.state_dict(spec, base + 17 * g), group=g)
    if hot is not None:
        twin.params[hot, spec.log_std_at:] = F32(HOT)
    return spec, twin


def consumed_of(groups):
    """uint64 [G]: 0 in the even groups, 2^32 + 5 in the odd ones."""
    return np.array([CONSUMED[g % 2] for g in range(groups)], dtype=np.uint64)


def hot_group(groups):
    return groups // 2 if groups >= 3 else None


def wanted_noise(index, groups, per_group, hot=None):
    """(twin, theta [G m][L]) after one reset_noise() of the twin whose generators had given consumed_of(G) draws."""
    spec, twin = twin_policy(index, groups, hot=hot)
    twin.set_rng_state(advanced_states_each(groups, consumed_of(groups)))
    twin.reset_noise(num_envs=groups * per_group)
    return twin, twin.noise()


def advanced_states_each(groups, consumed):
    states = []
    for seed, count in zip(seeds_of(groups), consumed):
        states.append(np.random.PCG64DXSM(seed).advance(int(count)).state)
    return states


def select_of(groups):
    """uint8 [G]: the first, a middle and the last group off."""
    select = np.ones(groups, dtype=np.uint8)
    select[[0, groups // 2, groups - 1]] = 0
    return select


def forward_inputs(index, groups, per_group):
    width, n = NETWORKS[index][0], groups * per_group
    return (policy_cases.hostile_rows(width, n, 70 * index + n, False), policy_cases.hostile_rows(width, n, 11 + n, True))


@functools.lru_cache(maxsize=None)
def wanted_forward(index, groups, per_group):
    """(params [G][P + L], theta, {sampled, deterministic}: the seven outputs of sde_numpy group by group, concatenated)."""
    from reinfocus_amd.environments import sde

    twin, theta = wanted_noise(index, groups, per_group)
    spec = twin.spec
    obs, final_obs = forward_inputs(index, groups, per_group)
    want = {}
    for mode in ("sampled", "deterministic"):
        parts = []
        for g in range(groups):
            rows = slice(g * per_group, (g + 1) * per_group)
            parts.append(sde.sde_numpy(spec, twin.params[g], obs[rows], final_obs[rows], theta[rows],
                                       deterministic=mode == "deterministic"))
        want[mode] = {name: np.concatenate([part[name] for part in parts]) for name in FORWARD_OUTPUTS}
    return twin.params.copy(), theta, want


# ---- updates ---------------------------------------------------------------------------------------------------------
def update_batch(index, groups, per_group, seed=0, steps=T, wide=False):
    """flat()'s arrays for G groups of m T rows: the raw actions are each group's own sampled ones (some past +-1), the
    stored log-probabilities its own, shifted so that the ratios lie inside the clip range and past both bounds."""
    from reinfocus_amd.environments import sde

    spec, twin = twin_policy(index, groups, base=300)
    rows = per_group * steps
    total = groups * rows
    rng = np.random.default_rng(1500 * index + 10 * per_group + seed)
    obs = rng.standard_normal((total, spec.obs_width)).astype(F32)
    actions, log_probs = np.zeros(total, dtype=F32), np.zeros(total, dtype=F32)
    for g in range(groups):
        piece = slice(g * rows, (g + 1) * rows)
        theta = sde.noise_numpy(twin.params[g, spec.log_std_at:], rng.random(rows * spec.latent))
        got = sde.sde_numpy(spec, twin.params[g], obs[piece], None, theta)
        assert np.isfinite(got["actions"]).all() and np.isfinite(got["log_probs"]).all()
        actions[piece] = got["actions"]
        log_probs[piece] = got["log_probs"] - rng.choice(np.array([0.0, 0.3, -0.3, 0.05, -0.05], dtype=F32), rows)
    batch = {"observations": obs, "actions": actions, "log_probs": log_probs,
             "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32)}
    return spec, twin, batch


def _chained(twin, flat, hypers, order):
    from reinfocus_amd.environments import harness

    learner = harness.PopulationLearner(twin, **hypers)
    seen = []
    for rows in order:
        stats = learner.update(flat, rows)
        seen.append((twin.params.copy(), twin_states(learner), stats.copy()))
    return seen


@functools.lru_cache(maxsize=None)
def twin_updates(index, batch, per_group):
    """Per update (params [G][P + L], states [G][S], stats [G][8]) of the twin population."""
    spec, twin, flat = update_batch(index, UPDATE_GROUPS, per_group)
    return _chained(twin, flat, group_hypers(UPDATE_GROUPS),
                    minibatches(update_permutations(UPDATE_GROUPS, per_group * T, 7 + batch), batch))


def wide_update_inputs():
    w = WIDE_UPDATE
    spec, twin, flat = update_batch(w["index"], w["groups"], w["per_group"], seed=9, steps=w["steps"])
    rows = w["per_group"] * w["steps"]
    return spec, twin, flat, wide_hypers(w["groups"]), minibatches(update_permutations(w["groups"], rows, 73), w["batch"])[:1]


@functools.lru_cache(maxsize=None)
def wide_twin_updates():
    spec, twin, flat, hypers, order = wide_update_inputs()
    return _chained(twin, flat, hypers, order)


def large_inputs(index, groups, batch):
    """(spec, twin, flat, hypers' keywords, the index arrays of the updates) of one of LARGE_CASES."""
    spec, twin, flat = update_batch(index, groups, LARGE["per_group"], seed=3, steps=LARGE["steps"])
    return spec, twin, flat, group_hypers(groups), pop_cases.large_indices(groups, batch, 900 + 7 * index + batch)


@functools.lru_cache(maxsize=None)
def large_twin_updates(index, groups, batch):
    spec, twin, flat, hypers, order = large_inputs(index, groups, batch)
    return _chained(twin, flat, hypers, order)


large_update_promises = pop_cases.large_update_promises


def isolation_inputs():
    """Four groups; group 1's minibatch holds a row whose raw action is NaN, group 2's one whose observation has a NaN."""
    index, groups, per_group, batch = 0, 4, 3, 5
    spec, twin, flat = update_batch(index, groups, per_group, seed=5)
    rows = per_group * T
    order = update_permutations(groups, rows, 3)[0][:, :batch].copy()
    flat["actions"][1 * rows + order[1, 2]] = np.nan
    flat["observations"][2 * rows + order[2, 1], 1] = np.nan
    return spec, twin, flat, order


# ---- the limit: 65535 groups of one row --------------------------------------------------------------------------------
def limit_spec():
    return sde_cases.spec_of(LIMIT_NETWORK)


@functools.lru_cache(maxsize=None)
def limit_parts():
    """(7 packed parameter sets, 5 blocks of one row each, 3 hyper-parameter sets).  Weights and observations are positive,
    so the one ReLU unit of either net is alive; log_std differs between the sets; adam_eps is large, so the first Adam
    step depends on the gradient's size."""
    from reinfocus_amd.environments import learner

    spec = limit_spec()
    rng = np.random.default_rng(65535)
    params = []
    for k in range(LIMIT_PERIODS[0]):
        packed = np.abs(spec.pack(sde_cases.state_dict(spec, 700 + k))) + F32(0.25 + 0.125 * k)
        packed[spec.log_std_at:] = F32(-1.0 + 0.25 * k)
        params.append(packed)
    blocks = []
    for j in range(LIMIT_PERIODS[1]):
        blocks.append(dict(observations=np.array([[0.5 + 0.75 * j]], dtype=F32), final=np.array([[3.0 - 0.5 * j]], dtype=F32),
                           actions=np.array([0.4 * j - 0.9], dtype=F32), log_probs=np.array([-0.7 + 0.1 * j], dtype=F32),
                           advantages=rng.standard_normal(1).astype(F32), returns=rng.standard_normal(1).astype(F32)))
    hypers = [learner.Hyper(learning_rate=1e-2 / (1 + h), clip_range=0.1 + 0.1 * h, ent_coef=0.01 * (1 + h),
                            vf_coef=0.5 + 0.25 * h, max_grad_norm=(1e6, 0.5, 0.05)[h], beta1=0.9 - 0.1 * h,
                            beta2=0.999 - 0.01 * h, adam_eps=(0.1, 0.3, 1.0)[h], normalize_advantage=h % 2)
              for h in range(LIMIT_PERIODS[2])]
    return params, blocks, hypers


@functools.lru_cache(maxsize=None)
def limit_results():
    """For each of the 105 combinations c (parameter set c % 7, block c % 5, hyper-parameters c % 3), by the existing twin
    functions: the deterministic forward's outputs and the first update's (params, state, stats) from a fresh optimizer."""
    from reinfocus_amd.environments import learner, sde

    spec = limit_spec()
    params, blocks, hypers = limit_parts()
    forwards, updates = [], []
    for c in range(105):
        k, j, h = (c % period for period in LIMIT_PERIODS)
        got = sde.sde_numpy(spec, params[k], blocks[j]["observations"], blocks[j]["final"], None, deterministic=True)
        forwards.append(tuple(got[name] for name in FORWARD_OUTPUTS))
        batch = {key: blocks[j][key] for key in learner.BATCH_KEYS}
        updates.append(learner.ppo_update_numpy(spec, params[k], learner.fresh_state(spec), batch, np.zeros(1, dtype=np.int64),
                                                hypers[h]))
    return forwards, updates


def limit_arrays(groups=LIMIT_GROUPS):
    """What group g gets and what it must give: (inputs dict, wanted theta [G][1], wanted forward outputs, wanted (params,
    states, stats)).  Group g draws from generator g % 11 with g draws taken before, so every group's draw is its own."""
    from reinfocus_amd.environments import learner, policy, population, sde

    spec = limit_spec()
    params, blocks, hypers = limit_parts()
    forwards, updates = limit_results()
    g = np.arange(groups)
    k, j, h, c = g % LIMIT_PERIODS[0], g % LIMIT_PERIODS[1], g % LIMIT_PERIODS[2], g % 105
    inputs = {"params": np.stack(params)[k], "hyper": population.hyper_records(hypers)[h], "consumed": g.astype(np.uint64)}
    for key in ("observations", "final") + tuple(key for key in learner.BATCH_KEYS if key != "observations"):
        inputs[key] = np.concatenate([block[key] for block in blocks])[j]
    generators = [np.random.PCG64DXSM(900 + i) for i in range(LIMIT_GENERATORS)]
    inputs["gens"] = np.array([policy.generator_words(generator) for generator in generators], dtype=np.uint64)[g % LIMIT_GENERATORS]
    draws = np.stack([np.random.Generator(generator).random(groups) for generator in generators])[g % LIMIT_GENERATORS, g]
    with np.errstate(all="ignore"):
        theta = policy.canonical(sde.normal32(draws) * sde.expw32(inputs["params"][:, spec.log_std_at]))
    wanted_forward = tuple(np.concatenate([forward[i] for forward in forwards])[c] for i in range(len(FORWARD_OUTPUTS)))
    wanted_update = tuple(np.stack([update[i] for update in updates])[c] for i in range(3))
    return inputs, theta.reshape(groups, 1), wanted_forward, wanted_update


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
e2e_permutations = pop_cases.e2e_permutations
e2e_hypers = pop_cases.e2e_hypers


def e2e_env(device_form):
    from reinfocus_amd.environments import harness

    extra = dict(episode_records=True, learner_view=harness.LearnerView(frame_stack=rollout_cases.STACK, gamma=E2E["gammas"],
                                                                        groups=E2E["groups"]))
    if device_form:
        return harness.DeviceVectorContinuousJumps(num_envs=E2E["envs"], device_initializer=True, **rollout_cases.ENV_KW,
                                                   **extra)
    return harness.VectorContinuousJumps(num_envs=E2E["envs"], **rollout_cases.ENV_KW, **extra)


def e2e_spec(env):
    from reinfocus_amd.environments import sde

    return sde.SdePolicySpec(int(env.single_observation_space.shape[0]), pi=(6,), vf=(5, 7), activation="tanh")


def e2e_states(spec):
    """One state_dict per group; log_std is left to log_std_init (the entry is dropped after packing)."""
    return [sde_cases.state_dict(spec, 500 + 17 * g) for g in range(E2E["groups"])]


def e2e_load(policy, spec, wrap):
    """Each group's weights, its log_std the group's log_std_init."""
    for g, state in enumerate(e2e_states(spec)):
        state["log_std"][:] = F32(E2E["log_std_init"][g])
        policy.load_state_dict({name: wrap(value) for name, value in state.items()}, group=g)


def e2e_runs(rollout, policy, learner, reset, unwrap, wrap):
    obs = reset()
    seen = []
    for iteration in range(E2E["iterations"]):
        rollout.start(obs if iteration == 0 else None)
        rollout.collect(policy, sde_sample_freq=E2E["freqs"])
        record = policy_cases.slabs_of(rollout, unwrap)
        record["theta"] = unwrap(policy.noise())
        record["stats"] = unwrap(learner.train(rollout, E2E["epochs"], E2E["batch"],
                                               permutations=wrap(e2e_permutations(iteration))))
        record["params"] = unwrap(policy.params)
        seen.append(record)
    return seen


def e2e_draws(spec):
    """Draws each group's generator has given after the iterations: resets of m L draws, 1 + (T or ceil(T / f) or 0) per
    rollout."""
    m, steps = E2E["envs"] // E2E["groups"], E2E["steps"]
    resets = [1 + (0 if f < 0 else -(-steps // f)) for f in E2E["freqs"]]
    return [E2E["iterations"] * r * m * spec.latent for r in resets]


@functools.lru_cache(maxsize=None)
def e2e_twin_runs():
    from reinfocus_amd.environments import harness

    env = e2e_env(False)
    try:
        spec = e2e_spec(env)
        policy = harness.SdePopulationPolicy(spec, E2E["groups"], seeds_of(E2E["groups"]), log_std_init=E2E["log_std_init"])
        e2e_load(policy, spec, lambda a: a)
        learner = harness.PopulationLearner(policy, **e2e_hypers())
        rollout = harness.Rollout(env, E2E["steps"], E2E["gammas"], E2E["gae_lambdas"], groups=E2E["groups"])
        runs = e2e_runs(rollout, policy, learner, lambda: env.reset()[0], np.array, lambda a: a)
        return runs, policy.rng_state(), twin_states(learner), spec
    finally:
        env.close()


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
_untouched = policy_cases._untouched
_cuda_states = pop_cases._cuda_states


def _slab(torch, rows, width=None, guard=1):
    """(whole, view): `rows` rows of float32 sentinels (of `width` floats each, or scalars) between `guard` guard rows."""
    shape = (rows + 2 * guard,) if width is None else (rows + 2 * guard, width)
    whole = torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    return whole, whole[guard:guard + rows]


def _guards(whole, rows, guard=1):
    return _untouched(whole[:guard]) and _untouched(whole[guard + rows:])


def _words(torch, array):
    """A uint64 host array as the device tensor of its bits."""
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.uint64).view(np.int64)).cuda()


def _noise(torch, ctx, spec, groups, per_group, params, table, consumed, select, theta, changed=()):
    a = dict(desc=spec.desc(), groups=groups, per_group=per_group, params=params.data_ptr(), gens=table.data_ptr(),
             consumed=consumed.data_ptr(), select=None if select is None else select.data_ptr(), theta=theta.data_ptr())
    a.update(changed)
    ctx.sde_noise_reset_grouped(a["desc"], a["groups"], a["per_group"], a["params"], a["gens"], a["consumed"], a["select"],
                                a["theta"], torch.cuda.current_stream().cuda_stream)


def _rows_differ(got, want):
    """Indices of the rows of two equally shaped arrays whose bytes differ."""
    x = np.ascontiguousarray(got).view(np.uint8).reshape(got.shape[0], -1)
    y = np.ascontiguousarray(want).view(np.uint8).reshape(want.shape[0], -1)
    return np.flatnonzero((x != y).any(axis=1))


def noise_case(torch, ctx, index, groups, per_group):
    """rf_sde_noise_reset_grouped against the twin as bytes: every group with its own log_std (one of them HOT where
    G >= 3) and 0 or 2^32 + 5 draws taken before; then with the first, a middle and the last group deselected, whose rows
    keep the sentinel; at G >= 5 also against G stand-alone rf_sde_noise_reset launches."""
    from reinfocus_amd.environments import policy

    hot = hot_group(groups)
    twin, want = wanted_noise(index, groups, per_group, hot)
    spec, n, L = twin.spec, groups * per_group, twin.spec.latent
    if hot is not None:
        piece = want[hot * per_group:(hot + 1) * per_group]
        assert not np.isfinite(piece).any() and np.isinf(piece).any()
        assert np.isfinite(np.delete(want, np.s_[hot * per_group:(hot + 1) * per_group], axis=0)).all()
    params = torch.from_numpy(twin.params).cuda()
    table = pop_cases._table(torch, groups)
    consumed = _words(torch, consumed_of(groups))
    whole, theta = _slab(torch, n, L)
    _noise(torch, ctx, spec, groups, per_group, params, table, consumed, None, theta)
    torch.cuda.synchronize()
    assert bits(theta.cpu().numpy()) == bits(want), f"theta differs in rows {_rows_differ(theta.cpu().numpy(), want)[:4]}"
    assert _guards(whole, n), "a guard row of theta was written"
    chosen = select_of(groups)
    whole, theta = _slab(torch, n, L)
    _noise(torch, ctx, spec, groups, per_group, params, table, consumed, torch.from_numpy(chosen).cuda(), theta)
    torch.cuda.synchronize()
    got = theta.cpu().numpy()
    for g in range(groups):
        rows = slice(g * per_group, (g + 1) * per_group)
        if chosen[g]:
            assert bits(got[rows]) == bits(want[rows]), f"selected group {g} differs"
        else:
            assert _untouched(theta[rows]), f"deselected group {g} was written"
    assert _guards(whole, n)
    if groups >= 5:
        alone = torch.zeros((n, L), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for g, state in enumerate(advanced_states_each(groups, consumed_of(groups))):
            generator = np.random.PCG64DXSM()
            generator.state = state
            ctx.sde_noise_reset(spec.desc(), params[g].data_ptr(), per_group, policy.generator_words(generator),
                                alone[g * per_group:(g + 1) * per_group].data_ptr(), stream)
        torch.cuda.synchronize()
        assert bits(alone.cpu().numpy()) == bits(want), "stand-alone launches differ"


def _forward(torch, ctx, spec, groups, per_group, params, obs, final_obs, theta, flags, out, changed=()):
    a = dict(desc=spec.desc(), groups=groups, per_group=per_group, params=params.data_ptr(), obs=obs.data_ptr(),
             final_obs=None if final_obs is None else final_obs.data_ptr(), theta=None if theta is None else theta.data_ptr(),
             flags=flags)
    a.update({name: None if out.get(name) is None else out[name].data_ptr() for name in FORWARD_OUTPUTS})
    a.update(changed)
    ctx.sde_forward_grouped(a["desc"], a["groups"], a["per_group"], a["params"], a["obs"], a["final_obs"], a["theta"],
                            a["flags"], *(a[name] for name in FORWARD_OUTPUTS), torch.cuda.current_stream().cuda_stream)


def _outputs(torch, n):
    slabs = {name: _slab(torch, n) for name in FORWARD_OUTPUTS}
    return {name: slab[0] for name, slab in slabs.items()}, {name: slab[1] for name, slab in slabs.items()}


def forward_case(torch, ctx, index, groups, per_group):
    """rf_sde_forward_grouped against the twin as bytes: sampled, deterministic and values only; every output a slice of a
    larger slab whose guard rows keep their sentinel; final_obs has NaN rows among live ones; where G >= 5 also against G
    stand-alone rf_sde_forward launches, and every group's mean differs from what group 0's parameters give."""
    from reinfocus_amd.environments import policy, sde

    spec = spec_of(index)
    n = groups * per_group
    params_h, theta_h, want = wanted_forward(index, groups, per_group)
    obs_h, final_h = forward_inputs(index, groups, per_group)
    params, obs, final_obs, theta = (torch.from_numpy(a).cuda() for a in (params_h, obs_h, final_h, theta_h))
    for mode, flags, noise in (("sampled", 0, theta), ("deterministic", policy.DETERMINISTIC, None)):
        whole, out = _outputs(torch, n)
        _forward(torch, ctx, spec, groups, per_group, params, obs, final_obs, noise, flags, out)
        torch.cuda.synchronize()
        for name in FORWARD_OUTPUTS:
            got = out[name].cpu().numpy()
            assert bits(got) == bits(want[mode][name]), f"{mode}: {name} differ in rows {_rows_differ(got, want[mode][name])[:4]}"
            assert _guards(whole[name], n), f"a guard row of {name} was written"
    finals = want["sampled"]["final_values"]
    assert np.isnan(finals).any() and not np.isnan(finals).all()  # (NaN-led final_obs rows among live ones)
    whole, out = _outputs(torch, n)
    only = {"values": out["values"], "final_values": out["final_values"]}
    _forward(torch, ctx, spec, groups, per_group, params, obs, final_obs, None, 0, only)
    torch.cuda.synchronize()
    for name in FORWARD_OUTPUTS:
        if name in only:
            assert bits(out[name].cpu().numpy()) == bits(want["sampled"][name]), f"values only: {name} differ"
        else:
            assert _untouched(whole[name]), f"values only: {name} was written"
    if groups >= 5:
        alone = {name: torch.zeros(n, dtype=torch.float32, device="cuda") for name in FORWARD_OUTPUTS}
        stream = torch.cuda.current_stream().cuda_stream
        for g in range(groups):
            rows = slice(g * per_group, (g + 1) * per_group)
            ctx.sde_forward(spec.desc(), params[g].data_ptr(), per_group, obs[rows].data_ptr(), final_obs[rows].data_ptr(),
                            theta[rows].data_ptr(), 0, *(alone[name][rows].data_ptr() for name in FORWARD_OUTPUTS), stream)
        torch.cuda.synchronize()
        for name in FORWARD_OUTPUTS:
            assert bits(alone[name].cpu().numpy()) == bits(want["sampled"][name]), f"stand-alone launches: {name} differ"
    everywhere = sde.sde_numpy(spec, params_h[0], obs_h, None, None, deterministic=True)["mean"]
    for g in range(1, groups):
        rows = slice(g * per_group, (g + 1) * per_group)
        assert np.isfinite(everywhere[rows]).any()
        assert bits(everywhere[rows]) != bits(want["sampled"]["mean"][rows]), f"group {g} does not tell its parameters from group 0's"


class _Learner(pop_cases._Learner):
    """Device copies of a twin population's parameters and batch, fresh optimizer states, and rf_sde_update_grouped."""

    def __init__(self, torch, ctx, spec, twin, flat, per_group, hypers, batch_most, steps=T, guarded=False):
        from reinfocus_amd.environments import learner, population

        params = twin if isinstance(twin, np.ndarray) else twin.params
        self.torch, self.ctx, self.spec, self.groups, self.per_group = torch, ctx, spec, params.shape[0], per_group
        self.steps, self.whole = steps, []
        self.params = self._slab(params.shape[1] if guarded else 0, params.reshape(-1))
        state_bytes = ctx.sde_grouped_state_size(spec.desc(), self.groups, per_group)
        assert state_bytes == self.groups * 4 * (learner.STATE_HEADER + 2 * spec.size)
        self.state = self._slab(state_bytes // 4 // self.groups if guarded else 0, np.zeros(state_bytes // 4, dtype=F32))
        size = ctx.sde_grouped_workspace_size(spec.desc(), self.groups, per_group, steps, batch_most)
        assert size == self.groups * ctx.sde_workspace_size(spec.desc(), batch_most) and size > 0
        self.workspace = self._slab(16 if guarded else 0, np.zeros(size // 4, dtype=F32))
        self.params = self.params.view(self.groups, -1)
        self.flat = {key: torch.from_numpy(np.ascontiguousarray(flat[key])).cuda() for key in learner.BATCH_KEYS}
        assert self.flat["actions"].dtype == torch.float32
        records = hypers if isinstance(hypers, np.ndarray) else population.hyper_records(hypers)
        self.hyper = torch.from_numpy(records.view(np.float64).copy()).cuda()
        self.stats = torch.full((self.groups + 2, 8), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)

    def update(self, index, changed=()):
        index = self.torch.from_numpy(np.ascontiguousarray(index)).cuda()
        a = dict(desc=self.spec.desc(), groups=self.groups, per_group=self.per_group, steps=self.steps,
                 hyper=self.hyper.data_ptr(),
                 params=self.params.data_ptr(), state=self.state.data_ptr(), workspace=self.workspace.data_ptr(),
                 obs=self.flat["observations"].data_ptr(), actions=self.flat["actions"].data_ptr(),
                 log_probs=self.flat["log_probs"].data_ptr(), advantages=self.flat["advantages"].data_ptr(),
                 returns=self.flat["returns"].data_ptr(), batch=index.shape[1], index=index.data_ptr(),
                 stats=self.stats[1:self.groups + 1].data_ptr())
        a.update(changed)
        self.ctx.sde_update_grouped(a["desc"], a["groups"], a["per_group"], a["steps"], a["hyper"], a["params"], a["state"],
                                    a["workspace"], a["obs"], a["actions"], a["log_probs"], a["advantages"], a["returns"],
                                    a["batch"], a["index"], a["stats"], self.torch.cuda.current_stream().cuda_stream)
        self.torch.cuda.synchronize()
        assert _untouched(self.stats[0]) and _untouched(self.stats[self.groups + 1]), "a guard row of the stats was written"
        assert self.guards_kept(), "a guard of the parameters, the states or the workspace was written"
        return (self.params.cpu().numpy(), self.state.cpu().numpy().reshape(self.groups, -1),
                self.stats[1:self.groups + 1].cpu().numpy())


_same_update = pop_cases._same_update


def _hypers(twin, keywords):
    from reinfocus_amd.environments import harness

    return harness.PopulationLearner(twin, **keywords).hypers()


def update_case(torch, ctx, index, batch, per_group):
    """rf_sde_update_grouped against the twin population over two epochs of chained updates (the last minibatch of an
    epoch is short); group 1 has learning_rate 0: its parameters keep their bytes while its Adam moments move; every
    group's log_std moves otherwise."""
    from reinfocus_amd.environments import learner

    want = twin_updates(index, batch, per_group)
    spec, twin, flat = update_batch(index, UPDATE_GROUPS, per_group)
    device = _Learner(torch, ctx, spec, twin, flat, per_group, _hypers(twin, group_hypers(UPDATE_GROUPS)), batch, guarded=True)
    before = twin.params.copy()
    rows = minibatches(update_permutations(UPDATE_GROUPS, per_group * T, 7 + batch), batch)
    assert len(rows) >= 3 and rows[-1].shape[1] < batch
    for update, index_rows in enumerate(rows):
        _same_update(device.update(index_rows), want[update], f"update {update}")
    params, states, stats = want[-1]
    assert (stats[:, 7] == 0).all() and bits(params[1]) == bits(before[1])
    for g in (0, 2):
        assert bits(params[g, spec.log_std_at:]) != bits(before[g, spec.log_std_at:]), f"group {g}'s log_std did not move"
    assert np.abs(states[1][learner.STATE_HEADER:]).max() > 0  # (m and v of the group with learning_rate 0 moved)


def wide_update_case(torch, ctx):
    """One rf_sde_update_grouped at G = 64 on m = 8, T = 32, B = 64 (P + L = 2023): all 64 groups as bytes, parameters and
    states between guard rows, the workspace of exactly rf_sde_grouped_workspace_size's bytes between guard floats."""
    want = wide_twin_updates()
    spec, twin, flat, hypers, order = wide_update_inputs()
    w = WIDE_UPDATE
    device = _Learner(torch, ctx, spec, twin, flat, w["per_group"], _hypers(twin, hypers), w["batch"], steps=w["steps"],
                      guarded=True)
    got = device.update(order[0])
    for g in (0, 31, 32, w["groups"] - 1):
        _same_update(tuple(x[g] for x in got), tuple(x[g] for x in want[0]), f"group {g}")
    _same_update(got, want[0], "wide")
    assert (want[0][2][:, 7] == 0).all()


def limit_case(torch, ctx):
    """RF_POPULATION_MAX_GROUPS groups of one row on the least network: one reset of every group's noise, a deterministic
    forward, one grouped update of fresh optimizers; every output byte of every group against its combination's result.
    Then 65536 groups: refused by all five entry points, nothing written."""
    from reinfocus_amd.environments import learner, policy

    spec, groups = limit_spec(), LIMIT_GROUPS
    inputs, want_theta, wanted_forward, wanted_update = limit_arrays()
    params, obs, final_obs = (torch.from_numpy(inputs[key]).cuda() for key in ("params", "observations", "final"))
    table, consumed = _words(torch, inputs["gens"]), _words(torch, inputs["consumed"])
    whole_theta, theta = _slab(torch, groups, 1)
    _noise(torch, ctx, spec, groups, 1, params, table, consumed, None, theta)
    torch.cuda.synchronize()
    differ = _rows_differ(theta.cpu().numpy(), want_theta)
    assert differ.size == 0, f"theta differs in {differ.size} groups, first {differ[:4]}"
    assert _guards(whole_theta, groups)
    whole, out = _outputs(torch, groups)
    _forward(torch, ctx, spec, groups, 1, params, obs, final_obs, None, policy.DETERMINISTIC, out)
    torch.cuda.synchronize()
    for name, wanted in zip(FORWARD_OUTPUTS, wanted_forward):
        differ = _rows_differ(out[name].cpu().numpy(), wanted)
        assert differ.size == 0, f"{name} differ in {differ.size} groups, first {differ[:4]}"
        assert _guards(whole[name], groups), f"a guard row of {name} was written"
    flat = {key: inputs[key] for key in learner.BATCH_KEYS}
    device = _Learner(torch, ctx, spec, inputs["params"], flat, 1, inputs["hyper"], 1, steps=1, guarded=True)
    got = device.update(np.zeros((groups, 1), dtype=np.int64))
    for name, x, y in zip(("params", "states", "stats"), got, wanted_update):
        differ = _rows_differ(x, y)
        assert differ.size == 0, f"{name} differ in {differ.size} groups, first {differ[:4]}"
    # one group more
    kept = [t.clone() for t in (device.params, device.state, device.stats, theta)]
    many = groups + 1
    assert ctx.sde_grouped_state_size(spec.desc(), many, 1) == 0 == ctx.sde_grouped_workspace_size(spec.desc(), many, 1, 1, 1)
    for call in (lambda: device.update(np.zeros((groups, 1), dtype=np.int64), dict(groups=many)),
                 lambda: _forward(torch, ctx, spec, many, 1, params, obs, final_obs, None, policy.DETERMINISTIC, out),
                 lambda: _noise(torch, ctx, spec, many, 1, params, table, consumed, None, theta)):
        try:
            call()
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert "must be in 1" in str(caught), str(caught)
        else:
            raise AssertionError("65536 groups were taken")
    torch.cuda.synchronize()
    for tensor, copy in zip((device.params, device.state, device.stats, theta), kept):
        assert torch.equal(tensor.view(torch.int32), copy.view(torch.int32)), "a refused call wrote an output"
    for name, wanted in zip(FORWARD_OUTPUTS, wanted_forward):
        assert bits(out[name].cpu().numpy()) == bits(wanted), f"a refused forward wrote {name}"
    assert device.guards_kept()


def isolation_case(torch, ctx):
    from reinfocus_amd.environments import harness, learner

    spec, twin, flat, order = isolation_inputs()
    before = twin.params.copy()
    twin_learner = harness.PopulationLearner(twin, learning_rate=1e-2)
    device = _Learner(torch, ctx, spec, twin, flat, 3, twin_learner.hypers(), order.shape[1])
    fresh = twin_states(twin_learner)
    stats = twin_learner.update(flat, order)
    want = (twin.params.copy(), twin_states(twin_learner), stats)
    assert list(stats[:, 7]) == [0, learner.INVALID, learner.NONFINITE, 0]
    got = device.update(order)
    _same_update(got, want, "isolation")
    for g in (1, 2):
        assert bits(got[0][g]) == bits(before[g]) and bits(got[1][g]) == bits(fresh[g]), f"group {g} was not skipped"
    for g in (0, 3):
        assert bits(got[0][g]) != bits(before[g])


def kernel_refusal_case(torch, ctx):
    """Each refusal of the entry points leaves every output as it was, and the unchanged call is then taken."""
    index, groups, per_group = 0, 5, 3
    spec = spec_of(index)
    n, L = groups * per_group, spec.latent
    params_h, theta_h, want = wanted_forward(index, groups, per_group)
    obs_h, final_h = forward_inputs(index, groups, per_group)
    params, obs, final_obs = (torch.from_numpy(a).cuda() for a in (params_h, obs_h, final_h))
    table, consumed = pop_cases._table(torch, groups), _words(torch, consumed_of(groups))
    select = torch.ones(groups, dtype=torch.uint8, device="cuda")
    whole_theta, theta = _slab(torch, n, L)
    whole, out = _outputs(torch, n)

    def refused(call, match, **changed):
        try:
            call(changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        torch.cuda.synchronize()
        assert _untouched(whole_theta) and all(_untouched(w) for w in whole.values()), f"an output was written ({match})"

    def noise(changed=()):
        _noise(torch, ctx, spec, groups, per_group, params, table, consumed, select, theta, changed)

    host = np.zeros((n + 2) * max(L, spec.obs_width), dtype=np.float32)
    refused(noise, "d_params is not device memory", params=np.zeros(groups * spec.size, dtype=F32).ctypes.data)
    refused(noise, "d_gens is not device memory", gens=np.zeros((groups, 4), dtype=np.uint64).ctypes.data)
    refused(noise, "d_consumed is not device memory", consumed=np.zeros(groups, dtype=np.uint64).ctypes.data)
    refused(noise, "d_select is not device memory", select=np.ones(groups, dtype=np.uint8).ctypes.data)
    refused(noise, "d_theta is not device memory", theta=host.ctypes.data)
    refused(noise, "not aligned", gens=table.data_ptr() + 4)
    refused(noise, "not aligned", consumed=consumed.data_ptr() + 4)
    refused(noise, "not aligned", theta=theta.data_ptr() + 2)
    refused(noise, "d_theta overlaps d_params", theta=params.data_ptr())
    refused(noise, "d_theta overlaps d_gens", theta=table.data_ptr())
    refused(noise, "must be in 1", groups=0)
    refused(noise, "must be in 1", per_group=0)
    refused(noise, "must be in 1", groups=65536)
    refused(noise, "outside the limits", desc=(spec.desc()[0], 2) + tuple(spec.desc()[2:]))  # (n_actions 2)
    noise()
    torch.cuda.synchronize()
    assert bits(theta.cpu().numpy()) == bits(theta_h) and _guards(whole_theta, n)
    noise_slab = whole_theta.clone()
    whole_theta.view(torch.int32).fill_(SENTINEL)

    def forward(changed=()):
        _forward(torch, ctx, spec, groups, per_group, params, obs, final_obs, noise_slab[1:n + 1], 0, out, changed)

    refused(forward, "d_obs is not device memory", obs=host.ctypes.data)
    refused(forward, "d_theta is not device memory", theta=host.ctypes.data)
    refused(forward, "d_values is not device memory", values=host.ctypes.data)
    refused(forward, "needs d_theta", theta=None)
    refused(forward, "not aligned", obs=obs.data_ptr() + 2)
    refused(forward, "d_values overlaps d_log_probs", values=out["log_probs"].data_ptr())
    refused(forward, "d_mean overlaps d_obs", mean=obs.data_ptr())
    refused(forward, "d_actions overlaps d_theta", actions=noise_slab[1:n + 1].data_ptr())
    refused(forward, "must be in 1", groups=0)
    refused(forward, "must be in 1", groups=65536)
    refused(forward, "outside the limits", desc=(spec.desc()[0], 2) + tuple(spec.desc()[2:]))
    refused(forward, "unknown flags", flags=2)
    forward()
    torch.cuda.synchronize()
    for name in FORWARD_OUTPUTS:
        assert bits(out[name].cpu().numpy()) == bits(want["sampled"][name]), name

    spec, twin, flat = update_batch(0, UPDATE_GROUPS, 3)
    device = _Learner(torch, ctx, spec, twin, flat, 3, _hypers(twin, group_hypers(UPDATE_GROUPS)), 5)
    rows = minibatches(update_permutations(UPDATE_GROUPS, 3 * T, 12), 5)[0]
    kept = [t.clone() for t in (device.params, device.state, device.stats)]

    def refused_update(match, index=rows, **changed):
        try:
            device.update(index, changed)
        except AssertionError as caught:
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        torch.cuda.synchronize()
        for tensor, copy in zip((device.params, device.state, device.stats), kept):
            assert torch.equal(tensor.view(torch.int32), copy.view(torch.int32)), f"an output was written ({match})"

    refused_update("d_obs is not device memory", obs=np.zeros((UPDATE_GROUPS * 12, spec.obs_width), dtype=F32).ctypes.data)
    refused_update("d_actions is not device memory", actions=np.zeros(UPDATE_GROUPS * 12, dtype=F32).ctypes.data)
    refused_update("d_hyper is not device memory", hyper=np.zeros(7 * UPDATE_GROUPS).ctypes.data)
    refused_update("must be in 1", groups=0)
    refused_update("must be in 1", per_group=0)
    refused_update("is not in 1", index=np.zeros((UPDATE_GROUPS, 13), dtype=np.int64))  # (B > m T)
    refused_update("d_stats overlaps d_params", stats=device.params.data_ptr())
    refused_update("d_workspace overlaps d_state", workspace=device.state.data_ptr())
    refused_update("not aligned", state=device.state.data_ptr() + 4)
    refused_update("outside the limits", desc=(spec.desc()[0], 2) + tuple(spec.desc()[2:]))
    first = _chained(twin, flat, group_hypers(UPDATE_GROUPS), [rows])[0]
    _same_update(device.update(rows), first, "after the refusals")


def one_group_case(torch):
    """G = 1: noise, act, three chained updates and rng_state() equal DeviceSdePolicy / DeviceLearner bit for bit."""
    from reinfocus_amd.environments import harness

    n = 11
    env = harness.DeviceVectorContinuousJumps(num_envs=n, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        spec = e2e_spec(env)
        state = _cuda_states(torch, sde_cases.state_dict(spec, 3))
        single = harness.DeviceSdePolicy(env, spec, 77)
        grouped = harness.DeviceSdePopulationPolicy(env, spec, 1, [77])
        single.load_state_dict(state)
        grouped.load_state_dict(state)
        assert torch.equal(grouped.params[0], single.params)
        rng = np.random.default_rng(2)
        obs = torch.from_numpy(rng.standard_normal((n, spec.obs_width)).astype(F32)).cuda()
        for deterministic in (False, True, False):
            single.reset_noise()
            grouped.reset_noise()
            assert bits(grouped.noise().cpu().numpy()) == bits(single.noise().cpu().numpy())
            ours = [t.clone() for t in grouped.act(obs, None, deterministic) if t is not None]
            theirs = [t for t in single.act(obs, None, deterministic) if t is not None]
            assert len(ours) == len(theirs) == 4
            for x, y in zip(ours, theirs):
                assert bits(x.cpu().numpy()) == bits(y.cpu().numpy())
            assert grouped.rng_state() == [single.rng_state()]
        assert bits(grouped.values(obs).cpu().numpy()) == bits(single.values(obs).cpu().numpy())
        total = n * T
        flat = {"observations": rng.standard_normal((total, spec.obs_width)).astype(F32),
                "actions": (0.7 * rng.standard_normal(total)).astype(F32),
                "log_probs": (-1.0 + 0.1 * rng.standard_normal(total)).astype(F32),
                "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32)}
        flat = _cuda_states(torch, flat)
        kw = dict(learning_rate=1e-2, ent_coef=0.01)
        one, many = harness.DeviceLearner(single, **kw), harness.DevicePopulationLearner(grouped, **kw)
        for update in range(3):
            index = torch.from_numpy(rng.permutation(total)[:13 - update].astype(np.int64)).cuda()
            theirs = one.update(flat, index)
            ours = many.update(flat, index[None, :].contiguous())
            assert bits(ours[0].cpu().numpy()) == bits(theirs.cpu().numpy()), f"update {update}: stats differ"
            assert float(theirs[7]) == 0
        assert bits(grouped.params[0].cpu().numpy()) == bits(single.params.cpu().numpy())
        assert bits(many.state[0].cpu().numpy()) == bits(one.state.cpu().numpy())
        assert many.state_dict()["step"] == [3]
    finally:
        env.close()


def end_to_end_case(torch):
    from reinfocus_amd.environments import harness

    want, want_rng, want_states, _ = e2e_twin_runs()
    env = e2e_env(True)
    try:
        spec = e2e_spec(env)
        groups = E2E["groups"]
        policy = harness.DeviceSdePopulationPolicy(env, spec, groups, seeds_of(groups), log_std_init=E2E["log_std_init"])
        e2e_load(policy, spec, lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
        learner = harness.DevicePopulationLearner(policy, **e2e_hypers())
        rollout = harness.DeviceRollout(env, E2E["steps"], E2E["gammas"], E2E["gae_lambdas"], groups=groups)
        got = e2e_runs(rollout, policy, learner, lambda: env.reset_tensors()[0], lambda t: t.cpu().numpy(),
                       lambda a: torch.from_numpy(a).cuda())
        policy_cases.same_runs(got, want)
        assert env.device_fault() is None
        assert policy.rng_state() == want_rng
        assert bits(learner.state.cpu().numpy()) == bits(want_states)
        for g, draws in enumerate(e2e_draws(spec)):
            assert want_rng[g] == np.random.PCG64DXSM(seeds_of(groups)[g]).advance(draws).state, f"group {g}'s draw count"
        assert (want[1]["stats"][:, :, 7] == 0).all() and bits(want[0]["params"][0]) != bits(want[1]["params"][0])
        assert np.abs(want[0]["flat/actions"]).max() > 1.0, "no raw action past the clamp"
        # resume: a second learner and policy from the state dicts go on bit for bit, log_std included
        kept, kept_params = learner.state_dict(), policy.params.clone()
        order = torch.from_numpy(e2e_permutations(9)).cuda()
        straight = learner.train(rollout, E2E["epochs"], E2E["batch"], permutations=order).clone()
        after = policy.params.clone()
        resumed = harness.DeviceSdePopulationPolicy(env, spec, groups, [0] * groups)
        policy.params.copy_(kept_params)
        for g in range(groups):
            resumed.load_state_dict(policy.state_dict(group=g), group=g)
        assert torch.equal(resumed.params, kept_params)
        second = harness.DevicePopulationLearner(resumed, **e2e_hypers())
        second.load_state_dict(kept)
        again = second.train(rollout, E2E["epochs"], E2E["batch"], permutations=order)
        assert torch.equal(again.view(torch.int32), straight.view(torch.int32)) and torch.equal(resumed.params, after)
        assert torch.equal(second.state.view(torch.int32), learner.state.view(torch.int32))
        resumed.set_rng_state(policy.rng_state())
        resumed.set_noise(policy.noise())
        mask = [True, False, True]
        resumed.reset_noise(groups=mask)
        policy.params.copy_(after)
        policy.reset_noise(groups=mask)
        assert torch.equal(resumed.noise().view(torch.int32), policy.noise().view(torch.int32))
        assert resumed.rng_state() == policy.rng_state()
    finally:
        env.close()


def surface_case(torch):
    """What the classes refuse, each with a message."""
    from reinfocus_amd.environments import harness, policy as policy_module

    env = harness.DeviceVectorContinuousJumps(num_envs=6, device_initializer=True, **rollout_cases.ENV_KW)
    steps = harness.DeviceVectorDiscreteSteps(num_envs=6, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        spec = e2e_spec(env)

        def raises(kind, match, call):
            try:
                call()
            except kind as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"not refused ({match})")

        make = harness.DeviceSdePopulationPolicy
        raises(ValueError, "not divisible", lambda: make(env, spec, 4, [1, 2, 3, 4]))
        raises(ValueError, "one seed per group", lambda: make(env, spec, 3, [1, 2]))
        raises(ValueError, "log_std_init has 2 entries", lambda: make(env, spec, 3, [1, 2, 3], log_std_init=[0.0, 1.0]))
        raises(ValueError, "Gaussian head", lambda: make(steps, spec, 3, [1, 2, 3]))
        raises(ValueError, "Gaussian head of SdePolicySpec",
               lambda: make(env, policy_module.MlpPolicySpec(spec.obs_width, 3), 3, [1, 2, 3]))
        raises(ValueError, "out of scope", lambda: harness.DevicePopulationPolicy(env, spec, 3, [1, 2, 3]))
        population = make(env, spec, 3, [1, 2, 3])
        obs = torch.zeros((6, spec.obs_width), dtype=torch.float32, device="cuda")
        raises(ValueError, "reset_noise", lambda: population.act(obs))
        raises(ValueError, "boolean sequence", lambda: population.reset_noise(groups=[True, False]))
        raises(ValueError, "boolean sequence", lambda: population.reset_noise(groups=[1, 2, 0]))
        assert population.rng_state() == [np.random.PCG64DXSM(seed).state for seed in (1, 2, 3)]
        population.reset_noise(groups=[True, False, True])
        raises(ValueError, "reset_noise", lambda: population.act(obs))
        population.reset_noise(groups=[False, True, False])
        population.act(obs)
        raises(ValueError, "rows", lambda: population.act(obs[:5].contiguous()))
        learner = harness.DevicePopulationLearner(population)
        rollout = harness.DeviceRollout(env, 2, groups=3)
        rollout.start(env.reset_tensors()[0])
        raises(ValueError, "sde_sample_freq has 2 entries", lambda: rollout.collect(population, sde_sample_freq=[1, 2]))
        raises(ValueError, "sde_sample_freq", lambda: rollout.collect(population, sde_sample_freq=[1, 0, 2]))
        raises(ValueError, "sde_sample_freq", lambda: rollout.collect(population, sde_sample_freq=[1, 2.5, 2]))
        two = harness.DeviceRollout(env, 2, groups=2)
        two.start(env.reset_tensors()[0])
        raises(ValueError, "population policy of 3 groups", lambda: two.collect(population))
        rollout.collect(population, sde_sample_freq=2)
        assert tuple(learner.train(rollout, 1, 4).shape) == (1, 3, 8)
        discrete = harness.DeviceRollout(steps, 2)
        raises(ValueError, "Gaussian head", lambda: learner.train(discrete, 1, 4))
        categorical = harness.DevicePopulationLearner(harness.DevicePopulationPolicy(
            steps, policy_module.MlpPolicySpec(spec.obs_width, 13), 3, [1, 2, 3]))
        raises(ValueError, "out of scope", lambda: categorical.train(rollout, 1, 4))
    finally:
        env.close()
        steps.close()


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    ctx = _native.Context(0)
    for index in range(len(NETWORKS)):
        for groups in GROUPS:
            for per_group in PER_GROUP:
                with record.case(f"noise/{index}/{groups}/{per_group}"):
                    noise_case(torch, ctx, index, groups, per_group)
                with record.case(f"forward/{index}/{groups}/{per_group}"):
                    forward_case(torch, ctx, index, groups, per_group)
        for batch, per_group in UPDATE_SHAPES:
            with record.case(f"update/{index}/{batch}"):
                update_case(torch, ctx, index, batch, per_group)
    for index, groups, per_group in WIDE:
        with record.case(f"noise/{index}/{groups}/{per_group}"):
            noise_case(torch, ctx, index, groups, per_group)
        with record.case(f"forward/{index}/{groups}/{per_group}"):
            forward_case(torch, ctx, index, groups, per_group)
    with record.case("update/wide"):
        wide_update_case(torch, ctx)
    for index, groups, batch in LARGE_CASES:
        with record.case(f"update/large/{index}/{groups}/{batch}"):
            pop_cases.large_update_case(torch, ctx, index, groups, batch, sys.modules[__name__])
    with record.case("limit"):
        limit_case(torch, ctx)
    with record.case("isolation"):
        isolation_case(torch, ctx)
    with record.case("kernel-refusals"):
        kernel_refusal_case(torch, ctx)
    ctx.close()
    with record.case("one-group"):
        one_group_case(torch)
    with record.case("end-to-end"):
        end_to_end_case(torch)
    with record.case("surface"):
        surface_case(torch)
    with record.case("finished"):
        pass


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    run_cases(sys.argv[1])
