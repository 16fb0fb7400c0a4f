"""TEST INFRASTRUCTURE: what tests/test_population_logic.py and tests/test_gpu_population.py share -- networks, inputs,
the numpy twins' results -- and the child process of the GPU file.

As tests/policy_io_cases.py: everything that needs torch and the library together runs in one fresh process that imports
torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.population_io_cases <results.jsonl>
"""

import functools
import os
import sys

import numpy as np

from tests import learner_io_cases as learner_cases
from tests import policy_io_cases as policy_cases
from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = policy_cases.bits
SENTINEL, SENTINEL64 = policy_cases.SENTINEL, policy_cases.SENTINEL64
# (obs_width, pi, vf, n_actions, activation): one hidden layer each, tanh, P = 59 < 256; one and two hidden layers, ReLU,
# P = 1324 > 1024 (more than one block of ppo_gradient_kernel's 256 leaves and of ppo_adam_kernel's 1024-parameter slices)
NETWORKS = ((3, (5,), (4,), 3, "tanh"), (20, (33,), (17, 9), 3, "relu"))
GROUPS = (1, 5)
PER_GROUP = (3, 8, 11)  # group borders inside what would be an ungrouped tile; exactly one tile; a ragged second tile
CONSUMED = (0, 2 ** 32 + 5)  # draws every generator has handed out before the call
T = 4
UPDATE_GROUPS = 3
UPDATE_SHAPES = ((5, 3), (8, 3), (13, 11))  # (B, m): m T = 12 or 44, so the last minibatch of an epoch is short
EPOCHS = 2
# wide: (network, G, m) of forwards with a group index past 4 -- 64 and 65 groups of the reference's n_envs = 8 (exactly one
# tile each) on both networks, 512 groups of 8 and of 1 on the first (tools/bench_population.py's largest G)
WIDE_FORWARD = ((0, 64, 8), (1, 64, 8), (0, 65, 8), (1, 65, 8), (0, 512, 8), (0, 512, 1))
# ppo_tuned.yml's first shape for 64 groups on NETWORKS[1]: m = 8, T = 32, B = 64, so 4 minibatches per epoch; one row of
# group 31 holds a NaN observation
WIDE_UPDATE = dict(index=1, groups=64, per_group=8, steps=32, batch=64, nan_group=31, nan_row=100)
# large minibatches on ppo_tuned.yml's ContinuousJumps shape, m = 8, T = 128 (N = 1024 rows per group): the sizes the
# ungrouped update is held to (learner_io_cases.LIMIT_BATCHES: the last single trip of the s_red reductions, the first
# second trip with a ragged last tile, no multiple of the tile, RF_PPO_MAX_BATCH) at G = 3 on NETWORKS[1], and 513 at G = 2
# on stable-baselines3's default network (LARGE_NETWORKS, index 2); two consecutive updates each.  LARGE_ALONE also runs as
# G stand-alone rf_ppo_update launches
LARGE = dict(per_group=8, steps=128, updates=2)
LARGE_NETWORKS = (learner_cases.NETWORKS[2],)
LARGE_CASES = tuple((1, 3, batch) for batch in learner_cases.LIMIT_BATCHES) + ((2, 2, 513),)  # (network, G, B)
LARGE_ALONE = (1, 3, 513)
ALONE_ENTRIES = ("ppo_update", "ppo_workspace_size")
# the limit: RF_POPULATION_MAX_GROUPS groups of one row on the least network; group g has parameter set g % 7, observation
# block g % 5 and hyper-parameter set g % 3, so neighbours differ in all three and g % 105 names the combination
LIMIT_GROUPS, LIMIT_PERIODS = 65535, (7, 5, 3)
LIMIT_NETWORK = (1, (1,), (1,), 2, "relu")
E2E = dict(envs=6, groups=3, steps=rollout_cases.T, epochs=2, batch=4, iterations=2)
GAMMA, GAE_LAMBDA = rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA


def seeds_of(groups):
    return [40 + 3 * g for g in range(groups)]


def spec_of(index):
    return policy_cases.spec_of((NETWORKS + LARGE_NETWORKS)[index])


def group_states(spec, groups, base):
    """One state_dict per group, each its own (hostile: logits that tie and one 200 below)."""
    return [policy_cases.state_dict(spec, base + 17 * g, hostile=g % 2 == 1) for g in range(groups)]


def twin_policy(index, groups, base=100):
    from reinfocus_amd.environments import harness

    spec = spec_of(index)
    twin = harness.PopulationPolicy(spec, groups, seeds_of(groups))
    for g, state in enumerate(group_states(spec, groups, base)):
        twin.load_state_dict(state, group=g)
    return spec, twin


def advanced_states(groups, consumed):
    states = []
    for seed in seeds_of(groups):
        generator = np.random.PCG64DXSM(seed)
        states.append(generator.advance(consumed).state)
    return states


def forward_inputs(index, groups, per_group):
    width, n = NETWORKS[index][0], groups * per_group
    return (policy_cases.hostile_rows(width, n, 50 * index + n, False), policy_cases.hostile_rows(width, n, 9 + n, True))


def wanted_forward(index, groups, per_group, consumed, deterministic):
    """(actions, values, log_probs, final_values) of the twin population, and the generator states afterwards."""
    _, twin = twin_policy(index, groups)
    twin.set_rng_state(advanced_states(groups, consumed))
    obs, final_obs = forward_inputs(index, groups, per_group)
    return twin.act(obs, final_obs, deterministic), twin.rng_state()


# ---- updates ---------------------------------------------------------------------------------------------------------
def group_hypers(groups):
    """Keyword arguments of the learners: every hyper-parameter differs between groups; group 1 has learning_rate 0."""
    lanes = np.arange(groups)
    return dict(learning_rate=[0.0 if g == 1 else 1e-2 / (1 + g) for g in range(groups)],
                clip_range=list(0.1 + 0.1 * lanes), ent_coef=list(0.01 * lanes), vf_coef=list(0.5 + 0.25 * lanes),
                max_grad_norm=[0.5, 1e6, 0.05][:groups] + [0.5] * max(0, groups - 3),
                normalize_advantage=[g % 2 == 0 for g in range(groups)],
                betas=[(0.9 - 0.1 * g, 0.999 - 0.01 * g) for g in range(groups)], adam_eps=list(1e-5 * (1 + lanes)))


def wide_hypers(groups):
    """group_hypers' pattern for more groups than its betas allow: its first five lanes repeat with periods 5, 4 and 3 (so
    neighbours differ in every hyper-parameter), the learning rate falls with g % 7, and group 1 alone has learning_rate 0."""
    five = group_hypers(5)

    def cycled(name, period):
        return [five[name][g % period] for g in range(groups)]

    return dict(learning_rate=[0.0 if g == 1 else 1e-2 / (1 + g % 7) for g in range(groups)],
                clip_range=cycled("clip_range", 5), ent_coef=cycled("ent_coef", 4), vf_coef=cycled("vf_coef", 5),
                max_grad_norm=cycled("max_grad_norm", 3), normalize_advantage=cycled("normalize_advantage", 2),
                betas=cycled("betas", 5), adam_eps=cycled("adam_eps", 4))


def update_batch(index, groups, per_group, seed=0, steps=T):
    """flat()'s arrays for G groups of m T rows; the stored log-probabilities are the twin's own, shifted so that the
    ratios lie inside the clip range and past both bounds."""
    from reinfocus_amd.environments import policy

    spec, twin = twin_policy(index, groups, base=300)
    rows = per_group * steps
    total = groups * rows
    rng = np.random.default_rng(1000 * index + 10 * per_group + seed)
    obs = rng.standard_normal((total, spec.obs_width)).astype(F32)
    actions = rng.integers(0, spec.n_actions, total).astype(np.int64)
    log_probs = np.zeros(total, dtype=F32)
    for g in range(groups):
        piece = slice(g * rows, (g + 1) * rows)
        own = policy.log_softmax(policy._net(spec, spec.nets(twin.params[g])[0], obs[piece]))[np.arange(rows), actions[piece]]
        log_probs[piece] = np.where(np.isfinite(own), own, F32(-1.0)) - rng.choice(
            np.array([0.0, 0.3, -0.3, 0.05, -0.05], dtype=F32), rows)
    batch = {"observations": obs, "actions": actions, "log_probs": log_probs,
             "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32)}
    return spec, twin, batch


def update_permutations(groups, rows, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.permutation(rows) for _ in range(groups)]) for _ in range(EPOCHS)]).astype(np.int64)


def minibatches(permutations, batch):
    """The index arrays [G][B] of every update, epoch by epoch; the last of an epoch may be short."""
    out = []
    for order in permutations:
        for first in range(0, order.shape[1], batch):
            out.append(np.ascontiguousarray(order[:, first:first + batch]))
    return out


def twin_states(learner):
    return np.stack([member.state for member in learner.learners])


@functools.lru_cache(maxsize=None)
def twin_updates(index, batch, per_group):
    """Per update (params [G][P], states [G][S], stats [G][8]) of the twin population."""
    from reinfocus_amd.environments import harness

    spec, twin, flat = update_batch(index, UPDATE_GROUPS, per_group)
    learner = harness.PopulationLearner(twin, **group_hypers(UPDATE_GROUPS))
    seen = []
    for rows in minibatches(update_permutations(UPDATE_GROUPS, per_group * T, 7 + batch), batch):
        stats = learner.update(flat, rows)
        seen.append((twin.params.copy(), twin_states(learner), stats.copy()))
    return seen


def wide_update_inputs():
    """(spec, twin, flat, hypers' keywords, the index arrays of two epochs) of WIDE_UPDATE."""
    w = WIDE_UPDATE
    spec, twin, flat = update_batch(w["index"], w["groups"], w["per_group"], seed=9, steps=w["steps"])
    rows = w["per_group"] * w["steps"]
    flat["observations"][w["nan_group"] * rows + w["nan_row"], 3] = np.nan
    return spec, twin, flat, wide_hypers(w["groups"]), minibatches(update_permutations(w["groups"], rows, 71), w["batch"])


@functools.lru_cache(maxsize=None)
def wide_twin_updates():
    """Per update (params [G][P], states [G][S], stats [G][8]) of the twin population on WIDE_UPDATE."""
    from reinfocus_amd.environments import harness

    spec, twin, flat, hypers, order = wide_update_inputs()
    learner = harness.PopulationLearner(twin, **hypers)
    seen = []
    for rows in order:
        stats = learner.update(flat, rows)
        seen.append((twin.params.copy(), twin_states(learner), stats.copy()))
    return seen


def wide_update_promises(want, before):
    """What WIDE_UPDATE's twin results hold: group 31 carries RF_PPO_NONFINITE in exactly the one update of each epoch
    whose minibatch holds the NaN row and keeps its bytes over it; group 1 (learning_rate 0) never moves; every other
    update of every group is taken."""
    from reinfocus_amd.environments import learner

    w = WIDE_UPDATE
    order = wide_update_inputs()[4]
    assert len(order) == 2 * (w["per_group"] * w["steps"] // w["batch"]) == 8 and all(rows.shape == (64, 64) for rows in order)
    hit = [update for update, rows in enumerate(order) if w["nan_row"] in rows[w["nan_group"]]]
    assert len(hit) == 2 and hit[0] < 4 <= hit[1]
    for update, (params, states, stats) in enumerate(want):
        flags = stats[:, 7].copy()
        assert flags[w["nan_group"]] == (learner.NONFINITE if update in hit else 0), update
        flags[w["nan_group"]] = 0
        assert (flags == 0).all(), update
        earlier = before if update == 0 else want[update - 1][0]
        assert (bits(params[w["nan_group"]]) == bits(earlier[w["nan_group"]])) == (update in hit), update
        if update in hit and update > 0:
            assert bits(states[w["nan_group"]]) == bits(want[update - 1][1][w["nan_group"]])
    params = want[-1][0]
    assert bits(params[1]) == bits(before[1]) and all(bits(params[g]) != bits(before[g]) for g in (0, 30, 31, 32, 63))


# ---- large minibatches ---------------------------------------------------------------------------------------------------
def chained_updates(twin, flat, hypers, order):
    """Per update of `order` (params [G][P], states [G][S], stats [G][8]) of a PopulationLearner over `twin`."""
    from reinfocus_amd.environments import harness

    learner = harness.PopulationLearner(twin, **hypers)
    seen = []
    for rows in order:
        stats = learner.update(flat, rows)
        seen.append((twin.params.copy(), twin_states(learner), stats.copy()))
    return seen


def large_indices(groups, batch, seed):
    """The index arrays [G][B] of LARGE's consecutive updates, every group's row its own: a permutation of the group's N
    rows where B = N, else B rows drawn with repeats."""
    rows = LARGE["per_group"] * LARGE["steps"]
    rng = np.random.default_rng(seed)
    order = []
    for _ in range(LARGE["updates"]):
        if batch == rows:
            order.append(np.stack([rng.permutation(rows) for _ in range(groups)]).astype(np.int64))
        else:
            order.append(rng.integers(0, rows, (groups, batch)).astype(np.int64))
    return order


def large_inputs(index, groups, batch):
    """(spec, twin, flat, hypers' keywords, the index arrays of the updates) of one of LARGE_CASES."""
    spec, twin, flat = update_batch(index, groups, LARGE["per_group"], seed=3, steps=LARGE["steps"])
    return spec, twin, flat, group_hypers(groups), large_indices(groups, batch, 500 + 7 * index + batch)


@functools.lru_cache(maxsize=None)
def large_twin_updates(index, groups, batch):
    spec, twin, flat, hypers, order = large_inputs(index, groups, batch)
    return chained_updates(twin, flat, hypers, order)


def large_update_promises(want, before, hypers):
    """No comparison of a large case is vacuous: every group is taken in every update (flags 0); every group whose
    learning rate is not 0 ends with other parameters than it began with, the one whose is 0 with the same."""
    assert len(want) == LARGE["updates"] and all((stats[:, 7] == 0).all() for _, _, stats in want)
    rates = hypers["learning_rate"]
    assert 0.0 in rates and any(rates)
    for g, rate in enumerate(rates):
        assert (bits(want[-1][0][g]) == bits(before[g])) == (rate == 0), f"group {g} with learning_rate {rate}"
    assert bits(want[0][1]) != bits(want[1][1])  # (the optimizer header and moments the first wrote, the second read)


# ---- the limit: 65535 groups of one row --------------------------------------------------------------------------------
def limit_spec():
    return policy_cases.spec_of(LIMIT_NETWORK)


@functools.lru_cache(maxsize=None)
def limit_parts():
    """(7 packed parameter sets, 5 observation blocks -- one row each: obs, final_obs, action, log_prob, advantage,
    return --, 3 hyper-parameter sets).  Weights and observations are positive, so the one ReLU unit of either net is
    alive and every output depends on both; adam_eps is large, so the first Adam step depends on the gradient's size."""
    from reinfocus_amd.environments import learner

    spec = limit_spec()
    rng = np.random.default_rng(65535)
    params = [np.abs(spec.pack(policy_cases.state_dict(spec, 700 + k))) + F32(0.25 + 0.125 * k) for k in range(LIMIT_PERIODS[0])]
    blocks = []
    for j in range(LIMIT_PERIODS[1]):
        blocks.append(dict(observations=np.array([[0.5 + 0.75 * j]], dtype=F32), final=np.array([[3.0 - 0.5 * j]], dtype=F32),
                           actions=np.array([j % 2], dtype=np.int64), log_probs=np.array([-0.7 + 0.1 * j], dtype=F32),
                           advantages=rng.standard_normal(1).astype(F32), returns=rng.standard_normal(1).astype(F32)))
    hypers = [learner.Hyper(learning_rate=1e-2 / (1 + h), clip_range=0.1 + 0.1 * h, ent_coef=0.01 * (1 + h),
                            vf_coef=0.5 + 0.25 * h, max_grad_norm=(1e6, 0.5, 0.05)[h], beta1=0.9 - 0.1 * h,
                            beta2=0.999 - 0.01 * h, adam_eps=(0.1, 0.3, 1.0)[h], normalize_advantage=h % 2)
              for h in range(LIMIT_PERIODS[2])]
    return params, blocks, hypers


@functools.lru_cache(maxsize=None)
def limit_results():
    """For each of the 105 combinations c (parameter set c % 7, block c % 5, hyper-parameters c % 3), by the existing
    twin functions: the deterministic forward's (actions, values, log_probs, final_values) and the first update's
    (params, state, stats) from a fresh optimizer."""
    from reinfocus_amd.environments import learner, policy

    spec = limit_spec()
    params, blocks, hypers = limit_parts()
    forwards, updates = [], []
    for c in range(105):
        k, j, h = (c % period for period in LIMIT_PERIODS)
        got = policy.policy_numpy(spec, params[k], blocks[j]["observations"], blocks[j]["final"], None, True)
        forwards.append(tuple(got[name] for name in ORDER))
        batch = {key: blocks[j][key] for key in learner.BATCH_KEYS}
        updates.append(learner.ppo_update_numpy(spec, params[k], learner.fresh_state(spec), batch, np.zeros(1, dtype=np.int64),
                                                hypers[h]))
    return forwards, updates


def limit_arrays(groups=LIMIT_GROUPS):
    """What group g gets and what it must give, for g = 0 .. groups - 1: (inputs dict, wanted forward outputs in ORDER,
    wanted (params [G][P], states [G][S], stats [G][8]))."""
    from reinfocus_amd.environments import learner, population

    params, blocks, hypers = limit_parts()
    forwards, updates = limit_results()
    g = np.arange(groups)
    k, j, h, c = g % LIMIT_PERIODS[0], g % LIMIT_PERIODS[1], g % LIMIT_PERIODS[2], g % 105
    inputs = {"params": np.stack(params)[k], "hyper": population.hyper_records(hypers)[h]}
    for key in ("observations", "final") + tuple(k for k in learner.BATCH_KEYS if k != "observations"):
        inputs[key] = np.concatenate([block[key] for block in blocks])[j]
    wanted_forward = tuple(np.concatenate([forward[i] for forward in forwards])[c] for i in range(len(ORDER)))
    wanted_update = tuple(np.stack([update[i] for update in updates])[c] for i in range(3))
    return inputs, wanted_forward, wanted_update


def isolation_inputs():
    """Four groups; group 1's minibatch holds an index past its rows, group 2's a row whose observation has a NaN."""
    index, groups, per_group, batch = 0, 4, 3, 5
    spec, twin, flat = update_batch(index, groups, per_group, seed=5)
    rows = per_group * T
    order = update_permutations(groups, rows, 3)[0][:, :batch].copy()
    order[1, 2] = rows  # (a row of the NEXT group: in range of the whole array, out of range of the group)
    flat["observations"][2 * rows + order[2, 1], 1] = np.nan
    return spec, twin, flat, order


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
def e2e_permutations(iteration):
    rows = E2E["steps"] * E2E["envs"] // E2E["groups"]
    rng = np.random.default_rng(800 + iteration)
    return np.stack([np.stack([rng.permutation(rows) for _ in range(E2E["groups"])])
                     for _ in range(E2E["epochs"])]).astype(np.int64)


def e2e_hypers():
    return dict(learning_rate=[1e-2, 3e-3, 0.0], ent_coef=[0.0, 0.01, 0.02], clip_range=0.2)


def e2e_runs(rollout, policy, learner, reset, unwrap, wrap):
    obs = reset()
    seen = []
    for iteration in range(E2E["iterations"]):
        rollout.start(obs if iteration == 0 else None)
        rollout.collect(policy)
        record = policy_cases.slabs_of(rollout, unwrap)
        record["stats"] = unwrap(learner.train(rollout, E2E["epochs"], E2E["batch"],
                                               permutations=wrap(e2e_permutations(iteration))))
        record["params"] = unwrap(policy.params)
        seen.append(record)
    return seen


def e2e_env(device_form):
    from reinfocus_amd.environments import harness

    if device_form:
        return harness.DeviceVectorDiscreteSteps(num_envs=E2E["envs"], device_initializer=True, episode_records=True,
                                                 **rollout_cases.ENV_KW)
    return harness.VectorDiscreteSteps(num_envs=E2E["envs"], episode_records=True, **rollout_cases.ENV_KW)


def e2e_spec():
    from reinfocus_amd.environments import policy

    return policy.MlpPolicySpec(4, 13, pi=(6,), vf=(5, 7), activation="tanh")


@functools.lru_cache(maxsize=None)
def e2e_twin_runs():
    from reinfocus_amd.environments import harness

    env = e2e_env(False)
    try:
        spec = e2e_spec()
        policy = harness.PopulationPolicy(spec, E2E["groups"], seeds_of(E2E["groups"]))
        for g, state in enumerate(group_states(spec, E2E["groups"], 500)):
            policy.load_state_dict(state, group=g)
        learner = harness.PopulationLearner(policy, **e2e_hypers())
        rollout = harness.Rollout(env, E2E["steps"], GAMMA, GAE_LAMBDA)
        runs = e2e_runs(rollout, policy, learner, lambda: env.reset()[0], np.array, lambda a: a)
        return runs, policy.rng_state(), twin_states(learner)
    finally:
        env.close()


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
def _guarded(torch, n):
    whole = {name: torch.full((n + 2,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
             for name in ("log_probs", "values", "final_values")}
    whole["actions"] = torch.full((n + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
    return whole, {name: tensor[1:n + 1] for name, tensor in whole.items()}


_untouched = policy_cases._untouched
ORDER = ("actions", "values", "log_probs", "final_values")


def _table(torch, groups, consumed=0):
    """The device table of the generators' words (advanced by `consumed` where the case passes consumed = 0)."""
    from reinfocus_amd.environments import policy

    words = []
    for state in advanced_states(groups, consumed):
        generator = np.random.PCG64DXSM()
        generator.state = state
        words.append(policy.generator_words(generator))
    return torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).cuda()


def _forward(torch, ctx, spec, groups, per_group, params, obs, final_obs, table, consumed, flags, out, changed=()):
    a = dict(desc=spec.desc(), groups=groups, per_group=per_group, params=params.data_ptr(), obs=obs.data_ptr(),
             final_obs=None if final_obs is None else final_obs.data_ptr(),
             gens=None if table is None else table.data_ptr(), consumed=consumed, flags=flags)
    a.update({name: None if tensor is None else tensor.data_ptr() for name, tensor in out.items()})
    a.update(changed)
    ctx.policy_forward_grouped(a["desc"], a["groups"], a["per_group"], a["params"], a["obs"], a["final_obs"], a["gens"],
                               a["consumed"], a["flags"], a["actions"], a["log_probs"], a["values"], a["final_values"], None,
                               torch.cuda.current_stream().cuda_stream)


def forward_case(torch, ctx, index, groups, per_group):
    """rf_policy_forward_grouped against the twin population as bytes: sampled at both draw counts, deterministic,
    values only; every output a slice of a larger slab whose guard rows keep their sentinel; where G > 1 also against G
    stand-alone rf_policy_forward calls, and every group's outputs differ from what group 0's parameters give."""
    from reinfocus_amd.environments import policy

    spec, twin = twin_policy(index, groups)
    n = groups * per_group
    obs_h, final_h = forward_inputs(index, groups, per_group)
    params, obs, final_obs = (torch.from_numpy(a).cuda() for a in (twin.params, obs_h, final_h))
    table = _table(torch, groups)
    for consumed, deterministic in ((CONSUMED[0], False), (CONSUMED[1], False), (0, True)):
        want, _ = wanted_forward(index, groups, per_group, consumed, deterministic)
        whole, out = _guarded(torch, n)
        _forward(torch, ctx, spec, groups, per_group, params, obs, final_obs, table, consumed,
                 policy.DETERMINISTIC if deterministic else 0, out)
        torch.cuda.synchronize()
        for name, wanted in zip(ORDER, want):
            assert bits(out[name].cpu().numpy()) == bits(wanted), f"consumed {consumed}, {deterministic}: {name} differ"
            assert _untouched(whole[name][0]) and _untouched(whole[name][n + 1]), f"a guard row of {name} was written"
    assert np.isnan(want[3]).any() and not np.isnan(want[3]).all()  # (NaN-led final_obs rows among live ones)
    whole, out = _guarded(torch, n)
    out.update(actions=None, log_probs=None)
    _forward(torch, ctx, spec, groups, per_group, params, obs, final_obs, None, 0, 0, out)
    torch.cuda.synchronize()
    assert bits(out["values"].cpu().numpy()) == bits(want[1]) and bits(out["final_values"].cpu().numpy()) == bits(want[3])
    assert _untouched(whole["actions"]) and _untouched(whole["log_probs"])
    if groups > 1:
        # the same device, G stand-alone launches over the groups' rows: the bytes of the grouped launch
        consumed = CONSUMED[1]
        want, _ = wanted_forward(index, groups, per_group, consumed, False)
        alone = {name: torch.zeros(n, dtype=torch.int64 if name == "actions" else torch.float32, device="cuda")
                 for name in ORDER}
        stream = torch.cuda.current_stream().cuda_stream
        for g, state in enumerate(advanced_states(groups, consumed)):
            generator = np.random.PCG64DXSM()
            generator.state = state
            rows = slice(g * per_group, (g + 1) * per_group)
            ctx.policy_forward(spec.desc(), params[g].data_ptr(), per_group, obs[rows].data_ptr(), final_obs[rows].data_ptr(),
                               policy.generator_words(generator), 0, alone["actions"][rows].data_ptr(),
                               alone["log_probs"][rows].data_ptr(), alone["values"][rows].data_ptr(),
                               alone["final_values"][rows].data_ptr(), None, stream)
        torch.cuda.synchronize()
        for name, wanted in zip(ORDER, want):
            assert bits(alone[name].cpu().numpy()) == bits(wanted), f"stand-alone launches: {name} differ"
        # a forward that read group 0's parameters everywhere would give other values in every later group
        everywhere = policy.policy_numpy(spec, twin.params[0], obs_h, values_only=True)["values"]
        for g in range(1, groups):
            rows = slice(g * per_group, (g + 1) * per_group)
            if per_group == 1 and not np.isfinite(everywhere[rows]).all():
                continue  # (a group's only row is a hostile one whose value is NaN or infinite under any parameters)
            assert bits(everywhere[rows]) != bits(want[1][rows]), f"group {g} does not tell its parameters from group 0's"


class _Learner:
    """Device copies of a twin population's parameters and batch, fresh optimizer states, and rf_ppo_update_grouped."""

    def __init__(self, torch, ctx, spec, twin, flat, per_group, hypers, batch_most, steps=T, guarded=False):
        """twin: a PopulationPolicy, or the packed parameters [G][P] themselves; hypers: learner.Hyper per group, or the
        packed records.  guarded: parameters and optimizer states lie between guard rows of one group's size, and the
        workspace has exactly rf_ppo_grouped_workspace_size's bytes between guard floats; update() checks them all."""
        from reinfocus_amd.environments import learner, population

        params = twin if isinstance(twin, np.ndarray) else twin.params
        self.torch, self.ctx, self.spec, self.groups, self.per_group = torch, ctx, spec, params.shape[0], per_group
        self.steps, self.whole = steps, []
        self.params = self._slab(params.shape[1] if guarded else 0, params.reshape(-1))
        state_bytes = ctx.ppo_grouped_state_size(spec.desc(), self.groups, per_group)
        assert state_bytes == self.groups * 4 * (learner.STATE_HEADER + 2 * spec.size)
        self.state = self._slab(state_bytes // 4 // self.groups if guarded else 0, np.zeros(state_bytes // 4, dtype=F32))
        size = ctx.ppo_grouped_workspace_size(spec.desc(), self.groups, per_group, steps, batch_most)
        assert size == self.groups * ctx.ppo_workspace_size(spec.desc(), batch_most) and size > 0
        self.workspace = self._slab(16 if guarded else 0, np.zeros(size // 4, dtype=F32))
        self.params = self.params.view(self.groups, -1)
        self.flat = {key: torch.from_numpy(np.ascontiguousarray(flat[key])).cuda() for key in learner.BATCH_KEYS}
        records = hypers if isinstance(hypers, np.ndarray) else population.hyper_records(hypers)
        self.hyper = torch.from_numpy(records.view(np.float64).copy()).cuda()
        self.stats = torch.full((self.groups + 2, 8), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)

    def _slab(self, guard, array):
        whole = self.torch.full((array.size + 2 * guard,), SENTINEL, dtype=self.torch.int32, device="cuda").view(
            self.torch.float32)
        view = whole[guard:guard + array.size]
        view.copy_(self.torch.from_numpy(np.ascontiguousarray(array, dtype=F32)))
        if guard:
            self.whole.append((whole, guard))
        return view

    def guards_kept(self):
        return all(_untouched(whole[:guard]) and _untouched(whole[-guard:]) for whole, guard in self.whole)

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
        self.ctx.ppo_update_grouped(a["desc"], a["groups"], a["per_group"], a["steps"], a["hyper"], a["params"], a["state"],
                                    a["workspace"], a["obs"], a["actions"], a["log_probs"], a["advantages"], a["returns"],
                                    a["batch"], a["index"], a["stats"], self.torch.cuda.current_stream().cuda_stream)
        self.torch.cuda.synchronize()
        assert _untouched(self.stats[0]) and _untouched(self.stats[self.groups + 1]), "a guard row of the stats was written"
        assert self.guards_kept(), "a guard of the parameters, the states or the workspace was written"
        return (self.params.cpu().numpy(), self.state.cpu().numpy().reshape(self.groups, -1),
                self.stats[1:self.groups + 1].cpu().numpy())


def _same_update(got, want, what):
    for name, x, y in zip(("params", "states", "stats"), got, want):
        assert bits(x) == bits(y), f"{what}: {name} differ"


def update_case(torch, ctx, index, batch, per_group):
    """rf_ppo_update_grouped against the twin population over two epochs of chained updates (the last minibatch of an
    epoch is short); group 1 has learning_rate 0: its parameters keep their bytes while its Adam moments move."""
    from reinfocus_amd.environments import harness, learner

    want = twin_updates(index, batch, per_group)
    spec, twin, flat = update_batch(index, UPDATE_GROUPS, per_group)
    hypers = harness.PopulationLearner(twin, **group_hypers(UPDATE_GROUPS)).hypers()
    device = _Learner(torch, ctx, spec, twin, flat, per_group, hypers, batch)
    before = twin.params.copy()
    rows = minibatches(update_permutations(UPDATE_GROUPS, per_group * T, 7 + batch), batch)
    assert len(rows) >= 3 and rows[-1].shape[1] < batch
    for update, index_rows in enumerate(rows):
        _same_update(device.update(index_rows), want[update], f"update {update}")
    params, states, stats = want[-1]
    assert (stats[:, 7] == 0).all() and bits(params[1]) == bits(before[1]) and bits(params[0]) != bits(before[0])
    assert np.abs(states[1][learner.STATE_HEADER:]).max() > 0  # (m and v of the group with learning_rate 0 moved)


def wide_update_case(torch, ctx):
    """rf_ppo_update_grouped at G = 64 on ppo_tuned.yml's first shape (WIDE_UPDATE) against the twin population over two
    epochs of chained updates: every group's parameters, state and stats as bytes after each; what the twin's results
    promise (group 31 flagged and kept in two updates, group 1 never moving) is wide_update_promises'."""
    want = wide_twin_updates()
    spec, twin, flat, hypers, order = wide_update_inputs()
    w = WIDE_UPDATE
    from reinfocus_amd.environments import harness

    device = _Learner(torch, ctx, spec, twin, flat, w["per_group"], harness.PopulationLearner(twin, **hypers).hypers(),
                      w["batch"], steps=w["steps"], guarded=True)
    for update, index_rows in enumerate(order):
        got = device.update(index_rows)
        for g in (0, w["nan_group"] - 1, w["nan_group"], w["nan_group"] + 1, w["groups"] - 1):
            _same_update(tuple(x[g] for x in got), tuple(x[g] for x in want[update]), f"update {update}, group {g}")
        _same_update(got, want[update], f"update {update}")
    wide_update_promises(want, twin.params)


def large_update_case(torch, ctx, index, groups, batch, cases=None):
    """The grouped update on m = 8, T = 128 at B = `batch`, index [G][B] with rows of its own per group, against the twin
    population over LARGE's consecutive updates: parameters, optimizer states and stats of every group as bytes, parameters
    and states between guard rows, the workspace of exactly the grouped size function's bytes between guard floats.  For
    LARGE_ALONE also G stand-alone ungrouped launches on contiguous copies of the groups' slices.  `cases`: this module, or
    the gSDE population's with the same names."""
    from reinfocus_amd.environments import learner

    cases = cases or sys.modules[__name__]
    spec, twin, flat, keywords, order = cases.large_inputs(index, groups, batch)
    want = cases.large_twin_updates(index, groups, batch)
    assert all(rows.shape == (groups, batch) for rows in order)
    hypers = chained_hypers(twin, keywords)
    per_group, steps = LARGE["per_group"], LARGE["steps"]
    device = cases._Learner(torch, ctx, spec, twin, flat, per_group, hypers, batch, steps=steps, guarded=True)
    for update, index_rows in enumerate(order):
        got = device.update(index_rows)
        for g in range(groups):
            _same_update(tuple(x[g] for x in got), tuple(x[g] for x in want[update]), f"update {update}, group {g}")
    large_update_promises(want, twin.params, keywords)
    if (index, groups, batch) != cases.LARGE_ALONE:
        return
    update_alone, size_alone = (getattr(ctx, name) for name in cases.ALONE_ENTRIES)
    rows = per_group * steps
    stream = torch.cuda.current_stream().cuda_stream
    for g in range(groups):
        piece = {key: torch.from_numpy(np.ascontiguousarray(flat[key][g * rows:(g + 1) * rows])).cuda()
                 for key in learner.BATCH_KEYS}
        params = torch.from_numpy(twin.params[g].copy()).cuda()
        state = torch.from_numpy(learner.fresh_state(spec)).cuda()
        workspace = torch.zeros(size_alone(spec.desc(), batch) // 4, dtype=torch.float32, device="cuda")
        stats = torch.zeros(8, dtype=torch.float32, device="cuda")
        for update, index_rows in enumerate(order):
            chosen = torch.from_numpy(np.ascontiguousarray(index_rows[g])).cuda()
            update_alone(spec.desc(), tuple(hypers[g]), params.data_ptr(), state.data_ptr(), workspace.data_ptr(), rows,
                         piece["observations"].data_ptr(), piece["actions"].data_ptr(), piece["log_probs"].data_ptr(),
                         piece["advantages"].data_ptr(), piece["returns"].data_ptr(), batch, chosen.data_ptr(),
                         stats.data_ptr(), stream)
            torch.cuda.synchronize()
            _same_update((params.cpu().numpy(), state.cpu().numpy(), stats.cpu().numpy()),
                         tuple(x[g] for x in want[update]), f"stand-alone group {g}, update {update}")


def chained_hypers(twin, keywords):
    """learner.Hyper per group of the keywords, without touching the twin."""
    from reinfocus_amd.environments import harness

    return harness.PopulationLearner(twin, **keywords).hypers()


def limit_case(torch, ctx):
    """RF_POPULATION_MAX_GROUPS groups of one row on the least network: one deterministic forward with values and final
    values, and one grouped update of fresh optimizers, every output byte of every group against the result of its
    combination (limit_arrays).  Then 65536 groups: refused by both entry points and both size functions, nothing written."""
    from reinfocus_amd.environments import learner, policy

    spec, groups = limit_spec(), LIMIT_GROUPS
    inputs, wanted_forward, wanted_update = limit_arrays()
    params, obs, final_obs = (torch.from_numpy(inputs[key]).cuda() for key in ("params", "observations", "final"))
    whole, out = _guarded(torch, groups)
    _forward(torch, ctx, spec, groups, 1, params, obs, final_obs, None, 0, policy.DETERMINISTIC, out)
    torch.cuda.synchronize()
    for name, wanted in zip(ORDER, wanted_forward):
        got = out[name].cpu().numpy()
        differ = np.flatnonzero((got.view(np.uint8).reshape(groups, -1) != wanted.view(np.uint8).reshape(groups, -1)).any(axis=1))
        assert differ.size == 0, f"{name} differ in {differ.size} groups, first {differ[:4]}"
        assert _untouched(whole[name][0]) and _untouched(whole[name][groups + 1]), f"a guard row of {name} was written"
    flat = {key: inputs[key] for key in learner.BATCH_KEYS}
    device = _Learner(torch, ctx, spec, inputs["params"], flat, 1, inputs["hyper"], 1, steps=1, guarded=True)
    got = device.update(np.zeros((groups, 1), dtype=np.int64))
    for name, x, y in zip(("params", "states", "stats"), got, wanted_update):
        differ = np.flatnonzero((x.view(np.uint32) != y.view(np.uint32)).any(axis=1))
        assert differ.size == 0, f"{name} differ in {differ.size} groups, first {differ[:4]}"
    # one group more
    kept = [t.clone() for t in (device.params, device.state, device.stats)]
    many = groups + 1
    assert ctx.ppo_grouped_state_size(spec.desc(), many, 1) == 0 == ctx.ppo_grouped_workspace_size(spec.desc(), many, 1, 1, 1)
    for call in (lambda: device.update(np.zeros((groups, 1), dtype=np.int64), dict(groups=many)),
                 lambda: _forward(torch, ctx, spec, many, 1, params, obs, final_obs, None, 0, policy.DETERMINISTIC, out)):
        try:
            call()
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert "must be in 1" in str(caught), str(caught)
        else:
            raise AssertionError("65536 groups were taken")
    torch.cuda.synchronize()
    for tensor, copy in zip((device.params, device.state, device.stats), kept):
        assert torch.equal(tensor.view(torch.int32), copy.view(torch.int32)), "a refused update wrote an output"
    for name, wanted in zip(ORDER, wanted_forward):
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
    """Each refusal of the two entry points leaves every output as it was."""
    from reinfocus_amd.environments import harness

    index, groups, per_group = 0, 5, 3
    spec, twin = twin_policy(index, groups)
    n = groups * per_group
    obs_h, final_h = forward_inputs(index, groups, per_group)
    params, obs, final_obs = (torch.from_numpy(a).cuda() for a in (twin.params, obs_h, final_h))
    table = _table(torch, groups)
    whole, out = _guarded(torch, n)

    def refused(match, **changed):
        try:
            _forward(torch, ctx, spec, groups, per_group, params, obs, final_obs, table, 0, 0, out, changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        torch.cuda.synchronize()
        assert all(_untouched(w) for w in whole.values()), f"an output was written ({match})"

    host = np.zeros((n + 2, spec.obs_width), dtype=np.float32)
    refused("d_obs is not device memory", obs=host.ctypes.data)
    refused("d_values is not device memory", values=host.ctypes.data)
    refused("d_gens is not device memory", gens=np.zeros((groups, 4), dtype=np.uint64).ctypes.data)
    refused("needs d_gens", gens=None)
    refused("must be in 1", groups=0)
    refused("must be in 1", per_group=0)
    refused("must be in 1", groups=65536)
    refused("not aligned", gens=table.data_ptr() + 4)
    refused("d_values overlaps d_log_probs", values=out["log_probs"].data_ptr())
    refused("d_values overlaps d_obs", values=obs.data_ptr())
    refused("d_actions overlaps d_gens", actions=table.data_ptr())
    refused("outside the limits", desc=(0,) + tuple(spec.desc()[1:]))
    refused("unknown flags", flags=2)
    _forward(torch, ctx, spec, groups, per_group, params, obs, final_obs, table, 0, 0, out)
    torch.cuda.synchronize()
    want, _ = wanted_forward(index, groups, per_group, 0, False)
    for name, wanted in zip(ORDER, want):
        assert bits(out[name].cpu().numpy()) == bits(wanted), name

    spec, twin, flat = update_batch(0, UPDATE_GROUPS, 3)
    hypers = harness.PopulationLearner(twin, **group_hypers(UPDATE_GROUPS)).hypers()
    device = _Learner(torch, ctx, spec, twin, flat, 3, hypers, 5)
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
    refused_update("d_hyper is not device memory", hyper=np.zeros(7 * UPDATE_GROUPS).ctypes.data)
    refused_update("must be in 1", groups=0)
    refused_update("must be in 1", per_group=0)
    refused_update("is not in 1", index=np.zeros((UPDATE_GROUPS, 13), dtype=np.int64))  # (B > m T)
    refused_update("d_stats overlaps d_params", stats=device.params.data_ptr())
    refused_update("d_workspace overlaps d_state", workspace=device.state.data_ptr())
    refused_update("not aligned", state=device.state.data_ptr() + 4)
    _same_update(device.update(rows), _first_update(spec, twin, flat, rows), "after the refusals")


def _first_update(spec, twin, flat, rows):
    from reinfocus_amd.environments import harness

    learner = harness.PopulationLearner(twin, **group_hypers(UPDATE_GROUPS))
    stats = learner.update(flat, rows)
    return twin.params.copy(), twin_states(learner), stats


def _cuda_states(torch, states):
    return {key: torch.from_numpy(np.ascontiguousarray(value)).cuda() for key, value in states.items()}


def one_group_case(torch):
    """G = 1: outputs, parameters and optimizer state after 3 chained updates and rng_state() equal the ungrouped
    DevicePolicy / DeviceLearner bit for bit."""
    from reinfocus_amd.environments import harness

    n = 11
    env = harness.DeviceVectorDiscreteSteps(num_envs=n, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        spec = e2e_spec()
        state = _cuda_states(torch, policy_cases.state_dict(spec, 3))
        single = harness.DevicePolicy(env, spec, 77)
        grouped = harness.DevicePopulationPolicy(env, spec, 1, [77])
        single.load_state_dict(state)
        grouped.load_state_dict(state)
        assert torch.equal(grouped.params[0], single.params)
        rng = np.random.default_rng(2)
        obs = torch.from_numpy(rng.standard_normal((n, 4)).astype(F32)).cuda()
        for deterministic in (False, True, False):
            ours = [t.clone() for t in grouped.act(obs, None, deterministic)[:3]]
            theirs = single.act(obs, None, deterministic)[:3]
            for x, y in zip(ours, theirs):
                assert bits(x.cpu().numpy()) == bits(y.cpu().numpy())
            assert grouped.rng_state() == [single.rng_state()]
        assert bits(grouped.values(obs).cpu().numpy()) == bits(single.values(obs).cpu().numpy())
        total = n * T
        flat = {"observations": rng.standard_normal((total, 4)).astype(F32), "actions": rng.integers(0, 13, total),
                "log_probs": (-2.5 + 0.1 * rng.standard_normal(total)).astype(F32),
                "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32)}
        flat = _cuda_states(torch, flat)
        kw = dict(learning_rate=1e-2, ent_coef=0.01)
        one, many = harness.DeviceLearner(single, **kw), harness.DevicePopulationLearner(grouped, **kw)
        for update in range(3):
            index = torch.from_numpy(rng.permutation(total)[:13 - update].astype(np.int64)).cuda()
            theirs = one.update(flat, index)
            ours = many.update(flat, index[None, :].contiguous())
            assert bits(ours[0].cpu().numpy()) == bits(theirs.cpu().numpy()), f"update {update}: stats differ"
        assert bits(grouped.params[0].cpu().numpy()) == bits(single.params.cpu().numpy())
        assert bits(many.state[0].cpu().numpy()) == bits(one.state.cpu().numpy())
        assert many.state_dict()["step"] == [3]
    finally:
        env.close()


def end_to_end_case(torch):
    from reinfocus_amd.environments import harness

    want, want_rng, want_states = e2e_twin_runs()
    env = e2e_env(True)
    try:
        spec = e2e_spec()
        policy = harness.DevicePopulationPolicy(env, spec, E2E["groups"], seeds_of(E2E["groups"]))
        for g, state in enumerate(group_states(spec, E2E["groups"], 500)):
            policy.load_state_dict(_cuda_states(torch, state), group=g)
        learner = harness.DevicePopulationLearner(policy, **e2e_hypers())
        rollout = harness.DeviceRollout(env, E2E["steps"], GAMMA, GAE_LAMBDA)
        got = e2e_runs(rollout, policy, learner, lambda: env.reset_tensors()[0], lambda t: t.cpu().numpy(),
                       lambda a: torch.from_numpy(a).cuda())
        policy_cases.same_runs(got, want)
        assert env.device_fault() is None
        assert policy.rng_state() == want_rng
        assert bits(learner.state.cpu().numpy()) == bits(want_states)
        assert want[0]["stats"].shape == (E2E["epochs"] * 4, E2E["groups"], 8) and (want[1]["stats"][:, :, 7] == 0).all()
        assert bits(want[0]["params"][0]) != bits(want[1]["params"][0])
        assert np.concatenate([run["truncated"] for run in want]).any(), "no environment ended"
        # resume: a second learner from state_dict() goes on bit for bit; its own permutations keep to the device
        kept, kept_params = learner.state_dict(), policy.params.clone()
        order = torch.from_numpy(e2e_permutations(9)).cuda()
        straight = learner.train(rollout, E2E["epochs"], E2E["batch"], permutations=order).clone()
        after = policy.params.clone()
        policy.params.copy_(kept_params)
        second = harness.DevicePopulationLearner(policy, **e2e_hypers())
        second.load_state_dict(kept)
        again = second.train(rollout, E2E["epochs"], E2E["batch"], permutations=order)
        assert torch.equal(again.view(torch.int32), straight.view(torch.int32)) and torch.equal(policy.params, after)
        assert torch.equal(second.state.view(torch.int32), learner.state.view(torch.int32))
        drawn = second.train(rollout, 1, E2E["batch"], generator=torch.Generator(device="cuda").manual_seed(1))
        assert tuple(drawn.shape) == (4, E2E["groups"], 8) and (drawn[:, :, 7] == 0).all()
    finally:
        env.close()


def surface_case(torch):
    """What the classes refuse, each with a message, the tensors unchanged afterwards and no draw consumed."""
    from reinfocus_amd.environments import harness

    env = e2e_env(True)
    jumps = harness.DeviceVectorContinuousJumps(num_envs=6, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        spec = e2e_spec()

        def raises(kind, match, call):
            try:
                call()
            except kind as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"not refused ({match})")

        raises(ValueError, "not divisible", lambda: harness.DevicePopulationPolicy(env, spec, 4, [1, 2, 3, 4]))
        raises(ValueError, "one seed per group", lambda: harness.DevicePopulationPolicy(env, spec, 3, [1, 2]))
        raises(ValueError, "one seed per group", lambda: harness.DevicePopulationPolicy(env, spec, 3, [1, 2, 3, 4]))
        raises(ValueError, "one seed per group", lambda: harness.DevicePopulationPolicy(env, spec, 3, 7))
        raises(ValueError, "out of scope", lambda: harness.DevicePopulationPolicy(jumps, spec, 3, [1, 2, 3]))
        policy = harness.DevicePopulationPolicy(env, spec, 3, [1, 2, 3])
        raises(TypeError, "DevicePopulationPolicy", lambda: harness.DevicePopulationLearner(harness.DevicePolicy(env, spec, 0)))
        raises(TypeError, "DevicePolicy", lambda: harness.DeviceLearner(policy))
        before = policy.rng_state()
        obs = torch.zeros((6, 4), dtype=torch.float32, device="cuda")
        raises(ValueError, "rows", lambda: policy.act(obs[:5].contiguous()))
        raises(ValueError, "not torch.float32", lambda: policy.act(obs.double()))
        raises(TypeError, "torch.Tensor", lambda: policy.act(obs.cpu().numpy()))
        slab = torch.full((8,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        actions = torch.full((6,), SENTINEL64, dtype=torch.int64, device="cuda")
        raises(AssertionError, "overlaps", lambda: policy.act(obs, out=(actions, slab[1:7], slab[2:8], None)))
        raises(ValueError, "out values", lambda: policy.act(obs, out=(actions, slab[1:6], slab[2:8], None)))
        torch.cuda.synchronize()
        assert _untouched(slab) and _untouched(actions) and policy.rng_state() == before
        learner = harness.DevicePopulationLearner(policy)
        raises(ValueError, "entries", lambda: setattr(learner, "learning_rate", [1e-3, 1e-3]) or learner.hypers())
        learner.learning_rate = 1e-3
        host_env = e2e_env(False)
        try:
            twin = harness.PopulationPolicy(spec, 3, [1, 2, 3])
            host_rollout = harness.Rollout(host_env, 2)
            host_rollout.start(host_env.reset()[0])
            host_rollout.collect(twin)
            raises(ValueError, "the host", lambda: learner.train(host_rollout, 1, 2))
        finally:
            host_env.close()
        rollout = harness.DeviceRollout(env, 2)
        rollout.start(env.reset_tensors()[0])
        rollout.collect(policy)
        kept = policy.params.clone()
        raises(ValueError, "more than the 4 rows", lambda: learner.train(rollout, 1, 5))
        flat = rollout.flat()
        raises(ValueError, "index is", lambda: learner.update(flat, torch.zeros((3, 5), dtype=torch.int64, device="cuda")))
        raises(ValueError, "index is", lambda: learner.update(flat, torch.zeros((2, 4), dtype=torch.int64, device="cuda")))
        raises(ValueError, "index is", lambda: learner.update(flat, torch.zeros((3, 4), dtype=torch.int32, device="cuda")))
        torch.cuda.synchronize()
        assert torch.equal(policy.params, kept)
        stats = learner.train(rollout, 1, 4)
        assert tuple(stats.shape) == (1, 3, 8)
    finally:
        env.close()
        jumps.close()


def sharded_case(torch):
    from reinfocus_amd.environments import harness

    env = harness.ShardedVectorDiscreteSteps(num_envs=6, devices=[0], frame_height=16, samples_per_pixel=1, seed=1)
    try:
        try:
            harness.DevicePopulationPolicy(env, e2e_spec(), 3, [1, 2, 3])
        except ValueError as caught:
            assert "tensors" in str(caught), str(caught)
        else:
            raise AssertionError("a sharded environment was not refused")
    finally:
        env.close()


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
                with record.case(f"forward/{index}/{groups}/{per_group}"):
                    forward_case(torch, ctx, index, groups, per_group)
        for batch, per_group in UPDATE_SHAPES:
            with record.case(f"update/{index}/{batch}"):
                update_case(torch, ctx, index, batch, per_group)
    for index, groups, per_group in WIDE_FORWARD:
        with record.case(f"forward/{index}/{groups}/{per_group}"):
            forward_case(torch, ctx, index, groups, per_group)
    with record.case("update/wide"):
        wide_update_case(torch, ctx)
    for index, groups, batch in LARGE_CASES:
        with record.case(f"update/large/{index}/{groups}/{batch}"):
            large_update_case(torch, ctx, index, groups, batch)
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
    with record.case("sharded"):
        sharded_case(torch)
    with record.case("finished"):
        pass


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    run_cases(sys.argv[1])
