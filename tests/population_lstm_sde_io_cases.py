"""TEST INFRASTRUCTURE: what tests/test_population_lstm_sde_logic.py and tests/test_gpu_population_lstm_sde.py share -- the
networks, the group shapes, the numpy twins' results (computed once and shared) -- and the child process of the GPU file.

As tests/population_lstm_io_cases.py: everything that needs torch and the library together runs in one fresh process that
imports torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.population_lstm_sde_io_cases <results.jsonl>
"""

import ctypes
import functools
import os
import sys

import numpy as np

from tests import lstm_learner_io_cases as lstm_learner_cases
from tests import lstm_sde_io_cases as lsde_cases
from tests import policy_io_cases as policy_cases
from tests import population_io_cases as population_cases
from tests import population_lstm_io_cases as lstm_pop
from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = policy_cases.bits
SENTINEL = policy_cases.SENTINEL
GAMMA, GAE_LAMBDA = rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA
seeds_of, group_hypers, twin_states = population_cases.seeds_of, population_cases.group_hypers, population_cases.twin_states
group_starts, group_slices, firsts_of, hypers_of = (lstm_pop.group_starts, lstm_pop.group_slices, lstm_pop.firsts_of,
                                                    lstm_pop.hypers_of)
critic_name = lstm_pop.critic_name
OUTPUTS, PI_OUTPUTS = lsde_cases.OUTPUTS, lsde_cases.PI_OUTPUTS

# lstm_sde_io_cases.NETWORKS: the least network (D = H = L = 1) and the one whose widths are no multiple of a wave or of
# a tile (H = 65, L = 65); SMALL (H = 16) carries the sequence structures and the width, UNTUNED (H = 256) the widest cell
NETS = (0, 3)
SMALL, UNTUNED = lsde_cases.SMALL, lsde_cases.UNTUNED
CRITICS = (True, False)  # enable_critic_lstm
GROUPS = (1, 3)
PER_GROUP = (3, 8, 11)  # a group border inside what would be an ungrouped tile; exactly one tile; a ragged second tile
STRIDE = (3, 3)  # (G, m) of the state-plane stride case
NOISE = dict(groups=3, per_group=3, consumed=(0, 2 ** 32 + 5, 7), masks=(None, (1, 0, 1), (0, 0, 0)))
UPDATE = dict(groups=3, steps=4, per_group=3, firsts=(0, 7, 11), batches=(5, 12), updates=2)
# T = 17, m = 4 (lstm_learner_io_cases.LIMIT_LAYOUTS): sequences of 1, 8, 9, 16 and 17 rows, the groups wrap at different rows
DEPTH = dict(index=SMALL, layout="depth/0/65", firsts=(0, 5, 30), updates=1)
LIMIT = dict(index=UNTUNED, groups=2, steps=3, per_group=2, batch=6, firsts=(0, 4))
WIDE_UPDATE = dict(index=SMALL, groups=64, steps=8, per_group=8, batch=8)
E2E = dict(groups=3, per_group=3, steps=4, epochs=2, batch=5, iterations=2, freqs=(-1, 2, 1), log_std=(-1.0, -0.5, 0.25))
# the group limit: RF_POPULATION_MAX_GROUPS groups of m = T = B = 1 on the least network, by population_io_cases' periodic
# scheme: group g has parameter set g % 7 (its own log_std), input block g % 5 (its state on level g % 5), hyper-parameter
# set g % 3 and theta level g % 3; a noise reset draws from generator g % 11 after LIMIT_CONSUMED[g % 3] draws and skips
# the groups with g % 5 = 2; firsts[g] = 1 = N (outside) where g % 11 = 5
LIMIT_GROUPS, LIMIT_PERIODS, LIMIT_GENERATORS = 65535, (7, 5, 3), 11
LIMIT_STARTS = (0, 0, 1, 0, 255)
LIMIT_CONSUMED = (0, 2 ** 32 + 5, 7)
LIMIT_THETA = (-0.75, 0.5, 1.25)
LIMIT_UNSELECTED = (5, 2)  # g % 5 == 2
LIMIT_OUTSIDE = (11, 5)  # g % 11 == 5
INVALID = 1  # RF_PPO_INVALID
ENTRY_POINTS = sorted(["rf_lstm_sde_noise_reset_grouped", "rf_lstm_sde_forward_grouped", "rf_lstm_sde_grouped_state_size",
                       "rf_lstm_sde_grouped_workspace_size", "rf_lstm_sde_update_grouped"])


def spec_of(index, critic_lstm, log_std_init=0.0, width=None):
    from reinfocus_amd.environments import lstm_sde

    obs_width, hidden, pi, vf, activation = lsde_cases.NETWORKS[index]
    return lstm_sde.LstmSdePolicySpec(obs_width if width is None else width, lstm_hidden=hidden, pi=pi, vf=vf,
                                      activation=activation, log_std_init=log_std_init, enable_critic_lstm=critic_lstm)


def group_params(spec, groups, base):
    """float32 [G][P + L]: every group its own parameters and its own log_std (hostile where L > 1: rows of -100, 0, +3)."""
    return np.stack([spec.pack(lsde_cases.state_dict(spec, base + 17 * g, hostile=spec.latent > 1 and g % 2 == 0))
                     for g in range(groups)])


def twin_policy(index, critic_lstm, groups, per_group, base=100):
    from reinfocus_amd.environments import harness

    spec = spec_of(index, critic_lstm)
    twin = harness.LstmSdePopulationPolicy(spec, groups, seeds_of(groups), num_envs=groups * per_group)
    twin.params[...] = group_params(spec, groups, base + index)
    return spec, twin


def fresh_twin(spec, twin):
    """A copy of the twin population (a cached one is never changed)."""
    from reinfocus_amd.environments import harness

    copy = harness.LstmSdePopulationPolicy(spec, twin.groups, seeds_of(twin.groups), num_envs=twin.num_envs)
    copy.params[...] = twin.params
    return copy


def generator_of(seed, consumed):
    return np.random.PCG64DXSM(seed).advance(consumed)


# ---- noise -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wanted_noise(index, critic_lstm, mask):
    """(theta [G m][L] with NaN rows where the mask leaves a group out, generator states afterwards) of the twin population
    whose generators had given NOISE["consumed"] draws before."""
    groups, per_group = NOISE["groups"], NOISE["per_group"]
    spec, twin = twin_policy(index, critic_lstm, groups, per_group)
    twin = fresh_twin(spec, twin)
    twin.set_rng_state([generator_of(seed, consumed).state for seed, consumed in zip(seeds_of(groups), NOISE["consumed"])])
    twin.set_noise(np.full((groups * per_group, spec.latent), np.nan, dtype=F32))
    twin.reset_noise(groups=None if mask is None else [bool(x) for x in mask])
    return twin.noise(), twin.rng_state()


# ---- forward ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_inputs(index, groups, per_group):
    """(obs [n, D], final_obs (NaN-led rows among live ones), starts uint8 [n] -- bytes 0, 1, 2, 255 mixed --, state
    [2, 2, n, H]: normal values, every group around its own non-zero level g + 1)."""
    width, hidden = lsde_cases.NETWORKS[index][:2]
    n = groups * per_group
    rng = np.random.default_rng(31 * index + n)
    starts = rng.choice(np.array([0, 0, 0, 1, 2, 255], dtype=np.uint8), n)
    starts[0] = 255
    if n > 1:
        starts[1] = 0
    state = (0.25 * rng.standard_normal((2, 2, n, hidden))).astype(F32)
    state += (1.0 + np.arange(n) // per_group).astype(F32)[None, None, :, None] * F32(0.125)
    return (policy_cases.hostile_rows(width, n, 50 * index + n, False), policy_cases.hostile_rows(width, n, 9 + n, True),
            starts, state)


@functools.lru_cache(maxsize=None)
def wanted_forward(index, critic_lstm, groups, per_group, deterministic):
    """({name: float32 [n]} for OUTPUTS and "state" [2, 2, n, H] of the twin population, theta [n, L] of one reset of every
    group).  mean and sigma, which act() does not return, are the definition's (lstm_sde_numpy) per group on the same
    slices; its other outputs are checked against the twin's here.  Computed once, shared, never changed."""
    from reinfocus_amd.environments import lstm_sde

    spec, twin = twin_policy(index, critic_lstm, groups, per_group)
    twin = fresh_twin(spec, twin)
    obs, final_obs, starts, state = forward_inputs(index, groups, per_group)
    twin.reset_noise()
    theta = twin.noise()
    after = np.full_like(state, np.nan)
    with np.errstate(all="ignore"):
        got = twin.act(obs, starts, final_obs, deterministic, states=(state.copy(), after))
        pieces = []
        for g in range(groups):
            rows = slice(g * per_group, (g + 1) * per_group)
            pieces.append(lstm_sde.lstm_sde_numpy(spec, twin.params[g], obs[rows], starts[rows],
                                                  np.ascontiguousarray(state[:, :, rows, :]), final_obs[rows], theta[rows],
                                                  deterministic))
    want = {name: np.concatenate([piece[name] for piece in pieces]) for name in OUTPUTS}
    for name, mine in zip(("actions", "values", "log_probs", "final_values", "env_actions"), got):
        assert bits(want[name]) == bits(mine), name
    assert bits(np.concatenate([piece["state"] for piece in pieces], axis=2)) == bits(after)
    want["state"] = after
    return want, theta


def regrouped_state(state, groups, per_group):
    return lstm_pop.regrouped_state(state, groups, per_group)


# ---- update ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def update_inputs(index, critic_lstm, groups, steps, per_group, kind="mixed"):
    """(spec, twin population with per-group parameters, parts dict over G m lanes as parts_of(rollout) hands it over).  The
    stored actions are each group's own sampled raw actions, the stored log-probabilities its own shifted by SHIFTS."""
    from reinfocus_amd.environments import learner, policy, sde

    spec, twin = twin_policy(index, critic_lstm, groups, per_group, base=300)
    lanes, rows = groups * per_group, steps * per_group
    total = groups * rows
    rng = np.random.default_rng(1000 * index + total)
    starts = group_starts(groups, steps, per_group, kind)
    states = (0.5 * rng.standard_normal((steps + 1,) + spec.state_shape(lanes))).astype(F32)
    parts = {"observations": lstm_learner_cases.learner_cases.finite_rows(spec.obs_width, total, 77 * index + total),
             "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32),
             "values": np.zeros(total, dtype=F32), "episode_starts": starts, "lstm_states": states, "n_steps": steps,
             "num_envs": lanes, "actions": np.zeros(total, dtype=F32), "log_probs": np.zeros(total, dtype=F32)}
    shifts = np.array(lstm_learner_cases.SHIFTS, dtype=F32)[np.arange(total) % len(lstm_learner_cases.SHIFTS)]
    for g in range(groups):
        piece = group_slices(parts, groups, g)
        mu, sigma, h = lsde_cases.own_head(spec, twin.params[g], piece, piece["episode_starts"], piece["lstm_states"], steps,
                                           per_group)
        theta = sde.noise_numpy(twin.params[g][spec.log_std_at:], rng.random(rows * spec.latent))
        with np.errstate(all="ignore"):
            actions = policy.canonical(mu + sde._rowdot(h, theta))
        parts["actions"][g * rows:(g + 1) * rows] = actions
        parts["log_probs"][g * rows:(g + 1) * rows] = sde.log_prob_of(actions, mu, sigma) - shifts[g * rows:(g + 1) * rows]
    assert np.isfinite(parts["actions"]).all() and np.isfinite(parts["log_probs"]).all()
    assert set(learner.BATCH_KEYS) <= set(parts)
    return spec, twin, parts


@functools.lru_cache(maxsize=None)
def twin_updates(index, critic_lstm, groups, steps, per_group, firsts, batch, updates, kind="mixed", nan_row=None):
    """Per consecutive update (params [G][P + L], states [G][S], stats [G][8]) of the twin population, update u from first
    rows (firsts + u) mod m T (a first row of m T, outside, stays).  nan_row: a row of flat()'s actions that holds a NaN.
    Computed once, shared, never changed."""
    from reinfocus_amd.environments import harness

    spec, twin, parts = update_inputs(index, critic_lstm, groups, steps, per_group, kind)
    if nan_row is not None:
        parts = dict(parts, actions=parts["actions"].copy())
        parts["actions"][nan_row] = np.nan
    twin = fresh_twin(spec, twin)
    learner = harness.PopulationLearner(twin, **hypers_of(groups))
    seen = []
    with np.errstate(all="ignore"):
        for update in range(updates):
            stats = learner.update(parts, firsts_of(firsts, update, steps * per_group), batch)
            seen.append((twin.params.copy(), twin_states(learner), stats))
    return seen


def wide_firsts():
    rows = WIDE_UPDATE["steps"] * WIDE_UPDATE["per_group"]
    return tuple((7 * g) % rows for g in range(WIDE_UPDATE["groups"]))


def depth_shape(critic_lstm):
    steps, per_group, kind, _, batch = lstm_learner_cases.LIMIT_LAYOUTS[DEPTH["layout"]]
    return (DEPTH["index"], critic_lstm, len(DEPTH["firsts"]), steps, per_group), kind, DEPTH["firsts"], batch


# ---- the limit: 65535 groups of one environment, one step ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def limit_parts(critic_lstm):
    """(7 packed parameter sets, each with its own log_std; 5 input blocks of one row; 3 hyper-parameter sets; 11
    generators)."""
    from reinfocus_amd.environments import learner

    spec = spec_of(0, critic_lstm)
    rng = np.random.default_rng(65535)
    params = []
    for k in range(LIMIT_PERIODS[0]):
        packed = np.abs(spec.pack(lsde_cases.state_dict(spec, 700 + k))) + F32(0.25 + 0.125 * k)
        packed[spec.log_std_at:] = F32(-1.0 + 0.25 * k)
        params.append(packed.astype(F32))
    blocks = []
    for j in range(LIMIT_PERIODS[1]):
        level = F32(0.125 * (1 + j)) + F32(0.03125) * np.arange(4, dtype=F32).reshape(2, 2, 1, 1)
        blocks.append(dict(observations=np.array([[0.5 + 0.75 * j]], dtype=F32), final=np.array([[3.0 - 0.5 * j]], dtype=F32),
                           starts=np.array([LIMIT_STARTS[j]], dtype=np.uint8), state=level.astype(F32),
                           actions=np.array([0.75 - 0.5 * j], dtype=F32), log_probs=np.array([-0.7 + 0.1 * j], dtype=F32),
                           advantages=rng.standard_normal(1).astype(F32), returns=rng.standard_normal(1).astype(F32),
                           episode_starts=np.array([[LIMIT_STARTS[j]], [1]], dtype=np.uint8),
                           lstm_states=np.stack([level, level + F32(7.0)]).astype(F32)))
    hypers = [learner.Hyper(learning_rate=1e-2 / (1 + h), clip_range=0.1 + 0.1 * h, ent_coef=0.01 * (1 + h),
                            vf_coef=0.5 + 0.25 * h, max_grad_norm=(1e6, 0.5, 0.05)[h], beta1=0.9 - 0.1 * h,
                            beta2=0.999 - 0.01 * h, adam_eps=(0.1, 0.3, 1.0)[h], normalize_advantage=h % 2)
              for h in range(LIMIT_PERIODS[2])]
    return params, blocks, hypers, [np.random.PCG64DXSM(900 + i) for i in range(LIMIT_GENERATORS)]


@functools.lru_cache(maxsize=None)
def limit_results(critic_lstm):
    """By the existing twin functions.  noise[k][i][c]: theta [1] of parameter set k from generator i after
    LIMIT_CONSUMED[c] draws; forwards[deterministic][k][j][t]: lstm_sde_numpy's dict of set k on block j with theta level t;
    updates[c]: the first update's (params, state, stats) of combination c (k = c % 7, j = c % 5, h = c % 3)."""
    from reinfocus_amd.environments import learner, lstm_learner, lstm_sde, sde

    spec = spec_of(0, critic_lstm)
    params, blocks, hypers, generators = limit_parts(critic_lstm)
    noise = [[[None] * len(LIMIT_CONSUMED) for _ in generators] for _ in params]
    for k, packed in enumerate(params):
        for i, generator in enumerate(generators):
            for c, consumed in enumerate(LIMIT_CONSUMED):
                moved = np.random.PCG64DXSM()
                moved.state = generator.state
                u = np.random.Generator(moved.advance(consumed)).random(spec.latent)
                noise[k][i][c] = sde.noise_numpy(packed[spec.log_std_at:], u).reshape(-1)
    forwards = {}
    for deterministic in (False, True):
        forwards[deterministic] = [[[None] * len(LIMIT_THETA) for _ in blocks] for _ in params]
        for k, packed in enumerate(params):
            for j, block in enumerate(blocks):
                for t, level in enumerate(LIMIT_THETA):
                    forwards[deterministic][k][j][t] = lstm_sde.lstm_sde_numpy(
                        spec, packed, block["observations"], block["starts"], block["state"], block["final"],
                        np.full((1, spec.latent), level, dtype=F32), deterministic)
    updates = []
    for c in range(105):
        k, j, h = (c % period for period in LIMIT_PERIODS)
        batch = {key: blocks[j][key] for key in learner.BATCH_KEYS}
        updates.append(lstm_learner.lstm_update_numpy(spec, params[k], learner.fresh_state(spec), batch,
                                                      blocks[j]["episode_starts"], blocks[j]["lstm_states"], 1, 1, 0, 1, hypers[h]))
    return noise, forwards, updates


def limit_arrays(critic_lstm, groups=LIMIT_GROUPS):
    """What group g gets and what it must give, for g = 0 .. groups - 1: (inputs dict, wanted theta [G][L] of the noise
    reset (NaN where unselected), {deterministic: {name: wanted}}, wanted (params, states, stats) of an update)."""
    from reinfocus_amd.environments import learner, policy, population

    spec = spec_of(0, critic_lstm)
    params, blocks, hypers, generators = limit_parts(critic_lstm)
    noise, forwards, updates = limit_results(critic_lstm)
    g = np.arange(groups)
    k, j, h, c, i = g % LIMIT_PERIODS[0], g % LIMIT_PERIODS[1], g % LIMIT_PERIODS[2], g % 105, g % LIMIT_GENERATORS
    outside = g % LIMIT_OUTSIDE[0] == LIMIT_OUTSIDE[1]
    selected = g % LIMIT_UNSELECTED[0] != LIMIT_UNSELECTED[1]
    inputs = {"params": np.stack(params)[k], "hyper": population.hyper_records(hypers)[h], "outside": outside,
              "firsts": outside.astype(np.int32), "selected": selected,
              "consumed": np.array(LIMIT_CONSUMED, dtype=np.uint64)[h],
              "theta": np.array(LIMIT_THETA, dtype=F32)[h][:, None].repeat(spec.latent, axis=1),
              "gens": np.array([policy.generator_words(generator) for generator in generators], dtype=np.uint64)[i]}
    for key in ("observations", "final", "starts") + tuple(key for key in learner.BATCH_KEYS if key != "observations"):
        inputs[key] = np.concatenate([block[key] for block in blocks])[j]
    inputs["state"] = np.ascontiguousarray(np.concatenate([block["state"] for block in blocks], axis=2)[:, :, j, :])
    inputs["episode_starts"] = np.ascontiguousarray(np.concatenate([block["episode_starts"] for block in blocks], axis=1)[:, j])
    inputs["lstm_states"] = np.ascontiguousarray(np.concatenate([block["lstm_states"] for block in blocks], axis=3)[:, :, :, j, :])
    table = np.array(noise, dtype=F32)  # [7][11][3][L]
    wanted_theta = table[k, i, h]
    wanted_theta[~selected] = np.nan
    wanted_forward = {}
    for deterministic, results in forwards.items():
        flat = [result for per_set in results for per_block in per_set for result in per_block]
        at = (k * len(blocks) + j) * len(LIMIT_THETA) + h
        wanted_forward[deterministic] = {name: np.concatenate([result[name] for result in flat])[at] for name in OUTPUTS}
        wanted_forward[deterministic]["state"] = np.ascontiguousarray(
            np.concatenate([result["state"] for result in flat], axis=2)[:, :, at, :])
    wanted_update = tuple(np.stack([update[part] for update in updates])[c] for part in range(3))
    return inputs, wanted_theta, wanted_forward, wanted_update


def hostcheck():
    from tests import helpers

    lib = ctypes.CDLL(helpers.built("tests/lstmsdepopcheck", "liblstmsdepopcheck.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.lspop_state_size.restype = lib.lspop_workspace_size.restype = ctypes.c_ulonglong
    lib.lspop_state_size.argtypes = [vp, i32, i32]
    lib.lspop_workspace_size.argtypes = [vp, i32, i32, i32, i32]
    lib.lspop_offsets.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.lspop_noise.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    lib.lspop_forward.argtypes = [vp, i32, i32] + [vp] * 12
    lib.lspop_update.argtypes = [vp, i32, i32, i32] + [vp] * 11 + [i32, vp]
    return lib


def critic_desc(spec):
    from reinfocus_amd import _native

    return _native.LstmCriticDesc(*spec.critic_desc())


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
def e2e_env(device_form):
    from reinfocus_amd.environments import harness

    n = E2E["groups"] * E2E["per_group"]
    if device_form:
        return harness.DeviceVectorContinuousJumps(num_envs=n, device_initializer=True, episode_records=True,
                                                   **rollout_cases.ENV_KW)
    return harness.VectorContinuousJumps(num_envs=n, episode_records=True, **rollout_cases.ENV_KW)


def e2e_spec(env, critic_lstm=True):
    from reinfocus_amd.environments import lstm_sde

    return lstm_sde.LstmSdePolicySpec(int(env.single_observation_space.shape[0]), lstm_hidden=9, pi=(6,), vf=(5, 7),
                                      activation="tanh", enable_critic_lstm=critic_lstm)


def e2e_states(spec):
    """One state_dict per group, without log_std: the groups keep their own log_std_init."""
    states = [lsde_cases.state_dict(spec, 500 + 17 * g) for g in range(E2E["groups"])]
    for g, state in enumerate(states):
        state["log_std"][:] = F32(E2E["log_std"][g])
    return states


def e2e_splits(iteration):
    rows = E2E["steps"] * E2E["per_group"]
    return np.random.default_rng(800 + iteration).integers(rows, size=(E2E["epochs"], E2E["groups"]))


def e2e_hypers():
    return dict(learning_rate=[1e-2, 3e-3, 0.0], ent_coef=[0.0, 0.01, 0.02], clip_range=0.2)


def e2e_runs(rollout, policy, learner, reset, unwrap):
    obs = reset()
    seen = []
    for iteration in range(E2E["iterations"]):
        rollout.start(obs if iteration == 0 else None)
        rollout.collect(policy, sde_sample_freq=E2E["freqs"])
        record = policy_cases.slabs_of(rollout, unwrap)
        record["episode_starts"], record["lstm_states"] = unwrap(rollout.episode_starts), unwrap(rollout.lstm_states)
        record["theta"] = unwrap(policy.noise())
        record["stats"] = unwrap(learner.train(rollout, E2E["epochs"], E2E["batch"], e2e_splits(iteration)))
        record["params"] = unwrap(policy.params)
        seen.append(record)
    return seen


@functools.lru_cache(maxsize=None)
def e2e_twin_runs(critic_lstm=True):
    from reinfocus_amd.environments import harness

    env = e2e_env(False)
    try:
        spec = e2e_spec(env, critic_lstm)
        groups = E2E["groups"]
        policy = harness.LstmSdePopulationPolicy(spec, groups, seeds_of(groups), log_std_init=E2E["log_std"],
                                                 num_envs=env.num_envs)
        for g, state in enumerate(e2e_states(spec)):
            policy.load_state_dict(state, group=g)
        learner = harness.PopulationLearner(policy, **e2e_hypers())
        rollout = harness.Rollout(env, E2E["steps"], GAMMA, GAE_LAMBDA)
        runs = e2e_runs(rollout, policy, learner, lambda: env.reset()[0], np.array)
        return runs, policy.rng_state(), twin_states(learner), policy.lstm_state()
    finally:
        env.close()


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
_untouched = policy_cases._untouched
_guarded_floats, _guards_kept, _same_update, _groups_that_differ = (lstm_pop._guarded_floats, lstm_pop._guards_kept,
                                                                    lstm_pop._same_update, lstm_pop._groups_that_differ)
_capturing, _cuda_states, _Packed = lstm_pop._capturing, lstm_pop._cuda_states, lstm_pop._Packed


def _sentinels(torch, shape):
    """Sentinel floats of `shape` between two guard floats: (whole, the view)."""
    whole, view = _guarded_floats(torch, np.zeros(shape, dtype=F32))
    view.view(torch.int32).fill_(SENTINEL)
    return whole, view


def _outputs(torch, n):
    whole, out = {}, {}
    for name in OUTPUTS:
        whole[name], out[name] = _sentinels(torch, (n,))
    return whole, out


def _stream(torch, stream=None):
    return torch.cuda.current_stream().cuda_stream if stream is None else stream


def _noise(torch, ctx, spec, groups, per_group, params, table, consumed, select, theta, changed=(), stream=None):
    pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = dict(desc=spec.critic_desc(), groups=groups, per_group=per_group, params=params.data_ptr(), gens=table.data_ptr(),
             consumed=consumed.data_ptr(), select=pointer(select), theta=theta.data_ptr())
    a.update(changed)
    ctx.lstm_sde_noise_reset_grouped(a["desc"], a["groups"], a["per_group"], a["params"], a["gens"], a["consumed"], a["select"],
                                     a["theta"], _stream(torch, stream))


def _forward(torch, ctx, spec, groups, per_group, params, obs, starts, final_obs, state_in, state_out, theta, flags, out,
             changed=(), stream=None):
    pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = dict(desc=spec.critic_desc(), groups=groups, per_group=per_group, params=params.data_ptr(), obs=obs.data_ptr(),
             starts=starts.data_ptr(), final_obs=pointer(final_obs), state_in=state_in.data_ptr(),
             state_out=pointer(state_out), theta=pointer(theta), flags=flags)
    a.update({name: pointer(out.get(name)) for name in OUTPUTS})
    a.update(changed)
    ctx.lstm_sde_forward_grouped(a["desc"], a["groups"], a["per_group"], a["params"], a["obs"], a["starts"], a["final_obs"],
                                 a["state_in"], a["state_out"], a["theta"], a["flags"], *(a[name] for name in OUTPUTS),
                                 _stream(torch, stream))


def _words(generator):
    from reinfocus_amd.environments import policy

    return policy.generator_words(generator)


def _table(torch, groups):
    words = np.array([_words(np.random.PCG64DXSM(seed)) for seed in seeds_of(groups)], dtype=np.uint64)
    return torch.from_numpy(words.view(np.int64)).cuda()


def noise_case(torch, ctx, index, critic_lstm):
    """rf_lstm_sde_noise_reset_grouped against the twin population as bytes for the three masks, theta sentinel-filled
    between guards: the unselected rows keep their sentinel bytes; then G stand-alone rf_lstm_critic_sde_noise_reset
    launches from generators advanced on the host give the selected rows."""
    groups, per_group = NOISE["groups"], NOISE["per_group"]
    spec, twin = twin_policy(index, critic_lstm, groups, per_group)
    params = torch.from_numpy(twin.params).cuda()
    table = _table(torch, groups)
    consumed = torch.from_numpy(np.array(NOISE["consumed"], dtype=np.uint64).view(np.int64)).cuda()
    cells = per_group * spec.latent
    for mask in NOISE["masks"]:
        want, _ = wanted_noise(index, critic_lstm, mask)
        whole, theta = _sentinels(torch, (groups * per_group, spec.latent))
        select = None if mask is None else torch.tensor(mask, dtype=torch.uint8, device="cuda")
        _noise(torch, ctx, spec, groups, per_group, params, table, consumed, select, theta)
        torch.cuda.synchronize()
        got = theta.cpu().numpy()
        for g in range(groups):
            rows = slice(g * per_group, (g + 1) * per_group)
            if mask is None or mask[g]:
                assert bits(got[rows]) == bits(want[rows]), f"mask {mask}: group {g} differs"
            else:
                assert (got[rows].view(np.uint32) == SENTINEL).all(), f"mask {mask}: group {g} was written"
        assert _guards_kept(whole), "a guard float of theta was written"
    want, _ = wanted_noise(index, critic_lstm, None)
    for g, (seed, taken) in enumerate(zip(seeds_of(groups), NOISE["consumed"])):
        whole, theta = _sentinels(torch, (per_group, spec.latent))
        ctx.lstm_critic_sde_noise_reset(spec.critic_desc(), params[g].data_ptr(), per_group, _words(generator_of(seed, taken)),
                                        theta.data_ptr(), _stream(torch))
        torch.cuda.synchronize()
        assert bits(theta.cpu().numpy()) == bits(want[g * per_group:(g + 1) * per_group]), f"stand-alone group {g}"
        assert cells == theta.numel() and _guards_kept(whole)


def forward_case(torch, ctx, index, critic_lstm, groups, per_group, alone=True):
    """rf_lstm_sde_forward_grouped against the twin population as bytes: sampled and deterministic (theta NULL), the state in
    place and from `in` to `out`; each pi output asked for by itself; values only (the state stays); every output between
    guard floats.  Then G stand-alone rf_lstm_critic_sde_forward launches on contiguous copies."""
    from reinfocus_amd.environments import policy

    spec, twin = twin_policy(index, critic_lstm, groups, per_group)
    n = groups * per_group
    obs_h, final_h, starts_h, state_h = forward_inputs(index, groups, per_group)
    params, obs, final_obs, starts = (torch.from_numpy(a).cuda() for a in (twin.params, obs_h, final_h, starts_h))
    for deterministic, in_place in ((False, True), (False, False), (True, False)):
        want, theta_h = wanted_forward(index, critic_lstm, groups, per_group, deterministic)
        theta = None if deterministic else torch.from_numpy(theta_h).cuda()
        whole, out = _outputs(torch, n)
        whole_in, state_in = _guarded_floats(torch, state_h)
        whole_out, state_out = (whole_in, state_in) if in_place else _guarded_floats(torch, np.full_like(state_h, np.nan))
        # (a deterministic call hands in no theta at all; the flag alone is the one-group case's)
        _forward(torch, ctx, spec, groups, per_group, params, obs, starts, final_obs, state_in, state_out, theta,
                 policy.DETERMINISTIC if deterministic else 0, out)
        torch.cuda.synchronize()
        what = f"deterministic {deterministic}, in place {in_place}"
        for name in OUTPUTS:
            assert bits(out[name].cpu().numpy()) == bits(want[name]), f"{what}: {name} differ"
            assert _guards_kept(whole[name]), f"{what}: a guard float of {name} was written"
        assert bits(state_out.cpu().numpy()) == bits(want["state"]), f"{what}: the state differs"
        assert _guards_kept(whole_in) and _guards_kept(whole_out), "a guard float of a state was written"
        if not in_place:
            assert bits(state_in.cpu().numpy()) == bits(state_h), "state_in was written"
    want, theta_h = wanted_forward(index, critic_lstm, groups, per_group, False)
    theta = torch.from_numpy(theta_h).cuda()
    for names, with_final in [((name,), False) for name in PI_OUTPUTS] + [(("values", "final_values"), True)]:
        whole, out = _outputs(torch, n)
        whole_in, state_in = _guarded_floats(torch, state_h)
        _forward(torch, ctx, spec, groups, per_group, params, obs, starts, final_obs if with_final else None, state_in, None,
                 theta, 0, {name: out[name] for name in names})
        torch.cuda.synchronize()
        for name in OUTPUTS:
            if name in names:
                assert bits(out[name].cpu().numpy()) == bits(want[name]), f"{names} alone: {name} differ"
                assert _guards_kept(whole[name])
            else:
                assert _untouched(whole[name]), f"{names} alone: {name} was written"
        assert bits(state_in.cpu().numpy()) == bits(state_h) and _guards_kept(whole_in), f"{names} alone: the state changed"
    if not alone:
        return
    got = {name: torch.zeros(n, dtype=torch.float32, device="cuda") for name in OUTPUTS}
    states_out = []
    for g in range(groups):
        rows = slice(g * per_group, (g + 1) * per_group)
        piece_in = torch.from_numpy(np.ascontiguousarray(state_h[:, :, rows, :])).cuda()
        piece_out = torch.zeros_like(piece_in)
        ctx.lstm_critic_sde_forward(spec.critic_desc(), params[g].data_ptr(), per_group, obs[rows].data_ptr(),
                                    starts[rows].data_ptr(), final_obs[rows].data_ptr(), piece_in.data_ptr(),
                                    piece_out.data_ptr(), theta[rows].data_ptr(), 0,
                                    *(got[name][rows].data_ptr() for name in OUTPUTS), _stream(torch))
        states_out.append(piece_out)
    torch.cuda.synchronize()
    for name in OUTPUTS:
        assert bits(got[name].cpu().numpy()) == bits(want[name]), f"stand-alone launches: {name} differ"
    assert bits(torch.cat(states_out, dim=2).cpu().numpy()) == bits(want["state"]), "stand-alone launches: the state differs"


def stride_promises(index, critic_lstm):
    """The twin over the bytes of the state read as [G][2][2][m][H] gives another next state and another mean (and, with
    the LSTM critic, other values): a kernel that added g times a size to the state pointer could not pass."""
    from reinfocus_amd.environments import lstm_sde

    groups, per_group = STRIDE
    spec, twin = twin_policy(index, critic_lstm, groups, per_group)
    obs, final_obs, starts, state = forward_inputs(index, groups, per_group)
    want, _ = wanted_forward(index, critic_lstm, groups, per_group, True)
    wrong = regrouped_state(state, groups, per_group)
    assert bits(wrong) != bits(state)
    with np.errstate(all="ignore"):
        pieces = [lstm_sde.lstm_sde_numpy(spec, twin.params[g], obs[g * per_group:(g + 1) * per_group],
                                          starts[g * per_group:(g + 1) * per_group],
                                          np.ascontiguousarray(wrong[:, :, g * per_group:(g + 1) * per_group, :]),
                                          final_obs[g * per_group:(g + 1) * per_group], None, True) for g in range(groups)]
    assert bits(np.concatenate([piece["state"] for piece in pieces], axis=2)) != bits(want["state"])
    if spec.lstm_hidden == 1:  # (the least network's one relu unit after one cell unit: the heads may not see the state)
        return
    assert bits(np.concatenate([piece["mean"] for piece in pieces])) != bits(want["mean"])
    if critic_lstm:
        assert bits(np.concatenate([piece["values"] for piece in pieces])) != bits(want["values"])


def stride_case(torch, ctx, index, critic_lstm):
    groups, per_group = STRIDE
    forward_case(torch, ctx, index, critic_lstm, groups, per_group, alone=False)
    stride_promises(index, critic_lstm)


class _Learner(lstm_pop._Learner):
    """The raw arrays of rf_lstm_sde_update_grouped on the device, parameters, states and stats between guard floats."""

    def __init__(self, torch, ctx, spec, twin, parts, hypers, batch):
        from reinfocus_amd.environments import learner, population

        self.torch, self.ctx, self.spec, self.groups = torch, ctx, spec, twin.groups
        self.steps, self.lanes = parts["n_steps"], parts["num_envs"]
        self.per_group = self.lanes // self.groups
        self.parts = {key: torch.from_numpy(value).cuda() for key, value in parts.items() if isinstance(value, np.ndarray)}
        self.whole_params, self.params = _guarded_floats(torch, twin.params)
        fresh = np.stack([learner.fresh_state(spec) for _ in range(self.groups)])
        self.whole_state = torch.full((fresh.size + 4,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.state = self.whole_state[2:-2].view(fresh.shape)  # (8-byte aligned between two guard floats on either side)
        self.state.copy_(torch.from_numpy(fresh))
        self.whole_stats, self.stats = _guarded_floats(torch, np.zeros((self.groups, 8), dtype=F32))
        self.stats.view(torch.int32).fill_(SENTINEL)
        records = hypers if isinstance(hypers, np.ndarray) else population.hyper_records(hypers)
        self.hyper = torch.from_numpy(records.view(np.float64).copy()).cuda()
        size = ctx.lstm_sde_grouped_workspace_size(spec.critic_desc(), self.groups, self.per_group, self.steps, batch)
        assert size > 0 and size % 8 == 0
        assert size == self.groups * ctx.lstm_critic_workspace_size(spec.critic_desc(), batch, sde=True)
        assert ctx.lstm_sde_grouped_state_size(spec.critic_desc(), self.groups, self.per_group) == 4 * fresh.size
        self.whole_workspace = torch.full((size // 4 + 4,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.workspace = self.whole_workspace[2:-2]
        self.batch = batch

    def enqueue(self, table, changed=(), stream=None):
        a = dict(desc=self.spec.critic_desc(), groups=self.groups, per_group=self.per_group, steps=self.steps,
                 hyper=self.hyper.data_ptr(), params=self.params.data_ptr(), state=self.state.data_ptr(),
                 workspace=self.workspace.data_ptr(), obs=self.parts["observations"].data_ptr(),
                 actions=self.parts["actions"].data_ptr(), log_probs=self.parts["log_probs"].data_ptr(),
                 advantages=self.parts["advantages"].data_ptr(), returns=self.parts["returns"].data_ptr(),
                 starts=self.parts["episode_starts"].data_ptr(), states=self.parts["lstm_states"].data_ptr(),
                 firsts=table.data_ptr(), batch=self.batch, stats=self.stats.data_ptr())
        a.update(changed)
        self.ctx.lstm_sde_update_grouped(a["desc"], a["groups"], a["per_group"], a["steps"], a["hyper"], a["params"],
                                         a["state"], a["workspace"], a["obs"], a["actions"], a["log_probs"], a["advantages"],
                                         a["returns"], a["starts"], a["states"], a["firsts"], a["batch"], a["stats"],
                                         _stream(self.torch, stream))


def _learner_of(torch, ctx, index, critic_lstm, groups, steps, per_group, batch, kind="mixed", parts=None):
    from reinfocus_amd.environments import harness

    spec, twin, cached = update_inputs(index, critic_lstm, groups, steps, per_group, kind)
    hypers = harness.PopulationLearner(fresh_twin(spec, twin), **hypers_of(groups)).hypers()
    return spec, twin, hypers, _Learner(torch, ctx, spec, twin, cached if parts is None else parts, hypers, batch)


def _alone_updates(torch, ctx, spec, twin, hypers, parts, firsts, batch, want):
    """The same device, G stand-alone learners over contiguous copies of the groups' slices: len(want) consecutive
    rf_lstm_critic_sde_update launches each give the bytes of want[update][.][g]."""
    from reinfocus_amd.environments import learner

    groups = twin.groups
    steps, per_group = parts["n_steps"], parts["num_envs"] // groups
    size_alone = ctx.lstm_critic_workspace_size(spec.critic_desc(), batch, sde=True)
    for g in range(groups):
        piece = {key: torch.from_numpy(value).cuda() for key, value in group_slices(parts, groups, g).items()
                 if isinstance(value, np.ndarray)}
        params = torch.from_numpy(twin.params[g].copy()).cuda()
        state = torch.from_numpy(learner.fresh_state(spec)).cuda()
        workspace = torch.zeros(size_alone // 4, dtype=torch.float32, device="cuda")
        stats = torch.zeros(8, dtype=torch.float32, device="cuda")
        for update in range(len(want)):
            ctx.lstm_critic_sde_update(spec.critic_desc(), hypers[g], params.data_ptr(), state.data_ptr(),
                                       workspace.data_ptr(), steps, per_group, piece["observations"].data_ptr(),
                                       piece["actions"].data_ptr(), piece["log_probs"].data_ptr(),
                                       piece["advantages"].data_ptr(), piece["returns"].data_ptr(),
                                       piece["episode_starts"].data_ptr(), piece["lstm_states"].data_ptr(),
                                       firsts_of(firsts, update, steps * per_group)[g], batch, stats.data_ptr(), _stream(torch))
            torch.cuda.synchronize()
            _same_update((params.cpu().numpy(), state.cpu().numpy(), stats.cpu().numpy()),
                         tuple(x[g] for x in want[update]), f"stand-alone group {g}, update {update}")


def update_promises(index, critic_lstm, batch):
    """No comparison of an update case is vacuous: no group is skipped, groups 0 and 2 move, group 1 (learning rate 0) stays,
    log_std moves with the rest, and the parameters -- log_std among them -- differ per group."""
    u = UPDATE
    spec, twin, _ = update_inputs(index, critic_lstm, u["groups"], u["steps"], u["per_group"])
    want = twin_updates(index, critic_lstm, u["groups"], u["steps"], u["per_group"], u["firsts"], batch, u["updates"])
    assert all((stats[:, 7] == 0).all() for _, _, stats in want)
    assert bits(want[1][0][1]) == bits(twin.params[1]) and bits(want[1][0][0]) != bits(twin.params[0])
    assert bits(want[1][0][2][spec.log_std_at:]) != bits(twin.params[2][spec.log_std_at:]), "log_std did not move"
    assert len({bits(row[spec.log_std_at:]) for row in twin.params}) == u["groups"]
    assert bits(want[0][1]) != bits(want[1][1])


def update_case(torch, ctx, index, critic_lstm, batch):
    """rf_lstm_sde_update_grouped against the twin population over two consecutive updates: parameters, optimizer states
    and stats as bytes between guards; then G stand-alone rf_lstm_critic_sde_update launches on contiguous slice copies give
    the same bytes."""
    u = UPDATE
    rows = u["steps"] * u["per_group"]
    spec, twin, hypers, device = _learner_of(torch, ctx, index, critic_lstm, u["groups"], u["steps"], u["per_group"], batch)
    want = twin_updates(index, critic_lstm, u["groups"], u["steps"], u["per_group"], u["firsts"], batch, u["updates"])
    for update in range(u["updates"]):
        _same_update(device.update(firsts_of(u["firsts"], update, rows)), want[update], f"update {update}")
    assert device.guards_kept(), "a guard was written"
    update_promises(index, critic_lstm, batch)
    _, _, parts = update_inputs(index, critic_lstm, u["groups"], u["steps"], u["per_group"])
    _alone_updates(torch, ctx, spec, twin, hypers, parts, u["firsts"], batch, want)


def isolation_rows():
    """(the row of flat()'s actions that holds the NaN: row 2 of group 1's minibatch; firsts with firsts[1] = N)."""
    u = UPDATE
    rows = u["steps"] * u["per_group"]
    return rows + (u["firsts"][1] + 2) % rows, (u["firsts"][0], rows, u["firsts"][2])


def isolation_case(torch, ctx, critic_lstm):
    """A NaN raw action in group 1's minibatch: group 1 carries RF_PPO_INVALID and keeps parameters and optimizer state
    byte for byte, groups 0 and 2 equal a run without the NaN.  The same with firsts[1] = N."""
    u = UPDATE
    index, batch = NETS[1], 5
    shape = (index, critic_lstm, u["groups"], u["steps"], u["per_group"])
    spec, twin, parts = update_inputs(*shape)
    clean = twin_updates(*shape, u["firsts"], batch, 1)[0]
    before = _learner_of(torch, ctx, *shape, batch)[3].outputs()
    nan_row, outside = isolation_rows()
    poisoned = dict(parts, actions=parts["actions"].copy())
    poisoned["actions"][nan_row] = np.nan
    device = _learner_of(torch, ctx, *shape, batch, parts=poisoned)[3]
    for what, got in (("a NaN raw action", device.update(u["firsts"])),
                      ("firsts[1] = N", _learner_of(torch, ctx, *shape, batch)[3].update(outside))):
        for g in (0, 2):
            _same_update(tuple(x[g] for x in got), tuple(x[g] for x in clean), f"{what}: group {g}")
        assert got[2][1][7] == INVALID, f"{what}: group 1 has flags {got[2][1][7]}"
        assert bits(got[0][1]) == bits(before[0][1]) and bits(got[1][1]) == bits(before[1][1]), f"{what}: group 1 moved"
    assert device.guards_kept()


def depth_case(torch, ctx, critic_lstm):
    """T = 17, m = 4, G = 3 at B = 65 on the H = 16 network: sequences of 1, 8, 9, 16 and 17 rows, every group with its own
    first row and -- its columns rolled -- sequence structure, against the twin group by group."""
    shape, kind, firsts, batch = depth_shape(critic_lstm)
    groups, steps, per_group = shape[2:]
    device = _learner_of(torch, ctx, *shape, batch, kind=kind)[3]
    want = twin_updates(*shape, firsts, batch, DEPTH["updates"], kind)
    for update in range(len(want)):
        got = device.update(firsts_of(firsts, update, steps * per_group))
        for g in range(groups):
            _same_update(tuple(x[g] for x in got), tuple(x[g] for x in want[update]), f"update {update}, group {g}")
    assert device.guards_kept() and all((stats[:, 7] == 0).all() for _, _, stats in want)


def limit_case(torch, ctx):
    """H = 256 (ppo_lstm_untuned.yml's network), G = 2, m = 2, T = 3, B = 6 = m T, both critic kinds."""
    c = LIMIT
    for critic_lstm in CRITICS:
        device = _learner_of(torch, ctx, c["index"], critic_lstm, c["groups"], c["steps"], c["per_group"], c["batch"],
                             kind="some")[3]
        want = twin_updates(c["index"], critic_lstm, c["groups"], c["steps"], c["per_group"], c["firsts"], c["batch"], 1, "some")
        _same_update(device.update(c["firsts"]), want[0], f"enable_critic_lstm={critic_lstm}")
        assert device.guards_kept() and (want[0][2][:, 7] == 0).all()


def wide_update_case(torch, ctx):
    """One update at G = 64, m = 8, T = 8, B = 8 on the H = 16 network, every group its own first row, against the twin."""
    c = WIDE_UPDATE
    shape = (c["index"], True, c["groups"], c["steps"], c["per_group"])
    device = _learner_of(torch, ctx, *shape, c["batch"], kind="none")[3]
    want = twin_updates(*shape, wide_firsts(), c["batch"], 1, "none")
    _same_update(device.update(wide_firsts()), want[0], "G = 64")
    assert device.guards_kept()


def group_limit_case(torch, ctx, critic_lstm):
    """RF_POPULATION_MAX_GROUPS groups of one environment on the least network (limit_arrays): one masked noise reset, the
    forward sampled and deterministic with the state in place, one update at m = T = B = 1 of fresh optimizers: every output
    byte of every group against its combination's result."""
    from reinfocus_amd.environments import learner, policy

    spec, groups = spec_of(0, critic_lstm), LIMIT_GROUPS
    inputs, wanted_theta, wanted_forward_, wanted_update = limit_arrays(critic_lstm)
    params, obs, final_obs, starts = (torch.from_numpy(inputs[key]).cuda() for key in ("params", "observations", "final", "starts"))
    table = torch.from_numpy(inputs["gens"].view(np.int64)).cuda()
    consumed = torch.from_numpy(inputs["consumed"].view(np.int64)).cuda()
    select = torch.from_numpy(inputs["selected"].astype(np.uint8)).cuda()
    whole, theta = _sentinels(torch, (groups, spec.latent))
    _noise(torch, ctx, spec, groups, 1, params, table, consumed, select, theta)
    torch.cuda.synchronize()
    got = theta.cpu().numpy()
    chosen = inputs["selected"]
    differ = _groups_that_differ(got[chosen], wanted_theta[chosen])
    assert differ.size == 0, f"theta differs in {differ.size} groups, first {np.flatnonzero(chosen)[differ[:4]]}"
    assert (got[~chosen].view(np.uint32) == SENTINEL).all() and (~chosen).sum() == 13107, "an unselected group was written"
    assert _guards_kept(whole)
    theta = torch.from_numpy(inputs["theta"]).cuda()
    for deterministic in (False, True):
        whole, out = _outputs(torch, groups)
        whole_state, state = _guarded_floats(torch, inputs["state"])
        _forward(torch, ctx, spec, groups, 1, params, obs, starts, final_obs, state, state, None if deterministic else theta,
                 policy.DETERMINISTIC if deterministic else 0, out)
        torch.cuda.synchronize()
        for name in OUTPUTS:
            differ = _groups_that_differ(out[name].cpu().numpy(), wanted_forward_[deterministic][name])
            assert differ.size == 0, f"deterministic {deterministic}: {name} differ in {differ.size} groups, first {differ[:4]}"
            assert _guards_kept(whole[name]), f"a guard float of {name} was written"
        differ = _groups_that_differ(state.cpu().numpy(), wanted_forward_[deterministic]["state"], axis=2)
        assert differ.size == 0, f"deterministic {deterministic}: the state differs in {differ.size} groups, first {differ[:4]}"
        assert _guards_kept(whole_state), "a guard float of the state was written"
    parts = {key: inputs[key] for key in learner.BATCH_KEYS + ("episode_starts", "lstm_states")}
    parts.update(n_steps=1, num_envs=groups)
    device = _Learner(torch, ctx, spec, _Packed(inputs["params"]), parts, inputs["hyper"], 1)
    before = device.outputs()
    got = device.update(inputs["firsts"])
    assert device.guards_kept(), "a guard was written"
    inside, outside = ~inputs["outside"], inputs["outside"]
    assert outside.sum() == 5958 and outside[5] and outside[16] and not outside[4] and not outside[6]
    for name, x, y, kept in zip(("parameters", "optimizer states", "stats"), got, wanted_update, before):
        differ = _groups_that_differ(x[inside], y[inside])
        assert differ.size == 0, f"{name} differ in {differ.size} groups, first {np.flatnonzero(inside)[differ[:4]]}"
        if name != "stats":
            differ = _groups_that_differ(x[outside], kept[outside])
            assert differ.size == 0, f"{name} of {differ.size} groups outside moved, first {np.flatnonzero(outside)[differ[:4]]}"
    assert (got[2][outside, 7] == INVALID).all(), "a group whose first row lies outside does not carry RF_PPO_INVALID"


def kernel_refusal_case(torch, ctx):
    """Each refusal of the three entry points leaves every output as it was; a capturing stream is refused by the forward
    and the update; the size functions return 0 where they refuse."""
    index, critic_lstm, groups, per_group = SMALL, True, 3, 3
    spec, twin = twin_policy(index, critic_lstm, groups, per_group)
    n = groups * per_group
    obs_h, final_h, starts_h, state_h = forward_inputs(index, groups, per_group)
    want, theta_h = wanted_forward(index, critic_lstm, groups, per_group, False)
    params, obs, final_obs, starts, theta_in = (torch.from_numpy(a).cuda() for a in (twin.params, obs_h, final_h, starts_h, theta_h))
    whole, out = _outputs(torch, n)
    whole_in, state_in = _guarded_floats(torch, state_h)
    whole_out, state_out = _sentinels(torch, state_h.shape)

    def attempt(call, changed, stream=None):
        try:
            call(changed, stream)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            return str(caught)
        return None

    def forward(changed, stream=None):
        _forward(torch, ctx, spec, groups, per_group, params, obs, starts, final_obs, state_in, state_out, theta_in, 0, out,
                 changed, stream)

    def refused(match, **changed):
        message = attempt(forward, changed)
        assert message is not None and match in message, f"not refused ({match}): {message}"
        torch.cuda.synchronize()
        assert all(_untouched(w) for w in whole.values()) and _untouched(whole_out), f"an output was written ({match})"

    host = np.zeros((n + 2, max(spec.obs_width, 4 * spec.lstm_hidden, spec.latent)), dtype=F32)
    refused("d_obs is not device memory", obs=host.ctypes.data)
    refused("d_episode_starts is not device memory", starts=host.ctypes.data)
    refused("d_state_in is not device memory", state_in=host.ctypes.data)
    refused("d_theta is not device memory", theta=host.ctypes.data)
    refused("d_sigma is not device memory", sigma=host.ctypes.data)
    refused("needs d_theta", theta=None)
    refused("NULL argument", starts=None)
    refused("NULL argument", state_in=None)
    refused("must be in 1", groups=0)
    refused("must be in 1", per_group=0)
    refused("must be in 1", groups=65536)
    refused("not aligned", theta=theta_in.data_ptr() + 2)
    refused("d_values overlaps d_log_probs", values=out["log_probs"].data_ptr())
    refused("d_values overlaps d_obs", values=obs.data_ptr())
    refused("d_actions overlaps d_theta", actions=theta_in.data_ptr())
    refused("d_state_out overlaps d_state_in", state_out=state_in.data_ptr() + 4 * spec.lstm_hidden)
    refused("d_state_out overlaps d_params", state_out=params.data_ptr())
    refused("outside the limits", desc=(0,) + tuple(spec.critic_desc()[1:]))
    refused("outside the limits", desc=tuple(spec.critic_desc()[:-1]) + (2,))
    refused("unknown flags", flags=2)
    refused("needs d_final_obs", final_obs=None)
    message = _capturing(torch, lambda stream: attempt(forward, {}, stream))
    assert message is not None and "being captured" in message, message
    torch.cuda.synchronize()
    assert all(_untouched(w) for w in whole.values()) and _untouched(whole_out), "an output was written (a capturing stream)"
    forward({})
    torch.cuda.synchronize()
    for name in OUTPUTS:
        assert bits(out[name].cpu().numpy()) == bits(want[name]), name
    assert bits(state_out.cpu().numpy()) == bits(want["state"]) and _guards_kept(whole_out) and _guards_kept(whole_in)

    table = _table(torch, groups)
    consumed = torch.zeros(groups, dtype=torch.int64, device="cuda")
    select = torch.ones(groups, dtype=torch.uint8, device="cuda")
    whole_theta, theta = _sentinels(torch, (n, spec.latent))

    def noise(changed, stream=None):
        _noise(torch, ctx, spec, groups, per_group, params, table, consumed, select, theta, changed, stream)

    def refused_noise(match, **changed):
        message = attempt(noise, changed)
        assert message is not None and match in message, f"not refused ({match}): {message}"
        torch.cuda.synchronize()
        assert _untouched(whole_theta), f"theta was written ({match})"

    for name in ("params", "gens", "consumed", "theta"):
        refused_noise("NULL argument", **{name: None})
    for name in ("params", "gens", "consumed", "select", "theta"):
        refused_noise("is not device memory", **{name: host.ctypes.data})
    refused_noise("must be in 1", groups=0)
    refused_noise("must be in 1", groups=65536)
    refused_noise("must be in 1", per_group=0)
    refused_noise("must be in 1", per_group=(1 << 20) + 1)
    refused_noise("not aligned", consumed=consumed.data_ptr() + 4)
    refused_noise("d_theta overlaps d_params", theta=params.data_ptr())
    refused_noise("outside the limits", desc=tuple(spec.critic_desc()[:-1]) + (2,))
    noise({})
    torch.cuda.synchronize()
    assert bits(theta.cpu().numpy()) == bits(theta_h) and _guards_kept(whole_theta)

    u = UPDATE
    rows, batch = u["steps"] * u["per_group"], 5
    device = _learner_of(torch, ctx, index, critic_lstm, u["groups"], u["steps"], u["per_group"], batch)[3]
    kept = device.outputs()
    firsts = torch.tensor(list(u["firsts"]), dtype=torch.int32, device="cuda")

    def update(changed, stream=None):
        device.enqueue(firsts, changed, stream)

    def refused_update(match, **changed):
        message = attempt(update, changed)
        assert message is not None and match in message, f"not refused ({match}): {message}"
        assert all(bits(x) == bits(y) for x, y in zip(device.outputs(), kept)), f"an output was written ({match})"

    assert (kept[2].view(np.uint32) == SENTINEL).all()
    big = np.zeros(1 << 16, dtype=F32)
    for name in ("hyper", "params", "state", "workspace", "obs", "actions", "log_probs", "advantages", "returns", "starts",
                 "states", "firsts", "stats"):
        refused_update("NULL argument", **{name: None})
        refused_update("is not device memory", **{name: big.ctypes.data})
    refused_update("must be in 1", groups=0)
    refused_update("must be in 1", groups=65536)
    refused_update("must be in 1", per_group=0)
    refused_update("must be in 1", steps=0)
    refused_update("B = ", batch=0)
    refused_update("B = ", batch=rows + 1)  # (B > m T)
    refused_update("B = ", batch=1025)
    refused_update("outside the limits", desc=tuple(spec.critic_desc()[:-1]) + (7,))
    refused_update("not aligned", firsts=device.parts["actions"].data_ptr() + 2)
    refused_update("not aligned", actions=device.parts["actions"].data_ptr() + 2)
    refused_update("not aligned", state=device.state.data_ptr() + 4)
    refused_update("d_stats overlaps d_params", stats=device.params.data_ptr())
    refused_update("d_workspace overlaps d_state", workspace=device.state.data_ptr())
    refused_update("d_stats overlaps d_lstm_states", stats=device.parts["lstm_states"].data_ptr())
    refused_update("d_params overlaps d_firsts", firsts=device.params.data_ptr())
    message = _capturing(torch, lambda stream: attempt(update, {}, stream))
    assert message is not None and "being captured" in message, message
    assert all(bits(x) == bits(y) for x, y in zip(device.outputs(), kept)), "a refused update wrote an output"
    want = twin_updates(index, critic_lstm, u["groups"], u["steps"], u["per_group"], u["firsts"], batch, u["updates"])
    _same_update(device.update(u["firsts"]), want[0], "after the refusals")
    assert device.guards_kept()
    desc = spec.critic_desc()
    assert ctx.lstm_sde_grouped_state_size(desc, 0, 3) == 0 and ctx.lstm_sde_grouped_state_size(desc, 65536, 1) == 0
    assert ctx.lstm_sde_grouped_state_size(tuple(desc[:-1]) + (2,), 3, 3) == 0
    assert ctx.lstm_sde_grouped_state_size(desc, 3, 3) == 3 * (32 + 8 * spec.size)
    for refused_shape in ((0, 3, 4, 5), (3, 0, 4, 5), (3, 3, 0, 5), (3, 3, 4, 13), (3, 3, 4, 0), (3, 400, 400, 1025)):
        assert ctx.lstm_sde_grouped_workspace_size(desc, *refused_shape) == 0, refused_shape


def one_group_case(torch, critic_lstm):
    """G = 1: noise, outputs, state, parameters and optimizer state after 3 chained updates and rng_state() equal the
    ungrouped DeviceLstmSdePolicy / DeviceLstmLearner bit for bit."""
    from reinfocus_amd.environments import harness

    n, steps = 11, 4
    env = harness.DeviceVectorContinuousJumps(num_envs=n, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        spec = e2e_spec(env, critic_lstm)
        width = spec.obs_width
        state = _cuda_states(torch, lsde_cases.state_dict(spec, 3))
        single = harness.DeviceLstmSdePolicy(env, spec, 77)
        grouped = harness.DevicePopulationLstmSdePolicy(env, spec, 1, [77])
        single.load_state_dict(state)
        grouped.load_state_dict(state)
        assert torch.equal(grouped.params[0], single.params)
        rng = np.random.default_rng(2)
        obs = torch.from_numpy(rng.standard_normal((n, width)).astype(F32)).cuda()
        starts = torch.from_numpy(rng.choice(np.array([0, 0, 1, 255], dtype=np.uint8), n)).cuda()
        for deterministic in (False, True, False):
            single.reset_noise()
            grouped.reset_noise()
            assert bits(grouped.noise().cpu().numpy()) == bits(single.noise().cpu().numpy())
            ours = [t.clone() for t in grouped.act(obs, starts, None, deterministic) if t is not None]
            theirs = [t for t in single.act(obs, starts, None, deterministic) if t is not None]
            assert len(ours) == len(theirs) == 4
            for x, y in zip(ours, theirs):
                assert bits(x.cpu().numpy()) == bits(y.cpu().numpy())
            assert grouped.rng_state() == [single.rng_state()]
            assert bits(grouped.lstm_state().cpu().numpy()) == bits(single.lstm_state().cpu().numpy())
            starts = torch.zeros_like(starts)
        assert bits(grouped.values(obs, starts).cpu().numpy()) == bits(single.values(obs, starts).cpu().numpy())
        assert grouped.lstm_state().abs().sum().item() > 0
        total = n * steps
        parts = {"observations": rng.standard_normal((total, width)).astype(F32),
                 "actions": (1.5 * rng.standard_normal(total)).astype(F32),
                 "log_probs": (-2.5 + 0.1 * rng.standard_normal(total)).astype(F32),
                 "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32),
                 "episode_starts": lstm_learner_cases.starts_of("drawn", steps, n),
                 "lstm_states": (0.5 * rng.standard_normal((steps + 1,) + spec.state_shape(n))).astype(F32)}
        parts = _cuda_states(torch, parts)
        parts.update(n_steps=steps, num_envs=n)
        kw = dict(learning_rate=1e-2, ent_coef=0.01)
        one, many = harness.DeviceLstmLearner(single, **kw), harness.DevicePopulationLearner(grouped, **kw)
        for update in range(3):
            first, count = (17 * update + 40) % total, 13 - update
            theirs = one.update(parts, first, count)
            ours = many.update(parts, [first], count)
            assert bits(ours[0].cpu().numpy()) == bits(theirs.cpu().numpy()), f"update {update}: stats differ"
        assert bits(grouped.params[0].cpu().numpy()) == bits(single.params.cpu().numpy())
        assert bits(many.state[0].cpu().numpy()) == bits(one.state.cpu().numpy())
        assert many.state_dict()["step"] == [3]
    finally:
        env.close()


def _same_runs(got, want):
    policy_cases.same_runs(got, want)


def e2e_promises(want):
    """The end-to-end run is not vacuous: group 0 (sde_sample_freq -1) keeps its theta over a rollout's steps while group 2
    (freq 1) draws anew, an environment ended, the states move, group 2 (learning rate 0) keeps its parameters."""
    groups, per_group, steps = E2E["groups"], E2E["per_group"], E2E["steps"]
    per_epoch = -(-steps * per_group // E2E["batch"])
    assert want[0]["stats"].shape == (E2E["epochs"] * per_epoch, groups, 8) and (want[1]["stats"][:, :, 7] == 0).all()
    assert bits(want[0]["params"][0]) != bits(want[1]["params"][0])
    assert bits(want[1]["params"][2]) == bits(want[0]["params"][2])  # (learning_rate 0)
    assert np.concatenate([run["truncated"] for run in want]).any(), "no environment ended"
    assert any(run["lstm_states"][1:].any() for run in want)
    assert want[0]["actions"].dtype == F32 and want[0]["flat/actions"].dtype == F32
    assert bits(want[0]["theta"][:per_group]) != bits(want[0]["theta"][per_group:2 * per_group])


def end_to_end_case(torch, critic_lstm):
    from reinfocus_amd.environments import harness

    want, want_rng, want_states, want_lstm = e2e_twin_runs(critic_lstm)
    groups = E2E["groups"]
    env = e2e_env(True)
    try:
        spec = e2e_spec(env, critic_lstm)
        make = lambda: harness.DevicePopulationLstmSdePolicy(env, spec, groups, seeds_of(groups),  # noqa: E731
                                                             log_std_init=E2E["log_std"])
        policy = make()
        for g, state in enumerate(e2e_states(spec)):
            policy.load_state_dict(_cuda_states(torch, state), group=g)
        learner = harness.DevicePopulationLearner(policy, **e2e_hypers())
        rollout = harness.DeviceRollout(env, E2E["steps"], GAMMA, GAE_LAMBDA)
        got = e2e_runs(rollout, policy, learner, lambda: env.reset_tensors()[0], lambda t: t.cpu().numpy())
        _same_runs(got, want)
        assert env.device_fault() is None
        assert policy.rng_state() == want_rng
        assert bits(learner.state.cpu().numpy()) == bits(want_states)
        assert bits(policy.lstm_state().cpu().numpy()) == bits(want_lstm)
        e2e_promises(want)
        # resume: a second policy and learner from both state_dict()s go on bit for bit, log_std included
        kept, kept_params = learner.state_dict(), [policy.state_dict(group=g) for g in range(groups)]
        assert all("log_std" in state for state in kept_params)
        splits = e2e_splits(9)
        straight = learner.train(rollout, E2E["epochs"], E2E["batch"], splits).clone()
        after = policy.params.clone()
        second_policy = make()
        for g in range(groups):
            second_policy.load_state_dict(kept_params[g], group=g)
        second_policy.set_rng_state(policy.rng_state())
        second_policy.set_lstm_state(policy.lstm_state())
        second_policy.set_noise(policy.noise())
        second = harness.DevicePopulationLearner(second_policy, **e2e_hypers())
        second.load_state_dict(kept)
        again = second.train(rollout, E2E["epochs"], E2E["batch"], splits=splits)
        assert torch.equal(again.view(torch.int32), straight.view(torch.int32))
        assert torch.equal(second_policy.params.view(torch.int32), after.view(torch.int32))
        assert torch.equal(second.state.view(torch.int32), learner.state.view(torch.int32))
        assert second_policy.rng_state() == policy.rng_state()
        drawn = second.train(rollout, 1, E2E["batch"], generator=np.random.default_rng(1))
        per_epoch = -(-E2E["steps"] * E2E["per_group"] // E2E["batch"])
        assert tuple(drawn.shape) == (per_epoch, groups, 8) and (drawn[:, :, 7] == 0).all()
    finally:
        env.close()


def surface_case(torch):
    """What the classes refuse, each with a message, the tensors unchanged afterwards and no draw consumed."""
    from reinfocus_amd.environments import harness

    env = e2e_env(True)
    steps_env = harness.DeviceVectorDiscreteSteps(num_envs=9, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        spec = e2e_spec(env)

        def raises(kind, match, call):
            try:
                call()
            except kind as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"not refused ({match})")

        make = harness.DevicePopulationLstmSdePolicy
        raises(ValueError, "not divisible", lambda: make(env, spec, 4, [1, 2, 3, 4]))
        raises(ValueError, "one seed per group", lambda: make(env, spec, 3, [1, 2]))
        raises(ValueError, "one seed per group", lambda: make(env, spec, 3, 7))
        raises(ValueError, "log_std_init has 2 entries", lambda: make(env, spec, 3, [1, 2, 3], log_std_init=[0.0, 1.0]))
        raises(ValueError, "Gaussian head over a Box", lambda: make(steps_env, spec, 3, [1, 2, 3]))
        raises(ValueError, "LstmSdePolicySpec", lambda: make(env, lstm_pop.e2e_spec(), 3, [1, 2, 3]))
        raises(ValueError, "LstmSdePolicySpec", lambda: make(env, harness.SdePolicySpec(spec.obs_width), 3, [1, 2, 3]))
        raises(ValueError, "next step", lambda: harness.DevicePopulationLstmPolicy(env, spec, 3, [1, 2, 3]))
        policy = make(env, spec, 3, [1, 2, 3], log_std_init=[-1.0, 0.0, 0.5])
        assert policy.spec.kind == "lstm_sde" and policy.groups == 3 and tuple(policy.params.shape) == (3, spec.size)
        assert policy.params[:, spec.log_std_at].tolist() == [-1.0, 0.0, 0.5]
        raises(TypeError, "DeviceLstmPolicy", lambda: harness.DeviceLstmLearner(policy))
        before = policy.rng_state()
        obs = torch.zeros((9, spec.obs_width), dtype=torch.float32, device="cuda")
        starts = torch.zeros(9, dtype=torch.uint8, device="cuda")
        raises(ValueError, "reset_noise() of every group", lambda: policy.act(obs, starts))
        raises(ValueError, "boolean sequence", lambda: policy.reset_noise(groups=[True, False]))
        raises(ValueError, "num_envs 8", lambda: policy.reset_noise(num_envs=8))
        assert policy.rng_state() == before and policy.noise() is None
        policy.reset_noise(groups=[True, False, True])
        raises(ValueError, "reset_noise() of every group", lambda: policy.act(obs, starts))
        policy.reset_noise(groups=[False, True, False])
        after = policy.rng_state()
        assert after != before and policy.noise() is not None
        raises(ValueError, "rows", lambda: policy.act(obs[:8].contiguous(), starts[:8].contiguous()))
        raises(ValueError, "episode_starts is", lambda: policy.act(obs, starts[:8].contiguous()))
        raises(ValueError, "states[1] is", lambda: policy.act(obs, starts, states=(policy.lstm_state(), obs)))
        raises(ValueError, "theta must be", lambda: policy.set_noise(obs))
        raises(ValueError, "generator states", lambda: policy.set_rng_state(before[:2]))
        raises(IndexError, "group 3", lambda: policy.state_dict(group=3))
        assert policy.rng_state() == after
        learner = harness.DevicePopulationLearner(policy)
        rollout = harness.DeviceRollout(env, 2)
        rollout.start(env.reset_tensors()[0])
        raises(ValueError, "sde_sample_freq has 2 entries", lambda: rollout.collect(policy, sde_sample_freq=[1, 2]))
        raises(ValueError, "is not -1 or a positive integer", lambda: rollout.collect(policy, sde_sample_freq=[1, 0, 2]))
        assert policy.rng_state() == after
        rollout.collect(policy, sde_sample_freq=[-1, 2, 1])
        kept = policy.params.clone()
        raises(ValueError, "more than the 6 rows", lambda: learner.train(rollout, 1, 7))
        raises(ValueError, "batch_size", lambda: learner.train(rollout, 1, 1025))
        raises(ValueError, "splits must be", lambda: learner.train(rollout, 2, 4, [[0, 1, 2]]))
        raises(ValueError, "splits must be", lambda: learner.train(rollout, 1, 4, [[0, 1, 6]]))
        raises(ValueError, "firsts must be", lambda: learner.update(rollout, [0, 1], 4))
        raises(ValueError, "firsts must be", lambda: learner.update(rollout, [0, 1, 6], 4))
        raises(ValueError, "a minibatch of 7", lambda: learner.update(rollout, [0, 1, 2], 7))
        raises(TypeError, "firsts, count", lambda: learner.update(rollout, [0, 1, 2]))
        other = harness.DeviceRollout(env, 2, groups=9)
        raises(ValueError, "groups=9", lambda: other.start(env.reset_tensors()[0]) or other.collect(policy))
        plain = harness.DeviceSdePopulationPolicy(env, harness.SdePolicySpec(spec.obs_width, pi=(6,), vf=(5,)), 3, [1, 2, 3])
        flat_rollout = harness.DeviceRollout(env, 2)
        flat_rollout.start(env.reset_tensors()[0])
        flat_rollout.collect(plain)
        raises(ValueError, "no lstm_states", lambda: learner.train(flat_rollout, 1, 4))
        host_env = e2e_env(False)
        try:
            twin = harness.LstmSdePopulationPolicy(spec, 3, [1, 2, 3], num_envs=9)
            host_rollout = harness.Rollout(host_env, 2)
            host_rollout.start(host_env.reset()[0])
            host_rollout.collect(twin)
            raises(ValueError, "the host", lambda: learner.train(host_rollout, 1, 2))
        finally:
            host_env.close()
        torch.cuda.synchronize()
        assert torch.equal(policy.params, kept)
        stats = learner.train(rollout, 1, 4, [[0, 5, 3]])
        assert tuple(stats.shape) == (2, 3, 8)
    finally:
        env.close()
        steps_env.close()


def sharded_case(torch):
    from reinfocus_amd.environments import harness

    env = harness.ShardedVectorContinuousJumps(num_envs=9, devices=[0], frame_height=16, samples_per_pixel=1, seed=1)
    try:
        try:
            harness.DevicePopulationLstmSdePolicy(env, e2e_spec(env), 3, [1, 2, 3])
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
    for critic_lstm in CRITICS:
        critic = critic_name(critic_lstm)
        for index in NETS:
            with record.case(f"noise/{critic}/{index}"):
                noise_case(torch, ctx, index, critic_lstm)
            for groups in GROUPS:
                for per_group in PER_GROUP:
                    with record.case(f"forward/{critic}/{index}/{groups}/{per_group}"):
                        forward_case(torch, ctx, index, critic_lstm, groups, per_group)
            with record.case(f"stride/{critic}/{index}"):
                stride_case(torch, ctx, index, critic_lstm)
            for batch in UPDATE["batches"]:
                with record.case(f"update/{critic}/{index}/{batch}"):
                    update_case(torch, ctx, index, critic_lstm, batch)
        with record.case(f"isolation/{critic}"):
            isolation_case(torch, ctx, critic_lstm)
        with record.case(f"depth/{critic}"):
            depth_case(torch, ctx, critic_lstm)
    with record.case("update/wide"):
        wide_update_case(torch, ctx)
    with record.case("limit"):
        limit_case(torch, ctx)
    for critic_lstm in CRITICS:
        with record.case(f"group-limit/{critic_name(critic_lstm)}"):
            group_limit_case(torch, ctx, critic_lstm)
    with record.case("kernel-refusals"):
        kernel_refusal_case(torch, ctx)
    ctx.close()
    for critic_lstm in CRITICS:
        with record.case(f"one-group/{critic_name(critic_lstm)}"):
            one_group_case(torch, critic_lstm)
        with record.case(f"end-to-end/{critic_name(critic_lstm)}"):
            end_to_end_case(torch, critic_lstm)
    with record.case("surface"):
        surface_case(torch)
    with record.case("sharded"):
        sharded_case(torch)
    with record.case("finished"):
        pass


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    run_cases(sys.argv[1])
