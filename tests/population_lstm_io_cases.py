"""TEST INFRASTRUCTURE: what tests/test_population_lstm_logic.py and tests/test_gpu_population_lstm.py share -- the
networks, the group shapes, the numpy twins' results (computed once and shared) -- and the child process of the GPU file.

As tests/population_io_cases.py: everything that needs torch and the library together runs in one fresh process that imports
torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.population_lstm_io_cases <results.jsonl>
"""

import ctypes
import functools
import os
import sys

import numpy as np

from tests import lstm_io_cases as lstm_cases
from tests import lstm_learner_io_cases as lstm_learner_cases
from tests import policy_io_cases as policy_cases
from tests import population_io_cases as population_cases
from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = policy_cases.bits
SENTINEL, SENTINEL64 = policy_cases.SENTINEL, policy_cases.SENTINEL64
GAMMA, GAE_LAMBDA = rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA
seeds_of, advanced_states, group_hypers, twin_states = (population_cases.seeds_of, population_cases.advanced_states,
                                                        population_cases.group_hypers, population_cases.twin_states)

# lstm_io_cases.NETWORKS: the least network, ppo_lstm_tuned.yml's (H = 16), widths that are no multiple of a wave with the
# most actions (H = 65, 64 actions); DEFAULT (H = 256) runs once, at the limit
NETS = (0, lstm_cases.TUNED, 3)
CRITICS = (True, False)  # enable_critic_lstm
GROUPS = (1, 3)
PER_GROUP = (3, 8, 11)  # a group border inside what would be an ungrouped tile; exactly one tile; a ragged second tile
CONSUMED = (0, 2 ** 32 + 5)
STRIDE = (3, 3)  # (G, m) of the state-plane stride case
WIDE_FORWARD = ((512, 1), (65, 8))
UPDATE = dict(groups=3, steps=4, per_group=3, firsts=(0, 7, 11), batches=(5, 12), updates=2)
LIMIT = dict(index=lstm_cases.DEFAULT, groups=2, steps=3, per_group=2, batch=6, firsts=(0, 4))
WIDE_UPDATE = dict(index=lstm_cases.TUNED, groups=64, steps=8, per_group=8, batch=8)
E2E = dict(groups=3, per_group=3, steps=4, epochs=2, batch=5, iterations=2)
# the grouped update on lstm_learner_io_cases.LIMIT_LAYOUTS, whose (T, m, starts kind, _, B) each entry takes; every group
# has its own first row (update u starts at firsts + u) and, by group_starts' roll, its own sequence structure:
#   depth/    T = 17, m = 4: sequences of 1, 8, 9, 16 and 17 rows.  G = 3 on the tuned network at B = 65 and at B = 68 = N,
#             where two groups wrap at different rows (these two also as G stand-alone launches); G = 2 on sb3-contrib's
#             default network (H = 256: every thread of a block owns a unit) at B = 65
#   untuned/  ppo_lstm_untuned.yml's T = 128, m = 8, B = 128, drawn starts: group 1 crosses an environment boundary, group 2
#             wraps; every group has a sequence of more than 64 rows and one of one row.  G = 3 on the tuned network, and
#             G = 2 on the default network with the LSTM critic (the real shape)
#   wave/     T = 16, m = 64, N = 1024, G = 2 on the tuned network: every row a start at B = 1024 (1024 one-row sequences
#             per group, 128 MLP tiles, the second trip of the reductions), no flagged start at B = 513
# updates: two consecutive ones (the second reads the optimizer header the first wrote) where the numpy twin is cheap, one
# at the 1024-row layouts and at H = 256 over 128 steps, whose twins cost seconds each
LAYOUT_CASES = {
    "depth/65": dict(layout="depth/0/65", index=lstm_cases.TUNED, critics=CRITICS, firsts=(0, 5, 30), updates=2, alone=True),
    "depth/68": dict(layout="depth/5/68", index=lstm_cases.TUNED, critics=CRITICS, firsts=(5, 0, 67), updates=2, alone=True),
    "depth/65/default": dict(layout="depth/0/65", index=lstm_cases.DEFAULT, critics=CRITICS, firsts=(0, 5), updates=2,
                             alone=False),
    "untuned": dict(layout="untuned/0/128", index=lstm_cases.TUNED, critics=CRITICS, firsts=(0, 100, 1000), updates=2,
                    alone=False),
    "untuned/default": dict(layout="untuned/0/128", index=lstm_cases.DEFAULT, critics=(True,), firsts=(0, 100), updates=1,
                            alone=False),
    "wave/1024": dict(layout="wave/7/1024", index=lstm_cases.TUNED, critics=CRITICS, firsts=(7, 0), updates=1, alone=False),
    "wave/513": dict(layout="wave/0/513", index=lstm_cases.TUNED, critics=CRITICS, firsts=(0, 9), updates=1, alone=False)}
LAYOUT_KINDS = ("depth", "drawn")  # the kinds whose sequence lengths are the point: group_starts adds no start to them
# the seed of the drawn starts: the first with which all three groups -- rolled by g, from rows 0, 100 and 1000 -- hold a
# sequence of more than 64 rows and one of one row in both updates (lstm_learner_io_cases.DRAWN_SEED gives group 2 neither)
DRAWN_SEED = 69
# the group limit: RF_POPULATION_MAX_GROUPS groups of m = T = B = 1 on the least network, by population_io_cases' scheme:
# group g has parameter set g % 7, input block g % 5 (its state on level g % 5) and hyper-parameter set g % 3; a sampled
# forward draws from generator g % 11; firsts[g] = 1 = N (outside) where g % 11 = 5
LIMIT_GROUPS, LIMIT_PERIODS, LIMIT_GENERATORS = 65535, (7, 5, 3), 11
LIMIT_STARTS = (0, 0, 1, 0, 255)  # the start byte of block j: three of the five levels are read through the state
LIMIT_OUTSIDE = (11, 5)  # g % 11 == 5
INVALID, NONFINITE = 1, 2  # RF_PPO_INVALID, RF_PPO_NONFINITE


def spec_of(index, critic_lstm):
    from reinfocus_amd.environments import lstm

    width, hidden, pi, vf, actions, activation = lstm_cases.NETWORKS[index]
    return lstm.LstmPolicySpec(width, actions, lstm_hidden=hidden, pi=pi, vf=vf, activation=activation,
                               enable_critic_lstm=critic_lstm)


def group_params(spec, groups, base):
    """float32 [G][P]: every group its own parameters (hostile: logits that tie and one 200 below)."""
    return np.stack([spec.pack(lstm_cases.state_dict(spec, base + 17 * g, hostile=True)) for g in range(groups)])


def twin_policy(index, critic_lstm, groups, base=100):
    from reinfocus_amd.environments import harness

    spec = spec_of(index, critic_lstm)
    twin = harness.LstmPopulationPolicy(spec, groups, seeds_of(groups))
    twin.params[...] = group_params(spec, groups, base + index)
    return spec, twin


# ---- forward ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_inputs(index, groups, per_group):
    """(obs [n, D], final_obs (NaN-led rows among live ones), starts uint8 [n] -- bytes 0, 1, 2, 255 mixed --, state
    [2, 2, n, H]: normal values, every group around its own non-zero level g + 1)."""
    width, hidden = lstm_cases.NETWORKS[index][:2]
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
def wanted_forward(index, critic_lstm, groups, per_group, consumed, deterministic):
    """The twin population's (actions, values, log_probs, final_values, state after) with every generator advanced by
    `consumed` before.  Computed once, shared, never changed."""
    spec, twin = twin_policy(index, critic_lstm, groups)
    obs, final_obs, starts, state = forward_inputs(index, groups, per_group)
    twin.set_rng_state(advanced_states(groups, consumed))
    after = np.full_like(state, np.nan)
    with np.errstate(all="ignore"):
        got = twin.act(obs, starts, final_obs, deterministic, states=(state.copy(), after))
        values = twin_values(twin, obs, starts, final_obs, state)
    return got + (after,), values


def twin_values(twin, obs, starts, final_obs, state):
    twin.set_lstm_state(state)
    return twin.values(obs, starts, final_obs)


def regrouped_state(state, groups, per_group):
    """The mistake the stride case must catch: the bytes of a state [2][2][n][H] read as [G][2][2][m][H]."""
    hidden = state.shape[-1]
    wrong = state.reshape(groups, 2, 2, per_group, hidden)
    return np.ascontiguousarray(np.concatenate([wrong[g] for g in range(groups)], axis=2))


# ---- update ----------------------------------------------------------------------------------------------------------------
def group_starts(groups, steps, per_group, kind="mixed"):
    """uint8 [T + 1][G m]: lstm_learner_io_cases.starts_of per group (drawn: from DRAWN_SEED), group g's columns rolled by g
    and -- but for LAYOUT_KINDS -- its bytes changed, so the sequence structure differs per group."""
    columns = []
    for g in range(groups):
        if kind == "some":  # (any shape: environment 0 starts at t = 0, environment 1 at the last step)
            piece = np.zeros((steps + 1, per_group), dtype=np.uint8)
            piece[0, 0], piece[steps - 1, per_group - 1] = 1, 255
        else:
            piece = lstm_learner_cases.starts_of(kind, steps, per_group, seed=DRAWN_SEED)
        piece = np.roll(piece, g, axis=1)
        if g % 3 == 2 and steps > 1 and kind not in LAYOUT_KINDS:
            piece[1, 0] = 2  # (one more start, in the middle of environment 0's rows)
        columns.append(piece)
    return np.concatenate(columns, axis=1)


@functools.lru_cache(maxsize=None)
def update_inputs(index, critic_lstm, groups, steps, per_group, kind="mixed"):
    """(spec, twin population with per-group parameters, parts dict over G m lanes as parts_of(rollout) hands it over)."""
    from reinfocus_amd.environments import learner

    spec, twin = twin_policy(index, critic_lstm, groups, base=300)
    lanes, rows = groups * per_group, steps * per_group
    total = groups * rows
    rng = np.random.default_rng(1000 * index + total)
    starts = group_starts(groups, steps, per_group, kind)
    states = (0.5 * rng.standard_normal((steps + 1,) + spec.state_shape(lanes))).astype(F32)
    parts = {"observations": lstm_learner_cases.learner_cases.finite_rows(spec.obs_width, total, 77 * index + total),
             "actions": rng.integers(0, spec.n_actions, total).astype(np.int64),
             "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32),
             "values": np.zeros(total, dtype=F32), "episode_starts": starts, "lstm_states": states, "n_steps": steps,
             "num_envs": lanes}
    shifts = np.array(lstm_learner_cases.SHIFTS, dtype=F32)[np.arange(total) % len(lstm_learner_cases.SHIFTS)]
    own = np.zeros(total, dtype=F32)
    for g in range(groups):
        piece = group_slices(parts, groups, g)
        own[g * rows:(g + 1) * rows] = lstm_learner_cases.own_log_probs(
            spec, twin.params[g], piece, piece["episode_starts"], piece["lstm_states"], steps, per_group)
    parts["log_probs"] = (own - shifts).astype(F32)
    assert set(learner.BATCH_KEYS) <= set(parts)
    return spec, twin, parts


def group_slices(parts, groups, g):
    """Group g's parts as CONTIGUOUS COPIES: what a stand-alone learner over the group's m lanes is handed."""
    steps, lanes = parts["n_steps"], parts["num_envs"]
    m = lanes // groups
    rows = m * steps
    out = {key: np.ascontiguousarray(value[g * rows:(g + 1) * rows]) for key, value in parts.items()
           if isinstance(value, np.ndarray) and key not in ("episode_starts", "lstm_states")}
    out.update(episode_starts=np.ascontiguousarray(parts["episode_starts"][:, g * m:(g + 1) * m]),
               lstm_states=np.ascontiguousarray(parts["lstm_states"][:, :, :, g * m:(g + 1) * m, :]), n_steps=steps, num_envs=m)
    return out


def hypers_of(groups):
    return group_hypers(groups) if groups <= 3 else population_cases.wide_hypers(groups)


def fresh_twin(spec, twin):
    """A copy of the twin population (the cached one is never changed)."""
    from reinfocus_amd.environments import harness

    copy = harness.LstmPopulationPolicy(spec, twin.groups, seeds_of(twin.groups))
    copy.params[...] = twin.params
    return copy


@functools.lru_cache(maxsize=None)
def twin_updates(index, critic_lstm, groups, steps, per_group, firsts, batch, updates, kind="mixed"):
    """Per consecutive update (params [G][P], states [G][S], stats [G][8]) of the twin population, update u from first rows
    (firsts + u) mod m T.  Computed once, shared, never changed."""
    from reinfocus_amd.environments import harness

    spec, twin, parts = update_inputs(index, critic_lstm, groups, steps, per_group, kind)
    twin = fresh_twin(spec, twin)
    learner = harness.PopulationLearner(twin, **hypers_of(groups))
    seen = []
    with np.errstate(all="ignore"):
        for update in range(updates):
            stats = learner.update(parts, firsts_of(firsts, update, steps * per_group), batch)
            seen.append((twin.params.copy(), twin_states(learner), stats))
    return seen


def firsts_of(firsts, update, rows):
    return [(first + update) % rows for first in firsts]


def wide_firsts():
    rows = WIDE_UPDATE["steps"] * WIDE_UPDATE["per_group"]
    return tuple((7 * g) % rows for g in range(WIDE_UPDATE["groups"]))


def layout_shape(name, critic_lstm):
    """(index, critic_lstm, G, T, m), kind, firsts, B of a case of LAYOUT_CASES."""
    case = LAYOUT_CASES[name]
    steps, per_group, kind, _, batch = lstm_learner_cases.LIMIT_LAYOUTS[case["layout"]]
    return (case["index"], critic_lstm, len(case["firsts"]), steps, per_group), kind, case["firsts"], batch


def layout_twin_updates(name, critic_lstm):
    shape, kind, firsts, batch = layout_shape(name, critic_lstm)
    return twin_updates(*shape, firsts, batch, LAYOUT_CASES[name]["updates"], kind)


def layout_update_promises(name, critic_lstm):
    """No comparison of a layout case is vacuous: every group is taken in every update (flags 0), every group whose
    learning rate is not 0 ends with other parameters than it began with (the one whose is 0 with the same), parameters
    differ per group and every hyper-parameter between neighbours."""
    from reinfocus_amd.environments import harness

    shape, kind, firsts, batch = layout_shape(name, critic_lstm)
    spec, twin, _ = update_inputs(*shape, kind)
    want = layout_twin_updates(name, critic_lstm)
    assert len(want) == LAYOUT_CASES[name]["updates"] and all((stats[:, 7] == 0).all() for _, _, stats in want)
    hypers = harness.PopulationLearner(fresh_twin(spec, twin), **hypers_of(shape[2])).hypers()
    assert len({bits(row) for row in twin.params}) == shape[2]
    for one, other in zip(hypers, hypers[1:]):
        assert all(x != y for x, y in zip(one, other))
    assert [h.learning_rate == 0 for h in hypers] == [g == 1 for g in range(shape[2])]
    for g, h in enumerate(hypers):
        assert (bits(want[-1][0][g]) == bits(twin.params[g])) == (h.learning_rate == 0), f"group {g}"
    if len(want) > 1:  # (the optimizer header and moments the first wrote, the second read)
        assert bits(want[0][1]) != bits(want[1][1])


# ---- the limit: 65535 groups of one environment, one step ---------------------------------------------------------------
def limit_spec(critic_lstm):
    return spec_of(0, critic_lstm)


@functools.lru_cache(maxsize=None)
def limit_parts(critic_lstm):
    """(7 packed parameter sets; 5 input blocks of one row -- obs, final_obs, start byte, state [2][2][1][1] around level
    0.125 (1 + j) (every plane its own value), action, log_prob, advantage, return, the rollout's stored states
    [2][2][2][1][1] --; 3 hyper-parameter sets; 11 generators).  adam_eps is large, so the first Adam step depends on the
    gradient's size."""
    from reinfocus_amd.environments import learner

    spec = limit_spec(critic_lstm)
    rng = np.random.default_rng(65535)
    params = [np.abs(spec.pack(lstm_cases.state_dict(spec, 700 + k))) + F32(0.25 + 0.125 * k) for k in range(LIMIT_PERIODS[0])]
    blocks = []
    for j in range(LIMIT_PERIODS[1]):
        level = F32(0.125 * (1 + j)) + F32(0.03125) * np.arange(4, dtype=F32).reshape(2, 2, 1, 1)
        blocks.append(dict(observations=np.array([[0.5 + 0.75 * j]], dtype=F32), final=np.array([[3.0 - 0.5 * j]], dtype=F32),
                           starts=np.array([LIMIT_STARTS[j]], dtype=np.uint8), state=level.astype(F32),
                           actions=np.array([j % 2], dtype=np.int64), log_probs=np.array([-0.7 + 0.1 * j], dtype=F32),
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
    """By the existing twin functions.  forwards[deterministic][k][j][i]: (actions, values, log_probs, final_values, next
    state [2][2][1][1]) of parameter set k on block j with the draw of generator i after CONSUMED[1] draws; updates[c]: the
    first update's (params, state, stats) of combination c (k = c % 7, j = c % 5, h = c % 3) from a fresh optimizer."""
    from reinfocus_amd.environments import learner, lstm, lstm_learner

    spec = limit_spec(critic_lstm)
    params, blocks, hypers, generators = limit_parts(critic_lstm)
    draws = []
    for generator in generators:
        moved = np.random.PCG64DXSM()
        moved.state = generator.state
        draws.append(np.random.Generator(moved.advance(CONSUMED[1])).random(1)[0])
    forwards = {}
    for deterministic in (False, True):
        forwards[deterministic] = [[[None] * LIMIT_GENERATORS for _ in blocks] for _ in params]
        for k, packed in enumerate(params):
            for j, block in enumerate(blocks):
                for i, u in enumerate(draws):
                    got = lstm.lstm_numpy(spec, packed, block["observations"], block["starts"], block["state"], block["final"],
                                          None if deterministic else np.array([u]), deterministic)
                    forwards[deterministic][k][j][i] = tuple(got[name] for name in ORDER) + (got["state"],)
    updates = []
    for c in range(105):
        k, j, h = (c % period for period in LIMIT_PERIODS)
        batch = {key: blocks[j][key] for key in learner.BATCH_KEYS}
        updates.append(lstm_learner.lstm_update_numpy(spec, params[k], learner.fresh_state(spec), batch,
                                                      blocks[j]["episode_starts"], blocks[j]["lstm_states"], 1, 1, 0, 1, hypers[h]))
    return forwards, updates


def limit_arrays(critic_lstm, groups=LIMIT_GROUPS):
    """What group g gets and what it must give, for g = 0 .. groups - 1: (inputs dict -- the forward's arrays, the update's
    parts, "firsts", "outside" (where firsts[g] = N), "hyper", "gens" --, {deterministic: wanted (actions, values,
    log_probs, final_values, state [2][2][G][1])}, wanted (params [G][P], states [G][S], stats [G][8]) of the groups that
    are inside)."""
    from reinfocus_amd.environments import learner, policy, population

    params, blocks, hypers, generators = limit_parts(critic_lstm)
    forwards, updates = limit_results(critic_lstm)
    g = np.arange(groups)
    k, j, h, c, i = g % LIMIT_PERIODS[0], g % LIMIT_PERIODS[1], g % LIMIT_PERIODS[2], g % 105, g % LIMIT_GENERATORS
    outside = g % LIMIT_OUTSIDE[0] == LIMIT_OUTSIDE[1]
    inputs = {"params": np.stack(params)[k], "hyper": population.hyper_records(hypers)[h], "outside": outside,
              "firsts": outside.astype(np.int32),
              "gens": np.array([policy.generator_words(generator) for generator in generators], dtype=np.uint64)[i]}
    for key in ("observations", "final", "starts") + tuple(key for key in learner.BATCH_KEYS if key != "observations"):
        inputs[key] = np.concatenate([block[key] for block in blocks])[j]
    inputs["state"] = np.ascontiguousarray(np.concatenate([block["state"] for block in blocks], axis=2)[:, :, j, :])
    inputs["episode_starts"] = np.ascontiguousarray(np.concatenate([block["episode_starts"] for block in blocks], axis=1)[:, j])
    inputs["lstm_states"] = np.ascontiguousarray(np.concatenate([block["lstm_states"] for block in blocks], axis=3)[:, :, :, j, :])
    at = (k * len(blocks) + j) * LIMIT_GENERATORS + i  # (the place of (k, j, i) in a table's order)
    wanted_forward = {}
    for deterministic, table in forwards.items():
        results = [result for per_set in table for per_block in per_set for result in per_block]
        wanted_forward[deterministic] = tuple(np.concatenate([result[part] for result in results])[at] for part in range(4)) + (
            np.ascontiguousarray(np.concatenate([result[4] for result in results], axis=2)[:, :, at, :]),)
    wanted_update = tuple(np.stack([update[part] for update in updates])[c] for part in range(3))
    return inputs, wanted_forward, wanted_update


def hostcheck():
    from tests import helpers

    lib = ctypes.CDLL(helpers.built("tests/lstmpopcheck", "liblstmpopcheck.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.lpop_state_size.restype = lib.lpop_workspace_size.restype = lib.lpop_state_at.restype = ctypes.c_ulonglong
    lib.lpop_state_size.argtypes = [vp, i32, i32]
    lib.lpop_workspace_size.argtypes = [vp, i32, i32, i32, i32]
    lib.lpop_first.argtypes = [i32, i32, vp]
    lib.lpop_sequences.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.lpop_state_at.argtypes = [i32] * 9
    return lib


def critic_desc(spec):
    from reinfocus_amd import _native

    return _native.LstmCriticDesc(*spec.critic_desc())


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
def e2e_env(device_form):
    from reinfocus_amd.environments import harness

    n = E2E["groups"] * E2E["per_group"]
    if device_form:
        return harness.DeviceVectorDiscreteSteps(num_envs=n, device_initializer=True, episode_records=True,
                                                 **rollout_cases.ENV_KW)
    return harness.VectorDiscreteSteps(num_envs=n, episode_records=True, **rollout_cases.ENV_KW)


def e2e_spec(critic_lstm=True):
    from reinfocus_amd.environments import lstm

    return lstm.LstmPolicySpec(4, 13, lstm_hidden=9, pi=(6,), vf=(5, 7), activation="tanh", enable_critic_lstm=critic_lstm)


def e2e_states(spec):
    return [lstm_cases.state_dict(spec, 500 + 17 * g) for g in range(E2E["groups"])]


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
        rollout.collect(policy)
        record = policy_cases.slabs_of(rollout, unwrap)
        record["episode_starts"], record["lstm_states"] = unwrap(rollout.episode_starts), unwrap(rollout.lstm_states)
        record["stats"] = unwrap(learner.train(rollout, E2E["epochs"], E2E["batch"], e2e_splits(iteration)))
        record["params"] = unwrap(policy.params)
        seen.append(record)
    return seen


@functools.lru_cache(maxsize=None)
def e2e_twin_runs(critic_lstm=True):
    from reinfocus_amd.environments import harness

    env = e2e_env(False)
    try:
        spec = e2e_spec(critic_lstm)
        policy = harness.LstmPopulationPolicy(spec, E2E["groups"], seeds_of(E2E["groups"]))
        for g, state in enumerate(e2e_states(spec)):
            policy.load_state_dict(state, group=g)
        learner = harness.PopulationLearner(policy, **e2e_hypers())
        rollout = harness.Rollout(env, E2E["steps"], GAMMA, GAE_LAMBDA)
        runs = e2e_runs(rollout, policy, learner, lambda: env.reset()[0], np.array)
        return runs, policy.rng_state(), twin_states(learner), policy.lstm_state()
    finally:
        env.close()


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
ORDER = ("actions", "values", "log_probs", "final_values")
_untouched = policy_cases._untouched


def _guarded(torch, n):
    whole = {name: torch.full((n + 2,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
             for name in ("log_probs", "values", "final_values")}
    whole["actions"] = torch.full((n + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
    return whole, {name: tensor[1:n + 1] for name, tensor in whole.items()}


def _guarded_floats(torch, host):
    """A device copy of `host` between two guard floats: (whole, the copy's view)."""
    flat = np.asarray(host, dtype=F32).reshape(-1)
    whole = torch.full((flat.size + 2,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    whole[1:-1].copy_(torch.from_numpy(flat))
    return whole, whole[1:-1].view(tuple(np.asarray(host).shape))


def _guards_kept(whole):
    return _untouched(whole[0]) and _untouched(whole[-1])


def _table(torch, groups, consumed=0):
    from reinfocus_amd.environments import policy

    words = []
    for state in advanced_states(groups, consumed):
        generator = np.random.PCG64DXSM()
        generator.state = state
        words.append(policy.generator_words(generator))
    return torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).cuda()


def _forward(torch, ctx, spec, groups, per_group, params, obs, starts, final_obs, state_in, state_out, table, consumed, flags,
             out, changed=(), stream=None):
    pointer = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = dict(desc=spec.critic_desc(), groups=groups, per_group=per_group, params=params.data_ptr(), obs=obs.data_ptr(),
             starts=starts.data_ptr(), final_obs=pointer(final_obs), state_in=state_in.data_ptr(),
             state_out=pointer(state_out), gens=pointer(table), consumed=consumed, flags=flags)
    a.update({name: pointer(tensor) for name, tensor in out.items()})
    a.update(changed)
    ctx.lstm_forward_grouped(a["desc"], a["groups"], a["per_group"], a["params"], a["obs"], a["starts"], a["final_obs"],
                             a["state_in"], a["state_out"], a["gens"], a["consumed"], a["flags"], a["actions"],
                             a["log_probs"], a["values"], a["final_values"], None,
                             torch.cuda.current_stream().cuda_stream if stream is None else stream)


def forward_case(torch, ctx, index, critic_lstm, groups, per_group, alone=True):
    """rf_lstm_forward_grouped against the twin population as bytes: sampled at both draw counts and deterministic, the
    state in place and from `in` to `out`, values only (the state stays); every output a slice of a larger slab and the
    states between guard floats; then G stand-alone rf_lstm_forward / rf_lstm_critic_forward launches on contiguous copies."""
    from reinfocus_amd.environments import policy

    spec, twin = twin_policy(index, critic_lstm, groups)
    n = groups * per_group
    obs_h, final_h, starts_h, state_h = forward_inputs(index, groups, per_group)
    params, obs, final_obs, starts = (torch.from_numpy(a).cuda() for a in (twin.params, obs_h, final_h, starts_h))
    table = _table(torch, groups)
    for consumed, deterministic, in_place in ((CONSUMED[0], False, True), (CONSUMED[1], False, False), (0, True, False)):
        want, _ = wanted_forward(index, critic_lstm, groups, per_group, consumed, deterministic)
        whole, out = _guarded(torch, n)
        whole_in, state_in = _guarded_floats(torch, state_h)
        whole_out, state_out = (whole_in, state_in) if in_place else _guarded_floats(torch, np.full_like(state_h, np.nan))
        _forward(torch, ctx, spec, groups, per_group, params, obs, starts, final_obs, state_in, state_out, table, consumed,
                 policy.DETERMINISTIC if deterministic else 0, out)
        torch.cuda.synchronize()
        what = f"consumed {consumed}, deterministic {deterministic}, in place {in_place}"
        for name, wanted in zip(ORDER, want):
            assert bits(out[name].cpu().numpy()) == bits(wanted), f"{what}: {name} differ"
            assert _untouched(whole[name][0]) and _untouched(whole[name][n + 1]), f"a guard row of {name} was written"
        assert bits(state_out.cpu().numpy()) == bits(want[4]), f"{what}: the state differs"
        assert _guards_kept(whole_in) and _guards_kept(whole_out), "a guard float of a state was written"
        if not in_place:
            assert bits(state_in.cpu().numpy()) == bits(state_h), "state_in was written"
    _, values = wanted_forward(index, critic_lstm, groups, per_group, 0, True)
    whole, out = _guarded(torch, n)
    out.update(actions=None, log_probs=None)
    whole_in, state_in = _guarded_floats(torch, state_h)
    _forward(torch, ctx, spec, groups, per_group, params, obs, starts, final_obs, state_in, None, None, 0, 0, out)
    torch.cuda.synchronize()
    assert bits(out["values"].cpu().numpy()) == bits(values[0]) and bits(out["final_values"].cpu().numpy()) == bits(values[1])
    assert _untouched(whole["actions"]) and _untouched(whole["log_probs"]) and bits(state_in.cpu().numpy()) == bits(state_h)
    if not alone:
        return
    consumed = CONSUMED[1]
    want, _ = wanted_forward(index, critic_lstm, groups, per_group, consumed, False)
    got = {name: torch.zeros(n, dtype=torch.int64 if name == "actions" else torch.float32, device="cuda") for name in ORDER}
    states_out = []
    stream = torch.cuda.current_stream().cuda_stream
    forward = ctx.lstm_forward if critic_lstm else ctx.lstm_critic_forward
    desc = spec.desc() if critic_lstm else spec.critic_desc()
    for g, state in enumerate(advanced_states(groups, consumed)):
        generator = np.random.PCG64DXSM()
        generator.state = state
        rows = slice(g * per_group, (g + 1) * per_group)
        piece_in = torch.from_numpy(np.ascontiguousarray(state_h[:, :, rows, :])).cuda()
        piece_out = torch.zeros_like(piece_in)
        forward(desc, params[g].data_ptr(), per_group, obs[rows].data_ptr(), starts[rows].data_ptr(),
                final_obs[rows].data_ptr(), piece_in.data_ptr(), piece_out.data_ptr(), policy.generator_words(generator), 0,
                got["actions"][rows].data_ptr(), got["log_probs"][rows].data_ptr(), got["values"][rows].data_ptr(),
                got["final_values"][rows].data_ptr(), None, stream)
        states_out.append(piece_out)
    torch.cuda.synchronize()
    for name, wanted in zip(ORDER, want):
        assert bits(got[name].cpu().numpy()) == bits(wanted), f"stand-alone launches: {name} differ"
    assert bits(torch.cat(states_out, dim=2).cpu().numpy()) == bits(want[4]), "stand-alone launches: the state differs"


def stride_case(torch, ctx, index, critic_lstm):
    """G = 3, m = 3 with a distinct non-zero state per group: the grouped launch equals the twin (forward_case), and the
    twin over the same bytes read as [G][2][2][m][H] gives another next state, other log-probabilities (more than two
    actions) and, with the LSTM critic, other values -- so a kernel that added g * size to the state pointer could not pass."""
    groups, per_group = STRIDE
    forward_case(torch, ctx, index, critic_lstm, groups, per_group, alone=False)
    spec, twin = twin_policy(index, critic_lstm, groups)
    obs, final_obs, starts, state = forward_inputs(index, groups, per_group)
    want, _ = wanted_forward(index, critic_lstm, groups, per_group, 0, True)
    wrong = regrouped_state(state, groups, per_group)
    assert bits(wrong) != bits(state)
    after = np.zeros_like(state)
    with np.errstate(all="ignore"):
        got = fresh_twin(spec, twin).act(obs, starts, final_obs, True, states=(wrong, after))
    assert bits(after) != bits(want[4]), "the regrouped state gives the same next state"
    if spec.n_actions > 2:  # (the least network has two actions whose logits tie: log 1/2 from any state)
        assert bits(got[2]) != bits(want[2]), "the regrouped state gives the same log-probabilities"
    if critic_lstm:
        assert bits(got[1]) != bits(want[1]), "the regrouped state gives the same values"


class _Learner:
    """The raw arrays of rf_lstm_ppo_update_grouped on the device, parameters, states and stats between guard floats."""

    def __init__(self, torch, ctx, spec, twin, parts, hypers, batch):
        """hypers: learner.Hyper per group, or the packed records."""
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
        size = ctx.lstm_ppo_grouped_workspace_size(spec.critic_desc(), self.groups, self.per_group, self.steps, batch)
        assert size > 0 and size % 8 == 0
        self.whole_workspace = torch.full((size // 4 + 4,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.workspace = self.whole_workspace[2:-2]
        self.batch = batch

    def update(self, firsts, changed=(), stream=None):
        self.enqueue(self.torch.from_numpy(np.array(firsts, dtype=np.int32)).cuda(), changed, stream)
        self.torch.cuda.synchronize()
        return self.outputs()

    def enqueue(self, table, changed=(), stream=None):
        torch = self.torch
        a = dict(desc=self.spec.critic_desc(), groups=self.groups, per_group=self.per_group, steps=self.steps,
                 hyper=self.hyper.data_ptr(), params=self.params.data_ptr(), state=self.state.data_ptr(),
                 workspace=self.workspace.data_ptr(), obs=self.parts["observations"].data_ptr(),
                 actions=self.parts["actions"].data_ptr(), log_probs=self.parts["log_probs"].data_ptr(),
                 advantages=self.parts["advantages"].data_ptr(), returns=self.parts["returns"].data_ptr(),
                 starts=self.parts["episode_starts"].data_ptr(), states=self.parts["lstm_states"].data_ptr(),
                 firsts=table.data_ptr(), batch=self.batch, stats=self.stats.data_ptr())
        a.update(changed)
        self.ctx.lstm_ppo_update_grouped(a["desc"], a["groups"], a["per_group"], a["steps"], a["hyper"], a["params"],
                                         a["state"], a["workspace"], a["obs"], a["actions"], a["log_probs"], a["advantages"],
                                         a["returns"], a["starts"], a["states"], a["firsts"], a["batch"], a["stats"],
                                         torch.cuda.current_stream().cuda_stream if stream is None else stream)

    def outputs(self):
        return self.params.cpu().numpy(), self.state.cpu().numpy(), self.stats.cpu().numpy()

    def guards_kept(self):
        return all(_untouched(w[:2]) and _untouched(w[-2:]) for w in (self.whole_state, self.whole_workspace)) \
            and _guards_kept(self.whole_params) and _guards_kept(self.whole_stats)


def _same_update(got, want, what):
    for name, x, y in zip(("parameters", "optimizer states", "stats"), got, want):
        assert bits(np.asarray(x)) == bits(np.asarray(y)), f"{what}: the {name} differ"


def _learner_of(torch, ctx, index, critic_lstm, groups, steps, per_group, batch, kind="mixed", parts=None):
    from reinfocus_amd.environments import harness

    spec, twin, cached = update_inputs(index, critic_lstm, groups, steps, per_group, kind)
    hypers = harness.PopulationLearner(fresh_twin(spec, twin), **hypers_of(groups)).hypers()
    return spec, twin, hypers, _Learner(torch, ctx, spec, twin, cached if parts is None else parts, hypers, batch)


def update_case(torch, ctx, index, critic_lstm, batch):
    """rf_lstm_ppo_update_grouped against the twin population over two consecutive updates: parameters, optimizer states
    and stats as bytes between guards; then G stand-alone rf_lstm_ppo_update / rf_lstm_critic_ppo_update launches on
    contiguous slice copies give the same bytes."""
    u = UPDATE
    rows = u["steps"] * u["per_group"]
    spec, twin, hypers, device = _learner_of(torch, ctx, index, critic_lstm, u["groups"], u["steps"], u["per_group"], batch)
    want = twin_updates(index, critic_lstm, u["groups"], u["steps"], u["per_group"], u["firsts"], batch, u["updates"])
    for update in range(u["updates"]):
        _same_update(device.update(firsts_of(u["firsts"], update, rows)), want[update], f"update {update}")
    assert device.guards_kept(), "a guard was written"
    assert all((stats[:, 7] == 0).all() for _, _, stats in want)
    assert bits(want[1][0][1]) == bits(twin.params[1]) and bits(want[1][0][0]) != bits(twin.params[0])  # (lr 0: group 1)
    _, _, parts = update_inputs(index, critic_lstm, u["groups"], u["steps"], u["per_group"])
    _alone_updates(torch, ctx, spec, twin, hypers, parts, u["firsts"], batch, want)


def _alone_updates(torch, ctx, spec, twin, hypers, parts, firsts, batch, want):
    """The same device, G stand-alone learners over contiguous copies of the groups' slices: len(want) consecutive
    rf_lstm_ppo_update (rf_lstm_critic_ppo_update) launches each give the bytes of want[update][.][g]."""
    from reinfocus_amd.environments import learner

    critic_lstm, groups = spec.enable_critic_lstm, twin.groups
    steps, per_group = parts["n_steps"], parts["num_envs"] // groups
    update_alone = ctx.lstm_ppo_update if critic_lstm else ctx.lstm_critic_ppo_update
    size_alone = (ctx.lstm_ppo_workspace_size(spec.desc(), batch) if critic_lstm
                  else ctx.lstm_critic_workspace_size(spec.critic_desc(), batch))
    desc = spec.desc() if critic_lstm else spec.critic_desc()
    stream = torch.cuda.current_stream().cuda_stream
    for g in range(groups):
        piece = {key: torch.from_numpy(value).cuda() for key, value in group_slices(parts, groups, g).items()
                 if isinstance(value, np.ndarray)}
        params = torch.from_numpy(twin.params[g].copy()).cuda()
        state = torch.from_numpy(learner.fresh_state(spec)).cuda()
        workspace = torch.zeros(size_alone // 4, dtype=torch.float32, device="cuda")
        stats = torch.zeros(8, dtype=torch.float32, device="cuda")
        for update in range(len(want)):
            update_alone(desc, hypers[g], params.data_ptr(), state.data_ptr(), workspace.data_ptr(), steps, per_group,
                         piece["observations"].data_ptr(), piece["actions"].data_ptr(), piece["log_probs"].data_ptr(),
                         piece["advantages"].data_ptr(), piece["returns"].data_ptr(), piece["episode_starts"].data_ptr(),
                         piece["lstm_states"].data_ptr(), firsts_of(firsts, update, steps * per_group)[g], batch,
                         stats.data_ptr(), stream)
            torch.cuda.synchronize()
            _same_update((params.cpu().numpy(), state.cpu().numpy(), stats.cpu().numpy()),
                         tuple(x[g] for x in want[update]), f"stand-alone group {g}, update {update}")


def layout_case(torch, ctx, name, critic_lstm):
    """rf_lstm_ppo_update_grouped on a case of LAYOUT_CASES against the twin population over the case's consecutive
    updates, group by group: parameters, optimizer states and stats as bytes between guard floats, the workspace of exactly
    rf_lstm_ppo_grouped_workspace_size(B)'s bytes between guards; where the case says so, also G stand-alone launches on
    contiguous slice copies."""
    shape, kind, firsts, batch = layout_shape(name, critic_lstm)
    groups, steps, per_group = shape[2:]
    spec, twin, hypers, device = _learner_of(torch, ctx, *shape, batch, kind=kind)
    want = layout_twin_updates(name, critic_lstm)
    for update in range(len(want)):
        got = device.update(firsts_of(firsts, update, steps * per_group))
        for g in range(groups):
            _same_update(tuple(x[g] for x in got), tuple(x[g] for x in want[update]), f"update {update}, group {g}")
    assert device.guards_kept(), "a guard was written"
    layout_update_promises(name, critic_lstm)
    if LAYOUT_CASES[name]["alone"]:
        _alone_updates(torch, ctx, spec, twin, hypers, update_inputs(*shape, kind)[2], firsts, batch, want)


def _groups_that_differ(got, want, axis=0):
    """Indices along `axis` (the groups') at which two equally shaped arrays differ in a byte."""
    x = np.moveaxis(np.ascontiguousarray(got), axis, 0)
    y = np.moveaxis(np.ascontiguousarray(want), axis, 0)
    x, y = (np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1) for a in (x, y))
    return np.flatnonzero((x != y).any(axis=1))


def group_limit_case(torch, ctx, critic_lstm):
    """RF_POPULATION_MAX_GROUPS groups of one environment on the least network (limit_arrays): rf_lstm_forward_grouped
    sampled (every generator CONSUMED[1] draws on) and deterministic with the state in place, then one
    rf_lstm_ppo_update_grouped at m = T = B = 1 of fresh optimizers: every output byte of every group against its
    combination's result.  The groups whose firsts[g] = 1 = N carry RF_PPO_INVALID and keep parameters and optimizer state;
    all others, their neighbours included, equal the twin."""
    from reinfocus_amd.environments import learner, policy

    spec, groups = limit_spec(critic_lstm), LIMIT_GROUPS
    inputs, wanted_forward, wanted_update = limit_arrays(critic_lstm)
    params, obs, final_obs, starts = (torch.from_numpy(inputs[key]).cuda() for key in ("params", "observations", "final", "starts"))
    table = torch.from_numpy(inputs["gens"].view(np.int64)).cuda()
    for deterministic in (False, True):
        whole, out = _guarded(torch, groups)
        whole_state, state = _guarded_floats(torch, inputs["state"])
        _forward(torch, ctx, spec, groups, 1, params, obs, starts, final_obs, state, state, table, CONSUMED[1],
                 policy.DETERMINISTIC if deterministic else 0, out)
        torch.cuda.synchronize()
        for name, wanted in zip(ORDER, wanted_forward[deterministic]):
            differ = _groups_that_differ(out[name].cpu().numpy(), wanted)
            assert differ.size == 0, f"deterministic {deterministic}: {name} differ in {differ.size} groups, first {differ[:4]}"
            assert _untouched(whole[name][0]) and _untouched(whole[name][groups + 1]), f"a guard row of {name} was written"
        differ = _groups_that_differ(state.cpu().numpy(), wanted_forward[deterministic][4], axis=2)
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


class _Packed:
    """What _Learner reads of a twin population, around packed parameters [G][P]."""

    def __init__(self, params):
        self.params, self.groups = params, params.shape[0]


def limit_case(torch, ctx):
    """H = 256 (sb3-contrib's default network), G = 2, m = 2, T = 3, B = 6 = m T, both critic kinds."""
    c = LIMIT
    for critic_lstm in CRITICS:
        _, _, _, device = _learner_of(torch, ctx, c["index"], critic_lstm, c["groups"], c["steps"], c["per_group"], c["batch"],
                                      kind="some")
        want = twin_updates(c["index"], critic_lstm, c["groups"], c["steps"], c["per_group"], c["firsts"], c["batch"], 1,
                            "some")
        _same_update(device.update(c["firsts"]), want[0], f"enable_critic_lstm={critic_lstm}")
        assert device.guards_kept() and (want[0][2][:, 7] == 0).all()


def isolation_case(torch, ctx, critic_lstm):
    """A NaN advantage in group 1's minibatch: group 1 is flagged RF_PPO_NONFINITE and keeps parameters and optimizer state
    byte for byte, groups 0 and 2 equal a run without the NaN.  The same with firsts[1] = N: RF_PPO_INVALID."""
    u = UPDATE
    index, batch, rows = lstm_cases.TUNED, 5, u["steps"] * u["per_group"]
    shape = (index, critic_lstm, u["groups"], u["steps"], u["per_group"])
    spec, twin, parts = update_inputs(*shape)
    clean = twin_updates(*shape, u["firsts"], batch, 1)[0]
    before = _learner_of(torch, ctx, *shape, batch)[3].outputs()
    poisoned = dict(parts)
    poisoned["advantages"] = parts["advantages"].copy()
    poisoned["advantages"][rows + (u["firsts"][1] + 2) % rows] = np.nan  # (a row of group 1's minibatch)
    device = _learner_of(torch, ctx, *shape, batch, parts=poisoned)[3]
    for what, got, flag in (("a NaN advantage", device.update(u["firsts"]), NONFINITE),
                            ("firsts[1] = N", _learner_of(torch, ctx, *shape, batch)[3].update((0, rows, 11)), INVALID)):
        for g in (0, 2):
            _same_update(tuple(x[g] for x in got), tuple(x[g] for x in clean), f"{what}: group {g}")
        assert got[2][1][7] == flag, f"{what}: group 1 has flags {got[2][1][7]}"
        assert bits(got[0][1]) == bits(before[0][1]) and bits(got[1][1]) == bits(before[1][1]), f"{what}: group 1 moved"
    assert device.guards_kept()


def wide_forward_case(torch, ctx, groups, per_group):
    forward_case(torch, ctx, lstm_cases.TUNED, True, groups, per_group, alone=False)


def wide_update_case(torch, ctx):
    """One update at G = 64 on ppo_lstm_tuned.yml's shape (m = 8, T = 8, B = 8, H = 16), no flagged start, every group its
    own first row, against the twin."""
    c = WIDE_UPDATE
    shape = (c["index"], True, c["groups"], c["steps"], c["per_group"])
    device = _learner_of(torch, ctx, *shape, c["batch"], kind="none")[3]
    want = twin_updates(*shape, wide_firsts(), c["batch"], 1, "none")
    _same_update(device.update(wide_firsts()), want[0], "G = 64")
    assert device.guards_kept()


def kernel_refusal_case(torch, ctx):
    """Each refusal of the two entry points leaves every output as it was; a capturing stream is refused."""
    index, critic_lstm, groups, per_group = lstm_cases.TUNED, True, 3, 3
    spec, twin = twin_policy(index, critic_lstm, groups)
    n = groups * per_group
    obs_h, final_h, starts_h, state_h = forward_inputs(index, groups, per_group)
    params, obs, final_obs, starts = (torch.from_numpy(a).cuda() for a in (twin.params, obs_h, final_h, starts_h))
    table = _table(torch, groups)
    whole, out = _guarded(torch, n)
    whole_in, state_in = _guarded_floats(torch, state_h)
    whole_out, state_out = _guarded_floats(torch, np.zeros_like(state_h))
    state_out.view(torch.int32).fill_(SENTINEL)

    def attempt(changed, stream=None):
        try:
            _forward(torch, ctx, spec, groups, per_group, params, obs, starts, final_obs, state_in, state_out, table, 0, 0,
                     out, changed, stream)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            return str(caught)
        return None

    def unwritten(match):
        torch.cuda.synchronize()
        assert all(_untouched(w) for w in whole.values()) and _untouched(whole_out), f"an output was written ({match})"

    def refused(match, **changed):
        message = attempt(changed)
        assert message is not None and match in message, f"not refused ({match}): {message}"
        unwritten(match)

    host = np.zeros((n + 2, max(spec.obs_width, 4 * spec.lstm_hidden)), dtype=F32)
    refused("d_obs is not device memory", obs=host.ctypes.data)
    refused("d_episode_starts is not device memory", starts=host.ctypes.data)
    refused("d_state_in is not device memory", state_in=host.ctypes.data)
    refused("d_values is not device memory", values=host.ctypes.data)
    refused("d_gens is not device memory", gens=np.zeros((groups, 4), dtype=np.uint64).ctypes.data)
    refused("needs d_gens", gens=None)
    refused("NULL argument", starts=None)
    refused("NULL argument", state_in=None)
    refused("must be in 1", groups=0)
    refused("must be in 1", per_group=0)
    refused("must be in 1", groups=65536)
    refused("not aligned", gens=table.data_ptr() + 4)
    refused("d_values overlaps d_log_probs", values=out["log_probs"].data_ptr())
    refused("d_values overlaps d_obs", values=obs.data_ptr())
    refused("d_actions overlaps d_gens", actions=table.data_ptr())
    refused("d_state_out overlaps d_state_in", state_out=state_in.data_ptr() + 4 * spec.lstm_hidden)
    refused("d_state_out overlaps d_params", state_out=params.data_ptr())
    refused("outside the limits", desc=(0,) + tuple(spec.critic_desc()[1:]))
    refused("outside the limits", desc=tuple(spec.critic_desc()[:-1]) + (2,))
    refused("unknown flags", flags=2)
    message = _capturing(torch, lambda stream: attempt({}, stream))
    assert message is not None and "being captured" in message, message
    unwritten("a capturing stream")
    _forward(torch, ctx, spec, groups, per_group, params, obs, starts, final_obs, state_in, state_out, table, 0, 0, out)
    torch.cuda.synchronize()
    want, _ = wanted_forward(index, critic_lstm, groups, per_group, 0, False)
    for name, wanted in zip(ORDER, want):
        assert bits(out[name].cpu().numpy()) == bits(wanted), name
    assert bits(state_out.cpu().numpy()) == bits(want[4]) and _guards_kept(whole_out) and _guards_kept(whole_in)

    u = UPDATE
    rows, batch = u["steps"] * u["per_group"], 5
    _, _, _, device = _learner_of(torch, ctx, index, critic_lstm, u["groups"], u["steps"], u["per_group"], batch)
    kept = device.outputs()

    table = torch.tensor(list(u["firsts"]), dtype=torch.int32, device="cuda")

    def attempt_update(changed, stream=None):
        try:
            device.enqueue(table, changed, stream)
        except AssertionError as caught:
            return str(caught)
        return None

    def refused_update(match, **changed):
        message = attempt_update(changed)
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
    refused_update("not aligned", state=device.state.data_ptr() + 4)
    refused_update("d_stats overlaps d_params", stats=device.params.data_ptr())
    refused_update("d_workspace overlaps d_state", workspace=device.state.data_ptr())
    refused_update("d_stats overlaps d_lstm_states", stats=device.parts["lstm_states"].data_ptr())
    refused_update("d_params overlaps d_firsts", firsts=device.params.data_ptr())
    message = _capturing(torch, lambda stream: attempt_update({}, stream))
    assert message is not None and "being captured" in message, message
    assert all(bits(x) == bits(y) for x, y in zip(device.outputs(), kept)), "a refused update wrote an output"
    want = twin_updates(index, critic_lstm, u["groups"], u["steps"], u["per_group"], u["firsts"], batch, u["updates"])
    _same_update(device.update(u["firsts"]), want[0], "after the refusals")
    assert device.guards_kept()


def _capturing(torch, call):
    """A stream of its own in (relaxed) capture, by the runtime's own calls: `call(stream)` runs while it captures; the
    capture ends with an empty graph that is never instantiated or replayed."""
    from reinfocus_amd import torch_interop

    hip = ctypes.CDLL(torch_interop.hip_runtimes()[0])
    stream, graph = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    assert hip.hipStreamBeginCapture(stream, 2) == 0  # hipStreamCaptureModeRelaxed
    try:
        got = call(stream.value)
    finally:
        ended = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
        if graph.value:
            hip.hipGraphDestroy(graph)
        hip.hipStreamDestroy(stream)
    assert ended == 0
    return got


def _cuda_states(torch, states):
    return {key: torch.from_numpy(np.ascontiguousarray(value)).cuda() for key, value in states.items()}


def one_group_case(torch, critic_lstm):
    """G = 1: outputs, state, parameters and optimizer state after 3 chained updates and rng_state() equal the ungrouped
    DeviceLstmPolicy / DeviceLstmLearner bit for bit."""
    from reinfocus_amd.environments import harness

    n, steps = 11, 4
    env = harness.DeviceVectorDiscreteSteps(num_envs=n, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        spec = e2e_spec(critic_lstm)
        state = _cuda_states(torch, lstm_cases.state_dict(spec, 3))
        single = harness.DeviceLstmPolicy(env, spec, 77)
        grouped = harness.DevicePopulationLstmPolicy(env, spec, 1, [77])
        single.load_state_dict(state)
        grouped.load_state_dict(state)
        assert torch.equal(grouped.params[0], single.params)
        rng = np.random.default_rng(2)
        obs = torch.from_numpy(rng.standard_normal((n, 4)).astype(F32)).cuda()
        starts = torch.from_numpy(rng.choice(np.array([0, 0, 1, 255], dtype=np.uint8), n)).cuda()
        for deterministic in (False, True, False):
            ours = [t.clone() for t in grouped.act(obs, starts, None, deterministic)[:3]]
            theirs = single.act(obs, starts, None, deterministic)[:3]
            for x, y in zip(ours, theirs):
                assert bits(x.cpu().numpy()) == bits(y.cpu().numpy())
            assert grouped.rng_state() == [single.rng_state()]
            assert bits(grouped.lstm_state().cpu().numpy()) == bits(single.lstm_state().cpu().numpy())
            starts = torch.zeros_like(starts)
        assert bits(grouped.values(obs, starts).cpu().numpy()) == bits(single.values(obs, starts).cpu().numpy())
        assert grouped.lstm_state().abs().sum().item() > 0
        total = n * steps
        parts = {"observations": rng.standard_normal((total, 4)).astype(F32), "actions": rng.integers(0, 13, total),
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
    for i, (x, y) in enumerate(zip(got, want)):
        for key in ("episode_starts", "lstm_states", "stats", "params"):
            assert bits(x[key]) == bits(y[key]), f"iteration {i}: {key} differ"


def end_to_end_case(torch, critic_lstm):
    from reinfocus_amd.environments import harness

    want, want_rng, want_states, want_lstm = e2e_twin_runs(critic_lstm)
    groups = E2E["groups"]
    env = e2e_env(True)
    try:
        spec = e2e_spec(critic_lstm)
        policy = harness.DevicePopulationLstmPolicy(env, spec, groups, seeds_of(groups))
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
        per_epoch = -(-E2E["steps"] * E2E["per_group"] // E2E["batch"])
        assert want[0]["stats"].shape == (E2E["epochs"] * per_epoch, groups, 8) and (want[1]["stats"][:, :, 7] == 0).all()
        assert bits(want[0]["params"][0]) != bits(want[1]["params"][0])
        assert bits(want[1]["params"][2]) == bits(want[0]["params"][2])  # (learning_rate 0)
        assert np.concatenate([run["truncated"] for run in want]).any(), "no environment ended"
        assert any(run["lstm_states"][1:].any() for run in want)
        # resume: a second policy and learner from both state_dict()s go on bit for bit
        kept, kept_params = learner.state_dict(), [policy.state_dict(group=g) for g in range(groups)]
        splits = e2e_splits(9)
        straight = learner.train(rollout, E2E["epochs"], E2E["batch"], splits).clone()
        after = policy.params.clone()
        second_policy = harness.DevicePopulationLstmPolicy(env, spec, groups, seeds_of(groups))
        for g in range(groups):
            second_policy.load_state_dict(kept_params[g], group=g)
        second_policy.set_rng_state(policy.rng_state())
        second_policy.set_lstm_state(policy.lstm_state())
        second = harness.DevicePopulationLearner(second_policy, **e2e_hypers())
        second.load_state_dict(kept)
        again = second.train(rollout, E2E["epochs"], E2E["batch"], splits=splits)
        assert torch.equal(again.view(torch.int32), straight.view(torch.int32))
        assert torch.equal(second_policy.params.view(torch.int32), after.view(torch.int32))
        assert torch.equal(second.state.view(torch.int32), learner.state.view(torch.int32))
        drawn = second.train(rollout, 1, E2E["batch"], generator=np.random.default_rng(1))
        assert tuple(drawn.shape) == (per_epoch, groups, 8) and (drawn[:, :, 7] == 0).all()
    finally:
        env.close()


def surface_case(torch):
    """What the classes refuse, each with a message, the tensors unchanged afterwards and no draw consumed."""
    from reinfocus_amd.environments import harness

    env = e2e_env(True)
    jumps = harness.DeviceVectorContinuousJumps(num_envs=9, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        spec = e2e_spec()

        def raises(kind, match, call):
            try:
                call()
            except kind as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"not refused ({match})")

        make = harness.DevicePopulationLstmPolicy
        raises(ValueError, "not divisible", lambda: make(env, spec, 4, [1, 2, 3, 4]))
        raises(ValueError, "one seed per group", lambda: make(env, spec, 3, [1, 2]))
        raises(ValueError, "one seed per group", lambda: make(env, spec, 3, 7))
        raises(ValueError, "next step", lambda: make(jumps, spec, 3, [1, 2, 3]))
        sde_spec = harness.LstmSdePolicySpec(4, lstm_hidden=9, pi=(6,), vf=(5,))
        raises(ValueError, "next step", lambda: make(jumps, sde_spec, 3, [1, 2, 3]))
        raises(ValueError, "LstmPolicySpec", lambda: make(env, population_cases.e2e_spec(), 3, [1, 2, 3]))
        policy = make(env, spec, 3, [1, 2, 3])
        assert policy.spec.kind == "lstm" and policy.groups == 3 and tuple(policy.params.shape) == (3, spec.size)
        raises(TypeError, "DeviceLstmPolicy", lambda: harness.DeviceLstmLearner(policy))
        before = policy.rng_state()
        obs = torch.zeros((9, 4), dtype=torch.float32, device="cuda")
        starts = torch.zeros(9, dtype=torch.uint8, device="cuda")
        raises(ValueError, "rows", lambda: policy.act(obs[:8].contiguous(), starts[:8].contiguous()))
        raises(ValueError, "episode_starts is", lambda: policy.act(obs, starts[:8].contiguous()))
        raises(ValueError, "states[1] is", lambda: policy.act(obs, starts, states=(policy.lstm_state(), obs)))
        raises(ValueError, "generator states", lambda: policy.set_rng_state(before[:2]))
        raises(IndexError, "group 3", lambda: policy.state_dict(group=3))
        assert policy.rng_state() == before
        learner = harness.DevicePopulationLearner(policy)
        rollout = harness.DeviceRollout(env, 2)
        rollout.start(env.reset_tensors()[0])
        rollout.collect(policy)
        kept = policy.params.clone()
        raises(ValueError, "more than the 6 rows", lambda: learner.train(rollout, 1, 7))
        raises(ValueError, "splits must be", lambda: learner.train(rollout, 2, 4, [[0, 1, 2]]))
        raises(ValueError, "splits must be", lambda: learner.train(rollout, 1, 4, [[0, 1, 6]]))
        raises(ValueError, "firsts must be", lambda: learner.update(rollout, [0, 1], 4))
        raises(ValueError, "firsts must be", lambda: learner.update(rollout, [0, 1, 6], 4))
        raises(ValueError, "a minibatch of 7", lambda: learner.update(rollout, [0, 1, 2], 7))
        raises(TypeError, "firsts, count", lambda: learner.update(rollout, [0, 1, 2]))
        other = harness.DeviceRollout(env, 2, groups=9)
        raises(ValueError, "groups=9", lambda: other.start(env.reset_tensors()[0]) or other.collect(policy))
        plain = harness.DevicePopulationPolicy(env, population_cases.e2e_spec(), 3, [1, 2, 3])
        flat_rollout = harness.DeviceRollout(env, 2)
        flat_rollout.start(env.reset_tensors()[0])
        flat_rollout.collect(plain)
        raises(ValueError, "no lstm_states", lambda: learner.train(flat_rollout, 1, 4))
        host_env = e2e_env(False)
        try:
            twin = harness.LstmPopulationPolicy(spec, 3, [1, 2, 3])
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
        jumps.close()


def sharded_case(torch):
    from reinfocus_amd.environments import harness

    env = harness.ShardedVectorDiscreteSteps(num_envs=9, devices=[0], frame_height=16, samples_per_pixel=1, seed=1)
    try:
        try:
            harness.DevicePopulationLstmPolicy(env, e2e_spec(), 3, [1, 2, 3])
        except ValueError as caught:
            assert "tensors" in str(caught), str(caught)
        else:
            raise AssertionError("a sharded environment was not refused")
    finally:
        env.close()


def critic_name(critic_lstm):
    return "lstm" if critic_lstm else "linear"


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
    for groups, per_group in WIDE_FORWARD:
        with record.case(f"forward/wide/{groups}/{per_group}"):
            wide_forward_case(torch, ctx, groups, per_group)
    with record.case("update/wide"):
        wide_update_case(torch, ctx)
    with record.case("limit"):
        limit_case(torch, ctx)
    for name, case in LAYOUT_CASES.items():
        for critic_lstm in case["critics"]:
            with record.case(f"layout/{name}/{critic_name(critic_lstm)}"):
                layout_case(torch, ctx, name, critic_lstm)
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
