"""CPU tests of the population of recurrent PPO learners (include/reinfocus_hip.h, "population lstm"): the numpy twins
harness.LstmPopulationPolicy / PopulationLearner over it are literally G of the existing twins (lstm.LstmPolicy,
lstm_learner.LstmLearner) over copied slices, the size rules and the grouped addressing helpers of the kernels' headers
(tests/lstmpopcheck, a host build) are G times the ungrouped sizes and the restated sequence rule per group, header,
binding and library agree on the four entry points, and the surface refuses what it cannot express.  The arithmetic of one
group is held to the host build of the kernels' functions by tests/test_lstm_logic.py and tests/test_lstm_learner_logic.py;
nothing here needs a GPU.  The layout cases (sequences of 1 to 17 and of more than 64 rows, 1024 and 513 rows, H = 256) and
the 65535 groups of the limit hold what their docstrings promise.  tests/test_gpu_population_lstm.py holds the device
classes and the grouped entry points to these twins as bytes."""

import ctypes
import os
import re

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, lstm_learner, population
from tests import helpers
from tests import lstm_io_cases as lstm_cases
from tests import lstm_learner_io_cases as lstm_learner_cases
from tests import population_io_cases as population_cases
from tests import population_lstm_io_cases as cases
from tests import rollout_io_cases as rollout_cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits
ENTRY_POINTS = ["rf_lstm_forward_grouped", "rf_lstm_ppo_grouped_state_size", "rf_lstm_ppo_grouped_workspace_size",
                "rf_lstm_ppo_update_grouped"]


def _members(spec, twin):
    """G stand-alone LstmPolicy twins with the population's seeds and parameters."""
    members = []
    for g, seed in enumerate(cases.seeds_of(twin.groups)):
        member = harness.LstmPolicy(spec, seed)
        member.params = twin.params[g].copy()
        members.append(member)
    return members


# ---- 1: the twins are G stand-alone twins over copied slices ------------------------------------------------------------
@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
@pytest.mark.parametrize("per_group", cases.PER_GROUP)
@pytest.mark.parametrize("groups", cases.GROUPS)
@pytest.mark.parametrize("index", cases.NETS)
def test_population_policy_is_g_policies_over_slices(index, groups, per_group, critic_lstm):
    """Two chained act() calls in place (sampled, then deterministic), one from `in` to `out`, and values(): every output
    and the whole state equal G LstmPolicy over contiguous copies of the lanes' slices, generator states included."""
    spec, twin = cases.twin_policy(index, critic_lstm, groups)
    members = _members(spec, twin)
    obs, final_obs, starts, state = cases.forward_inputs(index, groups, per_group)
    lanes = [slice(g * per_group, (g + 1) * per_group) for g in range(groups)]
    twin.set_lstm_state(state)
    for member, rows in zip(members, lanes):
        member.set_lstm_state(np.ascontiguousarray(state[:, :, rows, :]))
    with np.errstate(all="ignore"):
        for deterministic, flags in ((False, starts), (True, np.zeros_like(starts))):
            got = twin.act(obs, flags, final_obs, deterministic)
            for g, (member, rows) in enumerate(zip(members, lanes)):
                want = member.act(obs[rows].copy(), flags[rows].copy(), final_obs[rows].copy(), deterministic)
                for i in range(4):
                    assert bits(got[i][rows]) == bits(want[i]), (deterministic, g, i)
                assert bits(twin.lstm_state()[:, :, rows, :]) == bits(member.lstm_state()), (deterministic, g)
        kept = twin.lstm_state()
        after = np.zeros_like(state)
        got = twin.act(obs, starts, None, True, states=(state, after))
        assert got[3] is None and bits(twin.lstm_state()) == bits(kept)
        values, finals = twin.values(obs, starts, final_obs)
        for g, (member, rows) in enumerate(zip(members, lanes)):
            piece = np.zeros_like(member.lstm_state())
            member.act(obs[rows], starts[rows], None, True, states=(np.ascontiguousarray(state[:, :, rows, :]), piece))
            assert bits(after[:, :, rows, :]) == bits(piece), g
            want = member.values(obs[rows], starts[rows], final_obs[rows])
            assert bits(values[rows]) == bits(want[0]) and bits(finals[rows]) == bits(want[1]), g
    assert bits(twin.lstm_state()) == bits(kept), "values() advanced the state"
    assert twin.rng_state() == [member.rng_state() for member in members]
    assert np.isnan(finals).any() and not np.isnan(finals).all()  # (NaN-led final_obs rows among live ones)
    if groups > 1:  # the state-plane stride: the same bytes read as [G][2][2][m][H] give another state
        assert bits(cases.regrouped_state(state, groups, per_group)) != bits(state)


@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
@pytest.mark.parametrize("batch", cases.UPDATE["batches"])
@pytest.mark.parametrize("index", cases.NETS)
def test_population_learner_is_g_learners_over_slices(index, batch, critic_lstm):
    """Two consecutive updates of three groups with firsts (0, 7, 11) -- one group does not wrap, two wrap at different
    rows -- and starts that differ per group: parameters, optimizer states and stats equal G LstmLearner over contiguous
    copies of the slice-parts, each with its own hyper-parameters."""
    u = cases.UPDATE
    shape = (index, critic_lstm, u["groups"], u["steps"], u["per_group"])
    spec, twin, parts = cases.update_inputs(*shape)
    want = cases.twin_updates(*shape, u["firsts"], batch, u["updates"])
    hypers = harness.PopulationLearner(cases.fresh_twin(spec, twin), **cases.hypers_of(u["groups"])).hypers()
    rows = u["steps"] * u["per_group"]
    structures = set()
    for g, member in enumerate(_members(spec, twin)):
        alone = harness.LstmLearner(member, hypers[g].learning_rate, hypers[g].clip_range, hypers[g].ent_coef,
                                    hypers[g].vf_coef, hypers[g].max_grad_norm, bool(hypers[g].normalize_advantage),
                                    (hypers[g].beta1, hypers[g].beta2), hypers[g].adam_eps)
        piece = cases.group_slices(parts, u["groups"], g)
        structures.add(piece["episode_starts"].tobytes())
        with np.errstate(all="ignore"):
            for update in range(u["updates"]):
                stats = alone.update(piece, cases.firsts_of(u["firsts"], update, rows)[g], batch)
                assert bits(stats) == bits(want[update][2][g]), (g, update)
                assert bits(member.params) == bits(want[update][0][g]) and bits(alone.state) == bits(want[update][1][g])
    assert len(structures) == u["groups"], "the groups' sequence structures do not differ"
    assert bits(population.group_parts(parts, u["groups"], 1)["lstm_states"]) == \
        bits(cases.group_slices(parts, u["groups"], 1)["lstm_states"])


def _alone(member, h):
    return harness.LstmLearner(member, h.learning_rate, h.clip_range, h.ent_coef, h.vf_coef, h.max_grad_norm,
                               bool(h.normalize_advantage), (h.beta1, h.beta2), h.adam_eps)


def _sequences(lib, starts, groups, per_group, g, steps, first, batch):
    """Group g's minibatch by the kernels' own helpers, held to the restated rule over the group's own columns: (the
    lengths of its sequences in order, the lane read for every row)."""
    own = np.ascontiguousarray(starts[:, g * per_group:(g + 1) * per_group])
    want = lstm_learner_cases.restated_rows(own, steps, per_group, first, batch)
    rows, start, end, lane = (np.zeros(batch, dtype=np.int32) for _ in range(4))
    assert lib.lpop_sequences(starts.ctypes.data, groups, per_group, g, steps, first, batch, rows.ctypes.data,
                              start.ctypes.data, end.ctypes.data, lane.ctypes.data) == groups * per_group
    assert [int(r) for r in rows] == [row for row, _, _ in want]
    assert [bool(f) for f in start] == [is_start for _, is_start, _ in want]
    assert [int(x) for x in lane] == [g * per_group + row // steps for row, _, _ in want]  # (the lane read: g m + e)
    begins = [b for b in range(batch) if want[b][1]]
    lengths = [nxt - b for b, nxt in zip(begins, begins[1:] + [batch])]
    assert [int(end[b]) - b for b in begins] == lengths
    return lengths, rows


@pytest.mark.parametrize("name", cases.LAYOUT_CASES)
def test_layout_cases_hold_what_they_promise(name):
    """cases.LAYOUT_CASES through the kernels' own addressing helpers (tests/lstmpopcheck) and the restated sequence rule,
    per group and update: the depth cases hold sequences of exactly 1, 8, 9, 16 and 17 rows in every group's first
    minibatch (at B = 68 = N group 0's first row 5 cuts its 17-row environment into 12 + 5, so it holds the other four;
    groups 0 and 2 wrap, at different rows); every group of the untuned cases holds one sequence of more than 64 rows and
    one of one row, group 1 crosses an environment boundary and group 2 wraps; the wave cases hold 1024 one-row
    sequences, and 33 or 34 as the first row decides; the lane read for every row is g m + e; the groups' structures
    differ; the workspace size is G times the ungrouped one."""
    lib = cases.hostcheck()
    case = cases.LAYOUT_CASES[name]
    for critic_lstm in case["critics"]:
        shape, kind, firsts, batch = cases.layout_shape(name, critic_lstm)
        index, _, groups, steps, per_group = shape
        spec, twin, parts = cases.update_inputs(*shape, kind)
        starts = parts["episode_starts"]
        total = steps * per_group
        assert starts.shape == (steps + 1, groups * per_group) and len(firsts) == groups and batch <= min(total, 1024)
        structures = {np.ascontiguousarray(starts[:, g * per_group:(g + 1) * per_group]).tobytes() for g in range(groups)}
        assert len(structures) == (groups if kind != "none" else 1)
        for update in range(case["updates"]):
            for g, first in enumerate(cases.firsts_of(firsts, update, total)):
                lengths, rows = _sequences(lib, starts, groups, per_group, g, steps, first, batch)
                wraps = first + batch > total
                if kind == "depth" and update == 0:
                    assert {1, 8, 9, 16} <= set(lengths), (g, lengths)
                    if batch == total and g == 0:
                        assert first == 5 and 17 not in lengths and lengths[0] == 12 and lengths[-1] == 5
                    else:
                        assert 17 in lengths, (g, lengths)
                    if batch == total:
                        assert wraps == (g != 1) and firsts[0] != firsts[2]
                elif kind == "drawn":
                    assert max(lengths) > 64 and min(lengths) == 1, (update, g, lengths)
                    assert wraps == (g == 2)
                    if update == 0:  # (g = 1: across an environment boundary)
                        assert len({int(r) // steps for r in rows}) == (1 if g == 0 else 2)
                elif kind == "every":
                    assert batch == total == 1024 and lengths == [1] * 1024
                elif kind == "none":
                    touched = (first + batch - 1) // steps - first // steps + 1
                    assert batch == 513 and total == 1024 and len(lengths) == touched and touched in (33, 34)
                    assert max(lengths) == steps
        desc = cases.critic_desc(spec)
        one = lib.lpop_workspace_size(ctypes.byref(desc), 1, per_group, steps, batch)
        assert lib.lpop_workspace_size(ctypes.byref(desc), groups, per_group, steps, batch) == groups * one > 0
        if critic_lstm:
            plain = lstm_learner_cases._lstm_desc(spec)
            assert lstm_learner_cases.hostcheck().lpc_workspace_size(ctypes.byref(plain), batch) == one
    assert case["index"] == (lstm_cases.DEFAULT if name.endswith("default") else lstm_cases.TUNED)


@pytest.mark.parametrize("name,critic_lstm", [(name, critic_lstm) for name, case in cases.LAYOUT_CASES.items()
                                              for critic_lstm in case["critics"]])
def test_layout_twin_population_is_g_learners_over_slices(name, critic_lstm):
    """The twin results the GPU file compares rf_lstm_ppo_update_grouped with on cases.LAYOUT_CASES equal G LstmLearner over
    contiguous copies of the groups' slice-parts, each with its own hyper-parameters and first row, byte for byte; and no
    comparison is vacuous (cases.layout_update_promises): flags 0 in every group and update, every group with a learning
    rate ends with other parameters, parameters differ per group and hyper-parameters between neighbours."""
    cases.layout_update_promises(name, critic_lstm)
    shape, kind, firsts, batch = cases.layout_shape(name, critic_lstm)
    groups, steps, per_group = shape[2:]
    spec, twin, parts = cases.update_inputs(*shape, kind)
    want = cases.layout_twin_updates(name, critic_lstm)
    hypers = harness.PopulationLearner(cases.fresh_twin(spec, twin), **cases.hypers_of(groups)).hypers()
    for g, member in enumerate(_members(spec, twin)):
        alone = _alone(member, hypers[g])
        piece = cases.group_slices(parts, groups, g)
        with np.errstate(all="ignore"):
            for update in range(len(want)):
                stats = alone.update(piece, cases.firsts_of(firsts, update, steps * per_group)[g], batch)
                assert bits(stats) == bits(want[update][2][g]), (g, update)
                assert bits(member.params) == bits(want[update][0][g]) and bits(alone.state) == bits(want[update][1][g])


@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
def test_the_combinations_of_the_group_limit_are_distinct(critic_lstm):
    """cases.limit_results / limit_arrays, what stands for the 65535 groups of m = T = B = 1: the 105 combinations give 105
    different updated parameters, optimizer states and stats, all taken and all moved; the 35 (parameter set, block)
    pairs give 35 different values, final values and next states; both actions are sampled; the three blocks that read
    their state would give another result on another block's level (so a wrong state stride shows); neighbouring groups
    differ in parameters, inputs, state, hyper-parameters and generator; the groups with g % 11 = 5 have firsts[g] = N,
    which the kernels' lstm_ppo_first flags, and their neighbours have 0; the size functions take 65535 groups and
    refuse 65536."""
    from reinfocus_amd.environments import lstm

    lib = cases.hostcheck()
    spec = cases.limit_spec(critic_lstm)
    params, blocks, hypers, generators = cases.limit_parts(critic_lstm)
    forwards, updates = cases.limit_results(critic_lstm)
    for part, name in enumerate(("params", "state", "stats")):
        assert len({bits(update[part]) for update in updates}) == 105, name
    assert all(update[2][7] == 0 for update in updates)
    assert all(bits(update[0]) != bits(params[c % 7]) for c, update in enumerate(updates))
    pairs = [forwards[True][k][j][0] for k in range(7) for j in range(5)]
    for part in (1, 3, 4):
        assert len({bits(pair[part]) for pair in pairs}) == 35, part
    sampled = [forwards[False][k][j][i] for k in range(7) for j in range(5) for i in range(cases.LIMIT_GENERATORS)]
    assert {int(one[0][0]) for one in sampled} == {0, 1}
    assert np.isfinite(np.concatenate([np.concatenate([one[1], one[2], one[3]]) for one in sampled])).all()
    for j, block in enumerate(blocks):  # (another block's level under the same inputs)
        other = blocks[(j + 1) % 5]["state"]
        got = lstm.lstm_numpy(spec, params[0], block["observations"], block["starts"], other, block["final"], None, True)
        assert (bits(got["state"]) != bits(forwards[True][0][j][0][4])) == (cases.LIMIT_STARTS[j] == 0), j
    assert sum(byte == 0 for byte in cases.LIMIT_STARTS) == 3
    inputs, wanted_forward, wanted_update = cases.limit_arrays(critic_lstm)
    assert inputs["params"].shape == (65535, spec.size) and inputs["state"].shape == (2, 2, 65535, 1)
    assert inputs["lstm_states"].shape == (2, 2, 2, 65535, 1) and inputs["episode_starts"].shape == (2, 65535)
    for key in ("params", "observations", "hyper", "gens"):
        rows = inputs[key].reshape(65535, -1)
        assert all(rows[g].tobytes() != rows[g + 1].tobytes() for g in range(0, 65534, 257)), key
    state = inputs["state"]
    assert all(bits(state[:, :, g]) != bits(state[:, :, g + 1]) for g in range(0, 65534, 257))
    for g in (0, 5, 247, 65534):
        k, j, i = g % 7, g % 5, g % cases.LIMIT_GENERATORS
        for deterministic in (False, True):
            for part in range(4):
                assert bits(wanted_forward[deterministic][part][g:g + 1]) == bits(forwards[deterministic][k][j][i][part])
            assert bits(wanted_forward[deterministic][4][:, :, g:g + 1]) == bits(forwards[deterministic][k][j][i][4])
        assert all(bits(wanted_update[part][g]) == bits(updates[g % 105][part]) for part in range(3))
        assert bits(state[:, :, g:g + 1]) == bits(blocks[j]["state"])
    outside = inputs["outside"]
    assert list(np.flatnonzero(outside)[:3]) == [5, 16, 27] and outside.sum() == 5958
    flag = ctypes.c_int(0)
    for g in (4, 5, 6, 16, 65533):
        assert lib.lpop_first(int(inputs["firsts"][g]), 1, ctypes.byref(flag)) == 0 and flag.value == int(outside[g])
    desc = cases.critic_desc(spec)
    one = lib.lpop_workspace_size(ctypes.byref(desc), 1, 1, 1, 1)
    assert lib.lpop_workspace_size(ctypes.byref(desc), 65535, 1, 1, 1) == 65535 * one > 0
    assert lib.lpop_workspace_size(ctypes.byref(desc), 65536, 1, 1, 1) == 0 == lib.lpop_state_size(ctypes.byref(desc), 65536, 1)


class _Finished:
    """What train() reads of a finished recurrent rollout."""

    def __init__(self, parts, groups=None):
        self._parts, self.groups = parts, groups
        self.episode_starts, self.lstm_states = parts["episode_starts"], parts["lstm_states"]
        self.n_steps, self.num_envs = parts["n_steps"], parts["num_envs"]
        self.env = type("env", (), {"single_action_space": harness.spaces.Discrete(64)})

    def flat(self):
        return {key: self._parts[key] for key in lstm_learner.BATCH_KEYS}


def test_train_rotates_every_group_by_its_own_split():
    """train() with splits [n_epochs][G]: the updates are update() calls with firsts (split + i * batch_size) mod m T and
    the short last minibatch; a drawn run takes generator.integers(m T, size=G) per epoch."""
    u = cases.UPDATE
    shape = (lstm_cases.TUNED, True, u["groups"], u["steps"], u["per_group"])
    spec, twin, parts = cases.update_inputs(*shape)
    rows, batch = u["steps"] * u["per_group"], 5
    splits = np.array([[0, 7, 11], [3, 3, 9]])
    trained = cases.fresh_twin(spec, twin)
    with np.errstate(all="ignore"):
        stats = harness.PopulationLearner(trained, **cases.hypers_of(3)).train(_Finished(parts), 2, batch, splits)
        stepped = cases.fresh_twin(spec, twin)
        by_hand = harness.PopulationLearner(stepped, **cases.hypers_of(3))
        want = [by_hand.update(parts, (splits[epoch] + i * batch) % rows, min(batch, rows - i * batch))
                for epoch in range(2) for i in range(3)]
        assert stats.shape == (6, 3, 8) and bits(stats) == bits(np.stack(want)) and bits(trained.params) == bits(stepped.params)
        drawn = cases.fresh_twin(spec, twin)
        got = harness.PopulationLearner(drawn, **cases.hypers_of(3)).train(_Finished(parts), 1, batch,
                                                                           generator=np.random.default_rng(5))
        again = cases.fresh_twin(spec, twin)
        split = np.random.default_rng(5).integers(rows, size=3)
        same = harness.PopulationLearner(again, **cases.hypers_of(3)).train(_Finished(parts), 1, batch, splits=[split])
    assert bits(got) == bits(same) and bits(drawn.params) == bits(again.params)


def test_learner_state_dicts_resume_every_group():
    u = cases.UPDATE
    shape = (lstm_cases.TUNED, False, u["groups"], u["steps"], u["per_group"])
    spec, twin, parts = cases.update_inputs(*shape)
    first = cases.fresh_twin(spec, twin)
    learner = harness.PopulationLearner(first, **cases.hypers_of(3))
    with np.errstate(all="ignore"):
        learner.update(parts, u["firsts"], 5)
        second = cases.fresh_twin(spec, twin)
        for g in range(3):
            second.load_state_dict(first.state_dict(group=g), group=g)
        resumed = harness.PopulationLearner(second, **cases.hypers_of(3))
        resumed.load_state_dict(learner.state_dict())
        assert bits(resumed.update(parts, (1, 2, 3), 12)) == bits(learner.update(parts, (1, 2, 3), 12))
    assert bits(first.params) == bits(second.params) and bits(cases.twin_states(resumed)) == bits(cases.twin_states(learner))


# ---- 2: the host build of the headers' size rules and addressing helpers ------------------------------------------------
@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
@pytest.mark.parametrize("index", range(len(lstm_cases.NETWORKS)))
def test_sizes_are_g_times_the_ungrouped_sizes(index, critic_lstm):
    lib = cases.hostcheck()
    spec = cases.spec_of(index, critic_lstm)
    desc = cases.critic_desc(spec)
    state = 4 * (32 // 4 + 2 * spec.size)
    for groups, per_group, steps, batch in ((1, 8, 8, 8), (3, 3, 4, 12), (512, 8, 128, 128), (65535, 1, 1, 1)):
        assert lib.lpop_state_size(ctypes.byref(desc), groups, per_group) == groups * state
        one = lib.lpop_workspace_size(ctypes.byref(desc), 1, per_group, steps, batch)
        assert one > 0 and one % 8 == 0
        assert lib.lpop_workspace_size(ctypes.byref(desc), groups, per_group, steps, batch) == groups * one
        if critic_lstm:
            ungrouped = lstm_learner_cases.hostcheck()
            plain = lstm_learner_cases._lstm_desc(spec)
            assert ungrouped.lpc_state_size(ctypes.byref(plain)) == state
            assert ungrouped.lpc_workspace_size(ctypes.byref(plain), batch) == one
    for groups, per_group in ((0, 8), (65536, 8), (-1, 8), (3, 0), (3, -2), (65535, 1 << 20)):
        assert lib.lpop_state_size(ctypes.byref(desc), groups, per_group) == 0, (groups, per_group)
    for groups, per_group, steps, batch in ((0, 3, 4, 5), (65536, 3, 4, 5), (3, 0, 4, 5), (3, 3, 0, 5), (3, 3, 4, 13),
                                            (3, 3, 4, 0), (3, 1024, 2, 1025), (1 << 15, 1 << 10, 1 << 6, 8)):
        assert lib.lpop_workspace_size(ctypes.byref(desc), groups, per_group, steps, batch) == 0, (groups, per_group, steps)
    assert lib.lpop_workspace_size(ctypes.byref(desc), 3, 1024, 2, 1024) > 0
    wrong = cases.critic_desc(spec)
    wrong.critic = 2
    assert lib.lpop_state_size(ctypes.byref(wrong), 3, 3) == 0 and lib.lpop_workspace_size(ctypes.byref(wrong), 3, 3, 4, 5) == 0


def test_a_population_at_the_defaults_needs_size_t_offsets():
    """sb3-contrib's defaults (H = 256, B = 128, P = 567 k parameters): the workspace of one group holds the packed gradient
    (P floats) and 2 x 12 H floats per row of da, gates and states, several MB -- so G = 512 is past 2^31 bytes and
    G = 2048 past 2^32, which is why every offset that grows with G is size_t and the size functions return 64 bits."""
    lib = cases.hostcheck()
    spec = cases.spec_of(lstm_cases.DEFAULT, True)
    desc = cases.critic_desc(spec)
    one = lib.lpop_workspace_size(ctypes.byref(desc), 1, 8, 128, 128)
    assert one > 4 * (spec.size + 128 * 2 * 12 * 256)
    assert lib.lpop_workspace_size(ctypes.byref(desc), 512, 8, 128, 128) == 512 * one > 1 << 31
    assert lib.lpop_workspace_size(ctypes.byref(desc), 2048, 8, 128, 128) == 2048 * one > 1 << 32


@pytest.mark.parametrize("first", (0, 7, 11))
@pytest.mark.parametrize("batch", (5, 12))
def test_grouped_addressing_restates_the_sequence_rule_per_group(first, batch):
    """The helpers the grouped kernels walk with (rf_lstm_ppo.h, over the single-form episode_starts [T + 1][G m]) against
    lstm_learner_io_cases.restated_rows over the group's own columns: rows wrap modulo m T inside the group, starts are
    read at column g m + e with row stride G m, and the entering state is lstm_states at environment g m + e with plane
    stride G m."""
    lib = cases.hostcheck()
    groups, steps, per_group = cases.UPDATE["groups"], cases.UPDATE["steps"], cases.UPDATE["per_group"]
    starts = cases.group_starts(groups, steps, per_group)
    hidden, lanes = 5, groups * per_group
    for g in range(groups):
        own = np.ascontiguousarray(starts[:, g * per_group:(g + 1) * per_group])
        want = lstm_learner_cases.restated_rows(own, steps, per_group, first, batch)
        rows, start, end, lane = (np.zeros(batch, dtype=np.int32) for _ in range(4))
        stride = lib.lpop_sequences(starts.ctypes.data, groups, per_group, g, steps, first, batch, rows.ctypes.data,
                                    start.ctypes.data, end.ctypes.data, lane.ctypes.data)
        assert stride == lanes
        assert [int(r) for r in rows] == [row for row, _, _ in want]
        assert [bool(s) for s in start] == [is_start for _, is_start, _ in want]
        begins = [b for b in range(batch) if want[b][1]]
        for b, nxt in zip(begins, begins[1:] + [batch]):
            assert end[b] == nxt
        for b, (row, is_start, source) in enumerate(want):
            env, step = row // steps, row % steps
            assert lane[b] == g * per_group + env
            if is_start and source != "zero":
                for net in range(2):
                    for which in range(2):
                        at = lib.lpop_state_at(groups, per_group, g, hidden, step, net, which, env, 3)
                        index = np.ravel_multi_index((step, net, which, g * per_group + env, 3),
                                                     (steps + 1, 2, 2, lanes, hidden))
                        assert at == index, (g, b, net, which)
    outside = ctypes.c_int(0)
    rows_of_group = steps * per_group
    assert lib.lpop_first(rows_of_group, rows_of_group, ctypes.byref(outside)) == rows_of_group - 1 and outside.value == 1
    assert lib.lpop_first(-1, rows_of_group, ctypes.byref(outside)) == 0 and outside.value == 1
    assert lib.lpop_first(first, rows_of_group, ctypes.byref(outside)) == first and outside.value == 0


# ---- 3: header, binding and library --------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    """Every entry point of "population lstm" is declared with its section tag, bound with as many arguments as it declares
    and has a Context method."""
    raw = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    assert "---- population lstm:" in raw
    tagged = re.findall(r"\b(?:int|unsigned long long) /\* population lstm \*/ (rf_\w+)\s*\(", raw)
    assert sorted(tagged) == ENTRY_POINTS
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    for name in ENTRY_POINTS:
        arguments = re.search(rf"\b(?:int|unsigned long long)\s+{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        bound = re.search(rf"lib\.{name}\.argtypes = \[(.*?)\]", source, flags=re.S).group(1).split(",")
        assert len(bound) == len(arguments.split(",")), name
        assert name in _native.SYMBOLS and hasattr(_native.Context, name[3:]), name


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(helpers.built("reinfocus_amd", "libreinfocus_hip.so"))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_a_null_context_is_refused_by_the_size_functions(no_gpu):  # noqa: F811
    lib = _native.load()
    desc = cases.critic_desc(cases.spec_of(lstm_cases.TUNED, True))
    assert lib.rf_lstm_ppo_grouped_state_size(None, ctypes.byref(desc), 3, 3) == 0
    assert lib.rf_lstm_ppo_grouped_workspace_size(None, ctypes.byref(desc), 3, 3, 4, 5) == 0


# ---- 4: refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(no_gpu):  # noqa: F811
    spec = cases.e2e_spec()
    make = harness.LstmPopulationPolicy
    with pytest.raises(ValueError, match="one seed per group"):
        make(spec, 3, [1, 2])
    with pytest.raises(ValueError, match="one seed per group"):
        make(spec, 3, 5)
    with pytest.raises(ValueError, match="groups"):
        make(spec, 0, [])
    with pytest.raises(ValueError, match="next step"):  # (the lstm-sde population)
        make(harness.LstmSdePolicySpec(4, lstm_hidden=9, pi=(6,), vf=(5,)), 2, [1, 2])
    with pytest.raises(ValueError, match="PopulationPolicy / DevicePopulationPolicy"):
        make(population_cases.e2e_spec(), 2, [1, 2])
    with pytest.raises(ValueError, match="out of scope"):  # (the Categorical population keeps refusing an lstm spec)
        harness.PopulationPolicy(spec, 2, [1, 2])
    with pytest.raises(ValueError, match="not divisible"):
        make(spec, 3, [1, 2, 3], num_envs=7)
    twin = make(spec, 3, [1, 2, 3])
    before = twin.rng_state()
    with pytest.raises(ValueError, match="not divisible"):
        twin.act(np.zeros((7, 4), dtype=F32), np.zeros(7, dtype=np.uint8))
    with pytest.raises(ValueError, match="not divisible"):
        twin.values(np.zeros((2, 4), dtype=F32), np.zeros(2, dtype=np.uint8))
    with pytest.raises(ValueError, match="a state has shape"):
        twin.set_lstm_state(np.zeros((2, 2, 9, 8), dtype=F32))
    with pytest.raises(ValueError, match="not divisible"):
        twin.set_lstm_state(np.zeros((2, 2, 7, 9), dtype=F32))
    assert twin.rng_state() == before and twin.lstm_state() is None
    with pytest.raises(ValueError, match="generator states"):
        twin.set_rng_state(before[:2])
    with pytest.raises(TypeError, match="PopulationPolicy"):
        harness.PopulationLearner(harness.LstmPolicy(spec, 0))
    with pytest.raises(TypeError, match="DevicePopulationPolicy"):
        harness.DevicePopulationLearner(twin)
    with pytest.raises(TypeError, match="LstmPolicy"):
        harness.LstmLearner(twin)
    learner = harness.PopulationLearner(twin)
    env = cases.e2e_env(False)
    try:
        with pytest.raises(TypeError, match="device-resident"):
            harness.DevicePopulationLstmPolicy(env, spec, 3, [1, 2, 3])
        rollout = harness.Rollout(env, 2)
        rollout.start(env.reset()[0])
        rollout.collect(twin)
        assert rollout.lstm_states.shape == (3, 2, 2, 9, 9) and rollout.episode_starts.shape == (3, 9)
        kept = twin.params.copy()
        with pytest.raises(ValueError, match="more than the 6 rows"):
            learner.train(rollout, 1, 7)
        with pytest.raises(ValueError, match="batch_size"):
            learner.train(rollout, 1, 1025)
        for splits in ([[0, 1, 2]] * 2, [0, 1, 2], [[0, 1]], [[0, 1, 6]], [[0, -1, 2]], [[0.5, 1, 2]]):
            with pytest.raises(ValueError, match="splits must be"):
                learner.train(rollout, 1, 4, splits)
        with pytest.raises(ValueError, match="firsts must be"):
            learner.update(rollout, [0, 1], 4)
        with pytest.raises(ValueError, match="firsts must be"):
            learner.update(rollout, [0, 1, 6], 4)
        with pytest.raises(ValueError, match="a minibatch of 7"):
            learner.update(rollout, [0, 1, 2], 7)
        with pytest.raises(TypeError, match="firsts, count"):
            learner.update(rollout, [0, 1, 2])
        with pytest.raises(TypeError, match="splits belong"):
            harness.PopulationLearner(harness.PopulationPolicy(population_cases.e2e_spec(), 3, [1, 2, 3])).train(
                rollout, 1, 4, splits=[[0, 1, 2]])
        plain = harness.Rollout(env, 2)
        plain.start(env.reset()[0])
        plain.collect(harness.PopulationPolicy(population_cases.e2e_spec(), 3, [1, 2, 3]))
        with pytest.raises(ValueError, match="no lstm_states"):  # (collected without a recurrent policy)
            learner.train(plain, 1, 4)
        nine = harness.Rollout(env, 2, groups=9)
        nine.start(env.reset()[0])
        with pytest.raises(ValueError, match="population policy of 3 groups"):
            nine.collect(twin)
        nine.collect(make(spec, 9, list(range(9))))
        with pytest.raises(ValueError, match="groups=9"):  # (a rollout made with another groups=)
            learner.train(nine, 1, 2)
        assert bits(twin.params) == bits(kept)
        assert learner.train(rollout, 1, 4, [[0, 5, 3]]).shape == (2, 3, 8)
    finally:
        env.close()
    box = _Finished(cases.update_inputs(lstm_cases.TUNED, True, 3, 4, 3)[2])
    box.env = type("env", (), {"single_action_space": harness.spaces.Box(-1.0, 1.0, (1,))})
    with pytest.raises(ValueError, match="out of scope"):
        harness.PopulationLearner(cases.twin_policy(lstm_cases.TUNED, True, 3)[1]).train(box, 1, 4)


def test_collect_keeps_the_recurrent_slabs_of_a_population(no_gpu):  # noqa: F811
    """Rollout.collect with the twin population over 9 lanes equals three stand-alone rollouts' policies on their lanes: the
    slabs' lstm_states columns [g m, (g + 1) m) are what LstmPolicy(seed g) gives from the same observations."""
    runs, rng, states, lstm_state = cases.e2e_twin_runs(True)
    assert len(runs) == cases.E2E["iterations"] and len(rng) == 3 and states.shape[0] == 3
    first = runs[0]
    spec = cases.e2e_spec(True)
    lanes = cases.E2E["groups"] * cases.E2E["per_group"]
    assert first["lstm_states"].shape == (cases.E2E["steps"] + 1, 2, 2, lanes, spec.lstm_hidden)
    assert (first["episode_starts"][0] == 1).all() and not first["lstm_states"][0].any()
    for g, seed in enumerate(cases.seeds_of(3)):
        member = harness.LstmPolicy(spec, seed)
        member.load_state_dict(cases.e2e_states(spec)[g])
        rows = slice(g * 3, (g + 1) * 3)
        state = np.zeros(spec.state_shape(3), dtype=F32)
        for t in range(cases.E2E["steps"]):
            after = np.zeros_like(state)
            got = member.act(first["observations"][t][rows], first["episode_starts"][t][rows], None, False,
                             states=(state, after))
            assert bits(got[0]) == bits(first["actions"][t][rows]) and bits(got[2]) == bits(first["log_probs"][t][rows])
            assert bits(after) == bits(first["lstm_states"][t + 1][:, :, rows, :]), (g, t)
            state = after
    assert bits(runs[1]["lstm_states"][0]) == bits(first["lstm_states"][cases.E2E["steps"]])
    assert bits(lstm_state) == bits(runs[1]["lstm_states"][cases.E2E["steps"]])


def test_import_stays_free_of_torch():
    import subprocess
    import sys

    code = ("import sys; from reinfocus_amd.environments import harness; "
            "harness.LstmPopulationPolicy; harness.DevicePopulationLstmPolicy; assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
