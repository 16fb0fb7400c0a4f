"""CPU tests of the population of recurrent gSDE learners (include/reinfocus_hip.h, "population lstm sde"): the numpy twins
harness.LstmSdePopulationPolicy / PopulationLearner over it are literally G of the existing twins (lstm_sde.LstmSdePolicy,
lstm_learner.LstmLearner) over copied slices -- noise with a mask, act, values, two updates, collect() + train() with a
log_std_init and an sde_sample_freq per group --, the host build of the kernels' headers (tests/lstmsdepopcheck) gives the
twin's sizes, offsets and bytes through the grouped addressing, header, binding and library agree on the five entry points,
and the surface refuses what it cannot express.  The arithmetic of one group is held to the host build of the kernels'
functions by tests/test_lstm_sde_logic.py; nothing here needs a GPU.  tests/test_gpu_population_lstm_sde.py holds the device
classes and the grouped entry points to these twins as bytes."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, learner as learner_module, population
from tests import helpers
from tests import population_io_cases as population_cases
from tests import population_lstm_io_cases as lstm_pop
from tests import population_lstm_sde_io_cases as cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits


def _members(spec, twin, per_group):
    """G stand-alone LstmSdePolicy twins with the population's seeds and parameters."""
    members = []
    for g, seed in enumerate(cases.seeds_of(twin.groups)):
        member = harness.LstmSdePolicy(spec, seed, num_envs=per_group)
        member.params = twin.params[g].copy()
        members.append(member)
    return members


def _alone(member, h):
    return harness.LstmLearner(member, h.learning_rate, h.clip_range, h.ent_coef, h.vf_coef, h.max_grad_norm,
                               bool(h.normalize_advantage), (h.beta1, h.beta2), h.adam_eps)


# ---- 1: the twins are G stand-alone twins over copied slices ------------------------------------------------------------
@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
@pytest.mark.parametrize("per_group", cases.PER_GROUP)
@pytest.mark.parametrize("groups", cases.GROUPS)
@pytest.mark.parametrize("index", cases.NETS)
def test_population_policy_is_g_policies_over_slices(index, groups, per_group, critic_lstm):
    """reset_noise(), two chained act() calls in place (sampled, then deterministic), one from `in` to `out`, and values():
    theta, every output and the whole state equal G LstmSdePolicy over contiguous copies of the lanes' slices, generator
    states included; every group has its own log_std."""
    spec, twin = cases.twin_policy(index, critic_lstm, groups, per_group)
    twin = cases.fresh_twin(spec, twin)
    members = _members(spec, twin, per_group)
    obs, final_obs, starts, state = cases.forward_inputs(index, groups, per_group)
    lanes = [slice(g * per_group, (g + 1) * per_group) for g in range(groups)]
    assert len({bits(row[spec.log_std_at:]) for row in twin.params}) == groups
    twin.set_lstm_state(state)
    twin.reset_noise()
    for member, rows in zip(members, lanes):
        member.set_lstm_state(np.ascontiguousarray(state[:, :, rows, :]))
        member.reset_noise()
        assert bits(twin.noise()[rows]) == bits(member.noise())
    with np.errstate(all="ignore"):
        for deterministic, flags in ((False, starts), (True, np.zeros_like(starts))):
            got = twin.act(obs, flags, final_obs, deterministic)
            assert len(got) == 5 and got[0].dtype == F32
            for g, (member, rows) in enumerate(zip(members, lanes)):
                want = member.act(obs[rows].copy(), flags[rows].copy(), final_obs[rows].copy(), deterministic)
                for i in range(5):
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
    cases.wanted_forward(index, critic_lstm, groups, per_group, False)  # (its own checks against act())


@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
@pytest.mark.parametrize("index", cases.NETS)
def test_the_state_plane_stride_shows(index, critic_lstm):
    cases.stride_promises(index, critic_lstm)


@pytest.mark.parametrize("mask", cases.NOISE["masks"])
@pytest.mark.parametrize("index", cases.NETS)
def test_a_masked_reset_leaves_the_other_groups_alone(index, mask):
    """G = 3, m = 3, generators that had given (0, 2^32 + 5, 7) draws: a selected group's rows of theta are what a
    stand-alone LstmSdePolicy draws from the generator advanced that far, and its generator moves on by m L; an unselected
    group keeps its theta (the NaN rows it was given) and its generator state."""
    n = cases.NOISE
    groups, per_group = n["groups"], n["per_group"]
    spec, twin = cases.twin_policy(index, True, groups, per_group)
    theta, after = cases.wanted_noise(index, True, mask)
    for g, (seed, consumed) in enumerate(zip(cases.seeds_of(groups), n["consumed"])):
        rows = slice(g * per_group, (g + 1) * per_group)
        before = cases.generator_of(seed, consumed)
        if mask is None or mask[g]:
            member = harness.LstmSdePolicy(spec, seed, num_envs=per_group)
            member.params = twin.params[g].copy()
            member.set_rng_state(before.state)
            member.reset_noise()
            assert bits(theta[rows]) == bits(member.noise()), g
            assert after[g] == member.rng_state() == cases.generator_of(seed, consumed + per_group * spec.latent).state
        else:
            assert np.isnan(theta[rows]).all() and after[g] == before.state, g


@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
@pytest.mark.parametrize("batch", cases.UPDATE["batches"])
@pytest.mark.parametrize("index", cases.NETS)
def test_population_learner_is_g_learners_over_slices(index, batch, critic_lstm):
    """Two consecutive updates of three groups with firsts (0, 7, 11) and starts that differ per group over float32 raw
    actions: parameters (log_std included), optimizer states and stats equal G LstmLearner over contiguous copies of the
    slice-parts, each with its own hyper-parameters."""
    u = cases.UPDATE
    shape = (index, critic_lstm, u["groups"], u["steps"], u["per_group"])
    spec, twin, parts = cases.update_inputs(*shape)
    assert parts["actions"].dtype == F32
    want = cases.twin_updates(*shape, u["firsts"], batch, u["updates"])
    hypers = harness.PopulationLearner(cases.fresh_twin(spec, twin), **cases.hypers_of(u["groups"])).hypers()
    rows = u["steps"] * u["per_group"]
    for g, member in enumerate(_members(spec, twin, u["per_group"])):
        alone = _alone(member, hypers[g])
        piece = cases.group_slices(parts, u["groups"], g)
        with np.errstate(all="ignore"):
            for update in range(u["updates"]):
                stats = alone.update(piece, cases.firsts_of(u["firsts"], update, rows)[g], batch)
                assert bits(stats) == bits(want[update][2][g]), (g, update)
                assert bits(member.params) == bits(want[update][0][g]) and bits(alone.state) == bits(want[update][1][g])
    cases.update_promises(index, critic_lstm, batch)


@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
def test_a_skipped_group_leaves_the_others_alone(critic_lstm):
    """A NaN raw action in group 1's minibatch flags group 1 alone (RF_PPO_INVALID) and leaves it where it was; groups 0
    and 2 are those of the undisturbed run."""
    u = cases.UPDATE
    shape = (cases.NETS[1], critic_lstm, u["groups"], u["steps"], u["per_group"])
    spec, twin, _ = cases.update_inputs(*shape)
    nan_row, _ = cases.isolation_rows()
    clean = cases.twin_updates(*shape, u["firsts"], 5, 1)[0]
    got = cases.twin_updates(*shape, u["firsts"], 5, 1, nan_row=nan_row)[0]
    assert got[2][1][7] == cases.INVALID and bits(got[0][1]) == bits(twin.params[1])
    for g in (0, 2):
        assert all(bits(x[g]) == bits(y[g]) for x, y in zip(got, clean)), g
        assert clean[2][g][7] == 0


@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
def test_the_depth_layout_holds_its_sequences(critic_lstm):
    """T = 17, m = 4, B = 65: every group's minibatch holds sequences of 1, 8, 9, 16 and 17 rows (or the pieces its own first
    row cuts them into), the groups' structures differ, and no update of the twin is skipped."""
    shape, kind, firsts, batch = cases.depth_shape(critic_lstm)
    groups, steps, per_group = shape[2:]
    parts = cases.update_inputs(*shape, kind)[2]
    lib = lstm_pop.hostcheck()
    seen = set()
    for g in range(groups):
        rows, start, end, lane = (np.zeros(batch, dtype=np.int32) for _ in range(4))
        lib.lpop_sequences(parts["episode_starts"].ctypes.data, groups, per_group, g, steps, firsts[g], batch,
                           rows.ctypes.data, start.ctypes.data, end.ctypes.data, lane.ctypes.data)
        lengths = tuple(int(end[b]) - b for b in range(batch) if start[b])
        assert sum(lengths) == batch and max(lengths) >= 16 and min(lengths) == 1, (g, lengths)
        seen.add((lengths, tuple(rows)))
    assert len(seen) == groups
    want = cases.twin_updates(*shape, firsts, batch, cases.DEPTH["updates"], kind)
    assert all((stats[:, 7] == 0).all() for _, _, stats in want)


def test_collect_and_train_equal_a_loop_over_stand_alone_learners(no_gpu):  # noqa: F811
    """Two iterations of Rollout.collect(sde_sample_freq=(-1, 2, 1)) + train(splits) of the twin population on the numpy
    ContinuousJumps twin, groups with log_std_init (-1, -0.5, 0.25): group g's columns of every slab -- raw actions,
    log-probabilities, values, episode_starts, lstm_states -- are what a stand-alone LstmSdePolicy(seed g) gives from the
    same observations under its own noise schedule, and its parameters and optimizer state after train() what a
    stand-alone LstmLearner gives from the group's slice of the rollout."""
    e = cases.E2E
    groups, m, steps = e["groups"], e["per_group"], e["steps"]
    runs, rng, states, lstm_state = cases.e2e_twin_runs(True)
    cases.e2e_promises(runs)
    env = cases.e2e_env(False)
    try:
        spec = cases.e2e_spec(env, True)
    finally:
        env.close()
    hypers = harness.PopulationLearner(
        harness.LstmSdePopulationPolicy(spec, groups, cases.seeds_of(groups)), **cases.e2e_hypers()).hypers()
    for g, seed in enumerate(cases.seeds_of(groups)):
        rows = slice(g * m, (g + 1) * m)
        member = harness.LstmSdePolicy(spec, seed, num_envs=m)
        assert member.params[spec.log_std_at] == 0.0
        member.load_state_dict(cases.e2e_states(spec)[g])
        assert member.params[spec.log_std_at] == F32(e["log_std"][g])
        alone = _alone(member, hypers[g])
        freq = e["freqs"][g]
        for iteration, run in enumerate(runs):
            state = run["lstm_states"][0][:, :, rows, :].copy()
            member.reset_noise()
            for t in range(steps):
                if freq > 0 and t % freq == 0:
                    member.reset_noise()
                after = np.zeros_like(state)
                got = member.act(run["observations"][t][rows], run["episode_starts"][t][rows], None, False,
                                 states=(state, after))
                assert bits(got[0]) == bits(run["actions"][t][rows]), (g, iteration, t)
                assert bits(got[2]) == bits(run["log_probs"][t][rows]) and bits(got[1]) == bits(run["values"][t][rows])
                assert bits(after) == bits(run["lstm_states"][t + 1][:, :, rows, :]), (g, iteration, t)
                state = after
            assert bits(member.noise()) == bits(run["theta"][rows]), (g, iteration)
            parts = {key: run["flat/" + key] for key in learner_module.BATCH_KEYS}
            parts.update(episode_starts=run["episode_starts"], lstm_states=run["lstm_states"], n_steps=steps,
                         num_envs=groups * m)
            piece = lstm_pop.group_slices(parts, groups, g)
            stats = alone.train(_Finished(piece), e["epochs"], e["batch"], splits=cases.e2e_splits(iteration)[:, g])
            assert bits(stats) == bits(run["stats"][:, g]), (g, iteration)
            assert bits(member.params) == bits(run["params"][g]), (g, iteration)
        assert bits(alone.state) == bits(states[g]) and member.rng_state() == rng[g]
    assert bits(runs[1]["lstm_states"][0]) == bits(runs[0]["lstm_states"][steps])
    assert bits(lstm_state) == bits(runs[1]["lstm_states"][steps])


class _Finished:
    """A finished rollout of one group's slice, as LstmLearner.train reads it."""

    def __init__(self, parts):
        self._parts = parts
        self.n_steps, self.num_envs = parts["n_steps"], parts["num_envs"]
        self.episode_starts, self.lstm_states = parts["episode_starts"], parts["lstm_states"]
        self.env = type("env", (), {"single_action_space": harness.spaces.Box(-1.0, 1.0, (1,))})

    def flat(self):
        return {key: self._parts[key] for key in learner_module.BATCH_KEYS}


def test_state_dicts_resume_bit_for_bit():
    """PopulationLearner.state_dict() / load_state_dict() and the policy's per-group state_dict (log_std included) carry a
    second population on bit for bit."""
    u = cases.UPDATE
    shape = (cases.NETS[1], True, u["groups"], u["steps"], u["per_group"])
    spec, twin, parts = cases.update_inputs(*shape)
    first = cases.fresh_twin(spec, twin)
    one = harness.PopulationLearner(first, **cases.hypers_of(u["groups"]))
    with np.errstate(all="ignore"):
        one.update(parts, list(u["firsts"]), 5)
        second = harness.LstmSdePopulationPolicy(spec, u["groups"], cases.seeds_of(u["groups"]))
        for g in range(u["groups"]):
            state = first.state_dict(group=g)
            assert state["log_std"].shape == (spec.latent, 1)
            second.load_state_dict(state, group=g)
        assert bits(second.params) == bits(first.params)
        other = harness.PopulationLearner(second, **cases.hypers_of(u["groups"]))
        other.load_state_dict(one.state_dict())
        a, b = one.update(parts, [1, 8, 0], 5), other.update(parts, [1, 8, 0], 5)
    assert bits(a) == bits(b) and bits(first.params) == bits(second.params)
    assert bits(cases.twin_states(one)) == bits(cases.twin_states(other))


# ---- 2: the host build of the kernels' headers -----------------------------------------------------------------------------
@pytest.mark.parametrize("critic_lstm", cases.CRITICS)
@pytest.mark.parametrize("index", cases.NETS + (cases.SMALL,))
def test_sizes_and_offsets_of_the_host_build(index, critic_lstm):
    """rf_lstm_sde_grouped_state_size is G (32 + 8 (P + L)), rf_lstm_sde_grouped_workspace_size G times tests/lstmsdecheck's
    ungrouped lstm-sde workspace (LSTM critic) and 0 where the Categorical population's is; group g's theta begins at g m L
    floats, its raw actions at g m T floats -- not at int64 elements --, its log_std at g (P + L) + P."""
    from tests import lstm_sde_io_cases as lsde_cases

    lib = cases.hostcheck()
    spec = cases.spec_of(index, critic_lstm)
    desc = cases.critic_desc(spec)
    P = spec.size
    for groups, m, steps, batch in ((1, 1, 1, 1), (3, 3, 4, 5), (3, 3, 4, 12), (64, 8, 8, 8), (65535, 1, 1, 1)):
        assert lib.lspop_state_size(ctypes.byref(desc), groups, m) == groups * (32 + 8 * P)
        size = lib.lspop_workspace_size(ctypes.byref(desc), groups, m, steps, batch)
        assert size > 0 and size % (8 * groups) == 0
        if critic_lstm:
            alone = lsde_cases.hostcheck().lsc_workspace_size(ctypes.byref(lsde_cases._lstm_desc(spec)), batch)
            assert size == groups * alone
        plain = lstm_pop.hostcheck().lpop_workspace_size(ctypes.byref(desc), groups, m, steps, batch)
        assert plain == 0 or size > plain  # (the Gaussian head's per-row sigma terms and P + L gradients)
        for g in sorted({0, 1 % groups, groups - 1}):
            theta, actions, log_std = ctypes.c_ulonglong(), ctypes.c_ulonglong(), ctypes.c_ulonglong()
            total, latent = ctypes.c_uint(), ctypes.c_uint()
            assert lib.lspop_offsets(ctypes.byref(desc), m, steps, g, ctypes.byref(theta), ctypes.byref(actions),
                                     ctypes.byref(log_std), ctypes.byref(total), ctypes.byref(latent)) == 0
            assert (total.value, latent.value) == (P, spec.latent)
            assert theta.value == g * m * spec.latent and actions.value == g * m * steps
            assert log_std.value == g * P + spec.log_std_at == (g + 1) * P - spec.latent
    for refused in ((0, 3, 4, 5), (65536, 1, 1, 1), (3, 0, 4, 5), (3, 3, 0, 5), (3, 3, 4, 13), (3, 3, 4, 0), (3, 400, 400, 1025)):
        assert lib.lspop_workspace_size(ctypes.byref(desc), *refused) == 0, refused
    assert lib.lspop_state_size(ctypes.byref(desc), 0, 3) == 0 and lib.lspop_state_size(ctypes.byref(desc), 65536, 1) == 0
    bad = _native.LstmCriticDesc(*(tuple(spec.critic_desc()[:-1]) + (2,)))
    assert lib.lspop_state_size(ctypes.byref(bad), 3, 3) == 0


@pytest.mark.parametrize("index", cases.NETS)
def test_the_host_build_gives_the_twins_bytes(index):
    """The grouped noise reset (masked, generators (0, 2^32 + 5, 7) draws on), forward (sampled and deterministic, the state in
    its single form) and two updates as loops over the groups through the grouped addressing of the kernels' headers give
    the twin population's bytes (the LSTM critic: what tests/lstmsdecheck's host loops compute)."""
    from reinfocus_amd.environments import policy

    lib = cases.hostcheck()
    n = cases.NOISE
    groups, per_group = n["groups"], n["per_group"]
    spec, twin = cases.twin_policy(index, True, groups, per_group)
    desc = cases.critic_desc(spec)
    pointer = lambda a: a.ctypes.data  # noqa: E731
    gens = np.array([policy.generator_words(np.random.PCG64DXSM(seed)) for seed in cases.seeds_of(groups)], dtype=np.uint64)
    consumed = np.array(n["consumed"], dtype=np.uint64)
    for mask in n["masks"]:
        want, _ = cases.wanted_noise(index, True, mask)
        theta = np.full((groups * per_group, spec.latent), np.nan, dtype=F32)
        select = None if mask is None else np.array(mask, dtype=np.uint8)
        assert lib.lspop_noise(ctypes.byref(desc), groups, per_group, pointer(twin.params), pointer(gens), pointer(consumed),
                               None if select is None else pointer(select), pointer(theta)) == 0
        assert bits(theta) == bits(want), mask
    per_group = cases.STRIDE[1]
    obs, final_obs, starts, state = cases.forward_inputs(index, groups, per_group)
    for deterministic in (False, True):
        want, theta = cases.wanted_forward(index, True, groups, per_group, deterministic)
        out = {name: np.zeros(groups * per_group, dtype=F32) for name in cases.OUTPUTS}
        after = np.zeros_like(state)
        assert lib.lspop_forward(ctypes.byref(desc), groups, per_group, pointer(twin.params), pointer(obs), pointer(starts),
                                 pointer(state), pointer(after), None if deterministic else pointer(theta),
                                 *(pointer(out[name]) for name in cases.OUTPUTS if name != "final_values")) == 0
        for name in cases.OUTPUTS:
            if name != "final_values":
                assert bits(out[name]) == bits(want[name]), (deterministic, name)
        assert bits(after) == bits(want["state"]), deterministic
    u = cases.UPDATE
    shape = (index, True, u["groups"], u["steps"], u["per_group"])
    spec, twin, parts = cases.update_inputs(*shape)
    hypers = harness.PopulationLearner(cases.fresh_twin(spec, twin), **cases.hypers_of(u["groups"])).hypers()
    records = (_native.PpoDesc * u["groups"])(*(_native.PpoDesc(*h) for h in hypers))
    rows = u["steps"] * u["per_group"]
    for batch in u["batches"]:
        want = cases.twin_updates(*shape, u["firsts"], batch, u["updates"])
        params = twin.params.copy()
        state = np.stack([learner_module.fresh_state(spec) for _ in range(u["groups"])])
        stats = np.zeros((u["groups"], 8), dtype=F32)
        for update in range(u["updates"]):
            firsts = np.array(cases.firsts_of(u["firsts"], update, rows), dtype=np.int32)
            assert lib.lspop_update(ctypes.byref(desc), u["groups"], u["per_group"], u["steps"], records, pointer(params),
                                    pointer(state), pointer(parts["observations"]), pointer(parts["actions"]),
                                    pointer(parts["log_probs"]), pointer(parts["advantages"]), pointer(parts["returns"]),
                                    pointer(parts["episode_starts"]), pointer(parts["lstm_states"]), pointer(firsts), batch,
                                    pointer(stats)) == 0
            for name, x, y in zip(("parameters", "states", "stats"), (params, state, stats), want[update]):
                assert bits(x) == bits(y), (batch, update, name)
    _, outside = cases.isolation_rows()
    params, state = twin.params.copy(), np.stack([learner_module.fresh_state(spec) for _ in range(u["groups"])])
    firsts = np.array(outside, dtype=np.int32)
    assert lib.lspop_update(ctypes.byref(desc), u["groups"], u["per_group"], u["steps"], records, pointer(params),
                            pointer(state), pointer(parts["observations"]), pointer(parts["actions"]),
                            pointer(parts["log_probs"]), pointer(parts["advantages"]), pointer(parts["returns"]),
                            pointer(parts["episode_starts"]), pointer(parts["lstm_states"]), pointer(firsts), 5,
                            pointer(stats)) == 0
    clean = cases.twin_updates(*shape, u["firsts"], 5, 1)[0]
    assert stats[1][7] == cases.INVALID and bits(params[1]) == bits(twin.params[1])
    assert bits(params[0]) == bits(clean[0][0]) and bits(params[2]) == bits(clean[0][2])


def test_stand_alone_program_runs():
    """tests/lstmsdepopcheck/lstmsdepopcheck: the same source with its own main -- one grouped noise reset, forwards and one
    update of two groups on a tiny network, printed; the form a host sanitizer build takes."""
    helpers.built("tests/lstmsdepopcheck", "liblstmsdepopcheck.so")  # (the Makefile rule that builds both)
    done = subprocess.run([os.path.join(ROOT, "tests", "lstmsdepopcheck", "lstmsdepopcheck")], capture_output=True, text=True,
                          timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    lines = done.stdout.splitlines()
    assert len(lines) == 6 and lines[-1].startswith("group 1 stats:") and lines[0].startswith("group 0 env 0: action")
    for line in lines:
        figures = [float(word) for word in re.findall(r"-?\d+\.?\d*(?:e[-+]?\d+)?", line.split(":", 1)[1])]
        assert figures and np.isfinite(figures).all(), line


def test_the_limit_arrays_cover_every_combination():
    """The 65535 groups of the limit case: neighbours differ in parameters, log_std, input block, theta level, draw count
    and hyper-parameters; 5958 groups start outside, 13107 are left out of the noise reset; the twin functions skip no
    combination and leave none where it began."""
    inputs, theta, forwards, updates = cases.limit_arrays(True, groups=1200)
    spec = cases.spec_of(0, True)
    for key in ("params", "observations", "theta", "consumed", "actions"):
        a = inputs[key].reshape(1200, -1)
        assert (a[1:] != a[:-1]).any(axis=1).all(), key
    assert (inputs["params"][1:, spec.log_std_at] != inputs["params"][:-1, spec.log_std_at]).all()
    assert np.isnan(theta[~inputs["selected"]]).all() and np.isfinite(theta[inputs["selected"]]).all()
    assert inputs["actions"].dtype == F32 and inputs["firsts"].dtype == np.int32
    assert (updates[2][:, 7] == 0).all() and (updates[0] != inputs["params"]).any(axis=1).all()
    assert bits(forwards[False]["actions"]) != bits(forwards[True]["actions"])
    assert bits(forwards[True]["actions"]) == bits(forwards[True]["mean"])
    g = np.arange(cases.LIMIT_GROUPS)
    assert int((g % 11 == 5).sum()) == 5958 and int((g % 5 == 2).sum()) == 13107


# ---- 3: header, binding and library --------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    """Every entry point of "population lstm sde" is declared with its section tag, bound with as many arguments as it
    declares, has a Context method and a definition that selects the context's device in the unit of its own."""
    raw = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    assert "---- population lstm sde:" in raw
    tagged = re.findall(r"\b(?:int|unsigned long long) /\* population lstm sde \*/ (rf_\w+)\s*\(", raw)
    assert sorted(tagged) == cases.ENTRY_POINTS
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    unit = open(os.path.join(ROOT, "reinfocus_amd", "csrc", "rf_abi_lstm_sde_grouped.hip")).read()
    for name in cases.ENTRY_POINTS:
        arguments = re.search(rf"\b(?:int|unsigned long long)\s+{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        bound = re.search(rf"lib\.{name}\.argtypes = \[(.*?)\]", source, flags=re.S).group(1).split(",")
        assert len(bound) == len(arguments.split(",")), name
        assert name in _native.SYMBOLS and hasattr(_native.Context, name[3:]), name
        body = re.search(rf"\n(?:int|unsigned long long) {name}\(rf_ctx \*ctx,.*?\n}}\n", unit, flags=re.S)
        assert body is not None and "hipSetDevice(ctx->device)" in body.group(0), name
        if name.endswith("_size"):
            assert re.search(rf"lib\.{name}\.restype = ctypes\.c_ulonglong", source), name
    assert "rf_abi_lstm_sde_grouped.hip" in open(os.path.join(ROOT, "reinfocus_amd", "csrc", "Makefile")).read()
    for header in ("rf_lstm.h", "rf_lstm_ppo.h"):
        assert "has no population yet" not in open(os.path.join(ROOT, "reinfocus_amd", "csrc", header)).read()


def test_library_exports_the_entry_points():
    lib = ctypes.CDLL(helpers.built("reinfocus_amd", "libreinfocus_hip.so"))
    for name in cases.ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_a_null_context_is_refused_by_the_size_functions(no_gpu):  # noqa: F811
    lib = _native.load()
    desc = cases.critic_desc(cases.spec_of(cases.SMALL, True))
    assert lib.rf_lstm_sde_grouped_state_size(None, ctypes.byref(desc), 3, 3) == 0
    assert lib.rf_lstm_sde_grouped_workspace_size(None, ctypes.byref(desc), 3, 3, 4, 5) == 0


# ---- 4: refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(no_gpu):  # noqa: F811
    env = cases.e2e_env(False)
    steps_env = lstm_pop.e2e_env(False)
    try:
        spec = cases.e2e_spec(env)
        make = harness.LstmSdePopulationPolicy
        with pytest.raises(ValueError, match="one seed per group"):
            make(spec, 3, [1, 2])
        with pytest.raises(ValueError, match="one seed per group"):
            make(spec, 3, 5)
        with pytest.raises(ValueError, match="groups"):
            make(spec, 0, [])
        with pytest.raises(ValueError, match="log_std_init has 2 entries"):
            make(spec, 3, [1, 2, 3], log_std_init=[0.0, 1.0])
        for other in (lstm_pop.e2e_spec(), population_cases.e2e_spec(), harness.SdePolicySpec(4)):
            with pytest.raises(ValueError, match="Gaussian head of LstmSdePolicySpec"):
                make(other, 2, [1, 2])
        with pytest.raises(ValueError, match="next step"):  # (the Categorical recurrent population keeps refusing this head)
            harness.LstmPopulationPolicy(spec, 2, [1, 2])
        with pytest.raises(ValueError, match="lstm"):
            harness.SdePopulationPolicy(spec, 2, [1, 2])
        with pytest.raises(ValueError, match="not divisible"):
            make(spec, 3, [1, 2, 3], num_envs=7)
        twin = make(spec, 3, [1, 2, 3], log_std_init=[-1.0, 0.0, 0.5])
        assert twin.params[:, spec.log_std_at].tolist() == [-1.0, 0.0, 0.5]
        before = twin.rng_state()
        width = spec.obs_width
        with pytest.raises(ValueError, match="not divisible"):
            twin.act(np.zeros((7, width), dtype=F32), np.zeros(7, dtype=np.uint8))
        with pytest.raises(ValueError, match="reset_noise\\(\\) of every group"):
            twin.act(np.zeros((9, width), dtype=F32), np.zeros(9, dtype=np.uint8))
        with pytest.raises(ValueError, match="boolean sequence"):
            twin.reset_noise(groups=[True, False])
        with pytest.raises(ValueError, match="not divisible"):
            twin.reset_noise(num_envs=7)
        with pytest.raises(ValueError, match="a state has shape"):
            twin.set_lstm_state(np.zeros((2, 2, 9, 8), dtype=F32))
        assert twin.rng_state() == before and twin.lstm_state() is None and twin.noise() is None
        twin.reset_noise(groups=[True, False, True], num_envs=9)
        with pytest.raises(ValueError, match="reset_noise\\(\\) of every group"):  # (group 1 has none yet; no state moved)
            twin.act(np.zeros((9, width), dtype=F32), np.zeros(9, dtype=np.uint8))
        assert twin.lstm_state() is None and twin.rng_state()[1] == before[1] and twin.rng_state()[0] != before[0]
        with pytest.raises(ValueError, match="generator states"):
            twin.set_rng_state(before[:2])
        with pytest.raises(TypeError, match="PopulationPolicy"):
            harness.PopulationLearner(harness.LstmSdePolicy(spec, 0))
        with pytest.raises(TypeError, match="DevicePopulationPolicy"):
            harness.DevicePopulationLearner(twin)
        with pytest.raises(TypeError, match="LstmPolicy"):
            harness.LstmLearner(twin)
        with pytest.raises(TypeError, match="device-resident"):
            harness.DevicePopulationLstmSdePolicy(env, spec, 3, [1, 2, 3])
        learner = harness.PopulationLearner(twin)
        rollout = harness.Rollout(env, 2)
        rollout.start(env.reset()[0])
        kept_rng = twin.rng_state()
        with pytest.raises(ValueError, match="sde_sample_freq has 2 entries"):
            rollout.collect(twin, sde_sample_freq=[1, 2])
        with pytest.raises(ValueError, match="is not -1 or a positive integer"):
            rollout.collect(twin, sde_sample_freq=[1, 0, 2])
        assert twin.rng_state() == kept_rng
        rollout.collect(twin, sde_sample_freq=[-1, 2, 1])
        assert rollout.lstm_states.shape == (3, 2, 2, 9, 9) and rollout.episode_starts.shape == (3, 9)
        assert rollout.actions.dtype == F32
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
        plain = harness.Rollout(env, 2)
        plain.start(env.reset()[0])
        plain.collect(harness.SdePopulationPolicy(harness.SdePolicySpec(width, pi=(6,), vf=(5,)), 3, [1, 2, 3]))
        with pytest.raises(ValueError, match="no lstm_states"):  # (collected without a recurrent policy)
            learner.train(plain, 1, 4)
        nine = harness.Rollout(env, 2, groups=9)
        nine.start(env.reset()[0])
        with pytest.raises(ValueError, match="population policy of 3 groups"):
            nine.collect(twin)
        nine.collect(make(spec, 9, list(range(9))))
        with pytest.raises(ValueError, match="groups=9"):  # (a rollout made with another groups=)
            learner.train(nine, 1, 2)
        discrete = harness.Rollout(steps_env, 2)
        discrete.start(steps_env.reset()[0])
        with pytest.raises(ValueError):  # (a Discrete task has no Gaussian head)
            discrete.collect(twin)
        discrete.collect(harness.LstmPopulationPolicy(lstm_pop.e2e_spec(), 3, [1, 2, 3]))
        with pytest.raises(ValueError, match="Gaussian head over a Box"):
            learner.train(discrete, 1, 4)
        assert bits(twin.params) == bits(kept)
        assert learner.train(rollout, 1, 4, [[0, 5, 3]]).shape == (2, 3, 8)
    finally:
        env.close()
        steps_env.close()


def test_import_stays_free_of_torch():
    code = ("import sys; from reinfocus_amd.environments import harness; "
            "harness.LstmSdePopulationPolicy; harness.DevicePopulationLstmSdePolicy; assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
