"""CPU tests of the recurrent PPO minibatch update's definition (include/reinfocus_hip.h, "lstm update"): the numpy twin
(lstm_learner.lstm_update_numpy) against the host build of the kernels' own header (tests/lstmppocheck) as bytes, on the
networks and sequence layouts of the GPU tests (the limit layouts among them: sequences of exactly 8, of 16, 17, 68 and 100
rows, 1024 one-row sequences, what each promises asserted against a plain restatement of the rule); against torch's autograd through torch.nn.LSTM, clip_grad_norm_ and Adam on
the CPU; the sequence rule against a plain restatement; the loss and skip cases; the numpy LstmLearner; the binding.

The autograd comparison of a development run (printed by the test; profiles/lstm_update.md records it):
    (4, 16, relu):    grad twin 1.89e-08 / torch 1.27e-08; after 1 update 5.84e-08 / 5.84e-08; after 10 updates 2.53e-07 / 2.53e-07
    (7, 65, tanh):    grad twin 4.20e-08 / torch 3.26e-08; after 1 update 5.95e-08 / 5.95e-08; after 10 updates 2.63e-07 / 2.63e-07
    (4, 16, relu) on T = 128, n = 8, B = 128 (sequences of 22, 1, 9, 68 and 28 rows):
                      grad twin 1.71e-08 / torch 9.61e-09; after 1 update 5.85e-08 / 5.85e-08; after 10 updates 3.60e-07 / 3.60e-07
"""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, learner, lstm_learner
from tests import lstm_io_cases as lstm_cases
from tests import lstm_learner_io_cases as cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits


@pytest.fixture(scope="module")
def hostcheck():
    return cases.hostcheck()


def host_update(lib, spec, params, state, batch, starts, states, n_steps, num_envs, first, count, hyper):
    """lpc_update on copies: (params, state, stats, the packed gradient before clipping)."""
    params, state = params.copy(), state.copy()
    stats, grad = np.zeros(8, dtype=F32), np.zeros(spec.size, dtype=F32)
    arrays = [np.ascontiguousarray(batch[key]) for key in learner.BATCH_KEYS]
    starts, states = np.ascontiguousarray(starts, dtype=np.uint8), np.ascontiguousarray(states, dtype=F32)
    rc = lib.lpc_update(ctypes.byref(_native.LstmPolicyDesc(*spec.desc())), ctypes.byref(_native.PpoDesc(*hyper)),
                        params.ctypes.data, state.ctypes.data, n_steps, num_envs, *(a.ctypes.data for a in arrays),
                        starts.ctypes.data, states.ctypes.data, first, count, stats.ctypes.data, grad.ctypes.data)
    assert rc == 0
    return params, state, stats, grad


def twin_update(spec, params, state, batch, starts, states, n_steps, num_envs, first, count, hyper):
    grad = lstm_learner.lstm_gradient_numpy(spec, params, batch, starts, states, n_steps, num_envs, first, count, hyper)[0]
    return lstm_learner.lstm_update_numpy(spec, params, state, batch, starts, states, n_steps, num_envs, first, count,
                                          hyper) + (grad,)


def same(got, want, what):
    for name, x, y in zip(("params", "state", "stats", "gradient"), got, want):
        assert bits(x) == bits(y), f"{what}: {name} differ"


# ---- 1: the twin against the host build of rf_lstm_ppo.h --------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))
def test_update_of_the_header_equals_the_twin(index, hostcheck):
    """Three chained updates with changing hyper-parameters on every sequence layout of the GPU tests: parameters,
    optimizer state, stats and the gradient as bytes."""
    for name in cases.layouts_of(index):
        spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(index, name)
        want = cases.twin_updates(index, name)
        state = learner.fresh_state(spec)
        assert hostcheck.lpc_state_size(ctypes.byref(_native.LstmPolicyDesc(*spec.desc()))) == 4 * state.size
        for update in range(cases.UPDATES):
            got = host_update(hostcheck, spec, params, state, batch, starts, states, n_steps, num_envs, first, count,
                              cases.hyper_of(update))
            same(got, want[update], f"{name}, update {update}")
            params, state = got[0], got[1]
        assert learner.state_parts(spec, state)[0] == cases.UPDATES and np.isfinite(want[-1][2]).all()


LIMIT_CASES = [(index, name) for index in range(len(cases.NETWORKS)) for name in cases.limit_layouts_of(index)]


@pytest.mark.parametrize("index,name", LIMIT_CASES, ids=[f"{index}-{name}" for index, name in LIMIT_CASES])
def test_update_of_the_header_equals_the_twin_at_the_limits(index, name, hostcheck):
    """The same on the limit layouts (cases.LIMIT_LAYOUTS), one case each: sequences of exactly 8, of 16, 17 and more than
    64 rows, 1024 one-row sequences, minibatches past 512 rows.  The host build walks rows in plain loops; the tiles, the
    prefetch and the grids are the GPU test's."""
    spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(index, name)
    want = cases.twin_updates(index, name)
    state = learner.fresh_state(spec)
    for update in range(cases.UPDATES):
        got = host_update(hostcheck, spec, params, state, batch, starts, states, n_steps, num_envs, first, count,
                          cases.hyper_of(update))
        same(got, want[update], f"{name}, update {update}")
        params, state = got[0], got[1]
    assert learner.state_parts(spec, state)[0] == cases.UPDATES and np.isfinite(want[-1][2]).all()
    assert all(stats[7] == 0 for _, _, stats, _ in want) and n_steps * num_envs <= learner.MAX_BATCH


def lengths_of(name):
    """(sequence lengths, restated rows) of a layout's minibatch, by the restatement of the rule; the twin's
    sequence_rows and the header's agree with it."""
    n_steps, num_envs, kind, first, count = cases.LAYOUTS[name]
    starts = cases.starts_of(kind, n_steps, num_envs)
    rows = cases.restated_rows(starts, n_steps, num_envs, first, count)
    twin = lstm_learner.sequence_rows(starts, n_steps, num_envs, first, count)
    assert [(r, s, ("zero" if zero else ("stored", t, e)) if s else None) for r, e, t, s, zero in twin] == rows
    begins = [b for b, row in enumerate(rows) if row[1]]
    return [int(v) for v in np.diff(begins + [count])], rows


def test_limit_layouts_hold_what_they_promise(hostcheck):
    """tuned: every sequence has 8 rows, but a 5-row tail and a 3-row head at first 3, none enters from zero.  depth:
    sequences of 1, 8, 9, 16 and 17 rows, start bytes 1, 2 and 255, a wrap at first 5.  untuned: a sequence longer than 64
    rows and one of one row; the first minibatch is one whole environment entered from a stored non-zero state, the
    second crosses an environment boundary.  wave: 1024 one-row sequences from zero; 33 sequences without a flag."""
    assert lengths_of("tuned/0/8")[0] == [8] and lengths_of("tuned/3/8")[0] == [5, 3]
    lengths, rows = lengths_of("tuned/0/64")
    assert lengths == [8] * 8 and all(row[2] != "zero" for row in rows) and cases.TILE == 8
    lengths, rows = lengths_of("depth/0/65")
    assert lengths == [17, 1, 16, 8, 9, 14] and {1, 8, 9, 16, 17} <= set(lengths)
    assert [row[2] for row in rows if row[1]] == ["zero", ("stored", 0, 1), "zero", ("stored", 0, 2), "zero", ("stored", 0, 3)]
    lengths, rows = lengths_of("depth/5/68")
    assert lengths == [12, 1, 16, 8, 9, 16, 1, 5] and [row[0] for row in rows][62:64] == [67, 0] and rows[63][2] == "zero"
    assert lengths_of("depth/0/17")[0] == [17]
    starts = cases.starts_of("depth", 17, 4)
    assert sorted(starts[starts != 0]) == [1, 1, 2, 255] and (starts != 0).sum(axis=0).tolist() == [1, 1, 1, 1]
    lengths, rows = lengths_of("untuned/0/128")
    assert max(lengths) > 64 and 1 in lengths and sum(lengths) == 128
    assert rows[0] == (0, True, ("stored", 0, 0)) and all(row[0] < 128 for row in rows)
    states = cases.layout_inputs(cases.TUNED, "untuned/0/128")[4]
    assert np.abs(states[0, :, :, 0]).min() > 0
    lengths, rows = lengths_of("untuned/100/128")
    assert max(lengths) > 64 and [row[0] for row in rows][27:29] == [127, 128] and rows[28][1]
    starts = cases.starts_of("drawn", 128, 8)
    episodes = (starts[:128] != 0).sum(axis=0)
    assert episodes.min() >= 1 and episodes.max() <= 8 and {1, 2, 255} <= set(starts.reshape(-1).tolist())
    lengths, rows = lengths_of("wave/7/1024")
    assert lengths == [1] * 1024 and all(row[2] == "zero" for row in rows) and rows[-1][0] == 6
    assert lengths_of("wave/0/513")[0] == [16] * 32 + [1]
    for name in cases.LIMIT_LAYOUTS:  # (the header's rule, too)
        n_steps, num_envs, kind, first, count = cases.LAYOUTS[name]
        flat = np.ascontiguousarray(cases.starts_of(kind, n_steps, num_envs))
        row, start, end = (np.zeros(count, dtype=np.int32) for _ in range(3))
        hostcheck.lpc_sequences(flat.ctypes.data, n_steps, num_envs, first, count, row.ctypes.data, start.ctypes.data,
                                end.ctypes.data)
        want = lengths_of(name)[1]
        assert list(row) == [w[0] for w in want] and [bool(v) for v in start] == [w[1] for w in want], name
    norms = [stats[5] for _, _, stats, _ in cases.twin_updates(cases.TUNED, "wave/7/1024")]
    assert norms[1] < learner_schedule()[1][0] and norms[2] > learner_schedule()[2][0]


def test_layouts_hold_what_they_promise():
    """A ragged tile, a wrap, an environment boundary, a length-1 sequence, a sequence longer than a tile, a sequence of
    four rows that enters from a stored non-zero state; a norm that clips and one that does not."""
    spec, params, batch, starts, states, n_steps, num_envs, first, count = cases.layout_inputs(1, "mixed/7/15")
    rows = lstm_learner.sequence_rows(starts, n_steps, num_envs, first, count)
    assert [row[0] for row in rows] == list(range(7, 15)) + list(range(7))  # (a wrap)
    begins = [b for b, row in enumerate(rows) if row[3]]
    lengths = np.diff(begins + [count])
    assert 1 in lengths and any(rows[b][2] == 0 and not rows[b][4] for b in begins[1:])  # (an environment change inside)
    whole = lstm_learner.sequence_rows(starts, n_steps, num_envs, 0, 15)
    assert whole[5][3] and not whole[5][4] and not any(row[3] for row in whole[6:9])  # (env 1: four rows from a stored state)
    assert np.abs(states[0, :, :, 1]).min() > 0
    single = cases.layout_inputs(1, "single/0/9")
    rows = lstm_learner.sequence_rows(single[3], 9, 1, 0, 9)
    assert [row[3] for row in rows] == [True] + [False] * 8 and 9 > cases.TILE
    every = cases.layout_inputs(1, "every/3/15")
    assert all(row[3] and row[4] for row in lstm_learner.sequence_rows(every[3], 5, 3, 3, 15))
    norms = [stats[5] for _, _, stats, _ in cases.twin_updates(2, "mixed/0/15")]
    assert norms[1] < learner_schedule()[1][0] and norms[2] > learner_schedule()[2][0]


def learner_schedule():
    from tests import learner_io_cases

    return learner_io_cases.SCHEDULE


# ---- 2: the twin against torch's autograd through torch.nn.LSTM ------------------------------------------------------------
AUTOGRAD_STEPS, AUTOGRAD_ENVS, AUTOGRAD_FIRST = 8, 4, 5


def autograd_inputs(index, untuned=False):
    """A rollout of 8 steps of 4 environments taken as ONE minibatch of 32 rows rotated by 5 (so it wraps inside an
    environment); environment 1 runs all 8 rows from a stored non-zero state, the others start episodes inside.  The
    stored log-probabilities are the twin's own plus normal noise of scale 0.15.  untuned: the rollout of cases' untuned
    layouts instead (T = 128, n = 8, the drawn starts)."""
    spec = cases.spec_of(cases.NETWORKS[index])
    state = lstm_cases.state_dict(spec, 60 + index)
    params = spec.pack(state)
    n_steps, num_envs = (128, 8) if untuned else (AUTOGRAD_STEPS, AUTOGRAD_ENVS)
    total = n_steps * num_envs
    rng = np.random.default_rng(index)
    starts = np.zeros((n_steps + 1, num_envs), dtype=np.uint8)
    if untuned:
        starts = cases.starts_of("drawn", n_steps, num_envs)
    else:
        starts[0, 0], starts[3, 0], starts[5, 2], starts[0, 3], starts[6, 3] = 1, 1, 1, 1, 1
    states = (0.5 * rng.standard_normal((n_steps + 1,) + spec.state_shape(num_envs))).astype(F32)
    batch = {"observations": rng.standard_normal((total, spec.obs_width)).astype(F32),
             "actions": rng.integers(0, spec.n_actions, total).astype(np.int64),
             "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32)}
    own = cases.own_log_probs(spec, params, batch, starts, states, n_steps, num_envs)
    batch["log_probs"] = (own + 0.15 * rng.standard_normal(total)).astype(F32)
    return spec, state, params, batch, starts, states


@pytest.mark.parametrize("index", [1, 3])
def test_gradient_and_updates_are_no_further_from_float64_than_four_times_torch(index, tmp_path, hostcheck):
    """The twin's gradient before clipping, its parameters after the first update of a fresh optimizer and after 10
    updates on one minibatch, each against the same from torch in float64 (torch.nn.LSTM cells stepped per row with the
    definition's sequence rule and select, the stored states detached; stable-baselines3's loss, autograd,
    clip_grad_norm_, Adam(eps=1e-5)): the largest distance may be at most 4 x that of torch's own float32 run on the same
    inputs -- the rule and the factor of tests/test_learner_logic.py.  And back-propagation through time is there: with
    the gradient through h_prev / c_prev cut, torch's float64 gradient of weight_hh_l0 of either net moves by more than
    that bound, so an update truncated to one step cannot pass.  Both distances are printed."""
    held_to_float64(index, False, AUTOGRAD_STEPS, AUTOGRAD_ENVS, AUTOGRAD_FIRST, AUTOGRAD_STEPS * AUTOGRAD_ENVS, 4, tmp_path,
                    hostcheck)


def test_the_same_rule_through_sequences_longer_than_64_rows(tmp_path, hostcheck):
    """The rule above with the same factor on the untuned layout (T = 128, n = 8, B = 128 from row 0: ppo_lstm_untuned.yml's
    shape) on ppo_lstm_tuned.yml's network (H = 16): back-propagation through sequences of 22 rows (entered from a stored
    non-zero state), 1, 9, 68 and 28 rows, against torch's float64 run; cutting the recurrence still moves torch's float64
    gradient of weight_hh_l0 by more than the bound.  Both distances are printed (profiles/lstm_update.md records a run)."""
    held_to_float64(cases.TUNED, True, 128, 8, 0, 128, 65, tmp_path, hostcheck)


def held_to_float64(index, untuned, n_steps, num_envs, first, count, longest, tmp_path, hostcheck):
    """longest: some sequence must have at least that many rows."""
    spec, state, params, batch, starts, states = autograd_inputs(index, untuned)
    rows = lstm_learner.sequence_rows(starts, n_steps, num_envs, first, count)
    begins = [b for b, row in enumerate(rows) if row[3]]
    lengths = np.diff(begins + [count])
    print(f"{cases.NETWORKS[index]}: sequence lengths {list(lengths)}")
    assert any(length >= 4 and not rows[b][4] and np.abs(states[rows[b][2], :, :, rows[b][1]]).min() > 0
               for b, length in zip(begins, lengths)), "no sequence of 4 rows enters from a non-zero state"
    assert max(lengths) >= longest, f"no sequence has {longest} rows"
    hyper = learner.Hyper(3e-4, 0.2, 0.01, 0.5, 0.5, 0.9, 0.999, 1e-5, 1)
    updates = 10
    np.savez(tmp_path / "in.npz", names=np.array(spec.keys()), activation=spec.activation, obs=batch["observations"],
             actions=batch["actions"], old_log_probs=batch["log_probs"], advantages=batch["advantages"],
             returns=batch["returns"], lstm_states=states, row=np.array([row[0] for row in rows], dtype=np.int64),
             env=np.array([row[1] for row in rows], dtype=np.int64), step=np.array([row[2] for row in rows], dtype=np.int64),
             is_start=np.array([row[3] for row in rows]), zero=np.array([row[4] for row in rows]),
             clip_range=hyper.clip_range, ent_coef=hyper.ent_coef, vf_coef=hyper.vf_coef,
             max_grad_norm=hyper.max_grad_norm, learning_rate=hyper.learning_rate, updates=updates, **state)
    subprocess.run([sys.executable, "-m", "tests.lstm_learner_io_cases", "--torch-lstm-learner", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=600)
    theirs = np.load(tmp_path / "out.npz")
    grad, terms, invalid = lstm_learner.lstm_gradient_numpy(spec, params, batch, starts, states, n_steps, num_envs, first,
                                                            count, hyper)
    share = terms[4].mean()
    print(f"{cases.NETWORKS[index]}: share of ratios outside the clip range {share:.3f}")
    assert not invalid and 0.05 <= share <= 0.5 and abs(share - float(theirs["clip_fraction64"])) <= 2 / count
    ours = {"grad": grad}
    optimizer = learner.fresh_state(spec)
    for update in range(updates):
        params, optimizer, stats = lstm_learner.lstm_update_numpy(spec, params, optimizer, batch, starts, states, n_steps,
                                                                  num_envs, first, count, hyper)
        assert stats[7] == 0
        if update == 0:
            ours["first"] = params
    ours["last"] = params
    assert bits(host_update(hostcheck, spec, spec.pack(state), learner.fresh_state(spec), batch, starts, states, n_steps,
                            num_envs, first, count, hyper)[3]) == bits(grad)
    bound, distances = None, []
    for kind in ("grad", "first", "last"):
        exact = theirs[kind + "64"]
        assert theirs[kind + "32"].dtype == F32 and exact.dtype == np.float64
        twin = np.abs(ours[kind].astype(np.float64) - exact).max()
        torch = np.abs(theirs[kind + "32"].astype(np.float64) - exact).max()
        print(f"{cases.NETWORKS[index]}, {count} rows: {kind}: twin {twin:.3e}, torch {torch:.3e}, ratio {twin / torch:.2f}")
        distances.append((kind, twin, torch))
        if kind == "grad":
            bound = 4.0 * torch
    for kind, twin, torch in distances:  # (after all three were printed)
        assert twin <= 4.0 * torch, (kind, twin, torch)
    for name, at, shape, _ in spec.entries:
        if name.endswith("weight_hh_l0"):
            size = int(np.prod(shape))
            moved = np.abs(theirs["grad_cut64"][at:at + size] - theirs["grad64"][at:at + size]).max()
            print(f"{cases.NETWORKS[index]}: {name}: cutting the recurrence moves the float64 gradient by {moved:.3e}, "
                  f"the bound is {bound:.3e}")
            assert moved > bound, (name, moved, bound)


# ---- 3: the sequence rule ------------------------------------------------------------------------------------------------------
def rule_inputs(starts, nan_env=None, seed=5):
    spec = cases.spec_of(cases.NETWORKS[1])
    _, params, batch, _, states = cases.update_inputs(1, cases.STEPS, cases.ENVS, "mixed")
    states = states.copy()
    if nan_env is not None:
        states[:, :, :, nan_env, :] = np.nan
    return spec, params, batch, np.asarray(starts, dtype=np.uint8), states


def check_rule(hostcheck, starts, first, count):
    """sequence_rows and the header's functions against the restatement; returns the restatement."""
    n_steps, num_envs = cases.STEPS, cases.ENVS
    want = cases.restated_rows(starts, n_steps, num_envs, first, count)
    rows = lstm_learner.sequence_rows(starts, n_steps, num_envs, first, count)
    got = [(r, is_start, ("zero" if zero else ("stored", t, e)) if is_start else None) for r, e, t, is_start, zero in rows]
    assert got == want
    flat = np.ascontiguousarray(starts, dtype=np.uint8)
    row, start, end = (np.zeros(count, dtype=np.int32) for _ in range(3))
    hostcheck.lpc_sequences(flat.ctypes.data, n_steps, num_envs, first, count, row.ctypes.data, start.ctypes.data,
                            end.ctypes.data)
    assert list(row) == [w[0] for w in want] and [bool(s) for s in start] == [w[1] for w in want]
    begins = [b for b, w in enumerate(want) if w[1]]
    assert [int(end[b]) for b in begins] == begins[1:] + [count]
    return want


@pytest.mark.parametrize("first,count", [(0, 15), (7, 15), (3, 2)])
def test_sequence_rule_on_the_mixed_layout(first, count, hostcheck):
    starts = cases.starts_of("mixed", cases.STEPS, cases.ENVS)
    want = check_rule(hostcheck, starts, first, count)
    if (first, count) == (7, 15):
        assert [w[0] for w in want][7:9] == [14, 0] and want[0] == (7, True, ("stored", 2, 1))
        assert want[3] == (10, True, "zero") and want[8] == (0, True, "zero")  # (an environment change, and the wrap)
    if (first, count) == (3, 2):  # no start but b == 0: the entering state is the stored one
        assert want == [(3, True, ("stored", 3, 0)), (4, False, None)]
        spec, params, batch, starts, states = rule_inputs(starts)
        state = learner.fresh_state(spec)
        base = twin_update(spec, params, state, batch, starts, states, 5, 3, 3, 2, cases.hyper_of(0))
        moved = states.copy()
        moved[3, :, :, 0, :] += F32(0.25)
        other = twin_update(spec, params, state, batch, starts, moved, 5, 3, 3, 2, cases.hyper_of(0))
        assert bits(base[3]) != bits(other[3])  # (the stored state of (t = 3, e = 0) enters)
        same(host_update(hostcheck, spec, params, state, batch, starts, moved, 5, 3, 3, 2, cases.hyper_of(0)), other, "b == 0")


def test_every_row_a_start_and_none_but_row_zero(hostcheck):
    every = np.ones((cases.STEPS + 1, cases.ENVS), dtype=np.uint8)
    want = check_rule(hostcheck, every, 4, 15)
    assert all(w[1] and w[2] == "zero" for w in want)
    none = np.zeros((cases.STEPS + 1, cases.ENVS), dtype=np.uint8)
    none[0, 0] = 1
    want = check_rule(hostcheck, none, 0, 15)
    assert [b for b, w in enumerate(want) if w[1]] == [0, 5, 10]  # (t == 0 still starts a sequence: the environment changes)
    assert want[0][2] == "zero" and want[5][2] == ("stored", 0, 1)
    # with every row a start the stored states never enter
    spec, params, batch, _, states = rule_inputs(every)
    state = learner.fresh_state(spec)
    base = twin_update(spec, params, state, batch, every, states, 5, 3, 4, 15, cases.hyper_of(0))
    other = twin_update(spec, params, state, batch, every, np.full_like(states, np.nan), 5, 3, 4, 15, cases.hyper_of(0))
    same(other, base, "every row a start")
    assert base[2][7] == 0


def test_start_bytes_2_and_255_are_starts(hostcheck):
    ones = cases.starts_of("mixed", cases.STEPS, cases.ENVS)
    assert 2 in ones and 255 in ones
    plain = (ones != 0).astype(np.uint8)
    spec, params, batch, _, states = rule_inputs(ones)
    state = learner.fresh_state(spec)
    a = twin_update(spec, params, state, batch, ones, states, 5, 3, 0, 15, cases.hyper_of(0))
    b = twin_update(spec, params, state, batch, plain, states, 5, 3, 0, 15, cases.hyper_of(0))
    same(a, b, "bytes 2 and 255")
    same(host_update(hostcheck, spec, params, state, batch, ones, states, 5, 3, 0, 15, cases.hyper_of(0)), a, "the host build")
    assert check_rule(hostcheck, ones, 0, 15) == cases.restated_rows(plain, 5, 3, 0, 15)


def test_a_nan_state_behind_a_start_never_enters_and_one_without_does(hostcheck):
    """Environment 0's stored states are NaN throughout and its rows start episodes at t = 0 and t = 2: the result is
    finite and equals the one from zero states.  Environment 1's are NaN and row t = 0 has no start byte: the update is
    skipped (RF_PPO_NONFINITE) and nothing changes."""
    starts = cases.starts_of("mixed", cases.STEPS, cases.ENVS)
    spec, params, batch, starts, dead = rule_inputs(starts, nan_env=0)
    _, _, _, _, clean = rule_inputs(starts)
    zeroed = clean.copy()
    zeroed[:, :, :, 0, :] = 0.0
    state = cases.twin_updates(1, "mixed/0/15")[0][1]
    got = twin_update(spec, params, state, batch, starts, dead, 5, 3, 0, 15, cases.hyper_of(1))
    want = twin_update(spec, params, state, batch, starts, zeroed, 5, 3, 0, 15, cases.hyper_of(1))
    same(got, want, "a NaN state behind a start")
    assert got[2][7] == 0 and np.isfinite(got[0]).all() and np.isfinite(got[3]).all() and bits(got[0]) != bits(params)
    same(host_update(hostcheck, spec, params, state, batch, starts, dead, 5, 3, 0, 15, cases.hyper_of(1)), got, "the host")
    _, _, _, _, live = rule_inputs(starts, nan_env=1)
    skipped = twin_update(spec, params, state, batch, starts, live, 5, 3, 0, 15, cases.hyper_of(1))
    assert skipped[2][7] == learner.NONFINITE
    assert bits(skipped[0]) == bits(params) and bits(skipped[1]) == bits(state)
    same(host_update(hostcheck, spec, params, state, batch, starts, live, 5, 3, 0, 15, cases.hyper_of(1)), skipped, "the host")


# ---- 4: loss and skip cases ---------------------------------------------------------------------------------------------------------
def test_equal_advantages_a_single_row_and_an_action_out_of_range(hostcheck):
    spec, params, batch, starts, states, n_steps, num_envs, _, _ = cases.layout_inputs(1, "mixed/0/15")
    state = cases.twin_updates(1, "mixed/0/15")[0][1]
    args = (starts, states, n_steps, num_envs)
    flat = dict(batch, advantages=np.full(15, 0.7, dtype=F32))
    hyper = cases.hyper_of(0, ent_coef=0.0, vf_coef=0.0)
    fresh = learner.fresh_state(spec)  # (m = 0: a zero gradient then moves nothing)
    got = twin_update(spec, params, fresh, flat, *args, 3, 9, hyper)
    assert got[2][0] == 0 and got[2][5] == 0 and got[2][7] == 0 and bits(got[0]) == bits(params)
    assert learner.state_parts(spec, got[1])[0] == 1
    same(host_update(hostcheck, spec, params, fresh, flat, *args, 3, 9, hyper), got, "equal advantages")
    one = twin_update(spec, params, state, batch, *args, 6, 1, cases.hyper_of(0))
    raw = twin_update(spec, params, state, batch, *args, 6, 1, cases.hyper_of(0, normalize_advantage=0))
    same(one, raw, "B = 1")
    same(host_update(hostcheck, spec, params, state, batch, *args, 6, 1, cases.hyper_of(0)), one, "B = 1")
    for bad, row in ((spec.n_actions, 4), (-1, 12)):
        wrong = dict(batch, actions=batch["actions"].copy())
        wrong["actions"][row] = bad
        skipped = twin_update(spec, params, state, wrong, *args, 3, 12, cases.hyper_of(1))
        assert skipped[2][7] == learner.INVALID, bad
        assert bits(skipped[0]) == bits(params) and bits(skipped[1]) == bits(state), bad
        assert (skipped[2][:7].view(np.uint32) != 0x7FC00000).sum() >= 3  # (the loss entries are still written)
        same(host_update(hostcheck, spec, params, state, wrong, *args, 3, 12, cases.hyper_of(1)), skipped, "an invalid action")
        taken = twin_update(spec, params, state, wrong, *args, 5, 7, cases.hyper_of(1))  # (rows 5 .. 11: the bad one is outside)
        assert taken[2][7] == 0
    infinite = dict(batch, returns=np.full(15, np.inf, dtype=F32))
    skipped = twin_update(spec, params, state, infinite, *args, 0, 15, cases.hyper_of(1))
    assert skipped[2][7] == learner.NONFINITE and bits(skipped[0]) == bits(params) and bits(skipped[1]) == bits(state)
    same(host_update(hostcheck, spec, params, state, infinite, *args, 0, 15, cases.hyper_of(1)), skipped, "infinite returns")


def test_first_and_count_outside_their_limits_raise_before_anything_happens():
    spec, params, batch, starts, states, n_steps, num_envs, _, _ = cases.layout_inputs(0, "mixed/0/15")
    state = learner.fresh_state(spec)
    for first, count in ((0, 0), (0, 16), (-1, 4), (15, 4), (0, -3)):
        with pytest.raises(ValueError):
            lstm_learner.lstm_update_numpy(spec, params, state, batch, starts, states, n_steps, num_envs, first, count,
                                           cases.hyper_of(0))
        with pytest.raises(ValueError):
            lstm_learner.sequence_rows(starts, n_steps, num_envs, first, count)
    wide = lstm_learner.sequence_rows(np.zeros((1025, 2), dtype=np.uint8), 1024, 2, 0, 1024)
    assert len(wide) == 1024
    with pytest.raises(ValueError):
        lstm_learner.sequence_rows(np.zeros((1025, 2), dtype=np.uint8), 1024, 2, 0, 1025)  # (RF_PPO_MAX_BATCH)


# ---- 5: the surface and the binding ---------------------------------------------------------------------------------------------
def test_import_stays_free_of_torch():
    code = ("import sys; from reinfocus_amd.environments import harness, lstm_learner; harness.LstmLearner; "
            "harness.DeviceLstmLearner; harness.lstm_update_numpy; harness.lstm_gradient_numpy; "
            "assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def test_binding_matches_the_header():
    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    for entry, count in (("rf_lstm_ppo_update", 19), ("rf_lstm_ppo_state_size", 2), ("rf_lstm_ppo_workspace_size", 3)):
        declaration = re.search(r"\b%s\s*\((.*?)\)\s*;" % entry, text, flags=re.S).group(1)
        wanted = [ctypes.c_void_p if "*" in p else ctypes.c_int for p in declaration.split(",")]
        names = re.search(r"lib\.%s\.argtypes = \[(.*?)\]" % entry, source).group(1).split(",")
        assert [{"vp": ctypes.c_void_p, "i32": ctypes.c_int}[name.strip()] for name in names] == wanted
        assert len(wanted) == count and entry in _native.SYMBOLS
        assert re.search(r"lib\.%s\.restype = ctypes\.c_ulonglong" % entry, source) or entry == "rf_lstm_ppo_update"
    abi = open(os.path.join(ROOT, "reinfocus_amd", "csrc", "rf_abi_env.hip")).read()
    for entry in ("rf_lstm_ppo_update", "rf_lstm_ppo_state_size", "rf_lstm_ppo_workspace_size"):
        assert re.search(r"\n(int|unsigned long long) %s\(rf_ctx \*ctx," % entry, abi), entry
    assert lstm_learner.MAX_BATCH == learner.MAX_BATCH and lstm_learner.PART_KEYS[:5] == learner.BATCH_KEYS


def test_workspace_grows_with_the_batch_and_with_the_hidden_size(hostcheck):
    def size(network, count):
        return hostcheck.lpc_workspace_size(ctypes.byref(_native.LstmPolicyDesc(*cases.spec_of(network).desc())), count)

    sizes = [size(cases.NETWORKS[cases.LIMITS], count) for count in (1, 64, 65, 1024)]
    assert sizes == sorted(set(sizes)) and sizes[0] > 0 and all(s % 8 == 0 for s in sizes)
    assert size(cases.NETWORKS[cases.LIMITS], 0) == 0 and size(cases.NETWORKS[cases.LIMITS], 1025) == 0
    by_hidden = [size((4, hidden, (64, 64), (64, 64), 13, "tanh"), 128) for hidden in (1, 16, 64, 256)]
    assert by_hidden == sorted(set(by_hidden))
    bad = list(cases.spec_of(cases.NETWORKS[1]).desc())
    bad[9] = 257
    assert hostcheck.lpc_workspace_size(ctypes.byref(_native.LstmPolicyDesc(*bad)), 8) == 0


@pytest.mark.parametrize("n", cases.E2E_SIZES)
def test_train_with_splits_equals_the_explicit_loop_of_updates(n, no_gpu):  # noqa: F811
    """collect + train twice over the numpy twins (ppo_lstm_tuned.yml's network): 2 epochs of minibatches of 4 rows from
    given split indices equal the explicit loop of update() calls; the parameters move, every update is taken, and the
    second rollout differs from one collected with the first parameters."""
    kind = "view"
    runs = cases.twin_train_runs(kind, n)
    total = cases.T * n
    per_epoch = -(-total // cases.E2E_BATCH)
    assert runs[0]["stats/0"].shape == (cases.E2E_EPOCHS * per_epoch, 8) and (runs[1]["stats/0"][:, 7] == 0).all()
    assert bits(runs[0]["params"]) != bits(runs[1]["params"])
    unchanged = lstm_cases.twin_runs(kind, n)[0]
    assert bits(unchanged[0]["log_probs"]) == bits(runs[0]["log_probs"])
    assert bits(unchanged[1]["log_probs"]) != bits(runs[1]["log_probs"])  # (the updated parameters were used)
    # the explicit loop, on the first rollout
    env = lstm_cases.make_env(kind, n, False)
    try:
        spec = lstm_cases.e2e_spec(kind)
        twin = harness.LstmPolicy(spec, lstm_cases.SEED, num_envs=n)
        twin.load_state_dict(lstm_cases.state_dict(spec, 3))
        rollout = harness.Rollout(env, cases.T, cases.GAMMA, cases.GAE_LAMBDA)
        rollout.start(env.reset()[0])
        rollout.collect(twin)
        explicit = harness.LstmLearner(twin, **cases.LEARNER_KW)
        stats = []
        for split in cases.e2e_splits(0, total):
            for i in range(per_epoch):
                stats.append(explicit.update(rollout, (split + i * cases.E2E_BATCH) % total,
                                             min(cases.E2E_BATCH, total - i * cases.E2E_BATCH)))
        assert bits(np.stack(stats)) == bits(runs[0]["stats/0"])
        assert bits(twin.params) == bits(runs[0]["params"]) and bits(explicit.state) == bits(runs[0]["state"])
    finally:
        env.close()


def test_learner_surface(no_gpu):  # noqa: F811
    from tests import policy_io_cases as policy_cases

    spec = lstm_cases.e2e_spec("view")
    twin = harness.LstmPolicy(spec, 0, num_envs=2)
    twin.load_state_dict(lstm_cases.state_dict(spec, 3))
    with pytest.raises(TypeError, match="LstmPolicy"):
        harness.LstmLearner(spec)
    with pytest.raises(TypeError, match="DeviceLstmPolicy"):
        harness.DeviceLstmLearner(twin)
    with pytest.raises(TypeError, match="LstmPolicy"):
        harness.LstmLearner(harness.Policy(policy_cases.e2e_spec("plain"), 0))
    with pytest.raises(ValueError, match="betas"):
        harness.LstmLearner(twin, betas=(0.9, 1.0))
    env = lstm_cases.make_env("view", 2, False)
    plain = policy_cases.make_env("plain", 2, False)
    try:
        first = harness.LstmLearner(twin, learning_rate=1e-2)
        other = harness.Rollout(plain, cases.T, cases.GAMMA, cases.GAE_LAMBDA)
        other.start(plain.reset()[0])
        feedforward = harness.Policy(policy_cases.e2e_spec("plain"), 0)
        other.collect(feedforward)
        with pytest.raises(ValueError, match="not collected with a recurrent policy"):
            first.train(other, 1, 4)
        rollout = harness.Rollout(env, cases.T, cases.GAMMA, cases.GAE_LAMBDA)
        rollout.start(env.reset()[0])
        rollout.collect(twin)
        for bad in (dict(n_epochs=0, batch_size=4), dict(n_epochs=1, batch_size=1025), dict(n_epochs=2, batch_size=4, splits=[1]),
                    dict(n_epochs=1, batch_size=4, splits=[14])):
            with pytest.raises(ValueError):
                first.train(rollout, **bad)
        first.train(rollout, 1, 8, generator=np.random.default_rng(1))
        kept, kept_params = first.state_dict(), twin.params.copy()
        assert kept["step"] == 2 and kept["bc1"] == 1.0 - 0.9 * (1.0 - (1.0 - 0.9))
        straight = first.train(rollout, 1, 8, generator=np.random.default_rng(2))
        want = twin.params.copy(), first.state.copy()
        twin.params[:] = kept_params
        second = harness.LstmLearner(twin, learning_rate=1e-2)
        second.load_state_dict(kept)
        assert bits(second.train(rollout, 1, 8, generator=np.random.default_rng(2))) == bits(straight)
        assert bits(twin.params) == bits(want[0]) and bits(second.state) == bits(want[1])
    finally:
        env.close()
        plain.close()
