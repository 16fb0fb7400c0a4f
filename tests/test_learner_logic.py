"""CPU tests of the PPO minibatch update's definition (include/reinfocus_hip.h, "ppo update"): the numpy twin
(learner.ppo_update_numpy) against the host build of the kernels' own header (tests/ppocheck) as bytes, on the networks
and batches of the GPU tests (512, 513, 1000 and 1024 rows among them: RF_PPO_MAX_BATCH and the sizes around the second
trip of the kernels' reductions); against torch's autograd, clip_grad_norm_ and Adam on the CPU; the subgradient at the clip
bounds; the skip rules; the numpy Learner; the binding."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, learner, policy
from tests import helpers
from tests import learner_io_cases as cases
from tests import policy_io_cases as policy_cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits


@pytest.fixture(scope="module")
def ppocheck():
    lib = ctypes.CDLL(helpers.built("tests/ppocheck", "libppocheck.so"))
    vp = ctypes.c_void_p
    lib.ppc_state_size.restype = lib.ppc_workspace_size.restype = ctypes.c_ulonglong
    lib.ppc_state_size.argtypes = [vp]
    lib.ppc_workspace_size.argtypes = [vp, ctypes.c_int]
    lib.ppc_update.argtypes = [vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_int, vp, vp, vp]
    return lib


def host_update(lib, spec, params, state, batch, index, hyper, gradient=False):
    """ppc_update on copies: (params, state, stats[, the packed gradient before clipping])."""
    params, state = params.copy(), state.copy()
    stats, grad = np.zeros(8, dtype=F32), np.zeros(spec.size, dtype=F32)
    arrays = [np.ascontiguousarray(batch[key]) for key in learner.BATCH_KEYS]
    index = np.ascontiguousarray(index, dtype=np.int64)
    rc = lib.ppc_update(ctypes.byref(_native.PolicyDesc(*spec.desc())), ctypes.byref(_native.PpoDesc(*hyper)),
                        params.ctypes.data, state.ctypes.data, arrays[1].shape[0], *(a.ctypes.data for a in arrays),
                        index.size, index.ctypes.data, stats.ctypes.data, grad.ctypes.data)
    assert rc == 0
    return (params, state, stats, grad) if gradient else (params, state, stats)


def same(got, want, what):
    for name, x, y in zip(("params", "state", "stats"), got, want):
        assert bits(x) == bits(y), f"{what}: {name} differ"


# ---- 1: the twin against the host build of rf_ppo.h ------------------------------------------------------------------------
@pytest.mark.parametrize("count", cases.BATCHES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))
def test_update_of_the_header_equals_the_twin(index, count, ppocheck):
    spec, params, batch, indices = cases.update_inputs(index, count)
    want = cases.twin_updates(index, count)
    state = learner.fresh_state(spec)
    assert ppocheck.ppc_state_size(ctypes.byref(_native.PolicyDesc(*spec.desc()))) == 4 * state.size
    for update in range(cases.UPDATES):
        params, state, stats = host_update(ppocheck, spec, params, state, batch, indices[update], cases.hyper_of(update))
        same((params, state, stats), want[update], f"update {update}")
    assert learner.state_parts(spec, state)[0] == cases.UPDATES and np.isfinite(want[-1][2]).all()


@pytest.mark.parametrize("index,count", cases.LIMIT_CASES,
                         ids=lambda v: "-".join(str(x) for x in cases.NETWORKS[v]) if v < len(cases.NETWORKS) else str(v))
def test_update_of_the_header_equals_the_twin_at_the_batch_limits(index, count, ppocheck):
    """512, 513, 1000 and 1024 rows (cases.LIMIT_BATCHES): the host build walks the rows in plain loops, so what it holds
    here is the twin's own order of summation over more than 512 rows; the kernels' tiles and reduction trips are the GPU
    test's.  The hostile inputs are those of the small batches: the index still repeats a row and holds the last one, and
    the schedule still clips once and once not -- but for the least network at 1024 rows, whose one-unit gradient, a mean
    over 1024 rows, has a norm of 0.03: no update of that one case is clipped."""
    test_update_of_the_header_equals_the_twin(index, count, ppocheck)
    spec, params, batch, indices = cases.update_inputs(index, count)
    assert batch["actions"].shape[0] == count + 3 and all(chosen.size == count for chosen in indices)
    assert indices[0][-1] == indices[0][0] and any(count + 2 in chosen for chosen in indices)
    norms = [stats[5] for _, _, stats in cases.twin_updates(index, count)]
    assert norms[1] < cases.SCHEDULE[1][0] and (norms[2] > cases.SCHEDULE[2][0]) == ((index, count) != (0, 1024))


def test_hostile_minibatches_hold_what_they_promise():
    """Ties and e_i == 0 among the logits, ratios inside the range, past both bounds and at d > 0, a repeated index, a
    norm that clips and one that does not, +-0 and subnormal observations."""
    spec, params, batch, indices = cases.update_inputs(2, 64)
    logits = policy._net(spec, spec.nets(params)[0], batch["observations"])
    assert (logits[:, 0] == logits[:, 1]).all() and (policy.exp32(logits[:, -1] - logits.max(axis=1)) == 0).all()
    d = policy.log_softmax(logits)[np.arange(67), batch["actions"]] - batch["log_probs"]
    assert (d > 0.25).any() and (d < -0.25).any() and (np.abs(d) < 0.1).any()
    assert len(set(indices[0])) == 63 and indices[0][-1] == indices[0][0]
    obs = batch["observations"]
    assert (np.signbit(obs) & (obs == 0)).any() and ((obs != 0) & (np.abs(obs) < 1e-38)).any()
    norms = [stats[5] for _, _, stats in cases.twin_updates(2, 64)]
    assert norms[1] < cases.SCHEDULE[1][0] and norms[2] > cases.SCHEDULE[2][0]
    assert cases.twin_updates(2, 64)[0][2][4] > 0  # (some ratios were clipped)


# ---- 2: the twin against torch's autograd, clip_grad_norm_ and Adam ----------------------------------------------------------
def autograd_inputs(index, rows=64):
    """A minibatch of 64 (or `rows`) normal rows; the stored log-probabilities come from a copy of the parameters whose action head
    is perturbed, scaled (the first of a fixed list) so that about a quarter of the ratios leave the clip range."""
    spec = cases.spec_of(policy_cases.NETWORKS[index])
    state = policy_cases.state_dict(spec, 60 + index)
    rng = np.random.default_rng(index)
    obs = rng.standard_normal((rows, spec.obs_width)).astype(F32)
    actions = rng.integers(0, spec.n_actions, rows).astype(np.int64)
    noise = rng.standard_normal(state["action_net.weight"].shape).astype(F32)
    params = spec.pack(state)
    new = policy.log_softmax(policy._net(spec, spec.nets(params)[0], obs))[np.arange(rows), actions]
    for scale in (0.005, 0.01, 0.02, 0.03, 0.04, 0.06, 0.08, 0.12, 0.2):
        moved = dict(state)
        moved["action_net.weight"] = state["action_net.weight"] + F32(scale) * noise
        old = policy.log_softmax(policy._net(spec, spec.nets(spec.pack(moved))[0], obs))[np.arange(rows), actions]
        share = np.mean(np.abs(np.exp((new - old).astype(np.float64)) - 1) > 0.2)
        if share >= 0.2:
            break
    batch = {"observations": obs, "actions": actions, "log_probs": old, "advantages": rng.standard_normal(rows).astype(F32),
             "returns": rng.standard_normal(rows).astype(F32)}
    return spec, state, params, batch, share


@pytest.mark.parametrize("index", [1, 2])
def test_gradient_and_updates_are_no_further_from_float64_than_four_times_torch(index, tmp_path, ppocheck):
    """The twin's gradient before clipping, its parameters after the first update of a fresh (all-zero) optimizer and
    after 10 updates on one minibatch, each against the same from torch in float64 (stable-baselines3's loss, autograd,
    clip_grad_norm_, Adam(eps=1e-5)): the largest distance may be at most 4 x that of torch's own float32 run on the same
    inputs.  Both distances are printed (profiles/learner.md records a run); torch runs in a process of its own."""
    held_to_float64(index, 64, tmp_path, ppocheck)


@pytest.mark.xfail(strict=True, reason="the gradient's ratio is 6.99 at 1024 rows (twin 8.88e-08, torch 1.27e-08): the "
                                       "definition sums the batch in order, torch's float32 error shrinks with the batch")
def test_the_same_rule_at_1024_rows_on_the_default_network(tmp_path, ppocheck):
    """The rule above with the same factor at B = RF_PPO_MAX_BATCH = 1024 on stable-baselines3's 64-64 network: the
    definition's order of summation over 1024 rows (its float32 sums over the batch among them) against float64.  Both
    distances are printed (profiles/learner.md records a run).

    A finding, not yet a pass: the twin's gradient is as far from float64 as at 64 rows (8.88e-08 there, 8.88e-08 here)
    while torch's own float32 gradient comes three times closer (4.02e-08 at 64 rows, 1.27e-08 here), so the ratio is 6.99
    and the factor 4 is missed; after the first update the ratio is 1.40 and after ten 1.00.  The definition's summation
    order is what a later change would have to touch; this test then passes and the mark goes."""
    held_to_float64(1, 1024, tmp_path, ppocheck)


def held_to_float64(index, rows, tmp_path, ppocheck):
    spec, state, params, batch, share = autograd_inputs(index, rows)
    print(f"{policy_cases.NETWORKS[index]}: share of ratios outside the clip range {share:.3f}")
    assert 0.10 <= share <= 0.40
    hyper = learner.Hyper(3e-4, 0.2, 0.01, 0.5, 0.5, 0.9, 0.999, 1e-5, 1)
    updates = 10
    np.savez(tmp_path / "in.npz", names=np.array(spec.keys()), activation=spec.activation, obs=batch["observations"],
             actions=batch["actions"], old_log_probs=batch["log_probs"], advantages=batch["advantages"],
             returns=batch["returns"], clip_range=hyper.clip_range, ent_coef=hyper.ent_coef, vf_coef=hyper.vf_coef,
             max_grad_norm=hyper.max_grad_norm, learning_rate=hyper.learning_rate, updates=updates, **state)
    subprocess.run([sys.executable, "-m", "tests.learner_io_cases", "--torch-learner", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=300)
    theirs = np.load(tmp_path / "out.npz")
    every = np.arange(rows)
    grad, terms, invalid = learner.ppo_gradient_numpy(spec, params, batch, every, hyper)
    assert not invalid and abs(terms[4].mean() - float(theirs["clip_fraction64"])) <= 2 / rows
    ours = {"grad": grad}
    optimizer = learner.fresh_state(spec)
    for update in range(updates):
        params, optimizer, stats = learner.ppo_update_numpy(spec, params, optimizer, batch, every, hyper)
        assert stats[7] == 0
        if update == 0:
            ours["first"] = params
    ours["last"] = params
    assert bits(host_update(ppocheck, spec, spec.pack(state), learner.fresh_state(spec), batch, every, hyper, True)[3]) \
        == bits(grad)
    distances = []
    for kind in ("grad", "first", "last"):
        exact = theirs[kind + "64"]
        assert theirs[kind + "32"].dtype == F32 and exact.dtype == np.float64
        twin = np.abs(ours[kind].astype(np.float64) - exact).max()
        torch = np.abs(theirs[kind + "32"].astype(np.float64) - exact).max()
        print(f"{policy_cases.NETWORKS[index]}, {rows} rows: {kind}: twin {twin:.3e}, torch {torch:.3e}, "
              f"ratio {twin / torch:.2f}")
        distances.append((kind, twin, torch))
    for kind, twin, torch in distances:  # (after all three were printed)
        assert twin <= 4.0 * torch, (kind, twin, torch)


# ---- 3: the subgradient at the clip bounds ------------------------------------------------------------------------------------
def old_log_prob_for(log_prob, ds):
    """A float32 `old` with log_prob - old == d exactly for one of the candidates ds (searched among the neighbours of
    log_prob - d: the difference of two floats of this size is a multiple of their ulp, which not every d is)."""
    for d in ds:
        guess = F32(log_prob) - F32(d)
        for step in range(8):
            for old in ((guess.view(np.uint32) + np.uint32(step)).view(F32),
                        (guess.view(np.uint32) - np.uint32(step)).view(F32)):
                if F32(log_prob) - old == F32(d):
                    return old
    return None


def d_with_ratio(target):
    """Every float32 d near log(target) whose ratio (definition step 4) is exactly `target`."""
    centre = F32(np.log(np.float64(target)))
    around = (centre.view(np.uint32).astype(np.int64) + np.arange(-4000, 4001)).astype(np.uint32).view(F32)
    down = around <= 0
    with np.errstate(all="ignore"):
        ratio = np.where(down, policy.exp32(np.where(down, around, F32(0))), F32(1) / policy.exp32(np.where(down, F32(0), -around)))
    hits = around[ratio == F32(target)]
    assert hits.size, f"no float32 d gives the ratio {target}"
    return hits


def test_subgradient_cases_against_autograd(tmp_path, ppocheck):
    """Ratios exactly at 1 - c and 1 + c, inside, and outside on both sides, each with A > 0, A < 0 and A = 0: the head
    gradient of the surrogate is torch's (min and clamp by autograd, float32, in a process of its own) times the ratio;
    the twin and the host build agree as bytes.  Advantages are not normalised, so A is what the batch holds."""
    spec = cases.spec_of((3, (4,), (4,), 3, "tanh"))
    state = policy_cases.state_dict(spec, 5)
    state["action_net.weight"] *= F32(6)  # (peaked distributions: the log-probability of the likeliest action is fine-grained)
    params = spec.pack(state)
    c = F32(0.2)
    lo, hi = F32(1) - c, F32(1) + c
    wanted_ratios = [lo, hi, F32(1), F32(0.5), F32(1.5), F32(0.9), F32(1.1)]
    ds = [np.array([0], dtype=F32) if r == 1 else d_with_ratio(r) for r in wanted_ratios]
    rows = len(ds) * 3
    rng = np.random.default_rng(0)
    pool = rng.standard_normal((2000, 3)).astype(F32)  # (rows to choose from: not every log-probability can meet every d)
    pool_logits = policy._net(spec, spec.nets(params)[0], pool)
    pool_actions = pool_logits.argmax(axis=1).astype(np.int64)
    pool_log_probs = policy.log_softmax(pool_logits)[np.arange(2000), pool_actions]
    chosen, old, at = [], [], 0
    for candidates in ds:
        for _ in range(3):
            while old_log_prob_for(pool_log_probs[at], candidates) is None:
                at += 1
            chosen.append(at)
            old.append(old_log_prob_for(pool_log_probs[at], candidates))
            at += 1
    obs, actions, log_probs, old = pool[chosen], pool_actions[chosen], pool_log_probs[chosen], np.array(old, dtype=F32)
    adv = np.tile(np.array([1.5, -0.75, 0.0], dtype=F32), len(ds))
    batch = {"observations": obs, "actions": actions, "log_probs": old, "advantages": adv,
             "returns": rng.standard_normal(rows).astype(F32)}
    d = log_probs - old
    down = d <= 0
    ratio = np.where(down, policy.exp32(np.where(down, d, F32(0))), F32(1) / policy.exp32(np.where(down, F32(0), -d)))
    assert (ratio.reshape(-1, 3) == np.array(wanted_ratios, dtype=F32)[:, None]).all()  # (exactly at the bounds, too)
    np.savez(tmp_path / "in.npz", ratio=ratio, adv=adv, clip_range=0.2)
    subprocess.run([sys.executable, "-m", "tests.learner_io_cases", "--torch-subgradient", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=300)
    slope = np.load(tmp_path / "out.npz")["slope"]
    assert set(np.unique(slope)) == {F32(0), F32(1.5), F32(-0.75)}
    wanted_g = slope * ratio
    # the pi head's bias gradient is sum_b dlogit[b]; with ent_coef = 0 and B = 1 per call it is -g (onehot - p) / 1
    hyper = learner.Hyper(3e-4, 0.2, 0.0, 0.5, 0.5, 0.9, 0.999, 1e-5, 0)
    head_bias = [at for name, at, _, _ in spec.entries if name == "action_net.bias"][0]
    probabilities = np.exp(policy.log_softmax(policy._net(spec, spec.nets(params)[0], obs)).astype(np.float64))
    for b in range(rows):
        grad, terms, _ = learner.ppo_gradient_numpy(spec, params, batch, [b], hyper)
        onehot = np.eye(3)[actions[b]]
        want = -np.float64(wanted_g[b]) * (onehot - probabilities[b])
        assert np.allclose(grad[head_bias:head_bias + 3], want, rtol=1e-5, atol=1e-7), (b, ratio[b], adv[b])
        if wanted_g[b] == 0:
            assert (grad[head_bias:head_bias + 3] == 0).all()  # (an exact zero, not a small number)
        assert terms[4][0] == (1.0 if abs(ratio[b] - F32(1)) > c else 0.0)
    state = learner.fresh_state(spec)
    for index in (np.arange(rows), np.array([4]), np.array([0, 0, 3])):
        same(host_update(ppocheck, spec, params, state, batch, index, hyper),
             learner.ppo_update_numpy(spec, params, state, batch, index, hyper), "the subgradient batch")


def test_equal_advantages_and_a_single_sample(ppocheck):
    """All advantages equal: the standard deviation is 0, every normalised advantage is 0, the surrogate's gradient
    vanishes and the update is taken.  B = 1: no normalisation."""
    spec, params, batch, indices = cases.update_inputs(1, 9)
    flat = dict(batch, advantages=np.full(12, 0.7, dtype=F32))
    hyper = cases.hyper_of(0, ent_coef=0.0, vf_coef=0.0)
    state = learner.fresh_state(spec)
    got = learner.ppo_update_numpy(spec, params, state, flat, indices[0], hyper)
    assert got[2][0] == 0 and got[2][5] == 0 and got[2][7] == 0 and bits(got[0]) == bits(params)
    assert learner.state_parts(spec, got[1])[0] == 1
    same(host_update(ppocheck, spec, params, state, flat, indices[0], hyper), got, "equal advantages")
    one = learner.ppo_update_numpy(spec, params, state, batch, indices[0][:1], cases.hyper_of(0))
    raw = learner.ppo_update_numpy(spec, params, state, batch, indices[0][:1], cases.hyper_of(0, normalize_advantage=0))
    same(one, raw, "B = 1")
    same(host_update(ppocheck, spec, params, state, batch, indices[0][:1], cases.hyper_of(0)), one, "B = 1")


# ---- 4: the skip rules ------------------------------------------------------------------------------------------------------------
def test_skipped_updates_change_nothing(ppocheck):
    spec, params, batch, indices = cases.update_inputs(1, 9)
    first = cases.twin_updates(1, 9)[0]
    for name, (changed, chosen, flag) in cases.skip_variants(batch, indices).items():
        got = learner.ppo_update_numpy(spec, first[0], first[1], changed, chosen, cases.hyper_of(1))
        assert got[2][7] == flag, name
        assert bits(got[0]) == bits(first[0]) and bits(got[1]) == bits(first[1]), name
        assert (got[2][:7].view(np.uint32) != 0x7FC00000).sum() >= 3, name  # (the loss entries are still written)
        same(host_update(ppocheck, spec, first[0], first[1], changed, chosen, cases.hyper_of(1)), got, name)
    taken = learner.ppo_update_numpy(spec, first[0], first[1], batch, indices[1], cases.hyper_of(1))
    same(taken, cases.twin_updates(1, 9)[1], "the next valid update")


def test_returns_of_1e30(ppocheck):
    """Returns of 1e30: the value loss overflows float32 (inf in the stats), but the norm of the definition is a float64
    sum of float64 squares -- about 1e30, finite -- so the update is taken, clipped to max_grad_norm, and every parameter
    stays finite.  (torch takes the norm in float32, where it is inf; that is the case infinite returns cover here.)"""
    spec, params, batch, indices = cases.update_inputs(1, 9)
    huge = dict(batch, returns=np.full(12, 1e30, dtype=F32))
    state = learner.fresh_state(spec)
    got = learner.ppo_update_numpy(spec, params, state, huge, indices[0], cases.hyper_of(0))
    print("returns of 1e30: stats", got[2])
    assert np.isinf(got[2][1]) and np.isfinite(got[2][5]) and got[2][5] > 1e25 and got[2][7] == 0
    assert np.isfinite(got[0]).all() and bits(got[0]) != bits(params)
    same(host_update(ppocheck, spec, params, state, huge, indices[0], cases.hyper_of(0)), got, "returns of 1e30")


# ---- 5: the numpy Learner ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(cases.E2E_KINDS))
def test_twin_train_runs(kind, no_gpu):  # noqa: F811
    """collect + train twice over the numpy twins: 2 epochs of minibatches of 16 and 12; the parameters move, every
    update is taken, and the second rollout differs from one collected with the first parameters."""
    runs = cases.twin_train_runs(kind)
    assert runs[0]["stats/0"].shape == (4, 8) and (runs[1]["stats/0"][:, 7] == 0).all()
    assert bits(runs[0]["params"]) != bits(runs[1]["params"])
    assert learner.state_parts(policy_cases.e2e_spec(kind), runs[1]["state"])[0] == 8
    unchanged = policy_cases.twin_runs(kind, cases.E2E_ENVS)
    assert bits(unchanged[0]["log_probs"]) == bits(runs[0]["log_probs"])
    assert bits(unchanged[1]["log_probs"]) != bits(runs[1]["log_probs"])  # (the updated parameters were used)


def test_learner_surface(no_gpu):  # noqa: F811
    spec = policy_cases.e2e_spec("plain")
    twin = harness.Policy(spec, 0)
    twin.load_state_dict(policy_cases.state_dict(spec, 3))
    with pytest.raises(TypeError, match="Policy"):
        harness.Learner(spec)
    with pytest.raises(TypeError, match="DevicePolicy"):
        harness.DeviceLearner(twin)
    with pytest.raises(ValueError, match="betas"):
        harness.Learner(twin, betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="hyper-parameter"):
        harness.Learner(twin, learning_rate=float("nan"))
    env = policy_cases.make_env("plain", 2, False)
    try:
        rollout = harness.Rollout(env, cases.T, cases.GAMMA, cases.GAE_LAMBDA)
        rollout.start(env.reset()[0])
        first = harness.Learner(twin, learning_rate=1e-2)
        with pytest.raises(ValueError, match="not finished"):
            first.train(rollout, 1, 8)
        rollout.collect(twin)
        with pytest.raises(ValueError):
            first.train(rollout, 0, 8)
        with pytest.raises(ValueError):
            first.train(rollout, 1, 1025)
        first.train(rollout, 1, 8, generator=np.random.default_rng(1))
        kept, kept_params = first.state_dict(), twin.params.copy()
        assert kept["step"] == 2 and kept["bc1"] == 1.0 - 0.9 * (1.0 - (1.0 - 0.9))
        straight = first.train(rollout, 1, 8, generator=np.random.default_rng(2))
        want = twin.params.copy(), first.state.copy()
        twin.params[:] = kept_params
        second = harness.Learner(twin, learning_rate=1e-2)
        second.load_state_dict(kept)
        assert bits(second.train(rollout, 1, 8, generator=np.random.default_rng(2))) == bits(straight)
        assert bits(twin.params) == bits(want[0]) and bits(second.state) == bits(want[1])
    finally:
        env.close()


def test_import_stays_free_of_torch():
    code = ("import sys; from reinfocus_amd.environments import harness; harness.Learner; harness.DeviceLearner; "
            "harness.ppo_update_numpy; assert 'torch' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


# ---- 6: the binding and the constants ------------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    struct = re.search(r"typedef struct rf_ppo_desc \{(.*?)\} rf_ppo_desc;", text, flags=re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    fields = []
    for kind, names in re.findall(r"(double|int) ([\w, ]+);", struct):
        fields += [(name.strip(), ctypes.c_double if kind == "double" else ctypes.c_int) for name in names.split(",")]
    assert fields == list(_native.PpoDesc._fields_)
    assert [name for name, _ in fields[:9]] == list(learner.Hyper._fields)
    assert ctypes.sizeof(_native.PpoDesc) == 8 * 8 + 2 * 4
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    for entry, count in (("rf_ppo_update", 16), ("rf_ppo_state_size", 2), ("rf_ppo_workspace_size", 3)):
        declaration = re.search(r"\b%s\s*\((.*?)\)\s*;" % entry, text, flags=re.S).group(1)
        wanted = [ctypes.c_void_p if "*" in p else ctypes.c_int for p in declaration.split(",")]
        names = re.search(r"lib\.%s\.argtypes = \[(.*?)\]" % entry, source).group(1).split(",")
        assert [{"vp": ctypes.c_void_p, "i32": ctypes.c_int}[name.strip()] for name in names] == wanted
        assert len(wanted) == count
    for name, value in (("RF_PPO_MAX_BATCH", learner.MAX_BATCH), ("RF_PPO_INVALID", learner.INVALID),
                        ("RF_PPO_NONFINITE", learner.NONFINITE)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value
    kernels = open(os.path.join(ROOT, "reinfocus_amd", "csrc", "rf_ppo.h")).read()
    assert int(re.search(r"constexpr int kPpoStateHeader = (\d+);", kernels).group(1)) == learner.STATE_HEADER


def test_workspace_grows_with_the_batch(ppocheck):
    desc = ctypes.byref(_native.PolicyDesc(*cases.spec_of(cases.NETWORKS[3]).desc()))
    sizes = [ppocheck.ppc_workspace_size(desc, count) for count in (1, 64, 65, 1024)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and all(size % 8 == 0 for size in sizes)
    assert ppocheck.ppc_workspace_size(desc, 0) == 0 and ppocheck.ppc_workspace_size(desc, 1025) == 0
    assert ppocheck.ppc_workspace_size(desc, 512) < ppocheck.ppc_workspace_size(desc, 513)  # (refused on the GPU for 513)
