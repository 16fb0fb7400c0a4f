"""CPU tests of the sde policy's definition (include/reinfocus_hip.h, "sde policy"): the numpy twin (environments/sde.py,
learner.sde_gradient_numpy) against the host build of the kernels' own headers (tests/sdecheck) as bytes, on the networks
and batches of the GPU tests (513, 1000 and 1024 rows among them); normal32 and log32 against float64; the update against torch's Normal, autograd,
clip_grad_norm_ and Adam on the CPU; the log_std gradient alone; packing and the refusals of the surface.

Measured on the development machine (profiles/sde.md records the run): normal32's largest absolute error is 4.60e-7 (at
u = 3.33e-16, half an ulp of the float32 result there), log32's largest relative error over the normal float32 range
1.68e-7, log64's against math.log 3.19e-16.  normal32 is in order on all 444 596 224 pairs of neighbouring float32
arguments of [2^-54, 1/2], in either half (a run of ten minutes, not repeated here: the order test below takes the
joins, the ends and a dense sample)."""

import ctypes
import math
import os
import statistics
import subprocess
import sys

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, learner, policy, sde
from tests import helpers
from tests import policy_io_cases as policy_cases
from tests import rollout_io_cases as rollout_cases
from tests import sde_io_cases as cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = cases.bits
# twice the largest errors measured (the module docstring): what the issue allows
NORMAL32_BOUND, LOG32_BOUND, LOG64_BOUND = 2 * 4.60e-7, 2 * 1.68e-7, 2 * 3.19e-16


@pytest.fixture(scope="module")
def sdecheck():
    lib = ctypes.CDLL(helpers.built("tests/sdecheck", "libsdecheck.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.sdc_params_size.restype = lib.sdc_state_size.restype = lib.sdc_workspace_size.restype = ctypes.c_ulonglong
    lib.sdc_params_size.argtypes = lib.sdc_state_size.argtypes = [vp]
    lib.sdc_workspace_size.argtypes = [vp, i32]
    lib.sdc_normal32.argtypes = lib.sdc_log32.argtypes = lib.sdc_expw32.argtypes = lib.sdc_log64.argtypes = [vp, i32, vp]
    lib.sdc_noise.argtypes = [vp, vp, i32, vp, vp]
    lib.sdc_forward.argtypes = [vp, vp, i32] + [vp] * 10
    lib.sdc_update.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    return lib


def host_scalar(function, x, dtype):
    x = np.ascontiguousarray(x, dtype=dtype)
    out = np.zeros(x.size, dtype=F32)
    function(x.ctypes.data, x.size, out.ctypes.data)
    return out


def host_update(lib, spec, params, state, batch, index, hyper, gradient=False):
    """sdc_update on copies: (params, state, stats[, the packed gradient before clipping])."""
    params, state = params.copy(), state.copy()
    stats, grad = np.zeros(8, dtype=F32), np.zeros(spec.size, dtype=F32)
    arrays = [np.ascontiguousarray(batch[key]) for key in learner.BATCH_KEYS]
    index = np.ascontiguousarray(index, dtype=np.int64)
    rc = lib.sdc_update(ctypes.byref(_native.PolicyDesc(*spec.desc())), ctypes.byref(_native.PpoDesc(*hyper)),
                        params.ctypes.data, state.ctypes.data, arrays[1].shape[0], *(a.ctypes.data for a in arrays),
                        index.size, index.ctypes.data, stats.ctypes.data, grad.ctypes.data)
    assert rc == 0
    return (params, state, stats, grad) if gradient else (params, state, stats)


def same(got, want, what):
    for name, x, y in zip(("params", "state", "stats"), got, want):
        assert bits(x) == bits(y), f"{what}: {name} differ"


# ---- 1: the twin against the host build -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))
def test_reset_and_forward_of_the_header_equal_the_twin(index, n, sdecheck):
    spec, params, obs, final_obs = cases.forward_inputs(index, n)
    desc = ctypes.byref(_native.PolicyDesc(*spec.desc()))
    assert sdecheck.sdc_params_size(desc) == spec.size
    for offset in cases.OFFSETS:
        theta, sampled, deterministic = cases.wanted_forward(index, n, offset)
        words = (ctypes.c_ulonglong * 4)(*policy.generator_words(policy_cases.generator_at(offset)[0]))
        got_theta = np.zeros((n, spec.latent), dtype=F32)
        assert sdecheck.sdc_noise(desc, params.ctypes.data, n, words, got_theta.ctypes.data) == 0
        assert bits(got_theta) == bits(theta)
        for want, noise in ((sampled, got_theta), (deterministic, None)):
            outs = {name: np.zeros(n, dtype=F32) for name in cases.FORWARD_OUTPUTS}
            assert sdecheck.sdc_forward(desc, params.ctypes.data, n, obs.ctypes.data, final_obs.ctypes.data,
                                        None if noise is None else noise.ctypes.data,
                                        *(outs[name].ctypes.data for name in cases.FORWARD_OUTPUTS)) == 0
            for name in cases.FORWARD_OUTPUTS:
                assert bits(outs[name]) == bits(want[name]), (name, offset)


def test_hostile_forward_inputs_hold_what_they_promise():
    """log_std rows at -100, 0 and +3; raw actions past +-1 next to ones inside, clamped for the environment; +-0 and
    subnormal observations; a NaN row whose action is NaN and reaches the environment as NaN; the deterministic action
    is the mean."""
    spec, params, obs, _ = cases.forward_inputs(1, cases.TILE + 1)
    assert list(params[spec.log_std_at:spec.log_std_at + 3]) == [-100.0, 0.0, 3.0]
    assert list(cases.forward_inputs(0, 1)[1][-1:]) == [3.0]
    assert (np.signbit(obs) & (obs == 0)).any() and ((obs != 0) & (np.abs(obs) < 1e-38)).any()
    theta, sampled, deterministic = cases.wanted_forward(1, cases.TILE + 1, 0)
    assert (theta[:, 0] == 0).all() and np.isfinite(theta).all()
    raw, clamped = sampled["actions"], sampled["env_actions"]
    fine = np.isfinite(raw)
    assert (np.abs(raw[fine]) > 1).any() and (np.abs(raw[fine]) < 1).any()
    assert bits(clamped[fine]) == bits(np.clip(raw[fine], -1, 1)) and (np.abs(clamped[fine]) <= 1).all()
    # the row that is NaN throughout: relu turns it into zeros (the definition of "policy"), tanh passes it on
    nan_row = (cases.TILE + 1) // 2
    assert np.isfinite(raw[nan_row])
    through = cases.wanted_forward(2, cases.TILE + 1, 0)[1]
    assert np.isnan(cases.forward_inputs(2, cases.TILE + 1)[2][nan_row]).all()
    assert all(bits(through[name][nan_row]) == bits(policy._NAN) for name in ("actions", "env_actions", "log_probs", "sigma"))
    assert bits(deterministic["actions"]) == bits(deterministic["mean"]) == bits(sampled["mean"])


@pytest.mark.parametrize("count", cases.BATCHES)
@pytest.mark.parametrize("index", range(len(cases.NETWORKS)), ids=lambda i: "-".join(str(v) for v in cases.NETWORKS[i]))
def test_update_of_the_header_equals_the_twin(index, count, sdecheck):
    spec, params, batch, indices = cases.update_inputs(index, count)
    want = cases.twin_updates(index, count)
    state = learner.fresh_state(spec)
    assert sdecheck.sdc_state_size(ctypes.byref(_native.PolicyDesc(*spec.desc()))) == 4 * state.size
    for update in range(cases.UPDATES):
        params, state, stats = host_update(sdecheck, spec, params, state, batch, indices[update], cases.hyper_of(update))
        same((params, state, stats), want[update], f"update {update}")
    assert learner.state_parts(spec, state)[0] == cases.UPDATES and np.isfinite(want[-1][2]).all()


@pytest.mark.parametrize("index,count", cases.LIMIT_CASES,
                         ids=lambda v: "-".join(str(x) for x in cases.NETWORKS[v]) if v < len(cases.NETWORKS) else str(v))
def test_update_of_the_header_equals_the_twin_at_the_batch_limits(index, count, sdecheck):
    """513, 1000 and 1024 rows (cases.LIMIT_CASES): the twin's order of summation past 512 rows against the host build's
    plain loops.  The index still repeats a row and some index holds the last row; the schedule still clips once and
    once not."""
    test_update_of_the_header_equals_the_twin(index, count, sdecheck)
    spec, params, batch, indices = cases.update_inputs(index, count)
    assert batch["actions"].shape[0] == count + 3 and all(chosen.size == count for chosen in indices)
    assert indices[0][-1] == indices[0][0] and any(count + 2 in chosen for chosen in indices)
    norms = [stats[5] for _, _, stats in cases.twin_updates(index, count)]
    assert norms[1] < cases.SCHEDULE[1][0] and norms[2] > cases.SCHEDULE[2][0]
    desc = ctypes.byref(_native.PolicyDesc(*spec.desc()))
    assert sdecheck.sdc_workspace_size(desc, 512) < sdecheck.sdc_workspace_size(desc, 513)
    assert sdecheck.sdc_workspace_size(desc, 1024) > 0 and sdecheck.sdc_workspace_size(desc, 1025) == 0


def test_hostile_minibatches_hold_what_they_promise():
    """Ratios inside the range and past both bounds, a repeated index, a norm that clips and one that does not, raw
    actions past +-1, and a log_std that moves."""
    spec, params, batch, indices = cases.update_inputs(2, 64)
    got = sde.sde_numpy(spec, params, batch["observations"], None, None, deterministic=True)
    d = sde.log_prob_of(batch["actions"], got["mean"], got["sigma"]) - batch["log_probs"]
    assert (d > 0.25).any() and (d < -0.25).any() and (np.abs(d) < 0.1).any()
    assert len(set(indices[0])) == 63 and indices[0][-1] == indices[0][0]
    assert (np.abs(batch["actions"]) > 1).any()
    updates = cases.twin_updates(2, 64)
    norms = [stats[5] for _, _, stats in updates]
    assert norms[1] < cases.SCHEDULE[1][0] and norms[2] > cases.SCHEDULE[2][0] and updates[0][2][4] > 0
    moved = updates[-1][0][spec.log_std_at:] != params[spec.log_std_at:]
    assert moved[1:].all() and not moved[0]  # (log_std_0 = -100: its standard deviation is 0, and so is its gradient)


def test_skipped_updates_change_nothing(sdecheck):
    spec, params, batch, indices = cases.update_inputs(2, 64)
    first = cases.twin_updates(2, 64)[0]
    for name, (start, changed, chosen, flag) in cases.skip_variants(spec, first[0], batch, indices).items():
        got = learner.ppo_update_numpy(spec, start, first[1], changed, chosen, cases.hyper_of(1))
        assert got[2][7] == flag and bits(got[0]) == bits(start) and bits(got[1]) == bits(first[1]), name
        same(host_update(sdecheck, spec, start, first[1], changed, chosen, cases.hyper_of(1)), got, name)


# ---- 2: normal32 and the wide logarithm against float64 ----------------------------------------------------------------------
def normal_draws():
    """The grid (k + 1/2) / 2^16, then the 1024 smallest and the 1024 largest draws j * 2^-53: sorted."""
    return np.concatenate([np.arange(1024) * 2.0 ** -53, (np.arange(65536) + 0.5) / 65536,
                           1.0 - np.arange(1024, 0, -1) * 2.0 ** -53])


def test_normal32_against_float64(sdecheck):
    u = normal_draws()
    assert (np.diff(u) > 0).all() and u[0] == 0.0
    x = sde.normal32(u)
    assert bits(host_scalar(sdecheck.sdc_normal32, u, np.float64)) == bits(x)
    assert np.isfinite(x).all()  # (u = 0 included)
    assert (np.diff(x) >= 0).all()
    half = sde.normal32(np.array([0.5]))
    assert half[0] == 0 and not np.signbit(half[0])  # (the definition: normal32(1/2) is +0)
    inverse = statistics.NormalDist().inv_cdf
    exact = np.array([inverse(float(v)) for v in u[1:]])
    error = np.abs(x[1:].astype(np.float64) - exact)
    worst = int(error.argmax())
    print(f"normal32: largest absolute error {error.max():.3e} at u = {u[1:][worst]:.3e}; normal32(0) = {x[0]}")
    assert error.max() <= NORMAL32_BOUND
    assert -8.5 < x[0] < x[1]  # (u = 0 is the quantile of 2^-54)


def float32_run(first, count):
    """`count` consecutive float32 values from `first` on, as bit patterns in order."""
    start = int(np.array(first, dtype=F32).view(np.uint32))
    return np.arange(start, start + count, dtype=np.uint32).view(F32)


@pytest.mark.parametrize("upper", [False, True], ids=["lower-half", "upper-half"])
def test_normal32_never_decreases_between_neighbouring_arguments(upper, sdecheck):
    """The definition's claim, on every float32 argument p where it could fail first: 2^17 neighbours on either side of
    the join at p = 0.075 and of the one at r = 5 (p = exp(-25)), the smallest arguments from 2^-54 on, the ones below
    1/2, a stretch around p = 0.3 (where a float32 evaluation moves by about one ulp per step) -- and every 1009th
    float32 of [2^-54, 1/2]: no pair is out of order, and the host build gives the same bits on the runs through the
    draws that produce them."""
    span = 1 << 17
    runs = [float32_run(F32(0.075), span), float32_run(F32(0.075) - F32(0.075) * F32(2.0 ** -7), span),
            float32_run(F32(math.exp(-25.0)) * F32(1 - 2.0 ** -8), 2 * span), float32_run(2.0 ** -54, span),
            float32_run(F32(0.5) - F32(2.0 ** -9), (1 << 16) + 1), float32_run(0.3, span), float32_run(0.2, span)]
    low, high = (int(np.array(v, dtype=F32).view(np.uint32)) for v in (2.0 ** -54, 0.5))
    runs.append(np.arange(low, high + 1, 1009, dtype=np.uint32).view(F32))
    assert runs[0][0] == F32(0.075) and runs[1][0] < F32(0.075) < runs[1][-1] and runs[4][-1] == F32(0.5)
    assert runs[2][0] < F32(math.exp(-25.0)) < runs[2][-1]
    for p in runs:
        assert (np.diff(p) > 0).all() and p[0] >= F32(2.0 ** -54) and p[-1] <= F32(0.5)
        x = sde.normal32_of_p(p, np.full(p.size, upper))
        steps = np.diff(-x if upper else x)  # (as a function of p the upper half falls)
        assert np.isfinite(x).all() and (steps >= 0).all(), (float(p[0]), int((steps < 0).sum()), float(steps.min()))
        # the same through draws: u = p below 1/2, u = 1 - p above (both exact for these p >= 2^-29 or so)
        exact = p[p >= F32(2.0 ** -28)].astype(np.float64)[:4096]
        u = 1.0 - exact if upper else exact
        keep = (u >= 0.5) == upper
        got = host_scalar(sdecheck.sdc_normal32, u[keep], np.float64)
        assert bits(got) == bits(sde.normal32(u[keep])) == bits(sde.normal32_of_p(exact[keep].astype(F32), np.full(int(keep.sum()), upper)))


def test_log64_against_math_log(sdecheck):
    rng = np.random.default_rng(8)
    s = np.concatenate([np.exp2(rng.uniform(-1022, 1023.9, 100000)), np.exp2(rng.uniform(-60, 0, 100000)),
                        [1.0, 2.0 ** -54, 0.075, math.exp(-25.0), 2.2250738585072014e-308, 1.7976931348623157e308]])
    got = sde.log64(s)
    host = np.zeros(s.size)
    sdecheck.sdc_log64(np.ascontiguousarray(s).ctypes.data, s.size, host.ctypes.data)
    assert bits(host) == bits(got)
    exact = np.array([math.log(v) for v in s])
    apart = s != 1.0
    relative = np.abs(got[apart] - exact[apart]) / np.abs(exact[apart])
    print(f"log64: largest relative error {relative.max():.3e} against math.log over {s.size} values")
    assert relative.max() <= LOG64_BOUND and got[~apart][0] == 0


def test_log32_over_the_normal_range_against_float64(sdecheck):
    exponents = np.linspace(-126.0, 127.99, 200001)
    s = np.unique(np.concatenate([np.exp2(exponents).astype(F32), np.array([2.0 ** -126, 3.4028235e38, 1.0, 1e-3], dtype=F32)]))
    got = policy.log32(s)
    assert bits(host_scalar(sdecheck.sdc_log32, s, F32)) == bits(got)
    exact = np.array([math.log(float(v)) for v in s])
    apart = s != 1.0
    relative = np.abs(got[apart].astype(np.float64) - exact[apart]) / np.abs(exact[apart])
    print(f"log32: largest relative error {relative.max():.3e} over {s.size} values of [2^-126, 2^128)")
    assert relative.max() <= LOG32_BOUND and got[~apart][0] == 0
    x = np.array([-200.0, -87.5, -87.0, -3.0, -0.0, 0.0, 1e-3, 3.0, 87.0, 87.5, 90.0, np.inf, -np.inf, np.nan], dtype=F32)
    wide = sde.expw32(x)
    assert bits(host_scalar(sdecheck.sdc_expw32, x, F32)) == bits(wide)
    assert wide[0] == 0 and wide[4] == wide[5] == 1 and np.isinf(wide[[9, 10, 11, 13]]).all() and wide[12] == 0
    assert np.allclose(wide[[3, 6, 7]], np.exp(x[[3, 6, 7]].astype(np.float64)), rtol=1e-6)


# ---- 3: the twin against torch's Normal, autograd, clip_grad_norm_ and Adam -----------------------------------------------------
def autograd_inputs(index):
    """A minibatch of 64 normal rows with the twin's own sampled actions; the stored log-probabilities come from a copy
    of the parameters whose mean head is perturbed, scaled (the first of a fixed list) so that about a quarter of the
    ratios leave the clip range."""
    spec = cases.spec_of(cases.NETWORKS[index])
    state = cases.state_dict(spec, 60 + index)
    rng = np.random.default_rng(index)
    obs = rng.standard_normal((64, spec.obs_width)).astype(F32)
    noise = rng.standard_normal(state["action_net.weight"].shape).astype(F32)
    params = spec.pack(state)
    theta = sde.noise_numpy(params[spec.log_std_at:], rng.random(64 * spec.latent))
    new = sde.sde_numpy(spec, params, obs, None, theta)
    actions = new["actions"]
    for scale in (0.005, 0.01, 0.02, 0.03, 0.04, 0.06, 0.08, 0.12, 0.2, 0.3, 0.5):
        moved = dict(state)
        moved["action_net.weight"] = state["action_net.weight"] + F32(scale) * noise
        there = sde.sde_numpy(spec, spec.pack(moved), obs, None, None, deterministic=True)
        old = sde.log_prob_of(actions, there["mean"], there["sigma"])
        share = np.mean(np.abs(np.exp((new["log_probs"] - old).astype(np.float64)) - 1) > 0.2)
        if share >= 0.2:
            break
    batch = {"observations": obs, "actions": actions, "log_probs": old, "advantages": rng.standard_normal(64).astype(F32),
             "returns": rng.standard_normal(64).astype(F32)}
    return spec, state, params, batch, share


def torch_run(tmp_path, spec, state, batch, hyper, updates):
    np.savez(tmp_path / "in.npz", names=np.array(spec.keys()), activation=spec.activation, obs=batch["observations"],
             actions=batch["actions"], old_log_probs=batch["log_probs"], advantages=batch["advantages"],
             returns=batch["returns"], clip_range=hyper.clip_range, ent_coef=hyper.ent_coef, vf_coef=hyper.vf_coef,
             max_grad_norm=hyper.max_grad_norm, learning_rate=hyper.learning_rate, updates=updates, **state)
    subprocess.run([sys.executable, "-m", "tests.sde_io_cases", "--torch-learner", str(tmp_path / "in.npz"),
                    str(tmp_path / "out.npz")], cwd=ROOT, check=True, timeout=300)
    return np.load(tmp_path / "out.npz")


@pytest.fixture(scope="module")
def torch_runs(tmp_path_factory):
    """index -> (inputs, torch's results): one torch process per network, shared by the two tests below."""
    hyper = learner.Hyper(3e-4, 0.2, 0.01, 0.5, 0.5, 0.9, 0.999, 1e-5, 1)
    seen = {}

    def run(index):
        if index not in seen:
            inputs = autograd_inputs(index)
            seen[index] = inputs, torch_run(tmp_path_factory.mktemp(f"torch{index}"), inputs[0], inputs[1], inputs[3],
                                            hyper, 10), hyper
        return seen[index]
    return run


@pytest.mark.parametrize("index", [1, 2])
def test_gradient_and_updates_are_no_further_from_float64_than_four_times_torch(index, torch_runs, sdecheck):
    """As tests/test_learner_logic.py's table, log_std included: the twin's gradient before clipping, its parameters
    after the first update of a fresh optimizer and after 10 updates on one minibatch, each against the same from torch
    in float64 (torch.distributions.Normal, autograd, clip_grad_norm_, Adam(eps=1e-5)); the largest distance may be at
    most 4 x that of torch's own float32 run.  Both distances are printed (profiles/sde.md records a run)."""
    (spec, state, params, batch, share), theirs, hyper = torch_runs(index)
    print(f"{cases.NETWORKS[index]}: share of ratios outside the clip range {share:.3f}")
    assert 0.10 <= share <= 0.40
    every = np.arange(64)
    grad, terms, invalid = learner.sde_gradient_numpy(spec, params, batch, every, hyper)
    assert not invalid and abs(terms[4].mean() - float(theirs["clip_fraction64"])) <= 2 / 64
    ours = {"grad": grad}
    optimizer = learner.fresh_state(spec)
    for update in range(10):
        params, optimizer, stats = learner.ppo_update_numpy(spec, params, optimizer, batch, every, hyper)
        assert stats[7] == 0
        if update == 0:
            ours["first"] = params
    ours["last"] = params
    assert bits(host_update(sdecheck, spec, spec.pack(state), learner.fresh_state(spec), batch, every, hyper, True)[3]) \
        == bits(grad)
    for kind in ("grad", "first", "last"):
        exact = theirs[kind + "64"]
        assert theirs[kind + "32"].dtype == F32 and exact.dtype == np.float64 and exact.size == spec.size
        twin = np.abs(ours[kind].astype(np.float64) - exact).max()
        torch = np.abs(theirs[kind + "32"].astype(np.float64) - exact).max()
        print(f"{cases.NETWORKS[index]}: {kind}: twin {twin:.3e}, torch {torch:.3e}, ratio {twin / torch:.2f}")
        assert twin <= 4.0 * torch, (kind, twin, torch)


@pytest.mark.parametrize("index", [1, 2])
def test_log_std_gradient_is_autograd_with_the_latent_detached_inside_the_variance_only(index, torch_runs):
    """learn_features=False: torch's float64 gradient with the latent detached inside the variance and not in the mean.
    log_std's gradient agrees to float32 accuracy -- and so does the last pi hidden layer's, which a detach in the mean
    (or none in the variance) would change by far more: a gradient through the variance into the latent is of the size
    of the log_std gradient itself."""
    (spec, state, params, batch, _), theirs, hyper = torch_runs(index)
    grad, _, _ = learner.sde_gradient_numpy(spec, params, batch, np.arange(64), hyper)
    exact = theirs["grad64"]
    at = spec.log_std_at
    scale = np.abs(exact[at:]).max()
    error = np.abs(grad[at:].astype(np.float64) - exact[at:]).max()
    print(f"{cases.NETWORKS[index]}: log_std gradient: largest {scale:.3e}, largest error {error:.3e}")
    assert scale > 1e-4 and error <= 1e-5 * scale + 1e-9
    # the layer that feeds the latent: entry 2 * (layers - 1) of the packing is its weight
    _, first, shape, _ = spec.entries[2 * (len(spec.pi) - 1)]
    cells = slice(first, first + int(np.prod(shape)))
    inner = np.abs(exact[cells]).max()
    assert np.abs(grad[cells].astype(np.float64) - exact[cells]).max() <= 1e-5 * inner + 1e-9


# ---- 4: packing and the surface ---------------------------------------------------------------------------------------------------
def test_packing_round_trips_through_stable_baselines3_names():
    spec = cases.spec_of((20, (5, 7), (6,), "tanh"), log_std_init=-2.0)
    plain = policy.MlpPolicySpec(20, 2, pi=(5, 7), vf=(6,), activation="tanh")
    assert spec.keys()[-1] == "log_std" and spec.keys()[:-1] == plain.keys()
    # the offsets of the hidden layers are those of a Categorical network; log_std comes after everything else
    assert [e[1] for e in spec.entries[:4]] == [e[1] for e in plain.entries[:4]]
    assert spec.entries[-1][1] == spec.size - 7 == spec.log_std_at and spec.desc()[1] == 1
    initial = spec.initial()
    assert (initial[:spec.log_std_at] == 0).all() and (initial[spec.log_std_at:] == F32(-2.0)).all()
    state = cases.state_dict(spec, 4)
    assert state["log_std"].shape == (7, 1) and state["action_net.weight"].shape == (1, 7)
    packed = spec.pack(state)
    assert bits(packed[spec.log_std_at:]) == bits(state["log_std"][:, 0])
    back = spec.unpack(packed)
    assert list(back) == spec.keys() and all(bits(back[k]) == bits(state[k]) for k in state)
    twin = harness.SdePolicy(spec, 0)
    assert bits(twin.params) == bits(initial)
    twin.load_state_dict(state)
    assert all(bits(twin.state_dict()[k]) == bits(state[k]) for k in state)
    with pytest.raises(KeyError, match="log_std"):
        spec.pack({k: v for k, v in state.items() if k != "log_std"})
    with pytest.raises(ValueError, match="log_std"):
        spec.pack(dict(state, log_std=state["log_std"][:, 0]))


def test_generator_moves_by_n_times_L_per_reset_and_by_nothing_per_act():
    spec = cases.spec_of(cases.NETWORKS[1])
    twin = harness.SdePolicy(spec, 5, num_envs=3)
    twin.load_state_dict(cases.state_dict(spec, 1))
    obs = np.zeros((3, spec.obs_width), dtype=F32)
    with pytest.raises(ValueError, match="reset_noise"):
        twin.act(obs)
    twin.act(obs, deterministic=True)
    other = np.random.PCG64DXSM(5)
    assert twin.rng_state()["state"] == other.state["state"]
    twin.reset_noise()
    theta = twin.noise()
    first = twin.act(obs)
    assert bits(twin.act(obs)[0]) == bits(first[0]) and bits(twin.noise()) == bits(theta)  # (the same noise until a reset)
    other.advance(3 * spec.latent)
    assert twin.rng_state()["state"] == other.state["state"]
    twin.reset_noise()
    assert bits(twin.noise()) != bits(theta)
    kept = twin.state_dict(), twin.rng_state(), twin.noise()
    resumed = harness.SdePolicy(spec, 99, num_envs=3)
    resumed.load_state_dict(kept[0])
    resumed.set_rng_state(kept[1])
    resumed.set_noise(kept[2])
    assert bits(resumed.act(obs)[0]) == bits(twin.act(obs)[0])
    resumed.reset_noise()
    twin.reset_noise()
    assert bits(resumed.noise()) == bits(twin.noise())


def test_collect_resets_the_noise_as_collect_rollouts_does(no_gpu):  # noqa: F811
    """Rollout.collect(SdePolicy, sde_sample_freq): a reset before the loop and at every t % freq == 0; the slab keeps
    the raw action, the environment gets the clamped one; equal to the explicit loop."""
    env = harness.VectorContinuousJumps(num_envs=3, **rollout_cases.ENV_KW)
    try:
        spec = cases.e2e_spec(env)
        runs = {}
        for how in ("collect", "explicit"):
            twin = harness.SdePolicy(spec, cases.SEED)
            twin.load_state_dict(cases.e2e_state(spec))
            buffer = harness.Rollout(env, cases.T, cases.GAMMA, cases.GAE_LAMBDA)
            buffer.start(env.reset(seed=rollout_cases.ENV_KW["seed"])[0])
            if how == "collect":
                buffer.collect(twin, sde_sample_freq=3)
            else:
                twin.reset_noise(3)
                for t in range(cases.T):
                    if t % 3 == 0:
                        twin.reset_noise(3)
                    actions, values, log_probs, _, clamped = twin.act(buffer.observations[t])
                    assert bits(clamped) == bits(np.clip(actions, -1, 1))
                    buffer.step(actions, values, log_probs, clamped)
                buffer.finish(twin.values(buffer.observations[cases.T]))
            runs[how] = policy_cases.slabs_of(buffer, np.array), twin.rng_state()["state"]
        cases.same_runs([runs["collect"][0]], [runs["explicit"][0]])
        moved = np.random.PCG64DXSM(cases.SEED)
        moved.advance((1 + 3) * 3 * spec.latent)  # (t = 0, 3, 6 and the one before the loop)
        assert runs["collect"][1] == runs["explicit"][1] == moved.state["state"]
    finally:
        env.close()


def test_refusals_of_the_surface(no_gpu):  # noqa: F811
    jumps = harness.VectorContinuousJumps(num_envs=2, **rollout_cases.ENV_KW)
    steps = harness.VectorDiscreteSteps(num_envs=2, **rollout_cases.ENV_KW)
    try:
        spec = cases.e2e_spec(jumps)
        twin = harness.SdePolicy(spec, 0)
        categorical = harness.Policy(policy.MlpPolicySpec(spec.obs_width, 13), 0)
        # an sde policy on a Discrete environment, and the mirror that has always been refused
        buffer = harness.Rollout(steps, 2)
        buffer.start(steps.reset()[0])
        with pytest.raises(ValueError, match="Gaussian head"):
            buffer.collect(twin)
        buffer = harness.Rollout(jumps, 2)
        buffer.start(jumps.reset()[0])
        with pytest.raises(ValueError, match="out of scope"):
            buffer.collect(categorical)
        with pytest.raises(ValueError, match="sde_sample_freq"):
            buffer.collect(twin, sde_sample_freq=0)
        buffer = harness.Rollout(steps, 2)
        buffer.start(steps.reset()[0])
        with pytest.raises(ValueError, match="sde_sample_freq"):
            buffer.collect(categorical, sde_sample_freq=4)
        # the learners
        with pytest.raises(ValueError, match="Gaussian head"):
            harness.Learner(twin).train(harness.Rollout(steps, 2), 1, 4)
        with pytest.raises(ValueError, match="out of scope"):
            harness.Learner(categorical).train(harness.Rollout(jumps, 2), 1, 4)
        whole = {"observations": np.zeros((4, spec.obs_width), dtype=F32), "actions": np.zeros(4, dtype=np.int64),
                 "log_probs": np.zeros(4, dtype=F32), "advantages": np.zeros(4, dtype=F32), "returns": np.zeros(4, dtype=F32)}
        with pytest.raises(ValueError, match="int64 action slab"):  # (no silent cast of indices to raw actions)
            harness.Learner(twin).update(whole, np.arange(4))
        with pytest.raises(TypeError, match="device-resident"):
            harness.DeviceSdePolicy(jumps, spec, 0)
        with pytest.raises(TypeError, match="DevicePolicy"):
            harness.DeviceLearner(twin)
        with pytest.raises(TypeError, match="SdePolicySpec"):
            harness.SdePolicy(policy.MlpPolicySpec(4, 13), 0)
    finally:
        jumps.close()
        steps.close()
    # any other action width is refused: the spec has no such argument, and the desc of the entry points must say 1
    with pytest.raises(TypeError):
        sde.SdePolicySpec(4, 2)
    assert sde.SdePolicySpec(4).desc()[1] == 1
    for action_space in (harness.spaces.Box(-1.0, 1.0, (2,), np.float32), harness.spaces.Discrete(3)):
        with pytest.raises(ValueError, match="Gaussian head"):
            sde._refuse_discrete(action_space)


def test_stand_alone_host_program_runs():
    """tests/sdecheck/sdecheck: the same source with its own main -- one reset, forward and update on a tiny network
    outside any interpreter (the form a host sanitizer build of this arithmetic takes) -- ends with status 0 and prints
    finite figures."""
    helpers.built("tests/sdecheck", "libsdecheck.so")  # (the Makefile rule that builds both)
    done = subprocess.run([os.path.join(ROOT, "tests", "sdecheck", "sdecheck")], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, done.stdout + done.stderr
    lines = done.stdout.strip().splitlines()
    assert len(lines) == 3 and lines[2].startswith("stats:") and "nan" not in done.stdout and "inf" not in done.stdout


def test_binding_matches_the_header():
    """Every rf_sde_ entry point of the header is bound with as many arguments as it declares."""
    import re

    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    seen = 0
    for name, arguments in re.findall(r"\b(?:int|unsigned long long)\s+(rf_sde_\w+)\s*\((.*?)\)\s*;", text, flags=re.S):
        bound = re.search(rf"lib\.{name}\.argtypes = \[(.*?)\]", source).group(1).split(",")
        assert len(bound) == len(arguments.split(",")), name
        assert name in _native.SYMBOLS
        seen += 1
    assert seen == 6
