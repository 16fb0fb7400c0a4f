"""CPU tests of the PPO rollout buffers (harness.Rollout, environments/rollout.py): gae_numpy -- the oracle the kernel is
held to in tests/test_gpu_rollout.py -- against an independent scalar restatement of the definition
(include/reinfocus_hip.h, "rollout") that computes in Python floats and rounds to float32 after every operation, and
against known answers worked out by hand; the twin buffer over the host twins; what is refused; the binding's argument
types against the header; and that the seeds of the GPU file end environments inside a rollout and on its last step.
The GPU's render and focus measure are replaced by a function of the state (tests/test_composed_env_logic.py::no_gpu)."""

import ctypes
import os
import re
import struct

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import harness, rollout
from tests import rollout_io_cases as cases
from tests.test_composed_env_logic import no_gpu  # noqa: F401 -- a fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bits(a):
    a = np.asarray(a)
    return a.dtype.str, a.shape, a.tobytes()


# ---- the restatement ----------------------------------------------------------------------------------------------------
def rnd(x):
    """A Python float rounded to float32 (through struct where it is in range: an independent rounding).  The sum,
    difference or product of two float32 values, taken in float64 and rounded once more, is the correctly rounded
    float32 result (53 >= 2 * 24 + 2), so `rnd(a op b)` is a float32 operation."""
    x = float(x)
    if x != x or x in (float("inf"), float("-inf")) or abs(x) >= 3.4028235677973366e38:  # (struct refuses the overflow)
        return float(F32(x))
    return struct.unpack("f", struct.pack("f", x))[0]


def restated(rewards, values, truncated, final_values, last_values, gamma, gae_lambda):
    steps, n = len(rewards), len(rewards[0])
    g, gl = rnd(gamma), rnd(gamma * gae_lambda)
    advantages = [[0.0] * n for _ in range(steps)]
    returns = [[0.0] * n for _ in range(steps)]
    with np.errstate(all="ignore"):
        for e in range(n):
            last = 0.0
            for t in range(steps - 1, -1, -1):
                r = rnd(rewards[t][e])
                if final_values is not None and truncated[t][e]:
                    r = rnd(r + rnd(g * float(final_values[t][e])))
                nnt = rnd(1.0 - float(truncated[t][e]))
                next_v = float(last_values[e]) if t == steps - 1 else float(values[t + 1][e])
                delta = rnd(rnd(r + rnd(rnd(g * next_v) * nnt)) - float(values[t][e]))
                last = rnd(delta + rnd(rnd(gl * nnt) * last))
                advantages[t][e] = last
                returns[t][e] = rnd(last + float(values[t][e]))
    return np.array(advantages, dtype=F32), np.array(returns, dtype=F32)


# ---- 1: the arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bootstrap", [True, False])
@pytest.mark.parametrize("truncation", cases.TRUNCATIONS)
@pytest.mark.parametrize("steps,n", [(1, 1), (2, 3), (5, 64), (33, 65), (128, 8)])
def test_gae_numpy_equals_the_scalar_restatement(steps, n, truncation, bootstrap):
    """On the hostile inputs the kernel gets (zeros of either sign, infinities, subnormals, rewards float32 cannot
    hold, NaN final_values wherever the step did not end), as bytes."""
    rewards, values, truncated, final_values, last_values = cases.synthetic(steps, n, truncation, 7 * steps + n)
    final_values = final_values if bootstrap else None
    got = rollout.gae_numpy(rewards, values, truncated, final_values, last_values, cases.GAMMA, cases.GAE_LAMBDA)
    want = restated(rewards, values, truncated, final_values, last_values, cases.GAMMA, cases.GAE_LAMBDA)
    assert got[0].dtype == F32 and got[1].dtype == F32 and got[0].shape == (steps, n)
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])


def test_synthetic_inputs_hold_what_they_promise():
    rewards, values, truncated, final_values, _ = cases.synthetic(33, 65, "random", 3)
    raw = values.view(np.uint32)
    for special in (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001):  # +-0, +-inf, the least subnormal
        assert (raw == special).any(), hex(special)
    with np.errstate(over="ignore"):
        assert (rewards.astype(F32).astype(np.float64) != rewards).any()  # (not representable)
    assert np.isnan(final_values[truncated == 0]).all() and not np.isnan(final_values[truncated == 1]).any()
    assert 0 < truncated.sum() < truncated.size


def test_known_answers():
    """T = 2, n = 1, gamma = 0.5, lambda = 0.5 (g = 0.5, gl = 0.25), rewards 1 and 2, values 0.5 and 0.25, last 0.125.
    t = 1: delta = 2 + 0.5 * 0.125 - 0.25 = 1.8125 = last; t = 0: delta = 1 + 0.5 * 0.25 - 0.5 = 0.625,
    last = 0.625 + 0.25 * 1.8125 = 1.078125.  With truncated[0] = 1 and V(final) = 2: r = 1 + 0.5 * 2 = 2,
    delta = 2 - 0.5 = 1.5 = last (nothing crosses the boundary)."""
    rewards, values, last = np.array([[1.0], [2.0]]), np.array([[0.5], [0.25]], dtype=F32), np.array([0.125], dtype=F32)
    none = np.zeros((2, 1), dtype=np.uint8)
    advantages, returns = rollout.gae_numpy(rewards, values, none, None, last, 0.5, 0.5)
    assert advantages.tolist() == [[1.078125], [1.8125]] and returns.tolist() == [[1.578125], [2.0625]]
    first = np.array([[1], [0]], dtype=np.uint8)
    final = np.array([[2.0], [np.nan]], dtype=F32)
    advantages, returns = rollout.gae_numpy(rewards, values, first, final, last, 0.5, 0.5)
    assert advantages.tolist() == [[1.5], [1.8125]] and returns.tolist() == [[2.0], [2.0625]]
    # without the bootstrap the truncated step only cuts the chain: delta = 1 - 0.5
    advantages, _ = rollout.gae_numpy(rewards, values, first, None, last, 0.5, 0.5)
    assert advantages.tolist() == [[0.5], [1.8125]]


def test_nan_final_values_of_steps_that_did_not_end_never_reach_the_result():
    rewards, values, truncated, final_values, last_values = cases.synthetic(33, 65, "random", 11)
    with np.errstate(over="ignore"):
        finite = np.isfinite(values).all(axis=0) & np.isfinite(rewards.astype(F32)).all(axis=0) & np.isfinite(last_values)
    assert finite.sum() >= 5 and (truncated[:, finite] == 0).any() and (truncated[:, finite] == 1).any()
    got = rollout.gae_numpy(rewards, values, truncated, final_values, last_values, 0.99, 0.95)
    assert not np.isnan(got[0][:, finite]).any() and not np.isnan(got[1][:, finite]).any()
    other = np.where(truncated == 0, F32(123.0), final_values)  # whatever stands there changes nothing
    again = rollout.gae_numpy(rewards, values, truncated, other, last_values, 0.99, 0.95)
    assert bits(got[0]) == bits(again[0]) and bits(got[1]) == bits(again[1])


def test_gl_is_the_float32_of_the_float64_product():
    gamma, gae_lambda = cases.GAMMA, cases.GAE_LAMBDA  # (0.99 and 0.95 would not tell: both roundings agree there)
    one, two = F32(gamma * gae_lambda), F32(gamma) * F32(gae_lambda)
    assert type(two) is F32 and one != two  # (the pair tells the two definitions apart)
    rewards, values, last = np.zeros((2, 1)), np.zeros((2, 1), dtype=F32), np.array([1.0], dtype=F32)
    advantages, _ = rollout.gae_numpy(rewards, values, np.zeros((2, 1), dtype=np.uint8), None, last, gamma, gae_lambda)
    # t = 1: last = g; t = 0: last = 0 + gl * g
    assert advantages[0, 0] == one * F32(gamma) and advantages[0, 0] != two * F32(gamma)


# ---- 2: the twin buffer --------------------------------------------------------------------------------------------------
T = 7


def _twin(n, records=True, view=True, **kw):
    """TimeLimitEnder(3) | DivergingEnder, as tests/test_learner_view_logic.py's shapes"""
    kw = dict(max_episode_steps=3, num_envs=n, seed=31, frame_height=16, samples_per_pixel=1, episode_records=records,
              learner_view=harness.LearnerView(frame_stack=5) if view else None, **kw)
    return harness.VectorDiscreteSteps(**kw)


def _run(buffer, obs, first_step, records=True):
    for t in range(buffer.n_steps):
        values, log_probs = cases.policy(obs)
        obs, rewards, _, truncated, info = buffer.step(cases.index_schedule(first_step + t, buffer.num_envs), values,
                                                       log_probs)
        if records:
            buffer.bootstrap(info["final_observation"][:, 0] * 0.5)
    return obs


def test_twin_rollouts_carry_row_T_and_span_episodes(no_gpu):  # noqa: F811
    n = 5
    env = _twin(n)
    buffer = harness.Rollout(env, T)
    assert (buffer.gamma, buffer.gae_lambda) == (0.99, 0.95)
    assert buffer.observations.shape == (T + 1, n, 20) and buffer.observations.dtype == F32
    assert buffer.actions.dtype == np.int64 and buffer.rewards.dtype == np.float64 and buffer.truncated.dtype == np.uint8
    for name in ("values", "log_probs", "final_values", "advantages", "returns"):
        assert getattr(buffer, name).dtype == F32 and getattr(buffer, name).shape == (T, n)
    obs, _ = env.reset()
    buffer.start(obs)
    assert bits(buffer.observations[0]) == bits(obs)
    last_obs = _run(buffer, obs, 0)
    advantages, returns = buffer.finish(cases.policy(last_obs)[0])
    # a limit of 3 ends every environment in steps 2 and 5: the episode that began at step 6 spans the boundary
    assert buffer.truncated[[2, 5]].all() and not buffer.truncated[[0, 1, 3, 4, 6]].any()
    assert np.isnan(buffer.final_values[[0, 1, 3, 4, 6]]).all() and not np.isnan(buffer.final_values[[2, 5]]).any()
    want = rollout.gae_numpy(buffer.rewards, buffer.values, buffer.truncated, buffer.final_values,
                             cases.policy(last_obs)[0], 0.99, 0.95)
    assert bits(advantages) == bits(want[0]) and bits(returns) == bits(want[1]) and not np.isnan(advantages).any()
    # the last step did not end: its advantage holds last_values, not a reset's observation
    g = F32(0.99)
    delta = (buffer.rewards[6].astype(F32) + g * cases.policy(last_obs)[0]) - buffer.values[6]
    assert bits(advantages[6]) == bits(delta)
    first = {name: np.array(getattr(buffer, name)) for name in ("observations", "advantages")}
    state = env._state.copy()
    buffer.start()
    assert bits(buffer.observations[0]) == bits(first["observations"][T]) and bits(env._state) == bits(state)  # no reset
    last_obs = _run(buffer, buffer.observations[0], T)
    buffer.finish(cases.policy(last_obs)[0])
    assert buffer.truncated[[1, 4]].all() and buffer.truncated.sum() == 2 * n  # (global steps 8 and 11)
    assert bits(buffer.values[0]) == bits(first["observations"][T][:, 0] * F32(0.5))
    env.close()


@pytest.mark.parametrize("cls", ["VectorContinuousJumps", "VectorEnvironment"])
def test_twin_over_the_other_host_twins(cls, no_gpu):  # noqa: F811
    from tests import test_gpu_snapshot as gpu
    from tests.test_gpu_device_initializer import KW

    n = 4
    if cls == "VectorContinuousJumps":
        env = harness.VectorContinuousJumps(num_envs=n, episode_records=True, **cases.ENV_KW)
        action = lambda t: cases.jump_schedule(t, n)  # noqa: E731
    else:
        env = harness.VectorEnvironment(**gpu.stopped_objects(n), **KW)
        action = lambda t: cases.index_schedule(t, n)  # noqa: E731
    buffer = harness.Rollout(env, 3, gamma=0.9, gae_lambda=0.8)
    assert buffer.actions.dtype == (F32 if cls == "VectorContinuousJumps" else np.int64)
    obs, _ = env.reset()
    buffer.start(obs)
    for t in range(3):
        values, log_probs = cases.policy(obs)
        obs = buffer.step(action(t), values, log_probs)[0]
        assert bits(buffer.actions[t]) == bits(action(t)) and bits(buffer.observations[t + 1]) == bits(obs)
    advantages, returns = buffer.finish(cases.policy(obs)[0])
    want = rollout.gae_numpy(buffer.rewards, buffer.values, buffer.truncated, None, cases.policy(obs)[0], 0.9, 0.8)
    assert bits(advantages) == bits(want[0]) and bits(returns) == bits(want[1])
    env.close()


def test_flat_order_and_minibatches(no_gpu):  # noqa: F811
    n = 3
    env = _twin(n)
    buffer = harness.Rollout(env, T)
    obs, _ = env.reset()
    buffer.start(obs)
    with pytest.raises(ValueError, match="not finished"):
        buffer.flat()
    buffer.finish(cases.policy(_run(buffer, obs, 0))[0])
    flat = buffer.flat()
    assert sorted(flat) == sorted(rollout.FLAT_KEYS)
    assert flat["observations"].shape == (T * n, 20) and flat["returns"].shape == (T * n,)
    for e in range(n):
        for t in range(T):  # stable-baselines3's swap_and_flatten: index = e * T + t
            assert bits(flat["observations"][e * T + t]) == bits(buffer.observations[t, e])
            for key in rollout.FLAT_KEYS[1:]:
                assert bits(flat[key][e * T + t]) == bits(getattr(buffer, key)[t, e])
    batches = list(buffer.minibatches(4, np.random.default_rng(3)))
    assert [len(b["actions"]) for b in batches] == [4, 4, 4, 4, 4, 1]
    order = np.random.default_rng(3).permutation(T * n)
    assert sorted(order) == list(range(T * n))
    for key in rollout.FLAT_KEYS:  # every index once, by one permutation
        assert bits(np.concatenate([b[key] for b in batches])) == bits(flat[key][order])
    assert len(list(buffer.minibatches(100))) == 1
    env.close()


def test_refusals(no_gpu):  # noqa: F811
    n = 3
    env = _twin(n)
    buffer = harness.Rollout(env, 2)
    values = np.zeros(n, dtype=F32)
    with pytest.raises(ValueError, match="start"):
        buffer.step(cases.index_schedule(0, n), values, values)
    with pytest.raises(ValueError, match="none has been finished"):
        buffer.start()
    obs, _ = env.reset()
    buffer.start(obs)
    with pytest.raises(ValueError, match="no step was taken"):
        buffer.bootstrap(values)
    buffer.step(cases.index_schedule(0, n), values, values)
    buffer.bootstrap(values)
    with pytest.raises(ValueError, match="bootstrapped already"):
        buffer.bootstrap(values)
    with pytest.raises(ValueError, match="1 of its 2 steps"):
        buffer.finish(values)
    buffer.step(cases.index_schedule(1, n), values, values)
    with pytest.raises(ValueError, match="already holds its 2 steps"):  # too many steps
        buffer.step(cases.index_schedule(2, n), values, values)
    with pytest.raises(ValueError, match="1 of the rollout's 2 steps"):  # a partial bootstrap
        buffer.finish(values)
    buffer.bootstrap(values)
    buffer.finish(values)
    env.close()
    plain = _twin(n, records=False)
    buffer = harness.Rollout(plain, 2)
    buffer.start(plain.reset()[0])
    buffer.step(cases.index_schedule(0, n), values, values)
    with pytest.raises(ValueError, match="episode_records=True"):  # bootstrap without records
        buffer.bootstrap(values)
    with pytest.raises(TypeError, match="device-resident"):
        harness.DeviceRollout(plain, 2)
    with pytest.raises(ValueError, match="n_steps"):
        harness.Rollout(plain, 0)
    plain.close()


def test_import_stays_free_of_torch():
    import subprocess
    import sys

    code = "import sys; from reinfocus_amd.environments import harness; harness.Rollout; assert 'torch' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


# ---- 3: the seeds of the GPU file ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("steps", n) for n in cases.E2E_SIZES] + [("jumps", 65), ("no-records", 65)])
def test_seeds_of_the_gpu_tests_end_environments_inside_a_rollout_and_on_its_last_step(kind, n, no_gpu):  # noqa: F811
    """tests/test_gpu_rollout.py, end to end: the enders read the states only, so the ends seen here with a stand-in
    observer are the GPU's.  Every rollout ends some environment before its last step, and one of the rollouts ends one
    on its last step -- where `dones` of the definition is 1 and last_values must not be read into the advantage."""
    runs = cases.twin_run(kind, n)
    assert len(runs) == cases.ROLLOUTS
    ended = [run["truncated"].astype(bool) for run in runs]
    assert all(flags[:cases.T - 1].any() for flags in ended), [flags.sum(axis=1).tolist() for flags in ended]
    assert any(flags[cases.T - 1].any() for flags in ended), [flags.sum(axis=1).tolist() for flags in ended]
    if n > 1:
        assert any(0 < k < n for flags in ended for k in flags.sum(axis=1))  # (a part of the environments)
    if cases.E2E_KINDS[kind]["records"]:
        for run in runs:
            assert bits(np.isnan(run["final_values"])) == bits(run["truncated"] == 0)
    assert bits(runs[1]["observations"][0]) == bits(runs[0]["observations"][cases.T])


# ---- 4: the binding --------------------------------------------------------------------------------------------------------
def test_binding_argtypes_match_the_header():
    text = open(os.path.join(ROOT, "include", "reinfocus_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"\bint\s+rf_rollout_advantages\s*\((.*?)\)\s*;", text, flags=re.S)
    assert declaration, "rf_rollout_advantages is not declared"
    wanted = []
    for parameter in declaration.group(1).split(","):
        parameter = " ".join(parameter.split())
        if "*" in parameter:
            wanted.append(ctypes.c_void_p)
        else:
            wanted.append({"int": ctypes.c_int, "double": ctypes.c_double}[parameter.rsplit(" ", 1)[0]])
    assert len(wanted) == 13 and "rf_rollout_advantages" in _native.SYMBOLS
    pattern = r"lib\.rf_rollout_advantages\.argtypes = \[(.*?)\]"
    source = open(os.path.join(ROOT, "reinfocus_amd", "_native.py")).read()
    names = [name.strip() for name in re.search(pattern, source).group(1).split(",")]
    alias = {"vp": ctypes.c_void_p, "i32": ctypes.c_int, "ctypes.c_double": ctypes.c_double}
    assert [alias[name] for name in names] == wanted


def test_chunk_length_of_the_gpu_shapes_is_the_kernels():
    text = open(os.path.join(ROOT, "reinfocus_amd", "csrc", "rf_rollout.h")).read()
    assert int(re.search(r"constexpr int kRolloutChunk = (\d+);", text).group(1)) == cases.CHUNK
    assert int(re.search(r"constexpr int kRolloutTile = (\d+);", text).group(1)) == 64
    assert (cases.CHUNK + 1, 1100) in cases.KERNEL_SHAPES
