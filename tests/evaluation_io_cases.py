"""TEST INFRASTRUCTURE: what tests/test_evaluation_logic.py and tests/test_gpu_evaluation.py share -- the synthetic record
streams, the scenario runner over three backends (the numpy twin, the host build tests/evalcheck, the device), the twin's
results (computed once and shared, never changed) -- and the child process of the GPU file.

As tests/param_init_io_cases.py: everything that needs torch and the library together runs in one fresh process that
imports torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.evaluation_io_cases <results.jsonl>
"""

import ctypes
import functools
import os
import sys
import types

import numpy as np

from tests import policy_io_cases as policy_cases
from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = policy_cases.bits
FILL = 0xA7  # the byte every output holds before a call (float64 0xA7A7...: a negative number no stream produces)
GUARD = 16  # guard bytes on either side of an output on the device

# (G, m, E): the matrix of the issue, then K = 100 with more leaves than the block has threads, E = 257 (one leaf past a
# full block), and E = 1
SHAPES = tuple((G, m, E) for G in (1, 3) for m in (3, 8, 11) for E in (2, 5, 20)) + ((3, 3, 300), (1, 8, 257), (3, 8, 1))
# the evaluations of a scenario, in a row over the same best_*: every lane ends every step; the same records again (a
# tie: no group improves); the same plus 10 (every group improves); lanes that end at random; the last group's lanes
# never end (incomplete); then four rotations of the special values
KINDS = ("all", "tie", "higher", "some", "never", "special0", "special1", "special2", "special3")
SPECIALS = ((np.nan, 1.5, -2.5), (np.inf, -np.inf, 3.0), (-0.0, 0.0), (np.inf, 7.0))
KEYS = ("counts", "returns", "lengths", "results", "best_mean", "best_serial", "improved")


def shape_id(shape):
    return "G%d-m%d-E%d" % shape


def stream(kind, shape, index):
    """(final_return float64 [steps][n], final_length int32 [steps][n]) of one evaluation: what the step's episode
    records would hold (NaN / 0 where no episode ended)."""
    G, m, E = shape
    n, K = G * m, (E + m - 1) // m
    seed = [G, m, E, 0 if kind in ("all", "tie", "higher") else index]
    rng = np.random.default_rng(seed)
    steps = 4 * K + 4 if kind == "some" else K + 1
    returns = 10.0 * rng.standard_normal((steps, n))
    lengths = rng.integers(1, 50, size=(steps, n)).astype(np.int32)
    ended = np.ones((steps, n), dtype=bool)
    if kind == "higher":
        returns = returns + 10.0
    elif kind == "some":
        ended = rng.random((steps, n)) < 0.6
    elif kind == "never":
        ended[:, (G - 1) * m:] = False
    elif kind.startswith("special"):
        for g in range(G):
            values = np.array(SPECIALS[(g + int(kind[-1])) % len(SPECIALS)], dtype=np.float64)
            returns[:, g * m:(g + 1) * m] = values[rng.integers(len(values), size=(steps, m))]
            returns[0, g * m:(g + 1) * m] = np.resize(values, m)  # (every special value where E allows)
    returns = np.where(ended, returns, np.nan)
    lengths = np.where(ended, lengths, 0).astype(np.int32)
    return np.ascontiguousarray(returns, dtype=np.float64), lengths


def filled(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, dtype=np.uint8).view(dtype).reshape(shape)


def scenario(backend, shape):
    """The evaluations KINDS in a row through `backend` (twin_backend, host_backend or a device one): per evaluation the
    seven arrays KEYS as bits.  Tables and rows start as FILL bytes, counts as zeros, best_mean at -inf, best_serial at 0."""
    G, m, E = shape
    n, K = G * m, (E + m - 1) // m
    state = backend.begin(G, m, E, n, K)
    seen = []
    for index, kind in enumerate(KINDS):
        final_returns, final_lengths = stream(kind, shape, index)
        seen.append(backend.evaluate(state, G, m, E, index + 1, final_returns, final_lengths))
    return seen


class twin_backend:
    @staticmethod
    def begin(G, m, E, n, K):
        return dict(counts=np.zeros(n, dtype=np.int32), returns=filled((n, K), np.float64), lengths=filled((n, K), np.int32),
                    best_mean=np.full(G, -np.inf), best_serial=np.zeros(G, dtype=np.int64))

    @staticmethod
    def evaluate(state, G, m, E, serial, final_returns, final_lengths):
        from reinfocus_amd.environments import evaluation

        state["counts"][:] = 0
        for final_return, final_length in zip(final_returns, final_lengths):
            evaluation.accumulate_numpy(state["counts"], state["returns"], state["lengths"], final_return, final_length, m, E)
        state["results"], state["improved"] = evaluation.finish_numpy(
            state["counts"], state["returns"], state["lengths"], G, m, E, serial, state["best_mean"], state["best_serial"])
        return {key: bits(state[key]) for key in KEYS}


def hostcheck():
    from tests import helpers

    lib = ctypes.CDLL(helpers.built("tests/evalcheck", "libevalcheck.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.evc_target.argtypes = lib.evc_first.argtypes = [i32, i32, i32]
    lib.evc_slots.argtypes = [i32, i32]
    lib.evc_leaves.argtypes = [i32]
    lib.evc_locate.argtypes = [i32, i32, i32, vp]
    lib.evc_accumulate.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
    lib.evc_finish.argtypes = [i32, i32, i32, ctypes.c_ulonglong] + [vp] * 7
    return lib


def _p(array):
    return array.ctypes.data_as(ctypes.c_void_p)


class host_backend:
    def __init__(self, lib):
        self._lib = lib

    def begin(self, G, m, E, n, K):
        state = twin_backend.begin(G, m, E, n, K)
        state.update(results=filled((G, 8), np.float64), improved=filled((G,), np.uint8))
        return state

    def evaluate(self, state, G, m, E, serial, final_returns, final_lengths):
        state["counts"][:] = 0
        for final_return, final_length in zip(final_returns, final_lengths):
            self._lib.evc_accumulate(G, m, E, _p(final_return), _p(final_length), _p(state["counts"]), _p(state["returns"]),
                                     _p(state["lengths"]))
        self._lib.evc_finish(G, m, E, serial, _p(state["counts"]), _p(state["returns"]), _p(state["lengths"]),
                             _p(state["results"]), _p(state["best_mean"]), _p(state["best_serial"]), _p(state["improved"]))
        return {key: bits(state[key]) for key in KEYS}


@functools.lru_cache(maxsize=None)
def twin_scenario(shape):
    """scenario(twin_backend, shape): computed once per shape, shared, read-only."""
    return scenario(twin_backend, shape)


def first_difference(got, want):
    """None, or which evaluation and array of two scenario results differ."""
    for index, (a, b) in enumerate(zip(got, want)):
        for key in KEYS:
            if a[key] != b[key]:
                x, y = (np.frombuffer(r[key][2], dtype=np.dtype(r[key][0])) for r in (a, b))
                return f"evaluation {index} ({KINDS[index]}), {key}: {x!r} for {y!r}"
    return None


# ---- the environments and policies of the end-to-end runs (twin and device) ----------------------------------------------
E2E = dict(groups=3, per_group=3, episodes=5, max_steps=11, stack=2, warm=4)
E2E_KINDS = ("mlp", "sde", "lstm", "lstm-sde")
SEEDS, OTHER_SEEDS = (3, 2 ** 70 + 5, 11), (21, 22, 23)
LOG_STD = (-1.0, -0.5, -2.0)


def e2e_env(kind, device_form, training, n=None, records=True, view="grouped", seed=1, **extra):
    from reinfocus_amd.environments import harness

    jumps = kind in ("sde", "lstm-sde")
    n = E2E["groups"] * E2E["per_group"] if n is None else n
    kw = dict(rollout_cases.ENV_KW, seed=seed, episode_records=records)
    if view == "grouped":
        kw["learner_view"] = harness.LearnerView(frame_stack=E2E["stack"], groups=E2E["groups"], training=training)
    elif view is not None:
        kw["learner_view"] = view
    kw.update(extra)
    if device_form:
        cls = harness.DeviceVectorContinuousJumps if jumps else harness.DeviceVectorDiscreteSteps
        kw.setdefault("device_initializer", True)
        return cls(num_envs=n, **kw)
    cls = harness.VectorContinuousJumps if jumps else harness.VectorDiscreteSteps
    return cls(num_envs=n, **kw)


def e2e_spec(kind, env):
    from reinfocus_amd.environments import harness

    width = int(env.single_observation_space.shape[0])
    if kind == "mlp":
        return harness.MlpPolicySpec(width, int(env.single_action_space.n), pi=(7,), vf=(3, 2))
    if kind == "sde":
        return harness.SdePolicySpec(width, pi=(7,), vf=(3, 2), log_std_init=-2.0)
    if kind == "lstm":
        return harness.LstmPolicySpec(width, int(env.single_action_space.n), lstm_hidden=9, pi=(6,), vf=(5, 7))
    return harness.LstmSdePolicySpec(width, lstm_hidden=9, pi=(6,), vf=(5, 7), log_std_init=-2.0)


def e2e_policy(kind, env, spec, device_form):
    from reinfocus_amd.environments import harness

    G, n = E2E["groups"], E2E["groups"] * E2E["per_group"]
    kw = dict(log_std_init=list(LOG_STD)) if kind in ("sde", "lstm-sde") else {}
    if device_form:
        cls = {"mlp": harness.DevicePopulationPolicy, "sde": harness.DeviceSdePopulationPolicy,
               "lstm": harness.DevicePopulationLstmPolicy, "lstm-sde": harness.DevicePopulationLstmSdePolicy}[kind]
        policy = cls(env, spec, G, [1, 2, 3], **kw)
    else:
        if kind in ("lstm", "lstm-sde"):
            kw["num_envs"] = n
        cls = {"mlp": harness.PopulationPolicy, "sde": harness.SdePopulationPolicy, "lstm": harness.LstmPopulationPolicy,
               "lstm-sde": harness.LstmSdePopulationPolicy}[kind]
        policy = cls(spec, G, [1, 2, 3], **kw)
    policy.init_parameters(list(SEEDS), False)
    return policy


def e2e_warm(kind, env, policy, device_form, wrap):
    """A few scheduled steps of the training environment (its statistics move), then what gives the policy a noise, an
    LSTM state and generators that have drawn: reset_noise and one sampled act()."""
    n = env.num_envs
    jumps = kind in ("sde", "lstm-sde")
    obs = (env.reset_tensors() if device_form else env.reset())[0]
    for t in range(E2E["warm"]):
        actions = rollout_cases.jump_schedule(t, n) if jumps else rollout_cases.index_schedule(t, n) % 3
        obs = (env.step_tensors(wrap(actions)) if device_form else env.step(actions))[0]
    if jumps:
        policy.reset_noise(num_envs=n)
    if kind in ("lstm", "lstm-sde"):
        policy.act(obs, wrap(np.ones(n, dtype=np.uint8)))
    else:
        policy.act(obs)


def e2e_snapshot(kind, policy, unwrap):
    """rng_state(), noise() and lstm_state() of a policy, as far as its head has them."""
    seen = {"rng": policy.rng_state()}
    if kind in ("sde", "lstm-sde"):
        seen["noise"] = bits(unwrap(policy.noise()))
    if kind in ("lstm", "lstm-sde"):
        seen["lstm"] = bits(unwrap(policy.lstm_state()))
    return seen


def e2e_everything(evaluation, unwrap):
    seen = {key: bits(unwrap(getattr(evaluation, key))) for key in
            ("counts", "returns", "lengths", "improved", "best_mean", "best_serial", "best_params", "best_statistics")}
    seen["results"] = bits(evaluation.results())
    seen["params"] = bits(unwrap(evaluation.policy.params))
    return seen


def e2e_script(kind, device_form, wrap, unwrap):
    """The end-to-end run of one head, twin or device: warm up, evaluate, change the parameters of groups 0 and 2,
    evaluate again, load_best((0, 1, 1)).  Returns what was seen after each stage."""
    from reinfocus_amd.environments import harness

    train_env, eval_env = e2e_env(kind, device_form, True), e2e_env(kind, device_form, False, seed=5)
    try:
        spec = e2e_spec(kind, train_env)
        policy = e2e_policy(kind, train_env, spec, device_form)
        e2e_warm(kind, train_env, policy, device_form, wrap)
        before = e2e_snapshot(kind, policy, unwrap)
        cls = harness.DeviceEvaluation if device_form else harness.Evaluation
        evaluation = cls(eval_env, policy, n_eval_episodes=E2E["episodes"], train_env=train_env)
        seen = {}
        evaluation.run(E2E["max_steps"])
        seen["first"] = e2e_everything(evaluation, unwrap)
        seen["synced"] = bits(unwrap(train_env.view_statistics_tensor())) == bits(unwrap(eval_env.view_statistics_tensor()))
        policy.init_parameters(list(OTHER_SEEDS), False, groups=[True, False, True])
        evaluation.run(E2E["max_steps"])
        seen["second"] = e2e_everything(evaluation, unwrap)
        evaluation.load_best(groups=[False, True, True])
        seen["loaded"] = bits(unwrap(policy.params))
        seen["untouched"] = e2e_snapshot(kind, policy, unwrap) == before
        kept = evaluation.state_dict()
        other = cls(eval_env, policy, n_eval_episodes=E2E["episodes"], train_env=train_env)
        other.load_state_dict(kept)
        seen["resumed"] = all(bits(unwrap(getattr(other, key))) == bits(unwrap(getattr(evaluation, key)))
                              for key in ("best_params", "best_mean", "best_serial", "best_statistics")) \
            and other.serial == evaluation.serial == 2
        return seen
    finally:
        train_env.close()
        eval_env.close()


@functools.lru_cache(maxsize=None)
def e2e_twin(kind):
    return e2e_script(kind, False, lambda a: a, np.array)


def e2e_promises(seen):
    """What the two runs promise whatever the numbers are: the better mean is kept group-wise, with its parameters, and
    load_best restores only the selected groups."""
    unpack = lambda b: np.frombuffer(b[2], dtype=np.dtype(b[0])).reshape(b[1])  # noqa: E731
    first, second = seen["first"], seen["second"]
    rows1, rows2 = unpack(first["results"]), unpack(second["results"])
    assert (rows1[:, 6] == 0).all() and (rows2[:, 6] == 0).all(), "a group was not done within max_steps"
    assert (rows1[:, 5] == E2E["episodes"]).all() and (rows1[:, 7] == 1).all() and (rows2[:, 7] == 2).all()
    assert (unpack(first["improved"]) == 1).all() and bits(unpack(first["best_mean"])) == bits(rows1[:, 0])
    assert first["best_params"] == first["params"]
    better = rows2[:, 0] > rows1[:, 0]
    assert bits(unpack(second["improved"])) == bits(better.astype(np.uint8))
    assert bits(unpack(second["best_mean"])) == bits(np.where(better, rows2[:, 0], rows1[:, 0]))
    assert bits(unpack(second["best_serial"])) == bits(np.where(better, 2, 1).astype(np.int64))
    params1, params2 = unpack(first["params"]), unpack(second["params"])
    assert bits(params1[1]) == bits(params2[1]) and bits(params1[0]) != bits(params2[0])
    best = unpack(second["best_params"])
    for g in range(E2E["groups"]):
        assert bits(best[g]) == bits((params2 if better[g] else params1)[g]), f"group {g}"
    loaded = unpack(seen["loaded"])
    assert bits(loaded[0]) == bits(params2[0]) and bits(loaded[1:]) == bits(best[1:])
    assert seen["synced"] and seen["untouched"] and seen["resumed"]


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
def _guarded(torch, shape, dtype, fill=FILL):
    """A tensor of `shape` and `dtype` of FILL bytes between two guards of GUARD bytes: (whole uint8, the view)."""
    size = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((GUARD + size + GUARD,), fill, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + size].view(dtype).view(*shape)


def _guards_kept(whole):
    raw = whole.cpu().numpy()
    return bool((raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all())


class device_backend:
    def __init__(self, torch, ctx):
        self._torch, self._ctx = torch, ctx
        self._stream = torch.cuda.current_stream().cuda_stream

    def begin(self, G, m, E, n, K):
        torch = self._torch
        state = {}
        for key, shape, dtype in (("counts", (n,), torch.int32), ("returns", (n, K), torch.float64),
                                  ("lengths", (n, K), torch.int32), ("results", (G, 8), torch.float64),
                                  ("best_mean", (G,), torch.float64), ("best_serial", (G,), torch.int64),
                                  ("improved", (G,), torch.uint8)):
            state["whole_" + key], state[key] = _guarded(torch, shape, dtype)
        state["best_mean"].fill_(float("-inf"))
        state["best_serial"].zero_()
        return state

    def evaluate(self, state, G, m, E, serial, final_returns, final_lengths):
        torch, ctx, n = self._torch, self._ctx, G * m
        state["counts"].zero_()
        returns, lengths = torch.from_numpy(final_returns).cuda(), torch.from_numpy(final_lengths).cuda()
        for step in range(final_returns.shape[0]):
            ctx.eval_accumulate(n, G, m, E, returns[step].data_ptr(), lengths[step].data_ptr(), state["counts"].data_ptr(),
                                state["returns"].data_ptr(), state["lengths"].data_ptr(), self._stream)
        ctx.eval_finish(n, G, m, E, serial, state["counts"].data_ptr(), state["returns"].data_ptr(),
                        state["lengths"].data_ptr(), state["results"].data_ptr(), state["best_mean"].data_ptr(),
                        state["best_serial"].data_ptr(), state["improved"].data_ptr(), self._stream)
        torch.cuda.synchronize()
        for key in KEYS:
            assert _guards_kept(state["whole_" + key]), f"a guard of {key} was written"
        return {key: bits(state[key].cpu().numpy()) for key in KEYS}


def kernel_case(torch, ctx, shape):
    wrong = first_difference(scenario(device_backend(torch, ctx), shape), twin_scenario(shape))
    assert wrong is None, wrong


KEEP_MASKS = ((1, 0, 1), (0, 0, 0), (1, 1, 1))
KEEP_WORDS = (1, 3, 4, 1023, 1028)  # the dword tail alone, below one vector, one vector, an odd stride, a second block


def keep_rows_case(torch, ctx, words):
    """rf_eval_keep_rows at G = 3 for the three masks: rows `words` words long and as far apart (an odd stride leaves rows
    1 and 2 off a 16-byte boundary), and in a stride of words + 5; selected rows are the source's bytes, unselected rows,
    the gaps between rows and the guards keep theirs."""
    G = 3
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(words)
    for stride in (words, words + 5):
        cells = (G - 1) * stride + words
        source = torch.from_numpy(rng.integers(0, 2 ** 31, size=cells).astype(np.int32)).cuda()
        for mask in KEEP_MASKS:
            select = torch.tensor(mask, dtype=torch.uint8, device="cuda")
            for shift in (0, 1):  # (a destination one word off the source's alignment: the dword form)
                whole, inside = _guarded(torch, (cells + shift,), torch.int32)
                target = inside[shift:]
                ctx.eval_keep_rows(G, words, stride, select.data_ptr(), source.data_ptr(), target.data_ptr(), stream)
                torch.cuda.synchronize()
                assert _guards_kept(whole), f"stride {stride}, mask {mask}: a guard was written"
                got, want = target.cpu().numpy(), filled((cells,), np.int32)
                for g in range(G):
                    if mask[g]:
                        want[g * stride:g * stride + words] = source.cpu().numpy()[g * stride:g * stride + words]
                assert bits(got) == bits(want), f"stride {stride}, mask {mask}, shift {shift}"


def statistics_case(torch, grouped):
    """rf_env_view_get / set_statistics_device against view_statistics(), as bytes, after steps that moved the moments."""
    from reinfocus_amd.environments import harness

    G = 3 if grouped else None
    view = harness.LearnerView(frame_stack=2, groups=G)
    env = e2e_env("mlp", True, True, view=view)
    other = e2e_env("mlp", True, False, view=harness.LearnerView(frame_stack=2, groups=G, training=False), seed=9)
    try:
        n = env.num_envs
        env.reset_tensors()
        for t in range(3):
            env.step_tensors(torch.from_numpy(rollout_cases.index_schedule(t, n) % 3).cuda())
        want = env.view_statistics()
        stacked = np.stack([want[key] for key in ("mean", "var", "count")], axis=-2)
        whole, inside = _guarded(torch, stacked.shape, torch.float64)
        assert env.view_statistics_tensor(out=inside) is inside
        torch.cuda.synchronize()
        assert _guards_kept(whole) and bits(inside.cpu().numpy()) == bits(stacked)
        assert bits(env.view_statistics_tensor().cpu().numpy()) == bits(stacked)
        assert bits(np.stack([other.view_statistics()[key] for key in ("mean", "var", "count")], axis=-2)) != bits(stacked)
        other.set_view_statistics_tensor(inside)
        got = other.view_statistics()
        assert all(bits(got[key]) == bits(want[key]) for key in want)
        for wrong, error in ((inside.float(), ValueError), (inside.cpu(), ValueError), (inside[..., :-1], ValueError),
                             (stacked, TypeError)):
            try:
                other.set_view_statistics_tensor(wrong)
            except error as refusal:
                assert str(refusal)
            else:
                raise AssertionError("not refused")
    finally:
        env.close()
        other.close()


def kernel_refusal_case(torch, ctx):
    """What the entry points refuse, each with a message and nothing written."""
    G, m, E = 2, 3, 5
    n, K = 6, 2
    state = device_backend(torch, ctx).begin(G, m, E, n, K)
    returns = torch.zeros(n, dtype=torch.float64, device="cuda")
    lengths = torch.ones(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda key: state[key].data_ptr()  # noqa: E731

    def refused(words, call):
        try:
            call()
        except AssertionError as error:
            assert words in str(error), (words, str(error))
            return
        raise AssertionError(f"not refused: {words}")

    def accumulate(n=n, G=G, m=m, E=E, final_return=returns.data_ptr(), counts=None, table=None):
        ctx.eval_accumulate(n, G, m, E, final_return, lengths.data_ptr(), p("counts") if counts is None else counts,
                            p("returns") if table is None else table, p("lengths"), stream)

    def finish(n=n, G=G, m=m, E=E, serial=1, results=None):
        ctx.eval_finish(n, G, m, E, serial, p("counts"), p("returns"), p("lengths"), p("results") if results is None else
                        results, p("best_mean"), p("best_serial"), p("improved"), stream)

    for call in (accumulate, finish):
        refused("at least 1", lambda: call(E=0))
        refused("RF_EVAL_MAX_EPISODES", lambda: call(E=65537))
        refused("is not G m", lambda: call(n=7))
        refused("is not G m", lambda: call(G=0, n=0))
    refused("NULL", lambda: accumulate(final_return=None))
    refused("d_final_return is not device memory", lambda: accumulate(final_return=returns.cpu().data_ptr()))
    refused("d_returns overlaps d_final_return", lambda: accumulate(table=returns.data_ptr(), E=1, m=6, G=1))
    refused("not aligned", lambda: accumulate(counts=state["whole_counts"].data_ptr() + 1))
    refused("fewer than", lambda: accumulate(n=2 ** 25, m=2 ** 24))  # (past any block the allocator hands small tensors from)
    refused("d_results overlaps d_returns", lambda: finish(results=p("returns"), E=20, m=1, G=6))
    refused("2^53", lambda: finish(serial=2 ** 53))
    select = torch.ones(2, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(8, dtype=torch.int32, device="cuda")

    def keep(G=2, words=4, stride=4, src=rows.data_ptr(), dst=p("returns")):
        ctx.eval_keep_rows(G, words, stride, select.data_ptr(), src, dst, stream)

    refused("words = 0", lambda: keep(words=0))
    refused("words = 5", lambda: keep(words=5))
    refused("G = 0", lambda: keep(G=0))
    refused("d_dst overlaps d_src", lambda: keep(dst=rows.data_ptr() + 8, stride=2, words=2))
    refused("fewer than", lambda: keep(G=2, words=2 ** 22, stride=2 ** 22))
    from tests import population_lstm_io_cases as lstm_pop

    def captured(call):
        def attempt(capturing):
            try:
                call(capturing)
            except AssertionError as error:
                return str(error)
            return None
        message = lstm_pop._capturing(torch, attempt)
        assert message is not None and "being captured" in message, message

    captured(lambda s: ctx.eval_keep_rows(2, 4, 4, select.data_ptr(), rows.data_ptr(), p("returns"), s))
    captured(lambda s: ctx.eval_accumulate(n, G, m, E, returns.data_ptr(), lengths.data_ptr(), p("counts"), p("returns"),
                                           p("lengths"), s))
    captured(lambda s: ctx.eval_finish(n, G, m, E, 1, p("counts"), p("returns"), p("lengths"), p("results"), p("best_mean"),
                                       p("best_serial"), p("improved"), s))
    torch.cuda.synchronize()
    for key in ("returns", "lengths", "results", "improved"):
        raw = state["whole_" + key].cpu().numpy()
        assert (raw == FILL).all(), f"{key} was written"


def e2e_case(torch, kind):
    got = e2e_script(kind, True, lambda a: torch.from_numpy(a).cuda(), lambda t: t.cpu().numpy())
    want = e2e_twin(kind)
    for stage in ("first", "second"):
        for key in want[stage]:
            assert got[stage][key] == want[stage][key], f"{stage} run, {key} differs from the twin"
    assert got["loaded"] == want["loaded"]
    e2e_promises(got)
    e2e_promises(want)


def _trained(torch, kind, with_evaluation):
    """The parameters after warm-up, [an evaluation,] one collect() and one train()."""
    from reinfocus_amd.environments import harness

    G, m, T = E2E["groups"], E2E["per_group"], 4
    train_env, eval_env = e2e_env(kind, True, True), e2e_env(kind, True, False, seed=5)
    try:
        policy = e2e_policy(kind, train_env, e2e_spec(kind, train_env), True)
        e2e_warm(kind, train_env, policy, True, lambda a: torch.from_numpy(a).cuda())
        if with_evaluation:
            harness.DeviceEvaluation(eval_env, policy, E2E["episodes"], train_env=train_env).run(E2E["max_steps"])
        learner = harness.DevicePopulationLearner(policy, learning_rate=1e-2)
        rollout = harness.DeviceRollout(train_env, T, rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA, groups=G)
        rollout.start(train_env.reset_tensors()[0])
        rollout.collect(policy)
        rng = np.random.default_rng(4)
        if kind in ("lstm", "lstm-sde"):
            learner.train(rollout, 1, 6, splits=rng.integers(m * T, size=(1, G)))
        else:
            permutations = np.stack([rng.permutation(m * T) for _ in range(G)])[None].astype(np.int64)
            learner.train(rollout, 1, 6, permutations=torch.from_numpy(permutations).cuda())
        return bits(policy.params.cpu().numpy()), train_env.device_fault()
    finally:
        train_env.close()
        eval_env.close()


def training_case(torch, kind):
    """A collect() and a train() after an evaluation give the parameters they give without it."""
    with_it, fault = _trained(torch, kind, True)
    without, _ = _trained(torch, kind, False)
    assert fault is None and with_it == without


def single_case(torch):
    """The ungrouped classes are G = 1: DevicePolicy over an ungrouped view equals the twin."""
    from reinfocus_amd.environments import harness

    seen = []
    for device_form in (False, True):
        view = lambda training: harness.LearnerView(frame_stack=2, training=training)  # noqa: E731
        train_env = e2e_env("mlp", device_form, True, n=5, view=view(True))
        eval_env = e2e_env("mlp", device_form, False, n=5, view=view(False), seed=5)
        try:
            spec = e2e_spec("mlp", train_env)
            policy = harness.DevicePolicy(train_env, spec, 3) if device_form else harness.Policy(spec, 3)
            policy.init_parameters(SEEDS[1], False)
            cls = harness.DeviceEvaluation if device_form else harness.Evaluation
            evaluation = cls(eval_env, policy, n_eval_episodes=7, train_env=train_env)
            evaluation.run(11)
            unwrap = (lambda t: t.cpu().numpy()) if device_form else np.array
            seen.append(e2e_everything(evaluation, unwrap))
        finally:
            train_env.close()
            eval_env.close()
    assert seen[0] == seen[1]
    rows = np.frombuffer(seen[0]["results"][2], dtype=np.float64).reshape(1, 8)
    assert rows[0, 5] == 7 and rows[0, 6] == 0


def surface_case(torch):
    """What DeviceEvaluation refuses, each with a message, before anything is enqueued: the parameters keep their bytes."""
    from reinfocus_amd.environments import harness

    train_env = e2e_env("mlp", True, True)
    made = [train_env]
    try:
        policy = e2e_policy("mlp", train_env, e2e_spec("mlp", train_env), True)
        kept = policy.params.clone()

        def env(**kw):
            made.append(e2e_env("mlp", True, False, seed=5, **kw))
            return made[-1]

        def refused(error, words, call):
            try:
                call()
            except error as refusal:
                assert words in str(refusal), (words, str(refusal))
                return
            raise AssertionError(f"not refused: {words}")

        good = env()
        refused(ValueError, "episode records", lambda: harness.DeviceEvaluation(env(records=False), policy))
        elsewhere = types.SimpleNamespace(spec=policy.spec, _io=policy._io, device=torch.device("cuda", 1),
                                          params=policy.params, groups=policy.groups, _torch=torch)
        refused(ValueError, "one GPU only", lambda: harness.DeviceEvaluation(good, elsewhere))
        refused(ValueError, "6 environments", lambda: harness.DeviceEvaluation(env(n=6, view=None), policy))
        refused(ValueError, "groups=9", lambda: harness.DeviceEvaluation(
            env(view=harness.LearnerView(frame_stack=E2E["stack"], groups=9, training=False)), policy))
        refused(ValueError, "width", lambda: harness.DeviceEvaluation(env(view=None), policy))
        refused(ValueError, "device_initializer", lambda: harness.DeviceEvaluation(env(device_initializer=False), policy))
        refused(ValueError, "action space", lambda: harness.DeviceEvaluation(
            e2e_env_made(made, "sde", view="grouped"), policy))
        refused(TypeError, "device-resident", lambda: harness.DeviceEvaluation(e2e_env_made(made, "mlp", device_form=False),
                                                                                policy))
        refused(TypeError, "device policy", lambda: harness.DeviceEvaluation(good, harness.PopulationPolicy(
            policy.spec, 3, [1, 2, 3])))
        for episodes, words in ((0, "at least 1"), (65537, "RF_EVAL_MAX_EPISODES"), (2.5, "not an integer")):
            refused(ValueError, words, lambda: harness.DeviceEvaluation(good, policy, n_eval_episodes=episodes))
        sharded = harness.ShardedVectorDiscreteSteps(num_envs=9, devices=[0], frame_height=16, samples_per_pixel=1, seed=1)
        made.append(sharded)
        refused(ValueError, "no *_tensors methods", lambda: harness.DeviceEvaluation(sharded, policy))
        evaluation = harness.DeviceEvaluation(good, policy, train_env=train_env)
        rows = evaluation._results.clone()
        refused(ValueError, "at least 1", lambda: evaluation.run(0))
        refused(ValueError, "deterministic=False", lambda: evaluation.run(5, deterministic=False))
        refused(ValueError, "boolean sequence", lambda: evaluation.load_best(groups=[True]))
        torch.cuda.synchronize()
        assert evaluation.serial == 0 and torch.equal(evaluation._results, rows)
        assert torch.equal(policy.params.view(torch.int32), kept.view(torch.int32))
    finally:
        for one in made:
            one.close()


def e2e_env_made(made, kind, device_form=True, **kw):
    made.append(e2e_env(kind, device_form, False, seed=5, **kw))
    return made[-1]


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    ctx = _native.Context(0)
    for shape in SHAPES:
        with record.case("kernel/" + shape_id(shape)):
            kernel_case(torch, ctx, shape)
    for words in KEEP_WORDS:
        with record.case(f"keep/{words}"):
            keep_rows_case(torch, ctx, words)
    with record.case("kernel-refusals"):
        kernel_refusal_case(torch, ctx)
    ctx.close()
    for grouped in (False, True):
        with record.case(f"statistics/{int(grouped)}"):
            statistics_case(torch, grouped)
    for kind in E2E_KINDS:
        with record.case(f"e2e/{kind}"):
            e2e_case(torch, kind)
        with record.case(f"training/{kind}"):
            training_case(torch, kind)
    with record.case("single"):
        single_case(torch)
    with record.case("surface"):
        surface_case(torch)
    with record.case("finished"):
        pass


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    run_cases(sys.argv[1])
