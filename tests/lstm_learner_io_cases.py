"""TEST INFRASTRUCTURE: what tests/test_lstm_learner_logic.py and tests/test_gpu_lstm_learner.py share -- the networks, the
sequence layouts, the minibatches, the numpy twin's results (computed once and shared), the drivers of the end-to-end
runs -- and the child process of the GPU file.

As tests/learner_io_cases.py: everything that needs torch and the library together runs in one fresh process that imports
torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.lstm_learner_io_cases <results.jsonl>
    python -m tests.lstm_learner_io_cases --torch-lstm-learner <in.npz> <out.npz>   (torch on the CPU: autograd, Adam)
"""

import ctypes
import functools
import os
import sys

import numpy as np

from tests import learner_io_cases as learner_cases
from tests import lstm_io_cases as lstm_cases
from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = lstm_cases.TILE
NETWORKS = lstm_cases.NETWORKS
LIMITS = len(NETWORKS) - 1  # the network with every limit at once: the smallest layouts only
TUNED, DEFAULT = lstm_cases.TUNED, lstm_cases.DEFAULT
STEPS, ENVS = 5, 3
ROWS = STEPS * ENVS
UPDATES = learner_cases.UPDATES
SHIFTS = learner_cases.SHIFTS
hyper_of = learner_cases.hyper_of
bits = lstm_cases.bits
spec_of = lstm_cases.spec_of
SENTINEL = learner_cases.SENTINEL

# name -> (n_steps, num_envs, starts kind, first, B): every B with every first on the mixed starts; every row a start; one
# sequence that spans the whole minibatch (longer than a tile)
LAYOUTS = {f"mixed/{first}/{count}": (STEPS, ENVS, "mixed", first, count)
           for count in (1, 2, 7, TILE, TILE + 1, ROWS) for first in (0, 3, 7, ROWS - 1)}
LAYOUTS["every/3/15"] = (STEPS, ENVS, "every", 3, ROWS)
LAYOUTS["single/0/9"] = (9, 1, "none", 0, 9)

# at the limits of rf_lstm_ppo.h (the same form; each family says which of its networks runs which, limit_layouts_of):
#   tuned/    ppo_lstm_tuned.yml's T = 8, n = 8, no flagged start: every sequence has exactly the 8 rows whose weights both
#             walks load before the first is used; B = 8 (at first 3 a 5-row tail and a 3-row head), B = 64 = N (8 tiles)
#   depth/    T = 17, n = 4, one flagged start per environment (starts_of): sequences of 1, 8, 9, 16 and 17 rows; B = 65,
#             B = 68 = N from row 5 (a wrap), and B = 17 for the network with every limit at once
#   untuned/  ppo_lstm_untuned.yml's T = 128, n = 8, B = 128, starts drawn from a fixed seed: one whole environment that
#             enters from its stored state, and rows 100 .. 227 across an environment boundary
#   wave/     T = 16, n = 64, N = 1024: every row a start at B = 1024 (1024 one-row sequences, 128 tiles, the second trip
#             of the loss reductions), and no flagged start at B = 513 (33 sequences)
LIMIT_LAYOUTS = {"tuned/0/8": (8, 8, "none", 0, 8), "tuned/3/8": (8, 8, "none", 3, 8), "tuned/0/64": (8, 8, "none", 0, 64),
                 "depth/0/65": (17, 4, "depth", 0, 65), "depth/5/68": (17, 4, "depth", 5, 68),
                 "depth/0/17": (17, 4, "depth", 0, 17),
                 "untuned/0/128": (128, 8, "drawn", 0, 128), "untuned/100/128": (128, 8, "drawn", 100, 128),
                 "wave/7/1024": (16, 64, "every", 7, 1024), "wave/0/513": (16, 64, "none", 0, 513)}
LAYOUTS.update(LIMIT_LAYOUTS)
DEPTH_STARTS = ((0, 0, 1), (1, 1, 2), (8, 2, 255), (16, 3, 1))  # (step, environment, byte)
DRAWN_SEED, DRAWN_SHARE = 1, 3 / 128


def layouts_of(index):
    return [name for name, layout in LAYOUTS.items() if name not in LIMIT_LAYOUTS and (index != LIMITS or layout[4] <= 2)]


def limit_layouts_of(index):
    """TUNED runs every limit layout but the one of 17 rows; sb3-contrib's default network (H = 256) the two untuned ones,
    ppo_lstm_untuned.yml's real shape; the network with every limit at once the 17-row sequence alone."""
    if index == TUNED:
        return [name for name in LIMIT_LAYOUTS if name != "depth/0/17"]
    if index == DEFAULT:
        return ["untuned/0/128", "untuned/100/128"]
    return ["depth/0/17"] if index == LIMITS else []


def starts_of(kind, n_steps, num_envs, seed=DRAWN_SEED):
    """uint8 [T + 1, n].  mixed (T = 5, n = 3): environment 0 starts at t = 0 (byte 1) and t = 2 (byte 2), environment 1
    runs four rows from its stored, non-zero state and starts at t = 4 (byte 255), environment 2 starts at t = 0 and 3.
    depth (T = 17, n = 4): environment 0 starts at t = 0 (one sequence of 17 rows), environment 1 at t = 1 (1 and 16
    rows, the first from its stored state), environment 2 at t = 8 (8 and 9), environment 3 at t = 16 (16 and 1).
    drawn: every byte of rows 0 .. T - 1 is a start with probability DRAWN_SHARE, by turns 1, 2 and 255, from
    `seed` (DRAWN_SEED); environment 0's first row is none."""
    starts = np.zeros((n_steps + 1, num_envs), dtype=np.uint8)
    if kind == "every":
        starts[...] = np.array([1, 2, 255], dtype=np.uint8)[np.arange(starts.size) % 3].reshape(starts.shape)
    elif kind == "mixed":
        starts[0, 0], starts[2, 0], starts[4, 1], starts[0, 2], starts[3, 2] = 1, 2, 255, 1, 1
        starts[n_steps] = 1  # (row T is never read)
    elif kind == "depth":
        for step, env, byte in DEPTH_STARTS:
            starts[step, env] = byte
    elif kind == "drawn":
        drawn = np.random.default_rng(seed).random((n_steps, num_envs)) < DRAWN_SHARE
        drawn[0, 0] = False
        starts[:n_steps][drawn] = np.array([1, 2, 255], dtype=np.uint8)[np.arange(int(drawn.sum())) % 3]
    else:
        assert kind == "none", kind
    return starts


def restated_rows(episode_starts, n_steps, num_envs, first, count):
    """The sequence rule in plain Python, from the issue's words: [(row, is_start, entering state source)], the source
    "zero", ("stored", t, e) or None (the row before)."""
    out = []
    for b in range(count):
        row = (first + b) % (n_steps * num_envs)
        env, step = row // n_steps, row % n_steps
        flagged = episode_starts[step][env] != 0
        is_start = b == 0 or step == 0 or flagged
        out.append((row, bool(is_start), ("zero" if flagged else ("stored", step, env)) if is_start else None))
    return out


def own_log_probs(spec, params, batch, starts, states, n_steps, num_envs):
    """log pi(a | row) of every row of flat()'s order, by the twin's own forward over the whole rollout as one minibatch."""
    from reinfocus_amd.environments import lstm_learner, policy

    total = n_steps * num_envs
    rows = lstm_learner.sequence_rows(starts, n_steps, num_envs, 0, total)
    lstm, layers, last = spec.nets(params)[0]
    with np.errstate(all="ignore"):
        h1 = lstm_learner._cell_rows(batch["observations"], rows, (states[:, 0, 0], states[:, 0, 1]), lstm)[4]
        for weight_t, bias in layers:
            h1 = policy.activation(policy.linear(h1, weight_t, bias), spec.activation)
        logits = policy.linear(h1, *last)
    return policy.log_softmax(logits)[np.arange(total), batch["actions"]]


@functools.lru_cache(maxsize=None)
def update_inputs(index, n_steps, num_envs, kind):
    """(spec, packed parameters, batch dict of N rows, episode_starts, lstm_states).  The parameters are hostile as
    tests/learner_io_cases.py's (two logits tie, the last lies 200 below); the stored log-probabilities are the twin's
    own, shifted by SHIFTS in turn; the stored states are normal values of scale 1/2."""
    network = NETWORKS[index]
    spec = spec_of(network)
    params = spec.pack(lstm_cases.state_dict(spec, 300 + index, hostile=True))
    total = n_steps * num_envs
    rng = np.random.default_rng(1000 * index + total)
    starts = starts_of(kind, n_steps, num_envs)
    states = (0.5 * rng.standard_normal((n_steps + 1,) + spec.state_shape(num_envs))).astype(np.float32)
    batch = {"observations": learner_cases.finite_rows(network[0], total, 77 * index + total),
             "actions": rng.integers(0, spec.n_actions, total).astype(np.int64),
             "advantages": rng.standard_normal(total).astype(np.float32),
             "returns": rng.standard_normal(total).astype(np.float32)}
    shifts = np.array(SHIFTS, dtype=np.float32)[np.arange(total) % len(SHIFTS)]
    batch["log_probs"] = (own_log_probs(spec, params, batch, starts, states, n_steps, num_envs) - shifts).astype(np.float32)
    return spec, params, batch, starts, states


def layout_inputs(index, name):
    n_steps, num_envs, kind, first, count = LAYOUTS[name]
    return update_inputs(index, n_steps, num_envs, kind) + (n_steps, num_envs, first, count)


@functools.lru_cache(maxsize=None)
def twin_updates(index, name):
    """[(params, state, stats, gradient)] after each of UPDATES consecutive updates by the numpy twin on the layout's
    minibatch: the reference, computed once."""
    from reinfocus_amd.environments import learner, lstm_learner

    spec, params, batch, starts, states, n_steps, num_envs, first, count = layout_inputs(index, name)
    state = learner.fresh_state(spec)
    seen = []
    for update in range(UPDATES):
        grad = lstm_learner.lstm_gradient_numpy(spec, params, batch, starts, states, n_steps, num_envs, first, count,
                                                hyper_of(update))[0]
        params, state, stats = lstm_learner.lstm_update_numpy(spec, params, state, batch, starts, states, n_steps, num_envs,
                                                              first, count, hyper_of(update))
        seen.append((params, state, stats, grad))
    return seen


def hostcheck():
    from tests import helpers

    lib = ctypes.CDLL(helpers.built("tests/lstmppocheck", "liblstmppocheck.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.lpc_state_size.restype = lib.lpc_workspace_size.restype = lib.lpc_grad_offset.restype = ctypes.c_ulonglong
    lib.lpc_state_size.argtypes = [vp]
    lib.lpc_workspace_size.argtypes = lib.lpc_grad_offset.argtypes = [vp, i32]
    lib.lpc_sequences.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
    lib.lpc_update.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    return lib


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
T = rollout_cases.T
GAMMA, GAE_LAMBDA = rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA
E2E_SIZES, E2E_ITERATIONS, E2E_EPOCHS, E2E_BATCH = (1, 9), 2, 2, 4
E2E_KINDS = lstm_cases.E2E_KINDS
LEARNER_KW = dict(learning_rate=1e-2, ent_coef=0.01)


def e2e_splits(iteration, total):
    return [int(s) for s in np.random.default_rng(900 + iteration).integers(total, size=E2E_EPOCHS)]


def train_runs(rollout, policy, learner, reset, unwrap, trains=1):
    """E2E_ITERATIONS iterations of collect + train: per iteration the rollout's slabs (the recurrent ones included),
    the parameters, the optimizer state and the stats, unwrapped."""
    obs = reset()
    seen = []
    for iteration in range(E2E_ITERATIONS):
        rollout.start(obs if iteration == 0 else None)
        rollout.collect(policy)
        record = lstm_cases.slabs_of(rollout, policy, unwrap)
        for train in range(trains):
            stats = learner.train(rollout, E2E_EPOCHS, E2E_BATCH, splits=e2e_splits(iteration, T * rollout.num_envs))
            record[f"stats/{train}"] = unwrap(stats)
        record["params"], record["state"] = unwrap(policy.params), unwrap(learner.state)
        seen.append(record)
    return seen


@functools.lru_cache(maxsize=None)
def twin_train_runs(kind, n, trains=1):
    from reinfocus_amd.environments import harness

    env = lstm_cases.make_env(kind, n, False)
    try:
        spec = lstm_cases.e2e_spec(kind)
        policy = harness.LstmPolicy(spec, lstm_cases.SEED, num_envs=n)
        policy.load_state_dict(lstm_cases.state_dict(spec, 3))
        learner = harness.LstmLearner(policy, **LEARNER_KW)
        rollout = harness.Rollout(env, T, GAMMA, GAE_LAMBDA)
        return train_runs(rollout, policy, learner, lambda: env.reset()[0], np.array, trains)
    finally:
        env.close()


same_runs = rollout_cases.same_runs


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
_guarded, _guards_kept = learner_cases._guarded, learner_cases._guards_kept


class _Device:
    """One update's device arrays: outputs between guards, inputs as they are."""

    def __init__(self, torch, ctx, lib, spec, params, state, batch, starts, states, n_steps, num_envs, max_batch=None):
        """The workspace has exactly rf_lstm_ppo_workspace_size(max_batch) bytes between its guards (N's where none is
        given)."""
        self.torch, self.ctx, self.lib, self.spec = torch, ctx, lib, spec
        self.n_steps, self.num_envs = n_steps, num_envs
        self.whole = {}
        self.whole["params"], self.params = _guarded(torch, params)
        self.whole["state"], self.state = _guarded(torch, state)
        self.whole["stats"], self.stats = _guarded(torch, np.zeros(8, dtype=np.float32))
        self.stats.view(torch.int32).fill_(SENTINEL)
        total = n_steps * num_envs
        floats = ctx.lstm_ppo_workspace_size(spec.desc(), max_batch or total) // 4
        assert floats > 0 and ctx.lstm_ppo_state_size(spec.desc()) == 4 * state.size
        assert ctx.lstm_ppo_workspace_size(spec.desc(), 1) <= 4 * floats
        self.whole["workspace"], self.workspace = _guarded(torch, np.zeros(floats, dtype=np.float32))
        self.batch = {key: torch.from_numpy(value).cuda() for key, value in batch.items()}
        self.starts, self.states = torch.from_numpy(starts).cuda(), torch.from_numpy(states).cuda()

    def call(self, first, count, hyper, **changed):
        a = dict(desc=self.spec.desc(), hyper=tuple(hyper), params=self.params.data_ptr(), state=self.state.data_ptr(),
                 workspace=self.workspace.data_ptr(), n_steps=self.n_steps, num_envs=self.num_envs,
                 obs=self.batch["observations"].data_ptr(), actions=self.batch["actions"].data_ptr(),
                 log_probs=self.batch["log_probs"].data_ptr(), advantages=self.batch["advantages"].data_ptr(),
                 returns=self.batch["returns"].data_ptr(), starts=self.starts.data_ptr(), states=self.states.data_ptr(),
                 first=first, batch=count, stats=self.stats.data_ptr(),
                 stream=self.torch.cuda.current_stream().cuda_stream)
        a.update(changed)  # (arguments given by their names above, in place of the tensors')
        self.ctx.lstm_ppo_update(a["desc"], a["hyper"], a["params"], a["state"], a["workspace"], a["n_steps"], a["num_envs"],
                                 a["obs"], a["actions"], a["log_probs"], a["advantages"], a["returns"], a["starts"],
                                 a["states"], a["first"], a["batch"], a["stats"], a["stream"])

    def outputs(self):
        self.torch.cuda.synchronize()
        return self.params.cpu().numpy(), self.state.cpu().numpy(), self.stats.cpu().numpy()

    def gradient(self, count):
        """The packed gradient the last update of `count` rows left in the workspace."""
        at = int(self.lib.lpc_grad_offset(ctypes.byref(_lstm_desc(self.spec)), count))
        return self.workspace[at:at + self.spec.size].cpu().numpy()

    def guards_kept(self):
        return all(_guards_kept(whole) for whole in self.whole.values())


def _lstm_desc(spec):
    from reinfocus_amd import _native

    return _native.LstmPolicyDesc(*spec.desc())


def _same_update(got, want, what):
    learner_cases._same_update(got[:3], want[:3], what)
    if len(got) > 3:
        assert bits(got[3]) == bits(want[3]), f"{what}: the gradient differs"


def kernel_case(torch, ctx, lib, index, name):
    """rf_lstm_ppo_update against lstm_update_numpy as bytes over UPDATES consecutive updates, the gradient included; a
    limit layout's workspace is sized for its B, not for N."""
    from reinfocus_amd.environments import learner

    spec, params, batch, starts, states, n_steps, num_envs, first, count = layout_inputs(index, name)
    want = twin_updates(index, name)
    device = _Device(torch, ctx, lib, spec, params, learner.fresh_state(spec), batch, starts, states, n_steps, num_envs,
                     count if name in LIMIT_LAYOUTS else None)
    for update in range(UPDATES):
        device.call(first, count, hyper_of(update))
        _same_update(device.outputs() + (device.gradient(count),), want[update], f"update {update}")
    assert device.guards_kept(), "a guard was written"
    assert all(stats[7] == 0 for _, _, stats, _ in want)


def refusal_case(torch, ctx, lib):
    """Each refusal leaves parameters, state and stats as they were: nothing was enqueued."""
    from reinfocus_amd.environments import learner

    index, name = TUNED, f"mixed/3/{TILE + 1}"
    spec, params, batch, starts, states, n_steps, num_envs, first, count = layout_inputs(index, name)
    want = twin_updates(index, name)
    device = _Device(torch, ctx, lib, spec, params, learner.fresh_state(spec), batch, starts, states, n_steps, num_envs)
    before = None

    def refused(match, **changed):
        hyper = changed.pop("hyper", hyper_of(0))
        try:
            device.call(changed.pop("first", first), count, hyper, **changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        got = device.outputs()
        assert all(bits(x) == bits(y) for x, y in zip(got, before)), f"an output was written ({match})"

    before = device.outputs()
    assert (before[2].view(np.uint32) == SENTINEL).all()
    desc = list(spec.desc())
    for field, value in ((0, 0), (0, 257), (1, 1), (1, 65), (2, 2), (3, 0), (3, 3), (4, 257), (6, 3), (7, 0), (9, 0), (9, 257),
                         (9, -1)):
        refused("outside the limits", desc=tuple(desc[:field] + [value] + desc[field + 1:]))
    refused("at least 1", n_steps=0)
    refused("at least 1", num_envs=0)
    refused("B = ", batch=0)
    refused("B = ", batch=ROWS + 1)
    refused("B = ", batch=1025)
    refused("first = ", first=-1)
    refused("first = ", first=ROWS)
    for field in range(8):
        refused("hyper-parameter", hyper=hyper_of(0)._replace(**{learner.Hyper._fields[field]: -1.0}))
        refused("hyper-parameter", hyper=hyper_of(0)._replace(**{learner.Hyper._fields[field]: float("nan")}))
    refused("hyper-parameter", hyper=hyper_of(0)._replace(learning_rate=float("inf")))
    refused("hyper-parameter", hyper=hyper_of(0)._replace(beta1=1.0))
    refused("hyper-parameter", hyper=hyper_of(0)._replace(beta2=1.5))
    host = np.zeros(4 * spec.size + 64, dtype=np.float32)
    for name in ("params", "state", "workspace", "obs", "actions", "log_probs", "advantages", "returns", "starts", "states",
                 "stats"):
        refused("NULL argument", **{name: None})
        refused("is not device memory", **{name: host.ctypes.data})
    refused("not aligned", obs=device.batch["observations"].data_ptr() + 2)
    refused("not aligned", actions=device.batch["actions"].data_ptr() + 4)
    refused("not aligned", states=device.states.data_ptr() + 2)
    refused("not aligned", state=device.state.data_ptr() + 4)
    refused("not aligned", workspace=device.workspace.data_ptr() + 4)
    block = torch.zeros(32 * 1024 * 1024, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    refused("fewer than", obs=end - 4 * (ROWS * spec.obs_width - 1))
    refused("fewer than", params=end - 4 * (spec.size - 1))
    refused("fewer than", state=end - 8 * spec.size)  # (a state that is too small)
    refused("fewer than", workspace=end - 1024)  # (a workspace that is too small)
    refused("fewer than", stats=end - 16)
    refused("d_episode_starts has fewer than", starts=end - ((n_steps + 1) * num_envs - 1))  # (the slabs have T + 1 rows)
    refused("d_lstm_states has fewer than", states=end - 4 * (states.size - 1))
    refused("d_lstm_states has fewer than", states=end - 4 * n_steps * 4 * num_envs * spec.lstm_hidden)  # (T rows only)
    refused("d_params overlaps d_observations", params=device.batch["observations"].data_ptr())
    refused("d_stats overlaps d_returns", stats=device.batch["returns"].data_ptr())
    refused("d_workspace overlaps d_lstm_states", workspace=device.states.data_ptr())
    refused("d_state overlaps d_params", state=device.params.data_ptr())
    refused("d_workspace overlaps d_state", workspace=device.state.data_ptr())
    refused("d_stats overlaps d_workspace", stats=device.workspace.data_ptr())
    device.call(first, count, hyper_of(0))  # ... and the same arguments unchanged are taken
    _same_update(device.outputs() + (device.gradient(count),), want[0], "the unchanged call")
    assert device.guards_kept()
    _capturing_stream_is_refused(torch, device, first, count)


def _capturing_stream_is_refused(torch, device, first, count):
    """A stream of its own in (relaxed) capture, by the runtime's own calls: the update is refused, nothing was enqueued,
    the capture ends with an empty graph that is never instantiated or replayed."""
    from reinfocus_amd import torch_interop

    hip = ctypes.CDLL(torch_interop.hip_runtimes()[0])
    stream, graph = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    before = device.outputs()
    assert hip.hipStreamBeginCapture(stream, 2) == 0  # hipStreamCaptureModeRelaxed
    message = None
    try:
        device.call(first, count, hyper_of(1), stream=stream.value)
    except AssertionError as caught:  # (RF_ERR_INVALID)
        message = str(caught)
    finally:
        ended = hip.hipStreamEndCapture(stream, ctypes.byref(graph))
        if graph.value:
            hip.hipGraphDestroy(graph)
        hip.hipStreamDestroy(stream)
    assert ended == 0 and message is not None and "being captured" in message, message
    got = device.outputs()
    assert all(bits(x) == bits(y) for x, y in zip(got, before)), "a refused update wrote an output"


def _device_pair(torch, harness, env, kind):
    spec, policy = lstm_cases._device_policy(torch, harness, env, kind)
    return policy, harness.DeviceLstmLearner(policy, **LEARNER_KW)


def _unwrap(tensor):
    return tensor.cpu().numpy()


def end_to_end_case(torch, kind, n):
    from reinfocus_amd.environments import harness

    want = twin_train_runs(kind, n)
    env = lstm_cases.make_env(kind, n, True)
    try:
        policy, learner = _device_pair(torch, harness, env, kind)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        got = train_runs(rollout, policy, learner, lambda: env.reset_tensors()[0], _unwrap)
        same_runs(got, want)
        assert env.device_fault() is None
        assert bits(want[0]["params"]) != bits(want[1]["params"]) and (want[1]["stats/0"][:, 7] == 0).all()
        assert want[0]["stats/0"].shape == (E2E_EPOCHS * -(-T * n // E2E_BATCH), 8)
        if n > 1:  # (episode starts fall inside minibatches)
            assert want[1]["episode_starts"][1:T].any()
    finally:
        env.close()


def no_sync_case(torch):
    """Two iterations of collect + train enqueued back to back, nothing read in between; one synchronisation at the end."""
    from reinfocus_amd.environments import harness

    kind, n = "view", 9
    want = twin_train_runs(kind, n)
    env = lstm_cases.make_env(kind, n, True)
    try:
        policy, learner = _device_pair(torch, harness, env, kind)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        obs = env.reset_tensors()[0]
        torch.cuda.synchronize()
        kept = []
        for iteration in range(E2E_ITERATIONS):
            rollout.start(obs if iteration == 0 else None)
            rollout.collect(policy)
            stats = learner.train(rollout, E2E_EPOCHS, E2E_BATCH, splits=e2e_splits(iteration, T * n))
            kept.append((stats, policy.params.clone(), rollout.lstm_states.clone(), rollout.episode_starts.clone()))
        torch.cuda.synchronize()  # the only one
        for iteration, (stats, params, states, starts) in enumerate(kept):
            assert bits(_unwrap(stats)) == bits(want[iteration]["stats/0"]), iteration
            assert bits(_unwrap(params)) == bits(want[iteration]["params"]), iteration
            assert bits(_unwrap(states)) == bits(want[iteration]["lstm_states"]), iteration
            assert bits(_unwrap(starts)) == bits(want[iteration]["episode_starts"]), iteration
        assert bits(_unwrap(learner.state)) == bits(want[-1]["state"])
        assert env.device_fault() is None
    finally:
        env.close()


def resume_case(torch):
    """state_dict / load_state_dict of the optimizer resumes bit for bit in a fresh learner."""
    from reinfocus_amd.environments import harness

    kind, n = "view", 9
    env = lstm_cases.make_env(kind, n, True)
    try:
        policy, learner = _device_pair(torch, harness, env, kind)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        rollout.start(env.reset_tensors()[0])
        rollout.collect(policy)
        splits = e2e_splits(0, T * n)
        learner.train(rollout, E2E_EPOCHS, E2E_BATCH, splits=splits)
        kept, kept_params = learner.state_dict(), policy.state_dict()
        assert kept["step"] == E2E_EPOCHS * -(-T * n // E2E_BATCH)
        straight = _unwrap(learner.train(rollout, E2E_EPOCHS, E2E_BATCH, splits=splits))
        want = _unwrap(policy.params), _unwrap(learner.state)
        policy.load_state_dict(kept_params)
        fresh = harness.DeviceLstmLearner(policy, **LEARNER_KW)
        fresh.load_state_dict(kept)
        resumed = _unwrap(fresh.train(rollout, E2E_EPOCHS, E2E_BATCH, splits=splits))
        assert bits(resumed) == bits(straight)
        assert bits(_unwrap(policy.params)) == bits(want[0]) and bits(_unwrap(fresh.state)) == bits(want[1])
    finally:
        env.close()


def surface_case(torch):
    """The refusals of the Python surface, update() by itself, and train() without splits."""
    from reinfocus_amd.environments import harness, learner as learner_module, lstm_learner
    from tests import policy_io_cases as policy_cases

    spec = lstm_cases.e2e_spec("view")
    try:
        harness.DeviceLstmLearner(harness.LstmPolicy(spec, 0))
    except TypeError as caught:
        assert "DeviceLstmPolicy" in str(caught)
    else:
        raise AssertionError("a numpy LstmPolicy was taken")
    n = 3
    env = lstm_cases.make_env("view", n, True)
    plain = policy_cases.make_env("plain", n, True)
    jumps = harness.DeviceVectorContinuousJumps(num_envs=2, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        policy, learner = _device_pair(torch, harness, env, "view")
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        rollout.start(env.reset_tensors()[0])
        _, feedforward = policy_cases._device_policy(torch, harness, plain, "plain")
        other = harness.DeviceRollout(plain, T, GAMMA, GAE_LAMBDA)
        other.start(plain.reset_tensors()[0])
        other.collect(feedforward)
        for wrong, error, match in ((other, ValueError, "not collected with a recurrent policy"),
                                    (harness.DeviceRollout(jumps, T, GAMMA, GAE_LAMBDA), ValueError, "out of scope")):
            try:
                learner.train(wrong, 1, E2E_BATCH)
            except error as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"taken ({match})")
        rollout.collect(policy)
        for bad in (dict(n_epochs=0, batch_size=4), dict(n_epochs=1, batch_size=0), dict(n_epochs=1, batch_size=1025),
                    dict(n_epochs=2, batch_size=4, splits=[0]), dict(n_epochs=1, batch_size=4, splits=[T * n])):
            try:
                learner.train(rollout, **bad)
            except ValueError:
                pass
            else:
                raise AssertionError(f"taken ({bad})")
        parts = lstm_learner.parts_of(rollout)
        twin_parts = {key: _unwrap(value) if isinstance(value, torch.Tensor) else value for key, value in parts.items()}
        params = _unwrap(policy.params)
        for bad in ((0, 0), (0, T * n + 1), (-1, 4), (T * n, 4)):
            try:
                learner.update(rollout, *bad)
            except ValueError:
                pass
            else:
                raise AssertionError(f"taken ({bad})")
        stats = learner.update(rollout, 5, 6)
        want = lstm_learner.lstm_update_numpy(policy.spec, params, learner_module.fresh_state(policy.spec), twin_parts,
                                              twin_parts["episode_starts"], twin_parts["lstm_states"], T, n, 5, 6,
                                              learner.hyper())
        learner_cases._same_update((_unwrap(policy.params), _unwrap(learner.state), _unwrap(stats)), want, "update()")
        try:
            learner.update(dict(parts, lstm_states=parts["lstm_states"].cpu()), 0, 4)
        except ValueError:
            pass
        else:
            raise AssertionError("a slab on the host was taken")
        stats = learner.train(rollout, 1, 8, generator=np.random.default_rng(3))
        assert stats.shape == (3, 8) and (_unwrap(stats)[:, 7] == 0).all()
    finally:
        env.close()
        plain.close()
        jumps.close()


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    ctx = _native.Context(0)
    lib = hostcheck()
    for index in range(len(NETWORKS)):
        for name in layouts_of(index) + limit_layouts_of(index):
            with record.case(f"kernel/{index}/{name}"):
                kernel_case(torch, ctx, lib, index, name)
    with record.case("refusals"):
        refusal_case(torch, ctx, lib)
    ctx.close()
    for kind in E2E_KINDS:
        for n in E2E_SIZES:
            with record.case(f"end-to-end/{kind}/{n}"):
                end_to_end_case(torch, kind, n)
    with record.case("no-sync"):
        no_sync_case(torch)
    with record.case("resume"):
        resume_case(torch)
    with record.case("surface"):
        surface_case(torch)
    with record.case("finished"):
        pass


# ---- torch on the CPU: sb3-contrib's sequences, stable-baselines3's loss, autograd, clip_grad_norm_ and Adam -----------
def torch_lstm_learner(path_in, path_out):
    """From a state_dict, a rollout and one minibatch: the packed gradient before clipping, the same with the gradient
    through h_prev / c_prev cut (float64 only), and the packed parameters after 1 and after `updates` updates on that
    minibatch, in float64 and in float32.  torch.nn.LSTM cells stepped per row, with the sequence rule and the select
    of the definition; the stored states are constants.  In a process of its own."""
    import torch

    data = np.load(path_in)
    names = [str(name) for name in data["names"]]
    activation = torch.nn.Tanh if str(data["activation"]) == "tanh" else torch.nn.ReLU
    clip_range, ent_coef, vf_coef, max_grad_norm, learning_rate = (float(data[k]) for k in (
        "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "learning_rate"))
    updates = int(data["updates"])
    row, env, step, is_start, zero = (data[k] for k in ("row", "env", "step", "is_start", "zero"))
    out = {}
    for label, dtype in (("64", torch.float64), ("32", torch.float32)):
        tensors = {name: torch.from_numpy(data[name]).to(dtype) for name in names}
        stored = torch.from_numpy(data["lstm_states"]).to(dtype)  # (no gradient: a constant)
        obs = torch.from_numpy(data["obs"]).to(dtype)[torch.from_numpy(row)]
        hidden = stored.shape[-1]
        modules = {}

        def net(lstm_name, extractor, head_name):
            lstm = torch.nn.LSTM(obs.shape[1], hidden, num_layers=1).to(dtype)
            lstm.load_state_dict({part: tensors[f"{lstm_name}.{part}"] for part in
                                  ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
            modules[lstm_name] = lstm
            layers = []
            keys = [f"mlp_extractor.{extractor}.{i}" for i in (0, 2) if f"mlp_extractor.{extractor}.{i}.weight" in tensors]
            for key in keys + [head_name]:
                weight = tensors[key + ".weight"]
                linear = torch.nn.Linear(weight.shape[1], weight.shape[0]).to(dtype)
                with torch.no_grad():
                    linear.weight.copy_(weight)
                    linear.bias.copy_(tensors[key + ".bias"])
                modules[key] = linear
                layers += [linear, activation()]
            return lstm, torch.nn.Sequential(*layers[:-1])

        nets = [net("lstm_actor", "policy_net", "action_net"), net("lstm_critic", "value_net", "value_net")]

        def forward(which, cut):
            lstm, mlp = nets[which]
            outs = []
            h = c = None
            for b in range(len(row)):
                if is_start[b]:
                    if zero[b]:
                        h = torch.zeros(1, 1, hidden, dtype=dtype)
                        c = torch.zeros(1, 1, hidden, dtype=dtype)
                    else:
                        h = stored[step[b], which, 0, env[b]].view(1, 1, hidden)
                        c = stored[step[b], which, 1, env[b]].view(1, 1, hidden)
                elif cut:
                    h, c = h.detach(), c.detach()
                y, (h, c) = lstm(obs[b].view(1, 1, -1), (h, c))
                outs.append(y.view(hidden))
            return mlp(torch.stack(outs))

        def packed(grad):
            parts = []
            for name in names:
                key, part = name.rsplit(".", 1)
                tensor = getattr(modules[key], part)
                tensor = tensor.grad if grad else tensor.detach()
                parts.append((tensor.t() if part.startswith("weight") else tensor).reshape(-1))
            return torch.cat(parts).numpy().copy()

        index = torch.from_numpy(row)
        actions = torch.from_numpy(data["actions"])[index]
        old, advantages, returns = (torch.from_numpy(data[k]).to(dtype)[index] for k in
                                    ("old_log_probs", "advantages", "returns"))
        parameters = [p for lstm, mlp in nets for p in list(lstm.parameters()) + list(mlp.parameters())]
        optimizer = torch.optim.Adam(parameters, lr=learning_rate, eps=1e-5)

        def loss_of(cut):
            adv = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
            distribution = torch.distributions.Categorical(logits=forward(0, cut))
            log_prob = distribution.log_prob(actions)
            ratio = torch.exp(log_prob - old)
            policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
            value_loss = torch.nn.functional.mse_loss(returns, forward(1, cut).flatten())
            return policy_loss + ent_coef * -distribution.entropy().mean() + vf_coef * value_loss, ratio

        if label == "64":
            optimizer.zero_grad()
            loss_of(True)[0].backward()
            out["grad_cut64"] = packed(True)
        for update in range(updates):
            loss, ratio = loss_of(False)
            optimizer.zero_grad()
            loss.backward()
            if update == 0:
                out["grad" + label] = packed(True)
                out["clip_fraction" + label] = (torch.abs(ratio - 1) > clip_range).to(torch.float64).mean().numpy()
            torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)
            optimizer.step()
            if update == 0:
                out["first" + label] = packed(False)
        out["last" + label] = packed(False)
    np.savez(path_out, **out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "--torch-lstm-learner":
        torch_lstm_learner(sys.argv[2], sys.argv[3])
    else:
        run_cases(sys.argv[1])
