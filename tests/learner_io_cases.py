"""TEST INFRASTRUCTURE: what tests/test_learner_logic.py and tests/test_gpu_learner.py share -- the networks, the batch
sizes, hostile minibatches, the numpy twin's results (computed once and shared), the drivers of the end-to-end runs --
and the child process of the GPU file.

As tests/policy_io_cases.py: everything that needs torch and the library together runs in one fresh process that imports
torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.learner_io_cases <results.jsonl>
    python -m tests.learner_io_cases --torch-learner <in.npz> <out.npz>       (torch on the CPU: autograd, Adam)
    python -m tests.learner_io_cases --torch-subgradient <in.npz> <out.npz>   (torch on the CPU: min and clamp by autograd)
"""

import functools
import os
import sys

import numpy as np

from tests import policy_io_cases as policy_cases
from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = policy_cases.TILE
BATCHES = (1, 2, 7, TILE, TILE + 1, 64, 65)  # one sample, a pair, a ragged tile, a full one, one past it, 8 tiles, 8 + 1
# (obs_width, pi, vf, n_actions, activation): the least network; widths that are no multiple of a wave with one and two
# layers mixed; stable-baselines3's default; every limit at once; a narrow layer in front of a wide one
NETWORKS = ((1, (1,), (1,), 2, "relu"),
            (20, (63,), (65, 64), 13, "tanh"),
            (20, (64, 64), (64, 64), 13, "tanh"),
            (256, (256, 256), (256, 256), 64, "relu"),
            (20, (5, 256), (256,), 13, "relu"))
# at the limits of rf_ppo.h: the last minibatch whose s_red reductions take a single trip; the first past it, with a ragged
# last tile; no power of two and no multiple of the tile; RF_PPO_MAX_BATCH itself, the workspace at its largest.  On the
# least network and on stable-baselines3's default; on the network with every limit at once 513 alone (the twin's three
# updates and the host build's take 3.7 s there and 7.7 s at 1024, which is left out; 0.2 s on the default network)
LIMIT_BATCHES = (512, 513, 1000, 1024)
LIMIT_CASES = tuple((index, count) for index in (0, 2) for count in LIMIT_BATCHES) + ((3, 513),)
UPDATES = 3
# per update: (max_grad_norm, learning_rate): a norm that clips, one that does not, one that clips
SCHEDULE = ((0.5, 1e-2), (1e6, 3e-4), (0.05, 1e-2))
SHIFTS = (0.0, 0.3, -0.3, 0.05, -0.05, 1.0, -2.0)  # d = logp - old_logp: inside the clip range, past both bounds, d > 0
GUARD = 16  # floats on either side of every output
SENTINEL = policy_cases.SENTINEL
T, STACK = rollout_cases.T, rollout_cases.STACK
GAMMA, GAE_LAMBDA = rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA
E2E_ENVS, E2E_ITERATIONS, E2E_EPOCHS, E2E_BATCH = 4, 2, 2, 16  # 28 rows: minibatches of 16 and 12
E2E_KINDS = policy_cases.E2E_KINDS

bits = policy_cases.bits
spec_of = policy_cases.spec_of


def hyper_of(update, **changed):
    from reinfocus_amd.environments import learner

    max_grad_norm, learning_rate = SCHEDULE[update % len(SCHEDULE)]
    values = dict(learning_rate=learning_rate, clip_range=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=max_grad_norm,
                  beta1=0.9, beta2=0.999, adam_eps=1e-5, normalize_advantage=1)
    values.update(changed)
    return learner.Hyper(**values)


def finite_rows(width, n, seed):
    """float32 [n, width]: normal rows with +-0, subnormals and large values strewn in -- everything finite."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, width)).astype(np.float32)
    specials = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 30.0, -2.5e-3], dtype=np.float32)
    where = rng.random((n, width)) < 0.2
    rows[where] = rng.choice(specials, int(where.sum()))
    return rows


@functools.lru_cache(maxsize=None)
def update_inputs(index, count):
    """(spec, packed parameters, batch dict of N = count + 3 rows, [UPDATES] index arrays).  The parameters are hostile:
    the logits of actions 0 and 1 tie exactly, the last of three or more actions lies 200 below (e_i == 0).  The stored
    log-probabilities are the twin's own, shifted by SHIFTS in turn.  Every index array is part of a permutation with
    its last entry repeated from its first."""
    from reinfocus_amd.environments import policy

    network = NETWORKS[index]
    spec = spec_of(network)
    params = spec.pack(policy_cases.state_dict(spec, 200 + index, hostile=True))
    rows = count + 3
    rng = np.random.default_rng(1000 * index + count)
    obs = finite_rows(network[0], rows, 77 * index + count)
    actions = rng.integers(0, spec.n_actions, rows).astype(np.int64)
    log_probs = policy.log_softmax(policy._net(spec, spec.nets(params)[0], obs))[np.arange(rows), actions]
    shifts = np.array(SHIFTS, dtype=np.float32)[np.arange(rows) % len(SHIFTS)]
    batch = {"observations": obs, "actions": actions, "log_probs": (log_probs - shifts).astype(np.float32),
             "advantages": rng.standard_normal(rows).astype(np.float32),
             "returns": rng.standard_normal(rows).astype(np.float32),
             "values": np.zeros(rows, dtype=np.float32)}
    indices = []
    for _ in range(UPDATES):
        chosen = rng.permutation(rows)[:count].astype(np.int64)
        if count > 1:
            chosen[-1] = chosen[0]
        indices.append(chosen)
    return spec, params, batch, indices


@functools.lru_cache(maxsize=None)
def twin_updates(index, count):
    """[(params, state, stats)] after each of UPDATES consecutive updates by the numpy twin: the reference, computed
    once."""
    from reinfocus_amd.environments import learner

    spec, params, batch, indices = update_inputs(index, count)
    state = learner.fresh_state(spec)
    seen = []
    for update in range(UPDATES):
        params, state, stats = learner.ppo_update_numpy(spec, params, state, batch, indices[update], hyper_of(update))
        seen.append((params, state, stats))
    return seen


def skip_variants(batch, indices):
    """{name: (batch, index, flag)} of minibatches an update must skip."""
    from reinfocus_amd.environments import learner

    rows = batch["actions"].shape[0]
    high, low = indices[0].copy(), indices[0].copy()
    high[0], low[-1] = rows, -1
    bad_action = dict(batch, actions=batch["actions"].copy())
    bad_action["actions"][indices[0][0]] = 64
    negative_action = dict(batch, actions=batch["actions"].copy())
    negative_action["actions"][indices[0][-1]] = -1
    infinite = dict(batch, returns=np.full(rows, np.inf, dtype=np.float32))
    return {"index past the end": (batch, high, learner.INVALID), "negative index": (batch, low, learner.INVALID),
            "action past the end": (bad_action, indices[0], learner.INVALID),
            "negative action": (negative_action, indices[0], learner.INVALID),
            "infinite returns": (infinite, indices[0], learner.NONFINITE)}


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
def e2e_permutations(iteration):
    rng = np.random.default_rng(900 + iteration)
    return np.stack([rng.permutation(T * E2E_ENVS) for _ in range(E2E_EPOCHS)]).astype(np.int64)


def train_runs(rollout, policy, learner, reset, unwrap, permutations_of, trains=1):
    """E2E_ITERATIONS iterations of collect + train: per iteration the rollout's slabs, the parameters, the optimizer
    state and the stats, unwrapped."""
    obs = reset()
    seen = []
    for iteration in range(E2E_ITERATIONS):
        rollout.start(obs if iteration == 0 else None)
        rollout.collect(policy)
        record = policy_cases.slabs_of(rollout, unwrap)
        for train in range(trains):
            stats = learner.train(rollout, E2E_EPOCHS, E2E_BATCH, permutations=permutations_of(iteration))
            record[f"stats/{train}"] = unwrap(stats)
        record["params"], record["state"] = unwrap(policy.params), unwrap(learner.state)
        seen.append(record)
    return seen


LEARNER_KW = dict(learning_rate=1e-2, ent_coef=0.01)


@functools.lru_cache(maxsize=None)
def twin_train_runs(kind, trains=1):
    from reinfocus_amd.environments import harness

    env = policy_cases.make_env(kind, E2E_ENVS, False)
    try:
        spec = policy_cases.e2e_spec(kind)
        policy = harness.Policy(spec, policy_cases.SEED)
        policy.load_state_dict(policy_cases.state_dict(spec, 3))
        learner = harness.Learner(policy, **LEARNER_KW)
        rollout = harness.Rollout(env, T, GAMMA, GAE_LAMBDA)
        return train_runs(rollout, policy, learner, lambda: env.reset()[0], np.array, e2e_permutations, trains)
    finally:
        env.close()


same_runs = rollout_cases.same_runs


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
def _guarded(torch, array):
    """(whole, view): a device copy of the float32 array with GUARD sentinel floats on either side."""
    whole = torch.full((array.size + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    view = whole[GUARD:GUARD + array.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(array, dtype=np.float32).reshape(-1)))
    return whole, view


def _guards_kept(whole):
    raw = whole.cpu().numpy().view(np.uint32)
    return bool((raw[:GUARD] == SENTINEL).all() and (raw[-GUARD:] == SENTINEL).all())


class _Device:
    """One update's device arrays: outputs between guards, inputs as they are."""

    def __init__(self, torch, ctx, spec, params, state, batch, max_batch=None):
        """The workspace has exactly rf_ppo_workspace_size(max_batch) bytes between its guards (RF_PPO_MAX_BATCH's
        where none is given)."""
        from reinfocus_amd.environments import learner

        self.torch, self.ctx, self.spec = torch, ctx, spec
        self.whole = {}
        self.whole["params"], self.params = _guarded(torch, params)
        self.whole["state"], self.state = _guarded(torch, state)
        self.whole["stats"], self.stats = _guarded(torch, np.zeros(8, dtype=np.float32))
        self.stats.view(torch.int32).fill_(SENTINEL)
        floats = ctx.ppo_workspace_size(spec.desc(), max_batch or learner.MAX_BATCH) // 4
        assert floats > 0 and ctx.ppo_state_size(spec.desc()) == 4 * state.size
        assert ctx.ppo_workspace_size(spec.desc(), min(65, max_batch or 65)) <= 4 * floats
        self.whole["workspace"], self.workspace = _guarded(torch, np.zeros(floats, dtype=np.float32))
        self.load(batch)

    def load(self, batch):
        self.batch = {key: self.torch.from_numpy(value).cuda() for key, value in batch.items()}
        self.rows = batch["actions"].shape[0]

    def call(self, chosen, hyper, **changed):
        a = dict(desc=self.spec.desc(), hyper=tuple(hyper), params=self.params.data_ptr(), state=self.state.data_ptr(),
                 workspace=self.workspace.data_ptr(), rows=self.rows, obs=self.batch["observations"].data_ptr(),
                 actions=self.batch["actions"].data_ptr(), log_probs=self.batch["log_probs"].data_ptr(),
                 advantages=self.batch["advantages"].data_ptr(), returns=self.batch["returns"].data_ptr(),
                 batch=chosen.numel(), index=chosen.data_ptr(), stats=self.stats.data_ptr())
        a.update(changed)  # (arguments given by their names above, in place of the tensors')
        self.ctx.ppo_update(a["desc"], a["hyper"], a["params"], a["state"], a["workspace"], a["rows"], a["obs"],
                            a["actions"], a["log_probs"], a["advantages"], a["returns"], a["batch"], a["index"], a["stats"],
                            self.torch.cuda.current_stream().cuda_stream)

    def outputs(self):
        self.torch.cuda.synchronize()
        return self.params.cpu().numpy(), self.state.cpu().numpy(), self.stats.cpu().numpy()

    def guards_kept(self):
        return all(_guards_kept(whole) for whole in self.whole.values())


def _same_update(got, want, what):
    from reinfocus_amd.environments import learner

    size = want[0].size
    head = learner.STATE_HEADER
    assert bits(got[0]) == bits(want[0]), f"{what}: params differ"
    assert bits(got[1][:head]) == bits(want[1][:head]), f"{what}: the header differs"
    assert bits(got[1][head:head + size]) == bits(want[1][head:head + size]), f"{what}: m differs"
    assert bits(got[1][head + size:]) == bits(want[1][head + size:]), f"{what}: v differs"
    assert bits(got[2]) == bits(want[2]), f"{what}: stats differ: {got[2]} / {want[2]}"


def kernel_case(torch, ctx, index, count, max_batch=None):
    """rf_ppo_update against ppo_update_numpy as bytes over UPDATES consecutive updates."""
    from reinfocus_amd.environments import learner

    spec, params, batch, indices = update_inputs(index, count)
    want = twin_updates(index, count)
    device = _Device(torch, ctx, spec, params, learner.fresh_state(spec), batch, max_batch)
    for update in range(UPDATES):
        device.call(torch.from_numpy(indices[update]).cuda(), hyper_of(update))
        _same_update(device.outputs(), want[update], f"update {update}")
    assert device.guards_kept(), "a guard was written"
    # one norm that clips, one that does not (at the batch limits tests/test_learner_logic.py says which cases hold it)
    assert max_batch or want[2][2][5] > SCHEDULE[2][0] and want[1][2][5] < SCHEDULE[1][0]


def skip_case(torch, ctx):
    """An invalid index, an invalid action and a non-finite norm: nothing changes but the stats, the flag is set, and
    the next valid update is taken."""
    from reinfocus_amd.environments import learner

    index, count = 1, TILE + 1
    spec, params, batch, indices = update_inputs(index, count)
    want = twin_updates(index, count)
    device = _Device(torch, ctx, spec, params, learner.fresh_state(spec), batch)
    device.call(torch.from_numpy(indices[0]).cuda(), hyper_of(0))
    _same_update(device.outputs(), want[0], "the first update")
    for name, (changed, chosen, flag) in skip_variants(batch, indices).items():
        device.load(changed)
        device.call(torch.from_numpy(chosen).cuda(), hyper_of(1))
        twin = learner.ppo_update_numpy(spec, want[0][0], want[0][1], changed, chosen, hyper_of(1))
        assert twin[2][7] == flag and bits(twin[0]) == bits(want[0][0]) and bits(twin[1]) == bits(want[0][1]), name
        _same_update(device.outputs(), twin, name)
    device.load(batch)
    device.call(torch.from_numpy(indices[1]).cuda(), hyper_of(1))
    _same_update(device.outputs(), want[1], "the update after the skipped ones")
    assert device.guards_kept()


def refusal_case(torch, ctx):
    """Each refusal leaves parameters, state and stats as they were: nothing was enqueued."""
    from reinfocus_amd.environments import learner

    index, count = 2, TILE + 1
    spec, params, batch, indices = update_inputs(index, count)
    want = twin_updates(index, count)
    device = _Device(torch, ctx, spec, params, learner.fresh_state(spec), batch)
    chosen = torch.from_numpy(indices[0]).cuda()
    before = None

    def refused(match, **changed):
        hyper = changed.pop("hyper", hyper_of(0))
        try:
            device.call(chosen, hyper, **changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        got = device.outputs()
        assert all(bits(x) == bits(y) for x, y in zip(got, before)), f"an output was written ({match})"

    before = device.outputs()
    assert (before[2].view(np.uint32) == SENTINEL).all()
    desc = list(spec.desc())
    for field, value in ((0, 0), (0, 257), (1, 1), (1, 65), (2, 2), (3, 0), (3, 3), (4, 257), (6, 3), (7, 0)):
        refused("outside the limits", desc=tuple(desc[:field] + [value] + desc[field + 1:]))
    refused("at least 1", rows=0)
    refused("is not in 1 ..", batch=0)
    refused("is not in 1 ..", batch=1025)
    for field in range(8):
        refused("hyper-parameter", hyper=hyper_of(0)._replace(**{learner.Hyper._fields[field]: -1.0}))
        refused("hyper-parameter", hyper=hyper_of(0)._replace(**{learner.Hyper._fields[field]: float("nan")}))
    refused("hyper-parameter", hyper=hyper_of(0)._replace(learning_rate=float("inf")))
    refused("hyper-parameter", hyper=hyper_of(0)._replace(beta1=1.0))
    refused("hyper-parameter", hyper=hyper_of(0)._replace(beta2=1.5))
    host = np.zeros(4 * spec.size + 64, dtype=np.float32)
    for name in ("params", "state", "workspace", "obs", "actions", "log_probs", "advantages", "returns", "index", "stats"):
        refused("NULL argument", **{name: None})
        refused("is not device memory", **{name: host.ctypes.data})
    refused("not aligned", obs=device.batch["observations"].data_ptr() + 2)
    refused("not aligned", index=chosen.data_ptr() + 4)
    refused("not aligned", state=device.state.data_ptr() + 4)
    refused("not aligned", workspace=device.workspace.data_ptr() + 4)
    block = torch.zeros(32 * 1024 * 1024, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    refused("fewer than", obs=end - 4 * (device.rows * spec.obs_width - 1))
    refused("fewer than", index=end - 8 * (count - 1))
    refused("fewer than", params=end - 4 * (spec.size - 1))
    refused("fewer than", state=end - 8 * spec.size)  # (a state that is too small)
    refused("fewer than", workspace=end - 1024)  # (a workspace that is too small)
    # a workspace sized for 512 rows offered for 513, which index the same rows again; sized for 513 it would do
    again = torch.from_numpy(np.resize(indices[0], 513)).cuda()
    sized = ctx.ppo_workspace_size(spec.desc(), 512)
    assert 0 < sized < ctx.ppo_workspace_size(spec.desc(), 513) and ctx.ppo_workspace_size(spec.desc(), 1025) == 0
    refused("fewer than", workspace=end - sized, batch=513, index=again.data_ptr())
    refused("is not in 1 ..", workspace=end - sized, batch=1025, index=again.data_ptr())
    refused("fewer than", stats=end - 16)
    refused("d_params overlaps d_obs", params=device.batch["observations"].data_ptr())
    refused("d_stats overlaps d_returns", stats=device.batch["returns"].data_ptr())
    refused("d_workspace overlaps d_index", workspace=chosen.data_ptr())
    refused("d_state overlaps d_params", state=device.params.data_ptr())
    refused("d_workspace overlaps d_state", workspace=device.state.data_ptr())
    refused("d_stats overlaps d_workspace", stats=device.workspace.data_ptr())
    device.call(chosen, hyper_of(0))  # ... and the same arguments unchanged are taken
    _same_update(device.outputs(), want[0], "the unchanged call")
    assert device.guards_kept()


def _device_pair(torch, harness, env, kind):
    spec = policy_cases.e2e_spec(kind)
    policy = harness.DevicePolicy(env, spec, policy_cases.SEED)
    policy.load_state_dict({k: torch.from_numpy(v).cuda() for k, v in policy_cases.state_dict(spec, 3).items()})
    return policy, harness.DeviceLearner(policy, **LEARNER_KW)


def _unwrap(tensor):
    return tensor.cpu().numpy()


def end_to_end_case(torch, kind):
    from reinfocus_amd.environments import harness

    want = twin_train_runs(kind)
    env = policy_cases.make_env(kind, E2E_ENVS, True)
    try:
        policy, learner = _device_pair(torch, harness, env, kind)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        got = train_runs(rollout, policy, learner, lambda: env.reset_tensors()[0], _unwrap,
                         lambda i: torch.from_numpy(e2e_permutations(i)).cuda())
        same_runs(got, want)
        assert env.device_fault() is None
        assert bits(want[0]["params"]) != bits(want[1]["params"]) and (want[1]["stats/0"][:, 7] == 0).all()
        assert want[0]["stats/0"].shape == (E2E_EPOCHS * 2, 8)
    finally:
        env.close()


def no_sync_case(torch):
    """Two train() calls per iteration enqueued back to back, nothing read in between; one synchronisation at the end."""
    from reinfocus_amd.environments import harness

    kind = "view"
    want = twin_train_runs(kind, 2)
    env = policy_cases.make_env(kind, E2E_ENVS, True)
    try:
        policy, learner = _device_pair(torch, harness, env, kind)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        obs = env.reset_tensors()[0]
        torch.cuda.synchronize()
        rollout.start(obs)
        rollout.collect(policy)
        permutations = torch.from_numpy(e2e_permutations(0)).cuda()
        first = learner.train(rollout, E2E_EPOCHS, E2E_BATCH, permutations=permutations)
        second = learner.train(rollout, E2E_EPOCHS, E2E_BATCH, permutations=permutations)
        torch.cuda.synchronize()  # the only one
        assert bits(_unwrap(first)) == bits(want[0]["stats/0"]) and bits(_unwrap(second)) == bits(want[0]["stats/1"])
        assert bits(_unwrap(policy.params)) == bits(want[0]["params"])
        assert bits(_unwrap(learner.state)) == bits(want[0]["state"])
        # without permutations: torch.randperm on the device, and the stats say every update was taken
        stats = learner.train(rollout, 1, E2E_BATCH, generator=torch.Generator(device="cuda").manual_seed(3))
        assert stats.shape == (2, 8) and (_unwrap(stats)[:, 7] == 0).all()
        assert env.device_fault() is None
    finally:
        env.close()


def resume_case(torch):
    """state_dict / load_state_dict of the optimizer resumes bit for bit in a fresh learner."""
    from reinfocus_amd.environments import harness

    kind = "plain"
    env = policy_cases.make_env(kind, E2E_ENVS, True)
    try:
        policy, learner = _device_pair(torch, harness, env, kind)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        rollout.start(env.reset_tensors()[0])
        rollout.collect(policy)
        permutations = torch.from_numpy(e2e_permutations(0)).cuda()
        learner.train(rollout, E2E_EPOCHS, E2E_BATCH, permutations=permutations)
        kept, kept_params = learner.state_dict(), policy.state_dict()
        assert kept["step"] == 2 * E2E_EPOCHS
        straight = _unwrap(learner.train(rollout, E2E_EPOCHS, E2E_BATCH, permutations=permutations))
        want = _unwrap(policy.params), _unwrap(learner.state)
        policy.load_state_dict(kept_params)
        fresh = harness.DeviceLearner(policy, **LEARNER_KW)
        fresh.load_state_dict(kept)
        resumed = _unwrap(fresh.train(rollout, E2E_EPOCHS, E2E_BATCH, permutations=permutations))
        assert bits(resumed) == bits(straight)
        assert bits(_unwrap(policy.params)) == bits(want[0]) and bits(_unwrap(fresh.state)) == bits(want[1])
    finally:
        env.close()


def surface_case(torch):
    """The refusals of the Python surface, and update() by itself."""
    from reinfocus_amd.environments import harness
    from reinfocus_amd.environments import learner as learner_module

    try:
        harness.DeviceLearner(harness.Policy(policy_cases.e2e_spec("plain"), 0))
    except TypeError as caught:
        assert "DevicePolicy" in str(caught)
    else:
        raise AssertionError("a numpy Policy was taken")
    env = policy_cases.make_env("plain", E2E_ENVS, True)
    jumps = harness.DeviceVectorContinuousJumps(num_envs=2, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        policy, learner = _device_pair(torch, harness, env, "plain")
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        rollout.start(env.reset_tensors()[0])
        for wrong, error, match in ((rollout, ValueError, "not finished"),
                                    (harness.DeviceRollout(jumps, T, GAMMA, GAE_LAMBDA), ValueError, "out of scope")):
            try:
                learner.train(wrong, 1, E2E_BATCH)
            except error as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"taken ({match})")
        rollout.collect(policy)
        for bad in (dict(n_epochs=0, batch_size=16), dict(n_epochs=1, batch_size=0), dict(n_epochs=1, batch_size=1025)):
            try:
                learner.train(rollout, **bad)
            except ValueError:
                pass
            else:
                raise AssertionError(f"taken ({bad})")
        learner.learning_rate = -1.0
        try:
            learner.train(rollout, 1, E2E_BATCH)
        except ValueError as caught:
            assert "hyper-parameter" in str(caught)
        else:
            raise AssertionError("a negative learning rate was taken")
        learner.learning_rate = 3e-4  # (a plain attribute, changed between calls)
        flat = rollout.flat()
        twin_flat = {key: _unwrap(value) for key, value in flat.items()}
        index = torch.arange(5, dtype=torch.int64, device="cuda")
        params = _unwrap(policy.params)
        stats = learner.update(flat, index)
        want = learner_module.ppo_update_numpy(policy.spec, params, learner_module.fresh_state(policy.spec), twin_flat,
                                               np.arange(5), learner.hyper())
        _same_update((_unwrap(policy.params), _unwrap(learner.state), _unwrap(stats)), want, "update()")
        for bad, error in ((index.cpu(), ValueError), (index.int(), ValueError), (np.arange(5), TypeError)):
            try:
                learner.update(flat, bad)
            except error:
                pass
            else:
                raise AssertionError("an index of another kind was taken")
    finally:
        env.close()
        jumps.close()


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    ctx = _native.Context(0)
    for index in range(len(NETWORKS)):
        for count in BATCHES:
            with record.case(f"kernel/{index}/{count}"):
                kernel_case(torch, ctx, index, count)
    for index, count in LIMIT_CASES:
        with record.case(f"kernel/{index}/{count}"):
            kernel_case(torch, ctx, index, count, count)
    with record.case("skips"):
        skip_case(torch, ctx)
    with record.case("refusals"):
        refusal_case(torch, ctx)
    ctx.close()
    for kind in E2E_KINDS:
        with record.case(f"end-to-end/{kind}"):
            end_to_end_case(torch, kind)
    with record.case("no-sync"):
        no_sync_case(torch)
    with record.case("resume"):
        resume_case(torch)
    with record.case("surface"):
        surface_case(torch)
    with record.case("finished"):
        pass


# ---- torch on the CPU: stable-baselines3's loss, autograd, clip_grad_norm_ and Adam ------------------------------------
def torch_learner(path_in, path_out):
    """From a state_dict and one minibatch: the packed gradient before clipping and the packed parameters after 1 and
    after `updates` updates on that minibatch, in float64 and in float32.  In a process of its own: torch brings a HIP
    runtime of its own."""
    import torch

    data = np.load(path_in)
    names = [str(name) for name in data["names"]]
    activation = torch.nn.Tanh if str(data["activation"]) == "tanh" else torch.nn.ReLU
    clip_range, ent_coef, vf_coef, max_grad_norm, learning_rate = (float(data[k]) for k in (
        "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "learning_rate"))
    updates = int(data["updates"])
    out = {}
    for label, dtype in (("64", torch.float64), ("32", torch.float32)):
        tensors = {name: torch.from_numpy(data[name]).to(dtype) for name in names}

        def net(extractor, head_name):
            layers = []
            keys = [f"mlp_extractor.{extractor}.{i}" for i in (0, 2) if f"mlp_extractor.{extractor}.{i}.weight" in tensors]
            for key in keys + [head_name]:
                weight = tensors[key + ".weight"]
                linear = torch.nn.Linear(weight.shape[1], weight.shape[0]).to(dtype)
                with torch.no_grad():
                    linear.weight.copy_(weight)
                    linear.bias.copy_(tensors[key + ".bias"])
                layers += [linear, activation()]
            return torch.nn.Sequential(*layers[:-1]), keys + [head_name]

        (pi, pi_keys), (vf, vf_keys) = net("policy_net", "action_net"), net("value_net", "value_net")
        modules = dict(zip(pi_keys + vf_keys, [m for m in pi if isinstance(m, torch.nn.Linear)]
                           + [m for m in vf if isinstance(m, torch.nn.Linear)]))

        def packed(grad):
            parts = []
            for name in names:
                key, part = name.rsplit(".", 1)
                tensor = getattr(modules[key], part)
                tensor = tensor.grad if grad else tensor.detach()
                parts.append((tensor.t() if part == "weight" else tensor).reshape(-1))
            return torch.cat(parts).numpy().copy()

        obs = torch.from_numpy(data["obs"]).to(dtype)
        actions = torch.from_numpy(data["actions"])
        old, advantages, returns = (torch.from_numpy(data[k]).to(dtype) for k in ("old_log_probs", "advantages", "returns"))
        parameters = list(pi.parameters()) + list(vf.parameters())
        optimizer = torch.optim.Adam(parameters, lr=learning_rate, eps=1e-5)
        for update in range(updates):
            adv = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
            distribution = torch.distributions.Categorical(logits=pi(obs))
            log_prob = distribution.log_prob(actions)
            ratio = torch.exp(log_prob - old)
            policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
            value_loss = torch.nn.functional.mse_loss(returns, vf(obs).flatten())
            loss = policy_loss + ent_coef * -distribution.entropy().mean() + vf_coef * value_loss
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


def torch_subgradient(path_in, path_out):
    """d min(A r, A clamp(r, 1 - c, 1 + c)) / d r by autograd, float32, r and A given."""
    import torch

    data = np.load(path_in)
    ratio = torch.from_numpy(data["ratio"]).requires_grad_(True)
    adv = torch.from_numpy(data["adv"])
    c = torch.tensor(float(data["clip_range"]), dtype=torch.float32)
    torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).sum().backward()
    np.savez(path_out, slope=ratio.grad.numpy())


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "--torch-learner":
        torch_learner(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "--torch-subgradient":
        torch_subgradient(sys.argv[2], sys.argv[3])
    else:
        run_cases(sys.argv[1])
