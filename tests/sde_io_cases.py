"""TEST INFRASTRUCTURE: what tests/test_sde_logic.py and tests/test_gpu_sde.py share -- the networks, sizes and hostile
inputs of the sde policy (include/reinfocus_hip.h, "sde policy"), the numpy twin's results (computed once and shared),
the drivers of the end-to-end runs -- and the child process of the GPU file.

As tests/learner_io_cases.py: everything that needs torch and the library together runs in one fresh process that imports
torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.sde_io_cases <results.jsonl>
    python -m tests.sde_io_cases --torch-learner <in.npz> <out.npz>    (torch on the CPU: Normal, autograd, Adam)
"""

import functools
import os
import sys

import numpy as np

from tests import learner_io_cases as learner_cases
from tests import policy_io_cases as policy_cases
from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = policy_cases.TILE
SIZES = (1, TILE - 1, TILE, TILE + 1)  # one environment; the tile of 8 ragged on both sides, and full
# (obs_width, pi, vf, activation): a single-unit latent; SB3's default in both activations with a vf of another depth;
# the widest
NETWORKS = ((3, (1,), (2, 2), "tanh"),
            (20, (64, 64), (64,), "relu"),
            (20, (64, 64), (64,), "tanh"),
            (20, (256, 256), (256, 256), "relu"))
BATCHES = (1, 2, 64, 512)  # one sample, a pair, 8 tiles, the reference's minibatch (and a two-level Adam reduction)
# at the limits, as learner_io_cases.LIMIT_CASES (512 is above): the first size whose reductions take a second trip, one
# that is no multiple of the tile, RF_PPO_MAX_BATCH; on the single-unit latent and SB3's default in both activations, and
# at 513 on the widest
LIMIT_CASES = tuple((index, count) for index in (0, 1, 2) for count in (513, 1000, 1024)) + ((3, 513),)
UPDATES, SCHEDULE, SHIFTS = learner_cases.UPDATES, learner_cases.SCHEDULE, learner_cases.SHIFTS
OFFSETS = policy_cases.OFFSETS
SEED, SENTINEL, GUARD = policy_cases.SEED, policy_cases.SENTINEL, learner_cases.GUARD
T, STACK, GAMMA, GAE_LAMBDA = rollout_cases.T, rollout_cases.STACK, rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA
E2E_ENVS, E2E_ITERATIONS, E2E_EPOCHS, E2E_BATCH = 4, 2, 2, 16  # 28 rows: minibatches of 16 and 12
E2E_KINDS = {"view": dict(view=True, records=True), "records": dict(view=False, records=True),
             "plain": dict(view=False, records=False)}
E2E_FREQ = 3
LEARNER_KW = learner_cases.LEARNER_KW
FORWARD_OUTPUTS = ("actions", "env_actions", "log_probs", "values", "final_values", "mean", "sigma")

bits = policy_cases.bits
hyper_of = learner_cases.hyper_of
same_runs = rollout_cases.same_runs


def spec_of(network, log_std_init=0.0):
    from reinfocus_amd.environments import sde

    width, pi, vf, activation = network
    return sde.SdePolicySpec(width, pi=pi, vf=vf, activation=activation, log_std_init=log_std_init)


def state_dict(spec, seed, hostile=False):
    """policy_io_cases.state_dict's weights with log_std uniform in [-1.5, 0.5]; hostile: its first rows are -100 (a
    standard deviation of 0), 0 and +3 (one of 20: raw actions far past +-1) -- a single row is +3."""
    out = {name: value for name, value in policy_cases.state_dict(_Entries(spec), seed).items()}
    rng = np.random.default_rng(seed + 5000)
    log_std = rng.uniform(-1.5, 0.5, (spec.latent, 1)).astype(np.float32)
    if hostile:
        special = np.array([-100.0, 0.0, 3.0], dtype=np.float32)[-min(3, spec.latent):]
        log_std[:special.size, 0] = special
    out["log_std"] = log_std
    return out


class _Entries:
    """The entries of the two nets alone (log_std is no weight matrix of a layer)."""

    def __init__(self, spec):
        self.entries = [entry for entry in spec.entries if entry[0] != "log_std"]


def observations(width, n, seed):
    """hostile rows (+-0, subnormals, large values, infinities, a NaN cell) and -- from 7 rows on -- one row that is NaN
    throughout."""
    rows = policy_cases.hostile_rows(width, n, seed, False)
    if n >= TILE - 1:
        rows[n // 2] = np.nan
    return rows


@functools.lru_cache(maxsize=None)
def forward_inputs(index, n):
    network = NETWORKS[index]
    spec = spec_of(network)
    params = spec.pack(state_dict(spec, 300 + index, hostile=True))
    return spec, params, observations(network[0], n, 2000 * index + n), policy_cases.hostile_rows(network[0], n, 9 + n, True)


@functools.lru_cache(maxsize=None)
def wanted_forward(index, n, offset):
    """(theta, the sampled call, the deterministic call) of the twin, with the generator `offset` draws in."""
    from reinfocus_amd.environments import sde

    spec, params, obs, final_obs = forward_inputs(index, n)
    generator = policy_cases.generator_at(offset)[1]
    theta = sde.noise_numpy(params[spec.log_std_at:], generator.random(n * spec.latent))
    return (theta, sde.sde_numpy(spec, params, obs, final_obs, theta),
            sde.sde_numpy(spec, params, obs, final_obs, None, deterministic=True))


@functools.lru_cache(maxsize=None)
def update_inputs(index, count):
    """(spec, packed parameters, batch dict of N = count + 3 finite rows, [UPDATES] index arrays).  The stored actions
    are the twin's own sampled raw actions (some past +-1), the stored log-probabilities its own shifted by SHIFTS in
    turn; every index array is part of a permutation with its last entry repeated from its first."""
    from reinfocus_amd.environments import sde

    network = NETWORKS[index]
    spec = spec_of(network)
    params = spec.pack(state_dict(spec, 400 + index, hostile=spec.latent > 1))
    rows = count + 3
    rng = np.random.default_rng(3000 * index + count)
    obs = learner_cases.finite_rows(network[0], rows, 91 * index + count)
    theta = sde.noise_numpy(params[spec.log_std_at:], rng.random(rows * spec.latent))
    got = sde.sde_numpy(spec, params, obs, None, theta)
    shifts = np.array(SHIFTS, dtype=np.float32)[np.arange(rows) % len(SHIFTS)]
    batch = {"observations": obs, "actions": got["actions"], "log_probs": (got["log_probs"] - shifts).astype(np.float32),
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
    """[(params, state, stats)] after each of UPDATES consecutive updates by the numpy twin, computed once."""
    from reinfocus_amd.environments import learner

    spec, params, batch, indices = update_inputs(index, count)
    state = learner.fresh_state(spec)
    seen = []
    for update in range(UPDATES):
        params, state, stats = learner.ppo_update_numpy(spec, params, state, batch, indices[update], hyper_of(update))
        seen.append((params, state, stats))
    return seen


def skip_variants(spec, params, batch, indices):
    """{name: (params, batch, index, flag)} of updates that must change nothing."""
    from reinfocus_amd.environments import learner

    rows = batch["actions"].shape[0]
    high, low = indices[0].copy(), indices[0].copy()
    high[0], low[-1] = rows, -1
    nan_action = dict(batch, actions=batch["actions"].copy())
    nan_action["actions"][indices[0][0]] = np.nan
    infinite = dict(batch, returns=np.full(rows, np.inf, dtype=np.float32))
    wide = params.copy()
    wide[spec.log_std_at:] = np.float32(90.0)  # (std = 1 / exp32(-90) = +inf: sigma is infinite in every row)
    return {"index past the end": (params, batch, high, learner.INVALID),
            "negative index": (params, batch, low, learner.INVALID),
            "NaN action": (params, nan_action, indices[0], learner.INVALID),
            "infinite returns": (params, infinite, indices[0], learner.NONFINITE),
            "log_std of 90": (wide, batch, indices[0], learner.NONFINITE)}


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
def make_env(kind, n, device_form):
    from reinfocus_amd.environments import harness

    what = E2E_KINDS[kind]
    extra = dict(episode_records=what["records"],
                 learner_view=harness.LearnerView(frame_stack=STACK) if what["view"] else None)
    if device_form:
        return harness.DeviceVectorContinuousJumps(num_envs=n, device_initializer=True, **rollout_cases.ENV_KW, **extra)
    return harness.VectorContinuousJumps(num_envs=n, **rollout_cases.ENV_KW, **extra)


def e2e_spec(env):
    from reinfocus_amd.environments import sde

    return sde.SdePolicySpec(int(env.single_observation_space.shape[0]), pi=(64, 64), vf=(64, 64), activation="relu",
                             log_std_init=-0.5)


def e2e_state(spec):
    state = state_dict(spec, 3)
    state["log_std"][:] = np.float32(spec.log_std_init)
    return state


e2e_permutations = learner_cases.e2e_permutations


def train_runs(rollout, policy, learner, reset, unwrap, permutations_of, freq, iterations=E2E_ITERATIONS, seen=None,
               first=0):
    """Iterations of collect(sde_sample_freq=freq) + train: per iteration the rollout's slabs, theta, the parameters, the
    optimizer state and the stats, unwrapped."""
    seen = [] if seen is None else seen
    obs = reset() if first == 0 else None
    for iteration in range(first, iterations):
        rollout.start(obs if iteration == 0 else None)
        rollout.collect(policy, sde_sample_freq=freq)
        record = policy_cases.slabs_of(rollout, unwrap)
        record["theta"] = unwrap(policy.noise())
        record["stats"] = unwrap(learner.train(rollout, E2E_EPOCHS, E2E_BATCH, permutations=permutations_of(iteration)))
        record["params"], record["state"] = unwrap(policy.params), unwrap(learner.state)
        seen.append(record)
    return seen


@functools.lru_cache(maxsize=None)
def twin_train_runs(kind, freq, iterations=E2E_ITERATIONS):
    from reinfocus_amd.environments import harness

    env = make_env(kind, E2E_ENVS, False)
    try:
        spec = e2e_spec(env)
        policy = harness.SdePolicy(spec, SEED)
        policy.load_state_dict(e2e_state(spec))
        learner = harness.Learner(policy, **LEARNER_KW)
        rollout = harness.Rollout(env, T, GAMMA, GAE_LAMBDA)
        return train_runs(rollout, policy, learner, lambda: env.reset()[0], np.array, e2e_permutations, freq, iterations)
    finally:
        env.close()


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
_guarded, _guards_kept = learner_cases._guarded, learner_cases._guards_kept


def _unwrap(tensor):
    return tensor.cpu().numpy()


def _sentinels(torch, count):
    whole, view = _guarded(torch, np.zeros(count, dtype=np.float32))
    view.view(torch.int32).fill_(SENTINEL)
    return whole, view


def forward_case(torch, ctx, index, n):
    """rf_sde_noise_reset and rf_sde_forward against the twin as bytes: a reset at both draw offsets, a sampled call, a
    deterministic call, a values-only call; every output between guards."""
    spec, params, obs, final_obs = forward_inputs(index, n)
    d_params, d_obs, d_final = (torch.from_numpy(a).cuda() for a in (params, obs, final_obs))
    stream = torch.cuda.current_stream().cuda_stream
    assert ctx.sde_params_size(spec.desc()) == spec.size
    for offset in OFFSETS:
        theta, sampled, deterministic = wanted_forward(index, n, offset)
        bit_generator = policy_cases.generator_at(offset)[0]
        from reinfocus_amd.environments import policy

        whole_theta, d_theta = _sentinels(torch, n * spec.latent)
        ctx.sde_noise_reset(spec.desc(), d_params.data_ptr(), n, policy.generator_words(bit_generator), d_theta.data_ptr(),
                            stream)
        assert bits(_unwrap(d_theta).reshape(n, spec.latent)) == bits(theta), f"theta differs (offset {offset})"
        assert _guards_kept(whole_theta)
        for want, flags, noise in ((sampled, 0, d_theta), (deterministic, 1, None)):
            outs = {name: _sentinels(torch, n) for name in FORWARD_OUTPUTS}
            ctx.sde_forward(spec.desc(), d_params.data_ptr(), n, d_obs.data_ptr(), d_final.data_ptr(),
                            None if noise is None else noise.data_ptr(), flags,
                            *(outs[name][1].data_ptr() for name in FORWARD_OUTPUTS), stream)
            for name in FORWARD_OUTPUTS:
                assert bits(_unwrap(outs[name][1])) == bits(want[name]), f"{name} differ (offset {offset}, flags {flags})"
                assert _guards_kept(outs[name][0]), name
    # values only: the pi outputs are not asked for and no theta is needed
    whole, values = _sentinels(torch, n)
    ctx.sde_forward(spec.desc(), d_params.data_ptr(), n, d_obs.data_ptr(), None, None, 0, None, None, None,
                    values.data_ptr(), None, None, None, stream)
    assert bits(_unwrap(values)) == bits(sampled["values"]) and _guards_kept(whole)


class _Device(learner_cases._Device):
    """One update's device arrays, for rf_sde_update."""

    def __init__(self, torch, ctx, spec, params, state, batch, max_batch=None):
        from reinfocus_amd.environments import learner

        self.torch, self.ctx, self.spec = torch, ctx, spec
        self.whole = {}
        self.whole["params"], self.params = _guarded(torch, params)
        self.whole["state"], self.state = _guarded(torch, state)
        self.whole["stats"], self.stats = _sentinels(torch, 8)
        floats = ctx.sde_workspace_size(spec.desc(), max_batch or learner.MAX_BATCH) // 4
        assert floats > 0 and ctx.sde_state_size(spec.desc()) == 4 * state.size
        assert ctx.sde_workspace_size(spec.desc(), min(65, max_batch or 65)) <= 4 * floats
        self.whole["workspace"], self.workspace = _guarded(torch, np.zeros(floats, dtype=np.float32))
        self.load(batch)

    def call(self, chosen, hyper, **changed):
        a = dict(desc=self.spec.desc(), hyper=tuple(hyper), params=self.params.data_ptr(), state=self.state.data_ptr(),
                 workspace=self.workspace.data_ptr(), rows=self.rows, obs=self.batch["observations"].data_ptr(),
                 actions=self.batch["actions"].data_ptr(), log_probs=self.batch["log_probs"].data_ptr(),
                 advantages=self.batch["advantages"].data_ptr(), returns=self.batch["returns"].data_ptr(),
                 batch=chosen.numel(), index=chosen.data_ptr(), stats=self.stats.data_ptr())
        a.update(changed)
        self.ctx.sde_update(a["desc"], a["hyper"], a["params"], a["state"], a["workspace"], a["rows"], a["obs"],
                            a["actions"], a["log_probs"], a["advantages"], a["returns"], a["batch"], a["index"], a["stats"],
                            self.torch.cuda.current_stream().cuda_stream)


_same_update = learner_cases._same_update


def update_case(torch, ctx, index, count, max_batch=None):
    """rf_sde_update against the twin as bytes over UPDATES consecutive updates; with max_batch the workspace has exactly
    rf_sde_workspace_size(max_batch) bytes between its guards."""
    from reinfocus_amd.environments import learner

    spec, params, batch, indices = update_inputs(index, count)
    want = twin_updates(index, count)
    device = _Device(torch, ctx, spec, params, learner.fresh_state(spec), batch, max_batch)
    for update in range(UPDATES):
        device.call(torch.from_numpy(indices[update]).cuda(), hyper_of(update))
        _same_update(device.outputs(), want[update], f"update {update}")
    assert device.guards_kept(), "a guard was written"


def skip_case(torch, ctx):
    from reinfocus_amd.environments import learner

    index, count = 2, 64
    spec, params, batch, indices = update_inputs(index, count)
    want = twin_updates(index, count)
    device = _Device(torch, ctx, spec, params, learner.fresh_state(spec), batch)
    device.call(torch.from_numpy(indices[0]).cuda(), hyper_of(0))
    _same_update(device.outputs(), want[0], "the first update")
    for name, (start, changed, chosen, flag) in skip_variants(spec, want[0][0], batch, indices).items():
        device.params.copy_(torch.from_numpy(start))
        device.load(changed)
        device.call(torch.from_numpy(chosen).cuda(), hyper_of(1))
        twin = learner.ppo_update_numpy(spec, start, want[0][1], changed, chosen, hyper_of(1))
        assert twin[2][7] == flag and bits(twin[0]) == bits(start) and bits(twin[1]) == bits(want[0][1]), name
        _same_update(device.outputs(), twin, name)
    device.params.copy_(torch.from_numpy(want[0][0]))
    device.load(batch)
    device.call(torch.from_numpy(indices[1]).cuda(), hyper_of(1))
    _same_update(device.outputs(), want[1], "the update after the skipped ones")
    assert device.guards_kept()


def refusal_case(torch, ctx):
    """The refusals of the three new entry points: each leaves every output as it was."""
    from reinfocus_amd.environments import learner, policy

    index, count = 2, TILE + 1
    spec, params, batch, indices = update_inputs(index, count)
    device = _Device(torch, ctx, spec, params, learner.fresh_state(spec), batch)
    chosen = torch.from_numpy(indices[0][:count]).cuda()
    before = device.outputs()
    host = np.zeros(4 * spec.size + 64, dtype=np.float32)
    block = torch.zeros(32 * 1024 * 1024, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    end = block.data_ptr() + block.numel()
    desc = list(spec.desc())
    bad_descs = [tuple(desc[:field] + [value] + desc[field + 1:])
                 for field, value in ((0, 0), (0, 257), (1, 0), (1, 2), (2, 2), (3, 0), (3, 3), (4, 257), (6, 3), (7, 0))]

    def refused(call, match):
        try:
            call()
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")

    def update(match, **changed):
        hyper = changed.pop("hyper", hyper_of(0))
        refused(lambda: device.call(chosen, hyper, **changed), match)
        got = device.outputs()
        assert all(bits(x) == bits(y) for x, y in zip(got, before)), f"an output was written ({match})"

    for bad in bad_descs:
        update("outside the limits", desc=bad)
    update("at least 1", rows=0)
    update("is not in 1 ..", batch=0)
    update("is not in 1 ..", batch=1025)
    update("hyper-parameter", hyper=hyper_of(0)._replace(learning_rate=-1.0))
    update("hyper-parameter", hyper=hyper_of(0)._replace(beta1=1.0))
    for name in ("params", "state", "workspace", "obs", "actions", "log_probs", "advantages", "returns", "index", "stats"):
        update("NULL argument", **{name: None})
        update("is not device memory", **{name: host.ctypes.data})
    update("not aligned", actions=device.batch["actions"].data_ptr() + 2)
    update("not aligned", state=device.state.data_ptr() + 4)
    update("fewer than", actions=end - 4 * (device.rows - 1))
    update("fewer than", params=end - 4 * (spec.size - 1))  # (room for P but not for P + L would show here, too)
    update("fewer than", state=end - 8 * spec.size)
    # a workspace sized for 512 rows offered for 513, which index the same rows again
    again = torch.from_numpy(np.resize(indices[0][:count], 513)).cuda()
    sized = ctx.sde_workspace_size(spec.desc(), 512)
    assert 0 < sized < ctx.sde_workspace_size(spec.desc(), 513) and ctx.sde_workspace_size(spec.desc(), 1025) == 0
    update("fewer than", workspace=end - sized, batch=513, index=again.data_ptr())
    update("is not in 1 ..", workspace=end - sized, batch=1025, index=again.data_ptr())
    update("d_params overlaps d_obs", params=device.batch["observations"].data_ptr())
    update("d_state overlaps d_params", state=device.params.data_ptr())
    update("d_stats overlaps d_workspace", stats=device.workspace.data_ptr())

    # the reset and the forward
    n = TILE + 1
    fspec, fparams, obs, final_obs = forward_inputs(2, n)
    d_params, d_obs, d_final = (torch.from_numpy(a).cuda() for a in (fparams, obs, final_obs))
    stream = torch.cuda.current_stream().cuda_stream
    words = policy.generator_words(policy_cases.generator_at(0)[0])
    whole_theta, d_theta = _sentinels(torch, n * fspec.latent)
    outs = {name: _sentinels(torch, n) for name in FORWARD_OUTPUTS}
    theta_ok = torch.zeros(n * fspec.latent, dtype=torch.float32, device="cuda")

    def reset(match, **changed):
        a = dict(desc=fspec.desc(), params=d_params.data_ptr(), n=n, gen=words, theta=d_theta.data_ptr())
        a.update(changed)
        refused(lambda: ctx.sde_noise_reset(a["desc"], a["params"], a["n"], a["gen"], a["theta"], stream), match)
        assert (_unwrap(d_theta).view(np.uint32) == SENTINEL).all(), f"theta was written ({match})"

    def forward(match, **changed):
        a = dict(desc=fspec.desc(), params=d_params.data_ptr(), n=n, obs=d_obs.data_ptr(), final_obs=d_final.data_ptr(),
                 theta=theta_ok.data_ptr(), flags=0, **{name: outs[name][1].data_ptr() for name in FORWARD_OUTPUTS})
        a.update(changed)
        refused(lambda: ctx.sde_forward(a["desc"], a["params"], a["n"], a["obs"], a["final_obs"], a["theta"], a["flags"],
                                        *(a[name] for name in FORWARD_OUTPUTS), stream), match)
        for name in FORWARD_OUTPUTS:
            assert (_unwrap(outs[name][1]).view(np.uint32) == SENTINEL).all(), f"{name} were written ({match})"

    for bad in bad_descs:
        reset("outside the limits", desc=bad)
        forward("outside the limits", desc=bad)
    reset("at least 1", n=0)
    forward("at least 1", n=0)
    forward("unknown flags", flags=2)
    forward("needs d_final_obs", final_obs=None)
    forward("needs d_theta", theta=None)
    forward("no output", **{name: None for name in FORWARD_OUTPUTS})
    for name in ("params", "gen", "theta"):
        reset("NULL argument", **{name: None})
    for name in ("params", "theta"):
        reset("is not device memory", **{name: host.ctypes.data})
    reset("not aligned", theta=d_theta.data_ptr() + 2)
    reset("fewer than", theta=end - 4 * (n * fspec.latent - 1))
    reset("fewer than", params=end - 4 * (fspec.size - 1))
    reset("d_theta overlaps d_params", theta=d_params.data_ptr())
    for name in ("params", "obs"):
        forward("NULL argument", **{name: None})
    for name in ("params", "obs", "final_obs", "theta") + FORWARD_OUTPUTS:
        forward("is not device memory", **{name: host.ctypes.data})
    forward("not aligned", obs=d_obs.data_ptr() + 2)
    forward("not aligned", sigma=outs["sigma"][1].data_ptr() + 2)
    forward("fewer than", theta=end - 4 * (n * fspec.latent - 1))
    forward("fewer than", env_actions=end - 4 * (n - 1))
    forward("d_actions overlaps d_obs", actions=d_obs.data_ptr())
    forward("d_log_probs overlaps d_theta", log_probs=theta_ok.data_ptr())
    forward("overlaps d_actions", env_actions=outs["actions"][1].data_ptr())
    assert _guards_kept(whole_theta) and all(_guards_kept(outs[name][0]) for name in FORWARD_OUTPUTS)
    device.call(chosen, hyper_of(0))  # ... and the unchanged update is taken
    want = learner.ppo_update_numpy(spec, params, learner.fresh_state(spec), batch, indices[0][:count], hyper_of(0))
    _same_update(device.outputs(), want, "the unchanged call")
    assert device.guards_kept()


def _device_pair(torch, harness, env):
    spec = e2e_spec(env)
    policy = harness.DeviceSdePolicy(env, spec, SEED)
    policy.load_state_dict({k: torch.from_numpy(v).cuda() for k, v in e2e_state(spec).items()})
    return policy, harness.DeviceLearner(policy, **LEARNER_KW)


def end_to_end_case(torch, kind, freq):
    from reinfocus_amd.environments import harness

    want = twin_train_runs(kind, freq)
    env = make_env(kind, E2E_ENVS, True)
    try:
        policy, learner = _device_pair(torch, harness, env)
        before = policy.rng_state()["state"]["state"]
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        got = train_runs(rollout, policy, learner, lambda: env.reset_tensors()[0], _unwrap,
                         lambda i: torch.from_numpy(e2e_permutations(i)).cuda(), freq)
        same_runs(got, want)
        assert env.device_fault() is None
        assert bits(want[0]["params"]) != bits(want[1]["params"]) and (want[1]["stats"][:, 7] == 0).all()
        assert want[0]["stats"].shape == (E2E_EPOCHS * 2, 8)
        raw, clamped = want[0]["actions"], np.clip(want[0]["actions"], -1, 1)
        assert (raw != clamped).any(), "no raw action of the twin's rollout lies past +-1: the clamp is not exercised"
        # the generator moved by n * L per reset and by nothing else: 1 + ceil(T / freq) resets per collect
        resets = E2E_ITERATIONS * (1 + (-(-T // freq) if freq > 0 else 0))
        twin = np.random.PCG64DXSM(SEED)
        twin.advance(resets * E2E_ENVS * policy.spec.latent)
        assert policy.rng_state()["state"]["state"] == twin.state["state"]["state"] != before
    finally:
        env.close()


def no_sync_case(torch):
    """collect() + train() + collect() enqueued back to back, nothing read in between; one synchronisation at the end."""
    from reinfocus_amd.environments import harness

    kind = "view"
    want = twin_train_runs(kind, E2E_FREQ)
    env = make_env(kind, E2E_ENVS, True)
    try:
        policy, learner = _device_pair(torch, harness, env)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        obs = env.reset_tensors()[0]
        permutations = torch.from_numpy(e2e_permutations(0)).cuda()
        torch.cuda.synchronize()
        rollout.start(obs)
        rollout.collect(policy, sde_sample_freq=E2E_FREQ)
        stats = learner.train(rollout, E2E_EPOCHS, E2E_BATCH, permutations=permutations)
        rollout.start()
        rollout.collect(policy, sde_sample_freq=E2E_FREQ)
        torch.cuda.synchronize()  # the only one
        assert bits(_unwrap(stats)) == bits(want[0]["stats"]) and bits(_unwrap(policy.params)) == bits(want[0]["params"])
        for name in ("observations", "actions", "log_probs", "advantages", "returns"):
            assert bits(_unwrap(getattr(rollout, name))) == bits(want[1][name]), name
        assert env.device_fault() is None
    finally:
        env.close()


def resume_case(torch):
    """A fresh policy and learner rebuilt from state_dict + rng_state + noise() + the optimizer's state_dict: the next
    iteration equals the uninterrupted one."""
    from reinfocus_amd.environments import harness

    kind = "records"
    want = twin_train_runs(kind, -1, 3)  # (with -1 the second collect's first act would reuse theta were it not reset)
    env = make_env(kind, E2E_ENVS, True)
    try:
        policy, learner = _device_pair(torch, harness, env)
        rollout = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        permutations_of = lambda i: torch.from_numpy(e2e_permutations(i)).cuda()  # noqa: E731
        got = train_runs(rollout, policy, learner, lambda: env.reset_tensors()[0], _unwrap, permutations_of, -1, 2)
        kept = policy.state_dict(), policy.rng_state(), policy.noise(), learner.state_dict()
        fresh = harness.DeviceSdePolicy(env, policy.spec, 12345)
        fresh.load_state_dict(kept[0])
        fresh.set_rng_state(kept[1])
        fresh.set_noise(kept[2])
        assert bits(_unwrap(fresh.noise())) == bits(want[1]["theta"])
        fresh_learner = harness.DeviceLearner(fresh, **LEARNER_KW)
        fresh_learner.load_state_dict(kept[3])
        train_runs(rollout, fresh, fresh_learner, None, _unwrap, permutations_of, -1, 3, got, 2)
        same_runs(got, want)
    finally:
        env.close()


def surface_case(torch):
    """The refusals of the Python surface that need a device, and act() without out=."""
    from reinfocus_amd.environments import harness

    steps = harness.DeviceVectorDiscreteSteps(num_envs=2, device_initializer=True, **rollout_cases.ENV_KW)
    env = make_env("plain", E2E_ENVS, True)
    host_env = make_env("plain", 2, False)
    try:
        for build, error, match in (
                (lambda: harness.DeviceSdePolicy(steps, e2e_spec(steps), 0), ValueError, "Gaussian head"),
                (lambda: harness.DevicePolicy(env, policy_cases.e2e_spec("plain"), 0), ValueError, "out of scope"),
                (lambda: harness.DeviceSdePolicy(host_env, e2e_spec(env), 0), TypeError, "device-resident"),
                (lambda: harness.DeviceSdePolicy(env, policy_cases.e2e_spec("plain"), 0), TypeError, "SdePolicySpec")):
            try:
                build()
            except error as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"taken ({match})")
        policy, learner = _device_pair(torch, harness, env)
        obs = env.reset_tensors()[0]
        try:
            policy.act(obs)
        except ValueError as caught:
            assert "reset_noise" in str(caught)
        else:
            raise AssertionError("a sampled act() before reset_noise() was taken")
        before = policy.rng_state()["state"]["state"]
        actions, values, log_probs, final_values, env_actions = policy.act(obs, deterministic=True)
        assert policy.rng_state()["state"]["state"] == before and final_values is None
        twin = harness.SdePolicy(policy.spec, SEED)
        twin.load_state_dict(e2e_state(policy.spec))
        want = twin.act(_unwrap(obs), deterministic=True)
        for got, wanted in zip((actions, values, log_probs, env_actions), (want[0], want[1], want[2], want[4])):
            assert bits(_unwrap(got)) == bits(wanted)
        policy.reset_noise()
        twin.reset_noise(E2E_ENVS)
        assert bits(_unwrap(policy.noise())) == bits(twin.noise())
        assert bits(_unwrap(policy.act(obs)[0])) == bits(twin.act(_unwrap(obs))[0])
        # an sde learner given an int64 action slab; a Categorical one given the jumps rollout
        rollout = harness.DeviceRollout(steps, T, GAMMA, GAE_LAMBDA)
        flat = dict(observations=torch.zeros((4, policy.spec.obs_width), device="cuda"),
                    actions=torch.zeros(4, dtype=torch.int64, device="cuda"), log_probs=torch.zeros(4, device="cuda"),
                    advantages=torch.zeros(4, device="cuda"), returns=torch.zeros(4, device="cuda"))
        for call, match in ((lambda: learner.update(flat, torch.arange(4, device="cuda")), "int64 action slab"),
                            (lambda: learner.train(rollout, 1, 4), "Gaussian head")):
            try:
                call()
            except ValueError as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"taken ({match})")
    finally:
        env.close()
        steps.close()
        host_env.close()


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    ctx = _native.Context(0)
    for index in range(len(NETWORKS)):
        for n in SIZES:
            with record.case(f"forward/{index}/{n}"):
                forward_case(torch, ctx, index, n)
    for index in range(len(NETWORKS)):
        for count in BATCHES:
            with record.case(f"update/{index}/{count}"):
                update_case(torch, ctx, index, count)
    for index, count in LIMIT_CASES:
        with record.case(f"update/{index}/{count}"):
            update_case(torch, ctx, index, count, count)
    with record.case("skips"):
        skip_case(torch, ctx)
    with record.case("refusals"):
        refusal_case(torch, ctx)
    ctx.close()
    for kind in E2E_KINDS:
        with record.case(f"end-to-end/{kind}/{E2E_FREQ}"):
            end_to_end_case(torch, kind, E2E_FREQ)
    with record.case("end-to-end/records/-1"):
        end_to_end_case(torch, "records", -1)
    with record.case("no-sync"):
        no_sync_case(torch)
    with record.case("resume"):
        resume_case(torch)
    with record.case("surface"):
        surface_case(torch)
    with record.case("finished"):
        pass


# ---- torch on the CPU: stable-baselines3's sde distribution and loss, autograd, clip_grad_norm_ and Adam ---------------
def torch_learner(path_in, path_out):
    """From a state_dict and one minibatch: the packed gradient before clipping and the packed parameters after 1 and
    after `updates` updates on that minibatch, in float64 and in float32, with learn_features=False semantics: the latent
    is detached inside the variance and not in the mean.  In a process of its own."""
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
        log_std = torch.nn.Parameter(tensors["log_std"].clone())
        modules = dict(zip(pi_keys + vf_keys, [m for m in pi if isinstance(m, torch.nn.Linear)]
                           + [m for m in vf if isinstance(m, torch.nn.Linear)]))

        def packed(grad):
            parts = []
            for name in names:
                if name == "log_std":
                    tensor = log_std.grad if grad else log_std.detach()
                    parts.append(tensor.reshape(-1))
                    continue
                key, part = name.rsplit(".", 1)
                tensor = getattr(modules[key], part)
                tensor = tensor.grad if grad else tensor.detach()
                parts.append((tensor.t() if part == "weight" else tensor).reshape(-1))
            return torch.cat(parts).numpy().copy()

        obs = torch.from_numpy(data["obs"]).to(dtype)
        actions = torch.from_numpy(data["actions"]).to(dtype)
        old, advantages, returns = (torch.from_numpy(data[k]).to(dtype) for k in ("old_log_probs", "advantages", "returns"))
        parameters = list(pi.parameters()) + list(vf.parameters()) + [log_std]
        optimizer = torch.optim.Adam(parameters, lr=learning_rate, eps=1e-5)
        for update in range(updates):
            adv = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
            latent = pi[:-1](obs)
            mean = pi[-1](latent)[:, 0]
            # StateDependentNoiseDistribution.proba_distribution, full_std, learn_features=False
            variance = torch.mm(latent.detach() ** 2, torch.exp(log_std) ** 2)[:, 0]
            distribution = torch.distributions.Normal(mean, torch.sqrt(variance + 1e-6))
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


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "--torch-learner":
        torch_learner(sys.argv[2], sys.argv[3])
    else:
        run_cases(sys.argv[1])
