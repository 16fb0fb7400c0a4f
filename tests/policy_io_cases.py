"""TEST INFRASTRUCTURE: what tests/test_policy_logic.py and tests/test_gpu_policy.py share -- the networks, the sizes,
hostile inputs and parameters, the drivers of the end-to-end runs -- and the child process of the GPU file.

As tests/rollout_io_cases.py: everything that needs torch and the library together runs in one fresh process that imports
torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.policy_io_cases <results.jsonl>
"""

import os
import sys

import numpy as np

from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 8  # rf::kPolicyTile (tests/test_policy_logic.py reads csrc/rf_policy.h and compares)
SIZES = (1, TILE, TILE + 1, 3 * TILE + 5)
# (obs_width, pi, vf, n_actions, activation): the least network; stable-baselines3's default; ppo_tuned.yml's; widths
# that are no multiple of a wave, one and two layers mixed, the most actions; every limit at once
NETWORKS = ((1, (1,), (1,), 2, "relu"),
            (20, (64, 64), (64, 64), 13, "tanh"),
            (20, (256, 256), (256, 256), 13, "relu"),
            (7, (65,), (3, 200), 64, "tanh"),
            (256, (256, 256), (256,), 64, "relu"))
OFFSETS = (0, 2 ** 32 + 5)  # draws the generator has handed out before the call
SEED = 11
SENTINEL = 0x7FC12345  # a NaN no arithmetic produces: what the outputs hold before a call
SENTINEL64 = 0x7FC123457FC12345
OUTPUTS = ("actions", "log_probs", "values", "final_values", "logits")
T, ROLLOUTS, STACK = rollout_cases.T, rollout_cases.ROLLOUTS, rollout_cases.STACK
GAMMA, GAE_LAMBDA = rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA
E2E_SIZES = (1, 65)
E2E_KINDS = {"view": dict(view=True, records=True, pi=(64, 64), vf=(64, 64), activation="tanh"),
             "plain": dict(view=False, records=False, pi=(256, 256), vf=(256, 256), activation="relu")}


def bits(a):
    a = np.asarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def spec_of(network):
    from reinfocus_amd.environments import policy

    width, pi, vf, actions, activation = network
    return policy.MlpPolicySpec(width, actions, pi=pi, vf=vf, activation=activation)


def state_dict(spec, seed, hostile=False):
    """A state_dict in stable-baselines3's names and shapes: normal weights of scale 1 / sqrt(fan_in), biases of scale
    0.1.  hostile: actions 0 and 1 share their row and bias (their logits tie exactly in every row), and the last of
    three or more actions lies 200 below (its e_i is 0)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, _, shape, is_weight in spec.entries:
        if is_weight:
            out[name] = (rng.standard_normal(shape[::-1]) / np.sqrt(shape[0])).astype(np.float32)
        else:
            out[name] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
    if hostile:
        out["action_net.weight"][1] = out["action_net.weight"][0]
        out["action_net.bias"][1] = out["action_net.bias"][0]
        if spec.n_actions > 2:
            out["action_net.bias"][-1] -= np.float32(200.0)
    return out


def hostile_rows(width, n, seed, nan_rows):
    """float32 [n, width]: normal rows with +-0, subnormals and large values strewn in; every fifth row from row 3 holds
    an infinity, row 2 (if there) a NaN in its last column.  nan_rows: every third row from row 1 is NaN throughout, as
    the records leave final_observation where no episode ended, and row 0 -- if n > 3 -- has a NaN in column 0 only."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, width)).astype(np.float32)
    specials = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3.0e3, -2.5e-3], dtype=np.float32)
    where = rng.random((n, width)) < 0.2
    rows[where] = rng.choice(specials, int(where.sum()))
    for e in range(3, n, 5):
        rows[e, rng.integers(width)] = np.float32(np.inf if e % 2 else -np.inf)
    if n > 2:
        rows[2, -1] = np.nan
    if nan_rows:
        rows[1::3] = np.nan
        if n > 3:
            rows[0, 0] = np.nan
    return rows


def generator_at(offset, seed=SEED):
    """(bit generator advanced by offset, numpy Generator over it)."""
    bit_generator = np.random.PCG64DXSM(seed)
    bit_generator.advance(offset)
    return bit_generator, np.random.Generator(bit_generator)


MODES = (("sampled", OFFSETS[0]), ("sampled", OFFSETS[1]), ("deterministic", 0))


def forward_inputs(index, n):
    network = NETWORKS[index]
    spec = spec_of(network)
    params = spec.pack(state_dict(spec, 100 + index, hostile=True))
    return spec, params, hostile_rows(network[0], n, 1000 * index + n, False), hostile_rows(network[0], n, 7 + n, True)


def wanted_forward(spec, params, obs, final_obs, mode, offset):
    from reinfocus_amd.environments import policy

    u = generator_at(offset)[1].random(obs.shape[0]) if mode == "sampled" else None
    return policy.policy_numpy(spec, params, obs, final_obs, u, deterministic=mode == "deterministic")


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
def make_env(kind, n, device_form):
    from reinfocus_amd.environments import harness

    what = E2E_KINDS[kind]
    extra = dict(episode_records=what["records"],
                 learner_view=harness.LearnerView(frame_stack=STACK) if what["view"] else None)
    if device_form:
        return harness.DeviceVectorDiscreteSteps(num_envs=n, device_initializer=True, **rollout_cases.ENV_KW, **extra)
    return harness.VectorDiscreteSteps(num_envs=n, **rollout_cases.ENV_KW, **extra)


def e2e_spec(kind):
    from reinfocus_amd.environments import policy

    what = E2E_KINDS[kind]
    return policy.MlpPolicySpec(4 * (STACK if what["view"] else 1), 13, pi=what["pi"], vf=what["vf"],
                                activation=what["activation"])


def slabs_of(rollout, unwrap):
    slabs = {name: unwrap(getattr(rollout, name)) for name in
             ("observations", "actions", "rewards", "truncated", "values", "log_probs", "final_values", "advantages",
              "returns")}
    slabs.update({"flat/" + key: unwrap(value) for key, value in rollout.flat().items()})
    return slabs


def collect_runs(rollout, policy, reset, unwrap, rollouts=ROLLOUTS, between=None):
    """`rollouts` consecutive rollouts by collect(); between(r) runs before rollout r >= 1."""
    obs = reset()
    seen = []
    for r in range(rollouts):
        if r and between is not None:
            between(r)
        rollout.start(obs if r == 0 else None)
        rollout.collect(policy)
        seen.append(slabs_of(rollout, unwrap))
    return seen


def explicit_runs(rollout, policy, reset, unwrap, records, rollouts=ROLLOUTS):
    """The same by the explicit loop of start / act / step / bootstrap / finish."""
    obs = reset()
    seen = []
    for r in range(rollouts):
        rollout.start(obs if r == 0 else None)
        obs = rollout.observations[0]
        final_obs = None
        for _ in range(T):
            actions, values, log_probs, final_values = policy.act(obs, final_obs)
            if final_obs is not None:
                rollout.bootstrap(final_values)
            obs, _, _, _, info = rollout.step(actions, values, log_probs)
            final_obs = info["final_observation"] if records else None
        if records:
            last_values, final_values = policy.values(obs, final_obs)
            rollout.bootstrap(final_values)
        else:
            last_values = policy.values(obs)
        rollout.finish(last_values)
        seen.append(slabs_of(rollout, unwrap))
    return seen


def twin_runs(kind, n, rollouts=ROLLOUTS, explicit=False, second_state=None):
    """The numpy twins' rollouts; second_state: the state_dict seed loaded before rollout 1."""
    from reinfocus_amd.environments import harness

    env = make_env(kind, n, False)
    try:
        spec = e2e_spec(kind)
        policy = harness.Policy(spec, SEED)
        policy.load_state_dict(state_dict(spec, 3))
        rollout = harness.Rollout(env, T, GAMMA, GAE_LAMBDA)
        if explicit:
            return explicit_runs(rollout, policy, lambda: env.reset()[0], np.array, E2E_KINDS[kind]["records"], rollouts)
        between = None if second_state is None else lambda r: policy.load_state_dict(state_dict(spec, second_state))
        return collect_runs(rollout, policy, lambda: env.reset()[0], np.array, rollouts, between)
    finally:
        env.close()


same_runs = rollout_cases.same_runs


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
def _guarded(torch, n, count):
    """The five outputs, each with a guard row on either side, all sentinel: ({name: whole}, {name: view of n rows})."""
    whole = {name: torch.full((n + 2,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
             for name in ("log_probs", "values", "final_values")}
    whole["actions"] = torch.full((n + 2,), SENTINEL64, dtype=torch.int64, device="cuda")
    whole["logits"] = torch.full((n + 2, count), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    return whole, {name: tensor[1:n + 1] for name, tensor in whole.items()}


def _untouched(tensor):
    raw = tensor.contiguous().cpu().numpy()
    if raw.dtype == np.int64:
        return bool((raw == SENTINEL64).all())
    return bool((raw.view(np.uint32) == SENTINEL).all())


def _call(torch, ctx, spec, params, n, obs, final_obs, gen, flags, out, changed=()):
    a = dict(desc=spec.desc(), params=params.data_ptr(), n=n, obs=obs.data_ptr(),
             final_obs=None if final_obs is None else final_obs.data_ptr(), gen=gen, flags=flags)
    a.update({name: tensor.data_ptr() for name, tensor in out.items()})
    a.update(changed)  # (arguments given by their names above, in place of the tensors')
    ctx.policy_forward(a["desc"], a["params"], a["n"], a["obs"], a["final_obs"], a["gen"], a["flags"], a["actions"],
                       a["log_probs"], a["values"], a["final_values"], a["logits"], torch.cuda.current_stream().cuda_stream)


def kernel_case(torch, ctx, index, n):
    """rf_policy_forward against policy_numpy as bytes: sampled at both draw offsets, and deterministic."""
    from reinfocus_amd.environments import policy

    spec, params_h, obs_h, final_h = forward_inputs(index, n)
    assert ctx.policy_params_size(spec.desc()) == spec.size
    params, obs, final_obs = (torch.from_numpy(a).cuda() for a in (params_h, obs_h, final_h))
    for mode, offset in MODES:
        want = wanted_forward(spec, params_h, obs_h, final_h, mode, offset)
        whole, out = _guarded(torch, n, spec.n_actions)
        gen = policy.generator_words(generator_at(offset)[0]) if mode == "sampled" else None
        _call(torch, ctx, spec, params, n, obs, final_obs, gen, 0 if mode == "sampled" else policy.DETERMINISTIC, out)
        torch.cuda.synchronize()
        for name in OUTPUTS:
            assert bits(out[name].cpu().numpy()) == bits(want[name]), f"{mode} at {offset}: {name} differ"
            assert _untouched(whole[name][0]) and _untouched(whole[name][n + 1]), f"{mode}: a guard row of {name} was written"
    # values only: no pi block runs, no draw is needed
    whole, out = _guarded(torch, n, spec.n_actions)
    _call(torch, ctx, spec, params, n, obs, final_obs, None, 0, out, dict(actions=None, log_probs=None, logits=None))
    torch.cuda.synchronize()
    assert bits(out["values"].cpu().numpy()) == bits(want["values"])
    assert bits(out["final_values"].cpu().numpy()) == bits(want["final_values"])
    assert all(_untouched(whole[name]) for name in ("actions", "log_probs", "logits"))


def refusal_case(torch, ctx):
    """Each refusal leaves the outputs as they were: nothing was enqueued."""
    from reinfocus_amd.environments import policy

    index, n = 1, TILE + 1
    spec, params_h, obs_h, final_h = forward_inputs(index, n)
    params, obs, final_obs = (torch.from_numpy(a).cuda() for a in (params_h, obs_h, final_h))
    whole, out = _guarded(torch, n, spec.n_actions)
    gen = policy.generator_words(generator_at(0)[0])

    def refused(match, **changed):
        try:
            _call(torch, ctx, spec, params, n, obs, final_obs, gen, 0, out, changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        torch.cuda.synchronize()
        assert all(_untouched(w) for w in whole.values()), f"an output was written ({match})"

    host = np.zeros((n + 2, spec.obs_width), dtype=np.float32)
    refused("d_obs is not device memory", obs=host.ctypes.data)
    refused("d_values is not device memory", values=host.ctypes.data)
    refused("d_params is not device memory", params=params_h.ctypes.data)
    refused("at least 1", n=0)
    refused("not aligned", obs=obs.data_ptr() + 2)
    refused("not aligned", actions=out["actions"].data_ptr() + 4)
    refused("d_values overlaps d_obs", values=obs.data_ptr())
    refused("d_values overlaps d_log_probs", values=out["log_probs"].data_ptr())
    refused("d_logits overlaps d_params", logits=params.data_ptr())
    block = torch.zeros(32 * 1024 * 1024, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    # (were the length check to miss it, the aliased output of the same call is refused next: nothing can run past the end)
    alias = out["log_probs"].data_ptr()
    refused("fewer than", obs=block.data_ptr() + block.numel() - 4 * (n * spec.obs_width - 1), values=alias)
    refused("fewer than", params=block.data_ptr() + block.numel() - 4 * (spec.size - 1), values=alias)
    desc = list(spec.desc())
    for field, value in ((0, 0), (0, 257), (1, 1), (1, 65), (2, 2), (3, 0), (3, 3), (4, 257), (5, 0), (6, 3), (7, 0)):
        refused("outside the limits", desc=tuple(desc[:field] + [value] + desc[field + 1:]))
    refused("unknown flags", flags=2)
    refused("needs gen", gen=None)
    refused("needs d_final_obs", final_obs=None)
    refused("d_log_probs are those of d_actions", actions=None)
    _call(torch, ctx, spec, params, n, obs, final_obs, gen, 0, out)  # ... and the same arguments unchanged are taken
    torch.cuda.synchronize()
    want = wanted_forward(spec, params_h, obs_h, final_h, "sampled", 0)
    for name in OUTPUTS:
        assert bits(out[name].cpu().numpy()) == bits(want[name]), name


def _device_policy(torch, harness, env, kind, state_seed=3):
    spec = e2e_spec(kind)
    policy = harness.DevicePolicy(env, spec, SEED)
    policy.load_state_dict({k: torch.from_numpy(v).cuda() for k, v in state_dict(spec, state_seed).items()})
    return spec, policy


def end_to_end_case(torch, kind, n):
    from reinfocus_amd.environments import harness

    want = twin_runs(kind, n)
    env = make_env(kind, n, True)
    try:
        spec, policy = _device_policy(torch, harness, env, kind)
        assert bits(policy.params.cpu().numpy()) == bits(spec.pack(state_dict(spec, 3)))
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        got = collect_runs(buffer, policy, lambda: env.reset_tensors()[0], lambda a: a.cpu().numpy())
        same_runs(got, want)
        assert env.device_fault() is None
        assert np.concatenate([run["truncated"] for run in want]).any(), "no environment ended"
        twin = harness.Policy(spec, SEED)
        twin._generator.random(ROLLOUTS * T * n)  # (what the twin policy has drawn by now)
        assert policy.rng_state() == twin.rng_state()
    finally:
        env.close()


def explicit_case(torch):
    """collect() next to the explicit loop on the device: as bytes."""
    from reinfocus_amd.environments import harness

    kind, n = "view", 9
    runs = []
    for explicit in (False, True):
        env = make_env(kind, n, True)
        try:
            _, policy = _device_policy(torch, harness, env, kind)
            buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
            reset, unwrap = (lambda: env.reset_tensors()[0]), (lambda a: a.cpu().numpy())
            runs.append(explicit_runs(buffer, policy, reset, unwrap, True) if explicit
                        else collect_runs(buffer, policy, reset, unwrap))
            assert env.device_fault() is None
        finally:
            env.close()
    same_runs(runs[0], runs[1])
    same_runs(runs[0], twin_runs(kind, n))


def no_sync_case(torch):
    """Two collects enqueued back to back, nothing read in between; one synchronisation at the end."""
    from reinfocus_amd.environments import harness

    kind, n = "view", 65
    want = twin_runs(kind, n)
    env = make_env(kind, n, True)
    try:
        _, policy = _device_policy(torch, harness, env, kind)
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        obs = env.reset_tensors()[0]
        torch.cuda.synchronize()
        buffer.start(obs)
        advantages, returns = buffer.collect(policy)
        kept = {name: getattr(buffer, name).clone() for name in ("observations", "actions", "log_probs", "final_values")}
        kept.update(advantages=advantages.clone(), returns=returns.clone())
        buffer.start()
        buffer.collect(policy)
        torch.cuda.synchronize()  # the only one
        for name, tensor in kept.items():
            assert bits(tensor.cpu().numpy()) == bits(want[0][name]), name
        for name in ("observations", "actions", "values", "log_probs", "final_values", "advantages", "returns"):
            assert bits(getattr(buffer, name).cpu().numpy()) == bits(want[1][name]), name
        assert env.device_fault() is None
    finally:
        env.close()


def reload_case(torch):
    """load_state_dict between two collects changes the second one exactly as the twin's does."""
    from reinfocus_amd.environments import harness

    kind, n = "plain", 9
    want = twin_runs(kind, n, second_state=4)
    unchanged = twin_runs(kind, n)
    assert bits(want[0]["actions"]) == bits(unchanged[0]["actions"])
    assert bits(want[1]["log_probs"]) != bits(unchanged[1]["log_probs"])  # (the new parameters matter)
    env = make_env(kind, n, True)
    try:
        spec, policy = _device_policy(torch, harness, env, kind)
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        second = {k: torch.from_numpy(v).cuda() for k, v in state_dict(spec, 4).items()}
        got = collect_runs(buffer, policy, lambda: env.reset_tensors()[0], lambda a: a.cpu().numpy(),
                           between=lambda r: policy.load_state_dict(second))
        same_runs(got, want)
        back = policy.state_dict()
        for name, value in state_dict(spec, 4).items():
            assert bits(back[name].cpu().numpy()) == bits(value), name
    finally:
        env.close()


def surface_case(torch):
    """A Box action space is refused; act() without out=, deterministic and with rows of another shape."""
    from reinfocus_amd.environments import harness

    env = harness.DeviceVectorContinuousJumps(num_envs=2, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        try:
            harness.DevicePolicy(env, e2e_spec("plain"), 0)
        except ValueError as caught:
            assert "out of scope" in str(caught), str(caught)
        else:
            raise AssertionError("a Box action space was taken")
    finally:
        env.close()
    n = 5
    env = make_env("plain", n, True)
    try:
        spec, policy = _device_policy(torch, harness, env, "plain")
        twin = harness.Policy(spec, SEED)
        twin.load_state_dict(state_dict(spec, 3))
        obs_h = hostile_rows(4, n, 5, False)
        obs = torch.from_numpy(obs_h).cuda()
        before = policy.rng_state()
        for deterministic in (True, False):
            got = policy.act(obs, deterministic=deterministic)
            want = twin.act(obs_h, deterministic=deterministic)
            assert got[3] is None and want[3] is None
            for x, y in zip(got[:3], want[:3]):
                assert bits(x.cpu().numpy()) == bits(y)
            assert (policy.rng_state() == before) == deterministic
        assert bits(policy.values(obs).cpu().numpy()) == bits(twin.values(obs_h))
        assert policy.rng_state() == twin.rng_state()
        for bad, error in ((obs[:, :3], ValueError), (obs.double(), ValueError), (obs_h, TypeError), (obs.cpu(), ValueError)):
            try:
                policy.act(bad)
            except error:
                pass
            else:
                raise AssertionError("rows of another kind were taken")
        assert policy.rng_state() == twin.rng_state()  # (a refused call consumes nothing)
    finally:
        env.close()


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    ctx = _native.Context(0)
    for index in range(len(NETWORKS)):
        for n in SIZES:
            with record.case(f"kernel/{index}/{n}"):
                kernel_case(torch, ctx, index, n)
    with record.case("refusals"):
        refusal_case(torch, ctx)
    ctx.close()
    for kind in E2E_KINDS:
        for n in E2E_SIZES:
            with record.case(f"end-to-end/{kind}/{n}"):
                end_to_end_case(torch, kind, n)
    with record.case("explicit"):
        explicit_case(torch)
    with record.case("no-sync"):
        no_sync_case(torch)
    with record.case("reload"):
        reload_case(torch)
    with record.case("surface"):
        surface_case(torch)
    with record.case("finished"):
        pass


def torch_forward(path_in, path_out):
    """torch's CPU float32 forward of a state_dict (two nn.Sequential nets and the heads, log_softmax of the logits):
    what stable-baselines3 computes.  In a process of its own: torch brings a HIP runtime of its own."""
    import torch

    data = np.load(path_in)
    tensors = {k: torch.from_numpy(data[k]) for k in data.files if k not in ("obs", "activation")}
    act = torch.nn.Tanh if str(data["activation"]) == "tanh" else torch.nn.ReLU

    def net(extractor, head_name):
        layers = []
        for i in (0, 2):
            if f"mlp_extractor.{extractor}.{i}.weight" in tensors:
                weight = tensors[f"mlp_extractor.{extractor}.{i}.weight"]
                layers += [torch.nn.Linear(weight.shape[1], weight.shape[0]), act()]
        weight = tensors[head_name + ".weight"]
        model = torch.nn.Sequential(*layers, torch.nn.Linear(weight.shape[1], weight.shape[0]))
        keys = [f"mlp_extractor.{extractor}.{i}" for i in (0, 2)][:len(layers) // 2] + [head_name]
        model.load_state_dict({f"{2 * j}.{part}": tensors[f"{key}.{part}"] for j, key in enumerate(keys)
                               for part in ("weight", "bias")})
        return model

    with torch.no_grad():
        obs = torch.from_numpy(data["obs"])
        log_probs = torch.log_softmax(net("policy_net", "action_net")(obs), dim=1)
        values = net("value_net", "value_net")(obs)[:, 0]
    np.savez(path_out, log_probs=log_probs.numpy(), values=values.numpy())


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "--torch-forward":
        torch_forward(sys.argv[2], sys.argv[3])
    else:
        run_cases(sys.argv[1])
