"""TEST INFRASTRUCTURE: what tests/test_param_init_logic.py and tests/test_gpu_param_init.py share -- the networks, the
seeds, the numpy twin's results (computed once and shared, never changed) -- and the child process of the GPU file.

As tests/population_lstm_sde_io_cases.py: everything that needs torch and the library together runs in one fresh process
that imports torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.param_init_io_cases <results.jsonl>
"""

import functools
import os
import sys

import numpy as np

from tests import policy_io_cases as policy_cases
from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
bits = policy_cases.bits
SENTINEL = policy_cases.SENTINEL

HIGH_SEED = 2 ** 70 + 5
WIDE_SEED = 1
SEEDS = (3, HIGH_SEED, 11)  # (group 1's generator state has bits above 2^96 set: test_gpu_param_init checks that it does)
MASKS = (None, (1, 0, 1), (0, 0, 0))
LOG_STD = (-1.0, 0.5, 2.0)
SCHEMES = (False, True)  # ortho_init


def _mlp(width, actions, pi, vf):
    from reinfocus_amd.environments import harness

    return harness.MlpPolicySpec(width, actions, pi=pi, vf=vf)


def _sde(width, pi, vf, log_std_init=-2.0):
    from reinfocus_amd.environments import harness

    return harness.SdePolicySpec(width, pi=pi, vf=vf, log_std_init=log_std_init)


def _lstm(hidden, critic_lstm, sde, width=25):
    from reinfocus_amd.environments import harness

    if sde:
        return harness.LstmSdePolicySpec(width, lstm_hidden=hidden, pi=(6,), vf=(5, 7), log_std_init=-2.0,
                                         enable_critic_lstm=critic_lstm)
    return harness.LstmPolicySpec(width, 7, lstm_hidden=hidden, pi=(6,), vf=(5, 7), enable_critic_lstm=critic_lstm)


# the five heads (both critic kinds of the recurrent ones) at small networks: out > in, out < in, 1 x K and odd sizes
SMALL_SPECS = {
    "mlp": lambda: _mlp(5, 3, (7,), (3, 2)),
    "mlp-64": lambda: _mlp(25, 7, (64, 64), (64, 64)),
    "sde": lambda: _sde(5, (7,), (3, 2)),
    "lstm": lambda: _lstm(16, True, False),
    "lstm-linear": lambda: _lstm(16, False, False),
    "lstm-sde": lambda: _lstm(16, True, True),
    "lstm-sde-linear": lambda: _lstm(16, False, True),
}
# ... and at H = 256, the widest cell (the LSTM's run of arrays is cut into five segments)
WIDE_LSTM_SPECS = {
    "lstm-256": lambda: _lstm(256, True, False),
    "lstm-256-linear": lambda: _lstm(256, False, False),
    "lstm-sde-256": lambda: _lstm(256, True, True),
    "lstm-sde-256-linear": lambda: _lstm(256, False, True),
}


def wide_spec():
    """t = s = 256 (the full block of the orthogonal kernel) and an in = 1 head input."""
    return _mlp(256, 64, (256,), (256, 1))


def widest_lstm_spec():
    from reinfocus_amd.environments import harness

    return harness.LstmSdePolicySpec(256, lstm_hidden=256, pi=(256, 256), vf=(256, 256))


KERNEL_SPECS = dict(SMALL_SPECS, **WIDE_LSTM_SPECS)
KERNEL_SPECS["mlp-256"] = wide_spec


def populations():
    from reinfocus_amd.environments import harness

    return {"mlp": (SMALL_SPECS["mlp"], harness.Policy, harness.PopulationPolicy, False),
            "sde": (SMALL_SPECS["sde"], harness.SdePolicy, harness.SdePopulationPolicy, True),
            "lstm": (SMALL_SPECS["lstm-linear"], harness.LstmPolicy, harness.LstmPopulationPolicy, False),
            "lstm-sde": (SMALL_SPECS["lstm-sde"], harness.LstmSdePolicy, harness.LstmSdePopulationPolicy, True)}


POPULATION_KINDS = ("lstm", "lstm-sde", "mlp", "sde")  # (the keys of populations())


@functools.lru_cache(maxsize=None)
def twin(name, seed, ortho_init, log_std_init=None):
    """init_numpy of KERNEL_SPECS[name]: computed once per (network, seed, scheme), shared, read-only."""
    from reinfocus_amd.environments import param_init

    params = param_init.init_numpy(KERNEL_SPECS[name](), seed, ortho_init, log_std_init=log_std_init)
    params.setflags(write=False)
    return params


def wide_twin(ortho_init):
    return twin("mlp-256", WIDE_SEED, ortho_init)


# ---- the child process -----------------------------------------------------------------------------------------------------
def _guarded(torch, cells):
    """A float32 tensor of cells + 2 sentinel floats and its inside."""
    whole = torch.full((cells + 2,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    return whole, whole[1:cells + 1]


def _is_sentinel(array):
    return bool((np.ascontiguousarray(array).view(np.uint32) == SENTINEL).all())


def _device_inputs(torch, seeds, mask, constants):
    from reinfocus_amd.environments.policy import generator_words

    words = np.array([generator_words(np.random.PCG64DXSM(seed)) for seed in seeds], dtype=np.uint64)
    gens = torch.from_numpy(words.view(np.int64)).cuda()
    select = None if mask is None else torch.tensor(mask, dtype=torch.uint8, device="cuda")
    values = None if constants is None else torch.tensor(constants, dtype=torch.float32, device="cuda")
    return gens, select, values


def _pointer(tensor):
    return None if tensor is None else tensor.data_ptr()


def _run(torch, ctx, table, groups, stride, inside, gens, select, constants):
    from reinfocus_amd.environments import param_init

    array = param_init.segment_array(table)
    need = ctx.params_init_workspace_size(array, len(table), groups)
    assert need == 16 * groups * sum(out * in_ for _, out, in_, scheme, _ in table if scheme == param_init.ORTHOGONAL)
    workspace = torch.empty(max(need // 8, 1), dtype=torch.float64, device="cuda")
    ctx.params_init(array, len(table), groups, stride, inside.data_ptr(), gens.data_ptr(), _pointer(select),
                    _pointer(constants), workspace.data_ptr() if need else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def kernel_case(torch, ctx, name, ortho_init):
    """rf_params_init at G = 3 for the three masks: selected groups are the twin's bytes, unselected groups and the guard
    floats keep their sentinel bytes."""
    from reinfocus_amd.environments import param_init

    spec = KERNEL_SPECS[name]()
    table = param_init.segments(spec, ortho_init)
    has_log_std = hasattr(spec, "log_std_init")
    groups, stride = len(SEEDS), spec.size
    for mask in MASKS:
        whole, inside = _guarded(torch, groups * stride)
        gens, select, constants = _device_inputs(torch, SEEDS, mask, LOG_STD if has_log_std else None)
        _run(torch, ctx, table, groups, stride, inside, gens, select, constants)
        got = whole.cpu().numpy()
        assert _is_sentinel(got[:1]) and _is_sentinel(got[-1:]), f"mask {mask}: a guard float was written"
        rows = got[1:-1].reshape(groups, stride)
        for g, seed in enumerate(SEEDS):
            if mask is not None and not mask[g]:
                assert _is_sentinel(rows[g]), f"mask {mask}: unselected group {g} was written"
                continue
            want = twin(name, seed, ortho_init, LOG_STD[g] if has_log_std else None)
            if bits(rows[g]) != bits(want):
                wrong = np.flatnonzero(rows[g].view(np.uint32) != want.view(np.uint32))
                raise AssertionError(f"mask {mask}, group {g}: {wrong.size} of {stride} floats differ, first at {wrong[0]}: "
                                     f"{rows[g][wrong[0]]!r} for {want[wrong[0]]!r}")


def outside_case(torch, ctx):
    """Positions outside every segment keep their bytes: the table of the small MLP without its first weight and without
    an orthogonal segment in the middle; G = 1."""
    from reinfocus_amd.environments import param_init

    spec = KERNEL_SPECS["mlp"]()
    for ortho_init in SCHEMES:
        table = param_init.segments(spec, ortho_init)
        dropped = (table[0], table[4])
        kept = [row for row in table if row not in dropped]
        whole, inside = _guarded(torch, spec.size)
        gens, _, _ = _device_inputs(torch, [HIGH_SEED], None, None)
        _run(torch, ctx, kept, 1, spec.size, inside, gens, None, None)
        got = whole.cpu().numpy()
        want = twin("mlp", HIGH_SEED, ortho_init)
        assert _is_sentinel(got[:1]) and _is_sentinel(got[-1:])
        covered = np.ones(spec.size, dtype=bool)
        for at, out, in_, _, _ in dropped:
            covered[at:at + out * in_] = False
            assert _is_sentinel(got[1:-1][at:at + out * in_])
        assert bits(got[1:-1][covered]) == bits(want[covered])


def kernel_refusal_case(torch, ctx):
    """What rf_params_init refuses, each with a message and nothing written."""
    from reinfocus_amd.environments import param_init

    U, O, C, Z = param_init.UNIFORM, param_init.ORTHOGONAL, param_init.CONSTANT, param_init.ZERO
    whole, inside = _guarded(torch, 64)
    gens, select, constants = _device_inputs(torch, [1], (1,), (0.5,))
    workspace = torch.empty(64, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def refused(table, words, stride=24, groups=1, params=inside, gen=gens, consts=constants, work=workspace):
        array = param_init.segment_array(table)
        try:
            ctx.params_init(array, len(table), groups, stride, _pointer(params), _pointer(gen), _pointer(select),
                            _pointer(consts), _pointer(work), stream)
        except AssertionError as error:
            assert words in str(error), (words, str(error))
            return
        raise AssertionError(f"not refused: {words}")

    refused([(i, 1, 1, Z, 0.0) for i in range(33)], "RF_PARAM_MAX_SEGMENTS", stride=64)
    refused([(0, 4, 3, U, 0.5), (11, 4, 1, Z, 0.0)], "overlap")
    refused([(0, 4, 3, U, 0.5), (21, 4, 1, Z, 0.0)], "out of range")
    refused([(0, 4, 3, 7, 0.5)], "unknown")
    for scheme in (U, O):
        for scale in (0.0, -1.0, float("inf"), float("nan")):
            refused([(0, 4, 3, scheme, scale)], "scale")
    refused([(0, 4, 1, C, 0.0)], "d_constants", consts=None)
    refused([(0, 4, 3, O, 1.0)], "d_workspace", work=None)
    refused([(0, 257, 1, Z, 0.0)], "RF_POLICY_MAX_WIDTH", stride=64)
    refused([(0, 4, 3, U, 0.5)], "G = 0", groups=0)
    refused([(0, 4, 3, U, 0.5)], "stride", stride=0)
    refused([(0, 4, 3, U, 0.5)], "NULL", gen=None)
    refused([(0, 4, 3, O, 1.0)], "overlaps", work=whole)
    assert ctx.params_init_workspace_size(param_init.segment_array([(0, 4, 3, 7, 0.5)]), 1, 1) == 0
    torch.cuda.synchronize()
    assert _is_sentinel(whole.cpu().numpy())


def _env(kind, n):
    from reinfocus_amd.environments import harness

    cls = harness.DeviceVectorContinuousJumps if kind in ("sde", "lstm-sde") else harness.DeviceVectorDiscreteSteps
    return cls(num_envs=n, device_initializer=True, **rollout_cases.ENV_KW)


def _class_spec(kind, env, critic_lstm=True):
    from reinfocus_amd.environments import harness

    width = int(env.single_observation_space.shape[0])
    if kind == "mlp":
        return harness.MlpPolicySpec(width, int(env.single_action_space.n), pi=(7,), vf=(3, 2))
    if kind == "sde":
        return harness.SdePolicySpec(width, pi=(7,), vf=(3, 2), log_std_init=-2.0)
    if kind == "lstm":
        return harness.LstmPolicySpec(width, int(env.single_action_space.n), lstm_hidden=9, pi=(6,), vf=(5, 7),
                                      enable_critic_lstm=critic_lstm)
    return harness.LstmSdePolicySpec(width, lstm_hidden=9, pi=(6,), vf=(5, 7), log_std_init=-2.0,
                                     enable_critic_lstm=critic_lstm)


def _classes(kind):
    from reinfocus_amd.environments import harness

    return {"mlp": (harness.Policy, harness.DevicePolicy, harness.PopulationPolicy, harness.DevicePopulationPolicy),
            "sde": (harness.SdePolicy, harness.DeviceSdePolicy, harness.SdePopulationPolicy,
                    harness.DeviceSdePopulationPolicy),
            "lstm": (harness.LstmPolicy, harness.DeviceLstmPolicy, harness.LstmPopulationPolicy,
                     harness.DevicePopulationLstmPolicy),
            "lstm-sde": (harness.LstmSdePolicy, harness.DeviceLstmSdePolicy, harness.LstmSdePopulationPolicy,
                         harness.DevicePopulationLstmSdePolicy)}[kind]


def class_case(torch, kind):
    """Device*Policy.init_parameters equals its twin, both schemes; the population equals G stand-alone device objects and
    the twin population for the three masks, and at G = 1 the ungrouped class; the action generators are untouched."""
    twin_class, device_class, twin_population, device_population = _classes(kind)
    with_inits = kind in ("sde", "lstm-sde")
    groups = len(SEEDS)
    env, env1 = _env(kind, groups * 2), _env(kind, 2)
    try:
        spec = _class_spec(kind, env, critic_lstm=False)
        kw = dict(log_std_init=list(LOG_STD)) if with_inits else {}
        for ortho_init in SCHEMES:
            single, single_twin = device_class(env1, spec, 5), twin_class(spec, 5)
            state = single.rng_state()
            single.init_parameters(HIGH_SEED, ortho_init)
            single_twin.init_parameters(HIGH_SEED, ortho_init)
            assert bits(single.params.cpu().numpy()) == bits(single_twin.params)
            assert single.rng_state() == state == single_twin.rng_state()
            one = device_population(env1, spec, 1, [5])
            one.init_parameters([HIGH_SEED], ortho_init)
            assert bits(one.params[0].cpu().numpy()) == bits(single.params.cpu().numpy())
            population, population_twin = device_population(env, spec, groups, [1, 2, 3], **kw), \
                twin_population(spec, groups, [1, 2, 3], **kw)
            state = population.rng_state()
            for mask, seeds in zip(MASKS, (SEEDS, (21, 22, 23), (31, 32, 33))):
                selected = None if mask is None else [bool(x) for x in mask]
                population.init_parameters(list(seeds), ortho_init, groups=selected)
                population_twin.init_parameters(list(seeds), ortho_init, groups=selected)
                got = population.params.cpu().numpy()
                assert bits(got) == bits(population_twin.params), f"mask {mask}"
                if mask is None:  # (G stand-alone device objects, each with the group's own log_std_init)
                    for g, seed in enumerate(seeds):
                        alone_spec = spec
                        if with_inits:
                            alone_spec = _class_spec(kind, env, critic_lstm=False)
                            alone_spec.log_std_init = LOG_STD[g]
                        alone = device_class(env1, alone_spec, 5)
                        alone.init_parameters(seed, ortho_init)
                        assert bits(alone.params.cpu().numpy()) == bits(got[g]), f"group {g}"
            assert population.rng_state() == state
    finally:
        env.close()
        env1.close()


def surface_case(torch):
    """What the device classes refuse, before anything is enqueued: the parameters keep their bytes."""
    from reinfocus_amd.environments import harness

    env = _env("mlp", 6)
    try:
        spec = _class_spec("mlp", env)
        population = harness.DevicePopulationPolicy(env, spec, 3, [1, 2, 3])
        population.init_parameters([4, 5, 6], False)
        kept = population.params.clone()
        for call, error in ((lambda: population.init_parameters([1, 2], False), ValueError),
                            (lambda: population.init_parameters(7, False), ValueError),
                            (lambda: population.init_parameters([1, 2, 3], False, groups=[True, False]), ValueError),
                            (lambda: population.init_parameters([1, 2, 3], 1), TypeError),
                            (lambda: harness.DevicePolicy(env, spec, 1).init_parameters(1, None), TypeError)):
            try:
                call()
            except error as refusal:
                assert str(refusal)
            else:
                raise AssertionError("not refused")
        assert torch.equal(population.params.view(torch.int32), kept.view(torch.int32))
    finally:
        env.close()


def train_mlp_case(torch):
    """DevicePolicy: after init_parameters, one act() and one update() on the device equal the twin started from the same
    init; the first hidden layers have moved."""
    from reinfocus_amd.environments import harness

    n, total = 4, 32
    env = _env("mlp", n)
    try:
        spec = harness.MlpPolicySpec(int(env.single_observation_space.shape[0]), int(env.single_action_space.n), pi=(6,),
                                     vf=(5,))
        device, twin_policy = harness.DevicePolicy(env, spec, 9), harness.Policy(spec, 9)
        device.init_parameters(21, ortho_init=False)
        twin_policy.init_parameters(21, ortho_init=False)
        first = twin_policy.params.copy()
        rng = np.random.default_rng(6)
        obs = rng.standard_normal((n, spec.obs_width)).astype(F32)
        got = device.act(torch.from_numpy(obs).cuda())
        want = twin_policy.act(obs)
        for x, y in zip(got[:3], want[:3]):
            assert bits(x.cpu().numpy()) == bits(y)
        flat = {"observations": rng.standard_normal((total, spec.obs_width)).astype(F32),
                "actions": rng.integers(0, spec.n_actions, total).astype(np.int64),
                "log_probs": (-1.1 + 0.1 * rng.standard_normal(total)).astype(F32),
                "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32)}
        index = np.arange(16, dtype=np.int64)
        kw = dict(learning_rate=1e-2)
        stats = harness.DeviceLearner(device, **kw).update({k: torch.from_numpy(v).cuda() for k, v in flat.items()},
                                                           torch.from_numpy(index).cuda())
        want_stats = harness.Learner(twin_policy, **kw).update(flat, index)
        assert bits(stats.cpu().numpy()) == bits(want_stats)
        assert bits(device.params.cpu().numpy()) == bits(twin_policy.params)
        moved = spec.unpack(twin_policy.params)["mlp_extractor.policy_net.0.weight"] != \
            spec.unpack(first)["mlp_extractor.policy_net.0.weight"]
        assert moved.any()
    finally:
        env.close()


def train_population_case(torch):
    """DevicePopulationLstmPolicy at G = 2, m = 2: after init_parameters, one act() and one update() of the population
    equal the twin population started from the same init."""
    from reinfocus_amd.environments import harness

    groups, per_group, steps = 2, 2, 4
    n = groups * per_group
    env = _env("lstm", n)
    try:
        spec = harness.LstmPolicySpec(int(env.single_observation_space.shape[0]), int(env.single_action_space.n),
                                      lstm_hidden=4, pi=(5,), vf=(5,))
        device = harness.DevicePopulationLstmPolicy(env, spec, groups, [1, 2])
        twin_population = harness.LstmPopulationPolicy(spec, groups, [1, 2], num_envs=n)
        device.init_parameters([21, HIGH_SEED], ortho_init=True)
        twin_population.init_parameters([21, HIGH_SEED], ortho_init=True)
        first = twin_population.params.copy()
        rng = np.random.default_rng(7)
        obs = rng.standard_normal((n, spec.obs_width)).astype(F32)
        starts = np.ones(n, dtype=np.uint8)
        got = device.act(torch.from_numpy(obs).cuda(), torch.from_numpy(starts).cuda())
        want = twin_population.act(obs, starts)
        for x, y in zip(got[:3], want[:3]):
            assert bits(x.cpu().numpy()) == bits(y)
        assert bits(device.lstm_state().cpu().numpy()) == bits(twin_population.lstm_state())
        total = n * steps
        episode_starts = np.zeros((steps + 1, n), dtype=np.uint8)
        episode_starts[0] = 1
        episode_starts[2, 1] = 1
        parts = {"observations": rng.standard_normal((total, spec.obs_width)).astype(F32),
                 "actions": rng.integers(0, spec.n_actions, total).astype(np.int64),
                 "log_probs": (-0.7 + 0.1 * rng.standard_normal(total)).astype(F32),
                 "advantages": rng.standard_normal(total).astype(F32), "returns": rng.standard_normal(total).astype(F32),
                 "episode_starts": episode_starts,
                 "lstm_states": (0.5 * rng.standard_normal((steps + 1,) + spec.state_shape(n))).astype(F32)}
        on_device = {key: torch.from_numpy(value).cuda() for key, value in parts.items()}
        parts.update(n_steps=steps, num_envs=n)
        on_device.update(n_steps=steps, num_envs=n)
        kw = dict(learning_rate=1e-2)
        stats = harness.DevicePopulationLearner(device, **kw).update(on_device, [0, 3], 5)
        want_stats = harness.PopulationLearner(twin_population, **kw).update(parts, [0, 3], 5)
        assert bits(stats.cpu().numpy()) == bits(want_stats)
        assert bits(device.params.cpu().numpy()) == bits(twin_population.params)
        assert (twin_population.params != first).any(axis=1).all()
    finally:
        env.close()


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    ctx = _native.Context(0)
    for name in sorted(KERNEL_SPECS):
        for ortho_init in SCHEMES:
            with record.case(f"kernel/{name}/{int(ortho_init)}"):
                kernel_case(torch, ctx, name, ortho_init)
    with record.case("outside"):
        outside_case(torch, ctx)
    with record.case("kernel-refusals"):
        kernel_refusal_case(torch, ctx)
    ctx.close()
    for kind in POPULATION_KINDS:
        with record.case(f"classes/{kind}"):
            class_case(torch, kind)
    with record.case("surface"):
        surface_case(torch)
    with record.case("train/mlp"):
        train_mlp_case(torch)
    with record.case("train/population"):
        train_population_case(torch)
    with record.case("finished"):
        pass


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    run_cases(sys.argv[1])
