"""TEST INFRASTRUCTURE: what tests/test_rollout_logic.py and tests/test_gpu_rollout.py share -- shapes, seeds, the action
schedules and the "policy" of the end-to-end runs, the synthetic inputs of the kernel -- and the child process of the GPU
file.

As tests/device_io_cases.py: everything that needs torch and the library together runs in one fresh process that imports
torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.rollout_io_cases <results.jsonl>
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, STACK = 7, 5  # steps of a rollout of the end-to-end runs; the learner view's frame_stack
ROLLOUTS = 2
# 16 x 16 pixels, 1 sample; a limit of 5 steps, because the tasks' DivergingEnder needs 3: environments end at
# different steps (tests/test_rollout_logic.py checks: some inside each rollout, one on the last step of a rollout)
ENV_KW = dict(max_episode_steps=5, seed=1, frame_height=16, samples_per_pixel=1, device=0)
E2E_SIZES = (1, 3, 65)
E2E_KINDS = {"steps": dict(jumps=False, view=True, records=True), "jumps": dict(jumps=True, view=False, records=True),
             "no-records": dict(jumps=False, view=True, records=False)}
CHUNK = 32  # rf::kRolloutChunk (tests/test_rollout_logic.py reads csrc/rf_rollout.h and compares)
KERNEL_SHAPES = ((1, 1), (2, 3), (5, 64), (33, 65), (128, 8), (CHUNK + 1, 1100))
TRUNCATIONS = ("none", "all", "random")
GAMMA, GAE_LAMBDA = 0.99, 0.92  # float32(0.99 * 0.92) != float32(0.99) * float32(0.92): a wrong gl shows
SENTINEL = 0x7FC12345  # a NaN no arithmetic produces: what the output slabs hold before a call


def index_schedule(t, n):
    """The index actions of global step t: fixed, no generator."""
    return ((11 * t + 4 * np.arange(n) + 2) % 13).astype(np.int64)


def jump_schedule(t, n):
    """The float32 jump actions of global step t: multiples of 1/8 in [-1, 1], exact in float32."""
    return (((5 * t + 3 * np.arange(n)) % 17 - 8) / 8.0).astype(np.float32)


def schedule(kind, t, n):
    return jump_schedule(t, n) if E2E_KINDS[kind]["jumps"] else index_schedule(t, n)


def make_env(kind, n, device_form):
    """The twin (device_form False) or the device environment of an end-to-end kind."""
    from reinfocus_amd.environments import harness

    what = E2E_KINDS[kind]
    extra = dict(episode_records=what["records"],
                 learner_view=harness.LearnerView(frame_stack=STACK) if what["view"] else None)
    if device_form:
        cls = harness.DeviceVectorContinuousJumps if what["jumps"] else harness.DeviceVectorDiscreteSteps
        return cls(num_envs=n, device_initializer=True, **ENV_KW, **extra)
    cls = harness.VectorContinuousJumps if what["jumps"] else harness.VectorDiscreteSteps
    return cls(num_envs=n, **ENV_KW, **extra)


def policy(obs):
    """values and log_probs of an observation batch: exact in float32, no reduction -- numpy and torch agree bit for
    bit.  (A float32 array / tensor times the Python scalar 0.5 stays float32 in both.)"""
    values = obs[:, 0] * 0.5
    return values, -values


def synthetic(steps, n, truncation, seed):
    """Hostile inputs of the kernel: (rewards f64, values f32, truncated u8, final_values f32, last_values f32)."""
    rng = np.random.default_rng(seed)
    cells = steps * n
    values = (rng.standard_normal(cells) * 10.0 ** rng.uniform(-3, 3, cells)).astype(np.float32)
    rewards = rng.standard_normal(cells) * 10.0 ** rng.uniform(-3, 3, cells)  # (float64: not representable in float32)
    rewards[rng.random(cells) < 0.05] = 1.0 + 2.0 ** -30
    rewards[rng.random(cells) < 0.02] = 1e-42  # a float32 subnormal after the cast
    rewards[rng.random(cells) < 0.02] = 1e300  # +inf after the cast
    rewards[rng.random(cells) < 0.02] = -0.0
    specials = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 1.4e-45, 3.0e38], dtype=np.float32)
    where = rng.random(cells) < 0.15
    values[where] = rng.choice(specials, int(where.sum()))
    if cells >= len(specials):  # every special at least once, whatever the draw
        values[rng.permutation(cells)[:len(specials)]] = specials
    truncated = {"none": np.zeros(cells, dtype=np.uint8), "all": np.ones(cells, dtype=np.uint8),
                 "random": (rng.random(cells) < 0.3).astype(np.uint8)}[truncation]
    final_values = (rng.standard_normal(cells) * 10.0 ** rng.uniform(-2, 2, cells)).astype(np.float32)
    final_values[truncated == 0] = np.nan  # as the records leave them
    last_values = (rng.standard_normal(n) * 3.0).astype(np.float32)
    if n >= 4:
        last_values[:4] = [np.inf, -0.0, 1e-40, -np.inf]
    shape = (steps, n)
    return (rewards.reshape(shape), values.reshape(shape), truncated.reshape(shape), final_values.reshape(shape),
            last_values)


def drive(rollout, reset, wrap, unwrap, kind, n, rollouts=ROLLOUTS):
    """`rollouts` consecutive rollouts of T steps by the schedule and the policy; reset() gives the first observation,
    wrap makes an action array what the environment takes, unwrap makes a result a numpy array.  Returns one dict of
    numpy arrays per rollout: every slab, advantages, returns and flat()."""
    records = E2E_KINDS[kind]["records"]
    obs = reset()
    seen = []
    for r in range(rollouts):
        rollout.start(obs if r == 0 else None)
        for t in range(T):
            values, log_probs = policy(obs)
            obs, _, _, _, info = rollout.step(wrap(schedule(kind, r * T + t, n)), values, log_probs)
            if records:
                rollout.bootstrap(info["final_observation"][:, 0] * 0.5)
        rollout.finish(policy(obs)[0])
        slabs = {name: unwrap(getattr(rollout, name)) for name in
                 ("observations", "actions", "rewards", "truncated", "values", "log_probs", "final_values", "advantages",
                  "returns")}
        slabs.update({"flat/" + key: unwrap(value) for key, value in rollout.flat().items()})
        seen.append(slabs)
    return seen


def twin_run(kind, n, rollouts=ROLLOUTS):
    from reinfocus_amd.environments import harness

    env = make_env(kind, n, False)
    try:
        return drive(harness.Rollout(env, T, GAMMA, GAE_LAMBDA), lambda: env.reset()[0], lambda a: a,
                     lambda a: np.array(a), kind, n, rollouts)
    finally:
        env.close()


def _bits(a):
    a = np.asarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def same_runs(got, want):
    assert len(got) == len(want)
    for r, (x, y) in enumerate(zip(got, want)):
        assert sorted(x) == sorted(y)
        for name in sorted(x):
            assert _bits(x[name]) == _bits(y[name]), f"rollout {r}: {name} differs"


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
def _guarded(torch, steps, n):
    """Two output slabs of steps rows with a guard row on either side, all sentinel: (whole, [steps, n] view) each."""
    whole = [torch.full((steps + 2, n), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32) for _ in range(2)]
    return whole, [w[1:steps + 1] for w in whole]


def _untouched(tensor):
    return bool((tensor.contiguous().cpu().numpy().view(np.uint32) == SENTINEL).all())


def kernel_case(torch, ctx, steps, n, bootstrap):
    """rf_rollout_advantages against gae_numpy as bytes, for the three truncation patterns; the guard rows stay."""
    from reinfocus_amd.environments import rollout

    for index, truncation in enumerate(TRUNCATIONS):
        arrays = synthetic(steps, n, truncation, 1000 * steps + 10 * n + index)
        rewards, values, truncated, final_values, last_values = arrays
        want = rollout.gae_numpy(rewards, values, truncated, final_values if bootstrap else None, last_values, GAMMA,
                                 GAE_LAMBDA)
        device = [torch.from_numpy(a).cuda() for a in arrays]
        whole, (advantages, returns) = _guarded(torch, steps, n)
        ctx.rollout_advantages(steps, n, device[0].data_ptr(), device[1].data_ptr(), device[2].data_ptr(),
                               device[3].data_ptr() if bootstrap else None, device[4].data_ptr(), GAMMA, GAE_LAMBDA,
                               advantages.data_ptr(), returns.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for name, got, expected, slab in zip(("advantages", "returns"), (advantages, returns), want, whole):
            assert _bits(got.cpu().numpy()) == _bits(expected), f"{truncation}: {name} differ"
            assert _untouched(slab[0]) and _untouched(slab[steps + 1]), f"{truncation}: a guard row of {name} was written"


def refusal_case(torch, ctx):
    """Each refusal leaves the outputs as they were: nothing was enqueued."""
    from reinfocus_amd.environments import harness, rollout

    steps, n = 5, 64
    arrays = synthetic(steps, n, "random", 5)
    rewards, values, truncated, final_values, last_values = [torch.from_numpy(a).cuda() for a in arrays]
    whole, (advantages, returns) = _guarded(torch, steps, n)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**changed):
        a = dict(steps=steps, n=n, rewards=rewards.data_ptr(), values=values.data_ptr(), truncated=truncated.data_ptr(),
                 final=final_values.data_ptr(), last=last_values.data_ptr(), advantages=advantages.data_ptr(),
                 returns=returns.data_ptr())
        a.update(changed)
        ctx.rollout_advantages(a["steps"], a["n"], a["rewards"], a["values"], a["truncated"], a["final"], a["last"], GAMMA,
                               GAE_LAMBDA, a["advantages"], a["returns"], stream)

    def refused(match, **changed):
        try:
            call(**changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        torch.cuda.synchronize()
        assert all(_untouched(w) for w in whole), f"an output was written ({match})"

    before = values.clone()
    host = np.zeros((steps, n), dtype=np.float32)
    refused("d_values is not device memory", values=host.ctypes.data)
    refused("d_returns is not device memory", returns=host.ctypes.data)
    refused("at least 1", steps=0)
    refused("at least 1", n=0)
    refused("d_advantages overlaps d_values", advantages=values.data_ptr())
    refused("d_advantages overlaps d_values", values=whole[0].data_ptr())  # (a partial overlap: rows 0 .. T-1 of the slab)
    refused("d_advantages overlaps d_returns", advantages=returns.data_ptr())
    refused("not aligned", values=values.data_ptr() + 2)
    # an allocation of its own (32 MiB: the caching allocator asks the runtime for exactly that), and an array that
    # begins so late in it that its last element lies past the end
    block = torch.zeros(32 * 1024 * 1024, dtype=torch.uint8, device="cuda")
    # (were the length check to miss it, the aliased output of the same call is refused next: nothing can run past the end)
    refused("fewer than", values=block.data_ptr() + block.numel() - 4 * (steps * n - 1), advantages=rewards.data_ptr())
    assert _bits(values.cpu().numpy()) == _bits(before.cpu().numpy())
    call()  # ... and the same arguments unchanged are taken
    torch.cuda.synchronize()
    want = rollout.gae_numpy(*arrays, GAMMA, GAE_LAMBDA)
    assert _bits(advantages.cpu().numpy()) == _bits(want[0]) and _bits(returns.cpu().numpy()) == _bits(want[1])

    # a tensor of another shape, too short: refused by DeviceRollout before the library is called
    env = make_env("steps", 3, True)
    try:
        buffer = harness.DeviceRollout(env, 2, GAMMA, GAE_LAMBDA)
        obs, _ = env.reset_tensors()
        buffer.start(obs)
        for t in range(2):
            values_t, log_probs_t = policy(obs)
            obs = buffer.step(torch.from_numpy(index_schedule(t, 3)).cuda(), values_t, log_probs_t)[0]
        for slab in (buffer.advantages, buffer.returns):
            slab.view(torch.int32).fill_(SENTINEL)
        for bad in (torch.zeros(2, device="cuda"), torch.zeros((3, 2), device="cuda"), torch.zeros(3)):
            try:
                buffer.finish(bad)
            except ValueError as caught:
                assert "shape" in str(caught) or "live on cpu" in str(caught), str(caught)
            else:
                raise AssertionError("last_values of another shape were taken")
        torch.cuda.synchronize()
        assert _untouched(buffer.advantages) and _untouched(buffer.returns)
        assert env.device_fault() is None
    finally:
        env.close()


def end_to_end_case(torch, kind, n):
    from reinfocus_amd.environments import harness

    want = twin_run(kind, n)
    env = make_env(kind, n, True)
    try:
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        got = drive(buffer, lambda: env.reset_tensors()[0], lambda a: torch.from_numpy(a).cuda(),
                    lambda a: a.cpu().numpy(), kind, n)
        same_runs(got, want)
        # the step wrote the slab itself: what step_tensors returned are rows of it
        assert buffer.observations.shape == (T + 1, n, 4 * (STACK if E2E_KINDS[kind]["view"] else 1))
        assert env.device_fault() is None
        ended = np.concatenate([run["truncated"] for run in want])
        assert ended.any(), "no environment ended"
    finally:
        env.close()


def no_sync_case(torch):
    """A whole rollout, finish(), start() and the next rollout's first step enqueued without reading anything back."""
    from reinfocus_amd.environments import harness

    kind, n = "steps", 65
    want = twin_run(kind, n, 1)
    twin_env = make_env(kind, n, False)
    twin = harness.Rollout(twin_env, T, GAMMA, GAE_LAMBDA)
    # (the twin once more, now one step into its second rollout)
    drive(twin, lambda: twin_env.reset()[0], lambda a: a, np.array, kind, n, 1)
    twin.start()
    obs_h = twin.observations[0]
    values_h, log_probs_h = policy(obs_h)
    step_h = twin.step(schedule(kind, T, n), values_h, log_probs_h)
    env = make_env(kind, n, True)
    try:
        staged = [torch.from_numpy(schedule(kind, t, n)).cuda() for t in range(T + 1)]
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        obs = env.reset_tensors()[0]
        torch.cuda.synchronize()
        buffer.start(obs)
        for t in range(T):
            values, log_probs = policy(obs)
            obs, _, _, _, info = buffer.step(staged[t], values, log_probs)
            buffer.bootstrap(info["final_observation"][:, 0] * 0.5)
        advantages, returns = buffer.finish(policy(obs)[0])
        kept = advantages.clone(), returns.clone(), buffer.observations.clone()
        buffer.start()
        values, log_probs = policy(buffer.observations[0])
        step_d = buffer.step(staged[T], values, log_probs)
        torch.cuda.synchronize()  # the only one
        assert _bits(kept[0].cpu().numpy()) == _bits(want[0]["advantages"])
        assert _bits(kept[1].cpu().numpy()) == _bits(want[0]["returns"])
        assert _bits(kept[2].cpu().numpy()) == _bits(want[0]["observations"])
        assert _bits(buffer.observations[:2].cpu().numpy()) == _bits(twin.observations[:2])
        assert _bits(step_d[0].cpu().numpy()) == _bits(step_h[0]) and _bits(step_d[1].cpu().numpy()) == _bits(step_h[1])
        assert _bits(buffer.values[0].cpu().numpy()) == _bits(twin.values[0])
        assert step_d[0].data_ptr() == buffer.observations[1].data_ptr()  # (the step's own hand-over wrote the slab)
        assert env.device_fault() is None
    finally:
        env.close()
        twin_env.close()


def surface_case(torch):
    """minibatches on the device cover every index once; the refusals of the class."""
    from reinfocus_amd.environments import harness

    n = 3
    env = make_env("no-records", n, True)
    try:
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        drive(buffer, lambda: env.reset_tensors()[0], lambda a: torch.from_numpy(a).cuda(), lambda a: a.cpu().numpy(),
              "no-records", n, 1)
        flat = buffer.flat()
        generator = torch.Generator(device="cuda")
        generator.manual_seed(5)
        batches = list(buffer.minibatches(4, generator))
        assert [len(b["returns"]) for b in batches] == [4, 4, 4, 4, 4, 1]
        generator.manual_seed(5)
        order = torch.randperm(T * n, device="cuda", generator=generator)  # (the one permutation minibatches drew)
        assert sorted(order.tolist()) == list(range(T * n))
        for key in flat:
            assert _bits(torch.cat([b[key] for b in batches]).cpu().numpy()) == _bits(flat[key][order].cpu().numpy()), key
        for call, match in ((lambda: buffer.bootstrap(torch.zeros(n, device="cuda")), "episode_records"),
                            (lambda: buffer.step(torch.zeros(n, dtype=torch.int64, device="cuda"),
                                                 torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")),
                             "already holds")):
            try:
                call()
            except ValueError as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"not refused ({match})")
    finally:
        env.close()
    kw = {k: v for k, v in ENV_KW.items() if k != "device"}
    for make, match in ((lambda: harness.DeviceVectorDiscreteSteps(num_envs=2, **ENV_KW), "device_initializer=False"),
                        (lambda: harness.DeviceVectorDiscreteSteps(num_envs=2, render_mode="rgb_array",
                                                                   device_initializer=True, **ENV_KW), "render_mode"),
                        (lambda: harness.ShardedVectorDiscreteSteps(num_envs=4, devices=[0, 0], **kw), "one GPU")):
        env = make()
        try:
            harness.DeviceRollout(env, T)
        except ValueError as caught:
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        finally:
            env.close()


def run_cases(path):
    import torch

    torch.zeros(1, device="cuda")
    from reinfocus_amd import _native
    from tests import device_io_cases as cases

    record = cases.Recorder(path)
    ctx = _native.Context(0)
    for steps, n in KERNEL_SHAPES:
        for bootstrap in (True, False):
            with record.case(f"kernel/{steps}x{n}/{'bootstrap' if bootstrap else 'plain'}"):
                kernel_case(torch, ctx, steps, n, bootstrap)
    with record.case("refusals"):
        refusal_case(torch, ctx)
    ctx.close()
    for kind in E2E_KINDS:
        for n in (E2E_SIZES if kind == "steps" else (65,)):
            with record.case(f"end-to-end/{kind}/{n}"):
                end_to_end_case(torch, kind, n)
    with record.case("no-sync"):
        no_sync_case(torch)
    with record.case("surface"):
        surface_case(torch)
    with record.case("finished"):
        pass


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    run_cases(sys.argv[1])
