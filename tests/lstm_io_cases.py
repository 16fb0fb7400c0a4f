"""TEST INFRASTRUCTURE: what tests/test_lstm_logic.py and tests/test_gpu_lstm.py share -- the networks, the sizes, hostile
inputs, states and episode starts, the chains of steps, the drivers of the end-to-end runs -- and the child process of
the GPU file.

As tests/policy_io_cases.py: everything that needs torch and the library together runs in one fresh process that imports
torch first, every case recorded as one JSON line {"id", "ok", "message"}.

    python -m tests.lstm_io_cases <results.jsonl>
    python -m tests.lstm_io_cases --torch-sequence <in.npz> <out.npz>
"""

import functools
import os
import sys

import numpy as np

from tests import policy_io_cases as policy_cases
from tests import rollout_io_cases as rollout_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = policy_cases.TILE
SIZES = (1, TILE, TILE + 1, 3 * TILE + 5)
# (obs_width, lstm_hidden, pi, vf, n_actions, activation): the least network; ppo_lstm_tuned.yml's; sb3-contrib's default
# (ppo_lstm_untuned.yml's); widths that are no multiple of a wave, one and two layers mixed, the most actions; every limit
NETWORKS = ((1, 1, (1,), (1,), 2, "relu"),
            (4, 16, (64, 64), (64, 64), 13, "relu"),
            (4, 256, (64, 64), (64, 64), 13, "tanh"),
            (7, 65, (65,), (3, 200), 64, "tanh"),
            (256, 256, (256, 256), (256,), 64, "relu"))
TUNED, DEFAULT = 1, 2
STEPS = 5  # steps of a chain
OFFSETS, MODES, SEED = policy_cases.OFFSETS, policy_cases.MODES, policy_cases.SEED
SENTINEL, SENTINEL64 = policy_cases.SENTINEL, policy_cases.SENTINEL64
OUTPUTS = policy_cases.OUTPUTS
T, ROLLOUTS = rollout_cases.T, rollout_cases.ROLLOUTS
GAMMA, GAE_LAMBDA = rollout_cases.GAMMA, rollout_cases.GAE_LAMBDA
E2E_SIZES = (1, 65)
E2E_KINDS = {"view": dict(view=True, records=True, network=TUNED), "plain": dict(view=False, records=False, network=DEFAULT)}
bits, generator_at, hostile_rows, same_runs = (policy_cases.bits, policy_cases.generator_at, policy_cases.hostile_rows,
                                               policy_cases.same_runs)


def spec_of(network):
    from reinfocus_amd.environments import lstm

    width, hidden, pi, vf, actions, activation = network
    return lstm.LstmPolicySpec(width, actions, lstm_hidden=hidden, pi=pi, vf=vf, activation=activation)


def state_dict(spec, seed, hostile=False):
    """A state_dict in sb3-contrib's names and torch's shapes: normal weights of scale 1 / sqrt(fan_in), biases of scale
    0.1.  hostile: as tests/policy_io_cases.py (two logits tie exactly, the last lies 200 below)."""
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


def hostile_state(spec, n, seed):
    """float32 [2, 2, n, H]: normal values with +-0, subnormals, large values and +-inf strewn in; environment 0 is NaN
    throughout (its start byte is set in step 0: it must come out as from a zero state), and with n > 4 environment 4
    holds a NaN and an inf that no start clears in step 0."""
    rng = np.random.default_rng(seed)
    state = rng.standard_normal(spec.state_shape(n)).astype(np.float32)
    specials = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3.0e3, -2.5e-3, np.inf, -np.inf], dtype=np.float32)
    where = rng.random(state.shape) < 0.1
    state[where] = rng.choice(specials, int(where.sum()))
    state[:, :, 0, :] = np.nan
    if n > 4:
        state[0, 0, 4, 0] = np.nan
        state[1, 1, 4, -1] = np.inf
    return state


def hostile_starts(n, steps, seed):
    """uint8 [steps, n]: bytes 0, 1, 2 and 255 mixed; in step 0 environment 0 starts (byte 255) and environment 4 does not."""
    rng = np.random.default_rng(seed)
    starts = rng.choice(np.array([0, 0, 0, 0, 1, 2, 255], dtype=np.uint8), (steps, n))
    starts[0, 0] = 255
    if n > 4:
        starts[0, 4] = 0
    if n > 1:
        starts[1, 1], starts[2, 1], starts[3, 1] = 1, 2, 0
    return starts


@functools.lru_cache(maxsize=None)
def chain_inputs(index, n):
    """(spec, params, obs [STEPS, n, D], final_obs alike, starts uint8 [STEPS, n], state [2, 2, n, H])."""
    network = NETWORKS[index]
    spec = spec_of(network)
    params = spec.pack(state_dict(spec, 100 + index, hostile=True))
    obs = np.stack([hostile_rows(network[0], n, 1000 * index + n + 31 * s, False) for s in range(STEPS)])
    final_obs = np.stack([hostile_rows(network[0], n, 7 + n + 17 * s, True) for s in range(STEPS)])
    return spec, params, obs, final_obs, hostile_starts(n, STEPS, 50 * index + n), hostile_state(spec, n, 9 * index + n)


@functools.lru_cache(maxsize=None)
def wanted_chain(index, n, mode, offset):
    """The twin's STEPS results from chain_inputs (each the dict of lstm_numpy), each step from the state of the one
    before; the draws of a sampled chain follow one another in the generator.  Computed once, shared, never changed."""
    from reinfocus_amd.environments import lstm

    spec, params, obs, final_obs, starts, state = chain_inputs(index, n)
    generator = generator_at(offset)[1]
    steps = []
    for s in range(STEPS):
        u = generator.random(n) if mode == "sampled" else None
        steps.append(lstm.lstm_numpy(spec, params, obs[s], starts[s], state, final_obs[s], u, mode == "deterministic"))
        state = steps[-1]["state"]
    return steps


# ---- the end-to-end runs -------------------------------------------------------------------------------------------------
def make_env(kind, n, device_form):
    from reinfocus_amd.environments import harness

    what = E2E_KINDS[kind]
    extra = dict(episode_records=what["records"], learner_view=harness.LearnerView(frame_stack=1) if what["view"] else None)
    if device_form:
        return harness.DeviceVectorDiscreteSteps(num_envs=n, device_initializer=True, **rollout_cases.ENV_KW, **extra)
    return harness.VectorDiscreteSteps(num_envs=n, **rollout_cases.ENV_KW, **extra)


def e2e_spec(kind):
    return spec_of(NETWORKS[E2E_KINDS[kind]["network"]])


def slabs_of(rollout, policy, unwrap, recurrent=True):
    slabs = policy_cases.slabs_of(rollout, unwrap)
    if recurrent:
        slabs.update(episode_starts=unwrap(rollout.episode_starts), lstm_states=unwrap(rollout.lstm_states))
    slabs["policy_state"] = unwrap(policy.lstm_state())
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
        seen.append(slabs_of(rollout, policy, unwrap))
    return seen


def explicit_runs(rollout, policy, reset, unwrap, records, ones, rollouts=ROLLOUTS):
    """The same by the explicit loop of start / act / step / bootstrap / finish, the caller carrying the episode starts
    (ones: every environment starts an episode at the reset).  The two recurrent slabs are collect()'s alone."""
    obs = reset()
    seen = []
    starts = ones
    for r in range(rollouts):
        rollout.start(obs if r == 0 else None)
        obs = rollout.observations[0]
        final_obs = None
        for _ in range(T):
            actions, values, log_probs, final_values = policy.act(obs, starts, final_obs)
            if final_obs is not None:
                rollout.bootstrap(final_values)
            obs, _, _, starts, info = rollout.step(actions, values, log_probs)
            final_obs = info["final_observation"] if records else None
        if records:
            last_values, final_values = policy.values(obs, starts, final_obs)
            rollout.bootstrap(final_values)
        else:
            last_values = policy.values(obs, starts)
        rollout.finish(last_values)
        seen.append(slabs_of(rollout, policy, unwrap, recurrent=False))
    return seen


def without_recurrent(runs):
    return [{k: v for k, v in run.items() if k not in ("episode_starts", "lstm_states")} for run in runs]


def twin_runs(kind, n, rollouts=ROLLOUTS, explicit=False, second_state=None):
    """The numpy twins' rollouts; second_state: the state_dict seed loaded before rollout 1.  Returns (runs, policy)."""
    from reinfocus_amd.environments import harness

    env = make_env(kind, n, False)
    try:
        spec = e2e_spec(kind)
        policy = harness.LstmPolicy(spec, SEED, num_envs=n)
        policy.load_state_dict(state_dict(spec, 3))
        rollout = harness.Rollout(env, T, GAMMA, GAE_LAMBDA)
        if explicit:
            return explicit_runs(rollout, policy, lambda: env.reset()[0], np.array, E2E_KINDS[kind]["records"],
                                 np.ones(n, dtype=np.uint8), rollouts), policy
        between = None if second_state is None else lambda r: policy.load_state_dict(state_dict(spec, second_state))
        return collect_runs(rollout, policy, lambda: env.reset()[0], np.array, rollouts, between), policy
    finally:
        env.close()


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
def _guarded(torch, n, count):
    return policy_cases._guarded(torch, n, count)


_untouched = policy_cases._untouched


def _guarded_state(torch, spec, n, fill=None):
    """A state with a guard row of H floats on either side, all sentinel: (whole, the [2, 2, n, H] view)."""
    hidden = spec.lstm_hidden
    whole = torch.full((4 * n + 2, hidden), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    view = whole[1:4 * n + 1].view(2, 2, n, hidden)
    if fill is not None:
        view.copy_(torch.from_numpy(fill).cuda())
    return whole, view


def _guards_kept(whole):
    return _untouched(whole[0]) and _untouched(whole[-1])


def _call(torch, ctx, spec, params, n, obs, starts, final_obs, state_in, state_out, gen, flags, out, changed=()):
    a = dict(desc=spec.desc(), params=params.data_ptr(), n=n, obs=obs.data_ptr(), starts=starts.data_ptr(),
             final_obs=None if final_obs is None else final_obs.data_ptr(), state_in=state_in.data_ptr(),
             state_out=None if state_out is None else state_out.data_ptr(), gen=gen, flags=flags)
    a.update({name: tensor.data_ptr() for name, tensor in out.items()})
    a.update(changed)  # (arguments given by their names above, in place of the tensors')
    ctx.lstm_forward(a["desc"], a["params"], a["n"], a["obs"], a["starts"], a["final_obs"], a["state_in"], a["state_out"],
                     a["gen"], a["flags"], a["actions"], a["log_probs"], a["values"], a["final_values"], a["logits"],
                     torch.cuda.current_stream().cuda_stream)


def kernel_case(torch, ctx, index, n):
    """rf_lstm_forward against lstm_numpy as bytes over a chain of STEPS steps: sampled at both draw offsets and
    deterministic, each with the state in place and from one buffer into another; then a values-only call and a call
    that advances the state only."""
    from reinfocus_amd.environments import lstm, policy

    spec, params_h, obs_h, final_h, starts_h, state_h = chain_inputs(index, n)
    assert ctx.lstm_params_size(spec.desc()) == spec.size
    assert ctx.lstm_state_size(spec.desc(), n) == state_h.size
    params, obs, final_obs, starts = (torch.from_numpy(a).cuda() for a in (params_h, obs_h, final_h, starts_h))
    for mode, offset in MODES:
        want = wanted_chain(index, n, mode, offset)
        for in_place in (True, False):
            buffers = [_guarded_state(torch, spec, n, state_h), _guarded_state(torch, spec, n)]
            bit_generator = generator_at(offset)[0]
            for s in range(STEPS):
                source = buffers[0] if in_place else buffers[s % 2]
                target = buffers[0] if in_place else buffers[(s + 1) % 2]
                whole, out = _guarded(torch, n, spec.n_actions)
                gen = policy.generator_words(bit_generator) if mode == "sampled" else None
                _call(torch, ctx, spec, params, n, obs[s], starts[s], final_obs[s], source[1], target[1], gen,
                      0 if mode == "sampled" else policy.DETERMINISTIC, out)
                if mode == "sampled":
                    bit_generator.advance(n)
                torch.cuda.synchronize()
                where = f"{mode} at {offset}, {'in place' if in_place else 'apart'}, step {s}"
                for name in OUTPUTS:
                    assert bits(out[name].cpu().numpy()) == bits(want[s][name]), f"{where}: {name} differ"
                    assert _untouched(whole[name][0]) and _untouched(whole[name][n + 1]), f"{where}: a guard row of {name}"
                assert bits(target[1].cpu().numpy()) == bits(want[s]["state"]), f"{where}: the state differs"
                assert _guards_kept(target[0]) and _guards_kept(source[0]), f"{where}: a guard row of the state"
                if not in_place and s > 0:  # (the source keeps what the step before wrote)
                    assert bits(source[1].cpu().numpy()) == bits(want[s - 1]["state"]), f"{where}: the source changed"
    # values only: the vf net alone, masked; no draw; the state bytes stay
    whole_state, state = _guarded_state(torch, spec, n, state_h)
    whole, out = _guarded(torch, n, spec.n_actions)
    _call(torch, ctx, spec, params, n, obs[0], starts[0], final_obs[0], state, None, None, 0, out,
          dict(actions=None, log_probs=None, logits=None))
    torch.cuda.synchronize()
    want = lstm.lstm_numpy(spec, params_h, obs_h[0], starts_h[0], state_h, final_h[0], values_only=True)
    assert bits(out["values"].cpu().numpy()) == bits(want["values"]) == bits(wanted_chain(index, n, "deterministic", 0)[0]["values"])
    assert bits(out["final_values"].cpu().numpy()) == bits(want["final_values"])
    assert all(_untouched(whole[name]) for name in ("actions", "log_probs", "logits"))
    assert bits(state.cpu().numpy()) == bits(state_h) and _guards_kept(whole_state), "a values-only call wrote the state"
    # the state only: both cells run, no head does
    whole_target, target = _guarded_state(torch, spec, n)
    _call(torch, ctx, spec, params, n, obs[0], starts[0], None, state, target, None, 0, out,
          dict(actions=None, log_probs=None, logits=None, values=None, final_values=None))
    torch.cuda.synchronize()
    assert bits(target.cpu().numpy()) == bits(wanted_chain(index, n, "deterministic", 0)[0]["state"])
    assert _guards_kept(whole_target) and bits(state.cpu().numpy()) == bits(state_h)
    assert all(_untouched(whole[name]) for name in ("actions", "log_probs", "logits"))


def refusal_case(torch, ctx):
    """Each refusal leaves the outputs and the state as they were: nothing was enqueued."""
    from reinfocus_amd.environments import policy

    index, n = TUNED, TILE + 1
    spec, params_h, obs_h, final_h, starts_h, state_h = chain_inputs(index, n)
    params, obs, final_obs, starts = (torch.from_numpy(a).cuda() for a in (params_h, obs_h[0], final_h[0], starts_h[0]))
    whole, out = _guarded(torch, n, spec.n_actions)
    whole_in, state_in = _guarded_state(torch, spec, n, state_h)
    whole_out, state_out = _guarded_state(torch, spec, n)
    gen = policy.generator_words(generator_at(0)[0])

    def refused(match, **changed):
        try:
            _call(torch, ctx, spec, params, n, obs, starts, final_obs, state_in, state_out, gen, 0, out, changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        torch.cuda.synchronize()
        assert all(_untouched(w) for w in whole.values()), f"an output was written ({match})"
        assert _untouched(whole_out) and bits(state_in.cpu().numpy()) == bits(state_h), f"a state was written ({match})"

    host = np.zeros((n + 2, max(spec.obs_width, 4 * spec.lstm_hidden)), dtype=np.float32)
    refused("d_obs is not device memory", obs=host.ctypes.data)
    refused("d_values is not device memory", values=host.ctypes.data)
    refused("d_params is not device memory", params=params_h.ctypes.data)
    refused("d_episode_starts is not device memory", starts=starts_h.ctypes.data)
    refused("d_state_in is not device memory", state_in=state_h.ctypes.data)
    refused("at least 1", n=0)
    refused("not aligned", obs=obs.data_ptr() + 2)
    refused("not aligned", actions=out["actions"].data_ptr() + 4)
    refused("not aligned", state_out=state_out.data_ptr() + 2)
    refused("d_values overlaps d_obs", values=obs.data_ptr())
    refused("d_values overlaps d_log_probs", values=out["log_probs"].data_ptr())
    refused("d_logits overlaps d_params", logits=params.data_ptr())
    refused("d_values overlaps d_state_in", values=state_in.data_ptr())
    refused("d_state_out overlaps d_values", values=state_out.data_ptr())
    refused("d_state_out overlaps d_state_in without being it", state_out=state_in.data_ptr() + 4 * spec.lstm_hidden)
    refused("d_state_out overlaps d_state_in without being it", state_out=state_in.data_ptr() - 4)
    block = torch.zeros(32 * 1024 * 1024, dtype=torch.uint8, device="cuda")  # (an allocation of its own)
    # (were the length check to miss it, the aliased output of the same call is refused next: nothing can run past the end)
    alias = out["log_probs"].data_ptr()
    refused("fewer than", obs=block.data_ptr() + block.numel() - 4 * (n * spec.obs_width - 1), values=alias)
    refused("fewer than", params=block.data_ptr() + block.numel() - 4 * (spec.size - 1), values=alias)
    refused("fewer than", state_in=block.data_ptr() + block.numel() - 4 * (state_h.size - 1), values=alias)
    # (d_state_out is the last array checked, so no alias can stand behind it: the same check with the same length has
    # just refused d_state_in)
    refused("d_state_out has fewer than", state_out=block.data_ptr() + block.numel() - 4 * (state_h.size - 1))
    refused("fewer than", starts=block.data_ptr() + block.numel() - (n - 1), values=alias)
    desc = list(spec.desc())
    for field, value in ((0, 0), (0, 257), (1, 1), (1, 65), (2, 2), (3, 0), (3, 3), (4, 257), (5, 0), (6, 3), (7, 0), (9, 0),
                         (9, 257), (9, -1)):
        refused("outside the limits", desc=tuple(desc[:field] + [value] + desc[field + 1:]))
    refused("unknown flags", flags=2)
    refused("needs gen", gen=None)
    refused("needs d_final_obs", final_obs=None)
    refused("d_log_probs are those of d_actions", actions=None)
    refused("NULL argument", starts=None)
    refused("NULL argument", state_in=None)
    refused("no output is asked for", state_out=None, actions=None, log_probs=None, values=None, final_values=None, logits=None)
    _call(torch, ctx, spec, params, n, obs, starts, final_obs, state_in, state_out, gen, 0, out)  # ... unchanged: taken
    torch.cuda.synchronize()
    want = wanted_chain(index, n, "sampled", 0)[0]
    for name in OUTPUTS:
        assert bits(out[name].cpu().numpy()) == bits(want[name]), name
    assert bits(state_out.cpu().numpy()) == bits(want["state"]) and _guards_kept(whole_out)


def _device_policy(torch, harness, env, kind, state_seed=3):
    spec = e2e_spec(kind)
    policy = harness.DeviceLstmPolicy(env, spec, SEED)
    policy.load_state_dict({k: torch.from_numpy(v).cuda() for k, v in state_dict(spec, state_seed).items()})
    return spec, policy


def _unwrap(tensor):
    return tensor.cpu().numpy()


def end_to_end_case(torch, kind, n):
    from reinfocus_amd.environments import harness

    want, twin = twin_runs(kind, n)
    env = make_env(kind, n, True)
    try:
        spec, policy = _device_policy(torch, harness, env, kind)
        assert bits(policy.params.cpu().numpy()) == bits(spec.pack(state_dict(spec, 3)))
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        assert buffer.episode_starts is None and buffer.lstm_states is None  # (made on first use)
        got = collect_runs(buffer, policy, lambda: env.reset_tensors()[0], _unwrap)
        same_runs(got, want)
        assert env.device_fault() is None
        assert np.concatenate([run["truncated"] for run in want]).any(), "no environment ended"
        for r, run in enumerate(got):
            assert bits(run["episode_starts"][1:]) == bits(run["truncated"])
            assert bits(run["lstm_states"][T]) == bits(run["policy_state"])
            assert (run["episode_starts"][0] == 1).all() if r == 0 else \
                bits(run["episode_starts"][0]) == bits(got[r - 1]["truncated"][T - 1])
            assert bits(run["lstm_states"][0]) == bits(got[r - 1]["policy_state"] if r else np.zeros_like(run["policy_state"]))
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
            reset = lambda: env.reset_tensors()[0]  # noqa: E731
            ones = torch.ones(n, dtype=torch.uint8, device="cuda")
            runs.append(explicit_runs(buffer, policy, reset, _unwrap, True, ones) if explicit
                        else collect_runs(buffer, policy, reset, _unwrap))
            assert env.device_fault() is None
        finally:
            env.close()
    same_runs(without_recurrent(runs[0]), runs[1])
    same_runs(runs[0], twin_runs(kind, n)[0])


def no_sync_case(torch):
    """Two collects enqueued back to back, nothing read in between; one synchronisation at the end."""
    from reinfocus_amd.environments import harness

    kind, n = "view", 65
    want = twin_runs(kind, n)[0]
    env = make_env(kind, n, True)
    try:
        _, policy = _device_policy(torch, harness, env, kind)
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        obs = env.reset_tensors()[0]
        torch.cuda.synchronize()
        buffer.start(obs)
        advantages, returns = buffer.collect(policy)
        names = ("observations", "actions", "log_probs", "final_values", "episode_starts", "lstm_states")
        kept = {name: getattr(buffer, name).clone() for name in names}
        kept.update(advantages=advantages.clone(), returns=returns.clone())
        buffer.start()
        buffer.collect(policy)
        torch.cuda.synchronize()  # the only one
        for name, tensor in kept.items():
            assert bits(tensor.cpu().numpy()) == bits(want[0][name]), name
        for name in names + ("values", "advantages", "returns"):
            assert bits(getattr(buffer, name).cpu().numpy()) == bits(want[1][name]), name
        assert bits(policy.lstm_state().cpu().numpy()) == bits(want[1]["policy_state"])
        assert env.device_fault() is None
    finally:
        env.close()


def reload_case(torch):
    """load_state_dict between two collects changes the second one exactly as the twin's does."""
    from reinfocus_amd.environments import harness

    kind, n = "plain", 9
    want = twin_runs(kind, n, second_state=4)[0]
    unchanged = twin_runs(kind, n)[0]
    assert bits(want[0]["actions"]) == bits(unchanged[0]["actions"])
    assert bits(want[1]["log_probs"]) != bits(unchanged[1]["log_probs"])  # (the new parameters matter)
    env = make_env(kind, n, True)
    try:
        spec, policy = _device_policy(torch, harness, env, kind)
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        second = {k: torch.from_numpy(v).cuda() for k, v in state_dict(spec, 4).items()}
        got = collect_runs(buffer, policy, lambda: env.reset_tensors()[0], _unwrap,
                           between=lambda r: policy.load_state_dict(second))
        same_runs(got, want)
        back = policy.state_dict()
        for name, value in state_dict(spec, 4).items():
            assert bits(back[name].cpu().numpy()) == bits(value), name
    finally:
        env.close()


def feedforward_case(torch):
    """A rollout that only ever sees DevicePolicy never has the two recurrent slabs."""
    from reinfocus_amd.environments import harness

    env = policy_cases.make_env("plain", 3, True)
    try:
        _, policy = policy_cases._device_policy(torch, harness, env, "plain")
        buffer = harness.DeviceRollout(env, T, GAMMA, GAE_LAMBDA)
        got = policy_cases.collect_runs(buffer, policy, lambda: env.reset_tensors()[0], _unwrap)
        same_runs(got, policy_cases.twin_runs("plain", 3))
        assert buffer.episode_starts is None and buffer.lstm_states is None
    finally:
        env.close()


def surface_case(torch):
    """A Box action space is refused; act() without out= and deterministic; the state's accessors; bad inputs."""
    from reinfocus_amd.environments import harness

    env = harness.DeviceVectorContinuousJumps(num_envs=2, device_initializer=True, **rollout_cases.ENV_KW)
    try:
        try:
            harness.DeviceLstmPolicy(env, e2e_spec("view"), 0)
        except ValueError as caught:
            assert "out of scope" in str(caught) and "sde" in str(caught), str(caught)
        else:
            raise AssertionError("a Box action space was taken")
    finally:
        env.close()
    n = 5
    env = make_env("view", n, True)
    try:
        spec, policy = _device_policy(torch, harness, env, "view")
        twin = harness.LstmPolicy(spec, SEED, num_envs=n)
        twin.load_state_dict(state_dict(spec, 3))
        obs_h = hostile_rows(4, n, 5, False)
        starts_h = np.array([0, 1, 0, 255, 0], dtype=np.uint8)
        obs, starts = torch.from_numpy(obs_h).cuda(), torch.from_numpy(starts_h).cuda()
        start_state = hostile_state(spec, n, 1)
        start_state[:, :, 0, :] = 0.5
        policy.set_lstm_state(torch.from_numpy(start_state).cuda())
        twin.set_lstm_state(start_state)
        before = policy.rng_state()
        for deterministic in (True, False):
            got = policy.act(obs, starts, deterministic=deterministic)
            want = twin.act(obs_h, starts_h, deterministic=deterministic)
            assert got[3] is None and want[3] is None
            for x, y in zip(got[:3], want[:3]):
                assert bits(x.cpu().numpy()) == bits(y)
            assert bits(policy.lstm_state().cpu().numpy()) == bits(twin.lstm_state())
            assert (policy.rng_state() == before) == deterministic
        kept = policy.lstm_state()
        assert bits(policy.values(obs, starts).cpu().numpy()) == bits(twin.values(obs_h, starts_h))
        assert bits(policy.lstm_state().cpu().numpy()) == bits(kept.cpu().numpy())  # (values() never advances the state)
        assert policy.rng_state() == twin.rng_state()
        apart = (policy.lstm_state(), torch.zeros_like(kept))
        policy.act(obs, starts, deterministic=True, states=apart)
        twin_apart = (twin.lstm_state(), np.zeros_like(twin.lstm_state()))
        twin.act(obs_h, starts_h, deterministic=True, states=twin_apart)
        assert bits(apart[1].cpu().numpy()) == bits(twin_apart[1])
        assert bits(policy.lstm_state().cpu().numpy()) == bits(kept.cpu().numpy())  # (the own state stayed)
        for bad, error in (((obs[:, :3], starts), ValueError), ((obs.double(), starts), ValueError), ((obs_h, starts), TypeError),
                           ((obs.cpu(), starts), ValueError), ((obs, starts_h), TypeError), ((obs, starts.float()), ValueError),
                           ((obs[:4], starts[:4]), ValueError)):
            try:
                policy.act(*bad)
            except error:
                pass
            else:
                raise AssertionError("inputs of another kind were taken")
        try:
            policy.act(obs, starts, states=(kept, kept[:, :, :4]))
        except ValueError:
            pass
        else:
            raise AssertionError("a state of another shape was taken")
        assert policy.rng_state() == twin.rng_state()  # (a refused call consumes nothing)
        policy.reset_state()
        assert not policy.lstm_state().cpu().numpy().any()
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
    with record.case("feedforward"):
        feedforward_case(torch)
    with record.case("surface"):
        surface_case(torch)
    with record.case("finished"):
        pass


# ---- torch's own recurrent forward (CPU), for the accuracy test ---------------------------------------------------------------
SEQUENCE_STEPS, SEQUENCE_ROWS = 16, 32


def sequence_inputs(index):
    """(spec, state_dict, obs float32 [16, 32, D] of normal rows, starts uint8 [16, 32] with three episode starts inside
    the sequence -- whole rows of the batch at steps 4 and 9, every other environment at step 12)."""
    spec = spec_of(NETWORKS[index])
    obs = np.random.default_rng(index).standard_normal((SEQUENCE_STEPS, SEQUENCE_ROWS, spec.obs_width)).astype(np.float32)
    starts = np.zeros((SEQUENCE_STEPS, SEQUENCE_ROWS), dtype=np.uint8)
    starts[4], starts[9], starts[12, ::2] = 1, 1, 1
    return spec, state_dict(spec, 50 + index), obs, starts


def torch_sequence(path_in, path_out):
    """torch.nn.LSTM x 2, the state masked by (1 - start) as sb3-contrib does, nn.Sequential MLPs and the heads, from a
    zero state over the sequence of path_in -- in float32 and in float64 from the same state_dict.  In a process of its
    own: torch brings a HIP runtime of its own."""
    import torch

    data = np.load(path_in)
    skip = ("obs", "starts", "activation")
    act = torch.nn.Tanh if str(data["activation"]) == "tanh" else torch.nn.ReLU
    results = {}
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        tensors = {k: torch.from_numpy(data[k]).to(dtype) for k in data.files if k not in skip}
        obs = torch.from_numpy(data["obs"]).to(dtype)
        keep = 1.0 - torch.from_numpy(data["starts"]).to(dtype)
        hidden = tensors["lstm_actor.weight_hh_l0"].shape[1]

        def net(lstm_name, extractor, head_name):
            lstm = torch.nn.LSTM(obs.shape[2], hidden, num_layers=1).to(dtype)
            lstm.load_state_dict({part: tensors[f"{lstm_name}.{part}"] for part in
                                  ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
            layers, keys = [], []
            for i in (0, 2):
                if f"mlp_extractor.{extractor}.{i}.weight" in tensors:
                    weight = tensors[f"mlp_extractor.{extractor}.{i}.weight"]
                    layers += [torch.nn.Linear(weight.shape[1], weight.shape[0]), act()]
                    keys.append(f"mlp_extractor.{extractor}.{i}")
            weight = tensors[head_name + ".weight"]
            mlp = torch.nn.Sequential(*layers, torch.nn.Linear(weight.shape[1], weight.shape[0])).to(dtype)
            mlp.load_state_dict({f"{2 * j}.{part}": tensors[f"{key}.{part}"] for j, key in enumerate(keys + [head_name])
                                 for part in ("weight", "bias")})
            h = torch.zeros(1, obs.shape[1], hidden, dtype=dtype)
            c = torch.zeros_like(h)
            outs = []
            for t in range(obs.shape[0]):
                mask = keep[t].view(1, -1, 1)
                out, (h, c) = lstm(obs[t:t + 1], (h * mask, c * mask))
                outs.append(mlp(out[0]))
            return torch.stack(outs), h[0], c[0]

        with torch.no_grad():
            logits, h_pi, c_pi = net("lstm_actor", "policy_net", "action_net")
            values, h_vf, c_vf = net("lstm_critic", "value_net", "value_net")
        results["logits" + tag] = logits.numpy()
        results["values" + tag] = values[:, :, 0].numpy()
        results["state" + tag] = torch.stack([torch.stack([h_pi, c_pi]), torch.stack([h_vf, c_vf])]).numpy()
    np.savez(path_out, **results)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1] == "--torch-sequence":
        torch_sequence(sys.argv[2], sys.argv[3])
    else:
        run_cases(sys.argv[1])
