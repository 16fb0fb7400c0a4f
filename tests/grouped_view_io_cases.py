"""TEST INFRASTRUCTURE: the cases of tests/test_gpu_grouped_view.py and its child process.

The population view (include/reinfocus_hip.h, "population view"): a learner view with running moments and a gamma per
group of lanes, and GAE with discounts per group.  As tests/learner_view_io_cases.py: everything that needs torch and
the library together runs in one fresh process that imports torch first, every case recorded as one JSON line
{"id", "ok", "message"}.  Everything is compared as bytes against the numpy twins (harness._GroupedLearnerView, literally
G _LearnerView objects over lane slices; rollout.gae_numpy_grouped, gae_numpy per slice).

    python -m tests.grouped_view_io_cases <results.jsonl>

The head of the file (shapes, gammas, statistics, the hand-driven oracle) imports neither torch nor the library, so that
tests/test_grouped_view_logic.py computes on the CPU what the GPU cases rely on.
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK, STEPS, WIDTH = 5, 12, 4
SEED = 13  # tests/device_io_cases.make_env's

# (n, G): the reference's group size; a segment of one lane; a ragged segment whose last block is partly idle; a segment
# of 32 lanes; a whole wave per group; the block form with P_m = 128; the block form with two leaves per thread
VIEW_SHAPES = ((64, 8), (65, 65), (65, 13), (96, 3), (128, 2), (130, 2), (2050, 2))
# one case per shape -- the composed kinds end a part of the environments; records on at some shapes, off at others --
# and one each without norm_obs, without norm_reward, and with training switched off half-way
VIEW_CASES = tuple(
    [dict(kind="composed-i64" if index % 2 == 0 else "composed-i32", n=n, groups=groups, records=index % 2 == 0,
          config={}, freeze=False) for index, (n, groups) in enumerate(VIEW_SHAPES)]
    + [dict(kind="composed-i64", n=64, groups=8, records=True, config=dict(norm_obs=False), freeze=False),
       dict(kind="composed-i32", n=65, groups=13, records=True, config=dict(norm_reward=False), freeze=False),
       dict(kind="composed-i64", n=96, groups=3, records=False, config={}, freeze=True)])

GAE_STEPS = (1, 33, 70)  # one, two and three LDS chunks of rf::kRolloutChunk = 32 steps
GAE_SHAPES = ((1, 1), (64, 8), (65, 65), (65, 13), (130, 2))

E2E = dict(groups=4, per_group=8, steps=4, batch=8, epochs=2, iterations=2)
E2E_GAMMAS, E2E_LAMBDAS = (0.99, 0.9, 1.0, 0.5), (0.95, 1.0, 0.8, 0.0)
E2E_VIEW_GAMMAS = (0.99, 0.9, 1.0, 0.0)


def case_id(case):
    extra = ",".join(f"{k}={v}" for k, v in case["config"].items()) + (",freeze" if case["freeze"] else "")
    return f"view/{case['kind']}/{case['n']}x{case['groups']}/{'records' if case['records'] else 'plain'}" + (
        "/" + extra.strip(",") if extra else "")


def gammas_of(groups):
    """Gammas that differ per group and include 0.0 and 1.0 wherever there are two groups."""
    return tuple((0.0, 1.0, 0.99, 0.9, 0.95, 0.5, 0.999)[g % 7] for g in range(groups))


def lambdas_of(groups):
    return tuple((1.0, 0.0, 0.92, 0.95, 0.8)[g % 5] for g in range(groups))


def statistics_of(groups, width=WIDTH):
    """Distinct statistics per group and slot, set before the first step."""
    g, c = np.arange(groups, dtype=np.float64)[:, None], np.arange(width + 1, dtype=np.float64)[None, :]
    return {"mean": 0.01 * g - 0.1 * c + 0.05, "var": 1.0 + 0.5 * (g % 5) + 0.25 * c, "count": 3.0 + (g % 7) + 0.5 * c}


def bits(a):
    a = np.asarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def make_view(case):
    from reinfocus_amd.environments import harness

    return harness.LearnerView(frame_stack=STACK, gamma=gammas_of(case["groups"]), groups=case["groups"], **case["config"])


def make_twin_env(case, **extra):
    """The numpy twin of tests/device_io_cases.make_env(kind, n) for the composed kinds."""
    from reinfocus_amd.environments import harness
    from tests.test_gpu_device_initializer import _objects

    assert case["kind"].startswith("composed")
    return harness.VectorEnvironment(**_objects(case["n"], "multi", SEED), samples_per_pixel=1 + case["n"] % 2,
                                     frame_height=16, device=0, **extra)


HOLD_STEPS, HOLD_ACTION = 3, 6  # action 6 moves nothing: a lane that holds for the ender's three steps ends by the limit


def host_actions(case, rng, index):
    """The index actions of step `index`: drawn, except that the lanes of the even groups hold during the first three
    steps -- none of them ends in steps 0 and 1, all of them end in step 2 (TimeLimitEnder(3)) --, while the odd groups
    and every later step end a part of their lanes (DivergingEnder).  tests/test_grouped_view_logic.py checks that."""
    dtype = "int64" if case["kind"].endswith("i64") else "int32"
    actions = rng.integers(0, 13, case["n"])
    if index < HOLD_STEPS:
        even = (np.arange(case["n"]) // (case["n"] // case["groups"])) % 2 == 0
        actions[even] = HOLD_ACTION
    return actions.astype(dtype)


class Oracle:
    """G private _LearnerView objects of m lanes each, fed slice by slice with a step's raw results: the definition by
    hand, without _GroupedLearnerView."""

    def __init__(self, view, n, width=WIDTH):
        from reinfocus_amd.environments import harness

        self.groups, self.m = view.groups, n // view.groups
        self.views = [harness._LearnerView(harness.LearnerView(
            frame_stack=view.frame_stack, norm_obs=view.norm_obs, norm_reward=view.norm_reward, gamma=view.gammas[g],
            epsilon=view.epsilon, clip_obs=view.clip_obs, clip_reward=view.clip_reward, training=view.training), self.m,
            width) for g in range(self.groups)]

    def lanes(self, g):
        return slice(g * self.m, (g + 1) * self.m)

    def set_statistics(self, statistics):
        for g, view in enumerate(self.views):
            view.set_statistics(statistics["mean"][g], statistics["var"][g], statistics["count"][g])

    def set_training(self, training):
        for view in self.views:
            view.training = training

    def reset(self, raw):
        return np.concatenate([view.reset(raw[self.lanes(g)]) for g, view in enumerate(self.views)])

    def step(self, raw, rewards, done, raw_final):
        parts = [view.step(raw[self.lanes(g)], rewards[self.lanes(g)], done[self.lanes(g)],
                           None if raw_final is None else raw_final[self.lanes(g)]) for g, view in enumerate(self.views)]
        return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                None if raw_final is None else np.concatenate([p[2] for p in parts]))

    def state(self):
        return (np.concatenate([view.stack for view in self.views]), np.concatenate([view.returns for view in self.views]))

    def statistics(self):
        return {key: np.stack([getattr(view, key) for view in self.views]) for key in ("mean", "var", "count")}


def group_ends(done, groups):
    """Per step of `done` [steps, n]: how many lanes of each group ended, [steps, G]."""
    done = np.asarray(done)
    return done.reshape(done.shape[0], groups, -1).sum(axis=2)


def ends_promises(done, groups):
    """What the view cases rely on: some step has a group where none end, one where all end, and -- for groups of more
    than one lane, where alone it can happen -- one where some but not all end."""
    counts, m = group_ends(done, groups), np.asarray(done).shape[1] // groups
    assert (counts == 0).any(), "no step has a group where no lane ends"
    assert (counts == m).any(), "no step has a group where every lane ends"
    assert m == 1 or ((counts > 0) & (counts < m)).any(), "no step has a group where some but not all lanes end"


def same_view(env, oracle):
    for name, x, y in zip(("stack", "returns"), env.view_state(), oracle.state()):
        assert bits(x) == bits(y), f"the {name} differ"
    got, want = env.view_statistics(), oracle.statistics()
    for key in ("mean", "var", "count"):
        assert bits(got[key]) == bits(want[key]), f"the statistics' {key} differs"


def drive_view(case, env, reset, step, freeze_env):
    """STEPS steps of `env` held to the hand-driven oracle after each; reset() and step(index, actions) return the
    host-form results as numpy.  Returns the steps' done flags [STEPS, n]."""
    view, n = make_view(case), case["n"]
    oracle = Oracle(view, n)
    statistics = statistics_of(case["groups"])
    env.set_view_statistics(statistics)
    oracle.set_statistics(statistics)
    same_view(env, oracle)
    obs, info = reset()
    assert sorted(info) == ["raw_observation"] and obs.shape == (n, WIDTH * STACK) and obs.dtype == np.float32
    assert bits(obs) == bits(oracle.reset(info["raw_observation"])), "the reset's view observation differs"
    same_view(env, oracle)
    rng = np.random.default_rng(6)
    ended = []
    for index in range(STEPS):
        if case["freeze"] and index == STEPS // 2:
            freeze_env(env)
            oracle.set_training(False)
        got = step(index, host_actions(case, rng, index))
        done = got[2] | got[3]
        raw_final = got[4].get("raw_final_observation")
        assert (raw_final is not None) == case["records"]
        want = oracle.step(got[4]["raw_observation"], got[4]["raw_reward"], done, raw_final)
        assert bits(got[0]) == bits(want[0]), f"step {index}: the view observation differs"
        assert bits(got[1]) == bits(want[1]), f"step {index}: the view reward differs"
        if case["records"]:
            assert bits(got[4]["final_observation"]) == bits(want[2]), f"step {index}: final_observation differs"
        same_view(env, oracle)
        ended.append(done.copy())
    return np.array(ended)


def gae_inputs(steps, n, seed):
    from tests import rollout_io_cases

    return rollout_io_cases.synthetic(steps, n, "random", seed)


# ---- the child process: everything below needs torch and a GPU ------------------------------------------------------
def _numpy_step(torch, got):
    def host(x):
        return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)

    return tuple(host(x) for x in got[:4]) + ({key: host(value) for key, value in got[4].items()},)


def view_case(torch, cases, case):
    """step() and step_tensors() mixed step by step on a grouped device context against the hand-driven oracle."""
    env = cases.make_env(case["kind"], case["n"], episode_records=case["records"], learner_view=make_view(case))
    try:
        def step(index, actions):
            if index % 3 == 1:  # the host form in between
                return _numpy_step(torch, env.step(actions))
            return _numpy_step(torch, env.step_tensors(torch.from_numpy(actions).cuda()))

        done = drive_view(case, env, lambda: _reset_numpy(env), step, lambda e: e.set_view_training(False))
        ends_promises(done, case["groups"])
        assert env.device_fault() is None
        row = env.view_statistics(group=case["groups"] - 1)
        assert all(bits(row[key]) == bits(env.view_statistics()[key][-1]) for key in row)
    finally:
        env.close()


def one_group_case(torch, cases):
    """groups=1 against an ungrouped context at n = 65: every byte, only the statistics' shape differs."""
    from reinfocus_amd.environments import harness

    n, kind = 65, "composed-i64"
    plain = cases.make_env(kind, n, episode_records=True, learner_view=harness.LearnerView(frame_stack=STACK, gamma=0.9))
    one = cases.make_env(kind, n, episode_records=True,
                         learner_view=harness.LearnerView(frame_stack=STACK, gamma=[0.9], groups=1))
    try:
        a, b = plain.reset_tensors(), one.reset_tensors()
        assert bits(a[0].cpu().numpy()) == bits(b[0].cpu().numpy())
        rng = np.random.default_rng(6)
        for index in range(STEPS):
            actions = rng.integers(0, 13, n)
            if index % 3 == 1:
                x, y = _numpy_step(torch, plain.step(actions)), _numpy_step(torch, one.step(actions))
            else:
                x = _numpy_step(torch, plain.step_tensors(torch.from_numpy(actions).cuda()))
                y = _numpy_step(torch, one.step_tensors(torch.from_numpy(actions).cuda()))
            assert sorted(x[4]) == sorted(y[4])
            for name, p, q in list(zip("0123", x[:4], y[:4])) + [(key, x[4][key], y[4][key]) for key in sorted(x[4])]:
                assert bits(p) == bits(q), f"step {index}: result {name} differs"
            for p, q in zip(plain.view_state(), one.view_state()):
                assert bits(p) == bits(q)
            s, t = plain.view_statistics(), one.view_statistics()
            for key in ("mean", "var", "count"):
                assert t[key].shape == (1, WIDTH + 1) and bits(s[key]) == bits(t[key][0]), key
    finally:
        plain.close()
        one.close()


def _gae_device(torch, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def gae_case(torch, ctx, steps):
    """rf_rollout_advantages_grouped against gae_numpy_grouped as bytes, with and without final_values; the guard rows
    stay; G = 1 is also rf_rollout_advantages."""
    from reinfocus_amd.environments import rollout
    from tests import rollout_io_cases as rc

    stream = torch.cuda.current_stream().cuda_stream
    for n, groups in GAE_SHAPES:
        gammas, lambdas = gammas_of(groups), lambdas_of(groups)
        if groups == 1:
            gammas, lambdas = (0.99,), (0.92,)
        arrays = gae_inputs(steps, n, 7000 + 100 * steps + n + groups)
        device = _gae_device(torch, arrays)
        table = torch.from_numpy(rollout.discount_table(gammas, lambdas)).cuda()
        for bootstrap in (True, False):
            want = rollout.gae_numpy_grouped(arrays[0], arrays[1], arrays[2], arrays[3] if bootstrap else None, arrays[4],
                                             gammas, lambdas)
            whole, (advantages, returns) = rc._guarded(torch, steps, n)
            ctx.rollout_advantages_grouped(steps, n, groups, device[0].data_ptr(), device[1].data_ptr(),
                                           device[2].data_ptr(), device[3].data_ptr() if bootstrap else None,
                                           device[4].data_ptr(), table.data_ptr(), advantages.data_ptr(),
                                           returns.data_ptr(), stream)
            torch.cuda.synchronize()
            what = f"T={steps} n={n} G={groups} bootstrap={bootstrap}"
            for name, got, expected, slab in zip(("advantages", "returns"), (advantages, returns), want, whole):
                assert bits(got.cpu().numpy()) == bits(expected), f"{what}: {name} differ"
                assert rc._untouched(slab[0]) and rc._untouched(slab[steps + 1]), f"{what}: a guard row was written"
            if groups == 1:
                _, (plain_a, plain_r) = rc._guarded(torch, steps, n)
                ctx.rollout_advantages(steps, n, device[0].data_ptr(), device[1].data_ptr(), device[2].data_ptr(),
                                       device[3].data_ptr() if bootstrap else None, device[4].data_ptr(), gammas[0],
                                       lambdas[0], plain_a.data_ptr(), plain_r.data_ptr(), stream)
                torch.cuda.synchronize()
                assert torch.equal(plain_a.view(torch.int32), advantages.view(torch.int32)), what
                assert torch.equal(plain_r.view(torch.int32), returns.view(torch.int32)), what


def refusal_case(torch, cases, ctx):
    """Each refusal comes before anything is enqueued: the outputs and the view stay what they were."""
    from reinfocus_amd import _native
    from reinfocus_amd.environments import harness, rollout
    from tests import rollout_io_cases as rc

    steps, n, groups = 5, 64, 8
    arrays = gae_inputs(steps, n, 5)
    rewards, values, truncated, final_values, last_values = _gae_device(torch, arrays)
    table = torch.from_numpy(rollout.discount_table(gammas_of(groups), lambdas_of(groups))).cuda()
    whole, (advantages, returns) = rc._guarded(torch, steps, n)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**changed):
        a = dict(steps=steps, n=n, groups=groups, rewards=rewards.data_ptr(), values=values.data_ptr(),
                 truncated=truncated.data_ptr(), final=final_values.data_ptr(), last=last_values.data_ptr(),
                 table=table.data_ptr(), advantages=advantages.data_ptr(), returns=returns.data_ptr())
        a.update(changed)
        ctx.rollout_advantages_grouped(a["steps"], a["n"], a["groups"], a["rewards"], a["values"], a["truncated"], a["final"],
                                       a["last"], a["table"], a["advantages"], a["returns"], stream)

    def refused(match, **changed):
        try:
            call(**changed)
        except AssertionError as caught:  # (RF_ERR_INVALID)
            assert match in str(caught), str(caught)
        else:
            raise AssertionError(f"not refused ({match})")
        torch.cuda.synchronize()
        assert all(rc._untouched(w) for w in whole), f"an output was written ({match})"

    refused("do not divide", groups=7)
    refused("outside 1 to", groups=0)
    refused("outside 1 to", groups=65536)
    refused("NULL argument", table=None)
    host_table = rollout.discount_table(gammas_of(groups), lambdas_of(groups))
    refused("d_discounts is not device memory", table=host_table.ctypes.data)
    refused("d_advantages overlaps d_values", advantages=values.data_ptr())
    refused("d_returns overlaps d_discounts", returns=table.data_ptr(), steps=1, n=groups // 4, groups=groups // 4)
    refused("d_advantages overlaps d_returns", advantages=returns.data_ptr())
    call()  # ... and the same arguments unchanged are taken
    torch.cuda.synchronize()
    want = rollout.gae_numpy_grouped(*arrays, gammas_of(groups), lambdas_of(groups))
    assert bits(advantages.cpu().numpy()) == bits(want[0]) and bits(returns.cpu().numpy()) == bits(want[1])

    # the view: a bad grouped configuration is refused and the context keeps the view it has; the ungrouped statistics
    # accessors are refused on a grouped context, the grouped ones on an ungrouped one
    lib = _native.load()
    case = dict(kind="composed-i32", n=65, groups=13, records=False, config={}, freeze=False)
    env = cases.make_env(case["kind"], case["n"], learner_view=make_view(case))
    plain = cases.make_env(case["kind"], case["n"], learner_view=harness.LearnerView(frame_stack=STACK))
    try:
        good = _native.EnvViewConfig(STACK, 1, 1, 1, 0.99, 1e-8, 10.0, 10.0)
        good_gammas = np.array(gammas_of(13), dtype=np.float64)
        gammas = good_gammas.ctypes.data
        bad_gammas = np.array([0.5] * 12 + [1.5], dtype=np.float64)
        before = env.view_statistics()
        for groups_, pointer, match in ((0, gammas, "outside 1 to"), (65536, gammas, "outside 1 to"),
                                        (7, gammas, "do not divide"), (13, bad_gammas.ctypes.data, "outside [0, 1]")):
            assert lib.rf_env_configure_view_grouped(env._ctx._h, good, groups_, pointer) == _native.RF_ERR_INVALID
            assert match in lib.rf_last_error().decode(), lib.rf_last_error().decode()
        assert lib.rf_env_configure_view_grouped(env._ctx._h, None, 13, gammas) == _native.RF_ERR_INVALID
        after = env.view_statistics()
        assert all(bits(before[key]) == bits(after[key]) and after[key].shape == (13, WIDTH + 1) for key in before)
        for call_, match in ((env._ctx.env_view_statistics, "is grouped"),
                             (lambda: env._ctx.env_view_set_statistics(*[np.zeros(WIDTH + 1)] * 3), "is grouped"),
                             (plain._ctx.env_view_statistics_grouped, "is not grouped"),
                             (lambda: plain._ctx.env_view_set_statistics_grouped(*[np.zeros((1, WIDTH + 1))] * 3),
                              "is not grouped")):
            try:
                call_()
            except AssertionError as caught:
                assert match in str(caught), str(caught)
            else:
                raise AssertionError(f"not refused ({match})")
        assert all(bits(before[key]) == bits(env.view_statistics()[key]) for key in before)
        for bad_group in (-1, 13):
            try:
                env.view_statistics(group=bad_group)
            except ValueError as caught:
                assert "group" in str(caught)
            else:
                raise AssertionError("a group outside the view's was taken")
        try:
            plain.view_statistics(group=0)
        except ValueError as caught:
            assert "groups=" in str(caught)
        else:
            raise AssertionError("group= on an ungrouped view was taken")
        # the environment still resets and steps
        drive_view(case, env, lambda: _reset_numpy(env), lambda index, actions: _numpy_step(
            torch, env.step_tensors(torch.from_numpy(actions).cuda())), None)
    finally:
        env.close()
        plain.close()
    # a view whose groups do not divide the lanes never reaches the library
    try:
        cases.make_env("composed-i32", 65, learner_view=harness.LearnerView(frame_stack=STACK, groups=8))
    except ValueError as caught:
        assert "do not divide" in str(caught)
    else:
        raise AssertionError("8 groups over 65 lanes were taken")


def _reset_numpy(env):
    obs, info = env.reset_tensors()
    return obs.cpu().numpy(), {key: value.cpu().numpy() for key, value in info.items()}


def snapshot_case(torch, cases):
    """Snapshot, step, restore, step again on a grouped view: byte-equal to the uninterrupted run; and a blob of an
    ungrouped view, of other gammas or of other groups is refused with nothing changed, in either direction."""
    from reinfocus_amd.environments import harness

    n, kind, half = 65, "composed-i64", 4
    views = {"grouped": lambda: harness.LearnerView(frame_stack=STACK, gamma=gammas_of(13), groups=13),
             "other gammas": lambda: harness.LearnerView(frame_stack=STACK, gamma=gammas_of(13)[::-1], groups=13),
             "other groups": lambda: harness.LearnerView(frame_stack=STACK, gamma=gammas_of(5), groups=5),
             "one group": lambda: harness.LearnerView(frame_stack=STACK, gamma=[0.99], groups=1),
             "ungrouped": lambda: harness.LearnerView(frame_stack=STACK, gamma=0.99)}
    envs = {name: cases.make_env(kind, n, episode_records=True, learner_view=view()) for name, view in views.items()}
    try:
        rng = np.random.default_rng(6)
        actions = [rng.integers(0, 13, n) for _ in range(2 * half)]

        def seen(env):
            return [bits(x) for x in env.view_state()] + [bits(x) for x in env.view_statistics().values()]

        for env in envs.values():
            env.set_view_statistics({key: value[0] if env._learner_view.groups is None else value
                                     for key, value in statistics_of(env._learner_view.groups or 1).items()})
            env.reset()
            for action in actions[:half]:
                env.step(action)
        env = envs["grouped"]
        snap, at_snapshot = env.snapshot(), seen(env)
        straight = []
        for action in actions[half:]:
            straight.append(_numpy_step(torch, env.step(action)) + (seen(env),))
        assert seen(env) != at_snapshot
        env.restore(snap)
        assert seen(env) == at_snapshot
        for index, (action, want) in enumerate(zip(actions[half:], straight)):
            got = _numpy_step(torch, env.step(action)) + (seen(env),)
            assert [bits(x) for x in got[:4]] == [bits(x) for x in want[:4]], f"step {index} after the restore differs"
            assert sorted(got[4]) == sorted(want[4]) and all(bits(got[4][k]) == bits(want[4][k]) for k in got[4])
            assert got[5] == want[5], f"step {index} after the restore: the view differs"
        # the ungrouped blob is what it was: array 23 is 3 x 17 float64, the grouped one holds 13 of them
        aligned = lambda nbytes: (nbytes + 255) & ~255  # noqa: E731
        sizes = {name: e.snapshot().blob.size for name, e in envs.items()}
        assert sizes["grouped"] - sizes["ungrouped"] == aligned(13 * 3 * 17 * 8) - aligned(3 * 17 * 8)
        assert sizes["one group"] == sizes["ungrouped"]
        snaps = {name: e.snapshot() for name, e in envs.items()}
        for name, target in envs.items():
            for other in envs:
                if other == name:
                    continue
                before = seen(target)
                try:
                    target.restore(snaps[other])
                except AssertionError as caught:
                    assert "learner view" in str(caught), str(caught)
                else:
                    raise AssertionError(f"a blob of {other!r} was taken by {name!r}")
                assert seen(target) == before
                assert np.array_equal(target.snapshot().blob, snaps[name].blob)
    finally:
        for env in envs.values():
            env.close()


def e2e_env(device_form, view=True):
    from reinfocus_amd.environments import harness
    from tests import rollout_io_cases as rc

    n = E2E["groups"] * E2E["per_group"]
    extra = dict(episode_records=True, learner_view=harness.LearnerView(
        frame_stack=1, gamma=E2E_VIEW_GAMMAS, groups=E2E["groups"]) if view else None)
    if device_form:
        return harness.DeviceVectorDiscreteSteps(num_envs=n, device_initializer=True, **rc.ENV_KW, **extra)
    return harness.VectorDiscreteSteps(num_envs=n, **rc.ENV_KW, **extra)


def e2e_spec():
    """The least network of tests/population_io_cases.NETWORKS -- its hidden layers and activation -- at the
    environment's widths: 4 observation columns, 13 actions."""
    from reinfocus_amd.environments import policy
    from tests import population_io_cases as pop

    _, pi, vf, _, activation = pop.NETWORKS[0]
    return policy.MlpPolicySpec(WIDTH, 13, pi=pi, vf=vf, activation=activation)


def e2e_permutations(iteration):
    rows = E2E["steps"] * E2E["per_group"]
    rng = np.random.default_rng(800 + iteration)
    return np.stack([np.stack([rng.permutation(rows) for _ in range(E2E["groups"])])
                     for _ in range(E2E["epochs"])]).astype(np.int64)


def e2e_runs(env, rollout, policy, learner, reset, unwrap, wrap):
    from tests import policy_io_cases

    obs = reset()
    seen = []
    for iteration in range(E2E["iterations"]):
        rollout.start(obs if iteration == 0 else None)
        rollout.collect(policy)
        record = policy_io_cases.slabs_of(rollout, unwrap)
        record["stats"] = unwrap(learner.train(rollout, E2E["epochs"], E2E["batch"],
                                               permutations=wrap(e2e_permutations(iteration))))
        record["params"] = unwrap(policy.params)
        for key, value in env.view_statistics().items():
            record["view/" + key] = value
        seen.append(record)
    return seen


def e2e_twin_runs():
    from reinfocus_amd.environments import harness
    from tests import population_io_cases as pop

    env = e2e_env(False)
    try:
        spec = e2e_spec()
        policy = harness.PopulationPolicy(spec, E2E["groups"], pop.seeds_of(E2E["groups"]))
        learner = harness.PopulationLearner(policy, learning_rate=[1e-2, 3e-3, 1e-3, 0.0], ent_coef=0.01)
        rollout = harness.Rollout(env, E2E["steps"], E2E_GAMMAS, E2E_LAMBDAS, groups=E2E["groups"])
        return e2e_runs(env, rollout, policy, learner, lambda: env.reset()[0], np.array, lambda a: a)
    finally:
        env.close()


def end_to_end_case(torch):
    """A population of four learners over a grouped view through a grouped DeviceRollout: two iterations of collect()
    + train() equal the numpy twins in parameters, stats, advantages and view statistics."""
    from reinfocus_amd.environments import harness
    from tests import policy_io_cases
    from tests import population_io_cases as pop

    want = e2e_twin_runs()
    env = e2e_env(True)
    try:
        spec = e2e_spec()
        policy = harness.DevicePopulationPolicy(env, spec, E2E["groups"], pop.seeds_of(E2E["groups"]))
        learner = harness.DevicePopulationLearner(policy, learning_rate=[1e-2, 3e-3, 1e-3, 0.0], ent_coef=0.01)
        rollout = harness.DeviceRollout(env, E2E["steps"], E2E_GAMMAS, E2E_LAMBDAS, groups=E2E["groups"])
        got = e2e_runs(env, rollout, policy, learner, lambda: env.reset_tensors()[0], lambda t: t.cpu().numpy(),
                       lambda a: torch.from_numpy(a).cuda())
        policy_io_cases.same_runs(got, want)
        assert env.device_fault() is None
        assert np.concatenate([run["truncated"] for run in want]).any(), "no environment ended"
        assert bits(want[0]["params"][0]) != bits(want[1]["params"][0])
        assert len({bits(row) for row in want[1]["view/mean"]}) == E2E["groups"]  # (each group has its own normaliser)
        # the table follows the attributes: new discounts, one more finish(), the twin's bytes
        rollout.gamma, rollout.gae_lambda = 0.5, (0.0, 1.0, 0.5, 0.25)
        from reinfocus_amd.environments import rollout as rollout_module

        last = torch.zeros(env.num_envs, dtype=torch.float32, device="cuda")
        again = rollout.finish(last)
        expected = rollout_module.gae_numpy_grouped(got[1]["rewards"], got[1]["values"], got[1]["truncated"],
                                                    got[1]["final_values"], np.zeros(env.num_envs, dtype=np.float32),
                                                    (0.5,) * 4, (0.0, 1.0, 0.5, 0.25))
        assert bits(again[0].cpu().numpy()) == bits(expected[0]) and bits(again[1].cpu().numpy()) == bits(expected[1])
        # what the classes refuse
        for make, match in ((lambda: harness.DeviceRollout(env, 4, (0.9, 0.8), 0.95), "groups="),
                            (lambda: harness.DeviceRollout(env, 4, 0.9, 0.95, groups=8), "learner view has"),
                            (lambda: harness.DeviceRollout(env, 4, (0.9, 0.8), 0.95, groups=4), "one per group")):
            try:
                make()
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
    for case in VIEW_CASES:
        with record.case(case_id(case)):
            view_case(torch, cases, case)
    with record.case("one group"):
        one_group_case(torch, cases)
    for steps in GAE_STEPS:
        with record.case(f"gae/{steps}"):
            gae_case(torch, ctx, steps)
    with record.case("refusals"):
        refusal_case(torch, cases, ctx)
    with record.case("snapshots"):
        snapshot_case(torch, cases)
    with record.case("end to end"):
        end_to_end_case(torch)
    with record.case("finished"):
        pass
    ctx.close()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    run_cases(sys.argv[1])
