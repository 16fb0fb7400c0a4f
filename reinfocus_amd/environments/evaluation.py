"""Evaluation scores per group, on the device, with the best parameters kept.

What the reference's hyper-parameter search optimises is each trial's evaluation score: stable-baselines3's
evaluate_policy on a separate evaluation environment (rl_zoo3's TrialEvalCallback / SB3's EvalCallback) -- deterministic
actions, a VecNormalize that is frozen and synced from the training environment, raw rewards, a fixed number of episodes
per trial --, and the best model so far is kept.  Evaluation / DeviceEvaluation are that measurement for the G groups of a
population (G = 1 for the ungrouped policy classes), all groups in the same launches:

    evaluation = harness.DeviceEvaluation(eval_env, policy, n_eval_episodes=5, train_env=env)
    rows = evaluation.run(max_steps)          # float64 [G][8] on the device; nothing waited for
    evaluation.results()                      # the host copy (synchronises)
    evaluation.load_best(groups=mask)         # best_params -> policy.params for the selected groups

One definition (include/reinfocus_hip.h, "evaluation"): the lane with local index i of a group keeps its first
(E + i) // m episodes (SB3's episode_count_targets) in slots of its own; the kept values have fixed positions, lane-major
and slot-minor; mean, standard deviation and mean length are the learner view's treesum over those positions; a group that
has not reached its targets is flagged; a complete group whose mean is strictly above its best so far improves.  The
functions below are the numpy restatement and the oracle; eval_accumulate_kernel, eval_finish_kernel and
eval_keep_rows_kernel (csrc/rf_eval.h) compute the same bits.

Deliberate differences from SB3: the positional order and the float64 tree in place of numpy.mean over the
list in order of time (the same set of episodes, summed in another order), and a fixed max_steps in place of looping until
every lane is done (an early exit would need a host read per step).
"""

import numpy as np

MAX_EPISODES = 65536  # RF_EVAL_MAX_EPISODES
INCOMPLETE = 1  # RF_EVAL_INCOMPLETE
MEAN, STD, MINIMUM, MAXIMUM, MEAN_LENGTH, KEPT, FLAGS, SERIAL = range(8)  # the columns of a row


def targets(m, episodes):
    """SB3's episode_count_targets of one group: int32 [m], (E + i) // m; they sum to E."""
    return np.array([(episodes + i) // m for i in range(m)], dtype=np.int32)


def slots(m, episodes):
    """K = ceil(E / m), the slot count per lane."""
    return (episodes + m - 1) // m


def tables(n, m, episodes):
    """(counts int32 [n], returns float64 [n][K], lengths int32 [n][K]), zeroed."""
    K = slots(m, episodes)
    return np.zeros(n, dtype=np.int32), np.zeros((n, K), dtype=np.float64), np.zeros((n, K), dtype=np.int32)


def accumulate_numpy(counts, returns, lengths, final_return, final_length, m, episodes):
    """E2 of "evaluation", in place: the records of one step into the tables."""
    want = np.tile(targets(m, episodes), counts.shape[0] // m)
    for lane in np.flatnonzero((np.asarray(final_length) > 0) & (counts < want)):
        returns[lane, counts[lane]] = final_return[lane]
        lengths[lane, counts[lane]] = final_length[lane]
        counts[lane] += 1


def total_order_key(x):
    """int64 keys under which the non-NaN float64 are totally ordered, -0.0 below +0.0."""
    bits = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return np.where(bits < 0, bits ^ np.int64(2 ** 63 - 1), bits)


def kept_values(counts, returns, lengths, m, episodes, group):
    """(returns float64 [E], lengths int32 [E]) of a complete group in their positions (E3): lane-major, slot-minor."""
    lanes = slice(group * m, (group + 1) * m)
    want = targets(m, episodes)
    assert (counts[lanes] == want).all()
    return (np.concatenate([returns[group * m + i, :want[i]] for i in range(m)]),
            np.concatenate([lengths[group * m + i, :want[i]] for i in range(m)]))


def _canonical(value):
    return np.float64(np.nan) if np.isnan(value) else np.float64(value)


def finish_numpy(counts, returns, lengths, groups, m, episodes, serial, best_mean, best_serial):
    """E3 .. E6 of "evaluation": (results float64 [G][8], improved uint8 [G]); best_mean float64 [G] and best_serial int64
    [G] are updated in place."""
    from reinfocus_amd.environments import harness

    results = np.zeros((groups, 8), dtype=np.float64)
    improved = np.zeros(groups, dtype=np.uint8)
    N = np.float64(episodes)
    with np.errstate(all="ignore"):
        for g in range(groups):
            kept = int(np.maximum(counts[g * m:(g + 1) * m], 0).sum())
            results[g, KEPT], results[g, SERIAL] = kept, serial
            if kept != episodes:
                results[g, :KEPT] = np.nan
                results[g, FLAGS] = INCOMPLETE
                continue
            x, steps = kept_values(counts, returns, lengths, m, episodes, g)
            mean = harness.treesum(x) / N
            d = x - mean
            std = np.sqrt(harness.treesum(d * d) / N)
            results[g, MEAN], results[g, STD] = _canonical(mean), _canonical(std)
            if np.isnan(x).any():
                results[g, MINIMUM] = results[g, MAXIMUM] = np.nan
            else:
                keys = total_order_key(x)
                results[g, MINIMUM], results[g, MAXIMUM] = x[np.argmin(keys)], x[np.argmax(keys)]
            results[g, MEAN_LENGTH] = harness.treesum(steps.astype(np.float64)) / N
            if mean > best_mean[g]:  # (strict; False for NaN)
                best_mean[g], best_serial[g], improved[g] = mean, serial, 1
    return results, improved


def keep_rows_numpy(select, source, target):
    """rf_eval_keep_rows: target[g] = source[g] where select[g], in place."""
    for g in np.flatnonzero(np.asarray(select)):
        target[g] = source[g]


def _checked_episodes(n_eval_episodes):
    if isinstance(n_eval_episodes, (bool, np.bool_)) or int(n_eval_episodes) != n_eval_episodes:
        raise ValueError(f"n_eval_episodes {n_eval_episodes!r} is not an integer")
    if n_eval_episodes < 1:
        raise ValueError(f"n_eval_episodes {n_eval_episodes!r}: at least 1 episode per group")
    if n_eval_episodes > MAX_EPISODES:
        raise ValueError(f"n_eval_episodes {n_eval_episodes!r}: at most {MAX_EPISODES} episodes per group (RF_EVAL_MAX_EPISODES)")
    return int(n_eval_episodes)


class _Plan:
    """What both classes check and keep: the head (spec.kind, as collect() dispatches), G, m, E, K and the serial."""

    def _plan(self, eval_env, policy, n_eval_episodes, train_env, has_records, view_of):
        self.episodes = _checked_episodes(n_eval_episodes)
        kind = getattr(getattr(policy, "spec", None), "kind", None)
        if kind not in ("categorical", "sde", "lstm", "lstm_sde"):
            raise TypeError(f"an evaluation needs one of the policy classes of this package, not {type(policy).__name__}")
        self.env, self.policy, self.spec, self.train_env = eval_env, policy, policy.spec, train_env
        self._sde, self._lstm = kind in ("sde", "lstm_sde"), kind in ("lstm", "lstm_sde")
        if not has_records(eval_env):
            raise ValueError(f"the evaluation environment {type(eval_env).__name__} keeps no episode records: build it with "
                             "episode_records=True (the raw episode returns and lengths are what an evaluation reads)")
        self.num_envs = n = int(eval_env.num_envs)
        population = getattr(policy, "groups", None)
        self.groups = 1 if population is None else int(population)
        own = getattr(policy, "num_envs", None)
        if own is not None and hasattr(policy, "_io") and int(own) != n:  # (a twin's num_envs only sizes its noise)
            raise ValueError(f"the evaluation environment has {n} environments, the policy {own}: an evaluation runs as many "
                             "lanes as the policy trains with")
        if train_env is not None and int(train_env.num_envs) != n:
            raise ValueError(f"the evaluation environment has {n} environments, the training environment "
                             f"{train_env.num_envs}")
        if n % self.groups != 0:
            raise ValueError(f"{n} environments are not divisible into the policy's {self.groups} groups")
        self.per_group = n // self.groups
        width = int(eval_env.single_observation_space.shape[0])
        if width != self.spec.obs_width:
            raise ValueError(f"the evaluation environment's observations have width {width}, the policy's "
                             f"{self.spec.obs_width}")
        discrete = hasattr(eval_env.single_action_space, "n")
        if discrete == self._sde:
            raise ValueError(f"the evaluation environment's action space is {eval_env.single_action_space!r}, which is not "
                             f"what the policy's {'Gaussian' if self._sde else 'Categorical'} head acts in")
        if discrete and int(eval_env.single_action_space.n) != self.spec.n_actions:
            raise ValueError(f"the evaluation environment has {eval_env.single_action_space.n} actions, the policy "
                             f"{self.spec.n_actions}")
        view = view_of(eval_env)
        if view is not None and (view.groups or 1) != self.groups:
            raise ValueError(f"the evaluation environment's learner view has groups={view.groups}, the policy "
                             f"{self.groups} groups")
        train_view = None if train_env is None else view_of(train_env)
        self._sync = view is not None and train_view is not None
        if self._sync and (view.groups != train_view.groups
                           or train_env.single_observation_space.shape != eval_env.single_observation_space.shape):
            raise ValueError("the learner views of the training and the evaluation environment differ in groups or width: "
                             "their statistics cannot be copied")
        self._viewed = view is not None
        if self._viewed:
            eval_env.set_view_training(False)
        self.slots = slots(self.per_group, self.episodes)
        self.serial = 0

    @staticmethod
    def _checked_run(max_steps, deterministic):
        if isinstance(max_steps, (bool, np.bool_)) or int(max_steps) != max_steps or max_steps < 1:
            raise ValueError(f"max_steps {max_steps!r} is not an integer of at least 1")
        if not deterministic:
            raise ValueError("deterministic=False is refused for now: a sampled evaluation would consume the draws of the "
                             "training generators")
        return int(max_steps)


class Evaluation(_Plan):
    """The numpy twin of DeviceEvaluation and its oracle, over the twin environments and the twin policies."""

    def __init__(self, eval_env, policy, n_eval_episodes=5, train_env=None):
        self._plan(eval_env, policy, n_eval_episodes, train_env, lambda env: getattr(env, "_records", None) is not None,
                   lambda env: None if getattr(env, "_view", None) is None else env._view.config)
        G = self.groups
        self.counts, self.returns, self.lengths = tables(self.num_envs, self.per_group, self.episodes)
        self._results = np.zeros((G, 8), dtype=np.float64)
        self.improved = np.zeros(G, dtype=np.uint8)
        self.best_mean = np.full(G, -np.inf, dtype=np.float64)
        self.best_serial = np.zeros(G, dtype=np.int64)
        self.best_params = np.array(self.policy.params, dtype=np.float32).reshape(G, -1)
        self.best_statistics = eval_env.view_statistics_tensor() if self._viewed else None

    def _rows(self):
        """policy.params as [G][P] (a view)."""
        return self.policy.params.reshape(self.groups, -1)

    def run(self, max_steps, deterministic=True):
        max_steps = self._checked_run(max_steps, deterministic)
        env, policy, n = self.env, self.policy, self.num_envs
        if self._sync:
            env.set_view_statistics_tensor(self.train_env.view_statistics_tensor())
        obs, _ = env.reset()
        self.counts[:] = 0
        if self._lstm:
            state = np.zeros(self.spec.state_shape(n), dtype=np.float32)
            starts = np.ones(n, dtype=np.uint8)
        for _ in range(max_steps):
            if self._lstm:
                acted = policy.act(obs, starts, None, True, states=(state, state))
            else:
                acted = policy.act(obs, None, True)
            obs, _, terminated, truncated, info = env.step(acted[4] if self._sde else acted[0])
            accumulate_numpy(self.counts, self.returns, self.lengths, info["episode_return"], info["episode_length"],
                             self.per_group, self.episodes)
            if self._lstm:
                starts = (np.asarray(terminated) | np.asarray(truncated)).astype(np.uint8)
        self.serial += 1
        self._results, self.improved = finish_numpy(self.counts, self.returns, self.lengths, self.groups, self.per_group,
                                                    self.episodes, self.serial, self.best_mean, self.best_serial)
        keep_rows_numpy(self.improved, self._rows(), self.best_params)
        if self._viewed:
            statistics = env.view_statistics_tensor().reshape(self.groups, -1)
            keep_rows_numpy(self.improved, statistics, self.best_statistics.reshape(self.groups, -1))
        return self._results

    def results(self):
        return self._results.copy()

    def load_best(self, groups=None):
        """best_params -> policy.params for every group, or for those of a boolean mask."""
        from reinfocus_amd.environments import population

        keep_rows_numpy(population.group_mask(groups, self.groups), self.best_params, self._rows())

    def state_dict(self):
        state = {"best_params": self.best_params.copy(), "best_mean": self.best_mean.copy(),
                 "best_serial": self.best_serial.copy(), "results": self._results.copy(), "serial": self.serial}
        if self._viewed:
            state["best_statistics"] = self.best_statistics.copy()
        return state

    def load_state_dict(self, state):
        for name in ("best_params", "best_mean", "best_serial") + (("best_statistics",) if self._viewed else ()):
            own = getattr(self, name)
            value = np.asarray(state[name], dtype=own.dtype)
            if value.shape != own.shape:
                raise ValueError(f"{name} has shape {value.shape}, not {own.shape}")
            own[...] = value
        self._results = np.array(state["results"], dtype=np.float64).reshape(self.groups, 8)
        self.serial = int(state["serial"])


class DeviceEvaluation(_Plan):
    """evaluate_policy for the G groups of a device policy -- DevicePolicy, DeviceSdePolicy, DeviceLstmPolicy,
    DeviceLstmSdePolicy (G = 1) and the four DevicePopulation* classes -- over a device-resident evaluation environment
    of the same n = G m lanes, built with episode_records=True (and, where the policy trains on a learner view, with a
    learner view of the same groups whose training flag is off: the constructor calls set_view_training(False)).

    run(max_steps) enqueues, on torch's current stream: the statistics train_env -> eval_env (both with a view), a reset,
    max_steps times a deterministic act() into tensors of the evaluation's own -- recurrent heads from a fresh zero state of
    the evaluation's own, through states= --, step_tensors() and rf_eval_accumulate, then rf_eval_finish and
    rf_eval_keep_rows for the parameters and the statistics.  A deterministic act() draws nothing, so the policy's
    generators, its noise and its LSTM state are what they were; nothing synchronises the host.  max_steps is the caller's
    bound, ceil(E / m) times the task's longest episode: a group that is not done by then is flagged, not waited for.

    best_params float32 [G][P] starts as a copy of policy.params, best_statistics float64 [G][3][W + 1] as a copy of the
    evaluation environment's, best_mean at -inf, best_serial at 0; the first run has serial 1."""

    def __init__(self, eval_env, policy, n_eval_episodes=5, train_env=None):
        from reinfocus_amd.environments import harness

        for env, what in ((eval_env, "evaluation"),) + (() if train_env is None else ((train_env, "training"),)):
            if not isinstance(env, harness._DeviceVectorEnv):
                if hasattr(env, "_no_tensors"):  # (a sharded environment: its own refusal says why)
                    env._no_tensors()
                raise TypeError(f"DeviceEvaluation needs a device-resident {what} environment, not {type(env).__name__} "
                                "(the numpy twins have Evaluation)")
        if not hasattr(policy, "_io") or not hasattr(policy, "device"):
            raise TypeError(f"DeviceEvaluation needs a device policy, not {type(policy).__name__} (the numpy twins have "
                            "Evaluation)")
        if eval_env._ctx.device != policy.device.index:
            raise ValueError(f"the evaluation environment runs on cuda:{eval_env._ctx.device}, the policy on {policy.device}: "
                             "an evaluation reads and writes device memory of one GPU only")
        self._io = eval_env._tensor_io()  # (ValueError, as step_tensors': a host-drawn initializer, a render_mode)
        self._plan(eval_env, policy, n_eval_episodes, train_env, lambda env: bool(env._episode_records),
                   lambda env: env._learner_view)
        torch = self._torch = policy._torch
        self._ctx = eval_env._ctx
        device, n, G, K = policy.device, self.num_envs, self.groups, self.slots
        self.device = device
        self.counts = torch.zeros(n, dtype=torch.int32, device=device)
        self.returns = torch.zeros((n, K), dtype=torch.float64, device=device)
        self.lengths = torch.zeros((n, K), dtype=torch.int32, device=device)
        self._results = torch.zeros((G, 8), dtype=torch.float64, device=device)
        self.improved = torch.zeros(G, dtype=torch.uint8, device=device)
        self.best_mean = torch.full((G,), float("-inf"), dtype=torch.float64, device=device)
        self.best_serial = torch.zeros(G, dtype=torch.int64, device=device)
        self.best_params = policy.params.detach().clone().reshape(G, -1)
        self._statistics = self.best_statistics = None
        if self._viewed:
            self._statistics = eval_env.view_statistics_tensor()
            self.best_statistics = self._statistics.clone()
        self._select = torch.zeros(G, dtype=torch.uint8, device=device)
        self._ones = torch.ones(n, dtype=torch.uint8, device=device)
        self._state = torch.zeros(self.spec.state_shape(n), dtype=torch.float32, device=device) if self._lstm else None
        actions = torch.zeros(n, dtype=torch.float32 if self._sde else torch.int64, device=device)
        rows = [torch.zeros(n, dtype=torch.float32, device=device) for _ in range(3)]
        # out= of act(): (actions, values, log_probs, no final_values[, env_actions])
        self._out = (actions, rows[0], rows[1], None) + ((rows[2],) if self._sde else ())

    def _rows(self):
        """policy.params as [G][P] (a view)."""
        return self.policy.params.view(self.groups, -1)

    def _keep(self, select, source, target):
        words = source.shape[1] * source.element_size() // 4
        self._ctx.eval_keep_rows(self.groups, words, words, select.data_ptr(), source.data_ptr(), target.data_ptr(),
                                 self._io._stream())

    def run(self, max_steps, deterministic=True):
        """One evaluation: the float64 [G][8] rows (a tensor the evaluation owns and the next run overwrites)."""
        max_steps = self._checked_run(max_steps, deterministic)
        env, policy, n = self.env, self.policy, self.num_envs
        if self._sync:
            env.set_view_statistics_tensor(self.train_env.view_statistics_tensor(out=self._statistics))
        obs, _ = env.reset_tensors()
        self.counts.zero_()
        starts = self._ones
        if self._lstm:
            self._state.zero_()
        for _ in range(max_steps):
            if self._lstm:
                policy.act(obs, starts, None, True, out=self._out, states=(self._state, self._state))
            else:
                policy.act(obs, None, True, out=self._out)
            obs, _, _, truncated, info = env.step_tensors(self._out[4] if self._sde else self._out[0])
            self._ctx.eval_accumulate(n, self.groups, self.per_group, self.episodes, info["episode_return"].data_ptr(),
                                      info["episode_length"].data_ptr(), self.counts.data_ptr(), self.returns.data_ptr(),
                                      self.lengths.data_ptr(), self._io._stream())
            starts = truncated
        self.serial += 1
        self._ctx.eval_finish(n, self.groups, self.per_group, self.episodes, self.serial, self.counts.data_ptr(),
                              self.returns.data_ptr(), self.lengths.data_ptr(), self._results.data_ptr(),
                              self.best_mean.data_ptr(), self.best_serial.data_ptr(), self.improved.data_ptr(),
                              self._io._stream())
        self._keep(self.improved, self._rows(), self.best_params)
        if self._viewed:
            env.view_statistics_tensor(out=self._statistics)
            self._keep(self.improved, self._statistics.view(self.groups, -1), self.best_statistics.view(self.groups, -1))
        return self._results

    def results(self):
        """The host copy of the last run's rows, float64 [G][8].  Synchronises."""
        return self._results.cpu().numpy()

    def load_best(self, groups=None):
        """best_params -> policy.params for every group, or for those of a boolean mask: one launch; the mask goes up
        from pinned memory, stream-ordered."""
        from reinfocus_amd.environments import population

        torch = self._torch
        mask = population.group_mask(groups, self.groups).astype(np.uint8)
        self._select.copy_(torch.from_numpy(mask).pin_memory(), non_blocking=True)
        self._keep(self._select, self.best_params, self._rows())

    def state_dict(self):
        """Device tensors (copies) and the serial."""
        state = {"best_params": self.best_params.clone(), "best_mean": self.best_mean.clone(),
                 "best_serial": self.best_serial.clone(), "results": self._results.clone(), "serial": self.serial}
        if self._viewed:
            state["best_statistics"] = self.best_statistics.clone()
        return state

    def load_state_dict(self, state):
        torch = self._torch
        names = ("best_params", "best_mean", "best_serial", "results") + (("best_statistics",) if self._viewed else ())
        for name in names:
            own = self._results if name == "results" else getattr(self, name)
            value = state[name]
            if not isinstance(value, torch.Tensor) or value.dtype != own.dtype or tuple(value.shape) != tuple(own.shape):
                raise ValueError(f"{name} must be a {own.dtype} tensor of shape {tuple(own.shape)}")
            self._io._on_device(value, name)
        for name in names:
            (self._results if name == "results" else getattr(self, name)).copy_(state[name])
        self.serial = int(state["serial"])
