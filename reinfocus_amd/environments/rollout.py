"""PPO's rollout buffer for the vector environments: n_steps steps of observations, actions, rewards, values and
log-probabilities, then GAE(gamma, lambda) advantages and returns -- stable-baselines3's RolloutBuffer
(compute_returns_and_advantage) with the truncation bootstrap of OnPolicyAlgorithm.collect_rollouts, which every
training configuration of the reference (examples/ppo_*.yml) runs behind VecNormalize and VecFrameStack.

Every episode of these environments ends by truncation, and the step resets the environment in the same call: so
episode_starts[t + 1] == truncated[t], dones == truncated[T - 1], and a truncated step needs
reward += gamma * V(final_observation).

One definition of the arithmetic (include/reinfocus_hip.h, "rollout"): gae_numpy below is its numpy float32
restatement and the oracle; rollout_gae_kernel (csrc/rf_rollout.h) computes the same bits in one launch.

    Rollout        over the numpy twins (VectorDiscreteSteps, VectorContinuousJumps, VectorEnvironment)
    DeviceRollout  over the device-resident environments, from and to torch tensors on the environment's GPU: the step
                   writes its results into the buffer's slabs (step_tensors(out=...)), finish() is one kernel launch,
                   and nothing waits for the host

collect(policy) runs a whole rollout with a policy of environments/policy.py (Policy for Rollout, DevicePolicy for
DeviceRollout) or, over a Box(-1, 1, (1,)) action space, of environments/sde.py (SdePolicy, DeviceSdePolicy: the raw
action goes into the slab, the clamped one to the step, and sde_sample_freq says when the noise is resampled): on the
device a step is then one policy launch, which writes rows of the slabs, and the environment's step from those rows.
With a recurrent policy of environments/lstm.py (LstmPolicy, DeviceLstmPolicy) or, over the Box space, of
environments/lstm_sde.py (LstmSdePolicy, DeviceLstmSdePolicy: both rules at once) collect() also keeps what sb3-contrib's
RecurrentRolloutBuffer hands to the update -- episode_starts uint8 [T + 1, n] and lstm_states float32
[T + 1, 2, 2, n, H], made on first use with such a policy --; flat() and minibatches() are unchanged.  The populations of
environments/population.py are taken the same way, by their spec's kind and their `groups`: one with a Gaussian head
(SdePopulationPolicy, LstmSdePopulationPolicy and their device classes) has sde_sample_freq as a scalar or G values and
one masked reset per step, a recurrent one (LstmPopulationPolicy, LstmSdePopulationPolicy) keeps the two slabs.

torch is imported lazily, by DeviceRollout only (reinfocus_amd/torch_interop.py says why import order matters).
"""

import numpy as np

from reinfocus_amd.environments import spaces

FLAT_KEYS = ("observations", "actions", "values", "log_probs", "advantages", "returns")


def gae_numpy(rewards, values, truncated, final_values, last_values, gamma, gae_lambda):
    """(advantages, returns), float32 [T, n], of rewards float64 [T, n], values float32 [T, n], truncated uint8 [T, n]
    (0 / 1), final_values float32 [T, n] or None (no bootstrap) and last_values float32 [n]; gamma and gae_lambda are
    Python floats.  The definition, literally: every operation is a numpy float32 operation, left to right."""
    f32 = np.float32
    rewards = np.asarray(rewards, dtype=np.float64)
    steps, num_envs = rewards.shape
    values = np.asarray(values, dtype=f32).reshape(steps, num_envs)
    truncated = np.asarray(truncated, dtype=np.uint8).reshape(steps, num_envs)
    last_values = np.asarray(last_values, dtype=f32).reshape(num_envs)
    g = f32(float(gamma))
    gl = f32(float(gamma) * float(gae_lambda))  # (the product in float64 first)
    advantages = np.empty((steps, num_envs), dtype=f32)
    with np.errstate(all="ignore"):
        r = rewards.astype(f32)
        if final_values is not None:
            final_values = np.asarray(final_values, dtype=f32).reshape(steps, num_envs)
            r = np.where(truncated != 0, r + g * final_values, r)  # a select, never a multiplication by 0 / 1
        nnt = f32(1.0) - truncated.astype(f32)
        last = np.zeros(num_envs, dtype=f32)
        for t in range(steps - 1, -1, -1):
            next_v = last_values if t == steps - 1 else values[t + 1]
            delta = (r[t] + (g * next_v) * nnt[t]) - values[t]
            last = delta + (gl * nnt[t]) * last
            advantages[t] = last
        returns = advantages + values
    assert advantages.dtype == f32 and returns.dtype == f32
    return advantages, returns


def gae_numpy_grouped(rewards, values, truncated, final_values, last_values, gammas, gae_lambdas):
    """gae_numpy with discounts per group (include/reinfocus_hip.h, "population view"): gammas and gae_lambdas hold G
    values each, the n columns are G groups of m = n / G consecutive ones, and group g's columns are gae_numpy's of that
    slice with gammas[g] and gae_lambdas[g] -- literally so."""
    rewards = np.asarray(rewards, dtype=np.float64)
    steps, num_envs = rewards.shape
    gammas, gae_lambdas = _per_group(gammas, len(gammas), "gamma"), _per_group(gae_lambdas, len(gammas), "gae_lambda")
    groups = len(gammas)
    if num_envs % groups != 0:
        raise ValueError(f"{groups} groups do not divide {num_envs} environments")
    m = num_envs // groups
    values = np.asarray(values, dtype=np.float32).reshape(steps, num_envs)
    truncated = np.asarray(truncated, dtype=np.uint8).reshape(steps, num_envs)
    last_values = np.asarray(last_values, dtype=np.float32).reshape(num_envs)
    if final_values is not None:
        final_values = np.asarray(final_values, dtype=np.float32).reshape(steps, num_envs)
    advantages = np.empty((steps, num_envs), dtype=np.float32)
    returns = np.empty((steps, num_envs), dtype=np.float32)
    for g in range(groups):
        lanes = slice(g * m, (g + 1) * m)
        advantages[:, lanes], returns[:, lanes] = gae_numpy(
            rewards[:, lanes], values[:, lanes], truncated[:, lanes],
            None if final_values is None else final_values[:, lanes], last_values[lanes], gammas[g], gae_lambdas[g])
    return advantages, returns


def _per_group(value, groups, name):
    """`value` as a tuple of `groups` Python floats: a scalar for all groups, or one value per group."""
    values = np.asarray(value, dtype=np.float64)
    if values.ndim == 0:
        values = np.full(groups, float(values))
    if values.shape != (groups,):
        raise ValueError(f"{name} has shape {values.shape}: a scalar or {groups} values, one per group")
    return tuple(float(x) for x in values)


def discount_table(gammas, gae_lambdas):
    """float32 [G, 2]: (g, gl) per group as rf_rollout_advantages_grouped reads them -- g = float32(gamma),
    gl = float32(gamma * gae_lambda) with the product taken in float64."""
    return np.array([(np.float32(gamma), np.float32(gamma * gae_lambda)) for gamma, gae_lambda in zip(gammas, gae_lambdas)],
                    dtype=np.float32).reshape(len(gammas), 2)


def _index_task(env):
    return isinstance(env.single_action_space, spaces.Discrete)


class _Bookkeeping:
    """What both forms count on the host (plain Python integers: nothing is asked of the device): the step within the
    rollout, how many of its steps were bootstrapped, and whether a rollout is open."""

    def _configure(self, env, n_steps, gamma, gae_lambda, records, groups=None):
        self.env = env
        self.n_steps = int(n_steps)
        self.groups = None if groups is None else int(groups)
        self.num_envs = int(env.num_envs)
        if self.groups is None:
            if np.ndim(gamma) != 0 or np.ndim(gae_lambda) != 0:
                raise ValueError("gamma and gae_lambda are scalars without groups= (one value per group needs groups=G)")
            self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        else:
            # gamma and gae_lambda: scalars or G values; plain attributes, read again by every finish()
            if self.groups != groups or self.groups < 1:
                raise ValueError(f"groups {groups!r} is not a positive integer")
            if self.num_envs % self.groups != 0:
                raise ValueError(f"{self.groups} groups do not divide the environment's {self.num_envs} lanes")
            view = getattr(env, "_learner_view", None) or getattr(getattr(env, "_view", None), "config", None)
            view_groups = getattr(view, "groups", None)
            if view_groups is not None and view_groups != self.groups:
                raise ValueError(f"the rollout has groups={self.groups}, and the environment's learner view has "
                                 f"groups={view_groups}: group g owns the same lanes in both")
            self.gamma, self.gae_lambda = gamma, gae_lambda
            self._discounts()
        if self.n_steps < 1:
            raise ValueError(f"n_steps {n_steps!r} is not at least 1")
        self.obs_width = int(env.single_observation_space.shape[0])
        self._records = bool(records)
        self._t = None  # (None: no rollout is open)
        self._bootstrapped = 0
        self._last_bootstrap = -1
        self._complete = False  # (row T holds the observation the next rollout begins with)
        self._fresh = self._lstm = False
        self._sde_freqs = None  # (collect() with a population of gSDE learners: sde_sample_freq per group)
        # what collect() keeps of a recurrent policy (environments/lstm.py), made on first use with one: episode_starts
        # uint8 [T + 1, n] and lstm_states float32 [T + 1, 2, 2, n, H] -- what sb3-contrib's RecurrentRolloutBuffer hands
        # to the update.  A rollout that never sees such a policy allocates neither.
        self.episode_starts = self.lstm_states = None

    def _discounts(self):
        """(gammas, gae_lambdas) of a grouped rollout as tuples of G floats, from the attributes as they are now."""
        return (_per_group(self.gamma, self.groups, "gamma"), _per_group(self.gae_lambda, self.groups, "gae_lambda"))

    def _begin(self, obs):
        if obs is None and not self._complete:
            raise ValueError("start() without obs continues the rollout before it, and none has been finished: pass the "
                             "observation the environment's reset returned")
        self._t, self._bootstrapped, self._last_bootstrap = 0, 0, -1
        self._fresh = obs is not None  # (every environment starts an episode: row 0 of an lstm policy's episode_starts)

    def _next_step(self):
        if self._t is None:
            raise ValueError("no rollout is open: start() first")
        if self._t >= self.n_steps:
            raise ValueError(f"the rollout already holds its {self.n_steps} steps: finish() it and start() the next")
        return self._t

    def _bootstrap_step(self):
        if not self._records:
            raise ValueError(f"bootstrap() needs info['final_observation'], and {type(self.env).__name__} was built "
                             "without episode_records=True")
        if self._t is None or self._t == 0:
            raise ValueError("bootstrap() stores V(final_observation) of the step just taken, and no step was taken")
        t = self._t - 1
        if self._last_bootstrap == t:
            raise ValueError(f"step {t} of the rollout is bootstrapped already")
        self._last_bootstrap = t
        self._bootstrapped += 1
        return t

    def _finishing(self):
        """True: every step was bootstrapped; False: none was."""
        if self._t is None or self._t < self.n_steps:
            raise ValueError(f"the rollout holds {self._t or 0} of its {self.n_steps} steps")
        if self._bootstrapped not in (0, self.n_steps):
            raise ValueError(f"bootstrap() was called for {self._bootstrapped} of the rollout's {self.n_steps} steps: a "
                             "partially bootstrapped rollout has no defined advantages (call it after every step or "
                             "after none)")
        self._complete = True
        return self._bootstrapped == self.n_steps

    def _collecting(self, policy, sde_sample_freq):
        """True: `policy` has the Gaussian head of environments/sde.py."""
        if self._t != 0:
            raise ValueError("collect() runs a whole rollout: start() first, and take no step() before it")
        kind = getattr(getattr(policy, "spec", None), "kind", None)
        sde = kind in ("sde", "lstm_sde")
        # (a recurrent policy of environments/lstm.py or lstm_sde.py: collect() keeps its states)
        self._lstm = kind in ("lstm", "lstm_sde")
        if sde and _index_task(self.env):
            raise ValueError("collect() was given a policy with a Gaussian head, and the environment's action space is "
                             f"{self.env.single_action_space!r}: Discrete action spaces have Policy / DevicePolicy")
        if not sde and not _index_task(self.env):
            raise ValueError("collect() takes a policy with a Categorical head, and the environment's action space is "
                             f"{self.env.single_action_space!r}: continuous action spaces are out of scope")
        policy_groups = getattr(policy, "groups", None)
        if self.groups is not None and policy_groups is not None and int(policy_groups) != self.groups:
            raise ValueError(f"collect() of a rollout with groups={self.groups} was given a population policy of "
                             f"{policy_groups} groups")
        # (a population of gSDE learners, environments/population.py: a noise schedule per group)
        self._sde_freqs = None
        if sde and policy_groups is not None:
            self._sde_freqs = self._group_freqs(sde_sample_freq, int(policy_groups))
            return sde
        if int(sde_sample_freq) != sde_sample_freq or (sde_sample_freq < 1 and sde_sample_freq != -1):
            raise ValueError(f"sde_sample_freq {sde_sample_freq!r} is not -1 or a positive integer")
        if not sde and sde_sample_freq != -1:
            raise ValueError("sde_sample_freq belongs to the policies of environments/sde.py and lstm_sde.py")
        return sde

    @staticmethod
    def _group_freqs(sde_sample_freq, groups):
        """sde_sample_freq of a population as G integers: a scalar for all groups, or one value per group."""
        if isinstance(sde_sample_freq, (list, tuple, np.ndarray)):
            freqs = list(sde_sample_freq)
            if len(freqs) != groups:
                raise ValueError(f"sde_sample_freq has {len(freqs)} entries, the population {groups} groups")
        else:
            freqs = [sde_sample_freq] * groups
        for freq in freqs:
            if int(freq) != freq or (freq < 1 and freq != -1):
                raise ValueError(f"sde_sample_freq {freq!r} is not -1 or a positive integer")
        return [int(freq) for freq in freqs]

    def _reset_noise(self, policy, t, sde_sample_freq):
        """stable-baselines3's collect_rollouts: reset_noise before the loop (t None), and in it when _resample says so.
        A population resets every group before the loop and at step t, in ONE call, the groups that are due by their own
        sde_sample_freq -- none at all when no group is."""
        if self._sde_freqs is None:
            if t is None or self._resample(t, sde_sample_freq):
                policy.reset_noise(self.num_envs)
        elif t is None:
            policy.reset_noise(num_envs=self.num_envs)
        else:
            mask = [self._resample(t, freq) for freq in self._sde_freqs]
            if any(mask):
                policy.reset_noise(groups=mask, num_envs=self.num_envs)

    @staticmethod
    def _resample(t, sde_sample_freq):
        """stable-baselines3's collect_rollouts: reset_noise before the loop, and in it when
        sde_sample_freq > 0 and t % sde_sample_freq == 0 (so step 0 draws twice, as there)."""
        return sde_sample_freq > 0 and t % sde_sample_freq == 0

    def _finished(self):
        if not (self._complete and self._t == self.n_steps):
            raise ValueError("the rollout is not finished: advantages and returns are those of finish()")


class Rollout(_Bookkeeping):
    """The rollout buffer of a numpy twin: the oracle of DeviceRollout, with the same methods over numpy arrays.

        rollout = Rollout(env, n_steps=128)
        obs, info = env.reset()
        rollout.start(obs)
        for _ in range(128):
            obs, rewards, terminated, truncated, info = rollout.step(actions, values, log_probs)
            rollout.bootstrap(value_of(info["final_observation"]))      # episode_records=True only
        advantages, returns = rollout.finish(value_of(obs))
        for batch in rollout.minibatches(64): ...
        rollout.start()                                                 # row T becomes row 0
    """

    def __init__(self, env, n_steps, gamma=0.99, gae_lambda=0.95, groups=None):
        """groups=G: gamma and gae_lambda are scalars or G values, group g's for lanes [g m, (g + 1) m) (plain
        attributes: they may be reassigned between rollouts)."""
        self._configure(env, n_steps, gamma, gae_lambda, getattr(env, "_records", None) is not None
                        or bool(getattr(env, "_episode_records", False)), groups)
        steps, n = self.n_steps, self.num_envs
        self.observations = np.zeros((steps + 1, n, self.obs_width), dtype=np.float32)
        self.actions = np.zeros((steps, n), dtype=np.int64 if _index_task(env) else np.float32)
        self.rewards = np.zeros((steps, n), dtype=np.float64)
        self.truncated = np.zeros((steps, n), dtype=np.uint8)
        self.values, self.log_probs, self.final_values, self.advantages, self.returns = (
            np.zeros((steps, n), dtype=np.float32) for _ in range(5))

    def start(self, obs=None):
        self._begin(obs)
        self.observations[0] = self.observations[self.n_steps] if obs is None else obs

    def step(self, actions, values, log_probs, env_actions=None):
        """env_actions: what the environment is stepped with where that is not what the slab keeps (an sde policy's
        clamped actions next to its raw ones)."""
        t = self._next_step()
        self.actions[t] = np.asarray(actions).reshape(self.num_envs)
        self.values[t] = np.asarray(values).reshape(self.num_envs)
        self.log_probs[t] = np.asarray(log_probs).reshape(self.num_envs)
        result = self.env.step(actions if env_actions is None else env_actions)
        self.observations[t + 1], self.rewards[t], self.truncated[t] = result[0], result[1], result[3]
        self._t = t + 1
        return result

    def bootstrap(self, final_values):
        self.final_values[self._bootstrap_step()] = np.asarray(final_values).reshape(self.num_envs)

    def finish(self, last_values):
        final_values = self.final_values if self._finishing() else None
        if self.groups is None:
            self.advantages, self.returns = gae_numpy(self.rewards, self.values, self.truncated, final_values, last_values,
                                                      self.gamma, self.gae_lambda)
        else:
            self.advantages, self.returns = gae_numpy_grouped(self.rewards, self.values, self.truncated, final_values,
                                                              last_values, *self._discounts())
        return self.advantages, self.returns

    def collect(self, policy, deterministic=False, sde_sample_freq=-1):
        """The whole rollout after start(), by a policy.Policy or an sde.SdePolicy: act, step and -- with episode
        records -- the bootstrap of every step, then finish(V(observations[T])).  V(final_observation) of step t - 1
        comes from the act of step t (the last one from the values-only call that gives last_values).  Equal to the
        explicit loop.  With an SdePolicy the noise is reset first and then whenever t % sde_sample_freq == 0 (never
        again with -1), the slab keeps the raw action and the environment gets the clamped one.  With a population of gSDE
        learners (population.SdePopulationPolicy) sde_sample_freq is a scalar or G values: every group's noise is reset
        first, and at step t one reset_noise(groups=mask) covers the groups with f_g > 0 and t % f_g == 0 (no call when
        none is due).  With an LstmPolicy row 0
        of episode_starts is all ones after start(obs) and the row T of the rollout before after start(), row 0 of
        lstm_states is the policy's state, step t goes from lstm_states[t] to lstm_states[t + 1] with episode_starts[t],
        episode_starts[t + 1] = truncated[t], and afterwards the policy's state is row T."""
        sde = self._collecting(policy, sde_sample_freq)
        if sde:
            self._reset_noise(policy, None, sde_sample_freq)
        if self._lstm:
            self._recurrent_rows(policy)
        final_obs = None
        for t in range(self.n_steps):
            if sde:
                self._reset_noise(policy, t, sde_sample_freq)
            if self._lstm:
                actions, values, log_probs, final_values, *clamped = policy.act(
                    self.observations[t], self.episode_starts[t], final_obs, deterministic,
                    states=(self.lstm_states[t], self.lstm_states[t + 1]))
            else:
                actions, values, log_probs, final_values, *clamped = policy.act(self.observations[t], final_obs,
                                                                                deterministic)
            if final_obs is not None:
                self.bootstrap(final_values)
            info = self.step(actions, values, log_probs, *clamped)[4]
            if self._lstm:
                self.episode_starts[t + 1] = self.truncated[t]
            final_obs = info["final_observation"] if self._records else None
        last = (self.observations[self.n_steps],)
        if self._lstm:
            policy.set_lstm_state(self.lstm_states[self.n_steps])
            last += (self.episode_starts[self.n_steps],)
        if final_obs is None:
            return self.finish(policy.values(*last))
        last_values, final_values = policy.values(*last, final_obs)
        self.bootstrap(final_values)
        return self.finish(last_values)

    def _recurrent_rows(self, policy):
        """Row 0 of the two slabs a recurrent policy's collect() keeps (made on first use): every environment starts an
        episode after start(obs), after start() those do that the last step of the rollout before ended; the states
        are the policy's."""
        hidden = policy.spec.lstm_hidden
        if self.lstm_states is None or self.lstm_states.shape[-1] != hidden:
            self.episode_starts = np.zeros((self.n_steps + 1, self.num_envs), dtype=np.uint8)
            self.lstm_states = np.zeros((self.n_steps + 1, 2, 2, self.num_envs, hidden), dtype=np.float32)
        self.episode_starts[0] = 1 if self._fresh else self.truncated[self.n_steps - 1]
        state = policy.lstm_state()
        self.lstm_states[0] = 0.0 if state is None else state

    def flat(self):
        """The rollout as stable-baselines3's swap_and_flatten orders it: index e * T + t."""
        self._finished()
        slabs = dict(zip(FLAT_KEYS, (self.observations[:self.n_steps], self.actions, self.values, self.log_probs,
                                     self.advantages, self.returns)))
        return {key: slab.swapaxes(0, 1).reshape(self.n_steps * self.num_envs, *slab.shape[2:])
                for key, slab in slabs.items()}

    def minibatches(self, batch_size, generator=None):
        """Dicts of flat() rows chosen by one permutation (generator: a numpy.random.Generator); the last one may be
        shorter."""
        flat = self.flat()
        total = self.n_steps * self.num_envs
        order = (np.random.default_rng() if generator is None else generator).permutation(total)
        for first in range(0, total, int(batch_size)):
            index = order[first:first + int(batch_size)]
            yield {key: rows[index] for key, rows in flat.items()}


class DeviceRollout(_Bookkeeping):
    """The rollout buffer of a device-resident environment (DeviceVectorDiscreteSteps, DeviceVectorContinuousJumps or
    DeviceVectorEnvironment, each with device_initializer=True; with or without learner_view= and episode_records=), as
    torch tensors on the environment's GPU.  Used as Rollout is, with reset_tensors() in place of reset(), and bit for
    bit equal to it.

    The slabs are [T][n] row-major: observations float32 [T + 1, n, V], actions [T, n] in the task's dtype (int64 or
    float32), rewards float64, truncated uint8, values / log_probs / final_values / advantages / returns float32.
    step() hands rows of them to step_tensors(out=...), so the environment's own hand-over launch fills the buffer: no
    copy and no launch is added for the step's outputs.  finish() is one launch of rollout_gae_kernel
    (rf_rollout_advantages) on torch's current stream.  No method synchronises the host."""

    def __init__(self, env, n_steps, gamma=0.99, gae_lambda=0.95, groups=None):
        """groups=G: as Rollout's; finish() is then one launch of rollout_gae_kernel<true>
        (rf_rollout_advantages_grouped), which reads (g, gl) per group from a device table the rollout owns.  The
        table is repacked -- one small copy on the current stream -- when gamma or gae_lambda have changed since the
        last finish(), as the population learner repacks its hyper-parameter records."""
        from reinfocus_amd.environments import harness

        if not isinstance(env, harness._DeviceVectorEnv):
            if hasattr(env, "_no_tensors"):  # (a sharded environment: its own refusal says why)
                env._no_tensors()
            raise TypeError(f"DeviceRollout needs a device-resident environment, not {type(env).__name__} (the numpy "
                            "twins have Rollout)")
        io = env._tensor_io()  # (ValueError, as step_tensors': a host initializer, a render_mode)
        self._configure(env, n_steps, gamma, gae_lambda, env._episode_records, groups)
        from reinfocus_amd import torch_interop

        torch = self._torch = torch_interop._torch()
        self._io = io
        self._ctx = env._ctx
        self.device = torch.device("cuda", self._ctx.device)
        steps, n = self.n_steps, self.num_envs

        def slab(dtype, *shape):
            return torch.zeros(shape or (steps, n), dtype=dtype, device=self.device)

        self.observations = slab(torch.float32, steps + 1, n, self.obs_width)
        self.actions = slab(torch.int64 if _index_task(env) else torch.float32)
        self.rewards = slab(torch.float64)
        self.truncated = slab(torch.uint8)
        self.values, self.log_probs, self.final_values, self.advantages, self.returns = (
            slab(torch.float32) for _ in range(5))
        self._last_values = None  # (collect()'s V(observations[T]), made on first use)
        self._env_actions = None  # (collect()'s clamped actions of an sde policy, made on first use)
        self._table = self._table_of = None  # (a grouped rollout's (g, gl) float32 [G, 2] and what it was packed from)

    def _discount_table(self):
        """The device table of a grouped rollout, repacked when gamma or gae_lambda have changed."""
        discounts = self._discounts()
        if self._table_of != discounts:
            packed = self._torch.from_numpy(discount_table(*discounts))
            if self._table is None:
                self._table = self._torch.zeros((self.groups, 2), dtype=self._torch.float32, device=self.device)
            self._table.copy_(packed, non_blocking=True)
            self._table_of = discounts
        return self._table

    def _row(self, tensor, what):
        """`tensor` as a float32-or-whatever [n] row on the buffer's GPU (a view, never a host copy)."""
        if not isinstance(tensor, self._torch.Tensor):
            raise TypeError(f"{what} must be a torch.Tensor on {self.device}, not {type(tensor).__name__}")
        self._io._on_device(tensor, what)
        if tensor.numel() != self.num_envs:
            raise ValueError(f"{what} have shape {tuple(tensor.shape)}, not ({self.num_envs},) or ({self.num_envs}, 1)")
        return tensor.reshape(self.num_envs)

    def start(self, obs=None):
        """Begins a rollout: the first time with the observation reset_tensors() returned, which is copied into row 0;
        afterwards without, and row T of the rollout before becomes row 0 (one device copy on the current stream)."""
        self._begin(obs)
        if obs is None:
            self.observations[0].copy_(self.observations[self.n_steps])
        else:
            self._io._on_device(obs, "obs")
            self.observations[0].copy_(obs)

    def step(self, actions, values, log_probs, env_actions=None):
        """Stores the three tensors in row t and steps the environment into rows of the slabs; returns what
        step_tensors returned (its obs, rewards and truncated ARE the buffer's rows).  env_actions: as Rollout.step."""
        t = self._next_step()
        self._io.checked_actions(actions)  # (before anything is stored)
        if env_actions is not None:
            self._io.checked_actions(env_actions)
        values, log_probs = self._row(values, "values"), self._row(log_probs, "log_probs")
        self.actions[t].copy_(actions.reshape(self.num_envs))
        self.values[t].copy_(values)
        self.log_probs[t].copy_(log_probs)
        result = self.env.step_tensors(actions if env_actions is None else env_actions,
                                       out=(self.observations[t + 1], self.rewards[t], self.truncated[t]))
        self._t = t + 1
        return result

    def bootstrap(self, final_values):
        """Stores V(info["final_observation"]) of the step just taken (NaN where the step did not end an episode: never
        read).  For every step of a rollout or for none."""
        final_values = self._row(final_values, "final_values")
        self.final_values[self._bootstrap_step()].copy_(final_values)

    def finish(self, last_values):
        """(advantages, returns) of the rollout, given V(observations[T]): one kernel launch, nothing waited for."""
        last_values = self._row(last_values, "last_values")
        if last_values.dtype != self._torch.float32 or not last_values.is_contiguous():
            last_values = last_values.to(self._torch.float32).contiguous()
        table = None if self.groups is None else self._discount_table()  # (a refused value: before anything changes)
        bootstrapped = self._finishing()
        final_ptr = self.final_values.data_ptr() if bootstrapped else None
        if table is None:
            self._ctx.rollout_advantages(self.n_steps, self.num_envs, self.rewards.data_ptr(), self.values.data_ptr(),
                                         self.truncated.data_ptr(), final_ptr, last_values.data_ptr(), self.gamma,
                                         self.gae_lambda, self.advantages.data_ptr(), self.returns.data_ptr(),
                                         self._io._stream())
        else:
            self._ctx.rollout_advantages_grouped(self.n_steps, self.num_envs, self.groups, self.rewards.data_ptr(),
                                                 self.values.data_ptr(), self.truncated.data_ptr(), final_ptr,
                                                 last_values.data_ptr(), table.data_ptr(), self.advantages.data_ptr(),
                                                 self.returns.data_ptr(), self._io._stream())
        return self.advantages, self.returns

    def collect(self, policy, deterministic=False, sde_sample_freq=-1):
        """The whole rollout after start(), by a policy.DevicePolicy or an sde.DeviceSdePolicy (whose noise is reset as
        Rollout.collect says -- one launch each time --, whose raw action goes into actions[t] and whose clamped one,
        a row the rollout owns, to the step; with a population.DeviceSdePopulationPolicy and sde_sample_freq a scalar or
        G values, one launch resets the groups that are due): per step ONE policy launch, which writes
        actions[t], values[t], log_probs[t] and -- with episode records, from the final_observation of the step before
        -- final_values[t - 1] straight into the slabs (no row copies), and the environment's step from actions[t];
        after step T a values-only launch gives last_values and final_values[T - 1]; then finish().  As bytes what the
        explicit loop of act / step / bootstrap / finish gives, and Rollout.collect with the twin policy.  With a
        DeviceLstmPolicy the launch of step t also goes from lstm_states[t] to lstm_states[t + 1]; it reads truncated[t - 1]
        as its episode starts, and episode_starts[1:] is one copy of the truncated slab after the loop.  Nothing waits for
        the host."""
        sde = self._collecting(policy, sde_sample_freq)
        if sde:
            self._reset_noise(policy, None, sde_sample_freq)
            if self._env_actions is None:
                self._env_actions = self._torch.zeros(self.num_envs, dtype=self._torch.float32, device=self.device)
        if self._lstm:
            self._recurrent_rows(policy)
        final_obs = None
        for _ in range(self.n_steps):
            t = self._next_step()
            final_out = None if final_obs is None else self.final_values[self._bootstrap_step()]
            if sde:
                self._reset_noise(policy, t, sde_sample_freq)
            out = (self.actions[t], self.values[t], self.log_probs[t], final_out)
            if sde:
                out += (self._env_actions,)
            if self._lstm:
                # episode_starts[t + 1] IS truncated[t]: the call reads the step's own row, and the slab is filled by one
                # copy after the loop -- no launch per step, nothing waited for
                policy.act(self.observations[t], self.episode_starts[0] if t == 0 else self.truncated[t - 1], final_obs,
                           deterministic, out=out, states=(self.lstm_states[t], self.lstm_states[t + 1]))
            else:
                policy.act(self.observations[t], final_obs, deterministic, out=out)
            info = self.env.step_tensors(self._env_actions if sde else self.actions[t],
                                         out=(self.observations[t + 1], self.rewards[t], self.truncated[t]))[4]
            self._t = t + 1
            final_obs = info["final_observation"] if self._records else None
        if self._last_values is None:
            self._last_values = self._torch.zeros(self.num_envs, dtype=self._torch.float32, device=self.device)
        final_out = None if final_obs is None else self.final_values[self._bootstrap_step()]
        if self._lstm:
            self.episode_starts[1:].copy_(self.truncated)
            policy.set_lstm_state(self.lstm_states[self.n_steps])
            policy.values(self.observations[self.n_steps], self.truncated[self.n_steps - 1], final_obs,
                          out=(self._last_values, final_out))
        else:
            policy.values(self.observations[self.n_steps], final_obs, out=(self._last_values, final_out))
        return self.finish(self._last_values)

    def _recurrent_rows(self, policy):
        """As Rollout._recurrent_rows, in device copies on the current stream."""
        torch = self._torch
        hidden = policy.spec.lstm_hidden
        if self.lstm_states is None or self.lstm_states.shape[-1] != hidden:
            self.episode_starts = torch.zeros((self.n_steps + 1, self.num_envs), dtype=torch.uint8, device=self.device)
            self.lstm_states = torch.zeros((self.n_steps + 1, 2, 2, self.num_envs, hidden), dtype=torch.float32,
                                           device=self.device)
        if self._fresh:
            self.episode_starts[0].fill_(1)
        else:
            self.episode_starts[0].copy_(self.truncated[self.n_steps - 1])
        self.lstm_states[0].copy_(policy.lstm_state())

    def flat(self):
        """The rollout as stable-baselines3's swap_and_flatten orders it: index e * T + t.  The slabs are [T][n] (lanes
        of the kernels run along n), so each entry is the transposed view made contiguous: one device copy each."""
        self._finished()
        slabs = dict(zip(FLAT_KEYS, (self.observations[:self.n_steps], self.actions, self.values, self.log_probs,
                                     self.advantages, self.returns)))
        return {key: slab.transpose(0, 1).reshape(self.n_steps * self.num_envs, *slab.shape[2:])
                for key, slab in slabs.items()}

    def minibatches(self, batch_size, generator=None):
        """Dicts of flat() rows chosen by one torch.randperm on the device (generator: a torch.Generator of that
        device); the last one may be shorter."""
        flat = self.flat()
        total = self.n_steps * self.num_envs
        order = self._torch.randperm(total, device=self.device, generator=generator)
        for first in range(0, total, int(batch_size)):
            index = order[first:first + int(batch_size)]
            yield {key: rows[index] for key, rows in flat.items()}
