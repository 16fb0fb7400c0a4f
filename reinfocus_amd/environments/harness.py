"""Thin vector-environment harness for the DiscreteSteps-v0 and ContinuousJumps tasks.

The reference assembles this environment from six strategy objects
(examples/custom_environments.py:114-241 on top of
reinfocus/environments/vector_environment.py:19-176).  Only one of them touches the
GPU (FocusObserver); the others are O(N) numpy glue that SURVEY.md section 8 marks out
of scope for re-implementation.  The benchmark still has to *step* an environment, so
this module reproduces the reference's call order and numpy arithmetic for exactly that
task, vectorised, in one place:

    step:  transform -> ender.step -> observe (render + focus on the GPU) -> reward ->
           terminated/truncated -> same-step auto-reset of the done envs (partial render)

State is float32[N, 2] = [target position, focus plane]; observations are
float32[N, 4] = [focus plane, focus value, their changes], normalised to [-1, 1].
Deliberate difference: the reference's RangedInitializer is unseeded
(state_initializer.py:50); here `seed` makes runs reproducible.

ContinuousJumps (custom_environments.py:244-339) differs from DiscreteSteps in its transformer
(ContinuousJumpTransformer) and its rewarder (ObservationRewarder + StoppedRewarder *
OnTargetRewarder) only; its vector form (VectorContinuousJumps, DeviceVectorContinuousJumps,
ShardedVectorContinuousJumps) is what the reference's docstring prescribes for vectorising an
environment (custom_environments.py:117-133): the same strategies with num_envs in place of 1, driven
by VectorEnvironment with the vector DiscreteSteps' TimeLimitEnder | DivergingEnder.

VectorEnvironment / DeviceVectorEnvironment go further: any composition of the reference's strategy classes
(environments/state_transformer.py, episode_ender.py, episode_rewarder.py, state_initializer.py) around the same
observer -- or, with observer=, around any tree of the observer classes (environments/state_observer.py) that holds one
FocusObserver --, on the host and with the whole step on the GPU (rf_env_configure_composed, rf_env_configure_observed).
"""

import numpy as np

from reinfocus_amd.environments import episode_visualizer
from reinfocus_amd.environments import spaces
from reinfocus_amd.environments import state_initializer
from reinfocus_amd.environments import state_observer
from reinfocus_amd.graphics import render

TARGET, FOCUS = 0, 1  # state element indices (custom_environments.py:169-171)
JUMP_STOP = 0.25 / 2.0  # ContinuousJumps: target_radius / 2.0, the transformer's and the stopped rewarder's threshold


def jump_actions(actions, num_envs):
    """The float32[num_envs] actions of a ContinuousJumps vector step (also accepted as [num_envs, 1]).
    Deliberate difference from the reference: actions that are NaN, infinite or outside [-1, 1] are refused
    (AssertionError, before any state changes), as the device step refuses them (rf_env_step_jumps); the reference's
    ContinuousJumpTransformer would move the focus plane outside [5, 10] or make the camera non-finite."""
    actions = np.asarray(actions, dtype=np.float32)
    if actions.shape not in ((num_envs,), (num_envs, 1)):
        raise AssertionError(f"expected {num_envs} actions (shape ({num_envs},) or ({num_envs}, 1)), got {actions.shape}")
    actions = actions.reshape(num_envs)
    if not np.all(np.abs(actions) <= 1):  # (False for NaN)
        raise AssertionError("ContinuousJumps actions must be finite and in [-1, 1]")
    return actions


RECORD_KEYS = ("final_observation", "episode_return", "episode_length")


class _EpisodeRecords:
    """Episode records of a host twin (episode_records=True), by the one definition the device shares
    (include/reinfocus_hip.h, "episode records"): per environment a float64 return and an int32 length that take every
    step's reward in step order; every step reports, for the environments that ended, the observation row before the
    auto-reset overwrites it, the return and the length (the accumulators then start over), and NaN / NaN / 0 for the
    others.  A full reset zeroes the accumulators."""

    def __init__(self, num_envs):
        self._num_envs = num_envs
        self.reset()

    def reset(self):
        self.returns = np.zeros(self._num_envs, dtype=np.float64)
        self.lengths = np.zeros(self._num_envs, dtype=np.int32)

    def step(self, observations, rewards, done):
        """The step's info: to be called before `observations[done]` is overwritten."""
        self.returns += np.asarray(rewards, dtype=np.float64)  # (one numpy.float64 addition per environment and step)
        self.lengths += 1
        final_observation = np.full(observations.shape, np.nan, dtype=np.float32)
        final_observation[done] = observations[done]
        episode_return = np.full(self._num_envs, np.nan, dtype=np.float64)
        episode_return[done] = self.returns[done]
        episode_length = np.zeros(self._num_envs, dtype=np.int32)
        episode_length[done] = self.lengths[done]
        self.returns[done] = 0.0
        self.lengths[done] = 0
        return {"final_observation": final_observation, "episode_return": episode_return,
                "episode_length": episode_length}

    def accumulators(self):
        return self.returns.copy(), self.lengths.copy()


def _no_single_records(cls, kwargs):
    if kwargs.get("episode_records"):
        raise ValueError(f"{cls.__name__} has no episode records (episode_records=): the single-environment shell never "
                         "resets itself, so no observation is overwritten; use a vector environment")
    if kwargs.get("learner_view") is not None:
        raise ValueError(f"{cls.__name__} has no learner view (learner_view=): the single-environment shell has no batch "
                         "to take moments over; use a vector environment")


class LearnerView:
    """What the reference's PPO configurations wrap the environment in (normalize: true, frame_stack: 5) --
    stable-baselines3's VecNormalize followed by VecFrameStack -- as an opt-in stage of the environment itself
    (learner_view=LearnerView(frame_stack=5)): reset() / step() / reset_tensors() / step_tensors() then return the
    running-moment-normalised, clipped observation stacked frame_stack deep (float32 [n, frame_stack * W]) and the reward
    divided by the running standard deviation of the discounted return; info holds "raw_observation" and "raw_reward",
    and with episode_records=True "final_observation" is put through the same two transforms ("raw_final_observation"
    is the raw row).  The definition is include/reinfocus_hip.h's ("learner view"); defaults are SB3's.  One deliberate
    difference: the batch moments are taken in float64 by a fixed pairwise tree (treesum), not by numpy.mean / numpy.var
    in float32.

    groups=G (opt-in; include/reinfocus_hip.h, "population view"): the n lanes are G groups of m = n / G consecutive
    lanes, as the population (environments/population.py) owns them, and every group has running moments of its own --
    taken over its own m lanes -- and a gamma of its own (gamma: a scalar for all groups, or G values): G independent
    VecNormalize wrappers in one environment.  This gamma is VecNormalize's, the discount of the returns whose variance
    scales the reward; the rollout's gamma (rollout.Rollout / DeviceRollout) is passed separately -- rl_zoo3 sets both
    from the trial's gamma."""

    def __init__(self, frame_stack=1, norm_obs=True, norm_reward=True, gamma=0.99, epsilon=1e-8, clip_obs=10.0,
                 clip_reward=10.0, training=True, groups=None):
        self.frame_stack = int(frame_stack)
        self.norm_obs, self.norm_reward, self.training = bool(norm_obs), bool(norm_reward), bool(training)
        self.groups, self.gammas = None, None
        if groups is None:
            if np.ndim(gamma) != 0:
                raise ValueError(f"gamma {gamma!r} is a sequence, and that needs groups= (one gamma per group)")
        else:
            self.groups = int(groups)
            if self.groups != groups or not 1 <= self.groups <= MAX_VIEW_GROUPS:
                raise ValueError(f"groups {groups!r} is not in 1 .. {MAX_VIEW_GROUPS}")
            values = np.asarray(gamma, dtype=np.float64)
            if values.ndim == 0:
                values = np.full(self.groups, float(values), dtype=np.float64)
            if values.shape != (self.groups,):
                raise ValueError(f"gamma has shape {values.shape}: a scalar or {self.groups} values, one per group")
            self.gammas = tuple(float(value) for value in values)
            for value in self.gammas:
                if not 0.0 <= value <= 1.0:
                    raise ValueError(f"gamma {value!r} outside [0, 1]")
            gamma = self.gammas[0]
        self.gamma, self.epsilon = float(gamma), float(epsilon)
        self.clip_obs, self.clip_reward = float(clip_obs), float(clip_reward)
        if not 1 <= self.frame_stack <= 8:
            raise ValueError(f"frame_stack {frame_stack!r} outside 1 to 8")
        for name in ("epsilon", "clip_obs", "clip_reward"):
            if not (np.isfinite(getattr(self, name)) and getattr(self, name) > 0.0):
                raise ValueError(f"{name} {getattr(self, name)!r} is not finite and positive")
        if not 0.0 <= self.gamma <= 1.0:
            raise ValueError(f"gamma {gamma!r} outside [0, 1]")

    def describe(self):
        """The configuration without `training` (which may change later), as snapshots compare it."""
        if self.groups is not None:
            return (f"LearnerView(frame_stack={self.frame_stack}, norm_obs={self.norm_obs}, "
                    f"norm_reward={self.norm_reward}, groups={self.groups}, gamma={self.gammas!r}, "
                    f"epsilon={self.epsilon!r}, clip_obs={self.clip_obs!r}, clip_reward={self.clip_reward!r})")
        return (f"LearnerView(frame_stack={self.frame_stack}, norm_obs={self.norm_obs}, norm_reward={self.norm_reward}, "
                f"gamma={self.gamma!r}, epsilon={self.epsilon!r}, clip_obs={self.clip_obs!r}, "
                f"clip_reward={self.clip_reward!r})")

    def group(self, index):
        """The ungrouped LearnerView of group `index`: what a stand-alone trial over that group's lanes would have."""
        return LearnerView(self.frame_stack, self.norm_obs, self.norm_reward, self.gammas[index], self.epsilon,
                           self.clip_obs, self.clip_reward, self.training)

    def group_size(self, num_envs, who):
        """m = num_envs / groups of a grouped view; a num_envs the groups do not divide is refused."""
        if num_envs % self.groups != 0:
            raise ValueError(f"{who} has {num_envs} environments, which the learner view's {self.groups} groups do not "
                             "divide (group g owns lanes [g m, (g + 1) m))")
        return num_envs // self.groups

    def spaces(self, single_observation_space, num_envs):
        """(single_observation_space, observation_space) of the view: the bounds are +-clip_obs with norm_obs, else the
        raw ones, repeated frame_stack times."""
        low, high = single_observation_space.low, single_observation_space.high
        if self.norm_obs:
            low, high = np.full_like(low, -self.clip_obs), np.full_like(high, self.clip_obs)
        single = spaces.Box(np.tile(low, self.frame_stack).astype(np.float32),
                            np.tile(high, self.frame_stack).astype(np.float32), dtype=np.float32)
        return single, spaces.batch_space(single, num_envs)


MAX_VIEW_GROUPS = 65535  # RF_POPULATION_MAX_GROUPS


def io_torch():
    """torch, imported where a *_tensors method needs it (reinfocus_amd/torch_interop.py)."""
    from reinfocus_amd import torch_interop

    torch_interop.check_one_runtime()
    return torch_interop._torch()


def _checked_view(learner_view):
    if learner_view is not None and not isinstance(learner_view, LearnerView):
        raise TypeError(f"learner_view must be a harness.LearnerView or None, not {type(learner_view).__name__}")
    return learner_view


def treesum(x):
    """The learner view's sum of x[0..n): x as float64, padded with +0.0 to the next power of two, adjacent pairs added
    until one value is left, and that value + (+0.0) (which turns -0.0 into +0.0, so that any further zero padding gives
    the same bits).  The order is part of the contract: the device evaluates exactly this tree."""
    y = np.asarray(x, dtype=np.float64).ravel()
    size = 1
    while size < y.size:
        size *= 2
    y = np.concatenate([y, np.zeros(size - y.size, dtype=np.float64)])
    while y.size > 1:
        y = y[0::2] + y[1::2]
    return y[0] + np.float64(0.0)


class _LearnerView:
    """The learner view of a host twin (learner_view=), by the one definition the device shares
    (include/reinfocus_hip.h, "learner view"; kernels in csrc/rf_env_view.h), in numpy float64 without contraction."""

    def __init__(self, config, num_envs, width):
        self.config = config
        self.training = config.training
        self._n, self._width, self._cells = num_envs, width, config.frame_stack * width
        self.mean = np.zeros(width + 1, dtype=np.float64)
        self.var = np.ones(width + 1, dtype=np.float64)
        self.count = np.full(width + 1, 1e-4, dtype=np.float64)
        self.stack = np.zeros((num_envs, self._cells), dtype=np.float32)
        self.returns = np.zeros(num_envs, dtype=np.float64)

    def _update(self, slot, x):
        """RunningMeanStd.update_from_moments, left to right, the batch moments by treesum"""
        N = np.float64(self._n)
        bm = treesum(x) / N
        d = np.asarray(x, dtype=np.float64) - bm
        bv = treesum(d * d) / N
        mean, var, count = self.mean[slot], self.var[slot], self.count[slot]
        delta = bm - mean
        tot = count + N
        m2 = (var * count + bv * N) + (((delta * delta) * count) * N) / tot
        self.mean[slot] = mean + (delta * N) / tot
        self.var[slot] = m2 / tot
        self.count[slot] = tot

    def _update_observations(self, observations):
        if self.training and self.config.norm_obs:
            for column in range(self._width):
                self._update(column, observations[:, column])

    def _normalise(self, rows):
        if not self.config.norm_obs:
            return np.array(rows, dtype=np.float32)
        width, clip = self._width, self.config.clip_obs
        z = (rows.astype(np.float64) - self.mean[:width]) / np.sqrt(self.var[:width] + self.config.epsilon)
        return np.clip(z, -clip, clip).astype(np.float32)

    def reset(self, observations):
        """The view observation after a reset (a reset never resets the moments)."""
        with np.errstate(invalid="ignore"):
            self.returns = np.zeros(self._n, dtype=np.float64)
            self._update_observations(observations)
            self.stack = np.zeros((self._n, self._cells), dtype=np.float32)
            self.stack[:, self._cells - self._width:] = self._normalise(observations)
        return self.stack.copy()

    def step(self, observations, rewards, done, final_observation=None):
        """(view observation, view reward, view_final or None) of a step: `observations` as the step returns them (rows
        of environments that ended are already the first of their next episode), final_observation the raw record
        (episode_records=True) or None."""
        width, cells, config = self._width, self._cells, self.config
        rewards = np.asarray(rewards, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            self._update_observations(observations)                                                    # 1
            newest = self._normalise(observations)                                                     # 2
            if self.training:                                                                          # 3
                self.returns = self.returns * config.gamma + rewards
                self._update(width, self.returns)
            view_rewards = rewards.copy()                                                              # 4
            if config.norm_reward:
                view_rewards = np.clip(rewards / np.sqrt(self.var[width] + config.epsilon), -config.clip_reward,
                                       config.clip_reward)
            self.stack[:, :cells - width] = self.stack[:, width:].copy()                               # 5
            view_final = None
            if final_observation is not None:                                                          # 6
                view_final = np.full((self._n, cells), np.nan, dtype=np.float32)
                view_final[done, :cells - width] = self.stack[done, :cells - width]
                view_final[done, cells - width:] = self._normalise(final_observation[done])
            self.stack[done] = 0.0                                                                     # 7
            self.returns[done] = 0.0
            self.stack[:, cells - width:] = newest                                                     # 8
        return self.stack.copy(), view_rewards, view_final

    def statistics(self):
        return {"mean": self.mean.copy(), "var": self.var.copy(), "count": self.count.copy()}

    def set_statistics(self, mean, var, count):
        for name, value in (("mean", mean), ("var", var), ("count", count)):
            value = np.array(value, dtype=np.float64)
            assert value.shape == (self._width + 1,), f"{name} has shape {value.shape}, not ({self._width + 1},)"
            setattr(self, name, value)


class _GroupedLearnerView:
    """The learner view with groups=G (include/reinfocus_hip.h, "population view"), literally: G _LearnerView objects,
    group g's over lanes [g m, (g + 1) m) with gamma[g], results concatenated -- as PopulationPolicy is G Policy
    objects.  The oracle of the grouped kernels (csrc/rf_env_view.h)."""

    def __init__(self, config, num_envs, width):
        self.config = config
        self._m = config.group_size(num_envs, "the environment")
        self._n, self._width, self._cells = num_envs, width, config.frame_stack * width
        self.views = [_LearnerView(config.group(g), self._m, width) for g in range(config.groups)]

    def _lanes(self, g):
        return slice(g * self._m, (g + 1) * self._m)

    @property
    def training(self):
        return self.views[0].training

    @training.setter
    def training(self, value):
        for view in self.views:
            view.training = value

    @property
    def stack(self):
        return np.concatenate([view.stack for view in self.views])

    @property
    def returns(self):
        return np.concatenate([view.returns for view in self.views])

    def reset(self, observations):
        return np.concatenate([view.reset(observations[self._lanes(g)]) for g, view in enumerate(self.views)])

    def step(self, observations, rewards, done, final_observation=None):
        rewards = np.asarray(rewards, dtype=np.float64)
        parts = [view.step(observations[self._lanes(g)], rewards[self._lanes(g)], done[self._lanes(g)],
                           None if final_observation is None else final_observation[self._lanes(g)])
                 for g, view in enumerate(self.views)]
        view_obs, view_rewards, view_final = (list(column) for column in zip(*parts))
        return (np.concatenate(view_obs), np.concatenate(view_rewards),
                None if final_observation is None else np.concatenate(view_final))

    def statistics(self, group=None):
        """float64 [G, W + 1] each; with group=g that group's (W + 1,) rows."""
        if group is not None:
            return self.views[_checked_group(group, len(self.views))].statistics()
        rows = [view.statistics() for view in self.views]
        return {key: np.stack([row[key] for row in rows]) for key in ("mean", "var", "count")}

    def set_statistics(self, mean, var, count, group=None):
        if group is not None:
            self.views[_checked_group(group, len(self.views))].set_statistics(mean, var, count)
            return
        arrays = [np.array(value, dtype=np.float64) for value in (mean, var, count)]
        for value in arrays:
            assert value.shape == (len(self.views), self._width + 1), (
                f"statistics of shape {value.shape}, not ({len(self.views)}, {self._width + 1})")
        for g, view in enumerate(self.views):
            view.set_statistics(*(value[g] for value in arrays))


def _checked_group(group, groups):
    if groups is None:
        raise ValueError("group= belongs to a learner view with groups=")
    if int(group) != group or not 0 <= group < groups:
        raise ValueError(f"group {group!r} is not in 0 .. {groups - 1}")
    return int(group)


class _ViewedTwin:
    """What the host twins with learner_view= share: the view around reset() / step() results, and its accessors."""

    _view = None  # (a _LearnerView, or with groups= a _GroupedLearnerView, with learner_view=)

    def _configure_view(self, learner_view):
        learner_view = _checked_view(learner_view)
        if learner_view is None:
            return
        width = self.single_observation_space.shape[0]
        if learner_view.groups is None:
            self._view = _LearnerView(learner_view, self.num_envs, width)
        else:
            learner_view.group_size(self.num_envs, type(self).__name__)
            self._view = _GroupedLearnerView(learner_view, self.num_envs, width)
        self.single_observation_space, self.observation_space = learner_view.spaces(self.single_observation_space,
                                                                                    self.num_envs)

    def _viewed_reset(self, observations, info):
        if self._view is None:
            return observations, info
        return self._view.reset(observations), {"raw_observation": observations}

    def _viewed_step(self, observations, rewards, terminated, truncated, info):
        if self._view is None:
            return observations, rewards, terminated, truncated, info
        rewards = np.asarray(rewards, dtype=np.float64)
        view_obs, view_rewards, view_final = self._view.step(observations, rewards, terminated | truncated,
                                                             info.get("final_observation"))
        info = dict(info, raw_observation=observations, raw_reward=rewards)
        if view_final is not None:
            info["raw_final_observation"] = info["final_observation"]
            info["final_observation"] = view_final
        return view_obs, view_rewards, terminated, truncated, info

    def _the_view(self):
        if self._view is None:
            raise ValueError(f"{type(self).__name__} was built without learner_view=")
        return self._view

    def view_statistics(self, group=None):
        """{"mean", "var", "count"}: float64[W + 1] each, the returns last (what VecNormalize.save keeps).  With a
        grouped view float64[G, W + 1] each, or with group=g that group's (W + 1,) rows: that trial's VecNormalize."""
        view = self._the_view()
        if group is None:
            return view.statistics()
        _checked_group(group, view.config.groups)
        return view.statistics(group)

    def set_view_statistics(self, statistics, group=None):
        view = self._the_view()
        if group is None:
            view.set_statistics(statistics["mean"], statistics["var"], statistics["count"])
            return
        _checked_group(group, view.config.groups)
        view.set_statistics(statistics["mean"], statistics["var"], statistics["count"], group)

    def view_statistics_tensor(self, out=None):
        """The statistics as one float64 array [G, 3, W + 1] (mean, var, count; [3, W + 1] of an ungrouped view): what
        the device classes keep as a tensor (rf_env_view_get_statistics_device).  out=: written in place."""
        statistics = self.view_statistics()
        stacked = np.stack([statistics[key] for key in ("mean", "var", "count")], axis=-2)
        if out is None:
            return stacked
        out[...] = stacked
        return out

    def set_view_statistics_tensor(self, statistics):
        statistics = np.asarray(statistics, dtype=np.float64)
        mean, var, count = (statistics[..., row, :] for row in range(3))
        self.set_view_statistics({"mean": mean, "var": var, "count": count})

    def set_view_training(self, training):
        """VecNormalize.training: False freezes the moments and the returns."""
        self._the_view().training = bool(training)

    def view_state(self):
        """(stack float32[n, V], returns float64[n])"""
        view = self._the_view()
        return view.stack.copy(), view.returns.copy()


def _gymnasium_bases():
    """(Env base, VectorEnv base): gymnasium's classes when gymnasium is importable -- the
    reference's environments derive from gymnasium.Env (environments/environment.py:19) and
    gymnasium.experimental.vector.VectorEnv (environments/vector_environment.py:19; plain
    gymnasium.vector.VectorEnv from gymnasium 1.0 on), which gymnasium.make_vec, its wrappers and
    the SB3 shim rely on -- otherwise `object` (this image has no gymnasium)."""
    try:
        import gymnasium
    except ImportError:
        return object, object
    try:
        from gymnasium.experimental.vector import VectorEnv  # gymnasium ~= 0.29 (pyproject.toml:29)
    except ImportError:
        from gymnasium.vector import VectorEnv
    return gymnasium.Env, VectorEnv


_EnvBase, _VectorEnvBase = _gymnasium_bases()


class _Initializer:
    """Uniform states in `ends` (state_initializer.py:30-71, vectorised and seedable)."""

    def __init__(self, ends, seed):
        self._ends = ends
        self._generator = np.random.Generator(np.random.PCG64DXSM(seed))

    def initialize(self, num_envs):
        return self._generator.uniform(self._ends[0], self._ends[1], size=(num_envs, 2)).astype(np.float32)

    def propose(self, num_envs):
        """The rows initialize(num_envs) WOULD return, without consuming them: the device-resident step hands row r to the
        r-th environment that ends and initialize(k) then draws exactly the k rows that were used (same consumption as
        vector_environment.py:144).  The generator's state is saved and put back -- a deepcopy of the Generator cost 15-65 us
        per step, a quarter of a small environment's step -- and the rows are low + (high - low) * random(), which is what
        Generator.uniform computes (tests/test_harness_logic.py compares them bit for bit)."""
        bit_generator = self._generator.bit_generator
        state = bit_generator.state
        lo, hi = self._ends
        rows = (lo + (hi - lo) * self._generator.random((num_envs, 2))).astype(np.float32)
        bit_generator.state = state
        return rows


class _Ender:
    """TimeLimitEnder | DivergingEnder (episode_ender.py:580-656, :106-207, :369-452);
    max_steps None leaves only the diverging rule (the non-vector DiscreteSteps)."""

    def __init__(self, num_envs, max_steps, threshold, early_end_steps):
        self._num_envs = num_envs
        self._max_steps = max_steps
        self._threshold = threshold
        self._early_end_steps = early_end_steps
        self._steps = np.zeros(num_envs, dtype=np.int32)
        self._diverging_steps = np.zeros(num_envs, dtype=np.int32)
        self._last_diff = np.zeros(num_envs, dtype=np.float32)

    def step(self, states):
        self._steps += 1
        diff = abs(states[:, TARGET] - states[:, FOCUS])
        self._diverging_steps[diff > self._last_diff + self._threshold] += 1
        self._last_diff = diff

    def is_terminated(self):
        return np.full(self._num_envs, False)

    def is_truncated(self):
        truncated = self._diverging_steps >= self._early_end_steps
        if self._max_steps is not None:
            truncated = (self._steps >= self._max_steps) | truncated
        return truncated

    def reset(self, states, indices=None):
        if indices is None:
            indices = np.full(self._num_envs, True)
        self._steps[indices] = 0
        self._diverging_steps[indices] = 0
        self._last_diff[indices] = abs(states[:, TARGET] - states[:, FOCUS])

    def status(self, index):
        """episode_ender.py:646-656, :191-207, :439-452: what the visualiser prints."""
        diverging = self._diverging_steps[index]
        r_status = f"diverging {diverging} / {self._early_end_steps}" if diverging > 0 else ""
        if self._max_steps is None:
            return r_status
        l_status = f"step {self._steps[index]} / {self._max_steps}"
        return l_status + (", " if l_status and r_status else "") + r_status


def delta_bounds(lows, highs, max_change=None, include_original=False):
    """Observation bounds of DeltaObserver (state_observer.py:166-230): a change is bounded by
    high - low of what it is a change of, or by max_change where that is given (finite); with
    include_original the wrapped bounds come first.  float32, as gymnasium's Box."""
    lows = np.asarray(lows, dtype=np.float32)
    highs = np.asarray(highs, dtype=np.float32)
    diff = highs - lows
    if max_change is not None:
        max_change = np.asarray(max_change, dtype=np.float32)
        diff = np.where(np.isfinite(max_change), max_change, diff).astype(np.float32)
    if include_original:
        return np.append(lows, -diff), np.append(highs, diff)
    return -diff, diff


def normaliser_from_bounds(low, high):
    """mid / scale of NormalizedObserver (state_observer.py:440-470): observations are mapped
    from [low, high] to [-1, 1] as clip((x - mid) / scale, -1, 1); everything float32."""
    spans = np.vstack([low, high]).astype(np.float32)
    return np.average(spans, axis=0), np.diff(spans / 2, axis=0).reshape(spans.shape[1])


def normaliser_constants(ends, max_move, min_focus, max_focus):
    """mid / scale of NormalizedObserver over DeltaObserver([IndexedElement, Focus], True,
    [max_move, nan]) -- custom_environments.py:196-218."""
    low, high = delta_bounds([ends[0], min_focus], [ends[1], max_focus], [max_move, np.nan], True)
    return normaliser_from_bounds(low, high)


class _Observer:
    """NormalizedObserver(DeltaObserver([IndexedElementObserver, FocusObserver], True,
    [max_move, nan])) -- state_observer.py:166-292, :386-517."""

    def __init__(self, num_envs, ends, max_move, focus_observer):
        self._focus = focus_observer
        self._mid, self._scale = normaliser_constants(
            ends, max_move, focus_observer.single_observation_space.low[0],
            focus_observer.single_observation_space.high[0])
        self._old = np.full((num_envs, 2), np.nan, dtype=np.float32)
        self._num_envs = num_envs
        self.single_observation_space = spaces.Box(-np.ones(4, dtype=np.float32), np.ones(4, dtype=np.float32),
                                                   dtype=np.float32)
        self.observation_space = spaces.batch_space(self.single_observation_space, num_envs)

    def _wrapped(self, states, indices):
        position = states[:, FOCUS].reshape((indices.sum(), 1))
        return np.hstack([position, self._focus.observe(states, indices)], dtype=np.float32)

    def _normalize(self, values):
        return np.clip((values - self._mid) / self._scale, -1, 1, dtype=np.float32)

    def observe(self, states, indices=None):
        if indices is None:
            indices = np.full(self._num_envs, True)
        wrapped = self._wrapped(states, indices)
        observations = np.hstack([wrapped, wrapped - self._old[indices]], dtype=np.float32)
        self._old[indices] = wrapped
        return self._normalize(observations)

    def reset(self, states, indices=None):
        if indices is None:
            indices = np.full(self._num_envs, True)
        wrapped = self._wrapped(states, indices)
        observations = np.hstack([wrapped, np.zeros(wrapped.shape, dtype=np.float32)], dtype=np.float32)
        self._old[indices] = wrapped
        return self._normalize(observations)


def default_observer(num_envs, ends, max_focus_move, renderer, frame_height=300):
    """The built-in observer (_Observer) restated with the public classes: NormalizedObserver(DeltaObserver(
    [IndexedElementObserver(1), FocusObserver], True, [max_focus_move, nan])) over states [target, focus plane] in
    `ends` -- custom_environments.py:196-218.  Observations equal the built-in observer's bit for bit."""
    focus = state_observer.FocusObserver(num_envs, TARGET, FOCUS, ends, renderer, frame_height)
    position = state_observer.IndexedElementObserver(num_envs, FOCUS, ends[0], ends[1])
    return state_observer.NormalizedObserver(state_observer.DeltaObserver(
        [position, focus], True, np.array([max_focus_move, np.nan], dtype=np.float32)))


def _described_renderer(observer, frame_height, samples_per_pixel, device):
    """(FocusObserver, renderer, frame height, samples per pixel) of an environment given an observer tree: they are
    those of the tree's one FocusObserver, and the environment's own keywords must be left at their defaults or agree."""
    from reinfocus_amd.environments import strategy_program

    focus = strategy_program.focus_observer(observer)
    renderer = focus._renderer
    assert frame_height in (300, focus._frame_height), \
        f"frame_height {frame_height} is not the FocusObserver's {focus._frame_height}"
    assert samples_per_pixel in (100, renderer._samples_per_pixel), \
        f"samples_per_pixel {samples_per_pixel} is not the FocusObserver's renderer's {renderer._samples_per_pixel}"
    assert device is None or device == renderer._ctx.device, \
        f"device {device} is not the FocusObserver's renderer's {renderer._ctx.device}"
    return focus, renderer, focus._frame_height, renderer._samples_per_pixel


def _checked_focus_index(index, single_observation_space):
    width = single_observation_space.shape[0]
    assert isinstance(index, (int, np.integer)) and 0 <= index < width, \
        f"focus_observation_index {index!r} outside the {width} observation columns"
    return int(index)


class _Rewarder:
    """DeltaRewarder + ObservationRewarder + OnTargetRewarder
    (episode_rewarder.py:86-155, :210-292)."""

    def __init__(self, scale, span, focus_value_o_index=1):
        self._scale = scale
        self._span = span
        self._o_index = focus_value_o_index
        self._old_states = None

    def reset(self, states, observations, indices=None):
        if self._old_states is not None and indices is not None:
            self._old_states[indices] = states[:, FOCUS]
        else:
            self._old_states = states[:, FOCUS]

    def reward(self, states, observations):
        moved = abs(states[:, FOCUS] - self._old_states) * -1.0 / self._scale
        self._old_states = states[:, FOCUS]
        on_target = (abs(states[:, TARGET] - states[:, FOCUS]) < self._span) * 1.0 + 0.0
        return (moved + observations[:, self._o_index]) + on_target


class _JumpTransformer:
    """ContinuousJumpTransformer (state_transformer.py:66-118): the element `move_index` jumps to the position in
    `limits` proportional to the action's in [-1, 1], unless the jump is not longer than stop_threshold.  No clip."""

    def __init__(self, move_index, limits, stop_threshold):
        self._move_index = move_index
        self._limits = limits
        self._stop_threshold = abs(stop_threshold)

    def transform(self, states, actions):
        new_states = states.copy()
        actions = (np.asarray(actions).flatten() + 1) / 2.0
        moved_states = actions * (self._limits[1] - self._limits[0]) + self._limits[0]
        moved = abs(new_states[:, self._move_index] - moved_states) > self._stop_threshold
        new_states[moved, self._move_index] = moved_states[moved]
        return new_states


class _StoppedRewarder:
    """StoppedRewarder (episode_rewarder.py:361-429): `reward` where the element `check_index` moved less than
    threshold since the last step (or the episode's start)."""

    def __init__(self, check_index, threshold, reward=1.0):
        self._check_index = check_index
        self._threshold = abs(threshold)
        self._reward = reward
        self._old_states = None

    def reset(self, states, observations, indices=None):
        if self._old_states is not None and indices is not None:
            self._old_states[indices] = states[:, self._check_index]
        else:
            self._old_states = states[:, self._check_index]

    def reward(self, states, observations):
        reward = (abs(states[:, self._check_index] - self._old_states) < self._threshold) * self._reward
        self._old_states = states[:, self._check_index]
        return reward


class _JumpRewarder:
    """ObservationRewarder(1) + StoppedRewarder(1, stop_threshold) * OnTargetRewarder((0, 1), span)
    (custom_environments.py:316-323; episode_rewarder.py:210-292, :361-429): float64 focus value + [stopped] *
    [on target]."""

    def __init__(self, stop_threshold, span, focus_value_o_index=1):
        self._stopped = _StoppedRewarder(FOCUS, stop_threshold)
        self._span = span
        self._o_index = focus_value_o_index

    def reset(self, states, observations, indices=None):
        self._stopped.reset(states, observations, indices)

    def _on_target(self, states, observations):
        return (abs(states[:, TARGET] - states[:, FOCUS]) < self._span) * 1.0 + 0.0

    def reward(self, states, observations):
        return observations[:, self._o_index] + (self._stopped.reward(states, observations)
                                                 * self._on_target(states, observations))


def _jump_spaces(env, num_envs):
    """ContinuousJumpTransformer's action space (state_transformer.py:85), batched."""
    env.single_action_space = spaces.Box(-1, 1, (1,), dtype=np.float32)
    env.action_space = spaces.batch_space(env.single_action_space, num_envs)


class _HostGlue(_ViewedTwin):
    """The DiscreteSteps task with the reference's numpy glue on the host around the GPU
    render + focus (FocusObserver): everything VectorDiscreteSteps, DiscreteSteps and
    ContinuousJumps share.  Not an environment class by itself."""

    metadata = {"render_modes": ["rgb_array"], "render_fps": 4}
    _records = None  # (an _EpisodeRecords with episode_records=True)

    def __init__(self, max_episode_steps=20, num_envs=1, render_mode=None, *, frame_height=300,
                 samples_per_pixel=100, seed=None, device=None, first_state_index=0, host_frames=False,
                 _diverging_only=False, episode_records=False, learner_view=None):
        """host_frames=True: the literal drop-in route (FastRenderer(host_frames=True): frames come back to the
        host every render and vision.focus_values uploads them again), identical results.
        episode_records=True (opt-in): step()'s info holds "final_observation", "episode_return" and "episode_length"
        (_EpisodeRecords); episode_accumulators() reads the running ones.
        learner_view=LearnerView(...) (opt-in): reset() / step() return the learner view (_LearnerView)."""
        super().__init__()
        self._records = _EpisodeRecords(num_envs) if episode_records else None
        ends = (5.0, 10.0)
        target_radius = 0.25
        max_move = 5.0
        moves = max_move / 2.0 ** np.arange(6)

        assert render_mode is None or render_mode in self.metadata["render_modes"]
        self.render_mode = render_mode
        self.num_envs = num_envs

        self._renderer = render.FastRenderer(samples_per_pixel=samples_per_pixel, device=device,
                                             first_state_index=first_state_index, host_frames=host_frames)
        self._ender = _Ender(num_envs, None if _diverging_only else max_episode_steps, target_radius / 2, 3)
        self._initializer = _Initializer(ends, seed)
        self._focus_observer = state_observer.FocusObserver(num_envs, TARGET, FOCUS, ends, self._renderer,
                                                            frame_height)
        self._observer = _Observer(num_envs, ends, max_move, self._focus_observer)
        self._rewarder = _Rewarder(target_radius * 2, target_radius)
        # DiscreteMoveTransformer (state_transformer.py:222-266)
        self._action_set = np.concatenate([-moves, [0], moves[::-1]])
        self._limits = ends
        # custom_environments.py:229-238; observation element 1 is the focus value
        self._visualizer = episode_visualizer.HistoryVisualizer(
            num_envs, TARGET, FOCUS, 1, self._renderer, ends, ender=self._ender, target_radius=target_radius)

        self.single_action_space = spaces.Discrete(len(self._action_set))
        self.action_space = spaces.batch_space(self.single_action_space, num_envs)
        self.single_observation_space = self._observer.single_observation_space
        self.observation_space = self._observer.observation_space
        self._configure_view(learner_view)
        self._state = None

    # -- vector_environment.py:75-102 ------------------------------------------------------
    def reset(self, *, seed=None, options=None, state=None):
        """`state` (extension) pins the initial state instead of drawing it."""
        if seed is not None:
            self._initializer = _Initializer(self._limits, seed)
        self._state = (self._initializer.initialize(self.num_envs) if state is None
                       else np.array(state, dtype=np.float32).reshape(self.num_envs, 2))
        self._ender.reset(self._state)
        observations = self._observer.reset(self._state, None)
        self._rewarder.reset(self._state, observations)
        if self._records is not None:
            self._records.reset()
        if self.render_mode == "rgb_array":
            self._visualizer.reset(self._state, observations)
        return self._viewed_reset(observations, {})

    def episode_accumulators(self):
        """(returns float64[num_envs], lengths int32[num_envs]) of the running episodes (episode_records=True)."""
        if self._records is None:
            raise ValueError(f"{type(self).__name__} was built without episode_records=True")
        return self._records.accumulators()

    def _transform(self, states, actions):
        new_states = states.copy()
        new_states[:, FOCUS] += self._action_set[np.asarray(actions).flatten()]
        return np.clip(new_states, *self._limits)

    # -- vector_environment.py:104-164 -------------------------------------------------------
    def step(self, actions):
        assert self._state is not None
        self._state = self._transform(self._state, actions)
        self._ender.step(self._state)
        observations = self._observer.observe(self._state)
        rewards = self._rewarder.reward(self._state, observations)
        terminated = self._ender.is_terminated()
        truncated = self._ender.is_truncated()
        done = terminated | truncated
        info = {} if self._records is None else self._records.step(observations, rewards, done)
        if done.any():
            new_state = self._initializer.initialize(done.sum())
            self._state[done] = new_state
            self._ender.reset(new_state, done)
            new_observations = self._observer.reset(new_state, done)
            observations[done] = new_observations
            self._rewarder.reset(new_state, new_observations, done)
            if self.render_mode == "rgb_array":
                self._visualizer.reset(new_state, new_observations, done)
        if self.render_mode == "rgb_array":
            not_done = ~done
            self._visualizer.step(self._state[not_done], observations[not_done], not_done)
        return self._viewed_step(observations, rewards, terminated, truncated, info)

    def render(self):
        """vector_environment.py:166-176 -> HistoryVisualizer.visualize
        (episode_visualizer.py:188-201): the 600 px rendering of every environment (which
        advances / re-seeds the RNG states exactly as the reference's does) next to its
        performance plot."""
        if self.render_mode == "rgb_array":
            return self._visualizer.visualize()
        return None

    def render_frames(self):
        """Only the left halves of render(): uint8[num_envs, 600, 600, 3], no matplotlib."""
        return np.asarray(self._renderer.render(600))

    def close(self):
        self._renderer.close()


class VectorDiscreteSteps(_HostGlue, _VectorEnvBase):
    """The DiscreteSteps-v0 vector environment (custom_environments.py:114-241) with the
    reference's numpy glue on the host.  Same constructor arguments and defaults as the
    reference; frame_height / samples_per_pixel / seed / device / first_state_index are
    extensions (defaults = the reference's 300 px, 100 spp, device LOCAL_RANK).
    DeviceVectorDiscreteSteps is the same environment with the glue on the GPU (the default of
    registration.make_vec); results are identical bit for bit."""


class DiscreteSteps(_HostGlue, _EnvBase):
    """The single-environment DiscreteSteps (custom_environments.py:16-111 on
    environments/environment.py): one env, DivergingEnder only, unbatched returns."""

    def __init__(self, render_mode=None, **kwargs):
        _no_single_records(type(self), kwargs)
        super().__init__(num_envs=1, render_mode=render_mode, _diverging_only=True, **kwargs)
        self.action_space = self.single_action_space
        self.observation_space = self.single_observation_space

    def reset(self, *, seed=None, options=None, state=None):
        observations, info = super().reset(seed=seed, options=options, state=state)
        return observations[0], info

    def step(self, action):
        # environment.py: no auto-reset in the single-env shell
        self._state = self._transform(self._state, np.array([action]))
        self._ender.step(self._state)
        observations = self._observer.observe(self._state)
        if self.render_mode == "rgb_array":  # environment.py:119-120
            self._visualizer.step(self._state, observations)
        reward = self._rewarder.reward(self._state, observations)[0]
        return observations[0], reward, self._ender.is_terminated()[0], self._ender.is_truncated()[0], {}


class ContinuousJumps(_HostGlue, _EnvBase):
    """The single-environment ContinuousJumps (examples/custom_environments.py:244-339):
    one continuous action in [-1, 1] jumps the focus plane to the proportional position in
    [5, 10] unless the jump is shorter than target_radius / 2
    (ContinuousJumpTransformer, state_transformer.py:66-118); DivergingEnder only; reward =
    focus value + [stopped] * [on target] (ObservationRewarder + StoppedRewarder *
    OnTargetRewarder, episode_rewarder.py:210-292, :361-429)."""

    def __init__(self, render_mode=None, **kwargs):
        _no_single_records(type(self), kwargs)
        super().__init__(num_envs=1, render_mode=render_mode, _diverging_only=True, **kwargs)
        self._stop_threshold = abs(0.25 / 2.0)
        self.single_action_space = spaces.Box(-1, 1, dtype=np.float32)
        self.action_space = self.single_action_space
        self.observation_space = self.single_observation_space
        self._old_focus = None

    def reset(self, *, seed=None, options=None, state=None):
        observations, info = super().reset(seed=seed, options=options, state=state)
        self._old_focus = self._state[:, FOCUS]  # StoppedRewarder.reset keeps a view
        return observations[0], info

    def _transform(self, states, actions):
        new_states = states.copy()
        actions = (np.asarray(actions, dtype=np.float32).flatten() + 1) / 2.0
        moved_states = actions * (self._limits[1] - self._limits[0]) + self._limits[0]
        moved = abs(new_states[:, FOCUS] - moved_states) > self._stop_threshold
        new_states[moved, FOCUS] = moved_states[moved]
        return new_states

    def step(self, action):
        self._state = self._transform(self._state, np.array([action]))
        self._ender.step(self._state)
        observations = self._observer.observe(self._state)
        if self.render_mode == "rgb_array":
            self._visualizer.step(self._state, observations)
        stopped = (abs(self._state[:, FOCUS] - self._old_focus) < self._stop_threshold) * 1.0
        self._old_focus = self._state[:, FOCUS]
        on_target = (abs(self._state[:, TARGET] - self._state[:, FOCUS]) < 0.25) * 1.0 + 0.0
        reward = (observations[:, 1] + stopped * on_target)[0]
        return observations[0], reward, self._ender.is_terminated()[0], self._ender.is_truncated()[0], {}


class VectorContinuousJumps(_HostGlue, _VectorEnvBase):
    """A vector ContinuousJumps (custom_environments.py:244-339 with num_envs in place of 1, and the vector
    DiscreteSteps' TimeLimitEnder | DivergingEnder, :185-190) with the reference's numpy glue on the host, driven as
    VectorEnvironment.step drives its strategies (vector_environment.py:104-164).  Same extensions as
    VectorDiscreteSteps.  Actions: float32[num_envs] (or [num_envs, 1]) in [-1, 1]; NaN, infinite or out-of-range
    actions are refused before any state changes (jump_actions: a deliberate difference from the reference).
    DeviceVectorContinuousJumps is the same environment with the glue on the GPU; results are identical bit for bit."""

    def __init__(self, max_episode_steps=20, num_envs=1, render_mode=None, **kwargs):
        super().__init__(max_episode_steps, num_envs, render_mode, **kwargs)
        self._transformer = _JumpTransformer(FOCUS, self._limits, JUMP_STOP)
        self._rewarder = _JumpRewarder(JUMP_STOP, 0.25)
        _jump_spaces(self, num_envs)

    def _transform(self, states, actions):
        return self._transformer.transform(states, actions)

    def step(self, actions):
        return super().step(jump_actions(actions, self.num_envs))


class _DeviceShard:
    """One rf_ctx holding a contiguous range of device-resident environments (rf_env_*): the context, its RNG states
    at `first_state_index`, and the rf_env_config of the task (custom_environments.py:166-241) -- DiscreteSteps, or
    ContinuousJumps with jumps=True (rf_env_configure_jumps).  DeviceVectorDiscreteSteps /
    DeviceVectorContinuousJumps own one, the sharded environments one per device."""

    ENDS = (5.0, 10.0)
    TARGET_RADIUS = 0.25
    MAX_MOVE = 5.0
    EARLY_END_STEPS = 3  # DivergingEnder(..., early_end_steps=3), custom_environments.py:186-190

    def __init__(self, num_envs, max_episode_steps, frame_height, samples_per_pixel, device, first_state_index,
                 jumps=False, program=None, ends=None, max_move=None, observer_program=None):
        """program: an rf_env_program (rf_env_configure_composed) with the built-in observer's `ends` and `max_move`, or
        with observer_program, an rf_env_observer_program, in its place (rf_env_configure_observed)."""
        import math

        from reinfocus_amd import _native, vision
        from reinfocus_amd.graphics import camera

        ends = self.ENDS if ends is None else tuple(ends)
        max_move = self.MAX_MOVE if max_move is None else max_move
        moves = self.MAX_MOVE / 2.0 ** np.arange(6)
        self.action_set = np.concatenate([-moves, [0], moves[::-1]])
        self.num_envs = num_envs
        self.frame_height = frame_height
        self.samples_per_pixel = samples_per_pixel
        self.first_state_index = int(first_state_index)
        self.max_episode_steps = max_episode_steps
        self.ctx = _native.Context(device)
        try:
            min_focus, max_focus = state_observer.cached_focus_extrema(ends, frame_height, samples_per_pixel,
                                                                       self.ctx.device)
            box = spaces.Box(min_focus, max_focus, dtype=np.float32)  # float32 rounding of the extrema
            mid, scale = normaliser_constants(ends, max_move, box.low[0], box.high[0])
            cams = camera.FastCameras()
            cfg = _native.EnvConfig()
            cfg.n = num_envs
            cfg.n_actions = len(self.action_set)
            for i, a in enumerate(self.action_set):
                cfg.action_set[i] = float(a)
            cfg.limit_lo, cfg.limit_hi = self.ENDS
            cfg.max_steps = max_episode_steps if max_episode_steps else 0
            cfg.diverge_threshold = self.TARGET_RADIUS / 2
            cfg.early_end_steps = self.EARLY_END_STEPS
            for i in range(4):
                cfg.mid[i] = float(mid[i])
                cfg.scale[i] = float(scale[i])
            cfg.reward_scale = self.TARGET_RADIUS * 2
            cfg.on_target_span = self.TARGET_RADIUS
            cfg.half_width = cams._half_width
            cfg.half_height = cams._half_height
            cfg.tan_half_r = math.tan(math.radians(20 / 2))
            for i in range(3):
                cfg.look_from[i] = float(cams._look_from[i])
                cfg.cam_u[i] = float(cams._u[i])
                cfg.cam_v[i] = float(cams._v[i])
                cfg.cam_w[i] = float(cams._w[i])
            cfg.lens_radius = float(cams._half_aperture)
            cfg.frame_height = frame_height
            cfg.spp = samples_per_pixel
            cfg.gray_mode = vision.GRAY_MODE
            self.ctx.seed(num_envs * frame_height * frame_height, 0, self.first_state_index)
            if observer_program is not None:
                self.ctx.env_configure_observed(cfg, program, observer_program)
            elif program is not None:
                self.ctx.env_configure_composed(cfg, program)
            elif jumps:  # (limit_lo / limit_hi: the range the focus plane jumps in)
                self.ctx.env_configure_jumps(cfg, JUMP_STOP)
            else:
                self.ctx.env_configure(cfg)
        except Exception:
            self.ctx.close()
            raise

    # -- what HistoryVisualizer needs from a renderer / an ender (episode_visualizer.py:197, :268) --
    def render(self, frame_height):
        """FastRenderer.render on the renderer the reference's FocusObserver and visualiser share
        (render.py:165-188, :248-257): the scene set uploaded last, states re-created from seed 0
        when more are needed than exist."""
        needed = self.ctx.env_scene_len() * frame_height * frame_height
        if self.ctx.num_states() < needed:
            self.ctx.seed(needed, 0, self.first_state_index)
        return self.ctx.env_render(frame_height, self.samples_per_pixel)

    def status(self, index):
        """_Ender.status from the counters on the device."""
        steps, diverging = self.ctx.env_counters()
        r_status = f"diverging {diverging[index]} / {self.EARLY_END_STEPS}" if diverging[index] > 0 else ""
        if not self.max_episode_steps:
            return r_status
        l_status = f"step {steps[index]} / {self.max_episode_steps}"
        return l_status + (", " if l_status and r_status else "") + r_status


def _device_spaces(env, action_set, num_envs):
    """action_set None: ContinuousJumps' Box(-1, 1, (1,))."""
    if action_set is None:
        _jump_spaces(env, num_envs)
    else:
        env.single_action_space = spaces.Discrete(len(action_set))
        env.action_space = spaces.batch_space(env.single_action_space, num_envs)
    env.single_observation_space = spaces.Box(-np.ones(4, dtype=np.float32), np.ones(4, dtype=np.float32),
                                              dtype=np.float32)
    env.observation_space = spaces.batch_space(env.single_observation_space, num_envs)


class _DeviceVectorEnv(_VectorEnvBase):
    """The device-resident vector environment of either task (_JUMPS): DeviceVectorDiscreteSteps,
    DeviceVectorContinuousJumps.

    device_initializer=True (opt-in): the initializer is compiled into a device program as well
    (strategy_program.compile_initializer, rf_env_configure_initializer) and the context draws the reset states itself --
    reset() passes no states unless state= pins them, step() passes no pool and draws nothing on the host, and
    reset(seed=...) reseeds the host object and uploads its generator's state.  The initializer object, like the other
    strategy objects of a device environment, then only describes the environment: it is not advanced, and
    initializer_state() reads the device's generator.  Results are the same bit for bit either way."""

    metadata = {"render_modes": ["rgb_array"], "render_fps": 4}
    _JUMPS = False
    _episode_records = False
    _learner_view = None

    def __init__(self, max_episode_steps=20, num_envs=1, render_mode=None, *, frame_height=300,
                 samples_per_pixel=100, seed=None, device=None, first_state_index=0, device_initializer=False,
                 episode_records=False, learner_view=None):
        super().__init__()
        assert render_mode is None or render_mode in self.metadata["render_modes"]
        self.render_mode = render_mode
        self.num_envs = num_envs
        self._shard = _DeviceShard(num_envs, max_episode_steps, frame_height, samples_per_pixel, device,
                                   first_state_index, jumps=self._JUMPS)
        self._ctx = self._shard.ctx
        self._limits = _DeviceShard.ENDS
        self._device_initializer = bool(device_initializer)
        self._initializer = self._task_initializer(seed)
        self._configure_initializer()
        self._configure_records(episode_records)
        self._action_set = None if self._JUMPS else self._shard.action_set
        _device_spaces(self, self._action_set, num_envs)
        self._configure_view(learner_view)
        self._visualizer = None
        if render_mode == "rgb_array":  # custom_environments.py:229-238
            self._visualizer = episode_visualizer.HistoryVisualizer(
                num_envs, TARGET, FOCUS, 1, self._shard, self._limits, ender=self._shard,
                target_radius=_DeviceShard.TARGET_RADIUS)

    @property
    def _state(self):
        return self._ctx.env_states()

    def _task_initializer(self, seed):
        """The tasks' initializer: _Initializer, or for the device the RangedInitializer that draws exactly its rows
        (one range per element: low + (high - low) * random(), from the same generator)."""
        if self._device_initializer:
            return state_initializer.RangedInitializer([[self._limits], [self._limits]], seed)
        return _Initializer(self._limits, seed)

    def _configure_initializer(self):
        """device_initializer=True: compiles self._initializer and hands it to the context (which is closed if the
        initializer cannot run on the device)."""
        if not self._device_initializer:
            return
        from reinfocus_amd.environments import strategy_program

        try:
            self._ctx.env_configure_initializer(strategy_program.compile_initializer(self._initializer))
        except Exception:
            self._ctx.close()
            raise

    def _configure_records(self, episode_records):
        """episode_records=True (opt-in): the context keeps final observations, episode returns and lengths
        (rf_env_configure_records; the definition is _EpisodeRecords', the kernels' env_record_one).  step()'s info then
        holds the three arrays (fresh numpy arrays, fetched after the step), step_tensors()'s the same as torch tensors
        the environment owns, episode_accumulators() reads the running ones, and a snapshot holds the accumulators."""
        self._episode_records = bool(episode_records)
        if not self._episode_records:
            return
        try:
            self._ctx.env_configure_records(True)
        except Exception:
            self._ctx.close()
            raise

    def _configure_view(self, learner_view):
        """learner_view=LearnerView(...) (opt-in): the context keeps the learner view (rf_env_configure_view, after the
        records it reads; the definition is _LearnerView's, the kernels are csrc/rf_env_view.h's).  To be called once the
        raw spaces are set: they become the view's."""
        self._learner_view = _checked_view(learner_view)
        if self._learner_view is None:
            return
        from reinfocus_amd import _native

        view = self._learner_view
        try:
            config = _native.EnvViewConfig(view.frame_stack, view.norm_obs, view.norm_reward, view.training, view.gamma,
                                           view.epsilon, view.clip_obs, view.clip_reward)
            if view.groups is None:
                self._ctx.env_configure_view(config)
            else:  # (rf_env_configure_view_grouped: moments and a gamma per group of n / G lanes)
                view.group_size(self.num_envs, type(self).__name__)
                self._ctx.env_configure_view_grouped(config, view.groups, view.gammas)
        except Exception:
            self._ctx.close()
            raise
        self.single_observation_space, self.observation_space = view.spaces(self.single_observation_space, self.num_envs)

    def _the_view(self):
        if self._learner_view is None:
            raise ValueError(f"{type(self).__name__} was built without learner_view=")
        return self._learner_view

    def view_statistics(self, group=None):
        """{"mean", "var", "count"}: float64[W + 1] each, the returns last, from the device (what VecNormalize.save
        keeps).  With a grouped view float64[G, W + 1] each, or with group=g that group's (W + 1,) rows.
        Synchronises."""
        groups = self._the_view().groups
        if group is not None:
            group = _checked_group(group, groups)
        if groups is None:
            return dict(zip(("mean", "var", "count"), self._ctx.env_view_statistics()))
        arrays = self._ctx.env_view_statistics_grouped()
        return dict(zip(("mean", "var", "count"), arrays if group is None else (a[group].copy() for a in arrays)))

    def set_view_statistics(self, statistics, group=None):
        groups = self._the_view().groups
        arrays = [statistics[key] for key in ("mean", "var", "count")]
        if group is not None:  # (one group's rows: the others keep theirs)
            group = _checked_group(group, groups)
            rows = [np.array(a, dtype=np.float64) for a in arrays]
            arrays = self._ctx.env_view_statistics_grouped()
            for a, row in zip(arrays, rows):
                assert row.shape == a[group].shape, f"statistics of shape {row.shape}, not {a[group].shape}"
                a[group] = row
        if groups is None:
            self._ctx.env_view_set_statistics(*arrays)
        else:
            self._ctx.env_view_set_statistics_grouped(*arrays)

    def _statistics_shape(self):
        groups, columns = self._the_view().groups, self._ctx._env_obs_width + 1
        return (3, columns) if groups is None else (groups, 3, columns)

    def _checked_statistics_tensor(self, tensor, what):
        io = self._tensor_io()
        torch = io_torch()
        shape = self._statistics_shape()
        if not isinstance(tensor, torch.Tensor):
            raise TypeError(f"{what} must be a torch.Tensor on the environment's GPU, not {type(tensor).__name__}")
        if tensor.dtype != torch.float64 or tuple(tensor.shape) != shape or not tensor.is_contiguous():
            raise ValueError(f"{what} is {tensor.dtype} {tuple(tensor.shape)}, not contiguous torch.float64 {shape}")
        io._on_device(tensor, what)
        return io

    def view_statistics_tensor(self, out=None):
        """view_statistics() without the host: one torch.float64 tensor [G, 3, W + 1] (mean, var, count; [3, W + 1] of an
        ungrouped view) on the environment's GPU (rf_env_view_get_statistics_device).  Stream-ordered after the steps
        before it, never waits.  out=: written in place; otherwise a fresh tensor."""
        self._the_view()
        if out is None:
            self._tensor_io()
            torch = io_torch()
            out = torch.empty(self._statistics_shape(), dtype=torch.float64,
                              device=torch.device("cuda", self._ctx.device))
        io = self._checked_statistics_tensor(out, "out")
        self._ctx.env_view_statistics_device(out.data_ptr(), io._stream())
        return out

    def set_view_statistics_tensor(self, statistics):
        """set_view_statistics() from such a tensor (rf_env_view_set_statistics_device): what sync_envs_normalization
        does, training environment -> tensor -> evaluation environment, without crossing to the host."""
        self._the_view()
        io = self._checked_statistics_tensor(statistics, "statistics")
        self._ctx.env_view_set_statistics_device(statistics.data_ptr(), io._stream())

    def set_view_training(self, training):
        """VecNormalize.training: False freezes the moments and the returns."""
        self._the_view()
        self._ctx.env_view_set_training(training)

    def view_state(self):
        """(stack float32[n, V], returns float64[n]) from the device.  Synchronises."""
        self._the_view()
        return self._ctx.env_view_state()

    def episode_accumulators(self):
        """(returns float64[num_envs], lengths int32[num_envs]) of the running episodes, from the device
        (rf_env_get_record_accumulators).  Synchronises."""
        if not self._episode_records:
            raise ValueError(f"{type(self).__name__} was built without episode_records=True")
        return self._ctx.env_record_accumulators()

    def initializer_state(self):
        """(state, inc) of the initializer's PCG64DXSM generator as Python ints: the device's with
        device_initializer=True (rf_env_get_initializer_state), the host object's otherwise."""
        from reinfocus_amd.environments import strategy_program

        if self._device_initializer:
            return self._ctx.env_initializer_state()
        return strategy_program.initializer_state(self._initializer)

    # -- what the tasks and the composed environment differ in ---------------------------------
    def _reseed(self, seed):
        self._initializer = self._task_initializer(seed)

    def _checked(self, actions):
        """The step's actions, refused here where the task says so (the library checks the rest)."""
        return jump_actions(actions, self.num_envs) if self._JUMPS else actions

    def _float_actions(self):
        """float32 actions (rf_env_step_jumps), not int32 indices (rf_env_step)."""
        return self._JUMPS

    def reset(self, *, seed=None, options=None, state=None):
        if seed is not None:
            self._reseed(seed)
            if self._device_initializer:
                from reinfocus_amd.environments import strategy_program

                self._ctx.env_set_initializer_state(*strategy_program.initializer_state(self._initializer))
        if state is not None:
            initial = np.array(state, dtype=np.float32).reshape(self.num_envs, 2)
        elif self._device_initializer:
            initial = None  # (drawn on the device)
        else:
            initial = self._initializer.initialize(self.num_envs)
        observations = self._ctx.env_reset(initial)
        if self._visualizer is not None:
            self._visualizer.reset(self._state if initial is None else initial, observations)
        if self._learner_view is not None:
            return self._ctx.env_view(rewards=False)[0], {"raw_observation": observations}
        return observations, {}

    def step(self, actions):
        actions = self._checked(actions)
        pool = None if self._device_initializer else self._initializer.propose(self.num_envs)
        env_step = self._ctx.env_step_jumps if self._float_actions() else self._ctx.env_step
        observations, rewards, truncated, used = env_step(actions, pool)
        self._last_used = used
        if used and not self._device_initializer:
            self._initializer.initialize(used)  # consume exactly the rows that were used
        if self._visualizer is not None:  # vector_environment.py:149-156
            state = self._state
            if used:
                self._visualizer.reset(state[truncated], observations[truncated], truncated)
            self._visualizer.step(state[~truncated], observations[~truncated], ~truncated)
        info = dict(zip(RECORD_KEYS, self._ctx.env_records())) if self._episode_records else {}
        if self._learner_view is not None:  # (one more copy and synchronisation, as the records')
            info.update(raw_observation=observations, raw_reward=rewards)
            observations, rewards, view_final = self._ctx.env_view(final=self._episode_records)
            if view_final is not None:
                info["raw_final_observation"] = info["final_observation"]
                info["final_observation"] = view_final
        return observations, rewards, np.full(self.num_envs, False), truncated, info

    def render(self):
        """vector_environment.py:166-176."""
        if self._visualizer is not None:
            return self._visualizer.visualize()
        return None

    def render_frames(self):
        """Only the left halves of render(): the 600 px frames of the scene set uploaded last."""
        return self._shard.render(episode_visualizer.HistoryVisualizer.FRAME)

    # -- torch tensors in and out, nothing on the host (rf_env_step_device; reinfocus_amd/torch_interop.py) ----------
    def _tensor_io(self):
        """The environment's torch_interop.TensorIO, made on first use -- or the ValueError that says why there is none."""
        io = self.__dict__.get("_tensors")
        if io is not None:
            return io
        if not self._device_initializer:
            raise ValueError(f"{type(self).__name__} with device_initializer=False has no *_tensors methods: its "
                             "initializer lives on the host and advances by the number of environments that ended, "
                             "which only a host synchronisation per step can tell it (pass device_initializer=True)")
        if self.render_mode is not None:
            raise ValueError(f"{type(self).__name__} with render_mode={self.render_mode!r} has no *_tensors methods: "
                             "the visualiser reads states and observations on the host after every step")
        from reinfocus_amd import torch_interop

        io = self._tensors = torch_interop.TensorIO(self._ctx, self.num_envs, self._ctx._env_obs_width,
                                                    self._float_actions(), self._ctx.device, self._episode_records,
                                                    0 if self._learner_view is None else self._learner_view.frame_stack)
        return io

    def reset_tensors(self, *, seed=None):
        """reset() with the observations as a torch.float32 [num_envs, W] tensor on the environment's GPU: (obs, {}).
        Nothing is waited for (seed=... reseeds the device's generator, which does synchronise).  obs is the
        environment's own tensor: the next reset_tensors / step_tensors call without out= overwrites it."""
        io = self._tensor_io()
        if seed is not None:
            from reinfocus_amd.environments import strategy_program

            self._reseed(seed)
            self._ctx.env_set_initializer_state(*strategy_program.initializer_state(self._initializer))
        if self._learner_view is not None:  # (the view observation; info holds the raw one, owned alike)
            return io.reset_viewed()
        return io.reset(), {}

    def step_tensors(self, actions, *, out=None):
        """step() from a torch tensor of actions on the environment's GPU -- contiguous, shape [num_envs] or
        [num_envs, 1], torch.int32 / torch.int64 for index tasks, torch.float32 for float tasks; anything else raises
        TypeError / ValueError before the library is called -- to torch tensors there: (obs float32 [num_envs, W],
        rewards float64 [num_envs], terminated bool [num_envs] (all False), truncated bool [num_envs], info).  info is
        {} -- or with episode_records=True "final_observation" (float32 [num_envs, W]), "episode_return" (float64
        [num_envs]) and "episode_length" (int32 [num_envs]) as tensors the environment owns and the next call overwrites,
        whatever out= says.  The step is
        ordered after what torch's current stream holds, that stream waits for it, and the host waits for nothing.

        Without out= the environment owns ONE set of output tensors and overwrites it in the next call, as vector
        environments commonly do: clone what must outlive a step.  out=(obs, rewards, truncated) writes into the
        caller's tensors instead (truncated: torch.bool or torch.uint8).

        Actions are checked on the device.  An invalid one (an index outside the action set, NaN, a jump outside
        [-1, 1]) cannot refuse the step as step() does: it is replaced, the steps go on, and device_fault() -- or the
        next step(), snapshot() or render_frames() -- reports it; from then on the environment refuses everything until
        reset() / reset_tensors().  step() and step_tensors() may be mixed freely."""
        result = self._tensor_io().step(actions, out)
        self._last_used = None
        return result

    def device_fault(self):
        """None, or (step, env) of the earliest invalid action step_tensors met since the last reset -- steps counted
        from that reset, the lowest environment within the step.  Synchronises."""
        return self._tensor_io().fault()

    def last_reset_count(self):
        """How many environments ended (and were reset) in the last step of either form.  Synchronises."""
        if self.__dict__.get("_last_used") is None:
            self._last_used = self._tensor_io().reset_count()
        return self._last_used

    # -- snapshots (rf_env_snapshot* / rf_env_restore*; reinfocus_amd/environments/snapshot.py) -----------
    def _snapshots_possible(self):
        if self.render_mode is not None:
            raise ValueError(f"{type(self).__name__} with render_mode={self.render_mode!r} has no snapshots: the "
                             "visualiser's histories live in Python objects, and its 600 px render re-seeds the RNG "
                             "states a snapshot would hold")

    def _host_generator(self):
        """The host initializer's bit generator when it is the one that draws the reset states, else None."""
        return None if self._device_initializer else self._initializer._generator.bit_generator

    def _snapshot_described(self, blob, generator):
        from reinfocus_amd.environments import snapshot

        return snapshot.EnvSnapshot(blob, type(self).__name__, self.num_envs, self._shard.frame_height,
                                    self._shard.samples_per_pixel, generator, self._episode_records)

    def _host_generators(self):
        """slot -> the host generator's state when that resident slot was filled"""
        return self.__dict__.setdefault("_slot_generators", {})

    def snapshot(self):
        """Everything that decides what later reset() / step() / render_frames() calls return, as an EnvSnapshot (host
        memory; .save(path) writes it): the library's blob and, when the reset states are drawn on the host, the
        initializer's generator.  Refused before the first reset(), after a failed step, and with a render_mode."""
        self._snapshots_possible()
        generator = self._host_generator()
        return self._snapshot_described(self._ctx.env_snapshot(), None if generator is None else generator.state)

    def restore(self, snapshot):
        """Puts a snapshot() back: on the environment it was taken from (rewind), or on an equal one -- the same class
        and arguments, possibly in another process -- that may not have been reset() yet (resume).  The environment then
        goes on as the snapshotted one did.  A snapshot that does not fit is refused and nothing changes: ValueError
        where this environment can tell, AssertionError from the library (the message names the difference)."""
        self._snapshots_possible()
        mine = self._snapshot_described(snapshot.blob, None)
        if snapshot.describe() != mine.describe():
            raise ValueError(f"the snapshot is of {snapshot.describe()}, this environment is {mine.describe()}")
        generator = self._host_generator()
        if (generator is None) != (snapshot.host_generator is None):
            raise ValueError("the snapshot was taken with device_initializer=%s, this environment has device_initializer=%s"
                             % (snapshot.host_generator is None, generator is None))
        if generator is not None and generator.state["bit_generator"] != snapshot.host_generator["bit_generator"]:
            raise ValueError(f"the snapshot's initializer draws from a {snapshot.host_generator['bit_generator']}, this "
                             f"environment's from a {generator.state['bit_generator']}")
        self._ctx.env_restore(snapshot.blob)
        if generator is not None:
            generator.state = snapshot.host_generator

    def snapshot_resident(self, slot=0):
        """snapshot() into the context's slot `slot` (0-3) in device memory, for rewinding often: nothing crosses to the
        host, and the call only enqueues the copy.  A slot costs as much device memory as the snapshot has bytes --
        16 bytes per pixel for the RNG states, 4.29 GB at 4096 x 256 x 256 -- until drop_snapshot(slot)."""
        self._snapshots_possible()
        generator = self._host_generator()
        self._ctx.env_snapshot_resident(slot)
        if generator is not None:
            self._host_generators()[int(slot)] = generator.state

    def restore_resident(self, slot=0):
        """Puts the slot's snapshot back (any number of times); an empty slot is refused (AssertionError)."""
        self._snapshots_possible()
        self._ctx.env_restore_resident(slot)
        generator = self._host_generator()
        if generator is not None:
            generator.state = self._host_generators()[int(slot)]

    def drop_snapshot(self, slot=0):
        """Frees the slot's device memory."""
        self._ctx.env_snapshot_drop(slot)
        self._host_generators().pop(int(slot), None)

    def close(self):
        self._ctx.close()


class DeviceVectorDiscreteSteps(_DeviceVectorEnv):
    """VectorDiscreteSteps with the whole step resident on the GPU (rf_env_*, SURVEY.md
    section 8(f) item 1): same constructor, same reset/step results bit for bit, but a step
    only uploads the actions and the initializer's candidate states and downloads
    observations, rewards and flags.  This is what `DiscreteSteps-v0`'s vector entry point
    builds.  The initializer stays on the host (numpy PCG64DXSM): a copy of the generator
    proposes num_envs candidate states per step, the device hands row r to the r-th environment
    that ended, and the real generator then draws exactly the rows that were used -- the same
    consumption as VectorDiscreteSteps.  render_mode="rgb_array" works as in the reference
    (HistoryVisualizer on the environment's own renderer state: the 600 px render advances /
    re-seeds the RNG states the next step uses)."""


class DeviceVectorContinuousJumps(_DeviceVectorEnv):
    """VectorContinuousJumps with the whole step resident on the GPU (rf_env_configure_jumps, rf_env_step_jumps): the
    DiscreteSteps step's kernels with the continuous-jump transform and the stopped * on-target reward, selected by the
    context's task; same constructor and reset/step results bit for bit as VectorContinuousJumps, the same
    initializer consumption and render_mode="rgb_array" as DeviceVectorDiscreteSteps.  Actions: float32[num_envs]
    (or [num_envs, 1]) in [-1, 1]; NaN, infinite or out-of-range actions are refused before any state changes."""

    _JUMPS = True


def split_environments(num_envs, shards):
    """Contiguous env ranges [first, first + count) per shard, as even as possible."""
    counts = [num_envs // shards + (1 if g < num_envs % shards else 0) for g in range(shards)]
    firsts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(int)
    return [(int(f), int(c)) for f, c in zip(firsts, counts)]


class _ShardSet:
    """What HistoryVisualizer needs from "the renderer" and "the ender" of a sharded environment
    (episode_visualizer.py:197, :268): every shard draws the scene set it uploaded last -- each
    behaves like the reference's one shared renderer for its own environment range -- and the rows
    are stacked in shard order."""

    def __init__(self, env):
        self._env = env

    def render(self, frame_height):
        # After a step in which k > 0 environments ended, one device holds the k compacted rows of the auto-reset
        # (rf_env_scene_len): here those are the shards that had resets, in shard order -- global index order, the
        # compacted order.  A shard without resets that step still holds its full set and contributes nothing then.
        ended = self._env._last_ended
        partial = ended is not None and sum(ended) > 0
        chosen = [g for g in range(len(self._env._shards)) if not partial or ended[g] > 0]
        futures = [self._env._threads[g].submit(lambda shard=self._env._shards[g]: np.asarray(shard.render(frame_height)))
                   for g in chosen]
        return np.concatenate([f.result() for f in futures])

    def status(self, index):
        g, local = self._env._locate(index)
        return self._env._threads[g].submit(self._env._shards[g].status, local).result()


class _ShardedVectorEnv(_VectorEnvBase):
    """The device-resident environment of either task (_JUMPS) over several GPUs of one node: ShardedVectorDiscreteSteps
    is DeviceVectorDiscreteSteps, ShardedVectorContinuousJumps DeviceVectorContinuousJumps so sharded (the
    reference has no counterpart: vector_environment.py:104-164 steps all environments on one
    device).  Environments are independent, so device g owns the contiguous range
    [first_g, first_g + n_g) -- one rf_ctx and one host thread per device (a single-worker executor
    each; ctypes releases the GIL), no device-to-device traffic, the host concatenates observations /
    rewards / flags (8 + 16 + 1 bytes per environment).

    RNG states: shard g is seeded at global state index first_state_index + first_g * h * h
    (pixel index = e * h * w + y * w + x, render.py:217), so full renders draw exactly what one
    device holding all environments would draw.  Initializer: one generator for the whole
    environment; the r-th environment that ended, in global index order, takes the r-th drawn
    state, as on one device -- which is why a step has two halves: the rows a shard takes depend on
    how many environments ended before it.  The cut is before the render (rf_env_step_plan /
    rf_env_step_run: which environments end depends on their counters alone), so the first half is
    cheap and the second is the fused step -- one render launch per shard.

    Auto-reset renders.  On one device the partial render indexes RNG states from 0 over the
    compacted rows of all environments that ended (vector_environment.py:144 -> render.py:217):
    compacted row r draws from the states of environment slot r.
     * default: every shard renders its own ended environments from its own state base -- balanced,
       no traffic, but after the first auto-reset a sharded run and a one-device run are different
       (equally valid) sample paths;
     * exact=True: row r is rendered by the shard that owns slot r (rf_env_render_states) and the
       focus value returns through the host to the shard the environment lives on
       (rf_env_step_end_given): bit-identical to one device through any number of auto-resets, at the
       price of the first shards rendering everybody's resets.  Meant for tests and reproducibility
       studies, not for throughput.
    render_mode="rgb_array": HistoryVisualizer over the shards (each shard's 600 px render advances /
    re-seeds that shard's RNG states as the reference's single renderer would for its range; the
    exact mode does not extend to visualised runs).  `devices` may name a device more than once
    (several contexts on one GPU: tests, rehearsals).  numa_pin: every shard thread restricts itself
    to the CPUs of its GPU's NUMA node (`placements` says where each shard ended up)."""

    metadata = {"render_modes": ["rgb_array"], "render_fps": 4}
    _JUMPS = False

    def __init__(self, max_episode_steps=20, num_envs=1, render_mode=None, *, devices=None, frame_height=300,
                 samples_per_pixel=100, seed=None, first_state_index=0, exact=False, numa_pin=True,
                 device_initializer=False, episode_records=False, learner_view=None):
        import concurrent.futures
        from reinfocus_amd import _native

        if learner_view is not None:
            raise ValueError(f"{type(self).__name__} has no learner view (learner_view=): a sharded environment's step is "
                             "cut in two halves on several contexts, and the view's moments are one batch's; use a "
                             "Device* class on one device")

        if episode_records:
            raise ValueError(f"{type(self).__name__} has no episode records (episode_records=): a sharded environment's "
                             "step is cut in two halves on several contexts; use a Device* class on one device")

        if device_initializer:
            raise ValueError(f"{type(self).__name__} draws its reset states on the host; a sharded environment cannot "
                             "draw them on its devices (device_initializer=)")
        super().__init__()
        assert render_mode is None or render_mode in self.metadata["render_modes"]
        # (one array of RNG states aliased by 300 px and 600 px renders cannot be reproduced across devices, and the
        # exact mode's row renders replace the scene sets the visualiser would draw)
        assert not (exact and render_mode), "exact=True does not extend to visualised runs (render_mode)"
        self.render_mode = render_mode
        self.exact = bool(exact)
        self._last_ended = None  # environments that ended in the last step, per shard (None: after a reset)
        if devices is None:
            devices = list(range(_native.device_count()))
        devices = [int(d) for d in devices]
        assert 1 <= len(devices) <= num_envs, "need between 1 and num_envs devices"
        self.num_envs = num_envs
        self.devices = devices
        self._ranges = split_environments(num_envs, len(devices))
        self._limits = _DeviceShard.ENDS
        self._initializer = _Initializer(self._limits, seed)
        # one thread per shard for the life of the environment: a shard's context is only ever
        # touched from its own thread
        self._threads = [concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix=f"reinfocus-shard{g}")
                         for g in range(len(devices))]
        pixels = frame_height * frame_height
        options = {"jumps": True} if self._JUMPS else {}
        self._shards = []
        try:
            def make_shard(count, device, first):
                # (in the shard's own thread, before its context exists: the thread that will drive the GPU -- and
                # first-touch its pinned staging buffers -- runs on the CPUs of that GPU's NUMA node)
                placement = _native.device_info(device)
                placement["cpus"] = _native.pin_to_numa_node(placement["numa_node"]) if numa_pin else None
                shard = _DeviceShard(count, max_episode_steps, frame_height, samples_per_pixel, device,
                                     first_state_index + first * pixels, **options)
                shard.placement = placement
                return shard

            futures = [thread.submit(make_shard, count, device, first)
                       for thread, device, (first, count) in zip(self._threads, devices, self._ranges)]
            for future in futures:
                try:
                    self._shards.append(future.result())
                except Exception:
                    for thread, other in zip(self._threads, futures):
                        try:  # (a context is only ever touched from its own thread)
                            thread.submit(other.result().ctx.close).result()
                        except Exception:
                            pass
                    raise
        except Exception:
            for thread in self._threads:
                thread.shutdown(wait=True)
            raise
        self._action_set = None if self._JUMPS else self._shards[0].action_set
        _device_spaces(self, self._action_set, num_envs)
        self._visualizer = None
        if render_mode == "rgb_array":  # custom_environments.py:229-238
            both = _ShardSet(self)
            self._visualizer = episode_visualizer.HistoryVisualizer(
                num_envs, TARGET, FOCUS, 1, both, self._limits, ender=both, target_radius=_DeviceShard.TARGET_RADIUS)

    @property
    def placements(self):
        """Per shard: {"device", "pci_bus_id", "numa_node", "cpus"} -- which physical GPU the shard's context is on
        and the CPUs its host thread was restricted to (None: not pinned)."""
        return [dict(shard.placement) for shard in self._shards]

    def _submit(self, function, *per_shard):
        return [thread.submit(function, shard, *(a[g] for a in per_shard))
                for g, (thread, shard) in enumerate(zip(self._threads, self._shards))]

    def _each(self, function, *per_shard):
        """function(shard, *args_g) on every shard's own thread; results in shard order."""
        return [f.result() for f in self._submit(function, *per_shard)]

    @staticmethod
    def _results(futures):
        """Every future's result; all of them are waited for before the first error is raised (no shard is left
        running behind an exception)."""
        results, errors = [], []
        for future in futures:
            try:
                results.append(future.result())
            except Exception as error:  # noqa: BLE001 -- re-raised below
                errors.append(error)
        if errors:
            raise errors[0]
        return results

    def _slices(self, array):
        return [array[first:first + count] for first, count in self._ranges]

    def _locate(self, index):
        for g, (first, count) in enumerate(self._ranges):
            if first <= index < first + count:
                return g, index - first
        raise IndexError(index)

    @property
    def _state(self):
        return np.concatenate(self._each(lambda shard: shard.ctx.env_states()))

    def _no_tensors(self, *args, **kwargs):
        """reset_tensors / step_tensors / device_fault / last_reset_count of the one-device classes."""
        raise ValueError(f"{type(self).__name__} has no *_tensors methods: a tensor lives on one GPU, the shards' rows "
                         "are handed out by one host initializer between the two halves of a step, and the host "
                         "concatenates their results (use a Device* class with device_initializer=True per GPU)")

    reset_tensors = step_tensors = device_fault = last_reset_count = _no_tensors

    def reset(self, *, seed=None, options=None, state=None):
        if seed is not None:
            self._initializer = _Initializer(self._limits, seed)
        initial = (self._initializer.initialize(self.num_envs) if state is None
                   else np.array(state, dtype=np.float32).reshape(self.num_envs, 2))
        observations = np.concatenate(self._each(lambda shard, rows: shard.ctx.env_reset(rows), self._slices(initial)))
        self._last_ended = None
        if self._visualizer is not None:
            self._visualizer.reset(initial, observations)
        return observations, {}

    def _begin(self, actions):
        """First half of the step on every shard -- rf_env_step_plan (transform, enders, ranking: the cut before the
        render that lets the second half run as ONE render launch), in the exact mode rf_env_step_begin (the cut after
        the full render: its row renders happen on other shards).  If any shard fails, the shards whose half did run
        drop it (rf_env_step_abort: they then insist on a reset) and the first error is raised."""
        name = ("env_step_begin" if self.exact else "env_step_plan") + ("_jumps" if self._JUMPS else "")

        def first_half(shard, rows):
            result = getattr(shard.ctx, name)(rows)
            return result if self.exact else (None, None, result)  # (rewards and flags: rf_env_step_run's)

        futures = self._submit(first_half, self._slices(actions))
        results, errors = [], []
        for future in futures:
            try:
                results.append(future.result())
            except Exception as error:  # noqa: BLE001 -- re-raised below
                results.append(None)
                errors.append(error)
        if errors:
            aborts = [thread.submit(shard.ctx.env_step_abort)
                      for thread, shard, result in zip(self._threads, self._shards, results) if result is not None]
            for abort in aborts:
                abort.result()
            raise errors[0]
        return results

    def step(self, actions):
        # every shard validates its slice again, but a bad action must not leave some shards half way
        # through a step: check all of them before any shard begins
        if self._JUMPS:
            actions = jump_actions(actions, self.num_envs)
        else:
            actions = np.asarray(actions).reshape(self.num_envs)
            if actions.size and (actions.min() < 0 or actions.max() >= len(self._action_set)):
                raise AssertionError(f"action outside [0, {len(self._action_set)})")
        pool = self._initializer.propose(self.num_envs)
        firsts = self._begin(actions)
        ended = [k for _, _, k in firsts]
        starts = np.concatenate([[0], np.cumsum(ended)]).astype(int)
        total = int(starts[-1])
        rows = [pool[starts[g]:starts[g] + ended[g]] for g in range(len(self._shards))]
        try:
            if self.exact and total:
                # compacted row r is rendered where environment slot r's RNG states live
                spans = [(first, min(first + count, total)) for first, count in self._ranges]
                renders = [thread.submit(shard.ctx.env_render_states, pool[lo:hi])
                           for thread, shard, (lo, hi) in zip(self._threads, self._shards, spans) if lo < hi]
                focus = np.concatenate(self._results(renders))
                assert len(focus) == total
                values = [focus[starts[g]:starts[g] + ended[g]] for g in range(len(self._shards))]
                observations = self._results(self._submit(lambda shard, r, v: shard.ctx.env_step_end_given(r, v),
                                                          rows, values))
            elif self.exact:
                observations = self._results(self._submit(lambda shard, r: shard.ctx.env_step_end_given(r, np.zeros(0)),
                                                          rows))
            else:
                finished = self._results(self._submit(lambda shard, r: shard.ctx.env_step_run(r), rows))
                observations = [o for o, _, _ in finished]
                firsts = [(r, t, k) for (_, r, t), (_, _, k) in zip(finished, firsts)]
        except Exception:
            # some shard failed in the second half: the others must not keep a half-finished step (those that had
            # finished theirs refuse the abort, which is fine) -- every shard then insists on a reset or was done
            for abort in [thread.submit(shard.ctx.env_step_abort) for thread, shard in zip(self._threads, self._shards)]:
                try:
                    abort.result()
                except Exception:  # noqa: BLE001 -- no open step on that shard
                    pass
            raise
        self._last_ended = ended
        if total:
            self._initializer.initialize(total)  # consume exactly the rows that were used
        observations = np.concatenate(observations)
        rewards = np.concatenate([r for r, _, _ in firsts])
        truncated = np.concatenate([t for _, t, _ in firsts])
        if self._visualizer is not None:  # vector_environment.py:149-156
            state = self._state
            if total:
                self._visualizer.reset(state[truncated], observations[truncated], truncated)
            self._visualizer.step(state[~truncated], observations[~truncated], ~truncated)
        return observations, rewards, np.full(self.num_envs, False), truncated, {}

    def render(self):
        """vector_environment.py:166-176."""
        if self._visualizer is not None:
            return self._visualizer.visualize()
        return None

    def render_frames(self):
        """Only the left halves of render(): the 600 px frames every shard's renderer holds."""
        return _ShardSet(self).render(episode_visualizer.HistoryVisualizer.FRAME)

    def _no_snapshots(self, *args, **kwargs):
        """A sharded environment is several contexts and one host generator whose steps are cut in two: refused."""
        raise ValueError(f"{type(self).__name__} has no snapshots: they are one context's (DeviceVector* on one device)")

    snapshot = restore = snapshot_resident = restore_resident = drop_snapshot = _no_snapshots

    def close(self):
        for thread, shard in zip(self._threads, self._shards):
            thread.submit(shard.ctx.close).result()
        self._shards = []
        for thread in self._threads:
            thread.shutdown(wait=True)
        self._threads = []


class ShardedVectorDiscreteSteps(_ShardedVectorEnv):
    """DeviceVectorDiscreteSteps over several GPUs of one node (see _ShardedVectorEnv)."""


class ShardedVectorContinuousJumps(_ShardedVectorEnv):
    """DeviceVectorContinuousJumps over several GPUs of one node (see _ShardedVectorEnv): float32 actions, handed to
    every shard's slice (rf_env_step_plan_jumps; rf_env_step_begin_jumps in the exact mode); refused as a whole before
    any shard begins when one of them is NaN, infinite or outside [-1, 1]."""

    _JUMPS = True


def composed_actions(transformer, actions, num_envs, index_range=True):
    """The actions of a composed environment's step, checked before any state changes (AssertionError): num_envs
    integer indices in [0, n) for a discrete transformer; num_envs float32 values (also as [num_envs, 1]) for a
    continuous one -- finite, and in [-1, 1] for a ContinuousJumpTransformer (jump_actions); a ContinuousMoveTransformer
    clips finite values, as the reference does.  The device refuses the same (rf_env_configure_composed); the device
    environment leaves the range of discrete indices to it (index_range=False), as DeviceVectorDiscreteSteps does."""
    from reinfocus_amd.environments import state_transformer

    if transformer.kind == state_transformer.CONTINUOUS_JUMP:
        return jump_actions(actions, num_envs)
    if transformer.kind == state_transformer.CONTINUOUS_MOVE:
        actions = np.asarray(actions, dtype=np.float32)
        if actions.shape not in ((num_envs,), (num_envs, 1)):
            raise AssertionError(f"expected {num_envs} actions (shape ({num_envs},) or ({num_envs}, 1)), got {actions.shape}")
        if not np.all(np.isfinite(actions)):
            raise AssertionError("continuous actions must be finite")
        return actions.reshape(num_envs)
    actions = np.asarray(actions)
    if actions.shape not in ((num_envs,), (num_envs, 1)) or not np.issubdtype(actions.dtype, np.integer):
        raise AssertionError(f"expected {num_envs} integer actions, got {actions.dtype} {actions.shape}")
    actions = actions.reshape(num_envs)
    n = transformer.single_action_space.n
    if index_range and actions.size and (actions.min() < 0 or actions.max() >= n):
        raise AssertionError(f"action outside [0, {n})")
    return actions


class VectorEnvironment(_ViewedTwin, _VectorEnvBase):
    """A vector environment composed of the reference's strategy objects (vector_environment.py:19-176): an ender, an
    initializer, a rewarder and a transformer from environments/episode_ender.py, state_initializer.py,
    episode_rewarder.py and state_transformer.py, around the observer both tasks use --
    NormalizedObserver(DeltaObserver([IndexedElementObserver(1), FocusObserver], True, [max_focus_move, nan])) over
    states [target, focus plane] in `ends`.  The host twin: numpy glue around the GPU render and focus measure, in the
    reference's call order, same-step auto-reset included.  observer= replaces that observer by any tree of the observer
    classes (environments/state_observer.py) around one FocusObserver: the environment then renders with that
    FocusObserver's renderer at its frame height (frame_height / samples_per_pixel / device must be left at their
    defaults or agree), its spaces are the tree's, `ends` and `max_focus_move` only describe the visualiser's range, and
    focus_observation_index names the observation column the visualiser plots.  Rewards are returned as float64.
    Actions are checked before any state changes (composed_actions).  `reset(seed=...)` reseeds the initializer; `state=` (extension) pins the
    initial states.  DeviceVectorEnvironment is the same environment with the whole step on the GPU."""

    metadata = {"render_modes": ["rgb_array"], "render_fps": 4}
    _records = None  # (as _HostGlue's)

    def __init__(self, ender, initializer, rewarder, transformer, num_envs, ends=(5.0, 10.0), max_focus_move=5.0,
                 render_mode=None, *, frame_height=300, samples_per_pixel=100, device=None, observer=None,
                 focus_observation_index=1, episode_records=False, learner_view=None):
        super().__init__()
        assert render_mode is None or render_mode in self.metadata["render_modes"]
        self.render_mode = render_mode
        self.num_envs = num_envs
        self._records = _EpisodeRecords(num_envs) if episode_records else None  # (as _HostGlue's)
        self._ender = ender
        self._initializer = initializer
        self._rewarder = rewarder
        self._transformer = transformer
        if observer is None:
            self._renderer = render.FastRenderer(samples_per_pixel=samples_per_pixel, device=device)
            self._focus_observer = state_observer.FocusObserver(num_envs, TARGET, FOCUS, ends, self._renderer,
                                                                frame_height)
            self._observer = _Observer(num_envs, ends, max_focus_move, self._focus_observer)
        else:
            assert observer.observation_space.shape[0] == num_envs, \
                f"the observer has num_envs {observer.observation_space.shape[0]}, not {num_envs}"
            self._focus_observer, self._renderer, _, _ = _described_renderer(observer, frame_height, samples_per_pixel,
                                                                             device)
            self._observer = observer
        focus_observation_index = _checked_focus_index(focus_observation_index, self._observer.single_observation_space)
        self._visualizer = episode_visualizer.HistoryVisualizer(num_envs, TARGET, FOCUS, focus_observation_index,
                                                                self._renderer, ends, ender=ender)
        self.single_action_space = transformer.single_action_space
        self.action_space = transformer.action_space
        self.single_observation_space = self._observer.single_observation_space
        self.observation_space = self._observer.observation_space
        self._configure_view(learner_view)  # (as _HostGlue's)
        self._state = None

    def reset(self, *, seed=None, options=None, state=None):
        if seed is not None:
            self._initializer.seed(seed)
        self._state = (self._initializer.initialize(self.num_envs) if state is None
                       else np.array(state, dtype=np.float32).reshape(self.num_envs, 2))
        self._ender.reset(self._state)
        observations = self._observer.reset(self._state, None)
        self._rewarder.reset(self._state, observations)
        if self._records is not None:
            self._records.reset()
        if self.render_mode == "rgb_array":
            self._visualizer.reset(self._state, observations)
        return self._viewed_reset(observations, {})

    def step(self, actions):
        assert self._state is not None
        actions = composed_actions(self._transformer, actions, self.num_envs)
        self._state = self._transformer.transform(self._state, actions)
        self._ender.step(self._state)
        observations = self._observer.observe(self._state)
        rewards = self._rewarder.reward(self._state, observations)
        terminated = self._ender.is_terminated()
        truncated = self._ender.is_truncated()
        done = terminated | truncated
        rewards = np.asarray(rewards, dtype=np.float64)
        info = {} if self._records is None else self._records.step(observations, rewards, done)
        if done.any():
            new_state = self._initializer.initialize(done.sum())
            self._state[done] = new_state
            self._ender.reset(new_state, done)
            new_observations = self._observer.reset(new_state, done)
            observations[done] = new_observations
            self._rewarder.reset(new_state, new_observations, done)
            if self.render_mode == "rgb_array":
                self._visualizer.reset(new_state, new_observations, done)
        if self.render_mode == "rgb_array":
            not_done = ~done
            self._visualizer.step(self._state[not_done], observations[not_done], not_done)
        return self._viewed_step(observations, rewards, terminated, truncated, info)

    episode_accumulators = _HostGlue.episode_accumulators

    def strategy_state(self):
        """The per-leaf strategy state, laid out as DeviceVectorEnvironment.strategy_state returns it."""
        from reinfocus_amd.environments import strategy_program

        return strategy_program.host_strategy_state(self._ender, self._rewarder, self.num_envs)

    def observer_state(self):
        """The DeltaObservers' old values of an environment given an observer, float32[rows, n], laid out as
        DeviceVectorEnvironment.observer_state returns them."""
        from reinfocus_amd.environments import strategy_program

        assert not isinstance(self._observer, _Observer), "the environment was not given an observer"
        return strategy_program.host_observer_state(self._observer, self.num_envs)

    def status(self, index):
        return self._ender.status(index)

    def render(self):
        if self.render_mode == "rgb_array":
            return self._visualizer.visualize()
        return None

    def render_frames(self):
        return np.asarray(self._renderer.render(600))

    def close(self):
        self._renderer.close()


class DeviceVectorEnvironment(_DeviceVectorEnv):
    """VectorEnvironment with the whole step resident on the GPU (rf_env_configure_composed): the strategy objects are
    compiled into a device program (strategy_program.compile_program: AssertionError for anything the device cannot
    run) that every schedule of the DiscreteSteps step interprets; reset / step results equal VectorEnvironment's bit
    for bit, with the same initializer consumption (propose, then initialize the rows that were used).  The strategy
    objects only describe the environment here: their own state is not advanced (strategy_state() and status() read
    the device's).  Discrete transformers step through the int32 calls, continuous ones through the float32 ones.
    observer= and focus_observation_index= as VectorEnvironment's: the tree is compiled too
    (strategy_program.compile_observer, rf_env_configure_observed) and only describes the environment -- frame height,
    samples per pixel and device are those of its FocusObserver and that observer's renderer, which is never asked to
    render; observer_state() reads the device.  One device only: `devices=` (sharding) is refused.
    device_initializer=True: the initializer, a RangedInitializer of two elements, is compiled too
    (strategy_program.compile_initializer) and, like the other strategy objects, only describes the environment: the
    device draws the reset states and advances its own copy of the generator (initializer_state()); see
    _DeviceVectorEnv."""

    def __init__(self, ender, initializer, rewarder, transformer, num_envs, ends=(5.0, 10.0), max_focus_move=5.0,
                 render_mode=None, *, frame_height=300, samples_per_pixel=100, device=None, first_state_index=0,
                 devices=None, observer=None, focus_observation_index=1, device_initializer=False,
                 episode_records=False, learner_view=None):
        from reinfocus_amd.environments import state_transformer, strategy_program

        if devices is not None:
            raise ValueError("DeviceVectorEnvironment runs on one device (device=); a composed environment cannot be "
                             "sharded over several (devices=)" +
                             (", and episode records (episode_records=) are one context's" if episode_records else ""))
        _VectorEnvBase.__init__(self)
        assert render_mode is None or render_mode in self.metadata["render_modes"]
        observer_program = None
        if observer is None:
            program = strategy_program.compile_program(transformer, ender, rewarder, num_envs)
            single_observation_space = spaces.Box(-np.ones(4, dtype=np.float32), np.ones(4, dtype=np.float32),
                                                  dtype=np.float32)
        else:
            program, observer_program = strategy_program.compile_program(transformer, ender, rewarder, num_envs, observer)
            _, described, frame_height, samples_per_pixel = _described_renderer(observer, frame_height,
                                                                                samples_per_pixel, device)
            device = described._ctx.device
            single_observation_space = observer.single_observation_space
        focus_observation_index = _checked_focus_index(focus_observation_index, single_observation_space)
        self._observed = observer is not None
        self.render_mode = render_mode
        self.num_envs = num_envs
        self._ender = ender
        self._transformer = transformer
        self._discrete = transformer.kind in (state_transformer.DISCRETE_JUMP, state_transformer.DISCRETE_MOVE)
        self._shard = _DeviceShard(num_envs, None, frame_height, samples_per_pixel, device, first_state_index,
                                   program=program, ends=ends, max_move=max_focus_move,
                                   observer_program=observer_program)
        self._ctx = self._shard.ctx
        self._limits = tuple(ends)
        self._initializer = initializer
        self._device_initializer = bool(device_initializer)
        self._configure_initializer()
        self._configure_records(episode_records)
        self.single_action_space = transformer.single_action_space
        self.action_space = transformer.action_space
        self.single_observation_space = single_observation_space
        self.observation_space = spaces.batch_space(self.single_observation_space, num_envs)
        self._configure_view(learner_view)
        self._visualizer = None
        if render_mode == "rgb_array":
            self._visualizer = episode_visualizer.HistoryVisualizer(num_envs, TARGET, FOCUS, focus_observation_index,
                                                                    self._shard, self._limits, ender=self)

    def strategy_state(self):
        """(counters int32[n_enders, n], floats float32[n_enders, n], StoppedEnder histories float32[rows, n], old
        values float32[n_rewarders, n]) from the device (rf_env_get_strategy_state)."""
        return self._ctx.env_strategy_state()

    def observer_state(self):
        """The DeltaObservers' old values float32[rows, n], node-major in evaluation order, from the device
        (rf_env_get_observer_state)."""
        assert self._observed, "the environment was not given an observer"
        return self._ctx.env_observer_state()

    def status(self, index):
        """ender.status(index) from the device's strategy state."""
        from reinfocus_amd.environments import strategy_program

        return strategy_program.device_status(self._ender, self.strategy_state(), index)

    def _reseed(self, seed):
        self._initializer.seed(seed)

    def _checked(self, actions):
        return composed_actions(self._transformer, actions, self.num_envs, index_range=False)

    def _float_actions(self):
        return not self._discrete


from reinfocus_amd.environments.rollout import DeviceRollout, Rollout  # noqa: E402,F401 -- the PPO rollout buffers
from reinfocus_amd.environments.policy import DevicePolicy, MlpPolicySpec, Policy, policy_numpy  # noqa: E402,F401 -- the PPO actor-critic
from reinfocus_amd.environments.learner import DeviceLearner, Learner, ppo_update_numpy  # noqa: E402,F401 -- the PPO minibatch update
from reinfocus_amd.environments.population import DevicePopulationLearner, DevicePopulationPolicy, PopulationLearner, PopulationPolicy  # noqa: E402,F401 -- G learners in lock-step
from reinfocus_amd.environments.population import DeviceSdePopulationPolicy, SdePopulationPolicy  # noqa: E402,F401 -- G gSDE learners in lock-step
from reinfocus_amd.environments.population import DevicePopulationLstmPolicy, LstmPopulationPolicy  # noqa: E402,F401 -- G recurrent learners in lock-step
from reinfocus_amd.environments.population import DevicePopulationLstmSdePolicy, LstmSdePopulationPolicy  # noqa: E402,F401 -- G recurrent gSDE learners in lock-step
from reinfocus_amd.environments.sde import DeviceSdePolicy, SdePolicy, SdePolicySpec, sde_numpy  # noqa: E402,F401 -- the gSDE actor-critic
from reinfocus_amd.environments.lstm import DeviceLstmPolicy, LstmPolicy, LstmPolicySpec, lstm_numpy  # noqa: E402,F401 -- the recurrent actor-critic
from reinfocus_amd.environments.lstm_learner import DeviceLstmLearner, LstmLearner, lstm_gradient_numpy, lstm_update_numpy  # noqa: E402,F401 -- the recurrent PPO minibatch update
from reinfocus_amd.environments.lstm_sde import DeviceLstmSdePolicy, LstmSdePolicy, LstmSdePolicySpec, lstm_sde_numpy  # noqa: E402,F401 -- its Gaussian (gSDE) head
from reinfocus_amd.environments.param_init import init_numpy, segments  # noqa: E402,F401 -- the parameter initialisation (init_parameters of the policy classes)
from reinfocus_amd.environments.evaluation import DeviceEvaluation, Evaluation  # noqa: E402,F401 -- per-group evaluation scores, the best parameters kept
