"""Episode rewarders: the reward of a step (reference: environments/episode_rewarder.py).

Same class names, constructor arguments and numpy arithmetic as the reference.  Rewarders combine with `+` and `*`
into an OpRewarder.  Scalar parameters pass through scalars.parameter (on - off and high - low through
scalars.difference), so every term computes what numpy 1.26, the reference's numpy, computes under any numpy.  `dtype`
is a term's result dtype, evaluated by numpy itself.  With Python-number or numpy.float64 parameters it is fixed per
class: DeltaRewarder, DistanceRewarder and ObservationRewarder float32 (float32 arrays with scalars), OnTargetRewarder
and StoppedRewarder float64 (a bool array times a float64 scalar); with numpy.float32 on and off (OnTargetRewarder) or
reward (StoppedRewarder) those two are float32, as numpy 1.26 has them.  An OpRewarder's is the numpy promotion of its
two operands.  harness.VectorEnvironment drives them on the host; rf_env_configure_composed runs the same arithmetic on the
GPU, a float32 node in float32.

`kind` names a leaf for the device program (rf_env_program.rewarders).
"""

import numpy as np

from reinfocus_amd.environments import scalars

DELTA, DISTANCE, OBSERVATION, ON_TARGET, STOPPED = 0, 1, 2, 3, 4
ADD, MUL = -1, -2  # postfix operations of rf_env_program.reward_ops
_PROBE = np.zeros((1, 4), dtype=np.float32)  # (what `dtype` evaluates a term's expression on)


class BaseRewarder:
    """A rewarder that combines with `+` / `*` (numpy.add / numpy.multiply of the children's rewards)."""

    kind = None

    def __add__(self, other):
        return OpRewarder(self, other, np.add)

    def __mul__(self, other):
        return OpRewarder(self, other, np.multiply)

    def reset(self, states, observations, indices=None):
        pass


class _OldStateRewarder(BaseRewarder):
    """The reference's bookkeeping of one state element's previous value: a full reset keeps a view of the states'
    column, a partial one writes the selected rows."""

    def reset(self, states, observations, indices=None):
        if self._old_states is not None and indices is not None:
            self._old_states[indices] = states[:, self._check_index]
        else:
            self._old_states = states[:, self._check_index]


class DeltaRewarder(_OldStateRewarder):
    """`reward` per `scale` that the element `check_index` moved since the last step."""

    kind = DELTA

    def __init__(self, check_index, scale, reward=-1.0):
        self._check_index = check_index
        self._scale = scalars.parameter(scale, "DeltaRewarder scale")
        self._reward = scalars.parameter(reward, "DeltaRewarder reward")
        self._old_states = None

    @property
    def dtype(self):
        return (abs(_PROBE[:, 0]) * self._reward / self._scale).dtype

    def reward(self, states, observations):
        assert self._old_states is not None
        reward = abs(states[:, self._check_index] - self._old_states) * self._reward / self._scale
        self._old_states = states[:, self._check_index]
        return reward


class DistanceRewarder(BaseRewarder):
    """`high` where two elements coincide, `low` where they are `span` apart, linear in their distance."""

    kind = DISTANCE

    def __init__(self, check_indices, span, low=-1.0, high=0.0):
        self._check_indices = check_indices
        self._span = scalars.parameter(span, "DistanceRewarder span")
        self._low = scalars.parameter(low, "DistanceRewarder low")
        self._high = scalars.parameter(high, "DistanceRewarder high")
        self._width = scalars.difference(self._high, self._low, "DistanceRewarder high - low")

    @property
    def dtype(self):
        return ((1 - _PROBE[:, 0] / self._span) * self._width + self._low).dtype

    def reward(self, states, observations):
        distance = abs(states[:, self._check_indices[0]] - states[:, self._check_indices[1]])
        return (1 - distance / self._span) * self._width + self._low


class ObservationRewarder(BaseRewarder):
    """One element of the observation."""

    kind = OBSERVATION
    dtype = np.dtype(np.float32)

    def __init__(self, reward_observation_index):
        self._reward_observation_index = reward_observation_index

    def reward(self, states, observations):
        return observations[:, self._reward_observation_index]


class OnTargetRewarder(BaseRewarder):
    """`on` where two elements are closer than `span`, `off` elsewhere."""

    kind = ON_TARGET

    def __init__(self, check_indices, span, off=0.0, on=1.0):
        self._check_indices = check_indices
        self._span = scalars.parameter(span, "OnTargetRewarder span")
        self._off = scalars.parameter(off, "OnTargetRewarder off")
        self._delta = scalars.difference(scalars.parameter(on, "OnTargetRewarder on"), self._off, "OnTargetRewarder on - off")

    @property
    def dtype(self):
        return ((_PROBE[:, 0] < 1) * self._delta + self._off).dtype

    def reward(self, states, observations):
        close = abs(states[:, self._check_indices[0]] - states[:, self._check_indices[1]]) < self._span
        return close * self._delta + self._off


class StoppedRewarder(_OldStateRewarder):
    """`reward` where the element `check_index` moved less than `threshold` since the last step."""

    kind = STOPPED

    def __init__(self, check_index, threshold, reward=1.0):
        self._check_index = check_index
        self._threshold = abs(scalars.parameter(threshold, "StoppedRewarder threshold"))
        self._reward = scalars.parameter(reward, "StoppedRewarder reward")
        self._old_states = None

    @property
    def dtype(self):
        return ((_PROBE[:, 0] < 1) * self._reward).dtype

    def reward(self, states, observations):
        assert self._old_states is not None
        reward = (abs(states[:, self._check_index] - self._old_states) < self._threshold) * self._reward
        self._old_states = states[:, self._check_index]
        return reward


class OpRewarder(BaseRewarder):
    """Combines the rewards of two rewarders with `op` (numpy.add or numpy.multiply)."""

    def __init__(self, l_rewarder, r_rewarder, op):
        self._l_rewarder = l_rewarder
        self._r_rewarder = r_rewarder
        self._op = op

    @property
    def dtype(self):
        return np.promote_types(self._l_rewarder.dtype, self._r_rewarder.dtype)

    def reset(self, states, observations, indices=None):
        self._l_rewarder.reset(states, observations, indices)
        self._r_rewarder.reset(states, observations, indices)

    def reward(self, states, observations):
        return self._op(self._l_rewarder.reward(states, observations), self._r_rewarder.reward(states, observations))
