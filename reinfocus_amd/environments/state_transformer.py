"""State transformers: how an action moves a batch of states (reference: environments/state_transformer.py).

Same class names, constructor arguments and numpy arithmetic as the reference; states are float32[num_envs, n].  Every
expression mixes float32 arrays with scalar parameters, which the constructors pass through scalars.parameter (and
ContinuousJumpTransformer's span through scalars.difference), so it computes what numpy 1.26, the reference's numpy,
computes under any numpy, numpy.float64 parameters included.  Action sets are arrays and stay as given.  harness.VectorEnvironment drives them on the host; rf_env_configure_composed runs the same arithmetic on
the GPU (csrc/rf_env.h, composed task).

`kind` names the transformer for the device program (rf_env_program.transformer).
"""

import numpy as np

from reinfocus_amd.environments import scalars
from reinfocus_amd.environments import spaces

CONTINUOUS_JUMP, CONTINUOUS_MOVE, DISCRETE_JUMP, DISCRETE_MOVE = 0, 1, 2, 3


def _limits(limits):
    """(low, high) as scalars.parameter makes them: a tuple, whatever sequence or array they came in."""
    return tuple(scalars.parameter(x, "limits") for x in limits)


class StateTransformer:
    """The base of every transformer: the action spaces, single and batched."""

    kind = None

    def __init__(self, num_envs, single_action_space):
        self.num_envs = num_envs
        self.single_action_space = single_action_space
        self.action_space = spaces.batch_space(single_action_space, num_envs)

    def transform(self, states, actions):
        raise NotImplementedError


class ContinuousJumpTransformer(StateTransformer):
    """Element `move_index` jumps to the point of `limits` proportional to the action in [-1, 1], unless that point is
    no farther than stop_threshold from where it is.  No clip."""

    kind = CONTINUOUS_JUMP

    def __init__(self, num_envs, move_index, limits, stop_threshold=0.1):
        super().__init__(num_envs, spaces.Box(-1, 1, dtype=np.float32))
        self._limits = _limits(limits)
        self._move_index = move_index
        self._stop_threshold = abs(scalars.parameter(stop_threshold, "stop_threshold"))

    def transform(self, states, actions):
        new_states = states.copy()
        actions = (actions.flatten() + 1) / 2.0
        moved_states = actions * scalars.difference(self._limits[1], self._limits[0], "limits") + self._limits[0]
        moved = abs(new_states[:, self._move_index] - moved_states) > self._stop_threshold
        new_states[moved, self._move_index] = moved_states[moved]
        return new_states


class ContinuousMoveTransformer(StateTransformer):
    """Element `move_index` moves by speed times the action (clipped to [-1, 1]) where that move is longer than
    stop_threshold; every element is then clipped to `limits`."""

    kind = CONTINUOUS_MOVE

    def __init__(self, num_envs, move_index, limits, speed, stop_threshold=0.1):
        super().__init__(num_envs, spaces.Box(-1, 1, dtype=np.float32))
        self._limits = _limits(limits)
        self._move_index = move_index
        self._speed = scalars.parameter(speed, "ContinuousMoveTransformer speed")
        self._stop_threshold = abs(scalars.parameter(stop_threshold, "stop_threshold"))

    def transform(self, states, actions):
        new_states = states.copy()
        actions = np.clip(actions.flatten(), -1, 1) * self._speed
        new_states[:, self._move_index] += (abs(actions) > self._stop_threshold) * actions
        return np.clip(new_states, *self._limits)


class DiscreteJumpTransformer(StateTransformer):
    """Element `move_index` jumps to the action's entry of a float32 action set; every element is then clipped to
    `limits`."""

    kind = DISCRETE_JUMP

    def __init__(self, num_envs, move_index, limits, action_set):
        super().__init__(num_envs, spaces.Discrete(len(action_set)))
        self._limits = _limits(limits)
        self._move_index = move_index
        self._action_set = np.asarray(action_set, dtype=np.float32)

    def transform(self, states, actions):
        new_states = states.copy()
        new_states[:, self._move_index] = self._action_set[actions.flatten()]
        return np.clip(new_states, *self._limits)


class DiscreteMoveTransformer(StateTransformer):
    """Element `move_index` moves by the action's entry of the action set (float64 for Python floats: the float32
    state is added to in float64 and rounded back); every element is then clipped to `limits`."""

    kind = DISCRETE_MOVE

    def __init__(self, num_envs, move_index, limits, action_set):
        super().__init__(num_envs, spaces.Discrete(len(action_set)))
        self._limits = _limits(limits)
        self._move_index = move_index
        self._action_set = np.asarray(action_set)

    def transform(self, states, actions):
        new_states = states.copy()
        new_states[:, self._move_index] += self._action_set[actions.flatten()]
        return np.clip(new_states, *self._limits)
