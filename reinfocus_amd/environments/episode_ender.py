"""Episode enders: when episodes end (reference: environments/episode_ender.py).

Same class names, constructor arguments, numpy arithmetic and status strings as the reference.  Enders combine with
`|` and `&` into an OpEnder.  No ender of the reference ever terminates an episode; they truncate it, from the states
alone (never from observations) -- which is what lets the device step decide which environments end before it renders
(csrc/rf_env.h).  harness.VectorEnvironment drives them on the host; rf_env_configure_composed runs the same rules on
the GPU.

Thresholds, radii and spans pass through scalars.parameter, so the float32 comparisons are numpy 1.26's (the
reference's numpy) under any numpy, numpy.float64 parameters included.

`kind` names a leaf for the device program (rf_env_program.enders).
"""

import warnings

import numpy as np

from reinfocus_amd import histories
from reinfocus_amd.environments import scalars

DIVERGING, ENDLESS, ON_TARGET, STOPPED, TIME_LIMIT = 0, 1, 2, 3, 4
OR, AND = -1, -2  # postfix operations of rf_env_program.ender_ops


class BaseEnder:
    """An ender that combines with `|` / `&` (numpy.bitwise_or / numpy.bitwise_and of the children's flags)."""

    kind = None

    def __and__(self, other):
        return OpEnder(self, other, np.bitwise_and)

    def __or__(self, other):
        return OpEnder(self, other, np.bitwise_or)

    def is_terminated(self):
        return np.full(self._num_envs, False)

    def reset(self, states, indices=None):
        pass

    def step(self, states):
        pass

    def status(self, index):
        return ""


class DivergingEnder(BaseEnder):
    """Truncates once the distance between two state elements has grown by more than `threshold` in
    `early_end_steps` (not necessarily consecutive) steps."""

    kind = DIVERGING

    def __init__(self, num_envs, check_indices, threshold, early_end_steps=10):
        self._num_envs = num_envs
        self._check_indices = check_indices
        self._threshold = scalars.parameter(threshold, "DivergingEnder threshold")
        self._early_end_steps = early_end_steps
        self._diverging_steps = np.zeros(num_envs, dtype=np.int32)
        self._last_diff = np.zeros(num_envs, dtype=np.float32)

    def _diff(self, states):
        return abs(states[:, self._check_indices[0]] - states[:, self._check_indices[1]])

    def step(self, states):
        diff = self._diff(states)
        self._diverging_steps[diff > self._last_diff + self._threshold] += 1
        self._last_diff = diff

    def is_truncated(self):
        return self._diverging_steps >= self._early_end_steps

    def reset(self, states, indices=None):
        if indices is None:
            indices = np.full(self._num_envs, True)
        diff = self._diff(states)
        self._diverging_steps[indices] = 0
        self._last_diff[indices] = diff

    def status(self, index):
        diverging = self._diverging_steps[index]
        return f"diverging {diverging} / {self._early_end_steps}" if diverging > 0 else ""


class EndlessEnder(BaseEnder):
    """Never ends an episode."""

    kind = ENDLESS

    def __init__(self, num_envs):
        self._num_envs = num_envs

    def is_truncated(self):
        return np.full(self._num_envs, False)


class OnTargetEnder(BaseEnder):
    """Truncates once two state elements have been closer than `early_end_radius` for `early_end_steps` consecutive
    steps."""

    kind = ON_TARGET

    def __init__(self, num_envs, check_indices, early_end_radius, early_end_steps=10):
        self._num_envs = num_envs
        self._check_indices = check_indices
        self._radius = scalars.parameter(early_end_radius, "OnTargetEnder early_end_radius")
        self._early_end_steps = early_end_steps
        self._on_target_steps = np.zeros(num_envs, dtype=np.int32)

    def step(self, states):
        on_targets = abs(states[:, self._check_indices[0]] - states[:, self._check_indices[1]]) < self._radius
        self._on_target_steps[on_targets] += 1
        self._on_target_steps[np.invert(on_targets)] = 0

    def is_truncated(self):
        return self._on_target_steps >= self._early_end_steps

    def reset(self, states, indices=None):
        if indices is None:
            indices = np.full(self._num_envs, True)
        self._on_target_steps[indices] = 0

    def status(self, index):
        on_step = self._on_target_steps[index]
        return f"on target {on_step} / {self._early_end_steps}" if on_step > 0 else ""


class StoppedEnder(BaseEnder):
    """Truncates once one state element has stayed within a span narrower than `early_end_span` over its last
    early_end_steps + 1 values (a NaN-padded float32 history; an episode's first state is its first value)."""

    kind = STOPPED

    def __init__(self, num_envs, check_index, early_end_span, early_end_steps=10):
        self._num_envs = num_envs
        self._check_index = check_index
        self._early_end_span = scalars.parameter(early_end_span, "StoppedEnder early_end_span")
        self._early_end_steps = early_end_steps
        self._moves = histories.Histories(num_envs, early_end_steps + 1)

    def step(self, states):
        self._moves.append_events(states[:, self._check_index])

    def is_truncated(self):
        data = self._moves.data
        with warnings.catch_warnings():  # (all-NaN rows warn; the NaN test below rules them out)
            warnings.simplefilter("ignore", RuntimeWarning)
            span = abs(np.nanmax(data, 1) - np.nanmin(data, 1))
        return (span < self._early_end_span) & ~np.any(np.isnan(data), 1)

    def reset(self, states, indices=None):
        if indices is None:
            indices = np.full(self._num_envs, True)
        self._moves.reset(indices)
        self._moves.append_events(states[:, self._check_index], indices)

    def status(self, index):
        return stopped_status(self._moves.data[index], self._early_end_steps, self._early_end_span)


def stopped_status(moves, early_end_steps, early_end_span):
    """StoppedEnder.status from one environment's history (oldest first): how many of the latest steps the element
    has stayed within the span.  Shared with the device environment, which reads the history back."""
    top = bottom = moves[-1]
    for i, move in enumerate(moves[early_end_steps - 1::-1]):
        if np.isnan(move):
            return _stopped_message(i, early_end_steps)
        if move < bottom:
            bottom = move
        elif move > top:
            top = move
        if top - bottom > early_end_span:
            return _stopped_message(i, early_end_steps)
    return _stopped_message(early_end_steps, early_end_steps)


def _stopped_message(n_stopped, early_end_steps):
    return f"stopped {n_stopped} / {early_end_steps}" if n_stopped else ""


class TimeLimitEnder(BaseEnder):
    """Truncates after `max_steps` steps."""

    kind = TIME_LIMIT

    def __init__(self, num_envs, max_steps):
        self._num_envs = num_envs
        self._max_steps = max_steps
        self._steps = np.zeros(num_envs, dtype=np.int32)

    def step(self, states):
        self._steps += 1

    def is_truncated(self):
        return self._steps >= self._max_steps

    def reset(self, states, indices=None):
        if indices is None:
            indices = np.full(self._num_envs, True)
        self._steps[indices] = 0

    def status(self, index):
        return f"step {self._steps[index]} / {self._max_steps}"


class OpEnder(BaseEnder):
    """Combines the flags of two enders with `op` (numpy.bitwise_or or numpy.bitwise_and)."""

    def __init__(self, l_ender, r_ender, op):
        self._l_ender = l_ender
        self._r_ender = r_ender
        self._op = op

    def step(self, states):
        self._l_ender.step(states)
        self._r_ender.step(states)

    def is_terminated(self):
        return self._op(self._l_ender.is_terminated(), self._r_ender.is_terminated())

    def is_truncated(self):
        return self._op(self._l_ender.is_truncated(), self._r_ender.is_truncated())

    def reset(self, states, indices=None):
        self._l_ender.reset(states, indices)
        self._r_ender.reset(states, indices)

    def status(self, index):
        l_status = self._l_ender.status(index)
        r_status = self._r_ender.status(index)
        return l_status + (", " if l_status and r_status else "") + r_status
