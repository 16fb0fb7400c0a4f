"""The observer strategy classes; FocusObserver is the caller of the render-and-measure hot path.

Mirrors reinfocus/environments/state_observer.py:62-97 (BaseObserver), :100-164 (WrapperObserver), :167-292
(DeltaObserver), :295-320 (cached_focus_extrema), :323-383 (FocusObserver), :386-421 (IndexedElementObserver) and
:424-517 (NormalizedObserver): same constructor arguments and defaults, same spaces, same observe / reset semantics
and return shapes, float32 arithmetic operation by operation.  The render and the focus measure of FocusObserver run on
the GPU; only 8 bytes per environment come back to the host.  harness.VectorEnvironment(observer=...) drives a tree of
them on the host, harness.DeviceVectorEnvironment(observer=...) compiles it into the device-resident step
(strategy_program.compile_observer; `kind` is what the compiler knows a class by).
"""

import functools

import numpy as np

from reinfocus_amd import vision
from reinfocus_amd.environments import spaces
from reinfocus_amd.graphics import render


INDEXED_ELEMENT, FOCUS, DELTA, NORMALIZED = range(4)  # RF_OBS_* (include/reinfocus_hip.h)


class BaseObserver:
    """A state observer that produces observations within some range
    (state_observer.py:57-97)."""

    kind = None  # the classes the device program compiler knows set theirs

    def __init__(self, num_envs, min_obs, max_obs):
        self.single_observation_space = spaces.Box(min_obs, max_obs, dtype=np.float32)
        self.observation_space = spaces.batch_space(self.single_observation_space, num_envs)

    def observe(self, states, indices=None):
        raise NotImplementedError

    def reset(self, states, indices=None):
        if indices is None:
            indices = np.full(self.observation_space.shape[0], True)
        return self.observe(states, indices)


@functools.lru_cache(maxsize=None)
def _focus_extrema(ends, frame_height, samples_per_pixel, device):
    max_targets = np.linspace(*ends, 11)
    renderer = render.FastRenderer(samples_per_pixel=samples_per_pixel, device=device)
    try:
        renderer.update_targets(np.append(ends, max_targets))
        renderer.update_focus_planes(np.append(ends[::-1], max_targets))
        focus_values = vision.focus_values(renderer.render(frame_height))
    finally:
        renderer.close()  # the fresh renderer of state_observer.py:314 is garbage afterwards
    return min(focus_values[0:2]), max(focus_values[2:13])


def cached_focus_extrema(ends, frame_height, samples_per_pixel=100, device=None):
    """state_observer.py:295-320: the least focus (target and focus plane at opposite
    ends) and the greatest (both at the same place, 11 places), from one render of 13
    environments by a FRESH FastRenderer (seed-0 states), cached per argument set.
    samples_per_pixel is an extension (the reference always uses FastRenderer()'s 100)."""
    return _focus_extrema((float(ends[0]), float(ends[1])), int(frame_height), int(samples_per_pixel), device)


class FocusObserver(BaseObserver):
    """Observes the focus value of each environment's rendered scene
    (state_observer.py:323-383)."""

    kind = FOCUS

    def __init__(self, num_envs, target_index, focus_plane_index, ends, renderer, frame_height=300):
        min_focus, max_focus = cached_focus_extrema(
            ends, frame_height, renderer._samples_per_pixel, renderer._ctx.device
        )
        super().__init__(num_envs, min_focus, max_focus)
        self._target_index = target_index
        self._focus_plane_index = focus_plane_index
        self._renderer = renderer
        self._frame_height = frame_height

    def observe(self, states, indices=None):
        """state_observer.py:359-383: every row of `states` is rendered and scored;
        `indices` only sizes the result (k = indices.sum() rows on a partial reset)."""
        if indices is None:
            indices = np.full(self.observation_space.shape[0], True)
        self._renderer.update_targets(states[:, self._target_index])
        self._renderer.update_focus_planes(states[:, self._focus_plane_index])
        return np.reshape(
            vision.focus_values(self._renderer.render(self._frame_height)),
            (indices.sum(), self.observation_space.shape[1]),
        )


def _sequence(observers):
    return list(observers) if isinstance(observers, (list, tuple)) else [observers]


def _stacked(observers, bound):
    """The wrapped observers' low or high bounds side by side, float32."""
    return np.hstack([getattr(observer.single_observation_space, bound) for observer in observers], dtype=np.float32)


class WrapperObserver(BaseObserver):
    """Produces observations from those of other observers (state_observer.py:100-164).  Not an observer by
    itself: DeltaObserver and NormalizedObserver say what becomes of the stacked observations."""

    def __init__(self, observers, min_obs, max_obs):
        num_envs = {observer.observation_space.shape[0] for observer in observers}
        assert len(num_envs) == 1, "Appended observers must have the same number of environments"
        super().__init__(num_envs.pop(), min_obs, max_obs)
        self._observers = observers

    def reset(self, states, indices=None):
        """Resets every wrapped observer; their reset observations side by side."""
        return np.hstack([observer.reset(states, indices) for observer in self._observers], dtype=np.float32)

    def wrapped_observations(self, states, indices=None):
        """The wrapped observers' observations side by side, in the constructor's order."""
        return np.hstack([observer.observe(states, indices) for observer in self._observers], dtype=np.float32)


class DeltaObserver(WrapperObserver):
    """Observes the change of the wrapped observations since the last call, optionally after the observations
    themselves (state_observer.py:167-292).  max_change: None (a change is bounded by high - low of what it is a
    change of), a number for every element, or an array whose non-finite entries fall back to high - low."""

    kind = DELTA

    def __init__(self, observers, include_original=False, max_change=None):
        from reinfocus_amd.environments import harness  # (harness imports this module)

        observers = _sequence(observers)
        lows, highs = _stacked(observers, "low"), _stacked(observers, "high")
        if max_change is not None and np.ndim(max_change) == 0:
            max_change = np.full(len(lows), max_change, dtype=np.float32)
        low, high = harness.delta_bounds(lows, highs, max_change, include_original)
        super().__init__(observers, low, high)
        self._include_original = include_original
        self._old_wrapped_observations = np.full((self.observation_space.shape[0], len(lows)), np.nan, dtype=np.float32)

    def _all(self, indices):
        return np.full(self.observation_space.shape[0], True) if indices is None else indices

    def _with_original(self, wrapped, deltas):
        return np.hstack([wrapped, deltas], dtype=np.float32) if self._include_original else deltas

    def observe(self, states, indices=None):
        indices = self._all(indices)
        wrapped = self.wrapped_observations(states, indices)
        deltas = wrapped - self._old_wrapped_observations[indices]
        self._old_wrapped_observations[indices] = wrapped
        return self._with_original(wrapped, deltas)

    def reset(self, states, indices=None):
        """The wrapped observers' reset observations become the old values; the changes are zero."""
        indices = self._all(indices)
        wrapped = super().reset(states, indices)
        self._old_wrapped_observations[indices] = wrapped
        return self._with_original(wrapped, np.zeros(wrapped.shape, dtype=np.float32))


class IndexedElementObserver(BaseObserver):
    """Observes one element of the state as it is (state_observer.py:386-421)."""

    kind = INDEXED_ELEMENT

    def __init__(self, num_envs, element_index, min_obs, max_obs):
        super().__init__(num_envs, min_obs, max_obs)
        self._element_index = element_index

    def observe(self, states, indices=None):
        if indices is None:
            indices = np.full(self.observation_space.shape[0], True)
        return states[:, self._element_index].reshape((indices.sum(), self.observation_space.shape[1]))


class NormalizedObserver(WrapperObserver):
    """The wrapped observations side by side, mapped from their bounds to [-1, 1] and clipped
    (state_observer.py:424-517)."""

    kind = NORMALIZED

    def __init__(self, observers):
        from reinfocus_amd.environments import harness  # (harness imports this module)

        observers = _sequence(observers)
        lows, highs = _stacked(observers, "low"), _stacked(observers, "high")
        ones = np.ones(len(lows), dtype=np.float32)
        super().__init__(observers, ones * -1, ones)
        self._mid, self._scale = harness.normaliser_from_bounds(lows, highs)

    def observe(self, states, indices=None):
        return self._normalize(self.wrapped_observations(states, indices))

    def reset(self, states, indices=None):
        return self._normalize(super().reset(states, indices))

    def _normalize(self, values):
        return np.clip((values - self._mid) / self._scale, -1, 1, dtype=np.float32)
