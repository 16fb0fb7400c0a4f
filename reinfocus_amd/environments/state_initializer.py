"""State initializers: the first states of episodes (reference: environments/state_initializer.py).

RangedInitializer takes, per state element, one or several (low, high) ranges, as the reference's does.  Deliberate
difference: the reference draws from an unseeded PCG64DXSM generator; here `seed` makes runs reproducible, and the draw
order is defined:
 * one range per element: rows are low + (high - low) * random((num_envs, n)), low / high per element -- exactly what
   harness._Initializer draws (Generator.uniform's arithmetic);
 * several ranges for some element: every row draws random(2 n) -- n range choices (range floor(u * count) of the
   element's), then n values low + (high - low) * u in the chosen ranges.
Rows are drawn one after the other, so the first k rows of any draw are what a draw of k rows gives.  That keeps
_Initializer's propose / consume protocol: propose(num_envs) returns rows without consuming them, initialize(k) then
consumes exactly the k rows that were used (the device step hands row r to the r-th environment that ended).
"""

import numpy as np


class RangedInitializer:
    def __init__(self, ranges, seed=None):
        self._ranges = [[tuple(r) for r in element] for element in ranges]
        assert all(len(element) > 0 for element in self._ranges), "every element needs at least one range"
        self._counts = np.array([len(element) for element in self._ranges])
        self._lows = [np.array([r[0] for r in element], dtype=np.float64) for element in self._ranges]
        self._highs = [np.array([r[1] for r in element], dtype=np.float64) for element in self._ranges]
        self._single = bool(np.all(self._counts == 1))
        self._low = np.array([lows[0] for lows in self._lows])
        self._span = np.array([highs[0] for highs in self._highs]) - self._low
        self.seed(seed)

    def seed(self, seed):
        self._generator = np.random.Generator(np.random.PCG64DXSM(seed))

    def _draw(self, num_envs):
        n = len(self._ranges)
        if self._single:
            return (self._low + self._span * self._generator.random((num_envs, n))).astype(np.float32)
        u = self._generator.random((num_envs, 2 * n))
        rows = np.empty((num_envs, n), dtype=np.float64)
        for j in range(n):
            chosen = np.minimum((u[:, j] * self._counts[j]).astype(np.int64), self._counts[j] - 1)
            low, high = self._lows[j][chosen], self._highs[j][chosen]
            rows[:, j] = low + (high - low) * u[:, n + j]
        return rows.astype(np.float32)

    def initialize(self, num_envs):
        return self._draw(num_envs)

    def propose(self, num_envs):
        """The rows initialize(num_envs) would return, without consuming them (the generator's state is put back)."""
        bit_generator = self._generator.bit_generator
        state = bit_generator.state
        rows = self._draw(num_envs)
        bit_generator.state = state
        return rows
