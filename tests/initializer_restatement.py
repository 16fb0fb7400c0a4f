"""A pure-Python integer restatement of reinfocus_amd/csrc/rf_init.h (test infrastructure): numpy's PCG64DXSM, its
jump-ahead by a table of row jumps, and the rows of RangedInitializer._draw, over a compiled
rf_env_initializer_program (strategy_program.compile_initializer).  Python ints are exact and Python floats are IEEE
doubles evaluated one operation at a time, so this is the arithmetic the header writes, without its 64-bit pieces."""

import numpy as np

M64 = 2 ** 64 - 1
M128 = 2 ** 128 - 1
MULTIPLIER = 0xda942042e4dd58b5
JUMP_BITS = 31  # kInitJumpBits


def output(state):
    """The 64-bit output of a state (taken before the step)."""
    hi, lo = state >> 64, (state & M64) | 1
    hi ^= hi >> 32
    hi = hi * MULTIPLIER & M64
    hi ^= hi >> 48
    return hi * lo & M64


def step(state, inc):
    return (state * MULTIPLIER + inc) & M128


def jump(inc, delta):
    """(mult, plus) of `delta` steps at once: state -> mult * state + plus."""
    acc_mult, acc_plus, cur_mult, cur_plus = 1, 0, MULTIPLIER, inc
    while delta:
        if delta & 1:
            acc_mult = acc_mult * cur_mult & M128
            acc_plus = (acc_plus * cur_mult + cur_plus) & M128
        cur_plus = (cur_mult + 1) * cur_plus & M128
        cur_mult = cur_mult * cur_mult & M128
        delta >>= 1
    return acc_mult, acc_plus


def jump_table(inc, draws):
    """Entry i: 2^i rows of `draws` outputs each."""
    table = [jump(inc, draws)]
    for _ in range(1, JUMP_BITS):
        mult, plus = table[-1]
        table.append((mult * mult & M128, (mult + 1) * plus & M128))
    return table


def skip_rows(table, state, rows):
    assert 0 <= rows < 1 << JUMP_BITS
    for i in range(JUMP_BITS):
        if rows >> i & 1:
            mult, plus = table[i]
            state = (mult * state + plus) & M128
    return state


def unpack(program):
    """(counts, low, span, state, inc, draws) of an EnvInitializerProgram."""
    counts = [program.counts[0], program.counts[1]]
    low = [[program.low[j][c] for c in range(counts[j])] for j in range(2)]
    span = [[program.span[j][c] for c in range(counts[j])] for j in range(2)]
    state = program.state[0] | program.state[1] << 64
    inc = program.inc[0] | program.inc[1] << 64
    return counts, low, span, state, inc, 2 if counts == [1, 1] else 4


def draw_row(counts, low, span, draws, state, inc):
    """((element 0, element 1) as float32, the state after the row)."""
    u = []
    for _ in range(draws):
        u.append((output(state) >> 11) * 2.0 ** -53)
        state = step(state, inc)
    if draws == 2:
        return (np.float32(low[0][0] + span[0][0] * u[0]), np.float32(low[1][0] + span[1][0] * u[1])), state
    row = []
    for j in range(2):
        chosen = min(int(u[j] * float(counts[j])), counts[j] - 1)
        row.append(np.float32(low[j][chosen] + span[j][chosen] * u[2 + j]))
    return tuple(row), state


def draw(program, rows):
    """(float32[rows, 2], the state after them): every row jumps from the program's state on its own, as the draw
    kernel's lanes do; the state is where the advance kernel's jump of `rows` rows leads."""
    counts, low, span, state, inc, draws = unpack(program)
    table = jump_table(inc, draws)
    out = np.empty((rows, 2), dtype=np.float32)
    for r in range(rows):
        out[r], after = draw_row(counts, low, span, draws, skip_rows(table, state, r), inc)
        assert after == skip_rows(table, state, r + 1)
    return out, skip_rows(table, state, rows)
