"""The device initializer's arithmetic before any GPU sees it: a pure-Python integer restatement of
reinfocus_amd/csrc/rf_init.h (tests/initializer_restatement.py) against numpy -- RangedInitializer.initialize bit for
bit, the generator's state afterwards, the jump to a row against bit_generator.advance --, the compiler's refusals, and
the header itself compiled for the host (tests/initcheck) against numpy over 10^5 rows per initializer."""

import ctypes

import numpy as np
import pytest

from reinfocus_amd import _native
from reinfocus_amd.environments import state_initializer as si
from reinfocus_amd.environments import strategy_program as sp
from tests import helpers
from tests import initializer_restatement as ir

ENDS = (5.0, 10.0)
# one range per element (2 draws a row) and several (4 draws a row): counts of 1, 2, 3 and 8, ranges with high < low,
# zero-width ranges, ranges around zero and of very different magnitudes
INITIALIZERS = {
    "single": [[ENDS], [ENDS]],
    "single, reversed and zero-width": [[(10.0, 5.0)], [(7.25, 7.25)]],
    "single, mixed signs": [[(-3.5, 1e-3)], [(1e6, -1e-6)]],
    "counts 1 and 2": [[ENDS], [(5.0, 6.0), (9.0, 10.0)]],
    "counts 3 and 8": [[(5.0, 6.0), (10.0, 9.0), (7.5, 7.5)],
                       [(0.0, 1.0), (1.0, 0.5), (2.0, 2.0), (-4.0, -3.0), (1e-3, 2e-3), (100.0, 250.0), (6.0, 6.5),
                        (-0.125, 0.125)]],
    "counts 8 and 1": [[(float(i), float(i) + 0.5) for i in range(8)], [(9.0, 5.0)]],
    "counts 2 and 2": [[(5.0, 5.0), (6.0, 7.0)], [(10.0, 9.0), (8.0, 8.5)]],
}


def _initializer(name, seed):
    return si.RangedInitializer(INITIALIZERS[name], seed=seed)


def _generator_state(initializer):
    return initializer._generator.bit_generator.state["state"]["state"]


def _same_bits(got, want):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("k", [1, 2, 65, 1100])
@pytest.mark.parametrize("name", list(INITIALIZERS))
def test_restatement_equals_numpy(name, k):
    """The restated rows equal RangedInitializer.initialize(k) bit for bit, and the restated state after k rows is the
    numpy generator's; a second draw continues from there."""
    initializer = _initializer(name, 1234 + k)
    program = sp.compile_initializer(initializer)
    rows, after = ir.draw(program, k)
    _same_bits(rows, initializer.initialize(k))
    assert after == _generator_state(initializer)
    program = sp.compile_initializer(initializer)  # (the generator as it stands now)
    rows, after = ir.draw(program, 3)
    _same_bits(rows, initializer.initialize(3))
    assert after == _generator_state(initializer)


@pytest.mark.parametrize("name", ["single", "counts 3 and 8"])
def test_jump_to_a_row_equals_advance(name):
    """Row r starts r * d steps after the generator's state: the table's jump against bit_generator.advance(r * d) for
    every r up to 130, around every power of two up to 2^20, at the table's last bit, and at random r below 2^31."""
    initializer = _initializer(name, 99)
    counts, _, _, state, inc, draws = ir.unpack(sp.compile_initializer(initializer))
    assert draws == (2 if name == "single" else 4)
    assert ir.jump(inc, 0) == (1, 0) and ir.jump(inc, 1) == (ir.MULTIPLIER, inc)
    table = ir.jump_table(inc, draws)
    rng = np.random.default_rng(3)
    rows = set(range(131)) | {(1 << b) + d for b in range(7, 21) for d in (-1, 0, 1)} | {2 ** 20, 2 ** 30, 2 ** 31 - 1}
    rows |= {int(r) for r in rng.integers(0, 2 ** 31, 64)}
    for r in sorted(rows):
        bit_generator = np.random.PCG64DXSM(0)
        bit_generator.state = initializer._generator.bit_generator.state
        bit_generator.advance(r * draws)
        assert ir.skip_rows(table, state, r) == bit_generator.state["state"]["state"], r
        assert bit_generator.state["state"]["inc"] == inc


def test_restated_generator_equals_numpy_doubles():
    """Generator.random((5, 2)) and the state after it, from the restated output function and step."""
    generator = np.random.Generator(np.random.PCG64DXSM(7))
    state, inc = sp.initializer_state(si.RangedInitializer([[ENDS], [ENDS]], seed=7))
    want = generator.random((5, 2)).reshape(-1)
    for value in want:
        assert (ir.output(state) >> 11) * 2.0 ** -53 == value
        state = ir.step(state, inc)
    assert state == generator.bit_generator.state["state"]["state"]


def test_compiled_words_round_trip():
    initializer = _initializer("counts 3 and 8", 5)
    initializer.initialize(17)
    program = sp.compile_initializer(initializer)
    state = initializer._generator.bit_generator.state["state"]
    assert program.state[0] | program.state[1] << 64 == state["state"]
    assert program.inc[0] | program.inc[1] << 64 == state["inc"] and program.inc[0] & 1
    assert [program.counts[0], program.counts[1]] == [3, 8]
    assert program.low[0][1] == 10.0 and program.span[0][1] == -1.0 and program.span[0][2] == 0.0
    assert sp.initializer_state(initializer) == (state["state"], state["inc"])
    assert _native.words128(state["state"]) == (program.state[0], program.state[1])
    # compiling reads the generator and leaves it where it was
    assert initializer._generator.bit_generator.state["state"] == state


def test_compiler_refusals():
    from reinfocus_amd.environments import harness

    nine = [(float(i), float(i) + 1.0) for i in range(9)]
    for bad in (si.RangedInitializer([[ENDS], [ENDS], [ENDS]], seed=1),  # three elements
                si.RangedInitializer([[ENDS]], seed=1),
                si.RangedInitializer([[ENDS], nine], seed=1),  # nine ranges
                si.RangedInitializer([[ENDS], [(5.0, float("nan"))]], seed=1),
                si.RangedInitializer([[(float("inf"), 5.0)], [ENDS]], seed=1),
                si.RangedInitializer([[ENDS], [(-3.4e38, 0.0)]], seed=1),  # outside the float32 range
                harness._Initializer(ENDS, 1), object(), None):
        with pytest.raises(AssertionError):
            sp.compile_initializer(bad)
    sp.compile_initializer(si.RangedInitializer([[ENDS], nine[:8]], seed=1))


def test_sharded_environments_refuse_the_keyword():
    from reinfocus_amd.environments import harness

    for cls in (harness.ShardedVectorDiscreteSteps, harness.ShardedVectorContinuousJumps):
        with pytest.raises(ValueError, match="device_initializer"):
            cls(num_envs=4, devices=[0, 0], device_initializer=True)


@pytest.fixture(scope="module")
def initcheck():
    lib = ctypes.CDLL(helpers.built("tests/initcheck", "libinitcheck.so"))
    program = ctypes.POINTER(_native.EnvInitializerProgram)
    lib.ic_draw.argtypes = [program, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    lib.ic_draw.restype = ctypes.c_int
    lib.ic_skip.argtypes = [program, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    lib.ic_skip.restype = None
    return lib


@pytest.mark.parametrize("name", list(INITIALIZERS))
def test_header_on_the_cpu_equals_numpy(name, initcheck):
    """rf_init.h itself, compiled for the host: 10^5 rows per initializer -- each from its own jump, as the kernel's
    lanes draw them -- equal numpy's bit for bit, every row ends where the next one's jump starts, and the state after
    them is numpy's."""
    rows = 100_000
    initializer = _initializer(name, 2024)
    program = sp.compile_initializer(initializer)
    got = np.empty((rows, 2), dtype=np.float32)
    after = (ctypes.c_uint64 * 2)()
    assert initcheck.ic_draw(ctypes.byref(program), rows, got.ctypes.data_as(ctypes.c_void_p), after) == 0
    _same_bits(got, initializer.initialize(rows))
    assert after[0] | after[1] << 64 == _generator_state(initializer)


def test_header_jump_equals_the_restatement(initcheck):
    """The header's jump table against the restated one at the table's ends (rows up to 2^31 - 1)."""
    program = sp.compile_initializer(_initializer("counts 1 and 2", 8))
    _, _, _, state, inc, draws = ir.unpack(program)
    table = ir.jump_table(inc, draws)
    after = (ctypes.c_uint64 * 2)()
    for r in (0, 1, 2 ** 20, 2 ** 30 + 12345, 2 ** 31 - 1):
        initcheck.ic_skip(ctypes.byref(program), r, after)
        assert after[0] | after[1] << 64 == ir.skip_rows(table, state, r)
