// rf_init.h -- the arithmetic of a compiled RangedInitializer (rf_env_initializer_program): numpy's PCG64DXSM
// generator, its jump-ahead, and the rows RangedInitializer._draw makes of its doubles
// (reinfocus_amd/environments/state_initializer.py; the reference's environments/state_initializer.py:53-71).
//
// Plain C++ like rf_math.h, so that tests/initcheck compiles the very same text for the host and compares it with
// numpy on the CPU.  128-bit values are pairs of 64-bit words and every product is written out in 32-bit pieces: no
// __int128 (hipcc has no library call for it on the device), no intrinsics, no inline assembly.  64-bit multiplies run
// at a fraction of the 32-bit rate on gfx950; a lane draws one row, which is two to four outputs after a jump of at most
// one table entry per set bit of its row number.
#pragma once

#include <stdint.h>

#include "../../include/reinfocus_hip.h" // RF_ENV_MAX_RANGES
#include "rf_math.h"                     // RF_HD

namespace rf {

struct U128 {
    uint64_t lo, hi;
};

// high 64 bits of a * b
RF_HD uint64_t mul_hi64(uint64_t a, uint64_t b)
{
    const uint64_t a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull); // (< 3 * 2^32)
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

RF_HD U128 mul128(U128 a, U128 b) // mod 2^128
{
    return U128{a.lo * b.lo, mul_hi64(a.lo, b.lo) + a.lo * b.hi + a.hi * b.lo};
}

RF_HD U128 add128(U128 a, U128 b) // mod 2^128
{
    const uint64_t lo = a.lo + b.lo;
    return U128{lo, a.hi + b.hi + (lo < a.lo ? 1u : 0u)};
}

// ---- PCG64DXSM as numpy implements it (numpy/random/src/pcg64/pcg64.h: pcg_cm_random_r) ------------------------------
constexpr uint64_t kPcgCheapMultiplier = 0xda942042e4dd58b5ull;

struct Pcg {
    U128 state, inc; // inc is odd
};

// the affine map state -> mult * state + plus (mod 2^128): some number of generator steps at once
struct PcgJump {
    U128 mult, plus;
};

RF_HD U128 pcg_apply(const PcgJump &j, U128 state)
{
    return add128(mul128(j.mult, state), j.plus);
}

// the output is taken from the state before the step
RF_HD uint64_t pcg_next(Pcg &g)
{
    uint64_t hi = g.state.hi;
    const uint64_t lo = g.state.lo | 1u;
    hi ^= hi >> 32;
    hi *= kPcgCheapMultiplier;
    hi ^= hi >> 48;
    hi *= lo;
    g.state = pcg_apply(PcgJump{U128{kPcgCheapMultiplier, 0}, g.inc}, g.state);
    return hi;
}

// Generator.random(): (out >> 11) * 2^-53
RF_HD double pcg_double(Pcg &g)
{
    return (double)(pcg_next(g) >> 11) * (1.0 / 9007199254740992.0);
}

// `delta` steps as one map (bit_generator.advance: the O(log delta) composition of the step with itself)
RF_HD PcgJump pcg_jump(U128 inc, uint64_t delta)
{
    PcgJump acc{U128{1, 0}, U128{0, 0}}, cur{U128{kPcgCheapMultiplier, 0}, inc};
    for (; delta != 0; delta >>= 1) {
        if (delta & 1u) {
            acc.mult = mul128(acc.mult, cur.mult);
            acc.plus = add128(mul128(acc.plus, cur.mult), cur.plus);
        }
        cur.plus = mul128(add128(cur.mult, U128{1, 0}), cur.plus);
        cur.mult = mul128(cur.mult, cur.mult);
    }
    return acc;
}

// ---- the program the kernels read (made by rf_env_configure_initializer) --------------------------------------------
// jump[i] is 2^i rows, i.e. draws * 2^i generator steps: row r of a draw starts where the maps of r's set bits lead (they
// are powers of one map, so their order does not matter).  Row numbers and counts are below 2^31.
constexpr int kInitJumpBits = 31;

struct EnvInit {
    int counts[2];
    int draws; // doubles per row: 2 when every element has one range, else 4
    double low[2][RF_ENV_MAX_RANGES], span[2][RF_ENV_MAX_RANGES];
    PcgJump jump[kInitJumpBits];
};

RF_HD void init_jump_table(EnvInit &p, U128 inc) // host, at configure time and when the generator is reseeded
{
    p.jump[0] = pcg_jump(inc, (uint64_t)p.draws);
    for (int i = 1; i < kInitJumpBits; ++i) {
        const PcgJump &h = p.jump[i - 1];
        p.jump[i] = PcgJump{mul128(h.mult, h.mult), mul128(add128(h.mult, U128{1, 0}), h.plus)};
    }
}

// the kernels' form of a checked rf_env_initializer_program
RF_HD EnvInit init_program(const rf_env_initializer_program &h)
{
    EnvInit p{};
    p.draws = (h.counts[0] == 1 && h.counts[1] == 1) ? 2 : 4;
    for (int j = 0; j < 2; ++j) {
        p.counts[j] = h.counts[j];
        for (int c = 0; c < RF_ENV_MAX_RANGES; ++c) {
            p.low[j][c] = c < h.counts[j] ? h.low[j][c] : 0.0;
            p.span[j][c] = c < h.counts[j] ? h.span[j][c] : 0.0;
        }
    }
    init_jump_table(p, U128{h.inc[0], h.inc[1]});
    return p;
}

// the state `rows` rows later; P: EnvInit, or the kernels' view of it in the constant address space
template <class P>
RF_HD U128 init_skip_rows(const P &p, U128 state, uint32_t rows)
{
    for (int i = 0; i < kInitJumpBits && (rows >> i) != 0; ++i)
        if ((rows >> i) & 1u)
            state = add128(mul128(U128{p.jump[i].mult.lo, p.jump[i].mult.hi}, state),
                           U128{p.jump[i].plus.lo, p.jump[i].plus.hi});
    return state;
}

// One row of RangedInitializer._draw, operation by operation in float64 (no contraction: -ffp-contract=off), rounded
// to float32 once at the end (astype(float32)).  g is left after the row's draws.
template <class P>
RF_HD void init_draw_row(const P &p, Pcg &g, float &e0, float &e1)
{
    const double u0 = pcg_double(g), u1 = pcg_double(g);
    if (p.draws == 2) { // low + span * random((num_envs, 2))
        e0 = (float)(p.low[0][0] + p.span[0][0] * u0);
        e1 = (float)(p.low[1][0] + p.span[1][0] * u1);
        return;
    }
    // u = random((num_envs, 4)): range min(int64(u_j * count_j), count_j - 1) of element j, then low + (high - low) * u_{2+j}
    const double v0 = pcg_double(g), v1 = pcg_double(g);
    int64_t c0 = (int64_t)(u0 * (double)p.counts[0]), c1 = (int64_t)(u1 * (double)p.counts[1]);
    c0 = c0 < p.counts[0] - 1 ? c0 : p.counts[0] - 1;
    c1 = c1 < p.counts[1] - 1 ? c1 : p.counts[1] - 1;
    e0 = (float)(p.low[0][c0] + p.span[0][c0] * v0);
    e1 = (float)(p.low[1][c1] + p.span[1][c1] * v1);
}

} // namespace rf
