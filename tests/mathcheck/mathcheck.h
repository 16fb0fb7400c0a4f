// mathcheck.h -- TEST INFRASTRUCTURE: what tests/mathcheck's two libraries share -- the sweeps over the one-argument
// functions of reinfocus_amd/csrc/rf_policy_math.h (and the two compiler expansions flags.mk promises to be IEEE-exact),
// their domains, and the digest of a chunk.  The same text for hipcc (mathcheck.hip) and g++ (mathcheck_host.cpp).
//
//   which  function                 domain (bit patterns of the float32 argument x, or of normal32's p)
//   0      expw32(x)                all 2^32 (its half x <= 0 is exp32)
//   1      log32(x)                 the positive normals 0x00800000 .. 0x7F7FFFFF
//   2      tanh32(x)                all 2^32
//   3      sigmoid32(x)             all 2^32
//   4      sqrtf(x)                 all 2^32
//   5      1.0f / x                 all 2^32
//   6      normal32(double(p))      p in [2^-54, 1/2]: 0x24800000 .. 0x3F000000
//   7      normal32(1.0 - double(p)) p in [2^-29, 1/2]: 0x31000000 .. 0x3F000000 (the subtraction is exact there)
//
// Chunk k is the patterns [k * 2^22, (k + 1) * 2^22); digest[k] = the sum modulo 2^64, over the chunk's patterns inside
// the domain, of mix(pattern << 32 | bits(policy_canonical(f(x)))), mix = the splitmix64 finaliser.  The sum does not
// depend on the order, so threads may accumulate it in any split.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_policy_math.h"

namespace mc {

constexpr int kSweeps = 8, kChunks = 1024, kChunkShift = 22;
constexpr uint32_t kChunkSize = 1u << kChunkShift;

RF_HD uint32_t first_pattern(int which)
{
    return which == 1 ? 0x00800000u : which == 6 ? 0x24800000u : which == 7 ? 0x31000000u : 0u;
}

RF_HD uint32_t last_pattern(int which) // inclusive
{
    return which == 1 ? 0x7F7FFFFFu : (which == 6 || which == 7) ? 0x3F000000u : 0xFFFFFFFFu;
}

RF_HD bool in_domain(int which, uint32_t pattern)
{
    return pattern >= first_pattern(which) && pattern <= last_pattern(which);
}

// bits(policy_canonical(f(x))) of sweep W at a pattern of its domain
template <int W> RF_HD uint32_t eval(uint32_t pattern)
{
    const float x = rf::bits_f32(pattern);
    float y;
    if (W == 0)
        y = rf::expw32(x);
    else if (W == 1)
        y = rf::log32(x);
    else if (W == 2)
        y = rf::tanh32(x);
    else if (W == 3)
        y = rf::sigmoid32(x);
    else if (W == 4)
        y = sqrtf(x);
    else if (W == 5)
        y = 1.0f / x;
    else if (W == 6)
        y = rf::normal32((double)x);
    else
        y = rf::normal32(1.0 - (double)x);
    return rf::f32_bits(rf::policy_canonical(y));
}

RF_HD uint64_t mix(uint64_t z) // the splitmix64 finaliser
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

template <int W> RF_HD uint64_t term(uint32_t pattern)
{
    return mix((uint64_t)pattern << 32 | (uint64_t)eval<W>(pattern));
}

} // namespace mc
