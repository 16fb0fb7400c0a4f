// rf_env_init.h -- the initializer of the device-resident environment step on the device (rf_env_configure_initializer):
// the pool of candidate reset states that rf_env.h's kernels read is drawn here, where the host's copy of it would
// arrive, and the generator is advanced by what the step consumed.  Arithmetic: rf_init.h.
//   RangedInitializer.initialize           environments/state_initializer.py:53-71
//   as VectorEnvironment.step calls it     environments/vector_environment.py:138
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rf_common.h"
#include "rf_init.h"

namespace rf {

// The generator in device memory: state low / high word, increment low / high word.  The kernels of a replayed graph
// read it where it is, so every replay sees what the step before left.  Read with ordinary loads (it changes between
// launches); the program next to it only changes with the stream idle and is read through the constant address space.
__device__ __forceinline__ Pcg init_load(const unsigned long long *gen)
{
    return Pcg{U128{gen[0], gen[1]}, U128{gen[2], gen[3]}};
}

// One lane per row r < rows: rows[2 r], rows[2 r + 1] := row r of the draw that starts at the generator's state.
// The generator itself is left alone (env_init_advance_kernel moves it once the number of used rows is known).
__global__ void env_draw_pool_kernel(const EnvInit *init, const unsigned long long *gen, float *pool, int rows)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows)
        return;
    const_as<EnvInit> &p = *as_const(init);
    Pcg g = init_load(gen);
    g.state = init_skip_rows(p, g.state, (uint32_t)r);
    float e0, e1;
    init_draw_row(p, g, e0, e1);
    pool[2 * r] = e0;
    pool[2 * r + 1] = e1;
}

// initialize(k): the generator moves past the k rows that were used -- k = *count (EnvState::done_count, final by
// now), or `given` where count is null (rf_env_reset: all n).  One thread; stream order puts it after the kernels that
// read the pool and before the next draw.
__global__ void env_init_advance_kernel(const EnvInit *init, unsigned long long *gen, const int *count, int given)
{
    if (blockIdx.x != 0 || threadIdx.x != 0)
        return;
    const int k = count ? *count : given;
    const U128 state = init_skip_rows(*as_const(init), U128{gen[0], gen[1]}, (uint32_t)k);
    gen[0] = state.lo;
    gen[1] = state.hi;
}

} // namespace rf
