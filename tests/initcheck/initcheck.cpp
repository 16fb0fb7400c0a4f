// initcheck.cpp -- TEST INFRASTRUCTURE.  Compiles the device initializer's arithmetic (reinfocus_amd/csrc/rf_init.h,
// the exact text the gfx950 kernels inline) for the host, so that a CPU-only test can compare it with numpy before any
// GPU sees it.  Never loaded by the product package.
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_init.h"

using namespace rf;

extern "C" {

// Rows 0 .. rows-1 as env_draw_pool_kernel's lanes make them -- every row jumps from the program's state on its own --
// into out float32[rows][2]; state_after: where env_init_advance_kernel leaves the generator after `rows` rows.
// Returns how many rows did not end at the state the next row's jump starts from (0: jumps and steps agree).
int ic_draw(const rf_env_initializer_program *h, int rows, float *out, uint64_t state_after[2])
{
    const EnvInit p = init_program(*h);
    const U128 state{h->state[0], h->state[1]}, inc{h->inc[0], h->inc[1]};
    int mismatches = 0;
    for (int r = 0; r < rows; ++r) {
        Pcg g{init_skip_rows(p, state, (uint32_t)r), inc};
        init_draw_row(p, g, out[2 * r], out[2 * r + 1]);
        const U128 next = init_skip_rows(p, state, (uint32_t)r + 1u);
        mismatches += (next.lo != g.state.lo || next.hi != g.state.hi) ? 1 : 0;
    }
    const U128 after = init_skip_rows(p, state, (uint32_t)rows);
    state_after[0] = after.lo;
    state_after[1] = after.hi;
    return mismatches;
}

// the state `rows` rows after the program's (rows < 2^31)
void ic_skip(const rf_env_initializer_program *h, uint32_t rows, uint64_t state_after[2])
{
    const EnvInit p = init_program(*h);
    const U128 after = init_skip_rows(p, U128{h->state[0], h->state[1]}, rows);
    state_after[0] = after.lo;
    state_after[1] = after.hi;
}

} // extern "C"
