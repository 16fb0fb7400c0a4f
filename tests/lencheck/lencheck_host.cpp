// lencheck_host.cpp -- TEST INFRASTRUCTURE: the host branch of len_inv_rn_fast (reinfocus_amd/csrc/rf_math.h), compiled as
// tests/hostsim compiles the header, for tests/test_hostsim_len_inv.py.  Never loaded by the product package.
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_math.h"

// len[i], inv[i] of every sq[i]; -1 (and nothing computed past it) for an sq outside the range the function accepts
extern "C" int lc_host_len_inv(const float *sq, float *len, float *inv, long n)
{
    for (long i = 0; i < n; ++i) {
        if (!rf::in_fast_range(sq[i]))
            return -1;
        rf::len_inv_rn_fast(sq[i], len[i], inv[i]);
    }
    return 0;
}
