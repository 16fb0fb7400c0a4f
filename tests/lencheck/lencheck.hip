// lencheck.hip -- TEST INFRASTRUCTURE: exhaustive on-device check of len_inv_rn_fast (reinfocus_amd/csrc/rf_math.h),
// the rsq-seeded pair (len, inv) behind every shading direction of the render kernels, against the compiler's IEEE
// expansions: len == sqrtf(x) and inv == 1.0f / len for every float the fast path accepts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_math.h"

static constexpr uint32_t kFirstBits = 0x0D800000u, kEndBits = 0x71800000u; // [2^-100, 2^100): in_fast_range

__global__ void check_len_inv_kernel(unsigned long long *out /*[2]: mismatches, lowest mismatching bit pattern*/)
{
    unsigned long long bad = 0, first = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < kEndBits - kFirstBits;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t b = kFirstBits + (uint32_t)i;
        float x, len, inv;
        __builtin_memcpy(&x, &b, 4);
        rf::len_inv_rn_fast(x, len, inv);
        if (!(len == __builtin_sqrtf(x)) || !(inv == 1.0f / len)) {
            ++bad;
            first = b < first ? b : first;
        }
    }
    if (bad) {
        atomicAdd(&out[0], bad);
        atomicMin(&out[1], first);
    }
}

// out[0] = number of x with a wrong len or inv, out[1] = the bits of the smallest such x (all ones when there is
// none), out[2] = number of x visited; returns 0 when the check itself ran.
extern "C" int lc_check_len_inv(unsigned long long out[3])
{
    unsigned long long *d_out;
    const unsigned long long init[2] = {0ull, ~0ull};
    if (hipMalloc((void **)&d_out, sizeof init) != hipSuccess)
        return -1;
    if (hipMemcpy(d_out, init, sizeof init, hipMemcpyHostToDevice) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(check_len_inv_kernel, dim3(8192), dim3(256), 0, 0, d_out);
    if (hipDeviceSynchronize() != hipSuccess)
        return -2;
    if (hipMemcpy(out, d_out, sizeof init, hipMemcpyDeviceToHost) != hipSuccess)
        return -3;
    out[2] = kEndBits - kFirstBits;
    (void)hipFree(d_out);
    return 0;
}
