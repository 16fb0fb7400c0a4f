// mathcheck.hip -- TEST INFRASTRUCTURE: the one-argument functions of reinfocus_amd/csrc/rf_policy_math.h, and float32
// sqrtf and 1.0f / x as this repository's flags compile them, evaluated ON THE DEVICE for every float32 of their domains
// (mathcheck.h has the sweeps and the digest).  tests/test_gpu_scalar_math.py compares the digests with
// tests/golden/scalar_digests.npy, which the host build (mathcheck_host.cpp) and the numpy twins agree on.  Never loaded
// by the product package.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mathcheck.h"

static constexpr int kThreads = 256, kBlocksPerChunk = 8;
static constexpr uint32_t kSlice = mc::kChunkSize / kBlocksPerChunk; // patterns of one block: 2^19, 2048 per thread

// one chunk per kBlocksPerChunk blocks; a block outside the domain returns at once
template <int W>
__global__ __launch_bounds__(kThreads) void digest_kernel(unsigned long long *digest /*[1024]*/,
                                                          unsigned long long *visited /*[1024]*/)
{
    __shared__ unsigned long long sum_s[kThreads], count_s[kThreads];
    const uint32_t chunk = blockIdx.x / kBlocksPerChunk; // < mc::kChunks: the grid is kChunks * kBlocksPerChunk
    const uint32_t base = chunk * mc::kChunkSize + (blockIdx.x % kBlocksPerChunk) * kSlice;
    if (base + (kSlice - 1u) < mc::first_pattern(W) || base > mc::last_pattern(W))
        return;
    unsigned long long sum = 0, count = 0;
    for (uint32_t i = threadIdx.x; i < kSlice; i += kThreads) {
        const uint32_t pattern = base + i;
        if (mc::in_domain(W, pattern)) {
            sum += mc::term<W>(pattern);
            ++count;
        }
    }
    sum_s[threadIdx.x] = sum;
    count_s[threadIdx.x] = count;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half /= 2) {
        if ((int)threadIdx.x < half) {
            sum_s[threadIdx.x] += sum_s[threadIdx.x + half];
            count_s[threadIdx.x] += count_s[threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicAdd(&digest[chunk], sum_s[0]);
        atomicAdd(&visited[chunk], count_s[0]);
    }
}

template <int W> __global__ void map_kernel(uint32_t first, uint32_t count, uint32_t *out /*[count]*/)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const uint32_t pattern = first + i; // (no wrap: the caller checked first + count <= 2^32)
    out[i] = mc::in_domain(W, pattern) ? mc::eval<W>(pattern) : rf::kPolicyNaN;
}

static bool g_failed = false; // after a HIP error nothing more is launched
static unsigned long long g_visited[mc::kSweeps][mc::kChunks];
static bool g_ran[mc::kSweeps];

static void launch_digest(int which, unsigned long long *d)
{
    const dim3 grid(mc::kChunks * kBlocksPerChunk), block(kThreads);
    switch (which) {
    case 0: hipLaunchKernelGGL(digest_kernel<0>, grid, block, 0, 0, d, d + mc::kChunks); break;
    case 1: hipLaunchKernelGGL(digest_kernel<1>, grid, block, 0, 0, d, d + mc::kChunks); break;
    case 2: hipLaunchKernelGGL(digest_kernel<2>, grid, block, 0, 0, d, d + mc::kChunks); break;
    case 3: hipLaunchKernelGGL(digest_kernel<3>, grid, block, 0, 0, d, d + mc::kChunks); break;
    case 4: hipLaunchKernelGGL(digest_kernel<4>, grid, block, 0, 0, d, d + mc::kChunks); break;
    case 5: hipLaunchKernelGGL(digest_kernel<5>, grid, block, 0, 0, d, d + mc::kChunks); break;
    case 6: hipLaunchKernelGGL(digest_kernel<6>, grid, block, 0, 0, d, d + mc::kChunks); break;
    default: hipLaunchKernelGGL(digest_kernel<7>, grid, block, 0, 0, d, d + mc::kChunks); break;
    }
}

static void launch_map(int which, uint32_t first, uint32_t count, uint32_t *d)
{
    const dim3 grid((count + kThreads - 1) / kThreads), block(kThreads);
    switch (which) {
    case 0: hipLaunchKernelGGL(map_kernel<0>, grid, block, 0, 0, first, count, d); break;
    case 1: hipLaunchKernelGGL(map_kernel<1>, grid, block, 0, 0, first, count, d); break;
    case 2: hipLaunchKernelGGL(map_kernel<2>, grid, block, 0, 0, first, count, d); break;
    case 3: hipLaunchKernelGGL(map_kernel<3>, grid, block, 0, 0, first, count, d); break;
    case 4: hipLaunchKernelGGL(map_kernel<4>, grid, block, 0, 0, first, count, d); break;
    case 5: hipLaunchKernelGGL(map_kernel<5>, grid, block, 0, 0, first, count, d); break;
    case 6: hipLaunchKernelGGL(map_kernel<6>, grid, block, 0, 0, first, count, d); break;
    default: hipLaunchKernelGGL(map_kernel<7>, grid, block, 0, 0, first, count, d); break;
    }
}

static int fail(int code)
{
    g_failed = true;
    return code;
}

// out[k] = the digest of chunk k of sweep `which` (0 for a chunk outside its domain): one launch.  0 when the check
// itself ran; -1 .. -4 after a HIP error (and -9 from every later call), -8 for a `which` that is no sweep.
extern "C" int mc_digests(int which, unsigned long long out[1024])
{
    if (g_failed)
        return -9;
    if (which < 0 || which >= mc::kSweeps)
        return -8;
    unsigned long long *d;
    const size_t bytes = 2 * mc::kChunks * sizeof(unsigned long long); // the digests, then the patterns visited
    if (hipMalloc((void **)&d, bytes) != hipSuccess)
        return fail(-1);
    if (hipMemset(d, 0, bytes) != hipSuccess)
        return fail(-1);
    launch_digest(which, d);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(-2);
    if (hipMemcpy(out, d, bytes / 2, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(g_visited[which], d + mc::kChunks, bytes / 2, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(-3);
    if (hipFree(d) != hipSuccess)
        return fail(-4);
    g_ran[which] = true;
    return 0;
}

// out[k] = how many patterns of chunk k the last mc_digests(which) visited, as its kernel counted them; -7 before it
extern "C" int mc_visited(int which, unsigned long long out[1024])
{
    if (which < 0 || which >= mc::kSweeps)
        return -8;
    if (!g_ran[which])
        return -7;
    for (int k = 0; k < mc::kChunks; ++k)
        out[k] = g_visited[which][k];
    return 0;
}

// out[i] = policy_canonical(f(x)) at the pattern first_pattern + i, i < count <= 2^22, the canonical NaN for a pattern
// outside the sweep's domain: what names a failure.  -5 for a run that is too long or passes the last pattern.
extern "C" int mc_map(int which, unsigned first_pattern, unsigned count, float *out)
{
    if (g_failed)
        return -9;
    if (which < 0 || which >= mc::kSweeps)
        return -8;
    if (count > mc::kChunkSize || (uint64_t)first_pattern + count > (1ull << 32))
        return -5;
    if (count == 0)
        return 0;
    uint32_t *d;
    if (hipMalloc((void **)&d, (size_t)count * 4) != hipSuccess)
        return fail(-1);
    launch_map(which, first_pattern, count, d);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return fail(-2);
    if (hipMemcpy(out, d, (size_t)count * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(-3);
    if (hipFree(d) != hipSuccess)
        return fail(-4);
    return 0;
}
