// mathcheck_host.cpp -- TEST INFRASTRUCTURE: mathcheck.hip's entry points for the host, the very same header compiled with
// tests/policycheck's flags (mathcheck.h has the sweeps and the digest), and mc_errors, the distance of the four float32
// functions from glibc's float64 ones.  tests/golden/make_scalar_digests.py and tests/test_scalar_math_logic.py use it.
// Never loaded by the product package.
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "mathcheck.h"

namespace {

int threads_to_use()
{
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::min(16u, std::max(1u, hw));
}

// body(k) for every chunk k, the chunks handed out one by one to min(16, hardware_concurrency) threads
template <class Body> void over_chunks(Body body)
{
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < threads_to_use(); ++t)
        pool.emplace_back([&] {
            for (int k = next++; k < mc::kChunks; k = next++)
                body(k);
        });
    for (auto &t : pool)
        t.join();
}

unsigned long long g_visited[mc::kSweeps][mc::kChunks];
bool g_ran[mc::kSweeps];

template <int W> void digests(unsigned long long *out)
{
    over_chunks([&](int k) {
        unsigned long long sum = 0, count = 0;
        const uint32_t base = (uint32_t)k << mc::kChunkShift;
        for (uint32_t i = 0; i < mc::kChunkSize; ++i)
            if (mc::in_domain(W, base + i)) {
                sum += mc::term<W>(base + i);
                ++count;
            }
        out[k] = sum;
        g_visited[W][k] = count;
    });
    g_ran[W] = true;
}

template <int W> void map(uint32_t first, uint32_t count, float *out)
{
    for (uint32_t i = 0; i < count; ++i)
        out[i] = rf::bits_f32(mc::in_domain(W, first + i) ? mc::eval<W>(first + i) : rf::kPolicyNaN);
}

// the error of sweep W at x against glibc's float64 function, in the sweep's metric; 0 where the metric has no say
template <int W> double error_at(float x)
{
    const double wide = (double)x;
    if (W == 0) { // exp32: relative, on [-87, 0]
        if (!(x >= -87.0f && x <= 0.0f))
            return 0.0;
        const double want = exp(wide);
        return fabs((double)rf::exp32(x) - want) / want;
    }
    if (W == 1) { // log32: |err| / max(1, |ln s|)
        const double want = log(wide);
        return fabs((double)rf::log32(x) - want) / std::max(1.0, fabs(want));
    }
    if (x != x)
        return 0.0;
    if (W == 2) // tanh32: absolute
        return fabs((double)rf::tanh32(x) - tanh(wide));
    return fabs((double)rf::sigmoid32(x) - 1.0 / (1.0 + exp(-wide))); // sigmoid32: absolute
}

template <int W> void errors(double *out)
{
    over_chunks([&](int k) {
        double worst = 0.0;
        const uint32_t base = (uint32_t)k << mc::kChunkShift;
        for (uint32_t i = 0; i < mc::kChunkSize; ++i)
            if (mc::in_domain(W, base + i))
                worst = std::max(worst, error_at<W>(rf::bits_f32(base + i)));
        out[k] = worst;
    });
}

} // namespace

// out[k] = the digest of chunk k of sweep `which` (0 for a chunk outside its domain); 0, or -8 for a `which` that is no sweep
extern "C" int mc_digests(int which, unsigned long long out[1024])
{
    switch (which) {
    case 0: digests<0>(out); return 0;
    case 1: digests<1>(out); return 0;
    case 2: digests<2>(out); return 0;
    case 3: digests<3>(out); return 0;
    case 4: digests<4>(out); return 0;
    case 5: digests<5>(out); return 0;
    case 6: digests<6>(out); return 0;
    case 7: digests<7>(out); return 0;
    }
    return -8;
}

// out[k] = how many patterns of chunk k the last mc_digests(which) visited; -7 before it
extern "C" int mc_visited(int which, unsigned long long out[1024])
{
    if (which < 0 || which >= mc::kSweeps)
        return -8;
    if (!g_ran[which])
        return -7;
    std::copy(g_visited[which], g_visited[which] + mc::kChunks, out);
    return 0;
}

// out[i] = policy_canonical(f(x)) at the pattern first_pattern + i, i < count <= 2^22, the canonical NaN for a pattern
// outside the sweep's domain; -5 for a run that is too long or passes the last pattern
extern "C" int mc_map(int which, unsigned first_pattern, unsigned count, float *out)
{
    if (which < 0 || which >= mc::kSweeps)
        return -8;
    if (count > mc::kChunkSize || (uint64_t)first_pattern + count > (1ull << 32))
        return -5;
    switch (which) {
    case 0: map<0>(first_pattern, count, out); break;
    case 1: map<1>(first_pattern, count, out); break;
    case 2: map<2>(first_pattern, count, out); break;
    case 3: map<3>(first_pattern, count, out); break;
    case 4: map<4>(first_pattern, count, out); break;
    case 5: map<5>(first_pattern, count, out); break;
    case 6: map<6>(first_pattern, count, out); break;
    default: map<7>(first_pattern, count, out); break;
    }
    return 0;
}

// out[k] = the largest error of chunk k against glibc's float64 exp, log, tanh and 1 / (1 + exp(-x)), sweeps 0 to 3:
// relative on [-87, 0] for exp32, |err| / max(1, |ln s|) for log32, absolute for tanh32 and sigmoid32
extern "C" int mc_errors(int which, double out[1024])
{
    switch (which) {
    case 0: errors<0>(out); return 0;
    case 1: errors<1>(out); return 0;
    case 2: errors<2>(out); return 0;
    case 3: errors<3>(out); return 0;
    }
    return -8;
}
