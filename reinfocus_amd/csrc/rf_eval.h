// rf_eval.h -- the evaluation of G groups of m lanes on the device (include/reinfocus_hip.h, "evaluation"): what
// stable-baselines3's evaluate_policy keeps of a run over a vector environment -- the first target(i) episodes of every
// lane --, per group, from the episode records a step writes, and the best mean so far.
//
//   eval_accumulate_kernel   one thread per lane: an episode that ended in this step (final_length > 0) goes into the
//                            lane's next slot while the lane is below its target.  No atomics: a lane is one thread's.
//   eval_finish_kernel       one block of 256 threads per group: the fixed float64 pairwise tree over the E kept values in
//                            their fixed positions (lane-major, slot-minor) -- per-thread runs, an xor-butterfly per wave,
//                            the four wave results through LDS, as env_view_moments_kernel's --, three times (returns,
//                            squared differences, lengths); minimum and maximum by an integer key; the best rule; thread 0
//                            writes the row.
//   eval_keep_rows_kernel    grid (ceil(words / 1024), G): dst row g := src row g where select[g] != 0, in 16-byte vectors
//                            with dword head and tail.  Keeps the best parameters and statistics, and restores them.
// (eval_statistics_kernel, the moments of a learner view <-> a float64 [G][3][W + 1] tensor, is rf_abi_eval.hip's own.)
//
// The rules are plain C++ (RF_HD): tests/evalcheck loops over the same functions on the host, and the numpy twin is
// environments/evaluation.py.  Nothing is contracted (flags.mk); the float64 divide and sqrt are correctly rounded.
#pragma once
#include <stdint.h>
#include <string.h>

#include "rf_math.h" // RF_HD

#include "../../include/reinfocus_hip.h"

namespace rf {

constexpr int kEvalThreads = 256; // threads of eval_finish_kernel's block: 4 waves
constexpr int kEvalLevels = 9;    // tree levels inside one thread: 2^8 leaves x 256 threads = RF_EVAL_MAX_EPISODES
static_assert((1 << (kEvalLevels - 1)) * kEvalThreads == RF_EVAL_MAX_EPISODES, "a thread's run of leaves fits its levels");

// What the kernels take by value: G groups of m lanes, E episodes per group, K = ceil(E / m) slots per lane.
struct EvalShape {
    int groups, m, episodes, slots;
};

// SB3's episode_count_targets for the lane with local index i: (E + i) / m.  The targets of a group sum to E.
RF_HD int eval_target(int m, int E, int i) { return (E + i) / m; }

RF_HD int eval_slots(int m, int E) { return (E + m - 1) / m; }

// The sum of target(j) over j < i: the first m - E % m lanes have E / m each, the others one more.
RF_HD int eval_first(int m, int E, int i)
{
    const int q = E / m, plain = m - E % m;
    return i * q + (i > plain ? i - plain : 0);
}

// position p < E -> (lane i, slot k) with eval_first(i) + k == p and k < target(i)
RF_HD void eval_locate(int m, int E, int p, int &i, int &k)
{
    const int q = E / m, plain = m - E % m;
    const int low = plain * q; // positions of the lanes with target q (none when q is 0)
    if (p < low) {
        i = p / q;
        k = p - i * q;
    } else {
        const int rest = p - low;
        i = plain + rest / (q + 1);
        k = rest - (i - plain) * (q + 1);
    }
}

// One lane, one step: the record of an episode that ended goes into the next slot below the target.  A NaN return is a
// value and is kept; a lane at its target is ignored, as in SB3.  (A count outside 0 .. target is never written to.)
RF_HD void eval_accumulate_one(int target, double final_return, int final_length, int *count, double *returns,
                               int *lengths)
{
    const int c = *count;
    if (final_length > 0 && c >= 0 && c < target) {
        returns[c] = final_return;
        lengths[c] = final_length;
        *count = c + 1;
    }
}

// A total order of the non-NaN doubles as signed integers, -0.0 below +0.0: minimum and maximum do not depend on the order
// in which they are taken.
RF_HD int64_t eval_key(double x)
{
    int64_t b;
    memcpy(&b, &x, 8);
    return b < 0 ? (b ^ INT64_MAX) : b;
}

RF_HD double eval_unkey(int64_t key)
{
    const int64_t b = key < 0 ? (key ^ INT64_MAX) : key;
    double x;
    memcpy(&x, &b, 8);
    return x;
}

RF_HD double eval_nan()
{
    const uint64_t b = 0x7ff8000000000000ull;
    double x;
    memcpy(&x, &b, 8);
    return x;
}

// What a row holds of a NaN: the one quiet NaN above, whatever sign or payload the arithmetic gave it.
// Decided and written on the bits: a floating-point select of a NaN may keep the sign and payload it came with.
RF_HD double eval_canonical(double x)
{
    uint64_t b;
    memcpy(&b, &x, 8);
    if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull)
        b = 0x7ff8000000000000ull;
    memcpy(&x, &b, 8);
    return x;
}

// The tree over the `leaves` (a power of two) consecutive leaves one thread owns: env_view.h's view_thread_tree with this
// kernel's depth -- a binary counter of partial sums indexed by constants only.
#if defined(__clang__)
#define RF_EVAL_UNROLL _Pragma("unroll")
#else
#define RF_EVAL_UNROLL // (the host build's compiler: the loops are the same loops)
#endif
template <typename Leaf>
RF_HD double eval_thread_tree(int leaves, Leaf leaf)
{
    double acc[kEvalLevels];
RF_EVAL_UNROLL
    for (int l = 0; l < kEvalLevels; ++l)
        acc[l] = 0.0;
    double v = 0.0;
    for (int i = 0; i < leaves; ++i) {
        v = leaf(i);
        bool carry = true;
RF_EVAL_UNROLL
        for (int l = 0; l < kEvalLevels; ++l) {
            const bool bit = (i >> l) & 1;
            if (carry && bit)
                v = acc[l] + v;
            if (carry && !bit)
                acc[l] = v;
            carry = carry && bit;
        }
    }
    return v;
}

// leaves per thread for E positions: max(P / 256, 1), P the next power of two >= E
RF_HD int eval_leaves(int E)
{
    int P = 1;
    while (P < E)
        P <<= 1;
    return P > kEvalThreads ? P / kEvalThreads : 1;
}

// The row of a group, columns 0 .. 7 of "evaluation".
RF_HD void eval_write_row(double *row, bool complete, double mean, double std, bool any_nan, int64_t min_key,
                          int64_t max_key, double mean_length, int kept, unsigned long long serial)
{
    const double nan = eval_nan();
    row[0] = complete ? eval_canonical(mean) : nan;
    row[1] = complete ? eval_canonical(std) : nan;
    row[2] = complete && !any_nan ? eval_unkey(min_key) : nan;
    row[3] = complete && !any_nan ? eval_unkey(max_key) : nan;
    row[4] = complete ? mean_length : nan;
    row[5] = (double)kept;
    row[6] = complete ? 0.0 : (double)RF_EVAL_INCOMPLETE;
    row[7] = (double)serial;
}

// The best rule: strict, and a NaN mean never improves (the comparison is false).
RF_HD void eval_best(bool complete, double mean, unsigned long long serial, double *best_mean, long long *best_serial,
                     uint8_t *improved)
{
    const bool better = complete && mean > *best_mean;
    if (better) {
        *best_mean = mean;
        *best_serial = (long long)serial;
    }
    *improved = better ? 1 : 0;
}

#if defined(__HIPCC__)

__global__ __launch_bounds__(kEvalThreads) void eval_accumulate_kernel(EvalShape s, const double *final_return,
                                                                       const int *final_length, int *counts,
                                                                       double *returns, int *lengths)
{
    const long long lane = (long long)blockIdx.x * kEvalThreads + threadIdx.x;
    if (lane >= (long long)s.groups * s.m)
        return;
    const int i = (int)(lane % s.m);
    const size_t row = (size_t)lane * (size_t)s.slots;
    eval_accumulate_one(eval_target(s.m, s.episodes, i), final_return[lane], final_length[lane], counts + lane,
                        returns + row, lengths + row);
}

// The block's part of a tree: every thread brings the sum of its own aligned run, every thread gets the total.  Inside a
// wave the xor-butterfly of view_block_treesum, then the four wave results through LDS and the same butterfly over four
// lanes.  Additions with padding zeros are performed; the last one turns -0.0 into +0.0.
__device__ __forceinline__ double eval_block_treesum(double v, double *wave_sums)
{
    for (int off = 1; off < 64; off <<= 1)
        v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads(); // (wave_sums may still be read from the pass before)
    if (lane == 0)
        wave_sums[wave] = v;
    __syncthreads();
    double w = wave_sums[lane & 3];
    for (int off = 1; off < 4; off <<= 1)
        w += __shfl_xor(w, off, 64);
    return w + 0.0;
}

// The block's minimum of a and maximum of b, as integers: any order gives the same.
__device__ __forceinline__ void eval_block_minmax(long long &a, long long &b, long long *wave_keys)
{
    for (int off = 1; off < 64; off <<= 1) {
        const long long x = __shfl_xor(a, off, 64), y = __shfl_xor(b, off, 64);
        a = x < a ? x : a;
        b = y > b ? y : b;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
        wave_keys[wave] = a;
        wave_keys[4 + wave] = b;
    }
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
        const long long x = wave_keys[w], y = wave_keys[4 + w];
        a = x < a ? x : a;
        b = y > b ? y : b;
    }
}

__global__ __launch_bounds__(kEvalThreads) void eval_finish_kernel(EvalShape s, unsigned long long serial, int leaves,
                                                                   const int *counts, const double *returns,
                                                                   const int *lengths, double *results, double *best_mean,
                                                                   long long *best_serial, uint8_t *improved)
{
    __shared__ double wave_sums[4];
    __shared__ long long wave_keys[8];
    const int g = blockIdx.x, m = s.m, E = s.episodes;
    const size_t base = (size_t)g * (size_t)m;
    counts += base;
    returns += base * (size_t)s.slots;
    lengths += base * (size_t)s.slots;
    // how many episodes the group has kept (never more than E: a lane stops at its target), and whether one is NaN
    long long kept = 0;
    for (int i = threadIdx.x; i < m; i += kEvalThreads) {
        const int c = counts[i];
        kept += c > 0 ? c : 0;
    }
    for (int off = 1; off < 64; off <<= 1) // (integers: any order gives the same sum)
        kept += __shfl_xor(kept, off, 64);
    if ((threadIdx.x & 63) == 0)
        wave_keys[threadIdx.x >> 6] = kept;
    __syncthreads();
    kept = wave_keys[0] + wave_keys[1] + wave_keys[2] + wave_keys[3];
    const bool complete = kept == E; // (uniform over the block)
    if (!complete) {
        if (threadIdx.x == 0) {
            eval_write_row(results + (size_t)g * 8, false, 0.0, 0.0, false, 0, 0, 0.0, (int)kept, serial);
            improved[g] = 0;
        }
        return;
    }
    const int first = (int)threadIdx.x * leaves;
    long long min_key = INT64_MAX, max_key = INT64_MIN;
    bool any_nan = false;
    double t = eval_thread_tree(leaves, [&](int j) {
        const int p = first + j;
        if (p >= E)
            return 0.0;
        int i, k;
        eval_locate(m, E, p, i, k);
        const double x = returns[(size_t)i * (size_t)s.slots + k];
        if (x != x) {
            any_nan = true;
        } else {
            const long long key = eval_key(x);
            min_key = key < min_key ? key : min_key;
            max_key = key > max_key ? key : max_key;
        }
        return x;
    });
    const double N = (double)E;
    const double mean = eval_block_treesum(t, wave_sums) / N;
    t = eval_thread_tree(leaves, [&](int j) {
        const int p = first + j;
        if (p >= E)
            return 0.0;
        int i, k;
        eval_locate(m, E, p, i, k);
        const double d = returns[(size_t)i * (size_t)s.slots + k] - mean;
        return d * d;
    });
    const double std = sqrt(eval_block_treesum(t, wave_sums) / N);
    t = eval_thread_tree(leaves, [&](int j) {
        const int p = first + j;
        if (p >= E)
            return 0.0;
        int i, k;
        eval_locate(m, E, p, i, k);
        return (double)lengths[(size_t)i * (size_t)s.slots + k];
    });
    const double mean_length = eval_block_treesum(t, wave_sums) / N;
    // a NaN anywhere makes the minimum and the maximum NaN (numpy.min): its flag travels as the maximum of a third key
    long long nan_low = any_nan ? -1 : 0, nan_high = any_nan ? 1 : 0;
    eval_block_minmax(min_key, max_key, wave_keys);
    eval_block_minmax(nan_low, nan_high, wave_keys);
    if (threadIdx.x == 0) {
        eval_write_row(results + (size_t)g * 8, true, mean, std, nan_high != 0, min_key, max_key, mean_length, (int)kept,
                       serial);
        eval_best(true, mean, serial, best_mean + g, best_serial + g, improved + g);
    }
}

// dst row g := src row g where select[g] != 0.  Rows of `words` 4-byte words, `stride` words apart.  vec != 0 (the host
// has seen that src and dst are congruent mod 16 bytes): dwords up to the first 16-byte boundary of the row (block 0), the
// body as uint4, one per thread, then the last words % 4 dwords (block 0); vec == 0: dwords throughout.
__global__ __launch_bounds__(kEvalThreads) void eval_keep_rows_kernel(unsigned words, unsigned stride, int vec,
                                                                      const uint8_t *__restrict__ select,
                                                                      const uint32_t *__restrict__ src,
                                                                      uint32_t *__restrict__ dst)
{
    const unsigned g = blockIdx.y;
    // select[g], uniform over the block, as a scalar load and a scalar branch: gfx950 has no scalar byte load, so the
    // aligned dword that holds the byte is read (it lies in the pages of the array, whatever the array's own alignment)
    const uint8_t *mine = select + g;
    const unsigned odd = (unsigned)((uintptr_t)mine & 3);
    const uint32_t word = *(const uint32_t *)(mine - odd);
    if (((word >> (8 * odd)) & 0xffu) == 0)
        return;
    src += (size_t)g * stride;
    dst += (size_t)g * stride;
    if (!vec) {
        for (int j = 0; j < 4; ++j) {
            const unsigned w = blockIdx.x * (kEvalThreads * 4) + j * kEvalThreads + threadIdx.x;
            if (w < words)
                dst[w] = src[w];
        }
        return;
    }
    unsigned head = (unsigned)((4 - (((uintptr_t)src >> 2) & 3)) & 3);
    head = head < words ? head : words;
    const unsigned body = (words - head) / 4, tail = (words - head) - 4 * body;
    const unsigned v = blockIdx.x * kEvalThreads + threadIdx.x;
    if (v < body)
        ((uint4 *)(dst + head))[v] = ((const uint4 *)(src + head))[v];
    if (blockIdx.x == 0) {
        if (threadIdx.x < head)
            dst[threadIdx.x] = src[threadIdx.x];
        if (threadIdx.x < tail)
            dst[head + 4 * body + threadIdx.x] = src[head + 4 * body + threadIdx.x];
    }
}

#endif // __HIPCC__

} // namespace rf
