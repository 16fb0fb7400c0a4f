// rf_env_view.h -- the learner view of a device-resident environment (include/reinfocus_hip.h, "learner view"):
// VecNormalize followed by VecFrameStack, as the reference's PPO configurations wrap the environment (normalize: true,
// frame_stack: 5), computed on the step's own outputs by two kernels that follow the step on the ctx's stream, outside
// the replayed graphs.  One definition, shared with the numpy twin (harness._LearnerView), bit for bit:
//
//   treesum(x[0..n))   x as float64, padded with +0.0 to the next power of two P >= n, y = y[0::2] + y[1::2] until one
//                      value is left, that value + (+0.0).  The last addition turns -0.0 into +0.0 and changes nothing
//                      else; with it any further zero padding (a block wider than P) gives the same bits.
//   update(moments, x) RunningMeanStd.update_from_moments left to right, the batch mean and variance from two treesums.
//   normalise, the frame stack, the view reward, view_final: env_view_apply_kernel below.
//
// ONE DELIBERATE DIFFERENCE from stable-baselines3: SB3 takes the batch mean and variance with numpy.mean / numpy.var in
// the observation's dtype (float32) and in numpy's own order; the view takes them in float64 with the fixed tree above.
// That is more accurate, and it is reproducible on a GPU.  No FMA contraction anywhere (flags.mk).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rf_env_types.h" // EnvViewConfig, EnvViewMoments

namespace rf {

constexpr int kViewBlock = 1024; // threads of env_view_moments_kernel's block: 16 waves
constexpr int kViewLevels = 22; // tree levels inside one thread: 2^21 leaves x 1024 threads = 2^31 >= any int n

// The tree over the `leaves` (a power of two, the same for every thread) consecutive leaves one thread owns, leaf(i)
// for i = 0 .. leaves-1 in order: a binary counter of partial sums, acc[l] holding a finished sub-tree of 2^l leaves;
// leaf i is carried upwards through the levels whose bit of i is set and parked at the first one that is not.  The
// loop over the levels is unrolled and has one exit, so acc is indexed by constants only (registers, no scratch); i is
// uniform, so is every condition here.
template <typename Leaf>
__device__ __forceinline__ double view_thread_tree(int leaves, Leaf leaf)
{
    double acc[kViewLevels];
#pragma unroll
    for (int l = 0; l < kViewLevels; ++l)
        acc[l] = 0.0;
    double v = 0.0;
    for (int i = 0; i < leaves; ++i) {
        v = leaf(i);
        bool carry = true;
#pragma unroll
        for (int l = 0; l < kViewLevels; ++l) {
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

// The block's part of a treesum: every thread brings the sum of its own aligned sub-tree, every thread gets the total.
// Inside a wave a xor-butterfly (lane ^ 1, ^ 2, ... ^ 32: after step s every lane holds the sub-tree of its aligned
// group of 2^s lanes -- IEEE addition is commutative, so both partners compute the same bits), the 16 wave results go
// through LDS and are combined by the same butterfly over 16 lanes.  Additions with padding zeros are performed.
__device__ __forceinline__ double view_block_treesum(double v, double *wave_sums)
{
    for (int off = 1; off < 64; off <<= 1)
        v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads(); // (wave_sums may still be read from the pass before)
    if (lane == 0)
        wave_sums[wave] = v;
    __syncthreads();
    double w = wave_sums[lane & 15];
    for (int off = 1; off < 16; off <<= 1)
        w += __shfl_xor(w, off, 64);
    return w + 0.0;
}

// update(moments, x): RunningMeanStd.update_from_moments, left to right
__device__ __forceinline__ void view_update(EnvViewMoments *m, int slot, double bm, double bv, double N)
{
    const double mean = m->mean[slot], var = m->var[slot], count = m->count[slot];
    const double delta = bm - mean;
    const double tot = count + N;
    const double m2 = (var * count + bv * N) + (((delta * delta) * count) * N) / tot;
    m->mean[slot] = mean + (delta * N) / tot;
    m->var[slot] = m2 / tot;
    m->count[slot] = tot;
}

// Steps 1 and 3 of a step (and step "if training and norm_obs" of a reset): one block per updated slot -- blocks
// 0 .. obs_blocks-1 the observation columns (obs_blocks = W with norm_obs, else 0), the block after them the returns
// (with_returns: a step, not a reset), which first writes returns[e] = returns[e] * gamma + reward[e].  Launched only
// while training.  Two passes, mean and then squared deviations, each a treesum: thread t owns the aligned run of
// `leaves` = max(P / 1024, 1) leaves that starts at t * leaves (P the next power of two >= n), reads past n are +0.0.
// Thread 0 then applies the update.  Holds for any n: the run of leaves per thread grows, the block does not.
//
// kGrouped ("population view", groups of more than 64 lanes): blockIdx.y is the group, the block's batch is that
// group's m lanes [g m, (g + 1) m) -- P is P_m, N is m --, the returns are discounted by gamma[g], and the update goes
// to moments[g].  A template parameter, not a run-time flag: the ungrouped instantiation is the kernel of before,
// instruction for instruction.
template <bool kGrouped>
__global__ __launch_bounds__(kViewBlock) void env_view_moments_kernel(EnvViewConfig c, int obs_blocks, int leaves,
                                                                      const float *obs, const double *reward,
                                                                      double *returns, EnvViewMoments *moments,
                                                                      EnvViewGroups grp)
{
    __shared__ double wave_sums[16];
    const bool is_returns = (int)blockIdx.x >= obs_blocks;
    const int column = blockIdx.x; // (of an observation block)
    const long long first = (long long)threadIdx.x * leaves;
    const long long n = kGrouped ? grp.m : c.n;
    const size_t width = (size_t)c.width;
    if (kGrouped) { // this group's lanes and moments
        const size_t base = (size_t)blockIdx.y * (size_t)grp.m;
        obs += base * width;
        reward += base;
        returns += base;
        moments += blockIdx.y;
    }
    double s;
    if (is_returns) {
        const double gamma = kGrouped ? grp.gamma[blockIdx.y] : c.gamma;
        s = view_thread_tree(leaves, [&](int i) {
            const long long g = first + i;
            if (g >= n)
                return 0.0;
            const double r = returns[g] * gamma + reward[g];
            returns[g] = r; // (the second pass re-reads what this thread wrote itself)
            return r;
        });
    } else {
        s = view_thread_tree(leaves, [&](int i) {
            const long long g = first + i;
            return g < n ? (double)obs[(size_t)g * width + column] : 0.0;
        });
    }
    const double N = (double)(kGrouped ? grp.m : c.n);
    const double bm = view_block_treesum(s, wave_sums) / N;
    if (is_returns) {
        s = view_thread_tree(leaves, [&](int i) {
            const long long g = first + i;
            if (g >= n)
                return 0.0;
            const double d = returns[g] - bm;
            return d * d;
        });
    } else {
        s = view_thread_tree(leaves, [&](int i) {
            const long long g = first + i;
            if (g >= n)
                return 0.0;
            const double d = (double)obs[(size_t)g * width + column] - bm;
            return d * d;
        });
    }
    const double bv = view_block_treesum(s, wave_sums) / N;
    if (threadIdx.x == 0)
        view_update(moments, is_returns ? c.width : column, bm, bv, N);
}

constexpr int kViewPackedBlock = 256; // threads of env_view_moments_packed_kernel's block: 4 waves
constexpr int kViewPackedMax = 64; // the widest segment: one wave

// The same two passes for groups of at most 64 lanes (P_m <= 64; the reference's m is 8), where the kernel above would
// spend a 1024-thread block and four barriers on m values once per (slot, group).  Lanes are packed: the aligned
// segment of P_m consecutive threads number s = (blockIdx.x * 256 + threadIdx.x) / P_m is group s, the lane with index
// l inside it holds leaf l of that group -- +0.0 where l >= m or the group does not exist --, and blockIdx.y is the
// slot as blockIdx.x is above.  P_m divides 64, so a segment never crosses a wave: the tree is the xor-butterfly over
// offsets 1 .. P_m / 2 (after step s every lane holds the sub-tree of its aligned run of 2^s lanes; both partners
// compute the same bits), then + 0.0.  No LDS, no barrier; every lane of a wave reaches every butterfly step, idle
// lanes touch no memory.  m = 1 is the segment of one lane without a butterfly step.  Lane 0 of a segment applies the
// update to moments[g].
__global__ __launch_bounds__(kViewPackedBlock) void env_view_moments_packed_kernel(EnvViewConfig c, int obs_blocks,
                                                                                   const float *obs, const double *reward,
                                                                                   double *returns,
                                                                                   EnvViewMoments *moments,
                                                                                   EnvViewGroups grp)
{
    const bool is_returns = (int)blockIdx.y >= obs_blocks;
    const int column = blockIdx.y; // (of an observation block)
    const int thread = blockIdx.x * kViewPackedBlock + threadIdx.x; // < groups * P_m + 256 <= 2^22 + 256
    const int pm = 1 << grp.log2_pm;
    const int g = thread >> grp.log2_pm, leaf = thread & (pm - 1);
    const bool live = g < grp.groups && leaf < grp.m;
    const size_t e = live ? (size_t)g * (size_t)grp.m + (size_t)leaf : 0; // (dereferenced only where live)
    double x = 0.0;
    if (live) {
        if (is_returns) {
            x = returns[e] * grp.gamma[g] + reward[e];
            returns[e] = x;
        } else {
            x = (double)obs[e * (size_t)c.width + column];
        }
    }
    const double N = (double)grp.m;
    double s = x;
    for (int off = 1; off < pm; off <<= 1)
        s += __shfl_xor(s, off, 64);
    const double bm = (s + 0.0) / N;
    const double d = x - bm;
    s = live ? d * d : 0.0;
    for (int off = 1; off < pm; off <<= 1)
        s += __shfl_xor(s, off, 64);
    const double bv = (s + 0.0) / N;
    if (live && leaf == 0)
        view_update(moments + g, is_returns ? c.width : column, bm, bv, N);
}

__device__ __forceinline__ double view_clip(double z, double limit)
{
    return z < -limit ? -limit : (z > limit ? limit : z); // (a NaN passes through, as numpy.clip lets it)
}

// normalise(row)[c]
__device__ __forceinline__ float view_normalise(const EnvViewConfig &c, const EnvViewMoments *m, int column, float x)
{
    if (!c.norm_obs)
        return x;
    const double z = ((double)x - m->mean[column]) / sqrt(m->var[column] + c.epsilon);
    return (float)view_clip(z, c.clip_obs);
}

// Steps 2 and 4 to 8 of a step, or with reset != 0 the end of a reset; follows env_view_moments_kernel in stream order
// (it needs the updated moments).  One thread per (environment e, column c): it owns column c of all frame_stack slots
// of e's stack row, so the shift is in place without a hazard.  `stack` is the view observation; view_reward and
// view_final ([n][V], null without episode records: raw_final is then null too) are the step's other outputs.  The
// caller's arrays out_obs / out_reward / out_final (rf_env_step_device_view; each may be null) get the same values in
// the same launch.  kGrouped ("population view"): environment e is normalised by the moments of its group,
// moments[e / m]; nothing else differs, and the ungrouped instantiation is the kernel of before.
template <bool kGrouped>
__global__ void env_view_apply_kernel(EnvViewConfig c, int reset, const float *obs, const double *reward,
                                      const uint8_t *truncated, const float *raw_final, const EnvViewMoments *moments,
                                      float *stack, double *returns, double *view_reward, float *view_final,
                                      float *out_obs, double *out_reward, float *out_final, EnvViewGroups grp)
{
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= c.n * c.width)
        return;
    const int e = cell / c.width, column = cell - e * c.width;
    if (kGrouped)
        moments += e / grp.m;
    const bool ended = !reset && truncated[e];
    const bool fresh = reset || ended; // the stack starts over
    const size_t row = (size_t)e * c.frame_stack * c.width;
    const float nan = __builtin_nanf("");
    for (int j = 0; j + 1 < c.frame_stack; ++j) {
        const size_t at = row + (size_t)j * c.width + column;
        const float older = reset ? 0.0f : stack[at + c.width];
        const float kept = fresh ? 0.0f : older;
        stack[at] = kept;
        if (out_obs)
            out_obs[at] = kept;
        if (view_final) {
            const float f = ended ? older : nan;
            view_final[at] = f;
            if (out_final)
                out_final[at] = f;
        }
    }
    const size_t newest = row + (size_t)(c.frame_stack - 1) * c.width + column;
    const float o = view_normalise(c, moments, column, obs[cell]);
    stack[newest] = o;
    if (out_obs)
        out_obs[newest] = o;
    if (view_final) {
        const float f = ended ? view_normalise(c, moments, column, raw_final[cell]) : nan;
        view_final[newest] = f;
        if (out_final)
            out_final[newest] = f;
    }
    if (column == 0) {
        if (!reset) {
            double r = reward[e];
            if (c.norm_reward)
                r = view_clip(r / sqrt(moments->var[c.width] + c.epsilon), c.clip_reward);
            view_reward[e] = r;
            if (out_reward)
                out_reward[e] = r;
        }
        if (fresh)
            returns[e] = 0.0;
    }
}

} // namespace rf
