// rf_rollout.h -- the end of a PPO rollout (include/reinfocus_hip.h, "rollout"): GAE(gamma, lambda) advantages and
// returns over T steps of n environments in one launch, with the bootstrap of truncated steps.  One definition, shared
// with the numpy twin (environments/rollout.py gae_numpy), bit for bit; every operation is float32, left to right, no
// FMA contraction (flags.mk):
//
//   r      = float32(rewards[t][e]);  where final_values is given and truncated[t][e]: r = r + g * final_values[t][e]
//   nnt    = 1.0f - float32(truncated[t][e])
//   next_v = t == T-1 ? last_values[e] : values[t+1][e]
//   delta  = (r + (g * next_v) * nnt) - values[t][e]
//   last   = delta + (gl * nnt) * last          (last = 0.0f before t = T-1; t runs T-1 .. 0)
//   advantages[t][e] = last;  returns[t][e] = last + values[t][e]
//
// The recurrence is sequential in t (a scan over the affine maps would round differently), but delta and gl * nnt do
// not depend on it.  A block of kRolloutThreads threads owns kRolloutTile consecutive environments -- lanes run along
// n, so every global access is coalesced -- and walks T from the end in chunks of kRolloutChunk steps: all four waves
// compute delta, the coefficient and the value of a chunk into LDS (each wave every fourth step, its loads independent
// of one another), then the first wave runs the chain from LDS, two dependent float32 operations per step, and writes
// both outputs.  So 8 environments x 128 steps are four rounds of global-load latency, not 128, and 4096 x 32 is 64
// blocks of one chunk each.  LDS rows are 64 consecutive floats: conflict-free for ds_read_b32 / ds_write_b32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rf {

constexpr int kRolloutTile = 64; // environments of one block: one lane each
constexpr int kRolloutChunk = 32; // steps of one LDS chunk (3 arrays x 32 x 64 x 4 B = 24 KiB per block)
constexpr int kRolloutThreads = 256;

// kGrouped ("population view": rf_rollout_advantages_grouped): the n environments are groups of m consecutive ones
// with discounts of their own, discounts[e / m] = (g, gl) -- a tile of 64 lanes may span groups, and only these two
// coefficients differ per lane; the arguments g and gl are not read.  A template parameter, not a run-time flag: the
// ungrouped instantiation is the kernel of before, instruction for instruction.
template <bool kGrouped>
__global__ __launch_bounds__(kRolloutThreads) void rollout_gae_kernel(
    int T, int n, const double *__restrict__ rewards, const float *__restrict__ values,
    const uint8_t *__restrict__ truncated, const float *__restrict__ final_values /* or null */,
    const float *__restrict__ last_values, float g, float gl, float *__restrict__ advantages, float *__restrict__ returns,
    const float2 *__restrict__ discounts /* [n / m], kGrouped only */, int m)
{
    __shared__ float s_delta[kRolloutChunk][kRolloutTile];
    __shared__ float s_coef[kRolloutChunk][kRolloutTile];
    __shared__ float s_value[kRolloutChunk][kRolloutTile];
    const int lane = threadIdx.x % kRolloutTile, wave = threadIdx.x / kRolloutTile;
    const int e = blockIdx.x * kRolloutTile + lane;
    const bool live = e < n; // (the ragged last tile: its idle lanes touch no memory, and reach every barrier)
    if (kGrouped && live) { // this lane's coefficients
        const float2 mine = discounts[e / m];
        g = mine.x;
        gl = mine.y;
    }
    float last = 0.0f;
    for (int hi = T; hi > 0; hi -= kRolloutChunk) { // the chunk holds steps lo .. hi-1
        const int lo = hi > kRolloutChunk ? hi - kRolloutChunk : 0;
        if (live) {
            for (int t = lo + wave; t < hi; t += kRolloutThreads / kRolloutTile) {
                const size_t i = (size_t)t * (size_t)n + (size_t)e;
                const uint8_t flag = truncated[i];
                const float v = values[i];
                const float next_v = t == T - 1 ? last_values[e] : values[i + (size_t)n];
                float r = (float)rewards[i]; // (the one float64 operation)
                if (final_values != nullptr && flag != 0)
                    r = r + g * final_values[i]; // a select: the NaN of a step that did not end is never read
                const float nnt = 1.0f - (float)flag;
                s_delta[t - lo][lane] = (r + (g * next_v) * nnt) - v;
                s_coef[t - lo][lane] = gl * nnt;
                s_value[t - lo][lane] = v;
            }
        }
        __syncthreads();
        if (wave == 0 && live) {
#pragma unroll 4
            for (int t = hi - 1; t >= lo; --t) {
                const size_t i = (size_t)t * (size_t)n + (size_t)e;
                last = s_delta[t - lo][lane] + s_coef[t - lo][lane] * last;
                advantages[i] = last;
                returns[i] = last + s_value[t - lo][lane];
            }
        }
        __syncthreads(); // (the next chunk overwrites what the chain has read)
    }
}

} // namespace rf
