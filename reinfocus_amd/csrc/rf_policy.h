// rf_policy.h -- the PPO actor-critic forward with sampling in one launch (include/reinfocus_hip.h, "policy"):
// stable-baselines3's MlpPolicy with separate pi / vf nets and a Categorical head, in the fixed float32 order of the
// definition (rf_policy_math.h holds the scalar functions, shared with the host build of tests/policycheck), bit for
// bit equal to the numpy twin (environments/policy.py policy_numpy).
//
// A block of kPolicyThreads threads owns ONE net (blockIdx.y: pi or vf) and a tile of kPolicyTile consecutive
// environments.  Hidden layers: thread j owns hidden unit j and keeps one accumulator per environment of the tile
// (indexed by the constants of an unrolled loop: registers); parameters are stored transposed, [in][out], so the
// weight loads of a wave are 64 consecutive floats and each weight is read once per block; the tile's inputs and
// activations live in LDS as [k][tile], so the eight inputs of one k are two ds_read_b128 that every lane reads at the
// same address (a broadcast).  Heads: one chain per (output, environment) lane, outputs fastest, so the head's weight
// loads are consecutive too.  Then one lane per environment runs the softmax, the draw and the selection.  vf blocks
// run a second pass over final_obs.  No atomics; the ragged last tile computes on zeros and stores nothing.
// PolicyLayout and policy_layout are plain C++: tests/policycheck packs its host loop by the same offsets.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "rf_policy_math.h"

namespace rf {

constexpr int kPolicyTile = 8; // environments of one block (no result depends on it)
constexpr int kPolicyThreads = 256;
constexpr int kPolicyMaxWidth = RF_POLICY_MAX_WIDTH, kPolicyMaxActions = RF_POLICY_MAX_ACTIONS;
static_assert(kPolicyMaxWidth <= kPolicyThreads, "one thread per hidden unit");

// A checked rf_policy_desc as the kernel reads it: net 0 is pi, net 1 is vf; offsets in floats into the parameters
struct PolicyLayout {
    int obs_width, n_actions, activation;
    int layers[2];
    int width[2][2];
    unsigned weight[2][3], bias[2][3]; // [net][hidden layer 0, 1 or (at index `layers`) the head]
    unsigned total;
    unsigned log_std, sde; // the Gaussian head (sde_layout): log_std [sde] sits at `log_std`, after everything else; else 0
};

struct PolicyGen {
    uint64_t word[4]; // state low, state high, inc low, inc high
};

// The packing of both heads; min_actions is 2 for the Categorical head and 1 for the Gaussian one
RF_HD bool policy_layout_nets(const rf_policy_desc &d, PolicyLayout &p, int min_actions)
{
    p = PolicyLayout{};
    if (d.obs_width < 1 || d.obs_width > kPolicyMaxWidth || d.n_actions < min_actions || d.n_actions > kPolicyMaxActions)
        return false;
    if (d.activation != kPolicyRelu && d.activation != kPolicyTanh)
        return false;
    p.obs_width = d.obs_width;
    p.n_actions = d.n_actions;
    p.activation = d.activation;
    unsigned at = 0;
    for (int net = 0; net < 2; ++net) {
        const int layers = net == 0 ? d.pi_layers : d.vf_layers;
        const int *width = net == 0 ? d.pi_width : d.vf_width;
        if (layers < 1 || layers > 2)
            return false;
        p.layers[net] = layers;
        int in = d.obs_width;
        for (int l = 0; l <= layers; ++l) {
            const int out = l < layers ? width[l] : (net == 0 ? d.n_actions : 1);
            if (out < 1 || out > kPolicyMaxWidth)
                return false;
            if (l < layers)
                p.width[net][l] = out;
            p.weight[net][l] = at;
            at += (unsigned)(in * out);
            p.bias[net][l] = at;
            at += (unsigned)out;
            in = out;
        }
    }
    p.total = at;
    return true;
}

// false: desc is outside the limits of the definition
RF_HD bool policy_layout(const rf_policy_desc &d, PolicyLayout &p)
{
    return policy_layout_nets(d, p, 2);
}

// The Gaussian head of "sde policy": one action (n_actions must be 1: the mean), log_std [last pi width] packed last
RF_HD bool sde_layout(const rf_policy_desc &d, PolicyLayout &p)
{
    if (d.n_actions != 1 || !policy_layout_nets(d, p, 1))
        return false;
    p.log_std = p.total;
    p.sde = (unsigned)p.width[0][p.layers[0] - 1];
    p.total = p.log_std + p.sde;
    return true;
}

#if defined(__HIPCC__)
// One hidden layer of a block's tile (shared with ppo_backward_kernel, rf_ppo.h): thread j < H owns unit j with one
// accumulator per row of the tile; in / out are [k][tile] in LDS.  The caller puts a barrier after it.
__device__ __forceinline__ void policy_hidden_tile(const float *__restrict__ params, unsigned weight, unsigned bias, int K,
                                                   int H, int activation, const float (*in)[kPolicyTile],
                                                   float (*out)[kPolicyTile], int tid)
{
    if (tid < H) {
        const float *__restrict__ w = params + weight + tid;
        const float b = params[bias + tid];
        float acc[kPolicyTile];
#pragma unroll
        for (int e = 0; e < kPolicyTile; ++e)
            acc[e] = b;
#pragma unroll 8
        for (int k = 0; k < K; ++k) { // (unrolled: 8 independent weight loads in flight per round of latency)
            const float wk = w[(size_t)k * (size_t)H];
            const float4 *x = reinterpret_cast<const float4 *>(&in[k][0]);
            float xs[kPolicyTile];
#pragma unroll
            for (int v = 0; v < kPolicyTile / 4; ++v) {
                const float4 q = x[v];
                xs[4 * v] = q.x, xs[4 * v + 1] = q.y, xs[4 * v + 2] = q.z, xs[4 * v + 3] = q.w;
            }
#pragma unroll
            for (int e = 0; e < kPolicyTile; ++e)
                acc[e] = acc[e] + xs[e] * wk;
        }
#pragma unroll
        for (int e = 0; e < kPolicyTile; ++e)
            out[tid][e] = policy_activation(acc[e], activation);
    }
}

// kGrouped ("population"): grid (ceil(n / kPolicyTile), nets, G) with n the environments of ONE group.  Block (., ., g) is
// a block of the ungrouped kernel over group g's rows -- rows [g n, (g + 1) n) of every array -- with the parameters
// params + g P and the generator gens[g], whose draw number consumed + (row - g n) the row takes.  Tiles are cut per
// group: none spans two groups, and the ragged last tile of each group computes on zeros.  Ungrouped, gens and consumed
// are unused and the code is what it was without them.
template <bool kGrouped>
__global__ __launch_bounds__(kPolicyThreads) void policy_forward_kernel(
    PolicyLayout L, const float *__restrict__ params, int n, const float *__restrict__ obs,
    const float *__restrict__ final_obs /* or null */, PolicyGen gen, int sampled, int first_net,
    int64_t *__restrict__ actions, float *__restrict__ log_probs, float *__restrict__ values,
    float *__restrict__ final_values, float *__restrict__ logits, const PolicyGen *__restrict__ gens /* [G] or null */,
    uint64_t consumed)
{
    __shared__ __align__(16) float s_act[2][kPolicyMaxWidth][kPolicyTile]; // inputs / activations, [k][environment]
    __shared__ float s_logit[kPolicyTile][kPolicyMaxActions];
    __shared__ float s_sum[kPolicyTile][kPolicyMaxActions];
    if (kGrouped) { // (block-uniform: every pointer moves to the group's piece; null stays null)
        const size_t g = blockIdx.z, row = g * (size_t)n, cell = row * (size_t)L.obs_width;
        params += g * (size_t)L.total;
        obs += cell;
        final_obs = final_obs != nullptr ? final_obs + cell : nullptr;
        actions = actions != nullptr ? actions + row : nullptr;
        log_probs = log_probs != nullptr ? log_probs + row : nullptr;
        values = values != nullptr ? values + row : nullptr;
        final_values = final_values != nullptr ? final_values + row : nullptr;
        logits = logits != nullptr ? logits + row * (size_t)L.n_actions : nullptr;
        if (sampled)
            gen = gens[g];
    }
    const int tid = threadIdx.x;
    const int net = (int)blockIdx.y + first_net;
    const int e0 = (int)blockIdx.x * kPolicyTile;
    const int D = L.obs_width;
    for (int pass = 0; pass < 2; ++pass) { // (block-uniform: every thread reaches every barrier)
        const float *__restrict__ in = pass == 0 ? obs : final_obs;
        if (pass == 1 && (net == 0 || final_values == nullptr))
            break;
        if (pass == 0 && net == 1 && values == nullptr)
            continue;
        // the tile's rows are consecutive in memory: element i of the tile is row i / D, column i % D
        for (int i = tid; i < D * kPolicyTile; i += kPolicyThreads) {
            const int e = i / D, k = i - e * D;
            s_act[0][k][e] = e0 + e < n ? in[(size_t)e0 * (size_t)D + (size_t)i] : 0.0f;
        }
        __syncthreads();
        int cur = 0, K = D;
        for (int layer = 0; layer < L.layers[net]; ++layer) {
            const int H = L.width[net][layer];
            policy_hidden_tile(params, L.weight[net][layer], L.bias[net][layer], K, H, L.activation, s_act[cur],
                               s_act[cur ^ 1], tid);
            __syncthreads();
            cur ^= 1;
            K = H;
        }
        const int head = L.layers[net];
        const int O = net == 0 ? L.n_actions : 1;
        for (int i = tid; i < O * kPolicyTile; i += kPolicyThreads) {
            const int e = i / O, o = i - e * O;
            const float y = policy_dot(&s_act[cur][0][e], kPolicyTile, params + L.weight[net][head] + o, O,
                                       params[L.bias[net][head] + o], K);
            const int env = e0 + e;
            if (net == 0) {
                s_logit[e][o] = y;
                if (logits != nullptr && env < n)
                    logits[(size_t)env * (size_t)O + (size_t)o] = policy_canonical(y);
            } else if (env < n) {
                if (pass == 0)
                    values[env] = policy_canonical(y);
                else {
                    const float lead = in[(size_t)env * (size_t)D];
                    final_values[env] = lead != lead ? bits_f32(kPolicyNaN) : policy_canonical(y);
                }
            }
        }
        __syncthreads();
        if (net == 0 && actions != nullptr && tid < kPolicyTile && e0 + tid < n) {
            const int env = e0 + tid;
            const double u = sampled ? policy_draw(gen.word, kGrouped ? consumed + (uint64_t)env : (uint64_t)env) : 0.0;
            int64_t action;
            float log_prob;
            policy_head(&s_logit[tid][0], L.n_actions, !sampled, u, &s_sum[tid][0], &action, &log_prob);
            actions[env] = action;
            if (log_probs != nullptr)
                log_probs[env] = log_prob;
        }
        __syncthreads(); // (the second pass overwrites what the heads have read)
    }
}
#endif

} // namespace rf
