// rf_sde.h -- the state-dependent-exploration Gaussian actor-critic (include/reinfocus_hip.h, "sde policy"):
// stable-baselines3's ActorCriticPolicy(use_sde=True) for a one-dimensional Box, as the reference's PPO configurations
// train ContinuousJumps-v0.  The scalar arithmetic is rf_policy_math.h (normal32, expw32, sde_*), shared with the host
// build of tests/sdecheck, and bit for bit equal to the numpy twin (environments/sde.py).
//
//   sde_noise_kernel    one thread per (environment, unit): theta[e][k] = normal32(draw e * L + k) * exp(log_std_k); the
//                       draw is reached by jump-ahead from the four words the host passed, as policy_draw does.
//   sde_forward_kernel  policy_forward_kernel's blocks (one net, a tile of kPolicyTile environments; policy_hidden_tile
//                       and policy_dot of rf_policy.h), with the Gaussian head: the pi block keeps the last hidden
//                       activations of its tile in LDS, thread k squares exp(log_std_k) once, and one lane per
//                       environment runs the three chains over k -- the mean, the theta dot product and the variance.
// The update is rf_ppo.h's three kernels with the Gaussian head compiled in (ppo_backward_kernel<true>).
// Both kernels are templates over kGrouped ("population sde": G groups of n environments each in one launch, every group
// with its own parameters, generator and draw count); the ungrouped instantiations are the kernels they were.
#pragma once

#include "rf_ppo.h"

namespace rf {

// theta[e][k] of "sde policy": draw number e * L + k of the generator
RF_HD float sde_theta(const uint64_t gen[4], uint64_t i, float log_std)
{
    return policy_canonical(normal32(policy_draw(gen, i)) * expw32(log_std));
}

#if defined(__HIPCC__)
// kGrouped ("population sde"): grid (ceil(n L / kPolicyThreads), G) with n the environments of ONE group.  Block (., g) is
// a block of the ungrouped kernel over group g's rows of theta -- rows [g n, (g + 1) n) -- with the generator gens[g], whose
// draw number consumed[g] + e L + k the cell takes (64-bit), and the log_std of the group's parameters, log_std + g stride.
// A group whose select byte is 0 writes nothing (null selects every group).  Ungrouped, the four last arguments are unused
// and the code is what it was without them.
template <bool kGrouped>
__global__ __launch_bounds__(kPolicyThreads) void sde_noise_kernel(PolicyGen gen, const float *__restrict__ log_std, int n,
                                                                   int L, float *__restrict__ theta,
                                                                   const PolicyGen *__restrict__ gens /* [G] or null */,
                                                                   const uint64_t *__restrict__ consumed /* [G] or null */,
                                                                   const uint8_t *__restrict__ select /* [G] or null */,
                                                                   unsigned stride)
{
    uint64_t first = 0;
    if (kGrouped) { // (block-uniform; the test on select comes first)
        const size_t g = blockIdx.y;
        if (select != nullptr && select[g] == 0)
            return;
        gen = gens[g];
        first = consumed[g];
        log_std += g * (size_t)stride;
        theta += g * (size_t)n * (size_t)L;
    }
    const size_t i = (size_t)blockIdx.x * (size_t)kPolicyThreads + (size_t)threadIdx.x;
    if (i < (size_t)n * (size_t)L)
        theta[i] = sde_theta(gen.word, kGrouped ? first + (uint64_t)i : (uint64_t)i, log_std[i % (size_t)L]);
}

// kGrouped ("population sde"): grid (ceil(n / kPolicyTile), nets, G) as policy_forward_kernel<true>: block (., ., g) is a
// block of the ungrouped kernel over group g's rows of every array, with the parameters params + g (P + L) -- so s_std2 is
// the group's own log_std -- and the group's rows of theta.  Tiles are cut per group.  Only params moves to the group's
// piece; the rows are reached as row0 + env through the kernel's own argument pointers: moving all eleven (nine nullable)
// pointers at the top, as policy_forward_kernel<true> does, took this kernel from 39 to 92 VGPRs and from 8 to 5 waves per
// SIMD (profiles/population_sde.md).  Ungrouped, row0 is the constant 0 and the code is what it was.
template <bool kGrouped>
__global__ __launch_bounds__(kPolicyThreads) void sde_forward_kernel(
    PolicyLayout L, const float *__restrict__ params, int n, const float *__restrict__ obs,
    const float *__restrict__ final_obs /* or null */, const float *__restrict__ theta /* null: deterministic */,
    int first_net, float *__restrict__ actions, float *__restrict__ env_actions, float *__restrict__ log_probs,
    float *__restrict__ values, float *__restrict__ final_values, float *__restrict__ mean, float *__restrict__ sigma)
{
    __shared__ __align__(16) float s_act[2][kPolicyMaxWidth][kPolicyTile]; // inputs / activations, [k][environment]
    __shared__ float s_std2[kPolicyMaxWidth];
    if (kGrouped)
        params += (size_t)blockIdx.z * (size_t)L.total;
    const size_t row0 = kGrouped ? (size_t)blockIdx.z * (size_t)n : 0;
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
        for (int i = tid; i < D * kPolicyTile; i += kPolicyThreads) {
            const int e = i / D, k = i - e * D;
            s_act[0][k][e] = e0 + e < n ? in[(row0 + (size_t)e0) * (size_t)D + (size_t)i] : 0.0f;
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
        if (net == 0) {
            if (tid < K)
                s_std2[tid] = sde_std2(params[L.log_std + tid]);
            __syncthreads();
            const int env = e0 + tid;
            if (tid < kPolicyTile && env < n) {
                const size_t at = row0 + (size_t)env;
                const float *h = &s_act[cur][0][tid];
                const float mu = policy_dot(h, kPolicyTile, params + L.weight[0][head], 1, params[L.bias[0][head]], K);
                const float s = sde_sigma(h, kPolicyTile, s_std2, K);
                float a = mu;
                if (theta != nullptr)
                    a = mu + policy_dot(h, kPolicyTile, theta + at * (size_t)K, 1, 0.0f, K);
                if (actions != nullptr)
                    actions[at] = policy_canonical(a);
                if (env_actions != nullptr)
                    env_actions[at] = sde_env_action(a);
                if (log_probs != nullptr)
                    log_probs[at] = sde_log_prob(a, mu, s);
                if (mean != nullptr)
                    mean[at] = policy_canonical(mu);
                if (sigma != nullptr)
                    sigma[at] = policy_canonical(s);
            }
        } else {
            const int env = e0 + tid;
            if (tid < kPolicyTile && env < n) {
                const size_t at = row0 + (size_t)env;
                const float y = policy_dot(&s_act[cur][0][tid], kPolicyTile, params + L.weight[1][head], 1,
                                           params[L.bias[1][head]], K);
                if (pass == 0)
                    values[at] = policy_canonical(y);
                else {
                    const float lead = in[at * (size_t)D];
                    final_values[at] = lead != lead ? bits_f32(kPolicyNaN) : policy_canonical(y);
                }
            }
        }
        __syncthreads(); // (the second pass overwrites what the heads have read)
    }
}
#endif

} // namespace rf
