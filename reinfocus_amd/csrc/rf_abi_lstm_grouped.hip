// rf_abi_lstm_grouped.hip -- "population lstm" (include/reinfocus_hip.h): the recurrent forward and the recurrent PPO
// update over G groups, one launch per stage.  The entry points live in a translation unit of their own so that the
// grouped instantiations of rf_lstm.h and rf_lstm_ppo.h are compiled apart from the ungrouped ones of rf_abi_env.hip:
// side by side in one module the optimiser orders the ungrouped BPTT kernel's address arithmetic differently and it takes
// 75 VGPRs instead of 71, 6 waves per SIMD instead of 7 (profiles/population_lstm.md).
#include "rf_host.h"

#include "rf_lstm.h"
#include "rf_lstm_ppo.h"

using namespace rfh;

extern "C" {

// One set for both critic kinds (rf_lstm_critic_desc.critic); the Categorical head only.

int rf_lstm_forward_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m, const float *d_params,
                            const float *d_obs, const uint8_t *d_episode_starts, const float *d_final_obs,
                            const float *d_state_in, float *d_state_out, const unsigned long long *d_gens,
                            unsigned long long consumed, int flags, long long *d_actions, float *d_log_probs,
                            float *d_values, float *d_final_values, float *d_logits, void *caller_stream)
{
    const char *fn = "rf_lstm_forward_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_obs != nullptr && d_episode_starts != nullptr &&
               d_state_in != nullptr, "%s: NULL argument", fn);
    rf::LstmLayout layout;
    RF_REQUIRE(rf::lstm_layout_nets(desc->lstm, layout, false, desc->critic), RF_LSTM_LIMITS, fn, RF_POLICY_MAX_WIDTH,
               RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_ACTIONS);
    RF_REQUIRE(rf::population_rows(G, m), "%s: G = %d must be in 1 .. %d, m = %d at least 1 and G m at most 2^30", fn, G,
               RF_POPULATION_MAX_GROUPS, m);
    RF_REQUIRE((flags & ~RF_POLICY_DETERMINISTIC) == 0, "%s: unknown flags %d", fn, flags);
    RF_REQUIRE(d_actions || d_values || d_final_values || d_logits || d_state_out, "%s: no output is asked for", fn);
    RF_REQUIRE(d_log_probs == nullptr || d_actions != nullptr, "%s: d_log_probs are those of d_actions, which is NULL", fn);
    RF_REQUIRE(d_final_values == nullptr || d_final_obs != nullptr, "%s: d_final_values needs d_final_obs", fn);
    const bool sampled = d_actions != nullptr && (flags & RF_POLICY_DETERMINISTIC) == 0;
    RF_REQUIRE(!sampled || d_gens != nullptr, "%s: a sampled call needs d_gens", fn);
    RF_HIP(hipSetDevice(ctx->device));
    const int lanes = G * m;
    const size_t rows = (size_t)lanes;
    const size_t state_bytes = rf::lstm_state_floats(lanes, layout.hidden) * 4;
    const DeviceArray inputs[] = {{d_params, (size_t)G * (size_t)layout.total * 4, 4, "d_params"},
                                  {d_obs, rows * (size_t)layout.obs_width * 4, 4, "d_obs"},
                                  {d_episode_starts, rows, 1, "d_episode_starts"},
                                  {d_final_obs, rows * (size_t)layout.obs_width * 4, 4, "d_final_obs"},
                                  {d_state_in, state_bytes, 4, "d_state_in"},
                                  {sampled ? d_gens : nullptr, (size_t)G * 32, 8, "d_gens"}};
    const DeviceArray outputs[] = {{d_actions, rows * 8, 8, "d_actions"},
                                   {d_log_probs, rows * 4, 4, "d_log_probs"},
                                   {d_values, rows * 4, 4, "d_values"},
                                   {d_final_values, rows * 4, 4, "d_final_values"},
                                   {d_logits, rows * (size_t)layout.mlp.n_actions * 4, 4, "d_logits"},
                                   {d_state_out, state_bytes, 4, "d_state_out"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn, kStateInPlace))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // As rf_lstm_forward: one launch on the caller's stream, nothing allocated, nothing waited for; the generators' words
    // are read on the device and the draw count travels by value.  The state is one [2][2][G m][H] array: the kernel is
    // given its plane stride G m next to the group's m.
    static_assert(sizeof(rf::PolicyGen) == 32, "d_gens is uint64 [G][4]");
    const bool linear = desc->critic == RF_LSTM_CRITIC_LINEAR;
    const bool pi = d_actions != nullptr || d_logits != nullptr || d_state_out != nullptr;
    const bool vf = d_values != nullptr || d_final_values != nullptr || (!linear && d_state_out != nullptr);
    const unsigned tiles = (unsigned)(((size_t)m + rf::kPolicyTile - 1) / rf::kPolicyTile);
    const auto kernel = linear ? rf::lstm_forward_kernel<false, true, true> : rf::lstm_forward_kernel<false, false, true>;
    hipLaunchKernelGGL(kernel, dim3(tiles, pi && vf ? 2u : 1u, (unsigned)G), dim3(rf::kPolicyThreads), 0, caller, layout,
                       d_params, m, d_obs, d_episode_starts, d_final_obs, d_state_in, d_state_out, rf::PolicyGen{},
                       sampled ? 1 : 0, pi ? 0 : 1, (int64_t *)d_actions, d_log_probs, d_values, d_final_values, d_logits,
                       rf::LstmNoSde{}, (const rf::PolicyGen *)(sampled ? d_gens : nullptr), (uint64_t)consumed, lanes);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

unsigned long long rf_lstm_ppo_grouped_state_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m)
{
    if (ctx == nullptr || desc == nullptr)
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return rf::lstm_population_state_bytes(*desc, G, m);
}

unsigned long long rf_lstm_ppo_grouped_workspace_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m, int T,
                                                     int B)
{
    if (ctx == nullptr || desc == nullptr)
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return rf::lstm_population_workspace_bytes(*desc, G, m, T, B);
}

int rf_lstm_ppo_update_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m, int T, const rf_ppo_hyper *d_hyper,
                               float *d_params, void *d_state, void *d_workspace, const float *d_observations,
                               const long long *d_actions, const float *d_log_probs, const float *d_advantages,
                               const float *d_returns, const uint8_t *d_episode_starts, const float *d_lstm_states,
                               const int *d_firsts, int B, float *d_stats, void *caller_stream)
{
    const char *fn = "rf_lstm_ppo_update_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_HIP(hipSetDevice(ctx->device));
    RF_REQUIRE(desc && d_hyper && d_params && d_state && d_workspace && d_observations && d_actions && d_log_probs &&
               d_advantages && d_returns && d_episode_starts && d_lstm_states && d_firsts && d_stats, "%s: NULL argument",
               fn);
    rf::LstmLayout layout;
    RF_REQUIRE(rf::lstm_layout_nets(desc->lstm, layout, false, desc->critic), RF_LSTM_LIMITS, fn, RF_POLICY_MAX_WIDTH,
               RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_ACTIONS);
    RF_REQUIRE(m >= 1 && T >= 1 && rf::population_rows(G, (long long)m * (long long)T),
               "%s: G = %d must be in 1 .. %d, m = %d and T = %d at least 1 and G m T at most 2^30", fn, G,
               RF_POPULATION_MAX_GROUPS, m, T);
    const int N = m * T, lanes = G * m;
    const int most = N < RF_PPO_MAX_BATCH ? N : RF_PPO_MAX_BATCH;
    RF_REQUIRE(B >= 1 && B <= most, "%s: B = %d is not in 1 .. %d (min(m T, %d))", fn, B, most, RF_PPO_MAX_BATCH);
    rf::LstmPpoWork work;
    RF_REQUIRE(rf::lstm_ppo_work(layout, B, work), "%s: no workspace layout for B = %d", fn, B);
    const size_t groups = (size_t)G, rows = groups * (size_t)N, slab = (size_t)(T + 1) * (size_t)lanes;
    const size_t state_floats = (size_t)rf::kPpoStateHeader + 2 * (size_t)layout.total;
    const DeviceArray inputs[] = {{d_observations, rows * (size_t)layout.obs_width * 4, 4, "d_observations"},
                                  {d_actions, rows * 8, 8, "d_actions"},
                                  {d_log_probs, rows * 4, 4, "d_log_probs"},
                                  {d_advantages, rows * 4, 4, "d_advantages"},
                                  {d_returns, rows * 4, 4, "d_returns"},
                                  {d_episode_starts, slab, 1, "d_episode_starts"},
                                  {d_lstm_states, slab * 4 * (size_t)layout.hidden * 4, 4, "d_lstm_states"},
                                  {d_firsts, groups * 4, 4, "d_firsts"},
                                  {d_hyper, groups * sizeof(rf_ppo_hyper), 8, "d_hyper"}};
    const DeviceArray outputs[] = {{d_params, groups * (size_t)layout.total * 4, 4, "d_params"},
                                   {d_state, groups * state_floats * 4, 8, "d_state"},
                                   {d_workspace, groups * (size_t)work.total * 4, 8, "d_workspace"},
                                   {d_stats, groups * 32, 4, "d_stats"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // As rf_lstm_ppo_update: six launches on the caller's stream whatever G is, nothing allocated, nothing waited for;
    // the workspace of a group has the layout of B itself, and every group's first row is read on the device.
    float *ws = (float *)d_workspace;
    const rf::PpoHyper *hypers = (const rf::PpoHyper *)d_hyper;
    const dim3 threads(rf::kPpoThreads);
    const unsigned groups_z = (unsigned)G;
    const bool linear = desc->critic == RF_LSTM_CRITIC_LINEAR;
    const unsigned tiles = (unsigned)((B + rf::kPolicyTile - 1) / rf::kPolicyTile);
    const unsigned walks = linear ? 1u : 2u;
    const auto forward = linear ? rf::lstm_ppo_forward_kernel<true, true> : rf::lstm_ppo_forward_kernel<false, true>;
    hipLaunchKernelGGL(forward, dim3((unsigned)B + (linear ? tiles : 0u), walks, groups_z), threads, 0, caller, layout, work,
                       (const float *)d_params, ws, T, m, d_observations, d_episode_starts, d_lstm_states, 0, B, d_firsts,
                       lanes);
    RF_HIP(hipGetLastError());
    const auto mlp = rf::lstm_ppo_mlp_kernel<false, true>;
    hipLaunchKernelGGL(mlp, dim3(tiles, 2u, groups_z), threads, 0, caller, layout, work, rf::PpoHyper{},
                       (const float *)d_params, (const rf::PpoHeader *)d_state, ws, N, (const void *)d_actions, d_log_probs,
                       d_advantages, d_returns, 0, B, hypers, d_firsts);
    RF_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf::lstm_ppo_bptt_kernel<true>, dim3((unsigned)B, walks, groups_z), threads, 0, caller, layout, work,
                       (const float *)d_params, ws, T, m, d_episode_starts, 0, B, d_firsts, lanes);
    RF_HIP(hipGetLastError());
    const auto gradient = linear ? rf::lstm_ppo_gradient_kernel<false, true, true>
                                 : rf::lstm_ppo_gradient_kernel<false, false, true>;
    hipLaunchKernelGGL(gradient, dim3(work.mlp.partials, groups_z), threads, 0, caller, layout, work, ws, B,
                       (const float *)d_params);
    RF_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf::lstm_ppo_norm_kernel<true>, dim3(work.supers, groups_z), dim3(rf::kLstmPpoGroup), 0, caller, work,
                       ws);
    RF_HIP(hipGetLastError());
    const unsigned slices = (layout.total + rf::kPpoAdamSlice - 1) / rf::kPpoAdamSlice;
    hipLaunchKernelGGL(rf::ppo_adam_kernel<true>, dim3(slices + 1u, groups_z), threads, 0, caller, layout.total,
                       rf::lstm_ppo_adam_work(work), rf::PpoHyper{}, d_params, (float *)d_state, (const float *)ws, B,
                       d_stats, hypers);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

} // extern "C"
