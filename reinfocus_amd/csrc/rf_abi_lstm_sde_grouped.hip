// rf_abi_lstm_sde_grouped.hip -- "population lstm sde" (include/reinfocus_hip.h): the noise reset, the recurrent forward
// and the recurrent PPO update of the Gaussian head over G groups, one launch per stage.  The entry points live in a
// translation unit of their own for the reason rf_abi_lstm_grouped.hip has one: a further instantiation in a module may
// change a sibling's register allocation (profiles/population_lstm.md, finding 2), so the listings of rf_abi_env.hip and
// rf_abi_lstm_grouped.hip change with this head only through the headers (profiles/population_lstm_sde.md).
#include "rf_host.h"

#include "rf_lstm.h"
#include "rf_lstm_ppo.h"
#include "rf_sde.h"

using namespace rfh;

// (what rf_abi_env.hip says of an lstm-sde desc it refuses)
#define RF_LSTM_SDE_LIMITS "%s: the desc is outside the limits (obs_width and lstm_hidden 1 .. %d, 1 or 2 hidden layers of " \
                           "width 1 .. %d per net, n_actions 1: the Gaussian head has one action, activation RF_POLICY_RELU " \
                           "or RF_POLICY_TANH, critic RF_LSTM_CRITIC_LSTM or RF_LSTM_CRITIC_LINEAR)"
#define RF_POPULATION_LIMITS "%s: G = %d must be in 1 .. %d, m = %d in 1 .. 2^20 and G m at most 2^30"

extern "C" {

// One set for both critic kinds (rf_lstm_critic_desc.critic); the Gaussian head only.

int rf_lstm_sde_noise_reset_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m, const float *d_params,
                                    const unsigned long long *d_gens, const unsigned long long *d_consumed,
                                    const unsigned char *d_select, float *d_theta, void *caller_stream)
{
    const char *fn = "rf_lstm_sde_noise_reset_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_gens != nullptr && d_consumed != nullptr && d_theta != nullptr,
               "%s: NULL argument", fn);
    rf::LstmLayout layout;
    RF_REQUIRE(rf::lstm_layout_nets(desc->lstm, layout, true, desc->critic), RF_LSTM_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH,
               RF_POLICY_MAX_WIDTH);
    RF_REQUIRE(rf::population_rows(G, m) && m <= (1 << 20), RF_POPULATION_LIMITS, fn, G, RF_POPULATION_MAX_GROUPS, m);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t groups = (size_t)G, cells = (size_t)m * (size_t)layout.mlp.sde;
    const DeviceArray inputs[] = {{d_params, groups * (size_t)layout.total * 4, 4, "d_params"},
                                  {d_gens, groups * 32, 8, "d_gens"},
                                  {d_consumed, groups * 8, 8, "d_consumed"},
                                  {d_select, groups, 1, "d_select"}};
    const DeviceArray outputs[] = {{d_theta, groups * cells * 4, 4, "d_theta"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn, 0, nullptr))
        return rc;
    // As rf_sde_noise_reset_grouped: one launch on the caller's stream, nothing allocated, nothing waited for; the
    // generators' words, their draw counts and the selection are read on the device.  log_std is the lstm layout's: the
    // last L floats of each group's piece of P + L.
    static_assert(sizeof(rf::PolicyGen) == 32, "d_gens is uint64 [G][4]");
    const unsigned blocks = (unsigned)((cells + rf::kPolicyThreads - 1) / rf::kPolicyThreads);
    hipLaunchKernelGGL(rf::sde_noise_kernel<true>, dim3(blocks, (unsigned)G), dim3(rf::kPolicyThreads), 0,
                       (hipStream_t)caller_stream, rf::PolicyGen{}, d_params + layout.mlp.log_std, m, (int)layout.mlp.sde,
                       d_theta, (const rf::PolicyGen *)d_gens, (const uint64_t *)d_consumed, (const uint8_t *)d_select,
                       layout.total);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_lstm_sde_forward_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m, const float *d_params,
                                const float *d_obs, const uint8_t *d_episode_starts, const float *d_final_obs,
                                const float *d_state_in, float *d_state_out, const float *d_theta, int flags,
                                float *d_actions, float *d_env_actions, float *d_log_probs, float *d_values,
                                float *d_final_values, float *d_mean, float *d_sigma, void *caller_stream)
{
    const char *fn = "rf_lstm_sde_forward_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_obs != nullptr && d_episode_starts != nullptr &&
               d_state_in != nullptr, "%s: NULL argument", fn);
    rf::LstmLayout layout;
    RF_REQUIRE(rf::lstm_layout_nets(desc->lstm, layout, true, desc->critic), RF_LSTM_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH,
               RF_POLICY_MAX_WIDTH);
    RF_REQUIRE(rf::population_rows(G, m) && m <= (1 << 20), RF_POPULATION_LIMITS, fn, G, RF_POPULATION_MAX_GROUPS, m);
    RF_REQUIRE((flags & ~RF_POLICY_DETERMINISTIC) == 0, "%s: unknown flags %d", fn, flags);
    const bool pi_out = d_actions || d_env_actions || d_log_probs || d_mean || d_sigma;
    RF_REQUIRE(pi_out || d_values || d_final_values || d_state_out, "%s: no output is asked for", fn);
    RF_REQUIRE(d_final_values == nullptr || d_final_obs != nullptr, "%s: d_final_values needs d_final_obs", fn);
    const bool sampled = pi_out && (flags & RF_POLICY_DETERMINISTIC) == 0;
    RF_REQUIRE(!sampled || d_theta != nullptr, "%s: a sampled call needs d_theta (rf_lstm_sde_noise_reset_grouped)", fn);
    RF_HIP(hipSetDevice(ctx->device));
    const int lanes = G * m;
    const size_t rows = (size_t)lanes;
    const size_t state_bytes = rf::lstm_state_floats(lanes, layout.hidden) * 4;
    const DeviceArray inputs[] = {{d_params, (size_t)G * (size_t)layout.total * 4, 4, "d_params"},
                                  {d_obs, rows * (size_t)layout.obs_width * 4, 4, "d_obs"},
                                  {d_episode_starts, rows, 1, "d_episode_starts"},
                                  {d_final_obs, rows * (size_t)layout.obs_width * 4, 4, "d_final_obs"},
                                  {sampled ? d_theta : nullptr, rows * (size_t)layout.mlp.sde * 4, 4, "d_theta"},
                                  {d_state_in, state_bytes, 4, "d_state_in"}};
    const DeviceArray outputs[] = {{d_actions, rows * 4, 4, "d_actions"},       {d_env_actions, rows * 4, 4, "d_env_actions"},
                                   {d_log_probs, rows * 4, 4, "d_log_probs"},   {d_values, rows * 4, 4, "d_values"},
                                   {d_final_values, rows * 4, 4, "d_final_values"}, {d_mean, rows * 4, 4, "d_mean"},
                                   {d_sigma, rows * 4, 4, "d_sigma"},           {d_state_out, state_bytes, 4, "d_state_out"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn, kStateInPlace))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // As rf_lstm_forward_grouped: one launch on the caller's stream, nothing allocated, nothing waited for.  Nothing is
    // drawn (the noise is theta), so no generator travels.  The state is one [2][2][G m][H] array: the kernel is given its
    // plane stride G m next to the group's m.
    const bool linear = desc->critic == RF_LSTM_CRITIC_LINEAR;
    const bool pi = pi_out || d_state_out != nullptr;
    const bool vf = d_values != nullptr || d_final_values != nullptr || (!linear && d_state_out != nullptr);
    const unsigned tiles = (unsigned)(((size_t)m + rf::kPolicyTile - 1) / rf::kPolicyTile);
    const auto kernel = linear ? rf::lstm_forward_kernel<true, true, true> : rf::lstm_forward_kernel<true, false, true>;
    hipLaunchKernelGGL(kernel, dim3(tiles, pi && vf ? 2u : 1u, (unsigned)G), dim3(rf::kPolicyThreads), 0, caller, layout,
                       d_params, m, d_obs, d_episode_starts, d_final_obs, d_state_in, d_state_out, rf::PolicyGen{}, 0,
                       pi ? 0 : 1, d_actions, d_log_probs, d_values, d_final_values, d_mean,
                       rf::LstmSde{sampled ? d_theta : nullptr, d_env_actions, d_sigma}, (const rf::PolicyGen *)nullptr,
                       (uint64_t)0, lanes);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

unsigned long long rf_lstm_sde_grouped_state_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m)
{
    if (ctx == nullptr || desc == nullptr)
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return rf::lstm_population_state_bytes(*desc, G, m, true);
}

unsigned long long rf_lstm_sde_grouped_workspace_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m, int T,
                                                     int B)
{
    if (ctx == nullptr || desc == nullptr)
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return rf::lstm_population_workspace_bytes(*desc, G, m, T, B, true);
}

int rf_lstm_sde_update_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m, int T, const rf_ppo_hyper *d_hyper,
                               float *d_params, void *d_state, void *d_workspace, const float *d_observations,
                               const float *d_actions, const float *d_log_probs, const float *d_advantages,
                               const float *d_returns, const uint8_t *d_episode_starts, const float *d_lstm_states,
                               const int *d_firsts, int B, float *d_stats, void *caller_stream)
{
    const char *fn = "rf_lstm_sde_update_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_HIP(hipSetDevice(ctx->device));
    RF_REQUIRE(desc && d_hyper && d_params && d_state && d_workspace && d_observations && d_actions && d_log_probs &&
               d_advantages && d_returns && d_episode_starts && d_lstm_states && d_firsts && d_stats, "%s: NULL argument",
               fn);
    rf::LstmLayout layout;
    RF_REQUIRE(rf::lstm_layout_nets(desc->lstm, layout, true, desc->critic), RF_LSTM_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH,
               RF_POLICY_MAX_WIDTH);
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
                                  {d_actions, rows * 4, 4, "d_actions"},
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
    // As rf_lstm_ppo_update_grouped: six launches on the caller's stream whatever G is, nothing allocated, nothing waited
    // for.  The forward, BPTT, norm and Adam kernels are the Categorical population's (over P + L parameters); the MLP and
    // gradient kernels are the Gaussian head's.
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
    const auto mlp = rf::lstm_ppo_mlp_kernel<true, true>;
    hipLaunchKernelGGL(mlp, dim3(tiles, 2u, groups_z), threads, 0, caller, layout, work, rf::PpoHyper{},
                       (const float *)d_params, (const rf::PpoHeader *)d_state, ws, N, (const void *)d_actions, d_log_probs,
                       d_advantages, d_returns, 0, B, hypers, d_firsts);
    RF_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf::lstm_ppo_bptt_kernel<true>, dim3((unsigned)B, walks, groups_z), threads, 0, caller, layout, work,
                       (const float *)d_params, ws, T, m, d_episode_starts, 0, B, d_firsts, lanes);
    RF_HIP(hipGetLastError());
    const auto gradient = linear ? rf::lstm_ppo_gradient_kernel<true, true, true>
                                 : rf::lstm_ppo_gradient_kernel<true, false, true>;
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
