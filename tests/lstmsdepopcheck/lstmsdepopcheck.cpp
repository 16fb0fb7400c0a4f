// lstmsdepopcheck.cpp -- TEST INFRASTRUCTURE.  Compiles what "population lstm sde" (include/reinfocus_hip.h) adds to
// reinfocus_amd/csrc/rf_lstm.h and rf_lstm_ppo.h in plain C++ for the host: the size rules
// rf_lstm_sde_grouped_state_size and rf_lstm_sde_grouped_workspace_size return and the grouped addressing of the Gaussian
// head (a group's rows of theta, its float32 raw actions, its log_std), so that a CPU-only test can hold them to the
// header's words before any GPU sees them; and the grouped noise reset, forward and update as loops over the groups of
// tests/lstmsdecheck's host loops, reached through that addressing (the LSTM critic: what those loops compute).  With
// -DLSTMSDEPOPCHECK_MAIN the same source is a stand-alone program.  Never loaded by the product package.
#include "../lstmsdecheck/lstmsdecheck.cpp"

extern "C" {

unsigned long long lspop_state_size(const rf_lstm_critic_desc *desc, int G, int m)
{
    return lstm_population_state_bytes(*desc, G, m, true);
}

unsigned long long lspop_workspace_size(const rf_lstm_critic_desc *desc, int G, int m, int T, int B)
{
    return lstm_population_workspace_bytes(*desc, G, m, T, B, true);
}

// offsets in floats of group g's pieces: its rows of theta [G m][L], its raw actions [G N] (N = m T), its log_std inside
// params [G][P + L]; *total receives P + L, *latent L.  -1 for a desc outside the limits.
int lspop_offsets(const rf_lstm_critic_desc *desc, int m, int T, int g, unsigned long long *theta, unsigned long long *actions,
                  unsigned long long *log_std, unsigned *total, unsigned *latent)
{
    LstmLayout L;
    if (!lstm_layout_nets(desc->lstm, L, true, desc->critic))
        return -1;
    *theta = lstm_sde_group_theta(L, m, (size_t)g);
    *actions = lstm_sde_group_actions((size_t)g, m * T);
    *log_std = lstm_sde_group_log_std(L, (size_t)g);
    *total = L.total, *latent = L.mlp.sde;
    return 0;
}

// rf_lstm_sde_noise_reset_grouped on host arrays (S2): gens [G][4], consumed [G], select [G] or NULL
int lspop_noise(const rf_lstm_critic_desc *desc, int G, int m, const float *params, const unsigned long long *gens,
                const unsigned long long *consumed, const unsigned char *select, float *theta)
{
    LstmLayout L;
    if (!lstm_layout_nets(desc->lstm, L, true, desc->critic) || !population_rows(G, m))
        return -1;
    const size_t latent = L.mlp.sde;
    for (int g = 0; g < G; ++g) {
        if (select != nullptr && select[g] == 0)
            continue;
        const uint64_t words[4] = {gens[4 * g], gens[4 * g + 1], gens[4 * g + 2], gens[4 * g + 3]};
        const float *log_std = params + lstm_sde_group_log_std(L, (size_t)g);
        float *rows = theta + lstm_sde_group_theta(L, m, (size_t)g);
        for (size_t i = 0; i < (size_t)m * latent; ++i)
            rows[i] = sde_theta(words, consumed[g] + (uint64_t)i, log_std[i % latent]);
    }
    return 0;
}

// a group's columns of a state [2][2][G m][H] as a state [2][2][m][H] of its own, and back
static void gather_state(const float *all, const LstmLanes at, int m, int H, float *own)
{
    for (int plane = 0; plane < 4; ++plane)
        for (int e = 0; e < m; ++e)
            for (int k = 0; k < H; ++k)
                own[lstm_state_at(plane / 2, plane % 2, m, H, e, k)] =
                    all[lstm_state_at(plane / 2, plane % 2, at.lanes, H, at.lane0 + e, k)];
}

static void scatter_state(const float *own, const LstmLanes at, int m, int H, float *all)
{
    for (int plane = 0; plane < 4; ++plane)
        for (int e = 0; e < m; ++e)
            for (int k = 0; k < H; ++k)
                all[lstm_state_at(plane / 2, plane % 2, at.lanes, H, at.lane0 + e, k)] =
                    own[lstm_state_at(plane / 2, plane % 2, m, H, e, k)];
}

// rf_lstm_sde_forward_grouped on host arrays, the LSTM critic: every output is there; theta NULL: deterministic
int lspop_forward(const rf_lstm_critic_desc *desc, int G, int m, const float *params, const float *obs, const uint8_t *starts,
                  const float *state_in, float *state_out, const float *theta, float *actions, float *env_actions,
                  float *log_probs, float *values, float *mean, float *sigma)
{
    LstmLayout L;
    if (!lstm_layout_nets(desc->lstm, L, true, desc->critic) || desc->critic != RF_LSTM_CRITIC_LSTM || !population_rows(G, m))
        return -1;
    const int D = L.obs_width, H = L.hidden;
    std::vector<float> before(lstm_state_floats(m, H)), after(lstm_state_floats(m, H));
    for (int g = 0; g < G; ++g) {
        const LstmLanes at = lstm_group_lanes(G, m, g);
        const size_t row = (size_t)g * (size_t)m;
        gather_state(state_in, at, m, H, before.data());
        if (lsc_forward(&desc->lstm, params + (size_t)g * L.total, m, obs + row * (size_t)D, starts + row, nullptr, before.data(),
                        after.data(), theta != nullptr ? theta + lstm_sde_group_theta(L, m, (size_t)g) : nullptr,
                        actions + row, env_actions + row, log_probs + row, values + row, nullptr, mean + row, sigma + row) != 0)
            return -1;
        scatter_state(after.data(), at, m, H, state_out);
    }
    return 0;
}

// rf_lstm_sde_update_grouped on host arrays, the LSTM critic: hypers [G], firsts [G] (clamped; a value outside flags the
// group), stats [G][8]; episode_starts [T + 1][G m] and lstm_states [T + 1][2][2][G m][H] in their single form
int lspop_update(const rf_lstm_critic_desc *desc, int G, int m, int T, const rf_ppo_desc *hypers, float *params, float *state,
                 const float *obs, const float *actions, const float *log_probs, const float *advantages, const float *returns,
                 const uint8_t *starts, const float *states, const int *firsts, int B, float *stats)
{
    LstmLayout L;
    if (!lstm_layout_nets(desc->lstm, L, true, desc->critic) || desc->critic != RF_LSTM_CRITIC_LSTM || m < 1 || T < 1
        || !population_rows(G, (long long)m * (long long)T))
        return -1;
    const int D = L.obs_width, H = L.hidden, N = m * T;
    const size_t own_state = lstm_state_floats(m, H);
    std::vector<uint8_t> own_starts((size_t)(T + 1) * (size_t)m);
    std::vector<float> own_states((size_t)(T + 1) * own_state);
    for (int g = 0; g < G; ++g) {
        const LstmLanes at = lstm_group_lanes(G, m, g);
        for (int t = 0; t <= T; ++t) {
            for (int e = 0; e < m; ++e)
                own_starts[(size_t)t * (size_t)m + (size_t)e] = starts[(size_t)t * (size_t)at.lanes + (size_t)(at.lane0 + e)];
            gather_state(states + (size_t)t * lstm_state_floats(at.lanes, H), at, m, H, own_states.data() + (size_t)t * own_state);
        }
        const size_t row = (size_t)g * (size_t)N;
        const int first = lstm_ppo_first(firsts[g], N);
        float *group_stats = stats + 8 * (size_t)g;
        float *group_params = params + (size_t)g * L.total;
        float *group_state = state + (size_t)g * ((size_t)kPpoStateHeader + 2 * (size_t)L.total);
        std::vector<float> kept_params(group_params, group_params + L.total);
        std::vector<float> kept_state(group_state, group_state + kPpoStateHeader + 2 * (size_t)L.total);
        if (lsc_update(&desc->lstm, hypers + g, group_params, group_state, T, m, obs + row * (size_t)D,
                       actions + lstm_sde_group_actions((size_t)g, N), log_probs + row, advantages + row, returns + row,
                       own_starts.data(), own_states.data(), first, B, group_stats, nullptr) != 0)
            return -1;
        if (first != firsts[g]) { // (L4: the group is skipped and flagged, whatever its rows held)
            memcpy(group_params, kept_params.data(), kept_params.size() * sizeof(float));
            memcpy(group_state, kept_state.data(), kept_state.size() * sizeof(float));
            group_stats[7] = (float)RF_PPO_INVALID;
        }
    }
    return 0;
}

} // extern "C"

#if defined(LSTMSDEPOPCHECK_MAIN)
// One grouped noise reset, forward and update of G = 2 groups of m = 2 environments over T = 2 steps on a 2-input, 3-unit
// LSTM with 3 / 2 tanh MLPs, every group with its own parameters, log_std, generator and hyper-parameters: the grouped
// addressing under a plain host toolchain (and whatever instrumentation it is compiled with), printed for a person to read.
int main()
{
    const rf_lstm_critic_desc desc{{{2, 1, RF_POLICY_TANH, 1, {3, 0}, 1, {2, 0}}, 3}, RF_LSTM_CRITIC_LSTM};
    const int G = 2, m = 2, T = 2, D = 2, H = 3, n = G * m, N = m * T;
    unsigned long long theta_at = 0, actions_at = 0, log_std_at = 0;
    unsigned P = 0, latent = 0;
    if (lspop_offsets(&desc, m, T, 1, &theta_at, &actions_at, &log_std_at, &P, &latent) != 0)
        return 1;
    if (theta_at != (unsigned long long)m * latent || actions_at != (unsigned long long)N || log_std_at != 2ull * P - latent)
        return 1;
    if (lspop_state_size(&desc, G, m) != (unsigned long long)G * (32 + 8 * P) || lspop_workspace_size(&desc, G, m, T, 3) == 0)
        return 1;
    std::vector<float> params((size_t)G * P), state((size_t)G * (kPpoStateHeader + 2 * P), 0.0f), theta((size_t)n * latent, 0.0f);
    for (int g = 0; g < G; ++g) {
        for (unsigned p = 0; p < P; ++p)
            params[(size_t)g * P + p] = 0.25f * (float)((int)((p + 3 * g) % 7) - 3);
        for (unsigned k = 0; k < latent; ++k)
            params[(size_t)g * P + P - latent + k] = g == 0 ? -1.0f : 0.5f;
    }
    const unsigned long long gens[G * 4] = {0x9e3779b97f4a7c15ull, 0x2545f4914f6cdd1dull, 0xda3e39cb94b95bdbull, 1ull,
                                            0x0123456789abcdefull, 0xfedcba9876543211ull, 0x0f1e2d3c4b5a6978ull, 3ull};
    const unsigned long long consumed[G] = {0, (1ull << 32) + 5};
    if (lspop_noise(&desc, G, m, params.data(), gens, consumed, nullptr, theta.data()) != 0)
        return 1;
    // the rollout's slabs: observations [G N][D], group g's rows in flat()'s order e * T + t; lstm_states [T + 1][2][2][n][H]
    float flat_obs[G * N * D];
    for (int i = 0; i < G * N * D; ++i)
        flat_obs[i] = 0.125f * (float)((i * 5) % 17 - 8);
    std::vector<float> states((size_t)(T + 1) * 4 * n * H, 0.0f);
    const uint8_t starts[(T + 1) * n] = {1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0};
    float actions[G * N], log_probs[G * N], env_actions[n], values[n], mean[n], sigma[n];
    for (int t = 0; t < T; ++t) {
        float obs[n * D], step_actions[n], step_log_probs[n];
        for (int lane = 0; lane < n; ++lane)
            for (int k = 0; k < D; ++k)
                obs[lane * D + k] = flat_obs[((lane / m) * N + (lane % m) * T + t) * D + k];
        if (lspop_forward(&desc, G, m, params.data(), obs, starts + t * n, states.data() + (size_t)t * 4 * n * H,
                          states.data() + (size_t)(t + 1) * 4 * n * H, theta.data(), step_actions, env_actions, step_log_probs,
                          values, mean, sigma) != 0)
            return 1;
        for (int lane = 0; lane < n; ++lane) {
            const int row = (lane / m) * N + (lane % m) * T + t;
            actions[row] = step_actions[lane], log_probs[row] = step_log_probs[lane];
            if (t == 0)
                printf("group %d env %d: action %.9g (to the environment %.9g) log_prob %.9g value %.9g mean %.9g sigma %.9g\n",
                       lane / m, lane % m, step_actions[lane], env_actions[lane], step_log_probs[lane], values[lane],
                       mean[lane], sigma[lane]);
        }
    }
    const rf_ppo_desc hypers[G] = {{3e-4, 0.2, 0.01, 0.5, 0.5, 0.9, 0.999, 1e-5, 1, 0}, {1e-2, 0.1, 0.0, 0.25, 5.0, 0.8, 0.99, 1e-3, 0, 0}};
    float advantages[G * N], returns[G * N], stats[G * 8];
    for (int i = 0; i < G * N; ++i)
        advantages[i] = 0.25f * (float)((i * 3) % 7 - 3), returns[i] = 0.1f * (float)((i * 5) % 9 - 4);
    const int firsts[G] = {1, 3};
    if (lspop_update(&desc, G, m, T, hypers, params.data(), state.data(), flat_obs, actions, log_probs, advantages, returns,
                     starts, states.data(), firsts, 3, stats) != 0)
        return 1;
    int bad = 0;
    for (int g = 0; g < G; ++g) {
        printf("group %d stats:", g);
        for (int i = 0; i < 8; ++i) {
            printf(" %.9g", stats[8 * g + i]);
            bad |= !(stats[8 * g + i] == stats[8 * g + i]) || stats[8 * g + i] - stats[8 * g + i] != 0.0f;
        }
        printf("\n");
        bad |= stats[8 * g + 7] != 0.0f;
    }
    return bad;
}
#endif
