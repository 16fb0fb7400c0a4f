// lstmsdecheck.cpp -- TEST INFRASTRUCTURE.  Compiles the recurrent sde policy's arithmetic (include/reinfocus_hip.h, "lstm
// sde policy" and "lstm sde update": lstm_sde_layout and the cell of reinfocus_amd/csrc/rf_lstm.h, the Gaussian head of
// rf_policy_math.h / rf_sde.h / rf_ppo.h, the sequence rule, BPTT, workspace layout and parameter-to-source map of
// rf_lstm_ppo.h) for the host, with plain loops in place of the kernels, so that a CPU-only test can compare the
// definition with the numpy twins (environments/lstm_sde.py lstm_sde_numpy, environments/lstm_learner.py
// lstm_update_numpy) before any GPU sees it.  With -DLSTMSDECHECK_MAIN the same source is a stand-alone program.  Never
// loaded by the product package.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../reinfocus_amd/csrc/rf_lstm_ppo.h"
#include "../../reinfocus_amd/csrc/rf_sde.h"

using namespace rf;

extern "C" {

unsigned long long lsc_params_size(const rf_lstm_policy_desc *desc)
{
    LstmLayout L;
    return lstm_sde_layout(*desc, L) ? L.total : 0;
}

// offset in floats of log_std inside the packed parameters, and its length L; 0 if refused
unsigned long long lsc_log_std(const rf_lstm_policy_desc *desc, int *latent)
{
    LstmLayout L;
    if (!lstm_sde_layout(*desc, L))
        return 0;
    *latent = (int)L.mlp.sde;
    return L.mlp.log_std;
}

unsigned long long lsc_state_size(const rf_lstm_policy_desc *desc)
{
    LstmLayout L;
    return lstm_sde_layout(*desc, L) ? 4ull * kPpoStateHeader + 8ull * L.total : 0;
}

unsigned long long lsc_workspace_size(const rf_lstm_policy_desc *desc, int max_batch)
{
    LstmLayout L;
    LstmPpoWork W;
    return lstm_sde_layout(*desc, L) && lstm_ppo_work(L, max_batch, W) ? 4ull * W.total : 0;
}

// offset in floats of the packed gradient inside a workspace laid out for minibatches of max_batch; 0 if refused
unsigned long long lsc_grad_offset(const rf_lstm_policy_desc *desc, int max_batch)
{
    LstmLayout L;
    LstmPpoWork W;
    return lstm_sde_layout(*desc, L) && lstm_ppo_work(L, max_batch, W) ? W.mlp.grad : 0;
}

// rf_lstm_sde_noise_reset on host arrays
int lsc_noise(const rf_lstm_policy_desc *desc, const float *params, int n, const unsigned long long gen[4], float *theta)
{
    LstmLayout L;
    if (!lstm_sde_layout(*desc, L) || n < 1)
        return -1;
    const uint64_t words[4] = {gen[0], gen[1], gen[2], gen[3]};
    const size_t latent = L.mlp.sde;
    for (size_t i = 0; i < (size_t)n * latent; ++i)
        theta[i] = sde_theta(words, (uint64_t)i, params[L.mlp.log_std + i % latent]);
    return 0;
}

// one net's cell of environment e: h1 / c1 [H] from x [D] and the state (zero where `reset`)
static void cell_of(const LstmLayout &L, const float *params, int net, int n, int e, const float *x, const float *state,
                    bool reset, float *h1, float *c1)
{
    const int D = L.obs_width, H = L.hidden;
    float h[kPolicyMaxWidth];
    for (int k = 0; k < H; ++k)
        h[k] = reset ? 0.0f : state[lstm_state_at(net, 0, n, H, e, k)];
    for (int j = 0; j < H; ++j) {
        float a[4];
        for (int q = 0; q < 4; ++q) {
            const int col = q * H + j;
            float s = params[L.b_ih[net] + (unsigned)col];
            s = s + params[L.b_hh[net] + (unsigned)col];
            s = policy_dot(x, 1, params + L.w_ih[net] + col, 4 * H, s, D);
            s = policy_dot(h, 1, params + L.w_hh[net] + col, 4 * H, s, H);
            a[q] = s;
        }
        const float c = reset ? 0.0f : state[lstm_state_at(net, 1, n, H, e, j)];
        lstm_cell(a[0], a[1], a[2], a[3], c, &h1[j], &c1[j]);
    }
}

// the MLP of a net on h1: its last activations into `last` [K], returns K; *head receives the head's one output
static int mlp_of(const LstmLayout &L, const float *params, int net, const float *h1, float *last, float *head)
{
    float a[kPolicyMaxWidth], b[kPolicyMaxWidth];
    const PolicyLayout &M = L.mlp;
    float *x = a, *y = b;
    int K = L.hidden;
    for (int k = 0; k < K; ++k)
        x[k] = h1[k];
    for (int layer = 0; layer < M.layers[net]; ++layer) {
        const int W = M.width[net][layer];
        for (int j = 0; j < W; ++j)
            y[j] = policy_activation(policy_dot(x, 1, params + M.weight[net][layer] + j, W, params[M.bias[net][layer] + j], K),
                                     M.activation);
        float *t = x;
        x = y, y = t, K = W;
    }
    const int at = M.layers[net];
    *head = policy_dot(x, 1, params + M.weight[net][at], 1, params[M.bias[net][at]], K);
    for (int k = 0; k < K; ++k)
        last[k] = x[k];
    return K;
}

// rf_lstm_sde_forward on host arrays: 0, or -1 for a desc outside the limits.  theta NULL: deterministic.  state_out and
// every output may be NULL; state_out may be state_in.
int lsc_forward(const rf_lstm_policy_desc *desc, const float *params, int n, const float *obs, const uint8_t *starts,
                const float *final_obs, const float *state_in, float *state_out, const float *theta, float *actions,
                float *env_actions, float *log_probs, float *values, float *final_values, float *mean, float *sigma)
{
    LstmLayout L;
    if (!lstm_sde_layout(*desc, L))
        return -1;
    const int D = L.obs_width, H = L.hidden;
    float h1[kPolicyMaxWidth], c1[kPolicyMaxWidth], last[kPolicyMaxWidth], std2[kPolicyMaxWidth], y;
    for (unsigned k = 0; k < L.mlp.sde; ++k)
        std2[k] = sde_std2(params[L.mlp.log_std + k]);
    const bool pi_out = actions || env_actions || log_probs || mean || sigma;
    for (int e = 0; e < n; ++e) {
        if (final_obs != nullptr && final_values != nullptr) { // first: it reads state_in, which may be state_out
            const float *in = final_obs + (size_t)e * (size_t)D;
            cell_of(L, params, 1, n, e, in, state_in, false, h1, c1);
            mlp_of(L, params, 1, h1, last, &y);
            final_values[e] = in[0] != in[0] ? bits_f32(kPolicyNaN) : policy_canonical(y);
        }
        const float *x = obs + (size_t)e * (size_t)D;
        const bool reset = starts[e] != 0;
        for (int net = 0; net < 2; ++net) {
            const bool heads = net == 0 ? pi_out : values != nullptr;
            if (!heads && state_out == nullptr)
                continue;
            cell_of(L, params, net, n, e, x, state_in, reset, h1, c1);
            if (state_out != nullptr)
                for (int j = 0; j < H; ++j) {
                    state_out[lstm_state_at(net, 0, n, H, e, j)] = policy_canonical(h1[j]);
                    state_out[lstm_state_at(net, 1, n, H, e, j)] = policy_canonical(c1[j]);
                }
            if (!heads)
                continue;
            const int K = mlp_of(L, params, net, h1, last, &y);
            if (net == 1) {
                values[e] = policy_canonical(y);
                continue;
            }
            const float mu = y;
            const float s = sde_sigma(last, 1, std2, K);
            float a = mu;
            if (theta != nullptr)
                a = mu + policy_dot(last, 1, theta + (size_t)e * (size_t)K, 1, 0.0f, K);
            if (actions != nullptr)
                actions[e] = policy_canonical(a);
            if (env_actions != nullptr)
                env_actions[e] = sde_env_action(a);
            if (log_probs != nullptr)
                log_probs[e] = sde_log_prob(a, mu, s);
            if (mean != nullptr)
                mean[e] = policy_canonical(mu);
            if (sigma != nullptr)
                sigma[e] = policy_canonical(s);
        }
    }
    return 0;
}

// rf_lstm_sde_update on host arrays: 0, or -1 for what the entry point refuses by value.  grad_out (or NULL) receives
// the packed gradient before clipping.
int lsc_update(const rf_lstm_policy_desc *desc, const rf_ppo_desc *ppo, float *params, float *state, int T, int n,
               const float *obs, const float *actions, const float *old_log_probs, const float *advantages,
               const float *returns, const uint8_t *starts, const float *states, int first, int B, float *stats,
               float *grad_out)
{
    LstmLayout L;
    PpoHyper hy;
    LstmPpoWork W;
    if (!lstm_sde_layout(*desc, L) || !ppo_hyper(*ppo, hy) || T < 1 || n < 1 || (long long)T * n > (1ll << 30))
        return -1;
    const int N = T * n;
    if (B < 1 || B > N || first < 0 || first >= N || !lstm_ppo_work(L, B, W))
        return -1;
    const PolicyLayout &M = L.mlp;
    const int D = L.obs_width, H = L.hidden;
    std::vector<float> workspace(W.total, 0.0f);
    float *ws = workspace.data();
    // ---- lstm_ppo_forward_kernel ----
    for (int b0 = 0; b0 < B; ++b0) {
        if (!lstm_ppo_is_start(starts, T, n, first, b0))
            continue;
        const int end = lstm_ppo_end(starts, T, n, first, b0, B);
        for (int net = 0; net < 2; ++net) {
            float h[kPolicyMaxWidth], c[kPolicyMaxWidth], h1[kPolicyMaxWidth];
            {
                const int r = lstm_ppo_row(first, b0, N);
                const int e = r / T, t = r - e * T;
                const bool kept = starts[(size_t)t * (size_t)n + (size_t)e] == 0;
                for (int j = 0; j < H; ++j) {
                    h[j] = kept ? states[lstm_ppo_state_at(t, net, 0, n, H, e, j)] : 0.0f;
                    c[j] = kept ? states[lstm_ppo_state_at(t, net, 1, n, H, e, j)] : 0.0f;
                }
            }
            for (int b = b0; b < end; ++b) {
                const int r = lstm_ppo_row(first, b, N);
                const float *x = obs + (size_t)r * (size_t)D;
                for (int k = 0; k < D; ++k)
                    ws[W.x + (size_t)b * (size_t)D + (size_t)k] = x[k];
                for (int j = 0; j < H; ++j) {
                    const size_t at = (size_t)b * (size_t)H + (size_t)j;
                    ws[W.h_prev[net] + at] = h[j];
                    ws[W.c_prev[net] + at] = c[j];
                    float a[4], gate[4], c1;
                    for (int q = 0; q < 4; ++q) {
                        const int col = q * H + j;
                        float s = params[L.b_ih[net] + (unsigned)col] + params[L.b_hh[net] + (unsigned)col];
                        s = policy_dot(x, 1, params + L.w_ih[net] + col, 4 * H, s, D);
                        a[q] = policy_dot(h, 1, params + L.w_hh[net] + col, 4 * H, s, H);
                    }
                    lstm_cell_gates(a, c[j], gate, &h1[j], &c1);
                    for (int q = 0; q < 4; ++q)
                        ws[W.gates[net] + (size_t)b * (size_t)(4 * H) + (size_t)(q * H + j)] = gate[q];
                    ws[W.c1[net] + at] = c1;
                    ws[W.h1[net] + at] = h1[j];
                    c[j] = c1;
                }
                for (int j = 0; j < H; ++j)
                    h[j] = h1[j];
            }
        }
    }
    // ---- lstm_ppo_mlp_kernel<true> ----
    bool invalid = false;
    std::vector<double> tree((size_t)ppo_pow2(B > kPpoMaxPartials ? B : kPpoMaxPartials), 0.0);
    std::vector<int> row((size_t)B);
    for (int b = 0; b < B; ++b) {
        row[b] = lstm_ppo_row(first, b, N);
        const float action = actions[row[b]];
        invalid = invalid || action != action;
    }
    const bool normalise = hy.normalize != 0 && B > 1;
    double mean = 0.0, var = 0.0;
    if (normalise) {
        const int size = ppo_pow2(B);
        for (int b = 0; b < size; ++b)
            tree[b] = b < B ? (double)advantages[row[b]] : 0.0;
        mean = ppo_treesum_host(tree.data(), size) / (double)B;
        for (int b = 0; b < size; ++b) {
            const double t = b < B ? (double)advantages[row[b]] - mean : 0.0;
            tree[b] = b < B ? t * t : 0.0;
        }
        var = ppo_treesum_host(tree.data(), size) / (double)(B - 1);
    }
    const float Bf = (float)B;
    float std2[kPolicyMaxWidth];
    for (unsigned k = 0; k < M.sde; ++k)
        std2[k] = sde_std2(params[M.log_std + k]);
    for (int b = 0; b < B; ++b)
        for (int net = 0; net < 2; ++net) {
            const int layers = M.layers[net];
            const float *in = ws + W.h1[net] + (size_t)b * (size_t)H;
            int K = H;
            for (int layer = 0; layer < layers; ++layer) {
                const int Wd = M.width[net][layer];
                float *h = ws + W.mlp.h[net][layer] + (size_t)b * (size_t)Wd;
                for (int j = 0; j < Wd; ++j)
                    h[j] = policy_activation(policy_dot(in, 1, params + M.weight[net][layer] + j, Wd,
                                                        params[M.bias[net][layer] + j], K), M.activation);
                in = h, K = Wd;
            }
            const float y = policy_dot(in, 1, params + M.weight[net][layers], 1, params[M.bias[net][layers]], K);
            float *dhead = ws + W.mlp.d[net][layers] + (size_t)b;
            float *loss = ws + W.mlp.loss + b;
            if (net == 0) {
                const float A = normalise ? ppo_normalised(advantages[row[b]], mean, var) : advantages[row[b]];
                const float sigma = sde_sigma(in, 1, std2, K);
                sde_pi_sample(y, sigma, actions[row[b]], old_log_probs[row[b]], A, hy.clip, hy.ent, Bf, dhead,
                              ws + W.mlp.sde + b, &loss[0], &loss[2 * W.mlp.max_batch], &loss[3 * W.mlp.max_batch],
                              &loss[4 * W.mlp.max_batch]);
            } else {
                ppo_vf_sample(y, returns[row[b]], hy.vf * 2.0f, Bf, &loss[W.mlp.max_batch], dhead);
            }
            const float *dout = dhead;
            int outs = 1;
            for (int layer = layers - 1; layer >= 0; --layer) {
                const int Wd = M.width[net][layer];
                const float *h = ws + W.mlp.h[net][layer] + (size_t)b * (size_t)Wd;
                float *din = ws + W.mlp.d[net][layer] + (size_t)b * (size_t)Wd;
                for (int k = 0; k < Wd; ++k)
                    din[k] = ppo_back(params + M.weight[net][layer + 1] + (size_t)k * (size_t)outs, dout, 1, outs, h[k],
                                      M.activation);
                dout = din, outs = Wd;
            }
            float *dh = ws + W.dh[net] + (size_t)b * (size_t)H;
            for (int k = 0; k < H; ++k) { // the product into h': no activation derivative
                const float *w = params + M.weight[net][0] + (size_t)k * (size_t)outs;
                float acc = 0.0f;
                for (int o = 0; o < outs; ++o)
                    acc = acc + w[o] * dout[o];
                dh[k] = acc;
            }
        }
    // ---- lstm_ppo_bptt_kernel ----
    for (int b0 = 0; b0 < B; ++b0) {
        if (!lstm_ppo_is_start(starts, T, n, first, b0))
            continue;
        const int end = lstm_ppo_end(starts, T, n, first, b0, B);
        for (int net = 0; net < 2; ++net) {
            float dh_rec[kPolicyMaxWidth], dc_next[kPolicyMaxWidth];
            for (int j = 0; j < H; ++j)
                dh_rec[j] = dc_next[j] = 0.0f;
            for (int b = end - 1; b >= b0; --b) {
                float *da_row = ws + W.da[net] + (size_t)b * (size_t)(4 * H);
                for (int j = 0; j < H; ++j) {
                    const size_t at = (size_t)b * (size_t)H + (size_t)j;
                    const float *g = ws + W.gates[net] + (size_t)b * (size_t)(4 * H) + (size_t)j;
                    const float gate[4] = {g[0], g[H], g[2 * H], g[3 * H]};
                    float da[4];
                    dc_next[j] = lstm_bptt_unit(ws[W.dh[net] + at], dh_rec[j], gate, ws[W.c_prev[net] + at],
                                                ws[W.c1[net] + at], dc_next[j], da);
                    for (int q = 0; q < 4; ++q)
                        da_row[q * H + j] = da[q];
                }
                if (b == b0)
                    break;
                for (int k = 0; k < H; ++k)
                    dh_rec[k] = lstm_bptt_rec(params + L.w_hh[net] + (size_t)k * (size_t)(4 * H), da_row, H);
            }
        }
    }
    // ---- lstm_ppo_gradient_kernel<true> ----
    std::vector<double> partial((size_t)W.mlp.partials, 0.0);
    for (unsigned block = 0; block < W.mlp.partials; ++block) {
        double leaves[kPpoLeaves];
        for (unsigned t = 0; t < (unsigned)kPpoLeaves; ++t) {
            const unsigned p = block * kPpoLeaves + t;
            leaves[t] = 0.0;
            if (p < L.total) {
                const float g = policy_canonical(lstm_ppo_parameter_gradient(L, W, ws, params, p, B));
                ws[W.mlp.grad + p] = g;
                leaves[t] = (double)g * (double)g;
            }
        }
        for (int s = 1; s < kPpoLeaves; s <<= 1)
            for (int i = 0; i < kPpoLeaves; i += 2 * s)
                leaves[i] = leaves[i] + leaves[i + s];
        partial[block] = leaves[0];
    }
    if (grad_out != nullptr)
        for (unsigned p = 0; p < L.total; ++p)
            grad_out[p] = ws[W.mlp.grad + p];
    // ---- lstm_ppo_norm_kernel ----
    for (unsigned group = 0; group < W.supers; ++group) {
        double leaves[kLstmPpoGroup];
        for (unsigned t = 0; t < (unsigned)kLstmPpoGroup; ++t) {
            const unsigned i = group * kLstmPpoGroup + t;
            leaves[t] = i < W.mlp.partials ? partial[i] : 0.0;
        }
        for (int s = 1; s < kLstmPpoGroup; s <<= 1)
            for (int i = 0; i < kLstmPpoGroup; i += 2 * s)
                leaves[i] = leaves[i] + leaves[i + s];
        tree[group] = leaves[0];
    }
    // ---- ppo_adam_kernel ----
    const int size = ppo_pow2((int)W.supers);
    for (int i = (int)W.supers; i < size; ++i)
        tree[i] = 0.0;
    const double norm = sqrt(ppo_treesum_host(tree.data(), size));
    const int flags = invalid ? RF_PPO_INVALID : (ppo_finite(norm) ? 0 : RF_PPO_NONFINITE);
    PpoHeader now;
    memcpy(&now, state, sizeof now);
    const PpoStep step = ppo_step(hy, now, norm);
    double sums[5];
    for (int term = 0; term < 5; ++term) {
        const int batch = ppo_pow2(B);
        for (int b = 0; b < batch; ++b)
            tree[b] = b < B ? (double)ws[W.mlp.loss + (size_t)term * W.mlp.max_batch + b] : 0.0;
        sums[term] = ppo_treesum_host(tree.data(), batch);
    }
    ppo_stats(sums, B, norm, hy, flags, stats);
    if (flags != 0)
        return 0;
    float *m = state + kPpoStateHeader, *v = m + L.total;
    for (unsigned p = 0; p < L.total; ++p)
        ppo_adam(step, ws[W.mlp.grad + p], params + p, m + p, v + p);
    memcpy(state, &step.next, sizeof step.next);
    return 0;
}

} // extern "C"

#if defined(LSTMSDECHECK_MAIN)
// One noise reset, one forward and one update of a 2-input, 3-unit LSTM with 3 / 2 tanh MLPs over two environments and
// two steps: the arithmetic under a plain host toolchain (and whatever instrumentation it is compiled with), printed for
// a person to read.
int main()
{
    const rf_lstm_policy_desc desc{{2, 1, RF_POLICY_TANH, 1, {3, 0}, 1, {2, 0}}, 3};
    const int n = 2, T = 2, D = 2, H = 3;
    const unsigned P = (unsigned)lsc_params_size(&desc);
    int latent = 0;
    if (P == 0 || lsc_log_std(&desc, &latent) + (unsigned)latent != P)
        return 1;
    std::vector<float> params(P), state(kPpoStateHeader + 2 * P, 0.0f), theta((size_t)n * latent);
    for (unsigned p = 0; p < P; ++p)
        params[p] = 0.25f * (float)((int)(p % 7) - 3);
    const unsigned long long gen[4] = {0x9e3779b97f4a7c15ull, 0x2545f4914f6cdd1dull, 0xda3e39cb94b95bdbull, 1ull};
    if (lsc_noise(&desc, params.data(), n, gen, theta.data()) != 0)
        return 1;
    // the rollout's slabs: observations [N][D] in flat()'s order e * T + t, lstm_states [T + 1][2][2][n][H]
    const float flat_obs[T * n * D] = {0.5f, -1.0f, 2.0f, 0.25f, -0.75f, 0.125f, 1.5f, -0.5f};
    std::vector<float> states((size_t)(T + 1) * 4 * n * H, 0.0f);
    const uint8_t starts[(T + 1) * n] = {1, 1, 0, 1, 0, 0};
    float actions[T * n], log_probs[T * n], env_actions[n], values[n], mean[n], sigma[n];
    for (int t = 0; t < T; ++t) {
        float obs[n * D];
        for (int e = 0; e < n; ++e)
            for (int k = 0; k < D; ++k)
                obs[e * D + k] = flat_obs[(e * T + t) * D + k];
        float step_actions[n], step_log_probs[n];
        if (lsc_forward(&desc, params.data(), n, obs, starts + t * n, nullptr, states.data() + (size_t)t * 4 * n * H,
                        states.data() + (size_t)(t + 1) * 4 * n * H, theta.data(), step_actions, env_actions, step_log_probs,
                        values, nullptr, mean, sigma) != 0)
            return 1;
        for (int e = 0; e < n; ++e) {
            actions[e * T + t] = step_actions[e], log_probs[e * T + t] = step_log_probs[e];
            if (t == 0)
                printf("env %d: action %.9g (to the environment %.9g) log_prob %.9g value %.9g mean %.9g sigma %.9g\n", e,
                       step_actions[e], env_actions[e], step_log_probs[e], values[e], mean[e], sigma[e]);
        }
    }
    const rf_ppo_desc ppo{3e-4, 0.2, 0.01, 0.5, 0.5, 0.9, 0.999, 1e-5, 1, 0};
    const float advantages[T * n] = {1.0f, -0.5f, 0.25f, 0.75f}, returns[T * n] = {0.3f, -0.2f, 0.1f, 0.4f};
    float stats[8];
    if (lsc_update(&desc, &ppo, params.data(), state.data(), T, n, flat_obs, actions, log_probs, advantages, returns, starts,
                   states.data(), 1, 3, stats, nullptr) != 0)
        return 1;
    printf("stats:");
    for (int i = 0; i < 8; ++i)
        printf(" %.9g", stats[i]);
    printf("\n");
    return stats[7] == 0.0f ? 0 : 1;
}
#endif
