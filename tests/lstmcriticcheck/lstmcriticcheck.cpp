// lstmcriticcheck.cpp -- TEST INFRASTRUCTURE.  Compiles the arithmetic of the recurrent policy with a feed-forward critic
// (include/reinfocus_hip.h, "lstm critic": lstm_layout_nets with RF_LSTM_CRITIC_LINEAR and the cell of
// reinfocus_amd/csrc/rf_lstm.h, both heads of rf_policy_math.h / rf_sde.h / rf_ppo.h, the sequence rule, BPTT, workspace
// layout and parameter-to-source map of rf_lstm_ppo.h) for the host, with plain loops in place of the kernels, so that a
// CPU-only test can compare the definition with the numpy twins (environments/lstm.py, lstm_sde.py, lstm_learner.py with
// enable_critic_lstm=False) before any GPU sees it.  `sde` selects the Gaussian head (float32 actions, theta in place of
// gen).  With -DLSTMCRITICCHECK_MAIN the same source is a stand-alone program.  Never loaded by the product package.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../reinfocus_amd/csrc/rf_lstm_ppo.h"
#include "../../reinfocus_amd/csrc/rf_sde.h"

using namespace rf;

static bool layout_of(const rf_lstm_critic_desc *desc, int sde, LstmLayout &L)
{
    return lstm_layout_nets(desc->lstm, L, sde != 0, desc->critic);
}

extern "C" {

// floats of the packed parameters; 0 if refused (either critic mode: the layout alone)
unsigned long long lcc_params_size(const rf_lstm_critic_desc *desc, int sde)
{
    LstmLayout L;
    return layout_of(desc, sde, L) ? L.total : 0;
}

// offsets in floats of critic.weight^T and critic.bias inside the packed parameters; 0 if refused or not the linear mode
unsigned long long lcc_critic_at(const rf_lstm_critic_desc *desc, int sde, unsigned long long *bias)
{
    LstmLayout L;
    if (!layout_of(desc, sde, L) || L.critic != kLstmCriticLinear)
        return 0;
    *bias = L.b_ih[1];
    return L.w_ih[1];
}

unsigned long long lcc_state_size(const rf_lstm_critic_desc *desc, int sde)
{
    LstmLayout L;
    return layout_of(desc, sde, L) ? 4ull * kPpoStateHeader + 8ull * L.total : 0;
}

// bytes of the update's workspace (either critic mode); 0 if refused
unsigned long long lcc_workspace_size(const rf_lstm_critic_desc *desc, int sde, int max_batch)
{
    LstmLayout L;
    LstmPpoWork W;
    return layout_of(desc, sde, L) && lstm_ppo_work(L, max_batch, W) ? 4ull * W.total : 0;
}

// offset in floats of the packed gradient inside a workspace laid out for minibatches of max_batch; 0 if refused
unsigned long long lcc_grad_offset(const rf_lstm_critic_desc *desc, int sde, int max_batch)
{
    LstmLayout L;
    LstmPpoWork W;
    return layout_of(desc, sde, L) && lstm_ppo_work(L, max_batch, W) ? W.mlp.grad : 0;
}

// the pi net's cell of environment e: h1 / c1 [H] from x [D] and the state (zero where `reset`)
static void cell_of(const LstmLayout &L, const float *params, int n, int e, const float *x, const float *state, bool reset,
                    float *h1, float *c1)
{
    const int D = L.obs_width, H = L.hidden;
    float h[kPolicyMaxWidth];
    for (int k = 0; k < H; ++k)
        h[k] = reset ? 0.0f : state[lstm_state_at(0, 0, n, H, e, k)];
    for (int j = 0; j < H; ++j) {
        float a[4];
        for (int q = 0; q < 4; ++q) {
            const int col = q * H + j;
            float s = params[L.b_ih[0] + (unsigned)col];
            s = s + params[L.b_hh[0] + (unsigned)col];
            s = policy_dot(x, 1, params + L.w_ih[0] + col, 4 * H, s, D);
            s = policy_dot(h, 1, params + L.w_hh[0] + col, 4 * H, s, H);
            a[q] = s;
        }
        const float c = reset ? 0.0f : state[lstm_state_at(0, 1, n, H, e, j)];
        lstm_cell(a[0], a[1], a[2], a[3], c, &h1[j], &c1[j]);
    }
}

// C2: the vf net's linear layer on x [D]: out [H], no activation
static void critic_of(const LstmLayout &L, const float *params, const float *x, float *out)
{
    for (int j = 0; j < L.hidden; ++j)
        out[j] = policy_dot(x, 1, params + L.w_ih[1] + j, L.hidden, params[L.b_ih[1] + (unsigned)j], L.obs_width);
}

// the MLP and head of a net on its input `in` [H]: l[0 .. O-1]; `last` [K] receives the last activations, returns K
static int mlp_of(const LstmLayout &L, const float *params, int net, const float *in, float *last, float *l)
{
    float a[kPolicyMaxWidth], b[kPolicyMaxWidth];
    const PolicyLayout &M = L.mlp;
    float *x = a, *y = b;
    int K = L.hidden;
    for (int k = 0; k < K; ++k)
        x[k] = in[k];
    for (int layer = 0; layer < M.layers[net]; ++layer) {
        const int W = M.width[net][layer];
        for (int j = 0; j < W; ++j)
            y[j] = policy_activation(policy_dot(x, 1, params + M.weight[net][layer] + j, W, params[M.bias[net][layer] + j], K),
                                     M.activation);
        float *t = x;
        x = y, y = t, K = W;
    }
    const int head = M.layers[net], O = net == 0 ? M.n_actions : 1;
    for (int o = 0; o < O; ++o)
        l[o] = policy_dot(x, 1, params + M.weight[net][head] + o, O, params[M.bias[net][head] + o], K);
    for (int k = 0; k < K; ++k)
        last[k] = x[k];
    return K;
}

// rf_lstm_critic_forward (sde: rf_lstm_critic_sde_forward) on host arrays: 0, or -1 for a desc outside the limits or not in
// the linear mode.  Categorical: gen and flags, actions int64, logits [n][A].  Gaussian: theta (NULL: deterministic),
// actions float32 (raw), env_actions, logits receives the mean, sigma.  state_out and every output may be NULL; state_out
// may be state_in.  `starts` and `state_in` reach the pi net only.
int lcc_forward(const rf_lstm_critic_desc *desc, int sde, const float *params, int n, const float *obs, const uint8_t *starts,
                const float *final_obs, const float *state_in, float *state_out, const unsigned long long gen[4], int flags,
                const float *theta, void *actions_any, float *env_actions, float *log_probs, float *values,
                float *final_values, float *logits, float *sigma)
{
    LstmLayout L;
    if (!layout_of(desc, sde, L) || L.critic != kLstmCriticLinear)
        return -1;
    const int D = L.obs_width, H = L.hidden;
    const bool sampled = (flags & RF_POLICY_DETERMINISTIC) == 0;
    const uint64_t words[4] = {gen ? gen[0] : 0, gen ? gen[1] : 0, gen ? gen[2] : 0, gen ? gen[3] : 0};
    int64_t *actions = sde ? nullptr : static_cast<int64_t *>(actions_any);
    float *raw_actions = sde ? static_cast<float *>(actions_any) : nullptr;
    float h1[kPolicyMaxWidth], c1[kPolicyMaxWidth], last[kPolicyMaxWidth], std2[kPolicyMaxWidth];
    float l[kPolicyMaxActions], c[kPolicyMaxActions];
    for (unsigned k = 0; k < L.mlp.sde; ++k)
        std2[k] = sde_std2(params[L.mlp.log_std + k]);
    const bool pi_out = sde ? actions_any || env_actions || log_probs || logits || sigma : actions_any || logits;
    for (int e = 0; e < n; ++e) {
        if (final_obs != nullptr && final_values != nullptr) {
            const float *in = final_obs + (size_t)e * (size_t)D;
            critic_of(L, params, in, h1);
            mlp_of(L, params, 1, h1, last, l);
            final_values[e] = in[0] != in[0] ? bits_f32(kPolicyNaN) : policy_canonical(l[0]);
        }
        const float *x = obs + (size_t)e * (size_t)D;
        if (values != nullptr) {
            critic_of(L, params, x, h1);
            mlp_of(L, params, 1, h1, last, l);
            values[e] = policy_canonical(l[0]);
        }
        if (!pi_out && state_out == nullptr)
            continue;
        cell_of(L, params, n, e, x, state_in, starts[e] != 0, h1, c1);
        if (state_out != nullptr)
            for (int net = 0; net < 2; ++net) // C3: both halves are the pi net's
                for (int j = 0; j < H; ++j) {
                    state_out[lstm_state_at(net, 0, n, H, e, j)] = policy_canonical(h1[j]);
                    state_out[lstm_state_at(net, 1, n, H, e, j)] = policy_canonical(c1[j]);
                }
        if (!pi_out)
            continue;
        const int K = mlp_of(L, params, 0, h1, last, l);
        if (!sde) {
            const int O = L.mlp.n_actions;
            if (logits != nullptr)
                for (int o = 0; o < O; ++o)
                    logits[(size_t)e * (size_t)O + (size_t)o] = policy_canonical(l[o]);
            if (actions != nullptr) {
                int64_t action;
                float log_prob;
                policy_head(l, O, !sampled, sampled ? policy_draw(words, (uint64_t)e) : 0.0, c, &action, &log_prob);
                actions[e] = action;
                if (log_probs != nullptr)
                    log_probs[e] = log_prob;
            }
            continue;
        }
        const float mu = l[0];
        const float s = sde_sigma(last, 1, std2, K);
        float a = mu;
        if (theta != nullptr)
            a = mu + policy_dot(last, 1, theta + (size_t)e * (size_t)K, 1, 0.0f, K);
        if (raw_actions != nullptr)
            raw_actions[e] = policy_canonical(a);
        if (env_actions != nullptr)
            env_actions[e] = sde_env_action(a);
        if (log_probs != nullptr)
            log_probs[e] = sde_log_prob(a, mu, s);
        if (logits != nullptr)
            logits[e] = policy_canonical(mu);
        if (sigma != nullptr)
            sigma[e] = policy_canonical(s);
    }
    return 0;
}

// rf_lstm_critic_ppo_update (sde: rf_lstm_critic_sde_update) on host arrays: 0, or -1 for what the entry point refuses by
// value.  grad_out (or NULL) receives the packed gradient before clipping.
int lcc_update(const rf_lstm_critic_desc *desc, int sde, const rf_ppo_desc *ppo, float *params, float *state, int T, int n,
               const float *obs, const void *actions_any, const float *old_log_probs, const float *advantages,
               const float *returns, const uint8_t *starts, const float *states, int first, int B, float *stats,
               float *grad_out)
{
    LstmLayout L;
    PpoHyper hy;
    LstmPpoWork W;
    if (!layout_of(desc, sde, L) || L.critic != kLstmCriticLinear || !ppo_hyper(*ppo, hy) || T < 1 || n < 1 ||
        (long long)T * n > (1ll << 30))
        return -1;
    const int N = T * n;
    if (B < 1 || B > N || first < 0 || first >= N || !lstm_ppo_work(L, B, W))
        return -1;
    const int64_t *actions = sde ? nullptr : static_cast<const int64_t *>(actions_any);
    const float *raw_actions = sde ? static_cast<const float *>(actions_any) : nullptr;
    const PolicyLayout &M = L.mlp;
    const int D = L.obs_width, H = L.hidden;
    std::vector<float> workspace(W.total, 0.0f);
    float *ws = workspace.data();
    // ---- lstm_ppo_forward_kernel<true>: the pi walks ... ----
    for (int b0 = 0; b0 < B; ++b0) {
        if (!lstm_ppo_is_start(starts, T, n, first, b0))
            continue;
        const int end = lstm_ppo_end(starts, T, n, first, b0, B);
        float h[kPolicyMaxWidth], c[kPolicyMaxWidth], h1[kPolicyMaxWidth];
        {
            const int r = lstm_ppo_row(first, b0, N);
            const int e = r / T, t = r - e * T;
            const bool kept = starts[(size_t)t * (size_t)n + (size_t)e] == 0;
            for (int j = 0; j < H; ++j) {
                h[j] = kept ? states[lstm_ppo_state_at(t, 0, 0, n, H, e, j)] : 0.0f;
                c[j] = kept ? states[lstm_ppo_state_at(t, 0, 1, n, H, e, j)] : 0.0f;
            }
        }
        for (int b = b0; b < end; ++b) {
            const int r = lstm_ppo_row(first, b, N);
            const float *x = obs + (size_t)r * (size_t)D;
            for (int k = 0; k < D; ++k)
                ws[W.x + (size_t)b * (size_t)D + (size_t)k] = x[k];
            for (int j = 0; j < H; ++j) {
                const size_t at = (size_t)b * (size_t)H + (size_t)j;
                ws[W.h_prev[0] + at] = h[j];
                ws[W.c_prev[0] + at] = c[j];
                float a[4], gate[4], c1;
                for (int q = 0; q < 4; ++q) {
                    const int col = q * H + j;
                    float s = params[L.b_ih[0] + (unsigned)col] + params[L.b_hh[0] + (unsigned)col];
                    s = policy_dot(x, 1, params + L.w_ih[0] + col, 4 * H, s, D);
                    a[q] = policy_dot(h, 1, params + L.w_hh[0] + col, 4 * H, s, H);
                }
                lstm_cell_gates(a, c[j], gate, &h1[j], &c1);
                for (int q = 0; q < 4; ++q)
                    ws[W.gates[0] + (size_t)b * (size_t)(4 * H) + (size_t)(q * H + j)] = gate[q];
                ws[W.c1[0] + at] = c1;
                ws[W.h1[0] + at] = h1[j];
                c[j] = c1;
            }
            for (int j = 0; j < H; ++j)
                h[j] = h1[j];
        }
    }
    // ---- ... and the vf net's rows (C6): independent, from the observations alone ----
    for (int b = 0; b < B; ++b)
        critic_of(L, params, obs + (size_t)lstm_ppo_row(first, b, N) * (size_t)D, ws + W.h1[1] + (size_t)b * (size_t)H);
    // ---- lstm_ppo_mlp_kernel ----
    bool invalid = false;
    std::vector<double> tree((size_t)ppo_pow2(B > kPpoMaxPartials ? B : kPpoMaxPartials), 0.0);
    std::vector<int> row((size_t)B);
    for (int b = 0; b < B; ++b) {
        row[b] = lstm_ppo_row(first, b, N);
        if (sde) {
            const float action = raw_actions[row[b]];
            invalid = invalid || action != action;
        } else {
            const int64_t action = actions[row[b]];
            invalid = invalid || action < 0 || action >= M.n_actions;
        }
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
    float logit[kPolicyMaxActions], work[kPolicyMaxActions], std2[kPolicyMaxWidth];
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
            const int O = net == 0 ? M.n_actions : 1;
            for (int o = 0; o < O; ++o)
                logit[o] = policy_dot(in, 1, params + M.weight[net][layers] + o, O, params[M.bias[net][layers] + o], K);
            float *dhead = ws + W.mlp.d[net][layers] + (size_t)b * (size_t)O;
            float *loss = ws + W.mlp.loss + b;
            if (net == 0) {
                const float A = normalise ? ppo_normalised(advantages[row[b]], mean, var) : advantages[row[b]];
                if (sde)
                    sde_pi_sample(logit[0], sde_sigma(in, 1, std2, K), raw_actions[row[b]], old_log_probs[row[b]], A, hy.clip,
                                  hy.ent, Bf, dhead, ws + W.mlp.sde + b, &loss[0], &loss[2 * W.mlp.max_batch],
                                  &loss[3 * W.mlp.max_batch], &loss[4 * W.mlp.max_batch]);
                else
                    ppo_pi_sample(logit, O, (int)ppo_clamp(actions[row[b]], M.n_actions), old_log_probs[row[b]], A, hy.clip,
                                  hy.ent, Bf, work, dhead, 1, &loss[0], &loss[2 * W.mlp.max_batch],
                                  &loss[3 * W.mlp.max_batch], &loss[4 * W.mlp.max_batch]);
            } else {
                ppo_vf_sample(logit[0], returns[row[b]], hy.vf * 2.0f, Bf, &loss[W.mlp.max_batch], dhead);
            }
            const float *dout = dhead;
            int outs = O;
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
            for (int k = 0; k < H; ++k) { // the product into the MLP's input: no activation derivative
                const float *w = params + M.weight[net][0] + (size_t)k * (size_t)outs;
                float acc = 0.0f;
                for (int o = 0; o < outs; ++o)
                    acc = acc + w[o] * dout[o];
                dh[k] = acc;
            }
        }
    // ---- lstm_ppo_bptt_kernel: the pi net only (C7) ----
    for (int b0 = 0; b0 < B; ++b0) {
        if (!lstm_ppo_is_start(starts, T, n, first, b0))
            continue;
        const int end = lstm_ppo_end(starts, T, n, first, b0, B);
        float dh_rec[kPolicyMaxWidth], dc_next[kPolicyMaxWidth];
        for (int j = 0; j < H; ++j)
            dh_rec[j] = dc_next[j] = 0.0f;
        for (int b = end - 1; b >= b0; --b) {
            float *da_row = ws + W.da[0] + (size_t)b * (size_t)(4 * H);
            for (int j = 0; j < H; ++j) {
                const size_t at = (size_t)b * (size_t)H + (size_t)j;
                const float *g = ws + W.gates[0] + (size_t)b * (size_t)(4 * H) + (size_t)j;
                const float gate[4] = {g[0], g[H], g[2 * H], g[3 * H]};
                float da[4];
                dc_next[j] = lstm_bptt_unit(ws[W.dh[0] + at], dh_rec[j], gate, ws[W.c_prev[0] + at], ws[W.c1[0] + at],
                                            dc_next[j], da);
                for (int q = 0; q < 4; ++q)
                    da_row[q * H + j] = da[q];
            }
            if (b == b0)
                break;
            for (int k = 0; k < H; ++k)
                dh_rec[k] = lstm_bptt_rec(params + L.w_hh[0] + (size_t)k * (size_t)(4 * H), da_row, H);
        }
    }
    // ---- lstm_ppo_gradient_kernel<., true> ----
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

#if defined(LSTMCRITICCHECK_MAIN)
// Per head one forward per step and one update of a 2-input, 3-unit actor LSTM beside a 2 -> 3 linear critic, with 3 / 2
// tanh MLPs, over two environments and two steps: the arithmetic under a plain host toolchain (and whatever
// instrumentation it is compiled with), printed for a person to read.
int main()
{
    const int n = 2, T = 2, D = 2, H = 3;
    const float flat_obs[T * n * D] = {0.5f, -1.0f, 2.0f, 0.25f, -0.75f, 0.125f, 1.5f, -0.5f};
    const uint8_t starts[(T + 1) * n] = {1, 1, 0, 1, 0, 0};
    const unsigned long long gen[4] = {0x9e3779b97f4a7c15ull, 0x2545f4914f6cdd1dull, 0xda3e39cb94b95bdbull, 1ull};
    const rf_ppo_desc ppo{3e-4, 0.2, 0.01, 0.5, 0.5, 0.9, 0.999, 1e-5, 1, 0};
    const float advantages[T * n] = {1.0f, -0.5f, 0.25f, 0.75f}, returns[T * n] = {0.3f, -0.2f, 0.1f, 0.4f};
    for (int sde = 0; sde < 2; ++sde) {
        const rf_lstm_critic_desc desc{{{D, sde ? 1 : 3, RF_POLICY_TANH, 1, {3, 0}, 1, {2, 0}}, H}, RF_LSTM_CRITIC_LINEAR};
        const rf_lstm_critic_desc other{desc.lstm, RF_LSTM_CRITIC_LSTM}, unknown{desc.lstm, 2};
        const unsigned P = (unsigned)lcc_params_size(&desc, sde);
        if (P == 0 || lcc_params_size(&unknown, sde) != 0 ||
            lcc_params_size(&other, sde) - P != (unsigned)(4 * H * (D + H) + 8 * H - (D * H + H)) ||
            lcc_workspace_size(&desc, sde, 3) >= lcc_workspace_size(&other, sde, 3))
            return 1;
        std::vector<float> params(P), state(kPpoStateHeader + 2 * P, 0.0f), theta((size_t)n * 3);
        for (unsigned p = 0; p < P; ++p)
            params[p] = 0.25f * (float)((int)(p % 7) - 3);
        for (size_t i = 0; i < theta.size(); ++i)
            theta[i] = 0.125f * (float)((int)(i % 5) - 2);
        std::vector<float> states((size_t)(T + 1) * 4 * n * H, 0.0f);
        long long actions[T * n];
        float raw_actions[T * n], log_probs[T * n];
        for (int t = 0; t < T; ++t) {
            float obs[n * D], step_log_probs[n], values[n], raw[n];
            long long chosen[n];
            for (int e = 0; e < n; ++e)
                for (int k = 0; k < D; ++k)
                    obs[e * D + k] = flat_obs[(e * T + t) * D + k];
            if (lcc_forward(&desc, sde, params.data(), n, obs, starts + t * n, nullptr, states.data() + (size_t)t * 4 * n * H,
                            states.data() + (size_t)(t + 1) * 4 * n * H, gen, 0, theta.data(),
                            sde ? (void *)raw : (void *)chosen, nullptr, step_log_probs, values, nullptr, nullptr,
                            nullptr) != 0)
                return 1;
            for (int e = 0; e < n; ++e) {
                actions[e * T + t] = chosen[e], raw_actions[e * T + t] = raw[e], log_probs[e * T + t] = step_log_probs[e];
                if (sde)
                    printf("sde step %d env %d: action %.9g log_prob %.9g value %.9g\n", t, e, raw[e], step_log_probs[e],
                           values[e]);
                else
                    printf("step %d env %d: action %lld log_prob %.9g value %.9g\n", t, e, chosen[e], step_log_probs[e],
                           values[e]);
            }
        }
        // the vf half of every state is the pi half, and nothing of it is read: poison it before the update
        const size_t slab = (size_t)4 * n * H;
        for (int t = 0; t <= T; ++t)
            for (size_t i = 0; i < slab / 2; ++i) {
                if (t > 0 && memcmp(&states[t * slab + i], &states[t * slab + slab / 2 + i], 4) != 0)
                    return 1;
                states[t * slab + slab / 2 + i] = bits_f32(kPolicyNaN);
            }
        float stats[8];
        if (lcc_update(&desc, sde, &ppo, params.data(), state.data(), T, n, flat_obs,
                       sde ? (const void *)raw_actions : (const void *)actions, log_probs, advantages, returns, starts,
                       states.data(), 1, 3, stats, nullptr) != 0)
            return 1;
        printf(sde ? "sde stats:" : "stats:");
        for (int i = 0; i < 8; ++i)
            printf(" %.9g", stats[i]);
        printf("\n");
        if (stats[7] != 0.0f)
            return 1;
    }
    return 0;
}
#endif
