// lstmppocheck.cpp -- TEST INFRASTRUCTURE.  Compiles the recurrent PPO update's arithmetic (reinfocus_amd/csrc/
// rf_lstm_ppo.h: the sequence rule, the cell with its gates, the BPTT functions, the workspace layout and the
// parameter-to-source map, with what it takes from rf_ppo.h and rf_lstm.h) for the host, with plain loops in place of
// the kernels, so that a CPU-only test can compare the definition with the numpy twin (environments/lstm_learner.py
// lstm_update_numpy) before any GPU sees it.  Never loaded by the product package.
#include <stdint.h>

#include <vector>

#include "../../reinfocus_amd/csrc/rf_lstm_ppo.h"

using namespace rf;

extern "C" {

unsigned long long lpc_state_size(const rf_lstm_policy_desc *desc)
{
    LstmLayout L;
    return lstm_layout(*desc, L) ? 4ull * kPpoStateHeader + 8ull * L.total : 0;
}

unsigned long long lpc_workspace_size(const rf_lstm_policy_desc *desc, int max_batch)
{
    LstmLayout L;
    LstmPpoWork W;
    return lstm_layout(*desc, L) && lstm_ppo_work(L, max_batch, W) ? 4ull * W.total : 0;
}

// offset in floats of the packed gradient inside a workspace laid out for minibatches of max_batch; 0 if refused
unsigned long long lpc_grad_offset(const rf_lstm_policy_desc *desc, int max_batch)
{
    LstmLayout L;
    LstmPpoWork W;
    return lstm_layout(*desc, L) && lstm_ppo_work(L, max_batch, W) ? W.mlp.grad : 0;
}

// The sequence rule: rows[b] = r_b, start[b] = 1 where row b starts a sequence, end[b] = one past its sequence's last row
// (start rows only, else 0)
int lpc_sequences(const uint8_t *starts, int T, int n, int first, int B, int *rows, int *start, int *end)
{
    for (int b = 0; b < B; ++b) {
        rows[b] = lstm_ppo_row(first, b, T * n);
        start[b] = lstm_ppo_is_start(starts, T, n, first, b) ? 1 : 0;
        end[b] = start[b] ? lstm_ppo_end(starts, T, n, first, b, B) : 0;
    }
    return 0;
}

// rf_lstm_ppo_update on host arrays: 0, or -1 for what the entry point refuses by value.  grad_out (or NULL) receives
// the packed gradient before clipping.
int lpc_update(const rf_lstm_policy_desc *desc, const rf_ppo_desc *ppo, float *params, float *state, int T, int n,
               const float *obs, const long long *actions, const float *old_log_probs, const float *advantages,
               const float *returns, const uint8_t *starts, const float *states, int first, int B, float *stats,
               float *grad_out)
{
    LstmLayout L;
    PpoHyper hy;
    LstmPpoWork W;
    if (!lstm_layout(*desc, L) || !ppo_hyper(*ppo, hy) || T < 1 || n < 1 || (long long)T * n > (1ll << 30))
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
    // ---- lstm_ppo_mlp_kernel ----
    bool invalid = false;
    std::vector<double> tree((size_t)ppo_pow2(B > kPpoMaxPartials ? B : kPpoMaxPartials), 0.0);
    std::vector<int> row((size_t)B);
    for (int b = 0; b < B; ++b) {
        row[b] = lstm_ppo_row(first, b, N);
        const int64_t action = actions[row[b]];
        invalid = invalid || action < 0 || action >= M.n_actions;
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
    float logit[kPolicyMaxActions], work[kPolicyMaxActions];
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
                ppo_pi_sample(logit, O, (int)ppo_clamp(actions[row[b]], M.n_actions), old_log_probs[row[b]], A, hy.clip,
                              hy.ent, Bf, work, dhead, 1, &loss[0], &loss[2 * W.mlp.max_batch], &loss[3 * W.mlp.max_batch],
                              &loss[4 * W.mlp.max_batch]);
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
    // ---- lstm_ppo_gradient_kernel ----
    std::vector<double> partial((size_t)W.mlp.partials, 0.0);
    for (unsigned block = 0; block < W.mlp.partials; ++block) {
        double leaves[kPpoLeaves];
        for (unsigned t = 0; t < (unsigned)kPpoLeaves; ++t) {
            const unsigned p = block * kPpoLeaves + t;
            leaves[t] = 0.0;
            if (p < L.total) {
                const float g = policy_canonical(ppo_gradient(ws, lstm_ppo_source(L, W, p), B));
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
