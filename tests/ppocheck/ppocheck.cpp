// ppocheck.cpp -- TEST INFRASTRUCTURE.  Compiles the PPO update's arithmetic (reinfocus_amd/csrc/rf_ppo.h: the plain-C++
// functions the three kernels inline, the workspace layout and the parameter-to-source map) for the host, with plain
// loops in place of the kernels, so that a CPU-only test can compare the definition with the numpy twin
// (environments/learner.py ppo_update_numpy) before any GPU sees it.  Never loaded by the product package.
#include <stdint.h>

#include <vector>

#include "../../reinfocus_amd/csrc/rf_ppo.h"

using namespace rf;

extern "C" {

unsigned long long ppc_state_size(const rf_policy_desc *desc)
{
    PolicyLayout L;
    return policy_layout(*desc, L) ? 4ull * kPpoStateHeader + 8ull * L.total : 0;
}

unsigned long long ppc_workspace_size(const rf_policy_desc *desc, int max_batch)
{
    PolicyLayout L;
    PpoWork W;
    return policy_layout(*desc, L) && ppo_work(L, max_batch, W) ? 4ull * W.total : 0;
}

// rf_ppo_update on host arrays: 0, or -1 for what the entry point refuses by value.  grad_out (or NULL) receives the
// packed gradient before clipping.
int ppc_update(const rf_policy_desc *desc, const rf_ppo_desc *ppo, float *params, float *state, int N, const float *obs,
               const long long *actions, const float *old_log_probs, const float *advantages, const float *returns, int B,
               const long long *index, float *stats, float *grad_out)
{
    PolicyLayout L;
    PpoHyper hy;
    PpoWork W;
    if (!policy_layout(*desc, L) || !ppo_hyper(*ppo, hy) || N < 1 || !ppo_work(L, B, W))
        return -1;
    std::vector<float> workspace(W.total, 0.0f);
    float *ws = workspace.data();
    // ---- ppo_backward_kernel ----
    bool invalid = false;
    std::vector<double> tree((size_t)ppo_pow2(B > (int)W.partials ? B : (int)W.partials), 0.0);
    std::vector<int64_t> row((size_t)B);
    for (int b = 0; b < B; ++b) {
        row[b] = ppo_clamp(index[b], N);
        const int64_t action = actions[row[b]];
        invalid = invalid || row[b] != index[b] || action < 0 || action >= L.n_actions;
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
    for (int b = 0; b < B; ++b) {
        float *x = ws + W.x + (size_t)b * (size_t)L.obs_width;
        for (int k = 0; k < L.obs_width; ++k)
            x[k] = obs[(size_t)row[b] * (size_t)L.obs_width + (size_t)k];
        for (int net = 0; net < 2; ++net) {
            const int layers = L.layers[net];
            const float *in = x;
            int K = L.obs_width;
            for (int layer = 0; layer < layers; ++layer) {
                const int H = L.width[net][layer];
                float *h = ws + W.h[net][layer] + (size_t)b * (size_t)H;
                for (int j = 0; j < H; ++j)
                    h[j] = policy_activation(policy_dot(in, 1, params + L.weight[net][layer] + j, H,
                                                        params[L.bias[net][layer] + j], K), L.activation);
                in = h, K = H;
            }
            const int O = net == 0 ? L.n_actions : 1;
            for (int o = 0; o < O; ++o)
                logit[o] = policy_dot(in, 1, params + L.weight[net][layers] + o, O, params[L.bias[net][layers] + o], K);
            float *dhead = ws + W.d[net][layers] + (size_t)b * (size_t)O;
            float *loss = ws + W.loss + b;
            if (net == 0) {
                const float A = normalise ? ppo_normalised(advantages[row[b]], mean, var) : advantages[row[b]];
                ppo_pi_sample(logit, O, (int)ppo_clamp(actions[row[b]], L.n_actions), old_log_probs[row[b]], A, hy.clip,
                              hy.ent, Bf, work, dhead, 1, &loss[0], &loss[2 * W.max_batch], &loss[3 * W.max_batch],
                              &loss[4 * W.max_batch]);
            } else {
                ppo_vf_sample(logit[0], returns[row[b]], hy.vf * 2.0f, Bf, &loss[W.max_batch], dhead);
            }
            const float *dout = dhead;
            int outs = O;
            for (int layer = layers - 1; layer >= 0; --layer) {
                const int H = L.width[net][layer];
                const float *h = ws + W.h[net][layer] + (size_t)b * (size_t)H;
                float *din = ws + W.d[net][layer] + (size_t)b * (size_t)H;
                for (int k = 0; k < H; ++k)
                    din[k] = ppo_back(params + L.weight[net][layer + 1] + (size_t)k * (size_t)outs, dout, 1, outs, h[k],
                                      L.activation);
                dout = din, outs = H;
            }
        }
    }
    // ---- ppo_gradient_kernel ----
    for (unsigned block = 0; block < W.partials; ++block) {
        double leaves[kPpoLeaves];
        for (unsigned t = 0; t < (unsigned)kPpoLeaves; ++t) {
            const unsigned p = block * kPpoLeaves + t;
            leaves[t] = 0.0;
            if (p < L.total) {
                const float g = ppo_gradient(ws, ppo_source(L, W, p), B);
                ws[W.grad + p] = g;
                leaves[t] = (double)g * (double)g;
            }
        }
        for (int s = 1; s < kPpoLeaves; s <<= 1)
            for (int i = 0; i < kPpoLeaves; i += 2 * s)
                leaves[i] = leaves[i] + leaves[i + s];
        tree[block] = leaves[0];
    }
    if (grad_out != nullptr)
        for (unsigned p = 0; p < L.total; ++p)
            grad_out[p] = ws[W.grad + p];
    // ---- ppo_adam_kernel ----
    const int size = ppo_pow2((int)W.partials);
    for (int i = (int)W.partials; i < size; ++i)
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
            tree[b] = b < B ? (double)ws[W.loss + (size_t)term * W.max_batch + b] : 0.0;
        sums[term] = ppo_treesum_host(tree.data(), batch);
    }
    ppo_stats(sums, B, norm, hy, flags, stats);
    if (flags != 0)
        return 0;
    float *m = state + kPpoStateHeader, *v = m + L.total;
    for (unsigned p = 0; p < L.total; ++p)
        ppo_adam(step, ws[W.grad + p], params + p, m + p, v + p);
    memcpy(state, &step.next, sizeof step.next);
    return 0;
}

} // extern "C"
