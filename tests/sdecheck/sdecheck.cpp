// sdecheck.cpp -- TEST INFRASTRUCTURE.  Compiles the sde policy's arithmetic (reinfocus_amd/csrc/rf_policy_math.h: normal32,
// expw32, log32, the sde_* functions; rf_ppo.h: the Gaussian head of the update; rf_sde.h: sde_theta) for the host, with
// plain loops in place of the kernels, so that a CPU-only test can compare the definition with the numpy twin
// (environments/sde.py, environments/learner.py) before any GPU sees it.  Never loaded by the product package.
// With -DSDECHECK_MAIN it is a program: one reset, forward and update of a tiny network, printed.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../reinfocus_amd/csrc/rf_sde.h"

using namespace rf;

extern "C" {

void sdc_normal32(const double *u, int count, float *out)
{
    for (int i = 0; i < count; ++i)
        out[i] = normal32(u[i]);
}

void sdc_log64(const double *x, int count, double *out)
{
    for (int i = 0; i < count; ++i)
        out[i] = log64(x[i]);
}

void sdc_log32(const float *x, int count, float *out)
{
    for (int i = 0; i < count; ++i)
        out[i] = log32(x[i]);
}

void sdc_expw32(const float *x, int count, float *out)
{
    for (int i = 0; i < count; ++i)
        out[i] = expw32(x[i]);
}

unsigned long long sdc_params_size(const rf_policy_desc *desc)
{
    PolicyLayout L;
    return sde_layout(*desc, L) ? L.total : 0;
}

unsigned long long sdc_state_size(const rf_policy_desc *desc)
{
    PolicyLayout L;
    return sde_layout(*desc, L) ? 4ull * kPpoStateHeader + 8ull * L.total : 0;
}

unsigned long long sdc_workspace_size(const rf_policy_desc *desc, int max_batch)
{
    PolicyLayout L;
    PpoWork W;
    return sde_layout(*desc, L) && ppo_work(L, max_batch, W) ? 4ull * W.total : 0;
}

// rf_sde_noise_reset on host arrays
int sdc_noise(const rf_policy_desc *desc, const float *params, int n, const unsigned long long gen[4], float *theta)
{
    PolicyLayout L;
    if (!sde_layout(*desc, L) || n < 1)
        return -1;
    const uint64_t words[4] = {gen[0], gen[1], gen[2], gen[3]};
    for (size_t i = 0; i < (size_t)n * L.sde; ++i)
        theta[i] = sde_theta(words, (uint64_t)i, params[L.log_std + i % L.sde]);
    return 0;
}

// one net of one row: the last hidden activations go to h (kPolicyMaxWidth floats), the head's output is returned
static float net_row(const PolicyLayout &L, const float *params, int net, const float *x, float *h, int *K_out)
{
    float a[kPolicyMaxWidth], b[kPolicyMaxWidth];
    const float *in = x;
    int K = L.obs_width;
    for (int layer = 0; layer < L.layers[net]; ++layer) {
        float *out = layer == 0 ? a : b;
        const int H = L.width[net][layer];
        for (int j = 0; j < H; ++j)
            out[j] = policy_activation(policy_dot(in, 1, params + L.weight[net][layer] + j, H, params[L.bias[net][layer] + j], K),
                                       L.activation);
        in = out, K = H;
    }
    for (int k = 0; k < K; ++k)
        h[k] = in[k];
    *K_out = K;
    const int head = L.layers[net];
    return policy_dot(h, 1, params + L.weight[net][head], 1, params[L.bias[net][head]], K);
}

// rf_sde_forward on host arrays (theta NULL: deterministic).  Every output may be NULL.
int sdc_forward(const rf_policy_desc *desc, const float *params, int n, const float *obs, const float *final_obs,
                const float *theta, float *actions, float *env_actions, float *log_probs, float *values,
                float *final_values, float *mean, float *sigma)
{
    PolicyLayout L;
    if (!sde_layout(*desc, L) || n < 1)
        return -1;
    float std2[kPolicyMaxWidth], h[kPolicyMaxWidth];
    for (unsigned k = 0; k < L.sde; ++k)
        std2[k] = sde_std2(params[L.log_std + k]);
    for (int e = 0; e < n; ++e) {
        const float *x = obs + (size_t)e * (size_t)L.obs_width;
        int K;
        if (values != nullptr)
            values[e] = policy_canonical(net_row(L, params, 1, x, h, &K));
        if (final_values != nullptr) {
            const float *fx = final_obs + (size_t)e * (size_t)L.obs_width;
            const float y = net_row(L, params, 1, fx, h, &K);
            final_values[e] = fx[0] != fx[0] ? bits_f32(kPolicyNaN) : policy_canonical(y);
        }
        const float mu = net_row(L, params, 0, x, h, &K);
        const float s = sde_sigma(h, 1, std2, K);
        float a = mu;
        if (theta != nullptr)
            a = mu + policy_dot(h, 1, theta + (size_t)e * (size_t)K, 1, 0.0f, K);
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
    return 0;
}

// rf_sde_update on host arrays: 0, or -1 for what the entry point refuses by value.  grad_out (or NULL) receives the
// packed gradient (P + L) before clipping.
int sdc_update(const rf_policy_desc *desc, const rf_ppo_desc *ppo, float *params, float *state, int N, const float *obs,
               const float *actions, const float *old_log_probs, const float *advantages, const float *returns, int B,
               const long long *index, float *stats, float *grad_out)
{
    PolicyLayout L;
    PpoHyper hy;
    PpoWork W;
    if (!sde_layout(*desc, L) || !ppo_hyper(*ppo, hy) || N < 1 || !ppo_work(L, B, W))
        return -1;
    std::vector<float> workspace(W.total, 0.0f);
    float *ws = workspace.data();
    // ---- ppo_backward_kernel<true> ----
    bool invalid = false;
    std::vector<double> tree((size_t)ppo_pow2(B > (int)W.partials ? B : (int)W.partials), 0.0);
    std::vector<int64_t> row((size_t)B);
    for (int b = 0; b < B; ++b) {
        row[b] = ppo_clamp(index[b], N);
        const float action = actions[row[b]];
        invalid = invalid || row[b] != index[b] || action != action;
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
    for (unsigned k = 0; k < L.sde; ++k)
        std2[k] = sde_std2(params[L.log_std + k]);
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
            const float y = policy_dot(in, 1, params + L.weight[net][layers], 1, params[L.bias[net][layers]], K);
            float *dhead = ws + W.d[net][layers] + b;
            float *loss = ws + W.loss + b;
            if (net == 0) {
                const float A = normalise ? ppo_normalised(advantages[row[b]], mean, var) : advantages[row[b]];
                sde_pi_sample(y, sde_sigma(in, 1, std2, K), actions[row[b]], old_log_probs[row[b]], A, hy.clip, hy.ent, Bf,
                              dhead, ws + W.sde + b, &loss[0], &loss[2 * W.max_batch], &loss[3 * W.max_batch],
                              &loss[4 * W.max_batch]);
            } else {
                ppo_vf_sample(y, returns[row[b]], hy.vf * 2.0f, Bf, &loss[W.max_batch], dhead);
            }
            const float *dout = dhead;
            int outs = 1;
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
                const float g = ppo_parameter_gradient(L, W, ws, params, p, B);
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

#if defined(SDECHECK_MAIN)
// One reset, forward and update of a 2-3-1 / 2-2-1 tanh network over two environments: the arithmetic under a plain
// host toolchain (and whatever instrumentation it is compiled with), printed for a person to read.
int main()
{
    const rf_policy_desc desc{2, 1, RF_POLICY_TANH, 1, {3, 0}, 1, {2, 0}};
    const unsigned P = (unsigned)sdc_params_size(&desc);
    std::vector<float> params(P), state(kPpoStateHeader + 2 * P, 0.0f), theta(2 * 3);
    for (unsigned p = 0; p < P; ++p)
        params[p] = 0.25f * (float)((int)(p % 7) - 3);
    const unsigned long long gen[4] = {0x9e3779b97f4a7c15ull, 0x2545f4914f6cdd1dull, 0xda3e39cb94b95bdbull, 1ull};
    if (sdc_noise(&desc, params.data(), 2, gen, theta.data()) != 0)
        return 1;
    const float obs[4] = {0.5f, -1.0f, 2.0f, 0.25f};
    float actions[2], env_actions[2], log_probs[2], values[2], mean[2], sigma[2];
    if (sdc_forward(&desc, params.data(), 2, obs, nullptr, theta.data(), actions, env_actions, log_probs, values, nullptr, mean,
                    sigma) != 0)
        return 1;
    for (int e = 0; e < 2; ++e)
        printf("env %d: action %.9g (to the environment %.9g) log_prob %.9g value %.9g mean %.9g sigma %.9g\n", e, actions[e],
               env_actions[e], log_probs[e], values[e], mean[e], sigma[e]);
    const rf_ppo_desc ppo{3e-4, 0.2, 0.01, 0.5, 0.5, 0.9, 0.999, 1e-5, 1, 0};
    const float advantages[2] = {1.0f, -0.5f}, returns[2] = {0.3f, -0.2f};
    const long long index[2] = {1, 0};
    float stats[8];
    if (sdc_update(&desc, &ppo, params.data(), state.data(), 2, obs, actions, log_probs, advantages, returns, 2, index, stats,
                   nullptr) != 0)
        return 1;
    printf("stats:");
    for (int i = 0; i < 8; ++i)
        printf(" %.9g", stats[i]);
    printf("\n");
    return stats[7] == 0.0f ? 0 : 1;
}
#endif
