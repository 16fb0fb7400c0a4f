// policycheck.cpp -- TEST INFRASTRUCTURE.  Compiles the policy's arithmetic (reinfocus_amd/csrc/rf_policy_math.h, the
// exact text policy_forward_kernel inlines, and rf_policy.h's parameter layout) for the host, with a plain loop over the
// same functions in place of the kernel, so that a CPU-only test can compare the definition with the numpy twin before
// any GPU sees it.  Never loaded by the product package.
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_policy.h"

using namespace rf;

extern "C" {

// which: 0 exp32, 1 log32, 2 tanh32 -- y[i] = f(x[i]), stored as computed (no canonical NaN)
void pc_map(int which, const float *x, float *y, long long count)
{
    for (long long i = 0; i < count; ++i)
        y[i] = which == 0 ? exp32(x[i]) : which == 1 ? log32(x[i]) : tanh32(x[i]);
}

int pc_select(const float *c, int A, double u)
{
    return policy_select(c, A, u);
}

// draws number 0 .. lanes-1 after the state gen, each by its own jump as the kernel's lanes take them
void pc_draws(const unsigned long long gen[4], int lanes, double *out)
{
    const uint64_t words[4] = {gen[0], gen[1], gen[2], gen[3]};
    for (int e = 0; e < lanes; ++e)
        out[e] = policy_draw(words, (uint64_t)e);
}

unsigned long long pc_params_size(const rf_policy_desc *desc)
{
    PolicyLayout L;
    return policy_layout(*desc, L) ? L.total : 0;
}

// rf_policy_forward on host arrays: 0, or -1 for a desc outside the limits.  Every output may be NULL.
int pc_forward(const rf_policy_desc *desc, const float *params, int n, const float *obs, const float *final_obs,
               const unsigned long long gen[4], int flags, long long *actions, float *log_probs, float *values,
               float *final_values, float *logits)
{
    PolicyLayout L;
    if (!policy_layout(*desc, L))
        return -1;
    const bool sampled = (flags & RF_POLICY_DETERMINISTIC) == 0;
    const uint64_t words[4] = {gen ? gen[0] : 0, gen ? gen[1] : 0, gen ? gen[2] : 0, gen ? gen[3] : 0};
    float a[kPolicyMaxWidth], b[kPolicyMaxWidth], l[kPolicyMaxActions], c[kPolicyMaxActions];
    for (int e = 0; e < n; ++e) {
        for (int net = 0; net < 2; ++net) {
            for (int pass = 0; pass < (net == 1 && final_obs != nullptr && final_values != nullptr ? 2 : 1); ++pass) {
                const float *in = (pass == 0 ? obs : final_obs) + (size_t)e * (size_t)L.obs_width;
                float *x = a, *y = b;
                int K = L.obs_width;
                for (int k = 0; k < K; ++k)
                    x[k] = in[k];
                for (int layer = 0; layer < L.layers[net]; ++layer) {
                    const int H = L.width[net][layer];
                    for (int j = 0; j < H; ++j)
                        y[j] = policy_activation(policy_dot(x, 1, params + L.weight[net][layer] + j, H,
                                                            params[L.bias[net][layer] + j], K), L.activation);
                    float *t = x;
                    x = y, y = t, K = H;
                }
                const int head = L.layers[net], O = net == 0 ? L.n_actions : 1;
                for (int o = 0; o < O; ++o)
                    l[o] = policy_dot(x, 1, params + L.weight[net][head] + o, O, params[L.bias[net][head] + o], K);
                if (net == 1) {
                    if (pass == 0 && values != nullptr)
                        values[e] = policy_canonical(l[0]);
                    if (pass == 1)
                        final_values[e] = in[0] != in[0] ? bits_f32(kPolicyNaN) : policy_canonical(l[0]);
                    continue;
                }
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
            }
        }
    }
    return 0;
}

} // extern "C"
