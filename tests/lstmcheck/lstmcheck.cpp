// lstmcheck.cpp -- TEST INFRASTRUCTURE.  Compiles the lstm policy's arithmetic (reinfocus_amd/csrc/rf_policy_math.h:
// sigmoid32 and what "policy" has; rf_lstm.h: the cell and the parameter layout -- the exact text lstm_forward_kernel
// inlines) for the host, with a plain loop over the same functions in place of the kernel, so that a CPU-only test can
// compare the definition with the numpy twin before any GPU sees it.  Never loaded by the product package.
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_lstm.h"

using namespace rf;

extern "C" {

// y[i] = sigmoid32(x[i]), stored as computed
void lc_sigmoid(const float *x, float *y, long long count)
{
    for (long long i = 0; i < count; ++i)
        y[i] = sigmoid32(x[i]);
}

// lstm_cell on `count` rows of gate sums a[count][4] (i, f, g, o) and cell states c[count]
void lc_cell(const float *a, const float *c, float *h1, float *c1, long long count)
{
    for (long long i = 0; i < count; ++i)
        lstm_cell(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3], c[i], &h1[i], &c1[i]);
}

unsigned long long lc_params_size(const rf_lstm_policy_desc *desc)
{
    LstmLayout L;
    return lstm_layout(*desc, L) ? L.total : 0;
}

unsigned long long lc_state_size(const rf_lstm_policy_desc *desc, int n)
{
    LstmLayout L;
    return lstm_layout(*desc, L) && n >= 1 ? lstm_state_floats(n, L.hidden) : 0;
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

// the MLP and head of a net on h1: l[0 .. O-1]
static void mlp_of(const LstmLayout &L, const float *params, int net, const float *h1, float *l)
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
    const int head = M.layers[net], O = net == 0 ? M.n_actions : 1;
    for (int o = 0; o < O; ++o)
        l[o] = policy_dot(x, 1, params + M.weight[net][head] + o, O, params[M.bias[net][head] + o], K);
}

// rf_lstm_forward on host arrays: 0, or -1 for a desc outside the limits.  state_out and every output may be NULL;
// state_out may be state_in.
int lc_forward(const rf_lstm_policy_desc *desc, const float *params, int n, const float *obs, const uint8_t *starts,
               const float *final_obs, const float *state_in, float *state_out, const unsigned long long gen[4], int flags,
               long long *actions, float *log_probs, float *values, float *final_values, float *logits)
{
    LstmLayout L;
    if (!lstm_layout(*desc, L))
        return -1;
    const int D = L.obs_width, H = L.hidden;
    const bool sampled = (flags & RF_POLICY_DETERMINISTIC) == 0;
    const uint64_t words[4] = {gen ? gen[0] : 0, gen ? gen[1] : 0, gen ? gen[2] : 0, gen ? gen[3] : 0};
    float h1[kPolicyMaxWidth], c1[kPolicyMaxWidth], l[kPolicyMaxActions], c[kPolicyMaxActions];
    for (int e = 0; e < n; ++e) {
        if (final_obs != nullptr && final_values != nullptr) { // first: it reads state_in, which may be state_out
            const float *in = final_obs + (size_t)e * (size_t)D;
            cell_of(L, params, 1, n, e, in, state_in, false, h1, c1);
            mlp_of(L, params, 1, h1, l);
            final_values[e] = in[0] != in[0] ? bits_f32(kPolicyNaN) : policy_canonical(l[0]);
        }
        const float *x = obs + (size_t)e * (size_t)D;
        const bool reset = starts[e] != 0;
        for (int net = 0; net < 2; ++net) {
            const bool heads = net == 0 ? actions != nullptr || logits != nullptr : values != nullptr;
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
            mlp_of(L, params, net, h1, l);
            if (net == 1) {
                values[e] = policy_canonical(l[0]);
                continue;
            }
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
        }
    }
    return 0;
}

} // extern "C"
