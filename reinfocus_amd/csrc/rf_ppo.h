// rf_ppo.h -- one PPO minibatch update in three launches (include/reinfocus_hip.h, "ppo update"): stable-baselines3's
// PPO.train() body for the actor-critic of rf_policy.h -- loss, backward, clip_grad_norm_, Adam -- in the fixed order of
// the definition, bit for bit equal to the numpy twin (environments/learner.py ppo_update_numpy).
//
//   ppo_backward_kernel  grid ceil(B / 8) x 2 as policy_forward_kernel: a block owns one net and a tile of 8 samples.  pi
//                        blocks recompute the validity flag and the advantage moments from the B gathered values
//                        (identical bits in every block: no launch of their own), then every block runs the forward
//                        (policy_hidden_tile and policy_dot of rf_policy.h) with the activations kept in LDS, the head
//                        deltas of its 8 samples (one lane each) and the back-propagation (thread k owns hidden unit k
//                        with 8 accumulators), and writes x / h / delta per layer as [b][width] and the loss terms.
//   ppo_gradient_kernel  one thread per packed parameter (k, j), j fastest: delta[b][j] loads are coalesced, x[b][k] is
//                        wave-uniform; the loop over b is sequential and unrolled 8 times.  Writes grad[P] and one
//                        float64 tree sum of squares per block of 256.
//   ppo_adam_kernel      every block reduces those partials by the same tree (the same norm everywhere), applies the
//                        skip rule, the clip and Adam to its slice; one extra block writes the stats and the next header.
//                        The header the blocks read is the copy ppo_backward_kernel left in the workspace, so no block
//                        reads what another block of its launch writes.
// No atomics, no grid synchronisation.  The scalar arithmetic is plain C++ (RF_HD): tests/ppocheck loops over the same
// functions on the host.
// The Gaussian head of "sde policy" (rf_sde_update) is the same three kernels: ppo_backward_kernel<true> runs sde_pi_sample
// in place of ppo_pi_sample and leaves one float per sample in the workspace, ppo_gradient_kernel's threads past the two
// nets sum the log_std gradients from it, and ppo_adam_kernel covers the P + L parameters of sde_layout (tests/sdecheck).
#pragma once

#include "rf_policy.h"

namespace rf {

constexpr int kPpoMaxBatch = RF_PPO_MAX_BATCH;
constexpr int kPpoThreads = 256;
constexpr int kPpoLeaves = 256;        // packed gradients per block of ppo_gradient_kernel: one aligned subtree of the norm
constexpr int kPpoAdamSlice = 1024;    // parameters per block of ppo_adam_kernel
constexpr int kPpoMaxPartials = 2048;  // >= ceil(P / kPpoLeaves) for every desc inside the limits (checked by ppo_work)
constexpr int kPpoStateHeader = 8;     // floats: {int64 step, double bc1, double bc2, int64 0}
static_assert(kPpoThreads == kPolicyThreads && kPpoMaxBatch <= kPpoMaxPartials, "shared tile code and reduction buffer");

struct PpoHeader {
    int64_t step;
    double bc1, bc2;
    int64_t zero;
};

// rf_ppo_desc as the kernels read it
struct PpoHyper {
    double learning_rate, max_grad_norm, beta1, beta2, adam_eps;
    float clip, ent, vf;
    int normalize;
};
static_assert(sizeof(PpoHyper) == sizeof(rf_ppo_hyper) && sizeof(PpoHyper) == 56, "rf_ppo_hyper is PpoHyper (population)");

// false: a hyper-parameter is negative or not finite, or a beta is outside [0, 1)
RF_HD bool ppo_hyper(const rf_ppo_desc &d, PpoHyper &h)
{
    const double all[8] = {d.learning_rate, d.clip_range, d.ent_coef, d.vf_coef, d.max_grad_norm, d.beta1, d.beta2, d.adam_eps};
    for (int i = 0; i < 8; ++i)
        if (!(all[i] >= 0.0 && all[i] <= 1.7976931348623157e308))
            return false;
    if (!(d.beta1 < 1.0 && d.beta2 < 1.0) || (d.normalize_advantage != 0 && d.normalize_advantage != 1))
        return false;
    h.learning_rate = d.learning_rate, h.max_grad_norm = d.max_grad_norm, h.beta1 = d.beta1, h.beta2 = d.beta2;
    h.adam_eps = d.adam_eps;
    h.clip = (float)d.clip_range, h.ent = (float)d.ent_coef, h.vf = (float)d.vf_coef;
    h.normalize = d.normalize_advantage;
    return true;
}

// The workspace: offsets in floats, each even (float64 data sits at 8-byte boundaries).  Rows are [b][width].
struct PpoWork {
    unsigned header;  // PpoHeader as the update found it
    unsigned flag;    // int: 1 where the minibatch is invalid
    unsigned loss;    // [5][max_batch]: pg, vl, H, kl, clipped
    unsigned x;       // [max_batch][D]: the gathered observations
    unsigned h[2][2]; // [net][hidden layer]: activations
    unsigned d[2][3]; // [net][hidden layer, or the head at index `layers`]: deltas
    unsigned grad;    // [P]
    unsigned partial; // double [ceil(P / kPpoLeaves)]
    unsigned partials;
    unsigned max_batch;
    unsigned total;
    unsigned sde;     // [max_batch]: (dLoss / dsigma_b) / sigma_b of the Gaussian head (sde_layout only; taken last)
};

RF_HD bool ppo_work(const PolicyLayout &L, int max_batch, PpoWork &w)
{
    w = PpoWork{};
    if (max_batch < 1 || max_batch > kPpoMaxBatch)
        return false;
    const unsigned rows = (unsigned)max_batch;
    unsigned at = 0;
    auto take = [&at](unsigned floats) {
        const unsigned here = at;
        at += (floats + 1u) & ~1u;
        return here;
    };
    w.header = take(kPpoStateHeader);
    w.flag = take(2);
    w.loss = take(5 * rows);
    w.x = take(rows * (unsigned)L.obs_width);
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l <= L.layers[net]; ++l) {
            const unsigned width = l < L.layers[net] ? (unsigned)L.width[net][l] : (net == 0 ? (unsigned)L.n_actions : 1u);
            if (l < L.layers[net])
                w.h[net][l] = take(rows * width);
            w.d[net][l] = take(rows * width);
        }
    w.grad = take(L.total);
    w.partials = (L.total + kPpoLeaves - 1) / kPpoLeaves;
    if (w.partials > (unsigned)kPpoMaxPartials)
        return false;
    w.partial = take(2 * w.partials);
    if (L.sde != 0)
        w.sde = take(rows);
    w.max_batch = rows;
    w.total = at;
    return true;
}

// "population": G groups of `rows` rows each; false outside the limits of the definition
RF_HD bool population_rows(int G, long long rows)
{
    return G >= 1 && G <= RF_POPULATION_MAX_GROUPS && rows >= 1 && (long long)G * rows <= (1ll << 30);
}

// What rf_ppo_grouped_state_size and rf_ppo_grouped_workspace_size return for a ctx (0: refused): G times the ungrouped
// sizes, for minibatches of B out of the m T rows of a group.  sde ("population sde", rf_sde_grouped_*): over sde_layout's
// P + L parameters.
RF_HD unsigned long long population_state_bytes(const rf_policy_desc &d, int G, int m, bool sde = false)
{
    PolicyLayout L;
    if (!(sde ? sde_layout(d, L) : policy_layout(d, L)) || !population_rows(G, m))
        return 0;
    return (unsigned long long)G * (4ull * kPpoStateHeader + 8ull * L.total);
}

RF_HD unsigned long long population_workspace_bytes(const rf_policy_desc &d, int G, int m, int T, int B, bool sde = false)
{
    PolicyLayout L;
    PpoWork W;
    if (!(sde ? sde_layout(d, L) : policy_layout(d, L)) || m < 1 || T < 1 || !population_rows(G, (long long)m * (long long)T)
        || (long long)B > (long long)m * (long long)T || !ppo_work(L, B, W))
        return 0;
    return (unsigned long long)G * 4ull * W.total;
}

RF_HD int64_t ppo_clamp(int64_t i, int64_t n)
{
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

RF_HD bool ppo_finite(double x)
{
    return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308;
}

RF_HD int ppo_pow2(int n)
{
    int p = 1;
    while (p < n)
        p <<= 1;
    return p;
}

// A_b of definition step 2 from the batch moments
RF_HD float ppo_normalised(float adv, double mean, double var)
{
    return (float)(((double)adv - mean) / (sqrt(var) + 1e-8));
}

// Definition steps 4 and 5 from d = log_prob - old_log_prob on, shared by both heads: the loss terms, and g_b
RF_HD float ppo_surrogate(float d, float adv, float c, float *pg, float *kl, float *clipped)
{
    const float ratio = d <= 0.0f ? exp32(d) : 1.0f / exp32(-d);
    const float lo = 1.0f - c, hi = 1.0f + c;
    const float cl = ratio < lo ? lo : (ratio > hi ? hi : ratio);
    const float surr1 = adv * ratio, surr2 = adv * cl;
    *pg = -(surr2 < surr1 ? surr2 : surr1);
    const float r1 = ratio - 1.0f;
    *kl = r1 - d;
    *clipped = (r1 < 0.0f ? -r1 : r1) > c ? 1.0f : 0.0f;
    return ((ratio >= lo && ratio <= hi) || surr1 < surr2) ? surr1 : 0.0f;
}

// Definition steps 3 to 5 of one sample's pi head: logits l[0 .. A-1], its action a (clamped), the stored
// log-probability, A_b.  work: A floats (the e_i).  dlogit[i * stride] receives the head deltas.
RF_HD void ppo_pi_sample(const float *l, int A, int a, float old_log_prob, float adv, float c, float ec, float Bf,
                         float *work, float *dlogit, int stride, float *pg, float *entropy, float *kl, float *clipped)
{
    float m = l[0];
    for (int i = 1; i < A; ++i)
        if (l[i] > m)
            m = l[i];
    float s = 0.0f;
    for (int i = 0; i < A; ++i) {
        const float e = exp32(l[i] - m);
        work[i] = e;
        s = s + e;
    }
    const float lse = s >= 1.0f ? log32(s) : bits_f32(kPolicyNaN);
    float acc = 0.0f;
    for (int i = 0; i < A; ++i) {
        const float logp = (l[i] - m) - lse;
        const float p = work[i] / s;
        acc = acc + (work[i] == 0.0f ? 0.0f : p * logp);
    }
    const float H = -acc;
    const float d = ((l[a] - m) - lse) - old_log_prob;
    *entropy = H;
    const float ng = -ppo_surrogate(d, adv, c, pg, kl, clipped);
    for (int i = 0; i < A; ++i) {
        const float logp = (l[i] - m) - lse;
        const float p = work[i] / s;
        const float pull = ng * ((i == a ? 1.0f : 0.0f) - p);
        const float ent = work[i] == 0.0f ? 0.0f : (ec * p) * (logp + H);
        dlogit[(size_t)i * (size_t)stride] = (pull + ent) / Bf;
    }
}

// The same steps of the Gaussian head ("sde policy", steps 3', 5'): the stored raw action a, the mean mu, sigma.
// dmu is the head delta; dsig = (dLoss / dsigma_b) / sigma_b, what the log_std gradient sums.  A row whose sigma or
// log_prob is not finite makes both NaN, so the update ends in RF_PPO_NONFINITE.
RF_HD void sde_pi_sample(float mu, float sigma, float a, float old_log_prob, float adv, float c, float ec, float Bf,
                         float *dmu, float *dsig, float *pg, float *entropy, float *kl, float *clipped)
{
    const float lp = sde_log_prob(a, mu, sigma);
    *entropy = sde_entropy(sigma);
    const float ng = -ppo_surrogate(lp - old_log_prob, adv, c, pg, kl, clipped);
    const float t = a - mu;
    const float v2 = sigma * sigma;
    const float dlp_dmu = t / v2;
    const float dlp_dsig = (t * t) / (v2 * sigma) - 1.0f / sigma;
    const bool fine = sde_finite(sigma) && sde_finite(lp);
    *dmu = fine ? (ng * dlp_dmu) / Bf : bits_f32(kPolicyNaN);
    *dsig = fine ? ((ng * dlp_dsig - ec / sigma) / Bf) / sigma : bits_f32(kPolicyNaN);
}

RF_HD void ppo_vf_sample(float v, float ret, float vc2, float Bf, float *vl, float *dv)
{
    const float t = ret - v;
    *vl = t * t;
    *dv = (vc2 * (v - ret)) / Bf;
}

RF_HD float ppo_act_prime(float h, int activation)
{
    return activation == kPolicyTanh ? 1.0f - h * h : (h > 0.0f ? 1.0f : 0.0f);
}

// Definition step 6 for one input k: w is row k of the packed matrix (O consecutive outputs)
RF_HD float ppo_back(const float *w, const float *dout, int d_stride, int O, float h, int activation)
{
    float acc = 0.0f;
    for (int o = 0; o < O; ++o)
        acc = acc + w[o] * dout[(size_t)o * (size_t)d_stride];
    return ppo_act_prime(h, activation) * acc;
}

// Where packed parameter p < L.total gets its gradient from: x (offset into the workspace; stride; column k, or k = -1
// for a bias) and delta (offset; stride; column j)
struct PpoSource {
    unsigned x, d;
    int x_stride, d_stride, k, j;
};

RF_HD PpoSource ppo_source(const PolicyLayout &L, const PpoWork &W, unsigned p)
{
    PpoSource s{};
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l <= L.layers[net]; ++l) {
            const int out = l < L.layers[net] ? L.width[net][l] : (net == 0 ? L.n_actions : 1);
            if (p >= L.bias[net][l] + (unsigned)out)
                continue;
            s.d = W.d[net][l], s.d_stride = out;
            s.x = l == 0 ? W.x : W.h[net][l - 1];
            s.x_stride = l == 0 ? L.obs_width : L.width[net][l - 1];
            if (p >= L.bias[net][l]) {
                s.k = -1, s.j = (int)(p - L.bias[net][l]);
            } else {
                const unsigned at = p - L.weight[net][l];
                s.k = (int)(at / (unsigned)out), s.j = (int)(at % (unsigned)out);
            }
            return s;
        }
    // past both nets: log_std_j of the Gaussian head, from the last pi activations and the per-sample sigma terms
    s.k = -2, s.j = (int)(p - L.log_std);
    s.x = W.h[0][L.layers[0] - 1], s.x_stride = (int)L.sde;
    s.d = W.sde, s.d_stride = 1;
    return s;
}

// Definition step 7 for one parameter
RF_HD float ppo_gradient(const float *ws, const PpoSource &s, int B)
{
    const float *d = ws + s.d + s.j;
    float acc = 0.0f;
    if (s.k < 0) {
#if defined(__HIPCC__)
#pragma unroll 8
#endif
        for (int b = 0; b < B; ++b)
            acc = acc + d[(size_t)b * (size_t)s.d_stride];
        return acc;
    }
    const float *x = ws + s.x + s.k;
#if defined(__HIPCC__)
#pragma unroll 8 // (the loads of 8 samples in flight at once; the chain itself stays in batch order)
#endif
    for (int b = 0; b < B; ++b)
        acc = acc + x[(size_t)b * (size_t)s.x_stride] * d[(size_t)b * (size_t)s.d_stride];
    return acc;
}

// "sde policy" step 7': dlog_std_j = the sum over b = 0 .. B-1, from +0, of ((h[b][j] * h[b][j]) * std2_j) * dsig[b]
RF_HD float sde_log_std_gradient(const float *ws, const PpoSource &s, int B, float std2)
{
    const float *h = ws + s.x + s.j, *d = ws + s.d;
    float acc = 0.0f;
#if defined(__HIPCC__)
#pragma unroll 8
#endif
    for (int b = 0; b < B; ++b) {
        const float x = h[(size_t)b * (size_t)s.x_stride];
        acc = acc + ((x * x) * std2) * d[b];
    }
    return acc;
}

RF_HD float ppo_parameter_gradient(const PolicyLayout &L, const PpoWork &W, const float *ws, const float *params, unsigned p,
                                   int B)
{
    const PpoSource s = ppo_source(L, W, p);
    return s.k == -2 ? sde_log_std_gradient(ws, s, B, sde_std2(params[L.log_std + (unsigned)s.j])) : ppo_gradient(ws, s, B);
}

// Definition steps 8 and 9: the constants of one update, then one parameter
struct PpoStep {
    float coef, b1, ob1, b2, ob2, root_bc2, eps, rate;
    PpoHeader next;
};

RF_HD PpoStep ppo_step(const PpoHyper &h, const PpoHeader &now, double norm)
{
    PpoStep s{};
    const double q = h.max_grad_norm / (norm + 1e-6);
    s.coef = (float)(q < 1.0 ? q : 1.0);
    s.b1 = (float)h.beta1, s.ob1 = (float)(1.0 - h.beta1), s.b2 = (float)h.beta2, s.ob2 = (float)(1.0 - h.beta2);
    s.next.step = now.step + 1;
    s.next.bc1 = 1.0 - h.beta1 * (1.0 - now.bc1);
    s.next.bc2 = 1.0 - h.beta2 * (1.0 - now.bc2);
    s.next.zero = 0;
    s.root_bc2 = (float)sqrt(s.next.bc2);
    s.eps = (float)h.adam_eps;
    s.rate = (float)(h.learning_rate / s.next.bc1);
    return s;
}

RF_HD void ppo_adam(const PpoStep &s, float grad, float *p, float *m, float *v)
{
    const float g = grad * s.coef;
    const float mm = s.b1 * *m + s.ob1 * g;
    const float vv = s.b2 * *v + s.ob2 * (g * g);
    const float denom = sqrtf(vv) / s.root_bc2 + s.eps;
    *m = mm;
    *v = vv;
    *p = *p - s.rate * (mm / denom);
}

// Definition step 10; sums: the five treesums over b
RF_HD void ppo_stats(const double sums[5], int B, double norm, const PpoHyper &h, int flags, float out[8])
{
    for (int i = 0; i < 5; ++i)
        out[i] = policy_canonical((float)(sums[i] / (double)B));
    out[5] = policy_canonical((float)norm);
    out[6] = policy_canonical((out[0] + h.ent * (-out[2])) + h.vf * out[1]);
    out[7] = (float)flags;
}

// treesum of y[0 .. size), size a power of two, in place: y[0] + (+0.0)
RF_HD double ppo_treesum_host(double *y, int size)
{
    for (int s = 1; s < size; s <<= 1)
        for (int i = 0; i < size; i += 2 * s)
            y[i] = y[i] + y[i + s];
    return y[0] + 0.0;
}

#if defined(__HIPCC__)
// The same tree by a block, y in LDS (filled and padded with +0.0 by the caller, who need not have synchronised); every
// thread gets the result, and y may be overwritten when it returns.
__device__ __forceinline__ double ppo_treesum_block(double *y, int size, int tid)
{
    __syncthreads();
    for (int s = 1; s < size; s <<= 1) {
        for (int i = tid; i < size / (2 * s); i += kPpoThreads)
            y[2 * s * i] = y[2 * s * i] + y[2 * s * i + s];
        __syncthreads();
    }
    const double sum = y[0] + 0.0;
    __syncthreads();
    return sum;
}

// Back-propagation into one hidden layer of the tile: thread k < K owns unit k; row k of the packed matrix is O
// consecutive floats; dout is [o][tile] in LDS (two broadcast ds_read_b128 per o); h the layer's activations.
__device__ __forceinline__ void ppo_back_tile(const float *__restrict__ params, unsigned weight, int K, int O,
                                              int activation, const float (*dout)[kPolicyTile],
                                              const float (*h)[kPolicyTile], float (*din)[kPolicyTile], int tid)
{
    if (tid < K) {
        const float *__restrict__ w = params + weight + (size_t)tid * (size_t)O;
        float acc[kPolicyTile];
#pragma unroll
        for (int e = 0; e < kPolicyTile; ++e)
            acc[e] = 0.0f;
#pragma unroll 8
        for (int o = 0; o < O; ++o) {
            const float wo = w[o];
            const float4 *x = reinterpret_cast<const float4 *>(&dout[o][0]);
            float ds[kPolicyTile];
#pragma unroll
            for (int v = 0; v < kPolicyTile / 4; ++v) {
                const float4 q = x[v];
                ds[4 * v] = q.x, ds[4 * v + 1] = q.y, ds[4 * v + 2] = q.z, ds[4 * v + 3] = q.w;
            }
#pragma unroll
            for (int e = 0; e < kPolicyTile; ++e)
                acc[e] = acc[e] + wo * ds[e];
        }
#pragma unroll
        for (int e = 0; e < kPolicyTile; ++e)
            din[tid][e] = ppo_act_prime(h[tid][e], activation) * acc[e];
    }
}

// rows [b0, b0 + tile) of a [k][tile] LDS array to the workspace as [b][width]
__device__ __forceinline__ void ppo_store_tile(float *__restrict__ out, const float (*in)[kPolicyTile], int width, int b0,
                                               int B, int tid)
{
    for (int i = tid; i < width * kPolicyTile; i += kPpoThreads) {
        const int e = i / width, k = i - e * width;
        if (b0 + e < B)
            out[(size_t)(b0 + e) * (size_t)width + (size_t)k] = in[k][e];
    }
}

// kSde: the Gaussian head of "sde policy" (L from sde_layout; actions float32 [N]) in place of the Categorical one
// (actions int64 [N])
// kGrouped ("population", all three kernels): a group dimension on the grid (blockIdx.z here, blockIdx.y in the other two).
// A block of group g is a block of the ungrouped kernel over the group's own N rows (rows [g N, (g + 1) N) of every
// array), parameters params + g P, optimizer state + g (kPpoStateHeader + 2 P) floats (`header` is the first group's),
// workspace ws + g W.total (W.total is even: float64 data stays aligned), hyper-parameters hypers[g], index + g B (rows
// local to the group) and stats + 8 g.  No block reads what a block of another group writes.  Ungrouped, hypers is unused
// and the code is what it was without it.  With kSde as well ("population sde") the actions move as float rows and P is
// sde_layout's P + L.
template <bool kSde, bool kGrouped = false>
__global__ __launch_bounds__(kPpoThreads) void ppo_backward_kernel(
    PolicyLayout L, PpoWork W, PpoHyper hy, const float *__restrict__ params, const PpoHeader *__restrict__ header,
    float *__restrict__ ws, int N, const float *__restrict__ obs, const void *__restrict__ actions_any,
    const float *__restrict__ old_log_probs, const float *__restrict__ advantages, const float *__restrict__ returns,
    int B, const int64_t *__restrict__ index, const PpoHyper *__restrict__ hypers /* [G] or null */)
{
    if (kGrouped) { // (block-uniform)
        const size_t g = blockIdx.z, row = g * (size_t)N;
        hy = hypers[g];
        params += g * (size_t)L.total;
        header = reinterpret_cast<const PpoHeader *>(reinterpret_cast<const float *>(header)
                                                     + g * ((size_t)kPpoStateHeader + 2 * (size_t)L.total));
        ws += g * (size_t)W.total;
        obs += row * (size_t)L.obs_width;
        if (kSde)
            actions_any = static_cast<const float *>(actions_any) + row;
        else
            actions_any = static_cast<const int64_t *>(actions_any) + row;
        old_log_probs += row, advantages += row, returns += row;
        index += g * (size_t)B;
    }
    __shared__ __align__(16) float s_act[2][kPolicyMaxWidth][kPolicyTile];   // inputs / activations, [k][sample]
    __shared__ __align__(16) float s_delta[2][kPolicyMaxWidth][kPolicyTile]; // deltas of the hidden layers
    __shared__ __align__(16) float s_head[kPolicyMaxActions][kPolicyTile];   // deltas of the head, [o][sample]
    __shared__ float s_logit[kPolicyTile][kPolicyMaxActions];
    __shared__ float s_work[kPolicyTile][kPolicyMaxActions];
    __shared__ double s_red[kPpoMaxBatch];
    const int64_t *__restrict__ actions = static_cast<const int64_t *>(actions_any); // (!kSde)
    const float *__restrict__ raw_actions = static_cast<const float *>(actions_any); // (kSde)
    const int tid = threadIdx.x;
    const int net = (int)blockIdx.y;
    const int b0 = (int)blockIdx.x * kPolicyTile;
    const int D = L.obs_width;
    double mean = 0.0, var = 0.0;
    const bool normalise = hy.normalize != 0 && B > 1;
    if (net == 0) { // (block-uniform)
        const int size = ppo_pow2(B);
        int bad = 0;
        for (int b = tid; b < size; b += kPpoThreads) {
            double a = 0.0;
            if (b < B) {
                const int64_t raw = index[b];
                const int64_t row = ppo_clamp(raw, N);
                if (kSde) {
                    const float action = raw_actions[row];
                    bad |= raw != row || action != action;
                } else {
                    const int64_t action = actions[row];
                    bad |= raw != row || action < 0 || action >= L.n_actions;
                }
                a = (double)advantages[row];
            }
            s_red[b] = a;
        }
        bad = __syncthreads_or(bad);
        if (blockIdx.x == 0 && tid == 0) {
            *reinterpret_cast<int *>(ws + W.flag) = bad ? 1 : 0;
            *reinterpret_cast<PpoHeader *>(ws + W.header) = *header;
        }
        if (normalise) {
            mean = ppo_treesum_block(s_red, size, tid) / (double)B;
            for (int b = tid; b < size; b += kPpoThreads) {
                double q = 0.0;
                if (b < B) {
                    const double t = (double)advantages[ppo_clamp(index[b], N)] - mean;
                    q = t * t;
                }
                s_red[b] = q;
            }
            var = ppo_treesum_block(s_red, size, tid) / (double)(B - 1);
        }
    }
    // the tile's rows, gathered: element i of the tile is sample i / D, column i % D
    for (int i = tid; i < D * kPolicyTile; i += kPpoThreads) {
        const int e = i / D, k = i - e * D;
        float x = 0.0f;
        if (b0 + e < B) {
            x = obs[(size_t)ppo_clamp(index[b0 + e], N) * (size_t)D + (size_t)k];
            if (net == 0)
                ws[W.x + (size_t)(b0 + e) * (size_t)D + (size_t)k] = x;
        }
        s_act[0][k][e] = x;
    }
    __syncthreads();
    const int layers = L.layers[net];
    int cur = 0, K = D;
    for (int layer = 0; layer < layers; ++layer) { // input in buffer 0, h0 in buffer 1, h1 in buffer 0
        const int H = L.width[net][layer];
        policy_hidden_tile(params, L.weight[net][layer], L.bias[net][layer], K, H, L.activation, s_act[cur], s_act[cur ^ 1],
                           tid);
        __syncthreads();
        cur ^= 1;
        K = H;
        ppo_store_tile(ws + W.h[net][layer], s_act[cur], H, b0, B, tid);
    }
    const int O = net == 0 ? L.n_actions : 1;
    for (int i = tid; i < O * kPolicyTile; i += kPpoThreads) {
        const int e = i / O, o = i - e * O;
        s_logit[e][o] = policy_dot(&s_act[cur][0][e], kPolicyTile, params + L.weight[net][layers] + o, O,
                                   params[L.bias[net][layers] + o], K);
    }
    float *std2 = &s_work[0][0]; // (kSde: the K <= 256 squared standard deviations; s_work is otherwise unused then)
    if (kSde && net == 0 && tid < K)
        std2[tid] = sde_std2(params[L.log_std + tid]);
    __syncthreads();
    if (tid < kPolicyTile) { // one lane per sample: the loss terms and the head deltas
        const int b = b0 + tid;
        if (b < B) {
            const int64_t row = ppo_clamp(index[b], N);
            const float Bf = (float)B;
            if (net == 0) {
                const float adv = advantages[row];
                const float A = normalise ? ppo_normalised(adv, mean, var) : adv;
                float pg, H, kl, clipped;
                if (kSde) {
                    const float sigma = sde_sigma(&s_act[cur][0][tid], kPolicyTile, std2, K);
                    float dmu, dsig;
                    sde_pi_sample(s_logit[tid][0], sigma, raw_actions[row], old_log_probs[row], A, hy.clip, hy.ent, Bf, &dmu,
                                  &dsig, &pg, &H, &kl, &clipped);
                    s_head[0][tid] = dmu;
                    ws[W.sde + b] = dsig;
                } else
                    ppo_pi_sample(&s_logit[tid][0], L.n_actions, (int)ppo_clamp(actions[row], L.n_actions),
                                  old_log_probs[row], A, hy.clip, hy.ent, Bf, &s_work[tid][0], &s_head[0][tid], kPolicyTile,
                                  &pg, &H, &kl, &clipped);
                float *loss = ws + W.loss + b;
                loss[0] = pg, loss[2 * W.max_batch] = H, loss[3 * W.max_batch] = kl, loss[4 * W.max_batch] = clipped;
            } else {
                float vl, dv;
                ppo_vf_sample(s_logit[tid][0], returns[row], hy.vf * 2.0f, Bf, &vl, &dv);
                s_head[0][tid] = dv;
                ws[W.loss + W.max_batch + b] = vl;
            }
        } else {
            for (int o = 0; o < O; ++o) // (the ragged tile back-propagates zeros and stores nothing)
                s_head[o][tid] = 0.0f;
        }
    }
    __syncthreads();
    ppo_store_tile(ws + W.d[net][layers], s_head, O, b0, B, tid);
    // back through the hidden layers: h of layer l is in buffer (l + 1) & 1
    const float (*dout)[kPolicyTile] = s_head;
    int outs = O;
    for (int layer = layers - 1; layer >= 0; --layer) {
        const int H = L.width[net][layer];
        ppo_back_tile(params, L.weight[net][layer + 1], H, outs, L.activation, dout, s_act[(layer + 1) & 1], s_delta[layer],
                      tid);
        __syncthreads();
        ppo_store_tile(ws + W.d[net][layer], s_delta[layer], H, b0, B, tid);
        dout = s_delta[layer];
        outs = H;
    }
}

template <bool kGrouped>
__global__ __launch_bounds__(kPpoThreads) void ppo_gradient_kernel(PolicyLayout L, PpoWork W, float *__restrict__ ws, int B,
                                                                   const float *__restrict__ params)
{
    __shared__ double s_red[kPpoLeaves];
    if (kGrouped) {
        ws += (size_t)blockIdx.y * (size_t)W.total;
        params += (size_t)blockIdx.y * (size_t)L.total;
    }
    const int tid = threadIdx.x;
    const unsigned p = blockIdx.x * (unsigned)kPpoLeaves + (unsigned)tid;
    double square = 0.0;
    if (p < L.total) {
        const float g = ppo_parameter_gradient(L, W, ws, params, p, B);
        ws[W.grad + p] = g;
        square = (double)g * (double)g;
    }
    s_red[tid] = square;
    __syncthreads();
    for (int s = 1; s < kPpoLeaves; s <<= 1) {
        if (tid < kPpoLeaves / (2 * s))
            s_red[2 * s * tid] = s_red[2 * s * tid] + s_red[2 * s * tid + s];
        __syncthreads();
    }
    if (tid == 0)
        reinterpret_cast<double *>(ws + W.partial)[blockIdx.x] = s_red[0];
}

template <bool kGrouped>
__global__ __launch_bounds__(kPpoThreads) void ppo_adam_kernel(unsigned P, PpoWork W, PpoHyper hy, float *__restrict__ params,
                                                               float *__restrict__ state, const float *__restrict__ ws,
                                                               int B, float *__restrict__ stats,
                                                               const PpoHyper *__restrict__ hypers /* [G] or null */)
{
    __shared__ double s_red[kPpoMaxPartials];
    if (kGrouped) {
        const size_t g = blockIdx.y;
        hy = hypers[g];
        params += g * (size_t)P;
        state += g * ((size_t)kPpoStateHeader + 2 * (size_t)P);
        ws += g * (size_t)W.total;
        stats += 8 * g;
    }
    const int tid = threadIdx.x;
    const double *partial = reinterpret_cast<const double *>(ws + W.partial);
    const int size = ppo_pow2((int)W.partials);
    for (int i = tid; i < size; i += kPpoThreads)
        s_red[i] = i < (int)W.partials ? partial[i] : 0.0;
    const double norm = sqrt(ppo_treesum_block(s_red, size, tid));
    const bool invalid = *reinterpret_cast<const int *>(ws + W.flag) != 0;
    const int flags = invalid ? RF_PPO_INVALID : (ppo_finite(norm) ? 0 : RF_PPO_NONFINITE);
    const PpoHeader now = *reinterpret_cast<const PpoHeader *>(ws + W.header);
    const PpoStep step = ppo_step(hy, now, norm);
    const unsigned slices = (P + kPpoAdamSlice - 1) / kPpoAdamSlice;
    if (blockIdx.x < slices) {
        if (flags != 0)
            return;
        float *m = state + kPpoStateHeader, *v = m + P;
        const unsigned first = blockIdx.x * (unsigned)kPpoAdamSlice;
        for (unsigned p = first + (unsigned)tid; p < first + kPpoAdamSlice && p < P; p += kPpoThreads)
            ppo_adam(step, ws[W.grad + p], params + p, m + p, v + p);
        return;
    }
    // the last block: the stats and the next header
    double sums[5];
    const int batch = ppo_pow2(B);
    for (int term = 0; term < 5; ++term) {
        for (int b = tid; b < batch; b += kPpoThreads)
            s_red[b] = b < B ? (double)ws[W.loss + (size_t)term * W.max_batch + b] : 0.0;
        sums[term] = ppo_treesum_block(s_red, batch, tid);
    }
    if (tid == 0) {
        float out[8];
        ppo_stats(sums, B, norm, hy, flags, out);
        for (int i = 0; i < 8; ++i)
            stats[i] = out[i];
        if (flags == 0)
            *reinterpret_cast<PpoHeader *>(state) = step.next;
    }
}
#endif

} // namespace rf
