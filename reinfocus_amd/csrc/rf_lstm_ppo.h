// rf_lstm_ppo.h -- one recurrent PPO minibatch update in six launches (include/reinfocus_hip.h, "lstm update"):
// sb3-contrib's RecurrentPPO.train() body for the actor-critic of rf_lstm.h -- the sequences of a rotated minibatch, the
// forward through both LSTMs, the loss, back-propagation through the MLPs and through time, clip_grad_norm_, Adam -- in
// the fixed order of the definition, bit for bit equal to the numpy twin (environments/lstm_learner.py lstm_update_numpy).
//
//   lstm_ppo_forward_kernel   grid B x 2: block (b, net) owns the sequence of ONE net that starts at minibatch row b and
//                             returns at once where row b starts none; it finds the sequence's end by scanning
//                             episode_starts and t, so no sequence list and no host knowledge is needed.  Thread j owns
//                             unit j with its four gates (lstm_forward_kernel's organisation, one row at a time: x and h
//                             live in LDS and are read as broadcasts, W^T rows are 64 consecutive floats per wave), c stays
//                             in a register, and the block steps through its rows.  Per row it leaves x, h_prev, c_prev,
//                             the four gate values, c' and h' in the workspace as [b][width].  Both walks load the
//                             weights of eight steps into registers before the first is used (profiles/lstm_update.md).
//   lstm_ppo_mlp_kernel       grid ceil(B / 8) x 2, ppo_backward_kernel's body on tiles of kPolicyTile rows of h': the
//                             validity flag and the advantage moments (pi blocks), policy_hidden_tile / policy_dot,
//                             ppo_pi_sample / ppo_vf_sample, ppo_back_tile, and one more product through the first MLP
//                             matrix, without an activation derivative, which leaves dh_mlp[b][H].
//   lstm_ppo_bptt_kernel      the forward kernel's grid rule; the block walks its sequence backwards.  Thread j owns unit
//                             j: lstm_bptt_unit gives da[b][4H] and dc for the row before; then thread k takes the four
//                             chains of dh_rec[k] over its row of W_hh^T (lstm_bptt_rec).
//   lstm_ppo_gradient_kernel  one thread per packed parameter, ppo_gradient over lstm_ppo_source (ppo_source extended by
//                             the four LSTM pieces of either net); one float64 tree sum of squares per 256 gradients.
//   lstm_ppo_norm_kernel      the recurrent nets have up to 1.27 M parameters, more partial sums than ppo_adam_kernel's
//                             2048: one block per aligned group of 256 partials takes the next eight levels of the SAME
//                             tree, so ppo_adam_kernel finds at most 20 sums of 65 536 leaves each.
//   ppo_adam_kernel           rf_ppo.h's, unchanged: the rest of the tree, the skip rule, clip, Adam, stats and header.
// Why six and not fewer: the MLP tiles need every h' of their rows, the BPTT every dh_mlp of its sequence, the gradient
// every da, and the norm every gradient -- each a dependency between blocks, and there is no grid synchronisation here.
// No atomics, nothing allocated, nothing waited for.  The scalar arithmetic is plain C++ (RF_HD): tests/lstmppocheck
// loops over the same functions on the host.
// "lstm critic" (L.critic == kLstmCriticLinear: a feed-forward critic) keeps the six launches and drops one of the two
// walks and one of the two BPTTs: lstm_ppo_forward_kernel<true> has a grid of B + ceil(B / 8) blocks, the first B walk the
// pi sequences as before and the others each take a tile of kPolicyTile rows of the vf net's linear layer (no sequence
// scan, no state: rows are independent) and leave it as h1[1]; lstm_ppo_mlp_kernel is unchanged, its dh[1] is then the
// delta of the linear layer's output; lstm_ppo_bptt_kernel is launched for the pi net only; lstm_ppo_gradient_kernel<.,
// true> reads lstm_ppo_source_critic, which knows critic.weight^T and critic.bias.  The workspace has no h_prev, c_prev,
// gates, c' or da of the vf net.  The instantiations with the LSTM critic keep the code they had.
#pragma once

#include "rf_lstm.h"
#include "rf_ppo.h"

namespace rf {

#if defined(__HIPCC__)
#define RF_LSTM_UNROLL _Pragma("unroll")
#else
#define RF_LSTM_UNROLL
#endif

constexpr int kLstmPpoGroup = 256; // partials per block of lstm_ppo_norm_kernel: eight more levels of the norm's tree

// The workspace: offsets in floats, each even.  `mlp` is rf_ppo.h's layout of what the MLPs and ppo_adam_kernel use
// (header, flag, loss, h, d, grad, partial; its x is not used: the MLPs' input is h1); rows are [b][width].
struct LstmPpoWork {
    PpoWork mlp;
    unsigned x;                 // [max_batch][D]: the observations of the minibatch's rows
    unsigned h_prev[2], c_prev[2]; // [net][max_batch][H]: the state a row's cell starts from
    unsigned gates[2];          // [net][max_batch][4H]: i, f, g, o after their activations
    unsigned c1[2], h1[2];      // [net][max_batch][H]: c' and h'
    unsigned dh[2];             // [net][max_batch][H]: dh_mlp
    unsigned da[2];             // [net][max_batch][4H]: the deltas of the four gate sums
    unsigned super;             // double [supers]: the norm's tree above the partials
    unsigned supers;
    unsigned total;
};

// (with L.critic == kLstmCriticLinear the vf net has h1 and dh only; its other offsets stay 0 and name nothing)
RF_HD bool lstm_ppo_work(const LstmLayout &L, int max_batch, LstmPpoWork &w)
{
    w = LstmPpoWork{};
    if (max_batch < 1 || max_batch > kPpoMaxBatch)
        return false;
    const PolicyLayout &M = L.mlp;
    const unsigned rows = (unsigned)max_batch, H = (unsigned)L.hidden;
    unsigned at = 0;
    auto take = [&at](unsigned floats) {
        const unsigned here = at;
        at += (floats + 1u) & ~1u;
        return here;
    };
    w.mlp.header = take(kPpoStateHeader);
    w.mlp.flag = take(2);
    w.mlp.loss = take(5 * rows);
    for (int net = 0; net < 2; ++net)
        for (int l = 0; l <= M.layers[net]; ++l) {
            const unsigned width = l < M.layers[net] ? (unsigned)M.width[net][l] : (net == 0 ? (unsigned)M.n_actions : 1u);
            if (l < M.layers[net])
                w.mlp.h[net][l] = take(rows * width);
            w.mlp.d[net][l] = take(rows * width);
        }
    w.mlp.grad = take(L.total);
    w.mlp.partials = (L.total + kPpoLeaves - 1) / kPpoLeaves;
    w.mlp.partial = take(2 * w.mlp.partials);
    w.mlp.max_batch = rows;
    w.supers = (w.mlp.partials + kLstmPpoGroup - 1) / kLstmPpoGroup;
    if (w.supers > (unsigned)kPpoMaxPartials)
        return false;
    w.super = take(2 * w.supers);
    w.x = take(rows * (unsigned)L.obs_width);
    for (int net = 0; net < 2; ++net) {
        const bool cell = net == 0 || L.critic != kLstmCriticLinear;
        if (cell) {
            w.h_prev[net] = take(rows * H);
            w.c_prev[net] = take(rows * H);
            w.gates[net] = take(rows * 4u * H);
            w.c1[net] = take(rows * H);
        }
        w.h1[net] = take(rows * H);
        w.dh[net] = take(rows * H);
        if (cell)
            w.da[net] = take(rows * 4u * H);
    }
    if (M.sde != 0) // (lstm_sde_layout only; taken last, so every other offset is the Categorical layout's)
        w.mlp.sde = take(rows);
    w.total = at;
    w.mlp.total = at;
    return true;
}

// What ppo_adam_kernel reads: the sums lstm_ppo_norm_kernel left in place of the partials
RF_HD PpoWork lstm_ppo_adam_work(const LstmPpoWork &W)
{
    PpoWork a = W.mlp;
    a.partial = W.super;
    a.partials = W.supers;
    return a;
}

// Row b of the minibatch in flat()'s order r = e * T + t: (first + b) mod N, for 0 <= first < N and 0 <= b < N <= 2^30
RF_HD int lstm_ppo_row(int first, int b, int N)
{
    const int r = first + b;
    return r >= N ? r - N : r;
}

// "population lstm": where the n environments of ONE group lie among the `lanes` of the slabs the update reads --
// episode_starts [T + 1][lanes] and lstm_states [T + 1][2][2][lanes][H] keep their single form, so environment e of the
// group is lane lane0 + e and the row and plane stride is lanes, not n.  Ungrouped: {n, 0}.
struct LstmLanes {
    int lanes, lane0;
};

// group g of G groups of m environments each
RF_HD LstmLanes lstm_group_lanes(int G, int m, int g)
{
    return LstmLanes{G * m, g * m};
}

// "population lstm sde": where group g's raw actions begin in the float32 [G N] array of an update, in floats (N the rows
// of ONE group) -- not the int64 elements of the Categorical head
RF_HD size_t lstm_sde_group_actions(size_t g, int N)
{
    return g * (size_t)N;
}

// firsts[g] as the kernels take it: clamped into 0 .. N - 1 (a value outside sets the group's skip flag)
RF_HD int lstm_ppo_first(int raw, int N)
{
    return raw < 0 ? 0 : (raw >= N ? N - 1 : raw);
}

// Row b starts a sequence: b == 0, or t == 0 (the environment changes), or episode_starts[t][e] != 0.  Rows are local to
// the group: they wrap modulo T n, n the group's environments.
RF_HD bool lstm_ppo_is_start(const uint8_t *starts, int T, int n, int first, int b, LstmLanes at)
{
    if (b == 0)
        return true;
    const int r = lstm_ppo_row(first, b, T * n);
    const int e = r / T, t = r - e * T;
    return t == 0 || starts[(size_t)t * (size_t)at.lanes + (size_t)(at.lane0 + e)] != 0;
}

RF_HD bool lstm_ppo_is_start(const uint8_t *starts, int T, int n, int first, int b)
{
    return lstm_ppo_is_start(starts, T, n, first, b, LstmLanes{n, 0});
}

// One past the last row of the sequence that starts at row b
RF_HD int lstm_ppo_end(const uint8_t *starts, int T, int n, int first, int b, int B, LstmLanes at)
{
    int end = b + 1;
    while (end < B && !lstm_ppo_is_start(starts, T, n, first, end, at))
        ++end;
    return end;
}

RF_HD int lstm_ppo_end(const uint8_t *starts, int T, int n, int first, int b, int B)
{
    return lstm_ppo_end(starts, T, n, first, b, B, LstmLanes{n, 0});
}

// Element (t, net, which: 0 h / 1 c, env, unit) of the rollout's lstm_states [T + 1][2][2][n][H]
RF_HD size_t lstm_ppo_state_at(int t, int net, int which, int n, int H, int env, int unit)
{
    return (size_t)t * lstm_state_floats(n, H) + lstm_state_at(net, which, n, H, env, unit);
}

// "population lstm": what rf_lstm_ppo_grouped_state_size and rf_lstm_ppo_grouped_workspace_size return for a ctx (0:
// refused): G times the ungrouped sizes, for minibatches of B out of the m T rows of a group.  sde ("population lstm sde",
// rf_lstm_sde_grouped_state_size / rf_lstm_sde_grouped_workspace_size): the same over lstm_sde_layout
RF_HD unsigned long long lstm_population_state_bytes(const rf_lstm_critic_desc &d, int G, int m, bool sde = false)
{
    LstmLayout L;
    if (!lstm_layout_nets(d.lstm, L, sde, d.critic) || !population_rows(G, m))
        return 0;
    return (unsigned long long)G * (4ull * kPpoStateHeader + 8ull * L.total);
}

RF_HD unsigned long long lstm_population_workspace_bytes(const rf_lstm_critic_desc &d, int G, int m, int T, int B,
                                                         bool sde = false)
{
    LstmLayout L;
    LstmPpoWork W;
    if (!lstm_layout_nets(d.lstm, L, sde, d.critic) || m < 1 || T < 1
        || !population_rows(G, (long long)m * (long long)T) || (long long)B > (long long)m * (long long)T
        || !lstm_ppo_work(L, B, W))
        return 0;
    return (unsigned long long)G * 4ull * W.total;
}

// lstm_cell with the gate values kept: gate[0 .. 3] = i, f, g, o; the same operations, so the same h' and c'
RF_HD void lstm_cell_gates(const float a[4], float c, float gate[4], float *h1, float *c1)
{
    const float i = sigmoid32(a[0]), f = sigmoid32(a[1]), g = tanh32(a[2]), o = sigmoid32(a[3]);
    const float fc = f * c;
    const float ig = i * g;
    const float cn = fc + ig;
    gate[0] = i, gate[1] = f, gate[2] = g, gate[3] = o;
    *c1 = cn;
    *h1 = o * tanh32(cn);
}

// BPTT of one unit and row: dh = dh_mlp + dh_rec; da[0 .. 3] for the gate sums i, f, g, o; returns dc for the row before
RF_HD float lstm_bptt_unit(float dh_mlp, float dh_rec, const float gate[4], float c_prev, float c1, float dc_next,
                           float da[4])
{
    const float i = gate[0], f = gate[1], g = gate[2], o = gate[3];
    const float dh = dh_mlp + dh_rec;
    const float tc = tanh32(c1);
    const float d_o = dh * tc;
    const float dc = (dh * o) * (1.0f - tc * tc) + dc_next;
    da[0] = (dc * g) * (i * (1.0f - i));
    da[1] = (dc * c_prev) * (f * (1.0f - f));
    da[2] = (dc * i) * (1.0f - g * g);
    da[3] = d_o * (o * (1.0f - o));
    return dc * f;
}

// dh_rec[k] for the row before: w is row k of W_hh^T (4H consecutive floats), da the row's deltas [4][H]; four chains over
// j ascending from +0, joined as (i + f) + (g + o)
RF_HD float lstm_bptt_rec(const float *w, const float *da, int H)
{
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int j = 0;
    for (; j + 8 <= H; j += 8) { // (the 32 weights of eight steps are loaded before the first is used; the chains keep their order)
        float wj[8][4];
        RF_LSTM_UNROLL
        for (int u = 0; u < 8; ++u)
            RF_LSTM_UNROLL
            for (int q = 0; q < 4; ++q)
                wj[u][q] = w[q * H + j + u];
        RF_LSTM_UNROLL
        for (int u = 0; u < 8; ++u)
            RF_LSTM_UNROLL
            for (int q = 0; q < 4; ++q)
                acc[q] = acc[q] + wj[u][q] * da[q * H + j + u];
    }
    for (; j < H; ++j)
        for (int q = 0; q < 4; ++q)
            acc[q] = acc[q] + w[q * H + j] * da[q * H + j];
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// ppo_source over the two recurrent nets: where packed parameter p of the cells, MLPs and heads gets its gradient from
RF_HD PpoSource lstm_ppo_source_nets(const LstmLayout &L, const LstmPpoWork &W, unsigned p)
{
    PpoSource s{};
    const PolicyLayout &M = L.mlp;
    const int D = L.obs_width, H = L.hidden;
    const unsigned gates = 4u * (unsigned)H;
    for (int net = 0; net < 2; ++net) {
        if (p < L.b_hh[net] + gates) { // the cell: W_ih^T, W_hh^T, b_ih, b_hh
            s.d = W.da[net], s.d_stride = (int)gates;
            if (p < L.w_hh[net]) {
                const unsigned at = p - L.w_ih[net];
                s.x = W.x, s.x_stride = D, s.k = (int)(at / gates), s.j = (int)(at % gates);
            } else if (p < L.b_ih[net]) {
                const unsigned at = p - L.w_hh[net];
                s.x = W.h_prev[net], s.x_stride = H, s.k = (int)(at / gates), s.j = (int)(at % gates);
            } else {
                s.k = -1, s.j = (int)((p - L.b_ih[net]) % gates);
            }
            return s;
        }
        for (int l = 0; l <= M.layers[net]; ++l) {
            const int out = l < M.layers[net] ? M.width[net][l] : (net == 0 ? M.n_actions : 1);
            if (p >= M.bias[net][l] + (unsigned)out)
                continue;
            s.d = W.mlp.d[net][l], s.d_stride = out;
            s.x = l == 0 ? W.h1[net] : W.mlp.h[net][l - 1];
            s.x_stride = l == 0 ? H : M.width[net][l - 1];
            if (p >= M.bias[net][l]) {
                s.k = -1, s.j = (int)(p - M.bias[net][l]);
            } else {
                const unsigned at = p - M.weight[net][l];
                s.k = (int)(at / (unsigned)out), s.j = (int)(at % (unsigned)out);
            }
            return s;
        }
    }
    return s; // (p past both nets: no caller asks)
}

// "lstm critic" C7: lstm_ppo_source_nets with the two pieces of the vf net's linear layer in place of its cell --
// critic.weight^T [D][H] from the observations and dh[1] (the delta of the layer's output), critic.bias [H] from dh[1]
RF_HD PpoSource lstm_ppo_source_critic(const LstmLayout &L, const LstmPpoWork &W, unsigned p)
{
    const PolicyLayout &M = L.mlp;
    const int D = L.obs_width, H = L.hidden;
    if (p < L.w_ih[1])
        return lstm_ppo_source_nets(L, W, p); // (the pi net, packed first: its cell, MLP and head)
    PpoSource s{};
    if (p < L.b_ih[1] + (unsigned)H) { // the linear layer: critic.weight^T, critic.bias
        s.d = W.dh[1], s.d_stride = H;
        if (p < L.b_ih[1]) {
            const unsigned at = p - L.w_ih[1];
            s.x = W.x, s.x_stride = D, s.k = (int)(at / (unsigned)H), s.j = (int)(at % (unsigned)H);
        } else {
            s.k = -1, s.j = (int)(p - L.b_ih[1]);
        }
        return s;
    }
    for (int l = 0; l <= M.layers[1]; ++l) { // the vf MLP and head, with the layer's output h1[1] as the first input
        const int out = l < M.layers[1] ? M.width[1][l] : 1;
        if (p >= M.bias[1][l] + (unsigned)out)
            continue;
        s.d = W.mlp.d[1][l], s.d_stride = out;
        s.x = l == 0 ? W.h1[1] : W.mlp.h[1][l - 1];
        s.x_stride = l == 0 ? H : M.width[1][l - 1];
        if (p >= M.bias[1][l]) {
            s.k = -1, s.j = (int)(p - M.bias[1][l]);
        } else {
            const unsigned at = p - M.weight[1][l];
            s.k = (int)(at / (unsigned)out), s.j = (int)(at % (unsigned)out);
        }
        return s;
    }
    return s; // (p past both nets: no caller asks)
}

// ... and over everything packed, p < L.total: past both nets (lstm_sde_layout only) log_std_j of the Gaussian head gets
// it from the last pi activations and the per-row sigma terms (k == -2, as ppo_source).  kLinear: the critic mode, a
// compile-time constant for the kernels; lstm_ppo_source below reads it from the layout for the host.
template <bool kLinear> RF_HD PpoSource lstm_ppo_source_of(const LstmLayout &L, const LstmPpoWork &W, unsigned p)
{
    const PolicyLayout &M = L.mlp;
    if (M.sde == 0 || p < M.log_std)
        return kLinear ? lstm_ppo_source_critic(L, W, p) : lstm_ppo_source_nets(L, W, p);
    PpoSource s{};
    s.k = -2, s.j = (int)(p - M.log_std);
    s.x = W.mlp.h[0][M.layers[0] - 1], s.x_stride = (int)M.sde;
    s.d = W.mlp.sde, s.d_stride = 1;
    return s;
}

RF_HD PpoSource lstm_ppo_source(const LstmLayout &L, const LstmPpoWork &W, unsigned p)
{
    return L.critic == kLstmCriticLinear ? lstm_ppo_source_of<true>(L, W, p) : lstm_ppo_source_of<false>(L, W, p);
}

// Definition step U8 for one packed parameter (params: for std2_j of a log_std entry)
template <bool kLinear>
RF_HD float lstm_ppo_parameter_gradient_of(const LstmLayout &L, const LstmPpoWork &W, const float *ws, const float *params,
                                           unsigned p, int B)
{
    const PpoSource s = lstm_ppo_source_of<kLinear>(L, W, p);
    return s.k == -2 ? sde_log_std_gradient(ws, s, B, sde_std2(params[L.mlp.log_std + (unsigned)s.j])) : ppo_gradient(ws, s, B);
}

RF_HD float lstm_ppo_parameter_gradient(const LstmLayout &L, const LstmPpoWork &W, const float *ws, const float *params,
                                        unsigned p, int B)
{
    return L.critic == kLstmCriticLinear ? lstm_ppo_parameter_gradient_of<true>(L, W, ws, params, p, B)
                                         : lstm_ppo_parameter_gradient_of<false>(L, W, ws, params, p, B);
}

#if defined(__HIPCC__)
// acc[q] = acc[q] + in[k] * W^T[k][q * H + j] for k = 0 .. K-1, j = tid: the four gates of unit j for one row; `in` in LDS
__device__ __forceinline__ void lstm_gates_row(const float *__restrict__ params, unsigned weight, int K, int H,
                                               const float *in, float (&acc)[4], int tid)
{
    const float *__restrict__ w = params + weight + tid;
    const size_t row = (size_t)4 * (size_t)H;
    int k = 0;
    for (; k + 8 <= K; k += 8) { // (the 32 weights of eight steps are loaded before the first is used: one round of latency)
        float wk[8][4];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                wk[u][q] = w[(size_t)(k + u) * row + (size_t)q * (size_t)H];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float x = in[k + u];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc[q] = acc[q] + x * wk[u][q];
        }
    }
    for (; k < K; ++k) {
        const float x = in[k];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            acc[q] = acc[q] + x * w[(size_t)k * row + (size_t)q * (size_t)H];
    }
}

// kLinear: "lstm critic" -- the grid is B + ceil(B / kPolicyTile) blocks by 1: block b < B walks the pi sequence that
// starts at row b, block B + i takes rows [8 i, 8 i + 8) of the vf net's linear layer
// kGrouped ("population lstm", all five kernels here and ppo_adam_kernel<true>): a group dimension on the grid (the last
// one the kernel does not use yet).  A block of group g is a block of the ungrouped kernel over the group's own N = n T
// rows (rows [g N, (g + 1) N) of flat()'s arrays; n the environments of ONE group), with the parameters params + g P, the
// optimizer state + g (kPpoStateHeader + 2 P) floats, the workspace ws + g W.total (W.total is even: float64 data stays
// aligned), hyper-parameters hypers[g], stats + 8 g and its own first row firsts[g], read from a device table and clamped
// into 0 .. N - 1 (lstm_ppo_first; lstm_ppo_mlp_kernel flags a value outside).  Rows are local to the group and wrap inside
// it; episode_starts and lstm_states keep their single form over all G n lanes and are reached through LstmLanes, their
// pointers do not move.  No block reads what a block of another group writes.  Ungrouped, firsts / lanes_all (and hypers)
// are unused and the code is what it was without them.
template <bool kLinear = false, bool kGrouped = false>
__global__ __launch_bounds__(kPpoThreads) void lstm_ppo_forward_kernel(
    LstmLayout L, LstmPpoWork W, const float *__restrict__ params, float *__restrict__ ws, int T, int n,
    const float *__restrict__ obs, const uint8_t *__restrict__ starts, const float *__restrict__ states, int first, int B,
    const int *__restrict__ firsts /* [G] or null */, int lanes_all)
{
    LstmLanes at{n, 0};
    if (kGrouped) { // (block-uniform)
        const size_t g = blockIdx.z;
        params += g * (size_t)L.total;
        ws += g * (size_t)W.total;
        obs += g * (size_t)T * (size_t)n * (size_t)L.obs_width;
        first = lstm_ppo_first(firsts[g], T * n);
        at = LstmLanes{lanes_all, (int)blockIdx.z * n};
    }
    if constexpr (kLinear) {
        if ((int)blockIdx.x >= B) { // (block-uniform)
            __shared__ __align__(16) float s_in[kPolicyMaxWidth][kPolicyTile];  // the tile's observations, [k][row]
            __shared__ __align__(16) float s_out[kPolicyMaxWidth][kPolicyTile]; // the layer's outputs, [j][row]
            const int tid = threadIdx.x, D = L.obs_width, H = L.hidden, N = T * n;
            const int b0 = ((int)blockIdx.x - B) * kPolicyTile;
            for (int i = tid; i < D * kPolicyTile; i += kPpoThreads) { // (the ragged tile computes on zeros, stores nothing)
                const int e = i / D, k = i - e * D;
                s_in[k][e] = b0 + e < B ? obs[(size_t)lstm_ppo_row(first, b0 + e, N) * (size_t)D + (size_t)k] : 0.0f;
            }
            __syncthreads();
            lstm_linear_tile(params, L.w_ih[1], L.b_ih[1], D, H, s_in, s_out, tid);
            __syncthreads();
            ppo_store_tile(ws + W.h1[1], s_out, H, b0, B, tid);
            return;
        }
    }
    __shared__ float s_x[kPolicyMaxWidth];
    __shared__ float s_h[kPolicyMaxWidth];
    const int b0 = (int)blockIdx.x, net = (int)blockIdx.y, tid = threadIdx.x;
    if (!lstm_ppo_is_start(starts, T, n, first, b0, at)) // (block-uniform)
        return;
    const int end = lstm_ppo_end(starts, T, n, first, b0, B, at);
    const int D = L.obs_width, H = L.hidden, N = T * n;
    float c = 0.0f;
    {
        const int r = lstm_ppo_row(first, b0, N);
        const int e = r / T, t = r - e * T;
        // an episode start replaces the stored state by +0: a select, so no NaN or inf of a dead state enters
        const bool kept = starts[(size_t)t * (size_t)at.lanes + (size_t)(at.lane0 + e)] == 0;
        if (tid < H) {
            s_h[tid] = kept ? states[lstm_ppo_state_at(t, net, 0, at.lanes, H, at.lane0 + e, tid)] : 0.0f;
            c = kept ? states[lstm_ppo_state_at(t, net, 1, at.lanes, H, at.lane0 + e, tid)] : 0.0f;
        }
    }
    for (int b = b0; b < end; ++b) {
        const int r = lstm_ppo_row(first, b, N);
        if (tid < D) {
            const float x = obs[(size_t)r * (size_t)D + (size_t)tid];
            s_x[tid] = x;
            if (net == 0)
                ws[W.x + (size_t)b * (size_t)D + (size_t)tid] = x;
        }
        __syncthreads();
        float h1 = 0.0f;
        if (tid < H) {
            const size_t at = (size_t)b * (size_t)H + (size_t)tid;
            ws[W.h_prev[net] + at] = s_h[tid];
            ws[W.c_prev[net] + at] = c;
            float acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float bi = params[L.b_ih[net] + (unsigned)(q * H + tid)];
                const float bh = params[L.b_hh[net] + (unsigned)(q * H + tid)];
                acc[q] = bi + bh;
            }
            lstm_gates_row(params, L.w_ih[net], D, H, s_x, acc, tid);
            lstm_gates_row(params, L.w_hh[net], H, H, s_h, acc, tid);
            float gate[4], c1;
            lstm_cell_gates(acc, c, gate, &h1, &c1);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                ws[W.gates[net] + (size_t)b * (size_t)(4 * H) + (size_t)(q * H + tid)] = gate[q];
            ws[W.c1[net] + at] = c1;
            ws[W.h1[net] + at] = h1;
            c = c1;
        }
        __syncthreads(); // (every thread has read h and x of this row)
        if (tid < H)
            s_h[tid] = h1;
    }
}

// The product through the first MLP matrix that leaves dh_mlp: ppo_back_tile without an activation derivative (the LSTM's
// output has none).  Thread k < K owns unit k of h'; row k of the packed matrix is O consecutive floats.
__device__ __forceinline__ void lstm_ppo_back_input_tile(const float *__restrict__ params, unsigned weight, int K, int O,
                                                         const float (*dout)[kPolicyTile], float (*din)[kPolicyTile],
                                                         int tid)
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
            din[tid][e] = acc[e];
    }
}

// kSde: the Gaussian head of "lstm sde update" (L from lstm_sde_layout; actions float32 [N], the raw ones) in place of the
// Categorical one (actions int64 [N]), as ppo_backward_kernel<kSde>
// kGrouped: grid (ceil(B / 8), 2, G); N is the rows of ONE group; `header` is the first group's
template <bool kSde, bool kGrouped = false>
__global__ __launch_bounds__(kPpoThreads) void lstm_ppo_mlp_kernel(
    LstmLayout L, LstmPpoWork W, PpoHyper hy, const float *__restrict__ params, const PpoHeader *__restrict__ header,
    float *__restrict__ ws, int N, const void *__restrict__ actions_any, const float *__restrict__ old_log_probs,
    const float *__restrict__ advantages, const float *__restrict__ returns, int first, int B,
    const PpoHyper *__restrict__ hypers /* [G] or null */, const int *__restrict__ firsts /* [G] or null */)
{
    int outside = 0; // (kGrouped: firsts[g] was not a row of the group -- the update is skipped and flagged)
    if (kGrouped) {  // (block-uniform)
        const size_t g = blockIdx.z, row = g * (size_t)N;
        hy = hypers[g];
        params += g * (size_t)L.total;
        header = reinterpret_cast<const PpoHeader *>(reinterpret_cast<const float *>(header)
                                                     + g * ((size_t)kPpoStateHeader + 2 * (size_t)L.total));
        ws += g * (size_t)W.total;
        if constexpr (kSde) // ("population lstm sde": the raw actions are float32)
            actions_any = static_cast<const float *>(actions_any) + lstm_sde_group_actions(g, N);
        else
            actions_any = static_cast<const int64_t *>(actions_any) + row;
        old_log_probs += row, advantages += row, returns += row;
        const int raw = firsts[g];
        first = lstm_ppo_first(raw, N);
        outside = raw != first;
    }
    const int64_t *__restrict__ actions = static_cast<const int64_t *>(actions_any); // (!kSde)
    const float *__restrict__ raw_actions = static_cast<const float *>(actions_any); // (kSde)
    __shared__ __align__(16) float s_act[2][kPolicyMaxWidth][kPolicyTile];   // h' / activations, [k][sample]
    __shared__ __align__(16) float s_delta[2][kPolicyMaxWidth][kPolicyTile]; // deltas of the hidden layers
    __shared__ __align__(16) float s_head[kPolicyMaxActions][kPolicyTile];   // deltas of the head, [o][sample]
    __shared__ float s_logit[kPolicyTile][kPolicyMaxActions];
    __shared__ float s_work[kPolicyTile][kPolicyMaxActions];
    __shared__ double s_red[kPpoMaxBatch];
    const PolicyLayout &M = L.mlp;
    const int tid = threadIdx.x;
    const int net = (int)blockIdx.y;
    const int b0 = (int)blockIdx.x * kPolicyTile;
    const int H = L.hidden;
    double mean = 0.0, var = 0.0;
    const bool normalise = hy.normalize != 0 && B > 1;
    if (net == 0) { // (block-uniform)
        const int size = ppo_pow2(B);
        int bad = kGrouped ? outside : 0;
        for (int b = tid; b < size; b += kPpoThreads) {
            double a = 0.0;
            if (b < B) {
                const int row = lstm_ppo_row(first, b, N);
                if (kSde) {
                    const float action = raw_actions[row];
                    bad |= action != action;
                } else {
                    const int64_t action = actions[row];
                    bad |= action < 0 || action >= M.n_actions;
                }
                a = (double)advantages[row];
            }
            s_red[b] = a;
        }
        bad = __syncthreads_or(bad);
        if (blockIdx.x == 0 && tid == 0) {
            *reinterpret_cast<int *>(ws + W.mlp.flag) = bad ? 1 : 0;
            *reinterpret_cast<PpoHeader *>(ws + W.mlp.header) = *header;
        }
        if (normalise) {
            mean = ppo_treesum_block(s_red, size, tid) / (double)B;
            for (int b = tid; b < size; b += kPpoThreads) {
                double q = 0.0;
                if (b < B) {
                    const double t = (double)advantages[lstm_ppo_row(first, b, N)] - mean;
                    q = t * t;
                }
                s_red[b] = q;
            }
            var = ppo_treesum_block(s_red, size, tid) / (double)(B - 1);
        }
    }
    // the tile's rows of h' are consecutive in the workspace: element i of the tile is sample i / H, column i % H
    for (int i = tid; i < H * kPolicyTile; i += kPpoThreads) {
        const int e = i / H, k = i - e * H;
        s_act[0][k][e] = b0 + e < B ? ws[W.h1[net] + (size_t)b0 * (size_t)H + (size_t)i] : 0.0f;
    }
    __syncthreads();
    const int layers = M.layers[net];
    int cur = 0, K = H;
    for (int layer = 0; layer < layers; ++layer) { // h' in buffer 0, h0 in buffer 1, h1 in buffer 0
        const int Wd = M.width[net][layer];
        policy_hidden_tile(params, M.weight[net][layer], M.bias[net][layer], K, Wd, M.activation, s_act[cur], s_act[cur ^ 1],
                           tid);
        __syncthreads();
        cur ^= 1;
        K = Wd;
        ppo_store_tile(ws + W.mlp.h[net][layer], s_act[cur], Wd, b0, B, tid);
    }
    const int O = net == 0 ? M.n_actions : 1;
    for (int i = tid; i < O * kPolicyTile; i += kPpoThreads) {
        const int e = i / O, o = i - e * O;
        s_logit[e][o] = policy_dot(&s_act[cur][0][e], kPolicyTile, params + M.weight[net][layers] + o, O,
                                   params[M.bias[net][layers] + o], K);
    }
    float *std2 = &s_work[0][0]; // (kSde: the K <= 256 squared standard deviations; s_work is otherwise unused then)
    if (kSde && net == 0 && tid < K)
        std2[tid] = sde_std2(params[M.log_std + tid]);
    __syncthreads();
    if (tid < kPolicyTile) { // one lane per sample: the loss terms and the head deltas
        const int b = b0 + tid;
        if (b < B) {
            const int row = lstm_ppo_row(first, b, N);
            const float Bf = (float)B;
            if (net == 0) {
                const float adv = advantages[row];
                const float A = normalise ? ppo_normalised(adv, mean, var) : adv;
                float pg, Hb, kl, clipped;
                if (kSde) {
                    const float sigma = sde_sigma(&s_act[cur][0][tid], kPolicyTile, std2, K);
                    float dmu, dsig;
                    sde_pi_sample(s_logit[tid][0], sigma, raw_actions[row], old_log_probs[row], A, hy.clip, hy.ent, Bf, &dmu,
                                  &dsig, &pg, &Hb, &kl, &clipped);
                    s_head[0][tid] = dmu;
                    ws[W.mlp.sde + b] = dsig;
                } else
                    ppo_pi_sample(&s_logit[tid][0], M.n_actions, (int)ppo_clamp(actions[row], M.n_actions),
                                  old_log_probs[row], A, hy.clip, hy.ent, Bf, &s_work[tid][0], &s_head[0][tid], kPolicyTile,
                                  &pg, &Hb, &kl, &clipped);
                float *loss = ws + W.mlp.loss + b;
                loss[0] = pg, loss[2 * W.mlp.max_batch] = Hb, loss[3 * W.mlp.max_batch] = kl;
                loss[4 * W.mlp.max_batch] = clipped;
            } else {
                float vl, dv;
                ppo_vf_sample(s_logit[tid][0], returns[row], hy.vf * 2.0f, Bf, &vl, &dv);
                s_head[0][tid] = dv;
                ws[W.mlp.loss + W.mlp.max_batch + b] = vl;
            }
        } else {
            for (int o = 0; o < O; ++o) // (the ragged tile back-propagates zeros and stores nothing)
                s_head[o][tid] = 0.0f;
        }
    }
    __syncthreads();
    ppo_store_tile(ws + W.mlp.d[net][layers], s_head, O, b0, B, tid);
    // back through the hidden layers: the activations of layer l are in buffer (l + 1) & 1
    const float (*dout)[kPolicyTile] = s_head;
    int outs = O;
    for (int layer = layers - 1; layer >= 0; --layer) {
        const int Wd = M.width[net][layer];
        ppo_back_tile(params, M.weight[net][layer + 1], Wd, outs, M.activation, dout, s_act[(layer + 1) & 1], s_delta[layer],
                      tid);
        __syncthreads();
        ppo_store_tile(ws + W.mlp.d[net][layer], s_delta[layer], Wd, b0, B, tid);
        dout = s_delta[layer];
        outs = Wd;
    }
    // ... and into h': buffer 0 (h', or the second layer's activations) is not read any more
    lstm_ppo_back_input_tile(params, M.weight[net][0], H, outs, dout, s_act[0], tid);
    __syncthreads();
    ppo_store_tile(ws + W.dh[net], s_act[0], H, b0, B, tid);
}

// kGrouped: the forward kernel's grid rule, (B, walks, G)
template <bool kGrouped = false>
__global__ __launch_bounds__(kPpoThreads) void lstm_ppo_bptt_kernel(LstmLayout L, LstmPpoWork W,
                                                                    const float *__restrict__ params,
                                                                    float *__restrict__ ws, int T, int n,
                                                                    const uint8_t *__restrict__ starts, int first, int B,
                                                                    const int *__restrict__ firsts /* [G] or null */,
                                                                    int lanes_all)
{
    LstmLanes at{n, 0};
    if (kGrouped) { // (block-uniform)
        const size_t g = blockIdx.z;
        ws += g * (size_t)W.total;
        first = lstm_ppo_first(firsts[g], T * n);
        at = LstmLanes{lanes_all, (int)blockIdx.z * n};
    }
    // (the group's parameters are reached as params + group_params below: moving `params` itself here took the grouped
    // kernel from 71 to 90 VGPRs and from 7 to 5 waves per SIMD)
    const size_t group_params = kGrouped ? (size_t)blockIdx.z * (size_t)L.total : (size_t)0;
    __shared__ float s_da[4 * kPolicyMaxWidth]; // the row's deltas, [q][j]
    __shared__ float s_dh[kPolicyMaxWidth];     // dh_rec of the row
    const int b0 = (int)blockIdx.x, net = (int)blockIdx.y, tid = threadIdx.x;
    if (!lstm_ppo_is_start(starts, T, n, first, b0, at)) // (block-uniform)
        return;
    const int end = lstm_ppo_end(starts, T, n, first, b0, B, at);
    const int H = L.hidden;
    float dc_next = 0.0f;
    if (tid < H)
        s_dh[tid] = 0.0f;
    for (int b = end - 1; b >= b0; --b) {
        if (tid < H) {
            const size_t at = (size_t)b * (size_t)H + (size_t)tid;
            const float *g = ws + W.gates[net] + (size_t)b * (size_t)(4 * H) + (size_t)tid;
            const float gate[4] = {g[0], g[H], g[2 * H], g[3 * H]};
            float da[4];
            dc_next = lstm_bptt_unit(ws[W.dh[net] + at], s_dh[tid], gate, ws[W.c_prev[net] + at], ws[W.c1[net] + at],
                                     dc_next, da);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s_da[q * H + tid] = da[q];
                ws[W.da[net] + (size_t)b * (size_t)(4 * H) + (size_t)(q * H + tid)] = da[q];
            }
        }
        if (b == b0) // (block-uniform: the entering state is a constant, no gradient flows into it)
            break;
        __syncthreads();
        if (tid < H)
            s_dh[tid] = lstm_bptt_rec(params + group_params + L.w_hh[net] + (size_t)tid * (size_t)(4 * H), s_da, H);
        __syncthreads(); // (the row before overwrites s_da)
    }
}

// kSde: the threads past both nets sum the log_std gradients (sde_log_std_gradient, which needs params for std2_j)
// kLinear: "lstm critic" -- the sources of lstm_ppo_source_critic
// kGrouped: grid (partials, G); params moves with the group, so std2_j is read from the group's own log_std
template <bool kSde, bool kLinear = false, bool kGrouped = false>
__global__ __launch_bounds__(kPpoThreads) void lstm_ppo_gradient_kernel(LstmLayout L, LstmPpoWork W, float *__restrict__ ws,
                                                                        int B, const float *__restrict__ params)
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
        float raw;
        if constexpr (kSde)
            raw = lstm_ppo_parameter_gradient_of<kLinear>(L, W, ws, params, p, B);
        else if constexpr (kLinear)
            raw = ppo_gradient(ws, lstm_ppo_source_critic(L, W, p), B);
        else
            raw = ppo_gradient(ws, lstm_ppo_source_nets(L, W, p), B);
        const float g = policy_canonical(raw);
        ws[W.mlp.grad + p] = g;
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
        reinterpret_cast<double *>(ws + W.mlp.partial)[blockIdx.x] = s_red[0];
}

// Eight more levels of the norm's tree: block g sums partials [256 g, 256 g + 256), those past the end as +0.0
// kGrouped: grid (supers, G)
template <bool kGrouped = false>
__global__ __launch_bounds__(kLstmPpoGroup) void lstm_ppo_norm_kernel(LstmPpoWork W, float *__restrict__ ws)
{
    __shared__ double s_red[kLstmPpoGroup];
    if (kGrouped)
        ws += (size_t)blockIdx.y * (size_t)W.total;
    const int tid = threadIdx.x;
    const unsigned i = blockIdx.x * (unsigned)kLstmPpoGroup + (unsigned)tid;
    s_red[tid] = i < W.mlp.partials ? reinterpret_cast<const double *>(ws + W.mlp.partial)[i] : 0.0;
    __syncthreads();
    for (int s = 1; s < kLstmPpoGroup; s <<= 1) {
        if (tid < kLstmPpoGroup / (2 * s))
            s_red[2 * s * tid] = s_red[2 * s * tid] + s_red[2 * s * tid + s];
        __syncthreads();
    }
    if (tid == 0)
        reinterpret_cast<double *>(ws + W.super)[blockIdx.x] = s_red[0];
}
#endif

} // namespace rf
