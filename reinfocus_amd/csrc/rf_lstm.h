// rf_lstm.h -- the recurrent PPO actor-critic forward with its state and sampling in one launch
// (include/reinfocus_hip.h, "lstm policy"): sb3-contrib's RecurrentActorCriticPolicy with one LSTM layer per net
// (lstm_actor, lstm_critic), then the MLPs and heads of "policy", in the fixed float32 order of the definition
// (rf_policy_math.h holds the scalar functions, shared with the host build of tests/lstmcheck), bit for bit equal to the
// numpy twin (environments/lstm.py lstm_numpy).
//
// The organisation is rf_policy.h's.  A block of kPolicyThreads threads owns ONE net (blockIdx.y: pi or vf) and a tile of
// kPolicyTile consecutive environments.  The cell: thread j owns unit j with its four gates, one accumulator per gate and
// environment of the tile (32, indexed by the constants of unrolled loops: registers), so nothing is exchanged between
// threads before c' and h'; W_ih and W_hh are stored transposed, [k][4H], so the four weight loads of a wave per k are
// runs of 64 consecutive floats; x and h of the tile live in LDS as [k][tile] and are read as broadcasts; h' goes to LDS
// as the MLP's input, and from there on the block runs policy_hidden_tile, policy_dot and policy_head unchanged.  The vf
// block's pass over final_obs runs FIRST: it reads state_in, which the pass over obs may overwrite in place.  No atomics;
// the ragged last tile computes on zeros and stores nothing.
// "lstm critic" (enable_critic_lstm=False) is the kLinear instantiation: its vf block runs ONE linear layer D -> H in
// policy_hidden_tile's organisation without an activation (lstm_linear_tile) in place of the cell -- it loads no h and no
// c and reads neither the state nor the episode starts --, and its pi block stores h' and c' into both halves of the
// state.  The instantiations with the LSTM critic are compiled from the same text with every such branch folded away.
// LstmLayout and lstm_layout are plain C++: tests/lstmcheck packs its host loop by the same offsets.
#pragma once

#include <type_traits>

#include "rf_policy.h"

namespace rf {

// A checked rf_lstm_policy_desc as the kernel reads it: offsets in floats into the parameters.  Per net (pi, then vf):
// W_ih^T [D][4H], W_hh^T [H][4H], b_ih [4H], b_hh [4H], then what "policy" packs for that net with input width H.
// critic == kLstmCriticLinear ("lstm critic"): the vf net has critic.weight^T [D][H] at w_ih[1] and critic.bias [H] at
// b_ih[1] in place of its cell; w_hh[1] and b_hh[1] are b_ih[1] and name nothing.
constexpr int kLstmCriticLstm = RF_LSTM_CRITIC_LSTM, kLstmCriticLinear = RF_LSTM_CRITIC_LINEAR;

struct LstmLayout {
    PolicyLayout mlp; // the two MLPs and their heads (obs_width = lstm_hidden), offsets into the whole array
    int obs_width, hidden;
    unsigned w_ih[2], w_hh[2], b_ih[2], b_hh[2];
    unsigned total;
    int critic; // kLstmCriticLstm or kLstmCriticLinear (no instantiation with the LSTM critic reads it)
};

// The packing of both heads: `sde` packs the MLPs by sde_layout (a pi head of one output, log_std last of everything);
// `critic` is rf_lstm_critic_desc's (any value but the two modes is refused)
RF_HD bool lstm_layout_nets(const rf_lstm_policy_desc &d, LstmLayout &p, bool sde, int critic)
{
    p = LstmLayout{};
    const int D = d.policy.obs_width, H = d.lstm_hidden;
    if (D < 1 || D > kPolicyMaxWidth || H < 1 || H > kPolicyMaxWidth)
        return false;
    if (critic != kLstmCriticLstm && critic != kLstmCriticLinear)
        return false;
    rf_policy_desc mlp = d.policy;
    mlp.obs_width = H;
    if (!(sde ? sde_layout(mlp, p.mlp) : policy_layout(mlp, p.mlp)))
        return false;
    p.obs_width = D;
    p.hidden = H;
    const unsigned gates = 4u * (unsigned)H;
    const unsigned cell = gates * (unsigned)(D + H) + 2u * gates;
    const bool linear = critic == kLstmCriticLinear;
    const unsigned cells = cell + (linear ? (unsigned)(D * H + H) : cell); // (what precedes the vf MLP beyond the pi MLP)
    const unsigned pi_mlp = p.mlp.weight[1][0]; // (policy_layout packs the pi MLP first, from 0)
    for (int net = 0; net < 2; ++net) {
        const unsigned base = net == 0 ? 0u : cell + pi_mlp;
        p.w_ih[net] = base;
        if (net == 1 && linear) {
            p.b_ih[net] = base + (unsigned)(D * H);
            p.w_hh[net] = p.b_hh[net] = p.b_ih[net];
        } else {
            p.w_hh[net] = p.w_ih[net] + (unsigned)D * gates;
            p.b_ih[net] = p.w_hh[net] + (unsigned)H * gates;
            p.b_hh[net] = p.b_ih[net] + gates;
        }
        for (int l = 0; l <= p.mlp.layers[net]; ++l) {
            p.mlp.weight[net][l] += net == 0 ? cell : cells;
            p.mlp.bias[net][l] += net == 0 ? cell : cells;
        }
    }
    p.total = p.mlp.total + cells;
    p.mlp.total = p.total;
    if (sde)
        p.mlp.log_std += cells; // (past both nets of the whole array)
    p.critic = critic;
    return true;
}

// ... with the LSTM critic, as before "lstm critic"
RF_HD bool lstm_layout_nets(const rf_lstm_policy_desc &d, LstmLayout &p, bool sde)
{
    return lstm_layout_nets(d, p, sde, kLstmCriticLstm);
}

// false: desc is outside the limits of the definition
RF_HD bool lstm_layout(const rf_lstm_policy_desc &d, LstmLayout &p)
{
    return lstm_layout_nets(d, p, false);
}

// "lstm sde policy": lstm_layout over sde_layout -- n_actions must be 1, mlp.sde = L = the last pi width, and
// mlp.log_std [L] sits after both nets, so the packed array has P + L floats
RF_HD bool lstm_sde_layout(const rf_lstm_policy_desc &d, LstmLayout &p)
{
    return lstm_layout_nets(d, p, true);
}

// "population lstm sde": where group g's pieces begin, in floats -- its rows of theta [G n][L] (n the environments of ONE
// group), and its log_std inside the parameters [G][P + L]: the last L floats of its own piece
RF_HD size_t lstm_sde_group_theta(const LstmLayout &L, int n, size_t g)
{
    return g * (size_t)n * (size_t)L.mlp.sde;
}

RF_HD size_t lstm_sde_group_log_std(const LstmLayout &L, size_t g)
{
    return g * (size_t)L.total + (size_t)L.mlp.log_std;
}

// floats of the state [2 nets][2: h, c][n][H]
RF_HD size_t lstm_state_floats(int n, int H)
{
    return (size_t)4 * (size_t)n * (size_t)H;
}

// element (net, which: 0 h / 1 c, env, unit) of a state
RF_HD size_t lstm_state_at(int net, int which, int n, int H, int env, int unit)
{
    return ((size_t)(net * 2 + which) * (size_t)n + (size_t)env) * (size_t)H + (size_t)unit;
}

// torch.nn.LSTM's cell from the four gate sums (torch's order i, f, g, o) and the cell state c:
//   i = sigmoid32(a_i), f = sigmoid32(a_f), g = tanh32(a_g), o = sigmoid32(a_o)
//   c' = f * c + i * g (two multiplies, then one add),  h' = o * tanh32(c')
RF_HD void lstm_cell(float ai, float af, float ag, float ao, float c, float *h1, float *c1)
{
    const float i = sigmoid32(ai), f = sigmoid32(af), g = tanh32(ag), o = sigmoid32(ao);
    const float fc = f * c;
    const float ig = i * g;
    const float cn = fc + ig;
    *c1 = cn;
    *h1 = o * tanh32(cn);
}

#if defined(__HIPCC__)
// acc[q][e] = acc[q][e] + in[k][e] * W^T[k][q * H + j] for k = 0 .. K-1, j = tid: the four gates of unit j over the tile
__device__ __forceinline__ void lstm_gates_tile(const float *__restrict__ params, unsigned weight, int K, int H,
                                                const float (*in)[kPolicyTile], float (&acc)[4][kPolicyTile], int tid)
{
    const float *__restrict__ w = params + weight + tid;
    const size_t row = (size_t)4 * (size_t)H;
#pragma unroll 4
    for (int k = 0; k < K; ++k) { // (unrolled: 16 independent weight loads in flight per round of latency)
        float wk[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            wk[q] = w[(size_t)k * row + (size_t)q * (size_t)H];
        const float4 *x = reinterpret_cast<const float4 *>(&in[k][0]);
        float xs[kPolicyTile];
#pragma unroll
        for (int v = 0; v < kPolicyTile / 4; ++v) {
            const float4 t = x[v];
            xs[4 * v] = t.x, xs[4 * v + 1] = t.y, xs[4 * v + 2] = t.z, xs[4 * v + 3] = t.w;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < kPolicyTile; ++e)
                acc[q][e] = acc[q][e] + xs[e] * wk[q];
    }
}

// What only the Gaussian head of lstm_forward_kernel<true> is given: theta float32 [n][L] (null: deterministic) in place of
// gen and sampled, and two more outputs.  The Categorical instantiation takes the empty LstmNoSde in its place, so its
// arguments are what they were.
struct LstmSde {
    const float *theta;
    float *env_actions, *sigma;
};
struct LstmNoSde {
    static constexpr const float *theta = nullptr;
    static constexpr float *env_actions = nullptr, *sigma = nullptr;
};
template <bool kSde> struct LstmSdeOf {
    using type = LstmNoSde;
};
template <> struct LstmSdeOf<true> {
    using type = LstmSde;
};

// "lstm critic" C2 for a block's tile: out[j][e] = bias[j] + sum over k in index order of in[k][e] * W^T[k][j], no
// activation -- policy_hidden_tile's organisation (thread j < H owns unit j, one accumulator per row of the tile; in / out
// are [k][tile] in LDS).  The caller puts a barrier after it.
__device__ __forceinline__ void lstm_linear_tile(const float *__restrict__ params, unsigned weight, unsigned bias, int K,
                                                 int H, const float (*in)[kPolicyTile], float (*out)[kPolicyTile], int tid)
{
    if (tid < H) {
        const float *__restrict__ w = params + weight + tid;
        const float b = params[bias + tid];
        float acc[kPolicyTile];
#pragma unroll
        for (int e = 0; e < kPolicyTile; ++e)
            acc[e] = b;
#pragma unroll 8
        for (int k = 0; k < K; ++k) { // (unrolled: 8 independent weight loads in flight per round of latency)
            const float wk = w[(size_t)k * (size_t)H];
            const float4 *x = reinterpret_cast<const float4 *>(&in[k][0]);
            float xs[kPolicyTile];
#pragma unroll
            for (int v = 0; v < kPolicyTile / 4; ++v) {
                const float4 q = x[v];
                xs[4 * v] = q.x, xs[4 * v + 1] = q.y, xs[4 * v + 2] = q.z, xs[4 * v + 3] = q.w;
            }
#pragma unroll
            for (int e = 0; e < kPolicyTile; ++e)
                acc[e] = acc[e] + xs[e] * wk;
        }
#pragma unroll
        for (int e = 0; e < kPolicyTile; ++e)
            out[tid][e] = acc[e];
    }
}

// kSde: the Gaussian head of "lstm sde policy" (L from lstm_sde_layout) in place of the Categorical one.  actions_any is
// then float32 [n] (the raw actions) and `logits` receives the mean.
// kLinear: "lstm critic" (L.critic == kLstmCriticLinear): the vf block is the linear layer, the pi block stores both halves
// of the state; a launch asks for the vf block only where a value is wanted.
// kGrouped ("population lstm"): grid (ceil(n / kPolicyTile), nets, G) as policy_forward_kernel<true>, n the environments
// of ONE group.  Block (., ., g) is a block of the ungrouped kernel over group g's rows -- rows [g n, (g + 1) n) of obs,
// final_obs, starts and every output -- with the parameters params + g P and the generator gens[g], whose draw number
// consumed + (row - g n) the row takes.  The state keeps its single form [2][2][lanes][H] with lanes = G n: a group's rows
// are NOT one piece of it, each of the four planes contributes rows [g n, (g + 1) n), so the state is reached as
// (plane stride `lanes`, environment lane0 + e) and its pointers do not move.  Ungrouped, lanes is n, lane0 the constant
// 0, gens / consumed / lanes are unused and the code is what it was without them.
// kSde && kGrouped ("population lstm sde"): P is the lstm-sde layout's total, so group g's log_std is the last L floats of
// its own piece; theta, env_actions and sigma move with the rows; gens / consumed stay unused (the noise is theta).
template <bool kSde, bool kLinear = false, bool kGrouped = false>
__global__ __launch_bounds__(kPolicyThreads) void lstm_forward_kernel(
    LstmLayout L, const float *__restrict__ params, int n, const float *__restrict__ obs,
    const uint8_t *__restrict__ starts, const float *__restrict__ final_obs /* or null */, const float *state_in,
    float *state_out /* null, state_in itself, or a range that does not overlap it */, PolicyGen gen, int sampled,
    int first_net, typename std::conditional<kSde, float, int64_t>::type *__restrict__ actions,
    float *__restrict__ log_probs, float *__restrict__ values, float *__restrict__ final_values,
    float *__restrict__ logits, typename LstmSdeOf<kSde>::type sde, const PolicyGen *__restrict__ gens /* [G] or null */,
    uint64_t consumed, int lanes_all)
{
    const float *__restrict__ theta = sde.theta;
    float *__restrict__ env_actions = sde.env_actions, *__restrict__ sigma = sde.sigma;
    if (kGrouped) { // (block-uniform: every row pointer moves to the group's piece; null stays null; the state stays)
        const size_t g = blockIdx.z, row = g * (size_t)n, cell = row * (size_t)L.obs_width;
        params += g * (size_t)L.total;
        obs += cell;
        starts += row;
        final_obs = final_obs != nullptr ? final_obs + cell : nullptr;
        actions = actions != nullptr ? actions + row : nullptr;
        log_probs = log_probs != nullptr ? log_probs + row : nullptr;
        values = values != nullptr ? values + row : nullptr;
        final_values = final_values != nullptr ? final_values + row : nullptr;
        logits = logits != nullptr ? logits + row * (size_t)L.mlp.n_actions : nullptr;
        if constexpr (kSde) { // ("population lstm sde": theta [G n][L] and the head's two outputs; nothing is drawn)
            theta = theta != nullptr ? theta + lstm_sde_group_theta(L, n, g) : nullptr;
            env_actions = env_actions != nullptr ? env_actions + row : nullptr;
            sigma = sigma != nullptr ? sigma + row : nullptr;
        } else if (sampled)
            gen = gens[g];
    }
    const int lanes = kGrouped ? lanes_all : n;                    // the state's plane stride
    const int lane0 = kGrouped ? (int)blockIdx.z * n : 0;          // the state's environment of the group's row 0
    __shared__ __align__(16) float s_x[kPolicyMaxWidth][kPolicyTile];      // the tile's observations, [k][environment]
    __shared__ __align__(16) float s_act[2][kPolicyMaxWidth][kPolicyTile]; // [1]: h; [0]: h', then the MLP's activations
    __shared__ float s_logit[kPolicyTile][kPolicyMaxActions];
    __shared__ float s_sum[kPolicyTile][kPolicyMaxActions];
    const int tid = threadIdx.x;
    const int net = (int)blockIdx.y + first_net;
    const int e0 = (int)blockIdx.x * kPolicyTile;
    const int D = L.obs_width, H = L.hidden;
    for (int turn = 0; turn < 2; ++turn) { // (block-uniform: every thread reaches every barrier)
        const int pass = 1 - turn;         // 1: final_obs from state_in as it is; 0: obs, masked by starts, stores the state
        if (pass == 1 && (net == 0 || final_values == nullptr))
            continue;
        bool heads = pass == 1 || (net == 0 ? actions != nullptr || logits != nullptr : values != nullptr);
        if constexpr (kSde) // (each pi output of the Gaussian head may be asked for by itself)
            heads = heads || (net == 0 && (env_actions != nullptr || log_probs != nullptr || sigma != nullptr));
        if (!heads && (state_out == nullptr || (kLinear && net == 1))) // (the linear critic has no state to advance)
            continue;
        const float *__restrict__ in = pass == 0 ? obs : final_obs;
        // the tile's rows are consecutive in memory: element i of the tile is row i / D, column i % D
        for (int i = tid; i < D * kPolicyTile; i += kPolicyThreads) {
            const int e = i / D, k = i - e * D;
            s_x[k][e] = e0 + e < n ? in[(size_t)e0 * (size_t)D + (size_t)i] : 0.0f;
        }
        if (!(kLinear && net == 1)) // (the linear critic reads neither the state nor the episode starts)
            for (int i = tid; i < H * kPolicyTile; i += kPolicyThreads) {
                const int e = i / H, k = i - e * H, env = e0 + e;
                // an episode start replaces the state by +0: a select, so no NaN or inf of a dead state survives it
                const bool kept = env < n && (pass == 1 || starts[env] == 0);
                s_act[1][k][e] = kept ? state_in[lstm_state_at(net, 0, lanes, H, lane0 + env, k)] : 0.0f;
            }
        __syncthreads();
        if (kLinear && net == 1) {
            lstm_linear_tile(params, L.w_ih[1], L.b_ih[1], D, H, s_x, s_act[0], tid);
        } else if (tid < H) {
            float acc[4][kPolicyTile];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float bi = params[L.b_ih[net] + (unsigned)(q * H + tid)];
                const float bh = params[L.b_hh[net] + (unsigned)(q * H + tid)];
#pragma unroll
                for (int e = 0; e < kPolicyTile; ++e)
                    acc[q][e] = bi + bh;
            }
            lstm_gates_tile(params, L.w_ih[net], D, H, s_x, acc, tid);
            lstm_gates_tile(params, L.w_hh[net], H, H, s_act[1], acc, tid);
#pragma unroll
            for (int e = 0; e < kPolicyTile; ++e) {
                const int env = e0 + e;
                const bool kept = env < n && (pass == 1 || starts[env] == 0);
                const float c = kept ? state_in[lstm_state_at(net, 1, lanes, H, lane0 + env, tid)] : 0.0f;
                float h1, c1;
                lstm_cell(acc[0][e], acc[1][e], acc[2][e], acc[3][e], c, &h1, &c1);
                s_act[0][tid][e] = h1;
                if (pass == 0 && state_out != nullptr && env < n) {
                    state_out[lstm_state_at(net, 0, lanes, H, lane0 + env, tid)] = policy_canonical(h1);
                    state_out[lstm_state_at(net, 1, lanes, H, lane0 + env, tid)] = policy_canonical(c1);
                    if constexpr (kLinear) { // (net == 0: sb3-contrib's lstm_states_vf = lstm_states_pi; nothing reads it)
                        state_out[lstm_state_at(1, 0, lanes, H, lane0 + env, tid)] = policy_canonical(h1);
                        state_out[lstm_state_at(1, 1, lanes, H, lane0 + env, tid)] = policy_canonical(c1);
                    }
                }
            }
        }
        __syncthreads();
        if (!heads)
            continue;
        int cur = 0, K = H;
        for (int layer = 0; layer < L.mlp.layers[net]; ++layer) {
            const int W = L.mlp.width[net][layer];
            policy_hidden_tile(params, L.mlp.weight[net][layer], L.mlp.bias[net][layer], K, W, L.mlp.activation, s_act[cur],
                               s_act[cur ^ 1], tid);
            __syncthreads();
            cur ^= 1;
            K = W;
        }
        const int head = L.mlp.layers[net];
        const int O = net == 0 ? L.mlp.n_actions : 1;
        for (int i = tid; i < O * kPolicyTile; i += kPolicyThreads) {
            const int e = i / O, o = i - e * O;
            const float y = policy_dot(&s_act[cur][0][e], kPolicyTile, params + L.mlp.weight[net][head] + o, O,
                                       params[L.mlp.bias[net][head] + o], K);
            const int env = e0 + e;
            if (net == 0) {
                s_logit[e][o] = y;
                if (logits != nullptr && env < n)
                    logits[(size_t)env * (size_t)O + (size_t)o] = policy_canonical(y);
            } else if (env < n) {
                if (pass == 0)
                    values[env] = policy_canonical(y);
                else {
                    const float lead = in[(size_t)env * (size_t)D];
                    final_values[env] = lead != lead ? bits_f32(kPolicyNaN) : policy_canonical(y);
                }
            }
        }
        if constexpr (kSde) {
            float *std2 = &s_sum[0][0]; // (the K <= 256 squared standard deviations: s_sum is otherwise unused here)
            if (net == 0 && tid < K)
                std2[tid] = sde_std2(params[L.mlp.log_std + tid]);
            __syncthreads();
            if (net == 0 && tid < kPolicyTile && e0 + tid < n) { // one lane per environment: sde_forward_kernel's head
                const int env = e0 + tid;
                const float *h = &s_act[cur][0][tid];
                const float mu = s_logit[tid][0];
                const float s = sde_sigma(h, kPolicyTile, std2, K);
                float a = mu;
                if (theta != nullptr)
                    a = mu + policy_dot(h, kPolicyTile, theta + (size_t)env * (size_t)K, 1, 0.0f, K);
                if (actions != nullptr)
                    actions[env] = policy_canonical(a);
                if (env_actions != nullptr)
                    env_actions[env] = sde_env_action(a);
                if (log_probs != nullptr)
                    log_probs[env] = sde_log_prob(a, mu, s);
                if (sigma != nullptr)
                    sigma[env] = policy_canonical(s);
            }
        } else {
            __syncthreads();
            if (net == 0 && actions != nullptr && tid < kPolicyTile && e0 + tid < n) {
                const int env = e0 + tid;
                const double u = sampled ? policy_draw(gen.word, kGrouped ? consumed + (uint64_t)env : (uint64_t)env) : 0.0;
                int64_t action;
                float log_prob;
                policy_head(&s_logit[tid][0], L.mlp.n_actions, !sampled, u, &s_sum[tid][0], &action, &log_prob);
                actions[env] = action;
                if (log_probs != nullptr)
                    log_probs[env] = log_prob;
            }
        }
        __syncthreads(); // (the next pass overwrites what the heads have read)
    }
}
#endif

} // namespace rf
