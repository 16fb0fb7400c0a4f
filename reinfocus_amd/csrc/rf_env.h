// rf_env.h -- device-resident DiscreteSteps-v0, ContinuousJumps and composed step.
//
// The O(N) numpy glue the reference runs on the host every step --
//   DiscreteMoveTransformer.transform      environments/state_transformer.py:248-266
//   (ContinuousJumpTransformer.transform   environments/state_transformer.py:95-118, EnvConfig::task == kEnvTaskJumps)
//   TimeLimitEnder | DivergingEnder        environments/episode_ender.py:137-170, :602-628
//   FastCameras / FastWorlds packing       graphics/camera.py:144-179, graphics/world.py:110-123
//   NormalizedObserver(DeltaObserver(..))  environments/state_observer.py:232-292, :472-517
//   (any tree of the observer classes around one FocusObserver: the interpreter of rf_env_observer_program below)
//   Delta + Observation + OnTarget reward  environments/episode_rewarder.py:130-155, :226-292
//   (Observation + Stopped * OnTarget      environments/episode_rewarder.py:226-292, :361-429, kEnvTaskJumps)
//   same-step auto-reset                   environments/vector_environment.py:137-151
//   (any transformer, ender and rewarder tree of state_transformer.py / episode_ender.py / episode_rewarder.py,
//    EnvConfig::task == kEnvTaskComposed: the interpreter of EnvProgram below)
// -- as two small kernels around the render and focus kernels, so that a step moves only the
// actions and a pool of candidate reset states to the GPU and the observations / rewards /
// flags back.  Arithmetic follows the numpy expressions operation by operation (float32
// arrays with Python-float scalars stay float32, the action set is float64, rewards end up
// float64), so results equal reinfocus_amd/environments/harness.py bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reinfocus_hip.h"
#include "rf_common.h"
#include "rf_env_types.h"
#include "rf_math.h"

namespace rf {

// ndarray.var() of a frame's Laplacian from its exact integer sums -- focus_finalize's expression (rf_focus.h); the
// environment kernels take the variance from the sums themselves, which saves the replayed step a launch per measure
__device__ __forceinline__ double env_variance(const EnvConfig &c, const unsigned long long *sums, int slot)
{
    return variance_from_sums(c.frame_pixels, sums[2 * slot], sums[2 * slot + 1]);
}


// camera.py:144-179 + world.py:110-123 for one environment
__device__ __forceinline__ void pack_scene(const EnvConfig &c, float target, float fp, float *dyn, float *rc)
{
    const float a = (float)(c.half_width * (double)fp);   // f32(hw * fp)
    const float b = (float)(c.half_height * (double)fp);
    const float h2 = (float)((2.0 * c.half_width) * (double)fp);
    const float v2 = (float)((2.0 * c.half_height) * (double)fp);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sum = (a * c.cam_u[k] + b * c.cam_v[k]) + fp * c.cam_w[k]; // numpy.sum, left to right
        dyn[k] = c.look_from[k] - sum;
        dyn[3 + k] = h2 * c.cam_u[k];
        dyn[6 + k] = v2 * c.cam_v[k];
    }
    rc[0] = (float)((double)target * c.tan_half_r);
    rc[1] = -target;
}

// ---- kEnvTaskComposed: a small interpreter of the strategy program (EnvProgram) ------------------------------------
// The reference's strategy classes (state_transformer.py, episode_ender.py, episode_rewarder.py) operation by operation:
// float32 state arithmetic with the Python-scalar parameters rounded to float32 (the program holds them so), float64
// where numpy promotes to it.  Per-leaf state is leaf-major: [leaf][n].

__device__ __forceinline__ const_as<EnvProgram> &env_program(const EnvState &s)
{
    return *as_const(s.program);
}

// st[i] / obs[i] for a program index by selects (a dynamic index would put the small arrays in scratch memory)
__device__ __forceinline__ float pick2(const float st[2], int i)
{
    return i ? st[1] : st[0];
}

__device__ __forceinline__ float pick4(const float v[4], int i)
{
    return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
}

// What an ObservationRewarder reads: the built-in observer's four values in registers, or the environment's row of
// EnvState::obs that an observer program left (W columns; a program index is uniform, so the address is row + scalar)
struct ObsBuiltIn {
    float v[4];
    __device__ __forceinline__ float operator()(int i) const { return pick4(v, i); }
};

struct ObsRow {
    const float *row;
    __device__ __forceinline__ float operator()(int i) const { return row[i]; }
};

__device__ __forceinline__ float clip_limits(const_as<EnvProgram> &p, float v)
{
    return fminf(fmaxf(v, p.limit_lo), p.limit_hi); // numpy.clip(states, *limits) = minimum(maximum(x, lo), hi)
}

// transformer.transform for one environment; `action` is the 4-byte slot (int32 index or float32 action)
__device__ __forceinline__ void composed_transform(const_as<EnvProgram> &p, float st[2], int action)
{
    const int mi = p.move_index;
    float x = pick2(st, mi);
    const float a = __builtin_bit_cast(float, action);
    switch (p.transformer) {
    case RF_TRANSFORM_CONTINUOUS_JUMP: { // (a + 1) / 2.0 * (hi - lo) + lo, taken where farther than the threshold; no clip
        const float m = (a + 1.0f) / 2.0f * p.jump_span + p.limit_lo;
        if (fabsf(x - m) > p.stop_threshold) {
            st[0] = mi ? st[0] : m;
            st[1] = mi ? m : st[1];
        }
        return;
    }
    case RF_TRANSFORM_CONTINUOUS_MOVE: { // clip(a, -1, 1) * speed, added as (|move| > threshold) * move
        const float m = fminf(fmaxf(a, -1.0f), 1.0f) * p.speed;
        x = x + (fabsf(m) > p.stop_threshold ? 1.0f : 0.0f) * m;
        break;
    }
    case RF_TRANSFORM_DISCRETE_JUMP:
        x = p.jump32[action];
        break;
    default: // RF_TRANSFORM_DISCRETE_MOVE: float32 += float64 rounds the float64 sum
        x = (float)((double)x + p.move64[action]);
        break;
    }
    st[0] = clip_limits(p, mi ? st[0] : x);
    st[1] = clip_limits(p, mi ? x : st[1]);
}

// is_truncated of ender leaf i (its state after the step)
__device__ __forceinline__ bool composed_leaf_truncated(const EnvConfig &c, const EnvState &s, const_as<EnvProgram> &p,
                                                        int i, int e)
{
    const size_t at = (size_t)i * c.n + e;
    switch (p.enders[i].kind) {
    case RF_ENDER_ENDLESS:
        return false;
    case RF_ENDER_STOPPED: { // a full history (no NaN) whose span nanmax - nanmin is below early_end_span
        const int rows = p.enders[i].steps + 1, first = p.enders[i].history;
        float lo = s.history[(size_t)first * c.n + e], hi = lo;
        bool full = !isnan(lo);
        for (int k = 1; k < rows; ++k) {
            const float v = s.history[(size_t)(first + k) * c.n + e];
            full = full && !isnan(v);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
        return full && hi - lo < p.enders[i].threshold;
    }
    default: // Diverging, OnTarget, TimeLimit: counter >= steps
        return s.leaf_count[at] >= p.enders[i].steps;
    }
}

// the ender tree's is_truncated: the postfix list over the leaves' flags (a bit stack: | and & of numpy bools)
__device__ __forceinline__ bool composed_truncated(const EnvConfig &c, const EnvState &s, const_as<EnvProgram> &p, int e)
{
    unsigned stack = 0;
    for (int t = 0; t < p.n_ender_ops; ++t) {
        const int op = p.ender_ops[t];
        if (op >= 0) {
            stack = (stack << 1) | (composed_leaf_truncated(c, s, p, op, e) ? 1u : 0u);
        } else {
            const unsigned b = stack & 1u, a = (stack >> 1) & 1u;
            stack = ((stack >> 2) << 1) | (op == RF_OP_OR ? (a | b) : (a & b));
        }
    }
    return stack & 1u;
}

// ender.step for one environment (episode_ender.py: every leaf, whatever the tree's operations)
__device__ __forceinline__ void composed_enders_step(const EnvConfig &c, const EnvState &s, const_as<EnvProgram> &p,
                                                     const float st[2], int e)
{
    for (int i = 0; i < p.n_enders; ++i) {
        const size_t at = (size_t)i * c.n + e;
        const float diff = fabsf(pick2(st, p.enders[i].i0) - pick2(st, p.enders[i].i1));
        switch (p.enders[i].kind) {
        case RF_ENDER_DIVERGING:
            if (diff > s.leaf_float[at] + p.enders[i].threshold)
                s.leaf_count[at] += 1;
            s.leaf_float[at] = diff;
            break;
        case RF_ENDER_ON_TARGET:
            s.leaf_count[at] = diff < p.enders[i].threshold ? s.leaf_count[at] + 1 : 0;
            break;
        case RF_ENDER_TIME_LIMIT:
            s.leaf_count[at] += 1;
            break;
        case RF_ENDER_STOPPED: { // Histories.append_events: shift left by one, newest last
            const int rows = p.enders[i].steps + 1, first = p.enders[i].history;
            for (int k = 0; k + 1 < rows; ++k)
                s.history[(size_t)(first + k) * c.n + e] = s.history[(size_t)(first + k + 1) * c.n + e];
            s.history[(size_t)(first + rows - 1) * c.n + e] = pick2(st, p.enders[i].i0);
            break;
        }
        default: // Endless
            break;
        }
    }
}

// ender.reset for one environment that starts an episode in state st
__device__ __forceinline__ void composed_enders_reset(const EnvConfig &c, const EnvState &s, const_as<EnvProgram> &p,
                                                      const float st[2], int e)
{
    for (int i = 0; i < p.n_enders; ++i) {
        const size_t at = (size_t)i * c.n + e;
        s.leaf_count[at] = 0;
        if (p.enders[i].kind == RF_ENDER_DIVERGING)
            s.leaf_float[at] = fabsf(pick2(st, p.enders[i].i0) - pick2(st, p.enders[i].i1));
        if (p.enders[i].kind == RF_ENDER_STOPPED) { // Histories.reset, then the episode's first state as its first event
            const int rows = p.enders[i].steps + 1, first = p.enders[i].history;
            for (int k = 0; k + 1 < rows; ++k)
                s.history[(size_t)(first + k) * c.n + e] = __builtin_nanf("");
            s.history[(size_t)(first + rows - 1) * c.n + e] = pick2(st, p.enders[i].i0);
        }
    }
}

// rewarder.reset for one environment: Delta / Stopped remember the element's value
__device__ __forceinline__ void composed_rewarders_reset(const EnvConfig &c, const EnvState &s, const_as<EnvProgram> &p,
                                                         const float st[2], int e)
{
    for (int i = 0; i < p.n_rewarders; ++i)
        if (p.rewarders[i].kind == RF_REWARD_DELTA || p.rewarders[i].kind == RF_REWARD_STOPPED)
            s.leaf_old[(size_t)i * c.n + e] = pick2(st, p.rewarders[i].i0);
}

// reward of rewarder leaf i, carried as a double (a float32 term computes in float32: widening it is exact)
template <class Obs>
__device__ __forceinline__ double composed_leaf_reward(const EnvConfig &c, const EnvState &s, const_as<EnvProgram> &p,
                                                       const float st[2], const Obs &obs, int i, int e)
{
    const_as<EnvRewardLeaf> &r = p.rewarders[i];
    const size_t at = (size_t)i * c.n + e;
    switch (r.kind) {
    case RF_REWARD_DELTA: { // abs(x - old) * reward / scale, float32
        const float v = fabsf(pick2(st, r.i0) - s.leaf_old[at]) * r.f[0] / r.f[1];
        s.leaf_old[at] = pick2(st, r.i0);
        return v;
    }
    case RF_REWARD_DISTANCE: // (1 - abs(a - b) / span) * (high - low) + low, float32
        return (1.0f - fabsf(pick2(st, r.i0) - pick2(st, r.i1)) / r.f[0]) * r.f[1] + r.f[2];
    case RF_REWARD_OBSERVATION:
        return obs(r.i0);
    case RF_REWARD_ON_TARGET: // (abs(a - b) < span) * (on - off) + off, float64
        return (fabsf(pick2(st, r.i0) - pick2(st, r.i1)) < r.f[0] ? 1.0 : 0.0) * r.d[0] + r.d[1];
    default: { // RF_REWARD_STOPPED: (abs(x - old) < threshold) * reward, float64
        const double v = (fabsf(pick2(st, r.i0) - s.leaf_old[at]) < r.f[0] ? 1.0 : 0.0) * r.d[0];
        s.leaf_old[at] = pick2(st, r.i0);
        return v;
    }
    }
}

// the rewarder tree: every leaf once, in leaf order, then the postfix list of + / * (each node in its own dtype)
template <class Obs>
__device__ __forceinline__ double composed_reward(const EnvConfig &c, const EnvState &s, const_as<EnvProgram> &p,
                                                  const float st[2], const Obs &obs, int e)
{
    double leaf[kEnvMaxLeaves];
#pragma unroll
    for (int i = 0; i < kEnvMaxLeaves; ++i)
        leaf[i] = i < p.n_rewarders ? composed_leaf_reward(c, s, p, st, obs, i, e) : 0.0;
    double stack[kEnvMaxLeaves];
    int sp = 0;
    for (int t = 0; t < p.n_reward_ops; ++t) {
        const int op = p.reward_ops[t];
        if (op >= 0) {
            stack[sp++] = leaf[op];
            continue;
        }
        const double b = stack[--sp], a = stack[sp - 1];
        double v;
        if (p.reward_f64[t])
            v = op == RF_OP_ADD ? a + b : a * b;
        else
            v = op == RF_OP_ADD ? (double)((float)a + (float)b) : (double)((float)a * (float)b);
        stack[sp - 1] = v;
    }
    return stack[0];
}

// transformer -> ender.step -> scene of every env (vector_environment.py:124-126 + the
// update_targets / update_focus_planes of FocusObserver.observe)
__device__ __forceinline__ void env_pre_one(const EnvConfig &c, const EnvState &s, const int *actions, int e)
{
    float target = s.state[2 * e], focus = s.state[2 * e + 1];
    if (c.task == kEnvTaskComposed) {
        // The reference's enders read the state only, never observations (episode_ender.py), so which environments end
        // is settled here for every composition too: the fused step's ranking before the render still holds.
        const_as<EnvProgram> &p = env_program(s);
        float st[2] = {target, focus};
        if (actions) {
            composed_transform(p, st, actions[e]);
            s.state[2 * e] = st[0];
            s.state[2 * e + 1] = st[1];
            composed_enders_step(c, s, p, st, e);
            s.done[e] = composed_truncated(c, s, p, e) ? 1 : 0;
        } else {
            composed_enders_reset(c, s, p, st, e);
        }
        pack_scene(c, st[0], st[1], s.cam_dyn + 9 * e, s.rect + 2 * e);
        s.sums[2 * e] = 0;
        s.sums[2 * e + 1] = 0;
        return;
    }
    if (actions && c.task == kEnvTaskJumps) {
        // ContinuousJumpTransformer (state_transformer.py:95-118), float32 throughout: a1 = (a + 1) / 2.0,
        // m = a1 * (hi - lo) + lo, the focus plane jumps to m where |focus - m| > stop_threshold; no clip
        const float a = __builtin_bit_cast(float, actions[e]); // (the 4-byte action slot holds a float32 here)
        const float a1 = (a + 1.0f) / 2.0f;
        const float m = a1 * (float)((double)c.limit_hi - (double)c.limit_lo) + c.limit_lo;
        if (fabsf(focus - m) > c.stop_threshold)
            focus = m;
        s.state[2 * e + 1] = focus;
    } else if (actions) { // step: new = clip(f32(f64(old) + move), lo, hi) on BOTH columns
        focus = (float)((double)focus + c.action_set[actions[e]]);
        focus = fminf(fmaxf(focus, c.limit_lo), c.limit_hi);
        target = fminf(fmaxf(target, c.limit_lo), c.limit_hi);
        s.state[2 * e] = target;
        s.state[2 * e + 1] = focus;
    }
    if (actions) {
        // enders (episode_ender.py:137-148, :602-607)
        s.steps[e] += 1;
        const float diff = fabsf(target - focus);
        if (diff > s.last_diff[e] + c.diverge_threshold)
            s.diverging[e] += 1;
        s.last_diff[e] = diff;
        // which environments end is settled here already (env_post_kernel repeats it): the flags depend on the counters
        // alone, not on what the step observes -- the fused step ranks the ended ones BEFORE its render
        bool trunc = s.diverging[e] >= c.early_end_steps;
        if (c.max_steps > 0)
            trunc = (s.steps[e] >= c.max_steps) || trunc;
        s.done[e] = trunc ? 1 : 0;
    } else { // reset of every env
        s.steps[e] = 0;
        s.diverging[e] = 0;
        s.last_diff[e] = fabsf(target - focus);
    }
    pack_scene(c, target, focus, s.cam_dyn + 9 * e, s.rect + 2 * e);
    s.sums[2 * e] = 0; // (the focus measure of the render that follows accumulates into them)
    s.sums[2 * e + 1] = 0;
}

__global__ void env_pre_kernel(EnvConfig c, EnvState s, const int *actions)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < c.n)
        env_pre_one(c, s, actions, e);
}

// +0.0f as a value the compiler cannot see through.  Where a reset writes numpy.zeros deltas and normalises them,
// the subtraction is 0 - mid; with the zero known at compile time the gfx950 backend folds it into a negated operand
// of the division, and numpy's 0 - (+0) = +0 comes out as -0.  Equal as numbers, not as bits -- and the learner
// view's normalise (rf_env_view.h) divides what it is handed, sign of zero included.  A zero in a register keeps the
// subtraction a subtraction.
__device__ __forceinline__ float opaque_zero()
{
    float zero = 0.0f;
    asm volatile("" : "+v"(zero));
    return zero;
}

__device__ __forceinline__ float normalize1(const EnvConfig &c, int k, float v)
{
    return fminf(fmaxf((v - c.mid[k]) / c.scale[k], -1.0f), 1.0f);
}

// ---- rf_env_configure_observed: the interpreter of the observer program (rf_env_observer_program) -------------------
// observer.observe (`first` == 0) or observer.reset (`first` != 0: zero deltas, fresh old values) of one environment in
// state st whose frame measured focus_value: state_observer.py:143-164, :232-292, :403-421, :472-517 operation by
// operation in float32.  The column file is the environment's own row of EnvState::obs, worked on in place -- column
// numbers come from the program, so they are scalars and every access is the row's address plus a scalar offset: no
// array indexed at run time in registers (which would go to scratch memory), no LDS.  The last node leaves the
// observations there.
__device__ __forceinline__ void observe_program(const EnvConfig &c, const EnvState &s, const float st[2],
                                                float focus_value, int first, int e)
{
    const_as<rf_env_observer_program> &p = *as_const(s.observer);
    float *row = s.obs + (size_t)e * p.width;
    for (int k = 0; k < p.n_nodes; ++k) {
        const_as<rf_env_observer_node> &node = p.nodes[k];
        switch (node.kind) {
        case RF_OBS_INDEXED:
            row[node.first] = pick2(st, node.index);
            break;
        case RF_OBS_FOCUS: // hstack(..., dtype=float32) of the float64 focus value
            row[node.first] = focus_value;
            break;
        case RF_OBS_DELTA: { // wrapped - old (numpy.zeros in a reset), then old = wrapped
            float *out = row + (node.include_original ? node.first + node.width : node.first);
            float *old = s.obs_old + (size_t)node.old_first * c.n + e;
            for (int j = 0; j < node.width; ++j) {
                const float wrapped = row[node.first + j];
                out[j] = first ? opaque_zero() : wrapped - old[(size_t)j * c.n];
                old[(size_t)j * c.n] = wrapped;
            }
            break;
        }
        default: // RF_OBS_NORMALIZED: clip((values - mid) / scale, -1, 1)
            for (int j = 0; j < node.width; ++j)
                row[node.first + j] = fminf(fmaxf((row[node.first + j] - node.mid[j]) / node.scale[j], -1.0f), 1.0f);
            break;
        }
    }
}

// env_post_one for a context with an observer program (always kEnvTaskComposed)
__device__ __forceinline__ void env_post_observed(const EnvConfig &c, const EnvState &s, const double *focus_values,
                                                  int first, int e)
{
    const float st[2] = {s.state[2 * e], s.state[2 * e + 1]};
    observe_program(c, s, st, (float)(focus_values ? focus_values[e] : env_variance(c, s.sums, e)), first, e);
    const_as<EnvProgram> &p = env_program(s);
    if (first) {
        composed_rewarders_reset(c, s, p, st, e);
        s.truncated[e] = 0;
        s.done[e] = 0;
        s.reward[e] = 0.0;
        return;
    }
    const ObsRow obs{s.obs + (size_t)e * as_const(s.observer)->width};
    s.reward[e] = composed_reward(c, s, p, st, obs, e);
    const bool trunc = composed_truncated(c, s, p, e);
    s.truncated[e] = trunc ? 1 : 0;
    s.done[e] = trunc ? 1 : 0;
}

// observe -> reward -> done flags (vector_environment.py:128-135); `first` = reset() call
// focus_values == nullptr: the variance comes from the sums the focus kernel left (env_variance)
__device__ __forceinline__ void env_post_step(const EnvConfig &c, const EnvState &s, const double *focus_values, int first,
                                              int e)
{
    if (s.observer) {
        env_post_observed(c, s, focus_values, first, e);
        return;
    }
    const float target = s.state[2 * e], focus = s.state[2 * e + 1];
    const float w0 = focus, w1 = (float)(focus_values ? focus_values[e] : env_variance(c, s.sums, e));
    float d0 = 0.0f, d1 = 0.0f;
    if (!first) {
        d0 = w0 - s.old_wrapped[2 * e];
        d1 = w1 - s.old_wrapped[2 * e + 1];
    }
    s.old_wrapped[2 * e] = w0;
    s.old_wrapped[2 * e + 1] = w1;
    const float o0 = normalize1(c, 0, w0), o1 = normalize1(c, 1, w1), o2 = normalize1(c, 2, d0),
                o3 = normalize1(c, 3, d1);
    s.obs[4 * e] = o0;
    s.obs[4 * e + 1] = o1;
    s.obs[4 * e + 2] = o2;
    s.obs[4 * e + 3] = o3;
    if (c.task == kEnvTaskComposed) {
        const_as<EnvProgram> &p = env_program(s);
        const float st[2] = {target, focus};
        const ObsBuiltIn obs{{o0, o1, o2, o3}};
        if (first) {
            composed_rewarders_reset(c, s, p, st, e);
            s.truncated[e] = 0;
            s.done[e] = 0;
            s.reward[e] = 0.0;
            return;
        }
        s.reward[e] = composed_reward(c, s, p, st, obs, e);
        const bool trunc = composed_truncated(c, s, p, e);
        s.truncated[e] = trunc ? 1 : 0;
        s.done[e] = trunc ? 1 : 0;
        return;
    }
    if (first) {
        s.old_focus[e] = focus;
        s.truncated[e] = 0;
        s.done[e] = 0;
        s.reward[e] = 0.0;
        return;
    }
    const double on_target = (fabsf(target - focus) < c.on_target_span ? 1.0 : 0.0) * 1.0 + 0.0;
    if (c.task == kEnvTaskJumps) {
        // f64(obs[:, 1]) + f64(abs(focus - old) < threshold) * ((abs(target - focus) < span) * 1.0 + 0.0)
        const double stopped = fabsf(focus - s.old_focus[e]) < c.stop_threshold ? 1.0 : 0.0;
        s.old_focus[e] = focus;
        s.reward[e] = (double)o1 + stopped * on_target;
    } else {
        // (abs(focus - old) * -1.0 / scale + obs[:, 1]) + ((abs(target - focus) < span) * 1.0 + 0.0)
        const float moved = fabsf(focus - s.old_focus[e]) * -1.0f / c.reward_scale;
        s.old_focus[e] = focus;
        s.reward[e] = (double)(moved + o1) + on_target;
    }
    bool trunc = s.diverging[e] >= c.early_end_steps;
    if (c.max_steps > 0)
        trunc = (s.steps[e] >= c.max_steps) || trunc;
    s.truncated[e] = trunc ? 1 : 0;
    s.done[e] = trunc ? 1 : 0;
}

// Episode records (rf_env_configure_records) of environment e, once the step's row of observations, s.reward[e] and
// s.done[e] are written and before env_reset_post_one overwrites the row: the accumulators take the step (one float64
// addition, in step order), and every step writes all three record arrays -- the row, the return and the length where
// the episode ended (the accumulators then start over), NaN / NaN / 0 where it did not.  `first` (a reset) only zeroes
// the accumulators and writes the "not ended" records.  The row is copied by a uniform loop of plain loads and stores
// at the row's address (W is the same for every lane): the thread re-reads only what it wrote itself, as
// observe_program does, and no array is indexed at run time in registers.
__device__ __forceinline__ void env_record_one(const EnvState &s, int first, int e)
{
    const int width = s.observer ? as_const(s.observer)->width : 4;
    const bool ended = !first && s.done[e];
    const float *row = s.obs + (size_t)e * width;
    float *out = s.final_obs + (size_t)e * width;
    for (int j = 0; j < width; ++j)
        out[j] = ended ? row[j] : __builtin_nanf("");
    const double total = first ? 0.0 : s.ep_return[e] + s.reward[e];
    const int length = first ? 0 : s.ep_length[e] + 1;
    s.final_return[e] = ended ? total : __builtin_nan("");
    s.final_length[e] = ended ? length : 0;
    s.ep_return[e] = ended ? 0.0 : total;
    s.ep_length[e] = ended ? 0 : length;
}

// env_post_step, then the episode records of a context that keeps them
__device__ __forceinline__ void env_post_one(const EnvConfig &c, const EnvState &s, const double *focus_values, int first, int e)
{
    env_post_step(c, s, focus_values, first, e);
    if (s.ep_return)
        env_record_one(s, first, e);
}

__global__ void env_post_kernel(EnvConfig c, EnvState s, const double *focus_values, int first)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < c.n)
        env_post_one(c, s, focus_values, first, e);
}

// Ranks the done envs in index order (single block, running offset) and applies the
// initializer's r-th candidate state to the r-th done env (vector_environment.py:138-142),
// resets its enders, and packs the compacted scene of the partial render.
// mode kEnvResetBoth does all of it in one launch (rf_env_step); the two-phase step of a sharded
// environment (rf_env_step_begin / rf_env_step_end) ranks first (kEnvResetRank: done_index,
// done_count; no pool yet -- which rows of the initializer's pool a shard takes depends on how
// many environments ended in the shards before it) and applies later (kEnvResetApply).
// kEnvResetPlan (the fused step, before its render): the work of env_pre_kernel first (`actions`), then ranks and packs
// the compacted scene, but leaves the environments' state alone -- the step's observations and rewards still have to be
// taken from what the step left; env_finish_kernel applies the initializer's states afterwards.
// kEnvResetPack: kEnvResetPlan's packing half for a ranking that exists already (rf_env_step_plan / rf_env_step_run).
// `actions` != null in a ranking mode: the transformer / ender work of env_pre_kernel first.
constexpr int kEnvResetBoth = 0, kEnvResetRank = 1, kEnvResetApply = 2, kEnvResetPlan = 3, kEnvResetPack = 4;

__device__ __forceinline__ void env_apply_state(const EnvConfig &c, const EnvState &s, const float *pool, int r, int e)
{
    const float target = pool[2 * r], focus = pool[2 * r + 1];
    s.state[2 * e] = target;
    s.state[2 * e + 1] = focus;
    if (c.task == kEnvTaskComposed) {
        const float st[2] = {target, focus};
        composed_enders_reset(c, s, env_program(s), st, e);
        return;
    }
    s.steps[e] = 0;
    s.diverging[e] = 0;
    s.last_diff[e] = fabsf(target - focus);
}

__device__ __forceinline__ void env_apply_reset(const EnvConfig &c, const EnvState &s, const float *pool, int r, int e)
{
    env_apply_state(c, s, pool, r, e);
    pack_scene(c, pool[2 * r], pool[2 * r + 1], s.cam_dyn2 + 9 * r, s.rect2 + 2 * r);
}

__global__ __launch_bounds__(1024) void env_reset_kernel(EnvConfig c, EnvState s, const float *pool, int mode,
                                                         const int *actions = nullptr)
{
    __shared__ int wave_sum[16];
    __shared__ int running;
    if (mode == kEnvResetApply) {
        const int count = *s.done_count;
        for (int r = (int)threadIdx.x; r < count; r += 1024) {
            env_apply_reset(c, s, pool, r, s.done_index[r]);
            s.sums[2 * r] = 0; // (the auto-reset's focus measure accumulates into slot r)
            s.sums[2 * r + 1] = 0;
        }
        return;
    }
    if (mode == kEnvResetPack) {
        const int count = *s.done_count;
        for (int r = (int)threadIdx.x; r < count; r += 1024) {
            s.done_rank[s.done_index[r]] = r;
            pack_scene(c, pool[2 * r], pool[2 * r + 1], s.cam_dyn2 + 9 * r, s.rect2 + 2 * r);
            s.sums2[2 * r] = 0;
            s.sums2[2 * r + 1] = 0;
        }
        return;
    }
    if (threadIdx.x == 0)
        running = 0;
    __syncthreads();
    for (int base = 0; base < c.n; base += 1024) {
        const int e = base + threadIdx.x;
        if (actions != nullptr && e < c.n)
            env_pre_one(c, s, actions, e); // (sets done[e], read by the same thread below)
        const bool d = e < c.n && s.done[e];
        const unsigned long long ballot = __ballot(d);
        const int lane_rank = __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0));
        if ((threadIdx.x & 63) == 0)
            wave_sum[threadIdx.x >> 6] = __popcll(ballot);
        __syncthreads();
        int before = running, total = 0;
        for (int i = 0; i < 16; ++i) {
            before += (i < (int)(threadIdx.x >> 6)) ? wave_sum[i] : 0;
            total += wave_sum[i];
        }
        if (d) {
            const int r = before + lane_rank;
            s.done_index[r] = e;
            if (mode == kEnvResetBoth)
                env_apply_reset(c, s, pool, r, e);
            if (mode == kEnvResetPlan) {
                s.done_rank[e] = r;
                pack_scene(c, pool[2 * r], pool[2 * r + 1], s.cam_dyn2 + 9 * r, s.rect2 + 2 * r);
                s.sums2[2 * r] = 0;
                s.sums2[2 * r + 1] = 0;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            running += total;
        __syncthreads();
    }
    if (threadIdx.x == 0)
        *s.done_count = running;
    // the auto-reset render is enqueued for all n slots: mark the ones it has to skip
    if (mode == kEnvResetBoth) {
        for (int r = running + (int)threadIdx.x; r < c.n; r += 1024)
            s.rect2[2 * r] = __builtin_bit_cast(float, kSkipEnvBits);
        for (int r = (int)threadIdx.x; r < running; r += 1024) { // (the auto-reset's focus measure accumulates into slot r)
            s.sums[2 * r] = 0;
            s.sums[2 * r + 1] = 0;
        }
    }
}

// Scene of k given states as rows 0..k-1 of the compacted set (cam_dyn2 / rect2): the packing half of
// FocusObserver.observe(new_state, indices) (state_observer.py:377-378) for rows that belong to
// environments of OTHER contexts -- the exact mode of a sharded environment renders compacted row r
// on the context that owns the RNG states of pixel indices [r h w, (r + 1) h w) (render.py:217).
__global__ void env_pack_rows_kernel(EnvConfig c, EnvState s, const float *states, int k)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < k)
        pack_scene(c, states[2 * r], states[2 * r + 1], s.cam_dyn2 + 9 * r, s.rect2 + 2 * r);
}

// observations of the freshly reset envs (DeltaObserver.reset: zero deltas) and the
// rewarder's reset (vector_environment.py:144-148); planned_pool != null: the fused step -- the initializer's states
// are applied only now (kEnvResetPlan), and the re-rendered frames' sums are in sums2
__device__ __forceinline__ void env_reset_post_one(const EnvConfig &c, const EnvState &s, const double *focus_values,
                                                   const float *planned_pool, int r, int e)
{
    if (planned_pool)
        env_apply_state(c, s, planned_pool, r, e);
    if (s.observer) { // observer.reset(new_state, done), rewarder.reset
        const float st[2] = {s.state[2 * e], s.state[2 * e + 1]};
        observe_program(c, s, st,
                        (float)(focus_values ? focus_values[r] : env_variance(c, planned_pool ? s.sums2 : s.sums, r)), 1, e);
        composed_rewarders_reset(c, s, env_program(s), st, e);
        return;
    }
    const float focus = s.state[2 * e + 1];
    const float w0 = focus,
                w1 = (float)(focus_values ? focus_values[r] : env_variance(c, planned_pool ? s.sums2 : s.sums, r));
    s.old_wrapped[2 * e] = w0;
    s.old_wrapped[2 * e + 1] = w1;
    s.obs[4 * e] = normalize1(c, 0, w0);
    s.obs[4 * e + 1] = normalize1(c, 1, w1);
    const float zero = opaque_zero(); // (DeltaObserver.reset: numpy.zeros)
    s.obs[4 * e + 2] = normalize1(c, 2, zero);
    s.obs[4 * e + 3] = normalize1(c, 3, zero);
    if (c.task == kEnvTaskComposed) {
        const float st[2] = {s.state[2 * e], focus};
        composed_rewarders_reset(c, s, env_program(s), st, e);
        return;
    }
    s.old_focus[e] = focus;
}

__global__ void env_reset_post_kernel(EnvConfig c, EnvState s, const double *focus_values, const float *planned_pool)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < *s.done_count)
        env_reset_post_one(c, s, focus_values, planned_pool, r, s.done_index[r]);
}

// the fused step's last kernel: env_post_kernel and env_reset_post_kernel as one launch (both measures are done by then)
__global__ void env_finish_kernel(EnvConfig c, EnvState s, const float *planned_pool)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.n)
        return;
    env_post_one(c, s, nullptr, 0, e);
    if (s.done[e])
        env_reset_post_one(c, s, nullptr, planned_pool, s.done_rank[e], e);
}

} // namespace rf
