// rf_abi_env.hip -- the device-resident environment step (kernels in rf_env.h) and its
// schedules: the fused step (one render launch, one focus launch), the separate launches, the two-phase steps of a
// sharded environment, the hipGraph replay of small configurations.
#include "rf_host.h"

#include <math.h>
#include <string.h>

#include "rf_env.h"
#include "rf_env_init.h"
#include "rf_env_io.h"
#include "rf_env_view.h"
#include "rf_policy.h"
#include "rf_ppo.h"
#include "rf_sde.h"
#include "rf_lstm.h"
#include "rf_lstm_ppo.h"
#include "rf_rollout.h"

using namespace rfh;

namespace {

// The per-step traffic of the device-resident environment as ONE block on either side -- inputs first, then outputs --
// so that a step enqueued in one go moves it with one copy in and one copy out (a hipGraph node each, instead of two
// and four): [pool f32 n x 2 | actions i32 n | pad to 16] [rewards f64 n | observations f32 n x W | count i32 | truncated u8 n]
// (W = 4 columns, or the width of the context's observer program)
struct EnvIo {
    size_t o_pool, o_actions, in_bytes, o_rewards, o_obs, obs_bytes, o_count, o_truncated, bytes;
    EnvIo(size_t n, size_t width)
    {
        o_pool = 0;
        o_actions = n * 8;
        in_bytes = (n * 12 + 15) & ~(size_t)15;
        o_rewards = in_bytes;
        o_obs = o_rewards + n * 8;
        obs_bytes = n * width * 4;
        o_count = o_obs + obs_bytes;
        o_truncated = o_count + 4;
        bytes = (o_truncated + n + 15) & ~(size_t)15;
    }
};

// bytes of the context's observations, float32[n][W]
size_t env_obs_bytes(const rf_ctx *ctx)
{
    return (size_t)ctx->env_host.n * (size_t)ctx->env_obs_width * 4;
}

bool fused_step_possible(const rf_ctx *ctx)
{
    return ctx->env_fused && ctx->env_axis;
}

// ---- the learner view (rf_env_configure_view; kernels in rf_env_view.h) ------------------------------------------------
// Turns the view off and frees its allocation (any rf_env_configure*; the caller has synchronised the stream or does so
// here).
int drop_view(rf_ctx *ctx)
{
    ctx->env_view = false;
    ctx->view_after_step = false;
    if (ctx->view_block) {
        RF_HIP(hipStreamSynchronize(ctx->stream));
        RF_HIP(hipFree(ctx->view_block));
        ctx->view_block = nullptr;
    }
    ctx->view_reward = ctx->view_returns = nullptr;
    ctx->view_stack = ctx->view_final = nullptr;
    ctx->view_moments = nullptr;
    ctx->view_groups = 0;
    ctx->view_grp = rf::EnvViewGroups{};
    ctx->view_gammas.clear();
    return RF_OK;
}

// The view's two kernels, after a step's body or (reset) a reset's, on the ctx's stream and outside any replayed graph:
// env_view_moments_kernel while training -- one block per observation column with norm_obs, one more for the returns in
// a step --, then env_view_apply_kernel.  out_*: the caller's device arrays of rf_env_step_device_view /
// rf_env_reset_device_view, or null.  A grouped view (rf_env_configure_view_grouped) takes the kGrouped instantiations:
// the moments by env_view_moments_packed_kernel where a group fits a wave (P_m <= 64), else one block per (slot, group).
// Either way one moments launch and one apply launch.
int enqueue_view(rf_ctx *ctx, bool reset, float *out_obs, double *out_reward, float *out_final)
{
    const rf::EnvViewConfig &c = ctx->view_cfg;
    const rf::EnvViewGroups &grp = ctx->view_grp;
    const bool grouped = ctx->view_groups > 0;
    const int obs_blocks = c.norm_obs ? c.width : 0, blocks = obs_blocks + (reset ? 0 : 1);
    if (ctx->view_training && blocks > 0) {
        long long p = 1; // the next power of two >= n (grouped: >= m); a thread owns p / 1024 leaves (at least one)
        while (p < (grouped ? grp.m : c.n))
            p <<= 1;
        const int leaves = p > rf::kViewBlock ? (int)(p / rf::kViewBlock) : 1;
        if (!grouped) {
            hipLaunchKernelGGL(rf::env_view_moments_kernel<false>, dim3(blocks), dim3(rf::kViewBlock), 0, ctx->stream, c,
                               obs_blocks, leaves, (const float *)ctx->env.obs, (const double *)ctx->env.reward,
                               ctx->view_returns, ctx->view_moments, grp);
        } else if (p <= rf::kViewPackedMax) {
            const unsigned threads = (unsigned)grp.groups << grp.log2_pm; // <= 65535 * 64
            hipLaunchKernelGGL(rf::env_view_moments_packed_kernel,
                               dim3((threads + rf::kViewPackedBlock - 1) / rf::kViewPackedBlock, blocks),
                               dim3(rf::kViewPackedBlock), 0, ctx->stream, c, obs_blocks, (const float *)ctx->env.obs,
                               (const double *)ctx->env.reward, ctx->view_returns, ctx->view_moments, grp);
        } else {
            hipLaunchKernelGGL(rf::env_view_moments_kernel<true>, dim3(blocks, grp.groups), dim3(rf::kViewBlock), 0,
                               ctx->stream, c, obs_blocks, leaves, (const float *)ctx->env.obs,
                               (const double *)ctx->env.reward, ctx->view_returns, ctx->view_moments, grp);
        }
    }
    const int cells = c.n * c.width;
    const auto apply = grouped ? rf::env_view_apply_kernel<true> : rf::env_view_apply_kernel<false>;
    hipLaunchKernelGGL(apply, dim3((cells + 255) / 256), dim3(256), 0, ctx->stream, c, reset ? 1 : 0,
                       (const float *)ctx->env.obs, (const double *)ctx->env.reward, (const uint8_t *)ctx->env.truncated,
                       (const float *)(ctx->view_final ? ctx->env.final_obs : nullptr),
                       (const rf::EnvViewMoments *)ctx->view_moments, ctx->view_stack, ctx->view_returns, ctx->view_reward,
                       ctx->view_final, out_obs, out_reward, out_final, grp);
    RF_HIP(hipGetLastError());
    ctx->view_after_step = !reset;
    return RF_OK;
}

// The two-phase and planned forms leave a step half done between calls; the view follows whole steps only.
#define RF_REFUSE_VIEW(ctx, fn)                                                                                    \
    RF_REQUIRE(!((ctx)->env_ready && (ctx)->env_view),                                                             \
               "%s: the context has a learner view (rf_env_configure_view): only whole steps", fn)

// The actions of one step, checked on the host before anything is enqueued (a refused step changes no state).  The
// int32 form (DiscreteSteps-v0, the composed discrete transformers) takes indices into the action set; the float32 form
// (ContinuousJumps, the composed continuous transformers) takes finite values, in [-1, 1] for a jump -- NaN, infinities
// and jumps outside are refused, where the reference's ContinuousJumpTransformer would carry them into the focus plane
// (a ContinuousMoveTransformer clips finite values, as the reference does).  Calling the form of the other dtype is an
// error: the 4-byte slots are never reinterpreted.
bool composed_discrete(const rf_ctx *ctx)
{
    return ctx->env_program.transformer == RF_TRANSFORM_DISCRETE_JUMP ||
           ctx->env_program.transformer == RF_TRANSFORM_DISCRETE_MOVE;
}

int check_actions(const rf_ctx *ctx, const int32_t *actions, const char *fn)
{
    const int task = ctx->env_cfg.task;
    RF_REQUIRE(task == rf::kEnvTaskSteps || (task == rf::kEnvTaskComposed && composed_discrete(ctx)),
               "%s: the context takes float32 actions (%s_jumps)", fn, fn);
    const int n_actions = task == rf::kEnvTaskComposed ? ctx->env_program.n_actions : ctx->env_host.n_actions;
    for (int i = 0; i < ctx->env_host.n; ++i)
        RF_REQUIRE(actions[i] >= 0 && actions[i] < n_actions, "%s: action %d of env %d out of range", fn, actions[i], i);
    return RF_OK;
}

int check_actions(const rf_ctx *ctx, const float *actions, const char *fn)
{
    const int task = ctx->env_cfg.task;
    RF_REQUIRE(task == rf::kEnvTaskJumps || (task == rf::kEnvTaskComposed && !composed_discrete(ctx)),
               "%s: the context takes int32 actions", fn);
    const bool jump = task == rf::kEnvTaskJumps || ctx->env_program.transformer == RF_TRANSFORM_CONTINUOUS_JUMP;
    for (int i = 0; i < ctx->env_host.n; ++i) {
        if (jump)
            RF_REQUIRE(actions[i] >= -1.0f && actions[i] <= 1.0f, "%s: action %g of env %d outside [-1, 1]", fn,
                       (double)actions[i], i); // (false for NaN)
        else
            RF_REQUIRE(isfinite(actions[i]), "%s: action %g of env %d is not finite", fn, (double)actions[i], i);
    }
    return RF_OK;
}

// A postfix list over n_leaves leaves: every leaf exactly once, two operands for every operation, one value left.
bool postfix_ok(const int *ops, int n_ops, int n_leaves)
{
    if (n_leaves < 1 || n_leaves > RF_ENV_MAX_LEAVES || n_ops != 2 * n_leaves - 1)
        return false;
    unsigned seen = 0;
    int depth = 0;
    for (int t = 0; t < n_ops; ++t) {
        const int op = ops[t];
        if (op >= 0) {
            if (op >= n_leaves || (seen >> op) & 1u)
                return false;
            seen |= 1u << op;
            ++depth;
        } else {
            if ((op != -1 && op != -2) || depth < 2)
                return false;
            --depth;
        }
    }
    return depth == 1;
}

bool finite_all(const double *v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!isfinite(v[i]))
            return false;
    return true;
}

int check_program(const rf_env_program *p, int obs_width)
{
    auto state_index = [](int i) { return i == 0 || i == 1; };
    const int t = p->transformer;
    RF_REQUIRE(t >= RF_TRANSFORM_CONTINUOUS_JUMP && t <= RF_TRANSFORM_DISCRETE_MOVE,
               "rf_env_configure_composed: unknown transformer %d", t);
    RF_REQUIRE(state_index(p->move_index), "rf_env_configure_composed: move_index %d outside {0, 1}", p->move_index);
    const double params[4] = {p->limit_lo, p->limit_hi, p->speed, p->stop_threshold};
    RF_REQUIRE(finite_all(params, 4), "rf_env_configure_composed: a transformer parameter is not finite");
    if (t == RF_TRANSFORM_DISCRETE_JUMP || t == RF_TRANSFORM_DISCRETE_MOVE) {
        RF_REQUIRE(p->n_actions >= 1 && p->n_actions <= 32, "rf_env_configure_composed: n_actions %d outside [1, 32]",
                   p->n_actions);
        RF_REQUIRE(finite_all(p->action_set, p->n_actions), "rf_env_configure_composed: an action is not finite");
    }
    RF_REQUIRE(p->n_enders >= 1 && p->n_enders <= RF_ENV_MAX_LEAVES && p->n_rewarders >= 1 &&
                   p->n_rewarders <= RF_ENV_MAX_LEAVES,
               "rf_env_configure_composed: %d enders, %d rewarders (1 to %d each)", p->n_enders, p->n_rewarders,
               RF_ENV_MAX_LEAVES);
    RF_REQUIRE(postfix_ok(p->ender_ops, p->n_ender_ops, p->n_enders),
               "rf_env_configure_composed: the enders' postfix list is malformed");
    RF_REQUIRE(postfix_ok(p->reward_ops, p->n_reward_ops, p->n_rewarders),
               "rf_env_configure_composed: the rewarders' postfix list is malformed");
    for (int i = 0; i < p->n_enders; ++i) {
        const rf_env_ender &l = p->enders[i];
        RF_REQUIRE(l.kind >= RF_ENDER_DIVERGING && l.kind <= RF_ENDER_TIME_LIMIT,
                   "rf_env_configure_composed: ender %d: unknown kind %d", i, l.kind);
        RF_REQUIRE(state_index(l.index0) && state_index(l.index1),
                   "rf_env_configure_composed: ender %d: index outside {0, 1}", i);
        RF_REQUIRE(isfinite(l.threshold), "rf_env_configure_composed: ender %d: parameter not finite", i);
        RF_REQUIRE(l.kind != RF_ENDER_STOPPED || (l.steps >= 0 && l.steps <= RF_ENV_MAX_STOPPED_STEPS),
                   "rf_env_configure_composed: ender %d: StoppedEnder steps %d outside [0, %d]", i, l.steps,
                   RF_ENV_MAX_STOPPED_STEPS);
    }
    // every node's dtype: float64 for OnTarget / Stopped, float32 for the others, numpy's promotion for an operation
    unsigned stack = 0;
    for (int k = 0; k < p->n_reward_ops; ++k) {
        const int op = p->reward_ops[k];
        unsigned f64;
        if (op >= 0) {
            const int kind = p->rewarders[op].kind;
            f64 = (kind == RF_REWARD_ON_TARGET || kind == RF_REWARD_STOPPED) ? 1u : 0u;
            stack = (stack << 1) | f64;
        } else {
            f64 = (stack | (stack >> 1)) & 1u;
            stack = ((stack >> 2) << 1) | f64;
        }
        RF_REQUIRE(p->reward_f64[k] == (int)f64, "rf_env_configure_composed: reward_f64[%d] is not numpy's promotion", k);
    }
    for (int i = 0; i < p->n_rewarders; ++i) {
        const rf_env_rewarder &l = p->rewarders[i];
        RF_REQUIRE(l.kind >= RF_REWARD_DELTA && l.kind <= RF_REWARD_STOPPED,
                   "rf_env_configure_composed: rewarder %d: unknown kind %d", i, l.kind);
        if (l.kind == RF_REWARD_OBSERVATION)
            RF_REQUIRE(l.index0 >= 0 && l.index0 < obs_width, "rf_env_configure_composed: rewarder %d: observation index %d "
                       "outside 0-%d", i, l.index0, obs_width - 1);
        else
            RF_REQUIRE(state_index(l.index0) && state_index(l.index1),
                       "rf_env_configure_composed: rewarder %d: index outside {0, 1}", i);
        RF_REQUIRE(finite_all(l.p, 3), "rf_env_configure_composed: rewarder %d: parameter not finite", i);
    }
    return RF_OK;
}

// An observer program as rf_env_configure_observed takes it (include/reinfocus_hip.h): the nodes work on a stack of
// columns that never shrinks, so every column a node touches is below the final width.
int check_observer_program(const rf_env_observer_program *p)
{
    const char *fn = "rf_env_configure_observed";
    RF_REQUIRE(p->n_nodes >= 1 && p->n_nodes <= RF_ENV_MAX_OBS_NODES, "%s: %d observer nodes (1 to %d)", fn, p->n_nodes,
               RF_ENV_MAX_OBS_NODES);
    int top = 0, old = 0, focus = 0;
    for (int k = 0; k < p->n_nodes; ++k) {
        const rf_env_observer_node &node = p->nodes[k];
        switch (node.kind) {
        case RF_OBS_INDEXED:
        case RF_OBS_FOCUS:
            RF_REQUIRE(node.first == top && node.width == 1, "%s: node %d: a leaf writes the next free column", fn, k);
            RF_REQUIRE(node.kind == RF_OBS_FOCUS || node.index == 0 || node.index == 1,
                       "%s: node %d: element index %d outside {0, 1}", fn, k, node.index);
            focus += node.kind == RF_OBS_FOCUS ? 1 : 0;
            top += 1;
            break;
        case RF_OBS_DELTA:
        case RF_OBS_NORMALIZED:
            RF_REQUIRE(node.width >= 1 && node.first >= 0 && node.first + node.width == top,
                       "%s: node %d: columns [%d, %d) are not the top of the %d columns there", fn, k, node.first,
                       node.first + node.width, top);
            if (node.kind == RF_OBS_DELTA) {
                RF_REQUIRE(node.old_first == old, "%s: node %d: old-value rows are handed out in node order", fn, k);
                old += node.width;
                top += node.include_original ? node.width : 0;
            } else {
                for (int j = 0; j < node.width; ++j)
                    RF_REQUIRE(isfinite(node.mid[j]) && isfinite(node.scale[j]) && node.scale[j] != 0.0f,
                               "%s: node %d: column %d: mid %g / scale %g (finite, scale not zero)", fn, k, j,
                               (double)node.mid[j], (double)node.scale[j]);
            }
            break;
        default:
            RF_REQUIRE(false, "%s: node %d: unknown kind %d", fn, k, node.kind);
        }
        RF_REQUIRE(top <= RF_ENV_MAX_OBS_COLUMNS && old <= RF_ENV_MAX_OBS_COLUMNS,
                   "%s: node %d: %d columns, %d old-value rows (at most %d each)", fn, k, top, old, RF_ENV_MAX_OBS_COLUMNS);
    }
    RF_REQUIRE(p->nodes[p->n_nodes - 1].first == 0, "%s: the last node does not leave one observer's columns", fn);
    RF_REQUIRE(focus == 1, "%s: %d FocusObserver nodes (exactly one: a step renders once)", fn, focus);
    RF_REQUIRE(p->width == top && p->n_old == old, "%s: width %d / n_old %d, but the nodes leave %d / %d", fn, p->width,
               p->n_old, top, old);
    return RF_OK;
}

// the kernels' form of a checked program (rf::EnvProgram): parameters rounded to what numpy computes them in
rf::EnvProgram device_program(const rf_env_program &h)
{
    rf::EnvProgram d{};
    d.transformer = h.transformer;
    d.move_index = h.move_index;
    d.n_actions = h.n_actions;
    d.limit_lo = (float)h.limit_lo;
    d.limit_hi = (float)h.limit_hi;
    d.jump_span = (float)(h.limit_hi - h.limit_lo);
    d.speed = (float)h.speed;
    d.stop_threshold = (float)h.stop_threshold;
    for (int i = 0; i < 32; ++i) {
        d.move64[i] = h.action_set[i];
        d.jump32[i] = (float)h.action_set[i];
    }
    d.n_enders = h.n_enders;
    d.n_ender_ops = h.n_ender_ops;
    d.n_rewarders = h.n_rewarders;
    d.n_reward_ops = h.n_reward_ops;
    int rows = 0;
    for (int i = 0; i < h.n_enders; ++i) {
        const rf_env_ender &l = h.enders[i];
        d.enders[i] = rf::EnvEnderLeaf{l.kind, l.index0, l.index1, l.steps, (float)l.threshold, rows};
        if (l.kind == RF_ENDER_STOPPED)
            rows += l.steps + 1;
    }
    d.history_rows = rows;
    for (int i = 0; i < h.n_rewarders; ++i) {
        const rf_env_rewarder &l = h.rewarders[i];
        rf::EnvRewardLeaf &r = d.rewarders[i];
        r.kind = l.kind;
        r.i0 = l.index0;
        r.i1 = l.index1;
        for (int k = 0; k < 3; ++k)
            r.f[k] = (float)l.p[k];
        r.d[0] = l.p[1]; // OnTarget: on - off | Stopped: reward
        r.d[1] = l.p[2]; // OnTarget: off
    }
    for (int k = 0; k < RF_ENV_MAX_OPS; ++k) {
        d.ender_ops[k] = h.ender_ops[k];
        d.reward_ops[k] = h.reward_ops[k];
        d.reward_f64[k] = h.reward_f64[k];
    }
    return d;
}

int env_configure(rf_ctx *ctx, const rf_env_config *cfg, int task, float stop_threshold,
                  const rf_env_program *program = nullptr, const rf_env_observer_program *observer = nullptr)
{
    RF_REQUIRE(cfg->frame_height > 0 && cfg->spp > 0, "rf_env_configure: frame_height, spp must be positive");
    RF_REQUIRE(cfg->gray_mode == RF_GRAY_15BIT || cfg->gray_mode == RF_GRAY_14BIT, "rf_env_configure: gray_mode");
    const uint64_t need = (uint64_t)cfg->n * cfg->frame_height * cfg->frame_height;
    RF_REQUIRE(need <= ctx->n_states, "rf_env_configure: %llu pixels but only %llu RNG states (rf_seed first)",
               (unsigned long long)need, (unsigned long long)ctx->n_states);
    drop_env_graph(ctx);
    if (int rc = resolve_device_steps(ctx)) // (the pixels of the configuration that ends here)
        return rc;
    ctx->env_fault_step = ctx->env_fault_env = -1;
    ctx->env_step_index = 0;
    RF_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->env_block) {
        RF_HIP(hipFree(ctx->env_block));
        ctx->env_block = nullptr;
    }
    drop_env_snapshots(ctx); // (they belong to the configuration that ends here)
    if (int rc = drop_view(ctx))
        return rc;
    ctx->env_ready = false;
    ctx->env_started = false;
    ctx->env_init = false; // (rf_env_configure_initializer comes after the environment's configuration)
    const size_t n = (size_t)cfg->n;
    // carve one allocation (256-B aligned pieces)
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_state = take(n * 8), o_steps = take(n * 4), o_div = take(n * 4), o_last = take(n * 4),
                 o_oldw = take(n * 8), o_oldf = take(n * 4), o_cam = take(n * 36), o_rect = take(n * 8),
                 o_cam2 = take(n * 36), o_rect2 = take(n * 8), o_didx = take(n * 4), o_done = take(n), o_sums2 = take(n * 16),
                 o_drank = take(n * 4);
    // kEnvTaskComposed: the program, then the per-leaf strategy state ([leaf][n] each)
    const rf::EnvProgram prog = program ? device_program(*program) : rf::EnvProgram{};
    const size_t n_enders = program ? (size_t)program->n_enders : 0, n_rewarders = program ? (size_t)program->n_rewarders : 0;
    const size_t o_prog = take(program ? sizeof(rf::EnvProgram) : 0), o_count = take(n_enders * n * 4),
                 o_float = take(n_enders * n * 4), o_hist = take((size_t)prog.history_rows * n * 4),
                 o_old = take(n_rewarders * n * 4);
    // rf_env_configure_observed: the observer program, then the DELTA nodes' old values ([row][n])
    const size_t n_old = observer ? (size_t)observer->n_old : 0;
    const size_t o_obsprog = take(observer ? sizeof(*observer) : 0), o_obsold = take(n_old * n * 4);
    const int obs_width = observer ? observer->width : 4;
    const EnvIo io(n, (size_t)obs_width);
    const size_t o_io = take(io.bytes);
    // the episode records' arrays (rf_env_configure_records points EnvState at them; null until then)
    // (the three outputs as one piece, the float64 array first: one copy fetches them)
    const size_t rec_bytes = n * 8 + n * (size_t)obs_width * 4 + n * 4;
    const size_t o_epret = take(n * 8), o_eplen = take(n * 4), o_final = take(rec_bytes);
    const size_t rec_off[5] = {o_epret, o_eplen, o_final + n * 8, o_final, o_final + n * 8 + n * (size_t)obs_width * 4};
    RF_HIP(dev_malloc(&ctx->env_block, off));
    RF_HIP(hipMemsetAsync(ctx->env_block, 0, off, ctx->stream));
    char *base = (char *)ctx->env_block;
    rf::EnvState &s = ctx->env;
    s.state = (float *)(base + o_state);
    s.steps = (int *)(base + o_steps);
    s.diverging = (int *)(base + o_div);
    s.last_diff = (float *)(base + o_last);
    s.old_wrapped = (float *)(base + o_oldw);
    s.old_focus = (float *)(base + o_oldf);
    s.cam_dyn = (float *)(base + o_cam);
    s.rect = (float *)(base + o_rect);
    s.cam_dyn2 = (float *)(base + o_cam2);
    s.rect2 = (float *)(base + o_rect2);
    s.done_index = (int *)(base + o_didx);
    s.done_count = (int *)(base + o_io + io.o_count);
    s.obs = (float *)(base + o_io + io.o_obs);
    s.reward = (double *)(base + o_io + io.o_rewards);
    s.truncated = (uint8_t *)(base + o_io + io.o_truncated);
    s.done = (uint8_t *)(base + o_done);
    s.sums2 = (unsigned long long *)(base + o_sums2);
    s.done_rank = (int *)(base + o_drank);
    s.program = program ? (const rf::EnvProgram *)(base + o_prog) : nullptr;
    s.leaf_count = program ? (int *)(base + o_count) : nullptr;
    s.leaf_float = program ? (float *)(base + o_float) : nullptr;
    s.history = program ? (float *)(base + o_hist) : nullptr;
    s.leaf_old = program ? (float *)(base + o_old) : nullptr;
    s.observer = observer ? (const rf_env_observer_program *)(base + o_obsprog) : nullptr;
    s.obs_old = observer ? (float *)(base + o_obsold) : nullptr;
    s.ep_return = nullptr;
    s.ep_length = nullptr;
    s.final_obs = nullptr;
    s.final_return = nullptr;
    s.final_length = nullptr;
    ctx->env_records = false;
    ctx->env_stepped = false;
    for (int i = 0; i < 5; ++i)
        ctx->env_rec_off[i] = rec_off[i];
    ctx->env_rec_bytes = rec_bytes;
    ctx->env_obs_width = obs_width;
    ctx->env_observer = observer ? *observer : rf_env_observer_program{};
    if (observer) { // (DeltaObserver._old_wrapped_observations starts as NaN; ctx->env_observer outlives the copy)
        RF_HIP(hipMemcpyAsync(base + o_obsprog, &ctx->env_observer, sizeof(*observer), hipMemcpyHostToDevice, ctx->stream));
        if (n_old)
            RF_HIP(hipMemsetD32Async((hipDeviceptr_t)(base + o_obsold), 0x7fc00000, n_old * n, ctx->stream));
        RF_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (program) {
        ctx->env_program = *program;
        RF_HIP(hipMemcpyAsync(base + o_prog, &prog, sizeof(prog), hipMemcpyHostToDevice, ctx->stream));
        RF_HIP(hipStreamSynchronize(ctx->stream)); // (prog lives on this stack frame)
    } else {
        ctx->env_program = rf_env_program{};
    }
    ctx->d_actions = (int *)(base + o_io + io.o_actions);
    ctx->d_pool = (float *)(base + o_io + io.o_pool);

    rf::EnvConfig &c = ctx->env_cfg;
    c.task = task;
    c.stop_threshold = stop_threshold;
    c.n = cfg->n;
    c.n_actions = cfg->n_actions;
    for (int i = 0; i < 32; ++i)
        c.action_set[i] = cfg->action_set[i];
    c.limit_lo = cfg->limit_lo;
    c.limit_hi = cfg->limit_hi;
    c.max_steps = cfg->max_steps;
    c.diverge_threshold = cfg->diverge_threshold;
    c.early_end_steps = cfg->early_end_steps;
    for (int i = 0; i < 4; ++i) {
        c.mid[i] = cfg->mid[i];
        c.scale[i] = cfg->scale[i];
    }
    c.reward_scale = cfg->reward_scale;
    c.on_target_span = cfg->on_target_span;
    c.half_width = cfg->half_width;
    c.half_height = cfg->half_height;
    c.tan_half_r = cfg->tan_half_r;
    for (int i = 0; i < 3; ++i) {
        c.look_from[i] = cfg->look_from[i];
        c.cam_u[i] = cfg->cam_u[i];
        c.cam_v[i] = cfg->cam_v[i];
        c.cam_w[i] = cfg->cam_w[i];
    }
    c.frame_pixels = (unsigned long long)cfg->frame_height * (unsigned long long)cfg->frame_height;
    ctx->env_host = *cfg;
    {
        int rc = ensure_focus(ctx, cfg->n); // (the environment kernels zero and read the sums themselves)
        if (rc != RF_OK)
            return rc;
        ctx->env.sums = ctx->d_sums;
    }
    ctx->cs = rf::CamStatic{cfg->look_from[0], cfg->look_from[1], cfg->look_from[2], cfg->cam_u[0], cfg->cam_u[1],
                            cfg->cam_u[2],     cfg->cam_v[0],     cfg->cam_v[1],     cfg->cam_v[2], cfg->lens_radius,
                            0.0f,              0.0f,              0};
    lens_split(ctx->cs);
    // canonical frame -> horizontal = (h2, +0, +0), vertical = (+0, v2, +0): the AXIS kernels apply
    // the target's half side is target * tan_half_r at distance target; the frame's half width at
    // that distance is target * half_width (camera.py:147-160, world.py:114-116)
    ctx->hit_fraction = (cfg->half_width > 0.0 && cfg->tan_half_r > 0.0 && cfg->tan_half_r < cfg->half_width)
                            ? cfg->tan_half_r / cfg->half_width
                            : (cfg->tan_half_r >= cfg->half_width ? 1.0 : 0.658);
    ctx->env_axis = cfg->look_from[0] == 0.0f && cfg->look_from[1] == 0.0f && cfg->look_from[2] == 0.0f &&
                    cfg->cam_u[0] == 1.0f && cfg->cam_u[1] == 0.0f && cfg->cam_u[2] == 0.0f &&
                    cfg->cam_v[0] == 0.0f && cfg->cam_v[1] == 1.0f && cfg->cam_v[2] == 0.0f &&
                    !signbit(cfg->cam_u[1]) && !signbit(cfg->cam_u[2]) && !signbit(cfg->cam_v[0]) &&
                    !signbit(cfg->cam_v[2]) && cfg->half_width > 0.0 && cfg->half_height > 0.0;
    ctx->scene_n = 0; // the env owns the scene arrays from now on
    ctx->env_pending = -1;
    ctx->env_planned = false;
    ctx->env_ready = true;
    return RF_OK;
}

// What every launch of a schedule needs of the configured environment, made once from the context.  count: the
// schedule's renders count their pixels as they are launched; a schedule that is enqueued in one go counts after the
// step instead (its launches may be replayed, and skip slots).
struct EnvLaunch {
    int n, fh, spp, gray_mode;
    dim3 grid, block; // one thread per environment
    bool count;
    EnvLaunch(const rf_ctx *ctx, bool count_)
        : n(ctx->env_host.n), fh(ctx->env_host.frame_height), spp(ctx->env_host.spp),
          gray_mode(ctx->env_host.gray_mode), grid((n + 255) / 256), block(256), count(count_)
    {
    }
    unsigned long long pixels(int envs) const { return (unsigned long long)envs * (unsigned long long)fh * fh; }
};

constexpr int kEnvResetNone = -1; // fused_pass: nobody ended, nothing to pack

// In place of the pool's copy from the host: rows 0 .. rows-1 of the draw that starts at the generator's state, into
// `out` (float32[rows][2]: the pool, or in rf_env_reset the states themselves).
void launch_draw_pool(rf_ctx *ctx, float *out, int rows)
{
    hipLaunchKernelGGL(rf::env_draw_pool_kernel, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream,
                       (const rf::EnvInit *)ctx->d_init, (const unsigned long long *)init_gen(ctx), out, rows);
}

// initialize(k) of the host twin once the step's count is final on the device (count == null: `given` rows)
void launch_init_advance(rf_ctx *ctx, const int *count, int given)
{
    hipLaunchKernelGGL(rf::env_init_advance_kernel, dim3(1), dim3(64), 0, ctx->stream, (const rf::EnvInit *)ctx->d_init,
                       init_gen(ctx), count, given);
}

void launch_reset_kernel(rf_ctx *ctx, const float *pool, int mode, const int *actions)
{
    hipLaunchKernelGGL(rf::env_reset_kernel, dim3(1), dim3(1024), 0, ctx->stream, ctx->env_cfg, ctx->env, pool, mode,
                       actions);
}

// The full pass: env_pre_kernel (if `pre`), the render of all n environments, their focus measure, env_post_kernel.
// A pre kernel without actions starts the episodes (rf_env_reset): env_post_kernel then takes its `first` form.
int full_pass(rf_ctx *ctx, const EnvLaunch &d, bool pre, const int *actions)
{
    const bool first = pre && !actions;
    if (pre)
        hipLaunchKernelGGL(rf::env_pre_kernel, d.grid, d.block, 0, ctx->stream, ctx->env_cfg, ctx->env, actions);
    int rc = launch_render(ctx, d.n, d.fh, d.fh, d.spp, ctx->env.cam_dyn, ctx->env.rect, ctx->env_axis, d.count);
    if (rc == RF_OK && first && fused_step_possible(ctx))
        rc = ensure_frames2(ctx, d.n, d.fh, d.fh); // (not inside a step: the first one after this may already be captured)
    if (rc == RF_OK)
        rc = launch_focus(ctx, d.n, d.fh, d.fh, d.gray_mode, nullptr, true);
    if (rc != RF_OK)
        return rc;
    hipLaunchKernelGGL(rf::env_post_kernel, d.grid, d.block, 0, ctx->stream, ctx->env_cfg, ctx->env,
                       (const double *)nullptr, first ? 1 : 0);
    return RF_OK;
}

// The reset pass over `slots` compacted rows (vector_environment.py:137-151): env_reset_kernel in `mode` --
// kEnvResetApply for the k rows of a count the host knows, kEnvResetBoth for all n slots (it ranks too, and marks the
// unused slots, whose blocks exit at once) --, the render of the compacted set and its focus measure, or with
// render == false the focus values somebody else measured (in d_var), then env_reset_post_kernel.
int reset_pass(rf_ctx *ctx, const EnvLaunch &d, int slots, int mode, bool render)
{
    launch_reset_kernel(ctx, ctx->d_pool, mode, nullptr);
    if (render) {
        int rc = launch_render(ctx, slots, d.fh, d.fh, d.spp, ctx->env.cam_dyn2, ctx->env.rect2, ctx->env_axis, d.count);
        if (rc == RF_OK)
            rc = launch_focus(ctx, slots, d.fh, d.fh, d.gray_mode, mode == rf::kEnvResetBoth ? ctx->env.rect2 : nullptr,
                              true);
        if (rc != RF_OK)
            return rc;
    }
    hipLaunchKernelGGL(rf::env_reset_post_kernel, dim3((slots + 255) / 256), dim3(256), 0, ctx->stream, ctx->env_cfg,
                       ctx->env, render ? (const double *)nullptr : (const double *)ctx->d_var, (const float *)nullptr);
    return RF_OK;
}

// The fused pass: one render launch and one focus launch per step.  Which environments end depends on their counters
// alone (env_pre_kernel), so they are ranked and the compacted scene of the auto-reset is packed BEFORE the render --
// `mode` kEnvResetPlan: from the step's actions; kEnvResetPack: for a ranking that exists already (rf_env_step_plan);
// kEnvResetNone: nobody ended --; the r-th of them is rendered as row r of that set with the RNG streams of slot r
// (render.py:217), i.e. right after slot r's own frame: the blocks of the slots below the count make two passes
// (render_kernel_coop2<.., TWO>).  The step's frames of those slots go to frames2, so that the frame buffer ends up as
// the two launches leave it.  The render cannot count its own pixels: the count is on the device.
int fused_pass(rf_ctx *ctx, const EnvLaunch &d, int mode)
{
    if (mode != kEnvResetNone)
        launch_reset_kernel(ctx, ctx->d_pool, mode, mode == rf::kEnvResetPlan ? ctx->d_actions : nullptr);
    const SecondPass second{ctx->env.done_count, ctx->env.cam_dyn2, ctx->env.rect2};
    int rc = launch_render(ctx, d.n, d.fh, d.fh, d.spp, ctx->env.cam_dyn, ctx->env.rect, ctx->env_axis, false, &second);
    if (rc == RF_OK)
        rc = launch_focus(ctx, d.n, d.fh, d.fh, d.gray_mode, nullptr, true, ctx->env.done_count);
    if (rc != RF_OK)
        return rc;
    hipLaunchKernelGGL(rf::env_finish_kernel, d.grid, d.block, 0, ctx->stream, ctx->env_cfg, ctx->env,
                       (const float *)ctx->d_pool);
    return RF_OK;
}

// May a step start?  `open_step`: what the entry point `fn` says while a two-phase step is open.
template <typename T>
int step_may_start(const rf_ctx *ctx, const T *host_actions, const char *fn, const char *open_step)
{
    RF_REQUIRE(ctx->env_ready, "%s: rf_env_configure first", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: %s", fn, open_step);
    RF_REQUIRE(!ctx->env_needs_reset, "%s: a step was aborted (rf_env_reset first)", fn);
    RF_REFUSE_FAULTED(ctx, fn);
    return check_actions(ctx, host_actions, fn);
}

// The end of a whole step in which k environments ended: the renderer holds their compacted set, or the full one.
void finish_step(rf_ctx *ctx, int k)
{
    ctx->env_steps += 1;
    ctx->env_step_index += 1;
    ctx->env_stepped = true;
    ctx->env_scene_len = k > 0 ? k : ctx->env_host.n;
    ctx->env_last_partial = k > 0;
}

// A reset clears a fault: the host's record of it, and the word on the device (in stream order, after the device steps
// that may still write it).
int clear_fault(rf_ctx *ctx)
{
    ctx->env_fault_step = ctx->env_fault_env = -1;
    if (ctx->d_io_state)
        RF_HIP(hipMemsetAsync(&((rf::EnvIoState *)ctx->d_io_state)->fault, 0xFF, sizeof(unsigned long long), ctx->stream));
    return RF_OK;
}

bool env_one_sync(const rf_ctx *ctx)
{
    const int n = ctx->env_host.n, fh = ctx->env_host.frame_height;
    const long tiles = (long)((fh + 127) / 128) * ((fh + 5) / 6); // (blocks of the default 128 x 6 tiles, rf_coop2.h)
    return (long)n * tiles <= ctx->env_one_sync_max;
}

// What a step enqueued in one go runs between its inputs' arrival and its results' departure: the pool's draw on a
// context with a device initializer, the fused pass -- or the full pass and the reset pass over all n slots --, the
// generator's advance.  Reads the actions in ctx->d_actions; used directly and under stream capture.
int enqueue_env_step_body(rf_ctx *ctx, const EnvLaunch &d)
{
    const bool draw = ctx->env_init; // the pool is drawn here, where its copy would arrive
    if (draw)
        launch_draw_pool(ctx, ctx->d_pool, d.n);
    int rc;
    if (fused_step_possible(ctx)) {
        rc = fused_pass(ctx, d, rf::kEnvResetPlan);
    } else {
        rc = full_pass(ctx, d, true, ctx->d_actions);
        if (rc == RF_OK)
            rc = reset_pass(ctx, d, d.n, rf::kEnvResetBoth, true);
    }
    if (rc != RF_OK)
        return rc;
    if (draw)
        launch_init_advance(ctx, ctx->env.done_count, 0);
    return RF_OK;
}

// Enqueues one whole step on the ctx's stream without waiting for anything: uploads, the body above, the downloads.
// Used directly and under stream capture.
int enqueue_env_step(rf_ctx *ctx, const void *actions, const float *pool, float *obs, double *rewards,
                     uint8_t *truncated, int *count, uint8_t *host_io = nullptr)
{
    // host_io: the host side is an image of the device's io block (EnvIo: the pinned staging buffer of the replayed
    // step) -- one copy in, one copy out; otherwise the caller's six separate arrays
    const EnvLaunch d(ctx, false);
    const size_t n = (size_t)d.n;
    const EnvIo io(n, (size_t)ctx->env_obs_width);
    uint8_t *const d_io = (uint8_t *)ctx->d_pool; // (the io block starts with the pool)
    const bool draw = ctx->env_init; // (the body draws the pool where its copy would arrive)
    if (host_io && !draw) {
        RF_HIP(hipMemcpyAsync(d_io, host_io, io.in_bytes, hipMemcpyHostToDevice, ctx->stream));
    } else if (host_io) {
        RF_HIP(hipMemcpyAsync(d_io + io.o_actions, host_io + io.o_actions, io.in_bytes - io.o_actions, hipMemcpyHostToDevice,
                              ctx->stream));
    } else {
        RF_HIP(hipMemcpyAsync(ctx->d_actions, actions, n * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!draw)
            RF_HIP(hipMemcpyAsync(ctx->d_pool, pool, n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    if (int rc = enqueue_env_step_body(ctx, d))
        return rc;
    if (host_io) {
        RF_HIP(hipMemcpyAsync(host_io + io.o_rewards, d_io + io.o_rewards, io.bytes - io.o_rewards, hipMemcpyDeviceToHost,
                              ctx->stream));
    } else {
        RF_HIP(hipMemcpyAsync(count, ctx->env.done_count, 4, hipMemcpyDeviceToHost, ctx->stream));
        RF_HIP(hipMemcpyAsync(rewards, ctx->env.reward, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        RF_HIP(hipMemcpyAsync(truncated, ctx->env.truncated, n, hipMemcpyDeviceToHost, ctx->stream));
        RF_HIP(hipMemcpyAsync(obs, ctx->env.obs, io.obs_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    return RF_OK;
}

// The replayed step's pinned staging block (an image of the io block, `bytes`) and its graph, made when missing.
// Capture problems are not the caller's problem: RF_OK with ctx->env_graph still null says that the graph is disabled
// from now on and the step keeps being enqueued call by call (same kernels, same results).
int ensure_env_graph(rf_ctx *ctx, size_t bytes)
{
    if (ctx->h_stage_bytes < bytes) {
        if (ctx->env_graph)
            (void)hipGraphExecDestroy(ctx->env_graph);
        ctx->env_graph = nullptr;
        if (ctx->h_stage)
            RF_HIP(hipHostFree(ctx->h_stage));
        ctx->h_stage = nullptr;
        ctx->h_stage_bytes = 0;
        RF_HIP(host_malloc((void **)&ctx->h_stage, bytes));
        ctx->h_stage_bytes = bytes;
    }
    if (ctx->env_graph)
        return RF_OK;
    hipGraph_t captured = nullptr;
    hipError_t he = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
    int rc = RF_OK;
    if (he == hipSuccess) {
        rc = enqueue_env_step(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ctx->h_stage);
        he = hipStreamEndCapture(ctx->stream, &captured);
        if (he == hipSuccess && rc == RF_OK && ctx->env_graph_fail_once) {
            ctx->env_graph_fail_once = false; // test hook: behave as if instantiation had failed
            he = hipErrorUnknown;
        } else if (he == hipSuccess && rc == RF_OK)
            he = hipGraphInstantiate(&ctx->env_graph, captured, nullptr, nullptr, 0);
        if (captured)
            (void)hipGraphDestroy(captured);
    }
    if (he != hipSuccess || rc != RF_OK || !ctx->env_graph) {
        (void)hipGetLastError();
        ctx->env_graph = nullptr;
        ctx->env_graph_enabled = false;
    }
    return RF_OK;
}

// First half of a step: transform, enders, full render + focus, observations, rewards, flags, and
// the ranking of the environments that ended (vector_environment.py:124-135).  Synchronises once:
// *k, rewards and truncated are final on return; the observations of the environments that did not
// end are final on the device.
int env_step_begin(rf_ctx *ctx, const void *host_actions, double *host_rewards, uint8_t *host_truncated, int *k)
{
    const EnvLaunch d(ctx, true);
    const size_t n = (size_t)d.n;
    RF_HIP(hipMemcpyAsync(ctx->d_actions, host_actions, n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = full_pass(ctx, d, true, ctx->d_actions))
        return rc;
    launch_reset_kernel(ctx, nullptr, rf::kEnvResetRank, nullptr);
    RF_HIP(hipGetLastError());
    RF_HIP(hipMemcpyAsync(k, ctx->env.done_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipMemcpyAsync(host_rewards, ctx->env.reward, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipMemcpyAsync(host_truncated, ctx->env.truncated, n, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

// Second half: the k environments that ended take host_pool's rows 0..k-1 in index order and are rendered and scored
// again (the reset pass, sized by k) -- or, with host_focus, take the focus values that were measured elsewhere.
int env_step_end(rf_ctx *ctx, const float *host_pool, const double *host_focus, int k, float *host_obs)
{
    const EnvLaunch d(ctx, true);
    if (k > 0) {
        if (ctx->env_init) // (rf_env_step's count-sized schedule: only the k rows that are used are drawn)
            launch_draw_pool(ctx, ctx->d_pool, k);
        else
            RF_HIP(hipMemcpyAsync(ctx->d_pool, host_pool, (size_t)k * 8, hipMemcpyHostToDevice, ctx->stream));
        if (host_focus) // (they take the place launch_focus would have filled)
            RF_HIP(hipMemcpyAsync(ctx->d_var, host_focus, (size_t)k * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        if (int rc = reset_pass(ctx, d, k, rf::kEnvResetApply, host_focus == nullptr))
            return rc;
        if (ctx->env_init)
            launch_init_advance(ctx, ctx->env.done_count, 0);
        RF_HIP(hipGetLastError());
    }
    RF_HIP(hipMemcpyAsync(host_obs, ctx->env.obs, env_obs_bytes(ctx), hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

// The two-phase and sharded halves hand pool rows to a context by the caller's own offsets; a device initializer has none.
#define RF_REFUSE_DEVICE_INITIALIZER(ctx, fn)                                                                      \
    RF_REQUIRE(!((ctx)->env_ready && (ctx)->env_init),                                                             \
               "%s: the context draws its reset states itself (rf_env_configure_initializer): only whole steps", fn)

// rf_env_step / rf_env_step_jumps: T = int32_t or float (check_actions)
template <typename T>
int env_step(rf_ctx *ctx, const T *host_actions, const float *host_pool, float *host_obs, double *host_rewards,
             uint8_t *host_truncated, int *host_n_reset, const char *fn)
{
    RF_REQUIRE(ctx != nullptr && host_actions && host_obs && host_rewards && host_truncated, "%s: NULL argument", fn);
    RF_REQUIRE(host_pool || (ctx->env_ready && ctx->env_init), "%s: NULL argument", fn);
    RF_REQUIRE(!host_pool || !(ctx->env_ready && ctx->env_init),
               "%s: the context draws its reset states itself (rf_env_configure_initializer): host_pool must be NULL", fn);
    if (int rc = resolve_device_steps(ctx)) // (device steps before this one: their bookkeeping, and a fault of theirs)
        return rc;
    if (int rc = step_may_start(ctx, host_actions, fn, "a two-phase step is open (rf_env_step_end first)"))
        return rc;
    const EnvLaunch d(ctx, false);
    const size_t n = (size_t)d.n;
    int k = 0;
    // vector_environment.py:137-151: the envs that just ended are rendered again.  Small
    // configurations are launch- and sync-bound: their step is enqueued in one go (see
    // enqueue_env_step) and, from the second step on (all buffers have their final size by then),
    // replayed as one hipGraph through pinned staging buffers; it ends with its only host
    // synchronisation.  Large ones size the auto-reset launch by the count, which costs one round
    // trip and saves up to a few hundred thousand empty blocks.
    const bool fused = fused_step_possible(ctx); // (one render launch, no count to wait for: enqueued in one go at any size)
    if (fused || env_one_sync(ctx)) {
        const EnvIo io(n, (size_t)ctx->env_obs_width);
        bool graph = ctx->env_graph_enabled && !ctx->timing && ctx->env_steps >= 1;
        if (graph) {
            if (int rc = ensure_env_graph(ctx, io.bytes))
                return rc;
            graph = ctx->env_graph != nullptr;
        }
        if (graph) {
            uint8_t *st = ctx->h_stage;
            memcpy(st + io.o_actions, host_actions, n * 4);
            if (host_pool)
                memcpy(st + io.o_pool, host_pool, n * 8);
            RF_HIP(hipGraphLaunch(ctx->env_graph, ctx->stream));
            RF_HIP(hipStreamSynchronize(ctx->stream));
            memcpy(host_obs, st + io.o_obs, io.obs_bytes);
            memcpy(host_rewards, st + io.o_rewards, n * 8);
            memcpy(host_truncated, st + io.o_truncated, n);
            k = *(const int *)(st + io.o_count);
            ctx->env_last_branch = fused ? RF_ENV_BRANCH_FUSED_GRAPH : RF_ENV_BRANCH_GRAPH;
        } else {
            int rc = enqueue_env_step(ctx, host_actions, host_pool, host_obs, host_rewards, host_truncated, &k);
            if (rc != RF_OK)
                return rc;
            RF_HIP(hipGetLastError());
            RF_HIP(hipStreamSynchronize(ctx->stream));
            ctx->env_last_branch = fused ? RF_ENV_BRANCH_FUSED : RF_ENV_BRANCH_ONE_SYNC;
        }
        // what this step really rendered: all n environments, then the k that ended (the other slots of the
        // second launch exit at once)
        rfh::count_pixels(d.pixels(d.n + k));
    } else {
        // the step's flags and rewards are final after the first half; the count sizes the partial render
        int rc = env_step_begin(ctx, host_actions, host_rewards, host_truncated, &k);
        if (rc == RF_OK)
            rc = env_step_end(ctx, host_pool, nullptr, k, host_obs);
        if (rc != RF_OK)
            return rc;
        ctx->env_last_branch = RF_ENV_BRANCH_COUNT_SIZED;
    }
    finish_step(ctx, k);
    if (ctx->env_view) { // (after the step's own synchronisation: rf_env_get_view waits for it)
        if (int rc = enqueue_view(ctx, false, nullptr, nullptr, nullptr)) {
            ctx->env_needs_reset = true; // the step ran, its view did not
            return rc;
        }
    }
    if (host_n_reset)
        *host_n_reset = k;
    return RF_OK;
}

template <typename T>
int env_step_begin_checked(rf_ctx *ctx, const T *host_actions, double *host_rewards, uint8_t *host_truncated,
                           int *host_n_reset, const char *fn)
{
    RF_REQUIRE(ctx != nullptr && host_actions && host_rewards && host_truncated && host_n_reset, "%s: NULL argument", fn);
    RF_REFUSE_DEVICE_INITIALIZER(ctx, fn);
    RF_REFUSE_VIEW(ctx, fn);
    if (int rc = step_may_start(ctx, host_actions, fn, "the previous step was not finished (rf_env_step_end)"))
        return rc;
    drop_env_graph(ctx);
    int k = 0;
    int rc = env_step_begin(ctx, host_actions, host_rewards, host_truncated, &k);
    if (rc != RF_OK)
        return rc;
    ctx->env_pending = k;
    *host_n_reset = k;
    return RF_OK;
}

template <typename T>
int env_step_plan(rf_ctx *ctx, const T *host_actions, int *host_n_reset, const char *fn)
{
    RF_REQUIRE(ctx != nullptr && host_actions && host_n_reset, "%s: NULL argument", fn);
    RF_REFUSE_DEVICE_INITIALIZER(ctx, fn);
    RF_REFUSE_VIEW(ctx, fn);
    if (int rc = step_may_start(ctx, host_actions, fn, "the previous step was not finished"))
        return rc;
    drop_env_graph(ctx);
    RF_HIP(hipMemcpyAsync(ctx->d_actions, host_actions, (size_t)ctx->env_host.n * 4, hipMemcpyHostToDevice, ctx->stream));
    // the kernel below applies the actions and advances the counters: from here until the step is open (a HIP failure
    // returns early) only a reset makes the environment usable again -- a retried step would apply the actions twice
    ctx->env_needs_reset = true;
    launch_reset_kernel(ctx, nullptr, rf::kEnvResetRank, ctx->d_actions);
    RF_HIP(hipGetLastError());
    int k = 0;
    RF_HIP(hipMemcpyAsync(&k, ctx->env.done_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->env_pending = k;
    ctx->env_planned = true;
    ctx->env_needs_reset = false;
    *host_n_reset = k;
    return RF_OK;
}

// ---- device steps: rf_env_step_device, rf_env_reset_device (kernels: rf_env_io.h) -----------------------------------

// The ctx's stream waits for what the caller's stream holds now / the caller's stream waits for what the ctx's holds
// now: ordering by events only, no host synchronisation.
int wait_for_caller(rf_ctx *ctx, hipStream_t caller)
{
    RF_HIP(hipEventRecord(ctx->io_ev_in, caller));
    RF_HIP(hipStreamWaitEvent(ctx->stream, ctx->io_ev_in, 0));
    return RF_OK;
}

int let_caller_wait(rf_ctx *ctx, hipStream_t caller)
{
    RF_HIP(hipEventRecord(ctx->io_ev_out, ctx->stream));
    RF_HIP(hipStreamWaitEvent(caller, ctx->io_ev_out, 0));
    return RF_OK;
}

// The graph of a device step: enqueue_env_step_body alone -- no copy and no pointer of the caller's, so it is valid for
// whatever arrays the next call brings; the gather before it and the scatter after it are launched around the replay.
// As for ensure_env_graph, a capture problem disables replay and the step keeps being enqueued call by call.
int ensure_env_graph_dev(rf_ctx *ctx, const EnvLaunch &d)
{
    if (ctx->env_graph_dev)
        return RF_OK;
    hipGraph_t captured = nullptr;
    hipError_t he = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
    int rc = RF_OK;
    if (he == hipSuccess) {
        rc = enqueue_env_step_body(ctx, d);
        he = hipStreamEndCapture(ctx->stream, &captured);
        if (he == hipSuccess && rc == RF_OK)
            he = hipGraphInstantiate(&ctx->env_graph_dev, captured, nullptr, nullptr, 0);
        if (captured)
            (void)hipGraphDestroy(captured);
    }
    if (he != hipSuccess || rc != RF_OK || !ctx->env_graph_dev) {
        (void)hipGetLastError();
        ctx->env_graph_dev = nullptr;
        ctx->env_graph_enabled = false;
    }
    return RF_OK;
}

// rf_env_step_device / rf_env_step_device_records: the latter's three arrays are NULL for the former
int env_step_device(rf_ctx *ctx, const void *d_actions, int action_dtype, float *d_obs, double *d_rewards,
                    uint8_t *d_truncated, int32_t *d_n_reset, float *d_final_obs, double *d_returns, int32_t *d_lengths,
                    float *d_view_obs, double *d_view_rewards, float *d_view_final, void *caller_stream, const char *fn)
{
    RF_REQUIRE(d_actions && d_obs && d_rewards && d_truncated, "%s: NULL argument", fn);
    RF_REQUIRE(action_dtype == RF_ACTION_I32 || action_dtype == RF_ACTION_I64 || action_dtype == RF_ACTION_F32,
               "%s: unknown action_dtype %d", fn, action_dtype);
    RF_REQUIRE(ctx->env_ready, "%s: rf_env_configure first", fn);
    RF_REQUIRE(ctx->env_init, "%s: the context has no device initializer (rf_env_configure_initializer): the host's "
               "initializer advances by the number of environments that ended, which only a synchronisation can tell it", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase or planned step is open", fn);
    RF_REQUIRE(!ctx->env_needs_reset, "%s: a step was aborted (rf_env_reset first)", fn);
    RF_REFUSE_FAULTED(ctx, fn);
    RF_REQUIRE(ctx->env_records || !(d_final_obs || d_returns || d_lengths),
               "%s: the context keeps no episode records (rf_env_configure_records)", fn);
    RF_REQUIRE(ctx->env_view || !(d_view_obs || d_view_rewards || d_view_final),
               "%s: the context has no learner view (rf_env_configure_view)", fn);
    RF_REQUIRE(ctx->env_records || !d_view_final,
               "%s: d_view_final needs episode records (rf_env_configure_records before rf_env_configure_view)", fn);
    const int task = ctx->env_cfg.task;
    const bool index_task = task == rf::kEnvTaskSteps || (task == rf::kEnvTaskComposed && composed_discrete(ctx));
    RF_REQUIRE(index_task == (action_dtype != RF_ACTION_F32), "%s: the context takes %s actions", fn,
               index_task ? "RF_ACTION_I32 / RF_ACTION_I64" : "RF_ACTION_F32");
    const int rule = index_task ? rf::kActionRuleIndex
                     : (task == rf::kEnvTaskJumps || ctx->env_program.transformer == RF_TRANSFORM_CONTINUOUS_JUMP)
                         ? rf::kActionRuleJump
                         : rf::kActionRuleFinite;
    const int n_actions = task == rf::kEnvTaskComposed ? ctx->env_program.n_actions : ctx->env_host.n_actions;
    const EnvLaunch d(ctx, false);
    const size_t n = (size_t)d.n, action_bytes = action_dtype == RF_ACTION_I64 ? 8 : 4;
    int rc = check_device_array(ctx, d_actions, n * action_bytes, action_bytes, "d_actions", fn);
    if (rc == RF_OK)
        rc = check_device_array(ctx, d_obs, env_obs_bytes(ctx), 4, "d_obs", fn);
    if (rc == RF_OK)
        rc = check_device_array(ctx, d_rewards, n * 8, 8, "d_rewards", fn);
    if (rc == RF_OK)
        rc = check_device_array(ctx, d_truncated, n, 1, "d_truncated", fn);
    if (rc == RF_OK && d_n_reset)
        rc = check_device_array(ctx, d_n_reset, 4, 4, "d_n_reset", fn);
    if (rc == RF_OK && d_final_obs)
        rc = check_device_array(ctx, d_final_obs, env_obs_bytes(ctx), 4, "d_final_obs", fn);
    if (rc == RF_OK && d_returns)
        rc = check_device_array(ctx, d_returns, n * 8, 8, "d_returns", fn);
    if (rc == RF_OK && d_lengths)
        rc = check_device_array(ctx, d_lengths, n * 4, 4, "d_lengths", fn);
    const size_t view_bytes = ctx->env_view ? env_obs_bytes(ctx) * (size_t)ctx->view_cfg.frame_stack : 0;
    if (rc == RF_OK && d_view_obs)
        rc = check_device_array(ctx, d_view_obs, view_bytes, 4, "d_view_obs", fn);
    if (rc == RF_OK && d_view_rewards)
        rc = check_device_array(ctx, d_view_rewards, n * 8, 8, "d_view_rewards", fn);
    if (rc == RF_OK && d_view_final)
        rc = check_device_array(ctx, d_view_final, view_bytes, 4, "d_view_final", fn);
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (rc == RF_OK)
        rc = refuse_capturing(caller, fn);
    if (rc != RF_OK)
        return rc;
    // the schedule: as rf_env_step's enqueued-in-one-go branch at any size (the count-sized one needs a round trip)
    const bool fused = fused_step_possible(ctx);
    // ... replayed where rf_env_step replays: not at the sizes whose host form takes the count-sized schedule
    bool graph = ctx->env_graph_enabled && !ctx->timing && ctx->env_steps >= 1 && (fused || env_one_sync(ctx));
    ctx->env_needs_reset = true; // until the whole step is enqueued (a HIP failure below returns early)
    if (int rc2 = wait_for_caller(ctx, caller))
        return rc2;
    if (graph) { // (captured on the ctx's stream, which holds nothing of this step yet but the wait)
        if (int rc2 = ensure_env_graph_dev(ctx, d))
            return rc2;
        graph = ctx->env_graph_dev != nullptr;
    }
    rf::EnvIoState *io = (rf::EnvIoState *)ctx->d_io_state;
    hipLaunchKernelGGL(rf::env_gather_actions_kernel, d.grid, d.block, 0, ctx->stream, d_actions, action_dtype, rule,
                       n_actions, d.n, (unsigned)ctx->env_step_index, ctx->d_actions, io);
    if (graph) {
        RF_HIP(hipGraphLaunch(ctx->env_graph_dev, ctx->stream));
    } else if (int rc2 = enqueue_env_step_body(ctx, d)) {
        return rc2;
    }
    const int cells = d.n * ctx->env_obs_width, blocks = (cells + 255) / 256;
    hipLaunchKernelGGL(rf::env_scatter_results_kernel, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, ctx->stream,
                       (const float *)ctx->env.obs, (const double *)ctx->env.reward, (const uint8_t *)ctx->env.truncated,
                       (const int *)ctx->env.done_count, d.n, ctx->env_obs_width, d_obs, d_rewards, d_truncated, d_n_reset,
                       io, (const float *)ctx->env.final_obs, (const double *)ctx->env.final_return,
                       (const int *)ctx->env.final_length, d_final_obs, d_returns, d_lengths);
    RF_HIP(hipGetLastError());
    if (ctx->env_view) {
        if (int rc2 = enqueue_view(ctx, false, d_view_obs, d_view_rewards, d_view_final))
            return rc2;
    }
    if (int rc2 = let_caller_wait(ctx, caller))
        return rc2;
    ctx->env_needs_reset = false;
    ctx->env_last_branch = fused ? (graph ? RF_ENV_BRANCH_FUSED_GRAPH : RF_ENV_BRANCH_FUSED)
                                 : (graph ? RF_ENV_BRANCH_GRAPH : RF_ENV_BRANCH_ONE_SYNC);
    ctx->env_steps += 1;
    ctx->env_step_index += 1;
    ctx->env_stepped = true;
    ctx->io_unresolved = ctx->io_scene_pending = true; // (finish_step's words wait for somebody to ask)
    return RF_OK;
}

// rf_env_reset_device / rf_env_reset_device_view: d_view_obs is NULL for the former
int env_reset_device(rf_ctx *ctx, float *d_obs, float *d_view_obs, void *caller_stream, const char *fn)
{
    RF_REQUIRE(d_obs != nullptr, "%s: NULL argument", fn);
    RF_REQUIRE(ctx->env_ready, "%s: rf_env_configure first", fn);
    RF_REQUIRE(ctx->env_init, "%s: the context has no device initializer (rf_env_configure_initializer) to draw the "
               "states from", fn);
    RF_REQUIRE(ctx->env_view || !d_view_obs, "%s: the context has no learner view (rf_env_configure_view)", fn);
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = check_device_array(ctx, d_obs, env_obs_bytes(ctx), 4, "d_obs", fn))
        return rc;
    if (d_view_obs) {
        if (int rc = check_device_array(ctx, d_view_obs, env_obs_bytes(ctx) * (size_t)ctx->view_cfg.frame_stack, 4,
                                        "d_view_obs", fn))
            return rc;
    }
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    ctx->env_pending = -1;
    ctx->env_planned = false;
    ctx->env_needs_reset = true; // until everything is enqueued
    if (int rc = wait_for_caller(ctx, caller))
        return rc;
    if (int rc = clear_fault(ctx))
        return rc;
    const EnvLaunch d(ctx, true);
    launch_draw_pool(ctx, ctx->env.state, d.n); // initializer.initialize(num_envs), as rf_env_reset(ctx, NULL, obs)
    launch_init_advance(ctx, nullptr, d.n);
    if (int rc = full_pass(ctx, d, true, nullptr))
        return rc;
    const int cells = d.n * ctx->env_obs_width, blocks = (cells + 255) / 256;
    hipLaunchKernelGGL(rf::env_scatter_obs_kernel, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, ctx->stream,
                       (const float *)ctx->env.obs, cells, d_obs);
    RF_HIP(hipGetLastError());
    if (ctx->env_view) {
        if (int rc = enqueue_view(ctx, true, d_view_obs, nullptr, nullptr))
            return rc;
    }
    if (int rc = let_caller_wait(ctx, caller))
        return rc;
    ctx->env_needs_reset = false;
    ctx->env_step_index = 0;
    ctx->env_scene_len = d.n; // (known without asking the device; the pixels of earlier device steps stay open)
    ctx->env_last_partial = false;
    ctx->io_scene_pending = false;
    ctx->env_started = true;
    return RF_OK;
}

} // namespace

namespace rfh {

int resolve_device_steps(rf_ctx *ctx)
{
    if (!ctx->io_unresolved)
        return RF_OK;
    rf::EnvIoState io{};
    int k = 0;
    RF_HIP(hipMemcpyAsync(&io, ctx->d_io_state, sizeof(io), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->io_scene_pending)
        RF_HIP(hipMemcpyAsync(&k, ctx->env.done_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    // every device step rendered its n environments, then the k that ended: the running total holds the sum
    const unsigned long long fh = (unsigned long long)ctx->env_host.frame_height;
    count_pixels((io.env_renders - ctx->io_renders_seen) * fh * fh);
    ctx->io_renders_seen = io.env_renders;
    if (ctx->io_scene_pending) { // finish_step's words, of the last device step
        ctx->env_scene_len = k > 0 ? k : ctx->env_host.n;
        ctx->env_last_partial = k > 0;
    }
    if (io.fault != rf::kNoFault && ctx->env_fault_step < 0) {
        ctx->env_fault_step = (int)(io.fault >> 32);
        ctx->env_fault_env = (int)(io.fault & 0xffffffffull);
    }
    ctx->io_unresolved = ctx->io_scene_pending = false;
    return RF_OK;
}

} // namespace rfh

extern "C" {

int rf_env_configure(rf_ctx *ctx, const rf_env_config *cfg)
{
    RF_REQUIRE(ctx != nullptr && cfg != nullptr, "rf_env_configure: NULL argument");
    RF_REQUIRE(cfg->n > 0 && cfg->n_actions > 0 && cfg->n_actions <= 32, "rf_env_configure: bad n / n_actions");
    RF_HIP(hipSetDevice(ctx->device));
    return env_configure(ctx, cfg, rf::kEnvTaskSteps, 0.0f);
}

int rf_env_configure_jumps(rf_ctx *ctx, const rf_env_config *cfg, float stop_threshold)
{
    RF_REQUIRE(ctx != nullptr && cfg != nullptr, "rf_env_configure_jumps: NULL argument");
    RF_REQUIRE(cfg->n > 0, "rf_env_configure_jumps: bad n");
    RF_REQUIRE(isfinite(cfg->limit_lo) && isfinite(cfg->limit_hi) && cfg->limit_lo < cfg->limit_hi,
               "rf_env_configure_jumps: limit_lo < limit_hi must be finite");
    RF_REQUIRE(isfinite(stop_threshold) && stop_threshold >= 0.0f, "rf_env_configure_jumps: stop_threshold");
    RF_HIP(hipSetDevice(ctx->device));
    return env_configure(ctx, cfg, rf::kEnvTaskJumps, stop_threshold);
}

int rf_env_configure_composed(rf_ctx *ctx, const rf_env_config *cfg, const rf_env_program *program)
{
    RF_REQUIRE(ctx != nullptr && cfg != nullptr && program != nullptr, "rf_env_configure_composed: NULL argument");
    RF_REQUIRE(cfg->n > 0, "rf_env_configure_composed: bad n");
    if (int rc = check_program(program, 4))
        return rc;
    RF_HIP(hipSetDevice(ctx->device));
    return env_configure(ctx, cfg, rf::kEnvTaskComposed, 0.0f, program);
}

int rf_env_configure_observed(rf_ctx *ctx, const rf_env_config *cfg, const rf_env_program *program,
                              const rf_env_observer_program *observer)
{
    RF_REQUIRE(ctx != nullptr && cfg != nullptr && program != nullptr && observer != nullptr,
               "rf_env_configure_observed: NULL argument");
    RF_REQUIRE(cfg->n > 0, "rf_env_configure_observed: bad n");
    if (int rc = check_observer_program(observer))
        return rc;
    if (int rc = check_program(program, observer->width))
        return rc;
    RF_HIP(hipSetDevice(ctx->device));
    return env_configure(ctx, cfg, rf::kEnvTaskComposed, 0.0f, program, observer);
}

int rf_env_get_observer_state(rf_ctx *ctx, float *host_old)
{
    RF_REQUIRE(ctx != nullptr && host_old != nullptr, "rf_env_get_observer_state: NULL argument");
    RF_REQUIRE(ctx->env_ready && ctx->env.observer != nullptr, "rf_env_get_observer_state: rf_env_configure_observed first");
    RF_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->env_observer.n_old * (size_t)ctx->env_host.n * 4;
    if (bytes)
        RF_HIP(hipMemcpyAsync(host_old, ctx->env.obs_old, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

int rf_env_configure_initializer(rf_ctx *ctx, const rf_env_initializer_program *program)
{
    const char *fn = "rf_env_configure_initializer";
    RF_REQUIRE(ctx != nullptr && program != nullptr, "%s: NULL argument", fn);
    RF_REQUIRE(ctx->env_ready, "%s: rf_env_configure first", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase step is open", fn);
    for (int j = 0; j < 2; ++j) {
        const int count = program->counts[j];
        RF_REQUIRE(count >= 1 && count <= RF_ENV_MAX_RANGES, "%s: element %d has %d ranges (1 to %d)", fn, j, count,
                   RF_ENV_MAX_RANGES);
        for (int c = 0; c < count; ++c) {
            const double low = program->low[j][c], span = program->span[j][c];
            RF_REQUIRE(isfinite(low) && isfinite(span), "%s: element %d range %d: low %g / span %g is not finite", fn, j, c,
                       low, span);
            RF_REQUIRE(fabs(low) < 3.4e38 && fabs(low + span) < 3.4e38,
                       "%s: element %d range %d: [%g, %g] is outside the float32 range", fn, j, c, low, low + span);
        }
    }
    RF_REQUIRE(program->inc[0] & 1u, "%s: the generator's increment is even", fn);
    RF_HIP(hipSetDevice(ctx->device));
    drop_env_graph(ctx); // (a captured step copies its pool from the host)
    RF_HIP(hipStreamSynchronize(ctx->stream));
    if (!ctx->d_init)
        RF_HIP(dev_malloc(&ctx->d_init, kInitGenOffset + sizeof(ctx->env_gen_host)));
    ctx->env_init_host = rf::init_program(*program);
    const unsigned long long gen[4] = {program->state[0], program->state[1], program->inc[0], program->inc[1]};
    memcpy(ctx->env_gen_host, gen, sizeof(gen));
    RF_HIP(hipMemcpyAsync(ctx->d_init, &ctx->env_init_host, sizeof(rf::EnvInit), hipMemcpyHostToDevice, ctx->stream));
    RF_HIP(hipMemcpyAsync(init_gen(ctx), ctx->env_gen_host, sizeof(gen), hipMemcpyHostToDevice, ctx->stream));
    // what device steps need besides: the fault word and the running total, and the two events that order a step
    // against the caller's stream (made here, where waiting is allowed, so that no device step ever allocates)
    if (int rc = resolve_device_steps(ctx))
        return rc;
    if (!ctx->d_io_state)
        RF_HIP(dev_malloc(&ctx->d_io_state, sizeof(rf::EnvIoState)));
    if (!ctx->io_ev_in)
        RF_HIP(hipEventCreateWithFlags(&ctx->io_ev_in, hipEventDisableTiming));
    if (!ctx->io_ev_out)
        RF_HIP(hipEventCreateWithFlags(&ctx->io_ev_out, hipEventDisableTiming));
    const rf::EnvIoState fresh{rf::kNoFault, 0};
    RF_HIP(hipMemcpyAsync(ctx->d_io_state, &fresh, sizeof(fresh), hipMemcpyHostToDevice, ctx->stream));
    ctx->io_renders_seen = 0;
    RF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->env_init = true;
    return RF_OK;
}

int rf_env_set_initializer_state(rf_ctx *ctx, const uint64_t state[2], const uint64_t inc[2])
{
    const char *fn = "rf_env_set_initializer_state";
    RF_REQUIRE(ctx != nullptr && state != nullptr && inc != nullptr, "%s: NULL argument", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_init, "%s: rf_env_configure_initializer first", fn);
    RF_REQUIRE(inc[0] & 1u, "%s: the generator's increment is even", fn);
    RF_HIP(hipSetDevice(ctx->device));
    RF_HIP(hipStreamSynchronize(ctx->stream)); // (the host copies below are what an earlier upload may still read)
    rf::init_jump_table(ctx->env_init_host, rf::U128{inc[0], inc[1]}); // (the jumps' additive parts follow the increment)
    const unsigned long long gen[4] = {state[0], state[1], inc[0], inc[1]};
    memcpy(ctx->env_gen_host, gen, sizeof(gen));
    RF_HIP(hipMemcpyAsync(ctx->d_init, &ctx->env_init_host, sizeof(rf::EnvInit), hipMemcpyHostToDevice, ctx->stream));
    RF_HIP(hipMemcpyAsync(init_gen(ctx), ctx->env_gen_host, sizeof(gen), hipMemcpyHostToDevice, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

int rf_env_get_initializer_state(rf_ctx *ctx, uint64_t state[2], uint64_t inc[2])
{
    const char *fn = "rf_env_get_initializer_state";
    RF_REQUIRE(ctx != nullptr && state != nullptr && inc != nullptr, "%s: NULL argument", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_init, "%s: rf_env_configure_initializer first", fn);
    RF_HIP(hipSetDevice(ctx->device));
    unsigned long long gen[4];
    RF_HIP(hipMemcpyAsync(gen, init_gen(ctx), sizeof(gen), hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    state[0] = gen[0];
    state[1] = gen[1];
    inc[0] = gen[2];
    inc[1] = gen[3];
    return RF_OK;
}

int rf_env_get_strategy_state(rf_ctx *ctx, int32_t *host_counters, float *host_floats, float *host_histories,
                              float *host_old)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_get_strategy_state: ctx is NULL");
    RF_REQUIRE(ctx->env_ready && ctx->env_cfg.task == rf::kEnvTaskComposed,
               "rf_env_get_strategy_state: rf_env_configure_composed first");
    RF_HIP(hipSetDevice(ctx->device));
    const rf_env_program &p = ctx->env_program;
    const size_t n = (size_t)ctx->env_host.n;
    size_t rows = 0;
    for (int i = 0; i < p.n_enders; ++i)
        rows += p.enders[i].kind == RF_ENDER_STOPPED ? (size_t)p.enders[i].steps + 1 : 0;
    const rf::EnvState &s = ctx->env;
    if (host_counters)
        RF_HIP(hipMemcpyAsync(host_counters, s.leaf_count, p.n_enders * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (host_floats)
        RF_HIP(hipMemcpyAsync(host_floats, s.leaf_float, p.n_enders * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (host_histories && rows)
        RF_HIP(hipMemcpyAsync(host_histories, s.history, rows * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (host_old)
        RF_HIP(hipMemcpyAsync(host_old, s.leaf_old, p.n_rewarders * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

int rf_env_reset(rf_ctx *ctx, const float *host_states, float *host_obs)
{
    RF_REQUIRE(ctx != nullptr && host_obs != nullptr, "rf_env_reset: NULL argument");
    RF_REQUIRE(host_states != nullptr || (ctx->env_ready && ctx->env_init), "rf_env_reset: NULL argument");
    RF_REQUIRE(ctx->env_ready, "rf_env_reset: rf_env_configure first");
    RF_HIP(hipSetDevice(ctx->device));
    if (int rc = resolve_device_steps(ctx))
        return rc;
    if (int rc = clear_fault(ctx))
        return rc;
    ctx->env_pending = -1;
    ctx->env_planned = false;
    ctx->env_needs_reset = false;
    ctx->env_step_index = 0;
    const EnvLaunch d(ctx, true);
    if (host_states) {
        RF_HIP(hipMemcpyAsync(ctx->env.state, host_states, (size_t)d.n * 8, hipMemcpyHostToDevice, ctx->stream));
    } else { // initializer.initialize(num_envs): all n rows are the states, and the generator moves past them
        launch_draw_pool(ctx, ctx->env.state, d.n);
        launch_init_advance(ctx, nullptr, d.n);
    }
    if (int rc = full_pass(ctx, d, true, nullptr))
        return rc;
    RF_HIP(hipGetLastError());
    RF_HIP(hipMemcpyAsync(host_obs, ctx->env.obs, env_obs_bytes(ctx), hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->env_scene_len = d.n;
    ctx->env_last_partial = false;
    ctx->env_started = true;
    if (ctx->env_view)
        return enqueue_view(ctx, true, nullptr, nullptr, nullptr);
    return RF_OK;
}

int rf_env_step(rf_ctx *ctx, const int32_t *host_actions, const float *host_pool, float *host_obs,
                double *host_rewards, uint8_t *host_truncated, int *host_n_reset)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step: ctx is NULL");
    RF_HIP(hipSetDevice(ctx->device));
    return env_step(ctx, host_actions, host_pool, host_obs, host_rewards, host_truncated, host_n_reset, "rf_env_step");
}

int rf_env_step_jumps(rf_ctx *ctx, const float *host_actions, const float *host_pool, float *host_obs,
                      double *host_rewards, uint8_t *host_truncated, int *host_n_reset)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step_jumps: ctx is NULL");
    RF_HIP(hipSetDevice(ctx->device));
    return env_step(ctx, host_actions, host_pool, host_obs, host_rewards, host_truncated, host_n_reset,
                    "rf_env_step_jumps");
}

int rf_env_last_step_branch(rf_ctx *ctx, int *branch)
{
    RF_REQUIRE(ctx != nullptr && branch != nullptr, "rf_env_last_step_branch: NULL argument");
    *branch = ctx->env_last_branch;
    return RF_OK;
}

int rf_env_step_begin(rf_ctx *ctx, const int32_t *host_actions, double *host_rewards, uint8_t *host_truncated,
                      int *host_n_reset)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step_begin: ctx is NULL");
    RF_HIP(hipSetDevice(ctx->device));
    return env_step_begin_checked(ctx, host_actions, host_rewards, host_truncated, host_n_reset, "rf_env_step_begin");
}

int rf_env_step_begin_jumps(rf_ctx *ctx, const float *host_actions, double *host_rewards, uint8_t *host_truncated,
                            int *host_n_reset)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step_begin_jumps: ctx is NULL");
    RF_HIP(hipSetDevice(ctx->device));
    return env_step_begin_checked(ctx, host_actions, host_rewards, host_truncated, host_n_reset,
                                  "rf_env_step_begin_jumps");
}

int rf_env_step_end(rf_ctx *ctx, const float *host_pool, float *host_obs)
{
    RF_REQUIRE(ctx != nullptr && host_obs != nullptr, "rf_env_step_end: NULL argument");
    RF_REFUSE_DEVICE_INITIALIZER(ctx, "rf_env_step_end");
    RF_REFUSE_VIEW(ctx, "rf_env_step_end");
    RF_REQUIRE(ctx->env_ready && ctx->env_pending >= 0 && !ctx->env_planned, "rf_env_step_end: rf_env_step_begin first");
    RF_REQUIRE(ctx->env_pending == 0 || host_pool != nullptr, "rf_env_step_end: %d environments ended but host_pool is NULL",
               ctx->env_pending);
    RF_HIP(hipSetDevice(ctx->device));
    const int k = ctx->env_pending;
    ctx->env_pending = -1;
    int rc = env_step_end(ctx, host_pool, nullptr, k, host_obs);
    if (rc == RF_OK)
        finish_step(ctx, k);
    else
        ctx->env_needs_reset = true; // the second half failed part way: only a reset makes the environment usable again
    return rc;
}

int rf_env_step_plan(rf_ctx *ctx, const int32_t *host_actions, int *host_n_reset)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step_plan: ctx is NULL");
    RF_HIP(hipSetDevice(ctx->device));
    return env_step_plan(ctx, host_actions, host_n_reset, "rf_env_step_plan");
}

int rf_env_step_plan_jumps(rf_ctx *ctx, const float *host_actions, int *host_n_reset)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step_plan_jumps: ctx is NULL");
    RF_HIP(hipSetDevice(ctx->device));
    return env_step_plan(ctx, host_actions, host_n_reset, "rf_env_step_plan_jumps");
}

int rf_env_step_run(rf_ctx *ctx, const float *host_pool, float *host_obs, double *host_rewards, uint8_t *host_truncated)
{
    RF_REQUIRE(ctx != nullptr && host_obs && host_rewards && host_truncated, "rf_env_step_run: NULL argument");
    RF_REFUSE_DEVICE_INITIALIZER(ctx, "rf_env_step_run");
    RF_REFUSE_VIEW(ctx, "rf_env_step_run");
    RF_REQUIRE(ctx->env_ready && ctx->env_pending >= 0 && ctx->env_planned, "rf_env_step_run: rf_env_step_plan first");
    RF_REQUIRE(ctx->env_pending == 0 || host_pool != nullptr, "rf_env_step_run: %d environments ended but host_pool is NULL",
               ctx->env_pending);
    RF_HIP(hipSetDevice(ctx->device));
    const int k = ctx->env_pending;
    ctx->env_pending = -1;
    ctx->env_planned = false;
    ctx->env_needs_reset = true; // until the step has finished (a failure below returns early)
    const EnvLaunch d(ctx, false);
    const size_t n = (size_t)d.n;
    if (k > 0)
        RF_HIP(hipMemcpyAsync(ctx->d_pool, host_pool, (size_t)k * 8, hipMemcpyHostToDevice, ctx->stream));
    int rc;
    if (fused_step_possible(ctx)) {
        rc = fused_pass(ctx, d, k > 0 ? rf::kEnvResetPack : kEnvResetNone);
    } else { // (env_pre_kernel's work was rf_env_step_plan's)
        rc = full_pass(ctx, d, false, nullptr);
        if (rc == RF_OK && k > 0)
            rc = reset_pass(ctx, d, k, rf::kEnvResetApply, true);
    }
    if (rc != RF_OK)
        return rc;
    RF_HIP(hipGetLastError());
    RF_HIP(hipMemcpyAsync(host_rewards, ctx->env.reward, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipMemcpyAsync(host_truncated, ctx->env.truncated, n, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipMemcpyAsync(host_obs, ctx->env.obs, env_obs_bytes(ctx), hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    rfh::count_pixels(d.pixels(d.n + k));
    ctx->env_needs_reset = false;
    finish_step(ctx, k);
    return RF_OK;
}

int rf_env_render_states(rf_ctx *ctx, int k, const float *host_states, double *host_focus)
{
    RF_REQUIRE(ctx != nullptr && host_states != nullptr && host_focus != nullptr, "rf_env_render_states: NULL argument");
    RF_REFUSE_DEVICE_INITIALIZER(ctx, "rf_env_render_states");
    RF_REFUSE_VIEW(ctx, "rf_env_render_states");
    RF_REQUIRE(ctx->env_ready, "rf_env_render_states: rf_env_configure first");
    const rf_env_config &h = ctx->env_host;
    RF_REQUIRE(k > 0 && k <= h.n, "rf_env_render_states: k=%d outside [1, %d]", k, h.n);
    RF_HIP(hipSetDevice(ctx->device));
    drop_env_graph(ctx);
    const int fh = h.frame_height;
    RF_HIP(hipMemcpyAsync(ctx->d_pool, host_states, (size_t)k * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(rf::env_pack_rows_kernel, dim3((k + 255) / 256), dim3(256), 0, ctx->stream, ctx->env_cfg, ctx->env,
                       (const float *)ctx->d_pool, k);
    int rc = launch_render(ctx, k, fh, fh, h.spp, ctx->env.cam_dyn2, ctx->env.rect2, ctx->env_axis);
    if (rc == RF_OK)
        rc = launch_focus(ctx, k, fh, fh, h.gray_mode);
    if (rc != RF_OK)
        return rc;
    RF_HIP(hipGetLastError());
    RF_HIP(hipMemcpyAsync(host_focus, ctx->d_var, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->env_scene_len = k; // the renderer now holds this compacted set (what rf_env_render would draw)
    ctx->env_last_partial = true;
    return RF_OK;
}


int rf_env_step_end_given(rf_ctx *ctx, const float *host_pool, const double *host_focus, float *host_obs)
{
    RF_REQUIRE(ctx != nullptr && host_obs != nullptr, "rf_env_step_end_given: NULL argument");
    RF_REFUSE_DEVICE_INITIALIZER(ctx, "rf_env_step_end_given");
    RF_REFUSE_VIEW(ctx, "rf_env_step_end_given");
    RF_REQUIRE(ctx->env_ready && ctx->env_pending >= 0 && !ctx->env_planned, "rf_env_step_end_given: rf_env_step_begin first");
    const int k = ctx->env_pending;
    RF_REQUIRE(k == 0 || (host_pool != nullptr && host_focus != nullptr),
               "rf_env_step_end_given: %d environments ended but host_pool / host_focus is NULL", k);
    RF_REQUIRE(k <= ctx->focus_cap, "rf_env_step_end_given: focus buffer smaller than %d", k); // (before anything changes)
    RF_HIP(hipSetDevice(ctx->device));
    ctx->env_pending = -1;
    ctx->env_needs_reset = true; // until the second half has finished (a HIP failure below returns early)
    if (int rc = env_step_end(ctx, host_pool, host_focus, k, host_obs))
        return rc;
    ctx->env_needs_reset = false;
    ctx->env_steps += 1; // (the renderer's scene set is not this step's: rf_env_render_states says what it holds)
    ctx->env_step_index += 1;
    ctx->env_stepped = true;
    return RF_OK;
}
int rf_env_step_abort(rf_ctx *ctx)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step_abort: ctx is NULL");
    RF_REQUIRE(ctx->env_ready, "rf_env_step_abort: rf_env_configure first");
    if (ctx->env_pending >= 0) {
        // the episode bookkeeping of the environments that ended is half way through a step: only a
        // reset makes the environment usable again, and rf_env_step / _begin say so until then
        ctx->env_pending = -1;
        ctx->env_planned = false;
        ctx->env_needs_reset = true;
    }
    return RF_OK;
}

int rf_env_scene_len(rf_ctx *ctx, int *n_envs)
{
    RF_REQUIRE(ctx != nullptr && n_envs != nullptr, "rf_env_scene_len: NULL argument");
    RF_REQUIRE(ctx->env_ready, "rf_env_scene_len: rf_env_configure first");
    if (ctx->io_unresolved) { // (the last device step's count decides it)
        RF_HIP(hipSetDevice(ctx->device));
        if (int rc = resolve_device_steps(ctx))
            return rc;
    }
    *n_envs = ctx->env_scene_len;
    return RF_OK;
}

int rf_env_render(rf_ctx *ctx, int frame_height, int spp, uint8_t *host_out)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_render: ctx is NULL");
    if (ctx->io_unresolved) { // (which scene set the renderer holds is the last device step's to say)
        RF_HIP(hipSetDevice(ctx->device));
        if (int rc = resolve_device_steps(ctx))
            return rc;
    }
    RF_REQUIRE(ctx->env_ready && ctx->env_scene_len > 0, "rf_env_render: rf_env_reset first");
    RF_REQUIRE(ctx->env_pending < 0, "rf_env_render: a two-phase step is open (rf_env_step_end first)");
    RF_REQUIRE(frame_height > 0 && spp > 0, "rf_env_render: frame_height, spp must be positive");
    const int n = ctx->env_scene_len;
    const uint64_t need = (uint64_t)n * frame_height * frame_height;
    RF_REQUIRE(need <= ctx->n_states, "rf_env_render: %llu pixels but only %llu RNG states (rf_seed first)",
               (unsigned long long)need, (unsigned long long)ctx->n_states);
    RF_HIP(hipSetDevice(ctx->device));
    drop_env_graph(ctx);
    const bool partial = ctx->env_last_partial;
    int rc = launch_render(ctx, n, frame_height, frame_height, spp, partial ? ctx->env.cam_dyn2 : ctx->env.cam_dyn,
                           partial ? ctx->env.rect2 : ctx->env.rect, ctx->env_axis);
    if (rc != RF_OK)
        return rc;
    if (host_out)
        return rf_get_frames(ctx, 0, n, host_out);
    return RF_OK;
}

int rf_env_get_counters(rf_ctx *ctx, int32_t *host_steps, int32_t *host_diverging)
{
    RF_REQUIRE(ctx != nullptr && host_steps != nullptr && host_diverging != nullptr, "rf_env_get_counters: NULL argument");
    RF_REQUIRE(ctx->env_ready, "rf_env_get_counters: rf_env_configure first");
    RF_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->env_host.n * 4;
    RF_HIP(hipMemcpyAsync(host_steps, ctx->env.steps, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipMemcpyAsync(host_diverging, ctx->env.diverging, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

int rf_env_get_states(rf_ctx *ctx, float *host_states)
{
    RF_REQUIRE(ctx != nullptr && host_states != nullptr, "rf_env_get_states: NULL argument");
    RF_REQUIRE(ctx->env_ready, "rf_env_get_states: rf_env_configure first");
    RF_HIP(hipSetDevice(ctx->device));
    RF_HIP(hipMemcpyAsync(host_states, ctx->env.state, (size_t)ctx->env_host.n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

int rf_env_step_device(rf_ctx *ctx, const void *d_actions, int action_dtype, float *d_obs, double *d_rewards,
                       uint8_t *d_truncated, int32_t *d_n_reset, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step_device: NULL argument");
    RF_HIP(hipSetDevice(ctx->device));
    return env_step_device(ctx, d_actions, action_dtype, d_obs, d_rewards, d_truncated, d_n_reset, nullptr, nullptr, nullptr,
                           nullptr, nullptr, nullptr, caller_stream, "rf_env_step_device");
}

int rf_env_step_device_records(rf_ctx *ctx, const void *d_actions, int action_dtype, float *d_obs, double *d_rewards,
                               uint8_t *d_truncated, int32_t *d_n_reset, float *d_final_obs, double *d_returns,
                               int32_t *d_lengths, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step_device_records: NULL argument");
    RF_HIP(hipSetDevice(ctx->device));
    return env_step_device(ctx, d_actions, action_dtype, d_obs, d_rewards, d_truncated, d_n_reset, d_final_obs, d_returns,
                           d_lengths, nullptr, nullptr, nullptr, caller_stream, "rf_env_step_device_records");
}

int rf_env_step_device_view(rf_ctx *ctx, const void *d_actions, int action_dtype, float *d_obs, double *d_rewards,
                            uint8_t *d_truncated, int32_t *d_n_reset, float *d_final_obs, double *d_returns,
                            int32_t *d_lengths, float *d_view_obs, double *d_view_rewards, float *d_view_final,
                            void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_step_device_view: NULL argument");
    RF_HIP(hipSetDevice(ctx->device));
    return env_step_device(ctx, d_actions, action_dtype, d_obs, d_rewards, d_truncated, d_n_reset, d_final_obs, d_returns,
                           d_lengths, d_view_obs, d_view_rewards, d_view_final, caller_stream, "rf_env_step_device_view");
}

int rf_env_configure_records(rf_ctx *ctx, int on)
{
    const char *fn = "rf_env_configure_records";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready, "%s: rf_env_configure first", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase or planned step is open", fn);
    RF_REQUIRE(!ctx->env_stepped, "%s: the context has stepped (episode records are chosen before the first reset)", fn);
    RF_HIP(hipSetDevice(ctx->device));
    if (on != 0 && ctx->h_records_bytes < ctx->env_rec_bytes) { // (rf_env_get_records' pinned block; before anything changes)
        RF_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->h_records)
            RF_HIP(hipHostFree(ctx->h_records));
        ctx->h_records = nullptr;
        ctx->h_records_bytes = 0;
        RF_HIP(host_malloc((void **)&ctx->h_records, ctx->env_rec_bytes));
        ctx->h_records_bytes = ctx->env_rec_bytes;
    }
    drop_env_graph(ctx); // (a captured step holds EnvState by value)
    drop_env_snapshots(ctx); // (their layout is the other setting's)
    if (int rc = drop_view(ctx)) // (a view is configured after the records it reads: view_final exists with them only)
        return rc;
    rf::EnvState &s = ctx->env;
    char *base = (char *)ctx->env_block;
    const bool records = on != 0;
    s.ep_return = records ? (double *)(base + ctx->env_rec_off[0]) : nullptr;
    s.ep_length = records ? (int *)(base + ctx->env_rec_off[1]) : nullptr;
    s.final_obs = records ? (float *)(base + ctx->env_rec_off[2]) : nullptr;
    s.final_return = records ? (double *)(base + ctx->env_rec_off[3]) : nullptr;
    s.final_length = records ? (int *)(base + ctx->env_rec_off[4]) : nullptr;
    if (records) { // (a context that was reset already starts its episodes' accumulators here)
        const size_t n = (size_t)ctx->env_host.n;
        RF_HIP(hipMemsetAsync(s.ep_return, 0, n * 8, ctx->stream));
        RF_HIP(hipMemsetAsync(s.ep_length, 0, n * 4, ctx->stream));
    }
    ctx->env_records = records;
    return RF_OK;
}

int rf_env_get_records(rf_ctx *ctx, float *host_final_obs, double *host_returns, int32_t *host_lengths)
{
    const char *fn = "rf_env_get_records";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_records, "%s: the context keeps no episode records (rf_env_configure_records)", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase or planned step is open", fn);
    RF_REQUIRE(ctx->env_started && ctx->env_step_index > 0, "%s: no step since the last reset", fn);
    RF_HIP(hipSetDevice(ctx->device));
    // one copy of the piece [final_return | final_obs | final_length] into the pinned block, one synchronisation
    const size_t n = (size_t)ctx->env_host.n, obs_bytes = env_obs_bytes(ctx);
    RF_HIP(hipMemcpyAsync(ctx->h_records, ctx->env.final_return, ctx->env_rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    if (host_returns)
        memcpy(host_returns, ctx->h_records, n * 8);
    if (host_final_obs)
        memcpy(host_final_obs, ctx->h_records + n * 8, obs_bytes);
    if (host_lengths)
        memcpy(host_lengths, ctx->h_records + n * 8 + obs_bytes, n * 4);
    return RF_OK;
}

int rf_env_get_record_accumulators(rf_ctx *ctx, double *host_returns, int32_t *host_lengths)
{
    const char *fn = "rf_env_get_record_accumulators";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_records, "%s: the context keeps no episode records (rf_env_configure_records)", fn);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->env_host.n;
    if (host_returns)
        RF_HIP(hipMemcpyAsync(host_returns, ctx->env.ep_return, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (host_lengths)
        RF_HIP(hipMemcpyAsync(host_lengths, ctx->env.ep_length, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

int rf_env_reset_device(rf_ctx *ctx, float *d_obs, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_reset_device: NULL argument");
    RF_HIP(hipSetDevice(ctx->device));
    return env_reset_device(ctx, d_obs, nullptr, caller_stream, "rf_env_reset_device");
}

int rf_env_reset_device_view(rf_ctx *ctx, float *d_obs, float *d_view_obs, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "rf_env_reset_device_view: NULL argument");
    RF_HIP(hipSetDevice(ctx->device));
    return env_reset_device(ctx, d_obs, d_view_obs, caller_stream, "rf_env_reset_device_view");
}

// ---- the learner view's entry points (include/reinfocus_hip.h, "learner view") -----------------------------------------
// rf_env_configure_view (groups = 0) and rf_env_configure_view_grouped (groups >= 1; gammas: host double[groups], or
// NULL for cfg->gamma everywhere)
static int configure_view(rf_ctx *ctx, const rf_env_view_config *cfg, int groups, const double *gammas, const char *fn)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready, "%s: rf_env_configure first", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase or planned step is open", fn);
    RF_REQUIRE(!ctx->env_stepped, "%s: the context has stepped (a learner view is chosen before the first reset)", fn);
    if (cfg) {
        RF_REQUIRE(cfg->frame_stack >= 1 && cfg->frame_stack <= 8, "%s: frame_stack %d outside 1 to 8", fn, cfg->frame_stack);
        RF_REQUIRE(isfinite(cfg->epsilon) && cfg->epsilon > 0.0, "%s: epsilon %g is not finite and positive", fn, cfg->epsilon);
        RF_REQUIRE(isfinite(cfg->clip_obs) && cfg->clip_obs > 0.0, "%s: clip_obs %g is not finite and positive", fn,
                   cfg->clip_obs);
        RF_REQUIRE(isfinite(cfg->clip_reward) && cfg->clip_reward > 0.0, "%s: clip_reward %g is not finite and positive", fn,
                   cfg->clip_reward);
        RF_REQUIRE(cfg->gamma >= 0.0 && cfg->gamma <= 1.0, "%s: gamma %g outside [0, 1]", fn, cfg->gamma); // (false for NaN)
        RF_REQUIRE(ctx->env_obs_width <= rf::kViewMaxColumns, "%s: %d observation columns (at most %d)", fn,
                   ctx->env_obs_width, rf::kViewMaxColumns);
        RF_REQUIRE((long long)ctx->env_host.n * ctx->env_obs_width * cfg->frame_stack < (1ll << 31),
                   "%s: %d environments x %d columns x %d frames do not fit a 32-bit index", fn, ctx->env_host.n,
                   ctx->env_obs_width, cfg->frame_stack);
        if (groups) {
            RF_REQUIRE(groups >= 1 && groups <= RF_POPULATION_MAX_GROUPS, "%s: groups %d outside 1 to %d", fn, groups,
                       RF_POPULATION_MAX_GROUPS);
            RF_REQUIRE(ctx->env_host.n % groups == 0, "%s: %d groups do not divide %d environments", fn, groups,
                       ctx->env_host.n);
            for (int g = 0; gammas && g < groups; ++g)
                RF_REQUIRE(gammas[g] >= 0.0 && gammas[g] <= 1.0, "%s: gamma %g of group %d outside [0, 1]", fn, gammas[g], g);
        }
    }
    RF_HIP(hipSetDevice(ctx->device));
    drop_env_snapshots(ctx); // (their layout is the other setting's)
    if (int rc = drop_view(ctx))
        return rc;
    if (!cfg)
        return RF_OK;
    const size_t n = (size_t)ctx->env_host.n, width = (size_t)ctx->env_obs_width, cells = n * width * (size_t)cfg->frame_stack;
    const bool records = ctx->env_records;
    // [view_reward | stack | view_final]: the piece rf_env_get_view copies; then the returns and the moments (grouped:
    // one EnvViewMoments per group, then the groups' gammas)
    const size_t sets = groups ? (size_t)groups : 1;
    const size_t out_bytes = n * 8 + cells * 4 + (records ? cells * 4 : 0);
    const size_t o_returns = (out_bytes + 255) & ~(size_t)255, o_moments = (o_returns + n * 8 + 255) & ~(size_t)255;
    const size_t o_gammas = (o_moments + sets * sizeof(rf::EnvViewMoments) + 255) & ~(size_t)255;
    const size_t bytes = groups ? o_gammas + sets * 8 : o_moments + sizeof(rf::EnvViewMoments);
    if (ctx->h_view_bytes < out_bytes) { // (rf_env_get_view's pinned block; before anything changes)
        RF_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->h_view)
            RF_HIP(hipHostFree(ctx->h_view));
        ctx->h_view = nullptr;
        ctx->h_view_bytes = 0;
        RF_HIP(host_malloc((void **)&ctx->h_view, out_bytes));
        ctx->h_view_bytes = out_bytes;
    }
    RF_HIP(dev_malloc(&ctx->view_block, bytes));
    RF_HIP(hipMemsetAsync(ctx->view_block, 0, bytes, ctx->stream));
    char *base = (char *)ctx->view_block;
    ctx->view_reward = (double *)base;
    ctx->view_stack = (float *)(base + n * 8);
    ctx->view_final = records ? (float *)(base + n * 8 + cells * 4) : nullptr;
    ctx->view_returns = (double *)(base + o_returns);
    ctx->view_moments = (rf::EnvViewMoments *)(base + o_moments);
    ctx->view_out_bytes = out_bytes;
    rf::EnvViewMoments &m = ctx->view_moments_host;
    for (int i = 0; i < rf::kViewSlots; ++i) { // RunningMeanStd(): mean 0, var 1, count 1e-4 (the slots past W stay so)
        m.mean[i] = 0.0;
        m.var[i] = 1.0;
        m.count[i] = 1e-4;
    }
    if (groups) {
        ctx->view_moments_groups.assign(sets, m);
        ctx->view_gammas.assign(sets, cfg->gamma);
        if (gammas)
            ctx->view_gammas.assign(gammas, gammas + sets);
        RF_HIP(hipMemcpyAsync(ctx->view_moments, ctx->view_moments_groups.data(), sets * sizeof(m), hipMemcpyHostToDevice,
                              ctx->stream));
        RF_HIP(hipMemcpyAsync(base + o_gammas, ctx->view_gammas.data(), sets * 8, hipMemcpyHostToDevice, ctx->stream));
    } else {
        RF_HIP(hipMemcpyAsync(ctx->view_moments, &m, sizeof(m), hipMemcpyHostToDevice, ctx->stream));
    }
    RF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->view_host = *cfg;
    ctx->view_host.norm_obs = cfg->norm_obs != 0;
    ctx->view_host.norm_reward = cfg->norm_reward != 0;
    ctx->view_host.training = cfg->training != 0;
    ctx->view_cfg = rf::EnvViewConfig{ctx->env_host.n, ctx->env_obs_width, cfg->frame_stack, cfg->norm_obs != 0,
                                      cfg->norm_reward != 0, cfg->gamma, cfg->epsilon, cfg->clip_obs, cfg->clip_reward};
    ctx->view_groups = groups;
    if (groups) {
        const int m_lanes = ctx->env_host.n / groups;
        int log2_pm = 0;
        while ((1ll << log2_pm) < m_lanes)
            ++log2_pm;
        ctx->view_grp = rf::EnvViewGroups{groups, m_lanes, log2_pm, (const double *)(base + o_gammas)};
    }
    ctx->view_training = cfg->training != 0;
    ctx->view_after_step = false;
    ctx->env_view = true;
    return RF_OK;
}

int rf_env_configure_view(rf_ctx *ctx, const rf_env_view_config *cfg)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_env_configure_view");
    RF_HIP(hipSetDevice(ctx->device));
    return configure_view(ctx, cfg, 0, nullptr, "rf_env_configure_view");
}

int rf_env_configure_view_grouped(rf_ctx *ctx, const rf_env_view_config *cfg, int groups, const double *gammas)
{
    const char *fn = "rf_env_configure_view_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_HIP(hipSetDevice(ctx->device));
    RF_REQUIRE(cfg != nullptr, "%s: cfg is NULL (rf_env_configure_view(ctx, NULL) turns a view off)", fn);
    RF_REQUIRE(groups >= 1 && groups <= RF_POPULATION_MAX_GROUPS, "%s: groups %d outside 1 to %d", fn, groups,
               RF_POPULATION_MAX_GROUPS);
    return configure_view(ctx, cfg, groups, gammas, fn);
}

int rf_env_get_view(rf_ctx *ctx, float *host_obs, double *host_rewards, float *host_final)
{
    const char *fn = "rf_env_get_view";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_view, "%s: the context has no learner view (rf_env_configure_view)", fn);
    RF_REQUIRE(ctx->env_started, "%s: rf_env_reset first", fn);
    RF_REQUIRE(ctx->view_final || !host_final, "%s: host_final needs episode records (rf_env_configure_records before "
               "rf_env_configure_view)", fn);
    RF_REQUIRE(ctx->view_after_step || !(host_rewards || host_final), "%s: no step since the last reset (only host_obs)", fn);
    RF_HIP(hipSetDevice(ctx->device));
    // one copy of the piece [view_reward | stack | view_final] into the pinned block, one synchronisation
    const size_t n = (size_t)ctx->env_host.n, cells_bytes = env_obs_bytes(ctx) * (size_t)ctx->view_cfg.frame_stack;
    const size_t wanted = host_final ? ctx->view_out_bytes : n * 8 + cells_bytes;
    RF_HIP(hipMemcpyAsync(ctx->h_view, ctx->view_reward, wanted, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    if (host_rewards)
        memcpy(host_rewards, ctx->h_view, n * 8);
    if (host_obs)
        memcpy(host_obs, ctx->h_view + n * 8, cells_bytes);
    if (host_final)
        memcpy(host_final, ctx->h_view + n * 8 + cells_bytes, cells_bytes);
    return RF_OK;
}

int rf_env_view_get_statistics(rf_ctx *ctx, double *mean, double *var, double *count)
{
    const char *fn = "rf_env_view_get_statistics";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_view, "%s: the context has no learner view (rf_env_configure_view)", fn);
    RF_REQUIRE(ctx->view_groups == 0, "%s: the learner view is grouped (rf_env_view_get_statistics_grouped)", fn);
    RF_HIP(hipSetDevice(ctx->device));
    rf::EnvViewMoments m;
    RF_HIP(hipMemcpyAsync(&m, ctx->view_moments, sizeof(m), hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    const size_t bytes = ((size_t)ctx->env_obs_width + 1) * sizeof(double);
    if (mean)
        memcpy(mean, m.mean, bytes);
    if (var)
        memcpy(var, m.var, bytes);
    if (count)
        memcpy(count, m.count, bytes);
    return RF_OK;
}

int rf_env_view_set_statistics(rf_ctx *ctx, const double *mean, const double *var, const double *count)
{
    const char *fn = "rf_env_view_set_statistics";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_view, "%s: the context has no learner view (rf_env_configure_view)", fn);
    RF_REQUIRE(ctx->view_groups == 0, "%s: the learner view is grouped (rf_env_view_set_statistics_grouped)", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase or planned step is open", fn);
    RF_HIP(hipSetDevice(ctx->device));
    rf::EnvViewMoments &m = ctx->view_moments_host;
    RF_HIP(hipMemcpyAsync(&m, ctx->view_moments, sizeof(m), hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    const size_t bytes = ((size_t)ctx->env_obs_width + 1) * sizeof(double);
    if (mean)
        memcpy(m.mean, mean, bytes);
    if (var)
        memcpy(m.var, var, bytes);
    if (count)
        memcpy(m.count, count, bytes);
    RF_HIP(hipMemcpyAsync(ctx->view_moments, &m, sizeof(m), hipMemcpyHostToDevice, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

// float64 [G][W + 1] each, the returns last; each pointer may be NULL.  Synchronous.
int rf_env_view_get_statistics_grouped(rf_ctx *ctx, double *mean, double *var, double *count)
{
    const char *fn = "rf_env_view_get_statistics_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_view, "%s: the context has no learner view (rf_env_configure_view)", fn);
    RF_REQUIRE(ctx->view_groups > 0, "%s: the learner view is not grouped (rf_env_configure_view_grouped)", fn);
    RF_HIP(hipSetDevice(ctx->device));
    std::vector<rf::EnvViewMoments> sets((size_t)ctx->view_groups);
    RF_HIP(hipMemcpyAsync(sets.data(), ctx->view_moments, sets.size() * sizeof(rf::EnvViewMoments), hipMemcpyDeviceToHost,
                          ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    const size_t row = (size_t)ctx->env_obs_width + 1;
    for (size_t g = 0; g < sets.size(); ++g) {
        if (mean)
            memcpy(mean + g * row, sets[g].mean, row * sizeof(double));
        if (var)
            memcpy(var + g * row, sets[g].var, row * sizeof(double));
        if (count)
            memcpy(count + g * row, sets[g].count, row * sizeof(double));
    }
    return RF_OK;
}

int rf_env_view_set_statistics_grouped(rf_ctx *ctx, const double *mean, const double *var, const double *count)
{
    const char *fn = "rf_env_view_set_statistics_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_view, "%s: the context has no learner view (rf_env_configure_view)", fn);
    RF_REQUIRE(ctx->view_groups > 0, "%s: the learner view is not grouped (rf_env_configure_view_grouped)", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase or planned step is open", fn);
    RF_HIP(hipSetDevice(ctx->device));
    std::vector<rf::EnvViewMoments> &sets = ctx->view_moments_groups;
    sets.resize((size_t)ctx->view_groups);
    RF_HIP(hipMemcpyAsync(sets.data(), ctx->view_moments, sets.size() * sizeof(rf::EnvViewMoments), hipMemcpyDeviceToHost,
                          ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    const size_t row = (size_t)ctx->env_obs_width + 1;
    for (size_t g = 0; g < sets.size(); ++g) {
        if (mean)
            memcpy(sets[g].mean, mean + g * row, row * sizeof(double));
        if (var)
            memcpy(sets[g].var, var + g * row, row * sizeof(double));
        if (count)
            memcpy(sets[g].count, count + g * row, row * sizeof(double));
    }
    RF_HIP(hipMemcpyAsync(ctx->view_moments, sets.data(), sets.size() * sizeof(rf::EnvViewMoments), hipMemcpyHostToDevice,
                          ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

int rf_env_view_set_training(rf_ctx *ctx, int training)
{
    const char *fn = "rf_env_view_set_training";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_view, "%s: the context has no learner view (rf_env_configure_view)", fn);
    RF_HIP(hipSetDevice(ctx->device)); // (nothing is enqueued: the flag decides what the next step launches)
    ctx->view_training = training != 0;
    return RF_OK;
}

int rf_env_view_get_state(rf_ctx *ctx, float *host_stack, double *host_returns)
{
    const char *fn = "rf_env_view_get_state";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(ctx->env_ready && ctx->env_view, "%s: the context has no learner view (rf_env_configure_view)", fn);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->env_host.n;
    if (host_stack)
        RF_HIP(hipMemcpyAsync(host_stack, ctx->view_stack, env_obs_bytes(ctx) * (size_t)ctx->view_cfg.frame_stack,
                              hipMemcpyDeviceToHost, ctx->stream));
    if (host_returns)
        RF_HIP(hipMemcpyAsync(host_returns, ctx->view_returns, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

int rf_env_device_status(rf_ctx *ctx, int *fault_step, int *fault_env)
{
    const char *fn = "rf_env_device_status";
    RF_REQUIRE(ctx != nullptr && fault_step != nullptr && fault_env != nullptr, "%s: NULL argument", fn);
    RF_REQUIRE(ctx->env_ready, "%s: rf_env_configure first", fn);
    RF_HIP(hipSetDevice(ctx->device));
    if (int rc = resolve_device_steps(ctx))
        return rc;
    RF_HIP(hipStreamSynchronize(ctx->stream));
    *fault_step = ctx->env_fault_step;
    *fault_env = ctx->env_fault_env;
    return RF_OK;
}

// ---- the learner entry points: every array is the caller's, checked by check_device_arrays (rf_host.h) -------------------
// What they say of a desc, or of a population's shape, that they refuse (RF_LSTM_LIMITS: rf_host.h)
#define RF_POLICY_LIMITS "%s: the desc is outside the limits (obs_width 1 .. %d, 1 or 2 hidden layers of width 1 .. %d per " \
                         "net, n_actions 2 .. %d, activation RF_POLICY_RELU or RF_POLICY_TANH)"
#define RF_SDE_LIMITS "%s: the desc is outside the limits (obs_width 1 .. %d, 1 or 2 hidden layers of width 1 .. %d per net, " \
                      "n_actions 1: the Gaussian head has one action, activation RF_POLICY_RELU or RF_POLICY_TANH)"
#define RF_LSTM_SDE_LIMITS "%s: the desc is outside the limits (obs_width and lstm_hidden 1 .. %d, 1 or 2 hidden layers of " \
                           "width 1 .. %d per net, n_actions 1: the Gaussian head has one action, activation RF_POLICY_RELU " \
                           "or RF_POLICY_TANH, critic RF_LSTM_CRITIC_LSTM or RF_LSTM_CRITIC_LINEAR)"
#define RF_POPULATION_LIMITS "%s: G = %d must be in 1 .. %d, m = %d in 1 .. 2^20 and G m at most 2^30"

// rf_rollout_advantages (groups = 0: the scalars) and rf_rollout_advantages_grouped (groups >= 1: d_discounts)
static int rollout_advantages(rf_ctx *ctx, int T, int n, int groups, const double *d_rewards, const float *d_values,
                              const uint8_t *d_truncated, const float *d_final_values, const float *d_last_values,
                              double gamma, double gae_lambda, const float *d_discounts, float *d_advantages,
                              float *d_returns, void *caller_stream, const char *fn)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(d_rewards && d_values && d_truncated && d_last_values && d_advantages && d_returns &&
                   (groups == 0 || d_discounts),
               "%s: NULL argument", fn);
    RF_REQUIRE(T >= 1 && n >= 1, "%s: T = %d and n = %d must both be at least 1", fn, T, n);
    if (groups) {
        RF_REQUIRE(groups >= 1 && groups <= RF_POPULATION_MAX_GROUPS, "%s: groups %d outside 1 to %d", fn, groups,
                   RF_POPULATION_MAX_GROUPS);
        RF_REQUIRE(n % groups == 0, "%s: %d groups do not divide %d environments", fn, groups, n);
    }
    RF_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)T * (size_t)n;
    const DeviceArray inputs[] = {{d_rewards, cells * 8, 8, "d_rewards"},
                                  {d_values, cells * 4, 4, "d_values"},
                                  {d_truncated, cells, 1, "d_truncated"},
                                  {d_final_values, cells * 4, 4, "d_final_values"},
                                  {d_last_values, (size_t)n * 4, 4, "d_last_values"},
                                  {groups ? d_discounts : nullptr, (size_t)groups * 8, 8, "d_discounts"}};
    const DeviceArray outputs[] = {{d_advantages, cells * 4, 4, "d_advantages"}, {d_returns, cells * 4, 4, "d_returns"}};
    // (null inputs: d_final_values without a bootstrap, d_discounts with the scalars)
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn, kNotAmongOutputs,
                                     "the chain writes a step before the steps before it are read"))
        return rc;
    RF_REQUIRE(!ranges_overlap(d_advantages, cells * 4, d_returns, cells * 4), "%s: d_advantages overlaps d_returns", fn);
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // every array is the caller's, so the launch goes to the caller's stream: no event hand-over, nothing waited for
    const float g = (float)gamma, gl = (float)(gamma * gae_lambda); // (the product in float64 first, as numpy takes it)
    const unsigned blocks = (unsigned)(((size_t)n + rf::kRolloutTile - 1) / rf::kRolloutTile);
    if (groups)
        hipLaunchKernelGGL(rf::rollout_gae_kernel<true>, dim3(blocks), dim3(rf::kRolloutThreads), 0, caller, T, n, d_rewards,
                           d_values, d_truncated, d_final_values, d_last_values, 0.0f, 0.0f, d_advantages, d_returns,
                           (const float2 *)d_discounts, n / groups);
    else
        hipLaunchKernelGGL(rf::rollout_gae_kernel<false>, dim3(blocks), dim3(rf::kRolloutThreads), 0, caller, T, n, d_rewards,
                           d_values, d_truncated, d_final_values, d_last_values, g, gl, d_advantages, d_returns,
                           (const float2 *)nullptr, 0);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_rollout_advantages(rf_ctx *ctx, int T, int n, const double *d_rewards, const float *d_values,
                          const uint8_t *d_truncated, const float *d_final_values, const float *d_last_values, double gamma,
                          double gae_lambda, float *d_advantages, float *d_returns, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_rollout_advantages");
    RF_HIP(hipSetDevice(ctx->device));
    return rollout_advantages(ctx, T, n, 0, d_rewards, d_values, d_truncated, d_final_values, d_last_values, gamma,
                              gae_lambda, nullptr, d_advantages, d_returns, caller_stream, "rf_rollout_advantages");
}

int rf_rollout_advantages_grouped(rf_ctx *ctx, int T, int n, int groups, const double *d_rewards, const float *d_values,
                                  const uint8_t *d_truncated, const float *d_final_values, const float *d_last_values,
                                  const float *d_discounts, float *d_advantages, float *d_returns, void *caller_stream)
{
    const char *fn = "rf_rollout_advantages_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_HIP(hipSetDevice(ctx->device));
    RF_REQUIRE(groups >= 1 && groups <= RF_POPULATION_MAX_GROUPS, "%s: groups %d outside 1 to %d", fn, groups,
               RF_POPULATION_MAX_GROUPS);
    return rollout_advantages(ctx, T, n, groups, d_rewards, d_values, d_truncated, d_final_values, d_last_values, 0.0, 0.0,
                              d_discounts, d_advantages, d_returns, caller_stream, fn);
}

unsigned long long rf_policy_params_size(rf_ctx *ctx, const rf_policy_desc *desc)
{
    rf::PolicyLayout layout;
    if (ctx == nullptr || desc == nullptr || !rf::policy_layout(*desc, layout))
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return layout.total;
}

// rf_policy_forward (G = 0: n rows, gen the host's four words) and rf_policy_forward_grouped (G >= 1: m rows per group, gen
// the groups' generators on the device) are one function in two parts, between which each makes the device current: what
// a call may ask for (sampled: whether it draws) ...
static int policy_forward_asks(const char *fn, int G, const float *d_final_obs, const unsigned long long *gen, int flags,
                               const long long *d_actions, const float *d_log_probs, const float *d_values,
                               const float *d_final_values, const float *d_logits, bool &sampled)
{
    RF_REQUIRE((flags & ~RF_POLICY_DETERMINISTIC) == 0, "%s: unknown flags %d", fn, flags);
    RF_REQUIRE(d_actions || d_values || d_final_values || d_logits, "%s: no output is asked for", fn);
    RF_REQUIRE(d_log_probs == nullptr || d_actions != nullptr, "%s: d_log_probs are those of d_actions, which is NULL", fn);
    RF_REQUIRE(d_final_values == nullptr || d_final_obs != nullptr, "%s: d_final_values needs d_final_obs", fn);
    sampled = d_actions != nullptr && (flags & RF_POLICY_DETERMINISTIC) == 0;
    RF_REQUIRE(!sampled || gen != nullptr, "%s: a sampled call needs %s", fn, G ? "d_gens" : "gen");
    return RF_OK;
}

// ... and its arrays, their check and the launch
static int policy_forward_any(const char *fn, rf_ctx *ctx, const rf::PolicyLayout &layout, int G, int m, const float *d_params,
                              const float *d_obs, const float *d_final_obs, const unsigned long long *gen,
                              unsigned long long consumed, bool sampled, long long *d_actions, float *d_log_probs,
                              float *d_values, float *d_final_values, float *d_logits, void *caller_stream)
{
    static_assert(sizeof(rf::PolicyGen) == 32, "d_gens is uint64 [G][4]");
    const rf::PolicyGen *d_gens = (const rf::PolicyGen *)(G && sampled ? gen : nullptr);
    const size_t groups = G ? (size_t)G : 1, rows = groups * (size_t)m;
    const DeviceArray inputs[] = {{d_params, groups * (size_t)layout.total * 4, 4, "d_params"},
                                  {d_obs, rows * (size_t)layout.obs_width * 4, 4, "d_obs"},
                                  {d_final_obs, rows * (size_t)layout.obs_width * 4, 4, "d_final_obs"},
                                  {d_gens, groups * 32, 8, "d_gens"}};
    const DeviceArray outputs[] = {{d_actions, rows * 8, 8, "d_actions"},
                                   {d_log_probs, rows * 4, 4, "d_log_probs"},
                                   {d_values, rows * 4, 4, "d_values"},
                                   {d_final_values, rows * 4, 4, "d_final_values"},
                                   {d_logits, rows * (size_t)layout.n_actions * 4, 4, "d_logits"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    // Every array is the caller's; gen is read here, by value, or on the device with the draw count by value: one launch on
    // the caller's stream, nothing allocated, nothing waited for (a caller may capture it; a replay then repeats the same
    // draws).
    rf::PolicyGen words{};
    if (sampled && !G)
        for (int i = 0; i < 4; ++i)
            words.word[i] = gen[i];
    const bool pi = d_actions != nullptr || d_logits != nullptr, vf = d_values != nullptr || d_final_values != nullptr;
    const unsigned tiles = (unsigned)(((size_t)m + rf::kPolicyTile - 1) / rf::kPolicyTile);
    hipLaunchKernelGGL(G ? rf::policy_forward_kernel<true> : rf::policy_forward_kernel<false>,
                       dim3(tiles, pi && vf ? 2u : 1u, (unsigned)groups), dim3(rf::kPolicyThreads), 0,
                       (hipStream_t)caller_stream, layout, d_params, m, d_obs, d_final_obs, words, sampled ? 1 : 0,
                       pi ? 0 : 1, (int64_t *)d_actions, d_log_probs, d_values, d_final_values, d_logits, d_gens,
                       (uint64_t)consumed);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_policy_forward(rf_ctx *ctx, const rf_policy_desc *desc, const float *d_params, int n, const float *d_obs,
                      const float *d_final_obs, const unsigned long long gen[4], int flags, long long *d_actions,
                      float *d_log_probs, float *d_values, float *d_final_values, float *d_logits, void *caller_stream)
{
    const char *fn = "rf_policy_forward";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_obs != nullptr, "%s: NULL argument", fn);
    rf::PolicyLayout layout;
    RF_REQUIRE(rf::policy_layout(*desc, layout), RF_POLICY_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH,
               RF_POLICY_MAX_ACTIONS);
    RF_REQUIRE(n >= 1 && n <= (1 << 30), "%s: n = %d must be at least 1 (and at most 2^30)", fn, n);
    bool sampled;
    if (int rc = policy_forward_asks(fn, 0, d_final_obs, gen, flags, d_actions, d_log_probs, d_values, d_final_values, d_logits,
                                     sampled))
        return rc;
    RF_HIP(hipSetDevice(ctx->device));
    return policy_forward_any(fn, ctx, layout, 0, n, d_params, d_obs, d_final_obs, gen, 0, sampled, d_actions, d_log_probs,
                              d_values, d_final_values, d_logits, caller_stream);
}

unsigned long long rf_ppo_state_size(rf_ctx *ctx, const rf_policy_desc *policy)
{
    rf::PolicyLayout layout;
    if (ctx == nullptr || policy == nullptr || !rf::policy_layout(*policy, layout))
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return 4ull * rf::kPpoStateHeader + 8ull * layout.total;
}

unsigned long long rf_ppo_workspace_size(rf_ctx *ctx, const rf_policy_desc *policy, int max_batch)
{
    rf::PolicyLayout layout;
    rf::PpoWork work;
    if (ctx == nullptr || policy == nullptr || !rf::policy_layout(*policy, layout) || !rf::ppo_work(layout, max_batch, work))
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return 4ull * work.total;
}

// What rf_ppo_update and rf_sde_update do once they have checked ctx and made its device current: one body, the head
// chosen by `sde` (the layout, the dtype of the actions, the kernel)
static int ppo_update_any(const char *fn, bool sde, rf_ctx *ctx, const rf_policy_desc *policy, const rf_ppo_desc *ppo,
                          float *d_params, void *d_state, void *d_workspace, int N, const float *d_obs, const void *d_actions,
                          const float *d_old_log_probs, const float *d_advantages, const float *d_returns, int B,
                          const long long *d_index, float *d_stats, void *caller_stream)
{
    RF_REQUIRE(policy && ppo && d_params && d_state && d_workspace && d_obs && d_actions && d_old_log_probs && d_advantages
               && d_returns && d_index && d_stats, "%s: NULL argument", fn);
    rf::PolicyLayout layout;
    if (sde) {
        RF_REQUIRE(rf::sde_layout(*policy, layout), RF_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH);
    } else {
        RF_REQUIRE(rf::policy_layout(*policy, layout), RF_POLICY_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH,
                   RF_POLICY_MAX_ACTIONS);
    }
    RF_REQUIRE(N >= 1 && N <= (1 << 30), "%s: N = %d must be at least 1 (and at most 2^30)", fn, N);
    RF_REQUIRE(B >= 1 && B <= RF_PPO_MAX_BATCH, "%s: B = %d is not in 1 .. %d", fn, B, RF_PPO_MAX_BATCH);
    rf::PpoHyper hyper;
    RF_REQUIRE(rf::ppo_hyper(*ppo, hyper), "%s: a hyper-parameter is negative or not finite, a beta is outside [0, 1) or "
               "normalize_advantage is not 0 / 1", fn);
    rf::PpoWork work;
    RF_REQUIRE(rf::ppo_work(layout, B, work), "%s: no workspace layout for B = %d", fn, B);
    const size_t rows = (size_t)N;
    const DeviceArray inputs[] = {{d_obs, rows * (size_t)layout.obs_width * 4, 4, "d_obs"},
                                  {d_actions, rows * (sde ? 4 : 8), sde ? (size_t)4 : (size_t)8, "d_actions"},
                                  {d_old_log_probs, rows * 4, 4, "d_old_log_probs"},
                                  {d_advantages, rows * 4, 4, "d_advantages"},
                                  {d_returns, rows * 4, 4, "d_returns"},
                                  {d_index, (size_t)B * 8, 8, "d_index"}};
    const DeviceArray outputs[] = {{d_params, (size_t)layout.total * 4, 4, "d_params"},
                                   {d_state, 4 * (size_t)rf::kPpoStateHeader + 8 * (size_t)layout.total, 8, "d_state"},
                                   {d_workspace, (size_t)work.total * 4, 8, "d_workspace"},
                                   {d_stats, 32, 4, "d_stats"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // Every array is the caller's and the hyper-parameters travel by value: three launches on the caller's stream,
    // nothing allocated, nothing waited for.  The workspace layout is that of B itself: any workspace made for a larger
    // max_batch holds it.
    float *ws = (float *)d_workspace;
    const unsigned tiles = (unsigned)((B + rf::kPolicyTile - 1) / rf::kPolicyTile);
    hipLaunchKernelGGL(sde ? rf::ppo_backward_kernel<true> : rf::ppo_backward_kernel<false>, dim3(tiles, 2u),
                       dim3(rf::kPpoThreads), 0, caller, layout, work, hyper, (const float *)d_params,
                       (const rf::PpoHeader *)d_state, ws, N, d_obs, d_actions, d_old_log_probs, d_advantages, d_returns, B,
                       (const int64_t *)d_index, (const rf::PpoHyper *)nullptr);
    RF_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf::ppo_gradient_kernel<false>, dim3(work.partials), dim3(rf::kPpoThreads), 0, caller, layout, work, ws,
                       B, (const float *)d_params);
    RF_HIP(hipGetLastError());
    const unsigned slices = (layout.total + rf::kPpoAdamSlice - 1) / rf::kPpoAdamSlice;
    hipLaunchKernelGGL(rf::ppo_adam_kernel<false>, dim3(slices + 1u), dim3(rf::kPpoThreads), 0, caller, layout.total, work,
                       hyper, d_params, (float *)d_state, (const float *)ws, B, d_stats, (const rf::PpoHyper *)nullptr);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_ppo_update(rf_ctx *ctx, const rf_policy_desc *policy, const rf_ppo_desc *ppo, float *d_params, void *d_state,
                  void *d_workspace, int N, const float *d_obs, const long long *d_actions, const float *d_old_log_probs,
                  const float *d_advantages, const float *d_returns, int B, const long long *d_index, float *d_stats,
                  void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_ppo_update");
    RF_HIP(hipSetDevice(ctx->device));
    return ppo_update_any("rf_ppo_update", false, ctx, policy, ppo, d_params, d_state, d_workspace, N, d_obs, d_actions,
                          d_old_log_probs, d_advantages, d_returns, B, d_index, d_stats, caller_stream);
}

// ---- population (include/reinfocus_hip.h): the two entry points above over G groups, one launch per stage ----------------

int rf_policy_forward_grouped(rf_ctx *ctx, const rf_policy_desc *desc, int G, int m, const float *d_params,
                              const float *d_obs, const float *d_final_obs, const unsigned long long *d_gens,
                              unsigned long long consumed, int flags, long long *d_actions, float *d_log_probs,
                              float *d_values, float *d_final_values, float *d_logits, void *caller_stream)
{
    const char *fn = "rf_policy_forward_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_obs != nullptr, "%s: NULL argument", fn);
    rf::PolicyLayout layout;
    RF_REQUIRE(rf::policy_layout(*desc, layout), RF_POLICY_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH,
               RF_POLICY_MAX_ACTIONS);
    RF_REQUIRE(rf::population_rows(G, m), "%s: G = %d must be in 1 .. %d, m = %d at least 1 and G m at most 2^30", fn, G,
               RF_POPULATION_MAX_GROUPS, m);
    bool sampled;
    if (int rc = policy_forward_asks(fn, G, d_final_obs, d_gens, flags, d_actions, d_log_probs, d_values, d_final_values,
                                     d_logits, sampled))
        return rc;
    RF_HIP(hipSetDevice(ctx->device));
    return policy_forward_any(fn, ctx, layout, G, m, d_params, d_obs, d_final_obs, d_gens, consumed, sampled, d_actions,
                              d_log_probs, d_values, d_final_values, d_logits, caller_stream);
}

unsigned long long rf_ppo_grouped_state_size(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m)
{
    if (ctx == nullptr || policy == nullptr)
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return rf::population_state_bytes(*policy, G, m);
}

unsigned long long rf_ppo_grouped_workspace_size(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m, int T, int B)
{
    if (ctx == nullptr || policy == nullptr)
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return rf::population_workspace_bytes(*policy, G, m, T, B);
}

// What rf_ppo_update_grouped and rf_sde_update_grouped do once they have checked ctx and made its device current: one body,
// the head chosen by `sde` as in ppo_update_any
static int ppo_update_grouped_any(const char *fn, bool sde, rf_ctx *ctx, const rf_policy_desc *policy, int G, int m, int T,
                                  const rf_ppo_hyper *d_hyper, float *d_params, void *d_state, void *d_workspace,
                                  const float *d_obs, const void *d_actions, const float *d_old_log_probs,
                                  const float *d_advantages, const float *d_returns, int B, const long long *d_index,
                                  float *d_stats, void *caller_stream)
{
    RF_REQUIRE(policy && d_hyper && d_params && d_state && d_workspace && d_obs && d_actions && d_old_log_probs
               && d_advantages && d_returns && d_index && d_stats, "%s: NULL argument", fn);
    rf::PolicyLayout layout;
    if (sde) {
        RF_REQUIRE(rf::sde_layout(*policy, layout), RF_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH);
    } else {
        RF_REQUIRE(rf::policy_layout(*policy, layout), RF_POLICY_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH,
                   RF_POLICY_MAX_ACTIONS);
    }
    RF_REQUIRE(m >= 1 && T >= 1 && rf::population_rows(G, (long long)m * (long long)T),
               "%s: G = %d must be in 1 .. %d, m = %d and T = %d at least 1 and G m T at most 2^30", fn, G,
               RF_POPULATION_MAX_GROUPS, m, T);
    const int N = m * T;
    RF_REQUIRE(B >= 1 && B <= RF_PPO_MAX_BATCH && B <= N, "%s: B = %d is not in 1 .. min(m T = %d, %d)", fn, B, N,
               RF_PPO_MAX_BATCH);
    rf::PpoWork work;
    RF_REQUIRE(rf::ppo_work(layout, B, work), "%s: no workspace layout for B = %d", fn, B);
    const size_t groups = (size_t)G, rows = groups * (size_t)N;
    const size_t state_floats = (size_t)rf::kPpoStateHeader + 2 * (size_t)layout.total;
    const DeviceArray inputs[] = {{d_obs, rows * (size_t)layout.obs_width * 4, 4, "d_obs"},
                                  {d_actions, rows * (sde ? 4 : 8), sde ? (size_t)4 : (size_t)8, "d_actions"},
                                  {d_old_log_probs, rows * 4, 4, "d_old_log_probs"},
                                  {d_advantages, rows * 4, 4, "d_advantages"},
                                  {d_returns, rows * 4, 4, "d_returns"},
                                  {d_index, groups * (size_t)B * 8, 8, "d_index"},
                                  {d_hyper, groups * sizeof(rf_ppo_hyper), 8, "d_hyper"}};
    const DeviceArray outputs[] = {{d_params, groups * (size_t)layout.total * 4, 4, "d_params"},
                                   {d_state, groups * state_floats * 4, 8, "d_state"},
                                   {d_workspace, groups * (size_t)work.total * 4, 8, "d_workspace"},
                                   {d_stats, groups * 32, 4, "d_stats"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // As rf_ppo_update: three launches on the caller's stream, nothing allocated, nothing waited for; the workspace of a
    // group has the layout of B itself.
    float *ws = (float *)d_workspace;
    const rf::PpoHyper *hypers = (const rf::PpoHyper *)d_hyper;
    const unsigned tiles = (unsigned)((B + rf::kPolicyTile - 1) / rf::kPolicyTile);
    const auto backward = sde ? rf::ppo_backward_kernel<true, true> : rf::ppo_backward_kernel<false, true>;
    hipLaunchKernelGGL(backward, dim3(tiles, 2u, (unsigned)G), dim3(rf::kPpoThreads), 0, caller, layout, work, rf::PpoHyper{},
                       (const float *)d_params, (const rf::PpoHeader *)d_state, ws, N, d_obs, d_actions,
                       d_old_log_probs, d_advantages, d_returns, B, (const int64_t *)d_index, hypers);
    RF_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf::ppo_gradient_kernel<true>, dim3(work.partials, (unsigned)G), dim3(rf::kPpoThreads), 0, caller,
                       layout, work, ws, B, (const float *)d_params);
    RF_HIP(hipGetLastError());
    const unsigned slices = (layout.total + rf::kPpoAdamSlice - 1) / rf::kPpoAdamSlice;
    hipLaunchKernelGGL(rf::ppo_adam_kernel<true>, dim3(slices + 1u, (unsigned)G), dim3(rf::kPpoThreads), 0, caller,
                       layout.total, work, rf::PpoHyper{}, d_params, (float *)d_state, (const float *)ws, B, d_stats, hypers);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_ppo_update_grouped(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m, int T, const rf_ppo_hyper *d_hyper,
                          float *d_params, void *d_state, void *d_workspace, const float *d_obs, const long long *d_actions,
                          const float *d_old_log_probs, const float *d_advantages, const float *d_returns, int B,
                          const long long *d_index, float *d_stats, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_ppo_update_grouped");
    RF_HIP(hipSetDevice(ctx->device));
    return ppo_update_grouped_any("rf_ppo_update_grouped", false, ctx, policy, G, m, T, d_hyper, d_params, d_state, d_workspace,
                                  d_obs, d_actions, d_old_log_probs, d_advantages, d_returns, B, d_index, d_stats,
                                  caller_stream);
}

int rf_sde_update(rf_ctx *ctx, const rf_policy_desc *policy, const rf_ppo_desc *ppo, float *d_params, void *d_state,
                  void *d_workspace, int N, const float *d_obs, const float *d_actions, const float *d_old_log_probs,
                  const float *d_advantages, const float *d_returns, int B, const long long *d_index, float *d_stats,
                  void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_sde_update");
    RF_HIP(hipSetDevice(ctx->device));
    return ppo_update_any("rf_sde_update", true, ctx, policy, ppo, d_params, d_state, d_workspace, N, d_obs, d_actions,
                          d_old_log_probs, d_advantages, d_returns, B, d_index, d_stats, caller_stream);
}

unsigned long long rf_sde_params_size(rf_ctx *ctx, const rf_policy_desc *desc)
{
    rf::PolicyLayout layout;
    if (ctx == nullptr || desc == nullptr || !rf::sde_layout(*desc, layout))
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return layout.total;
}

unsigned long long rf_sde_state_size(rf_ctx *ctx, const rf_policy_desc *policy)
{
    rf::PolicyLayout layout;
    if (ctx == nullptr || policy == nullptr || !rf::sde_layout(*policy, layout))
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return 4ull * rf::kPpoStateHeader + 8ull * layout.total;
}

unsigned long long rf_sde_workspace_size(rf_ctx *ctx, const rf_policy_desc *policy, int max_batch)
{
    rf::PolicyLayout layout;
    rf::PpoWork work;
    if (ctx == nullptr || policy == nullptr || !rf::sde_layout(*policy, layout) || !rf::ppo_work(layout, max_batch, work))
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return 4ull * work.total;
}

int rf_sde_noise_reset(rf_ctx *ctx, const rf_policy_desc *desc, const float *d_params, int n,
                       const unsigned long long gen[4], float *d_theta, void *caller_stream)
{
    const char *fn = "rf_sde_noise_reset";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(desc != nullptr && d_params != nullptr && gen != nullptr && d_theta != nullptr, "%s: NULL argument", fn);
    rf::PolicyLayout layout;
    RF_REQUIRE(rf::sde_layout(*desc, layout), RF_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH);
    RF_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %d must be at least 1 (and at most 2^20)", fn, n);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)n * (size_t)layout.sde;
    const DeviceArray inputs[] = {{d_params, (size_t)layout.total * 4, 4, "d_params"}};
    const DeviceArray outputs[] = {{d_theta, cells * 4, 4, "d_theta"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn, 0, nullptr))
        return rc;
    rf::PolicyGen words{};
    for (int i = 0; i < 4; ++i)
        words.word[i] = gen[i];
    const unsigned blocks = (unsigned)((cells + rf::kPolicyThreads - 1) / rf::kPolicyThreads);
    hipLaunchKernelGGL(rf::sde_noise_kernel<false>, dim3(blocks), dim3(rf::kPolicyThreads), 0, (hipStream_t)caller_stream,
                       words, d_params + layout.log_std, n, (int)layout.sde, d_theta, (const rf::PolicyGen *)nullptr,
                       (const uint64_t *)nullptr, (const uint8_t *)nullptr, 0u);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

// rf_sde_forward (G = 0: n rows) and rf_sde_forward_grouped (G >= 1: m rows per group), in two parts as the policy forwards
// are: what a call may ask for (pi: something of the actor; sampled: with d_theta's noise) ...
static int sde_forward_asks(const char *fn, int G, const float *d_final_obs, const float *d_theta, int flags, bool pi,
                            const float *d_values, const float *d_final_values, bool &sampled)
{
    RF_REQUIRE((flags & ~RF_POLICY_DETERMINISTIC) == 0, "%s: unknown flags %d", fn, flags);
    RF_REQUIRE(pi || d_values || d_final_values, "%s: no output is asked for", fn);
    RF_REQUIRE(d_final_values == nullptr || d_final_obs != nullptr, "%s: d_final_values needs d_final_obs", fn);
    sampled = pi && (flags & RF_POLICY_DETERMINISTIC) == 0;
    RF_REQUIRE(!sampled || d_theta != nullptr, "%s: a sampled call needs d_theta (%s)", fn,
               G ? "rf_sde_noise_reset_grouped" : "rf_sde_noise_reset");
    return RF_OK;
}

// ... and its arrays, their check and the launch
static int sde_forward_any(const char *fn, rf_ctx *ctx, const rf::PolicyLayout &layout, int G, int m, const float *d_params,
                           const float *d_obs, const float *d_final_obs, const float *d_theta, bool sampled, float *d_actions,
                           float *d_env_actions, float *d_log_probs, float *d_values, float *d_final_values, float *d_mean,
                           float *d_sigma, void *caller_stream)
{
    const bool pi = d_actions || d_env_actions || d_log_probs || d_mean || d_sigma;
    const bool vf = d_values != nullptr || d_final_values != nullptr;
    const size_t groups = G ? (size_t)G : 1, rows = groups * (size_t)m;
    const DeviceArray inputs[] = {{d_params, groups * (size_t)layout.total * 4, 4, "d_params"},
                                  {d_obs, rows * (size_t)layout.obs_width * 4, 4, "d_obs"},
                                  {d_final_obs, rows * (size_t)layout.obs_width * 4, 4, "d_final_obs"},
                                  {sampled ? d_theta : nullptr, rows * (size_t)layout.sde * 4, 4, "d_theta"}};
    const DeviceArray outputs[] = {{d_actions, rows * 4, 4, "d_actions"},       {d_env_actions, rows * 4, 4, "d_env_actions"},
                                   {d_log_probs, rows * 4, 4, "d_log_probs"},   {d_values, rows * 4, 4, "d_values"},
                                   {d_final_values, rows * 4, 4, "d_final_values"}, {d_mean, rows * 4, 4, "d_mean"},
                                   {d_sigma, rows * 4, 4, "d_sigma"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    // one launch on the caller's stream, nothing allocated, nothing waited for (a caller may capture it)
    const unsigned tiles = (unsigned)(((size_t)m + rf::kPolicyTile - 1) / rf::kPolicyTile);
    hipLaunchKernelGGL(G ? rf::sde_forward_kernel<true> : rf::sde_forward_kernel<false>,
                       dim3(tiles, pi && vf ? 2u : 1u, (unsigned)groups), dim3(rf::kPolicyThreads), 0,
                       (hipStream_t)caller_stream, layout, d_params, m, d_obs, d_final_obs, sampled ? d_theta : nullptr,
                       pi ? 0 : 1, d_actions, d_env_actions, d_log_probs, d_values, d_final_values, d_mean, d_sigma);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_sde_forward(rf_ctx *ctx, const rf_policy_desc *desc, const float *d_params, int n, const float *d_obs,
                   const float *d_final_obs, const float *d_theta, int flags, float *d_actions, float *d_env_actions,
                   float *d_log_probs, float *d_values, float *d_final_values, float *d_mean, float *d_sigma,
                   void *caller_stream)
{
    const char *fn = "rf_sde_forward";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_obs != nullptr, "%s: NULL argument", fn);
    rf::PolicyLayout layout;
    RF_REQUIRE(rf::sde_layout(*desc, layout), RF_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH);
    RF_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %d must be at least 1 (and at most 2^20)", fn, n);
    const bool pi = d_actions || d_env_actions || d_log_probs || d_mean || d_sigma;
    bool sampled;
    if (int rc = sde_forward_asks(fn, 0, d_final_obs, d_theta, flags, pi, d_values, d_final_values, sampled))
        return rc;
    RF_HIP(hipSetDevice(ctx->device));
    return sde_forward_any(fn, ctx, layout, 0, n, d_params, d_obs, d_final_obs, d_theta, sampled, d_actions, d_env_actions,
                           d_log_probs, d_values, d_final_values, d_mean, d_sigma, caller_stream);
}

// ---- population sde (include/reinfocus_hip.h): the sde entry points above over G groups, one launch per stage ---------------
int rf_sde_noise_reset_grouped(rf_ctx *ctx, const rf_policy_desc *desc, int G, int m, const float *d_params,
                               const unsigned long long *d_gens, const unsigned long long *d_consumed,
                               const unsigned char *d_select, float *d_theta, void *caller_stream)
{
    const char *fn = "rf_sde_noise_reset_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_gens != nullptr && d_consumed != nullptr && d_theta != nullptr,
               "%s: NULL argument", fn);
    rf::PolicyLayout layout;
    RF_REQUIRE(rf::sde_layout(*desc, layout), RF_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH);
    RF_REQUIRE(rf::population_rows(G, m) && m <= (1 << 20), RF_POPULATION_LIMITS, fn, G, RF_POPULATION_MAX_GROUPS, m);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t groups = (size_t)G, cells = (size_t)m * (size_t)layout.sde;
    const DeviceArray inputs[] = {{d_params, groups * (size_t)layout.total * 4, 4, "d_params"},
                                  {d_gens, groups * 32, 8, "d_gens"},
                                  {d_consumed, groups * 8, 8, "d_consumed"},
                                  {d_select, groups, 1, "d_select"}};
    const DeviceArray outputs[] = {{d_theta, groups * cells * 4, 4, "d_theta"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn, 0, nullptr))
        return rc;
    // As rf_sde_noise_reset: one launch on the caller's stream, nothing allocated, nothing waited for; the generators'
    // words, their draw counts and the selection are read on the device.
    static_assert(sizeof(rf::PolicyGen) == 32, "d_gens is uint64 [G][4]");
    const unsigned blocks = (unsigned)((cells + rf::kPolicyThreads - 1) / rf::kPolicyThreads);
    hipLaunchKernelGGL(rf::sde_noise_kernel<true>, dim3(blocks, (unsigned)G), dim3(rf::kPolicyThreads), 0,
                       (hipStream_t)caller_stream, rf::PolicyGen{}, d_params + layout.log_std, m, (int)layout.sde, d_theta,
                       (const rf::PolicyGen *)d_gens, (const uint64_t *)d_consumed, (const uint8_t *)d_select, layout.total);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_sde_forward_grouped(rf_ctx *ctx, const rf_policy_desc *desc, int G, int m, const float *d_params, const float *d_obs,
                           const float *d_final_obs, const float *d_theta, int flags, float *d_actions, float *d_env_actions,
                           float *d_log_probs, float *d_values, float *d_final_values, float *d_mean, float *d_sigma,
                           void *caller_stream)
{
    const char *fn = "rf_sde_forward_grouped";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_obs != nullptr, "%s: NULL argument", fn);
    rf::PolicyLayout layout;
    RF_REQUIRE(rf::sde_layout(*desc, layout), RF_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH);
    RF_REQUIRE(rf::population_rows(G, m) && m <= (1 << 20), RF_POPULATION_LIMITS, fn, G, RF_POPULATION_MAX_GROUPS, m);
    const bool pi = d_actions || d_env_actions || d_log_probs || d_mean || d_sigma;
    bool sampled;
    if (int rc = sde_forward_asks(fn, G, d_final_obs, d_theta, flags, pi, d_values, d_final_values, sampled))
        return rc;
    RF_HIP(hipSetDevice(ctx->device));
    return sde_forward_any(fn, ctx, layout, G, m, d_params, d_obs, d_final_obs, d_theta, sampled, d_actions, d_env_actions,
                           d_log_probs, d_values, d_final_values, d_mean, d_sigma, caller_stream);
}

unsigned long long rf_sde_grouped_state_size(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m)
{
    if (ctx == nullptr || policy == nullptr)
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return rf::population_state_bytes(*policy, G, m, true);
}

unsigned long long rf_sde_grouped_workspace_size(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m, int T, int B)
{
    if (ctx == nullptr || policy == nullptr)
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return rf::population_workspace_bytes(*policy, G, m, T, B, true);
}

int rf_sde_update_grouped(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m, int T, const rf_ppo_hyper *d_hyper,
                          float *d_params, void *d_state, void *d_workspace, const float *d_obs, const float *d_actions,
                          const float *d_old_log_probs, const float *d_advantages, const float *d_returns, int B,
                          const long long *d_index, float *d_stats, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_sde_update_grouped");
    RF_HIP(hipSetDevice(ctx->device));
    return ppo_update_grouped_any("rf_sde_update_grouped", true, ctx, policy, G, m, T, d_hyper, d_params, d_state, d_workspace,
                                  d_obs, d_actions, d_old_log_probs, d_advantages, d_returns, B, d_index, d_stats,
                                  caller_stream);
}

// The recurrent entry points are written once, over (desc, sde, critic): the rf_lstm_ / rf_lstm_sde_ ones are these with
// RF_LSTM_CRITIC_LSTM, their rf_lstm_critic_ siblings hand in rf_lstm_critic_desc.critic ("lstm critic").  Each extern "C"
// wrapper checks ctx and selects its device; the bodies below do everything else.
static bool lstm_layout_any(const rf_lstm_policy_desc *desc, bool sde, int critic, rf::LstmLayout &layout)
{
    return desc != nullptr && rf::lstm_layout_nets(*desc, layout, sde, critic);
}

// floats of the packed parameters; 0 if refused
static unsigned long long lstm_params_size_any(rf_ctx *ctx, const rf_lstm_policy_desc *desc, bool sde, int critic)
{
    rf::LstmLayout layout;
    return ctx != nullptr && lstm_layout_any(desc, sde, critic, layout) ? layout.total : 0;
}

// bytes of the optimizer state; 0 if refused
static unsigned long long lstm_state_size_any(rf_ctx *ctx, const rf_lstm_policy_desc *desc, bool sde, int critic)
{
    rf::LstmLayout layout;
    return ctx != nullptr && lstm_layout_any(desc, sde, critic, layout) ? 4ull * rf::kPpoStateHeader + 8ull * layout.total : 0;
}

// bytes of the update's workspace; 0 if refused
static unsigned long long lstm_workspace_size_any(rf_ctx *ctx, const rf_lstm_policy_desc *desc, bool sde, int critic,
                                                  int max_batch)
{
    rf::LstmLayout layout;
    rf::LstmPpoWork work;
    if (ctx == nullptr || !lstm_layout_any(desc, sde, critic, layout) || !rf::lstm_ppo_work(layout, max_batch, work))
        return 0;
    return 4ull * work.total;
}

unsigned long long rf_lstm_params_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return lstm_params_size_any(ctx, desc, false, RF_LSTM_CRITIC_LSTM);
}

unsigned long long rf_lstm_state_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc, int n)
{
    rf::LstmLayout layout;
    if (ctx == nullptr || desc == nullptr || n < 1 || !rf::lstm_layout(*desc, layout))
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    return rf::lstm_state_floats(n, layout.hidden);
}

// rf_lstm_forward and rf_lstm_critic_forward: one body
static int lstm_forward_any(const char *fn, int critic, rf_ctx *ctx, const rf_lstm_policy_desc *desc, const float *d_params,
                            int n, const float *d_obs, const uint8_t *d_episode_starts, const float *d_final_obs,
                            const float *d_state_in, float *d_state_out, const unsigned long long gen[4], int flags,
                            long long *d_actions, float *d_log_probs, float *d_values, float *d_final_values,
                            float *d_logits, void *caller_stream)
{
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_obs != nullptr && d_episode_starts != nullptr &&
               d_state_in != nullptr, "%s: NULL argument", fn);
    rf::LstmLayout layout;
    RF_REQUIRE(lstm_layout_any(desc, false, critic, layout), RF_LSTM_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH,
               RF_POLICY_MAX_ACTIONS);
    RF_REQUIRE(n >= 1 && n <= (1 << 30), "%s: n = %d must be at least 1 (and at most 2^30)", fn, n);
    RF_REQUIRE((flags & ~RF_POLICY_DETERMINISTIC) == 0, "%s: unknown flags %d", fn, flags);
    RF_REQUIRE(d_actions || d_values || d_final_values || d_logits || d_state_out, "%s: no output is asked for", fn);
    RF_REQUIRE(d_log_probs == nullptr || d_actions != nullptr, "%s: d_log_probs are those of d_actions, which is NULL", fn);
    RF_REQUIRE(d_final_values == nullptr || d_final_obs != nullptr, "%s: d_final_values needs d_final_obs", fn);
    const bool sampled = d_actions != nullptr && (flags & RF_POLICY_DETERMINISTIC) == 0;
    RF_REQUIRE(!sampled || gen != nullptr, "%s: a sampled call needs gen", fn);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t rows = (size_t)n;
    const size_t state_bytes = rf::lstm_state_floats(n, layout.hidden) * 4;
    const DeviceArray inputs[] = {{d_params, (size_t)layout.total * 4, 4, "d_params"},
                                  {d_obs, rows * (size_t)layout.obs_width * 4, 4, "d_obs"},
                                  {d_episode_starts, rows, 1, "d_episode_starts"},
                                  {d_final_obs, rows * (size_t)layout.obs_width * 4, 4, "d_final_obs"},
                                  {d_state_in, state_bytes, 4, "d_state_in"}};
    const DeviceArray outputs[] = {{d_actions, rows * 8, 8, "d_actions"},
                                   {d_log_probs, rows * 4, 4, "d_log_probs"},
                                   {d_values, rows * 4, 4, "d_values"},
                                   {d_final_values, rows * 4, 4, "d_final_values"},
                                   {d_logits, rows * (size_t)layout.mlp.n_actions * 4, 4, "d_logits"},
                                   {d_state_out, state_bytes, 4, "d_state_out"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn, kStateInPlace))
        return rc;
    // As rf_policy_forward: every array is the caller's and gen is read here, by value: one launch on the caller's stream.
    rf::PolicyGen words{};
    if (sampled)
        for (int i = 0; i < 4; ++i)
            words.word[i] = gen[i];
    // with d_state_out both cells run, whatever is asked of the heads: the state of both nets advances together (the
    // linear critic has no cell: its block runs for a value only, and the pi block stores both halves of the state)
    const bool linear = critic == RF_LSTM_CRITIC_LINEAR;
    const bool pi = d_actions != nullptr || d_logits != nullptr || d_state_out != nullptr;
    const bool vf = d_values != nullptr || d_final_values != nullptr || (!linear && d_state_out != nullptr);
    const unsigned tiles = (unsigned)((rows + rf::kPolicyTile - 1) / rf::kPolicyTile);
    const auto kernel = linear ? rf::lstm_forward_kernel<false, true> : rf::lstm_forward_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(tiles, pi && vf ? 2u : 1u), dim3(rf::kPolicyThreads), 0,
                       (hipStream_t)caller_stream, layout, d_params, n, d_obs, d_episode_starts, d_final_obs, d_state_in,
                       d_state_out, words, sampled ? 1 : 0, pi ? 0 : 1, (int64_t *)d_actions, d_log_probs, d_values,
                       d_final_values, d_logits, rf::LstmNoSde{}, (const rf::PolicyGen *)nullptr, (uint64_t)0, 0);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_lstm_forward(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const float *d_params, int n, const float *d_obs,
                    const uint8_t *d_episode_starts, const float *d_final_obs, const float *d_state_in, float *d_state_out,
                    const unsigned long long gen[4], int flags, long long *d_actions, float *d_log_probs, float *d_values,
                    float *d_final_values, float *d_logits, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_forward");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_forward_any("rf_lstm_forward", RF_LSTM_CRITIC_LSTM, ctx, desc, d_params, n, d_obs, d_episode_starts,
                            d_final_obs, d_state_in, d_state_out, gen, flags, d_actions, d_log_probs, d_values,
                            d_final_values, d_logits, caller_stream);
}

unsigned long long rf_lstm_sde_params_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return lstm_params_size_any(ctx, desc, true, RF_LSTM_CRITIC_LSTM);
}

// rf_lstm_sde_noise_reset and rf_lstm_critic_sde_noise_reset: one body
static int lstm_sde_noise_reset_any(const char *fn, int critic, rf_ctx *ctx, const rf_lstm_policy_desc *desc,
                                    const float *d_params, int n, const unsigned long long gen[4], float *d_theta,
                                    void *caller_stream)
{
    RF_REQUIRE(desc != nullptr && d_params != nullptr && gen != nullptr && d_theta != nullptr, "%s: NULL argument", fn);
    rf::LstmLayout layout;
    RF_REQUIRE(lstm_layout_any(desc, true, critic, layout), RF_LSTM_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH);
    RF_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %d must be at least 1 (and at most 2^20)", fn, n);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)n * (size_t)layout.mlp.sde;
    const DeviceArray inputs[] = {{d_params, (size_t)layout.total * 4, 4, "d_params"}};
    const DeviceArray outputs[] = {{d_theta, cells * 4, 4, "d_theta"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn, 0, nullptr))
        return rc;
    rf::PolicyGen words{};
    for (int i = 0; i < 4; ++i)
        words.word[i] = gen[i];
    // sde_noise_kernel as rf_sde_noise_reset launches it, with this layout's log_std
    const unsigned blocks = (unsigned)((cells + rf::kPolicyThreads - 1) / rf::kPolicyThreads);
    hipLaunchKernelGGL(rf::sde_noise_kernel<false>, dim3(blocks), dim3(rf::kPolicyThreads), 0, (hipStream_t)caller_stream,
                       words, d_params + layout.mlp.log_std, n, (int)layout.mlp.sde, d_theta, (const rf::PolicyGen *)nullptr,
                       (const uint64_t *)nullptr, (const uint8_t *)nullptr, 0u);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_lstm_sde_noise_reset(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const float *d_params, int n,
                            const unsigned long long gen[4], float *d_theta, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_sde_noise_reset");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_sde_noise_reset_any("rf_lstm_sde_noise_reset", RF_LSTM_CRITIC_LSTM, ctx, desc, d_params, n, gen, d_theta,
                                    caller_stream);
}

// rf_lstm_sde_forward and rf_lstm_critic_sde_forward: one body
static int lstm_sde_forward_any(const char *fn, int critic, rf_ctx *ctx, const rf_lstm_policy_desc *desc,
                                const float *d_params, int n, const float *d_obs, const uint8_t *d_episode_starts,
                                const float *d_final_obs, const float *d_state_in, float *d_state_out, const float *d_theta,
                                int flags, float *d_actions, float *d_env_actions, float *d_log_probs, float *d_values,
                                float *d_final_values, float *d_mean, float *d_sigma, void *caller_stream)
{
    RF_REQUIRE(desc != nullptr && d_params != nullptr && d_obs != nullptr && d_episode_starts != nullptr &&
               d_state_in != nullptr, "%s: NULL argument", fn);
    rf::LstmLayout layout;
    RF_REQUIRE(lstm_layout_any(desc, true, critic, layout), RF_LSTM_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH);
    RF_REQUIRE(n >= 1 && n <= (1 << 20), "%s: n = %d must be at least 1 (and at most 2^20)", fn, n);
    RF_REQUIRE((flags & ~RF_POLICY_DETERMINISTIC) == 0, "%s: unknown flags %d", fn, flags);
    const bool pi_out = d_actions || d_env_actions || d_log_probs || d_mean || d_sigma;
    RF_REQUIRE(pi_out || d_values || d_final_values || d_state_out, "%s: no output is asked for", fn);
    RF_REQUIRE(d_final_values == nullptr || d_final_obs != nullptr, "%s: d_final_values needs d_final_obs", fn);
    const bool sampled = pi_out && (flags & RF_POLICY_DETERMINISTIC) == 0;
    RF_REQUIRE(!sampled || d_theta != nullptr, "%s: a sampled call needs d_theta (rf_lstm_sde_noise_reset)", fn);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t rows = (size_t)n;
    const size_t state_bytes = rf::lstm_state_floats(n, layout.hidden) * 4;
    const DeviceArray inputs[] = {{d_params, (size_t)layout.total * 4, 4, "d_params"},
                                  {d_obs, rows * (size_t)layout.obs_width * 4, 4, "d_obs"},
                                  {d_episode_starts, rows, 1, "d_episode_starts"},
                                  {d_final_obs, rows * (size_t)layout.obs_width * 4, 4, "d_final_obs"},
                                  {sampled ? d_theta : nullptr, rows * (size_t)layout.mlp.sde * 4, 4, "d_theta"},
                                  {d_state_in, state_bytes, 4, "d_state_in"}};
    const DeviceArray outputs[] = {{d_actions, rows * 4, 4, "d_actions"},       {d_env_actions, rows * 4, 4, "d_env_actions"},
                                   {d_log_probs, rows * 4, 4, "d_log_probs"},   {d_values, rows * 4, 4, "d_values"},
                                   {d_final_values, rows * 4, 4, "d_final_values"}, {d_mean, rows * 4, 4, "d_mean"},
                                   {d_sigma, rows * 4, 4, "d_sigma"},           {d_state_out, state_bytes, 4, "d_state_out"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn, kStateInPlace))
        return rc;
    // As rf_lstm_forward: one launch on the caller's stream; with d_state_out both cells run, whatever is asked of the heads
    const bool linear = critic == RF_LSTM_CRITIC_LINEAR;
    const bool pi = pi_out || d_state_out != nullptr;
    const bool vf = d_values != nullptr || d_final_values != nullptr || (!linear && d_state_out != nullptr);
    const unsigned tiles = (unsigned)((rows + rf::kPolicyTile - 1) / rf::kPolicyTile);
    const auto kernel = linear ? rf::lstm_forward_kernel<true, true> : rf::lstm_forward_kernel<true>;
    hipLaunchKernelGGL(kernel, dim3(tiles, pi && vf ? 2u : 1u), dim3(rf::kPolicyThreads), 0,
                       (hipStream_t)caller_stream, layout, d_params, n, d_obs, d_episode_starts, d_final_obs, d_state_in,
                       d_state_out, rf::PolicyGen{}, 0, pi ? 0 : 1, d_actions, d_log_probs, d_values, d_final_values, d_mean,
                       rf::LstmSde{sampled ? d_theta : nullptr, d_env_actions, d_sigma}, (const rf::PolicyGen *)nullptr,
                       (uint64_t)0, 0);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_lstm_sde_forward(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const float *d_params, int n, const float *d_obs,
                        const uint8_t *d_episode_starts, const float *d_final_obs, const float *d_state_in,
                        float *d_state_out, const float *d_theta, int flags, float *d_actions, float *d_env_actions,
                        float *d_log_probs, float *d_values, float *d_final_values, float *d_mean, float *d_sigma,
                        void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_sde_forward");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_sde_forward_any("rf_lstm_sde_forward", RF_LSTM_CRITIC_LSTM, ctx, desc, d_params, n, d_obs, d_episode_starts,
                                d_final_obs, d_state_in, d_state_out, d_theta, flags, d_actions, d_env_actions, d_log_probs,
                                d_values, d_final_values, d_mean, d_sigma, caller_stream);
}

unsigned long long rf_lstm_ppo_state_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return lstm_state_size_any(ctx, desc, false, RF_LSTM_CRITIC_LSTM);
}

unsigned long long rf_lstm_ppo_workspace_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc, int max_batch)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return lstm_workspace_size_any(ctx, desc, false, RF_LSTM_CRITIC_LSTM, max_batch);
}

// rf_lstm_ppo_update, rf_lstm_sde_update and their rf_lstm_critic_ siblings: one body; `sde` selects lstm_sde_layout,
// float32 actions and the Gaussian instantiations of the MLP and gradient kernels; `critic` the vf net ("lstm critic")
static int lstm_update_any(const char *fn, bool sde, int critic, rf_ctx *ctx, const rf_lstm_policy_desc *desc, const rf_ppo_desc *ppo,
                           float *d_params, void *d_state, void *d_workspace, int n_steps, int num_envs,
                           const float *d_observations, const void *d_actions, const float *d_log_probs,
                           const float *d_advantages, const float *d_returns, const uint8_t *d_episode_starts,
                           const float *d_lstm_states, int first, int B, float *d_stats, void *caller_stream)
{
    RF_REQUIRE(desc && ppo && d_params && d_state && d_workspace && d_observations && d_actions && d_log_probs &&
               d_advantages && d_returns && d_episode_starts && d_lstm_states && d_stats, "%s: NULL argument", fn);
    rf::LstmLayout layout;
    if (sde) {
        RF_REQUIRE(lstm_layout_any(desc, true, critic, layout), RF_LSTM_SDE_LIMITS, fn, RF_POLICY_MAX_WIDTH,
                   RF_POLICY_MAX_WIDTH);
    } else {
        RF_REQUIRE(lstm_layout_any(desc, false, critic, layout), RF_LSTM_LIMITS, fn, RF_POLICY_MAX_WIDTH, RF_POLICY_MAX_WIDTH,
                   RF_POLICY_MAX_ACTIONS);
    }
    RF_REQUIRE(n_steps >= 1 && num_envs >= 1 && (long long)n_steps * (long long)num_envs <= (1ll << 30),
               "%s: n_steps = %d and num_envs = %d must be at least 1 (and their product at most 2^30)", fn, n_steps, num_envs);
    const int N = n_steps * num_envs;
    const int most = N < RF_PPO_MAX_BATCH ? N : RF_PPO_MAX_BATCH;
    RF_REQUIRE(B >= 1 && B <= most, "%s: B = %d is not in 1 .. %d (min(n_steps * num_envs, %d))", fn, B, most,
               RF_PPO_MAX_BATCH);
    RF_REQUIRE(first >= 0 && first < N, "%s: first = %d is not in 0 .. %d", fn, first, N - 1);
    rf::PpoHyper hyper;
    RF_REQUIRE(rf::ppo_hyper(*ppo, hyper), "%s: a hyper-parameter is negative or not finite, a beta is outside [0, 1) or "
               "normalize_advantage is not 0 / 1", fn);
    rf::LstmPpoWork work;
    RF_REQUIRE(rf::lstm_ppo_work(layout, B, work), "%s: no workspace layout for B = %d", fn, B);
    const size_t rows = (size_t)N, slab = (size_t)(n_steps + 1) * (size_t)num_envs;
    const DeviceArray inputs[] = {{d_observations, rows * (size_t)layout.obs_width * 4, 4, "d_observations"},
                                  {d_actions, rows * (sde ? 4 : 8), sde ? (size_t)4 : (size_t)8, "d_actions"},
                                  {d_log_probs, rows * 4, 4, "d_log_probs"},
                                  {d_advantages, rows * 4, 4, "d_advantages"},
                                  {d_returns, rows * 4, 4, "d_returns"},
                                  {d_episode_starts, slab, 1, "d_episode_starts"},
                                  {d_lstm_states, slab * 4 * (size_t)layout.hidden * 4, 4, "d_lstm_states"}};
    const DeviceArray outputs[] = {{d_params, (size_t)layout.total * 4, 4, "d_params"},
                                   {d_state, 4 * (size_t)rf::kPpoStateHeader + 8 * (size_t)layout.total, 8, "d_state"},
                                   {d_workspace, (size_t)work.total * 4, 8, "d_workspace"},
                                   {d_stats, 32, 4, "d_stats"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // As rf_ppo_update: every array is the caller's and the hyper-parameters travel by value: six launches on the
    // caller's stream, nothing allocated, nothing waited for.  The workspace layout is that of B itself.
    float *ws = (float *)d_workspace;
    const dim3 threads(rf::kPpoThreads);
    // (the linear critic: B pi walks and the vf net's tiles of rows in the first launch, the pi net's BPTT alone in the third)
    const bool linear = critic == RF_LSTM_CRITIC_LINEAR;
    const unsigned tiles = (unsigned)((B + rf::kPolicyTile - 1) / rf::kPolicyTile);
    const unsigned walks = linear ? 1u : 2u;
    const auto forward = linear ? rf::lstm_ppo_forward_kernel<true> : rf::lstm_ppo_forward_kernel<false>;
    hipLaunchKernelGGL(forward, dim3((unsigned)B + (linear ? tiles : 0u), walks), threads, 0, caller, layout, work,
                       (const float *)d_params, ws, n_steps, num_envs, d_observations, d_episode_starts, d_lstm_states, first,
                       B, (const int *)nullptr, 0);
    RF_HIP(hipGetLastError());
    hipLaunchKernelGGL(sde ? rf::lstm_ppo_mlp_kernel<true> : rf::lstm_ppo_mlp_kernel<false>, dim3(tiles, 2u), threads, 0,
                       caller, layout, work, hyper, (const float *)d_params, (const rf::PpoHeader *)d_state, ws, N, d_actions,
                       d_log_probs, d_advantages, d_returns, first, B, (const rf::PpoHyper *)nullptr, (const int *)nullptr);
    RF_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf::lstm_ppo_bptt_kernel<false>, dim3((unsigned)B, walks), threads, 0, caller, layout, work,
                       (const float *)d_params, ws, n_steps, num_envs, d_episode_starts, first, B, (const int *)nullptr, 0);
    RF_HIP(hipGetLastError());
    const auto gradient = linear ? (sde ? rf::lstm_ppo_gradient_kernel<true, true> : rf::lstm_ppo_gradient_kernel<false, true>)
                                 : (sde ? rf::lstm_ppo_gradient_kernel<true> : rf::lstm_ppo_gradient_kernel<false>);
    hipLaunchKernelGGL(gradient, dim3(work.mlp.partials), threads, 0, caller, layout, work, ws, B, (const float *)d_params);
    RF_HIP(hipGetLastError());
    hipLaunchKernelGGL(rf::lstm_ppo_norm_kernel<false>, dim3(work.supers), dim3(rf::kLstmPpoGroup), 0, caller, work, ws);
    RF_HIP(hipGetLastError());
    const unsigned slices = (layout.total + rf::kPpoAdamSlice - 1) / rf::kPpoAdamSlice;
    hipLaunchKernelGGL(rf::ppo_adam_kernel<false>, dim3(slices + 1u), threads, 0, caller, layout.total,
                       rf::lstm_ppo_adam_work(work), hyper, d_params, (float *)d_state, (const float *)ws, B, d_stats,
                       (const rf::PpoHyper *)nullptr);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_lstm_ppo_update(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const rf_ppo_desc *ppo, float *d_params, void *d_state,
                       void *d_workspace, int n_steps, int num_envs, const float *d_observations, const long long *d_actions,
                       const float *d_log_probs, const float *d_advantages, const float *d_returns,
                       const uint8_t *d_episode_starts, const float *d_lstm_states, int first, int B, float *d_stats,
                       void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_ppo_update");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_update_any("rf_lstm_ppo_update", false, RF_LSTM_CRITIC_LSTM, ctx, desc, ppo, d_params, d_state, d_workspace, n_steps, num_envs,
                           d_observations, d_actions, d_log_probs, d_advantages, d_returns, d_episode_starts, d_lstm_states,
                           first, B, d_stats, caller_stream);
}

unsigned long long rf_lstm_sde_state_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return lstm_state_size_any(ctx, desc, true, RF_LSTM_CRITIC_LSTM);
}

unsigned long long rf_lstm_sde_workspace_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc, int max_batch)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return lstm_workspace_size_any(ctx, desc, true, RF_LSTM_CRITIC_LSTM, max_batch);
}

int rf_lstm_sde_update(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const rf_ppo_desc *ppo, float *d_params, void *d_state,
                       void *d_workspace, int n_steps, int num_envs, const float *d_observations, const float *d_actions,
                       const float *d_log_probs, const float *d_advantages, const float *d_returns,
                       const uint8_t *d_episode_starts, const float *d_lstm_states, int first, int B, float *d_stats,
                       void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_sde_update");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_update_any("rf_lstm_sde_update", true, RF_LSTM_CRITIC_LSTM, ctx, desc, ppo, d_params, d_state, d_workspace, n_steps, num_envs,
                           d_observations, d_actions, d_log_probs, d_advantages, d_returns, d_episode_starts, d_lstm_states,
                           first, B, d_stats, caller_stream);
}

// ---- "lstm critic": the siblings over rf_lstm_critic_desc -- thin wrappers around the bodies above --------------------------
unsigned long long rf_lstm_critic_params_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return desc == nullptr ? 0 : lstm_params_size_any(ctx, &desc->lstm, false, desc->critic);
}

int rf_lstm_critic_forward(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const float *d_params, int n, const float *d_obs,
                           const uint8_t *d_episode_starts, const float *d_final_obs, const float *d_state_in,
                           float *d_state_out, const unsigned long long gen[4], int flags, long long *d_actions,
                           float *d_log_probs, float *d_values, float *d_final_values, float *d_logits, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_critic_forward");
    RF_REQUIRE(desc != nullptr, "%s: NULL argument", "rf_lstm_critic_forward");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_forward_any("rf_lstm_critic_forward", desc->critic, ctx, &desc->lstm, d_params, n, d_obs, d_episode_starts,
                            d_final_obs, d_state_in, d_state_out, gen, flags, d_actions, d_log_probs, d_values,
                            d_final_values, d_logits, caller_stream);
}

unsigned long long rf_lstm_critic_ppo_state_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return desc == nullptr ? 0 : lstm_state_size_any(ctx, &desc->lstm, false, desc->critic);
}

unsigned long long rf_lstm_critic_ppo_workspace_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int max_batch)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return desc == nullptr ? 0 : lstm_workspace_size_any(ctx, &desc->lstm, false, desc->critic, max_batch);
}

int rf_lstm_critic_ppo_update(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const rf_ppo_desc *ppo, float *d_params,
                              void *d_state, void *d_workspace, int n_steps, int num_envs, const float *d_observations,
                              const long long *d_actions, const float *d_log_probs, const float *d_advantages,
                              const float *d_returns, const uint8_t *d_episode_starts, const float *d_lstm_states, int first,
                              int B, float *d_stats, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_critic_ppo_update");
    RF_REQUIRE(desc != nullptr, "%s: NULL argument", "rf_lstm_critic_ppo_update");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_update_any("rf_lstm_critic_ppo_update", false, desc->critic, ctx, &desc->lstm, ppo, d_params, d_state,
                           d_workspace, n_steps, num_envs, d_observations, d_actions, d_log_probs, d_advantages, d_returns,
                           d_episode_starts, d_lstm_states, first, B, d_stats, caller_stream);
}

unsigned long long rf_lstm_critic_sde_params_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return desc == nullptr ? 0 : lstm_params_size_any(ctx, &desc->lstm, true, desc->critic);
}

int rf_lstm_critic_sde_noise_reset(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const float *d_params, int n,
                                   const unsigned long long gen[4], float *d_theta, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_critic_sde_noise_reset");
    RF_REQUIRE(desc != nullptr, "%s: NULL argument", "rf_lstm_critic_sde_noise_reset");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_sde_noise_reset_any("rf_lstm_critic_sde_noise_reset", desc->critic, ctx, &desc->lstm, d_params, n, gen,
                                    d_theta, caller_stream);
}

int rf_lstm_critic_sde_forward(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const float *d_params, int n, const float *d_obs,
                               const uint8_t *d_episode_starts, const float *d_final_obs, const float *d_state_in,
                               float *d_state_out, const float *d_theta, int flags, float *d_actions, float *d_env_actions,
                               float *d_log_probs, float *d_values, float *d_final_values, float *d_mean, float *d_sigma,
                               void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_critic_sde_forward");
    RF_REQUIRE(desc != nullptr, "%s: NULL argument", "rf_lstm_critic_sde_forward");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_sde_forward_any("rf_lstm_critic_sde_forward", desc->critic, ctx, &desc->lstm, d_params, n, d_obs,
                                d_episode_starts, d_final_obs, d_state_in, d_state_out, d_theta, flags, d_actions,
                                d_env_actions, d_log_probs, d_values, d_final_values, d_mean, d_sigma, caller_stream);
}

unsigned long long rf_lstm_critic_sde_state_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return desc == nullptr ? 0 : lstm_state_size_any(ctx, &desc->lstm, true, desc->critic);
}

unsigned long long rf_lstm_critic_sde_workspace_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int max_batch)
{
    if (ctx != nullptr)
        ignore_error(hipSetDevice(ctx->device));
    return desc == nullptr ? 0 : lstm_workspace_size_any(ctx, &desc->lstm, true, desc->critic, max_batch);
}

int rf_lstm_critic_sde_update(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const rf_ppo_desc *ppo, float *d_params,
                              void *d_state, void *d_workspace, int n_steps, int num_envs, const float *d_observations,
                              const float *d_actions, const float *d_log_probs, const float *d_advantages,
                              const float *d_returns, const uint8_t *d_episode_starts, const float *d_lstm_states, int first,
                              int B, float *d_stats, void *caller_stream)
{
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", "rf_lstm_critic_sde_update");
    RF_REQUIRE(desc != nullptr, "%s: NULL argument", "rf_lstm_critic_sde_update");
    RF_HIP(hipSetDevice(ctx->device));
    return lstm_update_any("rf_lstm_critic_sde_update", true, desc->critic, ctx, &desc->lstm, ppo, d_params, d_state,
                           d_workspace, n_steps, num_envs, d_observations, d_actions, d_log_probs, d_advantages, d_returns,
                           d_episode_starts, d_lstm_states, first, B, d_stats, caller_stream);
}

} // extern "C"
