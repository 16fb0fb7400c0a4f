// rf_env_types.h -- configuration and device arrays of the device-resident environment step (kernels: rf_env.h)
#pragma once

#include <stdint.h>

#include "../../include/reinfocus_hip.h" // rf_env_observer_program: the kernels read it as the host wrote it

namespace rf {

// EnvConfig::task: which of the reference's two tasks (examples/__init__.py:6-18) the step computes.  Both share the
// ender, the observer, the scene packing, the auto-reset, the render and the focus measure; they differ in the
// transformer and the rewarder only.  The branch is on a kernel argument: uniform over every launch.
constexpr int kEnvTaskSteps = 0; // DiscreteSteps-v0: int32 action indices into action_set, Delta + Observation + OnTarget
constexpr int kEnvTaskJumps = 1; // ContinuousJumps-v0: float32 actions in [-1, 1], Observation + Stopped * OnTarget
constexpr int kEnvTaskComposed = 2; // any composition of the reference's strategy classes: EnvState::program

// The strategy program of kEnvTaskComposed (rf_env_program, include/reinfocus_hip.h), as the kernels read it: uploaded
// once by rf_env_configure_composed, with every parameter already rounded to the type numpy computes it in.  Every
// thread reads the same entries (through the constant address space: scalar loads).  EnvConfig, which every launch
// takes by value and the replayed graphs capture, does not grow.
constexpr int kEnvMaxLeaves = 8, kEnvMaxOps = 2 * kEnvMaxLeaves - 1;

struct EnvEnderLeaf {
    int kind, i0, i1, steps; // RF_ENDER_*, check indices, early_end_steps / max_steps
    float threshold;         // float32(threshold / early_end_radius / early_end_span)
    int history;             // StoppedEnder: first row of its history in EnvState::history (steps + 1 rows)
};

struct EnvRewardLeaf {
    int kind, i0, i1;        // RF_REWARD_*, check indices / observation index
    float f[3];              // float32 parameters: Delta reward, scale | Distance span, high - low, low | OnTarget span
                             // | Stopped threshold
    double d[2];             // float64 parameters: OnTarget on - off, off | Stopped reward
};

struct EnvProgram {
    int transformer, move_index, n_actions;
    float limit_lo, limit_hi;       // float32(limits): the clip limits; ContinuousJump: limit_lo is where a jump starts
    float jump_span;                // ContinuousJump: float32(hi - lo), the difference taken in float64
    float speed, stop_threshold;    // float32
    double move64[32];              // DiscreteMove
    float jump32[32];               // DiscreteJump
    int n_enders, n_ender_ops, n_rewarders, n_reward_ops;
    EnvEnderLeaf enders[kEnvMaxLeaves];
    int ender_ops[kEnvMaxOps];
    EnvRewardLeaf rewarders[kEnvMaxLeaves];
    int reward_ops[kEnvMaxOps];
    int reward_f64[kEnvMaxOps];
    int history_rows;               // rows of EnvState::history
};

struct EnvConfig {
    int task;                 // kEnvTaskSteps / kEnvTaskJumps / kEnvTaskComposed
    int n;                    // environments
    int n_actions;
    double action_set[32];    // float64 moves (state_transformer.py:246 numpy.asarray(action_set))
    float limit_lo, limit_hi; // clip limits (kEnvTaskSteps); the range the focus plane jumps in (kEnvTaskJumps)
    float stop_threshold;     // kEnvTaskJumps: ContinuousJumpTransformer / StoppedRewarder threshold (target_radius / 2)
    int max_steps;            // <= 0: no time limit (single-env DiscreteSteps)
    float diverge_threshold;  // target_radius / 2
    int early_end_steps;
    float mid[4], scale[4];   // NormalizedObserver (float32)
    float reward_scale;       // DeltaRewarder scale (target_radius * 2)
    float on_target_span;     // OnTargetRewarder span
    // camera / world packing
    double half_width, half_height, tan_half_r; // Python floats
    float look_from[3], cam_u[3], cam_v[3], cam_w[3];
    unsigned long long frame_pixels; // h * w of the frames the focus measure reduces
};

struct EnvState {            // all device arrays, length n unless noted
    float *state;            // [n][2] target, focus
    int *steps;              // TimeLimitEnder._steps
    int *diverging;          // DivergingEnder._diverging_steps
    float *last_diff;        // DivergingEnder._last_diff
    float *old_wrapped;      // [n][2] DeltaObserver._old_wrapped_observations
    float *old_focus;        // DeltaRewarder._old_states (kEnvTaskJumps: StoppedRewarder._old_states, same rules)
    // per-step scratch / outputs
    float *cam_dyn, *rect;   // scene of all n envs
    float *cam_dyn2, *rect2; // compacted scene of the envs that reset this step
    int *done_index;         // [n] env index of the r-th reset env
    int *done_rank;          // [n] the inverse for the envs that ended (fused step)
    int *done_count;         // [1]
    float *obs;              // [n][4]; [n][W] with an observer program
    double *reward;          // [n]
    uint8_t *truncated;      // [n]
    uint8_t *done;           // [n] scratch
    unsigned long long *sums; // [n][2] the focus measure's (sum, sum of squares): zeroed here before a measure, read after
    unsigned long long *sums2; // [n][2] the same for the re-rendered frames of a fused step (both measures are one launch there)
    // kEnvTaskComposed only (null otherwise): the program and the per-leaf strategy state, leaf-major ([leaf][n])
    const EnvProgram *program;
    int *leaf_count;         // [n_enders][n] Diverging / OnTarget / TimeLimit counters
    float *leaf_float;       // [n_enders][n] DivergingEnder._last_diff
    float *history;          // [history_rows][n] StoppedEnder histories, oldest first, NaN where empty
    float *leaf_old;         // [n_rewarders][n] Delta / Stopped: the element's previous value
    // rf_env_configure_observed only (null otherwise: the built-in observer of mid / scale / old_wrapped above)
    const rf_env_observer_program *observer; // read like `program`; every value in it is float32 or an index already
    float *obs_old;          // [n_old][n] the DELTA nodes' old values, node-major, NaN until the first reset
    // rf_env_configure_records only (all five null otherwise: a uniform branch on a kernel argument, as `observer`)
    double *ep_return;       // [n] state: the rewards of the running episode, added in step order
    int *ep_length;          // [n] state: its steps
    float *final_obs;        // [n][W] output of every step: the row of `obs` before the auto-reset overwrote it where
                             // the environment ended, NaN elsewhere
    double *final_return;    // [n] output: ep_return where the environment ended, NaN elsewhere
    int *final_length;       // [n] output: ep_length where it ended, 0 elsewhere
};

// The learner view (rf_env_configure_view; kernels in rf_env_view.h)
constexpr int kViewMaxColumns = 16; // RF_ENV_MAX_OBS_COLUMNS
constexpr int kViewSlots = kViewMaxColumns + 1; // the observation columns 0 .. W-1, then the returns at index W

// Running moments in float64, as the device keeps them (and a snapshot holds them): slot c < W is observation column
// c, slot W the discounted returns.
struct EnvViewMoments {
    double mean[kViewSlots], var[kViewSlots], count[kViewSlots];
};

// What both kernels of the view take by value.  Everything is uniform: a scalar.
struct EnvViewConfig {
    int n, width, frame_stack; // V = frame_stack * width
    int norm_obs, norm_reward;
    double gamma, epsilon, clip_obs, clip_reward;
};

// The groups of a grouped view (rf_env_configure_view_grouped; "population view"): group g owns lanes [g m, (g + 1) m)
// and moments[g]; its returns are discounted by gamma[g].  Read by the kGrouped instantiations of the view's kernels
// only; all zero without groups.
struct EnvViewGroups {
    int groups, m;       // m = n / groups
    int log2_pm;         // P_m = 1 << log2_pm, the next power of two >= m
    const double *gamma; // [groups], device memory
};

} // namespace rf
