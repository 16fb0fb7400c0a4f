// rf_env_io.h -- the boundary of a device step (rf_env_step_device): the caller's actions are taken where they are, in
// device memory and in the dtype a policy network produces, checked there, and the step's results are handed to the
// caller's device arrays.  No host copy, no host synchronisation.
//
// The rules are check_actions' (rf_abi_env.hip), moved to the device.  A host form refuses a step with an invalid
// action before anything runs; a device step cannot, because nobody looks at the actions before they are used.  So
// every rule here has two halves: whether the action is valid, and the value the step uses in its place when it is
// not.  That replacement exists only so that no kernel indexes the action set out of bounds or carries a NaN into the
// states: the trajectory after an invalid action is not a valid one, and the context says so once somebody asks
// (rf_env_device_status).
//
// The three functions are plain C++ like rf_init.h, so that tests/iocheck compiles the very same text for the host.
#pragma once

#include <stdint.h>

#include "rf_math.h" // RF_HD

namespace rf {

// rf_env_step_device's action_dtype (RF_ACTION_* of include/reinfocus_hip.h)
constexpr int kActionI32 = 0, kActionI64 = 1, kActionF32 = 2;
// what the float rules of a context are: a jump (ContinuousJumps, a composed ContinuousJumpTransformer) takes [-1, 1],
// every other continuous transformer any finite value
constexpr int kActionRuleIndex = 0, kActionRuleJump = 1, kActionRuleFinite = 2;

constexpr unsigned long long kNoFault = ~0ull;

// An index into the action set, judged on the full 64-bit value: 2^32 + 1 is invalid, not 1.
RF_HD bool io_index_action(int64_t a, int n_actions, int32_t &stored)
{
    const bool valid = a >= 0 && a < (int64_t)n_actions;
    stored = valid ? (int32_t)a : (a < 0 ? 0 : n_actions - 1);
    return valid;
}

// A jump in [-1, 1]: NaN becomes 0, everything else outside is clamped.
RF_HD bool io_jump_action(float a, float &stored)
{
    const bool valid = a >= -1.0f && a <= 1.0f; // (false for NaN)
    stored = valid ? a : (a != a ? 0.0f : (a < -1.0f ? -1.0f : 1.0f));
    return valid;
}

// Any finite value (a ContinuousMoveTransformer clips it itself): NaN and the infinities become 0.
RF_HD bool io_finite_action(float a, float &stored)
{
    const bool valid = (a - a) == 0.0f; // (NaN for NaN and the infinities)
    stored = valid ? a : 0.0f;
    return valid;
}

// the 64-bit key an invalid action leaves in the fault word: the smallest key is the earliest step, and the lowest
// environment within it
RF_HD unsigned long long io_fault_key(unsigned step, unsigned env)
{
    return ((unsigned long long)step << 32) | (unsigned long long)env;
}

} // namespace rf

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace rf {

// What the context keeps in device memory for its device steps (one allocation, ctx->d_io_state).
struct EnvIoState {
    unsigned long long fault;       // kNoFault, or the smallest io_fault_key of an invalid action since the last reset
    unsigned long long env_renders; // environments rendered by device steps: n + k each (pixels = that x frame pixels)
};

// One lane per environment: the caller's action e (dtype: kActionI32 / I64 / F32, uniform over the launch; rule:
// kActionRule*) into the 4-byte slot the step kernels read.  Consecutive lanes read consecutive elements (4 or 8
// bytes a lane) and write consecutive slots.  An invalid action leaves its key in the fault word with one 64-bit
// atomicMin (a vector atomic; valid launches issue none).  `step` is a kernel argument: the launch is never part of a
// replayed graph.
__global__ void env_gather_actions_kernel(const void *actions, int dtype, int rule, int n_actions, int n, unsigned step,
                                          int *slots, EnvIoState *io)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n)
        return;
    bool valid;
    int32_t slot;
    if (dtype == kActionF32) {
        const float a = ((const float *)actions)[e];
        float stored;
        valid = rule == kActionRuleJump ? io_jump_action(a, stored) : io_finite_action(a, stored);
        slot = __builtin_bit_cast(int32_t, stored);
    } else {
        const int64_t a = dtype == kActionI64 ? ((const int64_t *)actions)[e] : (int64_t)((const int32_t *)actions)[e];
        valid = io_index_action(a, n_actions, slot);
    }
    slots[e] = slot;
    if (!valid)
        atomicMin(&io->fault, io_fault_key(step, (unsigned)e));
}

// The step's results from the context's io block into the caller's arrays, as one launch: a grid-stride copy of
// observations (n x width floats), rewards, flags and -- thread 0 -- the count of environments that ended, which also
// goes into the running total the host accounts its pixels from once it asks.  Runs after the step on the same
// stream, outside the replayed graph: the caller's pointers may differ from call to call.  The episode records
// (final_obs / final_return / final_length, rf_env_step_device_records) go along in the same launch to whichever of
// out_final_obs / out_final_return / out_final_length is not null -- kernel arguments: uniform branches.
__global__ void env_scatter_results_kernel(const float *obs, const double *reward, const uint8_t *truncated,
                                           const int *done_count, int n, int width, float *out_obs, double *out_reward,
                                           uint8_t *out_truncated, int *out_count, EnvIoState *io, const float *final_obs,
                                           const double *final_return, const int *final_length, float *out_final_obs,
                                           double *out_final_return, int *out_final_length)
{
    const int stride = gridDim.x * blockDim.x, first = blockIdx.x * blockDim.x + threadIdx.x;
    const int cells = n * width;
    for (int i = first; i < cells; i += stride)
        out_obs[i] = obs[i];
    if (out_final_obs)
        for (int i = first; i < cells; i += stride)
            out_final_obs[i] = final_obs[i];
    for (int i = first; i < n; i += stride) {
        out_reward[i] = reward[i];
        out_truncated[i] = truncated[i];
        if (out_final_return)
            out_final_return[i] = final_return[i];
        if (out_final_length)
            out_final_length[i] = final_length[i];
    }
    if (first == 0) {
        const int k = *done_count;
        if (out_count)
            *out_count = k;
        io->env_renders += (unsigned long long)(n + k);
    }
}

// rf_env_reset_device: the observations alone
__global__ void env_scatter_obs_kernel(const float *obs, int cells, float *out_obs)
{
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += stride)
        out_obs[i] = obs[i];
}

} // namespace rf
#endif
