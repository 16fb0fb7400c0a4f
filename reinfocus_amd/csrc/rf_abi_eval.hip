// rf_abi_eval.hip -- "evaluation" (include/reinfocus_hip.h): the per-group scores of a population from the episode records,
// the copy that keeps the best rows, and the learner view's statistics to and from device memory.  A translation unit of
// its own for the reason rf_abi_param_init.hip has one: no existing unit's listing changes with these kernels
// (profiles/evaluation.md).
#include "rf_host.h"

#include "rf_eval.h"

using namespace rfh;

namespace rf {

// The moments of a learner view <-> a float64 [G][3][W + 1] tensor (mean, var, count), one thread per value.
__global__ void eval_statistics_kernel(EnvViewMoments *moments, double *tensor, int values, int w1, int set)
{
    const int at = blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= values)
        return;
    const int row = at / w1, column = at - row * w1;
    const int g = row / 3, which = row - 3 * g;
    double *slot = (which == 0 ? moments[g].mean : which == 1 ? moments[g].var : moments[g].count) + column;
    if (set)
        *slot = tensor[at];
    else
        tensor[at] = *slot;
}

} // namespace rf

namespace {

// the checked shape of a call, or RF_ERR_INVALID with the message of what is wrong with it
int checked_shape(const char *fn, int n, int groups, int m, int episodes, rf::EvalShape &shape)
{
    RF_REQUIRE(episodes >= 1, "%s: E = %d episodes: at least 1", fn, episodes);
    RF_REQUIRE(episodes <= RF_EVAL_MAX_EPISODES, "%s: E = %d episodes: at most %d (RF_EVAL_MAX_EPISODES)", fn, episodes,
               RF_EVAL_MAX_EPISODES);
    RF_REQUIRE(groups >= 1 && groups <= RF_POPULATION_MAX_GROUPS && m >= 1 && (long long)groups * m == (long long)n,
               "%s: n = %d is not G m = %d x %d (G in 1 .. %d, m >= 1)", fn, n, groups, m, RF_POPULATION_MAX_GROUPS);
    const int slots = rf::eval_slots(m, episodes);
    RF_REQUIRE((long long)n * slots <= (1ll << 31), "%s: n K = %d x %d slots exceed 2^31", fn, n, slots);
    shape = rf::EvalShape{groups, m, episodes, slots};
    return RF_OK;
}

int statistics_device(rf_ctx *ctx, double *d_tensor, bool set, void *caller_stream, const char *fn)
{
    // (the entry point has checked ctx and made its device current)
    RF_REQUIRE(ctx->env_ready && ctx->env_view, "%s: the context has no learner view (rf_env_configure_view)", fn);
    RF_REQUIRE(d_tensor != nullptr, "%s: NULL argument", fn);
    RF_REQUIRE(ctx->io_ev_in != nullptr && ctx->io_ev_out != nullptr,
               "%s: the context takes no device steps (rf_env_configure_initializer first)", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase or planned step is open", fn);
    const int G = ctx->view_groups > 0 ? ctx->view_groups : 1, w1 = ctx->env_obs_width + 1;
    const int values = G * 3 * w1;
    const DeviceArray tensor[] = {{d_tensor, (size_t)values * 8, 8, set ? "d_in" : "d_out"}};
    const DeviceArray none[] = {{nullptr, 0, 1, ""}};
    if (int rc = set ? check_device_arrays(ctx, tensor, none, fn) : check_device_arrays(ctx, none, tensor, fn))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // the moments are the context's stream's: it waits for the caller's, copies, and the caller's waits for it
    RF_HIP(hipEventRecord(ctx->io_ev_in, caller));
    RF_HIP(hipStreamWaitEvent(ctx->stream, ctx->io_ev_in, 0));
    hipLaunchKernelGGL(rf::eval_statistics_kernel, dim3((unsigned)(values + 255) / 256), dim3(256), 0, ctx->stream,
                       ctx->view_moments, d_tensor, values, w1, set ? 1 : 0);
    RF_HIP(hipGetLastError());
    RF_HIP(hipEventRecord(ctx->io_ev_out, ctx->stream));
    RF_HIP(hipStreamWaitEvent(caller, ctx->io_ev_out, 0));
    return RF_OK;
}

} // namespace

extern "C" {

int rf_eval_accumulate(rf_ctx *ctx, int n, int groups, int m, int episodes, const double *d_final_return,
                       const int *d_final_length, int *d_counts, double *d_returns, int *d_lengths, void *caller_stream)
{
    const char *fn = "rf_eval_accumulate";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(d_final_return != nullptr && d_final_length != nullptr && d_counts != nullptr && d_returns != nullptr &&
               d_lengths != nullptr, "%s: NULL argument", fn);
    rf::EvalShape shape;
    if (int rc = checked_shape(fn, n, groups, m, episodes, shape))
        return rc;
    RF_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n, cells = N * (size_t)shape.slots;
    const DeviceArray inputs[] = {{d_final_return, N * 8, 8, "d_final_return"}, {d_final_length, N * 4, 4, "d_final_length"}};
    const DeviceArray outputs[] = {{d_counts, N * 4, 4, "d_counts"},
                                   {d_returns, cells * 8, 8, "d_returns"},
                                   {d_lengths, cells * 4, 4, "d_lengths"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    const unsigned blocks = (unsigned)((N + (size_t)rf::kEvalThreads - 1) / (size_t)rf::kEvalThreads);
    hipLaunchKernelGGL(rf::eval_accumulate_kernel, dim3(blocks), dim3(rf::kEvalThreads), 0, caller, shape, d_final_return,
                       d_final_length, d_counts, d_returns, d_lengths);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_eval_finish(rf_ctx *ctx, int n, int groups, int m, int episodes, unsigned long long serial, const int *d_counts,
                   const double *d_returns, const int *d_lengths, double *d_results, double *d_best_mean,
                   long long *d_best_serial, unsigned char *d_improved, void *caller_stream)
{
    const char *fn = "rf_eval_finish";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(d_counts != nullptr && d_returns != nullptr && d_lengths != nullptr && d_results != nullptr &&
               d_best_mean != nullptr && d_best_serial != nullptr && d_improved != nullptr, "%s: NULL argument", fn);
    rf::EvalShape shape;
    if (int rc = checked_shape(fn, n, groups, m, episodes, shape))
        return rc;
    RF_REQUIRE(serial < (1ull << 53), "%s: the serial %llu is not below 2^53 (it is reported as a float64)", fn, serial);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t N = (size_t)n, cells = N * (size_t)shape.slots, G = (size_t)groups;
    const DeviceArray inputs[] = {{d_counts, N * 4, 4, "d_counts"},
                                  {d_returns, cells * 8, 8, "d_returns"},
                                  {d_lengths, cells * 4, 4, "d_lengths"}};
    const DeviceArray outputs[] = {{d_results, G * 64, 8, "d_results"},
                                   {d_best_mean, G * 8, 8, "d_best_mean"},
                                   {d_best_serial, G * 8, 8, "d_best_serial"},
                                   {d_improved, G, 1, "d_improved"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    hipLaunchKernelGGL(rf::eval_finish_kernel, dim3((unsigned)groups), dim3(rf::kEvalThreads), 0, caller, shape, serial,
                       rf::eval_leaves(episodes), d_counts, d_returns, d_lengths, d_results, d_best_mean, d_best_serial,
                       (uint8_t *)d_improved);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_eval_keep_rows(rf_ctx *ctx, int groups, unsigned words, unsigned stride, const unsigned char *d_select,
                      const void *d_src, void *d_dst, void *caller_stream)
{
    const char *fn = "rf_eval_keep_rows";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(d_select != nullptr && d_src != nullptr && d_dst != nullptr, "%s: NULL argument", fn);
    RF_REQUIRE(groups >= 1 && groups <= RF_POPULATION_MAX_GROUPS && words >= 1 && words <= stride &&
               (unsigned long long)groups * stride <= (1ull << 31),
               "%s: G = %d must be in 1 .. %d, words = %u in 1 .. stride = %u and G stride at most 2^31", fn, groups,
               RF_POPULATION_MAX_GROUPS, words, stride);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t G = (size_t)groups, bytes = ((G - 1) * (size_t)stride + (size_t)words) * 4;
    const DeviceArray inputs[] = {{d_select, G, 1, "d_select"}, {d_src, bytes, 4, "d_src"}};
    const DeviceArray outputs[] = {{d_dst, bytes, 4, "d_dst"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // 16-byte vectors where a row of d_src reaches a 16-byte boundary with the same word as that row of d_dst
    const int vec = (((uintptr_t)d_src ^ (uintptr_t)d_dst) & 15) == 0;
    const unsigned blocks = (words + (unsigned)rf::kEvalThreads * 4 - 1) / ((unsigned)rf::kEvalThreads * 4);
    hipLaunchKernelGGL(rf::eval_keep_rows_kernel, dim3(blocks, (unsigned)groups), dim3(rf::kEvalThreads), 0, caller, words,
                       stride, vec, (const uint8_t *)d_select, (const uint32_t *)d_src, (uint32_t *)d_dst);
    RF_HIP(hipGetLastError());
    return RF_OK;
}

int rf_env_view_get_statistics_device(rf_ctx *ctx, double *d_out, void *caller_stream)
{
    const char *fn = "rf_env_view_get_statistics_device";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_HIP(hipSetDevice(ctx->device));
    return statistics_device(ctx, d_out, false, caller_stream, fn);
}

int rf_env_view_set_statistics_device(rf_ctx *ctx, const double *d_in, void *caller_stream)
{
    const char *fn = "rf_env_view_set_statistics_device";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_HIP(hipSetDevice(ctx->device));
    return statistics_device(ctx, const_cast<double *>(d_in), true, caller_stream, fn);
}

} // extern "C"
