// rf_abi_param_init.hip -- "parameter init" (include/reinfocus_hip.h): the packed parameters of G learners initialised on
// the device in two launches.  A translation unit of its own for the reason rf_abi_lstm_grouped.hip has one: no existing
// unit's listing changes with these kernels (profiles/param_init.md).
#include "rf_host.h"

#include "rf_param_init.h"

using namespace rfh;

namespace {

// the checked table of a call, or RF_ERR_INVALID with the message of what is wrong with it
int checked_table(const char *fn, const rf_param_segment *segments, int count, int groups, unsigned long long stride,
                  bool constants, rf::ParamTable &table)
{
    RF_REQUIRE(count >= 0 && count <= RF_PARAM_MAX_SEGMENTS, "%s: %d segments are not 0 .. %d (RF_PARAM_MAX_SEGMENTS)", fn,
               count, RF_PARAM_MAX_SEGMENTS);
    RF_REQUIRE(count == 0 || segments != nullptr, "%s: segments is NULL", fn);
    RF_REQUIRE(groups >= 1 && groups <= RF_POPULATION_MAX_GROUPS && stride >= 1 && stride <= (1ull << 30) &&
               (unsigned long long)groups * stride <= (1ull << 31),
               "%s: G = %d must be in 1 .. %d, stride = %llu in 1 .. 2^30 and G stride at most 2^31", fn, groups,
               RF_POPULATION_MAX_GROUPS, stride);
    const char *wrong = rf::param_table(segments, count, stride, constants, table);
    RF_REQUIRE(wrong == nullptr, "%s: %s", fn, wrong);
    return RF_OK;
}

} // namespace

extern "C" {

unsigned long long rf_params_init_workspace_size(rf_ctx *ctx, const rf_param_segment *segments, int count, int groups)
{
    if (ctx == nullptr)
        return 0;
    ignore_error(hipSetDevice(ctx->device));
    rf::ParamTable table;
    // (the stride is not this function's to know: the segments are held against the largest one)
    if (groups < 1 || groups > RF_POPULATION_MAX_GROUPS ||
        rf::param_table(segments, segments != nullptr ? count : 0, 1ull << 30, true, table) != nullptr ||
        (segments == nullptr && count != 0))
        return 0;
    return 8ull * (unsigned long long)groups * table.workspace;
}

int rf_params_init(rf_ctx *ctx, const rf_param_segment *segments, int count, int groups, unsigned stride, float *d_params,
                   const unsigned long long *d_gens, const unsigned char *d_select, const float *d_constants,
                   void *d_workspace, void *caller_stream)
{
    const char *fn = "rf_params_init";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_REQUIRE(d_params != nullptr && d_gens != nullptr, "%s: NULL argument", fn);
    rf::ParamTable table;
    if (int rc = checked_table(fn, segments, count, groups, stride, d_constants != nullptr, table))
        return rc;
    RF_REQUIRE(table.n_ortho == 0 || d_workspace != nullptr,
               "%s: RF_INIT_ORTHOGONAL segments need d_workspace (rf_params_init_workspace_size)", fn);
    RF_HIP(hipSetDevice(ctx->device));
    const size_t G = (size_t)groups;
    const DeviceArray inputs[] = {{d_gens, G * 32, 8, "d_gens"},
                                  {d_select, G, 1, "d_select"},
                                  {d_constants, G * 4, 4, "d_constants"}};
    const DeviceArray outputs[] = {{d_params, G * (size_t)stride * 4, 4, "d_params"},
                                   {table.n_ortho ? d_workspace : nullptr, G * (size_t)table.workspace * 8, 8, "d_workspace"}};
    if (int rc = check_device_arrays(ctx, inputs, outputs, fn))
        return rc;
    const hipStream_t caller = (hipStream_t)caller_stream;
    if (int rc = refuse_capturing(caller, fn))
        return rc;
    // Two launches on the caller's stream, nothing allocated, nothing waited for.  They write disjoint positions (the fill
    // kernel leaves orthogonal segments alone), so their order does not matter; the generators' words, the selection and
    // the constants are read on the device.
    static_assert(sizeof(rf::ParamGen) == 32, "d_gens is uint64 [G][4]");
    if (table.count > 0) {
        const unsigned blocks = (stride + (unsigned)rf::kParamThreads - 1) / (unsigned)rf::kParamThreads;
        hipLaunchKernelGGL(rf::param_fill_kernel, dim3(blocks, (unsigned)groups), dim3(rf::kParamThreads), 0, caller, table,
                           stride, d_params, (const rf::ParamGen *)d_gens, (const uint8_t *)d_select, d_constants);
        RF_HIP(hipGetLastError());
    }
    if (table.n_ortho > 0) {
        hipLaunchKernelGGL(rf::param_orthogonal_kernel, dim3((unsigned)table.n_ortho, (unsigned)groups),
                           dim3(rf::kParamThreads), 0, caller, table, stride, d_params, (const rf::ParamGen *)d_gens,
                           (const uint8_t *)d_select, (double *)d_workspace);
        RF_HIP(hipGetLastError());
    }
    return RF_OK;
}

} // extern "C"
