// iocheck.cpp -- TEST INFRASTRUCTURE.  Compiles the action rules of a device step (reinfocus_amd/csrc/rf_env_io.h, the
// exact text env_gather_actions_kernel inlines) for the host, so that a CPU-only test can compare them with a numpy
// statement of the rules before any GPU sees them.  Never loaded by the product package.
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_env_io.h"

using namespace rf;

extern "C" {

// count actions of the launch's dtype (kActionI32 / I64 / F32) under `rule` (kActionRule*), as the kernel's lanes judge
// them: stored[i] := the 4-byte slot (a float32's bits under the float rules), valid[i] := 0 / 1.  Returns the fault
// word a launch of these actions at `step` would leave (kNoFault: none).
uint64_t io_gather(const void *actions, int dtype, int rule, int n_actions, int count, uint32_t step, int32_t *stored,
                   uint8_t *valid)
{
    unsigned long long fault = kNoFault;
    for (int e = 0; e < count; ++e) {
        bool ok;
        int32_t slot;
        if (dtype == kActionF32) {
            const float a = ((const float *)actions)[e];
            float value;
            ok = rule == kActionRuleJump ? io_jump_action(a, value) : io_finite_action(a, value);
            __builtin_memcpy(&slot, &value, 4);
        } else {
            const int64_t a = dtype == kActionI64 ? ((const int64_t *)actions)[e] : (int64_t)((const int32_t *)actions)[e];
            ok = io_index_action(a, n_actions, slot);
        }
        stored[e] = slot;
        valid[e] = ok ? 1 : 0;
        const unsigned long long key = io_fault_key(step, (unsigned)e);
        if (!ok && key < fault)
            fault = key;
    }
    return fault;
}

} // extern "C"
