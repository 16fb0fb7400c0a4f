// popcheck.cpp -- TEST INFRASTRUCTURE.  Compiles what "population" (include/reinfocus_hip.h) adds to
// reinfocus_amd/csrc/rf_ppo.h in plain C++ for the host: the size rules rf_ppo_grouped_state_size and
// rf_ppo_grouped_workspace_size return, and the layout of the hyper-parameter record the grouped kernels read, so that a
// CPU-only test can hold them to the header's words and to the numpy packing (environments/population.py) before any GPU
// sees them.  Never loaded by the product package.
#include <stddef.h>
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_ppo.h"

using namespace rf;

extern "C" {

unsigned long long pop_state_size(const rf_policy_desc *desc, int G, int m)
{
    return population_state_bytes(*desc, G, m);
}

unsigned long long pop_workspace_size(const rf_policy_desc *desc, int G, int m, int T, int B)
{
    return population_workspace_bytes(*desc, G, m, T, B);
}

// byte offsets of PpoHyper's nine fields, then its size: 10 ints
void pop_hyper_layout(int *out)
{
    const size_t at[10] = {offsetof(PpoHyper, learning_rate), offsetof(PpoHyper, max_grad_norm), offsetof(PpoHyper, beta1),
                           offsetof(PpoHyper, beta2), offsetof(PpoHyper, adam_eps), offsetof(PpoHyper, clip),
                           offsetof(PpoHyper, ent), offsetof(PpoHyper, vf), offsetof(PpoHyper, normalize), sizeof(PpoHyper)};
    for (int i = 0; i < 10; ++i)
        out[i] = (int)at[i];
}

// rf_ppo_desc as the record of one group: 0, or -1 for what rf_ppo_update refuses
int pop_hyper(const rf_ppo_desc *ppo, void *record)
{
    PpoHyper h;
    if (!ppo_hyper(*ppo, h))
        return -1;
    *static_cast<PpoHyper *>(record) = h;
    return 0;
}
}
