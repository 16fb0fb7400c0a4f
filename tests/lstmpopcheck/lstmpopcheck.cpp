// lstmpopcheck.cpp -- TEST INFRASTRUCTURE.  Compiles what "population lstm" (include/reinfocus_hip.h) adds to
// reinfocus_amd/csrc/rf_lstm.h and rf_lstm_ppo.h in plain C++ for the host: the size rules
// rf_lstm_ppo_grouped_state_size and rf_lstm_ppo_grouped_workspace_size return, and the grouped addressing helpers the
// kernels walk their sequences and reach the single-form state with, so that a CPU-only test can hold them to the header's
// words and to the restated sequence rule per group before any GPU sees them.  Never loaded by the product package.
#include <stddef.h>
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_lstm_ppo.h"

using namespace rf;

extern "C" {

unsigned long long lpop_state_size(const rf_lstm_critic_desc *desc, int G, int m)
{
    return lstm_population_state_bytes(*desc, G, m);
}

unsigned long long lpop_workspace_size(const rf_lstm_critic_desc *desc, int G, int m, int T, int B)
{
    return lstm_population_workspace_bytes(*desc, G, m, T, B);
}

// firsts[g] as the kernels take it, and whether it sets the group's skip flag
int lpop_first(int raw, int N, int *outside)
{
    const int first = lstm_ppo_first(raw, N);
    *outside = raw != first ? 1 : 0;
    return first;
}

// The sequence rule of group g of G groups of m environments over the single-form episode_starts [T + 1][G m]:
// rows[b] = r_b (local to the group), start[b] = 1 where row b starts a sequence, end[b] = one past its sequence's last
// row (start rows only, else 0), lane[b] = the column of episode_starts and lstm_states the row's environment is
int lpop_sequences(const uint8_t *starts, int G, int m, int g, int T, int raw_first, int B, int *rows, int *start, int *end,
                   int *lane)
{
    const LstmLanes at = lstm_group_lanes(G, m, g);
    const int first = lstm_ppo_first(raw_first, T * m);
    for (int b = 0; b < B; ++b) {
        rows[b] = lstm_ppo_row(first, b, T * m);
        start[b] = lstm_ppo_is_start(starts, T, m, first, b, at) ? 1 : 0;
        end[b] = start[b] ? lstm_ppo_end(starts, T, m, first, b, B, at) : 0;
        lane[b] = at.lane0 + rows[b] / T;
    }
    return at.lanes;
}

// offset in floats of element (t, net, which, environment e of group g, unit) of lstm_states [T + 1][2][2][G m][H]
unsigned long long lpop_state_at(int G, int m, int g, int H, int t, int net, int which, int e, int unit)
{
    const LstmLanes at = lstm_group_lanes(G, m, g);
    return lstm_ppo_state_at(t, net, which, at.lanes, H, at.lane0 + e, unit);
}
}
