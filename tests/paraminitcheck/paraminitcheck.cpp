// paraminitcheck.cpp -- TEST INFRASTRUCTURE.  Compiles the parameter initialiser's arithmetic
// (reinfocus_amd/csrc/rf_param_init.h: the checked table, the fill value and the steps of the orthogonal scheme) for the
// host, with plain loops in place of the two kernels' threads, so that a CPU-only test can compare the definition with the
// numpy twin (environments/param_init.py) before any GPU sees it.  Never loaded by the product package.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../reinfocus_amd/csrc/rf_param_init.h"

using namespace rf;

namespace {

// param_orthogonal_kernel's block (segment, group): thread a is the iteration a of each loop over components
void orthogonal(const rf_param_segment &seg, const uint64_t gen[4], float *packed, double *work)
{
    const int t = param_ortho_t(seg), s = param_ortho_s(seg);
    double *q_vector = work, *q_component = work + param_cells(seg);
    std::vector<double> v(t), next(t), c(s);
    for (int b = 0; b < s; ++b) {
        for (int a = 0; a < t; ++a)
            v[a] = (double)param_ortho_draw(seg, gen, a, b);
        for (int pass = 0; pass < 2; ++pass) {
            for (int p = 0; p < b; ++p)
                c[p] = param_ortho_dot(q_component + p, s, v.data(), t);
            for (int a = 0; a < t; ++a)
                next[a] = param_ortho_project(v[a], c.data(), q_vector + a, t, b);
            v = next;
        }
        const double n2 = param_ortho_norm2(v.data(), t);
        for (int a = 0; a < t; ++a) {
            const double q = param_ortho_unit(v[a], n2);
            q_vector[(size_t)b * (size_t)t + a] = q;
            q_component[(size_t)a * (size_t)s + b] = q;
        }
    }
    for (int p = 0; p < s; ++p)
        for (int a = 0; a < t; ++a)
            packed[param_ortho_packed_at(seg, p, a)] = param_ortho_packed(q_vector[(size_t)p * (size_t)t + a], seg.scale);
}

} // namespace

extern "C" {

// rf_params_init_workspace_size over one group, in doubles; -1 for a refused table
long long pic_workspace_doubles(const rf_param_segment *segments, int count, unsigned stride)
{
    ParamTable table;
    return param_table(segments, count, stride, true, table) == nullptr ? (long long)table.workspace : -1;
}

// rf_params_init on host arrays: 0, or -1 with what param_table says in `message`
int pic_params_init(const rf_param_segment *segments, int count, int groups, unsigned stride, float *params,
                    const uint64_t *gens /* [G][4] */, const uint8_t *select, const float *constants, char *message, int cap)
{
    ParamTable table;
    const char *wrong = param_table(segments, count, stride, constants != nullptr, table);
    if (wrong != nullptr) {
        snprintf(message, (size_t)cap, "%s", wrong);
        return -1;
    }
    std::vector<double> workspace(table.workspace);
    for (int g = 0; g < groups; ++g) {
        if (select != nullptr && select[g] == 0)
            continue;
        float *mine = params + (size_t)g * stride;
        const uint64_t *gen = gens + 4 * (size_t)g;
        for (unsigned i = 0; i < stride; ++i) {
            const int k = param_find(table, i);
            if (k >= 0 && table.seg[k].scheme != RF_INIT_ORTHOGONAL)
                mine[i] = param_fill_value(table.seg[k], gen, i, constants != nullptr ? constants[g] : 0.0f);
        }
        for (int x = 0; x < table.n_ortho; ++x) {
            const rf_param_segment &seg = table.seg[table.ortho[x]];
            orthogonal(seg, gen, mine + seg.at, workspace.data() + table.ortho_at[x]);
        }
    }
    return 0;
}

} // extern "C"
