// rf_param_init.h -- the initialiser of packed learner parameters (include/reinfocus_hip.h, "parameter init"): PyTorch's
// default initialisation and stable-baselines3's orthogonal one, for G groups in two launches.  Head-agnostic: the host
// describes a packed array as at most RF_PARAM_MAX_SEGMENTS segments, and the kernels know nothing of a network.
//
//   param_fill_kernel        grid (ceil(stride / 256), G): one thread per packed position; it finds its segment in the
//                            by-value table and writes ZERO / CONSTANT / UNIFORM.  Positions of ORTHOGONAL segments and
//                            positions outside every segment are left alone.
//   param_orthogonal_kernel  grid (orthogonal segments, G), 256 threads: the Q of the sign-fixed QR of a t x s matrix of
//                            normal32 draws, by Gram-Schmidt with the projection step done twice (CGS2) in the fixed
//                            float64 order of the header, rounded to float32 once.  Thread a owns component a of every vector.
// A group whose select byte is 0 writes nothing (null selects every group).  Packed position i of group g is computed from
// draw number i of the group's generator (policy_draw's jump-ahead), so no result depends on the launch shape.
//
// The scalar arithmetic is plain C++ (RF_HD): tests/paraminitcheck loops over the same functions on the host, and the numpy
// twin is environments/param_init.py.  Nothing is contracted (flags.mk); the divide and sqrtf are correctly rounded.
#pragma once

#include "rf_policy_math.h" // policy_draw, normal32

#include "../../include/reinfocus_hip.h"

namespace rf {

constexpr int kParamThreads = 256;

struct ParamGen {
    uint64_t word[4]; // state low, state high, inc low, inc high (rf_policy.h's PolicyGen)
};
static_assert(RF_POLICY_MAX_WIDTH <= kParamThreads, "one thread per component of an orthogonal segment's vectors");

// What the kernels take by value: the checked segments, and which of them are orthogonal (block x of
// param_orthogonal_kernel works on segment ortho[x], with its vectors at workspace double ortho_at[x] of the group's piece)
struct ParamTable {
    rf_param_segment seg[RF_PARAM_MAX_SEGMENTS];
    int count;
    int n_ortho;
    unsigned char ortho[RF_PARAM_MAX_SEGMENTS];
    unsigned ortho_at[RF_PARAM_MAX_SEGMENTS];
    unsigned workspace; // doubles of one group's piece of the workspace
};

RF_HD bool param_finite(double x)
{
    return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308;
}

RF_HD unsigned param_cells(const rf_param_segment &s)
{
    return (unsigned)s.out * (unsigned)s.in;
}

// The table of `count` segments over a packed array of `stride` floats, or what is wrong with them (null: nothing).
// Segments may come in any order and need not cover the array.
RF_HD const char *param_table(const rf_param_segment *segments, int count, unsigned long long stride, bool constants,
                              ParamTable &t)
{
    if (count < 0 || count > RF_PARAM_MAX_SEGMENTS)
        return "more segments than RF_PARAM_MAX_SEGMENTS";
    t.count = count;
    t.n_ortho = 0;
    t.workspace = 0;
    for (int i = 0; i < count; ++i) {
        const rf_param_segment &s = segments[i];
        if (s.out < 1 || s.out > RF_POLICY_MAX_WIDTH || s.in < 1 || s.in > RF_POLICY_MAX_WIDTH)
            return "a segment's out or in is outside 1 .. RF_POLICY_MAX_WIDTH";
        if ((unsigned long long)s.at + param_cells(s) > stride)
            return "a segment is out of range (at + out in exceeds the stride)";
        if (s.scheme != RF_INIT_ZERO && s.scheme != RF_INIT_CONSTANT && s.scheme != RF_INIT_UNIFORM &&
            s.scheme != RF_INIT_ORTHOGONAL)
            return "a segment's scheme is unknown";
        if ((s.scheme == RF_INIT_UNIFORM || s.scheme == RF_INIT_ORTHOGONAL) && !(param_finite(s.scale) && s.scale > 0.0))
            return "the scale of a UNIFORM or ORTHOGONAL segment is not finite and positive";
        if (s.scheme == RF_INIT_CONSTANT && !constants)
            return "a CONSTANT segment needs d_constants";
        for (int j = 0; j < i; ++j) {
            const rf_param_segment &o = segments[j];
            if (s.at < o.at + param_cells(o) && o.at < s.at + param_cells(s))
                return "two segments overlap";
        }
        t.seg[i] = s;
        if (s.scheme == RF_INIT_ORTHOGONAL) {
            t.ortho[t.n_ortho] = (unsigned char)i;
            t.ortho_at[t.n_ortho] = t.workspace;
            t.n_ortho += 1;
            t.workspace += 2u * param_cells(s); // (param_ortho_doubles)
        }
    }
    return nullptr;
}

// The segment that holds packed position i, or -1
RF_HD int param_find(const ParamTable &t, unsigned i)
{
    for (int k = 0; k < t.count; ++k)
        if (i >= t.seg[k].at && i - t.seg[k].at < param_cells(t.seg[k]))
            return k;
    return -1;
}

// RF_INIT_UNIFORM: float32((2 u - 1) scale), float64 inside: one multiply, one subtract, one multiply, one rounding
RF_HD float param_uniform(double u, double scale)
{
    return (float)((2.0 * u - 1.0) * scale);
}

// What param_fill_kernel stores at packed position i of segment s (not an orthogonal one)
RF_HD float param_fill_value(const rf_param_segment &s, const uint64_t gen[4], unsigned i, float constant)
{
    if (s.scheme == RF_INIT_UNIFORM)
        return param_uniform(policy_draw(gen, (uint64_t)i), s.scale);
    return s.scheme == RF_INIT_CONSTANT ? constant : 0.0f;
}

// ---- RF_INIT_ORTHOGONAL.  t = max(out, in) components, s = min(out, in) vectors.  The chains are float64: in float32 they
// miss the orthogonality the header asks for from 64 x 64 on (profiles/param_init.md), and so does keeping the finished
// vectors as float32.  Vector p's component a is therefore kept as a double, twice, in the workspace while the segment is
// worked on: at p t + a ("by vector": what thread a walks when it subtracts projections) and, after the t s doubles of
// that, at a s + p ("by component": what thread p walks when it takes its dot product) -- consecutive doubles across
// threads in both.  The destination is written once, at the end, rounded and scaled.
RF_HD int param_ortho_t(const rf_param_segment &s) { return s.out > s.in ? s.out : s.in; }
RF_HD int param_ortho_s(const rf_param_segment &s) { return s.out > s.in ? s.in : s.out; }
RF_HD unsigned param_ortho_doubles(const rf_param_segment &s) { return 2u * param_cells(s); }

// out >= in: W^T[k][j] = scale q_k[j] (vector k, component j: packed k out + j = p t + a); out < in: W^T[k][j] =
// scale q_j[k] (vector j, component k: packed k out + j = a s + p)
RF_HD size_t param_ortho_packed_at(const rf_param_segment &seg, int p, int a)
{
    return seg.out >= seg.in ? (size_t)p * (size_t)param_ortho_t(seg) + (size_t)a
                             : (size_t)a * (size_t)param_ortho_s(seg) + (size_t)p;
}

// A[a][b]: the draw of packed position at + a s + b
RF_HD float param_ortho_draw(const rf_param_segment &seg, const uint64_t gen[4], int a, int b)
{
    return normal32(policy_draw(gen, (uint64_t)seg.at + (uint64_t)a * (uint64_t)param_ortho_s(seg) + (uint64_t)b));
}

// c_p = the sum over a ascending, from +0, of q_p[a] * v[a] (by_component + p: vector p's components, `s` doubles apart)
RF_HD double param_ortho_dot(const double *q, int s, const double *v, int t)
{
    double c = 0.0;
    for (int a = 0; a < t; ++a)
        c = c + q[(size_t)a * (size_t)s] * v[a];
    return c;
}

// v[a] - c_0 q_0[a] - c_1 q_1[a] ... for p ascending below b (by_vector + a: component a of the vectors, `t` doubles apart)
RF_HD double param_ortho_project(double v, const double *c, const double *q, int t, int b)
{
    for (int p = 0; p < b; ++p)
        v = v - c[p] * q[(size_t)p * (size_t)t];
    return v;
}

// n2 = the same chain over v[a] * v[a]
RF_HD double param_ortho_norm2(const double *v, int t)
{
    double n2 = 0.0;
    for (int a = 0; a < t; ++a)
        n2 = n2 + v[a] * v[a];
    return n2;
}

// q_b[a] of v[a]; the column is all zeros where !(n2 > 0)
RF_HD double param_ortho_unit(double v, double n2)
{
    return n2 > 0.0 ? v / sqrt(n2) : 0.0;
}

// what is stored: float32(scale) * float32(q), one float32 multiply
RF_HD float param_ortho_packed(double q, double scale)
{
    return (float)scale * (float)q;
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(kParamThreads) void param_fill_kernel(ParamTable table, unsigned stride, float *params,
                                                                   const ParamGen *__restrict__ gens /* [G] */,
                                                                   const uint8_t *__restrict__ select /* [G] or null */,
                                                                   const float *__restrict__ constants /* [G] or null */)
{
    const size_t g = blockIdx.y;
    if (select != nullptr && select[g] == 0) // (block-uniform)
        return;
    const unsigned i = blockIdx.x * (unsigned)kParamThreads + threadIdx.x;
    if (i >= stride)
        return;
    // (the walk of param_find, with k uniform so that the table is read from the kernel's arguments by scalar loads)
    for (int k = 0; k < table.count; ++k) {
        const rf_param_segment &seg = table.seg[k];
        if (i >= seg.at && i - seg.at < param_cells(seg)) {
            if (seg.scheme != RF_INIT_ORTHOGONAL) {
                const ParamGen gen = gens[g];
                params[g * (size_t)stride + i] =
                    param_fill_value(seg, gen.word, i, constants != nullptr ? constants[g] : 0.0f);
            }
            return;
        }
    }
}

// Block (x, g): orthogonal segment x of group g.  Thread a < t owns component a: it draws A[a][b], keeps v[a] in a register
// and in LDS, where the others read it as a broadcast, and stores q_b[a] in both layouts; thread p < b owns c_p.  Per pass
// two barriers (after the c's, after the v's) and one per column after the draw; s_v is double-buffered by the column's
// parity so that the next column's draw does not wait for the threads still summing n2.  The finished vectors are read
// back through the caches: every store of one is followed by a barrier before another thread loads it (__syncthreads
// orders the block's global stores, and a block lives on one CU), and no load of them is uniform.  No atomics, no scratch.
__global__ __launch_bounds__(kParamThreads) void param_orthogonal_kernel(ParamTable table, unsigned stride, float *params,
                                                                         const ParamGen *__restrict__ gens,
                                                                         const uint8_t *__restrict__ select, double *workspace)
{
    __shared__ double s_v[2][kParamThreads];
    __shared__ double s_c[kParamThreads];
    const size_t g = blockIdx.y;
    if (select != nullptr && select[g] == 0) // (block-uniform: no thread reaches a barrier)
        return;
    const rf_param_segment seg = table.seg[table.ortho[blockIdx.x]];
    const int t = param_ortho_t(seg), s = param_ortho_s(seg);
    float *packed = params + g * (size_t)stride + seg.at;
    double *q_vector = workspace + g * (size_t)table.workspace + table.ortho_at[blockIdx.x]; // [p][a]
    double *q_component = q_vector + param_cells(seg);                                       // [a][p]
    const ParamGen gen = gens[g];
    const int tid = threadIdx.x;
    const bool mine = tid < t;
    for (int b = 0; b < s; ++b) {
        double *v_all = s_v[b & 1];
        double v = mine ? (double)param_ortho_draw(seg, gen.word, tid, b) : 0.0;
        v_all[tid] = v;
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {
            if (tid < b)
                s_c[tid] = param_ortho_dot(q_component + tid, s, v_all, t);
            __syncthreads();
            if (mine) {
                v = param_ortho_project(v, s_c, q_vector + tid, t, b);
                v_all[tid] = v;
            }
            __syncthreads();
        }
        if (mine) {
            const double q = param_ortho_unit(v, param_ortho_norm2(v_all, t));
            q_vector[(size_t)b * (size_t)t + tid] = q;
            q_component[(size_t)tid * (size_t)s + b] = q;
        }
    }
    // (thread a rounds and scales what it stored itself)
    if (mine)
        for (int p = 0; p < s; ++p)
            packed[param_ortho_packed_at(seg, p, tid)] = param_ortho_packed(q_vector[(size_t)p * (size_t)t + tid], seg.scale);
}
#endif

} // namespace rf
