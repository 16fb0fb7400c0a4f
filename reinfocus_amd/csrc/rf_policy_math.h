// rf_policy_math.h -- the scalar arithmetic of the actor-critic forward (include/reinfocus_hip.h, "policy"): the
// project's own exp32 / log32 / tanh32, the activation, the Categorical head and the draw of a lane.
//
// Plain C++ like rf_init.h, so that tests/policycheck compiles the very same text for the host and compares it with the
// numpy twin (environments/policy.py policy_numpy) on the CPU.  exp32 and log32 are built only from float32 + - * /
// (the divide is correctly rounded: flags.mk), comparisons, float <-> int conversions and integer operations on the
// exponent field, one rounding each and nothing contracted (-ffp-contract=off): numpy float32 reproduces them bit for
// bit, which no library exp / log does across a CPU and a GPU.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rf_init.h" // PCG64DXSM and its jump-ahead; RF_HD

namespace rf {

RF_HD uint32_t f32_bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

RF_HD float bits_f32(uint32_t u)
{
    float x;
    memcpy(&x, &u, 4);
    return x;
}

constexpr uint32_t kPolicyNaN = 0x7fc00000u; // the one NaN the policy ever stores

// What is stored: a NaN result is the same 32 bits everywhere (x86 and gfx950 differ in sign and payload of the NaNs
// their operations make).
RF_HD float policy_canonical(float x)
{
    return x != x ? bits_f32(kPolicyNaN) : x;
}

// ln 2 = kLn2Hi + kLn2Lo; kLn2Hi has 10 significant bits, so k * kLn2Hi is exact for |k| < 2^14
constexpr float kLn2Hi = 0.693359375f, kLn2Lo = -2.12194440e-4f, kLog2e = 1.44269504f;

// exp(x) for x <= 0.  +0 for x < -87 (and for -inf and NaN: the comparison fails), so the result is 0 or a normal number
// of [exp(-87), 1], never a subnormal; exp32(+-0) is exactly 1.
//   k = int(x * log2(e) - 0.5)   (truncation towards zero of a value <= -0.5: the nearest integer, within one)
//   r = (x - k * kLn2Hi) - k * kLn2Lo                                  |r| <= 0.35 + a rounding
//   p = 1 + r (1 + r (1/2 + r (1/6 + r (1/24 + r (1/120 + r (1/720 + r / 5040))))))      Horner, one rounding per op
//   exp32 = p * 2^k   (2^k made in the exponent field; k >= -126, p * 2^k >= exp(-87) is normal: an exact scaling)
RF_HD float exp32(float x)
{
    if (!(x >= -87.0f))
        return 0.0f;
    const int32_t k = (int32_t)(x * kLog2e - 0.5f);
    const float kf = (float)k;
    const float r = (x - kf * kLn2Hi) - kf * kLn2Lo;
    float p = 1.0f / 5040.0f;
    p = 1.0f / 720.0f + r * p;
    p = 1.0f / 120.0f + r * p;
    p = 1.0f / 24.0f + r * p;
    p = 1.0f / 6.0f + r * p;
    p = 0.5f + r * p;
    p = 1.0f + r * p;
    p = 1.0f + r * p;
    return p * bits_f32((uint32_t)(k + 127) << 23);
}

// ln(s) for s in [1, 64] (the sum of up to 64 terms of [0, 1] of which one is 1).  s = 2^e * m with m in
// (sqrt(1/2), sqrt(2)] from the exponent field; f = m - 1 (exact), q = f / (2 + f), z = q * q,
//   ln m = 2q + q z (2/3 + z (2/5 + z (2/7 + z (2/9 + z 2/11))))
//   log32 = e * kLn2Hi + (ln m + e * kLn2Lo)
RF_HD float log32(float s)
{
    const uint32_t u = f32_bits(s);
    int32_t e = (int32_t)(u >> 23) - 127;
    float m = bits_f32((u & 0x007fffffu) | 0x3f800000u);
    if (m > 1.41421354f) {
        m = m * 0.5f;
        e = e + 1;
    }
    const float f = m - 1.0f;
    const float q = f / (2.0f + f);
    const float z = q * q;
    float p = 2.0f / 11.0f;
    p = 2.0f / 9.0f + z * p;
    p = 2.0f / 7.0f + z * p;
    p = 2.0f / 5.0f + z * p;
    p = 2.0f / 3.0f + z * p;
    const float lnm = 2.0f * q + q * (z * p);
    const float ef = (float)e;
    return ef * kLn2Hi + (lnm + ef * kLn2Lo);
}

// tanh(x) = sign(x) (1 - t) / (1 + t), t = exp32(-2 |x|): +-0 stays +-0 (t = 1), +-inf is +-1 (t = 0); NaN is NaN.
RF_HD float tanh32(float x)
{
    if (x != x)
        return bits_f32(kPolicyNaN);
    const uint32_t u = f32_bits(x);
    const float a = bits_f32(u & 0x7fffffffu);
    const float t = exp32(-2.0f * a);
    const float q = (1.0f - t) / (1.0f + t);
    return bits_f32(f32_bits(q) | (u & 0x80000000u));
}

constexpr int kPolicyRelu = 0, kPolicyTanh = 1;

// relu(x) = x > 0 ? x : 0: NaN and -0 become +0
RF_HD float policy_activation(float x, int activation)
{
    return activation == kPolicyTanh ? tanh32(x) : (x > 0.0f ? x : 0.0f);
}

// y = b;  y = y + x[k * x_stride] * w[k * w_stride],  k = 0 .. K-1: a float32 multiply, then a float32 add
RF_HD float policy_dot(const float *x, int x_stride, const float *w, int w_stride, float b, int K)
{
    float y = b;
#if defined(__HIPCC__)
#pragma unroll 8 // (the loads of 8 steps in flight at once; the chain itself stays in index order)
#endif
    for (int k = 0; k < K; ++k)
        y = y + x[(size_t)k * (size_t)x_stride] * w[(size_t)k * (size_t)w_stride];
    return y;
}

// The sampled index: the first i with double(c_i) > u * double(s), s = c_{A-1}; the last index if there is none.
RF_HD int policy_select(const float *c, int A, double u)
{
    const double bound = u * (double)c[A - 1];
    for (int i = 0; i < A; ++i)
        if ((double)c[i] > bound)
            return i;
    return A - 1;
}

// The Categorical head of one environment: logits l[0 .. A-1] (stride 1), u the lane's draw (ignored when
// deterministic).  work: A floats of the caller's (the partial sums c).
//   m = first maximum by `l_i > m` from m = l_0 (a NaN l_0 stays the maximum; NaNs elsewhere are never one)
//   z_i = l_i - m,  e_i = exp32(z_i) (0 for NaN and -inf),  c_i = c_{i-1} + e_i,  s = c_{A-1}
//   degenerate (not s >= 1: m is NaN, +inf or -inf, so no e_i is 1): action = the first maximum, log_prob = NaN
//   else: action = deterministic ? the first maximum : policy_select(c, A, u);  log_prob = z_action - log32(s)
RF_HD void policy_head(const float *l, int A, bool deterministic, double u, float *work, int64_t *action, float *log_prob)
{
    float m = l[0];
    int first = 0;
    for (int i = 1; i < A; ++i)
        if (l[i] > m) {
            m = l[i];
            first = i;
        }
    float s = 0.0f;
    for (int i = 0; i < A; ++i) {
        s = s + exp32(l[i] - m);
        work[i] = s;
    }
    if (!(s >= 1.0f)) {
        *action = first;
        *log_prob = bits_f32(kPolicyNaN);
        return;
    }
    const int a = deterministic ? first : policy_select(work, A, u);
    *action = a;
    *log_prob = policy_canonical((l[a] - m) - log32(s));
}

// Draw number `lane` after the generator state the host passed: Generator(PCG64DXSM).random()'s (next64 >> 11) * 2^-53
RF_HD double policy_draw(const uint64_t gen[4], uint64_t lane)
{
    const U128 inc{gen[2], gen[3]};
    Pcg g{pcg_apply(pcg_jump(inc, lane), U128{gen[0], gen[1]}), inc};
    return pcg_double(g);
}

} // namespace rf
