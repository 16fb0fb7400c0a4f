// rf_policy_math.h -- the scalar arithmetic of the actor-critic forward (include/reinfocus_hip.h, "policy"): the
// project's own exp32 / log32 / tanh32, the activation, the Categorical head and the draw of a lane; and of the Gaussian
// head of "sde policy": expw32, log64, normal32 (the one function that is float64 inside) and the sde_* functions; and
// sigmoid32, the gates of "lstm policy" (rf_lstm.h has the cell).
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
// their operations make).  The test is on the bits, not `x != x`: to the compiler the payload of a NaN that an operation
// makes is anyone's choice, so it may drop a floating-point select whose two sides are both a NaN -- the gfx950 build did
// for policy_canonical(sqrtf(x)), which isnan(sqrt(x)) == !(x >= 0) turns into one (tests/mathcheck found 0x7fc00001).
RF_HD float policy_canonical(float x)
{
    return (f32_bits(x) & 0x7fffffffu) > 0x7f800000u ? bits_f32(kPolicyNaN) : x;
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

// ln(s) for every positive normal s (the Categorical head calls it on [1, 64], the Gaussian head on sigma >= 1e-3).
// Subnormals, 0, negatives, inf and NaN are outside its domain: the callers test for them first.  s = 2^e * m with m in
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

// exp(x) for either sign, as the update's ratio takes it: exp32(x) for x <= 0, else 1 / exp32(-x) (+inf for x > 87 and
// for NaN, whose comparison fails: a caller that cares tests the result).
RF_HD float expw32(float x)
{
    return x <= 0.0f ? exp32(x) : 1.0f / exp32(-x);
}

// ln(s) in float64 for every positive normal double s, by log32's scheme with float64 operations (correctly rounded + - * /
// on both sides, nothing contracted): s = 2^e * m, m in (sqrt(1/2), sqrt(2)], f = m - 1, q = f / (2 + f), z = q * q,
//   ln m = 2q + q z (2/3 + z (2/5 + ... + z 2/25)),   log64 = e * kLn2Hi64 + (ln m + e * kLn2Lo64)
// (kLn2Hi64 has 32 zero low bits: e * kLn2Hi64 is exact).  About 2e-16 relative: normal32 needs it, float32 does not.
constexpr double kLn2Hi64 = 6.93147180369123816490e-01, kLn2Lo64 = 1.90821492927058770002e-10;

RF_HD double log64(double s)
{
    uint64_t u;
    memcpy(&u, &s, 8);
    int64_t e = (int64_t)(u >> 52) - 1023;
    const uint64_t mu = (u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    memcpy(&m, &mu, 8);
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        e = e + 1;
    }
    const double f = m - 1.0;
    const double q = f / (2.0 + f);
    const double z = q * q;
    double p = 2.0 / 25.0;
    p = 2.0 / 23.0 + z * p;
    p = 2.0 / 21.0 + z * p;
    p = 2.0 / 19.0 + z * p;
    p = 2.0 / 17.0 + z * p;
    p = 2.0 / 15.0 + z * p;
    p = 2.0 / 13.0 + z * p;
    p = 2.0 / 11.0 + z * p;
    p = 2.0 / 9.0 + z * p;
    p = 2.0 / 7.0 + z * p;
    p = 2.0 / 5.0 + z * p;
    p = 2.0 / 3.0 + z * p;
    const double lnm = 2.0 * q + q * (z * p);
    const double ef = (double)e;
    return ef * kLn2Hi64 + (lnm + ef * kLn2Lo64);
}

// The inverse normal CDF of a draw u = j * 2^-53, j = 0 .. 2^53 - 1, as a float32: M. J. Wichura's AS 241 PPND16
// evaluated in FLOAT64 on a float32 argument, rounded to float32 once at the end.
//   p = float32(u) for u < 1/2, float32(1 - u) otherwise (1 - u is exact), raised to 2^-54 so that u = 0 is finite (-8.29);
//   both halves run the same arithmetic on double(p) and differ in the sign only (q is negated exactly):
//   p >= 0.075f:  q = p - 1/2 (1/2 - p in the upper half: normal32(1/2) is +0), r = 0.180625 - q * q, x = (q A(r)) / B(r)
//   else r = sqrt(-log64(p));  r <= 5: r = r - 1.6, x = C(r) / D(r);  else r = r - 5, x = E(r) / F(r); negated in the
//        lower half.  A .. F by Horner from the leading coefficient (c + r * acc), one float64 rounding per operation.
// Why float64, where everything else here is float32: the function must not decrease in u.  Neighbouring float32 p lie
// at least 2^-24 p apart, which moves the exact quantile by more than 7e-9, a million times the float64 evaluation's error
// and PPND16's own 1e-16, branch joins included: the float64 values are strictly increasing in p, and one final rounding
// to float32 keeps their order.  (A float32 evaluation moves by 1.5 ulp per step of p near |x| = 0.5 and errs by more.)
// tests/test_sde_logic.py checks the order on every float32 p around the joins and on a dense sample; profiles/sde.md
// records the run over all 4.4e8 float32 p of [2^-54, 1/2].
RF_HD float normal32(double u)
{
    const bool upper = u >= 0.5;
    float pf = upper ? (float)(1.0 - u) : (float)u;
    if (pf < 5.5511151231257827e-17f)
        pf = 5.5511151231257827e-17f;
    const double p = (double)pf;
    if (pf >= 0.075f) {
        const double q = upper ? 0.5 - p : p - 0.5;
        const double r = 0.180625 - q * q;
        double a = 2.5090809287301226727e+3;
        a = 3.3430575583588128105e+4 + r * a;
        a = 6.7265770927008700853e+4 + r * a;
        a = 4.5921953931549871457e+4 + r * a;
        a = 1.3731693765509461125e+4 + r * a;
        a = 1.9715909503065514427e+3 + r * a;
        a = 1.3314166789178437745e+2 + r * a;
        a = 3.3871328727963666080e+0 + r * a;
        double b = 5.2264952788528545610e+3;
        b = 2.8729085735721942674e+4 + r * b;
        b = 3.9307895800092710610e+4 + r * b;
        b = 2.1213794301586595867e+4 + r * b;
        b = 5.3941960214247511077e+3 + r * b;
        b = 6.8718700749205790830e+2 + r * b;
        b = 4.2313330701600911252e+1 + r * b;
        b = 1.0 + r * b;
        return (float)((q * a) / b);
    }
    double r = sqrt(-log64(p));
    double x;
    if (r <= 5.0) {
        r = r - 1.6;
        double c = 7.74545014278341407640e-4;
        c = 2.27238449892691845833e-2 + r * c;
        c = 2.41780725177450611770e-1 + r * c;
        c = 1.27045825245236838258e+0 + r * c;
        c = 3.64784832476320460504e+0 + r * c;
        c = 5.76949722146069140550e+0 + r * c;
        c = 4.63033784615654529590e+0 + r * c;
        c = 1.42343711074968357734e+0 + r * c;
        double d = 1.05075007164441684324e-9;
        d = 5.47593808499534494600e-4 + r * d;
        d = 1.51986665636164571966e-2 + r * d;
        d = 1.48103976427480074590e-1 + r * d;
        d = 6.89767334985100004550e-1 + r * d;
        d = 1.67638483018380384940e+0 + r * d;
        d = 2.05319162663775882187e+0 + r * d;
        d = 1.0 + r * d;
        x = c / d;
    } else {
        r = r - 5.0;
        double e = 2.01033439929228813265e-7;
        e = 2.71155556874348757815e-5 + r * e;
        e = 1.24266094738807843860e-3 + r * e;
        e = 2.65321895265761230930e-2 + r * e;
        e = 2.96560571828504891230e-1 + r * e;
        e = 1.78482653991729133580e+0 + r * e;
        e = 5.46378491116411436990e+0 + r * e;
        e = 6.65790464350110377720e+0 + r * e;
        double f = 2.04426310338993978564e-15;
        f = 1.42151175831644588870e-7 + r * f;
        f = 1.84631831751005468180e-5 + r * f;
        f = 7.86869131145613259100e-4 + r * f;
        f = 1.48753612908506148525e-2 + r * f;
        f = 1.36929880922735805310e-1 + r * f;
        f = 5.99832206555887937690e-1 + r * f;
        f = 1.0 + r * f;
        x = e / f;
    }
    return (float)(upper ? x : -x);
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

// sigmoid(x) = 1 / (1 + t) for x >= 0 and t / (1 + t) below, t = exp32(-|x|) (exp32 is defined for arguments <= 0 only):
// +-0 gives 1/2, +inf 1, -inf +0 (t = 0), and so does every x < -87; NaN is NaN.  The LSTM cell's gates ("lstm policy").
RF_HD float sigmoid32(float x)
{
    if (x != x)
        return bits_f32(kPolicyNaN);
    const float a = bits_f32(f32_bits(x) & 0x7fffffffu);
    const float t = exp32(-a);
    return x >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t);
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

// ---- the state-dependent-exploration Gaussian head (include/reinfocus_hip.h, "sde policy") ----
constexpr float kSdeEpsilon = 1e-6f;
constexpr float kSdeHalfLog2Pi = 0.9189385332046727f, kSdeEntropy0 = 1.4189385332046727f; // 1/2 log 2 pi; 1/2 + that

RF_HD bool sde_finite(float x)
{
    return x >= -3.4028234663852886e38f && x <= 3.4028234663852886e38f;
}

// std2_k = std_k * std_k, std_k = expw32(log_std_k)
RF_HD float sde_std2(float log_std)
{
    const float s = expw32(log_std);
    return s * s;
}

// sigma = sqrt32(var + 1e-6), var = the sum over k in index order, from +0, of (h_k * h_k) * std2_k
RF_HD float sde_sigma(const float *h, int h_stride, const float *std2, int K)
{
    float var = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float x = h[(size_t)k * (size_t)h_stride];
        var = var + (x * x) * std2[k];
    }
    return sqrtf(var + kSdeEpsilon);
}

// log N(a; mu, sigma): NaN where sigma is not finite (log32 has no value there)
RF_HD float sde_log_prob(float a, float mu, float sigma)
{
    if (!sde_finite(sigma))
        return bits_f32(kPolicyNaN);
    const float t = a - mu;
    const float q = (t * t) / (2.0f * (sigma * sigma));
    return policy_canonical(((-q) - log32(sigma)) - kSdeHalfLog2Pi);
}

RF_HD float sde_entropy(float sigma)
{
    return sde_finite(sigma) ? kSdeEntropy0 + log32(sigma) : bits_f32(kPolicyNaN);
}

// what goes to the environment: the raw action clamped to [-1, 1]; NaN stays NaN
RF_HD float sde_env_action(float a)
{
    return policy_canonical(a < -1.0f ? -1.0f : (a > 1.0f ? 1.0f : a));
}

// Draw number `lane` after the generator state the host passed: Generator(PCG64DXSM).random()'s (next64 >> 11) * 2^-53
RF_HD double policy_draw(const uint64_t gen[4], uint64_t lane)
{
    const U128 inc{gen[2], gen[3]};
    Pcg g{pcg_apply(pcg_jump(inc, lane), U128{gen[0], gen[1]}), inc};
    return pcg_double(g);
}

} // namespace rf
