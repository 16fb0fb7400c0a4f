// dirfast_host.cpp -- TEST INFRASTRUCTURE: PixelEnv::dir_fast (reinfocus_amd/csrc/rf_math.h) and the squared lengths
// of the directions sample_axis_shade normalises, compiled as tests/hostsim compiles the header, for
// tests/test_dir_fast_bound.py.  Never loaded by the product package.
#include <stdint.h>

#include "../../reinfocus_amd/csrc/rf_math.h"

namespace {

rf::CamStatic cam_static(double lens_radius, int lens_f32)
{
    rf::CamStatic cs{};
    cs.ux = 1.0f;
    cs.vy = 1.0f;
    cs.lens_radius = lens_radius;
    // (the float32 form of lens_offset: hi + lo is the radius to 2^-48 of it, as rf_abi_ctx.hip splits it)
    cs.lens_hi = (float)lens_radius;
    cs.lens_lo = (float)(lens_radius - (double)cs.lens_hi);
    cs.lens_f32 = lens_f32;
    return cs;
}

// the squared length the kernels hand to len_inv_rn_fast for a miss lane of this sample
float miss_sq(const rf::PixelEnv &e, const rf::CamStatic &cs, float p0, float p1, float s, float t)
{
    const rf::AxisRay r = rf::sample_axis_point<-1>(p0, p1, e, cs, s, t);
    return rf::sq_len(r.dx, r.dy, r.dz);
}

uint64_t splitmix(uint64_t &x)
{
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

} // namespace

// lens_bound(cs) of a camera with this radius
extern "C" float df_lens_bound(double lens_radius) { return rf::lens_bound(cam_static(lens_radius, 0)); }

// flag[i] = make_pixel_env(cam + 9 i, rect + 2 i, lens_bound).dir_fast for n environments
extern "C" void df_flags(const float *cam, const float *rect, double lens_radius, long n, uint8_t *flag)
{
    const float r = df_lens_bound(lens_radius);
    for (long i = 0; i < n; ++i)
        flag[i] = rf::make_pixel_env(cam + 9 * i, rect + 2 * i, r).dir_fast ? 1 : 0;
}

// The caller that does not say which lens it renders with (tests/hostsim) never gets the flag.
extern "C" int df_flag_without_lens(const float *cam, const float *rect) { return rf::make_pixel_env(cam, rect).dir_fast ? 1 : 0; }

// For every environment with the flag: in_fast_range(sq) of the miss direction at the 16 corners s, t in {0, 1},
// p0, p1 in {-1, 1} and at `samples` random (s, t, p0, p1) -- s, t uniform multiples of 2^-24 in [0, 1], p as
// disc_finish makes them (multiples of 2^-24 / 2^-23 in [-1, 1]) --, with both forms of lens_offset.  Returns the number
// of squared lengths outside the range; *first_env the first environment with one (-1: none); *checked how many were
// looked at.
extern "C" long df_check_miss(const float *cam, const float *rect, double lens_radius, long n, long samples, uint64_t seed,
                              long *first_env, long *checked)
{
    long bad = 0;
    *first_env = -1;
    *checked = 0;
    const float r = df_lens_bound(lens_radius);
    for (long i = 0; i < n; ++i) {
        const rf::PixelEnv e = rf::make_pixel_env(cam + 9 * i, rect + 2 * i, r);
        if (!e.dir_fast)
            continue;
        for (int form = 0; form < 2; ++form) {
            const rf::CamStatic cs = cam_static(lens_radius, form);
            auto look = [&](float p0, float p1, float s, float t) {
                ++*checked;
                if (!rf::in_fast_range(miss_sq(e, cs, p0, p1, s, t))) {
                    ++bad;
                    if (*first_env < 0)
                        *first_env = i;
                }
            };
            for (int c = 0; c < 16; ++c)
                look((c & 1) ? 1.0f : -1.0f, (c & 2) ? 1.0f : -1.0f, (c & 4) ? 1.0f : 0.0f, (c & 8) ? 1.0f : 0.0f);
            uint64_t state = seed + 0x1000003ull * (uint64_t)(2 * i + form);
            for (long k = 0; k < samples; ++k) {
                const uint64_t a = splitmix(state), b = splitmix(state);
                const float s = (float)(a >> 40) * 0x1p-24f, t = (float)(b >> 40) * 0x1p-24f;
                const float p0 = (float)((a >> 8) & 0xFFFFFFu) * 0x1p-23f - 1.0f, p1 = (float)((b >> 8) & 0xFFFFFFu) * 0x1p-23f - 1.0f;
                look(p0, p1, s, t);
            }
        }
    }
    return bad;
}

// the squared length of a hit lane's direction (q0, q1, 1 + q2), as sample_axis_shade forms it, and whether it is in range
extern "C" int df_hit_in_range(float q0, float q1, float q2, float *sq)
{
    *sq = rf::sq_len(q0, q1, 1.0f + q2);
    return rf::in_fast_range(*sq) ? 1 : 0;
}
