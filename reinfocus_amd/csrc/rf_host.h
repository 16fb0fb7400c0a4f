// rf_host.h -- what the translation units of libreinfocus_hip.so share on the host side: the context, the error
// plumbing and the helpers one unit exports to the others.
//
//   rf_abi_ctx.hip      contexts, RNG states (seed_kernel), scene upload, timing, device table
//   rf_abi_render.hip   which render kernel a launch takes (render_form, pick_tile_layout, launch_render), rf_render,
//                       the frame buffer, the focus measure (launch_focus, rf_focus, rf_step)
//   rf_abi_general.hip  rf_render_general
//   rf_abi_env.hip      the device-resident environment step and its schedules; then the learner
//                       entry points over caller-owned device arrays, ungrouped and grouped ("population") alike but for
//                       the grouped recurrent ones:
//                         rf_rollout_advantages*                   rollout_gae_kernel (rf_rollout.h)
//                         rf_policy_forward*                       policy_forward_kernel (rf_policy.h)
//                         rf_ppo_update*, rf_sde_update*           the three kernels of rf_ppo.h (either head)
//                         rf_sde_noise_reset*, rf_sde_forward*     rf_sde.h
//                         rf_lstm_*, rf_lstm_critic_* forwards     lstm_forward_kernel (rf_lstm.h), rf_sde.h's noise kernel
//                         ... and updates                          the five kernels of rf_lstm_ppo.h, then ppo_adam_kernel
//   rf_abi_snapshot.hip snapshots of a device-resident environment (rf_env_snapshot* / rf_env_restore*): copies only
//   rf_abi_lstm_grouped.hip  "population lstm": rf_lstm_forward_grouped, rf_lstm_ppo_update_grouped and their size
//                       functions -- the kGrouped instantiations of rf_lstm.h and rf_lstm_ppo.h, compiled apart from the
//                       ungrouped ones of rf_abi_env.hip (profiles/population_lstm.md)
//   rf_abi_lstm_sde_grouped.hip  "population lstm sde": rf_lstm_sde_noise_reset_grouped, rf_lstm_sde_forward_grouped,
//                       rf_lstm_sde_update_grouped and their size functions -- the kSde && kGrouped instantiations, compiled
//                       apart from both units above (profiles/population_lstm_sde.md)
//   rf_abi_param_init.hip  "parameter init": rf_params_init and rf_params_init_workspace_size -- param_fill_kernel and
//                       param_orthogonal_kernel (rf_param_init.h), compiled apart from every unit above
//                       (profiles/param_init.md)
//   rf_abi_eval.hip     "evaluation": rf_eval_accumulate, rf_eval_finish, rf_eval_keep_rows -- the three kernels of
//                       rf_eval.h -- and rf_env_view_get / set_statistics_device (eval_statistics_kernel), compiled apart
//                       from every unit above (profiles/evaluation.md)
//
// Every kernel instantiation is defined in the unit that launches it (ppo_adam_kernel<true>, the last launch of the three
// grouped updates, in three: each has its own copy; sde_noise_kernel<true> in two); the units share only host functions.
#pragma once
#include <cstring>

#include "../../include/reinfocus_hip.h"

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "rf_env_types.h" // EnvConfig / EnvState (plain structs of device pointers)
#include "rf_init.h" // EnvInit
#include "rf_math.h" // CamStatic, CheckerTable

typedef std::pair<hipEvent_t, hipEvent_t> EventPair;

struct rf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;

    ulonglong2 *d_states = nullptr;
    uint64_t n_states = 0;
    ulonglong2 *d_mats = nullptr;
    int *d_zero = nullptr; // a device int that stays 0: the second-pass count of a two-pass kernel launched for one pass
    // rf_render_general re-creates seed-0 states for every call, as the reference does (render.py:115): a copy of
    // the freshly seeded array turns all but the first seeding of a size into a device-to-device copy
    ulonglong2 *d_seed_cache = nullptr;
    uint64_t seed_cache_n = 0;

    float *d_cam = nullptr;
    float *d_rect = nullptr;
    int scene_n = 0;
    int scene_cap = 0;
    rf::CamStatic cs{};
    bool axis = false;
    bool coop = true; // cooperative rejection tails (REINFOCUS_RENDER_COOP=0: render_kernel for every launch)
    bool auto_form = true; // launches of few blocks take the kernel without cooperative tails, mid-size launches the
                           // wave-cooperative one (render_form; REINFOCUS_RENDER_SETS=3: three pixels per thread with
                           // block-cooperative tails for launches of every size)
    int wave_sets = 0;     // REINFOCUS_RENDER_SETS=w1 / w2 / w3: render_kernel_wave<K> for launches of every size
                           // (1 ... 3), REINFOCUS_RENDER_SETS=1: render_kernel (0: by launch size)
    bool one_px = false;
    bool strip = true; // a frame's last w % 64 <= 48 columns as tiles of 48 x 16 (REINFOCUS_RENDER_STRIP=0: one tile shape)
    double hit_fraction = 0.658; // target width / frame width of the current scene (tan 10 / tan 15 deg by default)
    bool general_one = true; // general renderer: cooperative kernel for one-shape worlds (REINFOCUS_GENERAL_ONE=0: never)
    bool general_one_always = false; // ... for launches of every size (REINFOCUS_GENERAL_ONE=1; default: large launches only)
    bool general_dense = true; // general renderer: the float32 kernel with abstentions for worlds of up to three shapes
                               // (REINFOCUS_GENERAL_DENSE=0: never)
    bool general_dense_always = false; // ... for launches of every size (REINFOCUS_GENERAL_DENSE=1; default: large launches only)

    uint8_t *d_frames = nullptr;
    size_t frames_cap = 0;
    int fn = 0, fh = 0, fw = 0;
    uint8_t *d_frames2 = nullptr; // the fused environment step: the step's frames of the environments whose slot renders twice
    size_t frames2_cap = 0;

    unsigned long long *d_sums = nullptr;
    double *d_var = nullptr;
    int focus_cap = 0;
    int focus_choice = 0; // REINFOCUS_FOCUS_KERNEL=quad / byte: the round-2 kernel where its rows fit into LDS / the
                          // byte-per-thread kernel, instead of focus_kernel_roll (A/B runs and tests)
    int focus_band = 0;   // REINFOCUS_FOCUS_BAND=r: rows per band of focus_kernel_roll (default: by launch size)

    rf::CheckerTable tab{};

    // device-resident env step (rf_env_*)
    bool env_ready = false;
    rf::EnvConfig env_cfg{};
    rf::EnvState env{};
    rf_env_config env_host{};
    void *env_block = nullptr; // one allocation holding every EnvState array
    int *d_actions = nullptr;
    float *d_pool = nullptr;
    // small configurations replay their (host-independent) step as one hipGraph
    bool env_graph_enabled = true; // REINFOCUS_ENV_GRAPH=0 disables
    hipGraphExec_t env_graph = nullptr;
    uint8_t *h_stage = nullptr;    // pinned: the host image of the io block (EnvIo) of the replayed step
    size_t h_stage_bytes = 0;
    uint64_t env_steps = 0;
    bool env_axis = false;
    bool env_last_partial = false; // that set is the compacted one of an auto-reset (cam_dyn2 / rect2)
    int env_scene_len = 0; // environments of the scene set uploaded last: n after a full render, k after a partial one
    int env_pending = -1; // >= 0: rf_env_step_begin ran and that many environments wait for rf_env_step_end
    bool env_planned = false; // the open step is rf_env_step_plan's (rf_env_step_run finishes it)
    bool env_graph_fail_once = false; // REINFOCUS_ENV_GRAPH_FAIL=1 (tests): the first instantiation "fails"
    int env_last_branch = RF_ENV_BRANCH_NONE; // rf_env_last_step_branch
    bool env_needs_reset = false; // rf_env_step_abort dropped a half-finished step
    bool env_started = false; // rf_env_reset (or a restore) has run since the configuration: there is something to snapshot
    // rf_env_configure_records: every rf_env_configure* carves the five arrays out of env_block (offsets below) and
    // leaves them unused; the call points EnvState at them (env_records), and any rf_env_configure* turns it off again
    bool env_records = false;
    size_t env_rec_off[5] = {0, 0, 0, 0, 0}; // ep_return, ep_length, final_obs, final_return, final_length
    // the three record arrays are one piece of env_block -- [final_return | final_obs | final_length], env_rec_bytes
    // from env_rec_off[3] -- so that rf_env_get_records is one copy into this pinned block and one synchronisation
    size_t env_rec_bytes = 0;
    uint8_t *h_records = nullptr;
    size_t h_records_bytes = 0;
    bool env_stepped = false; // a whole step of any form has run since the configuration
    // rf_env_configure_view: the learner view (kernels: rf_env_view.h, launched from rf_abi_env.hip).  One allocation of its own, view_block:
    // [view_reward f64 n | stack f32 n x V | view_final f32 n x V] -- the piece rf_env_get_view fetches with one copy
    // into h_view, view_final only with episode records --, then returns f64 n and the moments, 256-byte aligned each.
    // Any rf_env_configure* (rf_env_configure_records included) turns the view off again.
    bool env_view = false;
    bool view_training = false;     // rf_env_view_set_training; part of a snapshot's header
    bool view_after_step = false;   // the view's outputs are a step's (rewards and view_final mean something), not a reset's
    rf_env_view_config view_host{}; // as configured (the fingerprint's hash is over this, without `training`)
    rf::EnvViewConfig view_cfg{};
    void *view_block = nullptr;
    double *view_reward = nullptr, *view_returns = nullptr;
    float *view_stack = nullptr, *view_final = nullptr; // view_final: null without episode records
    rf::EnvViewMoments *view_moments = nullptr;
    rf::EnvViewMoments view_moments_host{}; // what an upload reads (outlives the asynchronous copy)
    size_t view_out_bytes = 0;      // bytes of the piece rf_env_get_view copies
    // rf_env_configure_view_grouped ("population view"): view_moments is then EnvViewMoments[view_groups], followed in
    // view_block by the groups' gammas float64[view_groups].  0: the ungrouped view.
    int view_groups = 0;
    rf::EnvViewGroups view_grp{};   // what the kGrouped kernels take by value (all zero without groups)
    std::vector<double> view_gammas;                     // as configured (part of the fingerprint's hash)
    std::vector<rf::EnvViewMoments> view_moments_groups; // what a grouped upload reads
    uint8_t *h_view = nullptr;
    size_t h_view_bytes = 0;
    // rf_env_snapshot_resident's slots: a device copy laid out as the host blob is (d == null: empty), the header that
    // blob would have had, and the generator's increment at that time (the jump table of env_init_host follows it)
    struct SnapshotSlot {
        void *d = nullptr;
        rf_env_snapshot_header head{};
        unsigned long long inc[2] = {0, 0};
    } env_slots[RF_ENV_SNAPSHOT_SLOTS];
    rf_env_program env_program{}; // rf_env_configure_composed's program (host copy: action checks, strategy readback)
    rf_env_observer_program env_observer{}; // rf_env_configure_observed's observer program (host copy; n_nodes 0: none)
    int env_obs_width = 4; // columns of the observations: 4, or that program's width
    // rf_env_configure_initializer: the reset states are drawn on the device (rf_env_init.h).  One allocation of its own
    // that outlives reconfigurations: the program (rf::EnvInit), then the generator (state, increment: four 64-bit words)
    bool env_init = false; // on for the configured environment (every rf_env_configure* turns it off)
    void *d_init = nullptr;
    rf::EnvInit env_init_host{};       // what the program on the device was uploaded from (outlives the async copy)
    unsigned long long env_gen_host[4] = {0, 0, 0, 0}; // ... and the generator
    bool env_fused = true; // the step's two renders and two focus measures as one launch each (REINFOCUS_ENV_FUSED=0: the
                           // three schedules of separate launches)
    long env_one_sync_max = 65536; // blocks of a full render up to which rf_env_step runs without the mid-step round
                                   // trip (REINFOCUS_ENV_ONE_SYNC_MAX; tests set 0 to reach the count-sized branch at small sizes)
    // device steps (rf_env_step_device / rf_env_reset_device; kernels in rf_env_io.h): actions and results stay in
    // device memory, nothing is waited for, and what the host keeps per step is settled later (resolve_device_steps)
    void *d_io_state = nullptr; // rf::EnvIoState (fault word, running total of rendered environments); allocated by
                                // rf_env_configure_initializer, which is what makes device steps possible
    hipEvent_t io_ev_in = nullptr, io_ev_out = nullptr; // the caller's stream -> the ctx's stream -> the caller's stream
    hipGraphExec_t env_graph_dev = nullptr; // the replayed step's body alone: no copy, no pointer of the caller's
    bool io_unresolved = false;    // device steps ran whose pixels and faults the host has not accounted yet
    bool io_scene_pending = false; // ... and the last of them decides env_scene_len / env_last_partial
    unsigned long long io_renders_seen = 0; // EnvIoState::env_renders as of the last resolution
    uint64_t env_step_index = 0;   // whole steps of either form since the last reset: the step number of a fault
    int env_fault_step = -1, env_fault_env = -1; // a resolved fault (>= 0): only a reset makes the environment usable
    const char *render_kernel = "none"; // the render kernel the last launch used (rf_render_kernel_name)
    void *general_scratch = nullptr;    // scene arrays of rf_render_general (grown on demand)
    unsigned general_redo_last = 0;     // pixels the launches of the last rf_render_general left to the fix-up kernel
    size_t general_scratch_bytes = 0;

    bool timing = false;
    std::vector<EventPair> ev_render, ev_focus;
    double render_ms = 0.0, focus_ms = 0.0;
    uint64_t render_n = 0, focus_n = 0;
};

namespace rfh {

// the calling thread's last error message (rf_last_error)
void set_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define RF_HIP(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            rfh::set_err("%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);  \
            return _e == hipErrorOutOfMemory ? RF_ERR_OOM : RF_ERR_HIP;                        \
        }                                                                                      \
    } while (0)

#define RF_REQUIRE(cond, ...)                                                                  \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            rfh::set_err(__VA_ARGS__);                                                         \
            return RF_ERR_INVALID;                                                             \
        }                                                                                      \
    } while (0)

inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// every pixel any render kernel of this process was launched for (rf_pixels_rendered)
void count_pixels(unsigned long long pixels);

int drain_events(std::vector<EventPair> &evs, double &ms, uint64_t &count);

// HIP events around a kernel's launches while rf_timing is on (the launch's own stream)
struct Timed {
    rf_ctx *ctx;
    std::vector<EventPair> *evs;
    hipEvent_t a = nullptr, b = nullptr;
    Timed(rf_ctx *c, std::vector<EventPair> *e) : ctx(c), evs(e)
    {
        if (ctx->timing) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            (void)hipEventRecord(a, ctx->stream);
        }
    }
    ~Timed()
    {
        if (ctx->timing) {
            (void)hipEventRecord(b, ctx->stream);
            evs->push_back(EventPair(a, b));
        }
    }
};

// The captured env step (rf_env_step) holds device pointers and kernel arguments by value: any
// call that may reallocate a buffer or change the scene / configuration drops it.
void drop_env_graph(rf_ctx *ctx);

// Settles what device steps (rf_env_step_device) left open on the host: synchronises the ctx's stream, accounts the
// pixels they rendered, takes the scene set of the last one (env_scene_len, env_last_partial) and records a fault.
// Every entry point that reads one of those calls it first; without open device steps it does nothing.
int resolve_device_steps(rf_ctx *ctx);
// ... and what such an entry point says once a fault is recorded
#define RF_REFUSE_FAULTED(ctx, fn)                                                                                  \
    RF_REQUIRE((ctx)->env_fault_step < 0,                                                                           \
               "%s: the action of environment %d in step %d was invalid, and the steps since then ran on its "      \
               "replacement (rf_env_reset or rf_env_reset_device first)", fn, (ctx)->env_fault_env, (ctx)->env_fault_step)

// Frees every resident snapshot slot (a new configuration, rf_destroy); the caller has synchronised the stream.
void drop_env_snapshots(rf_ctx *ctx);

// rf_env_configure_initializer's allocation (ctx->d_init): the program, then the generator
constexpr size_t kInitGenOffset = (sizeof(rf::EnvInit) + 255) & ~(size_t)255;

inline unsigned long long *init_gen(const rf_ctx *ctx)
{
    return (unsigned long long *)((char *)ctx->d_init + kInitGenOffset);
}

// states [first, first + count) of the context's array := the states of `seed` at indices first_state_index ...
// (rf_seed is this for the whole array)
int seed_range(rf_ctx *ctx, uint64_t first, uint64_t count, uint64_t seed, uint64_t first_state_index);

// Splits the lens radius for rf_math.h lens_offset and decides whether the float32 form is exact for it
void lens_split(rf::CamStatic &cs);
// ... the same question without the 60 ms proof for a radius the process has seen in fewer than 64 calls (rf_render_general)
bool lens_exact_if_known(double radius);

int ensure_frames(rf_ctx *ctx, int n, int h, int w);
int ensure_frames2(rf_ctx *ctx, int n, int h, int w);

// the second pass of a fused environment step's render (RenderArgs::count2 ...)
struct SecondPass {
    const int *count;
    const float *cam, *rect;
};
// 3 = three pixels per thread with block-cooperative tails (render_kernel_coop2 and its strip form), 0 = one pixel per
// thread without them (render_kernel), 20 + K = render_kernel_wave<K> (K pixels per thread, wave-cooperative tails)
int render_form(const rf_ctx *ctx, int n, int h, int w);
// enqueues the render of n envs whose scene arrays are cam / rect (device pointers)
int launch_render(rf_ctx *ctx, int n, int h, int w, int spp, const float *cam, const float *rect, bool axis,
                  bool count_pixels = true, const SecondPass *second = nullptr);
int ensure_focus(rf_ctx *ctx, int n);
int launch_focus(rf_ctx *ctx, int n, int h, int w, int gray_mode, const float *skip_rect = nullptr, bool in_env_step = false,
                 const int *fused_count = nullptr);

// hipMalloc / hipHostMalloc.  With REINFOCUS_POISON_ALLOC in the environment (tests/conftest.py sets it for the whole GPU suite)
// every allocation is filled with 0xA5 bytes first: nothing may depend on what fresh -- or recycled -- memory happens to hold.
inline bool poison_allocations()
{
    static const bool poison = getenv("REINFOCUS_POISON_ALLOC") != nullptr;
    return poison;
}
inline hipError_t dev_malloc(void **p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess && bytes && poison_allocations()) {
        e = hipMemset(*p, 0xA5, bytes);
        if (e == hipSuccess)
            e = hipDeviceSynchronize(); // (the ctx's stream does not wait for the null stream)
    }
    return e;
}
inline hipError_t host_malloc(void **p, size_t bytes)
{
    hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (e == hipSuccess && bytes && poison_allocations())
        memset(*p, 0xA5, bytes);
    return e;
}

// ---- what the entry points over caller-owned device arrays share (rf_abi_env.hip, the two grouped recurrent units, rf_abi_param_init.hip and rf_abi_eval.hip) ------
// check_device_array asks the runtime about one array (rf_abi_snapshot.hip and the device steps use it alone),
// refuse_capturing about the caller's stream, ranges_overlap compares two address ranges; check_device_arrays is the
// learner entry points' whole rule -- which arrays may alias and what a refusal says -- over the tables each of them keeps.
// A caller's array of `bytes` bytes: device memory of the context's GPU, aligned for its elements, and inside one
// allocation -- asked of the runtime, never dereferenced.
inline int check_device_array(const rf_ctx *ctx, const void *p, size_t bytes, size_t align, const char *what, const char *fn)
{
    hipPointerAttribute_t attr{};
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess)
        (void)hipGetLastError(); // (what the runtime says of a pointer it does not know)
    RF_REQUIRE(e == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == ctx->device,
               "%s: %s is not device memory of the context's GPU %d", fn, what, ctx->device);
    RF_REQUIRE((uintptr_t)p % align == 0, "%s: %s is not aligned to %zu bytes", fn, what, align);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess)
        RF_REQUIRE((const char *)p + bytes <= (const char *)base + size, "%s: %s has fewer than %zu bytes", fn, what, bytes);
    else
        (void)hipGetLastError();
    return RF_OK;
}

// Calling a device form while the caller's stream is being captured is out of scope: the events below would become
// nodes of the caller's graph, and the host bookkeeping would run once for any number of replays.
inline int refuse_capturing(hipStream_t caller, const char *fn)
{
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(caller, &status);
    if (e != hipSuccess)
        (void)hipGetLastError();
    RF_REQUIRE(e == hipSuccess && status == hipStreamCaptureStatusNone,
               "%s: the caller's stream is being captured (a device step cannot be part of the caller's graph)", fn);
    return RF_OK;
}

// [a, a + a_bytes) and [b, b + b_bytes) share a byte (addresses compared as integers, nothing dereferenced)
inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

// One row of an entry point's table of arrays: what it reads (inputs) or writes (outputs).  p == null: not handed in.
struct DeviceArray {
    const void *p;
    size_t bytes, align;
    const char *what;
};

// What an entry point may ask of check_device_arrays beyond the common rule
enum ArrayRule : unsigned {
    kStateInPlace = 1u,    // the output "d_state_out" may be the input "d_state_in" itself (the recurrent forwards)
    kNotAmongOutputs = 2u, // the outputs are not held against each other (the rollout does that itself, in its own words)
};

// The contract of every entry point over caller-owned arrays, in the order in which a call with several faults hears of
// them: every input that is there passes check_device_array, in table order; then every output that is there, in table
// order, passes it too, overlaps no input (table order) and no earlier output.  `why` is what the refusal of an aliased
// input ends on (null: the bare "overlaps").
template <size_t kIn, size_t kOut>
inline int check_device_arrays(const rf_ctx *ctx, const DeviceArray (&inputs)[kIn], const DeviceArray (&outputs)[kOut],
                               const char *fn, unsigned rules = 0, const char *why = "other blocks still read it")
{
    for (const DeviceArray &a : inputs)
        if (a.p != nullptr)
            if (int rc = check_device_array(ctx, a.p, a.bytes, a.align, a.what, fn))
                return rc;
    for (const DeviceArray &a : outputs) {
        if (a.p == nullptr)
            continue;
        if (int rc = check_device_array(ctx, a.p, a.bytes, a.align, a.what, fn))
            return rc;
        for (const DeviceArray &b : inputs) {
            if (b.p == nullptr || !ranges_overlap(a.p, a.bytes, b.p, b.bytes))
                continue;
            if ((rules & kStateInPlace) && !strcmp(a.what, "d_state_out") && !strcmp(b.what, "d_state_in")) {
                // in place (a block reads its own rows of the state before it writes them), or apart
                RF_REQUIRE(a.p == b.p, "%s: d_state_out overlaps d_state_in without being it (the same pointer updates the "
                           "state in place; any other overlap would have a block overwrite rows another still reads)", fn);
                continue;
            }
            if (why != nullptr)
                set_err("%s: %s overlaps %s (an output must not alias an input: %s)", fn, a.what, b.what, why);
            else
                set_err("%s: %s overlaps %s", fn, a.what, b.what);
            return RF_ERR_INVALID;
        }
        for (const DeviceArray *b = outputs; b != &a && !(rules & kNotAmongOutputs); ++b)
            RF_REQUIRE(b->p == nullptr || !ranges_overlap(a.p, a.bytes, b->p, b->bytes), "%s: %s overlaps %s", fn, a.what,
                       b->what);
    }
    return RF_OK;
}

// ignore_error(hipSetDevice(ctx->device)): the size functions make the context's device current as every entry point does,
// though they need nothing of it.  All they can return is a size, so what the runtime says to that is dropped.
inline void ignore_error(hipError_t e)
{
    if (e != hipSuccess)
        (void)hipGetLastError();
}

// what the recurrent entry points of both units say of a desc they refuse (the Categorical head)
#define RF_LSTM_LIMITS "%s: the desc is outside the limits (obs_width and lstm_hidden 1 .. %d, 1 or 2 hidden layers of width " \
                       "1 .. %d per net, n_actions 2 .. %d, activation RF_POLICY_RELU or RF_POLICY_TANH, critic " \
                       "RF_LSTM_CRITIC_LSTM or RF_LSTM_CRITIC_LINEAR)"

} // namespace rfh
