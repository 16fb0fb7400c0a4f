/*
 * reinfocus_hip.h -- C ABI of libreinfocus_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the render-and-measure hot path of jeffwhunter/reinfocus.
 * The reference has no FFI: its device side is numba @cuda.jit Python.  Each entry
 * point below names the reference interface it replaces (file:line relative to the
 * reference checkout); INTEGRATION.md shows the ctypes stub a reference maintainer
 * would add to bind them.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / numpy types cross the boundary.
 *  - every function returns 0 on success, a negative rf_status otherwise;
 *    rf_last_error() returns a thread-local message (HIP errors carry file:line).
 *  - an rf_ctx owns ALL device memory (RNG states, scene parameters, frames,
 *    reduction partials) of one renderer on one GPU.  Host buffers are caller-owned.
 *  - one ctx is not thread-safe; different ctxs (e.g. one per GPU) are independent.
 *  - calls are synchronous with respect to the host buffers they are handed;
 *    rf_render(..., NULL) only enqueues (frames stay in HBM).
 *  - there is NO CPU fallback: without a usable gfx950 device rf_create fails.
 */
#ifndef REINFOCUS_HIP_H
#define REINFOCUS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rf_ctx rf_ctx;

typedef enum rf_status {
    RF_OK = 0,
    RF_ERR_INVALID = -1,   /* bad argument / call order (maps to AssertionError) */
    RF_ERR_HIP = -2,       /* HIP runtime error (maps to RuntimeError)           */
    RF_ERR_NO_DEVICE = -3, /* no usable GPU                                      */
    RF_ERR_OOM = -4        /* device or pinned-host allocation failed            */
} rf_status;

/* gray_mode for rf_focus: fixed-point RGB->gray coefficients (vision.py:24,
 * cv2.cvtColor COLOR_RGB2GRAY).  15 = OpenCV >= 4 (9798/19235/3735 >> 15, the
 * reference's pinned opencv-python 4.9); 14 = OpenCV 2/3 (4899/9617/1868 >> 14). */
#define RF_GRAY_15BIT 15
#define RF_GRAY_14BIT 14

const char *rf_last_error(void);
int rf_abi_version(void);

/* Number of visible HIP devices (0 on a CPU-only host; never fails the process). */
int rf_device_count(int *count);

/* Which physical GPU `device` is: its PCI bus id ("0000:c1:00.0", NUL-terminated, into bus_id[len], len >= 16)
 * and the NUMA node the host reports for it (/sys/bus/pci/devices/<id>/numa_node; -1 if unknown).
 * No reference counterpart (the reference is single-device): bench.py prints one row per rank so that an
 * N-GPU line proves it ran on N distinct GPUs, and ranks / shard threads pin themselves to their GPU's node. */
int rf_device_info(int device, char *bus_id, int len, int *numa_node);

/* Creates the per-renderer context on `device`.
 * Replaces: FastRenderer.__init__ device-side state (graphics/render.py:127-145). */
int rf_create(int device, rf_ctx **out);
int rf_destroy(rf_ctx *ctx);

/* (Re)creates `n_states` xoroshiro128+ states on the device:
 *   state[i] = jump_2^64 ^ (first_state_index + i) ( splitmix64(seed) ),
 * bit-identical to numba's sequential host seeding, computed in parallel with a
 * GF(2) jump-ahead.  first_state_index lets GPU g of a sharded run own the states a
 * single-device run would have used for its env slice.
 * Replaces: random.make_random_states (graphics/random.py:8-18) as called from
 * FastRenderer._make_random_states (graphics/render.py:248-257). */
int rf_seed(rf_ctx *ctx, uint64_t n_states, uint64_t seed, uint64_t first_state_index);
int rf_num_states(rf_ctx *ctx, uint64_t *n_states);

/* Checkpoint / test access to the RNG states; layout uint64[count][2] = (s0, s1),
 * numba's xoroshiro128p_dtype.  No reference counterpart (states are not reachable
 * through any reference API). */
int rf_get_states(rf_ctx *ctx, uint64_t first, uint64_t count, uint64_t *host_out);
int rf_set_states(rf_ctx *ctx, uint64_t first, uint64_t count, const uint64_t *host_in);

/* Uploads the scene of `n` environments.
 *   cam_dyn  float32[n][3][3]  rows: lower_left, horizontal, vertical
 *   rect     float32[n][2]     (half_side, z_pos); a half_side with the bit pattern 0x7FC0DEAD (a
 *                              NaN no arithmetic produces) marks a slot that render and focus skip
 *   origin, u, v  float32[3]   shared camera frame;  lens_radius float64
 * Replaces: the two cuda.to_device uploads in FastCameras._make_device_data
 * (graphics/camera.py:144-179) and FastWorlds._make_device_data
 * (graphics/world.py:110-123); the tuple layout is camera.py:39-56. */
int rf_set_scene(rf_ctx *ctx, int n, const float *cam_dyn, const float *rect,
                 const float origin[3], const float u[3], const float v[3],
                 double lens_radius);

/* Renders n frames of h x w pixels with spp samples per pixel into the ctx's frame
 * buffer (uint8[n][h][w][3], row 0 = bottom of the scene), advancing RNG states
 * [0, n*h*w).  If host_out is non-NULL the frames are also copied to it.
 * n must equal the n of the last rf_set_scene; n*h*w must not exceed rf_num_states.
 * Replaces: FastRenderer.render's launch + copy_to_host (graphics/render.py:165-188)
 * and the kernel FastRenderer._device_render (graphics/render.py:190-246). */
int rf_render(rf_ctx *ctx, int n, int h, int w, int spp, uint8_t *host_out);

/* Copies frames [first_env, first_env + n_envs) of the last render to the host. */
int rf_get_frames(rf_ctx *ctx, int first_env, int n_envs, uint8_t *host_out);

/* Replaces the ctx's frame buffer by caller-supplied images uint8[n][h][w][3], so
 * that rf_focus can score frames that did not come from rf_render
 * (vision.focus_values called on a host array, vision.py:28-39). */
int rf_upload_frames(rf_ctx *ctx, int n, int h, int w, const uint8_t *host_in);

/* Focus score of every frame in the ctx's frame buffer:
 * RGB->gray, 3x3 median (replicate border), 3x3 Laplacian (reflect-101 border,
 * saturated to uint8), population variance; host_var float64[n].
 * Replaces: vision.focus_values / focus_value (vision.py:11-39), i.e. the
 * cv2.cvtColor + cv2.medianBlur + cv2.Laplacian + ndarray.var chain. */
int rf_focus(rf_ctx *ctx, int n, int h, int w, int gray_mode, double *host_var);

/* rf_render(host_out = NULL) followed by rf_focus: what FocusObserver.observe does
 * per step (environments/state_observer.py:377-381) without the frame D2H. */
int rf_step(rf_ctx *ctx, int n, int h, int w, int spp, int gray_mode, double *host_var);

/* Name of the render kernel (template instance included) the ctx's last render launch used,
 * e.g. "render_kernel_coop2<true, 1, 4, 32>"; "none" before the first render.  The string is static.
 * No reference counterpart (bench.py reports it next to the roofline figures). */
const char *rf_render_kernel_name(rf_ctx *ctx);

/* Pixels every render launch of this process (all contexts) was made for, n * h * w each, since the
 * library was loaded.  No reference counterpart: bench.py divides the PMC totals of a profiled run by
 * it, so that per-pixel figures count the pixels really rendered (not waves x pixels per wave). */
unsigned long long rf_pixels_rendered(void);

/* 1 when the process started with REINFOCUS_POISON_ALLOC in its environment: every device / pinned-host allocation of the
 * library is then filled with 0xA5 bytes before use (csrc/rf_host.h dev_malloc) -- a debugging aid under which the GPU test
 * suite runs, so that no result can depend on what fresh or recycled memory holds.  No reference counterpart. */
int rf_allocations_poisoned(void);

/* Pixels the launches of the ctx's last rf_render_general call left to the fix-up kernel, summed over the call's launches:
 * the pixels the one-shape or the dense kernel could not decide in float32 and the literal code rendered again
 * (csrc/rf_general_one.h, rf_general_dense.h); 0 for calls the literal kernel served and before the first call.
 * No reference counterpart (tools/bench_general.py reports the share). */
unsigned rf_general_redo_pixels(rf_ctx *ctx);

/* Blocks until everything enqueued on the ctx's stream has finished. */
int rf_synchronize(rf_ctx *ctx);

/* Per-kernel timing with HIP events recorded on the ctx's own stream (bench.py's
 * roofline figure).  rf_timing(ctx, 1) enables and resets the accumulators;
 * rf_timing_read synchronizes and returns total milliseconds and launch counts. */
int rf_timing(rf_ctx *ctx, int enable);
int rf_timing_read(rf_ctx *ctx, double *render_ms, uint64_t *render_launches,
                   double *focus_ms, uint64_t *focus_launches);

/* ---- general renderer ------------------------------------
 * Renders n environments of spheres and z-aligned rectangles seen through per-environment
 * cameras, with up to 50 diffuse bounces per sample, into the ctx's frame buffer
 * (uint8[n][h][w][3]) and optionally to host_out.  As the reference does for every call
 * (render.py:115) the RNG states [0, n*h*w) are re-created from seed 0 first.
 *   cameras float64[n][19]: lower_left, horizontal, vertical, origin, u, v (3 each), lens
 *           radius -- the numpy.hstack row of camera.Cameras (camera.py:63-83)
 *   params  float32[n][most][width], types int32[n][most] (0 sphere, 1 rectangle),
 *           sizes int32[n]: world.Worlds (world.py:30-65); a sphere is {x, y, z, r, fx, fy}
 *           (sphere.py:14-19), a rectangle {x_min, x_max, y_min, y_max, z, fx, fy}
 *           (rectangle.py:12-19)
 * Replaces: render.render (graphics/render.py:88-119) and kernel device_render (:31-85). */
int rf_render_general(rf_ctx *ctx, int n, int h, int w, int spp, const double *cameras,
                      const float *params, const int32_t *types, const int32_t *sizes, int most,
                      int width, uint8_t *host_out);

/* ---- device-resident DiscreteSteps-v0 step ------------
 * The per-step numpy glue of the reference's vector environment runs on the GPU around
 * the render and focus kernels; a step uploads the actions and a pool of candidate reset
 * states and downloads observations, rewards and flags.
 * Replaces, for the environment assembled in examples/custom_environments.py:114-241:
 *   VectorEnvironment.reset / step        environments/vector_environment.py:75-164
 *   DiscreteMoveTransformer.transform     environments/state_transformer.py:248-266
 *   TimeLimitEnder | DivergingEnder       environments/episode_ender.py:106-207, :580-656
 *   Normalized(Delta([Indexed, Focus]))   environments/state_observer.py:232-292, :472-517
 *   Delta + Observation + OnTarget reward environments/episode_rewarder.py:86-155, :210-292
 *   FastCameras / FastWorlds packing      graphics/camera.py:144-179, graphics/world.py:110-123
 */
typedef struct rf_env_config {
    int n;                    /* environments */
    int n_actions;            /* <= 32 */
    double action_set[32];    /* moves of the focus plane (float64, as the reference) */
    float limit_lo, limit_hi; /* clip limits of the state */
    int max_steps;            /* TimeLimitEnder; <= 0 disables it */
    float diverge_threshold;  /* DivergingEnder threshold */
    int early_end_steps;      /* DivergingEnder early_end_steps */
    float mid[4], scale[4];   /* NormalizedObserver mid / scale (float32) */
    float reward_scale;       /* DeltaRewarder scale */
    float on_target_span;     /* OnTargetRewarder span */
    double half_width, half_height; /* FastCameras: aspect * tan(vfov/2), tan(vfov/2) */
    double tan_half_r;        /* FastWorlds: tan(radians(r_size / 2)) */
    float look_from[3], cam_u[3], cam_v[3], cam_w[3];
    double lens_radius;
    int frame_height, spp, gray_mode;
} rf_env_config;

/* Allocates the per-env device state for cfg->n environments (RNG states must already
 * cover n * frame_height^2 pixels: rf_seed first). */
int rf_env_configure(rf_ctx *ctx, const rf_env_config *cfg);

/* vector_environment.py:75-102: installs host_states float32[n][2] = [target, focus plane],
 * renders and scores every environment, returns observations float32[n][4] (here and below: float32[n][W] for a
 * context configured by rf_env_configure_observed). */
int rf_env_reset(rf_ctx *ctx, const float *host_states, float *host_obs);

/* vector_environment.py:104-164: one step.  host_actions int32[n]; host_pool float32[n][2]
 * holds the initializer's candidate states, the r-th done environment (in index order)
 * takes row r; *host_n_reset returns how many rows were consumed.  Outputs:
 * observations float32[n][4], rewards float64[n], truncated uint8[n] (terminated is always
 * false for this environment). */
int rf_env_step(rf_ctx *ctx, const int32_t *host_actions, const float *host_pool, float *host_obs,
                double *host_rewards, uint8_t *host_truncated, int *host_n_reset);

/* The same step in two halves, for an environment sharded over several contexts / GPUs
 * (harness.ShardedVectorDiscreteSteps): which rows of the initializer's pool a shard takes depends
 * on how many environments ended in the shards before it (vector_environment.py:138-142 draws
 * done.sum() states for the done environments in index order).
 *   rf_env_step_begin   transform, enders, full render + focus, observations, rewards, flags
 *                       (vector_environment.py:124-135); *host_n_reset = k environments ended
 *   rf_env_step_end     those k environments take host_pool float32[k][2] in index order and are
 *                       rendered and scored again (vector_environment.py:137-151); observations
 *                       float32[n][4] of all environments.  host_pool may be NULL when k == 0.
 * rf_env_step == begin + end with the pool's first k rows -- on ONE context.  Several contexts that
 * share an environment range (harness.ShardedVectorDiscreteSteps) are not bit-equal to one context
 * holding all of it after the first auto-reset: each context's partial render indexes RNG states from
 * its own base, where a single context (like the reference, graphics/render.py:217 on
 * vector_environment.py:144's compacted rows) indexes the compacted set of ALL ended environments
 * from state 0 (the sharded environment's exact mode gathers them instead).
 *   rf_env_step_abort   drops an open two-phase step (after a failure on another shard): the
 *                       environments that ended stay un-reset and rf_env_reset must come next. */
int rf_env_step_begin(rf_ctx *ctx, const int32_t *host_actions, double *host_rewards, uint8_t *host_truncated,
                      int *host_n_reset);
int rf_env_step_end(rf_ctx *ctx, const float *host_pool, float *host_obs);
int rf_env_step_abort(rf_ctx *ctx);

/* The two halves a sharded environment uses by default (harness.ShardedVectorDiscreteSteps), cut where the fused
 * step (RF_ENV_BRANCH_FUSED below) allows -- BEFORE the render, because which environments end depends on their
 * counters alone (episode_ender.py:137-148, :602-607), not on what the step observes:
 *   rf_env_step_plan    transform + enders + ranking of the environments that end; *host_n_reset = k.  Cheap: no render.
 *   rf_env_step_run     the rest of the step with host_pool float32[k][2] for those k (NULL when k == 0): ONE render
 *                       launch (two-pass blocks for slots 0 .. k-1) and one focus launch where the two-pass kernel
 *                       exists, the separate launches of rf_env_step_begin / _end otherwise -- same results either way,
 *                       and the same as begin + end.  Outputs as rf_env_step.
 * rf_env_step_abort drops a planned step as it drops a begun one.  No reference counterpart
 * (vector_environment.py:104-164 is one synchronous schedule on one device). */
int rf_env_step_plan(rf_ctx *ctx, const int32_t *host_actions, int *host_n_reset);
int rf_env_step_run(rf_ctx *ctx, const float *host_pool, float *host_obs, double *host_rewards, uint8_t *host_truncated);

/* Exact mode of an environment sharded over several contexts (opt-in; harness.ShardedVectorDiscreteSteps
 * exact=True).  On one device the partial render of an auto-reset indexes RNG states from 0 over the
 * compacted rows of ALL environments that ended (vector_environment.py:144 -> state_observer.py:377-381
 * -> render.py:217), i.e. compacted row r draws from the states of environment slot r.  To reproduce
 * that, row r is rendered by the context that owns slot r, whichever context the ended environment
 * lives on, and the focus value travels back through the host:
 *   rf_env_render_states   packs host_states float32[k][2] (target, focus plane) as compacted rows
 *                          0..k-1, renders them at the environment's frame size / spp from THIS context's
 *                          RNG state 0 and scores them: host_focus float64[k].  Afterwards the context's
 *                          renderer holds that set (rf_env_render draws it), as the reference's does.
 *   rf_env_step_end_given  rf_env_step_end without the render: this context's k ended environments take
 *                          host_pool float32[k][2] in index order, and their reset observations are built
 *                          from host_focus float64[k]. */
int rf_env_render_states(rf_ctx *ctx, int k, const float *host_states, double *host_focus);
int rf_env_step_end_given(rf_ctx *ctx, const float *host_pool, const double *host_focus, float *host_obs);

/* Renders the scene set the environment uploaded last -- all n environments after a step in which
 * none ended, otherwise only the k that were reset, exactly what the reference's shared
 * FastRenderer holds at that point -- at frame_height x frame_height with spp samples, advancing
 * RNG states [0, len * frame_height^2); host_out uint8[len][frame_height][frame_height][3] may be
 * NULL (frames stay in the ctx's buffer).  rf_env_scene_len returns len.
 * Replaces: HistoryVisualizer.visualize's renderer.render(600)
 * (environments/episode_visualizer.py:197) on the renderer FocusObserver shares with it. */
int rf_env_scene_len(rf_ctx *ctx, int *n_envs);
int rf_env_render(rf_ctx *ctx, int frame_height, int spp, uint8_t *host_out);

/* TimeLimitEnder._steps and DivergingEnder._diverging_steps, int32[n] each (what the visualiser
 * prints: episode_ender.py:191-207, :646-656). */
int rf_env_get_counters(rf_ctx *ctx, int32_t *host_steps, int32_t *host_diverging);

/* How the last rf_env_step ran -- different schedules of the same arithmetic with the same results
 * (tests/test_gpu_environment.py runs each against the reference's numpy glue):
 *   RF_ENV_BRANCH_FUSED       the default for the canonical camera: ONE render launch and one focus launch per
 *                             step.  Which environments end depends on their counters alone, so they are ranked
 *                             before the render, and the blocks of slots 0 .. k-1 -- whose RNG streams the k
 *                             re-rendered frames continue (render.py:217) -- make two passes; one host
 *                             synchronisation at any size;
 *   RF_ENV_BRANCH_FUSED_GRAPH the same, replayed as one hipGraph from the second step on;
 * and, with REINFOCUS_ENV_FUSED=0 (or a camera / kernel choice without a two-pass instance), two launches each:
 *   RF_ENV_BRANCH_ONE_SYNC    whole step enqueued at once, auto-reset launch sized for all n slots,
 *                             one host synchronisation (small configurations);
 *   RF_ENV_BRANCH_GRAPH       the same, replayed as one hipGraph (from such a configuration's second
 *                             step on; REINFOCUS_ENV_GRAPH=0 disables);
 *   RF_ENV_BRANCH_COUNT_SIZED rf_env_step_begin + rf_env_step_end: one host round trip mid-step, the
 *                             auto-reset launch sized by the count (configurations whose full render
 *                             has more than REINFOCUS_ENV_ONE_SYNC_MAX = 65536 blocks, e.g. the
 *                             benchmarked 4096 x 256 x 256).
 * No reference counterpart (vector_environment.py:104-164 is one synchronous schedule); diagnostic. */
#define RF_ENV_BRANCH_NONE 0
#define RF_ENV_BRANCH_ONE_SYNC 1
#define RF_ENV_BRANCH_GRAPH 2
#define RF_ENV_BRANCH_COUNT_SIZED 3
#define RF_ENV_BRANCH_FUSED 4
#define RF_ENV_BRANCH_FUSED_GRAPH 5
int rf_env_last_step_branch(rf_ctx *ctx, int *branch);

/* Current states float32[n][2] (tests / checkpoint). */
int rf_env_get_states(rf_ctx *ctx, float *host_states);

/* ---- the same device-resident step for ContinuousJumps (examples/__init__.py:14-18) -------------------------------
 * A vector ContinuousJumps: the environment of examples/custom_environments.py:244-339 with num_envs in place of 1 and
 * the vector DiscreteSteps' TimeLimitEnder | DivergingEnder (:185-190), driven by VectorEnvironment
 * (environments/vector_environment.py:104-164).  It differs from the DiscreteSteps step in two strategies only:
 *   ContinuousJumpTransformer(n, 1, limits, stop_threshold)   environments/state_transformer.py:66-118
 *     a = float32 action; focus' = (a + 1) / 2.0 * (hi - lo) + lo where |focus - focus'| > stop_threshold; no clip
 *   ObservationRewarder(1) + StoppedRewarder(1, stop_threshold) * OnTargetRewarder((0, 1), on_target_span)
 *                                                             environments/episode_rewarder.py:210-292, :361-429
 * Everything else -- enders, observer, scene packing, auto-reset, render, focus measure, rf_env_reset / _step_end /
 * _step_run / _render_states / _step_end_given / _step_abort / _render / _get_* -- is the DiscreteSteps step's.
 *   rf_env_configure_jumps  rf_env_configure for this task: cfg as there, except that n_actions / action_set / reward_scale
 *                           are unused and limit_lo / limit_hi are the range the focus plane jumps in (the state's [5, 10]).
 *   rf_env_step_jumps, rf_env_step_begin_jumps, rf_env_step_plan_jumps
 *                           rf_env_step / _begin / _plan with host_actions float32[n]: same schedules, same outputs.
 *                           These are the float32-action forms: a composed context with a continuous transformer
 *                           (rf_env_configure_composed below) steps through them too.
 * Deliberate difference from the reference: an action that is NaN, infinite or outside [-1, 1] is refused
 * (RF_ERR_INVALID) before any state changes; the reference would carry it into the focus plane.  The int32 calls on a
 * context configured by rf_env_configure_jumps, and these on one configured by rf_env_configure, are refused too. */
int rf_env_configure_jumps(rf_ctx *ctx, const rf_env_config *cfg, float stop_threshold);
int rf_env_step_jumps(rf_ctx *ctx, const float *host_actions, const float *host_pool, float *host_obs,
                      double *host_rewards, uint8_t *host_truncated, int *host_n_reset);
int rf_env_step_begin_jumps(rf_ctx *ctx, const float *host_actions, double *host_rewards, uint8_t *host_truncated,
                            int *host_n_reset);
int rf_env_step_plan_jumps(rf_ctx *ctx, const float *host_actions, int *host_n_reset);

/* ---- the same device-resident step for an environment composed of strategy objects ---------------------------------
 * VectorEnvironment (environments/vector_environment.py:104-164) over any transformer, ender and rewarder the
 * reference's classes can express (environments/state_transformer.py, episode_ender.py, episode_rewarder.py).  The
 * observer is the one both tasks use, NormalizedObserver(DeltaObserver([IndexedElementObserver(1), FocusObserver])), for
 * rf_env_configure_composed, and any tree of the reference's observer classes around one FocusObserver for
 * rf_env_configure_observed (rf_env_observer_program below).  State is
 * [target, focus plane], so every state index is 0 or 1.  Python compiles the objects into an rf_env_program
 * (harness.DeviceVectorEnvironment); rf_env_configure_composed uploads it once, and every schedule of the step runs it.
 *
 * Ender and rewarder trees are postfix lists over their leaves: an entry >= 0 pushes leaf [entry], RF_OP_OR / RF_OP_ADD
 * (-1) and RF_OP_AND / RF_OP_MUL (-2) pop two operands and push the result.  reward_f64[i] says whether entry i's value
 * is float64 (numpy's promotion, decided by Python): a float32 node computes in float32.  Rewards are returned as
 * float64.  Parameters are doubles, rounded to float32 where numpy rounds a Python scalar next to a float32 array. */
#define RF_ENV_MAX_LEAVES 8
#define RF_ENV_MAX_OPS (2 * RF_ENV_MAX_LEAVES - 1)
#define RF_ENV_MAX_STOPPED_STEPS 31

enum { RF_TRANSFORM_CONTINUOUS_JUMP = 0, RF_TRANSFORM_CONTINUOUS_MOVE = 1, RF_TRANSFORM_DISCRETE_JUMP = 2,
       RF_TRANSFORM_DISCRETE_MOVE = 3 };
enum { RF_ENDER_DIVERGING = 0, RF_ENDER_ENDLESS = 1, RF_ENDER_ON_TARGET = 2, RF_ENDER_STOPPED = 3,
       RF_ENDER_TIME_LIMIT = 4 };
enum { RF_REWARD_DELTA = 0, RF_REWARD_DISTANCE = 1, RF_REWARD_OBSERVATION = 2, RF_REWARD_ON_TARGET = 3,
       RF_REWARD_STOPPED = 4 };
enum { RF_OP_OR = -1, RF_OP_AND = -2, RF_OP_ADD = -1, RF_OP_MUL = -2 };

typedef struct rf_env_ender {
    int kind;              /* RF_ENDER_* */
    int index0, index1;    /* check_indices (StoppedEnder: check_index in index0) */
    int steps;             /* early_end_steps (Diverging, OnTarget, Stopped <= 31) / max_steps (TimeLimit) */
    double threshold;      /* Diverging threshold / OnTarget early_end_radius / Stopped early_end_span */
} rf_env_ender;

typedef struct rf_env_rewarder {
    int kind;              /* RF_REWARD_* */
    int index0, index1;    /* check_index(es); Observation: reward_observation_index in index0 (0-3; below the
                              observation width of an rf_env_observer_program) */
    double p[3];           /* Delta: reward, scale | Distance: span, high - low, low | OnTarget: span, on - off, off
                              | Stopped: |threshold|, reward | Observation: unused */
} rf_env_rewarder;

typedef struct rf_env_program {
    int transformer;         /* RF_TRANSFORM_* */
    int move_index;          /* 0 or 1 */
    int n_actions;           /* discrete transformers: 1 ... 32 */
    double action_set[32];   /* DiscreteMove: the float64 moves; DiscreteJump: the float32 positions */
    double limit_lo, limit_hi; /* limits (clip limits; ContinuousJump: the range the element jumps in) */
    double speed;            /* ContinuousMove */
    double stop_threshold;   /* ContinuousJump / ContinuousMove: |stop_threshold| */
    int n_enders, n_ender_ops;
    rf_env_ender enders[RF_ENV_MAX_LEAVES];
    int ender_ops[RF_ENV_MAX_OPS];
    int n_rewarders, n_reward_ops;
    rf_env_rewarder rewarders[RF_ENV_MAX_LEAVES];
    int reward_ops[RF_ENV_MAX_OPS];
    int reward_f64[RF_ENV_MAX_OPS];
} rf_env_program;

/* rf_env_configure for a composed environment.  Of cfg, only n, mid, scale, the camera / world packing, lens_radius,
 * frame_height, spp and gray_mode are used: n_actions, action_set, limit_lo, limit_hi, max_steps, diverge_threshold,
 * early_end_steps, reward_scale and on_target_span are ignored (the program replaces them).  Refused (RF_ERR_INVALID,
 * nothing changes): more than RF_ENV_MAX_LEAVES leaves, a postfix list that is not one well-formed expression over
 * every leaf once, an unknown kind, a state index outside {0, 1} or an observation index outside 0-3, a StoppedEnder
 * with steps outside [0, 31], n_actions outside [1, 32] for a discrete transformer, a non-finite parameter.
 * Actions: the discrete transformers take the int32 rf_env_step / _begin / _plan (indices outside [0, n_actions) are
 * refused), the continuous ones the float32 forms rf_env_step_jumps / _begin_jumps / _plan_jumps (NaN and infinities
 * are refused; ContinuousJump also refuses values outside [-1, 1]; ContinuousMove clips them, as the reference does).
 * The other dtype's entry points are refused.  All else -- reset, the schedules, the sharded halves, render, states --
 * is the DiscreteSteps step's. */
int rf_env_configure_composed(rf_ctx *ctx, const rf_env_config *cfg, const rf_env_program *program);

/* The per-leaf strategy state of a composed environment, each array NULL or as laid out here:
 *   host_counters  int32[n_enders][n]    Diverging: diverging steps; OnTarget: on-target steps; TimeLimit: steps; else 0
 *   host_floats    float32[n_enders][n]  Diverging: the last difference; else 0
 *   host_histories float32[H][n]         the StoppedEnder histories in leaf order, steps + 1 rows each, oldest first,
 *                                        NaN where empty; H = the sum of those lengths
 *   host_old       float32[n_rewarders][n] Delta / Stopped: the element's previous value; else 0 */
int rf_env_get_strategy_state(rf_ctx *ctx, int32_t *host_counters, float *host_floats, float *host_histories,
                              float *host_old);

/* ---- the observer of a composed environment as a program -------------------------------------------------------------
 * Any tree of the reference's observer classes (environments/state_observer.py:100-292, :386-517) around exactly one
 * FocusObserver(target_index 0, focus_plane_index 1), as a list of nodes in evaluation order (children before their
 * wrapper, left to right) over a file of float32 columns per environment -- the environment's row of observations
 * itself.  The file is a stack: a leaf writes the next free column; a wrapper works on the `width` columns its children
 * left on top, starting at column `first`:
 *   RF_OBS_INDEXED     column first := state[index]                              IndexedElementObserver
 *   RF_OBS_FOCUS       column first := float32(variance of the frame's Laplacian) FocusObserver
 *   RF_OBS_DELTA       deltas := columns - old values (float32; zero in a reset); old values := columns; the deltas
 *                      replace the columns, or with include_original follow them (width more columns).  Its old
 *                      values are rows old_first ... old_first + width - 1 of the old-value rows, NaN until the first
 *                      reset                                                      DeltaObserver
 *   RF_OBS_NORMALIZED  columns := min(max((column - mid) / scale, -1), 1), float32 NormalizedObserver
 * The last node leaves `width` columns: the observations, float32[n][width].  n_old is the number of old-value rows.
 * Refused (RF_ERR_INVALID, nothing changes): more than RF_ENV_MAX_OBS_NODES nodes, more than RF_ENV_MAX_OBS_COLUMNS
 * columns at any point or old-value rows, an unknown kind, an element index outside {0, 1}, a node that does not work on
 * the top of the stack or old-value rows that are not handed out in node order, anything other than one RF_OBS_FOCUS
 * node, a width or n_old that is not what the nodes leave, and a NORMALIZED mid that is not finite or scale that is
 * zero or not finite (fminf / fmaxf do not propagate NaN as numpy.clip does). */
#define RF_ENV_MAX_OBS_NODES 16
#define RF_ENV_MAX_OBS_COLUMNS 16

enum { RF_OBS_INDEXED = 0, RF_OBS_FOCUS = 1, RF_OBS_DELTA = 2, RF_OBS_NORMALIZED = 3 };

typedef struct rf_env_observer_node {
    int kind;              /* RF_OBS_* */
    int index;             /* INDEXED: element_index */
    int first, width;      /* leaves: the column written, 1 | wrappers: the columns [first, first + width) worked on */
    int include_original;  /* DELTA */
    int old_first;         /* DELTA: first of its `width` old-value rows */
    float mid[RF_ENV_MAX_OBS_COLUMNS], scale[RF_ENV_MAX_OBS_COLUMNS]; /* NORMALIZED: per column, float32 */
} rf_env_observer_node;

typedef struct rf_env_observer_program {
    int n_nodes;           /* 1 ... RF_ENV_MAX_OBS_NODES */
    int width;             /* observation columns W the last node leaves */
    int n_old;             /* old-value rows D of all DELTA nodes */
    rf_env_observer_node nodes[RF_ENV_MAX_OBS_NODES];
} rf_env_observer_program;

/* rf_env_configure_composed with the observer as a program too: cfg's mid / scale are ignored as well, and an
 * ObservationRewarder's index must be below observer->width.  For a context configured so, EVERY host_obs argument of
 * the rf_env_* calls (rf_env_reset, rf_env_step, rf_env_step_jumps, rf_env_step_end, rf_env_step_run,
 * rf_env_step_end_given) is float32[n][observer->width] in place of float32[n][4].  rf_env_configure_composed keeps
 * the built-in observer, and its kernels' code path. */
int rf_env_configure_observed(rf_ctx *ctx, const rf_env_config *cfg, const rf_env_program *program,
                              const rf_env_observer_program *observer);

/* The DELTA nodes' old values of a context configured by rf_env_configure_observed, node-major: host_old
 * float32[observer->n_old][n] (DeltaObserver._old_wrapped_observations, one row per column, in node order). */
int rf_env_get_observer_state(rf_ctx *ctx, float *host_old);

/* ---- the initializer of a device-resident environment as a program --------------------------------------------------
 * A RangedInitializer over the two state elements (one or several (low, high) ranges each) and its numpy
 * Generator(PCG64DXSM), so that the states of the auto-reset are drawn on the device: without it every step takes a pool
 * of n candidate rows the host drew (host_pool) and the host draws the rows that were used a second time.
 * Replaces: RangedInitializer.initialize (environments/state_initializer.py:53-71) as VectorEnvironment calls it for
 * the environments that ended (environments/vector_environment.py:138) and in reset().
 * The generator is numpy's: 128-bit state and odd increment, two 64-bit words each (low word first); a double is
 * (output >> 11) * 2^-53.  Row r of a draw starts r * d outputs after the generator's state, d = 2 when both elements
 * have one range (element j = float32(low_j + span_j * u_j)) and 4 otherwise (u_0 ... u_3; element j takes range
 * min(int64(u_j * count_j), count_j - 1) and is float32(low + span * u_{2+j}) in it); float64 arithmetic, rounded once.
 *   rf_env_configure_initializer   after any rf_env_configure*: the context draws its reset states itself from now on
 *                                  (until the next rf_env_configure*).  Refused (RF_ERR_INVALID, nothing changes): a
 *                                  count outside [1, RF_ENV_MAX_RANGES], a low or span that is not finite, a low or
 *                                  low + span of magnitude >= 3.4e38 (environments/scalars.py: the float32 result stays
 *                                  finite), an even increment, a context without an environment.
 *   rf_env_set_initializer_state   reseeds: the generator's state and (odd) increment.
 *   rf_env_get_initializer_state   reads them back (Generator.bit_generator.state of the host twin's initializer).
 * On a context so configured rf_env_step / rf_env_step_jumps take host_pool == NULL (a pool is refused) and the
 * generator advances by d for every environment that ended, as initialize(k) advances the twin's; rf_env_reset with
 * host_states == NULL draws all n states (initialize(n)), with host_states it installs them and leaves the generator
 * alone.  The two-phase and sharded halves -- rf_env_step_begin*, _end, _plan*, _run, _end_given -- and
 * rf_env_render_states are refused: they have no row offset.  Everything else is unchanged. */
#define RF_ENV_MAX_RANGES 8
typedef struct rf_env_initializer_program {
    int counts[2];                        /* ranges of element 0 / 1: 1 ... RF_ENV_MAX_RANGES */
    double low[2][RF_ENV_MAX_RANGES], span[2][RF_ENV_MAX_RANGES];   /* span = high - low in float64 */
    uint64_t state[2], inc[2];            /* PCG64DXSM: low word, high word */
} rf_env_initializer_program;
int rf_env_configure_initializer(rf_ctx *ctx, const rf_env_initializer_program *program);
int rf_env_set_initializer_state(rf_ctx *ctx, const uint64_t state[2], const uint64_t inc[2]);
int rf_env_get_initializer_state(rf_ctx *ctx, uint64_t state[2], uint64_t inc[2]);

/* ---- snapshots of a device-resident environment ----------------------------------------------------------------------
 * Everything that decides the results of later rf_env_step*, rf_env_reset(NULL) and rf_env_render calls, taken and put
 * back bit for bit: to resume a run in another process (the host forms) and to rewind or branch one quickly and often
 * (the resident forms, whose copy stays in HBM).  No reference counterpart: the reference cannot serialise its RNG
 * states at all.  Only copies on the ctx's stream; no kernel.
 *
 * A snapshot is a blob of rf_env_snapshot_size bytes: the header below (256 bytes), then these arrays, each at the next
 * multiple of 256 bytes, in this order, arrays of zero length left out (n = environments, little-endian as the device):
 *    1 state        float32[n][2]                    11 done_index   int32[n]
 *    2 steps        int32[n]                         12 done_count   int32[1]
 *    3 diverging    int32[n]                         13 leaf_count   int32[n_enders][n]      (composed contexts)
 *    4 last_diff    float32[n]                       14 leaf_float   float32[n_enders][n]
 *    5 old_wrapped  float32[n][2]                    15 history      float32[rows][n]
 *    6 old_focus    float32[n]                       16 leaf_old     float32[n_rewarders][n]
 *    7 cam_dyn      float32[n][9]                    17 obs_old      float32[n_old][n]       (observer program)
 *    8 rect         float32[n][2]                    18 generator    uint64[4]: state, inc   (device initializer)
 *    9 cam_dyn2     float32[n][9]                    19 ep_return    float64[n]              (episode records)
 *   10 rect2        float32[n][2]                    20 ep_length    int32[n]
 *                                                    21 view stack   float32[n][V]           (learner view)
 *                                                    22 view returns float64[n]
 *                                                    23 view moments float64[3][17]: mean, var, count
 *                                                       (a grouped view, "population view": float64[G][3][17])
 *                                                    24 RNG states   uint64[rf_num_states][2]
 * (7-12: the scene sets of the last render and the ranks of the environments that ended; 2-6 are the built-in tasks'
 * and the built-in observer's, zero where a composed context does not use them.)  The header also carries the two
 * host-side words of the scene set, rf_env_scene_len and whether that set is the compacted one.  NOT in a snapshot: the frame buffers, the last step's
 * observations / rewards / flags and episode records (final_observation / episode_return / episode_length: outputs
 * like the observations -- only the two accumulators, 19 and 20, are state), the focus sums, timing accumulators, and the count of steps that decides when graph
 * replay starts (the restoring context keeps its own).  The blob is data: it holds no pointers.
 *
 * The header's fingerprint names the configuration the blob belongs to: n, frame height, spp, gray mode, task,
 * observation width, rf_num_states, whether a device initializer is configured, whether episode records are kept
 * (rf_env_configure_records: without them arrays 19 and 20 have zero length and the word is 0, so the blob is what it
 * was before that call existed, byte for byte, and the version stays 1), a hash of the learner view's configuration
 * (rf_env_configure_view: without a view arrays 21 to 23 have zero length and both view words are 0, so again the blob
 * is what it was, byte for byte), and 64-bit FNV-1a hashes of the
 * rf_env_config (with the stop threshold of rf_env_configure_jumps), the rf_env_program, the rf_env_observer_program and
 * the initializer's ranges as the library holds them -- not of the generator's words, which are content: a restore
 * brings the increment along.
 *   rf_env_snapshot_size      bytes of a snapshot of the configured context
 *   rf_env_snapshot           device -> host_out[bytes]; synchronous
 *   rf_env_restore            host_in[bytes] -> device, in place: an instantiated step graph stays valid, the next step
 *                             may be a replayed one.  Also into a context that was configured alike but never reset
 *                             (resume): the restore makes the one-time allocations rf_env_reset would have made.  Clears
 *                             the "aborted step" condition.  Synchronous.
 *   rf_env_snapshot_resident  device -> the ctx's slot (HBM, allocated on first use, freed by rf_env_snapshot_drop,
 *                             by any rf_env_configure* and by rf_destroy).  A slot costs rf_env_snapshot_size bytes of
 *                             HBM -- the RNG states are the bulk, 16 bytes per pixel: 4.29 GB for 4096 environments of
 *                             256 x 256 pixels, once per slot in use.
 *   rf_env_restore_resident   the slot -> device, in place.  Both resident forms only enqueue: later calls on the ctx
 *                             are ordered after them on its stream.
 * Refused (RF_ERR_INVALID, nothing changes): NULL arguments; a context without an environment; bytes other than
 * rf_env_snapshot_size; a blob with another magic number or version, or whose fingerprint differs from the context's
 * in any field (the message names it); a slot outside [0, RF_ENV_SNAPSHOT_SLOTS); restoring or dropping an empty slot;
 * a slot filled under a configuration the context no longer has (rf_seed, rf_env_configure_initializer); a snapshot
 * before the first rf_env_reset or after an aborted step; a snapshot or restore while a two-phase or planned step is
 * open. */
#define RF_ENV_SNAPSHOT_SLOTS 4
#define RF_ENV_SNAPSHOT_MAGIC 0x313050414e534652ull /* the bytes "RFSNAP01" */
#define RF_ENV_SNAPSHOT_VERSION 1
typedef struct rf_env_snapshot_header {
    uint64_t magic;              /* RF_ENV_SNAPSHOT_MAGIC */
    uint32_t version;            /* RF_ENV_SNAPSHOT_VERSION */
    uint32_t header_bytes;       /* 256: where the first array starts */
    uint64_t total_bytes;        /* rf_env_snapshot_size */
    /* fingerprint */
    int32_t n, frame_height, spp, gray_mode;
    int32_t task;                /* 0 DiscreteSteps, 1 ContinuousJumps, 2 composed */
    int32_t obs_width;
    int32_t device_initializer;  /* 0 / 1 */
    int32_t episode_records;     /* 0 / 1: rf_env_configure_records (was `reserved`, 0) */
    uint64_t n_states;           /* rf_num_states */
    uint64_t config_hash, program_hash, observer_hash, initializer_hash;
    /* host-side words of the scene set */
    int32_t scene_len;           /* rf_env_scene_len */
    int32_t last_partial;        /* 1: that set is the compacted one of an auto-reset */
    /* the learner view (rf_env_configure_view; both words were part of `zero`, and are 0 without a view) */
    uint64_t view_hash;          /* FNV-1a of the rf_env_view_config without `training`; never 0 with a view.  Grouped:
                                    of that without `gamma`, then G and the G gammas */
    int32_t view_training;       /* content, not fingerprint: rf_env_view_set_training's flag, restored with the blob */
    int32_t view_groups;         /* G of rf_env_configure_view_grouped; 0 (as when it was part of `zero`) ungrouped */
    uint8_t zero[136];
} rf_env_snapshot_header;
int rf_env_snapshot_size(rf_ctx *ctx, uint64_t *bytes);
int rf_env_snapshot(rf_ctx *ctx, void *host_out, uint64_t bytes);
int rf_env_restore(rf_ctx *ctx, const void *host_in, uint64_t bytes);
int rf_env_snapshot_resident(rf_ctx *ctx, int slot);
int rf_env_restore_resident(rf_ctx *ctx, int slot);
int rf_env_snapshot_drop(rf_ctx *ctx, int slot);

/* ---- device io: stepping from device arrays without a host synchronisation ---------------------------------------------
 * rf_env_step / rf_env_step_jumps take host pointers and end in a host synchronisation.  A policy network that runs on
 * the same GPU would bring its actions to the host only for the library to upload them again, and fetch results it
 * re-uploads.  The device forms take the actions where they are, in the dtype the network produces, hand the results
 * to device arrays, and only enqueue: on return nothing has necessarily run.  No reference counterpart.
 *
 * Arrays: device memory of the ctx's GPU, contiguous -- d_actions int32[n] (RF_ACTION_I32), int64[n] (RF_ACTION_I64)
 * or float32[n] (RF_ACTION_F32), d_obs float32[n][W] (W = 4, or the observer program's width), d_rewards float64[n],
 * d_truncated uint8[n] (0 / 1), d_n_reset int32[1] or NULL.  The library asks the runtime about every pointer
 * (hipPointerGetAttributes) and refuses, before anything is enqueued and without dereferencing it, whatever is not
 * device memory of that GPU, is misaligned, or is shorter than the array.  The pointers may differ from call to call.
 *
 * Ordering: caller_stream is a hipStream_t (0: the default stream).  The ctx's stream waits for an event recorded on
 * the caller's stream, the step runs, and the caller's stream waits for an event recorded after it -- so work the
 * caller enqueues next on that stream sees the results, and memory the caller's allocator hands out again later on
 * that stream is ordered after the step.  No host synchronisation.  A caller stream that is being captured is refused.
 *
 * Actions are checked on the device (env_gather_actions_kernel, one lane per environment), by the rules of the host
 * forms.  A host form refuses the whole step; a device step cannot, so an invalid action is replaced and recorded:
 *   int32 / int64 index   valid: 0 <= a < n_actions on the full 64-bit value     invalid: clamped into [0, n_actions - 1]
 *   float32 jump          valid: -1 <= a <= 1 (ContinuousJumps, ContinuousJump)  invalid: NaN -> 0, else clamped to [-1, 1]
 *   float32 otherwise     valid: finite                                          invalid: 0
 * The replacement exists only so that no kernel reads outside the action set or carries a NaN into the states: the
 * trajectory after an invalid action is NOT a valid one.  The fault word in device memory keeps the earliest step --
 * steps are counted from the last reset, whole steps of either form -- and the lowest environment within it.  FAULT
 * RULE: a recorded fault is sticky.  Device steps enqueued before anybody asks keep running on replacement values --
 * the price of not synchronising.  Once the host has seen it (rf_env_device_status, or any call listed under "deferred
 * bookkeeping"), every rf_env_step*, rf_env_snapshot* and rf_env_step_device is refused (RF_ERR_INVALID; the message
 * names step and environment) until rf_env_reset or rf_env_reset_device, which clear it.
 *
 * Schedule: the step enqueued in one go -- the fused pass, or with separate launches the full pass and the reset pass
 * over all n slots, at ANY size (the count-sized schedule of rf_env_step needs a round trip).  From the second step on
 * the step's body is replayed (where rf_env_step would replay: fused, or small enough for the one-sync schedule)
 * as a hipGraph of its own that holds none of the caller's pointers; the gather of the
 * actions and the hand-over of the results are launched around it.  rf_env_last_step_branch says RF_ENV_BRANCH_FUSED,
 * _FUSED_GRAPH, _ONE_SYNC or _GRAPH, never _COUNT_SIZED.  The graph of the host form is a different one and untouched.
 *
 * Deferred bookkeeping: what the host keeps per step that depends on the number k of environments that ended -- the
 * scene set the renderer holds (rf_env_scene_len, rf_env_render, the header of a snapshot) and the pixels rendered
 * (rf_pixels_rendered: the device keeps a running total of n + k per device step) -- is settled, with one
 * synchronisation, by the next of: rf_env_scene_len, rf_env_render, rf_env_snapshot*, rf_env_restore*, rf_timing_read,
 * rf_env_step / rf_env_step_jumps, rf_env_reset, rf_env_configure*, rf_env_device_status.  rf_pixels_rendered itself
 * takes no context and reports what has been settled.  Device and host steps may be mixed freely.
 *
 *   rf_env_step_device    one whole step.  Refused (RF_ERR_INVALID, nothing enqueued, nothing changes): a context
 *                         without a device initializer (rf_env_configure_initializer: the host's initializer advances
 *                         by k, which only a synchronisation can tell it); an open two-phase or planned step; an
 *                         aborted step; a fault already seen; RF_ACTION_I32 / _I64 on a float32 task and RF_ACTION_F32
 *                         on an index task; an array the runtime does not vouch for; a capturing caller stream.
 *   rf_env_reset_device   rf_env_reset(ctx, NULL, obs) with the observations to d_obs: all n states drawn on the
 *                         device, nothing waited for.  Clears a fault and an aborted step.
 *   rf_env_device_status  synchronises the ctx's stream, settles the bookkeeping and reports the fault: the step and
 *                         the environment, or -1 / -1. */
enum { RF_ACTION_I32 = 0, RF_ACTION_I64 = 1, RF_ACTION_F32 = 2 };
int rf_env_step_device(rf_ctx *ctx, const void *d_actions, int action_dtype, float *d_obs, double *d_rewards,
                       uint8_t *d_truncated, int32_t *d_n_reset, void *caller_stream);
int rf_env_reset_device(rf_ctx *ctx, float *d_obs, void *caller_stream);
int rf_env_device_status(rf_ctx *ctx, int *fault_step, int *fault_env);

/* ---- episode records: final observations, episode returns and lengths on the device ----------------------------------
 * Every episode of these environments ends by truncation and the step resets the environment in the same call
 * (environments/vector_environment.py:137-151): the observation row a step returns for an environment that ended is
 * already the first one of its next episode (:144-146).  With records on, the step also keeps what a learner reads at
 * an episode boundary.  No reference counterpart.  Off by default; with it off nothing a caller can observe changes.
 *
 * One definition, host twins and device alike.  Per environment e two accumulators, ep_return[e] (float64) and
 * ep_length[e] (int32); rf_env_reset / rf_env_reset_device zero them.  In a step, once the reward r[e] (the float64
 * value the step returns) and the flag are computed: ep_return[e] += r[e] (one float64 addition per step, in step
 * order), ep_length[e] += 1.  Three record arrays are then written for EVERY environment in EVERY step:
 *   where e ended this step   final_obs[e][0..W) = the observation row the step computed, before the auto-reset
 *                             overwrote it; returns[e] = ep_return[e]; lengths[e] = ep_length[e]; the accumulators are
 *                             zeroed
 *   where it did not          final_obs[e][..] = NaN; returns[e] = NaN; lengths[e] = 0
 * (W = 4, or the observer program's width.)  The records are outputs, written before they are read, like the
 * observations: they hold no stale rows, and only the accumulators are state (and part of a snapshot).  Kernels:
 * env_record_one in csrc/rf_env.h, called by env_post_kernel / env_finish_kernel -- every schedule of the step, the
 * two-phase and planned halves included.  The replayed hipGraphs hold the arrays' addresses by value: records are
 * chosen before the first step, so before any capture, and nothing in a graph depends on the caller's pointers (the
 * hand-over to the caller's arrays is launched after the replay, outside it).
 *   rf_env_configure_records       on != 0: the context keeps records from now on; 0: it stops.  After any
 *                                  rf_env_configure* (each of which turns records off again and, as before, drops the
 *                                  snapshot slots; this call drops them too) and before the first rf_env_reset.  The
 *                                  arrays are part of the environment's one allocation.  Refused (RF_ERR_INVALID,
 *                                  nothing changes): a context without an environment, one that has stepped, an open
 *                                  two-phase or planned step.
 *   rf_env_get_records             the records of the last step of any form: host_final_obs float32[n][W],
 *                                  host_returns float64[n], host_lengths int32[n], each of which may be NULL.
 *                                  Synchronous, ordered on the ctx's stream.  Refused without records, before the
 *                                  first step after a reset, and while a two-phase or planned step is open.
 *   rf_env_get_record_accumulators the running accumulators (tests, snapshot checks); either may be NULL.
 *   rf_env_step_device_records     rf_env_step_device with three more device arrays, each NULL or vouched for by the
 *                                  runtime exactly as the others: d_final_obs float32[n][W], d_returns float64[n],
 *                                  d_lengths int32[n], filled by the same hand-over launch (no extra launch).  Refused
 *                                  when records are off and any of the three is not NULL.  rf_env_step_device is this
 *                                  function with three NULLs. */
int rf_env_configure_records(rf_ctx *ctx, int on);
int rf_env_get_records(rf_ctx *ctx, float *host_final_obs, double *host_returns, int32_t *host_lengths);
int rf_env_get_record_accumulators(rf_ctx *ctx, double *host_returns, int32_t *host_lengths);
int rf_env_step_device_records(rf_ctx *ctx, const void *d_actions, int action_dtype, float *d_obs, double *d_rewards,
                               uint8_t *d_truncated, int32_t *d_n_reset, float *d_final_obs, double *d_returns,
                               int32_t *d_lengths, void *caller_stream);

/* ---- learner view: VecNormalize followed by VecFrameStack on the device ------------------------------------------------
 * Every training configuration the reference ships (examples/ppo_*.yml: normalize: true, frame_stack: 5) wraps the
 * environment in stable-baselines3's VecNormalize and then VecFrameStack.  With a view configured the context computes
 * what those wrappers hand to the learner, on the step's own outputs, by two kernels (csrc/rf_env_view.h) that follow
 * the step on the ctx's stream, outside the replayed graphs, which hold none of its pointers.  Off by
 * default; with it off nothing a caller can observe changes.
 *
 * One definition, host twin (harness._LearnerView) and device alike.  n environments, W observation columns (4, or the
 * observer program's width), k = frame_stack, V = k * W.  All parameters and moments are float64; no FMA contraction.
 * State: stack float32[n][V] (the newest frame in the last W columns), returns float64[n], and running moments (mean,
 * var, count) for each of the W columns and for the returns, which start at (0, 1, 1e-4).
 *   treesum(x[0..n))    x as float64, padded with +0.0 to the next power of two P >= n; y = y[0::2] + y[1::2] until one
 *                       value is left; that value + (+0.0) (-0.0 becomes +0.0, so further zero padding changes nothing).
 *   update(moments, x)  N = float64(n); bm = treesum(x) / N; bv = treesum((x - bm) * (x - bm)) / N; delta = bm - mean;
 *                       tot = count + N; mean' = mean + (delta * N) / tot; m2 = (var * count + bv * N) + (((delta * delta)
 *                       * count) * N) / tot; var' = m2 / tot; count' = tot  (RunningMeanStd.update_from_moments, left
 *                       to right).
 *   normalise(row)      with norm_obs, per column c: float32(clip((float64(row[c]) - mean[c]) / sqrt(var[c] + epsilon),
 *                       -clip_obs, clip_obs)); without, the row unchanged.
 * After a reset of any form (a reset never resets the moments): returns = 0; if training and norm_obs, update every
 * observation column with the reset's observations; o = normalise(obs); stack = 0, then stack[:, -W:] = o.
 * After a step, given its raw obs (rows of environments that ended are already the first of their next episode),
 * reward (float64), truncated and -- with episode records -- the raw final_obs:
 *   1 if training and norm_obs: update every observation column with obs        2 o = normalise(obs)
 *   3 if training: returns = returns * gamma + reward, then update the return moments with returns
 *   4 view reward: with norm_reward clip(reward / sqrt(ret_var + epsilon), -clip_reward, clip_reward), else reward
 *   5 every stack row moves left by W                                            8 stack[:, -W:] = o
 *   6 with records, where e ended: view_final[e] = concat(stack[e][:V - W], normalise(final_obs[e])), by the moments of
 *     step 1; NaN elsewhere.  Without records there is no view_final.
 *   7 where e ended: stack[e] = 0 and returns[e] = 0
 * This is VecNormalize.step_wait followed by StackedObservations.update, as rl_zoo3 applies them.  ONE DELIBERATE
 * DIFFERENCE: SB3 takes the batch mean and variance with numpy.mean / numpy.var in the observation's dtype (float32) and
 * in numpy's own order; the view takes them in float64 with the fixed tree above -- more accurate, and reproducible on
 * a GPU.  The view observation is `stack`.
 *
 *   rf_env_configure_view        cfg != NULL: the context keeps a view from now on; NULL: it stops.  After any
 *                                rf_env_configure* (each of which turns the view off again, rf_env_configure_records
 *                                included: ask for records first), before the first rf_env_reset.  Refused
 *                                (RF_ERR_INVALID, nothing changes): a context without an environment, one that has
 *                                stepped, an open two-phase or planned step, frame_stack outside 1 to 8, epsilon or a
 *                                clip that is not finite and positive, gamma outside [0, 1].
 *   With a view, rf_env_reset, rf_env_reset_device, rf_env_step, rf_env_step_jumps and rf_env_step_device* end by
 *   enqueueing the view's kernels, on every schedule; what they return stays raw.  The two-phase and planned forms
 *   (rf_env_step_begin*, _plan*, _run, _end*, rf_env_render_states) are refused while a view is configured.
 *   rf_env_get_view              the view of the last step or reset: host_obs float32[n][V], host_rewards float64[n]
 *                                (of a step), host_final float32[n][V] (of a step; refused without episode records).
 *                                Each may be NULL.  Synchronous: one copy into one pinned block.
 *   rf_env_view_get_statistics   mean / var / count, float64[W + 1] each, the returns last (what VecNormalize.save
 *   rf_env_view_set_statistics   keeps); each pointer may be NULL.  Synchronous.
 *   rf_env_view_set_training     VecNormalize.training: 0 freezes the moments and the returns.
 *   rf_env_view_get_state        stack float32[n][V] and returns float64[n] (tests); either may be NULL.
 *   rf_env_step_device_view      rf_env_step_device_records with d_view_obs float32[n][V], d_view_rewards float64[n] and
 *                                d_view_final float32[n][V], each NULL or vouched for by the runtime exactly as the
 *                                others and filled by the view's own launch, without a host synchronisation.
 *                                d_view_final is refused without records; all three without a view.
 *   rf_env_reset_device_view     rf_env_reset_device with the view observation to d_view_obs (or NULL). */
typedef struct rf_env_view_config {
    int32_t frame_stack;            /* 1 to 8 */
    int32_t norm_obs, norm_reward;  /* 0 / 1 */
    int32_t training;               /* 0 / 1; the only one rf_env_view_set_training changes later */
    double gamma, epsilon, clip_obs, clip_reward; /* SB3: 0.99, 1e-8, 10, 10 */
} rf_env_view_config;
int rf_env_configure_view(rf_ctx *ctx, const rf_env_view_config *cfg);
int rf_env_get_view(rf_ctx *ctx, float *host_obs, double *host_rewards, float *host_final);
int rf_env_view_get_statistics(rf_ctx *ctx, double *mean, double *var, double *count);
int rf_env_view_set_statistics(rf_ctx *ctx, const double *mean, const double *var, const double *count);
int rf_env_view_set_training(rf_ctx *ctx, int training);
int rf_env_view_get_state(rf_ctx *ctx, float *host_stack, double *host_returns);
int rf_env_step_device_view(rf_ctx *ctx, const void *d_actions, int action_dtype, float *d_obs, double *d_rewards,
                            uint8_t *d_truncated, int32_t *d_n_reset, float *d_final_obs, double *d_returns,
                            int32_t *d_lengths, float *d_view_obs, double *d_view_rewards, float *d_view_final,
                            void *caller_stream);
int rf_env_reset_device_view(rf_ctx *ctx, float *d_obs, float *d_view_obs, void *caller_stream);

/* ---- population view: a normaliser and GAE discounts per group of a population -----------------------------------------
 * The population ("population", below) trains G PPO learners in lock-step over one environment of n = G m lanes, group g
 * owning lanes [g m, (g + 1) m); write g(e) = e / m.  For those G learners to be G independent trials -- the
 * reference's examples/optimize_hyperparameters.py runs trials of n_envs: 8 with normalize: true, and gamma and
 * gae_lambda are among the first things rl_zoo3's sample_ppo_params draws -- each group has running moments of its own
 * and discounts of its own.  One definition, host twins (harness._GroupedLearnerView: literally G _LearnerView objects
 * over lane slices; rollout.gae_numpy_grouped) and device alike.
 *
 * State and parameters: moments float64 [G][3][17] (mean, var, count), every group starting at (0, 1, 1e-4); gamma
 * float64 [G].  The definition of "learner view" changes only as follows:
 *   update(moments[g], x[g m .. (g + 1) m))  N = float64(m); treesum runs over the group's m leaves, padded with +0.0 to
 *                       P_m, the next power of two >= m (treesum itself is unchanged, its final + (+0.0) included).
 *   step 3              returns[e] = returns[e] * gamma[g(e)] + reward[e], then one update of slot W per group, from that
 *                       group's returns.
 *   normalise           by moments[g(e)]; the view reward by moments[g(e)].var[W].
 * The stack shift, view_final, the zeroing of ended lanes, training, epsilon and the clips are unchanged and common to
 * all groups.  GAE ("rollout") changes only in that g and gl are per lane: g = float32(gamma[g(e)]),
 * gl = float32(gamma[g(e)] * gae_lambda[g(e)]) with the product taken in float64, also in the bootstrap
 * r + g * final_values.  With G = 1 every result is bit for bit the ungrouped one.  VecNormalize's gamma (here) and the
 * rollout's gamma (d_discounts) are passed separately; rl_zoo3 sets both from the trial's gamma.
 *
 * Kernels (csrc/rf_env_view.h, csrc/rf_rollout.h): a step still makes one moments launch and one apply launch.  Groups
 * of at most 64 lanes (P_m <= 64) take env_view_moments_packed_kernel -- 256 / P_m groups of one slot per 256-thread
 * block, the tree a xor-butterfly inside the segment's wave, no LDS and no barrier --, wider groups
 * env_view_moments_kernel<true> with one block per (slot, group).
 *
 *   rf_env_configure_view_grouped       rf_env_configure_view with `groups` groups; gammas: host double[groups], or NULL
 *                                       for cfg->gamma in every group (cfg->gamma is otherwise not used).  Refused with
 *                                       nothing changed: everything rf_env_configure_view refuses, a NULL cfg, groups
 *                                       outside 1 .. RF_POPULATION_MAX_GROUPS, n not divisible by groups, a gamma outside
 *                                       [0, 1].  rf_env_configure_view and rf_env_view_config do not change.
 *   rf_env_view_get_statistics_grouped  mean / var / count, float64 [G][W + 1] each; each pointer may be NULL.  The
 *   rf_env_view_set_statistics_grouped  ungrouped accessors are refused on a context configured with the grouped call,
 *                                       these on any other.
 *   rf_rollout_advantages_grouped       rf_rollout_advantages with d_discounts, device float32 [groups][2] holding
 *                                       (g, gl) per group, 8-byte aligned, the caller's and vouched for like the other
 *                                       arrays, in place of the two scalars.  Refusals: rf_rollout_advantages's, a NULL
 *                                       d_discounts, groups outside 1 .. RF_POPULATION_MAX_GROUPS, n not divisible by groups.
 * Snapshots: for a grouped context array 23 is float64 [G][3][17], the header's view_groups word is G, and view_hash also
 * covers G and the gammas; ungrouped blobs stay byte for byte what they are.  A grouped blob into an ungrouped context,
 * or into one with other gammas, is refused with nothing changed, and so is the reverse.
 *
 * Out of scope: the sde, lstm and lstm-sde heads; groups that differ in m, T, B or architecture; SB3Wrapper; and the
 * environment's shared reset-state generator -- lanes that end are ranked across all groups, so which reset state a lane
 * draws depends on other groups' episode ends.  The independence claimed here covers what the learner is given the raw
 * step; it does not cover the environment's draws. */
int rf_env_configure_view_grouped(rf_ctx *ctx, const rf_env_view_config *cfg, int groups, const double *gammas);
int rf_env_view_get_statistics_grouped(rf_ctx *ctx, double *mean, double *var, double *count);
int rf_env_view_set_statistics_grouped(rf_ctx *ctx, const double *mean, const double *var, const double *count);
int rf_rollout_advantages_grouped(rf_ctx *ctx, int T, int n, int groups, const double *d_rewards, const float *d_values,
                                  const uint8_t *d_truncated, const float *d_final_values, const float *d_last_values,
                                  const float *d_discounts, float *d_advantages, float *d_returns, void *caller_stream);

/* ---- rollout: GAE advantages and returns of a PPO rollout in one launch -----------------------------------------------
 * The consumer of device steps in the reference's PPO configurations is stable-baselines3's RolloutBuffer: T = n_steps
 * steps of n environments, then GAE(gamma, lambda) advantages and returns (compute_returns_and_advantage), with the
 * bootstrap of OnPolicyAlgorithm.collect_rollouts for steps that ended by truncation -- which is how every episode here
 * ends, the step resetting the environment in the same call.  No reference counterpart.  Needs no environment: the
 * context only says which GPU.
 *
 * One definition, numpy twin (environments/rollout.py gae_numpy) and kernel (csrc/rf_rollout.h) alike.  Arrays are
 * [T][n] row-major: d_rewards float64, d_values float32, d_truncated uint8 (0 / 1), d_final_values float32 or NULL,
 * d_advantages and d_returns float32; d_last_values float32[n].  g = float32(gamma), gl = float32(gamma * gae_lambda)
 * with the product taken in float64.  Every operation below is float32, left to right, no FMA contraction:
 *   r      = float32(rewards[t][e]);  where d_final_values is given and truncated[t][e]: r = r + g * final_values[t][e]
 *            (a select: final_values of a step that did not end -- NaN in practice -- never reaches the result)
 *   nnt    = 1.0f - float32(truncated[t][e])     (episode_starts[t+1] == truncated[t], dones == truncated[T-1])
 *   next_v = last_values[e] if t == T-1 else values[t+1][e]
 *   delta  = (r + (g * next_v) * nnt) - values[t][e]
 *   last   = delta + (gl * nnt) * last           (last = 0.0f before t = T-1; t runs T-1 .. 0)
 *   advantages[t][e] = last;  returns[t][e] = last + values[t][e]
 * ONE DELIBERATE DIFFERENCE: SB3 adds the bootstrap in whatever dtype the wrapper stack left the rewards in; here it is
 * a float32 addition after the cast.
 *
 *   rf_rollout_advantages   one launch on caller_stream (a hipStream_t; 0: the default stream): every array is the
 *                           caller's, so nothing is handed over by events and the host waits for nothing.  Refused
 *                           (RF_ERR_INVALID, nothing enqueued, no pointer dereferenced): T < 1 or n < 1; a NULL array
 *                           other than d_final_values; an array the runtime does not vouch for on the ctx's GPU, exactly
 *                           as for device io; an output that overlaps an input or the other output; a capturing caller
 *                           stream. */
int rf_rollout_advantages(rf_ctx *ctx, int T, int n, const double *d_rewards, const float *d_values,
                          const uint8_t *d_truncated, const float *d_final_values, const float *d_last_values, double gamma,
                          double gae_lambda, float *d_advantages, float *d_returns, void *caller_stream);

/* ---- policy: the PPO actor-critic forward with sampling in one launch -------------------------------------------------
 * What turns an observation into the next action, its log-probability and V(obs) in the reference's PPO configurations
 * is stable-baselines3's MlpPolicy (ActorCriticPolicy with separate pi / vf extractors and a Categorical head).  No
 * reference counterpart.  Needs no environment: the context only says which GPU.
 *
 * One definition, numpy twin (environments/policy.py policy_numpy), host build (tests/policycheck) and kernel
 * (csrc/rf_policy.h) alike; the scalar functions are csrc/rf_policy_math.h.
 *
 * Network.  Two nets, pi and vf, each with 1 or 2 hidden layers of width 1 .. RF_POLICY_MAX_WIDTH; input width
 * obs_width 1 .. RF_POLICY_MAX_WIDTH; the pi head has n_actions 2 .. RF_POLICY_MAX_ACTIONS outputs (the logits of a
 * Categorical), the vf head one.  One activation for both nets.  Continuous action spaces (the reference trains
 * ContinuousJumps with gSDE) have the Gaussian head of "sde policy" below; this entry point refuses them.
 * Parameters: one float32 array, every matrix TRANSPOSED ([in][out] row-major: SB3's weight.T), in this order:
 *   pi: W0^T, b0, (W1^T, b1,) Wa^T [last][n_actions], ba;   vf: W0^T, b0, (W1^T, b1,) Wv^T [last][1], bv
 * Linear layer: y_j = b_j; for k = 0 .. K-1: y_j = y_j + x_k * W[j][k] -- a float32 multiply, then a float32 add, in
 * that order, no FMA.  No MFMA: its internal accumulation order is not documented.
 * Activation: relu(x) = x > 0 ? x : 0 (NaN and -0 become +0), or tanh32(x) = sign(x) * (1 - t) / (1 + t) with
 * t = exp32(-2 |x|); tanh32(NaN) is NaN.
 * exp32 (x <= 0; +0 for x < -87, for -inf and for NaN; exp32(0) == 1; never a subnormal) and log32 (every positive normal number; the Categorical head
 * calls it on [1, 64]) are the project's own: float32 + - * / (correctly rounded), comparisons, float <-> int conversions and integer operations on
 * the exponent field only -- csrc/rf_policy_math.h is the text.
 * Head.  With logits l_i: m = the first maximum (m = l_0; l_i > m replaces it: a NaN l_0 stays, NaNs elsewhere are never
 * the maximum), z_i = l_i - m, e_i = exp32(z_i), c_i the sequential float32 partial sums of e, s = c_{A-1},
 * log_prob_i = z_i - log32(s).  Sampled action: the first i with double(c_i) > u * double(s) (one float64 multiply,
 * exact conversions), the last index if there is none.  Deterministic action: the first maximum.
 * NaN and +-inf logits: a -inf or NaN logit next to a finite maximum has e_i = 0 and is never sampled.  Where no e_i is
 * 1 -- l_0 is NaN, or the maximum is +inf or -inf -- s < 1: the row is degenerate, its action is the first maximum
 * (sampled or not; its draw is still consumed) and its log_prob is NaN.
 * Every NaN that is stored (logits, log_probs, values, final_values) is the bit pattern 0x7fc00000.
 * Random numbers.  u of environment e is draw number e of numpy.random.Generator(PCG64DXSM) in the state `gen` =
 * {state low, state high, inc low, inc high}: (next64 >> 11) * 2^-53.  The caller advances its generator by n after a
 * sampled call; a deterministic or values-only call uses none.  No generator state lives on the device.
 * V(final_observation).  With d_final_obs [n][obs_width] and d_final_values: final_values[e] = V(final_obs[e]), and NaN
 * where final_obs[e][0] is NaN (the rows episode records write where no episode ended).
 *
 *   rf_policy_params_size   floats of the packed parameters of desc; 0 for a desc outside the limits or a NULL ctx
 *                           (it takes the ctx as every entry point does and makes its GPU current, no more).
 *   rf_policy_forward       one launch on caller_stream (a hipStream_t; 0: the default stream), nothing allocated,
 *                           nothing waited for.  Outputs (each may be NULL): d_actions int64[n], d_log_probs float32[n]
 *                           (needs d_actions), d_values float32[n], d_final_values float32[n] (needs d_final_obs),
 *                           d_logits float32[n][n_actions]; at least one must be given.  gen is read on the host and
 *                           needed unless flags has RF_POLICY_DETERMINISTIC or d_actions is NULL.  Refused
 *                           (RF_ERR_INVALID, nothing enqueued, no device pointer dereferenced): a desc outside the
 *                           limits, n < 1, unknown flags, an array the runtime does not vouch for on the ctx's GPU
 *                           (a host pointer, a misaligned one, one that ends past its allocation) exactly as for
 *                           device io, an output that overlaps an input or another output. */
#define RF_POLICY_MAX_WIDTH 256
#define RF_POLICY_MAX_ACTIONS 64
#define RF_POLICY_RELU 0
#define RF_POLICY_TANH 1
#define RF_POLICY_DETERMINISTIC 1

typedef struct rf_policy_desc {
    int obs_width;   /* 1 .. RF_POLICY_MAX_WIDTH */
    int n_actions;   /* 2 .. RF_POLICY_MAX_ACTIONS */
    int activation;  /* RF_POLICY_RELU or RF_POLICY_TANH */
    int pi_layers;   /* 1 or 2 */
    int pi_width[2]; /* 1 .. RF_POLICY_MAX_WIDTH each; [1] ignored with one layer */
    int vf_layers;
    int vf_width[2];
} rf_policy_desc;

unsigned long long rf_policy_params_size(rf_ctx *ctx, const rf_policy_desc *desc);
int rf_policy_forward(rf_ctx *ctx, const rf_policy_desc *desc, const float *d_params, int n, const float *d_obs,
                      const float *d_final_obs, const unsigned long long gen[4], int flags, long long *d_actions,
                      float *d_log_probs, float *d_values, float *d_final_values, float *d_logits, void *caller_stream);

/* ---- ppo update: one PPO minibatch update on the device: loss, backward, clip, Adam ---------------------------------------
 * The other half of training in the reference's PPO configurations is stable-baselines3's PPO.train(): per minibatch the
 * clipped surrogate loss, the value loss and the entropy bonus of the actor-critic of "policy" above, their gradient,
 * clip_grad_norm_ and one Adam step.  No reference counterpart.  Needs no environment: the context only says which GPU.
 *
 * One definition, numpy twin (environments/learner.py ppo_update_numpy), host build (tests/ppocheck) and kernels
 * (csrc/rf_ppo.h) alike.  Everything is float32, left to right, one rounding per operation, nothing contracted, unless a
 * step says float64; no MFMA; every reduction has a fixed order.  treesum is the learner view's, above.
 *
 * Inputs.  Arrays of N rows (what a rollout's flat() holds): obs float32[N][D], actions int64[N], old_log_probs,
 * advantages, returns float32[N]; index int64[B], 1 <= B <= RF_PPO_MAX_BATCH: sample b of the minibatch is row
 * index[b], repeats allowed.  rf_ppo_desc holds the hyper-parameters, by value per call.
 *  1 Validity.  invalid = some index[b] outside [0, N) or some actions[row] outside [0, A).  Every gather uses
 *    row = clamp(index[b], 0, N - 1) and a = clamp(actions[row], 0, A - 1): no address outside the arrays is formed.
 *  2 Advantages.  With normalize_advantage and B > 1: mean = treesum(adv) / B, var = treesum((adv - mean) * (adv - mean))
 *    / (B - 1), float64 (adv converted exactly); A_b = float32((double(adv_b) - mean) / (sqrt(var) + 1e-8)).  Otherwise
 *    A_b = adv_b.
 *  3 Forward.  Both nets of "policy" on obs[row]: linear layers, activation, and for the logits l: m = the first maximum,
 *    z_i = l_i - m, e_i = exp32(z_i), s the sequential sum of e from +0; lse = log32(s), or NaN where not s >= 1 (a
 *    degenerate row: it ends in RF_PPO_NONFINITE); logp_i = z_i - lse, p_i = e_i / s.
 *    H_b = -(sum over i in index order, from +0, of (e_i == 0 ? +0 : p_i * logp_i)).
 *  4 Loss terms, a as above: d = logp_a - old_log_probs[row]; ratio = d <= 0 ? exp32(d) : 1.0f / exp32(-d);
 *    c = float32(clip_range), lo = 1.0f - c, hi = 1.0f + c; cl = ratio < lo ? lo : (ratio > hi ? hi : ratio);
 *    surr1 = A_b * ratio, surr2 = A_b * cl; pg_b = -(surr2 < surr1 ? surr2 : surr1); t = ret - v, vl_b = t * t;
 *    kl_b = (ratio - 1.0f) - d; r1 = ratio - 1.0f, clipped_b = (r1 < 0 ? -r1 : r1) > c ? 1.0f : 0.0f.
 *  5 Head gradients (torch's subgradient of min and clamp): g_b = surr1 if (ratio >= lo and ratio <= hi) or
 *    surr1 < surr2, else +0; Bf = float32(B), ec = float32(ent_coef), vc2 = float32(vf_coef) * 2.0f;
 *    dlogit_i = ((-g_b) * ((i == a ? 1.0f : 0.0f) - p_i) + (e_i == 0 ? +0 : (ec * p_i) * (logp_i + H_b))) / Bf;
 *    dv_b = (vc2 * (v - ret)) / Bf.
 *  6 Backward.  For a layer with outputs o and inputs k (a hidden activation h_k):
 *    delta_in[k] = act'(h_k) * (sum over o in index order, from +0, of W[o][k] * delta_out[o]) -- a multiply, then an add;
 *    act' = 1.0f - h * h for tanh, h > 0 ? 1.0f : 0.0f for ReLU (the multiply by it is always performed).
 *  7 Parameter gradients, in the packed layout: dW[k][j] = sum over b = 0 .. B-1, from +0, of x[b][k] * delta[b][j] (a
 *    multiply, then an add); db[j] = the same sum of delta[b][j].
 *  8 Clip.  norm = sqrt(treesum over the P packed gradients of double(g) * double(g)), float64.  (The kernels take the
 *    tree in two levels, aligned blocks of 256 leaves first: the same tree.)  If invalid, or norm is not finite
 *    (RF_PPO_NONFINITE -- a deliberate difference from SB3, which would write NaN into every parameter), the update
 *    changes nothing.  Otherwise q = max_grad_norm / (norm + 1e-6), coef = float32(q < 1.0 ? q : 1.0), g = g * coef
 *    (always applied, as clip_grad_norm_ does).
 *  9 Adam (torch's, no weight decay, no amsgrad).  State: a header {step int64, bc1 float64, bc2 float64, 0} of 32 bytes,
 *    then m float32[P], v float32[P]; all zero is a fresh optimizer.  bc1' = 1.0 - beta1 * (1.0 - bc1), bc2' alike
 *    (bc = 1 - beta^step without pow), step' = step + 1.  b1 = float32(beta1), ob1 = float32(1.0 - beta1), b2, ob2 alike;
 *    m = b1 * m + ob1 * g;  v = b2 * v + ob2 * (g * g);  denom = sqrt32(v) / float32(sqrt(bc2')) + float32(adam_eps);
 *    p = p - float32(learning_rate / bc1') * (m / denom).  Deliberate differences from torch: the running bc and this
 *    order in place of lerp / addcdiv.
 * 10 Stats float32[8]: [0..4] = float32(treesum over b / B) of pg, vl, H, kl, clipped (float64 sums of the float32
 *    terms); [5] = float32(norm) before clipping; [6] = (stats[0] + ec * (-stats[2])) + float32(vf_coef) * stats[1];
 *    [7] = 0, RF_PPO_INVALID (which takes precedence) or RF_PPO_NONFINITE as a number.  Stored NaNs are 0x7fc00000.  A
 *    skipped update still writes the stats; parameters, m, v and the header keep their bytes.
 *
 *   rf_ppo_state_size      bytes of the optimizer state of desc (32 + 8 P); 0 for a desc outside the limits or NULL ctx
 *   rf_ppo_workspace_size  bytes of the workspace for minibatches up to max_batch (1 .. RF_PPO_MAX_BATCH); 0 if refused
 *   rf_ppo_update          three launches on caller_stream, nothing allocated, nothing waited for; d_params, d_state and
 *                          d_stats (float32[8]) are updated in place, d_workspace is scratch.  Refused (RF_ERR_INVALID,
 *                          nothing enqueued, no device pointer dereferenced): a desc outside the limits; N < 1; B outside
 *                          1 .. RF_PPO_MAX_BATCH; a negative or non-finite hyper-parameter, a beta outside [0, 1); a NULL
 *                          array, one the runtime does not vouch for on the ctx's GPU (a host pointer, a misaligned one --
 *                          state and workspace to 8 bytes --, one that ends past its allocation: that is how a state or
 *                          workspace that is too small shows, where the allocation is the caller's own), exactly as for
 *                          device io; an output (params, state, workspace, stats) that overlaps an input or another
 *                          output; a capturing caller stream.  The workspace needs rf_ppo_workspace_size(B) bytes. */
#define RF_PPO_MAX_BATCH 1024
#define RF_PPO_INVALID 1
#define RF_PPO_NONFINITE 2

typedef struct rf_ppo_desc {
    double learning_rate, clip_range, ent_coef, vf_coef, max_grad_norm, beta1, beta2, adam_eps;
    int normalize_advantage; /* 0 / 1 */
    int reserved;            /* 0 */
} rf_ppo_desc;

unsigned long long rf_ppo_state_size(rf_ctx *ctx, const rf_policy_desc *policy);
unsigned long long rf_ppo_workspace_size(rf_ctx *ctx, const rf_policy_desc *policy, int max_batch);
int rf_ppo_update(rf_ctx *ctx, const rf_policy_desc *policy, const rf_ppo_desc *ppo, float *d_params, void *d_state,
                  void *d_workspace, int N, const float *d_obs, const long long *d_actions, const float *d_old_log_probs,
                  const float *d_advantages, const float *d_returns, int B, const long long *d_index, float *d_stats,
                  void *caller_stream);

/* ---- sde policy: the state-dependent-exploration Gaussian actor-critic and its PPO update ------------------------------
 * The reference's second task, ContinuousJumps-v0 (Box(-1, 1, (1,))), is trained by its PPO configurations with
 * use_sde: stable-baselines3's ActorCriticPolicy(use_sde=True), i.e. StateDependentNoiseDistribution with full_std=True,
 * use_expln=False, squash_output=False, learn_features=False, epsilon=1e-6, for an action of ONE dimension (any other
 * action width is refused: rf_policy_desc.n_actions must be 1 here).  No reference counterpart.
 *
 * One definition, numpy twin (environments/sde.py), host build (tests/sdecheck) and kernels (csrc/rf_sde.h, csrc/rf_ppo.h)
 * alike; the scalar functions are csrc/rf_policy_math.h.  Everything is float32, one rounding per operation, nothing
 * contracted, unless a step says float64.
 *
 *  S1 Network.  The two MLPs of "policy", unchanged; the pi head has one output, the mean mu.  New parameter log_std[L],
 *     L = the width of the last pi hidden layer (SB3's log_std [L, 1], state_dict name "log_std").
 *  S2 Packing.  Everything "policy" packs, at the same offsets (with a pi head of one output), then log_std[L]: P + L floats.
 *  S3 Scalar functions.  expw32(x) = x <= 0 ? exp32(x) : 1.0f / exp32(-x) (+inf for x > 87 and for NaN).  log32 as above.
 *     log64: log32's scheme in float64 (twelve series terms, a two-constant ln 2), about 2e-16 relative.
 *     normal32(u), u a draw j * 2^-53: M. J. Wichura's AS 241 PPND16 evaluated in FLOAT64 (correctly rounded + - * /
 *     sqrt, nothing contracted: the one scalar function here that is not float32 inside) on a float32 argument, and
 *     rounded to float32 once at the end.  upper = u >= 0.5; pf = float32(upper ? 1.0 - u : u) (the subtraction is exact),
 *     raised to 2^-54 if smaller (u = 0 gives about -8.29, finite); p = double(pf).  pf >= 0.075f: q = upper ? 0.5 - p :
 *     p - 0.5, r = 0.180625 - q * q, x = (q * A(r)) / B(r).  Else r = sqrt(-log64(p)); r <= 5: r = r - 1.6,
 *     x = C(r) / D(r); else r = r - 5.0, x = E(r) / F(r); x is negated in the lower half.  A .. F are PPND16's
 *     polynomials by Horner from the leading coefficient (c + r * acc).  normal32 = float32(x); normal32(0.5) is +0.
 *     It is finite for every draw and never decreases in u: neighbouring float32 arguments move the exact quantile by more
 *     than 7e-9, a million times the float64 evaluation's error (branch joins included), so the float64 values increase
 *     strictly and the final rounding keeps their order -- which a float32 evaluation, moving by about one ulp per step of
 *     p, cannot promise.  Checked on all 444 596 224 pairs of neighbouring float32 arguments of [2^-54, 1/2] in both
 *     halves (profiles/sde.md); tests/test_sde_logic.py repeats the joins, the ends and a dense sample.
 *  S4 Shared quantities, h = the activations of the last pi hidden layer: std_k = expw32(log_std_k), std2_k = std_k * std_k;
 *     var = sum over k in index order, from +0, of (h_k * h_k) * std2_k (multiply, multiply, add);
 *     sigma = sqrt32(var + 1e-6f).
 *  S5 Exploration noise.  theta[e][k] = normal32(u) * std_k, u = draw number e * L + k of Generator(PCG64DXSM) in the state
 *     `gen` (jump-ahead, as "policy" draws); a NaN product (0 * inf) is stored as 0x7fc00000.  theta changes only by a
 *     reset, which advances the caller's generator by n * L.  No generator state lives on the device.
 *  S6 Actions.  mu = the pi head (policy's linear layer).  Sampled raw action a = mu + (sum over k in index order, from
 *     +0, of h_k * theta[e][k]); deterministic: a = mu.  Environment action = a < -1 ? -1 : (a > 1 ? 1 : a): NaN stays
 *     NaN, so the environment's own check records it.  The rollout keeps the raw action, as SB3 does.
 *  S7 log_prob = ((-q) - log32(sigma)) - float32(0.9189385332046727), t = a - mu, q = (t * t) / (2.0f * (sigma * sigma));
 *     entropy = float32(1.4189385332046727) + log32(sigma).  Both are NaN where sigma is not finite.
 *  S8 Values: V(obs) and V(final_obs) exactly as "policy".  Stored NaNs are 0x7fc00000.
 * The update is "ppo update" with these steps replaced (2, 4 from d on, 8, 9 and 10 are unchanged, over P + L parameters):
 *  1' Validity.  invalid = some index[b] outside [0, N) or some actions[row] NaN (actions float32[N], the raw actions).
 *  3' Forward.  mu, sigma as S4 / S6 on obs[row]; logp = S7 for the stored action; H_b = the entropy of S7.
 *  5' Head gradients, g_b as step 5, ng = -g_b, t = a - mu, v2 = sigma * sigma:
 *     dmu_b  = (ng * (t / v2)) / Bf;
 *     dsig_b = (((ng * ((t * t) / (v2 * sigma) - 1.0f / sigma)) - ec / sigma) / Bf) / sigma.
 *     A row whose sigma or logp is not finite has dmu_b = dsig_b = NaN: the update ends in RF_PPO_NONFINITE.
 *  6' Backward.  The pi net gets its gradient through mu only (delta of the head = dmu_b); h is a constant inside var
 *     (learn_features=False).
 *  7' dlog_std_k = sum over b = 0 .. B-1, from +0, of ((h[b][k] * h[b][k]) * std2_k) * dsig_b: log_std gets its gradient
 *     through sigma only, from the policy loss and the entropy term.
 *
 *   rf_sde_params_size     floats of the packed parameters (P + L); 0 for a desc outside the limits or a NULL ctx
 *   rf_sde_noise_reset     one launch: d_theta float32[n][L] from gen and the log_std inside d_params
 *   rf_sde_forward         one launch.  Outputs (each may be NULL, one must be given): d_actions float32[n] (raw),
 *                          d_env_actions float32[n] (clamped), d_log_probs, d_values, d_final_values (needs d_final_obs),
 *                          d_mean, d_sigma float32[n].  d_theta is needed unless flags has RF_POLICY_DETERMINISTIC or no pi
 *                          output is asked for.  Refusals as rf_policy_forward's.
 *   rf_sde_state_size, rf_sde_workspace_size, rf_sde_update
 *                          as their rf_ppo_ siblings, over P + L parameters and float32 actions; the same refusals. */
unsigned long long rf_sde_params_size(rf_ctx *ctx, const rf_policy_desc *desc);
int rf_sde_noise_reset(rf_ctx *ctx, const rf_policy_desc *desc, const float *d_params, int n,
                       const unsigned long long gen[4], float *d_theta, void *caller_stream);
int rf_sde_forward(rf_ctx *ctx, const rf_policy_desc *desc, const float *d_params, int n, const float *d_obs,
                   const float *d_final_obs, const float *d_theta, int flags, float *d_actions, float *d_env_actions,
                   float *d_log_probs, float *d_values, float *d_final_values, float *d_mean, float *d_sigma,
                   void *caller_stream);
unsigned long long rf_sde_state_size(rf_ctx *ctx, const rf_policy_desc *policy);
unsigned long long rf_sde_workspace_size(rf_ctx *ctx, const rf_policy_desc *policy, int max_batch);
int rf_sde_update(rf_ctx *ctx, const rf_policy_desc *policy, const rf_ppo_desc *ppo, float *d_params, void *d_state,
                  void *d_workspace, int N, const float *d_obs, const float *d_actions, const float *d_old_log_probs,
                  const float *d_advantages, const float *d_returns, int B, const long long *d_index, float *d_stats,
                  void *caller_stream);

/* ---- lstm policy: the recurrent PPO actor-critic forward with its state and sampling in one launch ---------------------
 * The reference's other two training configurations (examples/ppo_lstm_*.yml) run policy: 'MlpLstmPolicy', sb3-contrib's
 * RecurrentPPO with RecurrentActorCriticPolicy at its defaults: lstm_hidden_size=256, n_lstm_layers=1, shared_lstm=False,
 * enable_critic_lstm=True.  No reference counterpart.  Needs no environment: the context only says which GPU.
 * The update (back-propagation through time) is "lstm update" below; the Gaussian (sde) head on top of the LSTM is "lstm
 * sde policy" further down; enable_critic_lstm=False (a feed-forward critic) is "lstm critic" at the end.  Out of scope:
 * n_lstm_layers > 1, shared_lstm=True, lstm_hidden_size > RF_POLICY_MAX_WIDTH.
 *
 * One definition, numpy twin (environments/lstm.py lstm_numpy), host build (tests/lstmcheck) and kernel (csrc/rf_lstm.h)
 * alike; the scalar functions are csrc/rf_policy_math.h.  Everything is float32, one rounding per operation, nothing
 * contracted; no MFMA.
 *
 *  L1 Network.  Two nets, pi and vf; each is ONE LSTM layer of input width obs_width D (1 .. RF_POLICY_MAX_WIDTH) and
 *     lstm_hidden units H (1 .. RF_POLICY_MAX_WIDTH, the same for both nets), followed by the MLP of "policy" (1 or 2 hidden
 *     layers, input width H) and its head: Categorical over n_actions for pi, one output for vf, exactly as "policy".
 *  L2 Cell: torch.nn.LSTM's, gates in torch's order q = i, f, g, o.  For unit j and gate q:
 *     a = b_ih[q][j];  a = a + b_hh[q][j];  for k = 0 .. D-1: a = a + x_k * W_ih[q][j][k];
 *     for k = 0 .. H-1: a = a + h_k * W_hh[q][j][k]  -- a float32 multiply, then a float32 add, in that order, no FMA.
 *     i = sigmoid32(a_i), f = sigmoid32(a_f), g = tanh32(a_g), o = sigmoid32(a_o);
 *     c' = f * c + i * g (two multiplies, then one add);  h' = o * tanh32(c').  h' is the MLP's input.
 *  L3 sigmoid32(x): t = exp32(-|x|) (exp32 is defined for arguments <= 0 only); x >= 0 ? 1 / (1 + t) : t / (1 + t);
 *     sigmoid32(NaN) is NaN.  tanh32 and exp32 as "policy".
 *  L4 Episode starts.  episode_starts uint8[n]; any non-zero byte is a start: that environment's h and c of BOTH nets are
 *     replaced by +0.0 before the cell -- a select, not sb3-contrib's multiplication by (1 - start): a NaN or inf in a dead
 *     state does not survive a reset (a deliberate difference).
 *  L5 State.  float32 [2 nets: pi, vf][2: h, c][n][H].  A forward reads d_state_in and, if d_state_out is given, writes
 *     h' and c' of both nets there.  d_state_out may be d_state_in itself (an update in place) or a range that does not
 *     overlap it; any other overlap is refused.
 *  L6 V(final_observation).  With d_final_obs and d_final_values a second pass of the vf net runs on final_obs, from
 *     d_state_in as it is (NOT masked by episode_starts); it stores no state; final_values[e] is NaN where
 *     final_obs[e][0] is NaN, as "policy".  (RecurrentPPO.collect_rollouts bootstraps a truncated step with
 *     predict_values(terminal_obs, lstm_states.vf) on the states the forward of that step returned; here
 *     V(final_observation) of step t - 1 comes from the call of step t, whose d_state_in are those states.)
 *  L7 Values-only call (d_values and / or d_final_values, no pi output, no d_state_out): sb3-contrib's
 *     predict_values(obs, lstm_states.vf, episode_starts): the vf net only, masked by episode_starts; no state is stored.
 *     d_state_out with no pi or vf output of the pass over obs is allowed and advances the state only.
 *  L8 Parameters: one float32 array, every matrix TRANSPOSED ([in][out] row-major: weight.T), per net, pi first:
 *     W_ih^T [D][4H], W_hh^T [H][4H], b_ih [4H], b_hh [4H], then what "policy" packs for that net with input width H.
 *     Both biases stay separate (state_dict() round-trips; a later update trains them as torch does).  Names:
 *     lstm_actor. / lstm_critic. weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0; mlp_extractor.policy_net.*,
 *     mlp_extractor.value_net.*, action_net.*, value_net.*.
 *  L9 Head, draws, NaN and +-inf logits: exactly as "policy".  Every NaN that is stored (the state included) is 0x7fc00000.
 *
 *   rf_lstm_params_size    floats of the packed parameters of desc; 0 for a desc outside the limits or a NULL ctx
 *   rf_lstm_state_size     floats of the state of n environments (4 n H); 0 if refused or n < 1
 *   rf_lstm_forward        one launch on caller_stream, nothing allocated, nothing waited for.  d_episode_starts and
 *                          d_state_in are needed; of d_state_out and the outputs of rf_policy_forward (each may be NULL)
 *                          at least one must be given.  Refusals as rf_policy_forward's, all before anything is enqueued;
 *                          also lstm_hidden outside its limits and a d_state_out that overlaps d_state_in without being it. */
typedef struct rf_lstm_policy_desc {
    rf_policy_desc policy; /* obs_width is the LSTMs' input width; the MLPs' input width is lstm_hidden */
    int lstm_hidden;       /* 1 .. RF_POLICY_MAX_WIDTH */
} rf_lstm_policy_desc;

unsigned long long rf_lstm_params_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc);
unsigned long long rf_lstm_state_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc, int n);
int rf_lstm_forward(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const float *d_params, int n, const float *d_obs,
                    const uint8_t *d_episode_starts, const float *d_final_obs, const float *d_state_in, float *d_state_out,
                    const unsigned long long gen[4], int flags, long long *d_actions, float *d_log_probs, float *d_values,
                    float *d_final_values, float *d_logits, void *caller_stream);

/* ---- lstm update: one recurrent PPO minibatch update on the device: sequences, BPTT, clip, Adam ------------------------
 * The other half of training in the reference's recurrent configurations (examples/ppo_lstm_*.yml) is sb3-contrib's
 * RecurrentPPO.train(): per minibatch the loss of "ppo update" on the actor-critic of "lstm policy", its gradient by
 * back-propagation through the MLPs and through time, clip_grad_norm_ and one Adam step.  No reference counterpart.  Needs
 * no environment: the context only says which GPU.  Categorical head only; one LSTM layer per net.
 *
 * One definition, numpy twin (environments/lstm_learner.py lstm_update_numpy), host build (tests/lstmppocheck) and kernels
 * (csrc/rf_lstm_ppo.h) alike.  Everything is float32, left to right, one rounding per operation, nothing contracted,
 * unless a step says float64; no MFMA; every reduction has a fixed order.
 *
 * Inputs.  A rollout of T = n_steps steps of n = num_envs environments, N = n * T: the five arrays of flat() (observations
 * float32[N][D], actions int64[N], log_probs, advantages, returns float32[N]; row r = e * T + t) and the rollout's two
 * recurrent slabs in their own layout, episode_starts uint8[T + 1][n] and lstm_states float32[T + 1][2 nets][2: h, c][n][H].
 *  U1 Minibatch.  sb3-contrib never permutes rows, it rotates them: the minibatch is B consecutive rows of flat()'s order
 *     starting at `first` and wrapping, r_b = (first + b) mod N, 1 <= B <= min(N, RF_PPO_MAX_BATCH), 0 <= first < N (host
 *     integers: what is outside is refused on the host).  e = r_b / T, t = r_b mod T.
 *  U2 Sequences.  Row b starts a sequence iff b == 0, or t == 0 (the environment changes), or episode_starts[t][e] != 0.
 *     The state that enters a sequence starting at (t, e) is lstm_states[t][net][h | c][e][:], or +0 where
 *     episode_starts[t][e] != 0 -- a select, as L4: a NaN of a dead state never enters.  It is a constant: no gradient
 *     flows into it.  Every other row takes h' and c' of row b - 1.
 *  U3 Validity.  invalid = some actions[r_b] outside [0, A); a = clamp(actions[r_b], 0, A - 1).
 *  U4 Forward.  Per row and net the cell of L2 on observations[r_b] from (h, c) of U2, which gives the gate values i, f, g,
 *     o, c' and h'; then the net's MLP and head on h' as "ppo update" step 3.
 *  U5 Advantages, loss terms and head deltas: "ppo update" steps 2, 4 and 5, over the B rows in minibatch order.
 *  U6 Backward through the MLPs: "ppo update" step 6, and one more product through the first MLP matrix W0^T [H][out]:
 *     dh_mlp[b][k] = sum over o in index order, from +0, of W0^T[k][o] * delta0[b][o] (the LSTM's output has no activation
 *     derivative: no further multiply).
 *  U7 BPTT.  Within each sequence, from its last row to its first, per net and unit j, with dh_rec = dc_next = +0 at the
 *     sequence's last row (both additions are still performed):
 *       dh = dh_mlp[b][j] + dh_rec[j];  tc = tanh32(c');  do = dh * tc;  dc = (dh * o) * (1 - tc * tc) + dc_next;
 *       da_i = (dc * g) * (i * (1 - i));  da_f = (dc * c_prev) * (f * (1 - f));  da_g = (dc * i) * (1 - g * g);
 *       da_o = do * (o * (1 - o));  dc_next of the row before = dc * f;
 *       dh_rec[k] of the row before: four chains, one per gate q, over j = 0 .. H-1 ascending from +0,
 *       acc_q = acc_q + W_hh^T[k][q * H + j] * da_q[j], joined as (acc_i + acc_f) + (acc_g + acc_o).
 *     c_prev of a sequence's first row is its entering c.
 *  U8 Parameter gradients, each one chain over b = 0 .. B-1 ascending from +0 (a multiply, then an add):
 *     dW_ih^T[k][col] of x[b][k] * da[b][col]; dW_hh^T[k][col] of h_prev[b][k] * da[b][col] (h_prev of a sequence's first row
 *     is its entering h); db_ih[col] = db_hh[col] of da[b][col]; the MLPs' as "ppo update" step 7 with h' as the first
 *     layer's input.  Packing: L8.  A NaN gradient is stored as 0x7fc00000.
 *  U9 "ppo update" steps 8 to 10 over the P packed parameters of L8: the float64 tree-summed norm, the skip rule
 *     (RF_PPO_INVALID for U3, RF_PPO_NONFINITE for a norm that is not finite: parameters and optimizer state keep their
 *     bytes), clip, Adam, stats and flags.  The optimizer state is "ppo update"'s: 32 bytes of header, m[P], v[P].
 *
 *   rf_lstm_ppo_state_size      bytes of the optimizer state (32 + 8 P); 0 for a desc outside the limits or a NULL ctx
 *   rf_lstm_ppo_workspace_size  bytes of the workspace for minibatches up to max_batch (1 .. RF_PPO_MAX_BATCH); 0 if refused
 *   rf_lstm_ppo_update          six launches on caller_stream, nothing allocated, nothing waited for; d_params, d_state and
 *                               d_stats (float32[8]) are updated in place, d_workspace is scratch.  Refused (RF_ERR_INVALID,
 *                               nothing enqueued, no device pointer dereferenced): what rf_ppo_update and rf_lstm_forward
 *                               refuse (a desc or lstm_hidden outside the limits, n_steps or num_envs < 1, a hyper-parameter,
 *                               a NULL array, one the runtime does not vouch for on the ctx's GPU -- the two slabs in their
 *                               [T + 1] lengths --, an output that overlaps an input or another output, a capturing caller
 *                               stream), and B or first outside the limits of U1. */
unsigned long long rf_lstm_ppo_state_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc);
unsigned long long rf_lstm_ppo_workspace_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc, int max_batch);
int rf_lstm_ppo_update(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const rf_ppo_desc *ppo, float *d_params, void *d_state,
                       void *d_workspace, int n_steps, int num_envs, const float *d_observations, const long long *d_actions,
                       const float *d_log_probs, const float *d_advantages, const float *d_returns,
                       const uint8_t *d_episode_starts, const float *d_lstm_states, int first, int B, float *d_stats,
                       void *caller_stream);

/* ---- lstm sde policy: the Gaussian (gSDE) head on top of the recurrent actor-critic -----------------------------------------
 * The reference's last training configuration (examples/ppo_lstm_untuned.yml, ContinuousJumps-v0: policy 'MlpLstmPolicy'
 * with use_sde: True): sb3-contrib's RecurrentActorCriticPolicy(use_sde=True) for ONE action dimension, at the defaults
 * "lstm policy" and "sde policy" already fix -- one nn.LSTM layer per net, enable_critic_lstm=True, shared_lstm=False,
 * full_std=True, learn_features=False, use_expln=False, squash_output=False, epsilon = 1e-6.  The noise features are the
 * activations of the last pi MLP layer, AFTER the LSTM, so log_std and theta have L = the last pi width entries.  No
 * reference counterpart.  Written as deltas of the two sections it composes; numpy twin environments/lstm_sde.py, host
 * build tests/lstmsdecheck, kernel lstm_forward_kernel<true> (csrc/rf_lstm.h).
 *
 *  Forward.  L1 to L8 of "lstm policy" (cell, episode starts, state, V(final_observation), values-only call), with a pi head
 *     of one output (rf_policy_desc.n_actions must be 1) and, on h = the last pi activations, S4 (std2, var, sigma), S6
 *     (mu, raw and clamped action), S7 (log_prob) and S8 of "sde policy".
 *  Noise.  theta float32[n][L] is S5: draw e * L + k of `gen`, with log_std read from THIS policy's parameters.
 *  Packing.  L8 for both nets with n_actions == 1, then log_std[L] last of everything: P + L floats.  Names: L8's, and
 *     "log_std".
 * enable_critic_lstm=False is "lstm critic" below.  Still out of scope: more than one action dimension, n_lstm_layers > 1,
 * shared_lstm=True, lstm_hidden_size > RF_POLICY_MAX_WIDTH, learn_features=True, use_expln, squash_output.
 *
 *   rf_lstm_sde_params_size  floats of the packed parameters (P + L); 0 for a desc outside the limits or a NULL ctx
 *   rf_lstm_sde_noise_reset  one launch (rf_sde_noise_reset's kernel): d_theta float32[n][L] from gen and the log_std
 *                            inside d_params
 *   rf_lstm_sde_forward      one launch.  Inputs as rf_lstm_forward's, with d_theta in place of gen (needed unless flags has
 *                            RF_POLICY_DETERMINISTIC or no pi output is asked for); outputs as rf_sde_forward's, and
 *                            d_state_out (each may be NULL, one must be given).  Refusals as the two siblings', all before
 *                            anything is enqueued; an n_actions other than 1 is refused as well. */
unsigned long long rf_lstm_sde_params_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc);
int rf_lstm_sde_noise_reset(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const float *d_params, int n,
                            const unsigned long long gen[4], float *d_theta, void *caller_stream);
int rf_lstm_sde_forward(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const float *d_params, int n, const float *d_obs,
                        const uint8_t *d_episode_starts, const float *d_final_obs, const float *d_state_in,
                        float *d_state_out, const float *d_theta, int flags, float *d_actions, float *d_env_actions,
                        float *d_log_probs, float *d_values, float *d_final_values, float *d_mean, float *d_sigma,
                        void *caller_stream);

/* ---- lstm sde update: the recurrent PPO minibatch update with the Gaussian head ----------------------------------------------
 * U1 to U9 of "lstm update" with these steps of "sde policy" in place of U3 and of the Categorical parts of U4 to U6
 * (actions float32[N], the raw actions; numpy twin environments/lstm_learner.py, host build tests/lstmsdecheck, kernels
 * lstm_ppo_mlp_kernel<true> and lstm_ppo_gradient_kernel<true> of csrc/rf_lstm_ppo.h; the other four launches are "lstm
 * update"'s, unchanged):
 *  1' Validity.  invalid = some actions[r_b] NaN.
 *  3' Forward.  mu = the pi head on the last pi activations h of row b; sigma as S4; logp and H_b as S7.
 *  5' Head gradients dmu_b, dsig_b as "sde policy".  A row whose sigma or logp is not finite has both NaN: the update ends
 *     in RF_PPO_NONFINITE and parameters and optimizer state keep their bytes.
 *  6' Backward.  The pi MLP, and through it dh_mlp and the pi LSTM (U6, U7), get their gradient through mu only (delta of
 *     the head = dmu_b); h is a constant inside var.
 *  7' dlog_std_k = sum over b = 0 .. B-1 in minibatch order, from +0, of ((h[b][k] * h[b][k]) * std2_k) * dsig_b: log_std
 *     gets its gradient through sigma only.
 * U8's packing and U9 run over the P + L floats of "lstm sde policy"; the optimizer state is 32 + 8 (P + L) bytes.
 *
 *   rf_lstm_sde_state_size, rf_lstm_sde_workspace_size, rf_lstm_sde_update
 *                            as their rf_lstm_ppo_ siblings, over P + L parameters and float32 actions; six launches; the
 *                            same refusals, and an n_actions other than 1. */
unsigned long long rf_lstm_sde_state_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc);
unsigned long long rf_lstm_sde_workspace_size(rf_ctx *ctx, const rf_lstm_policy_desc *desc, int max_batch);
int rf_lstm_sde_update(rf_ctx *ctx, const rf_lstm_policy_desc *desc, const rf_ppo_desc *ppo, float *d_params, void *d_state,
                       void *d_workspace, int n_steps, int num_envs, const float *d_observations, const float *d_actions,
                       const float *d_log_probs, const float *d_advantages, const float *d_returns,
                       const uint8_t *d_episode_starts, const float *d_lstm_states, int first, int B, float *d_stats,
                       void *caller_stream);

/* ---- lstm critic: the recurrent actor-critic with a feed-forward critic (enable_critic_lstm=False) --------------------------
 * sb3-contrib's RecurrentActorCriticPolicy(enable_critic_lstm=False, shared_lstm=False), which rl_zoo3's sampler for
 * RecurrentPPO draws in half of its trials: the policy has no lstm_critic but critic = nn.Linear(features_dim,
 * lstm_hidden_size); forward, evaluate_actions and predict_values compute latent_vf = critic(features) -- no activation, no
 * state, no episode-start mask -- and hand it to the vf MLP and value_net as before; the actor is unchanged; the returned
 * lstm_states.vf is a copy of lstm_states.pi.  No reference counterpart.  Written as deltas of "lstm policy" (L1 - L9), "lstm
 * update" (U1 - U9) and their two sde siblings; numpy twins environments/lstm.py, lstm_sde.py and lstm_learner.py (a spec
 * with enable_critic_lstm=False), host build tests/lstmcriticcheck, kernels lstm_forward_kernel<., true> (csrc/rf_lstm.h),
 * lstm_ppo_forward_kernel<true> and lstm_ppo_gradient_kernel<., true> (csrc/rf_lstm_ppo.h).  Everything is float32, a
 * multiply and then an add in index order, nothing contracted; no MFMA.
 *
 *  C1 Network.  The pi net is L1's.  The vf net is ONE linear layer D -> H, then the vf MLP (input width H) and its head,
 *     exactly as today.
 *  C2 Linear layer.  For unit j: a = bias[j]; for k = 0 .. D-1: a = a + x_k * W[j][k].  No activation: this a is the vf
 *     MLP's input ("policy"'s linear layer).
 *  C3 Starts and state.  episode_starts and the state have no influence on any value.  The state keeps its shape, float32
 *     [2][2][n][H]; a forward that stores a state writes the pi net's h' and c' into BOTH halves (sb3-contrib's
 *     lstm_states_vf = lstm_states_pi); nothing ever reads the vf half; a state updated in place stays legal.
 *  C4 V(final_observation) is the vf MLP on critic(final_obs), NaN where final_obs[e][0] is NaN (L6's rule).  A values-only
 *     call (L7) is the vf net on obs.  It reads neither d_state_in nor d_episode_starts; both pointers are still checked.
 *  C5 Packing.  The pi net as L8.  The vf net: critic.weight^T [D][H], critic.bias [H], then what "policy" packs for the vf
 *     MLP and head: P' = P - [4H (D + H) + 8H] + [D H + H] floats.  Names: critic.weight (torch shape [H, D]) and
 *     critic.bias in place of the four lstm_critic.* ones.  With the sde head log_std[L] stays last of everything.
 *  C6 Update, forward.  U2's sequences exist for the pi net only.  For the vf net row b's MLP input is C2 on
 *     observations[r_b].  The vf half of lstm_states is never read; episode_starts reaches the value path nowhere.
 *  C7 Update, backward.  U6 runs unchanged for both nets; for the vf net dh_mlp[b][j] is the delta of the linear layer's
 *     output.  U7 (BPTT) runs for the pi net only.  U8 gains dW^T[k][j], one chain over b = 0 .. B-1 ascending from +0 of
 *     x[b][k] * dh_mlp_vf[b][j], and dbias[j], the same chain of dh_mlp_vf[b][j].  Every other piece is as today.
 *  C8 Norm, skip, clip, Adam.  U9 over the P' packed floats of C5 (P' + L with sde); the optimizer state is 32 + 8 P' bytes
 *     (32 + 8 (P' + L)).  The workspace has no h_prev, c_prev, gates, c' or da of the vf net: it is smaller than the LSTM
 *     critic's at the same batch.
 *  Gaussian head.  Steps 1', 3', 5', 6' and 7' of "lstm sde update" and the noise of "lstm sde policy" apply unchanged: they
 *     touch only the pi net.
 * Still out of scope: shared_lstm=True (critic values other than the two below are refused, which leaves room for it),
 * n_lstm_layers > 1, lstm_hidden_size > RF_POLICY_MAX_WIDTH.
 *
 * Every entry point below is its rf_lstm_ sibling over rf_lstm_critic_desc: with critic == RF_LSTM_CRITIC_LSTM it IS the
 * sibling (the same launches, the same bytes); with RF_LSTM_CRITIC_LINEAR it computes the definition above, a forward in
 * one launch, an update in six.  The same arguments, the same refusals, all before anything is enqueued; any other critic
 * is refused as a desc outside the limits.  (rf_lstm_state_size needs no sibling: the state keeps its shape.) */
#define RF_LSTM_CRITIC_LSTM 0
#define RF_LSTM_CRITIC_LINEAR 1

typedef struct rf_lstm_critic_desc {
    rf_lstm_policy_desc lstm;
    int critic; /* RF_LSTM_CRITIC_LSTM or RF_LSTM_CRITIC_LINEAR */
} rf_lstm_critic_desc;

unsigned long long rf_lstm_critic_params_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc);
int rf_lstm_critic_forward(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const float *d_params, int n, const float *d_obs,
                           const uint8_t *d_episode_starts, const float *d_final_obs, const float *d_state_in,
                           float *d_state_out, const unsigned long long gen[4], int flags, long long *d_actions,
                           float *d_log_probs, float *d_values, float *d_final_values, float *d_logits, void *caller_stream);
unsigned long long rf_lstm_critic_ppo_state_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc);
unsigned long long rf_lstm_critic_ppo_workspace_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int max_batch);
int rf_lstm_critic_ppo_update(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const rf_ppo_desc *ppo, float *d_params,
                              void *d_state, void *d_workspace, int n_steps, int num_envs, const float *d_observations,
                              const long long *d_actions, const float *d_log_probs, const float *d_advantages,
                              const float *d_returns, const uint8_t *d_episode_starts, const float *d_lstm_states, int first,
                              int B, float *d_stats, void *caller_stream);
unsigned long long rf_lstm_critic_sde_params_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc);
int rf_lstm_critic_sde_noise_reset(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const float *d_params, int n,
                                   const unsigned long long gen[4], float *d_theta, void *caller_stream);
int rf_lstm_critic_sde_forward(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const float *d_params, int n, const float *d_obs,
                               const uint8_t *d_episode_starts, const float *d_final_obs, const float *d_state_in,
                               float *d_state_out, const float *d_theta, int flags, float *d_actions, float *d_env_actions,
                               float *d_log_probs, float *d_values, float *d_final_values, float *d_mean, float *d_sigma,
                               void *caller_stream);
unsigned long long rf_lstm_critic_sde_state_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc);
unsigned long long rf_lstm_critic_sde_workspace_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int max_batch);
int rf_lstm_critic_sde_update(rf_ctx *ctx, const rf_lstm_critic_desc *desc, const rf_ppo_desc *ppo, float *d_params,
                              void *d_state, void *d_workspace, int n_steps, int num_envs, const float *d_observations,
                              const float *d_actions, const float *d_log_probs, const float *d_advantages,
                              const float *d_returns, const uint8_t *d_episode_starts, const float *d_lstm_states, int first,
                              int B, float *d_stats, void *caller_stream);

/* ---- population: G independent PPO learners in lock-step, one launch per stage --------------------------------------------
 * The reference trains with n_envs 8 and runs its hyper-parameter search as 20 such trials side by side; at 8 environments
 * a forward is one or two blocks and an update three launch-bound kernels.  A population is G learners of ONE architecture
 * (the Categorical head of "policy") over one environment of n = G m lanes, each stage of all of them one launch.  No
 * reference counterpart.  Written as deltas of "policy" and "ppo update": the arithmetic of a group is exactly theirs, only
 * addressing changes.  numpy twins environments/population.py (G of the existing twins over slices), kernels
 * policy_forward_grouped_kernel (csrc/rf_policy.h) and ppo_backward_grouped_kernel, ppo_gradient_grouped_kernel,
 * ppo_adam_grouped_kernel (csrc/rf_ppo.h), each the ungrouped kernel's body behind a group dimension of the grid.
 *
 *  G1 Environments.  Group g of G owns environments [g m, (g + 1) m): rows [g m, (g + 1) m) of every array of a forward.
 *     Tiles of 8 rows are cut per group (a tile never spans two groups; no result depends on it).
 *  G2 Parameters.  d_params is float32 [G][P]: group g reads and updates params[g P .. (g + 1) P).
 *  G3 Draws.  d_gens is uint64 [G][4], the words of G generators as rf_policy_forward's gen; `consumed` travels by value.
 *     Row e of group g (e local, 0 .. m - 1) takes draw number consumed + e of generator g: what a stand-alone
 *     rf_policy_forward over the group's m rows takes whose generator was advanced by `consumed` before.  The caller adds m
 *     to consumed after a sampled call; the table is written at seeding only.
 *  G4 Update rows.  The arrays of an update have G N rows, group g owning rows [g N, (g + 1) N) -- with N = m T these are
 *     the group's rows of a rollout's flat(), which orders rows e T + t.  d_index is int64 [G][B] of rows LOCAL to the
 *     group, each in [0, N); validity, clamping and the gathers of steps 1 .. 3 are per group with the group's N.
 *     1 <= B <= min(N, RF_PPO_MAX_BATCH).
 *  G5 Hyper-parameters.  d_hyper is a device array of G rf_ppo_hyper, what rf_ppo_desc becomes: the float64 fields
 *     unchanged, clip_range, ent_coef and vf_coef converted to float32.  They are read on the device, so the entry point
 *     cannot check them: the caller vouches that each is what rf_ppo_update would accept.
 *  G6 State and workspace.  d_state is G optimizer states of "ppo update" back to back (32 + 8 P bytes each), the workspace
 *     G workspaces of rf_ppo_workspace_size(B) bytes each: the float64 trees of steps 2, 8 and 10 are per group and have
 *     the shape of the ungrouped tree for the same B and P.
 *  G7 Stats and skips.  d_stats is float32 [G][8].  A group whose minibatch is invalid or whose gradient norm is not finite
 *     is skipped and flagged in its own stats[7] exactly as step 8 says; the other groups are untouched by it.
 * Limits: G 1 .. RF_POPULATION_MAX_GROUPS (the grid's y / z limit), m >= 1, G m <= 2^30 (G N alike), B as in G4.
 * A normaliser and GAE discounts per group: "population view", above.  The Gaussian head: "population sde", below.  Out of
 * scope: groups that differ in architecture, m, T or B.  The recurrent head: "population lstm", below, and with the
 * Gaussian head "population lstm sde", at the end.
 *
 *   rf_policy_forward_grouped      rf_policy_forward over (G, m) in place of n: one launch, grid (ceil(m / 8), nets, G);
 *                                  the same outputs over G m rows, the same refusals (with d_gens, a device array, in
 *                                  place of gen, needed when the call samples), and G or m outside the limits.
 *   rf_ppo_grouped_state_size      G (32 + 8 P) bytes; 0 for a desc outside the limits, G outside its limits, m < 1 or a
 *                                  NULL ctx
 *   rf_ppo_grouped_workspace_size  G rf_ppo_workspace_size(policy, B) bytes; 0 if that is, for G < 1, m < 1, T < 1 or
 *                                  B > m T
 *   rf_ppo_update_grouped          rf_ppo_update over (G, m, T) in place of N, N = m T rows per group: three launches
 *                                  whatever G is, the same refusals over the G-fold arrays, and B > N. */
#define RF_POPULATION_MAX_GROUPS 65535

typedef struct rf_ppo_hyper {
    double learning_rate, max_grad_norm, beta1, beta2, adam_eps;
    float clip_range, ent_coef, vf_coef;
    int normalize_advantage; /* 0 / 1 */
} rf_ppo_hyper;               /* 56 bytes */

int rf_policy_forward_grouped(rf_ctx *ctx, const rf_policy_desc *desc, int G, int m, const float *d_params,
                              const float *d_obs, const float *d_final_obs, const unsigned long long *d_gens,
                              unsigned long long consumed, int flags, long long *d_actions, float *d_log_probs,
                              float *d_values, float *d_final_values, float *d_logits, void *caller_stream);
unsigned long long rf_ppo_grouped_state_size(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m);
unsigned long long rf_ppo_grouped_workspace_size(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m, int T, int B);
int rf_ppo_update_grouped(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m, int T, const rf_ppo_hyper *d_hyper,
                          float *d_params, void *d_state, void *d_workspace, const float *d_obs, const long long *d_actions,
                          const float *d_old_log_probs, const float *d_advantages, const float *d_returns, int B,
                          const long long *d_index, float *d_stats, void *caller_stream);

/* ---- population sde: a population of gSDE learners, each group with its own log_std and noise schedule -------------------
 * The reference's hyper-parameter search draws a sde_sample_freq and a log_std_init per trial for ContinuousJumps-v0
 * (use_sde).  Written as deltas of "population" and "sde policy": the arithmetic of a group is exactly that of "sde policy"
 * and its update (steps 1', 3', 5', 6', 7'); only addressing changes.  numpy twins environments/population.py (G of
 * sde.SdePolicy / learner.Learner over slices), kernels sde_noise_kernel<true>, sde_forward_kernel<true> (csrc/rf_sde.h),
 * ppo_backward_kernel<true, true>, ppo_gradient_kernel<true>, ppo_adam_kernel<true> (csrc/rf_ppo.h).
 *
 *  S1 G1, G4, G5, G6 and G7 of "population" hold unchanged, with P + L parameters (rf_sde_params_size) in place of P:
 *     d_params is float32 [G][P + L], group g's log_std its last L floats; d_actions of an update are the raw actions,
 *     float32 [G N].
 *  S2 Noise.  d_theta is float32 [G m][L]; d_gens is uint64 [G][4] as in G3, d_consumed uint64 [G], the draws each
 *     generator has given, read on the device and never written.  theta[(g m + e) L + k] = the theta of "sde policy" from
 *     draw number consumed[g] + e L + k (64-bit) of generator g and log_std_k of group g: what a stand-alone
 *     rf_sde_noise_reset over the group's m rows gives whose generator was advanced by consumed[g] before.  d_select is
 *     uint8 [G] or NULL: a group whose byte is 0 writes nothing, its rows of theta keep their bytes; NULL selects every
 *     group.  The caller adds m L to consumed[g] of every selected group after the call.
 *  S3 Forward.  Group g's rows are computed from params[g] (its own log_std in sigma) and its own rows of theta.
 * Limits: G 1 .. RF_POPULATION_MAX_GROUPS, m 1 .. 2^20 (an update: m >= 1), G m <= 2^30 (G m T alike),
 * 1 <= B <= min(m T, RF_PPO_MAX_BATCH), n_actions 1.  The Gaussian head on the LSTM: "population lstm sde", at the end.
 * Out of scope: more than one action dimension.
 *
 *   rf_sde_noise_reset_grouped     rf_sde_noise_reset over (G, m) in place of n: one launch, grid (ceil(m L / 256), G); the
 *                                  same refusals (with d_gens, a device array, in place of gen), d_consumed or d_select no
 *                                  device array of G elements, d_theta overlapping an input, and G or m outside the limits.
 *   rf_sde_forward_grouped         rf_sde_forward over (G, m) in place of n: one launch, grid (ceil(m / 8), nets, G); the
 *                                  same outputs over G m rows, the same refusals, and G or m outside the limits.
 *   rf_sde_grouped_state_size      G (32 + 8 (P + L)) bytes; 0 where rf_ppo_grouped_state_size is, over the sde limits
 *   rf_sde_grouped_workspace_size  G rf_sde_workspace_size(policy, B) bytes; 0 where rf_ppo_grouped_workspace_size is
 *   rf_sde_update_grouped          rf_sde_update over (G, m, T) in place of N, N = m T rows per group: three launches
 *                                  whatever G is, the refusals of rf_ppo_update_grouped (a capturing caller stream among
 *                                  them) with the sde limits of the desc.
 * A refused call enqueues nothing and dereferences no device pointer.
 * (The tag between return type and name marks the section a declaration belongs to: tests/test_sde_logic.py takes a census
 * of the six entry points of "sde policy" by their plain declarations, and these five are not among them.) */
int /* population sde */ rf_sde_noise_reset_grouped(rf_ctx *ctx, const rf_policy_desc *desc, int G, int m,
        const float *d_params, const unsigned long long *d_gens /* [G][4] */, const unsigned long long *d_consumed /* [G] */,
        const unsigned char *d_select /* [G] or NULL */, float *d_theta /* [G m][L] */, void *caller_stream);
int /* population sde */ rf_sde_forward_grouped(rf_ctx *ctx, const rf_policy_desc *desc, int G, int m, const float *d_params,
        const float *d_obs, const float *d_final_obs, const float *d_theta, int flags, float *d_actions,
        float *d_env_actions, float *d_log_probs, float *d_values, float *d_final_values, float *d_mean, float *d_sigma,
        void *caller_stream);
unsigned long long /* population sde */ rf_sde_grouped_state_size(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m);
unsigned long long /* population sde */ rf_sde_grouped_workspace_size(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m,
        int T, int B);
int /* population sde */ rf_sde_update_grouped(rf_ctx *ctx, const rf_policy_desc *policy, int G, int m, int T,
        const rf_ppo_hyper *d_hyper, float *d_params, void *d_state, void *d_workspace, const float *d_obs,
        const float *d_actions, const float *d_old_log_probs, const float *d_advantages, const float *d_returns, int B,
        const long long *d_index, float *d_stats, void *caller_stream);

/* ---- population lstm: a population of recurrent PPO learners (the Categorical head on the LSTM, either critic) -------------
 * The reference's hyper-parameter search has a ppo_lstm sampler next to ppo, 20 trials side by side with n_envs 8, and two
 * of its four training configurations are recurrent.  Written as deltas of "population", "lstm policy", "lstm update" and
 * "lstm critic": the arithmetic of a group is exactly that of rf_lstm_forward / rf_lstm_ppo_update (rf_lstm_critic_forward /
 * rf_lstm_critic_ppo_update with desc->critic == RF_LSTM_CRITIC_LINEAR); only addressing changes.  numpy twins
 * environments/population.py (G of lstm.LstmPolicy / lstm_learner.LstmLearner over slices), kernels
 * lstm_forward_kernel<false, kLinear, true> (csrc/rf_lstm.h), lstm_ppo_forward_kernel<kLinear, true>,
 * lstm_ppo_mlp_kernel<false, true>, lstm_ppo_bptt_kernel<true>, lstm_ppo_gradient_kernel<false, kLinear, true>,
 * lstm_ppo_norm_kernel<true> (csrc/rf_lstm_ppo.h) and ppo_adam_kernel<true> (csrc/rf_ppo.h).
 *
 *  L1 G1, G2, G3, G5, G6 and G7 of "population" hold unchanged, with the P of rf_lstm_params_size /
 *     rf_lstm_critic_params_size and the workspace of rf_lstm_ppo_workspace_size / rf_lstm_critic_ppo_workspace_size;
 *     d_episode_starts of a forward is uint8 [G m], group g's rows [g m, (g + 1) m).
 *  L2 State.  The state keeps its single form float32 [2][2][n][H] with n = G m: group g owns rows [g m, (g + 1) m) of EACH
 *     of the four [n][H] planes -- its rows are not one contiguous piece.  Element (net, which, e, unit) of group g is
 *     ((net * 2 + which) * n + g m + e) * H + unit.  d_state_out is NULL, d_state_in itself (in place) or a range that
 *     does not overlap it.  With the linear critic the pi block stores both halves, as "lstm critic" says.
 *  L3 Update rows.  The five arrays of flat() have G N rows, N = m T, group g owning rows [g N, (g + 1) N) (G4).
 *     d_episode_starts is uint8 [T + 1][n] and d_lstm_states float32 [T + 1][2][2][n][H] in their single form: environment e
 *     of group g is column g m + e, the row stride of episode_starts is n and the plane stride of lstm_states n H.
 *  L4 First rows.  d_firsts is int32 [G] on the device: group g's minibatch is rows (firsts[g] + b) mod N, b < B, LOCAL to
 *     the group -- they wrap inside the group, and the sequence rule of "lstm update" runs over (T, m) with the group's
 *     columns.  B is one value for all groups.  The host cannot check firsts[g]: the kernels clamp it into 0 .. N - 1, and a
 *     value outside sets the group's validity flag, so the group is skipped with RF_PPO_INVALID in its stats[7] exactly as
 *     an invalid index is in rf_ppo_update_grouped; the other groups are untouched by it.
 * Limits: G 1 .. RF_POPULATION_MAX_GROUPS, m >= 1, T >= 1, G m <= 2^30 (G m T alike), 1 <= B <= min(m T,
 * RF_PPO_MAX_BATCH); the desc as "lstm policy" / "lstm critic".  The lstm-sde head in a population: "population lstm
 * sde", below.  Out of scope: groups that differ in architecture, critic, m, T or B.
 *
 *   rf_lstm_forward_grouped             rf_lstm_forward / rf_lstm_critic_forward over (G, m) in place of n: one launch, grid
 *                                       (ceil(m / 8), nets, G); the same outputs over G m rows, the same refusals (with
 *                                       d_gens, a device array, in place of gen, needed when the call samples), G or m
 *                                       outside the limits, and a capturing caller stream.
 *   rf_lstm_ppo_grouped_state_size      G (32 + 8 P) bytes; 0 for a desc outside the limits, G outside its limits, m < 1 or
 *                                       a NULL ctx
 *   rf_lstm_ppo_grouped_workspace_size  G times the ungrouped workspace of B; 0 if that is, for G outside its limits, m < 1,
 *                                       T < 1 or B > min(m T, RF_PPO_MAX_BATCH)
 *   rf_lstm_ppo_update_grouped          rf_lstm_ppo_update / rf_lstm_critic_ppo_update over (G, m, T): six launches whatever
 *                                       G is; the refusals of rf_lstm_ppo_update and rf_ppo_update_grouped over the G-fold
 *                                       arrays (a capturing caller stream and overlapping outputs among them), a NULL
 *                                       d_firsts.
 * A refused call returns RF_ERR_INVALID, enqueues nothing and dereferences no device pointer.
 * (The tag between return type and name: several tests take a census of the rf_lstm_ entry points by their plain
 * declarations, and these four are not among them.) */
int /* population lstm */ rf_lstm_forward_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m,
        const float *d_params, const float *d_obs, const uint8_t *d_episode_starts, const float *d_final_obs,
        const float *d_state_in, float *d_state_out, const unsigned long long *d_gens /* [G][4] */,
        unsigned long long consumed, int flags, long long *d_actions, float *d_log_probs, float *d_values,
        float *d_final_values, float *d_logits, void *caller_stream);
unsigned long long /* population lstm */ rf_lstm_ppo_grouped_state_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G,
        int m);
unsigned long long /* population lstm */ rf_lstm_ppo_grouped_workspace_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc,
        int G, int m, int T, int B);
int /* population lstm */ rf_lstm_ppo_update_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m, int T,
        const rf_ppo_hyper *d_hyper, float *d_params, void *d_state, void *d_workspace, const float *d_observations,
        const long long *d_actions, const float *d_log_probs, const float *d_advantages, const float *d_returns,
        const uint8_t *d_episode_starts, const float *d_lstm_states, const int *d_firsts /* [G] */, int B,
        float *d_stats, void *caller_stream);

/* ---- population lstm sde: a population of recurrent gSDE learners (the Gaussian head on the LSTM, either critic) -----------
 * The reference trains ContinuousJumps-v0 with the recurrent policy and use_sde (examples/ppo_lstm_untuned.yml), and its
 * ppo_lstm search draws a log_std_init and a sde_sample_freq per trial.  Written as deltas of "population sde" (S1 - S3) and
 * "population lstm" (L1 - L4): the arithmetic of a group is exactly that of "lstm sde policy" / "lstm sde update" with
 * either critic kind of "lstm critic"; only addressing changes.  numpy twins environments/population.py (G of
 * lstm_sde.LstmSdePolicy / lstm_learner.LstmLearner over slices), kernels sde_noise_kernel<true> (csrc/rf_sde.h),
 * lstm_forward_kernel<true, kLinear, true> (csrc/rf_lstm.h), lstm_ppo_forward_kernel<kLinear, true>,
 * lstm_ppo_mlp_kernel<true, true>, lstm_ppo_bptt_kernel<true>, lstm_ppo_gradient_kernel<true, kLinear, true>,
 * lstm_ppo_norm_kernel<true> (csrc/rf_lstm_ppo.h) and ppo_adam_kernel<true> (csrc/rf_ppo.h).
 *
 *  S1' S1 with the P + L of rf_lstm_critic_sde_params_size: d_params is float32 [G][P + L], group g's log_std the last L
 *      floats of its own piece; d_actions of an update are the raw actions, float32 [G N].
 *  S2' S2 unchanged: theta[(g m + e) L + k] is what a stand-alone rf_lstm_critic_sde_noise_reset over the group's m rows
 *      gives whose generator was advanced by consumed[g] before; log_std_k is read at params + g (P + L) + P.
 *  S3' S3 over the recurrent forward: group g's rows are computed from params[g] and its own rows of theta, d_env_actions
 *      and d_sigma.  Nothing is drawn in a forward (the noise is theta): no generator travels, and a NULL d_theta or
 *      RF_POLICY_DETERMINISTIC gives the mean.  Each pi output may be asked for by itself.
 *  L1' - L4' L1 (without G3: no generators in a forward), L2, L3 and L4 hold unchanged, with the workspace of
 *      rf_lstm_critic_sde_workspace_size.  The validity rule of a group's minibatch is the Gaussian head's (a NaN raw
 *      action), OR-ed with L4's flag of a first row outside the group.
 * Limits: G 1 .. RF_POPULATION_MAX_GROUPS, m 1 .. 2^20 (an update: m >= 1), T >= 1, G m <= 2^30 (G m T alike),
 * 1 <= B <= min(m T, RF_PPO_MAX_BATCH); the desc as "lstm sde policy" / "lstm critic".  Out of scope: groups that differ in
 * architecture, critic, m, T or B; more than one action dimension.
 *
 *   rf_lstm_sde_noise_reset_grouped     rf_lstm_critic_sde_noise_reset over (G, m) in place of n: one launch, grid
 *                                       (ceil(m L / 256), G); the refusals of rf_sde_noise_reset_grouped with the lstm-sde
 *                                       limits of the desc.
 *   rf_lstm_sde_forward_grouped         rf_lstm_critic_sde_forward over (G, m) in place of n: one launch, grid (ceil(m / 8),
 *                                       nets, G); the same outputs over G m rows, the same refusals, G or m outside the
 *                                       limits, and a capturing caller stream.
 *   rf_lstm_sde_grouped_state_size      G (32 + 8 (P + L)) bytes; 0 where rf_lstm_ppo_grouped_state_size is, over the
 *                                       lstm-sde limits
 *   rf_lstm_sde_grouped_workspace_size  G times the ungrouped lstm-sde workspace of B; 0 where
 *                                       rf_lstm_ppo_grouped_workspace_size is
 *   rf_lstm_sde_update_grouped          rf_lstm_critic_sde_update over (G, m, T): six launches whatever G is; the refusals of
 *                                       rf_lstm_ppo_update_grouped with the lstm-sde limits of the desc.
 * A refused call returns RF_ERR_INVALID, enqueues nothing and dereferences no device pointer.
 * (The tag between return type and name: tests/test_lstm_sde_logic.py and tests/test_sde_logic.py take a census of the plain
 * rf_lstm_sde_ / rf_sde_ declarations, and these five are not among them.) */
int /* population lstm sde */ rf_lstm_sde_noise_reset_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m,
        const float *d_params, const unsigned long long *d_gens /* [G][4] */, const unsigned long long *d_consumed /* [G] */,
        const unsigned char *d_select /* [G] or NULL */, float *d_theta /* [G m][L] */, void *caller_stream);
int /* population lstm sde */ rf_lstm_sde_forward_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m,
        const float *d_params, const float *d_obs, const uint8_t *d_episode_starts, const float *d_final_obs,
        const float *d_state_in, float *d_state_out, const float *d_theta, int flags, float *d_actions,
        float *d_env_actions, float *d_log_probs, float *d_values, float *d_final_values, float *d_mean, float *d_sigma,
        void *caller_stream);
unsigned long long /* population lstm sde */ rf_lstm_sde_grouped_state_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc,
        int G, int m);
unsigned long long /* population lstm sde */ rf_lstm_sde_grouped_workspace_size(rf_ctx *ctx, const rf_lstm_critic_desc *desc,
        int G, int m, int T, int B);
int /* population lstm sde */ rf_lstm_sde_update_grouped(rf_ctx *ctx, const rf_lstm_critic_desc *desc, int G, int m, int T,
        const rf_ppo_hyper *d_hyper, float *d_params, void *d_state, void *d_workspace, const float *d_observations,
        const float *d_actions /* float32 raw */, const float *d_log_probs, const float *d_advantages,
        const float *d_returns, const uint8_t *d_episode_starts, const float *d_lstm_states,
        const int *d_firsts /* [G] */, int B, float *d_stats, void *caller_stream);

/* ---- parameter init: the packed parameters of G learners initialised on the device, as SB3 does ------------------------------
 * Every policy class starts with its parameters at zero, from which no net learns anything but its head biases: hidden
 * activations are 0, so every head weight's gradient is 0, so every delta handed back is 0.  The reference's tuned
 * configurations and every trial of its search use ortho_init=False (PyTorch's default initialisation); its untuned ones
 * leave SB3's ortho_init=True (orthogonal MLPs and heads with gains sqrt 2 / 0.01 / 1 and zero biases; the LSTMs and the
 * linear critic keep PyTorch's default).  Head-agnostic: the caller describes ONE group's packed array of `stride` floats
 * as at most RF_PARAM_MAX_SEGMENTS segments; what a segment means to a network is the caller's business
 * (environments/param_init.py builds the tables of the five specs).  numpy twin environments/param_init.py init_numpy,
 * kernels param_fill_kernel and param_orthogonal_kernel (csrc/rf_param_init.h), host build tests/paraminitcheck.
 *
 *  I1 Segments.  rf_param_segment {at, out, in, scheme, scale}: `at` the offset in floats, 1 <= out, in <=
 *     RF_POLICY_MAX_WIDTH; the segment covers the out * in floats from `at`.  Segments must not overlap and must lie inside
 *     the stride; they need not cover it, and a position outside every segment is not written.  A weight is packed as
 *     everywhere here, transposed: W^T[k][j] at at + k out + j, k < in, j < out.  A vector (a bias, log_std) has in = 1.
 *     Only RF_INIT_ORTHOGONAL reads out and in as a shape: the other schemes depend on the position alone, so for them a
 *     segment is a run of out * in floats however it is cut.  That is how the length of an LSTM's arrays is carried, whose
 *     4 H rows do not fit the width limit: W_ih^T [D][4H], W_hh^T [H][4H], b_ih and b_hh are packed one after the other
 *     and share one scale, so they are one run of 4 (D + H + 2) rows of H floats, passed as segments of out = H and
 *     in <= RF_POLICY_MAX_WIDTH rows each.  One draw per packed position either way (I2).
 *  I2 Draws.  Group g draws from numpy's Generator(PCG64DXSM(seed_g)), whose four words the caller passes (d_gens[g]: state
 *     low, state high, inc low, inc high).  Packed position i uses draw number i, u_i = the i-th random() after that state
 *     (the jump-ahead of "policy"), so no result depends on the launch shape; a position whose scheme needs no draw leaves
 *     its draw unused.
 *  I3 RF_INIT_ZERO: 0.0f.  RF_INIT_CONSTANT: d_constants[g], one float per group and call (log_std takes each group's
 *     log_std_init this way).
 *  I4 RF_INIT_UNIFORM: float32((2.0 * u_i - 1.0) * scale) in float64 -- one multiply, one subtract, one multiply, one
 *     rounding.  scale is computed once on the host as 1.0 / sqrt(float64(fan)), with PyTorch's fans: an nn.Linear(in, out)
 *     weight AND bias fan = in; every array of an nn.LSTM(D, H) fan = H; the linear critic nn.Linear(D, H) fan = D.
 *  I5 RF_INIT_ORTHOGONAL (scale = the gain): torch.nn.init.orthogonal_'s result -- the Q of the sign-fixed QR (positive
 *     diagonal of R, hence the same Haar distribution) -- by Gram-Schmidt in a fixed float64 order, rounded once.  t = max(out, in),
 *     s = min(out, in), A[a][b] = normal32(u_(at + a s + b)) for a < t, b < s (normal32 of "sde policy").  For b = 0 .. s - 1
 *     start from v[a] = float64(A[a][b]) and do the projection step TWICE (CGS2), every operation a float64 one: for every p < b, c_p = the sum over a ascending,
 *     from +0, of q_p[a] * v[a] (multiply, then add; every c_p from the same v); then for p ascending v[a] = v[a] -
 *     c_p * q_p[a].  After both passes n2 = the same chain over v[a] * v[a], and q_b[a] = v[a] / sqrt(n2), kept as float64; the column is
 *     all zeros where !(n2 > 0).  Packed result, with g = float32(scale) and q rounded to float32 (one float32 multiply):
 *        out >= in (t = out, orthonormal columns of W):  W^T[k][j] = g * q_k[j]   (vector k < in, component j < out)
 *        out <  in (t = in, orthonormal rows of W):      W^T[k][j] = g * q_j[k]   (vector j < out, component k < in)
 *     -- torch draws [out][in], transposes it where out < in, takes Q [t][s] and transposes back.  No FMA contraction; the
 *     float64 divide and sqrt are correctly rounded.
 *  I6 Groups.  d_params is float32 [G][stride]; the same table serves every group; d_select (uint8 [G] or NULL: every
 *     group) says which groups are written -- a group whose byte is 0 keeps every byte.  G = 1 is the ungrouped case.
 *     (Float32 chains, which an earlier draft of this definition had, are as good as LAPACK's float32 QR but miss the
 *     orthogonality of a float64 QR rounded once by a factor of 40 to 90 from 64 x 64 on: profiles/param_init.md.)
 *  I7 Workspace.  The orthogonal kernel keeps each finished vector as float64, twice, by vector and by component, so that
 *     both of its passes read consecutive doubles across threads; the destination is written once, at the end.
 *     rf_params_init_workspace_size: 16 G (the sum of out * in over the orthogonal segments) bytes; d_workspace is
 *     aligned to 8 bytes.
 * Deliberate differences from SB3: the project's generator and normal32 in place of torch's global RNG, CGS2 in
 * a fixed order in place of LAPACK's QR, one seed per group, draws indexed by position.
 * Limits: count 0 .. RF_PARAM_MAX_SEGMENTS, G 1 .. RF_POPULATION_MAX_GROUPS, stride 1 .. 2^30 and G stride <= 2^31.
 *
 *   rf_params_init_workspace_size  bytes of the workspace of rf_params_init (0 without orthogonal segments); 0 as well for a
 *                                  table rf_params_init refuses, G outside its limits or a NULL ctx
 *   rf_params_init                 two launches on caller_stream (one without orthogonal segments): param_fill_kernel, grid
 *                                  (ceil(stride / 256), G), then param_orthogonal_kernel, grid (orthogonal segments, G).
 *                                  Nothing is allocated, nothing waited for.  Refused with a message: more than
 *                                  RF_PARAM_MAX_SEGMENTS segments; out or in outside the limits; a segment out of range or
 *                                  overlapping another; an unknown scheme; a scale of a UNIFORM / ORTHOGONAL segment that is
 *                                  not finite and positive; a CONSTANT segment without d_constants; orthogonal segments
 *                                  without d_workspace; G or stride outside the limits; an array that is not device memory
 *                                  of the context's GPU, too small, misaligned or overlapping d_params; a capturing stream.
 * A refused call returns RF_ERR_INVALID, enqueues nothing and dereferences no device pointer. */
#define RF_PARAM_MAX_SEGMENTS 32
#define RF_INIT_ZERO 0
#define RF_INIT_CONSTANT 1
#define RF_INIT_UNIFORM 2
#define RF_INIT_ORTHOGONAL 3

typedef struct rf_param_segment {
    unsigned at;  /* offset in floats inside a group's piece */
    int out, in;  /* 1 .. RF_POLICY_MAX_WIDTH each; the segment covers out * in floats */
    int scheme;   /* RF_INIT_* */
    double scale; /* UNIFORM: 1 / sqrt(fan); ORTHOGONAL: the gain; unused otherwise */
} rf_param_segment;

unsigned long long rf_params_init_workspace_size(rf_ctx *ctx, const rf_param_segment *segments, int count, int groups);
int rf_params_init(rf_ctx *ctx, const rf_param_segment *segments, int count, int groups, unsigned stride, float *d_params,
        const unsigned long long *d_gens /* [G][4] */, const unsigned char *d_select /* [G] or NULL */,
        const float *d_constants /* [G] or NULL */, void *d_workspace, void *caller_stream);

/* ---- evaluation: per-group scores of a population on the device, the best parameters kept -----------------------------------
 * What the reference's hyper-parameter search optimises is each trial's evaluation score: stable-baselines3's
 * evaluate_policy on a separate evaluation environment -- deterministic actions, a frozen VecNormalize synced from the
 * training environment, raw rewards, a fixed number of episodes --, and the best model so far is kept.  This section is that
 * measurement for G groups of m lanes (n = G m; G = 1 is the ungrouped case) from the episode records a step writes
 * ("episode records": final_return float64 [n], final_length int32 [n], NaN / 0 where no episode ended).  numpy twin
 * environments/evaluation.py, kernels csrc/rf_eval.h, host build tests/evalcheck.
 *
 *  E1 Targets.  Group g owns lanes [g m, (g + 1) m).  The lane with local index i keeps its first target(i) = (E + i) / m
 *     episodes (integer division; SB3's episode_count_targets): the targets of a group sum to E.  K = ceil(E / m) is the slot
 *     count per lane.  Tables: counts int32 [n], returns float64 [n][K], lengths int32 [n][K]; the caller zeroes counts
 *     before a run, slots at or above a lane's count hold nothing.
 *  E2 Accumulation, per step and lane: if final_length > 0 and count < target then returns[lane][count] = final_return,
 *     lengths[lane][count] = final_length, count += 1.  A NaN return is a value and is kept with its bits; a lane at its
 *     target is ignored.
 *  E3 Positions.  The kept values of a group have fixed positions, lane-major and slot-minor: position(i, k) = the sum of
 *     target(j) over j < i, plus k.  Deliberately not SB3's order in time: the same set, summed in another order.
 *  E4 Sums.  treesum of "learner view" over the E positions: float64, padded with +0.0 to a power of two, adjacent pairs
 *     added until one value is left, that value + (+0.0).  No FMA contraction.
 *  E5 Result, float64 [G][8] per group: 0 mean return = treesum(x) / E; 1 population standard deviation =
 *     sqrt(treesum((x - mean)^2) / E), two passes as numpy.std; 2 minimum and 3 maximum return, NaN if any kept return is
 *     NaN, otherwise by the total order in which -0.0 is below +0.0; 4 mean length = treesum(lengths) / E; 5 episodes kept;
 *     6 flags; 7 the serial of this evaluation (the caller's number).  A NaN in columns 0 .. 4 is the quiet NaN
 *     0x7ff8000000000000 whatever sign the arithmetic gave it.  A group that has not reached all its targets gets
 *     RF_EVAL_INCOMPLETE in column 6, NaN in columns 0 .. 4 and its true count in column 5.
 *  E6 Best rule.  best_mean float64 [G] starts at -inf (the caller fills it), best_serial int64 [G].  A group improves iff it
 *     is complete and mean > best_mean[g] -- strict, so a tie and a NaN never improve --; then improved[g] = 1 and
 *     best_mean[g], best_serial[g] take the mean (as computed, before E5's canonical NaN, which it cannot be) and the serial;
 *     otherwise improved[g] = 0 and both stay.
 * Deliberate differences from SB3: E3 / E4 in place of numpy.mean over the time-ordered list; a fixed number of
 * steps in place of looping until every lane is done (the caller's bound; a group that is not done is flagged).
 * Limits: E 1 .. RF_EVAL_MAX_EPISODES, G 1 .. RF_POPULATION_MAX_GROUPS, m >= 1, n = G m, n K <= 2^31.
 *
 *   rf_eval_accumulate   E2: eval_accumulate_kernel, one thread per lane, no atomics.
 *   rf_eval_finish       E3 .. E6: eval_finish_kernel, one block of 256 threads per group; one thread writes the row.
 *   rf_eval_keep_rows    d_dst row g := d_src row g for the groups with d_select[g] != 0; rows of `words` 4-byte words,
 *                        `stride` words apart (1 <= words <= stride, G stride <= 2^31).  eval_keep_rows_kernel, grid
 *                        (ceil(words / 1024), G): 16-byte vectors with dword head and tail where d_src and d_dst are
 *                        congruent mod 16 bytes, dwords otherwise.  With `improved` as the selection it keeps the best
 *                        parameters and normaliser statistics; with a mask and the arrays exchanged it restores them.
 *   rf_env_view_get_statistics_device / rf_env_view_set_statistics_device
 *                        the running moments of the context's learner view to / from caller-owned device memory: float64
 *                        [G][3][W + 1] (mean, var, count; the returns last) of a grouped view, [3][W + 1] of an ungrouped
 *                        one.  One launch on the context's stream, ordered after what caller_stream holds, and caller_stream
 *                        waits for it: what sync_envs_normalization needs without crossing to the host.  The context must
 *                        be able to take device steps (rf_env_configure_initializer).
 * All five only enqueue on (or order against) caller_stream, allocate nothing and wait for nothing.  Every device array is
 * checked as the learner entry points' are (device memory of the context's GPU, aligned, large enough, outputs apart from
 * inputs and from each other); a capturing stream is refused.  A refused call returns RF_ERR_INVALID with a message,
 * enqueues nothing and dereferences no device pointer. */
#define RF_EVAL_MAX_EPISODES 65536
#define RF_EVAL_INCOMPLETE 1

int rf_eval_accumulate(rf_ctx *ctx, int n, int groups, int m, int episodes, const double *d_final_return,
        const int *d_final_length, int *d_counts, double *d_returns /* [n][K] */, int *d_lengths /* [n][K] */,
        void *caller_stream);
int rf_eval_finish(rf_ctx *ctx, int n, int groups, int m, int episodes, unsigned long long serial, const int *d_counts,
        const double *d_returns, const int *d_lengths, double *d_results /* [G][8] */, double *d_best_mean /* [G] */,
        long long *d_best_serial /* [G] */, unsigned char *d_improved /* [G] */, void *caller_stream);
int rf_eval_keep_rows(rf_ctx *ctx, int groups, unsigned words, unsigned stride, const unsigned char *d_select /* [G] */,
        const void *d_src, void *d_dst, void *caller_stream);
int rf_env_view_get_statistics_device(rf_ctx *ctx, double *d_out, void *caller_stream);
int rf_env_view_set_statistics_device(rf_ctx *ctx, const double *d_in, void *caller_stream);

#ifdef __cplusplus
}
#endif
#endif /* REINFOCUS_HIP_H */
