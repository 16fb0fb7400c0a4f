// rf_abi_snapshot.hip -- snapshots of a device-resident environment (include/reinfocus_hip.h: rf_env_snapshot*,
// rf_env_restore*): everything that decides what later steps, resets and renders compute, copied out of and back into the
// arrays the step works on.  Nothing here is compute: copies on the ctx's stream and nothing else, no kernel.  A restore
// writes in place, so an instantiated step graph -- which holds those arrays' addresses -- stays valid.
#include "rf_host.h"

#include <stddef.h>
#include <string.h>

using namespace rfh;

static_assert(sizeof(rf_env_snapshot_header) == 256, "the blob's first array starts at byte 256");

namespace {

constexpr size_t kAlign = 256;

uint64_t fnv1a(uint64_t h, const void *data, size_t bytes)
{
    const unsigned char *p = (const unsigned char *)data;
    for (size_t i = 0; i < bytes; ++i)
        h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;

// One array of a snapshot: where it lives on the device and where in the blob.
struct Piece {
    void *dev;
    size_t bytes, offset;
};

// The arrays of the configured context in the blob's order (the header's comment in include/reinfocus_hip.h), arrays
// of zero length left out; the blob's size.
struct Layout {
    std::vector<Piece> pieces;
    size_t total = sizeof(rf_env_snapshot_header);
    void add(void *dev, size_t bytes)
    {
        if (bytes == 0)
            return;
        pieces.push_back(Piece{dev, bytes, total});
        total += (bytes + kAlign - 1) & ~(kAlign - 1);
    }
    explicit Layout(const rf_ctx *ctx)
    {
        const rf::EnvState &s = ctx->env;
        const size_t n = (size_t)ctx->env_host.n;
        add(s.state, n * 8);
        add(s.steps, n * 4);
        add(s.diverging, n * 4);
        add(s.last_diff, n * 4);
        add(s.old_wrapped, n * 8);
        add(s.old_focus, n * 4);
        add(s.cam_dyn, n * 36);
        add(s.rect, n * 8);
        add(s.cam_dyn2, n * 36);
        add(s.rect2, n * 8);
        add(s.done_index, n * 4);
        add(s.done_count, 4);
        if (ctx->env_cfg.task == rf::kEnvTaskComposed) {
            const rf_env_program &p = ctx->env_program;
            size_t rows = 0;
            for (int i = 0; i < p.n_enders; ++i)
                rows += p.enders[i].kind == RF_ENDER_STOPPED ? (size_t)p.enders[i].steps + 1 : 0;
            add(s.leaf_count, (size_t)p.n_enders * n * 4);
            add(s.leaf_float, (size_t)p.n_enders * n * 4);
            add(s.history, rows * n * 4);
            add(s.leaf_old, (size_t)p.n_rewarders * n * 4);
        }
        if (s.observer)
            add(s.obs_old, (size_t)ctx->env_observer.n_old * n * 4);
        if (ctx->env_init)
            add(init_gen(ctx), 4 * sizeof(unsigned long long));
        if (ctx->env_records) { // (the accumulators decide later records; the records themselves are last-step outputs)
            add(s.ep_return, n * 8);
            add(s.ep_length, n * 4);
        }
        if (ctx->env_view) { // (the learner view's state; its rewards and view_final are last-step outputs)
            add(ctx->view_stack, n * (size_t)ctx->env_obs_width * (size_t)ctx->view_cfg.frame_stack * 4);
            add(ctx->view_returns, n * 8);
            // (a grouped view: float64 [G][3][17], one set of moments per group)
            add(ctx->view_moments, (ctx->view_groups ? (size_t)ctx->view_groups : 1) * sizeof(rf::EnvViewMoments));
        }
        add(ctx->d_states, (size_t)ctx->n_states * sizeof(ulonglong2));
    }
};

// The fingerprint of the learner view's configuration: everything but `training`, which is content.  0: no view.
uint64_t view_hash(const rf_ctx *ctx)
{
    if (!ctx->env_view)
        return 0;
    const rf_env_view_config &v = ctx->view_host;
    const int32_t words[3] = {v.frame_stack, v.norm_obs, v.norm_reward};
    const double reals[4] = {v.gamma, v.epsilon, v.clip_obs, v.clip_reward};
    const uint64_t h = fnv1a(fnv1a(kFnvBasis, words, sizeof(words)), reals, sizeof(reals));
    const uint64_t ungrouped = h ? h : 1;
    if (ctx->view_groups == 0)
        return ungrouped;
    // A grouped view (rf_env_configure_view_grouped): the same words, then G and the groups' gammas -- what cfg->gamma
    // was does not count, every group has its own.  Never 0 and never what this configuration hashes to ungrouped; the
    // header's view_groups word (0 ungrouped) tells the two kinds apart whatever the hashes are.
    const double grouped_reals[3] = {v.epsilon, v.clip_obs, v.clip_reward};
    const int32_t groups = ctx->view_groups;
    uint64_t x = fnv1a(fnv1a(kFnvBasis, words, sizeof(words)), grouped_reals, sizeof(grouped_reals));
    x = fnv1a(fnv1a(x, "groups", 6), &groups, sizeof(groups));
    x = fnv1a(x, ctx->view_gammas.data(), ctx->view_gammas.size() * sizeof(double));
    while (x == 0 || x == ungrouped)
        ++x;
    return x;
}

// The header a snapshot of the context taken now would have.
rf_env_snapshot_header make_header(const rf_ctx *ctx, size_t total)
{
    rf_env_snapshot_header h;
    memset(&h, 0, sizeof(h));
    h.magic = RF_ENV_SNAPSHOT_MAGIC;
    h.version = RF_ENV_SNAPSHOT_VERSION;
    h.header_bytes = (uint32_t)sizeof(h);
    h.total_bytes = total;
    h.n = ctx->env_host.n;
    h.frame_height = ctx->env_host.frame_height;
    h.spp = ctx->env_host.spp;
    h.gray_mode = ctx->env_host.gray_mode;
    h.task = ctx->env_cfg.task;
    h.obs_width = ctx->env_obs_width;
    h.device_initializer = ctx->env_init ? 1 : 0;
    h.episode_records = ctx->env_records ? 1 : 0;
    h.n_states = ctx->n_states;
    h.config_hash = fnv1a(fnv1a(kFnvBasis, &ctx->env_host, sizeof(ctx->env_host)), &ctx->env_cfg.stop_threshold,
                          sizeof(ctx->env_cfg.stop_threshold));
    h.program_hash = fnv1a(kFnvBasis, &ctx->env_program, sizeof(ctx->env_program));
    h.observer_hash = fnv1a(kFnvBasis, &ctx->env_observer, sizeof(ctx->env_observer));
    h.initializer_hash = kFnvBasis;
    if (ctx->env_init) { // the ranges; not the jump table, which follows the generator's increment
        const rf::EnvInit &p = ctx->env_init_host;
        uint64_t x = fnv1a(kFnvBasis, p.counts, sizeof(p.counts));
        x = fnv1a(x, &p.draws, sizeof(p.draws));
        x = fnv1a(x, p.low, sizeof(p.low));
        h.initializer_hash = fnv1a(x, p.span, sizeof(p.span));
    }
    h.scene_len = ctx->env_scene_len;
    h.last_partial = ctx->env_last_partial ? 1 : 0;
    h.view_hash = view_hash(ctx);
    h.view_training = ctx->env_view && ctx->view_training ? 1 : 0;
    h.view_groups = ctx->env_view ? ctx->view_groups : 0;
    return h;
}

// Does a snapshot with header `got` belong to the configuration whose header is `want`?  Names the first difference.
int check_header(const rf_env_snapshot_header &got, const rf_env_snapshot_header &want, const char *fn)
{
    RF_REQUIRE(got.magic == want.magic, "%s: not a snapshot (magic %016llx)", fn, (unsigned long long)got.magic);
    RF_REQUIRE(got.version == want.version && got.header_bytes == want.header_bytes,
               "%s: snapshot layout version %u with a header of %u bytes; this library reads version %u (%u bytes)", fn,
               got.version, got.header_bytes, want.version, want.header_bytes);
#define RF_SAME(field, what)                                                                                    \
    RF_REQUIRE(got.field == want.field, "%s: the snapshot was taken with " what " %lld, the context has %lld", fn, \
               (long long)got.field, (long long)want.field)
    RF_SAME(n, "n =");
    RF_SAME(frame_height, "frame height");
    RF_SAME(spp, "spp");
    RF_SAME(gray_mode, "gray mode");
    RF_SAME(task, "task");
    RF_SAME(obs_width, "observation width");
    RF_SAME(device_initializer, "device initializer =");
    RF_SAME(episode_records, "episode records =");
    RF_SAME(n_states, "rf_num_states =");
#undef RF_SAME
    RF_REQUIRE(got.config_hash == want.config_hash, "%s: the snapshot was taken under another rf_env_config", fn);
    RF_REQUIRE(got.program_hash == want.program_hash, "%s: the snapshot was taken under another rf_env_program", fn);
    RF_REQUIRE(got.observer_hash == want.observer_hash, "%s: the snapshot was taken under another observer program", fn);
    RF_REQUIRE(got.initializer_hash == want.initializer_hash,
               "%s: the snapshot was taken under another initializer program (ranges)", fn);
    RF_REQUIRE(got.view_hash == want.view_hash, "%s: the snapshot was taken %s, the context has %s", fn,
               got.view_hash ? "under another learner view configuration" : "without a learner view",
               want.view_hash ? "one" : "none");
    RF_REQUIRE(got.view_groups == want.view_groups, "%s: the snapshot was taken under %s learner view (%d groups), the "
               "context has %s (%d)", fn, got.view_groups ? "a grouped" : "an ungrouped", got.view_groups,
               want.view_groups ? "a grouped one" : "an ungrouped one", want.view_groups);
    RF_REQUIRE(got.view_training == 0 || got.view_training == 1, "%s: the snapshot's view_training word is %d", fn,
               got.view_training);
    RF_REQUIRE(got.total_bytes == want.total_bytes, "%s: the snapshot says %llu bytes, not %llu", fn,
               (unsigned long long)got.total_bytes, (unsigned long long)want.total_bytes);
    RF_REQUIRE(got.scene_len >= 1 && got.scene_len <= want.n && (got.last_partial == 0 || got.last_partial == 1),
               "%s: the snapshot's scene set (%d environments, partial %d) is not one of this configuration", fn,
               got.scene_len, got.last_partial);
    return RF_OK;
}

int may_snapshot(const rf_ctx *ctx, const char *fn)
{
    RF_REQUIRE(ctx->env_ready, "%s: rf_env_configure first", fn);
    RF_REQUIRE(ctx->env_started, "%s: rf_env_reset first", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase or planned step is open", fn);
    RF_REQUIRE(!ctx->env_needs_reset, "%s: a step was aborted (rf_env_reset first)", fn);
    RF_REFUSE_FAULTED(ctx, fn);
    return RF_OK;
}

int may_restore(const rf_ctx *ctx, const char *fn)
{
    RF_REQUIRE(ctx->env_ready, "%s: rf_env_configure first", fn);
    RF_REQUIRE(ctx->env_pending < 0, "%s: a two-phase or planned step is open", fn);
    return RF_OK;
}

int check_slot(int slot, const char *fn)
{
    RF_REQUIRE(slot >= 0 && slot < RF_ENV_SNAPSHOT_SLOTS, "%s: slot %d outside [0, %d)", fn, slot, RF_ENV_SNAPSHOT_SLOTS);
    return RF_OK;
}

// What a restore does besides its copies, before them: the one-time allocations of rf_env_reset for a context that
// was never reset (full_pass: the frame buffers, outside any captured step), and the generator's jump table when the
// snapshot's increment is not the context's (rf_env_set_initializer_state's upload; the caller synchronises).
int prepare_restore(rf_ctx *ctx, const unsigned long long inc[2])
{
    if (!ctx->env_started) {
        const int n = ctx->env_host.n, fh = ctx->env_host.frame_height;
        int rc = ensure_frames(ctx, n, fh, fh);
        if (rc == RF_OK && ctx->env_fused && ctx->env_axis)
            rc = ensure_frames2(ctx, n, fh, fh);
        if (rc != RF_OK)
            return rc;
    }
    if (ctx->env_init && (inc[0] != ctx->env_gen_host[2] || inc[1] != ctx->env_gen_host[3])) {
        RF_HIP(hipStreamSynchronize(ctx->stream)); // (an earlier upload may still read env_init_host)
        rf::init_jump_table(ctx->env_init_host, rf::U128{inc[0], inc[1]});
        ctx->env_gen_host[2] = inc[0];
        ctx->env_gen_host[3] = inc[1];
        RF_HIP(hipMemcpyAsync(ctx->d_init, &ctx->env_init_host, sizeof(rf::EnvInit), hipMemcpyHostToDevice, ctx->stream));
        RF_HIP(hipStreamSynchronize(ctx->stream));
    }
    return RF_OK;
}

// the host-side half of a restore, once its copies are enqueued
void restored(rf_ctx *ctx, const rf_env_snapshot_header &head)
{
    ctx->env_scene_len = head.scene_len;
    ctx->env_last_partial = head.last_partial != 0;
    ctx->env_needs_reset = false;
    ctx->env_planned = false;
    ctx->env_started = true;
    if (ctx->env_view) { // (the training flag is content; the stack holds whatever the snapshotted context last computed)
        ctx->view_training = head.view_training != 0;
        ctx->view_after_step = false;
    }
}

} // namespace

namespace rfh {

void drop_env_snapshots(rf_ctx *ctx)
{
    for (rf_ctx::SnapshotSlot &slot : ctx->env_slots) {
        if (slot.d)
            (void)hipFree(slot.d);
        slot = rf_ctx::SnapshotSlot{};
    }
}

} // namespace rfh

extern "C" {

int rf_env_snapshot_size(rf_ctx *ctx, uint64_t *bytes)
{
    RF_REQUIRE(ctx != nullptr && bytes != nullptr, "rf_env_snapshot_size: NULL argument");
    RF_REQUIRE(ctx->env_ready, "rf_env_snapshot_size: rf_env_configure first");
    RF_HIP(hipSetDevice(ctx->device));
    *bytes = Layout(ctx).total;
    return RF_OK;
}

int rf_env_snapshot(rf_ctx *ctx, void *host_out, uint64_t bytes)
{
    const char *fn = "rf_env_snapshot";
    RF_REQUIRE(ctx != nullptr && host_out != nullptr, "%s: NULL argument", fn);
    RF_HIP(hipSetDevice(ctx->device));
    if (int rc = resolve_device_steps(ctx)) // (the header holds the scene length)
        return rc;
    if (int rc = may_snapshot(ctx, fn))
        return rc;
    const Layout layout(ctx);
    RF_REQUIRE(bytes == layout.total, "%s: %llu bytes, but a snapshot of this context has %llu (rf_env_snapshot_size)", fn,
               (unsigned long long)bytes, (unsigned long long)layout.total);
    RF_HIP(hipSetDevice(ctx->device));
    char *out = (char *)host_out;
    const rf_env_snapshot_header head = make_header(ctx, layout.total);
    memcpy(out, &head, sizeof(head));
    for (const Piece &p : layout.pieces) {
        RF_HIP(hipMemcpyAsync(out + p.offset, p.dev, p.bytes, hipMemcpyDeviceToHost, ctx->stream));
        const size_t end = p.offset + p.bytes, next = (end + kAlign - 1) & ~(kAlign - 1);
        memset(out + end, 0, next - end); // (the gaps are part of the blob: equal snapshots are equal bytes)
    }
    RF_HIP(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

int rf_env_restore(rf_ctx *ctx, const void *host_in, uint64_t bytes)
{
    const char *fn = "rf_env_restore";
    RF_REQUIRE(ctx != nullptr && host_in != nullptr, "%s: NULL argument", fn);
    RF_HIP(hipSetDevice(ctx->device));
    if (int rc = resolve_device_steps(ctx)) // (before the scene words it would set are replaced)
        return rc;
    if (int rc = may_restore(ctx, fn))
        return rc;
    const Layout layout(ctx);
    const char *in = (const char *)host_in;
    rf_env_snapshot_header head;
    if (bytes >= sizeof(head)) { // (the two settings' blobs differ in size: name the setting, not the size)
        memcpy(&head, in, sizeof(head));
        RF_REQUIRE(head.magic != RF_ENV_SNAPSHOT_MAGIC || head.version != RF_ENV_SNAPSHOT_VERSION ||
                       head.episode_records == (ctx->env_records ? 1 : 0),
                   "%s: the snapshot was taken with episode records = %d, the context has %d", fn, head.episode_records,
                   ctx->env_records ? 1 : 0);
        RF_REQUIRE(head.magic != RF_ENV_SNAPSHOT_MAGIC || head.version != RF_ENV_SNAPSHOT_VERSION ||
                       head.view_hash == view_hash(ctx),
                   "%s: the snapshot was taken %s, the context has %s", fn,
                   head.view_hash ? "under another learner view configuration" : "without a learner view",
                   ctx->env_view ? "one" : "none");
    }
    RF_REQUIRE(bytes == layout.total, "%s: %llu bytes, but a snapshot of this context has %llu (rf_env_snapshot_size)", fn,
               (unsigned long long)bytes, (unsigned long long)layout.total);
    memcpy(&head, in, sizeof(head));
    if (int rc = check_header(head, make_header(ctx, layout.total), fn))
        return rc;
    unsigned long long inc[2] = {0, 0};
    if (ctx->env_init) {
        for (const Piece &p : layout.pieces)
            if (p.dev == (void *)init_gen(ctx))
                memcpy(inc, in + p.offset + 2 * sizeof(unsigned long long), sizeof(inc));
        RF_REQUIRE(inc[0] & 1u, "%s: the snapshot's generator has an even increment", fn);
    }
    RF_HIP(hipSetDevice(ctx->device));
    if (int rc = prepare_restore(ctx, inc))
        return rc;
    for (const Piece &p : layout.pieces)
        RF_HIP(hipMemcpyAsync(p.dev, in + p.offset, p.bytes, hipMemcpyHostToDevice, ctx->stream));
    RF_HIP(hipStreamSynchronize(ctx->stream));
    restored(ctx, head);
    return RF_OK;
}

int rf_env_snapshot_resident(rf_ctx *ctx, int slot)
{
    const char *fn = "rf_env_snapshot_resident";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_HIP(hipSetDevice(ctx->device));
    if (int rc = resolve_device_steps(ctx)) // (the header holds the scene length)
        return rc;
    if (int rc = may_snapshot(ctx, fn))
        return rc;
    if (int rc = check_slot(slot, fn))
        return rc;
    RF_HIP(hipSetDevice(ctx->device));
    const Layout layout(ctx);
    rf_ctx::SnapshotSlot &s = ctx->env_slots[slot];
    if (s.d && s.head.total_bytes != layout.total) { // (filled under a configuration of another size: rf_seed)
        RF_HIP(hipStreamSynchronize(ctx->stream));
        RF_HIP(hipFree(s.d));
        s = rf_ctx::SnapshotSlot{};
    }
    if (!s.d)
        RF_HIP(dev_malloc(&s.d, layout.total));
    s.head = make_header(ctx, layout.total);
    s.inc[0] = ctx->env_gen_host[2];
    s.inc[1] = ctx->env_gen_host[3];
    for (const Piece &p : layout.pieces)
        RF_HIP(hipMemcpyAsync((char *)s.d + p.offset, p.dev, p.bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return RF_OK;
}

int rf_env_restore_resident(rf_ctx *ctx, int slot)
{
    const char *fn = "rf_env_restore_resident";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    RF_HIP(hipSetDevice(ctx->device));
    if (int rc = resolve_device_steps(ctx)) // (before the scene words it would set are replaced)
        return rc;
    if (int rc = may_restore(ctx, fn))
        return rc;
    if (int rc = check_slot(slot, fn))
        return rc;
    const rf_ctx::SnapshotSlot &s = ctx->env_slots[slot];
    RF_REQUIRE(s.d != nullptr, "%s: slot %d is empty", fn, slot);
    const Layout layout(ctx);
    if (int rc = check_header(s.head, make_header(ctx, layout.total), fn))
        return rc;
    RF_HIP(hipSetDevice(ctx->device));
    if (int rc = prepare_restore(ctx, s.inc))
        return rc;
    for (const Piece &p : layout.pieces)
        RF_HIP(hipMemcpyAsync(p.dev, (const char *)s.d + p.offset, p.bytes, hipMemcpyDeviceToDevice, ctx->stream));
    restored(ctx, s.head);
    return RF_OK;
}

int rf_env_snapshot_drop(rf_ctx *ctx, int slot)
{
    const char *fn = "rf_env_snapshot_drop";
    RF_REQUIRE(ctx != nullptr, "%s: ctx is NULL", fn);
    if (int rc = check_slot(slot, fn))
        return rc;
    rf_ctx::SnapshotSlot &s = ctx->env_slots[slot];
    RF_REQUIRE(s.d != nullptr, "%s: slot %d is empty", fn, slot);
    RF_HIP(hipSetDevice(ctx->device));
    RF_HIP(hipStreamSynchronize(ctx->stream)); // (a copy into or out of the slot may still be running)
    RF_HIP(hipFree(s.d));
    s = rf_ctx::SnapshotSlot{};
    return RF_OK;
}

} // extern "C"
