// render.hip -- pt_render / pt_render_prepare / pt_trace: what runs behind vkCmdTraceRaysKHR (main.cpp:659) on the host side.
//
// A call renders its frames in batches of `frames in flight`; a batch is
//     set-up      its slot lanes (frame x sample group) are split over 1-3 PIPELINES, each with its own stream, queue pair and
//                 counters; k_generate fills queue 0 of each
//     rounds      per pipeline and round: [ray sort] -> closest hit -> k_shade [-> shadow rays -> k_shadow_add]; no stream is
//                 drained inside a batch: queue sizes live on the device, the live counts are polled one poll behind
//     finish      the pipelines join, a batch whose term log overflowed is redone with one sample group, k_resolve blends the
//                 batch's frames into the film in frame order (raygen.rgen:86-90)
// The scheduling rules (stagger of two pipelines, the shade rule of three, the lagged poll) are measured choices; each is
// documented where it is applied.  PT_PIPELINE_FUSED replaces rounds by one persistent kernel per batch (fused.hip).
#include "wavefront_host.h"

#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

namespace {
using namespace ptw;

pt_status check_params(pt_scene *s, pt_film *f, const pt_params *p)
{
    pt_ctx *ctx = s->ctx;
    if (p->width != f->w || p->height != f->h) { ctx->err = "params width/height differ from the film's"; return PT_ERR_INVALID_ARG; }
    if (p->world == 0 || p->rank >= p->world) { ctx->err = "rank/world invalid"; return PT_ERR_INVALID_ARG; }
    if (p->spp_per_frame == 0 || p->spp_per_frame > 0xFFFFu || p->max_depth == 0 || p->max_depth > 0xFFFFu) {
        ctx->err = "spp_per_frame and max_depth must be in 1..65535";
        return PT_ERR_INVALID_ARG;
    }
    if (p->frame < 0 || p->frame_count == 0) { ctx->err = "frame must be >= 0 and frame_count >= 1"; return PT_ERR_INVALID_ARG; }
    if (p->pipeline > PT_PIPELINE_AUTO) { ctx->err = "unknown pipeline"; return PT_ERR_UNSUPPORTED; }
    if (p->pipeline == PT_PIPELINE_FUSED && (p->flags & PT_FLAG_ASYNC)) {
        ctx->err = "the fused pipeline has no asynchronous form";
        return PT_ERR_UNSUPPORTED;
    }
    if (p->pipeline == PT_PIPELINE_WAVEFRONT_NEE || (p->flags & PT_FLAG_NEE)) {  // (both NEE pipelines: the wavefront one and k_fused_nee)
        if (p->sample_groups > 1) { ctx->err = "the NEE pipeline runs one sample group per pixel"; return PT_ERR_UNSUPPORTED; }
    }
    return PT_OK;
}


// 0 instanced scenes, 1 scenes walked out of L2 / MALL / HBM, 2 single-level scenes in LDS (film_work.hip ptw_choose_shape)
int launch_class(const pt_scene *s, const ExtendPlan &pl) { return s->n_inst ? 0 : pl.lds_scene ? 2 : 1; }

// The one-time objects of a context's renders: side streams, fork / join / poll / shade events, the pinned poll words.
pt_status ensure_schedule_objects(pt_ctx *ctx, int n_pipes)
{
    for (int k = 1; k < n_pipes; k++)
        if (!ctx->pipe_stream[k]) {
            PT_HIP(ctx, hipStreamCreateWithFlags(&ctx->pipe_stream[k], hipStreamNonBlocking));
            PT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_join[k], hipEventDisableTiming));
        }
    if (!ctx->ev_fork) PT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    if (!ctx->h_poll) PT_HIP(ctx, hipHostMalloc((void **)&ctx->h_poll, sizeof(uint32_t) * 2 * PT_MAX_PIPES, hipHostMallocDefault));
    for (int k = 0; k < n_pipes; k++) {
        for (int j = 0; j < 2; j++)
            if (!ctx->ev_poll[k][j]) PT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_poll[k][j], hipEventDisableTiming));
        if (!ctx->ev_shade[k]) PT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_shade[k], hipEventDisableTiming));
    }
    return PT_OK;
}

pt_status grow_event_pool(pt_ctx *ctx, size_t want)
{
    while (ctx->ev_pool.size() < want) {
        hipEvent_t e = nullptr;
        PT_HIP(ctx, hipEventCreate(&e));
        ctx->ev_pool.push_back(e);
    }
    return PT_OK;
}

// One wavefront pipeline of a batch: a contiguous range of slot lanes with its own stream, queue pair and counters.
struct Pipe {
    hipStream_t st;
    uint32_t slot_begin, n_slots;
    QueueView qv[2];
    float4 *hit;
    uint32_t *hit_inst;
    uint32_t *count;  // [2] queue sizes of this pipeline
    int cur;
    bool done;
    int polls;        // live-count polls queued on this pipeline's stream in the current batch
};

// What one render (a call of either pipeline, or the redo of one of its batches) decides once and every batch or launch uses.
struct Job {
    pt_scene *s; pt_film *f; const pt_params *p; pt_ctx *ctx;
    const TileView *sel = nullptr;  // pt_render_adaptive: the selected tiles (null: the film's own list) ...
    TileView picked;                // ... the selection itself (render_call)
    AdaptCall *ad = nullptr;        // pt_render_adaptive's call
    ExtendPlan pl;
    RenderShape sh;
    RenderConst rc;
    Radiance rad;
    bool fused = false, profile = false, count_visits = false, async = false, nee = false;
    bool shade_lds = false, sort_rays = false, stagger = false;
    int n_pipes = 1, sort_bits = 4, shade_grid = 0;
    size_t shade_smem = 0;
    const float4 *inst_frame = nullptr, *nee_lights = nullptr;
    uint32_t nee_n_lights = 0;
    float nee_light_area = 0.f;
    FusedPlan fp;                   // PT_PIPELINE_FUSED: the launch plan ...
    pt_params q;                    // ... the params with the shape the pipeline picked (p points here)
    int32_t rect[4] = { 0, 0, -1, -1 };  // subject_rect
    // pt_render_guided: every fused launch also writes the film's first-hit log, sized by the caller, and the reduce behind it folds it into the guides
    GuidedCall *gd = nullptr;
    std::vector<hipEvent_t> ev_extend, ev_shade, ev_reduce;  // pooled (start, stop) pairs: the launches' own (PT_FLAG_PROFILE), the guided reduces'
    size_t ev_used = 0;
};

// The next (start, stop) pair of the pool, remembered in `pairs` for add_event_pairs
pt_status take_event_pair(Job &j, std::vector<hipEvent_t> &pairs, hipEvent_t &e0, hipEvent_t &e1)
{
    PT_TRY(grow_event_pool(j.ctx, j.ev_used + 2));
    e0 = j.ctx->ev_pool[j.ev_used++]; e1 = j.ctx->ev_pool[j.ev_used++];
    pairs.push_back(e0); pairs.push_back(e1);
    return PT_OK;
}
void add_event_pairs(const std::vector<hipEvent_t> &pairs, float &ms)
{
    for (size_t i = 0; i + 1 < pairs.size(); i += 2) {
        float a = 0.f;
        if (hipEventElapsedTime(&a, pairs[i], pairs[i + 1]) == hipSuccess) ms += a;
    }
}

// The radiance record of the job's shape over the film's buffers as they stand, with the spill pool's share: worst-case logs never reach the pool.
// The fused kernels also read it from device memory, for the ends of the log they rarely take (Radiance::dev): uploaded when it changes.
pt_status set_radiance(Job &j)
{
    pt_ctx *ctx = j.ctx;
    const pt_film::Work &w = j.f->work;
    uint32_t spill_cap = j.sh.bounded ? SPILL_POOL_ENTRIES : 0u;
    if (ctx->tune.term_spill >= 0) spill_cap = std::min<uint32_t>(spill_cap, (uint32_t)ctx->tune.term_spill);  // tests
    static_assert(sizeof(Radiance) <= sizeof(pt_ctx::h_rad), "pt_ctx::h_rad holds a Radiance");
    j.rad = { w.d_color, w.d_terms, w.d_terms_over, w.d_nterm, w.d_spill, w.d_spill_head, ctx->d_stats + PT_STAT_SPILL_FILL, spill_cap,
              ctx->d_stats + PT_STAT_OVERFLOW, j.fused ? static_cast<const Radiance *>(ctx->d_rad) : nullptr };
    if (!j.fused || std::memcmp(ctx->h_rad, &j.rad, sizeof(j.rad)) == 0) return PT_OK;
    // On the stream, ahead of the launch that reads it, from the context's own (pageable) copy.  No kernel can be reading d_rad meanwhile: only the
    // fused kernels do, every fused call ends with a stream sync, and the redo syncs before it comes here.  A failed copy leaves h_rad equal to no record.
    std::memcpy(ctx->h_rad, &j.rad, sizeof(j.rad));
    const hipError_t e = hipMemcpyAsync(ctx->d_rad, ctx->h_rad, sizeof(j.rad), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) std::memset(ctx->h_rad, 0, sizeof(ctx->h_rad));
    PT_HIP(ctx, e);
    return PT_OK;
}

// The pixel rectangle the scene's box projects to (film_work.hip ptw_tiles_subject_first: its tiles are handed out first).  The camera of
// raygen.rgen:51-57 shoots from cam_origin through (target.x + dx, target.y + dy, target.z), dx, dy in [-1, 1] across the image: a point P in
// front of the origin lands at dx = o.x + (P.x - o.x) (t.z - o.z) / (P.z - o.z) - t.x.  A box is convex, so its image lies inside the bounding
// rectangle of its corners' images.  No rectangle (x1 < x0) when a corner is not in front of the origin (the camera is inside or beside the
// box).  Used twice: as a guess about cost (the hand-out order) and as a proof (the cull below):
// the pixel of slack on every side is far above the rounding of this projection and of raygen's own.
void subject_rect(const pt_scene *s, const pt_params *p, int32_t rect[4])
{
    rect[0] = rect[1] = 0; rect[2] = rect[3] = -1;
    const float *bmin = s->n_inst ? s->tlas_bmin : s->bmin, *bmax = s->n_inst ? s->tlas_bmax : s->bmax;  // (two-level: the union of the instances' world boxes)
    const float den = p->cam_target[2] - p->cam_origin[2];
    if (!(std::fabs(den) > 0.f)) return;
    float lo[2] = { 3.0e38f, 3.0e38f }, hi[2] = { -3.0e38f, -3.0e38f };
    for (int c = 0; c < 8; c++) {
        const float P[3] = { (c & 1) ? bmax[0] : bmin[0], (c & 2) ? bmax[1] : bmin[1], (c & 4) ? bmax[2] : bmin[2] };
        const float a = (P[2] - p->cam_origin[2]) / den;  // how far along the view axis the corner is, in units of the image plane's distance
        if (!(a > 1.0e-4f)) return;
        for (int k = 0; k < 2; k++) {
            const float d = p->cam_origin[k] + (P[k] - p->cam_origin[k]) / a - p->cam_target[k];
            lo[k] = std::min(lo[k], d); hi[k] = std::max(hi[k], d);
        }
    }
    const float size[2] = { (float)p->width, (float)p->height };
    int32_t r[4];
    for (int k = 0; k < 2; k++) {  // dx -> pixel (raygen.rgen:52-53 inverted), one pixel of slack, clamped to the image
        const float a = (lo[k] + 1.0f) * 0.5f * size[k] - 1.0f, b = (hi[k] + 1.0f) * 0.5f * size[k] + 1.0f;
        if (!(a == a) || !(b == b) || b < 0.f || a > size[k]) return;  // (NaN, or the box is off the image: no subject to put first)
        r[k] = (int32_t)std::max(a, 0.f);
        r[k + 2] = (int32_t)std::min(b, size[k] - 1.0f);
    }
    std::copy(r, r + 4, rect);
}

// Pixels outside the rectangle cannot see the scene: their slots are finished where they are handed out / generated (wavefront_types.h
// RenderConst::cull, fused_cull.h; pt_tuning.cull = 0: every camera ray is walked; an instrumented render measures the walk of every ray unless
// pt_tuning.cull = 1 asks for the walked ones only).  The sum a slot without a log stores is the reference's sequence of adds (raygen.rgen:76 with weight 1 and miss.rmiss:10), done here.
void apply_cull(const pt_ctx *ctx, const pt_params *p, const int32_t rect[4], RenderConst &rc)
{
    rc.cull_on = 0u;
    if (rect[2] < rect[0] || rect[3] < rect[1] || ctx->tune.cull == 0 || ((p->flags & PT_FLAG_COUNT_VISITS) && ctx->tune.cull != 1)) return;
    if (!std::isfinite(p->env[0]) || !std::isfinite(p->env[1]) || !std::isfinite(p->env[2])) return;
    rc.cull_on = 1u;
    std::copy(rect, rect + 4, rc.cull);
    for (int k = 0; k < 3; k++) {
        volatile float c = 0.0f;  // (volatile: one rounded float add per sample, nothing folded)
        for (uint32_t i = 0; i < p->spp_per_frame; i++) c = c + 1.0f * p->env[k];
        rc.cull_sum[k] = c;
    }
}

// ---- once per render, both pipelines: the radiance record, the render constants with the cull ---------------------------------------------
pt_status job_begin(Job &j)
{
    PT_TRY(set_radiance(j));
    j.rc = ptw_render_const(j.p, ptw_tile_view(j.f, j.sel).n_tiles, j.sh);
    subject_rect(j.s, j.p, j.rect);
    apply_cull(j.ctx, j.p, j.rect, j.rc);
    j.profile = (j.p->flags & PT_FLAG_PROFILE) != 0;  // (never a redo's: redo_batch)
    return PT_OK;
}
// ---- once per call: kernel plan, shape + workspace, number of pipelines, ray-sort scratch, shadow queue -----------------
pt_status job_setup(Job &j)
{
    pt_scene *s = j.s; pt_film *f = j.f; const pt_params *p = j.p; pt_ctx *ctx = j.ctx;
    pt_film::Work &w = f->work;
    const uint32_t lanes = j.sh.lanes, groups = j.sh.groups;
    PT_TRY(job_begin(j));
    j.count_visits = (p->flags & PT_FLAG_COUNT_VISITS) != 0;
    j.async = (p->flags & PT_FLAG_ASYNC) != 0;
    if (j.async && j.profile) { ctx->err = "PT_FLAG_ASYNC and PT_FLAG_PROFILE exclude each other"; return PT_ERR_INVALID_ARG; }

    // k_shade's launch shape and, for instanced scenes, its (instance, triangle) frame table (wavefront_host.h)
    ptw_shade_shape(ctx, s, j.pl, j.shade_grid, j.shade_smem, j.shade_lds);
    PT_TRY(ptw_shade_inst_frames(s, j.pl, j.inst_frame));
    // Pipelines: the slot lanes of a batch are split into parts that run their rounds independently on separate streams, so
    // the VALU-bound traversal of one overlaps the memory-bound shading of another.  Two for most shapes (a third: C4 -1 ... -3 %,
    // C5 -3 ... -6 %; a fourth loses everywhere).  THREE where both kernels keep their tables in LDS, the scene has one level and
    // the batch holds >= 24 M slots: free-running, two pipelines can settle with traversal beside traversal and shade beside
    // shade for a whole process (C2: 22.3-23.0 Grays/s in one pass of a box, 24.0-24.6 in the next); three, held in rotation by
    // the shade rule (run_rounds), cannot: C2 at K = 16 25.8-27.1 against 23.2-24.6, K = 8 +6 %, K = 4 +2.3 %, K = 2 +1.7 %
    // (profiles/r03v_c2_pipes.log, r03w_pipes_by_shape.log, r03aj_shade_rule_other_shapes.log).  Small batches keep one pipeline.
    const bool three = j.shade_lds && !s->n_inst && (uint64_t)w.n_slots >= (24ull << 20);
    int n_pipes = three ? 3 : ((uint64_t)w.n_slots >= (4ull << 20) ? 2 : 1);
    n_pipes = pt_tuned(ctx->tune.pipes, n_pipes, 1, PT_MAX_PIPES);
    j.n_pipes = std::max(1, std::min(n_pipes, std::min<int>(PT_MAX_PIPES, (int)(lanes * groups))));
    ctx->stats.pipelines = (uint32_t)j.n_pipes;
    const pt_status rce = ensure_schedule_objects(ctx, j.n_pipes);
    if (rce != PT_OK) return rce;
    // (two pipelines start half a round apart; three start together and keep the shade rule: run_rounds)
    j.stagger = ctx->tune.stagger < 0 ? j.n_pipes == 2 : ctx->tune.stagger == 1;

    // ray sorting (ray_sort.hip): the HBM kernels only; AUTO when the traversal working set does not fit the Infinity Cache
    if ((j.pl.variant == PT_EXTEND_HBM || j.pl.variant == PT_EXTEND_HBM8) && !s->n_inst) {
        const uint64_t working_set = j.pl.bvh8 ? 64ull * s->n_wide8 + 64ull * s->n_tris
                                               : 64ull * (j.pl.topdown4 ? s->n_wide16t : s->n_wide) + 48ull * s->n_tris;
        j.sort_rays = working_set > (256ull << 20);
        if (p->flags & PT_FLAG_SORT_RAYS) j.sort_rays = true;
        if (p->flags & PT_FLAG_NO_SORT_RAYS) j.sort_rays = false;
    }
    // 4 bits per axis + octant = 15-bit keys = two 8-bit passes (C5x: 6 bits, three passes: +0 %, 4 bits: +3.5 %)
    j.sort_bits = pt_tuned(ctx->tune.sort_bits, 4, 1, 9);
    if (j.sort_rays) {
        // one scratch area per pipeline, sized for that pipeline's share of the slots (+ slack for the uneven split)
        const size_t per_pipe = ptw_ray_sort_bytes((size_t)w.n_slots / (size_t)j.n_pipes + (size_t)j.rc.slots_per_lane + 1);
        const size_t need = per_pipe * (size_t)j.n_pipes;
        if (need > w.sort_bytes) {  // (in w.bytes, but no budget is asked; no room: render unsorted, and that is no error)
            const std::string keep = ctx->err;
            const bool ok = pt_scratch_alloc(ctx, "ray-sort scratch", { pt_buf_of(w.d_sort, need) }, &w.bytes, w.sort_bytes) == PT_OK;
            w.sort_bytes = ok ? need : 0;
            if (!ok) { j.sort_rays = false; ctx->err = keep; }
        }
    }
    j.nee = p->pipeline == PT_PIPELINE_WAVEFRONT_NEE;
    // the emitters the NEE pipeline samples (wavefront_host.h)
    PT_TRY(ptw_nee_lights(s, j.nee, j.nee_lights, j.nee_n_lights, j.nee_light_area));
    if (j.nee && (size_t)w.n_slots > w.cap_sq) {  // the shadow queue: at most one entry per live path and round
        const size_t ns = w.n_slots;
        w.cap_sq = 0;
        // (the pipelines' count words first: allocated once, kept, and not part of what pt_stats.workspace_bytes reports)
        pt_status rcq = w.d_sq_count ? PT_OK : pt_scratch_alloc(ctx, "shadow queue", { pt_buf_of(w.d_sq_count, sizeof(uint32_t) * PT_MAX_PIPES) }, nullptr, 0);
        if (rcq == PT_OK)
            rcq = pt_scratch_alloc(ctx, "shadow queue", { pt_buf_of(w.d_sq_rayA, sizeof(float4) * ns), pt_buf_of(w.d_sq_rayB, sizeof(float2) * ns),
                                                          pt_buf_of(w.d_sq_contrib, sizeof(float4) * ns), pt_buf_of(w.d_sq_slot, sizeof(uint32_t) * ns),
                                                          pt_buf_of(w.d_sq_tmax, sizeof(float) * ns), pt_buf_of(w.d_sq_hit, sizeof(float4) * ns) },
                                   &w.sq_bytes, w.sq_bytes);
        if (rcq != PT_OK) return rcq;
        w.cap_sq = ns;
    }
    ctx->stats.extend_variant = j.pl.variant;
    return PT_OK;
}

// ---- the overflow redo, the same for both pipelines -----------------------------------------------------------------------------
// A batch (wavefront) or launch (fused) whose term logs are bounded can overflow them (scenes where most surfaces emit): the kernels raise
// PT_STAT_OVERFLOW and nothing of the batch reaches the film -- the wavefront looks before its resolve, the fused pipeline's resolve skips on the flag.
// The host then puts the ray counters back, renders the same frames with one slot per (frame, pixel) -- the plain accumulator needs no log -- and
// returns to the call's workspace shape (redo_batch).
// arm: the two ray counters as they are before the batch, in spare device words: nothing waits for the device.  ON the stream, ahead of the launches
// that add to them: a plain device-to-device copy runs on the null stream, which the library's non-blocking streams are not ordered against.
pt_status redo_arm(Job &j)
{
    if (!j.sh.bounded) return PT_OK;
    pt_ctx *ctx = j.ctx;
    unsigned long long *const w = ctx->d_stats;
    PT_HIP(ctx, hipMemcpyAsync(w + PT_STAT_RAYS_SAVED, w + PT_STAT_RAYS, sizeof(*w), hipMemcpyDeviceToDevice, ctx->stream));
    PT_HIP(ctx, hipMemcpyAsync(w + PT_STAT_RAYS_CULLED_SAVED, w + PT_STAT_RAYS_CULLED, sizeof(*w), hipMemcpyDeviceToDevice, ctx->stream));
    PT_HIP(ctx, hipMemsetAsync(j.rad.spill_count, 0, sizeof(*w), ctx->stream));
    return PT_OK;
}
// check: did a slot fill its term log?  Drains the stream (after the last launch of a blocking call that is the wait the call ends with).
pt_status redo_check(Job &j, bool &redo)
{
    redo = false;
    if (!j.sh.bounded) return PT_OK;
    unsigned long long flag = 0;
    PT_HIP(j.ctx, hipStreamSynchronize(j.ctx->stream));
    PT_HIP(j.ctx, hipMemcpy(&flag, j.rad.overflow, sizeof(flag), hipMemcpyDeviceToHost));
    redo = flag != 0ull;
    return PT_OK;
}
pt_status redo_batch(Job &j);  // (the redo itself stands behind the two pipelines it re-enters)

// ---- per batch: the slot lanes split over the pipelines, queue 0 of each filled ---------------------------------------------
pt_status batch_begin(Job &j, Pipe *pipe, int &pipes_now)
{
    pt_ctx *ctx = j.ctx;
    pt_film::Work &w = j.f->work;
    hipStream_t st = ctx->stream;
    PT_TRY(redo_arm(j));
    PT_HIP(ctx, hipMemsetAsync(w.d_count, 0, sizeof(uint32_t) * 2 * PT_MAX_PIPES, st));
    const uint32_t slot_lanes = j.rc.lanes_active * j.sh.groups;
    pipes_now = std::min<int>(j.n_pipes, (int)slot_lanes);
    for (int k = 0; k < pipes_now; k++) {
        const uint32_t l0 = (uint32_t)((uint64_t)slot_lanes * k / pipes_now);
        const uint32_t l1 = (uint32_t)((uint64_t)slot_lanes * (k + 1) / pipes_now);
        Pipe &pp = pipe[k];
        pp.st = k == 0 ? st : ctx->pipe_stream[k];
        pp.slot_begin = l0 * j.rc.slots_per_lane;
        pp.n_slots = (l1 - l0) * j.rc.slots_per_lane;
        for (int i = 0; i < 2; i++)
            pp.qv[i] = { w.d_qid[i] + pp.slot_begin, w.d_qstate[i] + pp.slot_begin, w.d_qrayA[i] + pp.slot_begin, w.d_qrayB[i] + pp.slot_begin };
        pp.hit = w.d_hit + pp.slot_begin;
        pp.hit_inst = w.d_hit_inst + pp.slot_begin;
        pp.count = w.d_count + 2 * k;
        pp.cur = 0;
        pp.done = false;
        pp.polls = 0;
    }
    if (pipes_now > 1) {  // the other streams start after the counters are cleared
        PT_HIP(ctx, hipEventRecord(ctx->ev_fork, st));
        for (int k = 1; k < pipes_now; k++) PT_HIP(ctx, hipStreamWaitEvent(ctx->pipe_stream[k], ctx->ev_fork, 0));
    }
    for (int k = 0; k < pipes_now; k++) {
        Pipe &pp = pipe[k];
        ptw_launch_generate(j.rc, ptw_tile_view(j.f, j.sel).d_tiles, pp.slot_begin, pp.n_slots, j.rad, pp.qv[0], &pp.count[0], ctx->d_stats, ctx->num_cus, pp.st);
        ctx->stats.launches_other++;
    }
    return PT_OK;
}

// ---- one round of one pipeline: [sort] -> closest hit -> shade [-> shadow rays -> add] ---------------------------------
pt_status pipe_round(Job &j, Pipe *pipe, int k, int pipes_now, uint32_t round, bool shade_rule, bool *shade_recorded)
{
    pt_ctx *ctx = j.ctx; pt_scene *s = j.s; const pt_params *p = j.p;
    pt_film::Work &w = j.f->work;
    Pipe &pp = pipe[k];
    const int cur = pp.cur;
    hipEvent_t x0 = nullptr, x1 = nullptr, h0 = nullptr, h1 = nullptr;
    if (j.profile) {  // from the context's pool: creating ~2000 events per call showed in the wall time
        PT_TRY(take_event_pair(j, j.ev_extend, x0, x1));
        PT_TRY(take_event_pair(j, j.ev_shade, h0, h1));
    }
    const uint32_t *perm = nullptr;
    if (j.sort_rays && round > 0) {  // (round 0 is the primary rays: one origin, generated tile by tile)
        const size_t per_pipe = w.sort_bytes / (size_t)j.n_pipes;
        perm = ptw_sort_rays(pp.st, pp.qv[cur].rayA, pp.qv[cur].rayB, &pp.count[cur], pp.n_slots, s->bmin, s->bmax, j.sort_bits, ctx->num_cus,
                             static_cast<char *>(w.d_sort) + per_pipe * (size_t)k);
        ctx->stats.launches_other += 1 + 5 * (uint32_t)((3 * j.sort_bits + 3 + 7) / 8);
    }
    // Two pipelines start half a round apart: pipeline k > 0 begins its first traversal launch when pipeline k-1's first one
    // has finished.  Started together they can lock in phase -- traversal beside traversal, shade beside shade -- and whether
    // they do depended on the box: same-box A/B 22.45 -> 23.99 Grays/s where all plain runs were slow, no change where they
    // were fast; C4 unchanged (profiles/r02i_ab_stagger.log).  Only where the two kernels are of similar length (tables in
    // LDS) and more than one frame is in flight.  A strict token (one traversal launch at a time) is 20 % slower.
    const bool stag = j.stagger && j.shade_lds && j.rc.lanes_active > 1 && round == 0;
    if (stag && k > 0) PT_HIP(ctx, hipStreamWaitEvent(pp.st, ctx->ev_fork, 0));
    ptw_launch_extend(j.pl, s, pp.qv[cur].rayA, pp.qv[cur].rayB, pp.hit, pp.hit_inst, &pp.count[cur], &pp.count[cur ^ 1], ctx->d_stats, p->tmin,
                      p->tmax, j.count_visits, true, pp.st, k, x0, x1, perm);
    if (stag && k + 1 < pipes_now) PT_HIP(ctx, hipEventRecord(ctx->ev_fork, pp.st));
    // The shade rule (three pipelines): never all three in their shade launch at once.  Pipeline k's shade launch waits for the
    // end of the most recent shade launch of pipeline k + 1 -- the one a third of a rotation ahead, long over when the three are
    // evenly spread, so in the pattern the rule aims at nobody waits, and out of it the laggard is held back until the rotation
    // is restored.  Free-running, the three spend 11-19 % of a frame shade beside shade beside shade (latency-bound, VALUs
    // idle) and which pattern a process falls into is chance: 24.3-25.7 Grays/s over eight processes of one box; with the rule
    // 25.8-27.1, mean +6.0 % (profiles/r03ag_c2_rules_distribution.log).  The same rule on the traversal launches, on both, one
    // position further ahead, or with two / four pipelines: all slower (r03af_*, r03ah_*).
    const int ahead = (k + 1) % pipes_now;
    if (shade_rule && shade_recorded[ahead]) PT_HIP(ctx, hipStreamWaitEvent(pp.st, ctx->ev_shade[ahead], 0));
    ShadeLaunch sl;
    sl.rc = j.rc; sl.tiles = ptw_tile_view(j.f, j.sel).d_tiles; sl.scene = s; sl.bvh8 = j.pl.bvh8; sl.lds_tables = j.shade_lds; sl.nee = j.nee;
    sl.grid = j.shade_grid; sl.smem = j.shade_smem; sl.rad = j.rad; sl.hit = pp.hit; sl.hit_inst = pp.hit_inst;
    sl.in = pp.qv[cur]; sl.out = pp.qv[cur ^ 1]; sl.count_in = &pp.count[cur]; sl.count_out = &pp.count[cur ^ 1];
    sl.inst_frame = j.inst_frame; sl.lights = j.nee_lights; sl.n_lights = j.nee_n_lights; sl.light_area = j.nee_light_area;
    if (j.nee) {
        sl.sq = { w.d_sq_rayA + pp.slot_begin, w.d_sq_rayB + pp.slot_begin, w.d_sq_contrib + pp.slot_begin, w.d_sq_tmax + pp.slot_begin,
                  w.d_sq_slot + pp.slot_begin };
        sl.sq_count = w.d_sq_count + k;
        PT_HIP(ctx, hipMemsetAsync(sl.sq_count, 0, sizeof(uint32_t), pp.st));
    }
    ptw_launch_shade(sl, pp.st, h0, h1);
    if (j.nee && j.nee_n_lights) {
        // the shadow rays of this round: any-hit queries with their own tmax, then the unoccluded terms
        ptw_launch_extend(j.pl, s, sl.sq.rayA, sl.sq.rayB, w.d_sq_hit + pp.slot_begin, nullptr, sl.sq_count, nullptr, ctx->d_stats, p->tmin, p->tmax,
                          false, true, pp.st, k, nullptr, nullptr, nullptr, sl.sq.tmax);
        ptw_launch_shadow_add(j.rc, j.rad, w.d_sq_hit + pp.slot_begin, sl.sq.contrib, sl.sq.slot, sl.sq_count, j.shade_grid, pp.st);
        ctx->stats.launches_extend++;
        ctx->stats.launches_other++;
    }
    PT_HIP(ctx, hipGetLastError());  // a launch the runtime refused (LDS size, grid) must not pass for a rendered round
    if (shade_rule) { PT_HIP(ctx, hipEventRecord(ctx->ev_shade[k], pp.st)); shade_recorded[k] = true; }
    ctx->stats.launches_extend++;
    ctx->stats.launches_shade++;
    pp.cur ^= 1;
    return PT_OK;
}

// The live counts, one poll behind.  Every slot needs >= group_size rounds; after that the counts are polled every eighth
// round so that a batch whose paths have all ended stops early.  The host reads the count of the PREVIOUS poll -- eight rounds
// back -- while each stream still holds eight rounds of launches: waiting for the newest count drained the streams, restarted
// the pipelines in phase and left one of them idle until the other had caught up: 5.3 ms of the 147 ms of 16 C2 frames
// (profiles/r03r_c2_timeline_before.txt).  A pipeline found empty has at most sixteen empty rounds queued behind it.
pt_status poll_live_counts(Job &j, Pipe *pipe, int pipes_now, bool &all_done)
{
    pt_ctx *ctx = j.ctx;
    all_done = true;
    for (int k = 0; k < pipes_now; k++) {
        Pipe &pp = pipe[k];
        if (pp.done) continue;
        const int jj = pp.polls & 1;
        PT_HIP(ctx, hipMemcpyAsync(ctx->h_poll + 2 * k + jj, &pp.count[pp.cur], sizeof(uint32_t), hipMemcpyDeviceToHost, pp.st));
        PT_HIP(ctx, hipEventRecord(ctx->ev_poll[k][jj], pp.st));
        if (pp.polls > 0) {
            PT_HIP(ctx, hipEventSynchronize(ctx->ev_poll[k][jj ^ 1]));
            if (ctx->h_poll[2 * k + (jj ^ 1)] == 0u) pp.done = true;
        }
        pp.polls++;
        if (!pp.done) all_done = false;
    }
    return PT_OK;
}

pt_status run_rounds(Job &j, Pipe *pipe, int pipes_now)
{
    pt_ctx *ctx = j.ctx;
    const uint32_t group_size = j.sh.group_size;
    const uint32_t max_rounds = group_size * j.p->max_depth;  // every sample of a slot at full depth
    bool shade_recorded[PT_MAX_PIPES] = {};
    const bool shade_rule = pipes_now == 3 && ((ctx->tune.stagger < 0 && j.shade_lds) || ctx->tune.stagger == 2);
    for (uint32_t round = 0; round < max_rounds; round++) {
        for (int k = 0; k < pipes_now; k++) {
            if (pipe[k].done) continue;
            const pt_status rc = pipe_round(j, pipe, k, pipes_now, round, shade_rule, shade_recorded);
            if (rc != PT_OK) return rc;
        }
        ctx->stats.rounds++;
        if (!j.async && round + 1 >= group_size && ((round + 1) & 7u) == 0u && round + 1 < max_rounds) {
            bool all_done = false;
            const pt_status rc = poll_live_counts(j, pipe, pipes_now, all_done);
            if (rc != PT_OK) return rc;
            if (all_done) break;
        }
    }
    return PT_OK;
}

// A failure between batch_begin and the join leaves launches queued on the side streams that read and write the film's
// workspace: nothing may free or reuse it before they have drained.
void drain_side_streams(pt_ctx *ctx, int pipes_now)
{
    for (int k = 1; k < pipes_now; k++)
        if (ctx->pipe_stream[k]) (void)hipStreamSynchronize(ctx->pipe_stream[k]);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
}

// the blend of a batch's frames into the film: k_resolve over the film's own list, k_resolve_adapt over a selection
void launch_resolve(pt_film *f, const RenderConst &rc, const TileView &tv, const Radiance &rad, hipStream_t st, const unsigned long long *skip_if_set)
{
    if (tv.counts) ptw_launch_resolve_adapt(rc, tv.d_tiles, rad, f->d_rgb, f->d_bgra, st, skip_if_set, f->m2.ptr(), tv.counts);
    else ptw_launch_resolve(rc, tv.d_tiles, rad, f->d_rgb, f->d_bgra, st, skip_if_set, f->m2.ptr());
}

// ---- per batch: join, term-log overflow check, resolve (or the same frames once more with one sample group) -----------------
pt_status batch_finish(Job &j, int pipes_now)
{
    pt_ctx *ctx = j.ctx;
    hipStream_t st = ctx->stream;
    for (int k = 1; k < pipes_now; k++) {  // join before the resolve reads every pipeline's slots
        PT_HIP(ctx, hipEventRecord(ctx->ev_join[k], ctx->pipe_stream[k]));
        PT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_join[k], 0));
    }
    bool redo = false;
    PT_TRY(redo_check(j, redo));
    if (redo) return redo_batch(j);
    launch_resolve(j.f, j.rc, ptw_tile_view(j.f, j.sel), j.rad, st, nullptr);
    ctx->stats.launches_other++;
    return PT_OK;
}

pt_status wavefront_batch(Job &j)
{
    Pipe pipe[PT_MAX_PIPES];
    int pipes_now = 0;
    pt_status rc = batch_begin(j, pipe, pipes_now);
    if (rc == PT_OK) rc = run_rounds(j, pipe, pipes_now);
    if (rc == PT_OK) rc = batch_finish(j, pipes_now);
    if (rc != PT_OK) drain_side_streams(j.ctx, std::max(pipes_now, j.n_pipes));
    return rc;
}

// ---- the end of a call of either pipeline (it began with ev_a): the wait a blocking call ends with, the device times, the workspace, the samples started
pt_status call_tail(Job &j)
{
    pt_ctx *ctx = j.ctx; const pt_params *p = j.p;
    PT_HIP(ctx, hipEventRecord(ctx->ev_b, ctx->stream));
    if (!j.async) {
        float ms = 0.f;
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        PT_HIP(ctx, hipGetLastError());
        PT_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b));
        ctx->stats.ms_total += ms;
    }
    ctx->stats.workspace_bytes = ptw_workspace_bytes(j.f);
    ctx->stats.paths += (j.sel ? j.sel->pixels : ptw_valid_local_pixels(j.f, p)) * p->spp_per_frame * p->frame_count;  // samples started
    if (j.profile) {
        add_event_pairs(j.ev_extend, ctx->stats.ms_extend);
        add_event_pairs(j.ev_shade, ctx->stats.ms_shade);
    }
    if (j.gd) add_event_pairs(j.ev_reduce, j.gd->guide_ms);
    return PT_OK;
}

// ---- PT_PIPELINE_FUSED (fused.hip, fused_kernel.h) ---------------------------------------------------------------------------
// The shape of a fused render: frames in flight as the wavefront pipeline batches them (<= 32, equal batches), and ONE sample group from
// two frames per launch on; a single frame is cut into 32 groups (one-sample slots at the reference's 32 spp).  What decides is the drain of a launch -- the slots
// handed out last run alone, and a slot of 32 samples is up to 256 rays = ~2.5 ms of a lane's time against ~5.5 ms for a frame -- against
// what groups cost (a 16-B store per radiance term and a log k_resolve replays: ~10 % of a frame).  1080p Cornell box, ms per frame, with
// one-tile batches (fused_kernel.h PT_FUSED_BATCH1): 1 frame 7.2 / 6.9 / 6.4 with 1 / 8 / 32 groups; 2 frames 6.21 / 6.27 with 1 / 16;
// 4 frames 5.78 / 6.15 with 1 / 8 (profiles/r05c_fused_batch1.log, r05d_grouped_cost.log; with the 256-slot batches of round 4 groups
// paid up to 8 frames: r04k_fused_groups_by_frames.log).  Explicit frames_in_flight / sample_groups are taken as given.
// 32 x the head slots that are WALKED (frames x owned pixels that can see the scene: the tiles of the cull rectangle, or all of them where there
// is none) per lane of the fused grid: what the shape rules below go by.
uint32_t fused_slots_x32(const pt_ctx *ctx, const pt_film *f, const pt_params *p, uint32_t frames, const int32_t rect[4])
{
    uint64_t tiles = (uint64_t)((f->w + 7) / 8) * ((f->h + 7) / 8);
    if (rect[2] >= rect[0] && rect[3] >= rect[1] && ctx->tune.cull != 0)
        tiles = (uint64_t)(rect[2] / 8 - rect[0] / 8 + 1) * (uint64_t)(rect[3] / 8 - rect[1] / 8 + 1);
    const uint64_t world = std::max(p->world, 1u);
    const uint64_t heads = (uint64_t)frames * 64ull * ((tiles + world - 1) / world);
    const uint64_t grid_lanes = (uint64_t)std::max(ctx->num_cus, 1) * 6ull * 256ull;  // (six 256-thread workgroups per CU: fused.hip)
    return (uint32_t)std::min<uint64_t>(heads * 32ull / grid_lanes, 1u << 24);
}

void fused_shape_defaults(const pt_film *f, const pt_params *p, const FusedPlan &fp, const int32_t rect[4], pt_params &q)
{
    q = *p;
    if (q.frames_in_flight == 0) {
        const uint32_t cap = 32;
        const uint32_t batches = (p->frame_count + cap - 1) / cap;
        q.frames_in_flight = (p->frame_count + batches - 1) / batches;
    }
    q.frames_in_flight = std::max(1u, std::min(q.frames_in_flight, p->frame_count));
    if (fp.nee) {  // k_fused_nee: one sample group (a slot is a pixel's whole frame), so no term log and no redo
        q.sample_groups = 1;
        return;
    }
    if (q.sample_groups == 0) {
        // every sample its own slot (the smallest divisor of spp that is >= 32, or spp itself) where the launch has little more than one walked
        // slot per lane of the grid -- small films, whatever the frames: 256 x 256 x 4 frames 1.23 ms against 2.50 with one group -- and for a
        // single frame up to 10 per lane (1080p, 3 per lane: 6.43 against 7.24; 2160p, 12 per lane: 24.5 against 23.2, so not there); else one
        // group.  profiles/r05z4_tail_rule.log.  (Where fused_tail_samples below gives S > 0 the head + tail shape replaces either.)
        const uint32_t x32 = fused_slots_x32(f->ctx, f, p, q.frames_in_flight, rect);
        uint32_t g = 1;
        if (x32 < 36u || (q.frames_in_flight < 2u && x32 <= 324u))
            while (g < p->spp_per_frame && (g < 32u || p->spp_per_frame % g)) g++;
        // two-level scenes have no head + tail form: up to four walked slots per lane their slots are cut in eight (the smallest divisor of spp
        // that is >= 8).  The 10 000-instance grid, ms per frame with 1 / 8 / 32 groups: 2 frames 12.90 / 11.57 / 11.76, 4 frames 11.18 / 11.28 /
        // 11.60 (profiles/r05zk_c4_shapes.log)
        else if (fp.inst && x32 <= 130u)
            while (g < p->spp_per_frame && (g < 8u || p->spp_per_frame % g)) g++;
        q.sample_groups = g;
    }
}

// Tail samples per pixel of a fused launch (0: the one-group or all-groups shape above).  A launch with few slots per lane of the grid ends
// with whole 32-sample slots still running; with S of a pixel's samples as one-sample tail slots handed out after every head the launch ends with
// short work, and only those S samples' radiance terms go through the log.  Measured on one MI355X, the Cornell box (58 % of the tiles can see
// it: 3.05 walked slots per lane and 1080p frame), spp 32, depth 8, ms per call as all groups / one group / best S
// (profiles/r05z4_tail_rule.log, r05z_fused_tail_samples.log, r05z2_..., r05z3_... before the cull; r05zf_cull.log with it):
//   walked slots per lane  1.3 (720p x 1)  1.5 (540p x 2)  2.7 (720p x 2)  3.0 (1080p x 1)  6.1 (1080p x 2)  9.1 (1080p x 3)  12.2 (1080p x 4)
//   all / one              3.09 4.19       3.60 4.53       5.80 6.80       6.43 7.24        -    12.40       -    17.64       -     23.0
//   best S                 3.07 (S 24)     3.39 (S 20)     5.72 (S 20)     6.29 (S 16)      11.92 (S 12)     17.35 (S 8)      22.9 (S 4)
//   with the cull          .               .               .               7.11 / 6.15 (16) 12.37 / 11.67 (12) 17.39 / 16.94 (8) 22.70 / 22.32 (4)
// (a rank of world 8 at 16 frames, 6.1: 12.38 -> 12.19; of 4 at 8 frames: 12.38 -> 12.06; 8 and 16 frames: S 2 .. 4 within 0.3 % of none.)
// In single steps with the cull (r05zr_tail_fine.log): one frame S 15 .. 16, two frames S 10 (11.51 against 11.55 at 12), three S 8, four S 6
// (22.11 against 22.22 at 4).
// Round 6, the rule against hand-picked shapes at sizes it was not fitted on (1280 x 720, 1024 x 1024 -- the reference's own launch --, 2560 x 1440,
// 3840 x 2160; K = 1, 2, 20; scripts/probe_shape_rules.py, profiles/r06h_shape_rules.log): within 1 % of the best of twelve shapes everywhere (S 24 against
// the rule's S 20 on one small frame: 2.82 / 2.85 and 2.85 / 2.83 ms in two passes -- noise); nothing changed.
// So by walked slots per lane: under 1.1 -> 0 (all groups); to 2.5 -> 5 spp / 8; to 4.5 -> spp / 2; to 7.9 -> 5 spp / 16; to 10.1 -> spp / 4;
// above -> 0.  (Round 5 had two more steps, 3 spp / 16 up to 13.5 and spp / 8 up to 21.9 per lane: on round 6's kernel -- 17 % faster, its launches end
// sooner -- they cost what they gained or more: 4 / 5 / 6 / 7 frames with S 6 / 4 / 4 / 4 against none 19.43 / 23.89 / 28.51 / 33.10 against 19.44 / 23.62 /
// 28.02 / 32.39 ms, a rank of world 8 at 32 frames 19.69 against 19.15, of world 4 at 16 frames 19.52 against 19.19: profiles/r06u_tail_rule_refit.log.)
// pt_tuning.fused_tail >= 0 overrides.
uint32_t fused_tail_samples(const pt_ctx *ctx, const pt_film *f, const pt_params *p, uint32_t frames, const int32_t rect[4])
{
    const uint32_t spp = p->spp_per_frame;
    if (spp < 2u) return 0u;
    int t = ctx->tune.fused_tail;
    if (t < 0) {
        const uint32_t x = fused_slots_x32(ctx, f, p, frames, rect);
        t = x < 36u ? 0 : x <= 81u ? (int)(spp * 5u / 8u) : x <= 144u ? (int)(spp / 2u) : x <= 252u ? (int)(spp * 5u / 16u) : x <= 324u ? (int)(spp / 4u) : 0;
    }
    return (uint32_t)std::max(0, std::min<int>(t, (int)spp - 1));
}

// What every render entry decides first (plan_call): the params with the pipeline resolved, the closest-hit plan, and the fused launch plan --
// resolve_pipeline's when PT_PIPELINE_AUTO had it look, else made where the fused pipeline first needs it; a call plans the launch once.
struct CallPlan {
    pt_params p;
    ExtendPlan pl;
    FusedPlan fp;  // planned if fp_valid, and then for this value of PT_FLAG_NEE
    bool fp_valid = false, fp_nee = false;
};
pt_status call_fused_plan(pt_scene *s, CallPlan &cp)
{
    const bool nee = (cp.p.flags & PT_FLAG_NEE) != 0;
    if (cp.fp_valid && cp.fp_nee == nee) return PT_OK;
    cp.fp = FusedPlan{};
    cp.fp_nee = nee;
    const pt_status rc = ptw_plan_fused(s, cp.pl, cp.p.tmin, cp.fp, nee);
    cp.fp_valid = rc == PT_OK;
    return rc;
}

// HEAD + TAIL slots (fused_kernel.h MODE 2): where the library picks the groups itself and the launch holds few frames, a pixel's frame is one
// head slot of spp - S samples and S one-sample tail slots -- the launch ends with short work and only the tail's radiance terms go through
// the log (see fused_tail_samples for S).  PT_ERR_OOM: no room for the logs.
pt_status fused_tail_shape(Job &j, uint32_t tail)
{
    pt_film *f = j.f;
    const pt_params *p = &j.q;
    RenderShape &sh = j.sh;
    j.q.sample_groups = 1;
    sh = RenderShape{};
    sh.lanes = p->frames_in_flight; sh.groups = 1; sh.group_size = p->spp_per_frame; sh.tail = tail;
    const uint32_t worst = p->max_depth;                       // a tail slot is one sample: at most one term per ray
    sh.term_pcap = std::min(worst, 3u);
    const uint64_t n_tail = (uint64_t)sh.lanes * tail * (uint64_t)((f->w + 7) / 8) * ((f->h + 7) / 8) * 64ull / std::max(p->world, 1u) + 64;
    uint64_t ocap = std::min<uint64_t>(worst - sh.term_pcap, (1ull << 30) / std::max<uint64_t>(n_tail * sizeof(float4), 1));
    if (j.ctx->tune.term_ocap >= 0) ocap = std::min<uint64_t>(ocap, (uint64_t)j.ctx->tune.term_ocap);
    sh.term_cap = sh.term_pcap + (uint32_t)ocap;
    sh.bounded = sh.term_cap < worst;
    return ptw_ensure_work(f, p->rank, p->world, sh.lanes, 1, sh.term_cap, sh.term_pcap, false, tail);
}

// ---- step 1, shape and workspace: what pt_render_prepare stops after and pt_render_guided sizes its log by ----------------------------------
pt_status fused_shape(Job &j, CallPlan &cp)
{
    pt_scene *s = j.s; pt_film *f = j.f; pt_ctx *ctx = j.ctx;
    const pt_params *p_in = &cp.p;
    if (p_in->width > 0xFFFFu || p_in->height > 0xFFFFu) {  // (the kernel keeps a path's pixel as two 16-bit halves of one LDS word)
        ctx->err = "PT_PIPELINE_FUSED renders images up to 65535 x 65535";
        return PT_ERR_UNSUPPORTED;
    }
    PT_TRY(call_fused_plan(s, cp));
    j.fp = cp.fp;
    if ((p_in->flags & PT_FLAG_NEE) && (p_in->flags & PT_FLAG_COUNT_VISITS)) {
        ctx->err = "PT_FLAG_COUNT_VISITS on the fused pipeline: not with PT_FLAG_NEE (the NEE kernel has no instrumented form)";
        return PT_ERR_UNSUPPORTED;
    }
    if (p_in->flags & PT_FLAG_COUNT_VISITS) {  // the instrumented twin of the single-level kernel (wave-level block counts: pt_get_block_counts)
        if (j.fp.inst || !j.fp.pairs) {
            ctx->err = "PT_FLAG_COUNT_VISITS on the fused pipeline: single-level scenes with pair leaves only (the two-level kernel has no instrumented form)";
            return PT_ERR_UNSUPPORTED;
        }
        j.fp.count = true;
    }
    subject_rect(s, p_in, j.rect);
    fused_shape_defaults(f, p_in, j.fp, j.rect, j.q);
    j.p = &j.q;
    RenderShape &sh = j.sh;
    pt_status rc = PT_OK;
    const uint32_t tail = (!j.fp.inst && !j.fp.nee && p_in->sample_groups == 0) ? fused_tail_samples(ctx, f, p_in, j.q.frames_in_flight, j.rect) : 0u;
    if (tail) {
        rc = fused_tail_shape(j, tail);
        if (rc == PT_ERR_OOM) {  // (no room for the logs: the plain shape)
            fused_shape_defaults(f, p_in, j.fp, j.rect, j.q);
            sh = RenderShape{};
        }
    }
    for (; !sh.tail;) {
        rc = ptw_shape_and_work(f, j.p, sh, 3, false);
        if (rc != PT_ERR_OOM) break;
        // a shape this function chose (the caller passed 0) and that does not fit is planned again smaller, like the wavefront's AUTO
        // shapes: first fewer sample groups (the next smaller divisor of spp), then fewer frames in flight
        if (p_in->sample_groups == 0 && j.q.sample_groups > 1) {
            uint32_t g = j.q.sample_groups - 1;
            while (g > 1 && p_in->spp_per_frame % g) g--;
            j.q.sample_groups = g;
        } else if (p_in->frames_in_flight == 0 && j.q.frames_in_flight > 1) {
            j.q.frames_in_flight = (j.q.frames_in_flight + 1) / 2;
        } else {
            break;
        }
    }
    ctx->stats.frames_in_flight = sh.lanes;
    ctx->stats.sample_groups = sh.groups;
    ctx->stats.tail_samples = sh.tail;
    if (rc != PT_OK) return rc;
    if (j.fp.nee && (sh.groups != 1 || sh.tail || sh.bounded)) {  // (fused_shape_defaults plans nothing else for it: k_fused_nee is MODE 0 only)
        ctx->err = "PT_FLAG_NEE on the fused pipeline: one sample group only";
        return PT_ERR_UNSUPPORTED;
    }
    ctx->stats.workspace_bytes = ptw_workspace_bytes(f);
    return PT_OK;
}

// ---- per render (a call, or the redo of one of its launches): tile order, radiance record, render constants --------------------------------------
pt_status fused_begin(Job &j)
{
    pt_ctx *ctx = j.ctx;
    PT_TRY(job_begin(j));
    ctx->stats.extend_variant = j.pl.variant;
    ctx->stats.pipelines = 1;
    if (j.gd && (size_t)j.sh.lanes * j.rc.slots_per_lane * j.rc.spp > j.f->gd.cap) {  // (never: ptw_render_guided sized the log for this shape)
        ctx->err = "pt_render_guided: the first-hit log is smaller than the launch";
        return PT_ERR_OOM;
    }
    return PT_OK;
}
// the fused pipeline's hand-out order: the tiles that can see the scene first (a selection inherits the order of the list it was made from)
pt_status fused_order_tiles(Job &j)
{
    const int32_t none[4] = { 0, 0, -1, -1 };
    return j.sel || !j.fused ? PT_OK : ptw_tiles_subject_first(j.f, j.ctx->tune.fused_subject == 0 ? none : j.rect, j.ctx->stream);
}

// ---- step 2, one launch: its frames through the fused kernel and k_resolve (pt_render_guided: the log and its reduce), then a look at the overflow flag,
// which the host takes once the stream is idle anyway: after the call's last launch, or before the next of a longer call, whose blend must follow this one's
pt_status fused_launch(Job &j, uint32_t done)
{
    pt_ctx *ctx = j.ctx; pt_scene *s = j.s; pt_film *f = j.f; const pt_params *p = j.p;
    hipStream_t st = ctx->stream;
    RenderConst &rc = j.rc;
    const TileView tv = ptw_tile_view(f, j.sel);
    PT_TRY(redo_arm(j));
    PT_HIP(ctx, hipMemsetAsync(f->work.d_count, 0, sizeof(uint32_t) * PTW_COUNT_WORDS, st));  // the slot counters (fused_kernel.h: eight, 128 B apart)
    const uint32_t n_slots = rc.lanes_active * j.sh.groups * rc.slots_per_lane;  // (head + tail: the launch's head slots; its tail slots follow from rc)
    const int mode = rc.tail ? 2 : (j.sh.groups > 1 ? 1 : 0);
    FastDiv div_frames;
    div_frames.init(std::max(rc.lanes_active, 1u));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (j.profile) PT_TRY(take_event_pair(j, j.ev_extend, e0, e1));
    if (j.gd) {
        PT_TRY(ptw_launch_fused_log(j.fp, mode, div_frames, rc, tv.d_tiles, j.rad, s, n_slots, f->work.d_count, ctx->d_stats, p->tmin, p->tmax, f->gd.d_log, st));
        j.gd->launches++;
    } else {
        ptw_launch_fused(j.fp, mode, div_frames, rc, tv.d_tiles, j.rad, s, n_slots, f->work.d_count, ctx->d_stats, p->tmin, p->tmax, st, e0, e1);
    }
    PT_HIP(ctx, hipGetLastError());
    ctx->stats.launches_extend++;
    ctx->stats.rounds++;
    launch_resolve(f, rc, tv, j.rad, st, j.sh.bounded ? j.rad.overflow : nullptr);  // (leaves the film alone when the flag is up)
    ctx->stats.launches_other++;
    if (j.gd) {
        // The launch's frames into the guide planes, timed by a pair of pooled events (the call is not profiled).  Queued here, before the overflow
        // flag is looked at: a launch whose term log overflows still walks every path to its end, so its log is complete, and the redo --
        // which numbers its slots by the one-group tile order, another list than a grouped launch's (film_work.hip) -- neither writes nor needs it.
        hipEvent_t g0 = nullptr, g1 = nullptr;
        PT_TRY(take_event_pair(j, j.ev_reduce, g0, g1));
        PT_HIP(ctx, hipEventRecord(g0, st));
        const uint32_t last = p->frame_count - 1u - done;  // the call's last frame, counted from this launch's first
        ptg_launch_reduce(s, f, rc, tv.d_tiles, last, j.fp.inst_frame, st);
        PT_HIP(ctx, hipGetLastError());
        PT_HIP(ctx, hipEventRecord(g1, st));
        ctx->stats.launches_other++;
    }
    bool redo = false;
    PT_TRY(redo_check(j, redo));
    return redo ? redo_batch(j) : PT_OK;
}

// ---- both pipelines: the frames of a render, batch by batch or launch by launch -----------------------------------------------------------------
pt_status render_frames(Job &j)
{
    for (uint32_t done = 0; j.rc.n_slots > 0 && done < j.p->frame_count; done += j.sh.lanes) {
        j.rc.frame_base = j.p->frame + (int32_t)done;
        j.rc.lanes_active = std::min(j.sh.lanes, j.p->frame_count - done);
        PT_TRY(j.fused ? fused_launch(j, done) : wavefront_batch(j));
    }
    return PT_OK;
}
// step 1 of a call, and all of pt_render_prepare's: shape and workspace (pt_stats: frames_in_flight, sample_groups, tail_samples, workspace_bytes)
pt_status call_shape(Job &j, CallPlan &cp)
{
    if (j.fused) return fused_shape(j, cp);
    const pt_status rc = ptw_shape_and_work(j.f, j.p, j.sh, launch_class(j.s, j.pl));
    j.ctx->stats.frames_in_flight = j.sh.lanes;
    j.ctx->stats.sample_groups = j.sh.groups;
    if (rc == PT_OK) j.ctx->stats.workspace_bytes = ptw_workspace_bytes(j.f);
    return rc;
}
// a call: shape and workspace, [the adaptive selection,] the render's set-up, its frames between ev_a and ev_b, the timed tail
pt_status render_call(Job &j, CallPlan &cp)
{
    pt_ctx *ctx = j.ctx;
    PT_TRY(call_shape(j, cp));
    PT_TRY(fused_order_tiles(j));
    if (j.ad) {  // pt_render_adaptive: the work is planned for the full list; the selection over it, then nothing but the selection
        PT_TRY(ptad_select(j.f, j.ad->ap, ptw_tile_view(j.f, nullptr), &j.picked, &j.ad->res));
        if (j.ad->dry || j.picked.n_tiles == 0) return PT_OK;
        j.sel = &j.picked;
    }
    PT_TRY(j.fused ? fused_begin(j) : job_setup(j));
    PT_HIP(ctx, hipEventRecord(ctx->ev_a, ctx->stream));
    PT_TRY(render_frames(j));
    return call_tail(j);
}
// The redo of one batch or launch of j (redo_arm): its frames as a render of their own with one sample group -- below the call's timing and stats, and
// without PT_FLAG_PROFILE, which would re-record the caller's pooled events -- then back to the call's shape.
pt_status redo_batch(Job &j)
{
    pt_ctx *ctx = j.ctx;
    unsigned long long *const w = ctx->d_stats;
    PT_HIP(ctx, hipMemcpy(w + PT_STAT_RAYS, w + PT_STAT_RAYS_SAVED, sizeof(*w), hipMemcpyDeviceToDevice));  // (the stream is idle: redo_check)
    PT_HIP(ctx, hipMemcpy(w + PT_STAT_RAYS_CULLED, w + PT_STAT_RAYS_CULLED_SAVED, sizeof(*w), hipMemcpyDeviceToDevice));
    PT_HIP(ctx, hipMemset(j.rad.overflow, 0, sizeof(*w)));
    ctx->stats.redone_batches++;
    Job r{};
    r.s = j.s; r.f = j.f; r.ctx = ctx; r.sel = j.sel; r.pl = j.pl; r.fused = j.fused; r.fp = j.fp;
    std::copy(j.rect, j.rect + 4, r.rect);
    r.q = *j.p;
    r.q.frame = j.rc.frame_base; r.q.frame_count = r.q.frames_in_flight = j.rc.lanes_active; r.q.sample_groups = 1;
    r.q.flags &= ~(uint32_t)PT_FLAG_PROFILE;
    r.p = &r.q;
    PT_TRY(ptw_shape_and_work(r.f, r.p, r.sh, r.fused ? 3 : launch_class(r.s, r.pl), !r.fused));
    PT_TRY(fused_order_tiles(r));
    PT_TRY(r.fused ? fused_begin(r) : job_setup(r));
    PT_TRY(render_frames(r));
    if (j.gd) j.gd->launches++;
    if (!r.async) {
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        PT_HIP(ctx, hipGetLastError());
    }
    PT_TRY(ptw_ensure_work(j.f, j.p->rank, j.p->world, j.sh.lanes, j.sh.groups, j.sh.term_cap, j.sh.term_pcap, !j.fused, j.sh.tail));
    return set_radiance(j);  // (the workspace only grows, but its buffers may have moved)
}

// PT_PIPELINE_AUTO (what pt_params_default returns): the reference's raygen shader is one invocation per pixel that owns its path
// (raygen.rgen:41-91) and its host issues one blocking dispatch per frame (main.cpp:656-683) -- the fused kernel is that shape, and
// wherever it applies it is the faster bit-exact pipeline at every call shape measured (1080p Cornell box, K = 16 / 2 / 1 frames per call:
// 41.2 / 36.0 / 34.9 Grays/s against the wavefront's 28 / 27.5 / 26; a rank of world 8 at 16 frames 36 against 25; the 10 000-instance grid
// 14.9 against 13.9: profiles/r05c_fused_batch1.log) in a workspace of 16 B per slot.  So: fused for the scenes fused.hip plans (they live in
// LDS) when the call is one it can serve (blocking, not instrumented, tmin > 0, image <= 65535^2, the closest-hit kernel left to AUTO);
// the wavefront pipeline for everything else -- big scenes need its queues, sorting and long launches.
//
// PT_FLAG_NEE names the estimator, not the implementation: WAVEFRONT | NEE is PT_PIPELINE_WAVEFRONT_NEE, FUSED | NEE is k_fused_nee (single-level
// scenes of the fused class), and AUTO | NEE is k_fused_nee wherever AUTO would run the fused kernel for a single-level scene, else the
// wavefront NEE pipeline (instanced scenes, asynchronous or instrumented calls, a named closest-hit kernel, big scenes, oversized images).
// Measured on one MI355X, Cornell box, spp 32, depth 8, three alternations, ms per frame wavefront NEE / fused NEE (Grays/s with the shadow rays):
// 1080p 16 frames per call 14.90 / 10.40 (24.4 / 35.0); 1080p one blocking frame per call 26.06 / 12.94 (14.0 / 28.1); the reference's 1024 x 1024
// launch, one blocking frame 18.0 / 8.33 (10.2 / 22.1) -- same frame-0 film.  Fused NEE is ahead at every shape: no shape rule.
uint32_t resolve_pipeline(pt_scene *s, CallPlan &cp)
{
    const pt_params *p = &cp.p;
    const bool nee = (p->flags & PT_FLAG_NEE) != 0;
    if (nee && p->pipeline == PT_PIPELINE_WAVEFRONT) return PT_PIPELINE_WAVEFRONT_NEE;
    if (p->pipeline != PT_PIPELINE_AUTO) return p->pipeline;
    const uint32_t wavefront = nee ? PT_PIPELINE_WAVEFRONT_NEE : PT_PIPELINE_WAVEFRONT;
    if ((p->flags & (PT_FLAG_ASYNC | PT_FLAG_COUNT_VISITS)) || p->extend != PT_EXTEND_AUTO || p->width > 0xFFFFu || p->height > 0xFFFFu)
        return wavefront;
    const std::string keep = s->ctx->err;
    const pt_status rc = call_fused_plan(s, cp);  // (NEE: refuses instanced scenes; the plan stays with the call: fused_shape)
    if (rc != PT_OK) s->ctx->err = keep;  // (not an error of this call: the scene is simply not the fused kernel's)
    if (rc != PT_OK) return wavefront;
    if (nee) return PT_PIPELINE_FUSED;
    // Two-level scenes: the fused two-level kernel, in 0.4 .. 5 GB.  With the pixels that look past the instances out of its queues (the cull)
    // the wavefront pipeline is the faster one on launches of few frames -- the 10 000-instance grid at 1080p, ms per frame fused / wavefront:
    // 1 frame 11.95 / 10.40, 2 frames 11.41 / 10.98, 4 frames 11.08 / 10.55, 8 frames 10.49 / 10.39, 16 frames 10.21 / 10.30
    // (profiles/r06d_c4_pipelines.log) -- but it takes 13 .. 37 GB for that, and under the library's own workspace budget (8 GB,
    // pt_internal.h) its shapes shrink until the fused kernel is ahead at every frame count (8 frames: 15.0 against 15.5 Grays/s,
    // profiles/r06e_mem_budget.log).  So the queues only where they are >= 15 % ahead AND the caller has raised the budget to what they
    // take: one frame per launch with >= 16 GB.
    if (cp.fp.inst) {
        const uint32_t per_launch = p->frames_in_flight ? std::min(p->frames_in_flight, p->frame_count) : std::min(p->frame_count, 32u);
        const size_t budget = s->ctx->mem_budget;
        if (per_launch == 1u && (budget == 0 || budget >= ((size_t)16 << 30))) return PT_PIPELINE_WAVEFRONT;
    }
    return PT_PIPELINE_FUSED;
}

// What every entry begins with: the scene repaired, the params checked, the closest-hit kernel planned, the pipeline resolved (pt_stats.pipeline).
// pt_render and pt_render_prepare repair first -- a repair may bring back the instance set a failed pt_scene_update parked.  pt_render_adaptive and
// pt_render_guided, their own parameter struct validated, pass their rule about pt_params (-> why not, or null): tested behind check_params and
// ahead of the repair, as they always tested it.
using EntryRule = const char *(*)(const pt_params *);
pt_status plan_call(pt_scene *s, pt_film *f, const pt_params *p_in, CallPlan &cp, EntryRule rule = nullptr)
{
    pt_ctx *ctx = s->ctx;
    if (!rule && s->broken) PT_TRY(ptb_repair(s));
    PT_TRY(check_params(s, f, p_in));
    if (const char *why = rule ? rule(p_in) : nullptr) { ctx->err = why; return PT_ERR_UNSUPPORTED; }
    if (rule && s->broken) PT_TRY(ptb_repair(s));
    PT_TRY(ptw_plan_extend(s, p_in->extend, cp.pl));
    cp.p = *p_in;
    cp.p.pipeline = resolve_pipeline(s, cp);
    ctx->stats.pipeline = cp.p.pipeline;
    return PT_OK;
}
// the job of a planned call (the fused pipeline points p at its own shaped copy: fused_shape)
Job make_job(pt_scene *s, pt_film *f, const CallPlan &cp)
{
    Job j{};
    j.s = s; j.f = f; j.p = &cp.p; j.ctx = s->ctx; j.pl = cp.pl;
    j.fused = cp.p.pipeline == PT_PIPELINE_FUSED;
    return j;
}

}  // namespace

// pt_render_prepare: exactly the shape and workspace pt_render would pick, and the one-time objects of its schedule
pt_status ptw_prepare(pt_scene *s, pt_film *f, const pt_params *p_in)
{
    pt_ctx *ctx = s->ctx;
    CallPlan cp;
    PT_TRY(plan_call(s, f, p_in, cp));
    Job j = make_job(s, f, cp);
    PT_TRY(call_shape(j, cp));
    if (j.fused) return PT_OK;
    const pt_params *p = &cp.p;
    const RenderShape &sh = j.sh;
    PT_TRY(ensure_schedule_objects(ctx, 3));
    if (p->flags & PT_FLAG_PROFILE) {  // the pooled (start, stop) events of every extend / shade launch of one batch (4 per round and pipeline)
        const size_t batches = ((size_t)p->frame_count + sh.lanes - 1) / sh.lanes;
        PT_TRY(grow_event_pool(ctx, std::min<size_t>(4ull * sh.group_size * p->max_depth * 3ull * batches, 1u << 16)));
    }
    return PT_OK;
}

pt_status ptw_render(pt_scene *s, pt_film *f, const pt_params *p_in)
{
    CallPlan cp;
    PT_TRY(plan_call(s, f, p_in, cp));
    Job j = make_job(s, f, cp);
    const pt_status rc_ = render_call(j, cp);
    if (rc_ == PT_OK) f->m2.frames = (uint32_t)p_in->frame + p_in->frame_count;  // what the film and its second-moment plane now average
    return rc_;
}

// pt_render_adaptive: pt_render's plan over the tiles the selection pass keeps (adaptive.hip; include/pt_api.h has the definition).  Every
// refusal comes before anything is allocated, launched or written.
pt_status ptw_render_adaptive(pt_scene *s, pt_film *f, const pt_params *p_in, const pt_adaptive_params *ap, pt_adaptive_result *result)
{
    pt_ctx *ctx = s->ctx;
    if (result) *result = pt_adaptive_result{};
    if (!f->m2.d) return pt_bad(ctx, PT_NO_M_MSG " first");
    if (!f->cnt.d) return pt_bad(ctx, PT_NO_K_MSG " first");
    if (!(std::isfinite(ap->threshold) && ap->threshold >= 0.f)) return pt_bad(ctx, "pt_adaptive_params.threshold must be finite and >= 0");
    if (!(std::isfinite(ap->rel_floor) && ap->rel_floor > 0.f)) return pt_bad(ctx, "pt_adaptive_params.rel_floor must be finite and > 0");
    if (ap->min_frames < 2u || ap->min_frames > 0xFFFFu) return pt_bad(ctx, "pt_adaptive_params.min_frames must be in 2..65535");
    PT_TRY(pt_check_reserved(ctx, "pt_adaptive_params", ap->reserved));
    pt_params p_res = *p_in;
    AdaptCall ad;
    ad.ap = ap;
    ad.dry = p_in->frame_count == 0;
    if (ad.dry) p_res.frame_count = 1;  // (a dry run plans one frame's work: it needs the rank's tile list and nothing else)
    CallPlan cp;
    PT_TRY(plan_call(s, f, &p_res, cp, [](const pt_params *p) -> const char * {
        const bool bad = (p->flags & (PT_FLAG_ASYNC | PT_FLAG_PROFILE | PT_FLAG_COUNT_VISITS)) != 0;
        return bad ? "pt_render_adaptive: not with PT_FLAG_ASYNC, PT_FLAG_PROFILE or PT_FLAG_COUNT_VISITS (the call reads the selection's count back)" : nullptr;
    }));
    Job j = make_job(s, f, cp);
    j.ad = &ad;
    const pt_status rc_ = render_call(j, cp);
    if (rc_ == PT_OK && result) *result = ad.res;
    return rc_;
}

// pt_render_guided (include/pt_api.h has the contract): pt_render with the guides written from its own camera rays where a fused kernel renders,
// pt_render followed by pt_render_aov everywhere else.  Every refusal comes before anything is allocated, launched or written.
pt_status ptw_render_guided(pt_scene *s, pt_film *f, const pt_params *p_in, const pt_guided_params *gp, pt_guided_result *result)
{
    pt_ctx *ctx = s->ctx;
    if (result) *result = pt_guided_result{};
    if (!f->aov.enabled) return pt_bad(ctx, "the film has no guide buffers: pt_film_enable_aov first");
    if (gp->mode > PT_GUIDED_TWO_CALLS) return pt_bad(ctx, "pt_guided_params.mode is none of PT_GUIDED_AUTO, _SINGLE_PASS, _TWO_CALLS");
    PT_TRY(pt_check_reserved(ctx, "pt_guided_params", gp->reserved));
    CallPlan cp;
    PT_TRY(plan_call(s, f, p_in, cp, [](const pt_params *p) -> const char * {
        if (p->flags & ~(uint32_t)PT_FLAG_NEE) return "pt_render_guided takes no flag but PT_FLAG_NEE: blocking, not instrumented (pt_render_aov's rule)";
        const bool nee_by_pipeline = p->pipeline == PT_PIPELINE_WAVEFRONT_NEE;
        return nee_by_pipeline ? "pt_render_guided: PT_FLAG_NEE names the estimator (pt_render_aov takes PT_PIPELINE_WAVEFRONT, _FUSED or _AUTO)" : nullptr;
    }));
    // the single pass: where a fused kernel renders these params and pt_render_aov's fused or queue form would serve them too
    bool single = gp->mode != PT_GUIDED_TWO_CALLS && cp.p.pipeline == PT_PIPELINE_FUSED && p_in->extend == PT_EXTEND_AUTO && p_in->width <= 0xFFFFu &&
                  p_in->height <= 0xFFFFu;
    const char *why = "pt_render would not run a fused kernel for these params (PT_GUIDED_AUTO takes the two calls)";
    if (single) {  // (PT_PIPELINE_FUSED by name: the scene has to be of the fused kernels' class)
        const std::string keep = ctx->err;
        single = call_fused_plan(s, cp) == PT_OK;
        ctx->err = keep;
    }
    // the log: the frames per launch pt_render would take, or as many as fit beside its workspace (planned again for fewer: at most twice)
    bool have_log = false;
    for (int pass = 0; single && !have_log && pass < 4; pass++) {
        Job shape = make_job(s, f, cp);
        PT_TRY(fused_shape(shape, cp));
        const uint32_t lanes = std::max(ctx->stats.frames_in_flight, 1u);
        const size_t per_frame = (size_t)f->work.n_tiles * 64 * p_in->spp_per_frame;  // records
        if (per_frame == 0) { have_log = true; break; }  // (a rank without tiles: nothing is launched)
        size_t fit = lanes;
        if (ctx->mem_budget) fit = std::min<size_t>(fit, (ctx->mem_budget > f->work.bytes ? ctx->mem_budget - f->work.bytes : 0) / (per_frame * sizeof(uint2)));
        if (fit == 0) { single = false; why = "pt_render_guided: not one frame of the first-hit log fits the memory budget"; break; }
        if (fit < lanes) {  // (equal launches, as pt_render batches its frames: 16 frames where 15 fit are 8 + 8)
            const size_t batches = (p_in->frame_count + fit - 1) / fit;
            cp.p.frames_in_flight = (uint32_t)std::min<size_t>(fit, (p_in->frame_count + batches - 1) / batches);
            continue;
        }
        const std::string keep = ctx->err;
        if (ptg_ensure_log(f, per_frame * lanes) != PT_OK) {  // (the device has no room: the two calls need none)
            ctx->err = keep;
            single = false;
            why = "pt_render_guided: no room for the first-hit log";
        }
        have_log = single;
    }
    if (single && !have_log) { single = false; why = "pt_render_guided: the first-hit log does not fit beside the render workspace"; }
    if (!single && gp->mode == PT_GUIDED_SINGLE_PASS) { ctx->err = why; return PT_ERR_UNSUPPORTED; }
    if (single) {
        GuidedCall gd;
        Job j = make_job(s, f, cp);
        j.gd = &gd;
        PT_TRY(render_call(j, cp));
        f->m2.frames = (uint32_t)p_in->frame + p_in->frame_count;
        if (result) { result->single_pass = 1; result->launches = gd.launches; result->guide_ms = gd.guide_ms; }
        return PT_OK;
    }
    PT_TRY(ptw_render(s, f, p_in));
    const uint32_t rendered_by = ctx->stats.pipeline;
    const float ms_before = ctx->stats.ms_total;
    const pt_status rc_ = pta_render(s, f, p_in);
    ctx->stats.pipeline = rendered_by;
    if (rc_ == PT_OK && result) result->guide_ms = ctx->stats.ms_total - ms_before;
    return rc_;
}

// (aov.hip: the same proof for the guide buffers' single kernel)
void ptw_subject_rect(const pt_scene *s, const pt_params *p, int32_t rect[4]) { subject_rect(s, p, rect); }

pt_status ptw_trace(pt_scene *s, const float *rays6, uint32_t n, float tmin, float tmax, uint32_t extend, pt_hit *hits)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    if (n == 0) return PT_OK;
    ExtendPlan pl;
    pt_status rc_ = ptw_plan_extend(s, extend, pl);
    if (rc_ != PT_OK) return rc_;
    std::vector<float4> a(n);
    std::vector<float2> b(n);
    for (uint32_t i = 0; i < n; i++) {
        const float *r = rays6 + 6 * (size_t)i;
        a[i] = make_float4(r[0], r[1], r[2], r[3]);
        b[i] = make_float2(r[4], r[5]);
    }
    float4 *d_a = nullptr, *d_hit = nullptr;
    float2 *d_b = nullptr;
    uint32_t *d_cnt = nullptr, *d_hi = nullptr;
    pt_hit *d_out = nullptr;
    const std::vector<pt_buf> set = { pt_buf_of(d_a, sizeof(float4) * n), pt_buf_of(d_b, sizeof(float2) * n), pt_buf_of(d_hit, sizeof(float4) * n),
                                      pt_buf_of(d_out, sizeof(pt_hit) * n), pt_buf_of(d_cnt, sizeof(uint32_t) * 2), pt_buf_of(d_hi, sizeof(uint32_t) * n) };
    PT_TRY(pt_scratch_alloc(ctx, "the ray and hit buffers of pt_trace", set, nullptr, 0));
    pt_status ret = PT_OK;
    (void)hipMemcpyAsync(d_a, a.data(), sizeof(float4) * n, hipMemcpyHostToDevice, st);
    (void)hipMemcpyAsync(d_b, b.data(), sizeof(float2) * n, hipMemcpyHostToDevice, st);
    const uint32_t cnt_head[2] = { n, 0u };
    (void)hipMemcpyAsync(d_cnt, cnt_head, sizeof(cnt_head), hipMemcpyHostToDevice, st);
    (void)hipEventRecord(ctx->ev_a, st);
    ptw_launch_extend(pl, s, d_a, d_b, d_hit, d_hi, d_cnt, nullptr, ctx->d_stats, tmin, tmax, false, false, st);
    (void)hipEventRecord(ctx->ev_b, st);
    ptw_launch_hits_to_api(d_hit, pl.bvh8 ? s->d_tri4_8 : s->d_tri4, s->n_inst ? d_hi : nullptr, s->d_tlas_prim_of, n, d_out, st);
    (void)hipMemcpyAsync(hits, d_out, sizeof(pt_hit) * n, hipMemcpyDeviceToHost, st);
    hipError_t e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { ctx->err = std::string("pt_trace: ") + hipGetErrorString(e); ret = PT_ERR_HIP; }
    float ms = 0.f;
    if (ret == PT_OK && hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b) == hipSuccess) ctx->stats.ms_extend += ms;
    ctx->stats.launches_extend++;
    pt_scratch_free(set, nullptr, 0);
    return ret;
}
