// radiance_device.hip -- pt_radiance_device: path-traced radiance for rays in caller-owned device buffers.
//
// In the wavefront pipeline only k_generate (the camera ray) and k_resolve (the film) know about pixels.  With one sample per slot -- rc.spp = 1,
// one group of one sample -- k_shade never regenerates a slot from the camera, so k_shade, k_shadow_add and every extend kernel run a path that
// began anywhere, as they are.  Per chunk of m rays, m * spp slots laid out sample-major (slot = s * m + r):
//   k_radiance_generate  rows of d_rays6 (+ d_seeds or the hashed seed) -> queue 0 records, the slots' accumulators zeroed, the count words
//   max_depth rounds     ptw_launch_extend (the kernel pt_trace would take for the scene and desc.extend, raw hit records, the context's ray
//                        counter) + ptw_launch_shade; PT_RADIANCE_NEE and a scene with emitters: + the shadow-ray extend + ptw_launch_shadow_add;
//                        the two queues alternate as in render.hip's pipe_round.  One pipeline, the context's stream, nothing polled.
//   k_radiance_resolve   the slots' accumulators summed in sample order, / spp, stored or blended into d_radiance (and d_moment2)
// through a workspace that belongs to the context and only grows.  The per-lane bodies are radiance_device_kernel.h (compiled for the host by
// tests/radiance_device_host.cpp).  No LDS, no scratch.
// PT_RADIANCE_FUSED / PT_RADIANCE_AUTO, for scenes of the fused pipeline's single-level class: per chunk the slot counters zeroed, ONE launch of the
// fused kernel started from the caller's rays (fused_rays.hip; fused_kernel.h RAYS) and the same k_radiance_resolve, through a workspace of its
// own: 16 B per slot.
#include "wavefront_host.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "radiance_device_kernel.h"

namespace {
using namespace ptw;

// one thread per ray of the chunk, blockIdx.y = the sample; thread 0 of sample 0 also writes the count words the first round reads
__global__ __launch_bounds__(TB) void k_radiance_generate(const float *__restrict__ rays6, const uint32_t *__restrict__ seeds, RdCall c, uint64_t first,
                                                          uint32_t m, float4 *__restrict__ color, QueueView out, uint32_t *__restrict__ count)
{
    const uint32_t r = blockIdx.x * TB + threadIdx.x, s = blockIdx.y;
    if (r == 0u && s == 0u) { count[0] = m * c.spp; count[1] = 0u; }
    if (r >= m) return;
    rd_generate(rays6, seeds, c, first, r, s, m, color, out.id, out.state, out.rayA, out.rayB);
}

__global__ __launch_bounds__(TB) void k_radiance_resolve(const float4 *__restrict__ color, RdCall c, uint32_t m, float *__restrict__ radiance,
                                                         float *__restrict__ moment2)
{
    const uint32_t r = blockIdx.x * TB + threadIdx.x;
    if (r >= m) return;
    rd_resolve(color, c, r, m, radiance, moment2);
}

constexpr uint64_t RD_MAX_SLOTS = 1ull << 30;  // the queues are indexed in 32 bits

std::vector<pt_buf> slot_set(pt_ctx::Radiance &w, size_t n)
{
    std::vector<pt_buf> set;
    for (int i = 0; i < 2; i++) {
        set.push_back(pt_buf_of(w.d_qid[i], sizeof(uint2) * n));
        set.push_back(pt_buf_of(w.d_qstate[i], sizeof(float4) * n));
        set.push_back(pt_buf_of(w.d_qrayA[i], sizeof(float4) * n));
        set.push_back(pt_buf_of(w.d_qrayB[i], sizeof(float2) * n));
    }
    set.push_back(pt_buf_of(w.d_hit, sizeof(float4) * n));
    set.push_back(pt_buf_of(w.d_hit_inst, sizeof(uint32_t) * n));
    set.push_back(pt_buf_of(w.d_color, sizeof(float4) * n));
    set.push_back(pt_buf_of(w.d_count, sizeof(uint32_t) * 4));
    set.push_back(pt_buf_of(w.d_tiles, sizeof(uint32_t)));
    return set;
}
std::vector<pt_buf> shadow_set(pt_ctx::Radiance &w, size_t n)
{
    return { pt_buf_of(w.d_sq_rayA, sizeof(float4) * n), pt_buf_of(w.d_sq_rayB, sizeof(float2) * n), pt_buf_of(w.d_sq_contrib, sizeof(float4) * n),
             pt_buf_of(w.d_sq_hit, sizeof(float4) * n), pt_buf_of(w.d_sq_tmax, sizeof(float) * n), pt_buf_of(w.d_sq_slot, sizeof(uint32_t) * n) };
}

// the workspace holds at least `slots` slots afterwards, with the shadow queue if `nee` (PT_ERR_OOM: not within the budget / the device; the set
// that did not fit is then empty)
pt_status ensure_radiance(pt_ctx *ctx, size_t slots, bool nee)
{
    pt_ctx::Radiance &w = ctx->rd;
    const char *hint = ": a smaller chunk_rays fits";
    if (slots > w.cap) {
        const size_t held = w.bytes;
        w.cap = 0;
        PT_TRY(pt_scratch_alloc(ctx, "pt_radiance_device workspace", slot_set(w, slots), &w.bytes, held, w.sq_bytes + w.f_bytes, ctx->mem_budget, hint));
        w.cap = slots;
        // k_shade finds a slot's pixel through a tile list (slot_pixel reads tiles[local >> 6]) before it asks whether the slot has another sample.
        // These slots have no pixel and never another sample: with slots_per_lane = 64 every slot reads word 0 of this one-word list, zeroed here.
        PT_HIP(ctx, hipMemsetAsync(w.d_tiles, 0, sizeof(uint32_t), ctx->stream));
    }
    if (nee && slots > w.cap_sq) {  // at most one shadow ray per live path and round
        const size_t held = w.sq_bytes;
        w.cap_sq = 0;
        PT_TRY(pt_scratch_alloc(ctx, "pt_radiance_device shadow queue", shadow_set(w, slots), &w.sq_bytes, held, w.bytes + w.f_bytes, ctx->mem_budget, hint));
        w.cap_sq = slots;
    }
    return PT_OK;
}

// ---- PT_RADIANCE_FUSED: the single-kernel form ---------------------------------------------------------------------------------------------------
std::vector<pt_buf> fused_set(pt_ctx::Radiance &w, size_t n)
{
    return { pt_buf_of(w.d_fcolor, sizeof(float4) * n), pt_buf_of(w.d_fcount, PTW_FUSED_COUNT_BYTES) };
}
// the single-kernel form's workspace holds at least `slots` accumulators afterwards: 16 B per slot + PTW_FUSED_COUNT_BYTES (PT_ERR_OOM: the set is empty)
pt_status ensure_radiance_fused(pt_ctx *ctx, size_t slots)
{
    pt_ctx::Radiance &w = ctx->rd;
    if (slots <= w.cap_f) return PT_OK;
    const size_t held = w.f_bytes;
    w.cap_f = 0;
    PT_TRY(pt_scratch_alloc(ctx, "pt_radiance_device workspace (single-kernel form)", fused_set(w, slots), &w.f_bytes, held, w.bytes + w.sq_bytes, ctx->mem_budget,
                            ": a smaller chunk_rays fits"));
    w.cap_f = slots;
    return PT_OK;
}
// What PT_RADIANCE_AUTO takes where the single-kernel form applies, per estimator: the form that won DESIGN.md section 25's measurements on every
// shape of the class by more than the wavefront form's own spread, on both clocks
// (profiles/radiance_fused_probe.json: camera rays, incoherent rays and a small call, both estimators -- the fused form won all six)
constexpr bool RD_AUTO_TAKES_FUSED[2] = { true, true };  // { plain, PT_RADIANCE_NEE }

// Does the single-kernel form apply?  The rule is ptw_plan_fused's single-level class, with the extend variant left to the library.  PT_OK: fp is the
// launch plan.  PT_ERR_UNSUPPORTED: ctx->err names the class.
pt_status plan_radiance_fused(pt_scene *s, const pt_radiance_desc *d, const ExtendPlan &pl, bool nee, FusedPlan &fp)
{
    pt_ctx *ctx = s->ctx;
    if (s->n_inst) {
        ctx->err = "PT_RADIANCE_FUSED is for single-level scenes whose BVH4, triangles and shading tables fit LDS: instanced scenes run the wavefront form";
        return PT_ERR_UNSUPPORTED;
    }
    if (d->extend != PT_EXTEND_AUTO) {
        ctx->err = "PT_RADIANCE_FUSED walks the scene in LDS: pt_radiance_desc.extend must be PT_EXTEND_AUTO";
        return PT_ERR_UNSUPPORTED;
    }
    const pt_status rc = ptw_plan_fused(s, pl, d->tmin, fp, nee);
    if (rc == PT_ERR_UNSUPPORTED) ctx->err = "PT_RADIANCE_FUSED runs PT_PIPELINE_FUSED's kernel: " + ctx->err;
    return rc;
}

// the chunks of a call through the fused kernel (its workspace holds a chunk): per chunk the counters zeroed, ONE launch that carries every path to
// its end, the resolve
pt_status radiance_fused(pt_scene *s, const pt_radiance_desc *d, uint64_t n, uint64_t chunk, const ExtendPlan &pl, const FusedPlan &fp, float *device_ms)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t spp = d->spp;
    pt_ctx::Radiance &w = ctx->rd;
    // what the kernel takes per launch: one sample per slot, no pixels, no cull, one group, no tail
    RenderConst rc{};
    for (int k = 0; k < 3; k++) rc.env[k] = d->env[k];
    rc.tmin = d->tmin; rc.tmax = d->tmax;
    rc.width = rc.height = rc.tiles_x = 1u;
    rc.spp = 1u; rc.max_depth = d->max_depth;
    rc.frame_base = 0; rc.lanes_active = 1u;
    rc.slots_per_lane = 64u;
    rc.groups = 1u; rc.group_size = 1u;
    rc.div_spl.init(64u); rc.div_groups.init(1u); rc.div_tail.init(1u);
    rc.cull_on = 0u; rc.tail = 0u;
    Radiance rad{};
    rad.color = w.d_fcolor;
    const RdCall call = { d->spp, d->frame, d->index_base, (d->flags & PT_RADIANCE_ACCUMULATE) ? 1u : 0u };
    const float *rays6 = static_cast<const float *>(d->d_rays6);
    const uint32_t *seeds = static_cast<const uint32_t *>(d->d_seeds);
    float *radiance = static_cast<float *>(d->d_radiance), *moment2 = static_cast<float *>(d->d_moment2);

    if (device_ms) *device_ms = 0.f;
    PT_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    for (uint64_t c = 0; c < n_chunks; c++) {
        const uint64_t off = c * chunk;
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - off);
        rc.n_slots = m * d->spp;  // the live slots (<= 2^30); the launch hands out this rounded up to 64
        const RdRays rr = rdf_rays(rays6 + 6 * off, seeds ? seeds + off * spp : nullptr, call, off, m);
        PT_HIP(ctx, hipMemsetAsync(w.d_fcount, 0, PTW_FUSED_COUNT_BYTES, st));
        PT_TRY(ptw_launch_fused_rays(fp, rc, rad, s, w.d_fcount, ctx->d_stats, d->tmin, d->tmax, rr.rays6, rr.seeds, rr.m, rr.spp, rr.index0, rr.seed_m0, st));
        PT_HIP(ctx, hipGetLastError());  // a launch the runtime refused (LDS size, grid) must not pass for a traced chunk
        ctx->stats.launches_extend++;
        ctx->stats.rounds++;
        k_radiance_resolve<<<(m + TB - 1) / TB, TB, 0, st>>>(w.d_fcolor, call, m, radiance + 3 * off, moment2 ? moment2 + 3 * off : nullptr);
        ctx->stats.launches_other++;
    }
    ctx->stats.paths += n * spp;
    ctx->stats.extend_variant = pl.variant;
    ctx->stats.pipeline = PT_PIPELINE_FUSED;
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    if (device_ms) PT_HIP(ctx, hipEventElapsedTime(device_ms, ctx->ev_a, ctx->ev_b));
    return PT_OK;
}

}  // namespace

void ptr_free(pt_ctx *ctx)
{
    pt_ctx::Radiance &w = ctx->rd;
    pt_scratch_free(slot_set(w, 0), &w.bytes, w.bytes);
    pt_scratch_free(shadow_set(w, 0), &w.sq_bytes, w.sq_bytes);
    pt_scratch_free(fused_set(w, 0), &w.f_bytes, w.f_bytes);
    w.cap = w.cap_sq = w.cap_f = 0;
}

pt_status ptr_radiance_device(pt_scene *s, const pt_radiance_desc *d, uint64_t n, float *device_ms)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    // ---- refusals: nothing launched, nothing written
    if (d->flags & ~(uint32_t)(PT_RADIANCE_NEE | PT_RADIANCE_ACCUMULATE | PT_RADIANCE_FUSED | PT_RADIANCE_AUTO)) return pt_bad(ctx, "pt_radiance_desc.flags has bits other than PT_RADIANCE_NEE, _ACCUMULATE, _FUSED and _AUTO");
    const uint32_t form = d->flags & (uint32_t)(PT_RADIANCE_FUSED | PT_RADIANCE_AUTO);
    if (form == (uint32_t)(PT_RADIANCE_FUSED | PT_RADIANCE_AUTO)) return pt_bad(ctx, "pt_radiance_desc.flags: PT_RADIANCE_FUSED and PT_RADIANCE_AUTO exclude each other");
    PT_TRY(pt_check_reserved(ctx, "pt_radiance_desc", d->reserved));
    if (!(std::isfinite(d->tmin) && std::isfinite(d->tmax) && d->tmax > d->tmin)) return pt_bad(ctx, "pt_radiance_desc: tmin and tmax must be finite, tmin < tmax");
    if (!pt_finite3(d->env)) return pt_bad(ctx, "pt_radiance_desc.env must be finite");
    if (d->spp < 1u || d->spp > 65535u || d->max_depth < 1u || d->max_depth > 65535u) return pt_bad(ctx, "pt_radiance_desc: spp and max_depth must be in 1..65535");
    const bool nee = (d->flags & PT_RADIANCE_NEE) != 0, accumulate = (d->flags & PT_RADIANCE_ACCUMULATE) != 0;
    if (accumulate && d->frame < 0) return pt_bad(ctx, "PT_RADIANCE_ACCUMULATE blends by the frame index: frame must be >= 0");
    if (n && !d->d_rays6) return pt_bad(ctx, "pt_radiance_desc.d_rays6 is NULL");
    if (n && !d->d_radiance) return pt_bad(ctx, "pt_radiance_desc.d_radiance is NULL");
    if (d->extend > PT_EXTEND_HBM8) return pt_bad(ctx, "unknown extend variant");
    if (d->extend == PT_EXTEND_FLAT_REMOVED) {
        ctx->err = "PT_EXTEND_FLAT (the brute-force loop, never AUTO) was removed in API version 5: every tree walk returns the brute-force closest hit";
        return PT_ERR_UNSUPPORTED;
    }
    if (n == 0) { if (device_ms) *device_ms = 0.f; return PT_OK; }
    ExtendPlan pl;
    PT_TRY(ptw_plan_extend(s, d->extend, pl));  // (repairs a scene that lost its trees; builds the 8-wide tree on first request)
    // the form: the single-kernel one where PT_RADIANCE_FUSED asks for it (or refuses), or where PT_RADIANCE_AUTO finds it applies and measured faster
    FusedPlan fp;
    bool fused = false;
    if (form) {
        const std::string err_before = ctx->err;
        const pt_status rcf = plan_radiance_fused(s, d, pl, nee, fp);
        if (rcf != PT_OK && !(rcf == PT_ERR_UNSUPPORTED && form == PT_RADIANCE_AUTO)) return rcf;
        if (rcf != PT_OK) ctx->err = err_before;  // (AUTO: not an error)
        fused = rcf == PT_OK && (form == PT_RADIANCE_FUSED || RD_AUTO_TAKES_FUSED[nee ? 1 : 0]);
    }
    ShadeLaunch sl;
    PT_TRY(ptw_shade_inst_frames(s, pl, sl.inst_frame));
    PT_TRY(ptw_nee_lights(s, nee, sl.lights, sl.n_lights, sl.light_area));
    ptw_shade_shape(ctx, s, pl, sl.grid, sl.smem, sl.lds_tables);
    const bool shadows = nee && sl.n_lights != 0;

    // the chunk: rays per pass, a multiple of 64, no more than the rays there are, no more than 2^30 slots
    const uint64_t spp = d->spp;
    const auto up64 = [](uint64_t v) { return (v + 63u) & ~(uint64_t)63; };
    const uint64_t want = d->chunk_rays ? d->chunk_rays : std::max<uint64_t>(64, PT_RADIANCE_DEFAULT_CHUNK_SLOTS / spp);
    const uint64_t most = std::max<uint64_t>(64, (RD_MAX_SLOTS / spp) & ~(uint64_t)63);
    const uint64_t chunk = std::min(std::min(up64(want), most), up64(std::min(n, most)));
    if (fused) {
        const std::string err_before = ctx->err;
        const pt_status rce = ensure_radiance_fused(ctx, (size_t)(chunk * spp));
        if (rce == PT_OK) return radiance_fused(s, d, n, chunk, pl, fp, device_ms);
        // (PT_RADIANCE_AUTO is never an error the call would not be without it: the wavefront form's set may be there already, or fit where this did not)
        if (!(rce == PT_ERR_OOM && form == PT_RADIANCE_AUTO)) return rce;
        ctx->err = err_before;
    }
    PT_TRY(ensure_radiance(ctx, (size_t)(chunk * spp), nee));
    pt_ctx::Radiance &w = ctx->rd;

    // what k_shade and k_shadow_add take per call: one sample per slot, no pixels, no cull, no term logs
    RenderConst rc{};
    for (int k = 0; k < 3; k++) rc.env[k] = d->env[k];
    rc.tmin = d->tmin; rc.tmax = d->tmax;
    rc.width = rc.height = rc.tiles_x = 1u;
    rc.spp = 1u; rc.max_depth = d->max_depth;
    rc.frame_base = 0; rc.lanes_active = 1u;
    rc.slots_per_lane = 64u;
    rc.groups = 1u; rc.group_size = 1u;
    rc.div_spl.init(64u); rc.div_groups.init(1u); rc.div_tail.init(1u);
    rc.cull_on = 0u; rc.tail = 0u;
    sl.tiles = w.d_tiles; sl.scene = s; sl.bvh8 = pl.bvh8; sl.nee = nee;
    sl.rad = Radiance{};
    sl.rad.color = w.d_color;
    sl.hit = w.d_hit; sl.hit_inst = w.d_hit_inst;
    if (nee) {
        sl.sq = { w.d_sq_rayA, w.d_sq_rayB, w.d_sq_contrib, w.d_sq_tmax, w.d_sq_slot };
        sl.sq_count = w.d_count + 2;
    }
    const QueueView qv[2] = { { w.d_qid[0], w.d_qstate[0], w.d_qrayA[0], w.d_qrayB[0] }, { w.d_qid[1], w.d_qstate[1], w.d_qrayA[1], w.d_qrayB[1] } };
    const RdCall call = { d->spp, d->frame, d->index_base, accumulate ? 1u : 0u };
    const float *rays6 = static_cast<const float *>(d->d_rays6);
    const uint32_t *seeds = static_cast<const uint32_t *>(d->d_seeds);
    float *radiance = static_cast<float *>(d->d_radiance), *moment2 = static_cast<float *>(d->d_moment2);

    if (device_ms) *device_ms = 0.f;
    PT_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    for (uint64_t c = 0; c < n_chunks; c++) {
        const uint64_t off = c * chunk;
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - off);
        const uint32_t grid = (m + TB - 1) / TB;
        rc.n_slots = m * d->spp;
        sl.rc = rc;
        k_radiance_generate<<<dim3(grid, d->spp), TB, 0, st>>>(rays6 + 6 * off, seeds ? seeds + off * spp : nullptr, call, off, m, w.d_color, qv[0], w.d_count);
        ctx->stats.launches_other++;
        int cur = 0;
        for (uint32_t round = 0; round < d->max_depth; round++) {
            ptw_launch_extend(pl, s, qv[cur].rayA, qv[cur].rayB, w.d_hit, w.d_hit_inst, &w.d_count[cur], &w.d_count[cur ^ 1], ctx->d_stats, d->tmin, d->tmax,
                              false, true, st);
            sl.in = qv[cur]; sl.out = qv[cur ^ 1]; sl.count_in = &w.d_count[cur]; sl.count_out = &w.d_count[cur ^ 1];
            if (nee) PT_HIP(ctx, hipMemsetAsync(sl.sq_count, 0, sizeof(uint32_t), st));
            ptw_launch_shade(sl, st, nullptr, nullptr);
            if (shadows) {
                // the shadow rays of this round: any-hit queries with their own tmax, then the unoccluded terms
                ptw_launch_extend(pl, s, sl.sq.rayA, sl.sq.rayB, w.d_sq_hit, nullptr, sl.sq_count, nullptr, ctx->d_stats, d->tmin, d->tmax, false, true, st, 0,
                                  nullptr, nullptr, nullptr, sl.sq.tmax);
                ptw_launch_shadow_add(rc, sl.rad, w.d_sq_hit, sl.sq.contrib, sl.sq.slot, sl.sq_count, sl.grid, st);
                ctx->stats.launches_extend++;
                ctx->stats.launches_other++;
            }
            PT_HIP(ctx, hipGetLastError());  // a launch the runtime refused (LDS size, grid) must not pass for a traced round
            ctx->stats.launches_extend++;
            ctx->stats.launches_shade++;
            ctx->stats.rounds++;
            cur ^= 1;
        }
        k_radiance_resolve<<<grid, TB, 0, st>>>(w.d_color, call, m, radiance + 3 * off, moment2 ? moment2 + 3 * off : nullptr);
        ctx->stats.launches_other++;
    }
    ctx->stats.paths += n * spp;
    ctx->stats.extend_variant = pl.variant;
    if (form) ctx->stats.pipeline = nee ? PT_PIPELINE_WAVEFRONT_NEE : PT_PIPELINE_WAVEFRONT;  // (PT_RADIANCE_AUTO: the form that ran)
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    if (device_ms) PT_HIP(ctx, hipEventElapsedTime(device_ms, ctx->ev_a, ctx->ev_b));
    return PT_OK;
}
