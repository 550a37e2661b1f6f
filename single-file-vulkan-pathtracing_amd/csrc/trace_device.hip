// trace_device.hip -- pt_trace_device: ray queries on caller-owned device buffers (closest hit, any hit, the surface at the hit).
//
// pt_trace repacks its rays on the host, allocates six buffers per call and copies both ways.  Here the rays stay on the device:
//   k_trace_pack       rows of d_rays6 -> the extend kernels' queue (rayA float4, rayB float2), the any-hit bound plane, the chunk's count word
//   ptw_launch_extend  the kernel pt_trace would take for the scene and desc.extend -- its closest-hit instantiation, or, for PT_TRACE_ANY,
//                      its any-hit one (ray_tmax non-null: the NEE pipeline's shadow-ray kernels)
//   k_hits_to_api      (shade_kernels.hip, as pt_trace launches it) hit records -> d_hits
//   k_trace_surface    hit records -> position / normal / albedo / emission, gathered as k_aov_reduce gathers them
//   k_trace_occluded   hit records -> one byte per ray
// one chunk of desc.chunk_rays after the other on the context's stream, through a workspace that belongs to the context and only grows.
// The per-lane bodies are trace_device_kernel.h (compiled for the host by tests/trace_device_host.cpp).  No LDS, no scratch.
// PT_TRACE_FUSED / PT_TRACE_AUTO: where the scene is of the compact LDS kernel's class the rays of a launch go through ONE kernel instead
// (trace_fused.hip), with no workspace; this unit has the class test, PT_TRACE_AUTO's table and the launch loop (trace_fused below).
#include "wavefront_host.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#define TD_LOADS_DONE() __builtin_amdgcn_s_waitcnt(0x0F70)   // s_waitcnt vmcnt(0): the other counters at their maxima (gfx9 encoding)
#define TD_LD4(p) ptm::ld_stream<true>(p)
#include "trace_device_kernel.h"

namespace {

// one thread per ray of the chunk; thread 0 also writes the count word the extend kernel reads
__global__ __launch_bounds__(TB) void k_trace_pack(const float *__restrict__ rays6, const float *__restrict__ d_tmax, float tmax, uint32_t n,
                                                   float4 *__restrict__ rayA, float2 *__restrict__ rayB, float *__restrict__ bound,
                                                   uint32_t *__restrict__ count)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i == 0u) { count[0] = n; count[1] = 0u; }
    if (i >= n) return;
    td_pack(rays6, d_tmax, tmax, i, rayA, rayB, bound);
}

__global__ __launch_bounds__(TB) void k_trace_occluded(const float4 *__restrict__ hit, uint32_t n, uint8_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    out[i] = td_occluded(hit, i);
}

template <bool INST, bool FRAMES>
__global__ __launch_bounds__(TB) void k_trace_surface(TdScene sc, const float4 *__restrict__ hit, const uint32_t *__restrict__ hit_inst, uint32_t n,
                                                      TdPlanes pl)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    td_surface<INST, FRAMES>(sc, hit, hit_inst, pl, i);
}

constexpr uint64_t TD_MAX_CHUNK = 1ull << 30;  // the queues are indexed in 32 bits

std::vector<pt_buf> trace_set(pt_ctx::Trace &t, size_t rays)
{
    return { pt_buf_of(t.d_rayA, sizeof(float4) * rays), pt_buf_of(t.d_rayB, sizeof(float2) * rays), pt_buf_of(t.d_hit, sizeof(float4) * rays),
             pt_buf_of(t.d_hit_inst, sizeof(uint32_t) * rays), pt_buf_of(t.d_bound, sizeof(float) * rays), pt_buf_of(t.d_count, sizeof(uint32_t) * 2) };
}

// the workspace holds at least `rays` rays afterwards (PT_ERR_OOM: not within the budget / the device; the context then holds none)
pt_status ensure_trace(pt_ctx *ctx, size_t rays)
{
    pt_ctx::Trace &t = ctx->tr;
    if (rays <= t.cap) return PT_OK;
    const size_t held = t.bytes;
    t.cap = 0;
    const pt_status rc = pt_scratch_alloc(ctx, "pt_trace_device workspace", trace_set(t, rays), &t.bytes, held, 0, ctx->mem_budget, ": a smaller chunk_rays fits");
    if (rc == PT_OK) t.cap = rays;
    return rc;
}

// What PT_TRACE_AUTO takes where the single-kernel form applies, per kind of query { PT_TF_HITS, PT_TF_SURFACE, PT_TF_ANY }: the single-kernel form
// only where its max lay below the parent build's min on EVERY measured shape of that kind (profiles/trace_fused_probe.json:
// 2^20 and 2^24 rays, coherent and shuffled -- it did on all four shapes of all three kinds, by 1.36x .. 2.10x, 1.20x .. 1.98x and 1.45x .. 2.29x)
constexpr bool TD_AUTO_TAKES_FUSED[3] = { true, true, true };

// Does the single-kernel form apply?  The class is the compact LDS kernel's (k_extend_lds7 / _lds7p) with the variant left to the library.
// -> null, or what keeps the call out of the class
const char *trace_fused_refusal(const pt_scene *s, const pt_trace_desc *d, const ExtendPlan &pl)
{
    if (s->n_inst) return "the scene is instanced";
    if (d->extend != PT_EXTEND_AUTO) return "pt_trace_desc.extend names a kernel (it must be PT_EXTEND_AUTO)";
    if (!(pl.lds_scene && !pl.spill)) return "the scene is beyond the compact LDS kernel (24 KB of nodes and triangles, 2047 triangles, 16 stack entries)";
    if (!(d->tmin > 0.f)) return "tmin <= 0 (one-dword stack entries order like their distances for positive ones only)";
    return nullptr;
}

// the launches of a call through k_trace_fused: one per 2^30 rays, straight from the caller's rows to the caller's records
pt_status trace_fused(pt_scene *s, const pt_trace_desc *d, uint64_t n, const ExtendPlan &pl, const TraceFusedPlan &tp, float *device_ms)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    if (device_ms) *device_ms = 0.f;
    const uint64_t n_launches = (n + TD_MAX_CHUNK - 1) / TD_MAX_CHUNK;
    const bool async = (d->flags & PT_TRACE_ASYNC) != 0;
    if (!async) {
        while (ctx->ev_pool.size() < 2 * n_launches) {
            hipEvent_t e = nullptr;
            PT_HIP(ctx, hipEventCreate(&e));
            ctx->ev_pool.push_back(e);
        }
        PT_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    }
    for (uint64_t c = 0; c < n_launches; c++) {
        const uint64_t off = c * TD_MAX_CHUNK;
        const uint32_t m = (uint32_t)std::min<uint64_t>(TD_MAX_CHUNK, n - off);
        const auto plane = [&](void *p) { return p ? static_cast<float *>(p) + 3 * off : nullptr; };
        const TraceFusedIO io = { static_cast<const float *>(d->d_rays6) + 6 * off,
                                  d->d_tmax ? static_cast<const float *>(d->d_tmax) + off : nullptr,
                                  d->d_hits ? static_cast<pt_hit *>(d->d_hits) + off : nullptr,
                                  d->d_occluded ? static_cast<uint8_t *>(d->d_occluded) + off : nullptr,
                                  plane(d->d_position), plane(d->d_normal), plane(d->d_albedo), plane(d->d_emission) };
        ptw_launch_trace_fused(tp, s, io, m, d->tmin, d->tmax, st, async ? nullptr : ctx->ev_pool[2 * c], async ? nullptr : ctx->ev_pool[2 * c + 1]);
    }
    ctx->stats.launches_extend += (uint32_t)n_launches;
    ctx->stats.extend_variant = pl.variant;
    ctx->stats.pipeline = PT_PIPELINE_FUSED;
    PT_HIP(ctx, hipGetLastError());
    if (async) return PT_OK;
    PT_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    if (device_ms) PT_HIP(ctx, hipEventElapsedTime(device_ms, ctx->ev_a, ctx->ev_b));
    for (uint64_t c = 0; c < n_launches; c++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev_pool[2 * c], ctx->ev_pool[2 * c + 1]) == hipSuccess) ctx->stats.ms_extend += ms;
    }
    return PT_OK;
}

}  // namespace

void ptt_free(pt_ctx *ctx)
{
    pt_scratch_free(trace_set(ctx->tr, 0), &ctx->tr.bytes, ctx->tr.bytes);
    ctx->tr.cap = 0;
}

pt_status ptt_trace_device(pt_scene *s, const pt_trace_desc *d, uint64_t n, float *device_ms)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    // ---- refusals: nothing launched, nothing written
    if (d->mode > PT_TRACE_ANY) return pt_bad(ctx, "pt_trace_desc.mode is neither PT_TRACE_CLOSEST nor PT_TRACE_ANY");
    if (d->flags & ~(uint32_t)(PT_TRACE_ASYNC | PT_TRACE_FUSED | PT_TRACE_AUTO)) return pt_bad(ctx, "pt_trace_desc.flags has bits other than PT_TRACE_ASYNC, _FUSED and _AUTO");
    const uint32_t form = d->flags & (uint32_t)(PT_TRACE_FUSED | PT_TRACE_AUTO);
    if (form == (uint32_t)(PT_TRACE_FUSED | PT_TRACE_AUTO)) return pt_bad(ctx, "pt_trace_desc.flags: PT_TRACE_FUSED and PT_TRACE_AUTO exclude each other");
    PT_TRY(pt_check_reserved(ctx, "pt_trace_desc", d->reserved));
    if (!(std::isfinite(d->tmin) && std::isfinite(d->tmax) && d->tmax > d->tmin)) return pt_bad(ctx, "pt_trace_desc: tmin and tmax must be finite, tmin < tmax");
    const bool any = d->mode == PT_TRACE_ANY;
    const bool surface = d->d_position || d->d_normal || d->d_albedo || d->d_emission;
    if (any) {
        if (d->d_hits || surface) return pt_bad(ctx, "PT_TRACE_ANY writes d_occluded only: d_hits and the surface pointers must be NULL");
        if (!d->d_occluded) return pt_bad(ctx, "PT_TRACE_ANY: d_occluded is NULL");
    } else {
        if (d->d_occluded) return pt_bad(ctx, "PT_TRACE_CLOSEST: d_occluded must be NULL (PT_TRACE_ANY writes it)");
        if (!d->d_hits && !surface) return pt_bad(ctx, "PT_TRACE_CLOSEST: d_hits and all four surface pointers are NULL");
    }
    if (n && !d->d_rays6) return pt_bad(ctx, "pt_trace_desc.d_rays6 is NULL");
    if (d->extend > PT_EXTEND_HBM8) return pt_bad(ctx, "unknown extend variant");
    if (!any && d->d_tmax) {
        ctx->err = "PT_TRACE_CLOSEST takes no per-ray bound: the kernels' ray_tmax belongs to their any-hit instantiations (d_tmax must be NULL)";
        return PT_ERR_UNSUPPORTED;
    }
    if (d->extend == PT_EXTEND_FLAT_REMOVED) {
        ctx->err = "PT_EXTEND_FLAT (the brute-force loop, never AUTO) was removed in API version 5: every tree walk returns the brute-force closest hit";
        return PT_ERR_UNSUPPORTED;
    }
    if (n == 0) { if (device_ms) *device_ms = 0.f; return PT_OK; }
    ExtendPlan pl;
    PT_TRY(ptw_plan_extend(s, d->extend, pl));  // (repairs a scene that lost its trees; builds the 8-wide tree on first request)
    // the form: the single-kernel one where PT_TRACE_FUSED asks for it (or refuses), or where PT_TRACE_AUTO finds it applies and measured faster
    if (form) {
        const int kind = any ? PT_TF_ANY : surface ? PT_TF_SURFACE : PT_TF_HITS;
        const char *why = trace_fused_refusal(s, d, pl);
        if (why && form == PT_TRACE_FUSED) {
            ctx->err = std::string("PT_TRACE_FUSED is for single-level scenes that the compact LDS kernel walks (PT_EXTEND_AUTO, tmin > 0): ") + why;
            return PT_ERR_UNSUPPORTED;
        }
        if (!why && (form == PT_TRACE_FUSED || TD_AUTO_TAKES_FUSED[kind])) {
            TraceFusedPlan tp;
            PT_TRY(ptw_plan_trace_fused(s, pl, kind, tp));
            return trace_fused(s, d, n, pl, tp, device_ms);
        }
    }
    const float4 *inst_frame = nullptr;
    if (surface && s->n_inst && ctx->tune.inst_frames != 0) {  // the table k_shade<INST> and k_aov_reduce<INST> read, when the context uses it
        PT_TRY(ptb_ensure_inst_frames(s));
        inst_frame = s->d_inst_frame;
    }
    const uint64_t want = d->chunk_rays ? d->chunk_rays : PT_TRACE_DEFAULT_CHUNK_RAYS;
    const uint64_t chunk = std::min(std::min<uint64_t>((want + 63u) & ~(uint64_t)63, TD_MAX_CHUNK), n > TD_MAX_CHUNK ? TD_MAX_CHUNK : (n + 63u) & ~(uint64_t)63);
    PT_TRY(ensure_trace(ctx, (size_t)chunk));
    if (device_ms) *device_ms = 0.f;
    const uint64_t n_chunks = (n + chunk - 1) / chunk;
    const bool async = (d->flags & PT_TRACE_ASYNC) != 0;
    // blocking calls: the extend kernels' own start / stop stamps, a pair per chunk (render.hip's pool of events)
    if (!async) {
        while (ctx->ev_pool.size() < 2 * n_chunks) {
            hipEvent_t e = nullptr;
            PT_HIP(ctx, hipEventCreate(&e));
            ctx->ev_pool.push_back(e);
        }
        PT_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    }
    pt_ctx::Trace &t = ctx->tr;
    const float *rays6 = static_cast<const float *>(d->d_rays6), *tmax_in = static_cast<const float *>(d->d_tmax);
    const float4 *tri4 = pl.bvh8 ? s->d_tri4_8 : s->d_tri4;
    const TdScene sc = { tri4, pl.bvh8 ? s->d_shade64_8 : s->d_shade64, s->d_faces, s->d_inst6, inst_frame, s->n_tris };
    uint32_t others = 0;
    for (uint64_t c = 0; c < n_chunks; c++) {
        const uint64_t off = c * chunk;
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n - off);
        const uint32_t grid = (m + TB - 1) / TB;
        k_trace_pack<<<grid, TB, 0, st>>>(rays6 + 6 * off, tmax_in ? tmax_in + off : nullptr, d->tmax, m, t.d_rayA, t.d_rayB, any ? t.d_bound : nullptr, t.d_count);
        hipEvent_t e0 = async ? nullptr : ctx->ev_pool[2 * c], e1 = async ? nullptr : ctx->ev_pool[2 * c + 1];
        // (stats = null, as pt_render_aov's queue form passes it: the extend kernels would add the chunk to pt_stats.rays, which counts a render's rays)
        ptw_launch_extend(pl, s, t.d_rayA, t.d_rayB, t.d_hit, any ? nullptr : t.d_hit_inst, t.d_count, nullptr, nullptr, d->tmin, d->tmax, false, false, st, 0,
                          e0, e1, nullptr, any ? t.d_bound : nullptr);
        others++;
        if (any) {
            k_trace_occluded<<<grid, TB, 0, st>>>(t.d_hit, m, static_cast<uint8_t *>(d->d_occluded) + off);
            others++;
        }
        if (d->d_hits) {
            ptw_launch_hits_to_api(t.d_hit, tri4, s->n_inst ? t.d_hit_inst : nullptr, s->d_tlas_prim_of, m, static_cast<pt_hit *>(d->d_hits) + off, st);
            others++;
        }
        if (surface) {
            const auto plane = [&](void *p) { return p ? static_cast<float *>(p) + 3 * off : nullptr; };
            const TdPlanes planes = { plane(d->d_position), plane(d->d_normal), plane(d->d_albedo), plane(d->d_emission) };
            if (!s->n_inst) k_trace_surface<false, false><<<grid, TB, 0, st>>>(sc, t.d_hit, nullptr, m, planes);
            else if (inst_frame) k_trace_surface<true, true><<<grid, TB, 0, st>>>(sc, t.d_hit, t.d_hit_inst, m, planes);
            else k_trace_surface<true, false><<<grid, TB, 0, st>>>(sc, t.d_hit, t.d_hit_inst, m, planes);
            others++;
        }
    }
    ctx->stats.launches_extend += (uint32_t)n_chunks;
    ctx->stats.launches_other += others;
    if (form) ctx->stats.pipeline = PT_PIPELINE_WAVEFRONT;  // (PT_TRACE_AUTO: the form that ran)
    PT_HIP(ctx, hipGetLastError());
    if (async) return PT_OK;
    PT_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    if (device_ms) PT_HIP(ctx, hipEventElapsedTime(device_ms, ctx->ev_a, ctx->ev_b));
    for (uint64_t c = 0; c < n_chunks; c++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->ev_pool[2 * c], ctx->ev_pool[2 * c + 1]) == hipSuccess) ctx->stats.ms_extend += ms;
    }
    return PT_OK;
}
