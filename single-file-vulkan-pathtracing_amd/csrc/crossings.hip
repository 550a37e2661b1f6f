// crossings.hip -- pt_crossings_device: for every ray of a device array, HOW MANY triangles it crosses inside its range and the signed sum of the
// crossings -- what inside / outside tests, signed distance, thickness and occupancy grids are built from.  ONE persistent kernel per launch: a
// lane reads row i of the caller's rays, walks the scene's BVH4 without ever shrinking its range and writes ray i's two words straight into the
// caller's arrays.  No queues, no records in memory, no workspace (stack entries beyond the LDS share go to the context's spill area).
//
// What defines the result is in crossings_kernel.h (shared with tests/crossings_host.cpp): the triangle test (ptm::ray_setup + ptm::tri_test,
// unchanged), the triangle's own padded box, the slab test, and the lemma "a ray that passes a box passes every box that contains it".  By the
// lemma the walk below counts what a loop over all triangles counts, whatever the tree, the builder, the form or the launch shape.
//
// The tree: s->d_wide (128-B fp32 nodes) and s->d_tri4 (leaf position -> A, B, C and the primitive id), which every single-level scene has.
//
// The walk.  There is no best value to prune by: a node step tests the four slots with cx_slab against the ray's whole range, keeps the first
// that passes in hand and pushes the others in slot order (at most three).  Stack entries are the child word alone, 4 bytes: level
// l < lds_stack in LDS ([level][thread]: a lane's ds_read / write_b32 next to its neighbours', conflict-free, half of k_nearest's bytes), the
// levels above in the spill area ([level][grid thread]).  A pop needs no key test.  A leaf step runs cx_counts over the leaf's triangles.
// Nothing is kept in private memory.
//
// The loop is k_nearest's: a wave-private ray sequence, ballot-ranked refill of idle lanes at the plan's threshold, a node phase that yields to
// waiting leaves, a finished lane writes its two words at once.  A ray that does not walk (cx_live) is handed the empty walk at refill.
//
// Two forms.  LDS: nodes (128-B layout at the 144-B stride, lds_stage_nodes128) and ONE unpermuted copy of tri4 staged from LDS byte 0, the
// stack behind them.  GLOBAL: both through L1 / L2, only the stack in LDS.
#include "wavefront_host.h"

#include <algorithm>
#include <cmath>

#include "lds_scene.h"
#include "crossings_kernel.h"

namespace {

constexpr size_t CX_LDS_LIMIT = 96 * 1024;  // image + stack of PT_CROSSINGS_LDS: the bound PT_EXTEND_LDS and PT_NEAREST_LDS use
// PT_CROSSINGS_AUTO on scenes of the ray kernels' LDS class (lds_class_bytes <= 24 KB): the LDS form only where its slowest measured pass beat
// the GLOBAL form's fastest on every shape measured (NR_AUTO_TAKES_LDS's rule).  Measured on the MI355X (profiles/crossings_probe.json,
// DESIGN.md section 32): on all four box shapes -- 2^20 and 2^24 rays, coherent and shuffled -- the LDS form's slowest pass is below the
// GLOBAL form's fastest (the narrowest: 2^20 coherent, 0.1022 against 0.1059 ms; medians 1.09 .. 1.54x): true.
constexpr bool CX_AUTO_TAKES_LDS = true;
constexpr size_t CX_LDS_CLASS_BYTES = 24 * 1024;

__host__ __device__ constexpr size_t cx_image_bytes(size_t n_wide, size_t n_tris) { return lds_nodes128_bytes(n_wide) + sizeof(float4) * 3 * n_tris; }

struct CrossIO {
    const float *rays6, *points, *tmax_per;  // exactly one of rays6 / points; tmax_per: nullable
    uint32_t *count;                         // nullable
    int32_t *winding;                        // nullable
    float dx, dy, dz;                        // the one direction of `points`
};

template <bool LDS>
__global__ __launch_bounds__(TB) void k_crossings(const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4, uint32_t n_wide, uint32_t n_tris,
                                                  CrossIO io, float tmin, float tmax, float pad, uint32_t n, int refill_min_idle, int lds_stack,
                                                  uint32_t *__restrict__ spill, uint32_t spill_levels)
{
    constexpr uint32_t NODE_F4 = LDS ? LDS_NODE128_F4 : 8u;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const float4 *wide = g_wide, *tri4 = g_tri4;
    uint32_t *s_stack = reinterpret_cast<uint32_t *>(smem);
    if constexpr (LDS) {
        float4 *s_wide = reinterpret_cast<float4 *>(smem);
        float4 *s_tri = s_wide + LDS_NODE128_F4 * (size_t)n_wide;
        lds_stage_nodes128<TB>(s_wide, g_wide, n_wide);
        for (uint32_t i = threadIdx.x; i < 3 * n_tris; i += TB) s_tri[i] = g_tri4[i];
        __syncthreads();
        wide = s_wide;
        tri4 = s_tri;
        s_stack = reinterpret_cast<uint32_t *>(smem + cx_image_bytes(n_wide, n_tris));
    }
    s_stack += threadIdx.x;
    const uint32_t spill_stride = gridDim.x * TB;
    uint32_t *my_spill = spill + (size_t)blockIdx.x * TB + threadIdx.x;

    bool have = false, exhausted = false;
    uint32_t q = 0;
    // wave-private ray sequence: virtual index v -> row (v/64)*wave_stride + wave_base + v%64
    const uint32_t wave_base = (blockIdx.x * (TB / 64) + (threadIdx.x >> 6)) * 64u;
    const uint32_t wave_stride = gridDim.x * TB;
    uint32_t cursor = 0;
    CxRay ray{};
    float bound = 0.f;
    uint32_t count = 0;
    int32_t winding = 0;
    uint32_t cur = SENTINEL;  // a child word of d_wide: SENTINEL = nothing left | PT_LEAF | count - 1, first | node index
    int sp = 0;               // stack entries held

    // level l of the lane's stack: LDS below lds_stack, the spill area above (never beyond the levels the plan reserved)
    auto push = [&](uint32_t word) {
        if (sp < lds_stack) s_stack[(size_t)sp * TB] = word;
        else if ((uint32_t)(sp - lds_stack) < spill_levels) my_spill[(size_t)(sp - lds_stack) * spill_stride] = word;
        sp++;
    };
    auto pop = [&]() -> uint32_t {
        if (sp == 0) return SENTINEL;
        sp--;
        uint32_t w = SENTINEL;
        if (sp < lds_stack) w = s_stack[(size_t)sp * TB];
        else if ((uint32_t)(sp - lds_stack) < spill_levels) w = my_spill[(size_t)(sp - lds_stack) * spill_stride];
        return w;
    };

    for (;;) {
        // ---- refill idle lanes with the next rows of the wave's sequence
        const unsigned long long idle = __ballot(!have);
        const int n_idle = __popcll(idle);
        if (!exhausted && n_idle >= refill_min_idle) {
            if (!have) {
                const uint32_t v = cursor + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                const uint32_t qq = (v >> 6) * wave_stride + wave_base + (v & 63u);
                if (qq < n) {
                    q = qq;
                    ptm::f3 O, D;
                    cx_ray(io.rays6, io.points, { io.dx, io.dy, io.dz }, q, O, D);
                    bound = cx_bound(io.tmax_per, tmax, q);
                    count = 0u;
                    winding = 0;
                    sp = 0;
                    cur = SENTINEL;  // a ray that does not walk: the leaf phase below writes its two zeros
                    if (cx_live(O, D, tmin, bound)) {
                        ray = cx_setup(O, D);
                        cur = 0u;  // the root
                    }
                    have = true;
                }
            }
            cursor += (uint32_t)n_idle;
            exhausted = (cursor >> 6) * wave_stride + wave_base >= n;  // chunk of the next refill starts past the end
        }
        if (__ballot(have) == 0ull) break;

        // ---- node phase: every lane descends until it holds a leaf (or runs out of nodes)
        bool do_node = have && !(cur & PT_LEAF);
        const int n_have = __popcll(__ballot(have));
        while (do_node) {
            const float4 *nd = wide + (size_t)cur * NODE_F4;
            const float4 lx = nd[0], ly = nd[1], lz = nd[2], hx = nd[3], hy = nd[4], hz = nd[5];
            const float4 cw = nd[6];
            const uint32_t w0 = __float_as_uint(cw.x), w1 = __float_as_uint(cw.y), w2 = __float_as_uint(cw.z), w3 = __float_as_uint(cw.w);
            const ptm::f3 O = ray.pre.org;
            // an empty slot, or a box the ray does not pass: no child.  The range is the ray's own from the first step to the last.
            const bool p0 = w0 != SENTINEL && cx_slab({ lx.x, ly.x, lz.x }, { hx.x, hy.x, hz.x }, O, ray.inv, tmin, bound);
            const bool p1 = w1 != SENTINEL && cx_slab({ lx.y, ly.y, lz.y }, { hx.y, hy.y, hz.y }, O, ray.inv, tmin, bound);
            const bool p2 = w2 != SENTINEL && cx_slab({ lx.z, ly.z, lz.z }, { hx.z, hy.z, hz.z }, O, ray.inv, tmin, bound);
            const bool p3 = w3 != SENTINEL && cx_slab({ lx.w, ly.w, lz.w }, { hx.w, hy.w, hz.w }, O, ray.inv, tmin, bound);
            // slot order, no sort: the first passing child stays in hand, the others go onto the stack -- at most three pushes
            uint32_t next = SENTINEL;
            auto take = [&](bool p, uint32_t w) {
                if (!p) return;
                if (next == SENTINEL) next = w;
                else push(w);
            };
            take(p0, w0); take(p1, w1); take(p2, w2); take(p3, w3);
            cur = next != SENTINEL ? next : pop();
            do_node = !(cur & PT_LEAF);  // (SENTINEL has the bit: a lane with nothing left waits for the leaf phase to retire it)
            // fewer than 1/6 of the wave's rays still descending while the rest waits with a leaf: the leaves go first (k_nearest)
            const int n_cont = __popcll(__ballot(do_node));
            if (n_cont * 6 < n_have) break;
        }
        // ---- leaf phase
        if (have && (cur & PT_LEAF)) {
            if (cur != SENTINEL) {
                const uint32_t first = cur & 0x0FFFFFFFu, cnt = ((cur >> 28) & 7u) + 1u;
                for (uint32_t k = 0; k < cnt; k++) {
                    const size_t ti = 3 * (size_t)(first + k);
                    const float4 a = tri4[ti + 0], b = tri4[ti + 1], c = tri4[ti + 2];
                    const int s = cx_counts(ray, tmin, bound, pad, { a.x, a.y, a.z }, { b.x, b.y, b.z }, { c.x, c.y, c.z });
                    count += s != 0 ? 1u : 0u;
                    winding += s;
                }
                cur = pop();
            }
            if (cur == SENTINEL) {  // the walk is finished: the caller's two words, and the lane becomes idle
                cx_write(io.count, io.winding, q, count, winding);
                have = false;
            }
        }
    }
}

// ---- one picker for the family (wavefront_host.h): the plan prepares what it returns, the launch launches it
using CrossFn = decltype(&k_crossings<true>);
CrossFn pick_crossings(bool lds) { return lds ? k_crossings<true> : k_crossings<false>; }

struct CrossPlan {
    bool lds = false;
    size_t smem = 0;
    int grid = 0, refill = 16, lds_stack = 8;
    uint32_t spill_levels = 0;
    float pad = 0.f;
};

// the stack entries a walk can hold: nearest.hip's nearest_stack_bound for the same tree (a node step pushes at most three and descends)
uint32_t crossings_stack_bound(const pt_scene *s) { return s->stack_need != 0xFFFFFFFFu ? s->stack_need + 1u : 3u * (s->height_tree / 2u + 1u) + 1u; }

// scene_build.hip's leaf_pad_of, same float operations: what every builder and the refit put around every leaf of THIS scene box
float crossings_pad(const pt_scene *s)
{
    float scale = 0.f;
    for (int k = 0; k < 3; k++) scale = fmaxf(scale, fmaxf(fabsf(s->bmin[k]), fabsf(s->bmax[k])));
    return scale * 3.814697265625e-06f;
}

pt_status plan_crossings(pt_scene *s, uint32_t form, CrossPlan &cp)
{
    pt_ctx *ctx = s->ctx;
    const uint32_t bound = crossings_stack_bound(s);
    cp.lds_stack = pt_tuned(ctx->tune.lds_stack, (int)std::min(std::max(bound, 1u), 8u), 1, 32);
    cp.refill = pt_tuned(ctx->tune.refill, 16, 1, 64);  // k_nearest's threshold
    const size_t stack_bytes = (size_t)cp.lds_stack * TB * sizeof(uint32_t);
    const size_t image = cx_image_bytes(s->n_wide, s->n_tris);
    const bool fits = image + stack_bytes <= CX_LDS_LIMIT;
    if (form == PT_CROSSINGS_LDS && !fits) {
        ctx->err = "PT_CROSSINGS_LDS: the scene's image (" + std::to_string(image) + " bytes: 144 per BVH4 node, 48 per triangle) and the stack (" +
                   std::to_string(stack_bytes) + " bytes) do not fit 96 KB of LDS; PT_CROSSINGS_GLOBAL and PT_CROSSINGS_AUTO walk any scene";
        return PT_ERR_UNSUPPORTED;
    }
    cp.lds = form == PT_CROSSINGS_LDS ||
             (form == PT_CROSSINGS_AUTO && CX_AUTO_TAKES_LDS && fits && lds_class_bytes(s->n_wide, s->n_tris) <= CX_LDS_CLASS_BYTES);
    cp.smem = stack_bytes + (cp.lds ? image : 0);
    int per_cu = 0;
    PT_TRY(ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_crossings(cp.lds)), TB, cp.smem, &per_cu));
    cp.grid = ctx->num_cus * ptw_tuned_blocks(ctx, per_cu);
    cp.spill_levels = bound > (uint32_t)cp.lds_stack ? bound - (uint32_t)cp.lds_stack : 0u;
    cp.pad = crossings_pad(s);
    return ptw_reserve_spill(ctx, (size_t)std::max(cp.spill_levels, 1u) * (size_t)cp.grid * TB * sizeof(uint32_t));
}

void launch_crossings(const CrossPlan &cp, const pt_scene *s, const CrossIO &io, float tmin, float tmax, uint32_t n, hipStream_t st)
{
    hipLaunchKernelGGL(pick_crossings(cp.lds), dim3(cp.grid), dim3(TB), (uint32_t)cp.smem, st, s->d_wide, s->d_tri4, s->n_wide, s->n_tris, io, tmin, tmax,
                       cp.pad, n, cp.refill, cp.lds_stack, reinterpret_cast<uint32_t *>(s->ctx->d_spill), cp.spill_levels);
}

constexpr uint64_t CX_MAX_LAUNCH = 1ull << 30;  // the row index inside a launch is 32 bits

}  // namespace

pt_status ptx_crossings_device(pt_scene *s, const pt_crossings_desc *d, uint64_t n, float *device_ms)
{
    pt_ctx *ctx = s->ctx;
    // ---- refusals: nothing launched, nothing written
    if (d->form > PT_CROSSINGS_GLOBAL) return pt_bad(ctx, "pt_crossings_desc.form is none of PT_CROSSINGS_AUTO, _LDS, _GLOBAL");
    if (d->flags) return pt_bad(ctx, "pt_crossings_desc.flags must be 0");
    PT_TRY(pt_check_reserved(ctx, "pt_crossings_desc", d->reserved));
    if (!d->d_count && !d->d_winding) return pt_bad(ctx, "pt_crossings_desc: d_count and d_winding are both NULL");
    if (n && d->d_rays6 && d->d_points) return pt_bad(ctx, "pt_crossings_desc: d_rays6 and d_points are both set; exactly one of the two carries the origins");
    if (n && !d->d_rays6 && !d->d_points) return pt_bad(ctx, "pt_crossings_desc: d_rays6 and d_points are both NULL");
    if (!std::isfinite(d->tmin)) return pt_bad(ctx, "pt_crossings_desc.tmin must be finite");
    if (!d->d_tmax && !(d->tmax > d->tmin)) return pt_bad(ctx, "pt_crossings_desc.tmax must be > tmin (+inf: no bound) when d_tmax is NULL");
    if (d->d_points && !(std::isfinite(d->direction[0]) && std::isfinite(d->direction[1]) && std::isfinite(d->direction[2])))
        return pt_bad(ctx, "pt_crossings_desc.direction must be finite when d_points is set");
    if (s->n_inst) {
        ctx->err = "pt_crossings_device counts in the mesh's own space: counting under instances is well defined for rays but not built (it needs a "
                   "two-level walk and a pad per instance), so an instanced scene is refused; pt_scene_set_instances with n = 0 restores the mesh";
        return PT_ERR_UNSUPPORTED;
    }
    PT_TRY(ptb_repair(s));  // (a scene that lost its trees, as pt_nearest_device does)
    CrossPlan cp;
    PT_TRY(plan_crossings(s, d->form, cp));  // (PT_CROSSINGS_LDS outside its class is refused whatever n is)
    if (n == 0) { if (device_ms) *device_ms = 0.f; return PT_OK; }
    const uint64_t n_launches = (n + CX_MAX_LAUNCH - 1) / CX_MAX_LAUNCH;
    const pt_status rc = pt_timed_pass(ctx, device_ms, [&](hipStream_t st) {
        for (uint64_t c = 0; c < n_launches; c++) {
            const uint64_t off = c * CX_MAX_LAUNCH;
            const uint32_t m = (uint32_t)std::min<uint64_t>(CX_MAX_LAUNCH, n - off);
            const CrossIO io = { d->d_rays6 ? static_cast<const float *>(d->d_rays6) + 6 * off : nullptr,
                                 d->d_points ? static_cast<const float *>(d->d_points) + 3 * off : nullptr,
                                 d->d_tmax ? static_cast<const float *>(d->d_tmax) + off : nullptr,
                                 d->d_count ? static_cast<uint32_t *>(d->d_count) + off : nullptr,
                                 d->d_winding ? static_cast<int32_t *>(d->d_winding) + off : nullptr,
                                 d->direction[0], d->direction[1], d->direction[2] };
            launch_crossings(cp, s, io, d->tmin, d->tmax, m, st);
        }
    });
    PT_TRY(rc);
    ctx->stats.launches_other += (uint32_t)n_launches;
    return PT_OK;
}
