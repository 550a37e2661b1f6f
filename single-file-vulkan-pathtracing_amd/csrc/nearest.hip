// nearest.hip -- pt_nearest_device: for every point of a device array, the closest point of the mesh, its triangle and the squared distance.
// ONE persistent kernel per launch: a lane reads row i of the caller's d_points, walks the scene's BVH4 by box distance and writes query i's
// answer straight into the caller's arrays.  No queues, no records in memory, no workspace (stack entries beyond the LDS share go to the
// context's spill area, like the ray kernels').
//
// What defines the result is in nearest_kernel.h (shared with tests/nearest_host.cpp): the closest point of one triangle, the box distance, the
// accept rule, and the lemma "box distance <= dist2 for every box that contains the triangle's vertices".  By the lemma the walk below returns what
// a loop over all triangles returns -- the least dist2 within the radius, then the lowest primitive id -- whatever the tree, the builder, the form
// or the launch shape: a subtree is skipped only when its box lies STRICTLY beyond the best dist2 held (at an equal distance it may hold a lower id).
//
// The tree: s->d_wide (128-B fp32 nodes, what pt_scene_read_bvh4 returns) and s->d_tri4 (leaf position -> A, B, C and the primitive id), which every
// single-level scene has, whatever its ray kernels prefer; boxes are min / max of vertices in fp32 (padded outwards at most), through refits too.
// The fp16 nodes and the 8-wide tree are not used: the lemma wants boxes that contain the vertices as fp32 numbers.
//
// The walk.  A node step computes the four children's box distances, drops those > best, descends into the nearest and pushes the others farthest
// first (at most three) with their distances as keys; a pop discards entries whose key is > best by then.  A leaf step runs nr_closest over the
// leaf's triangles.  Stack entries are {key, child word}, 8 bytes: level l < lds_stack in LDS ([level][thread]: a lane's ds_read/write_b64 next to
// its neighbours', conflict-free), the levels above in the spill area ([level][grid thread]).  Nothing is kept in private memory.
//
// The loop is k_trace_fused's: a wave-private query sequence, ballot-ranked refill of idle lanes at the plan's threshold, a node phase that yields
// to waiting leaves, a finished lane writes its record at once.
//
// Two forms.  LDS: nodes and ONE unpermuted copy of tri4 staged from LDS byte 0, the stack behind them.  The nodes keep the 128-B layout at a
// 144-B stride (lds_stage_nodes128): lanes sit on different nodes and read the same 16-B field of them, and with ds_read_b128's 64 banks a stride
// of 36 dwords puts sixteen consecutive nodes' fields on sixteen different bank quads -- a 16-lane group reads conflict-free -- where 160 B (40
// dwords) folds them onto eight.  A triangle is 12 dwords: the same.  GLOBAL: both through L1 / L2, only the stack in LDS.
#include "wavefront_host.h"

#include <algorithm>
#include <cmath>

#include "lds_scene.h"
#include "nearest_kernel.h"

namespace {

constexpr size_t NR_LDS_LIMIT = 96 * 1024;  // image + stack of PT_NEAREST_LDS: the bound PT_EXTEND_LDS uses
// PT_NEAREST_AUTO on scenes of the ray kernels' LDS class (lds_class_bytes <= 24 KB): the LDS form only where its slowest pass beat the GLOBAL
// form's fastest on every box shape measured (TD_AUTO_TAKES_FUSED's rule).  Measured on the MI355X
// (profiles/nearest_probe.json): the LDS form's medians are 1.04 .. 1.21x faster on all eight box shapes, but on one of them (2^20 lattice queries
// in lattice order, 0.0614 against 0.0640 ms) its slowest pass, 0.0645 ms, does not beat the GLOBAL form's fastest, 0.0634 ms: GLOBAL everywhere.
constexpr bool NR_AUTO_TAKES_LDS = false;
constexpr size_t NR_LDS_CLASS_BYTES = 24 * 1024;

__host__ __device__ constexpr size_t nr_image_bytes(size_t n_wide, size_t n_tris) { return lds_nodes128_bytes(n_wide) + sizeof(float4) * 3 * n_tris; }

struct NearestIO {
    const float *points, *max_dist;  // max_dist: nullable
    uint32_t *nearest;               // pt_nearest rows, nullable
    float *point;                    // nullable
};

template <bool LDS>
__global__ __launch_bounds__(TB) void k_nearest(const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4, uint32_t n_wide, uint32_t n_tris,
                                                NearestIO io, float max_dist, uint32_t n, int refill_min_idle, int lds_stack, uint2 *__restrict__ spill,
                                                uint32_t spill_levels)
{
    constexpr uint32_t NODE_F4 = LDS ? LDS_NODE128_F4 : 8u;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const float4 *wide = g_wide, *tri4 = g_tri4;
    uint2 *s_stack = reinterpret_cast<uint2 *>(smem);
    if constexpr (LDS) {
        float4 *s_wide = reinterpret_cast<float4 *>(smem);
        float4 *s_tri = s_wide + LDS_NODE128_F4 * (size_t)n_wide;
        lds_stage_nodes128<TB>(s_wide, g_wide, n_wide);
        for (uint32_t i = threadIdx.x; i < 3 * n_tris; i += TB) s_tri[i] = g_tri4[i];
        __syncthreads();
        wide = s_wide;
        tri4 = s_tri;
        s_stack = reinterpret_cast<uint2 *>(smem + nr_image_bytes(n_wide, n_tris));
    }
    s_stack += threadIdx.x;
    const uint32_t spill_stride = gridDim.x * TB;
    uint2 *my_spill = spill + (size_t)blockIdx.x * TB + threadIdx.x;

    bool have = false, exhausted = false;
    uint32_t q = 0;
    // wave-private query sequence: virtual index v -> row (v/64)*wave_stride + wave_base + v%64
    const uint32_t wave_base = (blockIdx.x * (TB / 64) + (threadIdx.x >> 6)) * 64u;
    const uint32_t wave_stride = gridDim.x * TB;
    uint32_t cursor = 0;
    NrVec P{};
    float best_d = -1.f, best_u = 0.f, best_v = 0.f;
    NrVec best_q{};
    uint32_t best_prim = NR_MISS;
    uint32_t cur = SENTINEL;  // a child word of d_wide: SENTINEL = nothing left | PT_LEAF | count - 1, first | node index
    int sp = 0;               // stack entries held

    // level l of the lane's stack: LDS below lds_stack, the spill area above (never beyond the levels the plan reserved)
    auto push = [&](float key, uint32_t word) {
        const uint2 e = make_uint2(__float_as_uint(key), word);
        if (sp < lds_stack) s_stack[(size_t)sp * TB] = e;
        else if ((uint32_t)(sp - lds_stack) < spill_levels) my_spill[(size_t)(sp - lds_stack) * spill_stride] = e;
        sp++;
    };
    auto pop = [&]() -> uint32_t {
        while (sp > 0) {
            sp--;
            uint2 e = make_uint2(0x7F800000u, SENTINEL);
            if (sp < lds_stack) e = s_stack[(size_t)sp * TB];
            else if ((uint32_t)(sp - lds_stack) < spill_levels) e = my_spill[(size_t)(sp - lds_stack) * spill_stride];
            if (!(__uint_as_float(e.x) > best_d) && e.y != SENTINEL) return e.y;
        }
        return SENTINEL;
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
                    P = nr_point(io.points, q);
                    best_d = nr_radius2(nr_radius(io.max_dist, max_dist, q));
                    best_prim = NR_MISS;
                    best_u = 0.f; best_v = 0.f; best_q = { 0.f, 0.f, 0.f };
                    cur = 0u;  // the root
                    sp = 0;
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
            uint32_t w0 = __float_as_uint(cw.x), w1 = __float_as_uint(cw.y), w2 = __float_as_uint(cw.z), w3 = __float_as_uint(cw.w);
            float k0 = nr_box_dist2(P, { lx.x, ly.x, lz.x }, { hx.x, hy.x, hz.x });
            float k1 = nr_box_dist2(P, { lx.y, ly.y, lz.y }, { hx.y, hy.y, hz.y });
            float k2 = nr_box_dist2(P, { lx.z, ly.z, lz.z }, { hx.z, hy.z, hz.z });
            float k3 = nr_box_dist2(P, { lx.w, ly.w, lz.w }, { hx.w, hy.w, hz.w });
            // an empty slot, or a box strictly beyond the best: no child (the comparison is strict: a box AT best may hold a lower primitive id)
            if (k0 > best_d) w0 = SENTINEL;
            if (k1 > best_d) w1 = SENTINEL;
            if (k2 > best_d) w2 = SENTINEL;
            if (k3 > best_d) w3 = SENTINEL;
            // the four by distance, nearest first (five compare-exchanges; dropped children carry their distance along and are skipped below)
            auto cx = [](float &ka, uint32_t &wa, float &kb, uint32_t &wb) {
                const bool s = kb < ka;
                const float kt = s ? kb : ka, ku = s ? ka : kb;
                const uint32_t wt = s ? wb : wa, wu = s ? wa : wb;
                ka = kt; kb = ku; wa = wt; wb = wu;
            };
            cx(k0, w0, k1, w1); cx(k2, w2, k3, w3); cx(k0, w0, k2, w2); cx(k1, w1, k3, w3); cx(k1, w1, k2, w2);
            // farthest first onto the stack, the nearest stays in hand: at most three pushes
            uint32_t next = SENTINEL;
            float next_key = 0.f;
            auto take = [&](float k, uint32_t w) {
                if (w == SENTINEL) return;
                if (next != SENTINEL) push(next_key, next);
                next = w; next_key = k;
            };
            take(k3, w3); take(k2, w2); take(k1, w1); take(k0, w0);
            cur = next != SENTINEL ? next : pop();
            do_node = !(cur & PT_LEAF);  // (SENTINEL has the bit: a lane with nothing left waits for the leaf phase to retire it)
            // fewer than 1/6 of the wave's queries still descending while the rest waits with a leaf: the leaves go first (k_trace_fused)
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
                    const uint32_t prim = __float_as_uint(a.w);
                    const NrClosest r = nr_closest(P, { a.x, a.y, a.z }, { b.x, b.y, b.z }, { c.x, c.y, c.z });
                    if (nr_accept(r.dist2, prim, best_d, best_prim)) {
                        best_d = r.dist2; best_prim = prim; best_u = r.u; best_v = r.v; best_q = r.q;
                    }
                }
                cur = pop();
            }
            if (cur == SENTINEL) {  // the walk is finished: the caller's record, and the lane becomes idle
                if (io.nearest) nr_write_nearest(io.nearest, q, best_prim, best_d, best_u, best_v);
                if (io.point) nr_write_point(io.point, q, best_prim, best_q);
                have = false;
            }
        }
    }
}

// ---- one picker for the family (wavefront_host.h): the plan prepares what it returns, the launch launches it
using NearestFn = decltype(&k_nearest<true>);
NearestFn pick_nearest(bool lds) { return lds ? k_nearest<true> : k_nearest<false>; }

struct NearestPlan {
    bool lds = false;
    size_t smem = 0;
    int grid = 0, refill = 16, lds_stack = 8;
    uint32_t spill_levels = 0;
};

// the stack entries a walk can hold: the bound ptw_plan_extend computes for the same tree (a node step pushes at most three and descends)
uint32_t nearest_stack_bound(const pt_scene *s) { return s->stack_need != 0xFFFFFFFFu ? s->stack_need + 1u : 3u * (s->height_tree / 2u + 1u) + 1u; }

pt_status plan_nearest(pt_scene *s, uint32_t form, NearestPlan &np)
{
    pt_ctx *ctx = s->ctx;
    const uint32_t bound = nearest_stack_bound(s);
    np.lds_stack = pt_tuned(ctx->tune.lds_stack, (int)std::min(std::max(bound, 1u), 8u), 1, 32);
    np.refill = pt_tuned(ctx->tune.refill, 16, 1, 64);  // the LDS ray kernels' threshold; the fastest of 1 .. 64 swept on the box
    const size_t stack_bytes = (size_t)np.lds_stack * TB * sizeof(uint2);
    const size_t image = nr_image_bytes(s->n_wide, s->n_tris);
    const bool fits = image + stack_bytes <= NR_LDS_LIMIT;
    if (form == PT_NEAREST_LDS && !fits) {
        ctx->err = "PT_NEAREST_LDS: the scene's image (" + std::to_string(image) + " bytes: 144 per BVH4 node, 48 per triangle) and the stack (" +
                   std::to_string(stack_bytes) + " bytes) do not fit 96 KB of LDS; PT_NEAREST_GLOBAL and PT_NEAREST_AUTO walk any scene";
        return PT_ERR_UNSUPPORTED;
    }
    np.lds = form == PT_NEAREST_LDS ||
             (form == PT_NEAREST_AUTO && NR_AUTO_TAKES_LDS && fits && lds_class_bytes(s->n_wide, s->n_tris) <= NR_LDS_CLASS_BYTES);
    np.smem = stack_bytes + (np.lds ? image : 0);
    int per_cu = 0;
    PT_TRY(ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_nearest(np.lds)), TB, np.smem, &per_cu));
    np.grid = ctx->num_cus * ptw_tuned_blocks(ctx, per_cu);
    np.spill_levels = bound > (uint32_t)np.lds_stack ? bound - (uint32_t)np.lds_stack : 0u;
    return ptw_reserve_spill(ctx, (size_t)std::max(np.spill_levels, 1u) * (size_t)np.grid * TB * sizeof(uint2));
}

void launch_nearest(const NearestPlan &np, const pt_scene *s, const NearestIO &io, float max_dist, uint32_t n, hipStream_t st)
{
    hipLaunchKernelGGL(pick_nearest(np.lds), dim3(np.grid), dim3(TB), (uint32_t)np.smem, st, s->d_wide, s->d_tri4, s->n_wide, s->n_tris, io, max_dist, n,
                       np.refill, np.lds_stack, reinterpret_cast<uint2 *>(s->ctx->d_spill), np.spill_levels);
}

constexpr uint64_t NR_MAX_LAUNCH = 1ull << 30;  // the row index inside a launch is 32 bits

}  // namespace

pt_status ptn_nearest_device(pt_scene *s, const pt_nearest_desc *d, uint64_t n, float *device_ms)
{
    pt_ctx *ctx = s->ctx;
    // ---- refusals: nothing launched, nothing written
    if (d->form > PT_NEAREST_GLOBAL) return pt_bad(ctx, "pt_nearest_desc.form is none of PT_NEAREST_AUTO, _LDS, _GLOBAL");
    if (d->flags) return pt_bad(ctx, "pt_nearest_desc.flags must be 0");
    PT_TRY(pt_check_reserved(ctx, "pt_nearest_desc", d->reserved));
    if (!d->d_nearest && !d->d_point) return pt_bad(ctx, "pt_nearest_desc: d_nearest and d_point are both NULL");
    if (n && !d->d_points) return pt_bad(ctx, "pt_nearest_desc.d_points is NULL");
    if (!d->d_max_dist && !(d->max_dist >= 0.f)) return pt_bad(ctx, "pt_nearest_desc.max_dist must be >= 0 (+inf: no bound) when d_max_dist is NULL");
    if (s->n_inst) {
        ctx->err = "pt_nearest_device answers in the mesh's own space: under an instance's general 3x4 matrix distance is not object-space distance, "
                   "so an instanced scene is refused; pt_scene_set_instances with n = 0 restores the mesh";
        return PT_ERR_UNSUPPORTED;
    }
    PT_TRY(ptb_repair(s));  // (a scene that lost its trees, as pt_trace_device does)
    NearestPlan np;
    PT_TRY(plan_nearest(s, d->form, np));  // (PT_NEAREST_LDS outside its class is refused whatever n is)
    if (n == 0) { if (device_ms) *device_ms = 0.f; return PT_OK; }
    const uint64_t n_launches = (n + NR_MAX_LAUNCH - 1) / NR_MAX_LAUNCH;
    const pt_status rc = pt_timed_pass(ctx, device_ms, [&](hipStream_t st) {
        for (uint64_t c = 0; c < n_launches; c++) {
            const uint64_t off = c * NR_MAX_LAUNCH;
            const uint32_t m = (uint32_t)std::min<uint64_t>(NR_MAX_LAUNCH, n - off);
            const NearestIO io = { static_cast<const float *>(d->d_points) + 3 * off,
                                   d->d_max_dist ? static_cast<const float *>(d->d_max_dist) + off : nullptr,
                                   d->d_nearest ? static_cast<uint32_t *>(d->d_nearest) + 4 * off : nullptr,
                                   d->d_point ? static_cast<float *>(d->d_point) + 3 * off : nullptr };
            launch_nearest(np, s, io, d->max_dist, m, st);
        }
    });
    PT_TRY(rc);
    ctx->stats.launches_other += (uint32_t)n_launches;
    return PT_OK;
}
