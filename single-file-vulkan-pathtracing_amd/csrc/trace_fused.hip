// trace_fused.hip -- pt_trace_device with PT_TRACE_FUSED: ONE persistent kernel per launch that reads row i of the caller's d_rays6, walks the scene
// in LDS and writes ray i's answer straight into the caller's arrays.  No queues, no hit records in memory, no workspace.
//
// The walk is extend_body<true, false, false, PAIRS> (extend_kernel.h: k_extend_lds7 / _lds7p) restated, as fused_kernel.h restates it: the same node
// step (compact_node_step), the same leaf tests (ptl::pair_leaf_test / ptm::tri_test_perm), the same closest rule (least t, then lowest primitive
// id) and the same "first hit ends the walk" of the any-hit instantiations, in the same order -- so a ray's record has the bits the queue form's
// has.  Also kept: the wave-private ray sequence with its ballot-ranked refill, the scene image at LDS byte 0 with the one-dword LaneStack behind it
// (the plan's LDS bytes, unchanged), the plan's refill threshold.  New: the refill reads the caller's row (trace_fused_kernel.h tf_row, tf_bound)
// and the finish writes the caller's record (tf_record -> tf_hit_row / tf_surface / tf_occluded); primitive id and vertices come from the
// unpermuted triangle copy in LDS, normal / Kd / Ke from d_shade64 / d_faces (a few KB, cache-resident).
// A translation unit of its own, like fused_rays.hip, so that every other unit compiles what it compiled before.
#include "wavefront_host.h"

#include <algorithm>

#define PT_EXTEND_TEMPLATES_ONLY
#include "extend_kernel.h"

#define TD_LOADS_DONE()  // (the compiler's own waits: the surface gathers sit in the walk's epilogue, not in a kernel of their own)
#include "trace_fused_kernel.h"

// Where the epilogue runs.  0: where extend_body stores its hit record -- once per group of lanes that finish in the same pass of the loop.
// 1: a finished lane keeps its record in the registers that held it, and the records are written at the top of the next refill block (at least
// `refill` lanes together) and in a drain before the loop's exit.  DESIGN.md section 26 has the two measured.
#ifndef PT_TRACE_FUSED_DEFER
#define PT_TRACE_FUSED_DEFER 0
#endif

namespace {

template <bool PAIRS, int KIND>
__global__ __launch_bounds__(TB, PT_EXTEND_WAVES) void k_trace_fused(const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4, uint32_t n_wide,
                                                                     uint32_t n_tris, TraceFusedIO io, const float4 *__restrict__ g_rec64,
                                                                     const float *__restrict__ g_faces, uint32_t n, int refill_min_idle, float tmin, float tmax)
{
    // ANY (extend_body's ray_tmax != null): a per-ray upper bound instead of `tmax`, and the first hit below it ends the walk.  A template
    // parameter: the closest-hit instantiations must not carry these branches (extend_kernel.h on the _sh twins)
    constexpr bool ANY = KIND == PT_TF_ANY;
    constexpr bool DEFER = PT_TRACE_FUSED_DEFER != 0;
    constexpr uint32_t LEAF_BIT = C14_LEAF, DONE = C14_DONE;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // nodes | three triangle copies from LDS byte 0, the stack behind them (compact_stack_bytes, level -1 first): ExtendPlan::smem
    float4 *s_wide = reinterpret_cast<float4 *>(smem);
    float4 *s_tri = s_wide + LDS_NODE_F4 * (size_t)n_wide;
    lds_stage_nodes<TB, true>(s_wide, g_wide, n_wide);
    lds_stage_tris<TB>(s_tri, g_tri4, n_tris);
    __syncthreads();
    const float4 *wide = s_wide;
    const float4 *tri4 = s_tri;
    const float4 *tri_plain = s_tri + 6 * (size_t)n_tris;  // the kz = 2 copy: components as the scene has them
    LaneStack<TB> stk((lds_u32 *)reinterpret_cast<uint32_t *>(smem + lds_scene_bytes(n_wide, n_tris)) + threadIdx.x);

    bool have = false, exhausted = false;
    [[maybe_unused]] bool pending = false;  // DEFER: the lane's ray is finished and its record not yet written
    uint32_t q = 0;
    // wave-private ray sequence: virtual index v -> row (v/64)*wave_stride + wave_base + v%64
    const uint32_t wave_base = (blockIdx.x * (TB / 64) + (threadIdx.x >> 6)) * 64u;
    const uint32_t wave_stride = gridDim.x * TB;
    uint32_t cursor = 0;
    ptm::f3 inv{}, invf{}, on{}, of{}, orgp{};
    ptm::RayPre pre{};
    uint32_t ax = 0, ay = 0, az = 0;
    uint32_t tri_base = 0;
    float best_t = tmax, best_V = 0.f, best_W = 0.f, best_det = 1.f;
    uint32_t best_pos = PT_MISS;
    [[maybe_unused]] uint32_t best_prim = PT_MISS;
    uint32_t cur = DONE;

    auto pop_compact = [&](uint32_t cut) -> uint32_t {
        while (stk.has_entries()) {
            const uint32_t e = stk.pop();
            if (entry_within(e, cut)) return e & 0x3FFFu;
        }
        return DONE;
    };
    // the caller's record of ray q, from what the walk holds for it
    auto emit = [&] {
        if constexpr (ANY) {
            io.occluded[q] = tf_occluded(best_pos);
        } else {
            const float4 rec = tf_record({ best_pos, best_t, best_V, best_W, best_det });
            if (KIND == PT_TF_HITS || io.hits) tf_hit_row(static_cast<uint32_t *>(io.hits), q, rec, tri_plain);
            if constexpr (KIND == PT_TF_SURFACE) {
                const TdScene sc = { tri_plain, g_rec64, g_faces, nullptr, nullptr, n_tris };
                tf_surface(sc, rec, { io.position, io.normal, io.albedo, io.emission }, q);
            }
        }
    };

    for (;;) {
        // ---- refill idle lanes with the next rows of the wave's sequence
        const unsigned long long idle = __ballot(!have);
        const int n_idle = __popcll(idle);
        if (!exhausted && n_idle >= refill_min_idle) {
            if (!have) {
                if constexpr (DEFER) {
                    if (pending) emit();
                    pending = false;
                }
                // rank among the idle lanes (v_mbcnt in both leaf forms: the prefix mask k_extend_lds7 keeps is two registers held through the loop, which
                // the surface epilogue needs)
                const uint32_t v = cursor + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                const uint32_t qq = (v >> 6) * wave_stride + wave_base + (v & 63u);
                if (qq < n) {
                    q = qq;
                    const TfRay r = tf_row(io.rays6, q);
                    float bound = tmax;
                    if constexpr (ANY) bound = tf_bound(io.d_tmax, tmax, q);
                    const ptm::f3 org = { r.ox, r.oy, r.oz };
                    const ptm::f3 dir = { r.dx, r.dy, r.dz };
                    pre = ptm::ray_setup<PAIRS>(org, dir);  // (k_extend_lds7: pt_math.h)
                    inv = { ptm::safe_inv(dir.x), ptm::safe_inv(dir.y), ptm::safe_inv(dir.z) };
                    slab_setup(org, inv, invf, on, of);
                    ax = inv.x < 0.f ? LDS_NEG_AXIS : 0u;
                    ay = inv.y < 0.f ? LDS_NEG_AXIS : 0u;
                    az = inv.z < 0.f ? LDS_NEG_AXIS : 0u;
                    tri_base = (uint32_t)pre.kz * 3u * n_tris;
                    orgp = { ptm::sel3(pre.kz, org.y, org.z, org.x), ptm::sel3(pre.kz, org.z, org.x, org.y), ptm::sel3(pre.kz, org.x, org.y, org.z) };
                    best_t = bound; best_V = 0.f; best_W = 0.f; best_det = 1.f;
                    best_pos = PT_MISS; best_prim = PT_MISS;
                    cur = 0u;  // wide root
                    stk.clear();
                    have = true;
                }
            }
            cursor += (uint32_t)n_idle;
            exhausted = (cursor >> 6) * wave_stride + wave_base >= n;  // chunk of the next refill starts past the end
        }
        if (__ballot(have) == 0ull) break;

        // ---- node phase: every lane descends until it holds a leaf (or runs out of nodes)
        bool do_node = have && !(cur & LEAF_BIT);
        const int n_have = __popcll(__ballot(have));
        while (do_node) {
            cur = compact_node_step<TB, true>(wide, cur, inv, invf, on, of, ax, ay, az, tmin, best_t, stk, [&](uint32_t, uint32_t kcut) { return pop_compact(kcut); });
            do_node = !(cur & LEAF_BIT);
            // fewer than 1/6 of the wave's rays still descending while the rest waits with a leaf: the leaves go first (extend_body)
            const int n_cont = __popcll(__ballot(do_node));
            if (n_cont * 6 < n_have) break;
        }
        // ---- leaf phase
        if (have) {
            if constexpr (PAIRS) {
                if (cur != DONE && (cur & LEAF_BIT)) {
                    const uint32_t first = cur & 0x7FFu;
                    const bool two = ((cur >> 11) & 3u) != 0u;  // count - 1: a fan pair at positions first, first + 1
                    // (ANY: tmin < t < the ray's own bound, strictly -- best_t until the first hit, which ends the walk; tmax plays no part)
                    ptl::pair_leaf_test(tri4, (size_t)tri_base + 3 * (size_t)first, two, first, pre, orgp, tmin, ptl::leaf_upper(ANY, best_t, tmax),
                                        [&](float t, float V, float W, float det, uint32_t pos, uint32_t) {
                                            if (ptl::closer_single_level(tri4, tri_base, t, V, W, det, pos, best_t, best_V, best_W, best_det, best_pos) && ANY)
                                                stk.clear();  // any hit will do: nothing pending any more
                                        },
                                        [] {});
                    cur = pop_compact(pop_cut(best_t));
                }
            } else if (cur != DONE && (cur & LEAF_BIT)) {
                const uint32_t first = cur & 0x7FFu;
                const uint32_t cnt = ((cur >> 11) & 3u) + 1u;
                for (uint32_t k = 0; k < cnt; k++) {
                    const uint32_t pos = first + k;
                    const size_t ti = (size_t)tri_base + 3 * (size_t)pos;
                    const float4 a = tri4[ti + 0], b = tri4[ti + 1], c = tri4[ti + 2];
                    float t, V, W, det;
                    if (ptm::tri_test_perm(pre, orgp, { a.x, a.y, a.z }, { b.x, b.y, b.z }, { c.x, c.y, c.z }, tmin, ptl::leaf_upper(ANY, best_t, tmax), t, V, W, det)) {
                        // closest t; equal t -> lowest gl_PrimitiveID (the OBJ has coincident quads)
                        const uint32_t prim = __float_as_uint(a.w);
                        if (t < best_t || (t == best_t && prim < best_prim)) {
                            best_t = t; best_V = V; best_W = W; best_det = det; best_pos = pos; best_prim = prim;
                            if (ANY) stk.clear();
                        }
                    }
                }
                cur = pop_compact(pop_cut(best_t));
            }
            if (cur == DONE) {  // traversal finished: the lane becomes idle
                if constexpr (DEFER) pending = true;
                else emit();
                have = false;
            }
        }
    }
    if constexpr (DEFER) {  // the drain: lanes that finished after their wave's last refill
        if (pending) emit();
    }
}

// ---- one picker for the family (wavefront_host.h): the plan prepares what it returns, the launch launches it
using TraceFusedFn = decltype(&k_trace_fused<true, PT_TF_HITS>);
TraceFusedFn pick_trace_fused(bool pairs, int kind)
{
    switch (kind) {
    case PT_TF_HITS: return pairs ? k_trace_fused<true, PT_TF_HITS> : k_trace_fused<false, PT_TF_HITS>;
    case PT_TF_SURFACE: return pairs ? k_trace_fused<true, PT_TF_SURFACE> : k_trace_fused<false, PT_TF_SURFACE>;
    default: return pairs ? k_trace_fused<true, PT_TF_ANY> : k_trace_fused<false, PT_TF_ANY>;
    }
}

}  // namespace

pt_status ptw_plan_trace_fused(pt_scene *s, const ExtendPlan &pl, int kind, TraceFusedPlan &tp)
{
    pt_ctx *ctx = s->ctx;
    // the plan's LDS image and stack (ExtendPlan::smem), its leaf form and refill threshold; the grid from THIS kernel's occupancy
    tp.kind = kind;
    tp.pairs = pl.pairs;
    tp.smem = pl.smem;
    tp.refill = pl.refill;
    int per_cu = 0;
    PT_TRY(ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_trace_fused(tp.pairs, kind)), TB, tp.smem, &per_cu));
    tp.grid = ctx->num_cus * ptw_tuned_blocks(ctx, per_cu);
    return PT_OK;
}

void ptw_launch_trace_fused(const TraceFusedPlan &tp, const pt_scene *s, const TraceFusedIO &io, uint32_t n, float tmin, float tmax, hipStream_t st,
                            hipEvent_t ev0, hipEvent_t ev1)
{
    hipExtLaunchKernelGGL(pick_trace_fused(tp.pairs, tp.kind), dim3(tp.grid), dim3(TB), (uint32_t)tp.smem, st, ev0, ev1, 0u, s->d_wide, s->d_tri4, s->n_wide,
                          s->n_tris, io, s->d_shade64, s->d_faces, n, tp.refill, tmin, tmax);
}
