// extend_launch.hip -- which closest-hit kernel stands in for traceRayEXT (raygen.rgen:63-75) on a given scene, and its launch.
//
//   scene                                   kernel (AUTO)                          where the scene lives
//   single level, <= 24 KB                  k_extend_lds7p / k_extend_lds7         LDS (BVH4 + 3 permuted triangle copies)
//   single level, up to ~11 000 triangles   k_extend<hbm> (extend_hbm.hip)         L2: 64-B fp16 BVH4 nodes, top-down layout
//   single level, beyond                    k_extend8 (extend_hbm.hip)             L2 / MALL / HBM: 64-B byte-plane 8-wide nodes
//   instanced                               k_extend_inst16                        TLAS in L2 (top levels in LDS), BLAS in LDS
//   instanced, outside that kernel's limits k_extend_inst                          fp32 nodes, both levels through L1 / L2
// PT_EXTEND_* asks for a variant explicitly (tests, A/B); every variant returns the same hit records.
#include "wavefront_host.h"

#include <algorithm>

#include "extend_kernel.h"  // k_extend<>, k_extend_lds7 / _lds7p (+ their shadow-ray twins), the slab / stack helpers
#include "extend_inst16.h"  // k_extend_inst16
#include "extend_inst.h"    // k_extend_inst

namespace {

// ---- one picker per kernel family: the plan prepares what it returns, the launch launches it ---------------------------------------
// single-level scenes in LDS.  compact: one-dword stack entries (ExtendPlan::spill == false and tmin > 0), else the 8-byte-entry
// kernel; the instrumented twin (count) has no shadow-ray form, it takes ray_tmax as a run-time argument
using ExtendFn = decltype(&k_extend<true, false, true>);
ExtendFn pick_extend_lds(bool compact, bool pairs, bool count, bool shadow)
{
    if (!compact) return count ? k_extend<true, true, true> : k_extend<true, false, true>;
    if (count) return pairs ? k_extend<true, true, false, true> : k_extend<true, true, false>;
    if (pairs) return shadow ? k_extend_lds7p_sh : k_extend_lds7p;
    return shadow ? k_extend_lds7_sh : k_extend_lds7;
}
// two-level scenes, fp32 nodes (shadow rays: no instrumented twin)
using ExtendInstFn = decltype(&k_extend_inst<false, false>);
ExtendInstFn pick_extend_inst(bool lds_blas, bool count, bool shadow)
{
    if (shadow) return lds_blas ? k_extend_inst<false, true, true> : k_extend_inst<false, false, true>;
    if (count) return lds_blas ? k_extend_inst<true, true> : k_extend_inst<true, false>;
    return lds_blas ? k_extend_inst<false, true> : k_extend_inst<false, false>;
}
// two-level scenes, fp16 nodes and 15-bit child codes
using ExtendInst16Fn = decltype(&k_extend_inst16<false, false>);
ExtendInst16Fn pick_extend_inst16(bool pairs, bool count, bool shadow)
{
    if (shadow) return pairs ? k_extend_inst16<false, true, true> : k_extend_inst16<false, false, true>;
    if (count) return pairs ? k_extend_inst16<true, true> : k_extend_inst16<true, false>;
    return pairs ? k_extend_inst16<false, true> : k_extend_inst16<false, false>;
}

}  // namespace

pt_status ptw_plan_extend(pt_scene *s, uint32_t want, ExtendPlan &pl)
{
    pt_ctx *ctx = s->ctx;
    if (want > PT_EXTEND_HBM8) { ctx->err = "unknown extend variant"; return PT_ERR_INVALID_ARG; }
    if (want == PT_EXTEND_FLAT_REMOVED) {
        ctx->err = "PT_EXTEND_FLAT (the brute-force loop, never AUTO) was removed in API version 5: every tree walk returns the brute-force closest hit";
        return PT_ERR_UNSUPPORTED;
    }
    if (s->broken) {  // an earlier rebuild of the tree ran out of memory (lbvh_build.hip): never launch on null tables
        const pt_status rcb = ptb_repair(s);
        if (rcb != PT_OK) return rcb;
    }
    // AUTO walks scenes beyond L2 (at first; now nearly every scene beyond LDS, below) through the 8-wide tree (64-B nodes with byte planes): fewer distinct lines per ray -- measured on
    // MI355X, same box, three rounds: C5 2 465 -> 2 547 Mrays/s (+3.4 %), C5x 2 405 -> 2 546 (+5.9 %), 36.2 -> 27.7 and 29.5 -> 24.2
    // node visits per ray (profiles/r03_ab_c5_c5x_hbm8_64B_nodes.log); pt_tuning.hbm8 = 0 keeps the BVH4, 1 takes the 8-wide tree
    // for every scene that does not fit LDS
    const uint64_t ws4 = 64ull * (s->n_wide16t ? s->n_wide16t : s->n_wide) + 64ull * s->n_tris;
    // (round 3, last session: with the 8-wide kernel's new vote, refill threshold and spill-free instantiation the crossover fell from
    // 32 MiB of BVH4 nodes + records to ~1 MiB, i.e. ~11 000 triangles -- soups of 2 500 / 5 000 / 12 000 / 20 000 / 50 000 / 100 000 /
    // 200 000 / 400 000 triangles, 8-wide against BVH4 kernel: -4 / -1.7 / +1.7 / +3.8 / +11 / +11 / +18 / +21 %,
    // profiles/r03ca_bvh4_vs_8wide_midsize.log, r03cb_bvh4_vs_8wide_small.log)
    const bool auto8_big = want == PT_EXTEND_AUTO && ctx->tune.hbm8 != 0 && ws4 > (1ull << 20) && s->n_tris > PT_SAH_MAX_TRIS;
    if ((want == PT_EXTEND_HBM8 || (want == PT_EXTEND_AUTO && ctx->tune.hbm8 == 1) || auto8_big) && !s->n_inst && !s->d_wide8) {
        const pt_status rc8 = ptb_ensure_wide8(s);   // built on first request (260 B per triangle nobody else needs)
        if (rc8 != PT_OK) return rc8;
    }
    if (want == PT_EXTEND_HBM8 && (s->n_inst || !s->d_wide8)) { ctx->err = "no 8-wide nodes for this scene (instanced, or <= 2048 triangles)"; return PT_ERR_UNSUPPORTED; }
    if (s->n_inst) {  // two-level scenes: one kernel variant (BVH4s read through L1/L2)
        if (want == PT_EXTEND_LDS) { ctx->err = "instanced scenes only have the HBM extend variant"; return PT_ERR_UNSUPPORTED; }
        pl.variant = PT_EXTEND_HBM;
        const size_t blas_bytes = lds_scene128_bytes(s->n_wide, s->n_tris);  // (k_extend_inst keeps the 128-B node: lds_scene.h)
        pl.lds_scene = blas_bytes <= 24 * 1024;  // here: the BLAS (shared by all instances) is staged in LDS
        pl.smem = (size_t)LDS_STACK * TB * sizeof(uint2) + (pl.lds_scene ? blas_bytes : 0);
        int per_cu_i = 0;
        const pt_status rci = ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_extend_inst(pl.lds_scene, false, false)), TB, pl.smem, &per_cu_i);
        if (rci != PT_OK) return rci;
        pl.refill = 64;  // a wave takes new rays only when all its lanes are done: entering an instance (ray transform, three
                         // divides) and the TLAS root are too expensive to run for a few refilled lanes.  C4: 16: 8.2, 32: 8.85,
                         // 48: 9.26, 56: 9.2, 64: 9.38 Grays/s
        pl.refill = pt_tuned(ctx->tune.refill, pl.refill, 1, 64);
        pl.grid = ctx->num_cus * per_cu_i;
        pl.smem_inst_fallback = pl.smem; pl.grid_inst_fallback = pl.grid;
        // the round-2 kernel when both levels fit its 15-bit child codes and the BLAS fits LDS
        const size_t smem16_scene = lds_scene16_bytes(s->n_wide, s->n_tris);
        const int lds16 = pt_tuned(ctx->tune.lds_stack, 16, 1, 32);
        pl.inst16 = s->d_tlas16 && s->d_wide16 && s->n_inst < 32768u && s->n_tlas16 < 32767u && s->n_wide < 32767u && s->n_tris <= 2047u &&
                    smem16_scene <= 24 * 1024 && ctx->tune.inst16 != 0;
        if (pl.inst16) {
            pl.lds_stack = lds16;
            // top levels of the TLAS staged in LDS next to the BLAS.  8 KB (102 nodes: the top four levels) measured best on
            // C4: 0 / 4 / 8 / 16 / 24 KB -> 11.95 / 12.16 / 12.31 / 10.7 / 11.1 Grays/s (profiles/r02i_ab_c4_tlas_lds.log) --
            // from 16 KB on the four resident blocks leave the other pipeline's k_shade no LDS to run beside them
            const size_t tlas_lds_bytes = (size_t)pt_tuned(ctx->tune.tlas_lds_kb, 8, 0, 96) * 1024;
            pl.n_tlas_lds = (uint32_t)std::min<size_t>(s->n_tlas16, tlas_lds_bytes / lds_nodes16_bytes(1));
            pl.smem = (size_t)lds16 * TB * sizeof(uint32_t) + smem16_scene + lds_nodes16_bytes(pl.n_tlas_lds);
            // the instrumented twin and the shadow-ray twin (NEE pipeline) run with the same launch shape; the grid is the product kernel's
            int per16 = 0;
            const auto prepare16 = [&](bool count, bool shadow, int *per_cu) {
                return ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_extend_inst16(s->pair_leaves, count, shadow)), TB, pl.smem, per_cu);
            };
            pt_status rc16 = prepare16(true, false, nullptr);
            if (rc16 == PT_OK) rc16 = prepare16(false, true, nullptr);
            if (rc16 == PT_OK) rc16 = prepare16(false, false, &per16);
            if (rc16 != PT_OK) return rc16;
            // four blocks per CU and refill at 48 idle lanes measured best on the 10 000-instance grid (C4: 4/48 10.73,
            // 5/48 10.33, 4/40 10.66, 4/56 10.35, 4/64 9.74 Grays/s; the fp32 kernel at its best, 4/64: 9.33)
            per16 = pt_tuned(ctx->tune.inst16_blocks, std::min(per16, 4), 1, 8);
            pl.grid = ctx->num_cus * per16;
            pl.refill = pt_tuned(ctx->tune.refill, 48, 1, 64);
        }
        // TLAS pushes <= 3 per level + 3 extra instances of a leaf, + EXIT, + the BLAS walk: the exact bound of the
        // BVH4 that is TRAVERSED when the builder gave one (the surface-area BVH4 of a small scene can be deeper
        // than the balanced LBVH whose height s->height is), else 3 per level of the collapsed LBVH
        const uint32_t blas_bound = s->stack_need != 0xFFFFFFFFu ? s->stack_need + 1u : 3u * (s->height_tree / 2u + 1u);
        const uint32_t bound_i = 3u * (std::max(s->tlas_height / 2u + 1u, s->tlas16_levels)) + 4u + blas_bound + 2u;
        pl.spill_levels = bound_i > (uint32_t)LDS_STACK ? bound_i - (uint32_t)LDS_STACK : 0u;  // (sized for the 8-entry fallback kernel)
        return ptw_reserve_spill(ctx, PT_MAX_PIPES * (size_t)std::max(pl.spill_levels, 1u) * (size_t)std::max(pl.grid, pl.grid_inst_fallback) * TB * sizeof(uint2));
    }
    // scene_bytes: the image in LDS (160-B nodes); class_bytes: what the class limits below are drawn in (144-B nodes, as they were measured:
    // lds_scene.h) -- the wider node moved no scene across a limit
    const size_t scene_bytes = lds_scene_bytes(s->n_wide, s->n_tris), class_bytes = lds_class_bytes(s->n_wide, s->n_tris);
    // (round 2's 128-B eight-wide node with fp16 planes visited 26 % fewer nodes and fetched as many 128-B LINES -- two 64-B
    // BVH4 siblings share one -- and lost: 458 vs 395 ms of kernel time per 4 frames of C5; the 64-B node above is its successor)
    const bool auto8 = want == PT_EXTEND_AUTO && class_bytes > 24 * 1024 && s->d_wide8 && (ctx->tune.hbm8 == 1 || auto8_big);
    if (want == PT_EXTEND_HBM8 || auto8) {
        pl.variant = PT_EXTEND_HBM8;
        pl.bvh8 = true;
        pl.lds_scene = false;
        // one stack entry per visited node: at most one per level of the 8-wide tree.  The LDS stack is sized to exactly that (8 M
        // triangles: 10 entries) -- then the kernel is instantiated without the spill column's address arithmetic (C5 +1.9 %, C5x
        // +2.5 %) and the LDS it does not take is there for the co-resident k_shade (9 ... 11 entries instead of 12: C5 +1 %; one
        // entry too few, i.e. the spill kernel: -1.7 %; profiles/r03bk_*, r03bl_*)
        const uint32_t bound8 = s->levels8 + 1u;
        pl.lds_stack = pt_tuned(ctx->tune.lds_stack, (int)std::min(std::max(bound8, 4u), 12u), 1, 32);
        pl.smem = (size_t)pl.lds_stack * TB * sizeof(uint2);
        const bool spills8 = bound8 > (uint32_t)pl.lds_stack;
        // 7 waves per SIMD where the walk waits on HBM (same rule as AUTO ray sorting: nodes + records beyond the Infinity Cache);
        // pt_tuning.extend_blocks = 6 / 7 forces either
        pl.waves7 = !spills8 && pl.lds_stack <= 10 &&
                    (ctx->tune.extend_blocks == 7 || (ctx->tune.extend_blocks < 0 && 64ull * s->n_wide8 + 64ull * s->n_tris > (256ull << 20)));
        int per_cu8 = 0;
        const pt_status rc8b = ptw_prepare_kernel(ctx, ptw_extend8_fn(false, spills8, pl.waves7), TB, pl.smem, &per_cu8);
        if (rc8b != PT_OK) return rc8b;
        // with the triangle vote at 16 lanes (launch_extend) the refill optimum moved from 32 idle lanes to 12: C5 2 907 ->
        // 3 240 Mrays/s, C5x 2 715 -> 2 960 for both together (profiles/r03bb_*, r03bc_*: 32: 3 025, 24: 3 140, 16: 3 230, 8: 3 235, 4: 3 170)
        pl.refill = pt_tuned(ctx->tune.refill, 12, 1, 64);
        pl.grid = ctx->num_cus * per_cu8;
        pl.spill_levels = bound8 > (uint32_t)pl.lds_stack ? bound8 - (uint32_t)pl.lds_stack : 0u;
        return ptw_reserve_spill(ctx, PT_MAX_PIPES * (size_t)std::max(pl.spill_levels, 1u) * (size_t)pl.grid * TB * sizeof(uint2));
    }
    if (want == PT_EXTEND_LDS && class_bytes > 96 * 1024) { ctx->err = "scene does not fit LDS"; return PT_ERR_UNSUPPORTED; }
    pl.lds_scene = want == PT_EXTEND_LDS || (want == PT_EXTEND_AUTO && class_bytes <= 24 * 1024);
    pl.variant = pl.lds_scene ? PT_EXTEND_LDS : PT_EXTEND_HBM;
    // deep trees of big scenes: 12 LDS entries measured best on the 1M-triangle soup (4: -15 %, 8: -3 %,
    // 16: -5 %, 24: -16 %: beyond 12 the extra LDS costs occupancy; 9/10/11, which would admit a 7th block per CU: -2.4 %)
    pl.lds_stack = pl.lds_scene ? LDS_STACK : 12;
    // LDS-resident scenes are small enough for an exact stack bound (lbvh_build.hip: wide_stack_need):
    // if it fits 16 LDS entries the kernel is instantiated without the spill path (Cornell: 9)
    // (the no-spill kernel packs child words into 14 bits: <= 2047 triangles, <= 8191 nodes, leaves of <= 4)
    pl.spill = !(pl.lds_scene && s->stack_need <= 16u && s->n_tris <= 2047u && s->n_wide <= 8191u);
    if (!pl.spill) pl.lds_stack = (int)std::max(s->stack_need, 1u);
    pl.pairs = !pl.spill && s->pair_leaves && ctx->tune.pair_kernel != 0;
    pl.smem_wide_entries = (size_t)pl.lds_stack * TB * sizeof(uint2) + (pl.lds_scene ? scene_bytes : 0);
    pl.smem = pl.spill ? pl.smem_wide_entries : compact_stack_bytes(TB, pl.lds_stack) + scene_bytes;  // (one-dword entries, level -1 in front: LaneStack)
    // every kernel ptw_launch_extend can take for this plan, with the LDS size it would be launched with: the 8-byte-entry kernels of a
    // compact plan (tmin <= 0), the instrumented twin, the shadow-ray twin of a compact kernel (NEE pipeline), the product kernel --
    // whose occupancy makes the grid of them all
    const auto kernel_of = [&](bool compact, bool count, bool shadow) {
        return pl.lds_scene ? reinterpret_cast<const void *>(pick_extend_lds(compact, pl.pairs, count, shadow)) : ptw_extend_hbm_fn(count, ctx->tune.rec64 != 0);
    };
    int per_cu = 0;
    pt_status rck = PT_OK;
    if (!pl.spill)
        for (const bool count : { false, true })
            if (rck == PT_OK) rck = ptw_prepare_kernel(ctx, kernel_of(false, count, false), TB, pl.smem_wide_entries);
    if (rck == PT_OK) rck = ptw_prepare_kernel(ctx, kernel_of(!pl.spill, true, false), TB, pl.smem);
    if (rck == PT_OK && !pl.spill) rck = ptw_prepare_kernel(ctx, kernel_of(true, false, true), TB, pl.smem);
    if (rck == PT_OK) rck = ptw_prepare_kernel(ctx, kernel_of(!pl.spill, false, false), TB, pl.smem, &per_cu);
    if (rck != PT_OK) return rck;
    per_cu = ptw_tuned_blocks(ctx, per_cu);
    // big scenes (vote-scheduled steps): 32 idle lanes measured best on C5 (16: -2.5 %, 48: -3 %)
    pl.refill = pt_tuned(ctx->tune.refill, pl.lds_scene ? REFILL_MIN_IDLE : 32, 1, 64);
    pl.grid = ctx->num_cus * per_cu;
    // the HBM variant of a scene whose traversed BVH4 is the collapsed LBVH walks the top-down layout of it
    pl.topdown4 = !pl.lds_scene && s->bvh4_builder != 1 && s->d_wide16t && ctx->tune.topdown4 != 0;
    // stack bound: the exact one of the BVH4 that is traversed when its builder computed it (small scenes; the
    // surface-area BVH4 is not bounded by the LBVH's height), else a BVH4 node pushes <= 3 entries per level and the
    // collapsed LBVH's wide height is <= binary height/2 + 1
    const uint32_t bound = pl.topdown4 ? 3u * s->levels4t + 1u
                           : s->stack_need != 0xFFFFFFFFu ? s->stack_need + 1u : 3u * (s->height_tree / 2u + 1u) + 1u;
    pl.spill_levels = bound > (uint32_t)pl.lds_stack ? bound - (uint32_t)pl.lds_stack : 0u;
    return ptw_reserve_spill(ctx, PT_MAX_PIPES * (size_t)std::max(pl.spill_levels, 1u) * (size_t)pl.grid * TB * sizeof(uint2));
}

void ptw_launch_extend(const ExtendPlan &pl, pt_scene *s, const float4 *rayA, const float2 *rayB, float4 *hit, uint32_t *hit_inst,
                       const uint32_t *count_in, uint32_t *count_zero, unsigned long long *stats, float tmin, float tmax, bool count,
                       bool raw_hit, hipStream_t st, int pipe, hipEvent_t ev0, hipEvent_t ev1, const uint32_t *perm, const float *ray_tmax)
{
    const int raw = raw_hit ? 1 : 0;  // hit records as (pos, V, W, det) for k_shade instead of (pos, t, u, v)
    // hipExtLaunchKernelGGL stamps THIS kernel's start/stop into ev0/ev1 (null = plain launch): under
    // two overlapping pipelines an event recorded between kernels would also count queueing time
    // each concurrently running extend kernel owns its own [spill_levels][grid*TB] region
    const size_t spill_off = (size_t)pipe * std::max(pl.spill_levels, 1u) * (size_t)pl.grid * TB;
    if (s->n_inst && pl.inst16 && tmin > 0.f) {
        // own region of the spill buffer, counted in dwords (the buffer is sized in 8-byte entries for the larger grid)
        uint32_t *sp32 = reinterpret_cast<uint32_t *>(reinterpret_cast<uint2 *>(s->ctx->d_spill) + (size_t)pipe * std::max(pl.spill_levels, 1u) * (size_t)std::max(pl.grid, pl.grid_inst_fallback) * TB);
        const uint32_t str = (uint32_t)pl.grid * TB;
        const int enter_min = pt_tuned(s->ctx->tune.enter_min, 16, 1, 64);  // lanes that wait to enter an instance together (8, 16, 24 measured alike within 1 %)
        // ... and lanes that wait with a triangle leaf (extend_inst16.h): 8 until round 6; on the BLAS with the least-area cut 8 / 12 / 14 / 20 -> 16.12 / 16.33 /
        // 16.34 / 16.19 Grays/s on the 10 000-instance grid (profiles/r06o_c4_wavefront_knobs.log)
        const int leaf_min = pt_tuned(s->ctx->tune.leaf_min, 14, 1, 64);
        // the node loop yields to the lanes waiting with a leaf once fewer than 1/6 of the wave's rays still descend
        // (C4 11.7 -> 12.2 Grays/s; 2, 3, 4, 8 measured within 1 % of it, 0 = never: profiles/r02i_ab_c4_node_yield.log)
        const int node_yield = pt_tuned(s->ctx->tune.node_yield, 6, 0, 64);
        hipExtLaunchKernelGGL(pick_extend_inst16(s->pair_leaves, count, ray_tmax != nullptr), dim3(pl.grid), dim3(TB), (uint32_t)pl.smem, st, ev0, ev1, 0u, s->d_tlas16,
                              norm_box_tlas(s), reinterpret_cast<const uint4 *>(s->d_wide16), norm_box_blas(s), s->d_tri4, s->n_wide, s->n_tris, s->d_inst6,
                              s->d_tlas_prim_of, rayA, rayB, hit, hit_inst, count_in, count_zero, stats, sp32, str, pl.refill, tmin,
                              tmax, raw, pl.lds_stack, enter_min, leaf_min, node_yield, pl.n_tlas_lds, ray_tmax);
        return;
    }
    if (s->n_inst) {
        const int grid_i = pl.inst16 ? pl.grid_inst_fallback : pl.grid;
        const size_t smem_i = pl.inst16 ? pl.smem_inst_fallback : pl.smem;
        uint2 *sp = reinterpret_cast<uint2 *>(s->ctx->d_spill) + (size_t)pipe * std::max(pl.spill_levels, 1u) * (size_t)std::max(pl.grid, pl.grid_inst_fallback) * TB;
        const uint32_t str = (uint32_t)grid_i * TB;
        hipExtLaunchKernelGGL(pick_extend_inst(pl.lds_scene, count, ray_tmax != nullptr), dim3(grid_i), dim3(TB), (uint32_t)smem_i, st, ev0, ev1, 0u, s->d_tlas_wide,
                              s->d_wide, s->d_tri4, s->n_wide, s->n_tris, s->d_inst6, s->d_tlas_prim_of, rayA, rayB, hit,
                              hit_inst, count_in, count_zero, stats, sp, str, pl.refill, tmin, tmax, raw, ray_tmax);
        return;
    }
    uint2 *spill = reinterpret_cast<uint2 *>(s->ctx->d_spill) + spill_off;
    const uint32_t stride = (uint32_t)pl.grid * TB;
    if (pl.bvh8) {
        // the vote of the 8-wide kernel (extend8_kernel.h): a triangle step runs once tri_enter lanes wait with leaf triangles
        // (or more than descend), and repeats while tri_stay lanes still hold one.  Majority voting (64) parks ~25 lanes
        // behind every node step -- a node step is 240 instructions, a triangle step 110: 16 measured best (8: -2 %, 12: -0.5 %,
        // 20: equal on C5x, 24: -3 %; repeating triangle steps changes nothing: profiles/r03ba_ab_c5_vote.log)
        const int tri_enter = pt_tuned(s->ctx->tune.tri_enter, 16, 1, 64), tri_stay = pt_tuned(s->ctx->tune.tri_stay, 65, 1, 65);
        ptw_launch_extend8(count, pl.spill_levels > 0u, pl.waves7, pl.grid, pl.smem, st, ev0, ev1, s->d_wide8, s->norm_c, s->norm_s, s->norm_rs, s->d_tri4_8, s->d_shade64_8, rayA, rayB, hit,
                           count_in, count_zero, stats, spill, stride, pl.refill | (tri_enter << 8) | (tri_stay << 16), tmin, tmax, pl.lds_stack, raw, perm, ray_tmax);
        return;
    }
    // one-dword stack entries truncate the entry distance toward zero, which is only conservative for t >= 0, and the
    // sort of the one-dword keys takes entry distances for positive floats (tmin = 0 could make one -0): a tmin <= 0
    // (not valid in Vulkan, accepted here) runs the same plan through the 8-byte-entry kernel
    const bool no_spill = !pl.spill && tmin > 0.f;
    const size_t smem = (!pl.spill && !no_spill) ? pl.smem_wide_entries : pl.smem;
    if (!pl.lds_scene) {
        ptw_launch_extend_hbm(count, s->ctx->tune.rec64 != 0, pl.grid, smem, st, ev0, ev1, s->d_wide, pl.topdown4 ? reinterpret_cast<const uint2 *>(s->d_wide16t) : s->d_wide16, s->norm_c, s->norm_s, s->norm_rs, s->d_tri4,
                              s->d_shade64, s->n_wide, s->n_tris, rayA, rayB, hit, count_in, count_zero, stats, spill, stride,
                              pl.refill | (pt_tuned(s->ctx->tune.tri_enter, 0, 0, 64) << 8), tmin, tmax, pl.lds_stack, raw, perm, ray_tmax);
        return;
    }
    hipExtLaunchKernelGGL(pick_extend_lds(no_spill, pl.pairs, count, ray_tmax != nullptr), dim3(pl.grid), dim3(TB), (uint32_t)smem, st, ev0, ev1, 0u, s->d_wide,
                          s->d_wide16, norm_box_blas(s), s->d_tri4, s->n_wide, s->n_tris, rayA, rayB, hit, count_in, count_zero, stats, spill, stride,
                          pl.refill, tmin, tmax, pl.lds_stack, raw, nullptr, ray_tmax, nullptr);
}
