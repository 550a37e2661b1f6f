// fused.hip -- PT_PIPELINE_FUSED: the kernel (fused_kernel.h), the scenes it takes, its launch.
#include "wavefront_host.h"

#include <algorithm>

#define PT_EXTEND_TEMPLATES_ONLY
#include "extend_kernel.h"  // the LDS node / stack helpers the fused kernel shares with k_extend_lds7p
#include "extend_inst16.h"  // the two-level walk's node codes and register barrier (k_extend_inst16 itself is a template: not instantiated here)

#ifdef PT_FUSED_TIMELINE
__device__ unsigned long long *g_fused_timeline = nullptr;
extern "C" int pt_debug_fused_timeline(void *device_u64x4_per_wave)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_fused_timeline), &device_u64x4_per_wave, sizeof(void *));
}
#endif

#ifdef PT_FUSED_HIST
__device__ uint32_t *g_fused_hist = nullptr;
extern "C" int pt_debug_fused_hist(void *device_u32_2x8192x16)
{
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_fused_hist), &device_u32_2x8192x16, sizeof(void *));
}
#endif

#include "fused_cull.h"
#include "nee_sample.h"  // the light sample of k_fused_nee (shared with k_shade)
#include "self_leaf.h"   // which bounce rays leave out the leaf they start on (the per-triangle part: scene_build.hip)

namespace {
using namespace ptw;
#include "guided_kernel.h"  // (the first-hit log's index: the kernels with LOG are fused_guided.hip's)
#include "fused_dev.h"
#include "fused_kernel.h"
#include "fused_inst_kernel.h"
constexpr size_t FUSED_COUNT_LDS = sizeof(uint32_t) * 2 * FB_N * (FTB / 64);  // the instrumented twin's per-wave block counters, behind the product plan
static_assert((int)FB_N == (int)PT_FB_COUNT && FB_N <= PT_N_BLOCKS, "fused_kernel.h FusedBlock mirrors include/pt_api.h pt_fused_block");

// ---- one picker per kernel family: the plan prepares what it returns, the launch launches it ---------------------------------------
// mode: 0 one sample group, 1 several, 2 head + tail slots; count: the instrumented twin (pair-leaf trees: what the compact class gets by default)
using FusedFn = decltype(&k_fused<0, true>);
template <int MODE>
FusedFn pick_fused_mode(bool pairs, bool count)
{
    if (count) return k_fused_count<MODE, true>;
    return pairs ? k_fused<MODE, true> : k_fused<MODE, false>;
}
FusedFn pick_fused(int mode, bool pairs, bool count)
{
    return mode == 2 ? pick_fused_mode<2>(pairs, count) : mode == 1 ? pick_fused_mode<1>(pairs, count) : pick_fused_mode<0>(pairs, count);
}
using FusedNeeFn = decltype(&k_fused_nee<true>);
FusedNeeFn pick_fused_nee(bool pairs) { return pairs ? k_fused_nee<true> : k_fused_nee<false>; }
using FusedInstFn = decltype(&k_fused_inst<false, true>);
FusedInstFn pick_fused_inst(bool grouped, bool pairs)
{
    if (grouped) return pairs ? k_fused_inst<true, true> : k_fused_inst<true, false>;
    return pairs ? k_fused_inst<false, true> : k_fused_inst<false, false>;
}

// Blocks per CU of a fused plan, remembered per context and family (pt_ctx::fused_smem: 0 single-level, 1 two-level, 2 single-level NEE)
// for the last LDS size and leaf kind: `prepare(per_cu)` -- ptw_prepare_kernel on every kernel the family's picker returns for the plan --
// runs only when they change.
template <class Prepare>
pt_status fused_blocks_per_cu(pt_ctx *ctx, int family, size_t smem, bool pairs, int &per_cu, Prepare &&prepare)
{
    const size_t key = (smem << 1) | (pairs ? 1u : 0u);
    if (ctx->fused_smem[family] != key || ctx->fused_per_cu[family] <= 0) {
        int n = 0;
        const pt_status rc = prepare(&n);
        if (rc != PT_OK) return rc;
        ctx->fused_smem[family] = key;
        ctx->fused_per_cu[family] = n;
    }
    per_cu = ptw_tuned_blocks(ctx, ctx->fused_per_cu[family]);
    return PT_OK;
}

// two-level scenes: k_extend_inst16's class (extend_launch.hip: both levels in 15-bit child codes, BLAS in LDS, pair leaves)
pt_status plan_fused_inst(pt_scene *s, const ExtendPlan &pl, float tmin, FusedPlan &fp)
{
    pt_ctx *ctx = s->ctx;
    const size_t tables = sizeof(float4) * 3 * (size_t)s->n_tris;  // shade4 (the vertices are the kz = 2 triangle copy)
    if (!pl.inst16 || !(tmin > 0.f) || tables > 16 * 1024) {
        ctx->err = "PT_PIPELINE_FUSED takes instanced scenes of the fp16 two-level kernel's class: 2 .. 32767 instances, a BLAS of <= 2047 "
                   "triangles that fits LDS, tmin > 0";
        return PT_ERR_UNSUPPORTED;
    }
    fp.inst = true;
    fp.lds_stack = pl.lds_stack;
    // TLAS nodes staged in LDS: the wavefront kernel keeps 8 KB of them because the other pipeline's k_shade needs LDS beside it
    // (extend_launch.hip); this kernel has the CU to itself
    const size_t tlas_lds_bytes = (size_t)pt_tuned(ctx->tune.tlas_lds_kb, PT_FUSEDI_TLAS_KB, 0, 96) * 1024;
    fp.n_tlas_lds = (uint32_t)std::min<size_t>(s->n_tlas16, tlas_lds_bytes / lds_nodes16_bytes(1));
    fp.smem = (size_t)fp.lds_stack * FITB * sizeof(uint32_t) + lds_nodes16_bytes((size_t)s->n_wide + fp.n_tlas_lds) + lds_tris_bytes(s->n_tris) + tables +
              sizeof(uint32_t) * FS_FIELDS * FITB + sizeof(uint32_t) * (FITB / 64) * PT_FUSED_WTILES;
    if (fp.smem > 160 * 1024) { ctx->err = "PT_PIPELINE_FUSED: the two-level kernel's LDS plan exceeds 160 KB (pt_tuning lds_stack / tlas_lds_kb)"; return PT_ERR_UNSUPPORTED; }
    int per_cu = 0;
    const pt_status rcp = fused_blocks_per_cu(ctx, 1, fp.smem, s->pair_leaves, per_cu, [&](int *n) {  // (the grid: the ungrouped kernel's occupancy)
        const pt_status rcg = ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_fused_inst(true, s->pair_leaves)), FITB, fp.smem);
        return rcg != PT_OK ? rcg : ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_fused_inst(false, s->pair_leaves)), FITB, fp.smem, n);
    });
    if (rcp != PT_OK) return rcp;
    fp.grid = ctx->num_cus * per_cu;
    fp.block = FITB;
    fp.refill = pt_tuned(ctx->tune.refill, 48, 1, 64);
    // the waiting rules of k_extend_inst16 (extend_launch.hip has the measurements), re-swept for this kernel in round 6 on the tree with the
    // least-area cut (leaves are reached a node earlier): a leaf step waits for 14 lanes (8 / 10 / 12 / 14 / 20 / 24: 16.42 / 16.60 / 16.72 / 16.76 /
    // 16.52 / 16.32 Grays/s on the 10 000-instance grid at 16 frames), an instance entry for 12 (profiles/r06m_c4_fused_knobs.log)
    fp.enter_min = pt_tuned(ctx->tune.enter_min, 12, 1, 64);
    fp.leaf_min = pt_tuned(ctx->tune.leaf_min, 14, 1, 64);
    fp.node_yield = pt_tuned(ctx->tune.node_yield, 6, 0, 64);
    // stack entries beyond the LDS ones: one dword each, [level][thread], in the context's spill area (sized by ptw_plan_extend for
    // the wavefront kernels' grids; grown here if this grid asks for more)
    const pt_status rcs = ptw_reserve_spill(ctx, (size_t)std::max(pl.spill_levels, 1u) * (size_t)fp.grid * FITB * sizeof(uint32_t));
    if (rcs != PT_OK) return rcs;
    fp.spill = reinterpret_cast<uint32_t *>(ctx->d_spill);
    if (ctx->tune.inst_frames != 0) {
        const pt_status rcf = ptb_ensure_inst_frames(s);
        if (rcf != PT_OK) return rcf;
        fp.inst_frame = s->d_inst_frame;
    }
    return PT_OK;
}
}  // namespace

pt_status ptw_plan_fused(pt_scene *s, const ExtendPlan &pl, float tmin, FusedPlan &fp, bool nee)
{
    pt_ctx *ctx = s->ctx;
    if (s->n_inst && nee) {
        ctx->err = "PT_PIPELINE_FUSED with PT_FLAG_NEE is for single-level scenes (instanced scenes: PT_PIPELINE_WAVEFRONT_NEE)";
        return PT_ERR_UNSUPPORTED;
    }
    if (s->n_inst) return plan_fused_inst(s, pl, tmin, fp);
    const size_t tables = sizeof(float4) * 5 * (size_t)s->n_tris;  // shade4 + tangent frames (the vertices are the kz = 2 triangle copy)
    if (pl.variant != PT_EXTEND_LDS || pl.spill || !(tmin > 0.f) || tables > 16 * 1024) {
        ctx->err = "PT_PIPELINE_FUSED is for single-level scenes whose BVH4, triangles and shading tables fit LDS (the compact "
                   "kernels' class: <= 2047 triangles in <= 24 KB, stack bound <= 16, tmin > 0)";
        return PT_ERR_UNSUPPORTED;
    }
    // (the plan gives the stack one level in front of level 0: the BOTTOM entry every pop may take -- fused_lds)
    fp.lds_stack = pl.lds_stack;
    fp.smem = fused_lds(s->n_wide, s->n_tris, (uint32_t)fp.lds_stack).extra;
    fp.pairs = pl.pairs;
    fp.block = FTB;
    int per_cu = 0;
    pt_status rcp;
    if (nee) {  // k_fused_nee: the shadow ray's state behind the waves' tile words (fused_kernel.h FS_NEE_*), and the occupancy of that plan
        fp.nee = true;
        fp.smem += sizeof(uint32_t) * FS_NEE_FIELDS * FTB;
        rcp = fused_blocks_per_cu(ctx, 2, fp.smem, pl.pairs, per_cu,
                                  [&](int *n) { return ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_fused_nee(pl.pairs)), FTB, fp.smem, n); });
    } else {
        // the three sample-group modes and their instrumented twins (FUSED_COUNT_LDS on top) share the launch shape: the grid comes from mode 0's product kernel
        rcp = fused_blocks_per_cu(ctx, 0, fp.smem, pl.pairs, per_cu, [&](int *n) {
            pt_status rc = PT_OK;
            for (int mode = 2; mode >= 0 && rc == PT_OK; mode--) {
                rc = ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_fused(mode, pl.pairs, true)), FTB, fp.smem + FUSED_COUNT_LDS);
                if (rc == PT_OK) rc = ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_fused(mode, pl.pairs, false)), FTB, fp.smem, mode == 0 ? n : nullptr);
            }
            return rc;
        });
    }
    if (rcp != PT_OK) return rcp;
    fp.grid = ctx->num_cus * per_cu;
    // of 64: the share of a wave's live lanes that must wait with a finished ray before the shade block runs for them.  The block
    // is ~4x a node step, so it pays to run it fuller than k_extend's refill (16): 8 / 16 / 24 / 32 / 40 -> 33.9 / 34.1 / 34.6 /
    // 35.7 / 36.3 Grays/s on the Cornell box at 1080p (profiles/r04b_fused_refill_sweep.txt).  Round 6, after the shade block lost a fifth of
    // its instructions (the shared spawn steps) and the tree a node: 32 / 36 / 40 / 44 / 48 -> 73.1 / 73.1 / 73.8 / 75.1 / 76.1 ms per 16 frames,
    // one blocking frame 5.48 / 5.45 / 5.43 / 5.47 / 5.52 (profiles/r06l_refill_exit_resweep.log): 36.  NEE: the same value, not swept
    fp.refill = pt_tuned(ctx->tune.refill, 36, 1, 64);
    return PT_OK;
}

void ptw_launch_fused(const FusedPlan &fp, int mode, const ptw::FastDiv &div_frames, const ptw::RenderConst &rc, const uint32_t *tiles, const ptw::Radiance &rad,
                      const pt_scene *s, uint32_t n_slots, uint32_t *next_slot, unsigned long long *stats, float tmin, float tmax,
                      hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    if (fp.inst) {  // (never head + tail: mode 0 or 1)
        hipExtLaunchKernelGGL(pick_fused_inst(mode == 1, s->pair_leaves), dim3(fp.grid), dim3(FITB), (uint32_t)fp.smem, st, ev0, ev1, 0u, rc, tiles, rad, s->d_tlas16,
                              norm_box_tlas(s), reinterpret_cast<const uint4 *>(s->d_wide16), norm_box_blas(s), s->d_tri4, s->d_shade4, s->n_wide, s->n_tris, s->d_inst6,
                              s->d_tlas_prim_of, fp.inst_frame, 0u, n_slots, next_slot, stats, fp.spill, (uint32_t)fp.grid * FITB, fp.refill,
                              tmin, tmax, fp.lds_stack, fp.enter_min, fp.leaf_min, fp.node_yield, fp.n_tlas_lds);
        return;
    }
    if (fp.nee) {  // (one sample group, no head + tail: render.hip never plans another shape for it)
        if (mode != 0) return;
        hipExtLaunchKernelGGL(pick_fused_nee(fp.pairs), dim3(fp.grid), dim3(FTB), (uint32_t)fp.smem, st, ev0, ev1, 0u, rc, tiles, rad, s->d_wide, s->d_tri4, s->d_shade4,
                              s->d_frame4, s->n_wide, s->n_tris, 0u, n_slots, next_slot, stats, fp.refill, tmin, tmax, fp.lds_stack, div_frames, s->d_lights,
                              s->n_lights, s->light_area);
        return;
    }
    hipExtLaunchKernelGGL(pick_fused(mode, fp.pairs, fp.count), dim3(fp.grid), dim3(FTB), (uint32_t)(fp.smem + (fp.count ? FUSED_COUNT_LDS : 0)), st, ev0, ev1, 0u, rc, tiles,
                          rad, s->d_wide, s->d_tri4, s->d_shade4, s->d_frame4, s->n_wide, s->n_tris, 0u, n_slots, next_slot, stats, fp.refill, tmin, tmax, fp.lds_stack,
                          div_frames, ptsl::launch_c1(tmin));
}
