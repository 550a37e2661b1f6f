// fused_guided.hip -- pt_render_guided: the fused kernels with the first-hit log (fused_kernel.h / fused_inst_kernel.h, LOG) and their launch.
// A translation unit of its own, so that fused.hip compiles what it compiled before in the time it took before.  The plan is fused.hip's
// (ptw_plan_fused: same LDS, same block, same launch bounds, so the same blocks per CU); this unit adds the kernels and the launcher.
#include "wavefront_host.h"

#include <algorithm>

#define PT_EXTEND_TEMPLATES_ONLY
#include "extend_kernel.h"
#include "extend_inst16.h"
#include "fused_cull.h"
#include "nee_sample.h"
#include "self_leaf.h"

namespace {
using namespace ptw;
#include "guided_kernel.h"
#include "fused_dev.h"
#include "fused_kernel.h"
#define PT_FUSEDI_LOG 1  // (this unit's copy of the two-level kernel is k_fused_inst_log)
#include "fused_inst_kernel.h"

// ---- one picker per kernel family (wavefront_host.h): the launch prepares what it returns, then launches it
using FusedLogFn = decltype(&k_fused_log<0, true>);
template <int MODE> FusedLogFn pick_fused_log_mode(bool pairs) { return pairs ? k_fused_log<MODE, true> : k_fused_log<MODE, false>; }
FusedLogFn pick_fused_log(int mode, bool pairs) { return mode == 2 ? pick_fused_log_mode<2>(pairs) : mode == 1 ? pick_fused_log_mode<1>(pairs) : pick_fused_log_mode<0>(pairs); }
using FusedNeeLogFn = decltype(&k_fused_nee_log<true>);
FusedNeeLogFn pick_fused_nee_log(bool pairs) { return pairs ? k_fused_nee_log<true> : k_fused_nee_log<false>; }
using FusedInstLogFn = decltype(&k_fused_inst_log<false, true>);
FusedInstLogFn pick_fused_inst_log(bool grouped, bool pairs)
{
    if (grouped) return pairs ? k_fused_inst_log<true, true> : k_fused_inst_log<true, false>;
    return pairs ? k_fused_inst_log<false, true> : k_fused_inst_log<false, false>;
}
}  // namespace

pt_status ptw_launch_fused_log(const FusedPlan &fp, int mode, const ptw::FastDiv &div_frames, const ptw::RenderConst &rc, const uint32_t *tiles, const ptw::Radiance &rad, const pt_scene *s,
                               uint32_t n_slots, uint32_t *next_slot, unsigned long long *stats, float tmin, float tmax, uint2 *log, hipStream_t st)
{
    pt_ctx *ctx = s->ctx;
    if (fp.inst) {
        const FusedInstLogFn fn = pick_fused_inst_log(mode == 1, s->pair_leaves);
        PT_TRY(ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(fn), FITB, fp.smem));
        hipLaunchKernelGGL(fn, dim3(fp.grid), dim3(FITB), (uint32_t)fp.smem, st, rc, tiles, rad, s->d_tlas16, norm_box_tlas(s), reinterpret_cast<const uint4 *>(s->d_wide16),
                           norm_box_blas(s), s->d_tri4, s->d_shade4, s->n_wide, s->n_tris, s->d_inst6, s->d_tlas_prim_of, fp.inst_frame, 0u, n_slots, next_slot, stats,
                           fp.spill, (uint32_t)fp.grid * FITB, fp.refill, tmin, tmax, fp.lds_stack, fp.enter_min, fp.leaf_min, fp.node_yield, fp.n_tlas_lds, log);
        return PT_OK;
    }
    if (fp.nee) {
        if (mode != 0) { ctx->err = "PT_FLAG_NEE on the fused pipeline: one sample group only"; return PT_ERR_UNSUPPORTED; }
        const FusedNeeLogFn fn = pick_fused_nee_log(fp.pairs);
        PT_TRY(ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(fn), FTB, fp.smem));
        hipLaunchKernelGGL(fn, dim3(fp.grid), dim3(FTB), (uint32_t)fp.smem, st, rc, tiles, rad, s->d_wide, s->d_tri4, s->d_shade4, s->d_frame4, s->n_wide, s->n_tris, 0u,
                           n_slots, next_slot, stats, fp.refill, tmin, tmax, fp.lds_stack, div_frames, s->d_lights, s->n_lights, s->light_area, log);
        return PT_OK;
    }
    const FusedLogFn fn = pick_fused_log(mode, fp.pairs);
    PT_TRY(ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(fn), FTB, fp.smem));
    hipLaunchKernelGGL(fn, dim3(fp.grid), dim3(FTB), (uint32_t)fp.smem, st, rc, tiles, rad, s->d_wide, s->d_tri4, s->d_shade4, s->d_frame4, s->n_wide, s->n_tris, 0u, n_slots,
                       next_slot, stats, fp.refill, tmin, tmax, fp.lds_stack, div_frames, ptsl::launch_c1(tmin), log);
    return PT_OK;
}
