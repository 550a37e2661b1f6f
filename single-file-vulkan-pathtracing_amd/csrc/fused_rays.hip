// fused_rays.hip -- pt_radiance_device with PT_RADIANCE_FUSED: the fused kernels started from the caller's rays (fused_kernel.h, RAYS) and their launch.
// A translation unit of its own, like fused_guided.hip, so that fused.hip compiles what it compiled before.  The plan is fused.hip's
// (ptw_plan_fused: same LDS, same block, same launch bounds, same grid); this unit adds the four kernels and the launcher.
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
static_assert(PTW_FUSED_COUNT_BYTES == sizeof(uint32_t) * PT_FUSED_PARTS * PT_FUSED_PART_STRIDE, "wavefront_host.h sizes the slot counters the kernel draws from");

// ---- one picker per kernel family (wavefront_host.h): the launch prepares what it returns, then launches it
using FusedRaysFn = decltype(&k_fused_rays<true>);
FusedRaysFn pick_fused_rays(bool pairs) { return pairs ? k_fused_rays<true> : k_fused_rays<false>; }
using FusedNeeRaysFn = decltype(&k_fused_nee_rays<true>);
FusedNeeRaysFn pick_fused_nee_rays(bool pairs) { return pairs ? k_fused_nee_rays<true> : k_fused_nee_rays<false>; }
}  // namespace

pt_status ptw_launch_fused_rays(const FusedPlan &fp, const ptw::RenderConst &rc, const ptw::Radiance &rad, const pt_scene *s, uint32_t *next_slot, unsigned long long *stats,
                                float tmin, float tmax, const float *rays6, const uint32_t *seeds, uint32_t m, uint32_t spp, uint32_t index0, uint32_t seed_m0,
                                hipStream_t st)
{
    pt_ctx *ctx = s->ctx;
    if (fp.inst || fp.count) { ctx->err = "PT_RADIANCE_FUSED: single-level scenes, no instrumented twin"; return PT_ERR_UNSUPPORTED; }
    const RdRays rays = { rays6, seeds, m, spp, index0, seed_m0 };
    const uint32_t n_slots = rdf_launch_slots(rc.n_slots);  // (rc.n_slots = m * spp, the live slots; the kernel masks the rounding's excess)
    FastDiv div_m;
    div_m.init(std::max(m, 1u));
    if (fp.nee) {
        const FusedNeeRaysFn fn = pick_fused_nee_rays(fp.pairs);
        PT_TRY(ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(fn), FTB, fp.smem));
        hipLaunchKernelGGL(fn, dim3(fp.grid), dim3(FTB), (uint32_t)fp.smem, st, rc, rad, s->d_wide, s->d_tri4, s->d_shade4, s->d_frame4, s->n_wide, s->n_tris, n_slots,
                           next_slot, stats, fp.refill, tmin, tmax, fp.lds_stack, div_m, s->d_lights, s->n_lights, s->light_area, rays);
        return PT_OK;
    }
    const FusedRaysFn fn = pick_fused_rays(fp.pairs);
    PT_TRY(ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(fn), FTB, fp.smem));
    hipLaunchKernelGGL(fn, dim3(fp.grid), dim3(FTB), (uint32_t)fp.smem, st, rc, rad, s->d_wide, s->d_tri4, s->d_shade4, s->d_frame4, s->n_wide, s->n_tris, n_slots, next_slot,
                       stats, fp.refill, tmin, tmax, fp.lds_stack, div_m, ptsl::launch_c1(tmin), rays);
    return PT_OK;
}
