// guided.hip -- pt_render_guided: the reduce kernel that folds the fused kernels' first-hit log into the guide planes, and the log itself.
//
// pt_render's fused kernels trace every camera ray as the first ray of its sample; with LOG (fused_kernel.h, fused_inst_kernel.h) they store
// that ray's hit.  k_guided_reduce, one thread per pixel of the launch's tile list, then does what k_aov_reduce does with the hit records of
// pt_render_aov's own trace (guided_kernel.h has the body): the second walk of the camera rays is not made.  render.hip drives both.
#include "wavefront_host.h"

namespace {
using namespace ptw;
#include "guided_kernel.h"

template <bool INST>
__global__ __launch_bounds__(TB) void k_guided_reduce(GdConst gc, const uint32_t *__restrict__ tiles, int32_t frame0, uint32_t n_frames, uint32_t id_frame,
                                                      const uint2 *__restrict__ log, GdScene sc, AovPlanes planes)
{
    const uint32_t local = blockIdx.x * TB + threadIdx.x;
    if (local >= gc.slots_per_lane) return;
    gd_reduce_pixel<INST>(gc, tiles, local, frame0, n_frames, id_frame, log, sc, planes);
}
}  // namespace

pt_status ptg_ensure_log(pt_film *f, size_t records)
{
    pt_film::Guided &g = f->gd;
    if (records <= g.cap) return PT_OK;
    const size_t held = g.cap * sizeof(uint2);
    g.cap = 0;
    const pt_status rc = pt_scratch_alloc(f->ctx, "first-hit log", { pt_buf_of(g.d_log, sizeof(uint2) * records) }, &g.bytes, held, f->work.bytes, f->ctx->mem_budget,
                                          ": fewer frames per launch fit");
    if (rc == PT_OK) g.cap = records;
    return rc;
}

void ptg_free(pt_film *f)
{
    pt_film::Guided &g = f->gd;
    pt_scratch_free({ pt_buf_of(g.d_log) }, &g.bytes, g.bytes);
    g = pt_film::Guided{};
}

void ptg_launch_reduce(const pt_scene *s, pt_film *f, const RenderConst &rc, const uint32_t *tiles, uint32_t id_frame, const float4 *inst_frame, hipStream_t st)
{
    const pt_film::Aov &a = f->aov;
    GdConst gc{};
    gc.width = rc.width; gc.height = rc.height; gc.spp = rc.spp;
    gc.slots_per_lane = rc.slots_per_lane;
    gc.n_tris = s->n_tris;
    gc.cull_on = rc.cull_on;
    std::copy(rc.cull, rc.cull + 4, gc.cull);
    const GdScene sc = { s->d_tri4, s->d_shade4, s->d_faces, s->d_inst6, inst_frame, s->d_tlas_prim_of };
    const AovPlanes planes = { static_cast<float *>(a.plane[PT_AOV_ALBEDO]), static_cast<float *>(a.plane[PT_AOV_NORMAL]), static_cast<float *>(a.plane[PT_AOV_EMISSION]),
                               static_cast<float *>(a.plane[PT_AOV_DEPTH]), static_cast<float *>(a.plane[PT_AOV_ALPHA]), static_cast<uint2 *>(a.plane[PT_AOV_ID]) };
    if (rc.slots_per_lane == 0u) return;
    const int grid = (int)((rc.slots_per_lane + TB - 1) / TB);
    if (s->n_inst) k_guided_reduce<true><<<grid, TB, 0, st>>>(gc, tiles, rc.frame_base, rc.lanes_active, id_frame, f->gd.d_log, sc, planes);
    else k_guided_reduce<false><<<grid, TB, 0, st>>>(gc, tiles, rc.frame_base, rc.lanes_active, id_frame, f->gd.d_log, sc, planes);
}
