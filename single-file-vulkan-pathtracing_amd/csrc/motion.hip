// motion.hip -- pt_scene_snapshot_previous and pt_film_motion: where the surface point of every pixel's first hit was before the geometry moved.
//
// The definition (the first hit put back into the world as pt_film_reproject does it, its barycentrics in the triangle the id plane names by
// orthogonal projection, the same barycentrics in the snapshot's triangle) is the header's; tests/test_motion.py restates it in numpy and every
// comparison is byte equality.  So every operation here is one binary32 operation in the written order (-ffp-contract=off, __fdiv_rn, the
// correctly rounded square root), and nothing is reassociated.
//
//   k_motion<INST>   one launch, the denoiser's block: 64 x 4 pixels, a wave one row of 64.  A pixel reads 16 B of guides (Z, a and the id pair),
//                    then gathers six float4 vertex records -- the triangle now (d_tri_orig) and in the snapshot -- and, with INST, the three
//                    rows of the instance's matrix now and in the snapshot; it writes one float4 of Q.  The indices are clamped into their
//                    arrays and a pixel whose ids name nothing is dropped by a select, so no load stands behind a lane's branch; the loaded
//                    values are pinned after the last load (MO_KEEP), as reproject.hip does it.  No LDS, no scratch.  Its body is mo_pixel
//                    (motion_kernel.h).  DESIGN.md section 16 has what the assembly shows.
#include "pt_internal.h"
#include "pt_math.h"
#include "wavefront_host.h"  // ptw_camera

#include <cmath>
#include <cstring>

namespace {

#define MO_KEEP(v) asm volatile("" : "+v"(v))  // the value exists in a vector register at this point: its load cannot move below
#include "motion_kernel.h"  // MoConst, MoScene, MoFilm, mo_pixel: the kernel's body

template <bool INST>
__global__ __launch_bounds__(TB) void k_motion(MoConst mc, MoScene sc, MoFilm fl)
{
    int x, y; fp_pixel(mc.n_bx, x, y);
    if (x >= (int)mc.w || y >= (int)mc.h) return;
    mo_pixel<INST>(mc, sc, fl, x, y);
}

using MoFn = decltype(&k_motion<false>);
MoFn pick_motion(bool inst) { return inst ? k_motion<true> : k_motion<false>; }

}  // namespace

void ptm_free_previous(pt_scene *s)
{
    pt_scratch_free(ptb_scene_buffers(s, PT_LIFE_PREVIOUS), nullptr, 0);
    s->prev = pt_scene::Previous{};
}

pt_status ptm_snapshot(pt_scene *s)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const pt_status rb = s->broken ? ptb_repair(s) : PT_OK;  // (as pt_render: a repair may bring back a parked instance set)
    if (rb != PT_OK) return rb;
    const uint32_t n_inst = s->n_inst;
    if (pt_given_instances(s) != (size_t)n_inst) { ctx->err = "pt_scene_snapshot_previous: the scene's instance set is incomplete"; return PT_ERR_UNSUPPORTED; }
    const size_t tri_bytes = sizeof(float4) * 3 * (size_t)s->n_tris, xf_bytes = sizeof(float4) * 3 * (size_t)n_inst;
    // both new copies are made first and swapped in at the end, the old ones freed after them: a call that fails at any point leaves the
    // previous snapshot -- triangles and matrices -- as it was
    // (so the set is allocated into locals: the allocator frees the set it is given first)
    float4 *d_tri = nullptr, *d_xf = nullptr;
    std::vector<pt_buf> fresh = { pt_buf_of(d_tri, tri_bytes) };
    if (n_inst) fresh.push_back(pt_buf_of(d_xf, 2 * xf_bytes));
    PT_TRY(ptb_scene_alloc(s, "the previous geometry", fresh));
    // ordered after the work queued on the stream (an update's gather, a render that still reads the triangles)
    hipError_t e = hipMemcpyAsync(d_tri, s->d_tri_orig, tri_bytes, hipMemcpyDeviceToDevice, st);
    // (the matrices as given: from the host copy, or device to device after pt_scene_set_instances_device)
    if (e == hipSuccess && n_inst && s->d_xforms) e = hipMemcpyAsync(d_xf, s->d_xforms, xf_bytes, hipMemcpyDeviceToDevice, st);
    else if (e == hipSuccess && n_inst) e = hipMemcpyAsync(d_xf, s->h_xforms.data(), xf_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        pt_scratch_free(fresh, nullptr, 0);
        ctx->err = std::string("pt_scene_snapshot_previous: ") + hipGetErrorString(e);
        return PT_ERR_HIP;
    }
    ptm_free_previous(s);
    s->prev.have = true;
    s->prev.d_tri = d_tri;
    s->prev.d_xf = d_xf;
    s->prev.n_inst = n_inst;
    s->prev.bytes = tri_bytes + 2 * xf_bytes;
    return PT_OK;
}

pt_status ptm_motion(pt_scene *s, pt_film *f, const pt_motion_params *p, float *device_ms)
{
    pt_ctx *ctx = s->ctx;
    // every refusal of the header, before anything is written
    if (f->ctx != ctx) return pt_bad(ctx, "scene and film belong to different contexts");
    if (!f->aov.enabled) return pt_bad(ctx, PT_NO_GUIDES_MSG);
    if (!f->mo.d) return pt_bad(ctx, PT_NO_Q_MSG " first");
    if (!s->prev.have) return pt_bad(ctx, "the scene has no previous geometry: pt_scene_snapshot_previous first");
    if (!pt_finite3(p->cam_origin) || !pt_finite3(p->cam_target)) return pt_bad(ctx, "pt_motion_params: the camera must be finite");
    if (!(std::isfinite(p->bary_slack) && p->bary_slack >= 0.f)) return pt_bad(ctx, "pt_motion_params.bary_slack must be finite and >= 0");
    PT_TRY(pt_check_reserved(ctx, "pt_motion_params", p->reserved));
    const pt_status rb = s->broken ? ptb_repair(s) : PT_OK;
    if (rb != PT_OK) return rb;
    const uint32_t n_inst = s->n_inst;
    if (n_inst != s->prev.n_inst) return pt_bad(ctx, "the scene's instance count differs from the snapshot's");
    if (pt_given_instances(s) != (size_t)n_inst) { ctx->err = "pt_film_motion: the scene's instance set is incomplete"; return PT_ERR_UNSUPPORTED; }
    MoConst mc{};
    mc.w = f->w; mc.h = f->h;
    const uint32_t n_blocks = fp_grid(f->w, f->h, &mc.n_bx);
    mc.n_tris = s->n_tris;
    mc.n_inst = n_inst ? n_inst : 1u;
    mc.cam = ptw_camera_of(p->cam_origin, p->cam_target, f->w, f->h);   // the camera pt_render and pt_render_aov start their rays from
    mc.slack = p->bary_slack;
    const size_t xf_rows = 3 * (size_t)n_inst;
    const MoScene sc = { s->d_tri_orig, s->prev.d_tri, n_inst ? s->prev.d_xf + xf_rows : nullptr, s->prev.d_xf };
    const pt_film::Aov &a = f->aov;
    const MoFilm fl = { static_cast<const float *>(a.plane[PT_AOV_DEPTH]), static_cast<const float *>(a.plane[PT_AOV_ALPHA]),
                        static_cast<const uint2 *>(a.plane[PT_AOV_ID]), f->mo.ptr() };
    hipStream_t st = ctx->stream;
    // the scene's matrices as they are now, in gl_InstanceID order, into the second half of the snapshot's array
    // (once per pt_scene_set_instances, not once per call; compared as bytes: -0 is not +0 here)
    // (after pt_scene_set_instances_device: device to device, once per set -- the scene's set counter decides, nothing is compared)
    if (n_inst && s->d_xforms) {
        if (s->prev.now_set != s->xf_set) {
            s->prev.h_now.clear();
            s->prev.now_set = 0;
            PT_HIP(ctx, hipMemcpyAsync(s->prev.d_xf + xf_rows, s->d_xforms, sizeof(float4) * xf_rows, hipMemcpyDeviceToDevice, st));
            PT_HIP(ctx, hipStreamSynchronize(st));
            s->prev.now_set = s->xf_set;
        }
    } else if (n_inst && (s->prev.h_now.size() != s->h_xforms.size() || std::memcmp(s->prev.h_now.data(), s->h_xforms.data(), sizeof(float) * s->h_xforms.size()) != 0)) {
        s->prev.h_now.clear();
        s->prev.now_set = 0;
        PT_HIP(ctx, hipMemcpyAsync(s->prev.d_xf + xf_rows, s->h_xforms.data(), sizeof(float4) * xf_rows, hipMemcpyHostToDevice, st));
        PT_HIP(ctx, hipStreamSynchronize(st));
        s->prev.h_now = s->h_xforms;
    }
    return pt_timed_pass(ctx, device_ms, [&](hipStream_t ts) { hipLaunchKernelGGL(pick_motion(n_inst != 0), dim3(n_blocks), dim3(TB), 0, ts, mc, sc, fl); });
}
