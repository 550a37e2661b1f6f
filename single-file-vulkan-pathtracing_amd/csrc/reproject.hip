// reproject.hip -- pt_film_reproject: a film rendered at a new camera takes over the history of a film rendered at the previous camera.
//
// The definition (the first hit put back into the world through primary_target at jitter (0.5, 0.5), its projection into the previous
// camera, the four bilinear taps in the order j outer / i inner with their validity terms, the blend by the history length, the bgra8 form)
// is the header's; tests/test_reproject.py restates it in numpy and every comparison is byte equality.  So every operation here is one
// binary32 operation in the written order (-ffp-contract=off, __fdiv_rn, the correctly rounded square root), and nothing is reassociated.
//
//   k_reproject<HAS_M>   one launch, the denoiser's block: 64 x 4 pixels, a wave one row of 64.  A pixel reads its own 44 B (+ 12 B of M)
//                        of `film`, projects, and then issues the loads of all four taps of `prev` -- C', (M',) L', Z', a', N' and the id
//                        pair at coordinates clamped into the image -- before any validity test; a tap that does not count is dropped
//                        by selects.  (loads behind a tap's branch serialise.)  The compiler needs help to keep that shape:
//                        the validity terms are flags combined with & (a && chain became branches with loads behind them), and the loaded
//                        values are pinned after the last load (RP_KEEP) -- section 15 has what the assembly shows.  No LDS, no scratch; the film is
//                        rewritten in place, a pixel touching no other pixel of it.  Its body is rp_pixel (reproject_kernel.h).
//   k_reproject_motion<HAS_M>   pt_film_reproject_motion: rp_pixel<HAS_M, true>.  The point that goes through the previous camera is read from
//                        the film's plane Q (16 B more per pixel) instead of being put back into the world from Z / a; everything after it is
//                        k_reproject's.  A kernel of its own with an argument of its own.
#include "pt_internal.h"
#include "pt_math.h"
#include "wavefront_host.h"  // ptw_camera

#include <cmath>

namespace {

#define RP_KEEP(v) asm volatile("" : "+v"(v))  // the value exists in a vector register at this point: its load cannot move below
#include "reproject_kernel.h"  // RpConst, RpFilm, RpPrev, rp_pixel: the kernel's body

template <bool HAS_M>
__global__ __launch_bounds__(TB) void k_reproject(RpConst rc, RpFilm fl, RpPrev pv)
{
    int x, y; fp_pixel(rc.n_bx, x, y);
    if (x >= (int)rc.w || y >= (int)rc.h) return;
    rp_pixel<HAS_M>(rc, fl, pv, x, y);
}

using RpFn = decltype(&k_reproject<false>);
RpFn pick_reproject(bool has_m) { return has_m ? k_reproject<true> : k_reproject<false>; }

// pt_film_reproject_motion: the same body started from the film's plane Q, which is an argument of these instantiations alone (k_reproject's
// argument block, and with it its scalar loads, stay as they are)
template <bool HAS_M>
__global__ __launch_bounds__(TB) void k_reproject_motion(RpConst rc, RpFilm fl, RpPrev pv, const float *__restrict__ motion)
{
    int x, y; fp_pixel(rc.n_bx, x, y);
    if (x >= (int)rc.w || y >= (int)rc.h) return;
    rp_pixel<HAS_M, true>(rc, fl, pv, x, y, motion);
}

using RpMotionFn = decltype(&k_reproject_motion<false>);
RpMotionFn pick_reproject_motion(bool has_m) { return has_m ? k_reproject_motion<true> : k_reproject_motion<false>; }

// every refusal of the header, in one place; nothing is written before it returns PT_OK
pt_status rp_validate(pt_film *f, pt_film *prev, const pt_reproject_params *p, bool motion)
{
    pt_ctx *ctx = f->ctx;
    if (prev == f) return pt_bad(ctx, "pt_film_reproject: prev is the film itself (the history is read while the film is rewritten: two films, ping-ponged)");
    if (!f->aov.enabled) return pt_bad(ctx, PT_NO_GUIDES_MSG);
    if (!f->hist.d) return pt_bad(ctx, PT_NO_L_MSG " first");
    if (motion && !f->mo.d) return pt_bad(ctx, PT_NO_Q_MSG " (and pt_film_motion) first");
    if (prev) {
        if (prev->ctx != ctx) return pt_bad(ctx, "film and prev belong to different contexts");
        if (prev->w != f->w || prev->h != f->h) return pt_bad(ctx, "film and prev differ in size");
        if (!prev->aov.enabled) return pt_bad(ctx, "prev has no guide buffers: pt_film_enable_aov (and pt_render_aov) first");
        if (!prev->hist.d) return pt_bad(ctx, "prev has no history-length plane: pt_film_enable_history first");
        if ((prev->m2.d != nullptr) != (f->m2.d != nullptr)) return pt_bad(ctx, "exactly one of film and prev has a second-moment plane: both or neither");
    }
    if (!pt_finite3(p->cam_origin) || !pt_finite3(p->cam_target) || !pt_finite3(p->prev_cam_origin) || !pt_finite3(p->prev_cam_target))
        return pt_bad(ctx, "pt_reproject_params: the cameras must be finite");
    if (!(std::isfinite(p->gain) && p->gain > 0.f)) return pt_bad(ctx, "pt_reproject_params.gain must be finite and > 0");
    if (!(p->alpha >= 0.f && p->alpha <= 1.f)) return pt_bad(ctx, "pt_reproject_params.alpha must be in [0, 1]");
    if (!(std::isfinite(p->depth_tol) && p->depth_tol > 0.f)) return pt_bad(ctx, "pt_reproject_params.depth_tol must be finite and > 0");
    if (!(p->normal_min >= -1.f && p->normal_min <= 1.f)) return pt_bad(ctx, "pt_reproject_params.normal_min must be in [-1, 1]");
    if (p->max_history < 1 || p->max_history > 65535) return pt_bad(ctx, "pt_reproject_params.max_history must be in 1..65535");
    if (p->flags & ~(uint32_t)PT_REPROJECT_MATCH_ID) return pt_bad(ctx, "pt_reproject_params.flags: unknown bits");
    return pt_check_reserved(ctx, "pt_reproject_params", p->reserved);
}

}  // namespace

pt_status ptr_reproject(pt_film *f, pt_film *prev, const pt_reproject_params *p, float *device_ms, bool motion)
{
    pt_ctx *ctx = f->ctx;
    PT_TRY(rp_validate(f, prev, p, motion));
    RpConst rc{};
    rc.w = f->w; rc.h = f->h;
    const uint32_t n_blocks = fp_grid(f->w, f->h, &rc.n_bx);
    rc.match_id = p->flags & PT_REPROJECT_MATCH_ID;
    rc.cam = ptw_camera_of(p->cam_origin, p->cam_target, f->w, f->h);   // the camera pt_render and pt_render_aov start their rays from
    rc.pox = p->prev_cam_origin[0]; rc.poy = p->prev_cam_origin[1]; rc.poz = p->prev_cam_origin[2];
    rc.ptx = p->prev_cam_target[0]; rc.pty = p->prev_cam_target[1]; rc.ptz = p->prev_cam_target[2];
    rc.gain = p->gain; rc.alpha = p->alpha; rc.depth_tol = p->depth_tol; rc.normal_min = p->normal_min;
    rc.max_history = (float)p->max_history;
    const pt_film::Aov &a = f->aov;
    const RpFilm fl = { f->d_rgb, f->m2.ptr(), f->hist.ptr(), reinterpret_cast<uchar4 *>(f->d_bgra), static_cast<const float *>(a.plane[PT_AOV_NORMAL]),
                        static_cast<const float *>(a.plane[PT_AOV_DEPTH]), static_cast<const float *>(a.plane[PT_AOV_ALPHA]),
                        static_cast<const uint2 *>(a.plane[PT_AOV_ID]) };
    RpPrev pv{};
    if (prev) {
        const pt_film::Aov &b = prev->aov;
        pv = { prev->d_rgb, prev->m2.ptr(), prev->hist.ptr(), static_cast<const float *>(b.plane[PT_AOV_NORMAL]), static_cast<const float *>(b.plane[PT_AOV_DEPTH]),
               static_cast<const float *>(b.plane[PT_AOV_ALPHA]), static_cast<const uint2 *>(b.plane[PT_AOV_ID]) };
    }
    return pt_timed_pass(ctx, device_ms, [&](hipStream_t st) {
        if (motion) hipLaunchKernelGGL(pick_reproject_motion(f->m2.d != nullptr), dim3(n_blocks), dim3(TB), 0, st, rc, fl, pv, reinterpret_cast<const float *>(f->mo.d));
        else hipLaunchKernelGGL(pick_reproject(f->m2.d != nullptr), dim3(n_blocks), dim3(TB), 0, st, rc, fl, pv);
    });
}
