// upsample.hip -- pt_film_upsample: a low-resolution radiance film brought to the size of a film that holds full-size guides.
//
// The definition (lo's demodulated records, the position of a full-size pixel in lo's image, the four bilinear taps in the order j outer /
// i inner weighted by pt_film_denoise's t^16 of the guides, the 4 x 4 second ring by the guides alone, the nearest tap, remodulation with
// the full-size albedo and emission, the bgra8 form) is the header's; tests/test_upsample.py restates it in numpy and every comparison is
// byte equality.  So every operation here is one binary32 operation in the written order (-ffp-contract=off, __fdiv_rn), and nothing is
// reassociated.
//
//   k_dn_prepare   denoise.hip's kernel, unchanged, over lo (ptd_prepare_records): lo's film or its denoised plane and lo's guides -> two
//                  16-B records per lo pixel in lo's denoiser scratch, illum {I'.rgb, 0} and guide {N'.xyz, Z'}.
//   k_upsample     one launch over the full-size film, the film passes' block: 64 x 4 pixels, a wave one row of 64.  A lane loads its own
//                  44 B of guides, then the eight 128-bit loads of its four first-ring taps from addresses clamped into lo's image, ahead of
//                  any test; taps outside the image are dropped by selects (flags combined with &, loaded values pinned by UP_KEEP).  One
//                  wave-wide vote on den >= 0.01f takes the wave into the second ring only when a lane needs it (the shape of
//                  k_dn_var_spatial's vote); there the nearest tap and, row by row, the eight loads of a row of taps are issued together,
//                  and a lane that did not fall back keeps its first-ring result by a select.  No LDS, no scratch.  Its body is up_pixel
//                  (upsample_kernel.h).
#include "pt_internal.h"
#include "pt_math.h"

#include <cmath>

namespace {

#define DH_KEEP(v) asm volatile("" : "+v"(v))  // (wanted by denoise_history_kernel.h, whose dn_demod and dn_guide_x the body uses)
#define UP_KEEP(v) asm volatile("" : "+v"(v))  // the value exists in a vector register at this point: its load cannot move below
#define UP_ANY(b) (__builtin_amdgcn_ballot_w64(b) != 0)  // the lanes of a wave are one row's pixels inside the image
#include "upsample_kernel.h"  // UpConst, UpGuides, UpLo, UpOut, up_pixel: the kernel's body

__global__ __launch_bounds__(TB) void k_upsample(UpConst uc, UpGuides gd, UpLo lo, UpOut o)
{
    int x, y; fp_pixel(uc.n_bx, x, y);
    if (x >= (int)uc.w || y >= (int)uc.h) return;
    up_pixel(uc, gd, lo, o, x, y);
}

// every refusal of the header, in one place; nothing is written before it returns PT_OK
pt_status up_validate(pt_film *f, pt_film *lo, const pt_upsample_params *p)
{
    pt_ctx *ctx = f->ctx;
    if (lo == f) return pt_bad(ctx, "pt_film_upsample: lo is the film itself (two films: the full-size guides and the low-resolution radiance)");
    if (lo->ctx != ctx) return pt_bad(ctx, "film and lo belong to different contexts");
    if (lo->w > f->w || lo->h > f->h) return pt_bad(ctx, "pt_film_upsample: lo is larger than the film");
    if (!f->aov.enabled) return pt_bad(ctx, PT_NO_GUIDES_MSG);
    if (!lo->aov.enabled) return pt_bad(ctx, "lo has no guide buffers: pt_film_enable_aov (and pt_render_aov) first");
    if (p->source != PT_UPSAMPLE_SRC_FILM && p->source != PT_UPSAMPLE_SRC_DENOISED) return pt_bad(ctx, "pt_upsample_params.source: unknown value");
    if (p->source == PT_UPSAMPLE_SRC_DENOISED && !lo->dn.have_out)
        return pt_bad(ctx, "PT_UPSAMPLE_SRC_DENOISED: lo has no denoised image (pt_film_denoise with a NULL output first)");
    PT_TRY(pt_check_sigmas(ctx, "pt_upsample_params", { p->sigma_normal, p->sigma_depth }));
    return pt_check_reserved(ctx, "pt_upsample_params", p->reserved);
}

}  // namespace

void ptu_free(pt_film *f)
{
    pt_film::Upsample &u = f->up;
    pt_scratch_free({ pt_buf_of(u.d_out), pt_buf_of(u.d_out_bgra) }, &u.bytes, u.bytes);
    u = pt_film::Upsample{};
}

pt_status ptu_upsample(pt_film *f, pt_film *lo, const pt_upsample_params *p, void *device_out, float *device_ms)
{
    pt_ctx *ctx = f->ctx;
    PT_TRY(up_validate(f, lo, p));
    pt_film::Upsample &u = f->up;
    const size_t n_pix = (size_t)f->w * f->h;
    // the film's own output, then lo's records; a refusal of the second takes back what the first made, so that both films stay as they were
    const bool new_out = !device_out && !u.d_out;
    if (new_out)
        PT_TRY(pt_scratch_alloc(ctx, "upsample output", { pt_buf_of(u.d_out, sizeof(float) * 3 * n_pix), pt_buf_of(u.d_out_bgra, 4 * n_pix) }, &u.bytes, 0,
                                f->work.bytes + f->aov.bytes + f->dn.bytes, ctx->mem_budget));
    const pt_status rs = ptd_scratch(lo);
    if (rs != PT_OK) {
        if (new_out) ptu_free(f);
        return rs;
    }
    UpConst uc{};
    uc.w = f->w; uc.h = f->h;
    const uint32_t n_blocks = fp_grid(f->w, f->h, &uc.n_bx);
    uc.lw = lo->w; uc.lh = lo->h;
    uc.sx = (float)lo->w / (float)f->w; uc.sy = (float)lo->h / (float)f->h;
    uc.inv_n = 1.0f / (p->sigma_normal * p->sigma_normal);
    uc.sz2 = p->sigma_depth * p->sigma_depth;
    const pt_film::Aov &a = f->aov;
    const UpGuides gd = { static_cast<const float *>(a.plane[PT_AOV_ALBEDO]), static_cast<const float *>(a.plane[PT_AOV_NORMAL]),
                          static_cast<const float *>(a.plane[PT_AOV_EMISSION]), static_cast<const float *>(a.plane[PT_AOV_DEPTH]),
                          static_cast<const float *>(a.plane[PT_AOV_ALPHA]) };
    const UpLo lr = { lo->dn.d_guide, lo->dn.d_illum[0] };
    const UpOut out = { device_out ? static_cast<float *>(device_out) : u.d_out, device_out ? nullptr : reinterpret_cast<uchar4 *>(u.d_out_bgra) };
    const float *src = p->source == PT_UPSAMPLE_SRC_DENOISED ? lo->dn.d_out : lo->d_rgb;
    const pt_status rt = pt_timed_pass(ctx, device_ms, [&](hipStream_t st) {
        ptd_prepare_records(lo, src, st);
        k_upsample<<<n_blocks, TB, 0, st>>>(uc, gd, lr, out);
    });
    if (rt == PT_OK && !device_out) u.have_out = true;
    return rt;
}
