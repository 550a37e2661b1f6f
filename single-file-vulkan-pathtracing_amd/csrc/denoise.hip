// denoise.hip -- pt_film_denoise: the guide-driven edge-avoiding a-trous filter of include/pt_api.h over the radiance film.
//
// The definition (demodulation, the 5 x 5 taps at step 2^k in the order j outer / i inner, the t^16 weight, remodulation, the bgra8
// form) is the header's; tests/test_denoise.py restates it in numpy and every comparison is byte equality.  So every operation here is
// one binary32 operation in the written order (-ffp-contract=off, __fdiv_rn), and nothing is reassociated.
//
//   k_dn_prepare   one pass over the film and the five float guide planes (56 B per pixel, eleven scalar loads from six arrays) -> two
//                  16-B records per pixel: illum {I.rgb, 0} and guide {N.xyz, Z}.  A tap of the iterations is then two 128-bit loads.
//   k_dn_atrous    one launch per iteration, ping-ponging the illum records.  A block is 64 x 4 pixels, a wave one row of 64: every tap
//                  of a wave is 64 consecutive 16-B records (1 KiB per load instruction) at any step, and the row test of a tap is
//                  wave-uniform.  The last launch divides, remodulates (D and E from the planes again), writes `out` and its bgra8 form.
//
// pt_film_denoise_variance is the same filter with the header's colour stop.  The variance V of a pixel rides in the spare word of its illum
// record, so a tap is the same two 128-bit loads and the scratch the same 48 B per pixel:
//   k_dn_prepare_var   k_dn_prepare, and V0 from the film's second-moment plane (+ 12 B per pixel read) into illum.w
//   k_dn_var_blur      the 3 x 3 pre-blur of .w, from one ping-pong plane into the other (rgb copied)
//   k_dn_atrous_var    k_dn_atrous with x_c in the weight, and V' = sum w^2 V_q / den^2 into .w
//
// pt_film_denoise_history is pt_film_denoise_variance with V0 made per pixel, for a film that pt_film_reproject left with a history length L
// of its own in every pixel.  Two kernels in front of the pre-blur, their bodies in denoise_history_kernel.h:
//   k_dn_prepare_hist  k_dn_prepare_var with n = min(L * step_frames, n_max) from the film's L plane (+ 4 B per pixel read); 0 into .w where
//                      L < min_history
//   k_dn_var_spatial   illum[0] -> illum[1].  A lane reads its own L; a wave (one row of 64) in which no lane is short copies its records
//                      and is done -- one wave-wide vote and a uniform branch.  Otherwise the 5 x 5 window at step 1: per row of taps the ten
//                      128-bit loads together from clamped addresses, long lanes and taps outside the image dropped by selects.
// Both take arguments of their own (DhConst, DhPlanes): DnConst and DnPlanes, whose layout the older kernels' scalar loads depend on, stay.
//
// What the kernels share and what they do not, as the device-code comparison (scripts/device_asm_diff.py) decided it: the block (film_pass.h
// fp_pixel), dn_demod and the guide part of a tap's weight (dn_guide_x, in denoise_history_kernel.h for dn_tap and dh_tap) are one each.
// dn_tap_var keeps its own copy of the guide weight, k_dn_atrous and k_dn_atrous_var stay two bodies, and the bodies of the five older kernels
// stay in this file: each of those mergers changed the generated code (registers, schedule) of the a-trous kernels, which are sensitive to
// their source text.  DESIGN.md section 4, "Film passes", has the list.
#include "pt_internal.h"
#include "pt_math.h"

#include <cmath>

namespace {

#define DH_KEEP(v) asm volatile("" : "+v"(v))  // the value exists in a vector register at this point: its load cannot move below
#include "denoise_history_kernel.h"  // DhConst, DhPlanes, dh_prepare_pixel, dh_spatial_pixel: the two kernels' bodies; dn_demod, dn_guide_x

struct DnConst {
    uint32_t w, h, n_bx;  // image, blocks per row of blocks
    int32_t step;         // 2^k
    float inv_n, sz2;     // 1 / (sigma_normal * sigma_normal), sigma_depth * sigma_depth
};
struct DnPlanes {
    const float *film, *albedo, *normal, *emission, *depth, *alpha;
};
struct DnOut {
    float *rgb;      // w*h*3
    uchar4 *bgra;    // w*h, or null (a caller-owned output has no bgra8 form)
};

__global__ __launch_bounds__(TB) void k_dn_prepare(uint32_t n_pix, DnPlanes pl, float4 *__restrict__ illum, float4 *__restrict__ guide)
{
    const uint32_t p = blockIdx.x * TB + threadIdx.x;
    if (p >= n_pix) return;
    const size_t p3 = 3 * (size_t)p;
    const float al = pl.alpha[p];
    const float ir = ptm::fdiv(pl.film[p3 + 0] - pl.emission[p3 + 0], dn_demod(pl.albedo[p3 + 0], al));
    const float ig = ptm::fdiv(pl.film[p3 + 1] - pl.emission[p3 + 1], dn_demod(pl.albedo[p3 + 1], al));
    const float ib = ptm::fdiv(pl.film[p3 + 2] - pl.emission[p3 + 2], dn_demod(pl.albedo[p3 + 2], al));
    illum[p] = make_float4(ir, ig, ib, 0.f);
    guide[p] = make_float4(pl.normal[p3 + 0], pl.normal[p3 + 1], pl.normal[p3 + 2], pl.depth[p]);
}

// the same, and V0 = sum_c max(M_c - C_c^2, 0) / (n - 1) / D_c^2 into the record's fourth word (nm1 = (float)(n - 1))
__global__ __launch_bounds__(TB) void k_dn_prepare_var(uint32_t n_pix, DnPlanes pl, const float *__restrict__ m2, float nm1, float4 *__restrict__ illum,
                                                       float4 *__restrict__ guide)
{
    const uint32_t p = blockIdx.x * TB + threadIdx.x;
    if (p >= n_pix) return;
    const size_t p3 = 3 * (size_t)p;
    const float al = pl.alpha[p];
    float i3[3], v3[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float col = pl.film[p3 + c], d = dn_demod(pl.albedo[p3 + c], al);
        i3[c] = ptm::fdiv(col - pl.emission[p3 + c], d);
        v3[c] = ptm::fdiv(ptm::fdiv(fmaxf(m2[p3 + c] - col * col, 0.0f), nm1), d * d);
    }
    illum[p] = make_float4(i3[0], i3[1], i3[2], (v3[0] + v3[1]) + v3[2]);
    guide[p] = make_float4(pl.normal[p3 + 0], pl.normal[p3 + 1], pl.normal[p3 + 2], pl.depth[p]);
}

// V = the 3 x 3 binomial mean of V0 over the taps inside the image (j outer, i inner); the record's rgb goes along
__global__ __launch_bounds__(TB) void k_dn_var_blur(DnConst dc, const float4 *__restrict__ illum_in, float4 *__restrict__ illum_out)
{
    int x, y; fp_pixel(dc.n_bx, x, y);
    const int w = (int)dc.w, h = (int)dc.h;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * dc.w + (uint32_t)x;
    float4 rec = illum_in[p];
    float sum = 0.f, wsum = 0.f;
#pragma unroll
    for (int j = -1; j <= 1; j++) {
        const int qy = y + j;
        if (qy < 0 || qy >= h) continue;
        const float4 *row = illum_in + (size_t)qy * dc.w;
#pragma unroll
        for (int i = -1; i <= 1; i++) {
            const int qx = x + i;
            if (qx < 0 || qx >= w) continue;
            const float g = (j == 0 ? 0.5f : 0.25f) * (i == 0 ? 0.5f : 0.25f);
            sum = sum + g * (i == 0 && j == 0 ? rec.w : row[qx].w);
            wsum = wsum + g;
        }
    }
    rec.w = ptm::fdiv(sum, wsum);
    illum_out[p] = rec;
}

// pt_film_denoise_history: V0 per pixel from its own history length (the bodies: denoise_history_kernel.h)
__global__ __launch_bounds__(TB) void k_dn_prepare_hist(uint32_t n_pix, DhConst hc, DhPlanes pl, float4 *__restrict__ illum, float4 *__restrict__ guide)
{
    const uint32_t p = blockIdx.x * TB + threadIdx.x;
    if (p >= n_pix) return;
    dh_prepare_pixel(hc, pl, p, illum, guide);
}

__global__ __launch_bounds__(TB) void k_dn_var_spatial(DhConst hc, const float *__restrict__ len, const float4 *__restrict__ guide, const float4 *__restrict__ illum_in,
                                                       float4 *__restrict__ illum_out)
{
    int x, y; fp_pixel(hc.n_bx, x, y);
    if (x >= (int)hc.w || y >= (int)hc.h) return;
    const size_t p = (size_t)y * hc.w + (uint32_t)x;
    const float l = len[p];
    const float4 rec = illum_in[p];
    // the vote: the lanes of a wave are one row's pixels inside the image; on a steady reprojected film most waves hold no short pixel
    if (__builtin_amdgcn_ballot_w64(dh_short(l, hc.mh)) == 0) {
        illum_out[p] = rec;
        return;
    }
    illum_out[p] = dh_spatial_pixel(hc, guide, illum_in, x, y, l, rec);
}

// k_resolve's clamp and quantise (shade_kernels.hip to_unorm8)
__device__ __forceinline__ uint8_t dn_unorm8(float c)
{
    if (!(c > 0.0f)) return 0;
    if (c > 1.0f) c = 1.0f;
    return (uint8_t)(c * 255.0f + 0.5f);
}

struct DnSum {
    float r = 0.f, g = 0.f, b = 0.f, den = 0.f;
};
// one tap: the weight of q seen from p, then the four adds
__device__ __forceinline__ void dn_tap(DnSum &s, const DnConst &dc, float hh, const float4 gp, const float4 gq, const float4 iq)
{
    float t = fmaxf(0.0f, 1.0f - dn_guide_x(dc.inv_n, dc.sz2, gp, gq) * 0.0625f);
    t = t * t; t = t * t; t = t * t; t = t * t;
    const float w = hh * t;
    s.r = s.r + w * iq.x;
    s.g = s.g + w * iq.y;
    s.b = s.b + w * iq.z;
    s.den = s.den + w;
}
// the tap with the colour stop: ip = {I_p, V_p}, iq = {I_q, V_q}
struct DnSumVar : DnSum {
    float vnum = 0.f;
};
__device__ __forceinline__ void dn_tap_var(DnSumVar &s, const DnConst &dc, float sc2, float hh, const float4 gp, const float4 gq, const float4 ip, const float4 iq)
{
    const float dx = gp.x - gq.x, dy = gp.y - gq.y, dz3 = gp.z - gq.z;
    const float xn = ((dx * dx + dy * dy) + dz3 * dz3) * dc.inv_n;
    const float dz = gp.w - gq.w;
    const float xz = ptm::fdiv(dz * dz, dc.sz2 * (gp.w * gp.w + gq.w * gq.w) + 1e-12f);
    const float dr = ip.x - iq.x, dg = ip.y - iq.y, db = ip.z - iq.z;
    const float xc = ptm::fdiv((dr * dr + dg * dg) + db * db, sc2 * (ip.w + iq.w) + 1e-12f);
    float t = fmaxf(0.0f, 1.0f - ((xn + xz) + xc) * 0.0625f);
    t = t * t; t = t * t; t = t * t; t = t * t;
    const float w = hh * t;
    s.r = s.r + w * iq.x;
    s.g = s.g + w * iq.y;
    s.b = s.b + w * iq.z;
    s.den = s.den + w;
    s.vnum = s.vnum + (w * w) * iq.w;
}
__device__ __forceinline__ constexpr float dn_h(int k) { return k == 0 ? 0.375f : (k == 1 || k == -1) ? 0.25f : 0.0625f; }

// I' = num / den; the last iteration goes on to out = I' * D + E and the bgra8 form
// (vnum: the variance kernels' sum of w^2 V_q, for V' = vnum / den^2 in the record's fourth word)
template <bool LAST, bool VAR = false>
__device__ __forceinline__ void dn_finish(const DnSum &s, size_t p, float4 *__restrict__ illum_out, const DnPlanes &pl, const DnOut &o, float vnum = 0.f)
{
    const float ir = ptm::fdiv(s.r, s.den), ig = ptm::fdiv(s.g, s.den), ib = ptm::fdiv(s.b, s.den);
    if (!LAST) {
        illum_out[p] = make_float4(ir, ig, ib, VAR ? ptm::fdiv(vnum, s.den * s.den) : 0.f);
        return;
    }
    const size_t p3 = 3 * p;
    const float al = pl.alpha[p];
    const float r = ir * dn_demod(pl.albedo[p3 + 0], al) + pl.emission[p3 + 0];
    const float g = ig * dn_demod(pl.albedo[p3 + 1], al) + pl.emission[p3 + 1];
    const float b = ib * dn_demod(pl.albedo[p3 + 2], al) + pl.emission[p3 + 2];
    o.rgb[p3 + 0] = r; o.rgb[p3 + 1] = g; o.rgb[p3 + 2] = b;
    if (o.bgra) o.bgra[p] = make_uchar4(dn_unorm8(b), dn_unorm8(g), dn_unorm8(r), 255);
}

template <bool LAST>
__global__ __launch_bounds__(TB) void k_dn_atrous(DnConst dc, const float4 *__restrict__ guide, const float4 *__restrict__ illum_in,
                                                  float4 *__restrict__ illum_out, DnPlanes pl, DnOut o)
{
    int x, y; fp_pixel(dc.n_bx, x, y);
    const int w = (int)dc.w, h = (int)dc.h, s = dc.step;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * dc.w + (uint32_t)x;
    const float4 gp = guide[p];
    DnSum sum;
#pragma unroll
    for (int j = -2; j <= 2; j++) {
        const int qy = y + s * j;
        if (qy < 0 || qy >= h) continue;  // (the same for the whole wave: a wave is one row)
        // the row's ten loads first, from addresses clamped into the row, so that they are in flight together; a tap outside the image
        // is then skipped as a whole (its clamped operands are never used)
        const float4 *grow = guide + (size_t)qy * dc.w, *irow = illum_in + (size_t)qy * dc.w;
        float4 gq[5], iq[5];
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            const int qc = min(max(x + s * i, 0), w - 1);
            gq[i + 2] = grow[qc];
            iq[i + 2] = irow[qc];
        }
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            const int qx = x + s * i;
            if (qx >= 0 && qx < w) dn_tap(sum, dc, dn_h(j) * dn_h(i), gp, gq[i + 2], iq[i + 2]);
        }
    }
    dn_finish<LAST>(sum, p, illum_out, pl, o);
}

template <bool LAST>
__global__ __launch_bounds__(TB) void k_dn_atrous_var(DnConst dc, float sc2, const float4 *__restrict__ guide, const float4 *__restrict__ illum_in,
                                                      float4 *__restrict__ illum_out, DnPlanes pl, DnOut o)  // sc2 = sigma_color * sigma_color
{
    int x, y; fp_pixel(dc.n_bx, x, y);
    const int w = (int)dc.w, h = (int)dc.h, s = dc.step;
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * dc.w + (uint32_t)x;
    const float4 gp = guide[p], ip = illum_in[p];
    DnSumVar sum;
#pragma unroll
    for (int j = -2; j <= 2; j++) {
        const int qy = y + s * j;
        if (qy < 0 || qy >= h) continue;
        const float4 *grow = guide + (size_t)qy * dc.w, *irow = illum_in + (size_t)qy * dc.w;
        float4 gq[5], iq[5];
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            const int qc = min(max(x + s * i, 0), w - 1);
            gq[i + 2] = grow[qc];
            iq[i + 2] = irow[qc];
        }
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            const int qx = x + s * i;
            if (qx >= 0 && qx < w) dn_tap_var(sum, dc, sc2, dn_h(j) * dn_h(i), gp, gq[i + 2], ip, iq[i + 2]);
        }
    }
    dn_finish<LAST, true>(sum, p, illum_out, pl, o, sum.vnum);
}

// One picker for the family.  (An LDS-tiled form for steps 1 and 2 -- a block staging the (64 + 4 s) x (16 + 4 s) records its taps touch --
// was built and measured against this one on the same tree: same bytes, 4 % slower at step 1 and 12 % slower at step 2 on a 1080p
// frame, so it is not kept.  DESIGN.md section 13 has both sets of numbers.)
// The variance family has its own picker: its kernels take sigma_color^2 beside DnConst, whose layout the first family's ISA depends on.
using DnAtrousFn = decltype(&k_dn_atrous<false>);
using DnAtrousVarFn = decltype(&k_dn_atrous_var<false>);
DnAtrousFn pick_dn_atrous(bool last) { return last ? k_dn_atrous<true> : k_dn_atrous<false>; }
DnAtrousVarFn pick_dn_atrous_var(bool last) { return last ? k_dn_atrous_var<true> : k_dn_atrous_var<false>; }

// The three filters: the scratch, then prepare (+ the spatial estimate, the pre-blur), the iterations, the wait.  var: null for
// pt_film_denoise.  hist (with var; var->frames unused): pt_film_denoise_history.
struct DnVariance {
    float sigma_color;
    uint32_t frames;
};
struct DnHistory {
    float min_history, n_max;
    uint32_t step_frames;
};
pt_status dn_run(pt_film *f, uint32_t iterations, float sigma_normal, float sigma_depth, const DnVariance *var, void *device_out, float *device_ms,
                 const DnHistory *hist = nullptr)
{
    pt_ctx *ctx = f->ctx;
    pt_film::Denoise &d = f->dn;
    const size_t n_pix = (size_t)f->w * f->h;
    // each set whole or not at all, so that a refused call leaves the film as it was; all of the film's workspaces count against the budget
    const size_t others = f->work.bytes + f->aov.bytes + f->up.bytes;
    pt_status rc = ptd_scratch(f);
    if (rc == PT_OK && !device_out && !d.d_out)
        rc = pt_scratch_alloc(ctx, "denoiser workspace", { pt_buf_of(d.d_out, sizeof(float) * 3 * n_pix), pt_buf_of(d.d_out_bgra, 4 * n_pix) }, &d.bytes, 0, others,
                              ctx->mem_budget);
    if (rc != PT_OK) return rc;
    const pt_film::Aov &a = f->aov;
    const DnPlanes pl = { f->d_rgb, static_cast<const float *>(a.plane[PT_AOV_ALBEDO]), static_cast<const float *>(a.plane[PT_AOV_NORMAL]),
                          static_cast<const float *>(a.plane[PT_AOV_EMISSION]), static_cast<const float *>(a.plane[PT_AOV_DEPTH]),
                          static_cast<const float *>(a.plane[PT_AOV_ALPHA]) };
    const DnOut out = { device_out ? static_cast<float *>(device_out) : d.d_out, device_out ? nullptr : reinterpret_cast<uchar4 *>(d.d_out_bgra) };
    DnConst dc{};
    dc.w = f->w; dc.h = f->h;
    const uint32_t n_blocks = fp_grid(f->w, f->h, &dc.n_bx);
    dc.inv_n = 1.0f / (sigma_normal * sigma_normal);
    dc.sz2 = sigma_depth * sigma_depth;
    const pt_status rt = pt_timed_pass(ctx, device_ms, [&](hipStream_t st) {
        uint32_t in = 0;  // the ping-pong plane the first iteration reads
        if (hist) {
            DhConst hc{};
            hc.w = dc.w; hc.h = dc.h; hc.n_bx = dc.n_bx;
            hc.inv_n = dc.inv_n; hc.sz2 = dc.sz2;
            hc.mh = hist->min_history; hc.sf = (float)hist->step_frames; hc.n_max = hist->n_max;
            const DhPlanes hp = { pl.film, pl.albedo, pl.normal, pl.emission, pl.depth, pl.alpha, f->m2.ptr(), f->hist.ptr() };
            k_dn_prepare_hist<<<(uint32_t)((n_pix + TB - 1) / TB), TB, 0, st>>>((uint32_t)n_pix, hc, hp, d.d_illum[0], d.d_guide);
            k_dn_var_spatial<<<n_blocks, TB, 0, st>>>(hc, f->hist.ptr(), d.d_guide, d.d_illum[0], d.d_illum[1]);
            k_dn_var_blur<<<n_blocks, TB, 0, st>>>(dc, d.d_illum[1], d.d_illum[0]);
        } else if (var) {
            k_dn_prepare_var<<<(uint32_t)((n_pix + TB - 1) / TB), TB, 0, st>>>((uint32_t)n_pix, pl, f->m2.ptr(), (float)(var->frames - 1), d.d_illum[0], d.d_guide);
            k_dn_var_blur<<<n_blocks, TB, 0, st>>>(dc, d.d_illum[0], d.d_illum[1]);
            in = 1;
        } else {
            k_dn_prepare<<<(uint32_t)((n_pix + TB - 1) / TB), TB, 0, st>>>((uint32_t)n_pix, pl, d.d_illum[0], d.d_guide);
        }
        for (uint32_t k = 0; k < iterations; k++, in ^= 1u) {
            dc.step = 1 << k;
            const bool last = k + 1 == iterations;
            if (var) hipLaunchKernelGGL(pick_dn_atrous_var(last), dim3(n_blocks), dim3(TB), 0, st, dc, var->sigma_color * var->sigma_color, d.d_guide, d.d_illum[in], d.d_illum[in ^ 1u], pl, out);
            else hipLaunchKernelGGL(pick_dn_atrous(last), dim3(n_blocks), dim3(TB), 0, st, dc, d.d_guide, d.d_illum[in], d.d_illum[in ^ 1u], pl, out);
        }
    });
    if (rt == PT_OK && !device_out) d.have_out = true;
    return rt;
}

// What the three filters refuse alike, in the header's order: a film without the planes they read, iterations, the sigmas.  name: the struct's.
pt_status dn_checks(pt_film *f, const char *name, bool need_m, bool need_l, uint32_t iterations, std::initializer_list<float> sigmas)
{
    pt_ctx *ctx = f->ctx;
    if (!f->aov.enabled) return pt_bad(ctx, PT_NO_GUIDES_MSG);
    if (need_m && !f->m2.d) return pt_bad(ctx, PT_NO_M_MSG " before the frames are rendered");
    if (need_l && !f->hist.d) return pt_bad(ctx, PT_NO_L_MSG " (and pt_film_reproject) first");
    PT_TRY(pt_check_iterations(ctx, name, iterations));
    return pt_check_sigmas(ctx, name, sigmas);
}

}  // namespace

// the records' planes (48 B per pixel), made by the first call that needs them and kept
pt_status ptd_scratch(pt_film *f)
{
    pt_film::Denoise &d = f->dn;
    if (d.d_guide) return PT_OK;
    const size_t px4 = sizeof(float4) * (size_t)f->w * f->h;
    return pt_scratch_alloc(f->ctx, "denoiser workspace", { pt_buf_of(d.d_guide, px4), pt_buf_of(d.d_illum[0], px4), pt_buf_of(d.d_illum[1], px4) }, &d.bytes, 0,
                            f->work.bytes + f->aov.bytes + f->up.bytes, f->ctx->mem_budget);
}

// pt_film_upsample's records of a low-resolution film: k_dn_prepare over f with `src` (f's film or its denoised plane) as the film plane
void ptd_prepare_records(pt_film *f, const float *src, hipStream_t st)
{
    const pt_film::Aov &a = f->aov;
    const DnPlanes pl = { src, static_cast<const float *>(a.plane[PT_AOV_ALBEDO]), static_cast<const float *>(a.plane[PT_AOV_NORMAL]),
                          static_cast<const float *>(a.plane[PT_AOV_EMISSION]), static_cast<const float *>(a.plane[PT_AOV_DEPTH]),
                          static_cast<const float *>(a.plane[PT_AOV_ALPHA]) };
    const size_t n_pix = (size_t)f->w * f->h;
    k_dn_prepare<<<(uint32_t)((n_pix + TB - 1) / TB), TB, 0, st>>>((uint32_t)n_pix, pl, f->dn.d_illum[0], f->dn.d_guide);
}

void ptd_free(pt_film *f)
{
    pt_film::Denoise &d = f->dn;
    pt_scratch_free({ pt_buf_of(d.d_guide), pt_buf_of(d.d_illum[0]), pt_buf_of(d.d_illum[1]), pt_buf_of(d.d_out), pt_buf_of(d.d_out_bgra) }, &d.bytes, d.bytes);
    d = pt_film::Denoise{};
}

pt_status ptd_denoise(pt_film *f, const pt_denoise_params *p, void *device_out, float *device_ms)
{
    PT_TRY(dn_checks(f, "pt_denoise_params", false, false, p->iterations, { p->sigma_normal, p->sigma_depth }));
    PT_TRY(pt_check_reserved(f->ctx, "pt_denoise_params", p->reserved));
    return dn_run(f, p->iterations, p->sigma_normal, p->sigma_depth, nullptr, device_out, device_ms);
}

pt_status ptd_denoise_variance(pt_film *f, const pt_denoise_variance_params *p, void *device_out, float *device_ms)
{
    PT_TRY(dn_checks(f, "pt_denoise_variance_params", true, false, p->iterations, { p->sigma_normal, p->sigma_depth, p->sigma_color }));
    PT_TRY(pt_check_reserved(f->ctx, "pt_denoise_variance_params", p->reserved));
    const DnVariance v = { p->sigma_color, p->frames ? p->frames : f->m2.frames };
    if (v.frames < 2) return pt_bad(f->ctx, "pt_film_denoise_variance: a variance estimate needs a film of at least 2 frames (params.frames, or what pt_render recorded)");
    return dn_run(f, p->iterations, p->sigma_normal, p->sigma_depth, &v, device_out, device_ms);
}

pt_status ptd_denoise_history(pt_film *f, const pt_denoise_history_params *p, void *device_out, float *device_ms)
{
    pt_ctx *ctx = f->ctx;
    PT_TRY(dn_checks(f, "pt_denoise_history_params", true, true, p->iterations, { p->sigma_normal, p->sigma_depth, p->sigma_color }));
    if (!(p->min_history >= 1.f && p->min_history <= 65536.f)) return pt_bad(ctx, "pt_denoise_history_params.min_history must be finite and in 1..65536");
    if (!(std::isfinite(p->n_max) && p->n_max >= 2.f)) return pt_bad(ctx, "pt_denoise_history_params.n_max must be finite and >= 2");
    if (p->step_frames == 0) return pt_bad(ctx, "pt_denoise_history_params.step_frames must be >= 1");
    if (p->min_history * (float)p->step_frames < 2.f) return pt_bad(ctx, "pt_denoise_history_params: min_history * step_frames must be >= 2 (a variance estimate needs two frames)");
    PT_TRY(pt_check_reserved(ctx, "pt_denoise_history_params", p->reserved));
    const DnVariance v = { p->sigma_color, 0 };
    const DnHistory hs = { p->min_history, p->n_max, p->step_frames };
    return dn_run(f, p->iterations, p->sigma_normal, p->sigma_depth, &v, device_out, device_ms, &hs);
}
