// denoise_history_kernel.h -- the per-pixel bodies of k_dn_prepare_hist and k_dn_var_spatial (denoise.hip), the two kernels that
// pt_film_denoise_history puts in front of pt_film_denoise_variance's pre-blur and iterations.  In a header of its own, like
// reproject_kernel.h, so that tests/denoise_history_host.cpp can compile the very same statements for the host (plain IEEE divides stand in
// for pt_math.h's fdiv, their bitwise equal) and hold them against the numpy restatement without a GPU, under the host's sanitizers.
// It also holds what the three denoisers share on the device: dn_demod and the guide part of a tap's weight, dn_guide_x.
// Wants declared before it: ptm::fdiv (pt_math.h), float4, make_float4, min, max, fmaxf, fminf, TB and DH_KEEP(v) (the device: an empty asm
// that takes v in a vector register; the host: nothing).
#pragma once
#include "film_pass.h"

struct DhConst {
    uint32_t w, h, n_bx;    // image, blocks per row of blocks
    float inv_n, sz2;       // 1 / (sigma_normal * sigma_normal), sigma_depth * sigma_depth
    float mh, sf, n_max;    // min_history, (float)step_frames, n_max
};
struct DhPlanes {
    const float *film, *albedo, *normal, *emission, *depth, *alpha;
    const float *m2, *len;  // M and L
};

// pt_film_denoise's D
__device__ __forceinline__ float dn_demod(float a, float alpha) { return fmaxf(a + (1.0f - alpha), 0.001f); }
// the guide part of a tap's weight, x_n + x_z of q seen from p (records {N.xyz, Z}).  dn_tap and dh_tap share it; dn_tap_var (denoise.hip) keeps
// its own copy of the statements: calling this there re-allocates registers in both k_dn_atrous_var instantiations
__device__ __forceinline__ float dn_guide_x(float inv_n, float sz2, const float4 gp, const float4 gq)
{
    const float dx = gp.x - gq.x, dy = gp.y - gq.y, dz3 = gp.z - gq.z;
    const float xn = ((dx * dx + dy * dy) + dz3 * dz3) * inv_n;
    const float dz = gp.w - gq.w;
    const float xz = ptm::fdiv(dz * dz, sz2 * (gp.w * gp.w + gq.w * gq.w) + 1e-12f);
    return xn + xz;
}
// a pixel takes the spatial estimate unless L >= min_history (a NaN fails: short)
__device__ __forceinline__ bool dh_short(float len, float mh) { return !(len >= mh); }

// one pixel p of k_dn_prepare_hist: k_dn_prepare_var with n = min(L * step_frames, n_max) of the pixel's own L; a short pixel gets .w = 0
// (what it computed with its n is dropped by the select: n - 1 may be 0 or negative there)
__device__ __forceinline__ void dh_prepare_pixel(const DhConst &dc, const DhPlanes &pl, size_t p, float4 *__restrict__ illum, float4 *__restrict__ guide)
{
    const size_t p3 = 3 * p;
    const float al = pl.alpha[p], len = pl.len[p];
    const float nm1 = fminf(len * dc.sf, dc.n_max) - 1.0f;
    float i3[3], v3[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float col = pl.film[p3 + c], d = dn_demod(pl.albedo[p3 + c], al);
        i3[c] = ptm::fdiv(col - pl.emission[p3 + c], d);
        v3[c] = ptm::fdiv(ptm::fdiv(fmaxf(pl.m2[p3 + c] - col * col, 0.0f), nm1), d * d);
    }
    const float v0 = (v3[0] + v3[1]) + v3[2];
    illum[p] = make_float4(i3[0], i3[1], i3[2], dh_short(len, dc.mh) ? 0.0f : v0);
    guide[p] = make_float4(pl.normal[p3 + 0], pl.normal[p3 + 1], pl.normal[p3 + 2], pl.depth[p]);
}

struct DhSum {
    float S = 0.f, s1[3] = { 0.f, 0.f, 0.f }, s2[3] = { 0.f, 0.f, 0.f };
};
// one tap of the 5 x 5 window: pt_film_denoise's t^16 of the guides alone (no h), then the seven adds; a tap that does not count leaves the sums
__device__ __forceinline__ void dh_tap(DhSum &s, const DhConst &dc, bool ok, const float4 gp, const float4 gq, const float4 iq)
{
    float t = fmaxf(0.0f, 1.0f - dn_guide_x(dc.inv_n, dc.sz2, gp, gq) * 0.0625f);
    t = t * t; t = t * t; t = t * t; t = t * t;
    const float q[3] = { iq.x, iq.y, iq.z };
    const float S1 = s.S + t;
    s.S = ok ? S1 : s.S;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float a1 = s.s1[c] + t * q[c], a2 = s.s2[c] + t * (q[c] * q[c]);
        s.s1[c] = ok ? a1 : s.s1[c];
        s.s2[c] = ok ? a2 : s.s2[c];
    }
}

// one pixel (x, y) inside the image of k_dn_var_spatial: its record `rec` (= illum_in[p]) with .w replaced by the spatial estimate when the
// pixel is short, unchanged when it is long (a long lane walks the taps with its wave and drops every one of them).  A row of taps is ten
// 128-bit loads from addresses clamped into the row, issued together ahead of any test, as k_dn_atrous does it.
__device__ __forceinline__ float4 dh_spatial_pixel(const DhConst &dc, const float4 *__restrict__ guide, const float4 *__restrict__ illum_in, int x, int y, float len, float4 rec)
{
    const int w = (int)dc.w, h = (int)dc.h;
    const size_t p = (size_t)y * dc.w + (uint32_t)x;
    const bool sh = dh_short(len, dc.mh);
    const float4 gp = guide[p];
    DhSum sum;
#pragma unroll
    for (int j = -2; j <= 2; j++) {
        const int qy = y + j;
        if (qy < 0 || qy >= h) continue;  // (the same for the whole wave: a wave is one row)
        const float4 *grow = guide + (size_t)qy * dc.w, *irow = illum_in + (size_t)qy * dc.w;
        float4 gq[5], iq[5];
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            const int qc = min(max(x + i, 0), w - 1);
            gq[i + 2] = grow[qc];
            iq[i + 2] = irow[qc];
        }
        // every loaded word pinned after the row's last load: a tap's loads do not move behind another tap's arithmetic
#pragma unroll
        for (int i = 0; i < 5; i++) {
            DH_KEEP(gq[i].x); DH_KEEP(gq[i].y); DH_KEEP(gq[i].z); DH_KEEP(gq[i].w);
            DH_KEEP(iq[i].x); DH_KEEP(iq[i].y); DH_KEEP(iq[i].z);
        }
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            const int qx = x + i;
            dh_tap(sum, dc, sh & (qx >= 0) & (qx < w), gp, gq[i + 2], iq[i + 2]);
        }
    }
    const float ip[3] = { rec.x, rec.y, rec.z };
    float sv[3], ev[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float mu = ptm::fdiv(sum.s1[c], sum.S), m = ptm::fdiv(sum.s2[c], sum.S);
        sv[c] = fmaxf(m - mu * mu, 0.0f);
        const float e = ip[c] - mu;
        ev[c] = e * e;
    }
    const float vs = ((sv[0] + sv[1]) + sv[2]) + ((ev[0] + ev[1]) + ev[2]);
    const float v0 = vs * ptm::fdiv(dc.mh, fmaxf(len, 1.0f));
    rec.w = sh ? v0 : rec.w;
    return rec;
}
