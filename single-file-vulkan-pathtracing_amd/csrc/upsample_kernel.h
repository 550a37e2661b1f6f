// upsample_kernel.h -- the per-pixel body of k_upsample (upsample.hip), in a header of its own, like reproject_kernel.h, so that
// tests/upsample_host.cpp can compile the very same statements for the host (the IEEE divide stands in for pt_math.h's fdiv, its bitwise
// equal) and hold them against the numpy restatement without a GPU, under the host's sanitizers.
// Wants declared before it: ptm::fdiv (pt_math.h), float4, uchar4, make_uchar4, min, max, fmaxf, floorf, TB, DH_KEEP (for
// denoise_history_kernel.h, whose dn_demod and dn_guide_x are used here), UP_KEEP(v) (the device: an empty asm that takes v in a vector
// register; the host: nothing) and UP_ANY(b) (the device: does any lane of the wave have b; the host: true, so that every pixel walks
// the second ring and keeps its first-ring result by the select).
#pragma once
#include "film_pass.h"
#include "denoise_history_kernel.h"

struct UpConst {
    uint32_t w, h, n_bx;    // the full-size image, blocks per row of blocks
    uint32_t lw, lh;        // lo's image
    float sx, sy;           // (float)lw / (float)w, (float)lh / (float)h: one correctly rounded division each, on the host
    float inv_n, sz2;       // 1 / (sigma_normal * sigma_normal), sigma_depth * sigma_depth
};
struct UpGuides {           // the full-size film's guide planes as stored
    const float *albedo, *normal, *emission, *depth, *alpha;
};
struct UpLo {               // lo's records, as k_dn_prepare leaves them
    const float4 *guide;    // {N'.xyz, Z'}
    const float4 *illum;    // {I'.rgb, 0}
};
struct UpOut {
    float *rgb;             // w*h*3
    uchar4 *bgra;           // w*h, or null (a caller-owned output has no bgra8 form)
};

// k_resolve's clamp and quantise (shade_kernels.hip to_unorm8)
__device__ __forceinline__ uint8_t up_unorm8(float c)
{
    if (!(c > 0.0f)) return 0;
    if (c > 1.0f) c = 1.0f;
    return (uint8_t)(c * 255.0f + 0.5f);
}

// pt_film_denoise's t^16 of the guides alone: q seen from p
__device__ __forceinline__ float up_t(const UpConst &uc, const float4 gp, const float4 gq)
{
    float t = fmaxf(0.0f, 1.0f - dn_guide_x(uc.inv_n, uc.sz2, gp, gq) * 0.0625f);
    t = t * t; t = t * t; t = t * t; t = t * t;
    return t;
}

struct UpSum {
    float r = 0.f, g = 0.f, b = 0.f, den = 0.f;
};
// the four adds of a tap of weight wt; a tap that does not count leaves the sums
__device__ __forceinline__ void up_add(UpSum &s, bool ok, float wt, const float4 iq)
{
    const float r1 = s.r + wt * iq.x, g1 = s.g + wt * iq.y, b1 = s.b + wt * iq.z, d1 = s.den + wt;
    s.r = ok ? r1 : s.r;
    s.g = ok ? g1 : s.g;
    s.b = ok ? b1 : s.b;
    s.den = ok ? d1 : s.den;
}

// one pixel (x, y) inside the full-size image: everything k_upsample does.  Every tap address is clamped into lo's image and every load is
// issued ahead of the tests on what it returns; taps outside the image and lanes that do not fall back are dropped by selects.
__device__ __forceinline__ void up_pixel(const UpConst &uc, const UpGuides &gd, const UpLo &lo, const UpOut &o, int x, int y)
{
    const int lw = (int)uc.lw, lh = (int)uc.lh;
    const size_t p = (size_t)y * uc.w + (uint32_t)x, p3 = 3 * p;
    // the lane's own 44 B of guides
    const float al = gd.alpha[p];
    const float a3[3] = { gd.albedo[p3 + 0], gd.albedo[p3 + 1], gd.albedo[p3 + 2] };
    const float e3[3] = { gd.emission[p3 + 0], gd.emission[p3 + 1], gd.emission[p3 + 2] };
    const float4 gp = make_float4(gd.normal[p3 + 0], gd.normal[p3 + 1], gd.normal[p3 + 2], gd.depth[p]);
    const float fx = ((float)x + 0.5f) * uc.sx - 0.5f, fy = ((float)y + 0.5f) * uc.sy - 0.5f;   // in [-0.5, lw - 0.5) x [-0.5, lh - 0.5)
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float bx = fx - x0f, by = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;                                                   // in [-1, lw - 1] x [-1, lh - 1]
    // FIRST RING: the eight 128-bit loads of the four taps together ...
    float4 gq[4], iq[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {  // k = 2 j + i: j outer, i inner
        const int qx = min(max(x0 + (k & 1), 0), lw - 1), qy = min(max(y0 + (k >> 1), 0), lh - 1);
        const size_t q = (size_t)qy * uc.lw + (uint32_t)qx;
        gq[k] = lo.guide[q];
        iq[k] = lo.illum[q];
    }
    // ... and every loaded word pinned after the last load: a tap's loads do not move behind another tap's test or arithmetic
#pragma unroll
    for (int k = 0; k < 4; k++) {
        UP_KEEP(gq[k].x); UP_KEEP(gq[k].y); UP_KEEP(gq[k].z); UP_KEEP(gq[k].w);
        UP_KEEP(iq[k].x); UP_KEEP(iq[k].y); UP_KEEP(iq[k].z);
    }
    UpSum s1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        const float wq = ((k & 1) ? bx : 1.0f - bx) * ((k >> 1) ? by : 1.0f - by);
        const bool ok = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh);
        up_add(s1, ok, wq * up_t(uc, gp, gq[k]), iq[k]);
    }
    const bool fb = !(s1.den >= 0.01f);   // (a NaN den falls back)
    float i3[3] = { ptm::fdiv(s1.r, s1.den), ptm::fdiv(s1.g, s1.den), ptm::fdiv(s1.b, s1.den) };
    // SECOND RING and NEAREST, for the whole wave when one of its lanes asks: one vote, a uniform branch
    if (UP_ANY(fb)) {
        const int nx = min(max((int)floorf(fx + 0.5f), 0), lw - 1), ny = min(max((int)floorf(fy + 0.5f), 0), lh - 1);
        float4 in = lo.illum[(size_t)ny * uc.lw + (uint32_t)nx];
        UP_KEEP(in.x); UP_KEEP(in.y); UP_KEEP(in.z);
        UpSum s2;
#pragma unroll
        for (int j = -1; j <= 2; j++) {
            // a row of taps: its eight loads together, from clamped addresses
            const int qy = y0 + j, qyc = min(max(qy, 0), lh - 1);
            const float4 *grow = lo.guide + (size_t)qyc * uc.lw, *irow = lo.illum + (size_t)qyc * uc.lw;
            float4 g4[4], i4[4];
#pragma unroll
            for (int i = -1; i <= 2; i++) {
                const int qc = min(max(x0 + i, 0), lw - 1);
                g4[i + 1] = grow[qc];
                i4[i + 1] = irow[qc];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                UP_KEEP(g4[i].x); UP_KEEP(g4[i].y); UP_KEEP(g4[i].z); UP_KEEP(g4[i].w);
                UP_KEEP(i4[i].x); UP_KEEP(i4[i].y); UP_KEEP(i4[i].z);
            }
            const bool row_ok = (qy >= 0) & (qy < lh);
#pragma unroll
            for (int i = -1; i <= 2; i++) {
                const int qx = x0 + i;
                up_add(s2, row_ok & (qx >= 0) & (qx < lw), up_t(uc, gp, g4[i + 1]), i4[i + 1]);
            }
        }
        const bool ring2 = s2.den >= 0.01f;
        const float r3[3] = { ptm::fdiv(s2.r, s2.den), ptm::fdiv(s2.g, s2.den), ptm::fdiv(s2.b, s2.den) };
        const float n3[3] = { in.x, in.y, in.z };
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float f = ring2 ? r3[c] : n3[c];
            i3[c] = fb ? f : i3[c];   // a lane that did not fall back keeps its first-ring result
        }
    }
    float out[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        out[c] = i3[c] * dn_demod(a3[c], al) + e3[c];
        o.rgb[p3 + c] = out[c];
    }
    if (o.bgra) o.bgra[p] = make_uchar4(up_unorm8(out[2]), up_unorm8(out[1]), up_unorm8(out[0]), 255);
}
