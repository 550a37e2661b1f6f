// adaptive_kernel.h -- the per-lane bodies of k_adapt_select and k_resolve_adapt (adaptive.hip), in a header of their own, like upsample_kernel.h,
// so that tests/adaptive_host.cpp can compile the very same statements for the host (the IEEE divide and root stand in for pt_math.h's fdiv
// and fsqrt, their bitwise equals) and hold them against the numpy restatement without a GPU, under the host's sanitizers.
// The definition is include/pt_api.h's (pt_render_adaptive); every operation here is one binary32 operation in the written order.
// Wants declared before it: ptm::fdiv, ptm::fsqrt (pt_math.h), uchar4, fmaxf.
#pragma once
#include <stdint.h>

struct AdConst {
    uint32_t w, h;                  // the image
    float threshold, rel_floor;
    float min_frames, max_frames;   // (float) of the parameters: what K is compared with
    uint32_t has_max;               // max_frames > 0
};

// e_l of a lane: the relative standard error of the pixel's mean, 0 for a lane outside the image or a pixel with fewer than two frames.
// Computed for every lane and dropped by a select, so that no lane branches ahead of the butterfly.
__device__ __forceinline__ float ad_lane_error(bool valid, const float c[3], const float m[3], float k, float rel_floor)
{
    const float km1 = k - 1.0f;
    const float vr = ptm::fdiv(fmaxf(m[0] - c[0] * c[0], 0.0f), km1);
    const float vg = ptm::fdiv(fmaxf(m[1] - c[1] * c[1], 0.0f), km1);
    const float vb = ptm::fdiv(fmaxf(m[2] - c[2] * c[2], 0.0f), km1);
    const float e = ptm::fdiv(ptm::fsqrt((vr + vg) + vb), ((c[0] + c[1]) + c[2]) + rel_floor);
    return (valid && k >= 2.0f) ? e : 0.0f;
}
// what the wave votes on: a valid pixel below min_frames (any: the tile is short), a valid pixel below max_frames (none: the tile is capped)
__device__ __forceinline__ bool ad_lane_short(bool valid, float k, float min_frames) { return valid && !(k >= min_frames); }
__device__ __forceinline__ bool ad_lane_below_max(bool valid, float k, float max_frames) { return valid && !(k >= max_frames); }
// (a NaN e_T is not "greater")
__device__ __forceinline__ bool ad_selected(bool short_, bool capped, float e_t, float threshold) { return !capped && (short_ || e_t > threshold); }

// k_resolve's clamp and quantise (shade_kernels.hip to_unorm8)
__device__ __forceinline__ uint8_t ad_unorm8(float c)
{
    if (!(c > 0.0f)) return 0;
    if (c > 1.0f) c = 1.0f;
    return (uint8_t)(c * 255.0f + 0.5f);
}

// A pixel's planes in registers between its load and its store.
struct AdPixel {
    float c[3], m[3];
    uchar4 img;   // bytes B, G, R, A
    float n;      // K_p: the frames the pixel holds
};
// One frame colour (sum / spp, per channel) blended into the pixel: k_resolve's blend with the pixel's own count n in place of the frame.
__device__ __forceinline__ void ad_blend(AdPixel &p, float cr, float cg, float cb)
{
    const float ff = p.n, f1 = p.n + 1.0f;
    const bool first = p.n == 0.0f;  // old * 0: the old values are not read
    const float col[3] = { cr, cg, cb };
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p.c[k] = ptm::fdiv(col[k] + (first ? 0.f : p.c[k]) * ff, f1);
        p.m[k] = ptm::fdiv(col[k] * col[k] + (first ? 0.f : p.m[k]) * ff, f1);
    }
    const float orr = first ? 0.f : ptm::fdiv((float)p.img.z, 255.0f);
    const float og = first ? 0.f : ptm::fdiv((float)p.img.y, 255.0f);
    const float ob = first ? 0.f : ptm::fdiv((float)p.img.x, 255.0f);
    const float oa = first ? 0.f : ptm::fdiv((float)p.img.w, 255.0f);
    p.img.z = ad_unorm8(ptm::fdiv(cr + orr * ff, f1));
    p.img.y = ad_unorm8(ptm::fdiv(cg + og * ff, f1));
    p.img.x = ad_unorm8(ptm::fdiv(cb + ob * ff, f1));
    p.img.w = ad_unorm8(ptm::fdiv(1.0f + oa * ff, f1));
    p.n = f1;
}
