// nee_sample.h -- the light sample of next-event estimation (PT_PIPELINE_WAVEFRONT_NEE, PT_FLAG_NEE): ONE source for the wavefront
// pipeline's k_shade (shade_kernels.hip) and the fused kernel's NEE instantiation (fused_kernel.h), so the two draw the same numbers and
// compute the same contribution bit for bit.
#pragma once
#include "pt_math.h"

namespace ptn {

// One light sample for the hit at `pos` (normal n, brdf, path weight w); the operations and their order are part of the
// pipeline's definition (the CPU checker of the tests restates them, and the two agree bit for bit).  Returns false when no shadow ray is needed.
// lights: 5 float4 per emitter (v0 | cdf, v1, v2, normal, Ke) -- pt_scene::d_lights.  Three random numbers are drawn whatever it returns.
__device__ __forceinline__ bool nee_sample(const float4 *__restrict__ lights, uint32_t n_lights, float light_area, uint32_t &seed,
                                           const ptm::f3 pos, const ptm::f3 n, float br, float bg, float bb, float wr, float wg,
                                           float wb, ptm::f3 &wi, float4 &contrib)
{
    const float rl = ptm::rnd(seed), ru = ptm::rnd(seed), rv = ptm::rnd(seed);
    const float pick = rl * light_area;
    // first emitter whose running area exceeds pick (the last one if none does): binary search of the cdf
    uint32_t li = 0, hi_ = n_lights - 1u;
    while (li < hi_) {
        const uint32_t mid = (li + hi_) >> 1;
        if (lights[5 * (size_t)mid].w > pick) hi_ = mid; else li = mid + 1u;
    }
    const float4 A = lights[5 * (size_t)li + 0], B = lights[5 * (size_t)li + 1], C = lights[5 * (size_t)li + 2],
                 N = lights[5 * (size_t)li + 3], Ke = lights[5 * (size_t)li + 4];
    const float su = ptm::fsqrt(ru);
    const float b0 = 1.0f - su, b1 = su * (1.0f - rv), b2 = su * rv;
    const float dx = ((A.x * b0 + B.x * b1) + C.x * b2) - pos.x, dy = ((A.y * b0 + B.y * b1) + C.y * b2) - pos.y,
                dz = ((A.z * b0 + B.z * b1) + C.z * b2) - pos.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(d2 > 0.0f)) return false;
    const float dist = ptm::fsqrt(d2);
    ptm::div3_dominant(dx, dy, dz, dist, wi.x, wi.y, wi.z);
    const float cs = (wi.x * n.x + wi.y * n.y) + wi.z * n.z;
    const float cl = fabsf((wi.x * N.x + wi.y * N.y) + wi.z * N.z);
    if (!(cs > 0.0f && cl > 0.0f)) return false;
    const float fgeo = ptm::fdiv(cs * cl, d2) * light_area;
    contrib = make_float4(((wr * br) * Ke.x) * fgeo, ((wg * bg) * Ke.y) * fgeo, ((wb * bb) * Ke.z) * fgeo, dist * 0.999f);
    return true;
}

}  // namespace ptn
