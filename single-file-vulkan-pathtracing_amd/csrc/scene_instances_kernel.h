// scene_instances_kernel.h -- the per-thread statements of scene_instances.hip's kernels (pt_scene_set_instances_device: what
// pt_scene_set_instances does on the host with the caller's matrices, as device code), in a header of their own so that
// tests/scene_instances_host.cpp can compile the very same statements for the host and hold them against restatements of ptb_set_instances'
// loop and ptb_ensure_inst_lights' loop (scene_build.hip) without a GPU, under the host's sanitizers.  si_invert_3x4 is also what the host call
// itself runs: one set of statements for both.  Wants declared before it: float4 / make_float4, ptm::fsqrt and ptm::fdiv (pt_internal.h +
// pt_math.h on the device, tests/kernel_host.h on the host).  Compile with -ffp-contract=off: the records' bits are the host loop's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SI_HD __host__ __device__
#else
#define SI_HD
#endif

// ---- world -> object matrix: adjugate / determinant in binary64, nine divides by det, every value rounded once to float
SI_HD inline void si_invert_3x4(const float m[12], float inv[12])
{
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double i00 = c00 / det, i01 = (a02 * a21 - a01 * a22) / det, i02 = (a01 * a12 - a02 * a11) / det;
    const double i10 = c01 / det, i11 = (a00 * a22 - a02 * a20) / det, i12 = (a02 * a10 - a00 * a12) / det;
    const double i20 = c02 / det, i21 = (a01 * a20 - a00 * a21) / det, i22 = (a00 * a11 - a01 * a10) / det;
    const double tx = m[3], ty = m[7], tz = m[11];
    inv[0] = (float)i00; inv[1] = (float)i01; inv[2] = (float)i02;  inv[3] = (float)(-((i00 * tx + i01 * ty) + i02 * tz));
    inv[4] = (float)i10; inv[5] = (float)i11; inv[6] = (float)i12;  inv[7] = (float)(-((i10 * tx + i11 * ty) + i12 * tz));
    inv[8] = (float)i20; inv[9] = (float)i21; inv[10] = (float)i22; inv[11] = (float)(-((i20 * tx + i21 * ty) + i22 * tz));
}

// ptb_set_instances' test of one value, both for the matrix given and for its inverse
SI_HD inline bool si_bad_value(float x) { return !(x == x) || __builtin_isinf(x); }

// ---- 1. one instance: the verdict word of ptb_set_instances' loop at instance i -- (i << 1) | kind, kind 0 "has a NaN/Inf" (the input check,
// which comes first), kind 1 "is singular" (the check of the inverse) -- or SI_OK; the minimum over the instances is the loop's first error.
// All twelve values are loaded before any is tested.  The 96-byte record {m, inv} goes to rec6 (six float4: ptb_set_instances' d_in) and the
// matrix as given to kept3 (three float4: the scene's kept copy, gl_InstanceID order) whatever the verdict: a refused set is dropped whole.
constexpr uint32_t SI_OK = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t si_check_invert(const float *__restrict__ xforms3x4, uint32_t i, float4 *__restrict__ rec6, float4 *__restrict__ kept3)
{
    float m[12], inv[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = xforms3x4[12 * (size_t)i + k];
    bool bad_in = false, bad_inv = false;
#pragma unroll
    for (int k = 0; k < 12; k++) bad_in |= si_bad_value(m[k]);
    si_invert_3x4(m, inv);
#pragma unroll
    for (int k = 0; k < 12; k++) bad_inv |= si_bad_value(inv[k]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float4 row = make_float4(m[4 * r + 0], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]);
        rec6[r] = row;
        kept3[r] = row;
        rec6[3 + r] = make_float4(inv[4 * r + 0], inv[4 * r + 1], inv[4 * r + 2], inv[4 * r + 3]);
    }
    return bad_in ? (i << 1) : bad_inv ? ((i << 1) | 1u) : SI_OK;
}

// ---- 3. one (instance, emitter) copy: ptb_ensure_inst_lights' loop body.  xf3: the instance's three rows as given; base5: the emitter's
// record in object space (push_emitter's five float4; its cdf word is not read).  The three vertices go through the matrix with the loop's
// operation order, then push_emitter's statements; the cdf word is the fold's (scene_device_kernel.h) and is written as +0; -> 0.5f * len,
// the term the fold adds.
__device__ __forceinline__ float si_light_record(const float4 *__restrict__ xf3, const float4 *__restrict__ base5, float4 *__restrict__ rec5)
{
    const float4 r0 = xf3[0], r1 = xf3[1], r2 = xf3[2];
    const float m[12] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w };
    float w[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float4 v = base5[c];
#pragma unroll
        for (int r = 0; r < 3; r++) w[c][r] = ((m[4 * r] * v.x + m[4 * r + 1] * v.y) + m[4 * r + 2] * v.z) + m[4 * r + 3];
    }
    const float4 ke = base5[4];
    const float *a = w[0], *b = w[1], *c = w[2];
    const float e1[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, e2[3] = { c[0] - a[0], c[1] - a[1], c[2] - a[2] };
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const float len = ptm::fsqrt((cx * cx + cy * cy) + cz * cz);
    rec5[0] = make_float4(a[0], a[1], a[2], 0.f);
    rec5[1] = make_float4(b[0], b[1], b[2], 0.f);
    rec5[2] = make_float4(c[0], c[1], c[2], 0.f);
    rec5[3] = make_float4(-ptm::fdiv(cx, len), -ptm::fdiv(cy, len), -ptm::fdiv(cz, len), 0.f);
    rec5[4] = ke;
    return 0.5f * len;
}
