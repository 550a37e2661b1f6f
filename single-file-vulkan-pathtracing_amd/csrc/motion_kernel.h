// motion_kernel.h -- the per-pixel body of k_motion (motion.hip), in a header of its own so that tests/motion_host.cpp can compile the very
// same statements for the host (plain IEEE divides and square roots stand in for pt_math.h's helpers, which are their bitwise equals) and
// hold them against the numpy restatement without a GPU, under the host's sanitizers.
// Wants declared before it: ptm::Camera, ptm::fdiv, ptm::fsqrt, ptm::primary_target, ptm::div3_dominant (pt_math.h), uint2, float4,
// make_float4, min, TB and MO_KEEP(v) (the device: an empty asm that takes v in a vector register; the host: nothing).
#pragma once
#include "film_pass.h"

struct MoConst {
    uint32_t w, h, n_bx;       // image, blocks per row of blocks
    uint32_t n_tris, n_inst;   // the scene's triangles; max(instances, 1): what the two id words have to stay below
    ptm::Camera cam;           // of the film's guides
    float slack;               // bary_slack
};
struct MoScene {
    const float4 *tri, *tri_prev;   // 3 records per triangle in primitive order {v.xyz, *}: now, and the snapshot's
    const float4 *xf, *xf_prev;     // INST: 3 rows per instance in gl_InstanceID order {m0, m1, m2, m3}: now, and the snapshot's
};
struct MoFilm {
    const float *depth, *alpha;
    const uint2 *id;
    float4 *q;                 // Q: written
};

struct MoVec { float x, y, z; };

// one row-by-row product of a 3x4 matrix with a point: ((m0*V.x + m1*V.y) + m2*V.z) + m3
__device__ __forceinline__ MoVec mo_xform(const float4 *m, const MoVec &v)
{
    return { ((m[0].x * v.x + m[0].y * v.y) + m[0].z * v.z) + m[0].w, ((m[1].x * v.x + m[1].y * v.y) + m[1].z * v.z) + m[1].w,
             ((m[2].x * v.x + m[2].y * v.y) + m[2].z * v.z) + m[2].w };
}
__device__ __forceinline__ float mo_dot(const MoVec &a, const MoVec &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ MoVec mo_sub(const MoVec &a, const MoVec &b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }

// one pixel (x, y) inside the image: everything k_motion does
template <bool INST>
__device__ __forceinline__ void mo_pixel(const MoConst &mc, const MoScene &sc, const MoFilm &fl, int x, int y)
{
    const size_t p = (size_t)y * mc.w + (uint32_t)x;
    const float ap = fl.alpha[p], zp = fl.depth[p];
    const uint2 idp = fl.id[p];
    // a miss, or an id plane that holds something else: the indices are clamped into their arrays and the result is dropped by the select below
    const bool known = (ap > 0.0f) & (idp.x < mc.n_tris) & (idp.y < mc.n_inst);
    const uint32_t prim = min(idp.x, mc.n_tris - 1u), inst = min(idp.y, mc.n_inst - 1u);
    // every gathered record first, so that all of them are in flight together ...
    float4 now[3], was[3], m_now[3], m_was[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        now[k] = sc.tri[3 * (size_t)prim + k];
        was[k] = sc.tri_prev[3 * (size_t)prim + k];
        if (INST) {
            m_now[k] = sc.xf[3 * (size_t)inst + k];
            m_was[k] = sc.xf_prev[3 * (size_t)inst + k];
        }
    }
    // ... and pinned here, after the last load was issued (reproject_kernel.h has the reason)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        MO_KEEP(now[k].x); MO_KEEP(now[k].y); MO_KEEP(now[k].z);
        MO_KEEP(was[k].x); MO_KEEP(was[k].y); MO_KEEP(was[k].z);
        if (INST) {
            MO_KEEP(m_now[k].x); MO_KEEP(m_now[k].y); MO_KEEP(m_now[k].z); MO_KEEP(m_now[k].w);
            MO_KEEP(m_was[k].x); MO_KEEP(m_was[k].y); MO_KEEP(m_was[k].z); MO_KEEP(m_was[k].w);
        }
    }
    // the first hit, back in the world: pt_film_reproject's P
    const float t = ptm::fdiv(zp, ap);
    float vx, vy, vz;
    ptm::primary_target(mc.cam, (uint32_t)x, (uint32_t)y, 0.5f, 0.5f, vx, vy, vz);
    const float len = ptm::fsqrt((vx * vx + vy * vy) + vz * vz);
    float dx, dy, dz;
    ptm::div3_dominant(vx, vy, vz, len, dx, dy, dz);
    const MoVec P = { mc.cam.ox + dx * t, mc.cam.oy + dy * t, mc.cam.oz + dz * t };
    MoVec A = { now[0].x, now[0].y, now[0].z }, B = { now[1].x, now[1].y, now[1].z }, C = { now[2].x, now[2].y, now[2].z };
    MoVec A1 = { was[0].x, was[0].y, was[0].z }, B1 = { was[1].x, was[1].y, was[1].z }, C1 = { was[2].x, was[2].y, was[2].z };
    if (INST) {  // six vertices forward: no inverse anywhere
        A = mo_xform(m_now, A); B = mo_xform(m_now, B); C = mo_xform(m_now, C);
        A1 = mo_xform(m_was, A1); B1 = mo_xform(m_was, B1); C1 = mo_xform(m_was, C1);
    }
    const MoVec e1 = mo_sub(B, A), e2 = mo_sub(C, A), g = mo_sub(P, A), f1 = mo_sub(B1, A1), f2 = mo_sub(C1, A1);
    const float d11 = mo_dot(e1, e1), d12 = mo_dot(e1, e2), d22 = mo_dot(e2, e2), p1 = mo_dot(g, e1), p2 = mo_dot(g, e2);
    const float det = d11 * d22 - d12 * d12;
    const float u = ptm::fdiv(d22 * p1 - d12 * p2, det), v = ptm::fdiv(d11 * p2 - d12 * p1, det);
    const bool ok = known & (det > 0.0f) & (u >= -mc.slack) & (v >= -mc.slack) & ((u + v) <= 1.0f + mc.slack);  // (a NaN fails)
    const float qx = (A1.x + u * f1.x) + v * f2.x, qy = (A1.y + u * f1.y) + v * f2.y, qz = (A1.z + u * f1.z) + v * f2.z;
    fl.q[p] = make_float4(ok ? qx : 0.0f, ok ? qy : 0.0f, ok ? qz : 0.0f, ok ? 1.0f : 0.0f);
}
