// reproject_kernel.h -- the per-pixel body of k_reproject (reproject.hip), in a header of its own so that tests/reproject_host.cpp can compile
// the very same statements for the host (plain IEEE divides and square roots stand in for pt_math.h's helpers, which are their bitwise
// equals) and hold them against the numpy restatement without a GPU, under the host's sanitizers.
// Wants declared before it: ptm::Camera, ptm::fdiv, ptm::fsqrt, ptm::primary_target, ptm::div3_dominant (pt_math.h), uint2, uchar4,
// make_uchar4, min, max, TB and RP_KEEP(v) (the device: an empty asm that takes v in a vector register; the host: nothing).
#pragma once
#include "film_pass.h"

struct RpConst {
    uint32_t w, h, n_bx;       // image, blocks per row of blocks
    uint32_t match_id;         // PT_REPROJECT_MATCH_ID set
    ptm::Camera cam;           // of `film`
    float pox, poy, poz;       // the previous camera's origin ...
    float ptx, pty, ptz;       // ... and target
    float gain, alpha, depth_tol, normal_min, max_history;
};
struct RpFilm {
    float *rgb, *m2, *len;     // C, M (null without the plane), L: rewritten
    uchar4 *bgra;
    const float *normal, *depth, *alpha;
    const uint2 *id;
};
struct RpPrev {
    const float *rgb, *m2, *len, *normal, *depth, *alpha;   // rgb null: no previous film, every pixel takes the no-history path
    const uint2 *id;
};

// k_resolve's clamp and quantise (shade_kernels.hip to_unorm8)
__device__ __forceinline__ uint8_t rp_unorm8(float c)
{
    if (!(c > 0.0f)) return 0;
    if (c > 1.0f) c = 1.0f;
    return (uint8_t)(c * 255.0f + 0.5f);
}

struct RpTap {
    float c[3], m[3], n[3], len, z, a;
    uint2 id;
};

// one pixel (x, y) inside the image: everything k_reproject does.  MOTION (pt_film_reproject_motion): the point that goes through the previous
// camera is the film's plane Q (`motion`, 4 floats per pixel {x, y, z, valid}: where the surface point was) instead of the first hit P
template <bool HAS_M, bool MOTION = false>
__device__ __forceinline__ void rp_pixel(const RpConst &rc, const RpFilm &fl, const RpPrev &pv, int x, int y, const float *motion = nullptr)
{
    const int w = (int)rc.w, h = (int)rc.h;
    const size_t p = (size_t)y * rc.w + (uint32_t)x, p3 = 3 * p;
    float cc[3], mc[3] = { 0.f, 0.f, 0.f };
#pragma unroll
    for (int c = 0; c < 3; c++) {
        cc[c] = fl.rgb[p3 + c] * rc.gain;
        if (HAS_M) mc[c] = fl.m2[p3 + c] * rc.gain;
    }
    float oc[3] = { cc[0], cc[1], cc[2] }, om[3] = { mc[0], mc[1], mc[2] }, ol = 1.0f;  // the no-history path
    if (pv.rgb) {  // (uniform)
        const float ap = fl.alpha[p], zp = fl.depth[p];
        const float npx = fl.normal[p3 + 0], npy = fl.normal[p3 + 1], npz = fl.normal[p3 + 2];
        const uint2 idp = fl.id[p];
        // the first hit, back in the world: the ray of primary_ray at jitter (0.5, 0.5), Z / a along it
        const float t = ptm::fdiv(zp, ap);
        float vx, vy, vz;
        ptm::primary_target(rc.cam, (uint32_t)x, (uint32_t)y, 0.5f, 0.5f, vx, vy, vz);
        const float len = ptm::fsqrt((vx * vx + vy * vy) + vz * vz);
        float dx, dy, dz;
        ptm::div3_dominant(vx, vy, vz, len, dx, dy, dz);
        // MOTION: where the surface point was instead (pt_film_motion; one aligned 16-B record), and nothing of the above is computed
        const float *mq = MOTION ? static_cast<const float *>(__builtin_assume_aligned(motion + 4 * p, 16)) : nullptr;
        const float qx = MOTION ? mq[0] : 0.f, qy = MOTION ? mq[1] : 0.f, qz = MOTION ? mq[2] : 0.f, qw = MOTION ? mq[3] : 1.f;
        const float ux = MOTION ? qx - rc.pox : (rc.cam.ox + dx * t) - rc.pox, uy = MOTION ? qy - rc.poy : (rc.cam.oy + dy * t) - rc.poy,
                    uz = MOTION ? qz - rc.poz : (rc.cam.oz + dz * t) - rc.poz;
        // ... and through the previous camera: the inverse of primary_target
        const float vzp = rc.ptz - rc.poz;
        const float s = ptm::fdiv(vzp, uz);
        const float ex = (ux * s + rc.pox) - rc.ptx, ey = (uy * s + rc.poy) - rc.pty;
        const float fx = ((ex + 1.0f) * 0.5f) * rc.cam.w - 0.5f, fy = ((ey + 1.0f) * 0.5f) * rc.cam.h - 0.5f;
        const bool inside = (MOTION ? (ap > 0.0f) & (qw > 0.0f) : (ap > 0.0f)) & (uz * vzp > 0.0f) & (fx > -1.0f) & (fx < rc.cam.w) & (fy > -1.0f) & (fy < rc.cam.h);  // (a NaN fails)
        const float x0f = floorf(fx), y0f = floorf(fy);
        const float bx = fx - x0f, by = fy - y0f;
        const float d = ptm::fsqrt((ux * ux + uy * uy) + uz * uz);
        const int x0 = inside ? (int)x0f : 0, y0 = inside ? (int)y0f : 0;  // in [-1, w - 1] x [-1, h - 1]
        // the loads of all four taps first, from addresses clamped into the image, so that they are in flight together
        RpTap tap[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int qx = min(max(x0 + (k & 1), 0), w - 1), qy = min(max(y0 + (k >> 1), 0), h - 1);
            const size_t q = (size_t)qy * rc.w + (uint32_t)qx, q3 = 3 * q;
            RpTap &tp = tap[k];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                tp.c[c] = pv.rgb[q3 + c];
                tp.m[c] = HAS_M ? pv.m2[q3 + c] : 0.f;
                tp.n[c] = pv.normal[q3 + c];
            }
            tp.len = pv.len[q];
            tp.z = pv.depth[q];
            tp.a = pv.alpha[q];
            tp.id = pv.id[q];
        }
        // ... and every loaded value pinned here, after the last load was issued: a value that only a counting tap uses would otherwise
        // have its load moved behind that tap's test (the compiler did that to one word of tap 0)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            RpTap &tp = tap[k];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                RP_KEEP(tp.c[c]);
                if (HAS_M) RP_KEEP(tp.m[c]);
                RP_KEEP(tp.n[c]);
            }
            RP_KEEP(tp.len); RP_KEEP(tp.z); RP_KEEP(tp.a); RP_KEEP(tp.id.x); RP_KEEP(tp.id.y);
        }
        float W = 0.f, ch[3] = { 0.f, 0.f, 0.f }, mh[3] = { 0.f, 0.f, 0.f }, lh = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {  // k = 2 j + i: j outer, i inner
            const RpTap &tp = tap[k];
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            const float wq = ((k & 1) ? bx : 1.0f - bx) * ((k >> 1) ? by : 1.0f - by);
            // every term into a flag of its own, combined with & : no short-circuit, so no branch (and no load) between the tests
            const bool in_img = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h);
            const bool live = (tp.a > 0.0f) & (tp.len > 0.0f) & (wq > 0.0f);
            const bool same_id = (rc.match_id == 0u) | ((tp.id.x == idp.x) & (tp.id.y == idp.y));
            const bool near_z = fabsf(tp.z - d * tp.a) <= (rc.depth_tol * d) * tp.a;
            const bool facing = ((npx * tp.n[0] + npy * tp.n[1]) + npz * tp.n[2]) >= rc.normal_min * (ap * tp.a);
            const bool ok = in_img & live & same_id & near_z & facing;
            const float w1 = W + wq, l1 = lh + wq * tp.len;
            W = ok ? w1 : W;
            lh = ok ? l1 : lh;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float c1 = ch[c] + wq * tp.c[c];
                ch[c] = ok ? c1 : ch[c];
                if (HAS_M) {
                    const float m1 = mh[c] + wq * tp.m[c];
                    mh[c] = ok ? m1 : mh[c];
                }
            }
        }
        const bool hist = inside & (W >= 0.01f);
        const float lq = fminf(ptm::fdiv(lh, W), rc.max_history);
        const float al = fmaxf(rc.alpha, ptm::fdiv(1.0f, lq + 1.0f));
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float hc = ptm::fdiv(ch[c], W);
            const float nc = hc + al * (cc[c] - hc);
            oc[c] = hist ? nc : cc[c];
            if (HAS_M) {
                const float hm = ptm::fdiv(mh[c], W);
                const float nm = hm + al * (mc[c] - hm);
                om[c] = hist ? nm : mc[c];
            }
        }
        ol = hist ? lq + 1.0f : 1.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        fl.rgb[p3 + c] = oc[c];
        if (HAS_M) fl.m2[p3 + c] = om[c];
    }
    fl.len[p] = ol;
    fl.bgra[p] = make_uchar4(rp_unorm8(oc[2]), rp_unorm8(oc[1]), rp_unorm8(oc[0]), 255);
}

