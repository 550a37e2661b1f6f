// crossings_kernel.h -- the per-lane statements of k_crossings (crossings.hip) that DEFINE pt_crossings_device's result, in a header of their
// own like nearest_kernel.h, so that tests/crossings_host.cpp compiles the very same statements for the host and holds them against a numpy
// restatement without a GPU, under the host's sanitizers: the reciprocal of a direction component (cx_inv), the slab test (cx_slab), a
// triangle's own padded box (cx_own_box), which rays walk at all (cx_live), what counts (cx_counts), row i -> ray (cx_ray) and the writer.  The
// walk itself is the kernel's.
// Wants declared before it: ptm::f3, ptm::RayPre, ptm::ray_setup, ptm::tri_test and ptm::fdiv (the true IEEE divide) -- pt_math.h on the
// device; tests/crossings_host.cpp restates them for the host.  Compile with -ffp-contract=off.
//
// All arithmetic is binary32, every operation rounded on its own, denormals kept.  min and max are SELECTS (a comparison and a choice of one of
// the two operands).  On the values a walking ray meets they choose what ptm::box_test's fminf / fmaxf choose, up to the sign of a zero, which
// no comparison below sees: nothing here is a NaN (next paragraph).
//
// No NaN in the slab test.  A ray walks only if its six components are finite (cx_live); a scene's vertices are finite, so is pad, so are the
// boxes.  inv = 1 / copysign(max(|d|, 1e-20), d) is the correctly rounded reciprocal of a number between 1e-20 and FLT_MAX in magnitude: finite
// and, denormals kept, not zero.  fl(lo - O) is finite or an infinity (two finite operands never give a NaN); times a finite nonzero inv it is
// finite, an infinity or a zero -- there is no 0 * inf, because inv is neither zero nor infinite: a zero difference gives a zero, an infinite
// one an infinity.  min and max of such values are such values; tmin is finite, the bound b is finite or +inf (b > tmin), and
// fl(tf * 1.0000004) is then no NaN either.
//
// The lemma that makes the walk exact.  Let [lo, hi] and [lo', hi'] be fp32 boxes with lo' <= lo and hi' >= hi in every component, and a ray
// that walks.  If cx_slab passes [lo, hi] it passes [lo', hi'].
// Proof, per axis (x stands for any).  Rounding is monotone, so fl(lo'.x - O.x) <= fl(lo.x - O.x) and fl(hi'.x - O.x) >= fl(hi.x - O.x); a
// rounded product with one fixed finite factor is monotone too, increasing for inv.x > 0 and decreasing for inv.x < 0.  For inv.x > 0:
// x0' <= x0 <= x1 <= x1', so min(x0', x1') = x0' <= x0 = min(x0, x1) and max(x0', x1') = x1' >= x1 = max(x0, x1).  For inv.x < 0 the roles
// of x0 and x1 swap: x1' <= x1 <= x0 <= x0'.  Either way the near value does not grow and the far value does not shrink.  max and min of
// several such values with the same tmin and b: tn' <= tn and tf' >= tf; a rounded product with the constant 1.0000004 > 0 is monotone:
// fl(tf * c) <= fl(tf' * c).  So tn' <= tn <= fl(tf * c) <= fl(tf' * c).
// Consequence.  Every builder and the refit give a leaf slot the union (min / max) of fl(min vertex - pad), fl(max vertex + pad) over its
// triangles, with pad = leaf_pad_of(scene box) -- rounding is monotone, so that box contains every one of its triangles' OWN padded boxes as
// fp32 numbers -- and an inner slot the union of its children's.  Hence every box of d_wide on the path from the root to a triangle contains the
// triangle's own padded box, and a ray that passes the own box passes them all.  A walk that tests the slots with cx_slab and never shrinks
// its range therefore reaches every triangle whose own box passes; the leaf step's own-box test drops the others.  The set of triangles that
// count is a property of the triangles and the scene box alone: not of the tree, the builder, the form, the launch shape or a tuning knob.
#pragma once

__device__ __forceinline__ float cx_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float cx_max(float a, float b) { return a > b ? a : b; }

// ---- the reciprocal the slab test multiplies by: the correctly rounded 1 / d, a |d| below 1e-20 (zeros of either sign, denormals) taken as
// 1e-20 with d's sign.  Not ptm::safe_inv, whose v_rcp_f32 is within an ulp of this and has no statement of its bits.
__device__ __forceinline__ float cx_inv(float d)
{
    const float a = __builtin_fabsf(d);
    return ptm::fdiv(1.0f, __builtin_copysignf(a > 1e-20f ? a : 1e-20f, d));
}

// ---- the slab test of ptm::box_test on the range (tmin, b), the range never shrunk
__device__ __forceinline__ bool cx_slab(const ptm::f3 lo, const ptm::f3 hi, const ptm::f3 org, const ptm::f3 inv, float tmin, float b)
{
    const float x0 = (lo.x - org.x) * inv.x, x1 = (hi.x - org.x) * inv.x;
    const float y0 = (lo.y - org.y) * inv.y, y1 = (hi.y - org.y) * inv.y;
    const float z0 = (lo.z - org.z) * inv.z, z1 = (hi.z - org.z) * inv.z;
    const float tn = cx_max(cx_max(cx_min(x0, x1), cx_min(y0, y1)), cx_max(cx_min(z0, z1), tmin));
    const float tf = cx_min(cx_min(cx_max(x0, x1), cx_max(y0, y1)), cx_min(cx_max(z0, z1), b));
    return tn <= tf * 1.0000004f;
}

// ---- a triangle's own padded box: [fl(min(A, B, C) - pad), fl(max(A, B, C) + pad)], what a leaf of this triangle alone would carry
__device__ __forceinline__ void cx_own_box(const ptm::f3 A, const ptm::f3 B, const ptm::f3 C, float pad, ptm::f3 &lo, ptm::f3 &hi)
{
    lo = { cx_min(cx_min(A.x, B.x), C.x) - pad, cx_min(cx_min(A.y, B.y), C.y) - pad, cx_min(cx_min(A.z, B.z), C.z) - pad };
    hi = { cx_max(cx_max(A.x, B.x), C.x) + pad, cx_max(cx_max(A.y, B.y), C.y) + pad, cx_max(cx_max(A.z, B.z), C.z) + pad };
}

// ---- which rays walk: six finite components and a range that is not empty.  Every other ray -- a NaN or an infinity in O or D, a NaN bound,
// b <= tmin -- answers count = winding = 0 without a walk.  (An all-zero direction walks: its shears are 0 / 0 and tri_test rejects every triangle.)
__device__ __forceinline__ bool cx_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }
__device__ __forceinline__ bool cx_live(const ptm::f3 O, const ptm::f3 D, float tmin, float b)
{
    return cx_finite(O.x) && cx_finite(O.y) && cx_finite(O.z) && cx_finite(D.x) && cx_finite(D.y) && cx_finite(D.z) && b > tmin;
}

// ---- what a walking ray keeps: the canonical set-up of the triangle test, and the three reciprocals
struct CxRay { ptm::RayPre pre; ptm::f3 inv; };
__device__ __forceinline__ CxRay cx_setup(const ptm::f3 O, const ptm::f3 D)
{
    CxRay r;
    r.pre = ptm::ray_setup(O, D);
    r.inv = { cx_inv(D.x), cx_inv(D.y), cx_inv(D.z) };
    return r;
}

// ---- does triangle A B C count for the ray, and with which sign: 0 = no; +1 = yes and tri_test's det > 0; -1 = yes and det < 0.
// Own box first (the cheaper test; the two verdicts are independent and both have to hold).  box / tri / t / det (nullable): the verdicts and
// tri_test's values one by one, for the host program -- dead code on the device.
__device__ __forceinline__ int cx_counts(const CxRay &r, float tmin, float b, float pad, const ptm::f3 A, const ptm::f3 B, const ptm::f3 C,
                                         bool *box = nullptr, bool *tri = nullptr, float *t_out = nullptr, float *det_out = nullptr)
{
    ptm::f3 lo, hi;
    cx_own_box(A, B, C, pad, lo, hi);
    const bool in_box = cx_slab(lo, hi, r.pre.org, r.inv, tmin, b);
    if (box) *box = in_box;
    if (!in_box && !tri) return 0;
    float t = 0.f, V, W, det = 0.f;
    const bool hit = ptm::tri_test(r.pre, A, B, C, tmin, b, t, V, W, det);
    if (tri) { *tri = hit; *t_out = hit ? t : 0.f; *det_out = hit ? det : 0.f; }
    if (!(hit && in_box)) return 0;
    return det > 0.f ? 1 : -1;   // (det == 0 and a NaN det were rejected by tri_test)
}

// ---- refill: row i of d_rays6 (origin, direction), or row i of d_points with the descriptor's one direction; the bound.  Rows are only
// 4-byte aligned: dword loads, the idle lanes of a wave take consecutive rows.
__device__ __forceinline__ void cx_ray(const float *__restrict__ rays6, const float *__restrict__ points, const ptm::f3 dir, uint32_t i, ptm::f3 &O, ptm::f3 &D)
{
    if (rays6) {
        const float *p = rays6 + 6 * (size_t)i;
        O = { p[0], p[1], p[2] };
        D = { p[3], p[4], p[5] };
    } else {
        const float *p = points + 3 * (size_t)i;
        O = { p[0], p[1], p[2] };
        D = dir;
    }
}
__device__ __forceinline__ float cx_bound(const float *__restrict__ d_tmax, float tmax, uint32_t i) { return d_tmax ? d_tmax[i] : tmax; }

// ---- finish: word i of d_count and of d_winding, each nullable, plain dword stores
__device__ __forceinline__ void cx_write(uint32_t *__restrict__ count_out, int32_t *__restrict__ winding_out, uint32_t i, uint32_t count, int32_t winding)
{
    if (count_out) count_out[i] = count;
    if (winding_out) winding_out[i] = winding;
}
