// self_leaf.h -- when a bounce ray may skip the leaf of the triangle it starts on (k_fused; DESIGN.md section 6, "Bounce rays skip their own leaf").
//
// A bounce ray starts ON triangle p, so its origin lies inside the box of p's leaf and the walk visits that leaf first -- to find t ~ 0, which
// `t > tmin` rejects.  The walk may leave the leaf out when the oracle's arithmetic (pair_leaf.h, the watertight test) CANNOT accept either
// triangle of it inside (tmin, tmax).  Per ray that is one compare,
//
//     dt >= max(thr[p], c1 * g[p]),        dt = dir . n_p as the bounce computes it,
//
// with two per-triangle values fixed when the scene is packed (leaf_rule) and one per launch (launch_c1).  The bound behind it, u = 2^-24, E the
// scene's largest coordinate magnitude, D the leaf's diameter, A the smaller area of its triangles: a self-leaf triangle that passes the edge
// test yields
//
//     t_computed <= u * (C_ORIGIN * E + C_RANGE * D + C_SHAPE * D^3 / A) / dt = u * g / dt,
//
// so dt >= SAFETY * u * g / tmin gives t_computed <= tmin / SAFETY.  thr holds what the bound assumes: the fold of a fan pair (a ray at least
// four times steeper than the fold stays clear of the other half's plane: |dir . n_q| >= 0.7 dt), a floor of 1/16 for pairs, and
// C_VALID * u * D^2 / A, under which the edge functions' rounding errors are not small against their sum.
//
// One header for host and device: scene_build.hip evaluates leaf_rule per triangle, fused.hip launch_c1 per launch, and the CPU tests call the
// same functions through libpt_host.so (pth_self_leaf_rule, pth_self_leaf_c1).  Plain C++: no HIP header.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_SL_HD __host__ __device__ inline
#else
#define PT_SL_HD inline
#endif

namespace ptsl {

// (the constants: DESIGN.md section 6 derives each from pair_leaf.h and the bounce's position code)
constexpr double U24 = 1.0 / 16777216.0;
constexpr double C_ORIGIN = 27.0;        // the origin off p's plane (barycentric interpolation: <= 10 u E), seen from a fold's other half: 20 / 0.74
constexpr double C_RANGE = 14.0;         // rounding of the three depths, of T and of T / det for weights in [0, 1]
constexpr double C_SHAPE_SINGLE = 145.0; // the weights' error against the exact barycentrics: 4 * 36.3 u D^2 of an edge function over det = 2 A dt
constexpr double C_SHAPE_PAIR = 262.0;   // ... of the other half, whose plane the ray meets at >= 0.7 dt: 207 (1 + kappa / thr), kappa / thr <= 0.26
constexpr double C_VALID = 1162.0;       // 4 eps_U / det <= 1 / 8, twice over
constexpr double SAFETY = 1.5;           // the bound is first order in u
constexpr double FOLD_STEEPER = 4.0;     // thr >= 4 sin(fold)
constexpr double FOLD_MAX_SIN = 0.25;    // a fold beyond this never skips
constexpr double PAIR_FLOOR = 1.0 / 16.0;
constexpr uint32_t CODE_NONE = 0u;       // the root's code: no child carries it
constexpr uint32_t CODE_BITS = 0x3FFFu;  // g's low mantissa bits carry the leaf's 14-bit code

// the compact walk's code of a leaf (lds_scene.h: C14_LEAF | (count - 1) << 11 | first)
PT_SL_HD constexpr uint32_t leaf_code14(uint32_t first, uint32_t count) { return 0x2000u | ((count - 1u) << 11) | (first & 0x7FFu); }

struct Rule {
    float thr;  // +inf: never skip
    float g;    // a length; low 14 mantissa bits zero (rounded up)
};

PT_SL_HD float up_f32(double x)  // the smallest float >= x (x >= 0)
{
    float f = (float)x;
    if ((double)f < x) f = nextafterf(f, INFINITY);
    return f;
}
PT_SL_HD float up_clear14(double x)  // ... whose low 14 mantissa bits are zero
{
    union { float f; uint32_t u; } v;
    v.f = up_f32(x);
    if (!(v.f < INFINITY)) return INFINITY;
    if (v.u & CODE_BITS) v.u = (v.u | CODE_BITS) + 1u;
    return v.f;
}

// Triangle p = (e0, own, e1) of a leaf; `other`: the apex of the leaf's second triangle (e0, e1, other) across the shared edge e0-e1, or null for a
// single-triangle leaf.  E: the scene's largest coordinate magnitude.
PT_SL_HD Rule leaf_rule(const float *e0, const float *e1, const float *own, const float *other, float E)
{
    const Rule never = { INFINITY, INFINITY };
    const double a[3] = { (double)own[0] - e0[0], (double)own[1] - e0[1], (double)own[2] - e0[2] };
    const double b[3] = { (double)e1[0] - e0[0], (double)e1[1] - e0[1], (double)e1[2] - e0[2] };
    const double N[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
    const double nn = sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]), bb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    if (!(nn > 0.0) || !(nn < (double)INFINITY) || !(bb > 0.0) || !((double)E > 0.0) || !(E < INFINITY)) return never;  // degenerate, not finite
    double area = 0.5 * nn;
    auto dist2 = [](const float *p, const float *q) {
        const double x = (double)p[0] - q[0], y = (double)p[1] - q[1], z = (double)p[2] - q[2];
        return x * x + y * y + z * z;
    };
    double d2 = fmax(fmax(dist2(e0, e1), dist2(e0, own)), dist2(e1, own));
    double thr = 0.0, shape = C_SHAPE_SINGLE;
    if (other) {
        const double c[3] = { (double)other[0] - e0[0], (double)other[1] - e0[1], (double)other[2] - e0[2] };
        const double n[3] = { N[0] / nn, N[1] / nn, N[2] / nn }, e[3] = { b[0] / bb, b[1] / bb, b[2] / bb };
        double m[3] = { n[1] * e[2] - n[2] * e[1], n[2] * e[0] - n[0] * e[2], n[0] * e[1] - n[1] * e[0] };  // in p's plane, across the shared edge
        const double own_m = a[0] * m[0] + a[1] * m[1] + a[2] * m[2];
        if (!(own_m != 0.0)) return never;
        if (own_m > 0.0) { m[0] = -m[0]; m[1] = -m[1]; m[2] = -m[2]; }  // (p lies on the negative side)
        d2 = fmax(d2, fmax(fmax(dist2(other, e0), dist2(other, e1)), dist2(other, own)));
        const double rho = c[0] * m[0] + c[1] * m[1] + c[2] * m[2], h = fabs(c[0] * n[0] + c[1] * n[1] + c[2] * n[2]);
        if (!(rho > sqrt(d2) * (1.0 / 1024.0))) return never;  // the apex does not project strictly across the shared edge
        const double M[3] = { b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0] };
        const double mm = sqrt(M[0] * M[0] + M[1] * M[1] + M[2] * M[2]);
        if (!(mm > 0.0) || !(mm < (double)INFINITY)) return never;
        area = fmin(area, 0.5 * mm);
        const double kappa = h / rho, sin_fold = kappa / sqrt(1.0 + kappa * kappa);
        if (!(sin_fold <= FOLD_MAX_SIN)) return never;
        thr = fmax(FOLD_STEEPER * sin_fold, PAIR_FLOOR);
        shape = C_SHAPE_PAIR;
    }
    const double D = sqrt(d2);
    thr = fmax(thr, C_VALID * U24 * d2 / area);
    if (!(thr < 1.0)) return never;  // (dt <= 1: nothing to gain, and the bound's assumptions are in doubt)
    const double g = C_ORIGIN * (double)E + C_RANGE * D + shape * D * d2 / area;
    Rule r;
    r.thr = up_f32(thr * (1.0 + 1.0 / 1024.0) + 1.0 / 1048576.0);  // (dt itself and the stored normal carry a few u: the margin)
    r.g = up_clear14(g);
    if (!(r.g < INFINITY)) return never;
    return r;
}

// The launch's factor: dt >= c1 * g  <=>  u * g / dt <= tmin / SAFETY.  +inf (no ray skips) unless tmin is a positive finite number.
PT_SL_HD float launch_c1(float tmin)
{
    if (!(tmin > 0.f) || !(tmin < INFINITY)) return INFINITY;
    return up_f32(SAFETY * U24 / (double)tmin * (1.0 + 1.0 / 1048576.0));
}

// What the kernel evaluates: per triangle and launch the limit (when the tables are staged), per bounce one compare with it -> the code the
// walk leaves out, CODE_NONE for a ray that visits its own leaf like any other.  g_word: g with the leaf's code in its low mantissa bits (>= g)
PT_SL_HD float skip_limit(float thr, uint32_t g_word, float c1)
{
    union { uint32_t u; float f; } v;
    v.u = g_word;
    return fmaxf(thr, c1 * v.f);
}
PT_SL_HD uint32_t skip_code(float dt, float thr, uint32_t g_word, float c1)
{
    return dt >= skip_limit(thr, g_word, c1) ? (g_word & CODE_BITS) : CODE_NONE;
}

}  // namespace ptsl
