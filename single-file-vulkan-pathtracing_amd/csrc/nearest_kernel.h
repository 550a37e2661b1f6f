// nearest_kernel.h -- the per-lane statements of k_nearest (nearest.hip) that DEFINE pt_nearest_device's result, in a header of their own like
// trace_fused_kernel.h, so that tests/nearest_host.cpp compiles the very same statements for the host and holds them against a numpy restatement
// without a GPU, under the host's sanitizers: the closest point of a triangle (nr_closest), the distance to a box (nr_box_dist2), the accept rule
// (nr_accept), row i of d_points -> P (nr_point), the radius rule (nr_radius2) and the two output writers.  The walk itself is the kernel's.
// Wants declared before it: float4 and ptm::fdiv (the true IEEE divide).  Compile with -ffp-contract=off.
//
// All arithmetic is binary32, every operation rounded on its own, denormals kept; dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z.  min, max and
// the clamp are SELECTS (a comparison and a choice of one of the two operands), never fminf / fmaxf: a NaN stays a NaN where it is chosen, and no
// operand is re-quieted or has its zero's sign changed.
//
// The lemma that makes pruning exact.  Let [lo, hi] be any fp32 box that contains the triangle's three vertices, and dist2 and Q what nr_closest
// returns for a query P, neither NaN.  Then nr_box_dist2(P, lo, hi) <= dist2.
// Proof, per axis (x stands for any): nr_closest clamps Q.x into [min(A.x, B.x, C.x), max(A.x, B.x, C.x)], which lies inside [lo.x, hi.x], so
// lo.x <= Q.x <= hi.x.  Then P.x - hi.x <= P.x - Q.x and lo.x - P.x <= Q.x - P.x in exact arithmetic, and since rounding is monotone and
// fl(Q.x - P.x) = -fl(P.x - Q.x): fl(P.x - hi.x) <= D.x and fl(lo.x - P.x) <= -D.x, where D.x = fl(P.x - Q.x).  So the box's term
// b.x = max(max(fl(lo.x - P.x), fl(P.x - hi.x)), 0) satisfies 0 <= b.x <= |D.x|.  Squares of non-negative numbers, rounded, are monotone:
// fl(b.x * b.x) <= fl(D.x * D.x); a rounded sum of two non-negative terms is monotone in each; the two expressions add the same three terms in the
// same order, (x + y) + z.  Hence the box's sum is <= dist2.  (In exact arithmetic the clamp does nothing: Q is a convex combination of the
// vertices.  In binary32 it moves a Q that rounding pushed outside of the triangle's box back onto it -- by an ulp or two -- and dist2 is computed
// from the clamped Q, so the inequality holds for the number the caller gets, not for an idealised one.)
// Consequence: a subtree whose box lies farther than the best dist2 found so far (strictly) holds no triangle with a dist2 that small, whatever the
// tree; a subtree at exactly that distance may hold an equal dist2 with a lower primitive id and is visited.
#pragma once

constexpr uint32_t NR_MISS = 0xFFFFFFFFu;

struct NrVec { float x, y, z; };
__device__ __forceinline__ float nr_dot(const NrVec &a, const NrVec &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ NrVec nr_sub(const NrVec &a, const NrVec &b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ float nr_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float nr_max(float a, float b) { return a > b ? a : b; }

// ---- the closest point of triangle A B C to P: the region algorithm of Ericson, Real-Time Collision Detection 5.1.5, in the order of
// include/pt_api.h.  (u, v): the weights of B and C (pt_hit's convention); q: the point, clamped to the triangle's box; dist2 = |P - q|^2.
// region: which of the seven branches answered (0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 interior) -- the tests' coverage count, dead code on the device.
struct NrClosest { float u, v, dist2; NrVec q; int region; };
__device__ __forceinline__ NrClosest nr_closest(const NrVec &P, const NrVec &A, const NrVec &B, const NrVec &C)
{
    const NrVec ab = nr_sub(B, A), ac = nr_sub(C, A), ap = nr_sub(P, A);
    const float d1 = nr_dot(ab, ap), d2 = nr_dot(ac, ap);
    float u = 0.f, v = 0.f;
    int region = 0;
    bool done = false;
    if (d1 <= 0.f && d2 <= 0.f) { u = 0.f; v = 0.f; region = 0; done = true; }
    const NrVec bp = nr_sub(P, B);
    const float d3 = nr_dot(ab, bp), d4 = nr_dot(ac, bp);
    if (!done && d3 >= 0.f && d4 <= d3) { u = 1.f; v = 0.f; region = 1; done = true; }
    const float vc = d1 * d4 - d3 * d2;
    if (!done && vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { u = ptm::fdiv(d1, d1 - d3); v = 0.f; region = 2; done = true; }
    const NrVec cp = nr_sub(P, C);
    const float d5 = nr_dot(ab, cp), d6 = nr_dot(ac, cp);
    if (!done && d6 >= 0.f && d5 <= d6) { u = 0.f; v = 1.f; region = 3; done = true; }
    const float vb = d5 * d2 - d1 * d6;
    if (!done && vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { u = 0.f; v = ptm::fdiv(d2, d2 - d6); region = 4; done = true; }
    const float va = d3 * d6 - d5 * d4, e = d4 - d3, f = d5 - d6;
    if (!done && va <= 0.f && e >= 0.f && f >= 0.f) {
        const float w = ptm::fdiv(e, e + f);
        u = 1.f - w; v = w; region = 5; done = true;
    }
    if (!done) {
        const float s = (va + vb) + vc;
        u = ptm::fdiv(vb, s); v = ptm::fdiv(vc, s); region = 6;
    }
    NrClosest r;
    r.u = u; r.v = v; r.region = region;
    const auto comp = [&](float a, float b, float c, float eab, float eac, float p, float &q) {
        const float lo = nr_min(nr_min(a, b), c), hi = nr_max(nr_max(a, b), c);
        float x = (a + eab * u) + eac * v;
        x = x < lo ? lo : x;   // (selects: a NaN x fails both comparisons and stays)
        x = x > hi ? hi : x;
        q = x;
        return p - x;
    };
    const float dx = comp(A.x, B.x, C.x, ab.x, ac.x, P.x, r.q.x);
    const float dy = comp(A.y, B.y, C.y, ab.y, ac.y, P.y, r.q.y);
    const float dz = comp(A.z, B.z, C.z, ab.z, ac.z, P.z, r.q.z);
    r.dist2 = (dx * dx + dy * dy) + dz * dz;
    return r;
}

// ---- the distance of P to the box [lo, hi], squared: per axis max(max(lo - P, P - hi), 0), then the same squares and sums as dist2.  Never NaN
// for a finite box: a NaN difference loses both selects and the axis counts 0 (a NaN query's dist2 is NaN on every triangle, which never wins, so
// whatever the walk prunes for it is right).
__device__ __forceinline__ float nr_box_axis(float lo, float hi, float p) { return nr_max(nr_max(lo - p, p - hi), 0.f); }
__device__ __forceinline__ float nr_box_dist2(const NrVec &P, const NrVec &lo, const NrVec &hi)
{
    const float bx = nr_box_axis(lo.x, hi.x, P.x), by = nr_box_axis(lo.y, hi.y, P.y), bz = nr_box_axis(lo.z, hi.z, P.z);
    return (bx * bx + by * by) + bz * bz;
}

// ---- the radius rule: the search radius m (d_max_dist[i], or desc.max_dist) -> the bound r2 on dist2.  m >= 0: m * m (+inf stays +inf, -0 is 0);
// a negative or NaN m finds nothing: -1, which no dist2 (>= 0 or NaN) is within and no box distance (>= 0) is either.
__device__ __forceinline__ float nr_radius(const float *__restrict__ d_max_dist, float max_dist, uint32_t i) { return d_max_dist ? d_max_dist[i] : max_dist; }
__device__ __forceinline__ float nr_radius2(float m) { return m >= 0.f ? m * m : -1.f; }

// ---- the accept rule.  The walk keeps (best_d, best_prim), started at (r2, NR_MISS): a triangle wins over what is held when its dist2 is
// smaller, or equal with a lower primitive id.  Started so, "dist2 <= r2" needs no test of its own (NR_MISS is above every id), a NaN dist2 fails
// both comparisons, and over any set of triangles, in any order, the holder ends at the least dist2 <= r2 and the lowest id among those.
__device__ __forceinline__ bool nr_accept(float dist2, uint32_t prim, float best_d, uint32_t best_prim)
{
    return dist2 < best_d || (dist2 == best_d && prim < best_prim);
}

// ---- refill: row i of d_points.  Rows are 12 B apart and only 4-byte aligned: three dword loads per lane; the idle lanes of a wave take
// consecutive rows, so the wave's loads consume contiguous bytes.
__device__ __forceinline__ NrVec nr_point(const float *__restrict__ points, uint32_t i)
{
    const float *p = points + 3 * (size_t)i;
    return { p[0], p[1], p[2] };
}

// ---- finish: row i of d_nearest (pt_nearest {prim, dist2, u, v}: four dwords, written one by one -- the caller's array is only known to be
// 4-byte aligned) and of d_point.  A query that found nothing (prim == NR_MISS): prim = 0xFFFFFFFF and +0.0 everywhere else.
__device__ __forceinline__ void nr_write_nearest(uint32_t *__restrict__ out4, uint32_t i, uint32_t prim, float dist2, float u, float v)
{
    const bool miss = prim == NR_MISS;
    uint32_t *o = out4 + 4 * (size_t)i;
    o[0] = prim;
    o[1] = miss ? 0u : __builtin_bit_cast(uint32_t, dist2);
    o[2] = miss ? 0u : __builtin_bit_cast(uint32_t, u);
    o[3] = miss ? 0u : __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ void nr_write_point(float *__restrict__ out3, uint32_t i, uint32_t prim, const NrVec &q)
{
    const bool miss = prim == NR_MISS;
    float *o = out3 + 3 * (size_t)i;
    o[0] = miss ? 0.f : q.x;
    o[1] = miss ? 0.f : q.y;
    o[2] = miss ? 0.f : q.z;
}
