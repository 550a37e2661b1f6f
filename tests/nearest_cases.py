"""What tests/test_nearest_cpu.py and tests/test_nearest.py share: the definition of pt_nearest_device (include/pt_api.h) restated in numpy float32,
brute force over all triangles -- the reference of every comparison, computed once per session, never taken from the library and never changed --
and the query sets."""
import numpy as np

import trace_device_cases as tc

f32 = np.float32
MISS = 0xFFFFFFFF
NEAREST_DTYPE = np.dtype([("prim", "<u4"), ("dist2", "<f4"), ("u", "<f4"), ("v", "<f4")])
RADII = np.asarray([0.0, 1e-3, 0.1, np.inf, -1.0, np.nan], f32)   # per-query radii cycle through these by i % 6
BIG_N = 200_001   # queries of the persistent-loop test: with one block per CU every wave draws from at least three strides, and the last is ragged
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "interior")


def _dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(f32) + a[..., 2] * b[..., 2]).astype(f32)


def closest(P, A, B, C):
    """The point of triangle A B C closest to P, arrays [..., 3] float32 that broadcast: every operation a float32 operation of its own, in the
    header's order.  -> u, v, Q [..., 3], dist2, region (0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 interior)"""
    P, A, B, C = (np.asarray(x, f32) for x in (P, A, B, C))
    zero, one = f32(0), f32(1)
    with np.errstate(all="ignore"):
        ab, ac, ap = B - A, C - A, P - A
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = P - B
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = P - C
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e, f = d4 - d3, d5 - d6
        w = e / (e + f)
        s = (va + vb) + vc
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (f >= 0)]
        us = [zero, one, d1 / (d1 - d3), zero, zero, one - w]
        vs = [zero, zero, zero, one, d2 / (d2 - d6), w]
        u, v, region = vb / s, vc / s, np.full(np.shape(d1), 6, np.int32)
        for k in range(5, -1, -1):   # the first condition that holds answers
            u = np.where(conds[k], us[k], u).astype(f32)
            v = np.where(conds[k], vs[k], v).astype(f32)
            region = np.where(conds[k], np.int32(k), region)
        lo = np.where(A < B, A, B)       # selects, as the kernel's: min(min(a, b), c)
        lo = np.where(lo < C, lo, C)
        hi = np.where(A > B, A, B)
        hi = np.where(hi > C, hi, C)
        Q = ((A + ab * u[..., None]).astype(f32) + ac * v[..., None]).astype(f32)
        Q = np.where(Q < lo, lo, Q)
        Q = np.where(Q > hi, hi, Q).astype(f32)
        D = (P - Q).astype(f32)
        dist2 = ((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]).astype(f32) + D[..., 2] * D[..., 2]).astype(f32)
    shape = dist2.shape
    return np.broadcast_to(u, shape), np.broadcast_to(v, shape), Q, dist2, np.broadcast_to(region, shape)


def box_dist2(P, lo, hi):
    """per axis max(max(lo - P, P - hi), 0) by selects, then the squares and sums of dist2"""
    P, lo, hi = (np.asarray(x, f32) for x in (P, lo, hi))
    with np.errstate(all="ignore"):
        a, b = (lo - P).astype(f32), (P - hi).astype(f32)
        m = np.where(a > b, a, b)
        m = np.where(m > 0, m, f32(0)).astype(f32)
        return ((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]).astype(f32) + m[..., 2] * m[..., 2]).astype(f32)


def radius2(m):
    """-> (r2, valid): r2 = m * m where m >= 0; a negative or NaN m finds nothing"""
    m = np.asarray(m, f32)
    with np.errstate(all="ignore"):
        valid = m >= 0
        return (m * m).astype(f32), valid


def triangles(v, idx):
    return np.asarray(v, f32).reshape(-1, 3)[np.asarray(idx).reshape(-1, 3)]   # [T, 3 vertices, 3]


class Brute:
    """The answers of one (triangles, points, radii): records [n] NEAREST_DTYPE, point [n, 3], region [n] (-1 behind a miss), ties [n] (triangles
    that share the winning dist2)"""

    def __init__(self, tris, points, radii=None, pairs_per_chunk=1 << 20):
        tris, points = np.asarray(tris, f32), np.ascontiguousarray(points, f32)
        n, T = len(points), len(tris)
        r2, valid = radius2(np.full(n, np.inf, f32) if radii is None else radii)
        self.points, self.radii = points, radii
        self.rec = np.zeros(n, NEAREST_DTYPE)
        self.rec["prim"] = MISS
        self.point = np.zeros((n, 3), f32)
        self.region = np.full(n, -1, np.int32)
        self.ties = np.zeros(n, np.int64)
        step = max(1, pairs_per_chunk // max(T, 1))
        for i0 in range(0, n, step):
            sl = slice(i0, min(n, i0 + step))
            u, v, Q, d, reg = closest(points[sl, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
            with np.errstate(invalid="ignore"):
                ok = (d <= r2[sl, None]) & valid[sl, None]          # (a NaN dist2 is within nothing)
            dmin = np.where(ok, d, f32(np.inf)).min(1)
            win = ok & (d == dmin[:, None])
            found = win.any(1)
            w = win.argmax(1)                                        # the first: the lowest primitive id
            rows = np.arange(sl.stop - sl.start)
            k = np.flatnonzero(found) + i0
            self.rec["prim"][k] = w[found]
            self.rec["dist2"][k] = d[rows, w][found]
            self.rec["u"][k] = u[rows, w][found]
            self.rec["v"][k] = v[rows, w][found]
            self.point[k] = Q[rows, w][found]
            self.region[k] = reg[rows, w][found]
            self.ties[sl] = win.sum(1)

    @property
    def found(self):
        return self.rec["prim"] != MISS


def scene_box(tris, scale=1.5):
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * scale
    return (c - h).astype(f32), (c + h).astype(f32)


def specials(tris):
    """all vertices, edge midpoints and centroids"""
    A, B, C = tris[:, 0], tris[:, 1], tris[:, 2]
    mid = lambda a, b: ((a + b) * f32(0.5)).astype(f32)
    return np.concatenate([A, B, C, mid(A, B), mid(B, C), mid(C, A), ((A + B + C) / f32(3)).astype(f32)]).astype(f32)


def surface_points(tris, n, rng, offset):
    """points on random triangles, moved along the unit normal by +-offset (a float or [n] array)"""
    t = rng.integers(0, len(tris), n)
    b = rng.dirichlet((1, 1, 1), n).astype(f32)
    p = (tris[t] * b[:, :, None]).sum(1)
    nrm = np.cross(tris[t, 1] - tris[t, 0], tris[t, 2] - tris[t, 0]).astype(np.float64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1), 1e-30)[:, None]
    sign = np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0)
    return (p + nrm * (sign * offset)[:, None]).astype(f32)


def make_queries(tris, n=1000, seed=7, surface_share=0.3):
    """n points in a seeded random order: every vertex, edge midpoint and centroid (while they fit half of n), surface points moved by +-1e-4
    along the normal, the rest uniform in 1.5x the scene's box"""
    rng = np.random.default_rng(seed)
    sp = specials(tris)
    if len(sp) > n // 2:
        sp = sp[rng.permutation(len(sp))[:n // 2]]
    n_surf = int((n - len(sp)) * surface_share)
    lo, hi = scene_box(tris)
    uni = rng.uniform(lo, hi, (n - len(sp) - n_surf, 3)).astype(f32)
    q = np.concatenate([sp, surface_points(tris, n_surf, rng, 1e-4), uni]).astype(f32)
    return np.ascontiguousarray(q[rng.permutation(n)])


def cycled_radii(n):
    return np.ascontiguousarray(RADII[np.arange(n) % len(RADII)])


_cache = {}


def cached(key, make):
    """a named case, computed once per session and shared by the tests that need it"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def box_tris(cornell_arrays):
    return triangles(cornell_arrays[0], cornell_arrays[1])


def box_set(cornell_arrays):
    """the 1 000-query set on the Cornell box: unbounded, under the cycled radii, under the uniform radius 0.1"""
    def make():
        tris = box_tris(cornell_arrays)
        q = make_queries(tris)
        return {"free": Brute(tris, q), "cycled": Brute(tris, q, cycled_radii(len(q))), "uniform": Brute(tris, q, np.full(len(q), 0.1, f32))}
    return cached("box", make)


def box_big(cornell_arrays):
    return cached("box_big", lambda: Brute(box_tris(cornell_arrays), make_queries(box_tris(cornell_arrays), BIG_N, seed=8)))


def box_moved(cornell_arrays):
    """the box with its short block moved (tc.move_short_box), same queries"""
    def make():
        v = tc.move_short_box(cornell_arrays[0])
        return v, Brute(triangles(v, cornell_arrays[1]), box_set(cornell_arrays)["free"].points)
    return cached("box_moved", make)


SOUP = (4096, 11)


def soup_set():
    """tc.soup(4096, 11) with 2 000 queries"""
    def make():
        v, i, f = tc.soup(*SOUP)
        tris = triangles(v, i)
        return (v, i, f), Brute(tris, make_queries(tris, 2000, seed=9))
    return cached("soup", make)


# ---- float64, for the restatement's own error -----------------------------------------------------------------------------------------------
def dist_f64(P, tris):
    """exact-as-float64 distance [n, T] of points to triangles: the same region algorithm in float64 (Ericson 5.1.5)"""
    P = np.asarray(P, np.float64)[:, None, :]
    A, B, C = (np.asarray(tris, np.float64)[None, :, k] for k in range(3))
    dot = lambda a, b: (a * b).sum(-1)
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = B - A, C - A, P - A, P - B, P - C
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e, f = d4 - d3, d5 - d6
        w, s = e / (e + f), va + vb + vc
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (f >= 0)]
        us, vs = [0.0, 1.0, d1 / (d1 - d3), 0.0, 0.0, 1 - w], [0.0, 0.0, 0.0, 1.0, d2 / (d2 - d6), w]
        u, v = vb / s, vc / s
        for k in range(5, -1, -1):
            u, v = np.where(conds[k], us[k], u), np.where(conds[k], vs[k], v)
        Q = A + ab * u[..., None] + ac * v[..., None]
        return np.sqrt(((P - Q) ** 2).sum(-1))
