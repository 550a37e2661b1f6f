"""What tests/test_crossings_cpu.py and tests/test_crossings.py share: the definition of pt_crossings_device (include/pt_api.h) restated in numpy
float32 -- ray_setup, tri_test, the triangle's own padded box, the slab test, brute force over all triangles; the reference of every comparison,
computed once per session, never taken from the library and never changed -- the closed meshes and the ray sets."""
import numpy as np

import trace_device_cases as tc

f32 = np.float32
INF = f32(np.inf)
BIG_N = 200_001   # rays of the persistent-loop test: with one block per CU every wave draws from at least three strides, and the last is ragged
SOUP = (4096, 11)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------
def _sel(k, x, y, z):
    return np.where(k == 0, x, np.where(k == 1, y, z))


def _min(a, b):
    return np.where(a < b, a, b)   # a < b ? a : b


def _max(a, b):
    return np.where(a > b, a, b)   # a > b ? a : b


def ray_setup(D):
    """ptm::ray_setup: D [..., 3] float32 -> kz, Sx, Sy, Sz (dominant axis first-wins, shear by true divides)"""
    dx, dy, dz = D[..., 0], D[..., 1], D[..., 2]
    with np.errstate(all="ignore"):
        kz = np.where(np.abs(dy) > np.abs(dx), 1, 0)
        kz = np.where(np.abs(dz) > np.abs(_sel(kz, dx, dy, dz)), 2, kz)
        dkx, dky, dkz = _sel(kz, dy, dz, dx), _sel(kz, dz, dx, dy), _sel(kz, dx, dy, dz)
        return kz, (dkx / dkz).astype(f32), (dky / dkz).astype(f32), (f32(1) / dkz).astype(f32)


def tri_test(O, pre, A, B, C, tmin, b):
    """ptm::tri_test, arrays that broadcast: -> accepted, t, det (t and det 0 where rejected)"""
    kz, Sx, Sy, Sz = pre
    with np.errstate(all="ignore"):
        def shear(P):
            p = (P - O).astype(f32)
            pkx, pky, pkz = _sel(kz, p[..., 1], p[..., 2], p[..., 0]), _sel(kz, p[..., 2], p[..., 0], p[..., 1]), _sel(kz, p[..., 0], p[..., 1], p[..., 2])
            return (pkx - (Sx * pkz).astype(f32)).astype(f32), (pky - (Sy * pkz).astype(f32)).astype(f32), pkz
        Ax, Ay, Akz = shear(A)
        Bx, By, Bkz = shear(B)
        Cx, Cy, Ckz = shear(C)
        U = ((Cx * By).astype(f32) - (Cy * Bx).astype(f32)).astype(f32)
        V = ((Ax * Cy).astype(f32) - (Ay * Cx).astype(f32)).astype(f32)
        W = ((Bx * Ay).astype(f32) - (By * Ax).astype(f32)).astype(f32)
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = ((U + V).astype(f32) + W).astype(f32)
        Az, Bz, Cz = (Sz * Akz).astype(f32), (Sz * Bkz).astype(f32), (Sz * Ckz).astype(f32)
        T = (((U * Az).astype(f32) + (V * Bz).astype(f32)).astype(f32) + (W * Cz).astype(f32)).astype(f32)
        t = (T / det).astype(f32)
        ok = ~mixed & ~(det == 0) & (t > tmin) & (t < b)
    return ok, np.where(ok, t, f32(0)).astype(f32), np.where(ok, det, f32(0)).astype(f32)


def inv_of(D):
    """1 / copysign(max(|d|, 1e-20), d), the correctly rounded reciprocal"""
    with np.errstate(all="ignore"):
        a = np.abs(D)
        return (f32(1) / np.copysign(np.where(a > f32(1e-20), a, f32(1e-20)), D)).astype(f32)


def slab(lo, hi, O, inv, tmin, b):
    """ptm::box_test's arithmetic on the range (tmin, b): -> passes"""
    with np.errstate(all="ignore"):
        t0 = ((lo - O).astype(f32) * inv).astype(f32)
        t1 = ((hi - O).astype(f32) * inv).astype(f32)
        mn, mx = _min(t0, t1), _max(t0, t1)
        tn = _max(_max(mn[..., 0], mn[..., 1]), _max(mn[..., 2], tmin))
        tf = _min(_min(mx[..., 0], mx[..., 1]), _min(mx[..., 2], b))
        return tn <= (tf * f32(1.0000004)).astype(f32)


def own_box(A, B, C, pad):
    pad = np.asarray(pad, f32)[..., None]
    lo = (_min(_min(A, B), C) - pad).astype(f32)
    hi = (_max(_max(A, B), C) + pad).astype(f32)
    return lo, hi


def live(O, D, tmin, b):
    with np.errstate(all="ignore"):
        return np.isfinite(O).all(-1) & np.isfinite(D).all(-1) & (b > tmin)


def pad_of(tris):
    """scene_build.hip leaf_pad_of: the largest absolute ordinate of the scene's box times 2^-18"""
    return f32(np.abs(np.asarray(tris, f32)).max() * f32(3.814697265625e-06))


def pair_verdicts(O, D, tmin, b, A, B, C, pad):
    """one ray against one triangle, all [..., 3] / [...] arrays that broadcast -> dict: live, box, tri, t, det, s (0, +1, -1: what it adds)"""
    O, D, A, B, C = (np.asarray(x, f32) for x in (O, D, A, B, C))
    tmin, b = np.asarray(tmin, f32), np.asarray(b, f32)
    lo, hi = own_box(A, B, C, pad)
    box = slab(lo, hi, O, inv_of(D), tmin, b)
    tri, t, det = tri_test(O, ray_setup(D), A, B, C, tmin, b)
    with np.errstate(all="ignore"):
        s = np.where(tri & box, np.where(det > 0, 1, -1), 0).astype(np.int32)
    return {"live": live(O, D, tmin, b), "box": box, "tri": tri, "t": t, "det": det, "s": s, "lo": lo, "hi": hi}


def triangles(v, idx):
    return np.asarray(v, f32).reshape(-1, 3)[np.asarray(idx).reshape(-1, 3)]   # [T, 3 vertices, 3]


class Brute:
    """The answers of one (triangles, rays, bounds): count [n] uint32, winding [n] int32; phantoms [n]: triangles tri_test accepts and the own
    box drops; first_t / first_prim: the least accepted t and the lowest id at it (inf / -1 for none); ts (keep_t): the counted t's sorted, inf-padded"""

    def __init__(self, tris, rays, bounds=None, tmin=0.0, tmax=np.inf, pad=None, keep_t=False, pairs_per_chunk=1 << 20):
        tris, rays = np.asarray(tris, f32), np.ascontiguousarray(rays, f32)
        n, T = len(rays), len(tris)
        self.rays, self.tmin = rays, f32(tmin)
        self.bounds = np.full(n, tmax, f32) if bounds is None else np.ascontiguousarray(bounds, f32)
        self.pad = pad_of(tris) if pad is None else f32(pad)
        self.count, self.winding = np.zeros(n, np.uint32), np.zeros(n, np.int32)
        self.phantoms = np.zeros(n, np.int64)
        self.first_t, self.first_prim = np.full(n, np.inf, f32), np.full(n, -1, np.int64)
        ts = []
        step = max(1, pairs_per_chunk // max(T, 1))
        for i0 in range(0, n, step):
            sl = slice(i0, min(n, i0 + step))
            O, D = rays[sl, None, :3], rays[sl, None, 3:]
            r = pair_verdicts(O, D, self.tmin, self.bounds[sl, None], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2], self.pad)
            alive = r["live"]                       # [m, 1]: a ray that does not walk answers 0
            counts = (r["s"] != 0) & alive
            self.count[sl] = counts.sum(1)
            self.winding[sl] = np.where(alive, r["s"], 0).sum(1)
            self.phantoms[sl] = (r["tri"] & ~r["box"] & alive).sum(1)
            t_acc = np.where(r["tri"] & alive, r["t"], INF)
            self.first_t[sl] = t_acc.min(1)
            hit = np.isfinite(self.first_t[sl])
            self.first_prim[sl] = np.where(hit, (t_acc == self.first_t[sl, None]).argmax(1), -1)
            if keep_t:
                ts.append(np.sort(np.where(counts, r["t"], INF), 1)[:, :64])
        if keep_t:
            self.ts = np.concatenate(ts) if ts else np.zeros((0, 0), f32)


# ---- closed, consistently oriented meshes (outward: cross(B - A, C - A) points out of the solid) ------------------------------------------------
CENTRE = np.asarray([0.13, -0.21, 0.07])


def _grid_mesh(P, wrap_u, wrap_v):
    """P [nu, nv, 3] -> triangles of the quads (i, j) (i+1, j) (i+1, j+1) (i, j+1), wrapping as told"""
    nu, nv = P.shape[:2]
    out = []
    for i in range(nu if wrap_u else nu - 1):
        for j in range(nv if wrap_v else nv - 1):
            a, b, c, d = P[i, j], P[(i + 1) % nu, j], P[(i + 1) % nu, (j + 1) % nv], P[i, (j + 1) % nv]
            out += [(a, b, c), (a, c, d)]
    return out


def _outward(tris, inside_point_of):
    """orient every triangle so that its normal points away from inside_point_of(centroid)"""
    t = np.asarray(tris, np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    c = t.mean(1)
    flip = ((c - inside_point_of(c)) * n).sum(1) < 0
    t[flip] = t[flip][:, [0, 2, 1]]
    return t


def cube(h=0.75):
    """12 triangles, |x - c| <= h"""
    s = np.asarray([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float64) * h
    quads = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 3, 7, 4)]
    tris = [(s[a], s[b], s[c]) for a, b, c, d in quads] + [(s[a], s[c], s[d]) for a, b, c, d in quads]
    t = _outward(tris, lambda c: np.zeros_like(c)) + CENTRE
    return t.astype(f32)


def sphere(R=1.0, seg=32, rings=16):
    """UV sphere: 2 * seg * (rings - 1) = 960 triangles (the caps are single triangles)"""
    th = np.linspace(0, np.pi, rings + 1)[1:-1]
    ph = np.arange(seg) * 2 * np.pi / seg
    P = R * np.stack([np.sin(th)[None, :] * np.cos(ph)[:, None], np.sin(th)[None, :] * np.sin(ph)[:, None], np.cos(th)[None, :] * np.ones(seg)[:, None]], -1)
    tris = _grid_mesh(P, True, False)
    top, bot = np.asarray([0, 0, R]), np.asarray([0, 0, -R])
    for i in range(seg):
        tris += [(top, P[i, 0], P[(i + 1) % seg, 0]), (bot, P[i, -1], P[(i + 1) % seg, -1])]
    t = _outward(tris, lambda c: np.zeros_like(c)) + CENTRE
    assert len(t) == 2 * seg * (rings - 1)
    return t.astype(f32)


def torus(R=1.0, r=0.4, seg=32, sides=16):
    """2 * seg * sides = 1 024 triangles"""
    u = np.arange(seg) * 2 * np.pi / seg
    v = np.arange(sides) * 2 * np.pi / sides
    ring = R + r * np.cos(v)
    P = np.stack([ring[None, :] * np.cos(u)[:, None], ring[None, :] * np.sin(u)[:, None], (r * np.sin(v))[None, :] * np.ones(seg)[:, None]], -1)

    def core(c):   # the closest point of the torus's centre circle
        xy = c[:, :2] / np.maximum(np.linalg.norm(c[:, :2], axis=1), 1e-30)[:, None]
        return np.concatenate([R * xy, np.zeros((len(c), 1))], 1)
    t = _outward(_grid_mesh(P, True, True), core) + CENTRE
    return t.astype(f32)


def analytic(name):
    """-> (signed distance of the analytic solid, negative inside; the mesh's chord sag bound; the box to draw points from)"""
    if name == "cube":
        def sd(p):
            q = np.abs(p - CENTRE) - 0.75
            return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)
        return sd, 1e-3, 1.2
    if name == "sphere":
        return (lambda p: np.linalg.norm(p - CENTRE, axis=1) - 1.0), 0.02, 1.4
    if name == "torus":
        def sd(p):
            q = p - CENTRE
            return np.hypot(np.hypot(q[:, 0], q[:, 1]) - 1.0, q[:, 2]) - 0.4
        return sd, 0.03, 1.7
    raise KeyError(name)


MESHES = {"cube": cube, "sphere": sphere, "torus": torus}


def closed_case(name, n=1000):
    """-> (tris, points [n, 3] float32 farther from the analytic surface than the mesh's chord sag, inside [n] bool, sd [n])"""
    def make():
        tris = MESHES[name]()
        sd, sag, half = analytic(name)
        rng = np.random.default_rng({"cube": 41, "sphere": 42, "torus": 43}[name])
        pts = np.zeros((0, 3), f32)
        while len(pts) < n:
            p = (rng.uniform(-half, half, (4 * n, 3)) + CENTRE).astype(f32)
            pts = np.concatenate([pts, p[np.abs(sd(p.astype(np.float64))) > sag]])
        pts = np.ascontiguousarray(pts[:n])
        d = sd(pts.astype(np.float64))
        return tris, pts, d < 0, d
    return cached("closed_" + name, make)


def mesh_arrays(tris):
    """-> (vertices, indices, faces) for pt.Scene: every triangle its own three vertices, grey diffuse faces"""
    n = len(tris)
    faces = np.zeros((n, 6), f32)
    faces[:, :3] = 0.5
    return np.ascontiguousarray(tris, f32).reshape(-1), np.arange(3 * n, dtype=np.uint32), faces.reshape(-1)


def inside_votes(tris, points, directions):
    """[len(directions), n] bool: parity of the restatement's count for the rays (point, direction)"""
    out = []
    for d in directions:
        rays = np.concatenate([points, np.broadcast_to(np.asarray(d, f32), points.shape)], 1)
        out.append((Brute(tris, rays).count & 1).astype(bool))
    return np.stack(out)


# ---- ray sets ----------------------------------------------------------------------------------------------------------------------------------
def _norm(d):
    d = np.asarray(d, np.float64)
    return (d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-300)).astype(f32)


def nextup(x):
    return np.nextafter(np.asarray(x, f32), INF)


def nextdown(x):
    return np.nextafter(np.asarray(x, f32), -INF)


def grazing_rays(tris, pad, which, rng):
    """rays lying in a face plane of a triangle's own padded box and one ulp to either side, directed along another axis: for triangle k,
    axis a, side (lo / hi) and offset in (-1, 0, +1) ulps the origin sits on that plane, inside the box's extent on the axis the ray does not
    travel along, before the box on the axis it does; tn and tf meet at the boundary"""
    out = []
    for k in which:
        A, B, C = tris[k]
        lo, hi = own_box(A, B, C, pad)
        for a in range(3):
            for plane in (lo[a], hi[a]):
                for off in (nextdown(plane), plane, nextup(plane)):
                    b = (a + 1 + int(rng.integers(0, 2))) % 3        # the axis of travel
                    c = 3 - a - b
                    o = np.zeros(3, f32)
                    o[a] = off
                    o[b] = lo[b] - f32(0.5)
                    o[c] = f32(rng.uniform(lo[c], hi[c]))
                    d = np.zeros(3, f32)
                    d[b] = 1 if rng.integers(0, 2) else -1
                    if d[b] < 0:
                        o[b] = hi[b] + f32(0.5)
                    out.append(np.concatenate([o, d]))
    return np.asarray(out, f32)


def box_rays(cornell_arrays, n=1000, seed=77):
    """the 1 000 rays on the Cornell box: camera-like, random interior, axis-aligned, through vertices, along and through shared edges of the
    walls, and the grazing set -- in a seeded random order, ray 0 the camera axis"""
    tris = triangles(cornell_arrays[0], cornell_arrays[1])
    rng = np.random.default_rng(seed)
    pad = pad_of(tris)
    verts = tris.reshape(-1, 3)
    cam = np.asarray([0, -1, 5], f32)
    # camera-like: from the reference's eye through a pixel grid
    px = rng.uniform(-1, 1, (200, 2))
    cam_rays = np.concatenate([np.broadcast_to(cam, (200, 3)), _norm(np.stack([px[:, 0], px[:, 1] * 0.6, -np.ones(200) * 2.0], 1))], 1)
    interior = tc.make_rays(250, seed=seed + 1)
    ax = np.zeros((150, 6), f32)
    ax[:, :3] = rng.uniform(-1.2, 1.2, (150, 3)) + np.asarray([0, -1, 0])
    ax[np.arange(150), 3 + np.arange(150) % 3] = np.where(rng.integers(0, 2, 150) == 0, -1, 1)
    # through vertices: from the eye and from random interior points, aimed at a vertex exactly (to rounding)
    vi = rng.integers(0, len(verts), 120)
    o = np.where((np.arange(120) % 2 == 0)[:, None], cam, (rng.uniform(-0.9, 0.9, (120, 3)) + np.asarray([0, -1, 0])).astype(f32)).astype(f32)
    through_v = np.concatenate([o, (verts[vi] - o).astype(f32)], 1)      # (unnormalised on purpose: t = 1 at the vertex)
    # shared edges: aimed at a point of an edge, and rays that run ALONG an edge (origin on the edge's line, direction the edge)
    ti = rng.integers(0, len(tris), 120)
    e0, e1 = tris[ti, 0], tris[ti, 1]
    w = rng.uniform(0, 1, (120, 1)).astype(f32)
    w[::3] = f32(0.5)
    on_edge = (e0 + (e1 - e0) * w).astype(f32)
    o2 = (rng.uniform(-0.9, 0.9, (120, 3)) + np.asarray([0, -1, 0])).astype(f32)
    through_e = np.concatenate([o2, (on_edge - o2).astype(f32)], 1)
    along = np.concatenate([(e0 - (e1 - e0) * f32(0.5)).astype(f32), (e1 - e0).astype(f32)], 1)[:60]
    graze = grazing_rays(tris, pad, rng.permutation(len(tris))[:6], rng)   # 6 x 18 = 108
    rays = np.concatenate([cam_rays, interior, ax, through_v, through_e, along, graze]).astype(f32)
    assert len(rays) >= n - 0, len(rays)
    rays = rays[rng.permutation(len(rays))[:n]]
    rays[0] = tc.CAMERA_AXIS
    # rows SPECIAL_ROWS: all-zero directions (either sign of zero), which walk and hit nothing, and rays that do not walk -- a NaN or an
    # infinity in the origin or the direction -- spread over the first wave, the second and the tail
    for k, (slot, value) in zip(SPECIAL_ROWS, SPECIALS):
        if slot == "zero":
            rays[k, 3:] = value
        else:
            rays[k, slot] = value
    return np.ascontiguousarray(rays, f32)


SPECIAL_ROWS = (3, 17, 40, 62, 64, 66, 130, 515, 998, 999)
SPECIALS = (("zero", (0.0, 0.0, 0.0)), ("zero", (-0.0, 0.0, -0.0)), (0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (5, -np.inf),
            ("zero", (0.0, -0.0, 0.0)), (4, np.nan))


BOUND_KINDS = 13


def cycled_bounds(ts, tmin):
    """per-ray bounds cycled by i % 13 from each ray's sorted counted t's (ts [n, K], inf-padded): t_k, nextup(t_k), nextdown(t_k) for k = first,
    second and last; then +inf, tmin, -1 and NaN.  A ray without that crossing gets 1.0."""
    n = len(ts)
    k = np.isfinite(ts).sum(1)
    rows = np.arange(n)
    first = np.where(k >= 1, ts[rows, 0], f32(1))
    second = np.where(k >= 2, ts[rows, np.minimum(1, ts.shape[1] - 1)], f32(1))
    last = np.where(k >= 1, ts[rows, np.maximum(k - 1, 0)], f32(1))
    kinds = []
    for t in (first, second, last):
        kinds += [t, nextup(t), nextdown(t)]
    kinds += [np.full(n, np.inf, f32), np.full(n, tmin, f32), np.full(n, -1, f32), np.full(n, np.nan, f32)]
    return np.ascontiguousarray(np.stack(kinds, 1)[rows, rows % BOUND_KINDS].astype(f32))


def far_field_rays(n=2000, seed=5):
    """the adversarial far field: a soup of triangles about 6e-6 wide around the origin and rays that start 50 units away and pass the soup at a
    distance of several units -- 10^6 triangle sizes from every triangle, where an ulp of the origin (3.8e-6) is as large as the triangle"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.5, 0.5, (512, 1, 3))
    tris = (c + rng.uniform(-3e-6, 3e-6, (512, 3, 3))).astype(f32)
    o = _norm(rng.standard_normal((n, 3))) * f32(50)
    aim = _norm(rng.standard_normal((n, 3))) * f32(4)               # a point four units from the centre
    rays = np.concatenate([o, _norm(aim - o)], 1).astype(f32)
    return tris, np.ascontiguousarray(rays)


_cache = {}


def cached(key, make):
    """a named case, computed once per session and shared by the tests that need it"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def box_tris(cornell_arrays):
    return triangles(cornell_arrays[0], cornell_arrays[1])


TMIN_BOUNDS = f32(0.001)   # tmin of the per-ray-bound sets (and of the comparison with PT_TRACE_ANY, which wants tmin > 0)


def box_set(cornell_arrays):
    """the 1 000-ray set on the Cornell box: unbounded from tmin = 0; under the cycled per-ray bounds and under one uniform bound, tmin = 0.001"""
    def make():
        tris = box_tris(cornell_arrays)
        rays = box_rays(cornell_arrays)
        free = Brute(tris, rays)
        free_t = Brute(tris, rays, tmin=TMIN_BOUNDS, keep_t=True)
        bounds = cycled_bounds(free_t.ts, TMIN_BOUNDS)
        return {"free": free, "free_tmin": free_t, "cycled": Brute(tris, rays, bounds, tmin=TMIN_BOUNDS),
                "uniform": Brute(tris, rays, tmin=TMIN_BOUNDS, tmax=2.5)}
    return cached("box", make)


def box_points_set(cornell_arrays):
    """the d_points form: the same origins, one direction for all"""
    def make():
        rays = box_set(cornell_arrays)["free"].rays.copy()
        d = np.asarray([0.3, -0.5, 0.81], f32)
        rays[:, 3:] = d
        return d, Brute(box_tris(cornell_arrays), rays)
    return cached("box_points", make)


def box_big(cornell_arrays):
    def make():
        rays = tc.make_rays(BIG_N, seed=78)
        small = box_set(cornell_arrays)["free"].rays
        rays[1:1 + len(small) - 1] = small[1:]       # the special rays ride along
        return Brute(box_tris(cornell_arrays), rays)
    return cached("box_big", make)


def box_moved(cornell_arrays):
    """the box after a refit that ENLARGES the scene box (the short block moved and one wall vertex pulled outwards): pad changes"""
    def make():
        v = tc.move_short_box(cornell_arrays[0]).reshape(-1, 3).copy()
        k = int(np.abs(v).max(1).argmax())
        same = (v == v[k]).all(1)                    # every triangle's copy of that corner: the mesh stays connected, fan pairs stay pairs
        v[same] = v[same] * f32(1.5)
        v = v.reshape(-1)
        tris = triangles(v, cornell_arrays[1])
        return v, Brute(tris, box_set(cornell_arrays)["free"].rays)
    return cached("box_moved", make)


def soup_set():
    """tc.soup(4096, 11) with 2 000 rays, tmin = 0.001"""
    def make():
        v, i, f = tc.soup(*SOUP)
        tris = triangles(v, i)
        rays = tc.make_rays(2000, seed=79, half=1.0, centre=None)
        return (v, i, f), Brute(tris, rays, tmin=TMIN_BOUNDS)
    return cached("soup", make)
