"""What tests/test_ray_range_cpu.py and tests/test_ray_range.py share: hits placed exactly ON the ends of a ray's range (tmin, upper), one ulp to
either side of them, and per-ray bounds on the far side of the call's tmax.  The rule is include/pt_api.h's and the oracle's: a triangle counts
with tmin < t < upper, strictly, and an any-hit query's upper end is the ray's own bound and nothing else.  Every expected answer comes from the
oracle's closest-hit query in brute-force mode with the ray's bound as tmax (computed once per session and never changed)."""
import ctypes as C

import numpy as np

import trace_device_cases as tc

f32 = np.float32
MISS = tc.MISS
TMIN = f32(0.001)                 # the default tmin of every query here
INF = f32(np.inf)
KINDS = 8
KIND_NAMES = ("t", "nextup(t)", "nextdown(t)", "2 t", "tmin", "nextup(tmin)", "-1", "+inf")
CALL_TMAX = (10000.0, 1.0)        # every per-ray case runs under both: desc.tmax plays no part when d_tmax is given

_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def nextup(x):
    return np.nextafter(f32(x), INF)


def nextdown(x):
    return np.nextafter(f32(x), f32(0))


def bounds_of(hits):
    """the per-ray bound of ray i by i % 8, from the oracle's closest t_i; a ray that misses keeps the kind's constant, or 1.0 where the kind
    needs t_i"""
    n = len(hits)
    hit = hits["prim"] != MISS
    t = np.where(hit, hits["t"], f32(1.0)).astype(f32)
    kind = np.arange(n) % KINDS
    b = np.zeros(n, f32)
    b[kind == 0] = t[kind == 0]
    b[kind == 1] = np.where(hit, nextup(t), f32(1.0))[kind == 1]
    b[kind == 2] = np.where(hit, nextdown(t), f32(1.0))[kind == 2]
    b[kind == 3] = np.where(hit, (f32(2.0) * t).astype(f32), f32(1.0))[kind == 3]
    b[kind == 4] = TMIN
    b[kind == 5] = nextup(TMIN)
    b[kind == 6] = f32(-1.0)
    b[kind == 7] = INF
    return np.ascontiguousarray(b), kind, hit


def expected_occluded(osc, rays, bounds, kind, hit):
    """one byte per ray: "the oracle's closest-hit query (brute force) with the ray's bound as tmax finds a triangle"; kinds 4, 6 and 7 are decided
    directly (an empty range, an empty range, "hits at all"), not through an oracle call with an invalid range"""
    occ = np.zeros(len(rays), np.uint8)
    for i in range(len(rays)):
        if kind[i] in (4, 6):
            occ[i] = 0
        elif kind[i] == 7:
            occ[i] = hit[i]
        else:
            assert bounds[i] > TMIN, (i, bounds[i])
            h, _ = osc.trace(rays[i], tmin=float(TMIN), tmax=float(bounds[i]), mode=0)
            occ[i] = h["prim"][0] != MISS
    return occ


class RangeCase:
    """one (scene, ray set): the oracle's brute-force hits, the per-ray bounds by kind and the expected bytes"""

    def __init__(self, osc, rays):
        self.rays = np.ascontiguousarray(rays, f32)
        self.n = len(rays)
        self.hits, _ = osc.trace(self.rays, tmin=float(TMIN), mode=0)
        self.bounds, self.kind, self.hit = bounds_of(self.hits)
        self.occ = expected_occluded(osc, self.rays, self.bounds, self.kind, self.hit)

    def premises(self):
        """the conditions that make the GPU comparison mean something (tests/test_ray_range_cpu.py asserts them on the oracle alone; the GPU tests
        assert them again)"""
        assert self.hit.mean() >= 0.4, self.hit.mean()
        for k in range(KINDS):
            assert int(self.hit[self.kind == k].sum()) >= 50, (k, int(self.hit[self.kind == k].sum()))
        k = self.kind
        assert (self.occ[k == 0] == 0).all()                      # a hit ON the bound is outside the range
        assert (self.occ[(k == 1) & self.hit] == 1).all()         # one ulp beyond it: inside
        assert (self.occ[k == 2] == 0).all()                      # one ulp before it: outside
        for both in (3, 7):
            assert set(np.unique(self.occ[k == both])) == {0, 1}, both
        assert (self.occ[k == 5] == 0).all() and (self.occ[~self.hit] == 0).all()
        # the second run's edge: bounds beyond a call tmax of 1.0 whose hit lies beyond it too
        far = self.hit & (self.hits["t"] > f32(CALL_TMAX[1]))
        assert int((far & np.isin(k, (1, 3, 7))).sum()) >= 20, int((far & np.isin(k, (1, 3, 7))).sum())


# ---- the scenes, named by how they are walked -------------------------------------------------------------------------------------------------
def box_case(orc, cornell_arrays):
    """the Cornell box (the compact LDS kernels, both leaf forms; the HBM kernel by name)"""
    return once("box", lambda: RangeCase(orc.Scene(*cornell_arrays), tc.make_rays()))


def soup_arrays():
    return once("soup_arrays", lambda: tc.soup(4096, 11))


# (tests/test_trace_device.py draws the origins from half = 1.3: 41.8 % of those rays hit, but only 47 of the 125 under kind 1 -- fewer than the 50
# every kind needs; from half = 0.8, 76 % hit and every kind has 91 or more)
SOUP_RAYS = dict(seed=2024, half=0.8, centre=None)


def soup_case(orc):
    """a 4 096-triangle soup (walked out of L2: the BVH4 kernel over 64-B records, and the 8-wide tree)"""
    return once("soup", lambda: RangeCase(orc.Scene(*soup_arrays()), tc.make_rays(**SOUP_RAYS)))


INST_RAYS = dict(seed=7, x_seed=8)


def inst_case(orc, cornell_arrays):
    """the box under trace_device_cases.INSTANCES (both two-level kernels)"""
    def make():
        osc = orc.Scene(*cornell_arrays)
        osc.set_instances(tc.INSTANCES)
        return RangeCase(osc, tc.make_rays(**INST_RAYS))
    return once("inst", make)


# ---- the orthographic bundle: many rays that share their t bit for bit ------------------------------------------------------------------------
BUNDLE_GROUPS = ((f32(4.04), 553), (f32(4.0400004), 74), (f32(4.0399995), 60))   # (t, rays that hit at exactly that t) on the Cornell box


def bundle_rays():
    x, y = np.linspace(-0.95, 0.95, 32).astype(f32), np.linspace(-1.95, -0.05, 32).astype(f32)
    r = np.zeros((32, 32, 6), f32)
    r[..., 0], r[..., 1], r[..., 2], r[..., 5] = x[None, :], y[:, None], f32(3.0), f32(-1.0)
    return np.ascontiguousarray(r.reshape(-1, 6))


class Bundle:
    """the oracle's closest hits (brute force) of the bundle at the default range and, per shared t, at the four ends: tmax = t, tmax = nextup(t),
    tmin = t, tmin = nextdown(t)"""

    def __init__(self, osc, faces):
        self.rays = bundle_rays()
        self.n = len(self.rays)
        self.hits, _ = osc.trace(self.rays, tmin=float(TMIN), mode=0)
        self.groups = [(t, np.flatnonzero(self.hits["t"] == t)) for t, _ in BUNDLE_GROUPS]
        self.ends = {}      # (group, name) -> (tmin, tmax, hits, surface planes)
        for g, (t, _) in enumerate(BUNDLE_GROUPS):
            for name, lo, hi in (("tmax=t", TMIN, t), ("tmax=up", TMIN, nextup(t)), ("tmin=t", t, f32(10000.0)), ("tmin=down", nextdown(t), f32(10000.0))):
                h, _ = osc.trace(self.rays, tmin=float(lo), tmax=float(hi), mode=0)
                self.ends[g, name] = (float(lo), float(hi), h, tc.surface_oracle(osc, faces, h))

        self.uniform = {}   # (group, name) -> (the bound of all rays, the oracle's "a closest hit exists below it" per ray)
        for g, (t, _) in enumerate(BUNDLE_GROUPS):
            for name, b in (("t", t), ("up", nextup(t)), ("down", nextdown(t))):
                h, _ = osc.trace(self.rays, tmin=float(TMIN), tmax=float(b), mode=0)
                self.uniform[g, name] = (float(b), (h["prim"] != MISS).astype(np.uint8))


def bundle(orc, cornell_arrays):
    return once("bundle", lambda: Bundle(orc.Scene(*cornell_arrays), cornell_arrays[2]))


# ---- six triangles that tell "the shadow ray ends at 0.999 dist" from "... at min(0.999 dist, tmax)" ------------------------------------------
SIX_QUADS = ((0.0, 3.0, (0.8, 0.8, 0.8), (0.0, 0.0, 0.0)),       # wall:      z, half side, Kd, Ke
             (3.0, 1.0, (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)),       # occluder
             (4.0, 0.5, (0.0, 0.0, 0.0), (10.0, 10.0, 10.0)))    # emitter
SIX_RENDER = dict(width=24, height=16, spp_per_frame=4, max_depth=3, cam_origin=(0.0, 0.0, 1.0), cam_target=(0.0, 0.0, 0.0))
SIX_TMAX = 2.0            # between the wall and the occluder: every wall point's light sample has the occluder BEYOND tmax


def six_arrays():
    v, idx, faces = [], [], []
    for q, (z, h, kd, ke) in enumerate(SIX_QUADS):
        v += [(-h, h, z), (h, h, z), (h, -h, z), (-h, -h, z)]
        idx += [4 * q + 0, 4 * q + 1, 4 * q + 2, 4 * q + 0, 4 * q + 2, 4 * q + 3]
        faces += [kd + ke, kd + ke]
    return np.asarray(v, f32).reshape(-1), np.asarray(idx, np.uint32), np.asarray(faces, f32).reshape(-1)


def six_lights(v, idx, faces):
    """oracle/pt_oracle.c build_lights for a single-level scene -> ([n, 16] float32: v0 v1 v2 normal Ke cdf, total area)"""
    p = np.asarray(v, f32).reshape(-1, 3)[np.asarray(idx).reshape(-1, 3)]
    fc = np.asarray(faces, f32).reshape(-1, 6)
    rows, run = [], f32(0.0)
    for t in range(len(p)):
        if not (fc[t, 3:] != 0).any():
            continue
        e1, e2 = (p[t, 1] - p[t, 0]).astype(f32), (p[t, 2] - p[t, 0]).astype(f32)
        cx = f32(f32(e1[1] * e2[2]) - f32(e1[2] * e2[1]))
        cy = f32(f32(e1[2] * e2[0]) - f32(e1[0] * e2[2]))
        cz = f32(f32(e1[0] * e2[1]) - f32(e1[1] * e2[0]))
        ln = f32(np.sqrt(f32(f32(f32(cx * cx) + f32(cy * cy)) + f32(cz * cz))))
        run = f32(run + f32(f32(0.5) * ln))
        rows.append(np.concatenate([p[t].reshape(-1), [-(cx / ln), -(cy / ln), -(cz / ln)], fc[t, 3:], [run]]).astype(f32))
    return np.asarray(rows, f32), run


def _dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def nee_frame(orc, osc, lights, area, params, cut, log=None):
    """oracle/pt_oracle.c render_pixel with nee = 1, statement by statement in binary32, with the shadow ray's upper end left to `cut(0.999 dist,
    tmax)`: `lambda b, tmax: b` is the oracle's rule, `min` the rule that also cuts at tmax.  -> frame colour [h, w, 3] float32.
    log (a list): one record per light sample of sample 0 -- (px, py, wall point, wi, dist)"""
    lib = orc.lib()
    w, h, spp, depth_n = params.width, params.height, params.spp_per_frame, params.max_depth
    tmin, tmax = f32(params.tmin), f32(params.tmax)
    env = np.asarray(list(params.env), f32)
    img = np.zeros((h, w, 3), f32)
    for py in range(h):
        for px in range(w):
            color = np.zeros(3, f32)
            for s in range(spp):
                org, d, seed = orc.primary_ray(params, px, py, orc.seed(px, py, s, params.frame, spp))
                st = C.c_uint32(seed)
                rnd = lambda: f32(lib.orc_rand(C.byref(st)))
                weight = np.ones(3, f32)
                for depth in range(depth_n):
                    hh, _ = osc.trace(np.concatenate([org, d]), tmin=float(tmin), tmax=float(tmax))
                    if hh["prim"][0] == MISS:
                        color = (color + (weight * env).astype(f32)).astype(f32)
                        break
                    pos, n, brdf, emi = osc.shade_hit(hh[0])
                    if depth == 0:
                        color = (color + (weight * emi).astype(f32)).astype(f32)
                    if len(lights) and depth + 1 < depth_n:
                        rl, ru, rv = rnd(), rnd(), rnd()
                        pick = f32(rl * area)
                        li, hi_ = 0, len(lights) - 1
                        while li < hi_:
                            mid = (li + hi_) >> 1
                            if lights[mid, 15] > pick:
                                hi_ = mid
                            else:
                                li = mid + 1
                        L = lights[li]
                        su = f32(np.sqrt(ru))
                        b0, b1, b2 = f32(f32(1.0) - su), f32(su * f32(f32(1.0) - rv)), f32(su * rv)
                        dd = np.asarray([f32(f32(f32(f32(L[k] * b0) + f32(L[3 + k] * b1)) + f32(L[6 + k] * b2)) - pos[k]) for k in range(3)], f32)
                        d2 = _dot(dd, dd)
                        if d2 > 0:
                            dist = f32(np.sqrt(d2))
                            wi = (dd / dist).astype(f32)
                            cs, cl = _dot(wi, n), f32(abs(_dot(wi, L[9:12])))
                            if cs > 0 and cl > 0:
                                fgeo = f32(f32(f32(cs * cl) / d2) * area)
                                upper = f32(cut(f32(dist * f32(0.999)), tmax))
                                sh, _ = osc.trace(np.concatenate([pos, wi]), tmin=float(tmin), tmax=float(upper))
                                if log is not None and s == 0 and depth == 0:
                                    log.append((px, py, pos.copy(), wi.copy(), dist))
                                if sh["prim"][0] == MISS:
                                    color = (color + (((weight * brdf).astype(f32) * L[12:15]).astype(f32) * fgeo).astype(f32)).astype(f32)
                    org = pos
                    r1 = rnd()
                    r2 = rnd()
                    d = orc.sample_direction(r1, r2, n, int(params.libm_sincos))
                    dt = _dot(d, n)
                    weight = (weight * ((brdf * dt).astype(f32) / rcs_inv_2pi).astype(f32)).astype(f32)
            img[py, px] = (color / f32(spp)).astype(f32)
    return img


rcs_inv_2pi = f32(0.15915493667125702)


def six_oracle(orc):
    """-> (orc.Scene of the six triangles, its arrays)"""
    return once("six", lambda: (orc.Scene(*six_arrays()), six_arrays()))


def six_film(orc, frames, tmax, nee=1, **over):
    """-> (film float32, rays) of the oracle's render_frame over `frames` frames of SIX_RENDER (over: e.g. spp_per_frame=1)"""
    def make():
        osc, _ = six_oracle(orc)
        film, rays = None, 0
        for k in range(frames):
            img, r, _, _ = osc.render_frame(orc.default_params(frame=k, nee=nee, tmax=tmax, **dict(SIX_RENDER, **over)))
            if film is None:
                film = np.zeros_like(img)
            orc.accumulate_f32(film, img, k)
            rays += r
        return film, rays
    return once(("six_film", frames, tmax, nee, tuple(sorted(over.items()))), make)


SIX_RAYS = dict(seed=2024, half=0.45, centre=(0.0, 0.0, 3.5))   # origins between the occluder and the emitter


def six_case(orc):
    """the six-triangle scene (a tree of two levels of nodes at most: the root is nearly the whole walk)"""
    return once("six_case", lambda: RangeCase(six_oracle(orc)[0], tc.make_rays(**SIX_RAYS)))


def six_camera(orc):
    """the rays of SIX_RENDER's camera at 1 spp, row by row, and the seeds as primary_ray leaves them (radiance_cases.camera_rays, this camera)"""
    def make():
        w, h = SIX_RENDER["width"], SIX_RENDER["height"]
        p = orc.default_params(frame=0, **dict(SIX_RENDER, spp_per_frame=1))
        rays, seeds = np.zeros((w * h, 6), f32), np.zeros((w * h, 1), np.uint32)
        for py in range(h):
            for px in range(w):
                o, d, s = orc.primary_ray(p, px, py, orc.seed(px, py, 0, 0, 1))
                rays[py * w + px, :3], rays[py * w + px, 3:], seeds[py * w + px, 0] = o, d, s
        return rays, seeds
    return once("six_camera", make)
