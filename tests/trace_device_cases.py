"""What tests/test_trace_device_cpu.py and tests/test_trace_device.py share: the ray recipes, the scenes beside the Cornell box, the oracle's
answers to compare against (computed once per session and never changed), and the tables of trace_device_kernel.h built in numpy."""
import numpy as np

f32 = np.float32
MISS = 0xFFFFFFFF
PREFIXES = (1, 63, 64, 65, 257, 1000)
BOUNDS = np.asarray([1e-4, 0.5, 2.0, 10000.0], f32)        # per-ray bounds cycle through these by i % 4
INSTANCES = np.asarray([[1, 0, 0, -2.5, 0, 1, 0, 0, 0, 0, 1, 0],
                        [.5, 0, 0, 0, 0, .5, 0, -1, 0, 0, .5, 2],
                        [0, 0, 1, 2.5, 0, 1, 0, 0, -1, 0, 0, 0]], f32)
CAMERA_AXIS = np.asarray([0, -1, 5, 0, 0, -1], f32)         # ray 0 of every set on the box


def make_rays(n=1000, seed=2024, half=1.25, centre=(0.0, -1.0, 0.0), x_seed=None):
    """origins uniform in [-half, half]^3 + centre, directions normal draws normalised, all float32; ray 0 the camera axis (centre given);
    x_seed: origin x redrawn uniform in [-4, 4] from that seed (the instanced set)"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-half, half, (n, 3)).astype(f32) + np.asarray(centre if centre is not None else (0, 0, 0), f32)
    d = rng.standard_normal((n, 3)).astype(f32)
    d = (d / np.sqrt((d * d).sum(1, dtype=f32))[:, None]).astype(f32)
    if x_seed is not None:
        o[:, 0] = np.random.default_rng(x_seed).uniform(-4, 4, n).astype(f32)
    r = np.ascontiguousarray(np.concatenate([o, d], 1), f32)
    if centre is not None:
        r[0] = CAMERA_AXIS
    return r


def cycled_bounds(n):
    return np.ascontiguousarray(BOUNDS[np.arange(n) % 4])


def soup(n, seed, spread=0.1):
    """tests/test_gpu_parity.py::_soup"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)).astype(f32)
    v = (c + rng.uniform(-spread, spread, (n, 3, 3)).astype(f32)).astype(f32)
    faces = rng.uniform(0, 1, (n, 6)).astype(f32)
    faces[:, 3:] *= (rng.uniform(0, 1, (n, 1)) < 0.1)
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), faces.reshape(-1).astype(f32)


def move_short_box(v):
    """The Cornell box with its short block moved: every triangle with a vertex on the block's top (y = -0.6) shifted whole, so the quads' fan
    pairs stay pairs and a refit keeps its tree."""
    p = np.array(v, f32).reshape(-1, 3, 3).copy()
    block = (np.abs(p[:, :, 1] + f32(0.6)) < 1e-4).any(1)
    assert block.sum() == 12, block.sum()   # the top and the sides (the loader's fans: two triangles per quad)
    p[block] += f32([0.1, 0.0, 0.05])
    return p.reshape(-1).astype(f32)


def occluded_oracle(osc, rays, bounds, tmin=0.001):
    """the oracle's "closest hit exists" with each ray's own bound as tmax: one oracle call per distinct bound, each ray keeping its own"""
    occ = np.zeros(len(rays), np.uint8)
    for b in np.unique(bounds):
        h, _ = osc.trace(rays, tmin=tmin, tmax=float(b), mode=0)
        m = bounds == b
        occ[m] = (h["prim"][m] != MISS)
    return occ


def surface_oracle(osc, faces, hits):
    """-> position, normal, albedo, emission [n, 3] float32 by orc.Scene.shade_hit ray by ray (position, normal) and `faces` (Kd, Ke);
    +0.0 for a miss"""
    n = len(hits)
    out = [np.zeros((n, 3), f32) for _ in range(4)]
    fc = np.asarray(faces, f32).reshape(-1, 6)
    for k in range(n):
        if hits["prim"][k] == MISS:
            continue
        pos, nrm, _, _ = osc.shade_hit(hits[k])
        out[0][k], out[1][k] = pos, nrm
        out[2][k], out[3][k] = fc[hits["prim"][k], :3], fc[hits["prim"][k], 3:]
    return out


class Answers:
    """the oracle's answers for one (scene, ray set): hits at the default bounds, the surface record, occlusion under the cycled and a uniform bound"""

    def __init__(self, osc, faces, rays, uniform_bound=0.5):
        self.rays = rays
        self.hits, _ = osc.trace(rays, mode=0)
        self.surface = surface_oracle(osc, faces, self.hits)
        self.bounds = cycled_bounds(len(rays))
        self.occ_cycled = occluded_oracle(osc, rays, self.bounds)
        self.uniform_bound = uniform_bound
        self.occ_uniform = occluded_oracle(osc, rays, np.full(len(rays), uniform_bound, f32))

    def hit_share(self, n):
        return float((self.hits["prim"][:n] != MISS).mean())

    def occ_share(self, n):
        return float(self.occ_cycled[:n].mean())


_cache = {}


def answers(key, make):
    """the Answers of a named case, computed once per session (make() -> Answers) and shared by the tests that need them"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- the tables of trace_device_kernel.h in numpy, leaf order = primitive order -----------------------------------------------------------
def normals_f32(v, idx):
    """-normalize(cross(B - A, C - A)) in binary32, every operation rounded on its own (orc_shade_hit's statements)"""
    p = np.asarray(v, f32).reshape(-1, 3)[np.asarray(idx).reshape(-1, 3)]
    e1, e2 = (p[:, 1] - p[:, 0]).astype(f32), (p[:, 2] - p[:, 0]).astype(f32)
    cx = (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]).astype(f32)
    cy = (e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]).astype(f32)
    cz = (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]).astype(f32)
    ln = np.sqrt(((cx * cx + cy * cy).astype(f32) + cz * cz).astype(f32)).astype(f32)
    return np.stack([-(cx / ln), -(cy / ln), -(cz / ln)], 1).astype(f32)


def invert_3x4(m):
    """oracle/pt_oracle.c invert_3x4: the inverse in double, rounded to float at the end"""
    a = np.asarray(m, np.float64).reshape(3, 4)
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = a[0, 0], a[0, 1], a[0, 2], a[1, 0], a[1, 1], a[1, 2], a[2, 0], a[2, 1], a[2, 2]
    c00, c01, c02 = a11 * a22 - a12 * a21, a12 * a20 - a10 * a22, a10 * a21 - a11 * a20
    det = (a00 * c00 + a01 * c01) + a02 * c02
    i = np.array([[c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det],
                  [c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det],
                  [c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det]])
    t = a[:, 3]
    col = -((i[:, 0] * t[0] + i[:, 1] * t[1]) + i[:, 2] * t[2])
    return np.concatenate([i, col[:, None]], 1).astype(f32)


def kernel_tables(v, idx, faces, xforms=None, frames=False):
    """-> dict of the arrays TdScene points to, for a tree whose leaf order is the primitive order and a TLAS whose leaf order is the
    instance order: tri4 [3n, 4], rec64 [4n, 4], faces, inst6 [6 n_inst, 4], inst_frame [2 n_inst n, 4] (frames) -- float32, prim ids as bits"""
    p = np.asarray(v, f32).reshape(-1, 3)[np.asarray(idx).reshape(-1, 3)]
    n = len(p)
    nrm = normals_f32(v, idx)
    tri4 = np.zeros((n, 3, 4), f32)
    tri4[:, :, :3] = p
    tri4[:, 0, 3] = np.arange(n, dtype=np.uint32).view(f32)
    rec64 = np.zeros((n, 4, 4), f32)
    rec64[:, :3, :3] = p
    rec64[:, :3, 3] = nrm
    t = {"tri4": tri4.reshape(-1, 4), "rec64": rec64.reshape(-1, 4), "faces": np.asarray(faces, f32).reshape(-1),
         "inst6": np.zeros((0, 4), f32), "inst_frame": np.zeros((0, 4), f32)}
    if xforms is not None:
        x = np.asarray(xforms, f32).reshape(-1, 3, 4)
        inv = np.stack([invert_3x4(m) for m in x])
        t["inst6"] = np.concatenate([x, inv], 1).reshape(-1, 4).astype(f32)
        if frames:
            fr = np.zeros((len(x), n, 2, 4), f32)
            for k in range(len(x)):
                w = [((inv[k, 0, c] * nrm[:, 0] + inv[k, 1, c] * nrm[:, 1]).astype(f32) + inv[k, 2, c] * nrm[:, 2]).astype(f32) for c in range(3)]
                ln = np.sqrt(((w[0] * w[0] + w[1] * w[1]).astype(f32) + w[2] * w[2]).astype(f32)).astype(f32)
                fr[k, :, 0, :3] = np.stack([w[0] / ln, w[1] / ln, w[2] / ln], 1)
            t["inst_frame"] = fr.reshape(-1, 4)
    return t
