"""What tests/test_radiance_device_cpu.py and tests/test_radiance_device.py share: the recipes (rays, seeds, scenes), the oracle's radiance for them
(computed once per session and never changed), the header's seed rule, and a Python restatement of the path loop (oracle/pt_oracle.c
render_pixel, plain estimator) built from orc.Scene.trace, shade_hit, sample_direction and orc_rand -- the reference for rays that come from no
camera."""
import ctypes as C

import numpy as np

import trace_device_cases as tc

f32 = np.float32
MISS = tc.MISS
ENV = (f32(0.7), f32(0.6), f32(0.5))
INV_2PI = f32(0.15915493667125702)
CAM_W, CAM_H, DEPTH = 24, 16, 4            # the camera recipes
FREE_N, FREE_SPP = 257, 3                  # the free-ray recipe
PREFIXES = (1, 63, 64, 65, 257)

_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def hashed_seed(index, s, spp, frame):
    """include/pt_api.h: a + b (mod 2^32), (a, b) = pcg2d((uint32)index, m), m = s + (uint32)((int32)spp * frame) + 1"""
    from oracle import pt_oracle as orc
    m = (s + spp * frame + 1) & 0xFFFFFFFF
    a, b = orc.pcg2d(index & 0xFFFFFFFF, m)
    return (a + b) & 0xFFFFFFFF


def hashed_seeds(n, spp, frame=0, index_base=0):
    return np.asarray([[hashed_seed(i + index_base, s, spp, frame) for s in range(spp)] for i in range(n)], np.uint32)


def camera_rays(orc, width, height, frame=0):
    """the default camera's ray of every pixel, row by row, with spp_per_frame = 1: (rays [n, 6], the seed as primary_ray leaves it [n, 1])"""
    p = orc.default_params(width=width, height=height, spp_per_frame=1, frame=frame)
    rays, seeds = np.zeros((width * height, 6), f32), np.zeros((width * height, 1), np.uint32)
    for py in range(height):
        for px in range(width):
            o, d, s = orc.primary_ray(p, px, py, orc.seed(px, py, 0, frame, 1))
            rays[py * width + px, :3], rays[py * width + px, 3:], seeds[py * width + px, 0] = o, d, s
    return rays, seeds


class CameraCase:
    """one scene seen through the default camera at 1 spp: the rays and advanced seeds of every pixel, and the oracle's frame -- plain and with
    next-event estimation -- with its ray counts and first hits"""

    def __init__(self, orc, osc, width=CAM_W, height=CAM_H, depth=DEPTH):
        self.n = width * height
        self.rays, self.seeds = camera_rays(orc, width, height)
        self.depth = depth
        self.want, self.n_rays = {}, {}
        for nee in (0, 1):
            p = orc.default_params(width=width, height=height, spp_per_frame=1, max_depth=depth, frame=0, nee=nee)
            img, rays, _, fh = osc.render_frame(p, want_first_hits=True)
            self.want[nee], self.n_rays[nee] = np.ascontiguousarray(img.reshape(-1, 3)), rays
            self.first = fh
        self.hit = self.first["prim"] != MISS
        self.nee_differs = float((self.want[0] != self.want[1]).any(1).mean())


def path_radiance(orc, osc, ray, seed, depth, tmin=0.001, tmax=10000.0, env=ENV):
    """oracle/pt_oracle.c render_pixel:744-797 for one sample, plain estimator, from `ray` with the RNG at `seed` -> (c_s [3] float32, rays traced)"""
    lib = orc.lib()
    st = C.c_uint32(int(seed))
    org, d = np.array(ray[:3], f32), np.array(ray[3:], f32)
    color, weight = np.zeros(3, f32), np.ones(3, f32)
    traced = 0
    for _ in range(depth):
        h, _c = osc.trace(np.concatenate([org, d]), tmin=tmin, tmax=tmax)
        traced += 1
        if h["prim"][0] == MISS:
            for k in range(3):
                color[k] = color[k] + weight[k] * env[k]
            break
        pos, n, brdf, emi = osc.shade_hit(h[0])
        for k in range(3):
            color[k] = color[k] + weight[k] * emi[k]
        org = pos
        r1 = f32(lib.orc_rand(C.byref(st)))
        r2 = f32(lib.orc_rand(C.byref(st)))
        d = orc.sample_direction(r1, r2, n)
        dt = f32(f32(d[0] * n[0] + d[1] * n[1]) + d[2] * n[2])
        for k in range(3):
            weight[k] = weight[k] * f32(f32(brdf[k] * dt) / INV_2PI)
    return color, traced


def ordered_mean(c):
    """c [n, spp, 3] float32 -> (mean, second moment) by the header's reduce: C = +0; C = C + c_s ascending; / (float)spp"""
    n, spp, _ = c.shape
    a, q = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    for s in range(spp):
        a = (a + c[:, s]).astype(f32)
        q = (q + (c[:, s] * c[:, s]).astype(f32)).astype(f32)
    return (a / f32(spp)).astype(f32), (q / f32(spp)).astype(f32)


def blend(old, value, frame):
    """the film's blend: (value + old * (float)frame) / (float)(frame + 1); old is +0 at frame 0"""
    o = np.zeros_like(value) if frame == 0 else old
    return ((value + (o * f32(frame)).astype(f32)).astype(f32) / f32(frame + 1)).astype(f32)


class FreeCase:
    """the first 257 rows of trace_device_cases.make_rays() at 3 samples, depth 4, hashed seeds: every sample's c_s by the Python path loop"""

    def __init__(self, orc, osc, n=FREE_N, spp=FREE_SPP, depth=DEPTH, frame=0):
        self.n, self.spp, self.depth = n, spp, depth
        self.rays = np.ascontiguousarray(tc.make_rays()[:n])
        self.seeds = hashed_seeds(n, spp, frame)
        self.c = np.zeros((n, spp, 3), f32)
        self.traced = np.zeros((n, spp), np.uint64)
        for i in range(n):
            for s in range(spp):
                self.c[i, s], self.traced[i, s] = path_radiance(orc, osc, self.rays[i], self.seeds[i, s], depth)
        self.mean, self.m2 = ordered_mean(self.c)


def box_camera(orc, cornell_arrays):
    return once("box_camera", lambda: CameraCase(orc, orc.Scene(*cornell_arrays)))


def inst_camera(orc, cornell_arrays):
    def make():
        osc = orc.Scene(*cornell_arrays)
        osc.set_instances(tc.INSTANCES)
        return CameraCase(orc, osc)
    return once("inst_camera", make)


def soup_arrays():
    return once("soup_arrays", lambda: tc.soup(4096, 11))


def soup_camera(orc):
    return once("soup_camera", lambda: CameraCase(orc, orc.Scene(*soup_arrays()), 16, 16))


def box_free(orc, cornell_arrays):
    return once("box_free", lambda: FreeCase(orc, orc.Scene(*cornell_arrays)))
