"""What tests/test_trace_fused_cpu.py and tests/test_trace_fused.py share beside tests/trace_device_cases.py: the big ray set of the persistent-loop
test and the oracle's answers for it (computed once per session and never changed), and the refusal table of the queue form restated."""
import numpy as np

import trace_device_cases as tc

f32 = np.float32
BIG_N = 200_001   # rays of the persistent-loop test: with one block per CU every wave draws from at least three strides, and the last is ragged


def box_answers(orc, cornell_arrays):
    return tc.answers("box", lambda: tc.Answers(orc.Scene(*cornell_arrays), cornell_arrays[2], tc.make_rays()))


# The any-hit queries of the big set run with this tmin.  Under the default tmin of 0.001 the smallest cycled bound, 1e-4, lies BELOW tmin and can
# occlude nothing, so one of the four bounds would never see both answers; with tmin = 1e-5 a handful of the 50 001 rays that carry it start
# within 1e-4 of a surface.  (tmin > 0: still the single-kernel form's class.)
BIG_ANY_TMIN = 1e-5


class BigAnswers(tc.Answers):
    """tc.Answers of the big set; occ_cycled is the oracle's answer at tmin = BIG_ANY_TMIN (everything else at the default tmin)"""

    def __init__(self, osc, faces, rays):
        super().__init__(osc, faces, rays)
        self.occ_cycled = tc.occluded_oracle(osc, rays, self.bounds, tmin=BIG_ANY_TMIN)


def big_answers(orc, cornell_arrays):
    return tc.answers("box_big", lambda: BigAnswers(orc.Scene(*cornell_arrays), cornell_arrays[2], tc.make_rays(BIG_N)))


def big_shares(ans):
    """-> (hit share, occluded share under the cycled bounds, [(occluded share, count) per bound of tc.BOUNDS])"""
    per = []
    for k in range(4):
        o = ans.occ_cycled[k::4]
        per.append((float(o.mean()), len(o)))
    return ans.hit_share(len(ans.rays)), ans.occ_share(len(ans.rays)), per


PLANES = ("position", "normal", "albedo", "emission")


class Query:
    """The device buffers of one ray set (pt_device_alloc: no torch needed) and pt_trace_device calls over its prefixes.  Every output is filled
    with a canary (0xEE bytes) before every call and read back whole afterwards, so what a call leaves alone shows: rows beyond n, and outputs
    that were not named.  ray_offset: bytes between the rays' allocation and their first row (a multiple of 4)."""

    def __init__(self, pt, ctx, rays, bounds, ray_offset=0):
        self.pt, self.n = pt, len(rays)
        self.rays_buf = pt.DeviceBuffer(ctx, rays.nbytes + ray_offset)
        self.rays_buf.write(np.concatenate([np.zeros(ray_offset, np.uint8), np.ascontiguousarray(rays).view(np.uint8).reshape(-1)]))
        self.rays_ptr = self.rays_buf.ptr + ray_offset
        self.bounds = pt.DeviceBuffer(ctx, 4 * self.n)
        self.bounds.write(bounds)
        self.hits = pt.DeviceBuffer(ctx, 20 * self.n)
        self.occ = pt.DeviceBuffer(ctx, self.n)
        self.planes = [pt.DeviceBuffer(ctx, 12 * self.n) for _ in PLANES]
        self.ms = 0.0

    def outputs(self):
        return [self.hits, self.occ] + self.planes

    def canary(self):
        for b in self.outputs():
            b.write(np.full(b.nbytes, 0xEE, np.uint8))

    def untouched(self):
        return all((b.read(np.uint8, b.nbytes) == 0xEE).all() for b in self.outputs())

    def closest(self, scene, n, hits=True, planes=(0, 1, 2, 3), read=True, **kw):
        """-> (hit records or None, {plane index: [n, 3]}) of rays [0, n); asserts the canaries beyond row n and in every output not named"""
        self.canary()
        ptrs = {PLANES[k] + "_ptr": self.planes[k].ptr for k in planes}
        self.ms = scene.trace_device(n, self.rays_ptr, hits_ptr=self.hits.ptr if hits else None, mode=self.pt.TRACE_CLOSEST, **ptrs, **kw)
        return self.read_closest(n, hits, planes) if read else None

    def read_closest(self, n, hits=True, planes=(0, 1, 2, 3)):
        raw = self.hits.read(np.uint8, self.hits.nbytes)
        assert (raw[20 * n if hits else 0:] == 0xEE).all(), "d_hits beyond row n / not named"
        h = raw[:20 * n].view(self.pt.HIT_DTYPE) if hits else None
        s = {}
        for k, b in enumerate(self.planes):
            raw = b.read(np.uint8, b.nbytes)
            assert (raw[12 * n if k in planes else 0:] == 0xEE).all(), (PLANES[k], "beyond row n / not named")
            if k in planes:
                s[k] = raw[:12 * n].view(f32).reshape(n, 3)
        assert (self.occ.read(np.uint8, self.n) == 0xEE).all()
        return h, s

    def any(self, scene, n, per_ray=True, **kw):
        self.canary()
        self.ms = scene.trace_device(n, self.rays_ptr, tmax_ptr=self.bounds.ptr if per_ray else None, occluded_ptr=self.occ.ptr, mode=self.pt.TRACE_ANY, **kw)
        o = self.occ.read(np.uint8, self.n)
        assert (o[n:] == 0xEE).all()
        assert all((b.read(np.uint8, b.nbytes) == 0xEE).all() for b in [self.hits] + self.planes)
        return o[:n]

    def close(self):
        for b in [self.rays_buf, self.bounds] + self.outputs():
            b.close()


def check_closest(ans, n, got, what):
    """the call's records and planes against the oracle's, byte for byte"""
    h, s = got
    if h is not None:
        assert h.tobytes() == ans.hits[:n].tobytes(), (what, n, np.flatnonzero(h != ans.hits[:n])[:4])
    for k, a in s.items():
        assert a.tobytes() == ans.surface[k][:n].tobytes(), (what, n, PLANES[k], np.flatnonzero((a != ans.surface[k][:n]).any(1))[:4])


def same_closest(a, b):
    """two calls' outputs, byte for byte"""
    return (a[0] is None) == (b[0] is None) and (a[0] is None or a[0].tobytes() == b[0].tobytes()) and a[1].keys() == b[1].keys() and \
        all(a[1][k].tobytes() == b[1][k].tobytes() for k in a[1])
