"""pt_trace_device on the GPU (include/pt_api.h): rays in device memory, answers in device memory.  Every case is held
byte for byte against the CPU oracle (closest hits in brute-force mode, orc.Scene.shade_hit for the surface record, "a closest hit exists" for
occlusion) and, for the hit records, against pt_trace of the same rays.  The ray recipes and the oracle's answers are tests/trace_device_cases.py
(computed once per session); tests/test_trace_device_cpu.py checks the recipes against the oracle alone, and every test here asserts again that
the oracle's answer has both hits and misses."""
import ctypes as C

import numpy as np
import pytest

import trace_device_cases as tc

f32 = np.float32
MISS = tc.MISS
PLANES = ("position", "normal", "albedo", "emission")
pytestmark = pytest.mark.gpu


class Query:
    """the device buffers of one ray set (pt_device_alloc: no torch needed) and the calls over its prefixes; outputs are filled with a canary
    (0xEE bytes) before every call, so what a call leaves alone shows"""

    def __init__(self, pt, ctx, rays, bounds=None):
        self.pt, self.ctx, self.n = pt, ctx, len(rays)
        self.rays = pt.DeviceBuffer(ctx, rays.nbytes)
        self.rays.write(rays)
        self.bounds = pt.DeviceBuffer(ctx, 4 * self.n)
        if bounds is not None:
            self.bounds.write(bounds)
        self.hits = pt.DeviceBuffer(ctx, 20 * self.n)
        self.occ = pt.DeviceBuffer(ctx, self.n)
        self.planes = [pt.DeviceBuffer(ctx, 12 * self.n) for _ in PLANES]
        self.ms = 0.0

    def canary(self):
        for b in [self.hits, self.occ] + self.planes:
            b.write(np.full(b.nbytes, 0xEE, np.uint8))

    def untouched(self):
        return all((b.read(np.uint8, b.nbytes) == 0xEE).all() for b in [self.hits, self.occ] + self.planes)

    def closest(self, scene, n, hits=True, surface=True, sync=True, **kw):
        """-> (hit records or None, [position, normal, albedo, emission] or None) of rays [0, n)"""
        self.canary()
        ptrs = {name + "_ptr": b.ptr for name, b in zip(PLANES, self.planes)} if surface else {}
        self.ms = scene.trace_device(n, self.rays.ptr, hits_ptr=self.hits.ptr if hits else None, mode=self.pt.TRACE_CLOSEST, **ptrs, **kw)
        if not sync:
            return None
        return self.read_closest(n, hits, surface)

    def read_closest(self, n, hits=True, surface=True):
        h = self.hits.read(self.pt.HIT_DTYPE, n) if hits else None
        if not hits:
            assert (self.hits.read(np.uint8, self.hits.nbytes) == 0xEE).all()
        # nothing beyond ray n is written
        assert (self.hits.read(np.uint8, self.hits.nbytes)[20 * n:] == 0xEE).all()
        s = [b.read(f32, (n, 3)) for b in self.planes] if surface else None
        assert all((b.read(np.uint8, b.nbytes)[12 * n if surface else 0:] == 0xEE).all() for b in self.planes)
        return h, s

    def any(self, scene, n, per_ray=True, **kw):
        self.canary()
        self.ms = scene.trace_device(n, self.rays.ptr, tmax_ptr=self.bounds.ptr if per_ray else None, occluded_ptr=self.occ.ptr, mode=self.pt.TRACE_ANY, **kw)
        o = self.occ.read(np.uint8, self.n)
        assert (o[n:] == 0xEE).all()
        return o[:n]

    def close(self):
        for b in [self.rays, self.bounds, self.hits, self.occ] + self.planes:
            b.close()


def _check_closest(ans, n, got, what):
    h, s = got
    if h is not None:
        assert h.tobytes() == ans.hits[:n].tobytes(), (what, n, np.flatnonzero(h != ans.hits[:n])[:4])
    if s is not None:
        for k, name in enumerate(PLANES):
            assert s[k].tobytes() == ans.surface[k][:n].tobytes(), (what, n, name, np.abs(s[k] - ans.surface[k][:n]).max())


def _shares_ok(ans, n):
    if n >= 63:
        assert 0.3 <= ans.hit_share(n) <= 0.9 and 0.2 <= ans.occ_share(n) <= 0.8, (n, ans.hit_share(n), ans.occ_share(n))


@pytest.fixture(scope="module")
def box(orc, cornell_arrays):
    return tc.answers("box", lambda: tc.Answers(orc.Scene(*cornell_arrays), cornell_arrays[2], tc.make_rays()))


@pytest.fixture(scope="module")
def box_query(pt, gpu_ctx, box):
    q = Query(pt, gpu_ctx, box.rays, box.bounds)
    yield q
    q.close()


@pytest.mark.parametrize("extend", ["AUTO", "LDS", "HBM"])
def test_box_closest_hits_and_surface(pt, cornell_gpu, box, box_query, extend):
    """every prefix of the box's rays: d_hits == the oracle == pt_trace, the surface planes == shade_hit / faces; and the same with d_hits NULL"""
    ext = getattr(pt, "EXTEND_" + extend)
    assert box.hits["prim"][0] != MISS
    for n in tc.PREFIXES:
        _shares_ok(box, n)
        got = box_query.closest(cornell_gpu, n, extend=ext)
        _check_closest(box, n, got, extend)
        assert got[0].tobytes() == cornell_gpu.trace(box.rays[:n], extend=ext).tobytes()
        _check_closest(box, n, box_query.closest(cornell_gpu, n, hits=False, extend=ext), extend + " surface only")
    # hits alone, and one plane alone
    _check_closest(box, 257, box_query.closest(cornell_gpu, 257, surface=False, extend=ext), extend + " hits only")
    box_query.canary()
    cornell_gpu.trace_device(65, box_query.rays.ptr, normal_ptr=box_query.planes[1].ptr, extend=ext)
    assert box_query.planes[1].read(f32, (65, 3)).tobytes() == box.surface[1][:65].tobytes()
    assert (box_query.planes[0].read(np.uint8, 12) == 0xEE).all() and (box_query.hits.read(np.uint8, 20) == 0xEE).all()


@pytest.mark.parametrize("extend", ["AUTO", "LDS", "HBM"])
def test_box_any_hit(pt, cornell_gpu, box, box_query, extend):
    """occluded == the oracle's "a closest hit exists below the ray's bound": per-ray bounds cycling through 1e-4, 0.5, 2, 10000, and one bound
    for all (d_tmax NULL)"""
    ext = getattr(pt, "EXTEND_" + extend)
    assert box.occ_cycled[0] == 0 and box.hits["prim"][0] != MISS   # the camera axis hits, and its bound of 1e-4 hides the hit
    for n in tc.PREFIXES:
        _shares_ok(box, n)
        o = box_query.any(cornell_gpu, n, extend=ext)
        assert (o == box.occ_cycled[:n]).all(), (extend, n, np.flatnonzero(o != box.occ_cycled[:n])[:8])
        o = box_query.any(cornell_gpu, n, per_ray=False, tmax=box.uniform_bound, extend=ext)
        assert (o == box.occ_uniform[:n]).all(), (extend, n, "uniform")
    assert 0.05 < box.occ_uniform.mean() < 0.95


def test_chunks_stats_and_workspace(pt, cornell_arrays, box):
    """257 rays in chunks of 64 (five launches, the last of one ray) give the bytes of one chunk, in both modes; launches_extend grows by the
    chunks, launches_other by the pack and unpack launches, rays and paths stay; the workspace is the context's, is made by the first call,
    and only grows"""
    ctx = pt.Context(0)
    scene = pt.Scene(ctx, *cornell_arrays)
    q = Query(pt, ctx, box.rays, box.bounds)
    try:
        assert ctx.trace_workspace_bytes() == 0
        n = 257
        _shares_ok(box, n)
        ctx.reset_stats()
        got = q.closest(scene, n, chunk_rays=64)
        st = ctx.stats()
        assert (st.launches_extend, st.launches_other, st.rays, st.paths) == (5, 15, 0, 0), (st.launches_extend, st.launches_other, st.rays, st.paths)
        assert st.ms_extend > 0 and q.ms >= st.ms_extend * 0.99
        _check_closest(box, n, got, "chunks of 64")
        held = ctx.trace_workspace_bytes()
        assert held == 64 * 48 + 8, held
        ctx.reset_stats()
        o = q.any(scene, n, chunk_rays=64)
        assert (o == box.occ_cycled[:n]).all()
        assert (ctx.stats().launches_extend, ctx.stats().launches_other) == (5, 10)
        assert ctx.trace_workspace_bytes() == held                      # a second call allocates nothing
        _check_closest(box, n, q.closest(scene, n, chunk_rays=33), "chunk_rays 33 is 64")
        assert ctx.trace_workspace_bytes() == held
        _check_closest(box, n, q.closest(scene, n, chunk_rays=128), "chunks of 128")
        assert ctx.trace_workspace_bytes() == 128 * 48 + 8               # a larger chunk grows it
        q.closest(scene, n, chunk_rays=64)
        assert ctx.trace_workspace_bytes() == 128 * 48 + 8               # ... and it never shrinks
        ctx.reset_stats()
        _check_closest(box, n, q.closest(scene, n), "one chunk")          # the default chunk: no more than the rays, rounded up to 64
        assert ctx.trace_workspace_bytes() == 320 * 48 + 8 and ctx.stats().launches_extend == 1
    finally:
        q.close(); scene.close(); ctx.close()


def test_async_then_sync(pt, gpu_ctx, cornell_gpu, box, box_query):
    """PT_TRACE_ASYNC only queues (device_ms 0, ms_extend untouched); after pt_sync the outputs are the blocking call's"""
    n = 1000
    _shares_ok(box, n)
    gpu_ctx.reset_stats()
    assert box_query.closest(cornell_gpu, n, sync=False, flags=pt.TRACE_ASYNC, chunk_rays=256) is None
    assert box_query.ms == 0.0
    gpu_ctx.sync()
    st = gpu_ctx.stats()
    assert st.launches_extend == 4 and st.ms_extend == 0.0
    _check_closest(box, n, box_query.read_closest(n), "async")


def test_soup_hbm_class(pt, orc, gpu_ctx):
    """a 4 096-triangle soup (the class walked out of L2): AUTO, HBM and the 8-wide tree (its own triangle order), CLOSEST + surface, and ANY"""
    v, i, f = tc.soup(4096, 11)
    rays = tc.make_rays(seed=2024, half=1.3, centre=None)
    ans = tc.Answers(orc.Scene(v, i, f), f, rays)
    assert 0.05 < ans.hit_share(1000) < 0.95, ans.hit_share(1000)
    assert 0.02 < ans.occ_share(1000) < 0.95, ans.occ_share(1000)
    scene = pt.Scene(gpu_ctx, v, i, f)
    q = Query(pt, gpu_ctx, rays, ans.bounds)
    try:
        for name in ("AUTO", "HBM", "HBM8"):
            ext = getattr(pt, "EXTEND_" + name)
            got = q.closest(scene, 1000, extend=ext, chunk_rays=512)
            _check_closest(ans, 1000, got, name)
            assert got[0].tobytes() == scene.trace(rays, extend=ext).tobytes()
            assert (q.any(scene, 1000, extend=ext) == ans.occ_cycled).all(), name
            assert (q.any(scene, 1000, per_ray=False, tmax=ans.uniform_bound, extend=ext) == ans.occ_uniform).all(), name
    finally:
        q.close(); scene.close()


@pytest.mark.parametrize("knobs", [{}, {"inst16": 0}, {"inst_frames": 0}], ids=["default", "inst16_off", "inst_frames_off"])
def test_instanced_box(pt, orc, gpu_ctx, cornell_arrays, knobs):
    """the box three times (a translation, a scale by one half, a rotation): inst, the world-space position and normal equal the oracle's; both
    two-level kernels, the frame table and the inverse transpose"""
    def make():
        osc = orc.Scene(*cornell_arrays)
        osc.set_instances(tc.INSTANCES)
        return tc.Answers(osc, cornell_arrays[2], tc.make_rays(seed=7, x_seed=8))
    ans = tc.answers("inst", make)
    hit = ans.hits["prim"] != MISS
    assert 0.2 <= hit.mean() <= 0.8 and set(np.unique(ans.hits["inst"][hit])) == {0, 1, 2}
    old = gpu_ctx.set_tuning(**knobs)
    scene = pt.Scene(gpu_ctx, *cornell_arrays)
    q = Query(pt, gpu_ctx, ans.rays, ans.bounds)
    try:
        scene.set_instances(tc.INSTANCES)
        for n in (65, 1000):
            got = q.closest(scene, n)
            _check_closest(ans, n, got, str(knobs))
            assert got[0].tobytes() == scene.trace(ans.rays[:n]).tobytes()
            assert (q.any(scene, n) == ans.occ_cycled[:n]).all()
            assert (q.any(scene, n, per_ray=False, tmax=ans.uniform_bound) == ans.occ_uniform[:n]).all()
    finally:
        q.close(); scene.close()
        gpu_ctx.set_tuning(**old)


def test_after_scene_update(pt, orc, gpu_ctx, cornell_arrays, box):
    """REFIT of the box with the short block moved: the query equals the oracle of the new arrays (and differs from the old answer)"""
    v, i, f = cornell_arrays
    v2 = tc.move_short_box(v)
    ans = tc.Answers(orc.Scene(v2, i, f), f, box.rays)
    assert ans.hits.tobytes() != box.hits.tobytes()
    _shares_ok(ans, 1000)
    scene = pt.Scene(gpu_ctx, v, i, f)
    q = Query(pt, gpu_ctx, box.rays, box.bounds)
    try:
        _check_closest(box, 1000, q.closest(scene, 1000), "before the update")
        scene.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
        _check_closest(ans, 1000, q.closest(scene, 1000), "after the update")
        assert (q.any(scene, 1000) == ans.occ_cycled).all()
    finally:
        q.close(); scene.close()


def test_trace_tensors(pt, cornell_gpu, box):
    """torch tensors in and out: a contiguous tensor, a non-contiguous [n, 6] view, and rays made by a torch op on torch's stream immediately
    before the call"""
    import torch
    n = 1000
    _shares_ok(box, n)
    dev = torch.device("cuda", 0)
    host = torch.from_numpy(box.rays)

    def check(out):
        assert out["prim"].dtype == torch.int32 and out["t"].dtype == torch.float32 and out["prim"].data_ptr() + 4 == out["t"].data_ptr()
        got = np.zeros(n, pt.HIT_DTYPE)
        got["prim"], got["inst"] = out["prim"].cpu().numpy().view(np.uint32), out["inst"].cpu().numpy().view(np.uint32)
        got["t"], got["u"], got["v"] = out["t"].cpu().numpy(), out["u"].cpu().numpy(), out["v"].cpu().numpy()
        assert got.tobytes() == box.hits.tobytes()
        for k, name in enumerate(PLANES):
            assert out[name].shape == (n, 3) and out[name].cpu().numpy().tobytes() == box.surface[k].tobytes(), name

    check(cornell_gpu.trace_tensors(host.to(dev), surface=True))
    assert set(cornell_gpu.trace_tensors(host.to(dev))) == {"prim", "t", "u", "v", "inst"}
    wide = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    wide[:, 1:7] = host.to(dev)
    view = wide[:, 1:7]
    assert not view.is_contiguous()
    check(cornell_gpu.trace_tensors(view, surface=True))
    # made on torch's stream right before the call: the wrapper has to wait for it
    o, d = host[:, :3].to(dev), host[:, 3:].to(dev)
    big = torch.zeros((4096, 4096), device=dev)
    for _ in range(4):
        big = big @ big                                                    # (work ahead of the rays on torch's stream)
    check(cornell_gpu.trace_tensors(torch.cat((o, d), dim=1), surface=True))
    bounds = torch.from_numpy(box.bounds).to(dev)
    occ = cornell_gpu.trace_tensors(torch.cat((o, d), dim=1), tmax_per_ray=bounds, mode=pt.TRACE_ANY)
    assert occ.dtype == torch.bool and (occ.cpu().numpy() == box.occ_cycled.astype(bool)).all()
    occ = cornell_gpu.trace_tensors(host.to(dev), mode=pt.TRACE_ANY, tmax=box.uniform_bound)
    assert (occ.cpu().numpy() == box.occ_uniform.astype(bool)).all()
    with pytest.raises(ValueError):
        cornell_gpu.trace_tensors(host.to(dev).double())
    with pytest.raises(pt.PtError):   # the per-ray bound belongs to the any-hit query
        cornell_gpu.trace_tensors(host.to(dev), tmax_per_ray=bounds)


def test_refusals_leave_everything_untouched(pt, gpu_ctx, cornell_gpu, box, box_query):
    """every refusal of the header returns its status with nothing launched and nothing written; n == 0 is PT_OK and launches nothing; after a
    refusal, and after an out-of-memory chunk, the next good call works"""
    q, lib, n = box_query, pt.lib_amd(), 257
    nan, inf = float("nan"), float("inf")

    def desc(mode=pt.TRACE_CLOSEST, **kw):
        d = pt.trace_default_desc()
        d.d_rays6, d.mode = q.rays.ptr, mode
        if mode == pt.TRACE_ANY:
            d.d_occluded, d.d_tmax = q.occ.ptr, q.bounds.ptr
        else:
            d.d_hits, d.d_position, d.d_normal, d.d_albedo, d.d_emission = [q.hits.ptr] + [b.ptr for b in q.planes]
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[2] = v
            else:
                setattr(d, k, v)
        return d

    INVALID, UNSUPPORTED = 1, 5
    cases = [(desc(d_rays6=None), INVALID), (desc(mode=2), INVALID), (desc(flags=2), INVALID), (desc(flags=3), INVALID), (desc(reserved=1), INVALID),
             (desc(tmin=nan), INVALID), (desc(tmax=nan), INVALID), (desc(tmax=inf), INVALID), (desc(tmin=-inf), INVALID), (desc(tmin=1.0, tmax=1.0), INVALID),
             (desc(tmin=2.0, tmax=1.0), INVALID),
             (desc(d_hits=None, d_position=None, d_normal=None, d_albedo=None, d_emission=None), INVALID), (desc(d_occluded=q.occ.ptr), INVALID),
             (desc(pt.TRACE_ANY, d_hits=q.hits.ptr), INVALID), (desc(pt.TRACE_ANY, d_albedo=q.planes[2].ptr), INVALID),
             (desc(pt.TRACE_ANY, d_occluded=None), INVALID), (desc(extend=9), INVALID),
             (desc(d_tmax=q.bounds.ptr), UNSUPPORTED), (desc(extend=pt.EXTEND_FLAT), UNSUPPORTED), (desc(pt.TRACE_ANY, extend=pt.EXTEND_FLAT), UNSUPPORTED)]
    q.canary()
    gpu_ctx.reset_stats()
    for k, (d, want) in enumerate(cases):
        assert lib.pt_trace_device(cornell_gpu.h, C.byref(d), n, None) == want, k
    assert lib.pt_trace_device(None, C.byref(desc()), n, None) == INVALID
    assert lib.pt_trace_device(cornell_gpu.h, None, n, None) == INVALID
    ms = C.c_float(-1.0)
    assert lib.pt_trace_device(cornell_gpu.h, C.byref(desc()), 0, C.byref(ms)) == 0 and ms.value == 0.0       # n == 0
    assert lib.pt_trace_device(cornell_gpu.h, C.byref(desc(d_rays6=None)), 0, None) == 0
    gpu_ctx.sync()
    st = gpu_ctx.stats()
    assert (st.launches_extend, st.launches_other) == (0, 0) and q.untouched()
    _check_closest(box, n, q.closest(cornell_gpu, n), "after the refusals")
    # a chunk that does not fit the budget: 65 536 rays are 3 MB of workspace
    many = np.ascontiguousarray(np.tile(box.rays, (66, 1))[:65536])
    big = Query(pt, gpu_ctx, many)
    old = gpu_ctx.set_tuning(mem_budget_mb=1)
    try:
        with pytest.raises(pt.PtError) as e:
            big.closest(cornell_gpu, 65536)
        assert e.value.status == 4 and big.untouched()                       # PT_ERR_OOM
        got = big.closest(cornell_gpu, 65536, chunk_rays=4096)               # a smaller chunk fits
        assert got[0].tobytes() == np.tile(box.hits, 66)[:65536].tobytes()
        assert gpu_ctx.trace_workspace_bytes() == 4096 * 48 + 8
    finally:
        gpu_ctx.set_tuning(**old)
        big.close()
    _check_closest(box, n, q.closest(cornell_gpu, n), "after the out-of-memory chunk")
