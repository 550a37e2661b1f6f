"""pt_radiance_device on the GPU (include/pt_api.h): rays in device memory, path-traced radiance in device memory.  Every
comparison is bit for bit: against orc.Scene.render_frame where the rays are a camera's (plain estimator and next-event estimation, every
extend kernel), against the Python path loop of tests/radiance_cases.py where they are not, against numpy for the reduce, the chunks and the
blend.  tests/test_radiance_device_cpu.py checks the recipes against the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import radiance_cases as rcs
import trace_device_cases as tc

f32 = np.float32
pytestmark = pytest.mark.gpu
CANARY = 0xEE


class Call:
    """the device buffers of one ray set (pt_device_alloc: no torch needed); outputs are filled with a canary before every call"""

    def __init__(self, pt, ctx, rays, seeds=None):
        self.pt, self.ctx, self.n = pt, ctx, len(rays)
        self.rays = pt.DeviceBuffer(ctx, rays.nbytes)
        self.rays.write(rays)
        self.seeds = None
        if seeds is not None:
            self.set_seeds(seeds)
        self.out = pt.DeviceBuffer(ctx, 12 * self.n)
        self.m2 = pt.DeviceBuffer(ctx, 12 * self.n)
        self.ms = 0.0

    def set_seeds(self, seeds):
        if self.seeds is not None:
            self.seeds.close()
        s = np.ascontiguousarray(seeds, np.uint32)
        self.seeds = self.pt.DeviceBuffer(self.ctx, s.nbytes)
        self.seeds.write(s)

    def canary(self):
        for b in (self.out, self.m2):
            b.write(np.full(b.nbytes, CANARY, np.uint8))

    def untouched(self):
        return all((b.read(np.uint8, b.nbytes) == CANARY).all() for b in (self.out, self.m2))

    def run(self, scene, n=None, first=0, seeds=True, m2=False, keep=False, **kw):
        """rays [first, first + n) -> mean [n, 3] (and the second moment); nothing beyond them is written"""
        n = self.n - first if n is None else n
        if not keep:
            self.canary()
        sp = self.seeds.ptr + 4 * first * kw.get("spp", 32) if (seeds and self.seeds is not None) else None
        self.ms = scene.radiance_device(n, self.rays.ptr + 24 * first, self.out.ptr + 12 * first, seeds_ptr=sp,
                                        moment2_ptr=self.m2.ptr + 12 * first if m2 else None, **kw)
        raw = self.out.read(np.uint8, self.out.nbytes)
        if not keep:
            assert (raw[:12 * first] == CANARY).all() and (raw[12 * (first + n):] == CANARY).all()
            if not m2:
                assert (self.m2.read(np.uint8, self.m2.nbytes) == CANARY).all()
        got = self.out.read(f32, (self.n, 3))[first:first + n]
        return (got, self.m2.read(f32, (self.n, 3))[first:first + n]) if m2 else got

    def close(self):
        for b in (self.rays, self.seeds, self.out, self.m2):
            if b is not None:
                b.close()


def _camera_check(pt, ctx, scene, cam, nee, **kw):
    """spp = 1 with the advanced seeds of primary_ray == render_frame, and pt_stats.rays == the oracle's count"""
    q = Call(pt, ctx, cam.rays, cam.seeds)
    try:
        ctx.reset_stats()
        got = q.run(scene, spp=1, max_depth=cam.depth, flags=pt.RADIANCE_NEE if nee else 0, **kw)
        st = ctx.stats()
        want = cam.want[int(nee)]
        assert got.tobytes() == want.tobytes(), (kw, nee, int((got != want).any(1).sum()), float(np.abs(got - want).max()))
        assert st.rays == cam.n_rays[int(nee)], (st.rays, cam.n_rays[int(nee)])
        assert st.paths == cam.n and st.rounds == cam.depth and st.launches_shade == cam.depth
        return st
    finally:
        q.close()


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
@pytest.mark.parametrize("extend", ["AUTO", "LDS", "HBM"])
def test_camera_equivalence_box(pt, orc, gpu_ctx, cornell_gpu, cornell_arrays, extend, nee):
    cam = rcs.box_camera(orc, cornell_arrays)
    assert int(cam.hit.sum()) == 215 and cam.nee_differs > 0.5
    st = _camera_check(pt, gpu_ctx, cornell_gpu, cam, nee, extend=getattr(pt, "EXTEND_" + extend))
    assert st.extend_variant == (pt.EXTEND_HBM if extend == "HBM" else pt.EXTEND_LDS)
    assert st.launches_extend == cam.depth * (2 if nee else 1) and st.launches_other == 2 + (cam.depth if nee else 0)


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
@pytest.mark.parametrize("knobs", [{}, {"inst16": 0}, {"inst_frames": 0}], ids=["default", "inst16_off", "inst_frames_off"])
def test_camera_equivalence_instances(pt, orc, gpu_ctx, cornell_arrays, knobs, nee):
    cam = rcs.inst_camera(orc, cornell_arrays)
    assert set(np.unique(cam.first["inst"][cam.hit])) == {0, 1, 2}
    old = gpu_ctx.set_tuning(**knobs)
    scene = pt.Scene(gpu_ctx, *cornell_arrays)
    try:
        scene.set_instances(tc.INSTANCES)
        _camera_check(pt, gpu_ctx, scene, cam, nee)
    finally:
        scene.close()
        gpu_ctx.set_tuning(**old)


@pytest.fixture(scope="module")
def soup_gpu(pt, gpu_ctx):
    sc = pt.Scene(gpu_ctx, *rcs.soup_arrays())
    yield sc
    sc.close()


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
@pytest.mark.parametrize("extend", ["AUTO", "HBM", "HBM8"])
def test_camera_equivalence_soup(pt, orc, gpu_ctx, soup_gpu, extend, nee):
    cam = rcs.soup_camera(orc)
    assert 0.2 < cam.hit.mean() < 0.6 and cam.nee_differs > 0.2
    st = _camera_check(pt, gpu_ctx, soup_gpu, cam, nee, extend=getattr(pt, "EXTEND_" + extend))
    if extend != "AUTO":
        assert st.extend_variant == getattr(pt, "EXTEND_" + extend)


@pytest.fixture(scope="module")
def free(orc, cornell_arrays):
    return rcs.box_free(orc, cornell_arrays)


@pytest.fixture(scope="module")
def free_call(pt, gpu_ctx, free):
    q = Call(pt, gpu_ctx, free.rays, free.seeds)
    yield q
    q.close()


def test_free_rays_hashed_seeds(pt, gpu_ctx, cornell_gpu, free, free_call):
    """prefixes 1, 63, 64, 65, 257 of the free rays at 3 samples, depth 4, the header's seed rule (d_seeds NULL) == the Python path loop, reduced
    in order; pt_stats.paths == 3 n and pt_stats.rays == the loop's count"""
    assert (free.mean != 0).any(1).mean() >= 0.8
    for n in rcs.PREFIXES:
        gpu_ctx.reset_stats()
        got, m2 = free_call.run(cornell_gpu, n, seeds=False, m2=True, spp=free.spp, max_depth=free.depth)
        assert got.tobytes() == free.mean[:n].tobytes(), (n, np.flatnonzero((got != free.mean[:n]).any(1))[:4])
        assert m2.tobytes() == free.m2[:n].tobytes(), n
        st = gpu_ctx.stats()
        assert st.paths == 3 * n and st.rays == int(free.traced[:n].sum()), (n, st.paths, st.rays)
    # ... and the same seeds handed in through d_seeds
    assert free_call.run(cornell_gpu, 257, spp=free.spp, max_depth=free.depth).tobytes() == free.mean.tobytes()


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_reduce_is_independent_of_the_estimator(pt, gpu_ctx, cornell_gpu, free, nee):
    """spp = 3 with d_seeds == the numpy ordered sum of three spp = 1 calls with the matching seed columns; d_moment2 too"""
    flags = pt.RADIANCE_NEE if nee else 0
    q = Call(pt, gpu_ctx, free.rays, free.seeds)
    try:
        got, m2 = q.run(cornell_gpu, m2=True, spp=3, max_depth=free.depth, flags=flags)
        c = np.zeros((free.n, 3, 3), f32)
        for s in range(3):
            q.set_seeds(free.seeds[:, s])
            c[:, s], sq = q.run(cornell_gpu, m2=True, spp=1, max_depth=free.depth, flags=flags)
            assert sq.tobytes() == (c[:, s] * c[:, s]).astype(f32).tobytes()
        want, want2 = rcs.ordered_mean(c)
        assert got.tobytes() == want.tobytes() and m2.tobytes() == want2.tobytes()
        if nee:
            assert (want != free.mean).any(1).mean() > 0.3   # (another estimator: most rays get other bits)
        else:
            assert want.tobytes() == free.mean.tobytes()
    finally:
        q.close()


def test_chunks_index_base_and_workspace(pt, cornell_arrays, free):
    """257 rays in chunks of 64 == the automatic chunk; rays [100, 257) with index_base = 100 == that slice of the full call; the workspace is
    made by the first call, grows once, and a second call allocates nothing"""
    ctx = pt.Context(0)
    scene = pt.Scene(ctx, *cornell_arrays)
    q = Call(pt, ctx, free.rays)
    kw = dict(spp=free.spp, max_depth=free.depth)
    try:
        assert ctx.radiance_workspace_bytes() == 0
        ctx.reset_stats()
        got = q.run(scene, chunk_rays=64, **kw)
        assert got.tobytes() == free.mean.tobytes()
        st = ctx.stats()
        assert (st.rounds, st.launches_extend, st.launches_shade, st.launches_other) == (5 * 4, 5 * 4, 5 * 4, 5 * 2)
        assert st.paths == 3 * 257 and st.rays == int(free.traced.sum())
        held = ctx.radiance_workspace_bytes()
        assert held == 64 * 3 * 132 + 16 + 4, held
        assert q.run(scene, chunk_rays=33, **kw).tobytes() == free.mean.tobytes() and ctx.radiance_workspace_bytes() == held
        assert q.run(scene, **kw).tobytes() == free.mean.tobytes()                       # the automatic chunk: the rays there are, rounded up to 64
        grown = ctx.radiance_workspace_bytes()
        assert grown == 320 * 3 * 132 + 16 + 4, grown
        assert q.run(scene, 157, first=100, index_base=100, **kw).tobytes() == free.mean[100:].tobytes()
        assert q.run(scene, 157, first=100, **kw).tobytes() != free.mean[100:].tobytes()   # (without it the slice hashes as rays 0 .. 156)
        q.run(scene, chunk_rays=64, **kw)
        assert ctx.radiance_workspace_bytes() == grown                                      # it never shrinks
        q.run(scene, flags=pt.RADIANCE_NEE, **kw)                                           # the shadow queue, on first NEE use
        assert ctx.radiance_workspace_bytes() == grown + 320 * 3 * 64
    finally:
        q.close(); scene.close(); ctx.close()


def test_frames_and_accumulate(pt, gpu_ctx, cornell_gpu, free, free_call):
    """frames 0, 1, 2 with PT_RADIANCE_ACCUMULATE == numpy's blend of the three per-frame means (and second moments); frame 1 differs from
    frame 0; frame 0 into a NaN-filled output holds no NaN"""
    q, kw = free_call, dict(seeds=False, spp=free.spp, max_depth=free.depth)
    per = [q.run(cornell_gpu, m2=True, frame=k, **kw) for k in range(3)]
    assert per[0][0].tobytes() == free.mean.tobytes()
    assert (per[1][0] != per[0][0]).any(1).mean() > 0.3
    nan = np.full((free.n, 3), np.nan, f32)
    q.out.write(nan); q.m2.write(nan)
    film = film2 = None
    for k in range(3):
        got, got2 = q.run(cornell_gpu, m2=True, keep=True, frame=k, flags=pt.RADIANCE_ACCUMULATE, **kw)
        assert not np.isnan(got).any() and not np.isnan(got2).any(), k
        film, film2 = rcs.blend(film, per[k][0], k), rcs.blend(film2, per[k][1], k)
        assert got.tobytes() == film.tobytes() and got2.tobytes() == film2.tobytes(), k


def test_after_a_refit(pt, gpu_ctx, cornell_arrays, free):
    """after pt_scene_update REFIT the radiance equals a fresh scene's of the same arrays (and differs from the old scene's)"""
    v, i, f = cornell_arrays
    v2 = tc.move_short_box(v)
    kw = dict(seeds=False, spp=free.spp, max_depth=free.depth)
    scene, fresh = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v2, i, f)
    q = Call(pt, gpu_ctx, free.rays)
    try:
        before = q.run(scene, **kw).copy()
        assert before.tobytes() == free.mean.tobytes()
        scene.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
        after, want = q.run(scene, **kw).copy(), q.run(fresh, **kw).copy()
        assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()
    finally:
        q.close(); scene.close(); fresh.close()


def test_radiance_tensors(pt, cornell_gpu, free):
    """torch tensors in and out: a non-contiguous [n, 6] view, rays made on torch's stream just before the call, seeds, the second moment,
    accumulation into a caller's tensor"""
    import torch
    dev = torch.device("cuda", 0)
    host = torch.from_numpy(free.rays)
    kw = dict(spp=free.spp, max_depth=free.depth)
    wide = torch.zeros((free.n, 8), dtype=torch.float32, device=dev)
    wide[:, 1:7] = host.to(dev)
    view = wide[:, 1:7]
    assert not view.is_contiguous()
    out = cornell_gpu.radiance_tensors(view, **kw)
    assert out.shape == (free.n, 3) and out.dtype == torch.float32 and out.cpu().numpy().tobytes() == free.mean.tobytes()
    o, d = host[:, :3].to(dev), host[:, 3:].to(dev)
    big = torch.zeros((4096, 4096), device=dev)
    for _ in range(4):
        big = big @ big                                                    # (work ahead of the rays on torch's stream)
    seeds = torch.from_numpy(free.seeds.view(np.int32)).to(dev)
    out, m2 = cornell_gpu.radiance_tensors(torch.cat((o, d), dim=1), seeds=seeds, moment2=True, **kw)
    assert out.cpu().numpy().tobytes() == free.mean.tobytes() and m2.cpu().numpy().tobytes() == free.m2.tobytes()
    film = torch.full((free.n, 3), float("nan"), device=dev)
    assert cornell_gpu.radiance_tensors(host.to(dev), out=film, accumulate=True, frame=0, **kw) is film
    assert film.cpu().numpy().tobytes() == rcs.blend(None, free.mean, 0).tobytes()
    nee = cornell_gpu.radiance_tensors(host.to(dev), nee=True, **kw)
    assert (nee.cpu().numpy() != free.mean).any(1).mean() > 0.3
    with pytest.raises(ValueError):
        cornell_gpu.radiance_tensors(host.to(dev).double())
    with pytest.raises(ValueError):
        cornell_gpu.radiance_tensors(host.to(dev), out=torch.zeros((free.n, 4), device=dev)[:, :3], **kw)


def test_refusals_leave_everything_untouched(pt, gpu_ctx, cornell_gpu, cornell_arrays, free, free_call):
    """every refusal of the header returns its status with nothing launched and nothing written; n == 0 is PT_OK and launches nothing; after a
    refusal, and after an out-of-memory chunk, the next good call works"""
    q, lib, n = free_call, pt.lib_amd(), 257
    nan, inf = float("nan"), float("inf")

    def desc(**kw):
        d = pt.radiance_default_desc()
        d.d_rays6, d.d_seeds, d.d_radiance, d.d_moment2 = q.rays.ptr, q.seeds.ptr, q.out.ptr, q.m2.ptr
        d.spp, d.max_depth = free.spp, free.depth
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            elif k == "env":
                d.env[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    INVALID, UNSUPPORTED = 1, 5
    cases = [(desc(d_rays6=None), INVALID), (desc(d_radiance=None), INVALID), (desc(spp=0), INVALID), (desc(spp=65536), INVALID),
             (desc(max_depth=0), INVALID), (desc(max_depth=65536), INVALID), (desc(flags=4), INVALID), (desc(flags=0x80000001), INVALID),
             (desc(reserved=0), INVALID), (desc(reserved=3), INVALID), (desc(tmin=nan), INVALID), (desc(tmax=nan), INVALID), (desc(tmax=inf), INVALID),
             (desc(tmin=-inf), INVALID), (desc(tmin=1.0, tmax=1.0), INVALID), (desc(tmin=2.0, tmax=1.0), INVALID), (desc(env=(0, nan)), INVALID),
             (desc(env=(2, inf)), INVALID), (desc(flags=pt.RADIANCE_ACCUMULATE, frame=-1), INVALID), (desc(extend=9), INVALID),
             (desc(extend=pt.EXTEND_FLAT), UNSUPPORTED)]
    q.canary()
    gpu_ctx.reset_stats()
    for k, (d, want) in enumerate(cases):
        assert lib.pt_radiance_device(cornell_gpu.h, C.byref(d), n, None) == want, k
    # the variants a scene has no tree for, by pt_trace's rules: an instanced scene has neither the LDS kernel nor the 8-wide tree
    inst = pt.Scene(gpu_ctx, *cornell_arrays)
    try:
        inst.set_instances(tc.INSTANCES)
        for ext in (pt.EXTEND_LDS, pt.EXTEND_HBM8):
            with pytest.raises(pt.PtError) as e:
                inst.trace(free.rays[:1], extend=ext)
            assert e.value.status == UNSUPPORTED
            assert lib.pt_radiance_device(inst.h, C.byref(desc(extend=ext)), n, None) == UNSUPPORTED, ext
    finally:
        inst.close()
    assert lib.pt_radiance_device(None, C.byref(desc()), n, None) == INVALID
    assert lib.pt_radiance_device(cornell_gpu.h, None, n, None) == INVALID
    ms = C.c_float(-1.0)
    assert lib.pt_radiance_device(cornell_gpu.h, C.byref(desc()), 0, C.byref(ms)) == 0 and ms.value == 0.0       # n == 0
    assert lib.pt_radiance_device(cornell_gpu.h, C.byref(desc(d_rays6=None, d_radiance=None)), 0, None) == 0
    assert lib.pt_radiance_device(cornell_gpu.h, C.byref(desc(frame=-1)), 0, None) == 0                          # (a negative frame alone is no error)
    gpu_ctx.sync()
    st = gpu_ctx.stats()
    assert (st.launches_extend, st.launches_shade, st.launches_other, st.rays, st.paths) == (0, 0, 0, 0, 0) and q.untouched()
    kw = dict(spp=free.spp, max_depth=free.depth)
    assert q.run(cornell_gpu, **kw).tobytes() == free.mean.tobytes()
    # a chunk that does not fit the budget: 16 384 rays x 3 samples are 6.2 MB of workspace
    many = np.ascontiguousarray(np.tile(free.rays, (64, 1))[:16384])
    big = Call(pt, gpu_ctx, many, np.tile(free.seeds, (64, 1))[:16384])
    old = gpu_ctx.set_tuning(mem_budget_mb=1)
    try:
        with pytest.raises(pt.PtError) as e:
            big.run(cornell_gpu, **kw)
        assert e.value.status == 4 and big.untouched()                       # PT_ERR_OOM
        got = big.run(cornell_gpu, chunk_rays=1024, **kw)                    # a smaller chunk fits
        assert got.tobytes() == np.tile(free.mean, (64, 1))[:16384].tobytes()
        # (the slots of one chunk, and whatever shadow queue earlier tests of this context left: within the budget)
        assert 1024 * 3 * 132 + 20 <= gpu_ctx.radiance_workspace_bytes() <= 1 << 20
    finally:
        gpu_ctx.set_tuning(**old)
        big.close()
    assert q.run(cornell_gpu, **kw).tobytes() == free.mean.tobytes()
