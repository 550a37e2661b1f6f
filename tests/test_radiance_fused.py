"""The single-kernel form of pt_radiance_device on the GPU (PT_RADIANCE_FUSED / PT_RADIANCE_AUTO: include/pt_api.h).  The
result must not depend on the form, so every comparison is bit for bit: against the oracle where tests/radiance_cases.py has its answer,
against the wavefront form of the same call elsewhere.  The shapes -- 1, 63, 64, 65, 257 rays, 1 and 3 samples, chunks of 64 -- sit around the
64-slot chunks the kernel's hand-out counts in; 4097 rays at 2 samples fill many waves with paths of every length."""
import ctypes as C

import numpy as np
import pytest

import radiance_cases as rcs
import trace_device_cases as tc
from test_radiance_device import Call

f32 = np.float32
pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED, OOM = 1, 5, 4
COUNT_BYTES = 1024                      # the eight slot counters, 128 B apart (include/pt_api.h: the workspace formula)
# What PT_RADIANCE_AUTO takes on the box, per estimator (plain, NEE): DESIGN.md section 25's measurements decide, radiance_device.hip
# RD_AUTO_TAKES_FUSED states it
AUTO_TAKES_FUSED = (True, True)


def _flags(pt, nee, form=None):
    return (pt.RADIANCE_NEE if nee else 0) | (pt.RADIANCE_FUSED if form is None else form)


def _nee_pipeline(pt, nee):
    return pt.PIPELINE_WAVEFRONT_NEE if nee else pt.PIPELINE_WAVEFRONT


def _camera_fused(pt, ctx, scene, cam, nee):
    q = Call(pt, ctx, cam.rays, cam.seeds)
    try:
        ctx.reset_stats()
        got = q.run(scene, spp=1, max_depth=cam.depth, flags=_flags(pt, nee))
        st = ctx.stats()
        want = cam.want[int(nee)]
        assert got.tobytes() == want.tobytes(), (nee, int((got != want).any(1).sum()), float(np.abs(got - want).max()))
        assert st.rays == cam.n_rays[int(nee)], (st.rays, cam.n_rays[int(nee)])
        assert st.paths == cam.n
        assert st.pipeline == pt.PIPELINE_FUSED and st.extend_variant == pt.EXTEND_LDS
        assert (st.rounds, st.launches_extend, st.launches_shade, st.launches_other) == (1, 1, 0, 1), (st.rounds, st.launches_extend, st.launches_shade, st.launches_other)
    finally:
        q.close()


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
@pytest.mark.parametrize("pairs", [True, False], ids=["pair_leaves", "leaves_of_four"])
def test_camera_equivalence(pt, orc, gpu_ctx, cornell_gpu, cornell_arrays, pairs, nee):
    """the box through the default camera, 24 x 16, depth 4, spp 1 with primary_ray's advanced seeds == render_frame, the oracle's ray count; one
    round, one fused launch, one resolve, no shade launch -- on the pair-leaf tree and on a scene created under pt_tuning.pair_leaves = 0"""
    cam = rcs.box_camera(orc, cornell_arrays)
    assert int(cam.hit.sum()) == 215 and cam.nee_differs > 0.5
    if pairs:
        _camera_fused(pt, gpu_ctx, cornell_gpu, cam, nee)
        return
    old = gpu_ctx.set_tuning(pair_leaves=0)
    try:
        scene = pt.Scene(gpu_ctx, *cornell_arrays)
    finally:
        gpu_ctx.set_tuning(**old)
    try:
        _camera_fused(pt, gpu_ctx, scene, cam, nee)
    finally:
        scene.close()


@pytest.fixture(scope="module")
def free(orc, cornell_arrays):
    return rcs.box_free(orc, cornell_arrays)


@pytest.fixture(scope="module")
def free_call(pt, gpu_ctx, free):
    q = Call(pt, gpu_ctx, free.rays, free.seeds)
    yield q
    q.close()


@pytest.mark.parametrize("given", [False, True], ids=["hashed", "d_seeds"])
def test_free_rays(pt, gpu_ctx, cornell_gpu, free, free_call, given):
    """prefixes 1, 63, 64, 65, 257 of the free rays at 3 samples, depth 4 == the Python path loop reduced in order, with the second moment; the
    seeds hashed by the header's rule or handed in; pt_stats.rays == the loop's count"""
    for n in rcs.PREFIXES:
        gpu_ctx.reset_stats()
        got, m2 = free_call.run(cornell_gpu, n, seeds=given, m2=True, spp=free.spp, max_depth=free.depth, flags=pt.RADIANCE_FUSED)
        assert got.tobytes() == free.mean[:n].tobytes(), (n, np.flatnonzero((got != free.mean[:n]).any(1))[:4])
        assert m2.tobytes() == free.m2[:n].tobytes(), n
        st = gpu_ctx.stats()
        assert st.paths == 3 * n and st.rays == int(free.traced[:n].sum()), (n, st.paths, st.rays)
        assert st.pipeline == pt.PIPELINE_FUSED and st.rounds == 1


@pytest.fixture(scope="module")
def many(pt, gpu_ctx, cornell_gpu, cornell_arrays):
    """4097 rays from a fixed generator -- origins inside the box, directions on the sphere -- at 2 samples, depth 8: the wavefront form's answer
    for both estimators, computed once"""
    v = np.asarray(cornell_arrays[0], f32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    rng = np.random.default_rng(4097)
    o = (lo + (hi - lo) * rng.uniform(0.02, 0.98, (4097, 3))).astype(f32)
    d = rng.standard_normal((4097, 3)).astype(f32)
    d = (d / np.sqrt((d * d).sum(1, dtype=f32))[:, None]).astype(f32)
    rays = np.ascontiguousarray(np.concatenate([o, d], 1), f32)
    q = Call(pt, gpu_ctx, rays)
    want = {}
    for nee in (False, True):
        gpu_ctx.reset_stats()
        mean, m2 = q.run(cornell_gpu, m2=True, seeds=False, spp=2, max_depth=8, flags=_flags(pt, nee, 0))
        want[nee] = (mean.copy(), m2.copy(), gpu_ctx.stats().rays)
    yield q, want
    q.close()


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_form_independence_on_many_rays(pt, gpu_ctx, cornell_gpu, many, nee):
    """radiance, second moment and the pt_stats.rays delta of the fused form == the wavefront form's, in chunks of 64 rays and with the automatic
    chunk; the input is no trivial one: at least half the rays end with something other than env, and NEE changes at least 0.3 of them"""
    q, want = many
    env = np.asarray(rcs.ENV, f32)
    assert (want[False][0] != env).any(1).mean() >= 0.5, (want[False][0] != env).any(1).mean()
    assert (want[True][0] != want[False][0]).any(1).mean() >= 0.3, (want[True][0] != want[False][0]).any(1).mean()
    assert want[True][2] > want[False][2] > 2 * 4097
    mean, m2, rays = want[nee]
    for chunk in (64, 0):
        gpu_ctx.reset_stats()
        got, got2 = q.run(cornell_gpu, m2=True, seeds=False, spp=2, max_depth=8, flags=_flags(pt, nee), chunk_rays=chunk)
        st = gpu_ctx.stats()
        assert got.tobytes() == mean.tobytes(), (chunk, np.flatnonzero((got != mean).any(1))[:8])
        assert got2.tobytes() == m2.tobytes(), chunk
        assert st.rays == rays and st.paths == 2 * 4097, (chunk, st.rays, rays)
        chunks = 65 if chunk else 1
        assert (st.rounds, st.launches_extend, st.launches_shade, st.launches_other) == (chunks, chunks, 0, chunks)


def test_accumulate_and_index_base(pt, gpu_ctx, cornell_gpu, free, free_call):
    """rays [100, 257) with index_base = 100 == that slice of the full call; frames 0, 1, 2 with PT_RADIANCE_ACCUMULATE == numpy's blend of the
    per-frame means; frame 0 into a NaN-filled output holds no NaN"""
    q, kw = free_call, dict(seeds=False, spp=free.spp, max_depth=free.depth)
    F = pt.RADIANCE_FUSED
    assert q.run(cornell_gpu, 157, first=100, index_base=100, flags=F, **kw).tobytes() == free.mean[100:].tobytes()
    assert q.run(cornell_gpu, 157, first=100, flags=F, **kw).tobytes() != free.mean[100:].tobytes()
    per = [[a.copy() for a in q.run(cornell_gpu, m2=True, frame=k, flags=F, **kw)] for k in range(3)]
    assert per[0][0].tobytes() == free.mean.tobytes()
    assert (per[1][0] != per[0][0]).any(1).mean() > 0.3
    wave = [[a.copy() for a in q.run(cornell_gpu, m2=True, frame=k, **kw)] for k in (1, 2)]
    assert all(per[k + 1][j].tobytes() == wave[k][j].tobytes() for k in range(2) for j in range(2))
    nan = np.full((free.n, 3), np.nan, f32)
    q.out.write(nan); q.m2.write(nan)
    film = film2 = None
    for k in range(3):
        got, got2 = q.run(cornell_gpu, m2=True, keep=True, frame=k, flags=F | pt.RADIANCE_ACCUMULATE, **kw)
        assert not np.isnan(got).any() and not np.isnan(got2).any(), k
        film, film2 = rcs.blend(film, per[k][0], k), rcs.blend(film2, per[k][1], k)
        assert got.tobytes() == film.tobytes() and got2.tobytes() == film2.tobytes(), k


def test_scene_edge_cases(pt, gpu_ctx, cornell_arrays, free):
    """after pt_scene_update REFIT == a fresh scene of the moved arrays; one triangle at n = 65; NEE on a box whose faces all have Ke = 0 ==
    the wavefront form (no light to sample: no shadow ray in either)"""
    v, i, f = cornell_arrays
    v2 = tc.move_short_box(v)
    kw = dict(seeds=False, spp=free.spp, max_depth=free.depth)
    F = pt.RADIANCE_FUSED
    scene, fresh = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v2, i, f)
    q = Call(pt, gpu_ctx, free.rays)
    try:
        before = q.run(scene, flags=F, **kw).copy()
        assert before.tobytes() == free.mean.tobytes()
        scene.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
        after, want = q.run(scene, flags=F, **kw).copy(), q.run(fresh, **kw).copy()
        assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()
        assert q.run(fresh, flags=F, **kw).tobytes() == want.tobytes()
    finally:
        scene.close(); fresh.close()
    # one triangle in front of the camera axis; rays 0 .. 64 of the free set plus the axis (ray 0) see it or the environment
    tri = np.asarray([-1, -2, 0, 1, -2, 0, 0, 0.5, 0], f32)
    one = pt.Scene(gpu_ctx, tri, np.arange(3, dtype=np.uint32), np.asarray([0.5, 0.6, 0.7, 0.0, 0.0, 0.0], f32))
    try:
        for nee in (False, True):
            gpu_ctx.reset_stats()
            want = q.run(one, 65, flags=_flags(pt, nee, 0), **kw).copy()
            rays = gpu_ctx.stats().rays
            gpu_ctx.reset_stats()
            got = q.run(one, 65, flags=_flags(pt, nee), **kw)
            assert got.tobytes() == want.tobytes() and gpu_ctx.stats().rays == rays and gpu_ctx.stats().pipeline == pt.PIPELINE_FUSED
        assert (want != np.asarray(rcs.ENV, f32)).any(1).sum() >= 1            # (the axis ray hits the triangle)
    finally:
        one.close()
    dark_f = np.array(f, f32).reshape(-1, 6).copy()
    dark_f[:, 3:] = 0.0
    dark = pt.Scene(gpu_ctx, v, i, dark_f.reshape(-1))
    try:
        gpu_ctx.reset_stats()
        want = q.run(dark, flags=pt.RADIANCE_NEE, **kw).copy()
        rays = gpu_ctx.stats().rays
        gpu_ctx.reset_stats()
        got = q.run(dark, flags=_flags(pt, True), **kw)
        assert got.tobytes() == want.tobytes() and gpu_ctx.stats().rays == rays == int(free.traced.sum())
    finally:
        dark.close(); q.close()


@pytest.fixture(scope="module")
def other_scenes(pt, gpu_ctx, cornell_arrays):
    inst = pt.Scene(gpu_ctx, *cornell_arrays)
    inst.set_instances(tc.INSTANCES)
    soup = pt.Scene(gpu_ctx, *rcs.soup_arrays())
    yield {"instances": inst, "soup": soup}
    inst.close(); soup.close()


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_auto(pt, orc, gpu_ctx, cornell_gpu, cornell_arrays, other_scenes, free, free_call, nee):
    """PT_RADIANCE_AUTO on the box: the form the measurements chose ran, and the answer is the oracle's; on the 3-instance scene, the soup, with
    extend = HBM and with tmin = 0 the wavefront form ran, with the bits of the call without flags"""
    cam = rcs.box_camera(orc, cornell_arrays)
    q = Call(pt, gpu_ctx, cam.rays, cam.seeds)
    try:
        gpu_ctx.reset_stats()
        got = q.run(cornell_gpu, spp=1, max_depth=cam.depth, flags=_flags(pt, nee, pt.RADIANCE_AUTO))
        st = gpu_ctx.stats()
        assert got.tobytes() == cam.want[int(nee)].tobytes() and st.rays == cam.n_rays[int(nee)]
        assert st.pipeline == (pt.PIPELINE_FUSED if AUTO_TAKES_FUSED[int(nee)] else _nee_pipeline(pt, nee)), st.pipeline
    finally:
        q.close()
    kw = dict(seeds=False, spp=free.spp, max_depth=free.depth)
    cases = [(other_scenes["instances"], {}), (other_scenes["soup"], {}), (cornell_gpu, dict(extend=pt.EXTEND_HBM)), (cornell_gpu, dict(tmin=0.0))]
    for k, (scene, more) in enumerate(cases):
        gpu_ctx.reset_stats()
        want = free_call.run(scene, flags=_flags(pt, nee, 0), **kw, **more).copy()
        base = gpu_ctx.stats()
        gpu_ctx.reset_stats()
        got = free_call.run(scene, flags=_flags(pt, nee, pt.RADIANCE_AUTO), **kw, **more)
        st = gpu_ctx.stats()
        assert got.tobytes() == want.tobytes(), k
        assert st.pipeline == _nee_pipeline(pt, nee) and st.rays == base.rays and st.launches_shade == base.launches_shade == free.depth, k


def test_refusals(pt, gpu_ctx, cornell_gpu, other_scenes, free, free_call):
    """both form bits together: PT_ERR_INVALID_ARG; PT_RADIANCE_FUSED on the soup, on the 3-instance scene, with extend = PT_EXTEND_HBM or _LDS, or
    with tmin = 0: PT_ERR_UNSUPPORTED -- nothing launched, the canary-filled outputs untouched, and the next good call works"""
    q, lib = free_call, pt.lib_amd()

    def desc(**kw):
        d = pt.radiance_default_desc()
        d.d_rays6, d.d_seeds, d.d_radiance, d.d_moment2 = q.rays.ptr, q.seeds.ptr, q.out.ptr, q.m2.ptr
        d.spp, d.max_depth, d.flags = free.spp, free.depth, pt.RADIANCE_FUSED
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    q.canary()
    gpu_ctx.reset_stats()
    both = pt.RADIANCE_FUSED | pt.RADIANCE_AUTO
    assert lib.pt_radiance_device(cornell_gpu.h, C.byref(desc(flags=both)), free.n, None) == INVALID
    assert lib.pt_radiance_device(cornell_gpu.h, C.byref(desc(flags=both | pt.RADIANCE_NEE)), free.n, None) == INVALID
    assert lib.pt_radiance_device(cornell_gpu.h, C.byref(desc(flags=pt.RADIANCE_FUSED | 4)), free.n, None) == INVALID      # (4 stays no flag)
    for nee in (0, pt.RADIANCE_NEE):
        F = pt.RADIANCE_FUSED | nee
        assert lib.pt_radiance_device(other_scenes["soup"].h, C.byref(desc(flags=F)), free.n, None) == UNSUPPORTED
        assert b"LDS" in lib.pt_last_error(gpu_ctx.h)
        assert lib.pt_radiance_device(other_scenes["instances"].h, C.byref(desc(flags=F)), free.n, None) == UNSUPPORTED
        assert b"single-level" in lib.pt_last_error(gpu_ctx.h)
        assert lib.pt_radiance_device(cornell_gpu.h, C.byref(desc(flags=F, extend=pt.EXTEND_HBM)), free.n, None) == UNSUPPORTED
        assert lib.pt_radiance_device(cornell_gpu.h, C.byref(desc(flags=F, extend=pt.EXTEND_LDS)), free.n, None) == UNSUPPORTED
        assert lib.pt_radiance_device(cornell_gpu.h, C.byref(desc(flags=F, tmin=0.0)), free.n, None) == UNSUPPORTED
        assert b"tmin" in lib.pt_last_error(gpu_ctx.h)
    gpu_ctx.sync()
    st = gpu_ctx.stats()
    assert (st.launches_extend, st.launches_shade, st.launches_other, st.rays, st.paths) == (0, 0, 0, 0, 0) and q.untouched()
    assert q.run(cornell_gpu, spp=free.spp, max_depth=free.depth, flags=pt.RADIANCE_FUSED).tobytes() == free.mean.tobytes()


def test_workspace(pt, cornell_arrays, free):
    """on a fresh context: a fused call holds exactly 16 B per slot of its chunk + the counters; a second call allocates nothing; a larger chunk grows
    it once; the 132-B-per-slot set appears only with a wavefront-form call; a chunk beyond mem_budget_mb is PT_ERR_OOM with nothing written, and a
    smaller chunk_rays then works"""
    ctx = pt.Context(0)
    scene = pt.Scene(ctx, *cornell_arrays)
    q = Call(pt, ctx, free.rays)
    kw = dict(seeds=False, spp=free.spp, max_depth=free.depth)
    F = pt.RADIANCE_FUSED
    big = None
    try:
        assert ctx.radiance_workspace_bytes() == 0
        assert q.run(scene, chunk_rays=64, flags=F, **kw).tobytes() == free.mean.tobytes()
        held = ctx.radiance_workspace_bytes()
        assert held == 16 * 64 * 3 + COUNT_BYTES, held
        assert q.run(scene, chunk_rays=33, flags=F | pt.RADIANCE_NEE, **kw) is not None and ctx.radiance_workspace_bytes() == held
        assert q.run(scene, flags=F, **kw).tobytes() == free.mean.tobytes()                     # the automatic chunk: 257 rays rounded up to 64
        grown = ctx.radiance_workspace_bytes()
        assert grown == 16 * 320 * 3 + COUNT_BYTES, grown
        q.run(scene, chunk_rays=64, flags=F, **kw)
        assert ctx.radiance_workspace_bytes() == grown                                          # it never shrinks
        assert q.run(scene, **kw).tobytes() == free.mean.tobytes()                              # the wavefront form: its own set, now
        assert ctx.radiance_workspace_bytes() == grown + 320 * 3 * 132 + 16 + 4
        # 32 768 rays x 3 samples x 16 B = 1.5 MiB of accumulators: beyond a budget of 1 MiB
        n_big = 32768
        big = Call(pt, ctx, np.ascontiguousarray(np.tile(free.rays, (128, 1))[:n_big]), np.tile(free.seeds, (128, 1))[:n_big])
        old = ctx.set_tuning(mem_budget_mb=1)
        try:
            with pytest.raises(pt.PtError) as e:
                big.run(scene, spp=free.spp, max_depth=free.depth, flags=F)
            assert e.value.status == OOM and big.untouched()
            got = big.run(scene, spp=free.spp, max_depth=free.depth, flags=F, chunk_rays=1024)
            assert got.tobytes() == np.tile(free.mean, (128, 1))[:n_big].tobytes()
            assert ctx.radiance_workspace_bytes() <= 1 << 20
        finally:
            ctx.set_tuning(**old)
    finally:
        if big is not None:
            big.close()
        q.close(); scene.close(); ctx.close()


def test_radiance_tensors_forms(pt, cornell_gpu, free):
    """the torch wrapper: form="fused" and form="auto" equal form="wavefront" on 257 rays, radiance and second moment"""
    import torch
    rays = torch.from_numpy(free.rays).to(torch.device("cuda", 0))
    kw = dict(spp=free.spp, max_depth=free.depth, moment2=True)
    want, want2 = cornell_gpu.radiance_tensors(rays, form="wavefront", **kw)
    assert want.cpu().numpy().tobytes() == free.mean.tobytes()
    for form in ("fused", "auto"):
        for nee in (False, True):
            ref = (want, want2) if not nee else cornell_gpu.radiance_tensors(rays, nee=True, **kw)
            got, got2 = cornell_gpu.radiance_tensors(rays, form=form, nee=nee, **kw)
            assert torch.equal(got, ref[0]) and torch.equal(got2, ref[1]), (form, nee)
    with pytest.raises(ValueError):
        cornell_gpu.radiance_tensors(rays, form="persistent", **kw)
