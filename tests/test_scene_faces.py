"""pt_scene_set_faces / pt_scene_set_faces_device / pt_scene_read_faces (include/pt_api.h): new per-face materials for a
scene's triangles without a rebuild.  Bar: after the call the scene is, bit for bit, a scene created with the new faces that took the same
later calls -- checked against the CPU oracle of (vertices, indices, NEW faces) on every pipeline, against a FRESH scene of the new faces, and
against a twin that took the other form of the call.  Every face array is built by numpy from a fixed seed and its emitter count is asserted."""
import numpy as np
import pytest

from test_scene_update import KW, W, H, _cases, _check_pipelines, _deform, _mode, _oracle, _rays, _render, _soup
from test_scene_device import CAM16, _big_soup, _dev, _info, _one_emissive_triangle, _same_state
from trace_device_cases import surface_oracle

pytestmark = pytest.mark.gpu
f32 = np.float32
# the eight edge values of tests/scene_faces_host.cpp: 0, -0.0, a denormal, 1e-38, a negative, 3e38, +inf, NaN
EDGE = np.array([0.0, -0.0, 1.4e-45, 1e-38, -0.75, 3e38, np.inf, np.nan], f32)


def _emitters(f):
    return int((np.asarray(f, f32).reshape(-1, 6)[:, 3:] != 0).any(1).sum())


def _moved(f, seed=101, floor_ke=(8.0, 6.0, 4.0)):
    """The Cornell box's materials with its emitters moved: the ceiling light (the last two triangles) dark, the two floor triangles (the
    first two) emitting floor_ke, a new Kd on every triangle of the two boxes (triangles 10 .. n - 3)."""
    rng = np.random.default_rng(seed)
    fn = np.array(f, f32).reshape(-1, 6).copy()
    assert _emitters(fn) == 2 and (fn[-2:, 3:] != 0).any(1).all()
    fn[-2:, 3:] = 0
    fn[:2, 3:] = f32(floor_ke)
    fn[10:-2, :3] = rng.uniform(0.1, 0.9, (len(fn) - 12, 3)).astype(f32)
    assert _emitters(fn) == 2
    return fn.reshape(-1)


def _set(scene, fn, form):
    if form == "host":
        scene.set_faces(fn)
    else:
        import torch
        scene.set_faces_tensor(torch.from_numpy(np.ascontiguousarray(fn, f32).reshape(-1)).cuda())


def _films_equal(pt, ctx, a, b, pipelines, what="", **kw):
    for pipeline, flags in pipelines:
        x, y = _render(pt, ctx, a, 2, pipeline, flags, **kw), _render(pt, ctx, b, 2, pipeline, flags, **kw)
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2], (what, pipeline, flags)


def _bvh_bytes(scene):
    out = [a.tobytes() for a in scene.read_bvh()] + [scene.read_bvh4().tobytes()]
    if scene.info().n_tris > 1:
        out += [a.tobytes() for a in scene.read_bvh8()]
    return out


# ---- 1. the Cornell box, emitters moved ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["host", "tensor"])
def test_cornell_emitters_moved(pt, orc, gpu_ctx, cornell_arrays, form):
    v, i, f = cornell_arrays
    fn = _moved(f)
    gs = pt.Scene(gpu_ctx, v, i, f)
    old = _render(pt, gpu_ctx, gs, 2, pt.PIPELINE_AUTO)
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE)       # (the old emitter set has been sampled)
    trees, build_ms = _bvh_bytes(gs), gs.info().build_ms
    assert gs.read_faces().tobytes() == np.asarray(f, f32).tobytes()
    _set(gs, fn, form)
    new = _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn, _cases(pt))
    assert new[0].tobytes() != old[0].tobytes()
    assert gs.read_faces().tobytes() == fn.tobytes()
    assert _bvh_bytes(gs) == trees and gs.info().build_ms == build_ms       # the trees are not touched
    fresh = pt.Scene(gpu_ctx, v, i, fn)
    assert _info(gs) == _info(fresh)
    fresh.close(); gs.close()


def test_host_and_device_forms_leave_twins_in_the_same_state(pt, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    fn = _moved(f, seed=102)
    a, b = pt.Scene(gpu_ctx, v, i, f), pt.Scene.from_tensors(gpu_ctx, *_dev(v, i, f))
    _set(a, fn, "host"); _set(b, fn, "tensor")
    _same_state(a, b, "host / tensor")
    assert a.read_faces().tobytes() == b.read_faces().tobytes() == fn.tobytes()
    _films_equal(pt, gpu_ctx, a, b, [(pt.PIPELINE_AUTO, 0), (pt.PIPELINE_WAVEFRONT_NEE, 0), (pt.PIPELINE_FUSED, pt.FLAG_NEE)], "twins")
    # mixed freely: the other form on each, back to the first materials
    _set(a, f, "tensor"); _set(b, f, "host")
    _same_state(a, b, "mixed")
    _films_equal(pt, gpu_ctx, a, b, [(pt.PIPELINE_WAVEFRONT_NEE, 0)], "mixed")
    b.close(); a.close()


# ---- 2. emitter counts across the fold's edges and across zero -------------------------------------------------------------------------------

def _soup_faces(n, count, seed):
    rng = np.random.default_rng(seed)
    fn = rng.uniform(0, 1, (n, 6)).astype(f32)
    fn[:, 3:] = 0
    lit = rng.choice(n, count, replace=False)
    fn[lit, 3:] = rng.uniform(0.5, 4, (count, 3)).astype(f32)
    assert _emitters(fn) == count
    return fn.reshape(-1)


def test_emitter_counts_across_the_fold_edges_and_zero(pt, orc, gpu_ctx):
    """> 2048 triangles (the big-scene tables, the 8-wide ones built first): one scene whose emitter set shrinks, empties, grows from empty,
    crosses the single-wave boundary of the fold (64 / 65) and grows back."""
    v, i, f = _big_soup()
    n = len(i) // 3
    assert n == 3000 and 250 < _emitters(f) < 350
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.read_bvh8()
    assert gs.info().n_wide8_nodes > 0
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE)
    nee = [(pt.PIPELINE_WAVEFRONT_NEE, 0, True)]
    for step, count in enumerate((300, 0, 1, 64, 65, 300)):
        fn = _soup_faces(n, count, 200 + step)
        gs.set_faces(fn)
        _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn, nee)        # (count 0: the oracle's nee mode on a scene with no emitter)
        assert gs.read_faces().tobytes() == fn.tobytes()
    for ext in (pt.EXTEND_HBM, pt.EXTEND_HBM8, pt.EXTEND_AUTO):
        _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn, [(pt.PIPELINE_WAVEFRONT, 0, False)], extend=ext)
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn, nee, extend=pt.EXTEND_HBM8)     # the 8-wide tables' emission words
    gs.close()


# ---- 3. what later calls build from the kept state -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("later", ["quality", "refit", "rebuild", "refit_tensors"])
def test_later_calls_build_from_the_new_materials(pt, orc, gpu_ctx, cornell_arrays, later):
    v, i, f = cornell_arrays
    fn = _moved(f, seed=103)
    v2 = _deform(v, 51)
    gs, fresh = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v, i, fn)
    gs.set_faces(fn)
    if later == "quality":
        for q in (pt.BVH_PREFER_FAST_BUILD, pt.BVH_PREFER_FAST_TRACE):
            gs.set_bvh_quality(q); fresh.set_bvh_quality(q)
            _same_state(gs, fresh, (later, q))
            _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn, _cases(pt))
    else:
        for s in (gs, fresh):
            if later == "refit_tensors":
                s.update_tensors(*_dev(v2, i), mode=pt.SCENE_UPDATE_REFIT)
            else:
                s.update(v2, i, mode=_mode(pt, later))
        _same_state(gs, fresh, later)
        _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, fn, _cases(pt))
    assert gs.read_faces().tobytes() == fn.tobytes()
    fresh.close(); gs.close()


def test_device_ids_do_not_outlive_their_emitter_set(pt, orc, gpu_ctx, cornell_arrays):
    """A scene made from host arrays uploads its emitters' ids at its first device update.  Host set_faces with another emitter set in
    between: the next device update must compute its records from the NEW set's ids."""
    v, i, f = cornell_arrays
    fn = _moved(f, seed=104)
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.update_tensors(*_dev(_deform(v, 52), i))          # ids of triangles n-2, n-1 are on the device now
    gs.set_faces(fn)                                     # the emitters are triangles 0, 1
    v2 = _deform(v, 53)
    gs.update_tensors(*_dev(v2, i))
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, fn, _cases(pt)[2:])
    gs.update(v, i)                                      # ... and the host update's loop reads the new ids and Ke too
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn, _cases(pt)[2:])
    gs.close()


# ---- 4. instanced ----------------------------------------------------------------------------------------------------------------------------

def test_instanced_scene_drops_its_world_space_emitters(pt, orc, gpu_ctx, cornell_arrays):
    import torch
    v, i, f = cornell_arrays
    grid = pt.cornell_grid_instances()[:16]
    cases = [(pt.PIPELINE_AUTO, 0, False), (pt.PIPELINE_WAVEFRONT, 0, False), (pt.PIPELINE_WAVEFRONT_NEE, 0, True)]
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.set_instances(grid)
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE, **CAM16)       # the world-space copies of the OLD emitters exist
    fn = _moved(f, seed=105)
    gs.set_faces(fn)
    assert gs.info().n_instances == 16
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn, cases, instances=grid, **CAM16)
    # the set kept in device memory: its copies are made by a kernel
    gs.set_instances_tensor(torch.from_numpy(np.ascontiguousarray(grid, f32).reshape(-1)).cuda())
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE, **CAM16)
    fn2 = _moved(f, seed=106, floor_ke=(3.0, 5.0, 9.0))
    fn2.reshape(-1, 6)[-1, 3:] = f32([17, 12, 4])                         # three emitters now: the count changes as well
    assert _emitters(fn2) == 3
    _set(gs, fn2, "tensor")
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn2, cases, instances=grid, **CAM16)
    gs.close()


# ---- 5. the readers of the kept copy ---------------------------------------------------------------------------------------------------------

def _aov(pt, ctx, scene, call, **kw):
    film = pt.Film(ctx, W, H)
    film.enable_aov()
    call(scene, film, pt.default_params(frame=0, frame_count=2, **dict(KW, **kw)))
    out = {k: film.read_aov(k).tobytes() for k in range(pt.AOV_COUNT)}, film.read_f32().tobytes()
    film.close()
    return out


def test_readers_of_the_kept_materials(pt, orc, gpu_ctx, cornell_arrays):
    import torch
    v, i, f = cornell_arrays
    fn = _moved(f, seed=107)
    p = np.asarray(v, f32).reshape(-1, 3)
    rays = _rays(512, 54, p.min(0), p.max(0))
    tr = torch.from_numpy(rays).cuda()
    gs, fresh = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v, i, fn)

    def hits_of(out):
        got = np.zeros(len(rays), pt.HIT_DTYPE)
        got["prim"], got["inst"] = out["prim"].cpu().numpy().view(np.uint32), out["inst"].cpu().numpy().view(np.uint32)
        got["t"], got["u"], got["v"] = out["t"].cpu().numpy(), out["u"].cpu().numpy(), out["v"].cpu().numpy()
        return got
    before = hits_of(gs.trace_tensors(tr, surface=True))
    assert (before["prim"] != pt.MISS).mean() > 0.3
    gs.set_faces(fn)
    want = surface_oracle(orc.Scene(v, i, fn), fn, before)
    for form in ("queues", "fused"):
        out = gs.trace_tensors(tr, surface=True, form=form)
        assert hits_of(out).tobytes() == before.tobytes(), form
        for k, name in enumerate(("position", "normal", "albedo", "emission")):
            assert out[name].cpu().numpy().tobytes() == want[k].tobytes(), (form, name)
    assert want[3].any() and (want[2] != surface_oracle(orc.Scene(v, i, f), f, before)[2]).any()     # (the rays see what changed)
    # guide buffers: albedo and emission planes of the new materials; pt_render_guided = pt_render + pt_render_aov
    planes, _ = _aov(pt, gpu_ctx, gs, pt.render_aov)
    fplanes, _ = _aov(pt, gpu_ctx, fresh, pt.render_aov)
    assert planes == fplanes
    for pipeline in (pt.PIPELINE_AUTO, pt.PIPELINE_WAVEFRONT):
        gplanes, gfilm = _aov(pt, gpu_ctx, gs, pt.render_guided, pipeline=pipeline)
        assert gplanes == _aov(pt, gpu_ctx, fresh, pt.render_aov, pipeline=pipeline)[0], pipeline
        assert gfilm == _render(pt, gpu_ctx, fresh, 2, pipeline)[0].tobytes(), pipeline
    for form in ("wavefront", "fused"):
        for nee in (False, True):
            a = gs.radiance_tensors(tr, spp=4, max_depth=5, nee=nee, form=form)
            b = fresh.radiance_tensors(tr, spp=4, max_depth=5, nee=nee, form=form)
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and bool(a.any()), (form, nee)
    fresh.close(); gs.close()


# ---- 6. edge values --------------------------------------------------------------------------------------------------------------------------

def test_edge_values_are_taken_as_create_takes_them(pt, gpu_ctx, cornell_arrays):
    """Rows 0..7: an edge value in all of Kd; rows 8..15: in one component of Ke.  -0.0 and +0 emit nothing; the denormal, 1e-38, the
    negative, 3e38, +inf and NaN do: 6 emitters beside the ceiling light's 2."""
    v, i, f = cornell_arrays
    fn = np.array(f, f32).reshape(-1, 6).copy()
    for k in range(8):
        fn[k, :3] = EDGE[k]
        fn[8 + k, 3:] = 0
        fn[8 + k, 3 + k % 3] = EDGE[k]
    assert _emitters(fn) == 8
    fn = fn.reshape(-1)
    gs, fresh = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v, i, fn)
    gs.set_faces(fn)
    assert gs.read_faces().tobytes() == fn.tobytes()
    _films_equal(pt, gpu_ctx, gs, fresh, [(pt.PIPELINE_WAVEFRONT, 0), (pt.PIPELINE_AUTO, 0), (pt.PIPELINE_WAVEFRONT_NEE, 0)], "edges")
    twin = pt.Scene(gpu_ctx, v, i, f)
    _set(twin, fn, "tensor")
    _films_equal(pt, gpu_ctx, twin, fresh, [(pt.PIPELINE_WAVEFRONT, 0), (pt.PIPELINE_AUTO, 0)], "edges, device form")
    twin.close(); fresh.close(); gs.close()


# ---- 7. one triangle -------------------------------------------------------------------------------------------------------------------------

def test_one_triangle_becomes_an_emitter_and_back(pt, orc, gpu_ctx):
    v, i, lit = _one_emissive_triangle()
    dark = lit.copy()
    dark[3:] = 0
    assert (_emitters(dark), _emitters(lit)) == (0, 1)
    gs = pt.Scene(gpu_ctx, v, i, dark)
    for fn in (lit, dark, lit):
        gs.set_faces(fn)
        _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn, _cases(pt)[2:])
    gs.close()


# ---- 8. refusals and atomicity ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_scene_alone(pt, orc, gpu_ctx, cornell_arrays):
    import torch
    v, i, f = cornell_arrays
    f = np.ascontiguousarray(f, f32)
    fn = _moved(f, seed=108)
    fn.reshape(-1, 6)[4, 3:] = 1.0                     # (three emitters: the count changes too)
    assert _emitters(fn) == 3
    nt = len(i) // 3
    gs = pt.Scene(gpu_ctx, v, i, f)
    before = _render(pt, gpu_ctx, gs, 2, pt.PIPELINE_AUTO)
    before_nee = _render(pt, gpu_ctx, gs, 2, pt.PIPELINE_WAVEFRONT_NEE)
    L = pt.lib_amd()
    tf = torch.from_numpy(fn).cuda()
    torch.cuda.synchronize()

    def unchanged(what):
        assert gs.read_faces().tobytes() == f.tobytes(), what
        assert _render(pt, gpu_ctx, gs, 2, pt.PIPELINE_AUTO)[0].tobytes() == before[0].tobytes(), what
    for call, ptr in ((L.pt_scene_set_faces, fn.ctypes.data), (L.pt_scene_set_faces_device, tf.data_ptr())):
        for args in ((None, nt), (ptr, nt - 1), (ptr, nt + 1), (ptr, 0)):
            assert call(gs.h, *args) == 1, args
            unchanged(args)
        assert call(None, ptr, nt) == 1
    assert L.pt_scene_read_faces(gs.h, None) == 1 and L.pt_scene_read_faces(None, fn.ctypes.data) == 1
    with pytest.raises(pt.PtError) as e:
        gs.set_faces(fn[:-6])
    assert e.value.status == 1
    with pytest.raises(ValueError):
        gs.set_faces_tensor(tf[:-6])
    unchanged("wrappers")
    # the new emitter set cannot be allocated: PT_ERR_OOM, the old materials render on; the same call repeated succeeds
    for form in ("host", "tensor"):
        old = gpu_ctx.set_tuning(fail_rebuild=1)
        try:
            with pytest.raises(pt.PtError) as e:
                _set(gs, fn, form)
            assert e.value.status == 4
        finally:
            gpu_ctx.set_tuning(**old)
        unchanged("oom " + form)
        assert _render(pt, gpu_ctx, gs, 2, pt.PIPELINE_WAVEFRONT_NEE)[0].tobytes() == before_nee[0].tobytes()
    gs.set_faces(fn)
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, fn, _cases(pt))
    gs.close()


def test_a_broken_scene_refuses_and_works_after_the_repair(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    f = np.ascontiguousarray(f, f32)
    fn = _moved(f, seed=109)
    v2 = _deform(v, 55)
    gs = pt.Scene(gpu_ctx, v, i, f)
    old = gpu_ctx.set_tuning(fail_rebuild=1)
    try:
        with pytest.raises(pt.PtError) as e:
            gs.update(v2, i, mode=pt.SCENE_UPDATE_REBUILD)
        assert e.value.status == 4 and gs.info().n_wide_nodes == 0
    finally:
        gpu_ctx.set_tuning(**old)
    for form in ("host", "tensor"):
        with pytest.raises(pt.PtError) as e:
            _set(gs, fn, form)
        assert e.value.status == 5 and "lost its acceleration structure" in str(e.value)
        assert gs.info().n_wide_nodes == 0                                   # still broken: the refusal repaired nothing
        assert gs.read_faces().tobytes() == f.tobytes()                      # (the kept copy answers for a broken scene)
    gs.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)                             # the repair
    gs.set_faces(fn)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, fn, _cases(pt))
    gs.close()


# ---- 9. ordering -----------------------------------------------------------------------------------------------------------------------------

def test_set_faces_is_ordered_after_an_async_render(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    fn = _moved(f, seed=110)
    gs = pt.Scene(gpu_ctx, v, i, f)
    film = pt.Film(gpu_ctx, W, H)
    pt.render(gs, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_WAVEFRONT, flags=pt.FLAG_ASYNC, **KW))
    gs.set_faces(fn)                                     # no sync in between
    gpu_ctx.sync()
    want, wbgra, _ = _oracle(orc, orc.Scene(v, i, f), 2, **KW)
    assert film.read_f32().tobytes() == want.tobytes() and film.read_bgra8().tobytes() == wbgra.tobytes()
    film.close()
    new, nbgra, _ = _oracle(orc, orc.Scene(v, i, fn), 2, **KW)
    got = _render(pt, gpu_ctx, gs, 2, pt.PIPELINE_WAVEFRONT)
    assert got[0].tobytes() == new.tobytes() and got[1].tobytes() == nbgra.tobytes() and new.tobytes() != want.tobytes()
    gs.close()
