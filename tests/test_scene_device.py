"""pt_scene_create_device / pt_scene_update_device (include/pt_api.h): geometry handed over in device memory.  Bar: the
scene is in the state the host call leaves with host copies of the same bytes -- every comparison here is bit for bit, against a TWIN scene
that took the host call with .cpu().numpy() of the same tensors, and against the CPU oracle of the new arrays."""
import ctypes as C

import numpy as np
import pytest

from test_scene_update import KW, W, H, _cases, _check_pipelines, _deform, _mode, _oracle, _quads_in_cornell, _rays, _render, _soup

pytestmark = pytest.mark.gpu
MODES = ["refit", "rebuild"]
CAM16 = dict(cam_origin=(-0.88, -1.9, 0.5), cam_target=(-0.88, -1.9, 0.0))


def _dev(v, i, f=None):
    """the arrays as CUDA tensors: float32, int32 (the u32 bits), float32"""
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1)).cuda(),
           torch.from_numpy(np.ascontiguousarray(i, np.uint32).reshape(-1).view(np.int32)).cuda()]
    if f is not None:
        out.append(torch.from_numpy(np.ascontiguousarray(f, np.float32).reshape(-1)).cuda())
    return out


def _info(scene):
    i = scene.info()
    return {name: (list(getattr(i, name)) if hasattr(getattr(i, name), "__len__") else getattr(i, name)) for name, _ in i._fields_ if name != "build_ms"}


def _same_state(a, b, what=""):
    """read_bvh, read_bvh4, read_bvh8 and every field of info() but build_ms"""
    for k, (x, y) in enumerate(zip(a.read_bvh(), b.read_bvh())):
        assert x.tobytes() == y.tobytes(), (what, "read_bvh", k)
    assert a.read_bvh4().tobytes() == b.read_bvh4().tobytes(), (what, "read_bvh4")
    if a.info().n_tris > 1:                 # (a single triangle has no 8-wide tree: pt_scene_read_bvh8 is PT_ERR_UNSUPPORTED)
        for k, (x, y) in enumerate(zip(a.read_bvh8(), b.read_bvh8())):
            assert x.tobytes() == y.tobytes(), (what, "read_bvh8", k)
    assert _info(a) == _info(b), (what, _info(a), _info(b))


def _big_soup():
    v, i, f = _soup(3000, 21, spread=0.05)     # test_refit_of_a_big_scene's: about 300 emitters, several 64-wide passes of the fold
    v = (v.reshape(-1, 3) * np.float32([0.9, 0.9, 0.9]) + np.float32([0, -1, 0])).reshape(-1).astype(np.float32)
    return v, i, f


@pytest.mark.parametrize("mode", MODES)
def test_cornell_device_update_equals_the_host_update(pt, orc, gpu_ctx, cornell_arrays, mode):
    v, i, f = cornell_arrays
    gs, twin = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v, i, f)
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_AUTO)
    v2 = _deform(v, 31)
    tv, ti = _dev(v2, i)
    gs.update_tensors(tv, ti, mode=_mode(pt, mode))
    twin.update(tv.cpu().numpy(), ti.cpu().numpy().view(np.uint32), mode=_mode(pt, mode))
    _same_state(gs, twin, mode)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt))       # (the NEE cases read the new emitter table)
    rays = _rays(512, 32, v2.reshape(-1, 3).min(0), v2.reshape(-1, 3).max(0))
    ohits, _ = orc.Scene(v2, i, f).trace(rays, mode=1)
    assert gs.trace(rays).tobytes() == ohits.tobytes() and (ohits["prim"] != pt.MISS).mean() > 0.3
    twin.close(); gs.close()


def test_device_refit_that_breaks_a_pair_leaf(pt, orc, gpu_ctx, cornell_arrays):
    """One quad's half pulled away: the device REFIT becomes a rebuild with the twin's bits; a pair-keeping shift stays a refit; and what
    set_bvh_quality builds afterwards from h_pair and the host boxes equals the twin's."""
    v, i, f, first = _quads_in_cornell(cornell_arrays)
    gs, twin = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v, i, f)
    v2 = np.array(v, np.float32).reshape(-1, 3).copy()
    second = first + 2 * 2 + 1
    v2[int(np.asarray(i)[3 * second])] += np.float32([0.0, -0.05, 0.08])
    v2 = v2.reshape(-1)
    gs.update_tensors(*_dev(v2, i), mode=pt.SCENE_UPDATE_REFIT)
    twin.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
    fresh = pt.Scene(gpu_ctx, v2, i, f)
    assert gs.read_bvh4().tobytes() == fresh.read_bvh4().tobytes()      # a rebuild: the fresh scene's rows, not the old topology
    _same_state(gs, twin, "pair break")
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt)[:2])
    v3 = (np.array(v2, np.float32).reshape(-1, 3) + np.float32([0.01, 0.02, -0.01])).reshape(-1).astype(np.float32)
    words = gs.read_bvh4()[:, 24:].copy()
    gs.update_tensors(*_dev(v3, i), mode=pt.SCENE_UPDATE_REFIT)
    twin.update(v3, i, mode=pt.SCENE_UPDATE_REFIT)
    assert (gs.read_bvh4()[:, 24:] == words).all()                      # a refit: the child words kept
    _same_state(gs, twin, "pair-keeping shift")
    _check_pipelines(pt, orc, gpu_ctx, gs, v3, i, f, _cases(pt)[:2])
    for q in (pt.BVH_PREFER_FAST_BUILD, pt.BVH_PREFER_FAST_TRACE):
        gs.set_bvh_quality(q); twin.set_bvh_quality(q)
        _same_state(gs, twin, q)
    # (FAST_TRACE after FAST_BUILD keeps the held surface-area tree; a rebuild at FAST_BUILD drops it, so the next one is made from h_pair / h_tlo)
    for s in (gs, twin):
        s.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)
    gs.update_tensors(*_dev(v3, i), mode=pt.SCENE_UPDATE_REBUILD)
    twin.update(v3, i, mode=pt.SCENE_UPDATE_REBUILD)
    for s in (gs, twin):
        s.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)
    _same_state(gs, twin, "surface-area tree from the refreshed pairs")
    fresh3 = pt.Scene(gpu_ctx, v3, i, f)
    assert gs.info().bvh4_builder == 1 and gs.read_bvh4().tobytes() == fresh3.read_bvh4().tobytes()
    _check_pipelines(pt, orc, gpu_ctx, gs, v3, i, f, _cases(pt)[:1])
    fresh3.close(); fresh.close(); twin.close(); gs.close()


def test_device_refit_of_a_big_scene(pt, orc, gpu_ctx):
    v, i, f = _big_soup()
    gs, twin = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v, i, f)
    assert 200 < int((f.reshape(-1, 6)[:, 3:] != 0).any(1).sum()) < 400
    gs.read_bvh8(); twin.read_bvh8()                     # the 8-wide nodes exist before the update
    rng = np.random.default_rng(22)
    v2 = (v.reshape(-1, 3) + rng.uniform(-0.03, 0.03, (len(v) // 3, 3)).astype(np.float32)).reshape(-1).astype(np.float32)
    gs.update_tensors(*_dev(v2, i), mode=pt.SCENE_UPDATE_REFIT)
    twin.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
    for x, y in zip(gs.read_bvh8(), twin.read_bvh8()):
        assert x.tobytes() == y.tobytes()
    _same_state(gs, twin, "big refit")
    for ext in (pt.EXTEND_HBM, pt.EXTEND_HBM8, pt.EXTEND_AUTO):
        _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_WAVEFRONT, 0, False)], extend=ext)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_WAVEFRONT_NEE, 0, True)])
    twin.close(); gs.close()


@pytest.mark.parametrize("mode", MODES)
def test_device_update_of_an_instanced_scene(pt, orc, gpu_ctx, cornell_arrays, mode):
    v, i, f = cornell_arrays
    grid = pt.cornell_grid_instances()[:16]
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.set_instances(grid)
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE, **CAM16)      # world-space emitters / frames of the old BLAS exist
    v2 = _deform(v, 36)
    gs.update_tensors(*_dev(v2, i), mode=_mode(pt, mode))
    assert gs.info().n_instances == 16
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_AUTO, 0, False), (pt.PIPELINE_WAVEFRONT, 0, False),
                                                      (pt.PIPELINE_WAVEFRONT_NEE, 0, True)], instances=grid, **CAM16)
    gs.close()


def test_mixed_host_and_device_updates_return_to_the_first_bits(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs, twin = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v, i, f)
    first = gs.read_bvh4().tobytes()
    v2, v3 = _deform(v, 37, jitter=0.02), _deform(v, 38, jitter=0.02)
    gs.update(v2, i)
    gs.update_tensors(*_dev(v3, i))
    gs.update(v, i)
    for x in (v2, v3, v):
        twin.update(x, i)
    _same_state(gs, twin, "host, device, host")
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, f, _cases(pt))
    gs.update_tensors(*_dev(v2, i), mode=pt.SCENE_UPDATE_REBUILD)
    gs.update_tensors(*_dev(v, i), mode=pt.SCENE_UPDATE_REBUILD)
    assert gs.read_bvh4().tobytes() == first
    twin.close(); gs.close()


def test_motion_after_a_device_update(pt, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    v2 = _deform(v, 39, jitter=0.0)
    planes = []
    for device in (True, False):
        sc = pt.Scene(gpu_ctx, v, i, f)
        film = pt.Film(gpu_ctx, W, H)
        film.enable_aov(); film.enable_motion()
        sc.snapshot_previous()
        if device:
            sc.update_tensors(*_dev(v2, i))
        else:
            sc.update(v2, i)
        pt.render_aov(sc, film, pt.default_params(frame=0, frame_count=1, width=W, height=H, spp_per_frame=4))
        film.motion(sc)
        planes.append(film.read_motion())
        film.close(); sc.close()
    assert planes[0].tobytes() == planes[1].tobytes() and planes[0][..., 3].any()


def test_device_update_is_ordered_after_an_async_render(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    film = pt.Film(gpu_ctx, W, H)
    tv, ti = _dev(_deform(v, 40, jitter=0.03), i)
    pt.render(gs, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_WAVEFRONT, flags=pt.FLAG_ASYNC, **KW))
    gs.update_tensors(tv, ti)                           # no sync in between
    gpu_ctx.sync()
    want, wbgra, _ = _oracle(orc, orc.Scene(v, i, f), 2, **KW)
    assert film.read_f32().tobytes() == want.tobytes() and film.read_bgra8().tobytes() == wbgra.tobytes()
    film.close(); gs.close()


def _one_emissive_triangle():
    v = np.float32([[-0.5, -0.5, 0.2], [0.5, -0.5, 0.2], [0.0, 0.5, 0.3]]).reshape(-1)
    return v, np.arange(3, dtype=np.uint32), np.float32([0.5, 0.6, 0.7, 3.0, 2.0, 1.0])


@pytest.mark.parametrize("which", ["cornell", "quads", "soup3000", "one_emissive_triangle", "no_emitters"])
def test_from_tensors_equals_the_host_scene(pt, gpu_ctx, cornell_arrays, which):
    """Read-backs, info, two frames of AUTO and of WAVEFRONT_NEE (a scene without emitters: NEE renders as the twin's does)."""
    if which == "cornell":
        v, i, f = cornell_arrays
    elif which == "quads":
        v, i, f, _ = _quads_in_cornell(cornell_arrays)
    elif which == "soup3000":
        v, i, f = _big_soup()
    elif which == "one_emissive_triangle":
        v, i, f = _one_emissive_triangle()
    else:
        v, i, f = cornell_arrays
        f = np.array(f, np.float32).reshape(-1, 6).copy()
        f[:, 3:] = 0
        f[::3, 3] = -0.0                                 # (-0.0 is no emission)
        f = f.reshape(-1)
    tv, ti, tf = _dev(v, i, f)
    gs = pt.Scene.from_tensors(gpu_ctx, tv, ti, tf)
    twin = pt.Scene(gpu_ctx, tv.cpu().numpy(), ti.cpu().numpy().view(np.uint32), tf.cpu().numpy())
    _same_state(gs, twin, which)
    for pipeline in (pt.PIPELINE_AUTO, pt.PIPELINE_WAVEFRONT_NEE):
        a, b = _render(pt, gpu_ctx, gs, 2, pipeline), _render(pt, gpu_ctx, twin, 2, pipeline)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], (which, pipeline)
        if which != "no_emitters":
            assert a[0].any()
    # a scene made from device arrays takes updates in either form
    v2 = (np.array(v, np.float32).reshape(-1, 3) + np.float32([0.01, -0.02, 0.005])).reshape(-1).astype(np.float32)
    gs.update(v2, i); twin.update_tensors(*_dev(v2, i))
    _same_state(gs, twin, which + " updated")
    a, b = _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE), _render(pt, gpu_ctx, twin, 1, pt.PIPELINE_WAVEFRONT_NEE)
    assert a[0].tobytes() == b[0].tobytes()
    twin.close(); gs.close()


def test_non_contiguous_and_wrong_tensors(pt, gpu_ctx, cornell_arrays):
    import torch
    v, i, f = cornell_arrays
    tv, ti, tf = _dev(v, i, f)
    wide = torch.zeros((tv.numel(), 2), dtype=torch.float32, device="cuda")
    wide[:, 0] = tv
    gs = pt.Scene.from_tensors(gpu_ctx, wide[:, 0], ti, tf)          # a strided view: made contiguous
    twin = pt.Scene(gpu_ctx, v, i, f)
    _same_state(gs, twin, "strided vertices")
    for bad in [(tv.double(), ti), (tv, ti.long()), (tv[:-1], ti), (tv.cpu(), ti), (tv, ti.cpu())]:
        with pytest.raises(ValueError):
            gs.update_tensors(*bad)
    with pytest.raises(ValueError):
        pt.Scene.from_tensors(gpu_ctx, tv, ti, tf[:-6])
    twin.close(); gs.close()


def test_device_refusals_leave_the_scene_alone(pt, orc, gpu_ctx, cornell_arrays):
    import torch
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    v2 = _deform(v, 41)
    nv, nt = len(v2) // 3, len(i) // 3
    # ONE SPARE ROW beyond n_verts: an index equal to n_verts names allocated memory, so even a build that gathered before it checked
    # would read nothing it may not.  This is a refusal test, not a fault test.
    tv = torch.zeros(3 * (nv + 1), dtype=torch.float32, device="cuda")
    tv[:3 * nv] = torch.from_numpy(np.ascontiguousarray(v2, np.float32))
    ti = _dev(v2, i)[1]
    L = pt.lib_amd()
    torch.cuda.synchronize()
    calls = [(tv.data_ptr(), nv, ti.data_ptr(), nt - 1, 0), (tv.data_ptr(), nv, ti.data_ptr(), nt - 1, 1),     # wrong n_tris, either mode
             (None, nv, ti.data_ptr(), nt, 0), (tv.data_ptr(), nv, None, nt, 0),                               # NULL arrays
             (tv.data_ptr(), nv, ti.data_ptr(), nt, 2),                                                        # an unknown mode
             (tv.data_ptr(), 0, ti.data_ptr(), nt, 0)]                                                         # no vertices
    for args in calls:
        assert L.pt_scene_update_device(gs.h, *args) == 1, args
    assert L.pt_scene_update_device(None, tv.data_ptr(), nv, ti.data_ptr(), nt, 0) == 1
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, f, _cases(pt)[:1])
    for where in (0, (3 * nt) // 2, 3 * nt - 1):                       # an index equal to n_verts: first, middle, last
        bad = ti.clone()
        bad[where] = nv
        torch.cuda.synchronize()
        for mode in (0, 1):
            assert L.pt_scene_update_device(gs.h, tv.data_ptr(), nv, bad.data_ptr(), nt, mode) == 1, (where, mode)
            assert b"vertex index out of range" in L.pt_last_error(gpu_ctx.h)
        with pytest.raises(pt.PtError) as e:
            gs.update_tensors(tv[:3 * nv], bad)
        assert e.value.status == 1
        _check_pipelines(pt, orc, gpu_ctx, gs, v, i, f, _cases(pt)[:2])    # still the old geometry
    neg = ti.clone()
    neg[7] = -1                                                          # int32 -1 is u32 0xFFFFFFFF: out of range
    with pytest.raises(pt.PtError) as e:
        gs.update_tensors(tv[:3 * nv], neg)
    assert e.value.status == 1
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, f, _cases(pt)[2:])
    gs.close()


def test_from_tensors_with_a_bad_index_leaks_nothing(pt, gpu_ctx, cornell_arrays):
    import torch
    v, i, f = cornell_arrays
    nv, nt = len(v) // 3, len(i) // 3
    ref = pt.Scene(gpu_ctx, v, i, f)
    info0, ws0 = _info(ref), gpu_ctx.stats().workspace_bytes
    ref.close()
    tv = torch.zeros(3 * (nv + 1), dtype=torch.float32, device="cuda")   # (one spare row, as above)
    tv[:3 * nv] = torch.from_numpy(np.ascontiguousarray(v, np.float32))
    _, ti, tf = _dev(v, i, f)
    for where in (0, (3 * nt) // 2, 3 * nt - 1):
        bad = ti.clone()
        bad[where] = nv
        with pytest.raises(pt.PtError) as e:
            pt.Scene.from_tensors(gpu_ctx, tv[:3 * nv], bad, tf)
        assert e.value.status == 1 and "vertex index out of range" in str(e.value)
        out = C.c_void_p(123)
        assert pt.lib_amd().pt_scene_create_device(gpu_ctx.h, tv.data_ptr(), nv, bad.data_ptr(), nt, tf.data_ptr(), C.byref(out)) == 1
        assert not out.value                                              # *out = NULL
    L = pt.lib_amd()
    out = C.c_void_p(123)
    for args in [(None, nv, ti.data_ptr(), nt, tf.data_ptr()), (tv.data_ptr(), nv, None, nt, tf.data_ptr()), (tv.data_ptr(), nv, ti.data_ptr(), nt, None),
                 (tv.data_ptr(), 0, ti.data_ptr(), nt, tf.data_ptr()), (tv.data_ptr(), nv, ti.data_ptr(), 0, tf.data_ptr()),
                 (tv.data_ptr(), nv, ti.data_ptr(), 1 << 28, tf.data_ptr())]:
        assert L.pt_scene_create_device(gpu_ctx.h, *args, C.byref(out)) == 1, args
    assert L.pt_scene_create_device(gpu_ctx.h, tv.data_ptr(), nv, ti.data_ptr(), nt, tf.data_ptr(), None) == 1
    after = pt.Scene(gpu_ctx, v, i, f)
    assert _info(after) == info0 and gpu_ctx.stats().workspace_bytes == ws0
    after.close()


def test_failed_device_rebuild_breaks_and_repairs(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    v2 = _deform(v, 42)
    old = gpu_ctx.set_tuning(fail_rebuild=1)
    try:
        with pytest.raises(pt.PtError) as e:
            gs.update_tensors(*_dev(v2, i), mode=pt.SCENE_UPDATE_REBUILD)
        assert e.value.status == 4
        assert gs.info().n_wide_nodes == 0
    finally:
        gpu_ctx.set_tuning(**old)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_WAVEFRONT, 0, False)])
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt)[2:])      # NEE: the emitter table is the new arrays'
    gs.close()
