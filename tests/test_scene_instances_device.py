"""pt_scene_set_instances_device (include/pt_api.h): instance matrices handed over in device memory.  Bar: the scene is
in the state pt_scene_set_instances leaves with a host copy of the same bytes -- every comparison here is bit for bit, against a TWIN scene
that took set_instances(t.cpu().numpy()) of the same tensor, and, where test_scene_update._check_pipelines has it, against the CPU oracle."""
import numpy as np
import pytest

import trace_device_cases as tdc
from test_scene_device import CAM16, _dev, _info
from test_scene_update import KW, W, H, _check_pipelines, _deform, _mode, _rays, _render

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = [1, 2, 3, 63, 64, 65, 257]          # the wave and block edges of a one-thread-per-instance kernel
RAY_BOX = (f32([-4.0, -3.0, -2.0]), f32([4.0, 1.0, 2.0]))
_sets = {}


def _generated(n, seed):
    """n matrices: a rotation times a non-uniform scale over 1e-3 .. 1e3; every fifth sheared, every seventh mirrored (negative determinant),
    every third axis-aligned with -0.0 off the diagonal; translations on a grid"""
    rng = np.random.default_rng(seed)
    m = np.zeros((n, 3, 4), np.float64)
    for k in range(n):
        a, b, c = rng.uniform(0, 2 * np.pi, 3)
        rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        s = 10.0 ** rng.uniform(-3, 3, 3)
        if k % 7 == 3:
            s[1] = -s[1]
        r = (rz @ ry @ rx) * s[None, :]
        if k % 5 == 2:
            r[:, 1] += 0.5 * r[:, 0]
        if k % 3 == 1:
            r = np.full((3, 3), -0.0)
            r[0, 0], r[1, 1], r[2, 2] = s
        m[k, :, :3] = r
        m[k, :, 3] = [-4 + 0.5 * (k % 17), -2 + 0.25 * ((k // 17) % 17), -0.0 if k % 2 else 0.125 * (k // 289)]
    return m.astype(f32)


def _matrices(n, seed=0):
    """The set of a shape, generated once and inspected on the CPU: every matrix passes the host call's two checks in numpy."""
    key = (n, seed)
    if key not in _sets:
        x = np.ascontiguousarray(tdc.INSTANCES[:n].reshape(n, 3, 4)) if n <= 3 and seed == 0 else _generated(n, 7000 + 31 * n + seed)
        assert x.dtype == f32 and x.shape == (n, 3, 4) and np.isfinite(x).all()
        for k in range(n):
            assert np.isfinite(tdc.invert_3x4(x[k])).all(), (n, k)
        if n >= 63:
            assert (np.linalg.det(x[:, :, :3].astype(np.float64)) < 0).any() and np.signbit(x[x == 0]).any()
        _sets[key] = x
    return _sets[key]


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, f32).reshape(-1)).cuda()


def _pair(pt, ctx, arrays):
    v, i, f = arrays
    return pt.Scene(ctx, v, i, f), pt.Scene(ctx, v, i, f)


def _set_both(gs, twin, x):
    t = _t(x)
    gs.set_instances_tensor(t)
    twin.set_instances(t.cpu().numpy())


def _pipelines(pt):
    return [(pt.PIPELINE_AUTO, 0), (pt.PIPELINE_WAVEFRONT, 0), (pt.PIPELINE_WAVEFRONT_NEE, 0), (pt.PIPELINE_AUTO, pt.FLAG_NEE)]


def _same_films(pt, ctx, gs, twin, what, pipelines=None, **kw):
    for pipeline, flags in pipelines or _pipelines(pt):
        a, b = _render(pt, ctx, gs, 1, pipeline, flags, **kw), _render(pt, ctx, twin, 1, pipeline, flags, **kw)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], (what, pipeline, flags)


def _same_traces(pt, gs, twin, what, surface=True):
    rays = _rays(512, 77, *RAY_BOX)
    a, b = gs.trace(rays), twin.trace(rays)
    assert a.tobytes() == b.tobytes(), what
    if surface:
        import torch
        rt = torch.from_numpy(rays).cuda()
        ta, tb = gs.trace_tensors(rt, surface=True), twin.trace_tensors(rt, surface=True)
        assert set(ta) == set(tb) and {"inst", "position", "normal", "albedo", "emission"} <= set(ta)
        for key in ta:
            assert ta[key].cpu().numpy().tobytes() == tb[key].cpu().numpy().tobytes(), (what, key)
    return a


def _aov_planes(pt, ctx, scene, motion=False):
    film = pt.Film(ctx, W, H)
    film.enable_aov()
    if motion:
        film.enable_motion()
    pt.render_aov(scene, film, pt.default_params(frame=0, frame_count=1, width=W, height=H, spp_per_frame=4))
    out = {which: film.read_aov(which) for which in pt.AOV_SHAPES}
    if motion:
        film.motion(scene)
        out["Q"] = film.read_motion()
        film.motion(scene)                       # a second call of the same set: nothing is copied again, the plane is the same
        assert film.read_motion().tobytes() == out["Q"].tobytes()
    film.close()
    return out


@pytest.mark.parametrize("n", SIZES)
def test_device_set_equals_the_host_set(pt, gpu_ctx, cornell_arrays, n):
    """info, films and ray counts on four pipelines, 512 traced rays with inst, the surface planes, the guide planes, and the Q plane of
    snapshot -> a device set of moved matrices -> render_aov -> motion."""
    gs, twin = _pair(pt, gpu_ctx, cornell_arrays)
    x = _matrices(n)
    _set_both(gs, twin, x)
    assert gs.info().n_instances == n and _info(gs) == _info(twin)
    _same_films(pt, gpu_ctx, gs, twin, n)
    hits = _same_traces(pt, gs, twin, n)
    assert (hits["prim"] != pt.MISS).any() and (n == 1 or len(np.unique(hits["inst"][hits["prim"] != pt.MISS])) > 1)
    a, b = _aov_planes(pt, gpu_ctx, gs), _aov_planes(pt, gpu_ctx, twin)
    for which in a:
        assert a[which].tobytes() == b[which].tobytes(), (n, which)
    # the instances move: the snapshot's matrices and the current ones both come from the device copy
    moved = x.copy()
    moved[:, :, 3] += f32([0.03, -0.02, 0.01])
    for s in (gs, twin):
        s.snapshot_previous()
    _set_both(gs, twin, moved)
    a, b = _aov_planes(pt, gpu_ctx, gs, motion=True), _aov_planes(pt, gpu_ctx, twin, motion=True)
    for which in a:
        assert a[which].tobytes() == b[which].tobytes(), (n, which)
    assert a["Q"][..., 3].any()
    twin.close(); gs.close()


def test_radiance_and_guided_renders_after_a_device_set(pt, gpu_ctx, cornell_arrays):
    """pt_radiance_device (with and without NEE: the instanced emitter table made from the device copy) and pt_render_guided on the twins."""
    import torch
    gs, twin = _pair(pt, gpu_ctx, cornell_arrays)
    _set_both(gs, twin, _matrices(65))
    rays = torch.from_numpy(_rays(512, 78, *RAY_BOX)).cuda()
    for nee in (False, True):
        a, b = gs.radiance_tensors(rays, spp=4, max_depth=4, nee=nee), twin.radiance_tensors(rays, spp=4, max_depth=4, nee=nee)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and bool(a.any()), nee
    out = []
    for s in (gs, twin):
        film = pt.Film(gpu_ctx, W, H)
        film.enable_aov()
        pt.render_guided(s, film, pt.default_params(frame=0, frame_count=2, **KW))
        out.append([film.read_f32()] + [film.read_aov(which) for which in pt.AOV_SHAPES])
        film.close()
    for x, y in zip(*out):
        assert x.tobytes() == y.tobytes()
    twin.close(); gs.close()


def test_device_set_of_the_grid_equals_the_oracle(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    grid = pt.cornell_grid_instances()[:16]
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.set_instances_tensor(_t(grid))
    assert gs.info().n_instances == 16
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, f, [(pt.PIPELINE_AUTO, 0, False), (pt.PIPELINE_WAVEFRONT, 0, False), (pt.PIPELINE_WAVEFRONT_NEE, 0, True)],
                     instances=grid, **CAM16)
    gs.close()


@pytest.mark.parametrize("n", [32767, 32768])
def test_the_edge_of_the_fp16_two_level_class(pt, gpu_ctx, cornell_arrays, n):
    gs, twin = _pair(pt, gpu_ctx, cornell_arrays)
    _set_both(gs, twin, _matrices(n))
    assert gs.info().n_instances == n and _info(gs) == _info(twin)
    hits = _same_traces(pt, gs, twin, n, surface=False)
    assert (hits["prim"] != pt.MISS).any()
    twin.close(); gs.close()


def test_host_and_device_sets_mix(pt, gpu_ctx, cornell_arrays):
    gs, twin = _pair(pt, gpu_ctx, cornell_arrays)
    a, b, c = _matrices(65), _matrices(64), _matrices(63, seed=1)
    gs.set_instances(a)
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE)           # (the first set's emitter copies exist)
    gs.set_instances_tensor(_t(b))
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE)
    gs.set_instances(c)
    for x in (a, b, c):
        twin.set_instances(x)
    assert _info(gs) == _info(twin)
    _same_films(pt, gpu_ctx, gs, twin, "host, device, host")
    _same_traces(pt, gs, twin, "host, device, host")
    # and motion across the kinds: a snapshot of a host set, then a device set; a snapshot of a device set, then a host set
    for first, second in ((False, True), (True, False)):
        planes = []
        for s, device in ((gs, True), (twin, False)):
            (s.set_instances_tensor(_t(c)) if device and first else s.set_instances(c))
            s.snapshot_previous()
            (s.set_instances_tensor(_t(b[:63])) if device and second else s.set_instances(b[:63]))
            planes.append(_aov_planes(pt, gpu_ctx, s, motion=True)["Q"])
        assert planes[0].tobytes() == planes[1].tobytes() and planes[0][..., 3].any(), (first, second)
    twin.close(); gs.close()


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("form", ["tensors", "host"])
def test_blas_update_after_a_device_set(pt, orc, gpu_ctx, cornell_arrays, mode, form):
    """The update sets the instances again from the scene's device copy: n_instances is kept and the oracle's film comes out."""
    v, i, f = cornell_arrays
    grid = pt.cornell_grid_instances()[:16]
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.set_instances_tensor(_t(grid))
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE, **CAM16)      # world-space emitters / frames of the old BLAS exist
    v2 = _deform(v, 51)
    if form == "tensors":
        gs.update_tensors(*_dev(v2, i), mode=_mode(pt, mode))
    else:
        gs.update(v2, i, mode=_mode(pt, mode))
    assert gs.info().n_instances == 16
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_AUTO, 0, False), (pt.PIPELINE_WAVEFRONT, 0, False),
                                                      (pt.PIPELINE_WAVEFRONT_NEE, 0, True)], instances=grid, **CAM16)
    gs.close()


@pytest.mark.parametrize("way_out", ["set_bvh_quality", "render"])
def test_failed_update_keeps_a_device_set_parked(pt, orc, gpu_ctx, cornell_arrays, way_out):
    """test_scene_update's failed rebuild of an instanced scene, the set given in device memory: every way out brings the 16 instances back."""
    v, i, f = cornell_arrays
    grid = pt.cornell_grid_instances()[:16]
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.set_instances_tensor(_t(grid))
    v2 = _deform(v, 52)
    old = gpu_ctx.set_tuning(fail_rebuild=1)
    try:
        with pytest.raises(pt.PtError) as e:
            gs.update(v2, i, mode=pt.SCENE_UPDATE_REBUILD)
        assert e.value.status == 4
    finally:
        gpu_ctx.set_tuning(**old)
    if way_out == "set_bvh_quality":
        gs.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)
        assert gs.info().n_instances == 16
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_WAVEFRONT, 0, False), (pt.PIPELINE_WAVEFRONT_NEE, 0, True)], instances=grid, **CAM16)
    assert gs.info().n_instances == 16
    gs.close()


def test_device_set_of_a_scene_made_from_tensors(pt, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs, twin = pt.Scene.from_tensors(gpu_ctx, *_dev(v, i, f)), pt.Scene(gpu_ctx, v, i, f)
    _set_both(gs, twin, _matrices(65))
    assert _info(gs) == _info(twin)
    _same_films(pt, gpu_ctx, gs, twin, "from_tensors")
    twin.close(); gs.close()


def test_zero_instances_after_a_device_set(pt, gpu_ctx, cornell_arrays):
    import torch
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    rows, info0 = gs.read_bvh4().tobytes(), _info(gs)
    first = [_render(pt, gpu_ctx, gs, 1, p, fl) for p, fl in _pipelines(pt)]
    for empty in (torch.zeros(0, dtype=torch.float32, device="cuda"), None):
        gs.set_instances_tensor(_t(_matrices(65)))
        assert gs.info().n_instances == 65
        if empty is None:
            gs.set_instances_device(None, 0)
        else:
            gs.set_instances_tensor(empty)
        assert gs.read_bvh4().tobytes() == rows and _info(gs) == info0
        for (p, fl), want in zip(_pipelines(pt), first):
            got = _render(pt, gpu_ctx, gs, 1, p, fl)
            assert got[0].tobytes() == want[0].tobytes() and got[2] == want[2], (p, fl)
    gs.close()


def _refusals(n):
    """(name, instances changed, message): argument checks -- every value is read from the caller's n matrices, nothing out of range is passed"""
    nan, inf, mid, last = f32(np.nan), f32(np.inf), n // 2, n - 1

    def put(i, r, c, val):
        return lambda x: x.__setitem__((i, r, c), val)

    def zero_row(x):
        x[mid, 1, :] = 0

    def equal_rows(x):
        x[last] = f32([[1, 2, 3, 0.5], [4, 5, 6, -1], [1, 2, 3, 2]])        # (small integers: the determinant is exactly 0)

    def tiny(x):
        x[0] = 0
        x[0, 0, 0] = x[0, 1, 1] = x[0, 2, 2] = f32(1e-39)                 # the inverse overflows binary32

    def nan_and_singular(x):
        x[7, 0, 2] = nan
        x[3, 0, :] = 0

    return [("nan first", put(0, 1, 1, nan), "instance matrix has a NaN/Inf"), ("nan middle", put(mid, 0, 0, nan), "instance matrix has a NaN/Inf"),
            ("nan last", put(last, 2, 3, nan), "instance matrix has a NaN/Inf"), ("inf", put(mid, 0, 3, inf), "instance matrix has a NaN/Inf"),
            ("zero row", zero_row, "instance matrix is singular"), ("equal rows", equal_rows, "instance matrix is singular"),
            ("scale 1e-39", tiny, "instance matrix is singular"), ("nan at 7, singular at 3", nan_and_singular, "instance matrix is singular")]


def test_refusals_are_the_host_calls(pt, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs, twin = _pair(pt, gpu_ctx, cornell_arrays)
    info0 = _info(gs)
    single = _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_AUTO)
    good = _matrices(65)
    L = pt.lib_amd()
    for name, change, message in _refusals(65):
        _set_both(gs, twin, good)                                          # a set the refused call drops
        bad = good.copy()
        change(bad)
        assert not np.array_equal(bad, good, equal_nan=True)
        t = _t(bad)
        with pytest.raises(pt.PtError) as e:
            gs.set_instances_tensor(t)
        with pytest.raises(pt.PtError) as eh:
            twin.set_instances(t.cpu().numpy())
        assert e.value.status == eh.value.status == 1 and message in str(e.value) and str(e.value) == str(eh.value), (name, str(e.value), str(eh.value))
        assert gs.info().n_instances == 0 and _info(gs) == _info(twin) == info0, name     # single-level, as the host call leaves it
        got = _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_AUTO)
        assert got[0].tobytes() == single[0].tobytes() and got[2] == single[2], name
    # NULL with n > 0, and a good call afterwards
    import torch
    torch.cuda.synchronize()
    assert L.pt_scene_set_instances_device(gs.h, None, 3) == 1 and b"null argument" in L.pt_last_error(gpu_ctx.h)
    _set_both(gs, twin, good)
    assert gs.info().n_instances == 65 and _info(gs) == _info(twin)
    _same_films(pt, gpu_ctx, gs, twin, "after the refusals", pipelines=_pipelines(pt)[1:3])
    twin.close(); gs.close()


def test_broken_scene_refuses_as_the_host_call(pt, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs, twin = _pair(pt, gpu_ctx, cornell_arrays)
    errs = []
    for s, device in ((gs, True), (twin, False)):
        old = gpu_ctx.set_tuning(fail_rebuild=1)
        try:
            with pytest.raises(pt.PtError):
                s.update(_deform(v, 53), i, mode=pt.SCENE_UPDATE_REBUILD)
        finally:
            gpu_ctx.set_tuning(**old)
        with pytest.raises(pt.PtError) as e:
            (s.set_instances_tensor(_t(_matrices(3))) if device else s.set_instances(_matrices(3)))
        errs.append((e.value.status, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == 5, errs                   # PT_ERR_UNSUPPORTED, PT_BROKEN_SCENE_MSG
    twin.close(); gs.close()


def test_device_set_is_ordered_after_an_async_render(pt, gpu_ctx, cornell_arrays):
    gs, twin = _pair(pt, gpu_ctx, cornell_arrays)
    grid = pt.cornell_grid_instances()[:16]
    gs.set_instances_tensor(_t(grid))
    twin.set_instances(grid)
    want = _render(pt, gpu_ctx, twin, 2, pt.PIPELINE_WAVEFRONT, **CAM16)
    film = pt.Film(gpu_ctx, W, H)
    other = _t(_matrices(65))
    pt.render(gs, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_WAVEFRONT, flags=pt.FLAG_ASYNC, **dict(KW, **CAM16)))
    gs.set_instances_tensor(other)                       # no sync in between
    gpu_ctx.sync()
    assert film.read_f32().tobytes() == want[0].tobytes() and film.read_bgra8().tobytes() == want[1].tobytes() and want[0].any()
    assert gs.info().n_instances == 65
    film.close(); twin.close(); gs.close()
