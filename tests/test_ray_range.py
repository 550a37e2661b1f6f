"""The ends of a ray's range on every traversal kernel (include/pt_api.h: a triangle counts with tmin < t < upper, strictly; an any-hit query's
upper end is the ray's own bound and desc.tmax plays no part in it; a NEE shadow ray's range is (tmin, 0.999 dist) whatever tmax is).  Hits placed
exactly ON either end, one ulp to either side, per-ray bounds beyond the call's tmax, and a render whose tmax cuts inside the scene -- every
comparison is bytes against the CPU oracle's.  tests/range_cases.py has the recipes and the oracle's answers (computed once per session);
tests/test_ray_range_cpu.py holds their premises on the oracle alone, and the tests here assert them again."""
import numpy as np
import pytest

import range_cases as rc
import trace_device_cases as tc
from trace_fused_cases import Query, check_closest

f32 = np.float32
MISS = tc.MISS
pytestmark = pytest.mark.gpu


def _any_both_tmax(q, scene, case, what, **kw):
    """per-ray bounds: d_occluded == the oracle's bytes under desc.tmax = 10000 and again under desc.tmax = 1.0 (bounds beyond the call's tmax)"""
    wrong = []
    for tmax in rc.CALL_TMAX:
        o = q.any(scene, case.n, tmax=tmax, **kw)
        bad = np.flatnonzero(o != case.occ)
        if len(bad):
            wrong.append(("desc.tmax", tmax, "rays", len(bad), "per kind", {rc.KIND_NAMES[k]: int((case.kind[bad] == k).sum()) for k in sorted(set(case.kind[bad].tolist()))},
                          [(int(i), float(case.bounds[i]), float(case.hits["t"][i]), int(o[i])) for i in bad[:4]]))
    assert not wrong, (what, wrong)


# ---- 1. any-hit bound edges, per-ray d_tmax ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box(orc, cornell_arrays):
    case = rc.box_case(orc, cornell_arrays)
    case.premises()
    return case


@pytest.fixture(scope="module")
def box_query(pt, gpu_ctx, box):
    q = Query(pt, gpu_ctx, box.rays, box.bounds)
    yield q
    q.close()


@pytest.mark.parametrize("extend", ["AUTO", "LDS", "HBM"])
def test_any_box_queue(pt, cornell_gpu, box, box_query, extend):
    _any_both_tmax(box_query, cornell_gpu, box, extend, extend=getattr(pt, "EXTEND_" + extend))


def test_any_box_trace_auto(pt, gpu_ctx, cornell_gpu, box, box_query):
    """PT_TRACE_AUTO on the box (the single-kernel form where the table takes it)"""
    _any_both_tmax(box_query, cornell_gpu, box, "PT_TRACE_AUTO", flags=pt.TRACE_AUTO)


@pytest.mark.parametrize("form", ["queue", "fused"])
@pytest.mark.parametrize("leaves", ["pairs", "pair_leaves_0", "pair_kernel_0"])
def test_any_box_leaf_forms(pt, gpu_ctx, cornell_arrays, cornell_gpu, box, box_query, leaves, form):
    """the default box (fan-pair leaves), a box created under pair_leaves = 0 and the default box walked under pair_kernel = 0 (leaves of up to
    four), through the queue form and through PT_TRACE_FUSED"""
    old, scene = {}, cornell_gpu
    if leaves == "pair_leaves_0":
        was = gpu_ctx.set_tuning(pair_leaves=0)
        try:
            scene = pt.Scene(gpu_ctx, *cornell_arrays)
        finally:
            gpu_ctx.set_tuning(**was)
    elif leaves == "pair_kernel_0":
        old = gpu_ctx.set_tuning(pair_kernel=0)
    try:
        _any_both_tmax(box_query, scene, box, (leaves, form), flags=pt.TRACE_FUSED if form == "fused" else 0)
        if form == "fused":
            assert gpu_ctx.stats().pipeline == pt.PIPELINE_FUSED
    finally:
        gpu_ctx.set_tuning(**old)
        if scene is not cornell_gpu:
            scene.close()


def test_any_soup(pt, orc, gpu_ctx):
    """the soup walked out of L2: AUTO, the BVH4 kernel by name, and the 8-wide tree"""
    case = rc.soup_case(orc)
    case.premises()
    scene = pt.Scene(gpu_ctx, *rc.soup_arrays())
    q = Query(pt, gpu_ctx, case.rays, case.bounds)
    try:
        for name in ("AUTO", "HBM", "HBM8"):
            _any_both_tmax(q, scene, case, name, extend=getattr(pt, "EXTEND_" + name))
    finally:
        q.close(); scene.close()


@pytest.mark.parametrize("knobs", [{}, {"inst16": 0}], ids=["default", "inst16_off"])
def test_any_instanced_box(pt, orc, gpu_ctx, cornell_arrays, knobs):
    """both two-level kernels"""
    case = rc.inst_case(orc, cornell_arrays)
    case.premises()
    old = gpu_ctx.set_tuning(**knobs)
    scene = pt.Scene(gpu_ctx, *cornell_arrays)
    q = Query(pt, gpu_ctx, case.rays, case.bounds)
    try:
        scene.set_instances(tc.INSTANCES)
        _any_both_tmax(q, scene, case, str(knobs))
    finally:
        q.close(); scene.close()
        gpu_ctx.set_tuning(**old)


@pytest.mark.parametrize("form", ["queue", "fused"])
def test_any_six_triangles(pt, orc, gpu_ctx, six_gpu, form):
    """the smallest scene of the suite (section 4's), whose walk is hardly more than its root"""
    case = rc.six_case(orc)
    case.premises()
    q = Query(pt, gpu_ctx, case.rays, case.bounds)
    try:
        _any_both_tmax(q, six_gpu, case, form, flags=pt.TRACE_FUSED if form == "fused" else 0)
    finally:
        q.close()


# ---- 2. and 3.: the bundle, whose rays share their t bit for bit --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundle(orc, cornell_arrays):
    b = rc.bundle(orc, cornell_arrays)
    assert [len(ix) for _, ix in b.groups] == [c for _, c in rc.BUNDLE_GROUPS]
    return b


@pytest.fixture(scope="module")
def bundle_query(pt, gpu_ctx, bundle):
    q = Query(pt, gpu_ctx, bundle.rays, np.zeros(bundle.n, f32))
    yield q
    q.close()


@pytest.mark.parametrize("form", ["queue", "fused"])
def test_uniform_bound_on_the_bundle(pt, cornell_gpu, bundle, bundle_query, form):
    """d_tmax NULL and desc.tmax = each group's t, nextup(t), nextdown(t): the bytes of the group's rays (and of every other ray) are the oracle's"""
    flags = pt.TRACE_FUSED if form == "fused" else 0
    for g, (t, ix) in enumerate(bundle.groups):
        for name, want_group in (("t", 0), ("up", 1), ("down", 0)):
            b, want = bundle.uniform[g, name]
            assert (want[ix] == want_group).all()
            o = bundle_query.any(cornell_gpu, bundle.n, per_ray=False, tmax=b, flags=flags)
            assert (o[ix] == want[ix]).all(), (form, g, name, int((o[ix] != want[ix]).sum()), len(ix))
            assert (o == want).all(), (form, g, name, np.flatnonzero(o != want)[:8])


def _check_end(b, g, name, got, what):
    lo, hi, hits, surface = b.ends[g, name]
    h, s = got
    if h is not None:
        assert h.tobytes() == hits.tobytes(), (what, g, name, np.flatnonzero(h != hits)[:6])
    for k, a in s.items():
        assert a.tobytes() == surface[k].tobytes(), (what, g, name, rc_plane(k))


def rc_plane(k):
    return ("position", "normal", "albedo", "emission")[k]


ENDS = ("tmax=t", "tmax=up", "tmin=down", "tmin=t")


@pytest.mark.parametrize("extend", ["AUTO", "LDS", "HBM"])
def test_closest_ends_scene_trace_and_queue(pt, cornell_gpu, bundle, bundle_query, extend):
    """tmax in {t, nextup(t)} and tmin in {nextdown(t), t} per group: pt_trace's records, and pt_trace_device's records and surface planes in the
    queue form, are the oracle's byte for byte"""
    ext = getattr(pt, "EXTEND_" + extend)
    for g in range(len(bundle.groups)):
        for name in ENDS:
            lo, hi, hits, _ = bundle.ends[g, name]
            got = cornell_gpu.trace(bundle.rays, tmin=lo, tmax=hi, extend=ext)
            assert got.tobytes() == hits.tobytes(), ("pt_trace", extend, g, name, np.flatnonzero(got != hits)[:6])
            _check_end(bundle, g, name, bundle_query.closest(cornell_gpu, bundle.n, tmin=lo, tmax=hi, extend=ext), "queue " + extend)


@pytest.mark.parametrize("leaves", ["pairs", "pair_leaves_0"])
def test_closest_ends_trace_fused(pt, gpu_ctx, cornell_arrays, cornell_gpu, bundle, bundle_query, leaves):
    """... and under PT_TRACE_FUSED, with fan-pair leaves and with leaves of up to four"""
    scene = cornell_gpu
    if leaves == "pair_leaves_0":
        was = gpu_ctx.set_tuning(pair_leaves=0)
        try:
            scene = pt.Scene(gpu_ctx, *cornell_arrays)
        finally:
            gpu_ctx.set_tuning(**was)
    try:
        for g in range(len(bundle.groups)):
            for name in ENDS:
                lo, hi, _, _ = bundle.ends[g, name]
                _check_end(bundle, g, name, bundle_query.closest(scene, bundle.n, tmin=lo, tmax=hi, flags=pt.TRACE_FUSED), "fused " + leaves)
        assert gpu_ctx.stats().pipeline == pt.PIPELINE_FUSED
    finally:
        if scene is not cornell_gpu:
            scene.close()


# ---- 4. next-event estimation under a tmax inside the scene -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six_gpu(pt, gpu_ctx):
    sc = pt.Scene(gpu_ctx, *rc.six_arrays())
    yield sc
    sc.close()


@pytest.mark.parametrize("tmax", [rc.SIX_TMAX, 10000.0], ids=["tmax_2", "tmax_10000"])
@pytest.mark.parametrize("pipeline", ["wavefront_nee", "fused_nee"])
def test_nee_render_under_tmax(pt, orc, gpu_ctx, six_gpu, pipeline, tmax):
    """two frames of the six-triangle scene: the film and the ray count (shadow rays included) are the oracle's nee mode's, bit for bit -- at
    tmax = 2.0 every light sample's occluder lies BEYOND tmax and before 0.999 dist (tests/test_ray_range_cpu.py); tmax = 10000 is the control"""
    want, rays = rc.six_film(orc, 2, tmax)
    assert want.mean() > 0.3
    kw = dict(rc.SIX_RENDER, frame=0, frame_count=2, tmax=tmax)
    if pipeline == "wavefront_nee":
        kw.update(pipeline=pt.PIPELINE_WAVEFRONT_NEE)
    else:
        kw.update(pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_NEE)
    film = pt.Film(gpu_ctx, kw["width"], kw["height"])
    try:
        gpu_ctx.reset_stats()
        pt.render(six_gpu, film, pt.default_params(**kw))
        st = gpu_ctx.stats()
        got = film.read_f32()
        assert st.pipeline == kw["pipeline"]
        print(pipeline, tmax, "pixels that differ", int((got != want).any(2).sum()), "of", want.shape[0] * want.shape[1], "means", float(got.mean()), float(want.mean()),
              "rays", st.rays, rays)
        assert got.tobytes() == want.tobytes(), (int((got != want).any(2).sum()), float(got.mean()), float(want.mean()))
        assert st.rays == rays, (st.rays, rays)
    finally:
        film.close()


@pytest.mark.parametrize("tmax", [rc.SIX_TMAX, 10000.0], ids=["tmax_2", "tmax_10000"])
@pytest.mark.parametrize("form", ["queue", "fused"])
def test_nee_radiance_device_under_tmax(pt, orc, gpu_ctx, six_gpu, form, tmax):
    """pt_radiance_device with PT_RADIANCE_NEE, fed the camera's rays and advanced seeds at 1 spp: == the oracle's frame 0 and its ray count"""
    rays, seeds = rc.six_camera(orc)
    want, n_rays = rc.six_film(orc, 1, tmax, spp_per_frame=1)
    want = np.ascontiguousarray(want.reshape(-1, 3))
    n = len(rays)
    bufs = [pt.DeviceBuffer(gpu_ctx, a.nbytes) for a in (rays, seeds)] + [pt.DeviceBuffer(gpu_ctx, 12 * n + 64)]
    try:
        bufs[0].write(rays); bufs[1].write(seeds)
        bufs[2].write(np.full(12 * n + 64, 0xEE, np.uint8))
        gpu_ctx.reset_stats()
        six_gpu.radiance_device(n, bufs[0].ptr, bufs[2].ptr, seeds_ptr=bufs[1].ptr, spp=1, max_depth=rc.SIX_RENDER["max_depth"], tmax=tmax,
                                flags=pt.RADIANCE_NEE | (pt.RADIANCE_FUSED if form == "fused" else 0))
        raw = bufs[2].read(np.uint8, 12 * n + 64)
        assert (raw[12 * n:] == 0xEE).all()
        got = raw[:12 * n].view(f32).reshape(n, 3)
        print(form, tmax, "rays that differ", int((got != want).any(1).sum()), "of", n, "means", float(got.mean()), float(want.mean()), "rays", gpu_ctx.stats().rays, n_rays)
        assert got.tobytes() == want.tobytes(), (int((got != want).any(1).sum()), float(got.mean()), float(want.mean()))
        assert gpu_ctx.stats().rays == n_rays, (gpu_ctx.stats().rays, n_rays)
    finally:
        for b in bufs:
            b.close()
