"""pt_crossings_device on the GPU (include/pt_api.h): crossing counts and winding for rays in device memory.  Bar: every
byte of both outputs equals the numpy float32 restatement of the definition, brute force over all triangles (tests/crossings_cases.py, computed
once per session, never from the library) -- for every form, prefix, bound, tuning knob, builder and after every scene change; canaries stay
intact beyond row n and in an output that was not named."""
import ctypes as C

import numpy as np
import pytest

import crossings_cases as cc
import ploc_ref as pr
import trace_device_cases as tc

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, UNSUPPORTED = 1, 5
FORMS = ("AUTO", "LDS", "GLOBAL")
PREFIXES = (1, 63, 64, 65, 1000)


class Query:
    """The device buffers of one ray set (pt_device_alloc: no torch needed) and pt_crossings_device calls over its prefixes.  Both outputs are
    filled with a canary (0xEE bytes) before every call and read back whole afterwards.  offset: bytes between the rows' allocation and their
    first row (a multiple of 4).  rows: [n, 6] rays, or [n, 3] origins (then every call names a direction)."""

    def __init__(self, pt, ctx, rows, bounds=None, offset=0):
        self.pt, self.n, self.points_form = pt, len(rows), rows.shape[1] == 3
        self.rows_buf = pt.DeviceBuffer(ctx, rows.nbytes + offset)
        self.rows_buf.write(np.concatenate([np.zeros(offset, np.uint8), np.ascontiguousarray(rows, f32).view(np.uint8).reshape(-1)]))
        self.rows_ptr = self.rows_buf.ptr + offset
        self.bounds = pt.DeviceBuffer(ctx, 4 * self.n)
        self.bounds.write(np.ascontiguousarray(np.full(self.n, np.inf, f32) if bounds is None else bounds, f32))
        self.count = pt.DeviceBuffer(ctx, 4 * self.n)
        self.winding = pt.DeviceBuffer(ctx, 4 * self.n)
        self.ms = 0.0

    def canary(self):
        for b in (self.count, self.winding):
            b.write(np.full(b.nbytes, 0xEE, np.uint8))

    def untouched(self):
        return all((b.read(np.uint8, b.nbytes) == 0xEE).all() for b in (self.count, self.winding))

    def run(self, scene, n, count=True, winding=True, per_ray=False, **kw):
        """-> (count [n] u32 or None, winding [n] i32 or None) of rays [0, n); asserts the canaries beyond row n and in an output not named"""
        self.canary()
        where = dict(points_ptr=self.rows_ptr) if self.points_form else dict(rays_ptr=self.rows_ptr)
        self.ms = scene.crossings_device(n, tmax_ptr=self.bounds.ptr if per_ray else None, count_ptr=self.count.ptr if count else None,
                                         winding_ptr=self.winding.ptr if winding else None, **where, **kw)
        out = []
        for buf, named, dt in ((self.count, count, np.uint32), (self.winding, winding, np.int32)):
            raw = buf.read(np.uint8, buf.nbytes)
            assert (raw[4 * n if named else 0:] == 0xEE).all(), "an output beyond row n / not named"
            out.append(raw[:4 * n].view(dt) if named else None)
        return tuple(out)

    def close(self):
        for b in (self.rows_buf, self.bounds, self.count, self.winding):
            b.close()


def check(ref, n, got, what):
    """a call's outputs against the restatement's, byte for byte"""
    count, winding = got
    if count is not None:
        bad = np.flatnonzero(count != ref.count[:n])
        assert count.tobytes() == ref.count[:n].tobytes(), (what, n, bad[:4], count[bad[:4]], ref.count[bad[:4]])
    if winding is not None:
        bad = np.flatnonzero(winding != ref.winding[:n])
        assert winding.tobytes() == ref.winding[:n].tobytes(), (what, n, bad[:4], winding[bad[:4]], ref.winding[bad[:4]])


@pytest.fixture(scope="module")
def box(cornell_arrays):
    return cc.box_set(cornell_arrays)


@pytest.fixture(scope="module")
def box_query(pt, gpu_ctx, box):
    q = Query(pt, gpu_ctx, box["free"].rays, bounds=box["cycled"].bounds)
    yield q
    q.close()


def _form(pt, name):
    return getattr(pt, "CROSSINGS_" + name)


def test_box_all_forms_all_prefixes(pt, gpu_ctx, cornell_arrays, cornell_gpu, box, box_query):
    """1. every prefix in {1, 63, 64, 65, 1 000} of the 1 000-ray set (camera-like, random interior, axis-aligned, through vertices, through and
    along shared edges, the grazing set) under AUTO, LDS and GLOBAL: both outputs, d_count alone and d_winding alone equal the restatement byte
    for byte (hence the forms each other); canaries intact beyond row n and in the output not named.  Then the d_points + direction form on the
    same origins."""
    ref, q = box["free"], box_query
    assert len(ref.rays) == 1000 and (np.bincount(ref.count, minlength=7)[:7] > 0).all()
    # the rows that answer 0 on the device too: all-zero directions (they walk; the kernel's short-division ray_setup gives NaN shears as the
    # IEEE form does) and rays with a NaN or an infinity, which the refill retires without a walk -- in the first wave, the second and the tail
    rows = list(cc.SPECIAL_ROWS)
    special = ref.rays[rows]
    assert ((special[:, 3:] == 0).all(1) | ~np.isfinite(special).all(1)).all() and (special[:, 3:] == 0).all(1).sum() == 3
    assert (ref.count[rows] == 0).all() and (ref.winding[rows] == 0).all()
    for n in PREFIXES:
        for name in FORMS:
            form = _form(pt, name)
            check(ref, n, q.run(cornell_gpu, n, form=form), name)
            check(ref, n, q.run(cornell_gpu, n, winding=False, form=form), name + " d_count alone")
            check(ref, n, q.run(cornell_gpu, n, count=False, form=form), name + " d_winding alone")
    d, pref = cc.box_points_set(cornell_arrays)
    qp = Query(pt, gpu_ctx, np.ascontiguousarray(pref.rays[:, :3]))
    try:
        for n in (65, 1000):
            for name in FORMS:
                check(pref, n, qp.run(cornell_gpu, n, direction=[float(c) for c in d], form=_form(pt, name)), "d_points, " + name)
    finally:
        qp.close()


@pytest.mark.parametrize("form", ["LDS", "GLOBAL"])
def test_bounds(pt, cornell_gpu, box, box_query, form):
    """2. per-ray bounds cycled from each ray's own sorted crossings -- t_k, nextup(t_k), nextdown(t_k) for k = first, second, last, then +inf,
    tmin, -1 and NaN -- with tmin = 0.001, and one uniform bound 2.5: the restatement's bytes; rays whose bound is tmin, -1 or NaN answer 0"""
    q, n = box_query, 1000
    cyc, uni = box["cycled"], box["uniform"]
    count, winding = q.run(cornell_gpu, n, per_ray=True, tmin=float(cc.TMIN_BOUNDS), form=_form(pt, form))
    check(cyc, n, (count, winding), "cycled")
    for k in (10, 11, 12):
        assert (count[k::13] == 0).all() and (winding[k::13] == 0).all()
    assert cyc.count.tobytes() != box["free_tmin"].count.tobytes()
    check(uni, n, q.run(cornell_gpu, n, tmin=float(cc.TMIN_BOUNDS), tmax=2.5, form=_form(pt, form)), "uniform")
    check(box["free_tmin"], n, q.run(cornell_gpu, n, tmin=float(cc.TMIN_BOUNDS), form=_form(pt, form)), "unbounded")
    # (per-ray bounds win over tmax, which then plays no part -- not even an invalid one)
    check(cyc, n, q.run(cornell_gpu, n, per_ray=True, tmin=float(cc.TMIN_BOUNDS), tmax=-1.0, form=_form(pt, form)), "cycled, tmax ignored")


@pytest.fixture(scope="module")
def soup(pt, gpu_ctx):
    (v, i, f), ref = cc.soup_set()
    scene = pt.Scene(gpu_ctx, v, i, f)
    q = Query(pt, gpu_ctx, ref.rays)
    yield scene, q, ref
    q.close(); scene.close()


def test_beyond_lds_and_the_spill_path(pt, gpu_ctx, cornell_gpu, box, box_query, soup):
    """3. tc.soup(4096, 11), 2 000 rays: AUTO (which runs GLOBAL) and GLOBAL equal the restatement; PT_CROSSINGS_LDS is PT_ERR_UNSUPPORTED --
    4096 x 48 B of triangles alone exceed 96 KB; the soup and the box again under pt_tuning.lds_stack = 1, where every lane spills: same bytes"""
    scene, q, ref = soup
    n = len(ref.rays)
    kw = dict(tmin=float(cc.TMIN_BOUNDS))
    assert scene.info().n_tris == 4096 and 4096 * 48 > 96 * 1024 and ref.count.max() >= 6
    check(ref, n, q.run(scene, n, form=pt.CROSSINGS_AUTO, **kw), "soup AUTO")
    check(ref, n, q.run(scene, n, form=pt.CROSSINGS_GLOBAL, **kw), "soup GLOBAL")
    q.canary()
    with pytest.raises(pt.PtError) as e:
        scene.crossings_device(n, rays_ptr=q.rows_ptr, count_ptr=q.count.ptr, winding_ptr=q.winding.ptr, form=pt.CROSSINGS_LDS)
    assert e.value.status == UNSUPPORTED and "PT_CROSSINGS_LDS" in str(e.value) and q.untouched()
    old = gpu_ctx.set_tuning(lds_stack=1)
    try:
        check(ref, n, q.run(scene, n, form=pt.CROSSINGS_GLOBAL, **kw), "soup, lds_stack = 1")
        for name in ("LDS", "GLOBAL"):
            check(box["free"], 1000, box_query.run(cornell_gpu, 1000, form=_form(pt, name)), "box, lds_stack = 1, " + name)
    finally:
        gpu_ctx.set_tuning(**old)


@pytest.fixture(scope="module")
def big(cornell_arrays):
    return cc.box_big(cornell_arrays)


@pytest.fixture(scope="module")
def one_block(pt, cornell_arrays, big):
    """a context with pt_tuning.extend_blocks = 1 (one block per CU), the box, and the big set's buffers"""
    ctx = pt.Context(0)
    ctx.set_tuning(extend_blocks=1)
    scene = pt.Scene(ctx, *cornell_arrays)
    q = Query(pt, ctx, big.rays)
    yield ctx, scene, q
    q.close(); scene.close(); ctx.close()


@pytest.mark.parametrize("form", ["LDS", "GLOBAL"])
@pytest.mark.parametrize("refill", [-1, 1, 64], ids=["refill_default", "refill_1", "refill_64"])
def test_persistent_loop_edges(pt, big, one_block, refill, form):
    """4. 200 001 rays through a grid of one block per CU: every wave draws from at least three strides of its private sequence and the last is
    ragged -- a second refill round, a partial final round and the drain; again refilling at one idle lane and only at 64"""
    ctx, scene, q = one_block
    old = ctx.set_tuning(refill=refill)
    try:
        ctx.reset_stats()
        check(big, cc.BIG_N, q.run(scene, cc.BIG_N, form=_form(pt, form)), form)
        assert ctx.stats().launches_other == 1 and ctx.stats().launches_extend == 0
    finally:
        ctx.set_tuning(**old)


def test_rows_four_byte_aligned(pt, gpu_ctx, cornell_gpu, box):
    """5. rows 4 bytes into their allocation (rows_ptr % 8 == 4), prefixes 65 and 1 000, both forms"""
    q = Query(pt, gpu_ctx, box["free"].rays, offset=4)
    try:
        assert q.rows_ptr % 8 == 4
        for n in (65, 1000):
            for name in ("LDS", "GLOBAL"):
                check(box["free"], n, q.run(cornell_gpu, n, form=_form(pt, name)), name)
    finally:
        q.close()


def test_tree_independence(pt, gpu_ctx, cornell_arrays, box, box_query):
    """6. the same bytes after set_bvh_quality(FAST_BUILD) (another tree); after a REFIT that enlarges the scene box, where pad changes, the
    bytes the restatement gives with the new pad (and other than before); back again; unchanged by set_faces; the same bytes on a scene made by
    pt_scene_create_device"""
    import torch
    v, i, f = cornell_arrays
    ref, q, n = box["free"], box_query, 1000
    v2, moved = cc.box_moved(cornell_arrays)
    assert moved.pad > ref.pad and moved.count.tobytes() != ref.count.tobytes()
    scene = pt.Scene(gpu_ctx, v, i, f)
    try:
        check(ref, n, q.run(scene, n), "fresh")
        scene.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
        assert max(np.abs(scene.info().bbox_min).max(), np.abs(scene.info().bbox_max).max()) * f32(3.814697265625e-06) == moved.pad
        for name in FORMS:
            check(moved, n, q.run(scene, n, form=_form(pt, name)), "after the refit, " + name)
        scene.update(v, i, mode=pt.SCENE_UPDATE_REFIT)
        check(ref, n, q.run(scene, n), "refit back")
        scene.set_faces(np.ascontiguousarray(np.asarray(f, f32).reshape(-1, 6)[::-1]).reshape(-1))
        check(ref, n, q.run(scene, n), "after set_faces")
        before = scene.read_bvh4().tobytes()
        scene.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)
        assert scene.read_bvh4().tobytes() != before   # (another tree)
        for name in FORMS:
            check(ref, n, q.run(scene, n, form=_form(pt, name)), "FAST_BUILD, " + name)
    finally:
        scene.close()
    dev = torch.device("cuda", 0)
    gs = pt.Scene.from_tensors(gpu_ctx, torch.from_numpy(np.asarray(v, f32).reshape(-1, 3)).to(dev), torch.from_numpy(np.asarray(i).astype(np.int32).reshape(-1, 3)).to(dev),
                               torch.from_numpy(np.asarray(f, f32).reshape(-1, 6)).to(dev))
    try:
        for name in FORMS:
            check(ref, n, q.run(gs, n, form=_form(pt, name)), "pt_scene_create_device, " + name)
    finally:
        gs.close()


def test_ploc_tree(pt, gpu_ctx):
    """6b. pt.make_stadium(24, 24), whose PLOC tree the library adopts: 600 rays from inside its box equal the restatement"""
    v, i, f = pr.arrays(pt, "stadium")
    tris = cc.triangles(v, i)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    rng = np.random.default_rng(91)
    d = rng.standard_normal((600, 3))
    rays = np.ascontiguousarray(np.concatenate([rng.uniform(lo, hi, (600, 3)), d / np.linalg.norm(d, axis=1)[:, None]], 1), f32)
    ref = cc.Brute(tris, rays)
    assert ref.phantoms.sum() == 0 and ref.count.max() >= 2
    scene = pt.Scene(gpu_ctx, v, i, f)
    q = Query(pt, gpu_ctx, rays)
    try:
        assert scene.info().bvh4_builder == 2
        for name in ("AUTO", "GLOBAL"):
            check(ref, 600, q.run(scene, 600, form=_form(pt, name)), "stadium, " + name)
    finally:
        q.close(); scene.close()


def test_against_trace_any(pt, gpu_ctx, cornell_gpu, box, soup):
    """7. (count > 0) == occluded from trace_tensors in any-hit mode, on the box's rays (per-ray bounds and a uniform one) and the soup's, with
    tmin = 0.001.  Rests on a premise test_crossings_cpu.py asserts: on these sets the own box drops no triangle that tri_test accepts."""
    import torch
    dev = torch.device("cuda", 0)
    tmin = float(cc.TMIN_BOUNDS)
    cyc = box["cycled"]
    rays = torch.from_numpy(cyc.rays).to(dev)
    bounds = cyc.bounds.copy()
    ok = ~np.isnan(bounds)                                    # (a NaN bound is outside pt_trace_device's contract)
    occ = cornell_gpu.trace_tensors(rays, tmax_per_ray=torch.from_numpy(bounds).to(dev), mode=pt.TRACE_ANY, tmin=tmin).cpu().numpy()
    count = cornell_gpu.crossings_tensors(rays=rays, tmax_per_ray=torch.from_numpy(bounds).to(dev), tmin=tmin).cpu().numpy()
    assert count.view(np.uint32).tobytes() == cyc.count.tobytes()
    # (non-finite rays and zero directions: pt_crossings_device defines their answer, 0; pt_trace_device's contract does not cover them)
    live = np.isfinite(cyc.rays).all(1) & (cyc.rays[:, 3:] != 0).any(1)
    assert (~live).sum() == len(cc.SPECIAL_ROWS) and (count[~live] == 0).all()
    assert ((count > 0) == occ)[ok & live].all() and 0 < occ[ok & live].sum() < (ok & live).sum()
    occ = cornell_gpu.trace_tensors(rays, mode=pt.TRACE_ANY, tmin=tmin, tmax=2.5).cpu().numpy()
    assert ((box["uniform"].count > 0) == occ)[live].all()
    scene, _, ref = soup
    # (the soup's reference is unbounded, pt_trace_device wants a finite tmax: 3e38, and no t of the set is anywhere near it)
    occ = scene.trace_tensors(torch.from_numpy(ref.rays).to(dev), mode=pt.TRACE_ANY, tmin=tmin, tmax=3.0e38).cpu().numpy()
    assert ((ref.count > 0) == occ).all() and 0 < occ.sum() < len(occ)


@pytest.mark.parametrize("name", ["cube", "sphere", "torus"])
def test_closed_meshes(pt, gpu_ctx, name):
    """8. inside_tensors equals the analytic answer on test_crossings_cpu.py's 1 000 points per mesh with the same caps (a single direction
    wrong on at most 1 %, three votes on none); each direction's parity is the restatement's on every point; signed_distance_tensors has the sign
    of the analytic distance, |sdf| == sqrt(dist2) of nearest_tensors bit for bit, NaN beyond max_dist"""
    import torch
    tris, pts, inside, sd = cc.closed_case(name)
    scene = pt.Scene(gpu_ctx, *cc.mesh_arrays(tris))
    try:
        dev = torch.device("cuda", 0)
        p = torch.from_numpy(pts).to(dev)
        dirs = np.asarray(pt.INSIDE_DIRECTIONS[:3], f32)
        votes = cc.inside_votes(tris, pts, dirs)
        for d, v in zip(pt.INSIDE_DIRECTIONS[:3], votes):
            got = scene.crossings_tensors(points=p, direction=d).cpu().numpy()
            assert ((got & 1).astype(bool) == v).all()
            assert ((got & 1).astype(bool) != inside).mean() <= 0.01
        assert (scene.inside_tensors(p, votes=1).cpu().numpy() == votes[0]).all()
        got = scene.inside_tensors(p).cpu().numpy()
        assert got.dtype == np.bool_ and (got == inside).all()
        sdf, prim, u, v = scene.signed_distance_tensors(p)
        near = scene.nearest_tensors(p)
        sdf = sdf.cpu().numpy()
        assert (np.signbit(sdf) == (sd < 0)).all() and not np.isnan(sdf).any()
        assert np.abs(sdf).tobytes() == torch.sqrt(near["dist2"]).cpu().numpy().tobytes() and torch.equal(prim, near["prim"])
        assert np.abs(np.abs(sdf) - np.abs(sd)).max() < 0.05          # (the polyhedron against the analytic solid: the chord sag)
        sdf2, prim2, _, _ = scene.signed_distance_tensors(p, max_dist=0.1)
        miss = prim2.cpu().numpy() < 0
        assert 0 < miss.sum() < len(pts) and np.isnan(sdf2.cpu().numpy()[miss]).all() and (sdf2.cpu().numpy()[~miss] == sdf[~miss]).all()
    finally:
        scene.close()


def test_refusals_and_stats(pt, gpu_ctx, cornell_arrays, cornell_gpu, box, box_query):
    """9. every refusal of the header, an instanced box included, leaves the canaries intact and launches nothing; a good call afterwards adds
    exactly 1 to launches_other and nothing to launches_extend, rays, paths; stats.pipeline and extend_variant stay; device_ms > 0; n == 0 is
    PT_OK with device_ms == 0"""
    q, lib, n = box_query, pt.lib_amd(), 257
    nan, inf = float("nan"), float("inf")

    def desc(**kw):
        d = pt.crossings_default_desc()
        d.d_rays6, d.d_count, d.d_winding = q.rows_ptr, q.count.ptr, q.winding.ptr
        for k, v in kw.items():
            if k.startswith("reserved"):
                d.reserved[int(k[8:])] = v
            elif k == "direction":
                d.direction = (C.c_float * 3)(*v)
            else:
                setattr(d, k, v)
        return d

    pts = dict(d_rays6=None, d_points=q.rows_ptr)
    cases = [(desc(d_rays6=None), INVALID), (desc(d_points=q.rows_ptr), INVALID), (desc(d_count=None, d_winding=None), INVALID),
             (desc(form=3), INVALID), (desc(form=0xFFFFFFFF), INVALID), (desc(flags=1), INVALID), (desc(flags=0x80000000), INVALID),
             (desc(reserved0=1), INVALID), (desc(reserved2=1), INVALID), (desc(tmin=nan), INVALID), (desc(tmin=inf), INVALID), (desc(tmin=-inf), INVALID),
             (desc(tmax=nan), INVALID), (desc(tmax=0.0), INVALID), (desc(tmin=1.0, tmax=1.0), INVALID), (desc(tmax=-1.0), INVALID),
             (desc(direction=(nan, 0, 1), **pts), INVALID), (desc(direction=(0, inf, 1), **pts), INVALID), (desc(direction=(0, 1, -inf), **pts), INVALID)]
    q.canary()
    gpu_ctx.sync()
    gpu_ctx.reset_stats()
    st0 = gpu_ctx.stats()
    ws = gpu_ctx.trace_workspace_bytes()
    for k, (d, want) in enumerate(cases):
        assert lib.pt_crossings_device(cornell_gpu.h, C.byref(d), n, None) == want, k
    assert lib.pt_crossings_device(None, C.byref(desc()), n, None) == INVALID and lib.pt_crossings_device(cornell_gpu.h, None, n, None) == INVALID
    # (a direction plays no part with d_rays6, tmax none with d_tmax: neither is judged then)
    assert lib.pt_crossings_device(cornell_gpu.h, C.byref(desc(direction=(nan, nan, nan))), 0, None) == 0
    inst = pt.Scene(gpu_ctx, *cornell_arrays)
    try:
        inst.set_instances(tc.INSTANCES)
        with pytest.raises(pt.PtError) as e:
            inst.crossings_device(n, rays_ptr=q.rows_ptr, count_ptr=q.count.ptr, winding_ptr=q.winding.ptr)
        assert e.value.status == UNSUPPORTED and "instance" in str(e.value) and "n = 0" in str(e.value), str(e.value)
        assert q.untouched()
        inst.set_instances(np.zeros((0, 12), f32))   # n = 0 instances restores the mesh
        check(box["free"], n, q.run(inst, n), "instances removed")
    finally:
        inst.close()
    q.canary()
    gpu_ctx.reset_stats()
    ms = C.c_float(-1.0)
    assert lib.pt_crossings_device(cornell_gpu.h, C.byref(desc()), 0, C.byref(ms)) == 0 and ms.value == 0.0        # n == 0
    assert lib.pt_crossings_device(cornell_gpu.h, C.byref(desc(d_rays6=None)), 0, C.byref(ms)) == 0                # ... which needs no rays
    gpu_ctx.sync()
    st = gpu_ctx.stats()
    assert (st.launches_extend, st.launches_other, st.rays, st.paths) == (0, 0, 0, 0) and q.untouched()
    check(box["free"], n, q.run(cornell_gpu, n), "after the refusals")
    st = gpu_ctx.stats()
    assert (st.launches_extend, st.launches_other, st.rays, st.paths) == (0, 1, 0, 0)
    assert (st.pipeline, st.extend_variant) == (st0.pipeline, st0.extend_variant)
    assert q.ms > 0 and gpu_ctx.trace_workspace_bytes() == ws


def test_crossings_tensors(pt, cornell_arrays, cornell_gpu, box):
    """10. the torch wrapper on non-contiguous views ([n, 6] rays and [n, 3] points cut out of wider tensors): form="lds", "global" and "auto"
    agree bit for bit with each other and with the restatement; winding on request; per-ray bounds and one bound; what it refuses"""
    import torch
    n = 1000
    ref = box["free"]
    dev = torch.device("cuda", 0)
    wide = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    wide[:, 1:7] = torch.from_numpy(ref.rays).to(dev)
    view = wide[:, 1:7]
    assert not view.is_contiguous()
    for form in ("lds", "global", "auto"):
        count, winding = cornell_gpu.crossings_tensors(rays=view, winding=True, form=form)
        assert count.dtype == torch.int32 and winding.dtype == torch.int32
        assert count.cpu().numpy().view(np.uint32).tobytes() == ref.count.tobytes() and winding.cpu().numpy().tobytes() == ref.winding.tobytes(), form
    count = cornell_gpu.crossings_tensors(rays=view)
    assert torch.is_tensor(count) and count.cpu().numpy().view(np.uint32).tobytes() == ref.count.tobytes()
    d, pref = cc.box_points_set(cornell_arrays)
    count = cornell_gpu.crossings_tensors(points=wide[:, 1:4], direction=[float(c) for c in d])
    assert count.cpu().numpy().view(np.uint32).tobytes() == pref.count.tobytes()
    tmin = float(cc.TMIN_BOUNDS)
    count = cornell_gpu.crossings_tensors(rays=view, tmax_per_ray=torch.from_numpy(box["cycled"].bounds).to(dev), tmin=tmin)
    assert count.cpu().numpy().view(np.uint32).tobytes() == box["cycled"].count.tobytes()
    count = cornell_gpu.crossings_tensors(rays=view, tmin=tmin, tmax=2.5)
    assert count.cpu().numpy().view(np.uint32).tobytes() == box["uniform"].count.tobytes()
    count, winding = cornell_gpu.crossings_tensors(rays=wide[:0, 1:7], winding=True)      # n == 0: empty tensors, no call
    assert count.shape == (0,) and winding.shape == (0,) and count.dtype == torch.int32
    assert cornell_gpu.inside_tensors(wide[:0, 1:4]).shape == (0,)
    for bad in (dict(rays=view, form="fused"), dict(), dict(rays=view, points=wide[:, 1:4]), dict(points=wide[:, 1:4]), dict(rays=wide[:, 1:4])):
        with pytest.raises(ValueError):
            cornell_gpu.crossings_tensors(**bad)
