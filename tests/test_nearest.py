"""pt_nearest_device on the GPU (include/pt_api.h): closest point on the mesh for points in device memory.  Bar: every byte
of both outputs equals the numpy float32 restatement of the definition, brute force over all triangles (tests/nearest_cases.py, computed once
per session, never from the library) -- for every form, prefix, radius, tuning knob, builder and after every scene change; canaries stay intact
beyond row n and in an output that was not named."""
import ctypes as C

import numpy as np
import pytest

import nearest_cases as nc
import trace_device_cases as tc

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, UNSUPPORTED = 1, 5
FORMS = ("AUTO", "LDS", "GLOBAL")


class Query:
    """The device buffers of one point set (pt_device_alloc: no torch needed) and pt_nearest_device calls over its prefixes.  Both outputs are
    filled with a canary (0xEE bytes) before every call and read back whole afterwards, as trace_fused_cases.Query does.  offset: bytes between
    the points' allocation and their first row (a multiple of 4)."""

    def __init__(self, pt, ctx, points, radii=None, offset=0):
        self.pt, self.n = pt, len(points)
        self.points_buf = pt.DeviceBuffer(ctx, points.nbytes + offset)
        self.points_buf.write(np.concatenate([np.zeros(offset, np.uint8), np.ascontiguousarray(points).view(np.uint8).reshape(-1)]))
        self.points_ptr = self.points_buf.ptr + offset
        self.radii = pt.DeviceBuffer(ctx, 4 * self.n)
        self.radii.write(np.ascontiguousarray(nc.cycled_radii(self.n) if radii is None else radii))
        self.nearest = pt.DeviceBuffer(ctx, 16 * self.n)
        self.point = pt.DeviceBuffer(ctx, 12 * self.n)
        self.ms = 0.0

    def canary(self):
        for b in (self.nearest, self.point):
            b.write(np.full(b.nbytes, 0xEE, np.uint8))

    def untouched(self):
        return all((b.read(np.uint8, b.nbytes) == 0xEE).all() for b in (self.nearest, self.point))

    def run(self, scene, n, nearest=True, point=True, per_query=False, **kw):
        """-> (records [n] or None, points [n, 3] or None) of queries [0, n); asserts the canaries beyond row n and in an output not named"""
        self.canary()
        self.ms = scene.nearest_device(n, self.points_ptr, max_dist_ptr=self.radii.ptr if per_query else None,
                                       nearest_ptr=self.nearest.ptr if nearest else None, point_ptr=self.point.ptr if point else None, **kw)
        raw = self.nearest.read(np.uint8, self.nearest.nbytes)
        assert (raw[16 * n if nearest else 0:] == 0xEE).all(), "d_nearest beyond row n / not named"
        rec = raw[:16 * n].view(nc.NEAREST_DTYPE) if nearest else None
        raw = self.point.read(np.uint8, self.point.nbytes)
        assert (raw[12 * n if point else 0:] == 0xEE).all(), "d_point beyond row n / not named"
        return rec, (raw[:12 * n].view(f32).reshape(n, 3) if point else None)

    def close(self):
        for b in (self.points_buf, self.radii, self.nearest, self.point):
            b.close()


def check(ref, n, got, what):
    """a call's outputs against the restatement's, byte for byte"""
    rec, point = got
    if rec is not None:
        assert rec.tobytes() == ref.rec[:n].tobytes(), (what, n, np.flatnonzero(rec != ref.rec[:n])[:4], rec[rec != ref.rec[:n]][:2], ref.rec[:n][rec != ref.rec[:n]][:2])
    if point is not None:
        assert point.tobytes() == ref.point[:n].tobytes(), (what, n, np.flatnonzero((point.view(np.uint32) != ref.point[:n].view(np.uint32)).any(1))[:4])


@pytest.fixture(scope="module")
def box(cornell_arrays):
    return nc.box_set(cornell_arrays)


@pytest.fixture(scope="module")
def box_query(pt, gpu_ctx, box):
    q = Query(pt, gpu_ctx, box["free"].points)
    yield q
    q.close()


def _form(pt, name):
    return getattr(pt, "NEAREST_" + name)


def test_box_all_forms_all_prefixes(pt, gpu_ctx, cornell_gpu, box, box_query):
    """1. every prefix of the 1 000-query set (uniform in 1.5x the box, surface points moved by +-1e-4 along the normal, all vertices, edge
    midpoints and centroids) under AUTO, LDS and GLOBAL: both outputs, d_nearest alone and d_point alone equal the restatement byte for byte
    (hence the forms each other); canaries intact beyond row n and in the output not named (Query asserts them)"""
    ref, q = box["free"], box_query
    assert len(ref.points) == 1000 and (ref.ties >= 2).sum() >= 50 and 0.05 < (ref.region == 6).mean() < 0.95
    for n in tc.PREFIXES:
        for name in FORMS:
            form = _form(pt, name)
            check(ref, n, q.run(cornell_gpu, n, form=form), name)
            check(ref, n, q.run(cornell_gpu, n, point=False, form=form), name + " d_nearest alone")
            check(ref, n, q.run(cornell_gpu, n, nearest=False, form=form), name + " d_point alone")


@pytest.mark.parametrize("form", ["LDS", "GLOBAL"])
def test_radii(pt, cornell_gpu, box, box_query, form):
    """2. the per-query radii cycled through 0, 1e-3, 0.1, +inf, -1, NaN, and one uniform max_dist = 0.1: the restatement's bytes, the miss
    record {0xFFFFFFFF, +0, +0, +0} and the +0.0 point among them"""
    q, n = box_query, 1000
    cyc, uni = box["cycled"], box["uniform"]
    rec, point = q.run(cornell_gpu, n, per_query=True, form=_form(pt, form))
    check(cyc, n, (rec, point), "cycled")
    miss = ~cyc.found
    assert miss[4::6].all() and miss[5::6].all() and 0 < miss[1::6].sum() < len(miss[1::6])
    assert (rec.view(np.uint32).reshape(n, 4)[miss] == [nc.MISS, 0, 0, 0]).all() and (point[miss].view(np.uint32) == 0).all()
    check(uni, n, q.run(cornell_gpu, n, max_dist=0.1, form=_form(pt, form)), "uniform")
    assert 0 < uni.found.sum() < n
    # (per-query radii win over max_dist, which then plays no part -- not even an invalid one)
    check(cyc, n, q.run(cornell_gpu, n, per_query=True, max_dist=-1.0, form=_form(pt, form)), "cycled, max_dist ignored")


@pytest.fixture(scope="module")
def soup(pt, gpu_ctx):
    (v, i, f), ref = nc.soup_set()
    scene = pt.Scene(gpu_ctx, v, i, f)
    q = Query(pt, gpu_ctx, ref.points)
    yield scene, q, ref
    q.close(); scene.close()


def test_beyond_lds_and_the_spill_path(pt, gpu_ctx, cornell_gpu, box, box_query, soup):
    """3. tc.soup(4096, 11), 2 000 queries: AUTO (which runs GLOBAL) and GLOBAL equal the restatement; PT_NEAREST_LDS is PT_ERR_UNSUPPORTED --
    4096 x 48 B of triangles alone exceed 96 KB; the soup and the box again under pt_tuning.lds_stack = 1, where every lane spills: same bytes"""
    scene, q, ref = soup
    n = len(ref.points)
    assert scene.info().n_tris == 4096 and 4096 * 48 > 96 * 1024
    check(ref, n, q.run(scene, n, form=pt.NEAREST_AUTO), "soup AUTO")
    check(ref, n, q.run(scene, n, form=pt.NEAREST_GLOBAL), "soup GLOBAL")
    q.canary()
    with pytest.raises(pt.PtError) as e:
        scene.nearest_device(n, q.points_ptr, nearest_ptr=q.nearest.ptr, point_ptr=q.point.ptr, form=pt.NEAREST_LDS)
    assert e.value.status == UNSUPPORTED and "PT_NEAREST_LDS" in str(e.value) and q.untouched()
    old = gpu_ctx.set_tuning(lds_stack=1)
    try:
        check(ref, n, q.run(scene, n, form=pt.NEAREST_GLOBAL), "soup, lds_stack = 1")
        for name in ("LDS", "GLOBAL"):
            check(box["free"], 1000, box_query.run(cornell_gpu, 1000, form=_form(pt, name)), "box, lds_stack = 1, " + name)
    finally:
        gpu_ctx.set_tuning(**old)


@pytest.fixture(scope="module")
def big(cornell_arrays):
    return nc.box_big(cornell_arrays)


@pytest.fixture(scope="module")
def one_block(pt, cornell_arrays, big):
    """a context with pt_tuning.extend_blocks = 1 (one block per CU), the box, and the big set's buffers"""
    ctx = pt.Context(0)
    ctx.set_tuning(extend_blocks=1)
    scene = pt.Scene(ctx, *cornell_arrays)
    q = Query(pt, ctx, big.points)
    yield ctx, scene, q
    q.close(); scene.close(); ctx.close()


@pytest.mark.parametrize("form", ["LDS", "GLOBAL"])
@pytest.mark.parametrize("refill", [-1, 1, 64], ids=["refill_default", "refill_1", "refill_64"])
def test_persistent_loop_edges(pt, big, one_block, refill, form):
    """4. 200 001 queries through a grid of one block per CU: every wave draws from at least three strides of its private sequence and the last
    is ragged -- a second refill round, a partial final round and the drain; again refilling at one idle lane and only at 64"""
    ctx, scene, q = one_block
    old = ctx.set_tuning(refill=refill)
    try:
        ctx.reset_stats()
        check(big, nc.BIG_N, q.run(scene, nc.BIG_N, form=_form(pt, form)), form)
        assert ctx.stats().launches_other == 1 and ctx.stats().launches_extend == 0
    finally:
        ctx.set_tuning(**old)


def test_rows_four_byte_aligned(pt, gpu_ctx, cornell_gpu, box):
    """5. rows 4 bytes into their allocation (points_ptr % 8 == 4), prefixes 65 and 1 000, both forms"""
    q = Query(pt, gpu_ctx, box["free"].points, offset=4)
    try:
        assert q.points_ptr % 8 == 4
        for n in (65, 1000):
            for name in ("LDS", "GLOBAL"):
                check(box["free"], n, q.run(cornell_gpu, n, form=_form(pt, name)), name)
    finally:
        q.close()


def test_scene_changes(pt, gpu_ctx, cornell_arrays, box, box_query):
    """6. after update(REFIT) with the short block moved the answers are those of the new vertices (and differ from the old); unchanged by
    set_faces and by set_bvh_quality(FAST_BUILD) -- the answer does not depend on the builder; a scene made by pt_scene_create_device gives the
    same bytes"""
    import torch
    v, i, f = cornell_arrays
    ref, q, n = box["free"], box_query, 1000
    v2, moved = nc.box_moved(cornell_arrays)
    assert moved.rec.tobytes() != ref.rec.tobytes()
    scene = pt.Scene(gpu_ctx, v, i, f)
    try:
        check(ref, n, q.run(scene, n), "fresh")
        scene.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
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


def test_refusals_and_stats(pt, gpu_ctx, cornell_arrays, cornell_gpu, box, box_query):
    """7. every refusal of the header, an instanced box included, leaves the canaries intact and launches nothing; a good call afterwards adds
    exactly 1 to launches_other and nothing to launches_extend, rays, paths; trace_workspace_bytes() stays as it was (0 in a fresh context);
    device_ms > 0; n == 0 is PT_OK with device_ms == 0"""
    q, lib, n = box_query, pt.lib_amd(), 257
    nan = float("nan")

    def desc(**kw):
        d = pt.nearest_default_desc()
        d.d_points, d.d_nearest, d.d_point = q.points_ptr, q.nearest.ptr, q.point.ptr
        for k, v in kw.items():
            if k.startswith("reserved"):
                d.reserved[int(k[8:])] = v
            else:
                setattr(d, k, v)
        return d

    cases = [(desc(d_points=None), INVALID), (desc(d_nearest=None, d_point=None), INVALID), (desc(form=3), INVALID), (desc(form=0xFFFFFFFF), INVALID),
             (desc(flags=1), INVALID), (desc(flags=0x80000000), INVALID), (desc(reserved0=1), INVALID), (desc(reserved4=1), INVALID),
             (desc(max_dist=nan), INVALID), (desc(max_dist=-1.0), INVALID), (desc(max_dist=-float("inf")), INVALID)]
    q.canary()
    gpu_ctx.sync()
    gpu_ctx.reset_stats()
    ws = gpu_ctx.trace_workspace_bytes()
    for k, (d, want) in enumerate(cases):
        assert lib.pt_nearest_device(cornell_gpu.h, C.byref(d), n, None) == want, k
    assert lib.pt_nearest_device(None, C.byref(desc()), n, None) == INVALID and lib.pt_nearest_device(cornell_gpu.h, None, n, None) == INVALID
    inst = pt.Scene(gpu_ctx, *cornell_arrays)
    try:
        inst.set_instances(tc.INSTANCES)
        with pytest.raises(pt.PtError) as e:
            inst.nearest_device(n, q.points_ptr, nearest_ptr=q.nearest.ptr, point_ptr=q.point.ptr)
        assert e.value.status == UNSUPPORTED and "instance" in str(e.value) and "n = 0" in str(e.value), str(e.value)
        assert q.untouched()
        inst.set_instances(np.zeros((0, 12), f32))   # n = 0 instances restores the mesh
        check(box["free"], n, q.run(inst, n), "instances removed")
    finally:
        inst.close()
    q.canary()
    gpu_ctx.reset_stats()
    ms = C.c_float(-1.0)
    assert lib.pt_nearest_device(cornell_gpu.h, C.byref(desc()), 0, C.byref(ms)) == 0 and ms.value == 0.0        # n == 0
    assert lib.pt_nearest_device(cornell_gpu.h, C.byref(desc(d_points=None)), 0, C.byref(ms)) == 0               # ... which needs no points
    gpu_ctx.sync()
    st = gpu_ctx.stats()
    assert (st.launches_extend, st.launches_other, st.rays, st.paths) == (0, 0, 0, 0) and q.untouched()
    check(box["free"], n, q.run(cornell_gpu, n), "after the refusals")
    st = gpu_ctx.stats()
    assert (st.launches_extend, st.launches_other, st.rays, st.paths) == (0, 1, 0, 0)
    assert q.ms > 0 and gpu_ctx.trace_workspace_bytes() == ws
    fresh = pt.Context(0)
    try:
        sc = pt.Scene(fresh, *cornell_arrays)
        q2 = Query(pt, fresh, box["free"].points[:65])
        check(box["free"], 65, q2.run(sc, 65), "fresh context")
        assert fresh.trace_workspace_bytes() == 0
        q2.close(); sc.close()
    finally:
        fresh.close()


def test_nearest_tensors(pt, cornell_gpu, box):
    """8. the torch wrapper on a non-contiguous [n, 3] view: form="lds", "global" and "auto" agree bit for bit with each other and with the
    restatement; per-query radii and one radius"""
    import torch
    n = 1000
    ref = box["free"]
    dev = torch.device("cuda", 0)
    wide = torch.zeros((n, 5), dtype=torch.float32, device=dev)
    wide[:, 1:4] = torch.from_numpy(ref.points).to(dev)
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    outs = {}
    for form in ("lds", "global", "auto"):
        out = cornell_gpu.nearest_tensors(view, point=True, form=form)
        assert set(out) == {"prim", "dist2", "u", "v", "point"}
        for k in ("prim", "dist2", "u", "v"):
            assert out[k].cpu().numpy().view(np.uint32).tobytes() == ref.rec[k].view(np.uint32).tobytes(), (form, k)
        assert out["point"].cpu().numpy().tobytes() == ref.point.tobytes(), form
        outs[form] = out
    for k in outs["lds"]:
        assert torch.equal(outs["lds"][k].view(torch.int32), outs["global"][k].view(torch.int32)) and torch.equal(outs["lds"][k].view(torch.int32), outs["auto"][k].view(torch.int32))
    out = cornell_gpu.nearest_tensors(view, max_dist_per_query=torch.from_numpy(nc.cycled_radii(n)).to(dev))
    assert "point" not in out and out["prim"].cpu().numpy().view(np.uint32).tobytes() == box["cycled"].rec["prim"].tobytes()
    assert (out["prim"].cpu().numpy()[~box["cycled"].found] == -1).all()
    out = cornell_gpu.nearest_tensors(view, max_dist=0.1)
    assert out["dist2"].cpu().numpy().tobytes() == box["uniform"].rec["dist2"].tobytes()
    with pytest.raises(ValueError):
        cornell_gpu.nearest_tensors(view, form="fused")
