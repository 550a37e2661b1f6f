"""PT_TRACE_FUSED / PT_TRACE_AUTO on the GPU (include/pt_api.h): pt_trace_device through ONE kernel from the caller's rows to
the caller's records.  Every comparison is bytes against bytes: against the CPU oracle (closest hits in brute-force mode, orc.Scene.shade_hit,
"a closest hit exists" for occlusion) and against the queue form of the same desc.  The ray recipes and the oracle's answers are
tests/trace_device_cases.py and tests/trace_fused_cases.py (computed once per session); tests/test_trace_fused_cpu.py holds the big set against
the oracle alone.  Every output is canary-filled before every call and read back whole."""
import ctypes as C

import numpy as np
import pytest

import trace_device_cases as tc
import trace_fused_cases as tfc
from trace_fused_cases import Query, check_closest, same_closest

f32 = np.float32
MISS = tc.MISS
pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = 1, 5


@pytest.fixture(scope="module")
def box(orc, cornell_arrays):
    return tfc.box_answers(orc, cornell_arrays)


@pytest.fixture(scope="module")
def big(orc, cornell_arrays):
    return tfc.big_answers(orc, cornell_arrays)


@pytest.fixture(scope="module")
def box_query(pt, gpu_ctx, box):
    q = Query(pt, gpu_ctx, box.rays, box.bounds)
    yield q
    q.close()


def _all_kinds(pt, scene, q, ans, n, what, queue_too=True, flags=None):
    """the three kinds of query over rays [0, n) under `flags` (PT_TRACE_FUSED): == the oracle and == the queue form"""
    F = pt.TRACE_FUSED if flags is None else flags
    got = q.closest(scene, n, flags=F)
    check_closest(ans, n, got, what)
    if queue_too:
        assert same_closest(got, q.closest(scene, n)), (what, n, "queue form")
    got = q.closest(scene, n, planes=(), flags=F)
    check_closest(ans, n, got, what + " hits only")
    o = q.any(scene, n, flags=F)
    assert (o == ans.occ_cycled[:n]).all(), (what, n, np.flatnonzero(o != ans.occ_cycled[:n])[:8])
    if queue_too:
        assert (o == q.any(scene, n)).all(), (what, n, "queue form")
    o = q.any(scene, n, per_ray=False, tmax=ans.uniform_bound, flags=F)
    assert (o == ans.occ_uniform[:n]).all(), (what, n, "uniform")
    if queue_too:
        assert (o == q.any(scene, n, per_ray=False, tmax=ans.uniform_bound)).all(), (what, n, "uniform, queue form")


def test_all_prefixes_all_queries(pt, gpu_ctx, cornell_gpu, box, box_query):
    """1. every prefix of the box's rays with PT_TRACE_FUSED: hits + all four planes, d_hits NULL beside the planes, each plane alone, hits alone;
    ANY with the cycled per-ray bounds and with one bound -- equal to the oracle and to the queue form, canaries intact beyond row n and in every
    output that was not named (Query asserts them)"""
    q, F = box_query, pt.TRACE_FUSED
    assert box.hits["prim"][0] != MISS and box.occ_cycled[0] == 0
    for n in tc.PREFIXES:
        if n >= 63:
            assert 0.3 <= box.hit_share(n) <= 0.9 and 0.2 <= box.occ_share(n) <= 0.8
        _all_kinds(pt, cornell_gpu, q, box, n, "box")
        got = q.closest(cornell_gpu, n, hits=False, flags=F)
        check_closest(box, n, got, "planes, d_hits NULL")
        assert same_closest(got, q.closest(cornell_gpu, n, hits=False))
        for k in range(4):
            got = q.closest(cornell_gpu, n, hits=False, planes=(k,), flags=F)
            check_closest(box, n, got, "one plane")
            assert same_closest(got, q.closest(cornell_gpu, n, hits=False, planes=(k,)))
    assert gpu_ctx.stats().pipeline == pt.PIPELINE_FUSED


@pytest.fixture(scope="module")
def one_block(pt, cornell_arrays, big):
    """a context with pt_tuning.extend_blocks = 1 (one block per CU), the box, and the big ray set's buffers"""
    ctx = pt.Context(0)
    ctx.set_tuning(extend_blocks=1)
    scene = pt.Scene(ctx, *cornell_arrays)
    q = Query(pt, ctx, big.rays, big.bounds)
    yield ctx, scene, q
    q.close(); scene.close(); ctx.close()


@pytest.mark.parametrize("refill", [-1, 1, 64], ids=["refill_default", "refill_1", "refill_64"])
def test_persistent_loop_edges(pt, big, one_block, refill):
    """2. 200 001 rays through a grid of one block per CU, all three kinds: every wave draws from at least three strides of its private sequence
    and the last is ragged -- a second refill round, a partial final round and the drain; again refilling at one idle lane and only at 64.
    The bytes are the oracle's (ANY at tmin = BIG_ANY_TMIN, where every bound sees both answers)."""
    ctx, scene, q = one_block
    n = tfc.BIG_N
    hit, occ, per = tfc.big_shares(big)
    assert 0.3 < hit < 0.8 and 0.2 < occ < 0.7 and all(0 < round(s * c) < c for s, c in per)
    old = ctx.set_tuning(refill=refill)
    try:
        F = pt.TRACE_FUSED
        ctx.reset_stats()
        check_closest(big, n, q.closest(scene, n, planes=(), flags=F), "hits")
        assert ctx.stats().launches_extend == 1 and ctx.stats().launches_other == 0
        check_closest(big, n, q.closest(scene, n, flags=F), "hits + surface")
        o = q.any(scene, n, tmin=tfc.BIG_ANY_TMIN, flags=F)
        assert (o == big.occ_cycled).all(), np.flatnonzero(o != big.occ_cycled)[:8]
        o = q.any(scene, n, per_ray=False, tmax=big.uniform_bound, flags=F)
        assert (o == big.occ_uniform).all()
        assert ctx.trace_workspace_bytes() == 0
    finally:
        ctx.set_tuning(**old)


@pytest.mark.parametrize("form", ["pair_leaves_0", "pair_kernel_0"])
def test_both_leaf_forms(pt, gpu_ctx, cornell_arrays, cornell_gpu, box, box_query, form):
    """3. leaves of up to four: a scene created under pair_leaves = 0, and the default scene walked under pair_kernel = 0, prefixes 65 and 1000"""
    if form == "pair_leaves_0":
        old = gpu_ctx.set_tuning(pair_leaves=0)
        try:
            scene = pt.Scene(gpu_ctx, *cornell_arrays)
        finally:
            gpu_ctx.set_tuning(**old)
        old = {}
    else:
        scene = cornell_gpu
        old = gpu_ctx.set_tuning(pair_kernel=0)
    try:
        for n in (65, 1000):
            _all_kinds(pt, scene, box_query, box, n, form)
        assert gpu_ctx.stats().pipeline == pt.PIPELINE_FUSED
    finally:
        gpu_ctx.set_tuning(**old)
        if scene is not cornell_gpu:
            scene.close()


def test_rows_four_byte_aligned(pt, gpu_ctx, cornell_gpu, box):
    """4. a rays buffer whose first row lies 4 bytes into its allocation: six dword loads per row, no wider one"""
    q = Query(pt, gpu_ctx, box.rays, box.bounds, ray_offset=4)
    try:
        assert q.rays_ptr % 8 == 4
        for n in (65, 1000):
            _all_kinds(pt, cornell_gpu, q, box, n, "offset rows")
    finally:
        q.close()


def test_after_a_refit(pt, orc, gpu_ctx, cornell_arrays, box, box_query):
    """5. REFIT of the box with the short block moved: the single-kernel form answers for the new arrays (and differs from the old answer)"""
    v, i, f = cornell_arrays
    v2 = tc.move_short_box(v)
    ans = tc.answers("box_moved", lambda: tc.Answers(orc.Scene(v2, i, f), f, box.rays))
    assert ans.hits.tobytes() != box.hits.tobytes()
    scene = pt.Scene(gpu_ctx, v, i, f)
    try:
        check_closest(box, 1000, box_query.closest(scene, 1000, flags=pt.TRACE_FUSED), "before the update")
        scene.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
        _all_kinds(pt, scene, box_query, ans, 1000, "after the update")
    finally:
        scene.close()


def test_async_stats_and_workspace(pt, cornell_arrays, box):
    """6. PT_TRACE_ASYNC | PT_TRACE_FUSED only queues and pt_sync waits; one blocking call is one extend launch and no other, pipeline FUSED,
    variant LDS, ms_extend its own time, rays and paths stay; chunk_rays is ignored; a context that only ran this form holds no workspace"""
    ctx = pt.Context(0)
    scene = pt.Scene(ctx, *cornell_arrays)
    q = Query(pt, ctx, box.rays, box.bounds)
    try:
        n = 1000
        ctx.reset_stats()
        assert q.closest(scene, n, read=False, flags=pt.TRACE_ASYNC | pt.TRACE_FUSED) is None and q.ms == 0.0
        ctx.sync()
        st = ctx.stats()
        assert (st.launches_extend, st.launches_other, st.ms_extend) == (1, 0, 0.0)
        check_closest(box, n, q.read_closest(n), "async")
        ctx.reset_stats()
        check_closest(box, n, q.closest(scene, n, flags=pt.TRACE_FUSED, chunk_rays=64), "blocking, chunk_rays ignored")
        st = ctx.stats()
        assert (st.launches_extend, st.launches_other, st.launches_shade, st.rounds, st.rays, st.paths) == (1, 0, 0, 0, 0, 0)
        assert st.pipeline == pt.PIPELINE_FUSED and st.extend_variant == pt.EXTEND_LDS
        assert st.ms_extend > 0 and q.ms >= st.ms_extend * 0.99
        ctx.reset_stats()
        o = q.any(scene, n, flags=pt.TRACE_FUSED)
        assert (o == box.occ_cycled[:n]).all() and (ctx.stats().launches_extend, ctx.stats().launches_other) == (1, 0)
        assert ctx.trace_workspace_bytes() == 0
        # the queue form of the same context afterwards: its workspace, its stats, pipeline left alone without the bits
        ctx.reset_stats()
        check_closest(box, n, q.closest(scene, n), "queues afterwards")
        assert ctx.trace_workspace_bytes() == 1024 * 48 + 8 and (ctx.stats().launches_extend, ctx.stats().launches_other) == (1, 3)
        check_closest(box, n, q.closest(scene, n, flags=pt.TRACE_FUSED), "single kernel again")
        assert ctx.trace_workspace_bytes() == 1024 * 48 + 8
    finally:
        q.close(); scene.close(); ctx.close()


def test_auto(pt, orc, gpu_ctx, cornell_arrays, cornell_gpu, box, box_query):
    """7. PT_TRACE_AUTO: on the box the oracle's answers by a legal form; on the 3-instance scene, on a 4 096-triangle soup, with a named extend
    kernel and with tmin = 0 it is PT_OK, the queue form runs and the answers equal the same call without the flag"""
    A, q = pt.TRACE_AUTO, box_query
    for n in (65, 1000):
        gpu_ctx.reset_stats()
        _all_kinds(pt, cornell_gpu, q, box, n, "auto", flags=A)
        assert gpu_ctx.stats().pipeline in (pt.PIPELINE_FUSED, pt.PIPELINE_WAVEFRONT)

    def queues_ran(scene, qq, n, **kw):
        gpu_ctx.reset_stats()
        got = qq.closest(scene, n, flags=A, **kw)
        st = gpu_ctx.stats()
        assert st.pipeline == pt.PIPELINE_WAVEFRONT and st.launches_other == 3, (kw, st.pipeline, st.launches_other)
        assert same_closest(got, qq.closest(scene, n, **kw)), kw
        gpu_ctx.reset_stats()
        o = qq.any(scene, n, flags=A, **kw)
        assert gpu_ctx.stats().pipeline == pt.PIPELINE_WAVEFRONT and gpu_ctx.stats().launches_other == 2
        assert (o == qq.any(scene, n, **kw)).all(), kw
        return got

    check_closest(box, 1000, queues_ran(cornell_gpu, q, 1000, extend=pt.EXTEND_HBM), "auto, EXTEND_HBM")
    queues_ran(cornell_gpu, q, 1000, tmin=0.0)
    inst = pt.Scene(gpu_ctx, *cornell_arrays)
    rays_i = tc.make_rays(seed=7, x_seed=8)
    qi = Query(pt, gpu_ctx, rays_i, tc.cycled_bounds(len(rays_i)))
    v, i, f = tc.soup(4096, 11)
    soup = pt.Scene(gpu_ctx, v, i, f)
    rays_s = tc.make_rays(seed=2024, half=1.3, centre=None)
    qs = Query(pt, gpu_ctx, rays_s, tc.cycled_bounds(len(rays_s)))
    try:
        inst.set_instances(tc.INSTANCES)
        h, _ = queues_ran(inst, qi, 1000)
        assert set(np.unique(h["inst"][h["prim"] != MISS])) == {0, 1, 2}
        h, _ = queues_ran(soup, qs, 1000)
        assert 0.05 < (h["prim"] != MISS).mean() < 0.95
    finally:
        qi.close(); qs.close(); inst.close(); soup.close()


def test_refusals(pt, gpu_ctx, cornell_arrays, cornell_gpu, box, box_query):
    """8. FUSED | AUTO, flags 2 and 16 are INVALID; FUSED outside its class (instanced, beyond LDS, a named kernel, tmin = 0) and with CLOSEST +
    d_tmax is UNSUPPORTED with the class named; every INVALID of the queue form stays INVALID under FUSED -- outputs untouched, nothing
    launched, and a good call afterwards"""
    q, lib, n = box_query, pt.lib_amd(), 257
    nan, inf = float("nan"), float("inf")
    F = pt.TRACE_FUSED

    def desc(mode=pt.TRACE_CLOSEST, flags=F, **kw):
        d = pt.trace_default_desc()
        d.d_rays6, d.mode, d.flags = q.rays_ptr, mode, flags
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

    cases = [(desc(flags=F | pt.TRACE_AUTO), INVALID), (desc(flags=2), INVALID), (desc(flags=16), INVALID), (desc(flags=F | 2), INVALID),
             (desc(flags=pt.TRACE_AUTO | 16), INVALID), (desc(pt.TRACE_ANY, flags=F | pt.TRACE_AUTO | pt.TRACE_ASYNC), INVALID),
             # the queue form's table (tests/test_trace_device.py), under PT_TRACE_FUSED
             (desc(d_rays6=None), INVALID), (desc(mode=2), INVALID), (desc(flags=F | 3), INVALID), (desc(reserved=1), INVALID),
             (desc(tmin=nan), INVALID), (desc(tmax=nan), INVALID), (desc(tmax=inf), INVALID), (desc(tmin=-inf), INVALID), (desc(tmin=1.0, tmax=1.0), INVALID),
             (desc(tmin=2.0, tmax=1.0), INVALID),
             (desc(d_hits=None, d_position=None, d_normal=None, d_albedo=None, d_emission=None), INVALID), (desc(d_occluded=q.occ.ptr), INVALID),
             (desc(pt.TRACE_ANY, d_hits=q.hits.ptr), INVALID), (desc(pt.TRACE_ANY, d_albedo=q.planes[2].ptr), INVALID),
             (desc(pt.TRACE_ANY, d_occluded=None), INVALID), (desc(extend=9), INVALID),
             (desc(d_tmax=q.bounds.ptr), UNSUPPORTED), (desc(extend=pt.EXTEND_FLAT), UNSUPPORTED), (desc(pt.TRACE_ANY, extend=pt.EXTEND_FLAT), UNSUPPORTED),
             # outside the class
             (desc(extend=pt.EXTEND_LDS), UNSUPPORTED), (desc(extend=pt.EXTEND_HBM), UNSUPPORTED), (desc(tmin=0.0), UNSUPPORTED),
             (desc(pt.TRACE_ANY, extend=pt.EXTEND_HBM), UNSUPPORTED), (desc(pt.TRACE_ANY, tmin=0.0), UNSUPPORTED)]
    q.canary()
    gpu_ctx.reset_stats()
    for k, (d, want) in enumerate(cases):
        assert lib.pt_trace_device(cornell_gpu.h, C.byref(d), n, None) == want, k
    with pytest.raises(pt.PtError) as e:
        cornell_gpu.trace_device(n, q.rays_ptr, hits_ptr=q.hits.ptr, tmin=0.0, flags=F)
    assert e.value.status == UNSUPPORTED and "PT_TRACE_FUSED" in str(e.value) and "tmin" in str(e.value)
    inst = pt.Scene(gpu_ctx, *cornell_arrays)
    v, i, f = tc.soup(4096, 11)
    soup = pt.Scene(gpu_ctx, v, i, f)
    try:
        inst.set_instances(tc.INSTANCES)
        for scene, word in ((inst, "instanced"), (soup, "LDS")):
            for d in (desc(), desc(pt.TRACE_ANY)):
                assert lib.pt_trace_device(scene.h, C.byref(d), n, None) == UNSUPPORTED, word
            with pytest.raises(pt.PtError) as e:
                scene.trace_device(n, q.rays_ptr, hits_ptr=q.hits.ptr, flags=F)
            assert e.value.status == UNSUPPORTED and word in str(e.value), str(e.value)
    finally:
        inst.close(); soup.close()
    ms = C.c_float(-1.0)
    assert lib.pt_trace_device(cornell_gpu.h, C.byref(desc()), 0, C.byref(ms)) == 0 and ms.value == 0.0       # n == 0
    gpu_ctx.sync()
    st = gpu_ctx.stats()
    assert (st.launches_extend, st.launches_other) == (0, 0) and q.untouched()
    check_closest(box, n, q.closest(cornell_gpu, n, flags=F), "after the refusals")


def test_trace_tensors_forms(pt, cornell_gpu, box):
    """9. the torch wrapper on a non-contiguous [n, 6] view: form="fused" and form="auto" equal form="queues", hits, planes and occlusion"""
    import torch
    n = 1000
    dev = torch.device("cuda", 0)
    wide = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    wide[:, 1:7] = torch.from_numpy(box.rays).to(dev)
    view = wide[:, 1:7]
    assert not view.is_contiguous()
    bounds = torch.from_numpy(box.bounds).to(dev)
    ref = cornell_gpu.trace_tensors(view, surface=True, form="queues")
    assert ref["prim"].cpu().numpy().view(np.uint32).tobytes() == box.hits["prim"].tobytes()
    occ_ref = cornell_gpu.trace_tensors(view, tmax_per_ray=bounds, mode=pt.TRACE_ANY)
    assert (occ_ref.cpu().numpy() == box.occ_cycled.astype(bool)).all()
    for form in ("fused", "auto"):
        out = cornell_gpu.trace_tensors(view, surface=True, form=form)
        assert set(out) == set(ref)
        for k in ref:
            assert torch.equal(out[k].view(torch.int32), ref[k].view(torch.int32)), (form, k)
        assert torch.equal(cornell_gpu.trace_tensors(view, tmax_per_ray=bounds, mode=pt.TRACE_ANY, form=form), occ_ref), form
    with pytest.raises(ValueError):
        cornell_gpu.trace_tensors(view, form="wavefront")
