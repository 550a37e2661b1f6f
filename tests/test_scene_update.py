"""pt_scene_update (API version 6): new vertex positions for a scene's triangles, by refitting its trees (REFIT) or by building them
again (REBUILD).  Bar: every image, ray count and hit record equals what a scene freshly created from the new arrays gives -- checked
against the CPU oracle built from the NEW arrays, on every pipeline -- and the refitted trees stay valid trees of the old topology."""
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ["refit", "rebuild"]
W, H = 64, 48
KW = dict(width=W, height=H, spp_per_frame=4, max_depth=5)


def _mode(pt, name):
    return pt.SCENE_UPDATE_REFIT if name == "refit" else pt.SCENE_UPDATE_REBUILD


def _soup(n, seed, spread=0.1):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)).astype(np.float32)
    v = (c + rng.uniform(-spread, spread, (n, 3, 3)).astype(np.float32)).astype(np.float32)
    faces = rng.uniform(0, 1, (n, 6)).astype(np.float32)
    faces[:, 3:] *= (rng.uniform(0, 1, (n, 1)) < 0.1)
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), faces.reshape(-1).astype(np.float32)


def _deform(v, seed, jitter=0.01):
    """The Cornell box moved: the tall block's top raised and shifted, every vertex jittered.  Indices are untouched and vertices of
    equal coordinates move together, so shared vertices stay shared and the quads' fan pairs stay pairs (the refit keeps its tree)."""
    rng = np.random.default_rng(seed)
    p = np.array(v, np.float32).reshape(-1, 3).copy()
    lo, hi = p.min(0), p.max(0)
    ext = hi - lo
    top = (p[:, 1] > lo[1] + 0.5 * ext[1]) & (p[:, 1] < lo[1] + 0.7 * ext[1])  # the tall block's top (walls sit at the floor / ceiling)
    p[top] += np.float32([0.05, 0.15, -0.03]) * ext
    uniq, inv = np.unique(p, axis=0, return_inverse=True)
    uniq = uniq + rng.uniform(-jitter, jitter, uniq.shape).astype(np.float32) * ext
    return uniq.astype(np.float32)[inv.reshape(-1)].reshape(-1)


def _oracle(orc, osc, frames, nee=False, **kw):
    film = bgra = None
    rays = 0
    for k in range(frames):
        extra = dict(nee=1) if nee else {}
        img, r, _, _ = osc.render_frame(orc.default_params(frame=k, **extra, **kw))
        if film is None:
            film = np.zeros_like(img)
            bgra = np.zeros(img.shape[:2] + (4,), np.uint8)
        orc.accumulate_f32(film, img, k)
        orc.accumulate_bgra8(bgra, img, k)
        rays += r
    return film, bgra, rays


def _render(pt, ctx, scene, frames, pipeline, flags=0, **kw):
    args = dict(KW, **kw)
    film = pt.Film(ctx, args["width"], args["height"])
    ctx.reset_stats()
    pt.render(scene, film, pt.default_params(frame=0, frame_count=frames, pipeline=pipeline, flags=flags, **args))
    out = film.read_f32(), film.read_bgra8(), ctx.stats().rays
    film.close()
    return out


def _check_pipelines(pt, orc, ctx, gs, v, i, f, cases, instances=None, **kw):
    """(pipeline, flags, nee) cases, 2 frames each: film, rgba8 (the reference estimator) and ray count as the oracle's of (v, i, f)."""
    osc = orc.Scene(v, i, f)
    if instances is not None:
        osc.set_instances(instances)
    args = dict(KW, **kw)
    args.pop("extend", None)
    want = {}
    for pipeline, flags, nee in cases:
        if nee not in want:
            want[nee] = _oracle(orc, osc, 2, nee=nee, **args)
        film, bgra, rays = _render(pt, ctx, gs, 2, pipeline, flags, **kw)
        of, ob, orays = want[nee]
        assert rays == orays, (pipeline, flags, rays, orays)
        assert film.tobytes() == of.tobytes(), (pipeline, flags, float(np.abs(film - of).max()))
        if not nee:
            assert bgra.tobytes() == ob.tobytes(), (pipeline, flags)
    return want[cases[0][2]]


def _cases(pt):
    return [(pt.PIPELINE_AUTO, 0, False), (pt.PIPELINE_WAVEFRONT, 0, False), (pt.PIPELINE_FUSED, pt.FLAG_NEE, True),
            (pt.PIPELINE_WAVEFRONT_NEE, 0, True)]


def _rays(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    org = rng.uniform(lo - 0.5, hi + 0.5, (n, 3)).astype(np.float32)
    tgt = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([org, d.astype(np.float32)], 1).astype(np.float32)


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------

def test_header_declares_scene_update_and_the_package_binds_it(pt):
    txt = open(os.path.join(os.path.dirname(HERE), "include", "pt_api.h")).read()
    assert re.search(r"pt_status\s+pt_scene_update\s*\(\s*pt_scene\s*\*\s*scene\s*,\s*const float\s*\*\s*vertices\s*,\s*uint32_t n_verts\s*,"
                     r"\s*const uint32_t\s*\*\s*indices\s*,\s*uint32_t n_tris\s*,\s*uint32_t mode\s*\)", txt)
    assert re.search(r"PT_SCENE_UPDATE_REFIT\s*=\s*0\s*,\s*PT_SCENE_UPDATE_REBUILD\s*=\s*1", txt)
    assert "pt_scene_update" in pt.API_SYMBOLS
    assert callable(getattr(pt.Scene, "update", None))
    assert (pt.SCENE_UPDATE_REFIT, pt.SCENE_UPDATE_REBUILD) == (0, 1)


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_cornell_update_renders_like_a_fresh_scene(pt, orc, gpu_ctx, cornell_arrays, mode):
    """AUTO (the fused kernel), WAVEFRONT, FUSED | NEE and WAVEFRONT_NEE after an update: film, rgba8 and rays of the new arrays."""
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_AUTO)     # (plans and tables of the old geometry exist before the update)
    v2 = _deform(v, 1)
    gs.update(v2, i, mode=_mode(pt, mode))
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt))
    fresh = pt.Scene(gpu_ctx, v2, i, f)
    info, finfo = gs.info(), fresh.info()
    assert list(info.bbox_min) == list(finfo.bbox_min) and list(info.bbox_max) == list(finfo.bbox_max)
    assert info.build_ms > 0 and info.n_tris == len(i) // 3
    fresh.close(); gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_update_that_grows_the_scene_box(pt, orc, gpu_ctx, cornell_arrays, mode):
    """Geometry moved beyond the old box's projection: pixels the camera-ray cull resolved as misses before must now hit."""
    v, i, f = cornell_arrays
    p = np.array(v, np.float32).reshape(-1, 3)
    c = 0.5 * (p.min(0) + p.max(0))
    v2 = ((p - c) * np.float32(1.6) + c).astype(np.float32).reshape(-1)
    gs = pt.Scene(gpu_ctx, v, i, f)
    old = _render(pt, gpu_ctx, gs, 2, pt.PIPELINE_AUTO)
    gs.update(v2, i, mode=_mode(pt, mode))
    new = _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt)[:2])
    assert new[0].tobytes() != old[0].tobytes()
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_trace_after_update_equals_the_oracle(pt, orc, gpu_ctx, cornell_arrays, mode):
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    v2 = _deform(v, 2)
    gs.update(v2, i, mode=_mode(pt, mode))
    p = v2.reshape(-1, 3)
    rays = _rays(4096, 3, p.min(0), p.max(0))
    hits = gs.trace(rays)
    ohits, _ = orc.Scene(v2, i, f).trace(rays, mode=1)
    assert hits.tobytes() == ohits.tobytes()
    assert (hits["prim"] != pt.MISS).mean() > 0.3
    for ext in (pt.EXTEND_LDS, pt.EXTEND_HBM, pt.EXTEND_HBM8):
        assert gs.trace(rays, extend=ext).tobytes() == ohits.tobytes(), ext
    gs.close()


@pytest.mark.gpu
def test_refit_keeps_topology_and_stays_conservative_rebuild_equals_fresh(pt, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    nt = len(i) // 3
    gs = pt.Scene(gpu_ctx, v, i, f)
    before = gs.read_bvh4()
    for seed in (4, 5):   # twice: a refit of a refitted tree
        v2 = _deform(v, seed, jitter=0.03)
        tri = v2.reshape(-1, 3)[np.asarray(i).reshape(-1, 3)]          # [nt][3][xyz]
        gs.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
        rows = gs.read_bvh4()
        assert rows.shape == before.shape and (rows[:, 24:] == before[:, 24:]).all()   # child words (and the spare row) kept
        pl = rows[:, :24].copy().view(np.float32).reshape(-1, 6, 4)                    # [node][lo.x lo.y lo.z hi.x hi.y hi.z][slot]
        words = rows[:, 24:28]
        leaves = 0
        for n in range(rows.shape[0]):
            for k in range(4):
                w = int(words[n, k])
                if w == 0xFFFFFFFF:
                    continue
                if w & 0x80000000:
                    leaves += ((w >> 28) & 7) + 1
                    continue
                live = words[w] != 0xFFFFFFFF      # every child slot inside the parent's slot for that child
                assert (pl[n, 0:3, k][:, None] <= pl[w, 0:3][:, live]).all() and (pl[n, 3:6, k][:, None] >= pl[w, 3:6][:, live]).all()
        assert leaves == nt
        root = words[0] != 0xFFFFFFFF
        assert (pl[0, 0:3][:, root].min(1) <= tri.reshape(-1, 3).min(0)).all()
        assert (pl[0, 3:6][:, root].max(1) >= tri.reshape(-1, 3).max(0)).all()
        # every triangle inside its leaf's box, through the binary LBVH (refitted in place too; its leaves name sorted positions)
        _, prim, nodes = gs.read_bvh()
        nf = nodes[:, :12].copy().view(np.float32).reshape(-1, 4, 3)                  # lmin lmax rmin rmax
        for n in range(nodes.shape[0]):
            for side, (a, b) in enumerate(((0, 1), (2, 3))):
                ch = int(nodes[n, 12 + side])
                if ch & 0x80000000:
                    t = tri[prim[ch & 0x7FFFFFFF]]
                    assert (nf[n, a] <= t.min(0)).all() and (nf[n, b] >= t.max(0)).all()
        assert gs.info().build_ms > 0
    gs.update(v2, i, mode=pt.SCENE_UPDATE_REBUILD)
    fresh = pt.Scene(gpu_ctx, v2, i, f)
    assert gs.read_bvh4().tobytes() == fresh.read_bvh4().tobytes()
    for a, b in zip(gs.read_bvh(), fresh.read_bvh()):
        assert a.tobytes() == b.tobytes()
    assert gs.info().bvh4_builder == fresh.info().bvh4_builder == 1
    fresh.close(); gs.close()


def _quads_in_cornell(cornell_arrays, nq=6):
    """The Cornell box with a row of quads in front of its back wall: every quad two triangles (v0 v1 v2) (v0 v2 v3) with vertices of
    their own (no index shared), so the pairs form on bitwise-equal coordinates."""
    v, i, f = cornell_arrays
    p = np.array(v, np.float32).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    ext = hi - lo
    verts, faces = [], []
    for q in range(nq):
        x0 = lo[0] + ext[0] * (0.1 + 0.13 * q)
        x1 = x0 + ext[0] * 0.1
        y0, y1 = lo[1] + ext[1] * 0.3, lo[1] + ext[1] * 0.45
        z = lo[2] + ext[2] * 0.35
        a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
        verts += [a, b, c, a, c, d]
        faces += [(0.7, 0.3 + 0.05 * q, 0.2, 0, 0, 0)] * 2
    nv = p.shape[0]
    v2 = np.concatenate([p, np.array(verts, np.float32)]).reshape(-1).astype(np.float32)
    i2 = np.concatenate([np.asarray(i, np.uint32), nv + np.arange(6 * nq, dtype=np.uint32)])
    f2 = np.concatenate([np.asarray(f, np.float32), np.array(faces, np.float32).reshape(-1)]).astype(np.float32)
    return v2, i2, f2, len(np.asarray(i)) // 3


@pytest.mark.gpu
def test_refit_that_breaks_a_pair_leaf(pt, orc, gpu_ctx, cornell_arrays):
    """A quad whose halves no longer share their vertices cannot stay one pair leaf: the refit becomes a rebuild, same bits."""
    v, i, f, first = _quads_in_cornell(cornell_arrays)
    gs = pt.Scene(gpu_ctx, v, i, f)
    assert gs.info().bvh4_builder == 1
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, f, _cases(pt)[:1])
    v2 = np.array(v, np.float32).reshape(-1, 3).copy()
    second = first + 2 * 2 + 1                          # quad 2's second triangle: its v0 pulled away from the first's v0
    v2[int(np.asarray(i)[3 * second])] += np.float32([0.0, -0.05, 0.08])
    v2 = v2.reshape(-1)
    gs.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt)[:2])
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_WAVEFRONT, 0, False)], extend=pt.EXTEND_HBM)
    # a move that keeps every pair (the whole mesh shifted by one vector) stays a refit
    v3 = (np.array(v2, np.float32).reshape(-1, 3) + np.float32([0.01, 0.02, -0.01])).reshape(-1).astype(np.float32)
    gs.update(v3, i, mode=pt.SCENE_UPDATE_REFIT)
    _check_pipelines(pt, orc, gpu_ctx, gs, v3, i, f, _cases(pt)[:2])
    gs.close()


@pytest.mark.gpu
def test_refit_of_a_big_scene(pt, orc, gpu_ctx):
    """> 2048 triangles: the LBVH's collapse (this uniform soup's PLOC rebuild is not adopted, area ratio 0.988; tests/test_ploc_trees.py
    refits adopted trees), its 64-B top-down copy and the 8-wide nodes refitted in place."""
    from test_gpu_parity import _check_bvh8
    v, i, f = _soup(3000, 21, spread=0.05)
    v = (v.reshape(-1, 3) * np.float32([0.9, 0.9, 0.9]) + np.float32([0, -1, 0])).reshape(-1).astype(np.float32)
    gs = pt.Scene(gpu_ctx, v, i, f)
    words8 = gs.read_bvh8()[0][:, 14:16].copy()        # the 8-wide nodes exist before the update (built on first request)
    builder = gs.info().bvh4_builder
    rng = np.random.default_rng(22)
    v2 = (v.reshape(-1, 3) + rng.uniform(-0.03, 0.03, (len(v) // 3, 3)).astype(np.float32)).reshape(-1).astype(np.float32)
    gs.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
    assert gs.info().bvh4_builder == builder
    assert (gs.read_bvh8()[0][:, 14:16] == words8).all()
    _check_bvh8(pt, gs, v2, len(i) // 3)
    for ext in (pt.EXTEND_HBM, pt.EXTEND_HBM8, pt.EXTEND_AUTO):
        _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_WAVEFRONT, 0, False)], extend=ext)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_AUTO, 0, False)])
    rays = _rays(4096, 23, v2.reshape(-1, 3).min(0), v2.reshape(-1, 3).max(0))
    ohits, _ = orc.Scene(v2, i, f).trace(rays, mode=1)
    for ext in (pt.EXTEND_HBM, pt.EXTEND_HBM8):
        assert gs.trace(rays, extend=ext).tobytes() == ohits.tobytes(), ext
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_update_of_an_instanced_scene(pt, orc, gpu_ctx, cornell_arrays, mode):
    """The 16-instance grid: the BLAS updated, the TLAS built again from the stored transforms, world-space tables made again."""
    v, i, f = cornell_arrays
    grid = pt.cornell_grid_instances()[:16]
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.set_instances(grid)
    cam = dict(cam_origin=(-0.88, -1.9, 0.5), cam_target=(-0.88, -1.9, 0.0))
    _render(pt, gpu_ctx, gs, 1, pt.PIPELINE_WAVEFRONT_NEE, **cam)   # world-space emitters / frames of the old BLAS exist
    v2 = _deform(v, 6)
    gs.update(v2, i, mode=_mode(pt, mode))
    assert gs.info().n_instances == 16
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_AUTO, 0, False), (pt.PIPELINE_WAVEFRONT, 0, False),
                                                      (pt.PIPELINE_WAVEFRONT_NEE, 0, True)], instances=grid, **cam)
    gs.close()


@pytest.mark.gpu
def test_round_trip_returns_to_the_first_geometry(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    v2 = _deform(v, 7, jitter=0.02)
    gs.update(v2, i)
    gs.update(v, i)
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, f, _cases(pt)[:2])
    gs.update(v2, i, mode=pt.SCENE_UPDATE_REBUILD)
    gs.update(v, i, mode=pt.SCENE_UPDATE_REFIT)
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, f, _cases(pt)[:1])
    gs.close()


@pytest.mark.gpu
def test_update_is_ordered_after_an_async_render(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    film = pt.Film(gpu_ctx, W, H)
    pt.render(gs, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_WAVEFRONT, flags=pt.FLAG_ASYNC, **KW))
    gs.update(_deform(v, 8, jitter=0.03), i)        # no sync in between
    gpu_ctx.sync()
    want, wbgra, _ = _oracle(orc, orc.Scene(v, i, f), 2, **KW)
    assert film.read_f32().tobytes() == want.tobytes() and film.read_bgra8().tobytes() == wbgra.tobytes()
    film.close(); gs.close()


@pytest.mark.gpu
def test_update_refusals_leave_the_scene_alone_and_failed_rebuilds_repair(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    v2 = _deform(v, 9)
    L = pt.lib_amd()
    va = np.ascontiguousarray(v2, np.float32)
    ia = np.ascontiguousarray(i, np.uint32)
    ia_short = np.ascontiguousarray(ia[:-3])
    nv, nt = va.size // 3, ia.size // 3
    bad_idx = ia.copy()
    bad_idx[5] = nv
    calls = [(va.ctypes.data, nv, ia.ctypes.data, nt - 1, 0),          # wrong n_tris
             (va.ctypes.data, nv, ia_short.ctypes.data, nt - 1, 1),    # ... in either mode
             (va.ctypes.data, nv, bad_idx.ctypes.data, nt, 0),         # an index out of range
             (None, nv, ia.ctypes.data, nt, 0), (va.ctypes.data, nv, None, nt, 0),   # NULL arrays
             (va.ctypes.data, nv, ia.ctypes.data, nt, 2),              # an unknown mode
             (va.ctypes.data, 0, ia.ctypes.data, nt, 0)]               # no vertices
    for args in calls:
        assert L.pt_scene_update(gs.h, *args) == 1, args
    assert L.pt_scene_update(None, va.ctypes.data, nv, ia.ctypes.data, nt, 0) == 1
    with pytest.raises(pt.PtError) as e:
        gs.update(v2, ia_short)
    assert e.value.status == 1
    _check_pipelines(pt, orc, gpu_ctx, gs, v, i, f, _cases(pt)[:2])    # still the old geometry
    # an update whose rebuild fails: the scene is broken until its next use rebuilds it -- from the NEW triangles
    old = gpu_ctx.set_tuning(fail_rebuild=1)
    try:
        with pytest.raises(pt.PtError) as e:
            gs.update(v2, i, mode=pt.SCENE_UPDATE_REBUILD)
        assert e.value.status == 4
        assert gs.info().n_wide_nodes == 0
    finally:
        gpu_ctx.set_tuning(**old)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, [(pt.PIPELINE_WAVEFRONT, 0, False)])
    gs.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt)[:2])
    gs.close()


def _check_bvh4_leaves_lbvh(gs, v, i):
    """FAST_BUILD (the collapsed LBVH is traversed, bvh4_builder 0): every triangle inside its BVH4 leaf slot's box -- the leaf words
    name sorted positions of the LBVH, whose order pt_scene_read_bvh returns -- and every triangle in exactly one leaf."""
    assert gs.info().bvh4_builder == 0
    rows = gs.read_bvh4()
    _, prim, _ = gs.read_bvh()
    tri = np.asarray(v, np.float32).reshape(-1, 3)[np.asarray(i).reshape(-1, 3)]
    pl = rows[:, :24].copy().view(np.float32).reshape(-1, 6, 4)
    seen = np.zeros(len(prim), np.int64)
    for n in range(rows.shape[0]):
        for k in range(4):
            w = int(rows[n, 24 + k])
            if w == 0xFFFFFFFF or not (w & 0x80000000):
                continue
            first, cnt = w & 0x0FFFFFFF, ((w >> 28) & 7) + 1
            for pos in range(first, first + cnt):
                t = tri[prim[pos]]
                seen[prim[pos]] += 1
                assert (pl[n, 0:3, k] <= t.min(0)).all() and (pl[n, 3:6, k] >= t.max(0)).all(), (n, k, pos)
    assert (seen == 1).all()


@pytest.mark.gpu
def test_refit_without_a_pair_leaf_tree_then_fast_trace_uses_the_new_pairs(pt, orc, gpu_ctx, cornell_arrays):
    """Under FAST_BUILD no pair-leaf tree is held once a rebuild dropped it, so a refit that pulls a quad apart is allowed.  The surface-
    area tree a later FAST_TRACE builds must pair what the NEW arrays pair: same rows as a fresh scene's, same images as the oracle's."""
    v, i, f, first = _quads_in_cornell(cornell_arrays)
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)
    gs.update(v, i, mode=pt.SCENE_UPDATE_REBUILD)      # (the surface-area tree is not built again at FAST_BUILD)
    v2 = np.array(v, np.float32).reshape(-1, 3).copy()
    second = first + 2 * 2 + 1
    v2[int(np.asarray(i)[3 * second])] += np.float32([0.0, -0.05, 0.08])
    v2 = v2.reshape(-1)
    before = gs.read_bvh4()
    gs.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
    assert (gs.read_bvh4()[:, 24:] == before[:, 24:]).all()       # a refit: same LBVH collapse
    _check_bvh4_leaves_lbvh(gs, v2, i)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt)[:2])
    gs.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)
    fresh = pt.Scene(gpu_ctx, v2, i, f)
    assert gs.info().bvh4_builder == fresh.info().bvh4_builder == 1
    assert gs.read_bvh4().tobytes() == fresh.read_bvh4().tobytes()
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt))
    fresh.close(); gs.close()


@pytest.mark.gpu
def test_refit_under_fast_build_keeps_every_triangle_in_its_leaf(pt, orc, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)
    for seed in (11, 12):
        v2 = _deform(v, seed, jitter=0.03)
        gs.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
        _check_bvh4_leaves_lbvh(gs, v2, i)
    _check_pipelines(pt, orc, gpu_ctx, gs, v2, i, f, _cases(pt))
    gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("way_out", ["retry_update", "set_bvh_quality", "render"])
def test_failed_update_of_an_instanced_scene_keeps_its_instances(pt, orc, gpu_ctx, cornell_arrays, way_out):
    """An update of the instanced grid whose rebuild fails: the scene is broken, and every way out of that state -- another update, a
    pt_scene_set_bvh_quality, the next render's repair -- brings the 16 instances back with the new BLAS."""
    v, i, f = cornell_arrays
    grid = pt.cornell_grid_instances()[:16]
    cam = dict(cam_origin=(-0.88, -1.9, 0.5), cam_target=(-0.88, -1.9, 0.0))
    gs = pt.Scene(gpu_ctx, v, i, f)
    gs.set_instances(grid)
    v2 = _deform(v, 13)
    old = gpu_ctx.set_tuning(fail_rebuild=1)
    try:
        with pytest.raises(pt.PtError) as e:
            gs.update(v2, i, mode=pt.SCENE_UPDATE_REBUILD)
        assert e.value.status == 4
    finally:
        gpu_ctx.set_tuning(**old)
    want = v2
    if way_out == "retry_update":
        want = _deform(v, 14)
        gs.update(want, i, mode=pt.SCENE_UPDATE_REFIT)
    elif way_out == "set_bvh_quality":
        gs.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)
    if way_out != "render":
        assert gs.info().n_instances == 16
    _check_pipelines(pt, orc, gpu_ctx, gs, want, i, f, [(pt.PIPELINE_WAVEFRONT, 0, False), (pt.PIPELINE_AUTO, 0, False)],
                     instances=grid, **cam)
    assert gs.info().n_instances == 16
    gs.close()
