"""The PLOC rebuild of big scenes' binary trees (csrc/ploc_build.hip) on the GPU: the builder against its numpy restatement
(tests/ploc_ref.py; any valid tree returns the oracle's hits, so parity alone cannot see a wrong clustering), the structure of every adopted
tree, and adopted trees under everything that walks, reads or updates them -- the three HBM-class kernels, renders with NEE, ray sorting and
visit counting, pt_render_aov, pt_trace_device, pt_scene_update in both modes, and as the BLAS under instances.
Fixtures (tests/test_ploc_cpu.py checks, without a GPU, that each holds what it is here for): the 3394-triangle stadium, which the default
rule adopts; uniform soups of 2049 (one over the limit) and 2305 (9 x 256 + 1: the last block of k_ploc_nn holds one cluster) triangles and
a grid of 2304 equal tiles (every union area ties), which only ploc_adopt_pct = 1000 adopts."""
import contextlib

import numpy as np
import pytest

import knob_cases as kc
import ploc_ref as pr
import trace_device_cases as tc

pytestmark = pytest.mark.gpu
ADOPTED = [("stadium", -1), ("soup2305", 1000), ("tiles", 1000)]       # (fixture, ploc_adopt_pct) of the parity cases
WALK_RADII = (1, 8, 32)


@contextlib.contextmanager
def _built(pt, ctx, name, knobs):
    """-> (scene, vertices, indices, faces) of a fixture built under the knobs, which stay set for the length of the block: every build reads
    them -- the scene's creation, and also the rebuild behind the first request for the 8-wide nodes and behind SCENE_UPDATE_REBUILD"""
    v, i, f = pr.arrays(pt, name)
    with kc.tuning(ctx, knobs):
        gs = pt.Scene(ctx, v, i, f)
        try:
            yield gs, v, i, f
        finally:
            gs.close()


def _extends(pt):
    return (pt.EXTEND_AUTO, pt.EXTEND_HBM, pt.EXTEND_HBM8)


def _check_areas(info, ref, what):
    want_l, want_p = pr.info_value(ref["area_lbvh"], ref["root"]), pr.info_value(ref["area_ploc"], ref["root"])
    print(f"{what}: tree_area_lbvh {info.tree_area_lbvh!r} (restatement {want_l!r}), tree_area_ploc {info.tree_area_ploc!r} (restatement {want_p!r}), "
          f"ratio {info.tree_area_ploc / info.tree_area_lbvh:.4f} (restatement {ref['ratio']:.4f}), builder {info.bvh4_builder}")
    assert pr.within_one_ulp(info.tree_area_lbvh, want_l), (what, info.tree_area_lbvh, want_l)
    assert pr.within_one_ulp(info.tree_area_ploc, want_p), (what, info.tree_area_ploc, want_p)
    assert info.tree_area_ploc > 0


# ---- a. the builder against its restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", pr.RADII)
@pytest.mark.parametrize("name", pr.FIXTURES)
def test_area_sums_and_adoption_equal_the_restatement(pt, orc, gpu_ctx, name, radius):
    """tree_area_lbvh / tree_area_ploc == the restatement's sums through pt_scene_get_info's normalisation and float32 cast, within one
    float32 ulp: the two float64 summations differ only in their order (<= 4290 * 2^-53 relative), so only the final cast can land on the
    other side of a rounding boundary.  And for every ploc_adopt_pct the tree is adopted exactly when the restatement's ratio is below
    pct / 100 (tests/test_ploc_cpu.py: no ratio within 1e-3 of a threshold)."""
    ref = pr.fixture_reference(pt, orc, name, radius)
    for pct in pr.ADOPT_PCTS:
        with _built(pt, gpu_ctx, name, dict(ploc_radius=radius, ploc_adopt_pct=pct)) as (gs, _, _, _):
            info = gs.info()
            _check_areas(info, ref, f"{name} radius {radius} pct {pct}")
            want = pr.adopted(ref["area_ploc"], ref["area_lbvh"], pct)
            assert info.bvh4_builder == (2 if want else 0), (name, radius, pct, info.bvh4_builder, ref["ratio"])
            if pct == 1000:
                assert info.bvh4_builder == 2
            if pct == 0:
                assert info.bvh4_builder == 0


# ---- b. structure of every adopted tree ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", pr.RADII)
@pytest.mark.parametrize("name", pr.FIXTURES)
def test_adopted_tree_is_a_sound_tree(pt, orc, gpu_ctx, name, radius):
    """every triangle in exactly one BVH4 leaf, nested boxes, one parent per node, a sound 8-wide tree on top -- and the LBVH read-back
    still the oracle's, whatever is traversed"""
    from test_gpu_parity import _bvh4_facts, _check_bvh8, _leaf_cover
    with _built(pt, gpu_ctx, name, dict(ploc_radius=radius, ploc_adopt_pct=1000)) as (gs, v, i, f):
        nt = len(i) // 3
        info = gs.info()
        assert info.bvh4_builder == 2
        rows = gs.read_bvh4()
        assert rows.shape[0] == info.n_wide_nodes and (_leaf_cover(rows, nt) == 1).all()
        leaves, _, nested = _bvh4_facts(rows)
        assert nested and sum(((w >> 28) & 7) + 1 for w in leaves) == nt          # ... all of them reachable from node 0
        words = rows[:, 24:28]
        kids = words[(words != 0xFFFFFFFF) & (words & 0x80000000 == 0)]
        assert sorted(kids.tolist()) == list(range(1, rows.shape[0]))
        _check_bvh8(pt, gs, v.reshape(-1, 3)[i].reshape(-1), nt)
        osc = orc.Scene(v, i, f)
        keys, prim, nodes = gs.read_bvh()
        okeys, oprim = osc.bvh_keys()
        assert keys.tobytes() == okeys.tobytes() and prim.tobytes() == oprim.tobytes() and nodes.tobytes() == osc.bvh_nodes().tobytes()
        assert gs.info().bvh_height == osc.bvh_info().height and gs.info().bvh4_builder == 2


# ---- c. parity over adopted trees ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", WALK_RADII)
@pytest.mark.parametrize("name,pct", ADOPTED)
def test_adopted_tree_returns_the_oracles_hits_and_films(pt, orc, gpu_ctx, name, pct, radius):
    """20 000 rays (camera, incoherent, axis-parallel) through AUTO, HBM and the 8-wide kernel at both signs of tmin against the oracle's
    brute force; at radius 8 also the renders that read the per-triangle tables in the adopted tree's leaf order"""
    with _built(pt, gpu_ctx, name, dict(ploc_radius=radius, ploc_adopt_pct=pct)) as (gs, v, i, f):
        assert gs.info().bvh4_builder == 2
        rays, want = kc.oracle_traces(orc, name, v, i, f)
        kc.check_traces(pt, gs, rays, want, _extends(pt), (name, radius))
        if radius != 8:
            return
        film = kc.oracle_film(orc, name, v, i, f)
        kc.check_render(pt, gpu_ctx, gs, film, what=name)
        st = kc.check_render(pt, gpu_ctx, gs, film, flags=pt.FLAG_COUNT_VISITS, what=name)
        assert st.nodes_visited > 0 and st.tris_tested > 0
        kc.check_render(pt, gpu_ctx, gs, film, flags=pt.FLAG_SORT_RAYS, what=name)
        kc.check_render(pt, gpu_ctx, gs, kc.oracle_film(orc, name, v, i, f, nee=True), pipeline=pt.PIPELINE_WAVEFRONT_NEE, nee=True, what=name)


@contextlib.contextmanager
def _aov_case(pt, name):
    """tests/test_aov.py's helpers know their scenes by name: the fixture joins them for the length of the block"""
    import test_aov as ta
    case = "ploc_" + name
    old_arrays = ta._arrays
    ta._arrays = lambda pt_, scene: (pr.arrays(pt_, name) + (None,)) if scene == case else old_arrays(pt_, scene)
    ta.CASES[case] = (case, 48, 40, 4, {})
    try:
        yield ta, case
    finally:
        ta._arrays = old_arrays
        del ta.CASES[case]


@pytest.mark.parametrize("name,pct", ADOPTED)
def test_adopted_tree_under_render_aov(pt, orc, gpu_ctx, name, pct):
    """pt_render_aov reads albedo, normal, emission and ids through d_prim_of_sah: two frames equal tests/test_aov.py's definition"""
    with _built(pt, gpu_ctx, name, dict(ploc_adopt_pct=pct)) as (gs, _, _, _):
        assert gs.info().bvh4_builder == 2
        with _aov_case(pt, name) as (ta, case):
            want = ta._guides(pt, orc, case, [0, 1])
            assert 0.02 < float((want["alpha"] > 0).mean()) and want["albedo"].any() and want["normal"].any()
            for ext in ("EXTEND_AUTO", "EXTEND_HBM", "EXTEND_HBM8"):
                got, st = ta._run(pt, gpu_ctx, gs, case, [(0, 2)], pipeline=pt.PIPELINE_AUTO, extend=getattr(pt, ext))
                assert st.rays == ta._n_rays(case, 2)
                ta._same(got, want, (name, ext))


@pytest.mark.parametrize("name,pct", ADOPTED)
def test_adopted_tree_under_trace_device(pt, orc, gpu_ctx, name, pct):
    """pt_trace_device: CLOSEST with the surface outputs (position, normal, albedo, emission of the hit triangle) and ANY"""
    from test_trace_device import Query, _check_closest
    with _built(pt, gpu_ctx, name, dict(ploc_adopt_pct=pct)) as (gs, v, i, f):
        rays = np.ascontiguousarray(kc.make_rays(v, n=1000, seed=41, n_axis=40))
        ans = tc.answers("ploc_" + name, lambda: tc.Answers(orc.Scene(v, i, f), f, rays))
        q = Query(pt, gpu_ctx, rays, ans.bounds)
        try:
            assert gs.info().bvh4_builder == 2
            assert 0.1 < ans.hit_share(1000) < 0.98 and 0.02 < ans.occ_share(1000) < 0.98, (ans.hit_share(1000), ans.occ_share(1000))
            for ext in _extends(pt):
                _check_closest(ans, 1000, q.closest(gs, 1000, extend=ext), (name, ext))
                assert (q.any(gs, 1000, extend=ext) == ans.occ_cycled).all(), (name, ext)
                assert (q.any(gs, 1000, per_ray=False, tmax=ans.uniform_bound, extend=ext) == ans.occ_uniform).all(), (name, ext)
        finally:
            q.close()


# ---- d. update of an adopted tree -----------------------------------------------------------------------------------------------------
def _jitter(v, seed):
    rng = np.random.default_rng(seed)
    return (np.asarray(v, np.float32).reshape(-1, 3) + rng.uniform(-0.03, 0.03, (len(v) // 3, 3)).astype(np.float32)).reshape(-1).astype(np.float32)


@pytest.mark.parametrize("name,pct", ADOPTED[:2])
def test_refit_of_an_adopted_tree(pt, orc, gpu_ctx, name, pct):
    """SCENE_UPDATE_REFIT keeps the adopted tree: same builder, same child words of the 8-wide nodes, a sound tree around the new positions,
    tree_area_ploc kept (include/pt_api.h: the PLOC tree's binary form is not held after the collapse) and tree_area_lbvh recomputed for the
    REFITTED LBVH -- the old sorted order and child words around the new triangles, which tests/ploc_ref.py refit_lbvh restates from the
    oracle's LBVH of the OLD arrays.  (The oracle's LBVH of the NEW arrays is another tree, the one a rebuild makes, and its sum is not
    what a refit reports: measured on the MI355X for the stadium, 22.67364 refitted against 26.919401 rebuilt.)"""
    from test_gpu_parity import _check_bvh8
    with _built(pt, gpu_ctx, name, dict(ploc_adopt_pct=pct)) as (gs, v, i, f):
        nt = len(i) // 3
        words8 = gs.read_bvh8()[0][:, 14:16].copy()
        before = gs.info()
        assert before.bvh4_builder == 2
        v2 = _jitter(v, 51)
        gs.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
        info = gs.info()
        assert info.bvh4_builder == 2
        assert (gs.read_bvh8()[0][:, 14:16] == words8).all()
        _check_bvh8(pt, gs, v2.reshape(-1, 3)[i].reshape(-1), nt)
        assert info.tree_area_ploc > 0
        osc_old = orc.Scene(v, i, f)
        rows, area = pr.refit_lbvh(osc_old.bvh_nodes(), osc_old.bvh_keys()[1], v2, i)
        assert gs.read_bvh()[2].tobytes() == rows.tobytes()
        nb = orc.Scene(v2, i, f).bvh_info()
        root = pr.root_area(list(nb.bbox_min), list(nb.bbox_max))
        assert list(info.bbox_min) == list(nb.bbox_min) and list(info.bbox_max) == list(nb.bbox_max)
        want_l = pr.info_value(area, root)
        # the PLOC sum is kept; the value reported divides it by the NEW box's area
        old_root = pr.root_area(list(before.bbox_min), list(before.bbox_max))
        ref = pr.fixture_reference(pt, orc, name, -1)
        want_p = pr.info_value(ref["area_ploc"], root)
        print(f"{name} refitted: tree_area_lbvh {info.tree_area_lbvh!r} (restatement {want_l!r}; before {before.tree_area_lbvh!r}), tree_area_ploc "
              f"{info.tree_area_ploc!r} (kept sum over the new box {want_p!r}; before {before.tree_area_ploc!r}), box areas {old_root!r} -> {root!r}")
        assert pr.within_one_ulp(info.tree_area_lbvh, want_l), (info.tree_area_lbvh, want_l)
        assert pr.within_one_ulp(info.tree_area_ploc, want_p), (info.tree_area_ploc, want_p)
        rays, want = kc.oracle_traces(orc, (name, "jitter51"), v2, i, f)
        kc.check_traces(pt, gs, rays, want, _extends(pt), (name, "refit"))
        kc.check_render(pt, gpu_ctx, gs, kc.oracle_film(orc, (name, "jitter51"), v2, i, f), what=(name, "refit"))


@pytest.mark.parametrize("name,pct", ADOPTED[:2])
def test_rebuild_of_an_adopted_tree_equals_a_fresh_scene(pt, orc, gpu_ctx, name, pct):
    v, i, f = pr.arrays(pt, name)
    v2 = _jitter(v, 51)
    with kc.tuning(gpu_ctx, dict(ploc_adopt_pct=pct)):          # the rebuild reads the rule as the build did
        gs, fresh = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v2, i, f)
        try:
            assert gs.info().bvh4_builder == 2
            gs.update(v2, i, mode=pt.SCENE_UPDATE_REBUILD)
            a, b = gs.info(), fresh.info()
            for field in ("n_wide_nodes", "bvh4_builder", "bvh_height", "tree_area_lbvh", "tree_area_ploc"):
                assert getattr(a, field) == getattr(b, field), field
            ref = pr.reference(orc, v2, i, f, 8)
            _check_areas(a, ref, f"{name} rebuilt")
            if abs(ref["ratio"] - 0.01 * pr.tuned(pct, 90, 0, 1000)) >= 1e-3:
                assert a.bvh4_builder == (2 if pr.adopted(ref["area_ploc"], ref["area_lbvh"], pct) else 0)
            assert gs.read_bvh4().tobytes() == fresh.read_bvh4().tobytes()
            for x, y in zip(gs.read_bvh(), fresh.read_bvh()):
                assert x.tobytes() == y.tobytes()
            for x, y in zip(gs.read_bvh8(), fresh.read_bvh8()):
                assert x.tobytes() == y.tobytes()
            rays, want = kc.oracle_traces(orc, (name, "jitter51"), v2, i, f)
            kc.check_traces(pt, gs, rays, want, _extends(pt), (name, "rebuild"))
            kc.check_render(pt, gpu_ctx, gs, kc.oracle_film(orc, (name, "jitter51"), v2, i, f), what=(name, "rebuild"))
        finally:
            fresh.close(); gs.close()


# ---- e. an adopted tree as a BLAS -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inst,seed", [(1, 1), (3, 2), (60, 4)])
def test_adopted_tree_as_a_blas_under_instances(pt, orc, gpu_ctx, n_inst, seed):
    """the stadium's PLOC tree below a TLAS (3394 triangles: the general two-level kernel): traces and a render equal the oracle's"""
    from test_gpu_parity import _random_instances
    inst = _random_instances(n_inst, seed)
    with _built(pt, gpu_ctx, "stadium", dict()) as (gs, v, i, f):
        assert gs.info().bvh4_builder == 2
        gs.set_instances(inst)
        assert gs.info().n_instances == n_inst
        rng = np.random.default_rng(seed + 100)
        n = 20000
        org = rng.uniform(-3, 3, (n, 3)).astype(np.float32) + np.float32([0, -1, 0])
        tgt = inst[rng.integers(0, n_inst, n), :, 3] + rng.uniform(-0.4, 0.4, (n, 3)).astype(np.float32)
        d = tgt - org
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.ascontiguousarray(np.concatenate([org, d.astype(np.float32)], 1), np.float32)
        rays, want = kc.oracle_traces(orc, ("stadium_inst", n_inst), v, i, f, instances=inst, mode=1, rays=rays, hit_range=(0.2, 1.01))
        kc.check_traces(pt, gs, rays, want, (pt.EXTEND_AUTO,), ("stadium", n_inst))
        kc.check_render(pt, gpu_ctx, gs, kc.oracle_film(orc, ("stadium_inst", n_inst), v, i, f, instances=inst), what=("stadium", n_inst))
        kc.check_render(pt, gpu_ctx, gs, kc.oracle_film(orc, ("stadium_inst", n_inst), v, i, f, instances=inst), pipeline=pt.PIPELINE_AUTO,
                        what=("stadium", n_inst, "auto"))
