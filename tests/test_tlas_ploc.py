"""pt_tuning.tlas_ploc = 1: the TLAS's binary tree rebuilt by PLOC (csrc/scene_build.hip ptb_set_instances -> ptb_build_bvh(..., ploc)), which
no other test switches on.  Over the Cornell box as BLAS (it lives in LDS, so inst16 on / off gives the compact and the general two-level
kernel): ordinary instance sets, the default adoption rule and a forced one, traces at both signs of tmin and renders through the wavefront,
NEE and AUTO (fused instanced) pipelines, all against the CPU oracle; a witness that the knob changes the tree that is walked; and the way
back -- pt_scene_set_instances with the knob off again, pt_scene_update of the BLAS in both modes."""
import numpy as np
import pytest

import knob_cases as kc

pytestmark = pytest.mark.gpu
SETS = ["two", "three", "sixty", "many", "stadium"]


def _stadium_layout(seed=9):
    """4 instances scaled x 20 around 200 scaled x 0.05 that cluster in one corner: instance sizes over 2.6 orders of magnitude"""
    rng = np.random.default_rng(seed)
    m = np.zeros((204, 3, 4), np.float32)
    for k in range(204):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        big = k < 4
        m[k, :, :3] = (q * (20.0 if big else 0.05)).astype(np.float32)
        m[k, :, 3] = (rng.uniform(-30, 30, 3) if big else np.float32([1.2, -0.3, 1.0]) + rng.uniform(-0.5, 0.5, 3)).astype(np.float32)
    return m


def _instances(name):
    from test_gpu_parity import _random_instances
    return kc.cached(("tlas_set", name), lambda: {"two": lambda: _random_instances(2, 2), "three": lambda: _random_instances(3, 3),
                                                  "sixty": lambda: _random_instances(60, 4), "many": lambda: _random_instances(1500, 5),
                                                  "stadium": _stadium_layout}[name]())


def _rays(inst, seed, n=20000):
    """the recipe of test_instanced_trace_and_render_bit_exact: origins around the origin, aimed at the instances' translations"""
    rng = np.random.default_rng(seed)
    org = rng.uniform(-3, 3, (n, 3)).astype(np.float32) + np.float32([0, -1, 0])
    tgt = inst[rng.integers(0, len(inst), n), :, 3] + rng.uniform(-0.4, 0.4, (n, 3)).astype(np.float32)
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([org, d.astype(np.float32)], 1), np.float32)


def _check_everything(pt, orc, ctx, gs, key, arrays, inst, what):
    v, i, f = arrays
    rays, want = kc.oracle_traces(orc, key, v, i, f, instances=inst, mode=1, rays=_rays(inst, 77), hit_range=(0.2, 1.01))
    kc.check_traces(pt, gs, rays, want, (pt.EXTEND_AUTO,), what)
    film = kc.oracle_film(orc, key, v, i, f, instances=inst)
    kc.check_render(pt, ctx, gs, film, pipeline=pt.PIPELINE_WAVEFRONT, what=what)
    kc.check_render(pt, ctx, gs, film, pipeline=pt.PIPELINE_AUTO, what=what)
    kc.check_render(pt, ctx, gs, kc.oracle_film(orc, key, v, i, f, instances=inst, nee=True), pipeline=pt.PIPELINE_WAVEFRONT_NEE, nee=True, what=what)


@pytest.mark.parametrize("adopt", [dict(), dict(ploc_adopt_pct=1000)], ids=["default_rule", "forced"])
@pytest.mark.parametrize("inst16", [dict(), dict(inst16=0)], ids=["inst16", "general"])
@pytest.mark.parametrize("name", SETS)
def test_tlas_ploc_keeps_every_bit(pt, orc, gpu_ctx, cornell_arrays, name, inst16, adopt):
    inst = _instances(name)
    with kc.tuning(gpu_ctx, dict(tlas_ploc=1, **inst16, **adopt)):
        gs = pt.Scene(gpu_ctx, *cornell_arrays)
        try:
            gs.set_instances(inst)
            info = gs.info()
            assert info.n_instances == len(inst) and info.n_tlas_nodes >= 1
            _check_everything(pt, orc, gpu_ctx, gs, ("tlas", name), cornell_arrays, inst, (name, inst16, adopt))
        finally:
            gs.close()


def _visits(pt, ctx, cornell_arrays, inst, knobs):
    with kc.tuning(ctx, knobs):
        gs = pt.Scene(ctx, *cornell_arrays)
        try:
            gs.set_instances(inst)
            film, _, st = kc.render(pt, ctx, gs, flags=pt.FLAG_COUNT_VISITS)
            return film.tobytes(), st.rays, st.nodes_visited, gs.info().n_tlas_nodes
        finally:
            gs.close()


@pytest.mark.parametrize("inst16", [dict(), dict(inst16=0)], ids=["inst16", "general"])
def test_tlas_ploc_changes_the_tree_that_is_walked_and_two_instances_keep_the_lbvh(pt, gpu_ctx, cornell_arrays, inst16):
    """pt_scene_info has no TLAS area fields, so the witness is the walk: on the stadium layout with forced adoption a counted render visits
    another number of nodes than with the knob off -- same film, same rays.  Two instances (n > 2 is false) keep the LBVH: the same count."""
    inst = _instances("stadium")
    off = _visits(pt, gpu_ctx, cornell_arrays, inst, dict(tlas_ploc=0, **inst16))
    on = _visits(pt, gpu_ctx, cornell_arrays, inst, dict(tlas_ploc=1, ploc_adopt_pct=1000, **inst16))
    print(f"stadium layout {inst16}: nodes_visited {off[2]} (LBVH TLAS, {off[3]} nodes) / {on[2]} (PLOC TLAS, {on[3]} nodes)")
    assert on[:2] == off[:2] and off[2] > 0
    assert on[2] != off[2], (on[2:], off[2:])
    two = _instances("two")
    off = _visits(pt, gpu_ctx, cornell_arrays, two, dict(tlas_ploc=0, **inst16))
    on = _visits(pt, gpu_ctx, cornell_arrays, two, dict(tlas_ploc=1, ploc_adopt_pct=1000, **inst16))
    assert on == off


@pytest.mark.parametrize("knob_at_update", [0, 1])
@pytest.mark.parametrize("name", ["sixty", "stadium"])
def test_tlas_ploc_then_new_instances_and_blas_updates(pt, orc, gpu_ctx, cornell_arrays, name, knob_at_update):
    """A scene whose TLAS was built by PLOC, then: the same instances set again with the knob off (an LBVH TLAS replaces it), the BLAS
    refitted and rebuilt (the TLAS is made again from the stored transforms under whatever the knob says then).  The oracle's bits throughout."""
    from test_scene_update import _deform
    v, i, f = cornell_arrays
    inst = _instances(name)
    with kc.tuning(gpu_ctx, dict(tlas_ploc=1, ploc_adopt_pct=1000)):
        gs = pt.Scene(gpu_ctx, v, i, f)
        gs.set_instances(inst)
    try:
        kc.check_render(pt, gpu_ctx, gs, kc.oracle_film(orc, ("tlas", name), v, i, f, instances=inst), what=(name, "ploc tlas"))
        assert gpu_ctx.tuning().tlas_ploc != 1
        gs.set_instances(inst)
        _check_everything(pt, orc, gpu_ctx, gs, ("tlas", name), cornell_arrays, inst, (name, "set again, knob off"))
        for mode, seed in ((pt.SCENE_UPDATE_REFIT, 61), (pt.SCENE_UPDATE_REBUILD, 62)):
            v2 = _deform(v, seed)
            with kc.tuning(gpu_ctx, dict(tlas_ploc=knob_at_update, ploc_adopt_pct=1000)):
                gs.update(v2, i, mode=mode)
            assert gs.info().n_instances == len(inst)
            _check_everything(pt, orc, gpu_ctx, gs, ("tlas", name, seed), (v2, i, f), inst, (name, "update", mode, knob_at_update))
    finally:
        gs.close()
