"""The pt_tuning knobs that select code no other test reaches -- topdown4, rec64, hbm8, sort_bits, stagger, inst16_blocks -- each set off its
default and held against the CPU oracle: hit records at both signs of tmin and a 96 x 64, 4 spp, depth 6, two-frame film (float film, rgba8
image, ray count).  ploc_radius / ploc_adopt_pct are tests/test_ploc_trees.py's, tlas_ploc tests/test_tlas_ploc.py's.  The meta-test at the
end (no GPU) keeps the gap closed: every name of TUNING_NAMES must be set by some test."""
import ast
import glob
import os

import pytest

import knob_cases as kc
import ploc_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))


def _scene_arrays(pt, name, cornell_arrays):
    if name == "cornell":
        return cornell_arrays
    if name == "stadium":
        return pr.arrays(pt, "stadium")
    return kc.cached(("arrays", name), lambda: pr.soup({"soup3000": 3000, "soup16000": 16000}[name], {"soup3000": 21, "soup16000": 23}[name], 0.05))


def _traces(orc, name, v, i, f):
    # (brute force where it takes a second; the 16 000-triangle soup through the oracle's own tree)
    return kc.oracle_traces(orc, ("knobs", name), v, i, f, mode=0 if len(i) // 3 < 4000 else 1)


# ---- topdown4 / rec64: the HBM kernel over d_wide16 and its 48-B-record instantiations ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [dict(topdown4=0), dict(rec64=0), dict(topdown4=0, rec64=0)], ids=["topdown4_off", "rec64_off", "both_off"])
@pytest.mark.parametrize("name", ["soup3000", "stadium"])
def test_hbm_kernel_without_the_topdown_copy_and_with_48_byte_records(pt, orc, gpu_ctx, cornell_arrays, name, knobs):
    """topdown4 = 0: the collapsed tree's fp16 copy instead of the top-down one, with the other stack bound; rec64 = 0: leaves from the 48-B
    records.  The soup walks its LBVH, the stadium an adopted PLOC tree.  Beside the plain render: the counting instantiations
    (FLAG_COUNT_VISITS), the per-ray tmax path (NEE) and the permuted queue (FLAG_SORT_RAYS)."""
    v, i, f = _scene_arrays(pt, name, cornell_arrays)
    with kc.tuning(gpu_ctx, knobs):
        gs = pt.Scene(gpu_ctx, v, i, f)
        try:
            assert gs.info().bvh4_builder == (2 if name == "stadium" else 0)
            rays, want = _traces(orc, name, v, i, f)
            kc.check_traces(pt, gs, rays, want, (pt.EXTEND_AUTO, pt.EXTEND_HBM), (name, knobs))
            film = kc.oracle_film(orc, ("knobs", name), v, i, f)
            for flags in (0, pt.FLAG_COUNT_VISITS, pt.FLAG_SORT_RAYS):
                st = kc.check_render(pt, gpu_ctx, gs, film, flags=flags, what=(name, knobs))
                assert st.extend_variant == pt.EXTEND_HBM
                if flags == pt.FLAG_COUNT_VISITS:
                    assert st.nodes_visited > 0 and st.tris_tested > 0
            st = kc.check_render(pt, gpu_ctx, gs, kc.oracle_film(orc, ("knobs", name), v, i, f, nee=True), pipeline=pt.PIPELINE_WAVEFRONT_NEE,
                                 nee=True, what=(name, knobs))
            assert st.extend_variant == pt.EXTEND_HBM
        finally:
            gs.close()


# ---- hbm8: AUTO's choice between the BVH4 kernel and the 8-wide tree -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,knobs,variant,built_at_create", [("soup16000", dict(hbm8=0), "EXTEND_HBM", False), ("soup3000", dict(hbm8=1), "EXTEND_HBM8", True),
                                                                ("cornell", dict(hbm8=1), "EXTEND_LDS", True), ("soup16000", dict(), "EXTEND_HBM8", True)],
                         ids=["big_off", "mid_on", "cornell_on", "big_default"])
def test_hbm8_moves_autos_choice_and_no_bit(pt, orc, gpu_ctx, cornell_arrays, name, knobs, variant, built_at_create):
    v, i, f = _scene_arrays(pt, name, cornell_arrays)
    with kc.tuning(gpu_ctx, knobs):
        gs = pt.Scene(gpu_ctx, v, i, f)
        try:
            assert (gs.info().n_wide8_nodes > 0) == built_at_create          # (small scenes always have their few KB of 8-wide nodes)
            rays, want = _traces(orc, name, v, i, f)
            kc.check_traces(pt, gs, rays, want, (pt.EXTEND_AUTO,), (name, knobs))
            st = kc.check_render(pt, gpu_ctx, gs, kc.oracle_film(orc, ("knobs", name), v, i, f), what=(name, knobs))
            assert st.extend_variant == getattr(pt, variant), (name, knobs, st.extend_variant)
        finally:
            gs.close()


# ---- sort_bits: 6 .. 30-bit keys, 1, 2, 3 and 4 radix passes -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pipes", [1, 2])
@pytest.mark.parametrize("extend", [3, 4])
def test_ray_sort_key_widths_change_no_bit(pt, orc, gpu_ctx, cornell_arrays, extend, pipes):
    v, i, f = _scene_arrays(pt, "soup16000", cornell_arrays)
    gs = pt.Scene(gpu_ctx, v, i, f)
    try:
        film = kc.oracle_film(orc, ("knobs", "soup16000"), v, i, f)
        for bits in (1, 2, 5, 7, 8, 9):
            with kc.tuning(gpu_ctx, dict(sort_bits=bits, pipes=pipes)):
                st = kc.check_render(pt, gpu_ctx, gs, film, flags=pt.FLAG_SORT_RAYS, extend=extend, what=(bits, extend, pipes))
                assert st.extend_variant == extend and st.pipelines == pipes
    finally:
        gs.close()


# ---- stagger: the start rule and the shade rule of 2 and 3 pipelines -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pipes", [2, 3])
@pytest.mark.parametrize("stagger", [0, 1, 2])
@pytest.mark.parametrize("name", ["cornell", "soup3000"])
def test_stagger_rules_change_no_bit(pt, orc, gpu_ctx, cornell_arrays, name, stagger, pipes):
    v, i, f = _scene_arrays(pt, name, cornell_arrays)
    gs = pt.Scene(gpu_ctx, v, i, f)
    try:
        film = kc.oracle_film(orc, ("knobs", name), v, i, f)
        with kc.tuning(gpu_ctx, dict(stagger=stagger, pipes=pipes)):
            st = kc.check_render(pt, gpu_ctx, gs, film, what=(name, stagger, pipes))
            assert st.pipelines == pipes, (st.pipelines, pipes)
            rays, want = _traces(orc, name, v, i, f)
            kc.check_traces(pt, gs, rays, want, (pt.EXTEND_AUTO,), (name, stagger, pipes))
    finally:
        gs.close()


# ---- inst16_blocks: the grid of the compact two-level kernel, which is also its spill stride --------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 8])
def test_inst16_grid_size_changes_no_bit(pt, orc, gpu_ctx, cornell_arrays, blocks):
    from test_gpu_parity import _random_instances
    from test_tlas_ploc import _rays
    v, i, f = cornell_arrays
    inst = _random_instances(60, 4)
    with kc.tuning(gpu_ctx, dict(inst16_blocks=blocks)):
        gs = pt.Scene(gpu_ctx, v, i, f)
        try:
            gs.set_instances(inst)
            rays, want = kc.oracle_traces(orc, ("knobs", "inst60"), v, i, f, instances=inst, mode=1, rays=_rays(inst, 78), hit_range=(0.2, 1.01))
            kc.check_traces(pt, gs, rays, want, (pt.EXTEND_AUTO,), blocks)
            film = kc.oracle_film(orc, ("knobs", "inst60"), v, i, f, instances=inst)
            kc.check_render(pt, gpu_ctx, gs, film, what=blocks)
            kc.check_render(pt, gpu_ctx, gs, film, flags=pt.FLAG_COUNT_VISITS, what=blocks)
            kc.check_render(pt, gpu_ctx, gs, kc.oracle_film(orc, ("knobs", "inst60"), v, i, f, instances=inst, nee=True),
                            pipeline=pt.PIPELINE_WAVEFRONT_NEE, nee=True, what=blocks)
        finally:
            gs.close()


# ---- so that the gap stays closed (no GPU) -----------------------------------------------------------------------------------------------------
# name -> why no test sets it.  Empty: every knob is set somewhere.
NOT_SET_BY_ANY_TEST = {}


def _knob_names_set_in(path):
    """keywords of every set_tuning(...) call, and of every dict(...) call in a file that passes a dict on to set_tuning / kc.tuning"""
    tree = ast.parse(open(path).read(), path)
    names, dict_names, forwards = set(), set(), False
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call):
            continue
        fn = node.func.attr if isinstance(node.func, ast.Attribute) else getattr(node.func, "id", None)
        if fn == "set_tuning":
            names |= {k.arg for k in node.keywords if k.arg}
            forwards |= any(k.arg is None for k in node.keywords)
        elif fn == "tuning" and node.args[1:]:
            forwards = True
        elif fn == "dict":
            dict_names |= {k.arg for k in node.keywords if k.arg}
    return names | (dict_names if forwards else set())


def test_every_tuning_knob_is_set_by_some_test(pt):
    """Scans the test sources for knob names only: every name in TUNING_NAMES is a keyword of a set_tuning(...) call or of a dict(...) in a
    test file that hands dicts to it, or is listed above with its reason."""
    found = set()
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        found |= _knob_names_set_in(path)
    missing = [n for n in pt.TUNING_NAMES if n not in found and n not in NOT_SET_BY_ANY_TEST]
    assert not missing, missing
    stale = [n for n in NOT_SET_BY_ANY_TEST if n in found or n not in pt.TUNING_NAMES]
    assert not stale, stale
    assert "reserved" not in pt.TUNING_NAMES
