"""The radiance path at the edges of material and environment values: zero, -0.0, denormal, tiny, negative, huge and overflowing
Kd / Ke / env through every shading body, against the CPU oracle (oracle/pt_oracle.c), which defines the film for any finite
material.  The geometry is what other tests already render (the Cornell box, five instances of it, a 300-triangle soup); only the
numbers in the material table and in `env` change.

Family A tables cannot overflow at max_depth <= 6: the film must be the oracle's byte for byte.  Family B tables and environments
overflow, so the arithmetic generates infinities and NaNs (inf * 0, inf - inf): the NaN positions must agree and every other
value must be bit-equal (`material_tables.assert_same`).  No NaN is ever an input.  The CPU tests check, on the oracle's films alone, that every
fixture a GPU test renders holds the kinds of value it is there for."""
import importlib
import os

import numpy as np
import pytest

from test_gpu_parity import _random_instances, _soup
from test_denoise_variance import _moments_ref
import test_aov

from material_tables import (ENV_GUARD, ENV_HUGE, ENV_INF, ENV_MIXED, ENV_TINY, GUARD_HI, GUARD_LO, INF, SIDE_CAM, assert_same, f32, table_a,
                             table_b, table_g, u32)

W, H, SPP, DEPTH = 64, 48, 4, 6
KW = dict(width=W, height=H, spp_per_frame=SPP, max_depth=DEPTH)


# ---- material tables (material_tables.py) by (family, seed) ---------------------------------------------------------------------
def _table(spec, n):
    kind, seed = spec
    return {"A": table_a, "B": table_b, "G": table_g, "A_all_emit": lambda n, s: table_a(n, s, all_emit=True)}[kind](n, seed)


# ---- the cases: every (geometry, table, env, estimator, camera, frames) a GPU test renders --------------------------------------
# band: the conditions test_fixture_holds_the_values_it_is_there_for puts on the oracle's film (BANDS below)
INST_SEED, SOUP_SEED = 3, 5


def _case(geom, table, env, band, nee=0, cam=None, frames=2):
    return dict(geom=geom, table=table, env=env, band=band, nee=nee, cam=cam or {}, frames=frames)


CASES = {
    "cornell_a": _case("cornell", ("A", 4), ENV_MIXED, "A"),
    "cornell_a_3f": _case("cornell", ("A", 4), ENV_MIXED, "A", frames=3),
    "cornell_a_side": _case("cornell", ("A", 4), ENV_TINY, "A_side", cam=SIDE_CAM),
    "cornell_all_emit": _case("cornell", ("A_all_emit", 4), ENV_TINY, "A"),
    "cornell_nee_a": _case("cornell", ("A", 12), ENV_MIXED, "A", nee=1),
    "inst_a": _case("inst", ("A", 4), ENV_MIXED, "A"),
    "inst_nee_a": _case("inst", ("A", 12), ENV_MIXED, "A", nee=1),
    "soup_a": _case("soup", ("A", 5), ENV_MIXED, "A"),
    "soup_nee_a": _case("soup", ("A", 5), ENV_MIXED, "A", nee=1),
    "cornell_guard": _case("cornell", ("G", 1), ENV_GUARD, "G"),
    "cornell_b": _case("cornell", ("B", 15), ENV_MIXED, "B"),
    "cornell_b_3f": _case("cornell", ("B", 15), ENV_MIXED, "B", frames=3),
    "cornell_huge_env": _case("cornell", ("A", 4), ENV_HUGE, "huge_env"),
    "cornell_inf_env": _case("cornell", ("A", 4), ENV_INF, "inf_env"),
    "cornell_inf_env_side": _case("cornell", ("A", 4), ENV_INF, "inf_env", cam=SIDE_CAM),
    "cornell_nee_b": _case("cornell", ("B", 38), ENV_MIXED, "B", nee=1),
    "inst_b": _case("inst", ("B", 30), ENV_MIXED, "B"),
    "inst_nee_b": _case("inst", ("B", 44), ENV_MIXED, "B", nee=1),
    "soup_b": _case("soup", ("B", 5), ENV_MIXED, "B"),
    "soup_nee_b": _case("soup", ("B", 5), ENV_MIXED, "B", nee=1),
}
_arrays_cache, _oracle_cache = {}, {}


def _exact(case):
    """family A cases compare bytes; the others normalise generated NaNs first"""
    return CASES[case]["band"][0] in "AG"


def _arrays(pt, case):
    """-> (vertices, indices, faces [n, 6], instances or None) of a case"""
    c = CASES[case]
    key = (c["geom"], c["table"])
    if key not in _arrays_cache:
        inst = None
        if c["geom"] == "soup":
            v, i, _ = _soup(300, SOUP_SEED, spread=0.35)
            v = (v.reshape(-1, 3) + f32([0.0, -1.0, 0.0])).astype(f32).reshape(-1)
        else:
            v, i, _ = pt.load_obj(pt.ASSET_CORNELL)
            if c["geom"] == "inst":
                inst = _random_instances(5, INST_SEED)
        faces = _table(c["table"], len(i) // 3)
        for a in (v, i, faces):
            a.flags.writeable = False
        _arrays_cache[key] = (v, i, faces, inst)
    return _arrays_cache[key]


def _params_kw(case):
    c = CASES[case]
    return dict(KW, env=c["env"], **c["cam"])


def _oracle(pt, orc, case, mode=1):
    """-> (film after every frame [frames][H, W, 3], bgra8 after every frame, rays after every frame, frame colours): the oracle's
    answer for a case, rendered once and shared (read-only).  mode 1: the LBVH walk, 0: brute force over all triangles."""
    key = (case, mode)
    if key not in _oracle_cache:
        c = CASES[case]
        v, i, faces, inst = _arrays(pt, case)
        osc = orc.Scene(v, i, faces.reshape(-1))
        if inst is not None:
            osc.set_instances(inst)
        film, bgra, rays = np.zeros((H, W, 3), f32), np.zeros((H, W, 4), np.uint8), 0
        films, bgras, rayss, colours = [], [], [], []
        for k in range(c["frames"]):
            img, r, _, _ = osc.render_frame(orc.default_params(frame=k, nee=c["nee"], **_params_kw(case)), mode=mode,
                                            nthreads=min(16, os.cpu_count() or 1))
            orc.accumulate_f32(film, img, k)
            orc.accumulate_bgra8(bgra, img, k)
            rays += r
            films.append(film.copy()); bgras.append(bgra.copy()); rayss.append(rays); colours.append(img)
        for a in films + bgras + colours:
            a.flags.writeable = False
        _oracle_cache[key] = (films, bgras, rayss, colours)
    return _oracle_cache[key]


def _oracle_film(pt, orc, case, mode=1):
    """-> (film, bgra8, rays) after the case's last frame"""
    films, bgras, rayss, _ = _oracle(pt, orc, case, mode)
    return films[-1], bgras[-1], rayss[-1]


# ---- the comparison rule --------------------------------------------------------------------------------------------------------
def _assert_same(case, what, got, want, exact=None):
    """material_tables.assert_same by the case's family: family A (and the guard table) compares bytes, the others normalise NaNs"""
    assert_same(case, what, got, want, _exact(case) if exact is None else exact)


def _assert_image(case, what, got, want):
    assert got.dtype == np.uint8 and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        y, x, ch = (int(k) for k in np.argwhere(got != want)[0])
        raise AssertionError(f"{case}, {what}: bgra8 differs at pixel ({x}, {y}) byte {ch}: got {int(got[y, x, ch])}, oracle {int(want[y, x, ch])}")


# ---- without a GPU: the fixtures do what they are for ---------------------------------------------------------------------------
def _shares(film):
    """shares of a film's values by kind (below_2m100: of the non-zero values)"""
    a = np.abs(film.astype(np.float64))
    fin = np.isfinite(film)
    nz = fin & (a > 0)
    return dict(nan=float(np.isnan(film).mean()), inf=float(np.isinf(film).mean()), denormal=float((nz & (a < 2.0 ** -126)).mean()),
                below_2m100=float((nz & (a < 2.0 ** -100)).sum() / max(1, int((film != 0).sum()))),
                negative=float((film < 0).mean()), zero=float((film == 0).mean()), ordinary=float(((a > 1e-3) & (a < 1e3)).mean()),
                big=float((fin & (a > 2.0 ** 100)).mean()))


# name -> {kind: (at least, at most)}.  "A" and "B" are the issue's conditions, "huge_env" the band it grants the huge-env case: a family
# A table under a finite env that overflows at the second add, so most pixels that see the sky are infinite in two channels and denormal
# in the third.  Two kinds of case CANNOT meet their family's band, whatever the seed, and have one of their own with the same kind of
# margin under what the oracle gives:
# "A_side" (family A asks negative >= 20 %, ordinary >= 35 %): the box fills a third of the image and every other pixel is exactly
# ENV_TINY, (+0, +0, 1e-44) -- what the cull's host-made sum of a -0.0 and of a denormal is tested on -- so half of the values are zero
# and the negative and ordinary ones come from the box alone: 15.8 % and 15.5 % of the values (denormal 24.6 %, zero 51.8 %).
# "inf_env" (family B asks NaN <= 10 %, ordinary >= 30 %, finite above 2^100 >= 2 %): the table is a family A one, so nothing finite is
# large, and every path that reaches the sky adds (w * inf, w * 0.5, w * -inf): a zero weight gives inf * 0, weights of both signs in one
# pixel inf - inf, so about half of the R and B values of the pixels that see the box are NaN for every seed (seeds 1 .. 15: 25 - 35 % of
# all values); the G channel stays finite.  Front view: NaN 32.2 %, inf 34.2 %, ordinary 27.0 %; side view: 20.6 %, 45.9 %, 30.9 %.
BANDS = {
    "A": dict(nan=(0, 0), inf=(0, 0), denormal=(0.01, 1), below_2m100=(0.03, 1), negative=(0.20, 1), zero=(0.10, 1), ordinary=(0.35, 1)),
    "B": dict(nan=(0.005, 0.10), inf=(0.02, 1), big=(0.02, 1), ordinary=(0.30, 1)),
    # the guard table: a tenth of the values are weights between 2^-130 and 2^-100 (non-zero, most of them normal), nothing overflows
    "G": dict(nan=(0, 0), inf=(0, 0), below_2m100=(0.10, 1), zero=(0, 0.30), ordinary=(0.35, 1)),
    "huge_env": dict(inf=(0.10, 1), denormal=(0.10, 1), nan=(0, 0.10)),
    "A_side": dict(nan=(0, 0), inf=(0, 0), denormal=(0.10, 1), zero=(0.10, 1), negative=(0.10, 1), ordinary=(0.10, 1)),
    "inf_env": dict(nan=(0.005, 0.36), inf=(0.25, 1), ordinary=(0.20, 1)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fixture_holds_the_values_it_is_there_for(pt, orc, case):
    """The oracle's film of every case a GPU test renders, at the GPU tests' size, holds the kinds of value its family is about in
    the shares of BANDS (conditions on the fixture, checked after every frame count a test compares at), and the oracle's
    brute-force mode gives the same film, image and ray count as its LBVH walk."""
    films, bgras, rayss, _ = _oracle(pt, orc, case)
    band = BANDS[CASES[case]["band"]]
    for k, film in enumerate(films):
        s = _shares(film)
        print(f"{case} after frame {k}: " + " ".join(f"{n}={100 * v:.2f}%" for n, v in s.items()))
        if k + 1 >= min(2, len(films)):
            for kind, (lo, hi) in band.items():
                assert lo <= s[kind] <= hi, (case, k, kind, s[kind], (lo, hi))
    bfilms, bbgras, brayss, _ = _oracle(pt, orc, case, mode=0)
    assert brayss == rayss
    for k in range(len(films)):
        _assert_same(case, f"brute force against the LBVH walk, frame {k}", bfilms[k], films[k])
        _assert_image(case, f"brute force against the LBVH walk, frame {k}", bbgras[k], bgras[k])


def _cos_for(brdf, target):
    """cosines in (0, 1] whose float32 product with brdf is exactly `target` (empty if no float does it)"""
    c0 = f32(min(abs(float(target)) / abs(float(brdf)), 2.0))
    cand = np.array([c0], f32)
    for _ in range(8):
        cand = np.unique(np.concatenate([cand, np.nextafter(cand, f32(0)), np.nextafter(cand, f32(2))]))
    cand = cand[(cand > 0) & (cand <= 1)]
    return cand[np.abs(f32(brdf) * cand) == f32(abs(float(target)))]


@pytest.mark.parametrize("spec,n", [(("A", 4), 36), (("A_all_emit", 4), 36), (("A", 5), 300), (("B", 15), 36), (("B", 30), 36), (("A", 12), 36), (("B", 38), 36), (("B", 44), 36), (("B", 5), 300)])
def test_tables_reach_every_side_of_the_division_guard(spec, n):
    """ptm::div3_by_pdf takes its three-instruction quotient only when all three channels of (Kd / pi) * cos lie in
    [2^-100, 2^120].  Over a table's Kd values and cos in (0, 1] the products have members strictly inside, exactly on and outside
    the lower bound (family B: and the upper bound), and some triangles have one channel outside while the other two are ordinary,
    which sends ordinary channels through the IEEE divide."""
    t = _table(spec, n)
    brdf = (t[:, :3] / f32(np.pi)).astype(f32)
    cosines = np.concatenate([f32([1.0, 0.5, 0.999, 1e-3]), np.random.default_rng(1).uniform(0, 1, 64).astype(f32)])
    with np.errstate(over="ignore", under="ignore"):
        prod = np.abs(brdf.reshape(-1, 1) * cosines.reshape(1, -1)).astype(f32)
    for bound, needed in ((GUARD_LO, True), (GUARD_HI, spec[0] == "B")):
        if not needed:
            assert not (prod > GUARD_HI).any()      # family A never leaves the guard upwards
            continue
        on = [c for b in np.unique(np.abs(brdf)) if b > 0 and np.isfinite(b) for c in _cos_for(b, bound)]
        near = (prod > bound / f32(64)) & (prod < bound * f32(64))
        assert (near & (prod < bound)).any() and (near & (prod > bound)).any() and len(on) > 0, (spec, float(bound), len(on))
    outside = (np.abs(brdf) < GUARD_LO) | (np.abs(brdf) > GUARD_HI)
    ordinary = (np.abs(brdf) > 0.05) & (np.abs(brdf) < 10)
    assert ((outside.sum(1) == 1) & (ordinary.sum(1) == 2)).any()
    assert not np.isnan(t).any()
    if spec[0] != "B":
        assert np.isfinite(t).all() and np.abs(t).max() <= 7.0


def test_comparison_rule_on_made_up_films():
    """_assert_same: family A notices a -0.0 for a +0 and a NaN of another sign; family B accepts the two generated NaN patterns for each
    other and nothing else, and the message names pixel, channel and bits."""
    a = np.zeros((2, 3, 3), f32)
    b = a.copy()
    b[1, 2, 0] = -0.0
    with pytest.raises(AssertionError, match=r"pixel \(2, 1\) channel 0: got 0x80000000, oracle 0x00000000"):
        _assert_same("cornell_a", "made up", b, a)
    with pytest.raises(AssertionError, match="0x80000000"):
        _assert_same("cornell_b", "made up", b, a)
    x86, gpu = a.copy(), a.copy()
    x86.view(u32)[0, 1, 2], gpu.view(u32)[0, 1, 2] = 0xFFC00000, 0x7FC00000
    _assert_same("cornell_b", "made up", gpu, x86)
    with pytest.raises(AssertionError, match=r"pixel \(1, 0\) channel 2"):
        _assert_same("cornell_a", "made up", gpu, x86)
    with pytest.raises(AssertionError, match="oracle 0x7fc00000"):
        _assert_same("cornell_b", "made up", a, x86)
    gpu[0, 0, 0] = INF
    with pytest.raises(AssertionError, match="got 0x7f800000"):
        _assert_same("cornell_b", "made up", gpu, x86)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
class _Scene:
    """a case's scene on the device, closed on exit"""

    def __init__(self, pt, ctx, case, tuning=None):
        v, i, faces, inst = _arrays(pt, case)
        old = ctx.set_tuning(**(tuning or {}))
        try:
            self.sc = pt.Scene(ctx, v, i, faces.reshape(-1))
        finally:
            ctx.set_tuning(**old)
        if inst is not None:
            self.sc.set_instances(inst)

    def __enter__(self):
        return self.sc

    def __exit__(self, *exc):
        self.sc.close()


def _render(pt, ctx, sc, case, calls=None, tuning=None, film=None, **params):
    """frames of a case into one film (calls: [(first frame, count)]; default: all of them in one call) under `tuning` -> (film f32,
    bgra8, stats over all calls)"""
    c = CASES[case]
    calls = calls or [(0, c["frames"])]
    flags = params.pop("flags", 0)
    if c["nee"] and params.get("pipeline") != pt.PIPELINE_WAVEFRONT_NEE:
        flags |= pt.FLAG_NEE
    own = film is None
    film = pt.Film(ctx, W, H) if own else film
    old = ctx.set_tuning(**(tuning or {}))
    try:
        ctx.reset_stats()
        for f0, n in calls:
            pt.render(sc, film, pt.default_params(frame=f0, frame_count=n, flags=flags, **_params_kw(case), **params))
        out = film.read_f32(), film.read_bgra8(), ctx.stats()
    finally:
        ctx.set_tuning(**old)
        if own:
            film.close()
    return out


def _check(pt, orc, ctx, sc, case, what, pipeline_ran=None, **kw):
    """one render of a case == the oracle's film (by the family's rule), rgba8 image and ray count -> stats"""
    ofilm, obgra, orays = _oracle_film(pt, orc, case)
    film, bgra, st = _render(pt, ctx, sc, case, **kw)
    what = f"{what} {sorted((k, v) for k, v in kw.items() if k != 'film')}"
    assert st.rays == orays, (case, what, st.rays, orays)
    _assert_same(case, what, film, ofilm)
    _assert_image(case, what, bgra, obgra)
    if pipeline_ran is not None:
        assert st.pipeline == pipeline_ran, (case, what, st.pipeline)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("extend", ["AUTO", "LDS"])
@pytest.mark.parametrize("case", ["cornell_a", "cornell_b"])
def test_wavefront_lds_tables(pt, orc, gpu_ctx, case, extend):
    """k_shade<.., LDS_TABLES = true> (36 triangles: 4.5 KB of tables, render.hip job_setup stages them in LDS): the emission skip and
    div3_by_pdf's two branches with one accumulator per slot, and add_radiance's term log replayed by k_resolve with three sample
    groups and with a group per sample; one and two frames in flight."""
    with _Scene(pt, gpu_ctx, case) as sc:
        for groups, fif in ((1, 1), (3, 1), (1, 2), (3, 2), (SPP, 1)):
            st = _check(pt, orc, gpu_ctx, sc, case, "wavefront, LDS tables", pipeline_ran=pt.PIPELINE_WAVEFRONT, pipeline=pt.PIPELINE_WAVEFRONT,
                        extend=getattr(pt, "EXTEND_" + extend), sample_groups=groups, frames_in_flight=fif)
            # (three groups asked of four samples: two samples per group, so two groups run)
            assert st.sample_groups == {1: 1, 3: 2, SPP: SPP}[groups] and st.extend_variant == pt.EXTEND_LDS


@pytest.mark.gpu
def test_division_guard_below_its_lower_bound(pt, orc, gpu_ctx):
    """ptm::div3_by_pdf's IEEE branch where it matters (table_g: dividends between 2^-130 and 2^-110, for which the short quotient is
    wrong by an ulp in up to a sixth of the cases): k_shade with LDS tables and with the HBM records of the 8-wide tree, one accumulator
    and the term log, k_fused plain and head + tail."""
    case = "cornell_guard"
    with _Scene(pt, gpu_ctx, case) as sc:
        for kw in (dict(pipeline=pt.PIPELINE_WAVEFRONT, sample_groups=1), dict(pipeline=pt.PIPELINE_WAVEFRONT, sample_groups=2),
                   dict(pipeline=pt.PIPELINE_WAVEFRONT, extend=pt.EXTEND_HBM8), dict(pipeline=pt.PIPELINE_FUSED, sample_groups=1),
                   dict(pipeline=pt.PIPELINE_FUSED, tuning=dict(fused_tail=3)), dict(pipeline=pt.PIPELINE_AUTO)):
            _check(pt, orc, gpu_ctx, sc, case, "guard table", **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case,extend", [("soup_a", "HBM"), ("soup_a", "HBM8"), ("soup_b", "HBM"), ("soup_b", "HBM8"), ("cornell_a", "HBM8"),
                                         ("cornell_b", "HBM8")])
def test_wavefront_hbm_tables(pt, orc, gpu_ctx, case, extend):
    """k_shade<.., LDS_TABLES = false>: the 64-byte records of k_pack with their `emits` flag (scene_build.hip), which replaces Ke by +0
    unless a channel is != 0.  pt_stats does not say which k_shade ran; the cases rely on the rule of render.hip job_setup,
    `shade_lds = 128 B * n_tris <= 16 KB && !bvh8`: the 300-triangle soup has 37.5 KB of tables under either closest-hit kernel, and
    the 8-wide tree (PT_EXTEND_HBM8) takes the HBM tables on the 36 triangles of the Cornell box too.  One accumulator and the term log."""
    with _Scene(pt, gpu_ctx, case) as sc:
        n_tris = sc.info().n_tris
        assert extend == "HBM8" or 128 * n_tris > 16 * 1024
        for groups in (1, 2):
            st = _check(pt, orc, gpu_ctx, sc, case, "wavefront, HBM tables", pipeline_ran=pt.PIPELINE_WAVEFRONT, pipeline=pt.PIPELINE_WAVEFRONT,
                        extend=getattr(pt, "EXTEND_" + extend), sample_groups=groups)
            assert st.sample_groups == groups and st.extend_variant == getattr(pt, "EXTEND_" + extend)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["soup_a", "soup_b"])
def test_soup_through_the_library_default(pt, orc, gpu_ctx, case):
    """The 300-triangle soup through PT_PIPELINE_AUTO and PT_EXTEND_AUTO, whatever they pick (printed): the same film."""
    with _Scene(pt, gpu_ctx, case) as sc:
        st = _check(pt, orc, gpu_ctx, sc, case, "library default", pipeline=pt.PIPELINE_AUTO)
        print(f"{case}: AUTO ran pipeline {pt.PIPELINE_NAMES[st.pipeline]}, extend variant {st.extend_variant}, {sc.info().n_tris} triangles")
        assert st.pipeline in (pt.PIPELINE_WAVEFRONT, pt.PIPELINE_FUSED)


FUSED_SHAPES = {"plain": (dict(fused_tail=0), dict(sample_groups=1)), "groups": (dict(fused_tail=0), dict(sample_groups=3)),
                "tail": (dict(fused_tail=3), dict()), "rule": (dict(fused_tail=-1), dict())}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(FUSED_SHAPES))
@pytest.mark.parametrize("case", ["cornell_a", "cornell_a_side", "cornell_b", "cornell_huge_env", "cornell_inf_env", "cornell_inf_env_side"])
def test_fused(pt, orc, gpu_ctx, case, shape):
    """k_fused (fused_kernel.h): its own copy of the emission skip, of div3_by_pdf's call and of the term log (sample groups; the head +
    tail slots of pt_tuning.fused_tail = 3 and of the library's rule), named and through PT_PIPELINE_AUTO, with the cull of pixels that
    cannot see the scene (fused_cull.h: a host-made sum of spp adds of 1 * env, or env terms in the log) and without it.  For the
    infinite env the cull must stand down (pt_stats.rays_culled == 0) and the film is the oracle's either way; the side view leaves
    two thirds of the image to the cull."""
    tuning, params = FUSED_SHAPES[shape]
    with _Scene(pt, gpu_ctx, case) as sc:
        for cull in (0, 1):
            for pipeline in (pt.PIPELINE_FUSED, pt.PIPELINE_AUTO):
                st = _check(pt, orc, gpu_ctx, sc, case, f"fused, {shape}", pipeline_ran=pt.PIPELINE_FUSED, pipeline=pipeline,
                            tuning=dict(tuning, cull=cull), **params)
                assert shape == "rule" or st.tail_samples == (3 if shape == "tail" else 0), (case, shape, st.tail_samples)
                culls = cull == 1 and np.isfinite(CASES[case]["env"]).all()
                assert (st.rays_culled > 0) == culls and st.rays_culled % (SPP * CASES[case]["frames"]) == 0, (case, shape, cull, st.rays_culled)


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["WAVEFRONT", "FUSED"])
@pytest.mark.parametrize("case", ["cornell_a_side", "cornell_b", "cornell_inf_env_side"])
def test_every_rank_of_three_assembles_the_film(pt, orc, gpu_ctx, case, pipeline):
    """rank / world: each rank of three renders its tiles (k_fused / the queues with a tile subset); a rank's film is all-zero bits
    outside its pixels and the oracle's inside.  The pixels are put together by ownership, not by a float sum: +0 + -0.0 would lose the
    sign of a -0.0 and inf + 0 is fine but NaN + 0 hides which NaN it was."""
    d = importlib.import_module("single-file-vulkan-pathtracing_amd.distributed")
    ofilm, obgra, orays = _oracle_film(pt, orc, case)
    total, rays, seen = np.zeros((H, W, 3), f32), 0, np.zeros((H, W), bool)
    with _Scene(pt, gpu_ctx, case) as sc:
        for rank in range(3):
            film, _, st = _render(pt, gpu_ctx, sc, case, pipeline=getattr(pt, "PIPELINE_" + pipeline), rank=rank, world=3)
            mine = d.owned_mask(W, H, rank, 3)
            assert not (film.view(u32)[~mine] != 0).any() and not (seen & mine).any(), (case, rank)
            total[mine] = film[mine]
            seen |= mine
            rays += st.rays
    assert seen.all() and rays == orays, (case, rays, orays)
    _assert_same(case, f"{pipeline}, three ranks", total, ofilm)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["inst_a", "inst_b"])
def test_instanced(pt, orc, gpu_ctx, case):
    """k_shade<.., INST = true> with the (instance, triangle) frame table and with the per-hit transform (pt_tuning.inst_frames = 0), and
    k_fused_inst (fused_inst_kernel.h) with one accumulator and with the term log: five rotated and scaled Cornell boxes."""
    with _Scene(pt, gpu_ctx, case) as sc:
        assert sc.info().n_instances == 5
        for frames_knob in (0, 1):
            _check(pt, orc, gpu_ctx, sc, case, "wavefront, instanced", pipeline_ran=pt.PIPELINE_WAVEFRONT, pipeline=pt.PIPELINE_WAVEFRONT,
                   tuning=dict(inst_frames=frames_knob))
        _check(pt, orc, gpu_ctx, sc, case, "wavefront, instanced, term log", pipeline=pt.PIPELINE_WAVEFRONT, sample_groups=2)
        for groups in (1, 2, SPP):
            st = _check(pt, orc, gpu_ctx, sc, case, "fused, instanced", pipeline_ran=pt.PIPELINE_FUSED, pipeline=pt.PIPELINE_FUSED, sample_groups=groups)
            assert st.sample_groups == groups


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cornell_nee_a", "cornell_nee_b", "soup_nee_a", "soup_nee_b", "inst_nee_a", "inst_nee_b"])
def test_nee(pt, orc, gpu_ctx, case):
    """Next-event estimation against the oracle's nee mode: ptn::nee_sample in k_shade<.., NEE = true> (LDS tables, HBM tables, instanced)
    and k_shadow_add, and k_fused_nee on the Cornell box.  The emitter list takes every triangle with a Ke channel != 0
    (pt_oracle.c build_lights), so negative and denormal emitters are sampled and a triangle whose Ke is all -0.0 is not."""
    faces = _arrays(pt, case)[2]
    ke = faces[:, 3:]
    lights = (ke != 0).any(1)
    assert lights.any() and ((ke < 0).any(1) & lights).any() and ((np.abs(ke) < 2.0 ** -126) & (ke != 0)).any()
    assert (~lights & np.signbit(ke).any(1)).any(), case       # Ke all zeros with a -0.0 among them: no light
    with _Scene(pt, gpu_ctx, case) as sc:
        for fif in (1, 2):     # (the NEE pipeline runs one sample group per pixel: no term log)
            _check(pt, orc, gpu_ctx, sc, case, "wavefront NEE", pipeline_ran=pt.PIPELINE_WAVEFRONT_NEE, pipeline=pt.PIPELINE_WAVEFRONT_NEE,
                   frames_in_flight=fif)
        if CASES[case]["geom"] == "cornell":
            for tuning in (dict(cull=0), dict(cull=1)):
                _check(pt, orc, gpu_ctx, sc, case, "fused NEE", pipeline_ran=pt.PIPELINE_FUSED, pipeline=pt.PIPELINE_FUSED, tuning=tuning)
        else:
            _check(pt, orc, gpu_ctx, sc, case, "NEE by flag", pipeline=pt.PIPELINE_AUTO)


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if CASES[c]["nee"]])
def test_every_nee_table_has_an_emitter_of_each_awkward_kind(pt, case):
    """The NEE cases' claims, per case and without a GPU: its table has lights with a negative and with a denormal Ke channel, and a
    triangle whose Ke channels are all zeros with a -0.0 among them, which build_lights (pt_oracle.c) and the device's list leave out."""
    ke = _arrays(pt, case)[2][:, 3:]
    lights = (ke != 0).any(1)
    assert ((ke < 0).any(1) & lights).any() and ((np.abs(ke) < 2.0 ** -126) & (ke != 0)).any(), case
    assert (~lights & np.signbit(ke).any(1)).any(), case


@pytest.mark.gpu
@pytest.mark.parametrize("ocap,pool", [(0, 0), (3, 64), (0, None), (2, None)])
def test_all_emit_table_through_the_term_log_overflow_paths(pt, orc, gpu_ctx, ocap, pool):
    """Every triangle emits (family A: zero, -0.0, denormal, negative and ordinary Ke channels), so every hit logs a term unless all three
    are zero: past the primary log into the overflow log and the spill pool (add_radiance in wavefront_types.h, its restatement in
    fused_kernel.h, k_resolve's replay), and with a pool too small the batch is rendered again with one group -- the tuning values of
    test_full_term_log_spills_to_the_pool_or_the_batch_is_redone_exactly, on the queues and on k_fused."""
    case = "cornell_all_emit"
    tuning = dict(term_ocap=ocap, term_spill=-1 if pool is None else pool)
    with _Scene(pt, gpu_ctx, case) as sc:
        for what, kw in (("wavefront, 2 groups", dict(pipeline=pt.PIPELINE_WAVEFRONT, sample_groups=2)),
                         ("wavefront, 4 groups, 2 frames in flight", dict(pipeline=pt.PIPELINE_WAVEFRONT, sample_groups=4, frames_in_flight=2)),
                         ("fused, 2 groups", dict(pipeline=pt.PIPELINE_FUSED, sample_groups=2)),
                         ("fused, head + tail", dict(pipeline=pt.PIPELINE_FUSED, tuning=dict(fused_tail=3)))):
            kw["tuning"] = dict(kw.get("tuning", {}), **tuning)
            st = _check(pt, orc, gpu_ctx, sc, case, what, **kw)
            print(f"{what} ocap={ocap} pool={pool}: redone_batches={st.redone_batches}")
            # the default pool absorbs every term; without a pool and without an overflow log a slot of two samples (up to 12 terms) cannot
            # stay within the primary log (group_size + 2 = four entries: film_work.hip), so the batch is done again
            assert pool is not None or st.redone_batches == 0, (what, st.redone_batches)
            assert pool != 0 or "2 groups" not in what or st.redone_batches >= 1, (what, st.redone_batches)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cornell_a_3f", "cornell_b_3f"])
def test_resolve_after_every_frame_and_the_second_moment_plane(pt, orc, gpu_ctx, any_pipeline, case):
    """k_resolve / k_resolve_m2: the blend into the film, to_unorm8 (NaN and negatives give 0, values above 1 are clamped) and the squared
    frame colour.  Three frames batched and frame by frame equal the oracle after every frame, film and rgba8; with enable_moments()
    the second-moment plane equals _moments_ref of tests/test_denoise_variance.py fed the oracle's frame colours (family B: squares
    overflow, same NaN rule)."""
    films, bgras, rayss, colours = _oracle(pt, orc, case)
    with np.errstate(all="ignore"):
        m2_want = [_moments_ref(colours[:k + 1]) for k in range(3)]
    with _Scene(pt, gpu_ctx, case) as sc:
        film = pt.Film(gpu_ctx, W, H)
        film.enable_moments()
        try:
            for k in range(3):           # frame by frame on one film
                got, bgra, st = _render(pt, gpu_ctx, sc, case, calls=[(k, 1)], film=film, pipeline=any_pipeline)
                _assert_same(case, f"frame by frame, after frame {k}", got, films[k])
                _assert_image(case, f"frame by frame, after frame {k}", bgra, bgras[k])
                m2, n = film.read_moments()
                assert n == k + 1
                _assert_same(case, f"film restated by _moments_ref, after frame {k}", m2_want[k][0], films[k])
                _assert_same(case, f"second moments, after frame {k}", m2, m2_want[k][1])
            for first in (1, 2, 3):      # batched: frames 0 .. first-1 in one call, the rest in another
                film.clear()
                calls = [(0, first)] + ([(first, 3 - first)] if first < 3 else [])
                got, bgra, st = _render(pt, gpu_ctx, sc, case, calls=calls, film=film, pipeline=any_pipeline, frames_in_flight=2)
                assert st.rays == rayss[2]
                _assert_same(case, f"batched {calls}", got, films[2])
                _assert_image(case, f"batched {calls}", bgra, bgras[2])
                m2, n = film.read_moments()
                assert n == 3
                _assert_same(case, f"second moments, batched {calls}", m2, m2_want[2][1])
        finally:
            film.close()
    # what the planes are tested on: out-of-range values for to_unorm8, and (family B) squares that overflow
    assert (films[2] > 1).any() and (films[2] < 0).any()
    if not _exact(case):
        assert np.isnan(films[2]).any() and np.isinf(m2_want[2][1]).any() and np.isinf(films[2]).any()


AOV_TABLE = ("A", 4)


@pytest.mark.parametrize("aov_case", ["cornell", "one_inst"])
def test_guide_plane_fixtures_hold_awkward_averages(pt, orc, aov_case):
    """The expected guide planes of test_guide_planes_keep_awkward_table_values, by the oracle's bindings alone: the albedo and emission
    planes hold denormal, negative and ordinary averages.  No -0.0 can: the definition (test_aov._guides) sums a pixel's samples from
    +0, and +0 + -0.0 = +0, so a -0.0 table entry shows as +0 on both sides."""
    want = test_aov._guides(pt, orc, aov_case, [0, 1], faces=_table(AOV_TABLE, 36))
    for name in ("albedo", "emission"):
        a = np.abs(want[name])
        assert ((a > 0) & (a < 2.0 ** -126)).any() and (want[name] < 0).any() and (a > 0.1).any(), name
        assert not (np.signbit(want[name]) & (want[name] == 0)).any(), name


@pytest.mark.gpu
@pytest.mark.parametrize("aov_case", ["cornell", "one_inst"])
def test_guide_planes_keep_awkward_table_values(pt, orc, gpu_ctx, aov_case):
    """aov.hip: the albedo and emission planes average the table's Kd and Ke of the first hits.  With a family A table on the Cornell
    box and on the one-instance box, through the helpers of tests/test_aov.py (`_guides` with the table in place of the materials),
    every plane is bit-exact on the queues and (single level) on the fused kernel; what the expected planes hold is checked by
    test_guide_plane_fixtures_hold_awkward_averages."""
    faces = _table(AOV_TABLE, 36)
    want = test_aov._guides(pt, orc, aov_case, [0, 1], faces=faces)
    v, i, _, inst = test_aov._arrays(pt, test_aov.CASES[aov_case][0])
    sc = pt.Scene(gpu_ctx, v, i, faces.reshape(-1))
    try:
        if inst is not None:
            sc.set_instances(inst)
        for pipeline in (pt.PIPELINE_WAVEFRONT, pt.PIPELINE_AUTO):
            got, st = test_aov._run(pt, gpu_ctx, sc, aov_case, [(0, 2)], pipeline=pipeline)
            assert st.pipeline == (pt.PIPELINE_FUSED if pipeline == pt.PIPELINE_AUTO and inst is None else pt.PIPELINE_WAVEFRONT)
            test_aov._same(got, want, f"{aov_case}, family A table, pipeline {pipeline}")
    finally:
        sc.close()
