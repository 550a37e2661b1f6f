"""k_fused: a bounce ray leaves out the leaf of the triangle it starts on when csrc/self_leaf.h's rule says the oracle's arithmetic cannot accept
a triangle of that leaf inside (tmin, tmax): dir . n >= max(thr[p], c1(tmin) * g[p]).

CPU: the rule itself -- the functions the scene packer and the kernel evaluate, through libpt_host.so -- against the oracle's own triangle test, on
more than 10^6 rays that the rule lets skip: none of them may hit its own leaf.
GPU: films, ray counts and the twin's SKIP count of PT_PIPELINE_FUSED against the oracle and against PT_PIPELINE_WAVEFRONT (which never skips), on
the scenes where the rule has its edges: a valley fold whose halves see each other, a ridge and a planar quad in a fat box, a fan that is no convex
quad, tmin from far below the bound to beyond the scene, coincident quads, the three fused forms with and without the cull, pt_render_guided, and a
pt_scene_update that folds a planar quad.
"""
import numpy as np
import pytest

W, H = 64, 64
F32 = np.float32
FORMS = {"one_group": (dict(fused_tail=0), dict(sample_groups=1)),
         "groups": (dict(fused_tail=0), dict(sample_groups=4)),
         "head_tail": (dict(fused_tail=3), dict())}
CAM = dict(cam_origin=(0.3, 0.2, -3.0), cam_target=(0.0, 0.0, 0.0))   # the quads below bounce towards -z (their stored normal)


# ---- scenes: one quad (v0, v1, v2) + (v0, v2, v3) around the origin, z = f(x, y) ------------------------------------------------------
def _faces(n):
    f = np.zeros((n, 6), F32)
    f[:, 0:3] = (0.7, 0.6, 0.5)
    f[:, 3:6] = (0.5, 0.25, 0.125)     # every triangle emits: every hit shows in the film
    return f.reshape(-1)


def quad(dz1=0.0, dz3=0.0, tilt=True, v3=None):
    """the fan's apexes v1, v3 lifted by dz towards -z (the side the bounces leave on: a valley) or +z (a ridge); tilt: z += x / 2 + y / 4, exact in
    binary32 for these coordinates, so the quad's box is fat and a planar quad stays exactly planar"""
    v = np.array([[-0.75, -0.5, 0.0], [0.75, -0.5, -dz1], [0.75, 0.5, 0.0], [-0.75, 0.5, -dz3]], np.float64)
    if v3 is not None:
        v[3] = v3
    if tilt:
        v[:, 2] += 0.5 * v[:, 0] + 0.25 * v[:, 1]
    return v.astype(F32).reshape(-1), np.uint32([0, 1, 2, 0, 2, 3]), _faces(2)


VALLEY = quad(0.0625, 0.0625)
RIDGE = quad(-0.0078125, -0.0078125)
PLANAR = quad()
DART = quad(v3=[0.5, -0.25, 0.0])      # v3 on v1's side of the diagonal: the apex does not project across the shared edge


def two_coincident():
    v, i, f = quad()
    f = _faces(4).reshape(4, 6)
    f[2:, 3:6] = (0.125, 0.5, 0.25)     # the second copy emits another colour: which copy a ray hits shows in the film
    return np.concatenate([v, v]), np.concatenate([i, i + 4]).astype(np.uint32), f.reshape(-1)


def rule_limits(pt, arrays, tmin=1e-3):
    """the rule's dt limit of the two halves of a one-quad scene, as scene_build.hip and the kernel form it"""
    v = arrays[0].reshape(-1, 3)
    e = float(np.abs(v).max())
    c1 = pt.self_leaf_c1(tmin)
    out = []
    for own, other in ((1, 3), (3, 1)):
        thr, g = pt.self_leaf_rule(v[0], v[2], v[own], v[other], e)
        out.append(max(thr, F32(c1) * np.uint32(g).view(F32)) if np.isfinite(thr) else np.inf)
    return out


# ---- the oracle's answer, once per (scene, parameters); read-only -----------------------------------------------------------------------
_want = {}


def oracle(orc, name, arrays, frames, **kw):
    key = (name, frames, tuple(sorted(kw.items())))
    if key not in _want:
        osc = orc.Scene(*arrays)
        film, rays = np.zeros((H, W, 3), F32), 0
        for k in range(frames):
            img, r, _, _ = osc.render_frame(orc.default_params(frame=k, width=W, height=H, **kw))
            orc.accumulate_f32(film, img, k)
            rays += r
        film.setflags(write=False)
        _want[key] = (film, rays)
    return _want[key]


def render(pt, ctx, sc, frames, pipeline, form="one_group", flags=0, tuning=None, **kw):
    tune, params = FORMS[form]
    film = pt.Film(ctx, W, H)
    old = ctx.set_tuning(**dict(tune, **(tuning or {})))
    try:
        ctx.reset_stats()
        pt.render(sc, film, pt.default_params(frame=0, frame_count=frames, width=W, height=H, pipeline=pipeline, flags=flags, **params, **kw))
        st = ctx.stats()
        return film.read_f32(), film.read_bgra8(), st, (ctx.block_counts() if flags & pt.FLAG_COUNT_VISITS else None)
    finally:
        ctx.set_tuning(**old)
        film.close()


def check(pt, orc, ctx, name, arrays, frames=2, form="one_group", tuning=None, sc=None, **kw):
    """fused == oracle == wavefront (film bytes, rgba8 bytes, rays), the twin likewise -> (lanes that skipped, bounce rays) of the twin"""
    kw = dict(dict(spp_per_frame=4, max_depth=6, **CAM), **kw)
    want, rays = oracle(orc, name, arrays, frames, **kw)
    own = sc is None
    sc = sc or pt.Scene(ctx, *arrays)
    try:
        got, bgra, st, _ = render(pt, ctx, sc, frames, pt.PIPELINE_FUSED, form, tuning=tuning, **kw)
        assert st.pipeline == pt.PIPELINE_FUSED, (name, st.pipeline)
        assert st.rays == rays, (name, form, st.rays, rays)
        assert got.tobytes() == want.tobytes(), (name, form, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        ref, rbgra, rst, _ = render(pt, ctx, sc, frames, pt.PIPELINE_WAVEFRONT, "one_group", **kw)
        assert rst.rays == st.rays and ref.tobytes() == got.tobytes() and rbgra.tobytes() == bgra.tobytes(), (name, form)
        twin, _, tst, bc = render(pt, ctx, sc, frames, pt.PIPELINE_FUSED, form, flags=pt.FLAG_COUNT_VISITS, tuning=tuning, **kw)
        assert tst.rays == rays and twin.tobytes() == want.tobytes(), (name, form, "twin")
        return bc["SKIP"][1], bc["BOUNCE"][1]
    finally:
        if own:
            sc.close()


# ---- CPU: the rule against the oracle's triangle test -----------------------------------------------------------------------------------
def _tri_normal(a, b, c):
    """ptm::tri_normal in binary32, operation for operation"""
    e, f = (b - a).astype(F32), (c - a).astype(F32)
    cx = F32(e[1] * f[2]) - F32(e[2] * f[1]); cy = F32(e[2] * f[0]) - F32(e[0] * f[2]); cz = F32(e[0] * f[1]) - F32(e[1] * f[0])
    ln = np.sqrt(F32(F32(F32(cx * cx) + F32(cy * cy)) + F32(cz * cz)), dtype=F32)
    return np.array([-(cx / ln), -(cy / ln), -(cz / ln)], F32)


def _leaf(rng, k):
    """a random leaf: (vertices [3 or 4, 3] f32, pair?) -- scales over twelve orders of magnitude, offsets up to 64 x the size, slivers, folds"""
    scale = 10.0 ** rng.uniform(-6, 6)
    off = rng.uniform(-1, 1, 3) * scale * (0.0 if k % 3 == 0 else 10.0 ** rng.uniform(-1, 1.8))
    q = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float64) * rng.uniform(0.05 if k % 5 == 0 else 0.4, 1.0, (1, 3)) + rng.uniform(-0.2, 0.2, (4, 3)) * [1, 1, 0]
    q[1, 2] += rng.choice([0.0, 0.0, 1.0, -1.0]) * 10.0 ** rng.uniform(-7, -0.6)   # planar, valley or ridge, from a rounding error to a steep fold
    q[3, 2] += rng.choice([0.0, 0.0, 1.0, -1.0]) * 10.0 ** rng.uniform(-7, -0.6)
    rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    v = (q @ rot.T * scale + off).astype(F32)
    pair = k % 4 != 0
    return (v if pair else v[:3]), pair


def test_rays_the_rule_lets_skip_never_hit_their_own_leaf_in_the_oracle(pt, orc):
    """>= 10^6 rays from random leaves (fan pairs and single triangles; tiny and huge coordinates; slivers; folds of every size): origins by the
    kernel's barycentric formula (corners and edges included), directions whose dt lies within a few ulp above the rule's limit and random ones
    above it, tmin from 1e-6 x to 1e-1 x the leaf's size.  The oracle's own triangle test of the leaf alone accepts none of them."""
    rng = np.random.default_rng(20240611)
    total = skipping_leaves = never = 0
    k = 0
    while total < 1_050_000:
        v, pair = _leaf(rng, k)
        k += 1
        e = float(np.abs(v).max())
        size = float(np.linalg.norm(v.max(0) - v.min(0)))
        tmin = F32(size * 10.0 ** rng.uniform(-6, -1))
        c1 = pt.self_leaf_c1(tmin)
        idx = np.uint32([0, 1, 2, 0, 2, 3] if pair else [0, 1, 2])
        osc = None
        for own, other, tri in (((1, 3, (0, 1, 2)), (3, 1, (0, 2, 3))) if pair else ((1, None, (0, 1, 2)),)):
            thr, g = pt.self_leaf_rule(v[0], v[2], v[own], None if other is None else v[other], e)
            g_word = g | 0x2155
            lim = max(thr, F32(c1 * np.uint32(g_word).view(F32))) if np.isfinite(thr) else np.inf
            if not lim <= 1.0:
                never += 1
                continue
            a, b, c = v[tri[0]], v[tri[1]], v[tri[2]]
            n = _tri_normal(a, b, c)
            m = 600
            hu = rng.uniform(0, 1, m).astype(F32); hv = (rng.uniform(0, 1, m) * (1 - hu)).astype(F32)
            hu[:40:4] = 0; hv[1:40:4] = 0; hv[2:40:4] = (F32(1) - hu[2:40:4]).astype(F32); hu[3:40:8] = 1; hv[3:40:8] = 0   # edges and corners
            b0 = ((F32(1) - hu).astype(F32) - hv).astype(F32)
            org = ((a[None] * b0[:, None]).astype(F32) + (b[None] * hu[:, None]).astype(F32)).astype(F32)
            org = (org + (c[None] * hv[:, None]).astype(F32)).astype(F32)
            # directions: cos(theta) just above the limit (a few ulp steps) for half of them, anywhere above it for the rest
            cos = np.where(np.arange(m) % 2 == 0, np.float64(lim) * (1 + rng.integers(0, 12, m) * 2.0 ** -23), rng.uniform(lim, 1.0, m)).clip(0, 1)
            t = np.cross(n.astype(np.float64), [1.0, 0, 0] if abs(n[0]) < 0.7 else [0, 1.0, 0]); t /= np.linalg.norm(t)
            bt = np.cross(n.astype(np.float64), t)
            phi = rng.uniform(0, 2 * np.pi, m)
            d = (cos[:, None] * n[None] + np.sqrt(1 - cos ** 2)[:, None] * (np.cos(phi)[:, None] * t[None] + np.sin(phi)[:, None] * bt[None])).astype(F32)
            dt = (((d[:, 0] * n[0]).astype(F32) + (d[:, 1] * n[1]).astype(F32)).astype(F32) + (d[:, 2] * n[2]).astype(F32)).astype(F32)
            skip = pt.self_leaf_skip(dt, thr, g_word, c1) != 0
            assert ((dt >= lim) == skip).all()
            if not skip.any():
                continue
            osc = osc or orc.Scene(v.reshape(-1), idx, _faces(len(idx) // 3))
            hits, _ = osc.trace(np.concatenate([org[skip], d[skip]], axis=1), tmin=float(tmin), tmax=1e30)
            bad = hits["prim"] != 0xFFFFFFFF
            assert not bad.any(), (k, own, int(bad.sum()), float(thr), float(lim), hits[bad][:3], v.tolist())
            total += int(skip.sum())
            skipping_leaves += 1
    assert total >= 1_000_000 and skipping_leaves > 500 and never > 50, (total, skipping_leaves, never)


def test_the_rule_says_never_where_its_bound_does_not_hold(pt):
    """degenerate and non-finite triangles, an apex that does not cross the shared edge, a steep fold, a sliver: thr = +inf; no finite tmin below
    the bound lets a ray skip; a single triangle and a planar pair do"""
    v = PLANAR[0].reshape(-1, 3)
    assert np.isfinite(pt.self_leaf_rule(v[0], v[2], v[1], v[3], 1.0)[0]) and np.isfinite(pt.self_leaf_rule(v[0], v[2], v[1], None, 1.0)[0])
    d = DART[0].reshape(-1, 3)
    assert np.isinf(pt.self_leaf_rule(d[0], d[2], d[1], d[3], 1.0)[0]) and np.isinf(pt.self_leaf_rule(d[0], d[2], d[3], d[1], 1.0)[0])
    assert np.isinf(pt.self_leaf_rule(v[0], v[0], v[1], None, 1.0)[0])                                  # degenerate
    assert np.isinf(pt.self_leaf_rule(v[0], v[2], [np.nan, 0, 0], None, 1.0)[0])                         # not finite
    assert np.isinf(pt.self_leaf_rule(v[0], v[2], v[1], v[3] + F32([0, 0, 1.0]), 1.0)[0])                # a steep fold
    assert np.isinf(pt.self_leaf_rule([0, 0, 0], [1, 0, 0], [0.5, 1e-7, 0], None, 1.0)[0])               # a sliver
    assert np.isinf(pt.self_leaf_c1(0.0)) and np.isinf(pt.self_leaf_c1(-1.0)) and np.isinf(pt.self_leaf_c1(np.inf)) and np.isinf(pt.self_leaf_c1(np.nan))
    thr, g = pt.self_leaf_rule(v[0], v[2], v[1], v[3], 1.0)
    assert (pt.self_leaf_skip(F32([0.0, 0.5, 1.0]), thr, g | 0x2001, pt.self_leaf_c1(1e-9)) == 0).all()
    assert (pt.self_leaf_skip(F32([0.01, 0.5, 1.0, np.nan]), thr, g | 0x2001, pt.self_leaf_c1(1e-3)) == [0, 0x2001, 0x2001, 0]).all()


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_valley_fold_whose_halves_see_each_other(pt, orc, gpu_ctx):
    """(i) grazing bounce rays from one half legitimately hit the other: the oracle alone shows them (the scene is the quad alone, so a path's
    second hit is on the other half: rays(depth 3) - rays(depth 2) of them); the steeper rays skip, the flat ones do not"""
    kw = dict(spp_per_frame=8, **CAM)
    _, r2 = oracle(orc, "valley", VALLEY, 1, max_depth=2, **kw)
    _, r3 = oracle(orc, "valley", VALLEY, 1, max_depth=3, **kw)
    assert r3 - r2 >= 100, (r2, r3)
    lim = rule_limits(pt, VALLEY)
    assert all(0.3 < x < 1.0 for x in lim), lim
    skipped, bounces = check(pt, orc, gpu_ctx, "valley", VALLEY, spp_per_frame=8, max_depth=6)
    assert 0 < skipped < bounces, (skipped, bounces)
    assert abs(skipped - (1.0 - 0.5 * (lim[0] + lim[1])) * bounces) < 0.1 * bounces, (skipped, bounces, lim)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ridge", "planar"])
def test_ridge_and_planar_quad_in_a_fat_box_nearly_every_bounce_skips(pt, orc, gpu_ctx, name):
    """(ii) every bounce ray steeper than the rule's limit leaves its leaf out -- cos(theta) is uniform, so that is 1 - limit of them"""
    arrays = RIDGE if name == "ridge" else PLANAR
    lim = rule_limits(pt, arrays)
    assert all(x < 0.3 for x in lim), lim
    skipped, bounces = check(pt, orc, gpu_ctx, name, arrays, spp_per_frame=8, max_depth=8)
    assert bounces > 10000 and skipped > 0.7 * bounces, (skipped, bounces)
    assert abs(skipped - (1.0 - 0.5 * (lim[0] + lim[1])) * bounces) < 0.03 * bounces, (skipped, bounces, lim)


@pytest.mark.gpu
def test_fan_whose_apex_does_not_cross_the_shared_edge_never_skips(pt, orc, gpu_ctx):
    """(iii)"""
    assert all(np.isinf(x) for x in rule_limits(pt, DART))
    skipped, bounces = check(pt, orc, gpu_ctx, "dart", DART)
    assert skipped == 0 and bounces > 1000, (skipped, bounces)


@pytest.mark.gpu
def test_tmin_from_below_the_bound_to_beyond_the_scene(pt, orc, gpu_ctx):
    """(iv) the same scene at every tmin: the oracle's film each time; nothing skips far below the bound or where no ray can hit"""
    sc = pt.Scene(gpu_ctx, *PLANAR)
    try:
        counts = {}
        for tmin in (1e-9, 1e-6, 1e-4, 1e-3, 1e-1, 30.0):
            counts[tmin] = check(pt, orc, gpu_ctx, "planar", PLANAR, sc=sc, tmin=tmin)
        assert counts[1e-9][0] == 0 and counts[1e-9][1] > 1000 and counts[30.0] == (0, 0), counts
        assert counts[1e-6][0] == 0 and 0 < counts[1e-3][0] <= counts[1e-1][0] < counts[1e-1][1], counts
    finally:
        sc.close()


@pytest.mark.gpu
def test_coincident_quads_in_different_leaves(pt, orc, gpu_ctx):
    """(v) a ray that starts on one copy skips that copy's leaf only: the other copy is found (lowest primitive id wins the tie) as before"""
    skipped, bounces = check(pt, orc, gpu_ctx, "coincident", two_coincident(), max_depth=8)
    assert skipped > 0.5 * bounces, (skipped, bounces)


@pytest.mark.gpu
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("form", list(FORMS))
def test_three_forms_with_and_without_the_cull_on_the_cornell_box(pt, orc, gpu_ctx, cornell_gpu, cornell_arrays, form, cull):
    """(vi) one group and head + tail skip, several groups keep the old walk: the same film, rgba8 image and ray count from all of them"""
    skipped, bounces = check(pt, orc, gpu_ctx, "cornell", cornell_arrays, form=form, tuning=dict(cull=cull), sc=cornell_gpu, max_depth=8,
                             cam_origin=(0.0, 1.0, 3.0), cam_target=(0.0, 1.0, 0.0))
    assert (skipped == 0) if form == "groups" else (0 < skipped < bounces), (form, skipped, bounces)


@pytest.mark.gpu
def test_render_guided_on_a_folded_quad(pt, orc, gpu_ctx):
    """(vi) pt_render_guided's single pass (the kernels with the first-hit log) skips too: film and guide planes as the two calls leave them"""
    kw = dict(frame=0, frame_count=2, width=W, height=H, spp_per_frame=4, max_depth=6, pipeline=pt.PIPELINE_FUSED, **CAM)
    want, rays = oracle(orc, "valley", VALLEY, 2, spp_per_frame=4, max_depth=6, **CAM)
    sc = pt.Scene(gpu_ctx, *VALLEY)
    films = [pt.Film(gpu_ctx, W, H) for _ in range(2)]
    try:
        planes = []
        for film, mode in zip(films, (pt.GUIDED_SINGLE_PASS, pt.GUIDED_TWO_CALLS)):
            film.enable_aov()
            gpu_ctx.reset_stats()
            pt.render_guided(sc, film, pt.default_params(**kw), mode=mode)
            assert film.read_f32().tobytes() == want.tobytes(), mode
            planes.append([film.read_aov(a).tobytes() for a in (pt.AOV_ID, pt.AOV_DEPTH, pt.AOV_NORMAL)])
        assert planes[0] == planes[1]
    finally:
        for f in films:
            f.close()
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_scene_update_that_folds_a_planar_quad(pt, orc, gpu_ctx, mode):
    """(vii) the rule is recomputed where the tables are packed again: after the update the film is a fresh scene's (the planar quad's limit
    would let rays skip that now hit the other half)"""
    assert max(rule_limits(pt, PLANAR)) < min(rule_limits(pt, VALLEY))
    sc = pt.Scene(gpu_ctx, *PLANAR)
    try:
        check(pt, orc, gpu_ctx, "planar", PLANAR, sc=sc, spp_per_frame=8)
        sc.update(VALLEY[0], VALLEY[1], pt.SCENE_UPDATE_REFIT if mode == "refit" else pt.SCENE_UPDATE_REBUILD)
        skipped, bounces = check(pt, orc, gpu_ctx, "valley", VALLEY, sc=sc, spp_per_frame=8)
        assert 0 < skipped < bounces
    finally:
        sc.close()
