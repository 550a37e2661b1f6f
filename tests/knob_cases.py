"""What tests/test_ploc_trees.py, tests/test_tlas_ploc.py and tests/test_tuning_knobs.py share: pt_tuning set for the length of a block and
put back, the ray recipe, and the oracle's answers (computed once per session per key, never changed) with the comparisons against them."""
import contextlib

import numpy as np

f32 = np.float32
MISS = 0xFFFFFFFF
TMINS = (0.001, -0.25)
FILM = dict(width=96, height=64, spp_per_frame=4, max_depth=6)
FRAMES = 2
_cache = {}


@contextlib.contextmanager
def tuning(ctx, knobs):
    """pt_tuning knobs (a dict of TUNING_NAMES) on a shared context for the length of the block.  Set before pt.Scene(...): a build reads them."""
    old = ctx.set_tuning(**knobs)
    try:
        yield
    finally:
        ctx.set_tuning(**old)


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def make_rays(v, n=20000, seed=31, n_axis=300):
    """n rays for a scene with vertices v: camera rays from the default eye (0, -1, 5) at points of the scene's box, incoherent rays from
    inside the box, and n_axis axis-parallel rays (two zero direction components) from inside it"""
    p = np.asarray(v, np.float64).reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    ext = np.maximum(hi - lo, 0.05)
    rng = np.random.default_rng(seed)
    n_cam = (n - n_axis) // 2
    n_inc = n - n_axis - n_cam
    tgt = rng.uniform(lo - 0.05 * ext, hi + 0.05 * ext, (n_cam, 3))
    eye = np.tile(np.float64([0.0, -1.0, 5.0]), (n_cam, 1))
    cam = np.concatenate([eye, tgt - eye], 1)
    inc = np.concatenate([rng.uniform(lo - 0.1 * ext, lo + 1.1 * ext, (n_inc, 3)), rng.normal(size=(n_inc, 3))], 1)
    axis = np.concatenate([rng.uniform(lo - 0.1 * ext, lo + 1.1 * ext, (n_axis, 3)),
                           np.eye(3)[rng.integers(0, 3, n_axis)] * rng.choice([-1.0, 1.0], (n_axis, 1))], 1)
    r = np.concatenate([cam, inc, axis])
    r[:, 3:] /= np.linalg.norm(r[:, 3:], axis=1, keepdims=True)
    return np.ascontiguousarray(r, f32)


def oracle_traces(orc, key, v, i, f, instances=None, mode=0, rays=None, hit_range=(0.1, 0.98)):
    """-> (rays, {tmin: the oracle's hit records}) for a scene, once per key.  mode 0 = the oracle's brute force over every triangle."""
    def make():
        osc = orc.Scene(v, i, f)
        if instances is not None:
            osc.set_instances(instances)
        r = make_rays(v) if rays is None else rays
        want = {tmin: osc.trace(r, tmin=tmin, tmax=50.0, mode=mode)[0] for tmin in TMINS}
        hit = float((want[TMINS[0]]["prim"] != MISS).mean())
        assert hit_range[0] < hit < hit_range[1], (key, hit)          # hits and misses both (dense instance sets: hits enough)
        return r, want
    return cached(("trace", key), make)


def check_traces(pt, gs, rays, want, extends, what=""):
    for tmin in TMINS:
        for ext in extends:
            got = gs.trace(rays, tmin=tmin, tmax=50.0, extend=ext)
            bad = np.flatnonzero(got != want[tmin])
            assert got.tobytes() == want[tmin].tobytes(), (what, tmin, ext, len(bad), bad[:4])


def oracle_film(orc, key, v, i, f, instances=None, nee=False, frames=FRAMES, **kw):
    """-> (film f32, bgra8, rays) of the oracle after `frames` frames of FILM (kw overrides), once per key"""
    def make():
        osc = orc.Scene(v, i, f)
        if instances is not None:
            osc.set_instances(instances)
        args = dict(FILM, **kw)
        film = np.zeros((args["height"], args["width"], 3), f32)
        bgra = np.zeros((args["height"], args["width"], 4), np.uint8)
        rays = 0
        for k in range(frames):
            img, r, _, _ = osc.render_frame(orc.default_params(frame=k, **(dict(nee=1) if nee else {}), **args))
            orc.accumulate_f32(film, img, k)
            orc.accumulate_bgra8(bgra, img, k)
            rays += r
        assert film.any()
        return film, bgra, rays
    return cached(("film", key, nee, frames, tuple(sorted(kw.items()))), make)


def render(pt, ctx, gs, pipeline=None, flags=0, frames=FRAMES, **kw):
    """one pt_render of `frames` frames of FILM into a fresh film -> (film, bgra8, stats)"""
    args = dict(FILM, **kw)
    film = pt.Film(ctx, args["width"], args["height"])
    try:
        ctx.reset_stats()
        pt.render(gs, film, pt.default_params(frame=0, frame_count=frames, flags=flags, pipeline=pt.PIPELINE_WAVEFRONT if pipeline is None else pipeline, **args))
        return film.read_f32(), film.read_bgra8(), ctx.stats()
    finally:
        film.close()


def check_render(pt, ctx, gs, want, pipeline=None, flags=0, nee=False, what="", **kw):
    """film, bgra8 (the reference estimator's image; not under NEE) and ray count equal the oracle's -> stats"""
    film, bgra, st = render(pt, ctx, gs, pipeline, flags, **kw)
    ofilm, obgra, orays = want
    assert st.rays == orays, (what, pipeline, flags, st.rays, orays)
    assert film.tobytes() == ofilm.tobytes(), (what, pipeline, flags, float(np.abs(film - ofilm).max()))
    if not nee:
        assert bgra.tobytes() == obgra.tobytes(), (what, pipeline, flags)
    return st
