"""pt_film_enable_moments / pt_film_denoise_variance: the film's second-moment plane and the variance-guided a-trous filter of
include/pt_api.h.

`_variance_ref` is the numpy statement of the header's definition, written like test_denoise._denoise_ref: float32 throughout, the sums
written out, a shifted-array pass per tap in the order j outer / i inner.  `_moments_ref` restates the blend of the plane from the
oracle's per-frame colours.  The CPU tests check the value of the filter (the experiment of DESIGN.md section 14), that the colour stop is
exact where the variance is zero, the borders and the denormal weights; the GPU tests feed `_variance_ref` the film, the guides, the plane
and the frame count read back from the device.  Every GPU comparison is `tobytes()` equality."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_aov
import test_denoise
from test_denoise import GUIDES, H_TAPS, TINY, _denoise_ref, _oracle_guides, _rel_mse, _same, _to_bgra8

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
G_TAPS = [f32(0.25), f32(0.5), f32(0.25)]


def _shift(h, w, dx, dy):
    """-> (P, Q): the pixels whose tap (x + dx, y + dy) lies inside the image, and those taps; None when there are none"""
    x0, x1, y0, y1 = max(0, -dx), min(w, w - dx), max(0, -dy), min(h, h - dy)
    if x0 >= x1 or y0 >= y1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def _variance_ref(film, g, m2, frames, iterations=5, sigma_normal=0.5, sigma_depth=0.1, sigma_color=3.0, counts=None, parts=None):
    """-> (rgb float32 [H, W, 3], bgra uint8 [H, W, 4]).  film, g as in _denoise_ref; m2 [H, W, 3] the second-moment plane; frames = n.
    counts (a dict): taps whose weight is denormal / zero although t > 0 before the squarings.  parts (a dict): receives V0 and V."""
    C_ = np.ascontiguousarray(film, f32)
    M = np.ascontiguousarray(m2, f32)
    A, N, E, Z, al = (np.ascontiguousarray(g[k], f32) for k in GUIDES)
    assert all(a.dtype == f32 for a in (C_, M, A, N, E, Z, al)) and frames >= 2
    h, w = Z.shape
    one = f32(1.0)
    D = np.maximum(A + (one - al)[:, :, None], f32(0.001))
    I = (C_ - E) / D
    v = np.maximum(M - C_ * C_, f32(0.0)) / f32(frames - 1)
    vd = v / (D * D)
    V0 = (vd[:, :, 0] + vd[:, :, 1]) + vd[:, :, 2]
    assert V0.dtype == f32
    S = np.zeros((h, w), f32)
    W = np.zeros((h, w), f32)
    for j in range(-1, 2):
        for i in range(-1, 2):
            pq = _shift(h, w, i, j)
            if pq is None:
                continue
            P, Q = pq
            gg = G_TAPS[j + 1] * G_TAPS[i + 1]
            S[P] = S[P] + gg * V0[Q]
            W[P] = W[P] + gg
    V = S / W
    assert V.dtype == f32
    if parts is not None:
        parts["V0"], parts["V"] = V0, V
    inv_n = one / (f32(sigma_normal) * f32(sigma_normal))
    sz2 = f32(sigma_depth) * f32(sigma_depth)
    sc2 = f32(sigma_color) * f32(sigma_color)
    n_denormal = n_underflow = 0
    for k in range(iterations):
        s = 1 << k
        num = np.zeros((h, w, 3), f32)
        den = np.zeros((h, w), f32)
        vnum = np.zeros((h, w), f32)
        for j in range(-2, 3):
            for i in range(-2, 3):
                pq = _shift(h, w, s * i, s * j)
                if pq is None:
                    continue
                P, Q = pq
                dn = N[P] - N[Q]
                x_n = ((dn[:, :, 0] * dn[:, :, 0] + dn[:, :, 1] * dn[:, :, 1]) + dn[:, :, 2] * dn[:, :, 2]) * inv_n
                dz = Z[P] - Z[Q]
                x_z = (dz * dz) / (sz2 * (Z[P] * Z[P] + Z[Q] * Z[Q]) + f32(1e-12))
                di = I[P] - I[Q]
                with np.errstate(over="ignore"):   # (an infinite x_c is in the contract: weight 0)
                    x_c = ((di[:, :, 0] * di[:, :, 0] + di[:, :, 1] * di[:, :, 1]) + di[:, :, 2] * di[:, :, 2]) / (sc2 * (V[P] + V[Q]) + f32(1e-12))
                t = np.maximum(f32(0.0), one - ((x_n + x_z) + x_c) * f32(0.0625))
                t0 = t
                for _ in range(4):
                    t = t * t
                wgt = (H_TAPS[j + 2] * H_TAPS[i + 2]) * t
                assert wgt.dtype == f32
                n_denormal += int(((wgt > 0) & (wgt < TINY)).sum())
                n_underflow += int(((wgt == 0) & (t0 > 0)).sum())
                num[P] = num[P] + wgt[:, :, None] * I[Q]
                den[P] = den[P] + wgt
                vnum[P] = vnum[P] + (wgt * wgt) * V[Q]
        I = num / den[:, :, None]
        V = vnum / (den * den)
        assert I.dtype == f32 and V.dtype == f32
    out = I * D + E
    assert out.dtype == f32
    if counts is not None:
        counts["denormal"], counts["underflow"] = n_denormal, n_underflow
    return out, _to_bgra8(out)


def _blend(old, value, frame):
    """the film's blend: new = (value + old * frame) / (frame + 1), `old` not read for frame 0"""
    old = np.zeros_like(value) if frame == 0 else old
    out = (value + old * f32(frame)) / f32(frame + 1)
    assert out.dtype == f32
    return out


def _moments_ref(frame_colours, first=0, film=None, m2=None):
    """film and second-moment plane after the given frames' colours (float32 [H, W, 3] each), blended in order from frame `first`"""
    for k, c in enumerate(frame_colours):
        assert c.dtype == f32
        film = _blend(film, c, first + k)
        m2 = _blend(m2, c * c, first + k)
    return film, m2


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
def test_variance_params_layout_defaults_and_symbols(pt, tmp_path):
    """sizeof / offsetof of pt_denoise_variance_params by gcc from the header == the ctypes mirror (32 bytes); the defaults; the four new
    names in API_SYMBOLS and in the library; PT_API_VERSION stays 6."""
    fields = ["iterations", "sigma_normal", "sigma_depth", "sigma_color", "frames", "reserved"]
    src = tmp_path / "dv_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("%zu ' + "%zu " * len(fields) + '%d\\n",'
                   "sizeof(pt_denoise_variance_params), " + ", ".join(f"offsetof(pt_denoise_variance_params, {n})" for n in fields) +
                   ", PT_API_VERSION);return 0;}\n")
    exe = tmp_path / "dv_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = pt.DenoiseVarianceParams
    assert got == [C.sizeof(P)] + [getattr(P, n).offset for n in fields] + [6], got
    assert got[0] == 32
    for name in ("pt_film_enable_moments", "pt_film_read_moments", "pt_denoise_variance_params_default", "pt_film_denoise_variance"):
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    p = pt.denoise_variance_default_params()   # (touches no device)
    assert (p.iterations, p.sigma_normal, p.sigma_depth, p.sigma_color, p.frames, list(p.reserved)) == (5, 0.5, f32(0.1), 3.0, 0, [0] * 3)


def test_quality_variance_guided_against_guide_only(pt, orc):
    """The experiment of DESIGN.md section 14, test_denoise's own set-up: Cornell box 128 x 96, 4 spp per frame, frames 0..n-1 blended like
    the film (and their squares like the plane), guides of frame 0, 5 iterations, against the mean of 64 frames of 32 spp (frames
    1000..1063); relMSE as test_denoise._rel_mse.  Measured (noisy / guide-only / variance-guided at sigma_color 3 / at 4):
        n = 2    0.7999 / 0.0333 / 0.0215 / 0.0202
        n = 4    0.4328 / 0.0333 / 0.0145 / 0.0173        guide-only / variance-guided = 2.3
        n = 8    0.2171 / 0.0314 / 0.0097 / 0.0111        3.2
        n = 16   0.1096 / 0.0295 / 0.0080 / 0.0086        3.7
    (n = 2 and n = 16 are printed, not asserted: about 20 s of oracle time in all.)  Asserted: variance-guided <= guide-only / 1.5 at
    n = 4 and <= guide-only / 2 at n = 8 -- margins for other guide and seed choices, not for another filter."""
    q = test_denoise.QUALITY
    osc = test_aov._oracle_scene(pt, orc, q["scene"])
    kw = dict(width=q["w"], height=q["h"])
    ref = np.zeros((q["h"], q["w"], 3), np.float64)
    for k in range(q["ref_frames"]):
        ref += osc.render_frame(orc.default_params(frame=1000 + k, spp_per_frame=q["ref_spp"], **kw), nthreads=16)[0]
    ref /= q["ref_frames"]
    g = _oracle_guides(pt, orc, q["scene"], q["w"], q["h"], q["spp"], 0)
    film = m2 = None
    e = {}
    for n in range(1, 17):
        c = osc.render_frame(orc.default_params(frame=n - 1, spp_per_frame=q["spp"], **kw), nthreads=16)[0]
        film, m2 = _moments_ref([c], n - 1, film, m2)
        if n in (2, 4, 8, 16):
            e[n] = (_rel_mse(film, ref), _rel_mse(_denoise_ref(film, g)[0], ref), _rel_mse(_variance_ref(film, g, m2, n)[0], ref),
                    _rel_mse(_variance_ref(film, g, m2, n, sigma_color=4.0)[0], ref))
            print(f"n = {n}: relMSE noisy {e[n][0]:.4f}, guide-only {e[n][1]:.4f}, variance-guided sigma_color 3 {e[n][2]:.4f} "
                  f"(1 / {e[n][1] / e[n][2]:.2f}), sigma_color 4 {e[n][3]:.4f}")
    assert e[4][2] <= e[4][1] / 1.5, e[4]
    assert e[8][2] <= e[8][1] / 2.0, e[8]


def _two_levels(h, w, lo=0.25, hi=1.75):
    """uniform guides (albedo 1, no emission) under an image of two constant levels, zero variance: M = C * C exactly"""
    g = {"albedo": np.ones((h, w, 3), f32), "normal": np.zeros((h, w, 3), f32), "emission": np.zeros((h, w, 3), f32),
         "depth": np.full((h, w), 3.0, f32), "alpha": np.ones((h, w), f32)}
    g["normal"][:, :, 2] = 1.0
    film = np.full((h, w, 3), lo, f32)
    film[:, w // 2:] = f32(hi)
    return film, g, film * film


def test_colour_stop_is_exact_where_the_variance_is_zero():
    """Uniform guides, V = 0, an image of two constant levels: x_c across the step is step^2 * 3 / 1e-12, the weight 0, so every output
    pixel is a weighted mean of equal values -- within 1e-5 relative of its own side's level (26 roundings of such a mean are about
    1.6e-6).  The guide-only filter on the same planes moves the pixels at the edge by more than 1 % of the step."""
    film, g, m2 = _two_levels(24, 40)
    parts = {}
    out, _ = _variance_ref(film, g, m2, 2, iterations=5, parts=parts)
    assert not parts["V"].any()
    assert (np.abs(out - film) <= f32(1e-5) * film).all(), float((np.abs(out - film) / film).max())
    plain, _ = _denoise_ref(film, g, iterations=5)
    step = 1.75 - 0.25
    assert np.abs(plain[:, 19:21] - film[:, 19:21]).min() > 0.01 * step
    # and with variance on one side only the other side still stops at its own pixels' zero sum: V_p + V_q > 0 lets a tap through
    m2b = m2.copy()
    m2b[:, 20:] = m2b[:, 20:] + f32(4.0)
    out_b, _ = _variance_ref(film, g, m2b, 2, iterations=5)
    assert np.abs(out_b[:, 19:21] - film[:, 19:21]).max() > 0.01 * step


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (40, 5)])
def test_variance_borders_when_the_step_exceeds_the_image(shape):
    """1 x 1, 3 x 2 and 5 x 40 (width x height) with 8 iterations (steps up to 128): finite, no division by zero or invalid operation;
    the 1 x 1 image is the centre taps alone."""
    h, w = shape
    film, g = test_denoise._synthetic(h, w, 4)
    rng = np.random.default_rng(9)
    m2 = (film * film + rng.uniform(0.0, 0.5, film.shape).astype(f32)).astype(f32)
    g["alpha"][0, 0] = 0.0   # a miss: D = albedo + 1, depth and normal 0
    g["depth"][0, 0] = 0.0
    g["normal"][0, 0] = 0.0
    with np.errstate(divide="raise", invalid="raise", over="raise"):
        parts = {}
        out, bgra = _variance_ref(film, g, m2, 3, iterations=8, parts=parts)
    assert out.shape == (h, w, 3) and np.isfinite(out).all() and bgra.shape == (h, w, 4) and (parts["V"] > 0).all()
    if shape == (1, 1):
        D = test_denoise._demod(g)
        I = (film - g["emission"]) / D
        w0 = H_TAPS[2] * H_TAPS[2]
        for _ in range(8):
            I = (w0 * I) / w0
        assert out.tobytes() == (I * D + g["emission"]).tobytes()
        assert parts["V"].tobytes() == ((f32(0.25) * parts["V0"]) / f32(0.25)).tobytes()


def _sweep_with_variance(w, h):
    """test_denoise._sweep_planes (weights in and below the denormal range through x_n) with a plane M that gives the pixels variances over
    six decades, and none at all in two blocks, so that x_c takes part in the sweep"""
    film, g = test_denoise._sweep_planes(w, h)
    rng = np.random.default_rng(12)
    var = (10.0 ** rng.uniform(-4.0, 2.0, (h, w, 1)) * rng.uniform(0.2, 1.0, (h, w, 3))).astype(f32)
    var[: h // 4, : w // 3] = 0.0
    var[h // 2:, w // 2:] = 0.0
    m2 = (film * film + var).astype(f32)
    return film, g, m2


def test_reference_sees_denormal_weights_with_variance():
    """The sweep the GPU parity test uploads makes weights whose t^16 is denormal, and weights that underflow to 0, with V in play: V0 is
    positive in most pixels and exactly zero in the two blocks."""
    film, g, m2 = _sweep_with_variance(64, 48)
    counts, parts = {}, {}
    _variance_ref(film, g, m2, 4, iterations=3, sigma_color=8.0, counts=counts, parts=parts)
    assert counts["denormal"] > 100 and counts["underflow"] > 100, counts
    assert (parts["V0"] > 0).mean() > 0.5 and (parts["V0"][:10, :18] == 0).all() and (parts["V0"][26:, 34:] == 0).all()


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
_scene = test_denoise._scene


def _oracle_frames(pt, orc, scene, w, h, spp, cam, frames, nee=False, max_depth=4, faces=None):
    osc = test_aov._oracle_scene(pt, orc, scene, faces)
    extra = dict(nee=1) if nee else {}
    return [osc.render_frame(orc.default_params(frame=k, width=w, height=h, spp_per_frame=spp, max_depth=max_depth, **cam, **extra))[0] for k in frames]


# (case of test_denoise.CASES, frames, [(pipeline, flags)]): the soup does not fit the fused kernels' LDS, the fused NEE kernel takes no instances
MOMENT_CASES = [
    ("cornell_odd", 3, [("WAVEFRONT", 0), ("FUSED", 0), ("AUTO", 0), ("WAVEFRONT", "NEE"), ("FUSED", "NEE")]),
    ("grid16", 2, [("WAVEFRONT", 0), ("FUSED", 0), ("AUTO", 0)]),
    ("soup", 2, [("WAVEFRONT", 0), ("AUTO", 0), ("WAVEFRONT", "NEE")]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case,n,pipelines", MOMENT_CASES, ids=[c[0] for c in MOMENT_CASES])
def test_moments_parity(pt, orc, gpu_ctx, case, n, pipelines):
    """M after frames 0..n-1 == the blend of the oracle's squared frame colours, rendered as n frames in one call and as n calls of one
    frame; the film beside it is the oracle's; `frames` is frame + frame_count of the last call; pt_film_clear zeroes both."""
    scene, w, h, spp, cam = test_denoise.CASES[case]
    sc = _scene(pt, gpu_ctx, scene)
    want = {}
    for pipeline, flags in pipelines:
        nee = flags == "NEE"
        if nee not in want:
            want[nee] = _moments_ref(_oracle_frames(pt, orc, scene, w, h, spp, cam, range(n), nee=nee))
        ofilm, om2 = want[nee]
        kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=4, pipeline=getattr(pt, "PIPELINE_" + pipeline), flags=pt.FLAG_NEE if nee else 0, **cam)
        film = pt.Film(gpu_ctx, w, h)
        try:
            film.enable_moments()
            m2, frames = film.read_moments()
            assert not m2.any() and frames == 0
            for calls in ([(0, n)], [(k, 1) for k in range(n)]):
                for f0, cnt in calls:
                    pt.render(sc, film, pt.default_params(frame=f0, frame_count=cnt, **kw))
                    assert film.read_moments()[1] == f0 + cnt
                m2, frames = film.read_moments()
                what = (case, pipeline, flags, calls)
                assert frames == n and m2.dtype == f32 and m2.shape == (h, w, 3), what
                assert film.read_f32().tobytes() == ofilm.tobytes(), what
                assert m2.tobytes() == om2.tobytes(), (what, int((m2 != om2).sum()), float(np.abs(m2 - om2).max()))
                assert m2.any()
                film.clear()
                m2, frames = film.read_moments()
                assert not m2.any() and frames == 0 and not film.read_f32().any()
        finally:
            film.close()


@pytest.mark.gpu
def test_moments_through_every_resolve_shape(pt, orc, gpu_ctx, cornell_gpu, cornell_arrays):
    """The shapes k_resolve serves: frames in flight 1 and several (batches of frames), several sample groups (the term logs), the fused
    head + tail form, and a batch that is redone after a term-log overflow on both pipelines (the plane is blended once, from the redone
    batch).  One oracle statement per scene; the film is checked beside the plane."""
    w, h, spp, n = 52, 36, 8, 5
    kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=6)
    want = _moments_ref(_oracle_frames(pt, orc, "cornell", w, h, spp, {}, range(n), max_depth=6))

    def check(scene, want, calls, tuning, expect=None, **shape):
        old = gpu_ctx.set_tuning(**tuning)
        film = pt.Film(gpu_ctx, w, h)
        try:
            film.enable_moments()
            gpu_ctx.reset_stats()
            for f0, cnt in calls:
                pt.render(scene, film, pt.default_params(frame=f0, frame_count=cnt, **{**kw, **shape}))
            st = gpu_ctx.stats()
            m2, frames = film.read_moments()
            what = (calls, tuning, shape)
            assert frames == calls[-1][0] + calls[-1][1], what
            assert film.read_f32().tobytes() == want[0].tobytes(), what
            assert m2.tobytes() == want[1].tobytes(), (what, int((m2 != want[1]).sum()))
            if expect:
                expect(st)
        finally:
            film.close()
            gpu_ctx.set_tuning(**old)

    def groups(st):
        assert st.sample_groups == 4, st.sample_groups

    def tail(st):
        assert st.tail_samples == 3, st.tail_samples

    def redone(st):
        assert st.redone_batches > 0, st.redone_batches

    for pipeline in (pt.PIPELINE_WAVEFRONT, pt.PIPELINE_FUSED):
        for fif in (1, 2, n):
            check(cornell_gpu, want, [(0, n)], {}, pipeline=pipeline, frames_in_flight=fif)
        check(cornell_gpu, want, [(0, 2), (2, 3)], {}, pipeline=pipeline, sample_groups=4, expect=groups)
    check(cornell_gpu, want, [(0, 1), (1, 4)], dict(fused_tail=3), pipeline=pt.PIPELINE_FUSED, frames_in_flight=2, expect=tail)
    # every surface emits, so every ray logs a term: with a pool of three entries a batch overflows and is rendered again with one group
    v, i, f = cornell_arrays
    f = f.reshape(-1, 6).copy()
    f[:, 3:] = f32(0.25) + f[:, :3] * f32(0.5)
    gs = pt.Scene(gpu_ctx, v, i, f.reshape(-1))
    try:
        kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=12)
        want_e = _moments_ref(_oracle_frames(pt, orc, "cornell", w, h, spp, {}, range(n), max_depth=12, faces=f.reshape(-1)))
        check(gs, want_e, [(0, 1), (1, 4)], dict(term_ocap=0, term_spill=3), pipeline=pt.PIPELINE_WAVEFRONT, sample_groups=4, frames_in_flight=2, expect=redone)
        check(gs, want_e, [(0, 3), (3, 2)], dict(term_ocap=0, term_spill=3, fused_tail=4), pipeline=pt.PIPELINE_FUSED, frames_in_flight=2, expect=redone)
    finally:
        gs.close()


@pytest.mark.gpu
def test_moments_async_render_queues_the_blend(pt, gpu_ctx, cornell_gpu):
    """PT_FLAG_ASYNC: the blend of M is queued with the resolve -- the same bytes as the blocking render once the stream is idle."""
    w, h = 52, 36
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=4, frame=0, frame_count=3, pipeline=pt.PIPELINE_WAVEFRONT)
    a, b = pt.Film(gpu_ctx, w, h), pt.Film(gpu_ctx, w, h)
    try:
        a.enable_moments(); b.enable_moments()
        pt.render(cornell_gpu, a, pt.default_params(**kw))
        pt.render(cornell_gpu, b, pt.default_params(flags=pt.FLAG_ASYNC, **kw))
        gpu_ctx.sync()
        assert a.read_moments()[0].tobytes() == b.read_moments()[0].tobytes() and b.read_moments()[1] == 3 and a.read_moments()[0].any()
        assert a.read_f32().tobytes() == b.read_f32().tobytes()
    finally:
        a.close(); b.close()


def _film_with_everything(pt, ctx, case, pipeline, n_frames, moments=True, max_depth=4, one_call=False):
    """test_denoise._rendered_film with the second-moment plane enabled before the frames"""
    scene, w, h, spp, cam = test_denoise.CASES[case]
    sc = _scene(pt, ctx, scene)
    film = pt.Film(ctx, w, h)
    film.enable_aov()
    if moments:
        film.enable_moments()
    kw = dict(width=w, height=h, spp_per_frame=spp, pipeline=pipeline, **cam)
    for f0, cnt in ([(0, n_frames)] if one_call else [(k, 1) for k in range(n_frames)]):
        pt.render(sc, film, pt.default_params(frame=f0, frame_count=cnt, max_depth=max_depth, **kw))
    pt.render_aov(sc, film, pt.default_params(frame=0, frame_count=n_frames, **kw))
    return film


def _read_inputs(film, pt):
    rgb, g = test_denoise._read_inputs(film, pt)
    m2, frames = film.read_moments()
    return rgb, g, m2, frames


@pytest.mark.gpu
def test_the_plane_moves_nothing_else(pt, gpu_ctx):
    """Film, bgra8, pt_stats.rays / .paths of a film with the plane == those of a twin without it; pt_film_denoise gives the same bytes on
    both; pt_film_denoise_variance leaves film, bgra8, guides, M, frames and stats as they were, and rendering goes on afterwards."""
    for pipeline in (pt.PIPELINE_WAVEFRONT, pt.PIPELINE_AUTO):
        gpu_ctx.reset_stats()
        twin = _film_with_everything(pt, gpu_ctx, "cornell", pipeline, 3, moments=False)
        st_twin = gpu_ctx.stats()
        gpu_ctx.reset_stats()
        film = _film_with_everything(pt, gpu_ctx, "cornell", pipeline, 3)
        st = gpu_ctx.stats()
        try:
            assert (st.rays, st.paths, st.pipeline, st.workspace_bytes, st.launches_other) == (st_twin.rays, st_twin.paths, st_twin.pipeline, st_twin.workspace_bytes, st_twin.launches_other)
            assert film.read_f32().tobytes() == twin.read_f32().tobytes() and film.read_bgra8().tobytes() == twin.read_bgra8().tobytes()
            film.denoise(); twin.denoise()
            assert film.read_denoised().tobytes() == twin.read_denoised().tobytes() and film.read_denoised_bgra8().tobytes() == twin.read_denoised_bgra8().tobytes()

            def state():
                s = gpu_ctx.stats()
                m2, frames = film.read_moments()
                return ([film.read_f32().tobytes(), film.read_bgra8().tobytes(), m2.tobytes(), frames] + [film.read_aov(k).tobytes() for k in range(pt.AOV_COUNT)],
                        (s.rays, s.paths, s.ms_total))
            before = state()
            film.denoise_variance()
            film.denoise_variance(iterations=2, sigma_color=1.0)
            assert state() == before
            assert film.read_denoised().tobytes() != twin.read_denoised().tobytes()
            scene, w, h, spp, cam = test_denoise.CASES["cornell"]
            for f_ in (film, twin):
                pt.render(_scene(pt, gpu_ctx, scene), f_, pt.default_params(frame=3, frame_count=1, max_depth=4, width=w, height=h, spp_per_frame=spp, pipeline=pipeline, **cam))
            assert film.read_f32().tobytes() == twin.read_f32().tobytes() and film.read_moments()[1] == 4
        finally:
            film.close(); twin.close()


# (iterations, sigma_normal, sigma_depth, sigma_color): every rendered film runs all of them
COMBOS = [(5, 0.5, 0.1, 3.0), (1, 0.5, 0.1, 3.0), (3, 0.5, 0.1, 1.0), (8, 0.5, 0.1, 4.0), (5, 0.1, 0.02, 8.0), (4, 2.0, 0.1, 2.0), (2, 2.0, 0.02, 0.5)]


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["WAVEFRONT", "AUTO"])
@pytest.mark.parametrize("n_frames", [2, 4])
@pytest.mark.parametrize("case", sorted(test_denoise.CASES))
def test_denoise_variance_parity(pt, gpu_ctx, case, n_frames, pipeline):
    film = _film_with_everything(pt, gpu_ctx, case, getattr(pt, "PIPELINE_" + pipeline), n_frames, one_call=n_frames == 4)
    try:
        rgb, g, m2, frames = _read_inputs(film, pt)
        assert frames == n_frames and m2.any()
        for it, sn, sz, sc in COMBOS:
            ms = film.denoise_variance(iterations=it, sigma_normal=sn, sigma_depth=sz, sigma_color=sc)
            assert ms > 0
            _same(film.read_denoised(), film.read_denoised_bgra8(), _variance_ref(rgb, g, m2, frames, it, sn, sz, sc), (case, n_frames, pipeline, it, sn, sz, sc))
    finally:
        film.close()


def _external_film(pt, ctx, torch, rgb, g, m2):
    """test_denoise._external_film plus an external second-moment plane holding m2"""
    film, keep = test_denoise._external_film(pt, ctx, torch, rgb, g)
    t_m2 = torch.full(m2.shape, 5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()                      # (torch fills on its own stream, the library zeroes on the context's)
    film.enable_moments(t_m2.data_ptr())
    assert not t_m2.any().item()                  # (zeroed by the call: filled afterwards)
    t_m2.copy_(torch.from_numpy(np.ascontiguousarray(m2)))
    torch.cuda.synchronize()
    return film, (keep, t_m2)


@pytest.mark.gpu
def test_denoise_variance_synthetic_planes(pt, gpu_ctx):
    """Planes made on the host in external tensors, at an odd size: the denormal sweep with V over six decades and blocks of zero V;
    params.frames named explicitly (the film has rendered nothing: it recorded 0, which alone is refused); the two-level image."""
    import torch
    film_np, g, m2_np = _sweep_with_variance(77, 53)
    counts = {}
    want = _variance_ref(film_np, g, m2_np, 4, 3, 0.5, 0.1, 8.0, counts=counts)
    assert counts["denormal"] > 100 and counts["underflow"] > 100, counts
    film, keep = _external_film(pt, gpu_ctx, torch, film_np, g, m2_np)
    try:
        rgb, g_dev, m2, frames = _read_inputs(film, pt)
        assert frames == 0 and rgb.tobytes() == film_np.tobytes() and m2.tobytes() == m2_np.tobytes() and all(g_dev[n].tobytes() == g[n].tobytes() for n in GUIDES)
        with pytest.raises(pt.PtError) as e:
            film.denoise_variance()
        assert e.value.status == 1
        film.denoise_variance(iterations=3, sigma_color=8.0, frames=4)
        _same(film.read_denoised(), film.read_denoised_bgra8(), want, "sweep, 3 iterations, n = 4")
        for it, sc, n in ((8, 3.0, 2), (5, 1.0, 9), (1, 3.0, 1000)):
            film.denoise_variance(iterations=it, sigma_color=sc, frames=n)
            _same(film.read_denoised(), film.read_denoised_bgra8(), _variance_ref(film_np, g, m2_np, n, it, 0.5, 0.1, sc), ("sweep", it, sc, n))
    finally:
        film.close()
    del keep
    film_np, g, m2_np = _two_levels(37, 61)
    film, keep = _external_film(pt, gpu_ctx, torch, film_np, g, m2_np)
    try:
        film.denoise_variance(frames=2)
        got = film.read_denoised()
        _same(got, film.read_denoised_bgra8(), _variance_ref(film_np, g, m2_np, 2), "two levels")
        assert (np.abs(got - film_np) <= f32(1e-5) * film_np).all()
    finally:
        film.close()
    del keep


@pytest.mark.gpu
def test_denoise_variance_1080p_cornell_film(pt, gpu_ctx, cornell_gpu):
    """One 1920 x 1080 Cornell film of 8 frames x 4 spp, 5 iterations.  As test_denoise's 1080p test: three 256 x 256 crops, each crop's
    reference computed from inputs cropped with a 63-pixel halo (2 * (1 + 2 + 4 + 8 + 16) = 62 for the iterations, + 1 for the pre-blur),
    clipped at the image's edge."""
    w, h, spp, n, halo = 1920, 1080, 4, 8, 63
    film = pt.Film(gpu_ctx, w, h)
    film.enable_aov()
    film.enable_moments()
    try:
        kw = dict(width=w, height=h, spp_per_frame=spp, frame=0, frame_count=n, pipeline=pt.PIPELINE_AUTO)
        pt.render(cornell_gpu, film, pt.default_params(max_depth=8, **kw))
        pt.render_aov(cornell_gpu, film, pt.default_params(**kw))
        rgb, g, m2, frames = _read_inputs(film, pt)
        assert frames == n
        film.denoise_variance()
        got, got_bgra = film.read_denoised(), film.read_denoised_bgra8()
        for x0, y0 in ((0, 0), (w - 256, h - 256), (832, 412)):
            hx0, hy0, hx1, hy1 = max(0, x0 - halo), max(0, y0 - halo), min(w, x0 + 256 + halo), min(h, y0 + 256 + halo)
            sub = {k: np.ascontiguousarray(g[k][hy0:hy1, hx0:hx1]) for k in GUIDES}
            ref, ref_bgra = _variance_ref(np.ascontiguousarray(rgb[hy0:hy1, hx0:hx1]), sub, np.ascontiguousarray(m2[hy0:hy1, hx0:hx1]), frames)
            ys, xs = slice(y0 - hy0, y0 - hy0 + 256), slice(x0 - hx0, x0 - hx0 + 256)
            _same(np.ascontiguousarray(got[y0:y0 + 256, x0:x0 + 256]), np.ascontiguousarray(got_bgra[y0:y0 + 256, x0:x0 + 256]),
                  (np.ascontiguousarray(ref[ys, xs]), np.ascontiguousarray(ref_bgra[ys, xs])), ("crop", x0, y0))
        assert g["alpha"][412:668, 832:1088].any() and not np.array_equal(got, rgb)
    finally:
        film.close()


@pytest.mark.gpu
def test_denoise_variance_placement(pt, gpu_ctx):
    """External output == the film-owned plane (which that call leaves alone); a film over external radiance, guides and M == one that
    owns them; and external M together with external output."""
    import torch
    film = _film_with_everything(pt, gpu_ctx, "cornell_odd", pt.PIPELINE_AUTO, 3)
    try:
        _, w, h, _, _ = test_denoise.CASES["cornell_odd"]
        rgb, g, m2, frames = _read_inputs(film, pt)
        film.denoise_variance(iterations=4)
        own, own_bgra = film.read_denoised(), film.read_denoised_bgra8()
        _same(own, own_bgra, _variance_ref(rgb, g, m2, frames, 4), "owned")
        out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        film.denoise_variance(iterations=2)
        two = film.read_denoised()
        film.denoise_variance(iterations=4, device_out=out.data_ptr())
        assert out.cpu().numpy().tobytes() == own.tobytes()
        assert film.read_denoised().tobytes() == two.tobytes()
        ext, keep = _external_film(pt, gpu_ctx, torch, rgb, g, m2)
        try:
            ext.denoise_variance(iterations=4, frames=frames)
            _same(ext.read_denoised(), ext.read_denoised_bgra8(), (own, own_bgra), "external planes")
            out.fill_(7.0)
            torch.cuda.synchronize()
            ext.denoise_variance(iterations=4, frames=frames, device_out=out.data_ptr())
            assert out.cpu().numpy().tobytes() == own.tobytes()
        finally:
            ext.close()
        del keep
        # a film that renders into an external plane
        t_m2 = torch.full((h, w, 3), 3.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        scene, _, _, spp, cam = test_denoise.CASES["cornell_odd"]
        other = pt.Film(gpu_ctx, w, h)
        try:
            other.enable_moments(t_m2.data_ptr())
            pt.render(_scene(pt, gpu_ctx, scene), other, pt.default_params(frame=0, frame_count=3, max_depth=4, width=w, height=h, spp_per_frame=spp, pipeline=pt.PIPELINE_AUTO, **cam))
            assert t_m2.cpu().numpy().tobytes() == m2.tobytes() and other.read_moments()[0].tobytes() == m2.tobytes()
        finally:
            other.close()
    finally:
        film.close()


@pytest.mark.gpu
def test_denoise_variance_repeatability_and_memory(pt, cornell_arrays):
    """Two calls give the same bytes; free device memory is unchanged across further calls (of either filter: they share the scratch); a
    budget too small for the scratch is PT_ERR_OOM, writes no result, and the film renders on."""
    import torch
    w, h, spp = 160, 120, 4
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *cornell_arrays)
    kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=4, pipeline=pt.PIPELINE_AUTO)
    film, other, alone = pt.Film(ctx, w, h), pt.Film(ctx, w, h), pt.Film(ctx, w, h)
    try:
        for f in (film, other):
            f.enable_aov()
            f.enable_moments()
            pt.render(sc, f, pt.default_params(frame=0, frame_count=2, **kw))
            pt.render_aov(sc, f, pt.default_params(frame=0, frame_count=2, **kw))
        film.denoise_variance()
        first = film.read_denoised().tobytes(), film.read_denoised_bgra8().tobytes()
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        film.denoise_variance()
        film.denoise()
        film.denoise_variance()
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
        assert free1 == free0, (free0, free1)
        assert (film.read_denoised().tobytes(), film.read_denoised_bgra8().tobytes()) == first
        # `other` has no scratch yet: 160 * 120 pixels * 48 B = 0.9 MB of scratch + 0.3 MB of output do not fit 1 MB
        old = ctx.set_tuning(mem_budget_mb=1)
        with pytest.raises(pt.PtError) as e:
            other.denoise_variance()
        assert e.value.status == 4
        with pytest.raises(pt.PtError) as e:
            other.read_denoised()
        assert e.value.status == 1
        pt.render(sc, other, pt.default_params(frame=2, frame_count=1, **kw))      # the same shape again: nothing to allocate
        ctx.set_tuning(**old)
        pt.render(sc, alone, pt.default_params(frame=0, frame_count=3, **kw))
        assert other.read_f32().tobytes() == alone.read_f32().tobytes()
        other.denoise_variance()                                                    # and with the budget back the call goes through
        rgb, g, m2, frames = _read_inputs(other, pt)
        assert frames == 3
        _same(other.read_denoised(), other.read_denoised_bgra8(), _variance_ref(rgb, g, m2, frames), "after the refusal")
    finally:
        for f in (film, other, alone):
            f.close()
        sc.close()
        ctx.close()


@pytest.mark.gpu
def test_denoise_variance_errors(pt, gpu_ctx, cornell_gpu):
    """Every PT_ERR_INVALID_ARG case of the header; a refused call writes no result."""
    lib = pt.lib_amd()
    w, h = 48, 40
    film = pt.Film(gpu_ctx, w, h)

    def status(fn):
        with pytest.raises(pt.PtError) as e:
            fn()
        return e.value.status

    good = pt.denoise_variance_default_params()
    good.frames = 2
    assert lib.pt_film_denoise_variance(None, C.byref(good), None, None) == 1      # NULL film
    assert lib.pt_film_denoise_variance(film.h, None, None, None) == 1              # NULL params
    assert lib.pt_film_enable_moments(None, None) == 1
    assert lib.pt_film_read_moments(None, None, None) == 1
    assert status(lambda: film.read_moments()) == 1                                 # no plane
    assert status(lambda: film.denoise_variance(frames=2)) == 1                     # no guides (and no plane)
    film.enable_moments()
    assert status(lambda: film.denoise_variance(frames=2)) == 1                     # no guides
    assert status(lambda: film.enable_moments()) == 1                               # a second call
    assert lib.pt_film_read_moments(film.h, None, None) == 0                        # either pointer may be NULL
    plain = pt.Film(gpu_ctx, w, h)
    plain.enable_aov()
    assert status(lambda: plain.denoise_variance(frames=2)) == 1                    # guides, but no plane
    plain.close()
    film.enable_aov()
    assert status(lambda: film.denoise_variance()) == 1                             # nothing rendered: frames resolves to 0
    assert status(lambda: film.denoise_variance(frames=1)) == 1
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=3, pipeline=pt.PIPELINE_AUTO)
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=1, **kw))
    assert status(lambda: film.denoise_variance()) == 1                             # one frame: no variance estimate
    pt.render(cornell_gpu, film, pt.default_params(frame=1, frame_count=1, **kw))
    for it in (0, 9, 0xFFFFFFFF):
        assert status(lambda: film.denoise_variance(iterations=it)) == 1
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        for name in ("sigma_normal", "sigma_depth", "sigma_color"):
            assert status(lambda: film.denoise_variance(**{name: bad})) == 1, (name, bad)
    for k in range(3):
        p = pt.denoise_variance_default_params()
        p.reserved[k] = 1
        assert status(lambda: film.denoise_variance(params=p)) == 1
    assert status(lambda: film.read_denoised()) == 1                                # a refused call writes nothing
    film.denoise_variance()                                                         # two frames recorded: goes through
    assert film.read_denoised().shape == (h, w, 3)
    film.close()


@pytest.mark.gpu
def test_pt_main_sigma_color(pt, tmp_path):
    """pt_main --denoise 3 --sigma-color 3 writes the bytes of Film.read_denoised / read_denoised_bgra8 after the same calls through the
    library; the normal outputs and the JSON line's figures are those of a run without it; --sigma-color without --denoise, with --ranks or
    with a value that is not > 0 exits non-zero."""
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_main")
    if not os.path.exists(exe):
        pt.build()
    w, h = 48, 40
    base = [exe, "--obj", pt.ASSET_CORNELL, "--width", str(w), "--height", str(h), "--frames", "3", "--spp", "4", "--depth", "3"]
    plain = subprocess.run(base + ["--ppm", str(tmp_path / "a.ppm"), "--pfm", str(tmp_path / "a.pfm")], check=True, capture_output=True, text=True, cwd=pt.REPO)
    run = subprocess.run(base + ["--ppm", str(tmp_path / "b.ppm"), "--pfm", str(tmp_path / "b.pfm"), "--denoise", "3", "--sigma-color", "3"],
                         check=True, capture_output=True, text=True, cwd=pt.REPO)
    ja, jb = (json.loads(x.stdout.strip().splitlines()[-1]) for x in (plain, run))
    assert ja["rays"] == jb["rays"] and ja["paths"] == jb["paths"] == w * h * 4 * 3
    for ext in ("ppm", "pfm"):
        assert open(tmp_path / f"a.{ext}", "rb").read() == open(tmp_path / f"b.{ext}", "rb").read(), ext
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    raw = open(tmp_path / "b.denoised.pfm", "rb").read()
    assert raw.startswith(head)
    den = np.ascontiguousarray(np.frombuffer(raw[len(head):], f32).reshape(h, w, 3)[::-1])
    ppm_head = f"P6\n{w} {h}\n255\n".encode()
    ppm = open(tmp_path / "b.denoised.ppm", "rb").read()
    assert ppm.startswith(ppm_head) and len(ppm) == len(ppm_head) + w * h * 3
    for misuse in (["--sigma-color", "3"], ["--denoise", "--sigma-color", "3", "--ranks", "2"], ["--denoise", "--sigma-color", "0"], ["--denoise", "--sigma-color"]):
        bad = subprocess.run(base + misuse, capture_output=True, text=True, cwd=pt.REPO)
        assert bad.returncode != 0 and "--sigma-color" in bad.stderr, misuse
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    film = pt.Film(ctx, w, h)
    film.enable_moments()
    film.enable_aov()
    kw = dict(width=w, height=h, spp_per_frame=4, frame=0, frame_count=3, pipeline=pt.PIPELINE_AUTO)
    pt.render(sc, film, pt.default_params(max_depth=3, **kw))
    pt.render_aov(sc, film, pt.default_params(**kw))
    film.denoise_variance(iterations=3, sigma_color=3.0)
    assert den.tobytes() == film.read_denoised().tobytes()
    bgra = film.read_denoised_bgra8()
    assert ppm[len(ppm_head):] == np.ascontiguousarray(bgra[:, :, 2::-1]).tobytes()
    film.denoise(iterations=3)
    assert den.tobytes() != film.read_denoised().tobytes()
    film.close(); sc.close(); ctx.close()
