"""pt_film_denoise: the guide-driven edge-avoiding a-trous filter of include/pt_api.h.

`_denoise_ref` is the numpy statement of the header's definition: float32 throughout, the three-term sums written out, taps in the
order j = -2..2 (outer), i = -2..2 (inner), a tap outside the image skipped -- a shifted-array pass per tap adds exactly what the per-pixel
loop adds, in the same order.  The CPU tests check the value of the filter (against the oracle's converged render), that the edge stop is
exact, and the borders; the GPU tests feed `_denoise_ref` the film and guide planes read back from the device, so that the comparison
is about the filter alone.  Every GPU comparison is `tobytes()` equality, of the float plane and of the bgra8 image."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_aov

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
H_TAPS = [f32(1.0 / 16.0), f32(1.0 / 4.0), f32(3.0 / 8.0), f32(1.0 / 4.0), f32(1.0 / 16.0)]
GUIDES = ["albedo", "normal", "emission", "depth", "alpha"]
TINY = f32(2.0 ** -126)   # the smallest normal binary32


def _demod(g):
    return np.maximum(g["albedo"] + (f32(1.0) - g["alpha"])[:, :, None], f32(0.001))


def _to_bgra8(rgb):
    """k_resolve's clamp and quantise rule; A = 255 (what the film's rgba8 image holds after frame 0 of this colour)"""
    c = np.where(rgb > 0, np.minimum(rgb, f32(1.0)), f32(0.0)).astype(f32)
    q = (c * f32(255.0) + f32(0.5)).astype(np.uint8)
    out = np.empty(rgb.shape[:2] + (4,), np.uint8)
    out[:, :, 0], out[:, :, 1], out[:, :, 2], out[:, :, 3] = q[:, :, 2], q[:, :, 1], q[:, :, 0], 255
    return out


def _denoise_ref(film, g, iterations=5, sigma_normal=0.5, sigma_depth=0.1, counts=None):
    """-> (rgb float32 [H, W, 3], bgra uint8 [H, W, 4]).  g: {albedo, normal, emission [H, W, 3]; depth, alpha [H, W]} as stored.
    counts (a dict): receives how many taps had a weight that is denormal / zero although t > 0 before the squarings."""
    C_ = np.ascontiguousarray(film, f32)
    A, N, E, Z, al = (np.ascontiguousarray(g[k], f32) for k in GUIDES)
    assert all(a.dtype == f32 for a in (C_, A, N, E, Z, al))
    h, w = Z.shape
    one = f32(1.0)
    D = np.maximum(A + (one - al)[:, :, None], f32(0.001))
    I = (C_ - E) / D
    inv_n = one / (f32(sigma_normal) * f32(sigma_normal))
    sz2 = f32(sigma_depth) * f32(sigma_depth)
    n_denormal = n_underflow = 0
    for k in range(iterations):
        s = 1 << k
        num = np.zeros((h, w, 3), f32)
        den = np.zeros((h, w), f32)
        for j in range(-2, 3):
            for i in range(-2, 3):
                dx, dy = s * i, s * j
                x0, x1, y0, y1 = max(0, -dx), min(w, w - dx), max(0, -dy), min(h, h - dy)
                if x0 >= x1 or y0 >= y1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                dn = N[P] - N[Q]
                x_n = ((dn[:, :, 0] * dn[:, :, 0] + dn[:, :, 1] * dn[:, :, 1]) + dn[:, :, 2] * dn[:, :, 2]) * inv_n
                dz = Z[P] - Z[Q]
                x_z = (dz * dz) / (sz2 * (Z[P] * Z[P] + Z[Q] * Z[Q]) + f32(1e-12))
                t = np.maximum(f32(0.0), one - (x_n + x_z) * f32(0.0625))
                t0 = t
                for _ in range(4):
                    t = t * t
                wgt = (H_TAPS[j + 2] * H_TAPS[i + 2]) * t
                assert wgt.dtype == f32
                n_denormal += int(((wgt > 0) & (wgt < TINY)).sum())
                n_underflow += int(((wgt == 0) & (t0 > 0)).sum())
                num[P] = num[P] + wgt[:, :, None] * I[Q]
                den[P] = den[P] + wgt
        I = num / den[:, :, None]
        assert I.dtype == f32
    out = I * D + E
    assert out.dtype == f32
    if counts is not None:
        counts["denormal"], counts["underflow"] = n_denormal, n_underflow
    return out, _to_bgra8(out)


def _rel_mse(a, ref):
    a, ref = a.astype(np.float64), ref.astype(np.float64)
    return float(np.mean((a - ref) ** 2 / (ref ** 2 + 0.01)))


def _oracle_guides(pt, orc, scene, w, h, spp, frame, cam=None):
    """The five float guide planes of one frame into zeroed planes, the way test_aov._guides builds them (oracle bindings only)."""
    cam = cam or {}
    faces = np.asarray(test_aov._arrays(pt, scene)[2], f32).reshape(-1, 6)
    osc = test_aov._oracle_scene(pt, orc, scene)
    p = orc.default_params(frame=frame, width=w, height=h, spp_per_frame=spp, **cam)
    rays = np.zeros((h, w, spp, 6), f32)
    for y in range(h):
        for x in range(w):
            for s in range(spp):
                o, d, _ = orc.primary_ray(p, x, y, orc.seed(x, y, s, frame, spp))
                rays[y, x, s, :3] = o
                rays[y, x, s, 3:] = d
    hits, _ = osc.trace(rays.reshape(-1, 6), p.tmin, p.tmax)
    hits = hits.reshape(h, w, spp)
    val = np.zeros((h, w, spp, 11), f32)
    normals = {}
    for y, x, s in zip(*np.nonzero(hits["prim"] != test_aov.MISS)):
        hit = hits[y, x, s]
        k = (int(hit["inst"]), int(hit["prim"]))
        if k not in normals:
            normals[k] = osc.shade_hit(hit)[1]
        val[y, x, s, 0:3] = faces[k[1], 0:3]
        val[y, x, s, 3:6] = normals[k]
        val[y, x, s, 6:9] = faces[k[1], 3:6]
        val[y, x, s, 9] = hit["t"]
        val[y, x, s, 10] = f32(1.0)
    acc = np.zeros((h, w, 11), f32)
    for s in range(spp):
        acc = acc + val[:, :, s]
    value = acc / f32(spp)
    if frame != 0:   # blended into zeroed planes: (value + 0 * frame) / (frame + 1)
        value = (value + np.zeros_like(value) * f32(frame)) / f32(frame + 1)
    return {"albedo": np.ascontiguousarray(value[:, :, 0:3]), "normal": np.ascontiguousarray(value[:, :, 3:6]),
            "emission": np.ascontiguousarray(value[:, :, 6:9]), "depth": np.ascontiguousarray(value[:, :, 9]),
            "alpha": np.ascontiguousarray(value[:, :, 10])}


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
def test_params_layout_defaults_and_symbols(pt, tmp_path):
    """sizeof / offsetof of pt_denoise_params by gcc from the header == the ctypes mirror; the defaults; the names in API_SYMBOLS."""
    src = tmp_path / "dn_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n",'
                   'sizeof(pt_denoise_params), offsetof(pt_denoise_params, iterations), offsetof(pt_denoise_params, sigma_normal),'
                   'offsetof(pt_denoise_params, sigma_depth), offsetof(pt_denoise_params, reserved), PT_API_VERSION);return 0;}\n')
    exe = tmp_path / "dn_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = pt.DenoiseParams
    assert got == [C.sizeof(P), P.iterations.offset, P.sigma_normal.offset, P.sigma_depth.offset, P.reserved.offset, 6], got
    assert got[0] == 32
    for name in ("pt_denoise_params_default", "pt_film_denoise", "pt_film_read_denoised"):
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    p = pt.denoise_default_params()   # (the library loads without a device: this call touches none)
    assert (p.iterations, p.sigma_normal, p.sigma_depth, list(p.reserved)) == (5, 0.5, f32(0.1), [0] * 5)


def test_bgra8_rule_is_the_films(orc):
    """_to_bgra8 == the oracle's display image after frame 0 of the same colour (raygen.rgen:88-90 with old = 0), alpha included."""
    rng = np.random.default_rng(3)
    img = rng.uniform(-0.2, 1.3, (9, 11, 3)).astype(f32)
    img[0, 0] = [0.0, 1.0, -0.0]
    img[0, 1] = [0.5 / 255.0, 1.5 / 255.0, 254.5 / 255.0]
    want = np.zeros((9, 11, 4), np.uint8)
    orc.accumulate_bgra8(want, img, 0)
    assert _to_bgra8(img).tobytes() == want.tobytes()


QUALITY = dict(scene="cornell", w=128, h=96, spp=4, ref_frames=64, ref_spp=32)


def test_quality_against_the_converged_render(pt, orc):
    """Cornell box 128 x 96, 4 spp, frame 0, against the mean of 64 frames of 32 spp (frames 1000..1063): the experiment the defaults
    come from, not cut (about 15 s of oracle time on 8 cores).  relMSE = mean((a - ref)^2 / (ref^2 + 0.01)).  Measured: noisy 1.7487,
    5 iterations 0.0384 (1 / 45.5), 4 iterations 0.0342, 1 iteration 0.2008 (1 / 8.7).  Asserted: 5 iterations <= noisy / 8, 1 iteration
    <= noisy / 3 -- margins for other seeds, not for a different filter."""
    q = QUALITY
    osc = test_aov._oracle_scene(pt, orc, q["scene"])
    noisy, _, _, _ = osc.render_frame(orc.default_params(frame=0, width=q["w"], height=q["h"], spp_per_frame=q["spp"]), nthreads=16)
    ref = np.zeros((q["h"], q["w"], 3), np.float64)
    for k in range(q["ref_frames"]):
        img, _, _, _ = osc.render_frame(orc.default_params(frame=1000 + k, width=q["w"], height=q["h"], spp_per_frame=q["ref_spp"]), nthreads=16)
        ref += img
    ref /= q["ref_frames"]
    g = _oracle_guides(pt, orc, q["scene"], q["w"], q["h"], q["spp"], 0)
    e_noisy = _rel_mse(noisy, ref)
    e = {n: _rel_mse(_denoise_ref(noisy, g, iterations=n)[0], ref) for n in (1, 4, 5)}
    print(f"relMSE noisy {e_noisy:.4f}; iterations 1 / 4 / 5: {e[1]:.4f} / {e[4]:.4f} / {e[5]:.4f}; ratios {e_noisy / e[1]:.1f} / {e_noisy / e[4]:.1f} / {e_noisy / e[5]:.1f}")
    assert e[5] <= e_noisy / 8, (e[5], e_noisy)
    assert e[1] <= e_noisy / 3, (e[1], e_noisy)


def _synthetic(h, w, seed, normal_step=None):
    """random radiance over guides of a full-coverage surface; normal_step: the right half's normal differs by that vector"""
    rng = np.random.default_rng(seed)
    g = {"albedo": rng.uniform(0.2, 0.9, (h, w, 3)).astype(f32), "normal": np.zeros((h, w, 3), f32), "emission": np.zeros((h, w, 3), f32),
         "depth": np.full((h, w), 3.0, f32), "alpha": np.ones((h, w), f32)}
    g["normal"][:, :, 2] = 1.0
    if normal_step is not None:
        g["normal"][:, w // 2:] = g["normal"][:, w // 2:] + np.asarray(normal_step, f32)
    film = rng.uniform(0.0, 2.0, (h, w, 3)).astype(f32)
    return film, g


def test_edge_stop_is_exact_and_uniform_guides_stay_in_range():
    """A normal step of |dn|^2 / sigma_n^2 = 16 between the halves: t = max(0, 1 - 16 / 16) = 0 exactly, so no tap crosses it and changing
    one half's radiance leaves the other half's output bytes unchanged.  With uniform guides and albedo 1 the output is a convex
    combination of the input: inside its range up to the rounding of the sums (the bound below is 64 ulp of the maximum)."""
    film, g = _synthetic(24, 40, 1, normal_step=(2.0, 0.0, 0.0))   # |dn|^2 = 4, sigma_n = 0.5: x_n = 16
    out_a, bgra_a = _denoise_ref(film, g, iterations=5)
    film_b = film.copy()
    film_b[:, 20:] = film_b[:, 20:] * f32(7.0) + f32(1.0)
    out_b, bgra_b = _denoise_ref(film_b, g, iterations=5)
    assert out_a[:, :20].tobytes() == out_b[:, :20].tobytes() and bgra_a[:, :20].tobytes() == bgra_b[:, :20].tobytes()
    assert not np.array_equal(out_a[:, 20:], out_b[:, 20:])
    assert not np.array_equal(out_a[:, :20], film[:, :20])                     # ... and the half itself is filtered
    film, g = _synthetic(24, 40, 2)
    g["albedo"][:] = 1.0
    out, _ = _denoise_ref(film, g, iterations=5)
    eps = f32(64.0) * np.spacing(film.max())
    for c in range(3):
        assert film[:, :, c].min() - eps <= out[:, :, c].min() and out[:, :, c].max() <= film[:, :, c].max() + eps
    assert out.std() < 0.25 * film.std()


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (40, 5)])
def test_borders_when_the_step_exceeds_the_image(shape):
    """1 x 1, 3 x 2 and 5 x 40 (width x height) with 8 iterations (steps up to 128): finite, and no division by zero or invalid operation."""
    h, w = shape
    film, g = _synthetic(h, w, 4)
    g["alpha"][0, 0] = 0.0   # a miss: D = albedo + 1, depth and normal 0
    g["depth"][0, 0] = 0.0
    g["normal"][0, 0] = 0.0
    with np.errstate(divide="raise", invalid="raise", over="raise"):
        out, bgra = _denoise_ref(film, g, iterations=8)
    assert out.shape == (h, w, 3) and np.isfinite(out).all() and bgra.shape == (h, w, 4)
    if shape == (1, 1):   # the centre tap alone: I * 9/64 / (9/64), remodulated
        D = _demod(g)
        I = (film - g["emission"]) / D
        w0 = H_TAPS[2] * H_TAPS[2]
        assert out.tobytes() == (((w0 * I) / w0) * D + g["emission"]).tobytes()


def test_reference_sees_denormal_weights():
    """The sweep the GPU parity test uploads (`_sweep_planes`) makes weights whose t^16 is denormal, and weights that underflow to 0."""
    film, g = _sweep_planes(64, 48)
    counts = {}
    _denoise_ref(film, g, iterations=3, counts=counts)
    assert counts["denormal"] > 100 and counts["underflow"] > 100, counts


def _sweep_planes(w, h):
    """Guides whose neighbouring normals differ so that t = 1 - x_n / 16 sweeps [0, 6e-3] finely: t^16 crosses the denormal range
    (t ~ 1.5e-3 .. 2.6e-3) and underflows below it.  Row y: normal.x alternates 0 / d(x, y) from pixel to pixel, with d^2 / sigma_n^2
    (sigma_n = 0.5) = 16 (1 - t)."""
    rng = np.random.default_rng(11)
    t = (np.arange(w * h, dtype=np.float64).reshape(h, w) + 0.5) / (w * h) * 6e-3
    d = np.sqrt(16.0 * (1.0 - t) * 0.25)
    g = {"albedo": rng.uniform(0.2, 0.9, (h, w, 3)).astype(f32), "normal": np.zeros((h, w, 3), f32),
         "emission": (rng.uniform(0, 1, (h, w, 3)) * (rng.uniform(0, 1, (h, w, 1)) < 0.1)).astype(f32),
         "depth": rng.uniform(2.9, 3.1, (h, w)).astype(f32), "alpha": np.ones((h, w), f32)}
    g["depth"][:] = 3.0
    g["normal"][:, 1::2, 0] = d[:, 1::2].astype(f32)
    g["normal"][:, :, 2] = 1.0
    film = rng.uniform(0.0, 2.0, (h, w, 3)).astype(f32)
    return film, g


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
# name -> (scene, width, height, spp, camera): the scenes and cameras of tests/test_aov.py
CASES = {
    "cornell": ("cornell", 48, 40, 4, {}),
    "cornell_odd": ("cornell", 52, 36, 4, {}),
    "cornell_77": ("cornell", 77, 53, 4, {}),
    "soup": ("soup", 48, 40, 4, test_aov.SOUP_CAM),
    "grid16": ("grid16", 48, 40, 4, test_aov.GRID_CAM),
    "one_pixel": ("cornell", 1, 1, 4, {}),
    "three_by_two": ("cornell", 3, 2, 4, {}),
}
# (iterations, sigma_normal, sigma_depth): fourteen combinations, every case runs all of them
COMBOS = [(1, 0.5, 0.1), (3, 0.5, 0.1), (5, 0.5, 0.1), (8, 0.5, 0.1), (1, 0.1, 0.02), (3, 0.1, 0.1), (5, 0.1, 0.02), (8, 0.1, 0.1),
          (1, 2.0, 0.1), (3, 2.0, 0.02), (5, 2.0, 0.1), (8, 2.0, 0.02), (5, 0.5, 0.02), (2, 0.5, 0.1)]
_scenes = {}


def _scene(pt, ctx, name):
    if name not in _scenes:
        _scenes[name] = test_aov._gpu_scene(pt, ctx, name)
    return _scenes[name]


def _read_inputs(film, pt):
    g = {n: film.read_aov(getattr(pt, "AOV_" + n.upper())) for n in GUIDES}
    return film.read_f32(), g


def _same(got_rgb, got_bgra, want, what):
    assert got_rgb.dtype == f32 and got_rgb.shape == want[0].shape, what
    assert got_rgb.tobytes() == want[0].tobytes(), (what, int((got_rgb != want[0]).sum()), float(np.abs(got_rgb - want[0]).max()))
    if got_bgra is not None:
        assert got_bgra.tobytes() == want[1].tobytes(), (what, int((got_bgra != want[1]).sum()))


def _rendered_film(pt, ctx, case, pipeline, n_frames, max_depth=4):
    scene, w, h, spp, cam = CASES[case]
    sc = _scene(pt, ctx, scene)
    film = pt.Film(ctx, w, h)
    film.enable_aov()
    kw = dict(width=w, height=h, spp_per_frame=spp, pipeline=pipeline, **cam)
    for k in range(n_frames):
        pt.render(sc, film, pt.default_params(frame=k, frame_count=1, max_depth=max_depth, **kw))
    pt.render_aov(sc, film, pt.default_params(frame=0, frame_count=n_frames, **kw))
    return film


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["WAVEFRONT", "AUTO"])
@pytest.mark.parametrize("n_frames", [1, 4])
@pytest.mark.parametrize("case", sorted(CASES))
def test_denoise_parity(pt, gpu_ctx, case, n_frames, pipeline):
    film = _rendered_film(pt, gpu_ctx, case, getattr(pt, "PIPELINE_" + pipeline), n_frames)
    try:
        rgb, g = _read_inputs(film, pt)
        assert g["alpha"].any() or case in ("one_pixel", "three_by_two")
        for it, sn, sz in COMBOS:
            ms = film.denoise(iterations=it, sigma_normal=sn, sigma_depth=sz)
            assert ms > 0
            _same(film.read_denoised(), film.read_denoised_bgra8(), _denoise_ref(rgb, g, it, sn, sz), (case, n_frames, pipeline, it, sn, sz))
    finally:
        film.close()


def _external_film(pt, ctx, torch, rgb, g):
    """a film over external radiance and external guide tensors holding the given arrays -> (film, the tensors that keep them alive)"""
    h, w = g["depth"].shape
    t_rgb = torch.from_numpy(np.ascontiguousarray(rgb)).to("cuda:0")
    film = pt.Film(ctx, w, h, device_ptr=t_rgb.data_ptr())
    planes = {n: torch.zeros(g[n].shape, dtype=torch.float32, device="cuda:0") for n in GUIDES}
    ids = torch.zeros((h, w, 2), dtype=torch.int32, device="cuda:0")
    ptrs = [None] * pt.AOV_COUNT
    for n in GUIDES:
        ptrs[getattr(pt, "AOV_" + n.upper())] = planes[n].data_ptr()
    ptrs[pt.AOV_ID] = ids.data_ptr()
    film.enable_aov(ptrs)                       # (zeroes the planes and the film is cleared at creation: fill them afterwards)
    t_rgb.copy_(torch.from_numpy(np.ascontiguousarray(rgb)))
    for n in GUIDES:
        planes[n].copy_(torch.from_numpy(np.ascontiguousarray(g[n])))
    torch.cuda.synchronize()
    return film, (t_rgb, planes, ids)


@pytest.mark.gpu
def test_denoise_denormal_weights_and_synthetic_planes(pt, gpu_ctx):
    """Planes made on the host (`_sweep_planes`: weights in and below the denormal range), in external tensors, at an odd size."""
    import torch
    film_np, g = _sweep_planes(77, 53)
    counts = {}
    want = _denoise_ref(film_np, g, 3, 0.5, 0.1, counts=counts)
    assert counts["denormal"] > 100 and counts["underflow"] > 100, counts
    film, keep = _external_film(pt, gpu_ctx, torch, film_np, g)
    try:
        rgb, g_dev = _read_inputs(film, pt)
        assert rgb.tobytes() == film_np.tobytes() and all(g_dev[n].tobytes() == g[n].tobytes() for n in GUIDES)
        film.denoise(iterations=3, sigma_normal=0.5, sigma_depth=0.1)
        _same(film.read_denoised(), film.read_denoised_bgra8(), want, "sweep, 3 iterations")
        film.denoise(iterations=8, sigma_normal=0.5, sigma_depth=0.1)
        _same(film.read_denoised(), film.read_denoised_bgra8(), _denoise_ref(film_np, g, 8, 0.5, 0.1), "sweep, 8 iterations")
    finally:
        film.close()
    del keep


@pytest.mark.gpu
def test_denoise_1080p_cornell_frame(pt, gpu_ctx, cornell_gpu):
    """One 1920 x 1080 Cornell frame, 32 spp, 5 iterations.  Variant used: three 256 x 256 crops (the full-frame numpy pass is about 125
    shifted-array passes with temporaries over 2 M pixels); each crop's reference is computed from inputs cropped with a 62-pixel halo
    (2 * (1 + 2 + 4 + 8 + 16) = 62: what five iterations can reach), clipped at the image's edge.  Crops: the top-left corner, the
    bottom-right corner, and one inside the box's projection."""
    w, h, spp = 1920, 1080, 32
    film = pt.Film(gpu_ctx, w, h)
    film.enable_aov()
    try:
        kw = dict(width=w, height=h, spp_per_frame=spp, frame=0, frame_count=1, pipeline=pt.PIPELINE_AUTO)
        pt.render(cornell_gpu, film, pt.default_params(max_depth=8, **kw))
        pt.render_aov(cornell_gpu, film, pt.default_params(**kw))
        rgb, g = _read_inputs(film, pt)
        film.denoise()
        got, got_bgra = film.read_denoised(), film.read_denoised_bgra8()
        for x0, y0 in ((0, 0), (w - 256, h - 256), (832, 412)):
            hx0, hy0, hx1, hy1 = max(0, x0 - 62), max(0, y0 - 62), min(w, x0 + 256 + 62), min(h, y0 + 256 + 62)
            sub = {n: np.ascontiguousarray(g[n][hy0:hy1, hx0:hx1]) for n in GUIDES}
            ref, ref_bgra = _denoise_ref(np.ascontiguousarray(rgb[hy0:hy1, hx0:hx1]), sub)
            ys, xs = slice(y0 - hy0, y0 - hy0 + 256), slice(x0 - hx0, x0 - hx0 + 256)
            _same(np.ascontiguousarray(got[y0:y0 + 256, x0:x0 + 256]), np.ascontiguousarray(got_bgra[y0:y0 + 256, x0:x0 + 256]),
                  (np.ascontiguousarray(ref[ys, xs]), np.ascontiguousarray(ref_bgra[ys, xs])), ("crop", x0, y0))
        assert g["alpha"][412:668, 832:1088].any() and not np.array_equal(got, rgb)
    finally:
        film.close()


@pytest.mark.gpu
def test_denoise_placement(pt, gpu_ctx):
    """device_out in a torch tensor == the film-owned plane; a film over external radiance and guide tensors == one that owns them."""
    import torch
    film = _rendered_film(pt, gpu_ctx, "cornell_odd", pt.PIPELINE_AUTO, 2)
    try:
        _, w, h, _, _ = CASES["cornell_odd"]
        rgb, g = _read_inputs(film, pt)
        film.denoise(iterations=4)
        own, own_bgra = film.read_denoised(), film.read_denoised_bgra8()
        _same(own, own_bgra, _denoise_ref(rgb, g, 4), "owned")
        out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
        film.denoise(iterations=4, device_out=out.data_ptr())
        assert out.cpu().numpy().tobytes() == own.tobytes()
        assert film.read_denoised().tobytes() == own.tobytes()                  # the film's own plane is not touched by that call
        ext, keep = _external_film(pt, gpu_ctx, torch, rgb, g)
        try:
            ext.denoise(iterations=4)
            _same(ext.read_denoised(), ext.read_denoised_bgra8(), (own, own_bgra), "external planes")
        finally:
            ext.close()
        del keep
    finally:
        film.close()


@pytest.mark.gpu
def test_denoise_moves_nothing_else(pt, gpu_ctx):
    """Film, bgra8, all six guide planes and pt_stats.rays / .paths are the same before and after; rendering frame 1 after a denoise
    == rendering frames 0..1 without one."""
    scene, w, h, spp, cam = CASES["cornell"]
    sc = _scene(pt, gpu_ctx, scene)
    film = _rendered_film(pt, gpu_ctx, "cornell", pt.PIPELINE_AUTO, 1)
    alone = _rendered_film(pt, gpu_ctx, "cornell", pt.PIPELINE_AUTO, 2)
    try:
        def state():
            st = gpu_ctx.stats()
            return ([film.read_f32().tobytes(), film.read_bgra8().tobytes()] + [film.read_aov(k).tobytes() for k in range(pt.AOV_COUNT)], (st.rays, st.paths, st.ms_total))
        before = state()
        film.denoise()
        film.denoise(iterations=2, sigma_normal=2.0)
        assert state() == before
        kw = dict(width=w, height=h, spp_per_frame=spp, pipeline=pt.PIPELINE_AUTO, **cam)
        pt.render(sc, film, pt.default_params(frame=1, frame_count=1, max_depth=4, **kw))
        assert film.read_f32().tobytes() == alone.read_f32().tobytes() and film.read_bgra8().tobytes() == alone.read_bgra8().tobytes()
    finally:
        film.close()
        alone.close()


@pytest.mark.gpu
def test_denoise_repeatability_and_memory(pt, cornell_arrays):
    """Two calls give the same bytes; free device memory is unchanged across the second and third call; a budget too small for the scratch
    is PT_ERR_OOM and the film renders on."""
    import torch
    w, h, spp = 160, 120, 4
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *cornell_arrays)
    kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=4, pipeline=pt.PIPELINE_AUTO)
    film, other, alone = pt.Film(ctx, w, h), pt.Film(ctx, w, h), pt.Film(ctx, w, h)
    try:
        for f in (film, other):
            f.enable_aov()
            pt.render(sc, f, pt.default_params(frame=0, frame_count=1, **kw))
            pt.render_aov(sc, f, pt.default_params(frame=0, frame_count=1, **kw))
        film.denoise()
        first = film.read_denoised().tobytes(), film.read_denoised_bgra8().tobytes()
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        film.denoise()
        film.denoise()
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
        assert free1 == free0, (free0, free1)
        assert (film.read_denoised().tobytes(), film.read_denoised_bgra8().tobytes()) == first
        # `other` has no scratch yet: 160 * 120 pixels * 48 B = 0.9 MB of scratch + 0.3 MB of output do not fit 1 MB
        old = ctx.set_tuning(mem_budget_mb=1)
        with pytest.raises(pt.PtError) as e:
            other.denoise()
        assert e.value.status == 4
        with pytest.raises(pt.PtError) as e:
            other.read_denoised()
        assert e.value.status == 1
        pt.render(sc, other, pt.default_params(frame=1, frame_count=1, **kw))      # the same shape again: nothing to allocate
        ctx.set_tuning(**old)
        pt.render(sc, alone, pt.default_params(frame=0, frame_count=2, **kw))
        assert other.read_f32().tobytes() == alone.read_f32().tobytes()
        other.denoise()                                                             # and with the budget back the call goes through
        rgb, g = _read_inputs(other, pt)
        _same(other.read_denoised(), other.read_denoised_bgra8(), _denoise_ref(rgb, g), "after the refusal")
    finally:
        for f in (film, other, alone):
            f.close()
        sc.close()
        ctx.close()


@pytest.mark.gpu
def test_denoise_errors(pt, gpu_ctx):
    """Every PT_ERR_INVALID_ARG case of the header."""
    lib = pt.lib_amd()
    film = pt.Film(gpu_ctx, 48, 40)

    def status(fn):
        with pytest.raises(pt.PtError) as e:
            fn()
        return e.value.status

    good = pt.denoise_default_params()
    assert lib.pt_film_denoise(None, C.byref(good), None, None) == 1               # NULL film
    assert lib.pt_film_denoise(film.h, None, None, None) == 1                       # NULL params
    assert lib.pt_film_read_denoised(None, None, None) == 1
    assert status(lambda: film.denoise()) == 1                                      # no guides
    film.enable_aov()
    assert status(lambda: film.read_denoised()) == 1                                # nothing denoised yet
    for it in (0, 9, 0xFFFFFFFF):
        assert status(lambda: film.denoise(iterations=it)) == 1
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        assert status(lambda: film.denoise(sigma_normal=bad)) == 1
        assert status(lambda: film.denoise(sigma_depth=bad)) == 1
    for k in range(5):
        p = pt.denoise_default_params()
        p.reserved[k] = 1
        assert status(lambda: film.denoise(params=p)) == 1
    assert status(lambda: film.read_denoised()) == 1                                # a refused call writes nothing
    out_only = np.zeros(48 * 40 * 3, f32)
    dev = pt.DeviceBuffer(gpu_ctx, out_only.nbytes)
    film.denoise(device_out=dev.ptr)                                                # into caller memory only ...
    assert status(lambda: film.read_denoised_bgra8()) == 1                          # ... the film still owns no result
    film.denoise()
    assert film.read_denoised().shape == (40, 48, 3)
    dev.close()
    film.close()


@pytest.mark.gpu
def test_pt_main_writes_the_denoised_image(pt, tmp_path):
    """pt_main --denoise N writes out.denoised.pfm / out.denoised.ppm beside --pfm out.pfm / --ppm out.ppm: the bytes of
    Film.read_denoised / read_denoised_bgra8 after the same render, guide pass and filter through the library; the normal outputs and
    the JSON line's figures are those of a run without --denoise; --ranks refuses it."""
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_main")
    if not os.path.exists(exe):
        pt.build()
    w, h = 48, 40
    base = [exe, "--obj", pt.ASSET_CORNELL, "--width", str(w), "--height", str(h), "--frames", "2", "--spp", "4", "--depth", "3"]
    plain = subprocess.run(base + ["--ppm", str(tmp_path / "a.ppm"), "--pfm", str(tmp_path / "a.pfm")], check=True, capture_output=True, text=True, cwd=pt.REPO)
    run = subprocess.run(base + ["--ppm", str(tmp_path / "b.ppm"), "--pfm", str(tmp_path / "b.pfm"), "--denoise", "3"], check=True, capture_output=True, text=True, cwd=pt.REPO)
    ja, jb = (json.loads(x.stdout.strip().splitlines()[-1]) for x in (plain, run))
    assert ja["rays"] == jb["rays"] and ja["paths"] == jb["paths"] == w * h * 4 * 2
    for ext in ("ppm", "pfm"):
        assert open(tmp_path / f"a.{ext}", "rb").read() == open(tmp_path / f"b.{ext}", "rb").read(), ext
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    raw = open(tmp_path / "b.denoised.pfm", "rb").read()
    assert raw.startswith(head)
    den = np.ascontiguousarray(np.frombuffer(raw[len(head):], f32).reshape(h, w, 3)[::-1])
    ppm_head = f"P6\n{w} {h}\n255\n".encode()
    ppm = open(tmp_path / "b.denoised.ppm", "rb").read()
    assert ppm.startswith(ppm_head) and len(ppm) == len(ppm_head) + w * h * 3
    bad = subprocess.run(base + ["--denoise", "--ranks", "2"], capture_output=True, text=True, cwd=pt.REPO)
    assert bad.returncode != 0 and "--denoise" in bad.stderr
    # the same through the library
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    film = pt.Film(ctx, w, h)
    film.enable_aov()
    kw = dict(width=w, height=h, spp_per_frame=4, frame=0, frame_count=2, pipeline=pt.PIPELINE_AUTO)
    pt.render(sc, film, pt.default_params(max_depth=3, **kw))
    pt.render_aov(sc, film, pt.default_params(**kw))
    film.denoise(iterations=3)
    assert den.tobytes() == film.read_denoised().tobytes()
    bgra = film.read_denoised_bgra8()
    assert ppm[len(ppm_head):] == np.ascontiguousarray(bgra[:, :, 2::-1]).tobytes()
    film.close(); sc.close(); ctx.close()
