"""pt_film_upsample: guide-driven upsampling of a low-resolution film (include/pt_api.h).

`_upsample_ref` is the numpy statement of the header's definition: float32 throughout, the sums written out, one gathered pass per tap in
the order j outer / i inner, a tap outside lo's image leaving the sums as they are.  The CPU tests check the exact properties of the
definition on synthetic planes, the kernel's per-pixel body compiled for the host (plain and under the host's sanitizers) and the value of
the call (the experiment of DESIGN.md section 18); the GPU tests feed `_upsample_ref` the planes read back from the device.  Every GPU
comparison is `tobytes()` equality, of the float image and of the bgra8 bytes."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_aov
import test_denoise
from test_denoise import GUIDES, TINY, _denoise_ref, _oracle_guides, _rel_mse, _same, _to_bgra8

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GPU_STEP_S = 120   # the time limit of a step that runs in a process of its own
FIRST, SECOND, NEAREST = 0, 1, 2
DEFAULT_SIGMAS = (1.0, 0.2)   # pt_upsample_params_default's sigma_normal, sigma_depth: the best of the grid of DESIGN.md section 18


def _axis(n, n_lo):
    """one axis of the mapping: -> (fx float32 [n], x0 int [n], bx float32 [n])"""
    s = f32(n_lo) / f32(n)
    fx = (np.arange(n, dtype=f32) + f32(0.5)) * s - f32(0.5)
    x0f = np.floor(fx)
    assert fx.dtype == f32 and x0f.dtype == f32
    return fx, x0f.astype(np.int64), fx - x0f


def _upsample_ref(src, g_lo, g, sigma_normal=DEFAULT_SIGMAS[0], sigma_depth=DEFAULT_SIGMAS[1], parts=None, rows=None):
    """-> (rgb float32 [H, W, 3], bgra uint8 [H, W, 4]).  src [H', W', 3]: the plane `source` names (lo's film or its denoised result); g_lo,
    g: {albedo, normal, emission [.., 3]; depth, alpha} of lo and of the full-size film as stored.
    parts (a dict): receives path [H, W] (FIRST / SECOND / NEAREST), x0, bx (per column), y0, by (per row), I_lo, I, and the number of
    first-ring tap weights that are denormal / zero although t > 0 before the squarings.
    rows (ya, yb): only those full-size rows are computed and returned (a pixel depends on no other full-size pixel)."""
    S_ = np.ascontiguousarray(src, f32)
    A1, N1, E1, Z1, a1 = (np.ascontiguousarray(g_lo[k], f32) for k in GUIDES)
    ya, yb = rows if rows is not None else (0, g["depth"].shape[0])
    fy, y0, by = (v[ya:yb] for v in _axis(g["depth"].shape[0], Z1.shape[0]))
    A, N, E, Z, al = (np.ascontiguousarray(g[k][ya:yb], f32) for k in GUIDES)
    assert all(a.dtype == f32 for a in (S_, A1, N1, E1, Z1, a1, A, N, E, Z, al))
    h, w = Z.shape
    lh, lw = Z1.shape
    one = f32(1.0)
    I1 = (S_ - E1) / np.maximum(A1 + (one - a1)[:, :, None], f32(0.001))
    D = np.maximum(A + (one - al)[:, :, None], f32(0.001))
    inv_n = one / (f32(sigma_normal) * f32(sigma_normal))
    sz2 = f32(sigma_depth) * f32(sigma_depth)
    fx, x0, bx = _axis(w, lw)
    X0, Y0 = np.broadcast_to(x0[None, :], (h, w)), np.broadcast_to(y0[:, None], (h, w))
    n_denormal = n_underflow = 0

    def tap(i, j):
        """-> (inside lo's image [H, W], t [H, W], I'(q) [H, W, 3]) of the tap q = (x0 + i, y0 + j); outside: the clamped pixel's values"""
        qx, qy = X0 + i, Y0 + j
        ok = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh)
        qxc, qyc = np.clip(qx, 0, lw - 1), np.clip(qy, 0, lh - 1)
        dn = N - N1[qyc, qxc]
        x_n = ((dn[:, :, 0] * dn[:, :, 0] + dn[:, :, 1] * dn[:, :, 1]) + dn[:, :, 2] * dn[:, :, 2]) * inv_n
        Zq = Z1[qyc, qxc]
        dz = Z - Zq
        x_z = (dz * dz) / (sz2 * (Z * Z + Zq * Zq) + f32(1e-12))
        t = np.maximum(f32(0.0), one - (x_n + x_z) * f32(0.0625))
        t0 = t
        for _ in range(4):
            t = t * t
        assert t.dtype == f32
        return ok, t, t0, I1[qyc, qxc]

    with np.errstate(all="ignore"):   # (0 / 0 where den is 0: the value is dropped by the select)
        num = np.zeros((h, w, 3), f32)
        den = np.zeros((h, w), f32)
        for j in (0, 1):
            for i in (0, 1):
                ok, t, t0, Iq = tap(i, j)
                wq = (bx if i else one - bx)[None, :] * (by if j else one - by)[:, None]
                wt = wq * t
                assert wt.dtype == f32
                n_denormal += int((ok & (wt > 0) & (wt < TINY)).sum())
                n_underflow += int((ok & (wt == 0) & (t0 > 0) & (wq > 0)).sum())
                num = np.where(ok[:, :, None], num + wt[:, :, None] * Iq, num)
                den = np.where(ok, den + wt, den)
        first = den >= f32(0.01)
        Ia = num / den[:, :, None]
        num = np.zeros((h, w, 3), f32)
        den = np.zeros((h, w), f32)
        for j in range(-1, 3):
            for i in range(-1, 3):
                ok, t, t0, Iq = tap(i, j)
                num = np.where(ok[:, :, None], num + t[:, :, None] * Iq, num)
                den = np.where(ok, den + t, den)
        second = den >= f32(0.01)
        Ib = num / den[:, :, None]
        assert Ia.dtype == f32 and Ib.dtype == f32
    nx = np.clip(np.floor(fx + f32(0.5)).astype(np.int64), 0, lw - 1)
    ny = np.clip(np.floor(fy + f32(0.5)).astype(np.int64), 0, lh - 1)
    Ic = I1[ny[:, None], nx[None, :]]
    I = np.where(first[:, :, None], Ia, np.where(second[:, :, None], Ib, Ic))
    out = I * D + E
    assert out.dtype == f32
    if parts is not None:
        parts.update(path=np.where(first, FIRST, np.where(second, SECOND, NEAREST)), x0=x0, bx=bx, y0=y0, by=by, I_lo=I1, I=I,
                     denormal=n_denormal, underflow=n_underflow)
    return out, _to_bgra8(out)


def _shares(path):
    return [float((path == k).mean()) for k in (FIRST, SECOND, NEAREST)]


def _bilinear_resize(src, h, w):
    """the plain resize a caller without the pass would do: the same pixel-centre mapping, the four taps by their bilinear weights alone,
    renormalised over the taps inside the image (float64)"""
    lh, lw = src.shape[:2]
    _, x0, bx = _axis(w, lw)
    _, y0, by = _axis(h, lh)
    num = np.zeros((h, w, 3), np.float64)
    den = np.zeros((h, w), np.float64)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0[None, :] + i, y0[:, None] + j
            ok = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh)
            wq = ((bx if i else 1 - bx).astype(np.float64)[None, :] * (by if j else 1 - by).astype(np.float64)[:, None]) * ok
            num += wq[:, :, None] * src[np.clip(qy, 0, lh - 1), np.clip(qx, 0, lw - 1)].astype(np.float64)
            den += wq
    return num / den[:, :, None]


# ---- synthetic planes -----------------------------------------------------------------------------------------------------------------
def _layer_guides(layer, rng, tilt=0.3, partial=False):
    """guides of a surface whose pixel (y, x) lies on depth layer `layer[y, x]` (Z = 8^layer: between two layers x_z >= 18.8 and
    t = 0 exactly at a sigma_depth up to 0.2; a miss against any layer has x_z = 25), with a normal that varies inside [0, tilt] in x so that t takes values below 1 on one layer; emission in a tenth of
    the pixels; layer -1: a miss (all guides 0); partial: coverage 0.25 / 0.5 / 0.75 in a tenth of the hits (the planes are premultiplied)"""
    h, w = layer.shape
    hit = layer >= 0
    a = hit.astype(f32)
    if partial:
        part = hit & (rng.uniform(0, 1, (h, w)) < 0.1)
        a[part] = rng.choice(np.asarray([0.25, 0.5, 0.75], f32), int(part.sum()))
    nrm = np.zeros((h, w, 3), f32)
    nrm[:, :, 2] = 1.0
    nrm[:, :, 0] = rng.uniform(0.0, tilt, (h, w))
    depth = np.exp2(3 * np.maximum(layer, 0)).astype(f32)
    return {"albedo": (rng.uniform(0.2, 0.9, (h, w, 3)).astype(f32) * a[:, :, None]).astype(f32), "normal": (nrm * a[:, :, None]).astype(f32),
            "emission": ((rng.uniform(0, 1, (h, w, 3)) * (rng.uniform(0, 1, (h, w, 1)) < 0.1)).astype(f32) * hit[:, :, None]).astype(f32),
            "depth": (depth * a).astype(f32), "alpha": a}


def _random_layers(h, w, lh, lw, seed, n_layers=12):
    """both films on random depth layers, pixel by pixel, a twentieth of the pixels a miss: every path is taken by a good share of the pixels"""
    rng = np.random.default_rng(seed)
    layers = [np.where(rng.uniform(0, 1, s) < 0.05, -1, rng.integers(0, n_layers, s)) for s in ((h, w), (lh, lw))]
    g, g_lo = _layer_guides(layers[0], rng, partial=True), _layer_guides(layers[1], rng, partial=True)
    return rng.uniform(0.0, 2.0, (lh, lw, 3)).astype(f32), g_lo, g


def _wave_cliffs(h, w, lh, lw, seed):
    """Depth cliffs arranged by wave (one row's 64 consecutive full-size pixels; the last wave of a row is partial).  lo lies on layer 0 but
    for a sparse set of layer-1 pixels.  A full-size wave is of kind 0 (all on layer 0), kind 1 (one lane on layer 2, which exists nowhere
    in lo: that lane ends at NEAREST), kind 2 (all of its lanes on layers 2 and 3: all of them fall back) or kind 3 (a random mix of layers 0
    and 1: some lanes find their layer in the second ring)."""
    rng = np.random.default_rng(seed)
    lo_layer = np.where(rng.uniform(0, 1, (lh, lw)) < 0.15, 1, 0)
    layer = np.zeros((h, w), np.int64)
    for y in range(h):
        for xa in range(0, w, 64):
            xb = min(xa + 64, w)
            kind = (y + xa // 64) % 4
            if kind == 1:
                layer[y, rng.integers(xa, xb)] = 2
            elif kind == 2:
                layer[y, xa:xb] = rng.integers(2, 4, xb - xa)
            elif kind == 3:
                layer[y, xa:xb] = rng.integers(0, 2, xb - xa)
    g, g_lo = _layer_guides(layer, rng, tilt=0.1), _layer_guides(lo_layer, rng, tilt=0.1)
    return rng.uniform(0.0, 2.0, (lh, lw, 3)).astype(f32), g_lo, g


def _wave_kinds(path, w):
    """-> ({lanes that fell back, per full wave}, {the same per partial wave})"""
    fb = path != FIRST
    full, partial = set(), set()
    for y in range(path.shape[0]):
        for xa in range(0, w, 64):
            (full if xa + 64 <= w else partial).add(int(fb[y, xa:xa + 64].sum()))
    return full, partial


def _sweep_planes(h, w, lh, lw):
    """Guides whose t^16 crosses the denormal range and underflows (test_denoise._sweep_planes' recipe): the full-size normal is (0, 0, 1);
    lo's normal.x is 0 in the column pairs {0, 1}, {4, 5}, ... and d(q) in the others, with d^2 / sigma_n^2 = 16 (1 - t) at the default
    sigma_normal and t sweeping [0, 6e-3] over lo's pixels.  One depth everywhere."""
    rng = np.random.default_rng(11)
    t = (np.arange(lw * lh, dtype=np.float64).reshape(lh, lw) + 0.5) / (lw * lh) * 6e-3
    d = np.sqrt(16.0 * (1.0 - t) * DEFAULT_SIGMAS[0] ** 2)

    def flat(hh, ww):
        gg = {"albedo": rng.uniform(0.2, 0.9, (hh, ww, 3)).astype(f32), "normal": np.zeros((hh, ww, 3), f32),
              "emission": (rng.uniform(0, 1, (hh, ww, 3)) * (rng.uniform(0, 1, (hh, ww, 1)) < 0.1)).astype(f32),
              "depth": np.full((hh, ww), 3.0, f32), "alpha": np.ones((hh, ww), f32)}
        gg["normal"][:, :, 2] = 1.0
        return gg
    g, g_lo = flat(h, w), flat(lh, lw)
    swept = (np.arange(lw) // 2) % 2 == 1
    g_lo["normal"][:, swept, 0] = d[:, swept].astype(f32)
    src = rng.uniform(0.0, 2.0, (lh, lw, 3)).astype(f32)
    return src, g_lo, g


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
FIELDS = ["sigma_normal", "sigma_depth", "source", "reserved"]
NEW_SYMBOLS = ["pt_upsample_params_default", "pt_film_upsample", "pt_film_read_upsampled"]


def test_upsample_params_layout_defaults_and_symbols(pt, tmp_path):
    """sizeof / offsetof of pt_upsample_params by gcc from the header == the ctypes mirror (32 bytes); the source values; the defaults; the
    three new names in API_SYMBOLS and in the library; PT_API_VERSION stays 6."""
    src = tmp_path / "up_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("%zu ' + "%zu " * len(FIELDS) + '%d %d %d\\n",'
                   "sizeof(pt_upsample_params), " + ", ".join(f"offsetof(pt_upsample_params, {n})" for n in FIELDS) +
                   ", PT_UPSAMPLE_SRC_FILM, PT_UPSAMPLE_SRC_DENOISED, PT_API_VERSION);return 0;}\n")
    exe = tmp_path / "up_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = pt.UpsampleParams
    assert got == [C.sizeof(P)] + [getattr(P, n).offset for n in FIELDS] + [pt.UPSAMPLE_SRC_FILM, pt.UPSAMPLE_SRC_DENOISED, 6], got
    assert got[0] == 32 and got[1:5] == [0, 4, 8, 12]
    for name in NEW_SYMBOLS:
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    p = pt.upsample_default_params()   # (touches no device)
    assert (p.sigma_normal, p.sigma_depth, p.source, list(p.reserved)) == (f32(DEFAULT_SIGMAS[0]), f32(DEFAULT_SIGMAS[1]), pt.UPSAMPLE_SRC_FILM, [0] * 5)
    lib = pt.lib_amd()
    lib.pt_upsample_params_default(None)                                     # (a NULL is ignored)
    assert lib.pt_film_upsample(None, None, C.byref(p), None, None) == 1 and lib.pt_film_read_upsampled(None, None, None) == 1


def _uniform_guides(h, w, rng):
    g = {"albedo": rng.uniform(0.2, 0.9, (h, w, 3)).astype(f32), "normal": np.zeros((h, w, 3), f32), "emission": rng.uniform(0, 0.5, (h, w, 3)).astype(f32),
         "depth": np.full((h, w), 3.0, f32), "alpha": np.ones((h, w), f32)}
    g["normal"][:, :, 2] = 1.0
    return g


@pytest.mark.parametrize("shape", [((6, 8), (3, 4)), ((5, 13), (2, 4)), ((2, 3), (1, 1)), ((7, 9), (7, 5))])
def test_identical_guides_give_the_renormalised_bilinear_interpolation(shape):
    """Normal and depth the same everywhere in both films: every t is 1 exactly, so I is sum wq I'(q) / sum wq over the taps inside lo's
    image -- computed here by a per-pixel loop of binary32 scalars -- and every pixel takes the first ring."""
    (h, w), (lh, lw) = shape
    rng = np.random.default_rng(5)
    g, g_lo = _uniform_guides(h, w, rng), _uniform_guides(lh, lw, rng)
    src = rng.uniform(0.0, 2.0, (lh, lw, 3)).astype(f32)
    parts = {}
    out, _ = _upsample_ref(src, g_lo, g, parts=parts)
    assert (parts["path"] == FIRST).all()
    I1 = (src - g_lo["emission"]) / np.maximum(g_lo["albedo"] + f32(0.0), f32(0.001))
    sx, sy = f32(lw) / f32(w), f32(lh) / f32(h)
    want = np.zeros((h, w, 3), f32)
    for y in range(h):
        for x in range(w):
            fx, fy = (f32(x) + f32(0.5)) * sx - f32(0.5), (f32(y) + f32(0.5)) * sy - f32(0.5)
            x0, y0 = int(np.floor(fx)), int(np.floor(fy))
            bx, by = fx - f32(x0), fy - f32(y0)
            num, den = np.zeros(3, f32), f32(0.0)
            for j in (0, 1):
                for i in (0, 1):
                    if 0 <= x0 + i < lw and 0 <= y0 + j < lh:
                        wq = (bx if i else f32(1.0) - bx) * (by if j else f32(1.0) - by)
                        num = num + wq * I1[y0 + j, x0 + i]
                        den = den + wq
            want[y, x] = num / den
    assert parts["I"].dtype == f32 and parts["I"].tobytes() == want.tobytes()
    assert out.tobytes() == (want * np.maximum(g["albedo"] + f32(0.0), f32(0.001)) + g["emission"]).tobytes()


def test_same_size_is_the_identity_on_the_illumination():
    """w' = w, h' = h and lo's normal and depth equal to the full-size ones: fx = x, bx = 0, the tap (0, 0) weighs 1 and I == I' (so
    out == (S' - E') / D' * D + E, and == S' where the albedo and emission planes agree too)."""
    h, w = 9, 11
    src, g_lo, g = _random_layers(h, w, h, w, 3)
    for k in ("normal", "depth"):
        g_lo[k] = g[k].copy()
    parts = {}
    out, _ = _upsample_ref(src, g_lo, g, parts=parts)
    assert not parts["bx"].any() and not parts["by"].any() and (parts["x0"] == np.arange(w)).all() and (parts["path"] == FIRST).all()
    assert np.array_equal(parts["I"], parts["I_lo"])
    g_same = {k: g[k].copy() for k in GUIDES}
    out, _ = _upsample_ref(src, g_same, g)
    D = np.maximum(g["albedo"] + (f32(1.0) - g["alpha"])[:, :, None], f32(0.001))
    assert np.array_equal(out, ((src - g["emission"]) / D) * D + g["emission"])


def test_half_size_weights_are_quarters():
    """w' = w / 2: bx alternates 0.75, 0.25 exactly (x even: x0 = x / 2 - 1; x odd: x0 = (x - 1) / 2), so the four weights are products of
    {0.25, 0.75}; the first column and row have x0 = -1 and the last ones x0 + 1 = w'."""
    for n in (2, 6, 64, 130, 1920):
        _, x0, bx = _axis(n, n // 2)
        assert (bx[0::2] == f32(0.75)).all() and (bx[1::2] == f32(0.25)).all()
        assert (x0[0::2] == np.arange(n // 2) - 1).all() and (x0[1::2] == np.arange(n // 2)).all()
        assert x0[0] == -1 and x0[-1] + 1 == n // 2
    for n, n_lo in ((130, 43), (5, 2), (3, 1), (1080, 360), (77, 76)):     # any ratio: x0 stays in [-1, w' - 1]
        _, x0, bx = _axis(n, n_lo)
        assert x0.min() >= -1 and x0.max() <= n_lo - 1 and (bx >= 0).all() and (bx < 1).all()


def test_the_three_paths_are_each_taken():
    """Random depth layers (Z = 2^k: t = 0 exactly between layers) in both films: a pixel whose layer is on none of its four taps goes to the
    second ring, one whose layer is on none of the sixteen to NEAREST.  The shares are printed and each is > 0; every value is finite; a
    first-ring pixel's I lies inside the range of its layer's taps."""
    h, w, lh, lw = 40, 70, 20, 35
    src, g_lo, g = _random_layers(h, w, lh, lw, 7)
    parts = {}
    out, bgra = _upsample_ref(src, g_lo, g, parts=parts)
    sh = _shares(parts["path"])
    print(f"shares: first ring {sh[0]:.3f}, second ring {sh[1]:.3f}, nearest {sh[2]:.3f}")
    assert all(s > 0.05 for s in sh), sh
    assert np.isfinite(out).all() and bgra.shape == (h, w, 4)
    I1 = parts["I_lo"]
    assert (parts["I"].min(axis=(0, 1)) >= I1.min(axis=(0, 1)) - f32(1e-4)).all() and (parts["I"].max(axis=(0, 1)) <= I1.max(axis=(0, 1)) + f32(1e-4)).all()
    # NEAREST is the nearest lo pixel's I' itself
    ny, nx = np.nonzero(parts["path"] == NEAREST)
    qx = np.clip(np.floor((nx.astype(f32) + f32(0.5)) * (f32(lw) / f32(w)) - f32(0.5) + f32(0.5)).astype(int), 0, lw - 1)
    qy = np.clip(np.floor((ny.astype(f32) + f32(0.5)) * (f32(lh) / f32(h)) - f32(0.5) + f32(0.5)).astype(int), 0, lh - 1)
    assert np.array_equal(parts["I"][ny, nx], I1[qy, qx])
    # the waves of the GPU test: none, exactly one and all 64 lanes fall back; and the sweep makes denormal weights
    src, g_lo, g = _wave_cliffs(9, 130, 4, 43, 2)
    _upsample_ref(src, g_lo, g, parts=parts)
    full, partial = _wave_kinds(parts["path"], 130)
    assert {0, 1, 64} <= full and {0, 2} <= partial and (parts["path"] == NEAREST).any() and (parts["path"] == SECOND).any(), (full, partial)
    src, g_lo, g = _sweep_planes(53, 77, 26, 38)
    _upsample_ref(src, g_lo, g, parts=parts)
    assert parts["denormal"] > 100 and parts["underflow"] > 100, (parts["denormal"], parts["underflow"])
    assert all(s > 0 for s in _shares(parts["path"])[:2])


HOST_CASES = [("layers", (40, 70), (20, 35)), ("layers", (5, 130), (2, 43)), ("layers", (6, 70), (3, 35)), ("layers", (4, 64), (4, 64)),
              ("layers", (2, 3), (1, 1)), ("waves", (9, 130), (4, 43)), ("sweep", (53, 77), (26, 38)), ("layers", (31, 23), (30, 7))]


def _case_planes(kind, hw, lhw, seed=1):
    (h, w), (lh, lw) = hw, lhw
    if kind == "layers":
        return _random_layers(h, w, lh, lw, seed + h)
    if kind == "waves":
        return _wave_cliffs(h, w, lh, lw, seed)
    return _sweep_planes(h, w, lh, lw)


def _run_on_host(exe, d, src, g_lo, g, sigma_normal=DEFAULT_SIGMAS[0], sigma_depth=DEFAULT_SIGMAS[1]):
    """the kernel's body compiled for the host (tests/upsample_host.cpp) over the given planes -> (rgb [H, W, 3], bgra [H, W, 4])"""
    os.makedirs(d, exist_ok=True)
    h, w = g["depth"].shape
    lh, lw = g_lo["depth"].shape
    np.asarray([w, h, lw, lh, sigma_normal, sigma_depth, 0, 0], f32).tofile(os.path.join(d, "par"))
    np.ascontiguousarray(src, f32).tofile(os.path.join(d, "lo_src"))
    for n in GUIDES:
        np.ascontiguousarray(g[n], f32).tofile(os.path.join(d, n))
        np.ascontiguousarray(g_lo[n], f32).tofile(os.path.join(d, "lo_" + n))
    subprocess.check_call([exe, d])
    return np.fromfile(os.path.join(d, "o_rgb"), f32).reshape(h, w, 3), np.fromfile(os.path.join(d, "o_bgra"), np.uint8).reshape(h, w, 4)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_kernel_body_on_the_host_equals_the_reference(tmp_path, sanitize):
    """csrc/upsample_kernel.h -- the statements k_upsample runs per pixel -- compiled by g++ as a stand-alone program (-ffp-contract=off, the
    IEEE divide for pt_math.h's fdiv) gives the bytes of `_upsample_ref`: the shapes of the GPU tests, the three paths, the waves, the
    denormal sweep, a second parameter set.  The second build runs the same cases under AddressSanitizer and UBSan: every tap address is
    inside its plane."""
    exe = str(tmp_path / "upsample_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "upsample_host.cpp")])
    n_path = np.zeros(3, np.int64)
    for k, (kind, hw, lhw) in enumerate(HOST_CASES):
        src, g_lo, g = _case_planes(kind, hw, lhw)
        for kw in (dict(), dict(sigma_normal=2.0, sigma_depth=0.02)):
            parts = {}
            want = _upsample_ref(src, g_lo, g, parts=parts, **kw)
            rgb, bgra = _run_on_host(exe, str(tmp_path / f"c{k}_{len(kw)}"), src, g_lo, g, **kw)
            _same(rgb, bgra, want, (kind, hw, lhw, kw))
            n_path += np.bincount(parts["path"].reshape(-1), minlength=3)
    assert (n_path > 1000).all(), n_path


QUALITY = dict(scene="cornell", w=128, h=96, lw=64, lh=48, lo_spp=16, spp=4, ref_frames=64, ref_spp=32)
_quality_cache = {}


def _quality_inputs(pt, orc):
    """lo at 16 spp x 1 frame (the ray budget of the full size at 4 spp), the full-size film at 4 spp, both films' guides at frame 0, and the
    reference: the mean of 64 frames of 32 spp (frames 1000..1063), test_denoise's -- 2048 spp against 16: the reference's own relative MSE
    is about 1 / 128 of the 16-spp film's: the full-size 4-spp film measures 1.75 and 4 / 2048 of that is 0.0034, 2 % of the smaller figure
    of the asserted pair (0.17 against 0.73) and 9 % of the smallest figure printed (0.039)."""
    if not _quality_cache:
        q = QUALITY
        osc = test_aov._oracle_scene(pt, orc, q["scene"])
        lo = osc.render_frame(orc.default_params(frame=0, width=q["lw"], height=q["lh"], spp_per_frame=q["lo_spp"]), nthreads=16)[0]
        full = osc.render_frame(orc.default_params(frame=0, width=q["w"], height=q["h"], spp_per_frame=q["spp"]), nthreads=16)[0]
        ref = np.zeros((q["h"], q["w"], 3), np.float64)
        for k in range(q["ref_frames"]):
            ref += osc.render_frame(orc.default_params(frame=1000 + k, width=q["w"], height=q["h"], spp_per_frame=q["ref_spp"]), nthreads=16)[0]
        ref /= q["ref_frames"]
        _quality_cache.update(lo=lo, full=full, ref=ref, g_lo=_oracle_guides(pt, orc, q["scene"], q["lw"], q["lh"], q["lo_spp"], 0),
                              g=_oracle_guides(pt, orc, q["scene"], q["w"], q["h"], q["spp"], 0))
    return _quality_cache


def test_quality_against_the_converged_render(pt, orc):
    """The experiment of DESIGN.md section 18 on the oracle's Cornell box: full size 128 x 96, lo 64 x 48 at 16 spp x 1 frame.  relMSE =
    test_denoise._rel_mse against the converged reference (see _quality_inputs for its sample count).  Asserted: the guided upsample of lo's
    film is better than the plain bilinear resize of the same film.  Printed, without a threshold: that pair, the same pair with lo denoised
    first (SRC_DENOISED), and the full-size film at 4 spp raw and after pt_film_denoise.  Measured at the defaults (1.0, 0.2):
        lo 16 spp: bilinear resize 0.7275, guided upsample 0.1719 (ratio 4.23)
        lo 16 spp denoised (5 iterations): bilinear resize 0.6024, guided upsample 0.0393 (ratio 15.3)
        full size 4 spp: raw 1.7487, pt_film_denoise 0.0384
    (the plain resize smears the lamp's emission over its dark surround, which the relative measure punishes; the guided pass takes
    emission and albedo from the full-size planes)"""
    q = _quality_inputs(pt, orc)
    h, w = QUALITY["h"], QUALITY["w"]
    ref = q["ref"]
    e_bil = _rel_mse(_bilinear_resize(q["lo"], h, w), ref)
    e_up = _rel_mse(_upsample_ref(q["lo"], q["g_lo"], q["g"], *DEFAULT_SIGMAS)[0], ref)
    lo_dn = _denoise_ref(q["lo"], q["g_lo"])[0]
    e_bil_dn = _rel_mse(_bilinear_resize(lo_dn, h, w), ref)
    e_up_dn = _rel_mse(_upsample_ref(lo_dn, q["g_lo"], q["g"], *DEFAULT_SIGMAS)[0], ref)
    e_full, e_full_dn = _rel_mse(q["full"], ref), _rel_mse(_denoise_ref(q["full"], q["g"])[0], ref)
    print(f"lo 16 spp: bilinear resize {e_bil:.4f}, guided upsample {e_up:.4f} (ratio {e_bil / e_up:.2f})")
    print(f"lo 16 spp denoised: bilinear resize {e_bil_dn:.4f}, guided upsample {e_up_dn:.4f} (ratio {e_bil_dn / e_up_dn:.2f})")
    print(f"full size 4 spp: raw {e_full:.4f}, pt_film_denoise {e_full_dn:.4f}")
    assert e_up < e_bil, (e_up, e_bil)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
_scene = test_denoise._scene
SHAPES = [((128, 96), (64, 48)), ((130, 5), (43, 2)), ((70, 6), (35, 3)), ((64, 4), (64, 4)), ((3, 2), (1, 1))]   # (w, h) <- (w', h')


def _guides_of(film, pt):
    return {n: film.read_aov(getattr(pt, "AOV_" + n.upper())) for n in GUIDES}


def _rendered_pair(pt, ctx, sc, wh, lwh, pipeline, spp=4, max_depth=4, lo_frames=2, lo_pipeline=None):
    """-> (film, lo): the full-size film with its guides alone, lo with `lo_frames` frames of radiance and its guides, at the default camera"""
    (w, h), (lw, lh) = wh, lwh
    film, lo = pt.Film(ctx, w, h), pt.Film(ctx, lw, lh)
    film.enable_aov()
    lo.enable_aov()
    kw = dict(spp_per_frame=spp, frame=0, frame_count=lo_frames)
    lo_kw = dict(width=lw, height=lh, pipeline=pipeline if lo_pipeline is None else lo_pipeline, **kw)
    pt.render(sc, lo, pt.default_params(max_depth=max_depth, **lo_kw))
    pt.render_aov(sc, lo, pt.default_params(**lo_kw))
    pt.render_aov(sc, film, pt.default_params(width=w, height=h, pipeline=pipeline, **kw))
    return film, lo


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["WAVEFRONT", "AUTO"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}_from_{s[1][0]}x{s[1][1]}")
def test_upsample_rendered_chains(pt, gpu_ctx, shape, pipeline):
    """The Cornell box: lo rendered (two frames) with its guides, the full-size guides, then the call from lo's film and -- after a
    pt_film_denoise of lo -- from its denoised plane, at the defaults and at a second pair of sigmas, against the reference fed with the
    planes read back from the two films."""
    film, lo = _rendered_pair(pt, gpu_ctx, _scene(pt, gpu_ctx, "cornell"), shape[0], shape[1], getattr(pt, "PIPELINE_" + pipeline))
    try:
        g, g_lo, c_lo = _guides_of(film, pt), _guides_of(lo, pt), lo.read_f32()
        assert g["alpha"].any() or shape[0] == (3, 2)
        for kw in (dict(), dict(sigma_normal=2.0, sigma_depth=0.02)):
            ms = film.upsample(lo, **kw)
            assert ms > 0
            _same(film.read_upsampled(), film.read_upsampled_bgra8(), _upsample_ref(c_lo, g_lo, g, **kw), (shape, pipeline, "film", kw))
        lo.denoise(iterations=3)
        d_lo = lo.read_denoised()
        assert not np.array_equal(d_lo, c_lo) or shape[1] == (1, 1)
        for kw in (dict(), dict(sigma_normal=0.25, sigma_depth=0.2)):
            film.upsample(lo, source=pt.UPSAMPLE_SRC_DENOISED, **kw)
            _same(film.read_upsampled(), film.read_upsampled_bgra8(), _upsample_ref(d_lo, g_lo, g, **kw), (shape, pipeline, "denoised", kw))
        assert lo.read_denoised().tobytes() == d_lo.tobytes() and lo.read_f32().tobytes() == c_lo.tobytes()
    finally:
        film.close(); lo.close()


def _external_pair(pt, ctx, torch, src, g_lo, g):
    """two films over external tensors holding the given planes (the full-size film's radiance: zeros) -> (film, lo, what keeps them alive)"""
    h, w = g["depth"].shape
    film, keep = test_denoise._external_film(pt, ctx, torch, np.zeros((h, w, 3), f32), g)
    lo, keep_lo = test_denoise._external_film(pt, ctx, torch, src, g_lo)
    return film, lo, (keep, keep_lo)


SYNTHETIC = [("waves", (9, 130), (4, 43)), ("layers", (40, 70), (20, 35)), ("sweep", (53, 77), (26, 38)), ("layers", (31, 23), (30, 7)), ("layers", (2, 3), (1, 1))]


@pytest.mark.gpu
def test_upsample_synthetic_planes(pt, gpu_ctx):
    """Planes made on the host in external tensors; the restatement's path shares are asserted on each before the comparison.  130 x 9 from
    43 x 4 with depth cliffs by wave: waves in which no lane falls back, exactly one does, all 64 do (and the partial third wave), so both
    sides of k_upsample's vote and the select that keeps a first-ring result are hit; pixels that reach NEAREST; 77 x 53 whose t^16
    underflows into denormals and to zero; taps at x0 = -1 and x0 + 1 = w' (and the same in y)."""
    import torch
    for kind, hw, lhw in SYNTHETIC:
        src, g_lo, g = _case_planes(kind, hw, lhw)
        parts = {}
        want = _upsample_ref(src, g_lo, g, parts=parts)
        sh = _shares(parts["path"])
        print(kind, hw, lhw, "shares", sh)
        if kind == "waves":
            full, partial = _wave_kinds(parts["path"], hw[1])
            assert {0, 1, 64} <= full and {0, 2} <= partial and sh[1] > 0 and sh[2] > 0, (full, partial, sh)
        elif kind == "sweep":
            assert parts["denormal"] > 100 and parts["underflow"] > 100 and sh[0] > 0 and sh[1] > 0
        elif hw != (2, 3):
            assert all(s > 0.02 for s in sh), sh
        if lhw[1] < hw[1]:
            assert parts["x0"][0] == -1 and parts["x0"][-1] + 1 == lhw[1]
        if lhw[0] < hw[0]:
            assert parts["y0"][0] == -1 and parts["y0"][-1] + 1 == lhw[0]
        film, lo, keep = _external_pair(pt, gpu_ctx, torch, src, g_lo, g)
        try:
            assert lo.read_f32().tobytes() == src.tobytes() and all(_guides_of(lo, pt)[n].tobytes() == g_lo[n].tobytes() for n in GUIDES)
            assert all(_guides_of(film, pt)[n].tobytes() == g[n].tobytes() for n in GUIDES)
            film.upsample(lo)
            _same(film.read_upsampled(), film.read_upsampled_bgra8(), want, (kind, hw, lhw))
            film.upsample(lo, sigma_normal=2.0, sigma_depth=0.02)
            _same(film.read_upsampled(), film.read_upsampled_bgra8(), _upsample_ref(src, g_lo, g, 2.0, 0.02), (kind, hw, lhw, "second set"))
        finally:
            film.close(); lo.close()
        del keep


@pytest.mark.gpu
def test_upsample_both_outputs_and_memory(pt, cornell_arrays):
    """read_upsampled before any call is PT_ERR_INVALID_ARG; a caller-owned device_out holds the bytes of the film-owned plane and leaves
    that plane (and its absence) alone; a second and third call allocate nothing (free device memory and pt_stats.workspace_bytes
    unchanged); a budget too small for the film's output, and one too small for lo's records alone, are PT_ERR_OOM with no result, and both
    films render on."""
    import torch
    w, h, lw, lh = 160, 120, 144, 100
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *cornell_arrays)
    # the full-size film holds guides alone, made by the single-kernel guide pass (next to no scratch); lo went through the queues
    film, lo = _rendered_pair(pt, ctx, sc, (w, h), (lw, lh), pt.PIPELINE_AUTO, lo_frames=1, lo_pipeline=pt.PIPELINE_WAVEFRONT)
    big, alone = pt.Film(ctx, 320, 240), pt.Film(ctx, lw, lh)
    big.enable_aov()
    try:
        def free():
            ctx.sync()
            torch.cuda.synchronize()
            return torch.cuda.mem_get_info()[0]

        def status(fn):
            with pytest.raises(pt.PtError) as e:
                fn()
            return e.value.status
        assert status(film.read_upsampled) == 1 and status(film.read_upsampled_bgra8) == 1
        # 320 * 240 * 16 B of output = 1.2 MB do not fit 1 MB.  160 * 120 * 16 B = 0.3 MB do, but lo's 144 * 100 * 48 B = 0.7 MB of records do not
        # fit beside the queues lo rendered through: that refusal takes the output back
        old = ctx.set_tuning(mem_budget_mb=1)
        for f, what in ((big, "upsample output"), (film, "denoiser workspace")):
            with pytest.raises(pt.PtError) as e:
                f.upsample(lo)
            assert e.value.status == 4 and what in str(e.value), (what, str(e.value))
            assert status(f.read_upsampled) == 1
        ctx.set_tuning(**old)
        kw = dict(width=lw, height=lh, spp_per_frame=4, max_depth=4, pipeline=pt.PIPELINE_WAVEFRONT)
        pt.render(sc, lo, pt.default_params(frame=1, frame_count=1, **kw))
        pt.render_aov(sc, lo, pt.default_params(frame=0, frame_count=2, **kw))
        pt.render_aov(sc, film, pt.default_params(width=w, height=h, spp_per_frame=4, pipeline=pt.PIPELINE_AUTO, frame=0, frame_count=2))
        pt.render(sc, alone, pt.default_params(frame=0, frame_count=2, **kw))
        assert lo.read_f32().tobytes() == alone.read_f32().tobytes()
        out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        film.upsample(lo, device_out=out.data_ptr())                             # into caller memory only ...
        assert status(film.read_upsampled) == 1                                  # ... the film still owns no result
        want = _upsample_ref(lo.read_f32(), _guides_of(lo, pt), _guides_of(film, pt))
        assert out.cpu().numpy().tobytes() == want[0].tobytes()
        film.upsample(lo)
        _same(film.read_upsampled(), film.read_upsampled_bgra8(), want, "owned")
        f1, ws = free(), ctx.stats().workspace_bytes
        film.upsample(lo)
        film.upsample(lo, sigma_normal=0.25)
        out.fill_(7.0)
        film.upsample(lo, device_out=out.data_ptr())
        assert free() == f1 and ctx.stats().workspace_bytes == ws
        assert out.cpu().numpy().tobytes() == want[0].tobytes() and film.read_upsampled().tobytes() != want[0].tobytes()
        film.upsample(lo)
        _same(film.read_upsampled(), film.read_upsampled_bgra8(), want, "again")
    finally:
        for f in (film, lo, big, alone):
            f.close()
        sc.close()
        ctx.close()


def _strips_ref(src, g_lo, g, n_strips=8):
    """_upsample_ref over horizontal strips of full-size rows, in threads (lo is a quarter of the size and is given whole)"""
    from concurrent.futures import ThreadPoolExecutor
    h = g["depth"].shape[0]
    edges = [h * k // n_strips for k in range(n_strips + 1)]
    with ThreadPoolExecutor(n_strips) as ex:
        res = list(ex.map(lambda k: _upsample_ref(src, g_lo, g, rows=(edges[k], edges[k + 1])), range(n_strips)))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def test_the_reference_in_strips_is_the_reference():
    """_strips_ref (what the full-size GPU test compares against) gives the bytes of _upsample_ref: a non-integer ratio, every path."""
    src, g_lo, g = _random_layers(45, 70, 16, 35, 9)
    want = _upsample_ref(src, g_lo, g)
    got = _strips_ref(src, g_lo, g, n_strips=7)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.gpu
def test_upsample_1080p_cornell_step(pt, gpu_ctx, cornell_gpu):
    """One full-size step: 1920 x 1080 from a 960 x 540 Cornell film (4 spp), at the defaults: SHA-256 of the float and of the bgra8 result
    against the reference over the whole frame (computed in strips, in threads)."""
    film, lo = _rendered_pair(pt, gpu_ctx, cornell_gpu, (1920, 1080), (960, 540), pt.PIPELINE_AUTO, max_depth=8, lo_frames=1)
    try:
        g, g_lo, c_lo = _guides_of(film, pt), _guides_of(lo, pt), lo.read_f32()
        ms = film.upsample(lo)
        got, got_bgra = film.read_upsampled(), film.read_upsampled_bgra8()
        want, want_bgra = _strips_ref(c_lo, g_lo, g)
        assert want.shape == got.shape and int((got != want).sum()) == 0
        assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(want.tobytes()).hexdigest()
        assert hashlib.sha256(got_bgra.tobytes()).hexdigest() == hashlib.sha256(want_bgra.tobytes()).hexdigest()
        assert ms > 0 and g["alpha"].mean() > 0.5 and got.any()
    finally:
        film.close(); lo.close()


@pytest.mark.gpu
def test_upsample_moves_nothing_else_and_shares_the_scratch(pt, gpu_ctx):
    """Both films' C, bgra8, every guide plane, M, L, lo's denoised plane and pt_stats are byte-identical before and after the call (from
    either source, into either output); a pt_film_denoise on lo after the upsample still equals its own reference although the upsample
    wrote lo's records into the scratch they share, and the upsample after it equals its own."""
    import torch
    sc = _scene(pt, gpu_ctx, "cornell")
    (w, h), (lw, lh) = (70, 46), (35, 23)
    film, lo = pt.Film(gpu_ctx, w, h), pt.Film(gpu_ctx, lw, lh)
    try:
        for f, (fw, fh) in ((film, (w, h)), (lo, (lw, lh))):
            f.enable_aov()
            f.enable_moments()
            f.enable_history()
            kw = dict(width=fw, height=fh, spp_per_frame=4, pipeline=pt.PIPELINE_AUTO, frame=0, frame_count=2)
            pt.render(sc, f, pt.default_params(max_depth=4, **kw))
            pt.render_aov(sc, f, pt.default_params(**kw))
            f.reproject(None)                                                    # (L = 1 where covered: a plane that is not all zeros)
        lo.denoise(iterations=2)

        def state():
            return ([[f.read_f32().tobytes(), f.read_bgra8().tobytes(), f.read_moments()[0].tobytes(), f.read_history().tobytes()] +
                     [f.read_aov(k).tobytes() for k in range(pt.AOV_COUNT)] for f in (film, lo)], lo.read_denoised().tobytes(),
                    lo.read_denoised_bgra8().tobytes(), bytes(gpu_ctx.stats()))
        before = state()
        assert film.read_history().any() and lo.read_moments()[0].any()
        g, g_lo, c_lo, d_lo = _guides_of(film, pt), _guides_of(lo, pt), lo.read_f32(), lo.read_denoised()
        out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        film.upsample(lo)
        film.upsample(lo, source=pt.UPSAMPLE_SRC_DENOISED, device_out=out.data_ptr())
        assert state() == before
        _same(film.read_upsampled(), film.read_upsampled_bgra8(), _upsample_ref(c_lo, g_lo, g), "film")
        _same(out.cpu().numpy(), None, _upsample_ref(d_lo, g_lo, g), "denoised")
        lo.denoise(iterations=3)
        _same(lo.read_denoised(), lo.read_denoised_bgra8(), _denoise_ref(c_lo, g_lo, 3), "denoise after the upsample")
        film.upsample(lo, source=pt.UPSAMPLE_SRC_DENOISED)
        _same(film.read_upsampled(), film.read_upsampled_bgra8(), _upsample_ref(lo.read_denoised(), g_lo, g), "upsample after the denoise")
    finally:
        film.close(); lo.close()


@pytest.mark.gpu
def test_upsample_errors(pt, gpu_ctx, cornell_gpu):
    """Every PT_ERR_INVALID_ARG of the header; a refused call writes nothing: the caller's output keeps its bytes and the film has no
    upsampled image afterwards."""
    import torch
    lib = pt.lib_amd()
    w, h, lw, lh = 48, 40, 24, 20
    out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    films = []

    def new(fw, fh, aov=True, ctx=gpu_ctx):
        f = pt.Film(ctx, fw, fh)
        films.append(f)
        if aov:
            f.enable_aov()
        return f

    def status(f, l, **kw):
        with pytest.raises(pt.PtError) as e:
            f.upsample(l, device_out=out.data_ptr(), **kw)
        with pytest.raises(pt.PtError) as e2:
            f.upsample(l, **kw)
        return e.value.status, e2.value.status

    other_ctx = pt.Context(0)
    try:
        film, lo = new(w, h), new(lw, lh)
        good = pt.upsample_default_params()
        assert lib.pt_film_upsample(None, lo.h, C.byref(good), out.data_ptr(), None) == 1       # NULL film
        assert lib.pt_film_upsample(film.h, None, C.byref(good), out.data_ptr(), None) == 1     # NULL lo
        assert lib.pt_film_upsample(film.h, lo.h, None, out.data_ptr(), None) == 1              # NULL params
        assert status(film, film) == (1, 1)                                                     # lo == film
        assert status(film, new(lw, lh, ctx=other_ctx)) == (1, 1)                               # another context's film
        assert status(film, new(w + 1, h)) == (1, 1) and status(film, new(w, h + 1)) == (1, 1)  # w' > w, h' > h
        assert status(new(w, h, aov=False), lo) == (1, 1) and status(film, new(lw, lh, aov=False)) == (1, 1)   # either film without guides
        for bad in (2, 7, 0xFFFFFFFF):
            assert status(film, lo, source=bad) == (1, 1), bad
        assert status(film, lo, source=pt.UPSAMPLE_SRC_DENOISED) == (1, 1)                      # lo never denoised
        dev = pt.DeviceBuffer(gpu_ctx, lw * lh * 12)
        lo.denoise(device_out=dev.ptr)                                                          # ... into caller memory: still no film-owned result
        assert status(film, lo, source=pt.UPSAMPLE_SRC_DENOISED) == (1, 1)
        dev.close()
        for bad in (0.0, -0.5, float("inf"), float("nan")):
            for name in ("sigma_normal", "sigma_depth"):
                assert status(film, lo, **{name: bad}) == (1, 1), (name, bad)
        for k in range(5):
            p = pt.upsample_default_params()
            p.reserved[k] = 1
            assert status(film, lo, params=p) == (1, 1)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all().item())                                                  # nothing written ...
        with pytest.raises(pt.PtError) as e:
            film.read_upsampled()                                                               # ... into either place
        assert e.value.status == 1
        # the caller's params object is not modified; the edges of what is allowed go through
        p = pt.upsample_default_params()
        film.upsample(lo, sigma_normal=2.0, source=pt.UPSAMPLE_SRC_FILM, params=p)
        assert (p.sigma_normal, p.source) == (DEFAULT_SIGMAS[0], 0)
        lo.denoise(iterations=1)
        film.upsample(lo, source=pt.UPSAMPLE_SRC_DENOISED)
        film.upsample(new(w, h))                                                                # w' = w, h' = h
        assert film.read_upsampled().shape == (h, w, 3)
    finally:
        for f in films:
            f.close()
        other_ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("denoise", [False, True], ids=["plain", "denoise"])
def test_pt_main_render_scale(pt, tmp_path, denoise):
    """pt_main --render-scale 2 [--denoise 3] writes the bytes of the Python path: lo at ceil(w / 2) x ceil(h / 2) rendered with its guides,
    the full-size guides, (Film.denoise(3) on lo,) Film.upsample; the PPM is the film-owned bgra8 form."""
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_main")
    if not os.path.exists(exe):
        pt.build()
    w, h, spp, depth = 49, 41, 4, 3
    lw, lh = 25, 21
    cmd = [exe, "--obj", pt.ASSET_CORNELL, "--width", str(w), "--height", str(h), "--frames", "2", "--spp", str(spp), "--depth", str(depth),
           "--render-scale", "2", "--ppm", str(tmp_path / "a.ppm"), "--pfm", str(tmp_path / "a.pfm")] + (["--denoise", "3"] if denoise else [])
    subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=pt.REPO, timeout=GPU_STEP_S)
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    film, lo = _rendered_pair(pt, ctx, sc, (w, h), (lw, lh), pt.PIPELINE_AUTO, spp=spp, max_depth=depth, lo_frames=2)
    try:
        if denoise:
            lo.denoise(iterations=3)
        film.upsample(lo, source=pt.UPSAMPLE_SRC_DENOISED if denoise else pt.UPSAMPLE_SRC_FILM)
        head = f"PF\n{w} {h}\n-1.0\n".encode()
        raw = open(tmp_path / "a.pfm", "rb").read()
        assert raw.startswith(head) and np.ascontiguousarray(np.frombuffer(raw[len(head):], f32).reshape(h, w, 3)[::-1]).tobytes() == film.read_upsampled().tobytes()
        ppm_head = f"P6\n{w} {h}\n255\n".encode()
        ppm = open(tmp_path / "a.ppm", "rb").read()
        assert ppm.startswith(ppm_head) and ppm[len(ppm_head):] == np.ascontiguousarray(film.read_upsampled_bgra8()[:, :, 2::-1]).tobytes()
        bad = subprocess.run([exe, "--render-scale", "1"], capture_output=True, text=True, cwd=pt.REPO, timeout=GPU_STEP_S)
        assert bad.returncode != 0 and "--render-scale" in bad.stderr
    finally:
        film.close(); lo.close(); sc.close(); ctx.close()
