"""pt_film_denoise_history: the variance-guided a-trous filter with a variance per pixel, for the film pt_film_reproject leaves
(include/pt_api.h).

`_history_ref` is the numpy statement of the header's definition, written like test_denoise_variance._variance_ref: float32 throughout, the
sums written out, a shifted-array pass per tap in the order j outer / i inner; from V0 on it is that function's text.  The CPU tests check
the exact properties of the definition on synthetic planes, the kernels' per-pixel bodies compiled for the host (plain and under the host's
sanitizers) and the value of the call (the experiment of DESIGN.md section 17); the GPU tests feed `_history_ref` the film, the guides, M and
L read back from the device.  Every GPU comparison is `tobytes()` equality."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import test_aov
import test_denoise
import test_denoise_variance
import test_reproject
from test_denoise import GUIDES, H_TAPS, _denoise_ref, _oracle_guides, _rel_mse, _same, _to_bgra8
from test_denoise_variance import G_TAPS, _shift, _variance_ref
from test_reproject import _cam, _oracle_planes, _reproject_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GPU_STEP_S = 120   # the time limit of a step that runs in a process of its own


def _guide_terms(N, Z, P, Q, inv_n, sz2):
    dn = N[P] - N[Q]
    x_n = ((dn[:, :, 0] * dn[:, :, 0] + dn[:, :, 1] * dn[:, :, 1]) + dn[:, :, 2] * dn[:, :, 2]) * inv_n
    dz = Z[P] - Z[Q]
    x_z = (dz * dz) / (sz2 * (Z[P] * Z[P] + Z[Q] * Z[Q]) + f32(1e-12))
    return x_n, x_z


def _history_ref(film, g, m2, hist_len, iterations=5, sigma_normal=0.5, sigma_depth=0.1, sigma_color=3.0, min_history=4.0, n_max=9.0, step_frames=1, parts=None):
    """-> (rgb float32 [H, W, 3], bgra uint8 [H, W, 4]).  film, g, m2 as in _variance_ref; hist_len [H, W] the plane L as stored.
    parts (a dict): receives I, V0, V (after the pre-blur), "short" (the pixels that took the spatial estimate) and Vs."""
    C_ = np.ascontiguousarray(film, f32)
    M = np.ascontiguousarray(m2, f32)
    L = np.ascontiguousarray(hist_len, f32)
    A, N, E, Z, al = (np.ascontiguousarray(g[k], f32) for k in GUIDES)
    assert all(a.dtype == f32 for a in (C_, M, L, A, N, E, Z, al))
    h, w = Z.shape
    one = f32(1.0)
    mh = f32(min_history)
    inv_n = one / (f32(sigma_normal) * f32(sigma_normal))
    sz2 = f32(sigma_depth) * f32(sigma_depth)
    sc2 = f32(sigma_color) * f32(sigma_color)
    D = np.maximum(A + (one - al)[:, :, None], f32(0.001))
    I = (C_ - E) / D
    with np.errstate(all="ignore"):
        long_ = L >= mh                                             # (a NaN fails)
        # long history (what a short pixel computes here is dropped by the select: its n - 1 may be 0 or negative)
        n = np.minimum(L * f32(step_frames), f32(n_max))
        v = np.maximum(M - C_ * C_, f32(0.0)) / (n - one)[:, :, None]
        vd = v / (D * D)
        Vl = (vd[:, :, 0] + vd[:, :, 1]) + vd[:, :, 2]
        assert n.dtype == f32 and Vl.dtype == f32
    # short history
    S = np.zeros((h, w), f32)
    s1 = np.zeros((h, w, 3), f32)
    s2 = np.zeros((h, w, 3), f32)
    for j in range(-2, 3):
        for i in range(-2, 3):
            pq = _shift(h, w, i, j)
            if pq is None:
                continue
            P, Q = pq
            x_n, x_z = _guide_terms(N, Z, P, Q, inv_n, sz2)
            t = np.maximum(f32(0.0), one - (x_n + x_z) * f32(0.0625))
            for _ in range(4):
                t = t * t
            S[P] = S[P] + t
            s1[P] = s1[P] + t[:, :, None] * I[Q]
            s2[P] = s2[P] + t[:, :, None] * (I[Q] * I[Q])
    mu = s1 / S[:, :, None]
    mm = s2 / S[:, :, None]
    s = np.maximum(mm - mu * mu, f32(0.0))
    e = I - mu
    Vs = ((s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]) + ((e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2])
    Lc = np.where(L > one, L, one)                                  # max(L, 1.0f), a NaN counting as 1
    V0 = np.where(long_, Vl, Vs * (mh / Lc))
    assert V0.dtype == f32 and Vs.dtype == f32 and (S > 0).all()
    # from here on: _variance_ref's text
    Sb = np.zeros((h, w), f32)
    Wb = np.zeros((h, w), f32)
    for j in range(-1, 2):
        for i in range(-1, 2):
            pq = _shift(h, w, i, j)
            if pq is None:
                continue
            P, Q = pq
            gg = G_TAPS[j + 1] * G_TAPS[i + 1]
            Sb[P] = Sb[P] + gg * V0[Q]
            Wb[P] = Wb[P] + gg
    V = Sb / Wb
    assert V.dtype == f32
    if parts is not None:
        parts.update(I=I, V0=V0, V=V, short=~long_, Vs=Vs)
    for k in range(iterations):
        st = 1 << k
        num = np.zeros((h, w, 3), f32)
        den = np.zeros((h, w), f32)
        vnum = np.zeros((h, w), f32)
        for j in range(-2, 3):
            for i in range(-2, 3):
                pq = _shift(h, w, st * i, st * j)
                if pq is None:
                    continue
                P, Q = pq
                x_n, x_z = _guide_terms(N, Z, P, Q, inv_n, sz2)
                di = I[P] - I[Q]
                with np.errstate(over="ignore"):   # (an infinite x_c is in the contract: weight 0)
                    x_c = ((di[:, :, 0] * di[:, :, 0] + di[:, :, 1] * di[:, :, 1]) + di[:, :, 2] * di[:, :, 2]) / (sc2 * (V[P] + V[Q]) + f32(1e-12))
                t = np.maximum(f32(0.0), one - ((x_n + x_z) + x_c) * f32(0.0625))
                for _ in range(4):
                    t = t * t
                wgt = (H_TAPS[j + 2] * H_TAPS[i + 2]) * t
                assert wgt.dtype == f32
                num[P] = num[P] + wgt[:, :, None] * I[Q]
                den[P] = den[P] + wgt
                vnum[P] = vnum[P] + (wgt * wgt) * V[Q]
        I = num / den[:, :, None]
        V = vnum / (den * den)
        assert I.dtype == f32 and V.dtype == f32
    out = I * D + E
    assert out.dtype == f32
    return out, _to_bgra8(out)


def _history_ref_strips(film, g, m2, hist_len, iterations, n_strips=8, **kw):
    """_history_ref over horizontal strips in threads: a strip carries a halo of 2 (the window) + 1 (the pre-blur) + 2 (2^n - 1) (the
    iterations) rows, clipped at the image's edge, so its own rows get the bytes of the whole image's statement"""
    h = film.shape[0]
    halo = 3 + 2 * ((1 << iterations) - 1)
    edges = [h * k // n_strips for k in range(n_strips + 1)]

    def one(k):
        y0, y1 = edges[k], edges[k + 1]
        a, b = max(0, y0 - halo), min(h, y1 + halo)
        sub = {n: np.ascontiguousarray(g[n][a:b]) for n in GUIDES}
        out, bgra = _history_ref(film[a:b], sub, m2[a:b], hist_len[a:b], iterations, **kw)
        return out[y0 - a:y1 - a], bgra[y0 - a:y1 - a]
    with ThreadPoolExecutor(n_strips) as ex:
        res = list(ex.map(one, range(n_strips)))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def _planes(h, w, seed):
    """random radiance and M over guides with partial coverage, a normal and a depth that vary (so the guides' weight takes every value
    from 0 to 1), emission in a tenth of the pixels -> (film, g, m2)"""
    rng = np.random.default_rng(seed)
    a = np.ones((h, w), f32)
    part = rng.uniform(0, 1, (h, w)) < 0.1
    a[part] = rng.choice(np.asarray([0.25, 0.5, 0.75], f32), int(part.sum()))
    a[rng.uniform(0, 1, (h, w)) < 0.03] = 0.0
    nrm = np.zeros((h, w, 3), f32)
    nrm[:, :, 2] = 1.0
    nrm[:, :, 0] = (rng.uniform(0, 1, (h, w)) < 0.5) * rng.uniform(0.0, 0.6, (h, w))
    nrm[:, w // 2:, 1] = 0.3
    depth = (3.0 + 0.05 * np.arange(w)[None, :] + rng.uniform(0, 0.3, (h, w))).astype(f32)
    g = {"albedo": (rng.uniform(0.2, 0.9, (h, w, 3)).astype(f32) * a[:, :, None]).astype(f32), "normal": (nrm * a[:, :, None]).astype(f32),
         "emission": (rng.uniform(0, 1, (h, w, 3)) * (rng.uniform(0, 1, (h, w, 1)) < 0.1)).astype(f32), "depth": (depth * a).astype(f32), "alpha": a}
    film = rng.uniform(0.0, 2.0, (h, w, 3)).astype(f32)
    m2 = (film * film + rng.uniform(0.0, 0.5, film.shape).astype(f32) * (rng.uniform(0, 1, (h, w, 1)) < 0.9)).astype(f32)
    return film, g, m2


def _len_pattern(h, w, name, seed=3):
    """the L planes of the tests (min_history 4): what pt_film_reproject leaves holds fractions, so the long values do"""
    rng = np.random.default_rng(seed)
    long_ = np.where(rng.uniform(0, 1, (h, w)) < 0.5, rng.integers(4, 13, (h, w)), rng.uniform(4.0, 33.0, (h, w))).astype(f32)
    short = np.where(rng.uniform(0, 1, (h, w)) < 0.5, rng.integers(1, 4, (h, w)), rng.uniform(1.0, 3.99, (h, w))).astype(f32)
    if name == "all_long":
        return long_
    if name == "all_short":
        return short
    if name == "zero":
        return np.zeros((h, w), f32)
    if name == "bands":     # a short column band at the left and at the right border
        x = np.arange(w)[None, :]
        return np.where((x < 3) | (x >= w - 2), short, long_).astype(f32)
    if name == "isolated":  # single short pixels, one of them a NaN, one a zero
        L = np.where(rng.uniform(0, 1, (h, w)) < 0.06, short, long_).astype(f32)
        L[h // 2, w // 2] = np.nan
        L[0, 0] = 0.0
        return L
    if name == "waves":     # rows of 64-pixel waves that are all-long, all-short and mixed (the vote of k_dn_var_spatial, both sides)
        L = long_.copy()
        for y in range(h):
            for x0 in range(0, w, 64):
                kind = (y + x0 // 64) % 3
                if kind == 1:
                    L[y, x0:x0 + 64] = short[y, x0:x0 + 64]
                elif kind == 2:
                    mix = rng.uniform(0, 1, w)[x0:x0 + 64] < 0.3
                    L[y, x0:x0 + 64] = np.where(mix, short[y, x0:x0 + 64], long_[y, x0:x0 + 64])
        if w > 128:
            L[0, :] = long_[0, :]                      # a row that is long in every wave ...
            L[0, 128:] = short[0, 128:]                # ... but for the partial last wave
            L[h - 1, :] = short[h - 1, :]
            L[h - 1, 128:] = long_[h - 1, 128:]
        return L
    raise KeyError(name)


PATTERNS = ["all_long", "all_short", "zero", "bands", "isolated"]


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
FIELDS = ["iterations", "sigma_normal", "sigma_depth", "sigma_color", "min_history", "n_max", "step_frames", "reserved"]
NEW_SYMBOLS = ["pt_denoise_history_params_default", "pt_film_denoise_history"]


def test_history_params_layout_defaults_and_symbols(pt, tmp_path):
    """sizeof / offsetof of pt_denoise_history_params by gcc from the header == the ctypes mirror (32 bytes); the defaults; the two new names
    in API_SYMBOLS and in the library; PT_API_VERSION stays 6."""
    src = tmp_path / "dh_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("%zu ' + "%zu " * len(FIELDS) + '%d\\n",'
                   "sizeof(pt_denoise_history_params), " + ", ".join(f"offsetof(pt_denoise_history_params, {n})" for n in FIELDS) +
                   ", PT_API_VERSION);return 0;}\n")
    exe = tmp_path / "dh_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = pt.DenoiseHistoryParams
    assert got == [C.sizeof(P)] + [getattr(P, n).offset for n in FIELDS] + [6], got
    assert got[0] == 32
    for name in NEW_SYMBOLS:
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    p = pt.denoise_history_default_params()   # (touches no device)
    assert (p.iterations, p.sigma_normal, p.sigma_depth, p.sigma_color, p.min_history, p.n_max, p.step_frames, list(p.reserved)) == (5, 0.5, f32(0.1), 3.0, 4.0, 9.0, 1, [0])
    alpha = pt.reproject_default_params().alpha
    assert abs((2.0 - alpha) / alpha - p.n_max) < 1e-5


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (40, 5), (23, 31)])
def test_long_history_is_the_variance_filter(shape):
    """L = n everywhere with mh <= n <= n_max and step_frames = 1: the bytes of _variance_ref(frames = n); L >= n_max: those of frames = 9;
    L = 2, step_frames = 2, mh = 1: those of frames = 4."""
    h, w = shape
    film, g, m2 = _planes(h, w, 5)
    for n in (4, 6, 9):
        got = _history_ref(film, g, m2, np.full((h, w), n, f32), iterations=3)
        want = _variance_ref(film, g, m2, n, iterations=3)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), n
    want9 = _variance_ref(film, g, m2, 9, iterations=3)
    for L in (np.full((h, w), 9.0, f32), np.full((h, w), 33.0, f32), _len_pattern(h, w, "all_long") + f32(5.0)):
        got = _history_ref(film, g, m2, L, iterations=3)
        assert got[0].tobytes() == want9[0].tobytes() and got[1].tobytes() == want9[1].tobytes()
    got = _history_ref(film, g, m2, np.full((h, w), 2.0, f32), iterations=3, min_history=1.0, step_frames=2)
    want = _variance_ref(film, g, m2, 4, iterations=3)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    # and another cap
    got = _history_ref(film, g, m2, np.full((h, w), 20.0, f32), iterations=2, n_max=5.0)
    assert got[0].tobytes() == _variance_ref(film, g, m2, 5, iterations=2)[0].tobytes()


def _flat(h, w, level=0.75):
    g = {"albedo": np.ones((h, w, 3), f32), "normal": np.zeros((h, w, 3), f32), "emission": np.zeros((h, w, 3), f32),
         "depth": np.full((h, w), 3.0, f32), "alpha": np.ones((h, w), f32)}
    g["normal"][:, :, 2] = 1.0
    film = np.full((h, w, 3), level, f32)
    return film, g


def test_short_history_estimate_exact_properties():
    """A constant image with every pixel short: V0 == 0 exactly (whatever M says).  One outlier among constants (uniform guides: every t is
    1, D is 1): the outlier's V0 is e*e*mh plus the window term, its neighbours see it through s and their own small e.  L = 0 gives the
    values of L = 1; a NaN L takes the short path and counts as 1."""
    h, w = 11, 13
    film, g = _flat(h, w)
    m2 = film * film + f32(0.3)
    parts = {}
    out, _ = _history_ref(film, g, m2, np.ones((h, w), f32), parts=parts)
    assert parts["short"].all() and not parts["V0"].any() and not parts["V"].any()
    assert (np.abs(out - film) <= f32(1e-5) * film).all()
    # the outlier: 25 taps of weight 1 inside the image, the values 0.75 (24 times) and 2.75 (once), all exact in binary32 sums
    film[5, 6] = f32(2.75)
    for mh, Lval in ((4.0, 1.0), (4.0, 2.0), (2.0, 1.0)):
        L = np.full((h, w), Lval, f32)
        _history_ref(film, g, film * film, L, min_history=mh, parts=parts)
        V0 = parts["V0"]
        lo, hi = f32(0.75), f32(2.75)
        s1 = f32(24) * lo + hi                      # (the running sums of the definition are exact here: multiples of 0.25 below 2^24 ulp)
        s2 = f32(24) * (lo * lo) + hi * hi
        mu, m = s1 / f32(25), s2 / f32(25)
        s = np.maximum(m - mu * mu, f32(0))
        scale = f32(mh) / f32(Lval)
        e = hi - mu
        want_out = (((s + s) + s) + ((e * e + e * e) + e * e)) * scale
        assert V0[5, 6] == want_out, (V0[5, 6], want_out)
        assert V0[5, 6] > (f32(3) * (e * e)) * scale                  # e * e * mh / L per channel, plus the window term
        e_n = lo - mu
        want_n = (((s + s) + s) + ((e_n * e_n + e_n * e_n) + e_n * e_n)) * scale
        near = np.zeros((h, w), bool)
        near[3:8, 4:9] = True
        near[5, 6] = False
        assert (V0[near] == want_n).all() and want_n < V0[5, 6] / f32(10)
        far = np.ones((h, w), bool)
        far[3:8, 4:9] = False
        assert not V0[far].any()
    # L = 0 == L = 1; NaN == 1 and short, among long neighbours
    film, g, m2 = _planes(17, 19, 8)
    a = _history_ref(film, g, m2, np.zeros((17, 19), f32), iterations=2, parts=parts)
    assert parts["short"].all()
    b = _history_ref(film, g, m2, np.ones((17, 19), f32), iterations=2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    L = np.full((17, 19), 6.0, f32)
    L[4, 5] = np.nan
    pa, pb = {}, {}
    a = _history_ref(film, g, m2, L, iterations=2, parts=pa)
    L[4, 5] = 1.0
    b = _history_ref(film, g, m2, L, iterations=2, parts=pb)
    assert pa["short"].sum() == 1 and pa["short"][4, 5] and np.isfinite(pa["V0"]).all()
    assert a[0].tobytes() == b[0].tobytes() and pa["V0"].tobytes() == pb["V0"].tobytes()


def test_borders_with_short_pixels():
    """1 x 1, 3 x 2 and 5 x 40 with 8 iterations and every L pattern: finite, no division by zero or invalid operation among the values that
    are kept; the 1 x 1 short pixel has V0 = 0 (its window is itself)."""
    for h, w in ((1, 1), (2, 3), (40, 5)):
        film, g, m2 = _planes(h, w, 4)
        g["alpha"][:] = 1.0
        for name in PATTERNS:
            parts = {}
            out, bgra = _history_ref(film, g, m2, _len_pattern(h, w, name), iterations=8, parts=parts)
            assert np.isfinite(out).all() and np.isfinite(parts["V0"]).all() and (parts["V0"] >= 0).all() and bgra.shape == (h, w, 4), (h, w, name)
            if (h, w) == (1, 1) and parts["short"].all():
                assert parts["V0"][0, 0] == 0


HOST_SHAPES = [(1, 1), (2, 3), (40, 5), (53, 77), (9, 130)]   # (h, w): 1 x 1, 3 x 2, 5 x 40, 77 x 53, 130 x 9


def _run_on_host(exe, d, film, g, m2, L, sigma_normal=0.5, sigma_depth=0.1, min_history=4.0, n_max=9.0, step_frames=1):
    """the kernels' bodies compiled for the host (tests/denoise_history_host.cpp) over the given planes -> (illum [H, W, 4], guide [H, W, 4])"""
    os.makedirs(d, exist_ok=True)
    h, w = L.shape
    np.asarray([w, h, sigma_normal, sigma_depth, min_history, step_frames, n_max, 0], f32).tofile(os.path.join(d, "par"))
    np.ascontiguousarray(film, f32).tofile(os.path.join(d, "film"))
    for n in GUIDES:
        np.ascontiguousarray(g[n], f32).tofile(os.path.join(d, n))
    np.ascontiguousarray(m2, f32).tofile(os.path.join(d, "m2"))
    np.ascontiguousarray(L, f32).tofile(os.path.join(d, "len"))
    subprocess.check_call([exe, d])
    return np.fromfile(os.path.join(d, "o_illum"), f32).reshape(h, w, 4), np.fromfile(os.path.join(d, "o_guide"), f32).reshape(h, w, 4)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_kernel_bodies_on_the_host_equal_the_reference(tmp_path, sanitize):
    """csrc/denoise_history_kernel.h -- the statements k_dn_prepare_hist and k_dn_var_spatial run per pixel -- compiled by g++ as a
    stand-alone program (-ffp-contract=off, the IEEE divide for pt_math.h's fdiv) gives the bytes of `_history_ref`'s I and V0 and the packed
    guides: five shapes, five L patterns (and the rows of waves of the GPU test), a second parameter set.  The second build runs the same
    cases under AddressSanitizer and UBSan: every tap address is inside its plane."""
    exe = str(tmp_path / "denoise_history_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "denoise_history_host.cpp")])
    n_short = n_long = 0
    for h, w in HOST_SHAPES:
        film, g, m2 = _planes(h, w, 31 + h)
        for name in PATTERNS + (["waves"] if w == 130 else []):
            L = _len_pattern(h, w, name)
            for kw in (dict(), dict(sigma_normal=2.0, sigma_depth=0.02, min_history=2.5, n_max=6.5, step_frames=2)):
                parts = {}
                _history_ref(film, g, m2, L, iterations=1, parts=parts, **kw)
                illum, guide = _run_on_host(exe, str(tmp_path / f"c{h}_{w}_{name}_{len(kw)}"), film, g, m2, L, **kw)
                what = (h, w, name, kw)
                assert illum[:, :, :3].tobytes() == parts["I"].tobytes(), what
                assert illum[:, :, 3].tobytes() == parts["V0"].tobytes(), (what, int((illum[:, :, 3] != parts["V0"]).sum()))
                assert guide[:, :, :3].tobytes() == g["normal"].tobytes() and guide[:, :, 3].tobytes() == g["depth"].tobytes(), what
                n_short += int(parts["short"].sum())
                n_long += int((~parts["short"]).sum())
    assert n_short > 10000 and n_long > 10000


# camera step per time step -> (r, r'): history <= guide-only / r and history <= variance8 / r' (r None: the variance8 ratio alone)
Q_PATHS = [((0.1, 0.0, 0.0), 1.09, 3.90), ((0.0, 0.0, 0.0), 1.28, 4.73), ((0.0, 0.0, -0.05), 1.0, 8.81)]
Q_STEPS = 8


def _masked_rel_mse(a, ref, mask):
    return _rel_mse(a[mask], ref[mask]) if mask.any() else float("nan")


def _quality_path(pt, orc, move):
    """DESIGN.md section 15's experiment with M carried along -> (covered, L, {name: image}, ref) at the last camera"""
    q = test_denoise.QUALITY
    osc = test_aov._oracle_scene(pt, orc, q["scene"])
    kw = dict(width=q["w"], height=q["h"])
    prev = prev_cam = None
    for k in range(Q_STEPS):
        cam = _cam(None, move, k)
        c = osc.render_frame(orc.default_params(frame=k, spp_per_frame=q["spp"], **kw, **cam), nthreads=16)[0]
        film = c if k == 0 else (c + np.zeros_like(c) * f32(k)) / f32(k + 1)       # a cleared film after frame k alone: k_resolve's blend
        m = c * c
        m2 = m if k == 0 else (m + np.zeros_like(m) * f32(k)) / f32(k + 1)         # ... and the plane's
        cur = {"C": film, "M": m2, **_oracle_planes(pt, orc, q["scene"], q["w"], q["h"], q["spp"], cam)}
        res = _reproject_ref(cur, prev, cam, prev_cam, gain=f32(k + 1) / f32(1))
        prev, prev_cam = {**cur, "C": res["C"], "M": res["M"], "L": res["L"]}, cam
    ref = np.zeros((q["h"], q["w"], 3), np.float64)
    for k in range(q["ref_frames"]):
        ref += osc.render_frame(orc.default_params(frame=1000 + k, spp_per_frame=q["ref_spp"], **kw, **cam), nthreads=16)[0]
    ref /= q["ref_frames"]
    g = _oracle_guides(pt, orc, q["scene"], q["w"], q["h"], q["spp"], 0, cam)
    acc, M, L = res["C"], res["M"], res["L"]
    images = {"accumulated": acc, "guide_only": _denoise_ref(acc, g)[0], "variance8": _variance_ref(acc, g, M, 8)[0], "history": _history_ref(acc, g, M, L)[0]}
    return cur["a"] > 0, L, images, ref


def test_quality_on_reprojected_films(pt, orc):
    """The experiment of DESIGN.md section 17: section 15's set-up exactly (Cornell box 128 x 96, 4 spp per step, 8 steps, step k at frame = k
    into a cleared film, gain = k + 1, guides at frame 0, the camera moved by the step each time) with M carried along (m = c * c, blended
    like C); against the mean of 64 frames of 32 spp at the last camera; relMSE as test_denoise._rel_mse.  Printed per path: the accumulated
    film, _denoise_ref, _variance_ref(frames = 8) and _history_ref, over the whole image, over the covered pixels with L < 4 and over the
    pixels with L >= 4.  Measured (whole image / covered pixels with L < 4 / pixels with L >= 4):
        camera step (0.1, 0, 0), 523 of 5666 covered pixels short (0.092)
            accumulated  0.2402 /  2.5285 / 0.3128        guide-only  0.0287 / 0.0741 / 0.0602
            variance8    0.1028 /  2.1789 / 0.0200        history     0.0132 / 0.0518 / 0.0255      guide-only / history 2.18, variance8 / history 7.80
        none (static), 298 of 6980 (0.043)
            accumulated  0.3502 /  5.1786 / 0.4130        guide-only  0.0334 / 0.1589 / 0.0542
            variance8    0.1227 /  4.6978 / 0.0161        history     0.0130 / 0.1416 / 0.0174      2.57, 9.46
        (0, 0, -0.05), 473 of 8399 (0.056)
            accumulated  0.6054 / 11.8127 / 0.2333        guide-only  0.0354 / 0.1427 / 0.0458
            variance8    0.4600 / 11.5496 / 0.0234        history     0.0261 / 0.1751 / 0.0295      1.36, 17.63
    (about 20 s of oracle time per path.)  Asserted per path: history <= guide-only / r and history <= variance8 / r' over the whole image, r
    and r' half the measured ratios -- the margin for seed and guide choices that sections 14 to 16 took -- with r never below 1 (half of 1.36
    is no bound at all: the dolly path asserts that the call is no worse than the guide-only filter) and r' never below 1.5; and the covered
    pixels with L < 4 are between 1 % and 15 % of the covered pixels, so that both estimates are in play."""
    rows = []
    for move, r, r2 in Q_PATHS:
        covered, L, im, ref = _quality_path(pt, orc, move)
        short, long_ = covered & (L < 4), L >= 4
        share = float(short.sum()) / float(covered.sum())
        e = {k: (_rel_mse(v, ref), _masked_rel_mse(v, ref, short), _masked_rel_mse(v, ref, long_)) for k, v in im.items()}
        print(f"camera step {move}: covered pixels with L < 4: {int(short.sum())} of {int(covered.sum())} ({share:.3f})")
        for k, v in e.items():
            print(f"    {k:12s} whole {v[0]:.4f}   covered L < 4 {v[1]:.4f}   L >= 4 {v[2]:.4f}")
        print(f"    guide-only / history {e['guide_only'][0] / e['history'][0]:.2f}   variance8 / history {e['variance8'][0] / e['history'][0]:.2f}")
        rows.append((move, r, r2, share, e))
    for move, r, r2, share, e in rows:
        assert 0.01 <= share <= 0.15, (move, share)
        assert r2 >= 1.5 and (r is None or r >= 1.0)
        assert e["history"][0] <= e["variance8"][0] / r2, (move, e["history"][0], e["variance8"][0], r2)
        if r is not None:
            assert e["history"][0] <= e["guide_only"][0] / r, (move, e["history"][0], e["guide_only"][0], r)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
_scene = test_denoise._scene
CHAIN_MOVE = (0.15, 0.0, 0.0)     # a sideways step: the side the camera moves towards gains a band of pixels without history every step
CHAIN_COMBOS = [(it, mh) for it in (1, 3, 5) for mh in (2.0, 4.0)]


def _chain(pt, ctx, sc, w, h, spp, cam0, pipeline, steps, move=CHAIN_MOVE, max_depth=4):
    """step 0 and `steps` reprojection steps of one frame each over two ping-ponged films with M and L -> (the last film, the other one)"""
    films = [test_reproject._new_film(pt, ctx, w, h, True) for _ in range(2)]
    prev = prev_cam = None
    for k in range(steps + 1):
        f = films[k & 1]
        f.clear()
        cam = _cam(cam0, move, k)
        test_reproject._render_step(pt, sc, f, w, h, spp, cam, k, pipeline, max_depth=max_depth)
        f.reproject(prev, cam, prev_cam or cam, gain=float(f32(k + 1)))
        prev, prev_cam = f, cam
    return films[steps & 1], films[(steps & 1) ^ 1]


def _read_inputs(film, pt):
    rgb, g = test_denoise._read_inputs(film, pt)
    return rgb, g, film.read_moments()[0], film.read_history()


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["WAVEFRONT", "AUTO"])
@pytest.mark.parametrize("case", sorted(test_denoise.CASES))
def test_denoise_history_rendered_chains(pt, gpu_ctx, case, pipeline):
    """The shapes and scenes of test_denoise.CASES: step 0 and three reprojection steps with a sideways camera move, then the call at
    iterations 1, 3, 5 and min_history 2, 4 against the reference fed with C, M, L and the guides read back from the film."""
    scene, w, h, spp, cam0 = test_denoise.CASES[case]
    film, other = _chain(pt, gpu_ctx, _scene(pt, gpu_ctx, scene), w, h, spp, cam0, getattr(pt, "PIPELINE_" + pipeline), 3)
    try:
        rgb, g, m2, L = _read_inputs(film, pt)
        covered = g["alpha"] > 0
        if case.startswith("cornell"):   # both estimates in play at either min_history: pixels that just restarted, pixels that kept all four steps
            assert (covered & (L == 1)).sum() >= h and (L == 4).sum() >= h, (int((covered & (L == 1)).sum()), int((L == 4).sum()))
        for it, mh in CHAIN_COMBOS:
            ms = film.denoise_history(iterations=it, min_history=mh)
            assert ms > 0
            _same(film.read_denoised(), film.read_denoised_bgra8(), _history_ref(rgb, g, m2, L, it, min_history=mh), (case, pipeline, it, mh))
    finally:
        film.close(); other.close()


def _external_film(pt, ctx, torch, rgb, g, m2, L):
    """test_denoise_variance._external_film plus an external history-length plane holding L"""
    film, keep = test_denoise_variance._external_film(pt, ctx, torch, rgb, g, m2)
    t_len = torch.full(L.shape, 5.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    film.enable_history(t_len.data_ptr())
    assert not t_len.any().item()                 # (zeroed by the call: filled afterwards)
    t_len.copy_(torch.from_numpy(np.ascontiguousarray(L)))
    torch.cuda.synchronize()
    return film, (keep, t_len)


SYNTHETIC = [((9, 130), "waves", dict(iterations=3)), ((9, 130), "waves", dict(iterations=2, step_frames=2, n_max=6.5, min_history=2.5)),
             ((53, 77), "isolated", dict(iterations=3, step_frames=2, n_max=6.5)), ((53, 77), "bands", dict(iterations=5)),
             ((40, 5), "bands", dict(iterations=4, step_frames=2, n_max=12.0)), ((40, 5), "all_short", dict(iterations=8)),
             ((1, 1), "all_short", dict(iterations=2, step_frames=2, n_max=3.0)), ((1, 1), "all_long", dict(iterations=1, step_frames=2, n_max=3.0)),
             ((53, 77), "zero", dict(iterations=2)), ((53, 77), "all_long", dict(iterations=2))]


@pytest.mark.gpu
def test_denoise_history_synthetic_planes(pt, gpu_ctx):
    """Planes made on the host in external tensors.  130 x 9: rows whose three waves (64, 64 and 2 lanes) are all-long, all-short and mixed,
    so both sides of k_dn_var_spatial's vote and the partial last wave are hit -- asserted on the plane before the comparison.  77 x 53,
    5 x 40 and 1 x 1 with step_frames = 2 and other n_max; a NaN and a zero L among long pixels."""
    import torch
    L = _len_pattern(9, 130, "waves")
    sh = ~(L >= 4)
    kinds = {(bool(sh[y, a:b].all()), bool(sh[y, a:b].any())) for y in range(9) for a, b in ((0, 64), (64, 128))}
    assert kinds == {(True, True), (False, True), (False, False)}
    assert sh[0, 128:].all() and not sh[0, :128].any() and not sh[8, 128:].any() and sh[8, :128].all()
    for (h, w), name, kw in SYNTHETIC:
        film_np, g, m2_np = _planes(h, w, 31 + h)
        L = _len_pattern(h, w, name)
        film, keep = _external_film(pt, gpu_ctx, torch, film_np, g, m2_np, L)
        try:
            rgb, g_dev, m2, L_dev = _read_inputs(film, pt)
            assert rgb.tobytes() == film_np.tobytes() and m2.tobytes() == m2_np.tobytes() and L_dev.tobytes() == L.tobytes()
            film.denoise_history(**kw)
            ref_kw = dict(kw)
            it = ref_kw.pop("iterations")
            _same(film.read_denoised(), film.read_denoised_bgra8(), _history_ref(film_np, g, m2_np, L, it, **ref_kw), ((h, w), name, kw))
        finally:
            film.close()
        del keep


@pytest.mark.gpu
def test_denoise_history_1080p_cornell_step(pt, gpu_ctx, cornell_gpu):
    """One 1920 x 1080 Cornell film after step 0 and two reprojection steps (camera step (0.02, 0, 0)), 3 iterations: SHA-256 of the float and
    of the bgra8 result against the reference over the whole frame (computed in strips with halos, in threads)."""
    w, h, spp = 1920, 1080, 4
    film, other = _chain(pt, gpu_ctx, cornell_gpu, w, h, spp, None, pt.PIPELINE_AUTO, 2, move=(0.02, 0.0, 0.0), max_depth=8)
    try:
        rgb, g, m2, L = _read_inputs(film, pt)
        covered = g["alpha"] > 0
        assert (covered & (L < 3)).any() and (L == 3).mean() > 0.5
        film.denoise_history(iterations=3, min_history=3.0)
        got, got_bgra = film.read_denoised(), film.read_denoised_bgra8()
        want, want_bgra = _history_ref_strips(rgb, g, m2, L, 3, min_history=3.0)
        assert want.shape == got.shape and int((got != want).sum()) == 0
        assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(want.tobytes()).hexdigest()
        assert hashlib.sha256(got_bgra.tobytes()).hexdigest() == hashlib.sha256(want_bgra.tobytes()).hexdigest()
        assert not np.array_equal(got, rgb)
    finally:
        film.close(); other.close()


@pytest.mark.gpu
def test_denoise_history_moves_nothing_else_and_shares_the_scratch(pt, cornell_arrays):
    """Film, bgra8, M, L, the guides and pt_stats are byte-identical before and after a call; pt_film_denoise_variance and pt_film_denoise
    on the same film give the same bytes before and after it; an external output == the film-owned plane, which that call leaves alone.
    Scratch: it is pt_film_denoise_variance's -- pt_stats.workspace_bytes does not move, a budget of 1 MB refuses the first call of either
    filter on a fresh 160 x 120 film (0.9 MB of scratch + 0.3 MB of output) with PT_ERR_OOM and no result, and once either has run the other
    takes nothing more from the device."""
    import torch
    w, h, spp = 160, 120, 4
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *cornell_arrays)
    film, other = _chain(pt, ctx, sc, w, h, spp, None, pt.PIPELINE_AUTO, 3)
    twin, other2 = _chain(pt, ctx, sc, w, h, spp, None, pt.PIPELINE_AUTO, 3)
    try:
        def state(f):
            s = ctx.stats()
            return ([f.read_f32().tobytes(), f.read_bgra8().tobytes(), f.read_moments()[0].tobytes(), f.read_moments()[1], f.read_history().tobytes()] +
                    [f.read_aov(k).tobytes() for k in range(pt.AOV_COUNT)], bytes(s))

        def free():
            ctx.sync()
            torch.cuda.synchronize()
            return torch.cuda.mem_get_info()[0]

        def result(f):
            return f.read_denoised().tobytes(), f.read_denoised_bgra8().tobytes()
        assert state(film)[0] == state(twin)[0]
        before = state(film)
        ws = ctx.stats().workspace_bytes
        old = ctx.set_tuning(mem_budget_mb=1)
        for call in (lambda: film.denoise_history(), lambda: twin.denoise_variance(frames=4)):
            with pytest.raises(pt.PtError) as e:
                call()
            assert e.value.status == 4
        for f in (film, twin):
            with pytest.raises(pt.PtError) as e:
                f.read_denoised()
            assert e.value.status == 1
        ctx.set_tuning(**old)
        assert state(film) == before
        film.denoise_history()
        twin.denoise_variance(frames=4)
        f2 = free()
        assert ctx.stats().workspace_bytes == ws
        hist = result(film)
        rgb, g, m2, L = _read_inputs(film, pt)
        assert ((L < 4) & (g["alpha"] > 0)).any() and (L >= 4).any()
        _same(film.read_denoised(), film.read_denoised_bgra8(), _history_ref(rgb, g, m2, L), "owned")
        film.denoise_variance(frames=4)
        var = result(film)
        assert var == result(twin) and var != hist
        film.denoise()
        plain = result(film)
        twin.denoise_history()
        assert result(twin) == hist
        film.denoise_history(iterations=2, min_history=2.0)
        film.denoise_history()
        assert result(film) == hist
        film.denoise_variance(frames=4)
        assert result(film) == var
        film.denoise()
        assert result(film) == plain
        assert free() == f2 and ctx.stats().workspace_bytes == ws
        assert state(film) == before
        out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        f3 = free()
        film.denoise_history(device_out=out.data_ptr())
        assert out.cpu().numpy().tobytes() == hist[0] and film.read_denoised().tobytes() == plain[0]
        assert state(film) == before and free() == f3
    finally:
        for f in (film, other, twin, other2):
            f.close()
        sc.close()
        ctx.close()


@pytest.mark.gpu
def test_denoise_history_errors(pt, gpu_ctx, cornell_gpu):
    """Every PT_ERR_INVALID_ARG of the header; a refused call writes nothing: the caller's output keeps its bytes and the film has no
    denoised image afterwards."""
    import torch
    lib = pt.lib_amd()
    w, h = 48, 40
    out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def status(f, **kw):
        with pytest.raises(pt.PtError) as e:
            f.denoise_history(device_out=out.data_ptr(), **kw)
        with pytest.raises(pt.PtError) as e2:
            f.denoise_history(**kw)
        return e.value.status, e2.value.status

    good = pt.denoise_history_default_params()
    films = []
    try:
        # a film without guides, without M, without L: every combination but the complete one
        for aov, mom, hist in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0), (1, 0, 0)):
            f = pt.Film(gpu_ctx, w, h)
            films.append(f)
            if aov:
                f.enable_aov()
            if mom:
                f.enable_moments()
            if hist:
                f.enable_history()
            assert status(f) == (1, 1), (aov, mom, hist)
        film = test_reproject._new_film(pt, gpu_ctx, w, h, True)
        films.append(film)
        assert lib.pt_film_denoise_history(None, C.byref(good), out.data_ptr(), None) == 1      # NULL film
        assert lib.pt_film_denoise_history(film.h, None, out.data_ptr(), None) == 1             # NULL params
        lib.pt_denoise_history_params_default(None)                                             # (a NULL is ignored)
        cam = _cam()
        test_reproject._render_step(pt, cornell_gpu, film, w, h, 4, cam, 0, pt.PIPELINE_AUTO, max_depth=3)
        film.reproject(None, cam, cam)
        nan, inf = float("nan"), float("inf")
        for it in (0, 9, 0xFFFFFFFF):
            assert status(film, iterations=it) == (1, 1), it
        for bad in (0.0, -0.5, inf, nan):
            for name in ("sigma_normal", "sigma_depth", "sigma_color"):
                assert status(film, **{name: bad}) == (1, 1), (name, bad)
        for bad in (0.0, 0.5, -4.0, 65537.0, inf, nan):
            assert status(film, min_history=bad) == (1, 1), bad
        for bad in (1.0, 1.999, 0.0, -9.0, inf, nan):
            assert status(film, n_max=bad) == (1, 1), bad
        assert status(film, step_frames=0) == (1, 1)
        assert status(film, min_history=1.0) == (1, 1) and status(film, min_history=1.5, step_frames=1) == (1, 1)    # min_history * step_frames < 2
        p = pt.denoise_history_default_params()
        p.reserved[0] = 1
        assert status(film, params=p) == (1, 1)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all().item())                                                    # nothing written ...
        with pytest.raises(pt.PtError) as e:
            film.read_denoised()                                                                  # ... into either place
        assert e.value.status == 1
        for kw in (dict(min_history=1.0, step_frames=2), dict(min_history=2.0), dict(min_history=65536.0), dict(n_max=2.0), dict(iterations=1), dict(iterations=8)):
            film.denoise_history(**kw)                                                            # the ends of the ranges go through
        assert film.read_denoised().shape == (h, w, 3)
    finally:
        for f in films:
            f.close()


@pytest.mark.gpu
def test_pt_main_temporal_sigma_color(pt, tmp_path):
    """pt_main --temporal 3 --cam-step 0.02,0,0 --denoise --sigma-color 3 writes the bytes of the Python chain: films with M and L, three
    time steps, then Film.denoise_history(sigma_color = 3); the normal outputs are those of the run without --sigma-color."""
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_main")
    if not os.path.exists(exe):
        pt.build()
    w, h, spp, depth, K, move = 48, 40, 4, 3, 3, (0.02, 0.0, 0.0)
    base = [exe, "--obj", pt.ASSET_CORNELL, "--width", str(w), "--height", str(h), "--spp", str(spp), "--depth", str(depth), "--temporal", str(K), "--cam-step", "0.02,0,0"]
    run = dict(check=True, capture_output=True, text=True, cwd=pt.REPO, timeout=GPU_STEP_S)
    subprocess.run(base + ["--pfm", str(tmp_path / "a.pfm"), "--denoise"], **run)
    subprocess.run(base + ["--ppm", str(tmp_path / "b.ppm"), "--pfm", str(tmp_path / "b.pfm"), "--denoise", "--sigma-color", "3"], **run)
    assert open(tmp_path / "a.pfm", "rb").read() == open(tmp_path / "b.pfm", "rb").read()
    assert open(tmp_path / "a.denoised.pfm", "rb").read() != open(tmp_path / "b.denoised.pfm", "rb").read()
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    film, other = _chain(pt, ctx, sc, w, h, spp, None, pt.PIPELINE_AUTO, K - 1, move=move, max_depth=depth)
    try:
        head = f"PF\n{w} {h}\n-1.0\n".encode()
        raw = open(tmp_path / "b.pfm", "rb").read()
        assert raw.startswith(head) and np.ascontiguousarray(np.frombuffer(raw[len(head):], f32).reshape(h, w, 3)[::-1]).tobytes() == film.read_f32().tobytes()
        film.denoise_history(sigma_color=3.0)
        raw = open(tmp_path / "b.denoised.pfm", "rb").read()
        assert raw.startswith(head)
        den = np.ascontiguousarray(np.frombuffer(raw[len(head):], f32).reshape(h, w, 3)[::-1])
        assert den.tobytes() == film.read_denoised().tobytes()
        ppm_head = f"P6\n{w} {h}\n255\n".encode()
        ppm = open(tmp_path / "b.denoised.ppm", "rb").read()
        assert ppm.startswith(ppm_head) and ppm[len(ppm_head):] == np.ascontiguousarray(film.read_denoised_bgra8()[:, :, 2::-1]).tobytes()
        assert (film.read_history() == 3).any() and (film.read_history() == 1).any()
    finally:
        film.close(); other.close(); sc.close(); ctx.close()
