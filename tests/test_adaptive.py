"""pt_render_adaptive (include/pt_api.h): the film's variance decides which 8x8 tiles are traced, and their pixels are blended by their own
frame count K.  `_adaptive_ref` below restates the header's definition in numpy -- selection, blend and the byte rule -- and every comparison
with the device is byte equality: the planes C, M, K and bgra8, the result record, and the growth of pt_stats.rays / paths, against the
oracle's per-frame colours and ray maps fed through the restatement.  The order of the compacted tile list cannot be observed through the
ABI and is not tested."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_aov
import test_denoise

f32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(threshold=0.05, rel_floor=0.01, min_frames=4, max_frames=0)   # pt_adaptive_params_default


# ---- the definition, in numpy ---------------------------------------------------------------------------------------------------------
def _tile_list(w, h, rank=0, world=1):
    """the (rank, world) tiles of a w x h film, row by row -> [(tx, ty)]"""
    return [(tx, ty) for ty in range((h + 7) // 8) for tx in range((w + 7) // 8) if (tx + ty) % world == rank]


def _select_ref(Cp, M, K, threshold=0.05, rel_floor=0.01, min_frames=4, max_frames=0, rank=0, world=1):
    """-> dict: tiles [(tx, ty)], sel / short / capped [n_tiles] bool, et [n_tiles] f32, mask [H, W] bool (the valid pixels of the selected
    tiles) and the result record's fields"""
    h, w = K.shape
    tl = _tile_list(w, h, rank, world)
    tiles = np.asarray(tl, np.int64).reshape(-1, 2)
    lane = np.arange(64)
    px, py = tiles[:, 0:1] * 8 + (lane & 7), tiles[:, 1:2] * 8 + (lane >> 3)
    valid = (px < w) & (py < h)
    qx, qy = np.minimum(px, w - 1), np.minimum(py, h - 1)
    c, m, k = Cp[qy, qx], M[qy, qx], K[qy, qx]
    assert c.dtype == f32 and m.dtype == f32 and k.dtype == f32
    with np.errstate(all="ignore"):
        v = np.maximum(m - c * c, f32(0)) / (k - f32(1))[..., None]
        e = np.sqrt((v[..., 0] + v[..., 1]) + v[..., 2]) / (((c[..., 0] + c[..., 1]) + c[..., 2]) + f32(rel_floor))
    x = np.where(valid & (k >= f32(2)), e, f32(0)).astype(f32)
    for _ in range(6):
        x = x[:, 0::2] + x[:, 1::2]
    n_valid = valid.sum(1)
    et = (x[:, 0] / n_valid.astype(f32)).astype(f32) if len(tl) else np.zeros(0, f32)
    short = (valid & ~(k >= f32(min_frames))).any(1)
    capped = ~(valid & ~(k >= f32(max_frames))).any(1) if max_frames > 0 else np.zeros(len(tl), bool)
    sel = ~capped & (short | (et > f32(threshold)))
    mask = np.zeros((h, w), bool)
    mask[py[sel][valid[sel]], px[sel][valid[sel]]] = True
    me = et[~short]
    return dict(tiles=tl, sel=sel, short=short, capped=capped, et=et, mask=mask, n_valid=n_valid, tiles_total=len(tl), tiles_selected=int(sel.sum()),
                pixels_selected=int(n_valid[sel].sum()), max_error=f32(max(me.max(), f32(0))) if len(me) else f32(0))


class _State:
    """a film's four planes on the host"""

    def __init__(self, w, h):
        self.C, self.M = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
        self.K, self.bgra = np.zeros((h, w), f32), np.zeros((h, w, 4), np.uint8)

    def copy(self):
        s = _State(1, 1)
        s.C, s.M, s.K, s.bgra = self.C.copy(), self.M.copy(), self.K.copy(), self.bgra.copy()
        return s


def _blend_ref(st, col, mask):
    """one frame colour [H, W, 3] blended into the pixels of `mask`, by each pixel's own count"""
    n = st.K[mask]
    first, n1 = (n == f32(0))[:, None], (n + f32(1))[:, None]
    nn = n[:, None]
    c = np.ascontiguousarray(col, f32)[mask]
    for plane, val in ((st.C, c), (st.M, c * c)):
        plane[mask] = (val + np.where(first, f32(0), plane[mask]) * nn) / n1
    old = np.where(first, f32(0), st.bgra[mask].astype(f32) / f32(255))
    src = np.stack([c[:, 2], c[:, 1], c[:, 0], np.ones(len(c), f32)], 1)   # bytes B, G, R, A; A from 1.0
    new = ((src + old * nn) / n1).astype(f32)
    st.bgra[mask] = np.where(new > 0, np.minimum(new, f32(1)) * f32(255) + f32(0.5), f32(0)).astype(np.uint8)
    st.K[mask] = n1[:, 0]


def _adaptive_ref(st, cols, ray_maps=None, rank=0, world=1, **ap):
    """one pt_render_adaptive call: the selection from the state as it stands, then `cols` (the frames' colours, ascending) blended into the
    selected pixels -> (the selection, rays traced)"""
    s = _select_ref(st.C, st.M, st.K, rank=rank, world=world, **{**DEFAULTS, **ap})
    for col in cols:
        _blend_ref(st, col, s["mask"])
    rays = sum(int(r[s["mask"]].sum()) for r in ray_maps) if ray_maps is not None else 0
    return s, rays


# ---- synthetic planes: every edge of the selection in one film -----------------------------------------------------------------------------
KINDS = ["noisy", "miss", "short", "capped", "denormal", "quiet"]
EDGE_MAX_FRAMES = 16


def _edge_planes(w, h, seed=1, rot=0):
    """C, M, K whose tiles take the kinds in turn (tile i of the row-by-row list is KINDS[(i + rot) % 6]): noisy (e_T well above 0.05), a
    tile of misses (M = C*C: e_T = 0), short (one pixel with K = 1 in a quiet tile), capped (noisy, every K = EDGE_MAX_FRAMES), denormal
    variances (C = 0, M subnormal: e_T > 0 only where denormals are kept) and quiet (e_T around 0.01)."""
    rng = np.random.default_rng(seed)
    st = _State(w, h)
    st.C[:] = rng.uniform(0.1, 1.0, (h, w, 3)).astype(f32)
    st.K[:] = f32(8)
    st.bgra[:] = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    kinds = {}
    for i, (tx, ty) in enumerate(_tile_list(w, h)):
        kind = KINDS[(i + rot) % len(KINDS)]
        kinds[(tx, ty)] = kind
        sl = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
        c = st.C[sl]
        var = {"noisy": 0.5, "capped": 0.5, "quiet": 0.002, "short": 0.002}.get(kind, 0.0)
        st.M[sl] = c * c + (rng.uniform(0.5, 1.0, c.shape) * var).astype(f32) * c * c
        if kind == "miss":
            st.M[sl] = c * c
        elif kind == "short":
            st.K[sl][rng.integers(0, st.K[sl].shape[0]), rng.integers(0, st.K[sl].shape[1])] = f32(1)
        elif kind == "capped":
            st.K[sl] = f32(EDGE_MAX_FRAMES)
        elif kind == "denormal":
            st.C[sl] = f32(0)
            st.M[sl] = rng.uniform(1e-39, 9e-39, c.shape).astype(f32)
    return st, kinds


def _same_state(got, want, what):
    for name in ("C", "M", "K", "bgra"):
        g, w_ = getattr(got, name), getattr(want, name)
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, name)
        assert g.tobytes() == w_.tobytes(), (what, name, int((g != w_).sum()))


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------
P_FIELDS = ["threshold", "rel_floor", "min_frames", "max_frames", "reserved"]
R_FIELDS = ["tiles_total", "tiles_selected", "pixels_selected", "max_error", "select_ms", "reserved"]
NEW_SYMBOLS = ["pt_film_enable_counts", "pt_film_read_counts", "pt_adaptive_params_default", "pt_render_adaptive"]


def test_adaptive_layout_defaults_and_symbols(pt, tmp_path):
    """sizeof / offsetof of pt_adaptive_params and pt_adaptive_result by gcc from the header == the ctypes mirrors (32 bytes each); the
    defaults; the new names in API_SYMBOLS and in the library; PT_API_VERSION stays 6; NULL handles are PT_ERR_INVALID_ARG."""
    src = tmp_path / "ad_layout.c"
    offs = [f"offsetof(pt_adaptive_params, {n})" for n in P_FIELDS] + [f"offsetof(pt_adaptive_result, {n})" for n in R_FIELDS]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("' + "%zu " * (2 + len(offs)) + '%d\\n",'
                   "sizeof(pt_adaptive_params), sizeof(pt_adaptive_result), " + ", ".join(offs) + ", PT_API_VERSION);return 0;}\n")
    exe = tmp_path / "ad_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P, R = pt.AdaptiveParams, pt.AdaptiveResult
    assert got == [C.sizeof(P), C.sizeof(R)] + [getattr(P, n).offset for n in P_FIELDS] + [getattr(R, n).offset for n in R_FIELDS] + [6], got
    assert got[:2] == [32, 32] and got[2:7] == [0, 4, 8, 12, 16] and got[7:13] == [0, 4, 8, 16, 20, 24]
    for name in NEW_SYMBOLS:
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    p = pt.adaptive_default_params()   # (touches no device)
    assert (p.threshold, p.rel_floor, p.min_frames, p.max_frames, list(p.reserved)) == (f32(0.05), f32(0.01), 4, 0, [0] * 4)
    lib = pt.lib_amd()
    lib.pt_adaptive_params_default(None)                                     # (a NULL is ignored)
    assert lib.pt_render_adaptive(None, None, None, C.byref(p), None) == 1
    assert lib.pt_film_enable_counts(None, None) == 1 and lib.pt_film_read_counts(None, None) == 1


def test_the_reference_blend_with_equal_counts_is_the_oracles_blend(orc):
    """With K == frame everywhere the count blend and the byte rule of `_blend_ref` are the oracle's accumulate_f32 / accumulate_bgra8, frame
    after frame: the restatement's blend is pt_render's."""
    rng = np.random.default_rng(3)
    h, w = 11, 13
    st = _State(w, h)
    ofilm, obgra = np.zeros((h, w, 3), f32), np.zeros((h, w, 4), np.uint8)
    mask = np.ones((h, w), bool)
    for frame in range(6):
        col = (rng.uniform(-0.1, 1.4, (h, w, 3)) ** 3).astype(f32)
        _blend_ref(st, col, mask)
        orc.accumulate_f32(ofilm, col, frame)
        orc.accumulate_bgra8(obgra, col, frame)
        assert st.C.tobytes() == ofilm.tobytes() and st.bgra.tobytes() == obgra.tobytes(), frame
        assert (st.K == f32(frame + 1)).all()


def _threshold_tile(s):
    """a tile that is neither short nor capped, with the largest e_T below 0.05 -> its index"""
    ok = ~s["short"] & ~s["capped"] & (s["et"] > 0) & (s["et"] < f32(0.05))
    assert ok.any()
    return int(np.argmax(np.where(ok, s["et"], f32(-1))))


def test_selection_properties_on_synthetic_planes():
    """The exact properties of the definition, on the reference: a tile with e_T == threshold is not selected (and is with the next smaller
    threshold); the corner tile of a 9 x 9 film has one valid pixel; a tile of misses has e_T = 0; one pixel with K = 1 makes a tile short;
    max_frames stops a noisy tile; denormal variances give e_T > 0."""
    st, kinds = _edge_planes(76, 44)
    s = _select_ref(st.C, st.M, st.K, **DEFAULTS)
    s_cap = _select_ref(st.C, st.M, st.K, **{**DEFAULTS, "max_frames": EDGE_MAX_FRAMES})
    for i, t in enumerate(s["tiles"]):
        kind = kinds[t]
        if kind == "noisy":
            assert s["sel"][i] and s["et"][i] > f32(0.05) and not s["short"][i]
        elif kind == "miss":
            assert s["et"][i] == 0 and not s["sel"][i]
        elif kind == "short":
            assert s["short"][i] and s["sel"][i] and s["et"][i] < f32(0.05)
        elif kind == "capped":
            assert s["sel"][i] and s_cap["capped"][i] and not s_cap["sel"][i]
        elif kind == "denormal":
            assert 0 < s["et"][i] < f32(1e-10) and not s["sel"][i]
        else:
            assert 0 < s["et"][i] < f32(0.05) and not s["sel"][i]
    assert len(set(kinds.values())) == len(KINDS) and not s_cap["capped"][[kinds[t] != "capped" for t in s["tiles"]]].any()
    assert s["max_error"] == s["et"][~s["short"]].max() and s["pixels_selected"] == int(s["mask"].sum())
    k = _threshold_tile(s)
    at = _select_ref(st.C, st.M, st.K, **{**DEFAULTS, "threshold": float(s["et"][k])})
    below = _select_ref(st.C, st.M, st.K, **{**DEFAULTS, "threshold": float(np.nextafter(s["et"][k], f32(0)))})
    assert not at["sel"][k] and below["sel"][k] and (at["et"] == s["et"]).all()
    zero = _select_ref(st.C, st.M, st.K, **{**DEFAULTS, "threshold": 0.0})   # every tile with a nonzero error, the denormal ones included
    assert all(zero["sel"][i] == (kinds[t] != "miss") for i, t in enumerate(s["tiles"]))
    for rot in range(len(KINDS)):   # 9 x 9: four tiles, the last one a single pixel
        st9, kinds9 = _edge_planes(9, 9, rot=rot)
        s9 = _select_ref(st9.C, st9.M, st9.K, **DEFAULTS)
        assert list(s9["n_valid"]) == [64, 8, 8, 1] and s9["tiles"][3] == (1, 1)
        c, m, kk = st9.C[8, 8], st9.M[8, 8], st9.K[8, 8]
        with np.errstate(all="ignore"):
            v = np.maximum(m - c * c, f32(0)) / (kk - f32(1))
            e = np.sqrt((v[0] + v[1]) + v[2]) / (((c[0] + c[1]) + c[2]) + f32(0.01))
        assert s9["et"][3] == (e if kk >= 2 else f32(0))   # (the sum of one error and 63 zeros, divided by 1.0)


HOST_CASES = [(8, 8), (9, 9), (76, 44), (17, 3)]


def _run_on_host(exe, d, st, cols, **ap):
    """the kernels' bodies compiled for the host (tests/adaptive_host.cpp) over the given state -> (sel per tile, e_T per tile, the state after)"""
    os.makedirs(d, exist_ok=True)
    a = {**DEFAULTS, **ap}
    h, w = st.K.shape
    np.asarray([w, h, a["threshold"], a["rel_floor"], a["min_frames"], a["max_frames"], len(cols), 0], f32).tofile(os.path.join(d, "par"))
    for name in ("C", "M", "K", "bgra"):
        getattr(st, name).tofile(os.path.join(d, name))
    np.ascontiguousarray(np.stack(cols), f32).tofile(os.path.join(d, "col"))
    subprocess.check_call([exe, d])
    out = _State(w, h)
    out.C, out.M = np.fromfile(os.path.join(d, "o_C"), f32).reshape(h, w, 3), np.fromfile(os.path.join(d, "o_M"), f32).reshape(h, w, 3)
    out.K, out.bgra = np.fromfile(os.path.join(d, "o_K"), f32).reshape(h, w), np.fromfile(os.path.join(d, "o_bgra"), np.uint8).reshape(h, w, 4)
    return np.fromfile(os.path.join(d, "o_sel"), np.uint8).astype(bool), np.fromfile(os.path.join(d, "o_et"), f32), out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_kernel_bodies_on_the_host_equal_the_reference(tmp_path, sanitize):
    """csrc/adaptive_kernel.h -- the statements k_adapt_select runs per lane and k_resolve_adapt per frame -- compiled by g++ as a stand-alone
    program (-ffp-contract=off, the IEEE divide and root for pt_math.h's) give the bytes of `_adaptive_ref`: selection, e_T and the four
    planes after three frames, over every kind of tile, with and without max_frames, at the thresholds of the exact-property test.  The
    second build runs the same cases under AddressSanitizer and UBSan: every address is inside its plane."""
    exe = str(tmp_path / "adaptive_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "adaptive_host.cpp")])
    rng = np.random.default_rng(9)
    n_sel = n_not = 0
    for k, (w, h) in enumerate(HOST_CASES):
        for rot in range(len(KINDS) if w * h <= 81 else 1):
            st, _ = _edge_planes(w, h, seed=k + 1, rot=rot)
            if rot == 1:
                st.K[:] = f32(0)   # an empty film: the blend's first frame reads no old value
                st.C[:] = f32(np.nan); st.M[:] = f32(np.nan)
            et0 = _select_ref(st.C, st.M, st.K, **DEFAULTS)["et"]
            cols = [(rng.uniform(-0.1, 1.3, (h, w, 3)) ** 3).astype(f32) for _ in range(3)]
            for ap in (dict(), dict(max_frames=EDGE_MAX_FRAMES), dict(threshold=0.0), dict(threshold=float(et0[np.argmax(et0 < f32(0.05))]), rel_floor=0.01),
                       dict(threshold=0.02, rel_floor=1e-30, min_frames=9)):
                want = st.copy()
                s, _ = _adaptive_ref(want, cols, **ap)
                sel, et, got = _run_on_host(exe, str(tmp_path / f"c{k}_{rot}_{len(ap)}_{n_sel}"), st, cols, **ap)
                what = (w, h, rot, ap)
                assert sel.tobytes() == s["sel"].tobytes(), what
                assert et.tobytes() == s["et"].tobytes(), what
                _same_state(got, want, what)
                n_sel += int(s["sel"].sum()); n_not += int((~s["sel"]).sum())
    assert n_sel > 100 and n_not > 100, (n_sel, n_not)


# ---- the oracle's frames of the parity scene --------------------------------------------------------------------------------------------
PARITY = dict(w=76, h=44, spp=4, max_depth=8)   # half tiles on both axes: 10 x 6 = 60 tiles
# The threshold of the PT_FLAG_NEE passes.  With NEE 0.05 leaves 31, 28, 28, 28 of 60 tiles and the selected set soon stops changing; picked by
# test_the_parity_sequence_is_honest's check on the oracle, which holds it to the same condition as the plain estimator's 0.05.
NEE_THRESHOLD = 0.035
_frames_cache = {}


def _oracle_frames(pt, orc, nee, frames=12, scene="cornell", w=PARITY["w"], h=PARITY["h"], spp=PARITY["spp"], max_depth=PARITY["max_depth"], cam=None, faces=None):
    """-> (the frames' colours, their per-pixel ray counts), computed once per argument set and shared"""
    key = (nee, frames, scene, w, h, spp, max_depth, None if faces is None else np.asarray(faces, f32).tobytes())
    if key not in _frames_cache:
        osc = test_aov._oracle_scene(pt, orc, scene, faces)
        cols, maps = [], []
        for k in range(frames):
            rm = np.zeros((h, w), np.uint32)
            col = osc.render_frame(orc.default_params(frame=k, width=w, height=h, spp_per_frame=spp, max_depth=max_depth, **(cam or {}), **(dict(nee=1) if nee else {})), ray_map=rm)[0]
            cols.append(col); maps.append(rm)
        _frames_cache[key] = (cols, maps)
    return _frames_cache[key]


def _parity_calls(nee):
    """(first frame, frames, adaptive parameters) of the sequence: one call of 4 frames, then four passes of 2"""
    ap = dict(threshold=NEE_THRESHOLD if nee else 0.05, min_frames=4, rel_floor=0.01)
    return [(0, 4, ap)] + [(4 + 2 * k, 2, ap) for k in range(4)]


@pytest.mark.parametrize("nee", [False, True], ids=["plain", "nee"])
def test_the_parity_sequence_is_honest(pt, orc, nee):
    """What keeps the rendered-parity test honest, on the oracle: in each of the four passes the reference selects more than 1/4 and fewer
    than 3/4 of the 60 tiles, and the selected set changes at least once."""
    cols, maps = _oracle_frames(pt, orc, nee)
    st = _State(PARITY["w"], PARITY["h"])
    sets = []
    for f0, n, ap in _parity_calls(nee):
        s, _ = _adaptive_ref(st, cols[f0:f0 + n], maps[f0:f0 + n], **ap)
        sets.append(s["sel"].copy())
    counts = [int(x.sum()) for x in sets]
    print("tiles selected per call:", counts)
    assert counts[0] == 60 and all(15 < c < 45 for c in counts[1:]), counts
    assert any((a != b).any() for a, b in zip(sets[1:], sets[2:])), counts


QUALITY = dict(w=76, h=44, spp=4, frames=40, ref_frames=128, ref_spp=32)   # the reference: 4 096 spp against at most 160 in the compared films


def test_quality_on_the_oracle_is_recorded(pt, orc):
    """The experiment of DESIGN.md section 19, without a pass / fail ratio: relative MSE against a converged reference of the adaptive film
    (passes of 2 frames after 4 initial ones, until 40 frames or nothing is selected) and of the uniform film at the nearest equal ray count,
    for both estimators.  Prints what comes out; asserts only that both films are finite and that adaptive traced fewer rays than 40 uniform
    frames."""
    q = QUALITY
    refs = {}
    for nee, thr in ((False, 0.05), (True, NEE_THRESHOLD), (True, 0.05)):
        if nee not in refs:
            osc = test_aov._oracle_scene(pt, orc, "cornell")
            ex = dict(nee=1) if nee else {}
            refs[nee] = np.zeros((q["h"], q["w"], 3), np.float64)
            for k in range(q["ref_frames"]):
                refs[nee] += osc.render_frame(orc.default_params(frame=1000 + k, width=q["w"], height=q["h"], spp_per_frame=q["ref_spp"], max_depth=8, **ex))[0]
            refs[nee] /= q["ref_frames"]
        ref = refs[nee]
        cols, maps = _oracle_frames(pt, orc, nee, frames=q["frames"])
        st = _State(q["w"], q["h"])
        rays, f = _adaptive_ref(st, cols[:4], maps[:4], threshold=thr)[1], 4
        while f < q["frames"]:
            s, r = _adaptive_ref(st, cols[f:f + 2], maps[f:f + 2], threshold=thr)
            if s["tiles_selected"] == 0:
                break
            rays += r; f += 2
        uni, urays, uf = _State(q["w"], q["h"]), 0, 0
        everything = np.ones((q["h"], q["w"]), bool)
        while uf < q["frames"] and urays + int(maps[uf].sum()) // 2 < rays:   # the uniform film whose ray count is nearest
            _blend_ref(uni, cols[uf], everything)
            urays += int(maps[uf].sum()); uf += 1

        def rel_mse(x):
            return float((((x.astype(np.float64) - ref) ** 2) / (ref ** 2 + 1e-2)).mean())
        total = sum(int(m.sum()) for m in maps)
        print(f"nee={int(nee)} threshold={thr}: adaptive {rays} rays in {f} frames rel. MSE {rel_mse(st.C):.5f}; uniform {urays} rays in {uf} frames "
              f"rel. MSE {rel_mse(uni.C):.5f}; 40 uniform frames {total} rays; worst tile error left {float(_select_ref(st.C, st.M, st.K)['et'].max()):.4f}")
        assert np.isfinite(st.C).all() and np.isfinite(uni.C).all() and rays < total


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------
def _film(pt, ctx, w, h):
    film = pt.Film(ctx, w, h)
    film.enable_moments()
    film.enable_counts()
    return film


def _read_state(film):
    st = _State(1, 1)
    st.C, st.M, st.K, st.bgra = film.read_f32(), film.read_moments()[0], film.read_counts(), film.read_bgra8()
    return st


def _same_result(res, s, what):
    got = (res.tiles_total, res.tiles_selected, res.pixels_selected, f32(res.max_error).tobytes())
    want = (s["tiles_total"], s["tiles_selected"], s["pixels_selected"], f32(s["max_error"]).tobytes())
    assert got == want, (what, got, want, res.max_error, s["max_error"])
    assert list(res.reserved) == [0, 0] and res.select_ms >= 0


def _run_sequence(pt, ctx, scene, film, want, calls, cols, maps, what, rank=0, world=1, **kw):
    """every call of `calls` on the device and through the reference; after each: the four planes, the result record, rays and paths"""
    spp = kw["spp_per_frame"]
    sels = []
    for f0, n, ap in calls:
        ctx.reset_stats()
        res = pt.render_adaptive(scene, film, pt.default_params(frame=f0, frame_count=n, rank=rank, world=world, **kw), **ap)
        st = ctx.stats()
        s, rays = _adaptive_ref(want, cols[f0:f0 + n], maps[f0:f0 + n], rank=rank, world=world, **ap)
        w_ = (what, f0, n)
        _same_result(res, s, w_)
        _same_state(_read_state(film), want, w_)
        assert st.rays == rays, (w_, st.rays, rays)
        assert st.paths == s["pixels_selected"] * spp * n, (w_, st.paths)
        sels.append(s)
    return sels


PIPES = [("WAVEFRONT", False), ("FUSED", False), ("AUTO", False), ("WAVEFRONT", True), ("FUSED", True), ("AUTO", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline,nee", PIPES, ids=[p.lower() + ("_nee" if n else "") for p, n in PIPES])
def test_adaptive_rendered_parity(pt, orc, gpu_ctx, cornell_gpu, pipeline, nee):
    """Cornell box, 76 x 44, 4 spp, depth 8: one call of 4 frames, then four passes of 2 frames.  After every call C, M, K, bgra8, the result
    and the growth of rays / paths equal the oracle's frames fed through `_adaptive_ref` (test_the_parity_sequence_is_honest holds the
    sequence to selecting between 1/4 and 3/4 of the tiles, with a set that changes)."""
    cols, maps = _oracle_frames(pt, orc, nee)
    kw = dict(width=PARITY["w"], height=PARITY["h"], spp_per_frame=PARITY["spp"], max_depth=PARITY["max_depth"], pipeline=getattr(pt, "PIPELINE_" + pipeline),
              flags=pt.FLAG_NEE if nee else 0)
    film = _film(pt, gpu_ctx, PARITY["w"], PARITY["h"])
    try:
        sels = _run_sequence(pt, gpu_ctx, cornell_gpu, film, _State(PARITY["w"], PARITY["h"]), _parity_calls(nee), cols, maps, (pipeline, nee), **kw)
        assert all(15 < s["tiles_selected"] < 45 for s in sels[1:])
        want_pipe = {"WAVEFRONT": pt.PIPELINE_WAVEFRONT_NEE if nee else pt.PIPELINE_WAVEFRONT}.get(pipeline, pt.PIPELINE_FUSED)
        assert gpu_ctx.stats().pipeline == want_pipe
    finally:
        film.close()


# (pipeline, name, parameters, tuning): the NEE pipeline runs one sample group; head + tail slots are the fused pipeline's
DEGENERATE = [(p, "plain", {}, {}) for p in ("WAVEFRONT", "WAVEFRONT_NEE", "FUSED", "AUTO")] + \
             [(p, "groups2", dict(sample_groups=2), {}) for p in ("WAVEFRONT", "FUSED", "AUTO")] + \
             [("FUSED", "head_tail", dict(frames_in_flight=2), dict(fused_tail=3))]


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline,name,extra,tuning", DEGENERATE, ids=[f"{d[0].lower()}_{d[1]}" for d in DEGENERATE])
def test_adaptive_with_every_tile_selected_is_pt_render(pt, gpu_ctx, cornell_gpu, pipeline, name, extra, tuning):
    """min_frames above the total frame count selects every tile in every call: with frames 0, 1, 2, ... in calls of 1 and of 3 frames the
    film, M, bgra8 and the rays are pt_render's on a second film -- on every pipeline, with two sample groups (the log replay) and at the
    shape where the fused path plans head + tail slots (tail_samples > 0 asserted)."""
    w, h = 52, 36
    kw = dict(width=w, height=h, spp_per_frame=8, max_depth=6, pipeline=getattr(pt, "PIPELINE_" + pipeline), **extra)
    old = gpu_ctx.set_tuning(**tuning)
    film, plain = _film(pt, gpu_ctx, w, h), pt.Film(gpu_ctx, w, h)
    try:
        plain.enable_moments()
        for f0, n in ((0, 1), (1, 3), (4, 1), (5, 3)):
            gpu_ctx.reset_stats()
            res = pt.render_adaptive(cornell_gpu, film, pt.default_params(frame=f0, frame_count=n, **kw), min_frames=100)
            st = gpu_ctx.stats()
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, plain, pt.default_params(frame=f0, frame_count=n, **kw))
            sp = gpu_ctx.stats()
            what = (pipeline, name, f0, n)
            assert res.tiles_selected == res.tiles_total == 35 and res.pixels_selected == w * h, what
            assert (st.rays, st.paths, st.pipeline, st.tail_samples, st.sample_groups) == (sp.rays, sp.paths, sp.pipeline, sp.tail_samples, sp.sample_groups), what
            if name == "head_tail":
                assert st.tail_samples > 0, what
            if name == "groups2":
                assert st.sample_groups == 2, what
            got = _read_state(film)
            assert got.C.tobytes() == plain.read_f32().tobytes() and got.M.tobytes() == plain.read_moments()[0].tobytes(), what
            assert got.bgra.tobytes() == plain.read_bgra8().tobytes() and (got.K == f32(f0 + n)).all(), what
    finally:
        film.close(); plain.close()
        gpu_ctx.set_tuning(**old)


@pytest.mark.gpu
def test_adaptive_selection_alone_on_synthetic_planes(pt, gpu_ctx, cornell_gpu):
    """The selection over planes in caller memory (torch tensors), as dry runs (frame_count = 0): the result record equals the reference's
    on 8 x 8, 9 x 9 and 76 x 44 films, over every kind of tile (noisy, misses, short through one K = 1, capped, denormal variances, quiet),
    at the default threshold, at 0, at a tile's own e_T and just below it, with and without max_frames -- and nothing is written.  Then one
    frame for real on the largest film: K advances by one on exactly the reference's selected pixels and no other pixel moves in any plane."""
    torch = pytest.importorskip("torch")
    for (w, h) in ((8, 8), (9, 9), (76, 44)):
        for rot in range(len(KINDS) if w * h <= 81 else 2):
            st, _ = _edge_planes(w, h, seed=w + rot, rot=rot)
            tC, tM, tK = (torch.from_numpy(x.copy()).to("cuda:0") for x in (st.C, st.M, st.K))
            film = pt.Film(gpu_ctx, w, h, device_ptr=tC.data_ptr())
            try:
                film.enable_moments(tM.data_ptr())
                film.enable_counts(tK.data_ptr())
                tC.copy_(torch.from_numpy(st.C)); tM.copy_(torch.from_numpy(st.M)); tK.copy_(torch.from_numpy(st.K))   # (enabling zeroed them)
                torch.cuda.synchronize()
                st.bgra[:] = 0
                s0 = _select_ref(st.C, st.M, st.K, **DEFAULTS)
                ok = ~s0["short"] & ~s0["capped"] & (s0["et"] > 0)
                thr = [0.05, 0.0] + ([float(s0["et"][ok].max()), float(np.nextafter(s0["et"][ok].max(), f32(0)))] if ok.any() else [])
                kw = dict(width=w, height=h, spp_per_frame=2, max_depth=3)
                for pipeline in (pt.PIPELINE_WAVEFRONT, pt.PIPELINE_AUTO):
                    for t in thr:
                        for mx in (0, EDGE_MAX_FRAMES):
                            gpu_ctx.reset_stats()
                            res = pt.render_adaptive(cornell_gpu, film, pt.default_params(frame=9, frame_count=0, pipeline=pipeline, **kw), threshold=t, max_frames=mx)
                            _same_result(res, _select_ref(st.C, st.M, st.K, **{**DEFAULTS, "threshold": t, "max_frames": mx}), (w, h, rot, t, mx))
                            assert gpu_ctx.stats().rays == 0 and gpu_ctx.stats().paths == 0
                _same_state(_read_state(film), st, ("dry runs write nothing", w, h, rot))
                if (w, h) == (76, 44):
                    res = pt.render_adaptive(cornell_gpu, film, pt.default_params(frame=9, frame_count=1, pipeline=pt.PIPELINE_AUTO, **kw), max_frames=EDGE_MAX_FRAMES)
                    s = _select_ref(st.C, st.M, st.K, **{**DEFAULTS, "max_frames": EDGE_MAX_FRAMES})
                    _same_result(res, s, "one frame")
                    got = _read_state(film)
                    assert got.K.tobytes() == (st.K + s["mask"].astype(f32)).tobytes()
                    for name in ("C", "M", "bgra"):
                        assert getattr(got, name)[~s["mask"]].tobytes() == getattr(st, name)[~s["mask"]].tobytes(), name
                    assert 0 < s["tiles_selected"] < s["tiles_total"]
            finally:
                film.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["WAVEFRONT", "AUTO"])
def test_adaptive_world_two_on_one_device(pt, orc, gpu_ctx, cornell_gpu, pipeline):
    """World 2: ranks 0 and 1 render into one film, each over its own checkerboard of tiles; every call equals the reference of its rank."""
    cols, maps = _oracle_frames(pt, orc, False)
    kw = dict(width=PARITY["w"], height=PARITY["h"], spp_per_frame=PARITY["spp"], max_depth=PARITY["max_depth"], pipeline=getattr(pt, "PIPELINE_" + pipeline))
    film = _film(pt, gpu_ctx, PARITY["w"], PARITY["h"])
    want = _State(PARITY["w"], PARITY["h"])
    try:
        for f0, n, ap in _parity_calls(False)[:3]:
            for rank in (0, 1):
                s = _run_sequence(pt, gpu_ctx, cornell_gpu, film, want, [(f0, n, ap)], cols, maps, (pipeline, "rank", rank), rank=rank, world=2, **kw)[0]
                assert s["tiles_total"] == 30
    finally:
        film.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["WAVEFRONT", "FUSED", "AUTO"])
def test_adaptive_instanced_scene(pt, orc, gpu_ctx, pipeline):
    """A small instanced scene (the 16-instance grid of the guide tests): 3 frames, then two passes of 2 at a threshold that splits the tiles."""
    scene, w, h, spp, cam = test_denoise.CASES["grid16"]
    cols, maps = _oracle_frames(pt, orc, False, frames=7, scene=scene, w=w, h=h, spp=spp, max_depth=4, cam=cam)
    kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=4, pipeline=getattr(pt, "PIPELINE_" + pipeline), **cam)
    film = _film(pt, gpu_ctx, w, h)
    try:
        ap = dict(threshold=0.1, min_frames=3)
        sels = _run_sequence(pt, gpu_ctx, test_denoise._scene(pt, gpu_ctx, scene), film, _State(w, h), [(0, 3, ap), (3, 2, ap), (5, 2, ap)], cols, maps, pipeline, **kw)
        assert 0 < sels[1]["tiles_selected"] < sels[1]["tiles_total"], sels[1]["tiles_selected"]
    finally:
        film.close()


@pytest.mark.gpu
def test_adaptive_nothing_selected_and_max_frames(pt, orc, gpu_ctx, cornell_gpu):
    """A threshold no tile exceeds: tiles_selected == 0, PT_OK, no launch after the selection (no rays, no paths, no render launches) and no
    plane moves.  max_frames = 6 after six frames stops every tile whatever its error; max_frames = 8 lets them all go on."""
    cols, maps = _oracle_frames(pt, orc, False)
    kw = dict(width=PARITY["w"], height=PARITY["h"], spp_per_frame=PARITY["spp"], max_depth=PARITY["max_depth"], pipeline=pt.PIPELINE_AUTO)
    film = _film(pt, gpu_ctx, PARITY["w"], PARITY["h"])
    want = _State(PARITY["w"], PARITY["h"])
    try:
        _run_sequence(pt, gpu_ctx, cornell_gpu, film, want, [(0, 6, dict(min_frames=6))], cols, maps, "fill", **kw)
        for ap in (dict(threshold=1e9), dict(threshold=0.0, max_frames=6)):
            s = _run_sequence(pt, gpu_ctx, cornell_gpu, film, want, [(6, 2, ap)], cols, maps, ap, **kw)[0]
            st = gpu_ctx.stats()
            assert s["tiles_selected"] == 0 and (st.launches_extend, st.launches_shade, st.launches_other, st.rounds) == (0, 0, 0, 0), ap
        s1 = _run_sequence(pt, gpu_ctx, cornell_gpu, film, want, [(6, 2, dict(threshold=0.0, max_frames=8))], cols, maps, "max 8", **kw)[0]
        assert s1["tiles_selected"] > 15 and (want.K[s1["mask"]] == 8).all() and (want.K[~s1["mask"]] == 6).all()
        s2 = _run_sequence(pt, gpu_ctx, cornell_gpu, film, want, [(8, 2, dict(threshold=0.0, max_frames=8))], cols, maps, "max 8 again", **kw)[0]
        assert (s2["capped"] == s1["sel"]).all() and s2["tiles_selected"] == 0   # (the others are tiles of misses: e_T = 0)
    finally:
        film.close()


@pytest.mark.gpu
def test_adaptive_redo_blends_once(pt, orc, gpu_ctx, cornell_arrays):
    """Every surface emits, so every ray logs a term: with a pool of three entries a batch overflows its term logs and is rendered again with
    one group (pt_tuning.term_ocap / term_spill, as the overflow tests force it).  The film is blended once and K advances once, on both
    pipelines, over a selection that is a true subset."""
    w, h, spp = 52, 36, 8
    v, i, f = cornell_arrays
    f = f.reshape(-1, 6).copy()
    f[:, 3:] = f32(0.25) + f[:, :3] * f32(0.5)
    cols, maps = _oracle_frames(pt, orc, False, frames=7, w=w, h=h, spp=spp, max_depth=12, faces=f.reshape(-1))
    gs = pt.Scene(gpu_ctx, v, i, f.reshape(-1))
    try:
        for tuning, shape in ((dict(term_ocap=0, term_spill=3), dict(pipeline=pt.PIPELINE_WAVEFRONT, sample_groups=4, frames_in_flight=2)),
                              (dict(term_ocap=0, term_spill=3, fused_tail=4), dict(pipeline=pt.PIPELINE_FUSED, frames_in_flight=2))):
            old = gpu_ctx.set_tuning(**tuning)
            film = _film(pt, gpu_ctx, w, h)
            try:
                s0 = _select_ref(*[getattr(_warm(cols), n) for n in ("C", "M", "K")], **DEFAULTS)
                thr = float(np.sort(s0["et"])[len(s0["et"]) // 2])   # the median tile error after four frames: about half of the tiles go on
                ap = dict(threshold=thr)
                want = _State(w, h)
                kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=12, **shape)
                redone = 0
                for call in ((0, 4, ap), (4, 3, ap)):
                    s = _run_sequence(pt, gpu_ctx, gs, film, want, [call], cols, maps, (tuning, call), **kw)[0]
                    redone += gpu_ctx.stats().redone_batches
                assert 0 < s["tiles_selected"] < s["tiles_total"] and redone > 0, (s["tiles_selected"], redone)
            finally:
                film.close()
                gpu_ctx.set_tuning(**old)
    finally:
        gs.close()


def _warm(cols):
    """the state after the first four frames everywhere"""
    h, w, _ = cols[0].shape
    st = _State(w, h)
    for c in cols[:4]:
        _blend_ref(st, c, np.ones((h, w), bool))
    return st


@pytest.mark.gpu
def test_adaptive_refusals_leave_every_plane_untouched(pt, orc, gpu_ctx, cornell_gpu):
    """Every refusal of the header: PT_ERR_INVALID_ARG (NULL arguments, a film without M or without K, a size mismatch, out-of-range fields,
    a nonzero reserved word) and PT_ERR_UNSUPPORTED (PT_FLAG_ASYNC, _PROFILE, _COUNT_VISITS), with nothing written."""
    cols, maps = _oracle_frames(pt, orc, False)
    w, h = PARITY["w"], PARITY["h"]
    kw = dict(width=w, height=h, spp_per_frame=PARITY["spp"], max_depth=PARITY["max_depth"], pipeline=pt.PIPELINE_AUTO)
    film = _film(pt, gpu_ctx, w, h)
    bare, only_m, only_k = pt.Film(gpu_ctx, w, h), pt.Film(gpu_ctx, w, h), pt.Film(gpu_ctx, w, h)
    lib = pt.lib_amd()
    try:
        only_m.enable_moments(); only_k.enable_counts()
        with pytest.raises(pt.PtError):
            film.enable_counts()   # once per film
        with pytest.raises(pt.PtError):
            bare.read_counts()
        want = _State(w, h)
        _run_sequence(pt, gpu_ctx, cornell_gpu, film, want, [(0, 4, {})], cols, maps, "fill", **kw)
        p, ap = pt.default_params(frame=4, frame_count=2, **kw), pt.adaptive_default_params()
        gpu_ctx.reset_stats()
        for args in ((None, film.h, p, ap), (cornell_gpu.h, None, p, ap), (cornell_gpu.h, film.h, None, ap), (cornell_gpu.h, film.h, p, None)):
            a = [C.byref(x) if isinstance(x, C.Structure) else x for x in args]
            assert lib.pt_render_adaptive(a[0], a[1], a[2], a[3], None) == 1
        for other in (bare, only_m, only_k):
            with pytest.raises(pt.PtError, match="plane"):
                pt.render_adaptive(cornell_gpu, other, p)
            assert not other.read_f32().any() and not other.read_bgra8().any()
        bad = [dict(threshold=-0.01), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(rel_floor=0.0), dict(rel_floor=-1.0),
               dict(rel_floor=float("nan")), dict(rel_floor=float("inf")), dict(min_frames=1), dict(min_frames=0), dict(min_frames=65536)]
        for b in bad:
            with pytest.raises(pt.PtError):
                pt.render_adaptive(cornell_gpu, film, p, **b)
        for k in range(4):
            r = pt.adaptive_default_params()
            r.reserved[k] = 1
            with pytest.raises(pt.PtError, match="reserved"):
                pt.render_adaptive(cornell_gpu, film, p, adaptive_params=r)
        for size in (dict(width=w + 1), dict(height=h - 1)):
            with pytest.raises(pt.PtError, match="film"):
                pt.render_adaptive(cornell_gpu, film, pt.default_params(frame=4, frame_count=2, **{**kw, **size}))
        for flag in (pt.FLAG_ASYNC, pt.FLAG_PROFILE, pt.FLAG_COUNT_VISITS):
            for pipeline in (pt.PIPELINE_WAVEFRONT, pt.PIPELINE_AUTO):
                rc = lib.pt_render_adaptive(cornell_gpu.h, film.h, C.byref(pt.default_params(frame=4, frame_count=2, **{**kw, "pipeline": pipeline, "flags": flag})), C.byref(ap), None)
                assert rc == 5, (flag, pipeline, rc)   # PT_ERR_UNSUPPORTED
        assert gpu_ctx.stats().rays == 0
        _same_state(_read_state(film), want, "after the refusals")
        pt.render_adaptive(cornell_gpu, film, p, threshold=0.0, min_frames=65535)   # (the ends of the ranges are accepted)
    finally:
        for x in (film, bare, only_m, only_k):
            x.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["WAVEFRONT", "AUTO"])
def test_pt_render_without_counts_is_unchanged(pt, orc, cornell_arrays, pipeline):
    """pt_render on a film without K, in a context that never renders adaptively, against one whose other film does: film, bgra8, rays and
    workspace_bytes are equal, and equal the oracle's."""
    cols, maps = _oracle_frames(pt, orc, False)
    w, h = PARITY["w"], PARITY["h"]
    kw = dict(width=w, height=h, spp_per_frame=PARITY["spp"], max_depth=PARITY["max_depth"], pipeline=getattr(pt, "PIPELINE_" + pipeline))
    out = []
    for adaptive_first in (False, True):
        ctx = pt.Context(0)
        sc = pt.Scene(ctx, *cornell_arrays)
        film = pt.Film(ctx, w, h)
        try:
            if adaptive_first:
                other = _film(pt, ctx, w, h)
                pt.render_adaptive(sc, other, pt.default_params(frame=0, frame_count=2, **kw))
                other.close()
            ctx.reset_stats()
            pt.render(sc, film, pt.default_params(frame=0, frame_count=3, **kw))
            st = ctx.stats()
            out.append((film.read_f32().tobytes(), film.read_bgra8().tobytes(), st.rays, st.paths, st.workspace_bytes))
        finally:
            film.close(); sc.close(); ctx.close()
    assert out[0] == out[1], (out[0][2:], out[1][2:])
    want = _State(w, h)
    for c in cols[:3]:
        _blend_ref(want, c, np.ones((h, w), bool))
    assert out[0][0] == want.C.tobytes() and out[0][1] == want.bgra.tobytes() and out[0][2] == sum(int(m.sum()) for m in maps[:3])


@pytest.mark.gpu
def test_pt_main_adaptive(pt, orc, tmp_path):
    """pt_main --adaptive T --steps 2 --passes 3 writes the film of the Python loop -- a dry run, then a pass of 2 frames, three times -- which
    is the reference's; one line per pass on stderr with the tiles selected; the JSON line's rays and paths are the passes' together."""
    import json
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_main")
    if not os.path.exists(exe):
        pt.build()
    w, h, spp, depth = PARITY["w"], PARITY["h"], PARITY["spp"], PARITY["max_depth"]
    cols, maps = _oracle_frames(pt, orc, False)
    want, rays, paths, tiles = _State(w, h), 0, 0, []
    for k in range(3):
        s, r = _adaptive_ref(want, cols[2 * k:2 * k + 2], maps[2 * k:2 * k + 2], threshold=0.25, min_frames=2)
        rays += r; paths += s["pixels_selected"] * spp * 2
        tiles.append(s["tiles_selected"])
    assert tiles[0] == 60 and 0 < tiles[2] < 60, tiles
    cmd = [exe, "--obj", pt.ASSET_CORNELL, "--width", str(w), "--height", str(h), "--spp", str(spp), "--depth", str(depth), "--adaptive", "0.25", "--min-frames", "2",
           "--steps", "2", "--passes", "3", "--pfm", str(tmp_path / "a.pfm"), "--ppm", str(tmp_path / "a.ppm")]
    run = subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=pt.REPO, timeout=120)
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert (out["rays"], out["paths"], out["frames"]) == (rays, paths, 6), (out, rays, paths)
    assert [int(l.split(":")[1].split()[0]) for l in run.stderr.splitlines() if l.startswith("pass ")] == tiles, run.stderr
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    raw = open(tmp_path / "a.pfm", "rb").read()
    assert raw.startswith(head) and np.ascontiguousarray(np.frombuffer(raw[len(head):], f32).reshape(h, w, 3)[::-1]).tobytes() == want.C.tobytes()
    ppm_head = f"P6\n{w} {h}\n255\n".encode()
    ppm = open(tmp_path / "a.ppm", "rb").read()
    assert ppm.startswith(ppm_head) and ppm[len(ppm_head):] == np.ascontiguousarray(want.bgra[:, :, 2::-1]).tobytes()
    bad = subprocess.run([exe, "--adaptive", "0.1", "--denoise"], capture_output=True, text=True, cwd=pt.REPO, timeout=120)
    assert bad.returncode != 0 and "--adaptive" in bad.stderr
