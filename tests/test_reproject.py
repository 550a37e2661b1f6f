"""pt_film_reproject: temporal accumulation across camera moves (include/pt_api.h).

`_reproject_ref` is the numpy statement of the header's definition: float32 throughout, every operation written out in the header's order,
vectorised over the image, the four taps gathered at clamped coordinates and dropped by selects in the order j outer / i inner.  The CPU
tests check the value of the step (the experiment of DESIGN.md section 15) and the exact properties of the definition on synthetic planes;
the GPU tests feed `_reproject_ref` what the device's own planes hold, read back before the call.  Every GPU comparison is `tobytes()`
equality on C, M, L and the bgra8 image."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_aov
import test_denoise
from test_denoise import _rel_mse, _to_bgra8

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MATCH_ID = 1
DEFAULT_CAM = dict(cam_origin=(0.0, -1.0, 5.0), cam_target=(0.0, -1.0, 2.0))   # pt_params_default's (raygen.rgen:55-56)


def _cam(cam=None, move=(0.0, 0.0, 0.0), k=1):
    """the camera `cam` (a dict as default_params takes it, missing keys are the defaults) with origin and target moved k times by `move`"""
    c = {**DEFAULT_CAM, **(cam or {})}
    mv = np.asarray(move, f32) * f32(k)
    return {n: tuple(float(v) for v in (np.asarray(c[n], f32) + mv)) for n in ("cam_origin", "cam_target")}


def _reproject_ref(cur, prev, cam=None, prev_cam=None, gain=1.0, alpha=0.2, depth_tol=0.1, normal_min=0.9, max_history=32, flags=MATCH_ID, parts=None):
    """-> {"C", "M" (if cur has it), "L", "bgra"}.  cur: {"C" [H, W, 3], "M" [H, W, 3] or absent, "N" [H, W, 3], "Z" [H, W], "a" [H, W],
    "ID" uint32 [H, W, 2]} as stored; prev: the same plus "L" [H, W], or None (every pixel takes the no-history path).  parts (a dict):
    receives "hist" (pixels that blended), "subset" (bit 2 j + i: tap (i, j) counted), "x0", "y0", "fx", "fy", "front", "inside" and
    "reject" ({term: taps inside the image that this term alone rejected})."""
    C_ = np.ascontiguousarray(cur["C"], f32)
    h, w = C_.shape[:2]
    has_m = cur.get("M") is not None
    g = f32(gain)
    Cc = C_ * g
    out = {"C": Cc.copy(), "L": np.ones((h, w), f32)}
    assert Cc.dtype == f32
    if has_m:
        Mc = np.ascontiguousarray(cur["M"], f32) * g
        out["M"] = Mc.copy()
    if prev is None:
        out["bgra"] = _to_bgra8(out["C"])
        if parts is not None:
            parts["hist"] = np.zeros((h, w), bool)
        return out
    assert has_m == (prev.get("M") is not None)
    N, Z, a, ID = np.ascontiguousarray(cur["N"], f32), np.ascontiguousarray(cur["Z"], f32), np.ascontiguousarray(cur["a"], f32), np.ascontiguousarray(cur["ID"], np.uint32)
    pC, pN, pZ, pa, pL = (np.ascontiguousarray(prev[k], f32) for k in ("C", "N", "Z", "a", "L"))
    pID = np.ascontiguousarray(prev["ID"], np.uint32)
    pM = np.ascontiguousarray(prev["M"], f32) if has_m else None
    assert all(x.dtype == f32 for x in (N, Z, a, pC, pN, pZ, pa, pL))
    cam, prev_cam = _cam(cam), _cam(prev_cam)
    o, t = np.asarray(cam["cam_origin"], f32), np.asarray(cam["cam_target"], f32)
    po, pt_ = np.asarray(prev_cam["cam_origin"], f32), np.asarray(prev_cam["cam_target"], f32)
    wf, hf, one, half, two = f32(w), f32(h), f32(1.0), f32(0.5), f32(2.0)
    with np.errstate(all="ignore"):   # (a miss divides by a = 0; every such lane is dropped by a select below)
        depth = Z / a
        qx = (np.arange(w, dtype=f32) + half) / wf
        qy = (np.arange(h, dtype=f32) + half) / hf
        vx = (((qx * two - one) + t[0]) - o[0])[None, :]
        vy = (((qy * two - one) + t[1]) - o[1])[:, None]
        vz = t[2] - o[2]
        ln = np.sqrt((vx * vx + vy * vy) + vz * vz)
        Px, Py, Pz = o[0] + (vx / ln) * depth, o[1] + (vy / ln) * depth, o[2] + (vz / ln) * depth
        ux, uy, uz = Px - po[0], Py - po[1], Pz - po[2]
        vzp = pt_[2] - po[2]
        assert all(x.dtype == f32 and x.shape == (h, w) for x in (depth, ln, Px, Py, Pz, ux, uy, uz)) and vzp.dtype == f32
        front = (a > 0) & (uz * vzp > 0)
        s = vzp / uz
        ex, ey = (ux * s + po[0]) - pt_[0], (uy * s + po[1]) - pt_[1]
        fx, fy = ((ex + one) * half) * wf - half, ((ey + one) * half) * hf - half
        inside = front & (fx > -one) & (fx < wf) & (fy > -one) & (fy < hf)
        x0f, y0f = np.floor(fx), np.floor(fy)
        bx, by = fx - x0f, fy - y0f
        d = np.sqrt((ux * ux + uy * uy) + uz * uz)
        assert all(x.dtype == f32 for x in (s, ex, ey, fx, fy, bx, by, d))
        x0 = np.where(inside, x0f, 0).astype(np.int64)
        y0 = np.where(inside, y0f, 0).astype(np.int64)
        W = np.zeros((h, w), f32)
        Ch = np.zeros((h, w, 3), f32)
        Mh = np.zeros((h, w, 3), f32)
        Lh = np.zeros((h, w), f32)
        subset = np.zeros((h, w), np.uint8)
        reject = {k: 0 for k in ("alpha", "history", "weight", "id", "depth", "normal")}
        for j in (0, 1):
            for i in (0, 1):
                tx, ty = x0 + i, y0 + j
                in_img = inside & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                cx, cy = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
                wq = (bx if i else one - bx) * (by if j else one - by)
                aq, Lq, Zq, Nq = pa[cy, cx], pL[cy, cx], pZ[cy, cx], pN[cy, cx]
                terms = {"alpha": aq > 0, "history": Lq > 0, "weight": wq > 0,
                         "id": (pID[cy, cx] == ID).all(axis=2) if flags & MATCH_ID else np.ones((h, w), bool),
                         "depth": np.abs(Zq - d * aq) <= (f32(depth_tol) * d) * aq,
                         "normal": ((N[:, :, 0] * Nq[:, :, 0] + N[:, :, 1] * Nq[:, :, 1]) + N[:, :, 2] * Nq[:, :, 2]) >= f32(normal_min) * (a * aq)}
                valid = in_img.copy()
                for v in terms.values():
                    valid &= v
                for k in terms:
                    others = in_img.copy()
                    for k2, v in terms.items():
                        if k2 != k:
                            others &= v
                    reject[k] += int((others & ~terms[k]).sum())
                assert wq.dtype == f32
                W = np.where(valid, W + wq, W)
                Ch = np.where(valid[:, :, None], Ch + wq[:, :, None] * pC[cy, cx], Ch)
                if has_m:
                    Mh = np.where(valid[:, :, None], Mh + wq[:, :, None] * pM[cy, cx], Mh)
                Lh = np.where(valid, Lh + wq * Lq, Lh)
                subset |= (valid.astype(np.uint8) << np.uint8(2 * j + i))
        hist = inside & (W >= f32(0.01))
        Ch = Ch / W[:, :, None]
        Mh = Mh / W[:, :, None]
        Lh = np.minimum(Lh / W, f32(max_history))
        al = np.maximum(f32(alpha), one / (Lh + one))
        Cn = Ch + al[:, :, None] * (Cc - Ch)
        assert all(x.dtype == f32 for x in (W, Ch, Mh, Lh, al, Cn))
        out["C"] = np.where(hist[:, :, None], Cn, Cc)
        if has_m:
            Mn = Mh + al[:, :, None] * (Mc - Mh)
            assert Mn.dtype == f32
            out["M"] = np.where(hist[:, :, None], Mn, Mc)
        out["L"] = np.where(hist, Lh + one, one)
    assert out["C"].dtype == f32 and out["L"].dtype == f32
    out["bgra"] = _to_bgra8(out["C"])
    if parts is not None:
        parts.update(hist=hist, subset=np.where(hist, subset, 0).astype(np.uint8), x0=x0, y0=y0, fx=fx, fy=fy, front=front, inside=inside, reject=reject)
    return out


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
FIELDS = ["cam_origin", "cam_target", "prev_cam_origin", "prev_cam_target", "gain", "alpha", "depth_tol", "normal_min", "max_history", "flags", "reserved"]
NEW_SYMBOLS = ["pt_film_enable_history", "pt_film_read_history", "pt_reproject_params_default", "pt_film_reproject"]


def test_reproject_params_layout_defaults_and_symbols(pt, tmp_path):
    """sizeof / offsetof of pt_reproject_params by gcc from the header == the ctypes mirror (88 bytes); the defaults; the names in
    API_SYMBOLS and in the library; PT_API_VERSION stays 6."""
    src = tmp_path / "rp_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("%zu ' + "%zu " * len(FIELDS) + '%d %u\\n",'
                   "sizeof(pt_reproject_params), " + ", ".join(f"offsetof(pt_reproject_params, {n})" for n in FIELDS) +
                   ", PT_API_VERSION, (unsigned)PT_REPROJECT_MATCH_ID);return 0;}\n")
    exe = tmp_path / "rp_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = pt.ReprojectParams
    assert got == [C.sizeof(P)] + [getattr(P, n).offset for n in FIELDS] + [6, pt.REPROJECT_MATCH_ID], got
    assert got[0] == 88 and pt.REPROJECT_MATCH_ID == 1
    for name in NEW_SYMBOLS:
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    assert "ReprojectParams" in dir(pt._mod) and "reproject_default_params" in dir(pt._mod)   # (the fifth name: the Python mirror itself)
    p = pt.reproject_default_params()   # (touches no device)
    assert (p.gain, p.alpha, p.depth_tol, p.normal_min, p.max_history, p.flags, list(p.reserved)) == (1.0, f32(0.2), f32(0.1), f32(0.9), 32, 1, [0] * 4)
    assert list(p.cam_origin) == list(p.prev_cam_origin) == [0.0, -1.0, 5.0] and list(p.cam_target) == list(p.prev_cam_target) == [0.0, -1.0, 2.0]


def _oracle_planes(pt, orc, scene, w, h, spp, cam):
    """N, Z, a, ID of frame 0 at `cam`, the way test_aov._guides builds them (oracle bindings only)"""
    osc = test_aov._oracle_scene(pt, orc, scene)
    p = orc.default_params(frame=0, width=w, height=h, spp_per_frame=spp, **cam)
    rays = np.zeros((h, w, spp, 6), f32)
    for y in range(h):
        for x in range(w):
            for s in range(spp):
                o, d, _ = orc.primary_ray(p, x, y, orc.seed(x, y, s, 0, spp))
                rays[y, x, s, :3] = o
                rays[y, x, s, 3:] = d
    hits, _ = osc.trace(rays.reshape(-1, 6), p.tmin, p.tmax)
    hits = hits.reshape(h, w, spp)
    val = np.zeros((h, w, spp, 5), f32)   # normal 0:3, depth 3, alpha 4 -- all 0 on a miss
    normals = {}
    for y, x, s in zip(*np.nonzero(hits["prim"] != test_aov.MISS)):
        hit = hits[y, x, s]
        k = (int(hit["inst"]), int(hit["prim"]))
        if k not in normals:
            normals[k] = osc.shade_hit(hit)[1]
        val[y, x, s, 0:3] = normals[k]
        val[y, x, s, 3] = hit["t"]
        val[y, x, s, 4] = f32(1.0)
    acc = np.zeros((h, w, 5), f32)
    for s in range(spp):
        acc = acc + val[:, :, s]
    value = acc / f32(spp)
    ids = np.zeros((h, w, 2), np.uint32)
    ids[:, :, 0] = hits["prim"][:, :, 0]
    ids[:, :, 1] = np.where(hits["prim"][:, :, 0] == test_aov.MISS, test_aov.MISS, hits["inst"][:, :, 0])
    return {"N": np.ascontiguousarray(value[:, :, 0:3]), "Z": np.ascontiguousarray(value[:, :, 3]), "a": np.ascontiguousarray(value[:, :, 4]), "ID": ids}


# camera step per time step -> r of the assertion `accumulated <= one step / r` (None: printed only).  r is half the measured ratio.
PATHS = [((0.0, 0.0, 0.0), 2.89), ((0.02, 0.0, 0.0), 4.90), ((0.1, 0.0, 0.0), None), ((0.0, 0.0, -0.05), 1.85), ((0.03, 0.02, -0.03), None)]
STEPS = 8


def _experiment(pt, orc, move, steps=STEPS, ref_frames=None):
    """-> (one step's relMSE, accumulated relMSE, share of the covered pixels of the last step that found history)"""
    q = test_denoise.QUALITY
    osc = test_aov._oracle_scene(pt, orc, q["scene"])
    kw = dict(width=q["w"], height=q["h"])
    prev = prev_cam = None
    for k in range(steps):
        cam = _cam(None, move, k)
        c = osc.render_frame(orc.default_params(frame=k, spp_per_frame=q["spp"], **kw, **cam), nthreads=16)[0]
        film = c if k == 0 else (c + np.zeros_like(c) * f32(k)) / f32(k + 1)   # a cleared film after frame k alone: k_resolve's blend
        assert film.dtype == f32
        cur = {"C": film, **_oracle_planes(pt, orc, q["scene"], q["w"], q["h"], q["spp"], cam)}
        parts = {}
        gain = f32(k + 1) / f32(1)
        res = _reproject_ref(cur, prev, cam, prev_cam, gain=gain, parts=parts)
        one_step = film * gain
        prev, prev_cam = {**cur, "C": res["C"], "L": res["L"]}, cam
    ref = np.zeros((q["h"], q["w"], 3), np.float64)
    n_ref = ref_frames or q["ref_frames"]
    for k in range(n_ref):
        ref += osc.render_frame(orc.default_params(frame=1000 + k, spp_per_frame=q["ref_spp"], **kw, **cam), nthreads=16)[0]
    ref /= n_ref
    covered = cur["a"] > 0
    return _rel_mse(one_step, ref), _rel_mse(res["C"], ref), float(parts["hist"][covered].mean())


def test_quality_of_the_accumulated_film(pt, orc):
    """The experiment of DESIGN.md section 15, test_denoise's own set-up: Cornell box 128 x 96, 4 spp per step, 8 steps; step k renders its
    radiance at frame = k into a cleared film (gain = k + 1) and its guides at frame 0, camera origin and target moved by the step each
    time; against the mean of 64 frames of 32 spp (frames 1000..1063) at the last camera; relMSE as test_denoise._rel_mse.  Measured
    (camera step: one step's film / accumulated / ratio / covered pixels that found history):
        none (static)         2.0245 / 0.3502 /  5.78 / 0.957        r = 2.89
        (0.02, 0, 0)          1.7680 / 0.1804 /  9.80 / 0.939        r = 4.90
        (0.1, 0, 0)           1.5607 / 0.2402 /  6.50 / 0.923        (printed)
        (0, 0, -0.05)         2.2355 / 0.6054 /  3.69 / 0.953        r = 1.85
        (0.03, 0.02, -0.03)   2.2189 / 0.2326 /  9.54 / 0.954        (printed)
    (about 20 s of oracle time per path: the 64 reference frames at the path's last camera are most of it.)
    Asserted for the static, (0.02, 0, 0) and (0, 0, -0.05) paths: accumulated <= one step / r with r half the measured ratio (never below
    1.5) -- the margin is for seed and guide choices, as section 14 took -- and at least 0.85 of the covered pixels found history."""
    rows = []
    for move, r in PATHS:
        one, acc, found = _experiment(pt, orc, move)
        rows.append((move, r, one, acc, found))
        print(f"camera step {move}: one step's film {one:.4f}, accumulated {acc:.4f}, ratio {one / acc:.2f}, covered pixels that found history {found:.3f}")
    for move, r, one, acc, found in rows:
        if r is not None:
            assert r >= 1.5
            assert acc <= one / r, (move, one, acc, r)
            assert found >= 0.85, (move, found)


def _wall(h, w, z0=-1.0, cam=None, ids=(7, 0)):
    """the guides a camera at `cam` sees of the wall z = z0 (normal +z, full coverage, one primitive)"""
    cam = _cam(cam)
    o, t = np.asarray(cam["cam_origin"], f32), np.asarray(cam["cam_target"], f32)
    qx = (np.arange(w, dtype=f32) + f32(0.5)) / f32(w)
    qy = (np.arange(h, dtype=f32) + f32(0.5)) / f32(h)
    vx = (((qx * f32(2) - f32(1)) + t[0]) - o[0])[None, :]
    vy = (((qy * f32(2) - f32(1)) + t[1]) - o[1])[:, None]
    vz = t[2] - o[2]
    ln = np.sqrt((vx * vx + vy * vy) + vz * vz)
    Z = (ln * ((f32(z0) - o[2]) / vz)).astype(f32)
    N = np.zeros((h, w, 3), f32)
    N[:, :, 2] = 1.0
    ID = np.zeros((h, w, 2), np.uint32)
    ID[:, :, 0], ID[:, :, 1] = ids
    return {"N": N, "Z": Z, "a": np.ones((h, w), f32), "ID": ID}


def _wall_pair(h, w, seed, cam=None, prev_cam=None, m=True):
    rng = np.random.default_rng(seed)
    cur = {"C": rng.uniform(0, 2, (h, w, 3)).astype(f32), **_wall(h, w, cam=cam)}
    prev = {"C": rng.uniform(0, 2, (h, w, 3)).astype(f32), "L": rng.integers(1, 6, (h, w)).astype(f32), **_wall(h, w, cam=prev_cam)}
    if m:
        cur["M"], prev["M"] = rng.uniform(0, 4, (h, w, 3)).astype(f32), rng.uniform(0, 4, (h, w, 3)).astype(f32)
    return cur, prev


SHAPES = [(1, 1), (2, 3), (40, 5)]


@pytest.mark.parametrize("shape", SHAPES)
def test_no_previous_film_starts_a_sequence(shape):
    h, w = shape
    cur, _ = _wall_pair(h, w, 1)
    res = _reproject_ref(cur, None, gain=3.0)
    assert res["C"].tobytes() == (cur["C"] * f32(3)).tobytes() and res["M"].tobytes() == (cur["M"] * f32(3)).tobytes()
    assert (res["L"] == 1).all() and res["L"].shape == (h, w) and res["bgra"].tobytes() == _to_bgra8(res["C"]).tobytes()


@pytest.mark.parametrize("shape", SHAPES)
def test_static_wall_is_the_running_mean(shape):
    """Both cameras equal, a wall of constant z, alpha = 0, frames of one colour each: every pixel reprojects onto itself up to the rounding of
    the round trip (fx within ~1e-5 of x, so one tap carries all but that much of the weight, and the rest goes to a neighbour that holds the
    same value), L == L' + 1 capped at max_history + 1 and C within 2 ulp of the running mean C' + (Cc - C') / (L' + 1).  L is exact where L'
    is a power of two (the products wq * L' are exact, so the sum is W scaled); (w0 * 3 + w1 * 3) / W need not be 3 to the bit: 2 ulp."""
    h, w = shape
    cap = 3
    rng = np.random.default_rng(4)
    frames = [np.broadcast_to(rng.uniform(0.5, 2, 3).astype(f32), (h, w, 3)).copy() for _ in range(6)]
    prev = None
    with np.errstate(divide="raise", invalid="ignore", over="raise"):
        for k, c in enumerate(frames):
            cur = {"C": c, **_wall(h, w)}
            parts = {}
            res = _reproject_ref(cur, prev, alpha=0.0, max_history=cap, parts=parts)
            if prev is None:
                mean = c
            else:
                assert parts["hist"].all()
                n = np.minimum(prev["L"], f32(cap))
                mean = (prev["C"].astype(np.float64) + (c.astype(np.float64) - prev["C"]) / (n[:, :, None] + 1.0))
                want_l = np.minimum(prev["L"], f32(cap)) + f32(1)
                pow2 = np.isin(prev["L"], (1, 2, 4))
                assert (res["L"][pow2] == want_l[pow2]).all()
                assert (np.abs(res["L"] - np.round(want_l)) <= 2 * np.spacing(want_l)).all(), (k, res["L"])
                assert (np.abs(res["C"] - mean) <= 2 * np.spacing(np.abs(mean).astype(f32))).all(), float(np.abs(res["C"] - mean).max())
            assert (np.round(res["L"]) == min(k, cap) + 1).all(), (k, res["L"])
            prev = {**cur, "C": res["C"], "L": res["L"]}


def test_id_mismatch_takes_the_new_colour_bit_for_bit():
    cur, prev = _wall_pair(12, 16, 2)
    cur["ID"][5, 7] = (99, 0)
    cur["ID"][6, 2] = (7, 1)          # the second word alone
    parts = {}
    res = _reproject_ref(cur, prev, gain=2.0, parts=parts)
    for y, x in ((5, 7), (6, 2)):
        assert not parts["hist"][y, x] and res["L"][y, x] == 1
        assert res["C"][y, x].tobytes() == (cur["C"][y, x] * f32(2)).tobytes() and res["M"][y, x].tobytes() == (cur["M"][y, x] * f32(2)).tobytes()
    assert parts["hist"].sum() == 12 * 16 - 2 and parts["reject"]["id"] > 0
    off = _reproject_ref(cur, prev, gain=2.0, flags=0, parts=parts)
    assert parts["hist"].all() and abs(off["L"][5, 7] - (prev["L"][5, 7] + 1)) < 1e-4
    assert off["C"][5, 7].tobytes() != (cur["C"][5, 7] * f32(2)).tobytes()


def test_points_behind_outside_and_in_the_margin():
    """A previous camera that looks the other way sees every point behind it; one moved far sideways projects every point outside; one
    moved by 1.5 pixels' worth of the wall's parallax puts a column of reprojections into the one-pixel margin, where two taps (one at a
    corner) are inside; a miss takes the no-history path whatever the cameras."""
    h, w = 10, 16
    behind = dict(cam_origin=(0.0, -1.0, -8.0), cam_target=(0.0, -1.0, -11.0))     # beyond the wall z = -1, looking on along -z: u.z > 0, vz' < 0
    cur, prev = _wall_pair(h, w, 3, prev_cam=behind)
    parts = {}
    res = _reproject_ref(cur, prev, None, behind, parts=parts)
    assert not parts["front"].any() and not parts["hist"].any() and res["C"].tobytes() == cur["C"].tobytes() and (res["L"] == 1).all()
    far = _cam(None, (30.0, 0.0, 0.0))
    cur, prev = _wall_pair(h, w, 3, prev_cam=far)
    res = _reproject_ref(cur, prev, None, far, parts=parts)
    assert parts["front"].all() and not parts["inside"].any() and res["C"].tobytes() == cur["C"].tobytes() and (res["L"] == 1).all()
    # the wall is 6 from the origin and the target plane 3: a camera moved by m along x shifts the wall's projection by -m / 2 of the
    # square of side 2, that is by -m / 2 * w / 2 pixels; m = 0.75 at w = 16: 3 pixels, m = 0.3125: 1.25 pixels
    for m, n_margin in ((0.3125, h), (-0.3125, h)):
        pc = _cam(None, (m, 0.0, 0.0))
        cur, prev = _wall_pair(h, w, 5, prev_cam=pc)
        res = _reproject_ref(cur, prev, None, pc, depth_tol=0.5, parts=parts)
        edge = (parts["x0"] == (-1 if m > 0 else w - 1)) & parts["inside"]
        assert edge.sum() >= n_margin, (m, int(edge.sum()))
        # (the camera moved along x only: fy is y up to the round trip's rounding, and a pixel whose by comes out 0 carries one tap)
        got = set(int(v) for v in np.unique(parts["subset"][edge]))
        assert got <= ({0b1010, 0b0010, 0b1000} if m > 0 else {0b0101, 0b0001, 0b0100}) and (0b1010 if m > 0 else 0b0101) in got, got
        # (two taps of the same column, weights by and 1 - by: L is a mean of two of prev's L in 1..5, plus 1)
        assert parts["hist"][edge].all() and (res["L"][edge] >= 2).all() and (res["L"][edge] <= 6).all()
        col = 0 if m > 0 else w - 1
        lo, hi = np.minimum(prev["L"][:-1, col], prev["L"][1:, col]) + 1, np.maximum(prev["L"][:-1, col], prev["L"][1:, col]) + 1
        ys = np.nonzero(edge[1:-1].any(axis=1))[0] + 1
        for y in ys:   # row y's taps are rows y0, y0 + 1 of that column
            y0 = int(parts["y0"][y][edge[y]][0])
            if 0 <= y0 < h - 1:
                assert (res["L"][y][edge[y]] >= lo[y0] - 1e-4).all() and (res["L"][y][edge[y]] <= hi[y0] + 1e-4).all()
    # vertical margin and the corner: one tap
    pc = _cam(None, (0.3125, 0.5, 0.0))
    cur, prev = _wall_pair(h, w, 6, prev_cam=pc)
    res = _reproject_ref(cur, prev, None, pc, depth_tol=0.5, parts=parts)
    corner = parts["inside"] & (parts["x0"] == -1) & (parts["y0"] == -1)
    assert corner.any() and set(np.unique(parts["subset"][corner])) <= {0b1000}
    # misses
    cur, prev = _wall_pair(h, w, 7)
    cur["a"][3, 4] = 0.0
    cur["Z"][3, 4] = 0.0
    cur["N"][3, 4] = 0.0
    res = _reproject_ref(cur, prev, gain=2.0, parts=parts)
    assert not parts["hist"][3, 4] and res["L"][3, 4] == 1 and res["C"][3, 4].tobytes() == (cur["C"][3, 4] * f32(2)).tobytes()
    assert parts["hist"].sum() == h * w - 1


def _synthetic_pair(w, h, seed, sign):
    """Current and previous planes whose reprojections land across the whole image and its margin, and whose taps each validity term
    rejects alone somewhere: -> (cur, prev, cam, prev_cam).  The depth of a pixel grows smoothly from 0.15 to 4 times its ray's length
    to the target plane across the image (left to right for sign = 1, right to left for -1), so the parallax of the camera pair sweeps the
    reprojections from far outside through the margin and over the image; the previous depth plane is what those reprojections expect
    (scattered from the current pixels), so that a tap passes unless a perturbation breaks it.  Perturbations in 2 x 2 blocks of the
    previous planes, one term per block: id, depth, normal, alpha, history."""
    rng = np.random.default_rng(seed)
    cam = _cam()
    prev_cam = dict(cam_origin=(0.3 * sign, -0.9, 5.2), cam_target=(0.25 * sign, -0.75 if sign > 0 else -1.2, 2.1))
    o, t = np.asarray(cam["cam_origin"], f32), np.asarray(cam["cam_target"], f32)
    qx = (np.arange(w, dtype=f32) + f32(0.5)) / f32(w)
    qy = (np.arange(h, dtype=f32) + f32(0.5)) / f32(h)
    vx = np.broadcast_to((((qx * f32(2) - f32(1)) + t[0]) - o[0])[None, :], (h, w))
    vy = np.broadcast_to((((qy * f32(2) - f32(1)) + t[1]) - o[1])[:, None], (h, w))
    ln = np.sqrt((vx * vx + vy * vy) + (t[2] - o[2]) * (t[2] - o[2])).astype(f32)
    ramp = np.linspace(0.0, 1.0, w, dtype=np.float64)[None, :] ** 2
    if sign < 0:
        ramp = ramp[:, ::-1]
    k = 0.15 + 3.85 * ramp + 0.2 * np.linspace(0.0, 1.0, h)[:, None]
    a = np.ones((h, w), f32)
    part = rng.uniform(0, 1, (h, w)) < 0.15
    a[part] = rng.choice(np.asarray([0.25, 0.5, 0.75], f32), int(part.sum()))
    a[rng.uniform(0, 1, (h, w)) < 0.04] = 0.0
    n = np.asarray([0.36, 0.48, 0.8], f32)
    cur = {"C": rng.uniform(0, 2, (h, w, 3)).astype(f32), "M": rng.uniform(0, 4, (h, w, 3)).astype(f32),
           "N": (a[:, :, None] * n).astype(f32), "Z": ((ln * k).astype(f32) * a).astype(f32), "a": a, "ID": np.zeros((h, w, 2), np.uint32)}
    cur["ID"][:, :, 0], cur["ID"][:, :, 1] = 11, 3
    pa = np.ones((h, w), f32)
    part = rng.uniform(0, 1, (h, w)) < 0.15
    pa[part] = rng.choice(np.asarray([0.25, 0.5, 0.75], f32), int(part.sum()))
    prev = {"C": rng.uniform(0, 2, (h, w, 3)).astype(f32), "M": rng.uniform(0, 4, (h, w, 3)).astype(f32), "N": (pa[:, :, None] * n).astype(f32),
            "Z": np.zeros((h, w), f32), "a": pa, "ID": cur["ID"].copy(),
            "L": np.where(rng.uniform(0, 1, (h, w)) < 0.3, rng.uniform(0.5, 40, (h, w)), rng.integers(1, 40, (h, w))).astype(f32)}
    # what the reprojections expect of the previous depth plane: d of the pixel that lands there (neighbours agree within a few per cent)
    parts = {}
    probe = {**prev, "Z": np.ones((h, w), f32)}
    _reproject_ref(cur, probe, cam, prev_cam, parts=parts)
    po = np.asarray(prev_cam["cam_origin"], f32)
    with np.errstate(all="ignore"):
        depth = cur["Z"] / cur["a"]
        P = [o[c] + ((vx, vy, np.full((h, w), t[2] - o[2], f32))[c] / ln) * depth for c in range(3)]
        d = np.sqrt(sum((P[c] - po[c]).astype(np.float64) ** 2 for c in range(3)))
    dq = np.full((h, w), 5.0)
    ins = parts["inside"]
    for j in (0, 1):
        for i in (0, 1):
            tx, ty = parts["x0"] + i, parts["y0"] + j
            ok = ins & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            dq[ty[ok], tx[ok]] = d[ok]
    prev["Z"] = (dq * pa).astype(f32)
    # one broken term per 2 x 2 block, in 45 % of the blocks
    bh, bw = (h + 1) // 2, (w + 1) // 2
    what = np.where(rng.uniform(0, 1, (bh, bw)) < 0.45, rng.integers(1, 6, (bh, bw)), 0)
    what = np.repeat(np.repeat(what, 2, axis=0), 2, axis=1)[:h, :w]
    prev["ID"][what == 1] = (12, 3)
    prev["Z"][what == 2] = prev["Z"][what == 2] * f32(1.5)
    prev["N"][what == 3] = prev["N"][what == 3] * f32(-1.0)
    prev["a"][what == 4] = 0.0        # (a miss: its premultiplied depth and normal are 0 too)
    prev["Z"][what == 4] = 0.0
    prev["N"][what == 4] = 0.0
    prev["L"][what == 5] = 0.0
    return cur, prev, cam, prev_cam


SYN_KW = dict(gain=1.5, alpha=0.1, depth_tol=0.25, normal_min=0.9, max_history=32)


@pytest.mark.parametrize("sign", [1, -1])
def test_synthetic_planes_reach_every_tap_subset(sign):
    """The planes the GPU parity test uploads: each of the 16 tap subsets occurs at least 20 times among the pixels that passed the
    projection, each validity term alone rejects taps, reprojections land in the margin on the side the cameras' parallax pushes them to
    and on one of the vertical sides, outside and inside, the cap of the history length is reached."""
    cur, prev, cam, prev_cam = _synthetic_pair(77, 53, 21, sign)
    parts = {}
    res = _reproject_ref(cur, prev, cam, prev_cam, parts=parts, **SYN_KW)
    _check_synthetic(parts, res, sign)


def _check_synthetic(parts, res, sign):
    h, w = parts["hist"].shape
    counts = np.bincount(np.where(parts["hist"], parts["subset"], 0)[parts["inside"]].reshape(-1), minlength=16)
    empty = int((parts["inside"] & ~parts["hist"]).sum())
    assert empty >= 20 and (counts[1:] >= 20).all(), (empty, counts)
    assert all(parts["reject"][k] > 0 for k in ("id", "depth", "normal", "alpha", "history")), parts["reject"]
    ins = parts["inside"]
    assert (ins & (parts["x0"] == (-1 if sign > 0 else w - 1))).sum() > 0 and ((ins & (parts["y0"] == -1)).sum() > 0 or (ins & (parts["y0"] == h - 1)).sum() > 0)
    assert (parts["front"] & ~ins).sum() > 50 and (~parts["front"]).sum() > 50
    assert (res["L"] == 33).any() and (res["L"] == 1).any() and ((res["L"] > 1) & (res["L"] < 33)).any()


def _run_on_host(exe, d, cur, prev, cam, prev_cam, **kw):
    """the kernel's body compiled for the host (tests/reproject_host.cpp) over the given planes -> {"C", "M", "L", "bgra"}"""
    os.makedirs(d, exist_ok=True)
    h, w = cur["Z"].shape
    cam, prev_cam = _cam(cam), _cam(prev_cam)
    k = dict(gain=1.0, alpha=0.2, depth_tol=0.1, normal_min=0.9, max_history=32, flags=MATCH_ID)
    k.update(kw)
    has_m = cur.get("M") is not None
    par = np.zeros(24, f32)
    par[:4] = [w, h, prev is not None, k["flags"] & MATCH_ID]
    par[4:10] = list(cam["cam_origin"]) + list(cam["cam_target"])
    par[10:16] = list(prev_cam["cam_origin"]) + list(prev_cam["cam_target"])
    par[16:22] = [k["gain"], k["alpha"], k["depth_tol"], k["normal_min"], k["max_history"], has_m]
    par.tofile(os.path.join(d, "par"))
    zeros3 = np.zeros((h, w, 3), f32)
    for pre, x in (("c_", cur), ("p_", prev if prev is not None else {**cur, "L": np.zeros((h, w), f32)})):
        for n in ("C", "M", "N", "Z", "a", "ID") + (("L",) if pre == "p_" else ()):
            np.ascontiguousarray(x[n] if x.get(n) is not None else zeros3).tofile(os.path.join(d, pre + n))
    subprocess.check_call([exe, d])
    out = {"C": np.fromfile(os.path.join(d, "o_C"), f32).reshape(h, w, 3), "L": np.fromfile(os.path.join(d, "o_L"), f32).reshape(h, w),
           "bgra": np.fromfile(os.path.join(d, "o_bgra"), np.uint8).reshape(h, w, 4)}
    if has_m:
        out["M"] = np.fromfile(os.path.join(d, "o_M"), f32).reshape(h, w, 3)
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_kernel_body_on_the_host_equals_the_reference(tmp_path, sanitize):
    """csrc/reproject_kernel.h -- the statements k_reproject runs per pixel -- compiled by g++ as a stand-alone program (-ffp-contract=off,
    IEEE divides and roots for pt_math.h's helpers) gives the bytes of `_reproject_ref`: on the synthetic 77 x 53 planes of the GPU test
    (every tap subset, every rejecting term, the margin), with MATCH_ID off, without M, with prev = NULL, and on the small walls whose
    reprojections fall into the margin and the corner.  The second build runs the same cases under AddressSanitizer and UBSan: every tap
    address is inside its plane."""
    exe = str(tmp_path / "reproject_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "reproject_host.cpp")])
    cases = []
    for sign in (1, -1):
        cur, prev, cam, pc = _synthetic_pair(77, 53, 21, sign)
        cases += [(cur, prev, cam, pc, SYN_KW), (cur, prev, cam, pc, dict(SYN_KW, flags=0, alpha=0.0, max_history=7)), (cur, None, cam, pc, dict(gain=3.0)),
                  ({k: v for k, v in cur.items() if k != "M"}, {k: v for k, v in prev.items() if k != "M"}, cam, pc, SYN_KW)]
    pc = _cam(None, (0.3125, 0.5, 0.0))
    for h, w in SHAPES:
        cur, prev = _wall_pair(h, w, 3, prev_cam=pc)
        cases.append((cur, prev, None, pc, dict(depth_tol=0.5, gain=2.0)))
    hist = 0
    for n, (cur, prev, cam, pc, kw) in enumerate(cases):
        parts = {}
        want = _reproject_ref(cur, prev, cam, pc, parts=parts, **kw)
        got = _run_on_host(exe, str(tmp_path / f"case{n}"), cur, prev, cam, pc, **kw)
        assert ("M" in got) == ("M" in want)
        _same_planes(got, want, ("host", n, kw))
        hist += int(parts["hist"].sum())
    assert hist > 5000


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
_scene = test_denoise._scene
MOVES = [(0.0, 0.0, 0.0), (0.05, 0.0, 0.0), (0.0, 0.0, -0.1), (0.03, 0.02, -0.03)]


def _new_film(pt, ctx, w, h, moments):
    film = pt.Film(ctx, w, h)
    film.enable_aov()
    if moments:
        film.enable_moments()
    film.enable_history()
    return film


def _render_step(pt, sc, film, w, h, spp, cam, frame, pipeline, max_depth=4):
    kw = dict(width=w, height=h, spp_per_frame=spp, pipeline=pipeline, **cam)
    pt.render(sc, film, pt.default_params(frame=frame, frame_count=1, max_depth=max_depth, **kw))
    pt.render_aov(sc, film, pt.default_params(frame=0, frame_count=1, **kw))


def _read_planes(film, pt, moments):
    """what the device holds of a film: the reference's input (and, after a call, what its output is compared with)"""
    d = {"C": film.read_f32(), "N": film.read_aov(pt.AOV_NORMAL), "Z": film.read_aov(pt.AOV_DEPTH), "a": film.read_aov(pt.AOV_ALPHA),
         "ID": film.read_aov(pt.AOV_ID), "L": film.read_history(), "bgra": film.read_bgra8()}
    if moments:
        d["M"] = film.read_moments()[0]
    return d


def _same_planes(got, want, what):
    for k in ("C", "M", "L", "bgra"):
        if k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert got[k].tobytes() == want[k].tobytes(), (what, k, int((got[k] != want[k]).sum()))


def _step(pt, film, prev, cam, prev_cam, moments, what, **kw):
    """one pt_film_reproject against the reference fed with the device's planes -> (the parts of the reference, the film's planes after)"""
    cur_in = _read_planes(film, pt, moments)
    prev_in = _read_planes(prev, pt, moments) if prev is not None else None
    ms = film.reproject(prev, cam, prev_cam, **kw)
    assert ms > 0
    parts = {}
    want = _reproject_ref(cur_in, prev_in, cam, prev_cam, parts=parts, **kw)
    got = _read_planes(film, pt, moments)
    _same_planes(got, want, what)
    return parts, got


RENDERED = ["cornell", "cornell_odd", "cornell_77", "grid16", "soup", "one_pixel", "three_by_two"]


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["WAVEFRONT", "AUTO"])
@pytest.mark.parametrize("case", RENDERED)
def test_reproject_rendered_films(pt, gpu_ctx, case, pipeline):
    """Two steps per camera move, with and without M: step 0 with prev = NULL, step 1 at frame = 1 with gain = 2 at the moved camera."""
    scene, w, h, spp, cam0 = test_denoise.CASES[case]
    sc = _scene(pt, gpu_ctx, scene)
    pl = getattr(pt, "PIPELINE_" + pipeline)
    found = 0
    for moments in (False, True):
        a = _new_film(pt, gpu_ctx, w, h, moments)
        try:
            c0 = _cam(cam0)
            _render_step(pt, sc, a, w, h, spp, c0, 0, pl)
            parts, a_out = _step(pt, a, None, c0, c0, moments, (case, pipeline, moments, "step 0"))
            assert (a_out["L"] == 1).all()
            for move in MOVES:
                b = _new_film(pt, gpu_ctx, w, h, moments)
                try:
                    c1 = _cam(cam0, move)
                    _render_step(pt, sc, b, w, h, spp, c1, 1, pl)
                    parts, _ = _step(pt, b, a, c1, c0, moments, (case, pipeline, moments, move), gain=2.0)
                    found += int(parts["hist"].sum())
                    assert _read_planes(a, pt, moments)["C"].tobytes() == a_out["C"].tobytes()
                finally:
                    b.close()
        finally:
            a.close()
    assert found > 0 or case in ("one_pixel", "three_by_two")


@pytest.mark.gpu
def test_reproject_external_planes(pt, gpu_ctx):
    """Every plane of both films in torch tensors (radiance, guides, M, L) == films that own them."""
    import torch
    scene, w, h, spp, cam0 = test_denoise.CASES["cornell_odd"]
    sc = _scene(pt, gpu_ctx, scene)
    c0, c1 = _cam(cam0), _cam(cam0, (0.03, 0.02, -0.03))
    own = [_new_film(pt, gpu_ctx, w, h, True) for _ in range(2)]
    ext, keep = [], []
    try:
        for k in range(2):
            t = {"C": torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), "M": torch.full((h, w, 3), 5.0, dtype=torch.float32, device="cuda:0"),
                 "L": torch.full((h, w), 5.0, dtype=torch.float32, device="cuda:0")}
            shapes = {pt.AOV_ALBEDO: (h, w, 3), pt.AOV_NORMAL: (h, w, 3), pt.AOV_EMISSION: (h, w, 3), pt.AOV_DEPTH: (h, w), pt.AOV_ALPHA: (h, w), pt.AOV_ID: (h, w, 2)}
            g = {n: torch.zeros(s, dtype=torch.float32 if n != pt.AOV_ID else torch.int32, device="cuda:0") for n, s in shapes.items()}
            torch.cuda.synchronize()
            f = pt.Film(gpu_ctx, w, h, device_ptr=t["C"].data_ptr())
            f.enable_aov([g[n].data_ptr() for n in range(pt.AOV_COUNT)])
            f.enable_moments(t["M"].data_ptr())
            f.enable_history(t["L"].data_ptr())
            assert not t["L"].any().item()         # (zeroed by the call)
            ext.append(f)
            keep.append((t, g))
        for films in (own, ext):
            _render_step(pt, sc, films[0], w, h, spp, c0, 0, pt.PIPELINE_AUTO)
            _step(pt, films[0], None, c0, c0, True, "step 0")
            _render_step(pt, sc, films[1], w, h, spp, c1, 1, pt.PIPELINE_AUTO)
            parts, _ = _step(pt, films[1], films[0], c1, c0, True, "step 1", gain=2.0)
            assert parts["hist"].any()
        _same_planes(_read_planes(ext[1], pt, True), _read_planes(own[1], pt, True), "external == owned")
        torch.cuda.synchronize()
        t = keep[1][0]
        assert t["L"].cpu().numpy().tobytes() == own[1].read_history().tobytes() and t["C"].cpu().numpy().tobytes() == own[1].read_f32().tobytes()
        assert t["M"].cpu().numpy().tobytes() == own[1].read_moments()[0].tobytes()
    finally:
        for f in own + ext:
            f.close()
    del keep


@pytest.mark.gpu
def test_reproject_chain_of_six_steps(pt, gpu_ctx):
    """52 x 36 Cornell, two films ping-ponged over six steps after the first: L grows to the cap (max_history = 3) + 1, and every step is
    the reference applied to what the device held before it."""
    scene, w, h, spp, cam0 = test_denoise.CASES["cornell_odd"]
    sc = _scene(pt, gpu_ctx, scene)
    move = (0.02, 0.0, -0.01)
    films = [_new_film(pt, gpu_ctx, w, h, True) for _ in range(2)]
    try:
        prev = prev_cam = None
        for k in range(7):
            f = films[k & 1]
            f.clear()
            assert not f.read_history().any()
            cam = _cam(cam0, move, k)
            _render_step(pt, sc, f, w, h, spp, cam, k, pt.PIPELINE_AUTO)
            parts, got = _step(pt, f, prev, cam, prev_cam or cam, True, ("chain", k), gain=float(f32(k + 1)), max_history=3)
            assert got["L"].max() == min(k, 3) + 1, (k, got["L"].max())
            prev, prev_cam = f, cam
        assert (got["L"] == 4).mean() > 0.5
    finally:
        for f in films:
            f.close()


def _upload(pt, ctx, torch, d):
    """a film over external tensors holding the planes of `d` (test_denoise_variance's external film plus ids and L)"""
    h, w = d["Z"].shape
    zeros3 = np.zeros((h, w, 3), f32)
    g = {"albedo": zeros3, "normal": d["N"], "emission": zeros3, "depth": d["Z"], "alpha": d["a"]}
    film, (t_rgb, planes, ids) = test_denoise._external_film(pt, ctx, torch, d["C"], g)
    ids.copy_(torch.from_numpy(np.ascontiguousarray(d["ID"]).view(np.int32)))
    t_m = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    t_l = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    film.enable_moments(t_m.data_ptr())
    film.enable_history(t_l.data_ptr())
    t_m.copy_(torch.from_numpy(np.ascontiguousarray(d["M"])))
    if "L" in d:
        t_l.copy_(torch.from_numpy(np.ascontiguousarray(d["L"])))
    torch.cuda.synchronize()
    return film, (t_rgb, planes, ids, t_m, t_l)


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1, -1])
def test_reproject_synthetic_planes(pt, gpu_ctx, sign):
    """Planes made on the host at 77 x 53 in external tensors: every one of the 16 tap subsets at least 20 times, every validity term
    rejecting alone, the margin, outside, behind -- asserted on the reference's parts before the comparison.  Then MATCH_ID off."""
    import torch
    cur, prev, cam, prev_cam = _synthetic_pair(77, 53, 21, sign)
    for kw in (SYN_KW, dict(SYN_KW, flags=0, alpha=0.0, max_history=7)):
        fc, keep_c = _upload(pt, gpu_ctx, torch, cur)
        fp, keep_p = _upload(pt, gpu_ctx, torch, prev)
        try:
            got_in = _read_planes(fp, pt, True)
            assert all(got_in[k].tobytes() == prev[k].tobytes() for k in ("C", "M", "N", "Z", "a", "ID", "L"))
            if kw is SYN_KW:   # what the planes reach, by the reference alone, before anything is compared
                parts = {}
                _check_synthetic(parts, _reproject_ref(cur, prev, cam, prev_cam, parts=parts, **kw), sign)
            _step(pt, fc, fp, cam, prev_cam, True, ("synthetic", sign, kw), **kw)
        finally:
            fc.close(); fp.close()
        del keep_c, keep_p


@pytest.mark.gpu
def test_reproject_1080p_cornell_step(pt, gpu_ctx, cornell_gpu):
    """One 1920 x 1080 Cornell step, camera step (0.02, 0, 0): the whole planes against the reference (a tap pass is four gathers, so the
    full-frame numpy statement is affordable), as SHA-256 of C, M, L and bgra8 and on three 256 x 256 crops."""
    w, h, spp = 1920, 1080, 4
    c0, c1 = _cam(), _cam(None, (0.02, 0.0, 0.0))
    a, b = _new_film(pt, gpu_ctx, w, h, True), _new_film(pt, gpu_ctx, w, h, True)
    try:
        _render_step(pt, cornell_gpu, a, w, h, spp, c0, 0, pt.PIPELINE_AUTO, max_depth=8)
        a.reproject(None, c0, c0)
        _render_step(pt, cornell_gpu, b, w, h, spp, c1, 1, pt.PIPELINE_AUTO, max_depth=8)
        cur_in, prev_in = _read_planes(b, pt, True), _read_planes(a, pt, True)
        b.reproject(a, c1, c0, gain=2.0)
        parts = {}
        want = _reproject_ref(cur_in, prev_in, c1, c0, gain=2.0, parts=parts)
        got = _read_planes(b, pt, True)
        for x0, y0 in ((0, 0), (w - 256, h - 256), (832, 412)):
            crop = (slice(y0, y0 + 256), slice(x0, x0 + 256))
            _same_planes({k: np.ascontiguousarray(got[k][crop]) for k in ("C", "M", "L", "bgra")}, {k: np.ascontiguousarray(want[k][crop]) for k in ("C", "M", "L", "bgra")}, ("crop", x0, y0))
        for k in ("C", "M", "L", "bgra"):
            assert hashlib.sha256(got[k].tobytes()).hexdigest() == hashlib.sha256(want[k].tobytes()).hexdigest(), k
        covered = cur_in["a"] > 0
        assert parts["hist"][covered].mean() > 0.85
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_reproject_moves_nothing_else(pt, gpu_ctx):
    """The guides of `film`, every plane of `prev` and pt_stats are byte-identical before and after; free device memory does not change
    over three further calls; pt_film_clear zeroes L; a render into a film with L gives the same film, bgra8, ray counts and
    workspace_bytes as into one without."""
    import torch
    scene, w, h, spp, cam0 = test_denoise.CASES["cornell"]
    sc = _scene(pt, gpu_ctx, scene)
    c0, c1 = _cam(cam0), _cam(cam0, (0.05, 0.0, 0.0))
    a, b = _new_film(pt, gpu_ctx, w, h, True), _new_film(pt, gpu_ctx, w, h, True)
    plain = pt.Film(gpu_ctx, w, h)
    try:
        _render_step(pt, sc, a, w, h, spp, c0, 0, pt.PIPELINE_AUTO)
        a.reproject(None, c0, c0)
        gpu_ctx.reset_stats()
        _render_step(pt, sc, b, w, h, spp, c1, 1, pt.PIPELINE_AUTO)
        st_b = gpu_ctx.stats()
        gpu_ctx.reset_stats()
        plain.enable_aov()
        plain.enable_moments()
        _render_step(pt, sc, plain, w, h, spp, c1, 1, pt.PIPELINE_AUTO)
        st_p = gpu_ctx.stats()
        assert (st_b.rays, st_b.paths, st_b.pipeline, st_b.workspace_bytes) == (st_p.rays, st_p.paths, st_p.pipeline, st_p.workspace_bytes)
        assert b.read_f32().tobytes() == plain.read_f32().tobytes() and b.read_bgra8().tobytes() == plain.read_bgra8().tobytes()
        assert b.read_moments()[0].tobytes() == plain.read_moments()[0].tobytes() and not b.read_history().any()

        def rest():
            s = gpu_ctx.stats()
            pa = _read_planes(a, pt, True)
            return ([b.read_aov(k).tobytes() for k in range(pt.AOV_COUNT)] + [pa[k].tobytes() for k in sorted(pa)] + [a.read_aov(k).tobytes() for k in range(pt.AOV_COUNT)],
                    bytes(s))
        before = rest()
        b.reproject(a, c1, c0, gain=2.0)
        assert rest() == before
        first = _read_planes(b, pt, True)
        assert (first["L"] > 1).any()
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        for _ in range(3):
            b.reproject(a, c1, c0, gain=2.0)
        torch.cuda.synchronize()
        free1, _ = torch.cuda.mem_get_info()
        assert free1 == free0, (free0, free1)
        assert rest() == before
        b.clear()
        assert not b.read_history().any() and not b.read_f32().any()
    finally:
        a.close(); b.close(); plain.close()


@pytest.mark.gpu
def test_reproject_errors(pt, gpu_ctx, cornell_gpu):
    """Every PT_ERR_INVALID_ARG of the header; each leaves C, M, L and bgra8 as they were."""
    lib = pt.lib_amd()
    w, h = 48, 40
    cam = _cam()
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=3, pipeline=pt.PIPELINE_AUTO)

    def status(fn):
        with pytest.raises(pt.PtError) as e:
            fn()
        return e.value.status

    film, prev = _new_film(pt, gpu_ctx, w, h, True), _new_film(pt, gpu_ctx, w, h, True)
    others = []
    try:
        for f in (film, prev):
            pt.render(cornell_gpu, f, pt.default_params(frame=0, frame_count=1, **kw))
            pt.render_aov(cornell_gpu, f, pt.default_params(frame=0, frame_count=1, **kw))
        prev.reproject(None, cam, cam)
        before = {k: v.tobytes() for k, v in _read_planes(film, pt, True).items()}
        good = pt.reproject_default_params()
        assert lib.pt_film_reproject(None, prev.h, C.byref(good), None) == 1            # NULL film
        assert lib.pt_film_reproject(film.h, prev.h, None, None) == 1                    # NULL params
        assert lib.pt_film_enable_history(None, None) == 1 and lib.pt_film_read_history(None, None) == 1
        assert lib.pt_film_read_history(film.h, None) == 1
        assert status(lambda: film.enable_history()) == 1                               # a second call
        assert status(lambda: film.reproject(film, cam, cam)) == 1                      # prev == film
        small = _new_film(pt, gpu_ctx, w, h - 1, True)
        others.append(small)
        assert status(lambda: film.reproject(small, cam, cam)) == 1                     # another size
        ctx2 = pt.Context(0)
        try:
            foreign = _new_film(pt, ctx2, w, h, True)
            assert status(lambda: film.reproject(foreign, cam, cam)) == 1               # another context
            foreign.close()
        finally:
            ctx2.close()
        for aov, hist in ((False, True), (True, False)):
            f = pt.Film(gpu_ctx, w, h)
            others.append(f)
            if aov:
                f.enable_aov()
            f.enable_moments()
            if hist:
                f.enable_history()
            else:
                assert status(lambda: f.read_history()) == 1
            assert status(lambda: f.reproject(prev, cam, cam)) == 1                     # `film` without guides / without L
            assert status(lambda: f.reproject(None, cam, cam)) == 1
            assert status(lambda: film.reproject(f, cam, cam)) == 1                     # `prev` without guides / without L
        no_m = _new_film(pt, gpu_ctx, w, h, False)
        others.append(no_m)
        assert status(lambda: film.reproject(no_m, cam, cam)) == 1                      # exactly one of the two has M
        assert status(lambda: no_m.reproject(prev, cam, cam)) == 1
        nan, inf = float("nan"), float("inf")
        for name, bad in (("gain", (0.0, -1.0, nan, inf)), ("depth_tol", (0.0, -0.1, nan, inf)), ("alpha", (-0.1, 1.5, nan, inf)),
                          ("normal_min", (-1.5, 1.5, nan, inf)), ("max_history", (0, 65536, 0xFFFFFFFF)), ("flags", (2, 3, 0x80000000))):
            for v in bad:
                assert status(lambda: film.reproject(prev, cam, cam, **{name: v})) == 1, (name, v)
                assert status(lambda: film.reproject(None, cam, cam, **{name: v})) == 1, (name, v)
        for bad_cam in (dict(cam_origin=(nan, 0.0, 0.0)), dict(cam_target=(0.0, inf, 0.0))):
            assert status(lambda: film.reproject(prev, _cam() | bad_cam, cam)) == 1
            assert status(lambda: film.reproject(prev, cam, _cam() | bad_cam)) == 1
        for k in range(4):
            p = pt.reproject_default_params()
            p.reserved[k] = 1
            assert status(lambda: film.reproject(prev, cam, cam, params=p)) == 1
        assert {k: v.tobytes() for k, v in _read_planes(film, pt, True).items()} == before     # a refused call writes nothing
        for v in (dict(alpha=0.0), dict(alpha=1.0), dict(normal_min=-1.0), dict(normal_min=1.0), dict(max_history=1), dict(max_history=65535), dict(flags=0)):
            film.reproject(prev, cam, cam, **v)                                         # the ends of the ranges go through
    finally:
        for f in [film, prev] + others:
            f.close()


@pytest.mark.gpu
def test_pt_main_temporal(pt, tmp_path):
    """pt_main --temporal 3 --cam-step 0.02,0,0 writes the image of the Python chain: K time steps of one frame each at frame = k, the
    camera moved by the step each time, two films ping-ponged."""
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_main")
    if not os.path.exists(exe):
        pt.build()
    w, h, spp, depth, K, move = 48, 40, 4, 3, 3, (0.02, 0.0, 0.0)
    base = [exe, "--obj", pt.ASSET_CORNELL, "--width", str(w), "--height", str(h), "--spp", str(spp), "--depth", str(depth)]
    subprocess.run(base + ["--temporal", str(K), "--cam-step", "0.02,0,0", "--ppm", str(tmp_path / "t.ppm"), "--pfm", str(tmp_path / "t.pfm")],
                   check=True, capture_output=True, text=True, cwd=pt.REPO)
    for misuse in (["--cam-step", "0.02,0,0"], ["--temporal", "0"], ["--temporal", "3", "--cam-step", "1,2"], ["--temporal", "3", "--ranks", "2"]):
        bad = subprocess.run(base + misuse, capture_output=True, text=True, cwd=pt.REPO)
        assert bad.returncode != 0 and ("--temporal" in bad.stderr or "--cam-step" in bad.stderr), misuse
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    films = [_new_film(pt, ctx, w, h, False) for _ in range(2)]
    prev = prev_cam = None
    for k in range(K):
        f = films[k & 1]
        f.clear()
        cam = _cam(None, move, k)
        kw = dict(width=w, height=h, spp_per_frame=spp, frame=k, frame_count=1, pipeline=pt.PIPELINE_AUTO, **cam)
        pt.render(sc, f, pt.default_params(max_depth=depth, **kw))
        pt.render_aov(sc, f, pt.default_params(**{**kw, "frame": 0}))
        f.reproject(prev, cam, prev_cam or cam, gain=float(f32(k + 1)))
        prev, prev_cam = f, cam
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    raw = open(tmp_path / "t.pfm", "rb").read()
    assert raw.startswith(head)
    img = np.ascontiguousarray(np.frombuffer(raw[len(head):], f32).reshape(h, w, 3)[::-1])
    assert img.tobytes() == prev.read_f32().tobytes()
    ppm_head = f"P6\n{w} {h}\n255\n".encode()
    ppm = open(tmp_path / "t.ppm", "rb").read()
    assert ppm.startswith(ppm_head) and ppm[len(ppm_head):] == np.ascontiguousarray(prev.read_bgra8()[:, :, 2::-1]).tobytes()
    assert (prev.read_history() == 3).any()
    for f in films:
        f.close()
    sc.close(); ctx.close()
