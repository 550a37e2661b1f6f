"""pt_crossings_device without a GPU (include/pt_api.h): the ABI and the names; the statements that define the result
(csrc/crossings_kernel.h) compiled for the host (tests/crossings_host.cpp) and run as a program -- plain and under the address and
undefined-behaviour sanitizers -- bit for bit against the numpy restatement of tests/crossings_cases.py, with the walk's lemma checked on every
pair; the restatement's triangle test pinned to the oracle's brute force; the premises of tests/test_crossings.py and the inside / outside
votes judged from the restatement alone."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import crossings_cases as cc
import trace_device_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_crossings_abi_and_names(pt, tmp_path):
    """By gcc from the header: sizeof(pt_crossings_desc) == 80, the three enum values, PT_API_VERSION == 6, the offsets, the two prototypes; the
    names in API_SYMBOLS and in the built library; the Python constants and the default descriptor; crossings_tensors refuses an unknown form
    before it touches a device; NULL handles are PT_ERR_INVALID_ARG; the vote directions are unit vectors off every axis and coordinate plane."""
    src = tmp_path / "cx_abi.c"
    vals = ["sizeof(pt_crossings_desc)", "(size_t)PT_CROSSINGS_AUTO", "(size_t)PT_CROSSINGS_LDS", "(size_t)PT_CROSSINGS_GLOBAL", "(size_t)PT_API_VERSION",
            "offsetof(pt_crossings_desc, d_winding)", "offsetof(pt_crossings_desc, direction)", "offsetof(pt_crossings_desc, tmin)",
            "offsetof(pt_crossings_desc, form)", "offsetof(pt_crossings_desc, reserved)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\n'
                   "void (*p_default)(pt_crossings_desc *) = pt_crossings_desc_default;\n"
                   "pt_status (*p_call)(pt_scene *, const pt_crossings_desc *, uint64_t, float *) = pt_crossings_device;\n"
                   'int main(void){printf("' + "%zu " * len(vals) + '\\n",' + ", ".join(vals) + ");return p_default == 0 || p_call == 0;}\n")
    exe = tmp_path / "cx_abi"
    lib_dir = os.path.dirname(pt.__file__)
    subprocess.check_call([shutil.which("gcc") or "gcc", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src),
                           "-L", lib_dir, "-l:libpt_amd.so", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [80, 0, 1, 2, 6, 32, 40, 52, 60, 68], got
    L = pt.lib_amd()
    for name in ("pt_crossings_desc_default", "pt_crossings_device"):
        assert name in pt.API_SYMBOLS and hasattr(L, name), name
    assert (pt.CROSSINGS_AUTO, pt.CROSSINGS_LDS, pt.CROSSINGS_GLOBAL) == (0, 1, 2) and ctypes.sizeof(pt.CrossingsDesc) == 80
    d = pt.crossings_default_desc()
    assert d.tmin == 0.0 and d.tmax == np.inf and d.form == 0 and d.flags == 0 and not any(d.reserved) and not any(d.direction)
    assert not d.d_rays6 and not d.d_points and not d.d_tmax and not d.d_count and not d.d_winding
    with pytest.raises(ValueError):
        pt.Scene.crossings_tensors(None, None, form="fused")       # (no scene, no tensor: the form is judged first)
    assert L.pt_crossings_device(None, ctypes.byref(d), 1, None) == 1   # PT_ERR_INVALID_ARG
    L.pt_crossings_desc_default(None)                                    # (a no-op)
    dirs = np.asarray(pt.INSIDE_DIRECTIONS)
    assert dirs.shape == (5, 3) and np.allclose(np.linalg.norm(dirs, axis=1), 1) and (np.abs(dirs) > 0.1).all()


# ---- the host program ---------------------------------------------------------------------------------------------------------------------
def _write(d, name, a, dt=f32):
    np.ascontiguousarray(a, dt).tofile(os.path.join(d, name))


def _bits(x):
    return int(f32(x).view(np.uint32))


def _host_run(exe, d, pairs=None, boxes=None, rays=None, bounds=None, tris=None, tmin=0.0, tmax=np.inf, pad=0.0, direction=None, want_count=True,
              want_winding=True):
    """pairs [n, 18]; boxes [n, k, 2, 3]; rays [m, 6], or [m, 3] with a direction"""
    os.makedirs(d, exist_ok=True)
    pairs = np.zeros((0, 18), f32) if pairs is None else pairs
    boxes = np.zeros((len(pairs), 0, 2, 3), f32) if boxes is None else boxes
    rays = np.zeros((0, 6), f32) if rays is None else rays
    tris = np.zeros((0, 3, 3), f32) if tris is None else tris
    n, k, m = len(pairs), boxes.shape[1], len(rays)
    dr = (0.0, 0.0, 0.0) if direction is None else direction
    _write(d, "par", [n, k, m, len(tris), int(bounds is not None), int(direction is not None), int(want_count), int(want_winding), _bits(tmin), _bits(tmax),
                      _bits(pad), _bits(dr[0]), _bits(dr[1]), _bits(dr[2])], np.uint32)
    _write(d, "pairs", pairs)
    _write(d, "boxes", boxes)
    _write(d, "rays", np.concatenate([np.asarray([123.0], f32), np.asarray(rays, f32).reshape(-1)]))   # rows start one float into the allocation
    _write(d, "bounds", np.zeros(0, f32) if bounds is None else bounds)
    _write(d, "tris", tris)
    subprocess.check_call([exe, d])
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    return {"flags": rd("o_flags", np.uint8).reshape(n, 4), "vals": rd("o_vals", f32).reshape(n, 11), "boxes": rd("o_boxes", np.uint8).reshape(n, k),
            "count": rd("o_count", np.uint32), "winding": rd("o_winding", np.int32)}


def _same_bits(a, b):
    """bit for bit; a NaN equals a NaN (its sign and payload are the divider's business)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _pairs(O, D, tmin, b, pad, tris):
    n = len(O)
    col = lambda x: np.broadcast_to(np.asarray(x, f32), (n,)).reshape(n, 1)
    return np.ascontiguousarray(np.concatenate([O, D, col(tmin), col(b), col(pad), np.asarray(tris, f32).reshape(n, 9)], 1), f32)


def _pads(tris):
    return (np.abs(tris).max((1, 2)) * f32(3.814697265625e-06)).astype(f32)


def _aimed(n, seed, share=0.6, scale=1.0):
    """triangles uniform in [-1, 1]^3, origins in [-2, 2]^3; `share` of the rays aimed at a point inside their triangle (to rounding), the rest
    drawn freely; directions not normalised.  -> origins, directions, triangles, targets"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, (n, 3, 3)).astype(f32)
    o = rng.uniform(-2, 2, (n, 3)).astype(f32)
    bc = rng.dirichlet((1, 1, 1), n).astype(f32)
    target = (t * bc[:, :, None]).sum(1).astype(f32)
    d = np.where((rng.uniform(0, 1, n) < share)[:, None], (target - o) * rng.uniform(0.2, 3, (n, 1)), rng.standard_normal((n, 3))).astype(f32)
    return (o * f32(scale)).astype(f32), d, (t * f32(scale)).astype(f32), target


def _pair_sets():
    rng = np.random.default_rng(5)
    sets = {}
    o, d, t, _ = _aimed(20_000, 4)
    sets["random"] = _pairs(o, d, 0.0, np.inf, _pads(t), t)
    o, d, t, _ = _aimed(2000, 6)
    o, t = (o + f32(1e6)).astype(f32), (t + f32(1e6)).astype(f32)                     # coordinates near 1e6: sixteen ulps per unit
    sets["near_1e6"] = _pairs(o, d, 0.0, np.inf, _pads(t), t)
    o, d, t, _ = _aimed(2000, 7, scale=1e-41)                                           # every coordinate a denormal
    sets["denormal"] = _pairs(o, d, 0.0, np.inf, _pads(t), t)
    o, d, t, _ = _aimed(3000, 9)
    t[:1000, 2] = t[:1000, 1]                                                        # two equal vertices
    w = rng.uniform(-1, 2, (1000, 1)).astype(f32)
    t[1000:2000, 2] = (t[1000:2000, 0] + (t[1000:2000, 1] - t[1000:2000, 0]) * w).astype(f32)   # three collinear (to rounding)
    t[2000:, 1] = t[2000:, 0]                                                        # all equal
    t[2000:, 2] = t[2000:, 0]
    d[::2] = (t[::2, 0] - o[::2]).astype(f32)                                        # half of them aimed at vertex A
    sets["degenerate"] = _pairs(o, d, 0.0, np.inf, _pads(t), t)
    o, d, t, target = _aimed(3000, 10)                                                       # direction components 0, -0.0, denormal; all zero
    k = np.arange(3000)
    special = np.asarray([0.0, -0.0, 1e-41, -1e-41, 1e-21, -1e-21], f32)
    d[k, k % 3] = special[k % 6]
    d[1000:2000, (k[1000:2000] + 1) % 3] = special[(k[1000:2000] // 3) % 6]
    d[2000:2500] = special[k[2000:2500] % 2][:, None]                                # all three components 0 or -0.0
    d[2500:] = special[2 + k[2500:] % 4][:, None]                                    # all three tiny
    o[:2000] = (target[:2000] - d[:2000]).astype(f32)                                # (the first 2 000 still pass their triangle, at t = 1)
    sets["zero_direction"] = _pairs(o, d, 0.0, np.inf, _pads(t), t)
    o, d, t, _ = _aimed(1200, 11)                                                       # non-finite rays, NaN bounds
    bad = np.asarray([np.nan, np.inf, -np.inf], f32)
    k = np.arange(1200)
    o[k[:600], k[:600] % 3] = bad[(k[:600] // 3) % 3]
    d[k[600:1000], k[600:1000] % 3] = bad[(k[600:1000] // 3) % 3]
    b = np.full(1200, np.inf, f32)
    b[1000:] = np.nan
    sets["non_finite"] = _pairs(o, d, 0.0, b, _pads(t), t)
    # t exactly on, one ulp below and one ulp above tmin and the bound
    o, d, t, _ = _aimed(6000, 12, share=1.0)
    free = cc.pair_verdicts(o, d, f32(0), f32(np.inf), t[:, 0], t[:, 1], t[:, 2], _pads(t))
    hit = free["tri"] & (free["t"] > 1e-3)
    o, d, t, th = o[hit], d[hit], t[hit], free["t"][hit]
    m = len(th)
    assert m > 3000, m
    edge = np.stack([th, cc.nextup(th), cc.nextdown(th)], 1)[np.arange(m), np.arange(m) % 3]
    lo_end = (np.arange(m) // 3) % 2 == 0                                            # the end that sits on t: tmin or the bound
    sets["range_ends"] = _pairs(o, d, np.where(lo_end, edge, f32(0)), np.where(lo_end, f32(np.inf), edge), _pads(t), t)
    return sets


def _boxes_of(pairs, seed):
    """per pair: the triangle's own padded box and three grown by random amounts (>= 0, some 0, some huge) -> [n, 4, 2, 3]"""
    rng = np.random.default_rng(seed)
    tri = pairs[:, 9:].reshape(-1, 3, 3)
    lo, hi = cc.own_box(tri[:, 0], tri[:, 1], tri[:, 2], pairs[:, 8])
    out = np.zeros((len(pairs), 4, 2, 3), f32)
    out[:, 0, 0], out[:, 0, 1] = lo, hi
    scale = np.maximum(np.abs(pairs[:, 9:]).max(1), f32(1e-45))[:, None]
    for k, mag in enumerate((1e-6, 0.1, 100.0), 1):
        g = (rng.uniform(0, mag, (len(pairs), 2, 3)) * (rng.uniform(0, 1, (len(pairs), 2, 3)) < 0.8)).astype(f32) * scale[:, None]
        out[:, k, 0], out[:, k, 1] = (lo - g[:, 0]).astype(f32), (hi + g[:, 1]).astype(f32)
    assert (out[:, :, 0] <= lo[:, None]).all() and (out[:, :, 1] >= hi[:, None]).all()   # (they contain the own box as float32 numbers)
    return out


def _grazing_pairs():
    """every triangle of a small soup with the 18 rays of cc.grazing_rays in the planes of ITS OWN padded box"""
    rng = np.random.default_rng(21)
    tris = cc.triangles(*tc.soup(300, 3)[:2])
    pad = cc.pad_of(tris)
    rays = np.concatenate([cc.grazing_rays(tris, pad, [k], rng) for k in range(len(tris))])
    t = np.repeat(tris, 18, 0)
    return _pairs(rays[:, :3], rays[:, 3:], 0.0, np.inf, pad, t)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def host_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("crossings_host") / "crossings_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "crossings_host.cpp")])
    return exe


def test_pairs_and_lemma_on_the_host(host_exe, tmp_path):
    """cx_counts, cx_own_box, cx_inv, cx_live and cx_slab as a program, bit for bit against the restatement -- accept / reject, t, det, the
    own-box verdict, what the pair adds, the reciprocals, the box -- on 20 000 random ray / triangle pairs, pairs near 1e6, denormal pairs,
    degenerate triangles, zero / -0.0 / denormal direction components and all-zero directions (which hit nothing), non-finite rays and NaN
    bounds (which do not walk), and t exactly on, one ulp below and one ulp above tmin and the bound.  The lemma: on every pair with a finite
    ray whose own box passes, three grown boxes pass too -- zero violations, the grazing set (rays in the planes of the own box and one ulp to
    either side) included."""
    violations, checked = 0, 0
    sets = _pair_sets()
    sets["grazing"] = _grazing_pairs()
    for name, pairs in sets.items():
        boxes = _boxes_of(pairs, 11)
        out = _host_run(host_exe, str(tmp_path / name), pairs=pairs, boxes=boxes)
        tri = pairs[:, 9:].reshape(-1, 3, 3)
        O, D, tmin, b, pad = pairs[:, :3], pairs[:, 3:6], pairs[:, 6], pairs[:, 7], pairs[:, 8]
        ref = cc.pair_verdicts(O, D, tmin, b, tri[:, 0], tri[:, 1], tri[:, 2], pad)
        want_flags = np.stack([ref["live"], ref["box"], ref["tri"], ref["s"] + 1], 1).astype(np.uint8)
        assert (out["flags"] == want_flags).all(), (name, np.flatnonzero((out["flags"] != want_flags).any(1))[:4])
        want_vals = np.concatenate([ref["t"][:, None], ref["det"][:, None], cc.inv_of(D), ref["lo"], ref["hi"]], 1)
        same = _same_bits(out["vals"], want_vals)
        assert same.all(), (name, np.flatnonzero(~same.all(1))[:4])
        slabs = cc.slab(boxes[:, :, 0], boxes[:, :, 1], O[:, None], cc.inv_of(D)[:, None], tmin[:, None], b[:, None])
        assert (out["boxes"] == slabs).all(), name
        assert (out["boxes"][:, 0] == out["flags"][:, 1]).all(), name       # (box 0 is the own box)
        finite = np.isfinite(O).all(1) & np.isfinite(D).all(1) & ~np.isnan(b)
        own = finite & (out["boxes"][:, 0] == 1)
        checked += int(own.sum())
        violations += int((out["boxes"][own, 1:] == 0).sum())
        acc, live = ref["tri"], ref["live"]
        if name == "random":
            assert 0.3 < acc.mean() < 0.7 and (ref["s"] == 1).sum() > 2000 and (ref["s"] == -1).sum() > 2000, acc.mean()
            assert (acc & ~ref["box"]).sum() == 0           # (near pairs: no phantom)
        if name == "zero_direction":
            assert not acc[2000:2500].any() and live[2000:2500].all()       # an all-zero direction walks and hits nothing
            assert acc[:2000].sum() > 100
        if name == "non_finite":
            assert not live.any()
        if name == "range_ends":
            k = np.arange(len(acc))
            lo_end = (k // 3) % 2 == 0
            # t on the end: out (both ends exclusive); the end one ulp beyond t towards the outside: in; one ulp inside: out
            assert not acc[k % 3 == 0].any()
            assert acc[(k % 3 == 1) & ~lo_end].all() and not acc[(k % 3 == 1) & lo_end].any()     # bound = nextup(t): in; tmin = nextup(t): out
            assert acc[(k % 3 == 2) & lo_end].all() and not acc[(k % 3 == 2) & ~lo_end].any()     # tmin = nextdown(t): in; bound = nextdown(t): out
        if name == "grazing":
            share = out["boxes"][:, 0].mean()
            assert 0.2 < share < 0.999, share               # (the planes ARE the boundary: both verdicts occur)
    assert checked > 15_000 and violations == 0, (checked, violations)


def test_rows_bounds_and_writer_on_the_host(host_exe, cornell_arrays, tmp_path):
    """cx_ray at rows 4 bytes into their allocation in both forms, cx_bound per ray and uniform, cx_live, the loop over ALL triangles of the box
    and cx_write over canaries at exactly their size: count and winding are the restatement's byte for byte, and an output that was not asked
    for does not exist"""
    tris = cc.box_tris(cornell_arrays)
    sets = cc.box_set(cornell_arrays)
    rays, pad = sets["free"].rays, sets["free"].pad
    out = _host_run(host_exe, str(tmp_path / "free"), rays=rays, tris=tris, pad=pad)
    assert out["count"].tobytes() == sets["free"].count.tobytes() and out["winding"].tobytes() == sets["free"].winding.tobytes()
    c = sets["cycled"]
    out = _host_run(host_exe, str(tmp_path / "cycled"), rays=rays, bounds=c.bounds, tris=tris, pad=pad, tmin=cc.TMIN_BOUNDS, want_winding=False)
    assert out["count"].tobytes() == c.count.tobytes() and out["winding"].size == 0
    out = _host_run(host_exe, str(tmp_path / "uniform"), rays=rays, tris=tris, pad=pad, tmin=cc.TMIN_BOUNDS, tmax=2.5, want_count=False)
    assert out["winding"].tobytes() == sets["uniform"].winding.tobytes() and out["count"].size == 0
    d, p = cc.box_points_set(cornell_arrays)
    out = _host_run(host_exe, str(tmp_path / "points"), rays=p.rays[:, :3], direction=d, tris=tris, pad=pad)
    assert out["count"].tobytes() == p.count.tobytes() and out["winding"].tobytes() == p.winding.tobytes()


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------------
def test_restatement_pinned_to_the_oracle(orc, cornell_arrays, cornell_oracle):
    """On the Cornell box's 1 000 rays and a 4 096-triangle soup's 2 000, the restatement's least accepted t (own box or not) and the lowest
    primitive id at it equal the oracle's brute-force closest hit on the same rays: bits of t, and the primitive.  This pins the restatement's
    ray_setup + tri_test to the project's canonical test without touching the oracle."""
    (v, i, f), soup = cc.soup_set()
    cases = [("box", cornell_oracle, cc.box_tris(cornell_arrays), cc.box_set(cornell_arrays)["free"].rays), ("soup", orc.Scene(v, i, f), cc.triangles(v, i), soup.rays)]
    for name, osc, tris, rays in cases:
        hits, _ = osc.trace(rays, tmin=0.001, tmax=10000.0, mode=0)
        ref = cc.Brute(tris, rays, tmin=0.001, tmax=10000.0)
        hit = hits["prim"] != tc.MISS
        assert (hit == (ref.first_prim >= 0)).all(), name
        assert hit.sum() > len(rays) // 3, (name, hit.sum())
        assert hits["t"][hit].view(np.uint32).tobytes() == ref.first_t[hit].view(np.uint32).tobytes(), name
        assert (hits["prim"][hit] == ref.first_prim[hit]).all(), name


def test_premises_of_the_gpu_tests(cornell_arrays):
    """From the restatement alone.  On every ray set tests/test_crossings.py runs on the GPU, the number of triangles that tri_test accepts and
    the own box drops -- recorded here: 0 on each of them, which the equality with PT_TRACE_ANY rests on.  The sets are what they say: every
    count from 0 to 6 occurs on the box, both signs of the winding, rays that do not walk; the cycled bounds change the answers.  On an
    adversarial far-field set (triangles as small as an ulp of the origin) there ARE such phantom triangles, and the definition drops them."""
    sets = cc.box_set(cornell_arrays)
    _, points = cc.box_points_set(cornell_arrays)
    _, moved = cc.box_moved(cornell_arrays)
    _, soup = cc.soup_set()
    named = dict(sets, points=points, moved=moved, soup=soup, big=cc.box_big(cornell_arrays))
    phantoms = {k: int(b.phantoms.sum()) for k, b in named.items()}
    print("phantoms per GPU set:", phantoms)
    assert all(p == 0 for p in phantoms.values()), phantoms
    free = sets["free"]
    assert len(free.rays) == 1000 and (np.bincount(free.count, minlength=7)[:7] > 0).all() and (free.winding > 0).any() and (free.winding < 0).any()
    c = sets["cycled"]
    assert c.count.tobytes() != sets["free_tmin"].count.tobytes() and (c.count[11::13] == 0).all() and (c.count[12::13] == 0).all()
    assert np.isnan(c.bounds[12::13]).all() and (c.bounds[10::13] == cc.TMIN_BOUNDS).all() and (c.count[10::13] == 0).all()
    assert moved.pad > free.pad and moved.count.tobytes() != free.count.tobytes()
    tris, rays = cc.far_field_rays()
    far = cc.Brute(tris, rays)
    print("far field: phantom triangles", int(far.phantoms.sum()), "on", int((far.phantoms > 0).sum()), "rays; counted", int(far.count.sum()))
    assert far.phantoms.sum() >= 50 and far.count.sum() == 0     # (no ray of the set comes within 10^5 triangle sizes of a triangle)


@pytest.mark.parametrize("name", ["cube", "sphere", "torus"])
def test_inside_outside_from_the_restatement(pt, name):
    """1 000 points per closed mesh, farther from the analytic surface than the mesh's chord sag (so polyhedron and solid agree): a single
    direction's parity is wrong on at most 1 % of them, the majority of the first three INSIDE_DIRECTIONS on none; with the meshes oriented
    outwards, winding * sign(D.kz) is -1 inside (the ray leaves through one front face more than it enters) and 0 outside wherever the parity
    is right.  Computed with the restatement, so that the same caps on the GPU cannot hide a kernel error."""
    tris, pts, inside, _ = cc.closed_case(name)
    assert len(pts) == 1000 and 50 <= inside.sum() <= 950
    dirs = np.asarray(pt.INSIDE_DIRECTIONS[:3], f32)
    votes = cc.inside_votes(tris, pts, dirs)
    wrong = (votes != inside[None]).mean(1)
    print(name, "wrong share per direction", wrong)
    assert (wrong <= 0.01).all(), wrong
    assert ((votes.sum(0) * 2 > 3) == inside).all()
    for d, v in zip(dirs, votes):
        b = cc.Brute(tris, np.concatenate([pts, np.broadcast_to(d, pts.shape)], 1))
        good = v == inside
        w = b.winding * int(np.sign(d[np.abs(d).argmax()]))
        assert (w[good & inside] == -1).all() and (w[good & ~inside] == 0).all()


def test_winding_sign_known_answer():
    """One triangle A = (0, 0, 0), B = (1, 0, 0), C = (0, 1, 0): cross(B - A, C - A) = +z.  A ray travelling along -z meets its front, a ray
    along +z its back.  det has the sign of -(cross . D) * D.kz: the ray along -z (dominant component negative, cross . D < 0) gives -1, the ray
    along +z (dominant positive, cross . D > 0) gives -1 as well; rays with the dominant axis x show the two signs apart."""
    A, B, C = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    P = np.asarray([0.25, 0.25, 0], f32)
    for D, want in (([0.1, 0.2, -1.0], -1), ([0.1, 0.2, 1.0], -1), ([1.0, 0.2, 0.5], -1), ([1.0, 0.2, -0.5], 1), ([-1.0, 0.2, 0.5], 1), ([-1.0, 0.2, -0.5], -1)):
        D = np.asarray(D, f32)
        r = cc.pair_verdicts((P - D).astype(f32), D, f32(0), f32(np.inf), A, B, C, f32(1e-5))
        n_dot_d = float(np.cross(B - A, C - A) @ D)
        assert r["tri"] and r["box"] and int(r["s"]) == want == int(-np.sign(n_dot_d) * np.sign(D[np.abs(D).argmax()])), (D, r["s"])
