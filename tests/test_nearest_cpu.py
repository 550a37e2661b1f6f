"""pt_nearest_device without a GPU (include/pt_api.h): the ABI and the names; the statements that define the result
(csrc/nearest_kernel.h) compiled for the host (tests/nearest_host.cpp) and run as a program -- plain and under the address and
undefined-behaviour sanitizers -- bit for bit against the numpy restatement of tests/nearest_cases.py, with the pruning lemma checked on every
pair; the restatement against a float64 brute force; and the query sets of tests/test_nearest.py judged from the restatement alone."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import nearest_cases as nc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_nearest_abi_and_names(pt, tmp_path):
    """By gcc from the header: sizeof(pt_nearest_desc) == 64, sizeof(pt_nearest) == 16, the three enum values, PT_API_VERSION == 6, the two
    prototypes; the names in API_SYMBOLS and in the built library; the Python constants; nearest_tensors refuses an unknown form before it
    touches a device; NULL handles are PT_ERR_INVALID_ARG."""
    src = tmp_path / "nr_abi.c"
    vals = ["sizeof(pt_nearest_desc)", "sizeof(pt_nearest)", "(size_t)PT_NEAREST_AUTO", "(size_t)PT_NEAREST_LDS", "(size_t)PT_NEAREST_GLOBAL",
            "(size_t)PT_API_VERSION", "offsetof(pt_nearest_desc, max_dist)", "offsetof(pt_nearest_desc, reserved)", "offsetof(pt_nearest, v)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\n'
                   "void (*p_default)(pt_nearest_desc *) = pt_nearest_desc_default;\n"
                   "pt_status (*p_call)(pt_scene *, const pt_nearest_desc *, uint64_t, float *) = pt_nearest_device;\n"
                   'int main(void){printf("' + "%zu " * len(vals) + '\\n",' + ", ".join(vals) + ");return p_default == 0 || p_call == 0;}\n")
    exe = tmp_path / "nr_abi"
    lib_dir = os.path.dirname(pt.__file__)
    subprocess.check_call([shutil.which("gcc") or "gcc", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src),
                           "-L", lib_dir, "-l:libpt_amd.so", "-Wl,-rpath," + lib_dir])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [64, 16, 0, 1, 2, 6, 32, 44, 12], got
    L = pt.lib_amd()
    for name in ("pt_nearest_desc_default", "pt_nearest_device"):
        assert name in pt.API_SYMBOLS and hasattr(L, name), name
    assert (pt.NEAREST_AUTO, pt.NEAREST_LDS, pt.NEAREST_GLOBAL) == (0, 1, 2)
    assert pt.NEAREST_DTYPE.itemsize == 16 and pt.NEAREST_DTYPE == nc.NEAREST_DTYPE and ctypes.sizeof(pt.NearestDesc) == 64
    d = pt.nearest_default_desc()
    assert d.max_dist == np.inf and d.form == 0 and d.flags == 0 and not any(d.reserved) and not d.d_points and not d.d_nearest
    with pytest.raises(ValueError):
        pt.Scene.nearest_tensors(None, None, form="fused")       # (no scene, no tensor: the form is judged first)
    assert L.pt_nearest_device(None, ctypes.byref(d), 1, None) == 1   # PT_ERR_INVALID_ARG
    L.pt_nearest_desc_default(None)                                    # (a no-op)


# ---- the host program ---------------------------------------------------------------------------------------------------------------------
def _write(d, name, a, dt=f32):
    np.ascontiguousarray(a, dt).tofile(os.path.join(d, name))


def _host_run(exe, d, pairs=None, boxes=None, points=None, radii=None, tris=None, max_dist=np.inf, want_nearest=True, want_point=True):
    os.makedirs(d, exist_ok=True)
    pairs = np.zeros((0, 4, 3), f32) if pairs is None else pairs
    boxes = np.zeros((len(pairs), 0, 2, 3), f32) if boxes is None else boxes
    points = np.zeros((0, 3), f32) if points is None else points
    tris = np.zeros((0, 3, 3), f32) if tris is None else tris
    n, k, m = len(pairs), boxes.shape[1], len(points)
    _write(d, "par", [n, k, m, len(tris), int(radii is not None), int(want_nearest), int(want_point), int(f32(max_dist).view(np.uint32))], np.uint32)
    _write(d, "pairs", pairs)
    _write(d, "boxes", boxes)
    _write(d, "points", np.concatenate([np.asarray([123.0], f32), np.asarray(points, f32).reshape(-1)]))   # rows start one float into the allocation
    _write(d, "radii", np.zeros(0, f32) if radii is None else radii)
    _write(d, "tris", tris)
    subprocess.check_call([exe, d])
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    return {"pairs": rd("o_pairs", f32).reshape(n, 6), "region": rd("o_region", np.int32), "boxes": rd("o_boxes", f32).reshape(n, k),
            "points": rd("o_points", f32).reshape(m, 3), "r2": rd("o_r2", f32), "nearest": rd("o_nearest", np.uint8), "point": rd("o_point", f32)}


def _same_bits(a, b):
    """bit for bit; a NaN equals a NaN (its sign and payload are the divider's business)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _random_pairs(n, seed):
    """triangles with vertices uniform in [-1, 1]^3, points uniform in [-2, 2]^3 -> [n, 4, 3] {P, A, B, C}"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, (n, 3, 3)).astype(f32)
    p = rng.uniform(-2, 2, (n, 1, 3)).astype(f32)
    return np.concatenate([p, t], 1)


def _pair_sets():
    rng = np.random.default_rng(5)
    sets = {"random": _random_pairs(20_000, 4)}
    far = _random_pairs(2000, 6)
    sets["near_1e6"] = (far + f32(1e6)).astype(f32)                                  # coordinates near 1e6: eight ulps of 0.0625 per unit
    sets["denormal"] = (_random_pairs(2000, 7) * f32(1e-41)).astype(f32)             # every coordinate a denormal
    base = _random_pairs(3000, 8)
    on = base.copy()
    k = np.arange(3000)
    on[:1000, 0] = base[k[:1000], 1 + k[:1000] % 3]                                  # P exactly on a vertex
    a, b = base[k[1000:2000], 1 + k[1000:2000] % 3], base[k[1000:2000], 1 + (k[1000:2000] + 1) % 3]
    w = rng.uniform(0, 1, (1000, 1)).astype(f32)
    w[::4] = f32(0.5)
    on[1000:2000, 0] = (a + (b - a) * w).astype(f32)                                 # on an edge (as close as binary32 puts it)
    bc = rng.dirichlet((1, 1, 1), 1000).astype(f32)
    on[2000:, 0] = (base[2000:, 1:] * bc[:, :, None]).sum(1).astype(f32)             # in the plane, inside
    sets["on_triangle"] = on
    deg = _random_pairs(3000, 9)
    deg[:1000, 3] = deg[:1000, 2]                                                    # two equal vertices
    deg[500:1000, 2] = deg[500:1000, 1]
    t = rng.uniform(-1, 2, (1000, 1)).astype(f32)
    deg[1000:2000, 3] = (deg[1000:2000, 1] + (deg[1000:2000, 2] - deg[1000:2000, 1]) * t).astype(f32)   # three collinear (to rounding)
    deg[1000:1200, 1:] = np.round(deg[1000:1200, 1:2] * 4) / 4 + np.asarray([[[0, 0, 0]], [[1, 2, 3]], [[2, 4, 6]]], f32).reshape(1, 3, 3) * f32(0.25)   # exactly collinear
    deg[2000:, 2] = deg[2000:, 1]                                                    # all equal
    deg[2000:, 3] = deg[2000:, 1]
    sets["degenerate"] = deg.astype(f32)
    return sets


def _boxes_of(pairs, seed):
    """per pair: the triangle's own box and three grown by random amounts (>= 0, some 0, some huge) -> [n, 4, 2, 3]"""
    rng = np.random.default_rng(seed)
    tri = pairs[:, 1:]
    lo, hi = tri.min(1), tri.max(1)
    out = np.zeros((len(pairs), 4, 2, 3), f32)
    out[:, 0, 0], out[:, 0, 1] = lo, hi
    scale = np.maximum(np.abs(pairs).max((1, 2)), f32(1e-45))[:, None]
    for k, mag in enumerate((1e-6, 0.1, 100.0), 1):
        g = (rng.uniform(0, mag, (len(pairs), 2, 3)) * (rng.uniform(0, 1, (len(pairs), 2, 3)) < 0.8)).astype(f32) * scale[:, None]
        out[:, k, 0], out[:, k, 1] = (lo - g[:, 0]).astype(f32), (hi + g[:, 1]).astype(f32)
    assert (out[:, :, 0] <= lo[:, None]).all() and (out[:, :, 1] >= hi[:, None]).all()   # (they contain the vertices as float32 numbers)
    return out


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def host_exe(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nearest_host") / "nearest_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "nearest_host.cpp")])
    return exe


def test_closest_point_and_lemma_on_the_host(host_exe, tmp_path):
    """nr_closest and nr_box_dist2 as a program, bit for bit against the restatement (u, v, Q, dist2, the branch taken, the box distances) on
    20 000 random pairs, pairs near 1e6, denormal pairs, P on vertices / edges / in the plane, degenerate triangles.  Each of the seven branches
    answers at least 100 of the random pairs.  The lemma: dist2 >= the box distance to the triangle's own box and to three grown ones, on every
    pair whose dist2 is not NaN -- zero violations; the NaN pairs are counted, none in the random set (below 1 % asked)."""
    violations = 0
    for name, pairs in _pair_sets().items():
        boxes = _boxes_of(pairs, 11)
        out = _host_run(host_exe, str(tmp_path / name), pairs=pairs, boxes=boxes)
        u, v, Q, d2, region = nc.closest(pairs[:, 0], pairs[:, 1], pairs[:, 2], pairs[:, 3])
        want = np.concatenate([u[:, None], v[:, None], Q, d2[:, None]], 1)
        same = _same_bits(out["pairs"], want)
        assert same.all(), (name, np.flatnonzero(~same.all(1))[:4])
        assert (out["region"] == region).all(), name
        bd = nc.box_dist2(pairs[:, None, 0], boxes[:, :, 0], boxes[:, :, 1])
        assert (out["boxes"].view(np.uint32) == bd.view(np.uint32)).all() and not np.isnan(bd).any(), name
        nan = np.isnan(d2)
        violations += int((out["boxes"][~nan] > d2[~nan, None]).sum())
        if name == "random":
            counts = np.bincount(region, minlength=7)
            assert (counts >= 100).all(), dict(zip(nc.REGIONS, counts))
            assert nan.mean() < 0.01 and nan.sum() == 0, nan.sum()
        if name == "degenerate":
            assert nan.sum() > 0   # (the interior branch of a degenerate triangle: 0 / 0)
        if name == "on_triangle":
            # (P on vertex A is exactly 0; on B or C, Q = (A + ab * 1) + ac * 0 is the vertex only to rounding)
            # that the set is what it says, not a bound on the algorithm: near-zero everywhere (an edge point that rounding puts beside the
            # edge can fall into the interior branch with a small s: 3.7e-8 is the largest dist2 of the set)
            assert (d2[:1000:3] == 0).all() and (d2[:1000] < 1e-12).all() and (d2 < 1e-6).all()
    assert violations == 0, violations


def test_rows_radii_accept_and_writers_on_the_host(host_exe, cornell_arrays, tmp_path):
    """nr_point at rows 4 bytes into their allocation; nr_radius / nr_radius2 over 0, tiny, +inf, negative, NaN, -0 (per query and uniform);
    nr_accept as the loop over ALL triangles of the box, and the two writers over canaries at exactly their size: the records and points are the
    restatement's byte for byte, the miss record's bytes included, and an output that was not asked for does not exist."""
    tris = nc.box_tris(cornell_arrays)
    sets = nc.box_set(cornell_arrays)
    q = sets["free"].points
    n = 257
    radii = np.asarray([0.0, 1e-30, np.inf, -1.0, np.nan, -0.0, 1e-3, 0.1], f32)[np.arange(n) % 8]
    out = _host_run(host_exe, str(tmp_path / "radii"), points=q[:n], radii=radii, tris=tris)
    assert out["points"].tobytes() == q[:n].tobytes()
    with np.errstate(all="ignore"):
        want_r2 = np.where(radii >= 0, radii * radii, f32(-1)).astype(f32)
    assert out["r2"].tobytes() == want_r2.tobytes()
    ref = nc.Brute(tris, q[:n], radii)
    assert out["nearest"].tobytes() == ref.rec.tobytes() and out["point"].tobytes() == ref.point.tobytes()
    miss = ~ref.found
    assert miss[3::8].all() and miss[4::8].all() and 0 < miss.sum() < n
    assert (out["nearest"].view(np.uint32).reshape(n, 4)[miss] == [nc.MISS, 0, 0, 0]).all() and (out["point"].reshape(n, 3)[miss].view(np.uint32) == 0).all()
    # the session's sets: cycled radii per query; the uniform radius through max_dist, each output alone; unbounded
    m = len(q)
    out = _host_run(host_exe, str(tmp_path / "cycled"), points=q, radii=nc.cycled_radii(m), tris=tris)
    assert out["nearest"].tobytes() == sets["cycled"].rec.tobytes() and out["point"].tobytes() == sets["cycled"].point.tobytes()
    out = _host_run(host_exe, str(tmp_path / "uniform_a"), points=q, tris=tris, max_dist=0.1, want_point=False)
    assert out["nearest"].tobytes() == sets["uniform"].rec.tobytes() and out["point"].size == 0
    assert (out["r2"] == f32(0.1) * f32(0.1)).all()
    out = _host_run(host_exe, str(tmp_path / "uniform_b"), points=q, tris=tris, max_dist=0.1, want_nearest=False)
    assert out["point"].tobytes() == sets["uniform"].point.tobytes() and out["nearest"].size == 0
    out = _host_run(host_exe, str(tmp_path / "free"), points=q, tris=tris)
    assert out["nearest"].tobytes() == sets["free"].rec.tobytes() and out["point"].tobytes() == sets["free"].point.tobytes()
    assert sets["free"].found.all()


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------------
EXCESS_MEASURED = 2.220446049250313e-16   # see the docstring below


def test_restatement_against_float64_brute_force(cornell_arrays):
    """4 096 uniform queries in 1.5x the Cornell box: the float64 distance to the restatement's winning primitive may exceed the float64
    minimum over all triangles by at most a margin, which covers the restatement's binary32 rounding (it is not a property of the kernel).
    Measured maximum excess: 2.22e-16 = EXCESS_MEASURED (absolute, scene units; the box is about 2 units wide: one ulp of float64 there --
    the restatement's winner is the float64 winner on all 4 096, up to which of two coincident quads float64 prefers); asserted at 4x that value."""
    tris = nc.box_tris(cornell_arrays)
    lo, hi = nc.scene_box(tris)
    q = np.random.default_rng(31).uniform(lo, hi, (4096, 3)).astype(f32)
    ref = nc.Brute(tris, q)
    assert ref.found.all()
    d64 = nc.dist_f64(q, tris)
    excess = d64[np.arange(len(q)), ref.rec["prim"]] - d64.min(1)
    print("max excess", excess.max(), "max |sqrt(dist2) - d64|", np.abs(np.sqrt(ref.rec["dist2"].astype(np.float64)) - d64.min(1)).max())
    assert excess.min() >= 0 and excess.max() <= 4 * EXCESS_MEASURED, excess.max()
    assert np.abs(np.sqrt(ref.rec["dist2"].astype(np.float64)) - d64.min(1)).max() < 1e-5


def test_query_sets_from_the_restatement_alone(cornell_arrays):
    """The sets tests/test_nearest.py runs on the GPU, judged without one.  On the box, small and big set: between 5 % and 95 % of the queries
    are answered by a face region ("interior") and the rest by an edge or vertex region; at least 50 queries tie exactly in dist2 between
    different primitives (shared edges and vertices, the box's coincident quads); under the cycled radii every finite non-negative radius
    except 0 sees both found and not found, a negative or NaN radius finds nothing, +inf finds everything.  The moved box answers differently;
    the soup's set is found everywhere."""
    sets = nc.box_set(cornell_arrays)
    big = nc.box_big(cornell_arrays)
    assert len(sets["free"].points) == 1000 and len(big.points) == nc.BIG_N == 200_001
    for name, b in (("box", sets["free"]), ("big", big)):
        assert b.found.all()
        interior = float((b.region == 6).mean())
        assert 0.05 < interior < 0.95, (name, interior)
        assert (b.ties >= 2).sum() >= 50, (name, (b.ties >= 2).sum())
    c = sets["cycled"]
    for k, r in enumerate(nc.RADII):
        found = c.found[k::6]
        if np.isfinite(r) and r > 0:
            assert 0 < found.sum() < len(found), (float(r), found.sum())
        elif r == np.inf:
            assert found.all()
        elif not r >= 0:
            assert not found.any()
    assert 0 < sets["uniform"].found.sum() < 1000
    _, moved = nc.box_moved(cornell_arrays)
    assert moved.rec.tobytes() != sets["free"].rec.tobytes()
    _, soup = nc.soup_set()
    assert soup.found.all() and len(soup.points) == 2000
