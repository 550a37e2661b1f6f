"""The PLOC rebuild of a binary tree (csrc/ploc_build.hip) restated in numpy, and the fixtures the PLOC tests share.

The clustering is fully specified binary32 (the library is compiled without contraction), so the restatement is exact: the same
neighbour choices, the same merges, the same boxes.  Only the area SUMS are float64 additions in another order than the device's
(per-block tree reduction, blocks added in order), which moves them by at most (n - 1) * 2^-53 relative.

Inputs come from the CPU oracle's LBVH (orc.Scene.bvh_nodes(), which the suite pins to the device's read-back bit for bit): a row is
{left lo xyz, left hi xyz, right lo xyz, right hi xyz, left word, right word, 0, 0}; a child word with bit 31 names the sorted position of a
leaf, whose padded box is the one stored beside it; an internal node's box is the union of its two child boxes."""
import numpy as np

f32 = np.float32
LEAF = 0x80000000
TB = 256                 # threads per block of k_ploc_nn
PLOC_R_MAX = 32
PLOC_MIN_TRIS = 2049     # scenes above PT_SAH_MAX_TRIS = 2048 triangles get the rebuild
RADII = (-1, 1, 8, 31, 32)
ADOPT_PCTS = (-1, 0, 95, 1000)


def tuned(v, dflt, lo, hi):
    """pt_internal.h pt_tuned"""
    return dflt if v < 0 else min(max(v, lo), hi)


def area(lo, hi):
    """box_area / union_area: (x*y + y*z) + z*x, every product and sum rounded to binary32; lo, hi [..., 3] float32"""
    d = (hi - lo).astype(f32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return (((x * y).astype(f32) + (y * z).astype(f32)).astype(f32) + (z * x).astype(f32)).astype(f32)


def lbvh_boxes(nodes):
    """oracle / read-back LBVH rows [n - 1, 16] u32 -> (leaf lo, leaf hi [n, 3] in sorted order, node lo, node hi [n - 1, 3])"""
    nodes = np.asarray(nodes, np.uint32)
    n_int = nodes.shape[0]
    n = n_int + 1
    fl = nodes[:, :12].copy().view(f32).reshape(n_int, 4, 3)           # lmin lmax rmin rmax
    llo, lhi = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    seen = np.zeros(n, np.int64)
    for side in (0, 1):
        w = nodes[:, 12 + side]
        m = (w & LEAF) != 0
        pos = (w[m] & 0x7FFFFFFF).astype(np.int64)
        llo[pos], lhi[pos] = fl[m, 2 * side], fl[m, 2 * side + 1]
        np.add.at(seen, pos, 1)
    assert (seen == 1).all()
    nlo = np.minimum(fl[:, 0], fl[:, 2])
    nhi = np.maximum(fl[:, 1], fl[:, 3])
    return llo, lhi, nlo, nhi


def area_sum(lo, hi):
    """float64 sum of the float32 areas of boxes [k, 3]"""
    return float(area(lo, hi).astype(np.float64).sum())


def lbvh_area(nodes):
    _, _, nlo, nhi = lbvh_boxes(nodes)
    return area_sum(nlo, nhi)


def nearest(lo, hi, radius, tie="even"):
    """k_ploc_nn over the cluster arrays lo, hi [m, 3]: offsets walked ascending from -radius to radius, a candidate replaces the best on
    bj < 0 || a < best || (a == best && par < bpar), par = min(i, j) & 1 -> nn [m] int64.  tie: "even" is the kernel's rule; "odd" (the
    parity compared the other way) and "none" (no parity term) are the wrong rules the CPU tests hold it against."""
    m = len(lo)
    idx = np.arange(m)
    best = np.full(m, np.inf, f32)
    bj = np.full(m, -1, np.int64)
    bpar = np.zeros(m, np.int64)
    for d in range(-radius, radius + 1):
        if d == 0:
            continue
        j = idx + d
        ok = (j >= 0) & (j < m)
        jc = np.clip(j, 0, m - 1)
        a = area(np.minimum(lo, lo[jc]), np.maximum(hi, hi[jc]))
        par = np.minimum(idx, jc) & 1
        wins = par < bpar if tie == "even" else par > bpar if tie == "odd" else np.zeros(m, bool)
        take = ok & ((bj < 0) | (a < best) | ((a == best) & wins))
        best = np.where(take, a, best)
        bj = np.where(take, j, bj)
        bpar = np.where(take, par, bpar)
    return bj


def ploc(llo, lhi, radius, tie="even", block=None):
    """ptb_ploc_refine's rounds over leaf boxes in Morton order (tie, block: deliberately wrong variants, see nearest) -> dict: area (float64 sum of the merged boxes' float32 areas), merges
    per round, and the tree as children [n - 1, 2] in creation order (a child c < n is leaf position c, else merge c - n)"""
    lo, hi = np.asarray(llo, f32).copy(), np.asarray(lhi, f32).copy()
    ref = np.arange(len(lo), dtype=np.int64)
    n = len(lo)
    total, rounds, kids = 0.0, [], []
    while len(lo) > 1:
        m = len(lo)
        if block is None:
            nn = nearest(lo, hi, radius, tie)
        else:   # a wrong kernel that sees no neighbour outside its own block of `block` clusters
            nn = np.concatenate([b + nearest(lo[b:b + block], hi[b:b + block], radius, tie) if min(block, m - b) > 1 else
                                 np.asarray([b - 1 if b else 1]) for b in range(0, m, block)])
        idx = np.arange(m)
        mutual = nn[nn] == idx
        lower = mutual & (idx < nn)
        upper = mutual & (nn < idx)
        assert lower.any(), "a PLOC round without a merge"
        li, ui = idx[lower], nn[lower]
        mlo, mhi = np.minimum(lo[li], lo[ui]), np.maximum(hi[li], hi[ui])
        total += area_sum(mlo, mhi)
        new = n + len(kids) + np.arange(len(li))
        kids += list(zip(ref[li].tolist(), ref[ui].tolist()))
        lo[li], hi[li], ref[li] = mlo, mhi, new
        keep = ~upper
        lo, hi, ref = lo[keep], hi[keep], ref[keep]
        rounds.append(int(lower.sum()))
    return dict(area=total, rounds=rounds, children=np.asarray(kids, np.int64).reshape(-1, 2))


def root_area(bmin, bmax):
    """pt_scene_get_info's normalisation: the scene box's (x*y + y*z) + z*x in double from its float32 corners"""
    e = np.asarray(bmax, f32).astype(np.float64) - np.asarray(bmin, f32).astype(np.float64)
    return float((e[0] * e[1] + e[1] * e[2]) + e[2] * e[0])


def info_value(total, root):
    """an area sum as pt_scene_info reports it"""
    return f32(total / root) if root > 0.0 else f32(0.0)


def within_one_ulp(got, want):
    got, want = f32(got), f32(want)
    return bool(got == want or got == np.nextafter(want, f32(np.inf)) or got == np.nextafter(want, f32(-np.inf)))


def adopted(area_ploc, area_lbvh, pct):
    """ploc_build.hip's rule, as written there"""
    return bool(area_ploc < 0.01 * tuned(pct, 90, 0, 1000) * area_lbvh)


def tri_boxes(v, i):
    p = np.asarray(v, f32).reshape(-1, 3)[np.asarray(i).reshape(-1, 3)]
    return p.min(1), p.max(1)


def refit_lbvh(nodes, prim_of_pos, v, i):
    """The binary LBVH `nodes` (its child words and sorted order kept) refitted to the triangles (v, i), as pt_scene_update's REFIT does
    it (lbvh_build.hip ptb_refit_lbvh): leaves = triangle boxes padded by 2^-18 of the largest |coordinate| of the new scene box,
    internal boxes = unions bottom-up -> (rows like `nodes` with the new boxes, float64 area sum of the internal boxes)"""
    nodes = np.asarray(nodes, np.uint32)
    tlo, thi = tri_boxes(v, i)
    pad = f32(max(np.abs(tlo.min(0)).max(), np.abs(thi.max(0)).max())) * f32(3.814697265625e-06)
    order = np.asarray(prim_of_pos, np.int64)
    llo, lhi = (tlo[order] - pad).astype(f32), (thi[order] + pad).astype(f32)
    n_int = nodes.shape[0]
    nlo, nhi = np.zeros((n_int, 3), f32), np.zeros((n_int, 3), f32)
    out = nodes.copy()
    fl = np.zeros((n_int, 4, 3), f32)
    done = np.zeros(n_int, bool)
    # children first: an explicit stack instead of recursion (a Morton tree over duplicates can be deep)
    stack = [0]
    while stack:
        nd = stack[-1]
        kids = [int(nodes[nd, 12]), int(nodes[nd, 13])]
        wait = [k for k in kids if not (k & LEAF) and not done[k]]
        if wait:
            stack += wait
            continue
        stack.pop()
        for side, k in enumerate(kids):
            if k & LEAF:
                fl[nd, 2 * side], fl[nd, 2 * side + 1] = llo[k & 0x7FFFFFFF], lhi[k & 0x7FFFFFFF]
            else:
                fl[nd, 2 * side], fl[nd, 2 * side + 1] = nlo[k], nhi[k]
        nlo[nd], nhi[nd] = np.minimum(fl[nd, 0], fl[nd, 2]), np.maximum(fl[nd, 1], fl[nd, 3])
        done[nd] = True
    assert done.all()
    out[:, :12] = fl.reshape(n_int, 12).view(np.uint32)
    return out, area_sum(nlo, nhi)


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------
def soup(n, seed, spread=0.1):
    """tests/test_gpu_parity.py::_soup"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)).astype(f32)
    v = (c + rng.uniform(-spread, spread, (n, 3, 3)).astype(f32)).astype(f32)
    faces = rng.uniform(0, 1, (n, 6)).astype(f32)
    faces[:, 3:] *= (rng.uniform(0, 1, (n, 1)) < 0.1)
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), faces.reshape(-1).astype(f32)


def tile_grid(nx=48, ny=24):
    """nx x ny equal square quads of side 1/32 in the plane z = 0, from (-nx/64, -2) upwards, two triangles each with vertices of their
    own: every leaf box is the same size, so union areas tie all over and the parity term of the pair key decides.  48 x 24 -> 2304
    triangles = nine full blocks of k_ploc_nn.  Coordinates are multiples of 2^-5 and the largest |coordinate| is 2, so the leaf pad
    is 2^-17 and every padded box and every union area is exact in binary32: equal tiles tie bit for bit."""
    s = f32(1.0 / 32.0)
    verts, faces = [], []
    for y in range(ny):
        for x in range(nx):
            x0, y0 = f32(-nx / 64.0) + f32(x) * s, f32(-2.0) + f32(y) * s
            x1, y1 = f32(-nx / 64.0) + f32(x + 1) * s, f32(-2.0) + f32(y + 1) * s
            a, b, c, d = (x0, y0, 0.0), (x1, y0, 0.0), (x1, y1, 0.0), (x0, y1, 0.0)
            verts += [a, b, c, a, c, d]
            kd = (0.2 + 0.6 * ((x + y) & 1), 0.5, 0.3 + 0.4 * (x % 3 == 0))
            ke = (2.0, 2.0, 2.0) if (x % 11 == 5 and y % 7 == 3) else (0.0, 0.0, 0.0)
            faces += [kd + ke] * 2
    v = np.asarray(verts, f32).reshape(-1)
    return v, np.arange(len(v) // 3, dtype=np.uint32), np.asarray(faces, f32).reshape(-1)


FIXTURES = ("stadium", "soup2049", "soup2305", "tiles")
_arrays, _refs = {}, {}


def arrays(pt, name):
    """-> (vertices, indices, faces) of a named fixture, made once per session"""
    if name not in _arrays:
        _arrays[name] = {"stadium": lambda: pt.make_stadium(24, 24), "soup2049": lambda: soup(2049, 7, 0.3),
                         "soup2305": lambda: soup(2305, 8, 0.1), "tiles": tile_grid}[name]()
    return _arrays[name]


def reference(orc, v, i, f, radius, key=None):
    """The restatement's answer for a scene at a (tuned) radius, once per session when keyed -> dict: area_lbvh, area_ploc (float64
    sums), root (the box's area), ratio, rounds, children"""
    k = None if key is None else (key, radius)
    if k is not None and k in _refs:
        return _refs[k]
    osc = orc.Scene(v, i, f)
    nodes = osc.bvh_nodes()
    llo, lhi, nlo, nhi = lbvh_boxes(nodes)
    bi = osc.bvh_info()
    r = ploc(llo, lhi, radius)
    out = dict(area_lbvh=area_sum(nlo, nhi), area_ploc=r["area"], root=root_area(list(bi.bbox_min), list(bi.bbox_max)), rounds=r["rounds"],
               children=r["children"], n=len(llo))
    out["ratio"] = out["area_ploc"] / out["area_lbvh"]
    if k is not None:
        _refs[k] = out
    return out


def fixture_reference(pt, orc, name, radius_knob):
    return reference(orc, *arrays(pt, name), tuned(radius_knob, 8, 1, PLOC_R_MAX), key=name)
