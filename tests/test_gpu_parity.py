"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C-ABI,
against the CPU oracle on the same inputs.  Bar: BIT-EXACT float radiance, hit records, ray
counts and LBVH (the project's canonical arithmetic is fully specified)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _soup(n, seed, spread=0.1):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)).astype(np.float32)
    v = (c + rng.uniform(-spread, spread, (n, 3, 3)).astype(np.float32)).astype(np.float32)
    faces = rng.uniform(0, 1, (n, 6)).astype(np.float32)
    faces[:, 3:] *= (rng.uniform(0, 1, (n, 1)) < 0.1)
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), faces.reshape(-1).astype(np.float32)


def _render_oracle(orc, osc, frames, **kw):
    """-> (film f32, bgra8, rays) after `frames` frames through the oracle."""
    film = bgra = None
    rays = 0
    for k in range(frames):
        p = orc.default_params(frame=k, **kw)
        img, r, _, _ = osc.render_frame(p)
        if film is None:
            film = np.zeros_like(img)
            bgra = np.zeros(img.shape[:2] + (4,), np.uint8)
        orc.accumulate_f32(film, img, k)
        orc.accumulate_bgra8(bgra, img, k)
        rays += r
    return film, bgra, rays


def test_lbvh_build_matches_oracle_cornell(pt, orc, cornell_gpu, cornell_oracle):
    keys, prim, nodes = cornell_gpu.read_bvh()
    okeys, oprim = cornell_oracle.bvh_keys()
    onodes = cornell_oracle.bvh_nodes()
    assert (keys == okeys).all() and (prim == oprim).all()
    assert nodes.tobytes() == onodes.tobytes()
    gi, oi = cornell_gpu.info(), cornell_oracle.bvh_info()
    assert (gi.n_tris, gi.n_nodes, gi.bvh_height) == (oi.n_tris, oi.n_nodes, oi.height) == (36, 35, oi.height)
    assert list(gi.bbox_min) == list(oi.bbox_min) and list(gi.bbox_max) == list(oi.bbox_max)


@pytest.mark.parametrize("n,seed", [(1, 1), (2, 2), (3, 3), (257, 4), (5000, 5), (200000, 6)])
def test_lbvh_build_matches_oracle_soup(pt, orc, gpu_ctx, n, seed):
    v, i, f = _soup(n, seed)
    if n == 257:  # duplicated triangles -> duplicate Morton keys -> Karras' index tie-break
        v = np.concatenate([v.reshape(n, 9)[:128], v.reshape(n, 9)[:128], v.reshape(n, 9)[256:]]).reshape(-1)
    gs = pt.Scene(gpu_ctx, v, i, f)
    osc = orc.Scene(v, i, f)
    keys, prim, nodes = gs.read_bvh()
    okeys, oprim = osc.bvh_keys()
    assert (keys == okeys).all() and (prim == oprim).all()
    assert (np.diff(keys.astype(np.int64)) >= 0).all()  # sortedness
    assert nodes.tobytes() == osc.bvh_nodes().tobytes()
    assert gs.info().bvh_height == osc.bvh_info().height
    gs.close()


def _collapse_reference(nodes, n_tris, leaf_max=4):
    """Python restatement of the BVH4 collapse rule (csrc/lbvh_build.hip, step 7) applied to the
    ORACLE's binary LBVH: even-depth nodes with > leaf_max triangles become wide nodes, odd-depth
    internal children are absorbed, subtrees with <= leaf_max triangles become one leaf child."""
    LEAF = 0x80000000
    n_int = nodes.shape[0]
    fl = nodes.view(np.float32)
    left, right = nodes[:, 12].astype(np.int64), nodes[:, 13].astype(np.int64)
    rng, depth = {}, {0: 0}

    def walk(i, d):
        stack = [(i, d, 0)]
        while stack:
            i, d, st = stack.pop()
            if st == 0:
                depth[i] = d
                stack.append((i, d, 1))
                for c in (left[i], right[i]):
                    if not c & LEAF:
                        stack.append((int(c), d + 1, 0))
            else:
                lo, hi = [], []
                for c in (left[i], right[i]):
                    if c & LEAF:
                        lo.append(int(c & ~LEAF)); hi.append(int(c & ~LEAF))
                    else:
                        lo.append(rng[int(c)][0]); hi.append(rng[int(c)][1])
                rng[i] = (min(lo), max(hi))
    walk(0, 0)
    cnt = lambda i: rng[i][1] - rng[i][0] + 1
    flag = [i == 0 or (cnt(i) > leaf_max and depth[i] % 2 == 0) for i in range(n_int)]
    widx = np.cumsum([0] + flag[:-1])

    def box_of(parent, side):      # child box as stored in the binary parent
        o = 0 if side == 0 else 6
        return fl[parent, o:o + 3], fl[parent, o + 3:o + 6]

    def child(parent, side):
        c = int(left[parent] if side == 0 else right[parent])
        lo, hi = box_of(parent, side)
        if c & LEAF:
            return LEAF | (c & ~LEAF), lo, hi
        if cnt(c) <= leaf_max:
            return LEAF | ((cnt(c) - 1) << 28) | rng[c][0], lo, hi
        return None, lo, hi        # internal, not leaf-like

    out = np.zeros((int(sum(flag)), 32), np.uint32)
    of = out.view(np.float32)
    for i in range(n_int):
        if not flag[i]:
            continue
        slots = []
        if cnt(i) <= leaf_max:     # tiny scene: root is one leaf; its box = union of its children
            lo = np.minimum(fl[i, 0:3], fl[i, 6:9]); hi = np.maximum(fl[i, 3:6], fl[i, 9:12])
            slots.append((LEAF | ((cnt(i) - 1) << 28) | rng[i][0], lo, hi))
        else:
            for side in (0, 1):
                w, lo, hi = child(i, side)
                c = int(left[i] if side == 0 else right[i])
                if w is not None:
                    slots.append((w, lo, hi))
                else:
                    for s2 in (0, 1):
                        w2, lo2, hi2 = child(c, s2)
                        g = int(left[c] if s2 == 0 else right[c])
                        slots.append((w2 if w2 is not None else int(widx[g]), lo2, hi2))
        row = int(widx[i])
        of[row, 0:12] = np.inf
        of[row, 12:24] = np.inf
        out[row, 24:28] = 0xFFFFFFFF
        for k, (w, lo, hi) in enumerate(slots):
            for ax in range(3):
                of[row, 4 * ax + k] = lo[ax]
                of[row, 12 + 4 * ax + k] = hi[ax]
            out[row, 24 + k] = w
    return out


@pytest.mark.parametrize("n,seed", [(1, 1), (2, 2), (4, 3), (5, 4), (37, 5), (3000, 6), (60000, 7)])
def test_bvh4_collapse_matches_reference_rule(pt, orc, gpu_ctx, n, seed):
    v, i, f = _soup(n, seed)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    gs.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)   # the collapsed LBVH (small scenes default to the SAH BVH4)
    assert gs.info().bvh4_builder == 0
    wide = gs.read_bvh4()
    if n == 1:
        assert wide.shape[0] == 1 and wide[0, 24] == 0x80000000 and (wide[0, 25:28] == 0xFFFFFFFF).all()
    else:
        ref = _collapse_reference(osc.bvh_nodes(), n, leaf_max=gs.info().leaf_max)
        assert wide.shape == ref.shape
        assert wide.tobytes() == ref.tobytes()
    # every sorted position sits in exactly one leaf
    words = wide[:, 24:28].ravel()
    leaves = words[(words != 0xFFFFFFFF) & (words & 0x80000000 != 0)]
    seen = np.zeros(n, np.int64)
    for w in leaves:
        first, cnt = int(w & 0x0FFFFFFF), int((w >> 28) & 7) + 1
        seen[first:first + cnt] += 1
    assert (seen == 1).all()
    gs.close()


def test_bvh4_cornell(pt, orc, gpu_ctx, cornell_arrays, cornell_oracle):
    sc = pt.Scene(gpu_ctx, *cornell_arrays)
    assert sc.info().bvh4_builder == 1             # default = ePreferFastTrace (main.cpp:419): surface-area BVH4
    sc.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)
    wide = sc.read_bvh4()
    assert wide.tobytes() == _collapse_reference(cornell_oracle.bvh_nodes(), 36, leaf_max=sc.info().leaf_max).tobytes()
    assert sc.info().n_wide_nodes == wide.shape[0] <= 18 and sc.info().bvh4_builder == 0
    sc.close()


def _leaf_cover(wide, n):
    words = wide[:, 24:28].ravel()
    leaves = words[(words != 0xFFFFFFFF) & (words & 0x80000000 != 0)]
    seen = np.zeros(n, np.int64)
    for w in leaves:
        first, cnt = int(w & 0x0FFFFFFF), int((w >> 28) & 7) + 1
        seen[first:first + cnt] += 1
    return seen


@pytest.mark.parametrize("n,seed", [(0, 0), (1, 1), (2, 2), (3, 3), (7, 4), (100, 5), (2048, 6), (2049, 7)])
def test_fast_trace_bvh4_is_a_valid_tree_and_changes_no_hit(pt, orc, gpu_ctx, cornell_arrays, n, seed):
    """pt_scene_set_bvh_quality: the surface-area BVH4 of small scenes (n = 0 here is the Cornell box) covers
    every triangle exactly once, is reachable from node 0, and returns the oracle's hits -- as does the
    collapsed LBVH after switching back.  Above 2048 triangles FAST_TRACE is the cheaper of the LBVH and its PLOC rebuild."""
    v, i, f = cornell_arrays if n == 0 else _soup(n, seed, spread=0.3)
    nt = len(i) // 3
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    assert gs.info().bvh4_builder in ((1,) if nt <= 2048 else (0, 2))
    rng = np.random.default_rng(seed)
    rays = np.concatenate([rng.uniform(-1.2, 1.2, (30000, 3)), rng.normal(size=(30000, 3))], axis=1).astype(np.float32)
    want, _ = osc.trace(rays)
    for quality in (pt.BVH_PREFER_FAST_TRACE, pt.BVH_PREFER_FAST_BUILD, pt.BVH_PREFER_FAST_TRACE):
        gs.set_bvh_quality(quality)
        info = gs.info()
        assert info.bvh4_builder in ((0,) if quality == pt.BVH_PREFER_FAST_BUILD else ((1,) if nt <= 2048 else (0, 2)))
        if nt > 2048 and quality == pt.BVH_PREFER_FAST_TRACE:      # the kept tree is the one with the smaller area sum
            assert (info.bvh4_builder == 2) == (info.tree_area_ploc < 0.9 * info.tree_area_lbvh) and info.tree_area_ploc > 0
        wide = gs.read_bvh4()
        assert wide.shape[0] == info.n_wide_nodes
        assert (_leaf_cover(wide, nt) == 1).all()
        words = wide[:, 24:28]
        kids = words[(words != 0xFFFFFFFF) & (words & 0x80000000 == 0)]
        assert sorted(kids.tolist()) == list(range(1, wide.shape[0]))      # every node but the root has one parent
        fl = wide.view(np.float32)
        used = words != 0xFFFFFFFF
        for ax in range(3):
            assert (fl[:, 4 * ax:4 * ax + 4][used] <= fl[:, 12 + 4 * ax:16 + 4 * ax][used]).all()
            assert np.isinf(fl[:, 4 * ax:4 * ax + 4][~used]).all()
        for extend in (pt.EXTEND_AUTO, pt.EXTEND_HBM):
            assert gs.trace(rays, extend=extend).tobytes() == want.tobytes(), (n, quality, extend)
    with pytest.raises(pt.PtError):
        gs.set_bvh_quality(7)
    gs.close()


def test_fast_trace_bvh4_saves_traversal_work_on_the_cornell_box(pt, gpu_ctx, cornell_arrays):
    sc, film = pt.Scene(gpu_ctx, *cornell_arrays), pt.Film(gpu_ctx, 320, 180)
    work, films = [], []
    for quality in (pt.BVH_PREFER_FAST_BUILD, pt.BVH_PREFER_FAST_TRACE):
        sc.set_bvh_quality(quality)
        film.clear(); gpu_ctx.reset_stats()
        pt.render(sc, film, pt.default_params(width=320, height=180, spp_per_frame=8, max_depth=8, flags=pt.FLAG_COUNT_VISITS))
        st = gpu_ctx.stats()
        work.append((100 * st.nodes_visited + 60 * st.tris_tested) / st.rays)
        films.append(film.read_f32().tobytes())
    assert films[0] == films[1]
    assert work[1] < 0.9 * work[0], work
    sc.close(); film.close()


def test_trace_primary_rays_bit_exact(pt, orc, cornell_gpu, cornell_oracle):
    g = np.load(os.path.join(HERE, "golden", "c1_256_1spp_d4.npz"))
    p = orc.default_params(width=256, height=256)
    rays = np.zeros((256 * 256, 6), np.float32)
    for y in range(256):
        for x in range(256):
            o, d, _ = orc.primary_ray(p, x, y, orc.seed(x, y, 0, 0))
            rays[y * 256 + x] = np.concatenate([o, d])
    ohits, _ = cornell_oracle.trace(rays, mode=0)
    for variant in (pt.EXTEND_AUTO, pt.EXTEND_LDS, pt.EXTEND_HBM):
        hits = cornell_gpu.trace(rays, extend=variant)
        assert hits.tobytes() == ohits.tobytes(), variant
    prim = hits["prim"].astype(np.int64)
    prim[prim == pt.MISS] = 255
    assert (prim.reshape(256, 256) == g["first_prim"]).all()
    assert hits["u"].reshape(256, 256).tobytes() == g["first_u"].tobytes()


def test_trace_random_rays_soup_bit_exact(pt, orc, gpu_ctx):
    v, i, f = _soup(20000, 21, spread=0.05)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    rng = np.random.default_rng(22)
    n = 50000
    org = rng.uniform(-1.3, 1.3, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:30] = 0
    d[np.arange(30), np.arange(30) % 3] = np.where(np.arange(30) % 2, 1, -1)  # axis-aligned
    d[30] = np.nan
    rays = np.concatenate([org, d.astype(np.float32)], 1)
    ohits, _ = osc.trace(rays, mode=1)
    for variant in (pt.EXTEND_AUTO, pt.EXTEND_HBM):
        hits = gs.trace(rays, extend=variant)
        assert hits.tobytes() == ohits.tobytes()
    with pytest.raises(pt.PtError):
        gs.trace(rays, extend=1)                   # (PT_EXTEND_FLAT, the brute-force loop: removed in API version 5)
    assert 0.2 < (hits["prim"] != pt.MISS).mean() < 1.0
    assert gs.trace(rays[:0]).size == 0  # empty batch
    gs.close()


def test_ray_setup_divides_inside_and_outside_the_short_division_guards(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle):
    """ptm::ray_setup takes its three quotients by the exact short division (recip_rn / quot_rn) when the dominant direction
    component lies within 2^+-20 and the others are at least 2^-100 in magnitude, and by the IEEE divide otherwise: rays on
    both sides of every guard -- un-normalised directions from 2^-30 to 2^30 long, components that are zero, -0, denormal,
    2^-110, just inside and just outside the bounds -- must give the oracle's records on every kernel (single-level LDS /
    HBM / flat / 8-wide, and the two-level kernel, whose instance entry divides in object space)."""
    rng = np.random.default_rng(77)
    n = 6000
    org = (rng.uniform(-0.9, 0.9, (n, 3)) + np.array([0, -1, 0])).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    scale = 2.0 ** rng.integers(-30, 31, n)                      # the dominant component on either side of 2^+-20
    scale[: n // 3] = 1.0
    d = (d * scale[:, None]).astype(np.float32)
    tiny = np.float32([0.0, -0.0, 1e-45, -3e-42, 2.0 ** -110, -(2.0 ** -101), 2.0 ** -100, -(2.0 ** -99)])
    k = np.arange(n)
    sel = k % 5 == 0
    d[sel, (k[sel] // 5) % 3] = tiny[(k[sel] // 15) % len(tiny)]   # one small / zero component
    sel2 = k % 35 == 0
    d[sel2, (k[sel2] // 5 + 1) % 3] = tiny[(k[sel2] // 7) % len(tiny)]  # sometimes two
    edge = np.float32([2.0 ** -20, np.nextafter(np.float32(2.0 ** -20), np.float32(0)), 2.0 ** 20, np.nextafter(np.float32(2.0 ** 20), np.float32(np.inf))])
    for j, e in enumerate(edge):                                  # exactly on and one ulp off the divisor's bounds
        d[100 + j] = np.float32([0.3, -0.2, 1.0]) * e
    rays = np.concatenate([org, d], 1).astype(np.float32)
    ohits, _ = cornell_oracle.trace(rays, mode=0, tmax=1e30)
    for variant in (pt.EXTEND_AUTO, pt.EXTEND_LDS, pt.EXTEND_HBM):
        hits = cornell_gpu.trace(rays, extend=variant, tmax=1e30)
        assert hits.tobytes() == ohits.tobytes(), variant
    assert (ohits["prim"] != pt.MISS).mean() > 0.3
    v, i, f = _soup(20000, 23, spread=0.05)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    rays[:, :3] = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    want, _ = osc.trace(rays, mode=1, tmax=1e30)
    for variant in (pt.EXTEND_HBM, pt.EXTEND_HBM8):
        assert gs.trace(rays, extend=variant, tmax=1e30).tobytes() == want.tobytes(), variant
    gs.close()
    v, i, f = pt.load_obj(pt.ASSET_CORNELL)
    inst = _random_instances(7, 3)
    gi, oi = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    gi.set_instances(inst)
    oi.set_instances(inst)
    want, _ = oi.trace(rays, mode=1, tmax=1e30)
    assert gi.trace(rays, tmax=1e30).tobytes() == want.tobytes()
    gi.close()


@pytest.mark.parametrize("pipes", [1, 2, 3])
def test_round_loop_stops_early_on_the_lagged_live_count(pt, orc, gpu_ctx, pipes):
    """The round loop polls the live queue counts every eighth round and reads the count of the PREVIOUS poll (no stream is
    drained inside a batch): a scene nearly every path leaves after its first ray -- one small triangle -- must stop long before
    group_size x max_depth rounds (at most two poll intervals after the queues ran empty), with one, two and three pipelines,
    and render the oracle's bits; the Cornell box, whose paths do run to full depth, must still run every round."""
    v = np.float32([-0.1, -1.1, 0.0, 0.1, -1.1, 0.0, 0.0, -0.9, 0.0])
    i = np.uint32([0, 1, 2])
    f = np.float32([0.5, 0.5, 0.5, 0.0, 0.0, 0.0])
    old = gpu_ctx.set_tuning(pipes=pipes)
    try:
        gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
        W, H = 1280, 1024                                   # 1.3 M pixels x 4 frames: enough slots for three pipelines
        kw = dict(width=W, height=H, spp_per_frame=16, max_depth=16)
        film = pt.Film(gpu_ctx, W, H)
        gpu_ctx.reset_stats()
        pt.render(gs, film, pt.default_params(frame=0, frame_count=4, frames_in_flight=4, sample_groups=1, **kw))
        st = gpu_ctx.stats()
        assert st.pipelines == pipes
        assert st.rounds <= 32 + 16, st.rounds              # a pixel on the triangle: 16 samples x 2 rays in sequence; + two poll intervals; not 256
        ofilm, _, orays = _render_oracle(orc, osc, 4, **kw)
        assert st.rays == orays and film.read_f32().tobytes() == ofilm.tobytes()
        film.close(); gs.close()
    finally:
        gpu_ctx.set_tuning(**old)


def test_c1_render_bit_exact(pt, orc, gpu_ctx, cornell_gpu):
    """BASELINE.json config 1: 256x256, 1 spp, depth 4 -- against the committed golden."""
    g = np.load(os.path.join(HERE, "golden", "c1_256_1spp_d4.npz"))
    film = pt.Film(gpu_ctx, 256, 256)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(width=256, height=256, spp_per_frame=1, max_depth=4))
    st = gpu_ctx.stats()
    assert st.rays == int(g["rays"]) == 154427
    assert st.paths == 65536
    assert film.read_f32().tobytes() == g["image"].tobytes()
    film.close()


@pytest.mark.parametrize("w,h,spp,depth,frames,fif", [
    (64, 64, 8, 8, 3, 0), (64, 64, 8, 8, 3, 1), (64, 64, 8, 8, 3, 2),
    (100, 37, 5, 3, 2, 0),      # ragged: partial 8x8 tiles on both edges
    (8, 8, 32, 8, 1, 0), (1, 1, 4, 8, 1, 0), (257, 9, 1, 1, 1, 0), (128, 128, 32, 8, 2, 0)])
def test_progressive_render_bit_exact(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, any_pipeline, w, h, spp, depth, frames, fif):
    film = pt.Film(gpu_ctx, w, h)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(width=w, height=h, spp_per_frame=spp, max_depth=depth, pipeline=any_pipeline,
                                                   frame=0, frame_count=frames, frames_in_flight=fif))
    ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, frames, width=w, height=h, spp_per_frame=spp,
                                         max_depth=depth)
    st = gpu_ctx.stats()
    assert st.rays == orays
    assert st.paths == w * h * spp * frames
    assert film.read_f32().tobytes() == ofilm.tobytes()
    assert film.read_bgra8().tobytes() == obgra.tobytes()
    film.close()


@pytest.mark.parametrize("groups,fif", [(1, 1), (2, 1), (3, 2), (5, 1), (8, 3), (32, 1), (0, 0)])
def test_sample_groups_keep_the_sum_order_bit_exact(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, groups, fif):
    """Samples of a pixel traced concurrently by several slots (term logs replayed in order) must
    reproduce the reference's single sequential accumulator bit for bit."""
    kw = dict(width=88, height=40, spp_per_frame=32, max_depth=8)
    film = pt.Film(gpu_ctx, 88, 40)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=3, sample_groups=groups, frames_in_flight=fif, **kw))
    ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, 3, **kw)
    st = gpu_ctx.stats()
    assert st.rays == orays and st.paths == 88 * 40 * 32 * 3
    assert film.read_f32().tobytes() == ofilm.tobytes()
    assert film.read_bgra8().tobytes() == obgra.tobytes()
    film.close()


@pytest.mark.parametrize("variant", [2, 3, 4])
def test_every_extend_variant_renders_the_same_bits(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, variant):
    kw = dict(width=72, height=56, spp_per_frame=6, max_depth=8)
    film = pt.Film(gpu_ctx, 72, 56)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=2, extend=variant, **kw))
    st = gpu_ctx.stats()
    assert st.extend_variant == variant
    ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, 2, **kw)
    assert st.rays == orays
    assert film.read_f32().tobytes() == ofilm.tobytes()
    assert film.read_bgra8().tobytes() == obgra.tobytes()
    film.close()


def test_frame_by_frame_equals_batched(pt, gpu_ctx, cornell_gpu, any_pipeline):
    """The reference dispatches one frame per loop iteration (main.cpp:647-685); batching frames
    on the device must not change a bit."""
    a, b = pt.Film(gpu_ctx, 96, 80), pt.Film(gpu_ctx, 96, 80)
    kw = dict(width=96, height=80, spp_per_frame=4, max_depth=8, pipeline=any_pipeline)
    for k in range(5):
        pt.render(cornell_gpu, a, pt.default_params(frame=k, frame_count=1, **kw))
    pt.render(cornell_gpu, b, pt.default_params(frame=0, frame_count=5, frames_in_flight=3, **kw))
    assert a.read_f32().tobytes() == b.read_f32().tobytes()
    assert a.read_bgra8().tobytes() == b.read_bgra8().tobytes()
    a.close(); b.close()


def test_pixel_tile_sharding_sums_to_single_device(pt, gpu_ctx, cornell_gpu, any_pipeline):
    """Multi-GPU decomposition on one GPU: the world films are disjoint and add up bit-exactly."""
    import importlib
    d = importlib.import_module("single-file-vulkan-pathtracing_amd.distributed")
    w, h = 200, 120
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=8, frame=0, frame_count=2, pipeline=any_pipeline)
    full = pt.Film(gpu_ctx, w, h)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, full, pt.default_params(**kw))
    rays_full = gpu_ctx.stats().rays
    ref = full.read_f32()
    for world in (2, 3, 8):
        acc = np.zeros_like(ref)
        rays = 0
        for rank in range(world):
            film = pt.Film(gpu_ctx, w, h)
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.default_params(rank=rank, world=world, **kw))
            rays += gpu_ctx.stats().rays
            part = film.read_f32()
            mask = d.owned_mask(w, h, rank, world)
            assert (part[~mask] == 0).all()
            acc += part
            film.close()
        assert acc.tobytes() == ref.tobytes()
        assert rays == rays_full
    full.close()


def test_soup_render_bit_exact_global_memory_variant(pt, orc, gpu_ctx):
    """A scene too big for LDS goes through the L2/HBM extend variant; same bits expected."""
    v, i, f = _soup(30000, 31, spread=0.04)
    v = v.reshape(-1, 3) * np.float32([0.9, 0.9, 0.9]) + np.float32([0, -1, 0])  # into the camera's view
    gs, osc = pt.Scene(gpu_ctx, v.reshape(-1), i, f), orc.Scene(v.reshape(-1), i, f)
    film = pt.Film(gpu_ctx, 96, 96)
    gpu_ctx.reset_stats()
    pt.render(gs, film, pt.default_params(width=96, height=96, spp_per_frame=4, max_depth=6, frame_count=2))
    st = gpu_ctx.stats()
    assert st.extend_variant == pt.EXTEND_HBM8      # (AUTO beyond ~11 000 triangles since round 3; the BVH4 kernel: tests below)
    ofilm, obgra, orays = _render_oracle(orc, osc, 2, width=96, height=96, spp_per_frame=4, max_depth=6)
    assert st.rays == orays
    assert film.read_f32().tobytes() == ofilm.tobytes()
    film.close(); gs.close()


def test_c2_size_properties(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle):
    """BASELINE.json config 2 geometry (1920x1080, depth 8) at full size: bit-exact against the
    oracle at 2 spp (seconds of CPU), then size-independent properties of a full 32-spp frame."""
    w, h = 1920, 1080
    film = pt.Film(gpu_ctx, w, h)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(width=w, height=h, spp_per_frame=2, max_depth=8))
    ofilm, _, orays = _render_oracle(orc, cornell_oracle, 1, width=w, height=h, spp_per_frame=2, max_depth=8)
    assert gpu_ctx.stats().rays == orays
    assert film.read_f32().tobytes() == ofilm.tobytes()
    # full frame: determinism, path/ray bookkeeping, energy sanity
    imgs = []
    for _ in range(2):
        film.clear()
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.default_params(width=w, height=h, spp_per_frame=32, max_depth=8))
        st = gpu_ctx.stats()
        imgs.append(film.read_f32())
    assert imgs[0].tobytes() == imgs[1].tobytes()
    assert st.paths == w * h * 32
    assert 3.30 < st.rays / st.paths < 3.45            # SURVEY: 3.38 rays/path at depth 8
    assert np.isfinite(imgs[0]).all() and imgs[0].min() >= 0
    np.testing.assert_allclose(imgs[0].reshape(-1, 3).mean(0), [0.529, 0.416, 0.292], rtol=0.02)
    # primary misses see exactly the environment colour (miss.rmiss:10): top-left border pixel
    # (32 float adds of weight*env, then /32: raygen.rgen:76, 86)
    want = []
    for e in (0.7, 0.6, 0.5):
        c = np.float32(0)
        for _ in range(32):
            c = np.float32(c + np.float32(1.0) * np.float32(e))
        want.append(np.float32(c / np.float32(32)))
    assert list(imgs[0][4, 4]) == want
    film.close()


def _random_instances(n, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((n, 3, 4), np.float32)
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        m[k, :, :3] = (q * rng.uniform(0.2, 0.6)).astype(np.float32)
        m[k, :, 3] = rng.uniform(-1.5, 1.5, 3).astype(np.float32) + np.float32([0, -1, 0])
    return m


@pytest.mark.parametrize("n_inst,seed", [(1, 1), (2, 2), (5, 3), (60, 4), (1500, 5)])
def test_instanced_trace_and_render_bit_exact(pt, orc, gpu_ctx, cornell_arrays, n_inst, seed):
    """Two-level scenes (config C4's mechanism) with rotated + scaled instances."""
    inst = _random_instances(n_inst, seed)
    gs, osc = pt.Scene(gpu_ctx, *cornell_arrays), orc.Scene(*cornell_arrays)
    gs.set_instances(inst)
    osc.set_instances(inst)
    info = gs.info()
    assert info.n_instances == n_inst and info.n_tlas_nodes >= 1
    rng = np.random.default_rng(seed + 100)
    n = 20000
    org = rng.uniform(-3, 3, (n, 3)).astype(np.float32) + np.float32([0, -1, 0])
    tgt = inst[rng.integers(0, n_inst, n), :, 3] + rng.uniform(-0.4, 0.4, (n, 3)).astype(np.float32)
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([org, d.astype(np.float32)], 1)
    hits = gs.trace(rays)
    ohits, _ = osc.trace(rays, mode=1)
    assert hits.tobytes() == ohits.tobytes()
    assert (hits["prim"] != pt.MISS).mean() > 0.2
    kw = dict(width=80, height=64, spp_per_frame=3, max_depth=6)
    film = pt.Film(gpu_ctx, 80, 64)
    gpu_ctx.reset_stats()
    pt.render(gs, film, pt.default_params(frame=0, frame_count=2, **kw))
    ofilm, obgra, orays = _render_oracle(orc, osc, 2, **kw)
    assert gpu_ctx.stats().rays == orays
    assert film.read_f32().tobytes() == ofilm.tobytes()
    assert film.read_bgra8().tobytes() == obgra.tobytes()
    # dropping the instances restores the reference's single-instance scene
    gs.set_instances(np.zeros((0, 3, 4), np.float32))
    film.clear()
    pt.render(gs, film, pt.default_params(frame=0, frame_count=1, **kw))
    single = orc.Scene(*cornell_arrays)
    sfilm, _, _ = _render_oracle(orc, single, 1, **kw)
    assert film.read_f32().tobytes() == sfilm.tobytes()
    film.close(); gs.close()


def test_c4_grid_of_10000_instances(pt, orc, gpu_ctx, cornell_arrays):
    """BASELINE.json config 4: Cornell BLAS x 10 000 instances (100 x 100 grid), two-level BVH."""
    inst = pt.cornell_grid_instances()
    assert inst.shape == (10000, 3, 4)
    gs, osc = pt.Scene(gpu_ctx, *cornell_arrays), orc.Scene(*cornell_arrays)
    gs.set_instances(inst)
    osc.set_instances(inst)
    kw = dict(width=320, height=180, spp_per_frame=2, max_depth=8)
    film = pt.Film(gpu_ctx, 320, 180)
    gpu_ctx.reset_stats()
    pt.render(gs, film, pt.default_params(frame=0, frame_count=1, **kw))
    ofilm, _, orays = _render_oracle(orc, osc, 1, **kw)
    assert gpu_ctx.stats().rays == orays
    img = film.read_f32()
    assert img.tobytes() == ofilm.tobytes()
    # first hits at full resolution geometry: every primary ray inside the grid hits some instance
    p = orc.default_params(width=1920, height=1080)
    rays = np.array([np.concatenate(orc.primary_ray(p, x, y, orc.seed(x, y, 0, 0))[:2])
                     for y in range(300, 800, 23) for x in range(500, 1400, 29)], np.float32)
    h = gs.trace(rays)
    oh, _ = osc.trace(rays, mode=1)
    assert h.tobytes() == oh.tobytes()
    hit = h["prim"] != pt.MISS          # rays can slip through the 2 mm gaps between the mini boxes
    assert hit.mean() > 0.8 and len(np.unique(h["inst"][hit])) > 100
    film.close(); gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [dict(node_yield=0), dict(node_yield=2), dict(tlas_lds_kb=0),
                                   dict(tlas_lds_kb=24, node_yield=8), dict(inst16=0), dict(leaf_min=1), dict(leaf_min=24, enter_min=4),
                                   dict(leaf_min=64, enter_min=64), dict(inst_frames=0)])
def test_two_level_kernel_scheduling_knobs_keep_the_bits(pt, orc, gpu_ctx, cornell_arrays, knobs):
    """The scheduling of the compact two-level kernel (when the node loop yields to waiting leaves, how many TLAS nodes are
    staged in LDS, how many lanes wait before a leaf step or an instance entry runs; inst16 = 0: the general two-level kernel; inst_frames = 0: k_shade
    transforms the normal per hit instead of reading the per-(instance, triangle) table) must not show in the results: the 10 000-instance grid -- a partly LDS-resident
    TLAS -- and a 7-instance set -- an entirely LDS-resident one -- render and trace to the oracle's bits under every setting."""
    old = gpu_ctx.set_tuning(**knobs)      # include/pt_api.h pt_tuning (the library reads no tuning from the environment)
    try:
        for inst in (pt.cornell_grid_instances(), _random_instances(7, 3)):
            gs, osc = pt.Scene(gpu_ctx, *cornell_arrays), orc.Scene(*cornell_arrays)
            gs.set_instances(inst)
            osc.set_instances(inst)
            kw = dict(width=192, height=108, spp_per_frame=2, max_depth=8)
            film = pt.Film(gpu_ctx, 192, 108)
            gpu_ctx.reset_stats()
            pt.render(gs, film, pt.default_params(frame=0, frame_count=1, **kw))
            ofilm, _, orays = _render_oracle(orc, osc, 1, **kw)
            assert gpu_ctx.stats().rays == orays, knobs
            assert film.read_f32().tobytes() == ofilm.tobytes(), knobs
            film.close(); gs.close()
    finally:
        gpu_ctx.set_tuning(**old)


def test_pt_main_host_driver_writes_the_same_image(pt, gpu_ctx, cornell_gpu, tmp_path):
    """The C++20 host driver (reference main() without Vulkan/GLFW) against the Python path."""
    import json
    import subprocess
    exe = os.path.join(os.path.dirname(pt.__file__), "pt_main")
    if not os.path.exists(exe):
        pt.build()
    pfm, ppm = str(tmp_path / "o.pfm"), str(tmp_path / "o.ppm")
    out = subprocess.run([exe, "--obj", pt.ASSET_CORNELL, "--width", "96", "--height", "64", "--frames", "3", "--spp", "4",
                          "--depth", "8", "--pfm", pfm, "--ppm", ppm], check=True, capture_output=True, text=True, cwd=pt.REPO)
    info = json.loads(out.stdout.strip().splitlines()[-1])
    film = pt.Film(gpu_ctx, 96, 64)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(width=96, height=64, spp_per_frame=4, max_depth=8, frame_count=3))
    assert info["rays"] == gpu_ctx.stats().rays and info["triangles"] == 36 and info["paths"] == 96 * 64 * 4 * 3
    raw = open(pfm, "rb").read()
    head = b"PF\n96 64\n-1.0\n"
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], np.float32).reshape(64, 96, 3)[::-1]
    assert img.tobytes() == film.read_f32().tobytes()
    praw = open(ppm, "rb").read()
    rgb = np.frombuffer(praw[len(b"P6\n96 64\n255\n"):], np.uint8).reshape(64, 96, 3)
    assert (rgb == film.read_bgra8()[..., [2, 1, 0]]).all()
    film.close()


def test_prepare_then_render_and_degenerate_shapes(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle):
    film = pt.Film(gpu_ctx, 40, 24)
    p = pt.default_params(width=40, height=24, spp_per_frame=7, max_depth=1, frame_count=5)
    pt.render_prepare(cornell_gpu, film, p)
    st = gpu_ctx.stats()
    assert st.frames_in_flight >= 1 and st.sample_groups >= 1
    for spp, depth in ((1, 1), (1, 8), (7, 1), (33, 2)):
        film.clear()
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.default_params(width=40, height=24, spp_per_frame=spp, max_depth=depth, frame_count=2))
        ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, 2, width=40, height=24, spp_per_frame=spp, max_depth=depth)
        assert gpu_ctx.stats().rays == orays
        assert film.read_f32().tobytes() == ofilm.tobytes()
    # a later frame index and a moved camera
    film.clear()
    kw = dict(width=40, height=24, spp_per_frame=3, max_depth=4, cam_origin=(0.3, -1.2, 4.0), cam_target=(0.1, -0.9, 1.5),
              env=(0.2, 0.3, 0.9), tmin=0.01, tmax=50.0)
    pt.render(cornell_gpu, film, pt.default_params(frame=7, frame_count=1, **kw))
    img, _, _, _ = cornell_oracle.render_frame(orc.default_params(frame=7, **kw))
    o = np.zeros_like(img)
    orc.accumulate_f32(o, img, 7)
    assert film.read_f32().tobytes() == o.tobytes()
    film.close()


def test_4k_film_bit_exact(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, any_pipeline):
    """3840x2160 (8.3 M pixels, partial last tile row): 1 spp, depth 4 -- ~20 M rays on the oracle."""
    kw = dict(width=3840, height=2160, spp_per_frame=1, max_depth=4)
    film = pt.Film(gpu_ctx, 3840, 2160)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(pipeline=any_pipeline, **kw))
    img, rays, _, _ = cornell_oracle.render_frame(orc.default_params(**kw))
    st = gpu_ctx.stats()
    assert st.paths == 3840 * 2160 and st.rays == rays
    assert film.read_f32().tobytes() == img.tobytes()
    film.close()


def test_c5_full_size_soup_structure_and_hits(pt, orc, gpu_ctx, tmp_path):
    """BASELINE.json config 5 at full size: the 1 000 000-triangle soup through the OBJ loader, the
    on-device LBVH/BVH4 build and the HBM traversal variant; hit records bit-exact vs the oracle."""
    path = str(tmp_path / "soup1m.obj")
    pt.write_soup_obj(path, 1000000, 1)
    v, i, f = pt.load_obj(path)
    os.remove(path)
    assert i.size == 3000000
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    info = gs.info()
    assert info.n_tris == 1000000 and info.bvh_height == osc.bvh_info().height
    keys, prim, _ = gs.read_bvh()
    okeys, oprim = osc.bvh_keys()
    assert (np.diff(keys.astype(np.int64)) >= 0).all()                 # sorted
    assert (keys == okeys).all() and (prim == oprim).all()             # same order as the CPU builder
    assert (np.sort(prim) == np.arange(1000000)).all()                 # a permutation
    wide = gs.read_bvh4()
    words = wide[:, 24:28].ravel()
    leaves = words[(words != 0xFFFFFFFF) & (words & 0x80000000 != 0)]
    first, cnt = (leaves & 0x0FFFFFFF).astype(np.int64), ((leaves >> 28) & 7).astype(np.int64) + 1
    cover = np.zeros(1000001, np.int64)
    np.add.at(cover, first, 1)
    np.add.at(cover, first + cnt, -1)
    assert (np.cumsum(cover)[:-1] == 1).all()                          # every triangle in exactly one leaf
    p = orc.default_params(width=1920, height=1080)
    rng = np.random.default_rng(9)
    rays = [np.concatenate(orc.primary_ray(p, int(x), int(y), orc.seed(int(x), int(y), 0, 0))[:2])
            for x, y in zip(rng.integers(300, 1620, 4000), rng.integers(150, 930, 4000))]
    org = rng.uniform(-1, 1, (16000, 3)).astype(np.float32) + np.float32([0, -1, 0])
    d = rng.normal(size=(16000, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.array(rays, np.float32), np.concatenate([org, d.astype(np.float32)], 1)])
    hits = gs.trace(rays, tmax=10000.0)
    ohits, _ = osc.trace(rays, mode=1)
    assert hits.tobytes() == ohits.tobytes()
    assert (hits["prim"] != pt.MISS).mean() > 0.7
    # one small frame through the whole pipeline at full scene size
    film = pt.Film(gpu_ctx, 128, 72)
    gpu_ctx.reset_stats()
    kw = dict(width=128, height=72, spp_per_frame=2, max_depth=16)
    pt.render(gs, film, pt.default_params(**kw))
    ofilm, _, orays = _render_oracle(orc, osc, 1, **kw)
    # 128 MB of nodes + records: beyond L2, so AUTO walks the 8-wide tree (extend_launch.hip ptw_plan_extend)
    assert gpu_ctx.stats().rays == orays and gpu_ctx.stats().extend_variant == pt.EXTEND_HBM8
    assert film.read_f32().tobytes() == ofilm.tobytes()
    gpu_ctx.reset_stats()
    film2 = pt.Film(gpu_ctx, 128, 72)
    pt.render(gs, film2, pt.default_params(extend=pt.EXTEND_HBM, **kw))  # and the BVH4 kernel on the same scene
    assert gpu_ctx.stats().rays == orays and gpu_ctx.stats().extend_variant == pt.EXTEND_HBM
    assert film2.read_f32().tobytes() == ofilm.tobytes()
    film.close(); film2.close(); gs.close()


def test_c2_full_size_32spp_crop_matches_golden(pt, orc, gpu_ctx, cornell_gpu):
    """BASELINE config 2 exactly (1920x1080, 64 spp = 2 frames x 32, depth 8) on the GPU; the committed
    oracle crop of that launch must come out bit for bit, frame by frame and after the blend."""
    g = np.load(os.path.join(HERE, "golden", "c2_crop_1080p_32spp_d8.npz"))
    x0, y0, rw, rh = [int(v) for v in g["rect"]]
    kw = dict(width=1920, height=1080, spp_per_frame=32, max_depth=8)
    film = pt.Film(gpu_ctx, 1920, 1080)
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=1, **kw))
    assert np.ascontiguousarray(film.read_f32()[y0:y0 + rh, x0:x0 + rw]).tobytes() == g["frame0"].tobytes()
    pt.render(cornell_gpu, film, pt.default_params(frame=1, frame_count=1, **kw))
    want = g["frame0"].copy()
    orc.accumulate_f32(want, np.ascontiguousarray(g["frame1"]), 1)
    assert np.ascontiguousarray(film.read_f32()[y0:y0 + rh, x0:x0 + rw]).tobytes() == want.tobytes()
    # both frames in one call (batched, sample groups chosen automatically)
    film.clear()
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=2, **kw))
    assert np.ascontiguousarray(film.read_f32()[y0:y0 + rh, x0:x0 + rw]).tobytes() == want.tobytes()
    st = gpu_ctx.stats()
    assert st.paths == 1920 * 1080 * 64 and 3.36 < st.rays / st.paths < 3.40
    film.close()


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_tiny_scenes_end_to_end(pt, orc, gpu_ctx, n):
    """Degenerate trees (a root that is one leaf, a root with 2 leaves, ...) through trace and render,
    every extend variant."""
    rng = np.random.default_rng(n)
    v = np.zeros((n, 3, 3), np.float32)
    for k in range(n):
        c = np.float32([rng.uniform(-0.6, 0.6), rng.uniform(-1.6, -0.4), rng.uniform(-0.5, 0.5)])
        v[k] = c + rng.uniform(-0.5, 0.5, (3, 3)).astype(np.float32)
    f = np.tile(np.float32([0.7, 0.6, 0.5, 0.0, 0.0, 0.0]), (n, 1))
    f[0, 3:] = (5.0, 4.0, 3.0)
    i = np.arange(3 * n, dtype=np.uint32)
    gs, osc = pt.Scene(gpu_ctx, v.reshape(-1), i, f.reshape(-1)), orc.Scene(v.reshape(-1), i, f.reshape(-1))
    p = orc.default_params(width=64, height=64)
    rays = np.array([np.concatenate(orc.primary_ray(p, x, y, orc.seed(x, y, 0, 0))[:2])
                     for y in range(0, 64, 2) for x in range(0, 64, 2)], np.float32)
    oh, _ = osc.trace(rays, mode=0)
    for variant in (pt.EXTEND_AUTO, pt.EXTEND_LDS, pt.EXTEND_HBM):
        assert gs.trace(rays, extend=variant).tobytes() == oh.tobytes()
    assert (oh["prim"] != orc.MISS).any()
    kw = dict(width=48, height=48, spp_per_frame=5, max_depth=6)
    film = pt.Film(gpu_ctx, 48, 48)
    gpu_ctx.reset_stats()
    pt.render(gs, film, pt.default_params(frame_count=2, **kw))
    ofilm, obgra, orays = _render_oracle(orc, osc, 2, **kw)
    assert gpu_ctx.stats().rays == orays
    assert film.read_f32().tobytes() == ofilm.tobytes()
    film.close(); gs.close()


def test_no_device_memory_leak_over_object_lifecycles(pt, cornell_arrays):
    """Contexts, scenes (incl. instances), films and their workspaces give all device memory back."""
    import torch
    torch.cuda.synchronize()
    inst = pt.cornell_grid_instances(n=10)

    def cycle():
        ctx = pt.Context(0)
        sc = pt.Scene(ctx, *cornell_arrays)
        film = pt.Film(ctx, 320, 200)
        pt.render(sc, film, pt.default_params(width=320, height=200, spp_per_frame=4, max_depth=4, frame_count=3))
        sc.set_instances(inst)
        pt.render(sc, film, pt.default_params(width=320, height=200, spp_per_frame=4, max_depth=4, frame_count=1,
                                              sample_groups=2, flags=pt.FLAG_PROFILE | pt.FLAG_COUNT_VISITS))
        sc.trace(np.zeros((10, 6), np.float32) + np.float32([0, -1, 5, 0, 0, -1]))
        film.close(); sc.close(); ctx.close()

    cycle()                                   # first cycle pays one-time runtime allocations
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(10):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), f"leaked {(free0 - free1) / 2**20:.1f} MiB over 10 cycles"


def test_repeated_renders_are_bit_identical(pt, gpu_ctx, cornell_gpu):
    """Race detector for the scheduling machinery (two pipelines on two streams, lane refill, compaction
    atomics, ordered term logs): the same work must give the same bits and the same ray count every time,
    whatever order the hardware happened to run the waves in."""
    import hashlib
    film = pt.Film(gpu_ctx, 640, 360)
    for extend in (pt.EXTEND_LDS, pt.EXTEND_HBM):
        for kw in (dict(frame_count=6), dict(frame_count=6, sample_groups=4, frames_in_flight=2),
                   dict(frame_count=3, rank=1, world=3)):
            seen = set()
            for _ in range(6):
                film.clear(); gpu_ctx.reset_stats()
                pt.render(cornell_gpu, film, pt.default_params(width=640, height=360, spp_per_frame=16, max_depth=8,
                                                               extend=extend, **kw))
                seen.add((hashlib.sha256(film.read_f32().tobytes()).hexdigest(), gpu_ctx.stats().rays))
            assert len(seen) == 1, (extend, kw, seen)
    film.close()


def test_async_render_equals_blocking(pt, gpu_ctx, cornell_gpu):
    """PT_FLAG_ASYNC: frames are queued without the reference's per-frame waitIdle (main.cpp:683)."""
    kw = dict(width=160, height=96, spp_per_frame=8, max_depth=8)
    a, b = pt.Film(gpu_ctx, 160, 96), pt.Film(gpu_ctx, 160, 96)
    for k in range(4):
        pt.render(cornell_gpu, a, pt.default_params(frame=k, frame_count=1, flags=pt.FLAG_ASYNC, **kw))
    gpu_ctx.sync()
    pt.render(cornell_gpu, b, pt.default_params(frame=0, frame_count=4, **kw))
    assert a.read_f32().tobytes() == b.read_f32().tobytes()
    assert a.read_bgra8().tobytes() == b.read_bgra8().tobytes()
    with pytest.raises(pt.PtError):
        pt.render(cornell_gpu, a, pt.default_params(flags=pt.FLAG_ASYNC | pt.FLAG_PROFILE, **kw))
    a.close(); b.close()


def test_error_paths(pt, gpu_ctx, cornell_gpu):
    film = pt.Film(gpu_ctx, 32, 32)
    with pytest.raises(pt.PtError):
        pt.render(cornell_gpu, film, pt.default_params(width=64, height=32))      # size mismatch
    with pytest.raises(pt.PtError):
        pt.render(cornell_gpu, film, pt.default_params(width=32, height=32, rank=2, world=2))
    with pytest.raises(pt.PtError):
        pt.render(cornell_gpu, film, pt.default_params(width=32, height=32, spp_per_frame=0))
    with pytest.raises(pt.PtError):
        pt.Scene(gpu_ctx, np.zeros(9, np.float32), np.array([0, 1, 7], np.uint32), np.zeros(6, np.float32))
    with pytest.raises(pt.PtError):
        pt.Film(gpu_ctx, 0, 10)
    with pytest.raises(pt.PtError):
        cornell_gpu.set_instances(np.zeros((1, 3, 4), np.float32))       # singular matrix
    assert cornell_gpu.info().n_instances == 0
    film.close()


def _stack_need(wide, node=0):
    ch = [int(x) for x in wide[node, 24:28] if x != 0xFFFFFFFF]
    return max(len(ch) - 1, 0) + max([_stack_need(wide, c) for c in ch if not c & 0x80000000], default=0)


def _octave_chain(levels, per_level, seed):
    """Triangles clustered at 2^-k along the diagonal: the LBVH degenerates into a deep chain."""
    rng = np.random.default_rng(seed)
    v = []
    for k in range(levels):
        s = np.float32(2.0 ** -k)
        c = np.float32(0.9) * s * np.ones(3, np.float32)
        v.append(c + rng.uniform(-0.2, 0.2, (per_level, 3, 3)).astype(np.float32) * s)
    v = np.concatenate(v).astype(np.float32)
    n = v.shape[0]
    faces = rng.uniform(0.2, 1, (n, 6)).astype(np.float32)
    faces[:, 3:] *= (rng.uniform(0, 1, (n, 1)) < 0.2)
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), faces.reshape(-1).astype(np.float32)


@pytest.mark.parametrize("kind", ["soup40", "soup150", "soup450", "chain"])
def test_small_scenes_every_stack_regime_bit_exact(pt, orc, gpu_ctx, kind):
    """LDS-resident scenes pick their traversal-stack regime from the exact stack bound of their BVH4
    (no-spill kernel when it fits 16 LDS entries, LDS + HBM spill otherwise); the HBM variant always
    spills past 12.  All of them must return the oracle's hits and film."""
    v, i, f = _octave_chain(19, 6, 5) if kind == "chain" else _soup(int(kind[4:]), len(kind), spread=0.3)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    gs.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)         # the LBVH of the chain is the deep one
    need = _stack_need(_collapse_reference(osc.bvh_nodes(), osc.n_tris, leaf_max=2))
    assert (need > 16) == (kind == "chain"), need      # the chain is what exercises LDS + spill
    rng = np.random.default_rng(7)
    rays = np.concatenate([rng.uniform(-1.5, 1.5, (20000, 3)), rng.normal(size=(20000, 3))], axis=1).astype(np.float32)
    rays[:5000, :3] = rng.uniform(0, 1, (5000, 1)).astype(np.float32) ** 4 + rng.normal(size=(5000, 3)).astype(np.float32) * 0.01
    want, _ = osc.trace(rays)
    assert (want["prim"] != 0xFFFFFFFF).mean() > 0.02
    kw = dict(width=96, height=64, spp_per_frame=4, max_depth=12, cam_origin=(0.5, 0.5, 4.0), cam_target=(0.0, 0.0, 1.0))
    ofilm, _, orays = _render_oracle(orc, osc, 1, **kw)
    for extend in (pt.EXTEND_LDS, pt.EXTEND_HBM):
        got = gs.trace(rays, extend=extend)
        assert got.tobytes() == want.tobytes(), (kind, extend)
        film = pt.Film(gpu_ctx, 96, 64)
        gpu_ctx.reset_stats()
        pt.render(gs, film, pt.default_params(extend=extend, **kw))
        assert film.read_f32().tobytes() == ofilm.tobytes(), (kind, extend)
        assert gpu_ctx.stats().rays == orays
        film.close()
    gs.close()


def test_bench_multi_rank_flow_on_one_gpu(tmp_path):
    """bench.py's N > 1 path (per-rank tile shards, counters, one film reduce) with every rank on GPU 0 and gloo
    on host copies (PT_BENCH_EMULATE=1): same exact ray count as N = 1 and a well-formed JSON line."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(HERE)
    args = ["--steps", "2", "--warmup", "1", "--width", "320", "--height", "184", "--full", "--no-cpu-baseline", "--no-extra-legs", "--full-line"]
    one = subprocess.run([sys.executable, os.path.join(repo, "bench.py")] + args, capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    j1 = json.loads(one.stdout.strip().splitlines()[-1])
    env = dict(os.environ, PT_BENCH_EMULATE="1")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", "29533", os.path.join(repo, "bench.py"),
                          "--gpus", "2"] + args, capture_output=True, text=True, timeout=600, env=env)
    assert two.returncode == 0, two.stderr[-2000:]
    j2 = json.loads([l for l in two.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert j2["n_gpus"] == 2 and j2["scaling"] == "strong" and j2["steps"] == 2
    assert j2["rays"] == j1["rays"] and j2["paths"] == j1["paths"]
    assert j2["rccl_ranks"] == 2                                   # (gloo ranks in the emulation)
    assert abs(j2["presented_checksum"] - j1["presented_checksum"]) <= 1e-9 * abs(j1["presented_checksum"])   # same image assembled
    lo, hi = j2["rays_per_rank_min_max"]
    assert lo + hi == j2["rays"] and hi - lo < 0.02 * hi          # interleaved tiles balance the ranks
    for k in ("metric", "value", "unit", "ms_per_step", "roofline", "config"):
        assert k in j2


def _bench(args, env=None, timeout=600):
    import json
    import subprocess
    import sys
    repo = os.path.dirname(HERE)
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py")] + args, capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


def test_bench_gpus2_without_a_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 2` with WORLD_SIZE unset -- the form the driver's N = 1 command has -- must
    start its own two ranks instead of exiting.  On one GPU under PT_BENCH_EMULATE (gloo carries the packed tiles between
    the same kernels): the same rays and the same presented image as N = 1, and the multi-rank fields of the line."""
    args = ["--steps", "2", "--warmup", "1", "--reps", "2", "--width", "320", "--height", "184", "--no-cpu-baseline", "--no-extra-legs", "--full-line"]
    one, j1 = _bench(args)
    assert one.returncode == 0, one.stderr[-2000:]
    env = {"PT_BENCH_EMULATE": "1"}
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        assert k not in os.environ, "this test must run without a launcher's environment"
    two, j2 = _bench(["--gpus", "2", "--selftest"] + args, env=env)
    assert two.returncode == 0, two.stderr[-2000:]
    assert j2["n_gpus"] == 2 and j2["steps"] == 2 and j2["reps"] >= 2
    # --selftest: a rank-coloured film went through the run's own collective before the timing and every tile carried its owner's colour
    st = j2["selftest"]
    assert st["ok"] and st["wrong_pixels"] == 0 and st["ranks_seen"] == [0, 1] and st["rccl_ranks"] == 2 and sum(st["tiles_per_rank"]) == 40 * 23
    assert j2["launcher"].startswith("bench.py's own")
    assert j2["rays"] == j1["rays"] and j2["paths"] == j1["paths"]
    assert abs(j2["presented_checksum"] - j1["presented_checksum"]) <= 1e-9 * abs(j1["presented_checksum"])
    lo, hi = j2["rays_per_rank_min_max"]
    assert lo + hi == j2["rays"] and hi - lo < 0.02 * hi
    assert j2["rccl_ranks"] == 2 and j2["present_ms"] > 0.0
    assert j2["value_min"] <= j2["value"] <= j2["value_max"] and len(j2["values"]) == j2["reps"]
    assert j2["workspace_bytes"] > 0


def test_bench_gpus2_without_a_second_gpu_fails_cleanly():
    """The real (RCCL) N = 2 path on a box with one GPU: rank 1 has no device, says so, and bench.py's own launcher stops
    rank 0 too -- a non-zero status within seconds, never a hang inside a collective.  (With two GPUs it simply runs.)"""
    import time
    t0 = time.time()
    r, j = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--reps", "1", "--width", "256", "--height", "128",
                   "--no-cpu-baseline", "--no-extra-legs", "--full-line"], timeout=300)
    if _two_gpus():
        assert r.returncode == 0 and j["n_gpus"] == 2 and j["rccl_ranks"] == 2, r.stderr[-2000:]
    else:
        assert r.returncode != 0 and j is None
        assert "needs GPU 1" in r.stderr and "stopping the other ranks" in r.stderr
        assert time.time() - t0 < 120


def test_bench_config_c3_shape():
    """--config c3 = the Cornell box with 32 steps (1024 spp) unless --steps says otherwise; a small film keeps it short."""
    r, j = _bench(["--config", "c3", "--width", "160", "--height", "96", "--reps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-extra-legs", "--full-line"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert j["steps"] == 32 and "1024 spp" in j["metric"] and j["config"]["workload"].startswith("C3:")
    assert j["paths"] == 160 * 96 * 32 * 32


def test_bench_plain_run_times_k_steps_once_and_dumps_what_a_caller_gets(pt, gpu_ctx, cornell_gpu, tmp_path):
    """A plain run (no --full) times the K steps once and adds no other leg; --dump-outputs writes the film, the rgba8 display image and the ray
    count its last step left -- the same bytes a caller of pt_params_default gets for frames 0 .. K-1 -- and two runs write the same outputs."""
    W, H, K = 320, 184, 3
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r, j = _bench(["--steps", str(K), "--warmup", "1", "--width", str(W), "--height", str(H), "--full-line", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-2000:]
        assert j["steps"] == K and j["reps"] == 1 and len(j["values"]) == 1 and j["ms_per_step"] > 0
        for k in ("roofline", "cpu_baseline", "c2_exact", "latency_1frame", "reference_dispatch", "roofline_c4", "roofline_c5", "roofline_c5x", "wavefront"):
            assert k not in j, k
        assert sorted(os.listdir(d)) == ["display_bgra8.npy", "film.npy", "rays.npy"]
        out = {n: np.load(d / (n + ".npy")) for n in ("film", "display_bgra8", "rays")}
        assert out["film"].dtype == np.float32 and out["film"].shape == (H, W, 3)
        assert out["display_bgra8"].dtype == np.float32 and out["display_bgra8"].shape == (H, W, 4)
        assert out["rays"].dtype == np.float64 and int(out["rays"][0]) == j["rays"]
        assert abs(out["film"].astype(np.float64).sum() - j["presented_checksum"]) <= 1e-9 * abs(j["presented_checksum"])
        dumps.append(out)
    for n in ("film", "display_bgra8", "rays"):
        assert dumps[0][n].tobytes() == dumps[1][n].tobytes(), n
    film = pt.Film(gpu_ctx, W, H)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.library_default_params(frame=0, frame_count=K, width=W, height=H))
    assert gpu_ctx.stats().rays == int(dumps[0]["rays"][0])
    assert film.read_f32().tobytes() == dumps[0]["film"].tobytes()
    assert film.read_bgra8().astype(np.float32).tobytes() == dumps[0]["display_bgra8"].tobytes()
    film.close()


def test_pt_main_two_ranks_on_one_device_is_a_clean_error():
    """`pt_main --ranks 2 --devices 0,0`: RCCL refuses two ranks on one device.  The host threads agree on success before
    every collective (host/pt_main.cpp Agreement), so the process reports the error and exits -- it must not hang."""
    import subprocess
    repo = os.path.dirname(HERE)
    exe = os.path.join(repo, "single-file-vulkan-pathtracing_amd", "pt_main")
    r = subprocess.run([exe, "--obj", os.path.join(repo, "assets", "CornellBox-Original.obj"), "--width", "128", "--height", "64",
                        "--spp", "2", "--ranks", "2", "--devices", "0,0"], capture_output=True, text=True, timeout=180)
    assert r.returncode != 0, r.stdout
    assert "pt_main: rank" in r.stderr and ("pt_comm_create" in r.stderr or "RCCL" in r.stderr), r.stderr
    # ... and a rank with an ordinal that does not exist stops its peer before ncclCommInitRank
    r = subprocess.run([exe, "--obj", os.path.join(repo, "assets", "CornellBox-Original.obj"), "--width", "128", "--height", "64",
                        "--spp", "2", "--ranks", "2", "--devices", "0,99"], capture_output=True, text=True, timeout=180)
    assert r.returncode != 0 and "rank 1: pt_ctx_create" in r.stderr, r.stderr


def test_present_with_another_root_rebuilds_the_geometry(pt, gpu_ctx, cornell_gpu):
    """pt_film_present cached its tile lists and buffers per film size only; a later call with another root
    found no receive buffer.  World 1 has one possible root, so this checks the cache key through two film sizes and
    repeated presents; the root is part of the key now (csrc/present_rccl.hip)."""
    try:
        uid = pt.Comm.unique_id()
    except pt.PtError:
        pytest.skip("RCCL not installed")
    comm = pt.Comm(gpu_ctx, uid, 1, 0)
    for (w, h) in ((96, 40), (64, 64), (96, 40)):
        film = pt.Film(gpu_ctx, w, h)
        pt.render(cornell_gpu, film, pt.default_params(width=w, height=h, spp_per_frame=2, max_depth=4))
        img = pt.DeviceBuffer(gpu_ctx, w * h * 12)
        comm.present(film, img.ptr, root=0)
        assert img.read(np.float32, (h, w, 3)).tobytes() == film.read_f32().tobytes()
        img.close()
        film.close()
    comm.close()


def test_term_log_overflow_path_bit_exact(pt, orc, gpu_ctx, cornell_arrays):
    """Every surface emits, so every ray adds a radiance term: with sample groups the slots' logs run far past
    the dense primary part (group_size + 2 entries) into the overflow log.  Still the oracle's bits."""
    v, i, f = cornell_arrays
    f = f.reshape(-1, 6).copy()
    f[:, 3:] = np.float32(0.25) + f[:, :3] * np.float32(0.5)      # Ke > 0 everywhere
    gs, osc = pt.Scene(gpu_ctx, v, i, f.reshape(-1)), orc.Scene(v, i, f.reshape(-1))
    kw = dict(width=64, height=40, spp_per_frame=16, max_depth=12)
    ofilm, obgra, orays = _render_oracle(orc, osc, 2, **kw)
    for groups in (1, 2, 8, 16):
        film = pt.Film(gpu_ctx, 64, 40)
        gpu_ctx.reset_stats()
        pt.render(gs, film, pt.default_params(frame=0, frame_count=2, sample_groups=groups, **kw))
        assert gpu_ctx.stats().rays == orays
        assert film.read_f32().tobytes() == ofilm.tobytes(), groups
        assert film.read_bgra8().tobytes() == obgra.tobytes(), groups
        film.close()
    gs.close()


@pytest.mark.parametrize("shape", ["planar", "line", "far_from_origin", "huge"])
def test_fp16_node_boxes_stay_conservative_on_awkward_extents(pt, orc, gpu_ctx, shape):
    """The HBM traversal walks 64-B nodes whose boxes are fp16 of coordinates normalised to the scene box.
    Scenes with a degenerate axis, far from the origin or very large must still give the oracle's hits."""
    rng = np.random.default_rng(5)
    n = 3000
    v, i, f = _soup(n, 17, spread=0.05)
    v = v.reshape(n, 3, 3).copy()
    if shape == "planar":
        v[:, :, 2] = np.float32(0.25)                      # every triangle in the plane z = 0.25
    elif shape == "line":
        v[:, :, 1] = np.float32(-0.5); v[:, :, 2] *= np.float32(1e-3)
    elif shape == "far_from_origin":
        v += np.array([1000.0, -2000.0, 500.0], np.float32)
    elif shape == "huge":
        v *= np.float32(3.0e4)
    v = np.ascontiguousarray(v, np.float32).reshape(-1)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    ext = float((hi - lo).max())
    org = (rng.uniform(-0.2, 1.2, (40000, 3)) * (hi - lo) + lo + rng.normal(size=(40000, 3)) * 0.05 * ext).astype(np.float32)
    tgt = (rng.uniform(0, 1, (40000, 3)) * (hi - lo) + lo).astype(np.float32)
    rays = np.concatenate([org, (tgt - org) / np.linalg.norm(tgt - org, axis=1, keepdims=True)], axis=1).astype(np.float32)
    want, _ = osc.trace(rays, tmax=1e9)
    assert (want["prim"] != 0xFFFFFFFF).mean() > 0.05
    got = gs.trace(rays, tmax=1e9, extend=pt.EXTEND_HBM)
    assert got.tobytes() == want.tobytes(), shape
    gs.close()


def test_randomized_closest_hit_fuzz():
    """scripts/fuzz_trace.py: random scenes (scales 1e-3..1e4, far from the origin, planar, slivers, duplicates)
    and rays (axis-aligned, near-axis-aligned, starting on vertices) through every extend variant and both BVH
    qualities against the oracle; 800 scenes were run once by hand, 16 run here."""
    import subprocess
    import sys
    repo = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, os.path.join(repo, "scripts", "fuzz_trace.py"), "16", "77000"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "mismatching (scene, variant) pairs: 0" in out.stdout


def test_randomized_render_fuzz():
    """scripts/fuzz_render.py: random ragged film sizes, spp, depth, frame ranges, frames in flight, sample groups,
    rank/world splits, extend variants and cameras; film bits vs the oracle (1500 configurations run by hand)."""
    import subprocess
    import sys
    repo = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, os.path.join(repo, "scripts", "fuzz_render.py"), "40", "31000"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "mismatches: 0" in out.stdout


def test_randomized_instance_fuzz():
    """scripts/fuzz_instances.py: random base scenes x random instance sets (rotations, non-uniform and mirrored
    scales 0.005..15, translations up to 300, coincident instances) through the two-level extend kernel against the
    oracle's TLAS walk (and its brute force over every (instance, triangle)); 60 scenes ran clean by hand, 6 here."""
    import subprocess
    import sys
    repo = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, os.path.join(repo, "scripts", "fuzz_instances.py"), "6", "5100"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "mismatching scenes: 0" in out.stdout


# ---- the reference's own compiled shaders (tests/golden/spirv_pixels.npz, see tests/test_spirv_pin.py) -------------

def _spirv_fixture():
    return np.load(os.path.join(HERE, "golden", "spirv_pixels.npz"))


def test_spirv_reference_shaders_1080p_progressive(pt, gpu_ctx, cornell_gpu):
    """HIP path vs the outputs of shaders/*.spv executed by oracle/spirv_vm.py, with no oracle in between:
    1920x1080 launch, frames 0..2 one `pt_render` per frame as main.cpp:647-685 dispatches them, then the three
    frames batched in one call; float film at 275 pixels and the rgba8 display image at 46 pixels, every frame."""
    g = _spirv_fixture()
    w, h = [int(v) for v in g["a_launch"]]
    ax, ay = g["a_pixels"][:, 0], g["a_pixels"][:, 1]
    bx, by = g["b_pixels"][:, 0], g["b_pixels"][:, 1]
    kw = dict(width=w, height=h, spp_per_frame=32, max_depth=8)
    film = pt.Film(gpu_ctx, w, h)
    for frame in range(4):
        pt.render(cornell_gpu, film, pt.default_params(frame=frame, frame_count=1, **kw))
        if frame < g["a_texels"].shape[0]:
            got = np.ascontiguousarray(film.read_f32()[ay, ax])
            assert got.tobytes() == np.ascontiguousarray(g["a_texels"][frame, :, :3]).tobytes(), frame
        got8 = film.read_bgra8()[by, bx][:, [2, 1, 0, 3]]
        assert (got8 == g["b_rgba8"][frame]).all(), frame
    film.clear()
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=3, **kw))
    assert np.ascontiguousarray(film.read_f32()[ay, ax]).tobytes() == np.ascontiguousarray(g["a_texels"][2, :, :3]).tobytes()
    film.close()


@pytest.mark.parametrize("variant", [0, 2, 3, 4])
def test_spirv_reference_shaders_full_small_launch(pt, gpu_ctx, cornell_gpu, variant):
    """every invocation of a complete 120x68 launch, frames 0 and 1, every extend variant: texels and the exact
    number of traceRayEXT calls the reference's raygen made."""
    g = _spirv_fixture()
    w, h = [int(v) for v in g["c_launch"]]
    film = pt.Film(gpu_ctx, w, h)
    for frame in (0, 1):
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.default_params(width=w, height=h, spp_per_frame=32, max_depth=8, frame=frame,
                                                       frame_count=1, extend=variant))
        assert film.read_f32().tobytes() == np.ascontiguousarray(g["c_texels"][frame, :, :, :3]).tobytes()
        assert gpu_ctx.stats().rays == int(g["c_traces"][frame].sum())
    film.close()


def test_spirv_reference_shaders_c2_crop(pt, gpu_ctx, cornell_gpu):
    """BASELINE config 2 (1080p, 64 spp = 2 frames x 32, depth 8): the 96x64 rectangle at (912, 508) as the
    reference's shaders compute it."""
    g = _spirv_fixture()
    x0, y0, rw, rh = [int(v) for v in g["d_rect"]]
    film = pt.Film(gpu_ctx, 1920, 1080)
    pt.render(cornell_gpu, film, pt.default_params(width=1920, height=1080, spp_per_frame=32, max_depth=8, frame=0, frame_count=2))
    got = np.ascontiguousarray(film.read_f32()[y0:y0 + rh, x0:x0 + rw])
    assert got.tobytes() == np.ascontiguousarray(g["d_texels"][1, :, :, :3]).tobytes()
    film.close()


def test_negative_tmin_takes_the_wide_stack_entries(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle):
    """The no-spill LDS kernel packs a stack entry into one dword with the entry distance truncated toward zero,
    conservative only for t >= 0; a negative tmin (hits behind the origin count) must run the 8-byte-entry kernel
    and still give the oracle's records.  Rays start inside the box, so most have geometry on both sides."""
    rng = np.random.default_rng(11)
    n = 40000
    org = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-1.9, -0.1, n), rng.uniform(-0.9, 0.9, n)], 1)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([org, d], 1).astype(np.float32)
    for tmin in (-0.75, -1e-3, 0.0):
        want, _ = cornell_oracle.trace(rays, tmin=tmin, tmax=10.0, mode=0)
        for variant in (pt.EXTEND_AUTO, pt.EXTEND_LDS, pt.EXTEND_HBM):
            got = cornell_gpu.trace(rays, tmin=tmin, tmax=10.0, extend=variant)
            assert got.tobytes() == want.tobytes(), (tmin, variant)
    assert (want["t"] < 0.9).any()


@pytest.mark.parametrize("ocap,pool", [(0, 0), (3, 64), (0, None), (2, None)])
def test_full_term_log_spills_to_the_pool_or_the_batch_is_redone_exactly(pt, orc, gpu_ctx, cornell_arrays, cornell_gpu,
                                                                         cornell_oracle, ocap, pool):
    """The overflow part of the sample-group term log is sized to a memory budget, not to the worst case.  Terms beyond
    it go to a pool shared by all slots (per-slot chains, replayed in path order by k_resolve); when the pool is full
    too a flag is raised and the whole batch is rendered again with one group.  pt_tuning.term_ocap / .term_spill
    shrink both so that this happens at test sizes: (a) a scene where every surface emits (every ray logs a term),
    several batches and frames blended onto an existing film; (b) the Cornell box itself with the AUTO shape."""
    v, i, f = cornell_arrays
    f = f.reshape(-1, 6).copy()
    f[:, 3:] = np.float32(0.25) + f[:, :3] * np.float32(0.5)      # Ke > 0 everywhere
    gs, osc = pt.Scene(gpu_ctx, v, i, f.reshape(-1)), orc.Scene(v, i, f.reshape(-1))
    kw = dict(width=72, height=40, spp_per_frame=16, max_depth=12)
    ofilm, obgra, orays = _render_oracle(orc, osc, 5, **kw)
    gpu_ctx.set_tuning(term_ocap=ocap, term_spill=-1 if pool is None else pool)
    try:
        film = pt.Film(gpu_ctx, 72, 40)
        gpu_ctx.reset_stats()
        pt.render(gs, film, pt.default_params(frame=0, frame_count=1, sample_groups=4, **kw))            # 1 batch
        pt.render(gs, film, pt.default_params(frame=1, frame_count=4, sample_groups=8, frames_in_flight=2,
                                              flags=pt.FLAG_PROFILE, **kw))                               # 2 batches
        st = gpu_ctx.stats()
        assert st.redone_batches == (3 if pool is not None else 0)       # the default pool (4 M entries) absorbs it all
        assert st.rays == orays and st.paths == 72 * 40 * 16 * 5
        assert film.read_f32().tobytes() == ofilm.tobytes()
        assert film.read_bgra8().tobytes() == obgra.tobytes()
        film.close()
        # (b) the reference's scene, AUTO shape: exact whether terms spill, a batch is redone, or neither
        kw = dict(width=96, height=64, spp_per_frame=32, max_depth=8)
        ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, 2, **kw)
        film = pt.Film(gpu_ctx, 96, 64)
        for groups in (0, 4):
            film.clear()
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=2, sample_groups=groups, **kw))
            st = gpu_ctx.stats()
            assert st.sample_groups > 1 and st.redone_batches <= 1
            assert st.rays == orays and film.read_f32().tobytes() == ofilm.tobytes()
        gpu_ctx.set_tuning(term_ocap=-1, term_spill=-1)
        film.clear()
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=2, **kw))
        assert gpu_ctx.stats().redone_batches == 0 and gpu_ctx.stats().rays == orays
        assert film.read_f32().tobytes() == ofilm.tobytes()
        film.close()
    finally:
        gpu_ctx.set_tuning(term_ocap=-1, term_spill=-1)
        gs.close()


def test_spill_pool_at_full_size_two_pipelines(pt, gpu_ctx, cornell_gpu):
    """1080p, 4 frames x 4 sample groups (33 M slots, two pipelines) with a one-entry overflow log: tens of thousands of
    slots chain terms into the shared pool.  Same film and ray count as the single-group render, nothing redone."""
    kw = dict(width=1920, height=1080, spp_per_frame=32, max_depth=8, frame=0, frame_count=4)
    a, b = pt.Film(gpu_ctx, 1920, 1080), pt.Film(gpu_ctx, 1920, 1080)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, a, pt.default_params(sample_groups=1, **kw))
    rays = gpu_ctx.stats().rays
    gpu_ctx.set_tuning(term_ocap=1)
    try:
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, b, pt.default_params(sample_groups=4, **kw))
    finally:
        gpu_ctx.set_tuning(term_ocap=-1)
    st = gpu_ctx.stats()
    assert st.sample_groups == 4 and st.redone_batches == 0 and st.rays == rays
    assert a.read_f32().tobytes() == b.read_f32().tobytes()
    assert a.read_bgra8().tobytes() == b.read_bgra8().tobytes()
    a.close(); b.close()


@pytest.mark.parametrize("n_coincident", [150, 500, 2048])
def test_coincident_triangles_deep_sah_tree_keeps_the_stack_in_bounds(pt, orc, gpu_ctx, n_coincident):
    """n copies of ONE triangle (+ a few others): every split of the surface-area sweep costs the same, which used to give
    a chain n/3 deep whose traversal stack overran a spill region sized from the balanced LBVH's height.  The sweep now
    falls back to median splits below depth 24 and the spill region is sized from the stack bound of the BVH4 that is
    traversed.  Hits (closest t, lowest primitive id among the coincident ones) equal the oracle's on every variant,
    for both builders, also as a BLAS under instances."""
    rng = np.random.default_rng(5)
    one = np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, 0.0], [0.0, 0.7, -0.1]], np.float32)
    extra = rng.uniform(-1, 1, (16, 3, 3)).astype(np.float32)
    tris = np.concatenate([np.repeat(one[None], n_coincident - 16, 0), extra])
    v = tris.reshape(-1)
    i = np.arange(v.size // 3, dtype=np.uint32)
    f = rng.uniform(0, 1, (len(tris), 6)).astype(np.float32).reshape(-1)
    n = 30000
    org = rng.uniform(-1.5, 1.5, (n, 3))
    d = rng.normal(size=(n, 3))
    bary = rng.dirichlet([1, 1, 1], n // 2)                       # half of the rays aim at the coincident stack
    d[:n // 2] = bary @ one.astype(np.float64) - org[:n // 2]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([org, d], 1).astype(np.float32)
    osc = orc.Scene(v, i, f)
    want, _ = osc.trace(rays, tmin=0.001, tmax=100.0, mode=0)
    assert (want["prim"] == 0).sum() > 1000        # the coincident stack is hit, and its lowest id wins
    gs = pt.Scene(gpu_ctx, v, i, f)
    for quality in (pt.BVH_PREFER_FAST_TRACE, pt.BVH_PREFER_FAST_BUILD):
        gs.set_bvh_quality(quality)
        for variant in (pt.EXTEND_AUTO, pt.EXTEND_LDS if n_coincident <= 150 else pt.EXTEND_AUTO, pt.EXTEND_HBM):
            got = gs.trace(rays, tmin=0.001, tmax=100.0, extend=variant)
            assert got.tobytes() == want.tobytes(), (quality, variant)
    gs.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)
    xf = np.zeros((3, 3, 4), np.float32)
    for k in range(3):
        xf[k, 0, 0] = xf[k, 1, 1] = xf[k, 2, 2] = 0.5
        xf[k, :, 3] = [k - 1.0, 0.1 * k, 0.0]
    gs.set_instances(xf)
    osc.set_instances(xf)
    want, _ = osc.trace(rays, tmin=0.001, tmax=100.0, mode=1)
    assert gs.trace(rays, tmin=0.001, tmax=100.0).tobytes() == want.tobytes()
    gs.close()


def test_workspace_out_of_memory_is_reported_and_the_film_stays_usable(pt, orc, cornell_arrays, cornell_oracle):
    """PT_MEM_BUDGET_MB (read at pt_ctx_create) caps the wavefront workspace.  An explicit shape that does not fit is
    PT_ERR_OOM with nothing rendered; the film keeps its content and the next render -- AUTO shape, which plans for
    the memory there is -- continues it bit-exactly."""
    w, h = 256, 160
    kw = dict(width=w, height=h, spp_per_frame=8, max_depth=8)
    ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, 3, **kw)
    os.environ["PT_MEM_BUDGET_MB"] = "48"
    try:
        ctx = pt.Context(0)
    finally:
        os.environ.pop("PT_MEM_BUDGET_MB", None)
    scene = pt.Scene(ctx, *cornell_arrays)
    film = pt.Film(ctx, w, h)
    pt.render(scene, film, pt.default_params(frame=0, frame_count=1, **kw))              # fits: 41 k slots
    before = film.read_f32()
    with pytest.raises(pt.PtError) as e:                                                   # 64 frames x 8 groups: 2.6 GB
        pt.render(scene, film, pt.default_params(frame=1, frame_count=64, frames_in_flight=64, sample_groups=8, **kw))
    assert e.value.status == 4 and "budget" in str(e.value)                                # PT_ERR_OOM
    with pytest.raises(pt.PtError) as e:
        pt.render_prepare(scene, film, pt.default_params(frame=1, frame_count=64, frames_in_flight=64, sample_groups=8, **kw))
    assert e.value.status == 4
    assert film.read_f32().tobytes() == before.tobytes()                                   # nothing was blended
    ctx.reset_stats()
    pt.render(scene, film, pt.default_params(frame=1, frame_count=2, **kw))                # AUTO shrinks to the budget
    st = ctx.stats()
    assert st.frames_in_flight * st.sample_groups * w * h * 124 <= 48 << 20
    assert film.read_f32().tobytes() == ofilm.tobytes() and film.read_bgra8().tobytes() == obgra.tobytes()
    # a long AUTO render under the same budget: many small batches, same bits as one frame at a time
    a = pt.Film(ctx, w, h)
    pt.render(scene, a, pt.default_params(frame=0, frame_count=3, **kw))
    assert a.read_f32().tobytes() == ofilm.tobytes()
    # the same under what pt_params_default gives (PT_PIPELINE_AUTO: the fused kernel plans its slots and logs within the same budget) ...
    b = pt.Film(ctx, w, h)
    ctx.reset_stats()
    pt.render(scene, b, pt.library_default_params(frame=0, frame_count=3, **kw))
    assert ctx.stats().pipeline == pt.PIPELINE_FUSED and ctx.stats().rays == orays and ctx.stats().workspace_bytes <= 48 << 20
    assert b.read_f32().tobytes() == ofilm.tobytes() and b.read_bgra8().tobytes() == obgra.tobytes()
    # ... and an explicit fused shape that does not fit is the same clean error, the film untouched
    with pytest.raises(pt.PtError) as e:
        pt.render(scene, b, pt.library_default_params(frame=3, frame_count=64, frames_in_flight=64, sample_groups=8, pipeline=pt.PIPELINE_FUSED, **kw))
    assert e.value.status == 4
    assert b.read_f32().tobytes() == ofilm.tobytes()
    a.close(); b.close(); film.close(); scene.close(); ctx.close()


def test_present_pack_unpack_kernels_assemble_the_single_device_film(pt, gpu_ctx, cornell_gpu):
    """pt_film_present's two kernels without a communicator: the shards of world = 3 and 8 (ragged 250x131 image, partial
    edge tiles) are packed per rank and unpacked into one image = the single-device film, bit for bit; the device
    kernels agree with their numpy mirrors (what the gloo world-2 test runs on the CPU)."""
    import importlib
    d = importlib.import_module("single-file-vulkan-pathtracing_amd.distributed")
    w, h = 250, 131
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=8, frame=0, frame_count=2)
    full = pt.Film(gpu_ctx, w, h)
    pt.render(cornell_gpu, full, pt.default_params(**kw))
    want = full.read_f32()
    for world in (3, 8):
        image = pt.DeviceBuffer(gpu_ctx, w * h * 12)
        n_total = 0
        for rank in range(world):
            film = pt.Film(gpu_ctx, w, h)
            pt.render(cornell_gpu, film, pt.default_params(rank=rank, world=world, **kw))
            n = pt.film_tile_count(film, rank, world)
            assert n == len(d.tile_list(w, h, rank, world))
            n_total += n
            packed = pt.DeviceBuffer(gpu_ctx, max(n, 1) * 192 * 4)
            pt.film_pack_tiles(film, rank, world, packed.ptr)
            host = packed.read(np.float32, (n, 64, 3))
            assert host.tobytes() == d.pack_tiles_host(film.read_f32(), rank, world).tobytes()
            pt.film_unpack_tiles(film, rank, world, packed.ptr, image.ptr)
            packed.close(); film.close()
        assert n_total == ((w + 7) // 8) * ((h + 7) // 8)
        assert image.read(np.float32, (h, w, 3)).tobytes() == want.tobytes()
        image.close()
    full.close()


def test_present_through_rccl_world_1(pt, gpu_ctx, cornell_gpu):
    """The library's own RCCL communicator (dlopen'ed librccl, ncclCommInitRank) with one rank: pt_film_present packs,
    has nothing to gather, and unpacks into a SEPARATE image equal to the film; the film itself is untouched and can be
    rendered further and presented again (the old in-place reduce could not)."""
    w, h = 200, 120
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=8)
    film = pt.Film(gpu_ctx, w, h)
    comm = pt.Comm(gpu_ctx, pt.Comm.unique_id(), 1, 0)
    assert comm.ranks() == 1
    image = pt.DeviceBuffer(gpu_ctx, w * h * 12)
    for frame in range(3):
        pt.render(cornell_gpu, film, pt.default_params(frame=frame, frame_count=1, **kw))
        comm.present(film, image.ptr, root=0)
        assert image.read(np.float32, (h, w, 3)).tobytes() == film.read_f32().tobytes()
    ref = pt.Film(gpu_ctx, w, h)
    pt.render(cornell_gpu, ref, pt.default_params(frame=0, frame_count=3, **kw))
    assert film.read_f32().tobytes() == ref.read_f32().tobytes()
    with pytest.raises(pt.PtError):                                    # rendered as (0, 1), presented as another shape
        other = pt.Film(gpu_ctx, w, h)
        pt.render(cornell_gpu, other, pt.default_params(frame=0, frame_count=1, rank=1, world=2, **kw))
        comm.present(other, image.ptr, root=0)
    image.close(); comm.close(); film.close(); ref.close()


def _two_gpus():
    try:
        import torch
        return torch.cuda.device_count() >= 2
    except Exception:
        return False


@pytest.mark.skipif(not _two_gpus(), reason="needs >= 2 GPUs (RCCL cannot place two ranks on one device)")
def test_pt_main_two_ranks_over_rccl_equals_one_rank(tmp_path):
    """host/pt_main --ranks 2: two host threads, two GPUs, tiles interleaved, one RCCL gather of the packed tiles to rank
    0 -- the presented image equals the single-GPU image bit for bit, the ray counts add up."""
    import json
    import subprocess
    repo = os.path.dirname(HERE)
    exe = os.path.join(repo, "single-file-vulkan-pathtracing_amd", "pt_main")
    args = ["--obj", os.path.join(repo, "assets", "CornellBox-Original.obj"), "--width", "320", "--height", "200", "--frames", "2",
            "--spp", "8"]
    one = subprocess.run([exe] + args + ["--pfm", str(tmp_path / "one.pfm")], capture_output=True, text=True, timeout=600)
    two = subprocess.run([exe] + args + ["--ranks", "2", "--pfm", str(tmp_path / "two.pfm")], capture_output=True, text=True, timeout=600)
    assert one.returncode == 0 and two.returncode == 0, (one.stderr, two.stderr)
    j1, j2 = json.loads(one.stdout), json.loads(two.stdout)
    assert j2["ranks"] == 2 and j2["rccl_ranks"] == 2 and j2["rays"] == j1["rays"] and j2["paths"] == j1["paths"]
    assert open(tmp_path / "one.pfm", "rb").read() == open(tmp_path / "two.pfm", "rb").read()


def test_pair_leaves_fan_quads_share_work_but_not_bits(pt, orc, gpu_ctx, cornell_arrays, cornell_oracle):
    """The surface-area BVH4 of small scenes holds ONE primitive per leaf, a primitive being a triangle or the two halves
    (v0,v1,v2),(v0,v2,v3) of a quad, and the LDS kernel tests such a pair with shared vertex transforms and edge products.
    (a) Cornell: 18 two-triangle leaves, each a fan pair in input order.  (b) a scene mixing fan quads, lone triangles,
    a reversed-winding 'pair' that must NOT be paired, and duplicated quads: hit records equal the oracle's on every
    kernel variant, for rays through the shared diagonals (where the shared edge function is exactly 0 on both halves),
    through vertices, and random ones; tmin <= 0 takes the 8-byte-entry kernel over the same tree."""
    sc = pt.Scene(gpu_ctx, *cornell_arrays)
    wide = sc.read_bvh4()
    words = wide[:, 24:28].ravel()
    leaves = words[(words != 0xFFFFFFFF) & (words & 0x80000000 != 0)]
    assert len(leaves) == 18 and all(int((w >> 28) & 7) == 1 for w in leaves)
    sc.close()
    rng = np.random.default_rng(21)
    tris = []
    quads = []
    for k in range(40):                                  # planar and non-planar fan quads
        c = rng.uniform(-1, 1, 3)
        e1, e2 = rng.normal(size=3) * 0.4, rng.normal(size=3) * 0.4
        q = np.array([c, c + e1, c + e1 + e2 + rng.normal(size=3) * (0.05 if k % 3 == 0 else 0.0), c + e2])
        quads.append(q)
        tris += [q[[0, 1, 2]], q[[0, 2, 3]]]
        if k % 10 == 0:                                   # duplicated quad: coincident, lowest primitive id wins
            tris += [q[[0, 1, 2]], q[[0, 2, 3]]]
    for k in range(25):
        tris.append(rng.uniform(-1, 1, (3, 3)))           # lone triangles
    q = quads[0] + np.array([0.0, 0.0, 2.5])
    tris += [q[[0, 1, 2]], q[[2, 3, 0]]]                  # shares the diagonal but is not the fan pattern
    tris = np.array(tris, np.float32)
    v = tris.reshape(-1)
    i = np.arange(v.size // 3, dtype=np.uint32)
    f = rng.uniform(0, 1, (len(tris), 6)).astype(np.float32).reshape(-1)
    rays = []
    for q in quads:
        q = q.astype(np.float32).astype(np.float64)
        for s in rng.uniform(0.02, 0.98, 40):
            target = q[0] * (1 - s) + q[2] * s            # a point on the shared diagonal
            o = target + rng.normal(size=3)
            rays.append(np.concatenate([o, target - o]))
        for k in range(4):                                # through the vertices
            o = q[k] + rng.normal(size=3)
            rays.append(np.concatenate([o, q[k] - o]))
    rays = np.array(rays)
    rnd = np.concatenate([rng.uniform(-2, 2, (40000, 3)), rng.normal(size=(40000, 3))], 1)
    rays = np.concatenate([rays, rnd]).astype(np.float32)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    assert gs.info().bvh4_builder == 1
    wide = gs.read_bvh4()
    words = wide[:, 24:28].ravel()
    leaves = words[(words != 0xFFFFFFFF) & (words & 0x80000000 != 0)]
    n_pair = sum(int((w >> 28) & 7) == 1 for w in leaves)
    assert n_pair == 44 and len(leaves) == 44 + 25 + 2    # 40 quads + 4 duplicates paired; the reversed one is two singles
    for tmin in (0.001, 0.0, -0.5):
        want, _ = osc.trace(rays, tmin=tmin, tmax=100.0, mode=0)
        for variant in (pt.EXTEND_AUTO, pt.EXTEND_LDS, pt.EXTEND_HBM):
            got = gs.trace(rays, tmin=tmin, tmax=100.0, extend=variant)
            assert got.tobytes() == want.tobytes(), (tmin, variant)
    assert (want["prim"] != 0xFFFFFFFF).sum() > 5000
    gpu_ctx.set_tuning(pair_kernel=0)                       # the per-triangle kernel over the same pair-leaf tree
    try:
        want, _ = osc.trace(rays, tmin=0.001, tmax=100.0, mode=0)
        assert gs.trace(rays, tmin=0.001, tmax=100.0).tobytes() == want.tobytes()
    finally:
        gpu_ctx.set_tuning(pair_kernel=-1)
    gs.close()


def _half(u16):
    return np.asarray(u16, np.uint16).view(np.float16).astype(np.float64)


def _check_bvh8(pt, gs, v, n):
    """structure of the 8-wide tree: contiguous children, every triangle in exactly one leaf slot, decoded byte-plane boxes
    that contain their triangles (through every level)"""
    nodes, prim8 = gs.read_bvh8()
    info = gs.info()
    assert nodes.shape[0] == info.n_wide8_nodes >= 1 and sorted(prim8.tolist()) == list(range(n))
    bmin, bmax = np.array(list(info.bbox_min), np.float64), np.array(list(info.bbox_max), np.float64)
    ext = (bmax - bmin).max()
    c, s = 0.5 * (bmin + bmax), np.maximum(0.5 * (bmax - bmin), max(ext * 2.0 ** -10, 1e-30))
    tri = np.asarray(v, np.float64).reshape(-1, 3, 3)
    # 64-B nodes: byte planes on the node's grid (include/pt_api.h pt_scene_read_bvh8)
    q = nodes[:, :12].copy().view(np.uint8).reshape(-1, 6, 8).astype(np.float64)   # [node][lo.x lo.y lo.z hi.x hi.y hi.z][slot]
    o16 = np.stack([nodes[:, 12] & 0xFFFF, nodes[:, 12] >> 16, nodes[:, 13] & 0xFFFF], 1).astype(np.float64)
    ecode = np.stack([(nodes[:, 13] >> 16) & 31, (nodes[:, 13] >> 21) & 31, nodes[:, 13] >> 26], 1).astype(np.float64)
    origin, step = o16 * 2.0 ** -14 - 2.0, 2.0 ** -ecode
    lo = (origin[:, :, None] + q[:, 0:3, :] * step[:, :, None]) * s[None, :, None] + c[None, :, None]
    hi = (origin[:, :, None] + q[:, 3:6, :] * step[:, :, None]) * s[None, :, None] + c[None, :, None]
    child_base, tri_base = nodes[:, 14] & 0xFFFFFF, nodes[:, 15] & 0xFFFFFF
    imask, lmask = nodes[:, 14] >> 24, nodes[:, 15] >> 24
    assert ((imask & lmask) == 0).all()
    seen_node = np.zeros(len(nodes), np.int64)
    seen_tri = np.zeros(n, np.int64)
    # subtree boxes bottom-up: nodes of a level come after their parents, so walk the array backwards
    sub_lo = np.full((len(nodes), 3), np.inf)
    sub_hi = np.full((len(nodes), 3), -np.inf)
    tol = 1e-6 * max(ext, 1e-30)
    for i in range(len(nodes) - 1, -1, -1):
        ni = nl = 0
        for sl in range(8):
            if imask[i] >> sl & 1:
                ch = child_base[i] + ni
                ni += 1
                assert i < ch < len(nodes)
                seen_node[ch] += 1
                assert (lo[i, :, sl] <= sub_lo[ch] + tol).all() and (hi[i, :, sl] >= sub_hi[ch] - tol).all()
                sub_lo[i] = np.minimum(sub_lo[i], sub_lo[ch]); sub_hi[i] = np.maximum(sub_hi[i], sub_hi[ch])
            elif lmask[i] >> sl & 1:
                pos = tri_base[i] + nl
                nl += 1
                seen_tri[pos] += 1
                t = tri[prim8[pos]]
                assert (lo[i, :, sl] <= t.min(0) + tol).all() and (hi[i, :, sl] >= t.max(0) - tol).all()
                sub_lo[i] = np.minimum(sub_lo[i], t.min(0)); sub_hi[i] = np.maximum(sub_hi[i], t.max(0))
            else:
                assert (q[i, 0:3, sl] == 255).all() and (q[i, 3:6, sl] == 0).all()     # empty slot: an inverted interval on every axis
    assert (seen_tri == 1).all() and seen_node[0] == 0 and (seen_node[1:] == 1).all()
    return info


@pytest.mark.parametrize("n,seed,spread", [(0, 0, 0), (2, 2, 0.3), (3, 3, 0.3), (9, 4, 0.3), (100, 5, 0.3), (5000, 6, 0.1), (60000, 7, 0.02)])
def test_bvh8_structure_and_hits(pt, orc, gpu_ctx, cornell_arrays, n, seed, spread):
    """The BVH8 of scenes that are walked out of L2 / MALL / HBM (n = 0: the Cornell box, which AUTO keeps in LDS but which
    has one all the same): valid tree, and PT_EXTEND_HBM8 returns the oracle's hit records bit for bit -- random rays, rays
    along the axes (zero direction components) and from inside the boxes; a negative tmin too."""
    v, i, f = cornell_arrays if n == 0 else _soup(n, seed, spread=spread)
    nt = len(i) // 3
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    info = _check_bvh8(pt, gs, v, nt)
    assert info.wide8_levels >= 1 and info.n_wide8_nodes <= max(nt - 1, 1)
    rng = np.random.default_rng(seed)
    m = 40000
    org = rng.uniform(-1.3, 1.3, (m, 3))
    d = rng.normal(size=(m, 3))
    d[:300] = np.eye(3)[rng.integers(0, 3, 300)] * rng.choice([-1.0, 1.0], (300, 1))     # axis-parallel
    tri = np.asarray(v, np.float64).reshape(-1, 3, 3)
    tgt = tri[rng.integers(0, nt, m // 2)].mean(1)                                          # half aim at triangles
    d[m // 2:] = tgt - org[m // 2:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([org, d], 1).astype(np.float32)
    for tmin in (0.001, -0.25):
        want, _ = osc.trace(rays, tmin=tmin, tmax=50.0)
        got = gs.trace(rays, tmin=tmin, tmax=50.0, extend=pt.EXTEND_HBM8)
        assert got.tobytes() == want.tobytes(), (n, tmin)
    assert (want["prim"] != 0xFFFFFFFF).sum() > m // 4
    gs.close()


def test_bvh8_render_bit_exact_and_auto_selection(pt, orc, gpu_ctx):
    """A 30 000-triangle soup (does not fit LDS): PT_EXTEND_HBM walks the BVH4, PT_EXTEND_HBM8 and -- beyond 1 MiB of nodes + records,
    about 11 000 triangles -- AUTO the 8-wide tree; all render the oracle's film and ray count, progressive frames, sample groups
    and two pipelines included (k_shade reads the per-triangle tables in the order of whichever tree was walked).  A 6 000-triangle
    soup stays with the BVH4 kernel under AUTO."""
    v, i, f = _soup(30000, 11, spread=0.05)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    kw = dict(width=160, height=96, spp_per_frame=4, max_depth=6)
    ofilm, obgra, orays = _render_oracle(orc, osc, 3, **kw)
    for extend, name in ((pt.EXTEND_AUTO, 4), (pt.EXTEND_HBM8, 4), (pt.EXTEND_HBM, 3)):
        film = pt.Film(gpu_ctx, 160, 96)
        gpu_ctx.reset_stats()
        pt.render(gs, film, pt.default_params(frame=0, frame_count=1, extend=extend, **kw))
        pt.render(gs, film, pt.default_params(frame=1, frame_count=2, extend=extend, sample_groups=2, flags=pt.FLAG_COUNT_VISITS, **kw))
        st = gpu_ctx.stats()
        assert st.extend_variant == name and st.rays == orays and st.nodes_visited > 0 and st.tris_tested > 0
        assert film.read_f32().tobytes() == ofilm.tobytes() and film.read_bgra8().tobytes() == obgra.tobytes()
        film.close()
    gs.close()
    v, i, f = _soup(6000, 12, spread=0.05)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    ofilm, _, orays = _render_oracle(orc, osc, 1, **kw)
    film = pt.Film(gpu_ctx, 160, 96)
    gpu_ctx.reset_stats()
    pt.render(gs, film, pt.default_params(frame=0, frame_count=1, **kw))
    assert gpu_ctx.stats().extend_variant == pt.EXTEND_HBM and gpu_ctx.stats().rays == orays
    assert film.read_f32().tobytes() == ofilm.tobytes()
    film.close()
    gs.close()


@pytest.mark.parametrize("knobs", [dict(tri_enter=1, tri_stay=1), dict(tri_enter=8, tri_stay=4), dict(tri_enter=16, tri_stay=65),
                                   dict(tri_enter=64, tri_stay=1), dict(tri_enter=24, tri_stay=12, refill=8),
                                   dict(extend_blocks=7), dict(extend_blocks=6, lds_stack=3), dict(lds_stack=1, tri_enter=5)])
def test_bvh8_vote_knobs_keep_the_bits(pt, orc, gpu_ctx, knobs):
    """The vote of the 8-wide kernel (extend8_kernel.h: how many lanes wait with leaf triangles before a triangle step runs,
    and how long triangle steps repeat) decides the order in which a ray's candidates are met, never which hit it returns;
    nor does the instantiation: 7 waves per SIMD (extend_blocks = 7), or the spill kernel (fewer LDS stack entries than levels):
    hit records (closest-hit and a negative tmin) and a rendered film equal the oracle's under every setting."""
    v, i, f = _soup(20000, 23, spread=0.05)
    old = gpu_ctx.set_tuning(**knobs)
    try:
        gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
        rng = np.random.default_rng(5)
        m = 30000
        org = rng.uniform(-1.3, 1.3, (m, 3))
        d = rng.normal(size=(m, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.concatenate([org, d], 1).astype(np.float32)
        for tmin in (0.001, -0.25):
            want, _ = osc.trace(rays, tmin=tmin, tmax=50.0)
            for extend in (pt.EXTEND_HBM8, pt.EXTEND_HBM):     # (the BVH4 kernel of mid-size scenes takes the same knob)
                got = gs.trace(rays, tmin=tmin, tmax=50.0, extend=extend)
                assert got.tobytes() == want.tobytes(), (knobs, tmin, extend)
        kw = dict(width=160, height=96, spp_per_frame=4, max_depth=6)
        ofilm, _, orays = _render_oracle(orc, osc, 2, **kw)
        film = pt.Film(gpu_ctx, 160, 96)
        gpu_ctx.reset_stats()
        pt.render(gs, film, pt.default_params(frame=0, frame_count=2, extend=pt.EXTEND_HBM8, **kw))
        assert gpu_ctx.stats().rays == orays and film.read_f32().tobytes() == ofilm.tobytes(), knobs
        film.close(); gs.close()
    finally:
        gpu_ctx.set_tuning(**old)


@pytest.mark.parametrize("extend", [3, 4])
def test_ray_sorting_changes_no_bit(pt, orc, gpu_ctx, extend):
    """PT_FLAG_SORT_RAYS: before every extend pass after the first the queue is walked in (origin cell, direction octant)
    order through a permutation sorted on the device.  Film, display image and ray count equal the oracle's and the
    unsorted render's -- one pipeline and two, sample groups, progressive frames, BVH4 and BVH8 kernels."""
    v, i, f = _soup(30000, 17, spread=0.05)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    kw = dict(width=160, height=96, spp_per_frame=4, max_depth=6)
    ofilm, obgra, orays = _render_oracle(orc, osc, 3, **kw)
    for flags, groups in ((pt.FLAG_SORT_RAYS, 0), (pt.FLAG_SORT_RAYS | pt.FLAG_COUNT_VISITS, 2), (pt.FLAG_NO_SORT_RAYS, 0)):
        film = pt.Film(gpu_ctx, 160, 96)
        gpu_ctx.reset_stats()
        pt.render(gs, film, pt.default_params(frame=0, frame_count=1, extend=extend, flags=flags, **kw))
        pt.render(gs, film, pt.default_params(frame=1, frame_count=2, extend=extend, flags=flags, sample_groups=groups, **kw))
        assert gpu_ctx.stats().rays == orays
        assert film.read_f32().tobytes() == ofilm.tobytes() and film.read_bgra8().tobytes() == obgra.tobytes()
        film.close()
    # two pipelines (>= 4 M slots): 1080p, 1 spp x 2 groups... a large launch, compared with its unsorted twin
    kw = dict(width=1920, height=1080, spp_per_frame=2, max_depth=5, frame=0, frame_count=2, extend=extend)
    a, b = pt.Film(gpu_ctx, 1920, 1080), pt.Film(gpu_ctx, 1920, 1080)
    gpu_ctx.reset_stats()
    pt.render(gs, a, pt.default_params(flags=pt.FLAG_NO_SORT_RAYS, **kw))
    rays = gpu_ctx.stats().rays
    gpu_ctx.reset_stats()
    pt.render(gs, b, pt.default_params(flags=pt.FLAG_SORT_RAYS, **kw))
    assert gpu_ctx.stats().rays == rays and a.read_f32().tobytes() == b.read_f32().tobytes()
    a.close(); b.close(); gs.close()


def _render_oracle_nee(orc, osc, frames, **kw):
    film, rays = None, 0
    for k in range(frames):
        img, r, _, _ = osc.render_frame(orc.default_params(frame=k, nee=1, **kw))
        if film is None:
            film = np.zeros_like(img)
        orc.accumulate_f32(film, img, k)
        rays += r
    return film, rays


@pytest.mark.parametrize("extend", [0, 2, 3, 4])
def test_nee_pipeline_equals_the_oracles_nee_mode(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, extend):
    """PT_PIPELINE_WAVEFRONT_NEE (opt-in, not the reference's estimator): shade queues one shadow ray per hit whose light
    sample faces it, the extend kernels trace them as any-hit queries with a per-ray tmax, and the unoccluded contributions
    are added in path order.  Film and the count of ALL rays (path + shadow) equal the oracle's own `nee` mode bit for bit, on
    every extend variant that takes a per-ray tmax, progressive frames and several frames in flight."""
    kw = dict(width=80, height=56, spp_per_frame=8, max_depth=8)
    ofilm, orays = _render_oracle_nee(orc, cornell_oracle, 3, **kw)
    film = pt.Film(gpu_ctx, 80, 56)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=1, pipeline=pt.PIPELINE_WAVEFRONT_NEE, extend=extend, **kw))
    pt.render(cornell_gpu, film, pt.default_params(frame=1, frame_count=2, pipeline=pt.PIPELINE_WAVEFRONT_NEE, extend=extend,
                                                   frames_in_flight=2, **kw))
    st = gpu_ctx.stats()
    assert st.rays == orays and st.sample_groups == 1
    assert film.read_f32().tobytes() == ofilm.tobytes()
    for bad in (dict(extend=1), dict(sample_groups=4)):
        with pytest.raises(pt.PtError):
            pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=1, pipeline=pt.PIPELINE_WAVEFRONT_NEE, **dict(kw, **bad)))
    film.close()


def test_nee_pipeline_on_a_soup_with_many_emitters(pt, orc, gpu_ctx):
    """20 000 triangles, a tenth of them emitters (cdf search over 2 000 lights, tables in HBM, two pipelines' worth of
    slots at this size are not reached: one pipeline), BVH4 and BVH8 kernels, with and without ray sorting."""
    v, i, f = _soup(20000, 23, spread=0.06)
    gs, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    kw = dict(width=96, height=64, spp_per_frame=4, max_depth=5)
    ofilm, orays = _render_oracle_nee(orc, osc, 2, **kw)
    for extend, flags in ((pt.EXTEND_AUTO, 0), (pt.EXTEND_HBM8, 0), (pt.EXTEND_HBM, pt.FLAG_SORT_RAYS)):
        film = pt.Film(gpu_ctx, 96, 64)
        gpu_ctx.reset_stats()
        pt.render(gs, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_WAVEFRONT_NEE, extend=extend, flags=flags, **kw))
        assert gpu_ctx.stats().rays == orays
        assert film.read_f32().tobytes() == ofilm.tobytes(), extend
        film.close()
    gs.close()


@pytest.mark.parametrize("knobs", [dict(), dict(inst16=0)])
def test_nee_pipeline_on_instanced_scenes(pt, orc, gpu_ctx, cornell_arrays, knobs):
    """NEE x instances: the emitters of an instanced scene are every instance's copy in world space (one
    cdf over all of them), the shadow rays walk TLAS + BLAS as any-hit queries with a per-ray tmax -- through the compact
    two-level kernel and the general one.  Film and the count of all rays equal the oracle's nee mode bit for bit: 7 random
    instances (rotated, scaled) and a 12 x 12 corner of config C4's grid."""
    grid = pt.cornell_grid_instances().reshape(100, 100, 3, 4)[:12, :12].reshape(-1, 3, 4)
    old = gpu_ctx.set_tuning(**knobs)
    try:
        for inst, cam in ((_random_instances(7, 3), {}), (grid, dict(cam_origin=(-0.88, -1.9, 0.5), cam_target=(-0.88, -1.9, 0.0)))):
            gs, osc = pt.Scene(gpu_ctx, *cornell_arrays), orc.Scene(*cornell_arrays)
            gs.set_instances(inst)
            osc.set_instances(inst)
            kw = dict(width=80, height=56, spp_per_frame=4, max_depth=6, **cam)
            ofilm, orays = _render_oracle_nee(orc, osc, 2, **kw)
            film = pt.Film(gpu_ctx, 80, 56)
            gpu_ctx.reset_stats()
            pt.render(gs, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_WAVEFRONT_NEE, **kw))
            assert gpu_ctx.stats().rays == orays, knobs
            assert film.read_f32().tobytes() == ofilm.tobytes(), knobs
            assert ofilm.mean() > 0.05
            film.close(); gs.close()
    finally:
        gpu_ctx.set_tuning(**old)


def test_nee_converges_to_the_reference_estimators_mean(pt, gpu_ctx, cornell_gpu):
    """Same expectation, other variance: at 1024 spp on a 64x64 Cornell box the NEE image and the reference estimator's agree
    in the mean of the image to 1 % and tile by tile (8x8 pixels) to 3 % on average; the reference estimator's own two halves
    (frames 0-31 against 32-63) set the scale."""
    w = h = 64
    kw = dict(width=w, height=h, spp_per_frame=32, max_depth=8)
    def mean_of(frames, first, pipeline):
        acc = np.zeros((h, w, 3), np.float64)
        for k in range(frames):
            film = pt.Film(gpu_ctx, w, h)
            # a film's first frame must be frame 0 for the running mean; the seed depends on (frame, sample): render frame
            # `first + k` alone into a scratch film whose previous content is weighted by frame/(frame+1) -> undo that
            pt.render(cornell_gpu, film, pt.default_params(frame=first + k, frame_count=1, pipeline=pipeline, **kw))
            acc += film.read_f32().astype(np.float64) * (first + k + 1)
            film.close()
        return acc / frames
    a1 = mean_of(32, 0, pt.PIPELINE_WAVEFRONT)
    a2 = mean_of(32, 32, pt.PIPELINE_WAVEFRONT)
    b = mean_of(32, 0, pt.PIPELINE_WAVEFRONT_NEE)
    ref = 0.5 * (a1 + a2)
    assert abs(b.mean() - ref.mean()) <= 0.01 * ref.mean()
    tiles = lambda x: x.reshape(h // 8, 8, w // 8, 8, 3).mean((1, 3))
    rel = lambda x, y: np.abs(x - y) / np.maximum(y, 0.05)
    assert rel(tiles(b), tiles(ref)).mean() <= 0.03
    assert rel(tiles(a1), tiles(a2)).mean() <= 0.03       # (the scale: the reference estimator against itself)


def _bvh4_facts(rows):
    """-> (leaf words, surface-area cost, nesting ok) of BVH4 rows [n, 32] (pt_scene_read_bvh4 layout)."""
    f = rows.view(np.float32)
    lo = np.stack([f[:, 0:4], f[:, 4:8], f[:, 8:12]], -1)        # [node, child, axis]
    hi = np.stack([f[:, 12:16], f[:, 16:20], f[:, 20:24]], -1)
    words = rows[:, 24:28]
    area = lambda l, h: 2.0 * ((h[0] - l[0]) * (h[1] - l[1]) + (h[1] - l[1]) * (h[2] - l[2]) + (h[2] - l[2]) * (h[0] - l[0]))
    root_lo, root_hi = lo[0][words[0] != 0xFFFFFFFF].min(0), hi[0][words[0] != 0xFFFFFFFF].max(0)
    leaves, cost, nested = [], 0.0, True
    stack = [(0, root_lo, root_hi)]
    while stack:
        nd, plo, phi = stack.pop()
        cost += 1.0 * area(plo, phi)                                # one node visit
        for c in range(4):
            w = int(words[nd, c])
            if w == 0xFFFFFFFF:
                continue
            nested &= bool((lo[nd, c] >= plo - 1e-6).all() and (hi[nd, c] <= phi + 1e-6).all())
            if w & 0x80000000:
                leaves.append(w)
                cost += 0.6 * (((w >> 28) & 7) + 1) * area(lo[nd, c], hi[nd, c])
            else:
                stack.append((w, lo[nd, c], hi[nd, c]))
    return leaves, cost / area(root_lo, root_hi), nested


@pytest.mark.parametrize("n,seed,pairs", [(0, 0, 1), (0, 0, 0), (7, 3, 1), (300, 4, 1), (300, 4, 0), (2048, 5, 1)])
def test_device_sah_builder_trees_are_sound_and_better_than_the_lbvh(pt, orc, gpu_ctx, cornell_arrays, n, seed, pairs):
    """The surface-area BVH4 of small scenes (bvh4_sah_device.hip, ePreferFastTrace): every triangle sits in exactly one
    leaf, child boxes nest, leaves follow the leaf rule (one primitive = a triangle or a fan pair; pair_leaves = 0: up to
    four triangles), its surface-area cost is not above the collapsed LBVH's, and it returns the oracle's hits -- Cornell
    box (n = 0), soups with fan pairs mixed in, the 2048-triangle limit."""
    if n == 0:
        v, i, f = cornell_arrays
    else:
        v, i, f = _soup(n, seed, spread=0.3)
        tri = v.reshape(-1, 3, 3).copy()
        for k in range(0, n - 1, 5):                 # every fifth triangle gets a fan partner (v0, v2, v3)
            tri[k + 1, 0], tri[k + 1, 1] = tri[k, 0], tri[k, 2]
        v = tri.reshape(-1)
    nt = len(i) // 3
    old = gpu_ctx.set_tuning(pair_leaves=pairs)
    try:
        sc = pt.Scene(gpu_ctx, v, i, f)
    finally:
        gpu_ctx.set_tuning(**old)
    assert sc.info().bvh4_builder == 1
    leaves, cost, nested = _bvh4_facts(sc.read_bvh4())
    assert nested
    covered = np.zeros(nt, np.int32)
    for w in leaves:
        first, cnt = w & 0x0FFFFFFF, ((w >> 28) & 7) + 1
        assert cnt <= (2 if pairs else 4)
        covered[first:first + cnt] += 1
    assert (covered == 1).all()
    rays = np.concatenate([np.random.default_rng(1).uniform(-1.2, 1.2, (5000, 3)), np.random.default_rng(2).normal(size=(5000, 3))], 1).astype(np.float32)
    want, _ = orc.Scene(v, i, f).trace(rays, mode=0)
    assert sc.trace(rays).tobytes() == want.tobytes()
    sc.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)
    _, cost_lbvh, nested_lbvh = _bvh4_facts(sc.read_bvh4())
    assert nested_lbvh
    if nt >= 36:      # (a handful of triangles: the collapsed LBVH's multi-triangle leaves can undercut one-primitive leaves)
        assert cost <= cost_lbvh * 1.0001, (cost, cost_lbvh)
    assert sc.trace(rays).tobytes() == want.tobytes()
    sc.close()


def test_stadium_scene_ploc_tree_is_sound_and_cheaper_to_walk_than_the_lbvh(pt, orc, gpu_ctx):
    """ePreferFastTrace (main.cpp:419) above 2048 triangles: the binary tree is rebuilt by PLOC before the wide nodes are
    collapsed from it.  On the "teapot in a stadium" scene (primitive sizes over four orders of magnitude; here its
    25 k-triangle version so that the oracle traces it in seconds): every triangle in exactly one leaf, nested boxes, the
    oracle's hit records under both qualities and both extend kernels, the LBVH read-back untouched, a lower surface-area
    cost and fewer node visits per ray than the Morton-median tree; and the switch back and forth rebuilds cleanly."""
    v, i, f = pt.make_stadium(96, 40)
    nt = len(i) // 3
    sc, osc = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    assert nt > 2048 and sc.info().bvh4_builder == 2
    rng = np.random.default_rng(11)
    org = np.tile(np.float32([0, -1, 5]), (30000, 1))                      # the camera's rays ...
    tgt = np.stack([rng.uniform(-1, 1, 30000), rng.uniform(-2, 0, 30000), np.full(30000, 2.0)], 1)
    rays = np.concatenate([np.concatenate([org, tgt - org], 1),          # ... and incoherent ones from inside the room
                           np.concatenate([rng.uniform(-0.9, 0.9, (30000, 3)) * [1, 1, 1] + [0, -1, 0], rng.normal(size=(30000, 3))], 1)]).astype(np.float32)
    want, _ = osc.trace(rays, mode=1)
    assert (want["prim"] != pt.MISS).mean() > 0.6
    keys, prim_of, nodes = sc.read_bvh()                                   # the LBVH read-back is the LBVH's, whatever is traversed
    okeys, oprim = osc.bvh_keys()
    assert keys.tobytes() == okeys.tobytes() and prim_of.tobytes() == oprim.tobytes() and nodes.tobytes() == osc.bvh_nodes().tobytes()
    assert sc.info().bvh_height == osc.bvh_info().height
    facts, films = {}, {}
    info_area = lambda s_: (round(s_.info().tree_area_lbvh, 2), round(s_.info().tree_area_ploc, 2))
    for quality, builder in ((pt.BVH_PREFER_FAST_TRACE, 2), (pt.BVH_PREFER_FAST_BUILD, 0), (pt.BVH_PREFER_FAST_TRACE, 2)):
        sc.set_bvh_quality(quality)
        assert sc.info().bvh4_builder == builder
        leaves, cost, nested = _bvh4_facts(sc.read_bvh4())
        covered = np.zeros(nt, np.int32)
        for w in leaves:
            covered[(w & 0x0FFFFFFF):(w & 0x0FFFFFFF) + ((w >> 28) & 7) + 1] += 1
        assert nested and (covered == 1).all()
        for variant in (pt.EXTEND_AUTO, pt.EXTEND_HBM):
            assert sc.trace(rays, extend=variant).tobytes() == want.tobytes(), (quality, variant)
        film = pt.Film(gpu_ctx, 160, 90)
        gpu_ctx.reset_stats()
        pt.render(sc, film, pt.default_params(width=160, height=90, spp_per_frame=4, max_depth=8, flags=pt.FLAG_COUNT_VISITS))
        st = gpu_ctx.stats()
        facts[builder] = (float(cost), st.nodes_visited / st.rays, info_area(sc))
        films[builder] = (st.rays, film.read_f32().tobytes())
        film.close()
    assert films[2] == films[0]                                            # same rays, same film, bit for bit
    assert facts[2][0] < facts[0][0], facts                                # surface-area cost of the BVH4
    assert facts[2][1] < 0.95 * facts[0][1], facts                         # BVH4 node visits per ray of a render
    sc.close()


def test_pt_tune_environment_variable_is_parsed_once_at_context_creation(pt):
    """PT_TUNE="name=value,..." is the library's only tuning input from the environment, read by pt_ctx_create; a name it
    does not know is an error there (never silently ignored), and nothing is read afterwards."""
    os.environ["PT_TUNE"] = "node_yield=3, pipes=1;refill=24"
    try:
        ctx = pt.Context(0)
        os.environ["PT_TUNE"] = "pipes=2"              # too late: the context keeps what it was created with
        t = ctx.tuning()
        assert (t.node_yield, t.pipes, t.refill, t.lds_stack) == (3, 1, 24, -1)
        ctx.close()
        os.environ["PT_TUNE"] = "no_such_knob=1"
        with pytest.raises(pt.PtError) as e:
            pt.Context(0)
        assert e.value.status == 1 and "no_such_knob" in str(e.value)
        # fail_rebuild is failure injection for the tests, not a knob: a stray PT_TUNE must not be able to break a production rebuild
        os.environ["PT_TUNE"] = "fail_rebuild=1"
        with pytest.raises(pt.PtError) as e:
            pt.Context(0)
        assert e.value.status == 1 and "fail_rebuild" in str(e.value)
    finally:
        os.environ.pop("PT_TUNE", None)


def test_device_write_read_round_trip(pt, gpu_ctx):
    """pt_device_write / pt_device_read (API version 5): the host <-> device copies a host that does not link HIP uses (pt_main --selftest)."""
    import ctypes as C
    a = np.arange(1000, dtype=np.float32) * np.float32(0.5)
    buf = pt.DeviceBuffer(gpu_ctx, a.nbytes)
    gpu_ctx._check(pt.lib_amd().pt_device_write(gpu_ctx.h, C.c_void_p(buf.ptr), a.ctypes.data, a.nbytes))
    assert buf.read(np.float32, a.shape).tobytes() == a.tobytes()
    buf.close()


def test_presenter_falls_back_to_the_process_group_when_the_library_communicator_fails(tmp_path):
    """bench.py's Presenter: when the library's own RCCL communicator cannot be created on any rank, all ranks gather the
    packed tiles through torch.distributed's RCCL process group instead (same pack / unpack kernels) and say so.  One rank
    is all a 1-GPU box can run: the forced fallback presents an image equal to the film, bit for bit."""
    import subprocess
    import sys
    import textwrap
    repo = os.path.dirname(HERE)
    script = tmp_path / "fallback.py"
    script.write_text(textwrap.dedent(f"""
        import importlib, os, sys
        sys.path.insert(0, {repo!r})
        import torch, torch.distributed as dist
        os.environ["PT_PRESENT_FORCE_TORCH"] = "1"
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29577", rank=0, world_size=1)
        pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
        ptd = importlib.import_module("single-file-vulkan-pathtracing_amd.distributed")
        ctx = pt.Context(0)
        arrays = pt.load_obj(os.path.join({repo!r}, "assets", "CornellBox-Original.obj"))
        scene = pt.Scene(ctx, *arrays)
        w, h = 250, 131
        t = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        film = pt.Film(ctx, w, h)
        pt.render(scene, film, pt.default_params(width=w, height=h, spp_per_frame=4, max_depth=8, frame=0, frame_count=2))
        p = ptd.Presenter(pt, ctx, film, t, 0, 1, "cuda:0", False)
        assert p.comm is None and "torch.distributed" in p.describe() and p.ranks_seen == 1, p.describe()
        img = p.present()
        assert img.cpu().numpy().tobytes() == film.read_f32().tobytes()
        p.close(); film.close(); scene.close(); ctx.close()
        dist.destroy_process_group()
        print("FALLBACK_OK")
    """))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FALLBACK_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("config", ["c2", "c4", "c5"])
def test_full_size_frames_equal_the_oracle_known_answers(pt, gpu_ctx, config):
    """BASELINE's configurations at their FULL size (1920x1080; C2 / C4: 32 spp, depth 8; C5: the 1 M-triangle soup, 16 spp,
    depth 16): frame 0 on the GPU has exactly the oracle's ray count and its film is the oracle's bit for bit (SHA-256 of
    6.2 M floats, tests/golden/fullsize_hashes.json, written by tests/golden/make_fullsize_hashes.py from an oracle run).
    The same frame through other shapes of the pipeline (one slot lane and one sample group, eight sample groups, the
    kernels that read the scene from HBM, rays sorted per round) is the same film: size-independent invariances at the
    size the benchmark runs."""
    import hashlib
    import json
    path = os.path.join(HERE, "golden", "fullsize_hashes.json")
    gold = json.load(open(path)).get(config)
    if gold is None:
        pytest.skip(f"no known answer for {config} in {path}")
    repo = os.path.dirname(HERE)
    if config == "c5":
        arrays = pt.make_soup(1000000, 1)
    else:
        arrays = pt.load_obj(os.path.join(repo, "assets", "CornellBox-Original.obj"))
    scene = pt.Scene(gpu_ctx, *arrays)
    if config == "c4":
        scene.set_instances(pt.cornell_grid_instances())
    w, h = gold["width"], gold["height"]
    film = pt.Film(gpu_ctx, w, h)
    base = dict(width=w, height=h, spp_per_frame=gold["spp_per_frame"], max_depth=gold["max_depth"], frame=0, frame_count=1)
    variants = [dict(), dict(frames_in_flight=1, sample_groups=1), dict(frames_in_flight=1, sample_groups=8)]
    if config == "c2":
        variants += [dict(extend=pt.EXTEND_HBM), dict(extend=pt.EXTEND_HBM8)]
    if config == "c4":   # the fused pipeline's two-level kernel (k_fused_inst), one accumulator per slot and the term logs
        variants += [dict(pipeline=pt.PIPELINE_FUSED, frames_in_flight=1, sample_groups=1), dict(pipeline=pt.PIPELINE_FUSED)]
    if config == "c5":
        variants += [dict(flags=pt.FLAG_SORT_RAYS), dict(extend=pt.EXTEND_HBM8)]
    # what a caller gets from pt_params_default (PT_PIPELINE_AUTO): the fused kernels for C2 and -- under the library's 8 GB workspace budget -- for the
    # two-level scene, the wavefront queues for the soup
    variants += [dict(pipeline=pt.PIPELINE_AUTO)]
    for kw in variants:
        film.clear()
        gpu_ctx.reset_stats()
        pt.render(scene, film, pt.default_params(**base, **kw))
        if kw.get("pipeline") == pt.PIPELINE_AUTO:
            assert gpu_ctx.stats().pipeline == (pt.PIPELINE_WAVEFRONT if config == "c5" else pt.PIPELINE_FUSED), config
        assert gpu_ctx.stats().rays == gold["rays"], (config, kw)
        got = film.read_f32()
        assert got.shape == (h, w, 3)
        assert hashlib.sha256(got.astype("<f4").tobytes()).hexdigest() == gold["film_sha256"], (config, kw, float(got.astype(np.float64).sum()), gold["film_sum_f64"])
    film.close()
    scene.close()


def _c3_gold():
    import json
    path = os.path.join(HERE, "golden", "fullsize_hashes.json")
    gold = json.load(open(path)).get("c3")
    if gold is None:
        pytest.skip(f"no known answer for c3 in {path}")
    return gold


@pytest.mark.parametrize("pipeline", ["wavefront", "auto"])
def test_c3_full_size_1024spp_progressive_equals_the_oracle_known_answer(pt, gpu_ctx, cornell_gpu, pipeline):
    """BASELINE config C3 at its size on ONE device: the Cornell box at 1920x1080, 1024 spp = frames 0..31 of 32 spp (seed
    multipliers m = 1 .. 1024, raygen.rgen:47), depth 8, blended progressively (raygen.rgen:88-90).  The oracle's known
    answer (tests/golden/fullsize_hashes.json `c3`, tests/golden/make_fullsize_hashes.py) holds the SHA-256 of the float film
    and of the reference's rgba8 storage image after frames 0, 1, 3, 7, 15 and 31 and the exact ray count of every frame:
    the GPU renders the 32 frames in six calls that end on those frames (1 + 1 + 2 + 4 + 8 + 16 frames in flight) and has
    to meet every one of them to the bit -- 7.2 G rays, 6.2 M floats."""
    import hashlib
    gold = _c3_gold()
    w, h = gold["width"], gold["height"]
    # (`auto` = PT_PIPELINE_AUTO, what pt_params_default gives a caller: the fused kernel for this scene)
    kw = dict(width=w, height=h, spp_per_frame=gold["spp_per_frame"], max_depth=gold["max_depth"],
              pipeline=pt.PIPELINE_AUTO if pipeline == "auto" else pt.PIPELINE_WAVEFRONT)
    film = pt.Film(gpu_ctx, w, h)
    gpu_ctx.reset_stats()
    first = 0
    for mark in sorted(int(k) for k in gold["after_frame"]):
        pt.render(cornell_gpu, film, pt.default_params(frame=first, frame_count=mark + 1 - first, **kw))
        first = mark + 1
        g = gold["after_frame"][str(mark)]
        assert gpu_ctx.stats().rays == g["rays_so_far"] == sum(gold["rays_per_frame"][:mark + 1]), mark
        assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == g["film_sha256"], mark
        assert hashlib.sha256(film.read_bgra8().tobytes()).hexdigest() == g["bgra8_sha256"], mark
    assert first == gold["frames"] and gpu_ctx.stats().rays == gold["rays"]
    # and the whole job as ONE call (what bench.py --config c3 times): AUTO batches the 32 frames itself
    film.clear()
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=gold["frames"], **kw))
    last = gold["after_frame"][str(gold["frames"] - 1)]
    assert gpu_ctx.stats().rays == gold["rays"]
    assert gpu_ctx.stats().pipeline == (pt.PIPELINE_FUSED if pipeline == "auto" else pt.PIPELINE_WAVEFRONT)
    assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == last["film_sha256"]
    assert hashlib.sha256(film.read_bgra8().tobytes()).hexdigest() == last["bgra8_sha256"]
    film.close()


@pytest.mark.parametrize("pipeline", ["wavefront", "auto"])
def test_c3_full_size_as_eight_ranks_in_sequence_assembles_the_same_image(pt, gpu_ctx, cornell_gpu, pipeline):
    """BASELINE config C3 as the 8-GPU job it is, on the one GPU there is: ranks 0..7 of world 8 render their 8x8 tiles of
    the 1920x1080 x 1024-spp image one after the other (32 frames each, one call), pt_film_pack_tiles / _unpack_tiles --
    the two kernels of pt_film_present either side of the RCCL gather -- assemble one image: the oracle's film to the bit
    (same SHA-256 as the single-device render), every rank traces exactly the number of rays the oracle counted for its
    pixels, the counts add up to the job's 7.2 G rays and no rank is more than 1 % away from an eighth of them; each
    rank's rgba8 tiles are the oracle's too (the gather moves the float film only)."""
    import hashlib
    import importlib
    d = importlib.import_module("single-file-vulkan-pathtracing_amd.distributed")
    gold = _c3_gold()
    w, h, world = gold["width"], gold["height"], gold["world"]
    kw = dict(width=w, height=h, spp_per_frame=gold["spp_per_frame"], max_depth=gold["max_depth"], frame=0, frame_count=gold["frames"],
              pipeline=pt.PIPELINE_AUTO if pipeline == "auto" else pt.PIPELINE_WAVEFRONT)
    last = gold["after_frame"][str(gold["frames"] - 1)]
    image = pt.DeviceBuffer(gpu_ctx, w * h * 12)
    bgra = np.zeros((h, w, 4), np.uint8)
    rays, tiles = [], 0
    for rank in range(world):
        film = pt.Film(gpu_ctx, w, h)
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.default_params(rank=rank, world=world, **kw))
        rays.append(gpu_ctx.stats().rays)
        n = pt.film_tile_count(film, rank, world)
        tiles += n
        packed = pt.DeviceBuffer(gpu_ctx, n * 192 * 4)
        pt.film_pack_tiles(film, rank, world, packed.ptr)
        pt.film_unpack_tiles(film, rank, world, packed.ptr, image.ptr)
        mask = d.owned_mask(w, h, rank, world)
        part = film.read_bgra8()
        bgra[mask] = part[mask]
        packed.close(); film.close()
    assert tiles == ((w + 7) // 8) * ((h + 7) // 8)
    assert rays == gold["rays_per_rank_world8"], (rays, gold["rays_per_rank_world8"])
    assert sum(rays) == gold["rays"]
    assert max(abs(r - gold["rays"] / world) for r in rays) <= 0.01 * gold["rays"] / world, rays
    got = image.read(np.float32, (h, w, 3))
    assert hashlib.sha256(got.astype("<f4").tobytes()).hexdigest() == last["film_sha256"]
    assert hashlib.sha256(bgra.tobytes()).hexdigest() == last["bgra8_sha256"]
    image.close()


# ---- PT_PIPELINE_AUTO: what pt_params_default returns (API version 5) --------------------------------------------------
def test_auto_pipeline_picks_fused_where_it_applies_and_wavefront_elsewhere(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle):
    """pt_params_default names PT_PIPELINE_AUTO: the fused kernel for scenes that live in LDS when the call is one it can serve, the
    wavefront queues otherwise -- never an error where one of the two can render, pt_stats.pipeline says which ran (also after
    pt_render_prepare), and the bits do not depend on the choice: every case below is the oracle's film, rgba8 image and ray count."""
    w, h = 96, 56
    kw = dict(width=w, height=h, spp_per_frame=8, max_depth=8)
    p = pt.library_default_params(**kw)
    assert p.pipeline == pt.PIPELINE_AUTO == 3
    ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, 2, **kw)
    film = pt.Film(gpu_ctx, w, h)
    cases = [(dict(), pt.PIPELINE_FUSED), (dict(frames_in_flight=1, sample_groups=4), pt.PIPELINE_FUSED),
             (dict(flags=pt.FLAG_COUNT_VISITS), pt.PIPELINE_WAVEFRONT),            # no instrumented fused kernel
             (dict(flags=pt.FLAG_ASYNC), pt.PIPELINE_WAVEFRONT),                   # the fused pipeline is blocking
             (dict(extend=pt.EXTEND_HBM), pt.PIPELINE_WAVEFRONT),                  # a named closest-hit kernel is a wavefront kernel
             (dict(rank=1, world=3), pt.PIPELINE_FUSED)]
    for extra, want in cases:
        film.clear()
        gpu_ctx.reset_stats()
        q = pt.library_default_params(frame=0, frame_count=2, **kw, **extra)
        pt.render_prepare(cornell_gpu, film, q)
        assert gpu_ctx.stats().pipeline == want, extra
        pt.render(cornell_gpu, film, q)
        gpu_ctx.sync()
        st = gpu_ctx.stats()
        assert st.pipeline == want, extra
        if "world" not in extra:
            assert st.rays == orays, extra
            assert film.read_f32().tobytes() == ofilm.tobytes() and film.read_bgra8().tobytes() == obgra.tobytes(), extra
    # tmin <= 0 is not the fused kernel's: AUTO renders it through the queues (the explicit request is refused, tested below)
    kz = dict(kw, tmin=0.0)
    oz, _, rz = _render_oracle(orc, cornell_oracle, 1, **kz)
    film.clear()
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.library_default_params(frame=0, frame_count=1, **kz))
    assert gpu_ctx.stats().pipeline == pt.PIPELINE_WAVEFRONT and gpu_ctx.stats().rays == rz and film.read_f32().tobytes() == oz.tobytes()
    # a scene beyond LDS: the wavefront pipeline; an instanced scene of the compact two-level kernel's class: k_fused_inst
    v, i, f = _soup(3000, 5)
    big, obig = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    ob, _, rb = _render_oracle(orc, obig, 1, **kw)
    film.clear()
    gpu_ctx.reset_stats()
    pt.render(big, film, pt.library_default_params(frame=0, frame_count=1, **kw))
    assert gpu_ctx.stats().pipeline == pt.PIPELINE_WAVEFRONT and gpu_ctx.stats().rays == rb and film.read_f32().tobytes() == ob.tobytes()
    big.close()
    inst = pt.Scene(gpu_ctx, *pt.load_obj(pt.ASSET_CORNELL))
    xf = pt.cornell_grid_instances()[:16]
    inst.set_instances(xf)
    oi = orc.Scene(*pt.load_obj(pt.ASSET_CORNELL))
    oi.set_instances(xf)
    of_, _, ri = _render_oracle(orc, oi, 1, **kw)
    # (two-level scenes: k_fused_inst at every frame count under the library's own 8 GB workspace budget; the queues -- 15 % faster for one frame per
    # launch, in 13 GB where the fused kernel takes 5 -- only once the caller has raised the budget to what they take, >= 16 GB or none)
    for budget, want1 in ((-1, pt.PIPELINE_FUSED), (8192, pt.PIPELINE_FUSED), (16384, pt.PIPELINE_WAVEFRONT), (0, pt.PIPELINE_WAVEFRONT)):
        old = gpu_ctx.set_tuning(mem_budget_mb=budget)
        try:
            film.clear()
            gpu_ctx.reset_stats()
            pt.render(inst, film, pt.library_default_params(frame=0, frame_count=1, **kw))
            assert gpu_ctx.stats().pipeline == want1 and gpu_ctx.stats().rays == ri and film.read_f32().tobytes() == of_.tobytes(), budget
        finally:
            gpu_ctx.set_tuning(**old)
    of9, _, r9 = _render_oracle(orc, oi, 9, **kw)
    film.clear()
    gpu_ctx.reset_stats()
    pt.render(inst, film, pt.library_default_params(frame=0, frame_count=9, **kw))
    assert gpu_ctx.stats().pipeline == pt.PIPELINE_FUSED and gpu_ctx.stats().rays == r9 and film.read_f32().tobytes() == of9.tobytes()
    film.clear()
    pt.render(inst, film, pt.library_default_params(frame=0, frame_count=9, frames_in_flight=3, **kw))
    assert gpu_ctx.stats().pipeline == pt.PIPELINE_FUSED and film.read_f32().tobytes() == of9.tobytes()
    inst.set_instances(xf[:1])      # one instance: the general two-level kernel, wavefront only
    film.clear()
    pt.render(inst, film, pt.library_default_params(frame=0, frame_count=1, **kw))
    assert gpu_ctx.stats().pipeline == pt.PIPELINE_WAVEFRONT
    inst.close()
    film.close()


# ---- PT_PIPELINE_FUSED: the whole loop as one persistent kernel (csrc/fused_kernel.h) ----------------------------------
def test_fused_pipeline_bit_exact_vs_oracle_and_wavefront(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle):
    """The fused kernel (one lane owns its path like a raygen.rgen:41-91 invocation; traversal + closesthit.rchit:50-65 +
    miss.rmiss:8-12 + the bounce in the same lane, path state in LDS, no queues) renders the oracle's film, rgba8 image and ray
    count bit for bit: progressive frames one call each and batched, every sample-group shape (plain accumulator, term logs),
    a ragged image with partial 8x8 tiles, the reference's 32 spp."""
    for (w, h, spp, depth, frames) in ((64, 64, 4, 8, 3), (100, 37, 8, 5, 2), (120, 68, 32, 8, 2), (1, 1, 2, 3, 1)):
        kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=depth)
        ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, frames, **kw)
        shapes = [dict(), dict(frames_in_flight=1, sample_groups=1), dict(frames_in_flight=frames, sample_groups=1),
                  dict(sample_groups=2), dict(frames_in_flight=1, sample_groups=spp)]
        for shape in shapes:
            film = pt.Film(gpu_ctx, w, h)
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=frames, pipeline=pt.PIPELINE_FUSED, **kw, **shape))
            st = gpu_ctx.stats()
            assert st.rays == orays, (w, h, shape, st.rays, orays)
            assert film.read_f32().tobytes() == ofilm.tobytes(), (w, h, shape)
            assert film.read_bgra8().tobytes() == obgra.tobytes(), (w, h, shape)
            assert st.paths == w * h * spp * frames
            film.close()
        # one blocking call per frame, as main.cpp:647-685 dispatches
        film = pt.Film(gpu_ctx, w, h)
        for k in range(frames):
            pt.render(cornell_gpu, film, pt.default_params(frame=k, frame_count=1, pipeline=pt.PIPELINE_FUSED, **kw))
        assert film.read_f32().tobytes() == ofilm.tobytes() and film.read_bgra8().tobytes() == obgra.tobytes()
        film.close()


def test_fused_head_and_tail_slots_bit_exact(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, cornell_arrays):
    """k_fused's HEAD + TAIL shape (fused_kernel.h MODE 2; pt_tuning.fused_tail = S, or the library's own rule on launches with few slots
    per lane): a pixel's frame is one head slot of spp - S samples summed in LDS and S one-sample tail slots whose radiance terms go through the
    log and are replayed after the head's sum in sample order.  Film, rgba8 image and ray count equal the oracle's for every S (1, a middle
    one, spp - 1, beyond spp), ragged images, several frames in flight and batches of frames, shards, the log's three tiers and the redo of
    an overflowed launch, and on trees without pair leaves; explicit sample_groups never take the shape; pt_stats.tail_samples reports it."""
    import importlib
    d = importlib.import_module("single-file-vulkan-pathtracing_amd.distributed")
    for (w, h, spp, depth, frames) in ((64, 64, 4, 8, 3), (100, 37, 8, 5, 2), (120, 68, 32, 8, 2), (1, 1, 2, 3, 1), (33, 9, 5, 13, 4)):
        kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=depth)
        ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, frames, **kw)
        for S in sorted({1, spp // 2, spp - 1, spp + 7}):
            for shape in (dict(), dict(frames_in_flight=1), dict(frames_in_flight=frames)):
                old = gpu_ctx.set_tuning(fused_tail=S)
                try:
                    film = pt.Film(gpu_ctx, w, h)
                    gpu_ctx.reset_stats()
                    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=frames, pipeline=pt.PIPELINE_FUSED, **kw, **shape))
                    st = gpu_ctx.stats()
                    assert st.tail_samples == min(S, spp - 1) and st.sample_groups == 1, (S, st.tail_samples)
                    assert st.rays == orays, (w, h, S, shape, st.rays, orays)
                    assert film.read_f32().tobytes() == ofilm.tobytes(), (w, h, S, shape)
                    assert film.read_bgra8().tobytes() == obgra.tobytes(), (w, h, S, shape)
                    film.close()
                finally:
                    gpu_ctx.set_tuning(**old)
    w, h, spp, frames = 200, 120, 8, 2
    kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=8)
    ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, frames, **kw)
    # explicit groups are taken as given; fused_tail = 0 is the plain shape
    for knobs, shape, tail in ((dict(fused_tail=3), dict(sample_groups=2), 0), (dict(fused_tail=3), dict(sample_groups=1), 0), (dict(fused_tail=0), dict(), 0),
                               (dict(fused_tail=3), dict(pipeline=pt.PIPELINE_AUTO), 3)):
        old = gpu_ctx.set_tuning(**knobs)
        try:
            film = pt.Film(gpu_ctx, w, h)
            pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=frames, **{**dict(pipeline=pt.PIPELINE_FUSED), **kw, **shape}))
            assert gpu_ctx.stats().tail_samples == tail and film.read_f32().tobytes() == ofilm.tobytes(), (knobs, shape)
            film.close()
        finally:
            gpu_ctx.set_tuning(**old)
    # the log's tiers (primary only + pool, a pool of three entries: the launch is done again with the plain shape) and the shade block's fill
    for knobs in (dict(term_ocap=0, term_spill=1 << 20), dict(term_ocap=1, term_spill=1 << 20), dict(term_ocap=0, term_spill=3), dict(refill=1), dict(refill=64)):
        old = gpu_ctx.set_tuning(fused_tail=5, **knobs)
        try:
            film = pt.Film(gpu_ctx, w, h)
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=frames, pipeline=pt.PIPELINE_FUSED, **kw))
            st = gpu_ctx.stats()
            assert film.read_f32().tobytes() == ofilm.tobytes() and st.rays == orays and st.tail_samples == 5, knobs
            film.close()
        finally:
            gpu_ctx.set_tuning(**old)
    # every surface emits, so a tail slot's one sample logs a term per ray: past the three primary entries into the overflow log and the pool,
    # and with a pool of three entries the launch is done again with the plain shape (redone_batches)
    v, i, f = cornell_arrays
    f = f.reshape(-1, 6).copy()
    f[:, 3:] = np.float32(0.25) + f[:, :3] * np.float32(0.5)
    gs, osc = pt.Scene(gpu_ctx, v, i, f.reshape(-1)), orc.Scene(v, i, f.reshape(-1))
    ke = dict(width=64, height=40, spp_per_frame=6, max_depth=12)
    of3, ob3, or3 = _render_oracle(orc, osc, 3, **ke)
    for knobs in (dict(), dict(term_ocap=0, term_spill=1 << 20), dict(term_ocap=2, term_spill=1 << 20), dict(term_ocap=0, term_spill=3), dict(term_ocap=1, term_spill=0)):
        old = gpu_ctx.set_tuning(fused_tail=4, **knobs)
        try:
            film = pt.Film(gpu_ctx, 64, 40)
            gpu_ctx.reset_stats()
            pt.render(gs, film, pt.default_params(frame=0, frame_count=3, frames_in_flight=2, pipeline=pt.PIPELINE_FUSED, **ke))
            st = gpu_ctx.stats()
            assert film.read_f32().tobytes() == of3.tobytes() and film.read_bgra8().tobytes() == ob3.tobytes() and st.rays == or3, knobs
            if knobs.get("term_spill") in (0, 3):
                assert st.redone_batches >= 1, knobs
            film.close()
        finally:
            gpu_ctx.set_tuning(**old)
    gs.close()
    # shards add up; a rank's film is zero outside its tiles
    old = gpu_ctx.set_tuning(fused_tail=4)
    try:
        for world in (3, 8):
            acc, rays = np.zeros_like(ofilm), 0
            for rank in range(world):
                film = pt.Film(gpu_ctx, w, h)
                gpu_ctx.reset_stats()
                pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=frames, rank=rank, world=world, pipeline=pt.PIPELINE_FUSED, **kw))
                rays += gpu_ctx.stats().rays
                part = film.read_f32()
                assert (part[~d.owned_mask(w, h, rank, world)] == 0).all()
                acc += part
                film.close()
            assert acc.tobytes() == ofilm.tobytes() and rays == orays
        # progressive: frames 0..1 then 2..4 onto the same film, against five oracle frames
        o5, b5, r5 = _render_oracle(orc, cornell_oracle, 5, **kw)
        film = pt.Film(gpu_ctx, w, h)
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_FUSED, **kw))
        pt.render(cornell_gpu, film, pt.default_params(frame=2, frame_count=3, frames_in_flight=2, pipeline=pt.PIPELINE_FUSED, **kw))
        assert film.read_f32().tobytes() == o5.tobytes() and film.read_bgra8().tobytes() == b5.tobytes() and gpu_ctx.stats().rays == r5
        film.close()
    finally:
        gpu_ctx.set_tuning(**old)
    # the kernel's other instantiation (leaves of independent triangles)
    for arrays, pair in ((cornell_arrays, 0), (_soup(100, 5, spread=0.3), 1)):
        old = gpu_ctx.set_tuning(pair_leaves=pair)
        try:
            gs = pt.Scene(gpu_ctx, *arrays)
        finally:
            gpu_ctx.set_tuning(**old)
        osc = orc.Scene(*arrays)
        k2 = dict(width=90, height=50, spp_per_frame=6, max_depth=7)
        of2, ob2, or2 = _render_oracle(orc, osc, 2, **k2)
        old = gpu_ctx.set_tuning(fused_tail=2)
        try:
            film = pt.Film(gpu_ctx, 90, 50)
            gpu_ctx.reset_stats()
            pt.render(gs, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_FUSED, **k2))
            assert gpu_ctx.stats().rays == or2 and film.read_f32().tobytes() == of2.tobytes() and gpu_ctx.stats().tail_samples == 2, pair
            assert film.read_bgra8().tobytes() == ob2.tobytes()
            film.close()
        finally:
            gpu_ctx.set_tuning(**old)
        gs.close()


def test_fused_subject_first_order_changes_no_bit(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle):
    """The fused pipeline hands out first the tiles the scene's box projects to (render.hip fused_subject_rect, film_work.hip
    ptw_tiles_subject_first; pt_tuning.fused_subject = 0: centre first only).  Order only: for views with the box pushed to a side or a corner,
    far away, off the image, and with the camera inside or behind the box (no rectangle), the film, the rgba8 image and the ray count are the
    oracle's with and without it, for the plain, the all-groups and the head + tail shape, and when the view changes between calls on one film.
    The same rectangle is a proof: a pixel outside it (by a pixel of slack) cannot see the scene, and the kernel finishes its slots where it hands
    them out -- every sample one counted ray whose miss adds the environment (pt_tuning.cull, pt_stats.rays_culled).  Same bits, same rays."""
    w, h, spp = 136, 72, 4
    views = [dict(), dict(cam_origin=(1.1, -1.0, 5.0), cam_target=(1.1, -1.0, 2.0)), dict(cam_origin=(1.0, -0.2, 5.0), cam_target=(1.0, -0.2, 2.0)),
             dict(cam_origin=(0.0, -1.0, 9.0), cam_target=(0.0, -1.0, 6.0)), dict(cam_origin=(3.5, -1.0, 5.0), cam_target=(3.5, -1.0, 2.0)),
             dict(cam_origin=(0.0, -1.0, 0.5), cam_target=(0.0, -1.0, -2.5)), dict(cam_origin=(0.0, -1.0, -5.0), cam_target=(0.0, -1.0, -8.0)),
             dict(cam_origin=(0.0, -1.0, 5.0), cam_target=(0.0, -1.0, 8.0))]
    film = pt.Film(gpu_ctx, w, h)        # one film for every view: the tile table is re-ordered when the rectangle changes
    n_culled = []
    for cam in views:
        kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=6, **cam)
        ofilm, obgra, orays = _render_oracle(orc, cornell_oracle, 2, **kw)
        culled = set()
        for subject, cull in ((1, 1), (0, 1), (-1, -1), (1, 0), (0, 0)):
            for knobs, shape in ((dict(fused_tail=0), dict(sample_groups=1)), (dict(fused_tail=0), dict(sample_groups=spp)), (dict(fused_tail=0), dict(sample_groups=3)),
                                 (dict(fused_tail=2), dict())):
                old = gpu_ctx.set_tuning(fused_subject=subject, cull=cull, **knobs)
                try:
                    film.clear()
                    gpu_ctx.reset_stats()
                    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_FUSED, **kw, **shape))
                    st = gpu_ctx.stats()
                    assert st.rays == orays, (cam, subject, cull, shape)
                    assert film.read_f32().tobytes() == ofilm.tobytes() and film.read_bgra8().tobytes() == obgra.tobytes(), (cam, subject, cull, shape)
                    # pt_stats.rays_culled: camera rays finished without a walk -- whole pixels' worth, the same for every shape, none with the knob off
                    assert st.rays_culled % (2 * spp) == 0 and st.rays_culled <= w * h * spp * 2 and (cull != 0 or st.rays_culled == 0)
                    if cull != 0:
                        culled.add(st.rays_culled)
                finally:
                    gpu_ctx.set_tuning(**old)
        assert len(culled) == 1, (cam, culled)
        n_culled.append(culled.pop())
    film.close()
    # the reference's view leaves a quarter of this small image's pixels outside the box's projection; the far box most of them; a camera inside
    # the box, behind it or looking away has no rectangle to cull by
    assert 0 < n_culled[0] < n_culled[3] and n_culled[5] == n_culled[6] == n_culled[7] == 0, n_culled


def test_fused_cull_on_two_level_scenes(pt, orc, gpu_ctx, cornell_arrays):
    """The cull rectangle of a two-level scene is the projection of the union of its instances' world boxes (k_fused_inst, fused_cull.h): a patch of
    config C4's grid and a few rotated + scaled instances, seen so that they cover part of the image -- the oracle's film, rgba8 image and ray
    count with the cull and without, one group and several, several frames in flight, a shard; pixels are culled, and none with the knob off."""
    import importlib
    d = importlib.import_module("single-file-vulkan-pathtracing_amd.distributed")
    grid = pt.cornell_grid_instances().reshape(100, 100, 3, 4)[40:52, 40:52].reshape(-1, 3, 4)
    few = _random_instances(7, 21)
    few[:, :, :3] *= np.float32(0.4)
    for inst, cam in ((grid, dict(cam_origin=(-0.08, -1.08, 0.9), cam_target=(-0.08, -1.08, -2.1))), (few, dict(cam_origin=(0.0, -1.0, 9.0), cam_target=(0.0, -1.0, 6.0)))):
        gs, osc = pt.Scene(gpu_ctx, *cornell_arrays), orc.Scene(*cornell_arrays)
        gs.set_instances(inst)
        osc.set_instances(inst)
        w, h, spp, frames = 120, 72, 6, 3
        kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=7, **cam)
        ofilm, obgra, orays = _render_oracle(orc, osc, frames, **kw)
        assert (ofilm > 0).any()
        seen = set()
        for cull in (1, 0):
            for shape in (dict(), dict(sample_groups=1), dict(sample_groups=4), dict(sample_groups=spp, frames_in_flight=2)):
                old = gpu_ctx.set_tuning(cull=cull)
                try:
                    film = pt.Film(gpu_ctx, w, h)
                    gpu_ctx.reset_stats()
                    pt.render(gs, film, pt.default_params(frame=0, frame_count=frames, pipeline=pt.PIPELINE_FUSED, **kw, **shape))
                    st = gpu_ctx.stats()
                    assert st.rays == orays and film.read_f32().tobytes() == ofilm.tobytes() and film.read_bgra8().tobytes() == obgra.tobytes(), (len(inst), cull, shape)
                    assert (st.rays_culled > 0) == (cull == 1) and st.rays_culled % (spp * frames) == 0, (len(inst), cull, st.rays_culled)
                    if cull:
                        seen.add(st.rays_culled)
                    film.close()
                finally:
                    gpu_ctx.set_tuning(**old)
        assert len(seen) == 1
        acc, rays = np.zeros_like(ofilm), 0
        for rank in range(3):
            film = pt.Film(gpu_ctx, w, h)
            gpu_ctx.reset_stats()
            pt.render(gs, film, pt.default_params(frame=0, frame_count=frames, rank=rank, world=3, pipeline=pt.PIPELINE_AUTO, **kw))
            rays += gpu_ctx.stats().rays
            acc += film.read_f32()
            film.close()
        assert acc.tobytes() == ofilm.tobytes() and rays == orays
        gs.close()


def test_fused_tail_rule_at_full_size_against_the_known_answers(pt, gpu_ctx, cornell_gpu):
    """The library's own head + tail rule (render.hip fused_tail_samples: by head slots per lane of the grid) at 1920x1080, 32 spp: one frame
    per call takes spp / 2 tail samples, two frames 5 spp / 16, four frames 3 spp / 16 -- and each call's film is the oracle's known answer
    (tests/golden/fullsize_hashes.json: C2's frame 0, C3 after frames 1 and 3) whatever the shape."""
    import hashlib
    import json
    gold = json.load(open(os.path.join(HERE, "golden", "fullsize_hashes.json")))
    g2, g3 = gold["c2"], gold.get("c3")
    w, h, spp = g2["width"], g2["height"], g2["spp_per_frame"]
    kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=g2["max_depth"])
    film = pt.Film(gpu_ctx, w, h)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.library_default_params(frame=0, frame_count=1, **kw))
    st = gpu_ctx.stats()
    assert st.pipeline == pt.PIPELINE_FUSED and st.tail_samples == spp // 2 and st.rays == g2["rays"]
    assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == g2["film_sha256"]
    # 44 % of the reference's image lies outside the box's projection (raygen.rgen:52-53 has no aspect correction): 901 676 pixels' camera rays
    assert st.rays_culled == 901676 * spp
    if g3 is not None and "1" in g3["after_frame"]:
        film.clear()
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.library_default_params(frame=0, frame_count=2, **kw))
        st, m = gpu_ctx.stats(), g3["after_frame"]["1"]
        assert st.tail_samples == spp * 5 // 16 and st.frames_in_flight == 2 and st.rays == m["rays_so_far"]
        assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == m["film_sha256"]
    if g3 is not None:
        film.clear()
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.library_default_params(frame=0, frame_count=4, **kw))
        st, m = gpu_ctx.stats(), g3["after_frame"]["3"]
        # (12.2 walked slots per lane: round 6's rule leaves the plain shape above 10.1 -- the faster kernel's launches end sooner; round 5 took 3 spp / 16 here)
        assert st.tail_samples == 0 and st.rays == m["rays_so_far"] and st.rays_culled == 4 * 901676 * spp
        assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == m["film_sha256"]
        old = gpu_ctx.set_tuning(fused_tail=spp * 3 // 16)      # ... and the head + tail shape of that size, asked for: the same film
        try:
            film.clear()
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.library_default_params(frame=0, frame_count=4, **kw))
            assert gpu_ctx.stats().tail_samples == spp * 3 // 16 and gpu_ctx.stats().rays == m["rays_so_far"]
            assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == m["film_sha256"]
        finally:
            gpu_ctx.set_tuning(**old)
        # a rank of world 8 with 16 frames in flight holds as many slots as two whole frames: the same rule
        film.clear()
        pt.render(cornell_gpu, film, pt.library_default_params(frame=0, frame_count=16, rank=3, world=8, **kw))
        assert gpu_ctx.stats().tail_samples == spp * 5 // 16
    film.close()


def test_fused_pipeline_on_trees_without_pair_leaves(pt, orc, gpu_ctx, cornell_arrays):
    """k_fused's second instantiation -- leaves of up to four independent triangles, the trees k_extend_lds7 walks: the box built
    with pt_tuning.pair_leaves = 0, and small soups, which have no fan pairs to find -- against the oracle, both radiance forms."""
    for arrays, pair in ((cornell_arrays, 0), (_soup(100, 5, spread=0.3), 1), (_soup(37, 6, spread=0.5), 1)):
        old = gpu_ctx.set_tuning(pair_leaves=pair)
        try:
            gs = pt.Scene(gpu_ctx, *arrays)
        finally:
            gpu_ctx.set_tuning(**old)
        osc = orc.Scene(*arrays)
        kw = dict(width=90, height=50, spp_per_frame=4, max_depth=7)
        ofilm, obgra, orays = _render_oracle(orc, osc, 2, **kw)
        for shape in (dict(), dict(sample_groups=4), dict(frames_in_flight=1, sample_groups=2)):
            film = pt.Film(gpu_ctx, 90, 50)
            gpu_ctx.reset_stats()
            pt.render(gs, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_FUSED, **kw, **shape))
            assert gpu_ctx.stats().rays == orays and film.read_f32().tobytes() == ofilm.tobytes(), (pair, shape)
            assert film.read_bgra8().tobytes() == obgra.tobytes()
            film.close()
        gs.close()


def test_fused_pipeline_on_instanced_scenes(pt, orc, gpu_ctx, cornell_arrays):
    """PT_PIPELINE_FUSED on two-level scenes (k_fused_inst: the walk of k_extend_inst16 and k_shade<INST>'s hit shading in one
    lane): film, rgba8 image and ray count equal the oracle's bit for bit on rotated + scaled instance sets and on a corner of
    config C4's grid seen from close by -- one accumulator per slot and the term logs, several frames in flight, shards -- and
    under every knob of the kernel: TLAS nodes in LDS (none, all), an LDS stack so short that entries spill to HBM, the
    waiting rules of the leaf phase, the shade block's fill, the per-hit normal transform instead of the table."""
    import importlib
    d = importlib.import_module("single-file-vulkan-pathtracing_amd.distributed")
    grid = pt.cornell_grid_instances().reshape(100, 100, 3, 4)[:12, :12].reshape(-1, 3, 4)
    close = dict(cam_origin=(-0.88, -1.9, 0.5), cam_target=(-0.88, -1.9, 0.0))
    for inst, cam, (w, h, spp, depth, frames) in ((_random_instances(5, 3), {}, (80, 64, 3, 6, 2)), (_random_instances(60, 4), {}, (101, 37, 8, 8, 2)),
                                                   (_random_instances(1500, 5), {}, (64, 48, 4, 13, 1)), (grid, close, (96, 64, 8, 8, 3))):
        gs, osc = pt.Scene(gpu_ctx, *cornell_arrays), orc.Scene(*cornell_arrays)
        gs.set_instances(inst)
        osc.set_instances(inst)
        kw = dict(width=w, height=h, spp_per_frame=spp, max_depth=depth, **cam)
        ofilm, obgra, orays = _render_oracle(orc, osc, frames, **kw)
        assert (ofilm > 0).any()
        for shape in (dict(), dict(frames_in_flight=1, sample_groups=1), dict(sample_groups=spp), dict(frames_in_flight=frames, sample_groups=2 if spp % 2 == 0 else 1)):
            film = pt.Film(gpu_ctx, w, h)
            gpu_ctx.reset_stats()
            pt.render(gs, film, pt.default_params(frame=0, frame_count=frames, pipeline=pt.PIPELINE_FUSED, **kw, **shape))
            st = gpu_ctx.stats()
            assert st.rays == orays, (len(inst), shape, st.rays, orays)
            assert film.read_f32().tobytes() == ofilm.tobytes(), (len(inst), shape)
            assert film.read_bgra8().tobytes() == obgra.tobytes(), (len(inst), shape)
            film.close()
        for knobs in (dict(tlas_lds_kb=0), dict(tlas_lds_kb=64, lds_stack=8), dict(lds_stack=2), dict(enter_min=1, leaf_min=1, node_yield=0),
                      dict(enter_min=64, leaf_min=64, node_yield=2), dict(refill=1), dict(refill=64), dict(inst_frames=0), dict(extend_blocks=1)):
            old = gpu_ctx.set_tuning(**knobs)
            try:
                film = pt.Film(gpu_ctx, w, h)
                gpu_ctx.reset_stats()
                pt.render(gs, film, pt.default_params(frame=0, frame_count=frames, pipeline=pt.PIPELINE_FUSED, **kw))
                assert film.read_f32().tobytes() == ofilm.tobytes() and gpu_ctx.stats().rays == orays, (len(inst), knobs)
                film.close()
            finally:
                gpu_ctx.set_tuning(**old)
        acc, rays = np.zeros_like(ofilm), 0
        for rank in range(3):
            film = pt.Film(gpu_ctx, w, h)
            gpu_ctx.reset_stats()
            pt.render(gs, film, pt.default_params(frame=0, frame_count=frames, rank=rank, world=3, pipeline=pt.PIPELINE_FUSED, **kw))
            rays += gpu_ctx.stats().rays
            part = film.read_f32()
            assert (part[~d.owned_mask(w, h, rank, 3)] == 0).all()
            acc += part
            film.close()
        assert acc.tobytes() == ofilm.tobytes() and rays == orays
        gs.close()
    # BLAS leaves of up to four independent triangles instead of fan pairs (the kernel's other instantiation): the box built with
    # pt_tuning.pair_leaves = 0, and a 100-triangle soup, which has no pairs to find
    inst = _random_instances(9, 11)
    for arrays, pair in ((cornell_arrays, 0), (_soup(100, 5, spread=0.3), 1)):
        old = gpu_ctx.set_tuning(pair_leaves=pair)
        try:
            gs = pt.Scene(gpu_ctx, *arrays)
        finally:
            gpu_ctx.set_tuning(**old)
        osc = orc.Scene(*arrays)
        gs.set_instances(inst)
        osc.set_instances(inst)
        kw = dict(width=72, height=40, spp_per_frame=4, max_depth=6)
        ofilm, obgra, orays = _render_oracle(orc, osc, 2, **kw)
        for shape in (dict(), dict(sample_groups=4)):
            film = pt.Film(gpu_ctx, 72, 40)
            gpu_ctx.reset_stats()
            pt.render(gs, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_FUSED, **kw, **shape))
            assert gpu_ctx.stats().rays == orays and film.read_f32().tobytes() == ofilm.tobytes(), (pair, shape)
            assert film.read_bgra8().tobytes() == obgra.tobytes()
            film.close()
        gs.close()


def test_fused_pipeline_shards_term_log_tiers_and_refusals(pt, orc, gpu_ctx, cornell_gpu):
    """Fused renders of (rank, world) shards add up to the single-device film; the three tiers of the term log (primary,
    overflow, shared pool) and the redo of a batch whose pool overflowed give the same bits; the tuning knobs change no bit;
    what the kernel is not built for is refused with PT_ERR_UNSUPPORTED (one-instance scenes, scenes beyond LDS, tmin <= 0, async)."""
    import importlib
    d = importlib.import_module("single-file-vulkan-pathtracing_amd.distributed")
    w, h = 200, 120
    kw = dict(width=w, height=h, spp_per_frame=8, max_depth=8, frame=0, frame_count=2)
    ref = pt.Film(gpu_ctx, w, h)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, ref, pt.default_params(**kw))                                   # the wavefront pipeline
    want, rays_want = ref.read_f32(), gpu_ctx.stats().rays
    ref.close()
    for world in (2, 8):
        acc, rays = np.zeros_like(want), 0
        for rank in range(world):
            film = pt.Film(gpu_ctx, w, h)
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.default_params(rank=rank, world=world, pipeline=pt.PIPELINE_FUSED, **kw))
            rays += gpu_ctx.stats().rays
            part = film.read_f32()
            assert (part[~d.owned_mask(w, h, rank, world)] == 0).all()
            acc += part
            film.close()
        assert acc.tobytes() == want.tobytes() and rays == rays_want
    for knobs in (dict(term_ocap=0, term_spill=1 << 20), dict(term_ocap=1, term_spill=1 << 20), dict(term_ocap=0, term_spill=3),
                  dict(refill=1), dict(refill=40), dict(refill=64), dict(extend_blocks=2)):
        old = gpu_ctx.set_tuning(**knobs)
        try:
            film = pt.Film(gpu_ctx, w, h)
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, sample_groups=4, **kw))
            st = gpu_ctx.stats()
            assert film.read_f32().tobytes() == want.tobytes() and st.rays == rays_want, knobs
            if knobs.get("term_spill") == 3:
                assert st.redone_batches >= 1
            film.close()
        finally:
            gpu_ctx.set_tuning(**old)
    film = pt.Film(gpu_ctx, w, h)
    for bad in (dict(pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_ASYNC),
                dict(pipeline=pt.PIPELINE_FUSED, extend=pt.EXTEND_HBM), dict(pipeline=pt.PIPELINE_FUSED, tmin=0.0), dict(pipeline=4)):
        with pytest.raises(pt.PtError) as e:
            pt.render(cornell_gpu, film, pt.default_params(**{**kw, **bad}))
        assert e.value.status == 5, bad                                                     # PT_ERR_UNSUPPORTED
    inst = pt.Scene(gpu_ctx, *pt.load_obj(pt.ASSET_CORNELL))
    inst.set_instances(pt.cornell_grid_instances()[:1])       # one instance: no fp16 TLAS, the general two-level kernel's scene
    with pytest.raises(pt.PtError):
        pt.render(inst, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, **kw))
    inst.set_instances(pt.cornell_grid_instances()[:16])      # (k_fused_inst's class: test_fused_pipeline_on_instanced_scenes)
    with pytest.raises(pt.PtError):
        pt.render(inst, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, **{**kw, "tmin": 0.0}))
    inst.close()
    v, i, f = _soup(3000, 5)
    big = pt.Scene(gpu_ctx, v, i, f)
    with pytest.raises(pt.PtError):
        pt.render(big, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, **kw))
    big.close()
    # the film is still usable by the wavefront pipeline after the refusals and after fused renders (shared workspace)
    film.clear()
    pt.render(cornell_gpu, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, **kw))
    film.clear()
    pt.render(cornell_gpu, film, pt.default_params(**kw))
    assert film.read_f32().tobytes() == want.tobytes()
    film.close()


def test_fused_pipeline_full_size_c2_frame_equals_the_oracle_known_answer(pt, gpu_ctx, cornell_gpu):
    """BASELINE config C2's frame 0 at 1920x1080 through the fused kernel: the oracle's exact ray count and SHA-256, for one
    and for several sample groups; then frames 0..3 in one call against the C3 known answer after frame 3."""
    import hashlib
    import json
    gold = json.load(open(os.path.join(HERE, "golden", "fullsize_hashes.json")))
    g2 = gold["c2"]
    w, h = g2["width"], g2["height"]
    kw = dict(width=w, height=h, spp_per_frame=g2["spp_per_frame"], max_depth=g2["max_depth"], pipeline=pt.PIPELINE_FUSED)
    film = pt.Film(gpu_ctx, w, h)
    for shape in (dict(), dict(sample_groups=1), dict(sample_groups=4)):
        film.clear()
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=1, **kw, **shape))
        assert gpu_ctx.stats().rays == g2["rays"], shape
        assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == g2["film_sha256"], shape
    g3 = gold.get("c3")
    if g3 is not None:
        film.clear()
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=4, **kw))
        m = g3["after_frame"]["3"]
        assert gpu_ctx.stats().rays == m["rays_so_far"]
        assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == m["film_sha256"]
        assert hashlib.sha256(film.read_bgra8().tobytes()).hexdigest() == m["bgra8_sha256"]
    film.close()


def test_failed_rebuild_marks_the_scene_broken_and_the_next_use_repairs_it(pt, orc, gpu_ctx):
    """a rebuild of a big scene's tree products frees the old ones first; if it then fails (out of memory
    beside a large film workspace) the scene must not be traversed on null tables.  pt_tuning.fail_rebuild makes the next rebuild
    fail right after the free: the call returns an error, the scene is unusable for exactly as long as rebuilds fail -- every
    render / trace / read-back answers with a clean status, the film stays usable -- and the first call after that repairs it
    and renders the same bits as before."""
    v, i, f = _soup(6000, 77, spread=0.05)
    v = v.reshape(-1, 3) * np.float32([0.9, 0.9, 0.9]) + np.float32([0, -1, 0])
    scene = pt.Scene(gpu_ctx, v.reshape(-1), i, f)
    w, h = 96, 64
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=5, frame=0, frame_count=1)
    film = pt.Film(gpu_ctx, w, h)
    pt.render(scene, film, pt.default_params(**kw))
    want = film.read_f32().tobytes()
    rays = np.zeros((16, 6), np.float32); rays[:, 2] = 5; rays[:, 1] = -1; rays[:, 5] = -1
    hits_before = scene.trace(rays).tobytes()
    old = gpu_ctx.set_tuning(fail_rebuild=2)
    try:
        with pytest.raises(pt.PtError):
            scene.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)          # the rebuild fails after the old tree is gone
        film.clear()
        with pytest.raises(pt.PtError):
            pt.render(scene, film, pt.default_params(**kw))           # the repair attempt fails too (second forced failure)
        assert not film.read_f32().any()                              # nothing touched the film
        assert scene.info().n_wide_nodes == 0
    finally:
        gpu_ctx.set_tuning(**old)
    film.clear()
    pt.render(scene, film, pt.default_params(**kw))                   # repaired on this call (the quality that was asked for)
    assert film.read_f32().tobytes() == want
    assert scene.trace(rays).tobytes() == hits_before
    scene.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)
    film.clear()
    pt.render(scene, film, pt.default_params(**kw))
    assert film.read_f32().tobytes() == want
    film.close(); scene.close()


def test_sah_device_builder_makes_its_committed_trees(pt, gpu_ctx):
    """The device surface-area BVH4 builder against the rows committed in tests/golden/sah_rows.npz (made on a GPU box by
    tests/golden/make_sah_rows.py): the Cornell box and a 700-triangle soup, every node word."""
    path = os.path.join(HERE, "golden", "sah_rows.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/sah_rows.npz not generated yet")
    g = np.load(path)
    for name, arrays in (("cornell", pt.load_obj(pt.ASSET_CORNELL)), ("soup700", _soup(700, 11))):
        sc = pt.Scene(gpu_ctx, *arrays)
        assert sc.info().bvh4_builder == 1
        got = sc.read_bvh4()
        assert got.shape == g[name].shape and got.tobytes() == g[name].tobytes(), name
        sc.close()


def test_fused_block_counts_instrumented_twin_is_bit_exact_and_consistent(pt, gpu_ctx, cornell_gpu):
    """PT_FLAG_COUNT_VISITS on the fused pipeline (API v6): the instrumented twin of k_fused renders the same film and ray count as the product
    kernel, through its three forms (one group, several groups, head + tail), and its wave-level block counts (pt_get_block_counts) are
    consistent with the ray count: every walked ray is set up once and finished once, every shaded hit is a miss or a surface hit, a camera ray
    per sample.  Two-level scenes have no instrumented fused form."""
    w, h = 200, 120
    kw = dict(width=w, height=h, spp_per_frame=8, max_depth=8, frame=0, frame_count=3)
    for shape in (dict(sample_groups=1), dict(sample_groups=4), dict()):
        old = gpu_ctx.set_tuning(cull=1)
        try:
            film = pt.Film(gpu_ctx, w, h)
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, **shape, **kw))
            want, rays, culled = film.read_f32(), gpu_ctx.stats().rays, gpu_ctx.stats().rays_culled
            film.clear()
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_COUNT_VISITS, **shape, **kw))
            st = gpu_ctx.stats()
            bc = gpu_ctx.block_counts()
        finally:
            gpu_ctx.set_tuning(**old)
        assert film.read_f32().tobytes() == want.tobytes() and st.rays == rays and st.rays_culled == culled, shape
        film.close()
        walked = rays - culled
        assert bc["SETUP"][1] == walked and bc["FINISH"][1] == walked, (shape, bc, walked)
        assert bc["HIT"][1] == walked and bc["MISS"][1] + bc["SURFACE"][1] == walked
        assert bc["BOUNCE"][1] + bc["PRIMARY"][1] == walked                      # every walked ray is a bounce ray or a camera ray
        assert bc["NODE"][0] > 0 and bc["LEAF"][1] >= bc["DIV"][1] > 0 and bc["ITER"][0] >= bc["SHADE"][0] > 0
        assert all(wv <= ln <= 64 * wv for wv, ln in bc.values())
    inst = pt.Scene(gpu_ctx, *pt.load_obj(pt.ASSET_CORNELL))
    inst.set_instances(pt.cornell_grid_instances()[:16])
    film = pt.Film(gpu_ctx, w, h)
    with pytest.raises(pt.PtError) as e:
        pt.render(inst, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_COUNT_VISITS, **kw))
    assert e.value.status == 5
    film.close(); inst.close()


def test_reference_dispatch_1024_four_blocking_frames_equal_the_oracle_known_answers(pt, gpu_ctx, cornell_gpu):
    """The reference's OWN launch -- WIDTH = HEIGHT = 1024 (main.cpp:16-17), traceRaysKHR(WIDTH, HEIGHT, 1) (main.cpp:659), 32 spp (raygen.rgen:43), 8
    bounces: exactly what pt_params_default returns -- issued as its frame loop issues it (main.cpp:647-685): one blocking call per frame, frame = 0, 1, 2,
    3 as the push constant, through the library default (PT_PIPELINE_AUTO).  After every frame the exact ray count, the float film and the bgra8 storage
    image are the oracle's known answers (tests/golden/fullsize_hashes.json "ref1024", tests/golden/make_fullsize_hashes.py ref1024); then the same four
    frames as ONE call, and through the wavefront pipeline."""
    import hashlib
    import json
    path = os.path.join(HERE, "golden", "fullsize_hashes.json")
    gold = json.load(open(path)).get("ref1024")
    if gold is None:
        pytest.skip(f"no known answer for ref1024 in {path}")
    p0 = pt.library_default_params()
    assert (p0.width, p0.height, p0.spp_per_frame, p0.max_depth, p0.pipeline) == (gold["width"], gold["height"], 32, 8, pt.PIPELINE_AUTO)
    film = pt.Film(gpu_ctx, p0.width, p0.height)
    for g in gold["frames"]:
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.library_default_params(frame=g["frame"], frame_count=1))     # blocking: returns when the device is done
        st = gpu_ctx.stats()
        assert st.pipeline == pt.PIPELINE_FUSED and st.rays == g["rays"], g["frame"]
        assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == g["film_sha256"], g["frame"]
        assert hashlib.sha256(film.read_bgra8().tobytes()).hexdigest() == g["bgra8_sha256"], g["frame"]
    last = gold["frames"][-1]
    for kw in (dict(), dict(pipeline=pt.PIPELINE_WAVEFRONT)):
        film.clear()
        gpu_ctx.reset_stats()
        pt.render(cornell_gpu, film, pt.library_default_params(frame=0, frame_count=len(gold["frames"]), **kw))
        assert gpu_ctx.stats().rays == gold["rays"], kw
        assert hashlib.sha256(film.read_f32().astype("<f4").tobytes()).hexdigest() == last["film_sha256"], kw
        assert hashlib.sha256(film.read_bgra8().tobytes()).hexdigest() == last["bgra8_sha256"], kw
    film.close()


def test_reference_dispatch_1024_equals_the_references_own_shaders(pt, gpu_ctx, cornell_gpu):
    """The reference's own launch against the reference's own compiled shaders (tests/golden/spirv_ref1024.npz: shaders/*.spv executed by oracle/spirv_vm.py for a
    64 x 48 rectangle and a scattered pixel set of the 1024 x 1024 launch, frames 0 .. 3): pt_params_default untouched, one blocking call per frame through the
    library default (PT_PIPELINE_AUTO -> the fused kernel), and after every frame the film's texels -- and, for a sixth of the set, the bgra8 image -- are the
    shaders' bit for bit.  (test_reference_dispatch_1024_four_blocking_frames_* checks the WHOLE frames against the oracle's SHA-256.)"""
    path = os.path.join(HERE, "golden", "spirv_ref1024.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/spirv_ref1024.npz not generated")
    g = np.load(path)
    w, h = [int(v) for v in g["launch"]]
    p0 = pt.library_default_params()
    assert (p0.width, p0.height, p0.spp_per_frame, p0.max_depth) == (w, h, 32, 8)
    x0, y0, rw, rh = [int(v) for v in g["rect"]]
    film = pt.Film(gpu_ctx, w, h)
    for frame in range(g["rect_texels"].shape[0]):
        pt.render(cornell_gpu, film, pt.library_default_params(frame=frame, frame_count=1))
        assert gpu_ctx.stats().pipeline == pt.PIPELINE_FUSED
        got = film.read_f32()
        assert np.ascontiguousarray(got[y0:y0 + rh, x0:x0 + rw]).tobytes() == np.ascontiguousarray(g["rect_texels"][frame, :, :, :3]).tobytes(), frame
        px = g["pixels"]
        assert np.ascontiguousarray(got[px[:, 1], px[:, 0]]).tobytes() == np.ascontiguousarray(g["texels"][frame, :, :3]).tobytes(), frame
        bg = film.read_bgra8()
        pb = g["pixels_rgba8"]
        assert np.ascontiguousarray(bg[pb[:, 1], pb[:, 0]][:, [2, 1, 0, 3]]).tobytes() == np.ascontiguousarray(g["rgba8"][frame]).tobytes(), frame
    film.close()
