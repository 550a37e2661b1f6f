"""The LDS plan of the compact class (lds_scene.h, extend_kernel.h LaneStack, fused_kernel.h fused_lds): scene tables at LDS byte 0, the
stack behind them and held as the address of its top entry, nodes of ten float4 with the low plane of every axis twice.

Everything here is bit-exact against the CPU oracle (or, for the guide buffers, against their other pipeline), on scenes chosen for the
places where a plan can go wrong: the empty stack (a one-node tree), the stack's last level (a tree whose exact bound is the class maximum,
16), the read behind the last triangle record (single-triangle leaves), and the class limit itself (the largest scene it admits).
"""
import numpy as np
import pytest

W = H = 64
KW = dict(width=W, height=H, spp_per_frame=4, max_depth=8)
FRAMES = 2
CAM_Z = dict(cam_origin=(0.05, 0.1, 3.0), cam_target=(0.0, 0.0, 0.0))   # looks down -z: every camera ray's dominant axis is z (kz = 2)
PT_LEAF = 0x80000000
NONE = 0xFFFFFFFF


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _faces(n_tris, emit=()):
    """Kd varied per triangle, Ke on the triangles named in `emit`"""
    f = np.zeros((n_tris, 6), np.float32)
    k = np.arange(n_tris)
    f[:, 0], f[:, 1], f[:, 2] = 0.3 + 0.1 * (k % 5), 0.8 - 0.1 * (k % 7), 0.4 + 0.05 * (k % 9)
    for t in emit:
        f[t, 3:6] = (4.0, 3.0, 2.0)
    return f.reshape(-1)


def _quad(cx, cy, z, hx, hy):
    return np.float32([[cx - hx, cy - hy, z], [cx + hx, cy - hy, z], [cx + hx, cy + hy, z], [cx - hx, cy + hy, z]])


def _quads(quads, emit=()):
    """quads as fans (v0 v1 v2) (v0 v2 v3): the builder makes one pair leaf of each"""
    v = np.concatenate(quads).astype(np.float32)
    i = np.concatenate([np.uint32([4 * q, 4 * q + 1, 4 * q + 2, 4 * q, 4 * q + 2, 4 * q + 3]) for q in range(len(quads))])
    return v.reshape(-1), i, _faces(2 * len(quads), emit)


def one_quad():
    return _quads([_quad(0.0, 0.0, 0.0, 0.8, 0.6)], emit=(0, 1))


# Quads nested in a cone whose apex is the camera: quad q stands at CHAIN_RATIO ** q of the first one's distance and is that much smaller, so every
# camera ray inside the cone crosses all of them, nearest (smallest) first.  The boxes shrink fast enough that the surface-area builder peels the
# big quads off one after the other: a chain of nodes with three leaves and one inner child each, the inner child the nearest -- a ray descends
# into it with the three leaves pending, level after level.  CHAIN_N is the count at which the traversed tree's exact stack bound is 16, the most
# the compact class takes (the test computes the bound from the tree it reads back and says so if a change to the builder moved it).
CHAIN_N, CHAIN_RATIO, CHAIN_D = 18, 0.7, 40.0
CAM_CONE = dict(cam_origin=(0.0, 0.0, CHAIN_D), cam_target=(0.0, 0.0, 0.0))


def chain(n=None):
    n = CHAIN_N if n is None else n
    quads = []
    for q in range(n):
        k = CHAIN_RATIO ** q
        quads.append(_quad(0.3 * k, -0.2 * k, CHAIN_D * (1.0 - k), 9.0 * k, 8.0 * k))
    return _quads(quads, emit=(0, 1, 2 * (n - 1), 2 * (n - 1) + 1))


def lone_triangles(n=7):
    """n triangles that share no edge (no fan pairs: every leaf is ONE triangle), all facing the camera of CAM_Z and all seen by it"""
    v = []
    for k in range(n):
        cx, cy, z = -0.9 + 0.3 * k, 0.5 * np.sin(1.7 * k), -0.1 * k
        v += [[cx - 0.14, cy - 0.3, z], [cx + 0.14, cy - 0.25, z], [cx, cy + 0.3, z]]
    return np.float32(v).reshape(-1), np.arange(3 * n, dtype=np.uint32), _faces(n, emit=(3,))


def soup(n, seed=5):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3))
    v = (c + rng.uniform(-0.25, 0.25, (n, 3, 3))).astype(np.float32)
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), _faces(n, emit=(0,))


def stack_need(wide):
    """most entries a depth-first walk of a BVH4 can have pending (rows of 32 dwords, child words at 24..27): a node with k children pushes
    k - 1 of them before it descends"""
    def need(nd):
        kids = [int(w) for w in wide[nd, 24:28] if w != NONE]
        return max(len(kids) - 1, 0) + max([need(w) for w in kids if not w & PT_LEAF], default=0)
    return need(0)


def leaf_words(wide):
    w = wide[:, 24:28].reshape(-1)
    return w[(w != NONE) & ((w & PT_LEAF) != 0)]


# ---- references -------------------------------------------------------------------------------------------------------------------
_want = {}


def oracle_film(orc, name, arrays, nee=False, **cam):
    """-> (film f32 after FRAMES frames, ray count, prims the camera rays of frame 0 hit); computed once per scene and estimator"""
    key = (name, nee)
    if key not in _want:
        osc = orc.Scene(*arrays)
        film, rays, seen = np.zeros((H, W, 3), np.float32), 0, None
        for k in range(FRAMES):
            img, r, _, fh = osc.render_frame(orc.default_params(frame=k, **(dict(nee=1) if nee else {}), **KW, **cam), want_first_hits=(k == 0))
            orc.accumulate_f32(film, img, k)
            rays += r
            if k == 0:
                seen = set(int(p) for p in np.unique(fh["prim"])) - {NONE}
        film.setflags(write=False)
        _want[key] = (film, rays, seen)
    return _want[key]


def render(pt, ctx, sc, tuning=None, **params):
    film = pt.Film(ctx, W, H)
    old = ctx.set_tuning(**(tuning or {}))
    try:
        ctx.reset_stats()
        pt.render(sc, film, pt.default_params(frame=0, frame_count=FRAMES, **KW, **params))
        return film.read_f32(), ctx.stats()
    finally:
        ctx.set_tuning(**old)
        film.close()


# the three shapes of the fused pipeline (one sample group; several: every slot logs its terms; head + tail slots), NEE, and the wavefront
# pipeline, whose k_extend_lds7p stages the same image
SHAPES = {"fused": (dict(fused_tail=0), dict(pipeline="FUSED", sample_groups=1)),
          "fused_groups": (dict(fused_tail=0), dict(pipeline="FUSED", sample_groups=4)),
          "fused_tail": (dict(fused_tail=2), dict(pipeline="FUSED")),
          "fused_nee": (dict(fused_tail=0), dict(pipeline="FUSED", nee=True)),
          "wavefront": (dict(), dict(pipeline="WAVEFRONT"))}


def check(pt, orc, ctx, sc, name, arrays, shape, **cam):
    tuning, kw = SHAPES[shape]
    kw = dict(kw)
    nee = kw.pop("nee", False)
    pipeline = getattr(pt, "PIPELINE_" + kw.pop("pipeline"))
    want, rays, _ = oracle_film(orc, name, arrays, nee=nee, **cam)
    got, st = render(pt, ctx, sc, tuning, pipeline=pipeline, flags=pt.FLAG_NEE if nee else 0, **kw, **cam)
    assert st.pipeline == pipeline and st.extend_variant == pt.EXTEND_LDS, (name, shape, st.pipeline, st.extend_variant)
    assert st.rays == rays, (name, shape, st.rays, rays)
    assert got.tobytes() == want.tobytes(), (name, shape, int((got != want).sum()))
    return st


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_cornell(pt, orc, gpu_ctx, cornell_gpu, cornell_arrays, shape):
    st = check(pt, orc, gpu_ctx, cornell_gpu, "cornell", cornell_arrays, shape)
    if shape == "fused_groups":
        assert st.sample_groups == 4, st.sample_groups
    if shape.startswith("fused"):
        assert st.tail_samples == (2 if shape == "fused_tail" else 0), (shape, st.tail_samples)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_one_node_tree(pt, orc, gpu_ctx, shape):
    """a single quad: the root's one child is a leaf, nothing is ever pushed -- every read of the stack's top entry lands on level -1 and every
    pop finds the stack empty"""
    arrays = one_quad()
    sc = pt.Scene(gpu_ctx, *arrays)
    try:
        wide = sc.read_bvh4()
        assert wide.shape[0] == 1 and stack_need(wide) == 0 and len(leaf_words(wide)) == 1
        check(pt, orc, gpu_ctx, sc, "one_quad", arrays, shape, **CAM_Z)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_stack_bound_at_the_class_maximum(pt, orc, gpu_ctx, shape):
    """a chain of nested quads whose tree has the exact stack bound 16: pushes reach the last level of the plan.  The count of quads at which the
    builder's tree has that bound is searched around CHAIN_N, so a change to the builder moves the scene, not the verdict"""
    found = None
    for n in [CHAIN_N] + [m for m in range(12, 28) if m != CHAIN_N]:
        arrays = chain(n)
        sc = pt.Scene(gpu_ctx, *arrays)
        if stack_need(sc.read_bvh4()) == 16:
            found = n
            break
        sc.close()
    assert found is not None, "no chain of 12 .. 27 nested quads gives the builder's tree the stack bound 16"
    try:
        check(pt, orc, gpu_ctx, sc, f"chain{found}", arrays, shape, **CAM_CONE)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_single_triangle_leaves(pt, orc, gpu_ctx, shape):
    """every leaf one triangle, every triangle hit by camera rays whose dominant axis is z: the leaf step of the LAST record of the kz = 2
    copy runs, and the fused kernel's reads up to three float4 behind that record (pair_leaf.h LOAD_D_FIRST, D_FIRST_OVERREAD_F4) -- into the
    shade table, which the plan keeps right there.  What this proves is that the walk is right on such leaves: a single triangle does not USE
    what was read behind it, so a wrong placement of the shade table would not show here (the plans' static_asserts are what states it)"""
    arrays = lone_triangles()
    n = len(arrays[1]) // 3
    sc = pt.Scene(gpu_ctx, *arrays)
    try:
        leaves = leaf_words(sc.read_bvh4())
        assert len(leaves) == n and (((leaves >> 28) & 7) == 0).all()           # count - 1 == 0 everywhere
        assert sorted(int(w & 0x0FFFFFFF) for w in leaves) == list(range(n))    # ... and the last position is one of them
        _, _, seen = oracle_film(orc, "lone", arrays, **CAM_Z)
        assert seen == set(range(n))
        check(pt, orc, gpu_ctx, sc, "lone", arrays, shape, **CAM_Z)
    finally:
        sc.close()


@pytest.mark.gpu
def test_largest_scene_of_the_lds_class(pt, orc, gpu_ctx):
    """The class limit is 24 KB of triangle copies and nodes counted at 144 B: the biggest soup under it is still walked in LDS -- its image,
    with nodes of 160 B, is past 24 KB -- the next bigger one is not, and the hits are the oracle's."""
    def build(n):
        arrays = soup(n)
        sc = pt.Scene(gpu_ctx, *arrays)
        info = sc.info()
        return arrays, sc, 144 * (info.n_wide_nodes + info.n_tris), 160 * info.n_wide_nodes + 144 * info.n_tris
    rng = np.random.default_rng(11)
    rays = np.concatenate([rng.uniform(-1.2, 1.2, (20000, 3)), rng.normal(size=(20000, 3))], axis=1).astype(np.float32)
    found = None
    for n in range(140, 100, -1):
        arrays, sc, class_bytes, image_bytes = build(n)
        try:
            variant = render(pt, gpu_ctx, sc, pipeline=pt.PIPELINE_WAVEFRONT, **CAM_Z)[1].extend_variant   # (pt_render reports the walk it planned)
            got = sc.trace(rays)
            assert (variant == pt.EXTEND_LDS) == (class_bytes <= 24 * 1024), (n, class_bytes, variant)
            if variant == pt.EXTEND_LDS:
                found = (n, class_bytes, image_bytes)
                want, _ = orc.Scene(*arrays).trace(rays)
                assert got.tobytes() == want.tobytes()
                n_hit = int((got["prim"] != pt.MISS).sum())
                assert 1000 <= n_hit <= len(rays) - 1000, n_hit   # (hits and misses both: the comparison above is about something)
                break
        finally:
            sc.close()
    print("largest soup of the LDS class: n, class bytes, image bytes =", found)
    assert found and found[0] < 140 and found[2] > 24 * 1024, found


@pytest.mark.gpu
def test_aov_fused_equals_wavefront(pt, gpu_ctx, cornell_gpu):
    """pt_render_aov on the Cornell box: the single-kernel form (k_aov_fused: tables at LDS byte 0, LaneStack) against the queue form"""
    planes = {}
    for name in ("WAVEFRONT", "FUSED"):
        film = pt.Film(gpu_ctx, W, H)
        try:
            film.enable_aov()
            gpu_ctx.reset_stats()
            pt.render_aov(cornell_gpu, film, pt.default_params(frame=0, frame_count=FRAMES, pipeline=getattr(pt, "PIPELINE_" + name), width=W, height=H, spp_per_frame=4))
            assert gpu_ctx.stats().pipeline == getattr(pt, "PIPELINE_" + name)
            planes[name] = [film.read_aov(k) for k in range(6)]
        finally:
            film.close()
    for k, (a, b) in enumerate(zip(planes["WAVEFRONT"], planes["FUSED"])):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert planes["FUSED"][0].any()
