"""The compact walk's cut keys on the GPU (csrc/extend_kernel.h: compact_node_step culls a child by its KEY at the push, the pops compare the
raw entry, the BOTTOM entry's key is +0): film and ray count bit for bit against the CPU oracle, through the fused pipeline and through the
wavefront pipeline's LDS kernel, on the smallest scenes at which the rule can go wrong.  tests/test_cut_key_cpu.py has the identities.
"""
import numpy as np
import pytest

W = H = 32
KW = dict(width=W, height=H, spp_per_frame=2, max_depth=4)
FRAMES = 2
CAM_Z = dict(cam_origin=(0.05, 0.1, 3.0), cam_target=(0.0, 0.0, 0.0))
PT_LEAF = 0x80000000
NONE = 0xFFFFFFFF
PIPELINES = ("FUSED", "WAVEFRONT")


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _faces(n_tris, emit=()):
    f = np.zeros((n_tris, 6), np.float32)
    k = np.arange(n_tris)
    f[:, 0], f[:, 1], f[:, 2] = 0.3 + 0.1 * (k % 5), 0.8 - 0.1 * (k % 7), 0.4 + 0.05 * (k % 9)
    for t in emit:
        f[t, 3:6] = (4.0, 3.0, 2.0)
    return f.reshape(-1)


def _quad(cx, cy, z, hx, hy):
    return np.float32([[cx - hx, cy - hy, z], [cx + hx, cy - hy, z], [cx + hx, cy + hy, z], [cx - hx, cy + hy, z]])


def _quads(quads, emit=()):
    v = np.concatenate(quads).astype(np.float32)
    i = np.concatenate([np.uint32([4 * q, 4 * q + 1, 4 * q + 2, 4 * q, 4 * q + 2, 4 * q + 3]) for q in range(len(quads))])
    return v.reshape(-1), i, _faces(2 * len(quads), emit)


def coincident_quads():
    """(a) the SAME quad twice, as primitives 0, 1 and 14, 15 (different colours: the film shows which one won), six quads between them in
    the file -- satellites in front of and behind it and a floor -- so that the two copies are different leaves of a tree with more than one
    node: when the first copy's hit has set best_t the second one's entry starts exactly there, and has to survive the cull for the
    lowest-primitive-id rule"""
    main = _quad(0.0, 0.0, 0.0, 0.7, 0.5)
    floor = np.float32([[-2.0, -0.8, -2.0], [2.0, -0.8, -2.0], [2.0, -0.8, 2.0], [-2.0, -0.8, 2.0]])
    sats = [_quad(-1.1, 0.6, 0.4, 0.2, 0.2), _quad(1.1, 0.6, -0.4, 0.2, 0.2), _quad(-1.1, -0.4, -0.6, 0.2, 0.2), _quad(1.1, -0.4, 0.7, 0.2, 0.2),
            _quad(0.0, 0.9, -0.9, 0.3, 0.15)]
    return _quads([main, *sats[:3], floor, *sats[3:], main.copy()], emit=(8, 9, 12, 13))


def one_triangle():
    """(c) a one-node tree: nothing is ever pushed, the first pop takes the BOTTOM entry"""
    v = np.float32([[-0.9, -0.7, 0.0], [0.9, -0.6, 0.0], [0.1, 0.8, 0.0]])
    return v.reshape(-1), np.arange(3, dtype=np.uint32), _faces(1, emit=(0,))


# (d) the chain of tests/test_lds_plan.py::test_stack_bound_at_the_class_maximum: quads nested in a cone whose apex is the camera, a tree whose
# exact stack bound is 16 -- every level of the plan's stack is written by the new push
CHAIN_N, CHAIN_RATIO, CHAIN_D = 18, 0.7, 40.0
CAM_CONE = dict(cam_origin=(0.0, 0.0, CHAIN_D), cam_target=(0.0, 0.0, 0.0))


def chain(n):
    quads = []
    for q in range(n):
        k = CHAIN_RATIO ** q
        quads.append(_quad(0.3 * k, -0.2 * k, CHAIN_D * (1.0 - k), 9.0 * k, 8.0 * k))
    return _quads(quads, emit=(0, 1, 2 * (n - 1), 2 * (n - 1) + 1))


def stack_need(wide):
    def need(nd):
        kids = [int(w) for w in wide[nd, 24:28] if w != NONE]
        return max(len(kids) - 1, 0) + max([need(w) for w in kids if not w & PT_LEAF], default=0)
    return need(0)


def n_leaves(wide):
    w = wide[:, 24:28].reshape(-1)
    return int(((w != NONE) & ((w & PT_LEAF) != 0)).sum())


# ---- references -------------------------------------------------------------------------------------------------------------------
_want = {}


def oracle_film(orc, name, arrays, **params):
    """-> (film after FRAMES frames, ray count); computed once per scene and parameter set"""
    key = (name, tuple(sorted(params.items())))
    if key not in _want:
        osc = orc.Scene(*arrays)
        film, rays = np.zeros((H, W, 3), np.float32), 0
        for k in range(FRAMES):
            img, r, _, _ = osc.render_frame(orc.default_params(frame=k, **KW, **params))
            orc.accumulate_f32(film, img, k)
            rays += r
        film.setflags(write=False)
        _want[key] = (film, rays)
    return _want[key]


def check(pt, orc, ctx, sc, name, arrays, pipeline, **params):
    want, rays = oracle_film(orc, name, arrays, **params)
    film = pt.Film(ctx, W, H)
    old = ctx.set_tuning(fused_tail=0)
    try:
        ctx.reset_stats()
        pt.render(sc, film, pt.default_params(frame=0, frame_count=FRAMES, pipeline=getattr(pt, "PIPELINE_" + pipeline), **KW, **params))
        got, st = film.read_f32(), ctx.stats()
    finally:
        ctx.set_tuning(**old)
        film.close()
    assert st.pipeline == getattr(pt, "PIPELINE_" + pipeline) and st.extend_variant == pt.EXTEND_LDS, (name, pipeline, st.pipeline, st.extend_variant)
    assert st.rays == rays, (name, pipeline, st.rays, rays)
    assert got.tobytes() == want.tobytes(), (name, pipeline, int((got != want).sum()))
    return want, rays


def random_rays(n=4096, seed=17):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1.5, 1.5, (n, 3)), rng.normal(size=(n, 3))], axis=1).astype(np.float32)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_coincident_quads(pt, orc, gpu_ctx, pipeline):
    arrays = coincident_quads()
    sc = pt.Scene(gpu_ctx, *arrays)
    try:
        wide = sc.read_bvh4()
        assert n_leaves(wide) == 8 and wide.shape[0] >= 2, (n_leaves(wide), wide.shape)   # one pair leaf per quad: the two copies are two leaves
        want, _ = check(pt, orc, gpu_ctx, sc, "coincident", arrays, pipeline, **CAM_Z)
        assert want[H // 2, W // 2].any()   # (the centre pixel looks at the doubled quad)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tmax", [float("inf"), 10000.0, 0.25], ids=["inf", "10000", "short"])
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_cornell_tmax(pt, orc, gpu_ctx, cornell_gpu, cornell_arrays, pipeline, tmax):
    """(b) tmax = +inf: the cap of the push cut is all that keeps the miss keys out; tmax below every surface: every child of the root is
    culled at the push and the first pop takes the BOTTOM entry"""
    _, rays = check(pt, orc, gpu_ctx, cornell_gpu, "cornell", cornell_arrays, pipeline, tmax=tmax)
    if tmax < 1.0:
        assert rays == W * H * KW["spp_per_frame"] * FRAMES, rays   # (every camera ray misses: no bounce)
    else:
        assert rays > 2 * W * H * KW["spp_per_frame"] * FRAMES, rays


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_one_triangle(pt, orc, gpu_ctx, pipeline):
    arrays = one_triangle()
    sc = pt.Scene(gpu_ctx, *arrays)
    try:
        wide = sc.read_bvh4()
        assert wide.shape[0] == 1 and stack_need(wide) == 0 and n_leaves(wide) == 1
        want, _ = check(pt, orc, gpu_ctx, sc, "triangle", arrays, pipeline, **CAM_Z)
        assert want.any()
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_full_stack(pt, orc, gpu_ctx, pipeline):
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
        check(pt, orc, gpu_ctx, sc, f"chain{found}", arrays, pipeline, **CAM_CONE)
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["coincident", "triangle"])
def test_trace(pt, orc, gpu_ctx, scene):
    """pt_trace (k_extend_lds7 / _lds7p alone): 4 096 random rays, hit records bit for bit"""
    arrays = coincident_quads() if scene == "coincident" else one_triangle()
    rays = random_rays()
    sc = pt.Scene(gpu_ctx, *arrays)
    try:
        got = sc.trace(rays)
    finally:
        sc.close()
    want, _ = orc.Scene(*arrays).trace(rays)
    assert got.tobytes() == want.tobytes(), int((got["prim"] != want["prim"]).sum())
    n_hit = int((got["prim"] != pt.MISS).sum())
    assert 20 <= n_hit <= len(rays) - 20, n_hit   # (hits and misses both)
