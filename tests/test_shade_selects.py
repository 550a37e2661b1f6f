"""k_fused's shade block written as selects (fused_kernel.h step (1)): a miss is record n_tris of the shade table, `color +=` runs without a
vote with one sample group, and a path's end is a select -- only a complete slot is a branch.

The film and the ray count are the CPU oracle's byte for byte, through the three fused forms (one sample group, several groups, head + tail),
on the scenes and parameters where that control flow has its edges: passes that are nearly all misses, an environment with zero components, paths
that end at their first hit, slots of one sample, the miss record at index 1 and at the end of the largest table the plan admits.
"""
import numpy as np
import pytest

W, H = 64, 48
NONE = 0xFFFFFFFF
# the three forms of the fused pipeline: (pt_tuning, params).  fused_tail = 3 of 4 samples: the head slot is ONE sample (head_samples at its edge)
FORMS = {"one_group": (dict(fused_tail=0), dict(sample_groups=1)),
         "groups": (dict(fused_tail=0), dict(sample_groups=4)),
         "head_tail": (dict(fused_tail=3), dict())}
# the quad of the scenes below lies in z = 0; from here it is seen at a flat angle: half the image and most bounces see the environment
SIDE = dict(cam_origin=(2.6, 0.4, 0.9), cam_target=(0.0, 0.0, 0.0))
FRONT = dict(cam_origin=(0.05, 0.1, 3.0), cam_target=(0.0, 0.0, 0.0))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _faces(n_tris, emit=()):
    f = np.zeros((n_tris, 6), np.float32)
    k = np.arange(n_tris)
    f[:, 0], f[:, 1], f[:, 2] = 0.3 + 0.1 * (k % 5), 0.8 - 0.1 * (k % 7), 0.4 + 0.05 * (k % 9)
    for t in emit:
        f[t, 3:6] = (4.0, 3.0, 2.0)
    return f.reshape(-1)


def one_quad(emit=(0, 1)):
    v = np.float32([[-0.8, -0.6, 0.0], [0.8, -0.6, 0.0], [0.8, 0.6, 0.0], [-0.8, 0.6, 0.0]])
    return v.reshape(-1), np.uint32([0, 1, 2, 0, 2, 3]), _faces(2, emit)


def one_triangle():
    v = np.float32([[-0.9, -0.7, 0.0], [0.9, -0.6, 0.0], [0.1, 0.8, 0.0]])
    return v.reshape(-1), np.uint32([0, 1, 2]), _faces(1, emit=(0,))


def soup(n, seed=5):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3))
    v = (c + rng.uniform(-0.25, 0.25, (n, 3, 3))).astype(np.float32)
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), _faces(n, emit=(0, n - 1))


# ---- the oracle's answer, once per (scene, parameters) ---------------------------------------------------------------------------------
_want = {}


def oracle(orc, name, arrays, frames, **kw):
    """-> (film f32 after `frames` frames, rays, first hits of the camera rays of frame 0's first sample); read-only, shared"""
    key = (name, frames, tuple(sorted(kw.items())))
    if key not in _want:
        osc = orc.Scene(*arrays)
        film, rays, first = np.zeros((H, W, 3), np.float32), 0, None
        for k in range(frames):
            img, r, _, fh = osc.render_frame(orc.default_params(frame=k, width=W, height=H, **kw), want_first_hits=(k == 0))
            orc.accumulate_f32(film, img, k)
            rays += r
            if k == 0:
                first = fh["prim"].copy()
                first.setflags(write=False)
        film.setflags(write=False)
        _want[key] = (film, rays, first)
    return _want[key]


def render(pt, ctx, sc, form, frames, flags=0, extend=None, tuning=None, **kw):
    tune, params = FORMS[form]
    film = pt.Film(ctx, W, H)
    old = ctx.set_tuning(**dict(tune, **(tuning or {})))
    try:
        ctx.reset_stats()
        pt.render(sc, film, pt.default_params(frame=0, frame_count=frames, width=W, height=H, pipeline=pt.PIPELINE_FUSED, flags=flags,
                                              **({} if extend is None else dict(extend=extend)), **params, **kw))
        return film.read_f32(), ctx.stats()
    finally:
        ctx.set_tuning(**old)
        film.close()


def check(pt, orc, ctx, sc, name, arrays, form, frames=2, extend=None, **kw):
    want, rays, _ = oracle(orc, name, arrays, frames, **kw)
    got, st = render(pt, ctx, sc, form, frames, extend=extend, **kw)
    assert st.pipeline == pt.PIPELINE_FUSED and st.extend_variant == pt.EXTEND_LDS, (name, form, st.pipeline, st.extend_variant)
    assert st.rays == rays, (name, form, st.rays, rays)
    assert got.tobytes() == want.tobytes(), (name, form, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    return got, st


# ---- without a GPU: the identity the vote-free `color +=` rests on ---------------------------------------------------------------------
def test_adding_a_zero_keeps_the_bits_of_every_accumulator_that_is_not_minus_zero():
    """An accumulator starts at +0 and only ever receives sums.  x + (+0) and x + (-0) keep x's bits for every x but -0, and a sum of two
    values is -0 only for (-0) + (-0): so an accumulator is never -0 and adding a term of +-0 to it is the same film as skipping the add."""
    u32, f32 = np.uint32, np.float32
    rng = np.random.default_rng(1)
    bits = np.concatenate([
        u32([0x00000000, 0x00000001, 0x00000002, 0x007FFFFF, 0x00400000, 0x00800000, 0x00800001, 0x7F7FFFFF, 0x7F800000, 0xFF800000,   # +0, subnormals, min normal, max, +-inf
             0x80000001, 0x807FFFFF, 0x80800000, 0xFF7FFFFF, 0x3F800000, 0xBF800000,
             0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7FFFFFFF, 0xFFC12345, 0x7FD55555]),                                                 # quiet NaNs with payloads
        rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(u32),
        rng.integers(0, 1 << 23, 40, dtype=np.uint64).astype(u32),                                                                   # more subnormals
        (rng.integers(0, 1 << 23, 40, dtype=np.uint64) | 0x80000000).astype(u32)])
    # (signalling NaNs are quieted by any arithmetic, here as on the GPU: the kernel's accumulator never holds one, a sum is never signalling)
    snan = ((bits & u32(0x7F800000)) == u32(0x7F800000)) & ((bits & u32(0x007FFFFF)) != 0) & ((bits & u32(0x00400000)) == 0)
    bits = bits[~snan & (bits != u32(0x80000000))]
    assert len(bits) > 300 and (bits == 0).any() and (bits == u32(0x7F800000)).any() and (bits == u32(0xFF800000)).any()
    x = bits.view(f32)
    with np.errstate(all="ignore"):
        for zero in (u32([0x00000000]), u32([0x80000000])):
            got = (x + zero.view(f32)).view(u32)
            assert (got == bits).all(), [(hex(int(b)), hex(int(g))) for b, g in zip(bits, got) if b != g][:4]
        # a sum is -0 only for (-0) + (-0): every pair of a set that holds +-0, the smallest and the largest values of either sign, and ordinary ones
        pool = np.concatenate([u32([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000]),
                               bits[:120]])
        a, b = np.meshgrid(pool, pool)
        s = (a.view(f32) + b.view(f32)).view(u32)
        minus_zero = s == u32(0x80000000)
        assert minus_zero.sum() == 1 and (a[minus_zero] == u32(0x80000000)).all() and (b[minus_zero] == u32(0x80000000)).all()
        # x + (-x) is +0 (round to nearest), not -0
        fin = pool[np.isfinite(pool.view(f32))]
        assert ((fin.view(f32) + (fin ^ u32(0x80000000)).view(f32)).view(u32) == 0).all()


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_misses_everywhere_env_with_a_zero_component(pt, orc, gpu_ctx, form):
    """one quad seen from the side: about half the camera rays and most bounces miss -- passes of the shade block that are nearly all record
    n_tris -- under an environment whose green is zero (a term of +0 in every miss), with the cull of pixels that cannot see the quad and without"""
    arrays = one_quad()
    kw = dict(spp_per_frame=4, max_depth=8, env=(0.7, 0.0, 1.3), **SIDE)
    _, _, first = oracle(orc, "quad_side", arrays, 2, **kw)
    share = float((first == NONE).mean())
    assert 0.3 <= share <= 0.75, share   # (the camera does what it is there for)
    sc = pt.Scene(gpu_ctx, *arrays)
    try:
        for cull in (0, 1):
            got, _ = check_with_cull(pt, orc, gpu_ctx, sc, "quad_side", arrays, form, cull, **kw)
            assert (got[..., 1] != 0).any() and (got[..., 1] == 0).any()   # (green: from the emitter only)
    finally:
        sc.close()


def check_with_cull(pt, orc, ctx, sc, name, arrays, form, cull, frames=2, **kw):
    want, rays, _ = oracle(orc, name, arrays, frames, **kw)
    got, st = render(pt, ctx, sc, form, frames, tuning=dict(cull=cull), **kw)
    assert st.pipeline == pt.PIPELINE_FUSED and st.rays == rays, (name, form, cull, st.pipeline, st.rays, rays)
    assert cull == 1 or st.rays_culled == 0, (name, form, st.rays_culled)
    assert got.tobytes() == want.tobytes(), (name, form, cull, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    return got, st


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_black_environment_and_no_emitter_is_a_film_of_plus_zero(pt, orc, gpu_ctx, form):
    """the same view with env = (0, 0, 0) and no emitter: every term is +0 or 0 * weight; the film is the oracle's and holds nothing but the bit
    pattern of +0.0f -- no accumulator turned -0 where every lane adds its term"""
    arrays = one_quad(emit=())
    kw = dict(spp_per_frame=4, max_depth=8, env=(0.0, 0.0, 0.0), **SIDE)
    sc = pt.Scene(gpu_ctx, *arrays)
    try:
        for cull in (0, 1):
            got, _ = check_with_cull(pt, orc, gpu_ctx, sc, "quad_black", arrays, form, cull, **kw)
            assert not got.view(np.uint32).any(), np.unique(got.view(np.uint32))[:4]
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("edge", ["depth1", "spp1", "depth1_spp1"])
def test_paths_of_one_hit_and_slots_of_one_sample(pt, orc, gpu_ctx, cornell_gpu, cornell_arrays, form, edge):
    """max_depth = 1: every hit ends its path by depth, every miss by the miss -- no lane of a pass bounces.  spp_per_frame = 1: a slot is complete
    at its first ended path (the slot's store straight from the select form); with head + tail slots of four samples the head is one sample."""
    kw = dict(spp_per_frame=1 if "spp1" in edge else 4, max_depth=1 if "depth1" in edge else 8)
    _, st = check(pt, orc, gpu_ctx, cornell_gpu, "cornell", cornell_arrays, form, **kw)
    if "depth1" in edge:
        assert st.rays == 2 * W * H * kw["spp_per_frame"]   # (one ray per sample)
    if form == "head_tail":
        assert st.tail_samples == (3 if kw["spp_per_frame"] == 4 else 0), st.tail_samples


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_miss_record_behind_a_table_of_one_triangle(pt, orc, gpu_ctx, form):
    """n_tris = 1: the miss is record 1, right behind the only triangle's"""
    arrays = one_triangle()
    kw = dict(spp_per_frame=4, max_depth=8, env=(0.25, 0.5, 0.0), **FRONT)
    _, _, first = oracle(orc, "one_triangle", arrays, 2, **kw)
    assert (first == NONE).any() and (first == 0).any()
    sc = pt.Scene(gpu_ctx, *arrays)
    try:
        assert sc.info().n_tris == 1
        check(pt, orc, gpu_ctx, sc, "one_triangle", arrays, form, **kw)
    finally:
        sc.close()


LARGEST = 204   # 5 float4 of shading tables per triangle: 5 * 16 * 204 = 16 320 B <= 16 KB


@pytest.fixture(scope="module")
def largest_scene(pt, gpu_ctx):
    """the biggest soup the fused plan takes (tables <= 16 KB; its triangle copies are past the 24 KB of PT_EXTEND_AUTO's class, so the LDS walk is
    named): searched downward from the table limit, so that a change to the builder moves the scene and not the verdict"""
    found = None
    for n in range(LARGEST, LARGEST - 40, -1):
        arrays = soup(n)
        sc = pt.Scene(gpu_ctx, *arrays)
        try:
            render(pt, gpu_ctx, sc, "one_group", 1, extend=pt.EXTEND_LDS, spp_per_frame=1, max_depth=1, **FRONT)
            found = (n, arrays, sc)
            break
        except pt.PtError:
            sc.close()
    assert found is not None, "no soup of 165 .. 204 triangles is planned by PT_PIPELINE_FUSED"
    print("largest scene of the fused plan:", found[0], "triangles")
    yield found
    found[2].close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_miss_record_behind_the_largest_table(pt, orc, gpu_ctx, largest_scene, form):
    """the miss record at the far end of the class: behind the shade table of the largest scene PT_PIPELINE_FUSED plans, with hits and misses both"""
    n, arrays, sc = largest_scene
    assert 5 * 16 * n <= 16 * 1024 and sc.info().n_tris == n
    kw = dict(spp_per_frame=2, max_depth=8, env=(0.7, 0.0, 1.3), **FRONT)
    _, _, first = oracle(orc, f"soup{n}", arrays, 2, **kw)
    n_miss, n_hit = int((first == NONE).sum()), int((first != NONE).sum())
    assert n_miss > 0 and n_hit > 0, (n_miss, n_hit)
    check(pt, orc, gpu_ctx, sc, f"soup{n}", arrays, form, extend=pt.EXTEND_LDS, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_instrumented_twin_still_counts_misses_and_surface_hits(pt, orc, gpu_ctx, form):
    """PT_FLAG_COUNT_VISITS: the product kernel has no miss block any more, its twin still counts the miss lanes and the surface lanes of step (1).
    General render: same film, MISS = walked rays - SURFACE lanes, both present.  One sample of depth 1 of frame 0: every walked ray is a camera
    ray, so the miss lanes are the misses of the oracle's first-hit list less the culled rays (which are misses that were never walked)."""
    arrays = one_quad()
    sc = pt.Scene(gpu_ctx, *arrays)
    try:
        kw = dict(spp_per_frame=4, max_depth=8, env=(0.7, 0.0, 1.3), **SIDE)
        want, rays, _ = oracle(orc, "quad_side", arrays, 2, **kw)
        got, st = render(pt, gpu_ctx, sc, form, 2, flags=pt.FLAG_COUNT_VISITS, tuning=dict(cull=1), **kw)
        bc = gpu_ctx.block_counts()
        walked = st.rays - st.rays_culled
        assert got.tobytes() == want.tobytes() and st.rays == rays
        assert bc["HIT"][1] == walked and bc["MISS"][1] == walked - bc["SURFACE"][1], (form, bc, walked)
        assert bc["MISS"][1] > 0 and bc["SURFACE"][1] > 0 and bc["NEXT"][1] >= bc["MISS"][1]

        kw1 = dict(spp_per_frame=1, max_depth=1, env=(0.7, 0.0, 1.3), **SIDE)
        want, rays, first = oracle(orc, "quad_side", arrays, 1, **kw1)
        for cull in (0, 1):
            got, st = render(pt, gpu_ctx, sc, form, 1, flags=pt.FLAG_COUNT_VISITS, tuning=dict(cull=cull), **kw1)
            bc = gpu_ctx.block_counts()
            assert got.tobytes() == want.tobytes() and st.rays == rays == W * H
            misses = int((first == NONE).sum())
            assert bc["MISS"][1] == misses - st.rays_culled and bc["SURFACE"][1] == W * H - misses, (form, cull, bc["MISS"], bc["SURFACE"], misses, st.rays_culled)
            assert bc["NEXT"][1] == W * H - st.rays_culled and bc["DONE"][1] == W * H - st.rays_culled
    finally:
        sc.close()
