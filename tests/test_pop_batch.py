"""k_fused's pop loop on the GPU (csrc/fused_kernel.h pop_pending, csrc/pop_batch.h): a pop takes the first entry from the top that is within
the cut key and is not the lane's own leaf, the entries above it are gone, the BOTTOM entry ends the search.  Film and ray count bit for bit
against the CPU oracle at 32 x 32, 2 spp, depth 4, 2 frames, on the scenes where a pop that looks at several entries per pass could part from
the one-entry loop:

  chain        the nested-quad chain of tests/test_cut_key.py (stack bound 16): runs of rejected entries across several node steps' groups
  triangle     one triangle: BOTTOM is the first entry, and whatever a pass reads with it lies below the stack
  coincident   the same quad twice: entries whose key IS the cut's must survive
  box          a closed box of six quads, one of them an emitter, the camera inside: every bounce ray starts on a wall whose own leaf is among
               the entries its pops look at

through every fused kernel that has the loop: one sample group, several groups, head + tail slots, the tree without pair leaves, PT_FLAG_NEE,
pt_render_guided's kernels with the first-hit log, and the instrumented twin -- which also has to report the node and triangle counts of the
wavefront pipeline's instrumented kernel: the visit order is the same walk.  tests/test_pop_batch_cpu.py has the selection itself.
"""
import numpy as np
import pytest

import test_cut_key as ck

W = H = ck.W
KW = ck.KW
FRAMES = ck.FRAMES
CAM_BOX = dict(cam_origin=(0.15, 0.1, 0.6), cam_target=(-0.1, -0.05, -1.0))
FORMS = {"one_group": (dict(fused_tail=0), dict(sample_groups=1)),
         "groups": (dict(fused_tail=0), dict(sample_groups=2)),
         "head_tail": (dict(fused_tail=1), dict())}
SCENES = ("chain", "triangle", "coincident", "box")


def closed_box():
    """six quads of the cube [-1, 1]^3 (twelve triangles, six pair leaves, more than one node), wound so that a bounce leaves a wall towards
    the inside; the ceiling emits"""
    c = np.float32([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]])
    quads = [c[[3, 2, 1, 0]], c[[6, 7, 4, 5]], c[[7, 3, 0, 4]], c[[2, 6, 5, 1]], c[[0, 1, 5, 4]], c[[7, 6, 2, 3]]]
    return ck._quads(quads, emit=(10, 11))


_chain_n = {}


def scene_arrays(pt, ctx, name):
    """-> (arrays, camera); the chain's length is the one that gives the builder's tree the stack bound 16 (looked for once)"""
    if name == "triangle":
        return ck.one_triangle(), ck.CAM_Z
    if name == "coincident":
        return ck.coincident_quads(), ck.CAM_Z
    if name == "box":
        return closed_box(), CAM_BOX
    if "n" not in _chain_n:
        for n in [ck.CHAIN_N] + [m for m in range(12, 28) if m != ck.CHAIN_N]:
            sc = pt.Scene(ctx, *ck.chain(n))
            try:
                if ck.stack_need(sc.read_bvh4()) == 16:
                    _chain_n["n"] = n
                    break
            finally:
                sc.close()
        assert "n" in _chain_n, "no chain of 12 .. 27 nested quads gives the builder's tree the stack bound 16"
    return ck.chain(_chain_n["n"]), ck.CAM_CONE


_scenes = {}


@pytest.fixture
def scene(request, pt, gpu_ctx):
    """-> (name, arrays, camera, the GPU scene): built once per (scene, tree kind) and shared"""
    def get(name, pairs=True):
        key = (name, pairs)
        if key not in _scenes:
            arrays, cam = scene_arrays(pt, gpu_ctx, name)
            old = gpu_ctx.set_tuning(pair_leaves=-1 if pairs else 0)
            try:
                _scenes[key] = (arrays, cam, pt.Scene(gpu_ctx, *arrays))
            finally:
                gpu_ctx.set_tuning(**old)
        return (name,) + _scenes[key]
    return get


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for _, _, sc in _scenes.values():
        sc.close()
    _scenes.clear()


def render(pt, ctx, sc, pipeline, form="one_group", flags=0, **kw):
    tune, params = FORMS[form]
    film = pt.Film(ctx, W, H)
    old = ctx.set_tuning(**tune)
    try:
        ctx.reset_stats()
        pt.render(sc, film, pt.default_params(frame=0, frame_count=FRAMES, pipeline=pipeline, flags=flags, **KW, **params, **kw))
        return film.read_f32(), ctx.stats()
    finally:
        ctx.set_tuning(**old)
        film.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", SCENES)
def test_three_forms(pt, orc, gpu_ctx, scene, name, form):
    name, arrays, cam, sc = scene(name)
    want, rays = ck.oracle_film(orc, name, arrays, **cam)
    got, st = render(pt, gpu_ctx, sc, pt.PIPELINE_FUSED, form, **cam)
    assert st.pipeline == pt.PIPELINE_FUSED and st.extend_variant == pt.EXTEND_LDS, (name, form, st.pipeline, st.extend_variant)
    assert (st.sample_groups, st.tail_samples) == {"one_group": (1, 0), "groups": (2, 0), "head_tail": (st.sample_groups, 1)}[form], (form, st.sample_groups, st.tail_samples)
    assert st.rays == rays, (name, form, st.rays, rays)
    assert got.tobytes() == want.tobytes(), (name, form, int((got != want).sum()))
    assert want.any()
    if name == "box":
        # (closed: no bounce ray misses.  Even if every hit on the ceiling -- a sixth of the walls -- ended its path, a path of depth 4 would
        # have 1 + 5/6 + 25/36 + 125/216 = 3.1 rays)
        assert 2 * rays > 5 * W * H * KW["spp_per_frame"] * FRAMES, rays


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", SCENES)
def test_tree_without_pair_leaves(pt, orc, gpu_ctx, scene, name, form):
    """leaves of up to four triangles: the kernels with PAIRS = false, which have no own-leaf rule"""
    name, arrays, cam, sc = scene(name, pairs=False)
    want, rays = ck.oracle_film(orc, name, arrays, **cam)
    got, st = render(pt, gpu_ctx, sc, pt.PIPELINE_FUSED, form, **cam)
    assert st.pipeline == pt.PIPELINE_FUSED and st.rays == rays, (name, form, st.pipeline, st.rays, rays)
    assert got.tobytes() == want.tobytes(), (name, form, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("pairs", [True, False], ids=["pair_leaves", "leaves_of_four"])
@pytest.mark.parametrize("name", SCENES)
def test_nee(pt, orc, gpu_ctx, scene, name, pairs):
    """k_fused_nee: shadow rays pop too, and a hit of theirs clears the stack down to BOTTOM"""
    name, arrays, cam, sc = scene(name, pairs=pairs)
    want, rays = ck.oracle_film(orc, name, arrays, nee=1, **cam)
    got, st = render(pt, gpu_ctx, sc, pt.PIPELINE_FUSED, "one_group", flags=pt.FLAG_NEE, **cam)
    assert st.pipeline == pt.PIPELINE_FUSED and st.rays == rays, (name, st.pipeline, st.rays, rays)
    assert got.tobytes() == want.tobytes(), (name, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", SCENES)
def test_render_guided(pt, orc, gpu_ctx, scene, name, form):
    """the kernels with the first-hit log (pt_render_guided's single pass)"""
    name, arrays, cam, sc = scene(name)
    want, rays = ck.oracle_film(orc, name, arrays, **cam)
    tune, params = FORMS[form]
    film = pt.Film(gpu_ctx, W, H)
    old = gpu_ctx.set_tuning(**tune)
    try:
        film.enable_aov()
        gpu_ctx.reset_stats()
        res = pt.render_guided(sc, film, pt.default_params(frame=0, frame_count=FRAMES, pipeline=pt.PIPELINE_FUSED, **KW, **params, **cam),
                               mode=pt.GUIDED_SINGLE_PASS)
        assert res.single_pass == 1 and gpu_ctx.stats().rays == rays, (name, form, gpu_ctx.stats().rays, rays)
        assert film.read_f32().tobytes() == want.tobytes(), (name, form)
    finally:
        gpu_ctx.set_tuning(**old)
        film.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["one_group", "head_tail"])
@pytest.mark.parametrize("name", SCENES)
def test_instrumented_twin(pt, orc, gpu_ctx, scene, name, form):
    """PT_FLAG_COUNT_VISITS: the same film, and the node and triangle counts of the wavefront pipeline's instrumented kernel -- the pops hand
    out the same entries in the same order, whatever they read per pass"""
    name, arrays, cam, sc = scene(name)
    want, rays = ck.oracle_film(orc, name, arrays, **cam)
    got, st = render(pt, gpu_ctx, sc, pt.PIPELINE_FUSED, form, flags=pt.FLAG_COUNT_VISITS, **cam)
    bc = gpu_ctx.block_counts()
    assert st.pipeline == pt.PIPELINE_FUSED and st.rays == rays and got.tobytes() == want.tobytes(), (name, form)
    ref, rst = render(pt, gpu_ctx, sc, pt.PIPELINE_WAVEFRONT, "one_group", flags=pt.FLAG_COUNT_VISITS, **cam)
    assert rst.rays == rays and ref.tobytes() == want.tobytes(), name
    # (the twin reports its walk as block counts: the lanes of NODE are its node visits; the lanes of LEAF its leaf steps, to which the wavefront
    # kernel, which has no own-leaf rule, adds the leaves that the fused walk passed over -- the lanes of SKIP.  Every leaf of these scenes is a
    # fan pair except the lone triangle, so the wavefront kernel's triangle count is twice -- there once -- its leaf steps.)
    per_leaf = 1 if name == "triangle" else 2
    print(name, form, "NODE", bc["NODE"], "LEAF", bc["LEAF"], "SKIP", bc["SKIP"], "POP", bc["POP"], "POPTOP", bc["POPTOP"],
          "wavefront nodes", rst.nodes_visited, "tris", rst.tris_tested, "leaf lanes", rst.leaf_lanes)
    assert rst.nodes_visited > 0 and rst.tris_tested > 0 and bc["POP"][0] > 0
    assert bc["NODE"][1] == rst.nodes_visited, (name, form, bc["NODE"], rst.nodes_visited)
    assert per_leaf * (bc["LEAF"][1] + bc["SKIP"][1]) == rst.tris_tested, (name, form, bc["LEAF"], bc["SKIP"], rst.tris_tested)
