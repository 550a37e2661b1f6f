"""k_fused declares the shade block's path state, the camera ray's target and the reset of the hit record without a fill (ptm::undef, pt_math.h:
an empty asm's output -- a register as it happens to be).  That is right only if no lane reads such a value before a step has written it.

The poison twin: the library built once more from a copy of csrc/ with -DPT_UNDEF_POISON, where ptm::undef returns a quiet NaN (floats) or
0xDEADBEEF (integers, a wild slot index) instead -- a value that leaks shows in a film, an image, a ray count or a guide plane, not as a lucky
zero.  A child process renders every case below through that library (PT_LIB_AMD); the product library renders them here.  For every case the
two agree byte for byte, and both agree with PT_PIPELINE_WAVEFRONT of the same calls; the smallest ones are also held against the CPU oracle.

The shapes are the smallest at which a stale register can reach memory: images of 8x8 and 20x12 pixels (one tile; six tiles with lanes outside
the image -- a block's waves never all own a path), 1 and 3 samples, paths of 1, 2 and 8 rays, 1 - 3 frames per call, each of the kernel's three
forms, the cull on and off, a camera whose rays all miss (no accept ever writes the hit record), the first-hit log, NEE, the instrumented twin,
a scene of one triangle and the trees with leaves of up to four triangles.
"""
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "single-file-vulkan-pathtracing_amd"
SIZES = [(8, 8), (20, 12)]
# (pt_tuning, params) per form of the kernel; spp -> the values that force it (several groups: one sample each; head + tail: a head of one sample)
FORMS = {"one_group": lambda spp: (dict(fused_tail=0), dict(sample_groups=1)),
         "groups": lambda spp: (dict(fused_tail=0), dict(sample_groups=spp)),
         "head_tail": lambda spp: (dict(fused_tail=spp - 1), dict())}
# the box lies around the origin (|x|, |z| <= 1, 0 <= y <= 2): from here, looking away from it, every camera ray misses
AWAY = dict(cam_origin=(0.0, 1.0, 50.0), cam_target=(0.0, 1.0, 100.0))
ENV = dict(env=(0.25, 0.5, 0.75))


def one_triangle():
    v = np.float32([[-0.9, -0.7, 0.0], [0.9, -0.6, 0.0], [0.1, 0.8, 0.0]])
    f = np.float32([[0.6, 0.5, 0.4, 4.0, 3.0, 2.0]])
    return v.reshape(-1), np.uint32([0, 1, 2]), f.reshape(-1)


FRONT = dict(cam_origin=(0.05, 0.1, 3.0), cam_target=(0.0, 0.0, 0.0))


# ---- the cases: id -> spec.  A spec is plain data, so that the child process builds the same list ---------------------------------------------------
def grid(size, form):
    """every (spp, depth, frames per call, cull) of one image size and one form of the kernel"""
    out = {}
    for spp in (1, 3):
        if form != "one_group" and spp == 1:
            continue   # (several groups and a head + tail split need more than one sample)
        tune, params = FORMS[form](spp)
        for depth in (1, 2, 8):
            for frames in (1, 2, 3):
                for cull in (0, 1):
                    out[f"{size[0]}x{size[1]}-{form}-spp{spp}-d{depth}-f{frames}-cull{cull}"] = dict(
                        scene="cornell", size=size, spp=spp, depth=depth, tuning=dict(tune, cull=cull), params=params, calls=[dict(frames=frames)], form=form)
    return out


def specials():
    out = {}
    for form in FORMS:
        tune, params = FORMS[form](3)
        base = dict(scene="cornell", size=(20, 12), spp=3, depth=8, tuning=dict(tune, cull=0), params=dict(params, **ENV), form=form)
        # every ray misses; then, in the same context and film, a camera that sees the box
        out[f"sees_nothing-{form}"] = dict(base, calls=[dict(frames=2, **AWAY)], all_miss=True)
        out[f"sees_nothing_then_the_box-{form}"] = dict(base, calls=[dict(frames=1, **AWAY), dict(frames=2)])
        # the trees with leaves of up to four triangles (k_fused<., false>) and a scene of one triangle
        out[f"leaves_of_four-{form}"] = dict(scene="cornell_leaves4", size=(20, 12), spp=3, depth=8, tuning=dict(tune, cull=1), params=params,
                                            calls=[dict(frames=2)], form=form)
        out[f"one_triangle-{form}"] = dict(scene="one_triangle", size=(20, 12), spp=3, depth=8, tuning=dict(tune, cull=1), params=dict(params, **ENV, **FRONT),
                                          calls=[dict(frames=2)], form=form)
    one = FORMS["one_group"](1)
    out["guided-8x8"] = dict(scene="cornell", size=(8, 8), spp=1, depth=8, tuning=dict(one[0]), params=dict(one[1]), calls=[dict(frames=2)], guided=True, form="one_group")
    for size in SIZES:
        for depth in (1, 8):
            out[f"nee-{size[0]}x{size[1]}-d{depth}"] = dict(scene="cornell", size=size, spp=3, depth=depth, tuning={}, params={}, calls=[dict(frames=2)], nee=True)
    for form in FORMS:
        tune, params = FORMS[form](3)
        out[f"count_visits-{form}"] = dict(scene="cornell", size=(20, 12), spp=3, depth=8, tuning=dict(tune, cull=1), params=params, calls=[dict(frames=2)],
                                          count=True, form=form)
    return out


def all_cases():
    out = {}
    for size in SIZES:
        for form in FORMS:
            out.update(grid(size, form))
    out.update(specials())
    return out


# ---- one case through one library ---------------------------------------------------------------------------------------------------------------
class Scenes:
    """the scenes of the cases in one context, built when first asked for"""

    def __init__(self, mod, ctx):
        self.mod, self.ctx, self.made = mod, ctx, {}

    def get(self, name):
        if name not in self.made:
            mod, ctx = self.mod, self.ctx
            if name == "one_triangle":
                self.made[name] = mod.Scene(ctx, *one_triangle())
            else:
                old = ctx.set_tuning(pair_leaves=0 if name == "cornell_leaves4" else -1)
                try:
                    self.made[name] = mod.Scene(ctx, *mod.load_obj(mod.ASSET_CORNELL))
                finally:
                    ctx.set_tuning(**old)
        return self.made[name]

    def close(self):
        for sc in self.made.values():
            sc.close()


def run(mod, ctx, scenes, spec, fused):
    """-> {name: array} of the case's calls: through PT_PIPELINE_FUSED, or through the wavefront pipeline (the same calls without the fused kernel)"""
    w, h = spec["size"]
    sc = scenes.get(spec["scene"])
    film = mod.Film(ctx, w, h)
    if spec.get("guided"):
        film.enable_aov()
    flags = (mod.FLAG_NEE if spec.get("nee") else 0) | (mod.FLAG_COUNT_VISITS if spec.get("count") and fused else 0)
    old = ctx.set_tuning(**spec["tuning"])
    try:
        ctx.reset_stats()
        frame, single = 0, 1
        for call in spec["calls"]:
            kw = dict(call)
            n = kw.pop("frames")
            p = mod.default_params(frame=frame, frame_count=n, width=w, height=h, spp_per_frame=spec["spp"], max_depth=spec["depth"], flags=flags,
                                   pipeline=mod.PIPELINE_FUSED if fused else mod.PIPELINE_WAVEFRONT, **spec["params"], **kw)
            if spec.get("guided"):
                res = mod.render_guided(sc, film, p, mode=mod.GUIDED_SINGLE_PASS if fused else mod.GUIDED_AUTO)
                single &= int(res.single_pass)
            else:
                mod.render(sc, film, p)
            frame += n
        st = ctx.stats()
        out = {"film": film.read_f32(), "bgra8": film.read_bgra8(),
               "stats": np.uint64([st.rays, st.pipeline, st.sample_groups, st.tail_samples, st.rays_culled, single])}
        if spec.get("guided"):
            for a in range(mod.AOV_COUNT):
                out[f"aov{a}"] = film.read_aov(a)
        return out
    finally:
        ctx.set_tuning(**old)
        film.close()


def twin_main(out_path):
    """the child process: every case through the library PT_LIB_AMD names"""
    sys.path.insert(0, REPO)
    mod = importlib.import_module(PKG)
    assert os.environ.get("PT_LIB_AMD") and os.path.exists(os.environ["PT_LIB_AMD"])
    ctx = mod.Context(0)
    scenes = Scenes(mod, ctx)
    got = {}
    for cid, spec in all_cases().items():
        for k, v in run(mod, ctx, scenes, spec, True).items():
            got[f"{cid}/{k}"] = v
    scenes.close()
    ctx.close()
    np.savez(out_path, **got)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def poison_twin(pt, tmp_path_factory):
    """{case/name: array} of every case through the poison build: csrc/ copied (sources only), built with EXTRA=-DPT_UNDEF_POISON, rendered by a
    child process of its own"""
    root = tmp_path_factory.mktemp("poison_twin")
    pkg = os.path.join(REPO, PKG)
    shutil.copytree(os.path.join(pkg, "csrc"), root / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.s", "*.so"))
    shutil.copytree(os.path.join(REPO, "include"), root / "include")   # (csrc/Makefile names ../../include/pt_api.h)
    subprocess.run(["make", "-C", str(root / "pkg" / "csrc"), "-j16", "EXTRA=-DPT_UNDEF_POISON"], check=True, stdout=subprocess.DEVNULL)
    lib = root / "pkg" / "libpt_amd.so"
    # (the twin is the poison build and the product is not: the float pattern as a literal of the device code, little-endian)
    pattern = bytes.fromhex("addec07f")
    assert pattern in lib.read_bytes() and pattern not in open(os.path.join(pkg, "libpt_amd.so"), "rb").read()
    out = root / "twin.npz"
    env = dict(os.environ, PT_LIB_AMD=str(lib), PYTHONNOUSERSITE="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--twin", str(out)], check=True, env=env, cwd=REPO)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="session")
def undef_scenes(pt, gpu_ctx):
    s = Scenes(pt, gpu_ctx)
    yield s
    s.close()


def same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k, int((a[k] != b[k]).sum()))


def check(pt, gpu_ctx, scenes, twin, cid, spec):
    """product == poison twin == wavefront; -> the product's arrays"""
    got = run(pt, gpu_ctx, scenes, spec, True)
    tw = {k.split("/", 1)[1]: v for k, v in twin.items() if k.startswith(cid + "/")}
    assert tw, cid
    rays, pipeline, groups, tail, culled, single = (int(x) for x in got["stats"])
    assert pipeline == pt.PIPELINE_FUSED and single == 1, (cid, pipeline, single)
    # the form the case is there for did render (MODE 0 / 1 / 2 of k_fused)
    form = spec.get("form")
    if form == "one_group":
        assert groups == 1 and tail == 0, (cid, groups, tail)
    elif form == "groups":
        assert groups == spec["spp"] and tail == 0, (cid, groups, tail)
    elif form == "head_tail":
        assert groups == 1 and tail == spec["spp"] - 1, (cid, groups, tail)
    same(got, tw, (cid, "product / poison twin"))
    ref = run(pt, gpu_ctx, scenes, spec, False)
    for k in got:
        if k != "stats":
            assert got[k].tobytes() == ref[k].tobytes(), (cid, "fused / wavefront", k)
    # (the guides of the wavefront pipeline come from a second walk of the camera rays, which the single pass does not make)
    again = sum(c["frames"] for c in spec["calls"]) * spec["size"][0] * spec["size"][1] * spec["spp"] if spec.get("guided") else 0
    assert rays + again == int(ref["stats"][0]), (cid, rays, again, int(ref["stats"][0]))
    return got


# ---- the tests --------------------------------------------------------------------------------------------------------------------------------
def test_cases_are_the_ones_the_change_needs():
    """(without a GPU) the list holds every axis: both sizes, spp 1 and 3, depths 1 / 2 / 8, 1 - 3 frames, the three forms, cull on and off"""
    c = all_cases()
    g = [s for s in c.values() if "all_miss" not in s and s["scene"] == "cornell" and not s.get("guided") and not s.get("nee") and not s.get("count")]
    assert {tuple(s["size"]) for s in g} == set(SIZES) and {s["spp"] for s in g} == {1, 3} and {s["depth"] for s in g} == {1, 2, 8}
    assert {s["calls"][0]["frames"] for s in g} >= {1, 2, 3} and {s["tuning"]["cull"] for s in g} == {0, 1} and {s["form"] for s in g} == set(FORMS)
    assert any(s.get("guided") and tuple(s["size"]) == (8, 8) and s["spp"] == 1 for s in c.values())
    assert any(s.get("nee") and tuple(s["size"]) == (8, 8) for s in c.values()) and any(s.get("count") for s in c.values())
    assert {s["scene"] for s in c.values()} == {"cornell", "cornell_leaves4", "one_triangle"}


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_poison_twin_renders_the_same_small_images(pt, orc, gpu_ctx, undef_scenes, cornell_oracle, poison_twin, size, form):
    """8x8 and 20x12, spp 1 and 3, depth 1 / 2 / 8, 1 - 3 frames per call, cull off and on, per form of the kernel: product == poison twin ==
    wavefront in film, rgba8 image and ray count; the one-frame cases also equal the oracle"""
    for cid, spec in grid(size, form).items():
        got = check(pt, gpu_ctx, undef_scenes, poison_twin, cid, spec)
        if spec["calls"][0]["frames"] == 1 and spec["tuning"]["cull"] == 0:
            w, h = size
            img, rays, _, _ = cornell_oracle.render_frame(orc.default_params(frame=0, width=w, height=h, spp_per_frame=spec["spp"], max_depth=spec["depth"]))
            film, bgra = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 4), np.uint8)
            orc.accumulate_f32(film, img, 0)
            orc.accumulate_bgra8(bgra, img, 0)
            assert int(got["stats"][0]) == rays and got["film"].tobytes() == film.tobytes() and got["bgra8"].tobytes() == bgra.tobytes(), cid


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_a_camera_that_sees_nothing_then_one_that_sees_the_box(pt, gpu_ctx, undef_scenes, poison_twin, form):
    """cull = 0 and every ray a miss: no accept writes best_V / best_W / best_det, and a miss never reads them -- a film of the environment, one ray
    per sample; then the same call followed by frames of the usual camera, in the same context and film"""
    cid = f"sees_nothing-{form}"
    spec = all_cases()[cid]
    got = check(pt, gpu_ctx, undef_scenes, poison_twin, cid, spec)
    w, h = spec["size"]
    assert int(got["stats"][0]) == 2 * w * h * spec["spp"] and int(got["stats"][4]) == 0, got["stats"]
    assert (got["film"] == np.float32(ENV["env"])).all(), got["film"][0, 0]
    cid = f"sees_nothing_then_the_box-{form}"
    got = check(pt, gpu_ctx, undef_scenes, poison_twin, cid, all_cases()[cid])
    assert int(got["stats"][0]) > 3 * w * h * spec["spp"]   # (the box was seen: paths of more than one ray)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("scene", ["leaves_of_four", "one_triangle"])
def test_poison_twin_on_the_other_trees(pt, gpu_ctx, undef_scenes, poison_twin, scene, form):
    """k_fused<., false> (the box with leaves of up to four triangles) and a scene that is one triangle"""
    cid = f"{scene}-{form}"
    check(pt, gpu_ctx, undef_scenes, poison_twin, cid, all_cases()[cid])


@pytest.mark.gpu
def test_poison_twin_first_hit_log(pt, gpu_ctx, undef_scenes, poison_twin):
    """pt_render_guided's single pass (the LOG kernels) on 8x8, 1 spp: film, image, rays and the six guide planes"""
    got = check(pt, gpu_ctx, undef_scenes, poison_twin, "guided-8x8", all_cases()["guided-8x8"])
    assert sum(k.startswith("aov") for k in got) == pt.AOV_COUNT


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c for c in all_cases() if c.startswith("nee-")])
def test_poison_twin_nee(pt, gpu_ctx, undef_scenes, poison_twin, cid):
    """PT_FLAG_NEE (k_fused_nee: the spawn steps and the hit record's reset are shared with it)"""
    check(pt, gpu_ctx, undef_scenes, poison_twin, cid, all_cases()[cid])


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
def test_poison_twin_counts_the_same_rays(pt, gpu_ctx, undef_scenes, poison_twin, form):
    """PT_FLAG_COUNT_VISITS (k_fused_count): the twin's ray count and film are the product's"""
    cid = f"count_visits-{form}"
    check(pt, gpu_ctx, undef_scenes, poison_twin, cid, all_cases()[cid])


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--twin":
        twin_main(sys.argv[2])
    else:
        sys.exit("usage: test_fused_undef.py --twin OUT.npz (the child process of the poison_twin fixture)")
