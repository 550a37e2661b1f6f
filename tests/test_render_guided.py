"""pt_render_guided: the radiance film and the first-hit guides of one camera in one pass (include/pt_api.h).

The contract is equality with the two existing calls, so the reference of every GPU case is a second film of the same context filled by
pt_render and then pt_render_aov -- themselves pinned to the oracle by tests/test_gpu_parity.py and tests/test_aov.py -- and every comparison
is `tobytes()` equality of: the float film, bgra8, M and its `frames`, and the six guide planes.  One Cornell case and one instanced case are
also held against the oracle directly.  Without a GPU: the header, and the reduce kernel's per-pixel body (csrc/guided_kernel.h) compiled
for the host (tests/guided_host.cpp) against a numpy restatement of the guides' definition, plain and under the sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MISS = 0xFFFFFFFF
NAMES = ["albedo", "normal", "emission", "depth", "alpha", "id"]
NEW_SYMBOLS = ["pt_guided_params_default", "pt_render_guided"]


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------------
def test_guided_layout_defaults_and_symbols(pt, tmp_path):
    """sizeof / offsetof of pt_guided_params and pt_guided_result by gcc from the header == the ctypes mirrors (32 bytes each); the enum's
    values; the default; the new names in API_SYMBOLS and in the library; PT_API_VERSION stays 6; NULL handles are PT_ERR_INVALID_ARG."""
    src = tmp_path / "gd_layout.c"
    vals = ["sizeof(pt_guided_params)", "sizeof(pt_guided_result)", "offsetof(pt_guided_params, mode)", "offsetof(pt_guided_params, reserved)",
            "offsetof(pt_guided_result, single_pass)", "offsetof(pt_guided_result, launches)", "offsetof(pt_guided_result, guide_ms)",
            "offsetof(pt_guided_result, reserved)", "(size_t)PT_GUIDED_AUTO", "(size_t)PT_GUIDED_SINGLE_PASS", "(size_t)PT_GUIDED_TWO_CALLS", "(size_t)PT_API_VERSION"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("' + "%zu " * len(vals) + '\\n",' + ", ".join(vals) + ");return 0;}\n")
    exe = tmp_path / "gd_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P, R = pt.GuidedParams, pt.GuidedResult
    assert got == [32, 32, 0, 4, 0, 4, 8, 12, 0, 1, 2, 6], got
    assert got[:8] == [C.sizeof(P), C.sizeof(R), P.mode.offset, P.reserved.offset, R.single_pass.offset, R.launches.offset, R.guide_ms.offset, R.reserved.offset]
    assert (pt.GUIDED_AUTO, pt.GUIDED_SINGLE_PASS, pt.GUIDED_TWO_CALLS) == (0, 1, 2)
    for name in NEW_SYMBOLS:
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    p = pt.guided_default_params()   # (touches no device)
    assert (p.mode, list(p.reserved)) == (pt.GUIDED_AUTO, [0] * 7)
    lib = pt.lib_amd()
    lib.pt_guided_params_default(None)                                       # (a NULL is ignored)
    q = pt.default_params()
    assert lib.pt_render_guided(None, None, None, None, None) == 1
    assert lib.pt_render_guided(None, None, C.byref(q), C.byref(p), None) == 1


def _tile_list(w, h, rng):
    """every 8x8 tile of the image as tile x | tile y << 16, in a shuffled order (the reduce finds its pixels through the list alone)"""
    t = np.asarray([tx | (ty << 16) for ty in range((h + 7) // 8) for tx in range((w + 7) // 8)], np.uint32)
    return t[rng.permutation(len(t))]


def _host_case(w, h, spp, n_frames, frame0, inst, has_frame, cull, seed):
    """A synthetic launch: tables, a tile list, per-sample first hits, and the log the fused kernels would have written for them -- records of
    culled pixels and of pixels beyond the image's edge hold a position far outside the tables, so reading one is an out-of-bounds index."""
    rng = np.random.default_rng(seed)
    n_tris, n_inst = 37, (5 if inst else 0)
    tiles = _tile_list(w, h, rng)
    prim_of = rng.permutation(n_tris).astype(np.uint32)                 # leaf position -> primitive
    tri4 = rng.uniform(-1, 1, (n_tris, 3, 4)).astype(f32)
    tri4[:, 0, 3] = prim_of.view(f32)
    shade4 = rng.uniform(-1, 1, (n_tris, 3, 4)).astype(f32)
    faces = rng.uniform(0, 1, (n_tris, 6)).astype(f32)
    inst6 = rng.uniform(-1, 1, (n_inst, 6, 4)).astype(f32)
    inst_frame = rng.uniform(-1, 1, (n_inst, n_tris, 2, 4)).astype(f32) if has_frame else np.zeros((0,), f32)
    inst_id = rng.permutation(n_inst).astype(np.uint32)
    pos = rng.integers(0, n_tris, (n_frames, h, w, spp)).astype(np.uint32)
    pos[rng.uniform(0, 1, pos.shape) < 0.3] = MISS
    ip = rng.integers(0, max(n_inst, 1), pos.shape).astype(np.uint32)
    t = rng.uniform(0.5, 9.0, pos.shape).astype(f32)
    rect = (3, 2, w - 4, h - 3) if cull else (0, 0, -1, -1)
    yy, xx = np.mgrid[0:h, 0:w]
    culled = ((xx < rect[0]) | (xx > rect[2]) | (yy < rect[1]) | (yy > rect[3])) if cull else np.zeros((h, w), bool)
    pos[:, culled] = MISS                                                # (what such a pixel's samples are: misses)
    log = np.zeros((n_frames, spp, len(tiles) * 64, 2), np.uint32)                   # [frame][sample][pixel of the tile list]: guided_kernel.h gd_log_index
    log[..., 0] = 0x7FFFFFF0                                             # poison: never to be read
    for k, tw in enumerate(tiles):
        for l in range(64):
            px, py = int(tw & 0xFFFF) * 8 + (l & 7), int(tw >> 16) * 8 + (l >> 3)
            if px >= w or py >= h or culled[py, px]:
                continue
            word = pos[:, py, px] | ((ip[:, py, px] << 11) if inst else 0)
            log[:, :, k * 64 + l, 0] = np.where(pos[:, py, px] == MISS, MISS, word)
            log[:, :, k * 64 + l, 1] = t[:, py, px].view(np.uint32)
    return dict(w=w, h=h, spp=spp, n_frames=n_frames, frame0=frame0, inst=inst, has_frame=has_frame, cull=cull, rect=rect, tiles=tiles, n_tris=n_tris,
                n_inst=n_inst, prim_of=prim_of, tri4=tri4, shade4=shade4, faces=faces, inst6=inst6, inst_frame=inst_frame, inst_id=inst_id, pos=pos, ip=ip,
                t=t, log=log)


def _planes_ref(c, planes, id_frame):
    """DESIGN.md section 12 restated in float32 numpy: a sample's values are Kd, the normal, Ke, t and 1 (0 on a miss); a frame's value is
    ((0 + v_0) + v_1 ...) / spp, blended as (value + old * F) / (F + 1) with `old` not read for F = 0; id = {prim, inst} of sample 0 of frame
    `id_frame` of the launch.  The instanced normal: the table's, or the object normal through the inverse transpose, normalised."""
    h, w, spp = c["h"], c["w"], c["spp"]
    out = {n: planes[n].copy() for n in NAMES}
    for k in range(c["n_frames"]):
        F = c["frame0"] + k
        pos, ip, hit = c["pos"][k], c["ip"][k], c["pos"][k] != MISS
        p = np.where(hit, pos, 0)
        prim = c["prim_of"][p]
        nrm = c["shade4"][p, 0, :3]
        if c["inst"]:
            if c["has_frame"]:
                nrm = c["inst_frame"][ip, p, 0, :3]
            else:
                i0, i1, i2 = c["inst6"][ip, 3], c["inst6"][ip, 4], c["inst6"][ip, 5]
                wv = [(i0[..., a] * nrm[..., 0] + i1[..., a] * nrm[..., 1]) + i2[..., a] * nrm[..., 2] for a in range(3)]
                ln = np.sqrt((wv[0] * wv[0] + wv[1] * wv[1]) + wv[2] * wv[2])
                nrm = np.stack([wv[0] / ln, wv[1] / ln, wv[2] / ln], -1)
        val = np.zeros((h, w, spp, 11), f32)
        val[..., 0:3] = c["faces"][prim, 0:3]
        val[..., 3:6] = nrm
        val[..., 6:9] = c["faces"][prim, 3:6]
        val[..., 9] = c["t"][k]
        val[..., 10] = f32(1)
        val[~hit] = f32(0)
        acc = np.zeros((h, w, 11), f32)
        for s in range(spp):
            acc = acc + val[:, :, s]
        value = acc / f32(spp)
        for name, sl in (("albedo", slice(0, 3)), ("normal", slice(3, 6)), ("emission", slice(6, 9)), ("depth", 9), ("alpha", 10)):
            out[name] = value[..., sl] if F == 0 else (value[..., sl] + out[name] * f32(F)) / f32(F + 1)
            assert out[name].dtype == f32
        if k == id_frame:
            inst_of = c["inst_id"][ip[..., 0]] if c["inst"] else np.zeros((h, w), np.uint32)
            out["id"] = np.stack([np.where(hit[..., 0], prim[..., 0], MISS), np.where(hit[..., 0], inst_of, MISS)], -1).astype(np.uint32)
    return out


def _run_on_host(exe, d, c, planes, id_frame):
    os.makedirs(d, exist_ok=True)
    par = np.zeros(20, np.int32)
    par[:16] = [c["w"], c["h"], c["spp"], c["n_frames"], c["frame0"], id_frame, len(c["tiles"]), c["n_tris"], c["n_inst"], int(c["inst"]), int(c["has_frame"]),
                int(c["cull"])] + list(c["rect"])
    par.tofile(os.path.join(d, "par"))
    for name in ("tiles", "log", "tri4", "shade4", "faces", "inst6", "inst_frame", "inst_id"):
        np.ascontiguousarray(c[name]).tofile(os.path.join(d, name))
    for n in NAMES:
        np.ascontiguousarray(planes[n]).tofile(os.path.join(d, n))
    subprocess.check_call([exe, d])
    return {n: np.fromfile(os.path.join(d, "o_" + n), planes[n].dtype).reshape(planes[n].shape) for n in NAMES}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_reduce_body_on_the_host_equals_the_definition(tmp_path, sanitize):
    """csrc/guided_kernel.h -- what k_guided_reduce runs per pixel -- compiled by g++ as a stand-alone program (-ffp-contract=off, the IEEE
    divide and root for pt_math.h's) gives the bytes of `_planes_ref`: image sizes that are no multiples of 8, spp 1 and 5, culled pixels, two
    frames from frame 0 and from frame 3, single-level and instanced records with and without the normal table, the id frame inside and
    outside of the launch.  The logs are exactly their size and the records nobody wrote hold an index far outside the tables: the second
    build, under AddressSanitizer and UBSan, shows that none of them is read and no index leaves the log."""
    exe = str(tmp_path / "guided_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "guided_host.cpp")])
    rng = np.random.default_rng(4)
    n = 0
    for (w, h), spp, n_frames, frame0, inst, has_frame, cull, id_frame in (
            ((16, 8), 1, 1, 0, False, False, False, 0), ((21, 13), 5, 2, 0, False, False, True, 1), ((21, 13), 5, 2, 3, False, False, True, 2),
            ((9, 17), 5, 2, 0, True, False, False, 1), ((9, 17), 1, 2, 3, True, True, True, 1), ((30, 11), 5, 1, 7, True, False, True, 0)):
        c = _host_case(w, h, spp, n_frames, frame0, inst, has_frame, cull, seed=n + 1)
        planes = {k: rng.uniform(0, 1, (h, w) + ((3,) if k in NAMES[:3] else ())).astype(f32) for k in NAMES[:5]}
        planes["id"] = rng.integers(0, 99, (h, w, 2)).astype(np.uint32)
        want = _planes_ref(c, planes, id_frame)
        got = _run_on_host(exe, str(tmp_path / f"c{n}"), c, planes, id_frame)
        for k in NAMES:
            assert got[k].tobytes() == want[k].tobytes(), (n, k, int((got[k] != want[k]).sum()))
        if frame0 == 0:   # (the case holds hits, misses and -- with the cull -- pixels without a record)
            assert (want["alpha"] > 0).any() and (want["alpha"] < 1).any() and (not cull or (want["alpha"] == 0).any())
        n += 1


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------
KW = dict(spp_per_frame=4, max_depth=6)
GRID_CAM = dict(cam_origin=(-0.84, -1.99, 0.5), cam_target=(-0.84, -1.99, -19.5))   # (tests/test_aov.py: a square of side 0.05 around three instances)
AWAY_CAM = dict(cam_origin=(0.0, 1.0, 9.0), cam_target=(0.0, 1.0, 12.0))           # looks away from the box: background only, and no cull rectangle
# The default camera moved 2.9 to the side: the box (x in [-1.02, 1], z in [-1.04, 0.99]) projects to dx = (x - 2.9) / a, a = (5 - z) / 3 in
# [1.34, 2.01], i.e. dx <= -0.945 -- the two leftmost pixel columns of an 80-wide image with the rectangle's pixel of slack.  Every other slot is
# finished without a walk.
CORNER_CAM = dict(cam_origin=(2.9, -1.0, 5.0), cam_target=(2.9, -1.0, 2.0))


def _one_instance():
    """a single instance: rotated about z, scaled unevenly, moved -- the normal needs the inverse transpose (tests/test_aov.py)"""
    c, s = f32(np.cos(0.5)), f32(np.sin(0.5))
    return np.array([[[0.9 * c, -0.7 * s, 0.0, 0.15], [0.9 * s, 0.7 * c, 0.0, -0.4], [0.0, 0.0, 1.1, 0.1]]], f32)


def _soup(n, seed, spread=0.1):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)).astype(f32)
    v = (c + rng.uniform(-spread, spread, (n, 3, 3)).astype(f32)).astype(f32)
    faces = rng.uniform(0, 1, (n, 6)).astype(f32)
    faces[:, 3:] *= (rng.uniform(0, 1, (n, 1)) < 0.1)
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), faces.reshape(-1).astype(f32)


def _film(pt, ctx, w, h, planes=None):
    film = pt.Film(ctx, w, h)
    film.enable_aov(planes)
    film.enable_moments()
    return film


def _state(film):
    st = {"f32": film.read_f32(), "bgra8": film.read_bgra8()}
    st["M"], st["frames"] = film.read_moments()
    for k, n in enumerate(NAMES):
        st[n] = film.read_aov(k)
    return st


def _same(got, want, what):
    assert got["frames"] == want["frames"], (what, got["frames"], want["frames"])
    for n in ["f32", "bgra8", "M"] + NAMES:
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, (what, n)
        assert got[n].tobytes() == want[n].tobytes(), (what, n, int((got[n] != want[n]).sum()))


def _params(pt, w, h, **kw):
    return pt.default_params(width=w, height=h, **{**KW, "pipeline": pt.PIPELINE_AUTO, **kw})


def _pair(pt, ctx, sc, w, h, calls, mode=None, single=1, films=None, what=""):
    """Every call of `calls` (keyword sets of pt_params) through pt_render_guided into one film and through pt_render + pt_render_aov into another:
    equal bytes after every call, `single_pass` as expected, and rays / paths / rays_culled of the single pass equal to pt_render's alone (of the
    two-call form: to both calls').  -> the results."""
    mode = pt.GUIDED_AUTO if mode is None else mode
    got, ref = films if films else (_film(pt, ctx, w, h), _film(pt, ctx, w, h))
    out = []
    try:
        for kw in calls:
            p = _params(pt, w, h, **kw)
            ctx.reset_stats()
            res = pt.render_guided(sc, got, p, mode=mode)
            sg = ctx.stats()
            ctx.reset_stats()
            pt.render(sc, ref, p)
            sr = ctx.stats()
            pt.render_aov(sc, ref, p)
            sa = ctx.stats()
            assert res.single_pass == single, (what, kw, res.single_pass)
            want = sr if single else sa
            assert (sg.rays, sg.paths, sg.rays_culled) == (want.rays, want.paths, want.rays_culled), (what, kw, sg.rays, sr.rays, sa.rays)
            assert sg.pipeline == sr.pipeline and sr.rays > 0 and sa.rays > sr.rays
            assert res.guide_ms > 0 and (res.launches >= 1) == bool(single), (what, kw, res.guide_ms, res.launches)
            _same(_state(got), _state(ref), (what, kw))
            out.append(res)
    finally:
        if not films:
            got.close(); ref.close()
    return out


TWO = [dict(frame=0, frame_count=2), dict(frame=3, frame_count=2)]   # the second call: the blend's `frame != 0` path


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(80, 56), (77, 53)], ids=["80x56", "77x53_edge_tiles"])
@pytest.mark.parametrize("fif", [0, 1, 2])
def test_guided_cornell(pt, gpu_ctx, cornell_gpu, size, fif):
    res = _pair(pt, gpu_ctx, cornell_gpu, *size, [dict(frames_in_flight=fif, **c) for c in TWO], what=(size, fif))
    assert [r.launches for r in res] == ([2, 2] if fif == 1 else [1, 1])


@pytest.mark.gpu
def test_guided_cornell_against_the_oracle(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle):
    """film, bgra8 and the ray count of a guided call are the oracle's own"""
    w, h = 80, 56
    film = _film(pt, gpu_ctx, w, h)
    try:
        gpu_ctx.reset_stats()
        res = pt.render_guided(cornell_gpu, film, _params(pt, w, h, frame=0, frame_count=2))
        ofilm, obgra, orays = np.zeros((h, w, 3), f32), np.zeros((h, w, 4), np.uint8), 0
        for k in range(2):
            img, r, _, _ = cornell_oracle.render_frame(orc.default_params(frame=k, width=w, height=h, **KW))
            orc.accumulate_f32(ofilm, img, k); orc.accumulate_bgra8(obgra, img, k)
            orays += r
        assert res.single_pass == 1 and gpu_ctx.stats().rays == orays
        assert film.read_f32().tobytes() == ofilm.tobytes() and film.read_bgra8().tobytes() == obgra.tobytes()
    finally:
        film.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["one_group", "four_groups", "head_tail", "no_pair_kernel", "nee"])
def test_guided_every_kernel_shape(pt, gpu_ctx, cornell_gpu, cornell_arrays, shape):
    """one sample group, several, head + tail slots (pt_tuning.fused_tail), the kernel without pair leaves (pt_tuning.pair_kernel = 0: a scene
    built under it), and k_fused_nee"""
    kw, tuning = {"one_group": (dict(sample_groups=1), {}), "four_groups": (dict(sample_groups=4), {}), "head_tail": ({}, dict(fused_tail=2)),
                  "no_pair_kernel": ({}, dict(pair_kernel=0)), "nee": (dict(flags=pt.FLAG_NEE), {})}[shape]
    old = gpu_ctx.set_tuning(**tuning)
    sc = pt.Scene(gpu_ctx, *cornell_arrays) if shape == "no_pair_kernel" else cornell_gpu
    try:
        _pair(pt, gpu_ctx, sc, 77, 53, [dict(**kw, **c) for c in TWO], what=shape)
        st = gpu_ctx.stats()   # (of the reference's calls: the shape that was asked for is the shape that ran)
        if shape == "head_tail":
            assert st.tail_samples == 2
        if shape == "four_groups":
            assert st.sample_groups == 4
    finally:
        gpu_ctx.set_tuning(**old)
        if sc is not cornell_gpu:
            sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cull", [0, -1], ids=["cull_off", "cull_default"])
@pytest.mark.parametrize("groups", [0, 1, 4])
def test_guided_cull(pt, gpu_ctx, cornell_gpu, cull, groups):
    """the default camera, where an eighth of the pixels look past the box, and a camera that has the box in two pixel columns at the image's edge
    (every other slot is culled): such pixels have no records, and their samples are the misses they are"""
    old = gpu_ctx.set_tuning(cull=cull)
    try:
        for cam in ({}, CORNER_CAM):
            _pair(pt, gpu_ctx, cornell_gpu, 80, 56, [dict(sample_groups=groups, **cam, **c) for c in TWO], what=(cull, groups, bool(cam)))
            st = gpu_ctx.stats()   # (of the reference's calls)
            assert (st.rays_culled > 0) == (cull != 0), (cull, groups, cam, st.rays_culled)
            if cam and cull:
                assert st.rays_culled >= 76 * 56 * 4 * 2, st.rays_culled
    finally:
        gpu_ctx.set_tuning(**old)


@pytest.mark.gpu
def test_guided_stale_scratch(pt, gpu_ctx, cornell_gpu):
    """the log is reused: after a guided call at another camera and pt_film_clear, a record that was read without being written this time would
    show in the planes"""
    w, h = 80, 56
    got, ref = _film(pt, gpu_ctx, w, h), _film(pt, gpu_ctx, w, h)
    try:
        pt.render_guided(cornell_gpu, got, _params(pt, w, h, frame=0, frame_count=2, cam_origin=(0.3, 0.8, 2.5), cam_target=(0.3, 0.2, -0.5)))
        got.clear()
        _pair(pt, gpu_ctx, cornell_gpu, w, h, TWO, films=(got, ref), what="after another camera")
        got.clear(); ref.clear()
        _pair(pt, gpu_ctx, cornell_gpu, w, h, [dict(**AWAY_CAM, **c) for c in TWO], films=(got, ref), what="background after the box")
    finally:
        got.close(); ref.close()


def _inst_scene(pt, ctx, cornell_arrays, which):
    sc = pt.Scene(ctx, *cornell_arrays)
    inst = pt.cornell_grid_instances()[:16] if which == "grid16" else _one_instance()
    if which == "two_inst":   # the same rotated, unevenly scaled instance and a copy of it moved up and back: two instances, the fused kernel's class
        inst = np.concatenate([inst, inst + f32([[[0, 0, 0, 0.3], [0, 0, 0, 1.2], [0, 0, 0, -0.8]]])]).astype(f32)
    sc.set_instances(inst)
    return sc, inst


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["grid16", "one_inst", "two_inst"])
@pytest.mark.parametrize("inst_frames", [0, 1])
@pytest.mark.parametrize("groups", [1, 4], ids=["plain", "grouped"])
def test_guided_instanced(pt, gpu_ctx, cornell_arrays, which, inst_frames, groups):
    """the two-level kernel, grouped and not, with the (instance, triangle) normal table and by the inverse transpose.  The fused two-level kernel
    takes 2 .. 32767 instances, so pt_render gives the one-instance scene to the queues and PT_GUIDED_AUTO takes the two calls for it; the same
    rotated, unevenly scaled instance twice goes through the single pass."""
    old = gpu_ctx.set_tuning(inst_frames=inst_frames)
    sc, _ = _inst_scene(pt, gpu_ctx, cornell_arrays, which)
    cam = GRID_CAM if which == "grid16" else {}
    try:
        _pair(pt, gpu_ctx, sc, 52, 44, [dict(sample_groups=groups, **cam, **c) for c in TWO], single=0 if which == "one_inst" else 1, what=(which, inst_frames, groups))
    finally:
        sc.close()
        gpu_ctx.set_tuning(**old)


@pytest.mark.gpu
def test_guided_instanced_against_the_oracle(pt, orc, gpu_ctx, cornell_arrays):
    w, h = 48, 40
    sc, inst = _inst_scene(pt, gpu_ctx, cornell_arrays, "grid16")
    film = _film(pt, gpu_ctx, w, h)
    try:
        osc = orc.Scene(*cornell_arrays)
        osc.set_instances(inst)
        gpu_ctx.reset_stats()
        res = pt.render_guided(sc, film, _params(pt, w, h, frame=0, frame_count=1, **GRID_CAM))
        img, orays, _, _ = osc.render_frame(orc.default_params(frame=0, width=w, height=h, **KW, **GRID_CAM))
        ofilm = np.zeros((h, w, 3), f32)
        orc.accumulate_f32(ofilm, img, 0)
        assert res.single_pass == 1 and gpu_ctx.stats().rays == orays
        assert film.read_f32().tobytes() == ofilm.tobytes()
        assert (film.read_aov(pt.AOV_ALPHA) > 0).any()
    finally:
        film.close(); sc.close()


@pytest.mark.gpu
def test_guided_rank_of_a_world(pt, gpu_ctx, cornell_gpu):
    _pair(pt, gpu_ctx, cornell_gpu, 77, 53, [dict(rank=1, world=3, **c) for c in TWO], what="rank 1 of 3")


@pytest.mark.gpu
def test_guided_external_guide_planes(pt, gpu_ctx, cornell_gpu):
    import torch
    w, h = 77, 53
    t = [torch.zeros((h, w) + tail, dtype=torch.float32 if dt == np.float32 else torch.int32, device="cuda:0") for tail, dt in (pt.AOV_SHAPES[k] for k in range(pt.AOV_COUNT))]
    got, ref = _film(pt, gpu_ctx, w, h, [x.data_ptr() for x in t]), _film(pt, gpu_ctx, w, h)
    try:
        _pair(pt, gpu_ctx, cornell_gpu, w, h, TWO, films=(got, ref), what="external planes")
        torch.cuda.synchronize()
        for k, n in enumerate(NAMES):
            assert t[k].cpu().numpy().view(ref.read_aov(k).dtype).tobytes() == ref.read_aov(k).tobytes(), n
    finally:
        got.close(); ref.close()


@pytest.mark.gpu
def test_guided_after_a_scene_update(pt, gpu_ctx, cornell_arrays):
    v, i, f = cornell_arrays
    sc = pt.Scene(gpu_ctx, v, i, f)
    try:
        _pair(pt, gpu_ctx, sc, 80, 56, TWO[:1], what="before the refit")
        moved = (np.asarray(v, f32).reshape(-1, 3) * f32([0.8, 1.0, 0.9]) + f32([0.1, -0.05, 0.0])).astype(f32).reshape(-1)
        sc.update(moved, i)
        _pair(pt, gpu_ctx, sc, 80, 56, TWO, what="after the refit")
    finally:
        sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["soup", "wavefront", "named_extend"])
def test_guided_falls_back_to_the_two_calls(pt, gpu_ctx, cornell_gpu, case):
    """a 3000-triangle soup, PT_PIPELINE_WAVEFRONT and a named closest-hit kernel: PT_GUIDED_AUTO runs the two calls (same bytes, both calls'
    rays), PT_GUIDED_SINGLE_PASS is PT_ERR_UNSUPPORTED"""
    sc = pt.Scene(gpu_ctx, *_soup(3000, 5)) if case == "soup" else cornell_gpu
    kw = {"soup": dict(cam_origin=(0.0, 0.0, 4.5), cam_target=(0.0, 0.0, 1.5)), "wavefront": dict(pipeline=pt.PIPELINE_WAVEFRONT), "named_extend": dict(extend=pt.EXTEND_LDS)}[case]
    w, h = 48, 40
    try:
        _pair(pt, gpu_ctx, sc, w, h, [dict(**kw, **c) for c in TWO], single=0, what=case)
        film = _film(pt, gpu_ctx, w, h)
        try:
            gp = pt.guided_default_params()
            gp.mode = pt.GUIDED_SINGLE_PASS
            gpu_ctx.reset_stats()
            assert pt.lib_amd().pt_render_guided(sc.h, film.h, C.byref(_params(pt, w, h, frame=0, frame_count=1, **kw)), C.byref(gp), None) == 5
            assert gpu_ctx.stats().rays == 0 and not film.read_f32().any()
        finally:
            film.close()
    finally:
        if sc is not cornell_gpu:
            sc.close()


@pytest.mark.gpu
def test_guided_two_calls_mode(pt, gpu_ctx, cornell_gpu):
    _pair(pt, gpu_ctx, cornell_gpu, 80, 56, TWO, mode=pt.GUIDED_TWO_CALLS, single=0, what="PT_GUIDED_TWO_CALLS")


@pytest.mark.gpu
def test_guided_log_within_the_memory_budget(pt, gpu_ctx, cornell_gpu):
    """80 x 56 pads to 70 tiles = 4480 pixels.  At 16 spp a frame of the log is 4480 * 16 * 8 = 573 440 bytes: under a budget of 1 MB, beside a
    render workspace of ~0.3 MB, one frame fits and two cannot (2 * 573 440 > 1 MB), so a four-frame call takes four launches.  At 32 spp a
    frame is 1 146 880 bytes > 1 MB: no frame fits and PT_GUIDED_AUTO takes the two calls.  Same bytes both times."""
    old = gpu_ctx.set_tuning(mem_budget_mb=1)
    try:
        res = _pair(pt, gpu_ctx, cornell_gpu, 80, 56, [dict(frame=0, frame_count=4, sample_groups=1, spp_per_frame=16)], what="one frame fits")
        assert res[0].launches == 4
        _pair(pt, gpu_ctx, cornell_gpu, 80, 56, [dict(frame=0, frame_count=2, sample_groups=1, spp_per_frame=32)], single=0, what="no frame fits")
    finally:
        gpu_ctx.set_tuning(**old)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [dict(sample_groups=4, frames_in_flight=2), dict(frames_in_flight=2)], ids=["groups", "head_tail"])
def test_guided_term_log_overflow(pt, gpu_ctx, cornell_arrays, shape):
    """every surface emits, so every ray logs a term: with a pool of three entries (pt_tuning.term_ocap / term_spill, as the overflow tests force
    it) a launch overflows its term logs and its frames are rendered again -- the guides are folded once, from the same records"""
    v, i, f = cornell_arrays
    f = f.reshape(-1, 6).copy()
    f[:, 3:] = f32(0.25) + f[:, :3] * f32(0.5)
    sc = pt.Scene(gpu_ctx, v, i, f.reshape(-1))
    old = gpu_ctx.set_tuning(term_ocap=0, term_spill=3, **({} if "sample_groups" in shape else dict(fused_tail=4)))
    try:
        w, h = 52, 36
        got, ref = _film(pt, gpu_ctx, w, h), _film(pt, gpu_ctx, w, h)
        try:
            redone = 0
            for c in (dict(frame=0, frame_count=4), dict(frame=4, frame_count=3)):
                p = _params(pt, w, h, **{**shape, **c, "spp_per_frame": 8, "max_depth": 12})
                gpu_ctx.reset_stats()
                res = pt.render_guided(sc, got, p)
                sg = gpu_ctx.stats()
                redone += sg.redone_batches
                gpu_ctx.reset_stats()
                pt.render(sc, ref, p)
                assert res.single_pass == 1 and sg.rays == gpu_ctx.stats().rays
                pt.render_aov(sc, ref, p)
                _same(_state(got), _state(ref), (shape, c))
            assert redone > 0
        finally:
            got.close(); ref.close()
    finally:
        gpu_ctx.set_tuning(**old)
        sc.close()


@pytest.mark.gpu
def test_guided_refusals_leave_the_film_untouched(pt, gpu_ctx, cornell_gpu):
    """PT_FLAG_ASYNC, _PROFILE, _COUNT_VISITS -> PT_ERR_UNSUPPORTED; a film without guides, an unknown mode, a nonzero reserved word, a size that
    is not the film's -> PT_ERR_INVALID_ARG; nothing traced, nothing written; the film renders correctly afterwards"""
    w, h = 80, 56
    lib = pt.lib_amd()
    got, ref, bare = _film(pt, gpu_ctx, w, h), _film(pt, gpu_ctx, w, h), pt.Film(gpu_ctx, w, h)
    try:
        p = _params(pt, w, h, frame=0, frame_count=2)
        gp = pt.guided_default_params()
        gpu_ctx.reset_stats()
        for flag in (pt.FLAG_ASYNC, pt.FLAG_PROFILE, pt.FLAG_COUNT_VISITS):
            for pipeline in (pt.PIPELINE_WAVEFRONT, pt.PIPELINE_AUTO, pt.PIPELINE_FUSED):
                q = _params(pt, w, h, frame=0, frame_count=2, flags=flag, pipeline=pipeline)
                assert lib.pt_render_guided(cornell_gpu.h, got.h, C.byref(q), C.byref(gp), None) == 5, (flag, pipeline)
        for args in ((None, got.h, p, gp), (cornell_gpu.h, None, p, gp), (cornell_gpu.h, got.h, None, gp), (cornell_gpu.h, got.h, p, None)):
            a = [C.byref(x) if isinstance(x, C.Structure) else x for x in args]
            assert lib.pt_render_guided(a[0], a[1], a[2], a[3], None) == 1
        assert lib.pt_render_guided(cornell_gpu.h, bare.h, C.byref(p), C.byref(gp), None) == 1
        assert "guide" in gpu_ctx_error(pt, gpu_ctx)
        bad = pt.guided_default_params()
        bad.mode = 3
        assert lib.pt_render_guided(cornell_gpu.h, got.h, C.byref(p), C.byref(bad), None) == 1
        for k in range(7):
            r = pt.guided_default_params()
            r.reserved[k] = 1
            assert lib.pt_render_guided(cornell_gpu.h, got.h, C.byref(p), C.byref(r), None) == 1
        assert lib.pt_render_guided(cornell_gpu.h, got.h, C.byref(_params(pt, w + 1, h, frame=0, frame_count=2)), C.byref(gp), None) == 1
        assert gpu_ctx.stats().rays == 0
        st = _state(got)
        assert not any(st[n].any() for n in ["f32", "bgra8", "M"] + NAMES) and not bare.read_f32().any()
        _pair(pt, gpu_ctx, cornell_gpu, w, h, TWO, films=(got, ref), what="after the refusals")
    finally:
        got.close(); ref.close(); bare.close()


def gpu_ctx_error(pt, ctx):
    return pt.lib_amd().pt_last_error(ctx.h).decode()
