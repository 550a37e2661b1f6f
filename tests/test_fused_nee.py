"""PT_FLAG_NEE: the next-event estimator on any pipeline value, and the fused single kernel's NEE instantiation (k_fused_nee).

The estimator is the oracle's `nee` mode (oracle/pt_oracle.c) and PT_PIPELINE_WAVEFRONT_NEE; the fused kernel must give the same
film, rgba8 image and ray count (shadow rays included) bit for bit.  The suite's `pt.default_params` names the wavefront pipeline,
so every call here names its pipeline."""
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_nee(orc, osc, frames, **kw):
    """-> (film f32, bgra8, rays) after `frames` frames of the oracle's nee mode."""
    film = bgra = None
    rays = 0
    for k in range(frames):
        img, r, _, _ = osc.render_frame(orc.default_params(frame=k, nee=1, **kw))
        if film is None:
            film = np.zeros_like(img)
            bgra = np.zeros(img.shape[:2] + (4,), np.uint8)
        orc.accumulate_f32(film, img, k)
        orc.accumulate_bgra8(bgra, img, k)
        rays += r
    return film, bgra, rays


def _soup(n, seed, emit_share, spread=0.1):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)).astype(np.float32)
    v = (c + rng.uniform(-spread, spread, (n, 3, 3)).astype(np.float32)).astype(np.float32)
    faces = rng.uniform(0, 1, (n, 6)).astype(np.float32)
    faces[:, 3:] *= (rng.uniform(0, 1, (n, 1)) < emit_share)
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), faces.reshape(-1).astype(np.float32)


def _render(pt, ctx, scene, w, h, frames, pipeline, flags=0, **kw):
    """-> (film f32, bgra8, stats) of frames 0 .. frames-1 in one call."""
    film = pt.Film(ctx, w, h)
    ctx.reset_stats()
    pt.render(scene, film, pt.default_params(width=w, height=h, frame=0, frame_count=frames, pipeline=pipeline, flags=flags, **kw))
    out = film.read_f32(), film.read_bgra8(), ctx.stats()
    film.close()
    return out


def test_flag_nee_matches_header(pt, tmp_path):
    """PT_FLAG_NEE in include/pt_api.h == pt.FLAG_NEE == 32, read through gcc."""
    src = tmp_path / "flag.c"
    src.write_text('#include <stdio.h>\n#include "pt_api.h"\nint main(void){printf("%u %u %d\\n", (unsigned)PT_FLAG_NEE, '
                   '(unsigned)PT_PIPELINE_WAVEFRONT_NEE, PT_API_VERSION);return 0;}\n')
    exe = tmp_path / "flag"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [pt.FLAG_NEE, pt.PIPELINE_WAVEFRONT_NEE, 6] and pt.FLAG_NEE == 32


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(80, 56), (77, 53)])
@pytest.mark.parametrize("fif", [2, 0])
def test_fused_nee_equals_the_oracles_nee_mode(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, size, fif):
    """FUSED | NEE: frame 0 alone, then frames 1-2 in one call -- film f32, rgba8 and every ray (path + shadow) as the oracle's nee mode."""
    w, h = size
    kw = dict(width=w, height=h, spp_per_frame=8, max_depth=8)
    ofilm, obgra, orays = _oracle_nee(orc, cornell_oracle, 3, **kw)
    film = pt.Film(gpu_ctx, w, h)
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=1, pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_NEE, **kw))
    st0 = gpu_ctx.stats()
    assert st0.pipeline == pt.PIPELINE_FUSED and st0.sample_groups == 1 and st0.tail_samples == 0
    pt.render(cornell_gpu, film, pt.default_params(frame=1, frame_count=2, pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_NEE,
                                                   frames_in_flight=fif, **kw))
    st = gpu_ctx.stats()
    assert st.pipeline == pt.PIPELINE_FUSED and st.sample_groups == 1 and st.tail_samples == 0
    assert st.rays == orays
    assert film.read_f32().tobytes() == ofilm.tobytes(), float(np.abs(film.read_f32() - ofilm).max())
    assert film.read_bgra8().tobytes() == obgra.tobytes()
    assert ofilm.mean() > 0.05
    film.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rank_world", [(0, 1), (1, 3)])
def test_fused_nee_equals_the_wavefront_nee_pipeline(pt, gpu_ctx, cornell_gpu, rank_world):
    """More slots than the grid has lanes (lanes take new slots): FUSED | NEE == PIPELINE_WAVEFRONT_NEE in film and rays, also for a rank."""
    rank, world = rank_world
    kw = dict(spp_per_frame=32, max_depth=8, rank=rank, world=world)
    wf, wb, ws = _render(pt, gpu_ctx, cornell_gpu, 320, 180, 2, pt.PIPELINE_WAVEFRONT_NEE, **kw)
    ff, fb, fs = _render(pt, gpu_ctx, cornell_gpu, 320, 180, 2, pt.PIPELINE_FUSED, pt.FLAG_NEE, **kw)
    assert ws.pipeline == pt.PIPELINE_WAVEFRONT_NEE and fs.pipeline == pt.PIPELINE_FUSED
    assert fs.rays == ws.rays
    assert ff.tobytes() == wf.tobytes() and fb.tobytes() == wb.tobytes()
    # the reference estimator's film is another one (the flag is not ignored)
    rf, _, _ = _render(pt, gpu_ctx, cornell_gpu, 320, 180, 2, pt.PIPELINE_FUSED, **kw)
    assert rf.tobytes() != ff.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["depth1", "depth2", "no_lights", "many_lights"])
def test_fused_nee_edge_cases(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, cornell_arrays, case):
    """max_depth 1 (no shadow rays: rays == camera rays), max_depth 2, a Cornell box without emitters (n_lights == 0: no shadow ray),
    and a small soup where a third of the triangles emit that the fused plan still takes."""
    w, h = 64, 48
    kw = dict(width=w, height=h, spp_per_frame=8, max_depth=8)
    gs, osc, owned = cornell_gpu, cornell_oracle, False
    if case == "depth1":
        kw["max_depth"] = 1
    elif case == "depth2":
        kw["max_depth"] = 2
    elif case == "no_lights":
        v, i, f = cornell_arrays
        f = np.array(f, np.float32).reshape(-1, 6)
        f[:, 3:] = 0.0
        f = f.reshape(-1)
        gs, osc, owned = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f), True
    else:
        # the fused class ends near 204 triangles (shading tables <= 16 KB) and at a stack bound of 16: the first of these soups its plan takes
        film = pt.Film(gpu_ctx, w, h)
        for n, spread in ((150, 0.1), (150, 0.05), (120, 0.05), (96, 0.05)):
            v, i, f = _soup(n, 11, 1.0 / 3.0, spread)
            gs = pt.Scene(gpu_ctx, v, i, f)
            try:
                pt.render_prepare(gs, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_NEE, **kw))
                break
            except pt.PtError:
                gs.close()
                gs = None
        film.close()
        assert gs is not None, "no soup of the fused class"
        assert (np.asarray(f).reshape(-1, 6)[:, 3:].max(1) > 0).sum() >= n // 5
        osc, owned = orc.Scene(v, i, f), True
    ofilm, obgra, orays = _oracle_nee(orc, osc, 2, **kw)
    film, bgra, st = _render(pt, gpu_ctx, gs, w, h, 2, pt.PIPELINE_FUSED, pt.FLAG_NEE, **{k: v for k, v in kw.items() if k not in ("width", "height")})
    assert st.pipeline == pt.PIPELINE_FUSED
    assert st.rays == orays
    assert film.tobytes() == ofilm.tobytes() and bgra.tobytes() == obgra.tobytes()
    if case == "depth1":
        assert st.rays == w * h * 8 * 2   # camera rays only
    if owned:
        gs.close()


@pytest.mark.gpu
def test_auto_nee_picks_fused_or_wavefront_nee(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, cornell_arrays):
    """AUTO | NEE: the fused NEE kernel on the Cornell box; the wavefront NEE pipeline with ASYNC, with COUNT_VISITS, with a named
    closest-hit kernel, on 16 instances and on a 3000-triangle soup.  Every film equals the oracle's nee mode; pt_render_prepare
    reports the pipeline pt_render runs."""
    w, h = 48, 40
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=6)
    ofilm, _, orays = _oracle_nee(orc, cornell_oracle, 2, **kw)

    def run(scene, want_pipeline, want_film, want_rays, flags=0, **extra):
        film = pt.Film(gpu_ctx, w, h)
        p = pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_AUTO, flags=pt.FLAG_NEE | flags, **kw, **extra)
        gpu_ctx.reset_stats()
        pt.render_prepare(scene, film, p)
        assert gpu_ctx.stats().pipeline == want_pipeline, (flags, extra)
        gpu_ctx.reset_stats()
        pt.render(scene, film, p)
        if flags & pt.FLAG_ASYNC:
            gpu_ctx.sync()
        st = gpu_ctx.stats()
        assert st.pipeline == want_pipeline, (flags, extra)
        assert film.read_f32().tobytes() == want_film.tobytes(), (flags, extra)
        if not flags & pt.FLAG_ASYNC:
            assert st.rays == want_rays, (flags, extra)
        film.close()

    run(cornell_gpu, pt.PIPELINE_FUSED, ofilm, orays)
    run(cornell_gpu, pt.PIPELINE_WAVEFRONT_NEE, ofilm, orays, flags=pt.FLAG_ASYNC)
    run(cornell_gpu, pt.PIPELINE_WAVEFRONT_NEE, ofilm, orays, flags=pt.FLAG_COUNT_VISITS)
    run(cornell_gpu, pt.PIPELINE_WAVEFRONT_NEE, ofilm, orays, extend=pt.EXTEND_HBM)
    inst = pt.Scene(gpu_ctx, *cornell_arrays)
    oinst = orc.Scene(*cornell_arrays)
    grid = pt.cornell_grid_instances()[:16]
    inst.set_instances(grid)
    oinst.set_instances(grid)
    cam = dict(cam_origin=(-0.88, -1.9, 0.5), cam_target=(-0.88, -1.9, 0.0))
    ifilm, _, irays = _oracle_nee(orc, oinst, 2, **kw, **cam)
    run(inst, pt.PIPELINE_WAVEFRONT_NEE, ifilm, irays, **cam)
    inst.close()
    v, i, f = _soup(3000, 5, 0.1)
    big, obig = pt.Scene(gpu_ctx, v, i, f), orc.Scene(v, i, f)
    bfilm, _, brays = _oracle_nee(orc, obig, 2, **kw)
    run(big, pt.PIPELINE_WAVEFRONT_NEE, bfilm, brays)
    big.close()


@pytest.mark.gpu
def test_wavefront_with_flag_nee_is_the_wavefront_nee_pipeline(pt, gpu_ctx, cornell_gpu):
    """WAVEFRONT | NEE (and WAVEFRONT_NEE | NEE) is PIPELINE_WAVEFRONT_NEE, bit for bit."""
    kw = dict(spp_per_frame=8, max_depth=8)
    a = _render(pt, gpu_ctx, cornell_gpu, 96, 64, 2, pt.PIPELINE_WAVEFRONT_NEE, **kw)
    for pipeline in (pt.PIPELINE_WAVEFRONT, pt.PIPELINE_WAVEFRONT_NEE):
        b = _render(pt, gpu_ctx, cornell_gpu, 96, 64, 2, pipeline, pt.FLAG_NEE, **kw)
        assert b[2].pipeline == pt.PIPELINE_WAVEFRONT_NEE and b[2].rays == a[2].rays
        assert b[0].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes()


@pytest.mark.gpu
def test_fused_nee_refusals(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, cornell_arrays):
    """FUSED | NEE with several sample groups, asynchronous, instrumented or on an instanced scene: PT_ERR_UNSUPPORTED; the film renders
    correctly afterwards."""
    w, h = 48, 40
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=6)
    film = pt.Film(gpu_ctx, w, h)
    bad = [dict(sample_groups=4), dict(flags=pt.FLAG_NEE | pt.FLAG_ASYNC), dict(flags=pt.FLAG_NEE | pt.FLAG_COUNT_VISITS)]
    for b in bad:
        p = dict(kw, pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_NEE)
        p.update(b)
        with pytest.raises(pt.PtError) as e:
            pt.render(cornell_gpu, film, pt.default_params(**p))
        assert e.value.status == 5, b
    inst = pt.Scene(gpu_ctx, *cornell_arrays)
    inst.set_instances(pt.cornell_grid_instances()[:16])
    with pytest.raises(pt.PtError) as e:
        pt.render(inst, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_NEE, **kw))
    assert e.value.status == 5
    inst.close()
    ofilm, obgra, orays = _oracle_nee(orc, cornell_oracle, 2, **kw)
    film.clear()
    gpu_ctx.reset_stats()
    pt.render(cornell_gpu, film, pt.default_params(frame=0, frame_count=2, pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_NEE, **kw))
    assert gpu_ctx.stats().rays == orays
    assert film.read_f32().tobytes() == ofilm.tobytes() and film.read_bgra8().tobytes() == obgra.tobytes()
    film.close()


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [dict(cull=0), dict(fused_subject=0), dict(refill=1), dict(refill=64)])
def test_fused_nee_tuning_changes_no_bit(pt, orc, gpu_ctx, cornell_gpu, cornell_oracle, knobs):
    """The camera-ray cull, the hand-out order and the shade block's refill threshold change no bit of the NEE film or ray count."""
    w, h = 64, 48
    kw = dict(width=w, height=h, spp_per_frame=4, max_depth=8)
    ofilm, obgra, orays = _oracle_nee(orc, cornell_oracle, 2, **kw)
    old = gpu_ctx.set_tuning(**knobs)
    try:
        film, bgra, st = _render(pt, gpu_ctx, cornell_gpu, w, h, 2, pt.PIPELINE_FUSED, pt.FLAG_NEE, spp_per_frame=4, max_depth=8)
    finally:
        gpu_ctx.set_tuning(**old)
    assert st.pipeline == pt.PIPELINE_FUSED and st.rays == orays, knobs
    assert film.tobytes() == ofilm.tobytes() and bgra.tobytes() == obgra.tobytes(), knobs
