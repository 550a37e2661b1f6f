"""The device buffers of a scene (csrc/scene_build.hip ptb_scene_buffers / ptb_scene_alloc, DESIGN.md section 5 "Scene buffers"): every one of
them goes back to the device when the scene is closed, and a set that cannot be allocated -- the surface-area tree, the instance set, the
previous geometry -- leaves the scene as it was.  The failures are injected (pt_tuning.fail_rebuild): the call returns PT_ERR_OOM before it
allocates, no device fault is involved."""
import numpy as np
import pytest

from test_motion import BOX_MOVE, _moved_box

pytestmark = pytest.mark.gpu

W, H = 64, 48
KW = dict(width=W, height=H, spp_per_frame=2, max_depth=3)
OOM = 4


def _two_instances():
    m = np.zeros((2, 3, 4), np.float32)
    m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = 1.0
    m[1, 0, 3] = 2.5
    return m


def _film_bytes(pt, sc, film, pipeline=None):
    film.clear()
    pt.render(sc, film, pt.default_params(frame=0, frame_count=1, **({} if pipeline is None else {"pipeline": pipeline}), **KW))
    return film.read_f32().tobytes()


def _fails_with_oom(pt, ctx, call):
    old = ctx.set_tuning(fail_rebuild=1)
    try:
        with pytest.raises(pt.PtError) as e:
            call()
        assert e.value.status == OOM and "fail_rebuild" in str(e.value)
    finally:
        ctx.set_tuning(**old)


def test_every_scene_buffer_is_returned_on_close(pt, cornell_arrays):
    """One cycle reaches every lifetime of scene buffers and every lazily built one -- both BVH4s of a small scene, the instance set with
    its frame and emitter tables, the previous geometry (twice: the second replaces the first), a refit and a rebuild, the 8-wide nodes of
    a big scene on first request, a rebuild of its tree products, pt_trace's buffers -- and closes everything.  Pattern and threshold of
    test_no_device_memory_leak_over_object_lifecycles: a warm-up cycle, ten cycles, less than 8 MiB gone."""
    import torch
    torch.cuda.synchronize()
    v, i, f = cornell_arrays
    soup = pt.make_soup(2049)                 # one triangle over PT_SAH_MAX_TRIS: the smallest scene of the big-scene path
    rays = np.zeros((16, 6), np.float32); rays[:, 2] = 5; rays[:, 5] = -1

    def cycle():
        ctx = pt.Context(0)
        sc = pt.Scene(ctx, v, i, f)
        film = pt.Film(ctx, W, H)
        sc.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)
        sc.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)
        sc.set_instances(_two_instances())
        pt.render(sc, film, pt.default_params(pipeline=pt.PIPELINE_WAVEFRONT_NEE, frame=0, frame_count=1, **KW))   # d_lights_inst, d_inst_frame
        sc.snapshot_previous()
        sc.snapshot_previous()
        sc.update(_moved_box(v, BOX_MOVE), i, mode=pt.SCENE_UPDATE_REFIT)
        sc.update(v, i, mode=pt.SCENE_UPDATE_REBUILD)
        sc.read_bvh8()
        big = pt.Scene(ctx, *soup)
        big.read_bvh8()                                      # the 8-wide nodes and their tables, on first request
        big.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)        # a rebuild of the tree products
        big.trace(rays)
        big.close(); film.close(); sc.close(); ctx.close()

    cycle()                                   # first cycle pays one-time runtime allocations
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(10):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    print(f"free device memory: {free0} -> {free1} over 10 cycles ({(free0 - free1) / 2**20:.2f} MiB gone)")
    assert free0 - free1 < (8 << 20), f"leaked {(free0 - free1) / 2**20:.1f} MiB over 10 cycles"


def test_failed_surface_area_set_leaves_no_half_state(pt, gpu_ctx, cornell_arrays):
    """The surface-area tree is its nodes AND its leaf order.  A scene that holds neither (FAST_BUILD, then a rebuild) and cannot allocate
    them stays on the collapsed LBVH and renders what it rendered; the next request builds the tree a fresh scene has."""
    v, i, f = cornell_arrays
    sc, fresh = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v, i, f)
    film = pt.Film(gpu_ctx, W, H)
    try:
        sc.set_bvh_quality(pt.BVH_PREFER_FAST_BUILD)
        sc.update(v, i, mode=pt.SCENE_UPDATE_REBUILD)      # (the surface-area tree is not built again at FAST_BUILD)
        want = _film_bytes(pt, sc, film)
        _fails_with_oom(pt, gpu_ctx, lambda: sc.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE))
        assert sc.info().bvh4_builder == 0
        assert _film_bytes(pt, sc, film) == want
        sc.set_bvh_quality(pt.BVH_PREFER_FAST_TRACE)
        assert sc.info().bvh4_builder == fresh.info().bvh4_builder == 1
        assert sc.read_bvh4().tobytes() == fresh.read_bvh4().tobytes()
        assert _film_bytes(pt, sc, film) == want
    finally:
        film.close(); fresh.close(); sc.close()


def test_failed_instance_set_leaves_a_single_level_scene(pt, gpu_ctx, cornell_arrays):
    """Nothing of an instance set hangs on the scene before all of it exists: a set that cannot be allocated leaves the scene single-level,
    rendering what it rendered, and the next pt_scene_set_instances gives what a fresh scene gets."""
    v, i, f = cornell_arrays
    sc, fresh = pt.Scene(gpu_ctx, v, i, f), pt.Scene(gpu_ctx, v, i, f)
    film = pt.Film(gpu_ctx, W, H)
    try:
        want = _film_bytes(pt, sc, film)
        _fails_with_oom(pt, gpu_ctx, lambda: sc.set_instances(_two_instances()))
        info = sc.info()
        assert info.n_instances == 0 and info.n_tlas_nodes == 0
        assert _film_bytes(pt, sc, film) == want
        sc.set_instances(_two_instances())
        fresh.set_instances(_two_instances())
        assert sc.info().n_instances == 2 and sc.info().n_tlas_nodes == fresh.info().n_tlas_nodes
        assert _film_bytes(pt, sc, film) == _film_bytes(pt, fresh, film)
    finally:
        film.close(); fresh.close(); sc.close()


def test_failed_snapshot_keeps_the_old_one(pt, gpu_ctx, cornell_arrays):
    """pt_scene_snapshot_previous makes its new copies before it lets go of the old ones: a call that cannot allocate them leaves the previous
    geometry -- its bytes in pt_scene_info.device_bytes, what pt_film_motion computes from it -- as it was."""
    v, i, f = cornell_arrays
    sc = pt.Scene(gpu_ctx, v, i, f)
    film = pt.Film(gpu_ctx, W, H)
    try:
        film.enable_aov()
        film.enable_motion()
        sc.snapshot_previous()
        sc.update(_moved_box(v, BOX_MOVE), i, mode=pt.SCENE_UPDATE_REFIT)
        pt.render_aov(sc, film, pt.default_params(frame=0, frame_count=1, **KW))
        film.motion(sc)
        q = film.read_motion()
        assert q.any()
        held = sc.info().device_bytes
        _fails_with_oom(pt, gpu_ctx, sc.snapshot_previous)
        assert sc.info().device_bytes == held
        film.motion(sc)
        assert film.read_motion().tobytes() == q.tobytes()
    finally:
        film.close(); sc.close()
