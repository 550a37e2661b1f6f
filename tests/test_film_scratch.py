"""The device scratch that hangs on a film -- the wavefront workspace, the NEE shadow queue, the ray-sort scratch, the guide buffers' ray
scratch, the denoiser's planes (csrc/film_work.hip pt_scratch_alloc / pt_scratch_free, DESIGN.md section 4 "Film scratch"): all of it
goes back to the device when the film is closed, and pt_stats.workspace_bytes counts what include/pt_api.h says it counts."""
import pytest

from test_gpu_parity import _soup

pytestmark = pytest.mark.gpu

KW = dict(spp_per_frame=4, max_depth=4)


def test_every_film_scratch_is_returned_on_close(pt, cornell_arrays):
    """One cycle makes every kind of film scratch there is -- shape buffers with accumulators and with term logs + spill pool, the shadow
    queue, the ray-sort scratch, the guide buffers' tile list / counters / ray scratch, both denoisers' planes -- and closes everything.
    Pattern and threshold of test_no_device_memory_leak_over_object_lifecycles: a warm-up cycle, ten cycles, less than 8 MiB gone."""
    import torch
    torch.cuda.synchronize()
    soup = _soup(30000, 17, spread=0.05)

    def cycle():
        ctx = pt.Context(0)
        sc = pt.Scene(ctx, *cornell_arrays)
        film = pt.Film(ctx, 96, 56)
        film.enable_aov()
        film.enable_moments()
        kw = dict(width=96, height=56, **KW)
        pt.render(sc, film, pt.default_params(pipeline=pt.PIPELINE_WAVEFRONT_NEE, frame=0, frame_count=2, **kw))               # shadow queue
        pt.render(sc, film, pt.default_params(pipeline=pt.PIPELINE_WAVEFRONT, frame=2, frame_count=1, sample_groups=2, **kw))  # term logs, spill pool
        pt.render_aov(sc, film, pt.default_params(pipeline=pt.PIPELINE_WAVEFRONT, **kw))                                       # ray scratch
        pt.render_aov(sc, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, **kw))
        film.denoise()
        film.denoise_variance()
        big = pt.Scene(ctx, *soup)
        film2 = pt.Film(ctx, 160, 96)
        pt.render(big, film2, pt.default_params(width=160, height=96, extend=pt.EXTEND_HBM, flags=pt.FLAG_SORT_RAYS, **KW))     # sort scratch
        film2.close(); big.close(); film.close(); sc.close(); ctx.close()

    cycle()                                   # first cycle pays one-time runtime allocations
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(10):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), f"leaked {(free0 - free1) / 2**20:.1f} MiB over 10 cycles"


def test_workspace_bytes_and_paths_are_what_the_header_says(pt, gpu_ctx, cornell_gpu):
    """pt_stats.workspace_bytes = the film's wavefront workspace + its shadow queue + the context's stack-spill area: the same shape through
    the NEE pipeline on a fresh film holds exactly the shadow queue more, 16 + 8 + 16 + 4 + 4 + 16 = 64 B for each of the 64 slots of the 84
    tiles of a 96 x 56 film.  pt_stats.paths counts the samples of the pixels INSIDE the image: a 52 x 36 film has cut tiles in its last
    column and row, and the three ranks of world 3 start every sample of it exactly once."""
    kw = dict(width=96, height=56, frame=0, frame_count=1, frames_in_flight=1, **KW)
    a, b = pt.Film(gpu_ctx, 96, 56), pt.Film(gpu_ctx, 96, 56)
    try:
        pt.render(cornell_gpu, a, pt.default_params(pipeline=pt.PIPELINE_WAVEFRONT, sample_groups=1, **kw))
        plain = gpu_ctx.stats().workspace_bytes
        pt.render(cornell_gpu, b, pt.default_params(pipeline=pt.PIPELINE_WAVEFRONT_NEE, **kw))
        nee = gpu_ctx.stats().workspace_bytes
        print(f"workspace_bytes: wavefront {plain}, NEE {nee}, difference {nee - plain} (shadow queue: {64 * 84 * 64})")
        assert nee == plain + 64 * 84 * 64
    finally:
        a.close(); b.close()
    film = pt.Film(gpu_ctx, 52, 36)
    try:
        frames, paths = 2, []
        for rank in range(3):
            gpu_ctx.reset_stats()
            pt.render(cornell_gpu, film, pt.default_params(width=52, height=36, frame=0, frame_count=frames, rank=rank, world=3, **KW))
            paths.append(gpu_ctx.stats().paths)
        print(f"paths per rank {paths}, sum {sum(paths)}, pixels x spp x frames {52 * 36 * KW['spp_per_frame'] * frames}")
        assert sum(paths) == 52 * 36 * KW["spp_per_frame"] * frames
    finally:
        film.close()
