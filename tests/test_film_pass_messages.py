"""The text of every refusal of the film passes (pt_film_denoise / _variance / _history, pt_film_reproject / _motion, pt_film_motion and the
optional planes M, L, Q), as pt_last_error returns it.  The *_errors tests of each pass hold the status codes; this one holds the words, so
that the validation the passes share cannot reword one of them or change which check fires first.  The expected strings are the ones the
passes carried when each had its own copy of the checks."""
import pytest

W, H = 48, 40

GUIDES = "the film has no guide buffers: pt_film_enable_aov (and pt_render_aov) first"
NO_M = "the film has no second-moment plane: pt_film_enable_moments before the frames are rendered"
NO_M_READ = "the film has no second-moment plane: pt_film_enable_moments first"
NO_L = "the film has no history-length plane: pt_film_enable_history first"
NO_L_DENOISE = "the film has no history-length plane: pt_film_enable_history (and pt_film_reproject) first"
NO_Q = "the film has no motion plane: pt_film_enable_motion first"
NO_Q_REPROJECT = "the film has no motion plane: pt_film_enable_motion (and pt_film_motion) first"
SIGMAS3 = ".sigma_normal / sigma_depth / sigma_color must be finite and > 0"


def _film(pt, ctx, w=W, h=H, aov=True, m=True, l=True, q=True):
    f = pt.Film(ctx, w, h)
    if aov:
        f.enable_aov()
    if m:
        f.enable_moments()
    if l:
        f.enable_history()
    if q:
        f.enable_motion()
    return f


@pytest.mark.gpu
def test_every_refusal_says_what_it_said(pt, gpu_ctx, cornell_arrays):
    lib = pt.lib_amd()
    nan = float("nan")
    sc = pt.Scene(gpu_ctx, *cornell_arrays)
    ctx2 = pt.Context(0)
    buf = pt.DeviceBuffer(gpu_ctx, 16 * W * H + 16)
    films = dict(full=_film(pt, gpu_ctx), no_g=_film(pt, gpu_ctx, aov=False), no_m=_film(pt, gpu_ctx, m=False), no_l=_film(pt, gpu_ctx, l=False),
                 no_q=_film(pt, gpu_ctx, q=False), small=_film(pt, gpu_ctx, h=H - 1), foreign=_film(pt, ctx2))
    full, no_g, no_m, no_l, no_q, small, foreign = (films[k] for k in ("full", "no_g", "no_m", "no_l", "no_q", "small", "foreign"))

    def reserved(make, call):
        p = make()
        p.reserved[len(p.reserved) - 1] = 1
        return lambda: call(p)

    def zero_sigma_too(p):
        p.sigma_depth = 0.0
        full.denoise(params=p)

    def raw(fn, *args):   # a call the Python mirror cannot make (a null target): the status raised as the mirror raises it
        def call():
            rc = fn(*args)
            if rc != 0:
                raise pt.PtError(rc, "")
        return call

    table = [
        # a film without its guides, for every pass that reads them
        (lambda: no_g.denoise(), GUIDES),
        (lambda: no_g.denoise_variance(), GUIDES),
        (lambda: no_g.denoise_history(), GUIDES),
        (lambda: no_g.reproject(None), GUIDES),
        (lambda: no_g.reproject_motion(None), GUIDES),
        (lambda: no_g.motion(sc), GUIDES),
        (lambda: full.reproject(no_g), "prev has no guide buffers: pt_film_enable_aov (and pt_render_aov) first"),
        # ... without M
        (lambda: no_m.denoise_variance(), NO_M),
        (lambda: no_m.denoise_history(), NO_M),
        (lambda: no_m.read_moments(), NO_M_READ),
        # ... without L
        (lambda: no_l.denoise_history(), NO_L_DENOISE),
        (lambda: no_l.reproject(None), NO_L),
        (lambda: no_l.reproject_motion(None), NO_L),
        (lambda: no_l.read_history(), NO_L),
        (lambda: full.reproject(no_l), "prev has no history-length plane: pt_film_enable_history first"),
        # ... without Q
        (lambda: no_q.reproject_motion(None), NO_Q_REPROJECT),
        (lambda: no_q.motion(sc), NO_Q),
        (lambda: no_q.read_motion(), NO_Q),
        # a plane the film has already; a caller's Q that is not 16-byte aligned
        (lambda: full.enable_moments(), "the film already has a second-moment plane"),
        (lambda: full.enable_history(), "the film already has a history-length plane"),
        (lambda: full.enable_motion(), "the film already has a motion plane"),
        (lambda: no_q.enable_motion(buf.ptr + 4), "pt_film_enable_motion: the plane must be 16-byte aligned"),
        # null read targets (pt_film_read_moments takes a null plane: it is in the accepted calls below)
        (raw(lib.pt_film_read_history, full.h, None), "null argument"),
        (raw(lib.pt_film_read_motion, full.h, None), "null argument"),
        # iterations and sigmas, for each of the three denoisers
        (lambda: full.denoise(iterations=0), "pt_denoise_params.iterations must be in 1..8"),
        (lambda: full.denoise(iterations=9), "pt_denoise_params.iterations must be in 1..8"),
        (lambda: full.denoise_variance(iterations=0), "pt_denoise_variance_params.iterations must be in 1..8"),
        (lambda: full.denoise_variance(iterations=9), "pt_denoise_variance_params.iterations must be in 1..8"),
        (lambda: full.denoise_history(iterations=0), "pt_denoise_history_params.iterations must be in 1..8"),
        (lambda: full.denoise_history(iterations=9), "pt_denoise_history_params.iterations must be in 1..8"),
        (lambda: full.denoise(sigma_normal=0.0), "pt_denoise_params.sigma_normal / sigma_depth must be finite and > 0"),
        (lambda: full.denoise(sigma_depth=0.0), "pt_denoise_params.sigma_normal / sigma_depth must be finite and > 0"),
        (lambda: full.denoise_variance(sigma_color=0.0), "pt_denoise_variance_params" + SIGMAS3),
        (lambda: full.denoise_variance(sigma_normal=0.0), "pt_denoise_variance_params" + SIGMAS3),
        (lambda: full.denoise_history(sigma_depth=0.0), "pt_denoise_history_params" + SIGMAS3),
        (lambda: full.denoise_history(sigma_color=nan), "pt_denoise_history_params" + SIGMAS3),
        # which check fires first when several fail: the planes, then iterations, then the sigmas, then reserved
        (lambda: no_m.denoise_variance(iterations=0, sigma_color=0.0), NO_M),
        (lambda: full.denoise_variance(iterations=0, sigma_color=0.0), "pt_denoise_variance_params.iterations must be in 1..8"),
        (reserved(pt.denoise_default_params, zero_sigma_too), "pt_denoise_params.sigma_normal / sigma_depth must be finite and > 0"),
        (lambda: full.denoise_variance(), "pt_film_denoise_variance: a variance estimate needs a film of at least 2 frames (params.frames, or what pt_render recorded)"),
        # pt_denoise_history_params' own fields
        (lambda: full.denoise_history(min_history=0.5), "pt_denoise_history_params.min_history must be finite and in 1..65536"),
        (lambda: full.denoise_history(min_history=nan), "pt_denoise_history_params.min_history must be finite and in 1..65536"),
        (lambda: full.denoise_history(n_max=1.0), "pt_denoise_history_params.n_max must be finite and >= 2"),
        (lambda: full.denoise_history(step_frames=0), "pt_denoise_history_params.step_frames must be >= 1"),
        (lambda: full.denoise_history(min_history=1.0, step_frames=1),
         "pt_denoise_history_params: min_history * step_frames must be >= 2 (a variance estimate needs two frames)"),
        # pt_reproject_params, through both entry points
        (lambda: full.reproject(None, dict(cam_origin=(nan, 0.0, 0.0))), "pt_reproject_params: the cameras must be finite"),
        (lambda: full.reproject_motion(None, None, dict(cam_target=(0.0, float("inf"), 0.0))), "pt_reproject_params: the cameras must be finite"),
        (lambda: full.reproject(None, gain=0.0), "pt_reproject_params.gain must be finite and > 0"),
        (lambda: full.reproject(None, alpha=1.5), "pt_reproject_params.alpha must be in [0, 1]"),
        (lambda: full.reproject(None, depth_tol=0.0), "pt_reproject_params.depth_tol must be finite and > 0"),
        (lambda: full.reproject(None, normal_min=2.0), "pt_reproject_params.normal_min must be in [-1, 1]"),
        (lambda: full.reproject(None, max_history=0), "pt_reproject_params.max_history must be in 1..65535"),
        (lambda: full.reproject_motion(None, max_history=65536), "pt_reproject_params.max_history must be in 1..65535"),
        (lambda: full.reproject(None, flags=2), "pt_reproject_params.flags: unknown bits"),
        # the two films of a reprojection
        (lambda: full.reproject(full), "pt_film_reproject: prev is the film itself (the history is read while the film is rewritten: two films, ping-ponged)"),
        (lambda: full.reproject_motion(full), "pt_film_reproject: prev is the film itself (the history is read while the film is rewritten: two films, ping-ponged)"),
        (lambda: full.reproject(small), "film and prev differ in size"),
        (lambda: full.reproject(foreign), "film and prev belong to different contexts"),
        (lambda: full.reproject(no_m), "exactly one of film and prev has a second-moment plane: both or neither"),
        (lambda: no_m.reproject(full), "exactly one of film and prev has a second-moment plane: both or neither"),
        # pt_film_motion (the scene has no snapshot yet: that check stands behind the film's and in front of the parameters')
        (lambda: foreign.motion(sc), "scene and film belong to different contexts"),
        (lambda: full.motion(sc), "the scene has no previous geometry: pt_scene_snapshot_previous first"),
        (lambda: full.motion(sc, bary_slack=-0.5), "the scene has no previous geometry: pt_scene_snapshot_previous first"),
    ]
    after_snapshot = [
        (lambda: full.motion(sc, dict(cam_origin=(nan, 0.0, 0.0))), "pt_motion_params: the camera must be finite"),
        (lambda: full.motion(sc, bary_slack=-0.5), "pt_motion_params.bary_slack must be finite and >= 0"),
        (lambda: full.motion(sc, bary_slack=nan), "pt_motion_params.bary_slack must be finite and >= 0"),
        # a nonzero reserved word, for each of the five structs
        (reserved(pt.denoise_default_params, lambda p: full.denoise(params=p)), "pt_denoise_params.reserved must be 0"),
        (reserved(pt.denoise_variance_default_params, lambda p: full.denoise_variance(params=p)), "pt_denoise_variance_params.reserved must be 0"),
        (reserved(pt.denoise_history_default_params, lambda p: full.denoise_history(params=p)), "pt_denoise_history_params.reserved must be 0"),
        (reserved(pt.reproject_default_params, lambda p: full.reproject(None, params=p)), "pt_reproject_params.reserved must be 0"),
        (reserved(pt.reproject_default_params, lambda p: full.reproject_motion(None, params=p)), "pt_reproject_params.reserved must be 0"),
        (reserved(pt.motion_default_params, lambda p: full.motion(sc, params=p)), "pt_motion_params.reserved must be 0"),
    ]

    def check(rows, part):
        for k, (call, want) in enumerate(rows):
            with pytest.raises(pt.PtError) as e:
                call()
            got = lib.pt_last_error(gpu_ctx.h).decode()   # (every call above reports in gpu_ctx: pt_film_motion in its scene's context, the rest in `film`'s)
            assert e.value.status == 1 and got == want, (part, k, e.value.status, got, want)

    try:
        check(table, "table")
        sc.snapshot_previous()
        check(after_snapshot, "after the snapshot")
        # nothing above gave a film a plane or took one away, and the accepted forms still pass
        assert lib.pt_film_read_moments(full.h, None, None) == 0
        no_q.enable_motion(buf.ptr)
        assert no_q.read_motion().tobytes() == bytes(16 * W * H)
        assert full.read_history().tobytes() == bytes(4 * W * H)
    finally:
        for f in films.values():
            f.close()
        buf.close()
        sc.close()
        ctx2.close()
