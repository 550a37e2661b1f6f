"""MI355X-native wavefront path tracer -- Python mirror of the C-ABI (include/pt_api.h, pt_host.h).

The package directory name contains '-', so import it with
    importlib.import_module("single-file-vulkan-pathtracing_amd")
(`__graft_entry__.py`, `bench.py` and the tests do exactly that).

This module only loads the in-tree shared libraries and forwards to them:
    libpt_amd.so   hand-written HIP kernels for gfx950 + the pt_* entry points
    libpt_host.so  C++20 host code: OBJ/MTL ingest (reference loadFromFile, main.cpp:28-58), image output
There is NO CPU fallback: without the HIP library, or without a GPU, every compute call raises.
Names follow the reference: Scene = vertex/index/face buffers + acceleration structure
(main.cpp:492-538), Film = the storage image (main.cpp:481-484), render() = pushConstants +
traceRaysKHR (main.cpp:656-659).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(_HERE)
ASSET_CORNELL = os.path.join(REPO, "assets", "CornellBox-Original.obj")

PT_OK = 0
STATUS_NAMES = {0: "PT_OK", 1: "PT_ERR_INVALID_ARG", 2: "PT_ERR_NO_DEVICE", 3: "PT_ERR_HIP", 4: "PT_ERR_OOM",
                5: "PT_ERR_UNSUPPORTED"}
PIPELINE_WAVEFRONT = 0
PIPELINE_WAVEFRONT_NEE = 1
PIPELINE_FUSED = 2
PIPELINE_AUTO = 3
PIPELINE_NAMES = {0: "wavefront", 1: "wavefront_nee", 2: "fused", 3: "auto"}
FLAG_PROFILE = 1
FLAG_COUNT_VISITS = 2
FLAG_ASYNC = 4
FLAG_SORT_RAYS = 8
FLAG_NO_SORT_RAYS = 16
FLAG_NEE = 32         # the NEE estimator on any pipeline value (include/pt_api.h PT_FLAG_NEE)
EXTEND_AUTO, EXTEND_LDS, EXTEND_HBM, EXTEND_HBM8 = 0, 2, 3, 4
EXTEND_FLAT = 1   # deprecated: the brute-force loop was removed in API version 5 (PT_ERR_UNSUPPORTED); the name is kept for source compatibility
BVH_PREFER_FAST_TRACE, BVH_PREFER_FAST_BUILD = 0, 1
SCENE_UPDATE_REFIT, SCENE_UPDATE_REBUILD = 0, 1   # pt_scene_update modes
EXTEND_NAMES = {2: "BVH4, scene staged in LDS", 3: "BVH4, scene in HBM/L2",
                4: "8-wide tree (64-B nodes with byte planes, one stack entry per node), scene in HBM/L2"}
MISS = 0xFFFFFFFF


class PtError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class Params(C.Structure):
    _fields_ = [
        ("frame", C.c_int32), ("frame_count", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
        ("spp_per_frame", C.c_uint32), ("max_depth", C.c_uint32), ("tmin", C.c_float), ("tmax", C.c_float),
        ("cam_origin", C.c_float * 3), ("cam_target", C.c_float * 3), ("env", C.c_float * 3),
        ("rank", C.c_uint32), ("world", C.c_uint32), ("pipeline", C.c_uint32),
        ("frames_in_flight", C.c_uint32), ("flags", C.c_uint32), ("extend", C.c_uint32),
        ("sample_groups", C.c_uint32),
    ]


class SceneInfo(C.Structure):
    _fields_ = [("n_tris", C.c_uint32), ("n_nodes", C.c_uint32), ("bvh_height", C.c_uint32),
                ("n_wide_nodes", C.c_uint32), ("n_instances", C.c_uint32), ("n_tlas_nodes", C.c_uint32),
                ("leaf_max", C.c_uint32), ("bvh4_builder", C.c_uint32),
                ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3), ("build_ms", C.c_float),
                ("device_bytes", C.c_uint64), ("n_wide8_nodes", C.c_uint32), ("wide8_levels", C.c_uint32),
                ("device_bytes8", C.c_uint64), ("tree_area_lbvh", C.c_float), ("tree_area_ploc", C.c_float)]


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("paths", C.c_uint64), ("rounds", C.c_uint32),
                ("launches_extend", C.c_uint32), ("launches_shade", C.c_uint32), ("launches_other", C.c_uint32),
                ("ms_total", C.c_float), ("ms_extend", C.c_float), ("ms_shade", C.c_float),
                ("extend_variant", C.c_uint32), ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64),
                ("frames_in_flight", C.c_uint32), ("sample_groups", C.c_uint32),
                ("node_steps", C.c_uint64), ("tri_steps", C.c_uint64),
                ("redone_batches", C.c_uint32), ("pipelines", C.c_uint32),
                ("wave_refills", C.c_uint64), ("wave_pops", C.c_uint64), ("wave_hit_blocks", C.c_uint64),
                ("wave_finishes", C.c_uint64), ("wave_iterations", C.c_uint64),
                ("leaf_lanes", C.c_uint64), ("pop_lanes", C.c_uint64), ("hit_lanes", C.c_uint64),
                ("enter_steps", C.c_uint64), ("enter_lanes", C.c_uint64), ("workspace_bytes", C.c_uint64),
                ("pipeline", C.c_uint32), ("tail_samples", C.c_uint32), ("rays_culled", C.c_uint64)]


TUNING_NAMES = ["refill", "lds_stack", "extend_blocks", "pipes", "stagger", "sort_bits", "pair_leaves", "pair_kernel", "topdown4",
                "rec64", "inst16", "inst16_blocks", "enter_min", "node_yield", "tlas_lds_kb", "term_ocap", "term_spill", "mem_budget_mb",
                "hbm8", "ploc_radius", "leaf_min", "tri_enter", "tri_stay", "inst_frames", "tlas_ploc", "ploc_adopt_pct", "fail_rebuild", "fused_tail", "fused_subject", "cull"]


class Tuning(C.Structure):
    """include/pt_api.h pt_tuning: speed knobs of a context, -1 = the built-in choice; never changes a result."""
    _fields_ = [(n, C.c_int32) for n in TUNING_NAMES] + [("reserved", C.c_int32 * 2)]


class DenoiseParams(C.Structure):
    """include/pt_api.h pt_denoise_params: the a-trous filter of pt_film_denoise."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("reserved", C.c_uint32 * 5)]


class DenoiseVarianceParams(C.Structure):
    """include/pt_api.h pt_denoise_variance_params: the variance-guided filter of pt_film_denoise_variance."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_color", C.c_float),
                ("frames", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class DenoiseHistoryParams(C.Structure):
    """include/pt_api.h pt_denoise_history_params: the variance-guided filter with a per-pixel variance, pt_film_denoise_history."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_color", C.c_float),
                ("min_history", C.c_float), ("n_max", C.c_float), ("step_frames", C.c_uint32), ("reserved", C.c_uint32 * 1)]


UPSAMPLE_SRC_FILM, UPSAMPLE_SRC_DENOISED = 0, 1   # include/pt_api.h PT_UPSAMPLE_SRC_*


class UpsampleParams(C.Structure):
    """include/pt_api.h pt_upsample_params: the guide-driven upsampling of pt_film_upsample."""
    _fields_ = [("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("source", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class AdaptiveParams(C.Structure):
    """include/pt_api.h pt_adaptive_params: which tiles pt_render_adaptive traces."""
    _fields_ = [("threshold", C.c_float), ("rel_floor", C.c_float), ("min_frames", C.c_uint32), ("max_frames", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class AdaptiveResult(C.Structure):
    """include/pt_api.h pt_adaptive_result: what the selection pass of pt_render_adaptive found."""
    _fields_ = [("tiles_total", C.c_uint32), ("tiles_selected", C.c_uint32), ("pixels_selected", C.c_uint64), ("max_error", C.c_float),
                ("select_ms", C.c_float), ("reserved", C.c_uint32 * 2)]


TRACE_CLOSEST, TRACE_ANY = 0, 1   # include/pt_api.h PT_TRACE_*: the query pt_trace_device answers
TRACE_ASYNC = 1                   # ... PT_TRACE_ASYNC: queue only, Context.sync() waits
TRACE_FUSED, TRACE_AUTO = 4, 8    # ... its form: the single kernel (or PT_ERR_UNSUPPORTED) | the library's choice; neither: the queues


class TraceDesc(C.Structure):
    """include/pt_api.h pt_trace_desc: a ray query on device buffers (pt_trace_device)."""
    _fields_ = [("d_rays6", C.c_void_p), ("d_tmax", C.c_void_p), ("d_hits", C.c_void_p), ("d_occluded", C.c_void_p),
                ("d_position", C.c_void_p), ("d_normal", C.c_void_p), ("d_albedo", C.c_void_p), ("d_emission", C.c_void_p),
                ("tmin", C.c_float), ("tmax", C.c_float), ("mode", C.c_uint32), ("extend", C.c_uint32), ("flags", C.c_uint32),
                ("chunk_rays", C.c_uint32), ("reserved", C.c_uint32 * 4)]


NEAREST_AUTO, NEAREST_LDS, NEAREST_GLOBAL = 0, 1, 2   # include/pt_api.h PT_NEAREST_*: the form pt_nearest_device takes
NEAREST_DTYPE = np.dtype([("prim", "<u4"), ("dist2", "<f4"), ("u", "<f4"), ("v", "<f4")])   # pt_nearest


class NearestDesc(C.Structure):
    """include/pt_api.h pt_nearest_desc: closest-point queries on device buffers (pt_nearest_device)."""
    _fields_ = [("d_points", C.c_void_p), ("d_max_dist", C.c_void_p), ("d_nearest", C.c_void_p), ("d_point", C.c_void_p),
                ("max_dist", C.c_float), ("form", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 5)]


CROSSINGS_AUTO, CROSSINGS_LDS, CROSSINGS_GLOBAL = 0, 1, 2   # include/pt_api.h PT_CROSSINGS_*: the form pt_crossings_device takes


class CrossingsDesc(C.Structure):
    """include/pt_api.h pt_crossings_desc: crossing counts and winding for rays on device buffers (pt_crossings_device)."""
    _fields_ = [("d_rays6", C.c_void_p), ("d_points", C.c_void_p), ("d_tmax", C.c_void_p), ("d_count", C.c_void_p), ("d_winding", C.c_void_p),
                ("direction", C.c_float * 3), ("tmin", C.c_float), ("tmax", C.c_float), ("form", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


# Scene.inside_tensors' directions, in this order: unit vectors (to rounding), none along an axis, none in a coordinate plane, no two with the
# same dominant axis among the first three.  A ray from a point is wrong about "inside" only where it passes through an edge or a vertex (the
# acceptance rule counts both triangles / the whole fan) or grazes the surface; different directions do so at different points.
INSIDE_DIRECTIONS = tuple(tuple(float(c) / float(np.sqrt(float(x * x + y * y + z * z))) for c in (x, y, z))
                          for x, y, z in ((3, 2, 1), (-2, 6, -3), (2, -3, 6), (-6, -2, 3), (1, -4, -8)))


RADIANCE_NEE, RADIANCE_ACCUMULATE = 1, 2   # include/pt_api.h PT_RADIANCE_*: the estimator and the store of pt_radiance_device
RADIANCE_FUSED, RADIANCE_AUTO = 8, 16      # ... its form: the single-kernel one (or PT_ERR_UNSUPPORTED) | the library's choice; neither: the wavefront form


class RadianceDesc(C.Structure):
    """include/pt_api.h pt_radiance_desc: path-traced radiance for rays on device buffers (pt_radiance_device)."""
    _fields_ = [("d_rays6", C.c_void_p), ("d_seeds", C.c_void_p), ("d_radiance", C.c_void_p), ("d_moment2", C.c_void_p),
                ("tmin", C.c_float), ("tmax", C.c_float), ("env", C.c_float * 3), ("spp", C.c_uint32), ("max_depth", C.c_uint32),
                ("frame", C.c_int32), ("index_base", C.c_uint32), ("flags", C.c_uint32), ("extend", C.c_uint32), ("chunk_rays", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


GUIDED_AUTO = 0          # include/pt_api.h PT_GUIDED_*: which form pt_render_guided takes
GUIDED_SINGLE_PASS = 1
GUIDED_TWO_CALLS = 2


class GuidedParams(C.Structure):
    """include/pt_api.h pt_guided_params: the form of pt_render_guided."""
    _fields_ = [("mode", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class GuidedResult(C.Structure):
    """include/pt_api.h pt_guided_result: which form ran, its fused launches, the device time of the guides' part."""
    _fields_ = [("single_pass", C.c_uint32), ("launches", C.c_uint32), ("guide_ms", C.c_float), ("reserved", C.c_uint32 * 5)]


REPROJECT_MATCH_ID = 1   # include/pt_api.h PT_REPROJECT_MATCH_ID


class ReprojectParams(C.Structure):
    """include/pt_api.h pt_reproject_params: the temporal accumulation step of pt_film_reproject."""
    _fields_ = [("cam_origin", C.c_float * 3), ("cam_target", C.c_float * 3), ("prev_cam_origin", C.c_float * 3), ("prev_cam_target", C.c_float * 3),
                ("gain", C.c_float), ("alpha", C.c_float), ("depth_tol", C.c_float), ("normal_min", C.c_float),
                ("max_history", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class MotionParams(C.Structure):
    """include/pt_api.h pt_motion_params: the camera of the guides pt_film_motion reads, and the barycentric slack."""
    _fields_ = [("cam_origin", C.c_float * 3), ("cam_target", C.c_float * 3), ("bary_slack", C.c_float), ("reserved", C.c_uint32 * 5)]


class HostScene(C.Structure):
    _fields_ = [("vertices", C.POINTER(C.c_float)), ("n_verts", C.c_uint32), ("indices", C.POINTER(C.c_uint32)),
                ("n_tris", C.c_uint32), ("faces", C.POINTER(C.c_float))]


# include/pt_api.h pt_fused_block, in order
FUSED_BLOCKS = ["ITER", "SHADE", "HIT", "MISS", "SURFACE", "ADD", "BOUNCE", "NEXT", "DONE", "HANDOUT", "DRAW", "TAKE", "CULLED", "PRIMARY", "SETUP",
                "NODE", "POP", "LEAF", "DIV", "FINISH", "TRACE", "SPAWN", "PTARGET", "PDIR", "POPTOP", "SKIP"]
# include/pt_api.h PT_AOV_*: the guide planes of pt_render_aov and their (trailing shape, dtype)
AOV_ALBEDO, AOV_NORMAL, AOV_EMISSION, AOV_DEPTH, AOV_ALPHA, AOV_ID, AOV_COUNT = 0, 1, 2, 3, 4, 5, 6
AOV_SHAPES = {AOV_ALBEDO: ((3,), np.float32), AOV_NORMAL: ((3,), np.float32), AOV_EMISSION: ((3,), np.float32),
              AOV_DEPTH: ((), np.float32), AOV_ALPHA: ((), np.float32), AOV_ID: ((2,), np.uint32)}
# include/pt_api.h PT_PLANES_*: the plane sets of film_pack_planes / film_unpack_planes / Comm.present_planes
PLANES_FILM, PLANES_GUIDES, PLANES_MOMENTS, PLANES_HISTORY, PLANES_COUNTS, PLANES_MOTION, PLANES_ALL = 1, 2, 4, 8, 16, 32, 63
HIT_DTYPE = np.dtype([("prim", "<u4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("inst", "<u4")])

# every symbol include/pt_api.h and include/pt_host.h declare
API_SYMBOLS = ["pt_ctx_create", "pt_ctx_destroy", "pt_last_error", "pt_sync", "pt_scene_create", "pt_scene_destroy",
               "pt_scene_set_instances", "pt_scene_set_bvh_quality", "pt_scene_update", "pt_scene_create_device", "pt_scene_update_device",
               "pt_scene_set_instances_device", "pt_scene_set_faces", "pt_scene_set_faces_device", "pt_scene_read_faces",
               "pt_scene_get_info", "pt_scene_read_bvh", "pt_scene_read_bvh4", "pt_scene_read_bvh8", "pt_film_create", "pt_film_create_external", "pt_film_clear",
               "pt_film_read_f32", "pt_film_read_bgra8", "pt_film_destroy", "pt_params_default", "pt_render",
               "pt_render_prepare", "pt_trace", "pt_film_enable_aov", "pt_render_aov", "pt_film_read_aov",
               "pt_denoise_params_default", "pt_film_denoise", "pt_film_read_denoised",
               "pt_film_enable_moments", "pt_film_read_moments", "pt_denoise_variance_params_default", "pt_film_denoise_variance",
               "pt_film_enable_history", "pt_film_read_history", "pt_reproject_params_default", "pt_film_reproject",
               "pt_get_stats", "pt_reset_stats", "pt_get_block_counts",
               "pt_comm_unique_id", "pt_comm_create", "pt_comm_ranks", "pt_comm_destroy", "pt_film_present",
               "pt_film_tile_count", "pt_film_pack_tiles", "pt_film_unpack_tiles",
               "pt_film_planes_words", "pt_film_pack_planes", "pt_film_unpack_planes", "pt_film_present_planes",
               "pt_device_alloc", "pt_device_free", "pt_device_read", "pt_device_write", "pt_ctx_get_tuning", "pt_ctx_set_tuning",
               "pt_scene_snapshot_previous", "pt_film_enable_motion", "pt_film_read_motion", "pt_motion_params_default", "pt_film_motion",
               "pt_film_reproject_motion", "pt_denoise_history_params_default", "pt_film_denoise_history",
               "pt_upsample_params_default", "pt_film_upsample", "pt_film_read_upsampled",
               "pt_film_enable_counts", "pt_film_read_counts", "pt_adaptive_params_default", "pt_render_adaptive",
               "pt_guided_params_default", "pt_render_guided",
               "pt_trace_desc_default", "pt_trace_device", "pt_trace_workspace_bytes",
               "pt_radiance_desc_default", "pt_radiance_device", "pt_radiance_workspace_bytes",
               "pt_nearest_desc_default", "pt_nearest_device",
               "pt_crossings_desc_default", "pt_crossings_device"]
HOST_SYMBOLS = ["pth_load_obj", "pth_load_obj_ex", "pth_free_scene", "pth_write_ppm_bgra8", "pth_write_pfm", "pth_write_soup_obj", "pth_make_soup",
                "pth_make_stadium", "pth_self_leaf_rule", "pth_self_leaf_c1", "pth_self_leaf_skip"]

_amd = None
_host = None


def build(verbose=False):
    """Compile the HIP library for gfx950 and the host library/driver, in-tree."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], stdout=out)
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "host")], stdout=out)


def lib_amd():
    global _amd
    if _amd is None:
        # PT_LIB_AMD: a development build of the same library (scripts/: timeline instrumentation, an older revision for an A/B)
        path = os.environ.get("PT_LIB_AMD") or os.path.join(_HERE, "libpt_amd.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                              "there is no CPU fallback")
        L = C.CDLL(path)
        vp = C.c_void_p
        L.pt_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        L.pt_ctx_destroy.argtypes = [vp]
        L.pt_ctx_destroy.restype = None
        L.pt_last_error.argtypes = [vp]
        L.pt_last_error.restype = C.c_char_p
        L.pt_sync.argtypes = [vp]
        L.pt_ctx_get_tuning.argtypes = [vp, C.POINTER(Tuning)]
        L.pt_ctx_set_tuning.argtypes = [vp, C.POINTER(Tuning)]
        L.pt_scene_create.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(vp)]
        L.pt_scene_destroy.argtypes = [vp]
        L.pt_scene_destroy.restype = None
        L.pt_scene_set_instances.argtypes = [vp, vp, C.c_uint32]
        L.pt_scene_set_bvh_quality.argtypes = [vp, C.c_uint32]
        L.pt_scene_update.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32]
        L.pt_scene_create_device.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(vp)]
        L.pt_scene_update_device.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32]
        L.pt_scene_set_instances_device.argtypes = [vp, vp, C.c_uint32]
        if hasattr(L, "pt_scene_set_faces"):   # (materials without a rebuild; dev A/B runs load older builds through PT_LIB_AMD)
            L.pt_scene_set_faces.argtypes = [vp, vp, C.c_uint32]
            L.pt_scene_set_faces_device.argtypes = [vp, vp, C.c_uint32]
            L.pt_scene_read_faces.argtypes = [vp, vp]
        L.pt_scene_get_info.argtypes = [vp, C.POINTER(SceneInfo)]
        L.pt_scene_read_bvh.argtypes = [vp, vp, vp, vp]
        L.pt_scene_read_bvh4.argtypes = [vp, vp]
        L.pt_scene_read_bvh8.argtypes = [vp, vp, vp]
        L.pt_film_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.pt_film_create_external.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.POINTER(vp)]
        L.pt_film_clear.argtypes = [vp]
        L.pt_film_read_f32.argtypes = [vp, vp]
        L.pt_film_read_bgra8.argtypes = [vp, vp]
        L.pt_film_destroy.argtypes = [vp]
        L.pt_film_destroy.restype = None
        L.pt_params_default.argtypes = [C.POINTER(Params)]
        L.pt_params_default.restype = None
        L.pt_render.argtypes = [vp, vp, C.POINTER(Params)]
        L.pt_render_prepare.argtypes = [vp, vp, C.POINTER(Params)]
        if hasattr(L, "pt_render_aov"):   # (guide buffers; dev A/B runs load older builds through PT_LIB_AMD)
            L.pt_film_enable_aov.argtypes = [vp, C.POINTER(vp)]
            L.pt_render_aov.argtypes = [vp, vp, C.POINTER(Params)]
            L.pt_film_read_aov.argtypes = [vp, C.c_uint32, vp]
        if hasattr(L, "pt_film_denoise"):   # (the denoiser; dev A/B runs load older builds through PT_LIB_AMD)
            L.pt_denoise_params_default.argtypes = [C.POINTER(DenoiseParams)]
            L.pt_denoise_params_default.restype = None
            L.pt_film_denoise.argtypes = [vp, C.POINTER(DenoiseParams), vp, C.POINTER(C.c_float)]
            L.pt_film_read_denoised.argtypes = [vp, vp, vp]
        if hasattr(L, "pt_film_denoise_variance"):   # (the second-moment plane and its filter; as above)
            L.pt_film_enable_moments.argtypes = [vp, vp]
            L.pt_film_read_moments.argtypes = [vp, vp, C.POINTER(C.c_uint32)]
            L.pt_denoise_variance_params_default.argtypes = [C.POINTER(DenoiseVarianceParams)]
            L.pt_denoise_variance_params_default.restype = None
            L.pt_film_denoise_variance.argtypes = [vp, C.POINTER(DenoiseVarianceParams), vp, C.POINTER(C.c_float)]
        if hasattr(L, "pt_film_reproject"):   # (temporal accumulation; as above)
            L.pt_film_enable_history.argtypes = [vp, vp]
            L.pt_film_read_history.argtypes = [vp, vp]
            L.pt_reproject_params_default.argtypes = [C.POINTER(ReprojectParams)]
            L.pt_reproject_params_default.restype = None
            L.pt_film_reproject.argtypes = [vp, vp, C.POINTER(ReprojectParams), C.POINTER(C.c_float)]
        if hasattr(L, "pt_film_motion"):   # (motion for moved geometry; as above)
            L.pt_scene_snapshot_previous.argtypes = [vp]
            L.pt_film_enable_motion.argtypes = [vp, vp]
            L.pt_film_read_motion.argtypes = [vp, vp]
            L.pt_motion_params_default.argtypes = [C.POINTER(MotionParams)]
            L.pt_motion_params_default.restype = None
            L.pt_film_motion.argtypes = [vp, vp, C.POINTER(MotionParams), C.POINTER(C.c_float)]
            L.pt_film_reproject_motion.argtypes = [vp, vp, C.POINTER(ReprojectParams), C.POINTER(C.c_float)]
        if hasattr(L, "pt_film_denoise_history"):   # (per-pixel variance for reprojected films; as above)
            L.pt_denoise_history_params_default.argtypes = [C.POINTER(DenoiseHistoryParams)]
            L.pt_denoise_history_params_default.restype = None
            L.pt_film_denoise_history.argtypes = [vp, C.POINTER(DenoiseHistoryParams), vp, C.POINTER(C.c_float)]
        if hasattr(L, "pt_film_upsample"):   # (guide-driven upsampling; as above)
            L.pt_upsample_params_default.argtypes = [C.POINTER(UpsampleParams)]
            L.pt_upsample_params_default.restype = None
            L.pt_film_upsample.argtypes = [vp, vp, C.POINTER(UpsampleParams), vp, C.POINTER(C.c_float)]
            L.pt_film_read_upsampled.argtypes = [vp, vp, vp]
        if hasattr(L, "pt_render_adaptive"):   # (adaptive sampling; as above)
            L.pt_film_enable_counts.argtypes = [vp, vp]
            L.pt_film_read_counts.argtypes = [vp, vp]
            L.pt_adaptive_params_default.argtypes = [C.POINTER(AdaptiveParams)]
            L.pt_adaptive_params_default.restype = None
            L.pt_render_adaptive.argtypes = [vp, vp, C.POINTER(Params), C.POINTER(AdaptiveParams), C.POINTER(AdaptiveResult)]
        if hasattr(L, "pt_render_guided"):   # (film and guides in one pass; as above)
            L.pt_guided_params_default.argtypes = [C.POINTER(GuidedParams)]
            L.pt_guided_params_default.restype = None
            L.pt_render_guided.argtypes = [vp, vp, C.POINTER(Params), C.POINTER(GuidedParams), C.POINTER(GuidedResult)]
        L.pt_trace.argtypes = [vp, vp, C.c_uint32, C.c_float, C.c_float, C.c_uint32, vp]
        if hasattr(L, "pt_trace_device"):   # (ray queries on device buffers; dev A/B runs load older builds through PT_LIB_AMD)
            L.pt_trace_desc_default.argtypes = [C.POINTER(TraceDesc)]
            L.pt_trace_desc_default.restype = None
            L.pt_trace_device.argtypes = [vp, C.POINTER(TraceDesc), C.c_uint64, C.POINTER(C.c_float)]
            L.pt_trace_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
        if hasattr(L, "pt_radiance_device"):   # (radiance for caller-supplied rays; as above)
            L.pt_radiance_desc_default.argtypes = [C.POINTER(RadianceDesc)]
            L.pt_radiance_desc_default.restype = None
            L.pt_radiance_device.argtypes = [vp, C.POINTER(RadianceDesc), C.c_uint64, C.POINTER(C.c_float)]
            L.pt_radiance_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
        if hasattr(L, "pt_nearest_device"):   # (closest point on the mesh; as above)
            L.pt_nearest_desc_default.argtypes = [C.POINTER(NearestDesc)]
            L.pt_nearest_desc_default.restype = None
            L.pt_nearest_device.argtypes = [vp, C.POINTER(NearestDesc), C.c_uint64, C.POINTER(C.c_float)]
        if hasattr(L, "pt_crossings_device"):   # (crossing counts and winding; as above)
            L.pt_crossings_desc_default.argtypes = [C.POINTER(CrossingsDesc)]
            L.pt_crossings_desc_default.restype = None
            L.pt_crossings_device.argtypes = [vp, C.POINTER(CrossingsDesc), C.c_uint64, C.POINTER(C.c_float)]
        L.pt_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.pt_reset_stats.argtypes = [vp]
        if hasattr(L, "pt_get_block_counts"):   # (API version 6; dev A/B runs load older builds through PT_LIB_AMD)
            L.pt_get_block_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.c_uint32]
        L.pt_comm_unique_id.argtypes = [vp]
        L.pt_comm_create.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.pt_comm_ranks.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.pt_comm_destroy.argtypes = [vp]
        L.pt_comm_destroy.restype = None
        L.pt_film_present.argtypes = [vp, vp, C.c_uint32, vp]
        L.pt_device_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.pt_device_free.argtypes = [vp, vp]
        L.pt_device_read.argtypes = [vp, vp, vp, C.c_size_t]
        L.pt_device_write.argtypes = [vp, vp, vp, C.c_size_t]
        L.pt_film_tile_count.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        L.pt_film_pack_tiles.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
        L.pt_film_unpack_tiles.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp]
        if hasattr(L, "pt_film_present_planes"):   # (the gather of film planes; dev A/B runs load older builds through PT_LIB_AMD)
            L.pt_film_planes_words.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint32)]
            L.pt_film_pack_planes.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
            L.pt_film_unpack_planes.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
            L.pt_film_present_planes.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_float)]
        _amd = L
    return _amd


def lib_host():
    global _host
    if _host is None:
        path = os.path.join(_HERE, "libpt_host.so")
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: run __graft_entry__.build()")
        L = C.CDLL(path)
        L.pth_load_obj.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(HostScene), C.c_char_p, C.c_size_t]
        L.pth_load_obj_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(HostScene), C.c_char_p, C.c_size_t]
        L.pth_free_scene.argtypes = [C.POINTER(HostScene)]
        L.pth_free_scene.restype = None
        L.pth_write_ppm_bgra8.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.pth_write_pfm.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.pth_write_soup_obj.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32]
        L.pth_make_soup.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(HostScene)]
        L.pth_make_stadium.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(HostScene)]
        L.pth_self_leaf_rule.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
        L.pth_self_leaf_rule.restype = None
        L.pth_self_leaf_c1.argtypes = [C.c_float]
        L.pth_self_leaf_c1.restype = C.c_float
        L.pth_self_leaf_skip.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_float, C.c_void_p]
        L.pth_self_leaf_skip.restype = None
        _host = L
    return _host


# ---- host side: scene ingest / image output ---------------------------------------------------
def self_leaf_rule(e0, e1, own, other=None, scene_e=1.0):
    """csrc/self_leaf.h leaf_rule for triangle (e0, own, e1) of a leaf whose second triangle is (e0, e1, other), or a single triangle
    -> (thr f32, bits of g u32); thr = inf: a ray from this triangle never leaves its leaf out"""
    a = [np.ascontiguousarray(x, np.float32) for x in (e0, e1, own)]
    o = None if other is None else np.ascontiguousarray(other, np.float32)
    thr, g = C.c_float(), C.c_uint32()
    lib_host().pth_self_leaf_rule(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, None if o is None else o.ctypes.data, scene_e, C.byref(thr), C.byref(g))
    return np.float32(thr.value), int(g.value)


def self_leaf_c1(tmin):
    """csrc/self_leaf.h launch_c1: the launch's factor of the self-leaf rule"""
    return np.float32(lib_host().pth_self_leaf_c1(tmin))


def self_leaf_skip(dt, thr, g_word, c1):
    """csrc/self_leaf.h skip_code per element of dt -> u32 array: g_word's low 14 bits (the leaf's code) where the ray leaves its leaf out, else 0"""
    dt = np.ascontiguousarray(dt, np.float32)
    out = np.zeros(dt.size, np.uint32)
    lib_host().pth_self_leaf_skip(dt.ctypes.data, dt.size, thr, g_word, c1, out.ctypes.data)
    return out


QUAD_SHORTER_DIAGONAL = 1
SMALL_CHUNKS = 2  # test hook of the loader (include/pt_host.h)


def load_obj(path, mtl_dir=None, flags=0):
    """-> (vertices f32[3*nv], indices u32[3*nt], faces f32[6*nt]) as the reference's loadFromFile fills them
    (main.cpp:28-58); flags: QUAD_SHORTER_DIAGONAL (include/pt_host.h)."""
    hs = HostScene()
    err = C.create_string_buffer(512)
    rc = lib_host().pth_load_obj_ex(os.fsencode(path), os.fsencode(mtl_dir) if mtl_dir else None, flags, C.byref(hs), err, 512)
    if rc != 0:
        raise RuntimeError(f"load_obj({path}): {err.value.decode()}")  # reference: throw std::runtime_error (main.cpp:35)
    try:
        v = np.ctypeslib.as_array(hs.vertices, shape=(3 * hs.n_verts,)).copy()
        i = np.ctypeslib.as_array(hs.indices, shape=(3 * hs.n_tris,)).copy()
        f = np.ctypeslib.as_array(hs.faces, shape=(6 * hs.n_tris,)).copy()
    finally:
        lib_host().pth_free_scene(C.byref(hs))
    return v, i, f


def write_ppm(path, bgra):
    h, w = bgra.shape[:2]
    a = np.ascontiguousarray(bgra, dtype=np.uint8)
    if lib_host().pth_write_ppm_bgra8(os.fsencode(path), a.ctypes.data, w, h) != 0:
        raise RuntimeError(f"cannot write {path}")


def write_pfm(path, rgb):
    h, w = rgb.shape[:2]
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    if lib_host().pth_write_pfm(os.fsencode(path), a.ctypes.data, w, h) != 0:
        raise RuntimeError(f"cannot write {path}")


def write_soup_obj(path, n_tris, seed=1):
    if lib_host().pth_write_soup_obj(os.fsencode(path), n_tris, seed) != 0:
        raise RuntimeError(f"cannot write {path}")


def make_soup(n_tris, seed=1):
    """-> the arrays load_obj(write_soup_obj(...)) would return, without the OBJ text in between."""
    hs = HostScene()
    if lib_host().pth_make_soup(n_tris, seed, C.byref(hs)) != 0:
        raise RuntimeError("pth_make_soup failed")
    try:
        v = np.ctypeslib.as_array(hs.vertices, shape=(3 * hs.n_verts,)).copy()
        i = np.ctypeslib.as_array(hs.indices, shape=(3 * hs.n_tris,)).copy()
        f = np.ctypeslib.as_array(hs.faces, shape=(6 * hs.n_tris,)).copy()
    finally:
        lib_host().pth_free_scene(C.byref(hs))
    return v, i, f


def make_stadium(floor_side=384, sphere_seg=160):
    """The "teapot in a stadium" stress scene (include/pt_host.h pth_make_stadium): -> (vertices, indices, faces)."""
    hs = HostScene()
    if lib_host().pth_make_stadium(floor_side, sphere_seg, C.byref(hs)) != 0:
        raise RuntimeError("pth_make_stadium failed")
    try:
        v = np.ctypeslib.as_array(hs.vertices, shape=(3 * hs.n_verts,)).copy()
        i = np.ctypeslib.as_array(hs.indices, shape=(3 * hs.n_tris,)).copy()
        f = np.ctypeslib.as_array(hs.faces, shape=(6 * hs.n_tris,)).copy()
    finally:
        lib_host().pth_free_scene(C.byref(hs))
    return v, i, f


def cornell_grid_instances(n=100, cell=0.02, scale=0.009):
    """BASELINE config C4 (frozen recipe): n x n instances of the scene in the
    z = 0 plane filling x in [-1,1], y in [-2,0]: uniform scale `scale`, translation
    (-1 + (i+1/2) cell, -2 + (j+1/2) cell + scale, 0); row-major 3x4, instance id = j*n + i."""
    m = np.zeros((n * n, 3, 4), dtype=np.float32)
    i = np.arange(n, dtype=np.float32)
    tx = (np.float32(-1.0) + (i + np.float32(0.5)) * np.float32(cell)).astype(np.float32)
    ty = (np.float32(-2.0) + (i + np.float32(0.5)) * np.float32(cell) + np.float32(scale)).astype(np.float32)
    m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = np.float32(scale)
    m[:, 0, 3] = np.tile(tx, n)
    m[:, 1, 3] = np.repeat(ty, n)
    return m


# ---- device side --------------------------------------------------------------------------------
def default_params(**kw):
    p = Params()
    lib_amd().pt_params_default(C.byref(p))
    for k, v in kw.items():
        if k in ("cam_origin", "cam_target", "env"):
            setattr(p, k, (C.c_float * 3)(*v))
        else:
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
    return p


def _default_params(struct, fn):
    """-> a `struct` as the library's `fn` (a pt_*_params_default) fills it"""
    p = struct()
    getattr(lib_amd(), fn)(C.byref(p))
    return p


def denoise_default_params():
    return _default_params(DenoiseParams, "pt_denoise_params_default")


def denoise_variance_default_params():
    return _default_params(DenoiseVarianceParams, "pt_denoise_variance_params_default")


def denoise_history_default_params():
    return _default_params(DenoiseHistoryParams, "pt_denoise_history_params_default")


def upsample_default_params():
    return _default_params(UpsampleParams, "pt_upsample_params_default")


def adaptive_default_params():
    return _default_params(AdaptiveParams, "pt_adaptive_params_default")


def guided_default_params():
    return _default_params(GuidedParams, "pt_guided_params_default")


def reproject_default_params():
    return _default_params(ReprojectParams, "pt_reproject_params_default")


def trace_default_desc():
    return _default_params(TraceDesc, "pt_trace_desc_default")


def radiance_default_desc():
    return _default_params(RadianceDesc, "pt_radiance_desc_default")


def nearest_default_desc():
    return _default_params(NearestDesc, "pt_nearest_desc_default")


def crossings_default_desc():
    return _default_params(CrossingsDesc, "pt_crossings_desc_default")


def motion_default_params():
    return _default_params(MotionParams, "pt_motion_params_default")


class Context:
    """One GPU + one stream (reference: Context, main.cpp:74-267)."""

    def __init__(self, device=0, stream=None):
        self.h = C.c_void_p()
        rc = lib_amd().pt_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self.h))
        if rc != PT_OK:
            raise PtError(rc, lib_amd().pt_last_error(None).decode())

    def _check(self, rc):
        if rc != PT_OK:
            raise PtError(rc, lib_amd().pt_last_error(self.h).decode())

    def sync(self):
        self._check(lib_amd().pt_sync(self.h))

    def tuning(self):
        t = Tuning()
        self._check(lib_amd().pt_ctx_get_tuning(self.h, C.byref(t)))
        return t

    def set_tuning(self, **kw):
        """Change speed knobs (names: TUNING_NAMES; -1 = built-in choice) -> the previous values of the ones changed, so a
        caller can put them back: ctx.set_tuning(**ctx.set_tuning(node_yield=0))."""
        t = self.tuning()
        old = {}
        for k, v in kw.items():
            if k not in TUNING_NAMES:
                raise AttributeError(k)
            old[k] = getattr(t, k)
            setattr(t, k, int(v))
        self._check(lib_amd().pt_ctx_set_tuning(self.h, C.byref(t)))
        return old

    def stats(self):
        s = Stats()
        self._check(lib_amd().pt_get_stats(self.h, C.byref(s)))
        return s

    def reset_stats(self):
        self._check(lib_amd().pt_reset_stats(self.h))

    def trace_workspace_bytes(self):
        """Device bytes the context holds for Scene.trace_device / trace_tensors (pt_trace_workspace_bytes): 0 before the first call."""
        n = C.c_uint64(0)
        self._check(lib_amd().pt_trace_workspace_bytes(self.h, C.byref(n)))
        return n.value

    def radiance_workspace_bytes(self):
        """Device bytes the context holds for Scene.radiance_device / radiance_tensors (pt_radiance_workspace_bytes): 0 before the first call."""
        n = C.c_uint64(0)
        self._check(lib_amd().pt_radiance_workspace_bytes(self.h, C.byref(n)))
        return n.value

    def block_counts(self):
        """{block: (wave executions, lanes inside)} of the instrumented fused kernel since reset_stats (pt_get_block_counts; render with
        pipeline=PIPELINE_FUSED, flags=FLAG_COUNT_VISITS)."""
        a = (C.c_uint64 * (2 * len(FUSED_BLOCKS)))()
        self._check(lib_amd().pt_get_block_counts(self.h, a, len(FUSED_BLOCKS)))
        return {n: (int(a[2 * i]), int(a[2 * i + 1])) for i, n in enumerate(FUSED_BLOCKS)}

    def close(self):
        if self.h:
            lib_amd().pt_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene:
    """Vertex/index/face buffers + the device-built LBVH (reference: main.cpp:492-538)."""

    def __init__(self, ctx, vertices, indices, faces):
        self.ctx = ctx
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1)
        i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        f = np.ascontiguousarray(faces, dtype=np.float32).reshape(-1)
        if v.size % 3 or i.size % 3 or f.size != 2 * i.size:
            raise ValueError("vertices must be 3*nv, indices 3*nt, faces 6*nt")
        self.h = C.c_void_p()
        ctx._check(lib_amd().pt_scene_create(ctx.h, v.ctypes.data, v.size // 3, i.ctypes.data, i.size // 3,
                                             f.ctypes.data, C.byref(self.h)))

    @classmethod
    def from_obj(cls, ctx, path=ASSET_CORNELL):
        return cls(ctx, *load_obj(path))

    def set_instances(self, xforms3x4):
        """n object->world 3x4 matrices (VkTransformMatrixKHR layout); empty = the reference's
        single identity instance (main.cpp:515-538)."""
        x = np.ascontiguousarray(xforms3x4, dtype=np.float32).reshape(-1, 12)
        self.ctx._check(lib_amd().pt_scene_set_instances(self.h, x.ctypes.data if len(x) else None, len(x)))

    def set_bvh_quality(self, quality):
        """BVH_PREFER_FAST_TRACE (default; main.cpp:419) or BVH_PREFER_FAST_BUILD (always the collapsed LBVH)."""
        self.ctx._check(lib_amd().pt_scene_set_bvh_quality(self.h, quality))

    def update(self, vertices, indices, mode=SCENE_UPDATE_REFIT):
        """New positions for the scene's triangles (pt_scene_update): same triangle count, materials kept.  SCENE_UPDATE_REFIT
        keeps the trees' topology and refits them; SCENE_UPDATE_REBUILD builds them again.  Images and hits equal a fresh scene's."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1)
        i = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        if v.size % 3 or i.size % 3:
            raise ValueError("vertices must be 3*nv, indices 3*nt")
        self.ctx._check(lib_amd().pt_scene_update(self.h, v.ctypes.data, v.size // 3, i.ctypes.data, i.size // 3, mode))

    @staticmethod
    def _geometry_tensors(vertices, indices, faces=None):
        """The tensor rules of from_tensors / update_tensors -> contiguous (vertices, indices[, faces]); ValueError before a device is touched."""
        import torch
        index_types = (torch.int32, getattr(torch, "uint32", torch.int32))   # (int32 reinterpreted as u32: a negative index is out of range)
        for name, t, kinds, per in (("vertices", vertices, (torch.float32,), 3), ("indices", indices, index_types, 3), ("faces", faces, (torch.float32,), 6)):
            if t is None and name == "faces":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype not in kinds:
                raise ValueError(f"{name} must be a {'int32 / uint32' if name == 'indices' else 'float32'} CUDA tensor")
            if t.numel() % per or (name == "faces" and t.numel() != 2 * indices.numel()):
                raise ValueError("vertices must be 3*nv, indices 3*nt, faces 6*nt")
        for name, t in (("vertices", vertices), ("indices", indices), ("faces", faces)):
            if t is not None and not t.is_cuda:
                raise ValueError(f"{name} must be a CUDA tensor")
            if t is not None and t.device != vertices.device:
                raise ValueError("vertices, indices and faces must be on one device")
        out = [vertices.contiguous(), indices.contiguous()] + ([faces.contiguous()] if faces is not None else [])
        return out

    @classmethod
    def from_tensors(cls, ctx, vertices, indices, faces):
        """A scene from torch tensors on the GPU, nothing through the host (pt_scene_create_device): vertices and faces float32 CUDA tensors of
        3*nv and 6*nt elements, indices an int32 (or uint32) tensor of 3*nt; made contiguous if they are not.  Equal to Scene(ctx, ...) of
        their host copies, bit for bit."""
        import torch
        v, i, f = cls._geometry_tensors(vertices, indices, faces)
        self = cls.__new__(cls)
        self.ctx = ctx
        self.h = C.c_void_p()
        torch.cuda.current_stream(v.device).synchronize()   # (Scene.trace_tensors has the reasons)
        ctx._check(lib_amd().pt_scene_create_device(ctx.h, v.data_ptr(), v.numel() // 3, i.data_ptr(), i.numel() // 3, f.data_ptr(), C.byref(self.h)))
        return self

    def update_device(self, n_verts, vertices_ptr, n_tris, indices_ptr, mode=SCENE_UPDATE_REFIT):
        """pt_scene_update_device over raw DEVICE pointers: f32 [3 * n_verts] and u32 [3 * n_tris], dense (include/pt_api.h).  Blocking."""
        self.ctx._check(lib_amd().pt_scene_update_device(self.h, vertices_ptr, n_verts, indices_ptr, n_tris, mode))

    def update_tensors(self, vertices, indices, mode=SCENE_UPDATE_REFIT):
        """Scene.update for torch tensors on the GPU, nothing through the host: a float32 CUDA tensor of 3*nv elements and an int32 (or uint32)
        tensor of 3*nt on the same device, made contiguous if they are not.  The result equals update() of their host copies."""
        import torch
        v, i = self._geometry_tensors(vertices, indices)
        # The tensors were written on torch's current stream and the update reads them on the context's: torch's stream is drained first.  The
        # call is blocking, which orders the read before whatever torch queues next (Scene.trace_tensors).
        torch.cuda.current_stream(v.device).synchronize()
        self.update_device(v.numel() // 3, v.data_ptr(), i.numel() // 3, i.data_ptr(), mode=mode)

    def set_instances_device(self, xforms_ptr, n):
        """pt_scene_set_instances_device over a raw DEVICE pointer: n object->world 3x4 row-major f32 matrices, dense (include/pt_api.h).
        n = 0 restores the single-level scene (the pointer may then be None).  Blocking."""
        self.ctx._check(lib_amd().pt_scene_set_instances_device(self.h, xforms_ptr if n else None, n))

    @staticmethod
    def _instance_tensor(xforms):
        """The tensor rule of set_instances_tensor -> the contiguous tensor; ValueError before a device is touched."""
        import torch
        if not isinstance(xforms, torch.Tensor) or xforms.dtype != torch.float32:
            raise ValueError("xforms must be a float32 CUDA tensor")
        if xforms.numel() % 12:
            raise ValueError("xforms must hold 12*n elements (n 3x4 matrices)")
        if not xforms.is_cuda:
            raise ValueError("xforms must be a CUDA tensor")
        return xforms.contiguous()

    def set_instances_tensor(self, xforms):
        """Scene.set_instances for a torch tensor on the GPU, nothing through the host: a float32 CUDA tensor of 12*n elements (n 3x4
        matrices), made contiguous if it is not; an empty tensor restores the single-level scene.  The result equals set_instances() of
        its host copy, bit for bit."""
        import torch
        x = self._instance_tensor(xforms)
        torch.cuda.current_stream(x.device).synchronize()   # (update_tensors has the reasons)
        n = x.numel() // 12
        self.set_instances_device(x.data_ptr() if n else None, n)

    def set_faces(self, faces):
        """New per-face materials (Kd.rgb, Ke.rgb: 6 floats per triangle) for the scene's triangles, without a rebuild (pt_scene_set_faces):
        afterwards the scene is what Scene(ctx, vertices, indices, faces) followed by the same later calls would be, bit for bit."""
        f = np.ascontiguousarray(faces, dtype=np.float32).reshape(-1)
        if f.size % 6:
            raise ValueError("faces must be 6*nt")
        self.ctx._check(lib_amd().pt_scene_set_faces(self.h, f.ctypes.data, f.size // 6))

    def set_faces_device(self, faces_ptr, n_tris):
        """pt_scene_set_faces_device over a raw DEVICE pointer: f32 [6 * n_tris], dense (include/pt_api.h).  Blocking."""
        self.ctx._check(lib_amd().pt_scene_set_faces_device(self.h, faces_ptr, n_tris))

    def _n_tris(self):
        """the scene's triangle count (it never changes): asked once, from the scene's record -- no device call"""
        if getattr(self, "_nt", None) is None:
            self._nt = int(self.info().n_tris)
        return self._nt

    def _faces_tensor(self, faces):
        """The tensor rule of set_faces_tensor, in _geometry_tensors' order (type, sizes, device) -> the tensor; ValueError before a device is
        touched.  Unlike the geometry wrappers it copies nothing: a tensor that is not contiguous is refused."""
        import torch
        if not isinstance(faces, torch.Tensor) or faces.dtype != torch.float32:
            raise ValueError("faces must be a float32 CUDA tensor")
        if not faces.is_contiguous():
            raise ValueError("faces must be contiguous")
        if faces.numel() != 6 * self._n_tris():
            raise ValueError("faces must hold 6*nt elements, nt the scene's triangle count")
        if not faces.is_cuda:
            raise ValueError("faces must be a CUDA tensor")
        return faces

    def set_faces_tensor(self, faces):
        """Scene.set_faces for a torch tensor on the GPU, nothing through the host: a contiguous float32 CUDA tensor of 6*nt elements, nt the
        scene's triangle count.  The result equals set_faces() of its host copy, bit for bit."""
        import torch
        f = self._faces_tensor(faces)
        torch.cuda.current_stream(f.device).synchronize()   # (update_tensors has the reasons)
        self.set_faces_device(f.data_ptr(), f.numel() // 6)

    def read_faces(self):
        """-> the scene's kept copy of the materials, float32 [6 * n_tris] (pt_scene_read_faces)"""
        f = np.zeros(6 * self.info().n_tris, dtype=np.float32)
        self.ctx._check(lib_amd().pt_scene_read_faces(self.h, f.ctypes.data))
        return f

    def snapshot_previous(self):
        """Remembers the scene as it stands now -- vertex positions and instance matrices -- as "the previous geometry" of Film.motion
        (pt_scene_snapshot_previous).  Call it before the update / set_instances of a time step; a second call replaces the first."""
        self.ctx._check(lib_amd().pt_scene_snapshot_previous(self.h))

    def info(self):
        i = SceneInfo()
        self.ctx._check(lib_amd().pt_scene_get_info(self.h, C.byref(i)))
        return i

    def read_bvh(self):
        i = self.info()
        keys = np.zeros(i.n_tris, dtype=np.uint64)
        prim = np.zeros(i.n_tris, dtype=np.uint32)
        nodes = np.zeros((i.n_nodes, 16), dtype=np.uint32)
        self.ctx._check(lib_amd().pt_scene_read_bvh(self.h, keys.ctypes.data, prim.ctypes.data, nodes.ctypes.data))
        return keys, prim, nodes

    def read_bvh4(self):
        nodes = np.zeros((self.info().n_wide_nodes, 32), dtype=np.uint32)
        self.ctx._check(lib_amd().pt_scene_read_bvh4(self.h, nodes.ctypes.data))
        return nodes

    def read_bvh8(self):
        """-> (nodes [n_wide8, 16] u32, prim_of_pos8 [n_tris] u32) of the 8-wide tree (include/pt_api.h: pt_scene_read_bvh8)"""
        self.ctx._check(lib_amd().pt_scene_read_bvh8(self.h, None, None))      # big scenes build their 8-wide nodes on first request
        i = self.info()
        nodes = np.zeros((i.n_wide8_nodes, 16), dtype=np.uint32)
        prim = np.zeros(i.n_tris, dtype=np.uint32)
        self.ctx._check(lib_amd().pt_scene_read_bvh8(self.h, nodes.ctypes.data, prim.ctypes.data))
        return nodes, prim

    def trace(self, rays6, tmin=0.001, tmax=10000.0, extend=EXTEND_AUTO):
        """Closest-hit query alone (traceRayEXT, raygen.rgen:63-75)."""
        r = np.ascontiguousarray(rays6, dtype=np.float32).reshape(-1, 6)
        hits = np.zeros(r.shape[0], dtype=HIT_DTYPE)
        self.ctx._check(lib_amd().pt_trace(self.h, r.ctypes.data, r.shape[0], tmin, tmax, extend, hits.ctypes.data))
        return hits

    def trace_device(self, n, rays_ptr, tmax_ptr=None, hits_ptr=None, occluded_ptr=None, position_ptr=None, normal_ptr=None, albedo_ptr=None,
                     emission_ptr=None, mode=TRACE_CLOSEST, tmin=0.001, tmax=10000.0, extend=EXTEND_AUTO, flags=0, chunk_rays=0):
        """pt_trace_device over raw DEVICE pointers (include/pt_api.h has the layouts): n rays at rays_ptr, the outputs the mode allows.
        -> device_ms (0 under TRACE_ASYNC: the call only queues, Context.sync() waits)."""
        d = trace_default_desc()
        d.d_rays6, d.d_tmax, d.d_hits, d.d_occluded = rays_ptr, tmax_ptr, hits_ptr, occluded_ptr
        d.d_position, d.d_normal, d.d_albedo, d.d_emission = position_ptr, normal_ptr, albedo_ptr, emission_ptr
        d.tmin, d.tmax, d.mode, d.extend, d.flags, d.chunk_rays = tmin, tmax, mode, extend, flags, chunk_rays
        ms = C.c_float(0.0)
        self.ctx._check(lib_amd().pt_trace_device(self.h, C.byref(d), n, C.byref(ms)))
        return ms.value

    def trace_tensors(self, rays, tmax_per_ray=None, mode=TRACE_CLOSEST, surface=False, tmin=0.001, tmax=10000.0, extend=EXTEND_AUTO, chunk_rays=0,
                      form="queues"):
        """Ray queries on torch tensors, nothing through the host.  rays: float32 CUDA tensor [n, 6] {origin, direction} (made contiguous if it
        is not).  TRACE_CLOSEST -> dict of tensors: prim (int32, -1 = miss), t, u, v (float32), inst (int32) -- views of one [n, 5] buffer in
        pt_hit's layout, no copy -- and, with surface, position / normal / albedo / emission [n, 3].  TRACE_ANY -> bool tensor [n], True = some
        triangle with tmin < t < bound; the bound is tmax_per_ray[i] (float32 CUDA tensor [n]) or tmax.
        form: "queues" (pack, extend, unpack), "fused" (PT_TRACE_FUSED: the single kernel, an error where it does not apply) or "auto"
        (PT_TRACE_AUTO); the result does not depend on it."""
        import torch
        forms = {"queues": 0, "fused": TRACE_FUSED, "auto": TRACE_AUTO}
        if form not in forms:
            raise ValueError('form must be "queues", "fused" or "auto"')
        if rays.dtype != torch.float32 or not rays.is_cuda or rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError("rays must be a float32 CUDA tensor of shape [n, 6]")
        rays = rays.contiguous()
        n, dev = rays.shape[0], rays.device
        bound = None
        if tmax_per_ray is not None:
            if tmax_per_ray.dtype != torch.float32 or tmax_per_ray.device != dev or tmax_per_ray.numel() != n:
                raise ValueError("tmax_per_ray must be a float32 tensor of n elements on the rays' device")
            bound = tmax_per_ray.contiguous()
        kw = dict(tmax_ptr=bound.data_ptr() if bound is not None else None, mode=mode, tmin=tmin, tmax=tmax, extend=extend, chunk_rays=chunk_rays,
                  flags=forms[form])
        # The rays (and the outputs' allocations) were produced on torch's current stream; the query runs on the context's.  So torch's stream is
        # drained first.  The call itself is blocking -- it returns after the context's stream has finished -- which orders the outputs before
        # whatever torch queues next.  (No TRACE_ASYNC here: torch would have no event to wait on.)
        if mode == TRACE_ANY:
            occ = torch.empty(n, dtype=torch.uint8, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            self.trace_device(n, rays.data_ptr(), occluded_ptr=occ.data_ptr(), **kw)
            return occ.view(torch.bool)
        hits = torch.empty((n, 5), dtype=torch.int32, device=dev)
        hits_f = hits.view(torch.float32)   # the same memory: pt_hit is {u32, f32, f32, f32, u32}
        out = {"prim": hits[:, 0], "t": hits_f[:, 1], "u": hits_f[:, 2], "v": hits_f[:, 3], "inst": hits[:, 4]}
        planes = {}
        if surface:
            for name in ("position", "normal", "albedo", "emission"):
                out[name] = torch.empty((n, 3), dtype=torch.float32, device=dev)
                planes[name + "_ptr"] = out[name].data_ptr()
        torch.cuda.current_stream(dev).synchronize()
        self.trace_device(n, rays.data_ptr(), hits_ptr=hits.data_ptr(), **planes, **kw)
        return out

    def nearest_device(self, n, points_ptr, max_dist_ptr=None, nearest_ptr=None, point_ptr=None, max_dist=float("inf"), form=NEAREST_AUTO):
        """pt_nearest_device over raw DEVICE pointers (include/pt_api.h has the layouts and the arithmetic): n points at points_ptr, their
        closest triangle {prim, dist2, u, v} to nearest_ptr and / or the closest point itself to point_ptr.  Blocking -> device_ms."""
        d = nearest_default_desc()
        d.d_points, d.d_max_dist, d.d_nearest, d.d_point = points_ptr, max_dist_ptr, nearest_ptr, point_ptr
        d.max_dist, d.form = max_dist, form
        ms = C.c_float(0.0)
        self.ctx._check(lib_amd().pt_nearest_device(self.h, C.byref(d), n, C.byref(ms)))
        return ms.value

    def nearest_tensors(self, points, max_dist=None, max_dist_per_query=None, point=False, form="auto"):
        """Closest point on the mesh for torch points, nothing through the host.  points: float32 CUDA tensor [n, 3] (made contiguous if it is
        not); max_dist: one search radius (None: unbounded) or max_dist_per_query: float32 CUDA tensor [n].  -> dict of tensors: prim (int32,
        -1 = nothing within the radius), dist2, u, v (float32) -- views of one [n, 4] buffer in pt_nearest's layout, no copy -- and, with
        point, point [n, 3].  form: "auto", "lds" (PT_NEAREST_LDS: an error where the scene does not fit) or "global"; the result does not
        depend on it."""
        forms = {"auto": NEAREST_AUTO, "lds": NEAREST_LDS, "global": NEAREST_GLOBAL}
        if form not in forms:
            raise ValueError('form must be "auto", "lds" or "global"')
        import torch
        if points.dtype != torch.float32 or not points.is_cuda or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must be a float32 CUDA tensor of shape [n, 3]")
        points = points.contiguous()
        n, dev = points.shape[0], points.device
        radii = None
        if max_dist_per_query is not None:
            if max_dist_per_query.dtype != torch.float32 or max_dist_per_query.device != dev or max_dist_per_query.numel() != n:
                raise ValueError("max_dist_per_query must be a float32 tensor of n elements on the points' device")
            radii = max_dist_per_query.contiguous()
        rec = torch.empty((n, 4), dtype=torch.int32, device=dev)
        rec_f = rec.view(torch.float32)   # the same memory: pt_nearest is {u32, f32, f32, f32}
        out = {"prim": rec[:, 0], "dist2": rec_f[:, 1], "u": rec_f[:, 2], "v": rec_f[:, 3]}
        if point:
            out["point"] = torch.empty((n, 3), dtype=torch.float32, device=dev)
        # the points were produced on torch's current stream, the query runs on the context's: torch's is drained first, and the call is blocking
        # (trace_tensors' rule)
        torch.cuda.current_stream(dev).synchronize()
        self.nearest_device(n, points.data_ptr(), max_dist_ptr=radii.data_ptr() if radii is not None else None, nearest_ptr=rec.data_ptr(),
                            point_ptr=out["point"].data_ptr() if point else None, max_dist=float("inf") if max_dist is None else max_dist,
                            form=forms[form])
        return out

    def crossings_device(self, n, rays_ptr=None, points_ptr=None, direction=None, tmax_ptr=None, count_ptr=None, winding_ptr=None, tmin=0.0,
                         tmax=float("inf"), form=CROSSINGS_AUTO):
        """pt_crossings_device over raw DEVICE pointers (include/pt_api.h has the layouts and the arithmetic): n rays at rays_ptr, or n origins at
        points_ptr sharing `direction`; how many triangles each crosses in (tmin, bound) to count_ptr and / or the signed sum to winding_ptr.
        Blocking -> device_ms."""
        d = crossings_default_desc()
        d.d_rays6, d.d_points, d.d_tmax, d.d_count, d.d_winding = rays_ptr, points_ptr, tmax_ptr, count_ptr, winding_ptr
        if direction is not None:
            d.direction = (C.c_float * 3)(*direction)
        d.tmin, d.tmax, d.form = tmin, tmax, form
        ms = C.c_float(0.0)
        self.ctx._check(lib_amd().pt_crossings_device(self.h, C.byref(d), n, C.byref(ms)))
        return ms.value

    def crossings_tensors(self, rays=None, points=None, direction=None, tmin=0.0, tmax=None, tmax_per_ray=None, winding=False, form="auto"):
        """How many triangles torch rays cross, nothing through the host.  rays: float32 CUDA tensor [n, 6] {origin, direction}, or points: float32
        CUDA tensor [n, 3] with one `direction` (three floats) for all of them -- exactly one of the two; made contiguous if they are not.  The
        range is tmin < t < tmax (None: unbounded) or tmax_per_ray (float32 CUDA tensor [n]).  -> count, an int32 tensor [n] (the library's u32
        words viewed as int32), or with winding=True (count, winding).  form: "auto", "lds" (PT_CROSSINGS_LDS: an error where the scene does not
        fit) or "global"; the result does not depend on it."""
        forms = {"auto": CROSSINGS_AUTO, "lds": CROSSINGS_LDS, "global": CROSSINGS_GLOBAL}
        if form not in forms:
            raise ValueError('form must be "auto", "lds" or "global"')
        if (rays is None) == (points is None):
            raise ValueError("exactly one of rays and points")
        import torch
        src, width = (rays, 6) if rays is not None else (points, 3)
        if src.dtype != torch.float32 or not src.is_cuda or src.dim() != 2 or src.shape[1] != width:
            raise ValueError(f"{'rays' if rays is not None else 'points'} must be a float32 CUDA tensor of shape [n, {width}]")
        if points is not None and (direction is None or len(direction) != 3):
            raise ValueError("points need a direction of three floats")
        src = src.contiguous()
        n, dev = src.shape[0], src.device
        bound = None
        if tmax_per_ray is not None:
            if tmax_per_ray.dtype != torch.float32 or tmax_per_ray.device != dev or tmax_per_ray.numel() != n:
                raise ValueError("tmax_per_ray must be a float32 tensor of n elements on the rays' device")
            bound = tmax_per_ray.contiguous()
        count = torch.empty(n, dtype=torch.int32, device=dev)
        wind = torch.empty(n, dtype=torch.int32, device=dev) if winding else None
        if n == 0:   # (an empty tensor's data_ptr() is NULL, which the library would read as "no output named")
            return (count, wind) if winding else count
        # the rays were produced on torch's current stream, the query runs on the context's: torch's is drained first, and the call is blocking
        # (trace_tensors' rule)
        torch.cuda.current_stream(dev).synchronize()
        self.crossings_device(n, rays_ptr=src.data_ptr() if rays is not None else None, points_ptr=src.data_ptr() if points is not None else None,
                              direction=[float(c) for c in direction] if points is not None else None,
                              tmax_ptr=bound.data_ptr() if bound is not None else None, count_ptr=count.data_ptr(),
                              winding_ptr=wind.data_ptr() if winding else None, tmin=tmin, tmax=float("inf") if tmax is None else tmax,
                              form=forms[form])
        return (count, wind) if winding else count

    def inside_tensors(self, points, votes=3):
        """Which points lie inside the mesh: a bool tensor [n], the majority over the first `votes` (odd, at most 5) of INSIDE_DIRECTIONS of
        "the ray from the point crosses an odd number of triangles" -- one crossings_tensors(points=..., direction=...) call per direction.
        Caveat: the count follows pt_trace's acceptance rule.  A ray through a shared edge counts both triangles, a ray through a vertex the
        whole fan, a duplicated face counts twice (the Cornell OBJ has two duplicated quads, and the box is open anyway).  Such rays are why
        there is a vote; and the answer means something for CLOSED meshes only."""
        if votes not in (1, 3, 5):
            raise ValueError("votes must be 1, 3 or 5")
        odd = None
        for d in INSIDE_DIRECTIONS[:votes]:
            c = self.crossings_tensors(points=points, direction=d) & 1
            odd = c if odd is None else odd + c
        return odd * 2 > votes

    def signed_distance_tensors(self, points, votes=3, max_dist=None):
        """Signed distance to a closed mesh: one nearest_tensors call and one inside_tensors call -> (sdf, prim, u, v): sdf = sqrt(dist2) outside,
        -sqrt(dist2) inside, NaN where no triangle lies within max_dist (prim = -1 there)."""
        import torch
        near = self.nearest_tensors(points, max_dist=max_dist)
        inside = self.inside_tensors(points, votes=votes)
        dist = torch.sqrt(near["dist2"])
        sdf = torch.where(inside, -dist, dist)
        sdf = torch.where(near["prim"] < 0, torch.full_like(sdf, float("nan")), sdf)
        return sdf, near["prim"], near["u"], near["v"]

    def radiance_device(self, n, rays_ptr, radiance_ptr, seeds_ptr=None, moment2_ptr=None, spp=32, max_depth=8, tmin=0.001, tmax=10000.0, env=None,
                        frame=0, index_base=0, flags=0, extend=EXTEND_AUTO, chunk_rays=0):
        """pt_radiance_device over raw DEVICE pointers (include/pt_api.h has the layouts and the arithmetic): n rays at rays_ptr, their mean
        radiance to radiance_ptr (and the mean of the samples' squares to moment2_ptr).  Blocking -> device_ms."""
        d = radiance_default_desc()
        d.d_rays6, d.d_seeds, d.d_radiance, d.d_moment2 = rays_ptr, seeds_ptr, radiance_ptr, moment2_ptr
        d.tmin, d.tmax, d.spp, d.max_depth, d.frame, d.index_base = tmin, tmax, spp, max_depth, frame, index_base
        d.flags, d.extend, d.chunk_rays = flags, extend, chunk_rays
        if env is not None:
            d.env = (C.c_float * 3)(*env)
        ms = C.c_float(0.0)
        self.ctx._check(lib_amd().pt_radiance_device(self.h, C.byref(d), n, C.byref(ms)))
        return ms.value

    def radiance_tensors(self, rays, spp=32, max_depth=8, seeds=None, nee=False, out=None, moment2=False, frame=0, accumulate=False, tmin=0.001,
                         tmax=10000.0, env=None, index_base=0, extend=EXTEND_AUTO, chunk_rays=0, form="wavefront"):
        """Path-traced radiance along torch rays, nothing through the host.  rays: float32 CUDA tensor [n, 6] {origin, direction} (made contiguous
        if it is not); seeds: optional int32 / uint32 tensor of n * spp RNG states; out: a contiguous float32 [n, 3] tensor to store into (or, with
        accumulate, to blend into by `frame`), made here when None; moment2: True for a new second-moment tensor, or a tensor like `out`.
        form: "wavefront" (the queues), "fused" (PT_RADIANCE_FUSED: the single kernel, an error where it does not apply) or "auto"
        (PT_RADIANCE_AUTO); the result does not depend on it.
        -> the [n, 3] radiance tensor, or (radiance, moment2)."""
        import torch
        forms = {"wavefront": 0, "fused": RADIANCE_FUSED, "auto": RADIANCE_AUTO}
        if form not in forms:
            raise ValueError('form must be "wavefront", "fused" or "auto"')
        if rays.dtype != torch.float32 or not rays.is_cuda or rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError("rays must be a float32 CUDA tensor of shape [n, 6]")
        rays = rays.contiguous()
        n, dev = rays.shape[0], rays.device

        def plane(t, what):
            if t is None or t is True:
                return torch.zeros((n, 3), dtype=torch.float32, device=dev) if accumulate and frame else torch.empty((n, 3), dtype=torch.float32, device=dev)
            if t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (n, 3) or not t.is_contiguous():
                raise ValueError(what + " must be a contiguous float32 tensor [n, 3] on the rays' device")
            return t
        out = plane(out, "out")
        m2 = plane(moment2, "moment2") if moment2 is not False and moment2 is not None else None
        if seeds is not None:
            if seeds.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or seeds.device != dev or seeds.numel() != n * spp:
                raise ValueError("seeds must be an int32 / uint32 tensor of n * spp elements on the rays' device")
            seeds = seeds.contiguous()
        flags = (RADIANCE_NEE if nee else 0) | (RADIANCE_ACCUMULATE if accumulate else 0) | forms[form]
        # (torch's stream is drained first and the call blocks: Scene.trace_tensors has the reasons)
        torch.cuda.current_stream(dev).synchronize()
        self.radiance_device(n, rays.data_ptr(), out.data_ptr(), seeds_ptr=seeds.data_ptr() if seeds is not None else None,
                             moment2_ptr=m2.data_ptr() if m2 is not None else None, spp=spp, max_depth=max_depth, tmin=tmin, tmax=tmax, env=env,
                             frame=frame, index_base=index_base, flags=flags, extend=extend, chunk_rays=chunk_rays)
        return (out, m2) if m2 is not None else out

    def close(self):
        if self.h:
            lib_amd().pt_scene_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Film:
    """The storage image (main.cpp:481-484): float running mean + the reference's rgba8 image."""

    def __init__(self, ctx, width, height, device_ptr=None):
        self.ctx, self.width, self.height = ctx, width, height
        self.h = C.c_void_p()
        if device_ptr is None:
            rc = lib_amd().pt_film_create(ctx.h, width, height, C.byref(self.h))
        else:
            rc = lib_amd().pt_film_create_external(ctx.h, width, height, C.c_void_p(device_ptr), C.byref(self.h))
        ctx._check(rc)

    def clear(self):
        self.ctx._check(lib_amd().pt_film_clear(self.h))

    def read_f32(self):
        a = np.zeros((self.height, self.width, 3), dtype=np.float32)
        self.ctx._check(lib_amd().pt_film_read_f32(self.h, a.ctypes.data))
        return a

    def read_bgra8(self):
        a = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self.ctx._check(lib_amd().pt_film_read_bgra8(self.h, a.ctypes.data))
        return a

    def enable_aov(self, device_planes=None):
        """Gives the film its guide buffers (include/pt_api.h pt_film_enable_aov).  device_planes: None, or AOV_COUNT entries, each None
        (the film allocates that plane) or a device pointer to caller-owned memory of the plane's size (a torch tensor's data_ptr())."""
        arr = None
        if device_planes is not None:
            assert len(device_planes) == AOV_COUNT
            arr = (C.c_void_p * AOV_COUNT)(*[C.c_void_p(p) if p else None for p in device_planes])
        self.ctx._check(lib_amd().pt_film_enable_aov(self.h, arr))

    def read_aov(self, which):
        """-> the guide plane `which` (AOV_*): float32 [H, W, 3] / [H, W], uint32 [H, W, 2] {prim, inst} for AOV_ID."""
        if which in AOV_SHAPES:
            tail, dtype = AOV_SHAPES[which]
            a = np.zeros((self.height, self.width) + tail, dtype=dtype)
        else:
            a = np.zeros((self.height, self.width, 3), dtype=np.float32)  # (the library refuses the index)
        self.ctx._check(lib_amd().pt_film_read_aov(self.h, which, a.ctypes.data))
        return a

    def denoise(self, iterations=None, sigma_normal=None, sigma_depth=None, device_out=None, params=None):
        """The a-trous filter of include/pt_api.h pt_film_denoise over the film and its guide planes -> device ms.  Arguments left at
        None take pt_denoise_params_default's values (or `params`, a DenoiseParams, as it stands).  device_out: None for a plane the
        film owns (read_denoised), or a device pointer to width*height*3 floats (a torch tensor's data_ptr())."""
        p = params if params is not None else denoise_default_params()
        return self._denoise("pt_film_denoise", p, device_out, iterations=iterations, sigma_normal=sigma_normal, sigma_depth=sigma_depth)

    def _denoise(self, fn, p, device_out, **fields):
        """the library's denoiser `fn` with params `p`, the fields that are not None written into it first -> device ms"""
        for name, v in fields.items():
            if v is not None:
                setattr(p, name, v)
        ms = C.c_float(0.0)
        self.ctx._check(getattr(lib_amd(), fn)(self.h, C.byref(p), C.c_void_p(device_out) if device_out else None, C.byref(ms)))
        return ms.value

    def _enable_plane(self, fn, device_ptr):
        self.ctx._check(getattr(lib_amd(), fn)(self.h, C.c_void_p(device_ptr) if device_ptr else None))

    def _read_plane(self, fn, tail, *more):
        """-> float32 [H, W] + tail filled by the library's plane reader `fn` (more: its further arguments)"""
        a = np.zeros((self.height, self.width) + tail, dtype=np.float32)
        self.ctx._check(getattr(lib_amd(), fn)(self.h, a.ctypes.data, *more))
        return a

    def enable_moments(self, device_ptr=None):
        """Gives the film its second-moment plane (include/pt_api.h pt_film_enable_moments): from now on pt_render blends the squared frame
        colour into it.  device_ptr: None (the film allocates it) or a device pointer to width*height*3 floats of caller-owned memory.
        Call it while the film is empty (before frame 0, or straight after clear())."""
        self._enable_plane("pt_film_enable_moments", device_ptr)

    def read_moments(self):
        """-> (float32 [H, W, 3], frames): the second-moment plane and the number of frames it and the film average."""
        n = C.c_uint32(0)
        return self._read_plane("pt_film_read_moments", (3,), C.byref(n)), n.value

    def denoise_variance(self, iterations=None, sigma_normal=None, sigma_depth=None, sigma_color=None, frames=None, device_out=None, params=None):
        """The variance-guided filter of include/pt_api.h pt_film_denoise_variance over the film, its guide planes and its second-moment
        plane -> device ms.  Arguments as in denoise(); frames: how many frames the film averages (None / 0: what pt_render recorded).
        The film-owned result is read with read_denoised / read_denoised_bgra8."""
        p = params if params is not None else denoise_variance_default_params()
        return self._denoise("pt_film_denoise_variance", p, device_out, iterations=iterations, sigma_normal=sigma_normal, sigma_depth=sigma_depth,
                             sigma_color=sigma_color, frames=frames)

    def denoise_history(self, iterations=None, sigma_normal=None, sigma_depth=None, sigma_color=None, min_history=None, n_max=None, step_frames=None,
                        device_out=None, params=None):
        """The variance-guided filter with a per-pixel variance (include/pt_api.h pt_film_denoise_history) over a film that reproject()
        left: its guide planes, its second-moment plane and its history length -> device ms.  Arguments as in denoise_variance();
        min_history: pixels whose history is shorter take the spatial estimate; n_max: the cap of the sample count; step_frames: frames
        rendered per time step.  The film-owned result is read with read_denoised / read_denoised_bgra8."""
        p = DenoiseHistoryParams.from_buffer_copy(params) if params is not None else denoise_history_default_params()
        return self._denoise("pt_film_denoise_history", p, device_out, iterations=iterations, sigma_normal=sigma_normal, sigma_depth=sigma_depth,
                             sigma_color=sigma_color, min_history=min_history, n_max=n_max, step_frames=step_frames)

    def enable_history(self, device_ptr=None):
        """Gives the film its history-length plane L (include/pt_api.h pt_film_enable_history), which pt_film_reproject reads and writes.
        device_ptr: None (the film allocates it) or a device pointer to width*height floats of caller-owned memory."""
        self._enable_plane("pt_film_enable_history", device_ptr)

    def read_history(self):
        """-> float32 [H, W]: the history length of every pixel, in reprojection steps (0 before the first reproject)."""
        return self._read_plane("pt_film_read_history", ())

    def enable_counts(self, device_ptr=None):
        """Gives the film its frame-count plane K (include/pt_api.h pt_film_enable_counts), which render_adaptive blends by and advances.
        device_ptr: None (the film allocates it) or a device pointer to width*height floats of caller-owned memory.  Call it while the
        film is empty; a film that has K is filled by render_adaptive only."""
        self._enable_plane("pt_film_enable_counts", device_ptr)

    def read_counts(self):
        """-> float32 [H, W]: the frames every pixel holds."""
        return self._read_plane("pt_film_read_counts", ())

    def enable_motion(self, device_ptr=None):
        """Gives the film its motion plane Q (include/pt_api.h pt_film_enable_motion), which pt_film_motion writes and
        pt_film_reproject_motion reads.  device_ptr: None (the film allocates it) or a device pointer to width*height*4 floats of
        caller-owned, 16-byte aligned memory."""
        self._enable_plane("pt_film_enable_motion", device_ptr)

    def read_motion(self):
        """-> float32 [H, W, 4]: per pixel where its surface point was in the previous geometry {x, y, z} and 1, or zeros (none known)."""
        return self._read_plane("pt_film_read_motion", (4,))

    def motion(self, scene, cam=None, bary_slack=None, params=None):
        """Fills the motion plane from this film's guides, rendered (render_aov) for `scene` as it is now at camera `cam`, and the scene's
        snapshot_previous() (include/pt_api.h pt_film_motion) -> device ms.  cam: a dict as default_params takes it (cam_origin,
        cam_target; missing keys are the defaults); bary_slack None: pt_motion_params_default's 1 (or `params`, a MotionParams, as it
        stands)."""
        p = MotionParams.from_buffer_copy(params) if params is not None else motion_default_params()
        for k, v in (cam or {}).items():
            if k not in ("cam_origin", "cam_target"):
                raise AttributeError(k)
            setattr(p, k, (C.c_float * 3)(*v))
        if bary_slack is not None:
            p.bary_slack = bary_slack
        ms = C.c_float(0.0)
        self.ctx._check(lib_amd().pt_film_motion(scene.h, self.h, C.byref(p), C.byref(ms)))
        return ms.value

    def reproject_motion(self, prev, cam=None, prev_cam=None, params=None, **overrides):
        """reproject() started from the motion plane (include/pt_api.h pt_film_reproject_motion): a pixel looks for its history where its
        surface point WAS, so an object moved by Scene.update / set_instances keeps it.  Arguments as reproject()."""
        return self._reproject("pt_film_reproject_motion", prev, cam, prev_cam, params, overrides)

    def reproject(self, prev, cam=None, prev_cam=None, params=None, **overrides):
        """Temporal accumulation (include/pt_api.h pt_film_reproject): this film, rendered (render + render_aov) at camera `cam`, takes over
        the history of `prev`, rendered at `prev_cam` (prev None: starts a sequence) -> device ms.  In place: rewrites this film, its
        second-moment plane, its history length and its bgra8 image.  cam / prev_cam: dicts as default_params takes them (cam_origin,
        cam_target; missing keys are the defaults).  overrides: gain, alpha, depth_tol, normal_min, max_history, flags; anything left out
        takes pt_reproject_params_default's value (or `params`, a ReprojectParams, as it stands -- its cameras too when cam / prev_cam
        are None)."""
        return self._reproject("pt_film_reproject", prev, cam, prev_cam, params, overrides)

    def _reproject(self, fn, prev, cam, prev_cam, params, overrides):
        p = ReprojectParams.from_buffer_copy(params) if params is not None else reproject_default_params()   # (the caller's object stays as it is)
        for dst, c in (("", cam), ("prev_", prev_cam)):
            for k, v in (c or {}).items():
                if k not in ("cam_origin", "cam_target"):
                    raise AttributeError(k)
                setattr(p, dst + k, (C.c_float * 3)(*v))
        for k, v in overrides.items():
            if k not in ("gain", "alpha", "depth_tol", "normal_min", "max_history", "flags"):
                raise AttributeError(k)
            setattr(p, k, v)
        ms = C.c_float(0.0)
        self.ctx._check(getattr(lib_amd(), fn)(self.h, prev.h if prev is not None else None, C.byref(p), C.byref(ms)))
        return ms.value

    def upsample(self, lo, sigma_normal=None, sigma_depth=None, source=None, device_out=None, params=None):
        """Guide-driven upsampling (include/pt_api.h pt_film_upsample): the radiance of `lo`, a smaller film with guides of its own rendered
        at the same camera, brought to this film's size by this film's guides -> device ms.  Arguments left at None take
        pt_upsample_params_default's values (or those of `params`, an UpsampleParams, which is not modified).  source: UPSAMPLE_SRC_FILM
        (lo's film) or UPSAMPLE_SRC_DENOISED (the film-owned result of lo's last denoise).  device_out: None for a plane this film owns
        (read_upsampled / read_upsampled_bgra8), or a device pointer to width*height*3 floats (a torch tensor's data_ptr())."""
        p = UpsampleParams.from_buffer_copy(params) if params is not None else upsample_default_params()
        for name, v in (("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth), ("source", source)):
            if v is not None:
                setattr(p, name, v)
        ms = C.c_float(0.0)
        self.ctx._check(lib_amd().pt_film_upsample(self.h, lo.h if lo is not None else None, C.byref(p), C.c_void_p(device_out) if device_out else None, C.byref(ms)))
        return ms.value

    def read_upsampled(self):
        """-> float32 [H, W, 3]: the film-owned result of the last upsample(device_out=None)."""
        a = np.zeros((self.height, self.width, 3), dtype=np.float32)
        self.ctx._check(lib_amd().pt_film_read_upsampled(self.h, a.ctypes.data, None))
        return a

    def read_upsampled_bgra8(self):
        a = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self.ctx._check(lib_amd().pt_film_read_upsampled(self.h, None, a.ctypes.data))
        return a

    def read_denoised(self):
        """-> float32 [H, W, 3]: the film-owned result of the last denoise(device_out=None)."""
        a = np.zeros((self.height, self.width, 3), dtype=np.float32)
        self.ctx._check(lib_amd().pt_film_read_denoised(self.h, a.ctypes.data, None))
        return a

    def read_denoised_bgra8(self):
        a = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self.ctx._check(lib_amd().pt_film_read_denoised(self.h, None, a.ctypes.data))
        return a

    def close(self):
        if self.h:
            lib_amd().pt_film_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """One rank's RCCL communicator for presenting tile-sharded renders (include/pt_api.h: pt_comm_*)."""

    def __init__(self, ctx, unique_id, world, rank):
        self.ctx, self.world, self.rank = ctx, world, rank
        self.h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        ctx._check(lib_amd().pt_comm_create(ctx.h, buf, world, rank, C.byref(self.h)))

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        rc = lib_amd().pt_comm_unique_id(buf)
        if rc != PT_OK:
            raise PtError(rc, "pt_comm_unique_id (is RCCL installed?)")
        return buf.raw

    def ranks(self):
        n = C.c_uint32()
        self.ctx._check(lib_amd().pt_comm_ranks(self.h, C.byref(n)))
        return n.value

    def present(self, film, device_image_ptr, root=0):
        self.ctx._check(lib_amd().pt_film_present(film.h, self.h, root, C.c_void_p(device_image_ptr)))

    def present_planes(self, film, dst, planes, root=0):
        """The named planes (PLANES_*) of every rank's film gathered into the film `dst` on the root (include/pt_api.h
        pt_film_present_planes) -> this rank's device ms.  dst: a Film on the root, None elsewhere."""
        ms = C.c_float(0.0)
        self.ctx._check(lib_amd().pt_film_present_planes(film.h, self.h, root, planes, dst.h if dst is not None else None, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            lib_amd().pt_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """hipMalloc'ed memory through the C-ABI (for callers without torch): .ptr, .read(dtype, shape), .write(array)"""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = C.c_void_p()
        ctx._check(lib_amd().pt_device_alloc(ctx.h, nbytes, C.byref(p)))
        self.ptr = p.value

    def read(self, dtype, shape):
        a = np.zeros(shape, dtype=dtype)
        assert a.nbytes <= self.nbytes
        self.ctx._check(lib_amd().pt_device_read(self.ctx.h, C.c_void_p(self.ptr), a.ctypes.data, a.nbytes))
        return a

    def write(self, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes <= self.nbytes
        self.ctx._check(lib_amd().pt_device_write(self.ctx.h, C.c_void_p(self.ptr), a.ctypes.data, a.nbytes))

    def close(self):
        if self.ptr:
            lib_amd().pt_device_free(self.ctx.h, C.c_void_p(self.ptr))
            self.ptr = None


def film_tile_count(film, rank, world):
    n = C.c_uint32()
    film.ctx._check(lib_amd().pt_film_tile_count(film.h, rank, world, C.byref(n)))
    return n.value


def film_pack_tiles(film, rank, world, device_ptr):
    film.ctx._check(lib_amd().pt_film_pack_tiles(film.h, rank, world, C.c_void_p(device_ptr)))


def film_unpack_tiles(film, rank, world, device_packed_ptr, device_image_ptr):
    film.ctx._check(lib_amd().pt_film_unpack_tiles(film.h, rank, world, C.c_void_p(device_packed_ptr), C.c_void_p(device_image_ptr)))


def film_planes_words(film, planes):
    """-> S: the 32-bit words per pixel of the plane set `planes` (PLANES_*); a packed tile is one record of 64 * S words."""
    n = C.c_uint32()
    film.ctx._check(lib_amd().pt_film_planes_words(film.h, planes, C.byref(n)))
    return n.value


def film_pack_planes(film, rank, world, planes, device_ptr):
    """The named planes of the film's tiles of (rank, world) into device memory of film_tile_count * 64 * S words (include/pt_api.h
    pt_film_pack_planes has the layout; distributed.pack_planes_host is its numpy mirror)."""
    film.ctx._check(lib_amd().pt_film_pack_planes(film.h, rank, world, planes, C.c_void_p(device_ptr)))


def film_unpack_planes(dst, rank, world, planes, device_packed_ptr):
    """Such a buffer into the planes of the film `dst`: exactly the pixels of that rank's tiles, and their bgra8 when PLANES_FILM is named."""
    dst.ctx._check(lib_amd().pt_film_unpack_planes(dst.h, rank, world, planes, C.c_void_p(device_packed_ptr)))


def render(scene, film, params):
    """pushConstants(frame) + traceRaysKHR(W,H,1) + waitIdle (main.cpp:656-659, 683), for
    params.frame_count consecutive frames."""
    scene.ctx._check(lib_amd().pt_render(scene.h, film.h, C.byref(params)))


def render_adaptive(scene, film, params, adaptive_params=None, **adaptive):
    """params' frames for the 8x8 tiles whose error is still above the threshold, blended by each pixel's own frame count (include/pt_api.h
    pt_render_adaptive) -> AdaptiveResult.  The film has M and K (Film.enable_moments, Film.enable_counts).  adaptive: fields of
    AdaptiveParams (threshold, rel_floor, min_frames, max_frames) over pt_adaptive_params_default's values, or over those of
    `adaptive_params`, which is not modified.  params.frame_count == 0 is a dry run: the selection alone."""
    ap = AdaptiveParams.from_buffer_copy(adaptive_params) if adaptive_params is not None else adaptive_default_params()
    for k, v in adaptive.items():
        if not hasattr(ap, k):
            raise AttributeError(k)
        setattr(ap, k, v)
    res = AdaptiveResult()
    scene.ctx._check(lib_amd().pt_render_adaptive(scene.h, film.h, C.byref(params), C.byref(ap), C.byref(res)))
    return res


def render_guided(scene, film, params, mode=GUIDED_AUTO, guided_params=None):
    """pt_render and pt_render_aov of the same params in one call (include/pt_api.h pt_render_guided) -> GuidedResult: the film and its guide
    planes (Film.enable_aov) end up as the two calls leave them, bit for bit; where a fused kernel renders, the camera rays are walked once.
    mode: GUIDED_AUTO, GUIDED_SINGLE_PASS (PtError where AUTO would take the two calls) or GUIDED_TWO_CALLS; guided_params, if given, is used
    as it is."""
    gp = guided_params if guided_params is not None else guided_default_params()
    if guided_params is None:
        gp.mode = mode
    res = GuidedResult()
    scene.ctx._check(lib_amd().pt_render_guided(scene.h, film.h, C.byref(params), C.byref(gp), C.byref(res)))
    return res


def render_aov(scene, film, params):
    """The guide buffers (first-hit albedo, normal, emission, depth, alpha, id) of params' frames into a film that has them
    (Film.enable_aov): include/pt_api.h pt_render_aov.  Blocking; the radiance film is not touched."""
    scene.ctx._check(lib_amd().pt_render_aov(scene.h, film.h, C.byref(params)))


def render_prepare(scene, film, params):
    """Allocate the workspace pt_render would use for these params (no rendering)."""
    scene.ctx._check(lib_amd().pt_render_prepare(scene.h, film.h, C.byref(params)))
