// pt_api.hip -- the C-ABI (include/pt_api.h) over the HIP kernels.  No exception leaves this file.
#include "pt_internal.h"
#include "pt_math.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

static thread_local std::string g_create_err;

// The layers below use std::vector / std::string: a failed host allocation must come back as a status, never as
// an exception through the C boundary.
template <class F>
static pt_status guarded(pt_ctx *ctx, F &&body)
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        try { if (ctx) ctx->err = "out of host memory"; } catch (...) {}
        return PT_ERR_OOM;
    } catch (const std::exception &e) {
        try { if (ctx) ctx->err = std::string("internal error: ") + e.what(); } catch (...) {}
        return PT_ERR_HIP;
    } catch (...) {
        return PT_ERR_HIP;
    }
}

// what the render entries begin with (args: the other pointers are there): the handles belong together, the device is current, the body runs guarded
template <class Body>
static pt_status render_entry(pt_scene *s, pt_film *f, bool args, Body &&body)
{
    if (!s || !f || !args) return PT_ERR_INVALID_ARG;
    if (s->ctx != f->ctx) { s->ctx->err = "scene and film belong to different contexts"; return PT_ERR_INVALID_ARG; }
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, body);
}

// ---- tuning (include/pt_api.h pt_tuning): the names PT_TUNE and the Python mirror use, in field order
static const char *const k_tune_names[] = { "refill", "lds_stack", "extend_blocks", "pipes", "stagger", "sort_bits", "pair_leaves",
                                            "pair_kernel", "topdown4", "rec64", "inst16", "inst16_blocks", "enter_min", "node_yield",
                                            "tlas_lds_kb", "term_ocap", "term_spill", "mem_budget_mb", "hbm8", "ploc_radius", "leaf_min",
                                            "tri_enter", "tri_stay", "inst_frames", "tlas_ploc", "ploc_adopt_pct", "fail_rebuild", "fused_tail",
                                            "fused_subject", "cull" };
constexpr int k_tune_count = (int)(sizeof(k_tune_names) / sizeof(k_tune_names[0]));
static_assert(sizeof(pt_tuning) == sizeof(int32_t) * (k_tune_count + 2), "pt_tuning: names and fields out of step");

static void tuning_defaults(pt_tuning *t)
{
    int32_t *f = reinterpret_cast<int32_t *>(t);
    for (size_t i = 0; i < sizeof(pt_tuning) / sizeof(int32_t); i++) f[i] = -1;
}

// "name=value,name=value" (also ';' or blanks between pairs); unknown names and malformed pairs are reported, not ignored
static bool tuning_parse(const char *text, pt_tuning *t, std::string &err)
{
    int32_t *f = reinterpret_cast<int32_t *>(t);
    std::string s(text ? text : "");
    size_t i = 0;
    while (i < s.size()) {
        while (i < s.size() && (s[i] == ',' || s[i] == ';' || s[i] == ' ')) i++;
        if (i >= s.size()) break;
        size_t e = i;
        while (e < s.size() && s[e] != ',' && s[e] != ';' && s[e] != ' ') e++;
        const std::string pair = s.substr(i, e - i);
        i = e;
        const size_t eq = pair.find('=');
        int idx = -1;
        if (eq != std::string::npos)
            for (int k = 0; k < k_tune_count; k++)
                if (pair.compare(0, eq, k_tune_names[k]) == 0) idx = k;
        char *end = nullptr;
        const long v = eq != std::string::npos ? std::strtol(pair.c_str() + eq + 1, &end, 10) : 0;
        if (idx >= 0 && std::string(k_tune_names[idx]) == "fail_rebuild") idx = -1;  // fail_rebuild is failure injection for the tests, not a knob: never from the environment
        if (idx < 0 || !end || *end != 0 || end == pair.c_str() + eq + 1 || v < INT32_MIN || v > INT32_MAX) { err = "PT_TUNE: cannot use '" + pair + "'"; return false; }
        f[idx] = (int32_t)v;
    }
    return true;
}

extern "C" {

pt_status pt_ctx_get_tuning(const pt_ctx *ctx, pt_tuning *out)
{
    if (!ctx || !out) return PT_ERR_INVALID_ARG;
    *out = ctx->tune;
    return PT_OK;
}

pt_status pt_ctx_set_tuning(pt_ctx *ctx, const pt_tuning *in)
{
    if (!ctx || !in) return PT_ERR_INVALID_ARG;
    ctx->tune = *in;
    // mem_budget_mb: > 0 a budget, 0 none, -1 the built-in choice (PT_DEFAULT_MEM_BUDGET_MB) -- so writing back what pt_ctx_get_tuning returned
    // restores the state it described (pt_ctx_create applies the same rule)
    ctx->mem_budget = pt_budget_bytes(in->mem_budget_mb);
    return PT_OK;
}

pt_status pt_ctx_create(int device, void *stream, pt_ctx **out)
{
    if (!out) return PT_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_create_err = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        (void)hipGetLastError();
        return PT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        g_create_err = "device ordinal out of range";
        return PT_ERR_INVALID_ARG;
    }
    pt_ctx *ctx = new (std::nothrow) pt_ctx();
    if (!ctx) return PT_ERR_OOM;
    ctx->device = device;
    auto fail = [&](const char *what, hipError_t err) {
        g_create_err = std::string(what) + ": " + hipGetErrorString(err);
        pt_ctx_destroy(ctx);
        return PT_ERR_HIP;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return fail("hipGetDeviceProperties", e);
    ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // the only two environment variables the library reads, both here and only here
    tuning_defaults(&ctx->tune);
    const char *const env[2] = { "PT_TUNE", "PT_MEM_BUDGET_MB" };
    const char *val[2];
    for (int k = 0; k < 2; k++) val[k] = getenv(env[k]);
    if (val[0] && !tuning_parse(val[0], &ctx->tune, g_create_err)) { pt_ctx_destroy(ctx); return PT_ERR_INVALID_ARG; }
    if (val[1]) ctx->tune.mem_budget_mb = (int32_t)std::max(0ll, std::min(atoll(val[1]), 1ll << 30));  // (0: no bound)
    ctx->mem_budget = pt_budget_bytes(ctx->tune.mem_budget_mb);
    if (stream) {
        ctx->stream = reinterpret_cast<hipStream_t>(stream);
    } else {
        if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
        ctx->own_stream = true;
    }
    if ((e = hipEventCreate(&ctx->ev_a)) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipEventCreate(&ctx->ev_b)) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipMalloc((void **)&ctx->d_stats, sizeof(unsigned long long) * PT_N_STATS_ALL)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMemset(ctx->d_stats, 0, sizeof(unsigned long long) * PT_N_STATS_ALL)) != hipSuccess) return fail("hipMemset", e);
    if ((e = hipMalloc(&ctx->d_rad, sizeof(ctx->h_rad))) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMemset(ctx->d_rad, 0, sizeof(ctx->h_rad))) != hipSuccess) return fail("hipMemset", e);
    *out = ctx;
    return PT_OK;
}

void pt_ctx_destroy(pt_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->d_stats) (void)hipFree(ctx->d_stats);
    if (ctx->d_rad) (void)hipFree(ctx->d_rad);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->d_spill) (void)hipFree(ctx->d_spill);
    ptt_free(ctx);
    ptr_free(ctx);
    if (ctx->ev_a) (void)hipEventDestroy(ctx->ev_a);
    if (ctx->ev_b) (void)hipEventDestroy(ctx->ev_b);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->h_poll) (void)hipHostFree(ctx->h_poll);
    for (int k = 0; k < PT_MAX_PIPES; k++)
        for (int j = 0; j < 2; j++)
            if (ctx->ev_poll[k][j]) (void)hipEventDestroy(ctx->ev_poll[k][j]);
    for (int k = 0; k < PT_MAX_PIPES; k++)
        if (ctx->ev_shade[k]) (void)hipEventDestroy(ctx->ev_shade[k]);
    for (int k = 0; k < PT_MAX_PIPES; k++) {
        if (ctx->ev_join[k]) (void)hipEventDestroy(ctx->ev_join[k]);
        if (ctx->pipe_stream[k]) (void)hipStreamDestroy(ctx->pipe_stream[k]);
    }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *pt_last_error(const pt_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

pt_status pt_sync(pt_ctx *ctx)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

pt_status pt_scene_create(pt_ctx *ctx, const float *vertices, uint32_t n_verts, const uint32_t *indices, uint32_t n_tris,
                          const float *faces, pt_scene **out)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    if (!out || !vertices || !indices || !faces) { ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n_tris == 0 || n_verts == 0) { ctx->err = "empty scene"; return PT_ERR_INVALID_ARG; }
    // BVH4 leaf words keep the first sorted position in bits 0..27 and (count - 1) in bits 28..30
    if (n_tris >= (1u << 28)) { ctx->err = "too many triangles (the BVH4 leaf encoding holds 2^28 - 1)"; return PT_ERR_INVALID_ARG; }
    for (size_t i = 0; i < 3 * (size_t)n_tris; i++)
        if (indices[i] >= n_verts) { ctx->err = "vertex index out of range"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    pt_scene *s = new (std::nothrow) pt_scene();
    if (!s) return PT_ERR_OOM;
    s->ctx = ctx;
    pt_status rc = guarded(ctx, [&] { return ptb_build_scene(s, { vertices, n_verts, indices, faces, false }, n_tris); });
    if (rc != PT_OK) { pt_scene_destroy(s); return rc; }
    *out = s;
    return PT_OK;
}

// The arrays in device memory: the refusals of pt_scene_create, the index check as a kernel (scene_device.hip) before any kernel follows an index.
// A failure waits for the stream before it returns: the caller's arrays are not read after the call, whatever it answers.
pt_status pt_scene_create_device(pt_ctx *ctx, const void *d_vertices, uint32_t n_verts, const void *d_indices, uint32_t n_tris, const void *d_faces,
                                 pt_scene **out)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    if (!out || !d_vertices || !d_indices || !d_faces) { ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    *out = nullptr;
    if (n_tris == 0 || n_verts == 0) { ctx->err = "empty scene"; return PT_ERR_INVALID_ARG; }
    if (n_tris >= (1u << 28)) { ctx->err = "too many triangles (the BVH4 leaf encoding holds 2^28 - 1)"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_TRY(guarded(ctx, [&] { return ptsd_check_indices(ctx, static_cast<const uint32_t *>(d_indices), n_tris, n_verts); }));
    pt_scene *s = new (std::nothrow) pt_scene();
    if (!s) return PT_ERR_OOM;
    s->ctx = ctx;
    const pt_geometry g = { static_cast<const float *>(d_vertices), n_verts, static_cast<const uint32_t *>(d_indices), static_cast<const float *>(d_faces), true };
    pt_status rc = guarded(ctx, [&] { return ptb_build_scene(s, g, n_tris); });
    if (rc != PT_OK) { (void)hipStreamSynchronize(ctx->stream); pt_scene_destroy(s); return rc; }
    *out = s;
    return PT_OK;
}

pt_status pt_scene_set_instances(pt_scene *s, const float *xforms3x4, uint32_t n)
{
    if (!s) return PT_ERR_INVALID_ARG;
    if (n && !xforms3x4) { s->ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    if (n >= (1u << 28)) { s->ctx->err = "too many instances"; return PT_ERR_INVALID_ARG; }
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return ptb_set_instances(s, xforms3x4, n); });
}

// The matrices in device memory: the refusals of pt_scene_set_instances, its loop as a kernel (scene_instances.hip).  A failure waits for the
// stream before it returns: the caller's array is not read after the call, whatever it answers.
pt_status pt_scene_set_instances_device(pt_scene *s, const void *d_xforms3x4, uint32_t n)
{
    if (!s) return PT_ERR_INVALID_ARG;
    if (n && !d_xforms3x4) { s->ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    if (n >= (1u << 28)) { s->ctx->err = "too many instances"; return PT_ERR_INVALID_ARG; }
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    const pt_status rc = guarded(s->ctx, [&] { return ptb_set_instances_device(s, static_cast<const float *>(d_xforms3x4), n); });
    if (rc != PT_OK) (void)hipStreamSynchronize(s->ctx->stream);
    return rc;
}

void pt_scene_destroy(pt_scene *s)
{
    if (!s) return;
    ptm_free_previous(s);
    ptb_free_instances(s);
    ptb_free_scene_buffers(s);
    delete s;
}

pt_status pt_scene_set_bvh_quality(pt_scene *s, uint32_t quality)
{
    if (!s) return PT_ERR_INVALID_ARG;
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return ptb_set_bvh_quality(s, quality); });
}

pt_status pt_scene_update(pt_scene *s, const float *vertices, uint32_t n_verts, const uint32_t *indices, uint32_t n_tris, uint32_t mode)
{
    if (!s) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = s->ctx;
    if (!vertices || !indices) { ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    if (mode > PT_SCENE_UPDATE_REBUILD) { ctx->err = "unknown update mode"; return PT_ERR_INVALID_ARG; }
    if (n_tris == 0 || n_verts == 0) { ctx->err = "empty scene"; return PT_ERR_INVALID_ARG; }
    if (n_tris != s->n_tris) { ctx->err = "an update keeps the scene's triangles (and their materials): n_tris must equal the scene's"; return PT_ERR_INVALID_ARG; }
    for (size_t i = 0; i < 3 * (size_t)n_tris; i++)
        if (indices[i] >= n_verts) { ctx->err = "vertex index out of range"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    return guarded(ctx, [&] { return ptb_update_scene(s, { vertices, n_verts, indices, nullptr, false }, mode); });
}

pt_status pt_scene_update_device(pt_scene *s, const void *d_vertices, uint32_t n_verts, const void *d_indices, uint32_t n_tris, uint32_t mode)
{
    if (!s) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = s->ctx;
    if (!d_vertices || !d_indices) { ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    if (mode > PT_SCENE_UPDATE_REBUILD) { ctx->err = "unknown update mode"; return PT_ERR_INVALID_ARG; }
    if (n_tris == 0 || n_verts == 0) { ctx->err = "empty scene"; return PT_ERR_INVALID_ARG; }
    if (n_tris != s->n_tris) { ctx->err = "an update keeps the scene's triangles (and their materials): n_tris must equal the scene's"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    // on the context's stream, so behind whatever is queued there; nothing of the scene has changed when it refuses
    PT_TRY(guarded(ctx, [&] { return ptsd_check_indices(ctx, static_cast<const uint32_t *>(d_indices), n_tris, n_verts); }));
    const pt_geometry g = { static_cast<const float *>(d_vertices), n_verts, static_cast<const uint32_t *>(d_indices), nullptr, true };
    const pt_status rc = guarded(ctx, [&] { return ptb_update_scene(s, g, mode); });
    if (rc != PT_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// New per-face materials for the scene's triangles (scene_build.hip ptb_set_faces).  The host form uploads into the staged copy the device form
// fills by a device-to-device copy: one path from there, one set of bits.  A failure waits for the stream before it returns: the caller's array
// is not read after the call, whatever it answers.
static pt_status set_faces(pt_scene *s, const float *faces, uint32_t n_tris, bool on_device)
{
    if (!s) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = s->ctx;
    if (!faces) { ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    if (n_tris != s->n_tris) { ctx->err = "new materials keep the scene's triangles: n_tris must equal the scene's"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const pt_status rc = guarded(ctx, [&] { return ptb_set_faces(s, faces, on_device); });
    if (rc != PT_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

pt_status pt_scene_set_faces(pt_scene *s, const float *faces, uint32_t n_tris) { return set_faces(s, faces, n_tris, false); }

pt_status pt_scene_set_faces_device(pt_scene *s, const void *d_faces, uint32_t n_tris)
{
    return set_faces(s, static_cast<const float *>(d_faces), n_tris, true);
}

// The kept copy of the materials: of source lifetime, so a broken scene answers too.
pt_status pt_scene_read_faces(const pt_scene *s, float *faces)
{
    if (!s) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = s->ctx;
    if (!faces) { ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(faces, s->d_faces, sizeof(float) * 6 * (size_t)s->n_tris, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_scene_get_info(const pt_scene *s, pt_scene_info *info)
{
    if (!s || !info) return PT_ERR_INVALID_ARG;
    info->n_tris = s->n_tris; info->n_nodes = s->n_nodes; info->bvh_height = s->height;
    info->n_wide_nodes = s->n_wide;
    info->n_instances = s->n_inst;
    info->n_tlas_nodes = s->n_tlas_wide;
    info->leaf_max = PT_BLAS_LEAF_MAX;
    info->n_wide8_nodes = s->n_wide8; info->wide8_levels = s->levels8; info->device_bytes8 = s->device_bytes8;  // (0 until built: big scenes, first request)
    info->bvh4_builder = s->bvh4_builder;
    for (int k = 0; k < 3; k++) { info->bbox_min[k] = s->bmin[k]; info->bbox_max[k] = s->bmax[k]; }
    info->build_ms = s->build_ms;
    info->device_bytes = s->device_bytes + s->prev.bytes;  // (prev: 0 until pt_scene_snapshot_previous)
    // (normalised by the root's area = the scene box's: the same for both trees)
    const double ex = (double)s->bmax[0] - s->bmin[0], ey = (double)s->bmax[1] - s->bmin[1], ez = (double)s->bmax[2] - s->bmin[2];
    const double root = (ex * ey + ey * ez) + ez * ex;
    info->tree_area_lbvh = root > 0.0 ? (float)(s->area_lbvh / root) : 0.f;
    info->tree_area_ploc = root > 0.0 ? (float)(s->area_ploc / root) : 0.f;
    return PT_OK;
}

pt_status pt_scene_read_bvh(const pt_scene *s, uint64_t *keys, uint32_t *prim_of_pos, uint32_t *nodes16)
{
    if (!s) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = s->ctx;
    if (s->broken) { const pt_status rb = guarded(ctx, [&] { return ptb_repair(const_cast<pt_scene *>(s)); }); if (rb != PT_OK) return rb; }
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (keys) PT_HIP(ctx, hipMemcpy(keys, s->d_keys, sizeof(uint64_t) * (size_t)s->n_tris, hipMemcpyDeviceToHost));
    if (prim_of_pos) PT_HIP(ctx, hipMemcpy(prim_of_pos, s->d_prim_of, sizeof(uint32_t) * (size_t)s->n_tris, hipMemcpyDeviceToHost));
    if (nodes16) PT_HIP(ctx, hipMemcpy(nodes16, s->d_nodes, 64 * (size_t)s->n_nodes, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_scene_read_bvh4(const pt_scene *s, uint32_t *nodes32)
{
    if (!s || !nodes32) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = s->ctx;
    if (s->broken) { const pt_status rb = guarded(ctx, [&] { return ptb_repair(const_cast<pt_scene *>(s)); }); if (rb != PT_OK) return rb; }
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(nodes32, s->d_wide, 128 * (size_t)s->n_wide, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_scene_read_bvh8(const pt_scene *s, uint32_t *nodes32, uint32_t *prim_of_pos8)
{
    if (!s) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = s->ctx;
    if (s->broken) { const pt_status rb = guarded(ctx, [&] { return ptb_repair(const_cast<pt_scene *>(s)); }); if (rb != PT_OK) return rb; }
    if (!s->d_wide8) {   // big scenes build their 8-wide nodes on first request
        const pt_status rc = guarded(ctx, [&] { return ptb_ensure_wide8(const_cast<pt_scene *>(s)); });
        if (rc != PT_OK) return rc;
    }
    if (!s->d_wide8) { ctx->err = "the scene has no BVH8 (a single triangle, or instanced)"; return PT_ERR_UNSUPPORTED; }
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (nodes32) PT_HIP(ctx, hipMemcpy(nodes32, s->d_wide8, 64 * (size_t)s->n_wide8, hipMemcpyDeviceToHost));
    if (prim_of_pos8) PT_HIP(ctx, hipMemcpy(prim_of_pos8, s->d_prim_of8, sizeof(uint32_t) * (size_t)s->n_tris, hipMemcpyDeviceToHost));
    return PT_OK;
}

static pt_status film_create(pt_ctx *ctx, uint32_t w, uint32_t h, void *ext, pt_film **out)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    if (!out || w == 0 || h == 0 || w > 524280u || h > 524280u || (uint64_t)w * h >= (1ull << 28)) { ctx->err = "bad film size"; return PT_ERR_INVALID_ARG; }
    *out = nullptr;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    pt_film *f = new (std::nothrow) pt_film();
    if (!f) return PT_ERR_OOM;
    f->ctx = ctx; f->w = w; f->h = h;
    hipError_t e = hipSuccess;
    if (ext) { f->d_rgb = static_cast<float *>(ext); f->own_rgb = false; }
    else e = hipMalloc((void **)&f->d_rgb, sizeof(float) * 3 * (size_t)w * h);
    if (e == hipSuccess) e = hipMalloc((void **)&f->d_bgra, 4 * (size_t)w * h);
    if (e != hipSuccess) { ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e); pt_film_destroy(f); return PT_ERR_OOM; }
    pt_status rc = pt_film_clear(f);
    if (rc != PT_OK) { pt_film_destroy(f); return rc; }
    *out = f;
    return PT_OK;
}

pt_status pt_film_create(pt_ctx *ctx, uint32_t w, uint32_t h, pt_film **out) { return film_create(ctx, w, h, nullptr, out); }

pt_status pt_film_create_external(pt_ctx *ctx, uint32_t w, uint32_t h, void *device_rgb_f32, pt_film **out)
{
    if (ctx && !device_rgb_f32) { ctx->err = "null device buffer"; return PT_ERR_INVALID_ARG; }
    return film_create(ctx, w, h, device_rgb_f32, out);
}

pt_status pt_film_clear(pt_film *f)
{
    if (!f) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    PT_HIP(ctx, hipMemsetAsync(f->d_rgb, 0, sizeof(float) * 3 * (size_t)f->w * f->h, ctx->stream));
    PT_HIP(ctx, hipMemsetAsync(f->d_bgra, 0, 4 * (size_t)f->w * f->h, ctx->stream));
    const pt_status rc = pta_clear(f, ctx->stream);  // the guide buffers, if the film has them
    if (rc != PT_OK) return rc;
    PT_TRY(pt_planes_clear(f, ctx->stream));  // M, L, Q and K, where the film has them
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

pt_status pt_film_read_f32(pt_film *f, float *rgb)
{
    if (!f || !rgb) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(rgb, f->d_rgb, sizeof(float) * 3 * (size_t)f->w * f->h, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_film_read_bgra8(pt_film *f, uint8_t *bgra)
{
    if (!f || !bgra) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(bgra, f->d_bgra, 4 * (size_t)f->w * f->h, hipMemcpyDeviceToHost));
    return PT_OK;
}

void pt_film_destroy(pt_film *f)
{
    if (!f) return;
    ptw_free_work(f);
    pta_free(f);
    ptd_free(f);
    ptu_free(f);
    ptad_free(f);
    ptg_free(f);
    pt_planes_free(f);
    if (f->own_rgb) (void)hipFree(f->d_rgb);
    (void)hipFree(f->d_bgra);
    delete f;
}

void pt_params_default(pt_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->frame = 0; p->frame_count = 1;
    p->width = 1024; p->height = 1024;          // main.cpp:16-17
    p->spp_per_frame = 32; p->max_depth = 8;    // raygen.rgen:43, 62
    p->tmin = 0.001f; p->tmax = 10000.0f;       // raygen.rgen:71, 73
    p->cam_origin[0] = 0.f; p->cam_origin[1] = -1.f; p->cam_origin[2] = 5.f;  // raygen.rgen:55
    p->cam_target[0] = 0.f; p->cam_target[1] = -1.f; p->cam_target[2] = 2.f;  // raygen.rgen:56
    p->env[0] = 0.7f; p->env[1] = 0.6f; p->env[2] = 0.5f;                     // miss.rmiss:10
    p->rank = 0; p->world = 1;
    p->pipeline = PT_PIPELINE_AUTO;
    p->frames_in_flight = 0;
    p->flags = 0;
    p->extend = PT_EXTEND_AUTO;
    p->sample_groups = 0;
}

pt_status pt_render(pt_scene *s, pt_film *f, const pt_params *p) { return render_entry(s, f, p, [&] { return ptw_render(s, f, p); }); }
pt_status pt_render_prepare(pt_scene *s, pt_film *f, const pt_params *p) { return render_entry(s, f, p, [&] { return ptw_prepare(s, f, p); }); }

pt_status pt_film_enable_aov(pt_film *f, void *const *device_planes)
{
    if (!f) return PT_ERR_INVALID_ARG;
    PT_HIP(f->ctx, hipSetDevice(f->ctx->device));
    return guarded(f->ctx, [&] { return pta_enable(f, device_planes); });
}

pt_status pt_render_aov(pt_scene *s, pt_film *f, const pt_params *p)
{
    if (!s || !f || !p) return PT_ERR_INVALID_ARG;
    if (s->ctx != f->ctx) { s->ctx->err = "scene and film belong to different contexts"; return PT_ERR_INVALID_ARG; }
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return pta_render(s, f, p); });
}

pt_status pt_film_read_aov(pt_film *f, uint32_t which, void *host_out)
{
    if (!f || !host_out) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    if (!f->aov.enabled) { ctx->err = "the film has no guide buffers: pt_film_enable_aov first"; return PT_ERR_INVALID_ARG; }
    if (which >= PT_AOV_COUNT) { ctx->err = "unknown guide buffer"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(host_out, f->aov.plane[which], pta_plane_bytes(f, which), hipMemcpyDeviceToHost));
    return PT_OK;
}

void pt_denoise_params_default(pt_denoise_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->iterations = 5;
    p->sigma_normal = 0.5f;
    p->sigma_depth = 0.1f;
}

pt_status pt_film_denoise(pt_film *f, const pt_denoise_params *p, void *device_out_rgb_f32, float *device_ms)
{
    if (!f || !p) return PT_ERR_INVALID_ARG;
    PT_HIP(f->ctx, hipSetDevice(f->ctx->device));
    return guarded(f->ctx, [&] { return ptd_denoise(f, p, device_out_rgb_f32, device_ms); });
}

pt_status pt_film_read_denoised(pt_film *f, float *rgb, uint8_t *bgra)
{
    if (!f) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    if (!f->dn.have_out) { ctx->err = "no denoised image: pt_film_denoise with a NULL output first"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rgb) PT_HIP(ctx, hipMemcpy(rgb, f->dn.d_out, sizeof(float) * 3 * (size_t)f->w * f->h, hipMemcpyDeviceToHost));
    if (bgra) PT_HIP(ctx, hipMemcpy(bgra, f->dn.d_out_bgra, 4 * (size_t)f->w * f->h, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_film_enable_moments(pt_film *f, void *device_m2_f32)
{
    if (!f) return PT_ERR_INVALID_ARG;
    return guarded(f->ctx, [&] { return pt_plane_enable(f, f->m2, device_m2_f32, sizeof(float) * 3 * (size_t)f->w * f->h, 0, "pt_film_enable_moments", "the film already has a second-moment plane"); });
}

pt_status pt_film_read_moments(pt_film *f, float *m2, uint32_t *frames)
{
    if (!f) return PT_ERR_INVALID_ARG;
    const pt_status rc = pt_plane_read(f, f->m2, m2, sizeof(float) * 3 * (size_t)f->w * f->h, PT_NO_M_MSG " first");
    if (rc == PT_OK && frames) *frames = f->m2.frames;
    return rc;
}

void pt_denoise_variance_params_default(pt_denoise_variance_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->iterations = 5;
    p->sigma_normal = 0.5f;
    p->sigma_depth = 0.1f;
    p->sigma_color = 3.0f;
}

pt_status pt_film_denoise_variance(pt_film *f, const pt_denoise_variance_params *p, void *device_out_rgb_f32, float *device_ms)
{
    if (!f || !p) return PT_ERR_INVALID_ARG;
    PT_HIP(f->ctx, hipSetDevice(f->ctx->device));
    return guarded(f->ctx, [&] { return ptd_denoise_variance(f, p, device_out_rgb_f32, device_ms); });
}

void pt_denoise_history_params_default(pt_denoise_history_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->iterations = 5;
    p->sigma_normal = 0.5f;
    p->sigma_depth = 0.1f;
    p->sigma_color = 3.0f;
    p->min_history = 4.0f;
    p->n_max = 9.0f;
    p->step_frames = 1;
}

pt_status pt_film_denoise_history(pt_film *f, const pt_denoise_history_params *p, void *device_out_rgb_f32, float *device_ms)
{
    if (!f || !p) return PT_ERR_INVALID_ARG;
    PT_HIP(f->ctx, hipSetDevice(f->ctx->device));
    return guarded(f->ctx, [&] { return ptd_denoise_history(f, p, device_out_rgb_f32, device_ms); });
}

pt_status pt_film_enable_history(pt_film *f, void *device_len_f32)
{
    if (!f) return PT_ERR_INVALID_ARG;
    return guarded(f->ctx, [&] { return pt_plane_enable(f, f->hist, device_len_f32, sizeof(float) * (size_t)f->w * f->h, 0, "pt_film_enable_history", "the film already has a history-length plane"); });
}

pt_status pt_film_read_history(pt_film *f, float *len)
{
    if (!f) return PT_ERR_INVALID_ARG;
    if (!len) return pt_bad(f->ctx, "null argument");
    return pt_plane_read(f, f->hist, len, sizeof(float) * (size_t)f->w * f->h, PT_NO_L_MSG " first");
}

void pt_reproject_params_default(pt_reproject_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    pt_params cam;
    pt_params_default(&cam);
    for (int k = 0; k < 3; k++) {
        p->cam_origin[k] = p->prev_cam_origin[k] = cam.cam_origin[k];
        p->cam_target[k] = p->prev_cam_target[k] = cam.cam_target[k];
    }
    p->gain = 1.0f;
    p->alpha = 0.2f;
    p->depth_tol = 0.1f;
    p->normal_min = 0.9f;
    p->max_history = 32;
    p->flags = PT_REPROJECT_MATCH_ID;
}

pt_status pt_film_reproject(pt_film *f, pt_film *prev, const pt_reproject_params *p, float *device_ms)
{
    if (!f || !p) return PT_ERR_INVALID_ARG;
    PT_HIP(f->ctx, hipSetDevice(f->ctx->device));
    return guarded(f->ctx, [&] { return ptr_reproject(f, prev, p, device_ms); });
}

pt_status pt_scene_snapshot_previous(pt_scene *s)
{
    if (!s) return PT_ERR_INVALID_ARG;
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return ptm_snapshot(s); });
}

pt_status pt_film_enable_motion(pt_film *f, void *device_q_f32x4)
{
    if (!f) return PT_ERR_INVALID_ARG;
    return guarded(f->ctx, [&] { return pt_plane_enable(f, f->mo, device_q_f32x4, sizeof(float4) * (size_t)f->w * f->h, 16, "pt_film_enable_motion", "the film already has a motion plane"); });
}

pt_status pt_film_read_motion(pt_film *f, float *q4)
{
    if (!f) return PT_ERR_INVALID_ARG;
    if (!q4) return pt_bad(f->ctx, "null argument");
    return pt_plane_read(f, f->mo, q4, sizeof(float4) * (size_t)f->w * f->h, PT_NO_Q_MSG " first");
}

void pt_motion_params_default(pt_motion_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    pt_params cam;
    pt_params_default(&cam);
    for (int k = 0; k < 3; k++) { p->cam_origin[k] = cam.cam_origin[k]; p->cam_target[k] = cam.cam_target[k]; }
    p->bary_slack = 1.0f;
}

pt_status pt_film_motion(pt_scene *s, pt_film *f, const pt_motion_params *p, float *device_ms)
{
    if (!s || !f || !p) return PT_ERR_INVALID_ARG;
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return ptm_motion(s, f, p, device_ms); });
}

pt_status pt_film_reproject_motion(pt_film *f, pt_film *prev, const pt_reproject_params *p, float *device_ms)
{
    if (!f || !p) return PT_ERR_INVALID_ARG;
    PT_HIP(f->ctx, hipSetDevice(f->ctx->device));
    return guarded(f->ctx, [&] { return ptr_reproject(f, prev, p, device_ms, true); });
}

void pt_upsample_params_default(pt_upsample_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->sigma_normal = 1.0f;   // the best of the grid of DESIGN.md section 18
    p->sigma_depth = 0.2f;
    p->source = PT_UPSAMPLE_SRC_FILM;
}

pt_status pt_film_upsample(pt_film *f, pt_film *lo, const pt_upsample_params *p, void *device_out_rgb_f32, float *device_ms)
{
    if (!f || !lo || !p) return PT_ERR_INVALID_ARG;
    PT_HIP(f->ctx, hipSetDevice(f->ctx->device));
    return guarded(f->ctx, [&] { return ptu_upsample(f, lo, p, device_out_rgb_f32, device_ms); });
}

pt_status pt_film_read_upsampled(pt_film *f, float *rgb, uint8_t *bgra)
{
    if (!f) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    if (!f->up.have_out) { ctx->err = "no upsampled image: pt_film_upsample with a NULL output first"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rgb) PT_HIP(ctx, hipMemcpy(rgb, f->up.d_out, sizeof(float) * 3 * (size_t)f->w * f->h, hipMemcpyDeviceToHost));
    if (bgra) PT_HIP(ctx, hipMemcpy(bgra, f->up.d_out_bgra, 4 * (size_t)f->w * f->h, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_film_enable_counts(pt_film *f, void *device_k_f32)
{
    if (!f) return PT_ERR_INVALID_ARG;
    return guarded(f->ctx, [&] { return pt_plane_enable(f, f->cnt, device_k_f32, sizeof(float) * (size_t)f->w * f->h, 0, "pt_film_enable_counts", "the film already has a frame-count plane"); });
}

pt_status pt_film_read_counts(pt_film *f, float *k)
{
    if (!f) return PT_ERR_INVALID_ARG;
    if (!k) return pt_bad(f->ctx, "null argument");
    return pt_plane_read(f, f->cnt, k, sizeof(float) * (size_t)f->w * f->h, PT_NO_K_MSG " first");
}

void pt_adaptive_params_default(pt_adaptive_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->threshold = 0.05f;
    p->rel_floor = 0.01f;
    p->min_frames = 4;
}

pt_status pt_render_adaptive(pt_scene *s, pt_film *f, const pt_params *p, const pt_adaptive_params *ap, pt_adaptive_result *result)
{
    return render_entry(s, f, p && ap, [&] { return ptw_render_adaptive(s, f, p, ap, result); });
}

void pt_guided_params_default(pt_guided_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->mode = PT_GUIDED_AUTO;
}

pt_status pt_render_guided(pt_scene *s, pt_film *f, const pt_params *p, const pt_guided_params *gp, pt_guided_result *result)
{
    return render_entry(s, f, p && gp, [&] { return ptw_render_guided(s, f, p, gp, result); });
}

pt_status pt_trace(pt_scene *s, const float *rays6, uint32_t n, float tmin, float tmax, uint32_t extend, pt_hit *hits)
{
    if (!s) return PT_ERR_INVALID_ARG;
    if (n && (!rays6 || !hits)) { s->ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return ptw_trace(s, rays6, n, tmin, tmax, extend, hits); });
}

void pt_trace_desc_default(pt_trace_desc *d)
{
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->tmin = 0.001f;
    d->tmax = 10000.0f;
    d->mode = PT_TRACE_CLOSEST;
    d->extend = PT_EXTEND_AUTO;
}

pt_status pt_trace_device(pt_scene *s, const pt_trace_desc *d, uint64_t n, float *device_ms)
{
    if (!s) return PT_ERR_INVALID_ARG;
    if (!d) return pt_bad(s->ctx, "null argument");
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return ptt_trace_device(s, d, n, device_ms); });
}

void pt_nearest_desc_default(pt_nearest_desc *d)
{
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->max_dist = INFINITY;
    d->form = PT_NEAREST_AUTO;
}

pt_status pt_nearest_device(pt_scene *s, const pt_nearest_desc *d, uint64_t n, float *device_ms)
{
    if (!s) return PT_ERR_INVALID_ARG;
    if (!d) return pt_bad(s->ctx, "null argument");
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return ptn_nearest_device(s, d, n, device_ms); });
}

void pt_crossings_desc_default(pt_crossings_desc *d)
{
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->tmax = INFINITY;
    d->form = PT_CROSSINGS_AUTO;
}

pt_status pt_crossings_device(pt_scene *s, const pt_crossings_desc *d, uint64_t n, float *device_ms)
{
    if (!s) return PT_ERR_INVALID_ARG;
    if (!d) return pt_bad(s->ctx, "null argument");
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return ptx_crossings_device(s, d, n, device_ms); });
}

pt_status pt_trace_workspace_bytes(const pt_ctx *ctx, uint64_t *bytes)
{
    if (!ctx || !bytes) return PT_ERR_INVALID_ARG;
    *bytes = ctx->tr.bytes;
    return PT_OK;
}

void pt_radiance_desc_default(pt_radiance_desc *d)
{
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->tmin = 0.001f;
    d->tmax = 10000.0f;
    d->env[0] = 0.7f; d->env[1] = 0.6f; d->env[2] = 0.5f;  // miss.rmiss:10
    d->spp = 32;
    d->max_depth = 8;
    d->extend = PT_EXTEND_AUTO;
}

pt_status pt_radiance_device(pt_scene *s, const pt_radiance_desc *d, uint64_t n, float *device_ms)
{
    if (!s) return PT_ERR_INVALID_ARG;
    if (!d) return pt_bad(s->ctx, "null argument");
    PT_HIP(s->ctx, hipSetDevice(s->ctx->device));
    return guarded(s->ctx, [&] { return ptr_radiance_device(s, d, n, device_ms); });
}

pt_status pt_radiance_workspace_bytes(const pt_ctx *ctx, uint64_t *bytes)
{
    if (!ctx || !bytes) return PT_ERR_INVALID_ARG;
    *bytes = (uint64_t)ctx->rd.bytes + (uint64_t)ctx->rd.sq_bytes + (uint64_t)ctx->rd.f_bytes;
    return PT_OK;
}

pt_status pt_device_alloc(pt_ctx *ctx, size_t bytes, void **out)
{
    if (!ctx || !out) return PT_ERR_INVALID_ARG;
    *out = nullptr;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? PT_ERR_OOM : PT_ERR_HIP;
    }
    return PT_OK;
}

pt_status pt_device_free(pt_ctx *ctx, void *p)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipFree(p));
    return PT_OK;
}

pt_status pt_device_read(pt_ctx *ctx, const void *src, void *dst, size_t bytes)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    if (!src || !dst) { ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

pt_status pt_device_write(pt_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    if (!src || !dst) { ctx->err = "null argument"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

pt_status pt_get_stats(pt_ctx *ctx, pt_stats *out)
{
    if (!ctx || !out) return PT_ERR_INVALID_ARG;
    unsigned long long h[PT_N_STATS];
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(h, ctx->d_stats, sizeof(h), hipMemcpyDeviceToHost));
    ctx->stats.rays = h[PT_STAT_RAYS];
    ctx->stats.nodes_visited = h[PT_STAT_NODES];
    ctx->stats.tris_tested = h[PT_STAT_TRIS];
    ctx->stats.node_steps = h[PT_STAT_NODE_STEPS];
    ctx->stats.tri_steps = h[PT_STAT_TRI_STEPS];
    ctx->stats.wave_refills = h[PT_STAT_WAVE_REFILLS]; ctx->stats.wave_pops = h[PT_STAT_WAVE_POPS]; ctx->stats.wave_hit_blocks = h[PT_STAT_WAVE_HIT_BLOCKS];
    ctx->stats.wave_finishes = h[PT_STAT_WAVE_FINISHES]; ctx->stats.wave_iterations = h[PT_STAT_WAVE_ITERS];
    ctx->stats.leaf_lanes = h[PT_STAT_LEAF_LANES]; ctx->stats.pop_lanes = h[PT_STAT_POP_LANES]; ctx->stats.hit_lanes = h[PT_STAT_HIT_LANES];
    ctx->stats.enter_steps = h[PT_STAT_ENTER_STEPS]; ctx->stats.enter_lanes = h[PT_STAT_ENTER_LANES];
    ctx->stats.rays_culled = h[PT_STAT_RAYS_CULLED];    *out = ctx->stats;
    return PT_OK;
}

pt_status pt_get_block_counts(pt_ctx *ctx, uint64_t *waves_lanes, uint32_t n_blocks)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    if (!waves_lanes || n_blocks > (uint32_t)PT_N_BLOCKS) { ctx->err = "pt_get_block_counts: null array or more than 32 blocks"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(waves_lanes, ctx->d_stats + PT_N_STATS, sizeof(unsigned long long) * 2 * n_blocks, hipMemcpyDeviceToHost));
    return PT_OK;
}

pt_status pt_reset_stats(pt_ctx *ctx)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemset(ctx->d_stats, 0, sizeof(unsigned long long) * PT_N_STATS_ALL));
    ctx->stats = pt_stats{};
    return PT_OK;
}

}  // extern "C"
