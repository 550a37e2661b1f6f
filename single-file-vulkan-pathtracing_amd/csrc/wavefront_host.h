// wavefront_host.h -- the host-side pieces of pt_render and how they fit together (one translation unit each):
//
//   extend_launch.hip   which closest-hit kernel walks a scene and with what launch shape (ExtendPlan), and its launch
//   shade_kernels.hip   k_generate / k_shade / k_shadow_add / k_resolve / k_hits_to_api and their launchers
//   extend_hbm.hip      the closest-hit kernels that walk a scene out of L2 / MALL / HBM (their own instruction scheduler)
//   fused.hip           PT_PIPELINE_FUSED: k_fused (fused_kernel.h), its plan and its launcher
//   aov.hip             pt_render_aov: the guide buffers' kernels, plan and launch
//   adaptive.hip        pt_render_adaptive: the selection of the tiles a render runs over, and the resolve that blends by a pixel's own count
//   trace_device.hip    pt_trace_device: rays in device memory packed into the queues, the extend launch per chunk, hit records into the caller's arrays
//   trace_fused.hip     ... its single-kernel form (PT_TRACE_FUSED): k_trace_fused, its plan and its launch
//   nearest.hip         pt_nearest_device: k_nearest (closest point on the mesh for device points), its plan and its launch
//   crossings.hip       pt_crossings_device: k_crossings (crossing counts and winding for device rays), its plan and its launch
//   film_work.hip       the film's workspace: how many slots a render gets (RenderShape) and the buffers behind them
//   render.hip          pt_render / _prepare / _adaptive / _guided / pt_trace: one CallPlan (pipeline resolved, kernels planned once) and one Job per call;
//                       wavefront: batches, pipelines on streams, rounds, polls; fused: shape, launches; shared: redo, selection, radiance record, timed tail
//
// Kernels are launched from the translation unit that defines them, so each unit exports small launchers; what crosses
// the units is plain data (wavefront_types.h) and the structs below.  Inside a unit every kernel family has ONE picker
// (pick_*: the plan's switches -> a typed kernel pointer) that its plan prepares through ptw_prepare_kernel and its launcher
// launches, so the two cannot disagree about which instantiation runs.
#pragma once
#include "wavefront_types.h"

#include <hip/hip_ext.h>

#include <algorithm>

// ---- what every plan of the launch path does, once each (extend_launch.hip, extend_hbm.hip, fused.hip, aov.hip) -------------------
// The context's stack-spill area holds at least `bytes` afterwards (it only grows).
inline pt_status ptw_reserve_spill(pt_ctx *ctx, size_t bytes)
{
    if (bytes <= ctx->spill_bytes) return PT_OK;
    (void)hipFree(ctx->d_spill);
    ctx->d_spill = nullptr;
    ctx->spill_bytes = 0;
    PT_HIP(ctx, hipMalloc((void **)&ctx->d_spill, bytes));
    ctx->spill_bytes = bytes;
    return PT_OK;
}
// Makes kernel `fn` launchable with `smem` bytes of dynamic LDS (above 48 KB a kernel needs the attribute: one set on its sibling
// does not count, so a plan passes EVERY kernel its picker can return for the launch shape through here) and, where per_cu is
// given, asks how many blocks of `block` threads a CU holds of it: 1 .. 8.
inline pt_status ptw_prepare_kernel(pt_ctx *ctx, const void *fn, int block, size_t smem, int *per_cu = nullptr)
{
    if (smem > 48 * 1024) PT_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    if (!per_cu) return PT_OK;
    PT_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, fn, block, smem));
    *per_cu = std::max(1, std::min(*per_cu, 8));
    return PT_OK;
}
// ... and pt_tuning.extend_blocks on top: fewer resident blocks than fit, never more
inline int ptw_tuned_blocks(const pt_ctx *ctx, int per_cu) { return pt_tuned(ctx->tune.extend_blocks, per_cu, 1, per_cu); }

// ---- extend_launch.hip ---------------------------------------------------------------------------------------------
struct ExtendPlan {
    uint32_t variant = PT_EXTEND_LDS;  // PT_EXTEND_LDS / _HBM / _HBM8 that will run
    bool lds_scene = false;
    size_t smem = 0;
    int grid = 0;
    uint32_t spill_levels = 0;
    int refill = 16;
    int lds_stack = 8;          // stack entries per lane kept in LDS (single-level kernel)
    bool spill = true;          // false: the scene's exact stack bound fits lds_stack, kernel without spill path
                                // (and with one-dword stack entries: COMPACT in k_extend)
    bool pairs = false;         // ... and every leaf of the BVH4 is one triangle or one fan pair: the PAIRS kernel
    bool waves7 = false;        // 8-wide kernel: the 72-VGPR instantiation, 7 blocks per CU (scenes beyond the Infinity Cache)
    bool bvh8 = false;          // PT_EXTEND_HBM8: the 8-wide tree and ITS triangle order (s->d_tri4_8, d_shade64_8, d_ke4_8)
    bool topdown4 = false;      // HBM variant over the top-down BVH4 with contiguous children (s->d_wide16t)
    uint32_t n_tlas_lds = 0;    // k_extend_inst16: TLAS nodes staged in LDS (its top levels)
    bool inst16 = false;        // two-level scenes: k_extend_inst16 (64-B fp16 nodes on both levels, one-dword stack entries)
    size_t smem_inst_fallback = 0; int grid_inst_fallback = 0;  // k_extend_inst's launch shape (tmin <= 0 takes it)
    size_t smem_wide_entries = 0;  // LDS bytes of the same plan run by the 8-byte-entry kernel (negative tmin)
};
// Picks the kernel (`want`: PT_EXTEND_*, AUTO by scene size), sizes its launch and the context's stack-spill area; builds the
// 8-wide nodes of a big scene on first use; repairs a scene whose last rebuild failed.
pt_status ptw_plan_extend(pt_scene *s, uint32_t want, ExtendPlan &pl);
// One closest-hit launch over the rays [0, *count_in) of a queue.  ev0 / ev1 (nullable): the kernel's own start / stop
// events; perm: ray order of ray_sort.hip; ray_tmax: per-ray bound = the any-hit form for shadow rays.
void ptw_launch_extend(const ExtendPlan &pl, pt_scene *s, const float4 *rayA, const float2 *rayB, float4 *hit, uint32_t *hit_inst,
                       const uint32_t *count_in, uint32_t *count_zero, unsigned long long *stats, float tmin, float tmax, bool count,
                       bool raw_hit, hipStream_t st, int pipe = 0, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                       const uint32_t *perm = nullptr, const float *ray_tmax = nullptr);

// ---- trace_fused.hip (pt_trace_device with PT_TRACE_FUSED: one kernel from the caller's rows to the caller's records) --------------------
enum { PT_TF_HITS = 0, PT_TF_SURFACE = 1, PT_TF_ANY = 2 };  // the kinds of query: CLOSEST into d_hits alone | with surface planes | ANY
struct TraceFusedPlan {
    int kind = PT_TF_HITS;
    bool pairs = false;  // ExtendPlan::pairs
    size_t smem = 0;     // ExtendPlan::smem: the compact LDS kernel's image and stack
    int grid = 0, refill = 16;
};
// the caller's arrays of one launch, each at the launch's first ray.  hits: pt_hit rows (PT_TF_HITS: set; PT_TF_SURFACE: nullable, as is each
// plane); d_tmax (PT_TF_ANY): nullable
struct TraceFusedIO {
    const float *rays6, *d_tmax;
    void *hits;
    uint8_t *occluded;
    float *position, *normal, *albedo, *emission;
};
// for a plan of the compact LDS class (pl.lds_scene && !pl.spill; the caller has checked tmin > 0): the grid from the kernel's own occupancy
pt_status ptw_plan_trace_fused(pt_scene *s, const ExtendPlan &pl, int kind, TraceFusedPlan &tp);
// n <= 2^30 rays (the row index inside a launch is 32 bits); ev0 / ev1 (nullable): the kernel's own start / stop events
void ptw_launch_trace_fused(const TraceFusedPlan &tp, const pt_scene *s, const TraceFusedIO &io, uint32_t n, float tmin, float tmax, hipStream_t st,
                            hipEvent_t ev0, hipEvent_t ev1);

// ---- shade_kernels.hip -----------------------------------------------------------------------------------------------
// everything a k_shade launch takes; `in` / `out` / the counts change from round to round, the rest per batch
struct ShadeLaunch {
    ptw::RenderConst rc;
    const uint32_t *tiles = nullptr;
    const pt_scene *scene = nullptr;   // per-triangle tables (LDS-sized or the 64-B records), instances
    bool bvh8 = false;                 // ... in the 8-wide tree's triangle order
    bool lds_tables = false, nee = false;
    int grid = 0;
    size_t smem = 0;
    ptw::Radiance rad{};
    const float4 *hit = nullptr;
    const uint32_t *hit_inst = nullptr;
    ptw::QueueView in{}, out{};
    const uint32_t *count_in = nullptr;
    uint32_t *count_out = nullptr;
    const float4 *inst_frame = nullptr;  // world-space normal + tangent per (instance, triangle), or null
    const float4 *lights = nullptr;      // NEE
    uint32_t n_lights = 0;
    float light_area = 0.f;
    ptw::ShadowQueue sq{};
    uint32_t *sq_count = nullptr;
};
void ptw_launch_shade(const ShadeLaunch &a, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// What every caller of k_shade decides the same way (render.hip job_setup, radiance_device.hip), once each:
// the launch shape -- 2 paths per thread (one queue-tail atomic per 512 paths), 8 blocks per CU (flat between 4 and 16); the per-triangle tables of
// small scenes are staged in LDS (tri4 + shade4 + the tangent frames, in the BVH4's order)
inline void ptw_shade_shape(const pt_ctx *ctx, const pt_scene *s, const ExtendPlan &pl, int &grid, size_t &smem, bool &lds_tables)
{
    grid = ctx->num_cus * 8;
    smem = sizeof(float4) * 8 * (size_t)s->n_tris;
    lds_tables = smem <= 16 * 1024 && !pl.bvh8;
}
// ... instanced scenes: world-space normal + tangent per (instance, triangle), built once (lbvh_build.hip); pt_tuning.inst_frames = 0 keeps the
// per-hit transform (-> null)
inline pt_status ptw_shade_inst_frames(pt_scene *s, const ExtendPlan &pl, const float4 *&inst_frame)
{
    inst_frame = nullptr;
    if (!(s->n_inst && !pl.bvh8 && s->ctx->tune.inst_frames != 0)) return PT_OK;
    PT_TRY(ptb_ensure_inst_frames(s));
    inst_frame = s->d_inst_frame;
    return PT_OK;
}
// ... the emitters the NEE estimator samples: the scene's, or -- instanced -- every instance's copy of them in world space (built on first NEE use)
inline pt_status ptw_nee_lights(pt_scene *s, bool nee, const float4 *&lights, uint32_t &n_lights, float &light_area)
{
    if (nee && s->n_inst) PT_TRY(ptb_ensure_inst_lights(s));
    lights = s->n_inst ? s->d_lights_inst : s->d_lights;
    n_lights = s->n_inst ? s->n_lights_inst : s->n_lights;
    light_area = s->n_inst ? s->light_area_inst : s->light_area;
    return PT_OK;
}
// (stats: the context's counters -- k_generate counts the camera rays of the slots it finishes without a walk, RenderConst::cull)
void ptw_launch_generate(const ptw::RenderConst &rc, const uint32_t *tiles, uint32_t slot_base, uint32_t n_slots, const ptw::Radiance &rad,
                         const ptw::QueueView &out, uint32_t *count_out, unsigned long long *stats, int num_cus, hipStream_t st);
void ptw_launch_shadow_add(const ptw::RenderConst &rc, const ptw::Radiance &rad, const float4 *sq_hit, const float4 *contrib,
                           const uint32_t *slot, const uint32_t *count, int grid, hipStream_t st);
// (skip_if_set: a device word; the kernel leaves the film alone when it is non-zero -- the fused pipeline's overflow flag, read by the host afterwards)
void ptw_launch_resolve(const ptw::RenderConst &rc, const uint32_t *tiles, const ptw::Radiance &rad, float *film, uint8_t *bgra, hipStream_t st,
                        const unsigned long long *skip_if_set = nullptr, float *m2 = nullptr);  // m2: the film's second-moment plane, if it has one
void ptw_launch_hits_to_api(const float4 *hit, const float4 *tri4, const uint32_t *hit_inst, const uint32_t *inst_id, uint32_t n, pt_hit *out,
                            hipStream_t st);

// ---- the tile list a render runs over ------------------------------------------------------------------------------------------
// Every kernel finds its pixels through a list of 8x8 tiles (wavefront_types.h slot_pixel) and does not care which tiles are listed: pt_render
// runs over the film's own (rank, world) list, pt_render_adaptive over a selection of it.
struct TileView {
    const uint32_t *d_tiles = nullptr;  // tile x | tile y << 16
    uint32_t n_tiles = 0;
    uint64_t pixels = 0;                // pixels of them inside the image (what pt_stats.paths counts)
    float *counts = nullptr;            // a selection: the film's plane K, which its resolve blends by and advances (adaptive.hip)
};
// What pt_render_adaptive hands down to the pipeline that serves it: the pipeline plans its work as for pt_render, then -- its tile list in its
// final order, nothing traced yet -- has the selection made (ptad_select) and renders that.
struct AdaptCall {
    const pt_adaptive_params *ap = nullptr;
    pt_adaptive_result res{};
    bool dry = false;                   // frame_count == 0: select, render nothing
};
// the list a launch uses: the selection, or the film's own as it stands now (a workspace grow or another hand-out order rebuilds it)
inline TileView ptw_tile_view(const pt_film *f, const TileView *sel)
{
    if (sel) return *sel;
    return { f->work.d_tiles, f->work.n_tiles, 0, nullptr };
}

// ---- adaptive.hip ------------------------------------------------------------------------------------------------------------------
// The selection of pt_render_adaptive over the list `src`: the selected tile words compacted in src's order into the film's scratch (-> *out),
// the record read back once (-> *res: tiles_total, tiles_selected, pixels_selected, max_error, select_ms).  Blocking.
pt_status ptad_select(pt_film *f, const pt_adaptive_params *ap, const TileView &src, TileView *out, pt_adaptive_result *res);
// k_resolve_adapt: ptw_launch_resolve with the blend by the pixel's own count (the film has M and K)
void ptw_launch_resolve_adapt(const ptw::RenderConst &rc, const uint32_t *tiles, const ptw::Radiance &rad, float *film, uint8_t *bgra, hipStream_t st,
                              const unsigned long long *skip_if_set, float *m2, float *counts);

constexpr size_t PTW_COUNT_WORDS = 16 * 32;  // pt_film::Work::d_count: the wavefront's queue sizes (2 per pipeline) | eight slot counters of the fused kernel, one 128-B line each (sixteen with head + tail slots)

// ---- fused.hip ---------------------------------------------------------------------------------------------------------
struct FusedPlan {
    size_t smem = 0;
    int grid = 0, block = 0, lds_stack = 0, refill = 40;
    bool pairs = true;                   // single-level: the pair-leaf instantiation (ExtendPlan::pairs)
    bool count = false;                  // PT_FLAG_COUNT_VISITS: the instrumented twin (single-level scenes; wave-level block counts)
    bool nee = false;                    // PT_FLAG_NEE: k_fused_nee (single-level scenes, one sample group; its own LDS plan and occupancy)
    bool inst = false;                   // two-level scene: k_fused_inst (fused_inst_kernel.h) around k_extend_inst16's walk
    uint32_t n_tlas_lds = 0;             // ... its TLAS nodes staged in LDS
    uint32_t *spill = nullptr;           // ... its stack entries beyond lds_stack: [levels][grid * block] dwords of the context's spill area
    const float4 *inst_frame = nullptr;  // ... the (instance, triangle) normal + tangent table, or null
    int enter_min = 12, leaf_min = 14, node_yield = 6;  // ... the waiting rules of its walk (fused.hip plan_fused_inst)
};
pt_status ptw_plan_fused(pt_scene *s, const ExtendPlan &pl, float tmin, FusedPlan &fp, bool nee = false);
// mode: 0 one sample group, 1 several, 2 head + tail slots; div_frames: by rc.lanes_active, chunk -> (tile, frame) of one group's hand-out order (fused_kernel.h)
void ptw_launch_fused(const FusedPlan &fp, int mode, const ptw::FastDiv &div_frames, const ptw::RenderConst &rc, const uint32_t *tiles, const ptw::Radiance &rad,
                      const pt_scene *s, uint32_t n_slots, uint32_t *next_slot, unsigned long long *stats, float tmin, float tmax,
                      hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// fused_guided.hip: the same launch by the kernels that also write the first-hit log (pt_render_guided; guided_kernel.h has the log's layout)
pt_status ptw_launch_fused_log(const FusedPlan &fp, int mode, const ptw::FastDiv &div_frames, const ptw::RenderConst &rc, const uint32_t *tiles, const ptw::Radiance &rad, const pt_scene *s,
                               uint32_t n_slots, uint32_t *next_slot, unsigned long long *stats, float tmin, float tmax, uint2 *log, hipStream_t st);
// fused_rays.hip: the single-level kernels started from a caller's rays (pt_radiance_device with PT_RADIANCE_FUSED; fused_kernel.h RAYS).  rc.n_slots: the
// chunk's live slots, m * spp, sample-major; rays6 / seeds: the chunk's rows; index0, seed_m0: radiance_device_kernel.h RdRays.  next_slot: eight
// zeroed counters, PT_FUSED_PART_STRIDE dwords apart
pt_status ptw_launch_fused_rays(const FusedPlan &fp, const ptw::RenderConst &rc, const ptw::Radiance &rad, const pt_scene *s, uint32_t *next_slot, unsigned long long *stats,
                                float tmin, float tmax, const float *rays6, const uint32_t *seeds, uint32_t m, uint32_t spp, uint32_t index0, uint32_t seed_m0,
                                hipStream_t st);
constexpr size_t PTW_FUSED_COUNT_BYTES = 8 * 32 * sizeof(uint32_t);  // ... in bytes (fused_kernel.h PT_FUSED_PARTS x PT_FUSED_PART_STRIDE dwords)
// guided.hip: the records of the launch's frames folded into the film's guide planes (id_frame: the frame of the launch that is the call's last, or
// >= rc.lanes_active); inst_frame: FusedPlan::inst_frame
void ptg_launch_reduce(const pt_scene *s, pt_film *f, const ptw::RenderConst &rc, const uint32_t *tiles, uint32_t id_frame, const float4 *inst_frame, hipStream_t st);
// What pt_render_guided hands down to the fused pipeline (render.hip Job::gd): every launch writes the film's log and is followed by the reduce.
struct GuidedCall {
    uint32_t launches = 0;              // fused launches of the call
    float guide_ms = 0.f;               // device time of the reduce launches
};

// ---- film_work.hip -----------------------------------------------------------------------------------------------------
struct RenderShape {
    uint32_t lanes = 1, groups = 1, group_size = 1, term_cap = 0, term_pcap = 0;
    bool bounded = false;  // term_cap < group_size * max_depth: a full log is detected and the batch redone ungrouped
    uint32_t tail = 0;     // fused pipeline: one-sample tail slots per (frame, pixel) behind a head slot of spp - tail samples (groups == 1 then)
};
// launch_class: 0 instanced scenes, 1 scenes walked out of L2 / MALL / HBM, 2 single-level scenes in LDS, 3 the fused pipeline
RenderShape ptw_choose_shape(const pt_film *f, const pt_params *p, int launch_class, int shrink = 0);
pt_status ptw_ensure_work(pt_film *f, uint32_t rank, uint32_t world, uint32_t lanes, uint32_t groups, uint32_t term_cap, uint32_t term_pcap,
                          bool queues = true, uint32_t tail = 0);
pt_status ptw_shape_and_work(pt_film *f, const pt_params *p, RenderShape &sh, int launch_class, bool queues = true);
pt_status ptw_tiles_subject_first(pt_film *f, const int32_t rect[4], hipStream_t st);  // fused pipeline: tiles that can see the scene first (film_work.hip)
uint64_t ptw_workspace_bytes(const pt_film *f);
ptm::Camera ptw_camera(const pt_params *p);  // the camera of a launch: pt_render and pt_render_aov start the same rays from it
// ... of a film pass (reproject.hip, motion.hip), which is given a camera and a film and no pt_params
inline ptm::Camera ptw_camera_of(const float *origin, const float *target, uint32_t w, uint32_t h)
{
    pt_params cp{};
    for (int k = 0; k < 3; k++) { cp.cam_origin[k] = origin[k]; cp.cam_target[k] = target[k]; }
    cp.width = w; cp.height = h;
    return ptw_camera(&cp);
}
// (n_tiles: of the list the render runs over -- the slot numbering follows from it, the buffers are the full list's)
ptw::RenderConst ptw_render_const(const pt_params *p, uint32_t n_tiles, const RenderShape &sh);
uint64_t ptw_valid_local_pixels(const pt_film *f, const pt_params *p);
// render.hip: the pixel rectangle {x0, y0, x1, y1} outside of which no camera ray can reach the scene's box (x1 < x0: no such proof)
void ptw_subject_rect(const pt_scene *s, const pt_params *p, int32_t rect[4]);

// ---- extend_hbm.hip / ray_sort.hip (launchers of the kernels compiled with the max-ILP scheduler; the ray sorter) --------
const void *ptw_extend_hbm_fn(bool count, bool rec64);
void ptw_launch_extend_hbm(bool count, bool rec64, int grid, size_t smem, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1,
                           const float4 *wide, const uint2 *wide16, const float *norm_c, const float *norm_s,
                           const float *norm_rs, const float4 *tri4, const float4 *rec64_tab, uint32_t n_wide, uint32_t n_tris,
                           const float4 *rayA, const float2 *rayB, float4 *hit, const uint32_t *count_in, uint32_t *count_zero,
                           unsigned long long *stats, uint2 *spill, uint32_t spill_stride, int refill, float tmin,
                           float tmax, int lds_stack, int raw_hit, const uint32_t *perm, const float *ray_tmax);
const void *ptw_extend8_fn(bool count, bool spills, bool waves7);
void ptw_launch_extend8(bool count, bool spills, bool waves7, int grid, size_t smem, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, const uint4 *nodes8,
                        const float *norm_c, const float *norm_s, const float *norm_rs, const float4 *tri4, const float4 *rec64, const float4 *rayA,
                        const float2 *rayB, float4 *hit, const uint32_t *count_in, uint32_t *count_zero, unsigned long long *stats,
                        uint2 *spill, uint32_t spill_stride, int refill, float tmin, float tmax, int lds_stack, int raw_hit,
                        const uint32_t *perm, const float *ray_tmax);
size_t ptw_ray_sort_bytes(size_t cap);
const uint32_t *ptw_sort_rays(hipStream_t st, const float4 *rayA, const float2 *rayB, const uint32_t *count, size_t cap,
                              const float *bmin, const float *bmax, int bits, int num_cus, void *scratch);
