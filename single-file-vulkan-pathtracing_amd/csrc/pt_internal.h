// pt_internal.h -- host-side objects behind the opaque C-ABI handles, and the HBM data layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/pt_api.h"

// ---- HBM layout of a scene --------------------------------------------
// All per-triangle arrays are in LBVH leaf order (sorted Morton position), so neighbouring
// leaves are neighbouring memory.
//   tri4   : 3 x float4 per triangle  {v0.xyz, bits(prim id)} {v1.xyz, 0} {v2.xyz, 0}       48 B
//   shade4 : 3 x float4 per triangle  {n.xyz, brdf.r} {brdf.gb, emission.rg} {emission.b,0,0,0} 48 B
//   nodes  : binary LBVH, 4 x float4 per internal node {lmin.xyz,lmax.x} {lmax.yz,rmin.xy}
//            {rmin.z,rmax.xyz} {bits(left), bits(right), 0, 0}; child bit31 = leaf position       64 B
//   wide16 : the same BVH4 with fp16 boxes, 16 dwords per node: lo.x[4] lo.y[4] lo.z[4] hi.x[4] hi.y[4] hi.z[4]
//            as halves (2 dwords each), child[4]                                                      64 B
//   wide   : BVH4 collapsed from it, 8 x float4 per node: lo.x[4] lo.y[4] lo.z[4] hi.x[4] hi.y[4]
//            hi.z[4] child[4] spare; leaf child = LEAF | (count-1)<<28 | first sorted position     128 B
constexpr int PT_N_STATS = 24;  // u64 slots of pt_ctx::d_stats that pt_get_stats reads ...
constexpr int PT_N_BLOCKS = 32;  // ... followed by {wave executions, lanes} of up to this many kernel blocks (pt_get_block_counts; fused_kernel.h FusedBlock)
constexpr int PT_N_STATS_ALL = PT_N_STATS + 2 * PT_N_BLOCKS;
// The u64 words of pt_ctx::d_stats below PT_N_STATS (1 and 21 .. 23 are unused): the kernels add to them, pt_get_stats reads them
enum pt_stat_word : int {
    PT_STAT_RAYS = 0, PT_STAT_RAYS_CULLED = 19,        // the exact ray count; of it, camera rays of slots finished without a walk (pt_stats.rays_culled)
    PT_STAT_NODES = 2, PT_STAT_TRIS = 3,               // PT_FLAG_COUNT_VISITS: BVH nodes visited, triangles tested ...
    PT_STAT_NODE_STEPS = 4, PT_STAT_TRI_STEPS = 5,     // ... wave steps of the node code, of the triangle code
    PT_STAT_OVERFLOW = 6, PT_STAT_SPILL_FILL = 7,      // a slot filled its term log (the launch is redone: render.hip); entries taken from the term spill pool
    PT_STAT_WAVE_REFILLS = 8, PT_STAT_WAVE_POPS = 9, PT_STAT_WAVE_HIT_BLOCKS = 10, PT_STAT_WAVE_FINISHES = 11, PT_STAT_WAVE_ITERS = 12,  // wave executions
    PT_STAT_LEAF_LANES = 13, PT_STAT_POP_LANES = 14, PT_STAT_HIT_LANES = 15,  // lanes in leaf steps, pop iterations, divide blocks
    PT_STAT_ENTER_STEPS = 16, PT_STAT_ENTER_LANES = 17,                       // wave executions of the instance entry, lanes in them
    PT_STAT_RAYS_SAVED = 18, PT_STAT_RAYS_CULLED_SAVED = 20  // the two ray counters as they were before a launch whose term logs may overflow
};
constexpr int PT_MAX_PIPES = 4;  // concurrent wavefront pipelines (streams) per pt_render
namespace {
constexpr int TB = 256;                     // threads per block of every kernel of the library
constexpr uint32_t SENTINEL = 0xFFFFFFFFu;  // "no child" / "no node" in the BVH4 child words
}  // namespace

struct pt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    std::string err;
    unsigned long long *d_stats = nullptr;  // the counters in device memory: PT_N_STATS_ALL u64 words, named by pt_stat_word above
    void *d_rad = nullptr;                 // ptw::Radiance of the fused launch in device memory (wavefront_types.h: Radiance::dev) ...
    unsigned char h_rad[128] = {};         // ... and what it holds (uploaded when it changes: the film's buffers only move when they grow)
    pt_stats stats{};
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    hipStream_t pipe_stream[PT_MAX_PIPES] = {};  // extra pipelines of pt_render ([0] unused: that is `stream`)
    hipEvent_t ev_fork = nullptr, ev_join[PT_MAX_PIPES] = {};
    // live-count polls of the round loop (render.hip): per pipeline two pinned words and two events, used alternately,
    // so the host reads the count of eight rounds ago while the stream still holds eight rounds of work
    uint32_t *h_poll = nullptr;                      // [PT_MAX_PIPES][2], hipHostMalloc
    hipEvent_t ev_poll[PT_MAX_PIPES][2] = {};
    hipEvent_t ev_shade[PT_MAX_PIPES] = {};          // end of each pipeline's most recent shade launch (the shade rule of three pipelines)
    std::vector<hipEvent_t> ev_pool;  // PT_FLAG_PROFILE start/stop events, reused across pt_render calls
    void *d_spill = nullptr;   // HBM overflow of the traversal short stack: [level][thread] uint2
    size_t spill_bytes = 0;
    // Upper bound on the workspace of a film (0 = what hipMemGetInfo reports as free).  pt_tuning.mem_budget_mb / the environment variable
    // PT_MEM_BUDGET_MB at pt_ctx_create; left alone (-1) the library plans within PT_DEFAULT_MEM_BUDGET_MB: a scene of 400 MB should not
    // take 25 GB of the device without being asked (what each GB buys: profiles/r06e_mem_budget.log).
    size_t mem_budget = 0;
    pt_tuning tune;            // include/pt_api.h: defaults (-1) + PT_TUNE, filled once by pt_ctx_create
    // fused.hip: the launch attributes / occupancy of the fused kernels for the last LDS size planned ([0] single-level, [1] two-level,
    // [2] single-level with NEE).  A call plans its fused launch once (render.hip CallPlan); this is for the calls that follow it: a blocking
    // call per frame should not pay seven runtime calls for the same plan every time
    size_t fused_smem[3] = { 0, 0, 0 };  // key: LDS bytes << 1 | pair-leaf kernel
    int fused_per_cu[3] = { 0, 0, 0 };
    // pt_trace_device (trace_device.hip): one chunk of rays in the extend kernels' queue layout, their hit records and the any-hit kernels' bound
    // plane.  The context's scratch, made by the first call; it only grows, counts against mem_budget and is freed by pt_ctx_destroy.
    struct Trace {
        float4 *d_rayA = nullptr; float2 *d_rayB = nullptr;        // {origin.xyz, direction.x} {direction.y, direction.z}
        float4 *d_hit = nullptr; uint32_t *d_hit_inst = nullptr;   // {bits(pos), t, u, v}; the instance's TLAS leaf position
        float *d_bound = nullptr;                                  // PT_TRACE_ANY: ray_tmax
        uint32_t *d_count = nullptr;                               // [2]: the chunk's ray count (what the extend kernels read), a spare word
        size_t cap = 0;                                            // rays the per-ray arrays hold
        size_t bytes = 0;                                          // device bytes of all of the above
    } tr;
    // pt_radiance_device (radiance_device.hip): one chunk of path slots -- the two path queues of the wavefront kernels, the hit records, one
    // accumulator per slot -- and, from the first PT_RADIANCE_NEE call on, the shadow queue.  The context's scratch like `tr`: made by the first
    // call, only growing, counted against mem_budget, freed by pt_ctx_destroy.
    struct Radiance {
        uint2 *d_qid[2] = { nullptr, nullptr }; float4 *d_qstate[2] = { nullptr, nullptr };   // {slot, sample | depth << 16} {seed, weight}
        float4 *d_qrayA[2] = { nullptr, nullptr }; float2 *d_qrayB[2] = { nullptr, nullptr };
        float4 *d_hit = nullptr; uint32_t *d_hit_inst = nullptr;
        float4 *d_color = nullptr;                                 // a slot's accumulator (ptw::Radiance::color)
        uint32_t *d_count = nullptr;                               // [4]: the two queues' sizes, the shadow queue's, a spare word
        uint32_t *d_tiles = nullptr;                               // [1]: the zeroed tile word k_shade's slot_pixel reads
        float4 *d_sq_rayA = nullptr; float2 *d_sq_rayB = nullptr; float4 *d_sq_contrib = nullptr; float4 *d_sq_hit = nullptr;
        float *d_sq_tmax = nullptr; uint32_t *d_sq_slot = nullptr;
        size_t cap = 0, cap_sq = 0;                                // slots the per-slot arrays / the shadow queue hold
        size_t bytes = 0, sq_bytes = 0;                            // device bytes of the two sets
        // PT_RADIANCE_FUSED: a set of its own -- the accumulators k_radiance_resolve reads and the fused kernel's eight slot counters.  A context
        // that only ever runs the single-kernel form holds nothing else
        float4 *d_fcolor = nullptr;
        uint32_t *d_fcount = nullptr;                              // PTW_FUSED_COUNT_BYTES
        size_t cap_f = 0, f_bytes = 0;
    } rd;
};
// The workspace budget a context plans within when the caller names none: 8 GB.  Round 6, one MI355X, Grays/s at 2 / 4 / 8 / 16 / 32 GB / no
// bound: the 10 000-instance grid through the queues 13.6 / 15.0 / 15.0 / 15.1 / 15.4 / 15.3 (the fused kernel 15.5 in 0.6 GB at every budget);
// the 1 M-triangle soup 2.30 / 2.30 / 3.10 / 3.31 / 3.44 / 3.43; the 8 M-triangle soup 1.89 / 2.96 / 3.18 / 3.29 / 3.27 / 3.28
// (profiles/r06e_mem_budget.log).  A caller who wants the last 3 .. 10 % on big scenes says so (mem_budget_mb = 32768, or 0 for no bound).
constexpr int PT_DEFAULT_MEM_BUDGET_MB = 8192;
inline size_t pt_budget_bytes(int32_t mb) { return mb > 0 ? (size_t)mb << 20 : mb == 0 ? 0 : (size_t)PT_DEFAULT_MEM_BUDGET_MB << 20; }
// a tuning field with its built-in choice and its valid range
inline int pt_tuned(int32_t v, int dflt, int lo, int hi) { return v < 0 ? dflt : (v < lo ? lo : (v > hi ? hi : v)); }

struct pt_scene {
    pt_ctx *ctx = nullptr;
    uint32_t n_tris = 0, n_nodes = 0, height = 0;   // height: of the binary LBVH (read-back)
    uint32_t height_tree = 0;                       // height of the binary tree the traversed BVH4 was collapsed from (LBVH or PLOC)
    float bmin[3]{}, bmax[3]{};
    float build_ms = 0.f;
    float4 *d_tri4 = nullptr;
    float4 *d_shade4 = nullptr;
    float4 *d_shade64 = nullptr;  // 4 x float4 per leaf position {v0, n.x} {v1, n.y} {v2, n.z} {brdf, emits ? 1 : 0}: what k_shade gathers when the tables are not in LDS
    float4 *d_ke4 = nullptr;      // float4 per leaf position {Ke, 0}: read for emitters only
    float4 *d_frame4 = nullptr;   // 2 x float4 per leaf position {T.xyz, B.x} {B.yz, 0, 0}: the tangent frame of the normal (raygen.rgen:14-21), for k_shade's LDS tables
    float4 *d_nodes = nullptr;            // binary LBVH (parity read-back; the collapse reads it)
    float4 *d_wide = nullptr;             // BVH4, 8 x float4 = 128 B per node: what traversal walks
    uint32_t n_wide = 0;
    uint32_t stack_need = 0xFFFFFFFFu;    // exact bound of pending traversal-stack entries (small scenes), else unknown
    // BVH quality (main.cpp:419 asks the driver for ePreferFastTrace).  d_wide / n_wide / stack_need above and
    // the order of tri4/shade4 describe the BVH4 that is TRAVERSED: the collapsed LBVH (builder 0) or, for
    // scenes of <= PT_SAH_MAX_TRIS triangles, a surface-area sweep built on the device (builder 1, bvh4_sah_device.hip).
    // d_wide aliases one of the two owned arrays below.
    uint32_t bvh4_builder = 0;            // 0 collapsed LBVH, 1 surface-area sweep (small scenes), 2 PLOC rebuild of the binary tree (big scenes)
    uint32_t quality = 0;                 // pt_bvh_quality the products were built for
    bool broken = false;                  // a rebuild of the tree products failed (lbvh_build.hip build_tree_products): nothing to traverse
    double area_lbvh = 0.0, area_ploc = 0.0;  // big scenes: sum of the internal nodes' surface areas of the two binary trees (0 = not built)
    // 64-B copy of the traversed BVH4 for scenes that are walked in HBM/L2 (lbvh_build.hip make_wide16):
    // boxes as fp16 of coordinates normalised to the scene box, rounded outwards; halves the bytes per node
    uint2 *d_wide16 = nullptr;
    float norm_c[3]{}, norm_s[3]{1.f, 1.f, 1.f}, norm_rs[3]{1.f, 1.f, 1.f};  // x' = (x - c) * rs,  s = 1/rs
    // BVH8 of the same LBVH for scenes walked out of L2 / MALL / HBM (lbvh_build.hip k_w8_*): 128-B nodes, and the
    // per-triangle tables in ITS triangle order (a node's leaf triangles are contiguous), used instead of
    // d_tri4 / d_shade64 / d_ke4 whenever the BVH8 kernel traverses
    uint4 *d_wide8 = nullptr;
    uint32_t n_wide8 = 0, levels8 = 0;
    // BVH4 in the 64-B format built top-down (area-guided collapse, the children of a node contiguous): what
    // k_extend<hbm> walks for scenes whose traversed BVH4 is the collapsed LBVH (lbvh_build.hip k_w4_emit)
    uint4 *d_wide16t = nullptr;
    uint32_t n_wide16t = 0, levels4t = 0;
    uint32_t *d_prim_of8 = nullptr;
    float4 *d_tri4_8 = nullptr, *d_shade64_8 = nullptr, *d_ke4_8 = nullptr;
    uint64_t device_bytes8 = 0;
    float4 *d_wide_lbvh = nullptr; uint32_t n_wide_lbvh = 0, stack_need_lbvh = 0xFFFFFFFFu;
    float4 *d_wide_sah = nullptr;  uint32_t n_wide_sah = 0, stack_need_sah = 0xFFFFFFFFu;
    uint32_t *d_prim_of_sah = nullptr;      // leaf order of the SAH BVH4 (position -> prim id)
    float4 *d_tri_orig = nullptr;           // small scenes keep the unsorted triangles + materials so the
    float *d_faces = nullptr;               // per-triangle tables can be re-packed in another leaf order
    std::vector<float> h_tlo, h_thi;        // small scenes: unpadded triangle boxes (3 floats each)
    std::vector<uint8_t> h_pair;            // small scenes: [n] triangle i+1 = (v0, v2, v3) of the quad whose (v0, v1, v2) is triangle i
    bool sah_pair_leaves = false;           // ... of the surface-area BVH4 (d_wide_sah)
    bool pair_leaves = false;               // the traversed BVH4 has exactly one primitive (triangle or such a pair) per leaf
    unsigned long long *d_keys = nullptr;  // sorted Morton keys (kept for parity read-back)
    uint32_t *d_prim_of = nullptr;         // sorted position -> prim id
    uint64_t device_bytes = 0;
    // emitters (Ke != 0) in primitive order for PT_PIPELINE_WAVEFRONT_NEE: 5 float4 each {A, cdf} {B, 0} {C, 0} {N, 0} {Ke, 0}
    // (cdf = running float sum of the triangle areas, light_area its total)
    float4 *d_lights = nullptr;
    uint32_t n_lights = 0;
    float light_area = 0.f;
    std::vector<float4> h_lights;   // host copy of d_lights: instancing makes its world-space copies from it
    std::vector<uint32_t> h_light_prim;  // the primitive of each emitter (pt_scene_update recomputes the records from new vertices)
    uint32_t *d_light_prim = nullptr;    // ... on the device, for pt_scene_update_device (scene_device.hip; null until a device call needs it)
    // instanced scenes: every instance's emitters in world space, gl_InstanceID-major, same 5-float4 layout and running cdf
    std::vector<float> h_xforms;    // the instance set's object->world matrices as given (gl_InstanceID order): ptb_ensure_inst_lights
    // ... or, after pt_scene_set_instances_device, in device memory: 3 float4 per instance, gl_InstanceID order.  Exactly one of the two holds
    // the set (pt_given_instances); both survive parking (scene_build.hip restore_parked_instances).  xf_set counts the sets that succeeded.
    float4 *d_xforms = nullptr;
    uint32_t n_xforms_dev = 0;
    uint64_t xf_set = 0;
    float4 *d_lights_inst = nullptr;  // built on the first NEE render of the instance set
    uint32_t n_lights_inst = 0;
    float light_area_inst = 0.f;
    // two-level scenes: instances in TLAS leaf order, 6 float4 each {object->world rows, world->object rows}
    uint32_t n_inst = 0, n_tlas_wide = 0, tlas_height = 0;
    double tlas_area_lbvh = 0.0, tlas_area_ploc = 0.0;  // area sums of the TLAS's binary trees (ploc: 0 = not built)
    float4 *d_inst6 = nullptr;
    float4 *d_inst_frame = nullptr;  // [n_inst][n_tris][2]: world-space normal + tangent of every instanced triangle (ptb_ensure_inst_frames)
    float4 *d_tlas_wide = nullptr;        // BVH4 over the instances' world boxes
    uint32_t *d_tlas_prim_of = nullptr;   // sorted position -> instance id (gl_InstanceID)
    // the TLAS k_extend_inst16 walks: 64-B fp16 nodes (normalised to the TLAS box), built top-down, 16-bit child codes
    uint4 *d_tlas16 = nullptr;
    uint32_t n_tlas16 = 0, tlas16_levels = 0;
    float tlas_norm_c[3]{}, tlas_norm_s[3]{1.f, 1.f, 1.f}, tlas_norm_rs[3]{1.f, 1.f, 1.f};
    float tlas_bmin[3]{}, tlas_bmax[3]{};  // the union of the instances' world boxes (k_inst_boxes): what no ray outside of can hit
    // pt_scene_snapshot_previous (motion.hip): "the previous geometry" of pt_film_motion.  Nothing of it exists before the first call.
    struct Previous {
        bool have = false;
        float4 *d_tri = nullptr;   // a copy of d_tri_orig as it stood: 3 float4 per triangle in primitive order
        // [0, 3 n_inst): the instance matrices as they stood, 3 rows of float4 each in gl_InstanceID order; [3 n_inst, 6 n_inst): the place
        // pt_film_motion uploads the scene's current matrices to (the device holds those in TLAS leaf order only).  Null when n_inst == 0.
        float4 *d_xf = nullptr;
        uint32_t n_inst = 0;       // 0: single-level
        std::vector<float> h_now;  // what the second half of d_xf holds (empty: nothing yet): pt_film_motion uploads only when h_xforms differs
        uint64_t now_set = 0;      // ... after a device set: the pt_scene::xf_set it was copied at (0: not from a device set)
        uint64_t bytes = 0;        // device bytes of both: added to pt_scene_info.device_bytes
    } prev;
};
// the number of matrices the scene keeps as given -- on the host or on the device -- whether they are set (n_inst) or parked
inline size_t pt_given_instances(const pt_scene *s) { return s->d_xforms ? (size_t)s->n_xforms_dev : s->h_xforms.size() / 12; }

// An optional plane of a film (M, L, Q below): absent until its pt_film_enable_* call, then the film's own allocation or the caller's memory.
// pt_plane_enable / pt_plane_read / pt_planes_clear / pt_planes_free (film_work.hip) are all that allocate, zero, read back and free one.
struct pt_plane_any {
    void *d = nullptr;                                // null: the film has no such plane
    bool own = false;
};
template <class T> struct pt_plane : pt_plane_any {
    T *ptr() const { return static_cast<T *>(d); }
};

struct pt_film {
    pt_ctx *ctx = nullptr;
    uint32_t w = 0, h = 0;
    float *d_rgb = nullptr;   // w*h*3 running mean (canonical float film)
    bool own_rgb = true;
    uint8_t *d_bgra = nullptr;  // w*h*4 reference-display image
    // wavefront workspace, (re)allocated by pt_render for (rank, world, frames_in_flight)
    struct Work {
        uint32_t rank = 0, world = 0, lanes = 0;  // lanes = frames in flight
        uint32_t tile_order = 0;                  // 0: the rank's tiles row by row, 1: centre first (fused pipeline; film_work.hip)
        uint32_t groups = 0, term_cap = 0;        // sample groups per pixel, radiance-term log capacity per slot
        uint32_t tail = 0;                        // one-sample tail slots per (frame, pixel) of the last shape (fused head + tail form)
        uint32_t n_tiles = 0;                     // local 8x8 tiles
        uint32_t n_slots = 0;                     // lanes * n_tiles * 64
        uint32_t *d_tiles = nullptr;              // local tile -> global tile id
        std::vector<uint32_t> h_tiles;            // tile_order 1: the centre-first list as built (ptw_tiles_subject_first re-orders d_tiles from it)
        int32_t tile_rect[4] = { 0, 0, -1, -1 };  // ... the pixel rectangle {x0, y0, x1, y1} whose tiles currently go first in d_tiles (x1 < x0: none)
        float4 *d_color = nullptr;                // per slot: frame colour accumulator rgb + pad (groups == 1)
        float4 *d_terms = nullptr;                // per slot: ordered radiance terms, dense primary log   (groups > 1)
        float4 *d_terms_over = nullptr;           // per slot: overflow of the primary log (worst-case sized)
        uint32_t *d_nterm = nullptr;              // per slot: number of logged terms               (groups > 1)
        uint32_t *d_spill_head = nullptr;         // per slot: last entry of the slot in the spill pool (groups > 1)
        float4 *d_spill = nullptr;                // shared pool {r, g, b, previous entry of the slot}: terms beyond term_cap
        // double-buffered dense queues (index = queue position)
        uint2 *d_qid[2] = { nullptr, nullptr };       // {slot, sample | depth<<16}
        float4 *d_qstate[2] = { nullptr, nullptr };   // {bits(seed), weight.rgb}
        float4 *d_qrayA[2] = { nullptr, nullptr };    // {org.xyz, dir.x}
        float2 *d_qrayB[2] = { nullptr, nullptr };    // {dir.y, dir.z}
        float4 *d_hit = nullptr;                      // {bits(pos), t, u, v}
        uint32_t *d_hit_inst = nullptr;               // instance (TLAS sorted position); only for two-level scenes
        uint32_t *d_count = nullptr;                  // [2] queue sizes
        size_t cap_slots = 0, cap_meta = 0, cap_color = 0, cap_terms = 0, cap_terms_over = 0, cap_spill = 0;  // allocated capacities (buffers only grow); cap_slots: queues + hit records, cap_meta: d_nterm / d_spill_head
        size_t bytes = 0;                             // device bytes held by the buffers above
        // shadow queue of the NEE pipeline (one entry per hit whose light sample faces it)
        float4 *d_sq_rayA = nullptr; float2 *d_sq_rayB = nullptr; float4 *d_sq_contrib = nullptr;  // {r, g, b, tmax}
        uint32_t *d_sq_slot = nullptr; float *d_sq_tmax = nullptr; float4 *d_sq_hit = nullptr; uint32_t *d_sq_count = nullptr;
        size_t cap_sq = 0, sq_bytes = 0;              // (its bytes are counted here, not in `bytes`: no shape is planned against them)
        void *d_sort = nullptr;                       // ray_sort.hip scratch for all pipelines (ptw_ray_sort_bytes per slot range)
        size_t sort_bytes = 0;
    } work;
    // guide buffers (pt_film_enable_aov) and the scratch of pt_render_aov (aov.hip).  The scratch is the film's and only grows:
    // a second call of the same shape allocates nothing.
    struct Aov {
        bool enabled = false;
        void *plane[PT_AOV_COUNT] = {};               // dense, row-major: see the enum in include/pt_api.h
        bool own[PT_AOV_COUNT] = {};
        uint32_t rank = 0, world = 0, n_tiles = 0;    // the tile list below is this rank's, row by row
        uint64_t valid_pixels = 0;                    // ... and the pixels of it inside the image
        std::vector<uint64_t> h_valid;                // [n_tiles + 1] running count of those pixels over the tile list
        uint32_t *d_tiles = nullptr;                  // tile x | tile y << 16
        float4 *d_rayA = nullptr; float2 *d_rayB = nullptr;   // queue form: one chunk of camera rays in the extend kernels' layout,
        float4 *d_hit = nullptr; uint32_t *d_hit_inst = nullptr;  // ... and their hit records
        size_t cap_rays = 0;
        uint32_t *d_count = nullptr;                  // [0] rays of the chunk (what the extend kernels read), [32] next tile of the single-kernel form
        size_t bytes = 0;                             // device bytes of the scratch
    } aov;
    // pt_film_denoise (denoise.hip).  The scratch is the film's, allocated by the first call and kept: later calls allocate nothing
    // (the film-owned output comes with the first call that asks for it).
    struct Denoise {
        float4 *d_guide = nullptr;                    // per pixel {N.xyz, Z}
        float4 *d_illum[2] = { nullptr, nullptr };    // per pixel {I.rgb, 0}: the ping-pong planes of the iterations
        float *d_out = nullptr;                       // film-owned result, w*h*3 floats ...
        uint8_t *d_out_bgra = nullptr;                // ... and its bgra8 form
        bool have_out = false;                        // a denoise has written d_out / d_out_bgra
        size_t bytes = 0;                             // device bytes of all of the above
    } dn;
    // pt_film_upsample (upsample.hip): the film-owned result of the full-size film, made by the first call that asks for it and kept.
    struct Upsample {
        float *d_out = nullptr;                       // w*h*3 floats ...
        uint8_t *d_out_bgra = nullptr;                // ... and its bgra8 form
        bool have_out = false;                        // an upsample has written d_out / d_out_bgra
        size_t bytes = 0;                             // device bytes of both
    } up;
    // pt_film_enable_moments: the running mean of the squared frame colour, blended by the resolve kernel beside the film (shade_kernels.hip
    // k_resolve_m2).  A film plane like the guides, not a workspace.
    struct Moments : pt_plane<float> {                // w*h*3 floats
        uint32_t frames = 0;                          // frame + frame_count of the last pt_render: what the film and the plane average
    } m2;
    // pt_film_enable_history: the history length of pt_film_reproject (reproject.hip), in reprojection steps.  A film plane like M.
    pt_plane<float> hist;                             // w*h floats
    // pt_film_enable_motion: where the surface point of a pixel's first hit was in the previous geometry (motion.hip).  A film plane like L.
    pt_plane<float4> mo;                              // w*h float4 {x, y, z, valid}
    // pt_film_enable_counts: the frames each pixel holds, as pt_render_adaptive blends them (adaptive.hip).  A film plane like L.
    pt_plane<float> cnt;                              // w*h floats
    // pt_render_adaptive's selection (adaptive.hip): the film's scratch, made by the first call and kept; it grows with the rank's tile list.
    struct Adapt {
        uint32_t *d_sel = nullptr;                    // the selected tile words, in the source list's order
        uint32_t *d_off = nullptr;                    // [cap + 1] a flag per tile of the source list, then its exclusive scan
        uint32_t *d_err = nullptr;                    // a word per tile: the bits of its e_T (0 for a short tile)
        uint32_t *d_sums = nullptr;                   // the scan's block sums (device_scan.h)
        void *d_rec = nullptr;                        // the record the host reads once per call: count, max error, pixels
        size_t cap = 0;                               // tiles the arrays hold
        size_t bytes = 0;                             // device bytes of all of the above
    } ad;
    // pt_render_guided's first-hit log (guided.hip): the film's scratch, made by the first single-pass call; it only grows and counts against the
    // memory budget beside the render workspace.
    struct Guided {
        uint2 *d_log = nullptr;                       // 8 B per (frame of a launch, pixel of the tile list, sample): guided_kernel.h
        size_t cap = 0;                               // records it holds
        size_t bytes = 0;                             // its device bytes
    } gd;
};

#define PT_HIP(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e__ = (call);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                      \
            return PT_ERR_HIP;                                                                    \
        }                                                                                         \
    } while (0)

// ---- what every film pass (denoise.hip, reproject.hip, motion.hip, upsample.hip) takes its timing and its refusals from ("Film passes")
// The timed tail: ev_a, what `launches(stream)` queues, ev_b, the wait; the device time between the events into *device_ms (nullable).
template <class F>
inline pt_status pt_timed_pass(pt_ctx *ctx, float *device_ms, F &&launches)
{
    hipStream_t st = ctx->stream;
    PT_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    launches(st);
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    if (device_ms) PT_HIP(ctx, hipEventElapsedTime(device_ms, ctx->ev_a, ctx->ev_b));
    return PT_OK;
}
// A refusal: the message into the context, PT_ERR_INVALID_ARG out.  PT_TRY: a check's refusal is the caller's.
inline pt_status pt_bad(pt_ctx *ctx, const std::string &msg) { ctx->err = msg; return PT_ERR_INVALID_ARG; }
#define PT_TRY(call) do { const pt_status rc__ = (call); if (rc__ != PT_OK) return rc__; } while (0)
inline bool pt_finite3(const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
// The checks the parameter structs share; `name` is the struct's (pt_denoise_params, ...).
template <size_t N>
inline pt_status pt_check_reserved(pt_ctx *ctx, const char *name, const uint32_t (&reserved)[N])
{
    for (uint32_t r : reserved)
        if (r) return pt_bad(ctx, std::string(name) + ".reserved must be 0");
    return PT_OK;
}
inline pt_status pt_check_iterations(pt_ctx *ctx, const char *name, uint32_t n)
{
    return n >= 1 && n <= 8 ? PT_OK : pt_bad(ctx, std::string(name) + ".iterations must be in 1..8");
}
// sigmas: {sigma_normal, sigma_depth} or {sigma_normal, sigma_depth, sigma_color}
inline pt_status pt_check_sigmas(pt_ctx *ctx, const char *name, std::initializer_list<float> sigmas)
{
    for (float sg : sigmas)
        if (!(std::isfinite(sg) && sg > 0.f))
            return pt_bad(ctx, std::string(name) + ".sigma_normal / sigma_depth" + (sigmas.size() > 2 ? " / sigma_color" : "") + " must be finite and > 0");
    return PT_OK;
}
// what a film lacks; the plane messages end in what the refusing entry point wants done (" first", ...)
#define PT_NO_GUIDES_MSG "the film has no guide buffers: pt_film_enable_aov (and pt_render_aov) first"
#define PT_NO_M_MSG "the film has no second-moment plane: pt_film_enable_moments"
#define PT_NO_L_MSG "the film has no history-length plane: pt_film_enable_history"
#define PT_NO_Q_MSG "the film has no motion plane: pt_film_enable_motion"
#define PT_NO_K_MSG "the film has no frame-count plane: pt_film_enable_counts"

// A device array that is freed with its scope unless it is release()d to an owner.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { free(); }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, sizeof(T) * (n ? n : 1)); }
    void free() { if (p) (void)hipFree(p); p = nullptr; }
    T *release() { T *q = p; p = nullptr; return q; }
};

#define PT_BROKEN_SCENE_MSG "the scene lost its acceleration structure in a failed rebuild (out of memory?): call pt_scene_set_bvh_quality again, or recreate it"
// The scene arrays as a caller hands them over (include/pt_api.h has the layouts): in host memory (pt_scene_create, pt_scene_update) or in device
// memory (pt_scene_create_device, pt_scene_update_device).  faces: pt_scene_create* only.
struct pt_geometry { const float *vertices; uint32_t n_verts; const uint32_t *indices; const float *faces; bool on_device; };
// scene_build.hip
pt_status ptb_build_scene(pt_scene *s, const pt_geometry &g, uint32_t n_tris);
pt_status ptb_set_instances(pt_scene *s, const float *xforms3x4, uint32_t n);
pt_status ptb_set_bvh_quality(pt_scene *s, uint32_t quality);
void ptb_free_scene_buffers(pt_scene *s);
pt_status ptb_ensure_inst_lights(pt_scene *s);  // world-space emitter copies of an instanced scene (NEE pipeline only)
constexpr uint64_t PT_SOURCE_BYTES_PER_TRI = 72;  // d_tri_orig + d_faces, kept for rebuilds: part of pt_scene_info.device_bytes
pt_status ptb_ensure_inst_frames(pt_scene *s);  // the table k_shade reads instead of transforming the normal per hit (instanced scenes)
pt_status ptb_repair(pt_scene *s);        // no-op unless a rebuild of the tree products failed earlier: then one more try
pt_status ptb_ensure_wide8(pt_scene *s);  // builds the 8-wide nodes of a scene that was created without them
// pt_scene_update: new positions for the scene's triangles (mode PT_SCENE_UPDATE_REFIT / _REBUILD; arguments checked by the caller)
pt_status ptb_update_scene(pt_scene *s, const pt_geometry &g, uint32_t mode);
// scene_device.hip: what the host paths of the two do on the host, as kernels over arrays in device memory.  check_indices: PT_ERR_INVALID_ARG
// ("vertex index out of range") when one of the 3 * n_tris indices is >= n_verts; it reads d_indices only and waits for the answer.
// find_emitters (create): n_lights, h_light_prim / d_light_prim and an unfilled d_lights from d_faces.  host_products: d_lights, h_lights and
// light_area from d_tri_orig, d_faces and the emitters' ids, and (pair != nullptr: small scenes) find_fan_pairs' relation from d_tri_orig, behind
// one wait for the stream.
pt_status ptsd_check_indices(pt_ctx *ctx, const uint32_t *d_indices, uint32_t n_tris, uint32_t n_verts);
pt_status ptsd_find_emitters(pt_scene *s);
pt_status ptsd_host_products(pt_scene *s, std::vector<uint8_t> *pair);
// An emitter set by reference: the scene's own (what the two calls above fill), or a staged one that pt_scene_set_faces fills from the new
// materials while the scene renders the old ones on, and swaps in when it is whole.
struct pt_emitters {
    float4 *&d_lights; uint32_t *&d_light_prim; uint32_t &n_lights; float &light_area;
    std::vector<float4> &h_lights; std::vector<uint32_t> &h_light_prim;
};
inline pt_emitters pt_scene_emitters(pt_scene *s) { return { s->d_lights, s->d_light_prim, s->n_lights, s->light_area, s->h_lights, s->h_light_prim }; }
struct pt_staged_emitters {
    float4 *d_lights = nullptr; uint32_t *d_light_prim = nullptr; uint32_t n_lights = 0; float light_area = 0.f;
    std::vector<float4> h_lights; std::vector<uint32_t> h_light_prim;
    pt_staged_emitters() = default;
    pt_staged_emitters(const pt_staged_emitters &) = delete;
    pt_staged_emitters &operator=(const pt_staged_emitters &) = delete;
    ~pt_staged_emitters() { if (d_lights) (void)hipFree(d_lights); if (d_light_prim) (void)hipFree(d_light_prim); }  // (what was not swapped in)
    pt_emitters set() { return { d_lights, d_light_prim, n_lights, light_area, h_lights, h_light_prim }; }
};
// ... the same two for any set: the emitters of the materials d_faces (f32 [6 * n_tris], device) over the scene's d_tri_orig, into `e`
pt_status ptsd_find_emitters(pt_scene *s, const float *d_faces, pt_emitters e);
pt_status ptsd_host_products(pt_scene *s, const float *d_faces, pt_emitters e, std::vector<uint8_t> *pair);
// scene_build.hip: pt_scene_set_faces[_device] behind the argument checks -- faces: f32 [6 * n_tris] in host or device memory.  scene_faces.hip:
// its kernel, the material words of the per-triangle tables in leaf order `order` from d_faces (queued on st).
pt_status ptb_set_faces(pt_scene *s, const float *faces, bool on_device);
void ptsf_launch_set_faces(pt_scene *s, const float *d_faces, const uint32_t *order, hipStream_t st);
// ... and its fold alone: the cdf words of the n records of d_lights from their terms d_half[0..n), the total to *d_total (queued on st)
void ptsd_launch_fold(const float *d_half, uint32_t n, float4 *d_lights, float *d_total, hipStream_t st);
// scene_instances.hip: what pt_scene_set_instances does on the host with the matrices, as kernels.  check_invert: the
// n records {m, inv} into d_rec, the matrices as given into d_kept (3 float4 each), and the host loop's first error as one word (SI_OK: none;
// else (instance << 1) | kind), behind one wait for the stream.  inst_lights: ptb_ensure_inst_lights' table from s->d_xforms and d_lights.
pt_status ptsi_check_invert(pt_ctx *ctx, const float *d_xforms3x4, uint32_t n, float4 *d_rec, float4 *d_kept, uint32_t *d_verdict, uint32_t *verdict);
pt_status ptsi_inst_lights(pt_scene *s);
pt_status ptb_set_instances_device(pt_scene *s, const float *d_xforms3x4, uint32_t n);
constexpr uint32_t PT_SAH_MAX_TRIS = 2048;
// bvh4_sah_device.hip: surface-area sweep on the device (one workgroup) -> BVH4 rows (32 dwords each) + leaf order
// pair_with_next (nullable): [n] flags, triangle i and i+1 are the two halves (v0,v1,v2),(v0,v2,v3) of a quad and form ONE primitive
uint32_t pt_wide_stack_need(const std::vector<uint32_t> &rows32);
pt_status pt_sah_build_bvh4_device(pt_ctx *ctx, const float *tlo, const float *thi, uint32_t n, const uint8_t *pair_with_next, float pad,
                                   uint32_t leaf_max_prims, std::vector<uint32_t> &rows32, std::vector<uint32_t> &order);
void ptb_free_instances(pt_scene *s);
// film_work.hip: device scratch that hangs on a film (the wavefront workspace, the guide buffers' ray scratch, the denoiser's planes).
// A workspace names its buffers in SETS that are allocated and freed together, and keeps one byte counter ("Film scratch").
// A scene's device arrays go the same way, uncounted (scene_build.hip, DESIGN.md section 5, "Scene buffers").
struct pt_buf { void **p; size_t bytes; };  // one buffer of a set: where its pointer lives, the bytes it is to have (not read when it is freed)
template <class T> inline pt_buf pt_buf_of(T *&p, size_t bytes = 0) { return { reinterpret_cast<void **>(&p), bytes }; }
// scene_build.hip: every device pointer of a scene, named once, by lifetime -- what frees a lifetime is pt_scratch_free over its list
// (PT_LIFE_GIVEN: the instance set as given, in device memory -- freed with the instances, but carried across an update's parking)
enum pt_scene_life { PT_LIFE_SOURCE, PT_LIFE_TREE, PT_LIFE_INSTANCES, PT_LIFE_PREVIOUS, PT_LIFE_GIVEN };
std::vector<pt_buf> ptb_scene_buffers(pt_scene *s, pt_scene_life life);
// pt_scratch_alloc for a set of scene buffers (all of them or none; PT_ERR_OOM / PT_ERR_HIP with HIP's sticky error cleared), behind the
// tests' failure injection (pt_tuning.fail_rebuild)
pt_status ptb_scene_alloc(pt_scene *s, const char *what, const std::vector<pt_buf> &set);
// Frees the set's buffers, nulls its pointers and takes `held` (the bytes the set held) off *counter (null: a set nobody counts).
void pt_scratch_free(const std::vector<pt_buf> &set, size_t *counter, size_t held);
// Gives every buffer of the set its bytes, or none.  What the set holds now (`held` bytes) is freed FIRST, so that the peak is the new size and not
// old + new.  limit != 0: *counter + others + the set's bytes have to stay within it, else PT_ERR_OOM (message: `what` exceeds the memory budget,
// then `hint`) and nothing is allocated.  A hipMalloc that fails frees the buffers already made, nulls the set, clears HIP's sticky error and is
// PT_ERR_OOM for hipErrorOutOfMemory, PT_ERR_HIP otherwise: the context and the film stay usable.  *counter grows by the set's bytes on success only.
pt_status pt_scratch_alloc(pt_ctx *ctx, const char *what, const std::vector<pt_buf> &set, size_t *counter, size_t held, size_t others = 0,
                           size_t limit = 0, const char *hint = "");
// An optional film plane.  enable: refuses with `already_msg` when the film has it; else adopts `user_ptr` (align != 0: refused unless so aligned)
// or allocates `bytes`, zeroes it on the stream behind the renders already queued (which do not know the plane) and waits; a failure leaves the
// film without the plane.  `entry_name` is the entry point's, for the messages.  read: the plane into host_out (null: nothing is copied) after a
// wait for the stream; refuses with `missing_msg` when the film has no such plane.
pt_status pt_plane_enable(pt_film *f, pt_plane_any &plane, void *user_ptr, size_t bytes, size_t align, const char *entry_name, const char *already_msg);
pt_status pt_plane_read(pt_film *f, const pt_plane_any &plane, void *host_out, size_t bytes, const char *missing_msg);
pt_status pt_planes_clear(pt_film *f, hipStream_t st);  // zeroes the planes the film has (queued on st)
void pt_planes_free(pt_film *f);                        // frees the ones the film owns
// The 8x8 tiles of rank `rank` of `world` -- tile (tx, ty) belongs to rank (tx + ty) % world -- row by row as tx | ty << 16, appended to *tiles;
// *valid gets the running count of their pixels inside the w x h image, [n + 1] entries.  Both nullable.  -> that count over all of them.
uint64_t pt_rank_tiles(uint32_t w, uint32_t h, uint32_t rank, uint32_t world, std::vector<uint32_t> *tiles = nullptr, std::vector<uint64_t> *valid = nullptr);
// render.hip / film_work.hip
pt_status ptw_render(pt_scene *s, pt_film *f, const pt_params *p);
pt_status ptw_prepare(pt_scene *s, pt_film *f, const pt_params *p);
pt_status ptw_trace(pt_scene *s, const float *rays6, uint32_t n, float tmin, float tmax, uint32_t extend, pt_hit *hits);
void ptw_free_work(pt_film *f);
// trace_device.hip: pt_trace_device (validates everything but the null scene / desc) and the context's workspace behind it
pt_status ptt_trace_device(pt_scene *s, const pt_trace_desc *d, uint64_t n, float *device_ms);
void ptt_free(pt_ctx *ctx);
// nearest.hip: pt_nearest_device (validates everything but the null scene / desc); no workspace of its own
pt_status ptn_nearest_device(pt_scene *s, const pt_nearest_desc *d, uint64_t n, float *device_ms);
// crossings.hip: pt_crossings_device (validates everything but the null scene / desc); no workspace of its own
pt_status ptx_crossings_device(pt_scene *s, const pt_crossings_desc *d, uint64_t n, float *device_ms);
// radiance_device.hip: pt_radiance_device (validates everything but the null scene / desc) and the context's workspace behind it
pt_status ptr_radiance_device(pt_scene *s, const pt_radiance_desc *d, uint64_t n, float *device_ms);
void ptr_free(pt_ctx *ctx);
// aov.hip: guide buffers of the first hit
pt_status pta_enable(pt_film *f, void *const *device_planes);
pt_status pta_render(pt_scene *s, pt_film *f, const pt_params *p);
pt_status pta_clear(pt_film *f, hipStream_t st);   // zeroes the planes (queued on st; no-op without guides)
size_t pta_plane_bytes(const pt_film *f, uint32_t which);
void pta_free(pt_film *f);
// denoise.hip: the a-trous filter over the film and its guide planes
pt_status ptd_denoise(pt_film *f, const pt_denoise_params *p, void *device_out, float *device_ms);
pt_status ptd_denoise_variance(pt_film *f, const pt_denoise_variance_params *p, void *device_out, float *device_ms);
pt_status ptd_denoise_history(pt_film *f, const pt_denoise_history_params *p, void *device_out, float *device_ms);
void ptd_free(pt_film *f);
pt_status ptd_scratch(pt_film *f);  // the records' planes d_guide / d_illum of the film, if it has none yet (counted against the budget)
void ptd_prepare_records(pt_film *f, const float *src, hipStream_t st);  // k_dn_prepare over f into them, `src` standing in for the film plane
// upsample.hip: `lo`'s radiance to the size of `f` by f's guides (everything but the null checks is validated there)
pt_status ptu_upsample(pt_film *f, pt_film *lo, const pt_upsample_params *p, void *device_out, float *device_ms);
void ptu_free(pt_film *f);
// reproject.hip: temporal accumulation -- `f` takes over the history of `prev` (null: starts a sequence); validates everything but the null checks
// motion: pt_film_reproject_motion -- the reprojection starts from the film's plane Q
pt_status ptr_reproject(pt_film *f, pt_film *prev, const pt_reproject_params *p, float *device_ms, bool motion = false);
// motion.hip: the previous geometry of a scene and the plane Q made from it (everything but the null checks is validated there)
pt_status ptm_snapshot(pt_scene *s);
void ptm_free_previous(pt_scene *s);
pt_status ptm_motion(pt_scene *s, pt_film *f, const pt_motion_params *p, float *device_ms);
// render.hip: pt_render_adaptive (validates everything but the null checks); adaptive.hip: the selection's scratch
pt_status ptw_render_adaptive(pt_scene *s, pt_film *f, const pt_params *p, const pt_adaptive_params *ap, pt_adaptive_result *result);
void ptad_free(pt_film *f);
// render.hip: pt_render_guided (validates everything but the null checks); guided.hip: the first-hit log and the reduce that folds it into the guides
pt_status ptw_render_guided(pt_scene *s, pt_film *f, const pt_params *p, const pt_guided_params *gp, pt_guided_result *result);
pt_status ptg_ensure_log(pt_film *f, size_t records);  // the film's log holds at least `records` records (PT_ERR_OOM: not within the budget / the device)
void ptg_free(pt_film *f);
