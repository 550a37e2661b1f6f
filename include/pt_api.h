/*
 * pt_api.h -- C-ABI of the MI355X-native wavefront path tracer (libpt_amd.so).
 *
 * This is the drop-in boundary for the reference's per-pixel radiance loop.  The reference
 * (yknishidate/single-file-vulkan-pathtracing) has no FFI layer: its operator boundary is the
 * Vulkan dispatch itself, so every entry point below names the Vulkan-side interface it
 * replaces (file:line in the reference).  Plain pointers and sizes only; no C++/torch types;
 * no exceptions or aborts cross this boundary -- every call returns a pt_status and
 * pt_last_error() gives the text (the reference throws std::runtime_error, main.cpp:35, 118,
 * 151, 221, 594, 612, 681).
 *
 * Threading: calls on one context are serialised by the caller, as in the reference (single
 * host thread, single queue, main.cpp:224-238, 683).  One context per GPU; multi-GPU runs use
 * one process (or thread) per GPU, each rendering its interleaved pixel tiles.
 */
#ifndef PT_API_H
#define PT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_API_VERSION 6  /* 6: pt_get_block_counts (PT_FLAG_COUNT_VISITS on PT_PIPELINE_FUSED: the instrumented single-level fused kernel).
                           * 5: PT_PIPELINE_AUTO (what pt_params_default returns); pt_stats.pipeline / .tail_samples / .rays_culled (appended); pt_tuning.fused_tail /
                           *    .fused_subject / .cull (from the reserved words); pt_device_write.  4: PT_PIPELINE_FUSED; pt_tuning.tlas_ploc / ploc_adopt_pct / fail_rebuild */

typedef enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID_ARG = 1,
    PT_ERR_NO_DEVICE = 2,   /* no HIP device / HIP runtime unusable (replaces main.cpp:105,118) */
    PT_ERR_HIP = 3,         /* a HIP call failed; see pt_last_error                            */
    PT_ERR_OOM = 4,
    PT_ERR_UNSUPPORTED = 5
} pt_status;

typedef struct pt_ctx pt_ctx;     /* replaces Context (main.cpp:74-267): device + queue      */
typedef struct pt_scene pt_scene; /* replaces vertex/index/face Buffers + BLAS + TLAS        */
typedef struct pt_film pt_film;   /* replaces the storage Image (main.cpp:481-484)            */

/* ---- context ------------------------------------------------------------------------- */
/* device: HIP ordinal (the reference takes physical device 0, main.cpp:105).
 * stream: a hipStream_t to launch on, or NULL for the library's own stream.  The caller
 *         keeps ownership of a stream it passes in.                                        */
pt_status pt_ctx_create(int device, void *stream, pt_ctx **out);
void pt_ctx_destroy(pt_ctx *ctx);
/* Tuning knobs of a context: launch shapes and kernel choices that change SPEED, never results (every knob is set off
 * its default by a bit-exact parity test, and tests/test_tuning_knobs.py fails when a new one is not; of the COMBINATIONS
 * only those the tests name are covered).  -1 = the built-in choice, which is what was measured best on MI355X
 * (DESIGN.md section 6 has the numbers).  pt_ctx_create fills the defaults and then applies the environment variable
 * PT_TUNE once ("name=value,name=value", names as below) -- the library reads no other tuning from the environment,
 * and nothing at all inside pt_render.  Set before pt_scene_create (pair_leaves is read when a scene's BVH4 is built). */
typedef struct pt_tuning {
    int32_t refill;         /* idle lanes of a wave before it takes new rays (1..64)                                   */
    int32_t lds_stack;      /* traversal-stack entries per lane kept in LDS (kernels with a spill path)                */
    int32_t extend_blocks;  /* cap on persistent extend blocks per CU                                                  */
    int32_t pipes;          /* concurrent wavefront pipelines (streams) per pt_render, 1..4                            */
    int32_t stagger;        /* 0: free-running pipelines; 1: started half a round apart (2 pipelines); 2: shade rule (3)  */
    int32_t sort_bits;      /* ray sorting: Morton bits per axis of the origin cell (1..9)                             */
    int32_t pair_leaves;    /* 0: small scenes get leaves of <= 4 independent triangles instead of one primitive each  */
    int32_t pair_kernel;    /* 0: the per-triangle leaf loop over a pair-leaf tree instead of the pair test            */
    int32_t topdown4;       /* 0: the HBM kernel walks the collapsed LBVH instead of the top-down BVH4                 */
    int32_t rec64;          /* 0: the HBM kernel reads leaves from the 48-B tri4 records instead of the 64-B ones      */
    int32_t inst16;         /* 0: instanced scenes always take the general two-level kernel (32-bit child words)       */
    int32_t inst16_blocks;  /* compact two-level kernel: persistent blocks per CU                                      */
    int32_t enter_min;      /* ... lanes that wait to enter an instance together (1..64)                               */
    int32_t node_yield;     /* ... the node loop yields below 1/N descending lanes (0 = never)                         */
    int32_t tlas_lds_kb;    /* ... KB of TLAS top levels staged in LDS                                                 */
    int32_t term_ocap;      /* tests: cap on the per-slot overflow term log (entries)                                  */
    int32_t term_spill;     /* tests: cap on the shared term pool (entries)                                            */
    int32_t mem_budget_mb;  /* upper bound on a film's workspace, MB (also env PT_MEM_BUDGET_MB); 0 = none; -1 = 8192  */
    int32_t hbm8;           /* 1: AUTO walks big scenes through the 8-wide compressed nodes (PT_EXTEND_HBM8)           */
    int32_t ploc_radius;    /* PLOC rebuild of big scenes' binary tree: neighbours searched on either side (1..32, 8)  */
    int32_t leaf_min;       /* compact two-level kernel: lanes that wait with a triangle leaf before the leaf step runs */
    int32_t tri_enter;      /* 8-wide tree kernel: lanes that wait with leaf triangles before a triangle step runs     */
    int32_t tri_stay;       /* ... and triangle steps repeat while at least this many lanes still hold one (65 = never) */
    int32_t inst_frames;    /* 0: instanced scenes transform the normal and build its tangent frame per hit instead of reading
                               the per-(instance, triangle) table                                                         */
    int32_t tlas_ploc;      /* 1: the TLAS of an instanced scene is rebuilt by PLOC like a big scene's binary tree (0: LBVH)   */
    int32_t ploc_adopt_pct; /* a PLOC tree is kept when its area sum is below this percentage of the LBVH's (90; 1000 = always) */
    int32_t fail_rebuild;   /* NOT a speed knob -- failure injection for the tests: > 0 makes the next rebuilds of a scene's tree products fail
                               after the old ones were freed, and the next allocations of a set of scene buffers (the surface-area tree, the
                               instance set, the previous geometry, ...) of a scene that has, or has lost, a tree: each failure is PT_ERR_OOM
                               and takes one off the count.  Only pt_ctx_set_tuning sets it; PT_TUNE refuses the name.                        */
    int32_t fused_tail;     /* fused pipeline, sample_groups left at 0, single-level scenes: S of a pixel's spp samples are traced as one-sample
                               tail slots handed out after every head slot (spp - S samples) -- a launch with few slots per lane ends with short
                               work.  0 = never; -1: by the launch's slots per lane (render.hip fused_tail_samples); clamped to spp - 1.      */
    int32_t fused_subject;  /* fused pipeline: 0 = hand the tiles out centre first only; -1 / 1: the tiles the scene's box projects to first (render.hip) */
    int32_t cull;           /* 0 = walk every camera ray; -1 / 1: the slots of pixels outside the projection of the scene's box (two-level: of the instances'
                               boxes) are finished without a walk -- each of their samples is one counted ray that misses (pt_stats.rays_culled).
                               Every pipeline; with PT_FLAG_COUNT_VISITS (the walk of every ray is measured) only when set to 1             */
    int32_t reserved[2];
} pt_tuning;
pt_status pt_ctx_get_tuning(const pt_ctx *ctx, pt_tuning *out);
pt_status pt_ctx_set_tuning(pt_ctx *ctx, const pt_tuning *in);
/* Last error text of this context (ctx may be NULL: text of the last failed pt_ctx_create). */
const char *pt_last_error(const pt_ctx *ctx);
/* Blocks until everything queued on the context's stream is done (queue.waitIdle, main.cpp:683). */
pt_status pt_sync(pt_ctx *ctx);

/* ---- scene: descriptor bindings 0,2,3,4 (main.cpp:561-567, 628-641) -------------------- */
/* Takes the exact arrays the reference uploads (main.cpp:492-494):
 *   vertices f32[3*n_verts]  (closesthit.rchit:6, stride 3, closesthit.rchit:24-31)
 *   indices  u32[3*n_tris]   (closesthit.rchit:7)
 *   faces    f32[6*n_tris]   (closesthit.rchit:8: Kd.rgb, Ke.rgb, stride 6, :33-41)
 * Inputs are copied (main.cpp:321-325); the caller keeps its arrays.  Builds the LBVH on the
 * device (Morton keys + radix sort + Karras hierarchy + refit): the replacement of the BLAS/
 * TLAS builds at main.cpp:496-538 (one identity instance, opaque, no culling).              */
pt_status pt_scene_create(pt_ctx *ctx, const float *vertices, uint32_t n_verts,
                          const uint32_t *indices, uint32_t n_tris, const float *faces,
                          pt_scene **out);
void pt_scene_destroy(pt_scene *scene);

/* Two-level scenes (BASELINE config C4).  The reference builds exactly ONE identity instance
 * (main.cpp:515-538: VkAccelerationStructureInstanceKHR with an identity 3x4, mask 0xFF,
 * TriangleFacingCullDisable); this sets n instances of the scene's geometry instead.
 * xforms3x4: n object->world matrices, 3x4 row major (VkTransformMatrixKHR layout), copied.
 * n = 0 restores the single-level scene.  A TLAS (BVH4 over the instances' world boxes) is built
 * on the device.  Hits report gl_InstanceID in pt_hit.inst; ties in t go to the lowest
 * (instance, primitive).  Shading transforms the hit position by the matrix and the normal by the
 * inverse transpose (renormalised); materials are per primitive, shared by all instances.      */
pt_status pt_scene_set_instances(pt_scene *scene, const float *xforms3x4, uint32_t n);

typedef struct pt_scene_info {
    uint32_t n_tris, n_nodes /* binary LBVH */, bvh_height /* of the binary LBVH */;
    uint32_t n_wide_nodes;    /* BVH4 nodes (128 B each) the traversal kernels walk               */
    uint32_t n_instances;     /* 0 = single-level scene                                           */
    uint32_t n_tlas_nodes;    /* BVH4 nodes of the TLAS                                           */
    uint32_t leaf_max;        /* triangles per BVH4 leaf of the collapse rule (bvh4 read-back)    */
    uint32_t bvh4_builder;    /* which BVH4 is traversed: 0 collapsed LBVH, 1 surface-area sweep (small scenes), 2 PLOC tree */
    float    bbox_min[3], bbox_max[3];
    float    build_ms;        /* device time of the LBVH build, or of the last pt_scene_update (reported apart from rendering) */
    uint64_t device_bytes;    /* resident scene + BVH bytes of the BVH4 path, incl. the source arrays kept for rebuilds (72 B per triangle) */
    uint32_t n_wide8_nodes;   /* 8-wide nodes (64 B each: byte planes) of the PT_EXTEND_HBM8 path, levels of that tree */
    uint32_t wide8_levels;
    uint64_t device_bytes8;   /* resident triangle tables + BVH8 bytes of that path             */
    /* big scenes (> 2048 triangles): sum of the surface areas of the binary tree's internal nodes over the root's, for
     * the Morton-median LBVH and for its PLOC rebuild (0: not built -- FAST_BUILD, or small scene).  FAST_TRACE keeps
     * the rebuild when its sum is below 0.9 of the LBVH's (bvh4_builder says which tree is traversed).                                                      */
    float    tree_area_lbvh, tree_area_ploc;
} pt_scene_info;
pt_status pt_scene_get_info(const pt_scene *scene, pt_scene_info *info);

/* Build quality, the counterpart of vk::BuildAccelerationStructureFlagBitsKHR (main.cpp:419 passes
 * ePreferFastTrace, which is the default here too).  FAST_TRACE: scenes of <= 2048 triangles get their
 * BVH4 from an exhaustive surface-area sweep (one workgroup on the device) -- about 1/6 less traversal work
 * on the Cornell box; larger scenes get the LBVH's binary tree rebuilt bottom-up by parallel locally-ordered
 * clustering (PLOC, radius 8) before the wide nodes are collapsed from it -- what makes a finely tessellated
 * object in a large room cheap to walk.  FAST_BUILD: always the collapsed LBVH (Morton median splits).  Hit
 * records and images do not depend on the choice (closest t, lowest primitive id).  Changing the quality of
 * a big scene rebuilds its tree.  Call before pt_scene_set_instances.                                       */
typedef enum pt_bvh_quality { PT_BVH_PREFER_FAST_TRACE = 0, PT_BVH_PREFER_FAST_BUILD = 1 } pt_bvh_quality;
pt_status pt_scene_set_bvh_quality(pt_scene *scene, uint32_t quality);

/* Moves the scene's geometry: the counterpart of eAllowUpdate + BuildAccelerationStructureModeKHR::eUpdate.  vertices /
 * indices as for pt_scene_create, n_tris equal to the scene's (PT_ERR_INVALID_ARG otherwise, and on any argument error the
 * scene is left as it was); the per-face materials stay (pt_scene_set_faces changes those).  Blocking, and ordered after the work already queued on the context's
 * stream (a PT_FLAG_ASYNC render of the scene sees the old geometry); films are not touched.  Afterwards every render, trace and
 * read-back sees the new geometry, and images, ray counts and hit records equal those of a scene freshly created from the same
 * arrays, in either mode:
 *   PT_SCENE_UPDATE_REFIT    keeps the trees' topology (sorted order, leaves, node layout) and recomputes every box, table and
 *                            emitter from the new positions.  No sort and no new hierarchy: cheaper than a rebuild on small and
 *                            mid-size scenes, not yet on scenes of millions of triangles.  The trees degrade as
 *                            the geometry moves away from what they were built for: tree_area_lbvh is recomputed for the refitted
 *                            LBVH; tree_area_ploc keeps its build-time sum (the PLOC tree's binary form is not held after the
 *                            collapse).  build_ms spans the update on the stream, its host synchronisations included.  A quad whose
 *                            two halves no longer share their vertices bit for bit cannot stay one pair leaf: such a call rebuilds.
 *   PT_SCENE_UPDATE_REBUILD  builds the tree products again at the scene's quality: pt_scene_read_bvh4 then returns what a fresh
 *                            scene of the same arrays returns.
 * Instanced scenes: the BLAS is updated, then the TLAS is built again from the instances' transforms.  A failed update (out of
 * memory) leaves the scene broken like a failed rebuild (PT_BROKEN_SCENE_MSG): it holds the new triangles and builds its trees
 * from them on its next use, never a mix of old and new.                                                                   */
enum { PT_SCENE_UPDATE_REFIT = 0, PT_SCENE_UPDATE_REBUILD = 1 };
pt_status pt_scene_update(pt_scene *scene, const float *vertices, uint32_t n_verts,
                          const uint32_t *indices, uint32_t n_tris, uint32_t mode);

/* pt_scene_create and pt_scene_update for geometry that lives in DEVICE memory (a simulation, skinning, an optimiser moving a mesh): the
 * arrays have the layouts of pt_scene_create -- d_vertices f32 [3 * n_verts], d_indices u32 [3 * n_tris], d_faces f32 [6 * n_tris] -- dense,
 * 4-byte aligned, on the context's device.  After either call the scene is in the state the host call would have left with host copies of
 * the same bytes: every read-back, every field of pt_scene_get_info but build_ms, every render, trace and film pass, and whatever a later
 * pt_scene_set_bvh_quality, pt_scene_set_instances or update in either form builds from the scene's kept state are equal bit for bit.  Host
 * and device updates of one scene may be mixed freely.
 * Execution: blocking, and ordered after the work queued on the context's stream (a PT_FLAG_ASYNC render queued before the update sees the
 * old geometry).  The arrays are read on the context's stream: the caller must have finished writing them.  They are not retained: after
 * return -- whatever the status -- they may be freed or overwritten; the scene holds copies, as the host calls do.
 * No vertex, index or face array crosses to the host, in either direction.  What is read back is bounded: one word of the index check; the
 * emitters' count, their records (80 B each) and, at create, their primitive ids (a scene made from host arrays sends its ids, 4 B each, to
 * the device once, at its first device update); and, for scenes of at most 2048 triangles only, the triangles' boxes (32 B each, as the host
 * calls read them) and one byte per triangle of the pair relation: about 100 KB at most.
 * Refusals are those of the host calls, with nothing changed in the scene and *out = NULL for create: NULL arguments, empty arrays, n_tris
 * different from the scene's, an unknown mode, n_tris >= 2^28, and an index >= n_verts ("vertex index out of range").  The index check is a
 * kernel that reads only the 3 * n_tris words of d_indices and runs before any kernel follows an index: an index out of range is never
 * used as an address.  PT_SCENE_UPDATE_REFIT turns into a rebuild under pt_scene_update's rule, and a failed rebuild leaves the scene broken
 * as there.  DESIGN.md section 27.                                                                                                          */
pt_status pt_scene_create_device(pt_ctx *ctx, const void *d_vertices, uint32_t n_verts,
                                 const void *d_indices, uint32_t n_tris, const void *d_faces, pt_scene **out);
pt_status pt_scene_update_device(pt_scene *scene, const void *d_vertices, uint32_t n_verts,
                                 const void *d_indices, uint32_t n_tris, uint32_t mode);

/* pt_scene_set_instances for matrices that live in DEVICE memory (a rigid-body simulation, a pose optimiser): d_xforms3x4 holds n object->world
 * 3x4 row-major f32 matrices in pt_scene_set_instances' layout, dense, 4-byte aligned, on the context's device.  n = 0 restores the
 * single-level scene (the pointer may then be NULL); NULL with n > 0 is PT_ERR_INVALID_ARG.  After the call -- whatever its status -- the scene
 * is in the state pt_scene_set_instances leaves with a host copy of the same bytes: every field of pt_scene_get_info but build_ms, every
 * render on every pipeline (the NEE ones included), pt_trace, pt_trace_device, pt_radiance_device, pt_render_aov, pt_render_guided,
 * pt_scene_snapshot_previous + pt_film_motion + pt_film_reproject_motion, and whatever a later update, quality change, instance set or repair
 * builds from the scene's kept state are equal bit for bit.  Host and device sets of one scene may be mixed freely.
 * Refusals are the host call's and leave what it leaves (the old set is dropped before the matrices are looked at: a refused call leaves the
 * scene single-level): "instance matrix has a NaN/Inf" and "instance matrix is singular", decided for the lowest failing instance, its input
 * check before its inverse check; a broken scene is PT_ERR_UNSUPPORTED (PT_BROKEN_SCENE_MSG).
 * Execution: blocking, and ordered after the work queued on the context's stream (a PT_FLAG_ASYNC render queued before sees the old set).
 * The array is read on the context's stream; it is not retained and may be freed after return.  The scene keeps a copy in device memory
 * (48 B per instance).  One verdict word crosses to the host; no matrix and no inverse does, in either direction, neither in the call nor in
 * what follows it: the first render of any pipeline (the NEE pipelines' emitter copies are made by a kernel, and one float -- their total
 * area -- is read back), pt_scene_snapshot_previous and pt_film_motion (device-to-device copies), the re-set of the instances behind a
 * pt_scene_update[_device], the restoring of a parked set after a repair.  DESIGN.md section 28.                                        */
pt_status pt_scene_set_instances_device(pt_scene *scene, const void *d_xforms3x4, uint32_t n);

/* New per-face materials for the scene's triangles, without a rebuild: faces has pt_scene_create's layout (Kd.rgb, Ke.rgb: 6 floats per
 * triangle, n_tris rows) in host memory (pt_scene_set_faces) or, dense and 4-byte aligned, in DEVICE memory on the context's device
 * (pt_scene_set_faces_device).  After either call the scene is, bit for bit, in the state of a scene that had been created with the new
 * faces and had then taken the same later calls (quality changes, instance sets, updates, snapshots, the first request for the 8-wide tree):
 * every render on every pipeline (the NEE ones and instanced scenes included), pt_trace, pt_trace_device with its albedo and emission planes
 * and pt_radiance_device in both forms, pt_render_aov, pt_render_guided, every film pass fed by them and every field of pt_scene_get_info.
 * The trees are not touched: pt_scene_read_bvh, _bvh4 and _bvh8 return the bytes they returned before the call, and build_ms keeps its value.
 * What the call rewrites is the kept copy of the materials, a few words per triangle of the shading tables, the emitter set of the NEE
 * pipelines (its size may grow, shrink, reach 0 or leave 0) and, for instanced scenes, its world-space copies (made again by the next NEE
 * render, whose limit of 2^24 copies then applies to the new count).
 * Values are taken as pt_scene_create takes them, with no range check: -0.0, denormals, negative, overflowing, infinite, NaN (a triangle
 * emits where a Ke component is != 0: -0.0 emits nothing, a NaN does).  Host and device forms may be mixed freely, with each other and with
 * both forms of update and instance set.
 * Execution: blocking, and ordered after the work queued on the context's stream (a PT_FLAG_ASYNC render queued before the call sees the old
 * materials).  The array is read during the call and not retained: after return -- whatever the status -- it may be freed or overwritten.
 * The host form uploads the array and then takes the device form's path: one path, one set of bits.  In the device form no face array crosses
 * to the host; what is read back is what pt_scene_create_device reads back for emitters: their count, their ids (4 B each) and their records
 * (80 B each).
 * Refusals, each leaving the scene exactly as it was -- PT_ERR_INVALID_ARG: NULL scene or array; n_tris different from the scene's.
 * PT_ERR_UNSUPPORTED: a broken scene (PT_BROKEN_SCENE_MSG; pt_scene_set_instances' rule).  PT_ERR_OOM: the new emitter set, or the staged
 * copy of the materials (24 B per triangle, held during the call), cannot be allocated.  Every allocation and every read-back happens before
 * the first write to anything the scene owns: the call works on a staged copy of the faces and a staged emitter set, then swaps, so a failed
 * call renders the old materials on, never a mix.
 * pt_scene_read_faces: the scene's kept copy of the materials, f32 [6 * n_tris] (what it was created with, or the last set); NULL is
 * PT_ERR_INVALID_ARG.  It answers for a broken scene too.  DESIGN.md section 30.                                                          */
pt_status pt_scene_set_faces(pt_scene *scene, const float *faces, uint32_t n_tris);
pt_status pt_scene_set_faces_device(pt_scene *scene, const void *d_faces, uint32_t n_tris);
pt_status pt_scene_read_faces(const pt_scene *scene, float *faces);

/* Debug/parity read-back of the device-built LBVH.  keys/prim_of_pos: n_tris entries each;
 * nodes16: n_nodes x 16 dwords {lmin[3] lmax[3] rmin[3] rmax[3] left right 0 0}, child bit31 =
 * leaf (sorted position).  Any pointer may be NULL.                                         */
pt_status pt_scene_read_bvh(const pt_scene *scene, uint64_t *keys, uint32_t *prim_of_pos,
                            uint32_t *nodes16);
/* The BVH4 that is traversed (collapsed from that LBVH, or the surface-area one): n_wide_nodes x 32 dwords {lo.x[4] lo.y[4] lo.z[4] hi.x[4] hi.y[4]
 * hi.z[4] child[4] 0[4]}; child = 0xFFFFFFFF empty | node index | bit31: leaf,
 * (count-1)<<28 | first sorted position.                                                     */
pt_status pt_scene_read_bvh4(const pt_scene *scene, uint32_t *nodes32);
/* The 8-wide tree (PT_EXTEND_HBM8; big scenes build it on first request): n_wide8_nodes x 16 dwords = 64 B per node --
 * dwords 0..11: the rows lo.x lo.y lo.z hi.x hi.y hi.z of the eight children's boxes, one BYTE per child (two dwords per
 * row, child k in byte k & 3 of dword k >> 2); dword 12: origin.x | origin.y << 16; dword 13: origin.z | ex << 16 |
 * ey << 21 | ez << 26; dword 14: child_base | imask << 24; dword 15: tri_base | lmask << 24.  A plane is
 * origin16 * 2^-14 - 2 + byte * 2^-e in coordinates (x - c) / s normalised to the scene box (c, s: its centre and half
 * extent); lower planes are rounded down and upper planes up; an empty slot is lo = 255, hi = 0.  Internal children are
 * the nodes child_base + (rank of the slot in imask), leaf children the triangle positions tri_base + (rank in lmask).
 * prim_of_pos8: n_tris entries, 8-wide triangle position -> gl_PrimitiveID.  Either pointer may be NULL.               */
pt_status pt_scene_read_bvh8(const pt_scene *scene, uint32_t *nodes32, uint32_t *prim_of_pos8);

/* ---- film: descriptor binding 1 (raygen.rgen:7, main.cpp:481-484) ---------------------- */
/* float32 running-mean radiance (the canonical result) plus the reference's rgba8 display
 * image (B,G,R,A bytes, clamped + quantised on every frame like raygen.rgen:88-90).         */
pt_status pt_film_create(pt_ctx *ctx, uint32_t width, uint32_t height, pt_film **out);
/* Same, but the float film lives in caller-owned DEVICE memory (width*height*3 floats), e.g.
 * a torch tensor's data_ptr(), so a collective can reduce it in place.                      */
pt_status pt_film_create_external(pt_ctx *ctx, uint32_t width, uint32_t height,
                                  void *device_rgb_f32, pt_film **out);
pt_status pt_film_clear(pt_film *film);  /* (also zeroes the guide buffers of pt_film_enable_aov and the planes of pt_film_enable_moments / pt_film_enable_history / pt_film_enable_motion / pt_film_enable_counts) */
/* rgb: width*height*3 floats, row-major, linear radiance mean over all frames so far.       */
pt_status pt_film_read_f32(pt_film *film, float *rgb);
/* bgra: width*height*4 bytes = what main.cpp:661-667 copies to the swapchain.               */
pt_status pt_film_read_bgra8(pt_film *film, uint8_t *bgra);
void pt_film_destroy(pt_film *film);

/* ---- dispatch: pushConstants + traceRaysKHR (main.cpp:656-659) ------------------------- */
enum {
    PT_PIPELINE_WAVEFRONT = 0,     /* generate / extend / shade queues: the reference's estimator, bit for bit        */
    /* NOT the reference's estimator (opt-in, no parity with the reference's images at equal sample counts, only in
     * expectation): next-event estimation.  At every hit one point on one emitter (chosen by area) is sampled and a
     * SHADOW ray queued -- a third queue, compacted like the others and traced by the same extend kernels as an
     * any-hit query; the emission of a surface the path runs into counts for camera rays only.  Same random stream
     * otherwise (three more numbers per hit).  Fully specified arithmetic like the reference path's (the tests' CPU checker restates it bit for bit).  Instanced scenes sample every instance's copy of the emitters (world space, one cdf).
     * One sample group per pixel.  The same estimator is PT_FLAG_NEE on any pipeline value: WAVEFRONT | PT_FLAG_NEE is this pipeline.
     * The shadow ray's range is (tmin, 0.999 dist), dist the distance to the sampled point, whatever tmax is: tmax bounds the path's rays only
     * (PT_FLAG_NEE and PT_RADIANCE_NEE alike). */
    PT_PIPELINE_WAVEFRONT_NEE = 1,
    /* The reference's estimator, bit for bit, as ONE persistent kernel -- the shape of the reference's own raygen shader
     * (raygen.rgen:41-91: one invocation owns its path): traversal and shading in the same lane, path state in LDS, no
     * queues in HBM; the workspace is the per-slot radiance only (16 B per slot instead of ~150).  For scenes whose
     * triangles fit LDS: single-level ones (the Cornell-box class) and instanced ones of 2 .. 32767 instances over such a
     * BLAS (the TLAS stays in L2); PT_ERR_UNSUPPORTED otherwise, tmin > 0, blocking calls only.  Same films, same ray
     * counts as PT_PIPELINE_WAVEFRONT.  With PT_FLAG_NEE: the NEE estimator in the same single kernel (the shadow ray walks in the lane, between
     * a hit and its bounce), same films and ray counts as PT_PIPELINE_WAVEFRONT_NEE -- single-level scenes only, one sample group, no
     * PT_FLAG_COUNT_VISITS (PT_ERR_UNSUPPORTED otherwise).                                                             */
    PT_PIPELINE_FUSED = 2,
    /* What pt_params_default returns: the fastest pipeline that renders the reference's estimator bit for bit for THIS scene and call --
     * PT_PIPELINE_FUSED where it applies (scenes that live in LDS, see above; blocking calls without PT_FLAG_COUNT_VISITS), else
     * PT_PIPELINE_WAVEFRONT.  Films, rgba8 images and ray counts do not depend on the choice; pt_stats.pipeline says which one ran.
     * With PT_FLAG_NEE: PT_PIPELINE_FUSED where it would be chosen for a single-level scene, else PT_PIPELINE_WAVEFRONT_NEE.  */
    PT_PIPELINE_AUTO = 3
};
enum {
    PT_FLAG_PROFILE = 1u,      /* hipEvent-time every extend/shade launch (adds events to the stream)       */
    PT_FLAG_COUNT_VISITS = 2u, /* instrumented traversal: count BVH4 nodes / triangles visited (slower)      */
    PT_FLAG_ASYNC = 4u,        /* pt_render only queues the work (no waitIdle, main.cpp:683); pt_sync and the */
                               /* film read-backs wait for it.  No timing statistics; not with PT_FLAG_PROFILE */
    /* Ray sorting (scenes walked out of HBM): before every extend pass after the first the queue is put in (origin cell,
     * direction octant) order by a device radix sort of a permutation.  AUTO (neither flag): on when the traversal
     * working set (BVH4 nodes + triangles) exceeds the 256 MiB Infinity Cache.  Results do not depend on it.        */
    PT_FLAG_SORT_RAYS = 8u, PT_FLAG_NO_SORT_RAYS = 16u,
    /* The estimator of PT_PIPELINE_WAVEFRONT_NEE (next-event estimation, see there), independent of the implementation: WAVEFRONT | NEE =
     * PT_PIPELINE_WAVEFRONT_NEE; FUSED | NEE = the fused NEE kernel (single-level scenes of the fused class, one sample group, no
     * PT_FLAG_COUNT_VISITS); AUTO | NEE = the fused NEE kernel where AUTO would pick the fused kernel for a single-level scene, else
     * PT_PIPELINE_WAVEFRONT_NEE.  pt_stats.pipeline reports PT_PIPELINE_FUSED or PT_PIPELINE_WAVEFRONT_NEE.  (API version 6)            */
    PT_FLAG_NEE = 32u
};
/* Which closest-hit kernel runs.  All variants implement the same closest-hit definition and
 * return identical bits; AUTO picks by scene size. */
enum {
    PT_EXTEND_AUTO = 0,
    PT_EXTEND_FLAT = 1, /* deprecated (until API version 4: a brute-force loop over <= 1024 triangles, never AUTO): the name still compiles, pt_render /
                         * pt_trace return PT_ERR_UNSUPPORTED for it.  The CPU oracle (oracle/, tests only) is the brute-force reference since. */
    PT_EXTEND_FLAT_REMOVED = PT_EXTEND_FLAT,
    PT_EXTEND_LDS = 2,  /* BVH4 + triangles staged in LDS (scenes <= 24 KB by AUTO), lane refill             */
    PT_EXTEND_HBM = 3,  /* BVH4 + triangles read through L1/L2/MALL from HBM, LDS short stack + HBM spill    */
    PT_EXTEND_HBM8 = 4  /* 8-wide tree: 64-B nodes with byte planes, one stack entry per node (AUTO only with pt_tuning.hbm8) */
};

typedef struct pt_params {
    int32_t  frame;            /* push constant `frame` (main.cpp:658, raygen.rgen:8-10): first frame */
    uint32_t frame_count;      /* consecutive frames rendered by this call (reference: 1 per dispatch) */
    uint32_t width, height;    /* launch size (main.cpp:659); must equal the film's                   */
    uint32_t spp_per_frame;    /* maxSamples, 32 (raygen.rgen:43)                                      */
    uint32_t max_depth;        /* 8 (raygen.rgen:62)                                                   */
    float    tmin, tmax;       /* 0.001, 10000 (raygen.rgen:71,73)                                     */
    float    cam_origin[3];    /* (0,-1,5) (raygen.rgen:55)                                            */
    float    cam_target[3];    /* target = (d.x+tx, d.y+ty, tz); (0,-1,2) (raygen.rgen:56)             */
    float    env[3];           /* (0.7,0.6,0.5) (miss.rmiss:10)                                        */
    uint32_t rank, world;      /* this call renders the 8x8 pixel tiles (tx+ty) % world == rank        */
    uint32_t pipeline;         /* PT_PIPELINE_*                                                        */
    uint32_t frames_in_flight; /* frames traced concurrently (0 = auto); results do not depend on it   */
    uint32_t flags;            /* PT_FLAG_*                                                            */
    uint32_t extend;           /* PT_EXTEND_*                                                          */
    uint32_t sample_groups;    /* slots per (frame, pixel) tracing disjoint sample ranges concurrently  */
                               /* (0 = auto); results do not depend on it                              */
} pt_params;
void pt_params_default(pt_params *p); /* the reference's compile-time constants, 1024x1024, world 1, PT_PIPELINE_AUTO */

/* Renders frames [frame, frame+frame_count) into the film: each frame is one reference launch
 * (spp_per_frame samples/pixel, <= max_depth rays each) blended by raygen.rgen:88-90.
 * Blocking (returns after the device is done), like submit + waitIdle (main.cpp:672-683),
 * unless PT_FLAG_ASYNC is set.                                                               */
pt_status pt_render(pt_scene *scene, pt_film *film, const pt_params *params);
/* Allocates (or grows) the film's wavefront workspace for exactly the shape pt_render would pick
 * for these params, without rendering -- so the first timed pt_render does not pay for hipMalloc
 * (the pipeline / descriptor set-up of main.cpp:540-641 plays this role in the reference).
 * pt_get_stats afterwards reports the chosen frames_in_flight / sample_groups.              */
pt_status pt_render_prepare(pt_scene *scene, pt_film *film, const pt_params *params);

/* ---- guide buffers (AOVs): what a denoiser, a segmentation mask or a depth loss starts from ---------------
 * Per pixel, of the FIRST hit of the camera rays pt_render traces for the same params: albedo (Kd, not Kd / pi), the
 * shading normal of closesthit.rchit (never flipped towards the ray; instanced scenes: world space), emission (Ke),
 * depth (the hit distance t), alpha (coverage) and the {primitive, instance} id.  A frame's value of a float channel
 * is the sum over its spp_per_frame samples in sample order (a miss adds 0 to every channel: the values are
 * premultiplied by coverage, a consumer divides by alpha for the surface's own value) divided by spp_per_frame, and it
 * is blended into the plane like the film, new = (value + old * frame) / (frame + 1) -- binary32, no contraction.  The
 * id plane is not averaged: sample 0's hit of the last frame rendered, 0xFFFFFFFF twice on a miss.                  */
enum { PT_AOV_ALBEDO = 0, PT_AOV_NORMAL = 1, PT_AOV_EMISSION = 2,   /* width*height*3 f32 each */
       PT_AOV_DEPTH = 3, PT_AOV_ALPHA = 4,                          /* width*height   f32 each */
       PT_AOV_ID = 5,                                               /* width*height*2 u32      */
       PT_AOV_COUNT = 6 };
/* Gives the film its guide buffers (dense, row-major, zeroed).  device_planes: NULL, or PT_AOV_COUNT device
 * pointers; a non-NULL entry is caller-owned memory of that plane's size (a torch tensor's data_ptr(), as in
 * pt_film_create_external), a NULL entry is allocated and owned by the film.  Once per film: a second call is
 * PT_ERR_INVALID_ARG.                                                                                        */
pt_status pt_film_enable_aov(pt_film *film, void *const *device_planes);
/* Renders the guides of frames [frame, frame + frame_count) for params.  Blocking.  Does not touch the radiance film
 * or the rgba8 image; pt_render does not touch the guides.  max_depth, env, frames_in_flight and sample_groups are
 * ignored.  params->pipeline: PT_PIPELINE_WAVEFRONT generates the camera rays into a queue, traces them with the
 * closest-hit kernel params->extend names and reduces the hit records per pixel (every scene); PT_PIPELINE_FUSED is
 * one persistent kernel for single-level scenes that live in LDS with tmin > 0 (PT_ERR_UNSUPPORTED elsewhere, and with
 * a named extend kernel); PT_PIPELINE_AUTO takes the single kernel where it applies; PT_PIPELINE_WAVEFRONT_NEE is
 * PT_ERR_UNSUPPORTED.  Same bits either way; pt_stats.pipeline says which ran.  PT_FLAG_NEE is ignored, any other flag
 * is PT_ERR_UNSUPPORTED.  pt_stats.rays / .paths grow by one per sample.  PT_ERR_INVALID_ARG on a film without guides. */
pt_status pt_render_aov(pt_scene *scene, pt_film *film, const pt_params *params);
/* host_out: the plane's size (see the enum).  PT_ERR_INVALID_ARG for which >= PT_AOV_COUNT or a film without guides.  */
pt_status pt_film_read_aov(pt_film *film, uint32_t which, void *host_out);

/* ---- denoiser: guide-driven edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the radiance film ---------
 * Reads the film and the guide planes where they live and writes a separate image.  All arithmetic is binary32, every
 * operation rounded on its own, no contraction, operation order as written (the tests restate it in numpy, bit for bit).
 * Per pixel p: C the film's rgb; A, N, E, Z, a the planes albedo, normal, emission, depth, alpha exactly as stored
 * (premultiplied by coverage).
 *   demodulation   D_c = max(A_c + (1 - a), 0.001f)      (a miss counts as a surface of albedo 1 lit by the environment)
 *                  I_c = (C_c - E_c) / D_c
 *   iterations k = 0 .. n-1, step s = 2^k, h = {1/16, 1/4, 3/8, 1/4, 1/16}.  num_c = den = 0; for j = -2 .. 2 (outer), i = -2 .. 2
 *   (inner), tap q = (x + s*i, y + s*j), taps outside the image skipped:
 *                  dn  = N_p - N_q;   x_n = ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) * inv_n,   inv_n = 1.0f / (sigma_normal*sigma_normal)
 *                  dz  = Z_p - Z_q;   x_z = (dz*dz) / ((sigma_depth*sigma_depth) * (Z_p*Z_p + Z_q*Z_q) + 1e-12f)
 *                  t   = max(0, 1 - (x_n + x_z) * 0.0625f);   t = t*t, four times  (t^16: a compact-support stand-in for exp(-x))
 *                  w   = (h_j*h_i) * t;   num_c = num_c + w * I_c(q);   den = den + w
 *                  I'_c(p) = num_c / den                    (the centre tap always weighs 9/64: den > 0)
 *   remodulation   out_c = I_c * D_c + E_c after the last iteration.
 * The bgra8 form of the result is k_resolve's clamp and quantise rule on out (what the film's rgba8 image holds after frame 0 of
 * such a colour): bytes B, G, R = (uint8)(min(max(c, 0), 1) * 255.0f + 0.5f), 0 unless c > 0; A = 255.  Denormals are kept
 * (DESIGN.md section 2), so weights whose t^16 underflows follow IEEE gradual underflow.  NaN inputs are outside the contract.
 * The filter stops on normal and depth only: a colour term keeps the noise without a per-pixel variance estimate, and an albedo /
 * emission term changes little once the radiance is demodulated.
 * The defaults (5, 0.5, 0.1) come from one CPU experiment on the Cornell box at 128 x 96 and 4 spp (relative MSE 46 x below the
 * noisy film's); nobody has tuned them at 1080p.                                                                              */
typedef struct pt_denoise_params {
    uint32_t iterations;       /* 1..8; default 5 */
    float sigma_normal;        /* default 0.5  */
    float sigma_depth;         /* default 0.1  */
    uint32_t reserved[5];      /* must be 0 */
} pt_denoise_params;
void pt_denoise_params_default(pt_denoise_params *p);
/* Filters the film as it stands (the running mean of the frames rendered so far, with the guides of pt_render_aov) into
 * device_out_rgb_f32: caller-owned DEVICE memory of width*height*3 floats (a torch tensor's data_ptr()), or NULL for a plane the
 * film owns (pt_film_read_denoised).  Blocking; runs on the context's stream, ordered after the work already queued there.  Reads
 * the film and the guides and writes only the output and its own scratch: the film, the rgba8 image, the guides and pt_stats stay as
 * they were, so progressive rendering goes on afterwards.  The scratch (two ping-pong planes and the packed guides, 48 B per pixel,
 * plus 16 B per pixel for the film's own output) belongs to the film, only grows, counts against the context's memory budget with the
 * film's other workspaces (pt_tuning.mem_budget_mb) and is freed by pt_film_destroy.  device_ms (may be NULL): device time from
 * the first kernel to the last.
 * PT_ERR_INVALID_ARG: NULL film or params; a film without guides (pt_film_enable_aov); iterations outside 1..8; a sigma that is not
 * finite and > 0; a nonzero reserved word.  PT_ERR_OOM: the scratch does not fit the budget (the film renders on as before).
 * A film rendered as (rank, world) holds only its own tiles: the filter would read zeros from the other ranks' pixels.  Filter the
 * film that pt_film_present_planes assembles on the root instead: it gathers the radiance, the guides and the planes M, L, K, Q of all
 * ranks into a film (the multi-GPU section below), and this call runs on that film unchanged.                                   */
pt_status pt_film_denoise(pt_film *film, const pt_denoise_params *params, void *device_out_rgb_f32, float *device_ms);
/* The film-owned result of the last pt_film_denoise(..., NULL, ...): rgb width*height*3 floats, bgra width*height*4 bytes; either may
 * be NULL.  PT_ERR_INVALID_ARG before any denoise into the film's own plane.                                                     */
pt_status pt_film_read_denoised(pt_film *film, float *rgb, uint8_t *bgra);

/* ---- second-moment plane and the variance-guided form of the filter ---------------------------------------------------------
 * pt_film_enable_moments gives the film a plane M of width*height*3 floats, zeroed: device_m2_f32 NULL for a plane the film owns, or
 * caller-owned DEVICE memory of that size (a torch tensor's data_ptr()).  Once per film: a second call is PT_ERR_INVALID_ARG.  Like
 * the guide planes of pt_film_enable_aov it is a film plane, not a workspace: it is not counted against pt_tuning.mem_budget_mb.
 * From then on every frame pt_render resolves into this film also blends M, with c the frame's colour (sum / spp, per channel):
 *                  M_new = (c*c + M_old * (float)frame) / (float)(frame + 1)        (M_old not read when frame == 0)
 * -- the film's blend applied to c*c, binary32, every operation rounded on its own, no contraction -- in the same launch as the
 * film's blend (so PT_FLAG_ASYNC renders queue it with the resolve, and a batch redone after a term-log overflow blends it once).
 * The film, the rgba8 image, the ray counts and pt_stats of a render do not depend on whether the plane exists.  The film records
 * frames = params.frame + params.frame_count of its last pt_render; pt_film_clear zeroes M and frames.
 * Precondition: enable the plane while the film is empty -- before its frame 0, or straight after pt_film_clear.  The call does not
 * look at what the film holds: on a film that already has frames M starts at 0 beside a C that does not, M < C*C, v clamps to 0 and
 * the colour stop of pt_film_denoise_variance turns into a hard stop that keeps the noise.
 * pt_film_read_moments: m2 (width*height*3 floats) and frames, either may be NULL; PT_ERR_INVALID_ARG on a film without the plane. */
pt_status pt_film_enable_moments(pt_film *film, void *device_m2_f32);
pt_status pt_film_read_moments(pt_film *film, float *m2, uint32_t *frames);
/* pt_film_denoise_variance: pt_film_denoise with a colour stop scaled by the per-pixel variance of the film's mean, which the filter
 * carries along and propagates.  C, D, I, A, N, E, Z, a, h and the terms x_n and x_z are exactly those of pt_film_denoise; all
 * arithmetic is binary32, operation order as written.  n = params.frames, or what the film recorded when that is 0; n >= 2.
 *   variance of the mean, per channel    v_c = max(M_c - C_c*C_c, 0) / (float)(n - 1)
 *   demodulated and summed               V0  = ((v_r / (D_r*D_r)) + (v_g / (D_g*D_g))) + (v_b / (D_b*D_b))
 *                  (the expected squared distance of I from its mean: two pixels of equal true value differ by V_p + V_q in expectation)
 *   pre-blur, once: g = {1/4, 1/2, 1/4}, S = W = 0; for j = -1 .. 1 (outer), i = -1 .. 1 (inner), taps outside the image skipped:
 *                  S = S + (g_j*g_i) * V0(q);   W = W + (g_j*g_i);   V = S / W
 *   iteration k: taps and order as in pt_film_denoise; per tap, with I_p, V_p, V_q those of the iteration's input:
 *                  di  = I_p - I_q
 *                  x_c = ((di.r*di.r + di.g*di.g) + di.b*di.b) / ((sigma_color*sigma_color) * (V_p + V_q) + 1e-12f)
 *                  t   = max(0, 1 - ((x_n + x_z) + x_c) * 0.0625f);   t = t*t, four times;   w = (h_j*h_i) * t
 *                  num_c = num_c + w * I_c(q);   den = den + w;   vnum = vnum + (w*w) * V_q
 *                  I'_c(p) = num_c / den;   V'(p) = vnum / (den*den)
 *   remodulation and the bgra8 form as in pt_film_denoise.
 * An infinite x_c gives weight 0; NaN inputs are outside the contract.  sigma_color is in standard deviations of the difference of two
 * pixels: 1 keeps the noise, 8 oversmooths (DESIGN.md section 14 has the experiment the default comes from).  Placement, blocking,
 * scratch ownership (V rides in the spare word of the illumination records: the same 48 B per pixel), budget, device_ms and the caveat
 * about (rank, world) films are those of pt_film_denoise (gather with pt_film_present_planes, PT_PLANES_MOMENTS in the set: the
 * gathered film takes over `frames`); the film-owned result is read through pt_film_read_denoised.
 * PT_ERR_INVALID_ARG: NULL film or params; a film without guides or without the second-moment plane; frames resolving below 2;
 * iterations outside 1..8; a sigma that is not finite and > 0; a nonzero reserved word.  A refused call writes no result.        */
typedef struct pt_denoise_variance_params {
    uint32_t iterations;       /* 1..8; default 5 */
    float sigma_normal;        /* default 0.5  */
    float sigma_depth;         /* default 0.1  */
    float sigma_color;         /* default 3.0: in standard deviations of the difference of two pixels */
    uint32_t frames;           /* n: frames the film and M average; 0 = what the film recorded; must end up >= 2 */
    uint32_t reserved[3];      /* must be 0 */
} pt_denoise_variance_params;
void pt_denoise_variance_params_default(pt_denoise_variance_params *p);
pt_status pt_film_denoise_variance(pt_film *film, const pt_denoise_variance_params *params, void *device_out_rgb_f32, float *device_ms);

/* ---- temporal accumulation: a film rendered at a new camera takes over the history of the film of the previous camera ---------------
 * pt_film_enable_history gives the film a plane L of width*height floats, zeroed: the history length of a pixel, in reprojection steps.
 * device_len_f32 NULL for a plane the film owns, or caller-owned DEVICE memory of that size (a torch tensor's data_ptr()).  Once per film: a
 * second call is PT_ERR_INVALID_ARG.  Like the guide planes of pt_film_enable_aov and the plane of pt_film_enable_moments it is a film plane,
 * not a workspace: it is not counted against pt_tuning.mem_budget_mb.  pt_film_clear zeroes it; pt_render does not know it (the film, the
 * rgba8 image, the ray counts and pt_stats.workspace_bytes of a render do not depend on whether the plane exists).
 * pt_film_read_history: len width*height floats; PT_ERR_INVALID_ARG on a film without the plane or a NULL len.
 *
 * pt_film_reproject(film, prev, params, device_ms).  `film` holds the frames and the guides (pt_render, pt_render_aov) of the camera
 * (cam_origin, cam_target); `prev` those of (prev_cam_origin, prev_cam_target), and the history its own pt_film_reproject left in it.  The
 * call works IN PLACE on `film`: it rewrites C (the film), M (the second-moment plane) and L, and the film's bgra8 image by k_resolve's clamp
 * and quantise rule on the new C (pt_film_denoise's text above has the rule).  It leaves film's guides, everything of prev and pt_stats as
 * they were, and needs no scratch.  The result is a film again: pt_film_denoise, pt_film_denoise_variance and pt_film_present work on it
 * unchanged.  Blocking; runs on the context's stream, ordered after the work already queued there.  device_ms (may be NULL): device time of
 * the call's kernel.  prev == NULL starts a sequence: every pixel takes the "no history" path.  M is blended when both films have the plane
 * (prev == NULL: when film has it) and is not touched otherwise.
 * All arithmetic is binary32, every operation rounded on its own, no contraction, denormals kept, operation order as written (the tests
 * restate it in numpy, bit for bit).  Per pixel p = (x, y) of film: C, M its planes; N, Z, a, ID its normal, depth, alpha and id planes
 * exactly as stored (premultiplied by coverage); primed names are prev's; (o, t) = (cam_origin, cam_target), (o', t') the previous pair;
 * w, h the float sizes.
 *   Cc = C_p * gain;  Mc = M_p * gain                                      (per channel)
 *   NO HISTORY:  C_p = Cc;  M_p = Mc;  L_p = 1
 *   if prev == NULL or !(a_p > 0): NO HISTORY
 *   r   = Z_p / a_p                                                        (the first hit's distance along the camera ray)
 *   vx  = (((((float)x + 0.5f) / w) * 2 - 1) + t.x) - o.x;   vy likewise with y, h;   vz = t.z - o.z
 *   len = sqrt((vx*vx + vy*vy) + vz*vz)
 *   P   = o + (v / len) * r                                                (divide, multiply, add; per component)
 *   u   = P - o';   vz' = t'.z - o'.z
 *   if !(u.z * vz' > 0): NO HISTORY                                        (the point lies behind the previous camera)
 *   s   = vz' / u.z
 *   ex  = (u.x * s + o'.x) - t'.x;   ey likewise
 *   fx  = ((ex + 1) * 0.5f) * w - 0.5f;   fy likewise with h
 *   if !(fx > -1 && fx < w && fy > -1 && fy < h): NO HISTORY               (a NaN fails)
 *   x0 = floor(fx); bx = fx - x0;  y0, by likewise;   d = sqrt((u.x*u.x + u.y*u.y) + u.z*u.z)
 *   W = 0, Ch = Mh = 0, Lh = 0;   for j = 0, 1 (outer), i = 0, 1 (inner), q = (x0 + i, y0 + j), taps outside the image skipped:
 *       wq = (i ? bx : 1 - bx) * (j ? by : 1 - by)
 *       the tap counts when all of:  a'_q > 0;  L'_q > 0;  wq > 0;
 *           flags & PT_REPROJECT_MATCH_ID: both words of ID'_q equal ID_p's;
 *           |Z'_q - d * a'_q| <= (depth_tol * d) * a'_q;
 *           ((N_p.x*N'_q.x + N_p.y*N'_q.y) + N_p.z*N'_q.z) >= normal_min * (a_p * a'_q)
 *       W = W + wq;  Ch_c = Ch_c + wq * C'_q,c;  Mh_c = Mh_c + wq * M'_q,c;  Lh = Lh + wq * L'_q
 *   if !(W >= 0.01f): NO HISTORY
 *   Ch = Ch / W;  Mh = Mh / W;  Lh = min(Lh / W, (float)max_history)
 *   al = max(alpha, 1 / (Lh + 1))
 *   C_p = Ch + al * (Cc - Ch);   M_p = Mh + al * (Mc - Mh);   L_p = Lh + 1
 * The camera ray is pt_render's at jitter (0.5, 0.5).  NaN planes are outside the contract.
 * gain: a film cleared and then rendered at frames [f0, f0 + n) holds sum / (f0 + n), by k_resolve's blend new = (value + old * frame) /
 * (frame + 1); gain = (float)(f0 + n) / (float)n scales it back to the mean of its n frames.  The time steps of a sequence must render at
 * different `frame` values, or a static camera repeats its samples.  The guides can always be rendered at frame 0: every use of them above
 * is homogeneous in their scale (Z / a, and both sides of the depth and the normal test carry a_p * a'_q or a'_q).
 * alpha is the least weight of the new frames: 0 makes a static sequence the running mean of its steps up to max_history, 1 keeps no history.
 * After pt_scene_update the validation simply rejects what moved (pt_film_reproject_motion below follows it); a (rank, world) film holds only its own tiles,
 * the caveat of pt_film_denoise: reproject the films pt_film_present_planes gathers (PT_PLANES_HISTORY carries L).  DESIGN.md section 15 has the experiment the defaults were run on.
 * PT_ERR_INVALID_ARG: NULL film or params; prev == film; prev of another size or context; film or prev without guides or without L; exactly
 * one of the two with a second-moment plane; a camera component, gain or depth_tol that is not finite, gain or depth_tol not > 0, alpha outside
 * [0, 1], normal_min outside [-1, 1], max_history outside 1..65535; unknown flag bits; a nonzero reserved word.  A refused call writes nothing. */
pt_status pt_film_enable_history(pt_film *film, void *device_len_f32);
pt_status pt_film_read_history(pt_film *film, float *len);
enum { PT_REPROJECT_MATCH_ID = 1u };   /* a tap counts only if its {primitive, instance} id equals the pixel's */
typedef struct pt_reproject_params {
    float cam_origin[3], cam_target[3];            /* camera of `film`'s guides and frames */
    float prev_cam_origin[3], prev_cam_target[3];  /* camera of `prev`'s */
    float gain;            /* default 1 */
    float alpha;           /* default 0.2: least weight of the new frames; [0, 1] */
    float depth_tol;       /* default 0.1: relative */
    float normal_min;      /* default 0.9: least cosine; [-1, 1] */
    uint32_t max_history;  /* default 32; 1..65535 */
    uint32_t flags;        /* default PT_REPROJECT_MATCH_ID */
    uint32_t reserved[4];  /* must be 0 */
} pt_reproject_params;     /* 88 bytes */
void pt_reproject_params_default(pt_reproject_params *p);   /* the cameras: pt_params_default's */
pt_status pt_film_reproject(pt_film *film, pt_film *prev, const pt_reproject_params *params, float *device_ms);

/* ---- motion for moved geometry: where a pixel's surface point was, and a reprojection that starts from it ------------------------------
 * The caller's time step:  pt_scene_snapshot_previous -> pt_scene_update / pt_scene_set_instances (any number) -> pt_render, pt_render_aov
 * -> pt_film_motion -> pt_film_reproject_motion.
 *
 * pt_scene_snapshot_previous(scene) remembers the scene as it stands now as "the previous geometry": a device copy of the triangles' vertex
 * positions in primitive order (48 B per triangle) and the instance set's object->world matrices in gl_InstanceID order (48 B each, plus the
 * same again as the place pt_film_motion uploads the current matrices to) with their count n_i' (0: single-level).  Ordered after the work
 * queued on the context's stream; blocking.  A second call replaces the first.  The bytes are part of pt_scene_info.device_bytes from the
 * first call on (a scene that never calls it holds and reports what it did before) and are freed with the scene.  It is an explicit call and
 * not a side effect of pt_scene_update: one time step may be several updates and a pt_scene_set_instances.  A scene that lost its
 * acceleration structure is repaired first, as pt_render does it, and the call fails as that repair fails.
 *
 * pt_film_enable_motion gives the film a plane Q of width*height*4 floats, zeroed: per pixel {x, y, z, valid}.  device_q_f32x4 NULL for a
 * plane the film owns, or caller-owned DEVICE memory of that size, 16-byte aligned (a torch tensor's data_ptr()).  Once per film.  The rules
 * of pt_film_enable_history: a film plane outside pt_tuning.mem_budget_mb, zeroed by pt_film_clear, unknown to pt_render.
 * pt_film_read_motion: q4 width*height*4 floats; PT_ERR_INVALID_ARG on a film without the plane or a NULL q4.
 *
 * pt_film_motion(scene, film, params, device_ms) fills Q from the film's guides -- those rendered (pt_render_aov) for the scene as it is NOW
 * at the camera of params.  Blocking; runs on the context's stream; writes Q only (pt_stats, the guides and the film stay as they were).
 * Arithmetic as in pt_film_reproject: binary32, every operation rounded on its own, no contraction, denormals kept, order as written.  Per
 * pixel p, with n_tris the scene's triangles, n_i its instance count, (o, t) the camera, slack = bary_slack:
 *   Q_p = (0, 0, 0, 0)
 *   prim = ID_p.x;  inst = ID_p.y
 *   if !(a_p > 0) or prim >= n_tris or inst >= max(n_i, 1): done        (a miss, or an id plane that holds something else)
 *   P as in pt_film_reproject                                           (r = Z_p / a_p; v, len at jitter (0.5, 0.5); P = o + (v / len) * r)
 *   A, B, C = the triangle's vertices now;  A', B', C' = the snapshot's
 *   n_i > 0: every vertex V becomes, per row m of the instance's 3x4 matrix,  ((m0*V.x + m1*V.y) + m2*V.z) + m3
 *            (now: the scene's matrix of `inst`; primed: the snapshot's matrix of `inst`)
 *   e1 = B - A;  e2 = C - A;  g = P - A;   e1' = B' - A';  e2' = C' - A'
 *   d11 = e1.e1;  d12 = e1.e2;  d22 = e2.e2;  p1 = g.e1;  p2 = g.e2     (each (x*x + y*y) + z*z)
 *   det = d11*d22 - d12*d12
 *   u = (d22*p1 - d12*p2) / det;   v = (d11*p2 - d12*p1) / det
 *   if det > 0 and u >= -slack and v >= -slack and (u + v) <= 1 + slack   (a NaN fails):
 *       Q_p = ((A'.x + u*e1'.x) + v*e2'.x, likewise y, z, 1)
 * The barycentrics are the orthogonal projection of P onto the triangle's plane: P is an average over jittered samples and does not lie
 * on it exactly, and the id is sample 0's.  bary_slack bounds how far outside that triangle the pixel's centre may fall (in barycentric units:
 * 1 admits the neighbouring triangles of a regular tessellation, 0 only the triangle itself).  No inverse matrix is used: six vertices go
 * forward.  Primitive ids survive PT_SCENE_UPDATE_REFIT and _REBUILD, so nothing is remapped.
 * PT_ERR_INVALID_ARG, and nothing written: NULL scene, film or params; a film without guides or without Q; a film of another context than
 * the scene's; a scene without a snapshot; n_i different from the snapshot's; a camera component or bary_slack that is not finite,
 * bary_slack < 0; a nonzero reserved word.
 *
 * pt_film_reproject_motion(film, prev, params, device_ms) is pt_film_reproject -- the same parameters, refusals (plus: a film without Q),
 * effects and bgra8 rule -- with two changes to its text and nothing else:
 *   u = Q_p.xyz - o'   replaces   u = P - o'          (r, v, len and P are not computed)
 *   !(Q_p.w > 0) joins !(a_p > 0) on the NO HISTORY line
 * d = |u| is then the distance the surface point HAD from the previous camera, which is what prev's depth plane holds.  The id test needs no
 * change.  The normal test compares today's normal with yesterday's: an object that turns by more than acos(normal_min) per step loses its
 * history there (there is no previous-normal channel).  pt_film_reproject itself is unchanged.  DESIGN.md section 16 has the experiment. */
pt_status pt_scene_snapshot_previous(pt_scene *scene);
pt_status pt_film_enable_motion(pt_film *film, void *device_q_f32x4);
pt_status pt_film_read_motion(pt_film *film, float *q4);
typedef struct pt_motion_params {
    float cam_origin[3], cam_target[3];   /* camera of the film's guides */
    float bary_slack;                     /* default 1; finite, >= 0 */
    uint32_t reserved[5];                 /* must be 0 */
} pt_motion_params;                       /* 48 bytes */
void pt_motion_params_default(pt_motion_params *p);   /* the camera: pt_params_default's */
pt_status pt_film_motion(pt_scene *scene, pt_film *film, const pt_motion_params *params, float *device_ms);
pt_status pt_film_reproject_motion(pt_film *film, pt_film *prev, const pt_reproject_params *params, float *device_ms);

/* ---- per-pixel variance for reprojected films ------------------------------------------------------------------------------------------
 * pt_film_denoise_history is pt_film_denoise_variance for the film pt_film_reproject leaves: every pixel there has a history length L of
 * its own, so one caller-named n fits no pixel, and a pixel that just restarted (L = 1) holds M = C*C exactly -- its variance estimate is 0
 * and the colour stop a hard stop that keeps the noise.  This call makes V0 per pixel (the step SVGF calls variance estimation): the temporal
 * moments where the history is long enough, a spatial estimate over the 5 x 5 neighbourhood where it is not.  All arithmetic is binary32,
 * every operation rounded on its own, no contraction, denormals kept, operation order as written.  C, D, I, A, N, E, Z, a, h, x_n and x_z are
 * exactly those of pt_film_denoise; M and L are the film's planes as stored; mh = min_history.  Per pixel p = (x, y):
 *   LONG HISTORY, L_p >= mh (a NaN fails):
 *                  n   = min(L_p * (float)step_frames, n_max)
 *                  v_c = max(M_c - C_c*C_c, 0) / (n - 1)
 *                  V0  = ((v_r / (D_r*D_r)) + (v_g / (D_g*D_g))) + (v_b / (D_b*D_b))
 *   SHORT HISTORY, every other pixel (L = 0, a film that was never reprojected, included):
 *                  S = 0, s1_c = 0, s2_c = 0;  for j = -2 .. 2 (outer), i = -2 .. 2 (inner), q = (x + i, y + j), taps outside the image skipped:
 *                  t   = max(0, 1 - (x_n + x_z) * 0.0625f);   t = t*t, four times               (the guides' weight alone: no h, no colour)
 *                  S = S + t;   s1_c = s1_c + t * I_c(q);   s2_c = s2_c + t * (I_c(q) * I_c(q))
 *                  mu_c = s1_c / S;   m_c = s2_c / S;   s_c = max(m_c - mu_c*mu_c, 0);   e_c = I_c(p) - mu_c      (the centre tap has t = 1: S > 0)
 *                  Vs  = ((s_r + s_g) + s_b) + ((e_r*e_r + e_g*e_g) + e_b*e_b)
 *                  V0  = Vs * (mh / max(L_p, 1.0f))                                           (a NaN L_p counts as 1)
 * From V0 on the filter is pt_film_denoise_variance word for word: the 3 x 3 pre-blur, the iterations with x_c, V' = vnum / den^2,
 * remodulation and the bgra8 form.
 * The own-deviation term e is what a restarted pixel among converged neighbours needs: its neighbourhood's variance is small and its own
 * deviation large.  mh / max(L, 1) is SVGF's 4 / history: the estimate is of one step's variance, the pixel averages L of them, and the
 * factor errs to the blurry side.  n = min(L * step_frames, n_max) is an approximation: it is exact while 1 / (L + 1) >= alpha, where
 * pt_film_reproject is a running mean of L steps, and exact in the limit of an exponential average of weight alpha, whose effective sample
 * count tends to (2 - alpha) / alpha; between the two it is within that range.  DESIGN.md section 17 has the experiment.
 * Placement, blocking, scratch ownership (the same 48 B per pixel, V in the spare word), budget, device_ms, pt_film_read_denoised and the
 * caveat about (rank, world) films are those of pt_film_denoise_variance; the film, its planes M and L, the guides and pt_stats stay as they
 * were.
 * PT_ERR_INVALID_ARG, nothing written and nothing launched: NULL film or params; a film without guides, without the second-moment plane or
 * without L; iterations outside 1..8; a sigma that is not finite and > 0; min_history not finite or outside 1..65536; n_max not finite or < 2;
 * step_frames == 0; min_history * step_frames < 2; a nonzero reserved word.                                                              */
typedef struct pt_denoise_history_params {
    uint32_t iterations;       /* 1..8; default 5 */
    float sigma_normal;        /* default 0.5  */
    float sigma_depth;         /* default 0.1  */
    float sigma_color;         /* default 3.0  */
    float min_history;         /* default 4: pixels with L below it take the spatial estimate; finite, 1..65536 */
    float n_max;               /* default 9 = (2 - alpha) / alpha at pt_reproject_params_default's alpha: the effective sample count an
                                  exponential average tends to; finite, >= 2 */
    uint32_t step_frames;      /* default 1: frames rendered per time step; >= 1; min_history * step_frames >= 2 */
    uint32_t reserved[1];      /* must be 0 */
} pt_denoise_history_params;   /* 32 bytes */
void pt_denoise_history_params_default(pt_denoise_history_params *p);
pt_status pt_film_denoise_history(pt_film *film, const pt_denoise_history_params *params, void *device_out_rgb_f32, float *device_ms);

/* ---- guide-driven upsampling of a low-resolution film -----------------------------------------------------------------------------------
 * pt_film_upsample(film, lo, params, device_out_rgb_f32, device_ms) brings the radiance of `lo` (w' x h', w' <= w, h' <= h) to the size of
 * `film` (w x h).  Only the guides of `film` are read (pt_render_aov at the camera); `lo` holds radiance (pt_render) and guides of its own
 * (pt_render_aov), rendered at the same (cam_origin, cam_target): primary_target maps a pixel to ((x + jitter) / width) * 2 - 1 with no
 * aspect term, so a film of any size at one camera sees the same view.  All arithmetic is binary32, every operation rounded on its own, no
 * contraction, denormals kept, operation order as written; NaN planes are outside the contract.  A, N, E, Z, a are the full-size guides as
 * stored; primed names are lo's; S' is the plane params.source names (lo's film C', or the film-owned result of lo's last
 * pt_film_denoise*); inv_n and the 1e-12f of x_z are pt_film_denoise's.
 *   per lo pixel q:
 *                  D'_c = max(A'_c + (1 - a'), 0.001f);   I'_c(q) = (S'_c - E'_c) / D'_c        (pt_film_denoise's demodulation of S')
 *   once:          sx = (float)w' / (float)w;   sy = (float)h' / (float)h                        (one correctly rounded division each)
 *   per full-size pixel p = (x, y):
 *                  D_c = max(A_c + (1 - a), 0.001f)
 *                  fx = ((float)x + 0.5f) * sx - 0.5f;   x0 = floor(fx);   bx = fx - x0;        fy, y0, by likewise with y and sy
 *   FIRST RING     num_c = den = 0; for j = 0, 1 (outer), i = 0, 1 (inner), q = (x0 + i, y0 + j), taps outside lo's image skipped:
 *                  wq  = (i ? bx : 1 - bx) * (j ? by : 1 - by)
 *                  dn  = N_p - N'_q;   x_n = ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) * inv_n
 *                  dz  = Z_p - Z'_q;   x_z = (dz*dz) / ((sigma_depth*sigma_depth) * (Z_p*Z_p + Z'_q*Z'_q) + 1e-12f)
 *                  t   = max(0, 1 - (x_n + x_z) * 0.0625f);   t = t*t, four times
 *                  wt  = wq * t;   num_c = num_c + wt * I'_c(q);   den = den + wt
 *                  if den >= 0.01f:  I_c = num_c / den
 *   SECOND RING    otherwise (a NaN den included): num_c = den = 0; for j = -1 .. 2 (outer), i = -1 .. 2 (inner), the same q, taps outside
 *                  lo's image skipped, t as above:
 *                  num_c = num_c + t * I'_c(q);   den = den + t                                  (the guides' weight alone)
 *                  if den >= 0.01f:  I_c = num_c / den
 *   NEAREST        otherwise:  qn = (min(max((int)floor(fx + 0.5f), 0), w' - 1), likewise y);   I_c = I'_c(qn)
 *   remodulation   out_c = I_c * D_c + E_c
 * Demodulating with lo's albedo and remodulating with the full-size one carries albedo and emission edges at full resolution; a miss pixel
 * has D = 1, and the depth stop separates it from a surface.  The second ring serves silhouettes and thin features whose four taps all lie
 * on the other surface; the nearest tap is the last resort, so that every pixel has a defined value.  With w' = w / 2 the bilinear weights
 * are exactly {0.25, 0.75}; with w' = w, fx = x and bx = 0.  The defaults (1.0, 0.2) are the best of a 3 x 3 grid around the denoiser's
 * (0.5, 0.1) on the Cornell box at 128 x 96 from 64 x 48; nobody has tuned them at 1080p.
 * The output goes to device_out_rgb_f32: caller-owned DEVICE memory of w*h*3 floats (a torch tensor's data_ptr()), which has no bgra8
 * form; with NULL it goes to a plane `film` owns, with its bgra8 form by k_resolve's clamp and quantise rule (pt_film_denoise's text above),
 * read through pt_film_read_upsampled.  Blocking; runs on the context's stream, ordered after the work already queued there; device_ms (may
 * be NULL): device time from the first kernel to the last.  The call writes only the output and scratch: both films' C, bgra8, guides, M,
 * L, Q, lo's denoised plane and pt_stats stay as they were.  The scratch is lo's denoiser scratch (the records {I'.rgb, 0} and {N'.xyz, Z'}
 * of its pixels, 48 B per lo pixel, made here if lo never denoised) and the film-owned output (16 B per pixel of `film`, on first need);
 * both count against the context's memory budget with their film's other workspaces and are freed by pt_film_destroy.
 * PT_ERR_INVALID_ARG, nothing written and nothing launched: NULL film, lo or params; lo == film; films of different contexts; w' > w or
 * h' > h; either film without guides; an unknown source; PT_UPSAMPLE_SRC_DENOISED when lo has no film-owned denoised result; a sigma that
 * is not finite and > 0; a nonzero reserved word.  PT_ERR_OOM: the scratch does not fit pt_tuning.mem_budget_mb (both films are left as
 * they were).  The caveat about (rank, world) films is pt_film_denoise's: upsample films that pt_film_present_planes gathered.          */
enum { PT_UPSAMPLE_SRC_FILM = 0, PT_UPSAMPLE_SRC_DENOISED = 1 };
typedef struct pt_upsample_params {
    float    sigma_normal;     /* default 1.0  */
    float    sigma_depth;      /* default 0.2  */
    uint32_t source;          /* PT_UPSAMPLE_SRC_*: lo's film C', or the film-owned result of lo's last pt_film_denoise*; default _SRC_FILM */
    uint32_t reserved[5];      /* must be 0 */
} pt_upsample_params;          /* 32 bytes */
void pt_upsample_params_default(pt_upsample_params *p);
pt_status pt_film_upsample(pt_film *film, pt_film *lo, const pt_upsample_params *params, void *device_out_rgb_f32, float *device_ms);
/* The film-owned result of the last pt_film_upsample(..., NULL, ...): rgb width*height*3 floats, bgra width*height*4 bytes; either may be
 * NULL.  PT_ERR_INVALID_ARG before any upsample into the film's own plane.                                                             */
pt_status pt_film_read_upsampled(pt_film *film, float *rgb, uint8_t *bgra);

/* ---- adaptive sampling: the film's variance decides which 8x8 tiles are traced ------------------------------------------------------------
 * pt_film_enable_counts gives the film a plane K of width*height floats, zeroed: the frames each pixel holds.  device_k_f32 NULL for a plane
 * the film owns, or caller-owned DEVICE memory of that size (a torch tensor's data_ptr()).  Once per film: a second call is
 * PT_ERR_INVALID_ARG.  A film plane like L (pt_film_enable_history): not counted against pt_tuning.mem_budget_mb, zeroed by pt_film_clear,
 * and pt_render does not know it.  Precondition: a film that has K is filled by pt_render_adaptive only, starting empty -- enable K (and M,
 * pt_film_enable_moments) before the film's first frame or straight after pt_film_clear.  The calls do not look at what the film holds: after
 * a pt_render into such a film K says 0 frames beside a C that holds some, and the next adaptive blend overwrites them.
 * pt_film_read_counts: k (width*height floats); PT_ERR_INVALID_ARG on a film without the plane.
 *
 * pt_render_adaptive(scene, film, params, ap, result) renders frames [frame, frame + frame_count) for the tiles a selection pass keeps, and
 * blends each of their pixels by the pixel's own count.  All arithmetic is binary32, every operation rounded on its own, no contraction,
 * denormals kept, sqrt and / correctly rounded; NaN planes are outside the contract.  C is the film, M its second-moment plane, K the counts.
 * SELECTION, once per call, before anything is traced.  For every tile T of the film's (params.rank, params.world) tile list, lane l = 0 .. 63
 * stands for pixel (8*tx + (l & 7), 8*ty + (l >> 3)); a lane is valid if that pixel is inside the image; n_valid counts the valid lanes.
 *   short  = some valid pixel has !(K_p >= (float)min_frames)
 *   capped = max_frames > 0 and every valid pixel has K_p >= (float)max_frames
 *   e_l    = 0 for an invalid lane or !(K_p >= 2); otherwise
 *            v_c = max(M_c - C_c*C_c, 0) / (K_p - 1)
 *            e_l = sqrt((v_r + v_g) + v_b) / (((C_r + C_g) + C_b) + rel_floor)
 *   sum    : x = e; for k = 0 .. 5: x[l] = x[l] + x[l ^ (1 << k)]        (a butterfly: every lane ends with the same value)
 *   e_T    = sum / (float)n_valid
 *   selected = !capped && (short || e_T > threshold)                     (a NaN e_T is not "greater")
 * RENDER.  Pipeline, estimator, cull, frames in flight and sample groups are planned as pt_render plans them for the whole list; the frame
 * colour c of a pixel is pt_render's, bit for bit (a sample's seed depends on pixel, sample, frame and spp only).
 * BLEND.  Each valid pixel of a selected tile, in ascending frame order, starting with n = K_p:
 *   C = (c + C*n) / (n + 1);   M = (c*c + M*n) / (n + 1)                 (old values not read when n == 0)
 *   bgra8: pt_render's byte blend with n in place of the frame (old byte / 255, blend, clamp and quantise; A from 1.0)
 *   n = n + 1
 * and K_p = n at the end.  Pixels of unselected tiles are not touched in any plane.  With every tile selected in every call and frames
 * 0, 1, 2, ... the film, M and the bgra8 image are pt_render's.  The `frames` pt_film_read_moments reports is pt_render's record and is
 * not advanced: the pixels of such a film hold different numbers of frames, and K says how many.
 * pt_stats.rays grows by exactly the rays those pixels trace, paths by pixels_selected * spp_per_frame * frame_count; rays_culled follows
 * pt_render's rule; pipeline reports what ran.  frame_count == 0 is a dry run: the call selects, fills `result` and writes nothing -- the
 * caller's convergence query.  tiles_selected == 0 launches nothing after the selection and is PT_OK.  The caller uses distinct `frame`
 * values across calls (two calls with the same frame add the same samples twice: the note of pt_film_reproject).
 * Pipelines: PT_PIPELINE_WAVEFRONT, _WAVEFRONT_NEE, _FUSED and _AUTO with pt_render's support rules and fall-backs, instanced scenes
 * included; PT_FLAG_NEE, PT_FLAG_SORT_RAYS and PT_FLAG_NO_SORT_RAYS are accepted.  PT_FLAG_ASYNC, PT_FLAG_PROFILE and PT_FLAG_COUNT_VISITS
 * are PT_ERR_UNSUPPORTED: the call is blocking, it reads the count of selected tiles back.  The selection's scratch (a few words per tile of
 * the list) is the film's, counts against the context's memory budget and is freed by pt_film_destroy.
 * PT_ERR_INVALID_ARG, nothing written and nothing launched: NULL scene, film, params or ap; a film without M or without K; params whose size
 * differs from the film's (and pt_render's other refusals); threshold not finite or < 0; rel_floor not finite or <= 0; min_frames outside
 * 2..65535; a nonzero reserved word.                                                                                                  */
pt_status pt_film_enable_counts(pt_film *film, void *device_k_f32);
pt_status pt_film_read_counts(pt_film *film, float *k);
typedef struct pt_adaptive_params {
    float    threshold;    /* default 0.05: a tile is traced while its mean relative standard error exceeds it; finite, >= 0 */
    float    rel_floor;    /* default 0.01: added to the colour sum in the denominator; finite, > 0 */
    uint32_t min_frames;   /* default 4: a tile with a pixel below it is always traced; 2..65535 */
    uint32_t max_frames;   /* default 0 = none: a tile whose valid pixels all hold >= this many frames is never traced */
    uint32_t reserved[4];  /* must be 0 */
} pt_adaptive_params;      /* 32 bytes */
typedef struct pt_adaptive_result {
    uint32_t tiles_total, tiles_selected;
    uint64_t pixels_selected;       /* valid pixels of the selected tiles */
    float    max_error;             /* max e_T over the tiles without a short pixel (0 if none) */
    float    select_ms;             /* device time of the selection pass */
    uint32_t reserved[2];
} pt_adaptive_result;               /* 32 bytes */
void pt_adaptive_params_default(pt_adaptive_params *p);
pt_status pt_render_adaptive(pt_scene *scene, pt_film *film, const pt_params *params,
                             const pt_adaptive_params *ap, pt_adaptive_result *result /* may be NULL */);

/* ---- film and guides of one camera in one pass ------------------------------------------------------------------
 * Every film pass wants the radiance film and the first-hit guides of the same camera; pt_render followed by pt_render_aov walks the camera
 * rays twice.  pt_render_guided(scene, film, params, gp, result) walks them once: pt_render's fused kernels store the first hit of every
 * camera ray in a log, and a reduce kernel folds the log into the guide planes with pt_render_aov's arithmetic.
 * CONTRACT: after the call the film holds exactly what pt_render(scene, film, params) followed by pt_render_aov(scene, film, params) leaves,
 * bit for bit: C, bgra8, M if enabled, the recorded `frames`, and the six guide planes, film-owned or external.
 * mode  PT_GUIDED_AUTO         the single pass wherever pt_render would run a fused kernel for these params (single-level and instanced scenes
 *                              that live in LDS, with or without PT_FLAG_NEE, PT_PIPELINE_AUTO or _FUSED, params.extend = PT_EXTEND_AUTO) and the
 *                              log fits; everywhere else the two existing calls one after the other -- never an error they would not give
 *       PT_GUIDED_SINGLE_PASS  PT_ERR_UNSUPPORTED where AUTO would take the two calls
 *       PT_GUIDED_TWO_CALLS    the two calls, always
 * pt_stats: the single pass adds pt_render's rays, paths and rays_culled alone (no second trace happened), the two calls both calls'; `pipeline`
 * is what rendered.  result: single_pass says which form ran; launches is the number of fused launches of the single pass (0 in the two-call
 * form); guide_ms is the device time of the reduce launches, in the two-call form that of the pt_render_aov part.
 * The log is the film's scratch: 8 bytes x pixels of the rank's 8x8 tiles x spp x frames per launch (0.53 GB for one 1080p frame at 32 spp).  It only
 * grows, counts against pt_tuning.mem_budget_mb beside the render workspace and is freed by pt_film_destroy.  The call may render its frames in
 * more launches than pt_render would so that the log fits (the film does not depend on the frames in flight); if not even one frame fits,
 * AUTO takes the two calls.
 * Blocking: any flag but PT_FLAG_NEE -- PT_FLAG_ASYNC, PT_FLAG_PROFILE, PT_FLAG_COUNT_VISITS, and the ray-sort flags pt_render_aov refuses -- and
 * PT_PIPELINE_WAVEFRONT_NEE (pt_render_aov's refusal) are PT_ERR_UNSUPPORTED, before anything is launched.
 * PT_ERR_INVALID_ARG, nothing written and nothing launched: NULL scene, film, params or gp; a film without guides; an unknown mode; a nonzero
 * reserved word; every refusal of pt_render.                                                                                            */
enum { PT_GUIDED_AUTO = 0, PT_GUIDED_SINGLE_PASS = 1, PT_GUIDED_TWO_CALLS = 2 };
typedef struct pt_guided_params {
    uint32_t mode;         /* PT_GUIDED_*; default PT_GUIDED_AUTO */
    uint32_t reserved[7];  /* must be 0 */
} pt_guided_params;        /* 32 bytes */
typedef struct pt_guided_result {
    uint32_t single_pass;  /* 1: the single pass ran; 0: pt_render then pt_render_aov */
    uint32_t launches;     /* fused launches of the single pass */
    float    guide_ms;     /* device time of the guides' part */
    uint32_t reserved[5];
} pt_guided_result;        /* 32 bytes */
void pt_guided_params_default(pt_guided_params *p);
pt_status pt_render_guided(pt_scene *scene, pt_film *film, const pt_params *params,
                           const pt_guided_params *gp, pt_guided_result *result /* may be NULL */);

/* ---- closest-hit query alone: traceRayEXT (raygen.rgen:63-75) -------------------------- */
typedef struct pt_hit {
    uint32_t prim;  /* gl_PrimitiveID, 0xFFFFFFFF = miss                                   */
    float    t;     /* hit distance (0 on miss)                                             */
    float    u, v;  /* hitAttributeEXT attribs.xy: weights of v1, v2 (closesthit.rchit:56)  */
    uint32_t inst;  /* gl_InstanceID (0 without instances), 0xFFFFFFFF = miss              */
} pt_hit;
/* rays6: host array n x {origin.xyz, direction.xyz}; hits: host array of n.  Runs the same
 * extend kernel the renderer uses (opaque, no culling, tmin < t < tmax).                   */
pt_status pt_trace(pt_scene *scene, const float *rays6, uint32_t n, float tmin, float tmax,
                   uint32_t extend /* PT_EXTEND_* */, pt_hit *hits);

/* ---- ray queries on device buffers: closest hit, any hit, the surface at the hit ------------------------------------------------------
 * pt_trace_device(scene, desc, n, device_ms) answers n rays that already lie in DEVICE memory (a torch tensor's data_ptr()) into DEVICE memory:
 * no host loop, no copy, no allocation after the first call.  The rays are repacked by a kernel into the queue layout of the extend kernels the
 * renderer uses, walked in chunks of desc.chunk_rays by the kernel pt_trace would take for desc.extend (every scene class: LDS, HBM, the 8-wide
 * tree, both two-level kernels), and the hit records are turned into the caller's arrays by kernels again.  pt_trace is untouched.
 *
 *   PT_TRACE_CLOSEST  d_hits[i] is byte for byte what pt_trace returns for ray i with the same tmin, tmax and extend (instanced scenes too: inst,
 *                     ties to the lowest (instance, primitive)).  d_hits may be NULL when only the surface record is wanted.  d_tmax must be
 *                     NULL: PT_ERR_UNSUPPORTED otherwise -- the kernels' per-ray bound belongs to their any-hit instantiations, which end a walk
 *                     at the FIRST hit below the bound, and no closest-hit instantiation reads a per-ray bound.
 *   PT_TRACE_ANY      d_occluded[i] = 1 exactly when the closest-hit query of ray i with the ray's bound as tmax finds a triangle (tmin < t < bound,
 *                     opaque, no culling), else 0.  The bound is d_tmax[i], or desc.tmax for every ray when d_tmax is NULL (the call then fills its
 *                     bound plane with it).  Both ends are strict: a triangle at exactly t == bound does not occlude.  Where d_tmax is given,
 *                     desc.tmax plays no part in the answer (it must still be finite and above tmin): a bound beyond it, +inf included, is
 *                     honoured as it stands, and a bound at or below tmin occludes nothing.  Runs the any-hit instantiations (the
 *                     NEE pipeline's shadow-ray kernels), which stop at the first hit.  d_hits and the four surface pointers must be NULL.
 *
 * The surface record (PT_TRACE_CLOSEST; each of the four planes n x 3 floats, dense, any may be NULL) is what closesthit.rchit:50-65 computes at
 * the hit, in binary32 with every operation rounded on its own (no contraction, denormals kept), A B C the hit triangle's vertices, (u, v) the
 * hit's attributes:
 *   d_position  b0 = (1 - u) - v, then per component P = (A * b0 + B * u) + C * v.  Instanced scenes: per row (m0 m1 m2 m3) of the instance's
 *               3x4 object->world matrix the component becomes ((m0 * P.x + m1 * P.y) + m2 * P.z) + m3.
 *   d_normal    the triangle's shading normal -normalize(cross(B - A, C - A)), never flipped towards the ray: the per-sample value PT_AOV_NORMAL
 *               averages.  Instanced scenes: in world space -- the inverse transpose of the instance's matrix applied as
 *               (i0 * n.x + i1 * n.y) + i2 * n.z per component and renormalised by a correctly rounded square root and divide, or the same
 *               value read from the per-(instance, triangle) table where the context keeps one (pt_tuning.inst_frames).
 *   d_albedo    the face's Kd (not Kd / pi: PT_AOV_ALBEDO's convention).
 *   d_emission  the face's Ke.
 * A ray that misses gets +0.0 in all three components of every plane.  All five CLOSEST outputs NULL is PT_ERR_INVALID_ARG.
 *
 * Execution.  Everything runs on the context's stream, behind the work already queued there (pt_scene_update's rule: a query queued before an
 * update sees the old geometry).  The call blocks unless PT_TRACE_ASYNC is set; with the flag it only queues, pt_sync waits, the inputs have to
 * stay valid and the outputs are defined only after that wait.  *device_ms (nullable): first kernel to last kernel; 0, and no event is touched,
 * under PT_TRACE_ASYNC.  pt_stats: launches_extend grows by the number of chunks, ms_extend by the extend kernels' own time (blocking calls only),
 * launches_other by the pack and unpack launches; rays and paths stay (they count a render's rays and samples).  A scene that lost its trees is
 * repaired first, as pt_trace does.  NaN rays behave as in pt_trace; a NaN bound is outside the contract.  n == 0 is PT_OK and launches nothing.  n is 64-bit: a tensor of
 * rays can exceed 2^32 bytes; chunk_rays bounds the workspace, not n.
 *
 * Workspace: a chunk's rays, hit records and bound plane, 48 B per ray of min(chunk_rays, n rounded up to 64), belong to the CONTEXT: made by the
 * first call, only growing (a second call with the same or a smaller chunk allocates nothing), counted against pt_tuning.mem_budget_mb
 * (PT_ERR_OOM when a chunk does not fit: nothing is launched, the context stays usable and a smaller chunk_rays works), freed by pt_ctx_destroy.
 * pt_trace_workspace_bytes reports the bytes held.  PT_TRACE_DEFAULT_CHUNK_RAYS is 2^22 rays (192 MiB, and only for queries that large): of the
 * chunks 2^16 .. 2^22 swept on the MI355X over 2^24 rays (scripts/probe_trace_device.py, profiles/trace_device_probe.json) the largest was the
 * fastest on both scenes and no smaller one lay within its spread -- Cornell box 0.68 ms at 2^20, 0.52 at 2^21, 0.45 at 2^22; 1 M-triangle soup
 * 7.7 / 5.4 / 4.4 ms: every chunk ends in a tail in which the extend kernel's persistent waves run out of rays.  Nothing beyond 2^22 was swept
 * (DESIGN.md section 22).
 *
 * The single-kernel form.  PT_TRACE_FUSED runs the rays of a launch through ONE persistent kernel: a lane reads row i of d_rays6 (and, for
 * PT_TRACE_ANY, d_tmax[i]), walks the scene in LDS and writes ray i's answer straight into the caller's arrays -- no pack and unpack launches, no
 * queues, no hit records in memory and NO workspace (pt_trace_workspace_bytes is unchanged by such a call; a context that only ever runs this form
 * reports 0).  The outputs are byte for byte those of the queue form, for both modes and every subset of the output pointers, and every statement
 * and refusal above holds (d_tmax with PT_TRACE_CLOSEST stays PT_ERR_UNSUPPORTED).  It applies where the queue form would run the compact LDS
 * kernel: a single-level scene, desc.extend == PT_EXTEND_AUTO, nodes and triangles within the LDS class (24 KB, 2047 triangles, 16 stack entries)
 * and tmin > 0; pair-leaf trees and leaves of up to four (pt_tuning.pair_leaves = 0 or pair_kernel = 0).  Everywhere else -- instanced scenes,
 * scenes beyond the LDS class, a named extend kernel, tmin <= 0 -- PT_TRACE_FUSED is PT_ERR_UNSUPPORTED with nothing launched or written (the text
 * names the class).  chunk_rays bounds the queue form's workspace and is ignored: one launch per 2^30 rays.  pt_stats: launches_extend grows by one
 * per launch, ms_extend by the kernel's own time (blocking calls), launches_other and rounds stay, extend_variant = PT_EXTEND_LDS.
 * PT_TRACE_AUTO takes the single-kernel form where it applies AND won the measurements of DESIGN.md section 26 for the kind of query (PT_TRACE_CLOSEST
 * into d_hits alone, PT_TRACE_CLOSEST with surface planes, PT_TRACE_ANY), else the queue form; it is never an error the call would not be without
 * it.  Measured on the MI355X (Cornell box, 2^20 and 2^24 rays, coherent and shuffled, medians of 7 against the queue form of the previous
 * build, profiles/trace_fused_probe.json): the single-kernel form's slowest pass was faster than the queue form's fastest on every shape of every
 * kind -- d_hits alone 1.36x .. 2.10x, with the surface planes 1.20x .. 1.98x, PT_TRACE_ANY 1.45x .. 2.29x -- so PT_TRACE_AUTO takes it for all
 * three kinds wherever it applies.
 * Under either bit pt_stats.pipeline says which form ran (PT_PIPELINE_FUSED / PT_PIPELINE_WAVEFRONT); without them the field is not touched and the
 * call is exactly the queue form above.  PT_TRACE_ASYNC combines with both.  The two bits together are PT_ERR_INVALID_ARG.
 *
 * Refusals, with nothing launched and nothing written -- PT_ERR_INVALID_ARG: NULL scene or desc; NULL d_rays6 with n > 0; an unknown mode or
 * flag; PT_TRACE_FUSED together with PT_TRACE_AUTO; a nonzero reserved word; tmin or tmax not finite, or tmax <= tmin; PT_TRACE_CLOSEST with all of d_hits and the surface pointers NULL or
 * with d_occluded set; PT_TRACE_ANY with d_occluded NULL or with d_hits or a surface pointer set; an unknown extend value.  PT_ERR_UNSUPPORTED:
 * d_tmax with PT_TRACE_CLOSEST; PT_EXTEND_FLAT and the variants the scene has no tree for (pt_trace's rules); PT_TRACE_FUSED outside its class. */
enum { PT_TRACE_CLOSEST = 0, PT_TRACE_ANY = 1 };
enum { PT_TRACE_ASYNC = 1u, /* (2: no flag) */ PT_TRACE_FUSED = 4u, PT_TRACE_AUTO = 8u };
#define PT_TRACE_DEFAULT_CHUNK_RAYS (1u << 22)
typedef struct pt_trace_desc {
    const void *d_rays6;     /* DEVICE, n x {origin.xyz, direction.xyz} f32, dense, 4-byte aligned */
    const void *d_tmax;      /* DEVICE n f32 per-ray upper bound (PT_TRACE_ANY), or NULL: `tmax` for every ray */
    void *d_hits;            /* CLOSEST: DEVICE n x pt_hit (20 B), may be NULL */
    void *d_occluded;        /* ANY: DEVICE n x uint8, 1 = some triangle with tmin < t < bound */
    void *d_position, *d_normal, *d_albedo, *d_emission;  /* CLOSEST: DEVICE n x 3 f32 each, any may be NULL */
    float tmin, tmax;
    uint32_t mode;           /* PT_TRACE_* */
    uint32_t extend;         /* PT_EXTEND_*, pt_trace's rules */
    uint32_t flags;          /* PT_TRACE_ASYNC | one of PT_TRACE_FUSED, PT_TRACE_AUTO, or 0 */
    uint32_t chunk_rays;     /* rays per launch; 0 = PT_TRACE_DEFAULT_CHUNK_RAYS; rounded up to a multiple of 64 */
    uint32_t reserved[4];    /* must be 0 */
} pt_trace_desc;             /* 104 bytes */
void pt_trace_desc_default(pt_trace_desc *d);   /* pointers NULL, tmin 0.001, tmax 10000, CLOSEST, AUTO */
pt_status pt_trace_device(pt_scene *scene, const pt_trace_desc *desc, uint64_t n, float *device_ms /* may be NULL */);
/* the device bytes the context holds for pt_trace_device (0 before the first call) */
pt_status pt_trace_workspace_bytes(const pt_ctx *ctx, uint64_t *bytes);

/* ---- closest point on the mesh for points in device memory ------------------------------------------------------------------------------
 * pt_nearest_device(scene, desc, n, device_ms) answers, for n points that lie in DEVICE memory, "which point of the mesh is closest to P, on
 * which triangle, and how far away?" into DEVICE memory: penetration depth, contact candidates, a point-to-mesh or Chamfer loss, an unsigned
 * distance field.  One persistent kernel per launch reads row i of d_points, walks the scene's BVH4 (the tree pt_scene_read_bvh4 returns, kept
 * current by pt_scene_update[_device]) by box distance and writes query i's answer straight into the caller's arrays.
 *
 * Definition.  The result is bit-exact by construction: all arithmetic is binary32, every operation rounded on its own, no contraction, denormals
 * kept; dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; min, max and clamp are selects (a NaN stays a NaN).  For a query P and a triangle with
 * vertices A, B, C (as pt_scene_create got them), the region algorithm of Ericson, Real-Time Collision Detection 5.1.5, in this order:
 *   ab = B - A, ac = C - A, ap = P - A;  d1 = dot(ab, ap), d2 = dot(ac, ap);           d1 <= 0 && d2 <= 0             -> (u, v) = (0, 0)
 *   bp = P - B;  d3 = dot(ab, bp), d4 = dot(ac, bp);                                     d3 >= 0 && d4 <= d3            -> (1, 0)
 *   vc = d1 * d4 - d3 * d2;                                                              vc <= 0 && d1 >= 0 && d3 <= 0  -> (d1 / (d1 - d3), 0)
 *   cp = P - C;  d5 = dot(ab, cp), d6 = dot(ac, cp);                                     d6 >= 0 && d5 <= d6            -> (0, 1)
 *   vb = d5 * d2 - d1 * d6;                                                              vb <= 0 && d2 >= 0 && d6 <= 0  -> (0, d2 / (d2 - d6))
 *   va = d3 * d6 - d5 * d4, e = d4 - d3, f = d5 - d6;                                    va <= 0 && e >= 0 && f >= 0    -> w = e / (e + f), (1 - w, w)
 *   otherwise  s = (va + vb) + vc                                                                                       -> (vb / s, vc / s)
 * with the true IEEE divide; u and v are the weights of B and C (pt_hit's convention).  Then per component Q = (A + ab * u) + ac * v, CLAMPED to
 * [min(A, B, C), max(A, B, C)]; D = P - Q; dist2 = (D.x * D.x + D.y * D.y) + D.z * D.z.  (The clamp does nothing in exact arithmetic.  It is
 * what makes the tree walk exact: with it dist2 is never below the same expression's distance to any fp32 box that contains the triangle's
 * vertices -- csrc/nearest_kernel.h has the lemma -- so skipping a box that lies strictly beyond the best dist2 found loses nothing.)
 * Search radius: m = d_max_dist[i], or desc.max_dist for every query; r2 = m * m if m >= 0; a negative or NaN m finds nothing.
 * Winner: over ALL triangles with dist2 <= r2 the least dist2, then the lowest primitive id.  A NaN dist2 (the interior branch of a degenerate
 * triangle, a NaN query) never wins.  d_nearest[i] = {prim, dist2, u, v} of the winner, d_point[i] = its Q.
 * Miss: a query that finds nothing gets prim = 0xFFFFFFFF, dist2 = u = v = +0.0, and d_point = +0.0 three times.
 * The answer is a property of the triangles alone: it does not depend on the tree, the builder (pt_scene_set_bvh_quality), the form, the launch
 * shape or any pt_tuning knob, and equals the loop over all triangles bit for bit.
 *
 * Execution.  Blocking, on the context's stream, behind the work already queued there.  A scene that lost its trees is repaired first, as
 * pt_trace_device does.  n == 0 is PT_OK and launches nothing.  n is 64-bit: one launch per 2^30 queries.  No workspace: stack entries beyond
 * the per-lane LDS share (pt_tuning.lds_stack) go to the context's stack-spill area, which the ray kernels use too; pt_trace_workspace_bytes is
 * unchanged.  pt_stats: launches_other grows by the number of launches; rays, paths, launches_extend, pipeline and extend_variant are not
 * touched.  *device_ms (nullable): first kernel to last kernel.  pt_tuning.refill, lds_stack and extend_blocks shape the launch as they shape the
 * ray kernels'.
 * Forms.  PT_NEAREST_LDS stages the nodes (144 B each) and one copy of the triangles (48 B each) in LDS; it applies while that image and the
 * stack (lds_stack x 2 KB per block) fit 96 KB.  PT_NEAREST_GLOBAL reads both through the caches and always applies.  PT_NEAREST_AUTO is
 * PT_NEAREST_GLOBAL for every scene: it would take the LDS form for scenes of the ray kernels' LDS class (24 KB) only if that form's slowest
 * measured pass beat the GLOBAL form's fastest on every shape (pt_trace_device's rule for PT_TRACE_AUTO).  Measured on the MI355X (Cornell box,
 * 2^20 and 2^24 queries on a lattice and near the surface, in order and shuffled, medians of 7, profiles/nearest_probe.json): the LDS form's
 * medians are 1.04 .. 1.21x faster on all eight shapes -- 2^24 lattice queries 0.66 against 0.73 ms (25 against 23 G queries/s), 2^20 shuffled
 * 0.076 against 0.082 ms -- but on one shape its slowest pass (0.0645 ms) does not beat the GLOBAL form's fastest (0.0634 ms), so the rule keeps
 * AUTO on GLOBAL; a caller who knows the scene fits names PT_NEAREST_LDS.  The 1 M-triangle soup answers 2^20 queries in 0.71 .. 0.89 ms.
 *
 * Refusals, with nothing launched and nothing written -- PT_ERR_INVALID_ARG: NULL scene or desc; NULL d_points with n > 0; d_nearest and d_point
 * both NULL; an unknown form; flags != 0; a nonzero reserved word; max_dist NaN or negative when d_max_dist is NULL.  PT_ERR_UNSUPPORTED: an
 * instanced scene -- distance under an instance's general 3x4 matrix is not object-space distance (pt_scene_set_instances with n = 0 restores
 * the mesh); PT_NEAREST_LDS for a scene whose image does not fit.
 * Out of scope: instanced scenes; k nearest; an asynchronous flag.  (Signed distance: the sign is pt_crossings_device's business, below -- the
 * face normal of `prim` is the wrong answer wherever Q lies on an edge or a vertex; the Python binding's Scene.signed_distance_tensors puts the
 * two calls together.) */
typedef struct pt_nearest { uint32_t prim; float dist2, u, v; } pt_nearest;   /* 16 bytes */
enum { PT_NEAREST_AUTO = 0, PT_NEAREST_LDS = 1, PT_NEAREST_GLOBAL = 2 };
typedef struct pt_nearest_desc {
    const void *d_points;    /* DEVICE n x 3 f32, dense, 4-byte aligned */
    const void *d_max_dist;  /* DEVICE n f32 per-query search radius, or NULL: `max_dist` for every query */
    void *d_nearest;         /* DEVICE n x pt_nearest, may be NULL */
    void *d_point;           /* DEVICE n x 3 f32: the closest point itself, may be NULL */
    float max_dist;          /* default +inf */
    uint32_t form;           /* PT_NEAREST_* */
    uint32_t flags;          /* must be 0 */
    uint32_t reserved[5];    /* must be 0 */
} pt_nearest_desc;           /* 64 bytes */
void pt_nearest_desc_default(pt_nearest_desc *d);   /* pointers NULL, max_dist +inf, AUTO */
pt_status pt_nearest_device(pt_scene *scene, const pt_nearest_desc *desc, uint64_t n, float *device_ms /* may be NULL */);

/* ---- crossing counts and winding for rays in device memory ------------------------------------------------------------------------------
 * pt_crossings_device(scene, desc, n, device_ms) answers, for n rays that lie in DEVICE memory, "how many triangles does this ray cross inside
 * its range, and what is the signed sum of the crossings?" into DEVICE memory: the parity of the count says on which side of a closed surface
 * the origin lies (inside / outside, the sign of a signed distance), the count itself gives thickness and occupancy.  No other walk of the
 * library can say it: closest-hit walks shrink their range and any-hit walks stop.  One persistent kernel per launch reads row i, walks the
 * scene's BVH4 (the tree pt_scene_read_bvh4 returns) with the ray's whole range and writes ray i's two words straight into the caller's arrays.
 *
 * Definition.  Bit-exact by construction: all arithmetic is binary32, every operation rounded on its own, no contraction, denormals kept; min
 * and max are selects.  Ray i: origin O and direction D = row i of d_rays6, or O = row i of d_points and D = desc.direction; range (tmin, b)
 * with b = d_tmax[i], or desc.tmax for every ray.  A triangle (A, B, C) COUNTS when both hold:
 *   Triangle test.  pt_trace's canonical test accepts it with tmin < t < b (both ends exclusive): dominant axis kz = the first largest |D|
 *     component, kx = kz + 1, ky = kz + 2 (mod 3); Sx = D.kx / D.kz, Sy = D.ky / D.kz, Sz = 1 / D.kz by true divides; per vertex P' = P - O,
 *     x = P'.kx - Sx * P'.kz, y = P'.ky - Sy * P'.kz; U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax; rejected when some
 *     of U, V, W is < 0 and some is > 0 (a zero edge function counts as inside); det = (U + V) + W, rejected when det == 0;
 *     t = ((U * (Sz * A'.kz) + V * (Sz * B'.kz)) + W * (Sz * C'.kz)) / det; a NaN anywhere rejects.  No tie rule is involved: every accepted
 *     triangle counts, duplicates included.
 *   Own-box test.  pad = the largest absolute ordinate of the scene's box (pt_scene_info.bbox_min / bbox_max) times 2^-18 -- what every builder
 *     and the refit put around every leaf.  lo = min(A, B, C) - pad, hi = max(A, B, C) + pad per component.  inv = 1 / copysign(max(|d|, 1e-20), d)
 *     per component d of D, the correctly rounded reciprocal.  Per axis x0 = (lo - O) * inv, x1 = (hi - O) * inv;
 *     tn = max(max(min x, min y), max(min z, tmin));  tf = min(min(max x, max y), min(max z, b));  the test passes iff tn <= tf * 1.0000004f.
 * count[i] (u32) = the number of triangles that count.  winding[i] (i32) = the sum over them of +1 where det > 0 and -1 where det < 0.
 * What the sign means: det has the sign of -(cross(B - A, C - A) . D) * D.kz (the triangle test does not swap kx and ky for a negative
 * dominant component).  So for a ray whose dominant direction component is POSITIVE, det > 0 (+1) is a triangle whose geometric normal
 * cross(B - A, C - A) points against the ray -- the ray enters through its front -- and det < 0 (-1) one it leaves through the front of; for a
 * NEGATIVE dominant component the two swap.  winding * sign(D.kz) is therefore (entered - left) by cross(B - A, C - A): 0 outside a closed,
 * consistently oriented mesh whichever way it is oriented, +-1 inside, the sign telling the orientation.  (pth_load_obj negates Y, which
 * reverses the orientation of a loaded OBJ: a caller who needs the sign's meaning pins it on one triangle of the arrays given to
 * pt_scene_create.)
 * Rays that answer count = winding = 0 without a walk: a non-finite component of O or D; a NaN b; b <= tmin.  (A zero direction needs no rule:
 * its shears are 0 / 0 = NaN and the triangle test rejects every triangle.)
 * Why the own-box test is part of the definition.  A loop over all triangles meets triangles far away in units of their own size, whose
 * sheared coordinates are quantised so coarsely that two edge functions cancel to exactly 0: a "hit" at a vertex of a triangle the ray never
 * comes near.  A closest-hit walk is rarely hurt by them, a count over all triangles is exposed on every triangle; the own box drops them.  And
 * it makes the tree walk exact by a lemma (csrc/crossings_kernel.h): for a finite ray the slab test has no NaN and is monotone in the box, so a
 * ray that passes a triangle's own padded box passes every fp32 box that contains it -- every box on the path to the triangle, through
 * pt_scene_update refits too.  The result is a property of the triangles and the scene's box alone: it does not depend on the tree, the builder
 * (pt_scene_set_bvh_quality), the form, the launch shape or any pt_tuning knob, and equals the loop over all triangles bit for bit.
 * Caveats that follow from the acceptance rule: a ray through a shared edge counts both triangles, a ray through a vertex the whole fan, a
 * duplicated face twice.  Parity means inside / outside for closed meshes only, and off those measure-zero sets; callers vote over a few
 * directions (the Python binding's Scene.inside_tensors).
 *
 * Execution.  Blocking, on the context's stream, behind the work already queued there.  A scene that lost its trees is repaired first.
 * n == 0 is PT_OK and launches nothing.  n is 64-bit: one launch per 2^30 rays.  No workspace: stack entries (4 bytes) beyond the per-lane LDS
 * share (pt_tuning.lds_stack) go to the context's stack-spill area.  pt_stats: launches_other grows by the number of launches; rays, paths,
 * launches_extend, pipeline and extend_variant are not touched.  *device_ms (nullable): first kernel to last kernel.  pt_tuning.refill,
 * lds_stack and extend_blocks shape the launch as they shape pt_nearest_device's.
 * Forms.  PT_CROSSINGS_LDS stages the nodes (144 B each) and one copy of the triangles (48 B each) in LDS; it applies while that image and the
 * stack (lds_stack x 1 KB per block) fit 96 KB.  PT_CROSSINGS_GLOBAL reads both through the caches and always applies.  PT_CROSSINGS_AUTO takes
 * the LDS form for scenes of the ray kernels' LDS class (24 KB) and the GLOBAL form for every other scene.  The rule is pt_nearest_device's: the
 * LDS form only if its slowest measured pass beat the GLOBAL form's fastest on every shape measured.  Measured on the MI355X (Cornell box, 2^20
 * and 2^24 rays from a lattice, in order and shuffled, range (0.001, +inf), the forms alternated in one loop, medians of 7 with min .. max,
 * scripts/probe_crossings.py -> profiles/crossings_probe.json): 2^20 in order 0.0994 (0.0980 .. 0.1022) against 0.1084 (0.1059 .. 0.1104) ms
 * -- the narrowest of the four, 0.1022 below 0.1059 --, 2^20 shuffled 0.0996 against 0.1258, 2^24 in order 1.161 against 1.381, 2^24
 * shuffled 0.947 against 1.455 (17.7 against 11.5 G rays/s): the LDS form's slowest pass beat the GLOBAL form's fastest on all four, by
 * 1.09 .. 1.54x in the medians, outputs byte-equal.  The walk never prunes, so a big scene is slow: the 1 M-triangle soup (6.9 crossings per
 * ray on average) takes 8.8 .. 9.4 ms for 2^20 rays and 118 .. 144 ms for 2^24, 10 .. 17x pt_trace_device's any-hit on the same rays
 * (DESIGN.md section 32).
 *
 * Refusals, with nothing launched and nothing written -- PT_ERR_INVALID_ARG: NULL scene or desc; d_rays6 and d_points both set or both NULL
 * with n > 0; d_count and d_winding both NULL; an unknown form; flags != 0; a nonzero reserved word; tmin not finite; tmax NaN or <= tmin while
 * d_tmax is NULL; a non-finite direction while d_points is set.  PT_ERR_UNSUPPORTED: PT_CROSSINGS_LDS for a scene whose image does not fit;
 * an instanced scene -- counting under instances is well defined for rays (unlike distance) and is simply not built: it needs a two-level
 * walk and a pad per instance (pt_scene_set_instances with n = 0 restores the mesh).
 * Out of scope: instanced scenes; a fill rule that counts a shared edge once; the list of the hits; an asynchronous flag; the generalized
 * winding number. */
enum { PT_CROSSINGS_AUTO = 0, PT_CROSSINGS_LDS = 1, PT_CROSSINGS_GLOBAL = 2 };
typedef struct pt_crossings_desc {
    const void *d_rays6;     /* DEVICE n x {origin.xyz, direction.xyz} f32, dense, 4-byte aligned, or NULL */
    const void *d_points;    /* DEVICE n x 3 f32 origins sharing `direction`, or NULL; exactly one of the two */
    const void *d_tmax;      /* DEVICE n f32 per-ray upper end, or NULL: `tmax` for every ray */
    void *d_count;           /* DEVICE n x u32, may be NULL */
    void *d_winding;         /* DEVICE n x i32, may be NULL (not both) */
    float direction[3];      /* the direction of every d_points ray */
    float tmin, tmax;        /* defaults 0 and +inf; range tmin < t < bound, both ends exclusive */
    uint32_t form;           /* PT_CROSSINGS_* */
    uint32_t flags;          /* must be 0 */
    uint32_t reserved[3];    /* must be 0 */
} pt_crossings_desc;         /* 80 bytes */
void pt_crossings_desc_default(pt_crossings_desc *d);   /* pointers NULL, direction 0, tmin 0, tmax +inf, AUTO */
pt_status pt_crossings_device(pt_scene *scene, const pt_crossings_desc *desc, uint64_t n, float *device_ms /* may be NULL */);

/* ---- path-traced radiance for caller-supplied rays ------------------------------------------------------------------------------------
 * pt_radiance_device(scene, desc, n, device_ms) answers "what radiance arrives along these rays?" for n rays that lie in DEVICE memory, into
 * DEVICE memory: the estimator of pt_render started from the caller's rays instead of the camera of raygen.rgen:51-57 -- a perspective,
 * fisheye or thin-lens camera, a light probe, a bake, a batch of training rays.  The rays are put into the path queues of the wavefront
 * pipeline by a kernel; the extend, shade and shadow kernels pt_render runs (every scene class: LDS, HBM, the 8-wide tree, both two-level
 * kernels) carry the paths, one slot per (ray, sample); a kernel reduces the samples into the caller's arrays.  pt_render is untouched.
 *
 * Arithmetic: binary32, every operation rounded on its own, no contraction, denormals kept.  For ray i and sample s = 0 .. spp-1:
 *   Seed    with d_seeds: d_seeds[i*spp + s], verbatim.  Otherwise a + b (mod 2^32) with (a, b) = pcg2d((uint32)(i + index_base), m)
 *           (common.glsl:21-31) and m = s + (uint32)((int32)spp * frame) + 1, make_seed's m.  i is the ray's position in the whole call,
 *           never its position in a chunk.
 *   Path    sample s owns an accumulator c_s that starts at +0; weight = 1; the ray is ray i, taken as given (not normalised, as pt_trace
 *           takes it) and the same for every sample: the caller supplies jitter by supplying more rays.  From there the loop is
 *           raygen.rgen:62-83 exactly as pt_render runs it from a camera ray: a miss adds weight * env and ends the path; a hit adds
 *           weight * Ke (with PT_RADIANCE_NEE at depth 0 only); with PT_RADIANCE_NEE the hit then takes the light sample and shadow ray of
 *           PT_PIPELINE_WAVEFRONT_NEE (three random numbers, drawn before the bounce's two; none at the path's last hit); the bounce follows.
 *   Reduce  C = +0; for s ascending C = C + c_s; mean = C / (float)spp.  d_moment2 the same over c_s * c_s per channel.  This is NOT
 *           pt_render's single accumulator across the samples of a pixel (which adds every term of every sample to one sum); the two are
 *           the same at spp = 1.
 *   Store   without PT_RADIANCE_ACCUMULATE d_radiance[i] = mean.  With it (mean + old * (float)frame) / (float)(frame + 1), the film's
 *           blend; the old value is not read when frame == 0 (+0 stands for it).  d_moment2 follows the same rule.
 *
 * Execution.  Blocking.  Everything runs on the context's stream, behind the work already queued there.  Per chunk of desc.chunk_rays rays:
 * one generate launch, max_depth rounds of (extend, shade [, shadow extend, shadow add]) through one pipeline, one resolve launch; nothing is
 * polled, so a chunk whose paths have all ended still launches its remaining (empty) rounds.  *device_ms (nullable): first kernel to last.
 * pt_stats: rays grows by the closest-hit and shadow queries traced, exactly as pt_render counts them for the same estimator; paths by
 * n * spp; rounds, launches_extend, launches_shade, launches_other by what ran; extend_variant is the kernel that ran.  A scene that lost its
 * trees is repaired first, as pt_trace does.  n == 0 is PT_OK and launches nothing.
 *
 * Workspace: a chunk's slots (rays x spp) at 132 B each -- two path queues, hit records, instance words, accumulators -- plus 64 B per slot
 * for the shadow queue from the first PT_RADIANCE_NEE call on, belong to the CONTEXT: made by the first call, only growing, counted against
 * pt_tuning.mem_budget_mb (PT_ERR_OOM when a chunk does not fit: nothing is launched, the context stays usable and a smaller chunk_rays
 * works), freed by pt_ctx_destroy; pt_radiance_workspace_bytes reports the bytes held.  chunk_rays = 0 takes
 * max(64, PT_RADIANCE_DEFAULT_CHUNK_SLOTS / spp) rays, rounded up to a multiple of 64 and capped by n; a chunk never exceeds 2^30 slots.
 * PT_RADIANCE_DEFAULT_CHUNK_SLOTS is 2^24 slots (2.1 GiB, 3.1 GiB with the shadow queue, and only for calls that large): of the chunks
 * 2^18 .. 2^24 slots swept on the MI355X over the 1920 x 1080 camera rays at 8 samples, depth 8 (scripts/probe_radiance_device.py,
 * profiles/radiance_device_probe.json) the largest was the fastest on both scenes and no smaller one lay within its spread -- Cornell box
 * 4.72 ms at 2^20, 3.23 at 2^22, 2.95 at 2^23, 2.76 at 2^24; 1 M-triangle soup 52.0 / 27.0 / 21.0 / 18.3 ms: every chunk pays its rounds'
 * launches and ends each round in a tail in which the extend kernel's persistent waves run out of rays.  Nothing beyond 2^24 was swept; a
 * caller short of memory names a smaller chunk_rays.
 *
 * The single-kernel form.  PT_RADIANCE_FUSED runs the paths of a chunk through ONE persistent kernel, PT_PIPELINE_FUSED's, started from the
 * caller's rays: a lane keeps its path in registers and LDS from the given ray to the path's end and HBM sees one 16-B accumulator per slot.
 * Seed / Path / Reduce / Store above hold word for word: d_radiance and d_moment2 have the same bits in both forms, for both estimators, with
 * and without d_seeds, with PT_RADIANCE_ACCUMULATE; pt_stats.rays and .paths grow by the same amounts.  It applies to the single-level class
 * of PT_PIPELINE_FUSED (the same rule decides): a scene without instances whose BVH4, triangles and shading tables live in LDS
 * (PT_EXTEND_LDS plan, no stack spill, tables <= 16 KB), tmin > 0, desc.extend == PT_EXTEND_AUTO; the plain estimator and PT_RADIANCE_NEE;
 * pair-leaf trees and leaves of up to four (pt_tuning.pair_leaves = 0).  Everywhere else PT_RADIANCE_FUSED is PT_ERR_UNSUPPORTED with nothing
 * launched or written (the text names the class).  PT_RADIANCE_AUTO takes the single-kernel form where it applies AND won the measurements
 * of DESIGN.md section 25 for that estimator -- on the MI355X it won every measured shape, 1.1x to 2.4x, for both estimators, so AUTO takes it
 * wherever it applies -- the wavefront form everywhere else (also where the single-kernel form's workspace does not fit the budget), and is
 * never an error the call would not be without the flag.  Both bits together: PT_ERR_INVALID_ARG.  With neither bit the call is what it was: same kernels, same workspace, same pt_stats
 * fields.  The value 4 is no flag: it stays an unknown bit (PT_ERR_INVALID_ARG).
 * pt_stats under either bit: pipeline = PT_PIPELINE_FUSED, or PT_PIPELINE_WAVEFRONT / _WAVEFRONT_NEE, for the form that ran (without the
 * bits the field is not touched).  The single-kernel form adds, per chunk, one to each of rounds, launches_extend (the fused launch) and
 * launches_other (the resolve), nothing to launches_shade; extend_variant = PT_EXTEND_LDS.
 * Its workspace is a set of its own that belongs to the context like the other: exactly
 *     16 * C * spp + 1024 bytes,   C = the chunk's rays = min(up64(chunk_rays or the automatic chunk), up64(n)), up64 = rounded up to 64
 * (one accumulator per slot and the kernel's eight slot counters, 128 B apart), for the largest C * spp so far; made by the first such call,
 * only growing, counted against pt_tuning.mem_budget_mb together with the other sets (PT_ERR_OOM: nothing launched, the context stays usable,
 * a smaller chunk_rays works), freed by pt_ctx_destroy, included in pt_radiance_workspace_bytes.  A context that only ever runs this form
 * never allocates the 132-B-per-slot set.  chunk_rays = 0 is the rule above.
 *
 * Refusals, with nothing launched and nothing written -- PT_ERR_INVALID_ARG: NULL scene or desc; NULL d_rays6 or d_radiance with n > 0; spp
 * or max_depth outside 1..65535; unknown flag bits; PT_RADIANCE_FUSED together with PT_RADIANCE_AUTO; a nonzero reserved word; tmin, tmax or an env component not finite, or tmax <= tmin;
 * PT_RADIANCE_ACCUMULATE with frame < 0; an unknown extend value.  PT_ERR_UNSUPPORTED: PT_EXTEND_FLAT and the variants the scene has no
 * tree for (pt_trace's rules); PT_RADIANCE_FUSED outside its class.  PT_ERR_OOM: above.                                                   */
enum { PT_RADIANCE_NEE = 1u, PT_RADIANCE_ACCUMULATE = 2u, /* (4: no flag) */ PT_RADIANCE_FUSED = 8u, PT_RADIANCE_AUTO = 16u };
#define PT_RADIANCE_DEFAULT_CHUNK_SLOTS (1u << 24)
typedef struct pt_radiance_desc {
    const void *d_rays6;     /* DEVICE n x {origin.xyz, direction.xyz} f32, dense, 4-byte aligned; taken as given (not normalised), as pt_trace takes them */
    const void *d_seeds;     /* DEVICE n x spp u32: the RNG state sample s of ray i starts with, [i*spp + s]; NULL = the rule above */
    void *d_radiance;        /* DEVICE n x 3 f32, required */
    void *d_moment2;         /* DEVICE n x 3 f32, may be NULL */
    float tmin, tmax;        /* defaults 0.001, 10000 */
    float env[3];            /* default (0.7, 0.6, 0.5) */
    uint32_t spp, max_depth; /* defaults 32, 8; 1..65535 each (pt_render's limits) */
    int32_t  frame;          /* default 0 */
    uint32_t index_base;     /* default 0: ray i hashes as i + index_base */
    uint32_t flags;          /* PT_RADIANCE_* */
    uint32_t extend;         /* PT_EXTEND_*, pt_trace's rules */
    uint32_t chunk_rays;     /* rays per pass; 0 = automatic; rounded up to a multiple of 64 */
    uint32_t reserved[4];    /* must be 0 */
} pt_radiance_desc;          /* 96 bytes */
void pt_radiance_desc_default(pt_radiance_desc *d);   /* pointers NULL, the defaults above, no flags, AUTO */
pt_status pt_radiance_device(pt_scene *scene, const pt_radiance_desc *desc, uint64_t n, float *device_ms /* may be NULL */);
/* the device bytes the context holds for pt_radiance_device (0 before the first call) */
pt_status pt_radiance_workspace_bytes(const pt_ctx *ctx, uint64_t *bytes);

/* ---- multi-GPU: assembling the presented image of a tile-sharded render ---------- */
/* The reference renders on physical device 0 (main.cpp:105) and copies its storage image to the swapchain
 * (main.cpp:661-667).  Here N ranks -- processes or host threads, one context and one GPU each -- render the
 * interleaved 8x8 tiles of one image (pt_params.rank / .world); pt_film_present stands in for that copy: ONE RCCL
 * gather of the packed tiles to the root per presented image (W*H*12/N bytes per rank over xGMI), written to a
 * separate image, so every rank's accumulation film stays valid for further progressive frames.
 * RCCL is loaded at run time (dlopen) by the first pt_comm_* call: PT_ERR_UNSUPPORTED when it is not installed. */
typedef struct pt_comm pt_comm;
typedef struct pt_unique_id { char internal[128]; } pt_unique_id; /* = ncclUniqueId */
/* One rank makes the id (ncclGetUniqueId) and hands the 128 bytes to the others by any means (the launcher's
 * store, MPI, a file); then every rank creates its communicator (ncclCommInitRank; collective: returns when all
 * `world` ranks have called it).  One communicator per context.                                                   */
pt_status pt_comm_unique_id(pt_unique_id *id);
pt_status pt_comm_create(pt_ctx *ctx, const pt_unique_id *id, uint32_t world, uint32_t rank, pt_comm **out);
pt_status pt_comm_ranks(const pt_comm *comm, uint32_t *n); /* ncclCommCount: the ranks RCCL actually connected */
void pt_comm_destroy(pt_comm *comm);
/* Called by every rank once per presented image, with the film it rendered as (rank, world) of the communicator.
 * d_image: DEVICE memory for width*height*3 floats on the root (ignored elsewhere).  Blocking.               */
pt_status pt_film_present(pt_film *film, pt_comm *comm, uint32_t root, float *d_image);
/* The two kernels of that path alone (no communicator): a rank's tiles <-> a dense device buffer
 * [tile][64 pixels][rgb], tiles in row-major order of the tile grid.  pt_film_tile_count gives its length / 192.  */
pt_status pt_film_tile_count(const pt_film *film, uint32_t rank, uint32_t world, uint32_t *n_tiles);
pt_status pt_film_pack_tiles(pt_film *film, uint32_t rank, uint32_t world, float *d_packed);
pt_status pt_film_unpack_tiles(pt_film *film, uint32_t rank, uint32_t world, const float *d_packed, float *d_image);

/* ---- multi-GPU: gathering a film's planes into a FILM on the root, so that the film passes run on a sharded render ----------------------
 * pt_film_present moves the radiance plane into a bare image.  pt_film_present_planes moves any set of the planes a film can have -- the
 * radiance C, the six guide planes of pt_film_enable_aov, M, L, K, Q -- and lands them in the planes of another film, `dst`, on the root:
 * dst is then a film like one rendered on a single device, and pt_film_denoise, _denoise_variance, _denoise_history, pt_film_reproject,
 * _reproject_motion, pt_film_upsample and pt_render_adaptive's convergence query run on it unchanged.
 *
 * THE PACKED LAYOUT (the contract of the three calls below, and of distributed.py's numpy mirrors):
 *   - Data moves as 32-bit words and no arithmetic touches a value: NaN payloads, -0.0, denormals and the id plane's 0xFFFFFFFF arrive as
 *     they left.
 *   - The buffer holds the tiles of rank `rank` of `world` -- tile (tx, ty) belongs to rank (tx + ty) % world -- row by row over the tile
 *     grid, the order of pt_film_pack_tiles; pt_film_tile_count gives their number.
 *   - Per tile there is ONE record of 64 * S words, S the words per pixel of the named set (pt_film_planes_words: 3 .. 25).
 *   - Inside a record the named planes come in this fixed order: C, albedo, normal, emission, depth, alpha, id, M, L, K, Q.
 *   - Each plane is a block [64 pixels][channels]; pixel p of tile (tx, ty) is (8*tx + (p & 7), 8*ty + (p >> 3)).
 *   - A pixel outside the image packs as zero words; unpack skips it.
 *   - With planes == PT_PLANES_FILM the buffer equals pt_film_pack_tiles's output byte for byte.
 *
 * pt_film_pack_planes: the named planes of `film`'s tiles of (rank, world) into d_packed, DEVICE memory of tiles * 64 * S words.  Blocking.
 * pt_film_unpack_planes: such a buffer into dst's own planes, film-owned or caller-owned alike.  It writes exactly the pixels of that rank's
 * tiles and touches nothing else; when PT_PLANES_FILM is named it also writes those pixels' bgra8 from the new C by k_resolve's clamp and
 * quantise rule with A = 255 (the rule pt_film_reproject states).  Blocking.
 *
 * pt_film_present_planes(film, comm, root, planes, dst, device_ms): every rank of the communicator calls it with the film it rendered as
 * (rank, world) of the communicator and the same root and planes.  One pack launch per rank, ONE RCCL group of ncclSend / ncclRecv of the
 * packed buffers (the group shape of pt_film_present), one unpack launch on the root over all ranks' records.  On the root every named plane
 * of dst is overwritten completely -- every pixel belongs to exactly one rank -- and dst gets its bgra8 as under unpack; with
 * PT_PLANES_MOMENTS dst also takes over the `frames` record of the root's film, so that pt_film_denoise_variance(frames = 0) works on it.
 * `film` on every rank, the planes of dst that are not named and pt_stats stay as they were.  dst is read on the root only and ignored
 * elsewhere.  Blocking; runs on the context's stream, ordered after the work already queued there.  device_ms (may be NULL): the device time
 * on this rank's stream from the pack to the last unpack; on a rank that is not the root, from the pack to the send.
 * The staging buffers (a rank's records, on the root all ranks' records, and the tile lists) belong to the communicator, are keyed by
 * (film size, root, planes), are replaced only when that key changes and are freed by pt_comm_destroy: a second call with the same key
 * allocates nothing.  They are NOT counted against pt_tuning.mem_budget_mb.
 *
 * PT_ERR_INVALID_ARG -- nothing is launched and no collective is joined: NULL film or comm; planes == 0 or with bits outside
 * PT_PLANES_ALL; root >= the communicator's world; a film of another context than the communicator's; a film rendered as another
 * (rank, world) than the communicator's (pt_film_present's rule); a film that lacks a named plane (no guide buffers, no M, L, K or Q);
 * and on the root a dst that is NULL, is `film` itself, has another size or context, or lacks a named plane.  The standalone pack and
 * unpack refuse the same argument errors (and a NULL buffer, world == 0, rank >= world).
 * As with pt_film_present, THE RANKS MUST AGREE ON SUCCESS BEFORE THE CALL: a rank that refuses, or that failed earlier, while the others
 * send leaves them waiting in the collective.  Check on every rank what can be checked (the planes exist, dst on the root) and exchange the
 * outcome first; host/pt_main.cpp's Agreement is the pattern.                                                                          */
enum { PT_PLANES_FILM = 1u,      /* C: 3 words per pixel */
       PT_PLANES_GUIDES = 2u,    /* the six planes of pt_film_enable_aov: albedo 3, normal 3, emission 3, depth 1, alpha 1, id 2 */
       PT_PLANES_MOMENTS = 4u,   /* M: 3 */
       PT_PLANES_HISTORY = 8u,   /* L: 1 */
       PT_PLANES_COUNTS = 16u,   /* K: 1 */
       PT_PLANES_MOTION = 32u,   /* Q: 4 */
       PT_PLANES_ALL = 63u };
pt_status pt_film_planes_words(const pt_film *film, uint32_t planes, uint32_t *words_per_pixel);   /* S: 3 .. 25; a function of `planes` alone */
pt_status pt_film_pack_planes(pt_film *film, uint32_t rank, uint32_t world, uint32_t planes, void *d_packed);
pt_status pt_film_unpack_planes(pt_film *dst, uint32_t rank, uint32_t world, uint32_t planes, const void *d_packed);
pt_status pt_film_present_planes(pt_film *film, pt_comm *comm, uint32_t root, uint32_t planes,
                                 pt_film *dst /* root only; ignored elsewhere */, float *device_ms /* may be NULL */);

/* Device memory for the buffers a caller hands to the library (pt_film_create_external, pt_film_present), for hosts
 * that do not link HIP themselves (host/pt_main.cpp is plain g++): hipMalloc / hipFree / blocking copies either way,
 * ordered after the context's stream.                                                                            */
pt_status pt_device_alloc(pt_ctx *ctx, size_t bytes, void **out);
pt_status pt_device_free(pt_ctx *ctx, void *device_ptr);
pt_status pt_device_read(pt_ctx *ctx, const void *device_src, void *host_dst, size_t bytes);
pt_status pt_device_write(pt_ctx *ctx, void *device_dst, const void *host_src, size_t bytes); /* (API version 5) blocking host->device copy */

/* ---- statistics ------------------------------------------------------------------------ */
typedef struct pt_stats {
    uint64_t rays;             /* closest-hit queries (= traceRayEXT calls) since last reset, exact */
    uint64_t paths;            /* samples started                                                   */
    uint32_t rounds;           /* wavefront rounds executed                                         */
    uint32_t launches_extend, launches_shade, launches_other;
    float    ms_total;         /* device time of pt_render calls (first kernel .. last kernel)      */
    float    ms_extend, ms_shade; /* summed kernel times; only with PT_FLAG_PROFILE                 */
    uint32_t extend_variant;   /* PT_EXTEND_* that actually ran                                     */
    uint64_t nodes_visited;    /* BVH4 nodes fetched (128 B each) -- only with PT_FLAG_COUNT_VISITS  */
    uint64_t tris_tested;      /* triangles tested                -- only with PT_FLAG_COUNT_VISITS  */
    uint32_t frames_in_flight; /* shape of the last pt_render / pt_render_prepare                    */
    uint32_t sample_groups;
    /* wave64 steps of the single-level extend kernel (PT_FLAG_COUNT_VISITS): how often a WAVE ran the node
     * code / the triangle code.  nodes_visited / (64 * node_steps) is the lane occupancy of the node phase,
     * tris_tested / (64 * tri_steps) that of the triangle tests.                                        */
    uint64_t node_steps, tri_steps;
    /* batches whose sample-group term log filled up and that were rendered again with one group (exact either way) */
    uint32_t redone_batches;
    uint32_t pipelines;        /* concurrent wavefront pipelines (streams) of the last pt_render */
    /* PT_FLAG_COUNT_VISITS, single-level extend kernel: how often a WAVE executed the other blocks of the kernel --
     * the refill block, one iteration of the stack-pop loop, the hit block of the triangle test (the true divide),
     * the block that writes a hit record, one iteration of the outer loop.  With the per-block instruction counts
     * of the shipped ISA (bench.py) these give the VALU instructions a launch issues without a PMC run.     */
    uint64_t wave_refills, wave_pops, wave_hit_blocks, wave_finishes, wave_iterations;
    /* (API version 3) PT_FLAG_COUNT_VISITS: LANES inside those wave-level steps -- leaf_lanes: lanes that ran a leaf step (one
     * triangle, or a fan pair tested together: tris_tested counts two for those, so tris_tested / tri_steps can exceed 64
     * and is not a lane count); pop_lanes / hit_lanes: lanes in the pop iterations / divide blocks; the two-level kernel's
     * instance-entry block: enter_steps wave executions with enter_lanes lanes.  lanes / (64 * steps) is the occupancy
     * of a block; weighted by the blocks' instruction counts it gives the active lanes per VALU instruction.        */
    uint64_t leaf_lanes, pop_lanes, hit_lanes, enter_steps, enter_lanes;
    /* device bytes the last pt_render / pt_render_prepare holds for its wavefront workspace: the film's queues, hit
     * records, radiance accumulators or term logs, sort scratch and shadow queue, plus the context's traversal-stack
     * spill area (the scene and the film images themselves are not included: pt_scene_info.device_bytes, W*H*16)   */
    uint64_t workspace_bytes;
    uint32_t pipeline;         /* (API version 5) PT_PIPELINE_* the last pt_render / pt_render_prepare ran (never PT_PIPELINE_AUTO) */
    uint32_t tail_samples;     /* fused pipeline: samples per pixel and frame traced as one-sample tail slots behind a head slot (0: none) */
    uint64_t rays_culled;      /* of `rays`: camera rays of pixels outside the projection of the scene's box, which are resolved as the misses they
                                * are without a walk (pt_tuning.cull); the reference traces them (raygen.rgen:62), so they count */
} pt_stats;
pt_status pt_get_stats(pt_ctx *ctx, pt_stats *stats);
pt_status pt_reset_stats(pt_ctx *ctx);
/* (API version 6) Where the fused kernel's instructions go.  A render with pipeline = PT_PIPELINE_FUSED and PT_FLAG_COUNT_VISITS (single-level
 * scenes with pair leaves; never timed) runs the instrumented twin of the kernel: every block of its loop -- the restatement of raygen.rgen:41-91 --
 * counts how often a WAVE executed it and how many LANES were inside.  waves_lanes receives 2 * n_blocks words {wave executions, lanes} in the
 * order of pt_fused_block, summed since pt_reset_stats.  With the blocks' instruction counts in the shipped ISA (scripts/isa_regions.py,
 * profiles/isa_valu_model.json) these give the kernel's VALU wave-instructions and its active lanes per instruction block by block.          */
enum pt_fused_block {
    PT_FB_ITER = 0,  /* one pass of the outer loop                                              */
    PT_FB_SHADE,     /* the shade block ran (lanes: with a finished ray, or asking for a slot)  */
    PT_FB_HIT,       /* ... state loads of the lanes with a hit record                          */
    PT_FB_MISS,      /* ... miss.rmiss:8-12: counted lanes only -- the product kernel has no    */
                     /*     code of its own for it (a miss is a record of the shade table, run  */
                     /*     by PT_FB_SURFACE's instructions)                                    */
    PT_FB_SURFACE,   /* ... closesthit.rchit:33-41, 50-53: material, emission                   */
    PT_FB_ADD,       /* ... raygen.rgen:76 color += weight * emission                           */
    PT_FB_BOUNCE,    /* ... closesthit.rchit:56-57 + raygen.rgen:77-80                          */
    PT_FB_NEXT,      /* ... path ended: next sample or slot complete (raygen.rgen:43, 62, 81)   */
    PT_FB_DONE,      /* ... the slot's radiance goes to memory                                  */
    PT_FB_HANDOUT,   /* slot hand-out ran (lanes: asking for a slot)                            */
    PT_FB_DRAW,      /* ... the wave drew a batch of slots                                      */
    PT_FB_TAKE,      /* ... lanes that took a slot                                              */
    PT_FB_CULLED,    /* ... of them: finished here, the pixel cannot see the scene              */
    PT_FB_PRIMARY,   /* camera ray: the sample's seed (raygen.rgen:47-48)                       */
    PT_FB_SETUP,     /* state to LDS, ray set-up for the walk                                   */
    PT_FB_NODE,      /* one BVH4 node step                                                      */
    PT_FB_POP,       /* one iteration of the stack-pop loop                                     */
    PT_FB_LEAF,      /* one leaf step (a triangle or a fan pair)                                */
    PT_FB_DIV,       /* ... its divide block                                                    */
    PT_FB_FINISH,    /* a walk ended                                                            */
    PT_FB_TRACE,     /* (no code of its own) once per pass with a walk: the lanes that trace    */
    PT_FB_SPAWN,     /* the steps a bounce and a camera ray share: two rand, one square root    */
    PT_FB_PTARGET,   /* camera ray: pixel + jitter -> target - origin (raygen.rgen:51-56)       */
    PT_FB_PDIR,      /* camera ray: normalize (raygen.rgen:57)                                  */
    PT_FB_POPTOP,    /* a node step without a hit child takes the stack's top entry from a register */
    PT_FB_SKIP,      /* (no code of its own) lanes whose walk left out the leaf of the triangle their ray started on */
    PT_FB_COUNT
};
pt_status pt_get_block_counts(pt_ctx *ctx, uint64_t *waves_lanes, uint32_t n_blocks /* <= 32 */);

#ifdef __cplusplus
}
#endif
#endif
