// aov.hip -- pt_render_aov: guide buffers of the FIRST hit (albedo, normal, emission, depth, alpha, id), include/pt_api.h.
//
// For every frame F of the call, every owned pixel and s = 0 .. spp - 1: seed = make_seed(x, y, s, F, spp), the camera ray of
// raygen.rgen:51-57 from it (the very ray pt_render starts that sample with), its closest hit.  A sample's values are Kd, the
// normal k_shade uses, Ke, t and 1 -- all 0 on a miss; a frame's value is ((0 + v_0) + v_1 ...) / spp and goes into the plane as
// (value + old * F) / (F + 1), `old` not read for F = 0 (k_resolve's blend).  id = {prim, inst} of sample 0 of the call's last frame.
//
// Two forms, same bits:
//   queue form (every scene)     k_aov_generate writes a chunk's camera rays in the extend kernels' input layout (ray = pixel of the
//                                chunk * spp + sample, pixels in tile order), ptw_launch_extend traces them like pt_trace does, and
//                                k_aov_reduce, one thread per pixel, folds the spp hit records in order.
//   single kernel (k_aov_fused)  scenes of the compact LDS class (the Cornell box): a persistent kernel with BVH4, triangles and the
//                                per-triangle guide records in LDS.  A wave takes an 8x8 tile, a lane one pixel of it; the lane walks
//                                its samples one after the other (compact_node_step / pair_leaf.h: k_extend_lds7p's walk) with the
//                                frame's eleven sums in registers and blends them into the planes at the end of each frame.
#include "wavefront_host.h"

#include <algorithm>

#define PT_EXTEND_TEMPLATES_ONLY
#include "extend_kernel.h"  // compact_node_step, slab_setup, the LDS node layout

namespace {
using namespace ptw;
#include "guided_kernel.h"  // AovPlanes, Guide, guide_add / guide_blend / guide_load / guide_store: shared with pt_render_guided's reduce (guided.hip)

struct AovConst {
    ptm::Camera cam;
    float tmin, tmax;
    uint32_t width, height, spp;
    FastDiv div_spp;
    // single-kernel form: every camera ray of a pixel outside the pixel rectangle cull = {x0, y0, x1, y1} misses the scene's box (render.hip
    // subject_rect, the proof behind RenderConst::cull), so its samples are finished as the misses they are without a walk
    uint32_t cull_on;
    int32_t cull[4];
};
constexpr size_t AOV_RAY_BYTES = sizeof(float4) + sizeof(float2) + sizeof(float4) + sizeof(uint32_t);  // rayA, rayB, hit, hit_inst
constexpr size_t AOV_MAX_CHUNK_RAYS = (size_t)1 << 26;                                                  // 2.75 GB of them at most, whatever the budget
constexpr uint32_t AOV_NEXT_TILE = 32;  // word of Aov::d_count the single-kernel form hands tiles out of (a line of its own)

__device__ __forceinline__ void tile_pixel(const uint32_t *__restrict__ tiles, uint32_t pix, uint32_t &px, uint32_t &py)
{
    const uint32_t g = tiles[pix >> 6];  // tile x | tile y << 16
    px = (g & 0xFFFFu) * 8u + (pix & 7u);
    py = (g >> 16) * 8u + ((pix >> 3) & 7u);
}

// ---- queue form ------------------------------------------------------------------------------------------------------------
// the spp camera rays of every pixel of a chunk of tiles (pixels beyond the image's edge get theirs too: ordinary rays, whose
// records k_aov_reduce never reads and which are not counted)
__global__ __launch_bounds__(TB) void k_aov_generate(AovConst ac, const uint32_t *__restrict__ tiles, uint32_t n_rays, int32_t frame,
                                                     float4 *__restrict__ rayA, float2 *__restrict__ rayB, uint32_t *__restrict__ count)
{
    for (uint32_t r = blockIdx.x * TB + threadIdx.x; r < n_rays; r += gridDim.x * TB) {
        const uint32_t pix = ac.div_spp.div(r), s = r - pix * ac.spp;
        uint32_t px, py;
        tile_pixel(tiles, pix, px, py);
        uint32_t seed = ptm::make_seed(px, py, s, frame, ac.spp);
        ptm::f3 org, dir;
        ptm::primary_ray(ac.cam, px, py, seed, org, dir);
        ptm::st_stream<true>(rayA + r, make_float4(org.x, org.y, org.z, dir.x));
        ptm::st_stream<true>(rayB + r, make_float2(dir.y, dir.z));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = n_rays;  // what the extend kernel walks
}

// One thread per pixel of the chunk: its spp hit records in sample order.  tri4 / rec64 are the tables of the tree that was walked
// ({v, n.x} {v, n.y} {v, n.z} {brdf, emits}: k_shade's 64-B record carries the normal), faces the scene's Kd / Ke in primitive order.
// INST: the normal goes to world space as in k_shade<INST> -- from the (instance, triangle) table, or by the inverse transpose.
template <bool INST>
__global__ __launch_bounds__(TB) void k_aov_reduce(AovConst ac, const uint32_t *__restrict__ tiles, uint32_t n_pix, int32_t frame, int last_frame,
                                                   const float4 *__restrict__ hit, const uint32_t *__restrict__ hit_inst,
                                                   const float4 *__restrict__ tri4, const float4 *__restrict__ rec64,
                                                   const float *__restrict__ faces, const float4 *__restrict__ inst6,
                                                   const float4 *__restrict__ inst_frame, const uint32_t *__restrict__ inst_id, uint32_t n_tris,
                                                   AovPlanes planes, unsigned long long *stats, unsigned long long n_valid_rays)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && stats) atomicAdd(stats + PT_STAT_RAYS, n_valid_rays);  // the chunk's rays, once per launch
    const uint32_t pix = blockIdx.x * TB + threadIdx.x;
    if (pix >= n_pix) return;
    uint32_t px, py;
    tile_pixel(tiles, pix, px, py);
    if (px >= ac.width || py >= ac.height) return;
    Guide sum = {};
    uint2 id = make_uint2(PT_MISS, PT_MISS);
    for (uint32_t s = 0; s < ac.spp; s++) {
        const size_t r = (size_t)pix * ac.spp + s;
        const float4 h = ptm::ld_stream<true>(hit + r);
        const uint32_t pos = __float_as_uint(h.x);
        Guide v = {};
        if (pos != PT_MISS) {
            const uint32_t prim = __float_as_uint(tri4[3 * (size_t)pos].w);
            const float *f = faces + 6 * (size_t)prim;
            ptm::f3 nrm = { rec64[4 * (size_t)pos + 0].w, rec64[4 * (size_t)pos + 1].w, rec64[4 * (size_t)pos + 2].w };
            uint32_t inst = 0u;
            if (INST) {
                const uint32_t ip = hit_inst[r];
                inst = inst_id[ip];
                if (inst_frame) {
                    const float4 f0 = inst_frame[2 * ((size_t)ip * n_tris + pos)];
                    nrm = { f0.x, f0.y, f0.z };
                } else {
                    const float4 i0 = inst6[6 * (size_t)ip + 3], i1 = inst6[6 * (size_t)ip + 4], i2 = inst6[6 * (size_t)ip + 5];
                    const float nx = (i0.x * nrm.x + i1.x * nrm.y) + i2.x * nrm.z;
                    const float ny = (i0.y * nrm.x + i1.y * nrm.y) + i2.y * nrm.z;
                    const float nz = (i0.z * nrm.x + i1.z * nrm.y) + i2.z * nrm.z;
                    const float l = ptm::fsqrt((nx * nx + ny * ny) + nz * nz);
                    nrm = { ptm::fdiv(nx, l), ptm::fdiv(ny, l), ptm::fdiv(nz, l) };
                }
            }
            v = { f[0], f[1], f[2], nrm.x, nrm.y, nrm.z, f[3], f[4], f[5], h.y, 1.0f };
            if (s == 0u) id = make_uint2(prim, inst);
        }
        guide_add(sum, v);
    }
    const size_t o = (size_t)py * ac.width + px;
    Guide acc = {};
    if (frame != 0) acc = guide_load(planes, o);
    guide_blend(acc, sum, (float)ac.spp, frame);
    guide_store(planes, o, acc);
    if (last_frame) planes.id[o] = id;
}

// ---- single-kernel form ------------------------------------------------------------------------------------------------------
// The class of k_extend_lds7 / _lds7p (extend_kernel.h COMPACT: 14-bit child codes, one-dword stack entries, exact stack bound in
// LDS, tmin > 0).  Dynamic LDS, from byte 0: nodes (160 B each) | three permuted triangle copies | guide records 3 x float4 per leaf
// position {n, bits(prim)} {Kd, Ke.r} {Ke.gb, 0, 0} | stack (compact_stack_bytes: [lds_stack + 1][TB] dwords, LaneStack).
// A wave owns one tile at a time (one atomic per 64 pixels x spp x frames rays).  Its lanes run their samples independently -- a lane
// whose walk ended starts its next sample once AOV_START_IDLE lanes wait, as k_extend refills -- and meet again at the end of a frame.
constexpr int AOV_START_IDLE = 16;
// 107 VGPRs, no scratch: four waves per SIMD.  Asking the compiler for five spills four registers into the walk; five without spills by
// keeping the frame's sums in LDS ([11][TB] floats) measured within the spread of this form at 1080p, one and sixteen frames per call
// (DESIGN.md section 12), so the sums stay in registers.
#ifndef PT_AOV_WAVES
#define PT_AOV_WAVES 4  // waves per SIMD asked of the compiler
#endif
template <bool PAIRS>
__global__ __launch_bounds__(TB, PT_AOV_WAVES) void k_aov_fused(AovConst ac_arg, const uint32_t *__restrict__ tiles, uint32_t n_tiles, int32_t frame0, uint32_t n_frames,
                                                  const float4 *__restrict__ g_wide, const float4 *__restrict__ g_tri4,
                                                  const float4 *__restrict__ g_shade4, const float *__restrict__ g_faces, uint32_t n_wide,
                                                  uint32_t n_tris, AovPlanes planes_arg, uint32_t *next_tile,
                                                  unsigned long long *stats)
{
    const AovConst ac = ptm::own_sgprs(ac_arg);
    const AovPlanes planes = ptm::own_sgprs(planes_arg);
    constexpr uint32_t LEAF_BIT = C14_LEAF, DONE = C14_DONE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *s_wide = reinterpret_cast<float4 *>(smem);
    float4 *s_tri = s_wide + LDS_NODE_F4 * (size_t)n_wide;
    float4 *s_rec = s_tri + 9 * (size_t)n_tris;
    lds_stage_nodes<TB, true>(s_wide, g_wide, n_wide);
    lds_stage_tris<TB>(s_tri, g_tri4, n_tris);
    for (uint32_t pos = threadIdx.x; pos < n_tris; pos += TB) {
        const float4 n = g_shade4[3 * (size_t)pos];
        const float prim_bits = g_tri4[3 * (size_t)pos].w;
        const float *f = g_faces + 6 * (size_t)__float_as_uint(prim_bits);
        s_rec[3 * pos + 0] = make_float4(n.x, n.y, n.z, prim_bits);
        s_rec[3 * pos + 1] = make_float4(f[0], f[1], f[2], f[3]);
        s_rec[3 * pos + 2] = make_float4(f[4], f[5], 0.f, 0.f);
    }
    __syncthreads();
    const float4 *wide = s_wide, *tri4 = s_tri;
    LaneStack<TB> stk((lds_u32 *)reinterpret_cast<uint32_t *>(s_rec + 3 * (size_t)n_tris) + threadIdx.x);
    const int lane = threadIdx.x & 63;
    const float tmin = ac.tmin, tmax = ac.tmax;
    const float fspp = (float)ac.spp;
    unsigned long long n_rays_wave = 0, n_cull_wave = 0;

    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(next_tile, 1u);
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        if (t >= n_tiles) break;
        uint32_t px, py;
        tile_pixel(tiles, t * 64u + (uint32_t)lane, px, py);
        const bool valid = px < ac.width && py < ac.height;
        const uint32_t o = py * ac.width + px;  // (a film has fewer than 2^28 pixels)
        const bool culled = ac.cull_on && ((int32_t)px < ac.cull[0] || (int32_t)px > ac.cull[2] || (int32_t)py < ac.cull[1] || (int32_t)py > ac.cull[3]);
        n_rays_wave += (unsigned long long)__popcll(__ballot(valid)) * ac.spp * n_frames;
        n_cull_wave += (unsigned long long)__popcll(__ballot(valid && culled)) * ac.spp * n_frames;
        for (uint32_t k = 0; k < n_frames; k++) {
            const int32_t frame = frame0 + (int32_t)k;
            Guide sum = {};
            uint32_t s = valid && !culled ? 0u : ac.spp;  // the lane's next sample (a culled pixel's samples all miss: zeros, counted above)
            bool have = false;
            ptm::f3 inv{}, invf{}, on{}, of{}, orgp{};
            ptm::RayPre pre{};
            uint32_t ax = 0, ay = 0, az = 0, tri_base = 0;
            float best_t = tmax, best_V = 0.f, best_W = 0.f, best_det = 1.f;
            uint32_t best_pos = PT_MISS, best_prim = PT_MISS;
            uint32_t cur = DONE;
            stk.clear();
            auto pop = [&](uint32_t cut) -> uint32_t {  // (cut: the cut key of best_t, extend_kernel.h)
                while (stk.has_entries()) {
                    const uint32_t e = stk.pop();
                    if (entry_within(e, cut)) return e & 0x3FFFu;
                }
                return DONE;
            };
            for (;;) {
                // ---- lanes without a ray start their next sample
                const bool wants = !have && s < ac.spp;
                const int n_idle = __popcll(__ballot(wants)), n_have = __popcll(__ballot(have));
                if (n_idle == 0 && n_have == 0) break;
                if (wants && (n_idle >= AOV_START_IDLE || n_have == 0)) {
                    uint32_t seed = ptm::make_seed(px, py, s, frame, ac.spp);
                    ptm::f3 org, dir;
                    ptm::primary_ray(ac.cam, px, py, seed, org, dir);
                    pre = ptm::ray_setup<PAIRS>(org, dir);  // (as extend_body: the per-triangle leaf loop keeps the IEEE expansion)
                    inv = { ptm::safe_inv(dir.x), ptm::safe_inv(dir.y), ptm::safe_inv(dir.z) };
                    slab_setup(org, inv, invf, on, of);
                    ax = inv.x < 0.f ? LDS_NEG_AXIS : 0u; ay = inv.y < 0.f ? LDS_NEG_AXIS : 0u; az = inv.z < 0.f ? LDS_NEG_AXIS : 0u;
                    tri_base = (uint32_t)pre.kz * 3u * n_tris;
                    orgp = { ptm::sel3(pre.kz, org.y, org.z, org.x), ptm::sel3(pre.kz, org.z, org.x, org.y), ptm::sel3(pre.kz, org.x, org.y, org.z) };
                    best_t = tmax; best_V = 0.f; best_W = 0.f; best_det = 1.f;
                    best_pos = PT_MISS; best_prim = PT_MISS;
                    cur = 0u;  // root
                    stk.clear();
                    have = true;
                }
                // ---- node phase (k_extend's inner loop and its yield to the lanes that wait with a leaf)
                bool do_node = have && !(cur & LEAF_BIT);
                const int n_walk = __popcll(__ballot(have));
                while (do_node) {
                    cur = compact_node_step<TB>(wide, cur, inv, invf, on, of, ax, ay, az, tmin, best_t, stk, [&](uint32_t, uint32_t kcut) { return pop(kcut); });
                    do_node = !(cur & LEAF_BIT);
                    if (__popcll(__ballot(do_node)) * 6 < n_walk) break;
                }
                // ---- leaf phase
                if (have) {
                    if (cur != DONE && (cur & LEAF_BIT)) {
                        const uint32_t first = cur & 0x7FFu;
                        if (PAIRS) {
                            const bool two = ((cur >> 11) & 3u) != 0u;
                            ptl::pair_leaf_test(tri4, (size_t)tri_base + 3 * (size_t)first, two, first, pre, orgp, tmin, tmax,
                                                [&](float t_, float V, float W, float det, uint32_t pos, uint32_t) {
                                                    ptl::closer_single_level(tri4, tri_base, t_, V, W, det, pos, best_t, best_V, best_W, best_det, best_pos);
                                                },
                                                [] {});
                        } else {
                            const uint32_t cnt = ((cur >> 11) & 3u) + 1u;
                            for (uint32_t j = 0; j < cnt; j++) {
                                const uint32_t pos = first + j;
                                const size_t ti = (size_t)tri_base + 3 * (size_t)pos;
                                const float4 a = tri4[ti + 0], b = tri4[ti + 1], c = tri4[ti + 2];
                                float t_, V, W, det;
                                if (ptm::tri_test_perm(pre, orgp, { a.x, a.y, a.z }, { b.x, b.y, b.z }, { c.x, c.y, c.z }, tmin, tmax, t_, V, W, det, nullptr)) {
                                    const uint32_t prim = __float_as_uint(a.w);
                                    if (t_ < best_t || (t_ == best_t && prim < best_prim)) {
                                        best_t = t_; best_V = V; best_W = W; best_det = det; best_pos = pos; best_prim = prim;
                                    }
                                }
                            }
                        }
                        cur = pop(pop_cut(best_t));
                    }
                    if (cur == DONE) {  // the sample's first hit is known
                        Guide v = {};
                        if (best_pos != PT_MISS) {
                            const float4 r0 = s_rec[3 * best_pos + 0], r1 = s_rec[3 * best_pos + 1], r2 = s_rec[3 * best_pos + 2];
                            v = { r1.x, r1.y, r1.z, r0.x, r0.y, r0.z, r1.w, r2.x, r2.y, best_t, 1.0f };
                            if (s == 0u && k + 1u == n_frames) planes.id[o] = make_uint2(__float_as_uint(r0.w), 0u);  // (stored here: not carried through the walks)
                        } else if (s == 0u && k + 1u == n_frames) {
                            planes.id[o] = make_uint2(PT_MISS, PT_MISS);
                        }
                        guide_add(sum, v);
                        s++;
                        have = false;
                    }
                }
            }
            // the plane values go through memory between the frames of a call (L2 holds them): eleven registers the walks do not carry
            if (valid && culled && k + 1u == n_frames) planes.id[o] = make_uint2(PT_MISS, PT_MISS);
            if (valid) {
                Guide acc = {};
                if (frame != 0) acc = guide_load(planes, o);
                guide_blend(acc, sum, fspp, frame);
                guide_store(planes, o, acc);
            }
        }
    }
    if (lane == 0 && n_rays_wave && stats) atomicAdd(stats + PT_STAT_RAYS, n_rays_wave);
    if (lane == 0 && n_cull_wave && stats) atomicAdd(stats + PT_STAT_RAYS_CULLED, n_cull_wave);  // (pt_stats.rays_culled)
}

// this rank's 8x8 tiles, row by row (pt_render's own list before its hand-out order: pt_rank_tiles)
pt_status ensure_tiles(pt_film *f, uint32_t rank, uint32_t world)
{
    pt_film::Aov &a = f->aov;
    if (a.d_tiles && a.rank == rank && a.world == world) return PT_OK;
    std::vector<uint32_t> tiles;
    std::vector<uint64_t> prefix;
    const uint64_t valid = pt_rank_tiles(f->w, f->h, rank, world, &tiles, &prefix);
    const size_t held = a.d_tiles ? sizeof(uint32_t) * std::max<size_t>(a.n_tiles, 1) : 0;
    a.n_tiles = 0;
    const pt_status rc = pt_scratch_alloc(f->ctx, "guide-buffer workspace", { pt_buf_of(a.d_tiles, sizeof(uint32_t) * std::max<size_t>(tiles.size(), 1)) }, &a.bytes, held);
    if (rc != PT_OK) return rc;
    if (!tiles.empty()) PT_HIP(f->ctx, hipMemcpy(a.d_tiles, tiles.data(), sizeof(uint32_t) * tiles.size(), hipMemcpyHostToDevice));
    a.rank = rank; a.world = world; a.n_tiles = (uint32_t)tiles.size(); a.valid_pixels = valid;
    a.h_valid.swap(prefix);
    return PT_OK;
}

pt_status ensure_count(pt_film *f)
{
    pt_film::Aov &a = f->aov;
    if (a.d_count) return PT_OK;
    return pt_scratch_alloc(f->ctx, "guide-buffer workspace", { pt_buf_of(a.d_count, sizeof(uint32_t) * 64) }, &a.bytes, 0);
}

// Ray scratch for `rays` rays (grow only, all four or none).  Not checked against the budget here: render_aov_queues sizes the chunk to it beforehand.
pt_status ensure_rays(pt_film *f, size_t rays)
{
    pt_film::Aov &a = f->aov;
    if (rays <= a.cap_rays) return PT_OK;
    const size_t held = a.cap_rays * AOV_RAY_BYTES;
    a.cap_rays = 0;
    const pt_status rc = pt_scratch_alloc(f->ctx, "guide-buffer workspace", { pt_buf_of(a.d_rayA, sizeof(float4) * rays), pt_buf_of(a.d_rayB, sizeof(float2) * rays),
                                                                              pt_buf_of(a.d_hit, sizeof(float4) * rays), pt_buf_of(a.d_hit_inst, sizeof(uint32_t) * rays) }, &a.bytes, held);
    if (rc == PT_OK) a.cap_rays = rays;
    return rc;
}

AovPlanes planes_of(const pt_film *f)
{
    const pt_film::Aov &a = f->aov;
    return { static_cast<float *>(a.plane[PT_AOV_ALBEDO]), static_cast<float *>(a.plane[PT_AOV_NORMAL]), static_cast<float *>(a.plane[PT_AOV_EMISSION]),
             static_cast<float *>(a.plane[PT_AOV_DEPTH]), static_cast<float *>(a.plane[PT_AOV_ALPHA]), static_cast<uint2 *>(a.plane[PT_AOV_ID]) };
}

// the single-kernel form's class and launch shape
struct AovFusedPlan { size_t smem = 0; int grid = 0; bool pairs = false; };
using AovFusedFn = decltype(&k_aov_fused<true>);
AovFusedFn pick_aov_fused(bool pairs) { return pairs ? k_aov_fused<true> : k_aov_fused<false>; }
pt_status plan_aov_fused(pt_scene *s, const pt_params *p, const ExtendPlan &pl, AovFusedPlan &fp)
{
    pt_ctx *ctx = s->ctx;
    const size_t smem = pl.smem + sizeof(float4) * 3 * (size_t)s->n_tris;
    if (s->n_inst || p->extend != PT_EXTEND_AUTO || pl.variant != PT_EXTEND_LDS || pl.spill || !(p->tmin > 0.f) || smem > 64 * 1024) {
        ctx->err = "pt_render_aov: PT_PIPELINE_FUSED is for single-level scenes whose BVH4 and triangles live in LDS (the compact kernels' class: <= 24 KB, "
                   "stack bound <= 16), tmin > 0 and params.extend = PT_EXTEND_AUTO";
        return PT_ERR_UNSUPPORTED;
    }
    fp.smem = smem;
    fp.pairs = pl.pairs;
    int per_cu = 0;
    const pt_status rc = ptw_prepare_kernel(ctx, reinterpret_cast<const void *>(pick_aov_fused(pl.pairs)), TB, smem, &per_cu);
    fp.grid = ctx->num_cus * per_cu;
    return rc;
}

pt_status render_aov_fused(pt_scene *s, pt_film *f, const pt_params *p, const ExtendPlan &pl, const AovFusedPlan &fp, const AovConst &ac)
{
    pt_ctx *ctx = s->ctx;
    pt_film::Aov &a = f->aov;
    hipStream_t st = ctx->stream;
    if (a.n_tiles == 0) return PT_OK;
    PT_HIP(ctx, hipMemsetAsync(a.d_count + AOV_NEXT_TILE, 0, sizeof(uint32_t), st));
    const int grid = (int)std::min<uint32_t>((uint32_t)fp.grid, (a.n_tiles + TB / 64 - 1) / (TB / 64));  // a wave per tile at least
    hipLaunchKernelGGL(pick_aov_fused(fp.pairs), dim3(grid), dim3(TB), (uint32_t)fp.smem, st, ac, a.d_tiles, a.n_tiles, p->frame, p->frame_count, s->d_wide, s->d_tri4,
                       s->d_shade4, s->d_faces, s->n_wide, s->n_tris, planes_of(f), a.d_count + AOV_NEXT_TILE, ctx->d_stats);
    PT_HIP(ctx, hipGetLastError());
    ctx->stats.launches_extend++;
    return PT_OK;
}

pt_status render_aov_queues(pt_scene *s, pt_film *f, const pt_params *p, const ExtendPlan &pl, const AovConst &ac)
{
    pt_ctx *ctx = s->ctx;
    pt_film::Aov &a = f->aov;
    hipStream_t st = ctx->stream;
    if (a.n_tiles == 0) return PT_OK;
    const float4 *inst_frame = nullptr;
    if (s->n_inst && ctx->tune.inst_frames != 0) {  // the table k_shade<INST> reads, when the context uses it
        const pt_status rcf = ptb_ensure_inst_frames(s);
        if (rcf != PT_OK) return rcf;
        inst_frame = s->d_inst_frame;
    }
    // chunk of whole tiles: what the budget leaves beside the film's render workspace, the ray scratch already held counted as free
    const size_t tile_rays = 64 * (size_t)p->spp_per_frame;
    const size_t held = f->work.bytes + (a.bytes - a.cap_rays * AOV_RAY_BYTES);
    size_t fit_rays = AOV_MAX_CHUNK_RAYS;
    if (ctx->mem_budget) fit_rays = std::min(fit_rays, ctx->mem_budget > held ? (ctx->mem_budget - held) / AOV_RAY_BYTES : 0);
    size_t chunk_tiles = std::min<size_t>(a.n_tiles, fit_rays / tile_rays);
    if (chunk_tiles == 0) {
        if (ctx->mem_budget && tile_rays * AOV_RAY_BYTES + held > ctx->mem_budget) {
            ctx->err = "guide-buffer workspace exceeds the memory budget (" + std::to_string((held + tile_rays * AOV_RAY_BYTES) >> 20) + " MB wanted for one tile, " +
                       std::to_string(ctx->mem_budget >> 20) + " MB allowed)";
            return PT_ERR_OOM;
        }
        chunk_tiles = 1;  // (more than 2^20 samples per pixel cannot be asked for: spp <= 65535)
    }
    pt_status rc = ensure_rays(f, chunk_tiles * tile_rays);
    if (rc != PT_OK) return rc;
    const AovPlanes planes = planes_of(f);
    const float4 *tri4 = pl.bvh8 ? s->d_tri4_8 : s->d_tri4, *rec64 = pl.bvh8 ? s->d_shade64_8 : s->d_shade64;
    for (uint32_t k = 0; k < p->frame_count; k++) {
        const int32_t frame = p->frame + (int32_t)k;
        const int last = k + 1 == p->frame_count ? 1 : 0;
        for (uint32_t t0 = 0; t0 < a.n_tiles; t0 += (uint32_t)chunk_tiles) {
            const uint32_t nt = std::min<uint32_t>((uint32_t)chunk_tiles, a.n_tiles - t0);
            const uint32_t n_pix = nt * 64u, n_rays = n_pix * p->spp_per_frame;
            const unsigned long long valid = a.h_valid[t0 + nt] - a.h_valid[t0];  // the chunk's pixels inside the image
            const int grid_g = (int)std::min<uint32_t>((n_rays + TB - 1) / TB, (uint32_t)ctx->num_cus * 32u);
            k_aov_generate<<<grid_g, TB, 0, st>>>(ac, a.d_tiles + t0, n_rays, frame, a.d_rayA, a.d_rayB, a.d_count);
            // (stats = null: the extend kernels would count the rays of the pixels beyond the image's edge too; k_aov_reduce adds the chunk's)
            ptw_launch_extend(pl, s, a.d_rayA, a.d_rayB, a.d_hit, a.d_hit_inst, a.d_count, nullptr, nullptr, p->tmin, p->tmax, false, false, st);
            const int grid_r = (int)((n_pix + TB - 1) / TB);
            if (s->n_inst)
                k_aov_reduce<true><<<grid_r, TB, 0, st>>>(ac, a.d_tiles + t0, n_pix, frame, last, a.d_hit, a.d_hit_inst, tri4, rec64, s->d_faces, s->d_inst6, inst_frame,
                                                          s->d_tlas_prim_of, s->n_tris, planes, ctx->d_stats, valid * p->spp_per_frame);
            else
                k_aov_reduce<false><<<grid_r, TB, 0, st>>>(ac, a.d_tiles + t0, n_pix, frame, last, a.d_hit, nullptr, tri4, rec64, s->d_faces, nullptr, nullptr, nullptr,
                                                           s->n_tris, planes, ctx->d_stats, valid * p->spp_per_frame);
            PT_HIP(ctx, hipGetLastError());
            ctx->stats.launches_extend++;
            ctx->stats.launches_other += 2;
        }
    }
    return PT_OK;
}

}  // namespace

size_t pta_plane_bytes(const pt_film *f, uint32_t which)
{
    const size_t n = (size_t)f->w * f->h;
    return which <= PT_AOV_EMISSION ? sizeof(float) * 3 * n : which <= PT_AOV_ALPHA ? sizeof(float) * n : sizeof(uint32_t) * 2 * n;
}

pt_status pta_enable(pt_film *f, void *const *device_planes)
{
    pt_ctx *ctx = f->ctx;
    pt_film::Aov &a = f->aov;
    if (a.enabled) { ctx->err = "the film already has guide buffers"; return PT_ERR_INVALID_ARG; }
    for (uint32_t k = 0; k < PT_AOV_COUNT; k++) {
        void *ext = device_planes ? device_planes[k] : nullptr;
        a.own[k] = ext == nullptr;
        a.plane[k] = ext;
        if (!ext) {
            const hipError_t e = hipMalloc(&a.plane[k], pta_plane_bytes(f, k));
            if (e != hipSuccess) {
                (void)hipGetLastError();
                a.plane[k] = nullptr;
                ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e);
                pta_free(f);
                return PT_ERR_OOM;
            }
        }
    }
    a.enabled = true;
    const pt_status rc = pta_clear(f, ctx->stream);
    if (rc != PT_OK) { pta_free(f); return rc; }
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

pt_status pta_clear(pt_film *f, hipStream_t st)
{
    if (!f->aov.enabled) return PT_OK;
    for (uint32_t k = 0; k < PT_AOV_COUNT; k++) PT_HIP(f->ctx, hipMemsetAsync(f->aov.plane[k], 0, pta_plane_bytes(f, k), st));
    return PT_OK;
}

void pta_free(pt_film *f)
{
    pt_film::Aov &a = f->aov;
    for (uint32_t k = 0; k < PT_AOV_COUNT; k++) {
        if (a.own[k] && a.plane[k]) (void)hipFree(a.plane[k]);
        a.plane[k] = nullptr;
        a.own[k] = false;
    }
    pt_scratch_free({ pt_buf_of(a.d_tiles), pt_buf_of(a.d_rayA), pt_buf_of(a.d_rayB), pt_buf_of(a.d_hit), pt_buf_of(a.d_hit_inst), pt_buf_of(a.d_count) },
                    &a.bytes, a.bytes);
    a = pt_film::Aov{};
}

pt_status pta_render(pt_scene *s, pt_film *f, const pt_params *p)
{
    pt_ctx *ctx = s->ctx;
    pt_status rc = s->broken ? ptb_repair(s) : PT_OK;  // (as ptw_render: a repair may bring back a parked instance set)
    if (rc != PT_OK) return rc;
    if (!f->aov.enabled) { ctx->err = "the film has no guide buffers: pt_film_enable_aov first"; return PT_ERR_INVALID_ARG; }
    if (p->width != f->w || p->height != f->h) { ctx->err = "params width/height differ from the film's"; return PT_ERR_INVALID_ARG; }
    if (p->world == 0 || p->rank >= p->world) { ctx->err = "rank/world invalid"; return PT_ERR_INVALID_ARG; }
    if (p->spp_per_frame == 0 || p->spp_per_frame > 0xFFFFu) { ctx->err = "spp_per_frame must be in 1..65535"; return PT_ERR_INVALID_ARG; }
    if (p->frame < 0 || p->frame_count == 0) { ctx->err = "frame must be >= 0 and frame_count >= 1"; return PT_ERR_INVALID_ARG; }
    if (p->pipeline > PT_PIPELINE_AUTO) { ctx->err = "unknown pipeline"; return PT_ERR_UNSUPPORTED; }
    if (p->pipeline == PT_PIPELINE_WAVEFRONT_NEE) { ctx->err = "pt_render_aov: the guides do not depend on the estimator (PT_PIPELINE_WAVEFRONT, _FUSED or _AUTO)"; return PT_ERR_UNSUPPORTED; }
    if (p->flags & ~(uint32_t)PT_FLAG_NEE) { ctx->err = "pt_render_aov takes no flag but PT_FLAG_NEE (ignored): blocking, not instrumented"; return PT_ERR_UNSUPPORTED; }
    ExtendPlan pl;
    rc = ptw_plan_extend(s, p->extend, pl);
    if (rc != PT_OK) return rc;
    AovFusedPlan fp;
    bool fused = false;
    if (p->pipeline != PT_PIPELINE_WAVEFRONT) {
        const std::string keep = ctx->err;
        rc = plan_aov_fused(s, p, pl, fp);
        if (rc == PT_OK) fused = true;
        else if (p->pipeline == PT_PIPELINE_FUSED) return rc;
        else ctx->err = keep;  // (AUTO: not an error of this call, the scene is simply the queue form's)
    }
    ctx->stats.pipeline = fused ? PT_PIPELINE_FUSED : PT_PIPELINE_WAVEFRONT;
    rc = ensure_tiles(f, p->rank, p->world);
    if (rc == PT_OK) rc = ensure_count(f);
    if (rc != PT_OK) return rc;
    AovConst ac{};
    ac.cam = ptw_camera(p);
    ac.tmin = p->tmin; ac.tmax = p->tmax;
    ac.width = p->width; ac.height = p->height; ac.spp = p->spp_per_frame;
    ac.div_spp.init(p->spp_per_frame);
    if (fused && ctx->tune.cull != 0) {
        int32_t rect[4];
        ptw_subject_rect(s, p, rect);
        ac.cull_on = rect[2] >= rect[0] && rect[3] >= rect[1] ? 1u : 0u;
        std::copy(rect, rect + 4, ac.cull);
    }
    hipStream_t st = ctx->stream;
    PT_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    rc = fused ? render_aov_fused(s, f, p, pl, fp, ac) : render_aov_queues(s, f, p, pl, ac);
    if (rc != PT_OK) { (void)hipStreamSynchronize(st); return rc; }
    PT_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    float ms = 0.f;
    PT_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_a, ctx->ev_b));
    ctx->stats.ms_total += ms;
    ctx->stats.paths += f->aov.valid_pixels * p->spp_per_frame * p->frame_count;
    return PT_OK;
}
