// scene_build.hip -- pt_scene_create / pt_scene_set_bvh_quality / pt_scene_set_instances: what main.cpp:492-538 does with the
// three scene arrays.  De-indexes the triangles (k_gather), has the tree built (lbvh_build.hip; the surface-area BVH4 of small
// scenes: bvh4_sah_device.hip), packs the per-triangle tables in the traversed leaf order (k_pack: vertices, the geometric
// normal of closesthit.rchit:43-48, brdf = Kd / pi, the tangent frame of raygen.rgen:14-21 -- evaluated once with the
// per-hit operations), and for instanced scenes the TLAS, the per-instance matrices and the world-space emitter / frame tables.
#include "bvh_build.h"
#include "self_leaf.h"
#include "scene_instances_kernel.h"  // si_invert_3x4, SI_OK: one set of statements for the host call and the device call

#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

// 1. gather: de-indexed triangles + their boxes.  tri_orig: 3 float4 per triangle in prim-id order.
__global__ __launch_bounds__(TB) void k_gather(const float *__restrict__ vertices, const uint32_t *__restrict__ indices,
                                               uint32_t n_tris, float4 *__restrict__ tri_orig,
                                               float4 *__restrict__ tlo, float4 *__restrict__ thi)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (t < n_tris) {
        float v[3][3];
        for (int c = 0; c < 3; c++) {
            const uint32_t vi = indices[3 * (size_t)t + c];
            for (int k = 0; k < 3; k++) v[c][k] = vertices[3 * (size_t)vi + k];
        }
        for (int k = 0; k < 3; k++) {
            mn[k] = fminf(fminf(v[0][k], v[1][k]), v[2][k]);
            mx[k] = fmaxf(fmaxf(v[0][k], v[1][k]), v[2][k]);
        }
        tri_orig[3 * (size_t)t + 0] = make_float4(v[0][0], v[0][1], v[0][2], __uint_as_float(t));
        tri_orig[3 * (size_t)t + 1] = make_float4(v[1][0], v[1][1], v[1][2], 0.f);
        tri_orig[3 * (size_t)t + 2] = make_float4(v[2][0], v[2][1], v[2][2], 0.f);
        tlo[t] = make_float4(mn[0], mn[1], mn[2], 0.f);
        thi[t] = make_float4(mx[0], mx[1], mx[2], 0.f);
    }
}


// 6. leaf-ordered records
__global__ __launch_bounds__(TB) void k_pack(const float4 *__restrict__ tri_orig, const float *__restrict__ faces,
                                             const uint32_t *__restrict__ prim_of, uint32_t n,
                                             float4 *__restrict__ tri4, float4 *__restrict__ shade4,
                                             float4 *__restrict__ shade64, float4 *__restrict__ ke4,
                                             float4 *__restrict__ frame4 = nullptr)
{
    const uint32_t pos = blockIdx.x * TB + threadIdx.x;
    if (pos >= n) return;
    const uint32_t prim = prim_of[pos];
    const float4 a = tri_orig[3 * (size_t)prim + 0], b = tri_orig[3 * (size_t)prim + 1],
                 c = tri_orig[3 * (size_t)prim + 2];
    tri4[3 * (size_t)pos + 0] = a;  // .w = bits(prim)
    tri4[3 * (size_t)pos + 1] = b;
    tri4[3 * (size_t)pos + 2] = make_float4(c.x, c.y, c.z, a.w);  // .w = bits(prim) again: the pair-leaf test of k_extend
                                                                  // reads only this vertex of a quad's second triangle
    // closesthit.rchit:43-48 normal (never flipped), :60 brdf = Kd / pi (true divide), :61 emission
    const ptm::f3 nrm = ptm::tri_normal({ a.x, a.y, a.z }, { b.x, b.y, b.z }, { c.x, c.y, c.z });
    const float *f = faces + 6 * (size_t)prim;
    const float br = ptm::fdiv(f[0], 3.1415927410125732f), bg = ptm::fdiv(f[1], 3.1415927410125732f),
                bb = ptm::fdiv(f[2], 3.1415927410125732f);
    shade4[3 * (size_t)pos + 0] = make_float4(nrm.x, nrm.y, nrm.z, br);
    shade4[3 * (size_t)pos + 1] = make_float4(bg, bb, f[3], f[4]);
    shade4[3 * (size_t)pos + 2] = make_float4(f[5], 0.f, 0.f, 0.f);
    if (frame4) {  // raygen.rgen:14-21 for this triangle's normal: {T.xyz, B.x} {B.yz, 0, 0}
        ptm::f3 T, B;
        ptm::tangent_frame(nrm, T, B);
        frame4[2 * (size_t)pos + 0] = make_float4(T.x, T.y, T.z, B.x);
        // (.z, .w: the self-leaf rule of this triangle -- k_self_leaf, which knows the leaves, writes it; until then: never skip)
        frame4[2 * (size_t)pos + 1] = make_float4(B.y, B.z, INFINITY, 0.f);
    }
    // the same values regrouped for scenes whose tables stay in HBM (k_shade<.., false>): one 64-B record instead of
    // two 48-B ones (4 divergent 16-B loads per hit instead of 6, 1 instead of 3 for a path that ends at this hit),
    // the emission apart because almost no triangle has one
    const bool emits = !(f[3] == 0.f && f[4] == 0.f && f[5] == 0.f);
    shade64[4 * (size_t)pos + 0] = make_float4(a.x, a.y, a.z, nrm.x);
    shade64[4 * (size_t)pos + 1] = make_float4(b.x, b.y, b.z, nrm.y);
    shade64[4 * (size_t)pos + 2] = make_float4(c.x, c.y, c.z, nrm.z);
    shade64[4 * (size_t)pos + 3] = make_float4(br, bg, bb, emits ? 1.f : 0.f);
    ke4[pos] = make_float4(f[3], f[4], f[5], 0.f);
}


// 6b. the self-leaf rule (self_leaf.h) of every triangle of the traversed BVH4, beside its tangent frame: frame4[2 * pos + 1] = {.., .., thr,
// g | the leaf's 14-bit code}.  One thread per child word; a leaf that is no single triangle or fan pair of a pair-leaf tree, or that the compact
// codes cannot name, keeps k_pack's "never".  Runs wherever k_pack runs (pack_tables), so a refit or rebuild recomputes it from the moved vertices.
__global__ __launch_bounds__(TB) void k_self_leaf(const float4 *__restrict__ wide, uint32_t n_wide, const float4 *__restrict__ tri4, uint32_t n, float scene_e,
                                                  float4 *__restrict__ frame4)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= 4u * n_wide) return;
    const uint32_t w = reinterpret_cast<const uint32_t *>(wide + 8 * (size_t)(i >> 2) + 6)[i & 3u];
    if (w == SENTINEL || !(w & PT_LEAF)) return;
    const uint32_t cnt = ((w >> 28) & 7u) + 1u, first = w & 0x0FFFFFFFu;
    if (cnt > 2u || first + cnt > n || first + cnt > 0x7FFu) return;
    const float4 a = tri4[3 * (size_t)first + 0], b = tri4[3 * (size_t)first + 1], c = tri4[3 * (size_t)first + 2];
    const float v0[3] = { a.x, a.y, a.z }, v1[3] = { b.x, b.y, b.z }, v2[3] = { c.x, c.y, c.z };
    float *out = reinterpret_cast<float *>(frame4 + 2 * (size_t)first + 1);
    const uint32_t code = ptsl::leaf_code14(first, cnt);
    auto put = [&](float *o, const ptsl::Rule r) {  // (a triangle that never skips carries no code)
        o[2] = r.thr;
        o[3] = r.thr < INFINITY ? __uint_as_float(__float_as_uint(r.g) | code) : 0.f;
    };
    if (cnt == 1u) {
        put(out, ptsl::leaf_rule(v0, v2, v1, nullptr, scene_e));
        return;
    }
    const float4 d = tri4[3 * (size_t)first + 5];  // the fan pair (v0, v1, v2) + (v0, v2, v3): the second half's apex (pair_leaf.h)
    const float v3[3] = { d.x, d.y, d.z };
    put(out, ptsl::leaf_rule(v0, v2, v1, v3, scene_e));
    put(out + 8, ptsl::leaf_rule(v0, v2, v3, v1, scene_e));  // (the second half's record: two float4 on)
}


__global__ __launch_bounds__(TB) void k_compose(const uint32_t *__restrict__ order8, const uint32_t *__restrict__ prim_of, uint32_t n,
                                                uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i < n) out[i] = prim_of[order8[i]];
}


// behind every k_pack of the traversed tree's tables (d_wide, pair_leaves, bmin / bmax are the new tree's by then)
void pack_self_leaf(pt_scene *s, hipStream_t st)
{
    if (!s->pair_leaves || !s->d_frame4 || !s->n_wide) return;  // (leaves of several independent triangles: k_pack's "never" stands)
    float e = 0.f;
    for (int k = 0; k < 3; k++) e = std::max(e, std::max(std::fabs(s->bmin[k]), std::fabs(s->bmax[k])));
    k_self_leaf<<<(4 * s->n_wide + TB - 1) / TB, TB, 0, st>>>(s->d_wide, s->n_wide, s->d_tri4, s->n_tris, e, s->d_frame4);
}

}  // namespace

__global__ __launch_bounds__(TB) void k_wide_half(const float4 *__restrict__ wide, uint32_t n_wide, float cx, float cy,
                                                  float cz, float rsx, float rsy, float rsz, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n_wide) return;
    const float4 *nd = wide + 8 * (size_t)i;
    const float c[3] = { cx, cy, cz }, rs[3] = { rsx, rsy, rsz };
    uint32_t d[12];
    for (int ax = 0; ax < 3; ax++) {
        const float4 lo = nd[ax], hi = nd[3 + ax];
        const float l[4] = { lo.x, lo.y, lo.z, lo.w }, h[4] = { hi.x, hi.y, hi.z, hi.w };
        uint32_t hl[4], hh[4];
        for (int k = 0; k < 4; k++) {
            hl[k] = __half_as_ushort(__float2half_rd((l[k] - c[ax]) * rs[ax] - 3.814697265625e-06f));
            hh[k] = __half_as_ushort(__float2half_ru((h[k] - c[ax]) * rs[ax] + 3.814697265625e-06f));
        }
        d[2 * ax + 0] = hl[0] | (hl[1] << 16); d[2 * ax + 1] = hl[2] | (hl[3] << 16);
        d[6 + 2 * ax + 0] = hh[0] | (hh[1] << 16); d[6 + 2 * ax + 1] = hh[2] | (hh[3] << 16);
    }
    const float4 cw = nd[6];
    uint4 *o = out + 4 * (size_t)i;
    o[0] = make_uint4(d[0], d[1], d[2], d[3]);
    o[1] = make_uint4(d[4], d[5], d[6], d[7]);
    o[2] = make_uint4(d[8], d[9], d[10], d[11]);
    o[3] = make_uint4(__float_as_uint(cw.x), __float_as_uint(cw.y), __float_as_uint(cw.z), __float_as_uint(cw.w));
}

// ---- scene buffers ("Scene buffers") -------------------------------------------------------------------
// Every device pointer of a scene, once, by lifetime.  d_wide is not among them: it is a view of d_wide_lbvh or d_wide_sah.
std::vector<pt_buf> ptb_scene_buffers(pt_scene *s, pt_scene_life life)
{
    switch (life) {
    case PT_LIFE_SOURCE:  // live as long as the scene: the kept triangles and materials, the per-triangle tables, the emitters
        return { pt_buf_of(s->d_tri_orig), pt_buf_of(s->d_faces), pt_buf_of(s->d_tri4), pt_buf_of(s->d_shade4), pt_buf_of(s->d_shade64),
                 pt_buf_of(s->d_ke4), pt_buf_of(s->d_frame4), pt_buf_of(s->d_lights), pt_buf_of(s->d_light_prim) };
    case PT_LIFE_TREE:  // everything that hangs off the binary tree: dropped and made again by a rebuild
        return { pt_buf_of(s->d_nodes), pt_buf_of(s->d_keys), pt_buf_of(s->d_prim_of), pt_buf_of(s->d_prim_of_sah), pt_buf_of(s->d_wide_lbvh),
                 pt_buf_of(s->d_wide_sah), pt_buf_of(s->d_wide16), pt_buf_of(s->d_wide16t), pt_buf_of(s->d_wide8), pt_buf_of(s->d_prim_of8),
                 pt_buf_of(s->d_tri4_8), pt_buf_of(s->d_shade64_8), pt_buf_of(s->d_ke4_8) };
    case PT_LIFE_INSTANCES:
        return { pt_buf_of(s->d_inst6), pt_buf_of(s->d_tlas_wide), pt_buf_of(s->d_tlas_prim_of), pt_buf_of(s->d_tlas16), pt_buf_of(s->d_inst_frame),
                 pt_buf_of(s->d_lights_inst) };
    case PT_LIFE_GIVEN:
        return { pt_buf_of(s->d_xforms) };
    default:  // PT_LIFE_PREVIOUS
        return { pt_buf_of(s->prev.d_tri), pt_buf_of(s->prev.d_xf) };
    }
}

// tests: an allocation that is out of memory, without the memory (pt_tuning.fail_rebuild: a scene that has, or has lost, a tree)
static pt_status injected_failure(pt_scene *s)
{
    pt_ctx *ctx = s->ctx;
    if (!(ctx->tune.fail_rebuild > 0 && (s->broken || s->n_nodes))) return PT_OK;
    ctx->tune.fail_rebuild--;
    ctx->err = "hipMalloc: out of memory (pt_tuning.fail_rebuild)";
    return PT_ERR_OOM;
}

pt_status ptb_scene_alloc(pt_scene *s, const char *what, const std::vector<pt_buf> &set)
{
    const pt_status inj = injected_failure(s);
    if (inj != PT_OK) { pt_scratch_free(set, nullptr, 0); return inj; }  // (as the allocator leaves a set it could not give its memory)
    return pt_scratch_alloc(s->ctx, what, set, nullptr, 0);
}

// A set and the host arrays that fill its first buffers: the set is present only when it is whole, a failed upload frees it again.
static pt_status alloc_filled(pt_scene *s, const char *what, const std::vector<pt_buf> &set, std::initializer_list<const void *> sources)
{
    PT_TRY(ptb_scene_alloc(s, what, set));
    size_t k = 0;
    for (const void *src : sources) {
        const hipError_t e = hipMemcpy(*set[k].p, src, set[k].bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            pt_scratch_free(set, nullptr, 0);
            s->ctx->err = std::string("hipMemcpy to ") + what + ": " + hipGetErrorString(e);
            return PT_ERR_HIP;
        }
        k++;
    }
    return PT_OK;
}

// The leaf order the traversed tree's per-triangle tables are packed in -- the prim_of the last k_pack of d_tri4 / d_shade4 / d_shade64 / d_ke4 was
// given: the surface-area BVH4's (builder 1) or the PLOC tree's (builder 2), else the LBVH's.  What a refit re-packs in, and what
// pt_scene_set_faces rewrites the material words in.
static const uint32_t *traversed_order(const pt_scene *s) { return s->bvh4_builder != 0u ? s->d_prim_of_sah : s->d_prim_of; }

// leaf_pad() of the device build, same float operations
static float leaf_pad_of(const float *bmin, const float *bmax)
{
    float scale = 0.f;
    for (int k = 0; k < 3; k++) scale = fmaxf(scale, fmaxf(fabsf(bmin[k]), fabsf(bmax[k])));
    return scale * 3.814697265625e-06f;
}

// pt_scene_info.device_bytes / device_bytes8, a formula of the counts and not a counter of allocations: they report what a scene of this
// size keeps resident for traversal and rebuilds, the read-back arrays (d_keys, d_prim_of, d_nodes) and the lazily built tables left out.
// BVH4 path: triangle tables (tri4 48 + shade4 48 + shade64 64 + ke4 16 + frames 32 B each), the kept source arrays a rebuild re-packs
// from (d_tri_orig 48 + d_faces 24) + the 128-B and the two 64-B node arrays; the 8-wide path: its tables + nodes.
static void set_device_bytes(pt_scene *s)
{
    const uint64_t n = s->n_tris;
    s->device_bytes = n * (48 + 48 + 64 + 16 + 32 + PT_SOURCE_BYTES_PER_TRI) + 128ull * s->n_wide + 64ull * s->n_wide + 64ull * s->n_wide16t;
    s->device_bytes8 = s->d_wide8 ? n * (48 + 64 + 16 + 4) + 64ull * s->n_wide8 : 0ull;
}

// (re)builds s->d_wide16 from the BVH4 that is currently traversed
static pt_status make_wide16(pt_scene *s)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    ptb_norm_box(s->bmin, s->bmax, s->norm_c, s->norm_s, s->norm_rs);
    PT_TRY(ptb_scene_alloc(s, "the fp16 BVH4 nodes", { pt_buf_of(s->d_wide16, 64 * (size_t)s->n_wide) }));
    k_wide_half<<<(s->n_wide + TB - 1) / TB, TB, 0, st>>>(s->d_wide, s->n_wide, s->norm_c[0], s->norm_c[1], s->norm_c[2], s->norm_rs[0],
                                                         s->norm_rs[1], s->norm_rs[2], reinterpret_cast<uint4 *>(s->d_wide16));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    return PT_OK;
}

// triangle boxes from the de-indexed triangles (the same float operations as k_gather)
__global__ __launch_bounds__(TB) void k_tri_boxes(const float4 *__restrict__ tri_orig, uint32_t n, float4 *__restrict__ tlo,
                                                  float4 *__restrict__ thi)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t >= n) return;
    const float4 a = tri_orig[3 * (size_t)t + 0], b = tri_orig[3 * (size_t)t + 1], c = tri_orig[3 * (size_t)t + 2];
    tlo[t] = make_float4(fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z), 0.f);
    thi[t] = make_float4(fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z), 0.f);
}

// Everything that hangs off the binary tree -- the tree itself (LBVH, or its PLOC rebuild for big scenes under
// ePreferFastTrace), the BVH4 in both node formats, optionally the 8-wide nodes, the per-triangle tables in the traversed
// leaf order -- built (or rebuilt: quality change, first request for the 8-wide nodes) from the kept triangles.
static void free_tree_products(pt_scene *s)
{
    pt_scratch_free(ptb_scene_buffers(s, PT_LIFE_TREE), nullptr, 0);
    s->d_wide = nullptr;
    s->n_wide8 = s->levels8 = 0; s->n_wide16t = s->levels4t = 0;
}

static pt_status build_tree_products_unguarded(pt_scene *s, uint32_t quality, bool want8);

// A rebuild frees the old products first (peak memory = one set, and a scene of 8 M triangles holds 2.6 GB of them), so a
// rebuild that fails part-way -- out of memory beside a 70-100 GB film workspace is the plausible case -- leaves the scene
// WITHOUT a tree.  It is then marked broken: every product pointer null, every count zero, and plan_extend / pt_scene_read_* /
// pt_scene_set_instances answer PT_ERR_UNSUPPORTED instead of launching kernels on null tables.  The triangles and materials
// (d_tri_orig, d_faces) are untouched, so a later pt_scene_set_bvh_quality -- or the next render's request for the 8-wide
// nodes -- can build again; success clears the mark.
static void mark_broken(pt_scene *s, uint32_t quality)
{
    (void)hipGetLastError();  // an out-of-memory error is sticky until read
    free_tree_products(s);
    s->n_nodes = s->n_wide = s->n_wide_lbvh = 0;
    s->stack_need = s->stack_need_lbvh = 0xFFFFFFFFu;
    s->device_bytes = s->device_bytes8 = 0;
    s->quality = quality;  // what the scene is meant to have: ptb_repair / the next pt_scene_set_bvh_quality build exactly that
    s->broken = true;
}

// An instanced scene whose BLAS could not be built (pt_scene_update) keeps its instance set parked in h_xforms (or, given in device memory,
// in d_xforms) while n_inst = 0 and the scene is broken.  Every successful build of the tree products ends here and sets the instances again; if that fails, the scene is
// broken again with the set still parked, so no way out of the broken state drops the instances.
static pt_status restore_parked_instances(pt_scene *s, uint32_t quality)
{
    if (s->n_inst || !pt_given_instances(s)) return PT_OK;
    if (s->d_xforms) {  // the set lives on the device: set again from there (the call makes its own kept copy; this one is freed behind it)
        float4 *d_xf = s->d_xforms;
        const uint32_t n = s->n_xforms_dev;
        s->d_xforms = nullptr; s->n_xforms_dev = 0;
        const pt_status rc = ptb_set_instances_device(s, reinterpret_cast<const float *>(d_xf), n);
        if (rc != PT_OK) {
            const std::string err = s->ctx->err;
            mark_broken(s, quality);
            s->d_xforms = d_xf; s->n_xforms_dev = n;
            s->ctx->err = err;
        } else
            (void)hipFree(d_xf);
        return rc;
    }
    const std::vector<float> xf = s->h_xforms;
    const pt_status rc = ptb_set_instances(s, xf.data(), (uint32_t)(xf.size() / 12));
    if (rc != PT_OK) {
        const std::string err = s->ctx->err;
        mark_broken(s, quality);
        s->h_xforms = xf;
        s->ctx->err = err;
    }
    return rc;
}

static pt_status build_tree_products(pt_scene *s, uint32_t quality, bool want8)
{
    const pt_status rc = build_tree_products_unguarded(s, quality, want8);
    if (rc != PT_OK) { mark_broken(s, quality); return rc; }
    s->broken = false;
    return restore_parked_instances(s, quality);
}

static pt_status build_tree_products_unguarded(pt_scene *s, uint32_t quality, bool want8)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t n = s->n_tris, gt = (n + TB - 1) / TB;
    free_tree_products(s);
    PT_TRY(injected_failure(s));
    DevBuf<float4> d_tlo, d_thi;
    PT_HIP(ctx, d_tlo.alloc(n));
    PT_HIP(ctx, d_thi.alloc(n));
    PT_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    k_tri_boxes<<<gt, TB, 0, st>>>(s->d_tri_orig, n, d_tlo.p, d_thi.p);
    const bool ploc = quality == PT_BVH_PREFER_FAST_TRACE && n > PT_SAH_MAX_TRIS;
    BvhOut o;
    PT_TRY(ptb_build_bvh(ctx, d_tlo.p, d_thi.p, n, PT_BLAS_LEAF_MAX, o, 2 | (want8 ? 1 : 0), ploc));
    s->d_keys = o.d_keys.release(); s->d_prim_of = o.d_prim_of.release(); s->d_nodes = o.d_nodes.release();
    s->d_wide = s->d_wide_lbvh = o.d_wide.release();
    s->d_prim_of_sah = o.d_prim_q.release();
    s->d_wide8 = o.d_wide8.release(); s->n_wide8 = o.n_wide8; s->levels8 = o.levels8;
    s->d_wide16t = o.d_wide16t.release(); s->n_wide16t = o.n_wide16t; s->levels4t = o.levels4t;
    s->n_nodes = o.n_nodes; s->n_wide = o.n_wide; s->height = o.height; s->height_tree = o.height_tree; s->stack_need = o.stack_need;
    s->n_wide_lbvh = s->n_wide; s->stack_need_lbvh = s->stack_need;
    for (int k = 0; k < 3; k++) { s->bmin[k] = o.bmin[k]; s->bmax[k] = o.bmax[k]; }
    s->bvh4_builder = s->d_prim_of_sah ? 2u : 0u;
    s->area_lbvh = o.area_lbvh; s->area_ploc = o.area_ploc;
    s->pair_leaves = PT_BLAS_LEAF_MAX == 1u;
    const uint32_t *order = s->d_prim_of_sah ? s->d_prim_of_sah : s->d_prim_of;   // the traversed leaf order
    k_pack<<<gt, TB, 0, st>>>(s->d_tri_orig, s->d_faces, order, n, s->d_tri4, s->d_shade4, s->d_shade64, s->d_ke4, s->d_frame4);
    pack_self_leaf(s, st);
    if (s->d_wide8) {  // the 8-wide tree's own triangle order: its per-triangle tables (the LDS-sized shade4 is never used with it)
        PT_TRY(ptb_scene_alloc(s, "the 8-wide tree's triangle tables",
                               { pt_buf_of(s->d_prim_of8, sizeof(uint32_t) * (size_t)n), pt_buf_of(s->d_tri4_8, sizeof(float4) * 3 * (size_t)n),
                                 pt_buf_of(s->d_shade64_8, sizeof(float4) * 4 * (size_t)n), pt_buf_of(s->d_ke4_8, sizeof(float4) * (size_t)n) }));
        DevBuf<float4> d_shade4_scratch;
        PT_HIP(ctx, d_shade4_scratch.alloc(3 * (size_t)n));
        k_compose<<<gt, TB, 0, st>>>(o.d_order8.p, order, n, s->d_prim_of8);
        k_pack<<<gt, TB, 0, st>>>(s->d_tri_orig, s->d_faces, s->d_prim_of8, n, s->d_tri4_8, d_shade4_scratch.p, s->d_shade64_8, s->d_ke4_8);
        PT_HIP(ctx, hipStreamSynchronize(st));
    }
    PT_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipEventElapsedTime(&s->build_ms, ctx->ev_a, ctx->ev_b));
    set_device_bytes(s);
    s->quality = quality;
    return make_wide16(s);
}

// PT_EXTEND_HBM8 / pt_tuning.hbm8 on a scene that was built without the 8-wide nodes: build them now (extend_launch.hip asks)
pt_status ptb_ensure_wide8(pt_scene *s)
{
    if (s->d_wide8 || s->n_tris < 2 || s->n_inst) return PT_OK;
    PT_HIP(s->ctx, hipStreamSynchronize(s->ctx->stream));
    return build_tree_products(s, s->quality, true);
}

// a scene whose last rebuild failed (above) gets one more try per render / trace / read-back: the film whose workspace
// crowded it out may be gone by now
pt_status ptb_repair(pt_scene *s)
{
    if (!s->broken) return PT_OK;
    if (s->n_inst) { s->ctx->err = PT_BROKEN_SCENE_MSG; return PT_ERR_UNSUPPORTED; }  // (cannot happen: a broken scene has its instances parked)
    PT_HIP(s->ctx, hipStreamSynchronize(s->ctx->stream));
    const pt_status rc = build_tree_products(s, s->quality, s->ctx->tune.hbm8 != 0);
    if (rc != PT_OK) s->ctx->err = std::string(PT_BROKEN_SCENE_MSG) + " [" + s->ctx->err + "]";
    return rc;
}

// one emitter record of the NEE pipeline (pt_internal.h d_lights): normal as closesthit.rchit:43-48, area = |cross| / 2, cdf = the
// running float sum of the areas in primitive order (this file is compiled with -ffp-contract=off on the host side too)
static void push_emitter(const float *a, const float *b, const float *c, const float4 ke, float &run, std::vector<float4> &lights)
{
    const float e1[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, e2[3] = { c[0] - a[0], c[1] - a[1], c[2] - a[2] };
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
    run = run + 0.5f * len;
    lights.push_back(make_float4(a[0], a[1], a[2], run));
    lights.push_back(make_float4(b[0], b[1], b[2], 0.f));
    lights.push_back(make_float4(c[0], c[1], c[2], 0.f));
    lights.push_back(make_float4(-(cx / len), -(cy / len), -(cz / len), 0.f));
    lights.push_back(ke);
}

// fan pairs as a loader emits them for quads: the next triangle starts at the same vertex and continues from this one's third
// (bitwise equal coordinates); greedy, non-overlapping
static void find_fan_pairs(const float *h_vertices, const uint32_t *h_indices, uint32_t n, std::vector<uint8_t> &pair)
{
    pair.assign(n, 0);
    auto vtx = [&](uint32_t tri, int k) { return h_vertices + 3 * (size_t)h_indices[3 * (size_t)tri + k]; };
    for (uint32_t i = 0; i + 1 < n; i++) {
        const bool same = std::memcmp(vtx(i, 0), vtx(i + 1, 0), 12) == 0 && std::memcmp(vtx(i, 2), vtx(i + 1, 1), 12) == 0;
        if (same) { pair[i] = 1; i++; }
    }
}

// The caller's vertices and indices on the device -- copies of host arrays, or the caller's own device arrays, read where they lie -- and, after
// gather(), the de-indexed triangles in d_tri_orig with their boxes here.
struct GeometryUpload {
    DevBuf<float> d_vert;
    DevBuf<uint32_t> d_idx;
    DevBuf<float4> d_tlo, d_thi;
    const float *vert = nullptr;    // what gather() reads
    const uint32_t *idx = nullptr;
    pt_status upload(pt_ctx *ctx, const pt_geometry &g, uint32_t n)
    {
        hipStream_t st = ctx->stream;
        if (!g.on_device) {
            PT_HIP(ctx, d_vert.alloc(3 * (size_t)g.n_verts));
            PT_HIP(ctx, d_idx.alloc(3 * (size_t)n));
        }
        PT_HIP(ctx, d_tlo.alloc(n));
        PT_HIP(ctx, d_thi.alloc(n));
        vert = g.vertices; idx = g.indices;
        if (g.on_device) return PT_OK;
        PT_HIP(ctx, hipMemcpyAsync(d_vert.p, g.vertices, sizeof(float) * 3 * (size_t)g.n_verts, hipMemcpyHostToDevice, st));
        PT_HIP(ctx, hipMemcpyAsync(d_idx.p, g.indices, sizeof(uint32_t) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
        PT_HIP(ctx, hipStreamSynchronize(st));  // pageable host sources are done with
        vert = d_vert.p; idx = d_idx.p;
        return PT_OK;
    }
    void gather(pt_scene *s)
    {
        k_gather<<<(s->n_tris + TB - 1) / TB, TB, 0, s->ctx->stream>>>(vert, idx, s->n_tris, s->d_tri_orig, d_tlo.p, d_thi.p);
    }
};

// small scenes: the unpadded triangle boxes a build of the surface-area BVH4 reads, from the device's (gather())
static pt_status keep_host_boxes(pt_scene *s, const float4 *d_tlo, const float4 *d_thi)
{
    pt_ctx *ctx = s->ctx;
    const uint32_t n = s->n_tris;
    std::vector<float4> lo(n), hi(n);
    PT_HIP(ctx, hipMemcpyAsync(lo.data(), d_tlo, sizeof(float4) * n, hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP(ctx, hipMemcpyAsync(hi.data(), d_thi, sizeof(float4) * n, hipMemcpyDeviceToHost, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->h_tlo.resize(3 * (size_t)n);
    s->h_thi.resize(3 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        s->h_tlo[3 * i + 0] = lo[i].x; s->h_tlo[3 * i + 1] = lo[i].y; s->h_tlo[3 * i + 2] = lo[i].z;
        s->h_thi[3 * i + 0] = hi[i].x; s->h_thi[3 * i + 1] = hi[i].y; s->h_thi[3 * i + 2] = hi[i].z;
    }
    return PT_OK;
}

// The tree products as pt_scene_create and a REBUILD make them.  Big scenes: one build at `quality`.  Small scenes: the LBVH, then the
// BVH4 of `quality` on top of it (ePreferFastTrace: the exact surface-area BVH4), build_ms the two device times added.
static pt_status build_at_quality(pt_scene *s, uint32_t quality, bool want8)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const bool small = s->n_tris <= PT_SAH_MAX_TRIS;
    PT_TRY(build_tree_products(s, small ? PT_BVH_PREFER_FAST_TRACE : quality, want8));
    if (!small) return PT_OK;
    const float lbvh_ms = s->build_ms;
    float sah_ms = 0.f;
    PT_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    PT_TRY(ptb_set_bvh_quality(s, quality));
    s->quality = quality;  // (FAST_BUILD: the LBVH just built is already the traversed tree)
    PT_HIP(ctx, hipEventRecord(ctx->ev_b, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipEventElapsedTime(&sah_ms, ctx->ev_a, ctx->ev_b));
    s->build_ms = lbvh_ms + sah_ms;
    return PT_OK;
}

pt_status ptb_build_scene(pt_scene *s, const pt_geometry &g, uint32_t n_tris)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t n = n_tris;
    const float *h_vertices = g.vertices, *h_faces = g.faces;  // (host pointers on the host path only)
    const uint32_t *h_indices = g.indices;
    s->n_tris = n;
    // the de-indexed triangles and the per-face materials stay resident (72 B per triangle): a change of the BVH quality,
    // or the first request for the 8-wide nodes, re-packs the tables from them in another leaf order
    PT_TRY(ptb_scene_alloc(s, "the scene's triangle tables",
                           { pt_buf_of(s->d_tri_orig, sizeof(float4) * 3 * (size_t)n), pt_buf_of(s->d_faces, sizeof(float) * 6 * (size_t)n),
                             pt_buf_of(s->d_tri4, sizeof(float4) * 3 * (size_t)n), pt_buf_of(s->d_shade4, sizeof(float4) * 3 * (size_t)n),
                             pt_buf_of(s->d_shade64, sizeof(float4) * 4 * (size_t)n), pt_buf_of(s->d_ke4, sizeof(float4) * (size_t)n),
                             pt_buf_of(s->d_frame4, sizeof(float4) * 2 * (size_t)n) }));
    PT_HIP(ctx, hipMemcpyAsync(s->d_faces, g.faces, sizeof(float) * 6 * (size_t)n, g.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    GeometryUpload up;
    PT_TRY(up.upload(ctx, g, n));
    up.gather(s);
    if (g.on_device) {  // the emitters by kernels, from d_faces and the gathered triangles (scene_device.hip): the bits of the loop below
        PT_TRY(ptsd_find_emitters(s));
        PT_TRY(ptsd_host_products(s, n <= PT_SAH_MAX_TRIS ? &s->h_pair : nullptr));
    } else {   // emitters for the NEE pipeline (push_emitter), and which primitives they are (pt_scene_update recomputes them)
        std::vector<float4> lights;
        float run = 0.f;
        s->h_light_prim.clear();
        for (uint32_t t = 0; t < n; t++) {
            const float *f = h_faces + 6 * (size_t)t;
            if (!(f[3] != 0.f || f[4] != 0.f || f[5] != 0.f)) continue;
            const float *a = h_vertices + 3 * (size_t)h_indices[3 * (size_t)t + 0], *b = h_vertices + 3 * (size_t)h_indices[3 * (size_t)t + 1],
                        *c = h_vertices + 3 * (size_t)h_indices[3 * (size_t)t + 2];
            push_emitter(a, b, c, make_float4(f[3], f[4], f[5], 0.f), run, lights);
            s->h_light_prim.push_back(t);
        }
        s->n_lights = (uint32_t)(lights.size() / 5);
        s->light_area = run;
        s->h_lights = lights;
        if (s->n_lights) PT_TRY(alloc_filled(s, "the emitter table", { pt_buf_of(s->d_lights, sizeof(float4) * lights.size()) }, { lights.data() }));
    }
    if (n <= PT_SAH_MAX_TRIS) {  // small scene: keep what a build of the surface-area BVH4 reads
        PT_TRY(keep_host_boxes(s, up.d_tlo.p, up.d_thi.p));
        if (!g.on_device) find_fan_pairs(h_vertices, h_indices, n, s->h_pair);
    }
    // the tree of the default quality (ePreferFastTrace, main.cpp:419): PLOC for big scenes; small scenes get the LBVH and the exact
    // surface-area BVH4 on top.  The 8-wide nodes only when the context asks AUTO to use them.
    // (small scenes get the 8-wide nodes at once -- a few KB; big ones on first request: 260 B per triangle nobody else needs)
    // ... and scenes AUTO walks through them: more than 1 MiB of BVH4 nodes + records, ~96 B per triangle (extend_launch.hip ptw_plan_extend)
    return build_at_quality(s, PT_BVH_PREFER_FAST_TRACE, ctx->tune.hbm8 == 1 || n <= PT_SAH_MAX_TRIS || (ctx->tune.hbm8 != 0 && 96ull * n > (1ull << 20)));
}

// Chooses the BVH4 that is traversed (pt_internal.h).  Re-packs the per-triangle tables in its leaf order.
pt_status ptb_set_bvh_quality(pt_scene *s, uint32_t quality)
{
    pt_ctx *ctx = s->ctx;
    if (quality > PT_BVH_PREFER_FAST_BUILD) { ctx->err = "unknown BVH quality"; return PT_ERR_INVALID_ARG; }
    if (s->n_inst) { ctx->err = "set the BVH quality before the instances"; return PT_ERR_UNSUPPORTED; }
    if (s->n_tris > PT_SAH_MAX_TRIS) {  // big scene: PLOC tree <-> LBVH, everything that hangs off the tree is rebuilt
        if (quality == s->quality && !s->broken) return PT_OK;
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return build_tree_products(s, quality, s->d_wide8 != nullptr);
    }
    if (s->broken) {  // a small scene that lost its tree in a failed pt_scene_update: the LBVH first (and any parked instances), then as asked
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const pt_status rb = build_tree_products(s, quality, true);
        if (rb != PT_OK) return rb;
    }
    const bool want_sah = quality == PT_BVH_PREFER_FAST_TRACE && s->n_tris <= PT_SAH_MAX_TRIS && s->d_tri_orig;
    if (want_sah == (s->bvh4_builder == 1u)) return PT_OK;
    hipStream_t st = ctx->stream;
    const uint32_t n = s->n_tris;
    if (want_sah && !s->d_wide_sah) {
        const float pad = leaf_pad_of(s->bmin, s->bmax);
        std::vector<uint32_t> rows, order;
        // one primitive per leaf, a primitive being a triangle or a quad's two halves (pt_tuning.pair_leaves = 0: the former
        // rule, up to PT_SAH_LEAF_MAX independent triangles per leaf where splitting does not pay); built on the device
        const bool pairs = ctx->tune.pair_leaves != 0;
        const pt_status rc8 = pt_sah_build_bvh4_device(ctx, s->h_tlo.data(), s->h_thi.data(), n, pairs ? s->h_pair.data() : nullptr, pad,
                                                       pairs ? 1u : PT_SAH_LEAF_MAX, rows, order);
        if (rc8 != PT_OK) return rc8;
        if (order.size() != n || rows.empty()) { ctx->err = "internal: SAH build lost triangles"; return PT_ERR_HIP; }
        // (the scene has the surface-area tree from here on, or nothing of it)
        PT_TRY(alloc_filled(s, "the surface-area BVH4", { pt_buf_of(s->d_wide_sah, rows.size() * sizeof(uint32_t)), pt_buf_of(s->d_prim_of_sah, sizeof(uint32_t) * n) },
                            { rows.data(), order.data() }));
        s->sah_pair_leaves = pairs;
        s->n_wide_sah = (uint32_t)(rows.size() / 32);
        s->stack_need_sah = pt_wide_stack_need(rows);
    }
    PT_HIP(ctx, hipStreamSynchronize(st));  // nothing may still be traversing the old tables
    if (want_sah) {
        s->d_wide = s->d_wide_sah; s->n_wide = s->n_wide_sah; s->stack_need = s->stack_need_sah; s->bvh4_builder = 1;
        s->pair_leaves = s->sah_pair_leaves;
    } else {
        s->d_wide = s->d_wide_lbvh; s->n_wide = s->n_wide_lbvh; s->stack_need = s->stack_need_lbvh; s->bvh4_builder = 0;
        s->pair_leaves = PT_BLAS_LEAF_MAX == 1u;  // 1-triangle leaves are the degenerate case of the pair kernel
    }
    k_pack<<<(n + TB - 1) / TB, TB, 0, st>>>(s->d_tri_orig, s->d_faces, want_sah ? s->d_prim_of_sah : s->d_prim_of, n, s->d_tri4,
                                           s->d_shade4, s->d_shade64, s->d_ke4, s->d_frame4);
    pack_self_leaf(s, st);
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    pt_scratch_free({ pt_buf_of(s->d_inst_frame) }, nullptr, 0);  // (the triangle order changed: ptb_ensure_inst_frames builds it again on the next render)
    set_device_bytes(s);
    s->quality = quality;
    const pt_status rc = make_wide16(s);
    if (rc != PT_OK) mark_broken(s, quality);  // the tables are the new tree's and its fp16 nodes are missing: nothing to traverse until a repair
    return rc;
}

void ptb_free_scene_buffers(pt_scene *s)
{
    free_tree_products(s);
    pt_scratch_free(ptb_scene_buffers(s, PT_LIFE_SOURCE), nullptr, 0);
    s->n_lights = 0;
}

// ---- instances: TLAS over world boxes of the transformed BLAS root box --------------------------
// (beyond the reference, which builds ONE identity instance, main.cpp:515-538)
__global__ __launch_bounds__(TB) void k_inst_boxes(const float4 *__restrict__ blas_wide, const float4 *__restrict__ inst6,
                                                   uint32_t n, float4 *__restrict__ tlo, float4 *__restrict__ thi)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    // object box = union of the (padded) child boxes of the BLAS root
    float omin[3] = { INFINITY, INFINITY, INFINITY }, omax[3] = { -INFINITY, -INFINITY, -INFINITY };
    const float4 lx = blas_wide[0], ly = blas_wide[1], lz = blas_wide[2], hx = blas_wide[3], hy = blas_wide[4], hz = blas_wide[5];
    const float4 cw = blas_wide[6];
    const float l[3][4] = { { lx.x, lx.y, lx.z, lx.w }, { ly.x, ly.y, ly.z, ly.w }, { lz.x, lz.y, lz.z, lz.w } };
    const float h[3][4] = { { hx.x, hx.y, hx.z, hx.w }, { hy.x, hy.y, hy.z, hy.w }, { hz.x, hz.y, hz.z, hz.w } };
    const uint32_t w[4] = { __float_as_uint(cw.x), __float_as_uint(cw.y), __float_as_uint(cw.z), __float_as_uint(cw.w) };
    for (int c = 0; c < 4; c++)
        if (w[c] != PT_MISS)
            for (int k = 0; k < 3; k++) { omin[k] = fminf(omin[k], l[k][c]); omax[k] = fmaxf(omax[k], h[k][c]); }
    const float4 m0 = inst6[6 * (size_t)i + 0], m1 = inst6[6 * (size_t)i + 1], m2 = inst6[6 * (size_t)i + 2];
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int c = 0; c < 8; c++) {
        const float px = (c & 1) ? omax[0] : omin[0], py = (c & 2) ? omax[1] : omin[1], pz = (c & 4) ? omax[2] : omin[2];
        const float wx = ((m0.x * px + m0.y * py) + m0.z * pz) + m0.w;
        const float wy = ((m1.x * px + m1.y * py) + m1.z * pz) + m1.w;
        const float wz = ((m2.x * px + m2.y * py) + m2.z * pz) + m2.w;
        mn[0] = fminf(mn[0], wx); mn[1] = fminf(mn[1], wy); mn[2] = fminf(mn[2], wz);
        mx[0] = fmaxf(mx[0], wx); mx[1] = fmaxf(mx[1], wy); mx[2] = fmaxf(mx[2], wz);
    }
    tlo[i] = make_float4(mn[0], mn[1], mn[2], 0.f);
    thi[i] = make_float4(mx[0], mx[1], mx[2], 0.f);
}

__global__ __launch_bounds__(TB) void k_inst_sort(const float4 *__restrict__ inst6, const uint32_t *__restrict__ prim_of,
                                                  uint32_t n, float4 *__restrict__ sorted6)
{
    const uint32_t pos = blockIdx.x * TB + threadIdx.x;
    if (pos >= n) return;
    const uint32_t id = prim_of[pos];
    for (int k = 0; k < 6; k++) sorted6[6 * (size_t)pos + k] = inst6[6 * (size_t)id + k];
}

// (world -> object matrix: si_invert_3x4, scene_instances_kernel.h -- adjugate / determinant in binary64, rounded once to float)

// World-space normal and tangent of every (instance, triangle): what k_shade's instanced branch used to evaluate per hit -- the
// normal by the inverse transpose, renormalised (a square root and three true divides), and createCoordinateSystem on it (another
// square root and two divides) -- evaluated ONCE with exactly those operations (shade_kernels.hip k_shade; pt_math.h tangent_frame),
// so the bits are the same.  32 B per entry: {n.xyz, T.x} {T.yz, -, -}; the bitangent is the cross product k_shade forms anyway.
// Instance order = d_inst6's (TLAS leaf order), triangle order = d_shade4's (BVH4 leaf order): rebuilt when either changes.
__global__ __launch_bounds__(TB) void k_inst_frames(const float4 *__restrict__ inst6, const float4 *__restrict__ shade4, uint32_t n_inst,
                                                    uint32_t n_tris, float4 *__restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * TB + threadIdx.x;
    if (idx >= (size_t)n_inst * n_tris) return;
    const uint32_t ip = (uint32_t)(idx / n_tris), pos = (uint32_t)(idx - (size_t)ip * n_tris);
    const float4 s0 = shade4[3 * (size_t)pos];
    const float4 i0 = inst6[6 * (size_t)ip + 3], i1 = inst6[6 * (size_t)ip + 4], i2 = inst6[6 * (size_t)ip + 5];
    const float nx = (i0.x * s0.x + i1.x * s0.y) + i2.x * s0.z;
    const float ny = (i0.y * s0.x + i1.y * s0.y) + i2.y * s0.z;
    const float nz = (i0.z * s0.x + i1.z * s0.y) + i2.z * s0.z;
    const float l = ptm::fsqrt((nx * nx + ny * ny) + nz * nz);
    const ptm::f3 n = { ptm::fdiv(nx, l), ptm::fdiv(ny, l), ptm::fdiv(nz, l) };
    ptm::f3 T, B;
    ptm::tangent_frame(n, T, B);
    out[2 * idx + 0] = make_float4(n.x, n.y, n.z, T.x);
    out[2 * idx + 1] = make_float4(T.y, T.z, 0.f, 0.f);
}

pt_status ptb_ensure_inst_frames(pt_scene *s)
{
    pt_ctx *ctx = s->ctx;
    if (!s->n_inst || s->d_inst_frame) return PT_OK;
    const size_t entries = (size_t)s->n_inst * s->n_tris;
    if (entries * 32 > (512ull << 20)) return PT_OK;  // (a table beyond the caches would cost more than it saves: the per-hit transform stays)
    PT_TRY(ptb_scene_alloc(s, "the instances' frame table", { pt_buf_of(s->d_inst_frame, 32 * entries) }));
    k_inst_frames<<<(unsigned)((entries + TB - 1) / TB), TB, 0, ctx->stream>>>(s->d_inst6, s->d_shade4, s->n_inst, s->n_tris, s->d_inst_frame);
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipGetLastError());
    return PT_OK;
}

// Emitters of the NEE pipeline for an instanced scene: every instance's copy, in gl_InstanceID order, vertices taken to world
// space by the instance's matrix with the operation order of the shading transform; normal and area from the world-space
// triangle; one running cdf over all of them (the tests' CPU checker restates this loop).  Built on the first NEE render of
// the instance set -- 80 B per (instance, emitter) on host and device, nothing a scene that never samples lights should pay --
// and refused beyond 2^24 copies (1.3 GB; the float running sum of the areas stops resolving small emitters well before).
pt_status ptb_ensure_inst_lights(pt_scene *s)
{
    pt_ctx *ctx = s->ctx;
    if (!s->n_inst || !s->n_lights || s->d_lights_inst) return PT_OK;
    const uint64_t copies = (uint64_t)s->n_inst * s->n_lights;
    if (copies > (1ull << 24) || pt_given_instances(s) != (size_t)s->n_inst) {
        ctx->err = "the NEE pipeline would need " + std::to_string(copies) + " world-space emitter copies (instances x emitters); the limit is 16 777 216";
        return PT_ERR_UNSUPPORTED;
    }
    if (s->d_xforms) return ptsi_inst_lights(s);  // the set lives on the device: the same loop as a kernel (scene_instances.hip)
    const uint32_t n = s->n_inst;
    const float *xforms3x4 = s->h_xforms.data();
    std::vector<float4> wl;
    wl.reserve(5 * (size_t)copies);
    float run = 0.f;
    for (uint32_t i = 0; i < n; i++) {
        const float *m = xforms3x4 + 12 * (size_t)i;
        for (uint32_t k = 0; k < s->n_lights; k++) {
            float w[3][3];
            for (int c = 0; c < 3; c++) {
                const float4 v = s->h_lights[5 * (size_t)k + c];
                for (int r = 0; r < 3; r++) w[c][r] = ((m[4 * r] * v.x + m[4 * r + 1] * v.y) + m[4 * r + 2] * v.z) + m[4 * r + 3];
            }
            push_emitter(w[0], w[1], w[2], s->h_lights[5 * (size_t)k + 4], run, wl);
        }
    }
    PT_TRY(alloc_filled(s, "the instanced emitter table", { pt_buf_of(s->d_lights_inst, sizeof(float4) * wl.size()) }, { wl.data() }));
    s->n_lights_inst = (uint32_t)copies;
    s->light_area_inst = run;
    return PT_OK;
}

void ptb_free_instances(pt_scene *s)
{
    s->h_xforms.clear();
    s->h_xforms.shrink_to_fit();
    pt_scratch_free(ptb_scene_buffers(s, PT_LIFE_INSTANCES), nullptr, 0);
    pt_scratch_free(ptb_scene_buffers(s, PT_LIFE_GIVEN), nullptr, 0);
    s->n_xforms_dev = 0;
    s->n_lights_inst = 0; s->light_area_inst = 0.f;
    s->n_tlas16 = 0;
    s->n_inst = 0; s->n_tlas_wide = 0; s->tlas_height = 0;
}

static pt_status set_instances_from_records(pt_scene *s, DevBuf<float4> &d_in, uint32_t n, const float *h_given, DevBuf<float4> &d_given);

pt_status ptb_set_instances(pt_scene *s, const float *xforms3x4, uint32_t n)
{
    pt_ctx *ctx = s->ctx;
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ptb_free_instances(s);
    if (n == 0) return PT_OK;
    if (s->broken) { ctx->err = PT_BROKEN_SCENE_MSG; return PT_ERR_UNSUPPORTED; }
    std::vector<float> rec(24 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        const float *m = xforms3x4 + 12 * (size_t)i;
        for (int k = 0; k < 12; k++) {
            if (!(m[k] == m[k]) || __builtin_isinf(m[k])) { ctx->err = "instance matrix has a NaN/Inf"; return PT_ERR_INVALID_ARG; }
            rec[24 * (size_t)i + k] = m[k];
        }
        si_invert_3x4(m, &rec[24 * (size_t)i + 12]);
        for (int k = 12; k < 24; k++)
            if (!(rec[24 * (size_t)i + k] == rec[24 * (size_t)i + k]) || __builtin_isinf(rec[24 * (size_t)i + k])) {
                ctx->err = "instance matrix is singular";
                return PT_ERR_INVALID_ARG;
            }
    }
    DevBuf<float4> d_in;
    PT_HIP(ctx, d_in.alloc(6 * (size_t)n));
    PT_HIP(ctx, hipMemcpy(d_in.p, rec.data(), sizeof(float) * 24 * (size_t)n, hipMemcpyHostToDevice));
    DevBuf<float4> none;
    return set_instances_from_records(s, d_in, n, xforms3x4, none);
}

// The matrices in device memory: the same refusals decided by a kernel (scene_instances.hip), one verdict word back; the records never leave
// the device and the set as given is kept there (d_xforms) for what the host call keeps h_xforms for.
pt_status ptb_set_instances_device(pt_scene *s, const float *d_xforms3x4, uint32_t n)
{
    pt_ctx *ctx = s->ctx;
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ptb_free_instances(s);
    if (n == 0) return PT_OK;
    if (s->broken) { ctx->err = PT_BROKEN_SCENE_MSG; return PT_ERR_UNSUPPORTED; }
    DevBuf<float4> d_in, d_kept;
    DevBuf<uint32_t> d_verdict;
    PT_HIP(ctx, d_in.alloc(6 * (size_t)n));
    PT_HIP(ctx, d_kept.alloc(3 * (size_t)n));
    PT_HIP(ctx, d_verdict.alloc(1));
    uint32_t verdict = SI_OK;
    PT_TRY(ptsi_check_invert(ctx, d_xforms3x4, n, d_in.p, d_kept.p, d_verdict.p, &verdict));
    if (verdict != SI_OK) {
        ctx->err = (verdict & 1u) ? "instance matrix is singular" : "instance matrix has a NaN/Inf";
        return PT_ERR_INVALID_ARG;
    }
    return set_instances_from_records(s, d_in, n, nullptr, d_kept);
}

// d_in: the n records {m, inv} in gl_InstanceID order.  On success the scene keeps the set as given: h_given's copy, or d_given itself.
static pt_status set_instances_from_records(pt_scene *s, DevBuf<float4> &d_in, uint32_t n, const float *h_given, DevBuf<float4> &d_given)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    // nothing hangs on the scene before the whole set -- the TLAS and the sorted matrices -- exists: a failure leaves it single-level
    DevBuf<float4> d_tlo, d_thi, d_inst6;
    PT_HIP(ctx, d_tlo.alloc(n));
    PT_HIP(ctx, d_thi.alloc(n));
    const uint32_t g = (n + TB - 1) / TB;
    k_inst_boxes<<<g, TB, 0, st>>>(s->d_wide, d_in.p, n, d_tlo.p, d_thi.p);
    BvhOut o;
    // (n < 32768: also the top-down 64-B TLAS with 16-bit child codes that k_extend_inst16 walks)
    // (pt_tuning.tlas_ploc = 1: the TLAS's binary tree by PLOC, as for big single-level scenes; kept under the same area rule)
    PT_TRY(ptb_build_bvh(ctx, d_tlo.p, d_thi.p, n, PT_TLAS_LEAF_MAX, o, (n > 1 && n < 32768u && PT_TLAS_LEAF_MAX == 1u) ? 6 : 0,
                         ctx->tune.tlas_ploc == 1 && n > 2));
    // (a TLAS has no read-back.  Its keys and binary nodes go BEFORE the sorted matrices are allocated: with the matrices allocated first
    // the call measured 1.13-1.24 ms instead of 0.91-1.07 for 10 000 instances, profiles/scene_buffers_refactor_ab.json)
    o.d_keys.free();
    o.d_nodes.free();
    DevBuf<uint32_t> &prim_of = o.d_prim_q.p ? o.d_prim_q : o.d_prim_of;   // the leaf order of the tree that is walked
    PT_TRY(ptb_scene_alloc(s, "the instance matrices", { pt_buf_of(d_inst6.p, sizeof(float4) * 6 * (size_t)n) }));
    k_inst_sort<<<g, TB, 0, st>>>(d_in.p, prim_of.p, n, d_inst6.p);
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    s->d_tlas_wide = o.d_wide.release();
    s->d_tlas_prim_of = prim_of.release();
    s->d_tlas16 = o.d_wide16t.release(); s->n_tlas16 = o.n_wide16t; s->tlas16_levels = o.levels4t;
    s->d_inst6 = d_inst6.release();
    s->tlas_area_lbvh = o.area_lbvh; s->tlas_area_ploc = o.area_ploc;
    for (int k = 0; k < 3; k++) { s->tlas_norm_c[k] = o.norm_c[k]; s->tlas_norm_s[k] = o.norm_s[k]; s->tlas_norm_rs[k] = o.norm_rs[k]; }
    for (int k = 0; k < 3; k++) { s->tlas_bmin[k] = o.bmin[k]; s->tlas_bmax[k] = o.bmax[k]; }
    // (the emitters' world-space copies for the NEE pipeline are made on that pipeline's first render: ptb_ensure_inst_lights)
    if (h_given) s->h_xforms.assign(h_given, h_given + 12 * (size_t)n);
    else { s->d_xforms = d_given.release(); s->n_xforms_dev = n; }
    s->xf_set++;
    s->n_inst = n;
    s->n_tlas_wide = o.n_wide;
    s->tlas_height = std::max(o.height, o.height_tree);  // (of the tree the TLAS was collapsed from: the stack bound)
    return PT_OK;
}

// ---- pt_scene_update: new vertex positions (and indices) for the same triangles ----------------------------------------------
// REFIT keeps the topology of every tree the scene holds and recomputes what depends on positions: the kept triangles, the binary
// LBVH (k_refit), every wide tree in place (bvh_refit.hip), the fp16 copy of the traversed BVH4 on the new scene box, the per-triangle
// tables in their leaf orders, the emitters, the small scenes' host boxes.  Traversal only needs conservative boxes and reports the
// closest t / lowest primitive id, so images and hit records are those of a fresh scene; only the walk's cost drifts (pt_scene_info
// .tree_area_lbvh shows it).  A fan pair whose shared vertices no longer coincide cannot stay one leaf (the pair test reads only the
// second triangle's fourth vertex): the update is then a REBUILD, which builds the tree products afresh at the scene's quality.
static pt_status refit_tree_products(pt_scene *s, const float4 *d_tlo, const float4 *d_thi)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t n = s->n_tris, gt = (n + TB - 1) / TB;
    double area = s->area_lbvh;
    pt_status rc = ptb_refit_lbvh(ctx, d_tlo, d_thi, s->d_prim_of, n, s->d_nodes, s->bmin, s->bmax, &area);
    if (rc != PT_OK) return rc;
    s->area_lbvh = area;
    ptb_norm_box(s->bmin, s->bmax, s->norm_c, s->norm_s, s->norm_rs);
    const float pad = leaf_pad_of(s->bmin, s->bmax);
    // leaf positions of the binary tree the collapses ran on: the PLOC tree's (builder 2), else the LBVH's
    const uint32_t *kept = s->bvh4_builder == 2u ? s->d_prim_of_sah : s->d_prim_of;
    rc = ptb_refit_wide(ctx, 0, s->d_wide_lbvh, s->n_wide_lbvh, d_tlo, d_thi, kept, n, pad, s->norm_c, s->norm_rs);
    if (rc == PT_OK && s->d_wide_sah)
        rc = ptb_refit_wide(ctx, 0, s->d_wide_sah, s->n_wide_sah, d_tlo, d_thi, s->d_prim_of_sah, n, pad, s->norm_c, s->norm_rs);
    if (rc == PT_OK && s->d_wide16t)
        rc = ptb_refit_wide(ctx, 1, s->d_wide16t, s->n_wide16t, d_tlo, d_thi, kept, n, pad, s->norm_c, s->norm_rs);
    if (rc == PT_OK && s->d_wide8)
        rc = ptb_refit_wide(ctx, 2, s->d_wide8, s->n_wide8, d_tlo, d_thi, s->d_prim_of8, n, pad, s->norm_c, s->norm_rs);
    if (rc != PT_OK) return rc;
    const uint32_t *order = traversed_order(s);
    if (s->d_wide8)  // (d_shade4 is scratch here: the k_pack below writes it)
        k_pack<<<gt, TB, 0, st>>>(s->d_tri_orig, s->d_faces, s->d_prim_of8, n, s->d_tri4_8, s->d_shade4, s->d_shade64_8, s->d_ke4_8);
    k_pack<<<gt, TB, 0, st>>>(s->d_tri_orig, s->d_faces, order, n, s->d_tri4, s->d_shade4, s->d_shade64, s->d_ke4, s->d_frame4);
    pack_self_leaf(s, st);
    k_wide_half<<<(s->n_wide + TB - 1) / TB, TB, 0, st>>>(s->d_wide, s->n_wide, s->norm_c[0], s->norm_c[1], s->norm_c[2], s->norm_rs[0],
                                                         s->norm_rs[1], s->norm_rs[2], reinterpret_cast<uint4 *>(s->d_wide16));
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipStreamSynchronize(st));
    return PT_OK;
}

static pt_status update_tree_products(pt_scene *s, const float4 *d_tlo, const float4 *d_thi, bool refit, bool upload_lights)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const bool small = s->n_tris <= PT_SAH_MAX_TRIS;
    if (s->n_lights && upload_lights) PT_HIP(ctx, hipMemcpyAsync(s->d_lights, s->h_lights.data(), sizeof(float4) * s->h_lights.size(), hipMemcpyHostToDevice, st));
    if (small) PT_TRY(keep_host_boxes(s, d_tlo, d_thi));
    if (refit) {
        const pt_status rc = refit_tree_products(s, d_tlo, d_thi);
        if (rc != PT_OK) return rc;
        PT_HIP(ctx, hipEventRecord(ctx->ev_b, st));
        PT_HIP(ctx, hipStreamSynchronize(st));
        PT_HIP(ctx, hipEventElapsedTime(&s->build_ms, ctx->ev_a, ctx->ev_b));
        return PT_OK;
    }
    // REBUILD (or a refit that cannot keep its pair leaves): what pt_scene_create builds, at the scene's quality
    return build_at_quality(s, s->quality, small || s->d_wide8 != nullptr || ctx->tune.hbm8 == 1);
}

pt_status ptb_update_scene(pt_scene *s, const pt_geometry &g, uint32_t mode)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t n = s->n_tris;
    const bool small = n <= PT_SAH_MAX_TRIS;
    const float *h_vertices = g.vertices;  // (host pointers on the host path only)
    const uint32_t *h_indices = g.indices;
    PT_HIP(ctx, hipStreamSynchronize(st));  // after whatever is queued on the scene (a PT_FLAG_ASYNC render included)
    // host-side products first: until the triangles are overwritten below, a failure leaves the scene as it was
    // (arrays in device memory: the same products by kernels from the gathered triangles, below)
    std::vector<float4> lights;
    float run = 0.f;
    for (size_t k = 0; k < s->h_light_prim.size() && !g.on_device; k++) {
        const uint32_t t = s->h_light_prim[k];
        push_emitter(h_vertices + 3 * (size_t)h_indices[3 * (size_t)t + 0], h_vertices + 3 * (size_t)h_indices[3 * (size_t)t + 1],
                     h_vertices + 3 * (size_t)h_indices[3 * (size_t)t + 2], s->h_lights[5 * k + 4], run, lights);
    }
    std::vector<uint8_t> pair;
    if (small && !g.on_device) find_fan_pairs(h_vertices, h_indices, n, pair);
    GeometryUpload up;
    PT_TRY(up.upload(ctx, g, n));
    PT_HIP(ctx, hipEventRecord(ctx->ev_a, st));
    // from here on the scene holds the new triangles: a failure marks it broken (the repair builds from them, never from a mix)
    const uint32_t quality = s->quality;
    const std::vector<float> xforms = s->h_xforms;  // the instance set -- or the one an earlier failed update parked (restore_parked_instances)
    float4 *const d_xforms = s->d_xforms;           // ... given in device memory: the buffer itself is carried across
    const uint32_t n_xforms_dev = s->n_xforms_dev;
    const uint32_t n_inst = (uint32_t)pt_given_instances(s);
    s->d_xforms = nullptr;
    if (n_inst) ptb_free_instances(s);  // the TLAS, the instances' frames and emitters are made again from the new BLAS below
    up.gather(s);
    pt_status rc = PT_OK;
    if (g.on_device) {  // scene_device.hip: d_lights, h_lights and light_area; the pair relation (none where it could not be read: always a valid one)
        rc = ptsd_host_products(s, small ? &pair : nullptr);
        if (small && rc != PT_OK) pair.assign(n, 0);
    } else {
        s->h_lights = lights;
        s->light_area = run;
    }
    bool pairs_hold = true;  // every pair leaf of the held trees is still a pair (a pair that newly forms changes no bits)
    for (uint32_t i = 0; i < s->h_pair.size() && i < pair.size(); i++)
        if (s->h_pair[i] && !pair[i]) pairs_hold = false;
    const bool refit = mode == PT_SCENE_UPDATE_REFIT && !s->broken && (pairs_hold || !s->d_wide_sah || !s->sah_pair_leaves);
    // the fan-pair relation a later surface-area build reads: the new arrays' (a pair-leaf tree the refit keeps has only pairs that still hold)
    if (small) s->h_pair = pair;
    if (rc == PT_OK) rc = update_tree_products(s, up.d_tlo.p, up.d_thi.p, refit, !g.on_device);
    if (rc != PT_OK) mark_broken(s, quality);
    if (n_inst) { s->h_xforms = xforms; s->d_xforms = d_xforms; s->n_xforms_dev = n_xforms_dev; }  // parked: set again below, or by the next successful build of the broken scene
    if (rc != PT_OK) return rc;
    return restore_parked_instances(s, quality);
}

// ---- pt_scene_set_faces / pt_scene_set_faces_device: new per-face materials for the same triangles -------
// No tree, node or geometry table depends on a material.  What does: the kept copy d_faces (a rebuild, a quality change and the first 8-wide
// request re-pack from it), the material words of the per-triangle tables (scene_faces.hip), the emitter set of the NEE pipelines (scene_device.hip's
// kernels, the host loop's bits) and, instanced, its world-space copies (dropped: the next NEE render makes them again).  Everything the call
// allocates or reads back happens on a STAGED copy of the faces and a STAGED emitter set, before the first write to anything the scene owns: a
// call that fails leaves the scene rendering the old materials, never a mix.
static pt_status set_faces_staged(pt_scene *s, const float *faces, bool on_device, DevBuf<float> &d_new, pt_staged_emitters &em)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const size_t bytes = sizeof(float) * 6 * (size_t)s->n_tris;
    PT_TRY(pt_scratch_alloc(ctx, "the staged materials", { pt_buf_of(d_new.p, bytes) }, nullptr, 0));
    PT_HIP(ctx, hipMemcpyAsync(d_new.p, faces, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    PT_TRY(ptsd_find_emitters(s, d_new.p, em.set()));             // the count and the ids come back ...
    PT_TRY(ptsd_host_products(s, d_new.p, em.set(), nullptr));    // ... then the records and their total area
    // nothing below allocates or reads back: the material words in place, then the swap
    ptsf_launch_set_faces(s, d_new.p, traversed_order(s), st);
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipStreamSynchronize(st));
    return PT_OK;
}

pt_status ptb_set_faces(pt_scene *s, const float *faces, bool on_device)
{
    pt_ctx *ctx = s->ctx;
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // after whatever is queued on the scene (a PT_FLAG_ASYNC render included)
    if (s->broken) { ctx->err = PT_BROKEN_SCENE_MSG; return PT_ERR_UNSUPPORTED; }
    DevBuf<float> d_new;
    pt_staged_emitters em;
    const pt_status rc = set_faces_staged(s, faces, on_device, d_new, em);
    if (rc != PT_OK) {  // (nothing queued may outlive the staged set it writes to)
        const std::string err = ctx->err;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipGetLastError();
        ctx->err = err;
        return rc;
    }
    std::swap(s->d_faces, d_new.p);  // (the old copy goes with d_new)
    std::swap(s->d_lights, em.d_lights);
    std::swap(s->d_light_prim, em.d_light_prim);  // never the ids of another emitter set: refreshed with the set, or gone with it
    s->n_lights = em.n_lights;
    s->light_area = em.light_area;
    s->h_lights.swap(em.h_lights);
    s->h_light_prim.swap(em.h_light_prim);
    // the instances' world-space emitter copies were the old set's: ptb_ensure_inst_lights / ptsi_inst_lights make them again on the next NEE render
    pt_scratch_free({ pt_buf_of(s->d_lights_inst) }, nullptr, 0);
    s->n_lights_inst = 0; s->light_area_inst = 0.f;
    return PT_OK;
}
