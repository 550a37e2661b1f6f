// guided_kernel.h -- pt_render_guided: the first-hit log the fused kernels write (fused_kernel.h, fused_inst_kernel.h: LOG) and the per-pixel body
// of k_guided_reduce (guided.hip), which folds it into the guide planes -- in a header of its own, like adaptive_kernel.h, so that
// tests/guided_host.cpp can compile the very same statements for the host and hold them against the numpy restatement of DESIGN.md section 12
// without a GPU, under the host's sanitizers.  The eleven sums, their fold and their blend are pt_render_aov's (aov.hip includes this header for them).
// Wants declared before it: ptm::fdiv, ptm::fsqrt (pt_math.h), uint2, float4, make_uint2, __float_as_uint, PT_MISS.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- the guide planes and a pixel's eleven running sums: one frame's, or the plane values (pt_render_aov, pt_render_guided) ------------------
struct AovPlanes {
    float *albedo, *normal, *emission, *depth, *alpha;
    uint2 *id;
};
struct Guide {
    float ar, ag, ab, nx, ny, nz, er, eg, eb, d, a;
};
__device__ __forceinline__ void guide_add(Guide &g, const Guide &v)
{
    g.ar = g.ar + v.ar; g.ag = g.ag + v.ag; g.ab = g.ab + v.ab;
    g.nx = g.nx + v.nx; g.ny = g.ny + v.ny; g.nz = g.nz + v.nz;
    g.er = g.er + v.er; g.eg = g.eg + v.eg; g.eb = g.eb + v.eb;
    g.d = g.d + v.d; g.a = g.a + v.a;
}
// raygen.rgen:86, 88-90 per channel: sum / spp, then (value + old * frame) / (frame + 1)
__device__ __forceinline__ float blend1(float sum, float spp, float old, bool first, float ff, float f1)
{
    return ptm::fdiv(ptm::fdiv(sum, spp) + (first ? 0.f : old) * ff, f1);
}
__device__ __forceinline__ void guide_blend(Guide &acc, const Guide &sum, float spp, int32_t frame)
{
    const float ff = (float)frame, f1 = (float)(frame + 1);
    const bool first = frame == 0;
    acc.ar = blend1(sum.ar, spp, acc.ar, first, ff, f1); acc.ag = blend1(sum.ag, spp, acc.ag, first, ff, f1); acc.ab = blend1(sum.ab, spp, acc.ab, first, ff, f1);
    acc.nx = blend1(sum.nx, spp, acc.nx, first, ff, f1); acc.ny = blend1(sum.ny, spp, acc.ny, first, ff, f1); acc.nz = blend1(sum.nz, spp, acc.nz, first, ff, f1);
    acc.er = blend1(sum.er, spp, acc.er, first, ff, f1); acc.eg = blend1(sum.eg, spp, acc.eg, first, ff, f1); acc.eb = blend1(sum.eb, spp, acc.eb, first, ff, f1);
    acc.d = blend1(sum.d, spp, acc.d, first, ff, f1); acc.a = blend1(sum.a, spp, acc.a, first, ff, f1);
}
__device__ __forceinline__ Guide guide_load(const AovPlanes &pl, size_t pix)
{
    Guide g;
    g.ar = pl.albedo[3 * pix + 0]; g.ag = pl.albedo[3 * pix + 1]; g.ab = pl.albedo[3 * pix + 2];
    g.nx = pl.normal[3 * pix + 0]; g.ny = pl.normal[3 * pix + 1]; g.nz = pl.normal[3 * pix + 2];
    g.er = pl.emission[3 * pix + 0]; g.eg = pl.emission[3 * pix + 1]; g.eb = pl.emission[3 * pix + 2];
    g.d = pl.depth[pix]; g.a = pl.alpha[pix];
    return g;
}
__device__ __forceinline__ void guide_store(const AovPlanes &pl, size_t pix, const Guide &g)
{
    pl.albedo[3 * pix + 0] = g.ar; pl.albedo[3 * pix + 1] = g.ag; pl.albedo[3 * pix + 2] = g.ab;
    pl.normal[3 * pix + 0] = g.nx; pl.normal[3 * pix + 1] = g.ny; pl.normal[3 * pix + 2] = g.nz;
    pl.emission[3 * pix + 0] = g.er; pl.emission[3 * pix + 1] = g.eg; pl.emission[3 * pix + 2] = g.eb;
    pl.depth[pix] = g.d; pl.alpha[pix] = g.a;
}

// ---- the first-hit log of a fused launch ------------------------------------------------------------------------------------------------------
// One 8-byte record per camera ray: {leaf position of the triangle (two-level: | TLAS leaf position of the instance << 11), bits(t)}; a miss has
// PT_MISS in its first word.  Record of sample s of the pixel at position `local` of the launch's tile list, in frame f of the launch:
// ((f * spp) + s) * slots_per_lane + local -- sample-major, so that the 64 pixels of a tile lie side by side: the reduce's threads, one per pixel,
// read a sample's records as whole lines, and a wave's lanes, which hold pixels of few tiles, write theirs near each other.  (Pixel-major --
// k_aov_reduce's ray = pixel * spp + sample -- was measured first: a thread then strides 8 * spp bytes and the reduce of one 1080p frame at 32 spp
// took 0.76 ms, as long as the trace it replaces: DESIGN.md section 20.)
__device__ __forceinline__ size_t gd_log_index(uint32_t f, uint32_t local, uint32_t sample, uint32_t slots_per_lane, uint32_t spp)
{
    return ((size_t)f * spp + sample) * slots_per_lane + local;
}
constexpr uint32_t GD_POS_BITS = 11;  // k_fused_inst's class: <= 2047 triangles in the BLAS, < 32768 instances
// (a miss holds PT_MISS, all ones, in both: the packed word is PT_MISS again)
__device__ __forceinline__ uint32_t gd_pack_inst(uint32_t pos, uint32_t ipos) { return pos | (ipos << GD_POS_BITS); }

struct GdConst {
    uint32_t width, height, spp;
    uint32_t slots_per_lane;   // 64 * tiles of the launch's list: the pixels of a frame in the log
    uint32_t n_tris;           // (two-level: the row length of the inst_frame table)
    uint32_t cull_on;          // RenderConst::cull of the launch: the pixels it finished without a walk, which have NO records -- all misses
    int32_t cull[4];
};
struct GdScene {
    const float4 *tri4;        // 3 float4 per leaf position, [0].w = bits(prim)
    const float4 *shade4;      // 3 float4 per leaf position, [0].xyz = the normal k_shade uses
    const float *faces;        // Kd, Ke in primitive order (6 floats)
    const float4 *inst6;       // two-level: 6 float4 per instance in TLAS leaf order, rows 3..5 world -> object
    const float4 *inst_frame;  // ... the (instance, triangle) normal table, or null: the inverse transpose
    const uint32_t *inst_id;   // ... TLAS leaf position -> gl_InstanceID
};

// The pixel at position `local` of the tile list: the records of frames [frame0, frame0 + n_frames) of the launch, folded in sample order and
// blended into the planes frame after frame (k_aov_reduce's arithmetic; between two frames the plane values stay in registers -- a float stored
// and loaded is the same float).  id_frame: the frame of the launch (0 .. n_frames - 1) whose sample 0 gives the id plane -- the call's last --
// or >= n_frames when that frame is in a later launch.
template <bool INST>
__device__ __forceinline__ void gd_reduce_pixel(const GdConst &gc, const uint32_t *__restrict__ tiles, uint32_t local, int32_t frame0, uint32_t n_frames,
                                                uint32_t id_frame, const uint2 *__restrict__ log, const GdScene &sc, const AovPlanes &planes)
{
    const uint32_t g = tiles[local >> 6];  // tile x | tile y << 16
    const uint32_t px = (g & 0xFFFFu) * 8u + (local & 7u), py = (g >> 16) * 8u + ((local >> 3) & 7u);
    if (px >= gc.width || py >= gc.height) return;  // beyond the image's edge: no slot was started, no record written
    const bool culled = gc.cull_on && ((int32_t)px < gc.cull[0] || (int32_t)px > gc.cull[2] || (int32_t)py < gc.cull[1] || (int32_t)py > gc.cull[3]);
    const size_t o = (size_t)py * gc.width + px;
    Guide acc = {};
    if (frame0 != 0) acc = guide_load(planes, o);
    for (uint32_t k = 0; k < n_frames; k++) {
        Guide sum = {};
        uint2 id = make_uint2(PT_MISS, PT_MISS);
        for (uint32_t s = 0; s < gc.spp; s++) {
            Guide v = {};
            if (!culled) {
                const uint2 h = log[gd_log_index(k, local, s, gc.slots_per_lane, gc.spp)];
                if (h.x != PT_MISS) {
                    const uint32_t pos = INST ? (h.x & ((1u << GD_POS_BITS) - 1u)) : h.x;
                    const uint32_t prim = __float_as_uint(sc.tri4[3 * (size_t)pos].w);
                    const float *f = sc.faces + 6 * (size_t)prim;
                    const float4 n0 = sc.shade4[3 * (size_t)pos];
                    float nx = n0.x, ny = n0.y, nz = n0.z;
                    uint32_t inst = 0u;
                    if (INST) {  // the normal to world space as in k_shade<INST>: from the (instance, triangle) table, or by the inverse transpose
                        const uint32_t ip = h.x >> GD_POS_BITS;
                        inst = sc.inst_id[ip];
                        if (sc.inst_frame) {
                            const float4 f0 = sc.inst_frame[2 * ((size_t)ip * gc.n_tris + pos)];
                            nx = f0.x; ny = f0.y; nz = f0.z;
                        } else {
                            const float4 i0 = sc.inst6[6 * (size_t)ip + 3], i1 = sc.inst6[6 * (size_t)ip + 4], i2 = sc.inst6[6 * (size_t)ip + 5];
                            const float wx = (i0.x * nx + i1.x * ny) + i2.x * nz;
                            const float wy = (i0.y * nx + i1.y * ny) + i2.y * nz;
                            const float wz = (i0.z * nx + i1.z * ny) + i2.z * nz;
                            const float l = ptm::fsqrt((wx * wx + wy * wy) + wz * wz);
                            nx = ptm::fdiv(wx, l); ny = ptm::fdiv(wy, l); nz = ptm::fdiv(wz, l);
                        }
                    }
                    v = { f[0], f[1], f[2], nx, ny, nz, f[3], f[4], f[5], __uint_as_float(h.y), 1.0f };
                    if (s == 0u) id = make_uint2(prim, inst);
                }
            }
            guide_add(sum, v);
        }
        guide_blend(acc, sum, (float)gc.spp, frame0 + (int32_t)k);
        if (k == id_frame) planes.id[o] = id;
    }
    guide_store(planes, o, acc);
}
