// lds_scene.h -- the image of a scene in LDS: how it is staged (device) and how many bytes it takes (host and device), in one place.
//
//   fp32 nodes   160 B each (LDS_NODE_F4): the BVH4 node's planes, the low plane of every axis twice (lo hi lo), and its child words, kept
//                or re-coded to the 14-bit compact codes; k_extend_inst keeps the 128-B node as it is, padded to 144 B (LDS_NODE128_F4)
//   fp16 nodes    80 B each (I16_NODE_DW): the 64-B BVH4 node with 16-bit child codes; the TLAS's top levels behind the BLAS
//   triangles    three axis-permuted copies of tri4 (ptm::tri_test_perm needs no per-lane component selects)
// A kernel family that keeps a scene in LDS stages it with these helpers and its plan sizes it with the *_bytes functions; what a
// kernel keeps around the image (shading tables, stack and path state behind it) is the kernel's own.  The single-level kernels put the
// image at LDS byte 0 -- the dynamic LDS of a kernel without static LDS starts there, which the compiler knows: a node's address is then
// its number times the stride, without a base register.  The walks are NOT
// here: the hot loops are restated per kernel on purpose (fused_kernel.h).  Device code is held to "the same assembly as before"
// (scripts/device_asm_diff.py): k_fused_inst keeps its own copy of the staging loops because the helpers change its register allocation.
#pragma once
#include "pt_internal.h"
#include "pt_math.h"

namespace {

// A node in LDS is ten float4: lo_x hi_x lo_x | lo_y hi_y lo_y | lo_z hi_z lo_z | child words.  The near plane of an axis is float4 0 of its
// triple for a ray that goes up that axis and float4 1 for one that goes down; the far plane is ALWAYS the float4 behind the near one, so a node
// step forms one address per axis (node + 0 or 16 by the direction's sign) and reads the far plane at that address's immediate offset 16
// (extend_kernel.h PT_NODE_LOAD).  With the 128-B node's order (three lo planes, three hi planes) near and far lay 48 B apart in opposite
// directions: two addresses per axis, and a negation per axis to form them.
// The stride: lanes of a wave sit on DIFFERENT nodes but read the SAME field of them, so a stride that is a multiple of the 128-B bank cycle
// puts those 16-B reads on the same 4 banks.  160 B = 40 banks shifts consecutive nodes by 8 banks: the same field of different nodes falls on
// four groups of 4 banks, half of the 32 (the 144-B node this one replaces shifted by 4 and used all eight groups; 176 B would again, for 16 B
// more per node).  Not measured apart from the address arithmetic it saves; both together: +1.4 % on the Cornell box.
constexpr uint32_t LDS_NODE_F4 = 10;     // float4 per LDS node
constexpr uint32_t LDS_NODE_AXIS_F4 = 3; // ... per axis: lo hi lo
constexpr uint32_t LDS_NODE_CW_F4 = 9;   // ... where the child words are
// k_extend_inst walks its BLAS nodes in LDS and its TLAS nodes in memory with the same plane offsets: its LDS node is the 128-B node, spaced
// 144 B for the banks
constexpr uint32_t LDS_NODE128_F4 = 9;
// the compact codes of a child word (extend_kernel.h COMPACT): leaf = C14_LEAF | (count - 1) << 11 | first, inner = node index
constexpr uint32_t C14_LEAF = 0x2000u, C14_DONE = 0x3FFFu;
// the two-level fp16 kernels' codes (extend_inst16.h): leaf = I16_LEAF | (count - 1) << 11 | first (TLAS: | instance position)
constexpr uint32_t I16_EXIT = 0x7FFFu, I16_DONE = 0xFFFFu, I16_LEAF = 0x8000u;
constexpr uint32_t I16_NODE_DW = 20;  // dwords per fp16 node in LDS (16 used): 80-B stride spreads the banks

__host__ __device__ constexpr size_t lds_nodes_bytes(size_t n_wide) { return 16 * LDS_NODE_F4 * n_wide; }
__host__ __device__ constexpr size_t lds_nodes128_bytes(size_t n_wide) { return 16 * LDS_NODE128_F4 * n_wide; }
__host__ __device__ constexpr size_t lds_nodes16_bytes(size_t n_nodes) { return sizeof(uint32_t) * I16_NODE_DW * n_nodes; }
__host__ __device__ constexpr size_t lds_tris_bytes(size_t n_tris) { return sizeof(float4) * 9 * n_tris; }  // 3 permuted copies
// nodes | triangles, as the single-level kernels and k_extend_inst<.., LDS_BLAS> keep them; the fp16 form without the TLAS's share
__host__ __device__ constexpr size_t lds_scene_bytes(size_t n_wide, size_t n_tris) { return lds_nodes_bytes(n_wide) + lds_tris_bytes(n_tris); }
__host__ __device__ constexpr size_t lds_scene128_bytes(size_t n_wide, size_t n_tris) { return lds_nodes128_bytes(n_wide) + lds_tris_bytes(n_tris); }
// What decides whether a scene is of the LDS class (extend_launch.hip: <= 24 KB): nodes counted at 144 B, the stride the class was drawn and
// measured with.  The 160-B node did not move the line: the same scenes are in the class, their images up to 16 B per node (a ninth) bigger.
__host__ __device__ constexpr size_t lds_class_bytes(size_t n_wide, size_t n_tris) { return lds_nodes128_bytes(n_wide) + lds_tris_bytes(n_tris); }
__host__ __device__ constexpr size_t lds_scene16_bytes(size_t n_wide, size_t n_tris) { return lds_nodes16_bytes(n_wide) + lds_tris_bytes(n_tris); }

// 128-B nodes (three lo planes, three hi planes, child words, pad) -> 160-B LDS nodes.  COMPACT: the four child words re-coded to 14 bits
template <int BLOCK, bool COMPACT>
__device__ __forceinline__ void lds_stage_nodes(float4 *s_wide, const float4 *g_wide, uint32_t n_wide)
{
    for (uint32_t i = threadIdx.x; i < 8 * n_wide; i += BLOCK) {
        float4 v = g_wide[i];
        const uint32_t f = i & 7u;  // 0..2 lo x y z, 3..5 hi x y z, 6 child words, 7 unused
        float4 *nd = s_wide + (i >> 3) * LDS_NODE_F4;
        if (f < 3u) {
            nd[LDS_NODE_AXIS_F4 * f] = v;
            nd[LDS_NODE_AXIS_F4 * f + 2u] = v;
        } else if (f < 6u) {
            nd[LDS_NODE_AXIS_F4 * (f - 3u) + 1u] = v;
        } else if (f == 6u) {
            if (COMPACT) {
                auto cw = [](float c_) {
                    const uint32_t w = __float_as_uint(c_);
                    const uint32_t c = (w & PT_LEAF) ? (C14_LEAF | (((w >> 28) & 3u) << 11) | (w & 0x7FFu)) : (w & 0x1FFFu);
                    return __uint_as_float(w == SENTINEL ? C14_DONE : c);
                };
                v = make_float4(cw(v.x), cw(v.y), cw(v.z), cw(v.w));
            }
            nd[LDS_NODE_CW_F4] = v;
        }
    }
}
// ... -> 144-B LDS nodes in the 128-B node's own order (k_extend_inst)
template <int BLOCK>
__device__ __forceinline__ void lds_stage_nodes128(float4 *s_wide, const float4 *g_wide, uint32_t n_wide)
{
    for (uint32_t i = threadIdx.x; i < 8 * n_wide; i += BLOCK) s_wide[(i >> 3) * LDS_NODE128_F4 + (i & 7u)] = g_wide[i];
}

// a BVH4 child word -> the 16-bit code
__device__ __forceinline__ uint32_t lds_code16(uint32_t w)
{
    if (w == SENTINEL) return I16_DONE;
    return (w & PT_LEAF) ? (I16_LEAF | (((w >> 28) & 3u) << 11) | (w & 0x7FFu)) : (w & 0x7FFFu);
}
// (a function of its own: with this loop written out in lds_stage_nodes16, k_extend_inst16's staging code comes out with two moves swapped)
template <int BLOCK>
__device__ __forceinline__ void lds_stage_tlas16(uint32_t *s_blas, uint32_t n_blas_wide, const uint4 *__restrict__ tlas16, uint32_t n_tlas_lds)
{
    for (uint32_t i = threadIdx.x; i < 4 * n_tlas_lds; i += BLOCK)
        *reinterpret_cast<uint4 *>(s_blas + (size_t)(n_blas_wide + (i >> 2)) * I16_NODE_DW + 4 * (i & 3u)) = tlas16[i];
}
// 64-B fp16 nodes -> 80-B LDS nodes with 16-bit child codes; the first n_tlas_lds TLAS nodes -- its top levels: the builder numbers
// the nodes level by level -- sit behind the BLAS nodes, so a visit to one of them is the same LDS read as a BLAS node
template <int BLOCK>
__device__ __forceinline__ void lds_stage_nodes16(uint32_t *s_blas, const uint4 *__restrict__ g_blas16, uint32_t n_blas_wide, const uint4 *__restrict__ tlas16, uint32_t n_tlas_lds)
{
    lds_stage_tlas16<BLOCK>(s_blas, n_blas_wide, tlas16, n_tlas_lds);
    for (uint32_t i = threadIdx.x; i < 4 * n_blas_wide; i += BLOCK) {
        uint4 v = g_blas16[i];
        if ((i & 3u) == 3u) {  // the four child words -> 16-bit codes
            v = make_uint4(lds_code16(v.x), lds_code16(v.y), lds_code16(v.z), lds_code16(v.w));
        }
        *reinterpret_cast<uint4 *>(s_blas + (size_t)(i >> 2) * I16_NODE_DW + 4 * (i & 3u)) = v;
    }
}

// three copies of the triangles with components permuted to (kx,ky,kz) for kz = 0,1,2; EXTRA: a table of the same length copied in the same loop
template <int BLOCK, bool EXTRA = false>
__device__ __forceinline__ void lds_stage_tris(float4 *s_tri, const float4 *g_tri4, uint32_t n_tris, float4 *s_extra = nullptr, const float4 *g_extra = nullptr)
{
    for (uint32_t i = threadIdx.x; i < 3 * n_tris; i += BLOCK) {
        const float4 v = g_tri4[i];
        s_tri[i] = make_float4(v.y, v.z, v.x, v.w);               // kz = 0: (kx,ky,kz) = (1,2,0)
        s_tri[3 * n_tris + i] = make_float4(v.z, v.x, v.y, v.w);  // kz = 1: (2,0,1)
        s_tri[6 * n_tris + i] = v;                                // kz = 2: (0,1,2)
        if (EXTRA) s_extra[i] = g_extra[i];
    }
}

}  // namespace
