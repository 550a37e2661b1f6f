// pair_leaf.h -- ONE source of the fan-pair leaf step of the scenes that live in LDS: the watertight test (Woop, Benthin, Wald, JCGT 2013)
// of a leaf that is one triangle (v0, v1, v2) or a fan pair (v0, v1, v2) + (v0, v2, v3), with the sheared vertices and the products of the
// shared edge v0-v2 computed once, the true divide, the range check tmin < t < tmax (the caller's upper end: ptl::leaf_upper) -- the range check
// itself and the two closest-hit rules that go with it are hit_rule.h, which also compiles for the host.
// Stands in for what the driver does behind traceRayEXT (raygen.rgen:63-75) for opaque, un-culled triangles (main.cpp:508, 525, 536).
//
// Four kernels instantiate it: k_extend (PAIRS: k_extend_lds7p) and k_fused for single-level scenes, k_extend_inst16 and k_fused_inst for
// two-level ones.  Until round 5 each of them carried its own copy of these lines, kept equal by the parity tests only.
#pragma once
#include "pt_math.h"
#include "hit_rule.h"

namespace ptl {

// tri4: the permuted triangle records in LDS -- {v0, id} {v1} {v2} per triangle, a pair's second triangle behind the first, so the pair's
// fourth vertex is record 5 (.w = the second triangle's gl_PrimitiveID); ti: index of the first record; first: the leaf's first position.
// accept(t, V, W, det, pos, prim_bits): a hit inside the range, in primitive order (first half first); hit_block(): once per divide block.
// LOAD_D_FIRST: how far past a single triangle's record (three float4) the step reads: records ti + 3 .. ti + 5
constexpr unsigned D_FIRST_OVERREAD_F4 = 3;
template <bool LOAD_D_FIRST = false, bool PIN_BY_USE = false, class Accept, class HitBlock>
__device__ __forceinline__ void pair_leaf_test(const float4 *tri4, size_t ti, bool two, uint32_t first, const ptm::RayPre &pre,
                                               const ptm::f3 &orgp, float tmin, float tmax, Accept &&accept, HitBlock &&hit_block)
{
    const float4 a = tri4[ti + 0], b = tri4[ti + 1], c = tri4[ti + 2];
    // LOAD_D_FIRST: the pair's fourth vertex is read WITH the first three instead of behind `two` -- one LDS round trip per leaf step instead of
    // two (k_fused: -0.5 %, profiles/r06y_leaf_fourth_vertex_first.log).  A single triangle's step then reads 16 bytes of the record behind it:
    // only for callers whose triangle records are followed by more of their own LDS (the fused kernel: its shade table).
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (LOAD_D_FIRST) {
        d = tri4[ti + 5];
        // (keeps the load here: the compiler sinks it back behind the branch)
        // PIN_BY_USE: the pin is a USE of the loaded registers, not a tie ("+v").  A tied operand is a new value per component, and the compiler
        // copies three of the four out of the load's register tuple to make them: three v_mov_b32 per leaf step (k_fused; k_fused_inst keeps
        // the tie until its own listing is read)
        if (PIN_BY_USE) asm volatile("" :: "v"(d.x), "v"(d.y), "v"(d.z), "v"(d.w));
        else asm volatile("" : "+v"(d.x), "+v"(d.y), "+v"(d.z), "+v"(d.w));
    }
    // the sheared vertices and the products of the edge v0-v2 serve both halves (ptm::tri_test_perm, same operands in the same order:
    // bit-identical numerators)
    const float Az_ = a.z - orgp.z, Bz_ = b.z - orgp.z, Cz_ = c.z - orgp.z;
    const float Ax = (a.x - orgp.x) - pre.Sx * Az_, Ay = (a.y - orgp.y) - pre.Sy * Az_;
    const float Bx = (b.x - orgp.x) - pre.Sx * Bz_, By = (b.y - orgp.y) - pre.Sy * Bz_;
    const float Cx = (c.x - orgp.x) - pre.Sx * Cz_, Cy = (c.y - orgp.y) - pre.Sy * Cz_;
    const float pAC = Ax * Cy, qAC = Ay * Cx;
    // edge test of one half: inside (no strictly negative AND strictly positive edge function) and not edge-on
    // (no short-circuit evaluation: each `&&` was a branch -- exec-mask bookkeeping on the scalar unit for instructions the wave runs anyway)
    auto inside = [](float U, float V, float W) {
        const bool neg = fminf(fminf(U, V), W) < 0.0f, pos = fmaxf(fmaxf(U, V), W) > 0.0f, nz = ((U + V) + W) != 0.0f;
        return bool(!(neg & pos) & nz);
    };
    auto finish = [&](float U, float V, float W, float z0, float z1, float z2, uint32_t pos, uint32_t prim) {
        const float det = (U + V) + W;
        hit_block();
        const float T = (U * (pre.Sz * z0) + V * (pre.Sz * z1)) + W * (pre.Sz * z2);
        const float t = ptm::fdiv(T, det);
        // outside the range: a NaN goes on, which is neither closer than nor equal to anything (one select instead of two branches)
        accept(in_range(t, tmin, tmax) ? t : __builtin_nanf(""), V, W, det, pos, prim);
    };
    const float UA = Cx * By - Cy * Bx, VA = pAC - qAC, WA = Bx * Ay - By * Ax;
    const bool inA = inside(UA, VA, WA);
    float UB = 0.f, VB = 0.f, WB = 0.f, Dz_ = 0.f;
    uint32_t primB = 0u;
    bool inB = false;
    if (LOAD_D_FIRST || two) {  // (LOAD_D_FIRST: the second half is computed for every lane -- nearly every wave holds a pair, so the branch only cost its bookkeeping)
        if (!LOAD_D_FIRST) d = tri4[ti + 5];  // third vertex of the second half; .w = its primitive id (k_pack)
        Dz_ = d.z - orgp.z;
        const float Dx = (d.x - orgp.x) - pre.Sx * Dz_, Dy = (d.y - orgp.y) - pre.Sy * Dz_;
        // (v0, v2, v3): U = Dx*Cy - Dy*Cx, V = Ax*Dy - Ay*Dx, W = Cx*Ay - Cy*Ax = qAC - pAC
        UB = Dx * Cy - Dy * Cx; VB = Ax * Dy - Ay * Dx; WB = qAC - pAC;
        primB = __float_as_uint(d.w);
        inB = bool(two & inside(UB, VB, WB));
    }
    // A wave nearly always holds lanes inside the first half AND lanes inside the second, so two separate divide blocks both ran in 95 %
    // of the steps, each for a handful of lanes.  One block serves both: a lane inside the second half only brings that half's operands;
    // the lane inside BOTH (a ray through the shared diagonal, a folded quad) takes the first half here and the second in a block of its
    // own, in primitive order.  Same operations on the same operands: same bits.
    if (inA || inB) {
        const bool sb = !inA;
        finish(sb ? UB : UA, sb ? VB : VA, sb ? WB : WA, Az_, sb ? Cz_ : Bz_, sb ? Dz_ : Cz_, sb ? first + 1u : first, sb ? primB : __float_as_uint(a.w));
    }
    if (inA && inB) finish(UB, VB, WB, Az_, Cz_, Dz_, first + 1u, primB);
}

// (the two closest-hit rules that go with it, closer_single_level and closer_instanced: hit_rule.h)

}  // namespace ptl
