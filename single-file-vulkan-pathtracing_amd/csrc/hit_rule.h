// hit_rule.h -- ONE source of what a leaf step accepts: the range a walk hands its leaf test, the range check, and the closest-hit rules that
// follow it.  Plain C++ over float4 and 32-bit words (tests/range_host.cpp compiles it for the host and drives it over the ends of the range).
//
// The rule is include/pt_api.h's and the oracle's (orc_trace starts h.t = tmax and its tri_test rejects t >= tmax):
//   closest hit   tmin < t < tmax, strictly; least t, equal t -> lowest primitive id (two-level: lowest (instance id, primitive id))
//   any hit       tmin < t < bound, strictly, the ray's OWN bound; tmax plays no part; the first such hit ends the walk
// A walk keeps best_t = tmax (closest) or = bound (any hit) until its first hit, and the closest rules below take a hit AT best_t when nothing
// was hit yet (best_pos == PT_MISS, or the all-ones best_prim / best_iid): right for a closest-hit walk, whose leaf test has already required
// t < tmax, so that the tie can only be with a real hit -- and wrong for an any-hit walk whose leaf test still ended at tmax: a triangle at
// exactly t == bound occluded, and one beyond tmax did not, whatever the bound.  Hence leaf_upper: an any-hit walk's leaf test ends at best_t.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef PT_MISS
#define PT_MISS 0xFFFFFFFFu
#endif

namespace ptl {

__device__ __forceinline__ uint32_t word_of(float f) { return __builtin_bit_cast(uint32_t, f); }

// the upper end of the range (tmin, upper) a walk hands its leaf test.  any_hit: best_t -- the ray's bound until the first hit, and after it
// the walk is ending anyway -- at no register's cost; else tmax, so that a hit AT best_t reaches the tie rule
__device__ __forceinline__ float leaf_upper(bool any_hit, float best_t, float tmax) { return any_hit ? best_t : tmax; }

// inside the range?  Both ends strict; a NaN is outside.  (One `&`, no short-circuit: pair_leaf.h on its branches)
__device__ __forceinline__ bool in_range(float t, float tmin, float upper) { return bool((t > tmin) & (t < upper)); }

// (The walks over leaves of up to four keep their rule in place -- t < best_t || (t == best_t && prim < best_prim), best_prim all ones until the
// first hit: as a function of this header it changed the closest-hit kernels' code.  It takes a hit AT best_t in the same way.)

// Single-level rule: closest t; equal t -> lowest gl_PrimitiveID (the OBJ has coincident quads).  The ids of the two rivals are read when it
// happens (the third vertex of every record carries its triangle's id, k_pack), not kept.  -> true: the hit replaced the best one.
__device__ __forceinline__ bool closer_single_level(const float4 *tri4, uint32_t tri_base, float t, float V, float W, float det, uint32_t pos,
                                                    float &best_t, float &best_V, float &best_W, float &best_det, uint32_t &best_pos)
{
    bool closer = t < best_t;
    if (closer) {
        best_t = t; best_V = V; best_W = W; best_det = det; best_pos = pos;
    } else if (t == best_t) {  // (rare, and apart from the common path: merged into `closer` it cost every divide block seven scalar instructions)
        if (best_pos == PT_MISS || word_of(tri4[(size_t)tri_base + 3 * (size_t)pos + 2].w) <
                                       word_of(tri4[(size_t)tri_base + 3 * (size_t)best_pos + 2].w)) {
            best_t = t; best_V = V; best_W = W; best_det = det; best_pos = pos;
            closer = true;
        }
    }
    return closer;
}

// Two-level rule: closest t; equal t -> lowest (gl_InstanceID, gl_PrimitiveID).
__device__ __forceinline__ bool closer_instanced(float t, float V, float W, float det, uint32_t pos, uint32_t prim, uint32_t cur_ipos, uint32_t cur_iid,
                                                 float &best_t, float &best_V, float &best_W, float &best_det, uint32_t &best_pos, uint32_t &best_prim,
                                                 uint32_t &best_ipos, uint32_t &best_iid)
{
    if (t < best_t || (t == best_t && (cur_iid < best_iid || (cur_iid == best_iid && prim < best_prim)))) {
        best_t = t; best_V = V; best_W = W; best_det = det; best_pos = pos; best_prim = prim;
        best_ipos = cur_ipos; best_iid = cur_iid;
        return true;
    }
    return false;
}

}  // namespace ptl
