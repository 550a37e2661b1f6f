// scene_device_kernel.h -- the per-thread statements of scene_device.hip's kernels (pt_scene_create_device / pt_scene_update_device: what
// pt_scene_create / pt_scene_update do on the host, as device code), in a header of their own so that tests/scene_device_host.cpp can compile
// the very same statements for the host and hold them against restatements of push_emitter and find_fan_pairs (scene_build.hip) without a GPU,
// under the host's sanitizers.  Wants declared before it: float4 / make_float4, ptm::fsqrt and ptm::fdiv (pt_internal.h + pt_math.h on the
// device, tests/kernel_host.h on the host).  Compile with -ffp-contract=off: the records' bits are the host loop's.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- 1. the index check: thread `tid` of `n_threads` looks at the words tid, tid + n_threads, ... of the 3 * n_tris indices (a wave's loads
// are consecutive dwords) and reports whether one of them names no vertex.  It reads d_indices only: no index is used as an address.
__device__ __forceinline__ bool sd_any_bad_index(const uint32_t *__restrict__ indices, size_t n_words, uint32_t n_verts, size_t tid, size_t n_threads)
{
    bool bad = false;
    for (size_t i = tid; i < n_words; i += n_threads) bad |= indices[i] >= n_verts;
    return bad;
}

// ---- 2. emitter discovery: the test of push_emitter's caller on row `prim` of the faces, as floats (-0.0 emits nothing, a NaN does)
__device__ __forceinline__ bool sd_is_emitter(const float *__restrict__ faces, uint32_t prim)
{
    const float *f = faces + 6 * (size_t)prim;
    return f[3] != 0.f || f[4] != 0.f || f[5] != 0.f;
}
// ... and the compaction behind the scan of the n + 1 flags (the last one 0): primitive t is an emitter where its place differs from its
// successor's, and its id goes to that place -- ascending primitive order
__device__ __forceinline__ void sd_compact(const uint32_t *__restrict__ place, uint32_t t, uint32_t *__restrict__ light_prim)
{
    if (place[t] != place[t + 1]) light_prim[place[t]] = t;
}

// ---- 3. one emitter record, push_emitter's five float4 with its operation order: {a, cdf} {b} {c} {-(cross / len)} {ke}.  The cdf word is the
// fold's (below) and is written as +0 here; -> 0.5f * len, the term the fold adds.  tri_orig: k_gather's de-indexed triangles (.w is not a coordinate).
__device__ __forceinline__ float sd_emitter_record(const float4 *__restrict__ tri_orig, const float *__restrict__ faces, uint32_t prim, float4 *__restrict__ rec5)
{
    const float4 a = tri_orig[3 * (size_t)prim + 0], b = tri_orig[3 * (size_t)prim + 1], c = tri_orig[3 * (size_t)prim + 2];
    const float *f = faces + 6 * (size_t)prim;
    const float e1[3] = { b.x - a.x, b.y - a.y, b.z - a.z }, e2[3] = { c.x - a.x, c.y - a.y, c.z - a.z };
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const float len = ptm::fsqrt((cx * cx + cy * cy) + cz * cz);
    rec5[0] = make_float4(a.x, a.y, a.z, 0.f);
    rec5[1] = make_float4(b.x, b.y, b.z, 0.f);
    rec5[2] = make_float4(c.x, c.y, c.z, 0.f);
    rec5[3] = make_float4(-ptm::fdiv(cx, len), -ptm::fdiv(cy, len), -ptm::fdiv(cz, len), 0.f);
    rec5[4] = make_float4(f[3], f[4], f[5], 0.f);
    return 0.5f * len;
}

// ---- the cdf: run = run + half[k] in ascending emitter order from +0, a left fold (the host loop's bits; no tree).  One pass takes the `cnt`
// (1..64) terms a wave holds one per lane: every lane adds them in lane order -- lane_value(k) is lane k's term, the same for every caller --
// and lane `lane` keeps the sum as it stood after its own term.  `run` leaves as the sum after all cnt terms.
constexpr uint32_t SD_FOLD = 64;
template <bool FULL, class LaneValue>  // FULL: cnt == SD_FOLD, every pass but the last: no count is tested
__device__ __forceinline__ float sd_fold_pass(float &run, uint32_t cnt, uint32_t lane, LaneValue lane_value)
{
    float mine = run;
#pragma unroll
    for (uint32_t k = 0; k < SD_FOLD; k++) {
        if (FULL || k < cnt) run = run + lane_value(k);
        if (k == lane) mine = run;
    }
    return mine;
}

// ---- 4. fan pairs (find_fan_pairs): triangle i + 1 starts at triangle i's first vertex and continues from its third, the 12 bytes compared
// AS BITS (memcmp: -0.0 is not +0.0, equal NaN payloads match).  The last triangle has no successor.
__device__ __forceinline__ bool sd_same_bits3(const float4 &p, const float4 &q)
{
    return __builtin_bit_cast(uint32_t, p.x) == __builtin_bit_cast(uint32_t, q.x) && __builtin_bit_cast(uint32_t, p.y) == __builtin_bit_cast(uint32_t, q.y) &&
           __builtin_bit_cast(uint32_t, p.z) == __builtin_bit_cast(uint32_t, q.z);
}
__device__ __forceinline__ uint8_t sd_fan_with_next(const float4 *__restrict__ tri_orig, uint32_t i, uint32_t n)
{
    if (i + 1 >= n) return 0;
    return sd_same_bits3(tri_orig[3 * (size_t)i + 0], tri_orig[3 * (size_t)i + 3]) && sd_same_bits3(tri_orig[3 * (size_t)i + 2], tri_orig[3 * (size_t)i + 4]) ? 1 : 0;
}
// ... and the greedy, non-overlapping pass over at most PT_SAH_MAX_TRIS flags, on the host behind the read-back: a triangle that is the second
// half of a pair starts none
inline void sd_greedy_pairs(const uint8_t *same, uint32_t n, uint8_t *pair)
{
    for (uint32_t i = 0; i < n; i++) pair[i] = 0;
    for (uint32_t i = 0; i + 1 < n; i++)
        if (same[i]) { pair[i] = 1; i++; }
}
