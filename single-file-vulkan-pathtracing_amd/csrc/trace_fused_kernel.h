// trace_fused_kernel.h -- the per-lane statements of k_trace_fused (trace_fused.hip) that touch the caller's arrays, in a header of their own like
// trace_device_kernel.h, so that tests/trace_fused_host.cpp can compile the very same statements for the host and hold them against numpy and the
// oracle without a GPU, under the host's sanitizers: row of d_rays6 -> ray, the any-hit bound, the walk's finish record -> the queue form's hit
// record -> pt_hit row / surface planes / occluded byte.  The walk itself is the kernel's.  Wants declared before it what trace_device_kernel.h
// wants.  Compile with -ffp-contract=off.
#pragma once
#include "trace_device_kernel.h"  // TdScene, TdPlanes, TD_MISS, td_surface: the surface record's statements are the queue form's, not a copy

// ---- refill: row i of the launch's rays, caller's layout.  Rows are 24 B apart and only 4-byte aligned: six dword loads per lane; the idle lanes
// of a wave take consecutive rows, so the wave's loads consume contiguous bytes.
struct TfRay { float ox, oy, oz, dx, dy, dz; };
__device__ __forceinline__ TfRay tf_row(const float *__restrict__ rays6, uint32_t i)
{
    const float *r = rays6 + 6 * (size_t)i;
    return { r[0], r[1], r[2], r[3], r[4], r[5] };
}
// ... and the bound its any-hit walk starts from: what k_trace_pack writes to the bound plane, ray_tmax[i] = d_tmax ? d_tmax[i] : tmax
__device__ __forceinline__ float tf_bound(const float *__restrict__ d_tmax, float tmax, uint32_t i) { return d_tmax ? d_tmax[i] : tmax; }

// ---- finish: what the walk holds for a ray that ran out of subtrees -> the hit record the extend kernels would have stored (extend_kernel.h, the
// non-raw branch: u = V / det, v = W / det by the true divide, zeros behind a miss)
struct TfBest { uint32_t pos; float t, V, W, det; };  // pos: leaf position of the winning triangle | TD_MISS
__device__ __forceinline__ float4 tf_record(const TfBest &b)
{
    const bool miss = b.pos == TD_MISS;
    return make_float4(__builtin_bit_cast(float, b.pos), miss ? 0.f : b.t, miss ? 0.f : ptm::fdiv(b.V, b.det), miss ? 0.f : ptm::fdiv(b.W, b.det));
}
// record -> row i of d_hits (pt_hit {prim, t, u, v, inst}: five dwords, rows 20 B apart), k_hits_to_api's statements for a single-level scene.
// tri4: 3 x float4 per leaf position, .w of the first the primitive id (the device: the unpermuted copy in LDS)
__device__ __forceinline__ void tf_hit_row(uint32_t *__restrict__ hits5, uint32_t i, const float4 &rec, const float4 *tri4)
{
    const uint32_t pos = __builtin_bit_cast(uint32_t, rec.x);
    uint32_t *o = hits5 + 5 * (size_t)i;
    o[0] = pos == TD_MISS ? TD_MISS : __builtin_bit_cast(uint32_t, tri4[3 * (size_t)pos].w);
    o[1] = __builtin_bit_cast(uint32_t, rec.y);
    o[2] = __builtin_bit_cast(uint32_t, rec.z);
    o[3] = __builtin_bit_cast(uint32_t, rec.w);
    o[4] = pos == TD_MISS ? TD_MISS : 0u;
}
// record -> row i of the surface planes: td_surface<false, false> run over a queue of one record, the planes moved to the row.  A plane that is
// null stays null (the pointers are wave-uniform: the scalar unit's tests)
__device__ __forceinline__ void tf_surface(const TdScene &sc, const float4 &rec, const TdPlanes &pl, uint32_t i)
{
    const auto row = [&](float *p) { return p ? p + 3 * (size_t)i : nullptr; };
    const TdPlanes at = { row(pl.position), row(pl.normal), row(pl.albedo), row(pl.emission) };
    td_surface<false, false>(sc, &rec, nullptr, at, 0u);
}
// any-hit: k_trace_occluded's byte
__device__ __forceinline__ uint8_t tf_occluded(uint32_t pos) { return pos != TD_MISS ? 1 : 0; }
