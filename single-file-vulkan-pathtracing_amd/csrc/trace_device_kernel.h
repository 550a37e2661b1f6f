// trace_device_kernel.h -- the per-lane bodies of k_trace_pack / k_trace_occluded / k_trace_surface (trace_device.hip), in a header of their own,
// like upsample_kernel.h and present_planes_kernel.h, so that tests/trace_device_host.cpp can compile the very same statements for the host, run
// them over every ray of a chunk and hold the result against numpy and the oracle without a GPU, under the host's sanitizers.  Wants declared
// before it: float2, float4, make_float2, make_float4, ptm::fdiv, ptm::fsqrt, and TD_LOADS_DONE() (the device: one wait for every load issued so
// far; the host: nothing).  Compile with -ffp-contract=off: every operation of the surface record is rounded on its own.
//
// The queue layout is the extend kernels' (wavefront_types.h QueueView): rayA[i] = {origin.xyz, direction.x}, rayB[i] = {direction.y, direction.z},
// hit[i] = {bits(leaf position | TD_MISS), t, u, v}, hit_inst[i] = the instance's position in TLAS leaf order (two-level scenes, closest hits only).
#pragma once
#ifndef TD_LD4
#define TD_LD4(p) (*(p))   // the load of a whole hit record (the device: one streaming 16-B load, so that u and v arrive with the position word)
#endif

constexpr uint32_t TD_MISS = 0xFFFFFFFFu;  // pt_math.h PT_MISS: the position word of a ray that hit nothing

// ---- k_trace_pack: ray i of a chunk, caller's layout -> queue layout ------------------------------------------------------------------------
// rays6: the chunk's first row; rows are 24 B apart and only 4-byte aligned, so a lane reads six dwords -- a wave's 64 rows are 1536 contiguous
// bytes, every 128-B line of which is consumed whole by the wave's six loads.  All six (seven with a bound plane) are issued before the first
// store.  bound (nullable): the any-hit kernels' per-ray upper bound, ray_tmax[i] = d_tmax ? d_tmax[i] : tmax.
__device__ __forceinline__ void td_pack(const float *__restrict__ rays6, const float *__restrict__ d_tmax, float tmax, uint32_t i,
                                        float4 *__restrict__ rayA, float2 *__restrict__ rayB, float *__restrict__ bound)
{
    const float *r = rays6 + 6 * (size_t)i;
    const float r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5];
    float b = tmax;
    if (bound && d_tmax) b = d_tmax[i];
    TD_LOADS_DONE();
    rayA[i] = make_float4(r0, r1, r2, r3);
    rayB[i] = make_float2(r4, r5);
    if (bound) bound[i] = b;
}

// ---- k_trace_occluded: one byte per ray from the position word of its hit record ------------------------------------------------------------
__device__ __forceinline__ uint8_t td_occluded(const float4 *__restrict__ hit, uint32_t i)
{
    return __builtin_bit_cast(uint32_t, hit[i].x) != TD_MISS ? 1 : 0;
}

// ---- k_trace_surface: what closesthit.rchit:50-65 computes at the hit -----------------------------------------------------------------------
struct TdScene {
    const float4 *tri4;        // 3 x float4 per leaf position of the tree that was walked {A, bits(prim)} {B, 0} {C, 0}
    const float4 *rec64;       // 4 x float4 per leaf position of the same tree: .w of the first three is the shading normal
    const float *faces;        // 6 floats per primitive {Kd, Ke}
    const float4 *inst6;       // two-level: 6 x float4 per TLAS leaf position {object->world rows} {world->object rows}
    const float4 *inst_frame;  // two-level, FRAMES: 2 x float4 per (TLAS leaf position, leaf position), the first {world normal, .}
    uint32_t n_tris;
};
struct TdPlanes {
    float *position, *normal, *albedo, *emission;  // n x 3 floats each, any may be null
};
// INST: a two-level scene; FRAMES: its normals come from the (instance, triangle) table, else by the inverse transpose, renormalised.
// A lane that missed gathers the records of leaf position 0 (and TLAS position 0) -- always there -- and selects +0.0 at the end: one straight
// run of gathers for every lane, no branch between them, all of them issued before the first store.
template <bool INST, bool FRAMES>
__device__ __forceinline__ void td_surface(const TdScene &sc, const float4 *__restrict__ hit, const uint32_t *__restrict__ hit_inst,
                                           const TdPlanes &pl, uint32_t i)
{
    const float4 h = TD_LD4(hit + i);
    const uint32_t word = __builtin_bit_cast(uint32_t, h.x);
    const bool is_hit = word != TD_MISS;
    const uint32_t pos = is_hit ? word : 0u;
    uint32_t ip = 0u;
    if (INST) { ip = hit_inst[i]; ip = is_hit ? ip : 0u; }
    const float4 ta = sc.tri4[3 * (size_t)pos + 0], tb = sc.tri4[3 * (size_t)pos + 1], tc = sc.tri4[3 * (size_t)pos + 2];
    float nx = sc.rec64[4 * (size_t)pos + 0].w, ny = sc.rec64[4 * (size_t)pos + 1].w, nz = sc.rec64[4 * (size_t)pos + 2].w;
    const uint32_t prim = __builtin_bit_cast(uint32_t, ta.w);
    const float *f = sc.faces + 6 * (size_t)prim;
    const float f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3], f4 = f[4], f5 = f[5];
    float4 m0 = {}, m1 = {}, m2 = {}, i0 = {}, i1 = {}, i2 = {}, fr = {};
    if (INST) {
        m0 = sc.inst6[6 * (size_t)ip + 0]; m1 = sc.inst6[6 * (size_t)ip + 1]; m2 = sc.inst6[6 * (size_t)ip + 2];
        if (FRAMES) {
            fr = sc.inst_frame[2 * ((size_t)ip * sc.n_tris + pos)];
        } else {
            i0 = sc.inst6[6 * (size_t)ip + 3]; i1 = sc.inst6[6 * (size_t)ip + 4]; i2 = sc.inst6[6 * (size_t)ip + 5];
        }
    }
    TD_LOADS_DONE();
    // closesthit.rchit:52-56
    const float u = h.z, v = h.w;
    const float b0 = (1.0f - u) - v;
    float px = (ta.x * b0 + tb.x * u) + tc.x * v;
    float py = (ta.y * b0 + tb.y * u) + tc.y * v;
    float pz = (ta.z * b0 + tb.z * u) + tc.z * v;
    if (INST) {
        const float wx = ((m0.x * px + m0.y * py) + m0.z * pz) + m0.w;
        const float wy = ((m1.x * px + m1.y * py) + m1.z * pz) + m1.w;
        const float wz = ((m2.x * px + m2.y * py) + m2.z * pz) + m2.w;
        px = wx; py = wy; pz = wz;
        if (FRAMES) {
            nx = fr.x; ny = fr.y; nz = fr.z;
        } else {  // k_aov_reduce<INST>'s statements
            const float ax = (i0.x * nx + i1.x * ny) + i2.x * nz;
            const float ay = (i0.y * nx + i1.y * ny) + i2.y * nz;
            const float az = (i0.z * nx + i1.z * ny) + i2.z * nz;
            const float l = ptm::fsqrt((ax * ax + ay * ay) + az * az);
            nx = ptm::fdiv(ax, l); ny = ptm::fdiv(ay, l); nz = ptm::fdiv(az, l);
        }
    }
    if (pl.position) {
        float *o = pl.position + 3 * (size_t)i;
        o[0] = is_hit ? px : 0.0f; o[1] = is_hit ? py : 0.0f; o[2] = is_hit ? pz : 0.0f;
    }
    if (pl.normal) {
        float *o = pl.normal + 3 * (size_t)i;
        o[0] = is_hit ? nx : 0.0f; o[1] = is_hit ? ny : 0.0f; o[2] = is_hit ? nz : 0.0f;
    }
    if (pl.albedo) {
        float *o = pl.albedo + 3 * (size_t)i;
        o[0] = is_hit ? f0 : 0.0f; o[1] = is_hit ? f1 : 0.0f; o[2] = is_hit ? f2 : 0.0f;
    }
    if (pl.emission) {
        float *o = pl.emission + 3 * (size_t)i;
        o[0] = is_hit ? f3 : 0.0f; o[1] = is_hit ? f4 : 0.0f; o[2] = is_hit ? f5 : 0.0f;
    }
}
