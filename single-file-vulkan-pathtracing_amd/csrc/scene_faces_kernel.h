// scene_faces_kernel.h -- the per-thread statements of scene_faces.hip's kernel (pt_scene_set_faces / pt_scene_set_faces_device: the material
// words of the per-triangle tables from new per-face materials), in a header of their own so that
// tests/scene_faces_host.cpp compiles the very same statements for the host and holds them against a restatement of k_pack's lines
// (scene_build.hip) without a GPU, under the host's sanitizers.  k_pack's statements are RESTATED here, not shared: k_pack keeps its device code.
// Wants declared before it: float4 / make_float4 and ptm::fdiv (pt_internal.h + pt_math.h on the device, tests/kernel_host.h on the host).
// Compile with -ffp-contract=off.
#pragma once
#include <stddef.h>
#include <stdint.h>

// k_pack's divisor: pi rounded to float (closesthit.rchit:60, brdf = Kd / pi by a true divide)
constexpr float SF_PI = 3.1415927410125732f;

// the six floats of one row of the faces: Kd.rgb, Ke.rgb
struct SfFace { float kd[3], ke[3]; };

__host__ __device__ __forceinline__ SfFace sf_load(const float *__restrict__ faces, uint32_t prim)
{
    const float *f = faces + 6 * (size_t)prim;
    return { { f[0], f[1], f[2] }, { f[3], f[4], f[5] } };
}

// The emitter predicate as k_pack states it for shade64's flag word.  The same truth table as sd_is_emitter (scene_device_kernel.h) and the
// host loop of pt_scene_create: -0.0 emits nothing, a NaN does.
__host__ __device__ __forceinline__ bool sf_emits(const SfFace &m)
{
    return !(m.ke[0] == 0.f && m.ke[1] == 0.f && m.ke[2] == 0.f);
}

// The material words of table position `pos`, and nothing else of it:
//   shade4[3 pos + 0].w = Kd.r / pi        (.xyz: the normal -- not read, not written)
//   shade4[3 pos + 1]   = {Kd.g / pi, Kd.b / pi, Ke.r, Ke.g}
//   shade4[3 pos + 2].x = Ke.b             (.yzw: k_pack's zeros -- not written)
//   shade64[4 pos + 3]  = {Kd / pi, emits ? 1 : 0}
//   ke4[pos]            = {Ke, 0}
// shade4 == nullptr: the 8-wide tree's tables, which have no shade4.
__host__ __device__ __forceinline__ void sf_store(const SfFace &m, uint32_t pos, float4 *__restrict__ shade4, float4 *__restrict__ shade64,
                                                  float4 *__restrict__ ke4)
{
    const float br = ptm::fdiv(m.kd[0], SF_PI), bg = ptm::fdiv(m.kd[1], SF_PI), bb = ptm::fdiv(m.kd[2], SF_PI);
    if (shade4) {
        shade4[3 * (size_t)pos + 0].w = br;  // one dword: no read-modify-write of the float4
        shade4[3 * (size_t)pos + 1] = make_float4(bg, bb, m.ke[0], m.ke[1]);
        shade4[3 * (size_t)pos + 2].x = m.ke[2];
    }
    shade64[4 * (size_t)pos + 3] = make_float4(br, bg, bb, sf_emits(m) ? 1.f : 0.f);
    ke4[pos] = make_float4(m.ke[0], m.ke[1], m.ke[2], 0.f);
}

// One thread of k_set_faces<HAS8>: position `pos` of the traversed tree's tables and, HAS8, the same position of the 8-wide tree's.  Every
// load -- the one or two prim_of words, then the six or twelve face words -- stands ahead of the first store.
template <bool HAS8>
__host__ __device__ __forceinline__ void sf_set_position(const float *__restrict__ faces, const uint32_t *__restrict__ prim_of,
                                                         const uint32_t *__restrict__ prim_of8, uint32_t pos, float4 *__restrict__ shade4,
                                                         float4 *__restrict__ shade64, float4 *__restrict__ ke4, float4 *__restrict__ shade64_8,
                                                         float4 *__restrict__ ke4_8)
{
    const uint32_t prim = prim_of[pos];
    uint32_t prim8 = 0;
    if constexpr (HAS8) prim8 = prim_of8[pos];
    const SfFace m = sf_load(faces, prim);
    SfFace m8 = {};
    if constexpr (HAS8) m8 = sf_load(faces, prim8);
    sf_store(m, pos, shade4, shade64, ke4);
    if constexpr (HAS8) sf_store(m8, pos, nullptr, shade64_8, ke4_8);
}
