// scene_faces.hip -- pt_scene_set_faces / pt_scene_set_faces_device: the one kernel that rewrites the material words of
// the per-triangle tables from new per-face materials, in the leaf order the tables were last packed in, and nothing else of them.  The
// per-thread statements are scene_faces_kernel.h's (tests/scene_faces_host.cpp runs the same ones on the host).  The host side of the call --
// the staged copy of the faces, the staged emitter set (scene_device.hip's kernels), the swap -- is scene_build.hip's ptb_set_faces.
#include "pt_internal.h"
#include "pt_math.h"
#include "scene_faces_kernel.h"

namespace {

// One thread per table position; HAS8: the 8-wide tree's tables (d_prim_of8 order) by the same thread.  No LDS, no scratch.
template <bool HAS8>
__global__ __launch_bounds__(TB) void k_set_faces(const float *__restrict__ faces, const uint32_t *__restrict__ prim_of,
                                                  const uint32_t *__restrict__ prim_of8, uint32_t n, float4 *__restrict__ shade4,
                                                  float4 *__restrict__ shade64, float4 *__restrict__ ke4, float4 *__restrict__ shade64_8,
                                                  float4 *__restrict__ ke4_8)
{
    const uint32_t pos = blockIdx.x * TB + threadIdx.x;
    if (pos >= n) return;
    sf_set_position<HAS8>(faces, prim_of, prim_of8, pos, shade4, shade64, ke4, shade64_8, ke4_8);
}

}  // namespace

// d_faces: the new materials, f32 [6 * n_tris] in primitive order; order: the leaf order d_shade4 / d_shade64 / d_ke4 were last packed in.
// Queued on st; the caller checks hipGetLastError and waits.
void ptsf_launch_set_faces(pt_scene *s, const float *d_faces, const uint32_t *order, hipStream_t st)
{
    const uint32_t n = s->n_tris, g = (n + TB - 1) / TB;
    if (s->d_prim_of8 && s->d_shade64_8 && s->d_ke4_8)
        k_set_faces<true><<<g, TB, 0, st>>>(d_faces, order, s->d_prim_of8, n, s->d_shade4, s->d_shade64, s->d_ke4, s->d_shade64_8, s->d_ke4_8);
    else
        k_set_faces<false><<<g, TB, 0, st>>>(d_faces, order, nullptr, n, s->d_shade4, s->d_shade64, s->d_ke4, nullptr, nullptr);
}
