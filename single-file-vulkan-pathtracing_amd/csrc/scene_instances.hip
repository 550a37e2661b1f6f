// scene_instances.hip -- what pt_scene_set_instances does on the host with the caller's matrices, as kernels, for pt_scene_set_instances_device
// whose matrices are in device memory: the NaN/Inf check, the binary64 inverse and its check, the 96-byte records and
// the scene's kept copy of the set in one launch; and the world-space emitter copies of the NEE pipeline from that kept copy.  The per-thread
// statements are scene_instances_kernel.h's (tests/scene_instances_host.cpp runs the same ones on the host); scene_build.hip calls the
// launchers below where its host path runs its loops, and everything after them -- k_inst_boxes, the TLAS build, k_inst_sort, k_inst_frames --
// is the code both paths share.  What comes back to the host: one verdict word per set, one float (the emitters' total area) per emitter table.
#include "pt_internal.h"
#include "pt_math.h"
#include "scene_instances_kernel.h"

#include <string>

namespace {

// 1 + 2. one thread per instance: record, kept copy, verdict (a vector atomic; the minimum is the host loop's first error)
__global__ __launch_bounds__(TB) void k_si_check_invert(const float *__restrict__ xforms3x4, uint32_t n, float4 *__restrict__ rec, float4 *__restrict__ kept,
                                                        uint32_t *__restrict__ verdict)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = si_check_invert(xforms3x4, i, rec + 6 * (size_t)i, kept + 3 * (size_t)i);
    if (v != SI_OK) atomicMin(verdict, v);
}

// 3. one thread per (instance, emitter), instance-major: the record and, beside it, the term of the fold
__global__ __launch_bounds__(TB) void k_si_lights(const float4 *__restrict__ kept, const float4 *__restrict__ base, uint32_t n_lights, uint32_t copies,
                                                  float4 *__restrict__ lights, float *__restrict__ half)
{
    const uint32_t idx = blockIdx.x * TB + threadIdx.x;
    if (idx >= copies) return;
    const uint32_t i = idx / n_lights, k = idx - i * n_lights;
    float4 rec[5];
    half[idx] = si_light_record(kept + 3 * (size_t)i, base + 5 * (size_t)k, rec);
    for (int j = 0; j < 5; j++) lights[5 * (size_t)idx + j] = rec[j];
}

}  // namespace

pt_status ptsi_check_invert(pt_ctx *ctx, const float *d_xforms3x4, uint32_t n, float4 *d_rec, float4 *d_kept, uint32_t *d_verdict, uint32_t *verdict)
{
    hipStream_t st = ctx->stream;
    PT_HIP(ctx, hipMemsetAsync(d_verdict, 0xFF, sizeof(uint32_t), st));  // SI_OK
    k_si_check_invert<<<(n + TB - 1) / TB, TB, 0, st>>>(d_xforms3x4, n, d_rec, d_kept, d_verdict);
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipMemcpyAsync(verdict, d_verdict, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    return PT_OK;
}

// ptb_ensure_inst_lights for a set that lives in device memory (the caller has checked the counts and the 2^24 limit)
pt_status ptsi_inst_lights(pt_scene *s)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t copies = s->n_inst * s->n_lights;
    PT_TRY(ptb_scene_alloc(s, "the instanced emitter table", { pt_buf_of(s->d_lights_inst, sizeof(float4) * 5 * (size_t)copies) }));
    DevBuf<float> d_half;  // [copies] the terms of the fold, [1] its total
    float total = 0.f;
    hipError_t e = d_half.alloc((size_t)copies + 1);
    if (e == hipSuccess) {
        k_si_lights<<<(copies + TB - 1) / TB, TB, 0, st>>>(s->d_xforms, s->d_lights, s->n_lights, copies, s->d_lights_inst, d_half.p);
        ptsd_launch_fold(d_half.p, copies, s->d_lights_inst, d_half.p + copies, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, d_half.p + copies, sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {  // the table is present only when it is whole
        (void)hipGetLastError();
        pt_scratch_free({ pt_buf_of(s->d_lights_inst) }, nullptr, 0);
        ctx->err = std::string("the instanced emitter table: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? PT_ERR_OOM : PT_ERR_HIP;
    }
    s->n_lights_inst = copies;
    s->light_area_inst = total;
    return PT_OK;
}
