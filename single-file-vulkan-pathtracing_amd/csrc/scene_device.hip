// scene_device.hip -- what pt_scene_create / pt_scene_update do on the host with the caller's arrays, as kernels, for pt_scene_create_device /
// pt_scene_update_device whose arrays are in device memory: the index check, the discovery of the emitters, their records
// with the running cdf, the fan-pair flags of small scenes.  The per-thread statements are scene_device_kernel.h's (tests/scene_device_host.cpp
// runs the same ones on the host); scene_build.hip calls the launchers below where its host path runs push_emitter and find_fan_pairs, and
// everything after them -- k_gather, the builds and refits, k_pack -- is the code both paths share.
// What comes back to the host is bounded (include/pt_api.h): one word of the index check, the emitters' count, ids and records, and for scenes
// of at most PT_SAH_MAX_TRIS triangles the pair flags.  No vertex, index or face array does.
#include "pt_internal.h"
#include "pt_math.h"
#include "device_scan.h"
#include "scene_device_kernel.h"

#include <string>
#include <vector>

namespace {

constexpr uint32_t SD_CHECK_BLOCKS_MAX = 2048;  // (grid-stride beyond: 8 blocks per CU of the 256)

// 1. one word: was any index >= n_verts.  A wave votes; one lane of a wave that saw one sets the word (a vector atomic).
__global__ __launch_bounds__(TB) void k_sd_check_indices(const uint32_t *__restrict__ indices, size_t n_words, uint32_t n_verts, uint32_t *__restrict__ bad)
{
    const bool mine = sd_any_bad_index(indices, n_words, n_verts, (size_t)blockIdx.x * TB + threadIdx.x, (size_t)gridDim.x * TB);
    if (__any(mine) && (threadIdx.x & 63u) == 0u) atomicOr(bad, 1u);
}

// 2. emitter flags of the n primitives and a closing 0 (device_scan.h turns them into places), then the order-preserving compaction
__global__ __launch_bounds__(TB) void k_sd_emitter_flags(const float *__restrict__ faces, uint32_t n, uint32_t *__restrict__ place)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t <= n) place[t] = t < n && sd_is_emitter(faces, t) ? 1u : 0u;
}
__global__ __launch_bounds__(TB) void k_sd_emitter_compact(const uint32_t *__restrict__ place, uint32_t n, uint32_t *__restrict__ light_prim)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    if (t < n) sd_compact(place, t, light_prim);
}

// 3. the records in parallel, the half-areas beside them ...
__global__ __launch_bounds__(TB) void k_sd_emitter_records(const float4 *__restrict__ tri_orig, const float *__restrict__ faces, const uint32_t *__restrict__ light_prim,
                                                           uint32_t n_lights, float4 *__restrict__ lights, float *__restrict__ half)
{
    const uint32_t k = blockIdx.x * TB + threadIdx.x;
    if (k >= n_lights) return;
    float4 rec[5];
    half[k] = sd_emitter_record(tri_orig, faces, light_prim[k], rec);
    for (int j = 0; j < 5; j++) lights[5 * (size_t)k + j] = rec[j];
}
// ... then the fold, in order: ONE wave; a pass is one coalesced load of 64 half-areas (the next pass's is in flight meanwhile) and 64 dependent
// adds from registers, every lane keeping the sum as it stood after its own term.  total: the last run (light_area).
__global__ __launch_bounds__(SD_FOLD) void k_sd_emitter_fold(const float *__restrict__ half, uint32_t n_lights, float4 *__restrict__ lights, float *__restrict__ total)
{
    const uint32_t lane = threadIdx.x;
    float run = 0.f;
    float next = lane < n_lights ? half[lane] : 0.f;
    for (uint32_t base = 0; base < n_lights; base += SD_FOLD) {
        const float h = next;
        const uint32_t ahead = base + SD_FOLD + lane;
        next = ahead < n_lights ? half[ahead] : 0.f;
        const uint32_t cnt = n_lights - base < SD_FOLD ? n_lights - base : SD_FOLD;
        const auto term = [&](uint32_t k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(h), (int)k)); };  // (k: a constant of the unrolled pass)
        const float mine = cnt == SD_FOLD ? sd_fold_pass<true>(run, cnt, lane, term) : sd_fold_pass<false>(run, cnt, lane, term);
        if (lane < cnt) lights[5 * (size_t)(base + lane)].w = mine;
    }
    if (lane == 0) *total = run;
}

// 4. the fan-pair flags of a small scene, from the gathered triangles
__global__ __launch_bounds__(TB) void k_sd_fan_flags(const float4 *__restrict__ tri_orig, uint32_t n, uint8_t *__restrict__ same)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i < n) same[i] = sd_fan_with_next(tri_orig, i, n);
}

}  // namespace

void ptsd_launch_fold(const float *d_half, uint32_t n, float4 *d_lights, float *d_total, hipStream_t st)
{
    k_sd_emitter_fold<<<1, SD_FOLD, 0, st>>>(d_half, n, d_lights, d_total);
}

pt_status ptsd_check_indices(pt_ctx *ctx, const uint32_t *d_indices, uint32_t n_tris, uint32_t n_verts)
{
    hipStream_t st = ctx->stream;
    const size_t n_words = 3 * (size_t)n_tris;
    DevBuf<uint32_t> d_bad;
    PT_HIP(ctx, d_bad.alloc(1));
    PT_HIP(ctx, hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), st));
    const uint32_t blocks = (uint32_t)std::min<size_t>((n_words + TB - 1) / TB, SD_CHECK_BLOCKS_MAX);
    k_sd_check_indices<<<blocks, TB, 0, st>>>(d_indices, n_words, n_verts, d_bad.p);
    PT_HIP(ctx, hipGetLastError());
    uint32_t bad = 0;
    PT_HIP(ctx, hipMemcpyAsync(&bad, d_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    return bad ? pt_bad(ctx, "vertex index out of range") : PT_OK;
}

pt_status ptsd_find_emitters(pt_scene *s) { return ptsd_find_emitters(s, s->d_faces, pt_scene_emitters(s)); }

pt_status ptsd_find_emitters(pt_scene *s, const float *d_faces, pt_emitters e)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t n = s->n_tris, g = (n + 1 + TB - 1) / TB;
    DevBuf<uint32_t> d_place, d_sums;
    PT_HIP(ctx, d_place.alloc((size_t)n + 1));
    PT_HIP(ctx, d_sums.alloc(((size_t)n + 1 + SC_TILE - 1) / SC_TILE));
    k_sd_emitter_flags<<<g, TB, 0, st>>>(d_faces, n, d_place.p);
    exclusive_scan(d_place.p, n + 1, d_sums.p, st);
    uint32_t count = 0;
    PT_HIP(ctx, hipMemcpyAsync(&count, d_place.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    e.n_lights = count;
    e.h_light_prim.assign(count, 0u);
    if (!count) return PT_OK;
    PT_TRY(ptb_scene_alloc(s, "the emitter table", { pt_buf_of(e.d_lights, sizeof(float4) * 5 * (size_t)count), pt_buf_of(e.d_light_prim, sizeof(uint32_t) * count) }));
    k_sd_emitter_compact<<<g, TB, 0, st>>>(d_place.p, n, e.d_light_prim);
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipMemcpyAsync(e.h_light_prim.data(), e.d_light_prim, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, st));
    PT_HIP(ctx, hipStreamSynchronize(st));
    return PT_OK;
}

// One scratch allocation, one wait: the records and their fold, the pair flags of a small scene (pair != nullptr), then everything the host keeps.
pt_status ptsd_host_products(pt_scene *s, std::vector<uint8_t> *pair) { return ptsd_host_products(s, s->d_faces, pt_scene_emitters(s), pair); }

pt_status ptsd_host_products(pt_scene *s, const float *d_faces, pt_emitters e, std::vector<uint8_t> *pair)
{
    pt_ctx *ctx = s->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t n = e.n_lights, nt = s->n_tris;
    e.h_lights.assign(5 * (size_t)n, make_float4(0.f, 0.f, 0.f, 0.f));
    e.light_area = 0.f;
    if (!n && !pair) return PT_OK;
    if (n && !e.d_light_prim) {  // a scene made from host arrays: the emitters' ids go to the device once and stay
        PT_HIP(ctx, hipMalloc((void **)&e.d_light_prim, sizeof(uint32_t) * n));
        PT_HIP(ctx, hipMemcpyAsync(e.d_light_prim, e.h_light_prim.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
    }
    DevBuf<float> d_scratch;  // [n] the terms of the fold, [1] its total, then nt bytes of pair flags
    PT_HIP(ctx, d_scratch.alloc((size_t)n + 1 + (pair ? (nt + 3) / 4 : 0)));
    uint8_t *d_same = reinterpret_cast<uint8_t *>(d_scratch.p + n + 1);
    std::vector<uint8_t> same(pair ? nt : 0);
    if (n) {
        k_sd_emitter_records<<<(n + TB - 1) / TB, TB, 0, st>>>(s->d_tri_orig, d_faces, e.d_light_prim, n, e.d_lights, d_scratch.p);
        k_sd_emitter_fold<<<1, SD_FOLD, 0, st>>>(d_scratch.p, n, e.d_lights, d_scratch.p + n);
        PT_HIP(ctx, hipMemcpyAsync(e.h_lights.data(), e.d_lights, sizeof(float4) * 5 * (size_t)n, hipMemcpyDeviceToHost, st));
        PT_HIP(ctx, hipMemcpyAsync(&e.light_area, d_scratch.p + n, sizeof(float), hipMemcpyDeviceToHost, st));
    }
    if (pair) {
        k_sd_fan_flags<<<(nt + TB - 1) / TB, TB, 0, st>>>(s->d_tri_orig, nt, d_same);
        PT_HIP(ctx, hipMemcpyAsync(same.data(), d_same, nt, hipMemcpyDeviceToHost, st));
    }
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipStreamSynchronize(st));
    if (pair) {
        pair->resize(nt);
        sd_greedy_pairs(same.data(), nt, pair->data());
    }
    return PT_OK;
}
