// bvh_refit.hip -- pt_scene_update's REFIT mode: the wide trees of a scene refitted bottom-up in place after its vertices moved.
// Topology (child words, leaf order, node layout, pair leaves) stays; every box is recomputed from the new triangle boxes with the
// rules the builders use: a leaf slot holds the union of its triangles' boxes padded by leaf_pad (lbvh_build.hip k_refit), an
// internal slot the union of its child's slots.  One kernel template serves the three node formats the scene holds:
//   W4F  128-B BVH4, float planes (d_wide_lbvh, d_wide_sah, the PLOC collapse; the TLAS reads its root box)   pt_scene_read_bvh4
//   W4H  64-B BVH4, fp16 planes normalised to the scene box, rounded outwards (d_wide16t; lbvh_build.hip k_w4_emit)
//   W8B  64-B 8-wide nodes, byte planes on the node's own grid (d_wide8; lbvh_build.hip k_w8_emit)             pt_scene_read_bvh8
// Schedule: per-node arrival counters.  A thread starts at every node without internal children, writes it, publishes its union
// and arrives at its parent (agent-scope release, then the vmcnt wait, then the ticket atomic: the k_refit hand-off); the last
// child to arrive carries on with the parent.  Nobody waits on anybody, so nothing assumes the blocks are co-resident, and a
// thread climbs at most n_nodes times.
#include "bvh_build.h"

#include <hip/hip_fp16.h>

namespace {

enum : int { W4F = 0, W4H = 1, W8B = 2 };

constexpr float NORM_EPS = 3.814697265625e-06f;  // the allowance of k_wide_half / k_w4_emit / k_w8_emit for the normalisation's rounding

// the up-to-8 children of a node: kind 0 empty, 1 leaf (first position, count), 2 internal (node index)
template <int F>
__device__ __forceinline__ int node_children(const uint4 *nodes, uint32_t i, uint32_t kind[8], uint32_t a[8], uint32_t cnt[8])
{
    if (F == W8B) {
        const uint4 w = nodes[4 * (size_t)i + 3];
        const uint32_t child_base = w.z & 0xFFFFFFu, imask = w.z >> 24, tri_base = w.w & 0xFFFFFFu, lmask = w.w >> 24;
        uint32_t ni = 0, nl = 0;
        for (int k = 0; k < 8; k++) {
            cnt[k] = 1;
            if (imask >> k & 1u) { kind[k] = 2; a[k] = child_base + ni++; }
            else if (lmask >> k & 1u) { kind[k] = 1; a[k] = tri_base + nl++; }
            else { kind[k] = 0; a[k] = 0; }
        }
        return 8;
    }
    const uint4 w = F == W4F ? nodes[8 * (size_t)i + 6] : nodes[4 * (size_t)i + 3];
    const uint32_t word[4] = { w.x, w.y, w.z, w.w };
    for (int k = 0; k < 4; k++) {
        const uint32_t c = word[k];
        cnt[k] = 1;
        if (c == PT_MISS) { kind[k] = 0; a[k] = 0; }
        else if (c & PT_LEAF) { kind[k] = 1; a[k] = c & 0x0FFFFFFFu; cnt[k] = ((c >> 28) & 7u) + 1u; }
        else { kind[k] = 2; a[k] = c; }
    }
    return 4;
}

// parent of every node (PT_MISS: the root) and the number of internal children each node waits for
template <int F>
__global__ __launch_bounds__(TB) void k_rf_links(const uint4 *__restrict__ nodes, uint32_t n_nodes, uint32_t *__restrict__ parent,
                                                 uint32_t *__restrict__ pending)
{
    const uint32_t i = blockIdx.x * TB + threadIdx.x;
    if (i >= n_nodes) return;
    uint32_t kind[8], a[8], cnt[8];
    const int m = node_children<F>(nodes, i, kind, a, cnt);
    uint32_t p = 0;
    for (int k = 0; k < m; k++)
        if (kind[k] == 2u && a[k] < n_nodes) { parent[a[k]] = i; p++; }
    pending[i] = p;
}

template <int F>
__global__ __launch_bounds__(TB) void k_rf_up(uint4 *nodes, uint32_t n_nodes, const uint32_t *__restrict__ parent,
                                              const uint32_t *__restrict__ pending, uint32_t *arrive, float4 *ulo, float4 *uhi,
                                              const float4 *__restrict__ tlo, const float4 *__restrict__ thi,
                                              const uint32_t *__restrict__ prim_of, uint32_t n_tris, float pad,
                                              float cx, float cy, float cz, float rsx, float rsy, float rsz)
{
    uint32_t node = blockIdx.x * TB + threadIdx.x;
    if (node >= n_nodes || pending[node] != 0u) return;  // only the nodes without internal children start a climb
    const float c[3] = { cx, cy, cz }, rs[3] = { rsx, rsy, rsz };
    for (uint32_t step = 0; step < n_nodes; step++) {
        uint32_t kind[8], a[8], cnt[8];
        const int m = node_children<F>(nodes, node, kind, a, cnt);
        float lo[3][8], hi[3][8];
        float nlo[3] = { INFINITY, INFINITY, INFINITY }, nhi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (int k = 0; k < m; k++) {
            for (int ax = 0; ax < 3; ax++) { lo[ax][k] = INFINITY; hi[ax][k] = -INFINITY; }
            if (kind[k] == 1u) {
                for (uint32_t t = 0; t < cnt[k]; t++) {
                    const uint32_t pos = a[k] + t;
                    if (pos >= n_tris) break;
                    const uint32_t prim = prim_of[pos];
                    const float4 l = tlo[prim], h = thi[prim];
                    lo[0][k] = fminf(lo[0][k], l.x); lo[1][k] = fminf(lo[1][k], l.y); lo[2][k] = fminf(lo[2][k], l.z);
                    hi[0][k] = fmaxf(hi[0][k], h.x); hi[1][k] = fmaxf(hi[1][k], h.y); hi[2][k] = fmaxf(hi[2][k], h.z);
                }
                for (int ax = 0; ax < 3; ax++) { lo[ax][k] = lo[ax][k] - pad; hi[ax][k] = hi[ax][k] + pad; }
            } else if (kind[k] == 2u && a[k] < n_nodes) {
                const float4 l = ulo[a[k]], h = uhi[a[k]];  // published by the child's climb (acquired below)
                lo[0][k] = l.x; lo[1][k] = l.y; lo[2][k] = l.z;
                hi[0][k] = h.x; hi[1][k] = h.y; hi[2][k] = h.z;
            }
            if (kind[k] != 0u)
                for (int ax = 0; ax < 3; ax++) { nlo[ax] = fminf(nlo[ax], lo[ax][k]); nhi[ax] = fmaxf(nhi[ax], hi[ax][k]); }
        }
        if (F == W4F) {  // planes lo.x lo.y lo.z hi.x hi.y hi.z, empty slots keep +inf
            float4 *o = reinterpret_cast<float4 *>(nodes) + 8 * (size_t)node;
            for (int ax = 0; ax < 3; ax++) {
                float4 pl = o[ax], ph = o[3 + ax];
                if (kind[0]) { pl.x = lo[ax][0]; ph.x = hi[ax][0]; }
                if (kind[1]) { pl.y = lo[ax][1]; ph.y = hi[ax][1]; }
                if (kind[2]) { pl.z = lo[ax][2]; ph.z = hi[ax][2]; }
                if (kind[3]) { pl.w = lo[ax][3]; ph.w = hi[ax][3]; }
                o[ax] = pl; o[3 + ax] = ph;
            }
        } else if (F == W4H) {  // k_w4_emit's rounding; empty slots keep their +inf halves
            uint4 *o = nodes + 4 * (size_t)node;
            uint32_t d[12];
            { const uint4 q0 = o[0], q1 = o[1], q2 = o[2];
              d[0] = q0.x; d[1] = q0.y; d[2] = q0.z; d[3] = q0.w; d[4] = q1.x; d[5] = q1.y; d[6] = q1.z; d[7] = q1.w;
              d[8] = q2.x; d[9] = q2.y; d[10] = q2.z; d[11] = q2.w; }
            for (int k = 0; k < 4; k++) {
                if (!kind[k]) continue;
                const int sh = (k & 1) * 16;
                for (int ax = 0; ax < 3; ax++) {
                    const uint32_t hl = __half_as_ushort(__float2half_rd((lo[ax][k] - c[ax]) * rs[ax] - NORM_EPS));
                    const uint32_t hh = __half_as_ushort(__float2half_ru((hi[ax][k] - c[ax]) * rs[ax] + NORM_EPS));
                    uint32_t &wl = d[2 * ax + (k >> 1)], &wh = d[6 + 2 * ax + (k >> 1)];
                    wl = (wl & ~(0xFFFFu << sh)) | (hl << sh);
                    wh = (wh & ~(0xFFFFu << sh)) | (hh << sh);
                }
            }
            o[0] = make_uint4(d[0], d[1], d[2], d[3]);
            o[1] = make_uint4(d[4], d[5], d[6], d[7]);
            o[2] = make_uint4(d[8], d[9], d[10], d[11]);
        } else {  // W8B: k_w8_emit's grid and rounding
            float bl[3][8], bh[3][8], glo[3] = { INFINITY, INFINITY, INFINITY }, ghi[3] = { -INFINITY, -INFINITY, -INFINITY };
            for (int k = 0; k < 8; k++) {
                if (!kind[k]) continue;
                for (int ax = 0; ax < 3; ax++) {
                    bl[ax][k] = (lo[ax][k] - c[ax]) * rs[ax] - NORM_EPS;
                    bh[ax][k] = (hi[ax][k] - c[ax]) * rs[ax] + NORM_EPS;
                    glo[ax] = fminf(glo[ax], bl[ax][k]);
                    ghi[ax] = fmaxf(ghi[ax], bh[ax][k]);
                }
            }
            uint32_t o16[3], ecode[3], ql[3][8], qh[3][8];
            for (int ax = 0; ax < 3; ax++) {
                const double og = floor(((double)glo[ax] + 2.0) * 16384.0);
                o16[ax] = (uint32_t)fmin(fmax(og, 0.0), 65535.0);
                const double origin = (double)o16[ax] * (1.0 / 16384.0) - 2.0;
                const double ext = (double)ghi[ax] - origin;
                int e = -31;
                while (e < 0 && 255.0 * ldexp(1.0, e) < ext) e++;
                ecode[ax] = (uint32_t)(-e);
                const double inv_step = ldexp(1.0, -e);
                for (int k = 0; k < 8; k++) {
                    if (!kind[k]) { ql[ax][k] = 255u; qh[ax][k] = 0u; continue; }
                    ql[ax][k] = (uint32_t)fmin(fmax(floor(((double)bl[ax][k] - origin) * inv_step), 0.0), 255.0);
                    qh[ax][k] = (uint32_t)fmin(fmax(ceil(((double)bh[ax][k] - origin) * inv_step), 0.0), 255.0);
                }
            }
            auto pack4 = [](const uint32_t *q) { return q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24); };
            uint4 *o = nodes + 4 * (size_t)node;
            const uint4 w = o[3];
            o[0] = make_uint4(pack4(ql[0]), pack4(ql[0] + 4), pack4(ql[1]), pack4(ql[1] + 4));
            o[1] = make_uint4(pack4(ql[2]), pack4(ql[2] + 4), pack4(qh[0]), pack4(qh[0] + 4));
            o[2] = make_uint4(pack4(qh[1]), pack4(qh[1] + 4), pack4(qh[2]), pack4(qh[2] + 4));
            o[3] = make_uint4(o16[0] | (o16[1] << 16), o16[2] | (ecode[0] << 16) | (ecode[1] << 21) | (ecode[2] << 26), w.z, w.w);
        }
        ulo[node] = make_float4(nlo[0], nlo[1], nlo[2], 0.f);
        uhi[node] = make_float4(nhi[0], nhi[1], nhi[2], 0.f);
        const uint32_t p = parent[node];
        if (p >= n_nodes) return;  // the root
        // publish this node and its union, then arrive (agent-scope release; the explicit vmcnt wait keeps the arrival from
        // overtaking the write-back -- k_refit's hand-off)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t old = atomicAdd(&arrive[p], 1u);
        if (old + 1u != pending[p]) return;  // a sibling subtree is not finished: its last thread continues
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // acquire the siblings' unions
        node = p;
    }
}

template <int F>
pt_status refit_format(pt_ctx *ctx, void *nodes, uint32_t n_nodes, const float4 *tlo, const float4 *thi, const uint32_t *prim_of,
                       uint32_t n_tris, float pad, const float *c, const float *rs)
{
    hipStream_t st = ctx->stream;
    DevBuf<uint32_t> d_parent, d_pending, d_arrive;
    DevBuf<float4> d_ulo, d_uhi;
    PT_HIP(ctx, d_parent.alloc(n_nodes));
    PT_HIP(ctx, d_pending.alloc(n_nodes));
    PT_HIP(ctx, d_arrive.alloc(n_nodes));
    PT_HIP(ctx, d_ulo.alloc(n_nodes));
    PT_HIP(ctx, d_uhi.alloc(n_nodes));
    PT_HIP(ctx, hipMemsetAsync(d_parent.p, 0xFF, sizeof(uint32_t) * (size_t)n_nodes, st));
    PT_HIP(ctx, hipMemsetAsync(d_arrive.p, 0, sizeof(uint32_t) * (size_t)n_nodes, st));
    const uint32_t g = (n_nodes + TB - 1) / TB;
    uint4 *nd = static_cast<uint4 *>(nodes);
    k_rf_links<F><<<g, TB, 0, st>>>(nd, n_nodes, d_parent.p, d_pending.p);
    k_rf_up<F><<<g, TB, 0, st>>>(nd, n_nodes, d_parent.p, d_pending.p, d_arrive.p, d_ulo.p, d_uhi.p, tlo, thi, prim_of, n_tris, pad,
                                 c[0], c[1], c[2], rs[0], rs[1], rs[2]);
    PT_HIP(ctx, hipGetLastError());
    PT_HIP(ctx, hipStreamSynchronize(st));  // (the temporaries above are freed on return)
    return PT_OK;
}

}  // namespace

pt_status ptb_refit_wide(pt_ctx *ctx, int format, void *nodes, uint32_t n_nodes, const float4 *d_tlo, const float4 *d_thi,
                         const uint32_t *d_prim_of, uint32_t n_tris, float pad, const float *norm_c, const float *norm_rs)
{
    if (!nodes || !n_nodes) return PT_OK;
    switch (format) {
    case 0: return refit_format<W4F>(ctx, nodes, n_nodes, d_tlo, d_thi, d_prim_of, n_tris, pad, norm_c, norm_rs);
    case 1: return refit_format<W4H>(ctx, nodes, n_nodes, d_tlo, d_thi, d_prim_of, n_tris, pad, norm_c, norm_rs);
    case 2: return refit_format<W8B>(ctx, nodes, n_nodes, d_tlo, d_thi, d_prim_of, n_tris, pad, norm_c, norm_rs);
    default: ctx->err = "internal: unknown node format"; return PT_ERR_HIP;
    }
}
