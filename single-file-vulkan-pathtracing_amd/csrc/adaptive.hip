// adaptive.hip -- pt_render_adaptive's device passes: which 8x8 tiles of a rank's list are traced, and the blend of their frames by each
// pixel's own frame count.
//
// The definition (the per-pixel relative standard error from C, M and K, the six-step xor butterfly over a tile's 64 lanes, short / capped,
// the blend with n = K_p in place of the frame, the byte rule) is the header's; tests/test_adaptive.py restates it in numpy and every
// comparison is byte equality.  So every operation here is one binary32 operation in the written order (-ffp-contract=off, __fdiv_rn, the
// correctly rounded root), and nothing is reassociated.
//
//   k_adapt_select    one wave per tile of the source list, one lane per pixel, four tiles per 256-thread block.  A lane makes the seven loads
//                     of its pixel (C, M, K; a lane outside the image from the clamped address) together, ahead of any test, and the loaded
//                     words are pinned (AD_KEEP).  The tile sum is six __shfl_xor steps: each step's add is commutative, so every lane holds the
//                     same bits afterwards and lane 0's value is the definition's.  short and capped are wave votes (ballots).  Lane 0 writes
//                     the tile's flag and its error word (the bits of e_T, 0 for a short tile).  No LDS, no scratch, no atomics.
//   exclusive_scan    device_scan.h over the n + 1 flags (the last one 0): flag[t] becomes the tile's place in the selection, flag[n] the count.
//   k_adapt_compact   a thread per tile: tile t is selected where its place differs from its successor's; its word goes to that place: the source
//                     list's order.  The record's sums go through one wave reduction and one atomic per wave (pixels: an integer sum; max
//                     error: a max over non-negative floats as their bits -- both order-free): a 1080p film has 32 400 tiles, and one atomic
//                     per tile on one address cost more than everything else of the pass together (the pass: 0.437 ms with them, 0.035 ms so).
//   k_resolve_adapt   k_resolve_m2's term-log replay (shade_kernels.hip resolve_pixel, restated: sharing it would have to leave k_resolve's code
//                     as it is), then ad_blend per frame and the store of K.
#include "wavefront_host.h"
#include "device_scan.h"

#include <cstring>

namespace {
using namespace ptw;

#define AD_KEEP(v) asm volatile("" : "+v"(v))  // the value exists in a vector register at this point: its load cannot move below
#include "adaptive_kernel.h"  // AdConst, ad_lane_error, ad_selected, AdPixel, ad_blend: the kernels' bodies

struct AdRecord {              // what the host reads once per call
    uint32_t count;            // selected tiles
    uint32_t max_err_bits;     // max e_T over the tiles without a short pixel, as the bits of a non-negative float
    unsigned long long pixels; // valid pixels of the selected tiles
};

__global__ __launch_bounds__(TB) void k_adapt_select(AdConst ac, const uint32_t *__restrict__ tiles, uint32_t n_tiles, const float *__restrict__ film,
                                                     const float *__restrict__ m2, const float *__restrict__ counts, uint32_t *__restrict__ flag,
                                                     uint32_t *__restrict__ err, AdRecord *__restrict__ rec)
{
    if (blockIdx.x == 0u && threadIdx.x == 0u) {  // what the passes behind this one start from: the scan's last word, an empty record
        flag[n_tiles] = 0u;
        *rec = AdRecord{ 0u, 0u, 0ull };
    }
    const uint32_t t = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (t >= n_tiles) return;  // (wave-uniform)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = tiles[t];
    const uint32_t px = (g & 0xFFFFu) * 8u + (lane & 7u), py = (g >> 16) * 8u + (lane >> 3);
    const bool valid = px < ac.w && py < ac.h;
    const size_t pix = (size_t)min(py, ac.h - 1u) * ac.w + min(px, ac.w - 1u);  // (a lane outside the image loads the nearest pixel inside and drops it)
    float c[3] = { film[3 * pix + 0], film[3 * pix + 1], film[3 * pix + 2] };
    float m[3] = { m2[3 * pix + 0], m2[3 * pix + 1], m2[3 * pix + 2] };
    float k = counts[pix];
    AD_KEEP(c[0]); AD_KEEP(c[1]); AD_KEEP(c[2]); AD_KEEP(m[0]); AD_KEEP(m[1]); AD_KEEP(m[2]); AD_KEEP(k);
    float x = ad_lane_error(valid, c, m, k, ac.rel_floor);
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) x = x + __shfl_xor(x, s, 64);
    const uint32_t n_valid = (uint32_t)__popcll(__ballot(valid));  // >= 1: a listed tile has its first pixel inside the image
    const float e_t = ptm::fdiv(x, (float)n_valid);
    const bool short_ = __ballot(ad_lane_short(valid, k, ac.min_frames)) != 0ull;
    const bool capped = ac.has_max != 0u && __ballot(ad_lane_below_max(valid, k, ac.max_frames)) == 0ull;
    const bool sel = ad_selected(short_, capped, e_t, ac.threshold);
    if (lane == 0u) {
        flag[t] = sel ? 1u : 0u;
        err[t] = (!short_ && e_t > 0.0f) ? __float_as_uint(e_t) : 0u;
    }
}

__global__ __launch_bounds__(TB) void k_adapt_compact(AdConst ac, const uint32_t *__restrict__ tiles, uint32_t n_tiles, const uint32_t *__restrict__ off,
                                                      const uint32_t *__restrict__ err, uint32_t *__restrict__ sel, AdRecord *__restrict__ rec)
{
    const uint32_t t = blockIdx.x * TB + threadIdx.x;
    uint32_t pixels = 0u, worst = 0u;  // (a thread behind the list adds nothing; it stays for the wave's reduction)
    if (t < n_tiles) {
        const uint32_t o = off[t], g = tiles[t];
        worst = err[t];
        if (off[t + 1] != o) {
            sel[o] = g;  // (o < the count <= n_tiles)
            pixels = min(8u, ac.w - (g & 0xFFFFu) * 8u) * min(8u, ac.h - (g >> 16) * 8u);  // the tile's pixels inside the image
        }
        if (t == 0u) rec->count = off[n_tiles];
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        pixels += __shfl_xor(pixels, s, 64);
        worst = max(worst, __shfl_xor(worst, s, 64));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (pixels) atomicAdd(&rec->pixels, (unsigned long long)pixels);
        if (worst) atomicMax(&rec->max_err_bits, worst);
    }
}

__global__ __launch_bounds__(TB) void k_resolve_adapt(RenderConst rc, const uint32_t *__restrict__ tiles, Radiance rad, float *__restrict__ film,
                                                      uint8_t *__restrict__ bgra, const unsigned long long *__restrict__ skip_if_set,
                                                      float *__restrict__ m2, float *__restrict__ counts)
{
    const uint32_t local = blockIdx.x * TB + threadIdx.x;
    if (local >= rc.slots_per_lane) return;
    if (skip_if_set && *skip_if_set != 0ull) return;  // (a term log overflowed in the launch before: the host renders these frames again)
    uint32_t f0, g0, px, py;
    slot_pixel(rc, tiles, local, f0, g0, px, py);
    if (px >= rc.width || py >= rc.height) return;
    const size_t pix = (size_t)py * rc.width + px;
    AdPixel p;
#pragma unroll
    for (int k = 0; k < 3; k++) { p.c[k] = film[3 * pix + k]; p.m[k] = m2[3 * pix + k]; }
    p.img = reinterpret_cast<uchar4 *>(bgra)[pix];
    p.n = counts[pix];
    const float spp = (float)rc.spp;
    for (uint32_t f = 0; f < rc.lanes_active; f++) {
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rc.groups == 1u) c = rad.color[(size_t)f * rc.slots_per_lane + local];
        // (head + tail with the cull: the head slot of a pixel outside the rectangle holds all its samples, its tail slots were never written)
        const bool no_tails = rc.tail && rc.cull_on && ((int32_t)px < rc.cull[0] || (int32_t)px > rc.cull[2] || (int32_t)py < rc.cull[1] || (int32_t)py > rc.cull[3]);
        if ((rc.groups > 1u || rc.tail) && !no_tails) {  // the groups' (or the one-sample tail slots') term logs in sample order
            const uint32_t n_logs = rc.tail ? rc.tail : rc.groups;
            const size_t log_slots = rc.tail ? rc.n_tail : rc.n_slots;
            for (uint32_t g = 0; g < n_logs; g++) {
                const size_t slot = ((size_t)f * n_logs + g) * rc.slots_per_lane + local;
                const uint32_t nt_all = rad.nterm[slot], nt = min(nt_all, rc.term_cap);
                const float4 *to = rad.terms_over + slot * (rc.term_cap - rc.term_pcap);
                for (uint32_t k = 0; k < nt; k++) {
                    const float4 e = k < rc.term_pcap ? rad.terms[(size_t)k * log_slots + slot] : to[k - rc.term_pcap];
                    c.x = c.x + e.x;
                    c.y = c.y + e.y;
                    c.z = c.z + e.z;
                }
                // the few slots with more terms: pool entries chained newest-first, the j-th in path order m-1-j links down
                const uint32_t m = nt_all - nt;
                for (uint32_t j = 0; j < m; j++) {
                    uint32_t idx = rad.spill_head[slot];
                    for (uint32_t w = j + 1; w < m && idx != SPILL_NONE; w++) idx = __float_as_uint(rad.spill[idx].w);
                    if (idx == SPILL_NONE) break;
                    const float4 e = rad.spill[idx];
                    c.x = c.x + e.x;
                    c.y = c.y + e.y;
                    c.z = c.z + e.z;
                }
            }
        }
        ad_blend(p, ptm::fdiv(c.x, spp), ptm::fdiv(c.y, spp), ptm::fdiv(c.z, spp));  // raygen.rgen:86, then the blend by the pixel's count
    }
#pragma unroll
    for (int k = 0; k < 3; k++) { film[3 * pix + k] = p.c[k]; m2[3 * pix + k] = p.m[k]; }
    reinterpret_cast<uchar4 *>(bgra)[pix] = p.img;
    counts[pix] = p.n;
}

}  // namespace

void ptad_free(pt_film *f)
{
    pt_film::Adapt &a = f->ad;
    pt_scratch_free({ pt_buf_of(a.d_sel), pt_buf_of(a.d_off), pt_buf_of(a.d_err), pt_buf_of(a.d_sums), pt_buf_of(a.d_rec) }, &a.bytes, a.bytes);
    a = pt_film::Adapt{};
}

pt_status ptad_select(pt_film *f, const pt_adaptive_params *ap, const TileView &src, TileView *out, pt_adaptive_result *res)
{
    pt_ctx *ctx = f->ctx;
    pt_film::Adapt &a = f->ad;
    *out = TileView{};
    *res = pt_adaptive_result{};
    res->tiles_total = src.n_tiles;
    if (src.n_tiles == 0) return PT_OK;  // (a rank without tiles)
    const uint32_t n = src.n_tiles;
    if (n > a.cap) {
        const size_t scan_blocks = ((size_t)n + 1 + SC_TILE - 1) / SC_TILE;
        const pt_status ra = pt_scratch_alloc(ctx, "adaptive selection", { pt_buf_of(a.d_sel, sizeof(uint32_t) * n), pt_buf_of(a.d_off, sizeof(uint32_t) * ((size_t)n + 1)),
                                                                        pt_buf_of(a.d_err, sizeof(uint32_t) * n),
                                                                        pt_buf_of(a.d_sums, sizeof(uint32_t) * scan_blocks), pt_buf_of(a.d_rec, sizeof(AdRecord)) },
                                              &a.bytes, a.bytes, f->work.bytes + f->aov.bytes + f->dn.bytes + f->up.bytes, ctx->mem_budget);
        a.cap = ra == PT_OK ? n : 0;
        if (ra != PT_OK) return ra;
    }
    AdConst ac{};
    ac.w = f->w; ac.h = f->h;
    ac.threshold = ap->threshold; ac.rel_floor = ap->rel_floor;
    ac.min_frames = (float)ap->min_frames; ac.max_frames = (float)ap->max_frames;
    ac.has_max = ap->max_frames > 0u ? 1u : 0u;
    AdRecord *d_rec = static_cast<AdRecord *>(a.d_rec);
    AdRecord h_rec{};
    float ms = 0.f;
    PT_TRY(pt_timed_pass(ctx, &ms, [&](hipStream_t s_) {
        k_adapt_select<<<(n + TB / 64 - 1) / (TB / 64), TB, 0, s_>>>(ac, src.d_tiles, n, f->d_rgb, f->m2.ptr(), f->cnt.ptr(), a.d_off, a.d_err, d_rec);
        exclusive_scan(a.d_off, n + 1, a.d_sums, s_);
        k_adapt_compact<<<(n + TB - 1) / TB, TB, 0, s_>>>(ac, src.d_tiles, n, a.d_off, a.d_err, a.d_sel, d_rec);
    }));
    PT_HIP(ctx, hipMemcpy(&h_rec, d_rec, sizeof(h_rec), hipMemcpyDeviceToHost));  // the one read-back of the call
    res->tiles_selected = h_rec.count;
    res->pixels_selected = h_rec.pixels;
    std::memcpy(&res->max_error, &h_rec.max_err_bits, sizeof(float));
    res->select_ms = ms;
    *out = { a.d_sel, h_rec.count, h_rec.pixels, f->cnt.ptr() };
    return PT_OK;
}

void ptw_launch_resolve_adapt(const ptw::RenderConst &rc, const uint32_t *tiles, const ptw::Radiance &rad, float *film, uint8_t *bgra, hipStream_t st,
                              const unsigned long long *skip_if_set, float *m2, float *counts)
{
    const uint32_t grid = (rc.slots_per_lane + TB - 1) / TB;
    k_resolve_adapt<<<grid, TB, 0, st>>>(rc, tiles, rad, film, bgra, skip_if_set, m2, counts);
}
