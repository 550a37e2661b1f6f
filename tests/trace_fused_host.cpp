// trace_fused_host.cpp -- the per-lane statements of k_trace_fused that touch the caller's arrays (csrc/trace_fused_kernel.h: row -> ray, the any-hit
// bound, finish record -> pt_hit row / surface planes / occluded byte) compiled for the host and run over arrays read from files: what
// tests/test_trace_fused_cpu.py holds against numpy and the oracle without a GPU, and under the host's sanitizers.  The walk stays on the device:
// the program is fed what the walk holds at a ray's end, (leaf position | MISS, t, V, W, det).  Every array is a vector of exactly its size, so an
// index that leaves a table or an output is the sanitizer's to find; the rays are read at an offset of one float from their allocation, so rows
// are only 4-byte aligned.  The IEEE divide (kernel_host.h) stands in for pt_math.h's fdiv, its bitwise equal; compile with -ffp-contract=off.
// usage: trace_fused_host DIR   (DIR/par: 6 words, see main; rays6 (one float of padding first), dtmax, best, tri4, rec64, faces in;
// o_rays, o_bound, o_hits, o_occ, o_position, o_normal, o_albedo, o_emission out)
#include "kernel_host.h"
struct alignas(8) float2 { float x, y; };
inline float2 make_float2(float a, float b) { return { a, b }; }
#define TD_LOADS_DONE()
#include "trace_fused_kernel.h"
template <class T> void wr0(const std::string &p, const std::vector<T> &v) { if (v.empty()) { FILE *f = fopen(p.c_str(), "wb"); if (!f || fclose(f) != 0) exit(2); } else wr(p, v); }
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: trace_fused_host DIR\n"); return 2; }
    const std::string d = argv[1];
    // n n_tris has_dtmax want_hits planes (bit 0 position, 1 normal, 2 albedo, 3 emission) bits(tmax)
    auto par = rd<uint32_t>(d + "/par", 6);
    const uint32_t n = par[0], n_tris = par[1];
    const bool has_dtmax = par[2] != 0, want_hits = par[3] != 0;
    const uint32_t which = par[4];
    const float tmax = __builtin_bit_cast(float, par[5]);
    auto rays_alloc = rd<float>(d + "/rays6", 1 + 6 * (size_t)n);
    const float *rays6 = rays_alloc.data() + 1;
    auto dtmax = rd<float>(d + "/dtmax", has_dtmax ? n : 0);
    auto best = rd<TfBest>(d + "/best", n);
    auto tri4 = rd<float4>(d + "/tri4", 3 * (size_t)n_tris), rec64 = rd<float4>(d + "/rec64", 4 * (size_t)n_tris);
    auto faces = rd<float>(d + "/faces", 6 * (size_t)n_tris);
    const float canary = __builtin_bit_cast(float, 0x7FC0BEEFu);
    std::vector<float> o_rays(6 * (size_t)n, canary), o_bound(n, canary);
    std::vector<uint32_t> hits(want_hits ? 5 * (size_t)n : 0, 0xEEEEEEEEu);
    std::vector<uint8_t> occ(n, 0xEE);
    std::vector<float> plane[4];
    for (int k = 0; k < 4; k++) plane[k].assign((which >> k) & 1u ? 3 * (size_t)n : 0, canary);
    const TdScene sc = { tri4.data(), rec64.data(), faces.data(), nullptr, nullptr, n_tris };
    const auto ptr = [&](int k) { return (which >> k) & 1u ? plane[k].data() : nullptr; };
    const TdPlanes pl = { ptr(0), ptr(1), ptr(2), ptr(3) };
    for (uint32_t i = 0; i < n; i++) {  // (the kernel's refill and finish, lane by lane)
        const TfRay r = tf_row(rays6, i);
        const float ray[6] = { r.ox, r.oy, r.oz, r.dx, r.dy, r.dz };
        std::copy(ray, ray + 6, o_rays.begin() + 6 * (size_t)i);
        o_bound[i] = tf_bound(has_dtmax ? dtmax.data() : nullptr, tmax, i);
        const float4 rec = tf_record(best[i]);
        if (want_hits) tf_hit_row(hits.data(), i, rec, tri4.data());
        if (which) tf_surface(sc, rec, pl, i);
        occ[i] = tf_occluded(best[i].pos);
    }
    wr(d + "/o_rays", o_rays); wr(d + "/o_bound", o_bound); wr0(d + "/o_hits", hits); wr(d + "/o_occ", occ);
    wr0(d + "/o_position", plane[0]); wr0(d + "/o_normal", plane[1]); wr0(d + "/o_albedo", plane[2]); wr0(d + "/o_emission", plane[3]);
    return 0;
}
