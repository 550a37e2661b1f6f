// trace_device_host.cpp -- the per-lane bodies of k_trace_pack, k_trace_occluded and k_trace_surface (csrc/trace_device_kernel.h) compiled for the
// host and run over arrays read from files: what tests/test_trace_device_cpu.py holds against numpy and the oracle without a GPU, and under the
// host's sanitizers.  Every array is a vector of exactly its size, so an index that leaves the queue or a table is the sanitizer's to find.  The
// IEEE divide and root (kernel_host.h) stand in for pt_math.h's fdiv and fsqrt, their bitwise equals; compile with -ffp-contract=off.  What
// kernel_host.h lacks for this header (float2) is brought here.
// usage: trace_device_host DIR   (DIR/par: 8 words, see main; rays6, dtmax, hit, hit_inst, tri4, rec64, faces, inst6, inst_frame in;
// o_rayA, o_rayB, o_bound, o_occ, o_position, o_normal, o_albedo, o_emission out)
#include "kernel_host.h"
struct alignas(8) float2 { float x, y; };
inline float2 make_float2(float a, float b) { return { a, b }; }
#define TD_LOADS_DONE()
#include "trace_device_kernel.h"
// wr for an array that may have no elements (a plane that was not asked for): fwrite wants a pointer even for none
template <class T> void wr0(const std::string &p, const std::vector<T> &v) { if (v.empty()) { FILE *f = fopen(p.c_str(), "wb"); if (!f || fclose(f) != 0) exit(2); } else wr(p, v); }
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: trace_device_host DIR\n"); return 2; }
    const std::string d = argv[1];
    // n n_tris n_inst has_frame has_dtmax want_bound planes (bit 0 position, 1 normal, 2 albedo, 3 emission) bits(tmax)
    auto par = rd<uint32_t>(d + "/par", 8);
    const uint32_t n = par[0], n_tris = par[1], n_inst = par[2];
    const bool has_frame = par[3] != 0, has_dtmax = par[4] != 0, want_bound = par[5] != 0;
    const uint32_t which = par[6];
    const float tmax = __builtin_bit_cast(float, par[7]);
    auto rays6 = rd<float>(d + "/rays6", 6 * (size_t)n), dtmax = rd<float>(d + "/dtmax", has_dtmax ? n : 0);
    auto hit = rd<float4>(d + "/hit", n);
    auto hit_inst = rd<uint32_t>(d + "/hit_inst", n_inst ? n : 0);
    auto tri4 = rd<float4>(d + "/tri4", 3 * (size_t)n_tris), rec64 = rd<float4>(d + "/rec64", 4 * (size_t)n_tris);
    auto faces = rd<float>(d + "/faces", 6 * (size_t)n_tris);
    auto inst6 = rd<float4>(d + "/inst6", 6 * (size_t)n_inst), inst_frame = rd<float4>(d + "/inst_frame", has_frame ? 2 * (size_t)n_inst * n_tris : 0);
    // outputs start as a canary (a NaN pattern), so a word the bodies leave alone shows
    const float canary = __builtin_bit_cast(float, 0x7FC0BEEFu);
    std::vector<float4> rayA(n, make_float4(canary, canary, canary, canary));
    std::vector<float2> rayB(n, make_float2(canary, canary));
    std::vector<float> bound(want_bound ? n : 0, canary);
    std::vector<uint8_t> occ(n, 0xEE);
    std::vector<float> plane[4];
    for (int k = 0; k < 4; k++) plane[k].assign((which >> k) & 1u ? 3 * (size_t)n : 0, canary);
    const TdScene sc = { tri4.data(), rec64.data(), faces.data(), n_inst ? inst6.data() : nullptr, has_frame ? inst_frame.data() : nullptr, n_tris };
    const auto ptr = [&](int k) { return (which >> k) & 1u ? plane[k].data() : nullptr; };
    const TdPlanes pl = { ptr(0), ptr(1), ptr(2), ptr(3) };
    for (uint32_t i = 0; i < n; i++) {  // (the three kernels, thread by thread)
        td_pack(rays6.data(), has_dtmax ? dtmax.data() : nullptr, tmax, i, rayA.data(), rayB.data(), want_bound ? bound.data() : nullptr);
        occ[i] = td_occluded(hit.data(), i);
        if (!n_inst) td_surface<false, false>(sc, hit.data(), nullptr, pl, i);
        else if (has_frame) td_surface<true, true>(sc, hit.data(), hit_inst.data(), pl, i);
        else td_surface<true, false>(sc, hit.data(), hit_inst.data(), pl, i);
    }
    wr(d + "/o_rayA", rayA); wr(d + "/o_rayB", rayB); wr0(d + "/o_bound", bound); wr(d + "/o_occ", occ);
    wr0(d + "/o_position", plane[0]); wr0(d + "/o_normal", plane[1]); wr0(d + "/o_albedo", plane[2]); wr0(d + "/o_emission", plane[3]);
    return 0;
}
