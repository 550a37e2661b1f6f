// radiance_device_host.cpp -- the per-lane bodies of k_radiance_generate and k_radiance_resolve (csrc/radiance_device_kernel.h) compiled for the
// host and run over arrays read from files: what tests/test_radiance_device_cpu.py holds against numpy without a GPU, and under the host's
// sanitizers.  Every array is a vector of exactly its size, so an index that leaves a queue or a plane is the sanitizer's to find.  The IEEE
// divide (kernel_host.h) stands in for pt_math.h's fdiv, its bitwise equal; compile with -ffp-contract=off.  What kernel_host.h lacks for this
// header (float2, make_uint2) is brought here.
// usage: radiance_device_host DIR   (DIR/par: 8 words, see main; rays6, seeds, color, radiance, moment2 in;
// o_color, o_qid, o_qstate, o_rayA, o_rayB, o_radiance, o_moment2 out)
#include "kernel_host.h"
struct alignas(8) float2 { float x, y; };
inline float2 make_float2(float a, float b) { return { a, b }; }
inline uint2 make_uint2(uint32_t a, uint32_t b) { return { a, b }; }
#include "radiance_device_kernel.h"
template <class T> void wr0(const std::string &p, const std::vector<T> &v) { if (v.empty()) { FILE *f = fopen(p.c_str(), "wb"); if (!f || fclose(f) != 0) exit(2); } else wr(p, v); }
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: radiance_device_host DIR\n"); return 2; }
    const std::string d = argv[1];
    // m spp frame index_base accumulate has_seeds has_moment2 first (the chunk's first ray in the call)
    auto par = rd<uint32_t>(d + "/par", 8);
    const uint32_t m = par[0], spp = par[1];
    const RdCall call = { spp, (int32_t)par[2], par[3], par[4] };
    const bool has_seeds = par[5] != 0, has_m2 = par[6] != 0;
    const uint64_t first = par[7];
    const size_t slots = (size_t)m * spp;
    auto rays6 = rd<float>(d + "/rays6", 6 * (size_t)m);
    auto seeds = rd<uint32_t>(d + "/seeds", has_seeds ? slots : 0);
    auto color = rd<float4>(d + "/color", slots);  // the accumulators as the rounds left them (the resolve's input)
    auto radiance = rd<float>(d + "/radiance", 3 * (size_t)m);  // the old values (a canary where none may be read)
    auto moment2 = rd<float>(d + "/moment2", has_m2 ? 3 * (size_t)m : 0);
    const float canary = __builtin_bit_cast(float, 0x7FC0BEEFu);
    std::vector<float4> zeroed(slots, make_float4(canary, canary, canary, canary)), qstate(zeroed), rayA(zeroed);
    std::vector<uint2> qid(slots, make_uint2(0xEEEEEEEEu, 0xEEEEEEEEu));
    std::vector<float2> rayB(slots, make_float2(canary, canary));
    for (uint32_t s = 0; s < spp; s++)  // (the two kernels, thread by thread)
        for (uint32_t r = 0; r < m; r++)
            rd_generate(rays6.data(), has_seeds ? seeds.data() : nullptr, call, first, r, s, m, zeroed.data(), qid.data(), qstate.data(), rayA.data(), rayB.data());
    for (uint32_t r = 0; r < m; r++) rd_resolve(color.data(), call, r, m, radiance.data(), has_m2 ? moment2.data() : nullptr);
    wr(d + "/o_color", zeroed); wr(d + "/o_qid", qid); wr(d + "/o_qstate", qstate); wr(d + "/o_rayA", rayA); wr(d + "/o_rayB", rayB);
    wr(d + "/o_radiance", radiance); wr0(d + "/o_moment2", moment2);
    return 0;
}
