// radiance_fused_host.cpp -- the index arithmetic of pt_radiance_device's single-kernel form (csrc/radiance_device_kernel.h rdf_*: what the RAYS
// instantiations of csrc/fused_kernel.h hand slots out by) compiled for the host and run as the kernel's waves run it: eight part counters, each
// advanced 64 positions per draw, drained by draws that start on an arbitrary part and steal in ring order, as a wave does.  What
// tests/test_radiance_fused_cpu.py holds against numpy, plain and under the host's sanitizers.  Every array is a vector of exactly its size: a
// slot beyond the launch's, a ray beyond the chunk's or a seed beyond the table's is the sanitizer's to find.
// FastDiv is wavefront_types.h's, restated (that header needs HIP): the same init, __umulhi as a 64-bit product.
// usage: radiance_fused_host DIR   (DIR/par: 7 words, see main; seeds in; o_count, o_s, o_r, o_seed, o_meta out)
#include "kernel_host.h"
struct alignas(8) float2 { float x, y; };
inline float2 make_float2(float a, float b) { return { a, b }; }
inline uint2 make_uint2(uint32_t a, uint32_t b) { return { a, b }; }
#include "radiance_device_kernel.h"

struct FastDiv {
    uint32_t m = 1, s1 = 0, s2 = 0;
    void init(uint32_t d)
    {
        uint32_t l = 0;
        while ((1ull << l) < d) l++;
        m = (uint32_t)((((1ull << l) - d) << 32) / d + 1ull);
        s1 = l < 1u ? l : 1u;
        s2 = l > 0u ? l - 1u : 0u;
    }
    uint32_t div(uint32_t n) const
    {
        const uint32_t t = (uint32_t)(((uint64_t)m * n) >> 32);
        return (t + ((n - t) >> s1)) >> s2;
    }
};

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: radiance_fused_host DIR\n"); return 2; }
    const std::string d = argv[1];
    // m spp frame index_base has_seeds first (the chunk's first ray in the call) order (seeds the order of the draws)
    auto par = rd<uint32_t>(d + "/par", 7);
    const uint32_t m = par[0], spp = par[1];
    const RdCall call = { spp, (int32_t)par[2], par[3], 0u };
    const bool has_seeds = par[4] != 0;
    const uint64_t first = par[5];
    uint32_t order = par[6];
    const uint32_t live = m * spp, ns = rdf_launch_slots(live);
    auto seeds = rd<uint32_t>(d + "/seeds", has_seeds ? live : 0);
    std::vector<float> rays6(6 * (size_t)m, 0.f);
    const RdRays rr = rdf_rays(rays6.data(), has_seeds ? seeds.data() : nullptr, call, first, m);
    FastDiv div_m;
    div_m.init(m);
    std::vector<uint32_t> count(ns, 0u);                              // how often each slot of the LAUNCH was handed out
    std::vector<uint32_t> o_s(live, ~0u), o_r(live, ~0u), o_seed(live, 0u);
    uint32_t cnt[RDF_PARTS] = {};                                     // the part counters (fused_kernel.h: next_slot, one per 128-B line)
    uint32_t draws = 0, masked = 0, positions = 0;
    // the waves of the launch, one draw at a time: a wave starts on a part of its own and moves on in ring order when the part is exhausted; it is
    // out of slots once it has found all eight empty (fused_kernel.h FB_DRAW).  Each turn of this loop is one wave's whole life; the order in which
    // waves come and the part they start on are arbitrary, and a wave stops drawing at an arbitrary time (other waves take what it leaves).
    for (uint32_t wave = 0; wave < 4096u; wave++) {
        order = order * 1664525u + 1013904223u;
        uint32_t w_part = (order >> 24) % RDF_PARTS, w_tried = 0;
        uint32_t budget = wave < 4000u ? 1u + ((order >> 8) & 7u) : ~0u;  // (the last waves drain whatever is left)
        bool out_of_slots = false;
        while (!out_of_slots && budget--) {
            uint32_t w_next = 0, w_end = 0;
            for (;;) {
                const uint32_t part_end = rdf_part_end(ns, w_part);
                const uint32_t rel = cnt[w_part];
                cnt[w_part] += 64u;                                   // (atomicAdd(cnt, PT_FUSED_BATCH1))
                draws++;
                if (0u < part_end && rel < part_end) { w_next = rel; w_end = std::min(rel + 64u, part_end); break; }
                w_part = (w_part + 1u) % RDF_PARTS;
                if (++w_tried >= RDF_PARTS) { out_of_slots = true; break; }
            }
            for (uint32_t mine = w_next; mine < w_end; mine++) {      // (the lanes that take the positions of the draw)
                positions++;
                const uint32_t slot = rdf_slot(mine, w_part);
                count.at(slot)++;
                if (!rdf_live(slot, live)) { masked++; continue; }
                uint32_t s, r;
                rdf_sample_ray(slot, m, div_m, s, r);
                (void)rays6.at(6 * (size_t)r + 5);                    // (the row the kernel loads)
                o_s.at(slot) = s; o_r.at(slot) = r;
                o_seed.at(slot) = rdf_seed(rr, r, s);
            }
        }
    }
    uint32_t left = 0;
    for (uint32_t p = 0; p < RDF_PARTS; p++) left += cnt[p] < rdf_part_end(ns, p) ? 1u : 0u;
    wr(d + "/o_count", count); wr(d + "/o_s", o_s); wr(d + "/o_r", o_r); wr(d + "/o_seed", o_seed);
    wr(d + "/o_meta", std::vector<uint32_t>{ ns, live, positions, masked, left, draws });
    return 0;
}
