// range_host.cpp -- csrc/hit_rule.h (the range a walk hands its leaf test, the range check and the closest rules behind it) compiled for the host
// and driven over the ends of the range: what tests/test_ray_range_cpu.py holds against include/pt_api.h's rule written in numpy, plain and under
// the host's sanitizers.
// usage: range_host DIR  (DIR/par: n_cases; DIR/tmin, DIR/tmax, DIR/bound, DIR/t: one float per case.
//   Out, one byte per case and rule R in {single, inst}:
//     DIR/o_any_R      an any-hit walk that has hit nothing yet (best_t = bound) is offered a triangle at t: taken?  The leaf test ends at
//                      leaf_upper(true, best_t, tmax)
//     DIR/o_old_R      the same with the leaf test ending at tmax, as it did before the any-hit walks were given leaf_upper
//     DIR/o_closest_R  a closest-hit walk that has hit nothing yet (best_t = tmax), leaf test ending at leaf_upper(false, best_t, tmax)
//     DIR/o_tie_R      a closest-hit walk that HAS a hit at t (primitive id 7, instance id 3) is offered a second triangle at the same t with a
//                      lower id, then one with a higher id: bit 0 = the lower one was taken, bit 1 = the higher one was taken)
#include "kernel_host.h"
#include "hit_rule.h"

struct Best {
    float t, V = 0.f, W = 0.f, det = 1.f;
    uint32_t pos = PT_MISS, prim = PT_MISS, ipos = PT_MISS, iid = PT_MISS;
};

// two triangles' records (three float4 each, the id in the third one's .w): position 0 has id 7, position 1 has id 2, position 2 has id 9
static std::vector<float4> tri4_ids()
{
    std::vector<float4> v(9, float4{ 0.f, 0.f, 0.f, 0.f });
    const uint32_t ids[3] = { 7u, 2u, 9u };
    for (int k = 0; k < 3; k++) v[3 * k + 2].w = __builtin_bit_cast(float, ids[k]);
    return v;
}

template <bool INST>
static bool offer(const std::vector<float4> &tri4, Best &b, float t, float tmin, float upper, uint32_t pos, uint32_t prim, uint32_t iid)
{
    const float tt = ptl::in_range(t, tmin, upper) ? t : __builtin_nanf("");  // (pair_leaf.h: outside the range a NaN goes on)
    bool took;
    if (INST) took = ptl::closer_instanced(tt, 0.25f, 0.5f, 2.f, pos, prim, 5u, iid, b.t, b.V, b.W, b.det, b.pos, b.prim, b.ipos, b.iid);
    else took = ptl::closer_single_level(tri4.data(), 0u, tt, 0.25f, 0.5f, 2.f, pos, b.t, b.V, b.W, b.det, b.pos);
    if (took && !(b.t == t && b.pos == pos && b.V == 0.25f && b.W == 0.5f && b.det == 2.f)) { fprintf(stderr, "a taken hit is not the best hit\n"); exit(3); }
    return took;
}

template <bool INST>
static void run(const std::string &d, const char *name, const std::vector<float> &tmin, const std::vector<float> &tmax, const std::vector<float> &bound,
                const std::vector<float> &t)
{
    const size_t n = t.size();
    const std::vector<float4> tri4 = tri4_ids();
    std::vector<uint8_t> any(n), old(n), closest(n), tie(n);
    for (size_t c = 0; c < n; c++) {
        Best b;
        b.t = bound[c];
        any[c] = offer<INST>(tri4, b, t[c], tmin[c], ptl::leaf_upper(true, b.t, tmax[c]), 0u, 7u, 3u);
        b = Best();
        b.t = bound[c];
        old[c] = offer<INST>(tri4, b, t[c], tmin[c], tmax[c], 0u, 7u, 3u);
        b = Best();
        b.t = tmax[c];
        closest[c] = offer<INST>(tri4, b, t[c], tmin[c], ptl::leaf_upper(false, b.t, tmax[c]), 0u, 7u, 3u);
        uint8_t bits = 0;
        if (closest[c]) {  // the walk holds (t, position 0, id 7, instance 3): same t, a lower id (position 1, id 2), then a higher one (position 2, id 9)
            Best lo = b, hi = b;
            bits |= offer<INST>(tri4, lo, t[c], tmin[c], ptl::leaf_upper(false, lo.t, tmax[c]), 1u, 2u, 3u) ? 1u : 0u;
            bits |= offer<INST>(tri4, hi, t[c], tmin[c], ptl::leaf_upper(false, hi.t, tmax[c]), 2u, 9u, 3u) ? 2u : 0u;
            if (INST) {  // ... and the instance id goes first: a higher primitive id of a lower instance wins, a lower one of a higher instance loses
                Best a = b, z = b;
                if (!offer<INST>(tri4, a, t[c], tmin[c], tmax[c], 2u, 9u, 1u) || offer<INST>(tri4, z, t[c], tmin[c], tmax[c], 1u, 2u, 4u)) bits |= 4u;
            }
        }
        tie[c] = bits;
    }
    const std::string s = name;
    wr(d + "/o_any_" + s, any); wr(d + "/o_old_" + s, old); wr(d + "/o_closest_" + s, closest); wr(d + "/o_tie_" + s, tie);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: range_host DIR\n"); return 2; }
    const std::string d = argv[1];
    const size_t n = rd<uint32_t>(d + "/par", 1)[0];
    const auto tmin = rd<float>(d + "/tmin", n), tmax = rd<float>(d + "/tmax", n), bound = rd<float>(d + "/bound", n), t = rd<float>(d + "/t", n);
    run<false>(d, "single", tmin, tmax, bound, t);
    run<true>(d, "inst", tmin, tmax, bound, t);
    return 0;
}
