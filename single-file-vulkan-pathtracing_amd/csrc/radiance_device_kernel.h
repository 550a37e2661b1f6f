// radiance_device_kernel.h -- the per-lane bodies of k_radiance_generate / k_radiance_resolve (radiance_device.hip), in a header of their own, like
// trace_device_kernel.h, so that tests/radiance_device_host.cpp can compile the very same statements for the host, run them over every slot of a
// chunk and hold the result against numpy without a GPU, under the host's sanitizers.  Wants declared before it: uint2, float2, float4 and their
// make_ functions, ptm::fdiv.  Compile with -ffp-contract=off: every operation of the reduce and the blend is rounded on its own.
//
// A chunk of m rays at spp samples is m * spp slots, sample-major: slot = s * m + r.  Neighbouring lanes of both kernels are neighbouring rays:
// the generate kernel's stores and the resolve kernel's loads are contiguous across a wave, and the first extend launch walks neighbouring rays
// side by side.  The queue record is k_generate's (wavefront_types.h QueueView): id = {slot, sample | depth << 16} with sample = depth = 0 (a
// slot has one sample, so k_shade never regenerates), state = {bits(seed), weight = 1, 1, 1}, rayA = {origin.xyz, direction.x}, rayB = {direction.yz}.
#pragma once

// common.glsl:21-31 in plain words (pt_math.h pcg2d over a uint2): the seed of a ray the caller gave no seed for
__device__ __forceinline__ uint32_t rd_hashed_seed(uint32_t index, uint32_t m)
{
    uint32_t x = index, y = m;
    x = x * 1664525u + 1013904223u;
    y = y * 1664525u + 1013904223u;
    x += y * 1664525u;
    y += x * 1664525u;
    x ^= x >> 16u;
    y ^= y >> 16u;
    x += y * 1664525u;
    y += x * 1664525u;
    x ^= x >> 16u;
    y ^= y >> 16u;
    return x + y;
}

struct RdCall {
    uint32_t spp;
    int32_t frame;
    uint32_t index_base;
    uint32_t accumulate;  // PT_RADIANCE_ACCUMULATE
};

// ---- k_radiance_generate: sample s of ray r of a chunk of m rays -> its accumulator zeroed, its record in queue 0 -------------------------------
// rays6 / seeds: the chunk's first row (seeds: spp words per ray, nullable); first: the chunk's first ray in the whole call (the hash takes the
// ray's position in the call, never in the chunk).  Rows of rays6 are 24 B apart and only 4-byte aligned: six dword loads.
__device__ __forceinline__ void rd_generate(const float *__restrict__ rays6, const uint32_t *__restrict__ seeds, const RdCall &c, uint64_t first,
                                            uint32_t r, uint32_t s, uint32_t m, float4 *__restrict__ color, uint2 *__restrict__ qid,
                                            float4 *__restrict__ qstate, float4 *__restrict__ rayA, float2 *__restrict__ rayB)
{
    const float *p = rays6 + 6 * (size_t)r;
    const float r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3], r4 = p[4], r5 = p[5];
    uint32_t seed;
    if (seeds) seed = seeds[(size_t)r * c.spp + s];
    else seed = rd_hashed_seed((uint32_t)(first + r) + c.index_base, s + c.spp * (uint32_t)c.frame + 1u);  // (make_seed's m, in wrapping arithmetic)
    const uint32_t slot = s * m + r;
    color[slot] = make_float4(0.f, 0.f, 0.f, 0.f);
    qid[slot] = make_uint2(slot, 0u);
    qstate[slot] = make_float4(__builtin_bit_cast(float, seed), 1.f, 1.f, 1.f);
    rayA[slot] = make_float4(r0, r1, r2, r3);
    rayB[slot] = make_float2(r4, r5);
}

// ---- the single-kernel form (PT_RADIANCE_FUSED: fused_kernel.h RAYS, fused_rays.hip): the index arithmetic of its slot hand-out ---------------
// The chunk's m * spp slots keep the layout above (slot = s * m + r), so k_radiance_resolve reads what the fused kernel stored.  The kernel hands
// slots out as k_fused does with one sample group: the launch's slot count, a multiple of 64, is cut into 64-slot chunks, part p of RDF_PARTS owns
// every RDF_PARTS-th chunk beginning with chunk p and has a counter of its own; position `mine` of part p is slot ((mine >> 6) * RDF_PARTS + p) * 64
// + (mine & 63).  m * spp is no multiple of 64 in general and the part arithmetic drops a partial last chunk, so the launch hands out
// rdf_launch_slots (rounded UP) and the kernel leaves the slots that are not live alone.  tests/radiance_fused_host.cpp runs these statements.
constexpr uint32_t RDF_PARTS = 8u;
// what a launch takes beside k_fused's arguments: the chunk's rows and seeds, and the two halves of the hashed seed's inputs that do not change
// with the slot -- index0 = (uint32)first + index_base (the ray's position in the call is first + r), seed_m0 = spp * (uint32)frame + 1
struct RdRays {
    const float *rays6;
    const uint32_t *seeds;
    uint32_t m, spp, index0, seed_m0;
};
inline RdRays rdf_rays(const float *rays6, const uint32_t *seeds, const RdCall &c, uint64_t first, uint32_t m)
{
    return { rays6, seeds, m, c.spp, (uint32_t)first + c.index_base, c.spp * (uint32_t)c.frame + 1u };
}
constexpr uint32_t rdf_launch_slots(uint32_t live) { return (live + 63u) & ~63u; }  // (the launcher's, on the host)
// positions part p hands out of a launch of ns slots (ns a multiple of 64): 64 x the chunks q < ns / 64 with q % RDF_PARTS == p
__device__ __forceinline__ uint32_t rdf_part_end(uint32_t ns, uint32_t part) { return (((ns >> 6) + RDF_PARTS - 1u - part) / RDF_PARTS) << 6; }
__device__ __forceinline__ uint32_t rdf_slot(uint32_t mine, uint32_t part) { return (((mine >> 6) * RDF_PARTS + part) << 6) + (mine & 63u); }
__device__ __forceinline__ bool rdf_live(uint32_t slot, uint32_t live) { return slot < live; }
// slot -> (sample, ray of the chunk); div_m divides by m (wavefront_types.h FastDiv, or anything with its div)
template <class Div>
__device__ __forceinline__ void rdf_sample_ray(uint32_t slot, uint32_t m, const Div &div_m, uint32_t &s, uint32_t &r)
{
    s = div_m.div(slot);
    r = slot - s * m;
}
// the seed rd_generate gives sample s of ray r
__device__ __forceinline__ uint32_t rdf_seed(const RdRays &a, uint32_t r, uint32_t s)
{
    return a.seeds ? a.seeds[(size_t)r * a.spp + s] : rd_hashed_seed(r + a.index0, s + a.seed_m0);
}

// ---- k_radiance_resolve: ray r of the chunk -> the ordered sum of its samples' accumulators, / spp, the store or the film's blend -------------
// radiance / moment2: the chunk's first row (moment2 nullable).  An old value is read only under accumulate at frame != 0.
__device__ __forceinline__ void rd_resolve(const float4 *__restrict__ color, const RdCall &c, uint32_t r, uint32_t m, float *__restrict__ radiance,
                                           float *__restrict__ moment2)
{
    float cr = 0.f, cg = 0.f, cb = 0.f, qr = 0.f, qg = 0.f, qb = 0.f;
    for (uint32_t s = 0; s < c.spp; s++) {
        const float4 a = color[(size_t)s * m + r];
        cr = cr + a.x; cg = cg + a.y; cb = cb + a.z;
        qr = qr + a.x * a.x; qg = qg + a.y * a.y; qb = qb + a.z * a.z;
    }
    const float spp = (float)c.spp;
    float v[3] = { ptm::fdiv(cr, spp), ptm::fdiv(cg, spp), ptm::fdiv(cb, spp) };
    float w[3] = { ptm::fdiv(qr, spp), ptm::fdiv(qg, spp), ptm::fdiv(qb, spp) };
    float *o = radiance + 3 * (size_t)r, *o2 = moment2 ? moment2 + 3 * (size_t)r : nullptr;
    if (c.accumulate) {  // the film's blend (k_resolve): new = (value + old * frame) / (frame + 1), the old value never read at frame 0
        const bool first = c.frame == 0;
        const float ff = (float)c.frame, f1 = (float)((uint32_t)c.frame + 1u);  // (frame >= 0 under accumulate)
        for (int k = 0; k < 3; k++) {
            v[k] = ptm::fdiv(v[k] + (first ? 0.f : o[k]) * ff, f1);
            if (o2) w[k] = ptm::fdiv(w[k] + (first ? 0.f : o2[k]) * ff, f1);
        }
    }
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    if (o2) { o2[0] = w[0]; o2[1] = w[1]; o2[2] = w[2]; }
}
