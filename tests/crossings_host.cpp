// crossings_host.cpp -- the per-lane statements that define pt_crossings_device's result (csrc/crossings_kernel.h: the reciprocal, the slab test,
// the own padded box, which rays walk, what counts, row -> ray, the writer) compiled for the host and run over arrays read from files: what
// tests/test_crossings_cpu.py holds against the numpy restatement of tests/crossings_cases.py without a GPU, and under the host's sanitizers.
// The tree walk stays on the device; here cx_counts runs over ALL triangles of a scene, which is what the walk has to equal.  Every array is a
// vector of exactly its size, so an index that leaves a table or an output is the sanitizer's to find; the rays are read at an offset of one
// float from their allocation, so rows are only 4-byte aligned.
// ptm::ray_setup and ptm::tri_test live in pt_math.h, which is device code; they are restated below statement for statement (ray_setup in its
// IEEE form, which its short form is proven equal to; the IEEE divide of kernel_host.h stands in for fdiv).  What pins THEM is the oracle's
// brute-force closest hit (test_crossings_cpu.py) and the GPU tests' byte equality.  Compile with -ffp-contract=off.
// usage: crossings_host DIR   (DIR/par: n_pairs n_boxes n_rays n_tris has_bounds points_form want_count want_winding
//                                       bits(tmin) bits(tmax) bits(pad) bits(direction x, y, z))
//   pairs   n_pairs x {O, D, tmin, b, pad, A, B, C} (18 floats)  -> o_flags n_pairs x {live, box, tri, s + 1} bytes, o_vals n_pairs x {t, det,
//           inv.xyz, lo.xyz, hi.xyz} (11 floats)
//   boxes   n_pairs x n_boxes x {lo, hi}                          -> o_boxes n_pairs x n_boxes bytes: cx_slab of the pair's ray
//   rays    one float of padding, n_rays x 6 (x 3 in the points form); bounds n_rays (has_bounds); tris n_tris x {A, B, C} (9 floats)
//           -> o_count n_rays u32, o_winding n_rays i32 (the loop over all triangles, written by cx_write over canaries; an output not wanted
//           does not exist)
#include "kernel_host.h"
namespace ptm {
struct f3 { float x, y, z; };
struct RayPre { f3 org; float Sx, Sy, Sz; int kz; };
inline float sel3(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }
inline RayPre ray_setup(const f3 org, const f3 dir)
{
    RayPre r;
    int kz = 0;
    if (fabsf(dir.y) > fabsf(dir.x)) kz = 1;
    if (fabsf(dir.z) > fabsf(sel3(kz, dir.x, dir.y, dir.z))) kz = 2;
    const float dkx = sel3(kz, dir.y, dir.z, dir.x), dky = sel3(kz, dir.z, dir.x, dir.y), dkz = sel3(kz, dir.x, dir.y, dir.z);
    r.Sx = fdiv(dkx, dkz); r.Sy = fdiv(dky, dkz); r.Sz = fdiv(1.0f, dkz);
    r.kz = kz; r.org = org;
    return r;
}
inline bool tri_test(const RayPre &r, const f3 v0, const f3 v1, const f3 v2, float tmin, float tmax, float &t, float &Vn, float &Wn, float &detn)
{
    const f3 A = { v0.x - r.org.x, v0.y - r.org.y, v0.z - r.org.z };
    const f3 B = { v1.x - r.org.x, v1.y - r.org.y, v1.z - r.org.z };
    const f3 C = { v2.x - r.org.x, v2.y - r.org.y, v2.z - r.org.z };
    const int kz = r.kz;
    const float Akx = sel3(kz, A.y, A.z, A.x), Aky = sel3(kz, A.z, A.x, A.y), Akz = sel3(kz, A.x, A.y, A.z);
    const float Bkx = sel3(kz, B.y, B.z, B.x), Bky = sel3(kz, B.z, B.x, B.y), Bkz = sel3(kz, B.x, B.y, B.z);
    const float Ckx = sel3(kz, C.y, C.z, C.x), Cky = sel3(kz, C.z, C.x, C.y), Ckz = sel3(kz, C.x, C.y, C.z);
    const float Ax = Akx - r.Sx * Akz, Ay = Aky - r.Sy * Akz;
    const float Bx = Bkx - r.Sx * Bkz, By = Bky - r.Sy * Bkz;
    const float Cx = Ckx - r.Sx * Ckz, Cy = Cky - r.Sy * Ckz;
    const float U = Cx * By - Cy * Bx;
    const float V = Ax * Cy - Ay * Cx;
    const float W = Bx * Ay - By * Ax;
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
    const float det = (U + V) + W;
    if (det == 0.0f) return false;
    const float Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    const float T = (U * Az + V * Bz) + W * Cz;
    const float tt = fdiv(T, det);
    if (!(tt > tmin && tt < tmax)) return false;
    t = tt; Vn = V; Wn = W; detn = det;
    return true;
}
}  // namespace ptm
#include "crossings_kernel.h"
template <class T> void wr0(const std::string &p, const std::vector<T> &v) { if (v.empty()) { FILE *f = fopen(p.c_str(), "wb"); if (!f || fclose(f) != 0) exit(2); } else wr(p, v); }
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: crossings_host DIR\n"); return 2; }
    const std::string d = argv[1];
    auto par = rd<uint32_t>(d + "/par", 14);
    const size_t n_pairs = par[0], n_boxes = par[1], n_rays = par[2], n_tris = par[3];
    const bool has_bounds = par[4] != 0, points_form = par[5] != 0, want_count = par[6] != 0, want_winding = par[7] != 0;
    const float tmin = __builtin_bit_cast(float, par[8]), tmax = __builtin_bit_cast(float, par[9]), pad = __builtin_bit_cast(float, par[10]);
    const ptm::f3 dir = { __builtin_bit_cast(float, par[11]), __builtin_bit_cast(float, par[12]), __builtin_bit_cast(float, par[13]) };
    // ---- pairs and their boxes
    auto pairs = rd<float>(d + "/pairs", 18 * n_pairs);
    auto boxes = rd<float>(d + "/boxes", 6 * n_pairs * n_boxes);
    std::vector<uint8_t> o_flags(4 * n_pairs), o_boxes(n_pairs * n_boxes);
    std::vector<float> o_vals(11 * n_pairs);
    for (size_t i = 0; i < n_pairs; i++) {
        const float *p = pairs.data() + 18 * i;
        const ptm::f3 O = { p[0], p[1], p[2] }, D = { p[3], p[4], p[5] };
        const float lo_t = p[6], b = p[7], pd = p[8];
        const ptm::f3 A = { p[9], p[10], p[11] }, B = { p[12], p[13], p[14] }, C = { p[15], p[16], p[17] };
        const CxRay r = cx_setup(O, D);
        bool box = false, tri = false;
        float t = 0.f, det = 0.f;
        const int s = cx_counts(r, lo_t, b, pd, A, B, C, &box, &tri, &t, &det);
        ptm::f3 lo, hi;
        cx_own_box(A, B, C, pd, lo, hi);
        const uint8_t fl[4] = { (uint8_t)cx_live(O, D, lo_t, b), (uint8_t)box, (uint8_t)tri, (uint8_t)(s + 1) };
        std::copy(fl, fl + 4, o_flags.begin() + 4 * i);
        const float v[11] = { t, det, r.inv.x, r.inv.y, r.inv.z, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z };
        std::copy(v, v + 11, o_vals.begin() + 11 * i);
        for (size_t k = 0; k < n_boxes; k++) {
            const float *q = boxes.data() + 6 * (i * n_boxes + k);
            o_boxes[i * n_boxes + k] = cx_slab({ q[0], q[1], q[2] }, { q[3], q[4], q[5] }, O, r.inv, lo_t, b);
        }
    }
    wr0(d + "/o_flags", o_flags); wr0(d + "/o_vals", o_vals); wr0(d + "/o_boxes", o_boxes);
    // ---- a scene: rows, bounds, the loop over all triangles, the writer
    const size_t width = points_form ? 3 : 6;
    auto rays_alloc = rd<float>(d + "/rays", 1 + width * n_rays);
    const float *rows = rays_alloc.data() + 1;
    auto bounds = rd<float>(d + "/bounds", has_bounds ? n_rays : 0);
    auto tris = rd<float>(d + "/tris", 9 * n_tris);
    std::vector<uint32_t> o_count(want_count ? n_rays : 0, 0xEEEEEEEEu);
    std::vector<int32_t> o_winding(want_winding ? n_rays : 0, (int32_t)0xEEEEEEEEu);
    for (uint32_t i = 0; i < n_rays; i++) {  // (the kernel's refill and finish, lane by lane)
        ptm::f3 O, D;
        cx_ray(points_form ? nullptr : rows, points_form ? rows : nullptr, dir, i, O, D);
        const float b = cx_bound(has_bounds ? bounds.data() : nullptr, tmax, i);
        uint32_t count = 0;
        int32_t winding = 0;
        if (cx_live(O, D, tmin, b)) {
            const CxRay r = cx_setup(O, D);
            for (uint32_t k = 0; k < n_tris; k++) {
                const float *v = tris.data() + 9 * (size_t)k;
                const int s = cx_counts(r, tmin, b, pad, { v[0], v[1], v[2] }, { v[3], v[4], v[5] }, { v[6], v[7], v[8] });
                count += s != 0 ? 1u : 0u;
                winding += s;
            }
        }
        cx_write(want_count ? o_count.data() : nullptr, want_winding ? o_winding.data() : nullptr, i, count, winding);
    }
    wr0(d + "/o_count", o_count); wr0(d + "/o_winding", o_winding);
    return 0;
}
