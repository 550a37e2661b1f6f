// nearest_host.cpp -- the per-lane statements that define pt_nearest_device's result (csrc/nearest_kernel.h: closest point of a triangle, box
// distance, accept rule, row -> point, radius rule, the two writers) compiled for the host and run over arrays read from files: what
// tests/test_nearest_cpu.py holds against the numpy restatement of tests/nearest_cases.py without a GPU, and under the host's sanitizers.  The
// tree walk stays on the device; here the accept rule runs over ALL triangles of a scene, which is what the walk has to equal.  Every array is a
// vector of exactly its size, so an index that leaves a table or an output is the sanitizer's to find; the points are read at an offset of one
// float from their allocation, so rows are only 4-byte aligned.  The IEEE divide (kernel_host.h) stands in for pt_math.h's fdiv, its bitwise
// equal; compile with -ffp-contract=off.
// usage: nearest_host DIR   (DIR/par: n_pairs n_boxes n_points n_tris has_radii want_nearest want_point bits(max_dist))
//   pairs   n_pairs x {P, A, B, C} (12 floats)  -> o_pairs  n_pairs x {u, v, Q.xyz, dist2}, o_region n_pairs x int32
//   boxes   n_pairs x n_boxes x {lo, hi}        -> o_boxes  n_pairs x n_boxes box distances of the pair's P
//   points  one float of padding, n_points x 3; radii n_points (has_radii); tris n_tris x {A, B, C} (9 floats), primitive id = position
//           -> o_points (the rows as read), o_r2 (the radius rule), o_nearest n_points x pt_nearest, o_point n_points x 3 (the loop over all
//           triangles by nr_accept, written by the two writers over canaries; an output not wanted does not exist)
#include "kernel_host.h"
#include "nearest_kernel.h"
template <class T> void wr0(const std::string &p, const std::vector<T> &v) { if (v.empty()) { FILE *f = fopen(p.c_str(), "wb"); if (!f || fclose(f) != 0) exit(2); } else wr(p, v); }
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: nearest_host DIR\n"); return 2; }
    const std::string d = argv[1];
    auto par = rd<uint32_t>(d + "/par", 8);
    const size_t n_pairs = par[0], n_boxes = par[1], n_points = par[2], n_tris = par[3];
    const bool has_radii = par[4] != 0, want_nearest = par[5] != 0, want_point = par[6] != 0;
    const float max_dist = __builtin_bit_cast(float, par[7]);
    // ---- pairs and their boxes
    auto pairs = rd<float>(d + "/pairs", 12 * n_pairs);
    auto boxes = rd<float>(d + "/boxes", 6 * n_pairs * n_boxes);
    std::vector<float> o_pairs(6 * n_pairs), o_boxes(n_pairs * n_boxes);
    std::vector<int32_t> o_region(n_pairs);
    for (size_t i = 0; i < n_pairs; i++) {
        const float *p = pairs.data() + 12 * i;
        const NrVec P = { p[0], p[1], p[2] };
        const NrClosest r = nr_closest(P, { p[3], p[4], p[5] }, { p[6], p[7], p[8] }, { p[9], p[10], p[11] });
        const float o[6] = { r.u, r.v, r.q.x, r.q.y, r.q.z, r.dist2 };
        std::copy(o, o + 6, o_pairs.begin() + 6 * i);
        o_region[i] = r.region;
        for (size_t k = 0; k < n_boxes; k++) {
            const float *b = boxes.data() + 6 * (i * n_boxes + k);
            o_boxes[i * n_boxes + k] = nr_box_dist2(P, { b[0], b[1], b[2] }, { b[3], b[4], b[5] });
        }
    }
    wr0(d + "/o_pairs", o_pairs); wr0(d + "/o_region", o_region); wr0(d + "/o_boxes", o_boxes);
    // ---- a scene: rows, radii, the loop over all triangles, the writers
    auto points_alloc = rd<float>(d + "/points", 1 + 3 * n_points);
    const float *points = points_alloc.data() + 1;
    auto radii = rd<float>(d + "/radii", has_radii ? n_points : 0);
    auto tris = rd<float>(d + "/tris", 9 * n_tris);
    const float canary = __builtin_bit_cast(float, 0x7FC0BEEFu);
    std::vector<float> o_points(3 * n_points, canary), o_r2(n_points, canary), o_point(want_point ? 3 * n_points : 0, canary);
    std::vector<uint32_t> o_nearest(want_nearest ? 4 * n_points : 0, 0xEEEEEEEEu);
    for (uint32_t i = 0; i < n_points; i++) {  // (the kernel's refill and finish, lane by lane)
        const NrVec P = nr_point(points, i);
        const float row[3] = { P.x, P.y, P.z };
        std::copy(row, row + 3, o_points.begin() + 3 * (size_t)i);
        float best_d = nr_radius2(nr_radius(has_radii ? radii.data() : nullptr, max_dist, i)), best_u = 0.f, best_v = 0.f;
        o_r2[i] = best_d;
        uint32_t best_prim = NR_MISS;
        NrVec best_q = { 0.f, 0.f, 0.f };
        for (uint32_t t = 0; t < n_tris; t++) {
            const float *v = tris.data() + 9 * (size_t)t;
            const NrClosest r = nr_closest(P, { v[0], v[1], v[2] }, { v[3], v[4], v[5] }, { v[6], v[7], v[8] });
            if (nr_accept(r.dist2, t, best_d, best_prim)) { best_d = r.dist2; best_prim = t; best_u = r.u; best_v = r.v; best_q = r.q; }
        }
        if (want_nearest) nr_write_nearest(o_nearest.data(), i, best_prim, best_d, best_u, best_v);
        if (want_point) nr_write_point(o_point.data(), i, best_prim, best_q);
    }
    wr0(d + "/o_points", o_points); wr0(d + "/o_r2", o_r2); wr0(d + "/o_nearest", o_nearest); wr0(d + "/o_point", o_point);
    return 0;
}
