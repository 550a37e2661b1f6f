// scene_device_host.cpp -- the per-thread statements of scene_device.hip's kernels (csrc/scene_device_kernel.h: the index check, the discovery of
// the emitters, their records and the running cdf, the fan-pair flags) compiled for the host and run the way the kernels run them -- thread by
// thread, pass by pass -- against restatements of what pt_scene_create does on the host (scene_build.hip: push_emitter and its caller's loop,
// find_fan_pairs; pt_api.hip: the index loop), written here from the caller's vertices / indices / faces.  Every array is a vector of exactly
// its size, so an index that leaves one is the sanitizer's to find.  tests/test_scene_device_cpu.py builds it plain and under the address and
// undefined-behaviour sanitizers; compile with -ffp-contract=off.  Exit status 0 and a line per group when everything holds.
#include "kernel_host.h"
#include "scene_device_kernel.h"

#include <cstring>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    float uni() { return (float)(next() & 0xFFFFFF) / 16777216.0f; }  // [0, 1)
};
struct Mesh { std::vector<float> v; std::vector<uint32_t> i; std::vector<float> f; uint32_t n_tris() const { return (uint32_t)(i.size() / 3); } };

// ---- the host path restated ------------------------------------------------------------------------------------------------------------------
struct Lights { std::vector<float4> rec; std::vector<uint32_t> prim; float area; };
static void ref_push_emitter(const float *a, const float *b, const float *c, const float *ke, float &run, std::vector<float4> &lights)
{
    const float e1[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, e2[3] = { c[0] - a[0], c[1] - a[1], c[2] - a[2] };
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
    run = run + 0.5f * len;
    lights.push_back({ a[0], a[1], a[2], run });
    lights.push_back({ b[0], b[1], b[2], 0.f });
    lights.push_back({ c[0], c[1], c[2], 0.f });
    lights.push_back({ -(cx / len), -(cy / len), -(cz / len), 0.f });
    lights.push_back({ ke[0], ke[1], ke[2], 0.f });
}
static Lights ref_lights(const Mesh &m)
{
    Lights L;
    float run = 0.f;
    for (uint32_t t = 0; t < m.n_tris(); t++) {
        const float *f = m.f.data() + 6 * (size_t)t;
        if (!(f[3] != 0.f || f[4] != 0.f || f[5] != 0.f)) continue;
        ref_push_emitter(m.v.data() + 3 * (size_t)m.i[3 * (size_t)t + 0], m.v.data() + 3 * (size_t)m.i[3 * (size_t)t + 1],
                         m.v.data() + 3 * (size_t)m.i[3 * (size_t)t + 2], f + 3, run, L.rec);
        L.prim.push_back(t);
    }
    L.area = run;
    return L;
}
static std::vector<uint8_t> ref_fan_pairs(const Mesh &m)
{
    const uint32_t n = m.n_tris();
    std::vector<uint8_t> pair(n, 0);
    auto vtx = [&](uint32_t tri, int k) { return m.v.data() + 3 * (size_t)m.i[3 * (size_t)tri + k]; };
    for (uint32_t i = 0; i + 1 < n; i++) {
        const bool same = std::memcmp(vtx(i, 0), vtx(i + 1, 0), 12) == 0 && std::memcmp(vtx(i, 2), vtx(i + 1, 1), 12) == 0;
        if (same) { pair[i] = 1; i++; }
    }
    return pair;
}
static bool ref_bad_index(const std::vector<uint32_t> &idx, uint32_t n_verts)
{
    for (uint32_t w : idx)
        if (w >= n_verts) return true;
    return false;
}

// ---- the device path, thread by thread ---------------------------------------------------------------------------------------------------------
// k_gather's rows: {v0, bits(t)} {v1, 0} {v2, 0}
static std::vector<float4> gather(const Mesh &m)
{
    std::vector<float4> tri(3 * (size_t)m.n_tris());
    for (uint32_t t = 0; t < m.n_tris(); t++)
        for (int c = 0; c < 3; c++) {
            const float *p = m.v.data() + 3 * (size_t)m.i[3 * (size_t)t + c];
            tri[3 * (size_t)t + c] = { p[0], p[1], p[2], c == 0 ? __builtin_bit_cast(float, t) : 0.f };
        }
    return tri;
}
// k_sd_check_indices: the launch's grid (at most 2048 blocks of TB threads, grid-stride), every thread's answer or-ed
static bool dev_bad_index(const std::vector<uint32_t> &idx, uint32_t n_verts)
{
    const size_t n_words = idx.size();
    const size_t blocks = std::min<size_t>((n_words + TB - 1) / TB, 2048), n_threads = blocks * TB;
    bool bad = false;
    for (size_t tid = 0; tid < n_threads; tid++) bad |= sd_any_bad_index(idx.data(), n_words, n_verts, tid, n_threads);
    return bad;
}
// k_sd_emitter_flags, the scan of the n + 1 flags, k_sd_emitter_compact, k_sd_emitter_records, k_sd_emitter_fold
static Lights dev_lights(const Mesh &m, const std::vector<float4> &tri)
{
    const uint32_t n = m.n_tris();
    std::vector<uint32_t> place((size_t)n + 1);
    for (uint32_t t = 0; t <= n; t++) place[t] = t < n && sd_is_emitter(m.f.data(), t) ? 1u : 0u;
    uint32_t sum = 0;
    for (uint32_t t = 0; t <= n; t++) { const uint32_t x = place[t]; place[t] = sum; sum += x; }
    Lights L;
    const uint32_t count = place[n];
    L.prim.assign(count, 0xEEEEEEEEu);
    for (uint32_t t = 0; t < n; t++) sd_compact(place.data(), t, L.prim.data());
    const float canary = __builtin_bit_cast(float, 0x7FC0BEEFu);
    L.rec.assign(5 * (size_t)count, { canary, canary, canary, canary });
    std::vector<float> half(count, canary);
    for (uint32_t k = 0; k < count; k++) {
        float4 rec[5];
        half[k] = sd_emitter_record(tri.data(), m.f.data(), L.prim[k], rec);
        for (int j = 0; j < 5; j++) L.rec[5 * (size_t)k + j] = rec[j];
    }
    float run = 0.f;
    for (uint32_t base = 0; base < count; base += SD_FOLD) {
        const uint32_t cnt = std::min(count - base, SD_FOLD);
        float after = run;
        for (uint32_t lane = 0; lane < SD_FOLD; lane++) {  // (every lane folds the whole pass from the run the wave entered it with)
            float r = run;
            const auto term = [&](uint32_t k) { return half[base + k]; };  // (a read past the pass's count is past the array: the sanitizer's to find)
            const float mine = cnt == SD_FOLD ? sd_fold_pass<true>(r, cnt, lane, term) : sd_fold_pass<false>(r, cnt, lane, term);
            if (lane < cnt) L.rec[5 * (size_t)(base + lane)].w = mine;
            after = r;
        }
        run = after;
    }
    L.area = run;
    return L;
}
static std::vector<uint8_t> dev_fan_pairs(const std::vector<float4> &tri, uint32_t n)
{
    std::vector<uint8_t> same(n, 0xEE), pair(n, 0xEE);
    for (uint32_t i = 0; i < n; i++) same[i] = sd_fan_with_next(tri.data(), i, n);
    sd_greedy_pairs(same.data(), n, pair.data());
    return pair;
}

// ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
// `emitters` emitters among 2 * emitters + 3 triangles with vertices of their own; edge lengths over three decades: areas over six
static Mesh emitter_mesh(uint32_t emitters, uint64_t seed)
{
    Rng r = { seed };
    const uint32_t n = 2 * emitters + 3;
    Mesh m;
    m.v.resize(9 * (size_t)n); m.i.resize(3 * (size_t)n); m.f.assign(6 * (size_t)n, 0.f);
    for (uint32_t t = 0; t < n; t++) {
        const float scale = powf(10.f, -3.f * r.uni()), c[3] = { 2.f * r.uni() - 1.f, 2.f * r.uni() - 1.f, 2.f * r.uni() - 1.f };
        for (int k = 0; k < 9; k++) m.v[9 * (size_t)t + k] = c[k % 3] + scale * (2.f * r.uni() - 1.f);
        for (int k = 0; k < 3; k++) m.i[3 * (size_t)t + k] = 3 * t + k;
        for (int k = 0; k < 3; k++) m.f[6 * (size_t)t + k] = r.uni();
        if ((t & 1u) && t / 2 < emitters)
            for (int k = 0; k < 3; k++) m.f[6 * (size_t)t + 3 + k] = 1.f + 10.f * r.uni();
    }
    return m;
}
static float pairwise_sum(const float *x, size_t n) { return n == 0 ? 0.f : n == 1 ? x[0] : pairwise_sum(x, n / 2) + pairwise_sum(x + n / 2, n - n / 2); }
static bool same_bytes(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

static void test_emitters()
{
    int fold_differs = 0;
    for (uint32_t count : { 0u, 1u, 2u, 63u, 64u, 65u, 257u, 4097u }) {
        const Mesh m = emitter_mesh(count, 1000 + count);
        const Lights want = ref_lights(m), got = dev_lights(m, gather(m));
        CHECK(want.prim.size() == count, "%u: the restatement finds %zu emitters", count, want.prim.size());
        CHECK(got.prim == want.prim, "%u: emitter ids", count);
        CHECK(got.rec.size() == want.rec.size() && same_bytes(got.rec.data(), want.rec.data(), sizeof(float4) * want.rec.size()), "%u: records", count);
        CHECK(same_bytes(&got.area, &want.area, 4), "%u: light_area %a, want %a", count, got.area, want.area);
        if (count) CHECK(same_bytes(&want.rec[5 * (size_t)(count - 1)].w, &want.area, 4), "%u: the last cdf is the area", count);
        // the order shows: a pairwise sum of the same terms is another number somewhere
        const std::vector<float4> tri = gather(m);
        std::vector<float> half(count);
        float lo = INFINITY, hi = 0.f;
        for (uint32_t k = 0; k < count; k++) {
            float4 rec[5];
            half[k] = sd_emitter_record(tri.data(), m.f.data(), want.prim[k], rec);
            lo = std::min(lo, half[k]); hi = std::max(hi, half[k]);
        }
        if (count >= 257) CHECK(hi / lo > 1e5f, "%u: areas span %g", count, hi / lo);
        const float pw = pairwise_sum(half.data(), count);
        if (!same_bytes(&pw, &want.area, 4)) fold_differs++;
    }
    CHECK(fold_differs >= 1, "a pairwise sum equals the left fold at every count: the order would not show");
    printf("emitters ok (pairwise differs at %d counts)\n", fold_differs);
}

static void test_discovery()
{
    // one Ke row per triangle: +0 | -0.0 | a denormal | a negative value | a NaN | all zero, in each of the three components where it matters
    const float nz = -0.f, den = __builtin_bit_cast(float, 1u), nan = __builtin_bit_cast(float, 0x7FC00001u);
    const float rows[][3] = { { 0.f, 0.f, 0.f }, { nz, 0.f, 0.f }, { 0.f, nz, nz }, { den, 0.f, 0.f }, { 0.f, 0.f, den }, { -2.f, 0.f, 0.f }, { 0.f, -0.5f, 0.f },
                              { nan, 0.f, 0.f }, { 0.f, 0.f, nan }, { nz, nan, nz }, { 0.f, 0.f, 0.f }, { 1.f, 2.f, 3.f } };
    const bool emits[] = { false, false, false, true, true, true, true, true, true, true, false, true };
    const uint32_t n = sizeof(rows) / sizeof(rows[0]);
    Mesh m = emitter_mesh(5, 7);  // (13 triangles of random vertices: the first n of them)
    m.v.resize(9 * (size_t)n); m.i.resize(3 * (size_t)n); m.f.assign(6 * (size_t)n, 0.25f);
    for (uint32_t t = 0; t < n; t++)
        for (int k = 0; k < 3; k++) { m.f[6 * (size_t)t + 3 + k] = rows[t][k]; m.i[3 * (size_t)t + k] = 3 * t + k; }
    std::vector<uint32_t> want;
    for (uint32_t t = 0; t < n; t++) {
        CHECK(sd_is_emitter(m.f.data(), t) == emits[t], "row %u", t);
        if (emits[t]) want.push_back(t);
    }
    const Lights ref = ref_lights(m), got = dev_lights(m, gather(m));
    CHECK(ref.prim == want && got.prim == want, "discovered ids");
    CHECK(same_bytes(got.rec.data(), ref.rec.data(), sizeof(float4) * ref.rec.size()), "records of the discovered rows (NaN payloads included)");
    // all zero: no emitter, nothing written, area +0
    std::fill(m.f.begin(), m.f.end(), 0.f);
    const Lights none = dev_lights(m, gather(m));
    CHECK(none.prim.empty() && none.rec.empty() && __builtin_bit_cast(uint32_t, none.area) == 0u, "a scene without emitters");
    printf("discovery ok\n");
}

// a quad (v0 v1 v2) (v0 v2 v3) appended with shared indices or with six vertices of its own
static void add_quad(Mesh &m, const float q[4][3], bool shared)
{
    const uint32_t base = (uint32_t)(m.v.size() / 3);
    const int corner[6] = { 0, 1, 2, 0, 2, 3 };
    if (shared) {
        for (int c = 0; c < 4; c++) m.v.insert(m.v.end(), q[c], q[c] + 3);
        for (int k = 0; k < 6; k++) m.i.push_back(base + corner[k]);
    } else {
        for (int k = 0; k < 6; k++) { m.v.insert(m.v.end(), q[corner[k]], q[corner[k]] + 3); m.i.push_back(base + k); }
    }
    m.f.insert(m.f.end(), 12, 0.5f);
}
static void add_tri(Mesh &m, const float a[3], const float b[3], const float c[3])
{
    const uint32_t base = (uint32_t)(m.v.size() / 3);
    m.v.insert(m.v.end(), a, a + 3); m.v.insert(m.v.end(), b, b + 3); m.v.insert(m.v.end(), c, c + 3);
    for (int k = 0; k < 3; k++) m.i.push_back(base + k);
    m.f.insert(m.f.end(), 6, 0.5f);
}
static void test_pairs()
{
    const float nan = __builtin_bit_cast(float, 0x7FC00123u);
    const float q0[4][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 } }, q1[4][3] = { { 2, 0, 1 }, { 3, 0, 1 }, { 3, 1, 1 }, { 2, 1, 1 } };
    const float qn[4][3] = { { nan, 0, 2 }, { 1, 0, 2 }, { 1, nan, 2 }, { 0, 1, 2 } };  // equal NaN payloads match (memcmp)
    Mesh m;
    add_quad(m, q0, true);                       // 0 1: shared indices
    add_quad(m, q1, false);                      // 2 3: duplicated coordinates
    add_quad(m, qn, false);                      // 4 5: NaNs of equal payload at the shared vertices
    {   // 6 7: -0.0 against +0.0 at the shared first vertex: equal as floats, not as bits -- no pair
        const float a[3] = { 0.f, 5, 5 }, az[3] = { -0.f, 5, 5 }, b[3] = { 1, 5, 5 }, c[3] = { 1, 6, 5 }, d[3] = { 0, 6, 5 };
        add_tri(m, a, b, c); add_tri(m, az, c, d);
    }
    {   // 8 9 10 11: a fan of four triangles around one apex, three overlapping candidate pairs: greedy takes (8 9) and (10 11), not (9 10)
        const float o[3] = { 0, 0, 9 }, p[5][3] = { { 1, 0, 9 }, { 1, 1, 9 }, { 0, 1, 9 }, { -1, 1, 9 }, { -1, 0, 9 } };
        for (int k = 0; k < 4; k++) add_tri(m, o, p[k], p[k + 1]);
    }
    {   // 12 13 14: a fan of three: (12 13) pairs, 14 stays single although (13 14) matches too
        const float o[3] = { 0, 0, 12 }, p[4][3] = { { 1, 0, 12 }, { 1, 1, 12 }, { 0, 1, 12 }, { -1, 1, 12 } };
        for (int k = 0; k < 3; k++) add_tri(m, o, p[k], p[k + 1]);
    }
    {   // 15: a lone triangle, then 16 17: a quad as the LAST two triangles (the last triangle has no successor to read)
        const float a[3] = { 7, 7, 7 }, b[3] = { 8, 7, 7 }, c[3] = { 8, 8, 7 };
        add_tri(m, a, b, c);
        add_quad(m, q1, true);
    }
    const uint8_t want[18] = { 1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 1, 0 };
    const std::vector<float4> tri = gather(m);
    const std::vector<uint8_t> ref = ref_fan_pairs(m), got = dev_fan_pairs(tri, m.n_tris());
    CHECK(m.n_tris() == 18 && ref == std::vector<uint8_t>(want, want + 18), "the restatement's pairs");
    CHECK(got == ref, "pair flags");
    CHECK(sd_fan_with_next(tri.data(), 9, 18) == 1 && got[9] == 0 && sd_fan_with_next(tri.data(), 13, 18) == 1 && got[13] == 0, "greedy takes the first of overlapping fans");
    CHECK(sd_fan_with_next(tri.data(), 17, 18) == 0, "the last triangle");
    // every prefix too: each triangle in turn is the last one
    for (uint32_t n = 1; n <= 18; n++) {
        Mesh p = m;
        p.i.resize(3 * (size_t)n); p.f.resize(6 * (size_t)n);
        std::vector<float4> t(tri.begin(), tri.begin() + 3 * (size_t)n);  // exactly n triangles: a read of triangle n is out of bounds
        CHECK(dev_fan_pairs(t, n) == ref_fan_pairs(p), "prefix %u", n);
    }
    printf("pairs ok\n");
}

static void test_index_check()
{
    int cases = 0;
    for (uint32_t n_tris : { 1u, 21u, 22u, 2049u }) {
        const uint32_t n_verts = n_tris + 2, words = 3 * n_tris;
        std::vector<uint32_t> idx(words);
        Rng r = { n_tris };
        for (uint32_t &w : idx) w = r.next() % n_verts;
        idx[words / 3] = n_verts - 1;  // (the largest index that is in range)
        CHECK(!ref_bad_index(idx, n_verts) && !dev_bad_index(idx, n_verts), "n_tris %u: none bad", n_tris);
        for (uint32_t where : { 0u, words / 2, words - 1 })
            for (uint32_t value : { n_verts, 0xFFFFFFFFu }) {
                std::vector<uint32_t> bad = idx;
                bad[where] = value;
                CHECK(ref_bad_index(bad, n_verts) && dev_bad_index(bad, n_verts), "n_tris %u: %#x at word %u", n_tris, value, where);
                cases++;
            }
    }
    CHECK(cases == 24, "%d cases", cases);
    printf("index check ok\n");
}

int main()
{
    test_emitters();
    test_discovery();
    test_pairs();
    test_index_check();
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("scene_device_host: all ok\n");
    return 0;
}
