// scene_faces_host.cpp -- the per-thread statements of scene_faces.hip's kernel (csrc/scene_faces_kernel.h: the material words of the
// per-triangle tables from six floats, the emitter predicate) compiled for the host and run the way k_set_faces<HAS8> runs them -- one call per
// table position, under shuffled leaf orders -- against an independent restatement of k_pack's lines (scene_build.hip), written here from the
// faces.  The tables are pre-filled with a canary pattern: every word the call must not write -- the normal words, shade4[3p+2].yzw, the
// vertex / normal rows of shade64, everything past the arrays -- still holds it afterwards.  Once on vectors of exactly their size (an index
// that leaves one is the sanitizer's to find), once on arrays with a guarded tail (the plain build's check).  tests/test_scene_faces_cpu.py
// builds it plain and under the address and undefined-behaviour sanitizers; compile with -ffp-contract=off.  Exit status 0 and a line per group.
#include "kernel_host.h"
#define __host__
#include "scene_device_kernel.h"
#include "scene_faces_kernel.h"

#include <cstring>
#include <limits>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    float uni() { return (float)(next() & 0xFFFFFF) / 16777216.0f; }  // [0, 1)
};

static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static float canary(uint32_t table, size_t word) { const uint32_t u = 0xCA000000u | (table << 20) | (uint32_t)(word & 0xFFFFFu); float f; std::memcpy(&f, &u, 4); return f; }
static void fill(std::vector<float4> &t, uint32_t table)
{
    float *w = reinterpret_cast<float *>(t.data());
    for (size_t k = 0; k < 4 * t.size(); k++) w[k] = canary(table, k);
}
static bool is_canary(const std::vector<float4> &t, uint32_t table, size_t word)
{
    return bits(reinterpret_cast<const float *>(t.data())[word]) == bits(canary(table, word));
}

static std::vector<uint32_t> shuffled(uint32_t n, Rng &r)
{
    std::vector<uint32_t> p(n);
    for (uint32_t k = 0; k < n; k++) p[k] = k;
    for (uint32_t k = n; k > 1; k--) std::swap(p[k - 1], p[r.next() % k]);
    return p;
}

// the eight edge values of tests/test_material_edges.py's kind: 0, -0.0, a denormal, 1e-38, a negative, 3e38, +inf, NaN
static const float EDGE[8] = { 0.f, -0.f, 1.4e-45f, 1e-38f, -0.75f, 3e38f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN() };

// rows 0..7 (rotated by `shift`): the edge value in all of Kd; rows 8..15: in ONE component of Ke, the others +0 (so the predicate is the edge's)
static std::vector<float> make_faces(uint32_t n, uint32_t shift, Rng &r)
{
    std::vector<float> f(6 * (size_t)n);
    for (uint32_t t = 0; t < n; t++) {
        float *row = f.data() + 6 * (size_t)t;
        for (int k = 0; k < 3; k++) row[k] = r.uni();
        const bool emits = r.uni() < 0.25f;
        for (int k = 3; k < 6; k++) row[k] = emits ? 8.f * r.uni() : 0.f;
        const uint32_t kind = (t + shift) % 16u;
        if (t >= 16u) continue;
        if (kind < 8u) for (int k = 0; k < 3; k++) row[k] = EDGE[kind];
        else { for (int k = 3; k < 6; k++) row[k] = 0.f; row[3 + kind % 3u] = EDGE[kind - 8u]; }
    }
    return f;
}

// ---- k_pack's lines restated (scene_build.hip): brdf = Kd / pi by a true divide, the emission, the flag ---------------------------------
struct Words { float br, bg, bb, ke[3], flag; };
static Words ref_words(const float *f)
{
    Words w;
    w.br = f[0] / 3.1415927410125732f;
    w.bg = f[1] / 3.1415927410125732f;
    w.bb = f[2] / 3.1415927410125732f;
    w.ke[0] = f[3]; w.ke[1] = f[4]; w.ke[2] = f[5];
    const bool emits = !(f[3] == 0.f && f[4] == 0.f && f[5] == 0.f);
    w.flag = emits ? 1.f : 0.f;
    return w;
}

static void check_tables(uint32_t n, uint32_t guard, const std::vector<float> &faces, const std::vector<uint32_t> &order, const std::vector<float4> *shade4,
                         const std::vector<float4> &shade64, const std::vector<float4> &ke4, uint32_t id4, uint32_t id64, uint32_t idke)
{
    for (uint32_t p = 0; p < n; p++) {
        const Words w = ref_words(faces.data() + 6 * (size_t)order[p]);
        if (shade4) {
            const float *s = reinterpret_cast<const float *>(shade4->data() + 3 * (size_t)p);
            CHECK(bits(s[3]) == bits(w.br) && bits(s[4]) == bits(w.bg) && bits(s[5]) == bits(w.bb), "shade4 Kd/pi n %u pos %u", n, p);
            CHECK(bits(s[6]) == bits(w.ke[0]) && bits(s[7]) == bits(w.ke[1]) && bits(s[8]) == bits(w.ke[2]), "shade4 Ke n %u pos %u", n, p);
            for (size_t k : { 0, 1, 2, 9, 10, 11 }) CHECK(is_canary(*shade4, id4, 12 * (size_t)p + k), "shade4 word %zu of pos %u written (n %u)", k, p, n);
        }
        const float *r = reinterpret_cast<const float *>(shade64.data() + 4 * (size_t)p);
        CHECK(bits(r[12]) == bits(w.br) && bits(r[13]) == bits(w.bg) && bits(r[14]) == bits(w.bb) && bits(r[15]) == bits(w.flag), "shade64 n %u pos %u", n, p);
        for (size_t k = 0; k < 12; k++) CHECK(is_canary(shade64, id64, 16 * (size_t)p + k), "shade64 word %zu of pos %u written (n %u)", k, p, n);
        const float4 e = ke4[p];
        CHECK(bits(e.x) == bits(w.ke[0]) && bits(e.y) == bits(w.ke[1]) && bits(e.z) == bits(w.ke[2]) && bits(e.w) == 0u, "ke4 n %u pos %u", n, p);
    }
    // everything past the arrays
    if (shade4) for (size_t k = 12 * (size_t)n; k < 4 * shade4->size(); k++) CHECK(is_canary(*shade4, id4, k), "shade4 tail word %zu (n %u)", k, n);
    for (size_t k = 16 * (size_t)n; k < 4 * shade64.size(); k++) CHECK(is_canary(shade64, id64, k), "shade64 tail word %zu (n %u)", k, n);
    for (size_t k = 4 * (size_t)n; k < 4 * ke4.size(); k++) CHECK(is_canary(ke4, idke, k), "ke4 tail word %zu (n %u)", k, n);
    (void)guard;
}

template <bool HAS8>
static void run(uint32_t n, uint32_t shift, uint32_t guard, Rng &r)
{
    const std::vector<float> faces = make_faces(n, shift, r);
    const std::vector<uint32_t> order = shuffled(n, r), order8 = shuffled(n, r);
    std::vector<float4> shade4(3 * (size_t)n + guard), shade64(4 * (size_t)n + guard), ke4((size_t)n + guard), shade64_8(4 * (size_t)n + guard), ke4_8((size_t)n + guard);
    fill(shade4, 1); fill(shade64, 2); fill(ke4, 3); fill(shade64_8, 4); fill(ke4_8, 5);
    for (uint32_t pos = 0; pos < n; pos++)  // one call per thread of k_set_faces<HAS8>
        sf_set_position<HAS8>(faces.data(), order.data(), HAS8 ? order8.data() : nullptr, pos, shade4.data(), shade64.data(), ke4.data(),
                              HAS8 ? shade64_8.data() : nullptr, HAS8 ? ke4_8.data() : nullptr);
    check_tables(n, guard, faces, order, &shade4, shade64, ke4, 1, 2, 3);
    if (HAS8) check_tables(n, guard, faces, order8, nullptr, shade64_8, ke4_8, 0, 4, 5);
    else {
        for (size_t k = 0; k < 4 * shade64_8.size(); k++) CHECK(is_canary(shade64_8, 4, k), "shade64_8 word %zu written without HAS8", k);
        for (size_t k = 0; k < 4 * ke4_8.size(); k++) CHECK(is_canary(ke4_8, 5, k), "ke4_8 word %zu written without HAS8", k);
    }
    // the predicate: sf_emits, shade64's flag and sd_is_emitter (what the emitter kernels decide by) agree on every row
    for (uint32_t t = 0; t < n; t++) {
        const bool want = sd_is_emitter(faces.data(), t);
        CHECK(sf_emits(sf_load(faces.data(), t)) == want, "predicate n %u row %u", n, t);
        CHECK(ref_words(faces.data() + 6 * (size_t)t).flag == (want ? 1.f : 0.f), "restated flag n %u row %u", n, t);
    }
}

int main()
{
    Rng r{ 0x5CE9Eull };
    // the edge rows mean what tests/test_material_edges.py says: -0.0 and +0 emit nothing; a denormal, a negative, inf and NaN do
    {
        const bool emits[8] = { false, false, true, true, true, true, true, true };
        for (int k = 0; k < 8; k++) {
            const float row[6] = { 0.5f, 0.5f, 0.5f, 0.f, EDGE[k], 0.f };
            CHECK(sf_emits(sf_load(row, 0)) == emits[k] && sd_is_emitter(row, 0) == emits[k], "edge %d", k);
        }
        puts("predicate ok: 8 edge values");
    }
    const uint32_t sizes[5] = { 1, 63, 64, 65, 257 };
    uint32_t runs = 0;
    for (uint32_t guard : { 0u, 5u })
        for (uint32_t n : sizes)
            for (uint32_t shift = 0; shift < 16; shift++) {
                run<false>(n, shift, guard, r);
                run<true>(n, shift, guard, r);
                runs += 2;
            }
    if (!g_fail) printf("material words ok: %u runs over n = 1, 63, 64, 65, 257, exact and guarded arrays, with and without the 8-wide tables\n", runs);
    if (!g_fail) puts("canaries ok: normal words, shade4[3p+2].yzw, shade64 rows 0..2 and the tails untouched");
    if (g_fail) { fprintf(stderr, "scene_faces_host: %d failures\n", g_fail); return 1; }
    puts("scene_faces_host: all ok");
    return 0;
}
