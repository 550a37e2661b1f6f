// scene_instances_host.cpp -- the per-thread statements of scene_instances.hip's kernels (csrc/scene_instances_kernel.h: the check and the
// binary64 inverse of an instance matrix with its verdict word, the world-space copy of an emitter) compiled for the host and run the way the
// kernels run them -- thread by thread, the fold pass by pass -- against literal restatements of what pt_scene_set_instances and the NEE
// pipeline's first render did on the host before the device call existed (scene_build.hip: ptb_set_instances' loop with invert_3x4,
// ptb_ensure_inst_lights' loop with push_emitter).  Every array is a vector of exactly its size, so an index that leaves one is the sanitizer's
// to find.  tests/test_scene_instances_device_cpu.py builds it plain and under the address and undefined-behaviour sanitizers; compile with
// -ffp-contract=off.  Exit status 0 and a line per group when everything holds.
#include "kernel_host.h"
#include "scene_device_kernel.h"  // sd_fold_pass: the cdf's left fold
#include "scene_instances_kernel.h"

#include <cstring>

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    float uni() { return (float)(next() & 0xFFFFFF) / 16777216.0f; }  // [0, 1)
};
static bool same_bytes(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

// ---- the host path restated (the parent's statements, not the shared header's) ------------------------------------------------------------------
static void ref_invert_3x4(const float m[12], float inv[12])
{
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double i00 = c00 / det, i01 = (a02 * a21 - a01 * a22) / det, i02 = (a01 * a12 - a02 * a11) / det;
    const double i10 = c01 / det, i11 = (a00 * a22 - a02 * a20) / det, i12 = (a02 * a10 - a00 * a12) / det;
    const double i20 = c02 / det, i21 = (a01 * a20 - a00 * a21) / det, i22 = (a00 * a11 - a01 * a10) / det;
    const double tx = m[3], ty = m[7], tz = m[11];
    inv[0] = (float)i00; inv[1] = (float)i01; inv[2] = (float)i02;  inv[3] = (float)(-((i00 * tx + i01 * ty) + i02 * tz));
    inv[4] = (float)i10; inv[5] = (float)i11; inv[6] = (float)i12;  inv[7] = (float)(-((i10 * tx + i11 * ty) + i12 * tz));
    inv[8] = (float)i20; inv[9] = (float)i21; inv[10] = (float)i22; inv[11] = (float)(-((i20 * tx + i21 * ty) + i22 * tz));
}
// ptb_set_instances' loop: the records it filled before it returned, and where it returned as the verdict word ((instance << 1) | kind; SI_OK: it ran through)
static uint32_t ref_set_instances(const std::vector<float> &xf, uint32_t n, std::vector<float> &rec)
{
    rec.assign(24 * (size_t)n, 0.f);
    for (uint32_t i = 0; i < n; i++) {
        const float *m = xf.data() + 12 * (size_t)i;
        for (int k = 0; k < 12; k++) {
            if (!(m[k] == m[k]) || __builtin_isinf(m[k])) return i << 1;   // "instance matrix has a NaN/Inf"
            rec[24 * (size_t)i + k] = m[k];
        }
        ref_invert_3x4(m, &rec[24 * (size_t)i + 12]);
        for (int k = 12; k < 24; k++)
            if (!(rec[24 * (size_t)i + k] == rec[24 * (size_t)i + k]) || __builtin_isinf(rec[24 * (size_t)i + k])) return (i << 1) | 1u;   // "instance matrix is singular"
    }
    return 0xFFFFFFFFu;
}
static void ref_push_emitter(const float *a, const float *b, const float *c, const float4 ke, float &run, std::vector<float4> &lights)
{
    const float e1[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, e2[3] = { c[0] - a[0], c[1] - a[1], c[2] - a[2] };
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
    run = run + 0.5f * len;
    lights.push_back(make_float4(a[0], a[1], a[2], run));
    lights.push_back(make_float4(b[0], b[1], b[2], 0.f));
    lights.push_back(make_float4(c[0], c[1], c[2], 0.f));
    lights.push_back(make_float4(-(cx / len), -(cy / len), -(cz / len), 0.f));
    lights.push_back(ke);
}
// ptb_ensure_inst_lights' loop
static float ref_inst_lights(const std::vector<float> &xf, uint32_t n, const std::vector<float4> &h_lights, uint32_t n_lights, std::vector<float4> &wl)
{
    float run = 0.f;
    wl.clear();
    for (uint32_t i = 0; i < n; i++) {
        const float *m = xf.data() + 12 * (size_t)i;
        for (uint32_t k = 0; k < n_lights; k++) {
            float w[3][3];
            for (int c = 0; c < 3; c++) {
                const float4 v = h_lights[5 * (size_t)k + c];
                for (int r = 0; r < 3; r++) w[c][r] = ((m[4 * r] * v.x + m[4 * r + 1] * v.y) + m[4 * r + 2] * v.z) + m[4 * r + 3];
            }
            ref_push_emitter(w[0], w[1], w[2], h_lights[5 * (size_t)k + 4], run, wl);
        }
    }
    return run;
}

// ---- the device path, thread by thread ---------------------------------------------------------------------------------------------------------
static const float CANARY = __builtin_bit_cast(float, 0x7FC0BEEFu);
// k_si_check_invert over its grid: blocks of TB threads, a thread past n does nothing; the word is the minimum (atomicMin from SI_OK)
static uint32_t dev_check_invert(const std::vector<float> &xf, uint32_t n, std::vector<float4> &rec, std::vector<float4> &kept)
{
    rec.assign(6 * (size_t)n, make_float4(CANARY, CANARY, CANARY, CANARY));
    kept.assign(3 * (size_t)n, make_float4(CANARY, CANARY, CANARY, CANARY));
    uint32_t verdict = SI_OK;
    const uint32_t blocks = (n + TB - 1) / TB;
    for (uint32_t t = 0; t < blocks * TB; t++) {
        if (t >= n) continue;
        const uint32_t v = si_check_invert(xf.data(), t, rec.data() + 6 * (size_t)t, kept.data() + 3 * (size_t)t);
        if (v != SI_OK) verdict = std::min(verdict, v);
    }
    return verdict;
}
// k_si_lights, then k_sd_emitter_fold's passes over the copies
static float dev_inst_lights(const std::vector<float4> &kept, uint32_t n, const std::vector<float4> &base, uint32_t n_lights, std::vector<float4> &wl)
{
    const uint32_t copies = n * n_lights;
    wl.assign(5 * (size_t)copies, make_float4(CANARY, CANARY, CANARY, CANARY));
    std::vector<float> half(copies, CANARY);
    for (uint32_t idx = 0; idx < copies; idx++) {
        const uint32_t i = idx / n_lights, k = idx - i * n_lights;
        float4 rec[5];
        half[idx] = si_light_record(kept.data() + 3 * (size_t)i, base.data() + 5 * (size_t)k, rec);
        for (int j = 0; j < 5; j++) wl[5 * (size_t)idx + j] = rec[j];
    }
    float run = 0.f;
    for (uint32_t b = 0; b < copies; b += SD_FOLD) {
        const uint32_t cnt = std::min(copies - b, SD_FOLD);
        float after = run;
        for (uint32_t lane = 0; lane < SD_FOLD; lane++) {
            float r = run;
            const auto term = [&](uint32_t k) { return half[b + k]; };
            const float mine = cnt == SD_FOLD ? sd_fold_pass<true>(r, cnt, lane, term) : sd_fold_pass<false>(r, cnt, lane, term);
            if (lane < cnt) wl[5 * (size_t)(b + lane)].w = mine;
            after = r;
        }
        run = after;
    }
    return run;
}

// ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
// n good matrices: a rotation times a non-uniform scale over 1e-3 .. 1e3, every fifth sheared, every seventh mirrored, -0.0 entries,
// translations on a grid
static std::vector<float> good_matrices(uint32_t n, uint64_t seed)
{
    Rng r = { seed };
    std::vector<float> xf(12 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        const float a = 6.2831853f * r.uni(), b = 6.2831853f * r.uni();
        const float ca = cosf(a), sa = sinf(a), cb = cosf(b), sb = sinf(b);
        float R[3][3] = { { cb, 0.f, sb }, { sa * sb, ca, -sa * cb }, { -ca * sb, sa, ca * cb } };  // Rx(a) * Ry(b)
        float s[3];
        for (int k = 0; k < 3; k++) s[k] = powf(10.f, -3.f + 6.f * r.uni());
        if (i % 7 == 3) s[1] = -s[1];                       // mirrored: a negative determinant
        float *m = xf.data() + 12 * (size_t)i;
        for (int row = 0; row < 3; row++)
            for (int col = 0; col < 3; col++) m[4 * row + col] = R[row][col] * s[col];
        if (i % 5 == 2)                                     // a shear: x += 0.5 y
            for (int row = 0; row < 3; row++) m[4 * row + 1] += 0.5f * m[4 * row + 0];
        if (i % 3 == 1) {                                   // an axis-aligned scale with -0.0 off the diagonal
            for (int k = 0; k < 12; k++) m[k] = -0.f;
            m[0] = s[0]; m[5] = s[1]; m[10] = s[2];
        }
        m[3] = -4.f + 0.5f * (float)(i % 17); m[7] = -2.f + 0.25f * (float)((i / 17) % 17); m[11] = (i % 2) ? -0.f : 0.125f * (float)(i / 289);
    }
    return xf;
}

struct Refusal { const char *name; uint32_t kind; };
static void test_check_invert()
{
    int cases = 0, refusals = 0;
    const float nan = __builtin_bit_cast(float, 0x7FC00000u), inf = INFINITY;
    for (uint32_t n : { 1u, 63u, 64u, 65u, 257u }) {
        const std::vector<float> good = good_matrices(n, 500 + n);
        // the good set passes whole; records and kept copy are the host loop's
        {
            std::vector<float> want;
            std::vector<float4> rec, kept;
            const uint32_t wv = ref_set_instances(good, n, want), gv = dev_check_invert(good, n, rec, kept);
            CHECK(wv == 0xFFFFFFFFu, "%u: the restatement refuses the good set at word %#x", n, wv);
            CHECK(gv == wv, "%u: verdict %#x", n, gv);
            CHECK(same_bytes(rec.data(), want.data(), 96 * (size_t)n), "%u: records", n);
            CHECK(same_bytes(kept.data(), good.data(), 48 * (size_t)n), "%u: the kept copy", n);
            cases++;
        }
        // every refusal: {instance, what is written there}
        const uint32_t first = 0, mid = n / 2, last = n - 1;
        for (int c = 0; c < 9; c++) {
            std::vector<float> xf = good;
            uint32_t want_word = 0;
            auto at = [&](uint32_t i) { return xf.data() + 12 * (size_t)i; };
            switch (c) {
            case 0: at(first)[5] = nan; want_word = first << 1; break;
            case 1: at(mid)[0] = nan; want_word = mid << 1; break;
            case 2: at(last)[11] = nan; want_word = last << 1; break;       // the very last value of the array
            case 3: at(mid)[3] = inf; want_word = mid << 1; break;
            case 4: at(mid)[7] = -inf; want_word = mid << 1; break;
            case 5: for (int k = 0; k < 4; k++) at(mid)[4 + k] = 0.f; want_word = (mid << 1) | 1u; break;                     // a zero row
            case 6: {                                                                                                         // two equal rows (small integers: the determinant is exactly 0)
                const float rows[12] = { 1, 2, 3, 0.5f, 4, 5, 6, -1, 1, 2, 3, 2 };
                for (int k = 0; k < 12; k++) at(last)[k] = rows[k];
                want_word = (last << 1) | 1u;
                break;
            }
            case 7: {                                                                                                         // a scale of 1e-39: 1 / s overflows binary32
                for (int k = 0; k < 12; k++) at(first)[k] = 0.f;
                at(first)[0] = at(first)[5] = at(first)[10] = 1e-39f;
                want_word = (first << 1) | 1u;
                break;
            }
            default: {                                                                                                        // a NaN at 7 and a singular matrix at 3: "singular"
                if (n < 8) continue;
                at(7)[2] = nan;
                for (int k = 0; k < 4; k++) at(3)[k] = 0.f;
                want_word = (3u << 1) | 1u;
                break;
            }
            }
            std::vector<float> want;
            std::vector<float4> rec, kept;
            const uint32_t wv = ref_set_instances(xf, n, want), gv = dev_check_invert(xf, n, rec, kept);
            CHECK(wv == want_word, "%u case %d: the restatement says %#x, the case %#x", n, c, wv, want_word);
            CHECK(gv == wv, "%u case %d: verdict %#x, want %#x", n, c, gv, wv);
            // what the host loop had filled when it returned: every instance below the failing one
            CHECK(same_bytes(rec.data(), want.data(), 96 * (size_t)(wv >> 1)), "%u case %d: records below the refusal", n, c);
            refusals++;
        }
    }
    CHECK(cases == 5 && refusals == 5 * 9 - 1, "%d good sets, %d refusals", cases, refusals);
    printf("check/invert ok (%d refusals)\n", refusals);
}

static float pairwise_sum(const float *x, size_t n) { return n == 0 ? 0.f : n == 1 ? x[0] : pairwise_sum(x, n / 2) + pairwise_sum(x + n / 2, n - n / 2); }

static void test_lights()
{
    int fold_differs = 0;
    const uint32_t shapes[][2] = { { 3, 0 }, { 1, 1 }, { 32, 2 }, { 5, 13 }, { 257, 1 } };   // instances x emitters: 0, 1, 64, 65, 257 copies
    for (const auto &sh : shapes) {
        const uint32_t n = sh[0], nl = sh[1], copies = n * nl;
        Rng r = { 900 + copies };
        // object-space emitters with edges over a decade; the matrices' scales over two more: areas over six decades
        std::vector<float4> base(5 * (size_t)nl);
        for (uint32_t k = 0; k < nl; k++) {
            const float scale = powf(10.f, -1.f * r.uni());
            float run_unused = 0.f;
            float p[3][3];
            for (int c = 0; c < 3; c++)
                for (int j = 0; j < 3; j++) p[c][j] = (2.f * r.uni() - 1.f) + scale * (2.f * r.uni() - 1.f);
            std::vector<float4> one;
            ref_push_emitter(p[0], p[1], p[2], make_float4(1.f + r.uni(), 2.f * r.uni(), 3.f, 0.f), run_unused, one);
            for (int j = 0; j < 5; j++) base[5 * (size_t)k + j] = one[j];
            base[5 * (size_t)k].w = 123.f + (float)k;   // the base table's own cdf word: never read
        }
        std::vector<float> xf = good_matrices(n, 40 + copies);
        for (uint32_t i = 0; i < n; i++) {              // scales of 1e-2 .. 1e1 per axis (good_matrices' six decades would leave binary32's range of areas)
            const float s = powf(10.f, -2.f + 3.f * r.uni());
            for (int row = 0; row < 3; row++)
                for (int col = 0; col < 3; col++) xf[12 * (size_t)i + 4 * row + col] = (row == col ? s : 0.f) + 0.1f * s * (float)((int)(i + row + col) % 3 - 1);
        }
        std::vector<float4> kept(3 * (size_t)n);
        std::memcpy(kept.data(), xf.data(), 48 * (size_t)n);
        std::vector<float4> want, got;
        const float wa = ref_inst_lights(xf, n, base, nl, want), ga = dev_inst_lights(kept, n, base, nl, got);
        CHECK(want.size() == 5 * (size_t)copies && got.size() == want.size(), "%u copies: %zu records", copies, got.size());
        CHECK(same_bytes(got.data(), want.data(), sizeof(float4) * want.size()), "%u copies: records and cdf", copies);
        CHECK(same_bytes(&ga, &wa, 4), "%u copies: light_area_inst %a, want %a", copies, ga, wa);
        if (!copies) { CHECK(__builtin_bit_cast(uint32_t, ga) == 0u, "no copies: area +0"); continue; }
        std::vector<float> half(copies);
        float lo = INFINITY, hi = 0.f;
        for (uint32_t idx = 0; idx < copies; idx++) {
            float4 rec[5];
            half[idx] = si_light_record(kept.data() + 3 * (size_t)(idx / nl), base.data() + 5 * (size_t)(idx % nl), rec);
            lo = std::min(lo, half[idx]); hi = std::max(hi, half[idx]);
        }
        if (copies >= 257) CHECK(hi / lo > 1e5f, "%u copies: areas span %g", copies, hi / lo);
        const float pw = pairwise_sum(half.data(), copies);
        if (!same_bytes(&pw, &wa, 4)) fold_differs++;
    }
    CHECK(fold_differs >= 1, "a pairwise sum equals the left fold at every count: the order would not show");
    printf("lights ok (pairwise differs at %d counts)\n", fold_differs);
}

int main()
{
    test_check_invert();
    test_lights();
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("scene_instances_host: all ok\n");
    return 0;
}
