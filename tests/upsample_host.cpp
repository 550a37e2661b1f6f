// upsample_host.cpp -- the per-pixel body of k_upsample (csrc/upsample_kernel.h), compiled for the host and run over planes read from files:
// what tests/test_upsample.py holds against its numpy restatement without a GPU, and under the host's sanitizers.  The IEEE divide
// (kernel_host.h) stands in for pt_math.h's fdiv, its bitwise equal; compile with -ffp-contract=off.  lo's records are made here by
// k_dn_prepare's two statements (dn_demod and the divide), which the kernel header shares with the denoisers.
// usage: upsample_host DIR  (DIR/par; albedo, normal, emission, depth, alpha: the full-size guides; lo_src, lo_albedo, lo_normal, lo_emission,
// lo_depth, lo_alpha: lo's source plane and guides in; o_rgb, o_bgra out; see _run_on_host in the test)
#include "kernel_host.h"
#define DH_KEEP(v) ((void)(v))
#define UP_KEEP(v) ((void)(v))
#define UP_ANY(b) ((void)(b), true)   // every pixel walks the second ring: a lane that did not fall back keeps its first-ring result by the select
#include "upsample_kernel.h"
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: upsample_host DIR\n"); return 2; }
    const std::string d = argv[1];
    auto par = rd<float>(d + "/par", 8);  // w h lw lh sigma_normal sigma_depth - -
    const uint32_t w = (uint32_t)par[0], h = (uint32_t)par[1], lw = (uint32_t)par[2], lh = (uint32_t)par[3];
    const size_t n = (size_t)w * h, ln = (size_t)lw * lh;
    auto albedo = rd<float>(d + "/albedo", 3 * n), normal = rd<float>(d + "/normal", 3 * n), emission = rd<float>(d + "/emission", 3 * n);
    auto depth = rd<float>(d + "/depth", n), alpha = rd<float>(d + "/alpha", n);
    auto ls = rd<float>(d + "/lo_src", 3 * ln), la = rd<float>(d + "/lo_albedo", 3 * ln), lnr = rd<float>(d + "/lo_normal", 3 * ln), le = rd<float>(d + "/lo_emission", 3 * ln);
    auto lz = rd<float>(d + "/lo_depth", ln), lal = rd<float>(d + "/lo_alpha", ln);
    std::vector<float4> illum(ln), guide(ln);
    for (size_t q = 0; q < ln; q++) {  // (k_dn_prepare)
        float i3[3];
        for (int c = 0; c < 3; c++) i3[c] = ptm::fdiv(ls[3 * q + c] - le[3 * q + c], dn_demod(la[3 * q + c], lal[q]));
        illum[q] = make_float4(i3[0], i3[1], i3[2], 0.f);
        guide[q] = make_float4(lnr[3 * q + 0], lnr[3 * q + 1], lnr[3 * q + 2], lz[q]);
    }
    UpConst uc{};
    uc.w = w; uc.h = h; fp_grid(w, h, &uc.n_bx);
    uc.lw = lw; uc.lh = lh;
    uc.sx = (float)lw / (float)w; uc.sy = (float)lh / (float)h;            // (as ptu_upsample computes them)
    uc.inv_n = 1.0f / (par[4] * par[4]); uc.sz2 = par[5] * par[5];
    const UpGuides gd = { albedo.data(), normal.data(), emission.data(), depth.data(), alpha.data() };
    const UpLo lo = { guide.data(), illum.data() };
    std::vector<float> rgb(3 * n);
    std::vector<uchar4> bgra(n);
    const UpOut out = { rgb.data(), bgra.data() };
    for (int y = 0; y < (int)h; y++)
        for (int x = 0; x < (int)w; x++) up_pixel(uc, gd, lo, out, x, y);
    wr(d + "/o_rgb", rgb); wr(d + "/o_bgra", bgra);
    return 0;
}
