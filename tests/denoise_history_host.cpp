// denoise_history_host.cpp -- the per-pixel bodies of k_dn_prepare_hist and k_dn_var_spatial (csrc/denoise_history_kernel.h), compiled for the
// host and run over planes read from files: what tests/test_denoise_history.py holds against its numpy restatement without a GPU, and under
// the host's sanitizers.  The IEEE divide (kernel_host.h) stands in for pt_math.h's fdiv, its bitwise equal; compile with -ffp-contract=off.
// usage: denoise_history_host DIR  (DIR/par, film, albedo, normal, emission, depth, alpha, m2, len in; o_illum, o_guide out: the records the
// pre-blur reads, {I.rgb, V0} and {N.xyz, Z} per pixel; see _run_on_host in the test)
#include "kernel_host.h"
#define DH_KEEP(v) ((void)(v))
#include "denoise_history_kernel.h"
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: denoise_history_host DIR\n"); return 2; }
    const std::string d = argv[1];
    auto par = rd<float>(d + "/par", 8);  // w h sigma_normal sigma_depth min_history step_frames n_max -
    const uint32_t w = (uint32_t)par[0], h = (uint32_t)par[1]; const size_t n = (size_t)w * h;
    auto film = rd<float>(d + "/film", 3 * n), albedo = rd<float>(d + "/albedo", 3 * n), normal = rd<float>(d + "/normal", 3 * n), emission = rd<float>(d + "/emission", 3 * n);
    auto depth = rd<float>(d + "/depth", n), alpha = rd<float>(d + "/alpha", n), m2 = rd<float>(d + "/m2", 3 * n), len = rd<float>(d + "/len", n);
    DhConst dc{};
    dc.w = w; dc.h = h; fp_grid(w, h, &dc.n_bx);
    dc.inv_n = 1.0f / (par[2] * par[2]); dc.sz2 = par[3] * par[3];   // (as dn_run computes them)
    dc.mh = par[4]; dc.sf = par[5]; dc.n_max = par[6];
    const DhPlanes pl = { film.data(), albedo.data(), normal.data(), emission.data(), depth.data(), alpha.data(), m2.data(), len.data() };
    std::vector<float4> illum0(n), illum1(n), guide(n);
    for (size_t p = 0; p < n; p++) dh_prepare_pixel(dc, pl, p, illum0.data(), guide.data());
    // (the kernel's wave-wide vote only skips work whose result is the copy: every pixel goes through the body here)
    for (int y = 0; y < (int)h; y++)
        for (int x = 0; x < (int)w; x++) {
            const size_t p = (size_t)y * w + (uint32_t)x;
            illum1[p] = dh_spatial_pixel(dc, guide.data(), illum0.data(), x, y, len[p], illum0[p]);
        }
    wr(d + "/o_illum", illum1); wr(d + "/o_guide", guide);
    return 0;
}
