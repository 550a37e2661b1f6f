// reproject_host.cpp -- k_reproject's per-pixel body (csrc/reproject_kernel.h), compiled for the host and run over planes read from files:
// what tests/test_reproject.py holds against its numpy restatement without a GPU, and under the host's sanitizers.  The stand-ins (kernel_host.h) are
// the IEEE operations pt_math.h's helpers are proven equal to (quot_rn, div3_dominant: the correctly rounded quotient; fsqrt: the correctly
// rounded root); compile with -ffp-contract=off.  usage: reproject_host DIR  (DIR/par, c_*, p_* in, o_* out; see _run_on_host in the test)
#include "kernel_host.h"
#define RP_KEEP(v) ((void)(v))
#include "reproject_kernel.h"
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: reproject_host DIR\n"); return 2; }
    const std::string d = argv[1];
    auto par = rd<float>(d + "/par", 24);  // w h has_prev match_id cam(6) prev(6) gain alpha depth_tol normal_min max_history has_m
    const uint32_t w = (uint32_t)par[0], h = (uint32_t)par[1]; const size_t n = (size_t)w * h;
    auto C = rd<float>(d + "/c_C", 3 * n), M = rd<float>(d + "/c_M", 3 * n), N = rd<float>(d + "/c_N", 3 * n), Z = rd<float>(d + "/c_Z", n), A = rd<float>(d + "/c_a", n);
    auto ID = rd<uint2>(d + "/c_ID", n);
    std::vector<float> L(n, 7.f); std::vector<uchar4> bg(n);
    auto pC = rd<float>(d + "/p_C", 3 * n), pM = rd<float>(d + "/p_M", 3 * n), pN = rd<float>(d + "/p_N", 3 * n), pZ = rd<float>(d + "/p_Z", n), pA = rd<float>(d + "/p_a", n), pL = rd<float>(d + "/p_L", n);
    auto pID = rd<uint2>(d + "/p_ID", n);
    RpConst rc{};
    rc.w = w; rc.h = h; fp_grid(w, h, &rc.n_bx); rc.match_id = (uint32_t)par[3];
    rc.cam = { par[4], par[5], par[6], par[7], par[8], par[9], (float)w, (float)h, 0.f, 0.f };
    rc.pox = par[10]; rc.poy = par[11]; rc.poz = par[12]; rc.ptx = par[13]; rc.pty = par[14]; rc.ptz = par[15];
    rc.gain = par[16]; rc.alpha = par[17]; rc.depth_tol = par[18]; rc.normal_min = par[19]; rc.max_history = par[20];
    RpFilm fl = { C.data(), M.data(), L.data(), bg.data(), N.data(), Z.data(), A.data(), ID.data() };
    RpPrev pv{};
    if (par[2] != 0.f) pv = { pC.data(), pM.data(), pL.data(), pN.data(), pZ.data(), pA.data(), pID.data() };
    for (int y = 0; y < (int)h; y++)
        for (int x = 0; x < (int)w; x++) {
            if (par[21] != 0.f) rp_pixel<true>(rc, fl, pv, x, y);
            else rp_pixel<false>(rc, fl, pv, x, y);
        }
    wr(d + "/o_C", C); wr(d + "/o_M", M); wr(d + "/o_L", L); wr(d + "/o_bgra", bg);
    return 0;
}
