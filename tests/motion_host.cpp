// motion_host.cpp -- k_motion's per-pixel body (csrc/motion_kernel.h) and the MOTION instantiation of k_reproject's (csrc/reproject_kernel.h),
// compiled for the host and run over planes read from files: what tests/test_motion.py holds against its numpy restatements without a GPU, and
// under the host's sanitizers.  The stand-ins (kernel_host.h) are the IEEE operations pt_math.h's helpers are proven equal to; compile with
// -ffp-contract=off.  usage: motion_host DIR.  DIR/mpar present: Q from DIR/m_* (-> o_Q); DIR/par present: the reprojection of
// reproject_host.cpp's files plus DIR/c_Q (-> o_C, o_M, o_L, o_bgra).  Every array is read into a vector of exactly its size, so an index
// that leaves its array is the sanitizer's to find.
#include "kernel_host.h"
#define RP_KEEP(v) ((void)(v))
#define MO_KEEP(v) ((void)(v))
#include "reproject_kernel.h"
#include "motion_kernel.h"
static bool have(const std::string &p) { FILE *f = fopen(p.c_str(), "rb"); if (f) fclose(f); return f != nullptr; }

static void motion(const std::string &d)
{
    auto par = rd<float>(d + "/mpar", 16);  // w h n_tris n_inst cam(6) slack
    const uint32_t w = (uint32_t)par[0], h = (uint32_t)par[1], n_tris = (uint32_t)par[2], n_inst = (uint32_t)par[3]; const size_t n = (size_t)w * h;
    auto Z = rd<float>(d + "/m_Z", n), A = rd<float>(d + "/m_a", n);
    auto ID = rd<uint2>(d + "/m_ID", n);
    auto tri = rd<float4>(d + "/m_tri", 3 * (size_t)n_tris), tri_prev = rd<float4>(d + "/m_tri_prev", 3 * (size_t)n_tris);
    std::vector<float4> xf, xf_prev;
    if (n_inst) { xf = rd<float4>(d + "/m_xf", 3 * (size_t)n_inst); xf_prev = rd<float4>(d + "/m_xf_prev", 3 * (size_t)n_inst); }
    std::vector<float4> Q(n, make_float4(9.f, 9.f, 9.f, 9.f));
    MoConst mc{};
    mc.w = w; mc.h = h; fp_grid(w, h, &mc.n_bx); mc.n_tris = n_tris; mc.n_inst = n_inst ? n_inst : 1u;
    mc.cam = { par[4], par[5], par[6], par[7], par[8], par[9], (float)w, (float)h, 0.f, 0.f };
    mc.slack = par[10];
    const MoScene sc = { tri.data(), tri_prev.data(), n_inst ? xf.data() : nullptr, n_inst ? xf_prev.data() : nullptr };
    const MoFilm fl = { Z.data(), A.data(), ID.data(), Q.data() };
    for (int y = 0; y < (int)h; y++)
        for (int x = 0; x < (int)w; x++) {
            if (n_inst) mo_pixel<true>(mc, sc, fl, x, y);
            else mo_pixel<false>(mc, sc, fl, x, y);
        }
    wr(d + "/o_Q", Q);
}

static void reproject(const std::string &d)
{
    auto par = rd<float>(d + "/par", 24);  // w h has_prev match_id cam(6) prev(6) gain alpha depth_tol normal_min max_history has_m
    const uint32_t w = (uint32_t)par[0], h = (uint32_t)par[1]; const size_t n = (size_t)w * h;
    auto C = rd<float>(d + "/c_C", 3 * n), M = rd<float>(d + "/c_M", 3 * n), N = rd<float>(d + "/c_N", 3 * n), Z = rd<float>(d + "/c_Z", n), A = rd<float>(d + "/c_a", n);
    auto ID = rd<uint2>(d + "/c_ID", n);
    auto Q = rd<float4>(d + "/c_Q", n);
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
    const float *q = &Q.data()->x;
    for (int y = 0; y < (int)h; y++)
        for (int x = 0; x < (int)w; x++) {
            if (par[21] != 0.f) rp_pixel<true, true>(rc, fl, pv, x, y, q);
            else rp_pixel<false, true>(rc, fl, pv, x, y, q);
        }
    wr(d + "/o_C", C); wr(d + "/o_M", M); wr(d + "/o_L", L); wr(d + "/o_bgra", bg);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: motion_host DIR\n"); return 2; }
    const std::string d = argv[1];
    if (!have(d + "/mpar") && !have(d + "/par")) { fprintf(stderr, "neither %s/mpar nor %s/par\n", d.c_str(), d.c_str()); return 2; }
    if (have(d + "/mpar")) motion(d);
    if (have(d + "/par")) reproject(d);
    return 0;
}
