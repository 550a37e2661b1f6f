// adaptive_host.cpp -- the per-lane bodies of k_adapt_select and k_resolve_adapt (csrc/adaptive_kernel.h), compiled for the host and run over
// planes read from files: what tests/test_adaptive.py holds against its numpy restatement without a GPU, and under the host's sanitizers.
// The IEEE divide and root (kernel_host.h) stand in for pt_math.h's fdiv and fsqrt, their bitwise equals; compile with -ffp-contract=off.
// The selection runs the body over the 64 lanes of each tile of the world-1 list, row by row, with the butterfly as a loop and the votes as
// loops; the blend runs ad_blend over every valid pixel of the selected tiles, frame after frame.
// usage: adaptive_host DIR  (DIR/par: w h threshold rel_floor min_frames max_frames n_frames -; C, M, K, bgra in; col: n_frames frame colours
// [h][w][3]; o_sel (a byte per tile), o_et (e_T per tile), o_C, o_M, o_K, o_bgra out; see _run_on_host in the test)
#include "kernel_host.h"
#include <cstring>
#include "adaptive_kernel.h"
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: adaptive_host DIR\n"); return 2; }
    const std::string d = argv[1];
    auto par = rd<float>(d + "/par", 8);
    AdConst ac{};
    ac.w = (uint32_t)par[0]; ac.h = (uint32_t)par[1];
    ac.threshold = par[2]; ac.rel_floor = par[3];
    ac.min_frames = par[4]; ac.max_frames = par[5];   // ((float) of the integers, as ptad_select makes them)
    ac.has_max = par[5] > 0.f ? 1u : 0u;
    const uint32_t n_frames = (uint32_t)par[6];
    const size_t n = (size_t)ac.w * ac.h;
    auto C = rd<float>(d + "/C", 3 * n), M = rd<float>(d + "/M", 3 * n), K = rd<float>(d + "/K", n);
    auto bgra = rd<uchar4>(d + "/bgra", n);
    auto col = rd<float>(d + "/col", 3 * n * n_frames);
    const uint32_t tiles_x = (ac.w + 7) / 8, tiles_y = (ac.h + 7) / 8;
    std::vector<uint8_t> sel((size_t)tiles_x * tiles_y);
    std::vector<float> et((size_t)tiles_x * tiles_y);
    for (uint32_t ty = 0; ty < tiles_y; ty++)
        for (uint32_t tx = 0; tx < tiles_x; tx++) {
            float x[64];
            uint32_t n_valid = 0;
            bool short_ = false, below_max = false;
            for (uint32_t lane = 0; lane < 64; lane++) {   // (k_adapt_select, lane by lane)
                const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
                const bool valid = px < ac.w && py < ac.h;
                const size_t pix = (size_t)min(py, ac.h - 1u) * ac.w + min(px, ac.w - 1u);
                const float c[3] = { C[3 * pix + 0], C[3 * pix + 1], C[3 * pix + 2] };
                const float m[3] = { M[3 * pix + 0], M[3 * pix + 1], M[3 * pix + 2] };
                const float k = K[pix];
                x[lane] = ad_lane_error(valid, c, m, k, ac.rel_floor);
                n_valid += valid ? 1u : 0u;
                short_ |= ad_lane_short(valid, k, ac.min_frames);
                below_max |= ad_lane_below_max(valid, k, ac.max_frames);
            }
            for (int s = 1; s < 64; s <<= 1) {             // the xor butterfly
                float y[64];
                for (int lane = 0; lane < 64; lane++) y[lane] = x[lane] + x[lane ^ s];
                for (int lane = 0; lane < 64; lane++) x[lane] = y[lane];
            }
            for (int lane = 1; lane < 64; lane++)
                if (std::memcmp(&x[lane], &x[0], sizeof(float)) != 0) { fprintf(stderr, "lanes differ after the butterfly\n"); return 3; }
            const float e_t = ptm::fdiv(x[0], (float)n_valid);
            const bool capped = ac.has_max != 0u && !below_max;
            sel[(size_t)ty * tiles_x + tx] = ad_selected(short_, capped, e_t, ac.threshold) ? 1 : 0;
            et[(size_t)ty * tiles_x + tx] = e_t;
        }
    for (uint32_t py = 0; py < ac.h; py++)
        for (uint32_t px = 0; px < ac.w; px++) {           // (k_resolve_adapt's blend, pixel by pixel)
            if (!sel[(size_t)(py / 8) * tiles_x + px / 8]) continue;
            const size_t pix = (size_t)py * ac.w + px;
            AdPixel p;
            for (int k = 0; k < 3; k++) { p.c[k] = C[3 * pix + k]; p.m[k] = M[3 * pix + k]; }
            p.img = bgra[pix];
            p.n = K[pix];
            for (uint32_t f = 0; f < n_frames; f++) {
                const float *c = &col[3 * ((size_t)f * n + pix)];
                ad_blend(p, c[0], c[1], c[2]);
            }
            for (int k = 0; k < 3; k++) { C[3 * pix + k] = p.c[k]; M[3 * pix + k] = p.m[k]; }
            bgra[pix] = p.img;
            K[pix] = p.n;
        }
    wr(d + "/o_sel", sel); wr(d + "/o_et", et); wr(d + "/o_C", C); wr(d + "/o_M", M); wr(d + "/o_K", K); wr(d + "/o_bgra", bgra);
    return 0;
}
