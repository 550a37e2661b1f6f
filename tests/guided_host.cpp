// guided_host.cpp -- the per-pixel body of k_guided_reduce (csrc/guided_kernel.h: the log index, the cull and edge tests, the fold, the blend),
// compiled for the host and run over a first-hit log read from files: what tests/test_render_guided.py holds against its numpy restatement of
// the guides' definition without a GPU, and under the host's sanitizers.  Every array is a vector of exactly its size, so an index that leaves
// the log or a table is the sanitizer's to find.  The IEEE divide and root (kernel_host.h) stand in for pt_math.h's fdiv and fsqrt, their
// bitwise equals; compile with -ffp-contract=off.  What kernel_host.h lacks for this header is brought here.
// usage: guided_host DIR  (DIR/par: 20 words, see main; tiles, log, tri4, shade4, faces, inst6, inst_frame, inst_id and the six planes in;
// o_albedo .. o_id out; see _run_on_host in the test)
#include "kernel_host.h"
#include <cstring>
constexpr uint32_t PT_MISS = 0xFFFFFFFFu;
inline uint2 make_uint2(uint32_t a, uint32_t b) { return { a, b }; }
inline uint32_t __float_as_uint(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
#include "guided_kernel.h"
int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: guided_host DIR\n"); return 2; }
    const std::string d = argv[1];
    // w h spp n_frames frame0 id_frame n_tiles n_tris n_inst inst has_inst_frame cull_on cull[4] (as int32) - - - -
    auto par = rd<int32_t>(d + "/par", 20);
    GdConst gc{};
    gc.width = (uint32_t)par[0]; gc.height = (uint32_t)par[1]; gc.spp = (uint32_t)par[2];
    const uint32_t n_frames = (uint32_t)par[3];
    const int32_t frame0 = par[4];
    const uint32_t id_frame = (uint32_t)par[5], n_tiles = (uint32_t)par[6], n_tris = (uint32_t)par[7], n_inst = (uint32_t)par[8];
    const bool inst = par[9] != 0, has_frame = par[10] != 0;
    gc.slots_per_lane = 64u * n_tiles;
    gc.n_tris = n_tris;
    gc.cull_on = (uint32_t)par[11];
    for (int k = 0; k < 4; k++) gc.cull[k] = par[12 + k];
    const size_t n = (size_t)gc.width * gc.height;
    auto tiles = rd<uint32_t>(d + "/tiles", n_tiles);
    auto log = rd<uint2>(d + "/log", (size_t)n_frames * gc.slots_per_lane * gc.spp);
    auto tri4 = rd<float4>(d + "/tri4", 3 * (size_t)n_tris), shade4 = rd<float4>(d + "/shade4", 3 * (size_t)n_tris);
    auto faces = rd<float>(d + "/faces", 6 * (size_t)n_tris);
    auto inst6 = rd<float4>(d + "/inst6", 6 * (size_t)n_inst), inst_frame = rd<float4>(d + "/inst_frame", has_frame ? 2 * (size_t)n_inst * n_tris : 0);
    auto inst_id = rd<uint32_t>(d + "/inst_id", n_inst);
    auto albedo = rd<float>(d + "/albedo", 3 * n), normal = rd<float>(d + "/normal", 3 * n), emission = rd<float>(d + "/emission", 3 * n);
    auto depth = rd<float>(d + "/depth", n), alpha = rd<float>(d + "/alpha", n);
    auto id = rd<uint2>(d + "/id", n);
    const GdScene sc = { tri4.data(), shade4.data(), faces.data(), inst ? inst6.data() : nullptr, has_frame ? inst_frame.data() : nullptr, inst ? inst_id.data() : nullptr };
    const AovPlanes planes = { albedo.data(), normal.data(), emission.data(), depth.data(), alpha.data(), id.data() };
    for (uint32_t local = 0; local < gc.slots_per_lane; local++) {  // (k_guided_reduce, thread by thread)
        if (inst) gd_reduce_pixel<true>(gc, tiles.data(), local, frame0, n_frames, id_frame, log.data(), sc, planes);
        else gd_reduce_pixel<false>(gc, tiles.data(), local, frame0, n_frames, id_frame, log.data(), sc, planes);
    }
    wr(d + "/o_albedo", albedo); wr(d + "/o_normal", normal); wr(d + "/o_emission", emission); wr(d + "/o_depth", depth); wr(d + "/o_alpha", alpha); wr(d + "/o_id", id);
    return 0;
}
