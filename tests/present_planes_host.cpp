// present_planes_host.cpp -- the bodies of k_pack_planes / k_unpack_planes (csrc/present_planes_kernel.h), compiled for the host and run over every
// thread index of every block: what tests/test_present_planes_cpu.py holds against the numpy mirror (distributed.py pack_planes_host /
// unpack_planes_host) without a GPU, and under the host's sanitizers.  Every plane and every rank's packed buffer is a vector of exactly its
// size, so a word read or written outside its plane or its record is the sanitizer's to find.
// usage: present_planes_host DIR  (DIR/par: w h world planes as uint32; src_K, dst_K: plane K of the record's order, for the named ones, words;
// dst_bgra: w*h*4 bytes.  Writes packed_R for every rank R, then out_K and out_bgra: dst after all ranks' records were unpacked into it.)
#include "kernel_host.h"
#define PP_LOADS_DONE() ((void)0)
#include "present_planes_kernel.h"

static const uint32_t CH[PP_MAX_PLANES] = { 3, 3, 3, 3, 1, 1, 2, 3, 1, 1, 4 };
static const uint32_t BIT[PP_MAX_PLANES] = { 1, 2, 2, 2, 2, 2, 2, 4, 8, 16, 32 };

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: present_planes_host DIR\n"); return 2; }
    const std::string d = argv[1];
    const auto par = rd<uint32_t>(d + "/par", 4);
    const uint32_t w = par[0], h = par[1], world = par[2], planes = par[3];
    const size_t n = (size_t)w * h;
    std::vector<std::vector<uint32_t>> src(PP_MAX_PLANES), dst(PP_MAX_PLANES);
    PpTab st{}, dt{};
    for (uint32_t k = 0; k < PP_MAX_PLANES; k++)
        if (planes & BIT[k]) {
            src[k] = rd<uint32_t>(d + "/src_" + std::to_string(k), n * CH[k]);
            dst[k] = rd<uint32_t>(d + "/dst_" + std::to_string(k), n * CH[k]);
            st.p[st.n++] = { src[k].data(), CH[k], 64u * st.s };
            dt.p[dt.n++] = { dst[k].data(), CH[k], 64u * dt.s };
            st.s += CH[k]; dt.s += CH[k];
        }
    dt.n = st.n;
    auto bgra = rd<uchar4>(d + "/dst_bgra", n);
    const PpGeom g = { w, h };
    const uint32_t tiles_x = (w + 7) / 8, tiles_y = (h + 7) / 8;
    for (uint32_t rank = 0; rank < world; rank++) {
        std::vector<uint32_t> tiles;   // (pt_rank_tiles: row by row, tx | ty << 16)
        for (uint32_t ty = 0; ty < tiles_y; ty++)
            for (uint32_t tx = 0; tx < tiles_x; tx++)
                if ((tx + ty) % world == rank) tiles.push_back(tx | ty << 16);
        const size_t rec = 64u * (size_t)st.s;
        std::vector<uint32_t> packed(tiles.size() * rec, 0xDEADBEEFu);   // (the pack has to write every word)
        for (size_t i = 0; i < tiles.size(); i++)       // one block per tile ...
            for (uint32_t t = 0; t < 256; t++)          // ... of 256 threads
                pp_copy<false>(st, g, tiles[i], packed.data() + i * rec, t);
        if (packed.empty()) packed.reserve(1);   // (a rank without tiles writes an empty file: fwrite wants a pointer all the same)
        wr(d + "/packed_" + std::to_string(rank), packed);
        for (size_t i = 0; i < tiles.size(); i++)
            for (uint32_t t = 0; t < 256; t++) {
                pp_copy<true>(dt, g, tiles[i], packed.data() + i * rec, t);
                if ((planes & 1u) && t < 64u) pp_bgra(g, tiles[i], packed.data() + i * rec, bgra.data(), t);
            }
    }
    for (uint32_t k = 0; k < PP_MAX_PLANES; k++)
        if (planes & BIT[k]) wr(d + "/out_" + std::to_string(k), dst[k]);
    wr(d + "/out_bgra", bgra);
    return 0;
}
