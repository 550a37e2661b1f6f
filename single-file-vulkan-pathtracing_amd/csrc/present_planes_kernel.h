// present_planes_kernel.h -- the index arithmetic and the per-thread bodies of k_pack_planes / k_unpack_planes (present_rccl.hip), in a header of
// its own, like upsample_kernel.h, so that tests/present_planes_host.cpp can compile the very same statements for the host, run them over every
// thread index of a block and hold the result against the numpy mirror (distributed.py pack_planes_host) without a GPU, under the host's
// sanitizers.  Wants declared before it: uchar4, make_uchar4, min, and PP_LOADS_DONE() (the device: one wait for every load issued so far;
// the host: nothing).
//
// The packed layout (include/pt_api.h has it as the contract): per tile ONE record of 64 * S words, S the words per pixel of the named planes;
// inside it the planes in the table's order, each a block [64 pixels][channels]; pixel p of tile (tx, ty) is (8 tx + (p & 7), 8 ty + (p >> 3)).
// A tile row of a plane of c channels is therefore 8 c consecutive words on BOTH sides: words [8 c r, 8 c (r + 1)) of the plane's block, and the
// words of pixels (8 tx .. 8 tx + 7, 8 ty + r) of the film plane.  A block of 256 threads takes one tile; thread t takes word t of every plane's
// block (c <= 4: 64 c <= 256 words; the waves beyond 64 c skip the plane whole), so a wave's 64 lanes touch 256 consecutive bytes of the record
// and 8 / c .. 8 row segments of 32 c bytes of the film.  No division: the row of word t is ((t >> 3) * ceil(32 / c)) >> 5 (exact for t < 64 c,
// c = 1 .. 4: the test program walks all of them), and what lies outside the image is cut off by two comparisons against the tile's valid rows and
// valid words per row, which are the same for the whole block.  Nothing here depends on the lane but t: the table, the tile word and everything
// derived from them are wave-uniform and live in scalar registers.
#pragma once

constexpr uint32_t PP_MAX_PLANES = 11;   // C, the six guides, M, L, K, Q
struct PpPlane {
    uint32_t *ptr;   // the film's plane, [h][w][ch] words
    uint32_t ch;     // 1 .. 4
    uint32_t off;    // where the plane's block starts in a tile's record, in words: 64 * (the channels before it)
};
struct PpTab {       // a kernel argument, by value
    PpPlane p[PP_MAX_PLANES];
    uint32_t n;      // planes named
    uint32_t s;      // words per pixel of all of them: a record is 64 * s words
};
struct PpGeom {
    uint32_t w, h;
};

// what a block knows of its tile: where its first pixel lies in a plane of one channel, and how much of it is inside the image
struct PpTile {
    size_t first;        // y0 * w + x0
    uint32_t x0, y0;
    uint32_t rows, cols; // 0 .. 8 each
};
__device__ __forceinline__ PpTile pp_tile(const PpGeom &g, uint32_t tile_word)
{
    PpTile tl;
    tl.x0 = (tile_word & 0xFFFFu) * 8u;
    tl.y0 = (tile_word >> 16) * 8u;
    tl.cols = tl.x0 < g.w ? min(8u, g.w - tl.x0) : 0u;
    tl.rows = tl.y0 < g.h ? min(8u, g.h - tl.y0) : 0u;
    tl.first = (size_t)tl.y0 * g.w + tl.x0;
    return tl;
}

// word t of the block of a plane of c channels: does the block have it, is its pixel inside the image, and where it lies in the film plane
// counted in words from the tile's first pixel
struct PpWord {
    bool have, inside;
    uint32_t film;
};
__device__ __forceinline__ PpWord pp_word(const PpGeom &g, const PpTile &tl, uint32_t c, uint32_t t)
{
    const uint32_t m = (0x080B1020u >> (8u * (c - 1u))) & 0xFFu;   // ceil(32 / c): 32, 16, 11, 8
    const uint32_t row = ((t >> 3) * m) >> 5;                      // t / (8 c)
    const uint32_t in_row = t - row * (8u * c);
    PpWord o;
    o.have = t < 64u * c;
    o.inside = o.have & (row < tl.rows) & (in_row < c * tl.cols);
    o.film = row * (g.w * c) + in_row;
    return o;
}

// Thread t of the block of one tile: its word of every named plane, film -> record (pack) or record -> film (unpack).  All loads first, then
// all stores.  `rec` is the tile's record.  Pack writes every word of the record (zero for a pixel outside the image); unpack writes the words
// of pixels inside the image and nothing else.
template <bool UNPACK>
__device__ __forceinline__ void pp_copy(const PpTab &tab, const PpGeom &g, uint32_t tile_word, uint32_t *rec, uint32_t t)
{
    const PpTile tl = pp_tile(g, tile_word);
    uint32_t v[PP_MAX_PLANES];
#pragma unroll
    for (uint32_t k = 0; k < PP_MAX_PLANES; k++) {
        v[k] = 0u;
        if (k < tab.n) {
            const uint32_t c = tab.p[k].ch;
            const PpWord wd = pp_word(g, tl, c, t);
            if (wd.inside) v[k] = UNPACK ? rec[tab.p[k].off + t] : (tab.p[k].ptr + tl.first * c)[wd.film];
        }
    }
    // One wait for all the loads, here, where no store is in flight yet.  Left to the compiler, every store's block waits for "everything
    // before it" -- the loads sit in branches of their own, so it cannot count them -- and that includes the store before: eleven round trips.
    PP_LOADS_DONE();
#pragma unroll
    for (uint32_t k = 0; k < PP_MAX_PLANES; k++) {
        if (k < tab.n) {
            const uint32_t c = tab.p[k].ch;
            const PpWord wd = pp_word(g, tl, c, t);
            if (UNPACK) {
                if (wd.inside) (tab.p[k].ptr + tl.first * c)[wd.film] = v[k];
            } else {
                if (wd.have) rec[tab.p[k].off + t] = v[k];
            }
        }
    }
}

// k_resolve's clamp and quantise (shade_kernels.hip to_unorm8)
__device__ __forceinline__ uint8_t pp_unorm8(float c)
{
    if (!(c > 0.0f)) return 0;
    if (c > 1.0f) c = 1.0f;
    return (uint8_t)(c * 255.0f + 0.5f);
}

// Thread t < 64 of an unpacking block whose record starts with C: pixel t's bgra8 from the record's own words (not from the film plane another
// lane has just written), A = 255.
__device__ __forceinline__ void pp_bgra(const PpGeom &g, uint32_t tile_word, const uint32_t *rec, uchar4 *bgra, uint32_t t)
{
    const PpTile tl = pp_tile(g, tile_word);
    const uint32_t col = t & 7u, row = t >> 3;
    if (col < tl.cols && row < tl.rows) {
        const float r = __builtin_bit_cast(float, rec[3u * t + 0u]), gr = __builtin_bit_cast(float, rec[3u * t + 1u]), b = __builtin_bit_cast(float, rec[3u * t + 2u]);
        bgra[tl.first + (size_t)row * g.w + col] = make_uchar4(pp_unorm8(b), pp_unorm8(gr), pp_unorm8(r), 255);
    }
}
