// present_rccl.hip -- assembling the presented image of a tile-sharded render on one rank.
//
// The reference renders on physical device 0 only (main.cpp:105) and copies its storage image to the swapchain
// (main.cpp:661-667).  Here N ranks (processes or host threads, one GPU each) render the interleaved 8x8 pixel tiles
// of the SAME image; what stands in for that copy is ONE collective per presented image:
//     pack    every rank gathers the tiles it owns into a dense buffer [tile][64 pixels][rgb]   (k_pack_tiles)
//     gather  ncclSend of that buffer to the root / ncclRecv x (N-1) on the root, one RCCL group: a packed
//             direct-to-root gather moves W*H*12/N bytes per rank (3.1 MB at 1080p, N = 8) over each rank's own
//             xGMI link to the root instead of a 24.9 MB zero-padded ring reduce per rank
//     unpack  the root scatters all ranks' tiles into the presented image                          (k_unpack_tiles)
// The result is written to a separate buffer: every rank's accumulation film stays what it was, so progressive
// rendering can go on and present again (x + 0 = x is not even needed: no arithmetic touches the radiance).
//
// RCCL is loaded with dlopen at the first pt_comm_* call: libpt_amd.so itself does not link it, single-GPU users
// never load it, and a box without RCCL gets PT_ERR_UNSUPPORTED instead of a loader error.
//
// pt_film_present_planes is the same collective for any set of the film's planes -- C, the six guides, M, L, K, Q -- landed in a FILM on the
// root, so that every film pass runs on what N ranks rendered.  One record of 64 * S words per tile (S = words per pixel
// of the named planes), one pack launch per rank, one unpack launch on the root over all ranks' records (k_pack_planes / k_unpack_planes; the
// bodies are present_planes_kernel.h).
#include "pt_internal.h"
#define PP_LOADS_DONE() __builtin_amdgcn_s_waitcnt(0x0F70)   // s_waitcnt vmcnt(0): the other counters at their maxima (gfx9 encoding)
#include "present_planes_kernel.h"

#include <dlfcn.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

namespace {

constexpr int TBP = 256;
constexpr uint32_t TILE_FLOATS = 64 * 3;

// the few RCCL entry points used, by their published C signatures (rccl.h): ncclResult_t is an int (0 = success),
// ncclComm_t an opaque pointer, ncclUniqueId 128 opaque bytes, ncclFloat32 = 7
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(void *id) = nullptr;
    int (*CommInitRank)(void **comm, int nranks, pt_unique_id id, int rank) = nullptr;
    int (*CommDestroy)(void *comm) = nullptr;
    int (*CommCount)(void *comm, int *count) = nullptr;
    int (*Send)(const void *buf, size_t count, int dtype, int peer, void *comm, hipStream_t st) = nullptr;
    int (*Recv)(void *buf, size_t count, int dtype, int peer, void *comm, hipStream_t st) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string err;
};
Rccl g_rccl;
std::once_flag g_rccl_once;

bool rccl_load()
{
    std::call_once(g_rccl_once, [] {
        Rccl &r = g_rccl;
        for (const char *name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so" }) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
        }
        if (!r.lib) { r.err = std::string("RCCL not found: ") + dlerror(); return; }
        auto sym = [&](const char *n) {
            void *p = dlsym(r.lib, n);
            if (!p && r.err.empty()) r.err = std::string("RCCL symbol missing: ") + n;
            return p;
        };
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
        r.CommCount = reinterpret_cast<decltype(r.CommCount)>(sym("ncclCommCount"));
        r.Send = reinterpret_cast<decltype(r.Send)>(sym("ncclSend"));
        r.Recv = reinterpret_cast<decltype(r.Recv)>(sym("ncclRecv"));
        r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
        r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
    });
    return g_rccl.lib && g_rccl.err.empty();
}

uint32_t tile_count(uint32_t w, uint32_t h, uint32_t rank, uint32_t world)
{
    std::vector<uint32_t> t;
    pt_rank_tiles(w, h, rank, world, &t);
    return (uint32_t)t.size();
}

// one thread per float of the packed buffer: [tile][pixel 0..63][rgb]
__global__ __launch_bounds__(TBP) void k_pack_tiles(const float *__restrict__ film, uint32_t w, uint32_t h,
                                                    const uint32_t *__restrict__ tiles, uint32_t n_tiles,
                                                    float *__restrict__ packed)
{
    const uint32_t i = blockIdx.x * TBP + threadIdx.x;
    if (i >= n_tiles * TILE_FLOATS) return;
    const uint32_t t = i / TILE_FLOATS, r = i - t * TILE_FLOATS, px = r / 3u, c = r - 3u * px;
    const uint32_t g = tiles[t];
    const uint32_t x = (g & 0xFFFFu) * 8u + (px & 7u), y = (g >> 16) * 8u + (px >> 3);
    packed[i] = (x < w && y < h) ? film[3 * ((size_t)y * w + x) + c] : 0.f;
}

__global__ __launch_bounds__(TBP) void k_unpack_tiles(const float *__restrict__ packed, uint32_t w, uint32_t h,
                                                      const uint32_t *__restrict__ tiles, uint32_t n_tiles,
                                                      float *__restrict__ image)
{
    const uint32_t i = blockIdx.x * TBP + threadIdx.x;
    if (i >= n_tiles * TILE_FLOATS) return;
    const uint32_t t = i / TILE_FLOATS, r = i - t * TILE_FLOATS, px = r / 3u, c = r - 3u * px;
    const uint32_t g = tiles[t];
    const uint32_t x = (g & 0xFFFFu) * 8u + (px & 7u), y = (g >> 16) * 8u + (px >> 3);
    if (x < w && y < h) image[3 * ((size_t)y * w + x) + c] = packed[i];
}

// One block per tile, thread t word t of every named plane's block (present_planes_kernel.h).  The table is a kernel argument: its pointers,
// channel counts and offsets, the tile word and all that follows from them are wave-uniform.  tiles[i] and record i belong together: for a
// rank's own list, or for the root's concatenation of all ranks' lists over the concatenated receive buffer.
__global__ __launch_bounds__(TBP) void k_pack_planes(const PpTab tab, const PpGeom g, const uint32_t *__restrict__ tiles, uint32_t *__restrict__ packed)
{
    const uint32_t i = blockIdx.x;
    pp_copy<false>(tab, g, tiles[i], packed + (size_t)i * 64u * tab.s, threadIdx.x);
}

// bgra: the film's bgra8 image when the set holds C (the record's first block), else null
__global__ __launch_bounds__(TBP) void k_unpack_planes(const PpTab tab, const PpGeom g, const uint32_t *__restrict__ tiles, const uint32_t *__restrict__ packed,
                                                       uchar4 *__restrict__ bgra)
{
    const uint32_t i = blockIdx.x;
    uint32_t *rec = const_cast<uint32_t *>(packed) + (size_t)i * 64u * tab.s;
    pp_copy<true>(tab, g, tiles[i], rec, threadIdx.x);
    if (bgra && threadIdx.x < 64u) pp_bgra(g, tiles[i], rec, bgra, threadIdx.x);
}

// device copy of a rank's tile list, cached per (film geometry, rank, world) on the communicator / call
struct TileList {
    uint32_t *d = nullptr;
    uint32_t n = 0;
};
pt_status upload_tiles(pt_ctx *ctx, uint32_t w, uint32_t h, uint32_t rank, uint32_t world, TileList &out)
{
    std::vector<uint32_t> t;
    pt_rank_tiles(w, h, rank, world, &t);
    out.n = (uint32_t)t.size();
    out.d = nullptr;
    PT_HIP(ctx, hipMalloc((void **)&out.d, sizeof(uint32_t) * std::max<size_t>(t.size(), 1)));
    if (!t.empty()) PT_HIP(ctx, hipMemcpy(out.d, t.data(), sizeof(uint32_t) * t.size(), hipMemcpyHostToDevice));
    return PT_OK;
}

// ---- the plane sets of pt_film_*_planes ----
constexpr uint32_t PLANE_CH[PP_MAX_PLANES] = { 3, 3, 3, 3, 1, 1, 2, 3, 1, 1, 4 };   // C, albedo, normal, emission, depth, alpha, id, M, L, K, Q
// which PT_PLANES_* bit names entry k of the record's order
inline uint32_t plane_bit(uint32_t k) { return k == 0 ? PT_PLANES_FILM : k <= 6 ? PT_PLANES_GUIDES : k == 7 ? PT_PLANES_MOMENTS : k == 8 ? PT_PLANES_HISTORY : k == 9 ? PT_PLANES_COUNTS : PT_PLANES_MOTION; }
inline bool planes_ok(uint32_t planes) { return planes != 0 && (planes & ~(uint32_t)PT_PLANES_ALL) == 0; }
uint32_t planes_words(uint32_t planes)
{
    uint32_t s = 0;
    for (uint32_t k = 0; k < PP_MAX_PLANES; k++)
        if (planes & plane_bit(k)) s += PLANE_CH[k];
    return s;
}
// The table of the film's named planes in the record's order; a refusal (message: `who`, what the film lacks) when it has not all of them.
pt_status plane_table(pt_film *f, uint32_t planes, const std::string &who, PpTab &tab)
{
    pt_ctx *ctx = f->ctx;
    if ((planes & PT_PLANES_GUIDES) && !f->aov.enabled) return pt_bad(ctx, who + ": " PT_NO_GUIDES_MSG);
    if ((planes & PT_PLANES_MOMENTS) && !f->m2.d) return pt_bad(ctx, who + ": " PT_NO_M_MSG);
    if ((planes & PT_PLANES_HISTORY) && !f->hist.d) return pt_bad(ctx, who + ": " PT_NO_L_MSG);
    if ((planes & PT_PLANES_COUNTS) && !f->cnt.d) return pt_bad(ctx, who + ": " PT_NO_K_MSG);
    if ((planes & PT_PLANES_MOTION) && !f->mo.d) return pt_bad(ctx, who + ": " PT_NO_Q_MSG);
    void *const all[PP_MAX_PLANES] = { f->d_rgb, f->aov.plane[PT_AOV_ALBEDO], f->aov.plane[PT_AOV_NORMAL], f->aov.plane[PT_AOV_EMISSION], f->aov.plane[PT_AOV_DEPTH],
                                       f->aov.plane[PT_AOV_ALPHA], f->aov.plane[PT_AOV_ID], f->m2.d, f->hist.d, f->cnt.d, f->mo.d };
    tab = PpTab{};
    for (uint32_t k = 0; k < PP_MAX_PLANES; k++)
        if (planes & plane_bit(k)) {
            tab.p[tab.n++] = { static_cast<uint32_t *>(all[k]), PLANE_CH[k], 64u * tab.s };
            tab.s += PLANE_CH[k];
        }
    return PT_OK;
}
void launch_pack_planes(const PpTab &tab, const pt_film *f, const uint32_t *d_tiles, uint32_t n_tiles, uint32_t *d_packed, hipStream_t st)
{
    if (n_tiles) k_pack_planes<<<n_tiles, TBP, 0, st>>>(tab, PpGeom{ f->w, f->h }, d_tiles, d_packed);
}
// (planes: the set the table was made for -- with C in it the film's bgra8 image follows)
void launch_unpack_planes(const PpTab &tab, uint32_t planes, pt_film *dst, const uint32_t *d_tiles, uint32_t n_tiles, const uint32_t *d_packed, hipStream_t st)
{
    uchar4 *bgra = (planes & PT_PLANES_FILM) ? reinterpret_cast<uchar4 *>(dst->d_bgra) : nullptr;
    if (n_tiles) k_unpack_planes<<<n_tiles, TBP, 0, st>>>(tab, PpGeom{ dst->w, dst->h }, d_tiles, d_packed, bgra);
}
// what pt_film_pack_planes and pt_film_unpack_planes share: the argument checks, a tile list for the call, one launch, the wait
pt_status planes_standalone(pt_film *f, uint32_t rank, uint32_t world, uint32_t planes, void *d_packed, bool unpack)
{
    if (!f) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    const std::string who = unpack ? "pt_film_unpack_planes" : "pt_film_pack_planes";
    if (!d_packed || world == 0 || rank >= world || !planes_ok(planes)) return pt_bad(ctx, who + ": bad argument");
    PpTab tab;
    PT_TRY(plane_table(f, planes, who, tab));
    PT_HIP(ctx, hipSetDevice(ctx->device));
    TileList tl;
    PT_TRY(upload_tiles(ctx, f->w, f->h, rank, world, tl));
    if (unpack) launch_unpack_planes(tab, planes, f, tl.d, tl.n, static_cast<const uint32_t *>(d_packed), ctx->stream);
    else launch_pack_planes(tab, f, tl.d, tl.n, static_cast<uint32_t *>(d_packed), ctx->stream);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(tl.d);
    PT_HIP(ctx, e);
    PT_HIP(ctx, hipGetLastError());
    return PT_OK;
}

}  // namespace

struct pt_comm {
    pt_ctx *ctx = nullptr;
    void *nccl = nullptr;
    uint32_t world = 1, rank = 0;
    // per (film geometry, root): tile lists of every rank, the packed send buffer and the root's receive buffer
    uint32_t w = 0, h = 0, root = 0;
    std::vector<TileList> tiles;   // [world]
    float *d_send = nullptr;
    float *d_recv = nullptr;       // root: concatenation of all ranks' packed tiles
    std::vector<size_t> recv_off;  // [world + 1] in floats
    // pt_film_present_planes, per (film size, root, plane set): this rank's tile list -- on the root the concatenation of every rank's, in rank
    // order -- and the packed buffers in words; replaced only when the key changes
    struct Planes {
        uint32_t w = 0, h = 0, root = 0, planes = 0;   // planes == 0: nothing staged
        uint32_t *d_tiles = nullptr;
        std::vector<uint32_t> tile_off;                // [world + 1] tiles before each rank's
        uint32_t *d_buf = nullptr;                     // the root: all ranks' records; elsewhere: this rank's
    } pl;
};

static void comm_free_geometry(pt_comm *c)
{
    for (TileList &t : c->tiles) (void)hipFree(t.d);
    c->tiles.clear();
    (void)hipFree(c->d_send);
    (void)hipFree(c->d_recv);
    c->d_send = c->d_recv = nullptr;
    c->recv_off.clear();
    c->w = c->h = 0;
}

static void comm_free_planes(pt_comm *c)
{
    (void)hipFree(c->pl.d_tiles);
    (void)hipFree(c->pl.d_buf);
    c->pl = pt_comm::Planes{};
}

extern "C" {

pt_status pt_film_tile_count(const pt_film *f, uint32_t rank, uint32_t world, uint32_t *n_tiles)
{
    if (!f || !n_tiles || world == 0 || rank >= world) return PT_ERR_INVALID_ARG;
    *n_tiles = tile_count(f->w, f->h, rank, world);
    return PT_OK;
}

pt_status pt_film_pack_tiles(pt_film *f, uint32_t rank, uint32_t world, float *d_packed)
{
    if (!f) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    if (!d_packed || world == 0 || rank >= world) { ctx->err = "pt_film_pack_tiles: bad argument"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    TileList tl;
    pt_status rc = upload_tiles(ctx, f->w, f->h, rank, world, tl);
    if (rc != PT_OK) return rc;
    const uint32_t n = tl.n * TILE_FLOATS;
    if (n) k_pack_tiles<<<(n + TBP - 1) / TBP, TBP, 0, ctx->stream>>>(f->d_rgb, f->w, f->h, tl.d, tl.n, d_packed);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(tl.d);
    PT_HIP(ctx, e);
    PT_HIP(ctx, hipGetLastError());
    return PT_OK;
}

pt_status pt_film_unpack_tiles(pt_film *f, uint32_t rank, uint32_t world, const float *d_packed, float *d_image)
{
    if (!f) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    if (!d_packed || !d_image || world == 0 || rank >= world) { ctx->err = "pt_film_unpack_tiles: bad argument"; return PT_ERR_INVALID_ARG; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    TileList tl;
    pt_status rc = upload_tiles(ctx, f->w, f->h, rank, world, tl);
    if (rc != PT_OK) return rc;
    const uint32_t n = tl.n * TILE_FLOATS;
    if (n) k_unpack_tiles<<<(n + TBP - 1) / TBP, TBP, 0, ctx->stream>>>(d_packed, f->w, f->h, tl.d, tl.n, d_image);
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(tl.d);
    PT_HIP(ctx, e);
    PT_HIP(ctx, hipGetLastError());
    return PT_OK;
}

pt_status pt_comm_unique_id(pt_unique_id *id)
{
    if (!id) return PT_ERR_INVALID_ARG;
    if (!rccl_load()) return PT_ERR_UNSUPPORTED;
    return g_rccl.GetUniqueId(id) == 0 ? PT_OK : PT_ERR_HIP;
}

pt_status pt_comm_create(pt_ctx *ctx, const pt_unique_id *id, uint32_t world, uint32_t rank, pt_comm **out)
{
    if (!ctx) return PT_ERR_INVALID_ARG;
    if (!out || !id || world == 0 || rank >= world) { ctx->err = "pt_comm_create: bad argument"; return PT_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!rccl_load()) { ctx->err = g_rccl.err.empty() ? "RCCL unavailable" : g_rccl.err; return PT_ERR_UNSUPPORTED; }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    pt_comm *c = new (std::nothrow) pt_comm();
    if (!c) return PT_ERR_OOM;
    c->ctx = ctx; c->world = world; c->rank = rank;
    const int r = g_rccl.CommInitRank(&c->nccl, (int)world, *id, (int)rank);
    if (r != 0) {
        ctx->err = std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error");
        delete c;
        return PT_ERR_HIP;
    }
    *out = c;
    return PT_OK;
}

pt_status pt_comm_ranks(const pt_comm *c, uint32_t *n)
{
    if (!c || !n) return PT_ERR_INVALID_ARG;
    int cnt = 0;
    if (g_rccl.CommCount(c->nccl, &cnt) != 0) return PT_ERR_HIP;
    *n = (uint32_t)cnt;
    return PT_OK;
}

void pt_comm_destroy(pt_comm *c)
{
    if (!c) return;
    (void)hipSetDevice(c->ctx->device);
    comm_free_geometry(c);
    comm_free_planes(c);
    if (c->nccl) (void)g_rccl.CommDestroy(c->nccl);
    delete c;
}

// Every rank of the communicator calls this once per presented image, after its pt_render calls, with the film it
// rendered as (rank, world) of the communicator.  d_image: device memory for width*height*3 floats on the root
// (ignored elsewhere).  Blocking, like the copy + present it replaces (main.cpp:661-683).
pt_status pt_film_present(pt_film *f, pt_comm *c, uint32_t root, float *d_image)
{
    if (!f || !c) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    if (ctx != c->ctx) { ctx->err = "pt_film_present: film and communicator belong to different contexts"; return PT_ERR_INVALID_ARG; }
    if (root >= c->world || (c->rank == root && !d_image)) { ctx->err = "pt_film_present: bad root / null image on the root"; return PT_ERR_INVALID_ARG; }
    if (f->work.d_tiles && (f->work.rank != c->rank || f->work.world != c->world)) {
        ctx->err = "pt_film_present: the film was rendered as another (rank, world) than the communicator's";
        return PT_ERR_INVALID_ARG;
    }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (c->w != f->w || c->h != f->h || c->root != root) {  // first presentation of this (geometry, root): tile lists and staging buffers
        comm_free_geometry(c);
        c->tiles.resize(c->world);
        c->recv_off.assign(c->world + 1, 0);
        for (uint32_t r = 0; r < c->world; r++) {
            const bool need = r == c->rank || c->rank == root;  // the root unpacks everyone's tiles
            if (need) {
                const pt_status rc = upload_tiles(ctx, f->w, f->h, r, c->world, c->tiles[r]);
                if (rc != PT_OK) return rc;
            } else {
                c->tiles[r].n = tile_count(f->w, f->h, r, c->world);
            }
            c->recv_off[r + 1] = c->recv_off[r] + (size_t)c->tiles[r].n * TILE_FLOATS;
        }
        PT_HIP(ctx, hipMalloc((void **)&c->d_send, sizeof(float) * std::max<size_t>((size_t)c->tiles[c->rank].n * TILE_FLOATS, 1)));
        if (c->rank == root) PT_HIP(ctx, hipMalloc((void **)&c->d_recv, sizeof(float) * std::max<size_t>(c->recv_off[c->world], 1)));
        c->w = f->w; c->h = f->h; c->root = root;
    }
    const TileList &mine = c->tiles[c->rank];
    const uint32_t n_mine = mine.n * TILE_FLOATS;
    float *const send = c->rank == root ? c->d_recv + c->recv_off[root] : c->d_send;  // the root packs in place
    if (n_mine) k_pack_tiles<<<(n_mine + TBP - 1) / TBP, TBP, 0, st>>>(f->d_rgb, f->w, f->h, mine.d, mine.n, send);
    if (c->world > 1) {
        int r = g_rccl.GroupStart();
        if (c->rank == root) {
            for (uint32_t p = 0; p < c->world && r == 0; p++)
                if (p != root && c->tiles[p].n)
                    r = g_rccl.Recv(c->d_recv + c->recv_off[p], (size_t)c->tiles[p].n * TILE_FLOATS, 7 /* ncclFloat32 */, (int)p, c->nccl, st);
        } else if (n_mine) {
            r = g_rccl.Send(send, n_mine, 7, (int)root, c->nccl, st);
        }
        const int r2 = g_rccl.GroupEnd();
        if (r != 0 || r2 != 0) {
            ctx->err = std::string("RCCL gather of the packed tiles: ") + g_rccl.GetErrorString(r != 0 ? r : r2);
            return PT_ERR_HIP;
        }
    }
    if (c->rank == root)
        for (uint32_t p = 0; p < c->world; p++) {
            const uint32_t n = c->tiles[p].n * TILE_FLOATS;
            if (n) k_unpack_tiles<<<(n + TBP - 1) / TBP, TBP, 0, st>>>(c->d_recv + c->recv_off[p], f->w, f->h, c->tiles[p].d, c->tiles[p].n, d_image);
        }
    PT_HIP(ctx, hipStreamSynchronize(st));
    PT_HIP(ctx, hipGetLastError());
    return PT_OK;
}

pt_status pt_film_planes_words(const pt_film *f, uint32_t planes, uint32_t *words_per_pixel)
{
    if (!f || !words_per_pixel || !planes_ok(planes)) return PT_ERR_INVALID_ARG;
    *words_per_pixel = planes_words(planes);
    return PT_OK;
}

pt_status pt_film_pack_planes(pt_film *f, uint32_t rank, uint32_t world, uint32_t planes, void *d_packed)
{
    return planes_standalone(f, rank, world, planes, d_packed, false);
}

pt_status pt_film_unpack_planes(pt_film *dst, uint32_t rank, uint32_t world, uint32_t planes, const void *d_packed)
{
    return planes_standalone(dst, rank, world, planes, const_cast<void *>(d_packed), true);
}

// pt_film_present for a set of planes, into a film on the root: include/pt_api.h has the contract.
pt_status pt_film_present_planes(pt_film *f, pt_comm *c, uint32_t root, uint32_t planes, pt_film *dst, float *device_ms)
{
    if (!f || !c) return PT_ERR_INVALID_ARG;
    pt_ctx *ctx = f->ctx;
    const std::string who = "pt_film_present_planes";
    if (ctx != c->ctx) return pt_bad(ctx, who + ": film and communicator belong to different contexts");
    if (!planes_ok(planes)) return pt_bad(ctx, who + ": planes must name at least one of PT_PLANES_* and nothing else");
    if (root >= c->world) return pt_bad(ctx, who + ": bad root");
    if (f->work.d_tiles && (f->work.rank != c->rank || f->work.world != c->world))
        return pt_bad(ctx, who + ": the film was rendered as another (rank, world) than the communicator's");
    PpTab src_tab, dst_tab;
    PT_TRY(plane_table(f, planes, who, src_tab));
    const bool is_root = c->rank == root;
    if (is_root) {
        if (!dst) return pt_bad(ctx, who + ": null dst on the root");
        if (dst == f) return pt_bad(ctx, who + ": dst must be another film than the one presented");
        if (dst->ctx != ctx || dst->w != f->w || dst->h != f->h) return pt_bad(ctx, who + ": dst has another size or context than the film");
        PT_TRY(plane_table(dst, planes, who + " (dst)", dst_tab));
    }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    pt_comm::Planes &pl = c->pl;
    const size_t rec = 64u * (size_t)src_tab.s;   // words per tile
    if (pl.planes != planes || pl.w != f->w || pl.h != f->h || pl.root != root) {   // first presentation of this (size, root, plane set)
        comm_free_planes(c);
        std::vector<uint32_t> tiles;
        std::vector<uint32_t> off(c->world + 1, 0);
        for (uint32_t r = 0; r < c->world; r++) {
            std::vector<uint32_t> t;
            pt_rank_tiles(f->w, f->h, r, c->world, &t);
            off[r + 1] = off[r] + (uint32_t)t.size();
            if (is_root || r == c->rank) tiles.insert(tiles.end(), t.begin(), t.end());
        }
        const size_t n_buf = is_root ? off[c->world] : off[c->rank + 1] - off[c->rank];
        DevBuf<uint32_t> d_tiles, d_buf;
        PT_HIP(ctx, d_tiles.alloc(tiles.size()));
        PT_HIP(ctx, d_buf.alloc(n_buf * rec));
        if (!tiles.empty()) PT_HIP(ctx, hipMemcpy(d_tiles.p, tiles.data(), sizeof(uint32_t) * tiles.size(), hipMemcpyHostToDevice));
        pl.d_tiles = d_tiles.release(); pl.d_buf = d_buf.release();
        pl.tile_off = std::move(off);
        pl.w = f->w; pl.h = f->h; pl.root = root; pl.planes = planes;
    }
    const uint32_t n_mine = pl.tile_off[c->rank + 1] - pl.tile_off[c->rank];
    const size_t first = is_root ? pl.tile_off[c->rank] : 0;   // where this rank's tiles and records start in d_tiles / d_buf
    int rccl_err = 0;
    PT_TRY(pt_timed_pass(ctx, device_ms, [&](hipStream_t st) {
        launch_pack_planes(src_tab, f, pl.d_tiles + first, n_mine, pl.d_buf + first * rec, st);   // (the root packs in place)
        if (c->world > 1) {
            int r = g_rccl.GroupStart();
            if (is_root) {
                for (uint32_t p = 0; p < c->world && r == 0; p++) {
                    const uint32_t n = pl.tile_off[p + 1] - pl.tile_off[p];
                    if (p != root && n) r = g_rccl.Recv(pl.d_buf + pl.tile_off[p] * rec, n * rec, 3 /* ncclUint32 */, (int)p, c->nccl, st);
                }
            } else if (n_mine) {
                r = g_rccl.Send(pl.d_buf, n_mine * rec, 3, (int)root, c->nccl, st);
            }
            const int r2 = g_rccl.GroupEnd();
            rccl_err = r != 0 ? r : r2;
        }
        if (is_root && rccl_err == 0) launch_unpack_planes(dst_tab, planes, dst, pl.d_tiles, pl.tile_off[c->world], pl.d_buf, st);
    }));
    if (rccl_err != 0) {
        ctx->err = std::string("RCCL gather of the packed planes: ") + g_rccl.GetErrorString(rccl_err);
        return PT_ERR_HIP;
    }
    if (is_root && (planes & PT_PLANES_MOMENTS)) dst->m2.frames = f->m2.frames;
    return PT_OK;
}

}  // extern "C"
