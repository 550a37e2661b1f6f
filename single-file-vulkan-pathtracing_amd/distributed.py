"""Multi-GPU sharding of the radiance loop: one process per GPU, pixel tiles interleaved over the
ranks, ONE collective per presented image.

The path shards with no data-path exchange: a pixel's radiance depends only on (pixel, sample
index, scene) (raygen.rgen:47-48, 88-90 touch nothing but the own texel).  Every rank holds the
whole scene and builds the same LBVH; rank r renders the 8x8 pixel tiles with
(tile_x + tile_y) % world == r -- interleaved, because contiguous bands are badly unbalanced
(44 % of the image, the border, terminates after one ray).

Presenting: `pt_film_present` (csrc/present_rccl.hip) packs the tiles a rank owns, gathers them on
the root with ncclSend / ncclRecv over the library's OWN RCCL communicator (W*H*12/N bytes per rank)
and unpacks them into a separate image; a rank's accumulation film is never written by the
collective, so progressive rendering can continue and present again.  `Presenter` below is the glue
under `torch.distributed`: the launcher's process group only carries the 128-byte RCCL unique id
to the ranks (and, in the CPU emulation of the tests, the packed tiles over gloo).

Film passes on a sharded render: `pt_film_present_planes` gathers any set of the film's planes -- the radiance, the
guides, M, L, K, Q -- into a FILM on the root with the same one collective; `pack_planes_host`, `unpack_planes_host`
and `gather_planes_host` below mirror its packed layout, `Presenter.present_planes` is the glue.
"""
import os

import numpy as np

TILE = 8


def tile_owner(width, height, world):
    """-> int array [H, W]: the rank that renders each pixel (mirror of ensure_work() in
    csrc/film_work.hip ptw_ensure_work)."""
    ty, tx = np.meshgrid(np.arange(height) // TILE, np.arange(width) // TILE, indexing="ij")
    return (tx + ty) % world


def owned_mask(width, height, rank, world):
    return tile_owner(width, height, world) == rank


def tile_list(width, height, rank, world):
    """-> [(tile_x, tile_y)] of a rank in the order the device enumerates them (row major)."""
    tiles_x, tiles_y = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    return [(tx, ty) for ty in range(tiles_y) for tx in range(tiles_x) if (tx + ty) % world == rank]


def pack_tiles_host(film, rank, world):
    """numpy mirror of k_pack_tiles: [n_tiles, 64, 3] float32 (pixels beyond the image edge are 0)."""
    h, w = film.shape[:2]
    tl = tile_list(w, h, rank, world)
    out = np.zeros((len(tl), TILE, TILE, 3), np.float32)
    for k, (tx, ty) in enumerate(tl):
        blk = film[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
        out[k, :blk.shape[0], :blk.shape[1]] = blk
    return out.reshape(len(tl), TILE * TILE, 3)


def unpack_tiles_host(packed, image, rank, world):
    """numpy mirror of k_unpack_tiles: scatter a rank's packed tiles into `image` [H, W, 3]."""
    h, w = image.shape[:2]
    for k, (tx, ty) in enumerate(tile_list(w, h, rank, world)):
        blk = packed[k].reshape(TILE, TILE, 3)
        y1, x1 = min((ty + 1) * TILE, h), min((tx + 1) * TILE, w)
        image[ty * TILE:y1, tx * TILE:x1] = blk[:y1 - ty * TILE, :x1 - tx * TILE]
    return image


def gather_present_host(film, rank, world, dst=0, group=None):
    """The presentation collective on host arrays over any torch.distributed backend (the world-2 gloo test): every
    rank packs its tiles, the root gathers them and unpacks.  -> the presented image on `dst`, None elsewhere;
    `film` is not modified."""
    import torch
    import torch.distributed as dist
    mine = torch.from_numpy(pack_tiles_host(film, rank, world))
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return unpack_tiles_host(mine.numpy(), np.zeros_like(film), rank, world)
    h, w = film.shape[:2]
    counts = [len(tile_list(w, h, r, world)) for r in range(world)]
    if rank == dst:
        bufs = [torch.zeros((counts[r], TILE * TILE, 3), dtype=torch.float32) for r in range(world)]
        bufs[dst] = mine
        reqs = [dist.irecv(bufs[r], src=r, group=group) for r in range(world) if r != dst and counts[r]]
        for q in reqs:
            q.wait()
        image = np.zeros_like(film)
        for r in range(world):
            unpack_tiles_host(bufs[r].numpy(), image, r, world)
        return image
    if counts[rank]:
        dist.send(mine, dst=dst, group=group)
    return None


# ---- the gather of film planes (include/pt_api.h pt_film_present_planes): numpy mirrors of the packed layout ----
# the planes in the record's order: (key of the `planes` dict, channels, PLANES_* bit that names it)
PLANE_ORDER = [("film", 3, 1), ("albedo", 3, 2), ("normal", 3, 2), ("emission", 3, 2), ("depth", 1, 2), ("alpha", 1, 2), ("id", 2, 2),
               ("moments", 3, 4), ("history", 1, 8), ("counts", 1, 16), ("motion", 4, 32)]


def planes_named(which):
    """-> [(key, channels)] of the plane set `which` (PLANES_* bits) in the record's order."""
    if which == 0 or which & ~63:
        raise ValueError("planes must name at least one of PLANES_* and nothing else")
    return [(k, c) for k, c, bit in PLANE_ORDER if which & bit]


def planes_words(which):
    """-> S, the 32-bit words per pixel of the set (pt_film_planes_words)."""
    return sum(c for _, c in planes_named(which))


def _words(a, c):
    """a plane [H, W] or [H, W, c] of a 32-bit dtype as its words [H, W, c] (a view: writes go through)"""
    a = np.asarray(a)
    assert a.dtype.itemsize == 4 and a.flags.c_contiguous, "planes are C-contiguous arrays of a 32-bit type"
    return a.view(np.uint32).reshape(a.shape[0], a.shape[1], c)


def bgra8_host(film):
    """k_resolve's clamp and quantise of a float film [H, W, 3] with A = 255 -> uint8 [H, W, 4] {b, g, r, a}: what the unpack kernel writes."""
    c = np.asarray(film, np.float32)
    with np.errstate(invalid="ignore"):
        q = np.where(c > 0, np.minimum(c, np.float32(1)) * np.float32(255) + np.float32(0.5), np.float32(0)).astype(np.float32)
    out = np.empty(c.shape[:2] + (4,), np.uint8)
    out[..., :3] = q.astype(np.uint8)[..., ::-1]
    out[..., 3] = 255
    return out


def pack_planes_host(planes, rank, world, which):
    """numpy mirror of k_pack_planes: `planes` maps the keys of PLANE_ORDER to arrays [H, W(, channels)] of a 32-bit dtype (the named ones
    have to be there) -> uint32 [n_tiles, 64 * S]: per tile one record, inside it the named planes in the fixed order, each a block
    [64 pixels][channels]; pixels beyond the image edge are zero words."""
    named = planes_named(which)
    h, w = np.asarray(planes[named[0][0]]).shape[:2]
    tl = tile_list(w, h, rank, world)
    out = np.zeros((len(tl), TILE * TILE * planes_words(which)), np.uint32)
    off = 0
    for key, c in named:
        src = _words(planes[key], c)
        blk = np.zeros((len(tl), TILE, TILE, c), np.uint32)
        for k, (tx, ty) in enumerate(tl):
            part = src[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
            blk[k, :part.shape[0], :part.shape[1]] = part
        out[:, off:off + TILE * TILE * c] = blk.reshape(len(tl), TILE * TILE * c)
        off += TILE * TILE * c
    return out


def unpack_planes_host(packed, planes, rank, world, which):
    """numpy mirror of k_unpack_planes: scatter a rank's records into the named arrays of `planes`, in place: exactly the pixels of that
    rank's tiles.  With the film in the set and a "bgra8" array [H, W, 4] uint8 in `planes`, those pixels' bgra8 too."""
    named = planes_named(which)
    h, w = np.asarray(planes[named[0][0]]).shape[:2]
    tl = tile_list(w, h, rank, world)
    packed = np.asarray(packed, np.uint32).reshape(len(tl), TILE * TILE * planes_words(which))
    off = 0
    for key, c in named:
        dst = _words(planes[key], c)
        blk = packed[:, off:off + TILE * TILE * c].reshape(len(tl), TILE, TILE, c)
        for k, (tx, ty) in enumerate(tl):
            y1, x1 = min((ty + 1) * TILE, h), min((tx + 1) * TILE, w)
            dst[ty * TILE:y1, tx * TILE:x1] = blk[k, :y1 - ty * TILE, :x1 - tx * TILE]
            if key == "film" and "bgra8" in planes:
                planes["bgra8"][ty * TILE:y1, tx * TILE:x1] = bgra8_host(dst[ty * TILE:y1, tx * TILE:x1].view(np.float32))
        off += TILE * TILE * c
    return planes


def gather_planes_host(planes, rank, world, which, dst=0, group=None):
    """pt_film_present_planes on host arrays over any torch.distributed backend, in the shape of gather_present_host: every rank packs the
    named planes of its tiles, the root gathers the records and unpacks them.  -> on `dst` a dict of new arrays, the named planes of the whole
    image (and "bgra8" with the film in the set), None elsewhere; `planes` is not modified."""
    import torch
    import torch.distributed as dist
    named = planes_named(which)
    h, w = np.asarray(planes[named[0][0]]).shape[:2]
    rec = TILE * TILE * planes_words(which)
    mine = torch.from_numpy(pack_planes_host(planes, rank, world, which).view(np.int32))   # (gloo has no uint32)
    alone = not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1)
    if not alone and rank != dst:
        if mine.shape[0]:
            dist.send(mine, dst=dst, group=group)
        return None
    out = {k: np.zeros_like(np.asarray(planes[k])) for k, _ in named}
    if which & 1:
        out["bgra8"] = np.zeros((h, w, 4), np.uint8)
    if alone:
        return unpack_planes_host(mine.numpy().view(np.uint32), out, rank, world, which)
    counts = [len(tile_list(w, h, r, world)) for r in range(world)]
    bufs = [mine if r == dst else torch.zeros((counts[r], rec), dtype=torch.int32) for r in range(world)]
    for q in [dist.irecv(bufs[r], src=r, group=group) for r in range(world) if r != dst and counts[r]]:
        q.wait()
    for r in range(world):
        unpack_planes_host(bufs[r].numpy().view(np.uint32), out, r, world, which)
    return out


def selftest_film(width, height, rank, world):
    """The film of the presentation self-test: this rank's tiles carry ITS colour -- (rank + 1, 100 + rank, tile x + 1000 * tile y) -- and
    every other pixel is zero, as after a render of its shard."""
    ty, tx = np.meshgrid(np.arange(height) // TILE, np.arange(width) // TILE, indexing="ij")
    film = np.zeros((height, width, 3), np.float32)
    own = (tx + ty) % world == rank
    film[..., 0] = np.where(own, rank + 1, 0)
    film[..., 1] = np.where(own, 100 + rank, 0)
    film[..., 2] = np.where(own, tx + 1000 * ty, 0)
    return film


def selftest_check(image, world):
    """The presented image of the self-test on the root: every pixel must carry the colour of the rank that OWNS its tile.
    -> {"ok", "ranks_seen", "wrong_pixels", "tiles_per_rank"}"""
    h, w = image.shape[:2]
    ty, tx = np.meshgrid(np.arange(h) // TILE, np.arange(w) // TILE, indexing="ij")
    owner = (tx + ty) % world
    good = (image[..., 0] == owner + 1) & (image[..., 1] == 100 + owner) & (image[..., 2] == tx + 1000 * ty)
    tiles = [int(len(tile_list(w, h, r, world))) for r in range(world)]
    seen = sorted(set(int(x) - 1 for x in np.unique(image[..., 0]) if x >= 1))
    return {"ok": bool(good.all()), "ranks_seen": seen, "wrong_pixels": int((~good).sum()), "tiles_per_rank": tiles}


class Presenter:
    """bench.py's glue: this rank's film -> the presented image on rank 0, once per call.

    Real run: the library's own RCCL communicator (`Comm`), created from a unique id that rank 0 makes and
    torch.distributed broadcasts.  PT_BENCH_EMULATE (all ranks on GPU 0, gloo): the same pack / unpack kernels with
    the packed tiles carried by gloo -- RCCL cannot put two ranks on one device."""

    def __init__(self, pt, ctx, film, film_tensor, rank, world, cdev, emulate):
        import torch
        import torch.distributed as dist
        self.pt, self.ctx, self.film, self.rank, self.world, self.emulate = pt, ctx, film, rank, world, emulate
        self.torch, self.dist = torch, dist
        dev = film_tensor.device
        self.image = torch.zeros_like(film_tensor) if rank == 0 else None
        self.comm = None
        self.ranks_seen = None
        self.fallback = None
        if emulate:
            self.counts = [pt.film_tile_count(film, r, world) for r in range(world)]
            self.packed = torch.zeros((max(self.counts[rank], 1), 64, 3), dtype=torch.float32, device=dev)
            self.ranks_seen = dist.get_world_size()
        else:
            # the library's communicator; if ANY rank cannot create it (no librccl to dlopen, ncclCommInitRank refused)
            # every rank falls back to the same gather through torch.distributed's RCCL process group, so that a
            # multi-GPU run still presents its image -- and says so in the bench line (`describe`)
            err = None
            try:
                if os.environ.get("PT_PRESENT_FORCE_TORCH"):   # tests: take the fallback
                    raise RuntimeError("PT_PRESENT_FORCE_TORCH")
                box = [pt.Comm.unique_id() if rank == 0 else None]
            except Exception as e:          # rank 0 could not even make the id: the others must not wait for a peer
                box, err = [None], e
            dist.broadcast_object_list(box, src=0)
            if box[0] is not None:
                try:
                    self.comm = pt.Comm(ctx, box[0], world, rank)
                    self.ranks_seen = self.comm.ranks()
                except Exception as e:
                    err = e
            else:
                err = err or RuntimeError("rank 0 has no RCCL unique id")
            bad = torch.tensor([1 if err is not None else 0], dtype=torch.int32, device=dev)
            dist.all_reduce(bad, op=dist.ReduceOp.MAX)
            if int(bad.item()):
                if self.comm:
                    self.comm.close()
                    self.comm = None
                self.fallback = repr(err) if err is not None else "another rank failed to create the communicator"
                self.counts = [pt.film_tile_count(film, r, world) for r in range(world)]
                self.packed = torch.zeros((max(self.counts[rank], 1), 64, 3), dtype=torch.float32, device=dev)
                self.ranks_seen = dist.get_world_size()

    def describe(self):
        if self.emulate:
            return "packed tiles gathered over gloo (emulation)"
        if self.fallback:
            return ("one RCCL gather of the packed tiles to rank 0 through torch.distributed send/recv (the library's own "
                    "communicator could not be created: %s)" % self.fallback)
        return "one RCCL gather of the packed tiles to rank 0 (pt_film_present: ncclSend/ncclRecv, own communicator)"

    def present(self):
        pt, torch, dist = self.pt, self.torch, self.dist
        if self.comm:
            self.comm.present(self.film, self.image.data_ptr() if self.rank == 0 else 0, root=0)
            return self.image
        if not self.emulate:   # fallback: same pack / unpack kernels, device buffers through the process group (RCCL)
            pt.film_pack_tiles(self.film, self.rank, self.world, self.packed.data_ptr())
            torch.cuda.synchronize()
            if self.rank == 0:
                bufs = [self.packed] + [torch.zeros((max(self.counts[r], 1), 64, 3), dtype=torch.float32, device=self.packed.device)
                                        for r in range(1, self.world)]
                ops = [dist.P2POp(dist.irecv, bufs[r], r) for r in range(1, self.world) if self.counts[r]]
                for w in (dist.batch_isend_irecv(ops) if ops else []):
                    w.wait()
                torch.cuda.synchronize()
                for r in range(self.world):
                    pt.film_unpack_tiles(self.film, r, self.world, bufs[r].data_ptr(), self.image.data_ptr())
                return self.image
            if self.counts[self.rank]:
                for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, self.packed, 0)]):
                    w.wait()
            return None
        pt.film_pack_tiles(self.film, self.rank, self.world, self.packed.data_ptr())
        host = self.packed.cpu()
        if self.rank == 0:
            for r in range(self.world):
                if r == 0:
                    buf = host
                else:
                    buf = torch.zeros((max(self.counts[r], 1), 64, 3), dtype=torch.float32)
                    if self.counts[r]:
                        dist.recv(buf, src=r)
                d = buf.to(self.image.device)
                pt.film_unpack_tiles(self.film, r, self.world, d.data_ptr(), self.image.data_ptr())
            return self.image
        if self.counts[self.rank]:
            dist.send(host, dst=0)
        return None

    def present_planes(self, dst_film, planes):
        """present() for a set of film planes (pt.PLANES_*), into a FILM: this rank's film -> the named planes (and the bgra8) of `dst_film`
        on rank 0, over the transport the Presenter was built with.  dst_film: a Film of the same size that has the named planes on rank 0,
        None elsewhere; every film pass runs on it afterwards.  -> dst_film on rank 0, None elsewhere.  The ranks agree beforehand that
        their films have the planes (pt_film_present_planes in include/pt_api.h)."""
        pt, torch, dist = self.pt, self.torch, self.dist
        if self.comm:
            self.comm.present_planes(self.film, dst_film if self.rank == 0 else None, planes, root=0)
            return dst_film if self.rank == 0 else None
        rec = 64 * pt.film_planes_words(self.film, planes)
        dev = self.packed.device
        mine = torch.empty((max(self.counts[self.rank], 1), rec), dtype=torch.int32, device=dev)   # (no fill queued on torch's stream: the pack writes every word)
        pt.film_pack_planes(self.film, self.rank, self.world, planes, mine.data_ptr())
        if not self.emulate:   # fallback: the same kernels, device buffers through the process group (RCCL)
            torch.cuda.synchronize()
            if self.rank == 0:
                bufs = [mine] + [torch.zeros((max(self.counts[r], 1), rec), dtype=torch.int32, device=dev) for r in range(1, self.world)]
                ops = [dist.P2POp(dist.irecv, bufs[r], r) for r in range(1, self.world) if self.counts[r]]
                for w in (dist.batch_isend_irecv(ops) if ops else []):
                    w.wait()
                torch.cuda.synchronize()
                for r in range(self.world):
                    pt.film_unpack_planes(dst_film, r, self.world, planes, bufs[r].data_ptr())
                return dst_film
            if self.counts[self.rank]:
                for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, mine, 0)]):
                    w.wait()
            return None
        host = mine.cpu()   # emulation: all ranks on one device, the records carried by gloo
        if self.rank == 0:
            for r in range(self.world):
                buf = host
                if r != 0:
                    buf = torch.zeros((max(self.counts[r], 1), rec), dtype=torch.int32)
                    if self.counts[r]:
                        dist.recv(buf, src=r)
                d = buf.to(dev)
                torch.cuda.synchronize()   # (the copy is torch's stream's, the unpack the context's)
                pt.film_unpack_planes(dst_film, r, self.world, planes, d.data_ptr())
            return dst_film
        if self.counts[self.rank]:
            dist.send(host, dst=0)
        return None

    def selftest(self, film_tensor):
        """Before any timing: present a rank-coloured film through the very collective the run will use and check on the root that every tile
        arrived from the rank that owns it.  `film_tensor` (this rank's accumulation film, torch-owned) is overwritten and left cleared.
        -> the check's record on rank 0 (with how many ranks the communicator connected), None elsewhere."""
        torch = self.torch
        h, w = film_tensor.shape[:2]
        film_tensor.copy_(torch.from_numpy(selftest_film(w, h, self.rank, self.world)).to(film_tensor.device))
        torch.cuda.synchronize()
        img = self.present()
        torch.cuda.synchronize()
        rec = None
        if self.rank == 0:
            rec = selftest_check(img.cpu().numpy(), self.world)
            rec["rccl_ranks"] = self.ranks_seen
            rec["ok"] = bool(rec["ok"] and self.ranks_seen == self.world and rec["ranks_seen"] == list(range(self.world)))
            rec["path"] = self.describe()
        film_tensor.zero_()
        torch.cuda.synchronize()
        return rec

    def close(self):
        if self.comm:
            self.comm.close()
            self.comm = None


def sum_counters(values, device, group=None):
    """All-reduce a few exact integer counters (ray counts) as int64."""
    import torch
    import torch.distributed as dist
    t = torch.tensor(list(values), dtype=torch.int64, device=device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return [int(x) for x in t.tolist()]
