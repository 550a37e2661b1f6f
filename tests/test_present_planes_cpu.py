"""The packed layout of pt_film_present_planes without a GPU: the numpy mirrors (distributed.py pack_planes_host / unpack_planes_host /
gather_planes_host) on ragged sizes and every plane subset, the gather over gloo with two processes, and the kernels' own index arithmetic
(csrc/present_planes_kernel.h) compiled for the host and run over every thread index -- plainly and under AddressSanitizer + UBSan -- against
those mirrors."""
import importlib
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from planes_patterns import LAYOUT_CASES, PLANES, PLANE_SETS, SENTINEL, make_planes, same_words, sentinel_planes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "single-file-vulkan-pathtracing_amd"


@pytest.fixture(scope="module")
def d():
    return importlib.import_module(PKG + ".distributed")


def test_constants_symbols_and_words(pt, d):
    """The PLANES_* values, the four new names in API_SYMBOLS and in the library, S of every set against the mirror's (3 .. 25)."""
    assert (pt.PLANES_FILM, pt.PLANES_GUIDES, pt.PLANES_MOMENTS, pt.PLANES_HISTORY, pt.PLANES_COUNTS, pt.PLANES_MOTION, pt.PLANES_ALL) == (1, 2, 4, 8, 16, 32, 63)
    for name in ("pt_film_planes_words", "pt_film_pack_planes", "pt_film_unpack_planes", "pt_film_present_planes"):
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    assert [d.planes_words(b) for b in (1, 2, 4, 8, 16, 32, 63)] == [3, 13, 3, 1, 1, 4, 25]
    assert [c for _, c, _ in d.PLANE_ORDER] == [int(np.prod(t, dtype=np.int64)) for _, t, _ in PLANES]
    for bad in (0, 64, 127):
        with pytest.raises(ValueError):
            d.planes_named(bad)


@pytest.mark.parametrize("w,h,world", [c for c in LAYOUT_CASES if c[2] > 1])
def test_mirror_round_trip_on_every_subset(d, w, h, world):
    """pack of every rank + unpack into sentinel planes gives the source on the named planes and leaves the others alone, for all 63 sets;
    the records add up to the tile grid; a set of C alone is pack_tiles_host's bytes; pixels beyond the edge pack as zero words."""
    src = make_planes(w, h)
    for which in range(1, 64):
        dst = sentinel_planes(w, h)
        n = 0
        for r in range(world):
            packed = d.pack_planes_host(src, r, world, which)
            assert packed.dtype == np.uint32 and packed.shape == (len(d.tile_list(w, h, r, world)), 64 * d.planes_words(which))
            if which == 1:
                assert same_words(packed, d.pack_tiles_host(src["film"], r, world))
            n += len(packed)
            d.unpack_planes_host(packed, dst, r, world, which)
        assert n == ((w + 7) // 8) * ((h + 7) // 8)
        named = [k for k, _ in d.planes_named(which)]
        for key, _, _ in PLANES:
            if key in named:
                assert same_words(dst[key], src[key]), (which, key)
            else:
                assert (dst[key].view(np.uint32) == SENTINEL).all(), (which, key)
        if which & 1:
            assert same_words(dst["bgra8"], d.bgra8_host(src["film"]))
        else:
            assert (dst["bgra8"] == 0xA5).all()
    # the edge: tile (0, 0) of a 7 x 5 image keeps 35 pixels of its 64; the other words of the depth block are zero
    if (w, h) == (7, 5):
        rec = d.pack_planes_host(src, 0, world, 2)[0]
        depth = rec[64 * 9:64 * 10].reshape(8, 8)
        assert same_words(depth[:5, :7], src["depth"]) and not depth[5:].any() and not depth[:, 7:].any()


def test_bgra8_rule(d):
    """k_resolve's clamp and quantise, A = 255: what is not > 0 (NaN, -0.0, negatives) is 0, what is above 1 (inf) is 255, else c * 255 + 0.5 cut"""
    f = np.array([[[np.nan, -0.0, -1.0], [np.inf, 1.0, 2.0], [0.5, 0.001, 0.999], [1e-40, 0.25, 0.75]]], np.float32)
    assert d.bgra8_host(f).tolist() == [[[0, 0, 0, 255], [255, 255, 255, 255], [255, 0, 128, 255], [191, 64, 0, 255]]]


def _worker(rank, world, port, w, h, out):
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dd = importlib.import_module(PKG + ".distributed")
    full = dict(np.load(out + ".full.npz"))
    own = dd.owned_mask(w, h, rank, world)
    # what a rank's film holds: its own tiles, zero words elsewhere
    mine = {k: np.where(own.reshape(own.shape + (1,) * (v.ndim - 2)), v.view(np.uint32), np.uint32(0)).view(v.dtype) for k, v in full.items()}
    keep = {k: v.copy() for k, v in mine.items()}
    got = {which: dd.gather_planes_host(mine, rank, world, which, dst=0) for which in (63, 1 | 2, 8)}
    assert all(same_words(mine[k], keep[k]) for k in mine)   # the collective leaves the rank's planes alone
    if rank == 0:
        np.savez(out + ".got.npz", **{f"{which}_{k}": v for which, g in got.items() for k, v in g.items()})
    else:
        assert all(g is None for g in got.values())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("w,h", [(64, 40), (61, 37)])
def test_gloo_world2_gather_planes_is_bit_exact(orc, cornell_oracle, d, tmp_path, w, h):
    """Two processes over gloo: the oracle's Cornell film beside synthetic guide, moment, history, count and motion planes, every rank holding
    its own tiles only; the root's gathered planes are the full ones bit for bit, for three plane sets, and the bgra8 follows the film."""
    film, _, _, _ = cornell_oracle.render_frame(orc.default_params(width=w, height=h, spp_per_frame=2, max_depth=4))
    full = make_planes(w, h, seed=5)
    full["film"] = np.ascontiguousarray(film, np.float32)
    out = str(tmp_path / "x")
    np.savez(out + ".full.npz", **full)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, w, h, out), nprocs=2, join=True)
    got = np.load(out + ".got.npz")
    for which in (63, 1 | 2, 8):
        named = [k for k, _ in d.planes_named(which)]
        assert sorted(k.split("_", 1)[1] for k in got.files if k.startswith(f"{which}_")) == sorted(named + (["bgra8"] if which & 1 else []))
        for k in named:
            assert same_words(got[f"{which}_{k}"], full[k]), (which, k)
        if which & 1:
            assert same_words(got[f"{which}_bgra8"], d.bgra8_host(full["film"]))


def _run_on_host(exe, dirname, d, w, h, world, which):
    """tests/present_planes_host.cpp over seeded planes -> ([packed of every rank], dst planes after all unpacks, bgra8)"""
    os.makedirs(dirname, exist_ok=True)
    src, dst = make_planes(w, h), sentinel_planes(w, h)
    np.asarray([w, h, world, which], np.uint32).tofile(os.path.join(dirname, "par"))
    named = [(k, key) for k, (key, _, bit) in enumerate(d.PLANE_ORDER) if which & bit]
    for k, key in named:
        src[key].tofile(os.path.join(dirname, f"src_{k}"))
        dst[key].tofile(os.path.join(dirname, f"dst_{k}"))
    dst["bgra8"].tofile(os.path.join(dirname, "dst_bgra"))
    subprocess.check_call([exe, dirname])
    packed = [np.fromfile(os.path.join(dirname, f"packed_{r}"), np.uint32) for r in range(world)]
    out = {key: np.fromfile(os.path.join(dirname, f"out_{k}"), np.uint32) for k, key in named}
    return src, packed, out, np.fromfile(os.path.join(dirname, "out_bgra"), np.uint8)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_kernel_bodies_on_the_host_equal_the_mirror(d, tmp_path, sanitize):
    """csrc/present_planes_kernel.h -- the statements k_pack_planes / k_unpack_planes run per thread -- compiled by g++ as a stand-alone program
    and run over all 256 thread indices of every tile's block, for every layout case, rank and plane set (all, each alone, one mixed): the
    packed bytes are pack_planes_host's, the unpacked planes and the bgra8 are unpack_planes_host's.  The second build runs the same cases
    under AddressSanitizer and UBSan, every plane and packed buffer allocated at exactly its size: every address is inside its plane or its
    record."""
    exe = str(tmp_path / "present_planes_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20"] + flags +
                          ["-I", os.path.join(REPO, PKG, "csrc"), "-o", exe, os.path.join(REPO, "tests", "present_planes_host.cpp")])
    for n, (w, h, world) in enumerate(LAYOUT_CASES):
        for which in PLANE_SETS:
            src, packed, out, bgra = _run_on_host(exe, str(tmp_path / f"c{n}_{which}"), d, w, h, world, which)
            ref = sentinel_planes(w, h)
            for r in range(world):
                want = d.pack_planes_host(src, r, world, which)
                assert same_words(packed[r], want), (w, h, world, which, r)
                d.unpack_planes_host(want, ref, r, world, which)
            for key in out:
                assert same_words(out[key], ref[key]) and same_words(out[key], src[key]), (w, h, world, which, key)
            assert same_words(bgra, ref["bgra8"]), (w, h, world, which)
