"""pt_film_pack_planes / pt_film_unpack_planes / pt_film_present_planes on the GPU: the packed layout against the numpy mirror
(distributed.py pack_planes_host) byte for byte on ragged sizes, empty ranks and every kind of word; a world-3 render gathered into a film
that equals the one-device film and filters like it; the collective on a world-1 communicator; every refusal."""
import ctypes as C
import importlib

import numpy as np
import pytest

from planes_patterns import LAYOUT_CASES, PLANES, PLANE_SETS, SENTINEL, make_planes, same_words, sentinel_planes

pytestmark = pytest.mark.gpu
PKG = "single-file-vulkan-pathtracing_amd"
AOV_KEYS = ["albedo", "normal", "emission", "depth", "alpha", "id"]   # in PT_AOV_* order


@pytest.fixture(scope="module")
def d():
    return importlib.import_module(PKG + ".distributed")


class PlaneFilm:
    """A film with all eleven planes (or those of `have`, PLANES_* bits; C always), film-owned or in caller-owned DeviceBuffers."""

    def __init__(self, pt, ctx, w, h, external, have=63):
        self.pt, self.ctx, self.w, self.h, self.external, self.have = pt, ctx, w, h, external, have
        self.bufs = {}
        if external:
            for key, tail, _ in PLANES:
                self.bufs[key] = pt.DeviceBuffer(ctx, w * h * 4 * int(np.prod(tail, dtype=np.int64)))
        ptr = (lambda key: self.bufs[key].ptr) if external else (lambda key: None)
        self.film = pt.Film(ctx, w, h, device_ptr=ptr("film"))
        if have & pt.PLANES_GUIDES:
            self.film.enable_aov([ptr(k) for k in AOV_KEYS] if external else None)
        if have & pt.PLANES_MOMENTS:
            self.film.enable_moments(ptr("moments"))
        if have & pt.PLANES_HISTORY:
            self.film.enable_history(ptr("history"))
        if have & pt.PLANES_COUNTS:
            self.film.enable_counts(ptr("counts"))
        if have & pt.PLANES_MOTION:
            self.film.enable_motion(ptr("motion"))

    def write(self, planes, d):
        """every plane of the film from the arrays of `planes`: straight into caller-owned memory, or -- the film's own planes have no writer --
        by unpacking a world-1 record buffer made by the numpy mirror"""
        assert self.have == 63
        if self.external:
            for key, _, _ in PLANES:
                self.bufs[key].write(planes[key])
            return
        packed = d.pack_planes_host(planes, 0, 1, 63)
        buf = self.pt.DeviceBuffer(self.ctx, packed.nbytes)
        buf.write(packed)
        self.pt.film_unpack_planes(self.film, 0, 1, 63, buf.ptr)
        buf.close()

    def read(self):
        f, pt = self.film, self.pt
        out = {"film": f.read_f32(), "bgra8": f.read_bgra8()}
        if self.have & pt.PLANES_GUIDES:
            out.update({k: f.read_aov(i) for i, k in enumerate(AOV_KEYS)})
        if self.have & pt.PLANES_MOMENTS:
            out["moments"] = f.read_moments()[0]
        if self.have & pt.PLANES_HISTORY:
            out["history"] = f.read_history()
        if self.have & pt.PLANES_COUNTS:
            out["counts"] = f.read_counts()
        if self.have & pt.PLANES_MOTION:
            out["motion"] = f.read_motion()
        return out

    def close(self):
        self.film.close()
        for b in self.bufs.values():
            b.close()


def _pack(pt, ctx, film, rank, world, which):
    """pt_film_pack_planes into a fresh device buffer pre-filled with a pattern -> uint32 [n_tiles, 64 * S]"""
    n, s = pt.film_tile_count(film, rank, world), pt.film_planes_words(film, which)
    buf = pt.DeviceBuffer(ctx, max(n * 64 * s * 4, 4))
    buf.write(np.full(max(n * 64 * s, 1), 0xDEADBEEF, np.uint32))
    pt.film_pack_planes(film, rank, world, which, buf.ptr)
    out = buf.read(np.uint32, (n, 64 * s)) if n else np.zeros((0, 64 * s), np.uint32)   # (a rank without tiles: the call launches nothing)
    buf.close()
    return out


def _unpack(pt, ctx, film, rank, world, which, packed):
    buf = pt.DeviceBuffer(ctx, max(packed.nbytes, 4))
    if packed.size:
        buf.write(packed)
    pt.film_unpack_planes(film, rank, world, which, buf.ptr)
    buf.close()


@pytest.mark.parametrize("w,h,world,external", [c + (True,) for c in LAYOUT_CASES] + [(76, 44, 3, False), (7, 5, 4, False)])
def test_layout_against_the_mirror(pt, gpu_ctx, d, w, h, world, external):
    """Planes full of distinct words (NaN payloads, -0.0, denormals, 0xFFFFFFFF among them): every rank's pack of all planes, of each plane
    group alone and of a mixed set is pack_planes_host's bytes (C alone: also pt_film_pack_tiles's); all ranks unpacked into a film full of a
    sentinel give the source on the named planes, the sentinel on the others, and the bgra8 of the numpy rule where C is named."""
    planes = make_planes(w, h)
    src, dst = PlaneFilm(pt, gpu_ctx, w, h, external), PlaneFilm(pt, gpu_ctx, w, h, external)
    try:
        src.write(planes, d)
        got = src.read()
        for key, _, _ in PLANES:
            assert same_words(got[key], planes[key]), key
        for which in PLANE_SETS:
            assert pt.film_planes_words(src.film, which) == d.planes_words(which)
            sent = sentinel_planes(w, h)
            dst.film.clear()
            dst.write(sent, d)
            bgra_before = dst.read()["bgra8"]   # zeros under caller-owned planes; the sentinel film's own bgra8 where the prefill was an unpack
            assert same_words(bgra_before, np.zeros((h, w, 4), np.uint8) if external else d.bgra8_host(sent["film"]))
            for r in range(world):
                packed = _pack(pt, gpu_ctx, src.film, r, world, which)
                assert same_words(packed, d.pack_planes_host(planes, r, world, which)), (which, r)
                if which == pt.PLANES_FILM and packed.size:
                    tiles = pt.DeviceBuffer(gpu_ctx, max(packed.nbytes, 4))
                    pt.film_pack_tiles(src.film, r, world, tiles.ptr)
                    assert same_words(tiles.read(np.uint32, packed.shape), packed), r
                    tiles.close()
                _unpack(pt, gpu_ctx, dst.film, r, world, which, packed)
            got = dst.read()
            named = [k for k, _ in d.planes_named(which)]
            for key, _, _ in PLANES:
                if key in named:
                    assert same_words(got[key], planes[key]), (which, key)
                else:
                    assert (got[key].view(np.uint32) == SENTINEL).all(), (which, key)
            assert same_words(got["bgra8"], d.bgra8_host(planes["film"]) if which & pt.PLANES_FILM else bgra_before), which
        # the pack left its source alone
        got = src.read()
        for key, _, _ in PLANES:
            assert same_words(got[key], planes[key]), key
    finally:
        src.close(); dst.close()


def test_unpack_writes_only_its_ranks_pixels(pt, gpu_ctx, d):
    """One rank of world 3 unpacked into a sentinel film: its tiles' pixels arrive (bgra8 too), every other pixel of every plane stays."""
    w, h, world, r = 61, 37, 3, 1
    planes, sent = make_planes(w, h), sentinel_planes(w, h)
    dst = PlaneFilm(pt, gpu_ctx, w, h, True)
    try:
        dst.write(sent, d)
        _unpack(pt, gpu_ctx, dst.film, r, world, 63, d.pack_planes_host(planes, r, world, 63))
        got, own = dst.read(), d.owned_mask(w, h, r, world)
        for key, _, _ in PLANES:
            g, p = got[key].view(np.uint32).reshape(h, w, -1), planes[key].view(np.uint32).reshape(h, w, -1)
            assert (g[own] == p[own]).all() and (g[~own] == SENTINEL).all(), key
        assert (got["bgra8"][own] == d.bgra8_host(planes["film"])[own]).all() and not got["bgra8"][~own].any()
    finally:
        dst.close()


@pytest.fixture(scope="module")
def sharded(pt, gpu_ctx, cornell_gpu):
    """The Cornell box, 76 x 44, 4 spp, depth 4, frames 0 and 1, moments and guides: one film as world 1, and the three films of world 3
    packed and unpacked into `dst`.  -> (one, dst); neither is written again."""
    w, h, world = 76, 44, 3
    which = pt.PLANES_FILM | pt.PLANES_GUIDES | pt.PLANES_MOMENTS

    def rendered(rank, n):
        f = PlaneFilm(pt, gpu_ctx, w, h, False, have=which)
        p = pt.default_params(width=w, height=h, spp_per_frame=4, max_depth=4, frame=0, frame_count=2, rank=rank, world=n)
        pt.render(cornell_gpu, f.film, p)
        pt.render_aov(cornell_gpu, f.film, p)
        return f
    one, dst = rendered(0, 1), PlaneFilm(pt, gpu_ctx, w, h, False, have=which)
    for r in range(world):
        part = rendered(r, world)
        _unpack(pt, gpu_ctx, dst.film, r, world, which, _pack(pt, gpu_ctx, part.film, r, world, which))
        part.close()
    yield one, dst
    one.close(); dst.close()


def test_sharded_render_gathers_to_the_one_device_film(sharded, d):
    """C, the six guides and M of the gathered film equal the one-device film's, byte for byte; its bgra8 is the quantise rule on C (a render's
    own bgra8 blends through its 8-bit history, frame by frame: that one is not gathered)."""
    one, dst = sharded
    a, b = one.read(), dst.read()
    assert sorted(a) == sorted(b) and len(a) == 9
    assert np.abs(a["film"]).max() > 0 and a["alpha"].max() > 0 and a["moments"].max() > 0
    for key in a:
        if key != "bgra8":
            assert same_words(a[key], b[key]), key
    assert same_words(b["bgra8"], d.bgra8_host(a["film"]))


def test_film_passes_run_on_the_gathered_film(sharded):
    """pt_film_denoise and pt_film_denoise_variance(frames = 2) of the gathered film give the one-device film's filtered bytes, float and bgra8."""
    one, dst = sharded
    for run in (lambda f: f.denoise(), lambda f: f.denoise_variance(frames=2)):
        run(one.film); run(dst.film)
        assert same_words(one.film.read_denoised(), dst.film.read_denoised())
        assert same_words(one.film.read_denoised_bgra8(), dst.film.read_denoised_bgra8())
    assert not same_words(one.film.read_denoised(), one.film.read_f32())


@pytest.fixture()
def comm(pt, gpu_ctx):
    try:
        uid = pt.Comm.unique_id()
    except pt.PtError:
        pytest.skip("RCCL not installed")
    c = pt.Comm(gpu_ctx, uid, 1, 0)
    yield c
    c.close()


def test_collective_world1(pt, gpu_ctx, cornell_gpu, d, comm):
    """Comm.present_planes on a world-1 communicator: dst equals film on every plane (and has the rule's bgra8); two sizes and two plane sets
    in turn -- the staging key; with PLANES_MOMENTS dst takes over `frames`, so denoise_variance(frames = 0) runs on it."""
    for (w, h, which) in ((76, 44, 63), (61, 37, 63), (61, 37, pt.PLANES_FILM | pt.PLANES_HISTORY), (76, 44, 63)):
        planes, sent = make_planes(w, h, seed=w), sentinel_planes(w, h)
        src, dst = PlaneFilm(pt, gpu_ctx, w, h, True), PlaneFilm(pt, gpu_ctx, w, h, True)
        try:
            src.write(planes, d); dst.write(sent, d)
            for _ in range(2):
                ms = comm.present_planes(src.film, dst.film, which)
                assert ms >= 0.0
            got, named = dst.read(), [k for k, _ in d.planes_named(which)]
            for key, _, _ in PLANES:
                assert same_words(got[key], planes[key] if key in named else sent[key]), (w, h, which, key)
            assert same_words(got["bgra8"], d.bgra8_host(planes["film"]))
            assert all(same_words(v, planes[k]) for k, v in src.read().items() if k != "bgra8")
        finally:
            src.close(); dst.close()
    w, h, which = 76, 44, pt.PLANES_FILM | pt.PLANES_GUIDES | pt.PLANES_MOMENTS
    src, dst = PlaneFilm(pt, gpu_ctx, w, h, False, have=which), PlaneFilm(pt, gpu_ctx, w, h, False, have=which)
    try:
        p = pt.default_params(width=w, height=h, spp_per_frame=4, max_depth=4, frame=0, frame_count=2)
        pt.render(cornell_gpu, src.film, p)
        pt.render_aov(cornell_gpu, src.film, p)
        with pytest.raises(pt.PtError):
            dst.film.denoise_variance(frames=0)   # (a film that recorded no frames)
        comm.present_planes(src.film, dst.film, which)
        assert dst.film.read_moments()[1] == src.film.read_moments()[1] == 2
        src.film.denoise_variance(frames=0); dst.film.denoise_variance(frames=0)
        assert same_words(src.film.read_denoised(), dst.film.read_denoised())
    finally:
        src.close(); dst.close()


def _refused(pt, call, text=None):
    with pytest.raises(pt.PtError) as e:
        call()
    assert e.value.status == 1, e.value
    if text:
        assert text in str(e.value), e.value


LACKS = [("PLANES_GUIDES", "no guide buffers"), ("PLANES_MOMENTS", "no second-moment plane"), ("PLANES_HISTORY", "no history-length plane"),
         ("PLANES_COUNTS", "no frame-count plane"), ("PLANES_MOTION", "no motion plane")]


def test_standalone_refusals(pt, gpu_ctx, d):
    """pt_film_pack_planes / pt_film_unpack_planes / pt_film_planes_words: every argument error is PT_ERR_INVALID_ARG and writes nothing."""
    w, h = 61, 37
    L = pt.lib_amd()
    full, bare = PlaneFilm(pt, gpu_ctx, w, h, True), PlaneFilm(pt, gpu_ctx, w, h, True, have=pt.PLANES_FILM)
    buf = pt.DeviceBuffer(gpu_ctx, full.film.width * full.film.height * 4 * 25 * 2)
    try:
        sent = sentinel_planes(w, h)
        full.write(sent, d)
        guard = np.full(buf.nbytes // 4, SENTINEL, np.uint32)
        buf.write(guard)
        n = C.c_uint32(77)
        assert L.pt_film_planes_words(None, 1, C.byref(n)) == 1 and L.pt_film_planes_words(full.film.h, 1, None) == 1
        assert L.pt_film_planes_words(full.film.h, 0, C.byref(n)) == 1 and L.pt_film_planes_words(full.film.h, 64, C.byref(n)) == 1 and n.value == 77
        assert L.pt_film_pack_planes(None, 0, 1, 1, C.c_void_p(buf.ptr)) == 1 and L.pt_film_unpack_planes(None, 0, 1, 1, C.c_void_p(buf.ptr)) == 1
        for fn in (pt.film_pack_planes, pt.film_unpack_planes):
            for (rank, world, which, ptr) in ((0, 1, 0, buf.ptr), (0, 1, 64, buf.ptr), (0, 1, 63 | 128, buf.ptr), (0, 0, 63, buf.ptr), (1, 1, 63, buf.ptr),
                                              (3, 3, 63, buf.ptr), (0, 1, 63, 0)):
                _refused(pt, lambda: fn(full.film, rank, world, which, ptr), "bad argument")
            for name, text in LACKS:
                _refused(pt, lambda: fn(bare.film, 0, 1, getattr(pt, name), buf.ptr), text)
                _refused(pt, lambda: fn(bare.film, 0, 1, 63, buf.ptr), "no guide buffers")
        assert same_words(buf.read(np.uint32, guard.shape), guard)
        got = full.read()
        assert all(same_words(got[k], sent[k]) for k, _, _ in PLANES) and not got["bgra8"].any()
    finally:
        full.close(); bare.close(); buf.close()


def test_present_refusals(pt, gpu_ctx, cornell_gpu, d, comm):
    """pt_film_present_planes: every item of the header's refusal list is PT_ERR_INVALID_ARG, and dst keeps its sentinel."""
    w, h = 61, 37
    L = pt.lib_amd()
    sent = sentinel_planes(w, h)
    src, dst = PlaneFilm(pt, gpu_ctx, w, h, True), PlaneFilm(pt, gpu_ctx, w, h, True)
    bare = PlaneFilm(pt, gpu_ctx, w, h, True, have=pt.PLANES_FILM)
    other_size = PlaneFilm(pt, gpu_ctx, w + 8, h, True)
    ctx2 = pt.Context(0)
    foreign = PlaneFilm(pt, ctx2, w, h, False)
    sharded = pt.Film(gpu_ctx, w, h)
    try:
        src.write(make_planes(w, h), d); dst.write(sent, d)
        ms = C.c_float(0)
        assert L.pt_film_present_planes(None, comm.h, 0, 1, dst.film.h, C.byref(ms)) == 1
        assert L.pt_film_present_planes(src.film.h, None, 0, 1, dst.film.h, C.byref(ms)) == 1
        for which in (0, 64, 63 | 256):
            _refused(pt, lambda: comm.present_planes(src.film, dst.film, which), "planes must name")
        _refused(pt, lambda: comm.present_planes(src.film, dst.film, 63, root=1), "bad root")
        _refused(pt, lambda: comm.present_planes(foreign.film, dst.film, 63))   # (another context's film; the message is that context's)
        assert b"different contexts" in L.pt_last_error(ctx2.h)
        pt.render(cornell_gpu, sharded, pt.default_params(width=w, height=h, spp_per_frame=1, max_depth=2, rank=1, world=2))
        _refused(pt, lambda: comm.present_planes(sharded, dst.film, pt.PLANES_FILM), "another (rank, world)")
        for name, text in LACKS:
            _refused(pt, lambda: comm.present_planes(bare.film, dst.film, getattr(pt, name)), text)
            _refused(pt, lambda: comm.present_planes(src.film, bare.film, getattr(pt, name) | pt.PLANES_FILM), text)   # dst lacks it
        _refused(pt, lambda: comm.present_planes(src.film, None, 63), "null dst")
        _refused(pt, lambda: comm.present_planes(src.film, src.film, 63), "another film")
        _refused(pt, lambda: comm.present_planes(src.film, other_size.film, 63), "another size or context")
        _refused(pt, lambda: comm.present_planes(src.film, foreign.film, 63), "another size or context")
        got = dst.read()
        assert all(same_words(got[k], sent[k]) for k, _, _ in PLANES) and not got["bgra8"].any()
        assert not bare.read()["bgra8"].any()
        comm.present_planes(src.film, dst.film, 63)   # ... and the communicator still works
        assert same_words(dst.read()["motion"], src.read()["motion"])
    finally:
        for f in (src, dst, bare, other_size, foreign):
            f.close()
        sharded.close(); ctx2.close()


def test_presenter_present_planes_emulated(pt, gpu_ctx, d, tmp_path):
    """distributed.Presenter.present_planes over its emulation transport (records carried by gloo, the library's pack / unpack kernels) with a
    process group of one: dst_film takes the planes and the bgra8."""
    torch = pytest.importorskip("torch")
    import torch.distributed as dist
    w, h, which = 61, 37, pt.PLANES_FILM | pt.PLANES_GUIDES
    planes = make_planes(w, h, seed=9)
    src, dst = PlaneFilm(pt, gpu_ctx, w, h, True), PlaneFilm(pt, gpu_ctx, w, h, True)
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    try:
        src.write(planes, d); dst.write(sentinel_planes(w, h), d)
        p = d.Presenter(pt, gpu_ctx, src.film, torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0"), 0, 1, "cuda:0", True)
        assert p.present_planes(dst.film, which) is dst.film
        p.close()
        got, named = dst.read(), [k for k, _ in d.planes_named(which)]
        for key, _, _ in PLANES:
            assert same_words(got[key], planes[key]) == (key in named), key
        assert same_words(got["bgra8"], d.bgra8_host(planes["film"]))
    finally:
        dist.destroy_process_group()
        src.close(); dst.close()
