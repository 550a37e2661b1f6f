"""pt_trace_device without a GPU (include/pt_api.h): the header against the ctypes mirror; the ray recipes of
tests/test_trace_device.py held against the oracle alone, so that a recipe which drifts cannot hide a kernel that says "miss" everywhere; and
the per-lane bodies of the pack, occluded and surface kernels (csrc/trace_device_kernel.h) compiled for the host (tests/trace_device_host.cpp),
run as a program -- plain and under the address and undefined-behaviour sanitizers -- over the oracle's hit records, bit for bit against the
numpy repack, orc.Scene.shade_hit and `faces`."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import trace_device_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MISS = tc.MISS
NEW_SYMBOLS = ["pt_trace_desc_default", "pt_trace_device", "pt_trace_workspace_bytes"]
FIELDS = ["d_rays6", "d_tmax", "d_hits", "d_occluded", "d_position", "d_normal", "d_albedo", "d_emission", "tmin", "tmax", "mode", "extend", "flags",
          "chunk_rays", "reserved"]


def test_trace_desc_layout_defaults_and_symbols(pt, tmp_path):
    """sizeof / offsetof of pt_trace_desc by gcc from the header == the ctypes mirror (104 bytes); the enums' values; the defaults; the new names
    in API_SYMBOLS and in the library; PT_API_VERSION stays 6; NULL handles are PT_ERR_INVALID_ARG."""
    src = tmp_path / "td_layout.c"
    vals = ["sizeof(pt_trace_desc)", "sizeof(pt_hit)"] + ["offsetof(pt_trace_desc, %s)" % f for f in FIELDS] + \
           ["(size_t)PT_TRACE_CLOSEST", "(size_t)PT_TRACE_ANY", "(size_t)PT_TRACE_ASYNC", "(size_t)PT_TRACE_DEFAULT_CHUNK_RAYS", "(size_t)PT_API_VERSION"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("' + "%zu " * len(vals) + '\\n",' + ", ".join(vals) + ");return 0;}\n")
    exe = tmp_path / "td_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    D = pt.TraceDesc
    assert got[:2] == [104, 20] and got[:2] == [C.sizeof(D), pt.HIT_DTYPE.itemsize], got
    assert got[2:2 + len(FIELDS)] == [getattr(D, f).offset for f in FIELDS], got
    assert got[2 + len(FIELDS):] == [0, 1, 1, 1 << 22, 6], got
    assert (pt.TRACE_CLOSEST, pt.TRACE_ANY, pt.TRACE_ASYNC) == (0, 1, 1)
    for name in NEW_SYMBOLS:
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    d = pt.trace_default_desc()   # (touches no device)
    assert [getattr(d, f) for f in FIELDS[:8]] == [None] * 8
    assert (f32(d.tmin), f32(d.tmax), d.mode, d.extend, d.flags, d.chunk_rays, list(d.reserved)) == (f32(0.001), f32(10000.0), pt.TRACE_CLOSEST, pt.EXTEND_AUTO, 0, 0, [0] * 4)
    lib = pt.lib_amd()
    lib.pt_trace_desc_default(None)                                        # (a NULL is ignored)
    assert lib.pt_trace_device(None, C.byref(d), 0, None) == 1
    assert lib.pt_trace_workspace_bytes(None, None) == 1
    assert callable(getattr(pt.Scene, "trace_device", None)) and callable(getattr(pt.Scene, "trace_tensors", None))


def _box_answers(orc, cornell_arrays):
    return tc.answers("box", lambda: tc.Answers(orc.Scene(*cornell_arrays), cornell_arrays[2], tc.make_rays()))


def _inst_answers(orc, cornell_arrays):
    def make():
        osc = orc.Scene(*cornell_arrays)
        osc.set_instances(tc.INSTANCES)
        return tc.Answers(osc, cornell_arrays[2], tc.make_rays(seed=7, x_seed=8))
    return tc.answers("inst", make)


def test_ray_recipes_against_the_oracle_alone(orc, cornell_arrays):
    """What the GPU tests assume of their rays, from the oracle alone: enough hits and enough misses in every prefix, ray 0 a hit that the
    smallest bound does not occlude, most triangles reached, every instance hit, a soup that is neither empty nor opaque."""
    a = _box_answers(orc, cornell_arrays)
    for n in tc.PREFIXES[1:]:
        assert 0.3 <= a.hit_share(n) <= 0.9, (n, a.hit_share(n))
        assert 0.2 <= a.occ_share(n) <= 0.8, (n, a.occ_share(n))
    assert a.hits["prim"][0] != MISS and a.bounds[0] == f32(1e-4) and a.occ_cycled[0] == 0
    reached = np.unique(a.hits["prim"][a.hits["prim"] != MISS])
    assert len(reached) >= 30, len(reached)   # of 36
    b = _inst_answers(orc, cornell_arrays)
    assert 0.2 <= b.hit_share(1000) <= 0.8, b.hit_share(1000)
    ids = b.hits["inst"][b.hits["prim"] != MISS]
    assert set(np.unique(ids)) == {0, 1, 2}, np.unique(ids, return_counts=True)
    v, i, f = tc.soup(4096, 11)
    h, _ = orc.Scene(v, i, f).trace(tc.make_rays(seed=2024, half=1.3, centre=None), mode=0)
    share = float((h["prim"] != MISS).mean())
    assert 0.05 < share < 0.95, share


def _write(d, name, a):
    np.ascontiguousarray(a).tofile(os.path.join(d, name))


def _host_run(exe, d, n, ans, tables, n_inst, frames, with_dtmax, which=15):
    """one run of the host program over the first n rays of `ans`; -> its output arrays"""
    os.makedirs(d, exist_ok=True)
    h = ans.hits[:n]
    miss = h["prim"] == MISS
    hit = np.zeros((n, 4), f32)
    hit[:, 0] = h["prim"].astype(np.uint32).view(f32)   # (leaf order = primitive order; a miss keeps MISS)
    hit[:, 1], hit[:, 2], hit[:, 3] = h["t"], h["u"], h["v"]
    n_tris = len(tables["faces"]) // 6
    tmax = f32(ans.uniform_bound)
    _write(d, "par", np.asarray([n, n_tris, n_inst, int(frames), int(with_dtmax), 1, which, tmax.view(np.uint32)], np.uint32))
    _write(d, "rays6", ans.rays[:n])
    _write(d, "dtmax", ans.bounds[:n] if with_dtmax else np.zeros(0, f32))
    _write(d, "hit", hit)
    _write(d, "hit_inst", h["inst"].astype(np.uint32) if n_inst else np.zeros(0, np.uint32))   # (0xFFFFFFFF on a miss: never an index)
    for name in ("tri4", "rec64", "faces", "inst6"):
        _write(d, name, tables[name])
    _write(d, "inst_frame", tables["inst_frame"] if frames else np.zeros(0, f32))
    subprocess.check_call([exe, d])
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    out = {"rayA": rd("o_rayA", f32).reshape(n, 4), "rayB": rd("o_rayB", f32).reshape(n, 2), "bound": rd("o_bound", f32), "occ": rd("o_occ", np.uint8)}
    for k, name in enumerate(("position", "normal", "albedo", "emission")):
        a = rd("o_" + name, f32)
        out[name] = a.reshape(n, 3) if (which >> k) & 1 else a
    return out, miss


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_kernel_bodies_on_the_host(orc, cornell_arrays, tmp_path, sanitize):
    """The pack, occluded and surface bodies as a program: the packed queue equals the numpy repack, the surface planes equal
    orc.Scene.shade_hit ray by ray and `faces`, a miss gives +0.0, occluded is "position word != MISS" -- bit for bit, at n = 1, 63, 64, 65, 257,
    on the box and on the three-instance scene (inverse transpose and frame table), with all planes and with a single plane."""
    exe = str(tmp_path / "trace_device_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "trace_device_host.cpp")])
    v, i, f = cornell_arrays
    cases = [("box", _box_answers(orc, cornell_arrays), tc.kernel_tables(v, i, f), 0, False),
             ("inst", _inst_answers(orc, cornell_arrays), tc.kernel_tables(v, i, f, tc.INSTANCES), 3, False),
             ("inst_frames", _inst_answers(orc, cornell_arrays), tc.kernel_tables(v, i, f, tc.INSTANCES, frames=True), 3, True)]
    runs = 0
    for name, ans, tables, n_inst, frames in cases:
        for n in tc.PREFIXES[:5]:
            with_dtmax = n % 2 == 1
            out, miss = _host_run(exe, str(tmp_path / f"{name}_{n}"), n, ans, tables, n_inst, frames, with_dtmax)
            assert out["rayA"].tobytes() == ans.rays[:n, :4].tobytes() and out["rayB"].tobytes() == ans.rays[:n, 4:].tobytes(), (name, n)
            want_bound = ans.bounds[:n] if with_dtmax else np.full(n, ans.uniform_bound, f32)
            assert out["bound"].tobytes() == want_bound.tobytes(), (name, n)
            assert (out["occ"] == (~miss).astype(np.uint8)).all(), (name, n)
            for k, plane in enumerate(("position", "normal", "albedo", "emission")):
                want = ans.surface[k][:n]
                assert out[plane].tobytes() == want.tobytes(), (name, n, plane, np.abs(out[plane] - want).max())
                assert (out[plane][miss].view(np.uint32) == 0).all()   # +0.0, not -0.0 and not the canary
            runs += 1
        # a single plane: the others are not touched (they do not exist: a store to one is the sanitizer's to find)
        out, _ = _host_run(exe, str(tmp_path / f"{name}_one"), 65, ans, tables, n_inst, frames, True, which=2)
        assert out["normal"].tobytes() == ans.surface[1][:65].tobytes() and out["position"].size == 0
    assert runs == 15
