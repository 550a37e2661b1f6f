"""pt_radiance_device without a GPU (include/pt_api.h): the header against the ctypes mirror; the recipes of
tests/test_radiance_device.py held against the oracle alone, so that a recipe which drifts cannot hide a kernel that returns `env` everywhere;
the Python path loop of tests/radiance_cases.py against orc.Scene.render_frame; and the per-lane bodies of the generate and resolve kernels
(csrc/radiance_device_kernel.h) compiled for the host (tests/radiance_device_host.cpp), run as a program -- plain and under the address and
undefined-behaviour sanitizers -- bit for bit against numpy."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import radiance_cases as rcs
import trace_device_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MISS = tc.MISS
NEW_SYMBOLS = ["pt_radiance_desc_default", "pt_radiance_device", "pt_radiance_workspace_bytes"]
FIELDS = ["d_rays6", "d_seeds", "d_radiance", "d_moment2", "tmin", "tmax", "env", "spp", "max_depth", "frame", "index_base", "flags", "extend",
          "chunk_rays", "reserved"]


def test_radiance_desc_layout_defaults_and_symbols(pt, tmp_path):
    """sizeof / offsetof of pt_radiance_desc by gcc from the header == the ctypes mirror (96 bytes); the flags' values; the defaults; the new
    names in API_SYMBOLS and in the library; PT_API_VERSION stays 6; NULL handles are PT_ERR_INVALID_ARG."""
    src = tmp_path / "rd_layout.c"
    vals = ["sizeof(pt_radiance_desc)"] + ["offsetof(pt_radiance_desc, %s)" % f for f in FIELDS] + \
           ["(size_t)PT_RADIANCE_NEE", "(size_t)PT_RADIANCE_ACCUMULATE", "(size_t)PT_RADIANCE_DEFAULT_CHUNK_SLOTS", "(size_t)PT_API_VERSION"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("' + "%zu " * len(vals) + '\\n",' + ", ".join(vals) + ");return 0;}\n")
    exe = tmp_path / "rd_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    D = pt.RadianceDesc
    assert got[0] == 96 and got[0] == C.sizeof(D), got
    assert got[1:1 + len(FIELDS)] == [getattr(D, f).offset for f in FIELDS], got
    assert got[1 + len(FIELDS):1 + len(FIELDS) + 2] == [1, 2] and got[-1] == 6, got
    slots = got[-2]
    assert slots >= 1 << 18 and slots & (slots - 1) == 0, slots     # a power of two of the sweep 2^18 .. 2^24
    assert slots <= 1 << 24, slots
    assert (pt.RADIANCE_NEE, pt.RADIANCE_ACCUMULATE) == (1, 2)
    for name in NEW_SYMBOLS:
        assert name in pt.API_SYMBOLS and hasattr(pt.lib_amd(), name), name
    d = pt.radiance_default_desc()   # (touches no device)
    assert [getattr(d, f) for f in FIELDS[:4]] == [None] * 4
    assert (f32(d.tmin), f32(d.tmax), [f32(x) for x in d.env]) == (f32(0.001), f32(10000.0), [f32(0.7), f32(0.6), f32(0.5)])
    assert (d.spp, d.max_depth, d.frame, d.index_base, d.flags, d.extend, d.chunk_rays, list(d.reserved)) == (32, 8, 0, 0, 0, pt.EXTEND_AUTO, 0, [0] * 4)
    lib = pt.lib_amd()
    lib.pt_radiance_desc_default(None)                                        # (a NULL is ignored)
    assert lib.pt_radiance_device(None, C.byref(d), 0, None) == 1
    assert lib.pt_radiance_workspace_bytes(None, None) == 1
    assert callable(getattr(pt.Scene, "radiance_device", None)) and callable(getattr(pt.Scene, "radiance_tensors", None))
    assert callable(getattr(pt.Context, "radiance_workspace_bytes", None))


def test_camera_recipe_and_path_loop_against_the_oracle_alone(orc, cornell_arrays):
    """box, 24x16, default camera, depth 4, frame 0: 215 of 384 pixels hit, the NEE frame differs from the plain one on more than half of the
    pixels, 921 plain and 1379 NEE rays; and the Python path loop started from primary_ray's ray and advanced seed equals render_frame on
    every pixel, with the same ray count"""
    cam = rcs.box_camera(orc, cornell_arrays)
    assert cam.n == 384 and int(cam.hit.sum()) == 215, int(cam.hit.sum())
    assert cam.nee_differs > 0.5, cam.nee_differs
    assert (cam.n_rays[0], cam.n_rays[1]) == (921, 1379), cam.n_rays
    osc = orc.Scene(*cornell_arrays)
    got, traced = np.zeros((cam.n, 3), f32), 0
    for i in range(cam.n):
        got[i], t = rcs.path_radiance(orc, osc, cam.rays[i], cam.seeds[i, 0], cam.depth)
        traced += t
    assert got.tobytes() == cam.want[0].tobytes(), np.abs(got - cam.want[0]).max()
    assert traced == 921


def test_free_ray_recipe_against_the_oracle_alone(orc, cornell_arrays):
    """the first 257 rows of make_rays() at 3 samples, depth 4, hashed seeds: all 771 seeds distinct, most rays end with a non-zero mean, many
    have samples that differ from one another, 1965 rays"""
    fr = rcs.box_free(orc, cornell_arrays)
    assert fr.seeds.shape == (257, 3) and len(np.unique(fr.seeds)) == 771
    nonzero = float((fr.mean != 0).any(1).mean())
    differ = float(((fr.c[:, 0] != fr.c[:, 1]) | (fr.c[:, 0] != fr.c[:, 2])).any(1).mean())
    assert nonzero >= 0.8, nonzero      # measured 0.875
    assert differ >= 0.4, differ        # measured 0.49
    assert int(fr.traced.sum()) == 1965, int(fr.traced.sum())
    # the seed rule itself, on values worked by hand from common.glsl:21-31: pcg2d(0, 1)
    a, b = orc.pcg2d(0, 1)
    assert rcs.hashed_seed(0, 0, 3, 0) == (a + b) & 0xFFFFFFFF
    assert rcs.hashed_seed(5, 2, 3, 4) == sum(orc.pcg2d(5, 2 + 12 + 1)) & 0xFFFFFFFF
    assert rcs.hashed_seed(5, 0, 3, -1) == sum(orc.pcg2d(5, (0 - 3 + 1) & 0xFFFFFFFF)) & 0xFFFFFFFF


def test_instance_and_soup_recipes_against_the_oracle_alone(orc, cornell_arrays):
    """the three-instance scene through the same camera: every instance is hit (28 / 114 / 31 first hits); the 4 096-triangle soup at 16x16:
    a first-hit share between 0.2 and 0.6 and an NEE frame that differs on more than a fifth of the pixels"""
    inst = rcs.inst_camera(orc, cornell_arrays)
    ids, counts = np.unique(inst.first["inst"][inst.hit], return_counts=True)
    assert list(ids) == [0, 1, 2] and list(counts) == [28, 114, 31], (ids, counts)
    soup = rcs.soup_camera(orc)
    share = float(soup.hit.mean())
    assert 0.2 < share < 0.6, share                      # measured 0.33
    assert soup.nee_differs > 0.2, soup.nee_differs      # measured 0.32


def _write(d, name, a):
    np.ascontiguousarray(a).tofile(os.path.join(d, name))


def _host_run(exe, d, rays, spp, frame, index_base, accumulate, seeds, color, old, old2, first=0):
    os.makedirs(d, exist_ok=True)
    m = len(rays)
    _write(d, "par", np.asarray([m, spp, frame & 0xFFFFFFFF, index_base, int(accumulate), int(seeds is not None), int(old2 is not None), first], np.uint32))
    _write(d, "rays6", rays)
    _write(d, "seeds", seeds if seeds is not None else np.zeros(0, np.uint32))
    _write(d, "color", color)
    _write(d, "radiance", old)
    _write(d, "moment2", old2 if old2 is not None else np.zeros(0, f32))
    subprocess.check_call([exe, d])
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    return {"color": rd("o_color", f32).reshape(-1, 4), "qid": rd("o_qid", np.uint32).reshape(-1, 2), "qstate": rd("o_qstate", np.uint32).reshape(-1, 4),
            "rayA": rd("o_rayA", f32).reshape(-1, 4), "rayB": rd("o_rayB", f32).reshape(-1, 2), "radiance": rd("o_radiance", f32).reshape(-1, 3),
            "moment2": rd("o_moment2", f32).reshape(-1, 3)}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_kernel_bodies_on_the_host(tmp_path, sanitize):
    """The generate and resolve bodies as a program at n = 1, 63, 64, 65, 257 with spp = 1 and 3: the queue records and seeds (with d_seeds,
    hashed, hashed with index_base = 100 and a chunk that starts at ray 7 of its call), the ordered reduce, the second moment, the blend at
    frames 0, 1 and 5, and a frame-0 run over NaN-filled old values that produces no NaN -- bit for bit against numpy."""
    exe = str(tmp_path / "radiance_device_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "radiance_device_host.cpp")])
    all_rays = tc.make_rays()
    rng = np.random.default_rng(5)
    nan = np.float32("nan")
    runs = 0
    for n in rcs.PREFIXES:
        for spp in (1, 3):
            rays = all_rays[:n]
            # accumulators as rounds might leave them: sample-major [spp][n], values whose sums round (so the order of the adds shows)
            c = (rng.uniform(0, 4, (n, spp, 3)) ** 3).astype(f32)
            color = np.zeros((spp, n, 4), f32)
            color[:, :, :3] = c.transpose(1, 0, 2)
            color[:, :, 3] = nan                                  # (the pad is never read into a result)
            mean, m2 = rcs.ordered_mean(c)
            given = rng.integers(0, 1 << 32, (n, spp), dtype=np.uint64).astype(np.uint32)
            old, old2 = rng.uniform(0, 2, (n, 3)).astype(f32), rng.uniform(0, 9, (n, 3)).astype(f32)
            nans = np.full((n, 3), nan, f32)
            # (seeds, frame, index_base, first, accumulate, old, old2)
            cases = [(given, 0, 0, 0, False, nans, nans), (None, 0, 0, 0, False, nans, None), (None, 2, 100, 7, False, nans, nans),
                     (None, 0, 0, 0, True, nans, nans), (given, 1, 0, 0, True, old, old2), (None, 5, 0, 0, True, old, None), (None, -1, 0, 0, False, nans, None)]
            for k, (seeds, frame, base, first, acc, o, o2) in enumerate(cases):
                out = _host_run(exe, str(tmp_path / f"{n}_{spp}_{k}"), rays, spp, frame, base, acc, seeds, color, o, o2, first)
                what = (n, spp, k)
                slot = np.arange(n * spp, dtype=np.uint32)
                want_seed = seeds if seeds is not None else rcs.hashed_seeds(n, spp, frame, base + first)
                assert (out["color"].view(np.uint32) == 0).all(), what                       # +0.0 in all four words of every slot
                assert (out["qid"][:, 0] == slot).all() and (out["qid"][:, 1] == 0).all(), what
                assert (out["qstate"][:, 0] == want_seed.T.reshape(-1)).all(), what               # slot = s * n + r
                assert (out["qstate"][:, 1:] == f32(1.0).view(np.uint32)).all(), what
                assert out["rayA"].tobytes() == np.tile(rays[:, :4], (spp, 1)).tobytes() and out["rayB"].tobytes() == np.tile(rays[:, 4:], (spp, 1)).tobytes(), what
                want = rcs.blend(o, mean, frame) if acc else mean
                assert out["radiance"].tobytes() == want.tobytes(), what
                if o2 is not None:
                    want2 = rcs.blend(o2, m2, frame) if acc else m2
                    assert out["moment2"].tobytes() == want2.tobytes(), what
                    assert not np.isnan(out["moment2"]).any()
                else:
                    assert out["moment2"].size == 0
                assert not np.isnan(out["radiance"]).any(), what
                runs += 1
    assert runs == 70
    # the order of the adds is visible in these sums: a reversed reduce gives other bits somewhere
    c = (np.random.default_rng(5).uniform(0, 4, (257, 3, 3)) ** 3).astype(f32)
    assert rcs.ordered_mean(c)[0].tobytes() != rcs.ordered_mean(c[:, ::-1])[0].tobytes()
