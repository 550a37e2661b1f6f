"""PT_TRACE_FUSED / PT_TRACE_AUTO without a GPU (include/pt_api.h): the two constants against the header and the Python
names; the big ray set of tests/test_trace_fused.py held against the oracle alone; and the per-lane statements of k_trace_fused that touch the
caller's arrays (csrc/trace_fused_kernel.h) compiled for the host (tests/trace_fused_host.cpp), run as a program -- plain and under the address
and undefined-behaviour sanitizers -- bit for bit against the numpy tables of tc.kernel_tables and the oracle's records."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import trace_device_cases as tc
import trace_fused_cases as tfc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
MISS = tc.MISS
PLANES = ("position", "normal", "albedo", "emission")


def test_trace_fused_constants_and_names(pt, tmp_path):
    """PT_TRACE_FUSED = 4 and PT_TRACE_AUTO = 8 by gcc from the header (PT_TRACE_ASYNC stays 1, the value 2 stays free, the desc stays 104 bytes,
    PT_API_VERSION stays 6); the Python names; Scene.trace_tensors takes form= and defaults to the queues."""
    src = tmp_path / "tf_consts.c"
    vals = ["(size_t)PT_TRACE_ASYNC", "(size_t)PT_TRACE_FUSED", "(size_t)PT_TRACE_AUTO", "sizeof(pt_trace_desc)", "(size_t)PT_API_VERSION"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("' + "%zu " * len(vals) + '\\n",' + ", ".join(vals) + ");return 0;}\n")
    exe = tmp_path / "tf_consts"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [1, 4, 8, 104, 6], got
    assert (pt.TRACE_ASYNC, pt.TRACE_FUSED, pt.TRACE_AUTO) == (1, 4, 8)
    assert inspect.signature(pt.Scene.trace_tensors).parameters["form"].default == "queues"


def test_big_ray_set_against_the_oracle_alone(orc, cornell_arrays):
    """tc.make_rays(200 001) on the box, from the oracle alone: hit share strictly within (0.3, 0.8), occluded share under the cycled bounds
    strictly within (0.2, 0.7), and every one of the four bounds sees both answers.
    Measured: hit share 0.6121; occluded share 0.3847; per bound 1e-4 / 0.5 / 2 / 10000: 5 of 50 001, 16 487, 29 690 and 30 756 of 50 000 -- the
    any-hit answers at tmin = 1e-5 (trace_fused_cases.BIG_ANY_TMIN: under the default tmin of 0.001 the bound 1e-4 lies below tmin and occludes
    nothing, 0 of 50 001, so it could never see both answers); under the uniform bound 0.5 at the default tmin: 0.3275."""
    a = tfc.big_answers(orc, cornell_arrays)
    assert len(a.rays) == tfc.BIG_N == 200_001
    hit, occ, per = tfc.big_shares(a)
    assert 0.3 < hit < 0.8, hit
    assert 0.2 < occ < 0.7, occ
    for k, (share, count) in enumerate(per):
        assert 0 < round(share * count) < count, (float(tc.BOUNDS[k]), share, count)
    assert 0.05 < a.occ_uniform.mean() < 0.95


def _write(d, name, a):
    np.ascontiguousarray(a).tofile(os.path.join(d, name))


def _host_run(exe, d, n, ans, tables, with_dtmax, want_hits=True, which=15):
    """one run of the host program over the first n rays of `ans`; -> its output arrays"""
    os.makedirs(d, exist_ok=True)
    h = ans.hits[:n]
    # what the walk holds at a ray's end: (leaf position | MISS, t, V, W, det) with V = u, W = v, det = 1, so that fdiv gives the oracle's u and v
    best = np.zeros(n, np.dtype([("pos", np.uint32), ("t", f32), ("V", f32), ("W", f32), ("det", f32)]))
    best["pos"], best["t"], best["V"], best["W"], best["det"] = h["prim"], h["t"], h["u"], h["v"], 1.0   # (leaf order = primitive order)
    n_tris = len(tables["faces"]) // 6
    tmax = f32(ans.uniform_bound)
    _write(d, "par", np.asarray([n, n_tris, int(with_dtmax), int(want_hits), which, tmax.view(np.uint32)], np.uint32))
    _write(d, "rays6", np.concatenate([np.asarray([123.0], f32), ans.rays[:n].reshape(-1)]))   # rows start one float into the allocation
    _write(d, "dtmax", ans.bounds[:n] if with_dtmax else np.zeros(0, f32))
    _write(d, "best", best)
    for name in ("tri4", "rec64", "faces"):
        _write(d, name, tables[name])
    subprocess.check_call([exe, d])
    rd = lambda name, dt: np.fromfile(os.path.join(d, name), dt)
    out = {"rays": rd("o_rays", f32).reshape(n, 6), "bound": rd("o_bound", f32), "occ": rd("o_occ", np.uint8), "hits": rd("o_hits", np.uint8)}
    for k, name in enumerate(PLANES):
        a = rd("o_" + name, f32)
        out[name] = a.reshape(n, 3) if (which >> k) & 1 else a
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_fused_statements_on_the_host(pt, orc, cornell_arrays, tmp_path, sanitize):
    """tf_row / tf_bound / tf_record / tf_hit_row / tf_surface / tf_occluded as a program at n = 1, 63, 64, 65, 257 on the box, every array at
    exactly its size and the rays only 4-byte aligned: the rows come back as they went in, the bound is the ray's or the uniform one, the pt_hit
    rows are the oracle's records byte for byte (prim from tri4's .w; MISS, zeros, MISS behind a miss), the planes equal orc.Scene.shade_hit and
    `faces` with +0.0 behind a miss, occluded is "position != MISS"; d_hits absent beside the planes, and one plane alone."""
    exe = str(tmp_path / "trace_fused_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "trace_fused_host.cpp")])
    v, i, f = cornell_arrays
    ans = tfc.box_answers(orc, cornell_arrays)
    tables = tc.kernel_tables(v, i, f)
    assert ans.hits.dtype.itemsize == 20
    runs = 0
    for n in tc.PREFIXES[:5]:
        with_dtmax = n % 2 == 1
        out = _host_run(exe, str(tmp_path / f"box_{n}"), n, ans, tables, with_dtmax)
        miss = ans.hits["prim"][:n] == MISS
        assert out["rays"].tobytes() == ans.rays[:n].tobytes(), n
        want_bound = ans.bounds[:n] if with_dtmax else np.full(n, ans.uniform_bound, f32)
        assert out["bound"].tobytes() == want_bound.tobytes(), n
        assert out["hits"].tobytes() == ans.hits[:n].tobytes(), n
        assert (out["occ"] == (~miss).astype(np.uint8)).all(), n
        for k, plane in enumerate(PLANES):
            want = ans.surface[k][:n]
            assert out[plane].tobytes() == want.tobytes(), (n, plane, np.abs(out[plane] - want).max())
            assert (out[plane][miss].view(np.uint32) == 0).all()   # +0.0, not -0.0 and not the canary
        runs += 1
    assert runs == 5 and 0.3 <= ans.hit_share(257) <= 0.9
    # d_hits NULL beside the planes, and a single plane: what was not named does not exist (a store to it is the sanitizer's to find)
    out = _host_run(exe, str(tmp_path / "box_no_hits"), 65, ans, tables, True, want_hits=False)
    assert out["hits"].size == 0 and out["position"].tobytes() == ans.surface[0][:65].tobytes()
    for k, plane in enumerate(PLANES):
        out = _host_run(exe, str(tmp_path / f"box_only_{plane}"), 65, ans, tables, False, want_hits=False, which=1 << k)
        assert out[plane].tobytes() == ans.surface[k][:65].tobytes(), plane
        assert all(out[p].size == 0 for p in PLANES if p != plane)
