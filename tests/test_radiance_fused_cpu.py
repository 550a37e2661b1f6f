"""The single-kernel form of pt_radiance_device without a GPU (include/pt_api.h): the two new flags in the header and the
wrapper, and the index arithmetic of the kernel's slot hand-out (csrc/radiance_device_kernel.h rdf_*) compiled for the host
(tests/radiance_fused_host.cpp) and run as a program -- plain and under the address and undefined-behaviour sanitizers -- against numpy."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import radiance_cases as rcs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_in_the_header_and_the_wrapper(pt, tmp_path):
    """PT_RADIANCE_FUSED = 8, PT_RADIANCE_AUTO = 16 beside NEE = 1 and ACCUMULATE = 2 (4 stays no flag); pt_radiance_desc keeps its 96 bytes and
    PT_API_VERSION stays 6; the Python constants; radiance_tensors knows `form` and refuses an unknown one before it touches a device"""
    src = tmp_path / "rf_layout.c"
    vals = ["sizeof(pt_radiance_desc)", "(size_t)PT_API_VERSION", "(size_t)PT_RADIANCE_NEE", "(size_t)PT_RADIANCE_ACCUMULATE", "(size_t)PT_RADIANCE_FUSED",
            "(size_t)PT_RADIANCE_AUTO", "offsetof(pt_radiance_desc, reserved)"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_api.h"\nint main(void){printf("' + "%zu " * len(vals) + '\\n",' + ", ".join(vals) + ");return 0;}\n")
    exe = tmp_path / "rf_layout"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [96, 6, 1, 2, 8, 16, 80], got
    assert C.sizeof(pt.RadianceDesc) == 96 and pt.RadianceDesc.reserved.offset == 80 and pt.RadianceDesc.reserved.size == 16
    assert (pt.RADIANCE_NEE, pt.RADIANCE_ACCUMULATE, pt.RADIANCE_FUSED, pt.RADIANCE_AUTO) == (1, 2, 8, 16)

    class NotATensor:   # (the form is looked at first: nothing of the rays is)
        pass
    import inspect
    assert inspect.signature(pt.Scene.radiance_tensors).parameters["form"].default == "wavefront"
    with pytest.raises(ValueError, match="form"):
        pt.Scene.radiance_tensors(None, NotATensor(), form="persistent")


def _run(exe, d, m, spp, frame, index_base, seeds, first, order):
    os.makedirs(d, exist_ok=True)
    np.asarray([m, spp, frame & 0xFFFFFFFF, index_base, int(seeds is not None), first, order], np.uint32).tofile(os.path.join(d, "par"))
    (np.ascontiguousarray(seeds, np.uint32) if seeds is not None else np.zeros(0, np.uint32)).tofile(os.path.join(d, "seeds"))
    subprocess.check_call([exe, d])
    return {k: np.fromfile(os.path.join(d, "o_" + k), np.uint32) for k in ("count", "s", "r", "seed", "meta")}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_hand_out_arithmetic_on_the_host(tmp_path, sanitize):
    """m in {1, 63, 64, 65, 257, 4097} x spp in {1, 3}, the eight part counters drained by draws in three arbitrary orders: the launch hands out
    m * spp rounded up to 64 positions, every slot below m * spp exactly once, none at or beyond it (those positions are masked, and they are
    exactly the rounding's excess); slot -> (s, r) is (slot // m, slot % m); the seed is rd_generate's for that (ray, sample): given seeds
    [r * spp + s], hashed seeds with index_base, a non-zero first ray and frames 0, 2 and -1."""
    exe = str(tmp_path / "radiance_fused_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "radiance_fused_host.cpp")])
    rng = np.random.default_rng(25)
    runs = 0
    for m in (1, 63, 64, 65, 257, 4097):
        for spp in (1, 3):
            live = m * spp
            ns = (live + 63) // 64 * 64
            given = rng.integers(0, 1 << 32, (m, spp), dtype=np.uint64).astype(np.uint32)
            slot = np.arange(live, dtype=np.int64)
            # (seeds, frame, index_base, first, order of the draws)
            cases = [(given, 0, 0, 0, 1), (None, 0, 0, 0, 2), (None, 2, 100, 7, 3), (None, -1, 0, 4097 * 5, 1), (given, 1, 9, 64, 2)]
            hashed = {}
            for k, (seeds, frame, base, first, order) in enumerate(cases):
                out = _run(exe, str(tmp_path / f"{m}_{spp}_{k}"), m, spp, frame, base, seeds, first, order)
                what = (m, spp, k)
                assert list(out["meta"][:5]) == [ns, live, ns, ns - live, 0], (what, out["meta"])   # launch slots, live, positions, masked, parts left
                assert out["count"].shape == (ns,) and (out["count"] == 1).all(), what             # (the masked positions ARE the slots >= live)
                assert (out["s"] == slot // m).all() and (out["r"] == slot % m).all(), what
                if seeds is not None:
                    want = seeds[out["r"], out["s"]]
                else:
                    key = (frame, base + first)
                    if m <= 257:
                        hashed[key] = rcs.hashed_seeds(m, spp, frame, base + first)
                        want = hashed[key][out["r"], out["s"]]
                    else:   # (4097 rays: the rule on the first and last 130 rays, the oracle's pcg2d being a Python loop)
                        sel = np.r_[0:130, m - 130:m]
                        tab = np.asarray([[rcs.hashed_seed(int(i) + base + first, s, spp, frame) for s in range(spp)] for i in sel], np.uint32)
                        pick = np.isin(out["r"], sel)
                        assert pick.sum() == 260 * spp
                        pos = np.searchsorted(sel, out["r"][pick])
                        assert (out["seed"][pick] == tab[pos, out["s"][pick]]).all(), what
                        want = None
                if want is not None:
                    assert (out["seed"] == want).all(), what
                runs += 1
    assert runs == 60
