"""pt_scene_create_device / pt_scene_update_device without a GPU (include/pt_api.h): the two declarations against the
header and the Python names; the refusals that need no device; and the per-thread statements of scene_device.hip's kernels
(csrc/scene_device_kernel.h) compiled for the host (tests/scene_device_host.cpp) and run as a program -- plain and under the address and
undefined-behaviour sanitizers -- against restatements of push_emitter, its caller's loop, find_fan_pairs and the index loop."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_device_calls_and_the_package_binds_them(pt, tmp_path):
    """Both prototypes as the header states them; PT_API_VERSION stays 6 (by gcc from the header); the names in API_SYMBOLS and in the
    library; Scene.update_device / update_tensors / from_tensors exist; NULL handles are PT_ERR_INVALID_ARG."""
    txt = open(os.path.join(REPO, "include", "pt_api.h")).read()
    v = r"\s*const void\s*\*\s*"
    assert re.search(r"pt_status\s+pt_scene_create_device\s*\(\s*pt_ctx\s*\*\s*ctx\s*," + v + r"d_vertices\s*,\s*uint32_t n_verts\s*," + v +
                     r"d_indices\s*,\s*uint32_t n_tris\s*," + v + r"d_faces\s*,\s*pt_scene\s*\*\*\s*out\s*\)", txt)
    assert re.search(r"pt_status\s+pt_scene_update_device\s*\(\s*pt_scene\s*\*\s*scene\s*," + v + r"d_vertices\s*,\s*uint32_t n_verts\s*," + v +
                     r"d_indices\s*,\s*uint32_t n_tris\s*,\s*uint32_t mode\s*\)", txt)
    src = tmp_path / "sd_consts.c"
    src.write_text('#include <stdio.h>\n#include "pt_api.h"\nint main(void){printf("%d %d %d\\n", (int)PT_API_VERSION, (int)PT_SCENE_UPDATE_REFIT, '
                   '(int)PT_SCENE_UPDATE_REBUILD);return 0;}\n')
    exe = tmp_path / "sd_consts"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["6", "0", "1"]
    L = pt.lib_amd()
    for name in ("pt_scene_create_device", "pt_scene_update_device"):
        assert name in pt.API_SYMBOLS and hasattr(L, name), name
    for name in ("update_device", "update_tensors", "from_tensors"):
        assert callable(getattr(pt.Scene, name, None)), name
    a = np.zeros(16, np.float32)   # (never read: the NULL handle is refused first)
    import ctypes as C
    out = C.c_void_p(123)
    assert L.pt_scene_create_device(None, a.ctypes.data, 1, a.ctypes.data, 1, a.ctypes.data, C.byref(out)) == 1
    assert L.pt_scene_update_device(None, a.ctypes.data, 1, a.ctypes.data, 1, 0) == 1


def test_tensor_wrappers_refuse_before_a_device_is_touched(pt):
    """Wrong dtype, sizes that are no multiples of 3 and 6, faces that do not match the indices, CPU tensors: ValueError from update_tensors and
    from_tensors alike, with no context and no scene behind them (a call that got as far as the library would fail otherwise)."""
    import torch
    v = torch.zeros(9, dtype=torch.float32)
    i = torch.arange(3, dtype=torch.int32)
    f = torch.zeros(6, dtype=torch.float32)
    scene = pt.Scene.__new__(pt.Scene)     # no handle, no context: nothing a library call could work on
    scene.h, scene.ctx = None, None
    bad = [(v.double(), i), (v, i.long()), (v, i.float()), (v[:8], i), (v, torch.arange(4, dtype=torch.int32)), (v.numpy(), i), (v, i)]   # the last: CPU tensors
    for vv, ii in bad:
        with pytest.raises(ValueError):
            scene.update_tensors(vv, ii)
    for vv, ii, ff in [(v, i, f.double()), (v, i, f[:5]), (v, i, torch.zeros(12)), (v.half(), i, f), (v, i, f)]:
        with pytest.raises(ValueError):
            pt.Scene.from_tensors(None, vv, ii, ff)
    scene.h = None   # (Scene.__del__ closes nothing)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_scene_device_statements_on_the_host(tmp_path, sanitize):
    """tests/scene_device_host.cpp as a stand-alone program, every array at exactly its size: emitter records and the running cdf at 0, 1, 2,
    63, 64, 65, 257 and 4097 emitters with areas over six decades (bit for bit the host loop's; a pairwise sum of the same terms differs
    somewhere, so the fold's order shows); discovery on Ke rows of +0, -0.0, a denormal, a negative value, a NaN and all zero; the pair flags
    on quads with shared indices, duplicated coordinates, -0.0 against +0.0 at the shared vertex, at the last triangle and in overlapping
    fans; the index check with the bad index first, in the middle and last, at n_verts and 0xFFFFFFFF, and none bad, at 1, 21, 22 and 2049
    triangles."""
    exe = str(tmp_path / "scene_device_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off", "-Wno-unknown-pragmas"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "scene_device_host.cpp")])
    run = subprocess.run([exe], text=True, capture_output=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    for group in ("emitters ok", "discovery ok", "pairs ok", "index check ok", "scene_device_host: all ok"):
        assert any(ln.startswith(group) for ln in lines), (group, run.stdout)
