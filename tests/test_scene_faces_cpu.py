"""pt_scene_set_faces / pt_scene_set_faces_device / pt_scene_read_faces without a GPU (include/pt_api.h): the three
declarations against the header and the Python names; the refusals that need no device; and the per-thread statements of scene_faces.hip's
kernel (csrc/scene_faces_kernel.h) compiled for the host (tests/scene_faces_host.cpp) and run as a program -- plain and under the address and
undefined-behaviour sanitizers -- against a restatement of k_pack's lines."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_three_calls_and_the_package_binds_them(pt, tmp_path):
    """The prototypes as the header states them; a C program including pt_api.h compiles and PT_API_VERSION stays 6; the names in API_SYMBOLS
    and in the library; the four Scene methods exist; NULL handles and NULL arrays are PT_ERR_INVALID_ARG."""
    txt = open(os.path.join(REPO, "include", "pt_api.h")).read()
    assert re.search(r"pt_status\s+pt_scene_set_faces\s*\(\s*pt_scene\s*\*\s*scene\s*,\s*const float\s*\*\s*faces\s*,\s*uint32_t n_tris\s*\)", txt)
    assert re.search(r"pt_status\s+pt_scene_set_faces_device\s*\(\s*pt_scene\s*\*\s*scene\s*,\s*const void\s*\*\s*d_faces\s*,\s*uint32_t n_tris\s*\)", txt)
    assert re.search(r"pt_status\s+pt_scene_read_faces\s*\(\s*const pt_scene\s*\*\s*scene\s*,\s*float\s*\*\s*faces\s*\)", txt)
    src = tmp_path / "sf_consts.c"
    src.write_text('#include <stdio.h>\n#include "pt_api.h"\n'
                   'int main(void){pt_status (*a)(pt_scene *, const float *, uint32_t) = pt_scene_set_faces;\n'
                   'pt_status (*b)(pt_scene *, const void *, uint32_t) = pt_scene_set_faces_device;\n'
                   'pt_status (*c)(const pt_scene *, float *) = pt_scene_read_faces;\n'
                   'printf("%d %d\\n", (int)PT_API_VERSION, (int)(a && b && c));return 0;}\n')
    obj = tmp_path / "sf_consts.o"     # (compiled, not linked: the prototypes are the header's, the symbols the library's)
    subprocess.check_call([shutil.which("gcc") or "gcc", "-Wall", "-Werror", "-Wno-address", "-c", "-I", os.path.join(REPO, "include"), "-o", str(obj), str(src)])
    ver = tmp_path / "sf_ver.c"
    ver.write_text('#include <stdio.h>\n#include "pt_api.h"\nint main(void){printf("%d\\n", (int)PT_API_VERSION);return 0;}\n')
    exe = tmp_path / "sf_ver"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(ver)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["6"]
    L = pt.lib_amd()
    for name in ("pt_scene_set_faces", "pt_scene_set_faces_device", "pt_scene_read_faces"):
        assert name in pt.API_SYMBOLS and hasattr(L, name), name
    for name in ("set_faces", "set_faces_device", "set_faces_tensor", "read_faces"):
        assert callable(getattr(pt.Scene, name, None)), name
    a = np.zeros(12, np.float32)   # (never read: the NULL handle is refused first)
    assert L.pt_scene_set_faces(None, a.ctypes.data, 2) == 1
    assert L.pt_scene_set_faces_device(None, a.ctypes.data, 2) == 1
    assert L.pt_scene_read_faces(None, a.ctypes.data) == 1


def test_tensor_wrapper_refuses_before_a_device_is_touched(pt):
    """A CPU tensor, a wrong dtype, a non-contiguous tensor, a wrong length, something that is no tensor: ValueError from set_faces_tensor
    with no context and no scene behind it (a call that got as far as the library would fail otherwise)."""
    import torch
    scene = pt.Scene.__new__(pt.Scene)     # no handle, no context: nothing a library call could work on
    scene.h, scene.ctx = None, None
    scene._nt = 4                          # (what Scene._n_tris() would have asked the scene's record for)
    f = torch.zeros(24, dtype=torch.float32)
    wide = torch.zeros((24, 2), dtype=torch.float32)
    for bad in (f, f.double(), f.half(), f.int(), wide[:, 0], f[:23], f[:18], torch.zeros(30), f.numpy(), None):
        with pytest.raises(ValueError):
            scene.set_faces_tensor(bad)
    with pytest.raises(ValueError):
        scene.set_faces(np.zeros(7, np.float32))     # no 6 floats per triangle
    scene.h = None   # (Scene.__del__ closes nothing)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_scene_faces_statements_on_the_host(tmp_path, sanitize):
    """tests/scene_faces_host.cpp as a stand-alone program: sf_set_position<HAS8> over n = 1, 63, 64, 65 and 257 positions under shuffled leaf
    orders, random faces plus one row each of 0, -0.0, a denormal, 1e-38, a negative, 3e38, +inf and NaN in Kd and in Ke, on canary-filled
    tables: the material words equal a restatement of k_pack's lines bit for bit, the flag and sf_emits agree with sd_is_emitter, and every
    word the call must not write (normal words, shade4[3p+2].yzw, shade64's rows 0..2, everything past the arrays) keeps its canary."""
    exe = str(tmp_path / "scene_faces_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off", "-Wno-unknown-pragmas"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "scene_faces_host.cpp")])
    run = subprocess.run([exe], text=True, capture_output=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    for group in ("predicate ok", "material words ok", "canaries ok", "scene_faces_host: all ok"):
        assert any(ln.startswith(group) for ln in lines), (group, run.stdout)
