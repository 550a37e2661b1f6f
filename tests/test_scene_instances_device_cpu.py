"""pt_scene_set_instances_device without a GPU (include/pt_api.h): the declaration against the header and the Python
names; the tensor wrapper's refusals that need no device; and the per-thread statements of scene_instances.hip's kernels
(csrc/scene_instances_kernel.h) compiled for the host (tests/scene_instances_host.cpp) and run as a program -- plain and under the address
and undefined-behaviour sanitizers -- against literal restatements of ptb_set_instances' loop and ptb_ensure_inst_lights' loop."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_device_call_and_the_package_binds_it(pt, tmp_path):
    """The prototype as the header states it; PT_API_VERSION stays 6 (by gcc from the header); the name in API_SYMBOLS and in the library;
    Scene.set_instances_device / set_instances_tensor exist; a NULL handle is PT_ERR_INVALID_ARG."""
    txt = open(os.path.join(REPO, "include", "pt_api.h")).read()
    assert re.search(r"pt_status\s+pt_scene_set_instances_device\s*\(\s*pt_scene\s*\*\s*scene\s*,\s*const void\s*\*\s*d_xforms3x4\s*,\s*uint32_t n\s*\)", txt)
    src = tmp_path / "si_consts.c"
    src.write_text('#include <stdio.h>\n#include "pt_api.h"\nint main(void){printf("%d\\n", (int)PT_API_VERSION);return 0;}\n')
    exe = tmp_path / "si_consts"
    subprocess.check_call([shutil.which("gcc") or "gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["6"]
    L = pt.lib_amd()
    assert "pt_scene_set_instances_device" in pt.API_SYMBOLS and hasattr(L, "pt_scene_set_instances_device")
    for name in ("set_instances_device", "set_instances_tensor"):
        assert callable(getattr(pt.Scene, name, None)), name
    a = np.zeros(12, np.float32)   # (never read: the NULL handle is refused first)
    assert L.pt_scene_set_instances_device(None, a.ctypes.data, 1) == 1
    assert L.pt_scene_set_instances_device(None, None, 0) == 1


def test_tensor_wrapper_refuses_before_a_device_is_touched(pt):
    """Not a tensor, not float32, an element count that is no multiple of 12, a CPU tensor: ValueError with no context and no scene behind
    the call (one that got as far as the library would fail otherwise)."""
    import torch
    x = torch.zeros(24, dtype=torch.float32)
    scene = pt.Scene.__new__(pt.Scene)     # no handle, no context: nothing a library call could work on
    scene.h, scene.ctx = None, None
    for bad in (x.numpy(), [0.0] * 12, None, x.double(), x.half(), x.int(), x[:23], x[:13], torch.zeros((2, 3, 3)), x, x.reshape(2, 3, 4),
                torch.zeros(0, dtype=torch.float32)):       # the last three: well formed, but CPU tensors
        with pytest.raises(ValueError):
            scene.set_instances_tensor(bad)
    scene.h = None   # (Scene.__del__ closes nothing)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_scene_instances_statements_on_the_host(tmp_path, sanitize):
    """tests/scene_instances_host.cpp as a stand-alone program, every array at exactly its size.  The check/invert statement at 1, 63, 64, 65
    and 257 instances (rotations times scales over six decades, shears, mirrored matrices, -0.0 entries): the 96-byte records, the kept copy
    and the verdict word against the parent's host loop, for the good set and for every refusal -- a NaN at the first, a middle and the last
    instance, +Inf, -Inf, a zero row, two equal rows, a scale of 1e-39, and a NaN at instance 7 beside a singular matrix at instance 3
    (which reports "singular").  The light statement and the fold at 0, 1, 64, 65 and 257 (instance, emitter) copies with areas over six
    decades: records, cdf words and the total, bit for bit the host loop's (a pairwise sum of the same terms differs somewhere)."""
    exe = str(tmp_path / "scene_instances_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off", "-Wno-unknown-pragmas"] + flags +
                          ["-I", os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "csrc"), "-I", os.path.join(REPO, "tests"), "-o", exe,
                           os.path.join(REPO, "tests", "scene_instances_host.cpp")])
    run = subprocess.run([exe], text=True, capture_output=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    for group in ("check/invert ok (44 refusals)", "lights ok", "scene_instances_host: all ok"):
        assert any(ln.startswith(group) for ln in lines), (group, run.stdout)
