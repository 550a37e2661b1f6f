"""The single-kernel form of pt_trace_device (PT_TRACE_FUSED) against the queue form AS BUILT FROM THE PARENT COMMIT, on one MI355X, as one JSON
record under profiles/ (DESIGN.md section 26).  Sibling of scripts/probe_trace_device.py, whose shapes these are.

Scene: the Cornell box.  Rays: the 1920 x 1080 pinhole rays of pt_params_default's camera repeated to 2^20 and 2^24 rays, in image order
("coherent") and as a shuffled copy.  Kinds of query: `hits` (CLOSEST into d_hits), `surface` (CLOSEST into d_hits and the four planes), `any`
(PT_TRACE_ANY, one bound for all).  Per shape and kind the libraries are alternated in one loop -- the parent library's pt_trace_device without
form flags, this library's with PT_TRACE_FUSED, and, with --variant-lib, a second build of this tree (the other epilogue placement,
-DPT_TRACE_FUSED_DEFER=1) with PT_TRACE_FUSED -- two warm-up passes, then --reps (7) timed ones: device_ms of the call (its own events), median
with min .. max.  Once per shape and kind the outputs are compared byte for byte.  `fused_wins`: the single-kernel form's MAX lies below the
parent's MIN.  `auto` per kind: true only if fused_wins on EVERY shape of that kind -- what PT_TRACE_AUTO may take (trace_device.hip
TD_AUTO_TAKES_FUSED).
Usage: python scripts/probe_trace_fused.py --parent-lib PATH [--variant-lib PATH] [--reps 7] [--small] [--out profiles/trace_fused_probe.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
from probe_trace_device import camera_rays, sized, summary  # noqa: E402

KINDS = ("hits", "surface", "any")


class OtherLib:
    """pt_trace_device of another build of the library through its own context and scene in this process; rays and outputs are the caller's
    device pointers"""

    def __init__(self, pt, path, arrays):
        L = self.L = C.CDLL(path)
        self.pt = pt
        vp = C.c_void_p
        L.pt_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        L.pt_scene_create.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(vp)]
        L.pt_trace_desc_default.argtypes = [C.POINTER(pt.TraceDesc)]; L.pt_trace_desc_default.restype = None
        L.pt_trace_device.argtypes = [vp, C.POINTER(pt.TraceDesc), C.c_uint64, C.POINTER(C.c_float)]
        for fn in (L.pt_scene_destroy, L.pt_ctx_destroy):
            fn.argtypes = [vp]; fn.restype = None
        v, i, f = arrays
        self.ctx, self.scene = vp(), vp()
        assert L.pt_ctx_create(0, None, C.byref(self.ctx)) == 0
        assert L.pt_scene_create(self.ctx, v.ctypes.data, v.size // 3, i.ctypes.data, i.size // 3, f.ctypes.data, C.byref(self.scene)) == 0

    def call(self, n, rays_ptr, out, kind, flags):
        d = self.pt.TraceDesc()
        self.L.pt_trace_desc_default(C.byref(d))
        d.d_rays6, d.flags = rays_ptr, flags
        fill(d, out, kind, self.pt)
        ms = C.c_float(0.0)
        assert self.L.pt_trace_device(self.scene, C.byref(d), n, C.byref(ms)) == 0
        return ms.value

    def close(self):
        self.L.pt_scene_destroy(self.scene); self.L.pt_ctx_destroy(self.ctx)


def fill(d, out, kind, pt):
    """the output pointers of a kind of query; out: {"hits", "occ", "planes"} tensors"""
    if kind == "any":
        d.mode, d.d_occluded = pt.TRACE_ANY, out["occ"].data_ptr()
        return
    d.mode, d.d_hits = pt.TRACE_CLOSEST, out["hits"].data_ptr()
    if kind == "surface":
        d.d_position, d.d_normal, d.d_albedo, d.d_emission = [p.data_ptr() for p in out["planes"]]


def child(reps, parent_lib, variant_lib, small):
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    dev = torch.device("cuda:0")
    ctx = pt.Context(0)
    arrays = pt.load_obj(pt.ASSET_CORNELL)
    scene = pt.Scene(ctx, *arrays)
    parent = OtherLib(pt, parent_lib, arrays)
    variant = OtherLib(pt, variant_lib, arrays) if variant_lib else None
    cam = camera_rays((0.0, -1.0, 5.0), (0.0, -1.0, 2.0))
    sizes = [1 << 14, 1 << 16] if small else [1 << 20, 1 << 24]
    rec = {"sizes": sizes, "shapes": {}}
    auto = {k: True for k in KINDS}

    def outputs(n):
        return {"hits": torch.empty((n, 5), dtype=torch.int32, device=dev), "occ": torch.empty(n, dtype=torch.uint8, device=dev),
                "planes": [torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(4)]}

    def this_call(n, t, out, kind):
        d = pt.trace_default_desc()
        d.d_rays6, d.flags = t.data_ptr(), pt.TRACE_FUSED
        fill(d, out, kind, pt)
        ms = C.c_float(0.0)
        ctx._check(pt.lib_amd().pt_trace_device(scene.h, C.byref(d), n, C.byref(ms)))
        return ms.value

    def equal(a, b, kind):
        if kind == "any":
            return bool(torch.equal(a["occ"], b["occ"]))
        return bool(torch.equal(a["hits"], b["hits"])) and (kind == "hits" or all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a["planes"], b["planes"])))

    for n in sizes:
        for order in ("coherent", "shuffled"):
            t = torch.from_numpy(sized(cam, n, order == "shuffled")).to(dev)
            out_old, out_new = outputs(n), outputs(n)
            torch.cuda.synchronize()
            for kind in KINDS:
                m = {"queues_parent": [], "fused": [], "fused_variant": []}
                for k in range(2 + reps):   # two warm-up passes, then the measured ones, the libraries alternated
                    a = parent.call(n, t.data_ptr(), out_old, kind, 0)
                    b = this_call(n, t, out_new, kind)
                    c = variant.call(n, t.data_ptr(), out_new, kind, pt.TRACE_FUSED) if variant else 0.0
                    if k >= 2:
                        m["queues_parent"].append(a); m["fused"].append(b); m["fused_variant"].append(c)
                same = equal(out_old, out_new, kind)   # (out_new: the variant's where there is one -- it ran last; this library's is compared below)
                this_call(n, t, out_new, kind)
                same = same and equal(out_old, out_new, kind)
                if not variant:
                    del m["fused_variant"]
                r = {k: summary(v) for k, v in m.items()}
                wins = bool(r["fused"]["max_ms"] < r["queues_parent"]["min_ms"])
                r.update(bytes_equal=same, parent_over_fused=round(r["queues_parent"]["median_ms"] / r["fused"]["median_ms"], 3), fused_wins=wins,
                         mrays_per_s_parent=round(n / r["queues_parent"]["median_ms"] / 1e3, 1), mrays_per_s_fused=round(n / r["fused"]["median_ms"] / 1e3, 1))
                if variant:
                    r["fused_over_variant"] = round(r["fused"]["median_ms"] / r["fused_variant"]["median_ms"], 3)
                auto[kind] = auto[kind] and wins and same
                rec["shapes"].setdefault(f"cornell/{n}/{order}", {})[kind] = r
            del t, out_old, out_new
    rec["auto"] = auto
    rec["workspace_bytes_fused_only_context"] = ctx.trace_workspace_bytes()
    print(json.dumps(rec))
    parent.close()
    if variant:
        variant.close()
    scene.close(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", help="libpt_amd.so of the parent commit: the yardstick (required for a measurement)")
    ap.add_argument("--variant-lib", help="a second build of this tree (the other epilogue placement), measured in the same loop")
    ap.add_argument("--small", action="store_true", help="a quick pass over small shapes (a check of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trace_fused_probe.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.parent_lib, a.variant_lib, a.small)
    if not a.parent_lib:
        raise SystemExit("--parent-lib: the queue form is measured as built from the parent commit, never from this tree")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--parent-lib", a.parent_lib] +
                       (["--variant-lib", a.variant_lib] if a.variant_lib else []) + (["--small"] if a.small else []), capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode}): {r.stderr[-3000:]}")
    rec = {"probe": "trace_fused", "reps": a.reps, "small": a.small, "yardstick": "pt_trace_device (queue form) of the parent commit's build",
           "variant": "this tree built with -DPT_TRACE_FUSED_DEFER=1" if a.variant_lib else None}
    rec.update(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
