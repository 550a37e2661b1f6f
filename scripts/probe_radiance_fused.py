"""The single-kernel form of pt_radiance_device (PT_RADIANCE_FUSED) against the wavefront form AS BUILT FROM THE PARENT COMMIT, on one MI355X, as
one JSON record under profiles/ (DESIGN.md section 25).  Sibling of scripts/probe_radiance_device.py.

Scene: the Cornell box.  Depth 8, hashed seeds, both estimators.  Shapes:
  camera      the 1920 x 1080 pinhole rays of pt_params_default's camera (pixel centres), 8 samples -- section 24's shape
  incoherent  as many rays with origins uniform in the box and directions uniform on the sphere, 8 samples
  small       2^16 of the incoherent rays, 1 sample
Per shape and estimator the two forms are alternated in one loop -- the parent library's pt_radiance_device without form flags, this library's
with PT_RADIANCE_FUSED -- two warm-up passes, then --reps (7) timed ones: device ms (the call's own events), wall ms, Grays/s from the median
wall time and pt_stats.rays; the outputs of the two are compared bit for bit.  `fused_wins`: the fused median lies below the parent's median by
more than the parent's own min .. max spread, on both clocks.  `auto` per estimator: true only if fused_wins on EVERY shape -- what
PT_RADIANCE_AUTO may take (radiance_device.hip RD_AUTO_TAKES_FUSED).
  chunks      device ms of the fused form on the camera shape, plain, with chunk_rays = 2^18 .. 2^24 slots / 8
  kernels     only where the fused form loses on the incoherent shape: the kernels' total times of ONE `rocprofv3 --kernel-trace --stats` run,
              in a run of its own, of a child that repeats that call
Usage: python scripts/probe_radiance_fused.py --parent-lib PATH [--reps 7] [--small] [--out profiles/radiance_fused_probe.json]"""
import argparse
import csv
import ctypes as C
import glob
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
from probe_radiance_device import camera_rays, summary  # noqa: E402

f32 = np.float32
DEPTH = 8


class ParentRadiance:
    """pt_radiance_device of another build of the library (the parent commit's) through its own context and scene in this process; the rays and
    the outputs are the caller's device pointers"""

    def __init__(self, pt, path, arrays):
        L = self.L = C.CDLL(path)
        self.pt = pt
        vp = C.c_void_p
        L.pt_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        L.pt_scene_create.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(vp)]
        L.pt_radiance_desc_default.argtypes = [C.POINTER(pt.RadianceDesc)]; L.pt_radiance_desc_default.restype = None
        L.pt_radiance_device.argtypes = [vp, C.POINTER(pt.RadianceDesc), C.c_uint64, C.POINTER(C.c_float)]
        L.pt_get_stats.argtypes = [vp, C.POINTER(pt.Stats)]
        L.pt_reset_stats.argtypes = [vp]
        for fn in (L.pt_scene_destroy, L.pt_ctx_destroy):
            fn.argtypes = [vp]; fn.restype = None
        v, i, f = arrays
        self.ctx, self.scene = vp(), vp()
        assert L.pt_ctx_create(0, None, C.byref(self.ctx)) == 0
        assert L.pt_scene_create(self.ctx, v.ctypes.data, v.size // 3, i.ctypes.data, i.size // 3, f.ctypes.data, C.byref(self.scene)) == 0

    def call(self, n, rays_ptr, out_ptr, spp, flags):
        """-> (device ms, wall ms, rays)"""
        d = self.pt.RadianceDesc()
        self.L.pt_radiance_desc_default(C.byref(d))
        d.d_rays6, d.d_radiance, d.spp, d.max_depth, d.flags = rays_ptr, out_ptr, spp, DEPTH, flags
        ms = C.c_float(0.0)
        self.L.pt_reset_stats(self.ctx)
        t0 = time.perf_counter()
        assert self.L.pt_radiance_device(self.scene, C.byref(d), n, C.byref(ms)) == 0
        wall = (time.perf_counter() - t0) * 1e3
        st = self.pt.Stats()
        self.L.pt_get_stats(self.ctx, C.byref(st))
        return ms.value, wall, int(st.rays)

    def close(self):
        self.L.pt_scene_destroy(self.scene); self.L.pt_ctx_destroy(self.ctx)


def incoherent_rays(arrays, n, seed=25):
    v = np.asarray(arrays[0], f32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    rng = np.random.default_rng(seed)
    o = (lo + (hi - lo) * rng.uniform(0.02, 0.98, (n, 3))).astype(f32)
    d = rng.standard_normal((n, 3)).astype(f32)
    d /= np.sqrt((d * d).sum(1, dtype=f32))[:, None]
    return np.ascontiguousarray(np.concatenate([o, d], 1), f32)


def shapes(arrays, small):
    w, h = (480, 270) if small else (1920, 1080)
    cam = camera_rays(w, h)
    inc = incoherent_rays(arrays, len(cam))
    return [("camera", cam, 8), ("incoherent", inc, 8), ("small", inc[:(1 << 12) if small else (1 << 16)], 1)]


def child(reps, parent_lib, small, trace_only):
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    dev = torch.device("cuda:0")
    ctx = pt.Context(0)
    arrays = pt.load_obj(pt.ASSET_CORNELL)
    scene = pt.Scene(ctx, *arrays)
    rec = {"max_depth": DEPTH, "shapes": {}, "chunks": {}}
    if trace_only:
        _, rays, spp = shapes(arrays, small)[1]
        t = torch.from_numpy(rays).to(dev)
        out = torch.empty((len(rays), 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for _ in range(1 + reps):
            scene.radiance_device(len(rays), t.data_ptr(), out.data_ptr(), spp=spp, max_depth=DEPTH, flags=pt.RADIANCE_FUSED)
        scene.close(); ctx.close()
        return
    parent = ParentRadiance(pt, parent_lib, arrays)
    auto = {"plain": True, "nee": True}
    for name, rays, spp in shapes(arrays, small):
        n = len(rays)
        t = torch.from_numpy(rays).to(dev)
        out_new = torch.empty((n, 3), dtype=torch.float32, device=dev)
        out_old = torch.empty((n, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for est, nee in (("plain", 0), ("nee", pt.RADIANCE_NEE)):
            m = {"wavefront_parent_device": [], "wavefront_parent_wall": [], "fused_device": [], "fused_wall": []}
            rays_new = rays_old = 0
            for k in range(2 + reps):
                dms_o, wall_o, rays_old = parent.call(n, t.data_ptr(), out_old.data_ptr(), spp, nee)
                ctx.reset_stats()
                t0 = time.perf_counter()
                dms_n = scene.radiance_device(n, t.data_ptr(), out_new.data_ptr(), spp=spp, max_depth=DEPTH, flags=nee | pt.RADIANCE_FUSED)
                wall_n = (time.perf_counter() - t0) * 1e3
                rays_new = int(ctx.stats().rays)
                if k >= 2:
                    m["wavefront_parent_device"].append(dms_o); m["wavefront_parent_wall"].append(wall_o)
                    m["fused_device"].append(dms_n); m["fused_wall"].append(wall_n)
            r = {k: summary(v) for k, v in m.items()}
            wins = {}
            for clock in ("device", "wall"):
                o, f = r["wavefront_parent_" + clock], r["fused_" + clock]
                wins[clock] = bool(f["median_ms"] < o["median_ms"] - (o["max_ms"] - o["min_ms"]))
            r.update(rays=n, spp=spp, rays_traced_parent=rays_old, rays_traced_fused=rays_new, bits_equal=bool(torch.equal(out_new, out_old)),
                     grays_per_s_parent_wall=round(rays_old / r["wavefront_parent_wall"]["median_ms"] / 1e6, 3),
                     grays_per_s_fused_wall=round(rays_new / r["fused_wall"]["median_ms"] / 1e6, 3),
                     grays_per_s_parent_device=round(rays_old / r["wavefront_parent_device"]["median_ms"] / 1e6, 3),
                     grays_per_s_fused_device=round(rays_new / r["fused_device"]["median_ms"] / 1e6, 3),
                     fused_wins=wins["device"] and wins["wall"], fused_wins_by_clock=wins)
            auto[est] = auto[est] and r["fused_wins"]
            rec["shapes"].setdefault(name, {})[est] = r
        if name == "camera":
            for lg in (range(14, 21) if small else range(18, 25)):
                xs = []
                for k in range(2 + reps):   # (the first grows the workspace, the second warms)
                    ms = scene.radiance_device(n, t.data_ptr(), out_new.data_ptr(), spp=spp, max_depth=DEPTH, flags=pt.RADIANCE_FUSED, chunk_rays=max(64, (1 << lg) // spp))
                    if k >= 2:
                        xs.append(ms)
                rec["chunks"][f"2^{lg}"] = summary(xs)
    rec["auto"] = auto
    rec["workspace_bytes_fused_only_context"] = ctx.radiance_workspace_bytes()
    print(json.dumps(rec))
    parent.close(); scene.close(); ctx.close()


def kernel_stats(reps, small):
    if not shutil.which("rocprofv3"):
        return "rocprofv3 not found: not measured"
    d = tempfile.mkdtemp(prefix="rf_trace_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "--trace-only",
                            "--reps", str(reps)] + (["--small"] if small else []), capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            return f"the traced child failed ({r.returncode}): not measured"
        tot = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                nm = row["Kernel_Name"].split("(")[0][-60:]
                e = tot.setdefault(nm, [0.0, 0])
                e[0] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
                e[1] += 1
        return {k: {"total_ms": round(v[0], 3), "calls": v[1]} for k, v in sorted(tot.items(), key=lambda kv: -kv[1][0])[:6]} or "no dispatch in the trace: not measured"
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", help="libpt_amd.so of the parent commit: the yardstick (required for a measurement)")
    ap.add_argument("--small", action="store_true", help="a quick pass over small shapes (a check of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "radiance_fused_probe.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.parent_lib, a.small, a.trace_only)
    if not a.parent_lib:
        raise SystemExit("--parent-lib: the wavefront form is measured as built from the parent commit, never from this tree")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--parent-lib", a.parent_lib] + (["--small"] if a.small else []),
                       capture_output=True, text=True, timeout=500)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode}): {r.stderr[-3000:]}")
    rec = {"probe": "radiance_fused", "reps": a.reps, "small": a.small, "yardstick": "pt_radiance_device (wavefront form) of the parent commit's build"}
    rec.update(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    loses = [e for e, v in rec["shapes"]["incoherent"].items() if not v["fused_wins"]]
    rec["kernels_incoherent_fused"] = kernel_stats(3, a.small) if loses else "the fused form wins on the incoherent shape: not measured"
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
