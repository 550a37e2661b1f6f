"""pt_radiance_device on one MI355X, as one JSON record under profiles/ (DESIGN.md section 24).

Scenes: the Cornell box (LDS kernels) and the 1 M-triangle soup (8-wide tree).  Rays: the 1920 x 1080 pinhole rays of pt_params_default's camera
(pixel centres, no jitter), SPP samples each with hashed seeds, depth 8, plain estimator.  Every shape is warmed; 7 repetitions, median with
min .. max:
  chunks   device_ms of the call with chunk_rays = 2^18 .. 2^24 slots / SPP: what PT_RADIANCE_DEFAULT_CHUNK_SLOTS is chosen from (the smallest
           value whose time lies within the spread of the fastest)
  rate     wall time and rays/s of the call at the default chunk against pt_render with PT_PIPELINE_WAVEFRONT at the same size, spp and depth by
           the library named with --parent-lib (the parent commit's build; without the option: this library, and the record says so), the two
           alternated in one loop; `ratio` = this call's rays/s over pt_render's
  kernels  only where the ratio is below 0.5: the kernels' total times from ONE `rocprofv3 --kernel-trace --stats` run of a child that repeats
           the call (without rocprofv3: "not measured")
Usage: python scripts/probe_radiance_device.py [--parent-lib PATH] [--reps 7] [--spp 8] [--small] [--out profiles/radiance_device_probe.json]"""
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
f32 = np.float32
DEPTH = 8


def summary(x, unit="ms"):
    return {"median_" + unit: round(statistics.median(x), 4), "min_" + unit: round(min(x), 4), "max_" + unit: round(max(x), 4), "n": len(x)}


def camera_rays(w, h, origin=(0.0, -1.0, 5.0), target=(0.0, -1.0, 2.0)):
    """raygen.rgen:51-57 without the jitter: through the 2 x 2 square around `target`"""
    px, py = np.meshgrid(np.arange(w, dtype=f32) + f32(0.5), np.arange(h, dtype=f32) + f32(0.5))
    d = np.stack([px / f32(w) * 2 - 1 + target[0] - origin[0], py / f32(h) * 2 - 1 + target[1] - origin[1], np.full_like(px, target[2] - origin[2])], -1).reshape(-1, 3).astype(f32)
    d /= np.sqrt((d * d).sum(1, dtype=f32))[:, None]
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(np.asarray(origin, f32), d.shape), d], 1), f32)


class ParentRender:
    """pt_render of another build of the library (the parent commit's), through its own context, scene and film in this process"""

    def __init__(self, pt, path, arrays, w, h, spp):
        L = self.L = C.CDLL(path)
        self.pt = pt
        vp = C.c_void_p
        L.pt_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        L.pt_scene_create.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(vp)]
        L.pt_film_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.pt_params_default.argtypes = [C.POINTER(pt.Params)]; L.pt_params_default.restype = None
        L.pt_render.argtypes = [vp, vp, C.POINTER(pt.Params)]
        L.pt_get_stats.argtypes = [vp, C.POINTER(pt.Stats)]
        L.pt_reset_stats.argtypes = [vp]
        for fn in (L.pt_scene_destroy, L.pt_film_destroy, L.pt_ctx_destroy):
            fn.argtypes = [vp]; fn.restype = None
        v, i, f = arrays
        self.ctx, self.scene, self.film = vp(), vp(), vp()
        assert L.pt_ctx_create(0, None, C.byref(self.ctx)) == 0
        assert L.pt_scene_create(self.ctx, v.ctypes.data, v.size // 3, i.ctypes.data, i.size // 3, f.ctypes.data, C.byref(self.scene)) == 0
        assert L.pt_film_create(self.ctx, w, h, C.byref(self.film)) == 0
        self.p = pt.Params()
        L.pt_params_default(C.byref(self.p))
        self.p.width, self.p.height, self.p.spp_per_frame, self.p.max_depth, self.p.frame, self.p.frame_count = w, h, spp, DEPTH, 0, 1
        self.p.pipeline = pt.PIPELINE_WAVEFRONT

    def render(self):
        """-> (wall ms, rays)"""
        self.L.pt_reset_stats(self.ctx)
        t0 = time.perf_counter()
        assert self.L.pt_render(self.scene, self.film, C.byref(self.p)) == 0
        ms = (time.perf_counter() - t0) * 1e3
        st = self.pt.Stats()
        self.L.pt_get_stats(self.ctx, C.byref(st))
        return ms, int(st.rays)

    def close(self):
        self.L.pt_film_destroy(self.film); self.L.pt_scene_destroy(self.scene); self.L.pt_ctx_destroy(self.ctx)


def scenes(pt, small):
    v, i, f = pt.load_obj(pt.ASSET_CORNELL)
    yield "cornell", (v, i, f)
    sv, si, sf = pt.make_soup((1 << 14) if small else (1 << 20), 1)
    yield "soup_1m", (np.ascontiguousarray(sv, f32).reshape(-1), np.ascontiguousarray(si, np.uint32).reshape(-1), np.ascontiguousarray(sf, f32).reshape(-1))


def child(reps, parent_lib, small, spp, trace_only):
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    dev = torch.device("cuda:0")
    ctx = pt.Context(0)
    ctx.set_tuning(mem_budget_mb=0)   # (the largest chunks of the sweep are 2.2 GB of workspace)
    w, h = (480, 270) if small else (1920, 1080)
    rays = camera_rays(w, h)
    n = len(rays)
    rec = {"width": w, "height": h, "spp": spp, "max_depth": DEPTH, "rays": n, "slots": n * spp, "chunks": {}, "rate": {}}
    t = torch.from_numpy(rays).to(dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for name, arrays in scenes(pt, small):
        scene = pt.Scene(ctx, *arrays)
        kw = dict(spp=spp, max_depth=DEPTH)
        if trace_only:
            for _ in range(1 + reps):
                scene.radiance_device(n, t.data_ptr(), out.data_ptr(), **kw)
            scene.close()
            continue
        sweep = {}
        for lg in (range(14, 21) if small else range(18, 25)):
            xs = []
            for k in range(2 + reps):   # (the first grows the workspace, the second warms)
                ms = scene.radiance_device(n, t.data_ptr(), out.data_ptr(), chunk_rays=max(64, (1 << lg) // spp), **kw)
                if k >= 2:
                    xs.append(ms)
            sweep[f"2^{lg}"] = summary(xs)
        rec["chunks"][name] = sweep
        parent = ParentRender(pt, parent_lib or os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "libpt_amd.so"), arrays, w, h, spp)
        m = {"radiance_wall": [], "radiance_device": [], "render_wall": []}
        rays_new = rays_old = 0
        for k in range(2 + reps):
            ctx.reset_stats()
            t0 = time.perf_counter()
            dms = scene.radiance_device(n, t.data_ptr(), out.data_ptr(), **kw)
            wall = (time.perf_counter() - t0) * 1e3
            rays_new = int(ctx.stats().rays)
            rms, rays_old = parent.render()
            if k >= 2:
                m["radiance_wall"].append(wall); m["radiance_device"].append(dms); m["render_wall"].append(rms)
        r = {k: summary(v) for k, v in m.items()}
        new_rate, old_rate = rays_new / r["radiance_wall"]["median_ms"] / 1e6, rays_old / r["render_wall"]["median_ms"] / 1e6
        r.update(rays_radiance=rays_new, rays_render=rays_old, grays_per_s_radiance=round(new_rate, 3), grays_per_s_render=round(old_rate, 3),
                 ratio=round(new_rate / old_rate, 3), extend_variant=int(ctx.stats().extend_variant), mean_radiance=[round(float(x), 5) for x in out.mean(0).cpu()])
        rec["rate"][name] = r
        parent.close()
        scene.close()
    rec["workspace_bytes"] = ctx.radiance_workspace_bytes()
    print(json.dumps(rec))
    ctx.close()


def kernel_stats(reps, small, spp):
    """the kernels' total times of a child that repeats the call on both scenes, from one rocprofv3 run; or a string saying why not"""
    if not shutil.which("rocprofv3"):
        return "rocprofv3 not found: not measured"
    d = tempfile.mkdtemp(prefix="rd_trace_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "--trace-only",
                            "--reps", str(reps), "--spp", str(spp)] + (["--small"] if small else []), capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return f"the traced child failed ({r.returncode}): not measured"
        tot = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                nm = row["Kernel_Name"].split("(")[0][-60:]
                tot[nm] = tot.get(nm, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
        return {k: round(v, 3) for k, v in sorted(tot.items(), key=lambda kv: -kv[1])[:8]} or "no dispatch in the trace: not measured"
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--parent-lib", help="libpt_amd.so of the parent commit for the pt_render side")
    ap.add_argument("--small", action="store_true", help="a quick pass over small shapes (a check of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "radiance_device_probe.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.parent_lib, a.small, a.spp, a.trace_only)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--spp", str(a.spp)] + (["--small"] if a.small else []) +
                       (["--parent-lib", a.parent_lib] if a.parent_lib else []), capture_output=True, text=True, timeout=1100)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode}): {r.stderr[-3000:]}")
    rec = {"probe": "radiance_device", "reps": a.reps, "small": a.small,
           "render_library": "the parent commit's build" if a.parent_lib else "THIS library (no --parent-lib given)"}
    rec.update(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    slow = [k for k, v in rec["rate"].items() if v["ratio"] < 0.5]
    rec["kernels_total_ms"] = kernel_stats(a.reps, a.small, a.spp) if slow else "no scene below half of pt_render's rate: not measured"
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
