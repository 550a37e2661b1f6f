"""pt_trace_device on one MI355X, as one JSON record under profiles/ (DESIGN.md section 22).

Scenes: the Cornell box (LDS kernel) and the 1 M-triangle soup (8-wide tree).  Rays: the 1920 x 1080 pinhole rays of pt_params_default's camera
(pixel centres, no jitter), repeated to 2^20 and 2^24 rays, in image order ("coherent") and as a shuffled copy.  Per shape, after a
warm-up of everything, 7 repetitions, median with min .. max:
  closest      device_ms of pt_trace_device CLOSEST with d_hits (first kernel to last), and the extend kernels' share of it (pt_stats.ms_extend)
  surface      the same with the four surface planes as well
  any          device_ms of PT_TRACE_ANY with one bound for all (d_tmax NULL), same rays
  host_trace   wall time of pt_trace on the same rays in host memory, by the library named with --parent-lib (the parent commit's build;
               without the option: this library, and the record says so), alternated with `closest` in one loop
  chunks       `closest` at 2^24 coherent rays with chunk_rays 2^16 .. 2^22
  copy         torch's device-to-device copy of 24 / 20 / 48 bytes per ray by device events: the yardstick for the pack, hits and surface kernels
Kernel times per dispatch come from ONE `rocprofv3 --kernel-trace -f csv` run of a child that repeats the 2^20-ray CLOSEST + surface and ANY
calls on both scenes (one chunk each): k_trace_pack, k_hits_to_api, k_trace_surface, k_trace_occluded by name.  Without rocprofv3 that part is
"not measured".
Usage: python scripts/probe_trace_device.py [--parent-lib PATH] [--reps 7] [--small] [--out profiles/trace_device_probe.json]"""
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
W, H = 1920, 1080
f32 = np.float32


def summary(x, unit="ms"):
    return {"median_" + unit: round(statistics.median(x), 4), "min_" + unit: round(min(x), 4), "max_" + unit: round(max(x), 4), "n": len(x)}


def camera_rays(origin, target):
    """raygen.rgen:51-57 without the jitter: through the 2 x 2 square around `target`"""
    px, py = np.meshgrid(np.arange(W, dtype=f32) + f32(0.5), np.arange(H, dtype=f32) + f32(0.5))
    d = np.stack([px / f32(W) * 2 - 1 + target[0] - origin[0], py / f32(H) * 2 - 1 + target[1] - origin[1], np.full_like(px, target[2] - origin[2])], -1).reshape(-1, 3).astype(f32)
    d /= np.sqrt((d * d).sum(1, dtype=f32))[:, None]
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(np.asarray(origin, f32), d.shape), d], 1), f32)


def sized(rays, n, shuffle):
    r = np.ascontiguousarray(np.tile(rays, ((n + len(rays) - 1) // len(rays), 1))[:n])
    return np.ascontiguousarray(r[np.random.default_rng(5).permutation(n)]) if shuffle else r


class ParentLib:
    """pt_trace of another build of the library (the parent commit's), through its own context and scene in this process"""

    def __init__(self, path, v, i, f):
        L = self.L = C.CDLL(path)
        vp = C.c_void_p
        L.pt_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
        L.pt_scene_create.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.POINTER(vp)]
        L.pt_trace.argtypes = [vp, vp, C.c_uint32, C.c_float, C.c_float, C.c_uint32, vp]
        L.pt_scene_destroy.argtypes = [vp]; L.pt_scene_destroy.restype = None
        L.pt_ctx_destroy.argtypes = [vp]; L.pt_ctx_destroy.restype = None
        self.ctx, self.scene = vp(), vp()
        assert L.pt_ctx_create(0, None, C.byref(self.ctx)) == 0
        assert L.pt_scene_create(self.ctx, v.ctypes.data, v.size // 3, i.ctypes.data, i.size // 3, f.ctypes.data, C.byref(self.scene)) == 0

    def trace_wall_ms(self, rays, hits):
        t0 = time.perf_counter()
        assert self.L.pt_trace(self.scene, rays.ctypes.data, len(rays), 0.001, 10000.0, 0, hits.ctypes.data) == 0
        return (time.perf_counter() - t0) * 1e3

    def close(self):
        self.L.pt_scene_destroy(self.scene); self.L.pt_ctx_destroy(self.ctx)


def scenes(pt, small):
    v, i, f = pt.load_obj(pt.ASSET_CORNELL)
    cam = camera_rays((0.0, -1.0, 5.0), (0.0, -1.0, 2.0))   # pt_params_default's camera; the soup fills the box's volume
    yield "cornell", (v, i, f), cam
    sv, si, sf = pt.make_soup((1 << 14) if small else (1 << 20), 1)
    yield "soup_1m", (np.ascontiguousarray(sv, f32).reshape(-1), np.ascontiguousarray(si, np.uint32).reshape(-1), np.ascontiguousarray(sf, f32).reshape(-1)), cam


def child(reps, parent_lib, small, trace_only):
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    dev = torch.device("cuda:0")
    ctx = pt.Context(0)
    sizes = [1 << 14, 1 << 16] if small else [1 << 20, 1 << 24]
    rec = {"sizes": sizes, "shapes": {}, "chunks": {}, "copy": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy_ms(nbytes):
        a, b = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = []
        for k in range(2 + reps):
            ev[0].record(); b.copy_(a); ev[1].record()
            torch.cuda.synchronize()
            if k >= 2:
                out.append(ev[0].elapsed_time(ev[1]))
        return out

    for name, arrays, cam in scenes(pt, small):
        scene = pt.Scene(ctx, *arrays)
        parent = None if trace_only else ParentLib(parent_lib or os.path.join(REPO, "single-file-vulkan-pathtracing_amd", "libpt_amd.so"), *arrays)
        for n in sizes[:1] if trace_only else sizes:
            for order in ("coherent",) if trace_only else ("coherent", "shuffled"):
                rays = sized(cam, n, order == "shuffled")
                t = torch.from_numpy(rays).to(dev)
                hits = torch.empty((n, 5), dtype=torch.int32, device=dev)
                occ = torch.empty(n, dtype=torch.uint8, device=dev)
                planes = [torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(4)]
                host_hits = np.zeros(n, pt.HIT_DTYPE)
                torch.cuda.synchronize()
                sp = dict(position_ptr=planes[0].data_ptr(), normal_ptr=planes[1].data_ptr(), albedo_ptr=planes[2].data_ptr(), emission_ptr=planes[3].data_ptr())
                m = {"closest": [], "extend_share": [], "surface": [], "any": [], "host_trace_wall": []}
                for k in range(2 + reps):   # two warm-up rounds, then the measured ones
                    ctx.reset_stats()
                    ms = scene.trace_device(n, t.data_ptr(), hits_ptr=hits.data_ptr())
                    share = ctx.stats().ms_extend / ms
                    wall = parent.trace_wall_ms(rays, host_hits) if parent else 0.0
                    ms_s = scene.trace_device(n, t.data_ptr(), hits_ptr=hits.data_ptr(), **sp)
                    ms_a = scene.trace_device(n, t.data_ptr(), occluded_ptr=occ.data_ptr(), mode=pt.TRACE_ANY)
                    if k >= 2:
                        m["closest"].append(ms); m["extend_share"].append(share); m["surface"].append(ms_s); m["any"].append(ms_a); m["host_trace_wall"].append(wall)
                if parent:
                    same = bool(hits.cpu().numpy().tobytes() == host_hits.tobytes())
                    hit_share = float((host_hits["prim"] != pt.MISS).mean())
                    r = {k: summary(v, "share" if k == "extend_share" else "ms") for k, v in m.items()}
                    r.update(hits_equal_host_trace=same, hit_share=round(hit_share, 4), occluded_share=round(float(occ.float().mean()), 4),
                             host_over_device=round(r["host_trace_wall"]["median_ms"] / r["closest"]["median_ms"], 1),
                             any_over_closest=round(r["any"]["median_ms"] / r["closest"]["median_ms"], 3), mrays_per_s=round(n / r["closest"]["median_ms"] / 1e3, 1))
                    rec["shapes"][f"{name}/{n}/{order}"] = r
                if n == sizes[-1] and order == "coherent" and not trace_only:
                    sweep = {}
                    for lg in (range(10, 15) if small else range(16, 23)):
                        xs = []
                        for k in range(1 + reps):
                            ms = scene.trace_device(n, t.data_ptr(), hits_ptr=hits.data_ptr(), chunk_rays=1 << lg)
                            if k >= 1:
                                xs.append(ms)
                        sweep[f"2^{lg}"] = summary(xs)
                    rec["chunks"][name] = sweep
                del t, hits, occ, planes
        if parent:
            parent.close()
        scene.close()
    if not trace_only:
        for label, per_ray in (("pack_24B", 24), ("hits_20B", 20), ("surface_48B", 48)):
            rec["copy"][label] = summary(copy_ms(per_ray * sizes[0]))
        rec["workspace_bytes"] = ctx.trace_workspace_bytes()
    print(json.dumps(rec))
    ctx.close()


def kernel_trace(reps, small):
    """per-dispatch kernel times of the new kernels from one rocprofv3 run, or a string saying why not"""
    if not shutil.which("rocprofv3"):
        return "rocprofv3 not found: not measured"
    d = tempfile.mkdtemp(prefix="td_trace_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "--trace-only", "--reps", str(reps)] +
                           (["--small"] if small else []), capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return f"the traced child failed ({r.returncode}): not measured"
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3, row["Kernel_Name"]))
        rows.sort()
        # the scenes come one after the other: the first half of a kernel's dispatches is the box, the second the soup
        out = {}
        for key in ("k_trace_pack", "k_hits_to_api", "k_trace_surface", "k_trace_occluded"):
            us = [u for _, u, nm in rows if key in nm]
            half = len(us) // 2
            if half >= 3:
                out[key] = {"cornell": summary(us[:half][-reps:], "us"), "soup_1m": summary(us[half:][-reps:], "us")}
        return out or "no dispatch of the new kernels in the trace: not measured"
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", help="libpt_amd.so of the parent commit for the pt_trace side")
    ap.add_argument("--small", action="store_true", help="a quick pass over small shapes (a check of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trace_device_probe.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.parent_lib, a.small, a.trace_only)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--small"] if a.small else []) +
                       (["--parent-lib", a.parent_lib] if a.parent_lib else []), capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode}): {r.stderr[-3000:]}")
    rec = {"probe": "trace_device", "reps": a.reps, "small": a.small, "rays": f"{W} x {H} pinhole rays repeated to size; shuffled: a permutation of them",
           "host_trace_library": "the parent commit's build" if a.parent_lib else "THIS library (no --parent-lib given)"}
    rec.update(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    rec["kernels_us_at_%d_rays" % rec["sizes"][0]] = kernel_trace(a.reps, a.small)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
