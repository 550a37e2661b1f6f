"""What the host round trip of a scene update costs on one MI355X, and what pt_scene_update_device costs instead, as one JSON record under
profiles/ (DESIGN.md section 27).

Shapes: the Cornell box (REFIT), the 1 M-triangle soup (REFIT and REBUILD), the 8 M soup (REFIT; skipped, and the record says so, when it does
not fit).  Per shape ONE scene takes, alternated in one loop with the same arrays (two vertex sets in turn, so every update moves something):
  a   Scene.update from numpy arrays                               -- the parent's path when the geometry is on the host anyway
  b   tensor.cpu() of both tensors, then Scene.update              -- the parent's path when the geometry is made on the GPU
  c   Scene.update_tensors                                         -- pt_scene_update_device
wall ms each, two warm-up passes, then medians of --reps (7) with min .. max; pt_scene_read_bvh4's bytes after a, b and c are compared in every
pass.  build_ms of c (the update's own span on the stream) is reported beside its wall time.
Kernel times per dispatch come from one `rocprofv3 --kernel-trace -f csv` run per shape of a child that repeats c: the new kernels by name
(k_sd_*, the emitter fold apart), and k_gather / k_refit* / k_pack for scale.  Without rocprofv3 that part is "not measured".
Usage: python scripts/probe_scene_device.py [--reps 7] [--small] [--out profiles/scene_device_probe.json]"""
import argparse
import csv
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
SHAPES = {"cornell/refit": ("cornell", 0), "soup_1m/refit": ("soup_1m", 0), "soup_1m/rebuild": ("soup_1m", 1), "soup_8m/refit": ("soup_8m", 0)}
NEW_KERNELS = ("k_sd_check_indices", "k_sd_emitter_flags", "k_sd_emitter_compact", "k_sd_emitter_records", "k_sd_emitter_fold", "k_sd_fan_flags")
OLD_KERNELS = ("k_gather", "k_refit", "k_pack", "k_wide_half")


def summary(x, unit="ms"):
    return {"median_" + unit: round(statistics.median(x), 4), "min_" + unit: round(min(x), 4), "max_" + unit: round(max(x), 4), "n": len(x)}


def arrays(pt, scene, small):
    if scene == "cornell":
        v, i, f = pt.load_obj(pt.ASSET_CORNELL)
    else:
        n = {"soup_1m": 1 << 20, "soup_8m": 1 << 23}[scene]
        v, i, f = pt.make_soup(n >> 6 if small else n, 1)
    v = np.ascontiguousarray(v, f32).reshape(-1)
    # the second vertex set: the whole mesh shifted by one vector (fan pairs stay pairs, so a REFIT stays a refit)
    v2 = (v.reshape(-1, 3) + f32([0.01, 0.02, -0.01])).reshape(-1).astype(f32)
    return [v, v2], np.ascontiguousarray(i, np.uint32).reshape(-1), np.ascontiguousarray(f, f32).reshape(-1)


def child(shape, reps, small, trace_only):
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    scene_name, mode = SHAPES[shape]
    ctx = pt.Context(0)
    try:
        vs, i, f = arrays(pt, scene_name, small)
        tvs = [torch.from_numpy(v).cuda() for v in vs]
        ti, tf = torch.from_numpy(i.view(np.int32)).cuda(), torch.from_numpy(f).cuda()
        scene = pt.Scene.from_tensors(ctx, tvs[0], ti, tf)
    except (pt.PtError, RuntimeError, MemoryError) as e:
        print(json.dumps({"skipped": f"{type(e).__name__}: {e}"[:300]}))
        return
    rec = {"n_tris": len(i) // 3, "n_verts": len(vs[0]) // 3, "emitters": int((f.reshape(-1, 6)[:, 3:] != 0).any(1).sum()),
           "bytes_each_way": int(vs[0].nbytes + i.nbytes), "mode": "rebuild" if mode else "refit"}
    m = {"a_numpy_update": [], "b_cpu_then_update": [], "c_update_tensors": [], "c_build_ms": []}
    equal = True
    for k in range(2 + reps):
        v, tv = vs[k % 2], tvs[k % 2]
        torch.cuda.synchronize()
        if trace_only:
            scene.update_tensors(tv, ti, mode=mode)
            continue
        t0 = time.perf_counter(); scene.update(v, i, mode=mode); a = (time.perf_counter() - t0) * 1e3
        rows_a = scene.read_bvh4().tobytes()
        t0 = time.perf_counter(); scene.update(tv.cpu().numpy(), ti.cpu().numpy().view(np.uint32), mode=mode); b = (time.perf_counter() - t0) * 1e3
        rows_b = scene.read_bvh4().tobytes()
        t0 = time.perf_counter(); scene.update_tensors(tv, ti, mode=mode); c = (time.perf_counter() - t0) * 1e3
        equal = equal and rows_a == rows_b == scene.read_bvh4().tobytes()
        if k >= 2:
            m["a_numpy_update"].append(a); m["b_cpu_then_update"].append(b); m["c_update_tensors"].append(c); m["c_build_ms"].append(scene.info().build_ms)
    if not trace_only:
        rec.update({k: summary(x) for k, x in m.items()})
        rec["read_bvh4_equal_in_every_pass"] = equal
        b, c = rec["b_cpu_then_update"], rec["c_update_tensors"]
        rec["b_minus_c_ms"] = round(b["median_ms"] - c["median_ms"], 4)
        rec["b_spread_ms"] = round(b["max_ms"] - b["min_ms"], 4)
        rec["c_below_b_by_more_than_b_spread"] = bool(rec["b_minus_c_ms"] > rec["b_spread_ms"])
    print(json.dumps(rec))
    scene.close(); ctx.close()


def run_child(shape, reps, small, extra=(), prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(reps)] + (["--small"] if small else []) + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


def kernel_trace(shape, reps, small):
    """per-dispatch times of the update's kernels from one rocprofv3 run of the shape, or a string saying why not"""
    if not shutil.which("rocprofv3"):
        return "rocprofv3 not found: not measured"
    d = tempfile.mkdtemp(prefix="sd_trace_")
    try:
        r = run_child(shape, reps, small, ["--trace-only"], ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "--"])
        if r.returncode != 0:
            raise SystemExit(f"{shape}: the traced child failed ({r.returncode}): {r.stderr[-3000:]}")
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3, row["Kernel_Name"]))
        rows.sort()
        # every call begins with the index check: its dispatches cut the trace into calls; the last `reps` of them are the measured updates
        starts = [k for k, (_, _, nm) in enumerate(rows) if "k_sd_check_indices" in nm]
        if len(starts) < reps:
            return "no dispatch of the update's kernels in the trace: not measured"
        calls = [rows[s:e] for s, e in zip(starts, starts[1:] + [len(rows)])][-reps:]
        out = {}
        for key in NEW_KERNELS + OLD_KERNELS + ("",):   # "": every kernel of the call
            per_call = [sum(u for _, u, nm in call if key in nm) for call in calls]
            if any(per_call):
                out[key or "all_kernels"] = dict(summary(per_call, "us"), dispatches_per_update=sum(1 for _, _, nm in calls[-1] if key in nm))
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a quick pass over small shapes (a check of the script, not a measurement)")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scene_device_probe.json"))
    ap.add_argument("--child")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.small, a.trace_only)
    rec = {"probe": "scene_device", "reps": a.reps, "small": a.small, "shapes": {}}
    for shape in a.shapes:
        r = run_child(shape, a.reps, a.small)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:   # (a shape that does not fit says so itself and exits 0; anything else ends the probe: nothing more is started)
            raise SystemExit(f"{shape}: child failed ({r.returncode}): {r.stderr[-3000:]}")
        s = json.loads(lines[-1])
        if "skipped" not in s:
            s["kernels_us"] = kernel_trace(shape, a.reps, a.small)
        rec["shapes"][shape] = s
        print(shape, json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
