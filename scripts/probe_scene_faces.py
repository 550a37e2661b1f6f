"""What pt_scene_set_faces / pt_scene_set_faces_device cost on one MI355X beside the only way to get the same scene without them -- creating
it again -- as one JSON record under profiles/ (DESIGN.md section 30).

Shapes: the Cornell box; the 1 M-triangle soup; the 8 M soup (skipped, and the record says so, when it does not fit); the 10 000-instance grid of
the Cornell box with a NEE render behind every step (where the world-space emitter copies are made again).
Per shape, alternated in one loop with two face arrays in turn (so every step changes something):
  r_host    Scene(...) created again from numpy arrays (+ set_instances for the grid)     -- the yardstick of a
  r_dev     Scene.from_tensors(...) created again (+ set_instances_tensor for the grid)   -- the yardstick of c
  a         Scene.set_faces from a numpy array
  b         tensor.cpu() then Scene.set_faces                                              -- the yardstick of c when only set_faces existed
  c         Scene.set_faces_tensor
wall ms each, two warm-up passes, then medians of --reps (7) with min .. max.  The kept copy (read_faces) after a, b and c is compared with the
array in every pass.  Beside them: a device-to-device copy of the same bytes (torch, events).
Kernel times per dispatch come from one `rocprofv3 --kernel-trace -f csv` run per shape of a child that repeats c, then one REFIT update for
k_pack's time over the same scene: k_set_faces, the emitter kernels (k_sd_emitter_flags, the scan, _compact, _records, the fold apart).  Without
rocprofv3 that part is "not measured".
Usage: python scripts/probe_scene_faces.py [--reps 7] [--small] [--shapes ...] [--out profiles/scene_faces_probe.json]"""
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
SHAPES = ("cornell", "soup_1m", "soup_8m", "grid_10000")
KERNELS = ("k_set_faces", "k_sd_emitter_flags", "k_scan", "k_sd_emitter_compact", "k_sd_emitter_records", "k_sd_emitter_fold", "k_pack")
NEE_KW = dict(width=64, height=48, spp_per_frame=1, max_depth=5, cam_origin=(-0.88, -1.9, 0.5), cam_target=(-0.88, -1.9, 0.0))


def summary(x, unit="ms"):
    return {"median_" + unit: round(statistics.median(x), 4), "min_" + unit: round(min(x), 4), "max_" + unit: round(max(x), 4), "n": len(x)}


def arrays(pt, shape, small):
    if shape in ("cornell", "grid_10000"):
        v, i, f = pt.load_obj(pt.ASSET_CORNELL)
    else:
        n = {"soup_1m": 1 << 20, "soup_8m": 1 << 23}[shape]
        v, i, f = pt.make_soup(n >> 6 if small else n, 1)
    f = np.ascontiguousarray(f, f32).reshape(-1, 6)
    # the second face array: every Kd moved, every tenth triangle's emission toggled (so the emitter set changes in both directions)
    f2 = f.copy()
    f2[:, :3] = (f2[:, :3] * f32(0.5) + f32(0.25)).astype(f32)
    lit = (f2[:, 3:] != 0).any(1)
    sel = np.arange(len(f2)) % 10 == 0
    f2[sel & lit, 3:] = 0
    f2[sel & ~lit, 3:] = f32([2.0, 1.5, 1.0])
    grid = pt.cornell_grid_instances()[:100 if small else 10000] if shape == "grid_10000" else None
    return np.ascontiguousarray(v, f32).reshape(-1), np.ascontiguousarray(i, np.uint32).reshape(-1), [f.reshape(-1), f2.reshape(-1)], grid


def child(shape, reps, small, trace_only):
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    try:
        v, i, fs, grid = arrays(pt, shape, small)
        tv, ti = torch.from_numpy(v).cuda(), torch.from_numpy(i.view(np.int32)).cuda()
        tfs = [torch.from_numpy(f).cuda() for f in fs]
        tgrid = torch.from_numpy(np.ascontiguousarray(grid, f32).reshape(-1)).cuda() if grid is not None else None
        scene = pt.Scene.from_tensors(ctx, tv, ti, tfs[0])
        if grid is not None:
            scene.set_instances_tensor(tgrid)
        film = pt.Film(ctx, NEE_KW["width"], NEE_KW["height"])
    except (pt.PtError, RuntimeError, MemoryError) as e:
        print(json.dumps({"skipped": f"{type(e).__name__}: {e}"[:300]}))
        return
    nee = pt.default_params(frame=0, frame_count=1, pipeline=pt.PIPELINE_WAVEFRONT_NEE, **NEE_KW)

    def first_nee(s):   # the grid only: the render that makes the world-space emitter copies again
        if grid is None:
            return 0.0
        t0 = time.perf_counter(); pt.render(s, film, nee); return (time.perf_counter() - t0) * 1e3

    rec = {"n_tris": len(i) // 3, "emitters": [int((f.reshape(-1, 6)[:, 3:] != 0).any(1).sum()) for f in fs], "bytes": int(fs[0].nbytes),
           "instances": 0 if grid is None else len(grid), "build_ms_at_create": round(scene.info().build_ms, 4)}
    keys = ("r_host", "r_dev", "a_set_faces", "b_cpu_then_set_faces", "c_set_faces_tensor", "d2d_copy_device", "nee_after_r_dev", "nee_after_c")
    m = {k: [] for k in keys}
    equal = True
    dst = torch.empty_like(tfs[0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in range(2 + reps):
        f, tf = fs[k % 2], tfs[k % 2]
        torch.cuda.synchronize()
        if trace_only:
            scene.set_faces_tensor(tf)
            continue
        t0 = time.perf_counter()
        s = pt.Scene(ctx, v, i, f)
        if grid is not None:
            s.set_instances(grid)
        r_host = (time.perf_counter() - t0) * 1e3
        s.close()
        t0 = time.perf_counter()
        s = pt.Scene.from_tensors(ctx, tv, ti, tf)
        if grid is not None:
            s.set_instances_tensor(tgrid)
        r_dev = (time.perf_counter() - t0) * 1e3
        nee_r = first_nee(s)
        s.close()
        t0 = time.perf_counter(); scene.set_faces(f); a = (time.perf_counter() - t0) * 1e3
        equal = equal and scene.read_faces().tobytes() == f.tobytes()
        scene.set_faces(fs[(k + 1) % 2])
        t0 = time.perf_counter(); scene.set_faces(tf.cpu().numpy()); b = (time.perf_counter() - t0) * 1e3
        equal = equal and scene.read_faces().tobytes() == f.tobytes()
        scene.set_faces(fs[(k + 1) % 2])
        first_nee(scene)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); scene.set_faces_tensor(tf); c = (time.perf_counter() - t0) * 1e3
        nee_c = first_nee(scene)
        equal = equal and scene.read_faces().tobytes() == f.tobytes()
        e0.record(); dst.copy_(tf); e1.record(); torch.cuda.synchronize()
        if k >= 2:
            for key, val in zip(keys, (r_host, r_dev, a, b, c, e0.elapsed_time(e1), nee_r, nee_c)):
                m[key].append(val)
    if trace_only:
        scene.update_tensors(tv, ti, mode=pt.SCENE_UPDATE_REFIT)    # k_pack over the same scene, for scale
    else:
        rec.update({k: summary(x) for k, x in m.items() if grid is not None or not k.startswith("nee_")})
        rec["read_faces_equal_in_every_pass"] = equal
        rec["c_loses_to_recreation"] = bool(rec["c_set_faces_tensor"]["median_ms"] >= rec["r_dev"]["median_ms"])
        rec["a_loses_to_recreation"] = bool(rec["a_set_faces"]["median_ms"] >= rec["r_host"]["median_ms"])
    print(json.dumps(rec))
    film.close(); scene.close(); ctx.close()


def run_child(shape, reps, small, extra=(), prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(reps)] + (["--small"] if small else []) + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


def kernel_trace(shape, reps, small):
    """per-dispatch times of the call's kernels from one rocprofv3 run of the shape, or a string saying why not"""
    if not shutil.which("rocprofv3"):
        return "rocprofv3 not found: not measured"
    d = tempfile.mkdtemp(prefix="sf_trace_")
    try:
        r = run_child(shape, reps, small, ["--trace-only"], ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "--"])
        if r.returncode != 0:
            raise SystemExit(f"{shape}: the traced child failed ({r.returncode}): {r.stderr[-3000:]}")
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                rows.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3, row["Kernel_Name"]))
        rows.sort()
        # every call ends with k_set_faces: its dispatches cut the trace into calls; the last `reps` of them are the measured ones
        ends = [k for k, (_, _, nm) in enumerate(rows) if "k_set_faces" in nm]
        if len(ends) < reps + 1:
            return "no dispatch of the call's kernels in the trace: not measured"
        calls = [rows[s + 1:e + 1] for s, e in zip(ends[-reps - 1:-1], ends[-reps:])]
        out = {}
        for key in KERNELS[:-1] + ("",):   # "": every kernel of the call
            per_call = [sum(u for _, u, nm in call if key in nm) for call in calls]
            if any(per_call):
                out[key or "all_kernels"] = dict(summary(per_call, "us"), dispatches_per_call=sum(1 for _, _, nm in calls[-1] if key in nm))
        pack = [u for _, u, nm in rows[ends[-1] + 1:] if "k_pack" in nm]
        if pack:
            out["k_pack_of_one_refit"] = {"us_each": [round(u, 2) for u in pack]}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a quick pass over small shapes (a check of the script, not a measurement)")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scene_faces_probe.json"))
    ap.add_argument("--child")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.small, a.trace_only)
    rec = {"probe": "scene_faces", "reps": a.reps, "small": a.small, "shapes": {}}
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
