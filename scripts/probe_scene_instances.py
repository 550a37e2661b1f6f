"""What the host round trip of an instance set costs on one MI355X, and what pt_scene_set_instances_device costs instead, as one JSON record
under profiles/ (DESIGN.md section 28).

Shapes: 3, 10 000 (config C4's grid), 32 768 and 2^20 instances of the Cornell box (grids in the z = 0 plane).  Per shape ONE scene takes,
alternated in one loop with two matrix sets in turn (so every set moves something), on the same build:
  b   tensor.cpu(), then Scene.set_instances                      -- the host path when the matrices are made on the GPU
  c   Scene.set_instances_tensor                                  -- pt_scene_set_instances_device
wall ms each, two warm-up passes, then medians of --reps (7) with min .. max.  After each of the two, the first render on PT_PIPELINE_WAVEFRONT_NEE
(64 x 48, 1 spp: where the world-space emitter copies are made -- the host loop after b, k_si_lights and the single-wave fold after c) and a
second one (the same render without that work) are timed too, and their films compared.
Kernel times per dispatch come from one `rocprofv3 --kernel-trace -f csv` run per shape of a child that repeats c and its first render: the new
kernels by name and the fold, k_inst_boxes / k_inst_sort for scale.  Without rocprofv3 that part is "not measured".
Usage: python scripts/probe_scene_instances.py [--reps 7] [--shapes 3 10000 ...] [--out profiles/scene_instances_probe.json]"""
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
SHAPES = [3, 10000, 32768, 1 << 20]
KERNELS = ("k_si_check_invert", "k_si_lights", "k_sd_emitter_fold", "k_inst_boxes", "k_inst_sort", "k_inst_frames")
W, H = 64, 48


def summary(x, unit="ms"):
    return {"median_" + unit: round(statistics.median(x), 4), "min_" + unit: round(min(x), 4), "max_" + unit: round(max(x), 4), "n": len(x)}


def matrices(pt, n):
    side = int(np.ceil(np.sqrt(n)))
    a = pt.cornell_grid_instances(side, cell=2.0 / side, scale=0.9 / side)[:n]
    b = a.copy()
    b[:, :, 3] += f32([0.25 / side, -0.25 / side, 0.0])
    return [np.ascontiguousarray(a, f32).reshape(-1), np.ascontiguousarray(b, f32).reshape(-1)]


def child(n, reps, trace_only):
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    v, i, f = pt.load_obj(pt.ASSET_CORNELL)
    scene = pt.Scene(ctx, v, i, f)
    xs = matrices(pt, n)
    txs = [torch.from_numpy(x).cuda() for x in xs]
    emitters = int((np.asarray(f, f32).reshape(-1, 6)[:, 3:] != 0).any(1).sum())
    rec = {"n_instances": n, "emitters": emitters, "emitter_copies": n * emitters, "bytes_each_way": int(xs[0].nbytes)}
    p = pt.default_params(frame=0, frame_count=1, width=W, height=H, spp_per_frame=1, max_depth=3, pipeline=pt.PIPELINE_WAVEFRONT_NEE)

    def nee_render():
        film = pt.Film(ctx, W, H)
        t0 = time.perf_counter()
        pt.render(scene, film, p)
        ms = (time.perf_counter() - t0) * 1e3
        out = film.read_f32().tobytes()
        film.close()
        return ms, out

    m = {k: [] for k in ("b_cpu_then_set", "b_first_nee_render", "b_second_nee_render", "c_set_tensor", "c_first_nee_render", "c_second_nee_render")}
    equal = True
    for k in range(2 + reps):
        tx = txs[k % 2]
        torch.cuda.synchronize()
        if trace_only:
            scene.set_instances_tensor(tx)
            nee_render()
            continue
        t0 = time.perf_counter(); scene.set_instances(tx.cpu().numpy()); b = (time.perf_counter() - t0) * 1e3
        b1, film_b = nee_render()
        b2, _ = nee_render()
        t0 = time.perf_counter(); scene.set_instances_tensor(tx); c = (time.perf_counter() - t0) * 1e3
        c1, film_c = nee_render()
        c2, _ = nee_render()
        equal = equal and film_b == film_c
        if k >= 2:
            for key, val in zip(m, (b, b1, b2, c, c1, c2)):
                m[key].append(val)
    if not trace_only:
        rec.update({k: summary(x) for k, x in m.items()})
        rec["nee_films_equal_in_every_pass"] = equal
        rec["b_emitter_copies_ms"] = round(rec["b_first_nee_render"]["median_ms"] - rec["b_second_nee_render"]["median_ms"], 4)
        rec["c_emitter_copies_ms"] = round(rec["c_first_nee_render"]["median_ms"] - rec["c_second_nee_render"]["median_ms"], 4)
        rec["b_minus_c_ms"] = round(rec["b_cpu_then_set"]["median_ms"] - rec["c_set_tensor"]["median_ms"], 4)
    print(json.dumps(rec))
    scene.close(); ctx.close()


def run_child(n, reps, extra=(), prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(reps)] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def kernel_trace(n, reps):
    """per-dispatch times of the set's kernels from one rocprofv3 run of the shape, or a string saying why not"""
    if not shutil.which("rocprofv3"):
        return "rocprofv3 not found: not measured"
    d = tempfile.mkdtemp(prefix="si_trace_")
    try:
        r = run_child(n, reps, ["--trace-only"], ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "--"])
        if r.returncode != 0:
            raise SystemExit(f"{n}: the traced child failed ({r.returncode}): {r.stderr[-3000:]}")
        per = {k: [] for k in KERNELS}
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in KERNELS:
                    if k in row["Kernel_Name"]:
                        per[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        return {k: dict(summary(x[-reps:], "us"), dispatches=len(x)) for k, x in per.items() if x} or "no dispatch of the set's kernels in the trace: not measured"
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", nargs="*", type=int, default=SHAPES)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scene_instances_probe.json"))
    ap.add_argument("--child", type=int)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.trace_only)
    rec = {"probe": "scene_instances", "reps": a.reps, "shapes": {}}
    for n in a.shapes:
        r = run_child(n, a.reps)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:   # a child that fails ends the probe: nothing more is started
            raise SystemExit(f"{n}: child failed ({r.returncode}): {r.stderr[-3000:]}")
        s = json.loads(lines[-1])
        s["kernels_us"] = kernel_trace(n, a.reps)
        rec["shapes"][str(n)] = s
        print(n, json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
