"""pt_film_denoise_history: what the per-pixel variance costs beside pt_film_denoise_variance on the same film, on one MI355X, written as one
JSON record under profiles/.

Two Cornell films of 1920 x 1080 with guides, M and L, ping-ponged over step 0 and three reprojection steps of one frame x 4 spp each
(PT_PIPELINE_AUTO, depth 8, camera step (0.1, 0, 0)).  The last film's L lives in a torch tensor, so that the same film is measured under
three history planes:
  all_long    L = 8 everywhere: k_dn_var_spatial only copies (one extra pass of 32 B per pixel over pt_film_denoise_variance)
  band        L as the reprojection left it: a band without history at the side the camera moves towards, disocclusions elsewhere;
              short_wave_share = the share of 64-pixel waves (rows of k_dn_var_spatial's blocks) with at least one pixel below min_history
  all_short   L = 0 everywhere: every wave walks the 5 x 5 window
Every ms figure is the call's own device events, 5 iterations, median of --reps alternated repetitions after a warm-up call of each leg, with
min and max.  history_minus_variance_ms is the difference of the medians of the two calls under the same plane;
atrous_iteration_ms_from_variance_call is pt_film_denoise_variance's median / 5, an upper bound of the yardstick "one a-trous iteration" (the
kernel trace has the k_dn_atrous_var launches themselves).
  kernels     per-kernel times from one `rocprofv3 --kernel-trace --stats -f csv` run of the measuring child, in a run of its own
              (--no-trace skips it)
Usage: python scripts/probe_denoise_history.py [--reps 7] [--no-trace] [--out profiles/denoise_history_probe.json]"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H, SPP, STEPS, ITERATIONS, MOVE, MIN_HISTORY = 1920, 1080, 4, 3, 5, (0.1, 0.0, 0.0), 4.0


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def child(reps):
    """the measurement itself, in this process -> dict"""
    import importlib
    import numpy as np
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    t_len = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    films = [pt.Film(ctx, W, H), pt.Film(ctx, W, H)]
    for k, f in enumerate(films):
        f.enable_aov()
        f.enable_moments()
        f.enable_history(t_len.data_ptr() if k == (STEPS & 1) else None)
    base = pt.default_params()
    prev = prev_cam = None
    for k in range(STEPS + 1):
        f = films[k & 1]
        f.clear()
        cam = {n: tuple(float(v) + MOVE[c] * k for c, v in enumerate(getattr(base, n))) for n in ("cam_origin", "cam_target")}
        kw = dict(width=W, height=H, spp_per_frame=SPP, frame_count=1, pipeline=pt.PIPELINE_AUTO, **cam)
        pt.render(sc, f, pt.default_params(frame=k, max_depth=8, **kw))
        pt.render_aov(sc, f, pt.default_params(frame=0, **kw))
        f.reproject(prev, cam, prev_cam or cam, gain=float(k + 1))
        prev, prev_cam = f, cam
    film = films[STEPS & 1]
    ctx.sync()
    band = t_len.clone()
    L = band.cpu().numpy()
    covered = film.read_aov(pt.AOV_ALPHA) > 0
    short = ~(L >= MIN_HISTORY)
    pad = (-W) % 64
    waves = np.pad(short, ((0, 0), (0, pad))).reshape(H, -1, 64).any(axis=2)
    planes = {"all_long": torch.full_like(band, 8.0), "band": band, "all_short": torch.zeros_like(band)}

    def leg(name, call):
        def run():
            t_len.copy_(planes[name])
            torch.cuda.synchronize()
            return call()
        return run
    legs = {}
    for name in planes:
        legs[name + "/variance"] = leg(name, lambda: film.denoise_variance(iterations=ITERATIONS, frames=STEPS + 1))
        legs[name + "/history"] = leg(name, lambda: film.denoise_history(iterations=ITERATIONS, min_history=MIN_HISTORY))
    for fn in legs.values():   # warm-up: every leg once (the first call allocates the scratch)
        fn()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(fn())
    out = {"films": {}}
    for name in planes:
        v, h = summary(ms[name + "/variance"]), summary(ms[name + "/history"])
        out["films"][name] = {"denoise_variance": v, "denoise_history": h, "history_minus_variance_ms": round(h["median_ms"] - v["median_ms"], 4),
                              "history_over_variance": round(h["median_ms"] / v["median_ms"], 4)}
    out["short_pixel_share"] = round(float(short.mean()), 5)
    out["short_covered_pixel_share"] = round(float((short & covered).sum()) / float(covered.sum()), 5)
    out["short_wave_share"] = round(float(waves.mean()), 5)
    out["atrous_iteration_ms_from_variance_call"] = round(out["films"]["band"]["denoise_variance"]["median_ms"] / ITERATIONS, 4)
    out["pipeline"] = int(ctx.stats().pipeline)
    for f in films:
        f.close()
    sc.close(); ctx.close()
    return out


def run_child(reps, trace_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", trace_dir, "--"] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


def kernel_stats(trace_dir):
    rows = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
            if "k_dn_" in name or "k_reproject" in name:
                rows[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(int(r["MinNs"]) / 1e3, 2),
                              "max_us": round(int(r["MaxNs"]) / 1e3, 2)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "denoise_history_probe.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.reps)), flush=True)
        return
    rec = {"image": [W, H], "spp": SPP, "reprojection_steps": STEPS, "camera_step": list(MOVE), "iterations": ITERATIONS, "min_history": MIN_HISTORY, "reps": args.reps}
    rec.update(run_child(args.reps))
    if not args.no_trace:
        if shutil.which("rocprofv3"):
            d = tempfile.mkdtemp(prefix="dnh_trace_")
            try:
                run_child(1, trace_dir=d)
                rec["kernels"] = kernel_stats(d)   # (k_dn_var_spatial's min / max span the three planes: all-long copies, all-short walks)
            finally:
                shutil.rmtree(d, ignore_errors=True)
        else:
            rec["kernels"] = "rocprofv3 not found: not measured"
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec, indent=1))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
