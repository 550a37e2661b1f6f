"""pt_film_enable_moments / pt_film_denoise_variance: what the second-moment plane costs a render and what the variance-guided filter costs
beside pt_film_denoise, on one MI355X, written as one JSON record under profiles/.

One Cornell film of 1920 x 1080, 8 frames x 4 spp in one pt_render call (PT_PIPELINE_AUTO, depth 8), with its guides.  Every ms figure is
the call's own device events, median of --reps alternated repetitions after a warm-up call of each leg, with min and max:
  render_plain / render_moments     pt_render of the 8 frames into a film without / with the plane (two films of one context, alternated);
                                    moments_share_of_render = (with - without) / with
  denoise / denoise_variance        pt_film_denoise and pt_film_denoise_variance on the film with the plane, 5 iterations both, alternated;
                                    variance_over_plain = their ratio
  kernels                           per-kernel times from one `rocprofv3 --kernel-trace --stats -f csv` run of the measuring child, in a
                                    run of its own (--no-trace skips it): the split between k_dn_prepare_var, k_dn_var_blur and the
                                    k_dn_atrous_var launches against k_dn_prepare and k_dn_atrous
Usage: python scripts/probe_denoise_variance.py [--reps 5] [--no-trace] [--out profiles/denoise_variance_probe.json]"""
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
W, H, SPP, FRAMES, ITERATIONS = 1920, 1080, 4, 8, 5


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def child(reps):
    """the measurement itself, in this process -> dict"""
    import importlib
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    plain, film = pt.Film(ctx, W, H), pt.Film(ctx, W, H)
    film.enable_moments()
    kw = dict(width=W, height=H, spp_per_frame=SPP, frame=0, frame_count=FRAMES, pipeline=pt.PIPELINE_AUTO)

    def render(f):
        before = ctx.stats().ms_total
        pt.render(sc, f, pt.default_params(max_depth=8, **kw))
        return ctx.stats().ms_total - before

    legs = {"render_plain": lambda: render(plain), "render_moments": lambda: render(film)}
    for fn in legs.values():
        fn()
    for f in (plain, film):
        f.enable_aov()
        pt.render_aov(sc, f, pt.default_params(**kw))
    legs["denoise"] = lambda: film.denoise(iterations=ITERATIONS)
    legs["denoise_variance"] = lambda: film.denoise_variance(iterations=ITERATIONS)
    for fn in legs.values():   # warm-up: every leg once (the first denoise allocates the scratch)
        fn()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(fn())
    out = {k: summary(v) for k, v in ms.items()}
    a, b = out["render_plain"]["median_ms"], out["render_moments"]["median_ms"]
    out["moments_ms_per_render_call"] = round(b - a, 4)
    out["moments_share_of_render"] = round((b - a) / b, 5)
    out["variance_over_plain"] = round(out["denoise_variance"]["median_ms"] / out["denoise"]["median_ms"], 4)
    out["pipeline"] = int(ctx.stats().pipeline)
    plain.close(); film.close(); sc.close(); ctx.close()
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
            if "k_dn_" in name or "k_resolve" in name or "k_fused" in name:
                rows[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(int(r["MinNs"]) / 1e3, 2),
                              "max_us": round(int(r["MaxNs"]) / 1e3, 2)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "denoise_variance_probe.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.reps)), flush=True)
        return
    rec = {"image": [W, H], "spp": SPP, "frames": FRAMES, "iterations": ITERATIONS, "reps": args.reps}
    rec.update(run_child(args.reps))
    if not args.no_trace:
        if shutil.which("rocprofv3"):
            d = tempfile.mkdtemp(prefix="dnv_trace_")
            try:
                run_child(1, trace_dir=d)
                rec["kernels"] = kernel_stats(d)
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
