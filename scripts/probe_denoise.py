"""pt_film_denoise: device ms of the a-trous filter on one MI355X, written as one JSON record under profiles/.

One Cornell film of 1920 x 1080, 32 spp, one frame, with its guides.  Reported (every ms figure: the call's own device events, median of
--reps alternated repetitions after a warm-up call of each shape, with min and max):
  denoise_N_iterations    pt_film_denoise with N = 1 .. 5 iterations (k_dn_prepare + N k_dn_atrous launches); wall_median_ms: the blocking call
                          as the host sees it (what a change of the host code around the kernels can move)
  render_32spp            pt_render of the same frame (PT_PIPELINE_AUTO, depth 8) in the same alternation: what a 5-iteration denoise costs
                          beside the frame it filters
  per_iteration           the differences between consecutive N: the cost of step 2^(N-1), with the algorithmic bytes (W * H * 48 B: two
                          16-B reads and one 16-B write per pixel) over that time
  free_bytes_moved_by_further_calls   free device memory before and after three further calls
  kernels                 per-kernel times from one `rocprofv3 --kernel-trace --stats` run of this script's measuring child (--no-trace skips
                          it); kernels_by_step: k_dn_atrous by its step, from the dispatch order in the same trace
--ab LIB[,LIB...]: the same measurement on other builds of libpt_amd.so (PT_LIB_AMD: a development build with another form of a kernel),
each in a process of its own, alternated with the in-tree build for --rounds rounds.
Usage: python scripts/probe_denoise.py [--reps 5] [--ab a.so,b.so] [--rounds 2] [--no-trace] [--out profiles/denoise_probe.json]"""
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
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H, SPP = 1920, 1080, 32


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def child(reps):
    """the measurement itself, in this process -> dict"""
    import ctypes
    import importlib
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")

    def free_bytes():
        hip = ctypes.CDLL("libamdhip64.so")
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    film = pt.Film(ctx, W, H)
    film.enable_aov()
    kw = dict(width=W, height=H, spp_per_frame=SPP, frame=0, frame_count=1, pipeline=pt.PIPELINE_AUTO)

    def render():
        before = ctx.stats().ms_total
        pt.render(sc, film, pt.default_params(max_depth=8, **kw))
        return ctx.stats().ms_total - before

    render()
    pt.render_aov(sc, film, pt.default_params(**kw))
    legs = {f"denoise_{n}_iterations": (lambda n=n: film.denoise(iterations=n)) for n in range(1, 6)}
    legs["render_32spp"] = render
    for fn in legs.values():   # warm-up: every shape once (the first denoise allocates the scratch)
        fn()
    ms, wall = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            ms[k].append(fn())
            wall[k].append((time.perf_counter() - t0) * 1e3)
    out = {k: summary(v) for k, v in ms.items()}
    for k in legs:
        if k.startswith("denoise_"):
            out[k]["wall_median_ms"] = round(statistics.median(wall[k]), 4)
    per = {}
    for n in range(1, 6):
        cur = out[f"denoise_{n}_iterations"]["median_ms"]
        prev = out[f"denoise_{n - 1}_iterations"]["median_ms"] if n > 1 else None
        step_ms = cur - prev if prev is not None else None
        per[f"step_{1 << (n - 1)}"] = {"ms": None if step_ms is None else round(step_ms, 4),
                                        "algorithmic_GB_per_s": None if not step_ms or step_ms <= 0 else round(W * H * 48 / (step_ms * 1e-3) / 1e9, 1)}
    out["per_iteration"] = per
    out["algorithmic_bytes_per_iteration"] = W * H * 48
    out["denoise5_over_render"] = round(out["denoise_5_iterations"]["median_ms"] / out["render_32spp"]["median_ms"], 4)
    free0 = free_bytes()
    for _ in range(3):
        film.denoise(iterations=5)
    out["free_bytes_moved_by_further_calls"] = free0 - free_bytes()
    film.close(); sc.close(); ctx.close()
    return out


def run_child(lib, reps, trace_dir=None):
    env = dict(os.environ)
    if lib:
        env["PT_LIB_AMD"] = os.path.abspath(lib)
    else:
        env.pop("PT_LIB_AMD", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", trace_dir, "--"] + cmd
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}): {r.stderr[-2000:]}")
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    return json.loads(line)


def short(name):
    return name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()


def kernel_stats(trace_dir):
    """-> (per-kernel stats of the trace, k_dn_atrous by step: the n-th k_dn_atrous dispatch after a k_dn_prepare runs step 2^(n-1))"""
    rows, by_step = {}, {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = short(r["Name"])
            if "k_dn_" in name or "k_fused" in name or "k_aov" in name:
                rows[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(int(r["MinNs"]) / 1e3, 2),
                              "max_us": round(int(r["MaxNs"]) / 1e3, 2)}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        disp = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
        n = 0
        for r in disp:
            name = short(r["Kernel_Name"])
            if "k_dn_prepare" in name:
                n = 0
            elif "k_dn_atrous" in name:
                by_step.setdefault(f"step_{1 << n}{'_last' if 'true' in name or 'Lb1' in name else ''}", []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                n += 1
    return rows, {k: {"calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in sorted(by_step.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--ab", default="")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "denoise_probe.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.reps)), flush=True)
        return
    rec = {"image": [W, H], "spp": SPP, "reps": args.reps}
    libs = [("in-tree", None)] + [(os.path.basename(p), p) for p in args.ab.split(",") if p]
    runs = {name: [] for name, _ in libs}
    for _ in range(args.rounds if len(libs) > 1 else 1):
        for name, path in libs:
            runs[name].append(run_child(path, args.reps))
            print(name, {k: (v["median_ms"], v["wall_median_ms"]) for k, v in runs[name][-1].items() if k.startswith("denoise_") and isinstance(v, dict)}, flush=True)
    rec.update(runs["in-tree"][0])
    if len(libs) > 1:
        rec["builds"] = {name: [{k: r[k] for k in r if k.startswith("denoise_") and k.endswith("iterations") or k == "per_iteration"} for r in rs]
                         for name, rs in runs.items()}
    if not args.no_trace:
        if shutil.which("rocprofv3"):
            d = tempfile.mkdtemp(prefix="dn_trace_")
            try:
                run_child(None, 1, trace_dir=d)
                rec["kernels"], rec["kernels_by_step"] = kernel_stats(d)
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
