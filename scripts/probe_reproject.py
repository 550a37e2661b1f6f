"""pt_film_reproject: what the temporal accumulation step costs beside the step's own render and the denoiser, on one MI355X, written as
one JSON record under profiles/.

Two Cornell films of 1920 x 1080 (with guides, second-moment plane and history length) and two without the second-moment plane: one
rendered at the default camera (step 0, reprojected with prev = NULL), one at the camera moved by (0.02, 0, 0) (frame 1, 4 spp, depth 8,
PT_PIPELINE_AUTO).  Every ms figure is the call's own device events, median of --reps alternated repetitions after a warm-up call of each
leg, with min and max:
  reproject / reproject_m     pt_film_reproject of the moved film against the first, without / with the second-moment plane (gain 1, so that
                              repeating the in-place call keeps the film's values in range; the time does not depend on them)
  denoise                     pt_film_denoise, 5 iterations, on the moved film
  render                      the step's own pt_render (one frame of 4 spp)
  gbytes_per_s                the call's algorithmic bytes over its time (the events' time: launch overhead included): per pixel 44 B read and 20 B written of `film` and 48 B of `prev`
                              counted once (112 B), with M 12 B more in each of the three (148 B)
  kernels                     per-dispatch kernel times from one `rocprofv3 --kernel-trace -f csv` run of the measuring child, in a run of its
                              own (--no-trace skips it): k_reproject (its calls with `prev` set) beside k_dn_prepare, a kernel of the same
                              streaming shape (56 B read, 32 B written per pixel), each with its bytes over its median kernel time;
                              reproject_over_prepare_rate / reproject_m_over_prepare_rate are the ratios of those two rates
Usage: python scripts/probe_reproject.py [--reps 5] [--no-trace] [--out profiles/reproject_probe.json]"""
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
W, H, SPP, ITERATIONS = 1920, 1080, 4, 5
STEP = (0.02, 0.0, 0.0)
BYTES = {"reproject": 112, "reproject_m": 148, "k_dn_prepare": 88}


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def rate(bytes_per_pixel, ms):
    return round(bytes_per_pixel * W * H / (ms * 1e-3) / 1e9, 1)


def child(reps):
    """the measurement itself, in this process -> dict"""
    import importlib
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    base = pt.default_params()
    cams = [{"cam_origin": tuple(base.cam_origin[c] + k * STEP[c] for c in range(3)), "cam_target": tuple(base.cam_target[c] + k * STEP[c] for c in range(3))}
            for k in (0, 1)]
    films = {}
    for moments in (False, True):
        pair = []
        for k in (0, 1):
            f = pt.Film(ctx, W, H)
            f.enable_aov()
            if moments:
                f.enable_moments()
            f.enable_history()
            kw = dict(width=W, height=H, spp_per_frame=SPP, frame_count=1, pipeline=pt.PIPELINE_AUTO, **cams[k])
            pt.render(sc, f, pt.default_params(frame=k, max_depth=8, **kw))
            pt.render_aov(sc, f, pt.default_params(frame=0, **kw))
            pair.append(f)
        pair[0].reproject(None, cams[0], cams[0])
        films[moments] = pair
    scratch = pt.Film(ctx, W, H)

    def render():
        before = ctx.stats().ms_total
        pt.render(sc, scratch, pt.default_params(frame=1, frame_count=1, width=W, height=H, spp_per_frame=SPP, max_depth=8, pipeline=pt.PIPELINE_AUTO, **cams[1]))
        return ctx.stats().ms_total - before

    legs = {"reproject": lambda: films[False][1].reproject(films[False][0], cams[1], cams[0]),
            "reproject_m": lambda: films[True][1].reproject(films[True][0], cams[1], cams[0]),
            "denoise": lambda: films[True][1].denoise(iterations=ITERATIONS),
            "render": render}
    for fn in legs.values():   # warm-up: every leg once (the first denoise allocates the scratch)
        fn()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(fn())
    out = {k: summary(v) for k, v in ms.items()}
    for k in ("reproject", "reproject_m"):
        out[k]["bytes_per_pixel"] = BYTES[k]
        out[k]["gbytes_per_s"] = rate(BYTES[k], out[k]["median_ms"])
    hist = films[True][1].read_history()
    alpha = films[True][1].read_aov(pt.AOV_ALPHA)
    out["covered_pixels_with_history"] = round(float((hist[alpha > 0] > 1).mean()), 4)
    out["reproject_m_over_render"] = round(out["reproject_m"]["median_ms"] / out["render"]["median_ms"], 4)
    out["reproject_m_over_denoise"] = round(out["reproject_m"]["median_ms"] / out["denoise"]["median_ms"], 4)
    out["pipeline"] = int(ctx.stats().pipeline)
    for pair in films.values():
        for f in pair:
            f.close()
    scratch.close(); sc.close(); ctx.close()
    return out


def run_child(reps, trace_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", trace_dir, "--"] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


def kernel_stats(trace_dir):
    """per-dispatch kernel times of the trace run -> {kernel: {calls, median_us, min_us, max_us[, bytes_per_pixel, gbytes_per_s]}}.  k_reproject's first
    dispatch of each instantiation is the set-up's prev = NULL call, which reads no previous film: it is left out, so that the rate is that of
    calls with `prev` set.  Both rates are bytes over the MEDIAN kernel time of this one run."""
    durs = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
            if "k_reproject" in name or "k_dn_" in name:
                durs.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for name, us in durs.items():
        b = None
        if "k_reproject" in name:
            us = us[1:]
            b = BYTES["reproject_m"] if "<true>" in name else BYTES["reproject"]
        elif name == "k_dn_prepare":
            b = BYTES["k_dn_prepare"]
        if not us:
            continue
        out[name] = {"calls": len(us), "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
        if b:
            out[name]["bytes_per_pixel"] = b
            out[name]["gbytes_per_s"] = rate(b, out[name]["median_us"] * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "reproject_probe.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.reps)), flush=True)
        return
    rec = {"image": [W, H], "spp": SPP, "cam_step": list(STEP), "iterations": ITERATIONS, "reps": args.reps}
    rec.update(run_child(args.reps))
    if not args.no_trace:
        if shutil.which("rocprofv3"):
            d = tempfile.mkdtemp(prefix="rp_trace_")
            try:
                run_child(args.reps, trace_dir=d)
                rec["kernels"] = kernel_stats(d)
                # the test that decides on the packed form: both sides from this one trace run, kernel time against kernel time
                prep = rec["kernels"].get("k_dn_prepare")
                for key, inst in (("reproject", "k_reproject<false>"), ("reproject_m", "k_reproject<true>")):
                    k = rec["kernels"].get(inst)
                    if prep and k:
                        rec[key + "_over_prepare_rate"] = round(k["gbytes_per_s"] / prep["gbytes_per_s"], 3)
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
