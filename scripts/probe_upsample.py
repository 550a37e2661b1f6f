"""pt_film_upsample: what the pass costs on one MI355X beside one a-trous iteration and beside the radiance it saves, written as one JSON
record under profiles/.

A 1920 x 1080 Cornell film with guides (PT_PIPELINE_AUTO, depth 8) and two low-resolution films, 960 x 540 and 640 x 360, each with --spp
samples of radiance and guides of its own in torch tensors, so that the same film is measured under two depth planes:
  rendered       lo's guides as pt_render_aov left them; second_ring_wave_share = the share of 64-pixel waves (rows of k_upsample's blocks)
                 in which the numpy statement of the first ring leaves a pixel below den = 0.01 (960 x 540 only: the host pass is slow)
  all_fallback   lo's depth plane times 100: every tap of both rings is rejected, so every wave walks the second ring and every pixel ends
                 at the nearest tap -- the upper end of the pass's cost
Every ms figure of `upsample` and `denoise` is the call's own device events, median of --reps alternated repetitions after a warm-up call of
each leg, with min and max.  atrous_iteration_ms is the difference of the medians of pt_film_denoise with 2 and with 1 iterations on the
full-size film, in the same loop.
  whole_step     wall ms of the blocking calls, alternated in the same loop: pt_render at 1080p against pt_render at 960 x 540 + the two
                 pt_render_aov + pt_film_upsample, at equal samples per pixel
  kernels        per-kernel times from one `rocprofv3 --kernel-trace --stats -f csv` run of the measuring child, in a run of its own
                 (--no-trace skips it)
Usage: python scripts/probe_upsample.py [--reps 7] [--spp 32] [--no-trace] [--out profiles/upsample_probe.json]"""
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
W, H = 1920, 1080
LOWS = [(960, 540), (640, 360)]
GUIDES = ["albedo", "normal", "emission", "depth", "alpha"]


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def child(reps, spp):
    """the measurement itself, in this process -> dict"""
    import importlib
    import numpy as np
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))

    def params(w, h, **kw):
        return pt.default_params(width=w, height=h, spp_per_frame=spp, frame=0, frame_count=1, pipeline=pt.PIPELINE_AUTO, **kw)
    film = pt.Film(ctx, W, H)
    film.enable_aov()
    pt.render(sc, film, params(W, H, max_depth=8))
    pt.render_aov(sc, film, params(W, H))
    lows = {}
    for lw, lh in LOWS:
        planes = {n: torch.zeros((lh, lw, 3) if n in ("albedo", "normal", "emission") else (lh, lw), dtype=torch.float32, device="cuda:0") for n in GUIDES}
        ids = torch.zeros((lh, lw, 2), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ptrs = [None] * pt.AOV_COUNT
        for n in GUIDES:
            ptrs[getattr(pt, "AOV_" + n.upper())] = planes[n].data_ptr()
        ptrs[pt.AOV_ID] = ids.data_ptr()
        lo = pt.Film(ctx, lw, lh)
        lo.enable_aov(ptrs)
        pt.render(sc, lo, params(lw, lh, max_depth=8))
        pt.render_aov(sc, lo, params(lw, lh))
        ctx.sync()
        depth = planes["depth"].clone()
        lows[(lw, lh)] = dict(film=lo, planes=planes, ids=ids, depth={"rendered": depth, "all_fallback": depth * 100.0})

    def up_leg(key, name):
        d = lows[key]

        def run():
            d["planes"]["depth"].copy_(d["depth"][name])
            torch.cuda.synchronize()
            return film.upsample(d["film"])
        return run

    def wall(fn):
        def run():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3
        return run
    scratch = pt.Film(ctx, W, H)     # the full-size render of the whole-step comparison goes into a film of its own
    half = lows[LOWS[0]]

    def step_low():
        half["planes"]["depth"].copy_(half["depth"]["rendered"])
        pt.render(sc, half["film"], params(LOWS[0][0], LOWS[0][1], max_depth=8))
        pt.render_aov(sc, half["film"], params(*LOWS[0]))
        pt.render_aov(sc, film, params(W, H))
        film.upsample(half["film"])
    legs = {f"upsample/{lw}x{lh}/{name}": up_leg((lw, lh), name) for lw, lh in LOWS for name in ("rendered", "all_fallback")}
    legs["denoise/1"] = lambda: film.denoise(iterations=1)
    legs["denoise/2"] = lambda: film.denoise(iterations=2)
    legs["step/render_1080p"] = wall(lambda: pt.render(sc, scratch, params(W, H, max_depth=8)))
    legs["step/render_960x540_two_aov_upsample"] = wall(step_low)
    for fn in legs.values():   # warm-up: every leg once (the first calls allocate the scratch)
        fn()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(fn())
    out = {"upsample": {}, "pipeline": int(ctx.stats().pipeline)}
    for lw, lh in LOWS:
        out["upsample"][f"{lw}x{lh}"] = {name: summary(ms[f"upsample/{lw}x{lh}/{name}"]) for name in ("rendered", "all_fallback")}
    d1, d2 = summary(ms["denoise/1"]), summary(ms["denoise/2"])
    out["denoise_1_iteration"], out["denoise_2_iterations"] = d1, d2
    out["atrous_iteration_ms"] = round(d2["median_ms"] - d1["median_ms"], 4)
    a, b = summary(ms["step/render_1080p"]), summary(ms["step/render_960x540_two_aov_upsample"])
    out["whole_step"] = {"spp": spp, "render_1080p_wall": a, "render_960x540_two_aov_upsample_wall": b, "low_over_full": round(b["median_ms"] / a["median_ms"], 4)}
    # the share of waves that walk the second ring on the rendered 960 x 540 film: the first ring's den, by numpy, from the planes read back
    lo = half["film"]
    half["planes"]["depth"].copy_(half["depth"]["rendered"])
    torch.cuda.synchronize()
    f32 = np.float32
    N, Z = film.read_aov(pt.AOV_NORMAL), film.read_aov(pt.AOV_DEPTH)
    N1, Z1 = lo.read_aov(pt.AOV_NORMAL), lo.read_aov(pt.AOV_DEPTH)
    p = pt.upsample_default_params()
    inv_n, sz2 = f32(1.0) / (f32(p.sigma_normal) * f32(p.sigma_normal)), f32(p.sigma_depth) * f32(p.sigma_depth)
    lw, lh = LOWS[0]
    axis = []
    for n, n_lo in ((W, lw), (H, lh)):
        fx = (np.arange(n, dtype=f32) + f32(0.5)) * (f32(n_lo) / f32(n)) - f32(0.5)
        x0 = np.floor(fx)
        axis.append((x0.astype(np.int64), fx - x0))
    (x0, bx), (y0, by) = axis
    den = np.zeros((H, W), f32)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0[None, :] + i, y0[:, None] + j
            ok = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh)
            qxc, qyc = np.clip(qx, 0, lw - 1), np.clip(qy, 0, lh - 1)
            dn = N - N1[qyc, qxc]
            x_n = ((dn[:, :, 0] * dn[:, :, 0] + dn[:, :, 1] * dn[:, :, 1]) + dn[:, :, 2] * dn[:, :, 2]) * inv_n
            Zq = Z1[qyc, qxc]
            dz = Z - Zq
            t = np.maximum(f32(0.0), f32(1.0) - (x_n + (dz * dz) / (sz2 * (Z * Z + Zq * Zq) + f32(1e-12))) * f32(0.0625))
            for _ in range(4):
                t = t * t
            wq = (bx if i else f32(1.0) - bx)[None, :] * (by if j else f32(1.0) - by)[:, None]
            den = np.where(ok, den + wq * t, den)
    fb = ~(den >= f32(0.01))
    out["second_ring_pixel_share"] = round(float(fb.mean()), 6)
    out["second_ring_wave_share"] = round(float(np.pad(fb, ((0, 0), (0, (-W) % 64))).reshape(H, -1, 64).any(axis=2).mean()), 6)
    for d in lows.values():
        d["film"].close()
    film.close(); scratch.close()
    sc.close(); ctx.close()
    return out


def run_child(reps, spp, trace_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps), "--spp", str(spp)]
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
            if "k_dn_" in name or "k_upsample" in name:
                rows[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(int(r["MinNs"]) / 1e3, 2),
                              "max_us": round(int(r["MaxNs"]) / 1e3, 2)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "upsample_probe.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.reps, args.spp)), flush=True)
        return
    rec = {"image": [W, H], "lows": [list(x) for x in LOWS], "spp": args.spp, "reps": args.reps}
    rec.update(run_child(args.reps, args.spp))
    if not args.no_trace:
        if shutil.which("rocprofv3"):
            d = tempfile.mkdtemp(prefix="up_trace_")
            try:
                run_child(1, args.spp, trace_dir=d)
                rec["kernels"] = kernel_stats(d)   # (k_upsample's min / max span the two sizes and the two depth planes)
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
