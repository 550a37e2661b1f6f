"""pt_render_aov: device ms (pt_stats.ms_total) of the guide buffers on one MI355X, written as one JSON record under profiles/.

Legs (every figure: median of --reps alternated repetitions after a warm-up call of the same shape, with min and max):
  cornell   Cornell box, 1920 x 1080, 32 spp, 1 and 16 frames per call: pt_render_aov through PT_PIPELINE_FUSED and _WAVEFRONT, and the
            yardstick pt_render(PT_PIPELINE_AUTO, max_depth = 1), which traces exactly the same camera rays through k_fused and writes
            16 B per pixel where the guides write 56 B.  Also: free device memory before and after three further calls of each shape
            (the scratch stays with the film: no allocation).
  big       the 10 000-instance grid and the 1 M-triangle soup, one frame per call: the queue form, and a full pt_render of the same
            parameters (what share of a frame the separate pass costs a denoising user).
--baseline-only runs the yardstick alone: it needs pt_render only, so it also runs on a build without pt_render_aov (PT_LIB_AMD).
Usage: python scripts/probe_aov.py [--legs cornell,big] [--reps 5] [--baseline-only] [--out profiles/aov_probe.json]"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pt = importlib.import_module("single-file-vulkan-pathtracing_amd")


def free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def device_ms(ctx, fn):
    before = ctx.stats().ms_total
    fn()
    return ctx.stats().ms_total - before


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def alternate(ctx, legs, reps):
    """legs: {name: callable}; one warm-up each, then `reps` rounds that run every leg once -> {name: summary}"""
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            ms[k].append(device_ms(ctx, fn))
    return {k: summary(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="cornell,big")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "aov_probe.json"))
    args = ap.parse_args()
    ctx = pt.Context(0)
    w, h, spp = 1920, 1080, 32
    rec = {"image": [w, h], "spp": spp, "reps": args.reps, "lib": os.environ.get("PT_LIB_AMD", "in-tree")}
    legs = args.legs.split(",")
    if "cornell" in legs:
        sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
        film = pt.Film(ctx, w, h)
        if not args.baseline_only:
            film.enable_aov()
        for k in (1, 16):
            kw = dict(width=w, height=h, spp_per_frame=spp, frame=0, frame_count=k)
            run = {"render_depth1_auto": lambda: pt.render(sc, film, pt.default_params(max_depth=1, pipeline=pt.PIPELINE_AUTO, **kw))}
            if not args.baseline_only:
                run["aov_fused"] = lambda: pt.render_aov(sc, film, pt.default_params(pipeline=pt.PIPELINE_FUSED, **kw))
                run["aov_wavefront"] = lambda: pt.render_aov(sc, film, pt.default_params(pipeline=pt.PIPELINE_WAVEFRONT, **kw))
            out = alternate(ctx, run, args.reps)
            if not args.baseline_only:
                out["fused_over_yardstick"] = round(out["aov_fused"]["median_ms"] / out["render_depth1_auto"]["median_ms"], 4)
                out["wavefront_over_fused"] = round(out["aov_wavefront"]["median_ms"] / out["aov_fused"]["median_ms"], 4)
                free0 = free_bytes()
                for _ in range(3):
                    run["aov_fused"]()
                    run["aov_wavefront"]()
                out["free_bytes_moved_by_further_calls"] = free0 - free_bytes()
            rec[f"cornell_{k}_frames_per_call"] = out
            print(k, out, flush=True)
        film.close(); sc.close()
    if "big" in legs and not args.baseline_only:
        for name in ("grid10000", "soup1m"):
            cam = {}
            if name == "grid10000":
                sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
                sc.set_instances(pt.cornell_grid_instances())
                cam = dict(cam_origin=(0.0, -1.0, 1.2), cam_target=(0.0, -1.0, 0.0))
            else:
                sc = pt.Scene(ctx, *pt.make_soup(1000000, 1))
            film = pt.Film(ctx, w, h)
            film.enable_aov()
            kw = dict(width=w, height=h, spp_per_frame=spp, frame=0, frame_count=1, **cam)
            out = alternate(ctx, {"aov_wavefront": lambda: pt.render_aov(sc, film, pt.default_params(pipeline=pt.PIPELINE_WAVEFRONT, **kw)),
                                  "render_full_auto": lambda: pt.render(sc, film, pt.default_params(max_depth=8, pipeline=pt.PIPELINE_AUTO, **kw))}, args.reps)
            out["aov_share_of_a_frame"] = round(out["aov_wavefront"]["median_ms"] / out["render_full_auto"]["median_ms"], 4)
            rec[name] = out
            print(name, out, flush=True)
            film.close(); sc.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
