"""pt_render_adaptive: what the selection costs, what the count blend costs beside pt_render, and what a threshold run saves, on one MI355X,
written as one JSON record under profiles/.

A 1920 x 1080 Cornell film (PT_PIPELINE_AUTO, --spp samples per frame, depth 8) with the planes M and K.
  select         device ms of the selection pass alone (pt_adaptive_result.select_ms of dry runs, frame_count = 0) on a film that holds
                 four frames: median, min, max of --reps calls
  all_selected   one frame through pt_render_adaptive with every tile selected (min_frames = 65535) against the same frame through pt_render
                 on a film with M, alternated in one loop: device ms (pt_stats.ms_total of the call, which for the adaptive call excludes the
                 selection; select_ms is added) and wall ms of the blocking call.  The difference is the feature's overhead: the selection, one
                 small read-back, and the count blend.
  threshold_run  passes of --steps frames at --threshold until a dry run selects nothing (or --passes passes): per pass the tiles selected, the
                 worst tile error and the rays; then the rays, the device ms and the wall ms of the whole run
  uniform_run    every tile in every pass of --steps frames (min_frames = 65535) until the worst tile error (a dry run's max_error) is at or
                 below what threshold_run ended with: the uniform render of the same quality by the selection's own measure
The default threshold is 0.15, not the library's 0.05: without next-event estimation the box's small light leaves a 1080p tile at 32 spp per
frame near 1.2 / sqrt(frames), so 0.05 takes some 600 frames and 0.15 ends within the pass limit.
Usage: python scripts/probe_adaptive.py [--reps 7] [--spp 32] [--threshold 0.15] [--steps 4] [--passes 48] [--out profiles/adaptive_probe.json]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H = 1920, 1080


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=0.15)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--passes", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adaptive_probe.json"))
    a = ap.parse_args()
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))

    def params(frame, count):
        return pt.default_params(width=W, height=H, spp_per_frame=a.spp, max_depth=8, frame=frame, frame_count=count, pipeline=pt.PIPELINE_AUTO)

    def film_mk():
        f = pt.Film(ctx, W, H)
        f.enable_moments()
        f.enable_counts()
        return f

    def timed(fn):
        """-> (device ms of the call by pt_stats.ms_total, wall ms, what fn returned)"""
        ctx.sync()
        before = ctx.stats().ms_total
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        return ctx.stats().ms_total - before, wall, r

    out = {"device": "MI355X", "width": W, "height": H, "spp": a.spp, "max_depth": 8, "pipeline": "auto", "threshold": a.threshold, "steps": a.steps}

    # ---- the selection alone, and the all-selected call against pt_render -------------------------------------------------------------
    film, plain = film_mk(), pt.Film(ctx, W, H)
    plain.enable_moments()
    pt.render_adaptive(sc, film, params(0, 4))
    pt.render(sc, plain, params(0, 4))
    sel = [pt.render_adaptive(sc, film, params(4, 0), threshold=a.threshold).select_ms for _ in range(a.reps + 1)][1:]
    out["select"] = summary(sel)
    legs = {"adaptive_device": [], "adaptive_wall": [], "adaptive_select": [], "render_device": [], "render_wall": []}
    for rep in range(a.reps + 1):
        frame = 4 + rep
        d, wl, r = timed(lambda: pt.render_adaptive(sc, film, params(frame, 1), min_frames=65535))
        assert r.tiles_selected == r.tiles_total
        d2, wl2, _ = timed(lambda: pt.render(sc, plain, params(frame, 1)))
        if rep:   # (the first pair warms both legs up)
            legs["adaptive_device"].append(d + r.select_ms); legs["adaptive_wall"].append(wl); legs["adaptive_select"].append(r.select_ms)
            legs["render_device"].append(d2); legs["render_wall"].append(wl2)
    out["all_selected"] = {k: summary(v) for k, v in legs.items()}
    out["all_selected"]["overhead_device_ms"] = round(statistics.median(legs["adaptive_device"]) - statistics.median(legs["render_device"]), 4)
    out["all_selected"]["overhead_wall_ms"] = round(statistics.median(legs["adaptive_wall"]) - statistics.median(legs["render_wall"]), 4)
    film.close(); plain.close()

    # ---- a threshold run to exhaustion, and the uniform render that reaches the same worst tile error -----------------------------------
    def run(adaptive_kw, stop):
        f = film_mk()
        ctx.reset_stats()
        passes, frame, dev, wall, last = [], 0, 0.0, 0.0, None
        for _ in range(a.passes):
            d, wl, q = timed(lambda: pt.render_adaptive(sc, f, params(frame, 0), threshold=a.threshold))   # the convergence query
            dev += q.select_ms; wall += wl
            last = q
            if stop(q, frame):
                break
            rays0 = ctx.stats().rays
            d, wl, r = timed(lambda: pt.render_adaptive(sc, f, params(frame, a.steps), **adaptive_kw))
            dev += d + r.select_ms; wall += wl
            frame += a.steps
            passes.append({"tiles": r.tiles_selected, "worst_tile_error": round(r.max_error, 5), "rays": ctx.stats().rays - rays0})
        st = ctx.stats()
        res = {"passes": passes, "frames": frame, "rays": st.rays, "paths": st.paths, "device_ms": round(dev, 3), "wall_ms": round(wall, 3),
               "tiles_total": last.tiles_total, "tiles_left": last.tiles_selected, "worst_tile_error_left": round(last.max_error, 5)}
        f.close()
        return res

    thr = run(dict(threshold=a.threshold), lambda q, frame: frame > 0 and q.tiles_selected == 0)
    target = max(thr["worst_tile_error_left"], 1e-9)
    uni = run(dict(min_frames=65535), lambda q, frame: frame > 0 and q.max_error <= target)
    out["threshold_run"], out["uniform_run"] = thr, uni
    out["rays_ratio_uniform_over_adaptive"] = round(uni["rays"] / max(thr["rays"], 1), 3)
    out["device_ms_ratio_uniform_over_adaptive"] = round(uni["device_ms"] / max(thr["device_ms"], 1e-9), 3)
    sc.close(); ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    brief = {k: out[k] for k in ("select", "rays_ratio_uniform_over_adaptive", "device_ms_ratio_uniform_over_adaptive")}
    brief["overhead_device_ms"] = out["all_selected"]["overhead_device_ms"]
    brief["threshold_run"] = {k: thr[k] for k in ("frames", "rays", "device_ms", "tiles_left", "worst_tile_error_left")}
    brief["uniform_run"] = {k: uni[k] for k in ("frames", "rays", "device_ms", "worst_tile_error_left")}
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
