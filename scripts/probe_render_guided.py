"""pt_render_guided: the single pass against the two calls it replaces, on one MI355X, written as one JSON record under profiles/.

Per shape one film with guide planes; the call in PT_GUIDED_SINGLE_PASS and in PT_GUIDED_TWO_CALLS (pt_render then pt_render_aov: the kernels as
they were), alternated in one loop after a warm-up of both: device ms by the calls' own events (the growth of pt_stats.ms_total, which for the
single pass spans the fused launches, k_resolve and the reduce, and for the two calls is the sum of both calls') and wall ms of the blocking
call, as the median of --reps repetitions with min and max; the reduce's own device time (pt_guided_result.guide_ms) beside them.
  wins   the single pass's median is below the two-call median by more than the two-call form's own min-max spread -- the condition under which
         PT_GUIDED_AUTO may take the single pass for that scene class
Shapes: the Cornell box at 1920 x 1080 with 32 spp x 1 frame, 4 spp x 1 frame and 32 spp x 16 frames; the 10 000-instance grid with 32 spp x 1 frame.
Usage: python scripts/probe_render_guided.py [--reps 5] [--out profiles/render_guided_probe.json]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_guided_probe.json"))
    a = ap.parse_args()
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    v, i, f = pt.load_obj(pt.ASSET_CORNELL)
    box = pt.Scene(ctx, v, i, f)
    grid = pt.Scene(ctx, v, i, f)
    grid.set_instances(pt.cornell_grid_instances())
    shapes = [("cornell_1080p_32spp_x1", box, 32, 1), ("cornell_1080p_4spp_x1", box, 4, 1), ("cornell_1080p_32spp_x16", box, 32, 16),
              ("grid10000_1080p_32spp_x1", grid, 32, 1)]
    out = {"probe": "render_guided", "width": W, "height": H, "reps": a.reps, "shapes": {}}
    for name, sc, spp, frames in shapes:
        film = pt.Film(ctx, W, H)
        film.enable_aov()
        p = pt.default_params(width=W, height=H, spp_per_frame=spp, max_depth=8, frame=0, frame_count=frames, pipeline=pt.PIPELINE_AUTO)

        def timed(mode):
            ctx.sync()
            before = ctx.stats().ms_total
            t0 = time.perf_counter()
            res = pt.render_guided(sc, film, p, mode=mode)
            wall = (time.perf_counter() - t0) * 1e3
            return ctx.stats().ms_total - before, wall, res

        modes = {"single_pass": pt.GUIDED_SINGLE_PASS, "two_calls": pt.GUIDED_TWO_CALLS}
        for m in list(modes.values()) * 2:   # warm-up, two rounds: workspaces, the log, kernel attributes, clocks
            timed(m)
        dev = {k: [] for k in modes}
        wall = {k: [] for k in modes}
        guide = {k: [] for k in modes}
        launches = {}
        for _ in range(a.reps):
            for k, m in modes.items():
                d, w_, res = timed(m)
                dev[k].append(d); wall[k].append(w_); guide[k].append(res.guide_ms)
                launches[k] = res.launches
                assert res.single_pass == (1 if k == "single_pass" else 0)
        rec = {"spp": spp, "frames": frames, "pipeline": pt.PIPELINE_NAMES[ctx.stats().pipeline], "fused_launches": launches["single_pass"],
               "log_mb": round(8 * ((W + 7) // 8) * ((H + 7) // 8) * 64 * spp * min(frames, max(ctx.stats().frames_in_flight, 1)) / 2 ** 20, 1)}
        for k in modes:
            rec[k] = {"device": summary(dev[k]), "wall": summary(wall[k]), "guide": summary(guide[k])}
        for what in ("device", "wall"):
            two, one = rec["two_calls"][what], rec["single_pass"][what]
            rec[what + "_saved_ms"] = round(two["median_ms"] - one["median_ms"], 4)
            rec[what + "_wins"] = bool(two["median_ms"] - one["median_ms"] > two["max_ms"] - two["min_ms"])
        out["shapes"][name] = rec
        print(name, json.dumps(rec), flush=True)
        film.close()
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    box.close(); grid.close(); ctx.close()


if __name__ == "__main__":
    main()
