"""pt_film_motion and pt_film_reproject_motion: what the two calls cost beside pt_film_reproject and the step's own render, on one MI355X,
written as one JSON record under profiles/.

Two Cornell films of 1920 x 1080 with guides, second-moment plane, history length and motion plane: one rendered at the default camera
(step 0, reprojected with prev = NULL); then pt_scene_snapshot_previous, the short box moved by (0.02, 0, 0) through pt_scene_update, and the
second film rendered at frame 1 (4 spp, depth 8, PT_PIPELINE_AUTO, same camera).  A third pair does the same on a 16-instance grid of the box
with one instance's matrix changed (the INST instantiation).  Every ms figure is the call's own device events, median of --reps alternated
repetitions after a warm-up call of each leg, with min and max:
  motion / motion_inst        pt_film_motion (k_motion<false> / <true>)
  reproject_motion            pt_film_reproject_motion of the second film against the first (with M; gain 1, so that repeating the in-place
                              call keeps the film's values in range)
  reproject                   pt_film_reproject of the same pair
  render                      the step's own pt_render (one frame of 4 spp)
  snapshot_host_ms            pt_scene_snapshot_previous, host wall clock (a 1.7 KB device copy and a synchronise: the call's fixed cost)
  gbytes_per_s                the call's algorithmic bytes over its time (the events' time: launch overhead included).  pt_film_motion: 16 B of
                              guides read and 16 B of Q written per pixel (32 B; the gathered records are 36 triangles x 96 B, L2-resident, and
                              not counted); pt_film_reproject_motion: pt_film_reproject's 148 B plus 16 B of Q (164 B)
Usage: python scripts/probe_motion.py [--reps 5] [--out profiles/motion_probe.json]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H, SPP = 1920, 1080, 4
STEP = (0.02, 0.0, 0.0)
SHORT_BOX_VERTS = slice(30, 66)   # the loader de-indexes: the short box is triangles 10..21
BYTES = {"motion": 32, "motion_inst": 32, "reproject": 148, "reproject_motion": 164}


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def rate(bytes_per_pixel, ms):
    return round(bytes_per_pixel * W * H / (ms * 1e-3) / 1e9, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "motion_probe.json"))
    args = ap.parse_args()
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    v, i, f = pt.load_obj(pt.ASSET_CORNELL)
    v = np.asarray(v, np.float32).reshape(-1, 3)
    v1 = v.copy()
    v1[SHORT_BOX_VERTS] += np.asarray(STEP, np.float32)
    cam = {"cam_origin": tuple(pt.default_params().cam_origin), "cam_target": tuple(pt.default_params().cam_target)}
    grid_cam = dict(cam_origin=(-0.84, -1.99, 0.5), cam_target=(-0.84, -1.99, -19.5))   # a square of side 0.05 around three instances of the grid

    def film():
        fl = pt.Film(ctx, W, H)
        fl.enable_aov()
        fl.enable_moments()
        fl.enable_history()
        fl.enable_motion()
        return fl

    def step(sc, fl, frame, c):
        kw = dict(width=W, height=H, spp_per_frame=SPP, frame_count=1, pipeline=pt.PIPELINE_AUTO, **c)
        pt.render(sc, fl, pt.default_params(frame=frame, max_depth=8, **kw))
        pt.render_aov(sc, fl, pt.default_params(frame=0, **kw))

    sc = pt.Scene(ctx, v, i, f)
    a, b = film(), film()
    step(sc, a, 0, cam)
    a.reproject_motion(None, cam, cam)
    t0 = time.perf_counter()
    sc.snapshot_previous()
    snapshot_ms = (time.perf_counter() - t0) * 1e3
    sc.update(v1, i)
    step(sc, b, 1, cam)

    grid = pt.Scene(ctx, v, i, f)
    now = pt.cornell_grid_instances()[:16].copy()
    was = now.copy()
    was[7, 0, 3] -= np.float32(0.004)   # (an instance the camera below sees)
    grid.set_instances(was)
    grid.snapshot_previous()
    grid.set_instances(now)
    g = film()
    step(grid, g, 1, grid_cam)
    scratch = pt.Film(ctx, W, H)

    def render():
        before = ctx.stats().ms_total
        pt.render(sc, scratch, pt.default_params(frame=1, frame_count=1, width=W, height=H, spp_per_frame=SPP, max_depth=8, pipeline=pt.PIPELINE_AUTO, **cam))
        return ctx.stats().ms_total - before

    legs = {"motion": lambda: b.motion(sc, cam), "motion_inst": lambda: g.motion(grid, grid_cam),
            "reproject_motion": lambda: b.reproject_motion(a, cam, cam), "reproject": lambda: b.reproject(a, cam, cam), "render": render}
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            ms[k].append(fn())
    rec = {"image": [W, H], "spp": SPP, "box_step": list(STEP), "reps": args.reps, "snapshot_host_ms": round(snapshot_ms, 3)}
    rec.update({k: summary(x) for k, x in ms.items()})
    for k, bpp in BYTES.items():
        rec[k]["bytes_per_pixel"] = bpp
        rec[k]["gbytes_per_s"] = rate(bpp, rec[k]["median_ms"])
    q = b.read_motion()
    ids = b.read_aov(pt.AOV_ID)[..., 0]
    alpha = b.read_aov(pt.AOV_ALPHA)
    on_box = (ids >= 10) & (ids < 22)
    b.motion(sc, cam)
    b.reproject_motion(a, cam, cam)
    hist = b.read_history()
    rec["covered_pixels_with_q"] = round(float((q[..., 3] > 0)[alpha > 0].mean()), 4)
    rec["box_pixels"] = int(on_box.sum())
    rec["box_pixels_with_history"] = round(float((hist[on_box] > 1).mean()), 4)
    rec["motion_over_reproject"] = round(rec["motion"]["median_ms"] / rec["reproject"]["median_ms"], 4)
    rec["motion_plus_reproject_motion_over_render"] = round((rec["motion"]["median_ms"] + rec["reproject_motion"]["median_ms"]) / rec["render"]["median_ms"], 4)
    rec["pipeline"] = int(ctx.stats().pipeline)
    for fl in (a, b, g, scratch):
        fl.close()
    sc.close(); grid.close(); ctx.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec, indent=1))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
