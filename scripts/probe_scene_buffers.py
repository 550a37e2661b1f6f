"""The host paths that allocate a scene's device buffers, as one JSON line: device ms (pt_scene_info.build_ms) and wall ms of pt_scene_create
for the Cornell box and a 1 M-triangle soup, wall ms of pt_scene_set_instances for the 10 000-instance grid, device / wall ms of
pt_scene_update REFIT and REBUILD on the Cornell box.  Every figure is the median of --reps calls after one unrecorded call.  Run it in
separate processes, alternating two builds of the library through PT_LIB_AMD, to compare them (profiles/scene_buffers_refactor_ab.json).
Usage: python scripts/probe_scene_buffers.py [--reps 5] [--soup 1000000]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pt = importlib.import_module("single-file-vulkan-pathtracing_amd")


def medians(reps, fn):
    """fn() -> a tuple of figures; -> their medians over `reps` calls, after one call that is not recorded"""
    fn()
    rows = [fn() for _ in range(reps)]
    return [round(statistics.median(col), 4) for col in zip(*rows)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--soup", type=int, default=1000000)
    args = ap.parse_args()
    ctx = pt.Context(0)
    out = {"lib": os.environ.get("PT_LIB_AMD", "in-tree"), "reps": args.reps}

    def create(arrays):
        t0 = time.perf_counter()
        sc = pt.Scene(ctx, *arrays)
        wall = (time.perf_counter() - t0) * 1e3
        ms = sc.info().build_ms
        sc.close()
        return ms, wall

    cornell = pt.load_obj(pt.ASSET_CORNELL)
    out["create_cornell_build_ms"], out["create_cornell_wall_ms"] = medians(args.reps, lambda: create(cornell))
    soup = pt.make_soup(args.soup, 1)
    out["create_soup_build_ms"], out["create_soup_wall_ms"] = medians(args.reps, lambda: create(soup))

    sc = pt.Scene(ctx, *cornell)
    grid = pt.cornell_grid_instances()

    def set_instances():
        t0 = time.perf_counter()
        sc.set_instances(grid)
        return ((time.perf_counter() - t0) * 1e3,)

    out["set_instances_10000_wall_ms"], = medians(args.reps, set_instances)
    sc.set_instances(grid[:0])
    v, i, _ = cornell
    moved = (np.asarray(v, np.float32) + np.float32(0.001)).reshape(-1)   # (a translation: every fan pair still holds)

    def update(mode, flip=[0]):
        flip[0] ^= 1
        t0 = time.perf_counter()
        sc.update(moved if flip[0] else v, i, mode=mode)
        return sc.info().build_ms, (time.perf_counter() - t0) * 1e3

    out["refit_cornell_build_ms"], out["refit_cornell_wall_ms"] = medians(args.reps, lambda: update(pt.SCENE_UPDATE_REFIT))
    out["rebuild_cornell_build_ms"], out["rebuild_cornell_wall_ms"] = medians(args.reps, lambda: update(pt.SCENE_UPDATE_REBUILD))
    sc.close(); ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
