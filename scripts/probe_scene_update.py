"""pt_scene_update: device ms (pt_scene_info.build_ms) and wall ms of create, REFIT and REBUILD, for the Cornell box, the 10 000-instance
grid and pt.make_soup at 1 M / 8 M triangles; then the ms per frame after a refit against a fresh scene of the same deformed arrays
(how far the refitted tree has degraded).  Usage: python scripts/probe_scene_update.py [--sizes cornell,grid,1m,8m] [--reps 3]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pt = importlib.import_module("single-file-vulkan-pathtracing_amd")


def deform(v, seed, amount):
    """every vertex moved by up to `amount` of the scene's extent (indices untouched)"""
    p = np.asarray(v, np.float32).reshape(-1, 3)
    ext = float((p.max(0) - p.min(0)).max())
    rng = np.random.default_rng(seed)
    return (p + rng.uniform(-amount, amount, p.shape).astype(np.float32) * np.float32(ext)).reshape(-1).astype(np.float32)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def frame_ms(ctx, scene, film, w, h, frames=4, **kw):
    p = pt.default_params(width=w, height=h, spp_per_frame=4, max_depth=5, frame=0, frame_count=1, **kw)
    pt.render(scene, film, p)                                # warm-up: plans, workspace
    t0 = time.perf_counter()
    for k in range(frames):
        pt.render(scene, film, pt.default_params(width=w, height=h, spp_per_frame=4, max_depth=5, frame=k, frame_count=1, **kw))
    return (time.perf_counter() - t0) * 1e3 / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="cornell,grid,1m,8m")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--amount", type=float, default=0.002, help="deformation: largest vertex move as a fraction of the scene extent")
    args = ap.parse_args()
    ctx = pt.Context(0)
    w, h = 960, 540
    film = pt.Film(ctx, w, h)
    for name in args.sizes.split(","):
        inst = None
        if name == "cornell":
            v, i, f = pt.load_obj(pt.ASSET_CORNELL)
        elif name == "grid":
            v, i, f = pt.load_obj(pt.ASSET_CORNELL)
            inst = pt.cornell_grid_instances()
        else:
            v, i, f = pt.make_soup({"1m": 1000000, "8m": 8000000}[name], 1)
        v2 = deform(v, 7, args.amount)
        create = []
        for _ in range(args.reps):
            sc, ms = timed(lambda: pt.Scene(ctx, v, i, f))
            if inst is not None:
                _, ms2 = timed(lambda: sc.set_instances(inst))
                ms += ms2
            create.append((round(sc.info().build_ms, 3), round(ms, 2)))
            sc.close()
        sc = pt.Scene(ctx, v, i, f)
        if inst is not None:
            sc.set_instances(inst)
        rows = {"create": create}
        for mode, label in ((pt.SCENE_UPDATE_REFIT, "refit"), (pt.SCENE_UPDATE_REBUILD, "rebuild")):
            out = []
            for r in range(args.reps):
                _, ms = timed(lambda: sc.update(v2 if r % 2 == 0 else v, i, mode=mode))
                out.append((round(sc.info().build_ms, 3), round(ms, 2)))
            rows[label] = out
        print(name, "device ms / wall ms:", rows, flush=True)
        # degradation: the same deformed arrays, refitted from the original tree vs built fresh
        sc.update(v, i, mode=pt.SCENE_UPDATE_REBUILD)
        sc.update(v2, i, mode=pt.SCENE_UPDATE_REFIT)
        fresh = pt.Scene(ctx, v2, i, f)
        if inst is not None:
            fresh.set_instances(inst)
        cam = dict(cam_origin=(0.0, -1.0, 1.2), cam_target=(0.0, -1.0, 0.0)) if inst is not None else {}
        a, b = frame_ms(ctx, sc, film, w, h, **cam), frame_ms(ctx, fresh, film, w, h, **cam)
        ia, ib = sc.info(), fresh.info()
        print(f"{name} ms/frame ({w}x{h}, 4 spp, depth 5) refit {a:.3f} fresh {b:.3f} ({a / b:.3f}x); tree_area_lbvh refit "
              f"{ia.tree_area_lbvh:.3f} fresh {ib.tree_area_lbvh:.3f}", flush=True)
        fresh.close(); sc.close()
    film.close(); ctx.close()


if __name__ == "__main__":
    main()
