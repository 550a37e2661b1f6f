"""pt_crossings_device on one MI355X: the LDS form against the GLOBAL form, as one JSON record under profiles/ (DESIGN.md section 32).

Shapes: the Cornell box with 2^20 and 2^24 rays (both forms); the 1 M-triangle soup with 2^20 and 2^24 rays (GLOBAL only: its image is far
beyond LDS).  Rays: origins on a lattice over the scene's box in lattice order, directions towards a second lattice point a fixed stride away
("coherent": neighbours in memory are neighbours in space and direction), and a shuffled copy.  Range (0.001, +inf).  Per shape the forms are
alternated in one loop, two warm-up passes, then --reps (7) timed ones: device_ms of the call (its own events), median with min .. max; once
per shape the two forms' outputs are compared byte for byte.  `lds_wins`: the LDS form's MAX lies below the GLOBAL form's MIN.
`auto_takes_lds`: true only if lds_wins on EVERY box shape -- what PT_CROSSINGS_AUTO may take (crossings.hip CX_AUTO_TAKES_LDS).
For scale, not for any threshold: pt_trace_device in PT_TRACE_ANY and PT_TRACE_CLOSEST mode (PT_TRACE_AUTO form) on the same rays, in the same loop.
Usage: python scripts/probe_crossings.py [--reps 7] [--small] [--out profiles/crossings_probe.json]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
f32 = np.float32
TMIN = 0.001


def summary(x, unit="ms"):
    return {"median_" + unit: round(statistics.median(x), 4), "min_" + unit: round(min(x), 4), "max_" + unit: round(max(x), 4), "n": len(x)}


def ray_set(tris, n):
    """[n, 6] float32 in lattice order: origin = lattice point k of the scene's box, direction = towards lattice point (k * 7 + 3) mod n, normalised"""
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    side = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.linspace(0.02, 0.98, side, dtype=f32)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    o = (lo + g * (hi - lo)).astype(f32)
    k = (np.arange(n, dtype=np.int64) * 7 + 3) % n
    d = o[k] - o + f32(1e-3)
    d /= np.maximum(np.linalg.norm(d, axis=1), 1e-20)[:, None]
    return np.ascontiguousarray(np.concatenate([o, d.astype(f32)], 1), f32)


def child(reps, small):
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    dev = torch.device("cuda:0")
    ctx = pt.Context(0)
    rec = {"shapes": {}, "tuning": {k: int(getattr(ctx.tuning(), k)) for k in ("refill", "lds_stack", "extend_blocks")}}
    bv, bi, bf = pt.load_obj(pt.ASSET_CORNELL)
    sv, si, sf = pt.make_soup((1 << 14) if small else (1 << 20), 1)
    sizes = [1 << 14, 1 << 16] if small else [1 << 20, 1 << 24]
    scenes = [("cornell", (bv, bi, bf), ("lds", "global")), ("soup_1m", (sv, si, sf), ("global",))]
    forms = {"lds": pt.CROSSINGS_LDS, "global": pt.CROSSINGS_GLOBAL}
    auto = True
    for name, (v, i, f), which in scenes:
        v, i, f = (np.ascontiguousarray(v, f32).reshape(-1), np.ascontiguousarray(i, np.uint32).reshape(-1), np.ascontiguousarray(f, f32).reshape(-1))
        scene = pt.Scene(ctx, v, i, f)
        tris = v.reshape(-1, 3)[i.reshape(-1, 3)]
        for n in sizes:
            base = ray_set(tris, n)
            for order in ("coherent", "shuffled"):
                r6 = base[np.random.default_rng(5).permutation(n)] if order == "shuffled" else base
                t = torch.from_numpy(np.ascontiguousarray(r6)).to(dev)
                outs = {k: (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)) for k in which}
                occ = torch.empty(n, dtype=torch.uint8, device=dev)
                hits = torch.empty((n, 5), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                runs = {k: (lambda k=k: scene.crossings_device(n, rays_ptr=t.data_ptr(), count_ptr=outs[k][0].data_ptr(), winding_ptr=outs[k][1].data_ptr(),
                                                                 tmin=TMIN, form=forms[k])) for k in which}
                runs["trace_any"] = lambda: scene.trace_device(n, t.data_ptr(), occluded_ptr=occ.data_ptr(), mode=pt.TRACE_ANY, tmin=TMIN, flags=pt.TRACE_AUTO)
                runs["trace_closest"] = lambda: scene.trace_device(n, t.data_ptr(), hits_ptr=hits.data_ptr(), mode=pt.TRACE_CLOSEST, tmin=TMIN, flags=pt.TRACE_AUTO)
                m = {k: [] for k in runs}
                for r in range(2 + reps):   # two warm-up passes, then the measured ones, everything alternated
                    for k, fn in runs.items():
                        ms = fn()
                        if r >= 2:
                            m[k].append(ms)
                row = {k: summary(x) for k, x in m.items()}
                for k in which:
                    row["mrays_per_s_" + k] = round(n / row[k]["median_ms"] / 1e3, 1)
                c = outs[which[-1]][0]
                row["mean_count"] = round(float(c.float().mean()), 3)
                row["max_count"] = int(c.max())
                row["occluded_equals_count_gt_0"] = bool(torch.equal(occ.bool(), c > 0))
                if len(which) == 2:
                    a, b = outs["lds"], outs["global"]
                    row["bytes_equal"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
                    row["lds_wins"] = bool(row["lds"]["max_ms"] < row["global"]["min_ms"])
                    row["global_over_lds"] = round(row["global"]["median_ms"] / row["lds"]["median_ms"], 3)
                    auto = auto and row["lds_wins"] and row["bytes_equal"]
                rec["shapes"][f"{name}/{n}/{order}"] = row
                print(f"{name}/{n}/{order}", json.dumps(row), file=sys.stderr, flush=True)   # (progress; the record is the last stdout line)
                del t, outs, occ, hits, runs
        scene.close()
    rec["auto_takes_lds"] = auto
    print(json.dumps(rec))
    ctx.close()
    differ = [k for k, row in rec["shapes"].items() if row.get("bytes_equal") is False]
    if differ:   # the record is printed and kept, and the run fails: the two forms must agree byte for byte
        raise SystemExit(f"the LDS and the GLOBAL form differ on {differ}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a quick pass over small shapes (a check of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "crossings_probe.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.small)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--small"] if a.small else []),
                       stdout=subprocess.PIPE, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if not lines:
        raise SystemExit(f"child failed ({r.returncode})")
    rec = {"probe": "crossings", "reps": a.reps, "small": a.small, "child_status": r.returncode}
    rec.update(json.loads(lines[-1]))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    if r.returncode != 0:   # (the forms' outputs differ, or the child died after its record: the record is kept, the run fails)
        raise SystemExit(f"child failed ({r.returncode})")


if __name__ == "__main__":
    main()
