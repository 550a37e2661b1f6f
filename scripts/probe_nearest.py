"""pt_nearest_device on one MI355X: the LDS form against the GLOBAL form, as one JSON record under profiles/ (DESIGN.md section 31).

Shapes: the Cornell box with 2^20 and 2^24 queries (both forms); the 1 M-triangle soup with 2^20 queries (GLOBAL only: its image is far beyond
LDS).  Query sets: `uniform` -- a lattice over 1.5x the scene's box, in lattice order -- and `surface` -- points on the triangles, in triangle
order, moved along the normal by up to 1 % of the box's diagonal; each in generation order ("coherent") and as a shuffled copy.  Per shape the
forms are alternated in one loop, two warm-up passes, then --reps (7) timed ones: device_ms of the call (its own events), median with min ..
max; once per shape the two forms' outputs are compared byte for byte.  `lds_wins`: the LDS form's MAX lies below the GLOBAL form's MIN.
`auto_takes_lds`: true only if lds_wins on EVERY box shape -- what PT_NEAREST_AUTO may take (nearest.hip NR_AUTO_TAKES_LDS).
For scale, not for any threshold: a brute-force torch evaluation (float32, all triangles per query, chunked) of the box's 2^20 uniform queries.
--sweep: the refill threshold and the blocks per CU on the box's 2^20 shuffled uniform queries, both forms (medians of --reps).
Usage: python scripts/probe_nearest.py [--reps 7] [--small] [--sweep] [--out profiles/nearest_probe.json]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
f32 = np.float32


def summary(x, unit="ms"):
    return {"median_" + unit: round(statistics.median(x), 4), "min_" + unit: round(min(x), 4), "max_" + unit: round(max(x), 4), "n": len(x)}


def query_sets(tris, n):
    """-> {"uniform": [n, 3], "surface": [n, 3]} float32, in generation order"""
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    side = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.linspace(-1, 1, side, dtype=f32)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    uniform = (c + g * h).astype(f32)
    rng = np.random.default_rng(3)
    t = np.sort(rng.integers(0, len(tris), n))
    b = rng.dirichlet((1, 1, 1), n).astype(f32)
    p = (tris[t] * b[:, :, None]).sum(1)
    nrm = np.cross(tris[t, 1] - tris[t, 0], tris[t, 2] - tris[t, 0]).astype(np.float64)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1), 1e-30)[:, None]
    off = rng.uniform(-0.01, 0.01, n) * float(np.linalg.norm(hi - lo))
    return {"uniform": np.ascontiguousarray(uniform), "surface": np.ascontiguousarray((p + nrm * off[:, None]).astype(f32))}


def torch_brute(torch, tris_t, pts, chunk=1 << 16):
    """closest squared distance by the same region algorithm, float32, every triangle per query (the scale, not a reference: torch may contract)"""
    A, B, C = tris_t[None, :, 0], tris_t[None, :, 1], tris_t[None, :, 2]
    ab, ac = B - A, C - A
    out = torch.empty(len(pts), dtype=torch.float32, device=pts.device)
    for i0 in range(0, len(pts), chunk):
        P = pts[i0:i0 + chunk, None, :]
        ap, bp, cp = P - A, P - B, P - C
        d1, d2, d3, d4, d5, d6 = (ab * ap).sum(-1), (ac * ap).sum(-1), (ab * bp).sum(-1), (ac * bp).sum(-1), (ab * cp).sum(-1), (ac * cp).sum(-1)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e, f = d4 - d3, d5 - d6
        w, s = e / (e + f), va + vb + vc
        u, v = vb / s, vc / s
        zero, one = torch.zeros_like(u), torch.ones_like(u)
        for cond, uu, vv in reversed([((d1 <= 0) & (d2 <= 0), zero, zero), ((d3 >= 0) & (d4 <= d3), one, zero),
                                      ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero), ((d6 >= 0) & (d5 <= d6), zero, one),
                                      ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)), ((va <= 0) & (e >= 0) & (f >= 0), 1 - w, w)]):
            u, v = torch.where(cond, uu, u), torch.where(cond, vv, v)
        D = P - (A + ab * u[..., None] + ac * v[..., None])
        out[i0:i0 + chunk] = torch.nan_to_num((D * D).sum(-1), nan=float("inf")).min(1).values
    return out


def child(reps, small, sweep):
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    dev = torch.device("cuda:0")
    ctx = pt.Context(0)
    rec = {"shapes": {}, "tuning": {k: int(getattr(ctx.tuning(), k)) for k in ("refill", "lds_stack", "extend_blocks")}}
    bv, bi, bf = pt.load_obj(pt.ASSET_CORNELL)
    sv, si, sf = pt.make_soup((1 << 14) if small else (1 << 20), 1)
    scenes = [("cornell", (bv, bi, bf), [1 << 14, 1 << 16] if small else [1 << 20, 1 << 24], ("lds", "global")),
              ("soup_1m", (sv, si, sf), [1 << 14] if small else [1 << 20], ("global",))]
    forms = {"lds": pt.NEAREST_LDS, "global": pt.NEAREST_GLOBAL}
    auto = True

    def timed(scene, t, rec_t, point_t, form):
        return scene.nearest_device(len(t), t.data_ptr(), nearest_ptr=rec_t.data_ptr(), point_ptr=point_t.data_ptr(), form=forms[form])

    for name, (v, i, f), sizes, which in scenes:
        v, i, f = (np.ascontiguousarray(v, f32).reshape(-1), np.ascontiguousarray(i, np.uint32).reshape(-1), np.ascontiguousarray(f, f32).reshape(-1))
        scene = pt.Scene(ctx, v, i, f)
        tris = v.reshape(-1, 3)[i.reshape(-1, 3)]
        for n in sizes:
            for kind, pts in query_sets(tris, n).items():
                for order in ("coherent", "shuffled"):
                    p = pts[np.random.default_rng(5).permutation(n)] if order == "shuffled" else pts
                    t = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
                    outs = {k: (torch.empty((n, 4), dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)) for k in which}
                    torch.cuda.synchronize()
                    m = {k: [] for k in which}
                    for r in range(2 + reps):   # two warm-up passes, then the measured ones, the forms alternated
                        for k in which:
                            ms = timed(scene, t, *outs[k], k)
                            if r >= 2:
                                m[k].append(ms)
                    row = {k: summary(x) for k, x in m.items()}
                    for k in which:
                        row["mqueries_per_s_" + k] = round(n / row[k]["median_ms"] / 1e3, 1)
                    if len(which) == 2:
                        a, b = outs["lds"], outs["global"]
                        row["bytes_equal"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
                        row["lds_wins"] = bool(row["lds"]["max_ms"] < row["global"]["min_ms"])
                        row["global_over_lds"] = round(row["global"]["median_ms"] / row["lds"]["median_ms"], 3)
                        auto = auto and row["lds_wins"] and row["bytes_equal"]
                    if name == "cornell" and n == sizes[0] and kind == "uniform" and order == "coherent":
                        tt = torch.from_numpy(tris).to(dev)
                        ts = []
                        for r in range(3):
                            torch.cuda.synchronize(); t0 = time.perf_counter()
                            d = torch_brute(torch, tt, t)
                            torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
                        got = outs[which[0]][0].view(torch.float32)[:, 1]
                        row["torch_brute_force"] = dict(summary(ts[1:]), max_abs_diff_dist2=float((d - got).abs().max()))
                    rec["shapes"][f"{name}/{n}/{kind}/{order}"] = row
                    print(f"{name}/{n}/{kind}/{order}", json.dumps(row), file=sys.stderr, flush=True)   # (progress; the record is the last stdout line)
                    del t, outs
        if sweep and name == "cornell":
            n = sizes[0]
            p = query_sets(tris, n)["uniform"][np.random.default_rng(5).permutation(n)]
            t = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
            out = (torch.empty((n, 4), dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev))
            sw = {}
            for knob, values in (("refill", (1, 8, 16, 32, 48, 64)), ("extend_blocks", (1, 2, 4, 6, 8))):
                for val in values:
                    old = ctx.set_tuning(**{knob: val})
                    for k in which:
                        ms = [timed(scene, t, *out, k) for _ in range(2 + reps)][2:]
                        sw[f"{knob}={val}/{k}"] = summary(ms)
                    ctx.set_tuning(**old)
            rec["sweep"] = sw
        scene.close()
    rec["auto_takes_lds"] = auto
    print(json.dumps(rec))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="a quick pass over small shapes (a check of the script, not a measurement)")
    ap.add_argument("--sweep", action="store_true", help="also sweep pt_tuning.refill and extend_blocks on the box")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nearest_probe.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.small, a.sweep)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)] + (["--small"] if a.small else []) +
                       (["--sweep"] if a.sweep else []), stdout=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"child failed ({r.returncode})")
    rec = {"probe": "nearest", "reps": a.reps, "small": a.small}
    rec.update(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
