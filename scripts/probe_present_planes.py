"""pt_film_pack_planes / pt_film_unpack_planes beside a device-to-device copy of the same bytes, on one MI355X, as one JSON record under profiles/.

One GPU, emulated ranks; no multi-GPU hardware has run it: a 1920 x 1080 film with all eleven planes (PT_PLANES_ALL, 25 words per pixel) stands
in for every rank of world 8.
  pack     k_pack_planes of ONE rank's tiles (rank r of world 8, r cycling): 4050 records of 6400 B
  unpack   k_unpack_planes over ALL 32 400 records in one launch, as the root of pt_film_present_planes runs it; here through
           pt_film_unpack_planes(world = 1), whose tile list is row-major where the root's is the ranks' lists one after the other
  copy     torch's tensor.copy_ (hipMemcpyAsync, device to device) of the same byte count, straight after each of them in the same loop: the
           yardstick.  A copy reads and writes every byte once, as the kernels do.
Kernel times are per dispatch from ONE `rocprofv3 --kernel-trace -f csv` run of the measuring child (the standalone calls allocate and upload a
tile list, so events around them would time the host): the planes kernels by name, and the runtime's copy kernel that follows each of them in
start order.  The copies are also timed by device events in the same loop (these include the event pair's own few microseconds).  After a
warm-up of everything; median with min - max over --reps repetitions; ratio = kernel median / copy median.
Usage: python scripts/probe_present_planes.py [--reps 9] [--out profiles/present_planes_probe.json]"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H, WORLD = 1920, 1080, 8


def summary(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "n": len(us)}


def child(reps):
    import numpy as np
    import torch
    pt = importlib.import_module("single-file-vulkan-pathtracing_amd")
    ctx = pt.Context(0)
    dev = torch.device("cuda:0")
    film = pt.Film(ctx, W, H)
    dst = pt.Film(ctx, W, H)
    for f in (film, dst):
        f.enable_aov(); f.enable_moments(); f.enable_history(); f.enable_counts(); f.enable_motion()
    s = pt.film_planes_words(film, pt.PLANES_ALL)
    n_all = pt.film_tile_count(film, 0, 1)
    n_rank = [pt.film_tile_count(film, r, WORLD) for r in range(WORLD)]
    # the root's receive buffer, full of seeded words; unpacked into `film` it is also the film the packs read
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    recv = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_all, 64 * s), dtype=torch.int32, device=dev, generator=g)
    send = torch.empty((max(n_rank), 64 * s), dtype=torch.int32, device=dev)
    send_copy, recv_copy = torch.empty_like(send), torch.empty_like(recv)
    torch.cuda.synchronize()
    pt.film_unpack_planes(film, 0, 1, pt.PLANES_ALL, recv.data_ptr())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy(a, b):
        ev[0].record(); b.copy_(a); ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    copies = {"pack": [], "unpack": []}
    for k in range(2 + reps):   # two warm-up rounds, then the measured ones
        r = k % WORLD
        pt.film_pack_planes(film, r, WORLD, pt.PLANES_ALL, send.data_ptr())
        cp = copy(send[:n_rank[r]], send_copy[:n_rank[r]])
        pt.film_unpack_planes(dst, 0, 1, pt.PLANES_ALL, recv.data_ptr())
        cu = copy(recv, recv_copy)
        if k >= 2:
            copies["pack"].append(cp); copies["unpack"].append(cu)
    ok = bool((film.read_motion().view(np.uint32) == dst.read_motion().view(np.uint32)).all())
    print(json.dumps({"words_per_pixel": s, "tiles_rank": n_rank, "tiles_all": n_all, "bytes_pack": n_rank[0] * 256 * s, "bytes_unpack": n_all * 256 * s,
                      "copy_by_events": {k: summary(v) for k, v in copies.items()}, "round_trip_equal": ok}))
    film.close(); dst.close(); ctx.close()


def dispatches(trace_dir):
    """[(start ns, duration us, kernel name)] of the child, in start order"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, r["Kernel_Name"]))
    return sorted(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "present_planes_probe.json"))
    ap.add_argument("--keep-trace", metavar="DIR", help="keep rocprofv3's output here")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    if not shutil.which("rocprofv3"):
        raise SystemExit("rocprofv3 not found: nothing is measured")
    d = a.keep_trace or tempfile.mkdtemp(prefix="pp_trace_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"child failed ({r.returncode}): {r.stderr[-3000:]}")
        rec = {"probe": "present_planes", "caveat": "one GPU, emulated ranks; no multi-GPU hardware has run it", "image": [W, H], "world": WORLD, "planes": "PT_PLANES_ALL",
               "reps": a.reps}
        rec.update(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
        rows = dispatches(d)
        times = {"pack": [], "unpack": [], "copy_after_pack": [], "copy_after_unpack": []}
        last = None
        for _, us, name in rows:
            if "k_pack_planes" in name or "k_unpack_planes" in name:
                last = "unpack" if "k_unpack_planes" in name else "pack"
                times[last].append(us)
            elif last and "copy" in name.lower():   # the runtime's device-to-device copy kernel: the first one after a planes kernel is the loop's
                times["copy_after_" + last].append(us)
                last = None
        rec["copy_kernel_names"] = sorted({n for _, _, n in rows if "copy" in n.lower()})
        # the first unpack is the set-up's and the next two rounds are the warm-up
        for k, skip in (("pack", 2), ("unpack", 3), ("copy_after_pack", 2), ("copy_after_unpack", 3)):
            rec["kernel_" + k] = summary(times[k][skip:]) if len(times[k]) > skip else "not in the kernel trace: not measured"
        for side in ("pack", "unpack"):
            kk, cc = rec["kernel_" + side], rec["kernel_copy_after_" + side]
            if isinstance(kk, dict):
                rec["ratio_" + side + "_over_copy_kernel"] = round(kk["median_us"] / cc["median_us"], 2) if isinstance(cc, dict) else "not measured"
                rec["ratio_" + side + "_over_copy_events"] = round(kk["median_us"] / rec["copy_by_events"][side]["median_us"], 2)
                rec["gb_per_s_" + side] = round(2 * rec["bytes_" + side] / kk["median_us"] / 1e3, 1)   # read + written
    finally:
        if not a.keep_trace:
            shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
