"""The premises of tests/test_ray_range.py, on the CPU oracle alone (tests/range_cases.py has the recipes): per scene enough rays hit under every
kind of bound and the oracle puts a hit ON the bound outside the range and one ulp beyond it inside; the bundle's rays share their t bit for bit
and the four ends behave as the header says; and on the six-triangle scene the rule "a shadow ray ends at 0.999 dist" and the rule "... at
min(0.999 dist, tmax)" give different films in every pixel, so a film equal to the oracle's tells them apart."""
import numpy as np
import pytest

import range_cases as rc

f32 = np.float32
MISS = rc.MISS


@pytest.mark.parametrize("scene", ["box", "soup", "inst", "six"])
def test_bound_kinds_on_the_oracle(orc, cornell_arrays, scene):
    case = {"box": lambda: rc.box_case(orc, cornell_arrays), "soup": lambda: rc.soup_case(orc), "inst": lambda: rc.inst_case(orc, cornell_arrays),
            "six": lambda: rc.six_case(orc)}[scene]()
    assert case.n == 1000
    case.premises()
    # the bounds are what the table says, bit for bit
    k, t, hit = case.kind, case.hits["t"], case.hit
    assert (case.bounds[(k == 0) & hit] == t[(k == 0) & hit]).all()
    assert (case.bounds[(k == 1) & hit].view(np.uint32) == t[(k == 1) & hit].view(np.uint32) + 1).all()
    assert (case.bounds[(k == 2) & hit].view(np.uint32) == t[(k == 2) & hit].view(np.uint32) - 1).all()
    assert (case.bounds[(k == 3) & hit] == f32(2.0) * t[(k == 3) & hit]).all()
    assert (case.bounds[(k < 4) & ~hit] == f32(1.0)).all()
    assert (case.bounds[k == 4] == rc.TMIN).all() and (case.bounds[k == 5].view(np.uint32) == rc.TMIN.view(np.uint32) + 1).all()
    assert (case.bounds[k == 6] == f32(-1.0)).all() and np.isposinf(case.bounds[k == 7]).all()
    if scene == "inst":
        assert set(np.unique(case.hits["inst"][hit])) == {0, 1, 2}
    if scene == "six":
        assert set(np.unique(case.hits["prim"][hit]).tolist()) >= {2, 3, 4, 5}      # both triangles of the occluder and of the emitter


def test_box_first_thousand_rays(orc, cornell_arrays):
    """59.5 % of the box's rays hit; with bound = t none of them is occluded, with nextup(t) all, with nextdown(t) none (every ray, not one kind)"""
    case = rc.box_case(orc, cornell_arrays)
    osc = orc.Scene(*cornell_arrays)
    assert int(case.hit.sum()) == 595
    ix = np.flatnonzero(case.hit)
    for name, bound, want in (("t", case.hits["t"], 0), ("up", rc.nextup(case.hits["t"]), 1), ("down", rc.nextdown(case.hits["t"]), 0)):
        got = [int(osc.trace(case.rays[i], tmin=float(rc.TMIN), tmax=float(bound[i]), mode=0)[0]["prim"][0] != MISS) for i in ix]
        assert got == [want] * len(ix), name


def test_bundle_on_the_oracle(orc, cornell_arrays):
    b = rc.bundle(orc, cornell_arrays)
    assert b.n == 1024 and (b.hits["prim"] != MISS).all()
    for g, ((t, count), (_, ix)) in enumerate(zip(rc.BUNDLE_GROUPS, b.groups)):
        assert len(ix) == count, (g, len(ix))
        miss = lambda h: (h["prim"][ix] == MISS).all()
        same = lambda h: (h["prim"][ix] == b.hits["prim"][ix]).all() and (h["t"][ix] == t).all()
        assert miss(b.ends[g, "tmax=t"][2]) and same(b.ends[g, "tmax=up"][2]) and miss(b.ends[g, "tmin=t"][2]) and same(b.ends[g, "tmin=down"][2]), g
        assert (b.uniform[g, "t"][1][ix] == 0).all() and (b.uniform[g, "up"][1][ix] == 1).all() and (b.uniform[g, "down"][1][ix] == 0).all()
        # ... and under the bounds that hide the group the bundle still has both answers (the rays that stop at the blocks are occluded)
        assert all(set(np.unique(b.uniform[g, name][1])) == {0, 1} for name in ("t", "down")), g
    # a tmin at the hit: the rays of the group go on to what lies behind it or to nothing -- never to the same t
    for g in range(len(rc.BUNDLE_GROUPS)):
        h = b.ends[g, "tmin=t"][2]
        assert (h["t"][h["prim"] != MISS] > rc.BUNDLE_GROUPS[g][0]).all()


def test_six_triangles_separate_the_two_shadow_ranges(orc):
    """frame 0 at tmax = 2.0: the oracle's film == the Python restatement with the shadow ray cut at 0.999 dist (so the restatement is the
    oracle's), and the restatement with the cut at min(0.999 dist, tmax) differs from it in 384 of 384 pixels; at tmax = 10000 the two are one.
    Why: every light sample seen from the wall has the occluder between tmax and 0.999 dist."""
    osc, (v, idx, faces) = rc.six_oracle(orc)
    lights, area = rc.six_lights(v, idx, faces)
    assert len(lights) == 2 and area == f32(1.0)
    bound_only, with_tmax = (lambda b, tmax: b), min
    for tmax in (rc.SIX_TMAX, 10000.0):
        p = orc.default_params(frame=0, nee=1, tmax=tmax, **rc.SIX_RENDER)
        want, _, _, first = osc.render_frame(p, want_first_hits=True)
        log = []
        a = rc.nee_frame(orc, osc, lights, area, p, bound_only, log)
        assert a.tobytes() == want.tobytes(), tmax
        b = rc.nee_frame(orc, osc, lights, area, p, with_tmax)
        differ = int((a != b).any(2).sum())
        if tmax == 10000.0:
            assert differ == 0
            continue
        assert differ == 384 and abs(float(a.mean()) - 0.490) < 0.001 and abs(float(b.mean()) - 0.634) < 0.001, (differ, a.mean(), b.mean())
        # every camera ray sees the wall (prims 0, 1) closer than tmax, and its light sample runs from z = 0 to the emitter at z = 4: where it
        # crosses z = 3 (at 3/4 of its length, beyond tmax and before 0.999 dist) it is inside the occluder's square -- for the first light sample of every pixel
        assert set(np.unique(first["prim"])) <= {0, 1} and (first["t"] < f32(tmax)).all()
        assert len(log) == 384
        inside = 0
        for px, py, pos, wi, dist in log:
            assert abs(pos[2]) < 1e-6 and wi[2] > 0
            t3 = 3.0 / float(wi[2])
            assert tmax < t3 < 0.999 * float(dist)
            x, y = float(pos[0]) + t3 * float(wi[0]), float(pos[1]) + t3 * float(wi[1])
            inside += abs(x) < 1.0 and abs(y) < 1.0
        assert inside == len(log)


# ---- the accept rule itself, compiled for the host (csrc/hit_rule.h through tests/range_host.cpp) ------------------------------------------------
def _twin_cases():
    """(tmin, tmax, bound, t) float32: every t among {one ulp below, on, one ulp above} each of tmin, tmax and the bound, a few values between, and a
    NaN -- under call tmax 1.0 and 10000, bounds below, on and beyond them, +inf, at and below tmin, zero and negative"""
    tmin, inf = rc.TMIN, f32(np.inf)
    down = lambda x: np.nextafter(f32(x), -inf)
    rows = []
    for tmax in (f32(1.0), f32(10000.0)):
        for b in (f32(0.5), f32(1.0), f32(4.04), f32(100.0), f32(10000.0), f32(20000.0), inf, rc.nextup(tmin), tmin, f32(0.0), f32(-1.0)):
            ts = {f32(0.0005), f32(0.75), f32(2.0), f32(5000.0), f32(15000.0), f32(np.nan)}
            for e in (tmin, tmax, b):
                ts |= {down(e), f32(e), np.nextafter(f32(e), inf)}
            rows += [(tmin, tmax, b, t) for t in sorted(ts, key=lambda x: (np.isnan(x), x))]
    return [np.ascontiguousarray(c, f32) for c in zip(*rows)]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_twin_of_the_accept_rule(tmp_path, sanitize):
    """A walk that has hit nothing yet (best_t = the bound, best_pos = MISS) is offered a triangle at t.  With the leaf test ending at leaf_upper the
    any-hit walks take it exactly when tmin < t < bound; with the leaf test ending at tmax, as before, they also took t == bound and refused
    tmax <= t < bound -- the two findings, and nothing else.  The closest-hit walks take tmin < t < tmax, and a second triangle at the same t
    exactly when its (instance, primitive) id is lower."""
    import os, shutil, subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(repo, "single-file-vulkan-pathtracing_amd", "csrc")
    exe = str(tmp_path / "range_host")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++20", "-ffp-contract=off"] + flags +
                          ["-I", csrc, "-I", os.path.join(repo, "tests"), "-o", exe, os.path.join(repo, "tests", "range_host.cpp")])
    tmin, tmax, bound, t = _twin_cases()
    d = str(tmp_path)
    np.asarray([len(t)], np.uint32).tofile(os.path.join(d, "par"))
    for name, a in (("tmin", tmin), ("tmax", tmax), ("bound", bound), ("t", t)):
        a.tofile(os.path.join(d, name))
    r = subprocess.run([exe, d], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    with np.errstate(invalid="ignore"):
        header_any = (t > tmin) & (t < bound)                       # include/pt_api.h, PT_TRACE_ANY
        header_closest = (t > tmin) & (t < tmax)
        on_bound = (t == bound) & header_closest                    # finding 1
        cut_by_tmax = (t >= tmax) & header_any                      # finding 2
    assert header_any.sum() > 40 and on_bound.sum() >= 6 and cut_by_tmax.sum() >= 20 and (~header_any & ~on_bound).sum() > 100
    for rule in ("single", "inst"):
        got = {k: np.fromfile(os.path.join(d, f"o_{k}_{rule}"), np.uint8) for k in ("any", "old", "closest", "tie")}
        assert (got["any"] == header_any).all(), (rule, np.flatnonzero(got["any"] != header_any)[:8])
        assert ((got["old"] != header_any) == (on_bound | cut_by_tmax)).all(), rule
        assert (got["closest"] == header_closest).all(), rule
        assert (got["tie"] == np.where(header_closest, 1, 0)).all(), (rule, np.unique(got["tie"]))


def test_every_any_hit_walk_ends_its_leaf_test_at_leaf_upper():
    """the kernels' sources: every leaf test of a walk that has an any-hit or shadow instantiation gets ptl::leaf_upper(<that instantiation>, best_t,
    tmax) as its upper end, and no leaf test of those files gets a bare tmax"""
    import os, re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "single-file-vulkan-pathtracing_amd", "csrc")
    want = {"extend_kernel.h": ("ray_tmax != nullptr", 2), "extend8_kernel.h": ("ray_tmax != nullptr", 1), "extend_inst.h": ("SHADOW", 1),
            "extend_inst16.h": ("SHADOW", 2), "trace_fused.hip": ("ANY", 2), "fused_kernel.h": ("NEE && shadow_walk", 2)}
    for name, (flag, count) in want.items():
        src = open(os.path.join(csrc, name)).read()
        assert src.count(f"ptl::leaf_upper({flag}, best_t, tmax)") == count, name
        tests = re.findall(r"(?:pair_leaf_test(?:<[^>]*>)?|tri_test(?:_perm)?)\((?:[^;]|\n)*?;", src)
        assert len(tests) >= count, name
        for call in tests:
            assert re.search(r"tmin,\s*(?:upper|ptl::leaf_upper\()", call), (name, call[:200])
    assert '#include "hit_rule.h"' in open(os.path.join(csrc, "pair_leaf.h")).read()
