"""What the planning step of a render call decides, pinned against the commit before the call plan was introduced.

tests/golden/render_plan_table.json was recorded by this file's generator (`python tests/test_render_plan_table.py --record`) on that
commit: for a fixed list of cases the (pipeline, frames_in_flight, sample_groups, tail_samples, workspace_bytes) pt_render_prepare leaves in
pt_stats, and for a short list of doubly-bad inputs the status and pt_last_error text that win.  The test replays both lists and compares
for equality.  The shape rules go by walked slots per lane of the fused grid (num_cus * 6 * 256 lanes), so the table holds for the
recorded compute-unit count only; elsewhere the test skips.  pt_render_prepare launches nothing: the whole table takes a few seconds."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_plan_table.json")
FIELDS = ("pipeline", "frames_in_flight", "sample_groups", "tail_samples", "workspace_bytes")
W = 1024  # 128 tiles across: with cull = 0 a film of height 8 b has x32 = floor(frames * 128 b / 192) on 256 compute units


def _tail_rule_cases():
    """Cornell box, spp 32, heights that put x32 (render.hip fused_slots_x32) on both sides of 36, 81, 144, 252 and 324 on a 256-CU device:
    x32 = 35|36, 81|82, 144|145, 252|253, 324|325 at one frame; 34|36, 81|82, 144|145, 252|253, 324|325 at two; 34|37 and 322|325 at four."""
    heights = {1: (424, 432, 976, 984, 1736, 1744, 3032, 3040, 3896, 3904),
               2: (208, 216, 488, 496, 864, 872, 1512, 1520, 1944, 1952),
               4: (104, 112, 968, 976)}
    return {f"tail_{k}x{h}": ("cornell", W, h, dict(frame_count=k, spp_per_frame=32), {}) for k, hs in heights.items() for h in hs}


def plan_cases(pt):
    """name -> (scene, width, height, pt_params fields over the library's defaults, pt_tuning fields over cull = 0)"""
    c = _tail_rule_cases()
    c["spp1_no_tail"] = ("cornell", W, 976, dict(frame_count=1, spp_per_frame=1), {})
    c["explicit_groups"] = ("cornell", W, 976, dict(frame_count=1, spp_per_frame=32, sample_groups=4), {})
    c["explicit_in_flight"] = ("cornell", W, 488, dict(frame_count=6, spp_per_frame=32, frames_in_flight=2), {})
    c["fused_tail_0"] = ("cornell", W, 976, dict(frame_count=1, spp_per_frame=32), dict(fused_tail=0))
    c["fused_tail_5"] = ("cornell", W, 976, dict(frame_count=1, spp_per_frame=32), dict(fused_tail=5))
    c["world4_rank1"] = ("cornell", W, 1736, dict(frame_count=1, spp_per_frame=32, rank=1, world=4), {})
    for k in (1, 2, 4):  # x32 = 48, 96, 192: all groups, groups of eight, one group
        c[f"grid_{k}_frames"] = ("grid", W, 576, dict(frame_count=k, spp_per_frame=32), {})
    c["fused_nee"] = ("cornell", W, 976, dict(frame_count=1, spp_per_frame=32, pipeline=pt.PIPELINE_FUSED, flags=pt.FLAG_NEE), {})
    c["wavefront_small"] = ("cornell", 200, 120, dict(frame_count=3, spp_per_frame=8, pipeline=pt.PIPELINE_WAVEFRONT), {})
    c["wavefront_1080p"] = ("cornell", 1920, 1080, dict(frame_count=16, spp_per_frame=32, pipeline=pt.PIPELINE_WAVEFRONT), {})
    for mb in (256, 3, 1):  # the shrink loop: fewer groups; one group, then fewer frames in flight; nothing fits
        c[f"shrink_{mb}"] = ("cornell", 256, 256, dict(frame_count=4, spp_per_frame=32), dict(mem_budget_mb=mb))
    return c


def refusal_cases(pt):
    """name -> (entry, film planes, pt_params fields, fields of the entry's own parameter struct): two things wrong at once"""
    size_pipe = dict(width=72, pipeline=7)
    async_fused = dict(flags=pt.FLAG_ASYNC, pipeline=pt.PIPELINE_FUSED)
    nee_groups = dict(flags=pt.FLAG_NEE, sample_groups=2, pipeline=pt.PIPELINE_AUTO)
    c = {}
    for entry in ("render", "prepare", "adaptive", "guided"):
        c[f"{entry}_size_and_pipeline"] = (entry, "all", size_pipe, {})
        c[f"{entry}_async_and_fused"] = (entry, "all", async_fused, {})
        c[f"{entry}_nee_and_two_groups"] = (entry, "all", nee_groups, {})
    c["adaptive_no_moments_and_threshold"] = ("adaptive", "none", {}, dict(threshold=-1.0))
    c["adaptive_threshold_and_size"] = ("adaptive", "all", dict(width=72), dict(threshold=-1.0))
    c["guided_no_guides_and_mode"] = ("guided", "none", {}, dict(mode=3))
    c["guided_mode_and_size"] = ("guided", "all", dict(width=72), dict(mode=3))
    return c


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def grid_scene(pt, ctx):
    sc = pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL))
    sc.set_instances(pt.cornell_grid_instances())
    return sc


def plan_of(pt, ctx, scene, case):
    """the FIELDS of pt_stats after pt_render_prepare on a fresh film"""
    _, w, h, fields, tune = case
    old = ctx.set_tuning(cull=0, **tune)
    film = pt.Film(ctx, w, h)
    try:
        ctx.reset_stats()
        try:
            pt.render_prepare(scene, film, pt.library_default_params(frame=0, width=w, height=h, max_depth=8, **fields))
        except pt.PtError as e:  # (a refused plan is a row too)
            return [int(e.status), pt.lib_amd().pt_last_error(ctx.h).decode()]
        st = ctx.stats()
        return [int(getattr(st, n)) for n in FIELDS]
    finally:
        film.close()
        ctx.set_tuning(**old)


def refusal_of(pt, ctx, scene, case):
    """[status, pt_last_error] of the call"""
    entry, planes, fields, own = case
    w, h = 64, 48
    film = pt.Film(ctx, w, h)
    try:
        if planes == "all":
            film.enable_aov(); film.enable_moments(); film.enable_counts()
        p = pt.library_default_params(**dict(dict(frame=0, frame_count=2, width=w, height=h, spp_per_frame=4, max_depth=4), **fields))
        try:
            if entry == "render":
                pt.render(scene, film, p)
            elif entry == "prepare":
                pt.render_prepare(scene, film, p)
            elif entry == "adaptive":
                pt.render_adaptive(scene, film, p, **own)
            else:
                gp = pt.guided_default_params()
                for k, v in own.items():
                    setattr(gp, k, v)
                pt.render_guided(scene, film, p, guided_params=gp)
        except pt.PtError as e:
            return [int(e.status), pt.lib_amd().pt_last_error(ctx.h).decode()]
        return [0, ""]
    finally:
        film.close()


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def table(pt):
    g = _golden()
    if num_cus() != g["num_cus"]:
        pytest.skip(f"the table was recorded on a device with {g['num_cus']} compute units, this one has {num_cus()}")
    return g


@pytest.fixture(scope="module")
def plan_ctx(pt):
    """a context of this module's own, as the generator's: what other tests left in the session's context (tuning, grown scratch) plays no part"""
    ctx = pt.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def scenes(pt, plan_ctx, cornell_arrays):
    sc = {"cornell": pt.Scene(plan_ctx, *cornell_arrays), "grid": grid_scene(pt, plan_ctx)}
    yield sc
    for s in sc.values():
        s.close()


def _report(wrong):
    """the whole difference as (got, recorded) per case, and the device's free memory: the shape rules plan within min(free, budget)"""
    import torch
    free, total = torch.cuda.mem_get_info()
    return json.dumps({"free_bytes": free, "total_bytes": total, "wrong": wrong}, indent=1)


@pytest.mark.gpu
def test_render_plan_table(pt, plan_ctx, scenes, table):
    """every case of plan_cases: pt_render_prepare decides what it decided when the table was recorded"""
    cases = plan_cases(pt)
    assert sorted(cases) == sorted(table["plans"])
    got = {name: plan_of(pt, plan_ctx, scenes[case[0]], case) for name, case in cases.items()}
    wrong = {name: (got[name], table["plans"][name]) for name in cases if got[name] != table["plans"][name]}
    assert not wrong, _report(wrong)


@pytest.mark.gpu
def test_render_refusal_table(pt, plan_ctx, scenes, table):
    """every case of refusal_cases: of two things wrong at once, the same status and the same message win"""
    cases = refusal_cases(pt)
    assert sorted(cases) == sorted(table["refusals"])
    got = {name: refusal_of(pt, plan_ctx, scenes["cornell"], case) for name, case in cases.items()}
    wrong = {name: (got[name], table["refusals"][name]) for name in cases if got[name] != table["refusals"][name]}
    assert not wrong, _report(wrong)


def record():
    """The generator: writes the table from the library as it is built in this tree."""
    import importlib
    cus = num_cus()  # (torch first: it has to bring up its own runtime before the library loads one)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [repo, os.path.join(repo, "tests")]
    from conftest import _WavefrontByDefault
    pt = _WavefrontByDefault(importlib.import_module("single-file-vulkan-pathtracing_amd"))
    ctx = pt.Context(0)
    scenes = {"cornell": pt.Scene(ctx, *pt.load_obj(pt.ASSET_CORNELL)), "grid": grid_scene(pt, ctx)}
    out = {"num_cus": cus, "fields": list(FIELDS), "plans": {}, "refusals": {}}
    for name, case in plan_cases(pt).items():
        out["plans"][name] = plan_of(pt, ctx, scenes[case[0]], case)
        print(name, out["plans"][name], flush=True)
    for name, case in refusal_cases(pt).items():
        out["refusals"][name] = refusal_of(pt, ctx, scenes["cornell"], case)
        print(name, out["refusals"][name], flush=True)
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for s in scenes.values():
        s.close()
    ctx.close()


if __name__ == "__main__" and sys.argv[1:2] == ["--record"]:
    record()
