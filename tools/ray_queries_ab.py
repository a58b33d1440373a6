#!/usr/bin/env python3
"""Ray queries (swr_query_rays): that swr_cast_rays costs what it cost in the parent commit, and what an occlusion ray
costs against a nearest-hit ray.  Scene and ray sets are those of tools/rays_ab.py (the posed torus of 1 000 000 triangles; 1 ray,
1 024 random rays, 65 536 camera rays), plus
  65 536 shadow rays   from the camera rays' hit points (a miss starts at the ray's origin) towards one light direction, tmin just off
                       the surface.
  --sides PARENT_LIB [--tree-first]: fresh processes alternating parent, tree, parent, tree (SWR_LIBRARY selects the parent's build;
    --tree-first: tree, parent, tree, parent, so that a drift over the call falls on the other side): per side the
    median whole-call ms of swr_cast_rays on the three sets, and on this tree's sides also of swr_query_rays in nearest mode (back faces
    culled) and in any-hit mode on the random, camera and shadow rays, with the occluded share of each set.  The two parent sides give
    the spread of the parent against itself.
  --kernel cast|nearest|any: 20 calls of each ray set in that mode and nothing else, for a profiler run of its own
    (rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/ray_queries_ab.py --kernel any; SWR_LIBRARY selects the build).
  --parse NAME=DIR [NAME=DIR ...]: the kernel times of such runs, per kernel and ray set (the dispatches of a run come in the order
    of its calls, 20 per set).
Run each under its own time limit; --out FILE keeps what was printed."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays_ab as RA  # noqa: E402  (puts the repository and tests/ on sys.path)

B = RA.B
LIGHT = np.array([0.3, 0.2, 1.0], dtype=np.float32)
CALLS = 20
MODES = {"cast": None, "nearest": dict(cull="back"), "any": dict(any_hit=True)}


def shadow_rays(ctx, cam):
    hits = ctx.cast_rays(cam)
    hit = hits["primitive"] != B.ID_NONE
    rays = np.zeros(cam.size, dtype=B.RAY_DTYPE)
    rays["origin"] = cam["origin"] + np.where(hit, hits["t"], 0.0)[:, None].astype(np.float32) * cam["dir"]
    rays["dir"] = LIGHT
    rays["tmin"], rays["tmax"] = 1e-3, 4.0
    return rays


def all_sets(ctx):
    sets = RA.ray_sets()
    return sets + [("65 536 shadow rays", shadow_rays(ctx, sets[2][1]))]


def run(ctx, rays, mode):
    return ctx.cast_rays(rays) if MODES[mode] is None else ctx.query_rays(rays, **MODES[mode])


def kernel_loop(mode):
    v, idx = RA.torus()
    with RA.swr_amd.Context() as ctx:
        RA.resident(ctx, v, idx)
        sets = all_sets(ctx)
        ctx.sync()
        for _, rays in sets:
            for _ in range(CALLS):
                run(ctx, rays, mode)


def one_side():
    """One side of --sides: prints one JSON line."""
    v, idx = RA.torus()
    out = {}
    with RA.swr_amd.Context() as ctx:
        RA.resident(ctx, v, idx)
        sets = all_sets(ctx)
        for name, rays in sets:
            out["cast " + name] = RA.median_ms(lambda: ctx.cast_rays(rays))[0]
        if hasattr(ctx._L, "swr_query_rays"):
            for name, rays in sets[1:]:
                near = ctx.query_rays(rays)
                occ = ctx.query_rays(rays, any_hit=True)
                assert ((occ["primitive"] != B.ID_NONE) == (near["primitive"] != B.ID_NONE)).all() and not occ["t"].any(), name
                assert near.tobytes() == ctx.cast_rays(rays).tobytes(), name
                out["share " + name] = float((occ["primitive"] == B.RAY_OCCLUDED).mean())
                for mode in ("nearest", "any"):
                    out[mode + " " + name] = RA.median_ms(lambda: run(ctx, rays, mode))[0]
    print(json.dumps(out))


def sides(parent, say, tree_first=False):
    order = [("parent", parent), ("tree", None), ("parent", parent), ("tree", None)]
    if tree_first:      # (the other order: a drift over the call then falls on the other side)
        order = order[1:] + order[:1]
    res = []
    for side, lib in order:
        env = dict(os.environ)
        env.pop("SWR_LIBRARY", None)
        if lib:
            env["SWR_LIBRARY"] = os.path.abspath(lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-side"], env=env, capture_output=True, text=True, timeout=280,
                           check=True)
        res.append((side, json.loads(p.stdout.strip().splitlines()[-1])))
        print(f"# {side}: done", file=sys.stderr, flush=True)
    say(f"fresh processes alternating {', '.join(s for s, _ in order)}; median whole-call ms of {RA.REPS} calls after {RA.WARM}")
    keys = []
    for _, r in res:
        keys += [k for k in r if k not in keys]
    for k in keys:
        say(f"  {k:32s} " + "   ".join(f"{side} {r[k]:9.4f}" if k in r else f"{side} {'-':>9s}" for side, r in res))


def parse(runs, say):
    for spec in runs:
        name, d = spec.split("=", 1)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        assert len(files) == 1, (d, files)
        rows = [r for r in csv.DictReader(open(files[0])) if "k_rays" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        labels = ["1 ray", "1 024 random rays", "65 536 camera rays", "65 536 shadow rays"]
        for kind in ("k_rays_init", "k_rays_any<", "k_rays<", "k_rays_finish"):
            mine = [r for r in rows if kind in r["Kernel_Name"]]
            # (every run casts the camera rays once, up front, to make the shadow rays: that call is left out)
            extra = len(mine) - CALLS * len(labels)
            if extra < 0:
                continue
            assert extra in (0, 1), (name, kind, len(mine))
            mine = mine[extra:]
            for k, label in enumerate(labels):
                us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine[CALLS * k:CALLS * (k + 1)]]
                say(f"{name:16s} {kind.rstrip('<'):14s} {label:20s} calls {len(us)}  median {statistics.median(us):10.2f} us  min {min(us):10.2f}  max {max(us):10.2f}")


def main():
    a = sys.argv[1:]
    if "--one-side" in a:
        return one_side()
    if "--kernel" in a:
        return kernel_loop(a[a.index("--kernel") + 1])
    out = a[a.index("--out") + 1] if "--out" in a else None
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    if "--sides" in a:
        sides(a[a.index("--sides") + 1], say, "--tree-first" in a)
    if "--parse" in a:
        parse([x for x in a[a.index("--parse") + 1:] if "=" in x], say)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
