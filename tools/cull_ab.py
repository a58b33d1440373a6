#!/usr/bin/env python3
"""Cost and gain of face culling (SWR_FLAG_CULL_BACK): ms per frame over 200 untimed, pipelined frames, min of --reps, interleaved:
  (a) cfg4 (1 M triangles, 3840x2160) depth-only and colour + depth, no cull against CULL_BACK;
  (b) cfg3 (the torus, z-test, 3840x2160), no cull against CULL_BACK (front = clockwise: the visible side is kept);
  (c) the 8-object draw list of tools/draw_list_ab.py (the eighths of cfg4, each with its own matrix), no cull against CULL_BACK;
  the (triangle, tile) pairs binned of every case (swr_timings.tile_pairs);
  (d) --parent LIB: frames without cull bits of another build of the library (the parent commit's) against this tree, alternating
      in fresh processes (SWR_LIBRARY), so both run on the same box in one call.
Run it under its own time limit: timeout -k 10 900 python3 tools/cull_ab.py [--reps 3] [--parent LIB]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import swr_amd  # noqa: E402
from draw_list_ab import obj  # noqa: E402

S = swr_amd.scenes
N = 200
DT, NC = S.FLAG_DEPTH_TEST, S.FLAG_NO_COLOR
CB = swr_amd.binding.FLAG_CULL_BACK


def ms_per_frame(ctx, draw):
    for _ in range(20):
        draw()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(N):
        draw()
    ctx.sync()
    return (time.perf_counter() - t0) / N * 1e3


def pairs(ctx, draw):
    draw()
    ctx.sync()
    return ctx.timings()["tile_pairs"]


def cases(ctx, sc):
    """(name, draw(flags)) of every row on the scene resident in ctx."""
    n = sc.indices.size
    eighth = n // 8 // 3 * 3
    objs = ctx.draw_items([(k * eighth, eighth if k < 7 else n - 7 * eighth, obj(k)) for k in range(8)])
    return [("(a) cfg4 depth-only", DT | NC, lambda f: ctx.draw(sc.transform, f)),
            ("(a) cfg4 colour+depth", DT, lambda f: ctx.draw(sc.transform, f)),
            ("(c) 8 objects depth-only", DT | NC, lambda f: ctx.draw_list(objs, f)),
            ("(c) 8 objects colour+depth", DT, lambda f: ctx.draw_list(objs, f))]


def parent_side(reps):
    """(d), one side: frames without cull bits; prints one JSON line."""
    out = {}
    sc, s3 = S.cfg4_soup(), S.cfg3_bunny_scale()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(sc.vertices, sc.indices)
        ctx.target_set(sc.width, sc.height)
        for name, base, draw in cases(ctx, sc):
            out[name] = min(ms_per_frame(ctx, lambda: draw(base)) for _ in range(reps))
    with swr_amd.Context() as ctx:
        ctx.scene_upload(s3.vertices, s3.indices)
        ctx.target_set(s3.width, s3.height)
        out["(b) cfg3 z-test"] = min(ms_per_frame(ctx, lambda: ctx.draw(s3.transform, s3.flags)) for _ in range(reps))
    print(json.dumps(out))


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    if "--no-cull-only" in sys.argv:
        return parent_side(reps)
    rows, tp = {}, {}
    sc, s3 = S.cfg4_soup(), S.cfg3_bunny_scale()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(sc.vertices, sc.indices)
        ctx.target_set(sc.width, sc.height)
        for name, base, draw in cases(ctx, sc):
            for _ in range(reps):
                for kind, flags in (("none", base), ("back", base | CB)):
                    rows.setdefault((name, kind), []).append(ms_per_frame(ctx, lambda: draw(flags)))
            for kind, flags in (("none", base), ("back", base | CB)):
                tp[(name, kind)] = pairs(ctx, lambda: draw(flags))
    with swr_amd.Context() as ctx:
        ctx.scene_upload(s3.vertices, s3.indices)
        ctx.target_set(s3.width, s3.height)
        name = "(b) cfg3 z-test"
        for _ in range(reps):
            for kind, flags in (("none", s3.flags), ("back", s3.flags | CB)):
                rows.setdefault((name, kind), []).append(ms_per_frame(ctx, lambda: ctx.draw(s3.transform, flags)))
        for kind, flags in (("none", s3.flags), ("back", s3.flags | CB)):
            tp[(name, kind)] = pairs(ctx, lambda: ctx.draw(s3.transform, flags))
    for (name, kind), v in rows.items():
        print(f"{name:28s} {kind:5s} ms/frame {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})  tile_pairs {tp[(name, kind)]}")
    for name in dict.fromkeys(n for n, _ in rows):
        a, b = min(rows[(name, "none")]), min(rows[(name, "back")])
        print(f"{name:28s} back - none {1e3 * (b - a):+.1f} us per frame ({100 * (b / a - 1):+.1f} %), "
              f"tile_pairs {tp[(name, 'back')]} / {tp[(name, 'none')]} = {tp[(name, 'back')] / max(1, tp[(name, 'none')]):.3f}")
    if "--parent" in sys.argv:
        lib = sys.argv[sys.argv.index("--parent") + 1]
        res = {"parent": [], "tree": []}
        for _ in range(reps):
            for side in ("parent", "tree"):
                env = dict(os.environ)
                env.pop("SWR_LIBRARY", None)
                if side == "parent":
                    env["SWR_LIBRARY"] = lib
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--no-cull-only", "--reps", "1"], env=env,
                                   capture_output=True, text=True, timeout=300, check=True)
                res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
        for name in res["tree"][0]:
            for side in ("parent", "tree"):
                v = [r[name] for r in res[side]]
                print(f"(d) {name:28s} {side:6s} ms/frame {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})")
    print(json.dumps({f"{n}|{k}": min(v) for (n, k), v in rows.items()}))


if __name__ == "__main__":
    main()
