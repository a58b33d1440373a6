#!/usr/bin/env python3
"""Cost of depth clipping (SWR_FLAG_DEPTH_CLIP): ms per frame over 200 untimed, pipelined frames, min of --reps,
the two sides interleaved:
  (a) cfg4 (1 M triangles, 3840x2160, entirely in front) depth-only and colour + depth, without against with the flag;
  (b) cfg5 textured (Sponza-scale grid, entirely in front), without against with the flag;
  (c) a fly-through: cfg4's soup seen by a Metal [0, 1] perspective from inside it (a few per cent of the triangles cross the
      near plane), without against with the flag, and the (triangle, tile) pairs binned of both;
  (d) --parent LIB: frames without the flag of another build of the library (the parent commit's) against this tree, alternating
      in fresh processes (SWR_LIBRARY), so both run on the same box in one call.
Run it under its own time limit: timeout -k 10 900 python3 tools/clip_ab.py [--reps 3] [--parent LIB]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import swr_amd  # noqa: E402

S = swr_amd.scenes
N = 200
DT, NC = S.FLAG_DEPTH_TEST, S.FLAG_NO_COLOR
CLIP = swr_amd.binding.FLAG_DEPTH_CLIP


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


def fly_through(sc):
    """cfg4's triangles spread through a 16 x 9 x 24 box around an eye near its centre, looking down +z (near 0.25, far 24): each
    triangle at the depth of its first vertex (+- 0.1), so the ones near the eye plane cross the near plane."""
    v = np.array(sc.vertices, copy=True).reshape(-1, 3, 8)
    v[..., 0] *= 8.0
    v[..., 1] *= 4.5
    z0 = v[:, 0:1, 2] * 24.0 - 4.0
    v[..., 2] = z0 + (v[..., 2] - v[:, 0:1, 2]) * 0.2
    v = v.reshape(-1, 8)
    near, far, fy = 0.25, 24.0, 1.0
    a = far / (far - near)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1], m[2, 2], m[2, 3], m[3, 2] = fy * sc.height / sc.width, fy, a, -near * a, 1.0
    return v, np.ascontiguousarray(m.astype(np.float32).T).reshape(16)


def scenes():
    sc, s5 = S.cfg4_soup(), S.cfg5_textured()
    fv, fm = fly_through(sc)
    return [("(a) cfg4 depth-only", sc.vertices, sc.indices, sc.transform, sc.width, sc.height, DT | NC, None),
            ("(a) cfg4 colour+depth", sc.vertices, sc.indices, sc.transform, sc.width, sc.height, DT, None),
            ("(b) cfg5 textured", s5.vertices, s5.indices, s5.transform, s5.width, s5.height, s5.flags, s5.shading),
            ("(c) fly-through depth-only", fv, sc.indices, fm, sc.width, sc.height, DT | NC, None),
            ("(c) fly-through colour+depth", fv, sc.indices, fm, sc.width, sc.height, DT, None)]


def run(reps, sides):
    rows, tp = {}, {}
    for name, v, i, m, w, h, flags, sh in scenes():
        with swr_amd.Context() as ctx:
            ctx.scene_upload(v, i)
            if sh is not None:
                ctx.shading_set(sh)
            ctx.target_set(w, h)
            for _ in range(reps):
                for kind, f in sides(flags):
                    rows.setdefault((name, kind), []).append(ms_per_frame(ctx, lambda: ctx.draw(m, f)))
            for kind, f in sides(flags):
                tp[(name, kind)] = pairs(ctx, lambda: ctx.draw(m, f))
    return rows, tp


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    if "--no-clip-only" in sys.argv:
        rows, _ = run(reps, lambda f: [("none", f)])
        print(json.dumps({n: min(v) for (n, _), v in rows.items()}))
        return
    rows, tp = run(reps, lambda f: [("none", f), ("clip", f | CLIP)])
    for (name, kind), v in rows.items():
        print(f"{name:30s} {kind:5s} ms/frame {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})  tile_pairs {tp[(name, kind)]}")
    for name in dict.fromkeys(n for n, _ in rows):
        a, b = min(rows[(name, "none")]), min(rows[(name, "clip")])
        print(f"{name:30s} clip - none {1e3 * (b - a):+.1f} us per frame ({100 * (b / a - 1):+.1f} %), "
              f"tile_pairs {tp[(name, 'clip')]} / {tp[(name, 'none')]}")
    if "--parent" in sys.argv:
        lib = sys.argv[sys.argv.index("--parent") + 1]
        res = {"parent": [], "tree": []}
        for _ in range(reps):
            for side in ("parent", "tree"):
                env = dict(os.environ)
                env.pop("SWR_LIBRARY", None)
                if side == "parent":
                    env["SWR_LIBRARY"] = lib
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--no-clip-only", "--reps", "1"], env=env,
                                   capture_output=True, text=True, timeout=600, check=True)
                res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
        for name in res["tree"][0]:
            for side in ("parent", "tree"):
                v = [r[name] for r in res[side]]
                print(f"(d) {name:30s} {side:6s} ms/frame {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})")


if __name__ == "__main__":
    main()
