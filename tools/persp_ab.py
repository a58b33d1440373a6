#!/usr/bin/env python3
"""Cost of perspective-correct interpolation (SWR_FLAG_PERSPECTIVE): ms per frame over 200 untimed, pipelined frames,
min of --reps, the two sides interleaved:
  (a) cfg3 Phong at 4K (already a perspective camera), without against with the flag;
  (b) cfg5 textured under scenes.app_transform (its own transform is the identity, where the flag costs nothing), without / with;
  (c) cfg4 colour + depth under scenes.app_transform, without against with the flag;
  (d) --parent LIB: frames without the flag of another build of the library (the parent commit's) against this tree, alternating
      in fresh processes (SWR_LIBRARY), so both run on the same box in one call.
Run it under its own time limit: timeout -k 10 900 python3 tools/persp_ab.py [--reps 3] [--parent LIB]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import swr_amd  # noqa: E402

S = swr_amd.scenes
N = 200
DT = S.FLAG_DEPTH_TEST
PERSP = swr_amd.binding.FLAG_PERSPECTIVE


def ms_per_frame(ctx, draw):
    for _ in range(20):
        draw()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(N):
        draw()
    ctx.sync()
    return (time.perf_counter() - t0) / N * 1e3


def scenes():
    s3, s5, s4 = S.cfg3_phong(), S.cfg5_textured(), S.cfg4_soup()
    app = S.app_transform(0.3, scale=1.0)
    return [("(a) cfg3 Phong 4K", s3.vertices, s3.indices, s3.transform, s3.width, s3.height, s3.flags, s3.shading),
            ("(b) cfg5 textured app_transform", s5.vertices, s5.indices, app, s5.width, s5.height, s5.flags, s5.shading),
            ("(c) cfg4 colour+depth app_transform", s4.vertices, s4.indices, app, s4.width, s4.height, DT, None)]


def run(reps, sides):
    rows = {}
    for name, v, i, m, w, h, flags, sh in scenes():
        with swr_amd.Context() as ctx:
            ctx.scene_upload(v, i)
            if sh is not None:
                ctx.shading_set(sh)
            ctx.target_set(w, h)
            for _ in range(reps):
                for kind, f in sides(flags):
                    rows.setdefault((name, kind), []).append(ms_per_frame(ctx, lambda: ctx.draw(m, f)))
    return rows


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    if "--no-flag-only" in sys.argv:
        rows = run(reps, lambda f: [("none", f)])
        print(json.dumps({n: min(v) for (n, _), v in rows.items()}))
        return
    rows = run(reps, lambda f: [("none", f), ("persp", f | PERSP)])
    for (name, kind), v in rows.items():
        print(f"{name:36s} {kind:5s} ms/frame {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})")
    for name in dict.fromkeys(n for n, _ in rows):
        a, b = min(rows[(name, "none")]), min(rows[(name, "persp")])
        print(f"{name:36s} persp - none {1e3 * (b - a):+.1f} us per frame ({100 * (b / a - 1):+.1f} %)")
    if "--parent" in sys.argv:
        lib = sys.argv[sys.argv.index("--parent") + 1]
        res = {"parent": [], "tree": []}
        for _ in range(reps):
            for side in ("parent", "tree"):
                env = dict(os.environ)
                env.pop("SWR_LIBRARY", None)
                if side == "parent":
                    env["SWR_LIBRARY"] = lib
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--no-flag-only", "--reps", "1"], env=env,
                                   capture_output=True, text=True, timeout=600, check=True)
                res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
        for name in res["tree"][0]:
            for side in ("parent", "tree"):
                v = [r[name] for r in res[side]]
                print(f"(d) {name:36s} {side:6s} ms/frame {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})")


if __name__ == "__main__":
    main()
