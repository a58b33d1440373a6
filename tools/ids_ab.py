#!/usr/bin/env python3
"""Cost of primitive IDs (SWR_FLAG_PRIMITIVE_IDS): ms per frame over 200 untimed, pipelined frames at 3840x2160.
  (a) cfg4 (1 M triangles) depth-only and colour + depth, without and with the flag, interleaved A/B/A/B;
  (b) --parent LIB: clear frames of this tree against another build of the library (the parent commit's), alternating in fresh
      processes (SWR_LIBRARY), so both run on the same box in one call;
  (c) cfg4 cut into 8 objects with their own matrices, one draw list, without and with the flag.
Run it under its own time limit: timeout -k 10 600 python3 tools/ids_ab.py [--reps 3] [--parent LIB]"""
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
DT, NC = S.FLAG_DEPTH_TEST, S.FLAG_NO_COLOR
IDS = 32


def ms_per_frame(draw):
    for _ in range(20):
        draw()
    draw.ctx.sync()
    t0 = time.perf_counter()
    for _ in range(N):
        draw()
    draw.ctx.sync()
    return (time.perf_counter() - t0) / N * 1e3


class Draw:
    def __init__(self, ctx, fn):
        self.ctx, self.fn = ctx, fn

    def __call__(self):
        self.fn()


def clear_only(reps):
    """(b), one side: cfg4 clear frames without the flag; prints one JSON line."""
    sc = S.cfg4_soup()
    out = {}
    with swr_amd.Context() as ctx:
        ctx.scene_upload(sc.vertices, sc.indices)
        ctx.target_set(sc.width, sc.height)
        for name, flags in (("depth-only", DT | NC), ("colour+depth", DT)):
            out[name] = min(ms_per_frame(Draw(ctx, lambda: ctx.draw(sc.transform, flags))) for _ in range(reps))
    print(json.dumps(out))


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    if "--clear-only" in sys.argv:
        return clear_only(reps)
    sc = S.cfg4_soup()
    rows = {}
    with swr_amd.Context() as ctx:
        ctx.scene_upload(sc.vertices, sc.indices)
        ctx.target_set(sc.width, sc.height)
        for name, base in (("cfg4 depth-only", DT | NC), ("cfg4 colour+depth", DT)):
            for _ in range(reps):
                for kind, flags in (("plain", base), ("ids", base | IDS)):
                    rows.setdefault(("(a) " + name, kind), []).append(ms_per_frame(Draw(ctx, lambda: ctx.draw(sc.transform, flags))))
        n = sc.indices.size // 8 // 3 * 3
        items = [(k * n, n, S.app_transform(0.1 * k, scale=1.0)) for k in range(8)]
        for name, base in (("8 objects depth-only", DT | NC), ("8 objects colour+depth", DT)):
            for _ in range(reps):
                for kind, flags in (("plain", base), ("ids", base | IDS)):
                    rows.setdefault(("(c) " + name, kind), []).append(ms_per_frame(Draw(ctx, lambda: ctx.draw_list(items, flags))))
    for (name, kind), v in rows.items():
        print(f"{name:28s} {kind:5s} ms/frame {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})")
    for name in sorted({n for n, _ in rows}):
        a, b = min(rows[(name, "plain")]), min(rows[(name, "ids")])
        print(f"{name:28s} ids - plain {1e3 * (b - a):+.1f} us per frame ({100 * (b / a - 1):+.1f} %)")
    if "--parent" in sys.argv:
        lib = sys.argv[sys.argv.index("--parent") + 1]
        res = {"parent": [], "tree": []}
        for _ in range(reps):
            for side, env in (("parent", dict(os.environ, SWR_LIBRARY=lib)), ("tree", dict(os.environ))):
                env.pop("SWR_LIBRARY", None) if side == "tree" else None
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--clear-only", "--reps", "1"], env=env,
                                   capture_output=True, text=True, timeout=300, check=True)
                res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
        for name in ("depth-only", "colour+depth"):
            for side in ("parent", "tree"):
                v = [r[name] for r in res[side]]
                print(f"(b) cfg4 {name:13s} {side:6s} ms/frame {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})")
    print(json.dumps({f"{n}|{k}": min(v) for (n, k), v in rows.items()}))


if __name__ == "__main__":
    main()
