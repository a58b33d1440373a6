#!/usr/bin/env python3
"""Cost of the load action: ms per frame over 200 untimed, pipelined frames of cfg4 (1 M triangles, 3840x2160), depth-only and
colour + depth, clear frames against load frames (SWR_FLAG_LOAD: every frame starts from the last one's image), interleaved
A/B/A/B.  Run it under its own time limit: timeout -k 10 300 python3 tools/load_ab.py [--reps 3]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import swr_amd  # noqa: E402

S = swr_amd.scenes
N = 200


def ms_per_frame(ctx, transform, flags):
    for _ in range(20):
        ctx.draw(transform, flags)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(N):
        ctx.draw(transform, flags)
    ctx.sync()
    return (time.perf_counter() - t0) / N * 1e3


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    sc = S.cfg4_soup()
    rows = {}
    with swr_amd.Context() as ctx:
        ctx.scene_upload(sc.vertices, sc.indices)
        ctx.target_set(sc.width, sc.height)
        for name, base in (("cfg4 depth-only", S.FLAG_DEPTH_TEST | S.FLAG_NO_COLOR), ("cfg4 colour+depth", S.FLAG_DEPTH_TEST)):
            for _ in range(reps):
                for kind, flags in (("clear", base), ("load", base | swr_amd.binding.FLAG_LOAD)):
                    rows.setdefault((name, kind), []).append(ms_per_frame(ctx, sc.transform, flags))
    for (name, kind), v in rows.items():
        print(f"{name:18s} {kind:5s} ms/frame {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})")
    for name in ("cfg4 depth-only", "cfg4 colour+depth"):
        c, l = min(rows[(name, "clear")]), min(rows[(name, "load")])
        print(f"{name:18s} load - clear {1e3 * (l - c):+.1f} us per frame ({100 * (l / c - 1):+.1f} %)")
    print(json.dumps({f"{n}|{k}": min(v) for (n, k), v in rows.items()}))


if __name__ == "__main__":
    main()
