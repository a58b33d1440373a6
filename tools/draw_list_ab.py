#!/usr/bin/env python3
"""Cost of draw lists (swr_draw_list), ms per image over 200 untimed, pipelined frames, interleaved A/B/A/B on one box:
  (a) cfg4 (1 M triangles, 3840x2160) as 8 items of 125 K with cfg4's transform against one swr_draw: the same image, so the list's
      own overhead; depth-only and colour + depth;
  (b) 8 objects (the eighths of cfg4, each with its own matrix, obj()) as one list against the chain of 8 one-item frames (first clear,
      the rest SWR_FLAG_LOAD);
  (c) instancing: a 125 K mesh 8 times, one list against 8 load frames of swr_draw;
  (d) the one-time stream rebuild of a list with new boundaries: its first frame against the same list once the stream is cut.
Run it under its own time limit: timeout -k 10 600 python3 tools/draw_list_ab.py [--reps 3] [--out profiles/draw_list/ab.txt]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import swr_amd  # noqa: E402

S = swr_amd.scenes
LOAD = swr_amd.binding.FLAG_LOAD
N = 200


def obj(k):
    """Object k's matrix: moved by a few per cent of the screen, every other one with a mild perspective (w = 1 + z / 16), so the
    triangles keep cfg4's sizes."""
    tx, ty = 0.04 * (k % 4) - 0.06, 0.05 * (k // 4) - 0.025
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.0625 * (k % 2), tx, ty, 0, 1], dtype=np.float32)


def ms_per_image(ctx, frame):
    for _ in range(10):
        frame()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(N):
        frame()
    ctx.sync()
    return (time.perf_counter() - t0) / N * 1e3


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    sc = S.cfg4_soup()
    n = sc.indices.size
    eighth = n // 8 // 3 * 3
    rows, lines = {}, []
    with swr_amd.Context() as ctx:
        ctx.scene_upload(sc.vertices, sc.indices)
        ctx.target_set(sc.width, sc.height)
        # (d) first: the stream is still one segment
        cuts8 = ctx.draw_items([(k * eighth, eighth if k < 7 else n - 7 * eighth, sc.transform) for k in range(8)])
        ctx.draw(sc.transform, S.FLAG_DEPTH_TEST | S.FLAG_NO_COLOR)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.draw_list(cuts8, S.FLAG_DEPTH_TEST | S.FLAG_NO_COLOR)
        ctx.sync()
        first = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ctx.draw_list(cuts8, S.FLAG_DEPTH_TEST | S.FLAG_NO_COLOR)
        ctx.sync()
        again = (time.perf_counter() - t0) * 1e3
        lines.append(f"(d) first frame of a list with new boundaries {first:.2f} ms, the same list again {again:.2f} ms: "
                     f"rebuild ~{first - again:.2f} ms")
        objs = ctx.draw_items([(k * eighth, eighth if k < 7 else n - 7 * eighth, obj(k))
                               for k in range(8)])
        for name, base in (("depth-only", S.FLAG_DEPTH_TEST | S.FLAG_NO_COLOR), ("colour+depth", S.FLAG_DEPTH_TEST)):
            # the images of (a) are the same: checked once
            ctx.draw(sc.transform, base)
            ctx.sync()
            d0 = ctx.read_depth().copy()
            ctx.draw_list(cuts8, base)
            ctx.sync()
            assert ctx.read_depth().tobytes() == d0.tobytes(), "(a) the list's image differs from swr_draw's"

            def chain(base=base):
                for k in range(8):
                    ctx.draw_list(objs[k:k + 1], base | (LOAD if k else 0))
            cases = [(f"(a) {name} swr_draw", lambda base=base: ctx.draw(sc.transform, base)),
                     (f"(a) {name} list of 8", lambda base=base: ctx.draw_list(cuts8, base)),
                     (f"(b) {name} 8 objects, list", lambda base=base: ctx.draw_list(objs, base)),
                     (f"(b) {name} 8 objects, load chain", chain)]
            for _ in range(reps):
                for label, fr in cases:
                    rows.setdefault(label, []).append(ms_per_image(ctx, fr))
    small_n = (125_000 * 3)
    with swr_amd.Context() as ctx:
        ctx.scene_upload(sc.vertices, sc.indices[:small_n])
        ctx.target_set(sc.width, sc.height)
        ms = [obj(k) for k in range(8)]
        inst = ctx.draw_items([(0, small_n, m) for m in ms])
        for name, base in (("depth-only", S.FLAG_DEPTH_TEST | S.FLAG_NO_COLOR), ("colour+depth", S.FLAG_DEPTH_TEST)):
            def loads(base=base):
                for k, m in enumerate(ms):
                    ctx.draw(m, base | (LOAD if k else 0))
            cases = [(f"(c) {name} 125 K x 8, list", lambda base=base: ctx.draw_list(inst, base)),
                     (f"(c) {name} 125 K x 8, load frames", loads)]
            for _ in range(reps):
                for label, fr in cases:
                    rows.setdefault(label, []).append(ms_per_image(ctx, fr))
    for label, v in rows.items():
        lines.append(f"{label:42s} ms/image {' '.join('%.4f' % x for x in v)}  (min {min(v):.4f})")
    for a, b in (("(a) depth-only list of 8", "(a) depth-only swr_draw"), ("(a) colour+depth list of 8", "(a) colour+depth swr_draw"),
                 ("(b) depth-only 8 objects, list", "(b) depth-only 8 objects, load chain"),
                 ("(b) colour+depth 8 objects, list", "(b) colour+depth 8 objects, load chain"),
                 ("(c) depth-only 125 K x 8, list", "(c) depth-only 125 K x 8, load frames"),
                 ("(c) colour+depth 125 K x 8, list", "(c) colour+depth 125 K x 8, load frames")):
        x, y = min(rows[a]), min(rows[b])
        lines.append(f"{a} vs {b.split(' ', 2)[2]}: {1e3 * (x - y):+.1f} us per image ({100 * (x / y - 1):+.1f} %)")
    lines.append(json.dumps({k: min(v) for k, v in rows.items()}))
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
