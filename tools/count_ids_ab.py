#!/usr/bin/env python3
"""Visibility counts (swr_count_ids) against what a user did before: read_ids into page-locked memory plus np.bincount
on the host (per item: plus the mapping of binding.list_ids_to_items).  cfg4 (1 M triangles, 3840x2160) drawn z-tested with IDs,
as one draw and as the 8-object draw list of tools/draw_list_ab.py; per call the median of REPS calls after WARM warm-up calls, the
frame drawn once and complete (the calls measure the query, not the frame).
  (a) per primitive, whole target: host route, swr_count_ids; plus a 256 x 256 rectangle and one pixel (picking);
  (b) per item, 8 objects: host route, swr_count_ids;
  (c) one screen-filling triangle at the same size: every 64-pixel segment belongs to ONE counter — the worst case of the integer
      atomics, which the carry of one-ID segments takes out — next to cfg4, where the adds spread over a million counters; the groups
      per call are counted on the host from the ID image for both wave-level reductions (runs per 64-pixel row segment, distinct IDs
      per segment; a group is one add, except that consecutive one-ID segments of a wave share one);
  (d) --variant LIB [--variant LIB ...]: the same swr_count_ids calls against other builds of the library, each in a fresh process
      (SWR_LIBRARY), alternating with this one.  The product reduces a mixed segment with the leader loop per primitive and with run
      heads per item; the other combinations are  make ab NAME=count_runs ABFLAGS=-DSWR_TUNE_COUNT_REDUCE=0  (run heads for both) and
      make ab NAME=count_leader ABFLAGS=-DSWR_TUNE_COUNT_REDUCE=1  (leader loop for both).
Every result of swr_count_ids is compared with the host route's before it is timed.
Run it under its own time limit: timeout -k 10 600 python3 tools/count_ids_ab.py [--variant LIB ...] [--out profiles/count_ids/count_ids_ab.txt]"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import swr_amd  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
from draw_list_ab import obj  # noqa: E402

S, B = swr_amd.scenes, swr_amd.binding
DT, IDS = S.FLAG_DEPTH_TEST, B.FLAG_PRIMITIVE_IDS
WARM, REPS = 5, 30
NONE = B.ID_NONE


def median_ms(call):
    for _ in range(WARM):
        call()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def adds_per_call(ids):
    """(run heads, leader loop): the adds one whole-target query issues, from the ID image: runs of equal IDs and distinct IDs per
    64-pixel row segment (segments start at column 0; 3840 = 60 whole segments)."""
    h, w = ids.shape
    seg = ids[:, :w // 64 * 64].reshape(h, w // 64, 64)
    runs = int((seg[..., 1:] != seg[..., :-1]).sum()) + h * (w // 64)
    srt = np.sort(seg, axis=-1)
    distinct = int((srt[..., 1:] != srt[..., :-1]).sum()) + h * (w // 64)
    return runs, distinct


def scenes(ctx):
    """[(name, draw the frame, n per primitive, items or None)] on a context with cfg4 resident at 3840 x 2160."""
    sc = S.cfg4_soup()
    n = sc.indices.size
    eighth = n // 8 // 3 * 3
    items = [(k * eighth, eighth if k < 7 else n - 7 * eighth, obj(k)) for k in range(8)]
    return sc, [("cfg4, one draw", lambda: ctx.draw(sc.transform, DT | IDS), None),
                ("cfg4, 8 objects", lambda: ctx.draw_list(items, DT | IDS), items)]


def count_only():
    """(d), one side: the swr_count_ids calls alone; prints one JSON line."""
    out = {}
    with swr_amd.Context() as ctx:
        sc, cases = scenes(ctx)
        ctx.scene_upload(sc.vertices, sc.indices)
        ctx.target_set(sc.width, sc.height)
        for name, draw, items in cases:
            draw()
            ctx.sync()
            out[f"{name} | per primitive"] = median_ms(lambda: ctx.count_ids(B.COUNT_PER_PRIMITIVE))[0]
            out[f"{name} | per item"] = median_ms(lambda: ctx.count_ids(B.COUNT_PER_ITEM))[0]
        ctx.scene_upload(*fill_scene())
        ctx.draw(S.identity(), DT | IDS)
        ctx.sync()
        out["one triangle | per primitive"] = median_ms(lambda: ctx.count_ids(B.COUNT_PER_PRIMITIVE))[0]
        out["one triangle | per item"] = median_ms(lambda: ctx.count_ids(B.COUNT_PER_ITEM))[0]
    print(json.dumps(out))


def fill_scene():
    xyz = np.array([[-3.0, -3.0, 0.5], [3.0, -3.0, 0.5], [0.0, 6.0, 0.5]], dtype=np.float32)
    return S.pack_vertices(xyz, np.full((3, 3), 0.5, dtype=np.float32)), np.arange(3, dtype=np.int64)


def main():
    if "--count-only" in sys.argv:
        return count_only()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []
    with swr_amd.Context() as ctx:
        sc, cases = scenes(ctx)
        W, H = sc.width, sc.height
        ctx.scene_upload(sc.vertices, sc.indices)
        ctx.target_set(W, H)
        pinned = B.HostImage((H, W), np.uint32)
        for name, draw, items in cases:
            draw()
            ctx.sync()
            n = sc.indices.size // 3

            def host_prim():
                ids = ctx.read_ids(out=pinned.array)
                live = ids[ids != NONE]
                return np.bincount(live, minlength=n), ids.size - live.size

            def host_item():
                ids = ctx.read_ids(out=pinned.array)
                k, _ = B.list_ids_to_items(ids, items)
                return np.bincount(k[k >= 0], minlength=len(items)), int((k < 0).sum())

            hc, hn = host_prim()
            gc, gn = ctx.count_ids(B.COUNT_PER_PRIMITIVE)
            assert np.array_equal(gc, hc.astype(np.uint32)) and gn == hn, name
            runs, distinct = adds_per_call(pinned.array)
            lines.append(f"{name}: {np.count_nonzero(hc)} visible primitives, {hn} pixels without; groups per whole-target query: "
                         f"run heads {runs}, leader loop {distinct} (of {W * H} pixels)")
            rows = [("read_ids (page-locked) alone", lambda: ctx.read_ids(out=pinned.array)),
                    ("host route, per primitive", host_prim),
                    ("swr_count_ids, per primitive", lambda: ctx.count_ids(B.COUNT_PER_PRIMITIVE)),
                    ("swr_count_ids, per primitive, 256 x 256", lambda: ctx.count_ids(B.COUNT_PER_PRIMITIVE, (1001, 777, 1257, 1033))),
                    ("swr_count_ids, per primitive, 1 x 1", lambda: ctx.count_ids(B.COUNT_PER_PRIMITIVE, (1919, 1079, 1920, 1080))),
                    ("swr_count_ids, per item", lambda: ctx.count_ids(B.COUNT_PER_ITEM))]
            if items is not None:
                ic, inone = host_item()
                gi, gin = ctx.count_ids(B.COUNT_PER_ITEM)
                assert np.array_equal(gi, ic.astype(np.uint32)) and gin == inone, name
                rows.insert(2, ("host route, per item", host_item))
            res = {}
            for label, call in rows:
                res[label] = median_ms(call)
                lines.append(f"  {label:42s} median {res[label][0]:8.3f} ms  (min {res[label][1]:.3f})")
            a, b = res["host route, per primitive"][0], res["swr_count_ids, per primitive"][0]
            lines.append(f"  per primitive: host route / swr_count_ids = {a / b:.1f} x")
            if items is not None:
                a, b = res["host route, per item"][0], res["swr_count_ids, per item"][0]
                lines.append(f"  per item:      host route / swr_count_ids = {a / b:.1f} x")
        # (c) one counter takes every add
        ctx.scene_upload(*fill_scene())
        ctx.draw(S.identity(), DT | IDS)
        ctx.sync()
        gc, gn = ctx.count_ids(B.COUNT_PER_PRIMITIVE)
        assert gc.tolist() == [W * H] and gn == 0
        runs, distinct = adds_per_call(ctx.read_ids(out=pinned.array))
        lines.append(f"one screen-filling triangle: groups per whole-target query: run heads {runs}, leader loop {distinct}, all of one counter")
        for label, call in (("swr_count_ids, per primitive", lambda: ctx.count_ids(B.COUNT_PER_PRIMITIVE)),
                            ("swr_count_ids, per item", lambda: ctx.count_ids(B.COUNT_PER_ITEM))):
            m = median_ms(call)
            lines.append(f"  {label:42s} median {m[0]:8.3f} ms  (min {m[1]:.3f})")
        pinned.free()
    libs = [sys.argv[i + 1] for i, v in enumerate(sys.argv[:-1]) if v == "--variant"]
    if libs:
        sides = ["this build"] + libs
        res = {side: [] for side in sides}
        for _ in range(2):
            for side in sides:
                env = dict(os.environ)
                env.pop("SWR_LIBRARY", None)
                if side != "this build":
                    env["SWR_LIBRARY"] = side
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--count-only"], env=env, capture_output=True, text=True,
                                   timeout=300, check=True)
                res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
        lines.append("(d) fresh processes alternating (" + ", ".join(os.path.basename(x) for x in sides) + "), median ms per call, two rounds:")
        for key in res["this build"][0]:
            lines.append(f"  {key:36s} " + "   ".join(os.path.basename(side) + " " + " ".join("%.3f" % r[key] for r in res[side]) for side in sides))
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
