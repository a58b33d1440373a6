#!/usr/bin/env python3
"""Depth queries (swr_query_depth) against what a user did before: read_depth into page-locked memory plus a numpy loop
over the boxes on the host.  cfg4 (1 M triangles, 3840x2160) drawn z-tested once and complete (the calls measure the query, not the
frame); per call the median of REPS calls after WARM warm-up calls (the host loop over 4096 boxes: HOST_REPS calls).  Cases:
  8 object boxes (a 4 x 2 grid of 700 x 700 boxes at the octiles of the frame's finite depths);
  4096 boxes of mixed sizes (4 .. 400 pixels a side, depths drawn from the frame's);
  one whole-target box at the median depth (the worst case of a scan: most tiles straddle nothing, one workgroup would read them all);
  one 1 x 1 box.
For each: the host route, the read_depth copy alone, and swr_query_depth of this build.
  --variant LIB [--variant LIB ...]: the same swr_query_depth calls against other builds of the library, each in a fresh process
    (SWR_LIBRARY), alternating with this one, two rounds.  The builds:
      make ab NAME=dq_scan    ABFLAGS=-DSWR_TUNE_DEPTH_QUERY=0    the plain scan of every box: no summary, no split (the A/B base)
      make ab NAME=dq_noskip  ABFLAGS=-DSWR_TUNE_DEPTH_QUERY=1    the summary always, also for a query far smaller than the band
      make ab NAME=dq_nosplit ABFLAGS=-DSWR_TUNE_DEPTH_QUERY=2    large boxes walked by their one workgroup
      make ab NAME=dq_t8 / dq_t16 / dq_t32  ABFLAGS=-DSWR_TUNE_DEPTH_QUERY=8 / 16 / 32    the tile height T
Every result of swr_query_depth is compared with the host route's before it is timed.
Run it under its own time limit: timeout -k 10 600 python3 tools/depth_query_ab.py [--variant LIB ...] [--out profiles/depth_query/depth_query_ab.txt]"""
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

S, B = swr_amd.scenes, swr_amd.binding
DT = S.FLAG_DEPTH_TEST
WARM, REPS, HOST_REPS = 5, 30, 7


def median_ms(call, reps=REPS, warm=WARM):
    for _ in range(warm):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def host_counts(depth, boxes):
    out = np.zeros(boxes.size, dtype=np.uint32)
    for k, b in enumerate(boxes):
        out[k] = np.count_nonzero(b["z"] < depth[b["y0"]:b["y1"], b["x0"]:b["x1"]])
    return out


def boxes_of(rows):
    a = np.zeros(len(rows), dtype=B.DEPTH_BOX_DTYPE)
    for k, r in enumerate(rows):
        a[k] = (*r, (0, 0, 0))
    return a


def cases(depth):
    """[(name, boxes)] for a frame's depth image."""
    h, w = depth.shape
    finite = depth[np.isfinite(depth)]
    q = np.quantile(finite, np.linspace(0.1, 0.9, 8)).astype(np.float32) if finite.size else np.full(8, 0.5, np.float32)
    rng = np.random.default_rng(0xD0)
    objects = [(100 + 900 * (k % 4), 200 + 1000 * (k // 4), 800 + 900 * (k % 4), 900 + 1000 * (k // 4), q[k]) for k in range(8)]
    side = rng.integers(4, 401, (4096, 2))
    x, y = rng.integers(0, w - side[:, 0]), rng.integers(0, h - side[:, 1])
    z = finite[rng.integers(0, finite.size, 4096)] if finite.size else np.full(4096, 0.5, np.float32)
    mixed = [(int(x[k]), int(y[k]), int(x[k] + side[k, 0]), int(y[k] + side[k, 1]), z[k]) for k in range(4096)]
    med = np.float32(np.median(finite)) if finite.size else np.float32(0.5)
    return [("8 object boxes", boxes_of(objects)), ("4096 mixed boxes", boxes_of(mixed)),
            ("whole target, median depth", boxes_of([(0, 0, w, h, med)])), ("one 1 x 1 box", boxes_of([(w // 2, h // 2, w // 2 + 1, h // 2 + 1, med)]))]


def frame(ctx):
    sc = S.cfg4_soup()
    ctx.scene_upload(sc.vertices, sc.indices)
    ctx.target_set(sc.width, sc.height)
    ctx.draw(sc.transform, DT)
    ctx.sync()
    return sc


def query_only():
    """One side of --variant: the swr_query_depth calls alone; prints one JSON line."""
    out = {}
    with swr_amd.Context() as ctx:
        frame(ctx)
        depth = ctx.read_depth()
        for name, boxes in cases(depth):
            assert np.array_equal(ctx.query_depth(boxes), host_counts(depth, boxes)), name
            out[name] = median_ms(lambda: ctx.query_depth(boxes))[0]
    print(json.dumps(out))


def main():
    if "--query-only" in sys.argv:
        return query_only()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []

    def say(line):                  # (printed as it comes: a long run shows where it is)
        lines.append(line)
        print(line, flush=True)

    with swr_amd.Context() as ctx:
        sc = frame(ctx)
        W, H = sc.width, sc.height
        pinned = B.HostImage((H, W), np.float32)
        depth = ctx.read_depth(out=pinned.array)
        finite = np.isfinite(depth)
        say(f"cfg4 at {W}x{H}, z-tested: {int(finite.sum())} of {W * H} pixels covered, depths {depth[finite].min():.4f} .. "
            f"{depth[finite].max():.4f}, median {np.median(depth[finite]):.4f}")
        copy = median_ms(lambda: ctx.read_depth(out=pinned.array))
        say(f"  {'read_depth (page-locked) alone':44s} median {copy[0]:8.3f} ms  (min {copy[1]:.3f})")
        for name, boxes in cases(depth.copy()):
            area = int(((boxes["x1"] - boxes["x0"]).astype(np.int64) * (boxes["y1"] - boxes["y0"])).sum())
            want = host_counts(depth, boxes)
            got = ctx.query_depth(boxes)
            assert np.array_equal(got, want), name
            say(f"{name}: total box area {area} pixels ({area / (W * H):.2f} of the target), {int(want.sum(dtype=np.int64))} pixels pass")

            def host_route():
                return host_counts(ctx.read_depth(out=pinned.array), boxes)

            hr = median_ms(host_route, reps=HOST_REPS if boxes.size > 100 else REPS, warm=2 if boxes.size > 100 else WARM)
            dq = median_ms(lambda: ctx.query_depth(boxes))
            say(f"  {'host route (read_depth + numpy loop)':44s} median {hr[0]:8.3f} ms  (min {hr[1]:.3f})")
            say(f"  {'swr_query_depth':44s} median {dq[0]:8.3f} ms  (min {dq[1]:.3f})")
            say(f"  host route / swr_query_depth = {hr[0] / dq[0]:.1f} x; read_depth copy alone / swr_query_depth = {copy[0] / dq[0]:.2f} x")
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
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--query-only"], env=env, capture_output=True, text=True,
                                   timeout=200, check=True)
                res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(f"# {os.path.basename(side)}: done", file=sys.stderr, flush=True)
        say("fresh processes alternating (" + ", ".join(os.path.basename(x) for x in sides) + "), median ms per swr_query_depth call, two rounds:")
        for key in res["this build"][0]:
            say(f"  {key:28s} " + "   ".join(os.path.basename(side) + " " + " ".join("%.3f" % r[key] for r in res[side]) for side in sides))
    text = "\n".join(lines)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
