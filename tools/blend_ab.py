#!/usr/bin/env python3
"""Cost of alpha blending (SWR_FLAG_BLEND): the blend load frame (SWR_BLEND_OVER, opacity 128) of a scene against the
same scene's painter's-order load frame on the existing kernel, passthrough fragment stage on both sides:
  (a) cfg3's mesh at 4K,  (b) cfg5's mesh,  (c) 300 screen-filling triangles at 1080p,  (d) cfg4 (1 M tiny triangles) at 4K.
Per side: HIP-event times (swr_timing_enable(2), pipelining off) summed over --frames frames — the raster share (for a blend frame:
k_blend_order + k_raster_blend) and the whole frame — the two sides alternating --reps times, medians reported.
Run it under its own time limit: timeout -k 10 600 python3 tools/blend_ab.py [--reps 5] [--frames 30] [--only c]"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import swr_amd  # noqa: E402

S = swr_amd.scenes
B = swr_amd.binding
LOAD, BLEND = B.FLAG_LOAD, B.FLAG_BLEND


def screen_fillers(n=300, seed=7):
    rng = np.random.default_rng(seed)
    v = np.zeros((3 * n, 8), dtype=np.float32)
    base = np.array([(-1.3, -1.2), (1.4, -1.1), (0.0, 1.5)], dtype=np.float32)
    v[:, 0:2] = (base[None] + rng.uniform(-0.2, 0.2, (n, 3, 2))).reshape(-1, 2)
    v[:, 2] = rng.uniform(0.1, 0.9, 3 * n)
    v[:, 4:7] = rng.uniform(0, 1, (3 * n, 3))
    return v, np.arange(3 * n, dtype=np.int64)


def scenes(only):
    ident = np.eye(4, dtype=np.float32).T.reshape(16)
    if "a" in only:
        s = S.cfg3_phong()
        yield "(a) cfg3 mesh", s.vertices, s.indices, s.transform, s.width, s.height
    if "b" in only:
        s = S.cfg5_textured()
        yield "(b) cfg5 mesh", s.vertices, s.indices, s.transform, s.width, s.height
    if "c" in only:
        v, i = screen_fillers()
        yield "(c) 300 screen-filling 1080p", v, i, ident, 1920, 1080
    if "d" in only:
        s = S.cfg4_soup()
        yield "(d) cfg4 1M tiny 4K", s.vertices, s.indices, s.transform, s.width, s.height


def measure(ctx, m, flags, frames):
    for _ in range(3):
        ctx.draw(m, flags)
    ctx.sync()
    ctx.timing_reset()
    for _ in range(frames):
        ctx.draw(m, flags)
    ctx.sync()
    t, n = ctx.timing_totals()
    return t["raster_ms"] / max(n, 1), t["total_ms"] / max(n, 1)


def main():
    arg = lambda k, d: type(d)(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
    reps, frames, only = arg("--reps", 5), arg("--frames", 30), arg("--only", "abcd")
    for name, v, i, m, w, h in scenes(only):
        with swr_amd.Context() as ctx:
            ctx.scene_upload(v, i)
            ctx.target_set(w, h)
            ctx.pipeline_enable(False)
            ctx.timing_enable(2)
            ctx.blend_set(B.BLEND_OVER, 128)
            ctx.draw(m, 0)
            ctx.sync()
            rows = {"painter": [], "blend": []}
            for _ in range(reps):
                rows["painter"].append(measure(ctx, m, LOAD, frames))
                rows["blend"].append(measure(ctx, m, LOAD | BLEND, frames))
            med = {k: (statistics.median(x[0] for x in r), statistics.median(x[1] for x in r)) for k, r in rows.items()}
            for k in ("painter", "blend"):
                print(f"{name:30s} {k:8s} raster ms {' '.join('%.4f' % x[0] for x in rows[k])}  (median {med[k][0]:.4f})   "
                      f"frame ms (median) {med[k][1]:.4f}", flush=True)
            print(f"{name:30s} blend / painter: raster x{med['blend'][0] / med['painter'][0]:.2f}, "
                  f"frame x{med['blend'][1] / med['painter'][1]:.2f}", flush=True)


if __name__ == "__main__":
    main()
