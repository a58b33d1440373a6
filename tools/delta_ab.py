#!/usr/bin/env python3
"""Delta reads (swr_read_color_delta / swr_render_delta) against what a caller did before: swr_read_color into
page-locked memory, and the cached swr_render, both of the PARENT build — the yardstick is never the code under test.  3840x2160, one
device; per call the median of REPS calls after WARM warm-up calls; every side runs in a fresh process (SWR_LIBRARY), the sides
alternate, ROUNDS rounds.  A timed read starts after swr_sync, so it measures the read, not the frame.  Cases:
  the app's scene: examples/frame_loop.py's sphere, a new transform every frame (App.swift:169-183): the delta read into page-locked
    and into pageable memory against read_color, and swr_render_delta against the cached swr_render;
  a static frame: nothing changed, the cost of the compare and the round trip of the flag table alone;
  a half-changed frame: the top half of the image differs (images written with swr_target_write);
  cfg4 (1 M triangles) drawn with two transforms in turn: every tile changes, the worst case.
Every delivered image is compared with read_color's before anything is timed.
  --parent LIB     the parent commit's library (the yardsticks); without it the yardsticks are this build's and are marked so
  --variant LIB    another build of this tree: make ab NAME=delta_pack ABFLAGS=-DSWR_TUNE_DELTA_DIRECT=0 (the changed rectangle gathered
                   on the device, one linear copy into page-locked staging, rows copied by the host, also for a page-locked
                   destination) against the default (k_delta_tiles stores the changed tiles straight into a page-locked destination)
  --kernel         only a loop of static delta reads, for a profiler run of its own:
                   rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/delta_ab.py --kernel
Run it under its own time limit: timeout -k 10 900 python3 tools/delta_ab.py --parent LIB [--variant LIB] [--out profiles/delta/delta_ab.txt]"""
import importlib.util
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
W, H = 3840, 2160
WARM, REPS, ROUNDS = 5, 30, 2


def sphere():
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    return fl.sphere_mesh()


def timed(prepare, call, reps=REPS, warm=WARM):
    """Median and minimum ms of `call`, each after an untimed `prepare(k)`."""
    t = []
    for k in range(warm + reps):
        prepare(k)
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if k >= warm:
            t.append((t1 - t0) * 1e3)
    return round(statistics.median(t), 4), round(min(t), 4)


def side():
    """One side: every case the loaded library can run; prints one JSON line {case: [median ms, min ms] or a count}."""
    L = swr_amd.load_library()
    have = hasattr(L, "swr_read_color_delta")
    out = {}
    v, i = sphere()
    color, depth = swr_amd.HostImage((H, W, 4), np.uint8), swr_amd.HostImage((H, W), np.float32)
    pageable = np.zeros((H, W, 4), dtype=np.uint8)
    clock = [0.0]

    def transform():
        clock[0] += 1.0 / 60.0
        return S.app_transform(clock[0])

    with swr_amd.Context() as ctx:
        # the app's calling pattern: the same mesh, a new transform, the same two host images
        out["swr_render, cached"] = timed(lambda k: None, lambda: ctx.render(v, i, transform(), W, H, DT, color=color.array, depth=depth.array, scene_id=1))
        if have:
            stats = []
            out["swr_render_delta, cached"] = timed(lambda k: None, lambda: stats.append(
                ctx.render_delta(v, i, transform(), W, H, color, depth, DT, scene_id=1)))
            out["app scene: colour tiles changed (median)"] = statistics.median(s[0].tiles_changed for s in stats[WARM:])
            out["app scene: colour bytes copied (median)"] = statistics.median(s[0].bytes_copied for s in stats[WARM:])
            out["app scene: tiles"] = stats[-1][0].tiles
            assert np.array_equal(color.array, ctx.read_color()) and np.array_equal(depth.array.view(np.uint32), ctx.read_depth().view(np.uint32))
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)

        def frame(k):
            ctx.draw(transform(), DT)
            ctx.sync()

        frame(0)
        out["app scene: read_color, page-locked"] = timed(frame, lambda: ctx.read_color(out=color.array))
        if have:
            ctx.read_color_delta(color)
            ctx.read_color_delta(pageable)      # (one baseline: both images hold what it holds)
            frame(0)
            ctx.read_color_delta(color)
            assert np.array_equal(color.array, ctx.read_color())
            pageable[...] = color.array
            out["app scene: read_color_delta, page-locked"] = timed(frame, lambda: ctx.read_color_delta(color))
            pageable[...] = color.array
            out["app scene: read_color_delta, pageable"] = timed(frame, lambda: ctx.read_color_delta(pageable))
            assert np.array_equal(pageable, ctx.read_color())
            color.array[...] = pageable
            out["static frame: read_color_delta"] = timed(lambda k: None, lambda: ctx.read_color_delta(color))
            # a half-changed frame: two images that differ in the top half, written in turn
            a = ctx.read_color()
            b = a.copy()
            b[:H // 2] ^= 1
            ctx.target_write(a, None)
            ctx.read_color_delta(color)
            out["half changed: read_color_delta, page-locked"] = timed(lambda k: ctx.target_write(b if k % 2 == 0 else a, None),
                                                                       lambda: ctx.read_color_delta(color))
            assert np.array_equal(color.array, ctx.read_color())
        # cfg4 with two transforms in turn: every tile changes
        sc = S.cfg4_soup()
        ctx.scene_upload(sc.vertices, sc.indices)
        shifted = np.array(sc.transform, dtype=np.float32).reshape(16).copy()
        shifted[12] += 0.01

        def cfg4(k):
            ctx.draw(shifted if k % 2 == 0 else sc.transform, DT)
            ctx.sync()

        cfg4(1)
        out["cfg4: read_color, page-locked"] = timed(cfg4, lambda: ctx.read_color(out=color.array))
        if have:
            st = ctx.read_color_delta(color)
            cfg4(1)
            st = ctx.read_color_delta(color)
            out["cfg4: tiles changed"] = [st.tiles_changed, st.tiles]
            out["cfg4: read_color_delta, page-locked"] = timed(cfg4, lambda: ctx.read_color_delta(color))
            assert np.array_equal(color.array, ctx.read_color())
    color.free(); depth.free()
    print(json.dumps(out))


def kernel_loop():
    v, i = sphere()
    color = swr_amd.HostImage((H, W, 4), np.uint8)
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw(S.app_transform(0.0), DT)
        ctx.read_color_delta(color)
        for _ in range(50):
            assert ctx.read_color_delta(color).tiles_changed == 0
    color.free()
    print(f"50 static delta reads at {W}x{H}: k_delta_tiles reads {2 * W * H * 4} bytes per call")


def main():
    if "--side" in sys.argv:
        return side()
    if "--kernel" in sys.argv:
        return kernel_loop()
    arg = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
    out, parent, variant = arg("--out"), arg("--parent"), arg("--variant")
    sides = ([("parent", parent)] if parent else []) + [("this build", None)] + ([("variant " + os.path.basename(variant), variant)] if variant else [])
    res = {name: [] for name, _ in sides}
    for _ in range(ROUNDS):
        for name, lib in sides:
            env = dict(os.environ)
            env.pop("SWR_LIBRARY", None)
            if lib:
                env["SWR_LIBRARY"] = os.path.abspath(lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side"], env=env, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:
                sys.exit(f"{name}: exit {p.returncode}\n{p.stderr[-3000:]}")
            res[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"# {name}: done", file=sys.stderr, flush=True)
    lines = [f"{W}x{H}, one device; median ms per call (minimum in brackets) of {REPS} calls after {WARM}, fresh processes alternating, "
             f"{ROUNDS} rounds: " + ", ".join(name for name, _ in sides)]
    if not parent:
        lines.append("NO PARENT LIBRARY GIVEN: the yardsticks below are this build's own swr_read_color / swr_render")
    keys = []
    for name, _ in sides:
        for k in res[name][0]:
            if k not in keys:
                keys.append(k)
    for k in keys:
        lines.append(k)
        for name, _ in sides:
            vals = [r[k] for r in res[name] if k in r]
            if not vals:
                continue
            if isinstance(vals[0], list) and len(vals[0]) == 2 and isinstance(vals[0][0], float):
                lines.append(f"    {name:32s} " + "   ".join(f"{m:8.3f} ({lo:.3f})" for m, lo in vals))
            else:
                lines.append(f"    {name:32s} " + "   ".join(str(x) for x in vals))
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
