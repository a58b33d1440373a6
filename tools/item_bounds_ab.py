#!/usr/bin/env python3
"""Item bounds (swr_item_bounds): what a call costs, against what a user did before and against drawing the items.
The scene is a torus of 1 000 000 triangles (1000 x 500 quads) at 3840x2160, resident; per call the median of REPS calls after WARM
warm-up calls.  Lists:
  1 item          the whole torus under the app's matrix;
  9 ranges        the torus cut into 9 consecutive ranges, each under its own matrix (1 M triangles in all);
  512 ranges      the same with 512 ranges;
  9 instances     the whole torus under 9 matrices (9 M triangle transforms: the instancing case K = 9);
  512 instances   one range of 32 000 triangles under 512 matrices (16.4 M: a list holds fewer than 2^24 triangles; K = 512).
States: unposed, posed (swr_scene_skin + swr_pose_set), morphed (swr_scene_morph + swr_morph_set).  For each list and state the call,
and the bytes per second of the compulsory 48 bytes per triangle it reads; for the unposed state also
  the parent's route: examples/frame_loop.py's object_boxes, float64 numpy on the host (whole-mesh items only, few repetitions);
  the depth-only z-tested swr_draw_list frame of the same items, drawn and waited for (median of 10 after 3).
Every result is compared with tests/item_bounds_model.py on a sample of the items before it is timed.  The lists are converted to the
structured array swr_item_bounds reads once, ahead of the clock (512 tuples take Python half a millisecond per call otherwise).
  --variant LIB [--variant LIB ...]: the same swr_item_bounds calls against other builds of the library, each in a fresh process
    (SWR_LIBRARY), alternating with this one, two rounds.  The builds:
      make ab NAME=ib_gather    ABFLAGS=-DSWR_TUNE_ITEM_BOUNDS=1   the index gather through the vertex array in effect, no cut
      make ab NAME=ib_instanced ABFLAGS=-DSWR_TUNE_ITEM_BOUNDS=2   items over one range read their triangles once (per chunk, from L2 after the first matrix)
  --kernel: 50 calls of the 1-item list and 50 of the 9 instances and nothing else, for a profiler run of its own
    (rocprofv3 --kernel-trace --stats -- python3 tools/item_bounds_ab.py --kernel; SWR_LIBRARY selects the build).
Run it under its own time limit: timeout -k 10 600 python3 tools/item_bounds_ab.py [--variant LIB ...] [--out profiles/item_bounds/item_bounds_ab.txt]"""
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import swr_amd  # noqa: E402
import item_bounds_model as M  # noqa: E402

S, B = swr_amd.scenes, swr_amd.binding
DT, NC = S.FLAG_DEPTH_TEST, S.FLAG_NO_COLOR
WARM, REPS = 5, 30
W, H = 3840, 2160
STATES = ("unposed", "posed", "morphed")


def frame_loop():
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    return fl


def median_ms(call, reps=REPS, warm=WARM):
    for _ in range(warm):
        call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def torus():
    xyz, rgb, idx = S.torus_mesh(1000, 500, 0.3, 0.1)
    return S.pack_vertices(xyz, rgb), idx


def lists(fl, ntri):
    """[(name, items as tuples, triangle transforms)]"""
    def ranges(n):
        cut = [ntri * k // n for k in range(n + 1)]
        m = fl.object_transforms(0.3, n)
        return [(3 * cut[k], 3 * (cut[k + 1] - cut[k]), m[k]) for k in range(n)]
    m9, m512 = fl.object_transforms(0.3, 9), fl.object_transforms(0.3, 512)
    return [("1 item", [(0, 3 * ntri, S.app_transform(0.3))], ntri),
            ("9 ranges", ranges(9), ntri),
            ("512 ranges", ranges(512), ntri),
            ("9 instances", [(0, 3 * ntri, m) for m in m9], 9 * ntri),
            ("512 instances", [(3 * 1000, 3 * 32000, m) for m in m512], 512 * 32000)]


def enter(ctx, fl, v, state):
    """Puts the resident scene into `state` (the states are entered in the order of STATES)."""
    if state == "posed":
        ctx.scene_skin(*fl.bend_skin(v))
        ctx.pose_set(fl.bend_pose(0.3))
    elif state == "morphed":
        ctx.scene_skin(None)                    # the bind pose again
        ctx.scene_morph(fl.morph_targets(v))
        ctx.morph_set(fl.morph_weights(0.3))


def check_sample(ctx, v, idx, items, flags=0):
    """A few items of the list against the numpy model (unposed vertices only)."""
    got = ctx.item_bounds(items, flags)
    for k in sorted({0, len(items) // 2, len(items) - 1}):
        want = M.item_bound(v, idx, items[k][0], min(items[k][1], 3 * 40000), items[k][2], W, H, flags)
        part = ctx.item_bounds([(items[k][0], min(items[k][1], 3 * 40000), items[k][2])], flags)[0]
        assert part.tobytes() == want.tobytes(), (k, part, want)
    return got


def kernel_loop():
    fl = frame_loop()
    v, idx = torus()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.target_set(W, H)
        for name, items, _ in lists(fl, idx.size // 3):
            if name in ("1 item", "9 instances"):
                arr = B.Context.draw_items(items)
                for _ in range(50):
                    ctx.item_bounds(arr)


def bounds_only():
    """One side of --variant: the swr_item_bounds calls alone; prints one JSON line."""
    fl = frame_loop()
    v, idx = torus()
    out = {}
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.target_set(W, H)
        for state in STATES:
            enter(ctx, fl, v, state)
            for name, items, _ in lists(fl, idx.size // 3):
                if state == "unposed":
                    check_sample(ctx, v, idx, items)
                arr = B.Context.draw_items(items)
                out[f"{name}, {state}"] = median_ms(lambda: ctx.item_bounds(arr))[0]
    print(json.dumps(out))


def main():
    if "--bounds-only" in sys.argv:
        return bounds_only()
    if "--kernel" in sys.argv:
        return kernel_loop()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []

    def say(line):                  # (printed as it comes: a long run shows where it is)
        lines.append(line)
        print(line, flush=True)

    fl = frame_loop()
    v, idx = torus()
    ntri = idx.size // 3
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.target_set(W, H)
        say(f"torus of {ntri} triangles ({v.shape[0]} vertices) at {W}x{H}; median of {REPS} calls after {WARM}, ms (min in brackets)")
        for state in STATES:
            enter(ctx, fl, v, state)
            for name, items, work in lists(fl, ntri):
                if state == "unposed":
                    b = check_sample(ctx, v, idx, items)
                    say(f"{name}: {work} triangle transforms; item 0: x [{b['x0'][0]}, {b['x1'][0]}) y [{b['y0'][0]}, {b['y1'][0]}) "
                        f"z [{b['zmin'][0]:.4f}, {b['zmax'][0]:.4f}], drawable {b['drawable'][0]}, behind {b['behind'][0]}")
                arr = B.Context.draw_items(items)
                ib = median_ms(lambda: ctx.item_bounds(arr))
                say(f"  {name + ', ' + state:26s} swr_item_bounds {ib[0]:8.3f} ({ib[1]:.3f})   {work * 48 / (ib[0] * 1e-3) / 1e9:8.1f} GB/s of 48 B per triangle")
                if state != "unposed":
                    continue
                if len(items) <= 9 and items[0][1] == 3 * ntri:
                    hr = median_ms(lambda: fl.object_boxes(v, [m for _, _, m in items], W, H), reps=5, warm=1)
                    say(f"  {'':26s} object_boxes on the host (numpy float64, all vertices) {hr[0]:8.3f} ({hr[1]:.3f})   = {hr[0] / ib[0]:.1f} x the call")

                def frame():
                    ctx.draw_list(arr, DT | NC)
                    ctx.sync()
                fr = median_ms(frame, reps=10, warm=3)
                say(f"  {'':26s} the depth-only z-tested swr_draw_list frame of the same items, waited for {fr[0]:8.3f} ({fr[1]:.3f})   "
                    f"bounds / frame = {ib[0] / fr[0]:.2f}")
    libs = [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--variant"]
    if libs:
        sides = ["this build"] + libs
        res = {side: [] for side in sides}
        for _ in range(2):
            for side in sides:
                env = dict(os.environ)
                env.pop("SWR_LIBRARY", None)
                if side != "this build":
                    env["SWR_LIBRARY"] = side
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--bounds-only"], env=env, capture_output=True, text=True,
                                   timeout=250, check=True)
                res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(f"# {os.path.basename(side)}: done", file=sys.stderr, flush=True)
        say("fresh processes alternating (" + ", ".join(os.path.basename(x) for x in sides) + "), median ms per swr_item_bounds call, two rounds:")
        for key in res["this build"][0]:
            say(f"  {key:26s} " + "   ".join(os.path.basename(side) + " " + " ".join("%.3f" % r[key] for r in res[side]) for side in sides))
    text = "\n".join(lines)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
