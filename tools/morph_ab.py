#!/usr/bin/env python3
"""Morph targets (swr_scene_morph / swr_morph_set) against the only route a morphing mesh had before: swr_scene_upload of
vertices morphed on the CPU, every frame, on the PARENT build — the yardstick is never the code under test.  The scene is that of
tools/skin_ab.py: torus_mesh(1024, 512, 0.55, 0.2), 524 288 vertices, 1 048 576 triangles, 3840x2160, z-test, one device.
Per frame, the median of REPS after WARM, every side in a fresh process (SWR_LIBRARY), the sides alternating, ROUNDS rounds:
  (a) morph_set + draw + sync           new weights every frame: 1, 4 and 16 active targets of 16 resident, and 4 of 64 (this build,
                                        and --variant: the other delta layout);
  (b) scene_upload + draw + sync        the vertices morphed ahead of the clock by the numpy model (their cost is not counted);
  (c) draw + sync                       the unmorphed scene: the floor;
  morph_set alone                       the blocking call: the active list's copy, two kernels, one wait;
  morph_set + pose_set                  with the skin of tools/skin_ab.py: today the skin and stream passes run twice.
Before anything is timed, the depth image of (a) is compared with that of (b) for the same weights.
  --parent LIB     the parent commit's library (the yardstick (b)); without it (b) is this build's and is marked so
  --variant LIB    another build of this tree: make ab NAME=morph_pad ABFLAGS=-DSWR_TUNE_MORPH_PAD=1 (deltas as padded float4)
  --kernel N       only a loop of weight sets with N of 16 targets active, for a profiler run of its own (time against compulsory bytes):
                   rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/morph_ab.py --kernel 4
Run it under its own time limit: timeout -k 10 600 python3 tools/morph_ab.py --parent LIB [--variant LIB] [--out profiles/morph/morph_ab.txt]"""
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import swr_amd  # noqa: E402
import morph_model as MM  # noqa: E402
import skin_ab  # noqa: E402

S, B = swr_amd.scenes, swr_amd.binding
DT = S.FLAG_DEPTH_TEST
W, H = skin_ab.W, skin_ab.H
WARM, REPS, ROUNDS = 5, 30, 2
CASES = ((1, 16), (4, 16), (16, 16), (4, 64))       # (active, resident)


def targets(v, count):
    """`count` smooth targets: target t displaces every vertex along a direction that turns with t, by a wave of its own frequency
    around the ring.  Small: the image stays that of a torus."""
    p = v[:, 0:3]
    ring = np.arctan2(p[:, 1], p[:, 0])
    d = np.zeros((count, v.shape[0], 3), dtype=np.float32)
    for t in range(count):
        wave = (0.03 * np.sin((1 + t % 7) * ring + 0.37 * t)).astype(np.float32)
        d[t, :, 0] = wave * np.float32(math.cos(0.9 * t))
        d[t, :, 1] = wave * np.float32(math.sin(0.9 * t))
        d[t, :, 2] = wave * np.float32(0.5)
    return d


def weights(k, active, resident):
    """Weight set k: `active` non-zero weights, spread over the resident targets, new values every k."""
    w = np.zeros(resident, dtype=np.float32)
    pick = (np.arange(active) * resident) // active
    w[pick] = [0.2 + 0.8 * abs(math.sin(0.31 * k + 0.7 * j)) for j in range(active)]
    return w


def timed(call, reps=REPS, warm=WARM):
    t = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        call(k)
        t1 = time.perf_counter()
        if k >= warm:
            t.append((t1 - t0) * 1e3)
    return round(statistics.median(t), 4), round(min(t), 4)


def side():
    """One side: every case the loaded library can run; prints one JSON line {case: [median ms, min ms]}."""
    L = swr_amd.load_library()
    have = hasattr(L, "swr_morph_set")
    out = {}
    v, idx, joint, weight = skin_ab.scene()
    d16 = targets(v, 16)
    morphed = [MM.morph_vertices(v, d16, weights(k, 4, 16)) for k in range(2)]
    m = S.identity()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.target_set(W, H)

        def frame(k):
            ctx.draw(m, DT)
            ctx.sync()

        frame(0)
        out["(c) draw + sync, unmorphed"] = timed(frame)

        def upload_frame(k):
            ctx.scene_upload(morphed[k % 2], idx)
            frame(k)

        upload_frame(0)
        want = ctx.read_depth()
        out["(b) scene_upload + draw + sync"] = timed(upload_frame)
        if have:
            for active, resident in CASES:
                ctx.scene_upload(v, idx)
                ctx.scene_morph(d16 if resident == 16 else targets(v, resident))

                def morph_frame(k, active=active, resident=resident):
                    ctx.morph_set(weights(k, active, resident))
                    frame(k)

                morph_frame(0)
                if (active, resident) == (4, 16):
                    assert ctx.read_depth().tobytes() == want.tobytes(), "the morphed frame is not the uploaded one"
                out[f"(a) morph_set + draw + sync, {active} of {resident} active"] = timed(morph_frame)
                if (active, resident) == (4, 16):
                    out["morph_set alone, 4 of 16 active"] = timed(lambda k: ctx.morph_set(weights(k, 4, 16)))
            ctx.scene_upload(v, idx)
            ctx.scene_morph(d16)
            ctx.scene_skin(joint, weight)
            poses = [skin_ab.pose(k) for k in range(8)]

            def both(k):
                ctx.morph_set(weights(k, 4, 16))
                ctx.pose_set(poses[k % len(poses)])

            both(0)
            out["morph_set + pose_set, 4 of 16 active, 64 joints"] = timed(both)
    print(json.dumps(out))


def kernel_loop(active):
    v, idx, _, _ = skin_ab.scene()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.scene_morph(targets(v, 16))
        for k in range(50):
            ctx.morph_set(weights(k, active, 16))
    nv = v.shape[0]
    print(f"50 weight sets of {active} of 16 targets on {nv} vertices; compulsory bytes per call of k_morph_vertices: "
          f"{nv * (64 + 12 * active)} (32 read + 32 written + 12 per active target and vertex)")


def main():
    if "--side" in sys.argv:
        return side()
    if "--kernel" in sys.argv:
        return kernel_loop(int(sys.argv[sys.argv.index("--kernel") + 1]))
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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side"], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"{name}: exit {p.returncode}\n{p.stderr[-3000:]}")
            res[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"# {name}: done", file=sys.stderr, flush=True)
    lines = [f"torus {skin_ab.NU} x {skin_ab.NV}: {skin_ab.NU * skin_ab.NV} vertices, {2 * skin_ab.NU * skin_ab.NV} triangles, {W}x{H}, z-test, one "
             f"device; median ms per frame (minimum in brackets) of {REPS} after {WARM}, fresh processes alternating, {ROUNDS} rounds: "
             + ", ".join(name for name, _ in sides)]
    if not parent:
        lines.append("NO PARENT LIBRARY GIVEN: (b) below is this build's own swr_scene_upload")
    keys = []
    for name, _ in sides:
        for k in res[name][0]:
            if k not in keys:
                keys.append(k)
    for k in keys:
        lines.append(k)
        for name, _ in sides:
            vals = [r[k] for r in res[name] if k in r]
            if vals:
                lines.append(f"    {name:32s} " + "   ".join(f"{md:8.3f} ({lo:.3f})" for md, lo in vals))
    med = lambda name, k: statistics.median(r[k][0] for r in res[name])
    b_side = "parent" if parent else "this build"
    a = med("this build", "(a) morph_set + draw + sync, 4 of 16 active")
    b, c = med(b_side, "(b) scene_upload + draw + sync"), med("this build", "(c) draw + sync, unmorphed")
    lines.append(f"4 of 16 active: (b) / (a) = {b / a:.1f}    (a) - (c) = {a - c:.3f} ms")
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
