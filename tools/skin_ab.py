#!/usr/bin/env python3
"""Skinned meshes (swr_scene_skin / swr_pose_set) against the only route a deforming mesh had before: swr_scene_upload
of vertices posed on the CPU, every frame, on the PARENT build — the yardstick is never the code under test.  The scene:
torus_mesh(1024, 512, 0.55, 0.2), 524 288 vertices, 1 048 576 triangles, 64 joints along the ring, 3840x2160, z-test, one device.
Per frame, the median of REPS after WARM, every side in a fresh process (SWR_LIBRARY), the sides alternating, ROUNDS rounds:
  (a) pose_set + draw + sync            a new pose every frame (this build, and --variant);
  (b) scene_upload + draw + sync        the vertices posed ahead of the clock by the numpy model (their cost is not counted);
  (c) draw + sync                       the unposed scene: the floor;
  pose_set alone                        the blocking call: the pose table's copy, two kernels, one wait.
Before anything is timed, the depth image of (a) is compared with that of (b) for the same pose.
  --parent LIB     the parent commit's library (the yardstick (b)); without it (b) is this build's and is marked so
  --variant LIB    another build of this tree: make ab NAME=skin_l2 ABFLAGS=-DSWR_TUNE_SKIN_LDS=0 (the pose table left to L2)
  --kernel         only a loop of poses, for a profiler run of its own (per kernel: time against compulsory bytes):
                   rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/skin_ab.py --kernel
Run it under its own time limit: timeout -k 10 600 python3 tools/skin_ab.py --parent LIB [--variant LIB] [--out profiles/skin/skin_ab.txt]"""
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
import swr_amd  # noqa: E402
import skin_model as SM  # noqa: E402

S, B = swr_amd.scenes, swr_amd.binding
DT = S.FLAG_DEPTH_TEST
W, H = 3840, 2160
NU, NV, JOINTS = 1024, 512, 64
WARM, REPS, ROUNDS = 5, 30, 2


def scene():
    xyz, rgb, idx = S.torus_mesh(NU, NV, 0.55, 0.2)
    v = S.pack_vertices(xyz, rgb)
    iu = np.repeat(np.arange(NU), NV)
    f = iu * (JOINTS / NU)
    j0 = np.floor(f).astype(np.int64)
    t = (f - j0).astype(np.float32)
    joint = np.stack([j0 % JOINTS, (j0 + 1) % JOINTS, (j0 + 2) % JOINTS, (j0 + 3) % JOINTS], axis=1).astype(np.uint32)
    weight = np.stack([1 - t, t, np.zeros_like(t), np.zeros_like(t)], axis=1).astype(np.float32)
    return v, idx, joint, weight


def pose(k):
    """Pose k: every joint turns and breathes a little, out of phase with its neighbours."""
    return np.stack([SM.joint_matrix(0.05 * math.sin(0.3 * k + 0.4 * j), 1.0 + 0.05 * math.sin(0.2 * k + 0.7 * j),
                                     0.0, 0.02 * math.cos(0.25 * k + 0.5 * j)) for j in range(JOINTS)])


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
    have = hasattr(L, "swr_pose_set")
    out = {}
    v, idx, joint, weight = scene()
    poses = [pose(k) for k in range(8)]
    posed = [SM.pose_vertices(v, joint, weight, p) for p in poses[:2]]
    m = S.identity()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.target_set(W, H)

        def frame(k):
            ctx.draw(m, DT)
            ctx.sync()

        frame(0)
        out["(c) draw + sync, unposed"] = timed(frame)

        def upload_frame(k):
            ctx.scene_upload(posed[k % 2], idx)
            frame(k)

        upload_frame(0)
        want = ctx.read_depth()
        out["(b) scene_upload + draw + sync"] = timed(upload_frame)
        if have:
            ctx.scene_upload(v, idx)
            ctx.scene_skin(joint, weight)

            def pose_frame(k):
                ctx.pose_set(poses[k % len(poses)])
                frame(k)

            pose_frame(0)
            assert ctx.read_depth().tobytes() == want.tobytes(), "the posed frame is not the uploaded one"
            out["(a) pose_set + draw + sync"] = timed(pose_frame)
            out["pose_set alone"] = timed(lambda k: ctx.pose_set(poses[k % len(poses)]))
            out["pose_set(NULL) alone: the bind pose (every other call)"] = timed(lambda k: ctx.pose_set(None if k % 2 else poses[0]))
    print(json.dumps(out))


def kernel_loop():
    v, idx, joint, weight = scene()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.scene_skin(joint, weight)
        for k in range(50):
            ctx.pose_set(pose(k % 8))
    nv, ntri = v.shape[0], idx.size // 3
    print(f"50 poses of {nv} vertices, {ntri} triangles, {JOINTS} joints; compulsory bytes per call: k_skin_vertices {nv * 96} "
          f"(32 read + 32 skin + 32 written per vertex), k_skin_stream {ntri * 64} (24 index + 4 original index + 36 written per "
          f"triangle; the 48 gathered come from the {nv * 32}-byte posed array)")


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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side"], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"{name}: exit {p.returncode}\n{p.stderr[-3000:]}")
            res[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"# {name}: done", file=sys.stderr, flush=True)
    lines = [f"torus {NU} x {NV}: {NU * NV} vertices, {2 * NU * NV} triangles, {JOINTS} joints, {W}x{H}, z-test, one device; median ms per "
             f"frame (minimum in brackets) of {REPS} after {WARM}, fresh processes alternating, {ROUNDS} rounds: " + ", ".join(name for name, _ in sides)]
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
    a, b, c = med("this build", "(a) pose_set + draw + sync"), med(b_side, "(b) scene_upload + draw + sync"), med("this build", "(c) draw + sync, unposed")
    lines.append(f"(b) / (a) = {b / a:.1f}    (a) - (c) = {a - c:.3f} ms")
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
