#!/usr/bin/env python3
"""Dual-quaternion skinning (swr_pose_set_dq) against the matrix pose (swr_pose_set, §23) of the SAME library: the
matrix kernel is byte for byte the parent's (profiles/skin_dq/vgprs.txt), so it is the yardstick.  The scene is §23's:
torus_mesh(1024, 512, 0.55, 0.2), 524 288 vertices, 1 048 576 triangles, 64 joints along the ring, 3840x2160, z-test, one device.  The
joints are rigid (a turn and a shift: what both kinds can express), the same motions for both kinds.
Per call, the median of REPS after WARM, every side in a fresh process, the sides alternating, ROUNDS rounds:
  pose + draw + sync          a new pose every frame, as swr_pose_set_dq and as swr_pose_set;
  pose alone                  the blocking call: the pose table's copy, two kernels, one wait.
Before anything is timed, the depth image after swr_pose_set_dq is compared with that of a swr_scene_upload of the model-posed
vertices (tests/skin_dq_model.py).
  --kernel         only a loop of 50 poses of each kind, for a profiler run of its own (per kernel: time against compulsory bytes):
                   rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/skin_dq_ab.py --kernel
  --attrs          with --kernel: the scene has attributes (the NRM instantiations: + 16 read + 16 written per vertex)
Run it under its own time limit: timeout -k 10 600 python3 tools/skin_dq_ab.py [--out profiles/skin_dq/skin_dq_ab.txt]"""
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
import skin_dq_model as DQ  # noqa: E402

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
    """Pose k as (JOINTS, 4, 4) rigid matrices: every joint turns about its own axis and shifts a little, out of phase with its
    neighbours."""
    return np.stack([DQ.rigid_matrix((math.sin(0.9 * j), math.cos(0.9 * j), 0.5), 0.08 * math.sin(0.3 * k + 0.4 * j),
                                     (0.0, 0.02 * math.cos(0.25 * k + 0.5 * j), 0.0)) for j in range(JOINTS)])


def timed(call, reps=REPS, warm=WARM):
    t = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        call(k)
        t1 = time.perf_counter()
        if k >= warm:
            t.append((t1 - t0) * 1e3)
    return round(statistics.median(t), 4), round(min(t), 4)


def side(kind):
    """One side: the calls of one kind; prints one JSON line {case: [median ms, min ms]}."""
    out = {}
    v, idx, joint, weight = scene()
    mats = [pose(k) for k in range(8)]
    tables = [B.dual_quats(m) for m in mats] if kind == "dq" else [DQ.column_major(m) for m in mats]
    m = S.identity()
    with swr_amd.Context() as ctx:
        ctx.target_set(W, H)
        setter = ctx.pose_set_dq if kind == "dq" else ctx.pose_set

        def frame(k):
            ctx.draw(m, DT)
            ctx.sync()

        if kind == "dq":
            ctx.scene_upload(DQ.pose_vertices(v, joint, weight, tables[0]), idx)
            frame(0)
            want = ctx.read_depth()
        ctx.scene_upload(v, idx)
        ctx.scene_skin(joint, weight)

        def pose_frame(k):
            setter(tables[k % len(tables)])
            frame(k)

        pose_frame(0)
        if kind == "dq":
            assert ctx.read_depth().tobytes() == want.tobytes(), "the posed frame is not the uploaded one"
        out["pose + draw + sync"] = timed(pose_frame)
        out["pose alone"] = timed(lambda k: setter(tables[k % len(tables)]))
    print(json.dumps(out))


def kernel_loop(attrs):
    v, idx, joint, weight = scene()
    mats = [pose(k) for k in range(8)]
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        if attrs:
            ctx.scene_attributes(S.torus_attrs(NU, NV))
        ctx.scene_skin(joint, weight)
        for k in range(50):
            ctx.pose_set_dq(B.dual_quats(mats[k % 8]))
        for k in range(50):
            ctx.pose_set(DQ.column_major(mats[k % 8]))
    nv = v.shape[0]
    per = 128 if attrs else 96
    print(f"50 poses of each kind, {nv} vertices, {JOINTS} joints, {'with' if attrs else 'no'} attributes; compulsory bytes per call of "
          f"k_skin_vertices_dq and of k_skin_vertices alike: {nv * per} ({per} per vertex)")


def main():
    if "--side" in sys.argv:
        return side(sys.argv[sys.argv.index("--side") + 1])
    if "--kernel" in sys.argv:
        return kernel_loop("--attrs" in sys.argv)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    sides = [("swr_pose_set_dq", "dq"), ("swr_pose_set", "matrix")]
    res = {name: [] for name, _ in sides}
    for _ in range(ROUNDS):
        for name, kind in sides:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", kind], capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"{name}: exit {p.returncode}\n{p.stderr[-3000:]}")
            res[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"# {name}: done", file=sys.stderr, flush=True)
    lines = [f"torus {NU} x {NV}: {NU * NV} vertices, {2 * NU * NV} triangles, {JOINTS} rigid joints, {W}x{H}, z-test, one device, one library; "
             f"median ms per call (minimum in brackets) of {REPS} after {WARM}, fresh processes alternating, {ROUNDS} rounds"]
    for k in res[sides[0][0]][0]:
        lines.append(k)
        for name, _ in sides:
            lines.append(f"    {name:18s} " + "   ".join(f"{md:8.3f} ({lo:.3f})" for md, lo in (r[k] for r in res[name])))
    med = lambda name, k: statistics.median(r[k][0] for r in res[name])
    for k in res[sides[0][0]][0]:
        a, b = med("swr_pose_set_dq", k), med("swr_pose_set", k)
        lines.append(f"{k}: swr_pose_set_dq - swr_pose_set = {a - b:+.4f} ms ({(a / b - 1) * 100:+.1f} %)")
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
