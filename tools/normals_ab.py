#!/usr/bin/env python3
"""Computed normals (swr_scene_normals) against the parent build, which has two routes to a lit deforming mesh: the
posed uploaded normals (swr_pose_set alone: wrong under scale, and all a morph without normal deltas gets), and normals from the host
every frame (swr_scene_attributes).  The yardstick is never the code under test.  The scene: torus_mesh(1024, 512, 0.55, 0.2),
524 288 vertices, 1 048 576 triangles, 64 joints along the ring, its own normals as attributes, a Phong material, 3840x2160, z-test,
one device.  Per frame, the median of REPS after WARM, every side in a fresh process (SWR_LIBRARY), the sides alternating, ROUNDS rounds:
  (p) pose_set + draw + sync                    the parent's, and this build's under SWR_NORMALS_UPLOADED: must be the same;
  (s) / (f) pose_set + draw + sync              this build under SWR_NORMALS_SMOOTH / SWR_NORMALS_FLAT: the added cost;
  (h) scene_attributes + draw + sync            the alternative today: normals from the host every frame — the upload alone, the
                                                host's own computation of them is not counted, which is generous to the parent;
  the setup call                                the first swr_scene_normals(SMOOTH) of a scene: the adjacency build on the host.
Before anything is timed, the SMOOTH frame is compared with the frame of a context that uploaded the model's normals.
  --parent LIB     the parent commit's library; without it the parent's rows are this build's and are marked so
  --kernel         only a loop of poses under SMOOTH, then FLAT, for a profiler run of its own (per kernel: time against compulsory
                   bytes):  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/normals_ab.py --kernel
Run it under its own time limit: timeout -k 10 600 python3 tools/normals_ab.py --parent LIB [--out profiles/normals/kernel.txt]"""
import dataclasses
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
import normals_model as NM  # noqa: E402
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
    return v, idx, joint, weight, S.torus_attrs(NU, NV)


def pose(k):
    """Pose k: every joint turns and breathes a little, out of phase with its neighbours."""
    return np.stack([SM.joint_matrix(0.05 * math.sin(0.3 * k + 0.4 * j), 1.0 + 0.05 * math.sin(0.2 * k + 0.7 * j),
                                     0.0, 0.02 * math.cos(0.25 * k + 0.5 * j)) for j in range(JOINTS)])


def material():
    light, half = S.light_rig()
    return B.Material.from_shading(S.Shading(np.zeros((1, 8), dtype=np.float32), S.SHADER_PHONG, 4, light, half, 0.2, 0.7, 0.5, None))


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
    have = hasattr(L, "swr_scene_normals")
    out = {}
    v, idx, joint, weight, attrs = scene()
    poses = [pose(k) for k in range(8)]
    m = S.identity()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.target_set(W, H)
        ctx.scene_attributes(attrs)
        ctx.material_set(material())
        ctx.scene_skin(joint, weight)

        def frame(k):
            ctx.draw(m, DT)
            ctx.sync()

        def pose_frame(k):
            ctx.pose_set(poses[k % len(poses)])
            frame(k)

        pose_frame(0)
        out["(p) pose_set + draw + sync, uploaded normals"] = timed(pose_frame)
        two = [attrs, np.ascontiguousarray(attrs[::-1])]

        def attr_frame(k):
            ctx.scene_attributes(two[k % 2])
            frame(k)

        attr_frame(0)
        out["(h) scene_attributes + draw + sync"] = timed(attr_frame)
        ctx.scene_attributes(attrs)
        if have:
            t0 = time.perf_counter()
            ctx.scene_normals("smooth")
            out["the setup call: the first swr_scene_normals(SMOOTH)"] = [round((time.perf_counter() - t0) * 1e3, 3)] * 2
            ctx.pose_set(poses[0])
            frame(0)
            got = (ctx.read_depth(), ctx.read_color())
            pv = SM.pose_vertices(v, joint, weight, poses[0])
            with swr_amd.Context() as ref:
                ref.scene_upload(pv, idx)
                ref.target_set(W, H)
                ref.scene_attributes(NM.smooth_attrs(attrs, pv, idx))
                ref.material_set(material())
                ref.draw(m, DT)
                ref.sync()
                assert ref.read_depth().tobytes() == got[0].tobytes() and np.array_equal(ref.read_color(), got[1]), "SMOOTH is not the model's frame"
            out["(s) pose_set + draw + sync, SMOOTH"] = timed(pose_frame)
            out["pose_set alone, SMOOTH"] = timed(lambda k: ctx.pose_set(poses[k % len(poses)]))
            out["swr_scene_normals alone: SMOOTH <-> FLAT (the adjacency is kept)"] = timed(lambda k: ctx.scene_normals("flat" if k % 2 == 0 else "smooth"))
            ctx.scene_normals("flat")
            out["(f) pose_set + draw + sync, FLAT"] = timed(pose_frame)
            out["pose_set alone, FLAT"] = timed(lambda k: ctx.pose_set(poses[k % len(poses)]))
            ctx.scene_normals(None)
            out["(p) pose_set + draw + sync, uploaded normals, after the modes"] = timed(pose_frame)
            out["pose_set alone, UPLOADED"] = timed(lambda k: ctx.pose_set(poses[k % len(poses)]))
    print(json.dumps(out))


def kernel_loop():
    v, idx, joint, weight, attrs = scene()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.scene_attributes(attrs)
        ctx.scene_skin(joint, weight)
        for mode in ("smooth", "flat"):
            ctx.scene_normals(mode)
            for k in range(50):
                ctx.pose_set(pose(k % 8))
    nv, ntri = v.shape[0], idx.size // 3
    print(f"50 poses each under SMOOTH and FLAT of {nv} vertices, {ntri} triangles, {JOINTS} joints; compulsory bytes per call: "
          f"k_face_normals {ntri * 88} (24 index + 48 gathered + 16 written per triangle), k_vertex_normals {nv * 24 + 3 * ntri * 20} "
          f"(8 row bounds + 16 written per vertex, 4 + 16 per adjacency entry), k_flat_normals {ntri * 84} (48 read + 36 written per slot); "
          f"resident for SMOOTH: {(nv + 1) * 4 + 3 * ntri * 4} bytes of adjacency, {ntri * 16} of faces, {nv * 16} of vertex normals")


def main():
    if "--side" in sys.argv:
        return side()
    if "--kernel" in sys.argv:
        return kernel_loop()
    arg = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
    out, parent = arg("--out"), arg("--parent")
    sides = ([("parent", parent)] if parent else []) + [("this build", None)]
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
    lines = [f"torus {NU} x {NV}: {NU * NV} vertices, {2 * NU * NV} triangles, {JOINTS} joints, Phong, {W}x{H}, z-test, one device; median ms "
             f"per frame (minimum in brackets) of {REPS} after {WARM}, fresh processes alternating, {ROUNDS} rounds: " + ", ".join(name for name, _ in sides)]
    if not parent:
        lines.append("NO PARENT LIBRARY GIVEN: the parent's rows are this build's own")
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
    p_side = "parent" if parent else "this build"
    kp, kh = "(p) pose_set + draw + sync, uploaded normals", "(h) scene_attributes + draw + sync"
    p, h = med(p_side, kp), med(p_side, kh)
    u, s, f = med("this build", kp), med("this build", "(s) pose_set + draw + sync, SMOOTH"), med("this build", "(f) pose_set + draw + sync, FLAT")
    lines.append(f"UPLOADED - parent = {u - p:+.3f} ms    SMOOTH - parent = {s - p:+.3f} ms    FLAT - parent = {f - p:+.3f} ms    "
                 f"parent's (h) - (p) = {h - p:+.3f} ms")
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
