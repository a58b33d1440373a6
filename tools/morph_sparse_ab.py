#!/usr/bin/env python3
"""Sparse morph targets and swr_morph_pose_set against the PARENT build — the yardstick is never the code under test.
The scene is that of tools/skin_ab.py and tools/morph_ab.py: torus_mesh(1024, 512, 0.55, 0.2), 524 288 vertices, 1 048 576 triangles,
3840x2160, z-test, one device.  The rig: 64 targets, each a compact patch of about 3 % of the vertices (a run of consecutive vertex
numbers: a strip of the torus), neighbours overlapping by half.  This build holds it as sparse targets (swr_scene_morph_sparse); the
parent holds the same rig as 64 dense planes, zeros elsewhere (swr_scene_morph).
Per frame, the median of REPS after WARM, every side in a fresh process (SWR_LIBRARY), the sides alternating, ROUNDS rounds:
  target upload                          the blocking call that installs the rig (median of 3);
  morph_set + draw + sync                new weights every frame, 4 and 16 of the 64 active;
  weights and pose + draw + sync         with the skin of tools/skin_ab.py: the parent's morph_set + pose_set, this build's
                                         morph_pose_set (and, for reference, its own two-call sequence).
Before anything is timed, this build's sparse frame is compared with its own dense frame for the same weights.
  --parent LIB     the parent commit's library; without it only this build is measured
  --kernel N       only a loop of 50 weight sets with N of 64 active, for a profiler run of its own (k_morph_sparse here, k_morph_vertices
                   with SWR_LIBRARY set to the parent's library):  rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/morph_sparse_ab.py --kernel 4
Run it under its own time limit: timeout -k 10 900 python3 tools/morph_sparse_ab.py --parent LIB [--out profiles/morph_sparse/morph_sparse_ab.txt]"""
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
import skin_ab  # noqa: E402

S, B = swr_amd.scenes, swr_amd.binding
DT = S.FLAG_DEPTH_TEST
W, H = skin_ab.W, skin_ab.H
WARM, REPS, ROUNDS = 5, 30, 2
TARGETS, COVER = 64, 0.03
ACTIVE = (4, 16)


def rig(v):
    """The 64 sparse targets: (indices, deltas) per target."""
    nv = v.shape[0]
    n = int(nv * COVER)
    out = []
    for t in range(TARGETS):
        first = (t * (nv - n)) // (TARGETS - 1)
        idx = np.arange(first, first + n, dtype=np.uint32)
        bump = (0.03 * np.sin(np.linspace(0.0, math.pi, n)) ** 2).astype(np.float32)
        d = np.zeros((n, 3), dtype=np.float32)
        d[:, 0] = bump * np.float32(math.cos(0.9 * t))
        d[:, 1] = bump * np.float32(math.sin(0.9 * t))
        d[:, 2] = bump * np.float32(0.5)
        out.append((idx, d))
    return out


def dense(T, nv):
    d = np.zeros((len(T), nv, 3), dtype=np.float32)
    for t, (idx, x) in enumerate(T):
        d[t, idx] = x
    return d


def weights(k, active):
    w = np.zeros(TARGETS, dtype=np.float32)
    pick = (np.arange(active) * TARGETS) // active
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


def install(ctx, T, D, sparse):
    ctx.scene_morph_sparse(T) if sparse else ctx.scene_morph(D)


def side():
    """One side: what the loaded library can run; prints one JSON line {case: [median ms, min ms]}."""
    L = swr_amd.load_library()
    sparse = hasattr(L, "swr_scene_morph_sparse")
    kind = "sparse" if sparse else "dense"
    out = {}
    v, idx, joint, weight = skin_ab.scene()
    T = rig(v)
    D = dense(T, v.shape[0])
    m = S.identity()
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        ctx.target_set(W, H)

        def frame(k):
            ctx.draw(m, DT)
            ctx.sync()

        if sparse:      # the sparse frame is the dense frame (the torus has no -0 coordinate, the weights are finite)
            ctx.scene_morph(D)
            ctx.morph_set(weights(0, 4))
            frame(0)
            want = ctx.read_depth()
            ctx.scene_morph_sparse(T)
            ctx.morph_set(weights(0, 4))
            frame(0)
            assert ctx.read_depth().tobytes() == want.tobytes(), "the sparse frame is not the dense one"
        out["target upload"] = timed(lambda k: install(ctx, T, D, sparse), reps=3, warm=1)
        for active in ACTIVE:
            def morph_frame(k, active=active):
                ctx.morph_set(weights(k, active))
                frame(k)

            morph_frame(0)
            out[f"morph_set + draw + sync, {active} of {TARGETS} active"] = timed(morph_frame)
            out[f"morph_set alone, {active} of {TARGETS} active"] = timed(lambda k, active=active: ctx.morph_set(weights(k, active)))
        ctx.scene_skin(joint, weight)
        poses = [skin_ab.pose(k) for k in range(8)]

        def two_calls(k):
            ctx.morph_set(weights(k, 4))
            ctx.pose_set(poses[k % len(poses)])
            frame(k)

        two_calls(0)
        out["morph_set + pose_set + draw + sync, 4 active, 64 joints"] = timed(two_calls)
        if sparse:
            def one_call(k):
                ctx.morph_pose_set(weights(k, 4), poses[k % len(poses)])
                frame(k)

            one_call(0)
            out["morph_pose_set + draw + sync, 4 active, 64 joints"] = timed(one_call)
    entries = sum(t[0].size for t in T)
    touched = np.unique(np.concatenate([t[0] for t in T])).size
    out["resident bytes"] = [TARGETS * v.shape[0] * 12, 0] if not sparse else [entries * 16 + touched * 12 + 8, 0]
    print(json.dumps({"kind": kind, "cases": out}))


def kernel_loop(active):
    L = swr_amd.load_library()
    sparse = hasattr(L, "swr_scene_morph_sparse")
    v, idx, _, _ = skin_ab.scene()
    T = rig(v)
    with swr_amd.Context() as ctx:
        ctx.scene_upload(v, idx)
        install(ctx, T, None if sparse else dense(T, v.shape[0]), sparse)
        for k in range(50):
            ctx.morph_set(weights(k, active))
    print(f"50 weight sets of {active} of {TARGETS} {'sparse' if sparse else 'dense'} targets on {v.shape[0]} vertices")


def main():
    if "--side" in sys.argv:
        return side()
    if "--kernel" in sys.argv:
        return kernel_loop(int(sys.argv[sys.argv.index("--kernel") + 1]))
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
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side"], env=env, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:
                sys.exit(f"{name}: exit {p.returncode}\n{p.stderr[-3000:]}")
            r = json.loads(p.stdout.strip().splitlines()[-1])
            res[name].append(r["cases"])
            print(f"# {name} ({r['kind']} targets): done", file=sys.stderr, flush=True)
    lines = [f"torus {skin_ab.NU} x {skin_ab.NV}: {skin_ab.NU * skin_ab.NV} vertices, {2 * skin_ab.NU * skin_ab.NV} triangles, {W}x{H}, z-test, one "
             f"device; {TARGETS} targets of {COVER:.0%} of the vertices each (parent: dense planes, this build: sparse); median ms per frame "
             f"(minimum in brackets) of {REPS} after {WARM}, fresh processes alternating, {ROUNDS} rounds: " + ", ".join(name for name, _ in sides)]
    keys = []
    for name, _ in sides:
        for k in res[name][0]:
            if k not in keys:
                keys.append(k)
    for k in keys:
        lines.append(k)
        for name, _ in sides:
            vals = [r[k] for r in res[name] if k in r]
            if vals and k == "resident bytes":
                lines.append(f"    {name:32s} {vals[0][0]:12d}")
            elif vals:
                lines.append(f"    {name:32s} " + "   ".join(f"{md:8.3f} ({lo:.3f})" for md, lo in vals))
    text = "\n".join(lines)
    print(text)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
