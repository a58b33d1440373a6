#!/usr/bin/env python3
"""Ray casts (swr_cast_rays): what a call costs, what the group cull saves, and what it is measured against.
The scene is a torus of 1 000 000 triangles (1000 x 500 quads) skinned to 64 joints around the ring and posed, resident.  Ray sets:
  1 ray           straight down onto the tube of the torus;
  1 024 rays      random origins on a sphere around the torus, aimed at random points inside its box;
  65 536 rays     the camera rays of the 256 x 256 target (binding.pixel_ray of every pixel).
For each set: the whole call (median of REPS calls after WARM, upload and read-back included); the per-ray work the numpy model counts
on the posed vertices in the order of the index array (group boxes tested, groups entered, triangles tested: tests/rays_model.work on
up to 256 of the rays); the bytes per second of the 32 bytes per group box a ray's pass over box64 reads; and, for the single ray,
swr_item_bounds with one item over the same stream — the project's measured cost of one 48-byte-per-triangle walk.  Every set is
compared with tests/rays_model.py on a sample before it is timed.
  --variant LIB [--variant LIB ...]: the same calls against other builds of the library, each in a fresh process (SWR_LIBRARY),
    alternating with this one, two rounds.  The build this is for:
      make ab NAME=rays_brute ABFLAGS=-DSWR_TUNE_RAYS_CULL=0        every group is entered: brute force, the upper bound
  --kernel: 20 calls of each ray set, then 20 of swr_item_bounds, and nothing else, for a profiler run of its own
    (rocprofv3 --kernel-trace --stats -- python3 tools/rays_ab.py --kernel; SWR_LIBRARY selects the build).
Run it under its own time limit: timeout -k 10 600 python3 tools/rays_ab.py [--variant LIB ...] [--out profiles/rays/bench_ab.txt]"""
import json
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
import rays_model as R  # noqa: E402
import skin_model as SM  # noqa: E402

S, B = swr_amd.scenes, swr_amd.binding
WARM, REPS = 3, 15
SIZE = 256
JOINTS = 64


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


def ring_skin(v):
    """64 joints around the ring: a vertex at angle a blends the two joints next to it."""
    a = (np.arctan2(v[:, 1], v[:, 0]) / (2 * np.pi) % 1.0) * JOINTS
    j0 = np.floor(a).astype(np.uint32) % JOINTS
    t = (a - np.floor(a)).astype(np.float32)
    joints = np.zeros((v.shape[0], 4), dtype=np.uint32)
    joints[:, 0], joints[:, 1] = j0, (j0 + 1) % JOINTS
    weights = np.zeros((v.shape[0], 4), dtype=np.float32)
    weights[:, 0], weights[:, 1] = 1.0 - t, t
    return joints, weights


def ring_pose():
    """Every joint turns a little about z and lifts along z: the ring waves."""
    k = np.arange(JOINTS)
    return np.stack([SM.joint_matrix(0.05 * np.sin(k[j] * 0.4), 1.0, 0.0, 0.0, 0.04 * np.sin(k[j] * 2 * np.pi / JOINTS * 3)) for j in range(JOINTS)])


def ray_sets():
    m = S.app_transform(0.3)
    one = np.zeros(1, dtype=B.RAY_DTYPE)
    one["origin"], one["dir"], one["tmax"] = (0.3, 0.01, 1.0), (0.0, 0.0, -1.0), 4.0
    rng = np.random.default_rng(0x4AB)
    d = rng.normal(size=(1024, 3))
    o = d / np.linalg.norm(d, axis=1, keepdims=True) * 0.9
    target = rng.uniform(-1, 1, (1024, 3)) * np.array([0.4, 0.4, 0.1])
    rnd = np.zeros(1024, dtype=B.RAY_DTYPE)
    rnd["origin"], rnd["dir"], rnd["tmax"] = o, target - o, 4.0
    xs, ys = np.meshgrid(np.arange(SIZE), np.arange(SIZE))
    cam = B.pixel_ray(m, SIZE, SIZE, xs, ys).reshape(-1)
    return [("1 ray", one), ("1 024 random rays", rnd), ("65 536 camera rays", cam)]


def resident(ctx, v, idx):
    ctx.scene_upload(v, idx)
    ctx.target_set(SIZE, SIZE)
    ctx.scene_skin(*ring_skin(v))
    ctx.pose_set(ring_pose())


def kernel_loop():
    v, idx = torus()
    with swr_amd.Context() as ctx:
        resident(ctx, v, idx)
        for _, rays in ray_sets():
            for _ in range(20):
                ctx.cast_rays(rays)
        item = B.Context.draw_items([(0, idx.size, S.app_transform(0.3))])
        for _ in range(20):                     # (k_item_bounds over the same stream: the cost of one walk)
            ctx.item_bounds(item)


def casts_only():
    """One side of --variant: the swr_cast_rays calls alone; prints one JSON line."""
    v, idx = torus()
    out = {}
    with swr_amd.Context() as ctx:
        resident(ctx, v, idx)
        for name, rays in ray_sets():
            out[name] = median_ms(lambda: ctx.cast_rays(rays))[0]
    print(json.dumps(out))


def main():
    if "--casts-only" in sys.argv:
        return casts_only()
    if "--kernel" in sys.argv:
        return kernel_loop()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    v, idx = torus()
    ntri = idx.size // 3
    groups = (ntri + 63) // 64
    joints, weights = ring_skin(v)
    tri = R.triangles(SM.pose_vertices(v, joints, weights, ring_pose()), idx)
    with swr_amd.Context() as ctx:
        resident(ctx, v, idx)
        say(f"torus of {ntri} triangles ({groups} groups of 64) posed by {JOINTS} joints; median of {REPS} calls after {WARM}, ms (min in brackets)")
        for name, rays in ray_sets():
            got = ctx.cast_rays(rays)
            sample = np.unique(np.linspace(0, rays.size - 1, 8).astype(int))
            want = R.cast(tri, rays[sample])
            assert got[sample].tobytes() == want.tobytes(), (name, got[sample], want)
            wide = np.unique(np.linspace(0, rays.size - 1, 256).astype(int))
            tested, entered, tris = R.work(tri, rays[wide])
            hits = int((got["primitive"] != B.ID_NONE).sum())
            t = median_ms(lambda: ctx.cast_rays(rays))
            box_bytes = rays.size * groups * 32
            say(f"  {name:20s} swr_cast_rays {t[0]:9.3f} ({t[1]:.3f})   {hits} of {rays.size} rays hit   per ray (model, index order, {wide.size} rays): "
                f"{tested.mean():.0f} boxes tested, {entered.mean():.1f} groups entered, {tris.mean():.0f} triangles tested   "
                f"{box_bytes / (t[0] * 1e-3) / 1e9:8.1f} GB/s of 32 B per group box")
        item = B.Context.draw_items([(0, 3 * ntri, S.app_transform(0.3))])
        ib = median_ms(lambda: ctx.item_bounds(item))
        say(f"  {'':20s} swr_item_bounds, 1 item over the same stream (one walk of 48 B per triangle) {ib[0]:9.3f} ({ib[1]:.3f})")
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
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--casts-only"], env=env, capture_output=True, text=True,
                                   timeout=280, check=True)
                res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(f"# {os.path.basename(side)}: done", file=sys.stderr, flush=True)
        say("fresh processes alternating (" + ", ".join(os.path.basename(x) for x in sides) + "), median ms per swr_cast_rays call, two rounds:")
        for key in res["this build"][0]:
            say(f"  {key:20s} " + "   ".join(os.path.basename(side) + " " + " ".join("%.3f" % r[key] for r in res[side]) for side in sides))
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
