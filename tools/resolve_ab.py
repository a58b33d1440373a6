#!/usr/bin/env python3
"""Cost of the supersampled resolve, two scenarios: 7680x4320 -> 3840x2160 (S = 2) and 15360x8640 -> 3840x2160
(S = 4), colour + depth (the depth filter is MIN: every sample of both images is read).

On the device, HIP events on one stream, the two alternating, medians of --reps repetitions after a warm-up:
  (a) k_resolve — the library's own launch (swr::launch_resolve of the loaded libswr_hip.so, colour + depth in one launch), over two
      source images filled with a seeded pattern (the kernel's time does not depend on the values);
  (b) hipMemcpyAsync device-to-device of the same source bytes (both images, back to back).
GB/s: (a) bytes read + bytes written, (b) bytes read + bytes written, each over its own time; and the source bytes over the time of both,
which is the like-for-like figure (the resolve writes 1/S^2 of what the copy writes).
Through the library, after one cfg4-shaped frame at the sample resolution, wall clock around the blocking calls (HIP events cannot
bracket a call that waits on the host), alternating, medians of --reps:
  (c) swr_read_color_resolved + swr_read_depth_resolved into page-locked images;
  (d) swr_read_color + swr_read_depth of the full-size images into page-locked images.
Run it under its own time limit: timeout -k 10 600 python3 tools/resolve_ab.py [--reps 50] [--tris 1000000] [--only 2,4]"""
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import swr_amd  # noqa: E402

S = swr_amd.scenes
B = swr_amd.binding
LAUNCH_RESOLVE = "_ZN3swr14launch_resolveEPKvS1_PvS2_iiiiP12ihipStream_t"     # swr::launch_resolve (csrc/swr_internal.h)
D2D, H2D = 3, 1


def hip_runtime():
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    raise SystemExit("libamdhip64.so not found")


def ok(rc, what):
    if rc:
        raise SystemExit(f"{what} failed: hipError {rc}")


def device_side(w, h, factor, reps, warm=5):
    """(a) and (b): medians in ms."""
    hip, L = hip_runtime(), swr_amd.load_library()
    launch = getattr(L, LAUNCH_RESOLVE)
    vp = ctypes.c_void_p
    launch.argtypes = [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    launch.restype = None
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    hip.hipStreamCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipFree.argtypes = [vp]
    hip.hipStreamDestroy.argtypes = [vp]
    hip.hipEventDestroy.argtypes = [vp]
    W, H = w * factor, h * factor
    src_bytes, dst_bytes = W * H * 4, w * h * 4
    bufs = [vp() for _ in range(6)]             # colour, depth sources; their copies; the resolved colour, depth
    for b, n in zip(bufs, (src_bytes, src_bytes, src_bytes, src_bytes, dst_bytes, dst_bytes)):
        ok(hip.hipMalloc(ctypes.byref(b), n), "hipMalloc")
    rng = np.random.default_rng(0x5EED)
    row = rng.integers(0, 1 << 32, W * 64, dtype=np.uint32)             # a 64-row pattern, repeated down the image
    depth_row = rng.uniform(0.0, 1.0, W * 64).astype(np.float32)
    for k in range(0, H, 64):
        n = min(64, H - k) * W * 4
        ok(hip.hipMemcpy(bufs[0].value + k * W * 4, row.ctypes.data, n, H2D), "hipMemcpy")
        ok(hip.hipMemcpy(bufs[1].value + k * W * 4, depth_row.ctypes.data, n, H2D), "hipMemcpy")
    stream, e0, e1 = vp(), vp(), vp()
    ok(hip.hipStreamCreate(ctypes.byref(stream)), "hipStreamCreate")
    ok(hip.hipEventCreate(ctypes.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(ctypes.byref(e1)), "hipEventCreate")

    def timed(fn):
        ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
        fn()
        ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = ctypes.c_float()
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
        return ms.value

    def resolve():
        launch(bufs[0], bufs[1], bufs[4], bufs[5], W, H, factor, B.RESOLVE_DEPTH_MIN, stream)
        ok(hip.hipGetLastError(), "k_resolve")

    def copy():
        ok(hip.hipMemcpyAsync(bufs[2], bufs[0], src_bytes, D2D, stream), "hipMemcpyAsync")
        ok(hip.hipMemcpyAsync(bufs[3], bufs[1], src_bytes, D2D, stream), "hipMemcpyAsync")

    ta, tb = [], []
    for k in range(warm + reps):
        a, b = timed(resolve), timed(copy)
        if k >= warm:
            ta.append(a)
            tb.append(b)
    for b in bufs:
        hip.hipFree(b)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    hip.hipStreamDestroy(stream)
    return ta, tb, 2 * src_bytes, 2 * dst_bytes


def host_visible(w, h, factor, reps, tris, warm=3):
    """(c) and (d): medians in ms, after one cfg4-shaped frame at the sample resolution."""
    W, H = w * factor, h * factor
    s = S.cfg4_soup(ntri=tris, width=W, height=H)
    small = swr_amd.HostImage((h, w, 4), np.uint8), swr_amd.HostImage((h, w), np.float32)
    full = swr_amd.HostImage((H, W, 4), np.uint8), swr_amd.HostImage((H, W), np.float32)
    tc, td = [], []
    try:
        with swr_amd.Context() as ctx:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(W, H)
            ctx.draw(s.transform, B.FLAG_DEPTH_TEST)
            ctx.sync()
            for k in range(warm + reps):
                t0 = time.perf_counter()
                ctx.read_color_resolved(factor, out=small[0])
                ctx.read_depth_resolved(factor, B.RESOLVE_DEPTH_MIN, out=small[1])
                t1 = time.perf_counter()
                ctx.read_color(out=full[0].array)
                ctx.read_depth(out=full[1].array)
                t2 = time.perf_counter()
                if k >= warm:
                    tc.append((t1 - t0) * 1e3)
                    td.append((t2 - t1) * 1e3)
            covered = float((small[0].array[..., 3] > 0).mean())
    finally:
        for x in small + full:
            x.free()
    return tc, td, covered


def main():
    arg = lambda k, d: type(d)(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d     # noqa: E731
    reps, tris, only = arg("--reps", 50), arg("--tris", 1_000_000), arg("--only", "2,4")
    w, h = 3840, 2160
    med = statistics.median
    print(swr_amd.load_library().swr_version().decode())
    for factor in (int(x) for x in only.split(",")):
        name = f"{w * factor}x{h * factor} -> {w}x{h} (S = {factor})"
        ta, tb, src, dst = device_side(w, h, factor, reps)
        a, b = med(ta), med(tb)
        print(f"{name}: (a) k_resolve      median {a:.4f} ms  min {min(ta):.4f}  max {max(ta):.4f}   "
              f"{(src + dst) / a / 1e6:.0f} GB/s read + written, {src / a / 1e6:.0f} GB/s of source", flush=True)
        print(f"{name}: (b) D2D memcpy     median {b:.4f} ms  min {min(tb):.4f}  max {max(tb):.4f}   "
              f"{2 * src / b / 1e6:.0f} GB/s read + written, {src / b / 1e6:.0f} GB/s of source", flush=True)
        print(f"{name}: (a) / (b) = {a / b:.3f}  ({reps} alternating repetitions, HIP events)", flush=True)
        tc, td, covered = host_visible(w, h, factor, reps, tris)
        c, d = med(tc), med(td)
        print(f"{name}: (c) resolved reads median {c:.3f} ms  min {min(tc):.3f}   (d) full-size reads median {d:.3f} ms  min {min(td):.3f}   "
              f"(c) / (d) = {c / d:.3f}  (page-locked destinations, wall clock, {reps} alternating repetitions; {covered:.3f} of the "
              f"resolved pixels covered)", flush=True)


if __name__ == "__main__":
    main()
