"""The boundary of the ray casts (include/swr.h "Ray casts"): the symbol, the layout of swr_ray and swr_ray_hit, the header's normative
sentences that tests/rays_model.py rests on, and the pure helper of the binding.  CPU only; the error codes that need a device are in
tests/test_rays.py."""
import os
import re

import numpy as np

import rays_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
RAY_LAYOUT = [("origin", 0), ("tmin", 12), ("dir", 16), ("tmax", 28)]
HIT_LAYOUT = [("primitive", 0), ("t", 4), ("u", 8), ("v", 12)]


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def test_symbol_and_structs(swr):
    L = swr.load_library()
    B = swr.binding
    assert hasattr(L, "swr_cast_rays") and "swr_cast_rays" in B.ABI_SYMBOLS
    assert B.RAY_DTYPE.itemsize == 32 and B.RAY_HIT_DTYPE.itemsize == 16
    assert [(f, B.RAY_DTYPE.fields[f][1]) for f in B.RAY_DTYPE.names] == RAY_LAYOUT
    assert [(f, B.RAY_HIT_DTYPE.fields[f][1]) for f in B.RAY_HIT_DTYPE.names] == HIT_LAYOUT
    assert B.RAY_DTYPE == M.RAY_DTYPE and B.RAY_HIT_DTYPE == M.HIT_DTYPE
    assert B.RAYS_MAX == M.RAYS_MAX == 1 << 16 and B.ID_NONE == M.ID_NONE
    assert L.swr_abi_version() == 6


def test_header_text():
    h = header()
    assert re.search(r"typedef struct swr_ray \{\s*float origin\[3\];\s*float tmin;\s*float dir\[3\];\s*float tmax;\s*\} swr_ray;", h)
    assert re.search(r"typedef struct swr_ray_hit \{\s*uint32_t primitive;[^}]*float t, u, v;\s*\} swr_ray_hit;", h)
    assert re.search(r"#define SWR_RAYS_MAX \(1 << 16\)", h)
    assert re.search(r"int\s+swr_cast_rays\(swr_context\*\s*\w*,\s*const swr_ray\*\s*\w*,\s*int64_t\s*\w*,\s*uint32_t\s*\w*[^,]*,\s*"
                     r"swr_ray_hit\*\s*\w*\);", h)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    assert h.index("---- Computed normals") < h.index("---- Ray casts") < h.index("---- Load frames")
    for text in ("the presence of the swr_cast_rays symbol is the feature test",
                 "IEEE binary32, one rounding per operation, no FMA; / is correctly rounded",
                 "dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z",
                 "A triangle with a corner coordinate that is not finite is never hit",
                 "Start [nr, fr] = [tmin, tmax]", "r = 1.0f / dir[j]",
                 "If dir[j] == 0.0f or !(fabsf(r) <= FLT_MAX), the axis is parallel",
                 "lo <= origin[j] && origin[j] <= hi",
                 "t0 = (lo - origin[j]) * r;  t1 = (hi - origin[j]) * r;  near = t0 < t1 ? t0 : t1;  far = t0 < t1 ? t1 : t0;",
                 "nr = near > nr ? near : nr;  fr = far < fr ? far : fr",
                 "rejected unless nr <= fr", "r is finite and not zero",
                 "e1 = b - a;  e2 = c - a;  pv = cross(dir, e2);  det = dot(e1, pv).  Reject unless fabsf(det) > 0.0f.",
                 "inv = 1.0f / det;  tv = origin - a;  u = dot(tv, pv) * inv.  Reject unless u >= 0.0f && u <= 1.0f.",
                 "qv = cross(tv, e1);  v = dot(dir, qv) * inv.  Reject unless v >= 0.0f && u + v <= 1.0f.",
                 "t = dot(e2, qv) * inv + 0.0f", "Reject unless t >= tmin && t <= tmax.", "Both facings are hit.",
                 "the smallest t wins; on equal t the smallest p",
                 "A miss is primitive = SWR_ID_NONE,\n *     t = u = v = 0.",
                 "The call changes nothing", "answers\n *     from its first band's copy of the scene",
                 "SWR_ERR_UNSUPPORTED: n > SWR_RAYS_MAX", "the message names the ray's index",
                 "n == 0 succeeds.  A scene without triangles answers every ray with a miss.",
                 "Not covered: any-hit / occlusion-only rays", "watertight edges", "an un-waited call; and the C++ and Swift mirrors"):
        assert text in h, text


def test_pixel_ray_helper(swr):
    B = swr.binding
    ident = np.eye(4, dtype=np.float32).T.reshape(16)
    r = B.pixel_ray(ident, 4, 2, 0, 0)
    assert r.dtype == B.RAY_DTYPE and r.shape == ()
    # the centre of pixel (0, 0) of a 4 x 2 target: NDC (-0.75, 0.5), from depth 0 to depth 1
    assert r["origin"].tolist() == [-0.75, 0.5, 0.0] and r["dir"].tolist() == [0.0, 0.0, 1.0] and (r["tmin"], r["tmax"]) == (0.0, 1.0)
    xs, ys = np.meshgrid(np.arange(4), np.arange(2))
    grid = B.pixel_ray(ident, 4, 2, xs, ys)
    assert grid.shape == (2, 4) and grid["origin"][1, 3].tolist() == [0.75, -0.5, 0.0]
    # through a perspective transform the far point is the un-projected one, and dir is not normalised
    k = 0.25
    m = np.eye(4)
    m[3, 2] = k                                       # w = 1 + k z
    r = B.pixel_ray(m.T.astype(np.float32).reshape(16), 8, 8, 7, 0)
    nx, ny = 0.875, 0.875
    # depth 1: z / (1 + k z) = 1 -> z = 1 / (1 - k), x = nx (1 + k z)
    z1 = 1.0 / (1.0 - k)
    far = np.array([nx * (1 + k * z1), ny * (1 + k * z1), z1])
    assert np.allclose(r["origin"], [nx, ny, 0.0], rtol=0, atol=1e-7) and np.allclose(r["origin"] + r["dir"], far, rtol=1e-6)
    assert abs(np.linalg.norm(r["dir"]) - 1.0) > 0.1
    # a projection without a far plane (w = z + 1, depth = z / (z + 1): depth 1 at infinity): the direction, and the largest tmax;
    # the point of depth d is origin + d / (1 - d) * dir
    m = np.eye(4)
    m[3, 2] = 1.0
    r = B.pixel_ray(m.T.astype(np.float32).reshape(16), 8, 8, 7, 0)
    assert r["tmin"] == 0.0 and r["tmax"] == np.finfo(np.float32).max and np.isfinite(r["dir"]).all()
    p = r["origin"].astype(np.float64) + (0.25 / 0.75) * r["dir"].astype(np.float64)
    assert np.allclose([p[0] / (p[2] + 1), p[1] / (p[2] + 1), p[2] / (p[2] + 1)], [0.875, 0.875, 0.25], rtol=1e-6)


def test_null_context_is_refused(swr):
    L = swr.load_library()
    rays = np.zeros(2, dtype=swr.binding.RAY_DTYPE)
    rays["dir"] = (0, 0, 1)
    out = np.full(2 * 4, 0xA5A5A5A5, dtype=np.uint32)
    assert L.swr_cast_rays(None, rays.ctypes.data, 2, 0, out.ctypes.data) == BAD_ARG
    assert L.swr_cast_rays(None, None, 0, 0, None) == BAD_ARG
    assert (out == 0xA5A5A5A5).all()
