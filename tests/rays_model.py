"""The numpy model of include/swr.h "Ray casts", written from the header's text: IEEE binary32, one rounding per operation, no FMA (numpy
float32 arithmetic never fuses), brute force over every triangle: the skip, the box pre-test, Moeller-Trumbore, the winner.  Nothing
here looks at the library.  A plain helper module of tests/test_rays_model.py and tests/test_rays.py; not a test file."""
import numpy as np

F = np.float32
ID_NONE = 0xFFFFFFFF        # SWR_ID_NONE
RAYS_MAX = 1 << 16          # SWR_RAYS_MAX
FLT_MAX = np.finfo(np.float32).max

# swr_ray, 32 bytes, and swr_ray_hit, 16 bytes
RAY_DTYPE = np.dtype([("origin", np.float32, (3,)), ("tmin", np.float32), ("dir", np.float32, (3,)), ("tmax", np.float32)])
HIT_DTYPE = np.dtype([("primitive", np.uint32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])


def ray(origin, direction, tmin=0.0, tmax=np.inf):
    """One RAY_DTYPE record (tmax defaults to the largest finite float: the call refuses an infinite one)."""
    r = np.zeros((), dtype=RAY_DTYPE)
    r["origin"], r["dir"], r["tmin"] = origin, direction, tmin
    r["tmax"] = FLT_MAX if np.isinf(tmax) else tmax
    return r


def rays(rows):
    """A RAY_DTYPE array from RAY_DTYPE records or (origin, dir[, tmin[, tmax]]) tuples."""
    out = np.zeros(len(rows), dtype=RAY_DTYPE)
    for k, r in enumerate(rows):
        out[k] = r if isinstance(r, np.ndarray) else ray(*r)
    return out


def triangles(vertices, indices):
    """(ntri, 3, 3) float32 corners a, b, c of the triangles indices[3p .. 3p + 2]; trailing indices are ignored."""
    v = np.asarray(vertices, dtype=np.float32)
    v = v.reshape(-1, v.shape[-1])[:, 0:3]
    idx = np.asarray(indices, dtype=np.int64)
    idx = idx[:idx.size // 3 * 3].reshape(-1, 3)
    return np.ascontiguousarray(v[idx])


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pretest(r, lo, hi):
    """Step 2 on the boxes [lo, hi] (..., 3) for one ray record: whether each box passes."""
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    o, d = r["origin"].astype(np.float32), r["dir"].astype(np.float32)
    nr = np.full(lo.shape[:-1], r["tmin"], dtype=np.float32)
    fr = np.full(lo.shape[:-1], r["tmax"], dtype=np.float32)
    ok = np.ones(lo.shape[:-1], dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(3):
            inv = F(1.0) / d[j]
            if d[j] == F(0.0) or not (np.abs(inv) <= FLT_MAX):
                ok &= (lo[..., j] <= o[j]) & (o[j] <= hi[..., j])
                continue
            t0 = (lo[..., j] - o[j]) * inv
            t1 = (hi[..., j] - o[j]) * inv
            near = np.where(t0 < t1, t0, t1)
            far = np.where(t0 < t1, t1, t0)
            nr = np.where(near > nr, near, nr)
            fr = np.where(far < fr, far, fr)
            assert nr.dtype == np.float32 and fr.dtype == np.float32
        return ok & (nr <= fr)


def candidates(tri, r):
    """Steps 1-3 for one ray over tri (n, 3, 3): (accepted, t, u, v), each of length n."""
    tri = np.asarray(tri, dtype=np.float32)
    o, d = r["origin"].astype(np.float32), r["dir"].astype(np.float32)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(tri).all(axis=(1, 2))
        box = pretest(r, tri.min(axis=1), tri.max(axis=1))
        e1, e2 = b - a, c - a
        pv = cross(d[None, :], e2)
        det = dot(e1, pv)
        inv = F(1.0) / det
        tv = o[None, :] - a
        u = dot(tv, pv) * inv
        qv = cross(tv, e1)
        v = dot(d[None, :], qv) * inv
        t = dot(e2, qv) * inv + F(0.0)
        assert all(x.dtype == np.float32 for x in (det, inv, u, v, t))
        ok = finite & box & (np.abs(det) > F(0.0)) & (u >= F(0.0)) & (u <= F(1.0)) & (v >= F(0.0)) & (u + v <= F(1.0))
        ok &= (t >= r["tmin"]) & (t <= r["tmax"])
    return ok, t, u, v


def cast(tri, ray_array):
    """swr_cast_rays by brute force: a HIT_DTYPE array, hits[k] the winner of ray_array[k] over tri (n, 3, 3) (step 4)."""
    tri = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    ray_array = np.asarray(ray_array, dtype=RAY_DTYPE).reshape(-1)
    out = np.zeros(ray_array.size, dtype=HIT_DTYPE)
    out["primitive"] = ID_NONE
    if tri.shape[0] == 0:
        return out
    for k, r in enumerate(ray_array):
        ok, t, u, v = candidates(tri, r)
        if not ok.any():
            continue
        p = np.flatnonzero(ok)
        p = p[t[p] == t[p].min()][0]        # the smallest t; on equal t the smallest p (+0 == -0, and t carries no -0)
        out[k] = (p, t[p], u[p], v[p])
    return out


def check_ray(r):
    """What SWR_ERR_BAD_ARG refuses in one ray: the reason, or None."""
    f = np.concatenate([r["origin"], [r["tmin"]], r["dir"], [r["tmax"]]])
    if not np.isfinite(f).all():
        return "not finite"
    if (r["dir"] == 0).all():
        return "zero direction"
    if r["tmin"] > r["tmax"]:
        return "tmin > tmax"
    return None


def work(tri_stream, ray_array):
    """Per-ray work of the group cull over a stream (n, 3, 3) in slot order: (group boxes tested, groups entered, triangles tested),
    each an array per ray.  A group with a corner that is not finite is always entered."""
    tri = np.asarray(tri_stream, dtype=np.float32).reshape(-1, 3, 3)
    n = tri.shape[0]
    groups = (n + 63) // 64
    pad = np.concatenate([tri, np.repeat(tri[-1:], groups * 64 - n, axis=0)]).reshape(groups, 192, 3)
    lo, hi = pad.min(axis=1), pad.max(axis=1)
    bad = ~np.isfinite(pad).all(axis=(1, 2))
    last = n - (groups - 1) * 64
    tested, entered, tris = [], [], []
    for r in np.asarray(ray_array, dtype=RAY_DTYPE).reshape(-1):
        with np.errstate(all="ignore"):
            e = bad | pretest(r, lo, hi)
        tested.append(groups)
        entered.append(int(e.sum()))
        tris.append(int(e[:-1].sum()) * 64 + (last if e[-1] else 0))
    return np.array(tested), np.array(entered), np.array(tris)
