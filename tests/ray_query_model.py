"""The numpy model of include/swr.h "Ray queries", written from the header's text on top of tests/rays_model.py: the candidates of steps
1 to 3, masked by the range of primitives and by the facing that the det of step 3 gives, then either the winner of step 4 or one bit
per ray.  Nothing here looks at the library.  A plain helper module of tests/test_ray_query_model.py and tests/test_ray_queries.py; not
a test file."""
import numpy as np

import rays_model as R

F = np.float32
ANY_HIT, CULL_BACK, CULL_FRONT, FRONT_CW = 1, 2, 4, 8       # SWR_RAYS_*
KNOWN = ANY_HIT | CULL_BACK | CULL_FRONT | FRONT_CW
OCCLUDED = 0xFFFFFFFE                                       # SWR_RAY_OCCLUDED
ID_NONE = R.ID_NONE
CULLS = [0, CULL_BACK, CULL_FRONT, FRONT_CW, FRONT_CW | CULL_BACK, FRONT_CW | CULL_FRONT]      # every combination except "both"
BOTH = CULL_BACK | CULL_FRONT

# swr_ray_query, 24 bytes
QUERY_DTYPE = np.dtype([("flags", np.uint32), ("reserved", np.uint32), ("first_primitive", np.int64), ("primitive_count", np.int64)])


def det_of(tri, r):
    """det of step 3 for one ray over tri (n, 3, 3): dot(e1, cross(dir, e2)), with the dot and cross of "Ray casts"."""
    tri = np.asarray(tri, dtype=np.float32)
    d = r["dir"].astype(np.float32)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    with np.errstate(all="ignore"):
        det = R.dot(b - a, R.cross(d[None, :], c - a))
    assert det.dtype == np.float32
    return det


def resolve(ntri, first=0, count=-1):
    """[begin, end) of a legal range over ntri primitives."""
    assert first >= 0 and count >= -1 and first <= ntri and (count < 0 or first + count <= ntri)
    return first, ntri if count < 0 else first + count


def steps(tri, ray_array):
    """Per ray (accepted, t, u, v, det) of steps 1 to 3 over tri: what every query of the same rays on the same triangles starts from
    (query(..., steps=...) then only masks and picks; nothing of a query is in here)."""
    tri = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    return [R.candidates(tri, r) + (det_of(tri, r),) for r in np.asarray(ray_array, dtype=R.RAY_DTYPE).reshape(-1)]


def survivors(tri, r, flags=0, first=0, count=-1, step=None):
    """(kept, t, u, v) for one ray: the candidates of steps 1 to 3 that the range and the cull leave."""
    tri = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    ok, t, u, v, det = step if step is not None else R.candidates(tri, r) + (det_of(tri, r),)
    begin, end = resolve(tri.shape[0], first, count)
    p = np.arange(tri.shape[0])
    with np.errstate(all="ignore"):
        front = (det < F(0.0)) if flags & FRONT_CW else (det > F(0.0))
    keep = (p >= begin) & (p < end)
    if flags & CULL_BACK:
        keep &= front
    if flags & CULL_FRONT:
        keep &= ~front
    return ok & keep, t, u, v


def query(tri, ray_array, flags=0, first=0, count=-1, steps=None):
    """swr_query_rays by brute force: a rays_model.HIT_DTYPE array.  steps: steps(tri, ray_array), when the caller keeps it."""
    assert flags & ~KNOWN == 0
    tri = np.asarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    ray_array = np.asarray(ray_array, dtype=R.RAY_DTYPE).reshape(-1)
    out = np.zeros(ray_array.size, dtype=R.HIT_DTYPE)
    out["primitive"] = ID_NONE
    if tri.shape[0] == 0:
        assert (first, count) in ((0, -1), (0, 0))
        return out
    for k, r in enumerate(ray_array):
        ok, t, u, v = survivors(tri, r, flags, first, count, None if steps is None else steps[k])
        if not ok.any():
            continue
        if flags & ANY_HIT:
            out[k] = (OCCLUDED, 0.0, 0.0, 0.0)
            continue
        p = np.flatnonzero(ok)
        p = p[t[p] == t[p].min()][0]        # step 4: the smallest t; on equal t the smallest p
        out[k] = (p, t[p], u[p], v[p])
    return out


def occluded(hits):
    return np.asarray(hits)["primitive"] != ID_NONE


def check_query(ntri, flags=0, reserved=0, first=0, count=-1):
    """What SWR_ERR_BAD_ARG refuses in a query over ntri primitives: the reason, or None."""
    if flags & ~KNOWN:
        return "unknown flags"
    if reserved:
        return "reserved"
    if first < 0:
        return "first_primitive"
    if count < -1:
        return "primitive_count"
    if first > ntri or (count >= 0 and first + count > ntri):
        return "beyond the scene"
    return None
