"""The numpy model of include/swr.h "Item bounds", written from the header's text: per corner IEEE binary32, one rounding per operation,
no FMA (numpy float32 arithmetic never fuses), then the drawable rule, the truncated rectangle, the folded depth range and the three
counts.  Nothing here looks at the library."""
import numpy as np

FLAG_METAL_RULES = 4        # SWR_FLAG_METAL_RULES
LIMIT = np.float32(2.0 ** 30)

# swr_item_bound, 48 bytes
DTYPE = np.dtype([("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32), ("zmin", np.float32), ("zmax", np.float32),
                  ("drawable", np.uint32), ("skipped", np.uint32), ("behind", np.uint32), ("reserved", np.uint32, (3,))])


def roundf(x):
    """round half away from zero: copysign(floor(|x| + 0.5), x) in float64, exact for float32 inputs."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    return np.copysign(np.floor(np.abs(x64) + 0.5), x64).astype(np.float32)


def corners(xyz, transform, width, height, metal):
    """(sx, sy, sz, w) of every position of xyz (..., 3): r = c0*x; r += c1*y; r += c2*z; r += c3*1; ndc = r.xyz / r.w; the screen map."""
    xyz = np.asarray(xyz, dtype=np.float32)
    c = np.asarray(transform, dtype=np.float32).reshape(4, 4)            # [column][row]
    x, y, z = xyz[..., 0:1], xyz[..., 1:2], xyz[..., 2:3]
    one, half = np.float32(1.0), np.float32(0.5)
    with np.errstate(all="ignore"):
        r = c[0] * x
        r = r + c[1] * y
        r = r + c[2] * z
        r = r + c[3] * one
        w = r[..., 3]
        nx, ny, nz = r[..., 0] / w, r[..., 1] / w, r[..., 2] / w
        sx = (nx * half + half) * np.float32(width)
        sy = (ny * np.float32(-0.5) + half) * np.float32(height)
    if metal:
        sx, sy = roundf(sx), roundf(sy)
    assert sx.dtype == np.float32 and sy.dtype == np.float32 and nz.dtype == np.float32
    return sx, sy, nz, w


def item_bound(vertices, indices, first_index, index_count, transform, width, height, flags=0):
    """The record of one item over the triangles indices[first_index, first_index + index_count) of an (n, 8) or (n, 3+) vertex array."""
    metal = bool(flags & FLAG_METAL_RULES)
    v = np.asarray(vertices, dtype=np.float32)
    v = v.reshape(-1, v.shape[-1])[:, 0:3]
    idx = np.asarray(indices, dtype=np.int64)[first_index:first_index + index_count].reshape(-1, 3)
    out = np.zeros((), dtype=DTYPE)
    out["zmin"], out["zmax"] = np.inf, -np.inf
    if idx.shape[0] == 0:
        return out
    sx, sy, sz, w = corners(v[idx], transform, width, height, metal)     # (T, 3) each
    with np.errstate(all="ignore"):
        ok = (np.abs(sx) < LIMIT) & (np.abs(sy) < LIMIT)
        if metal:
            ok &= (sx >= 0) & (sy >= 0)
    drawable = ok.all(axis=1)
    out["drawable"] = int(drawable.sum())
    out["skipped"] = int((~drawable).sum())
    with np.errstate(all="ignore"):
        out["behind"] = int((drawable & ~(w > 0).all(axis=1)).sum())
    if not drawable.any():
        return out
    ix = np.trunc(sx[drawable].astype(np.float64)).astype(np.int64)
    iy = np.trunc(sy[drawable].astype(np.float64)).astype(np.int64)
    out["x0"] = min(max(int(ix.min()), 0), width)
    out["x1"] = min(max(int(ix.max()) + 1, 0), width)
    out["y0"] = min(max(int(iy.min()), 0), height)
    out["y1"] = min(max(int(iy.max()) + 1, 0), height)
    zmin, zmax = np.float32(np.inf), np.float32(-np.inf)
    for s in sz[drawable].reshape(-1):                                   # s < m ? s : m skips a NaN by itself
        zmin = s if s < zmin else zmin
        zmax = s if s > zmax else zmax
    out["zmin"] = zmin + np.float32(0.0)
    out["zmax"] = zmax + np.float32(0.0)
    return out


def item_bounds(vertices, indices, items, width, height, flags=0):
    """The records of a list of (first_index, index_count, transform) items."""
    out = np.zeros(len(items), dtype=DTYPE)
    for k, (first, count, transform) in enumerate(items):
        out[k] = item_bound(vertices, indices, int(first), int(count), transform, width, height, flags)
    return out


def same(a, b):
    """Bit for bit: the two record arrays as bytes."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize == 48 and a.tobytes() == b.tobytes()
