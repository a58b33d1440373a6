"""The numpy model of include/swr.h "Computed normals": the face vectors, the smooth vertex normals and the flat, de-indexed scene,
operation for operation — IEEE binary32, one rounding each, no FMA (numpy float32 arithmetic never fuses) — and the two scenes the
tests share.  The sums of SWR_NORMALS_SMOOTH are taken in rounds over the sorted adjacency: round r adds, to every vertex that has
one, the face of its r-th corner in ascending corner order, so every vertex sees its faces in the header's order.  It composes with
tests/morph_model.py, tests/morph_sparse_model.py, tests/skin_model.py and tests/skin_dq_model.py: morph, then skin, then normals."""
import numpy as np

import morph_model as MM
import morph_sparse_model as MS
import skin_model as SM

W, H = SM.W, SM.H
UPLOADED, SMOOTH, FLAT = 0, 1, 2        # SWR_NORMALS_*
FLIP = 1                                # SWR_NORMALS_FLIP


def _xyz(vertices):
    return np.asarray(vertices, dtype=np.float32).reshape(-1, 8)[:, 0:3]


def _tris(indices):
    i = np.asarray(indices, dtype=np.int64).reshape(-1)
    return i[: i.size // 3 * 3].reshape(-1, 3)          # trailing indices are ignored


def cross(a, b):
    """"Dual-quaternion skinning": two products and one subtraction per component."""
    with np.errstate(all="ignore"):
        x = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        y = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        z = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    r = np.stack([x, y, z], axis=-1)
    assert r.dtype == np.float32
    return r


def face_vectors(vertices, indices, flip=False):
    """(ntri, 3): f_p = cross(b - a, c - a), or, flip, cross(c - a, b - a)."""
    p, t = _xyz(vertices), _tris(indices)
    with np.errstate(all="ignore"):
        e1, e2 = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    return cross(e2, e1) if flip else cross(e1, e2)


def adjacency(indices, nv):
    """(off[nv + 1], tri[3 * ntri]): row i = the triangle of every corner that names vertex i, ascending by corner number 3p + k,
    duplicates kept."""
    c = _tris(indices).reshape(-1)
    order = np.argsort(c, kind="stable")
    off = np.zeros(nv + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(c, minlength=nv))
    return off, order // 3


def vertex_normals(vertices, indices, flip=False):
    """(nv, 3): the n_i of SWR_NORMALS_SMOOTH."""
    nv = _xyz(vertices).shape[0]
    f = face_vectors(vertices, indices, flip)
    off, tri = adjacency(indices, nv)
    count = np.diff(off)
    n = np.zeros((nv, 3), dtype=np.float32)             # (+0, +0, +0)
    with np.errstate(all="ignore"):
        for r in range(int(count.max()) if nv else 0):
            sel = np.flatnonzero(count > r)
            n[sel] = n[sel] + f[tri[off[sel] + r]]
        l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = l > np.float32(0.0)                        # (false for 0 and for NaN: n stays as it is)
        inv = np.float32(1.0) / l[ok]
        n[ok] = n[ok] * inv[:, None]
    assert n.dtype == np.float32 and l.dtype == np.float32
    return n


def smooth_attrs(attrs, vertices, indices, flip=False):
    """The attribute array a context uploads to show the SMOOTH scene: the same uv (and padding lanes) with the n_i."""
    a = np.array(attrs, dtype=np.float32, copy=True).reshape(-1, 8)
    a[:, 0:3] = vertex_normals(vertices, indices, flip)
    return a


def flat_scene(vertices, attrs, indices, flip=False):
    """(vertices, attrs, indices) of the de-indexed scene: vertex 3p + k is corner k of triangle p with the normal f_p."""
    c = _tris(indices).reshape(-1)
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 8)[c])
    a = np.ascontiguousarray(np.asarray(attrs, dtype=np.float32).reshape(-1, 8)[c])
    a[:, 0:3] = np.repeat(face_vectors(vertices, indices, flip), 3, axis=0)
    return v, a, np.arange(c.size, dtype=np.int64)


def expected_scene(mode, vertices, attrs, indices, flip=False):
    """(vertices, attrs, indices) a second context uploads to show what `mode` shows of the (deformed) vertices."""
    if mode == SMOOTH:
        return np.asarray(vertices, dtype=np.float32), smooth_attrs(attrs, vertices, indices, flip), np.asarray(indices, dtype=np.int64)
    if mode == FLAT:
        return flat_scene(vertices, attrs, indices, flip)
    return np.asarray(vertices, dtype=np.float32), np.asarray(attrs, dtype=np.float32), np.asarray(indices, dtype=np.int64)


# ---- scene 1: the torus of tests/morph_model.py with the bend skin and the sparse rig -----------------------------------------------
def torus(S):
    """(vertices, indices): 768 vertices, 1536 triangles, every vertex in six triangles."""
    return MM.torus(S)


def torus_uploaded_attrs(S):
    """The torus's own normals and uv: what a caller uploads."""
    return S.torus_attrs(48, 16)


def torus_skin(vertices):
    return SM.bend_skin(vertices)


def torus_rig(S, vertices, normals=False):
    return MS.rig(S, vertices, normals)


# ---- scene 2: a hub ------------------------------------------------------------------------------------------------------------------
HUB, RING = 0, 300                      # the hub vertex, the triangles (and ring vertices) around it
HUB_NV, HUB_NTRI = 312, 304             # 256 + 56 vertices, 256 + 48 triangles: two workgroups, the second partly filled
LONE, UNUSED, TWICE, NAN_TRI, NEIGHBOUR = 301, 304, 305, 307, 310      # first vertex of each extra part
NAN_VERTEX, SHARED = 307, 308


def hub(S):
    """(vertices, indices).  Vertex 0 is shared by 300 triangles (0, 1 + j, 1 + (j + 1) % 300) over a wavy ring: a row longer than
    a wave and longer than a workgroup, next to the ring's rows of 2.  Then: a lone triangle (rows of 1); a vertex no triangle
    references; a triangle that names vertex 305 twice (a row of 2 with the same triangle twice, next to a row of 1); a triangle with
    a NaN corner (its three vertices get NaN normals); and a finite triangle that shares vertex 308 with it (308 stays NaN, its other
    two vertices stay finite)."""
    j = np.arange(RING, dtype=np.float64)
    t = j / RING * 2 * np.pi
    ring = np.stack([0.55 * np.cos(t), 0.8 * np.sin(t), 0.5 + 0.12 * np.sin(5 * t)], axis=-1)
    xyz = np.zeros((HUB_NV, 3), dtype=np.float32)
    xyz[HUB] = (0.0, 0.0, 0.3)
    xyz[1:1 + RING] = ring.astype(np.float32)
    xyz[LONE:LONE + 3] = [[-0.95, 0.7, 0.2], [-0.7, 0.95, 0.25], [-0.95, 0.95, 0.4]]
    xyz[UNUSED] = (0.9, 0.9, 0.1)
    xyz[TWICE:TWICE + 2] = [[0.7, -0.9, 0.2], [0.9, -0.7, 0.2]]
    xyz[NAN_TRI:NAN_TRI + 3] = [[np.nan, -0.9, 0.2], [-0.8, -0.95, 0.2], [-0.6, -0.9, 0.25]]
    xyz[NEIGHBOUR:NEIGHBOUR + 2] = [[-0.95, -0.7, 0.3], [-0.7, -0.7, 0.15]]
    rgb = (0.35 + 0.65 * np.abs(np.sin(np.arange(HUB_NV)[:, None] * np.array([0.37, 0.61, 0.83])))).astype(np.float32)
    fan = np.stack([np.zeros(RING, dtype=np.int64), 1 + np.arange(RING), 1 + (np.arange(RING) + 1) % RING], axis=-1)
    extra = np.array([[LONE, LONE + 1, LONE + 2], [TWICE, TWICE, TWICE + 1], [NAN_VERTEX, SHARED, NAN_TRI + 2],
                      [SHARED, NEIGHBOUR, NEIGHBOUR + 1]], dtype=np.int64)
    idx = np.concatenate([fan, extra]).reshape(-1)
    assert idx.size == 3 * HUB_NTRI and HUB_NV % 64 and HUB_NV > 256
    return S.pack_vertices(xyz, rgb), idx


def hub_attrs(S, seed=0x4B):
    """Attributes for the hub: uploaded normals that are nothing like the computed ones, uv for the textured shader."""
    return S.random_shading(HUB_NV, seed).attrs
