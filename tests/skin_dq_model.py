"""The numpy model of include/swr.h "Dual-quaternion skinning": the posed vertices and normals, operation for operation — IEEE
binary32, one rounding each, no FMA (numpy float32 arithmetic never fuses; its float32 sqrt and divide are correctly rounded) — and
the scene the tests share: the torus, the skin and the 320 x 192 target of tests/skin_model.py under a twisting pose."""
import math

import numpy as np

import skin_model as SM

W, H = SM.W, SM.H
F = np.float32


def _cross(a, b):
    """(a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x): two products, one subtraction."""
    ax, ay, az = a
    bx, by, bz = b
    return (ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx)


def _blend(joint, weight, dq):
    """C: the eight components of the normalised blend, each an (n,) float32 array."""
    q = np.asarray(dq, dtype=np.float32).reshape(-1, 8)
    Q = [q[joint[:, k]] for k in range(4)]                          # [k][n][8]
    u = [weight[:, 0]]
    for k in (1, 2, 3):
        s = Q[0][:, 0] * Q[k][:, 0] + Q[0][:, 1] * Q[k][:, 1]
        s = s + Q[0][:, 2] * Q[k][:, 2]
        s = s + Q[0][:, 3] * Q[k][:, 3]
        u.append(np.where(s < F(0.0), -weight[:, k], weight[:, k]))
    B = []
    for c in range(8):
        b = u[0] * Q[0][:, c]
        for k in (1, 2, 3):
            b = b + u[k] * Q[k][:, c]
        B.append(b)
    n = B[0] * B[0] + B[1] * B[1]
    n = n + B[2] * B[2]
    n = n + B[3] * B[3]
    l = np.sqrt(n)
    i = F(1.0) / l
    C = [b * i for b in B]
    assert all(c.dtype == np.float32 for c in C)
    return C


def _rotate(C, x):
    q, w = (C[0], C[1], C[2]), C[3]
    a = _cross(q, x)
    b = tuple(a[j] + w * x[j] for j in range(3))
    c = _cross(q, b)
    return tuple(x[j] + F(2.0) * c[j] for j in range(3))


def _translation(C):
    q, w, d, dw = (C[0], C[1], C[2]), C[3], (C[4], C[5], C[6]), C[7]
    e = _cross(q, d)
    return tuple(F(2.0) * ((w * d[j] - dw * q[j]) + e[j]) for j in range(3))


def _args(joint, weight):
    return np.asarray(joint).reshape(-1, 4).astype(np.int64), np.asarray(weight, dtype=np.float32).reshape(-1, 4)


def pose_vertices(vertices, joint, weight, dq):
    """The posed copy of an (n, 8) vertex array: positions rot(v) + t, colours and padding lanes as they are."""
    v = np.array(vertices, dtype=np.float32, copy=True).reshape(-1, 8)
    joint, weight = _args(joint, weight)
    with np.errstate(all="ignore"):
        C = _blend(joint, weight, dq)
        r = _rotate(C, (v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()))
        t = _translation(C)
        for j in range(3):
            v[:, j] = r[j] + t[j]
    return v


def pose_attrs(attrs, joint, weight, dq):
    """The posed copy of an (n, 8) attribute array: normals rot(n), uv as it is."""
    a = np.array(attrs, dtype=np.float32, copy=True).reshape(-1, 8)
    joint, weight = _args(joint, weight)
    with np.errstate(all="ignore"):
        r = _rotate(_blend(joint, weight, dq), (a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()))
        for j in range(3):
            a[:, j] = r[j]
    return a


# ---- joints ------------------------------------------------------------------------------------------------------------------------
def rigid_matrix(axis, angle, t=(0.0, 0.0, 0.0)):
    """The 4 x 4 mathematical matrix (float64) of a turn by `angle` about the unit vector `axis`, then the translation t."""
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    c, s = math.cos(angle), math.sin(angle)
    k = 1 - c
    M = np.eye(4)
    M[:3, :3] = [[c + x * x * k, x * y * k - z * s, x * z * k + y * s],
                 [y * x * k + z * s, c + y * y * k, y * z * k - x * s],
                 [z * x * k - y * s, z * y * k + x * s, c + z * z * k]]
    M[:3, 3] = t
    return M


def dq_joint(axis, angle, t=(0.0, 0.0, 0.0)):
    """The same rigid motion as eight floats, computed in float64 and rounded once (no w >= 0 convention: the half angle decides)."""
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    s, w = math.sin(angle / 2), math.cos(angle / 2)
    q = np.array([x * s, y * s, z * s, w])
    tx, ty, tz = t
    d = 0.5 * np.array([tx * w + ty * q[2] - tz * q[1], -tx * q[2] + ty * w + tz * q[0], tx * q[1] - ty * q[0] + tz * w,
                        -(tx * q[0] + ty * q[1] + tz * q[2])])
    return np.concatenate([q, d]).astype(np.float32)


def column_major(M):
    """(J, 4, 4) mathematical matrices as swr_pose_set takes them: J x 16 floats, column-major."""
    return np.ascontiguousarray(np.asarray(M, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1).reshape(-1, 16), dtype=np.float32)


def matrices_of(dq):
    """The rigid motions of (J, 8) dual quaternions as swr_pose_set takes them (float64, rounded once; q and -q give the same matrix)."""
    out = []
    for q in np.asarray(dq, dtype=np.float64).reshape(-1, 8):
        l = np.linalg.norm(q[0:4])
        x, y, z, s = q[0:4] / l
        r, d, ds = np.array([x, y, z]), q[4:7] / l, q[7] / l
        M = np.eye(4)
        M[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s)],
                     [2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s)],
                     [2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)]]
        M[:3, 3] = 2.0 * ((s * d - ds * r) + np.cross(r, d))
        out.append(M)
    return column_major(out)


IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 0], dtype=np.float32)
TWIST, TWIST_T = 2.5, (0.04, -0.03, 0.0)


def twist_pose(angle=TWIST, t=TWIST_T):
    """Four joints: identity; a twist of `angle` rad about x with a small translation; 2 and 3 (weight 0 in bend_skin, as FAR is in
    tests/skin_model.py) are the negations of 1 and 0: the same motions, the other sign."""
    j1 = dq_joint((1, 0, 0), angle, t)
    return np.stack([IDENTITY, j1, -j1, -IDENTITY])


def twist_matrices(angle=TWIST, t=TWIST_T):
    """The same two motions (and two far joints of weight 0) as the matrices swr_pose_set blends linearly."""
    far = SM.bend_pose()[2:]
    return np.concatenate([column_major([np.eye(4), rigid_matrix((1, 0, 0), angle, t)]), far])


def lift_pose(dy, angle=0.0):
    """One rigid joint that shrinks nothing (a dual quaternion cannot): a turn about z and a shift along y."""
    return dq_joint((0, 0, 1), angle, (0.0, dy, 0.0))[None]


UP = lift_pose(1.3, 0.2)        # rows 0-43 of 192: band 0 of three 64-row bands (the rest of the torus is above the target)
DOWN = lift_pose(-1.3, -0.3)    # rows 148-191: band 2
