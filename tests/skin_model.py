"""The numpy model of include/swr.h "Skinned meshes": the posed vertices and normals, operation for operation — IEEE binary32, one
rounding each, no FMA (numpy float32 arithmetic never fuses) — and the scene the tests share."""
import math

import numpy as np

SKIN_MAX_JOINTS = 1024
W, H = 320, 192


def joint_matrix(angle=0.0, scale=1.0, tx=0.0, ty=0.0, tz=0.0):
    """An affine joint — a turn about z, a uniform scale, a translation — as 16 floats, column-major."""
    c, s = math.cos(angle) * scale, math.sin(angle) * scale
    return np.array([c, s, 0, 0, -s, c, 0, 0, 0, 0, scale, 0, tx, ty, tz, 1], dtype=np.float32)


def _blend(xyz, joint, weight, joints, translate):
    """acc = w0 r0; acc += w1 r1; acc += w2 r2; acc += w3 r3, with r_k = c0 x; += c1 y; += c2 z; (+= c3 * 1)."""
    m = np.asarray(joints, dtype=np.float32).reshape(-1, 4, 4)          # [j][column][row]
    x, y, z = xyz[:, 0:1], xyz[:, 1:2], xyz[:, 2:3]
    acc = None
    with np.errstate(all="ignore"):
        for k in range(4):
            c = m[joint[:, k]]                                          # [n][column][row]
            r = c[:, 0, 0:3] * x
            r = r + c[:, 1, 0:3] * y
            r = r + c[:, 2, 0:3] * z
            if translate:
                r = r + c[:, 3, 0:3] * np.float32(1.0)
            t = weight[:, k:k + 1] * r
            acc = t if acc is None else acc + t
    assert acc.dtype == np.float32
    return acc


def pose_vertices(vertices, joint, weight, joints):
    """The posed copy of an (n, 8) vertex array: positions blended, colours and padding lanes as they are."""
    v = np.array(vertices, dtype=np.float32, copy=True).reshape(-1, 8)
    joint = np.asarray(joint).reshape(-1, 4).astype(np.int64)
    weight = np.asarray(weight, dtype=np.float32).reshape(-1, 4)
    v[:, 0:3] = _blend(v[:, 0:3].copy(), joint, weight, joints, True)
    return v


def pose_attrs(attrs, joint, weight, joints):
    """The posed copy of an (n, 8) attribute array: normals blended without the translation column, uv as it is."""
    a = np.array(attrs, dtype=np.float32, copy=True).reshape(-1, 8)
    joint = np.asarray(joint).reshape(-1, 4).astype(np.int64)
    weight = np.asarray(weight, dtype=np.float32).reshape(-1, 4)
    a[:, 0:3] = _blend(a[:, 0:3].copy(), joint, weight, joints, False)
    return a


# ---- the shared scene: a torus bending between two joints --------------------------------------------------------------------------
def torus(S):
    """(vertices, indices): torus_mesh(48, 16, 0.55, 0.2) — 768 vertices, 1536 triangles, 24 groups of 64."""
    xyz, rgb, idx = S.torus_mesh(48, 16, 0.55, 0.2)
    return S.pack_vertices(xyz, rgb), idx


def bend_skin(vertices):
    """(joint, weight): weights (1 - t, t, 0, 0) with t = clip(x / 1.1 + 0.5, 0, 1) on joints (0, 1, 2, 3); joints 2 and 3 weigh 0."""
    x = np.asarray(vertices, dtype=np.float32).reshape(-1, 8)[:, 0]
    t = np.clip(x / np.float32(1.1) + np.float32(0.5), np.float32(0), np.float32(1)).astype(np.float32)
    n = x.shape[0]
    joint = np.tile(np.array([0, 1, 2, 3], dtype=np.uint32), (n, 1))
    weight = np.zeros((n, 4), dtype=np.float32)
    weight[:, 0] = np.float32(1) - t
    weight[:, 1] = t
    return joint, weight


FAR = (40.0, -30.0, 5.0)


def bend_pose(a0=0.5, a1=-0.6, dy=0.1):
    """Four joints: 0 and 1 bend the torus, 2 and 3 (weight 0) lie far away."""
    return np.stack([joint_matrix(a0, 0.9, -0.05, dy), joint_matrix(a1, 1.05, 0.08, -dy),
                     joint_matrix(1.0, 3.0, *FAR), joint_matrix(-2.0, 0.5, -FAR[0], FAR[1], FAR[2])])


def rigid_skin(n, joint=0):
    """Every vertex on one joint with weight 1."""
    j = np.zeros((n, 4), dtype=np.uint32)
    j[:, 0] = joint
    w = np.zeros((n, 4), dtype=np.float32)
    w[:, 0] = 1.0
    return j, w


UP = joint_matrix(0.0, 0.3, 0.0, 0.6)       # rows 16-60 of 192: band 0 of three 64-row bands
DOWN = joint_matrix(0.4, 0.3, 0.0, -0.6)    # rows 132-175: band 2
