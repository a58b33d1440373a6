"""The numpy model of include/swr.h "Morph targets": the morphed vertices and normals, operation for operation — IEEE binary32, one
rounding each, no FMA (numpy float32 arithmetic never fuses), an explicit skip of every target whose weight compares equal to 0 —
and the scene the tests share.  It composes with tests/skin_model.py: morph first, then skin."""
import numpy as np

import skin_model as SM

MORPH_MAX_TARGETS = 256
W, H = SM.W, SM.H


def _morph(base, deltas, weights):
    """p = b; for t ascending with w[t] != 0: p = p + w[t] * d[t] (the product rounded, then the sum)."""
    p = np.array(base, dtype=np.float32, copy=True)
    d = np.asarray(deltas, dtype=np.float32)
    w = np.asarray(weights, dtype=np.float32).reshape(-1)
    assert d.ndim == 3 and d.shape[0] == w.shape[0] and d.shape[1:] == p.shape, (d.shape, w.shape, p.shape)
    with np.errstate(all="ignore"):
        for t in range(w.shape[0]):
            if w[t] != np.float32(0.0):         # (false for +0 and -0, true for NaN)
                p = p + w[t] * d[t]
    assert p.dtype == np.float32
    return p


def morph_vertices(vertices, position_deltas, weights):
    """The morphed copy of an (n, 8) vertex array: positions morphed, colours and padding lanes as they are."""
    v = np.array(vertices, dtype=np.float32, copy=True).reshape(-1, 8)
    v[:, 0:3] = _morph(v[:, 0:3], position_deltas, weights)
    return v


def morph_attrs(attrs, normal_deltas, weights):
    """The morphed copy of an (n, 8) attribute array: normals morphed (normal_deltas None: as they are), uv as it is."""
    a = np.array(attrs, dtype=np.float32, copy=True).reshape(-1, 8)
    if normal_deltas is not None:
        a[:, 0:3] = _morph(a[:, 0:3], normal_deltas, weights)
    return a


def morph_then_skin(vertices, position_deltas, weights, joint, weight, joints):
    return SM.pose_vertices(morph_vertices(vertices, position_deltas, weights), joint, weight, joints)


# ---- the shared scene: the torus of tests/skin_model.py with five targets ----------------------------------------------------------
SWELL, SHEAR, LIFT, NONFINITE, UNSWELL = range(5)
SWELL_AMP, SHEAR_AMP, LIFT_Y = 0.08, 0.5, 0.7


def torus(S):
    return SM.torus(S)


def torus_normals(S):
    return S.torus_attrs(48, 16)[:, 0:3]


def targets(S, vertices):
    """(5, nv, 3) position deltas: a swell along the normal; a shear (y += SHEAR_AMP * x) of the half with x > 0; a lift in y by
    LIFT_Y, which takes the torus (rows 24-168 of 192, in all three 64-row bands) out of the lowest band; a target of NaN and
    infinities, only ever given weight 0; and the exact negative of the first."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 8)
    n = v.shape[0]
    d = np.zeros((5, n, 3), dtype=np.float32)
    d[SWELL] = torus_normals(S) * np.float32(SWELL_AMP)
    x = v[:, 0]
    d[SHEAR, :, 1] = np.where(x > 0, x * np.float32(SHEAR_AMP), np.float32(0))
    d[LIFT, :, 1] = np.float32(LIFT_Y)
    pattern = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    d[NONFINITE] = pattern
    d[NONFINITE, 1::2] = pattern[::-1]
    d[UNSWELL] = -d[SWELL]
    return d


def normal_targets(nv, seed=0x40F):
    """(5, nv, 3) normal deltas: pseudo-random tilts for the finite targets, non-finite for NONFINITE, UNSWELL the negative of SWELL."""
    rng = np.random.RandomState(seed)
    d = (rng.random_sample((5, nv, 3)) - 0.5).astype(np.float32)
    d[NONFINITE] = np.float32(np.nan)
    d[NONFINITE, ::3, 1] = np.float32(np.inf)
    d[UNSWELL] = -d[SWELL]
    return d


WEIGHTS_A = np.array([0.75, 1.0, 0.0, 0.0, 0.0], dtype=np.float32)          # swell and shear
WEIGHTS_B = np.array([-0.5, 0.25, 0.5, -0.0, 0.375], dtype=np.float32)      # every finite target, the non-finite one at -0
