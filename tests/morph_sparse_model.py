"""The numpy model of include/swr.h "Sparse morph targets": per target, p[idx] = p[idx] + w * d on the vertices the target lists and
on no others — IEEE binary32, one rounding each, no FMA, an explicit skip of every target whose weight compares equal to 0 — and the
rig the tests share: the torus of tests/morph_model.py with seven sparse targets.  It composes with tests/skin_model.py: morph first,
then skin."""
import numpy as np

import morph_model as MM
import skin_model as SM

W, H = MM.W, MM.H


def _morph(base, targets, weights, which=1):
    """p = b; for t ascending with w[t] != 0: p[idx_t] = p[idx_t] + w[t] * d_t (the product rounded, then the sum).  targets[t] is
    (indices, position deltas[, normal deltas]); `which` picks the deltas."""
    p = np.array(base, dtype=np.float32, copy=True)
    w = np.asarray(weights, dtype=np.float32).reshape(-1)
    assert len(targets) == w.shape[0], (len(targets), w.shape)
    with np.errstate(all="ignore"):
        for t, target in enumerate(targets):
            idx = np.asarray(target[0], dtype=np.int64).reshape(-1)
            if idx.size == 0 or not w[t] != np.float32(0.0):          # (skipped for +0 and -0, applied for NaN)
                continue
            assert (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < p.shape[0], "strictly ascending, in range"
            d = np.asarray(target[which], dtype=np.float32).reshape(-1, 3)
            assert d.shape[0] == idx.size
            p[idx] = p[idx] + w[t] * d
    assert p.dtype == np.float32
    return p


def morph_vertices(vertices, targets, weights):
    """The morphed copy of an (n, 8) vertex array: listed positions morphed, everything else as it is."""
    v = np.array(vertices, dtype=np.float32, copy=True).reshape(-1, 8)
    v[:, 0:3] = _morph(v[:, 0:3], targets, weights)
    return v


def morph_attrs(attrs, targets, weights):
    """The morphed copy of an (n, 8) attribute array: listed normals morphed (targets without normal deltas: none), uv as it is."""
    a = np.array(attrs, dtype=np.float32, copy=True).reshape(-1, 8)
    if any(len(t) > 2 and t[2] is not None for t in targets):
        a[:, 0:3] = _morph(a[:, 0:3], targets, weights, which=2)
    return a


def morph_then_skin(vertices, targets, weights, joint, weight, joints):
    return SM.pose_vertices(morph_vertices(vertices, targets, weights), joint, weight, joints)


def dense(targets, nv, which=1):
    """The (T, nv, 3) dense targets with zero rows where a sparse target lists nothing."""
    d = np.zeros((len(targets), nv, 3), dtype=np.float32)
    for t, target in enumerate(targets):
        if len(target[0]):
            d[t, np.asarray(target[0], dtype=np.int64)] = target[which]
    return d


# ---- the shared rig: the torus of tests/morph_model.py with seven sparse targets ----------------------------------------------------
SWELL, SHEAR, LIFT, NONFINITE, UNSWELL, EMPTY, LAST = range(7)
TARGETS = 7


def rig(S, vertices, normals=False):
    """Seven targets.  With R the vertices with x > 0: the swell, the shear and the unswell of tests/morph_model.py on R; its lift
    listing every vertex; its non-finite target on every fifth vertex (only ever given weight +0 or -0, or 1e-30 on purpose); an empty
    target; and the last vertex alone.  normals: every non-empty target also carries normal deltas (pseudo-random tilts; not finite
    for the non-finite target; the unswell's the negative of the swell's)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 8)
    nv = v.shape[0]
    d = MM.targets(S, v)
    R = np.flatnonzero(v[:, 0] > 0).astype(np.uint32)
    every = np.arange(nv, dtype=np.uint32)
    fifth = every[::5]
    last = np.array([nv - 1], dtype=np.uint32)
    lists = [R, R, every, fifth, R, np.zeros(0, dtype=np.uint32), last]
    deltas = [d[MM.SWELL][R], d[MM.SHEAR][R], d[MM.LIFT], d[MM.NONFINITE][fifth], d[MM.UNSWELL][R], np.zeros((0, 3), dtype=np.float32),
              np.array([[0.3, 0.3, 0.0]], dtype=np.float32)]
    if not normals:
        return [(i, np.ascontiguousarray(x)) for i, x in zip(lists, deltas)]
    nd = MM.normal_targets(nv)
    tilt = [nd[MM.SWELL][R], nd[MM.SHEAR][R], nd[MM.LIFT], nd[MM.NONFINITE][fifth], nd[MM.UNSWELL][R], np.zeros((0, 3), dtype=np.float32),
            np.array([[0.25, -0.5, 0.125]], dtype=np.float32)]
    return [(i, np.ascontiguousarray(x), np.ascontiguousarray(n)) for i, x, n in zip(lists, deltas, tilt)]


def touched(targets, skip=()):
    """The union of the index lists (without the targets in `skip`), ascending."""
    lists = [np.asarray(t[0], dtype=np.int64) for k, t in enumerate(targets) if k not in skip]
    return np.unique(np.concatenate(lists)) if lists else np.zeros(0, dtype=np.int64)


def one(t, value=1.0):
    w = np.zeros(TARGETS, dtype=np.float32)
    w[t] = value
    return w


WEIGHTS_A = np.array([0.75, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)          # swell and shear: rows of length 0, 1 (none here) and 2
WEIGHTS_B = np.array([-0.5, 0.25, 0.5, -0.0, 0.375, 2.0, 1.0], dtype=np.float32)      # every finite target, the non-finite one at -0
