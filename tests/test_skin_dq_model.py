"""The model of the dual-quaternion skinning arithmetic (tests/skin_dq_model.py, include/swr.h "Dual-quaternion skinning"): the facts
the header's arithmetic must have, the helper binding.dual_quats, and the floors that keep the GPU cases of tests/test_skin_dq.py
from being vacuous.  CPU only."""
import numpy as np
import pytest

import kernel_matrix as KM
import skin_dq_model as DQ
import skin_model as SM

DT = 1
N = 4096


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cloud():
    """4096 N(0,1) vertices, 8 random unit joints with translations, random influences with normalised weights."""
    rng = np.random.default_rng(0xD0A1)
    v = np.zeros((N, 8), dtype=np.float32)
    v[:, 0:3] = rng.standard_normal((N, 3))
    v[:, 3:8] = rng.random((N, 5))
    joints = np.stack([DQ.dq_joint(rng.standard_normal(3), rng.uniform(-3.1, 3.1), rng.uniform(-1, 1, 3)) for _ in range(8)])
    j = rng.integers(0, 8, (N, 4)).astype(np.uint32)
    w = rng.random((N, 4)).astype(np.float32)
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    return v, j, w, joints


def one(v3, joint, weight, dq):
    v = np.zeros((1, 8), dtype=np.float32)
    v[0, 0:3] = v3
    return DQ.pose_vertices(v, np.array([joint]), np.array([weight], dtype=np.float32), np.asarray(dq, dtype=np.float32))[0, 0:3]


# ---- the six facts -----------------------------------------------------------------------------------------------------------------
def test_identity_joints_return_the_vertex_exactly(cloud):
    v, j, _, _ = cloud
    w = np.full((N, 4), 0.25, dtype=np.float32)
    p = DQ.pose_vertices(v, j, w, np.tile(DQ.IDENTITY, (8, 1)))
    assert np.array_equal(bits(p), bits(v))


def test_a_pure_translation_adds_it_exactly(cloud):
    v, _, _, _ = cloud
    t = np.array([0.375, -1.25, 2.5], dtype=np.float32)
    q = np.array([0, 0, 0, 1, t[0] / 2, t[1] / 2, t[2] / 2, 0], dtype=np.float32)
    p = DQ.pose_vertices(v, *SM.rigid_skin(N), q[None])
    assert np.array_equal(bits(p[:, 0:3]), bits(v[:, 0:3] + t)) and np.array_equal(bits(p[:, 3:]), bits(v[:, 3:]))


def test_a_half_turn_about_z_negates_x_and_y_exactly(cloud):
    v, _, _, _ = cloud
    q = np.array([0, 0, 1, 0, 0, 0, 0, 0], dtype=np.float32)
    p = DQ.pose_vertices(v, *SM.rigid_skin(N), q[None])
    assert np.array_equal(bits(p[:, 0:3]), bits(v[:, 0:3] * np.array([-1, -1, 1], dtype=np.float32)))


def test_negating_a_joint_changes_no_bit(cloud):
    """q and -q are the same motion: all eight floats of any one joint negated, the pivots' joints included."""
    v, j, w, joints = cloud
    want, want_n = DQ.pose_vertices(v, j, w, joints), DQ.pose_attrs(v, j, w, joints)
    assert not np.array_equal(bits(want[:, 0:3]), bits(v[:, 0:3]))
    for k in range(8):
        assert (j[:, 0] == k).any() and (j[:, 1:] == k).any(), "joint k is a pivot somewhere and a follower somewhere"
        neg = joints.copy()
        neg[k] = -neg[k]
        assert np.array_equal(bits(DQ.pose_vertices(v, j, w, neg)), bits(want)), k
        assert np.array_equal(bits(DQ.pose_attrs(v, j, w, neg)), bits(want_n)), k


def test_the_candy_wrapper(cloud):
    """Identity and a half turn about x, weights (1/2, 1/2).  The dual-quaternion blend is a quarter turn: the distance from the x axis
    is kept.  The linear blend of the two matrices puts every vertex ON the axis: the reason the feature exists."""
    v, _, _, _ = cloud
    j = np.tile(np.array([0, 1, 0, 0], dtype=np.uint32), (N, 1))
    w = np.tile(np.array([0.5, 0.5, 0, 0], dtype=np.float32), (N, 1))
    half = np.array([1, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)
    p = DQ.pose_vertices(v, j, w, np.stack([DQ.IDENTITY, half]))
    r = np.hypot(v[:, 1].astype(np.float64), v[:, 2].astype(np.float64))
    r1 = np.hypot(p[:, 1].astype(np.float64), p[:, 2].astype(np.float64))
    ratio = r1 / r
    print("r'/r in [%.9f, %.9f]" % (ratio.min(), ratio.max()))
    assert r.min() > 1e-3
    assert (0.999 <= ratio).all() and (ratio <= 1.001).all()
    assert np.array_equal(bits(p[:, 0]), bits(v[:, 0])), "x stays"
    m_half = np.diag([1.0, -1.0, -1.0, 1.0])
    lin = SM.pose_vertices(v, j, w, DQ.column_major([np.eye(4), m_half]))
    assert (np.hypot(lin[:, 1], lin[:, 2]) == 0).all(), "linear blend: r' == 0"


RIGID_BOUND = 3.0e-6    # measured on these inputs: 1.08e-6 (about 14 roundings of 2^-24 relative on terms of up to |v| + |t| ~ 6)


def test_one_rigid_joint_against_float64(cloud):
    v, _, _, _ = cloud
    rng = np.random.default_rng(77)
    worst = 0.0
    for _ in range(8):
        axis, angle, t = rng.standard_normal(3), rng.uniform(-3.1, 3.1), rng.uniform(-1, 1, 3)
        p = DQ.pose_vertices(v, *SM.rigid_skin(N), DQ.dq_joint(axis, angle, t)[None])
        M = DQ.rigid_matrix(axis, angle, t)
        want = v[:, 0:3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        worst = max(worst, float(np.abs(p[:, 0:3].astype(np.float64) - want).max()))
    print("one rigid joint against float64: max abs error %.3g" % worst)
    assert worst <= RIGID_BOUND
    assert RIGID_BOUND <= 8 * 1.08e-6


# ---- the corners of the arithmetic -------------------------------------------------------------------------------------------------
def test_a_zero_or_nan_dot_product_keeps_the_weight():
    x_half = [1, 0, 0, 0, 0, 0, 0, 0]           # orthogonal to the identity: s == 0
    ident = [0, 0, 0, 1, 0, 0, 0, 0]
    # s == 0 keeps +1/2: the blend is (1/2, 0, 0, 1/2), a quarter turn about x: (0, 1, 0) -> (0, 0, 1)
    p = one([0, 1, 0], [0, 1, 0, 0], [0.5, 0.5, 0, 0], [ident, x_half])
    assert np.allclose(p, [0, 0, 1], atol=1e-6)
    # had the weight been negated the blend were (-1/2, 0, 0, 1/2): the quarter turn the other way
    q = one([0, 1, 0], [0, 1, 0, 0], [0.5, -0.5, 0, 0], [ident, x_half])
    assert np.allclose(q, [0, 0, -1], atol=1e-6)
    # -0 is not < 0 either
    neg0 = [1, 0, 0, -0.0, 0, 0, 0, 0]
    assert np.array_equal(bits(one([0, 1, 0], [0, 1, 0, 0], [0.5, 0.5, 0, 0], [ident, neg0])), bits(p))
    # a NaN s_k (a NaN real part) keeps the weight: the sign is not flipped, and the NaN reaches the vertex
    nanj = [np.nan, 0, 0, 1, 0, 0, 0, 0]
    C = DQ._blend(np.array([[0, 1, 0, 0]]), np.array([[0.5, 0.25, 0, 0]], dtype=np.float32), np.array([ident, nanj], dtype=np.float32))
    assert np.isnan(C[0][0])
    assert np.isnan(one([0, 1, 0], [0, 1, 0, 0], [0.5, 0.25, 0, 0], [ident, nanj])).all()


def test_all_zero_weights_give_nan():
    """B = 0, l = 0, i = inf, C = 0 * inf = NaN."""
    p = one([1, 2, 3], [0, 0, 0, 0], [0, 0, 0, 0], [[0, 0, 0, 1, 0, 0, 0, 0]])
    assert np.isnan(p).all()
    # and so do two opposite halves of one rotation whose dot product is not negative: s == 0 is the only such case
    p = one([1, 2, 3], [0, 1, 0, 0], [0.5, -0.5, 0, 0], [[0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0]])
    assert np.isnan(p).all()


def test_a_zero_weight_does_not_skip_a_nan_joint():
    ident = [0, 0, 0, 1, 0, 0, 0, 0]
    for bad in ([0, 0, 0, 1, np.nan, 0, 0, 0], [0, np.inf, 0, 1, 0, 0, 0, 0]):
        p = one([1, 2, 3], [0, 1, 0, 0], [1, 0, 0, 0], [ident, bad])
        assert np.isnan(p).any(), bad
    assert np.array_equal(one([1, 2, 3], [0, 0, 0, 0], [1, 0, 0, 0], [ident, [0, 0, 0, 1, np.nan, 0, 0, 0]]), [1, 2, 3])


def test_normals_take_no_translation(swr):
    v, _ = SM.torus(swr.scenes)
    a = swr.scenes.torus_attrs(48, 16)
    j, w = SM.bend_skin(v)
    pose = DQ.twist_pose()
    shifted = DQ.twist_pose(t=(3.0, -2.0, 7.0))
    assert not np.array_equal(bits(DQ.pose_vertices(v, j, w, pose)), bits(DQ.pose_vertices(v, j, w, shifted)))
    assert np.array_equal(bits(DQ.pose_attrs(a, j, w, pose)), bits(DQ.pose_attrs(a, j, w, shifted)))
    assert np.array_equal(DQ.pose_attrs(a, j, w, pose)[:, 4:8], a[:, 4:8])
    assert not np.array_equal(DQ.pose_attrs(a, j, w, pose)[:, 0:3], a[:, 0:3])
    # no renormalisation is needed: the blend is a rotation, so the length stays to rounding
    n0 = np.linalg.norm(a[:, 0:3].astype(np.float64), axis=1)
    n1 = np.linalg.norm(DQ.pose_attrs(a, j, w, pose)[:, 0:3].astype(np.float64), axis=1)
    assert np.abs(n1 / n0 - 1).max() < 1e-6


def test_the_order_of_the_influences_matters():
    """B = ((u0 Q0 + u1 Q1) + u2 Q2) + u3 Q3 in float32, and influence 0 is the pivot: the dual parts 1e8, -1e8 and 0.25 cancel or
    round away depending on the order."""
    j0 = [0, 0, 0, 1, 1.0e8, 0, 0, 0]
    j1 = [0, 0, 0, 1, -1.0e8, 0, 0, 0]
    j2 = [0, 0, 0, 1, 0.25, 0, 0, 0]
    a = one([0, 0, 0], [0, 1, 2, 0], [1, 1, 1, 0], [j0, j1, j2])
    b = one([0, 0, 0], [2, 1, 0, 0], [1, 1, 1, 0], [j0, j1, j2])
    # l = 3, i = fl(1/3); the dual x is 0.25 * i or 0 * i; t.x = 2 * that
    third = np.float32(1.0) / np.float32(3.0)
    assert a[0] == np.float32(2.0) * (np.float32(0.25) * third) and b[0] == 0.0
    assert bits(a)[0] != bits(b)[0]


# ---- binding.dual_quats ------------------------------------------------------------------------------------------------------------
DUAL_QUATS_BOUND = 1.2e-7   # one rounding to float32 of components of at most 1 (2^-24 = 6e-8) over float64 noise


def test_dual_quats_round_trips_rigid_matrices(swr):
    D = swr.binding.dual_quats
    cases = [((1, 0, 0), 0.7, (0.1, -0.2, 0.3)), ((0, 1, 0), -2.9, (1, 2, -3)), ((0, 0, 1), 3.1, (0, 0.5, 0)),
             ((1, 0, 0), 3.14159, (0, 0, 0)), ((0, 1, 0), 3.14159, (0, 0, 1)), ((0, 0, 1), 0.0, (0.25, 0, 0)), ((1, 2, -3), 4.0, (-1, 1, 0.5))]
    M = np.stack([DQ.rigid_matrix(*c) for c in cases])
    q = D(M)
    assert q.shape == (len(cases), 8) and q.dtype == np.float32
    assert (q[:, 3] >= 0).all(), "w >= 0"
    assert np.abs(np.linalg.norm(q[:, 0:4].astype(np.float64), axis=1) - 1).max() < 1e-7
    for k, c in enumerate(cases):
        want = DQ.dq_joint(*c).astype(np.float64)
        if want[3] < 0 or (want[3] == 0 and want[:3].sum() < 0):
            want = -want
        err = np.abs(q[k].astype(np.float64) - want).max() / max(1.0, np.abs(want).max())
        print(c, "error %.3g" % err)
        assert err <= DUAL_QUATS_BOUND, (c, q[k], want)
    # ... and back: the model on the table moves points as the matrix does
    pts = np.zeros((5, 8), dtype=np.float32)
    pts[:, 0:3] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.3, -0.7, 0.2], [-1, -1, -1]]
    for k in range(len(cases)):
        got = DQ.pose_vertices(pts, *SM.rigid_skin(5), q[k][None])[:, 0:3].astype(np.float64)
        want = pts[:, 0:3].astype(np.float64) @ M[k][:3, :3].T + M[k][:3, 3]
        assert np.abs(got - want).max() < 5e-6, k
    assert np.array_equal(D(np.eye(4)[None]), DQ.IDENTITY[None])
    assert np.array_equal(D(SM.joint_matrix(0.0, 1.0, 0.5, -1.0, 2.0).reshape(4, 4).T[None]),
                          np.array([[0, 0, 0, 1, 0.25, -0.5, 1.0, 0]], dtype=np.float32))


# ---- the floors of tests/test_skin_dq.py -------------------------------------------------------------------------------------------
POSED_PIXELS = 18919        # what the oracle covers of the model-posed torus under the z-test (the linear blend of the same joints: 14082)


def test_the_shared_cases_are_not_vacuous(swr, oracle):
    v, i = SM.torus(swr.scenes)
    assert v.shape[0] == 768 and i.size == 3 * 1536
    j, w = SM.bend_skin(v)
    assert ((w[:, 0] > 0) & (w[:, 1] > 0)).sum() > 300
    pose = DQ.twist_pose()
    assert np.array_equal(pose[2], -pose[1]) and np.array_equal(pose[3], -pose[0]) and (w[:, 2:] == 0).all()
    posed = DQ.pose_vertices(v, j, w, pose)
    assert np.isfinite(posed).all()
    linear = SM.pose_vertices(v, j, w, DQ.twist_matrices())
    flags = DT | oracle.TINV_PER_TRIANGLE
    c0, d0, _, code0 = oracle.render(v, i, KM.IDENT, DQ.W, DQ.H, flags)
    c1, d1, _, code1 = oracle.render(posed, i, KM.IDENT, DQ.W, DQ.H, flags)
    c2, d2, _, code2 = oracle.render(linear, i, KM.IDENT, DQ.W, DQ.H, flags)
    assert code0 == 0 and code1 == 0 and code2 == 0
    cov1 = int(np.isfinite(d1).sum())
    differ = int(((c1 != c2).any(axis=-1) | (d1.view(np.uint32) != d2.view(np.uint32))).sum())
    print("bind pixels", int(np.isfinite(d0).sum()), "dual-quaternion pixels", cov1, "linear pixels", int(np.isfinite(d2).sum()),
          "dq against linear", differ, "dq against bind", int((c0 != c1).any(axis=-1).sum()))
    assert np.isfinite(d0).sum() == 21334       # the bind pose under the z-test
    assert cov1 >= POSED_PIXELS
    assert differ > 1000, "the two skinning modes draw different frames of the same two joints"
    assert (c0 != c1).any(axis=-1).sum() > 5000, "the pose moves the image"
    # the three-band poses lie in bands 0 and 2
    jr, wr = SM.rigid_skin(v.shape[0])
    for dq, band in ((DQ.UP, 0), (DQ.DOWN, 2)):
        _, d, _, code = oracle.render(DQ.pose_vertices(v, jr, wr, dq), i, KM.IDENT, DQ.W, DQ.H, flags)
        rows = np.nonzero(np.isfinite(d).any(axis=1))[0]
        print("band", band, "rows", int(rows[0]), int(rows[-1]), "pixels", int(np.isfinite(d).sum()))
        assert code == 0 and rows.size > 20 and 64 * band <= rows[0] and rows[-1] < 64 * (band + 1)
