"""The model of the skinning arithmetic (tests/skin_model.py, include/swr.h "Skinned meshes") against the project's other models,
and the floors that keep the GPU cases of tests/test_skin.py from being vacuous.  CPU only."""
import numpy as np
import pytest

import kernel_matrix as KM
import skin_model as SM

DT = 1


@pytest.fixture(scope="module")
def scene(swr):
    return SM.torus(swr.scenes)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_one_joint_is_the_vertex_transform(scene):
    """One affine joint with weights (1, 0, 0, 0) is Vertex.apply of that matrix, bit for bit: 1 * r = r, and r + 0 * r' = r for the
    finite r' of the three other joints."""
    v, _ = scene
    m = SM.joint_matrix(0.37, 0.81, 0.11, -0.07, 0.05)
    j, w = SM.rigid_skin(v.shape[0], joint=1)
    pose = np.stack([SM.joint_matrix(1.0, 2.0, 3.0), m])
    posed = SM.pose_vertices(v, j, w, pose)
    want = KM.pretransform(v, m)
    assert np.array_equal(bits(posed), bits(want))
    assert not np.array_equal(bits(posed[:, 0:3]), bits(v[:, 0:3]))


def test_the_order_of_the_influences_matters():
    """acc = ((w0 r0 + w1 r1) + w2 r2) + w3 r3 in float32: swapping influences 0 and 2 changes the bits."""
    v = np.zeros((1, 8), dtype=np.float32)
    v[0, 0] = 1.0
    pose = np.stack([SM.joint_matrix(0, 1.0, 1.0e8), SM.joint_matrix(0, 1.0, -1.0e8), SM.joint_matrix(0, 1.0, 0.25)])
    w = np.array([[1, 1, 1, 0]], dtype=np.float32)
    a = SM.pose_vertices(v, np.array([[0, 1, 2, 0]]), w, pose)
    b = SM.pose_vertices(v, np.array([[2, 1, 0, 0]]), w, pose)
    assert a[0, 0] == np.float32(1.25)          # (1e8 - 1e8) + 1.25: the big terms cancel first
    assert b[0, 0] == np.float32(0.0)           # (1.25 - 1e8) + 1e8: the small term is rounded away
    assert bits(a)[0, 0] != bits(b)[0, 0]


def test_nan_and_inf_propagate():
    v = np.zeros((3, 8), dtype=np.float32)
    v[:, 0:3] = [[1, 2, 3], [np.inf, 0, 0], [1, 1, 1]]
    j = np.zeros((3, 4), dtype=np.uint32)
    w = np.zeros((3, 4), dtype=np.float32)
    w[:, 0] = 1.0
    w[2, 3] = np.nan                            # a NaN weight on an otherwise unused influence
    ident = SM.joint_matrix()
    p = SM.pose_vertices(v, j, w, ident[None])
    assert np.array_equal(p[0, 0:3], [1, 2, 3])
    assert np.isnan(p[1, 0:3]).all()            # 0 * inf: in the other rows, and in x under the zero weights of influences 1..3
    assert np.isnan(p[2, 0:3]).all()
    w[:, 0] = np.inf
    p = SM.pose_vertices(v[:1], j[:1], w[:1], ident[None])
    assert np.isposinf(p[0, 0:3]).all()
    # a zero weight does not skip a non-finite joint: 0 * inf is NaN
    pose = np.stack([ident, SM.joint_matrix(0, 1, np.inf)])
    p = SM.pose_vertices(v[:1], np.array([[0, 1, 0, 0]]), np.array([[1, 0, 0, 0]], dtype=np.float32), pose)
    assert np.isnan(p[0, 0]) and p[0, 1] == 2 and p[0, 2] == 3


def test_negative_zero_becomes_positive_zero():
    """x = -0 through the identity joint: -0 * 1 = -0, but the sum with the +0 terms of the other columns and influences is +0."""
    v = np.zeros((1, 8), dtype=np.float32)
    v[0, 0:3] = [-0.0, -0.0, 1.0]
    j, w = SM.rigid_skin(1)
    p = SM.pose_vertices(v, j, w, SM.joint_matrix()[None])
    assert bits(v)[0, 0] == 0x80000000 and bits(p)[0, 0] == 0 and bits(p)[0, 1] == 0 and p[0, 2] == 1.0


def test_normals_take_no_translation(swr, scene):
    v, _ = scene
    a = swr.scenes.torus_attrs(48, 16)
    j, w = SM.bend_skin(v)
    pose = SM.bend_pose()
    shifted = pose.copy()
    shifted[:, 12:15] += 5.0
    assert np.array_equal(bits(SM.pose_attrs(a, j, w, pose)), bits(SM.pose_attrs(a, j, w, shifted)))
    assert np.array_equal(SM.pose_attrs(a, j, w, pose)[:, 4:8], a[:, 4:8])
    assert not np.array_equal(SM.pose_attrs(a, j, w, pose)[:, 0:3], a[:, 0:3])


def test_the_shared_cases_are_not_vacuous(oracle, scene):
    """The floors of tests/test_skin.py: the bend moves the image, and the up and down poses lie in bands 0 and 2 of three."""
    v, i = scene
    assert v.shape[0] == 768 and i.size == 3 * 1536
    j, w = SM.bend_skin(v)
    assert (w[:, 0] > 0).any() and (w[:, 1] > 0).any() and ((w[:, 0] > 0) & (w[:, 1] > 0)).any()
    posed = SM.pose_vertices(v, j, w, SM.bend_pose())
    c0, d0, _, code0 = oracle.render(v, i, KM.IDENT, SM.W, SM.H, DT | oracle.TINV_PER_TRIANGLE)
    c1, d1, _, code1 = oracle.render(posed, i, KM.IDENT, SM.W, SM.H, DT | oracle.TINV_PER_TRIANGLE)
    assert code0 == 0 and code1 == 0
    cov0, cov1 = np.isfinite(d0), np.isfinite(d1)
    print("bind pixels", int(cov0.sum()), "posed pixels", int(cov1.sum()), "differ", int((c0 != c1).any(axis=-1).sum()))
    assert cov0.sum() == 21334                  # the bind pose under the z-test
    assert cov1.sum() > 10000 and (c0 != c1).any(axis=-1).sum() > 10000
    jr, wr = SM.rigid_skin(v.shape[0])
    for m, band in ((SM.UP, 0), (SM.DOWN, 2)):
        _, d, _, code = oracle.render(SM.pose_vertices(v, jr, wr, m[None]), i, KM.IDENT, SM.W, SM.H, DT | oracle.TINV_PER_TRIANGLE)
        rows = np.nonzero(np.isfinite(d).any(axis=1))[0]
        print("band", band, "rows", int(rows[0]), int(rows[-1]))
        assert code == 0 and rows.size > 30 and 64 * band <= rows[0] and rows[-1] < 64 * (band + 1)
