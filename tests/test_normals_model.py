"""The numpy model of "Computed normals" (tests/normals_model.py) against hand-computed cases, and the floors that keep the GPU cases
of tests/test_normals.py from being vacuous, computed with the oracle.  CPU only."""
import dataclasses

import numpy as np
import pytest

import kernel_matrix as KM
import morph_sparse_model as MS
import normals_model as NM
import skin_model as SM

DT = KM.DT


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def pack(swr, xyz):
    xyz = np.asarray(xyz, dtype=np.float32)
    return swr.scenes.pack_vertices(xyz, np.full(xyz.shape, 0.5, dtype=np.float32))


# ---- hand-computed cases -------------------------------------------------------------------------------------------------------------
def test_a_single_triangle(swr):
    v = pack(swr, [[0, 0, 0], [2, 0, 0], [0, 3, 0]])
    i = np.array([0, 1, 2], dtype=np.int64)
    assert NM.face_vectors(v, i).tolist() == [[0.0, 0.0, 6.0]], "cross((2,0,0), (0,3,0))"
    assert NM.vertex_normals(v, i).tolist() == [[0.0, 0.0, 1.0]] * 3
    fv, fa, fi = NM.flat_scene(v, np.zeros((3, 8), dtype=np.float32), i)
    assert fi.tolist() == [0, 1, 2] and np.array_equal(fv, v) and fa[:, 0:3].tolist() == [[0.0, 0.0, 6.0]] * 3, "flat: not normalised"
    # every operation rounds once: the products of the cross product are rounded before they are subtracted
    a, b = np.float32(1.0) + np.float32(2.0 ** -12), np.float32(1.0) - np.float32(2.0 ** -12)
    w = pack(swr, [[0, 0, 0], [a, b, 0], [b, a, 0]])
    exact = float(a) * float(a) - float(b) * float(b)
    fz = NM.face_vectors(w, i)[0, 2]
    assert fz == np.float32(np.float32(a * a) - np.float32(b * b)) and float(fz) != exact, "a fused multiply-subtract would give the exact value"
    # trailing indices are ignored
    assert NM.face_vectors(v, np.array([0, 1, 2, 1, 2], dtype=np.int64)).shape == (1, 3)


def test_a_quad_of_two_triangles(swr):
    """(0, 1, 2) and (0, 2, 3) over a folded quad: the shared vertices 0 and 2 get the sum of two faces, in triangle order."""
    v = pack(swr, [[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0]])
    i = np.array([0, 1, 2, 0, 2, 3], dtype=np.int64)
    f = NM.face_vectors(v, i)
    assert f.tolist() == [[0.0, -0.5, 1.0], [-0.5, 0.0, 1.0]]
    n = NM.vertex_normals(v, i)
    s = (f[0] + f[1]).astype(np.float32)                 # (-0.5, -0.5, 2)
    l = np.sqrt(np.float32(np.float32(s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
    shared = s * (np.float32(1.0) / l)
    assert np.array_equal(bits(n[0]), bits(shared)) and np.array_equal(bits(n[2]), bits(shared))
    for k, face in ((1, f[0]), (3, f[1])):
        lk = np.sqrt(np.float32(np.float32(face[0] * face[0] + face[1] * face[1]) + face[2] * face[2]))
        assert np.array_equal(bits(n[k]), bits(face * (np.float32(1.0) / lk)))
    off, tri = NM.adjacency(i, 4)
    assert off.tolist() == [0, 2, 3, 5, 6] and tri.tolist() == [0, 1, 0, 0, 1, 1]


def test_the_walk_order_decides_the_bits(swr):
    """Three faces at one vertex whose sum depends on the order: the model adds them in ascending triangle order."""
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    # triangles with face z = 2^24, 1, 1 around vertex 0 (z = the doubled area in the xy plane)
    v = pack(swr, [[0, 0, 0], [big, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0]])
    small = [0, 3, 4]
    for order, want in (([[0, 1, 2], small, small], big), ([small, small, [0, 1, 2]], big + np.float32(2.0))):
        i = np.array(order, dtype=np.int64).reshape(-1)
        f = NM.face_vectors(v, i)
        assert sorted(f[:, 2].tolist()) == [1.0, 1.0, float(big)]
        n = np.zeros(3, dtype=np.float32)
        for p in range(3):
            n = n + f[p]
        assert n[2] == want, "(2^24 + 1) + 1 = 2^24, (1 + 1) + 2^24 = 2^24 + 2"
        assert NM.vertex_normals(v, i)[0].tolist() == [0.0, 0.0, 1.0]
    # a triangle that names a vertex twice adds twice: its row holds the triangle twice
    off, tri = NM.adjacency(np.array([5, 5, 6], dtype=np.int64), 7)
    assert tri[off[5]:off[6]].tolist() == [0, 0] and tri[off[6]:off[7]].tolist() == [0]


def test_flip_is_the_negation_up_to_the_sign_of_zeros(swr):
    v, i = NM.torus(swr.scenes)
    f, g = NM.face_vectors(v, i), NM.face_vectors(v, i, flip=True)
    assert np.array_equal(f, -g) and not np.array_equal(bits(f), bits(g))
    n, m = NM.vertex_normals(v, i), NM.vertex_normals(v, i, flip=True)
    assert np.array_equal(n, -m), "sums of negated terms in the same order, and a symmetric normalisation"
    assert np.isfinite(n).all() and np.abs(np.sqrt((n.astype(np.float64) ** 2).sum(axis=1)) - 1).max() < 1e-6
    own = swr.scenes.torus_attrs(48, 16)[:, 0:3]
    assert (n * own).sum(axis=1).min() > 0.999, "the torus's computed normals point where its own do"
    # the sign of zeros: the faces of a degenerate triangle are zeros of whichever sign, and from (+0, +0, +0) they sum to +0
    w = pack(swr, [[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    t = np.array([0, 1, 2], dtype=np.int64)
    assert set(bits(NM.face_vectors(w, t)).reshape(-1).tolist()) | set(bits(NM.face_vectors(w, t, True)).reshape(-1).tolist()) <= {0, 0x80000000}
    assert bits(NM.vertex_normals(w, t, True)).tolist() == [[0, 0, 0]] * 3 == bits(NM.vertex_normals(w, t)).tolist()


def test_the_hub_scene(swr):
    v, i = NM.hub(swr.scenes)
    assert v.shape[0] == NM.HUB_NV == 312 and i.size == 3 * NM.HUB_NTRI and NM.HUB_NV % 64 == 56 and NM.HUB_NTRI % 64 == 48
    off, tri = NM.adjacency(i, NM.HUB_NV)
    rows = np.diff(off)
    assert rows[NM.HUB] == 300 and tri[off[0]:off[1]].tolist() == list(range(300))
    assert set(rows[1:301].tolist()) == {2} and rows[NM.LONE:NM.LONE + 3].tolist() == [1, 1, 1]
    assert rows[NM.UNUSED] == 0 and rows[NM.TWICE:NM.TWICE + 2].tolist() == [2, 1] and tri[off[NM.TWICE]:off[NM.TWICE + 1]].tolist() == [301, 301]
    assert tri[off[1]:off[2]].tolist() == [0, 299], "vertex 1: corner 1 of triangle 0, corner 2 of triangle 299"
    assert tri[off[NM.SHARED]:off[NM.SHARED + 1]].tolist() == [302, 303]
    n = NM.vertex_normals(v, i)
    assert bits(n[NM.UNUSED]).tolist() == [0, 0, 0], "the unreferenced vertex is zero"
    assert bits(n[NM.TWICE]).tolist() == [0, 0, 0], "twice a zero face"
    bad = np.flatnonzero(np.isnan(n).any(axis=1))
    assert bad.tolist() == [NM.NAN_VERTEX, NM.SHARED, NM.NAN_TRI + 2], "the NaN reaches the vertices of its triangle and nothing else"
    assert np.isfinite(n[NM.NEIGHBOUR:NM.NEIGHBOUR + 2]).all() and np.isnan(NM.face_vectors(v, i)).any(axis=1).sum() == 1
    # the hub's normal is the sum of 300 faces in order: another order gives other bits
    f = NM.face_vectors(v, i)[:300]
    fwd, back = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    for p in range(300):
        fwd, back = fwd + f[p], back + f[299 - p]
    l = np.sqrt(np.float32(np.float32(fwd[0] * fwd[0] + fwd[1] * fwd[1]) + fwd[2] * fwd[2]))
    assert np.array_equal(bits(n[0]), bits(fwd * (np.float32(1.0) / l))) and not np.array_equal(bits(fwd), bits(back))
    fv, fa, fi = NM.flat_scene(v, NM.hub_attrs(swr.scenes), i)
    assert fv.shape == (912, 8) and fi.tolist() == list(range(912)) and np.array_equal(bits(fa[:, 3:]), bits(NM.hub_attrs(swr.scenes)[i][:, 3:]))


# ---- the floors of tests/test_normals.py ---------------------------------------------------------------------------------------------
def test_the_floors(swr, oracle):
    """Under SWR_SHADER_PHONG on the torus in pose A (the counts are the oracle's own, so the oracle alone passes them): the SMOOTH
    frame is not the frame of the posed uploaded normals, FLAT is not SMOOTH, FLIP is not no FLIP; and a morph without normal deltas
    changes the SMOOTH frame also where it leaves the depth as it is — triangles that did not move beside vertices that did — where
    the frame of the uploaded normals does not change at all."""
    S = swr.scenes
    v, i = NM.torus(S)
    a = NM.torus_uploaded_attrs(S)
    sh = S.random_shading(768, 0x51, 1)
    joint, weight = NM.torus_skin(v)
    P = SM.bend_pose()
    pv, pa = SM.pose_vertices(v, joint, weight, P), SM.pose_attrs(a, joint, weight, P)

    def frame(scene):
        vv, aa, ii = scene
        return KM.oracle_clear(oracle, vv, ii, KM.IDENT, NM.W, NM.H, DT, shading=dataclasses.replace(sh, attrs=aa))

    def differ(x, y):
        return int((x[0] != y[0]).any(axis=-1).sum())

    up = frame((pv, pa, i))
    smooth, flat = frame(NM.expected_scene(NM.SMOOTH, pv, a, i)), frame(NM.expected_scene(NM.FLAT, pv, a, i))
    smooth_f, flat_f = frame(NM.expected_scene(NM.SMOOTH, pv, a, i, True)), frame(NM.expected_scene(NM.FLAT, pv, a, i, True))
    assert up[1].tobytes() == smooth[1].tobytes() == flat[1].tobytes() == flat_f[1].tobytes(), "normals never move a depth"
    counts = (differ(smooth, up), differ(flat, smooth), differ(smooth, smooth_f), differ(flat, flat_f))
    print("covered", int(np.isfinite(up[1]).sum()), "pixels; differing", counts)
    assert counts[0] >= 18042 and counts[1] >= 19066 and counts[2] >= 21103 and counts[3] >= 21120
    assert min(counts) > NM.W * NM.H // 5
    T = MS.rig(S, v)
    mpv = SM.pose_vertices(MS.morph_vertices(v, T, MS.WEIGHTS_A), joint, weight, P)
    up_m, smooth_m = frame((mpv, pa, i)), frame(NM.expected_scene(NM.SMOOTH, mpv, a, i))
    still = (bits(up[1]) == bits(up_m[1])) & np.isfinite(up[1])
    moved_up, moved_smooth = (up[0] != up_m[0]).any(axis=-1), (smooth[0] != smooth_m[0]).any(axis=-1)
    print("pixels of unmoved depth", int(still.sum()), "recoloured: uploaded", int((moved_up & still).sum()), "smooth", int((moved_smooth & still).sum()))
    assert still.sum() >= 8244 and (moved_up & still).sum() == 0 and (moved_smooth & still).sum() >= 599
    assert differ(smooth, smooth_m) >= 18389


def test_the_hub_floors(swr, oracle):
    S = swr.scenes
    v, i = NM.hub(S)
    a = NM.hub_attrs(S)
    sh = S.random_shading(NM.HUB_NV, 0x4B, 1)

    def frame(scene):
        vv, aa, ii = scene
        return KM.oracle_clear(oracle, vv, ii, KM.IDENT, NM.W, NM.H, DT, shading=dataclasses.replace(sh, attrs=aa))

    up, smooth, flat = frame((v, a, i)), frame(NM.expected_scene(NM.SMOOTH, v, a, i)), frame(NM.expected_scene(NM.FLAT, v, a, i))
    smooth_f = frame(NM.expected_scene(NM.SMOOTH, v, a, i, True))
    counts = [int((x[0] != y[0]).any(axis=-1).sum()) for x, y in ((up, smooth), (smooth, flat), (smooth, smooth_f))]
    print("hub: covered", int(np.isfinite(up[1]).sum()), "differing", counts)
    assert np.isfinite(up[1]).sum() >= 22495 and counts[0] >= 11197 and counts[1] >= 548 and counts[2] >= 21947
