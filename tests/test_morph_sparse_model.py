"""The model of the sparse morph arithmetic (tests/morph_sparse_model.py, include/swr.h "Sparse morph targets"), the helper of the
binding that makes sparse targets from dense ones, and the floors that keep the GPU cases of tests/test_morph_sparse.py from being
vacuous.  CPU only."""
import numpy as np
import pytest

import kernel_matrix as KM
import morph_model as MM
import morph_sparse_model as MS

DT = 1
PIXELS = MS.W * MS.H


@pytest.fixture(scope="module")
def scene(swr):
    v, i = MM.torus(swr.scenes)
    return v, i, MS.rig(swr.scenes, v)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_model_is_the_headers_loop(scene):
    """Per target p[idx] = p[idx] + w * d, written out by hand for weights B."""
    v, _, T = scene
    p = v[:, 0:3].copy()
    for t in (MS.SWELL, MS.SHEAR, MS.LIFT, MS.UNSWELL, MS.LAST):        # (NONFINITE is at -0, EMPTY lists nothing)
        idx = T[t][0].astype(np.int64)
        p[idx] = p[idx] + MS.WEIGHTS_B[t] * T[t][1]
    m = MS.morph_vertices(v, T, MS.WEIGHTS_B)
    assert np.array_equal(bits(m[:, 0:3]), bits(p)) and np.isfinite(m).all()
    assert np.array_equal(bits(m[:, 3:8]), bits(v[:, 3:8])), "colour and padding lanes never change"


def test_a_set_that_lists_every_vertex_is_the_dense_model(swr, scene):
    v, _, _ = scene
    d = MM.targets(swr.scenes, v)
    every = np.arange(v.shape[0], dtype=np.uint32)
    full = [(every, d[t]) for t in range(5)]
    for w in (MM.WEIGHTS_A, MM.WEIGHTS_B):
        assert np.array_equal(bits(MS.morph_vertices(v, full, w)), bits(MM.morph_vertices(v, d, w)))
    # and the rig's shear, restricted to the vertices it moves, is the dense shear bit for bit: the torus has no -0 coordinate
    T = MS.rig(swr.scenes, v)
    assert not (bits(v[:, 0:3]) == 0x80000000).any()
    assert np.array_equal(bits(MS.morph_vertices(v, T, MS.one(MS.SHEAR))), bits(MM.morph_vertices(v, d, np.eye(5, dtype=np.float32)[MM.SHEAR])))


def test_the_helper_drops_the_all_zero_rows(swr, scene):
    v, _, T = scene
    d = MM.targets(swr.scenes, v)
    S = swr.binding.sparse_targets(d[[MM.SWELL, MM.SHEAR, MM.LIFT]])
    assert [t[0].size for t in S] == [768, 384, 768] and all(t[0].dtype == np.uint32 and t[1].shape == (t[0].size, 3) for t in S)
    assert np.array_equal(S[1][0], T[MS.SHEAR][0]) and np.array_equal(bits(S[1][1]), bits(T[MS.SHEAR][1]))
    w = np.array([0.75, 1.0, -0.5], dtype=np.float32)
    assert np.array_equal(bits(MS.morph_vertices(v, S, w)), bits(MM.morph_vertices(v, d[[MM.SWELL, MM.SHEAR, MM.LIFT]], w)))
    both = swr.binding.sparse_targets(d[[MM.SHEAR]], np.zeros((1, 768, 3), dtype=np.float32))
    assert len(both[0]) == 3 and both[0][2].shape == (384, 3)
    assert MS.dense(T, 768).shape == (7, 768, 3) and np.array_equal(bits(MS.dense(T, 768)[MS.SHEAR]), bits(d[MM.SHEAR]))


def test_the_order_of_the_targets_shows_in_the_bits(scene):
    v, _, T = scene
    swap = [1, 0, 2, 3, 4, 5, 6]
    a = MS.morph_vertices(v, T, MS.WEIGHTS_A)
    b = MS.morph_vertices(v, [T[k] for k in swap], MS.WEIGHTS_A[swap])
    differ = np.nonzero((bits(a) != bits(b)).any(axis=1))[0]
    assert differ.size > 0 and np.isin(differ, T[MS.SWELL][0]).all(), differ[:5]
    assert np.allclose(a, b, rtol=0, atol=1e-6)


def test_negative_zero_survives_unlisted_and_not_a_listed_zero_delta():
    """The hand-made three-vertex scene of the GPU case: vertex 0 is listed with a zero delta, vertex 1 is not listed."""
    base = np.array([[-0.0, -0.0, 1.0], [-0.0, -0.0, 1.0], [0.5, 0.5, 0.5]], dtype=np.float32)
    T = [(np.array([0, 2], dtype=np.uint32), np.array([[0, 0, 0], [0.25, 0, 0]], dtype=np.float32))]
    p = MS._morph(base, T, [1.0])
    assert bits(p).tolist() == [[0, 0, 0x3F800000], [0x80000000, 0x80000000, 0x3F800000], [0x3F400000, 0x3F000000, 0x3F000000]]
    # the dense target with zero rows makes both +0
    assert bits(MM._morph(base, MS.dense(T, 3), [1.0]))[1].tolist() == [0, 0, 0x3F800000]
    for zero in (0.0, -0.0):
        assert np.array_equal(bits(MS._morph(base, T, [zero])), bits(base))


def test_a_nan_weight_poisons_listed_vertices_only(scene):
    v, _, T = scene
    for bad in (np.nan, np.inf):
        m = MS.morph_vertices(v, T, MS.one(MS.SHEAR, bad))
        listed = np.zeros(768, dtype=bool)
        listed[T[MS.SHEAR][0]] = True
        assert not np.isfinite(m[listed, 0:3]).all(axis=1).any(), "every listed vertex has a non-finite lane (0 * inf, NaN * 0)"
        assert np.array_equal(bits(m[~listed]), bits(v[~listed])), "an unlisted vertex is untouched"
        assert not np.isfinite(MM.morph_vertices(v, MS.dense(T, 768)[:5], MS.one(MS.SHEAR, bad)[:5])[~listed, 0:3]).all(axis=1).any(), \
            "where the dense target with its zero rows poisons them all"


def test_a_zero_weight_skips_the_non_finite_target(scene):
    v, _, T = scene
    assert not np.isfinite(T[MS.NONFINITE][1]).any() and T[MS.NONFINITE][0].size == 154
    for zero in (0.0, -0.0):
        w = MS.WEIGHTS_A.copy()
        w[MS.NONFINITE] = zero
        assert np.array_equal(bits(MS.morph_vertices(v, T, w)), bits(MS.morph_vertices(v, T, MS.WEIGHTS_A)))
    w = MS.WEIGHTS_A.copy()
    w[MS.NONFINITE] = 1e-30
    bad = ~np.isfinite(MS.morph_vertices(v, T, w)[:, 0:3]).all(axis=1)
    assert np.array_equal(np.flatnonzero(bad), T[MS.NONFINITE][0])


def test_a_target_and_its_negative_need_not_cancel(scene):
    v, _, T = scene
    m = MS.morph_vertices(v, T, MS.one(MS.SWELL) + MS.one(MS.UNSWELL))
    idx = T[MS.SWELL][0].astype(np.int64)
    want = v[:, 0:3].copy()
    want[idx] = (want[idx] + T[MS.SWELL][1]) + T[MS.UNSWELL][1]
    assert np.array_equal(bits(m[:, 0:3]), bits(want))
    off = int((bits(m) != bits(v)).sum())
    print("components that do not cancel:", off)
    assert 0 < off < 3 * idx.size and np.abs(m - v).max() < 1e-7


def test_normals_take_the_same_loop(swr, scene):
    v, _, _ = scene
    a = swr.scenes.torus_attrs(48, 16)
    T = MS.rig(swr.scenes, v, normals=True)
    m = MS.morph_attrs(a, T, MS.WEIGHTS_B)
    assert np.array_equal(bits(m[:, 0:3]), bits(MS._morph(a[:, 0:3], T, MS.WEIGHTS_B, which=2)))
    assert np.array_equal(bits(m[:, 3:8]), bits(a[:, 3:8])), "uv and the padding lanes never change"
    assert np.isfinite(m).all() and not np.array_equal(m[:, 0:3], a[:, 0:3])
    assert np.array_equal(bits(MS.morph_attrs(a, MS.rig(swr.scenes, v), MS.WEIGHTS_B)), bits(a)), "without normal deltas the normals stay"


def test_the_rig_and_its_floors(oracle, scene):
    """The floors of tests/test_morph_sparse.py: each of the four large targets alone moves at least 1 % of the pixels (the counts are
    the oracle's); the lifted torus has left the lowest of three 64-row bands, which the base reaches; the touched union without the
    full-length target is 7 waves and 13 lanes."""
    v, i, T = scene
    assert v.shape[0] == 768 and i.size == 3 * 1536 and len(T) == MS.TARGETS
    assert [t[0].size for t in T] == [384, 384, 768, 154, 384, 0, 1] and T[MS.LAST][0][0] == 767
    assert MS.touched(T).size == 768 and MS.touched(T, skip=(MS.LIFT,)).size == 461 == 7 * 64 + 13
    rows = np.zeros(768, dtype=int)
    for t in T:
        rows[t[0].astype(np.int64)] += 1
    assert set(np.unique(rows)) == {1, 2, 4, 5}, "row lengths of the rig (with the lift)"
    fl = DT | oracle.TINV_PER_TRIANGLE
    c0, d0, _, code = oracle.render(v, i, KM.IDENT, MS.W, MS.H, fl)
    assert code == 0
    base_rows = np.nonzero(np.isfinite(d0).any(axis=1))[0]
    assert (base_rows[0], base_rows[-1]) == (24, 168), "the base lies in all three bands"
    counts = {}
    for t in (MS.SWELL, MS.SHEAR, MS.LIFT, MS.UNSWELL, MS.LAST):
        c1, d1, _, code = oracle.render(MS.morph_vertices(v, T, MS.one(t)), i, KM.IDENT, MS.W, MS.H, fl)
        assert code == 0
        counts[t] = int(((c0 != c1).any(axis=-1) | (bits(d0) != bits(d1))).sum())
        if t == MS.LIFT:
            lifted = np.nonzero(np.isfinite(d1).any(axis=1))[0]
            assert (lifted[0], lifted[-1]) == (0, 100) and lifted[-1] < 128 <= base_rows[-1], "the lifted torus lies in bands 0 and 1 only"
    print("pixels moved", counts)
    assert counts[MS.SWELL] >= 15336 and counts[MS.SHEAR] >= 13183 and counts[MS.LIFT] >= 30697 and counts[MS.UNSWELL] >= 11101
    assert min(counts[t] for t in (MS.SWELL, MS.SHEAR, MS.LIFT, MS.UNSWELL)) >= PIXELS // 100 + 1 == 615
    assert 0 < counts[MS.LAST] < 615, "the single vertex is an edge case of the kernel, not a floor"
