"""The model of the morph arithmetic (tests/morph_model.py, include/swr.h "Morph targets"), and the floors that keep the GPU cases of
tests/test_morph.py from being vacuous.  CPU only."""
import numpy as np
import pytest

import kernel_matrix as KM
import morph_model as MM
import skin_model as SM

DT = 1
PIXELS = MM.W * MM.H


@pytest.fixture(scope="module")
def scene(swr):
    v, i = MM.torus(swr.scenes)
    return v, i, MM.targets(swr.scenes, v)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def one(t, value=1.0):
    w = np.zeros(5, dtype=np.float32)
    w[t] = value
    return w


def test_one_target_with_weight_one_is_base_plus_delta(scene):
    v, _, d = scene
    for t in (MM.SWELL, MM.SHEAR, MM.LIFT):
        m = MM.morph_vertices(v, d, one(t))
        assert np.array_equal(bits(m[:, 0:3]), bits(v[:, 0:3] + d[t]))      # 1 * d = d exactly
        assert np.array_equal(bits(m[:, 3:8]), bits(v[:, 3:8])), "colour and padding lanes never change"
        assert not np.array_equal(bits(m[:, 0:3]), bits(v[:, 0:3]))


def test_the_order_of_the_targets_shows_in_the_bits(scene):
    """p = (b + w0 d0) + w1 d1 in float32: walking the swell and the shear in the other order rounds differently somewhere."""
    v, _, d = scene
    swap = [1, 0, 2, 3, 4]
    a = MM.morph_vertices(v, d, MM.WEIGHTS_A)
    b = MM.morph_vertices(v, d[swap], MM.WEIGHTS_A[swap])
    differ = np.nonzero((bits(a) != bits(b)).any(axis=1))[0]
    assert differ.size > 0 and differ[0] == 22, differ[:5]
    assert np.allclose(a, b, rtol=0, atol=1e-6)
    # the textbook case: (1 + 1e8) - 1e8 against (1 - 1e8) + 1e8
    base = np.array([[1.0, 0, 0]], dtype=np.float32)
    dd = np.array([[[1.0e8, 0, 0]], [[-1.0e8, 0, 0]], [[0.25, 0, 0]]], dtype=np.float32)
    w = np.ones(3, dtype=np.float32)
    assert MM._morph(base, dd, w)[0, 0] == np.float32(0.25)                 # ((1 + 1e8) - 1e8) + 0.25: the 1 is rounded away
    assert MM._morph(base, dd[[2, 0, 1]], w)[0, 0] == np.float32(0.0)       # ((1 + 0.25) + 1e8) - 1e8


def test_a_zero_weight_skips_a_non_finite_target(scene):
    v, _, d = scene
    assert not np.isfinite(d[MM.NONFINITE]).any()
    for zero in (0.0, -0.0):
        w = MM.WEIGHTS_A.copy()
        w[MM.NONFINITE] = zero
        assert np.array_equal(bits(MM.morph_vertices(v, d, w)), bits(MM.morph_vertices(v, np.delete(d, MM.NONFINITE, 0), np.delete(w, MM.NONFINITE))))
        assert np.isfinite(MM.morph_vertices(v, d, w)).all()
    # ... where the unskipped arithmetic would not: 0 * inf and 0 * NaN are NaN
    assert not np.isfinite(MM.morph_vertices(v, d, one(MM.NONFINITE, 1e-30))[:, 0:3]).any()


def test_a_nan_weight_poisons(scene):
    v, _, d = scene
    m = MM.morph_vertices(v, d, one(MM.LIFT, np.nan))
    assert np.isnan(m[:, 0:3]).all(), "NaN != 0: applied, and NaN * 0 is NaN in the lanes whose delta is 0 as well"
    assert np.array_equal(bits(m[:, 3:8]), bits(v[:, 3:8]))


def test_negative_zero_survives_zero_weights_and_not_an_applied_zero_delta():
    base = np.array([[-0.0, -0.0, 1.0]], dtype=np.float32)
    d = np.zeros((2, 1, 3), dtype=np.float32)
    d[1, 0, 0] = np.inf
    for w in ([0.0, 0.0], [-0.0, 0.0], [0.0, -0.0]):
        p = MM._morph(base, d, np.array(w, dtype=np.float32))
        assert bits(p).tolist() == [[0x80000000, 0x80000000, 0x3F800000]], w
    p = MM._morph(base, d, np.array([1.0, 0.0], dtype=np.float32))
    assert bits(p).tolist() == [[0, 0, 0x3F800000]], "-0 + 1 * (+0) = +0"


def test_a_target_and_its_negative_need_not_cancel(scene):
    """Targets 0 and 4 at equal weight: (b + d) - d is b only where b + d was exact.  What the arithmetic gives is asserted."""
    v, _, d = scene
    assert np.array_equal(bits(d[MM.UNSWELL]), bits(-d[MM.SWELL]))
    w = one(MM.SWELL) + one(MM.UNSWELL)
    m = MM.morph_vertices(v, d, w)
    want = (v[:, 0:3] + d[MM.SWELL]) + d[MM.UNSWELL]
    assert np.array_equal(bits(m[:, 0:3]), bits(want))
    off = int((bits(m) != bits(v)).sum())
    print("components that do not cancel:", off)
    assert off == 508
    assert np.abs(m - v).max() < 1e-7


def test_normals_take_the_same_loop(swr, scene):
    v, _, d = scene
    a = swr.scenes.torus_attrs(48, 16)
    nd = MM.normal_targets(v.shape[0])
    m = MM.morph_attrs(a, nd, MM.WEIGHTS_B)
    assert np.array_equal(bits(m[:, 0:3]), bits(MM._morph(a[:, 0:3], nd, MM.WEIGHTS_B)))
    assert np.array_equal(bits(m[:, 3:8]), bits(a[:, 3:8])), "uv and the padding lanes never change"
    assert np.isfinite(m).all() and not np.array_equal(m[:, 0:3], a[:, 0:3])
    assert np.array_equal(bits(MM.morph_attrs(a, None, MM.WEIGHTS_B)), bits(a)), "without normal deltas the normals stay"
    # the same function on the same numbers as the positions
    assert np.array_equal(bits(MM.morph_attrs(v, d, MM.WEIGHTS_A)[:, 0:3]), bits(MM.morph_vertices(v, d, MM.WEIGHTS_A)[:, 0:3]))


def test_morph_then_skin_is_not_skin_then_morph(scene):
    v, _, d = scene
    j, w = SM.bend_skin(v)
    pose = SM.bend_pose()
    ms = MM.morph_then_skin(v, d, MM.WEIGHTS_A, j, w, pose)
    sm = MM.morph_vertices(SM.pose_vertices(v, j, w, pose), d, MM.WEIGHTS_A)
    assert (bits(ms) != bits(sm)).any(axis=1).sum() == 768
    assert np.abs(ms - sm).max() > 0.01


def test_the_shared_cases_are_not_vacuous(oracle, scene):
    """The floors of tests/test_morph.py: each finite target alone moves at least 1 % of the pixels (the counts are the oracle's), and
    the lifted torus has left the lowest of three 64-row bands, which the base reaches."""
    v, i, d = scene
    assert v.shape[0] == 768 and i.size == 3 * 1536 and d.shape == (5, 768, 3)
    fl = DT | oracle.TINV_PER_TRIANGLE
    c0, d0, _, code = oracle.render(v, i, KM.IDENT, MM.W, MM.H, fl)
    assert code == 0 and np.isfinite(d0).sum() == 21334
    base_rows = np.nonzero(np.isfinite(d0).any(axis=1))[0]
    assert (base_rows[0], base_rows[-1]) == (24, 168), "the base lies in all three bands"
    counts = {}
    for t in (MM.SWELL, MM.SHEAR, MM.LIFT, MM.UNSWELL):
        c1, d1, _, code = oracle.render(MM.morph_vertices(v, d, one(t)), i, KM.IDENT, MM.W, MM.H, fl)
        assert code == 0
        counts[t] = int(((c0 != c1).any(axis=-1) | (bits(d0) != bits(d1))).sum())
        if t == MM.LIFT:
            rows = np.nonzero(np.isfinite(d1).any(axis=1))[0]
            print("lifted rows", int(rows[0]), int(rows[-1]))
            assert rows.size > 30 and rows[-1] < 128 <= base_rows[-1], "the lifted torus lies in bands 0 and 1 only"
    print("pixels moved", counts)
    assert counts == {MM.SWELL: 29829, MM.SHEAR: 13183, MM.LIFT: 30697, MM.UNSWELL: 21334}
    assert min(counts.values()) >= PIXELS // 100 + 1
    for wts in (MM.WEIGHTS_A, MM.WEIGHTS_B):
        c1, d1, _, code = oracle.render(MM.morph_vertices(v, d, wts), i, KM.IDENT, MM.W, MM.H, fl)
        assert code == 0 and np.isfinite(d1).sum() > 10000 and (c0 != c1).any(axis=-1).sum() > 10000
