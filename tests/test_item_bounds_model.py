"""The numpy model of the item bounds (tests/item_bounds_model.py) against answers worked out by hand from include/swr.h "Item bounds".
CPU only."""
import numpy as np

import item_bounds_model as M

IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


def verts(*xyz):
    v = np.zeros((len(xyz), 8), dtype=np.float32)
    v[:, 0:3] = np.asarray(xyz, dtype=np.float32)
    return v


def ndc(px, size):
    """the NDC coordinate whose screen coordinate is exactly px (px / size * 2 - 1 is exact for these sizes)"""
    return px / size * 2.0 - 1.0


def test_the_culling_example_triangle():
    # NDC (-0.5,-0.5), (0.5,-0.5), (0,0.5) at 64 x 64 through the identity: pixels (16,48), (48,48), (32,16)
    v = verts((-0.5, -0.5, 0.25), (0.5, -0.5, 0.5), (0.0, 0.5, 0.75))
    idx = np.array([0, 1, 2], dtype=np.int64)
    sx, sy, sz, w = M.corners(v[:, 0:3], IDENTITY, 64, 64, False)
    assert sx.tolist() == [16, 48, 32] and sy.tolist() == [48, 48, 16] and sz.tolist() == [0.25, 0.5, 0.75] and w.tolist() == [1, 1, 1]
    for flags in (0, M.FLAG_METAL_RULES):
        b = M.item_bound(v, idx, 0, 3, IDENTITY, 64, 64, flags)
        assert (b["x0"], b["y0"], b["x1"], b["y1"]) == (16, 16, 49, 49)
        assert (b["zmin"], b["zmax"]) == (0.25, 0.75)
        assert (b["drawable"], b["skipped"], b["behind"]) == (1, 0, 0) and not b["reserved"].any()


def test_truncation_toward_zero_and_the_metal_rules():
    # sx = -0.5 truncates to 0 under the CPU rules; under the Metal rules roundf(-0.5) = -1 < 0 and the triangle is skipped
    v = verts((ndc(-0.5, 64), ndc(10, 64) * -1, 0.5), (ndc(20, 64), ndc(10, 64) * -1, 0.5), (ndc(20, 64), ndc(30.5, 64) * -1, 0.5))
    idx = np.array([0, 1, 2], dtype=np.int64)
    sx, sy, _, _ = M.corners(v[:, 0:3], IDENTITY, 64, 64, False)
    assert sx.tolist() == [-0.5, 20, 20] and sy.tolist() == [10, 10, 30.5]
    b = M.item_bound(v, idx, 0, 3, IDENTITY, 64, 64, 0)
    assert (b["x0"], b["y0"], b["x1"], b["y1"], b["drawable"]) == (0, 10, 21, 31, 1)
    m = M.item_bound(v, idx, 0, 3, IDENTITY, 64, 64, M.FLAG_METAL_RULES)
    assert (m["drawable"], m["skipped"]) == (0, 1) and (m["x0"], m["y0"], m["x1"], m["y1"]) == (0, 0, 0, 0)
    assert np.isposinf(m["zmin"]) and np.isneginf(m["zmax"])
    # half away from zero: 30.5 -> 31, 2.5 -> 3, -2.5 -> -3, and large values stay
    assert M.roundf(np.float32([30.5, 2.5, -2.5, 0.49999997, 8388609.0, -0.0])).tolist() == [31, 3, -3, 0, 8388609.0, -0.0]
    v[0, 0] = ndc(0.5, 64)
    m = M.item_bound(v, idx, 0, 3, IDENTITY, 64, 64, M.FLAG_METAL_RULES)
    assert (m["x0"], m["y0"], m["x1"], m["y1"], m["drawable"]) == (1, 10, 21, 32, 1)     # 0.5 -> 1, 30.5 -> 31


def test_a_nan_vertex_skips_its_triangle_only():
    v = verts((-0.5, -0.5, 0.25), (0.5, -0.5, 0.5), (0.0, 0.5, 0.75), (np.nan, 0.0, 0.1), (0.9, 0.9, -0.9))
    idx = np.array([0, 1, 2, 0, 3, 4, 2, 1, 0], dtype=np.int64)
    b = M.item_bound(v, idx, 0, 9, IDENTITY, 64, 64, 0)
    assert (b["drawable"], b["skipped"], b["behind"]) == (2, 1, 0)
    assert (b["x0"], b["y0"], b["x1"], b["y1"]) == (16, 16, 49, 49) and (b["zmin"], b["zmax"]) == (0.25, 0.75)
    # a NaN z coordinate makes w NaN too (0 * NaN), and the triangle is skipped like the one above
    v[3] = (0.0, 0.0, np.nan, 0, 0, 0, 0, 0)
    assert M.item_bound(v, idx, 0, 9, IDENTITY, 64, 64, 0).tobytes() == b.tobytes()
    # a NaN sz alone (inf - inf in the z row, x = y: the row (3e38, -3e38, 1, 0) cancels below the overflow) is left out by the
    # fold, and the triangle, collinear as it is, stays drawable
    m = np.eye(4, dtype=np.float32)
    m[0, 2], m[1, 2] = 3e38, -3e38
    t = verts((0.25, 0.25, 0.1), (0.5, 0.5, 0.2), (1.5, 1.5, 0.3))
    sx, sy, sz, w = M.corners(t[:, 0:3], m.reshape(16), 64, 64, False)
    assert sz[:2].tolist() == [np.float32(0.1), np.float32(0.2)] and np.isnan(sz[2]) and sx.tolist() == [40, 48, 80] and (w == 1).all()
    b = M.item_bound(t, idx, 0, 3, m.reshape(16), 64, 64, 0)
    assert (b["drawable"], b["skipped"]) == (1, 0) and (b["zmin"], b["zmax"]) == (np.float32(0.1), np.float32(0.2))
    assert (b["x0"], b["x1"], b["y0"], b["y1"]) == (40, 64, 0, 25)
    # 2^30 is not below 2^30
    v[3] = (ndc(2.0 ** 30, 64), 0.0, 0.0, 0, 0, 0, 0, 0)
    assert M.corners(v[3:4, 0:3], IDENTITY, 64, 64, False)[0][0] == 2.0 ** 30
    assert M.item_bound(v, idx, 3, 3, IDENTITY, 64, 64, 0)["skipped"] == 1


def test_a_negative_zero_depth_comes_back_positive():
    # (through the identity 0*x + 0*y + 1*(-0) + 0*1 is +0 already: a sum is -0 only if every term is, so the z row is (-0, -0, 1, -0)
    # and x, y are positive)
    m = np.eye(4, dtype=np.float32)
    m[0, 2] = m[1, 2] = m[3, 2] = -0.0
    m = m.reshape(16)
    v = verts((0.25, 0.25, -0.0), (0.5, 0.25, -0.0), (0.25, 0.5, -0.0))
    idx = np.array([0, 1, 2], dtype=np.int64)
    sz = M.corners(v[:, 0:3], m, 64, 64, False)[2]
    assert np.signbit(sz).all() and (sz == 0).all()
    b = M.item_bound(v, idx, 0, 3, m, 64, 64, 0)
    assert b["zmin"] == 0 and b["zmax"] == 0 and not np.signbit(b["zmin"]) and not np.signbit(b["zmax"])


def test_an_item_right_of_the_target_is_empty_at_the_edge():
    v = verts((1.5, -0.5, 0.5), (2.5, -0.5, 0.5), (2.0, 0.5, 0.5))
    idx = np.array([0, 1, 2], dtype=np.int64)
    b = M.item_bound(v, idx, 0, 3, IDENTITY, 64, 48, 0)
    assert b["x0"] == b["x1"] == 64 and (b["y0"], b["y1"]) == (12, 37) and b["drawable"] == 1
    # ... and above it: negative sy clamps to 0
    v[:, 1] += 3.0
    b = M.item_bound(v, idx, 0, 3, IDENTITY, 64, 48, 0)
    assert b["y0"] == b["y1"] == 0


def test_behind_and_the_empty_item():
    # w = -z: the corner at z = +1 has w = -1 and mirrors through the eye; the triangle is drawable and counted as behind
    m = np.eye(4, dtype=np.float32)
    m[2, 3] = -1.0                          # column 2, row 3 (w)
    m[3, 3] = 0.0
    v = verts((0.1, 0.1, -1.0), (0.2, 0.1, -1.0), (0.1, 0.2, 1.0))
    idx = np.array([0, 1, 2], dtype=np.int64)
    b = M.item_bound(v, idx, 0, 3, m.reshape(16), 64, 64, 0)
    assert (b["drawable"], b["skipped"], b["behind"]) == (1, 0, 1)
    e = M.item_bound(v, idx, 3, 0, IDENTITY, 64, 64, 0)
    assert (e["drawable"], e["skipped"], e["behind"], e["x0"], e["x1"], e["y0"], e["y1"]) == (0, 0, 0, 0, 0, 0, 0)
    assert np.isposinf(e["zmin"]) and np.isneginf(e["zmax"])
    both = M.item_bounds(v, idx, [(0, 3, m.reshape(16)), (3, 0, IDENTITY)], 64, 64)
    assert M.same(both, np.stack([b, e])) and not M.same(both, both[::-1])
