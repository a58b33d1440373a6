"""The design of tests/coord_edge.py, pinned on the CPU through oracle.project and the oracle's frames alone: every far triangle falls
in its class, triangles_skipped is the skip rule's count, every drawn far class wins pixels under the z-test and under painter's
order, some far triangle shows in every tile, and every skipped triangle would have covered the target with its offending corner
pulled just inside the limit.

The expected IDs come from the colour-coded copies of kernel_matrix.expected_ids, unchanged: a far triangle's float weights are
coarse, but w2 = 1 - w0 - w1 keeps their sum within a few ulps of one, and the odd code values absorb that.  Only the class g span
(NaN weights) has no decodable colour: under painter's order its pixels are LIVE, under the z-test its NaN depth never wins."""
import numpy as np
import pytest

import coord_edge as CE
import kernel_matrix as K
import test_coord_edge as T          # (its rows and scenes; importing it needs no GPU)

NAMES = ("wide", "tall")
L = CE.LIMIT
DECADES = [2.0 ** 17, 2.0 ** 20, 2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 27, 0.75 * L]


def corners(oracle, fs, name, tri, metal=False):
    """Screen (x, y) [3, 2] of a triangle in float64 (Metal rules: rounded half away from zero)."""
    w, h = CE.TARGETS[name]
    sx, sy, _ = oracle.project(fs.vertices[3 * tri:3 * tri + 3], K.IDENT, w, h)
    p = np.stack([sx, sy], axis=1).astype(np.float64)
    if metal:
        with np.errstate(invalid="ignore"):
            p = np.sign(p) * np.floor(np.abs(p) + 0.5)
    return p


def inside(p, q):
    """q strictly inside the triangle p (float64; the coordinates are integers below 2^31 or small, the products exact enough)."""
    s = [(p[(k + 1) % 3, 0] - p[k, 0]) * (q[1] - p[k, 1]) - (p[(k + 1) % 3, 1] - p[k, 1]) * (q[0] - p[k, 0]) for k in range(3)]
    return all(v > 0 for v in s) or all(v < 0 for v in s)


def on_target(p, w, h):
    return (p[:, 0] >= 0) & (p[:, 0] < w) & (p[:, 1] >= 0) & (p[:, 1] < h)


def drawable(p, metal=False):
    with np.errstate(invalid="ignore"):
        ok = (np.abs(p) < L).all()
        return bool(ok and (not metal or (p >= 0).all()))


def alone(oracle, fs, name, tri, flags=0, vertices=None):
    """Pixels the triangle covers drawn alone."""
    w, h = CE.TARGETS[name]
    v = fs.vertices[3 * tri:3 * tri + 3] if vertices is None else vertices
    c, _ = K.oracle_clear(oracle, v, np.arange(3), K.IDENT, w, h, flags)
    return int((c[..., 3] == 255).sum())


@pytest.mark.parametrize("name", NAMES)
def test_reachable_limits(oracle, name):
    """On the power-of-two axis 2^30 - 64 and -(2^30 - 128) are the last screen coordinates inside the limit, and +-2^30 are reachable."""
    w, h = CE.TARGETS[name]
    size, flip = (w, False) if w == 256 else (h, True)
    for p, mode, want in ((CE.BELOW, "inside", L - 64), (-CE.BELOW, "inside", -(L - 128)), (L, "exact", L), (-L, "exact", -L),
                          (L + 64, "beyond", L + 128)):
        n = CE.ndc_for(p, size, flip, mode)
        v = np.zeros((1, 8), np.float32)
        v[0, 1 if flip else 0] = n
        sx, sy, _ = oracle.project(v, K.IDENT, w, h)
        assert float((sy if flip else sx)[0]) == want, (p, mode)


@pytest.mark.parametrize("name", NAMES)
def test_classes(oracle, name):
    w, h = CE.TARGETS[name]
    fs = CE.edge_set(name)
    assert fs.far.size <= 40 and fs.triangles - fs.far.size == CE.N_SOUP
    assert sorted(set(fs.cls)) == list("abcdefgh")
    assert (np.diff(fs.far) > 1).all() and fs.far[0] > 0 and fs.far[-1] < fs.triangles - 1, "far and small triangles alternate in index order"
    big = CE.max_coordinate(oracle, fs.vertices, fs.indices, K.IDENT, w, h)
    small = np.setdiff1d(np.arange(fs.triangles), fs.far)
    assert big[small].max() < 2 * max(w, h), "the small triangles are ordinary"
    pow_axis = 0 if w == 256 else 1
    corners4 = [(0.0, 0.0), (w, 0.0), (0.0, h), (w, h)]
    decades, full_c = [], 0
    exact = {"+": 0, "-": 0, "beyond": 0, "huge": 0}
    for cls, tri in zip(fs.cls, fs.far):
        p = corners(oracle, fs, name, tri)
        far = np.abs(p).max(axis=1) >= L - 128
        if cls == "a":
            assert drawable(p) and far.sum() == 1 and on_target(p[~far], w, h).all(), (cls, tri, p)
        elif cls in "bh":
            assert drawable(p) and not on_target(p, w, h).any() and (np.abs(p).max(axis=1) >= 0.5 * L).all(), (cls, tri, p)
            assert all(inside(p, q) for q in corners4), (cls, tri, p)
            assert len({(np.sign(a), np.sign(b)) for a, b in p}) == 3, "three different sides"
        elif cls == "c":
            ix = np.trunc(p).astype(np.int64)
            ext = ix.max(axis=0) - ix.min(axis=0)
            assert drawable(p) and ext.min() >= (1 << 31) - 512, (tri, ext)
            full_c += int(ext[pow_axis] == (1 << 31) - 192)          # from -(2^30 - 128) to 2^30 - 64
        elif cls == "d":
            assert drawable(p) and on_target(p, w, h).sum() == 1, (tri, p)
            decades.append(float(np.abs(p).max()))
            assert (np.abs(p[~on_target(p, w, h)]).max(axis=1) == decades[-1]).all(), "both far corners at the decade"
        elif cls == "e":
            assert not drawable(p), (tri, p)
            bad = np.abs(p)[~(np.abs(p) < L)]
            assert bad.size == 1, "one offending coordinate"
            v = float(p.reshape(-1)[np.argmax(~(np.abs(p.reshape(-1)) < L))])
            exact["+" if v == L else "-" if v == -L else "beyond" if abs(v) == L + 128 else "huge" if abs(v) > 1e38 else "?"] += 1
        elif cls == "f":
            assert drawable(p) and alone(oracle, fs, name, tri) == 0, (tri, p)
        elif cls == "g":
            ix = np.trunc(p).astype(np.int64)
            area = (ix[1, 0] - ix[0, 0]) * (ix[2, 1] - ix[0, 1]) - (ix[2, 0] - ix[0, 0]) * (ix[1, 1] - ix[0, 1])
            assert drawable(p) and area == 0 and ix[:, 0].max() - ix[:, 0].min() >= (1 << 31) - 512, (tri, ix)
    assert decades == DECADES + [0.75 * L], decades
    assert full_c >= 1
    assert exact == {"+": 1, "-": 1, "beyond": 2, "huge": 1}, exact
    # f: the box of the first meets the target, the box of the second misses it
    f = [corners(oracle, fs, name, t) for t in fs.of("f")]
    meets = [bool(p[:, 0].min() < w and p[:, 0].max() >= 0 and p[:, 1].min() < h and p[:, 1].max() >= 0) for p in f]
    assert meets == [True, False]
    # h: the same positions as its original, other colours
    a, b = fs.twin
    assert fs.cls[list(fs.far).index(a)] == "b" and fs.cls[list(fs.far).index(b)] == "h" and b > a
    assert np.array_equal(fs.vertices[3 * a:3 * a + 3, :3], fs.vertices[3 * b:3 * b + 3, :3])
    assert not np.array_equal(fs.vertices[3 * a:3 * a + 3, 4:7], fs.vertices[3 * b:3 * b + 3, 4:7])
    # c: both windings, so every cull setting drops one and keeps one
    areas = K.signed_areas(oracle, fs.vertices, fs.indices, K.IDENT, w, h, 0)
    assert sorted(np.sign(areas[fs.of("c")])) == [-1, 1] and np.abs(areas[fs.of("c")]).min() > 2.0 ** 61


@pytest.mark.parametrize("name", NAMES)
def test_metal_classes(oracle, name):
    w, h = CE.TARGETS[name]
    fs = CE.metal_set(name)
    assert sorted(set(fs.cls)) == list("abcdefghnz") and fs.far.size <= 40
    decades = []
    for cls, tri in zip(fs.cls, fs.far):
        p = corners(oracle, fs, name, tri, metal=True)
        if cls in "abcdh":
            assert drawable(p, True) and p.min() > 0 and np.abs(p).max() >= 2.0 ** 17, (cls, tri, p)
        if cls in "bh":
            assert (p.min(axis=0) <= 3).all() and all(inside(p, q) for q in [(12.0, 12.0), (w, 12.0), (12.0, h), (w, h)]), (tri, p)
        if cls == "c":
            ext = p.max(axis=0) - p.min(axis=0)
            assert ext.min() >= L - 512, (tri, ext)
        if cls == "d":
            decades.append(float(p.max()))
        if cls == "e":
            assert not drawable(p, True) and (p >= 0).all()
        if cls == "z":
            assert drawable(p, True) and p.min() == 0, (tri, p)
        if cls == "n":
            assert p.min() < 0 and (np.abs(p) < L).all(), (tri, p)
        if cls == "g":
            assert drawable(p, True) and p.min() > 0 and np.unique(p[:, 1]).size == 1
    assert decades == DECADES, decades
    a, b = fs.twin
    assert np.array_equal(fs.vertices[3 * a:3 * a + 3, :3], fs.vertices[3 * b:3 * b + 3, :3]) and b > a


def skip_model(oracle, fs, name, metal):
    """The skip rule's count over a set, from oracle.project: a coordinate that is not inside the limit; under the Metal rules the
    rounded coordinates, a negative one, and a bounding box that starts at 0 (the ROI skip)."""
    n = 0
    for t in range(fs.triangles):
        p = corners(oracle, fs, name, t, metal)
        n += (not drawable(p, metal)) or bool(metal and p.min() == 0)
    return n


@pytest.mark.parametrize("name", NAMES)
def test_skipped_counts(oracle, name):
    w, h = CE.TARGETS[name]
    fs = CE.edge_set(name)
    for flags in (0, K.DT):
        st = oracle.render(fs.vertices, fs.indices, K.IDENT, w, h, flags | oracle.TINV_PER_TRIANGLE)[2]
        assert st.triangles_skipped == skip_model(oracle, fs, name, False) == fs.cls.count("e") == 5
    ms = CE.metal_set(name)
    st = oracle.render_metal(ms.vertices, ms.indices, K.IDENT, w, h, 0)[2]
    far_skipped = sum(ms.cls.count(c) for c in "ezn")
    assert st.triangles_skipped == skip_model(oracle, ms, name, True) >= far_skipped == 6


# pixels the oracle's frame shows of every triangle of a class at least (z-test; the Metal rules test depth too), of every class in
# all (painter's order: a triangle with the target strictly inside hides what came before it, so the class b triangles show through
# their duplicate, class h, which wins the tie as the later one; the class g span has no decodable colour: LIVE pixels)
Z_EACH = 20
Z_CLASS = {"a": 9000, "b": 1000, "c": 3000, "d": 20000}
PAINTER_CLASS = {"a": 15000, "h": 200, "c": 1000, "d": 15000}


@pytest.mark.parametrize("name", NAMES)
def test_far_classes_win_pixels(oracle, name):
    w, h = CE.TARGETS[name]
    for fs, flags in ((CE.edge_set(name), K.DT), (CE.metal_set(name), K.METAL), (CE.edge_set(name), 0)):
        rid = CE.frame_ids(oracle, fs, name, flags)
        n = CE.shown(rid, fs.triangles)
        what = f"{name}, flags {flags}: {dict(zip([f'{c}{t}' for c, t in zip(fs.cls, fs.far)], n[fs.far]))}"
        if flags:
            assert (n[fs.of("abcd")] >= Z_EACH).all(), what
            for cls, floor in Z_CLASS.items():
                assert n[fs.of(cls)].sum() >= floor // (2 if flags & K.METAL and cls in "ac" else 1), what
            assert n[fs.of("h")].sum() == 0 and n[fs.twin[0]] >= 200, "the tie goes to the earlier triangle: " + what
            assert (rid != K.LIVE).all()
        else:
            for cls, floor in PAINTER_CLASS.items():
                assert n[fs.of(cls)].sum() >= floor, what
            assert n[fs.of("b")].sum() == 0, "the tie goes to the later triangle: " + what
            assert (rid[int(0.37 * h)] == K.LIVE).sum() >= 100, "the class g span, one row: " + what
        assert n[fs.of("efzn")].sum() == 0, what
        # some far triangle shows in every tile
        far = np.isin(rid, fs.far)
        for ty in range(0, h, K.TILE_H):
            for tx in range(0, w, K.TILE_W):
                assert far[ty:ty + K.TILE_H, tx:tx + K.TILE_W].sum() >= 100, f"tile ({tx}, {ty}): {what}"
        # ... and the small triangles fight them
        assert n[np.setdiff1d(np.arange(fs.triangles), fs.far)].sum() >= 3000, what


@pytest.mark.parametrize("name", NAMES)
def test_skipped_triangles_would_have_shown(oracle, name):
    """Each skipped triangle drawn alone covers nothing; with its offending coordinate pulled just inside the limit (Metal rules:
    the zero or negative one to 2) it covers most of the target."""
    w, h = CE.TARGETS[name]
    for fs, flags, letters in ((CE.edge_set(name), 0, "e"), (CE.metal_set(name), K.METAL, "ezn")):
        for tri in fs.of(letters):
            assert alone(oracle, fs, name, tri, flags) == 0
            p = corners(oracle, fs, name, tri, bool(flags))
            v = fs.vertices[3 * tri:3 * tri + 3].copy()
            for k in range(3):
                for axis, size in ((0, w), (1, h)):
                    s = p[k, axis]
                    if not abs(s) < L:
                        v[k, axis] = CE.ndc_for(np.sign(s) * CE.BELOW, size, axis == 1)
                    elif flags and s <= 0:
                        v[k, axis] = CE.ndc_for(2.0, size, axis == 1)
            assert alone(oracle, fs, name, tri, flags, v) >= w * h // 2, (name, flags, tri)


@pytest.mark.parametrize("name", NAMES)
def test_perspective_variant(oracle, name):
    w, h = CE.TARGETS[name]
    fs = CE.perspective_set(oracle, name)
    m = K.perspective_matrix()
    big = CE.max_coordinate(oracle, fs.vertices, fs.indices, m, w, h)
    p, q = fs.of("p"), fs.of("q")
    assert ((big[p] >= 2.0 ** 29) & (big[p] < L)).sum() >= 3 and p.size >= 3
    assert ((big[q] >= L) & (big[q] < 2.0 ** 31)).sum() >= 3 and q.size >= 3
    st = oracle.render(fs.vertices, fs.indices, m, w, h, K.DT | oracle.TINV_PER_TRIANGLE)[2]
    assert st.triangles_skipped == q.size
    n = CE.shown(CE.frame_ids(oracle, fs, name, K.DT, m, key="persp"), fs.triangles)
    assert (n[p] > 0).sum() >= 3 and n[p].sum() >= 300 and n[q].sum() == 0, n[fs.far]


@pytest.mark.parametrize("name", NAMES)
def test_points_and_lines(oracle, name):
    """The point and line scenes: through oracle.project the lines have the steps meant, and the oracle's real-line frame draws the
    2^20-step line across the target and not the one of 2^20 + 1 steps."""
    w, h = CE.TARGETS[name]
    v, i = CE.line_scene(name)
    sx, sy, _ = oracle.project(v, K.IDENT, w, h)
    ix, iy = np.trunc(sx.astype(np.float64)), np.trunc(sy.astype(np.float64))
    steps = np.maximum(np.abs(ix[1::2] - ix[0::2]), np.abs(iy[1::2] - iy[0::2]))
    S = float(1 << 20)
    assert list(steps[:3]) == [S, S + 1, S] and steps[4] == S and steps[6] == S and steps[7] == S, steps
    long_axis = sx if w == 256 else sy
    assert long_axis[4] > 2.0 ** 24 and long_axis[6] == L and long_axis[8] == L - 64
    per_line = []
    for k in range(8):
        c = oracle.render(v, i[2 * k:2 * k + 2], K.IDENT, w, h, CE.REAL_LINES, primitive_type=1)[0]
        per_line.append(int((c[..., 3] == 255).sum()))
    assert per_line[0] >= 100 and per_line[1] == 0 and per_line[3] == 0 and per_line[5] >= 100 and per_line[7] >= 100, per_line
    assert per_line[6] >= 100, per_line
    pv, pi = CE.point_scene(name)
    c, _, st, code = oracle.render(pv, pi, K.IDENT, w, h, 0, primitive_type=2)
    assert code == 0 and st.triangles_skipped == 5 and (c[..., 3] == 255).sum() >= 250


def test_class_c_is_culled_by_some_rows_and_kept_by_others(oracle):
    """On the CPU, from K.signed_areas: over the binning rows with cull bits, each class c triangle (areas of +-2^62) is dropped by one
    row and kept by another under the CPU rules; under the Metal rules the rows' cull bits all drop the same winding, so there each row
    drops one of the two class c triangles and keeps the other."""
    for name in NAMES:
        w, h = CE.TARGETS[name]
        kept, rows = {}, 0
        for row in T.BIN_ROWS:
            if not row.affine or not row.flags & (K.CB | K.CF):
                continue
            fs, m, items = T.bin_scene(oracle, row, name)
            v, i, mm = (*K.concat(fs.vertices, fs.indices, items), K.IDENT) if row.draw_list else (fs.vertices, fs.indices, m)
            keep = K.kept_triangles(K.signed_areas(oracle, v, i, mm, w, h, row.flags), row.flags)
            here = [bool(np.isin(t, keep)) for t in fs.of("c")]            # (the first item holds them under their own numbers)
            assert sorted(here) == [False, True], (row.name, here)
            rows += 1
            for t, k in zip(fs.of("c"), here):
                kept.setdefault((bool(row.flags & K.METAL), int(t)), set()).add(k)
        assert rows >= 4 and len(kept) == 4, kept
        assert all(v == {True, False} for (metal, _), v in kept.items() if not metal), kept
