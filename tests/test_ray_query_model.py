"""tests/ray_query_model.py against hand-computed cases of include/swr.h "Ray queries", against tests/rays_model.py where the two must
agree, and the preconditions the shapes of tests/test_ray_queries.py rely on, so that none of the device's comparisons is vacuous.  CPU
only; nothing here touches the library."""
import numpy as np

import ray_query_model as Q
import rays_model as R
import test_ray_queries as D

NONE, OCC = R.ID_NONE, Q.OCCLUDED
ANY, BACK, FRONT, CW = Q.ANY_HIT, Q.CULL_BACK, Q.CULL_FRONT, Q.FRONT_CW
SMALL = D.SIZES[:-1]


def test_constants():
    assert (ANY, BACK, FRONT, CW, OCC, NONE) == (1, 2, 4, 8, 0xFFFFFFFE, 0xFFFFFFFF)
    assert Q.QUERY_DTYPE.itemsize == 24
    assert sorted(Q.CULLS + [Q.BOTH, CW | Q.BOTH]) == [0, 2, 4, 6, 8, 10, 12, 14]


def test_one_triangle_from_its_front_and_its_back():
    """TRI = (0,0,0), (4,0,0), (0,4,0): cross(b - a, c - a) = (0, 0, 16) points to +z.  The ray from z = 2 downwards arrives from that
    side: det = dot(e1, cross(dir, e2)) = dot((4,0,0), cross((0,0,-1), (0,4,0))) = dot((4,0,0), (4,0,0)) = 16 > 0, the front.  The ray
    from z = -2 upwards has det = -16."""
    rs = R.rays(D.PROBES[:2])
    assert Q.det_of(D.TRI, rs[0]).tolist() == [16.0] and Q.det_of(D.TRI, rs[1]).tolist() == [-16.0]
    for flags, hit in D.facing_cases():
        got = Q.query(D.TRI, rs, flags)
        assert (got["primitive"] != NONE).tolist() == hit, flags
        for k in range(2):
            if hit[k]:
                assert got[k].tolist() == (0, 2.0, 0.25, 0.25), (flags, k)
            else:
                assert got[k].tolist() == (NONE, 0.0, 0.0, 0.0), (flags, k)
        got = Q.query(D.TRI, rs, flags | ANY)
        assert [tuple(g) for g in got.tolist()] == [(OCC if h else NONE, 0.0, 0.0, 0.0) for h in hit], flags
    # the same triangle with the other winding: the facings swap
    flipped = D.TRI[:, ::-1]
    assert (Q.query(flipped, rs, BACK)["primitive"] != NONE).tolist() == [False, True]
    assert (Q.query(flipped, rs, CW | BACK)["primitive"] != NONE).tolist() == [True, False]


def test_both_cull_bits_give_all_misses():
    for n in SMALL:
        for flags in (Q.BOTH, CW | Q.BOTH, ANY | Q.BOTH):
            got = Q.query(D.soup(n), D.ray_set(256), flags)
            assert (got["primitive"] == NONE).all() and not got["t"].any() and not got["u"].any() and not got["v"].any()


def test_defaults_equal_the_ray_cast_model():
    for n in SMALL:
        for rays in D.RAY_COUNTS:
            want = R.cast(D.soup(n), D.ray_set(rays))
            assert Q.query(D.soup(n), D.ray_set(rays)).tobytes() == want.tobytes()
            assert Q.query(D.soup(n), D.ray_set(rays), 0, 0, n).tobytes() == want.tobytes()
            assert Q.query(D.soup(n), D.ray_set(rays), CW).tobytes() == want.tobytes(), "FRONT_CW alone culls nothing"
    assert D.expected(D.BIG, D.BIG_RAYS).tobytes() == R.cast(D.soup(D.BIG), D.ray_set(D.BIG_RAYS)).tobytes()


def test_a_range_equals_the_cast_on_the_sliced_index_array():
    for n in D.SIZES:
        rays = D.ray_counts(n)[-1]
        tri = D.soup(n)
        v, i = D.scene_of(tri)
        for first, count in D.ranges(n) + [(0, -1)]:
            begin, end = Q.resolve(n, first, count)
            want = R.cast(R.triangles(v, i[3 * begin:3 * end]), D.ray_set(rays))
            hit = want["primitive"] != NONE
            want["primitive"][hit] += begin
            assert D.expected(n, rays, 0, first, count).tobytes() == want.tobytes(), (n, first, count)


def test_any_hit_is_nearest_is_not_a_miss():
    rng = np.random.default_rng(0x51C)
    for n in SMALL:
        for rays in D.RAY_COUNTS:
            for flags in Q.CULLS + [Q.BOTH]:
                first = int(rng.integers(0, n + 1))
                count = int(rng.integers(-1, n - first + 1))
                near = Q.query(D.soup(n), D.ray_set(rays), flags, first, count)
                occ = Q.query(D.soup(n), D.ray_set(rays), flags | ANY, first, count)
                assert (Q.occluded(occ) == Q.occluded(near)).all()
                assert set(occ["primitive"].tolist()) <= {OCC, NONE} and not occ["t"].any() and not occ["u"].any() and not occ["v"].any()


def test_a_culled_face_is_rejected_before_the_winner():
    """Two coincident triangles of opposite winding: without a cull the lower number wins the tie, with one the facing decides."""
    tri = np.concatenate([D.TRI, D.TRI[:, ::-1]])
    rs = R.rays(D.PROBES[:2])
    assert Q.query(tri, rs)["primitive"].tolist() == [0, 0]
    assert Q.query(tri, rs, BACK)["primitive"].tolist() == [0, 1]
    assert Q.query(tri, rs, FRONT)["primitive"].tolist() == [1, 0]
    assert Q.query(tri, rs, BACK, 1, 1)["primitive"].tolist() == [NONE, 1]
    assert Q.query(tri, rs, ANY | BACK, 1, 1)["primitive"].tolist() == [NONE, OCC]


def test_refusals():
    refused, accepted = D.error_table(129)
    assert all(Q.check_query(129, *q) is not None for q in refused) and all(Q.check_query(129, *q) is None for q in accepted)
    assert {Q.check_query(129, *q) for q in refused} == {"unknown flags", "reserved", "first_primitive", "primitive_count", "beyond the scene"}


# ---- what the shapes on the device rely on ------------------------------------------------------------------------------------------------
def test_every_seeded_set_has_occluded_and_free_rays():
    """In every seeded set used on the device (64 rays and more; the sets of 1 and 63 rays are prefixes in kind, not in content) at
    least a quarter of the rays are occluded and at least a quarter are not."""
    for n in D.SIZES:
        for rays in D.ray_counts(n):
            if rays < D.BIG_RAYS:
                continue
            occ = Q.occluded(D.expected(n, rays, ANY))
            assert rays / 4 <= occ.sum() <= 3 * rays / 4, (n, rays, int(occ.sum()))


def test_every_cull_changes_an_answer():
    """Every cull combination except "both" that has a cull bit changes at least one answer of the largest ray set of every scene, in
    nearest mode, and FRONT_CW swaps the two culls; the lone triangle faces one way, so one of its two culls changes nothing."""
    for n in D.SIZES:
        rays = D.ray_counts(n)[-1]
        base = D.expected(n, rays)
        changed = {f: D.expected(n, rays, f).tobytes() != base.tobytes() for f in (BACK, FRONT, CW | BACK, CW | FRONT) if f in D.culls(n)}
        assert any(changed.values()) if n == 1 else all(changed.values()), (n, changed)
        if n != D.BIG:
            assert D.expected(n, rays, CW | BACK).tobytes() == D.expected(n, rays, FRONT).tobytes()
            assert D.expected(n, rays, CW | FRONT).tobytes() == D.expected(n, rays, BACK).tobytes()
            assert D.expected(n, rays, BACK).tobytes() != D.expected(n, rays, FRONT).tobytes()
    for n in D.SIZES[1:]:
        rays = D.ray_counts(n)[-1]
        assert Q.occluded(D.expected(n, rays, ANY | BACK)).sum() < Q.occluded(D.expected(n, rays, ANY)).sum(), n


def test_every_range_cuts_a_hit_away():
    for n in D.SIZES:
        rays = D.ray_counts(n)[-1]
        base = D.expected(n, rays)
        for first, count in D.ranges(n):
            begin, end = Q.resolve(n, first, count)
            want = D.expected(n, rays, 0, first, count)
            if (begin, end) == (0, n):
                assert want.tobytes() == base.tobytes()
                continue
            assert want.tobytes() != base.tobytes(), (n, first, count)
            assert begin < end or (want["primitive"] == NONE).all(), (n, first, count)
            occ = D.expected(n, rays, ANY, first, count)
            assert (Q.occluded(occ) <= Q.occluded(D.expected(n, rays, ANY))).all(), (n, first, count)
    # the one-triangle range that names the last triangle of the last, partial group is hit
    for n in (65, 129, D.BIG):
        rays = D.ray_counts(n)[-1]
        assert (D.expected(n, rays, 0, n - 1, 1)["primitive"] == n - 1).any(), n


def test_the_placed_scenes():
    want = D.placed_expected()
    last, both, every = (want[name] for name, _, _ in D.placed_cases())
    assert last[0]["primitive"].tolist() == [OCC, OCC, NONE, NONE] and last[2]["primitive"].tolist()[:2] == [2 * 64 * D.GPW - 1] * 2
    # (the third probe meets every filler triangle: for it every group occludes; the others meet the placed triangles or nothing)
    assert both[0]["primitive"].tolist() == [OCC, OCC, OCC, NONE, NONE, OCC] and both[2]["primitive"].tolist()[:3] == [0, 0, 1]
    assert every[0]["primitive"].tolist() == [OCC, OCC, NONE, NONE, NONE, OCC]
    assert every[1]["primitive"].tolist() == [OCC, NONE, NONE, NONE, NONE, OCC]
    for name, tri, _ in D.placed_cases():
        assert tri.shape[0] > 64 * D.GPW, name          # two workgroups a ray


def test_the_item_scene():
    tri, rays = D.item_scene()
    first = np.concatenate([[0], np.cumsum(D.ITEM_TRIS)])
    for k in range(3):
        for j in range(3):
            got = Q.query(tri, rays[j], 0, int(first[k]), D.ITEM_TRIS[k])
            assert (got["primitive"] != NONE).any() == (j == k), (k, j)
        # without the range the rays of an item hit that item only, whatever the range: the items are far apart
        assert Q.query(tri, rays[k]).tobytes() == Q.query(tri, rays[k], 0, int(first[k]), D.ITEM_TRIS[k]).tobytes()
