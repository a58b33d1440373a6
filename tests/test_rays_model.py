"""tests/rays_model.py against hand-computed cases of include/swr.h "Ray casts", and the property the group cull of swr_rays.hip rests
on: the box pre-test never rejects an enclosing box when it passes the triangle's own.  CPU only."""
import numpy as np

import rays_model as R

F = np.float32
NONE = R.ID_NONE

# legs of 4 along x and y in the plane z = 0: det = +-16 for a ray along z, so every quotient below is exact
A, B, C = (0, 0, 0), (4, 0, 0), (0, 4, 0)
TRI = np.array([[A, B, C]], dtype=np.float32)
DOWN, UP = (0, 0, -1), (0, 0, 1)


def one(tri, *ray):
    return R.cast(tri, R.rays([ray]))[0]


def is_miss(h):
    return h["primitive"] == NONE and h["t"].tobytes() == h["u"].tobytes() == h["v"].tobytes() == F(0).tobytes()


def test_dtypes_are_the_header_structs():
    assert R.RAY_DTYPE.itemsize == 32 and R.HIT_DTYPE.itemsize == 16
    assert [R.RAY_DTYPE.fields[n][1] for n in ("origin", "tmin", "dir", "tmax")] == [0, 12, 16, 28]
    assert [R.HIT_DTYPE.fields[n][1] for n in ("primitive", "t", "u", "v")] == [0, 4, 8, 12]


def test_exact_hit():
    h = one(TRI, (1, 1, 2), DOWN)
    # pv = (4, 0, 0), det = 16, tv = (1, 1, 2), u = 4 / 16; qv = (0, 8, -4), v = 4 / 16, t = 32 / 16
    assert (h["primitive"], h["t"], h["u"], h["v"]) == (0, F(2), F(0.25), F(0.25))
    # the other facing is hit too: pv = (-4, 0, 0), det = -16
    h = one(TRI, (1, 1, -2), UP)
    assert (h["primitive"], h["t"], h["u"], h["v"]) == (0, F(2), F(0.25), F(0.25))


def test_unit_triangle_at_its_centroid():
    tri = np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]], dtype=np.float32)
    third = F(1) / F(3)
    h = one(tri, (third, third, 1), DOWN)
    # pv = (1, 0, 0), det = 1, inv = 1: u = tv.x = fl(1/3), v = tv.y = fl(1/3), t = tv.z = 1, all exact
    assert (h["primitive"], h["t"], h["u"], h["v"]) == (0, F(1), third, third)
    o = np.array([third, third, 1], dtype=np.float32) + h["t"] * np.array(DOWN, dtype=np.float32)
    assert np.array_equal(o, (F(1) - h["u"] - h["v"]) * tri[0, 0] + h["u"] * tri[0, 1] + h["v"] * tri[0, 2])


def test_t_exactly_tmin_and_exactly_tmax():
    assert one(TRI, (1, 1, 2), DOWN, 2.0, 5.0)["primitive"] == 0
    assert one(TRI, (1, 1, 2), DOWN, 0.0, 2.0)["primitive"] == 0
    assert one(TRI, (1, 1, 2), DOWN, 2.0, 2.0)["primitive"] == 0            # tmin == tmax
    assert is_miss(one(TRI, (1, 1, 2), DOWN, np.nextafter(F(2), F(3)), 5.0))
    assert is_miss(one(TRI, (1, 1, 2), DOWN, 0.0, np.nextafter(F(2), F(1))))
    # a negative tmin reaches behind the origin
    h = one(TRI, (1, 1, -2), DOWN, -3.0, 0.0)
    assert h["primitive"] == 0 and h["t"] == F(-2)


def test_ray_starting_on_the_triangle_gives_plus_zero():
    for d in (DOWN, UP):            # (UP: inv = -1/16 and dot(e2, qv) = +0 give -0, which the + 0.0f turns into +0)
        h = one(TRI, (1, 1, 0), d, 0.0, 1.0)
        assert h["primitive"] == 0 and h["t"].tobytes() == F(0).tobytes(), d
        assert (h["u"], h["v"]) == (F(0.25), F(0.25))


def test_coincident_triangles_the_lower_primitive_wins():
    far = TRI + np.array([0, 0, -1], dtype=np.float32)
    tri = np.concatenate([far, TRI, TRI, far])
    h = one(tri, (1, 1, 2), DOWN)
    assert (h["primitive"], h["t"]) == (1, F(2))
    h = one(tri[::-1], (1, 1, 2), DOWN)     # slots 1 and 2 again
    assert (h["primitive"], h["t"]) == (1, F(2))


def test_degenerate_triangle_and_nan_corner():
    line = np.array([[A, A, C]], dtype=np.float32)
    assert is_miss(one(line, (0, 1, 2), DOWN))
    edge_on = np.array([[(0, 0, 0), (4, 0, 0), (0, 0, 4)]], dtype=np.float32)      # the ray lies in the triangle's plane: det = 0
    assert is_miss(one(edge_on, (1, 0, 2), DOWN))
    for bad in (np.nan, np.inf, -np.inf):
        for corner in range(3):
            for axis in range(3):
                t = TRI.copy()
                t[0, corner, axis] = bad
                both = np.concatenate([t, TRI + np.array([0, 0, -1], dtype=np.float32)])
                assert is_miss(one(t, (1, 1, 2), DOWN)), (bad, corner, axis)
                h = one(both, (1, 1, 2), DOWN)
                assert (h["primitive"], h["t"]) == (1, F(3)), (bad, corner, axis)


def test_axis_parallel_ray_with_the_origin_on_the_box_face():
    h = one(TRI, (0, 1, 2), DOWN)           # x and y are parallel axes; origin.x == lo.x
    assert (h["primitive"], h["t"], h["u"], h["v"]) == (0, F(2), F(0), F(0.25))
    h = one(TRI, (4, 0, 2), DOWN)           # origin.x == hi.x, origin.y == lo.y: the corner b
    assert (h["primitive"], h["u"], h["v"]) == (0, F(1), F(0))
    assert is_miss(one(TRI, (np.nextafter(F(0), F(-1)), 1, 2), DOWN))
    assert is_miss(one(TRI, (np.nextafter(F(4), F(5)), 0, 2), DOWN))
    # -0 is on the face at 0
    assert one(TRI, (-0.0, 1, 2), DOWN)["primitive"] == 0


def test_direction_component_whose_reciprocal_overflows():
    tiny = np.float32(1e-45)                # the smallest denormal: 1 / tiny = inf, so x is treated as a parallel axis
    with np.errstate(all="ignore"):
        assert np.isinf(F(1) / tiny)
    h = one(TRI, (1, 1, 2), (tiny, 0, -1))
    assert (h["primitive"], h["t"]) == (0, F(2))
    assert is_miss(one(TRI, (5, 1, 2), (tiny, 0, -1)))
    assert is_miss(one(TRI, (5, 1, 2), (-tiny, 0, -1)))
    # 2e-39 still overflows (1 / FLT_MAX is about 2.9e-39); the largest denormal does not: its axis goes through the slab arithmetic
    assert is_miss(one(TRI, (5, 1, 2), (F(2e-39), 0, -1)))
    big_denormal = np.nextafter(np.finfo(np.float32).tiny, F(0))
    assert np.isfinite(F(1) / big_denormal)
    lo, hi = TRI.min(axis=1), TRI.max(axis=1)
    assert R.pretest(R.ray((1, 1, 2), (big_denormal, 0, -1)), lo, hi)[0]
    # (from x = 5 the slab of x is reached at t = 8.5e37, the plane z = 0 at t = 2: rejected by the intervals, not by the parallel rule)
    assert not R.pretest(R.ray((5, 1, 2), (-big_denormal, 0, -1), 0.0, R.FLT_MAX), lo, hi)[0]
    tall = (np.array([[0, 0, -3e38]], dtype=np.float32), np.array([[4, 4, 0]], dtype=np.float32))
    assert R.pretest(R.ray((5, 1, 2), (-big_denormal, 0, -1), 0.0, R.FLT_MAX), *tall)[0]
    assert not R.pretest(R.ray((5, 1, 2), (big_denormal, 0, -1), 0.0, R.FLT_MAX), *tall)[0]


def test_a_scene_without_triangles_and_check_ray():
    h = R.cast(np.zeros((0, 3, 3), dtype=np.float32), R.rays([((0, 0, 1), DOWN)]))
    assert is_miss(h[0])
    assert R.check_ray(R.ray((0, 0, 0), DOWN)) is None
    assert R.check_ray(R.ray((0, 0, 0), (0, -0.0, 0))) == "zero direction"
    assert R.check_ray(R.ray((0, 0, 0), DOWN, 2.0, 1.0)) == "tmin > tmax"
    bad = R.ray((0, 0, 0), DOWN)
    bad["tmax"] = np.inf
    assert R.check_ray(bad) == "not finite"


def _specials(rng, shape):
    """Floats that stress the comparisons: zeros of both signs, denormals, small integers, ordinary values."""
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0, 2.0, 0.5, -0.5], dtype=np.float32)
    x = rng.uniform(-4, 4, shape).astype(np.float32)
    pick = rng.random(shape) < 0.35
    return np.where(pick, pool[rng.integers(0, pool.size, shape)], x).astype(np.float32)


def test_pretest_is_monotone_in_the_box():
    """Whenever the pre-test passes a triangle's own box it passes every box that encloses it: what makes the group cull exact."""
    rng = np.random.default_rng(0x7A95)
    passed = rejected = 0
    for _ in range(400):
        n = 64
        tri = _specials(rng, (n, 3, 3))
        if rng.random() < 0.3:
            tri[:, :, rng.integers(0, 3)] = _specials(rng, (n, 1))          # flat boxes: every corner in one axis-aligned plane
        lo, hi = tri.min(axis=1), tri.max(axis=1)
        grow_lo = np.where(rng.random((n, 3)) < 0.4, F(0), np.abs(_specials(rng, (n, 3))))
        grow_hi = np.where(rng.random((n, 3)) < 0.4, F(0), np.abs(_specials(rng, (n, 3))))
        with np.errstate(all="ignore"):
            blo, bhi = (lo - grow_lo).astype(np.float32), (hi + grow_hi).astype(np.float32)
        # a zero of the other sign is the same bound (fminf may return either)
        blo = np.where((blo == 0) & (rng.random((n, 3)) < 0.5), -blo, blo)
        bhi = np.where((bhi == 0) & (rng.random((n, 3)) < 0.5), -bhi, bhi)
        assert (blo <= lo).all() and (bhi >= hi).all()
        glo, ghi = lo.min(axis=0), hi.max(axis=0)                          # the box of the whole group, as box_fold builds it
        d = _specials(rng, 3)
        if (d == 0).all():
            d[rng.integers(0, 3)] = F(1)
        t = np.sort(_specials(rng, 2) * F(3))
        r = R.ray(_specials(rng, 3), d, t[0], t[1])
        own, enclosing, group = R.pretest(r, lo, hi), R.pretest(r, blo, bhi), R.pretest(r, glo[None], ghi[None])[0]
        assert not (own & ~enclosing).any()
        assert group or not own.any()
        passed += int(own.sum())
        rejected += int((~own).sum())
    assert passed > 1000 and rejected > 1000       # both outcomes are exercised


def test_group_cull_equals_brute_force():
    """cast() over only the groups whose box passes (or is poisoned) gives the brute-force hits, bit for bit."""
    rng = np.random.default_rng(0x6011)
    n = 64 * 5 + 17
    centre = rng.uniform(-3, 3, (n, 1, 3))
    tri = (centre + rng.uniform(-0.9, 0.9, (n, 3, 3))).astype(np.float32)     # (large enough that about half of the rays hit)
    tri[100, 1, 2] = np.inf                         # group 1 is poisoned
    o = rng.uniform(-4, 4, (50, 3)).astype(np.float32)
    d = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    d[::7, 0] = 0
    d[::5, 1] = -0.0
    rs = R.rays([(o[k], d[k], 0.0, 100.0) for k in range(50)])
    brute = R.cast(tri, rs)
    assert (brute["primitive"] != NONE).sum() >= 10
    groups = (n + 63) // 64
    for k, r in enumerate(rs):
        keep = np.zeros(n, dtype=bool)
        for g in range(groups):
            part = tri[64 * g:64 * g + 64].reshape(-1, 3)
            with np.errstate(all="ignore"):
                if not np.isfinite(part).all() or R.pretest(r, part.min(axis=0)[None], part.max(axis=0)[None])[0]:
                    keep[64 * g:64 * g + 64] = True
        culled = tri.copy()
        culled[~keep] = np.nan                      # a triangle that is never hit
        assert R.cast(culled, rs[k:k + 1]).tobytes() == brute[k:k + 1].tobytes()
    tested, entered, tris = R.work(tri, rs)
    assert (tested == groups).all() and (entered >= 1).all() and (entered <= groups).all() and (tris <= n).all()
