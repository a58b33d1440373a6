"""Ray queries on the GPU (swr_query_rays; include/swr.h "Ray queries"): occlusion rays, facing culls and primitive ranges
on the resident triangle stream, as it is now.

Equality is exact everywhere — the 16-byte records as bytes — and no expectation comes from the code under test: it is the brute-force
numpy float32 model of tests/ray_query_model.py (on top of tests/rays_model.py), written from the header's text, on the uploaded vertices
or on the vertices tests/skin_model.py and tests/morph_model.py produce.

Scene sizes are those of tests/test_rays.py: 1, 63, 64, 65 and 129 triangles (the 64-slot group and a partial last group) with 1, 63, 64,
65 and 256 rays, and 64 * RAYS_GROUPS_PER_WG + 65 triangles (a ray has a second workgroup, whose last group is partly filled) with 32
rays, the brute-force model taking its time there.  Every scene is queried with the stream Morton-ordered, in the caller's order and as
for 2^24 primitives (swr_debug_set, SWR_DEBUG_STREAM_ORDER).  The model's answers are computed once per (scene, rays, query) and shared
by the stream orders; tests/test_ray_query_model.py asserts, on the CPU, that none of them is vacuous."""
import functools

import numpy as np
import pytest

import kernel_matrix as K
import morph_model as MM
import ray_query_model as Q
import rays_model as R
import skin_model as SM
import test_rays as TR

gpu = pytest.mark.gpu
F = np.float32
NONE, OCC = R.ID_NONE, Q.OCCLUDED
ANY, BACK, FRONT, CW = Q.ANY_HIT, Q.CULL_BACK, Q.CULL_FRONT, Q.FRONT_CW
DT, IDS = K.DT, K.IDS
BAD_ARG, UNSUPPORTED, NO_SCENE = -1, -5, -6
ORDERS = TR.ORDERS
SIZES = TR.SIZES
BIG = SIZES[-1]
RAY_COUNTS = [1, 63, 64, 65, 256]
BIG_RAYS = 32
GPW = TR.groups_per_wg()
scene_of, check, resident = TR.scene_of, TR.check, TR.resident


# ---- scenes, rays, queries ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup(n):
    """n triangles of either winding with centres in [-0.8, 0.8]^2 x [-0.5, 0.5], large enough that the rays of ray_set(…) from above
    are occluded about half of the time at every size.  One triangle alone covers half of the rays' square.  From 65 triangles on,
    triangle 1 is a large one near the top and the last triangle repeats it with the other winding (the one-triangle range that names
    the last slot of the last, partial group has something to hit), and triangle 40 has an infinite corner (its group's box is
    poisoned)."""
    rng = np.random.default_rng(0x51A + n)
    half = min(0.9, max(0.022, 3.0 / np.sqrt(n)))
    c = np.concatenate([rng.uniform(-0.8, 0.8, (n, 1, 2)), rng.uniform(-0.5, 0.5, (n, 1, 1))], axis=-1)
    tri = (c + rng.uniform(-half, half, (n, 3, 3)) * np.array([1, 1, 0.3])).astype(np.float32)
    if n == 1:
        tri[0] = [(-0.9, -0.9, 0.1), (0.9, -0.9, 0.0), (0.0, 0.9, -0.1)]
    if n >= 65:
        tri[1] = [(-0.5, -0.5, 0.45), (0.5, -0.4, 0.45), (0.0, 0.5, 0.45)]
        tri[n - 1] = tri[1][::-1]
        tri[40, 2, 1] = np.inf
    tri.setflags(write=False)
    return tri


def ray_set(n):
    return TR.ray_set(n, seed=0x51B)


def ray_counts(n):
    return [BIG_RAYS] if n == BIG else RAY_COUNTS


def ranges(n):
    """(first, count) of the ranges a scene of n triangles is queried with, the whole scene left out."""
    if n == 129:
        return [(10, 40), (60, 10), (64, 64), (0, 0), (129, 0), (50, 0), (128, 1), (0, 129)]
    if n == BIG:
        return [(64 * GPW - 3, 40), (BIG - 1, 1)]       # across the two workgroups' chunks; the last slot of the second chunk
    if n == 65:
        return [(64, 1), (0, 64), (3, 30)]
    if n == 1:
        return [(0, 0), (1, 0), (0, 1)]
    return [(n // 3, n // 3), (n - 1, 1), (n // 2, 0)]


def culls(n):
    """The flag words of the nearest-mode cull tests: every combination, at every size."""
    return Q.CULLS + [Q.BOTH]


def combined(n):
    """(flags, first, count) of the any-hit queries that also cull and restrict."""
    first, count = ranges(n)[0]
    return [(ANY | BACK, 0, -1), (ANY | CW | BACK, first, count), (ANY | FRONT, first, count), (ANY | Q.BOTH, 0, -1)]


@functools.lru_cache(maxsize=None)
def model_steps(n_tri, n_rays):
    """Steps 1 to 3 of the model for ray_set(n_rays) on soup(n_tri): what every query of that pair shares (the largest scene's brute
    force takes its time)."""
    return Q.steps(soup(n_tri), ray_set(n_rays))


@functools.lru_cache(maxsize=None)
def expected(n_tri, n_rays, flags=0, first=0, count=-1):
    """The model's answer of the query on soup(n_tri) and ray_set(n_rays): computed once, shared by every stream order."""
    want = Q.query(soup(n_tri), ray_set(n_rays), flags, first, count, steps=model_steps(n_tri, n_rays))
    want.setflags(write=False)
    return want


def cull_name(flags):
    return {0: None, BACK: "back", FRONT: "front", Q.BOTH: "both"}[flags & Q.BOTH]


def ask(ctx, rays, flags=0, first=0, count=-1):
    return ctx.query_rays(rays, any_hit=bool(flags & ANY), cull=cull_name(flags), front_cw=bool(flags & CW), first_primitive=first,
                          primitive_count=count)


# ---- defaults ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order", ORDERS)
def test_defaults_are_swr_cast_rays(swr, order):
    """query == NULL and the all-defaults query write the bytes swr_cast_rays writes on the same context, and the model's."""
    L = swr.load_library()
    for n in SIZES:
        with resident(swr, soup(n), order) as ctx:
            for rays in ray_counts(n):
                rs = np.ascontiguousarray(ray_set(rays))
                cast = ctx.cast_rays(rs)
                check(cast, expected(n, rays), f"swr_cast_rays, {n} triangles, {rays} rays, order {order}")
                assert ask(ctx, rs).tobytes() == cast.tobytes(), (n, rays, "the all-defaults query")
                assert ask(ctx, rs, 0, 0, n).tobytes() == cast.tobytes(), (n, rays, "the whole range, spelt out")
                assert ask(ctx, rs, CW).tobytes() == cast.tobytes(), (n, rays, "FRONT_CW without a cull bit")
                out = np.full(rays, 0xA5, dtype=swr.binding.RAY_HIT_DTYPE)
                assert L.swr_query_rays(ctx._h, None, rs.ctypes.data, rays, out.ctypes.data) == 0
                assert out.tobytes() == cast.tobytes(), (n, rays, "query == NULL")
            assert ask(ctx, np.zeros(0, dtype=R.RAY_DTYPE), ANY).shape == (0,)


# ---- nearest mode: culls and ranges -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", SIZES)
def test_culls_against_the_model(swr, n, order):
    with resident(swr, soup(n), order) as ctx:
        for rays in ray_counts(n):
            for flags in culls(n):
                check(ask(ctx, ray_set(rays), flags), expected(n, rays, flags), f"{n} triangles, {rays} rays, flags {flags}, order {order}")


@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", SIZES)
def test_ranges_against_the_model(swr, n, order):
    with resident(swr, soup(n), order) as ctx:
        for rays in ray_counts(n):
            for first, count in ranges(n):
                want = expected(n, rays, 0, first, count)
                check(ask(ctx, ray_set(rays), 0, first, count), want, f"{n} triangles, {rays} rays, range {first} + {count}, order {order}")
                hit = want["primitive"] != NONE
                assert ((want["primitive"][hit] >= first) & (want["primitive"][hit] < first + count)).all()
        rays = ray_counts(n)[-1]
        first, count = ranges(n)[0]
        check(ask(ctx, ray_set(rays), BACK, first, count), expected(n, rays, BACK, first, count), f"{n}: a range and a cull")
        if count > 0:       # -1 from first: to the end of the scene
            check(ask(ctx, ray_set(rays), 0, first, -1), expected(n, rays, 0, first, -1), f"{n}: from {first} to the end")


# ---- any-hit ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", SIZES)
def test_any_hit_against_the_model(swr, n, order):
    with resident(swr, soup(n), order) as ctx:
        for rays in ray_counts(n):
            want = expected(n, rays, ANY)
            check(ask(ctx, ray_set(rays), ANY), want, f"any-hit, {n} triangles, {rays} rays, order {order}")
            assert (Q.occluded(want) == Q.occluded(expected(n, rays))).all()
            for flags, first, count in combined(n):
                check(ask(ctx, ray_set(rays), flags, first, count), expected(n, rays, flags, first, count),
                      f"any-hit, {n} triangles, {rays} rays, flags {flags}, range {first} + {count}, order {order}")
            for first, count in ranges(n):
                check(ask(ctx, ray_set(rays), ANY, first, count), expected(n, rays, ANY, first, count),
                      f"any-hit, {n} triangles, {rays} rays: range {first} + {count}")


A, B, C = (0, 0, 0), (4, 0, 0), (0, 4, 0)
TRI = np.array([[A, B, C]], dtype=np.float32)
DOWN, UP = (0, 0, -1), (0, 0, 1)
FAR = np.array([50, 50, 0], dtype=np.float32)
PROBES = [((1, 1, 2), DOWN), ((1, 1, -2), UP), ((51, 51, 2), DOWN), ((1, 1, 2), UP), ((-1, -1, 2), DOWN), ((1, 1, 2), DOWN, 0.0, 2.1)]


def placed_cases():
    """(name, triangles, rays): scenes of two workgroups per ray in which the place of the occluders is chosen."""
    n = 64 * GPW + 65
    last_slot = np.tile(TRI + FAR, (2 * 64 * GPW, 1, 1))        # two full chunks: the last slot of the second is the last triangle
    last_slot[-1] = TRI[0]
    first_and_last = np.tile(TRI + FAR, (n, 1, 1))
    first_and_last[0] = first_and_last[n - 1] = TRI[0]
    every = np.tile(TRI, (n, 1, 1))                              # every group of both chunks occludes: the early exits are taken
    every[:, :, 2] = -(np.arange(n, dtype=np.float32) % 7)[:, None] / 16
    return [("only the last slot of the second chunk occludes", last_slot, PROBES[:2] + PROBES[3:5]),   # (no ray meets the filler)
            ("the first and the last triangle occlude", first_and_last, PROBES),
            ("every group occludes", every, PROBES)]


@functools.lru_cache(maxsize=None)
def placed_expected():
    return {name: (Q.query(tri, R.rays(rays), ANY), Q.query(tri, R.rays(rays), ANY | BACK), Q.query(tri, R.rays(rays)))
            for name, tri, rays in placed_cases()}


@gpu
@pytest.mark.parametrize("order", ORDERS)
def test_any_hit_where_the_occluders_are_placed(swr, order):
    with swr.Context(0) as ctx:
        ctx.debug_set(TR.DEBUG_STREAM_ORDER, order)
        for name, tri, rays in placed_cases():
            ctx.scene_upload(*scene_of(tri))
            rs = R.rays(rays)
            want_any, want_back, want_near = placed_expected()[name]
            for _ in range(3):                  # the answer does not move with the timing of the workgroups
                check(ask(ctx, rs, ANY), want_any, f"{name}, order {order}")
            check(ask(ctx, rs, ANY | BACK), want_back, f"{name}, back faces culled, order {order}")
            check(ask(ctx, rs), want_near, f"{name}, nearest, order {order}")
            # the same ray 256 times: every workgroup of every copy races for a word of its own
            many = np.resize(rs[:2], 256)
            check(ask(ctx, many, ANY), np.resize(want_any[:2], 256), f"{name}, 256 copies, order {order}")


@gpu
def test_256_occlusion_rays_that_all_miss(swr):
    rays = np.array(ray_set(256))
    rays["origin"][:, 2] = 2.0
    rays["dir"][:, 2] = np.abs(rays["dir"][:, 2])           # from above the scene upwards, away from it
    rays["tmin"] = 0.0
    want = Q.query(soup(129), rays, ANY)
    assert (want["primitive"] == NONE).all() and not want["t"].any() and not want["u"].any() and not want["v"].any()
    with resident(swr, soup(129)) as ctx:
        check(ask(ctx, rays, ANY), want, "all miss")
    with swr.Context(0) as ctx:                              # a scene without triangles: every ray misses, in both modes
        v, _ = scene_of(soup(1))
        ctx.scene_upload(v, np.zeros(0, dtype=np.int64))
        none = Q.query(np.zeros((0, 3, 3), dtype=np.float32), ray_set(65), ANY)
        check(ask(ctx, ray_set(65), ANY), none, "no triangles, any-hit")
        check(ask(ctx, ray_set(65), BACK, 0, 0), none, "no triangles, nearest")


# ---- hand cases: one triangle from its front and from its back -----------------------------------------------------------------------------
def facing_cases():
    """[(flags, [front ray hit?, back ray hit?])]: TRI is counter-clockwise seen from +z, so the ray from above meets its front."""
    return [(0, [True, True]), (BACK, [True, False]), (FRONT, [False, True]), (CW, [True, True]), (CW | BACK, [False, True]),
            (CW | FRONT, [True, False]), (Q.BOTH, [False, False]), (CW | Q.BOTH, [False, False])]


@gpu
def test_one_triangle_from_its_front_and_its_back(swr):
    rs = R.rays(PROBES[:2])
    with resident(swr, TRI) as ctx:
        for flags, hit in facing_cases():
            got = ask(ctx, rs, flags)
            check(got, Q.query(TRI, rs, flags), f"flags {flags}")
            assert (got["primitive"] != NONE).tolist() == hit, flags
            got = ask(ctx, rs, flags | ANY)
            assert got["primitive"].tolist() == [OCC if h else NONE for h in hit] and not got["t"].any(), flags


# ---- deformation ----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_ray_occluded_at_rest_is_free_once_the_pose_moves_the_limb_away(swr):
    S = swr.scenes
    v, i = SM.torus(S)
    rays = R.rays([((0.55, 0.0, 1.5), DOWN, 0.0, 10.0), ((0.55 + SM.FAR[0], SM.FAR[1], 1.5 + SM.FAR[2]), DOWN, 0.0, 10.0)])
    away = SM.joint_matrix(0.0, 1.0, *SM.FAR)[None]
    j, w = SM.rigid_skin(v.shape[0])
    moved = SM.pose_vertices(v, j, w, away)
    rest, posed = Q.query(R.triangles(v, i), rays, ANY), Q.query(R.triangles(moved, i), rays, ANY)
    assert rest["primitive"].tolist() == [OCC, NONE] and posed["primitive"].tolist() == [NONE, OCC]
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        check(ask(ctx, rays, ANY), rest, "at rest")
        ctx.scene_skin(j, w)
        ctx.pose_set(away)
        check(ask(ctx, rays, ANY), posed, "moved away")
        check(ask(ctx, rays, BACK), Q.query(R.triangles(moved, i), rays, BACK), "moved away, the outside only")
        ctx.pose_set(None)
        check(ask(ctx, rays, ANY), rest, "back at rest")


@gpu
def test_morphed_scene(swr):
    S = swr.scenes
    v, i = SM.torus(S)
    rays = TR.torus_rays()
    deltas = MM.targets(S, v)
    moved = R.triangles(MM.morph_vertices(v, deltas, MM.WEIGHTS_A), i)
    ntri = moved.shape[0]
    rest = Q.query(R.triangles(v, i), rays, ANY)
    want = Q.query(moved, rays, ANY)
    assert want.tobytes() != rest.tobytes() and 100 <= Q.occluded(want).sum() <= 380
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        check(ask(ctx, rays, ANY), rest, "the rest shape")
        ctx.scene_morph(deltas)
        ctx.morph_set(MM.WEIGHTS_A)
        check(ask(ctx, rays, ANY), want, "morphed, any-hit")
        check(ask(ctx, rays, BACK), Q.query(moved, rays, BACK), "morphed, the outside only")
        check(ask(ctx, rays, FRONT, ntri // 4, ntri // 2), Q.query(moved, rays, FRONT, ntri // 4, ntri // 2), "morphed, a range from inside")
        ctx.morph_set(None)
        check(ask(ctx, rays, ANY), rest, "back in the rest shape")


# ---- draw items, bands, state -----------------------------------------------------------------------------------------------------------------
W, H = 200, 136
ITEM_TRIS = [40, 25, 63]


def item_scene():
    """Three items of one index array, each a soup of its own around its own centre, 10 apart along x, and 64 rays per item from above
    it.  A ray of item k passes the other items' triangles far away."""
    tri, rays = [], []
    for k, n in enumerate(ITEM_TRIS):
        shift = np.array([10.0 * k, 0, 0], dtype=np.float32)
        tri.append(soup(63)[:n] + shift)
        r = np.array(ray_set(64))
        r["origin"] += shift
        rays.append(r)
    return np.concatenate(tri).astype(np.float32), rays


@gpu
@pytest.mark.parametrize("order", [1, 0])
def test_each_item_of_a_draw_list_by_its_own_range(swr, order):
    tri, rays = item_scene()
    first = np.concatenate([[0], np.cumsum(ITEM_TRIS)])
    m = K.perspective_matrix()
    items = [(3 * int(first[k]), 3 * ITEM_TRIS[k], m) for k in range(3)]
    with resident(swr, tri, order) as ctx:
        ctx.target_set(W, H)
        ctx.draw_list(items, DT)                # (the list cuts the resident stream into its items)
        for k in range(3):
            for j in range(3):
                got = ask(ctx, rays[j], 0, items[k][0] // 3, items[k][1] // 3)
                check(got, Q.query(tri, rays[j], 0, int(first[k]), ITEM_TRIS[k]), f"item {k}, the rays of item {j}, order {order}")
                hit = got["primitive"] != NONE
                assert hit.any() == (j == k), (k, j)
                assert ((got["primitive"][hit] >= first[k]) & (got["primitive"][hit] < first[k + 1])).all()
                check(ask(ctx, rays[j], ANY, int(first[k]), ITEM_TRIS[k]), Q.query(tri, rays[j], ANY, int(first[k]), ITEM_TRIS[k]),
                      f"item {k}, the rays of item {j}, any-hit")


@gpu
def test_three_bands(swr):
    n = 129
    with resident(swr, soup(n), device_count=3) as ctx:
        ctx.target_set(W, H)
        assert len(ctx.bands()) == 3
        check(ask(ctx, ray_set(256), ANY), expected(n, 256, ANY), "three bands, any-hit")
        ctx.draw(K.perspective_matrix(), DT)
        check(ask(ctx, ray_set(256), BACK, 10, 40), expected(n, 256, BACK, 10, 40), "three bands, behind a frame")


@gpu
@pytest.mark.parametrize("order", [1, 0])
def test_the_call_changes_nothing(swr, order):
    """A frame and swr_cast_rays give equal bytes before and after the queries."""
    n = 129
    m = K.perspective_matrix()
    with resident(swr, soup(n), order) as ctx:
        ctx.target_set(W, H)
        ctx.draw(m, DT | IDS)
        before = (ctx.read_color(), ctx.read_depth(), ctx.read_ids())
        cast = ctx.cast_rays(ray_set(256))
        check(ask(ctx, ray_set(256), ANY), expected(n, 256, ANY), "behind a frame")
        check(ask(ctx, ray_set(256), CW | BACK, 60, 10), expected(n, 256, CW | BACK, 60, 10), "behind a frame")
        check(ask(ctx, ray_set(256), ANY | FRONT, 64, 64), expected(n, 256, ANY | FRONT, 64, 64), "behind a frame")
        for a, b in zip(before, (ctx.read_color(), ctx.read_depth(), ctx.read_ids())):
            assert a.tobytes() == b.tobytes()
        assert ctx.cast_rays(ray_set(256)).tobytes() == cast.tobytes()
        ctx.draw(m, DT | IDS)
        for a, b in zip(before, (ctx.read_color(), ctx.read_depth(), ctx.read_ids())):
            assert a.tobytes() == b.tobytes(), "a frame drawn after the calls"


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def error_table(ntri):
    """(flags, reserved, first, count) of every query swr_query_rays refuses over ntri primitives, and of some it accepts."""
    refused = [(16, 0, 0, -1), (1 << 31, 0, 0, -1), (ANY | 32, 0, 0, -1), (0, 1, 0, -1), (ANY, 1 << 31, 0, -1), (0, 0, -1, -1), (0, 0, -1, 0),
               (0, 0, 0, -2), (0, 0, 0, ntri + 1), (0, 0, ntri, 1), (0, 0, ntri + 1, 0), (0, 0, ntri + 1, -1), (0, 0, 1, ntri),
               (0, 0, 1 << 62, 1 << 62), (0, 0, 5, (1 << 63) - 1)]
    accepted = [(15, 0, 0, -1), (0, 0, ntri, 0), (0, 0, ntri, -1), (0, 0, 0, ntri), (ANY, 0, ntri - 1, 1)]
    return refused, accepted


@gpu
def test_errors(swr):
    B = swr.binding
    L = swr.load_library()
    rays = np.array(ray_set(65))
    hits = np.full(65 * 4, 0xA5A5A5A5, dtype=np.uint32)

    def last_error(ctx):
        return (L.swr_last_error(ctx._h) or b"").decode()

    def call(ctx, q=(0, 0, 0, -1), r=rays, n=65, out=hits):
        query = np.zeros(1, dtype=B.RAY_QUERY_DTYPE)
        query[0] = q
        return L.swr_query_rays(ctx._h, query.ctypes.data, r.ctypes.data if r is not None else None, n,
                                out.ctypes.data if out is not None else None)

    with swr.Context(0) as ctx:
        assert call(ctx) == NO_SCENE and call(ctx, n=0) == NO_SCENE
        ctx.scene_upload(*scene_of(soup(129)))
        refused, accepted = error_table(129)
        for q in refused:
            assert Q.check_query(129, *q) is not None
            assert call(ctx, q) == BAD_ARG, q
            assert "swr_query_rays:" in last_error(ctx), q
            assert call(ctx, q, r=None, n=0, out=None) == BAD_ARG, q
        assert call(ctx, n=-1) == BAD_ARG and call(ctx, r=None) == BAD_ARG and call(ctx, out=None) == BAD_ARG
        assert call(ctx, n=B.RAYS_MAX + 1) == UNSUPPORTED
        assert call(ctx, r=None, n=0, out=None) == 0
        for word, bad in [(0, np.nan), (3, -np.inf), (6, np.inf), (7, np.nan)]:
            r = rays.copy()
            r.view(np.float32).reshape(-1, 8)[37, word] = bad
            assert call(ctx, (ANY, 0, 0, -1), r=r) == BAD_ARG and "swr_query_rays: ray 37:" in last_error(ctx)
        r = rays.copy()
        r["dir"][64] = (0.0, -0.0, 0.0)
        assert call(ctx, r=r) == BAD_ARG and "ray 64: the direction is zero" in last_error(ctx)
        r = rays.copy()
        r["tmin"][0], r["tmax"][0] = 2.0, 1.0
        assert call(ctx, r=r) == BAD_ARG and "ray 0: tmin" in last_error(ctx)
        assert (hits == 0xA5A5A5A5).all(), "an error writes nothing"
        for q in accepted:
            assert Q.check_query(129, *q) is None
            assert call(ctx, q) == 0, q
            want = Q.query(soup(129), rays, q[0], q[2], q[3])
            assert hits.tobytes() == want.tobytes(), q
        # after the errors the scene answers as before; SWR_RAYS_MAX occlusion rays are accepted
        many = np.resize(np.array(ray_set(256)), B.RAYS_MAX)
        got = ask(ctx, many, ANY)
        assert got.tobytes() == np.resize(np.array(expected(129, 256, ANY)), B.RAYS_MAX).tobytes(), "SWR_RAYS_MAX rays"
