"""Item bounds (swr_item_bounds; include/swr.h "Item bounds"): the screen rectangle, the depth range and the triangle
counts of draw items, reduced on the device from the resident triangle stream.

Equality is exact everywhere, and no expectation comes from the code under test:
  (a) the numpy float32 model of tests/item_bounds_model.py, written from the header's text, bit for bit (the 48-byte records as bytes);
  (b) containment, which does not go through the model: the list drawn with SWR_FLAG_PRIMITIVE_IDS, read back and mapped to items —
      every pixel an item wins lies inside the item's rectangle; the same over the ID image frame_model.expect builds from the oracle;
  (c) for posed and morphed scenes also a fresh context that uploaded the vertices of tests/skin_model.py / tests/morph_model.py.

The scene is a seeded soup of 1 100 small triangles (object space, z in [-0.5, 0.5]) on a 200 x 136 target — neither dimension a
multiple of 64 or 32 — through a perspective matrix (w = z + 2).  The items' triangle counts are 1, 63, 64, 65, 300 and 1 025: one lane,
either side of a wave, more than one wave of a workgroup; whether more than one workgroup folds into one record depends on
ITEM_BOUNDS_CHUNK, so the scene of test_more_than_one_workgroup_per_item takes its size from that constant."""
import os
import re

import numpy as np
import pytest

import frame_model as FM
import item_bounds_model as M
import kernel_matrix as K
import morph_model as MM
import skin_model as SM

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_item_bounds.hip")
DT, NC, METAL, LOAD, IDS, CLIP, CB = FM.DT, FM.NC, FM.METAL, FM.LOAD, FM.IDS, FM.CLIP, FM.CB
IDENT = K.IDENT
W, H = 200, 136
NTRI = 1100
NAN_TRI = 700
BAD_ARG, INDEX_COUNT, HIP, UNSUPPORTED, NO_SCENE = -1, -2, -4, -5, -6
DEBUG_STREAM_ORDER = 1


def chunk():
    """ITEM_BOUNDS_CHUNK: the stream slots one k_item_bounds workgroup folds."""
    src = open(os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_internal.h")).read()
    assert "constexpr int ITEM_BOUNDS_CHUNK = SWR_TUNE_ITEM_BOUNDS_CHUNK;" in src
    return int(re.search(r"#define SWR_TUNE_ITEM_BOUNDS_CHUNK (\d+)\b", src).group(1))


# ---- matrices (16 floats, column-major: m[4 * column + row]) ----------------------------------------------------------------------
def matrix(sx=1.0, sy=1.0, tx=0.0, ty=0.0, wz=0.0, ww=1.0):
    m = np.zeros(16, dtype=np.float32)
    m[0], m[5], m[10] = sx, sy, 1.0
    m[12], m[13] = tx, ty
    m[11], m[15] = wz, ww
    return m


PERSP = matrix(2.0, 2.0, wz=1.0, ww=2.0)                    # w = z + 2 in [1.5, 2.5]
AFFINE = matrix(0.9, 0.8, tx=0.05, ty=-0.1)
OFF = matrix(1.0, 1.0, tx=5.0)                              # wholly right of the target
LEFT = matrix(1.0, 1.0, tx=-1.0)                            # straddles x = 0: negative sx
BEHIND = matrix(1.0, 1.0, wz=1.0, ww=0.0)                   # w = z in [-0.5, 0.5]: corners with w <= 0
INSTANCES = [matrix(0.5, 0.5, tx=0.4 * j - 0.8, ty=0.3 * j - 0.6, wz=0.25 * j, ww=1.5) for j in range(5)]


def soup(seed=0x1B0):
    """1 100 triangles, three vertices each (not shared), centres in [-0.7, 0.7]^2, z in [-0.5, 0.5]; triangle NAN_TRI has a NaN x."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.7, 0.7, (NTRI, 1, 2))
    xy = c + rng.uniform(-0.06, 0.06, (NTRI, 3, 2))
    z = rng.uniform(-0.5, 0.5, (NTRI, 3, 1))
    xyz = np.concatenate([xy, z], axis=-1).reshape(-1, 3)
    v = K._pack(xyz, rng.uniform(0, 1, (3 * NTRI, 3)))
    v[3 * NAN_TRI + 1, 0] = np.nan
    return np.ascontiguousarray(v), np.arange(3 * NTRI, dtype=np.int64)


def tri_item(first, count, m):
    return (3 * first, 3 * count, m)


def items_all():
    """Every case of the issue in one list: counts 1, 63, 64, 65, 300, 1 025 at starts off a multiple of 64, an empty item, a repeated
    and an overlapping range, one range under five matrices, the NaN triangle, off screen, straddling x = 0, w <= 0, affine and
    non-affine matrices side by side."""
    it = [tri_item(5, 1, PERSP), tri_item(70, 63, AFFINE), tri_item(130, 64, PERSP), tri_item(3, 65, AFFINE), tri_item(333, 300, PERSP),
          tri_item(37, 1025, PERSP), tri_item(200, 0, PERSP), tri_item(130, 64, PERSP), tri_item(150, 100, AFFINE)]
    it += [tri_item(400, 200, m) for m in INSTANCES]
    it += [tri_item(690, 30, PERSP), tri_item(NAN_TRI, 1, AFFINE), tri_item(5, 40, OFF), tri_item(5, 40, LEFT), tri_item(600, 80, BEHIND),
           tri_item(0, NTRI, IDENT), tri_item(NTRI, 0, IDENT)]
    return it


def items_drawn():
    """The items of the containment frames: as items_all without the w <= 0 item (mirrored triangles of millions of pixels)."""
    return [it for it in items_all() if it[2] is not BEHIND]


@pytest.fixture(scope="module")
def scene():
    return soup()


@pytest.fixture(scope="module")
def want(scene):
    v, i = scene
    return {flags: M.item_bounds(v, i, items_all(), W, H, flags) for flags in (0, METAL)}


def check(got, expected, what):
    assert got.dtype.itemsize == 48 and got.shape == expected.shape, what
    for k in range(expected.size):
        assert got[k].tobytes() == expected[k].tobytes(), f"{what}: item {k}: {got[k]} is not the model's {expected[k]}"


# ---- the model's answers for this scene are not vacuous (CPU) -------------------------------------------------------------------------
def test_the_scene_reaches_every_case(want):
    for flags in (0, METAL):
        b = want[flags]
        its = items_all()
        assert [int(x) for x in b["drawable"] + b["skipped"]] == [c // 3 for _, c, _ in its]
        k = {name: n for n, name in enumerate(["one", "n63", "n64", "n65", "n300", "n1025", "empty", "repeat", "overlap", "i0", "i1", "i2", "i3",
                                               "i4", "nan30", "nan1", "off", "left", "behind", "all", "end"])}
        assert b[k["repeat"]].tobytes() == b[k["n64"]].tobytes()
        assert b["drawable"][k["empty"]] == 0 and np.isposinf(b["zmin"][k["empty"]]) and b[k["empty"]].tobytes() == b[k["end"]].tobytes()
        assert (b["skipped"][k["nan30"]], b["drawable"][k["nan30"]]) == (1, 29)
        assert (b["skipped"][k["nan1"]], b["drawable"][k["nan1"]], b["x1"][k["nan1"]]) == (1, 0, 0)
        assert b["x0"][k["off"]] == b["x1"][k["off"]] == W and b["drawable"][k["off"]] == 40
        assert b["behind"][k["behind"]] > 0 and b["behind"][k["behind"]] < b["drawable"][k["behind"]]
        assert b["behind"].sum() == b["behind"][k["behind"]]
        assert len({b[k[f"i{j}"]].tobytes() for j in range(5)}) == 5
        assert (b["x1"] > b["x0"]).sum() >= 15
    v, i = soup()
    sx = M.corners(v[15:135, 0:3], LEFT, W, H, False)[0]
    assert (sx < 0).any() and (sx > 0).any() and want[0]["x0"][17] == 0 and want[0]["x1"][17] > 0
    # under the Metal rules the negative corners skip their triangles instead
    assert want[METAL]["skipped"][17] > 0 and want[0]["skipped"][17] == 0


# ---- against the model ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order", [1, 0, -1])
def test_against_the_model(swr, scene, want, order):
    """Both rule sets; the stream Morton-sorted (cut by the call), in the caller's order and as for 2^24 primitives; before a draw
    list of the same items (the cuts not there yet) and after it (in place)."""
    v, i = scene
    its = items_all()
    with swr.Context(0) as ctx:
        ctx.debug_set(DEBUG_STREAM_ORDER, order)
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        for flags in (0, METAL):
            check(ctx.item_bounds(its, flags), want[flags], f"order {order}, flags {flags}, before the list")
        ctx.draw_list(items_drawn(), DT | NC)         # (all but the w <= 0 item: its cut is made by the next call)
        for flags in (METAL, 0, DT | NC | CB | IDS | LOAD):
            check(ctx.item_bounds(its, flags), want[flags & METAL], f"order {order}, flags {flags}, after the list")
        # a list with other boundaries, then the first one again
        other = [tri_item(1, 1099, PERSP), tri_item(64, 64, AFFINE)]
        check(ctx.item_bounds(other), M.item_bounds(v, i, other, W, H), "other boundaries")
        check(ctx.item_bounds(its), want[0], "the first list again")
        assert ctx.item_bounds([]).shape == (0,)
    # the list drawn first: the call finds the cuts in place
    with swr.Context(0) as ctx:
        ctx.debug_set(DEBUG_STREAM_ORDER, order)
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw_list(items_drawn(), DT | NC)         # (all but the w <= 0 item: its cut is made by the next call)
        check(ctx.item_bounds(its, METAL), want[METAL], f"order {order}: drawn first")


@gpu
def test_more_than_one_workgroup_per_item(swr):
    """An item of 2 * ITEM_BOUNDS_CHUNK + 1 triangles (three workgroups fold into one record, the last with one triangle), one of
    exactly a chunk and one of a chunk and a bit starting off its multiple, next to each other."""
    C = chunk()
    n = 3 * C + 77
    rng = np.random.default_rng(0x1B1)
    xyz = np.concatenate([rng.uniform(-0.9, 0.9, (3 * n, 2)), rng.uniform(-0.5, 0.5, (3 * n, 1))], axis=-1)
    v, i = K._pack(xyz, rng.uniform(0, 1, (3 * n, 3))), np.arange(3 * n, dtype=np.int64)
    # the extremes of the big item lie in its last workgroup's only triangle and in its first lane
    v[3 * (2 * C + 10), 2] = 0.6
    v[3 * 10, 2] = -0.6
    its = [tri_item(10, 2 * C + 1, PERSP), tri_item(5, C, AFFINE), tri_item(C - 3, C + 5, PERSP), tri_item(0, n, IDENT)]
    expected = M.item_bounds(v, i, its, W, H)
    assert expected["zmax"][0] > expected["zmax"][2] and expected["zmin"][0] < expected["zmin"][2] and expected["drawable"][0] == 2 * C + 1
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        check(ctx.item_bounds(its), expected, "chunks")
        check(ctx.item_bounds(its, METAL), M.item_bounds(v, i, its, W, H, METAL), "chunks, Metal rules")


# ---- containment ------------------------------------------------------------------------------------------------------------------
def contained(item_of, bounds, what):
    """Every pixel whose ID belongs to item k lies inside item k's rectangle."""
    seen = 0
    for k in range(bounds.size):
        ys, xs = np.nonzero(item_of == k)
        if ys.size == 0:
            continue
        seen += 1
        b = bounds[k]
        assert b["x0"] <= xs.min() and xs.max() < b["x1"] and b["y0"] <= ys.min() and ys.max() < b["y1"], \
            f"{what}: item {k} wins pixels in x [{xs.min()}, {xs.max()}] y [{ys.min()}, {ys.max()}], outside {b}"
    return seen


@gpu
@pytest.mark.parametrize("rules", [0, DT, METAL])
def test_every_pixel_an_item_wins_lies_in_its_rectangle(swr, oracle, scene, rules):
    """Painter's order, z-tested and under the Metal rules; the IDs of the library's own frame and the oracle's (frame_model.expect)."""
    v, i = scene
    its = items_drawn()
    B = swr.binding
    spec = FM.FrameSpec(v, i, W, H, rules | IDS, items=its)
    _, _, wi = FM.expect(oracle, spec)
    ids_model = np.where(wi == FM.LIVE, np.int64(FM.NONE), wi).astype(np.uint32)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        bounds = ctx.item_bounds(its, rules)
        ctx.draw_list(its, rules | IDS)
        ids = ctx.read_ids()
    FM.same((None, None, ids), (None, None, wi), f"IDs, rules {rules}")
    for name, image in (("library", ids), ("oracle", ids_model)):
        item_of, _ = B.list_ids_to_items(image, its)
        assert contained(item_of, bounds, f"{name} IDs, rules {rules}") >= 12
    # ... and the model's rectangles hold the same pixels (the two agree bit for bit anyway: test_against_the_model)
    contained(B.list_ids_to_items(ids_model, its)[0], M.item_bounds(v, i, its, W, H, rules & METAL), "the model's rectangles")


# ---- skin and morph ---------------------------------------------------------------------------------------------------------------
def torus_items(ni):
    t = ni // 3
    return [tri_item(0, t, PERSP), tri_item(0, t // 3, AFFINE), tri_item(t // 3 + 5, t // 2, PERSP), tri_item(t - 100, 100, INSTANCES[3])]


@gpu
@pytest.mark.parametrize("what", ["pose", "morph", "both"])
def test_posed_and_morphed_scenes(swr, what):
    """What the host cannot answer today: the bounds follow swr_pose_set and swr_morph_set, equal the model's on the vertices of
    skin_model / morph_model, and equal the bounds of a fresh context that uploaded those vertices."""
    S = swr.scenes
    v, i = SM.torus(S)
    joint, weight = SM.bend_skin(v)
    pose = SM.bend_pose()
    deltas = MM.targets(S, v)
    its = torus_items(i.size)
    moved = v
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(SM.W, SM.H)
        rest = ctx.item_bounds(its)
        check(rest, M.item_bounds(v, i, its, SM.W, SM.H), "bind pose")
        if what in ("morph", "both"):
            ctx.scene_morph(deltas)
            ctx.morph_set(MM.WEIGHTS_A)
            moved = MM.morph_vertices(moved, deltas, MM.WEIGHTS_A)
        if what in ("pose", "both"):
            ctx.scene_skin(joint, weight)
            ctx.pose_set(pose)
            moved = SM.pose_vertices(moved, joint, weight, pose)
        for flags in (0, METAL):
            expected = M.item_bounds(moved, i, its, SM.W, SM.H, flags)
            check(ctx.item_bounds(its, flags), expected, f"{what}, flags {flags}")
            assert expected.tobytes() != M.item_bounds(v, i, its, SM.W, SM.H, flags).tobytes()
        # the same list drawn and asked again; then back to the rest shape
        ctx.draw_list(its, DT)
        check(ctx.item_bounds(its), M.item_bounds(moved, i, its, SM.W, SM.H), f"{what}, after the list")
        if what in ("morph", "both"):
            ctx.morph_set(None)
        if what in ("pose", "both"):
            ctx.pose_set(None)
        check(ctx.item_bounds(its), rest, "back in the rest shape")
    with swr.Context(0) as fresh:
        fresh.scene_upload(np.ascontiguousarray(moved), i)
        fresh.target_set(SM.W, SM.H)
        check(fresh.item_bounds(its), M.item_bounds(moved, i, its, SM.W, SM.H), f"{what}: a fresh context with the moved vertices")


# ---- neutrality -------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_call_changes_no_image_and_is_no_frame(swr, oracle, scene, want):
    v, i = scene
    its = items_drawn()
    B = swr.binding
    cache = {}
    first = FM.FrameSpec(v, i, W, H, DT | IDS, items=its, key="first")
    top = [tri_item(333, 300, AFFINE), tri_item(5, 1, PERSP)]
    second = FM.FrameSpec(v, i, W, H, DT | IDS | LOAD, items=top, key="second")
    w1 = FM.expect(oracle, first, cache=cache)
    w2 = FM.expect(oracle, second, start=(w1[0], w1[1]), cache=cache)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw_list(its, DT | IDS)
        before = (ctx.read_color(), ctx.read_depth(), ctx.read_ids())
        counts = ctx.count_ids(B.COUNT_PER_ITEM)
        FM.same(before, w1, "the frame")
        check(ctx.item_bounds(items_all(), METAL), want[METAL], "between two reads")
        check(ctx.item_bounds(top), M.item_bounds(v, i, top, W, H), "new boundaries between two reads")
        after = (ctx.read_color(), ctx.read_depth(), ctx.read_ids())
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
        again = ctx.count_ids(B.COUNT_PER_ITEM)           # still the last frame's items: the call was no frame
        assert np.array_equal(again[0], counts[0]) and again[1] == counts[1] and counts[0].size == len(its)
        ctx.draw_list(top, DT | IDS | LOAD)
        FM.same((ctx.read_color(), ctx.read_depth(), ctx.read_ids()), w2, "a load frame on top")


@gpu
def test_first_waiting_call_after_an_overflowed_frame(swr, oracle):
    """Forced as tests/test_depth_query.py forces it: a fresh context whose fixed-stride bins are too small for 20 000 triangles in a
    few tiles.  swr_item_bounds is the first call that waits: the frame is repaired, and the image afterwards is the oracle's."""
    w, h = 1280, 720
    s = swr.scenes.random_soup(20000, w, h, 555, r_ndc=0.01, flags=DT, margin=1.0)
    v = s.vertices.copy()
    v[:, 0] = 0.30 + (v[:, 0] * 0.5 + 0.5) * 0.07
    v[:, 1] = 0.10 + (v[:, 1] * 0.5 + 0.5) * 0.06
    v = np.ascontiguousarray(v)
    d = FM.expect(oracle, FM.FrameSpec(v, s.indices, w, h, DT, transform=s.transform))[1]
    its = [(0, s.indices.size, s.transform), (300, 3000, s.transform)]
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, s.indices)
        ctx.draw(s.transform, DT)
        check(ctx.item_bounds(its), M.item_bounds(v, s.indices, its, w, h), "after an overflowed frame")
        assert ctx.read_depth().tobytes() == d.tobytes()


# ---- bands ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_bands_and_samples(swr, scene, want):
    v, i = scene
    its = items_all()
    with swr.Context(0, device_count=3) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        assert len(ctx.bands()) == 3
        check(ctx.item_bounds(its), want[0], "three bands")
        ctx.draw_list(items_drawn(), DT | NC)         # (all but the w <= 0 item: its cut is made by the next call)
        check(ctx.item_bounds(its, METAL), want[METAL], "three bands, after the list")
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H, 32, 96)
        check(ctx.item_bounds(its), want[0], "a context that owns rows [32, 96)")
        ctx.target_set(W, H, 96, 96)
        check(ctx.item_bounds(its, METAL), want[METAL], "a context without rows")
    # after swr_render_resolved the target is the sample grid: the rectangles are in samples
    with swr.Context(0) as ctx:
        ctx.render_resolved(v, i, PERSP, W // 2, H // 2, DT, factor=2)
        assert (ctx.width, ctx.height) == (W, H)
        check(ctx.item_bounds(its), want[0], "in samples after a resolved render")
        ctx.render_resolved(v, i, PERSP, W, H, DT, factor=2)
        check(ctx.item_bounds(its), M.item_bounds(v, i, its, 2 * W, 2 * H), "2W x 2H samples")


# ---- the chain into swr_query_depth ---------------------------------------------------------------------------------------------------
CHAIN_MARGIN = 2.0 ** -24       # see chain_margin: the smallest candidate, computed from the oracle's image on the CPU
CHAIN_CANDIDATES = [2.0 ** -k for k in range(24, -1, -1)]      # below 2^-24 the subtraction no longer moves a depth near 1


def chain_scene():
    """One large occluder at z = 0.5 — the triangle (0, -H), (0, 2H), (0.9 W, H / 2): every pixel left of 0.69 W in the rows used —
    then 8 groups of 20 small triangles: groups 0-3 wholly behind it (z 0.7 .. 0.9), groups 4-5 over it and in front (z 0.1 .. 0.3),
    groups 6-7 further right, in front too."""
    rng = np.random.default_rng(0x1B2)
    ox, oy = K._ndc(np.array([0, 0, 0.9]) * W, np.array([-1.0, 2.0, 0.5]) * H, W, H)
    occ = np.stack([ox, oy, np.full(3, 0.5)], axis=-1)
    parts, items = [occ], []
    base = 1
    for g in range(8):
        x0 = (0.05 + 0.13 * (g % 4)) * W if g < 6 else (0.75 + 0.11 * (g - 6)) * W
        z0, z1 = (0.7, 0.9) if g < 4 else (0.1, 0.3)
        xyz, _ = K._tris(rng, 20, x0, 0.15 * H, x0 + 0.1 * W, 0.85 * H, 3.0, z0, z1, W, H)
        parts.append(xyz)
        items.append(tri_item(base, 20, IDENT))
        base += 20
    xyz = np.concatenate(parts)
    v = K._pack(xyz, rng.uniform(0, 1, (xyz.shape[0], 3)))
    return v, np.arange(v.shape[0], dtype=np.int64), [tri_item(0, 1, IDENT)], items


def chain_expected(depth, bounds, margin):
    z = bounds["zmin"].astype(np.float32) - np.float32(margin)
    return np.array([int((z[k] < depth[b["y0"]:b["y1"], b["x0"]:b["x1"]]).sum()) for k, b in enumerate(bounds)])


def chain_margin(oracle):
    """The smallest candidate for which, on the oracle's own image of the occluders and with the model's bounds, the items behind pass
    0 pixels and the items in front or beside pass at least 1."""
    v, i, occluders, items = chain_scene()
    depth = FM.expect(oracle, FM.FrameSpec(v, i, W, H, DT, items=occluders))[1]
    bounds = M.item_bounds(v, i, items, W, H)
    for margin in CHAIN_CANDIDATES:
        passed = chain_expected(depth, bounds, margin)
        if (passed[:4] == 0).all() and (passed[4:] >= 1).all():
            return margin, depth, bounds
    raise AssertionError("no margin satisfies the chain on the oracle's image")


def test_chain_margin_is_the_oracles(oracle):
    assert chain_margin(oracle)[0] == CHAIN_MARGIN


@gpu
def test_bounds_feed_the_depth_query(swr, oracle):
    v, i, occluders, items = chain_scene()
    margin, depth, bounds = chain_margin(oracle)
    B = swr.binding
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw_list(occluders, DT)
        got = ctx.item_bounds(items)
        check(got, bounds, "the chain's items")
        passed = ctx.query_depth(B.depth_boxes(got, margin))
        assert (passed[:4] == 0).all() and (passed[4:] >= 1).all(), passed
        assert np.array_equal(passed, chain_expected(depth, bounds, margin))


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def code_of(swr, call):
    with pytest.raises(swr.SwrError) as e:
        call()
    return e.value.code


@gpu
@pytest.mark.parametrize("device_count", [0, 2])
def test_errors(swr, scene, want, device_count):
    v, i = scene
    its = items_all()
    L, B = swr.load_library(), swr.binding
    good = B.Context.draw_items(its)
    out = np.full(good.size * 12 + 12, 0xA5A5A5A5, dtype=np.uint32)
    with swr.Context(0, device_count=device_count) as ctx:
        def raw(items, n, flags=0, dst=out):
            return L.swr_item_bounds(ctx._h, None if items is None else items.ctypes.data, n, flags, None if dst is None else dst.ctypes.data)
        assert raw(good, good.size) == NO_SCENE                             # no scene, no target
        ctx.scene_upload(v, i)
        assert raw(good, good.size) == NO_SCENE                             # no target
        ctx.target_set(W, H)
        assert raw(None, good.size) == BAD_ARG
        assert raw(good, good.size, dst=None) == BAD_ARG
        assert raw(good, -1) == BAD_ARG
        assert raw(good, good.size, 1 << 9) == BAD_ARG                      # unknown flag bits, as for a frame
        assert raw(good, good.size, CLIP) == UNSUPPORTED
        assert raw(good, good.size, CLIP | DT | NC) == UNSUPPORTED
        for field, delta, code in (("first_index", 1, INDEX_COUNT), ("index_count", -1, INDEX_COUNT), ("first_index", 3 * NTRI, BAD_ARG),
                                   ("index_count", 3 * NTRI, BAD_ARG), ("first_index", -3 * NTRI, BAD_ARG)):
            bad = good.copy()
            bad[field][4] += delta
            assert raw(bad, bad.size) == code, (field, delta)
        one = B.Context.draw_items([tri_item(5, 1, PERSP)])
        most = np.repeat(one, B.DRAW_LIST_MAX)
        big = np.full((B.DRAW_LIST_MAX + 1) * 12, 0xA5A5A5A5, dtype=np.uint32)
        assert raw(np.repeat(one, B.DRAW_LIST_MAX + 1), B.DRAW_LIST_MAX + 1, dst=big) == UNSUPPORTED
        assert (out == 0xA5A5A5A5).all() and (big == 0xA5A5A5A5).all(), "after an error nothing was written"
        assert code_of(swr, lambda: ctx.item_bounds(its, CLIP)) == UNSUPPORTED
        # 4 096 items are accepted; n == 0 is legal with NULL pointers; the context is still usable
        got = ctx.item_bounds(most)
        assert got.size == B.DRAW_LIST_MAX and all(got[k].tobytes() == want[0][0].tobytes() for k in (0, 1, 4095))
        assert raw(None, 0, dst=None) == 0
        check(ctx.item_bounds(its), want[0], "after the refusals")


@gpu
def test_failed_context_returns_its_sticky_error(swr, scene):
    v, i = scene
    ctx = swr.Context(0, wait_budget_ms=300)
    try:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw(IDENT, DT)
        ctx.sync()
        assert ctx.item_bounds([tri_item(0, NTRI, IDENT)])["drawable"][0] == NTRI - 1
        ctx.debug_fault(swr.binding.FAULT_ENQUEUE)      # the next frame's raster share fails as if a launch had returned an error
        try:
            ctx.draw(IDENT, DT)
        except swr.SwrError as e:
            assert e.code == HIP
        assert code_of(swr, lambda: ctx.sync()) == HIP
        assert code_of(swr, lambda: ctx.item_bounds([tri_item(0, 1, IDENT)])) == HIP
    finally:
        ctx.close()


# ---- the example ------------------------------------------------------------------------------------------------------------------
@gpu
def test_frame_loop_example_bounds_of_a_posed_mesh(swr, capsys):
    """examples/frame_loop.py --objects 9 --depth-test --occlusion --bounds --skin: the copies' boxes come from the device, which is
    what lets the occlusion test run on a mesh that is posed there."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    fl.run(3, 128, None, depth_test=True, objects=9, occlusion=True, bounds=True, skin=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("occlusion:")]
    assert len(lines) == 2          # every frame but the first is tested against its predecessor
    for ln in lines:
        m = re.match(r"occlusion: frame (\d+): (\d+) of (\d+) objects could be skipped \(pixels that pass per object: \[(.*)\]\)", ln)
        skipped, total = int(m.group(2)), int(m.group(3))
        per = [int(t) for t in m.group(4).split(",")]
        assert total == 9 and len(per) == 9 and skipped == sum(1 for p in per if p == 0) and max(per) > 0
    with pytest.raises(ValueError):
        fl.run(1, 64, None, depth_test=True, objects=2, occlusion=True, skin=True)      # a posed mesh needs --bounds


# ---- the table: every kernel instantiation launched in swr_item_bounds.hip has a GPU case above --------------------------------------
GPU_CASES = {
    "k_item_bounds_init": ("test_against_the_model", "test_errors"),
    "k_item_bounds<false>": ("test_against_the_model", "test_more_than_one_workgroup_per_item", "test_posed_and_morphed_scenes"),
    "k_item_bounds<true>": ("test_against_the_model", "test_more_than_one_workgroup_per_item", "test_posed_and_morphed_scenes"),
    "k_item_bounds_finish": ("test_against_the_model", "test_bands_and_samples"),
}


def test_every_launched_kernel_has_a_gpu_case():
    src = open(SRC).read()
    body = src[src.index("void launch_item_bounds("):].replace(" ", "")
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(k_item_bounds\w*(?:<[^>]*>)?)\)?,", body))
    assert launched, "launch_item_bounds launches nothing"
    assert launched == set(re.findall(r"k_item_bounds(?:_\w+|<[^>]*>)", body)), "an instantiation outside hipLaunchKernelGGL"
    assert set(re.findall(r"__global__[^;{]*?(k_item_bounds\w*)\(", src)) == {"k_item_bounds_init", "k_item_bounds", "k_item_bounds_finish"}
    missing = launched - set(GPU_CASES)
    assert not missing, f"no GPU case for {sorted(missing)}"
    for variant, tests in GPU_CASES.items():
        assert variant in launched, f"{variant} is not launched"
        for name in tests:
            fn = globals().get(name)
            assert callable(fn) and any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), (variant, name)
