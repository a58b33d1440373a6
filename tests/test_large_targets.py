"""Targets beyond 8K (tests/target_sizes.py is the table of thresholds; tests/test_target_sizes_table.py keeps it honest): triangles that
run the length of a 65535-pixel axis, so that their extents leave the 16-bit vertex deltas and the dense walk's bound and every pixel of
them is on the screen, coordinates that fill the 16-bit halves of a packed box, and tile grids on both sides of the LDS binning limit,
of 64 KB of dynamic LDS and of one tile per k_scan thread.  Every expectation comes from the oracle or from the existing models
(frame_model.expect, resolve_model, delta_model, item_bounds_model, test_depth_query.expected); results are compared as bits.  Each case
first asserts on the CPU, from the oracle alone, that the triangles it is about have the extents meant and that their pixels are in
the expected image."""
import dataclasses
import time

import numpy as np
import pytest

import delta_model as DM
import frame_model as FM
import item_bounds_model as IBM
import kernel_matrix as K
import resolve_model as RM
import target_sizes as TS
import test_depth_query as TDQ

gpu = pytest.mark.gpu
DT, NC, METAL, LOAD, IDS = K.DT, K.NC, K.METAL, K.LOAD, K.IDS
CB, CF, CCW, CLIP, PERSP, BLEND = FM.CB, FM.CF, FM.CCW, FM.CLIP, FM.PERSP, FM.BLEND
REAL_LINES = FM.REAL_LINES
TRI, LINE, VERTICES = 0, 1, 2
IDENT = K.IDENT
COUNT_PER_PRIMITIVE, COUNT_PER_ITEM = 0, 1

# case -> the rows of target_sizes.ROWS it crosses
CROSSES = {
    "test_frames[WIDE]": ("small_x", "box_x"),
    "test_frames[TALL]": ("small_y", "box_y"),
    "test_x16k": ("dense_x",),
    "test_tile_counts[EXACT-DT]": ("fill_lds",),
    "test_tile_counts[LDS_TOP-DT]": ("bin_lds",),
    "test_tile_counts[LDS_TOP-exact]": ("hist_lds",),
    "test_tile_counts[ATOMIC-DT]": ("plan_lds", "scan_per"),
}

_SCENES, _CACHE = {}, {}


class Clock:
    """Prints the time of each step of a case (collected into profiles/large_targets/times.txt)."""
    def __init__(self, case):
        self.case, self.t = case, time.perf_counter()

    def __call__(self, what):
        now = time.perf_counter()
        print(f"TIME {self.case}: {what}: {now - self.t:.2f} s")
        self.t = now


def the_scene(oracle, name):
    """(scene, x extents, y extents) of a target, once; asserts that the scene is what the case needs."""
    if name not in _SCENES:
        w, h = TS.TARGETS.get(name, name)
        s = TS.scene(name)
        ex, ey = TS.extents(oracle, s.vertices, s.indices, IDENT, w, h)
        along = ex if w >= h else ey
        E = 16384 if max(w, h) < 32768 else 32768
        assert (along[list(s.pair)] == (E - 1, E)).all(), f"the pair's extents are {along[list(s.pair)]}"
        assert along[s.long[:6]].min() >= max(w, h) - 120 and along[s.long[:6]].max() >= max(w, h) - 6
        assert along[s.tied[:, 1]].min() >= max(w, h) - 120 and along[s.sliver] >= max(w, h) - 120
        sx, sy, _ = oracle.project(s.vertices, IDENT, w, h)
        assert int(sx[3 * s.corner]) == w - 1 and int(sy[3 * s.corner]) == h - 1, "a vertex in the last column and the last row"
        assert (along[list(s.pair2)] == (E - TS.TILE_H - 1, E - TS.TILE_H)).all(), f"the second pair's extents are {along[list(s.pair2)]}"
        assert s.indices.size // 3 == TS.SMALL_TRIANGLES + TS.LONG_TRIANGLES
        _SCENES[name] = (s, ex, ey)
    return _SCENES[name]


def spec_of(name, s, flags, **kw):
    w, h = TS.TARGETS.get(name, name)
    kw.setdefault("transform", IDENT)
    kw.setdefault("key", (name, "scene"))
    return FM.FrameSpec(s.vertices, s.indices, w, h, flags, **kw)


def expect(oracle, spec, start=None):
    return FM.expect(oracle, spec, start, _CACHE.setdefault(spec.key[0] if spec.key else None, {}))


def draw(ctx, spec):
    flags = spec.flags | (BLEND if spec.blend is not None else 0)
    if spec.blend is not None:
        ctx.blend_set(*spec.blend)
    if spec.items is not None:
        ctx.draw_list(spec.items, flags)
    else:
        ctx.draw(spec.transform, flags)
    ctx.sync()


def read(ctx, spec):
    return (None if spec.flags & NC else ctx.read_color(), ctx.read_depth(), ctx.read_ids() if spec.flags & IDS else None)


def check(ctx, oracle, spec, what, start=None):
    want = expect(oracle, spec, start)
    if start is not None:
        ctx.target_write(*start)
    draw(ctx, spec)
    FM.same(read(ctx, spec), want, what)
    return want


def shown(ids, n):
    """Pixels per triangle of an expected ID image."""
    ids = np.asarray(ids).reshape(-1)
    return np.bincount(ids[(ids >= 0) & (ids != K.NONE)], minlength=n)


def not_small(name, s, ex, ey):
    """The triangles that setup does not mark GEOM_SMALL (X16K: that the raster walks cooperatively for their x extent)."""
    w, h = TS.TARGETS.get(name, name)
    E = 16384 if max(w, h) < 32768 else 32768
    return np.nonzero((ex >= E) | (ey >= (E - TS.TILE_H if E == 32768 else 1 << 30)))[0]


def across_shift(name, pixels=2):
    """A translation by `pixels` across the long axis: the long triangles keep their extents."""
    w, h = TS.TARGETS.get(name, name)
    m = IDENT.copy()
    if w >= h:
        m[13] = np.float32(-2.0 * pixels / h)
    else:
        m[12] = np.float32(2.0 * pixels / w)
    return m


def list_items(name, s):
    """Three items: the small triangles before the long ones, the long ones shifted by two pixels, the rest."""
    a, b = 3 * int(s.long[0]), 3 * (int(s.sliver) + 1)
    return [(0, a, IDENT), (a, b - a, across_shift(name)), (b, s.indices.size - b, IDENT)]


def visible_not_small(oracle, name, s, ex, ey, flags=DT | IDS):
    """From the oracle: the not-small triangles are there in the number meant, and a z-tested frame shows their pixels."""
    big = not_small(name, s, ex, ey)
    w, h = TS.TARGETS.get(name, name)
    assert big.size >= ((10 if w >= h else 11) if max(w, h) > 32768 else 1), f"{big.size} triangles are not small"
    want = expect(oracle, spec_of(name, s, flags))
    n = shown(want[2], s.indices.size // 3)
    first = np.setdiff1d(big, np.concatenate([s.tied[:, 1], [s.sliver]]))        # (a z-tested tie goes to the earlier triangle)
    print(f"{name}: {big.size} triangles not small; pixels shown of each: {n[big]}")
    assert (n[first] >= 1000).all(), f"a not-small triangle shows {n[first].min()} pixels"
    assert (want[2][:, w - 1] == s.corner).any() and (want[2][h - 1] == s.corner).any(), "the last column and the last row show the corner triangle"
    return big


def last_column_pixel(d):
    """(x, y) of the lowest pixel of the last column that a fragment reached."""
    ys = np.nonzero(np.isfinite(d[:, -1]))[0]
    assert ys.size, "nothing is drawn in the last column"
    return d.shape[1] - 1, int(ys[-1])


# ---- 1. frames on WIDE and TALL -----------------------------------------------------------------------------------------------------
RULES = [("painter", 0), ("DT", DT), ("DT|NC", DT | NC), ("METAL", METAL), ("METAL|NC", METAL | NC), ("DT|IDS", DT | IDS),
         ("METAL|IDS", METAL | IDS)]


@gpu
@pytest.mark.parametrize("name", ["WIDE", "TALL"])
def test_frames(swr, oracle, name):
    """Every rule set, depth-only frames on 32-bit and on 64-bit keys, and ID frames, with ten not-small triangles visible: the
    cooperative walk with GeomFull in k_raster, k_raster_depth and the colour resolve, boxes with x1 (y1) up to 65534."""
    s, ex, ey = the_scene(oracle, name)
    w, h = TS.TARGETS[name]
    clock = Clock(f"test_frames[{name}]")
    visible_not_small(oracle, name, s, ex, ey)
    clock("scene and oracle IDs")
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        for what, flags in RULES:
            check(ctx, oracle, spec_of(name, s, flags), f"{name}, {what}")
            clock(what)
    with swr.Context(0) as ctx:
        ctx.debug_set(K.DEBUG_DEPTH_KEYS32, 0)
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        check(ctx, oracle, spec_of(name, s, DT | NC), f"{name}, DT|NC on 64-bit keys")
        clock("DT|NC, 64-bit keys")


FEATURES = [("DT|CB", DT | CB, 0), ("painter|CF|CCW|IDS", CF | CCW | IDS, 0), ("DT|CLIP", DT | CLIP, 0), ("DT|PERSP", DT | PERSP, 0),
            ("DT, shader 1", DT, 1), ("painter, shader 2", 0, 2), ("METAL|PERSP, shader 1", METAL | PERSP, 1)]


@gpu
@pytest.mark.parametrize("name", ["WIDE", "TALL"])
def test_features(swr, oracle, name):
    """Culling, depth clipping (a long triangle crosses the near plane), SWR_FLAG_PERSPECTIVE under an affine transform, the extended
    fragment stage, load frames over special depths and a three-item draw list, on the same scene."""
    s, ex, ey = the_scene(oracle, name)
    w, h = TS.TARGETS[name]
    clock = Clock(f"test_features[{name}]")
    big = not_small(name, s, ex, ey)
    z = s.vertices[s.indices.reshape(-1, 3)[big], 2]
    assert ((z.min(axis=1) < 0) & (z.max(axis=1) > 0)).sum() >= 1, "a not-small triangle crosses the near plane"
    areas = K.signed_areas(oracle, s.vertices, s.indices, IDENT, w, h, 0)
    assert (areas[big] > 0).sum() >= 2 and (areas[big] < 0).sum() >= 2, "not-small triangles of both windings"
    shading = {k: swr.scenes.random_shading(s.vertices.shape[0], 0x51 + k, k) for k in (1, 2)}
    start = K.special_start(w, h, 0x57B)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        for what, flags, shader in FEATURES:
            sh = shading.get(shader)
            ctx.shading_set(sh)
            check(ctx, oracle, spec_of(name, s, flags, shading=sh, key=(name, "scene", shader)), f"{name}, {what}")
            clock(what)
        ctx.shading_set(None)
        for what, flags in (("DT|LOAD", DT | LOAD), ("painter|LOAD|IDS", LOAD | IDS), ("METAL|NC|LOAD", METAL | NC | LOAD)):
            check(ctx, oracle, spec_of(name, s, flags), f"{name}, {what}", start=start)
            clock(what)
        items = list_items(name, s)
        lex, ley = TS.extents(oracle, *K.concat(s.vertices, s.indices, items), IDENT, w, h)
        assert not_small(name, s, lex, ley).size == big.size, "the shifted long triangles keep their extents"
        for what, flags in (("list, DT|IDS", DT | IDS), ("list, painter", 0)):
            check(ctx, oracle, spec_of(name, s, flags, items=items, key=(name, "list")), f"{name}, {what}")
            clock(what)


@gpu
@pytest.mark.parametrize("name,bands", [("WIDE", 2), ("TALL", 3)])
def test_bands(swr, oracle, name, bands):
    """Two bands of WIDE (the second starts at row 32 or 64) and three of TALL (y1 - row_begin of the later bands)."""
    s, ex, ey = the_scene(oracle, name)
    w, h = TS.TARGETS[name]
    clock = Clock(f"test_bands[{name}]")
    with swr.Context(0, device_count=bands) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        rows = [(a, b) for _, a, b in ctx.bands()]
        assert len(rows) == bands and rows[0][0] == 0 and rows[-1][1] == h and all(b > a for a, b in rows)
        for what, flags in (("DT", DT), ("METAL|IDS", METAL | IDS), ("painter", 0)):
            check(ctx, oracle, spec_of(name, s, flags), f"{name}, {bands} bands, {what}")
            clock(what)


# ---- 2. .vertices and lines -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["WIDE", "TALL"])
def test_points_and_lines(swr, oracle, name):
    """k_points, k_lines, k_points_resolve and k_clear_band with x (y) up to 65534: the scene's vertices as points, and its first two
    corners of every triangle as line segments, one of them 65 534 steps long."""
    s, ex, ey = the_scene(oracle, name)
    w, h = TS.TARGETS[name]
    clock = Clock(f"test_points_and_lines[{name}]")
    v = s.vertices.copy()
    L = max(w, h)
    far = K._ndc(np.array([0.5, L - 0.5]), np.array([5.5, 9.5]), w, h) if w >= h else K._ndc(np.array([5.5, 9.5]), np.array([0.5, L - 0.5]), w, h)
    v[0, 0:2], v[1, 0:2] = (far[0][0], far[1][0]), (far[0][1], far[1][1])
    lines = s.indices.reshape(-1, 3)[:, :2].reshape(-1)
    sx, sy, _ = oracle.project(v, IDENT, w, h)
    along = sx if w >= h else sy
    assert int(along[1]) - int(along[0]) == L - 1 == 65534, "a line of 65 534 steps"
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        for what, idx, ptype, flags in (("vertices", s.indices, VERTICES, 0), ("real lines", lines, LINE, REAL_LINES),
                                        ("line stub", lines, LINE, 0)):
            c, d, _, code = oracle.render(v, idx, IDENT, w, h, flags, primitive_type=ptype)
            assert code == 0
            landed = c[..., 3] == 255
            if what != "line stub":
                assert landed.sum() >= 1000 and (landed[:, -64:].any() if w >= h else landed[-32:].any())
            if what == "real lines":
                assert landed.sum() >= 65535, "the long line's pixels are in the expected image"
            ctx.scene_upload(v, idx)
            ctx.draw(IDENT, flags, ptype)
            ctx.sync()
            FM.same((ctx.read_color(), ctx.read_depth(), None), (c, d, None), f"{name}, {what}")
            clock(what)


# ---- 3. blend frames ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["WIDE", "TALL"])
def test_blend(swr, oracle, name):
    """k_raster_blend with not-small triangles: the long triangles alone (the model draws every primitive by itself), OVER and ADD,
    painter's order over a loaded image and z-tested."""
    s, ex, ey = the_scene(oracle, name)
    w, h = TS.TARGETS[name]
    clock = Clock(f"test_blend[{name}]")
    tri = np.concatenate([s.long, [s.corner], s.tied[:, 1]])
    idx = s.indices.reshape(-1, 3)[tri].reshape(-1)
    assert not_small(name, s, ex[tri], ey[tri]).size >= 9
    rng = np.random.default_rng(0xB1E)
    start = (rng.integers(0, 256, (h, w, 4), dtype=np.uint8), rng.uniform(0.3, 0.7, (h, w)).astype(np.float32))
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, idx)
        ctx.target_set(w, h)
        for what, flags, blend in (("OVER 150, painter, load", LOAD, (FM.OVER, 150)), ("ADD 90, z-tested, load", DT | LOAD, (FM.ADD, 90))):
            spec = FM.FrameSpec(s.vertices, idx, w, h, flags, transform=IDENT, key=(name, "long"), blend=blend)
            passed, rejected, who = FM.contributions(oracle, spec, start, _CACHE.setdefault(name, {}))
            assert who.size >= 9 and (passed >= 2).sum() >= 1000, "long triangles overlap: the order of the blends shows"
            assert not flags & DT or (rejected >= 1).sum() >= 1000
            want = expect(oracle, spec, start)
            ctx.target_write(*start)
            draw(ctx, spec)
            FM.same((ctx.read_color(), ctx.read_depth(), None), want, f"{name}, blend {what}")
            clock(what)


# ---- 4. queries on the frame just drawn ------------------------------------------------------------------------------------------------
def query_boxes(w, h, d):
    """Boxes of full length, 1 x 1 boxes at the far corner and boxes that end at x = w (y = h), each with several z."""
    rows = []
    x, y = last_column_pixel(d)
    zs = [np.float32(0.5), np.float32(0.3), np.float32(np.inf), d[y, x], np.nextafter(d[y, x], np.float32(-1))]
    for z in zs:
        rows += [(0, 0, w, h, z), (0, h // 2, w, h // 2 + 1, z), (w // 2, 0, w // 2 + 1, h, z), (w - 1, h - 1, w, h, z),
                 (x, y, x + 1, y + 1, z), (w - 70, max(0, h - 40), w, h, z), (w - 1, 0, w, h, z), (0, h - 1, w, h, z),
                 (3, 1, w - 5, h - 2, z)]
    return TDQ.as_boxes(rows)


@gpu
@pytest.mark.parametrize("name", ["WIDE", "TALL"])
def test_queries(swr, oracle, name):
    """swr_query_depth, swr_count_ids and swr_item_bounds on a z-tested ID draw-list frame; delta reads of colour and depth over two
    frames that differ only in the last tile."""
    s, ex, ey = the_scene(oracle, name)
    w, h = TS.TARGETS[name]
    n = s.indices.size // 3
    clock = Clock(f"test_queries[{name}]")
    items = list_items(name, s)
    spec = spec_of(name, s, DT | IDS, items=items, key=(name, "list"))
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        c, d, ids = check(ctx, oracle, spec, f"{name}, list frame")
        clock("list frame")
        boxes = query_boxes(w, h, d)
        want = TDQ.expected(d, boxes)
        assert np.unique(want).size >= 8 and list(want[4::9][2:]) == [0, 0, 1], "the 1 x 1 box in the last column passes just below its depth"
        got = ctx.query_depth(boxes)
        assert np.array_equal(got, want), f"{name}: swr_query_depth, boxes {np.nonzero(got != want)[0]}: {got} is not {want}"
        clock("query_depth")
        per = shown(ids, n)
        none = int((ids == K.NONE).sum())
        gc, gn = ctx.count_ids(COUNT_PER_PRIMITIVE)
        assert gn == none and np.array_equal(gc, per), f"{name}: swr_count_ids over the whole target"
        x, y = last_column_pixel(d)
        assert ids[y, x] != K.NONE
        for rect in ((x, y, x + 1, y + 1), (w - 1, h - 1, w, h), (w - 1, 0, w, h), (0, h - 1, w, h)):
            sub = ids[rect[1]:rect[3], rect[0]:rect[2]]
            gc, gn = ctx.count_ids(COUNT_PER_PRIMITIVE, rect)
            assert gn == int((sub == K.NONE).sum()) and np.array_equal(gc, shown(sub, n)), f"{name}: swr_count_ids in {rect}"
        bounds = np.cumsum([0] + [cnt // 3 for _, cnt, _ in items])
        gc, gn = ctx.count_ids(COUNT_PER_ITEM)
        assert gn == none and np.array_equal(gc, [per[bounds[k]:bounds[k + 1]].sum() for k in range(3)])
        clock("count_ids")
        for flags in (0, METAL):
            wb = IBM.item_bounds(s.vertices, s.indices, items, w, h, flags)
            assert (wb["x1"].max(), wb["y1"].max()) == (w, h) or flags, "an item reaches the last column and the last row"
            gb = ctx.item_bounds(items, flags)
            assert IBM.same(gb, wb), f"{name}: swr_item_bounds, flags {flags}: {gb} is not {wb}"
        clock("item_bounds")
        # two frames that differ only in the last tile: the corner triangle, nearer and in other colours
        v2 = s.vertices.copy()
        v2[3 * s.corner:3 * s.corner + 3, 2] = -0.5
        v2[3 * s.corner:3 * s.corner + 3, 4:7] = 1.0 - v2[3 * s.corner:3 * s.corner + 3, 4:7]
        spec2 = dataclasses.replace(spec_of(name, s, DT), vertices=v2, key=(name, "corner"))
        first, second = expect(oracle, spec_of(name, s, DT)), expect(oracle, spec2)
        ctx.draw(IDENT, DT)
        dst = [np.zeros((h, w, 4), np.uint8), np.zeros((h, w), np.float32)]
        for k, fn in enumerate((ctx.read_color_delta, ctx.read_depth_delta)):
            st = fn(dst[k])
            assert st.full == 1 and DM.as_words(dst[k]).tobytes() == DM.as_words(first[k]).tobytes()
        ctx.scene_upload(v2, s.indices)
        ctx.draw(IDENT, DT)
        for k, fn in enumerate((ctx.read_color_delta, ctx.read_depth_delta)):
            m, after = DM.delta(first[k], second[k], [(0, h)], dst[k])
            assert m.tiles_changed == 1 and m.rect == ((w - 1) // 64 * 64, (h - 1) // 32 * 32, w, h), m.rect
            st = fn(dst[k])
            assert (st.tiles, st.tiles_changed, st.full, st.rect) == (m.tiles, 1, 0, m.rect), (st.tiles, st.tiles_changed, st.rect)
            assert DM.as_words(dst[k]).tobytes() == after.tobytes() == DM.as_words(second[k]).tobytes()
        clock("delta reads")


@gpu
@pytest.mark.parametrize("name", ["WIDE", "TALL"])
def test_resolved_reads(swr, oracle, name):
    """k_resolve with S = 2 and S = 4 and both depth filters on 65532 x 96 and 96 x 65532."""
    size = TS.RESOLVED[name]
    s, ex, ey = the_scene(oracle, size)
    w, h = size
    clock = Clock(f"test_resolved_reads[{name}]")
    assert not_small(size, s, ex, ey).size >= 10
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        c, d, _ = check(ctx, oracle, spec_of(size, s, DT), f"{size}, DT")
        clock("frame")
        for S in (2, 4):
            rc = RM.color(c, S)
            assert RM.partial_fraction(rc) > 0.001 and rc[:, -1, 3].any() | rc[-1, :, 3].any()
            assert ctx.read_color_resolved(S).tobytes() == rc.tobytes(), f"{size}: colour, S = {S}"
            for filt in (K.RESOLVE_SAMPLE0, K.RESOLVE_MIN):
                assert ctx.read_depth_resolved(S, filt).tobytes() == RM.depth(d, S, filt).tobytes(), f"{size}: depth, S = {S}, filter {filt}"
            clock(f"S = {S}")


# ---- 5. the dense walk's bound ---------------------------------------------------------------------------------------------------------
@gpu
def test_x16k(swr, oracle):
    """16448 x 64: a triangle of x extent 16383 takes the dense walk, its twin of 16384 the cooperative one (both GEOM_SMALL)."""
    name = "X16K"
    s, ex, ey = the_scene(oracle, name)
    w, h = TS.TARGETS[name]
    row = TS.BY_KEY["dense_x"]
    assert (ex[list(s.pair)] == (row.below, row.above)).all() and ex.max() < 32768 and ey.max() < 32768
    visible_not_small(oracle, name, s, ex, ey)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        for what, flags in RULES:
            check(ctx, oracle, spec_of(name, s, flags), f"{name}, {what}")
        check(ctx, oracle, spec_of(name, s, DT, items=list_items(name, s), key=(name, "list")), f"{name}, list")


# ---- 6. tile counts ----------------------------------------------------------------------------------------------------------------------
KINDS = {"DT": DT, "DT|NC": DT | NC, "painter": 0, "METAL": METAL, "DT|IDS": DT | IDS}
TILE_CASES = [(name, kind) for name in ("EXACT", "LDS_TOP", "ATOMIC") for kind in list(KINDS) + ["list"]] + \
             [("LDS_TOP", "exact"), ("LDS_TOP", "bands")]
GRIDS = {"EXACT": 17408, "LDS_TOP": 34816, "ATOMIC": 35840}


def ids_once(oracle, s, w, h, depth):
    """The IDs of a z-tested frame from ONE colour-coded copy drawn by the oracle (kernel_matrix.coded; a z-tested frame has no LIVE
    pixels, and the copy's depth image must be the frame's own): half the oracle frames of kernel_matrix.expected_ids, decoded in
    32-bit words, for the 71-Mpixel targets."""
    cv, ci = K.coded(s.vertices, s.indices)
    c, d = K.oracle_clear(oracle, cv, ci, IDENT, w, h, DT)
    assert d.tobytes() == depth.tobytes(), "the coded copy's depth is not the frame's"
    ids = (c[..., 2] >> 1).astype(np.uint32)
    ids |= (c[..., 1] >> 1).astype(np.uint32) << 7
    ids |= (c[..., 0] >> 1).astype(np.uint32) << 14
    ids[c[..., 3] == 0] = K.NONE
    return ids


@gpu
@pytest.mark.parametrize("name,kind", TILE_CASES, ids=[f"{n}-{k}" for n, k in TILE_CASES])
def test_tile_counts(swr, oracle, name, kind):
    """17 408 tiles with exact-size bins (k_fill_lds asks for 70 656 bytes of LDS), 34 816 tiles (the last LDS size: k_bin asks for
    about 69.7 KB; with exact-size bins k_setup_hist does; once more as two bands) and 35 840 tiles (the plan itself takes the
    global-atomic chain; k_scan walks 35 tiles per thread).  One kind of resident frame per case, drawn twice (the second frame takes
    what the first learned: bin capacities, the deferred list), or one draw list; timings()["tiles"] is the grid's."""
    s, ex, ey = the_scene(oracle, name)
    w, h = TS.TARGETS[name]
    ntri, nt = s.indices.size // 3, TS.tiles(name)
    clock = Clock(f"test_tile_counts[{name}-{kind}]")
    assert nt == GRIDS[name] and not_small(name, s, ex, ey).size >= 10
    if name == "EXACT":
        assert TS.lds_bytes("k_fill_lds", nt, ntri) > TS.LDS_DEFAULT >= TS.lds_bytes("k_bin", nt, ntri)
    elif name == "LDS_TOP":
        assert min(TS.lds_bytes(k, nt, ntri) for k in ("k_bin", "k_fill_lds", "k_setup_hist")) > TS.LDS_DEFAULT and nt * 4 == 136 * 1024
    else:
        assert nt * 4 > 136 * 1024 and (nt + 1023) // 1024 == 35
    exact = name == "EXACT" or kind == "exact"
    with swr.Context(0, device_count=2 if kind == "bands" else 0) as ctx:
        if exact:
            ctx.debug_set(K.DEBUG_BIN_MODE, K.BIN_MODE_EXACT)
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        if kind == "bands":
            assert [(a, b) for _, a, b in ctx.bands()] == [(0, h // 2), (h // 2, h)]
        clock("context")
        if kind == "list":
            check(ctx, oracle, spec_of(name, s, DT, items=list_items(name, s), key=(name, "list")), f"{name}, list")
            clock("list frame")
            return
        ctx.timing_enable(1)
        for label in (("DT", "METAL") if kind in ("exact", "bands") else (kind,)):
            spec = spec_of(name, s, KINDS[label])
            want = expect(oracle, dataclasses.replace(spec, flags=spec.flags & ~IDS))
            ids = None
            if spec.flags & IDS:
                ids = ids_once(oracle, s, w, h, want[1])
                n = np.bincount(ids[ids != K.NONE], minlength=ntri)
                assert (n[np.setdiff1d(not_small(name, s, ex, ey), np.concatenate([s.tied[:, 1], [s.sliver]]))] >= 1000).all()
            clock(f"{label}: oracle")
            for k in range(1 if kind in ("exact", "bands") else 2):
                draw(ctx, spec)
                if kind != "bands":
                    assert ctx.timings()["tiles"] == nt, f"{ctx.timings()['tiles']} tiles"
                last = k == 1 or kind in ("exact", "bands")
                got = (None if spec.flags & NC or not last else ctx.read_color(), ctx.read_depth(), None)
                FM.same(got, want, f"{name}, {kind}, {label}, frame {k}")
                if ids is not None and last:
                    bad = np.nonzero(ctx.read_ids() != ids)
                    assert bad[0].size == 0, f"{name}, {label}: {bad[0].size} IDs differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"
            clock(f"{label}: frames")
