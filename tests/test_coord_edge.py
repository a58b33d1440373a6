"""Screen coordinates up to the skip rule's limit of 2^30 pixels on every kernel path (tests/coord_edge.py: the scenes;
tests/test_coord_edge_model.py pins their design on the CPU).  Each case draws the edge set of a target (about 25 far triangles with
corners up to the last float below +-2^30, mixed in index order into 200 small ones) or one of its variants and compares colour, depth
and IDs bit for bit with the oracle (kernel_matrix.expected_frame, frame_model.expect / model) or with item_bounds_model:

  raster rows   every raster row of K.ROWS on both targets, with the row's flags, material, hooks, sorts, LOAD start image and IDS
                pair; rows that only a scene beyond 2^20 primitives reaches draw the padded edge set;
  bin rows      every k_bin row and K.PATH_ROWS: the edge set under an affine transform (AFF rows) or the perspective variant under
                K.perspective_matrix(), as a draw or as a 3-item draw list with one mirrored item, with the row's cull bits;
  blend rows    the far triangles and a part of the small ones against frame_model's per-primitive model;
  other flags   SWR_FLAG_PERSPECTIVE and SWR_FLAG_DEPTH_CLIP over the perspective variant;
  points, lines .vertices frames with points at the limit, just inside it and at the decades; real-line frames with lines of 2^20 and
                2^20 + 1 steps, a start beyond 2^24 and an endpoint at exactly 2^30;
  item bounds   one item per far class under flags 0 and METAL;
  three bands   the edge set on three bands, and a 64-slot group with one NaN corner whose other triangles show in the top band while
                (0, 0, 0) projects into the bottom one (the box poison).
"""
import numpy as np
import pytest

import coord_edge as CE
import frame_model as FM
import item_bounds_model as IBM
import kernel_matrix as K

pytestmark = pytest.mark.gpu

NAMES = ("wide", "tall")
RASTER_ROWS = [r for r in K.ROWS if not r.name.startswith("k_bin<")]
BIN_ROWS = [r for r in K.ROWS if r.name.startswith("k_bin<")] + K.PATH_ROWS
BLEND_RASTER_ROWS = [r for r in K.BLEND_ROWS if r.name.startswith("k_raster_blend<")]
LINE, VERTICES = 1, 2
# far corners sit at NDC of about 2^23, where a translation of a few hundredths is below half an ulp: they keep their coordinates,
# the corners on the target move by a few pixels (to the right and down: nothing turns negative under the Metal rules)
AFFINE = K.affine_matrix(0.0, 1.0, 0.03, -0.02)
AFFINE2 = K.affine_matrix(0.0, 1.0, 0.05, -0.04)
BEHIND = K.perspective_matrix(-2.5)            # w = 1 - 2.5 z
START = {name: K.special_start(w, h, 0xC57A + k) for k, (name, (w, h)) in enumerate(CE.TARGETS.items())}
_PADDED, _SHADING, _CACHE = {}, {}, {}


def padded_set(name, flags):
    key = (name, bool(flags & K.METAL))
    if key not in _PADDED:
        fs = CE.rules_set(name, flags)
        v, i, far = CE.padded(fs)
        _PADDED[key] = CE.FarSet(v, i, far, fs.cls, ())
    return _PADDED[key]


def shading(swr, fs, shader):
    if shader == 0:
        return None
    key = (id(fs), shader)
    if key not in _SHADING:
        _SHADING[key] = swr.scenes.random_shading(fs.vertices.shape[0], 0xC0E, shader)
    return _SHADING[key]


def check(ctx, flags, want, what):
    """Reads the frame back and compares it with a kernel_matrix.Expected; returns (colour or None, depth)."""
    ctx.sync()
    got = (None if flags & K.NC else ctx.read_color(), ctx.read_depth(), ctx.read_ids() if flags & K.IDS else None)
    FM.same(got, (want.color, want.depth, want.ids), what)
    return got[0], got[1]


def far_shown(want, fs, what, floor=2000):
    """The frame the case compares with shows the far triangles (by its expected IDs)."""
    n = CE.shown(want.ids, max(fs.triangles, int(fs.far.max()) + 1))
    assert n[fs.far].sum() >= floor, f"{what}: the far triangles show {n[fs.far].sum()} pixels"
    return n


# ---- raster rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", RASTER_ROWS, ids=[r.name for r in RASTER_ROWS])
def test_raster_kernel(swr, oracle, row):
    for scene_name in row.scenes:
        for name in NAMES:
            w, h = CE.TARGETS[name]
            fs = padded_set(name, row.flags) if scene_name == "padded" else CE.rules_set(name, row.flags)
            sh = shading(swr, fs, row.shader)
            want = CE.frame(oracle, fs, name, row.flags, start=START[name], shading=sh, key=scene_name)
            what = f"{row.name}, {scene_name}, {name}"
            n = far_shown(want, fs, what, 1000 if row.load else 5000)
            if scene_name == "padded":       # far triangles on both sides of the filler show; the last triangle is number 2^20
                behind = fs.far[fs.far > 1 << 19]
                assert fs.triangles == K.PADDED_TRIANGLES and n[behind].sum() >= 100 and n[fs.far[fs.far < 1 << 19]].sum() >= 100, what

            def fresh(extra=()):
                ctx = swr.Context(0)
                for key, value in row.hooks + extra:
                    ctx.debug_set(key, value)
                ctx.scene_upload(fs.vertices, fs.indices)
                if sh is not None:
                    ctx.shading_set(sh)
                ctx.target_set(w, h)
                return ctx

            def draw(ctx, flags, label):
                if row.load:
                    c0, d0 = START[name]
                    ctx.target_write(None if flags & K.NC else c0, d0)
                ctx.draw(K.IDENT, flags)
                return check(ctx, flags, want, label)

            if row.sorts:
                for sort in row.sorts:
                    with fresh(((K.DEBUG_RASTER_SORT, sort),)) as ctx:
                        draw(ctx, row.flags, f"{what}, sort {sort}")
                continue
            with fresh() as ctx:
                c, d = draw(ctx, row.flags, what)
                if row.ids:          # colour and depth do not depend on the flag
                    c2, d2 = draw(ctx, row.flags & ~K.IDS, what + ", without IDS")
                    assert d2.tobytes() == d.tobytes() and (c is None or np.array_equal(c2, c)), what


# ---- bin rows ------------------------------------------------------------------------------------------------------------------------
def bin_scene(oracle, row, name):
    """(set, matrix of a draw, items of a draw list) of a binning row."""
    if row.affine:
        fs, m, m2 = CE.rules_set(name, row.flags), AFFINE, AFFINE2
    else:
        fs, m, m2 = CE.perspective_set(oracle, name), K.perspective_matrix(), AFFINE
    n = fs.triangles
    a, b = n // 2, n // 8
    return fs, m, [(0, 3 * a, m), (3 * a, 3 * (n - a), m2), (3 * b, 3 * (n // 2), K.mirrored(m))]


@pytest.mark.parametrize("row", BIN_ROWS, ids=[r.name for r in BIN_ROWS])
def test_binning_kernel(swr, oracle, row):
    for name in NAMES:
        w, h = CE.TARGETS[name]
        fs, m, items = bin_scene(oracle, row, name)
        cache = _CACHE.setdefault((row.name, name), {})
        if row.draw_list:
            cv, ci = K.concat(fs.vertices, fs.indices, items)
            want = K.expected_frame(oracle, cv, ci, K.IDENT, w, h, row.flags, cache=cache)
            total = ci.size // 3
        else:
            want = K.expected_frame(oracle, fs.vertices, fs.indices, m, w, h, row.flags, cache=cache)
            total = fs.triangles
        what = f"{row.name}, {name}"
        if row.flags & (K.CB | K.CF):
            assert 0 < want.kept.size < total, f"{what}: nothing culled"
        n = CE.shown(want.ids, total)
        # (a draw list's IDs count through its items: the first item's triangles keep their numbers)
        if row.affine:
            assert n[fs.far].sum() >= 3000, f"{what}: the far triangles show {n[fs.far].sum()} pixels"
        elif not row.draw_list:
            assert n[fs.of("p")].sum() >= 50 and n[fs.of("q")].sum() == 0, f"{what}: {n[fs.far]}"
        assert n.sum() >= 5000, what
        with swr.Context(0) as ctx:
            for key, value in row.hooks:
                ctx.debug_set(key, value)
            ctx.scene_upload(fs.vertices, fs.indices)
            ctx.target_set(w, h)
            for frame in range(2 if row.defer else 1):
                if row.draw_list:
                    ctx.draw_list(items, row.flags)
                else:
                    ctx.draw(m, row.flags)
                check(ctx, row.flags, want, f"{what}, frame {frame}")


# ---- blend rows ----------------------------------------------------------------------------------------------------------------------
def blend_part(fs):
    """The far triangles and every third small one, in the set's order."""
    t = np.arange(fs.triangles)
    sel = t[np.isin(t, fs.far) | (t % 3 == 0)]
    return fs.indices.reshape(-1, 3)[sel].reshape(-1), np.nonzero(np.isin(sel, fs.far))[0]


@pytest.mark.parametrize("row", BLEND_RASTER_ROWS, ids=[r.name for r in BLEND_RASTER_ROWS])
def test_blend_kernel(swr, oracle, row):
    for name in NAMES:
        w, h = CE.TARGETS[name]
        fs = CE.rules_set(name, row.flags)
        idx, far = blend_part(fs)
        start = START[name] if row.load else None
        cache = _CACHE.setdefault(("blend", name), {})
        spec = FM.FrameSpec(fs.vertices, idx, w, h, row.flags, transform=K.IDENT, key=("coord edge blend", name, bool(row.flags & K.METAL)))
        want = FM.model(oracle, spec, row.mode, row.opacity, start, cache)
        passed, rejected, who = FM.contributions(oracle, spec, start, cache)
        assert np.isin(far, who).sum() >= 10 and (passed >= 3).sum() >= 5000, f"{row.name}, {name}: far triangles blend over each other"
        with swr.Context(0) as ctx:
            ctx.scene_upload(fs.vertices, idx)
            ctx.target_set(w, h)
            ctx.blend_set(row.mode, row.opacity)
            if row.load:
                ctx.target_write(*START[name])
            ctx.draw(K.IDENT, row.flags | K.BLEND)
            ctx.sync()
            FM.same((ctx.read_color(), ctx.read_depth(), None), (want[0], want[1], None), f"{row.name}, {name}")


# ---- SWR_FLAG_PERSPECTIVE, SWR_FLAG_DEPTH_CLIP ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,flags", [("PERSP", K.DT | FM.PERSP), ("PERSP, METAL", K.METAL | FM.PERSP), ("CLIP", K.DT | FM.CLIP),
                                        ("CLIP, painter, IDS", FM.CLIP | K.IDS)])
def test_other_flags_over_the_perspective_variant(swr, oracle, what, flags):
    for name in NAMES:
        w, h = CE.TARGETS[name]
        fs = CE.perspective_set(oracle, name)
        m = K.perspective_matrix()
        spec = FM.FrameSpec(fs.vertices, fs.indices, w, h, flags, transform=m, key=("coord edge persp", name))
        want = FM.expect(oracle, spec, None, _CACHE.setdefault(("persp", name), {}))
        assert (np.isfinite(want[1]) if flags & (K.DT | K.METAL) else want[0][..., 3] == 255).sum() >= 3000
        with swr.Context(0) as ctx:
            ctx.scene_upload(fs.vertices, fs.indices)
            ctx.target_set(w, h)
            ctx.draw(m, flags)
            ctx.sync()
            FM.same((ctx.read_color(), ctx.read_depth(), ctx.read_ids() if flags & K.IDS else None), want, f"{what}, {name}")


# ---- points and lines ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_points_and_lines(swr, oracle, name):
    """k_points and k_lines: the skip rule at the limit (tests/test_coord_edge_model.py checks what each point and line is)."""
    w, h = CE.TARGETS[name]
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        for what, (v, i), ptype, flags in (("vertices", CE.point_scene(name), VERTICES, 0),
                                           ("real lines", CE.line_scene(name), LINE, CE.REAL_LINES)):
            c, d, _, code = oracle.render(v, i, K.IDENT, w, h, flags, primitive_type=ptype)
            assert code == 0 and (c[..., 3] == 255).sum() >= 250
            ctx.scene_upload(v, i)
            ctx.draw(K.IDENT, flags, ptype)
            ctx.sync()
            FM.same((ctx.read_color(), ctx.read_depth(), None), (c, d, None), f"{name}, {what}")
        # each line by itself: a line the frame wrongly drew or dropped cannot hide behind a later one
        v, i = CE.line_scene(name)
        for k in range(i.size // 2):
            c, d, _, code = oracle.render(v, i[2 * k:2 * k + 2], K.IDENT, w, h, CE.REAL_LINES, primitive_type=LINE)
            ctx.scene_upload(v, i[2 * k:2 * k + 2])
            ctx.draw(K.IDENT, CE.REAL_LINES, LINE)
            ctx.sync()
            FM.same((ctx.read_color(), ctx.read_depth(), None), (c, d, None), f"{name}, line {k}")


# ---- item bounds ---------------------------------------------------------------------------------------------------------------------
def class_items(fs, transforms):
    """(index array with the far triangles grouped by class, then the small ones; one item per class, one for the rest, and the rest
    again behind the eye)."""
    t = fs.indices.reshape(-1, 3)
    order, items, at = [], [], 0
    for k, cls in enumerate(sorted(set(fs.cls))):
        tri = fs.of(cls)
        order.append(tri)
        items.append((3 * at, 3 * tri.size, transforms[k % len(transforms)]))
        at += tri.size
    rest = np.setdiff1d(np.arange(fs.triangles), fs.far)
    order.append(rest)
    items.append((3 * at, 3 * rest.size, transforms[0]))
    items.append((3 * at, 3 * rest.size, BEHIND))          # the small ones once more, those with z > 0.4 behind the eye
    return t[np.concatenate(order)].reshape(-1), items


@pytest.mark.parametrize("name", NAMES)
def test_item_bounds(swr, oracle, name):
    """k_item_bounds: rectangles, depth ranges and the drawable / skipped / behind counts of one item per far class."""
    w, h = CE.TARGETS[name]
    for flags in (0, K.METAL):
        sets = [(CE.rules_set(name, flags), [K.IDENT, AFFINE]), (CE.perspective_set(oracle, name), [K.perspective_matrix()])]
        for fs, transforms in sets:
            idx, items = class_items(fs, transforms)
            want = IBM.item_bounds(fs.vertices, idx, items, w, h, flags)
            if len(transforms) == 2:
                assert want["skipped"][:-2].sum() >= 4 and want["drawable"][:-2].sum() >= 15 and want["drawable"][-2] >= 180
                assert want["behind"][-1] >= 10 and want["behind"][:-1].sum() == 0
                assert ((want["x1"] - want["x0"] >= w - 30) & (want["y1"] - want["y0"] >= h - 30)).sum() >= 3, "items that cover the target"
                assert ((want["drawable"] == 0) & (want["skipped"] > 0)).sum() >= 1, "an item with skipped triangles only (class e)"
            with swr.Context(0) as ctx:
                ctx.scene_upload(fs.vertices, idx)
                ctx.target_set(w, h)
                got = ctx.item_bounds(items, flags)
            assert IBM.same(got, want), f"{name}, flags {flags}: {got} is not {want}"


# ---- three bands ---------------------------------------------------------------------------------------------------------------------
def test_three_bands(swr, oracle):
    name = "tall"
    w, h = CE.TARGETS[name]
    for flags in (K.DT, K.METAL, K.DT | K.NC, 0):
        fs = CE.rules_set(name, flags)
        want = CE.frame(oracle, fs, name, flags)
        with swr.Context(0, device_count=3) as ctx:
            ctx.scene_upload(fs.vertices, fs.indices)
            ctx.target_set(w, h)
            rows = [(a, b) for _, a, b in ctx.bands()]
            assert len(rows) == 3 and rows[0][0] == 0 and rows[-1][1] == h
            ctx.draw(K.IDENT, flags)
            check(ctx, flags, want, f"three bands, flags {flags}")


def poison_scene(w, h):
    """128 triangles in the caller's order, the groups of 64 slots: group 0 is one triangle with a NaN corner and 63 small ones that
    show in the top band; group 1 shows in the bottom band.  The transform moves the model by -0.8 in NDC y, so the model's (0, 0, 0)
    lands at 0.9 h, in the bottom band, and the first group's own box, y in [1.2, 1.7], in the top one."""
    rng = np.random.default_rng(0xB0C5)
    xyz, rgb = K._tris(rng, 128, 8, 0.05 * h, w - 8, 0.25 * h, 10, 0.1, 0.9, w, h)
    xyz = xyz.reshape(128, 3, 3)
    xyz[64:, :, 1] -= 1.4                      # the second group: 0.7 h further down
    xyz[..., 1] += 0.8
    xyz[0, 1, 0] = np.nan
    m = K.IDENT.copy()
    m[13] = -0.8
    return K._pack(xyz.reshape(-1, 3), rgb), np.arange(384, dtype=np.int64), m


@pytest.mark.parametrize("flags", [K.DT, K.METAL, 0], ids=["ztest", "metal", "painter"])
def test_nan_corner_does_not_cull_its_group(swr, oracle, flags):
    """Finding (3) of profiles/shared_rules/mutations.txt: a group with a coordinate that is not finite gets a NaN box, which no band
    culls.  A box of (0, 0, 0) - (0, 0, 0) instead would project into the bottom band here and cull the group from the top one."""
    name = "tall"
    w, h = CE.TARGETS[name]
    v, i, m = poison_scene(w, h)
    want = K.expected_frame(oracle, v, i, m, w, h, flags | K.IDS)
    n = CE.shown(want.ids, 128)
    with swr.Context(0, device_count=3) as ctx:
        ctx.debug_set(K.DEBUG_STREAM_ORDER, 0)
        ctx.scene_upload(v, i)
        ctx.target_set(w, h)
        rows = [(a, b) for _, a, b in ctx.bands()]
        assert len(rows) == 3
        top = CE.shown(want.ids[rows[0][0]:rows[0][1]], 128)
        assert n[0] == 0 and (top[1:64] > 0).sum() >= 50 and top[1:64].sum() >= 1500, "group 0 shows in the top band"
        assert n[64:].sum() >= 1500 and top[64:].sum() == 0 and rows[2][0] <= int(0.9 * h) < rows[2][1], "(0, 0, 0) lands in the bottom band"
        ctx.draw(m, flags | K.IDS)
        check(ctx, flags | K.IDS, want, f"NaN corner, flags {flags}")
