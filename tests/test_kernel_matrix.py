"""Every raster and binning kernel instantiation once, bit for bit against the oracle (tests/kernel_matrix.py: the rows, the scenes,
the expectations).

Raster rows draw the visible set (below 2^20 primitives: the winner-table kernels) or the same set padded with off-screen filler
to 2^20 + 1 primitives (the PLAIN kernels; the filler sits in the middle, so the last visible triangle is number 2^20), on a small
ragged target and on one of 460 tiles.  LOAD rows start from a swr_target_write image with NaN (one with a payload), +-0, +-inf,
+-denormals and ordinary depths.  IDS rows also draw the frame without the flag and compare: colour and depth are the same.
Binning rows (k_bin) draw with affine and perspective transforms, as draws and as 3-item draw lists (one item mirrored), with face
culling on some; DEFER rows are drawn twice on the large target, and both frames are checked.
Blend rows (K.BLEND_ROWS) draw a part of the visible set, alone and padded to 2^20 + 1 primitives, against the per-primitive blend
model of tests/frame_model.py; resolve rows (K.RESOLVE_ROWS) resolve injected images against tests/resolve_model.py.
"""
import numpy as np
import pytest

import frame_model as FM
import kernel_matrix as K
import resolve_model as RM
import test_blend as TB
import test_resolve as TR

pytestmark = pytest.mark.gpu

RASTER_ROWS = [r for r in K.ROWS if not r.name.startswith("k_bin<")]
BIN_ROWS = [r for r in K.ROWS if r.name.startswith("k_bin<")] + K.PATH_ROWS

_SCENES = {}


def scene(name, target):
    """(vertices, indices, first triangle of the tail, visible set, expectation cache) of a scene on a target, built once."""
    key = (name, target)
    if key not in _SCENES:
        w, h = K.TARGETS[target]
        vs = K.visible_set(w, h)
        v, i, first = vs.vertices, vs.indices, vs.n_head
        if name == "padded":
            v, i, first = K.padded(v, i, vs.n_head, K.PADDED_TRIANGLES)
        _SCENES[key] = (v, i, first, vs, {})
    return _SCENES[key]


def shading(swr, nv, shader):
    return None if shader == 0 else swr.scenes.random_shading(nv, 0x3A7, shader)


START = {t: K.special_start(w, h, 0x57A + k) for k, (t, (w, h)) in enumerate(K.TARGETS.items())}


def check(ctx, flags, want, what):
    """Reads the frame back and compares it with the expectation; returns (colour or None, depth, IDs or None)."""
    ctx.sync()
    d = ctx.read_depth()
    bad = np.nonzero(d.view(np.uint32) != want.depth.view(np.uint32))
    assert bad[0].size == 0, f"{what}: {bad[0].size} depth values differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"
    c = None
    if not flags & K.NC:
        c = ctx.read_color()
        bad = np.nonzero((c != want.color).any(axis=-1))
        assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"
    ids = None
    if flags & K.IDS:
        ids = ctx.read_ids()
        assert (ids[want.ids == K.LIVE] != K.NONE).all(), what
        bad = np.nonzero((ids != want.ids) & (want.ids >= 0))
        assert bad[0].size == 0, (f"{what}: {bad[0].size} IDs differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): "
                                  f"{ids[bad][0]} vs {want.ids[bad][0]}")
    return c, d, ids


def non_vacuous(row, want, first, vs, padded, what):
    """The frame meets what its row is there for."""
    r = want.ids
    hit = (r >= 0) & (r != K.NONE)
    assert hit.sum() > 1000, what
    if padded:                               # numbers from 2^20 on are visible (the PLAIN kernels' keys)
        assert (r[hit] >= 1 << K.PRIM_BITS).any(), what
    shift = first - vs.n_head
    if row.flags & (K.DT | K.METAL):         # exact ties decided for the earlier index
        assert np.isin(r, vs.tied[:, 0]).sum() > 100, what
    else:                                    # ... and for the later one under painter's order
        assert np.isin(r, vs.tied[:, 1] + shift).sum() > 100, what
    if row.load:                             # the loaded image wins some pixels the frame covers, the frame wins others
        clear_hit = (want.clear_ids >= 0) & (want.clear_ids != K.NONE)
        if row.flags & (K.DT | K.METAL):
            assert (clear_hit & (r == K.NONE)).sum() > 100, what
        assert (clear_hit & (r != K.NONE)).sum() > 1000, what


def draw_and_check(ctx, row, flags, want, target, what):
    if row.load:
        c0, d0 = START[target]
        ctx.target_write(None if flags & K.NC else c0, d0)
    ctx.draw(K.IDENT, flags)
    return check(ctx, flags, want, what)


@pytest.mark.parametrize("row", RASTER_ROWS, ids=[r.name for r in RASTER_ROWS])
def test_raster_kernel(swr, oracle, row):
    for scene_name in row.scenes:
        for target in row.targets:
            v, i, first, vs, cache = scene(scene_name, target)        # (the visible set is laid out in the target's tiles)
            w, h = K.TARGETS[target]
            sh = shading(swr, v.shape[0], row.shader)
            want = K.expected_frame(oracle, v, i, K.IDENT, w, h, row.flags, sh, START[target], cache)
            what = f"{row.name}, {scene_name}, {target}"
            non_vacuous(row, want, first, vs, scene_name == "padded", what)

            def fresh(extra=()):
                ctx = swr.Context(0)
                for key, value in row.hooks + extra:
                    ctx.debug_set(key, value)
                ctx.scene_upload(v, i)
                if sh is not None:
                    ctx.shading_set(sh)
                ctx.target_set(w, h)
                return ctx

            if row.sorts:
                # the 32-bit depth keys: the first frame of a fresh context (a frame with many redone tiles, like one over
                # loaded zeros, moves the scene to the 64-bit kernel for good), once with the bins sorted by k_sort_bins, once
                # inside the raster workgroups
                for sort in row.sorts:
                    with fresh(((K.DEBUG_RASTER_SORT, sort),)) as ctx:
                        draw_and_check(ctx, row, row.flags, want, target, f"{what}, sort {sort}")
                continue
            with fresh() as ctx:
                c, d, _ = draw_and_check(ctx, row, row.flags, want, target, what)
                if row.ids:          # the header's promise: colour and depth do not depend on the flag
                    c2, d2, _ = draw_and_check(ctx, row, row.flags & ~K.IDS, want, target, what + ", without IDS")
                    assert d2.tobytes() == d.tobytes() and (c is None or np.array_equal(c2, c)), what


def list_items(row, n):
    """Three items of the visible set's index array: two ranges that split it, and an instance of a part of it, mirrored."""
    m1 = K.affine_matrix()
    m2 = K.affine_matrix(-0.05, 1.02, -0.02, 0.01) if row.affine else K.perspective_matrix()
    a, b = n // 2, n // 5
    return [(0, 3 * a, m1), (3 * a, 3 * (n - a), m2), (3 * b, 3 * 400, K.mirrored(m1))]


@pytest.mark.parametrize("row", BIN_ROWS, ids=[r.name for r in BIN_ROWS])
def test_binning_kernel(swr, oracle, row):
    assert row.metal == bool(row.flags & K.METAL)
    for target in row.targets:
        w, h = K.TARGETS[target]
        v, i, first, vs, _ = scene("visible", target)
        m = K.affine_matrix() if row.affine else K.perspective_matrix()
        if row.draw_list:
            items = list_items(row, i.size // 3)
            cv, ci = K.concat(v, i, items)
            want = K.expected_frame(oracle, cv, ci, K.IDENT, w, h, row.flags)
        else:
            want = K.expected_frame(oracle, v, i, m, w, h, row.flags)
        what = f"{row.name}, {target}"
        if row.flags & (K.CB | K.CF):
            assert 0 < want.kept.size < (ci.size if row.draw_list else i.size) // 3, f"{what}: nothing culled"
        hit = (want.ids >= 0) & (want.ids != K.NONE)
        assert hit.sum() > 1000, what
        with swr.Context(0) as ctx:
            for key, value in row.hooks:
                ctx.debug_set(key, value)
            ctx.scene_upload(v, i)
            ctx.target_set(w, h)
            # DEFER: the first frame meets triangles that cover hundreds of tiles; the second one defers them to k_sort_bins
            for frame in range(2 if row.defer else 1):
                if row.draw_list:
                    ctx.draw_list(items, row.flags)
                else:
                    ctx.draw(m, row.flags)
                check(ctx, row.flags, want, f"{what}, frame {frame}")


# ---- the blend kernels (K.BLEND_ROWS) ------------------------------------------------------------------------------------------------
BLEND_RASTER_ROWS = [r for r in K.BLEND_ROWS if r.name.startswith("k_raster_blend<")]
_BLEND = {}         # the blend scene and frame_model's per-primitive images of it, shared by the rows


def meets_target(oracle, v, i, w, h):
    """Per triangle: its projected bounding box meets the target (one pixel of margin: a primitive that does not, drawn alone,
    covers nothing, so leaving it out of the per-primitive model is exact)."""
    sx, sy, _ = oracle.project(v, K.IDENT, w, h)
    t = np.asarray(i, dtype=np.int64).reshape(-1, 3)
    x, y = sx[t].astype(np.float64), sy[t].astype(np.float64)
    ok = np.isfinite(x).all(axis=1) & np.isfinite(y).all(axis=1)
    with np.errstate(invalid="ignore"):
        return ok & (x.max(axis=1) >= -1) & (x.min(axis=1) <= w + 1) & (y.max(axis=1) >= -1) & (y.min(axis=1) <= h + 1)


def blend_scene(oracle):
    """A part of the visible set on the small target the per-primitive model can afford (at most 1 500 primitives), in the set's
    order: the big triangles, the sparse tile, the medium ones with the tied duplicates that meet the target, a part of the busy and of the
    crowded tile, the slivers, the nearer triangles and the last one; and the same padded to 2^20 + 1 primitives."""
    if "scene" not in _BLEND:
        w, h = K.TARGETS["small"]
        vs = K.visible_set(w, h)
        nh = vs.n_head
        n = vs.indices.size // 3
        sel = set(range(0, 305)) | set(range(305, 505)) | set(range(805, 1005)) | set(range(3105, nh))
        sel |= set(vs.tied.reshape(-1).tolist()) | set(range(nh + 64, nh + 64 + 40 + 100)) | {n - 3, n - 2, n - 1}
        sel = np.array(sorted(sel), dtype=np.int64)
        t = vs.indices.reshape(-1, 3)
        sel = sel[meets_target(oracle, vs.vertices, t[sel].reshape(-1), w, h)]
        assert 800 < sel.size <= 1500
        tied = np.stack([np.searchsorted(sel, vs.tied[:, 0]), np.searchsorted(sel, vs.tied[:, 1])], axis=1)
        both = np.isin(vs.tied[:, 0], sel) & np.isin(vs.tied[:, 1], sel)
        assert both.sum() > 50
        i = t[sel].reshape(-1)
        n_head = int((sel < nh).sum())
        pv, pi, first = K.padded(vs.vertices, i, n_head, K.PADDED_TRIANGLES)
        seen = np.nonzero(meets_target(oracle, pv, pi, w, h))[0]
        # the modelled primitives of the padded scene are the visible ones, in their order
        assert seen.size == sel.size and np.array_equal(pv[pi.reshape(-1, 3)[seen]], vs.vertices[i.reshape(-1, 3)])
        assert seen[-1] == 1 << K.PRIM_BITS
        _BLEND["scene"] = (vs.vertices, i, tied[both], pv, pi, seen)
    return _BLEND["scene"]


def same_images(got, want, what):
    FM.same((got[0], got[1], None), (want[0], want[1], None), what)


@pytest.mark.parametrize("row", BLEND_RASTER_ROWS, ids=[r.name for r in BLEND_RASTER_ROWS])
def test_blend_kernel(swr, oracle, row):
    w, h = K.TARGETS["small"]
    v, i, tied, pv, pi, seen = blend_scene(oracle)
    start = START["small"] if row.load else None
    spec = FM.FrameSpec(v, i, w, h, row.flags, transform=K.IDENT, key="blend rows")
    want = FM.model(oracle, spec, row.mode, row.opacity, start, _BLEND)
    # the frame meets what its row is there for
    passed, rejected, who = FM.contributions(oracle, spec, start, _BLEND)
    assert (passed >= 3).sum() > 1000, row.name
    assert np.isin(tied[:, 0], who).sum() > 20 and np.isin(tied[:, 1], who).sum() > 20, row.name
    if row.load and row.flags & (K.DT | K.METAL):
        assert (rejected > 0).sum() > 100 and (passed > 0).sum() > 1000, row.name
    assert (seen[who] >= 1 << K.PRIM_BITS).any(), "no primitive numbered 2^20 or more contributes in the padded scene"
    assert not np.array_equal(want[0], np.zeros_like(want[0]) if start is None else start[0])

    def draw(ctx, flags, target):
        if row.load:
            ctx.target_write(*START[target])
        ctx.draw(K.IDENT, flags)
        ctx.sync()
        return ctx.read_color(), ctx.read_depth()

    for name, (sv, si) in (("visible", (v, i)), ("padded", (pv, pi))):
        with swr.Context(0) as ctx:
            ctx.scene_upload(sv, si)
            ctx.target_set(w, h)
            ctx.blend_set(row.mode, row.opacity)
            same_images(draw(ctx, row.flags | K.BLEND, "small"), want, f"{row.name}, {name}, small")
    # the large target has no per-primitive model: library against library, on the whole visible set
    W, H = K.TARGETS["large"]
    lv, li, _, _, _ = scene("visible", "large")
    d0 = START["large"][1] if row.load else np.full((H, W), np.inf, dtype=np.float32)
    with swr.Context(0) as ctx:
        ctx.scene_upload(lv, li)
        ctx.target_set(W, H)
        if not row.flags & (K.DT | K.METAL):
            # (a) OVER with opacity 255 and no z-test: the colour of the k_raster painter row's frame
            plain = draw(ctx, row.flags, "large")
            ctx.blend_set(K.BLEND_OVER, 255)
            c, d = draw(ctx, row.flags | K.BLEND, "large")
            assert np.array_equal(c, plain[0]) and d.tobytes() == d0.tobytes(), f"{row.name}, large: property (a)"
        else:
            # (c) one z-tested blend frame is the chain of its sub-ranges (depth never changes)
            ctx.blend_set(row.mode, row.opacity)
            whole = draw(ctx, row.flags | K.BLEND, "large")
            if row.load:
                ctx.target_write(*START["large"])
            n = li.size // 3
            cuts = [0, n // 4, n // 2, 3 * n // 4, n]
            for k in range(4):
                ctx.draw_list([(3 * cuts[k], 3 * (cuts[k + 1] - cuts[k]), K.IDENT)], row.flags | K.BLEND | (K.LOAD if k else 0))
            ctx.sync()
            assert np.array_equal(ctx.read_color(), whole[0]) and ctx.read_depth().tobytes() == whole[1].tobytes() == d0.tobytes(), \
                f"{row.name}, large: property (c)"
            assert whole[0].any()


@pytest.mark.parametrize("flags", [0, K.DT], ids=["painter", "ztest"])
def test_blend_order_kernel(swr, flags):
    """k_blend_order on a bin of more than one sorted run (5 000 triangles in one tile) under every stream order: the order numbers
    come from the geometry records (reordered stream) or are the slots themselves.  Library against library: the one frame is the
    chain of five blend load frames of 1 000 triangles (bins of one run, which the model covers), and the same under every order."""
    row = next(r for r in K.BLEND_ROWS if r.name == "k_blend_order")
    w, h = 130, 70
    v, i = TB.soup(5000, 0xCC, cx=0.3, cy=0.3, spread=0.05, r=0.12)
    c0, d0 = K.special_start(w, h, 0xCD)
    images = []
    for order in (1, 0, -1):
        with swr.Context(0) as ctx:
            ctx.debug_set(K.DEBUG_STREAM_ORDER, order)
            ctx.target_set(w, h)
            ctx.scene_upload(v, i)
            ctx.blend_set(row.mode, row.opacity)
            ctx.target_write(c0, d0)
            ctx.draw(K.IDENT, flags | K.BLEND | K.LOAD)
            ctx.sync()
            whole = ctx.read_color(), ctx.read_depth()
            ctx.target_write(c0, d0)
            for k in range(5):
                ctx.draw_list([(3000 * k, 3000, K.IDENT)], flags | K.BLEND | K.LOAD)
            ctx.sync()
            assert np.array_equal(ctx.read_color(), whole[0]) and ctx.read_depth().tobytes() == whole[1].tobytes(), f"order {order}"
            assert whole[1].tobytes() == d0.tobytes() and not np.array_equal(whole[0], c0)
            images.append(whole[0])
    assert np.array_equal(images[0], images[1]) and np.array_equal(images[0], images[2])


# ---- the resolve kernels (K.RESOLVE_ROWS) --------------------------------------------------------------------------------------------
CARRY_SUMS = {2: (1, 2, 3, 1019, 1020), 4: (7, 8, 4079, 4080)}       # the block sums of tests/test_resolve.py::test_rounding_and_carries


def resolve_source(W, H, S, seed):
    """(colour, depth) to inject: colour with every byte value and, where they fit, blocks whose sums sit at the rounding and carry
    edges in each channel; depth from K.special_start (NaN with a payload, +-0, +-inf, denormals)."""
    rng = np.random.default_rng(seed)
    c, d = K.special_start(max(W, 8), max(H, 8), seed)
    c, d = np.ascontiguousarray(c[:H, :W]), np.ascontiguousarray(d[:H, :W])
    blocks = []
    for t in CARRY_SUMS[S]:
        for ch in range(4):
            b = rng.integers(0, 256, (S, S, 4), dtype=np.uint8)
            b[..., ch] = TR.block_with_sum(S, t, rng)
            blocks.append(b)
        blocks.append(np.stack([TR.block_with_sum(S, t, rng) for _ in range(4)], axis=-1))
    blocks.append(np.full((S, S, 4), 255, dtype=np.uint8))
    per_row = max(1, min(8, W // S))
    for k, b in enumerate(blocks):
        y, x = (k // per_row) * S, (k % per_row) * S
        if y + S <= H:
            c[y:y + S, x:x + S] = b
    if W * H >= 4096:
        assert np.unique(c).size == 256
    return c, d


def resolve_sizes(S):
    w, h = K.TARGETS["small"]
    return [(w // 4 * 4, h // 4 * 4), (4, 8), (520 * S, 130 * S)]       # ragged in tiles; 4 wide; more than 2^16 output pixels


@pytest.mark.parametrize("row", K.RESOLVE_ROWS, ids=[r.name for r in K.RESOLVE_ROWS])
def test_resolve_kernel(swr, oracle, row):
    S = row.S
    assert 520 * 130 > 1 << 16
    for k, (W, H) in enumerate(resolve_sizes(S)):
        what = f"{row.name}, {W}x{H}"
        if row.color and row.depth:
            # colour and depth through one launch: only swr_render_resolved's gather reaches these instances, and it refuses
            # SWR_FLAG_LOAD, so the source is a drawn frame (a z-tested soup), not an injected image.  Not covered by these four
            # rows: NaN, +-0, -inf and denormals in the MIN filter of the combined instance (its depth holds +inf and ordinary
            # values), the carry-edge blocks and all 256 byte values in its colour.  The one-image rows below inject them.
            s = swr.scenes.random_soup(300, W, H, 0x2E50 + k, r_ndc=0.2, margin=1.1)
            c, d, _ = FM.expect(oracle, FM.FrameSpec(s.vertices, s.indices, W, H, K.DT, transform=s.transform))
            with swr.Context(0) as ctx:
                gc, gd = ctx.render_resolved(s.vertices, s.indices, s.transform, W // S, H // S, K.DT, factor=S, depth_filter=row.depth_filter)
            FM.same((gc, gd, None), (RM.color(c, S), RM.depth(d, S, row.depth_filter), None), what)
            assert c.any()
            continue
        c, d = resolve_source(W, H, S, 0x2E60 + k)
        with swr.Context(0) as ctx:
            ctx.target_set(W, H)
            ctx.target_write(c, d)
            if row.color:
                FM.same((ctx.read_color_resolved(S), None, None), (RM.color(c, S), None, None), what)
            else:
                got = ctx.read_depth_resolved(S, row.depth_filter)
                FM.same((None, got, None), (None, RM.depth(d, S, row.depth_filter), None), what)
                if row.depth_filter == K.RESOLVE_MIN:
                    assert got.tobytes() != RM.depth(d, S, K.RESOLVE_SAMPLE0).tobytes()
            # the full-size images are not modified
            FM.same((ctx.read_color(), ctx.read_depth(), None), (c, d, None), what + ": the source afterwards")
