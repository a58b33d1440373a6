"""Every raster and binning kernel instantiation once, bit for bit against the oracle (tests/kernel_matrix.py: the rows, the scenes,
the expectations).

Raster rows draw the visible set (below 2^20 primitives: the winner-table kernels) or the same set padded with off-screen filler
to 2^20 + 1 primitives (the PLAIN kernels; the filler sits in the middle, so the last visible triangle is number 2^20), on a small
ragged target and on one of 460 tiles.  LOAD rows start from a swr_target_write image with NaN (one with a payload), +-0, +-inf,
+-denormals and ordinary depths.  IDS rows also draw the frame without the flag and compare: colour and depth are the same.
Binning rows (k_bin) draw with affine and perspective transforms, as draws and as 3-item draw lists (one item mirrored), with face
culling on some; DEFER rows are drawn twice on the large target, and both frames are checked.
"""
import numpy as np
import pytest

import kernel_matrix as K

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
