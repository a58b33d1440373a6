"""Draw lists (swr_draw_list, include/swr.h): several draws, each an index range with its own transform, in one frame.

Expected images come from the unchanged oracle through the composition identity: a draw-list frame is bit for bit the clear frame
of the concatenation of its items, every item's triangles pre-transformed by the item's matrix (Vertex.apply order, float32, no
FMA) and drawn with the identity.  The same frame is also compared with the chain of one-item frames (the first clear, the others
SWR_FLAG_LOAD) and with swr_draw, both on the GPU.
"""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, NC, METAL, LOAD = 1, 2, 4, 16
W, H = 640, 360
IDENT = np.eye(4, dtype=np.float32).T.reshape(16)


def same(c, d, rc, rd, what=""):
    if rc is not None:
        bad = np.nonzero((c != rc).any(axis=-1))
        assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"
    bad = np.nonzero(d.view(np.uint32) != rd.view(np.uint32))
    assert bad[0].size == 0, f"{what}: {bad[0].size} depth values differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"


def pretransform(vertices, m):
    """Vertex.apply in float32 without FMA: r = c0 x; r += c1 y; r += c2 z; r += c3; ndc = r.xyz / r.w."""
    v = np.array(vertices, dtype=np.float32, copy=True).reshape(-1, 8)
    c = np.asarray(m, dtype=np.float32).reshape(4, 4)          # column-major: c[k] = column k
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    r = c[0][None, :] * x
    r = r + c[1][None, :] * y
    r = r + c[2][None, :] * z
    r = r + c[3][None, :]
    v[:, 0:3] = r[:, 0:3] / r[:, 3:4]
    return v


def concat(vertices, indices, items, attrs=None):
    """The pre-transformed concatenation of the items (each item: its triangles, its own copy of the vertices) and its indices
    (and the matching per-vertex attributes)."""
    vs, ix, ats, base = [], [], [], 0
    for first, count, m in items:
        vs.append(pretransform(vertices, m))
        ix.append(np.asarray(indices[first:first + count], dtype=np.int64) + base)
        if attrs is not None:
            ats.append(attrs)
        base += vertices.shape[0]
    if not vs:
        return np.zeros((0, 8), np.float32), np.zeros(0, np.int64), None
    return np.concatenate(vs), np.concatenate(ix), (np.concatenate(ats) if attrs is not None else None)


def expected(oracle, vertices, indices, items, flags, w=W, h=H, shading=None):
    v, i, at = concat(vertices, indices, items, None if shading is None else shading.attrs)
    sh = None if shading is None else dataclasses.replace(shading, attrs=at)
    if flags & METAL:
        c, d, _, code = oracle.render_metal(v, i, IDENT, w, h, flags & NC, shading=sh)
    else:
        c, d, _, code = oracle.render(v, i, IDENT, w, h, flags | oracle.TINV_PER_TRIANGLE, shading=sh)
    assert code == 0
    return c, d


def read(ctx, flags):
    ctx.sync()
    return (None if flags & NC else ctx.read_color().copy()), ctx.read_depth().copy()


def affine(sx, sy, tx, ty, z=1.0):
    return np.array([sx, 0, 0, 0, 0, sy, 0, 0, 0, 0, z, 0, tx, ty, 0, 1], dtype=np.float32)


def soup(swr, ntri=3000, seed=0xD1, w=W, h=H, r_ndc=0.12):
    return swr.scenes.random_soup(ntri, w, h, seed, r_ndc=r_ndc, margin=1.1)


def mixed_items(swr, ntri, k, seed):
    """k disjoint ranges over [0, ntri): boundaries not aligned to 64, a 1-triangle item, an empty item, out of index order;
    perspective and affine matrices mixed."""
    S = swr.scenes
    rng = np.random.default_rng(seed)
    cuts = sorted(rng.choice(np.arange(1, ntri - 1), size=k - 1, replace=False).tolist())
    bounds = [0] + cuts + [ntri]
    ranges = [(bounds[j], bounds[j + 1] - bounds[j]) for j in range(k)]
    if k >= 3:
        ranges[1] = (ranges[1][0], 1)                         # a one-triangle item
    if k >= 8:
        ranges[4] = (ranges[4][0], 0)                         # an empty item
    order = list(range(k))[::-1] if k >= 3 else list(range(k))
    items = []
    for n, j in enumerate(order):
        first, count = ranges[j]
        m = S.app_transform(0.3 + 0.41 * n, scale=1.0 + 0.15 * (n % 3)) if n % 2 == 0 else \
            affine(0.9 + 0.05 * n, -0.8 - 0.03 * n, 0.02 * n - 0.05, 0.03 - 0.01 * n)
        items.append((3 * first, 3 * count, m))
    return items


MODES = {
    "painter": (0, None), "ztest": (DT, None), "depth_only": (DT | NC, None), "depth_only_64": (DT | NC, None),
    "metal": (METAL, None), "metal_depth": (METAL | NC, None), "phong": (DT, 1), "textured": (DT, 2),
}


def setup(swr, ctx, s, mode, shader, w=W, h=H):
    if mode == "depth_only_64":
        ctx.debug_set(swr.binding.DEBUG_DEPTH_KEYS32, 0)
    ctx.scene_upload(s.vertices, s.indices)
    sh = None
    if shader is not None:
        sh = swr.scenes.random_shading(s.vertices.shape[0], 0x5A, shader)
        ctx.shading_set(sh)
    ctx.target_set(w, h)
    return sh


# ---- 1: one item over the whole index array is swr_draw ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_one_item_equals_draw(swr, oracle, mode):
    flags, shader = MODES[mode]
    s = soup(swr)
    m = swr.scenes.app_transform(0.7, scale=1.3)
    with swr.Context(0) as ctx:
        sh = setup(swr, ctx, s, mode, shader)
        ctx.draw(m, flags)
        c0, d0 = read(ctx, flags)
        ctx.draw_list([(0, s.indices.size, m)], flags)
        c1, d1 = read(ctx, flags)
    same(c1, d1, c0, d0, f"{mode}: list of one vs swr_draw")
    rc, rd = expected(oracle, s.vertices, s.indices, [(0, s.indices.size, m)], flags, shading=sh)
    same(c1, d1, None if flags & NC else rc, rd, f"{mode}: list of one vs oracle")


# ---- 2: disjoint ranges, several matrices -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("mode", ["painter", "ztest", "depth_only", "metal", "phong"])
def test_disjoint_items_equal_the_concatenation(swr, oracle, k, mode):
    flags, shader = MODES[mode]
    s = soup(swr, 2500, seed=0xD2 + k)
    items = mixed_items(swr, 2500, k, seed=k)
    with swr.Context(0) as ctx:
        sh = setup(swr, ctx, s, mode, shader)
        ctx.draw_list(items, flags)
        c, d = read(ctx, flags)
    rc, rd = expected(oracle, s.vertices, s.indices, items, flags, shading=sh)
    same(c, d, None if flags & NC else rc, rd, f"{mode}, {k} items")


@pytest.mark.parametrize("flags", [DT, 0, DT | NC])
def test_empty_list_clears_or_keeps(swr, oracle, flags):
    s = soup(swr, 800)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        ctx.draw(s.transform, flags)
        c0, d0 = read(ctx, flags)
        ctx.draw_list([], flags | LOAD)                      # keeps the image
        c1, d1 = read(ctx, flags)
        same(c1, d1, c0, d0, "empty list under SWR_FLAG_LOAD")
        ctx.draw_list([], flags)                             # clears it
        c2, d2 = read(ctx, flags)
    assert np.all(np.isinf(d2)) and np.all(d2 > 0)
    if c2 is not None:
        assert not c2.any()


# ---- 3: instancing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ztest", "painter", "depth_only", "metal"])
def test_instancing(swr, oracle, mode):
    flags, _ = MODES[mode]
    S = swr.scenes
    s = soup(swr, 1200, seed=0x1A, r_ndc=0.08)
    n = s.indices.size
    four = [(0, n, S.app_transform(0.25 * j, scale=0.8 + 0.2 * j)) for j in range(4)]
    sub = (300, 1200)                                        # one range twice with the SAME matrix, plus a neighbour range
    m = S.app_transform(0.5, scale=1.4)
    twice = [(sub[0], sub[1], m), (0, 600, affine(0.7, 0.7, 0.1, 0.0)), (sub[0], sub[1], m)]
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        for items in (four, twice):
            ctx.draw_list(items, flags)
            c, d = read(ctx, flags)
            rc, rd = expected(oracle, s.vertices, s.indices, items, flags)
            same(c, d, None if flags & NC else rc, rd, f"{mode}: {len(items)} instances")


@pytest.mark.parametrize("flags", [DT, 0])
def test_ties_between_items(swr, oracle, flags):
    """Two ranges with the same geometry and other colours, drawn with one matrix: exact depth ties everywhere.  The z-test keeps
    the first item, painter's order the last one."""
    s = soup(swr, 900, seed=0x71E, r_ndc=0.1)
    v = np.concatenate([s.vertices, s.vertices])
    v[s.vertices.shape[0]:, 4:7] = v[s.vertices.shape[0]:, 4:7][::-1]
    i = np.arange(v.shape[0], dtype=np.int64)
    m = swr.scenes.app_transform(0.9, scale=1.2)
    n = s.indices.size
    items = [(0, n, m), (n, n, m)]
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw_list(items, flags)
        c, d = read(ctx, flags)
    rc, rd = expected(oracle, v, i, items, flags)
    same(c, d, rc, rd, "ties")
    first, _ = expected(oracle, v, i, items[:1], flags)
    last, _ = expected(oracle, v, i, items[1:], flags)
    cov = first[..., 3] == 255
    assert cov.sum() > 1000
    assert np.array_equal(c[cov], (first if flags & DT else last)[cov])


# ---- 4: the chain of one-item frames; a list over a written image -----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ztest", "painter", "depth_only", "phong"])
def test_list_equals_the_chain_of_load_frames(swr, oracle, mode):
    flags, shader = MODES[mode]
    s = soup(swr, 2000, seed=0xC4A1)
    items = mixed_items(swr, 2000, 5, seed=11)
    with swr.Context(0) as ctx:
        setup(swr, ctx, s, mode, shader)
        for k, it in enumerate(items):
            ctx.draw_list([it], flags | (LOAD if k else 0))
        c0, d0 = read(ctx, flags)
        ctx.draw_list(items, flags)
        c1, d1 = read(ctx, flags)
    same(c1, d1, c0, d0, f"{mode}: list vs chain")


@pytest.mark.parametrize("flags", [DT, 0, DT | NC])
def test_load_list_over_a_written_image(swr, oracle, flags):
    s = soup(swr, 1500, seed=0x3E7)
    items = mixed_items(swr, 1500, 3, seed=5)
    rng = np.random.default_rng(3)
    d0 = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    d0[::7, ::5] = np.inf
    c0 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        ctx.target_write(None if flags & NC else c0, d0)
        ctx.draw_list(items, flags | LOAD)
        c1, d1 = read(ctx, flags)
        ctx.target_write(None if flags & NC else c0, d0)
        for it in items:
            ctx.draw_list([it], flags | LOAD)
        c2, d2 = read(ctx, flags)
    same(c1, d1, c2, d2, "load list vs chain over a written image")
    cb, db = expected(oracle, s.vertices, s.indices, items, flags)
    if flags & DT:
        win = db < d0
        rd, rc = np.where(win, db, d0), np.where(win[..., None], cb, c0)
    else:
        rd, rc = d0, np.where((cb[..., 3] == 255)[..., None], cb, c0)
    same(c1, d1, None if flags & NC else rc, rd, "load list vs the per-pixel rule")


# ---- 5: every binning path --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bin_mode", [1, 3])
@pytest.mark.parametrize("flags", [DT, DT | NC])
def test_exact_bin_paths(swr, oracle, bin_mode, flags):
    s = soup(swr, 2500, seed=0xB1)
    items = mixed_items(swr, 2500, 8, seed=8) + [(0, 900, affine(0.5, 0.5, -0.3, 0.2))]
    with swr.Context(0) as ctx:
        ctx.debug_set(swr.binding.DEBUG_BIN_MODE, bin_mode)
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        ctx.draw_list(items, flags)
        c, d = read(ctx, flags)
    rc, rd = expected(oracle, s.vertices, s.indices, items, flags)
    same(c, d, None if flags & NC else rc, rd, f"bin mode {bin_mode}")


@pytest.mark.parametrize("bins", ["fixed", "exact"])
def test_bin_overflow_and_regrow(swr, oracle, bins):
    """A small dense patch instanced many times into a few tiles: far more entries than the first guess of the bins (sized by the
    scene, not by the list) holds.  The frame is redrawn with grown bins, silently right."""
    w, h = 1280, 720
    s = swr.scenes.random_soup(3000, w, h, 555, r_ndc=0.01, margin=1.0)
    v = s.vertices.copy()
    v[:, 0] = 0.30 + (v[:, 0] * 0.5 + 0.5) * 0.07
    v[:, 1] = 0.10 + (v[:, 1] * 0.5 + 0.5) * 0.06
    items = [(0, s.indices.size, affine(1.0, 1.0, 0.004 * j, -0.003 * j)) for j in range(12)]
    with swr.Context(0) as ctx:
        if bins == "exact":
            ctx.debug_set(swr.binding.DEBUG_BIN_MODE, swr.binding.BIN_MODE_EXACT)
        ctx.scene_upload(v, s.indices)
        ctx.target_set(w, h)
        ctx.draw_list(items, DT)
        hc, hd = swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)
        ctx.present(hc, hd)
        ctx.present_wait()
        c, d = hc.array.copy(), hd.array.copy()
        hc.free(); hd.free()
    rc, rd = expected(oracle, v, s.indices, items, DT, w, h)
    same(c, d, rc, rd, f"{bins}: overflow redrawn")


def test_deferred_big_triangles(swr, oracle):
    """Screen-filling triangles in one item among small ones: the second frame defers them (k_bin's big-triangle list)."""
    w, h = 1280, 720
    small = swr.scenes.random_soup(1500, w, h, 0xB16, r_ndc=0.05, margin=1.0)
    big = swr.scenes.random_soup(150, w, h, 77, r_ndc=1.4, margin=0.3)
    v = np.concatenate([small.vertices, big.vertices])
    i = np.concatenate([small.indices, big.indices + small.vertices.shape[0]])
    items = [(0, small.indices.size, affine(0.9, 0.9, 0.05, 0.0)), (small.indices.size, big.indices.size, IDENT),
             (0, 900, swr.scenes.app_transform(0.4, scale=1.1))]
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(w, h)
        for frame in range(3):
            for flags in (DT, DT | NC):
                ctx.draw_list(items, flags)
                c, d = read(ctx, flags)
                rc, rd = expected(oracle, v, i, items, flags, w, h)
                same(c, d, None if flags & NC else rc, rd, f"frame {frame}, flags {flags}")


@pytest.mark.parametrize("flags", [DT, DT | NC, 0])
def test_more_than_2_20_primitives(swr, oracle, flags):
    """A 300 000-triangle mesh drawn four times: 1.2 M primitives in the frame, past 2^20 (the PLAIN colour kernels)."""
    s = swr.scenes.random_soup(300_000, W, H, 0x2020, r_ndc=0.01, margin=1.0)
    S = swr.scenes
    n = s.indices.size
    items = [(0, n, S.app_transform(0.2 * j, scale=1.0 + 0.1 * j)) for j in range(4)]
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        ctx.draw_list(items, flags)
        c, d = read(ctx, flags)
    rc, rd = expected(oracle, s.vertices, s.indices, items, flags)
    same(c, d, None if flags & NC else rc, rd, "1.2 M primitives")


# ---- 6: stream segmentation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 0, -1])
def test_stream_segmentation(swr, oracle, order):
    """A list that cuts the stream, a plain swr_draw after it, another list with other boundaries, a re-upload, the first list
    again: every frame right."""
    flags = DT
    s = soup(swr, 3000, seed=0x5E6)
    a = mixed_items(swr, 3000, 8, seed=21)
    b = mixed_items(swr, 3000, 3, seed=22)
    m = swr.scenes.app_transform(1.3, scale=1.2)
    with swr.Context(0) as ctx:
        ctx.debug_set(swr.binding.DEBUG_STREAM_ORDER, order)
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        steps = [("list a", a), ("draw", None), ("list b", b), ("list a again", a), ("upload", None), ("list b after upload", b),
                 ("draw after upload", None)]
        for what, items in steps:
            if what == "upload":
                ctx.scene_upload(s.vertices, s.indices)
                continue
            if items is None:
                ctx.draw(m, flags)
                items = [(0, s.indices.size, m)]
            else:
                ctx.draw_list(items, flags)
            c, d = read(ctx, flags)
            rc, rd = expected(oracle, s.vertices, s.indices, items, flags)
            same(c, d, rc, rd, f"order {order}: {what}")


# ---- 7: multi-device; an un-waited burst -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bands", [2, 3])
@pytest.mark.parametrize("flags", [DT, DT | NC])
def test_multi_device(swr, oracle, bands, flags):
    s = soup(swr, 2500, seed=0xBA4D)
    items = mixed_items(swr, 2500, 8, seed=30)
    with swr.Context(0, device_count=bands) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        ctx.draw_list(items, flags)
        c, d = read(ctx, flags)
    rc, rd = expected(oracle, s.vertices, s.indices, items, flags)
    same(c, d, None if flags & NC else rc, rd, f"{bands} bands")


@pytest.mark.parametrize("bands", [1, 2])
def test_unwaited_burst_of_lists_and_draws(swr, oracle, bands):
    """Lists with different items alternating with plain draws, none waited for, every frame presented into its own image; the
    caller's item array is overwritten right after every call."""
    S = swr.scenes
    s = soup(swr, 2000, seed=0xB0B)
    n = s.indices.size
    lists = [mixed_items(swr, 2000, 3 + (k % 4), seed=40 + k) for k in range(6)]
    frames = []
    for k in range(12):
        if k % 3 == 2:
            frames.append(("draw", S.app_transform(0.31 * k, scale=1.1)))
        else:
            frames.append(("list", lists[k % len(lists)]))
    imgs = [(swr.HostImage((H, W, 4), np.uint8), swr.HostImage((H, W), np.float32)) for _ in frames]
    try:
        with swr.Context(0, device_count=bands if bands > 1 else 0) as ctx:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(W, H)
            for (kind, what), img in zip(frames, imgs):
                if kind == "draw":
                    ctx.draw(what, DT)
                else:
                    arr = swr.Context.draw_items(what)
                    ctx.draw_list(arr, DT)
                    arr["transform"] = np.float32(np.nan)        # the call copied the list
                    arr["first_index"] = 0
                    arr["index_count"] = n
                ctx.present(*img)
            ctx.present_wait()
        for k, ((kind, what), img) in enumerate(zip(frames, imgs)):
            items = [(0, n, what)] if kind == "draw" else what
            rc, rd = expected(oracle, s.vertices, s.indices, items, DT)
            same(img[0].array, img[1].array, rc, rd, f"burst frame {k} ({kind})")
    finally:
        for a, b in imgs:
            a.free(); b.free()


# ---- 8: errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(swr, oracle):
    s = soup(swr, 600, seed=0xE44)
    n = s.indices.size
    m = s.transform
    with swr.Context(0) as ctx:
        with pytest.raises(swr.SwrError) as e:
            ctx.draw_list([(0, n, m)], DT)
        assert e.value.code == -6                                  # no scene, no target
        ctx.scene_upload(s.vertices, s.indices)
        with pytest.raises(swr.SwrError) as e:
            ctx.draw_list([(0, n, m)], DT)
        assert e.value.code == -6                                  # no target
        ctx.target_set(W, H)
        bad = [([(1, 3, m)], -2), ([(0, 4, m)], -2), ([(0, n + 3, m)], -1), ([(-3, 3, m)], -1), ([(n, 3, m)], -1),
               ([(0, n, m)] * 4097, -5)]
        for items, code in bad:
            with pytest.raises(swr.SwrError) as e:
                ctx.draw_list(items, DT)
            assert e.value.code == code, items[:1]
        L = ctx._L
        assert L.swr_draw_list(ctx._h, None, 2, DT) == -1          # NULL items with item_count > 0
        assert L.swr_draw_list(ctx._h, None, -1, DT) == -1         # item_count < 0
        # 2^24 triangles or more in one list: refused before anything is drawn
        s2 = soup(swr, 5000, seed=0xE45)
        ctx.scene_upload(s2.vertices, s2.indices)
        big = swr.Context.draw_items([(0, s2.indices.size, m)] * ((1 << 24) // 5000 + 1))
        assert big.size <= 4096
        assert L.swr_draw_list(ctx._h, big.ctypes.data, big.size, DT) == -5
        assert L.swr_draw_list(ctx._h, big.ctypes.data, big.size - 1, DT | NC) == 0     # just below: drawn
        ctx.sync()
        ctx.scene_upload(s.vertices, s.indices)
        with pytest.raises(swr.SwrError) as e:
            ctx.draw_list([(0, n, m)], 1 << 9)                     # an unknown flag
        assert e.value.code == -1
        # still usable
        ctx.draw_list([(0, n, m), (0, 30, IDENT)], DT)
        c, d = read(ctx, DT)
    rc, rd = expected(oracle, s.vertices, s.indices, [(0, n, m), (0, 30, IDENT)], DT)
    same(c, d, rc, rd, "after the errors")


def test_frame_loop_example_objects(swr, oracle):
    """examples/frame_loop.py --objects: N copies of the mesh, each with its own matrix, one draw list per frame."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(root, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    v, i, res = fl.run(2, 256, None, depth_test=True, objects=5)
    for c, d, ms in res:
        assert len(ms) == 5
        rc, rd = expected(oracle, v, i, [(0, i.size, m) for m in ms], DT, 256, 256)
        same(c, d, rc, rd, "frame loop with 5 objects")
        assert (c[..., 3] == 255).mean() > 0.005
