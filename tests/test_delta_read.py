"""Delta reads on the GPU (include/swr.h "Delta reads"): swr_read_color_delta, swr_read_depth_delta,
swr_delta_reset and swr_render_delta.  Equality is exact everywhere.  The expectation is never the code under test: what the caller's
image must hold comes from the numpy model tests/delta_model.py, fed with the image the test itself wrote (swr_target_write) or the
library's plain swr_read_color / swr_read_depth delivered, and on one drawn frame from frame_model.expect (the oracle).  Before most
reads the test plants wrong words outside the rectangle the model allows to be written, and finds them again.
The shapes are the smallest at which it can go wrong (delta_model.SHAPES): one tile, one pixel, 3 x 3 whole tiles, a ragged target
whose width is no multiple of four (the dword path of the kernels), three bands, and a context that owns one band of a larger target."""
import ctypes
import os
import re

import numpy as np
import pytest

import delta_model as M
import frame_model as FM
import kernel_matrix as K

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, NC, METAL, LOAD, IDS, BLEND = FM.DT, FM.NC, FM.METAL, FM.LOAD, FM.IDS, FM.BLEND
IDENT = K.IDENT
BAD_ARG, HIP, UNSUPPORTED, NO_SCENE = -1, -4, -5, -6
SENTINEL = 0xA5A5A5A5
COLOR, DEPTH = 0, 1


def context_of(swr, shape):
    w, h, n, rows = M.SHAPES[shape]
    ctx = swr.Context(0, device_count=n if n > 1 else 0)
    if rows:
        ctx.target_set(w, h, rows[0], rows[1])
    else:
        ctx.target_set(w, h)
    return ctx


def words(x):
    return M.as_words(x.array if hasattr(x, "array") else x)


class Side:
    """One image kind of one context: the caller's image, and what the device's baseline must be (what was last delivered)."""

    def __init__(self, swr, ctx, kind, pinned=False):
        self.swr, self.ctx, self.kind = swr, ctx, kind
        shape, dtype = ((ctx.height, ctx.width, 4), np.uint8) if kind == COLOR else ((ctx.height, ctx.width), np.float32)
        self.image = swr.HostImage(shape, dtype) if pinned else np.zeros(shape, dtype=dtype)
        words(self.image)[...] = SENTINEL
        self.base = None

    def free(self):
        if hasattr(self.image, "free"):
            self.image.free()

    def bands(self):
        return [(a, b) for _, a, b in self.ctx.bands()]

    def plain(self):
        """What swr_read_color / swr_read_depth deliver now, as words (the library's own read: not the code under test)."""
        return words(self.ctx.read_color() if self.kind == COLOR else self.ctx.read_depth()).copy()

    def read(self, what="", cur=None, plant=True):
        """One delta read, checked against the model; returns (stats, the model's Delta)."""
        ctx = self.ctx
        cur = self.plain() if cur is None else words(cur)
        dst = words(self.image)
        d, want = M.delta(self.base, cur, self.bands(), dst)
        planted = []
        if plant:
            free = M.outside(d, dst.shape)
            ys, xs = np.nonzero(free)
            if ys.size:
                planted = {(int(ys[0]), int(xs[0])), (int(ys[-1]), int(xs[-1])), (int(ys[ys.size // 2]), int(xs[ys.size // 2]))}
                for (a, b), r in zip(self.bands(), d.band_rects):       # and in every band of the context that has nothing to deliver
                    if r is None and b > a:
                        planted |= {(a, 0), (b - 1, dst.shape[1] - 1)}
            for y, x in planted:
                dst[y, x] ^= 0x00FF00FF
                want[y, x] ^= 0x00FF00FF
        st = ctx.read_color_delta(self.image) if self.kind == COLOR else ctx.read_depth_delta(self.image)
        got = (st.tiles, st.tiles_changed, st.full, st.reserved, st.rect)
        print(f"{what}: tiles {st.tiles} changed {st.tiles_changed} full {st.full} rect {st.rect} bytes {st.bytes_copied} "
              f"(model: changed {d.tiles_changed}, rect {d.rect}, bytes {d.changed_pixels * 4} .. {d.rect_bytes})")
        assert got == (d.tiles, d.tiles_changed, d.full, 0, d.rect), (what, got, d)
        assert d.changed_pixels * 4 <= st.bytes_copied <= d.rect_bytes, (what, st.bytes_copied, d)
        if d.full:
            assert st.bytes_copied == d.rect_bytes, what
        bad = np.nonzero(dst != want)
        assert bad[0].size == 0, f"{what}: {bad[0].size} words differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"
        for y, x in planted:                # (the planted words broke the promise: mended before the next read)
            dst[y, x] ^= 0x00FF00FF
        self.base = cur.copy()
        return st, d


def write(ctx, kind, w32):
    if kind == COLOR:
        ctx.target_write(np.ascontiguousarray(w32).view(np.uint8).reshape(w32.shape[0], w32.shape[1], 4), None)
    else:
        ctx.target_write(None, np.ascontiguousarray(w32).view(np.float32))


def random_words(w, h, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, (h, w), dtype=np.uint32)


# ---- images the test writes itself: every bit is the test's --------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page_locked"])
@pytest.mark.parametrize("shape", sorted(M.SHAPES))
def test_change_sets(swr, shape, pinned):
    """The first read is full; an identical image copies nothing and leaves the destination alone; then every change set of the shape,
    one after the other, for both image kinds: single words at tile corners and in the ragged edge tiles, a column and a row of tiles,
    every tile.  Wrong words planted outside the rectangle — on three bands also in the bands that have nothing to deliver — are
    found again."""
    w, h, n, rows = M.SHAPES[shape]
    with context_of(swr, shape) as ctx:
        assert len(ctx.bands()) == n
        for kind in (COLOR, DEPTH):
            side = Side(swr, ctx, kind, pinned)
            img = random_words(w, h, 11 + kind)
            write(ctx, kind, img)
            st, d = side.read(f"{shape} first", cur=None)
            assert st.full == 1 and st.tiles_changed == st.tiles > 0
            ya, yb = side.bands()[0][0], side.bands()[-1][1]
            assert (words(side.image)[:ya] == SENTINEL).all() and (words(side.image)[yb:] == SENTINEL).all()
            assert np.array_equal(words(side.image)[ya:yb], img[ya:yb])
            st, d = side.read(f"{shape} identical")
            assert (st.tiles_changed, st.bytes_copied, st.rect, st.full) == (0, 0, (0, 0, 0, 0), 0)
            for name, pts in M.change_sets(shape).items():
                for x, y in pts:
                    img[y, x] ^= 0x80000001
                write(ctx, kind, img)
                st, d = side.read(f"{shape} {name}", cur=img)
                assert np.array_equal(words(side.image)[ya:yb], img[ya:yb]), name
                if name == "none":
                    assert st.tiles_changed == 0 and st.bytes_copied == 0
                elif len(pts) == 1:
                    assert st.tiles_changed == 1 and st.rect[2] - st.rect[0] <= 64 and st.rect[3] - st.rect[1] <= 32
                elif name == "all":
                    assert st.tiles_changed == st.tiles and st.bytes_copied == w * (yb - ya) * 4
            side.free()


@gpu
def test_depth_is_compared_as_bits(swr):
    """A depth image whose only change is a NaN payload is a change; -0 against +0 is one; identical NaNs are none."""
    with context_of(swr, "ragged") as ctx:
        w, h = ctx.width, ctx.height
        side = Side(swr, ctx, DEPTH)
        d0 = np.random.default_rng(3).uniform(0, 1, (h, w)).astype(np.float32)
        d0[5, 70] = np.nan
        d0[40, 129] = np.nan
        d0[69, 0] = 0.0
        ctx.target_write(None, d0)
        side.read("nan first", cur=d0)
        ctx.target_write(None, d0.copy())                        # the same NaNs again
        st, _ = side.read("identical nans", cur=d0)
        assert st.tiles_changed == 0 and st.bytes_copied == 0
        d1 = d0.copy()
        d1.view(np.uint32)[5, 70] ^= 0x1                          # another payload, still a NaN
        assert np.isnan(d1[5, 70]) and np.array_equal(np.isnan(d0), np.isnan(d1))
        ctx.target_write(None, d1)
        st, _ = side.read("nan payload", cur=d1)
        assert st.tiles_changed == 1 and st.rect == (64, 0, 128, 32)
        assert words(side.image)[5, 70] == d1.view(np.uint32)[5, 70]
        d2 = d1.copy()
        d2[69, 0] = -0.0
        assert d2[69, 0] == d1[69, 0]
        ctx.target_write(None, d2)
        st, _ = side.read("minus zero", cur=d2)
        assert st.tiles_changed == 1 and st.rect == (0, 64, 64, 70) and words(side.image)[69, 0] == 0x80000000


@gpu
def test_baselines_are_independent_and_reset_per_bit(swr):
    B = swr.binding
    with context_of(swr, "3x3_tiles") as ctx:
        w, h = ctx.width, ctx.height
        c, d = Side(swr, ctx, COLOR), Side(swr, ctx, DEPTH)
        ci, di = random_words(w, h, 1), random_words(w, h, 2)
        write(ctx, COLOR, ci); write(ctx, DEPTH, di)
        assert c.read("colour first")[0].full == 1
        assert d.read("depth first")[0].full == 1               # (the colour's baseline is not the depth's)
        ci[50, 100] ^= 1
        write(ctx, COLOR, ci)
        assert c.read("colour changed")[0].tiles_changed == 1
        assert d.read("depth unchanged")[0].tiles_changed == 0
        ctx.delta_reset(B.DELTA_DEPTH)
        d.base = None
        assert c.read("colour after the depth's reset")[0].full == 0
        assert d.read("depth after its reset")[0].full == 1
        ctx.delta_reset(B.DELTA_COLOR)
        c.base = None
        assert d.read("depth after the colour's reset")[0].full == 0
        assert c.read("colour after its reset")[0].full == 1
        ctx.delta_reset()
        c.base = d.base = None
        assert c.read("colour after both")[0].full == 1 and d.read("depth after both")[0].full == 1
        assert c.read("colour again")[0].tiles_changed == 0 and d.read("depth again")[0].tiles_changed == 0


@gpu
def test_the_same_target_keeps_the_baseline_another_drops_it(swr):
    with context_of(swr, "3x3_tiles") as ctx:
        w, h = ctx.width, ctx.height
        side = Side(swr, ctx, COLOR)
        img = random_words(w, h, 5)
        write(ctx, COLOR, img)
        side.read("first")
        ctx.target_set(w, h)                                    # the same target again (swr_render does this every frame)
        write(ctx, COLOR, img)
        st, _ = side.read("same target", cur=img)
        assert st.full == 0 and st.tiles_changed == 0
        ctx.target_set(w, h + 32)                               # other rows
        big = Side(swr, ctx, COLOR)
        write(ctx, COLOR, random_words(w, h + 32, 6))
        assert big.read("larger target")[0].full == 1
        ctx.target_set(w, h)                                    # and back: dropped again
        write(ctx, COLOR, img)
        side.base = None
        assert side.read("back", cur=img)[0].full == 1
        ctx.target_set(w, h, 32, 96)                            # the same size, other rows
        write(ctx, COLOR, img)
        side.base = None
        st, _ = side.read("a band of it", cur=img)
        assert st.full == 1 and st.rect == (0, 32, w, 96)


# ---- drawn frames ------------------------------------------------------------------------------------------------------------------
def small_mesh():
    """Two triangles of about 40 x 30 pixels of a 192 x 96 target, at different depths."""
    xyz = np.array([[-0.2, -0.3, 0.3], [0.2, -0.3, 0.3], [0.0, 0.3, 0.3], [-0.1, -0.2, 0.6], [0.25, 0.1, 0.6], [-0.15, 0.25, 0.6]])
    rgb = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]], dtype=np.float64)
    return K._pack(xyz, rgb), np.arange(6, dtype=np.int64)


def moved(dx, dy):
    m = np.array(IDENT, dtype=np.float32).reshape(16).copy()
    m[12], m[13] = dx, dy
    return m


SEQUENCE = [("ztest", DT, (-0.6, 0.0)), ("painter", 0, (-0.3, 0.2)), ("metal", METAL | DT, (0.0, -0.2)), ("load", DT | LOAD, (0.3, 0.1)),
            ("blend", DT | BLEND | LOAD, (0.35, 0.0)), ("depth_only", DT | NC, (0.6, -0.1))]


@gpu
@pytest.mark.parametrize("shape", ["3x3_tiles", "three_bands"])
def test_a_drawn_sequence(swr, oracle, shape):
    """A small mesh moved over six frames with mixed flags.  After every frame both images the delta reads keep up to date equal what
    the plain reads deliver; the first frame also equals the oracle's."""
    v, i = small_mesh()
    w, h, n, _ = M.SHAPES[shape]
    with context_of(swr, shape) as ctx:
        ctx.scene_upload(v, i)
        ctx.blend_set(swr.binding.BLEND_OVER, 128)
        c, d = Side(swr, ctx, COLOR, pinned=True), Side(swr, ctx, DEPTH)
        for k, (name, flags, (dx, dy)) in enumerate(SEQUENCE):
            ctx.draw(moved(dx, dy), flags)
            sd, md = d.read(f"{name} depth")
            sc, mc = c.read(f"{name} colour")                   # after the depth-only frame: whatever swr_read_color delivers
            assert np.array_equal(words(c.image), words(ctx.read_color())), name
            assert np.array_equal(words(d.image), words(ctx.read_depth())), name
            if k == 0:
                want = FM.expect(oracle, FM.FrameSpec(v, i, w, h, flags, transform=moved(dx, dy)))
                FM.same((np.asarray(c.image.array), d.image, None), want, "the first frame against the oracle")
                assert sc.full == 1 and sd.full == 1
            else:
                assert sc.full == 0 and sd.full == 0 and sd.tiles_changed < sd.tiles
            if name in ("ztest", "painter", "metal"):
                assert 0 < sc.tiles_changed
        c.free()


@gpu
def test_other_calls_in_between_change_nothing(swr):
    v, i = small_mesh()
    with context_of(swr, "3x3_tiles") as ctx:
        w, h = ctx.width, ctx.height
        ctx.scene_upload(v, i)
        ctx.draw(moved(0.1, 0.0), DT | IDS)
        c, d = Side(swr, ctx, COLOR), Side(swr, ctx, DEPTH)
        c.read("first colour"); d.read("first depth")
        color, depth = ctx.read_color(), ctx.read_depth()
        pc, pd = swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)

        def present():
            ctx.present(pc, pd)
            ctx.present_wait()

        for call in (ctx.read_color, ctx.read_depth, ctx.read_ids, ctx.count_ids, lambda: ctx.query_depth([(0, 0, w, h, 0.5)]), present,
                     ctx.sync):
            call()
            sc, _ = c.read("colour after another call")
            sd, _ = d.read("depth after another call")
            assert sc.tiles_changed == 0 and sd.tiles_changed == 0 and sc.bytes_copied == 0 and sd.bytes_copied == 0
        # and the delta reads modify no framebuffer image
        assert np.array_equal(ctx.read_color(), color) and np.array_equal(ctx.read_depth().view(np.uint32), depth.view(np.uint32))
        assert np.array_equal(pc.array, color)
        pc.free(); pd.free()


@gpu
def test_bin_overflow_of_the_last_frame(swr, oracle):
    """Forced as tests/test_depth_query.py forces it: a fresh context whose fixed-stride bins are too small for 20 000 triangles in a
    few tiles.  The delta read is the first call that waits: it repairs the frame and delivers the repaired image."""
    w, h = 1280, 720
    s = swr.scenes.random_soup(20000, w, h, 555, r_ndc=0.01, flags=DT, margin=1.0)
    v = s.vertices.copy()
    v[:, 0] = 0.30 + (v[:, 0] * 0.5 + 0.5) * 0.07
    v[:, 1] = 0.10 + (v[:, 1] * 0.5 + 0.5) * 0.06
    v = np.ascontiguousarray(v)
    want = FM.expect(oracle, FM.FrameSpec(v, s.indices, w, h, DT, transform=s.transform))
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, s.indices)
        empty = np.full((h, w), np.inf, dtype=np.float32)
        ctx.target_write(None, empty)
        depth = np.zeros((h, w), dtype=np.float32)
        assert ctx.read_depth_delta(depth).full == 1            # a baseline: the cleared depth
        ctx.draw(s.transform, DT)
        st = ctx.read_depth_delta(depth)                        # the first call that waits
        FM.same((None, depth, None), want, "overflowed last frame")
        ys, xs = np.nonzero(np.isfinite(want[1]))
        assert ys.size > 200 and 0 < st.tiles_changed <= 4 and st.full == 0
        assert st.rect[0] <= xs.min() and xs.max() < st.rect[2] and st.rect[1] <= ys.min() and ys.max() < st.rect[3]
        assert np.array_equal(depth.view(np.uint32), ctx.read_depth().view(np.uint32))


# ---- swr_render_delta ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("device_count", [0, 3])
def test_render_delta_over_six_cached_frames(swr, device_count):
    """swr_render_delta into the same two images equals swr_render on a second context, frame by frame; the stats are the model's."""
    v, i = small_mesh()
    w, h = 192, 128
    color, depth = np.full((h, w, 4), 0xA5, dtype=np.uint8), np.full((h, w), -7.0, dtype=np.float32)
    prev_c = prev_d = None
    with swr.Context(0, device_count=device_count) as a, swr.Context(0) as b:
        for k in range(6):
            flags = DT if k != 4 else DT | NC
            m = moved(-0.5 + 0.2 * k, 0.1 * (k % 2))
            before_c, before_d = color.copy(), depth.copy()
            sc, sd = a.render_delta(v, i, m, w, h, None if flags & NC else color, depth, flags, scene_id=7)
            wc, wd = b.render(v, i, m, w, h, flags, scene_id=7)
            bands = [(r0, r1) for _, r0, r1 in a.bands()]
            md, want_d = M.delta(prev_d, wd, bands, before_d)
            assert np.array_equal(depth.view(np.uint32), want_d) and np.array_equal(depth.view(np.uint32), wd.view(np.uint32)), k
            assert (sd.tiles, sd.tiles_changed, sd.full, sd.rect) == (md.tiles, md.tiles_changed, md.full, md.rect), (k, md)
            assert md.changed_pixels * 4 <= sd.bytes_copied <= md.rect_bytes
            prev_d = M.as_words(wd).copy()
            if flags & NC:
                assert (sc.tiles, sc.tiles_changed, sc.bytes_copied, sc.full, sc.rect) == (0, 0, 0, 0, (0, 0, 0, 0))
                assert np.array_equal(color, before_c)
            else:
                mc, want_c = M.delta(prev_c, wc, bands, before_c)
                assert np.array_equal(M.as_words(color), want_c) and np.array_equal(color, wc), k
                assert (sc.tiles, sc.tiles_changed, sc.full, sc.rect) == (mc.tiles, mc.tiles_changed, mc.full, mc.rect), (k, mc)
                prev_c = M.as_words(wc).copy()
            assert (sd.full == 1) == (k == 0)
            if k > 0:
                assert 0 < sd.tiles_changed < sd.tiles
            t = swr.binding.RenderTimes()
            assert a._L.swr_render_timings(a._h, ctypes.byref(t)) == 0
            assert t.scene_cached == (1 if k else 0) and t.gather_ms > 0


def code_of(swr, call):
    with pytest.raises(swr.SwrError) as e:
        call()
    return e.value.code, str(e.value)


@gpu
def test_render_delta_with_a_load_frame_is_refused(swr):
    v, i = small_mesh()
    color, depth = np.full((96, 192, 4), 0xA5, dtype=np.uint8), np.full((96, 192), -7.0, dtype=np.float32)
    with swr.Context(0) as ctx:
        code, text = code_of(swr, lambda: ctx.render_delta(v, i, IDENT, 192, 96, color, depth, DT | LOAD))
        assert code == UNSUPPORTED and "SWR_FLAG_LOAD" in text
        assert (color == 0xA5).all() and (depth == -7.0).all()
        sc, sd = ctx.render_delta(v, i, IDENT, 192, 96, color, depth, DT)       # the context goes on working
        assert sc.full == 1 and sd.full == 1 and np.isinf(depth).any()


# ---- errors -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("device_count", [0, 2])
def test_errors(swr, device_count):
    L, B = swr.load_library(), swr.binding
    w, h = 192, 96
    img = np.full((h, w), SENTINEL, dtype=np.uint32)
    st = B.DeltaStats()
    ctypes.memset(ctypes.byref(st), 0x7F, 48)
    with swr.Context(0, device_count=device_count) as ctx:
        assert L.swr_read_color_delta(ctx._h, img.ctypes.data, ctypes.byref(st)) == NO_SCENE        # no target
        assert L.swr_read_depth_delta(ctx._h, img.ctypes.data, ctypes.byref(st)) == NO_SCENE
        ctx.target_set(w, h)
        write(ctx, COLOR, random_words(w, h, 9))
        assert L.swr_read_color_delta(ctx._h, None, ctypes.byref(st)) == BAD_ARG
        assert L.swr_read_depth_delta(ctx._h, None, ctypes.byref(st)) == BAD_ARG
        for bits in (0, 4, 8 | B.DELTA_COLOR, 0xFFFFFFFF):
            assert L.swr_delta_reset(ctx._h, bits) == BAD_ARG, bits
        assert code_of(swr, lambda: ctx.delta_reset(0))[0] == BAD_ARG
        assert bytes(st) == b"\x7f" * 48 and (img == SENTINEL).all(), "after an error nothing was written"
        # no baseline was made either: the first read that succeeds is full; stats may be NULL
        assert L.swr_read_color_delta(ctx._h, img.ctypes.data, None) == 0
        side = Side(swr, ctx, COLOR)
        assert ctx.read_color_delta(img.view(np.uint8).reshape(h, w, 4)).tiles_changed == 0
        ctx.delta_reset(B.DELTA_COLOR)
        assert side.read("after the errors")[0].full == 1


@gpu
def test_failed_context_returns_its_sticky_error(swr):
    v, i = small_mesh()
    w, h = 192, 96
    ctx = swr.Context(0, wait_budget_ms=300)
    try:
        ctx.scene_upload(v, i)
        ctx.target_set(w, h)
        ctx.draw(IDENT, DT)
        depth = np.zeros((h, w), dtype=np.float32)
        assert ctx.read_depth_delta(depth).full == 1
        ctx.debug_fault(swr.binding.FAULT_ENQUEUE)      # the next frame's raster share fails as if a launch had returned an error
        try:
            ctx.draw(IDENT, DT)
        except swr.SwrError as e:
            assert e.code == HIP
        keep = depth.copy()
        assert code_of(swr, lambda: ctx.read_depth_delta(depth))[0] == HIP
        assert code_of(swr, lambda: ctx.read_color_delta(np.zeros((h, w, 4), dtype=np.uint8)))[0] == HIP
        assert code_of(swr, lambda: ctx.delta_reset())[0] == HIP
        assert np.array_equal(depth.view(np.uint32), keep.view(np.uint32))
    finally:
        ctx.close()


@gpu
def test_frame_loop_example_prints_the_tiles_that_changed(swr, capsys):
    """examples/frame_loop.py --delta: the host-visible loop through swr_render_delta equals the loop through the plain reads."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    res, stats = fl.run_delta(3, 256, None, depth_test=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("delta:")]
    assert len(lines) == 3 and "(full)" in lines[0] and "(full)" not in lines[1]
    for k, ln in enumerate(lines):
        m = re.match(r"delta: frame (\d+): colour (\d+) of (\d+) tiles changed, (\d+) bytes copied( \(full\))?; depth (\d+) of (\d+) tiles, (\d+) bytes", ln)
        assert m and int(m.group(1)) == k and int(m.group(3)) == 32 and int(m.group(2)) == stats[k][0].tiles_changed
        assert 0 < int(m.group(2)) <= 32 and int(m.group(6)) == stats[k][1].tiles_changed
    _, _, plain = fl.run(3, 256, None, depth_test=True)
    for (c, d), (pc, pd, _) in zip(res, plain):
        assert np.array_equal(c, pc) and np.array_equal(d.view(np.uint32), pd.view(np.uint32))
