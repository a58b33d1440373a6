"""Alpha blending (SWR_FLAG_BLEND, swr_blend_set; include/swr.h "Alpha blending").

The expected images come from a NumPy model written from the header text alone: every primitive of the frame, in order, is drawn
ALONE by the unchanged oracle as a clear frame under the frame's rule set — that gives its covered pixels, its source bytes and
(z-test) its fragment depths; a pixel the single-triangle z frame leaves at +inf carries no passing fragment — and folded into the
starting image with the header's integer formulas.  Draw lists, clip frames and culling use the restatements of tests/frame_model.py.
Everything is compared bit for bit: colour and depth, no tolerance anywhere.
"""
import numpy as np
import pytest

import frame_model as FM
import kernel_matrix as K
import test_depth_clip as DC

DT, NC, METAL, LOAD, IDS = 1, 2, 4, 16, 32
CB, CF, CCW, CLIP, PERSP, BLEND = 64, 128, 256, 1024, 2048, 4096
OVER, ADD = 0, 1
IDENT = K.IDENT
gpu = pytest.mark.gpu


# ---- the model (tests/frame_model.py holds it: the frame model uses it for blend frames) -----------------------------------------------
blend_bytes, primitives, model = FM.blend_bytes, FM.primitives, FM.model


def same(got, want, what=""):
    FM.same((got[0], got[1], None), (want[0], want[1], None), what)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def soup(n, seed, cx=0.0, cy=0.0, spread=0.9, r=0.35, z=(0.05, 0.95)):
    rng = np.random.default_rng(seed)
    cen = np.stack([rng.uniform(cx - spread, cx + spread, n), rng.uniform(cy - spread, cy + spread, n)], axis=1)
    xy = cen[:, None, :] + rng.uniform(-r, r, (n, 3, 2))
    v = np.zeros((3 * n, 8), dtype=np.float32)
    v[:, 0:2] = xy.reshape(-1, 2)
    v[:, 2] = rng.uniform(z[0], z[1], 3 * n)
    v[:, 4:7] = rng.uniform(0.0, 1.0, (3 * n, 3))
    return v, np.arange(3 * n, dtype=np.int64)


def spec_of(v, i, w, h, flags, m=IDENT, items=None, key=None):
    return FM.FrameSpec(v, i, w, h, flags, transform=None if items is not None else np.asarray(m, dtype=np.float32),
                        items=items, key=key)


def frame(ctx, spec, mode, opacity, start=None, upload=True):
    """Draw the blend frame on ctx (target set by the caller) and read it back."""
    if upload:
        ctx.scene_upload(spec.vertices, spec.indices)
    if start is not None:
        ctx.target_write(start[0], start[1])
    ctx.blend_set(mode, opacity)
    if spec.items is not None:
        ctx.draw_list(spec.items, spec.flags | BLEND)
    else:
        ctx.draw(spec.transform, spec.flags | BLEND)
    ctx.sync()
    return ctx.read_color(), ctx.read_depth()


def check(swr, oracle, spec, mode, opacity, start=None, what="", prepare=None, device_count=0):
    want = model(oracle, spec, mode, opacity, start)
    with swr.Context(0, device_count=device_count) as ctx:
        if prepare:
            prepare(ctx)
        ctx.target_set(spec.width, spec.height)
        got = frame(ctx, spec, mode, opacity, start if spec.flags & LOAD else None)
    same(got, want, what)
    return got


# ---- CPU: the arithmetic's identities ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [OVER, ADD])
def test_arithmetic_identities(mode):
    s, d = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for A in (0, 1, 127, 128, 254, 255):
        r = blend_bytes(s, d, A, mode)
        assert r.min() >= 0 and r.max() <= 255
        if A == 0:
            assert (r == d).all()                                       # opacity 0 is the identity
        if A == 255 and mode == OVER:
            assert (r == s).all()                                       # opacity 255 replaces
        if A == 255 and mode == ADD:
            assert (r == np.minimum(255, s + d)).all()
        if mode == OVER:
            assert ((r >= np.minimum(s, d)) & (r <= np.maximum(s, d))).all()        # a weighted mean of s and d
            assert (blend_bytes(s, s, A, mode) == s).all()              # a constant stays
            assert (np.diff(r, axis=0) >= 0).all() and (np.diff(r, axis=1) >= 0).all()
        else:
            assert (r >= d).all() and (np.diff(r, axis=0) >= 0).all() and (np.diff(r, axis=1) >= 0).all()
            assert (r == np.minimum(255, d + np.rint(s * A / 255.0).astype(np.int64))).all()


# ---- 1: order inside one tile -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order", [1, 0, -1])
@pytest.mark.parametrize("mode,opacity", [(OVER, 128), (ADD, 90)])
def test_order_inside_one_tile(swr, oracle, order, mode, opacity):
    """300 overlapping triangles with distinct colours over one 16x16 block: more than a chunk of 64 and more than 256 lanes; a
    wrong order changes bytes.  The Morton-reordered stream, the caller's order, and the no-reordering path of huge scenes."""
    w, h = 130, 70
    v, i = soup(300, 0xB1, cx=-0.6, cy=0.35, spread=0.06, r=0.16)
    spec = spec_of(v, i, w, h, 0, key="one-tile")
    check(swr, oracle, spec, mode, opacity, what=f"order {order}",
          prepare=lambda ctx: ctx.debug_set(swr.binding.DEBUG_STREAM_ORDER, order))


# ---- 2: target sizes ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h", [(1, 1), (64, 32), (65, 33), (130, 70), (513, 257)])
def test_target_sizes(swr, oracle, w, h):
    v, i = soup(120, 0xB2 + w, r=0.5)
    check(swr, oracle, spec_of(v, i, w, h, 0), OVER, 77, what=f"{w}x{h} painter")
    check(swr, oracle, spec_of(v, i, w, h, DT), ADD, 200, what=f"{w}x{h} z-test")


# ---- 3: the transparent pass over an opaque scene -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("flags", [DT, METAL])
def test_ztested_blend_over_opaque_frame(swr, oracle, flags):
    w, h = 130, 70
    va, ia = soup(200, 0xB3, r=0.4)
    vb, ib = soup(200, 0xB4, r=0.4)
    ca, da = K.oracle_clear(oracle, va, ia, IDENT, w, h, flags)
    spec = spec_of(vb, ib, w, h, flags | LOAD)
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(va, ia)
        ctx.draw(IDENT, flags)
        ctx.sync()
        same((ctx.read_color(), ctx.read_depth()), (ca, da), "the opaque frame")
        got = frame(ctx, spec, OVER, 128)
        same(got, model(oracle, spec, OVER, 128, (ca, da)), "blend over the opaque frame")
        assert got[1].tobytes() == da.tobytes()
        # a starting image with NaN (one with a payload), -0, +-inf and denormals: depth comes back bit for bit
        c0, d0 = K.special_start(w, h, 0xB5)
        got = frame(ctx, spec, OVER, 128, start=(c0, d0), upload=False)
        same(got, model(oracle, spec, OVER, 128, (c0, d0)), "blend over a special starting image")
        assert got[1].tobytes() == d0.tobytes()


# ---- 4: the header's properties, library against library ----------------------------------------------------------------------------
@gpu
def test_property_a_opacity_255_is_painters_order(swr):
    w, h = 130, 70
    v, i = soup(400, 0xB6, r=0.3)
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, i)
        ctx.draw(IDENT, 0)
        ctx.sync()
        plain = ctx.read_color()
        ctx.blend_set(OVER, 255)
        ctx.draw(IDENT, BLEND)
        ctx.sync()
        assert np.array_equal(ctx.read_color(), plain)
        assert np.isposinf(ctx.read_depth()).all()


@gpu
@pytest.mark.parametrize("mode", [OVER, ADD])
@pytest.mark.parametrize("flags", [0, DT, METAL])
def test_property_b_opacity_0_keeps_the_image(swr, mode, flags):
    w, h = 130, 70
    v, i = soup(300, 0xB7, r=0.3)
    c0, d0 = K.special_start(w, h, 0xB8)
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, i)
        ctx.blend_set(mode, 0)
        ctx.draw(IDENT, flags | BLEND)
        ctx.sync()
        assert not ctx.read_color().any() and np.isposinf(ctx.read_depth()).all()
        ctx.target_write(c0, d0)
        ctx.draw(IDENT, flags | BLEND | LOAD)
        ctx.sync()
        assert np.array_equal(ctx.read_color(), c0) and ctx.read_depth().tobytes() == d0.tobytes()


@gpu
@pytest.mark.parametrize("flags", [0, DT])
@pytest.mark.parametrize("loaded", [False, True])
def test_property_c_draw_list_equals_its_chain(swr, flags, loaded):
    w, h = 130, 70
    v, i = soup(240, 0xB9, r=0.35)
    ms = [K.affine_matrix(0.1 * k, 0.9 - 0.05 * k, 0.05 * k, -0.03 * k) for k in range(5)]
    items = [(0, 360, ms[0]), (180, 540, ms[1]), (0, 720, ms[2]), (360, 0, ms[3]), (90, 300, ms[4])]     # overlapping ranges, an empty item
    c0, d0 = K.special_start(w, h, 0xBA)
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, i)
        ctx.blend_set(OVER, 150)
        if loaded:
            ctx.target_write(c0, d0)
        ctx.draw_list(items, flags | BLEND | (LOAD if loaded else 0))
        ctx.sync()
        lc, ld = ctx.read_color(), ctx.read_depth()
        ctx.target_set(w, h)
        if loaded:
            ctx.target_write(c0, d0)
        for k, it in enumerate(items):
            ctx.draw_list([it], flags | BLEND | (LOAD if loaded or k else 0))
        ctx.sync()
        assert np.array_equal(ctx.read_color(), lc) and ctx.read_depth().tobytes() == ld.tobytes()
        assert lc.any()


@gpu
@pytest.mark.parametrize("flags", [0, DT])
def test_draw_list_against_the_model(swr, oracle, flags):
    w, h = 130, 70
    v, i = soup(120, 0xBB, r=0.35)
    items = [(0, 180, K.affine_matrix(0.2, 0.8)), (90, 270, K.affine_matrix(-0.3, 1.1, 0.1, 0.1)), (0, 360, K.mirrored(K.affine_matrix()))]
    start = K.special_start(w, h, 0xBC)
    check(swr, oracle, spec_of(v, i, w, h, flags | LOAD, items=items), OVER, 99, start, "draw list")


# ---- 5: saturation, the clear start's alpha, the extreme opacities ------------------------------------------------------------------
@gpu
def test_add_saturates(swr, oracle):
    w, h = 130, 70
    v, i = soup(200, 0xBD, r=0.5)
    v[:, 4:7] = 0.5 + 0.5 * v[:, 4:7]
    got = check(swr, oracle, spec_of(v, i, w, h, 0, key="bright"), ADD, 255, what="ADD 255, clear start")
    assert (got[0] == 255).all(axis=-1).any() and (got[0][..., 3] == 0).any()


@gpu
@pytest.mark.parametrize("mode", [OVER, ADD])
@pytest.mark.parametrize("opacity", [1, 254])
def test_extreme_opacities(swr, oracle, mode, opacity):
    w, h = 130, 70
    v, i = soup(200, 0xBD, r=0.5)
    v[:, 4:7] = 0.5 + 0.5 * v[:, 4:7]
    check(swr, oracle, spec_of(v, i, w, h, 0, key="bright"), mode, opacity, what="clear start")
    check(swr, oracle, spec_of(v, i, w, h, LOAD, key="bright"), mode, opacity, K.special_start(w, h, 0xBE), "load start")


# ---- 6: cull, depth clip, Metal rules -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("flags", [CB, CF | CCW, DT | CB | CCW, METAL, METAL | CF], ids=lambda f: f"flags{f}")
@pytest.mark.parametrize("loaded", [False, True])
def test_cull_and_metal_rules(swr, oracle, flags, loaded):
    w, h = 130, 70
    v, i = soup(250, 0xBF, r=0.4)
    m = K.mirrored(K.affine_matrix()) if flags & CCW else K.affine_matrix()
    spec = spec_of(v, i, w, h, flags | (LOAD if loaded else 0), m=m, key=("cull", bool(flags & CCW)))
    check(swr, oracle, spec, OVER, 128, K.special_start(w, h, 0xC0) if loaded else None, f"flags {flags}")


@gpu
@pytest.mark.parametrize("flags", [CLIP, CLIP | DT, CLIP | METAL, CLIP | DT | CB], ids=lambda f: f"flags{f}")
@pytest.mark.parametrize("loaded", [False, True])
def test_depth_clip(swr, oracle, flags, loaded):
    """Triangles that cross the near plane: their fans blend in fan order, in their original's place."""
    w, h = 130, 70
    v, i = DC.straddling_soup(150, 0xC1)
    m = DC.metal_perspective(aspect=w / h)
    assert DC.crosses(v, i, m).sum() > 20
    spec = spec_of(v, i, w, h, flags | (LOAD if loaded else 0), m=m, key="clip")
    check(swr, oracle, spec, OVER, 128, K.special_start(w, h, 0xC2) if loaded else None, f"flags {flags}")


# ---- 7: degenerate triangles --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("flags", [0, DT])
def test_degenerate_triangles(swr, oracle, flags):
    """det == 0 (collinear after truncation): the painter's span blends (0, 0, 0); under the z-test its NaN depth never passes."""
    w, h = 130, 70
    v, i = soup(60, 0xC3, r=0.4)
    v[0:90:3, 1] = v[1:90:3, 1] = v[2:90:3, 1]                  # the first 30 triangles: all three vertices on one row
    v[90:120, 0:2] = np.repeat(v[90:120:3, 0:2], 3, axis=0)     # the next 10: a single point
    start = (np.full((h, w, 4), 200, dtype=np.uint8), np.full((h, w), 0.5, dtype=np.float32))
    check(swr, oracle, spec_of(v, i, w, h, flags | LOAD), OVER, 128, start, "degenerate")
    if not flags:
        alone = spec_of(v[:90], i[:90], w, h, LOAD)
        c, _ = model(oracle, alone, OVER, 128, start)
        assert (c != 200).any(), "the degenerate spans cover pixels"


# ---- 8: bands -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bands", [2, 3])
def test_bands(swr, oracle, bands):
    w, h = 64, 96
    v, i = soup(300, 0xC4, r=0.4)
    start = K.special_start(w, h, 0xC5)
    check(swr, oracle, spec_of(v, i, w, h, DT | LOAD, key="bands"), OVER, 128, start, f"{bands} bands", device_count=bands)
    check(swr, oracle, spec_of(v, i, w, h, 0), ADD, 60, None, f"{bands} bands, clear start", device_count=bands)


# ---- 9: swr_render ------------------------------------------------------------------------------------------------------------------
@gpu
def test_swr_render(swr, oracle):
    w, h = 130, 70
    v, i = soup(200, 0xC6, r=0.4)
    c0, d0 = K.special_start(w, h, 0xC7)
    spec = spec_of(v, i, w, h, DT | LOAD, m=K.affine_matrix())
    with swr.Context(0) as ctx:
        ctx.blend_set(ADD, 111)
        c, d = ctx.render(v, i, spec.transform, w, h, DT | LOAD | BLEND, color=c0.copy(), depth=d0.copy())
        same((c, d), model(oracle, spec, ADD, 111, (c0, d0)), "swr_render, caller images as the start")
        c, d = ctx.render(v, i, spec.transform, w, h, BLEND)
        same((c, d), model(oracle, spec_of(v, i, w, h, 0, m=K.affine_matrix()), ADD, 111), "swr_render, clear start")


# ---- 10, 11: bin overflow and the other binning paths -------------------------------------------------------------------------------
@gpu
def test_bin_overflow_is_repaired(swr, oracle):
    """1 500 triangles in one tile of a 256x256 target (tile regions of 1 024 entries): the overflowed blend load frame is redrawn
    from the same starting image."""
    w, h = 256, 256
    v, i = soup(1500, 0xC8, cx=0.4, cy=-0.3, spread=0.02, r=0.08)
    c0, d0 = K.special_start(w, h, 0xC9)
    spec = spec_of(v, i, w, h, LOAD, key="crowd")
    want = model(oracle, spec, OVER, 128, (c0, d0))
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v[:30], i[:30])
        ctx.draw(IDENT, 0)
        same(frame(ctx, spec, OVER, 128, start=(c0, d0)), want, "the last blend load frame of a chain")
    with swr.Context(0) as ctx:
        ctx.blend_set(OVER, 128)
        c, d = ctx.render(v, i, IDENT, w, h, LOAD | BLEND, color=c0.copy(), depth=d0.copy())
        same((c, d), want, "swr_render")
        assert ctx.render_timings()["frames"] == 2


@gpu
@pytest.mark.parametrize("bin_mode", [1, 3])
@pytest.mark.parametrize("flags", [0, DT])
def test_other_binning_paths(swr, oracle, bin_mode, flags):
    w, h = 256, 256
    v, i = soup(1500, 0xC8, cx=0.4, cy=-0.3, spread=0.02, r=0.08)
    start = K.special_start(w, h, 0xC9)
    check(swr, oracle, spec_of(v, i, w, h, flags | LOAD, key="crowd"), OVER, 128, start, f"bin mode {bin_mode}",
          prepare=lambda ctx: ctx.debug_set(swr.binding.DEBUG_BIN_MODE, bin_mode))


# ---- 12: the big-triangle path ------------------------------------------------------------------------------------------------------
@gpu
def test_triangle_covering_hundreds_of_tiles(swr, oracle):
    w, h = 1024, 1024
    v = np.zeros((3, 8), dtype=np.float32)
    v[:, 0:3] = [(-0.98, -0.97, 0.2), (0.99, -0.9, 0.5), (0.05, 0.98, 0.8)]
    v[:, 4:7] = [(1.0, 0.1, 0.2), (0.2, 1.0, 0.1), (0.1, 0.3, 1.0)]
    i = np.arange(3, dtype=np.int64)
    want1 = model(oracle, spec_of(v, i, w, h, 0), OVER, 128)
    want2 = model(oracle, spec_of(v, i, w, h, LOAD), OVER, 128, want1)
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, i)
        ctx.blend_set(OVER, 128)
        ctx.draw(IDENT, BLEND)
        ctx.sync()
        same((ctx.read_color(), ctx.read_depth()), want1, "blended once")
        ctx.draw(IDENT, BLEND | LOAD)
        ctx.draw(IDENT, BLEND)              # (the frame after one that met a big triangle)
        ctx.sync()
        same((ctx.read_color(), ctx.read_depth()), want1, "a clear-start frame again")
        ctx.draw(IDENT, BLEND | LOAD)
        ctx.sync()
        same((ctx.read_color(), ctx.read_depth()), want2, "blended twice")


# ---- 13: frames without the bit are untouched ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("flags", [0, DT, DT | NC, METAL])
def test_plain_frames_around_blend_frames(swr, flags):
    w, h = 130, 70
    v, i = soup(400, 0xCA, r=0.3)
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, i)
        ctx.draw(IDENT, flags)
        ctx.sync()
        fresh = (None if flags & NC else ctx.read_color(), ctx.read_depth())
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, i)
        ctx.blend_set(ADD, 40)
        for k in range(3):
            ctx.draw(IDENT, flags)
            if k == 0:
                ctx.sync()
                assert ctx.read_depth().tobytes() == fresh[1].tobytes()
            ctx.draw(IDENT, (flags & ~NC) | BLEND | LOAD)
            ctx.draw(IDENT, BLEND)
        ctx.draw(IDENT, flags)
        ctx.sync()
        assert ctx.read_depth().tobytes() == fresh[1].tobytes()
        if fresh[0] is not None:
            assert np.array_equal(ctx.read_color(), fresh[0])


# ---- 14: the state travels with the frame -------------------------------------------------------------------------------------------
@gpu
def test_blend_set_between_frames_in_flight(swr, oracle):
    w, h = 130, 70
    v, i = soup(300, 0xCB, r=0.4)
    first = model(oracle, spec_of(v, i, w, h, 0, key="flight"), OVER, 60)
    second = model(oracle, spec_of(v, i, w, h, LOAD, key="flight"), ADD, 200, first)
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, i)
        imgs = [(swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)) for _ in range(2)]
        ctx.blend_set(OVER, 60)
        ctx.draw(IDENT, BLEND)
        ctx.present(*imgs[0])
        ctx.blend_set(ADD, 200)
        ctx.draw(IDENT, BLEND | LOAD)
        ctx.present(*imgs[1])
        ctx.blend_set(OVER, 0)
        ctx.present_wait()
        same((imgs[0][0].array, imgs[0][1].array), first, "the first frame keeps OVER 60")
        same((imgs[1][0].array, imgs[1][1].array), second, "the second frame keeps ADD 200")
        for a, b in imgs:
            a.free(); b.free()


# ---- bins of more than one sorted run -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bin_mode", [0, 1])
@pytest.mark.parametrize("flags", [0, DT])
def test_bin_longer_than_one_sorted_run(swr, bin_mode, flags):
    """5 000 small triangles in one tile: the bin is ordered in two runs of 4 096 merged through global memory.  Library against
    library: the one frame equals the chain of five blend load frames of 1 000 triangles each (bins of one run, which the model
    covers), with and without the z-test."""
    w, h = 130, 70
    v, i = soup(5000, 0xCC, cx=0.3, cy=0.3, spread=0.05, r=0.12)
    c0, d0 = K.special_start(w, h, 0xCD)
    with swr.Context(0) as ctx:
        ctx.debug_set(swr.binding.DEBUG_BIN_MODE, bin_mode)
        ctx.target_set(w, h)
        ctx.scene_upload(v, i)
        ctx.blend_set(OVER, 140)
        ctx.target_write(c0, d0)
        ctx.draw(IDENT, flags | BLEND | LOAD)
        ctx.sync()
        whole = ctx.read_color(), ctx.read_depth()
        ctx.target_write(c0, d0)
        for k in range(5):
            ctx.draw_list([(3000 * k, 3000, IDENT)], flags | BLEND | LOAD)
        ctx.sync()
        assert np.array_equal(ctx.read_color(), whole[0]) and ctx.read_depth().tobytes() == whole[1].tobytes()
        assert whole[1].tobytes() == d0.tobytes() and not np.array_equal(whole[0], c0)
