"""Supersampled resolve (swr_read_color_resolved, swr_read_depth_resolved, swr_render_resolved; include/swr.h "Supersampled resolve",
DESIGN.md §19).

The expected images come from tests/resolve_model.py, a NumPy model written from the header text.  Its inputs are images the test
itself wrote with swr_target_write, or the CPU oracle's frame at S*w x S*h (through tests/frame_model.py; the blend frame through the
model of tests/test_blend.py, which restates it with frame_model's pieces).  The model is never fed by the library.  Everything is
compared bit for bit: colour bytes and depth bits, no tolerance anywhere.
"""
import numpy as np
import pytest

import frame_model as FM
import kernel_matrix as K
import resolve_model as RM
import test_blend as TB

DT, NC, METAL, LOAD, IDS, BLEND = 1, 2, 4, 16, 32, 4096
SAMPLE0, MIN = RM.SAMPLE0, RM.MIN
IDENT = K.IDENT
VERTICES = 2
gpu = pytest.mark.gpu

# depth specials: NaNs with distinct payloads (quiet, signalling, negative), +-0, +-inf, +-denormals (the smallest and the largest),
# the smallest normals and ordinary values
SPECIAL_BITS = np.array([0x7FC00000, 0x7FC01234, 0x7F800001, 0xFFC00ABC, 0x7FFFFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                         0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x3F000000, 0x3F000001, 0xBF000000,
                         0x3E99999A, 0x3F7FFFFF], dtype=np.uint32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_depth(got, want, what):
    bad = np.nonzero(bits(got) != bits(want))
    assert bad[0].size == 0, f"{what}: {bad[0].size} depth values differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): " \
                             f"{bits(got)[bad][0]:#010x} vs {bits(want)[bad][0]:#010x}"


def same_color(got, want, what):
    bad = np.nonzero((got != want).any(axis=-1))
    assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): " \
                             f"{got[bad[0][0], bad[1][0]]} vs {want[bad[0][0], bad[1][0]]}"


def injected(W, H, seed):
    """Seeded random colour bytes and a depth image that is half specials, half ordinary values in (0, 1)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    d = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    mask = rng.uniform(size=(H, W)) < 0.5
    bits(d)[mask] = SPECIAL_BITS[rng.integers(0, SPECIAL_BITS.size, (H, W))][mask]
    return c, d


def check_reads(ctx, c, d, factors=(1, 2, 4), what=""):
    """Every resolved read of the context's current image against the model of (c, d)."""
    for S in factors:
        same_color(ctx.read_color_resolved(S), RM.color(c, S), f"{what} colour, S={S}")
        for filt in (SAMPLE0, MIN):
            same_depth(ctx.read_depth_resolved(S, filt), RM.depth(d, S, filt), f"{what} depth, S={S}, filter {filt}")


def write_and_check(swr, c, d, factors=(1, 2, 4), what=""):
    H, W = d.shape
    with swr.Context(0) as ctx:
        ctx.target_set(W, H)
        ctx.target_write(c, d)
        check_reads(ctx, c, d, factors, what)
        return ctx.read_color(), ctx.read_depth()


# ---- CPU: the model against the header's own examples ----------------------------------------------------------------------------------
def test_model_follows_the_header():
    c = np.zeros((2, 2, 4), dtype=np.uint8)
    c[0, 0] = (1, 2, 3, 255)
    assert RM.color(c, 2).tolist() == [[[0, 1, 1, 64]]]                       # (1 + 2) / 4 = 0, (2 + 2) / 4 = 1, (3 + 2) / 4 = 1, (255 + 2) / 4
    d = np.array([[np.nan, 3.0], [-0.0, 0.0]], dtype=np.float32)
    assert bits(RM.depth(d, 2, MIN))[0, 0] == 0x80000000                      # NaN loses; -0 met first is kept over +0
    assert bits(RM.depth(d, 2, SAMPLE0))[0, 0] == bits(d)[0, 0]
    n = np.zeros((2, 2), dtype=np.float32)
    bits(n)[:] = [[0x7FC01234, 0x7FC00000], [0xFFC00ABC, 0x7F800001]]
    assert bits(RM.depth(n, 2, MIN))[0, 0] == 0x7FC01234                      # all NaN: the first one's bits, payload included


# ---- 1: injected images, no draw ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("W,H", [(4, 4), (72, 36), (200, 100), (4096, 8)])
def test_injected_images(swr, W, H):
    c, d = injected(W, H, 0x5E50 + W)
    rc, rd = write_and_check(swr, c, d, what=f"{W}x{H}")
    # factor 1 is byte for byte the plain read (checked against the model above, and here against the plain read itself)
    assert np.array_equal(rc, c) and bits(rd).tobytes() == bits(d).tobytes()


# ---- 2: rounding and carries -------------------------------------------------------------------------------------------------------------
def block_with_sum(S, total, rng):
    """S*S bytes that add up to `total`, spread at random."""
    n = S * S
    assert 0 <= total <= 255 * n
    v = np.full(n, total // n, dtype=np.int64)
    v[:total - int(v.sum())] += 1
    for _ in range(4 * n):                       # move weight around, keeping the sum
        a, b = rng.integers(0, n, 2)
        k = int(min(v[a], 255 - v[b], rng.integers(0, 256)))
        v[a] -= k
        v[b] += k
    assert v.sum() == total and v.min() >= 0 and v.max() <= 255
    return rng.permutation(v).reshape(S, S).astype(np.uint8)


@gpu
@pytest.mark.parametrize("S,sums", [(2, (1, 2, 3, 1019, 1020)), (4, (7, 8, 4079, 4080))])
def test_rounding_and_carries(swr, S, sums):
    rng = np.random.default_rng(0xCA44 + S)
    blocks = []
    for t in sums:                               # the sum in one channel, every channel in turn; the other channels random
        for ch in range(4):
            b = rng.integers(0, 256, (S, S, 4), dtype=np.uint8)
            b[..., ch] = block_with_sum(S, t, rng)
            blocks.append(b)
        blocks.append(np.stack([block_with_sum(S, t, rng) for _ in range(4)], axis=-1))      # ... and in all four at once
    blocks.append(np.full((S, S, 4), 255, dtype=np.uint8))
    for pattern in ((0, 255, 0, 255), (255, 0, 255, 0), (255, 255, 0, 0), (0, 0, 255, 255), (255, 0, 0, 255)):
        blocks.append(np.broadcast_to(np.array(pattern, dtype=np.uint8), (S, S, 4)).copy())   # channels alternating 0 and 255
        b = np.zeros((S, S, 4), dtype=np.uint8)
        b[0, 0] = pattern                                                                        # ... and one such sample among zeros
        blocks.append(b)
    while len(blocks) % 8:
        blocks.append(rng.integers(0, 256, (S, S, 4), dtype=np.uint8))
    rows = [np.concatenate(blocks[k:k + 8], axis=1) for k in range(0, len(blocks), 8)]
    c = np.ascontiguousarray(np.concatenate(rows, axis=0))
    want = RM.color(c, S)
    full = np.nonzero((c.reshape(c.shape[0] // S, S, c.shape[1] // S, S, 4) == 255).all(axis=(1, 3, 4)))
    assert full[0].size >= 1 and (want[full] == 255).all()                                       # all-255 blocks give 255 in every channel
    d = np.zeros(c.shape[:2], dtype=np.float32)
    write_and_check(swr, c, d, factors=(S,), what="hand-made blocks")


# ---- 3: MIN specials, one block each -----------------------------------------------------------------------------------------------------
def min_blocks(S):
    n = S * S
    F = lambda x: np.array([x], dtype=np.float32).view(np.uint32)[0]   # noqa: E731
    NAN_A, NAN_B, NAN_C = 0x7FC01234, 0xFFC00ABC, 0x7F800001
    PZ, NZ, PINF, NINF = 0x00000000, 0x80000000, 0x7F800000, 0xFF800000
    out = []
    out.append(([NAN_A] + [F(0.5 + 0.01 * k) for k in range(n - 1)], F(0.5)))                    # NaN first with numbers after
    out.append(([NAN_A, NAN_B, NAN_C] + [NAN_B] * (n - 3), NAN_A))                               # all NaN: the first payload is kept
    out.append(([NAN_B, NAN_A] + [PINF] * (n - 2), PINF))                                        # +inf beats a NaN
    out.append(([PZ, NZ] + [F(1.0)] * (n - 2), PZ))                                              # (+0, -0, ...): the first met
    out.append(([NZ, PZ] + [F(1.0)] * (n - 2), NZ))                                              # (-0, +0, ...)
    out.append(([F(1.0), NZ, PZ] + [NAN_A] * (n - 3), NZ))
    out.append(([F(0.25), NINF, F(-3.0)] + [NAN_C] * (n - 3), NINF))                             # -inf present
    out.append(([PINF] * n, PINF))                                                               # all +inf (the cleared depth)
    out.append(([0x00000002, 0x00000001, 0x80000001, 0x80000002][:n] + [PZ] * (n - 4), 0x80000002))   # denormals compare exactly
    for pos in range(n):                                                                         # the minimum at each position in turn
        blk = [F(0.5 + 0.001 * ((k * 7) % n)) for k in range(n)]
        blk[pos] = F(0.125)
        out.append((blk, F(0.125)))
        blk = [NAN_A if k % 2 else F(0.75) for k in range(n)]                                    # ... among NaNs
        blk[pos] = F(-2.0)
        out.append((blk, F(-2.0)))
    return out


@gpu
@pytest.mark.parametrize("S", [2, 4])
def test_min_specials(swr, S):
    blocks = min_blocks(S)
    while len(blocks) % 4:
        blocks.append(blocks[-1])
    img = [np.array(b, dtype=np.uint32).reshape(S, S) for b, _ in blocks]
    d = np.ascontiguousarray(np.concatenate([np.concatenate(img[k:k + 4], axis=1) for k in range(0, len(img), 4)], axis=0)).view(np.float32)
    hand = np.array([m for _, m in blocks], dtype=np.uint32).reshape(-1, 4)
    assert np.array_equal(bits(RM.depth(d, S, MIN)), hand), "the model disagrees with the hand-worked minima"
    c = np.zeros(d.shape + (4,), dtype=np.uint8)
    with swr.Context(0) as ctx:
        ctx.target_set(d.shape[1], d.shape[0])
        ctx.target_write(c, d)
        got = ctx.read_depth_resolved(S, MIN)
        assert np.array_equal(bits(got), hand), f"S={S}: {bits(got).tolist()} vs {hand.tolist()}"
        same_depth(ctx.read_depth_resolved(S, SAMPLE0), d[::S, ::S], f"S={S}, sample 0")


# ---- 4: drawn frames against the oracle --------------------------------------------------------------------------------------------------
w0, h0 = 160, 96
_CACHE = {}


def soup_spec(swr, S, flags, m=None, n=300, seed=0x55A1, r=0.12):
    s = swr.scenes.random_soup(n, w0 * S, h0 * S, seed, r_ndc=r, margin=1.1)
    m = s.transform if m is None else m
    return FM.FrameSpec(s.vertices, s.indices, w0 * S, h0 * S, flags, transform=np.asarray(m, dtype=np.float32),
                        key=("soup", S, n, seed, np.asarray(m, dtype=np.float32).tobytes()))


@gpu
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("flags", [DT, 0, METAL])
def test_drawn_frames(swr, oracle, S, flags):
    spec = soup_spec(swr, S, flags)
    c, d, _ = FM.expect(oracle, spec, cache=_CACHE)
    frac = RM.partial_fraction(RM.color(c, S))
    assert frac >= 0.05, f"only {frac:.3f} of the oracle's resolved pixels are partial"
    with swr.Context(0) as ctx:
        ctx.scene_upload(spec.vertices, spec.indices)
        ctx.target_set(spec.width, spec.height)
        ctx.draw(spec.transform, flags)
        check_reads(ctx, c, d, (S,), f"flags {flags}")
        got = ctx.read_color_resolved(S)
        assert RM.partial_fraction(got) >= 0.05


@gpu
@pytest.mark.parametrize("S", [2, 4])
def test_blend_frame_over_the_opaque_one(swr, oracle, S):
    opaque = soup_spec(swr, S, DT)
    c0, d0, _ = FM.expect(oracle, opaque, cache=_CACHE)
    glass = soup_spec(swr, S, DT | LOAD, m=K.affine_matrix(), n=60, seed=0x55B2, r=0.2)
    c, d = TB.model(oracle, glass, TB.OVER, 150, (c0, d0))
    with swr.Context(0) as ctx:
        ctx.target_set(opaque.width, opaque.height)
        ctx.scene_upload(opaque.vertices, opaque.indices)
        ctx.draw(opaque.transform, DT)
        ctx.scene_upload(glass.vertices, glass.indices)
        ctx.blend_set(TB.OVER, 150)
        ctx.draw(glass.transform, BLEND | LOAD | DT)
        check_reads(ctx, c, d, (S,), "blend frame")
    assert not np.array_equal(c, c0)


# ---- 5: bands ----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("S", [2, 4])
def test_one_band_leaves_the_other_rows_untouched(swr, S):
    w, h = 40, 40
    W, H = w * S, h * S                          # 80 or 160 rows: the band [32, 64) lies inside
    c, d = injected(W, H, 0xBA2D + S)
    with swr.Context(0) as ctx:
        ctx.target_set(W, H, row_begin=32, row_end=64)
        ctx.target_write(c, d)
        r0, r1 = 32 // S, 64 // S
        oc = np.full((h, w, 4), 0xA5, dtype=np.uint8)
        ctx.read_color_resolved(S, out=oc)
        want = np.full((h, w, 4), 0xA5, dtype=np.uint8)
        want[r0:r1] = RM.color(c, S)[r0:r1]
        same_color(oc, want, "band rows")
        for filt in (SAMPLE0, MIN):
            od = np.full((h, w), -77.0, dtype=np.float32)
            ctx.read_depth_resolved(S, filt, out=od)
            wd = np.full((h, w), -77.0, dtype=np.float32)
            wd[r0:r1] = RM.depth(d, S, filt)[r0:r1]
            same_depth(od, wd, f"band rows, filter {filt}")


@gpu
@pytest.mark.parametrize("bands", [2, 3])
@pytest.mark.parametrize("S", [2, 4])
def test_multi_device_bands(swr, bands, S):
    W, H = 40 * S, 200 * S // 2                  # H / 32 is not whole: the last band ends inside a tile row
    assert H % 32 != 0 and H % S == 0
    c, d = injected(W, H, 0xBA4D + S)
    with swr.Context(0, device_count=bands) as ctx:
        ctx.target_set(W, H)
        assert ctx.bands()[-1][2] == H
        ctx.target_write(c, d)
        got = ctx.read_color_resolved(S), ctx.read_depth_resolved(S, SAMPLE0), ctx.read_depth_resolved(S, MIN)
    with swr.Context(0) as ctx:
        ctx.target_set(W, H)
        ctx.target_write(c, d)
        one = ctx.read_color_resolved(S), ctx.read_depth_resolved(S, SAMPLE0), ctx.read_depth_resolved(S, MIN)
    same_color(got[0], one[0], "bands against one context")
    same_depth(got[1], one[1], "bands against one context, sample 0")
    same_depth(got[2], one[2], "bands against one context, min")
    same_color(got[0], RM.color(c, S), "bands against the model")
    same_depth(got[2], RM.depth(d, S, MIN), "bands against the model")


# ---- 6: the last frame, on every framebuffer ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("S", [2, 4])
def test_last_frame_of_a_burst(swr, oracle, S):
    ms = [K.affine_matrix(angle=0.1 * k, scale=0.9 - 0.05 * k, tx=0.02 * k, ty=-0.03 * k) for k in range(5)]
    specs = [soup_spec(swr, S, DT, m=m) for m in ms]
    c5, d5, _ = FM.expect(oracle, specs[-1], cache=_CACHE)
    with swr.Context(0) as ctx:
        ctx.scene_upload(specs[0].vertices, specs[0].indices)
        ctx.target_set(specs[0].width, specs[0].height)
        for sp in specs:                         # five frames, no sync: the frame lanes rotate four framebuffers
            ctx.draw(sp.transform, DT)
        check_reads(ctx, c5, d5, (S,), "fifth frame of a burst")
        # the full-size images are untouched ...
        same_color(ctx.read_color(), c5, "read_color after the resolve")
        same_depth(ctx.read_depth(), d5, "read_depth after the resolve")
        # ... and a load frame composes on them
        over = soup_spec(swr, S, DT | LOAD, m=K.affine_matrix(angle=-0.4, scale=0.7))
        c6, d6, _ = FM.expect(oracle, over, start=(c5, d5), cache=_CACHE)
        ctx.draw(over.transform, DT | LOAD)
        check_reads(ctx, c6, d6, (S,), "load frame after the resolve")
        same_color(ctx.read_color(), c6, "read_color of the load frame")


@gpu
def test_ids_stay_at_sample_resolution(swr, oracle):
    S = 2
    spec = soup_spec(swr, S, DT | IDS)
    c, d, ids = FM.expect(oracle, spec, cache=_CACHE)
    with swr.Context(0) as ctx:
        ctx.scene_upload(spec.vertices, spec.indices)
        ctx.target_set(spec.width, spec.height)
        ctx.draw(spec.transform, DT | IDS)
        check_reads(ctx, c, d, (S,), "ID frame")
        FM.same((None, None, ctx.read_ids()), (None, None, ids), "IDs after the resolve")


# ---- 7: overflow repair ------------------------------------------------------------------------------------------------------------------
@gpu
def test_overflowed_last_frame_is_repaired_before_the_resolve(swr, oracle):
    """The recipe of tests/test_blend.py: 1 500 triangles in one tile of a 256x256 target, on bins sized for ten triangles."""
    W = H = 256
    S = 2
    v, i = TB.soup(1500, 0xC8, cx=0.4, cy=-0.3, spread=0.02, r=0.08)
    spec = FM.FrameSpec(v, i, W, H, DT, transform=IDENT)
    c, d, _ = FM.expect(oracle, spec)
    with swr.Context(0) as ctx:
        ctx.target_set(W, H)
        ctx.scene_upload(v[:30], i[:30])
        ctx.draw(IDENT, 0)
        ctx.scene_upload(v, i)
        ctx.draw(IDENT, DT)                      # overflows; no sync in between
        check_reads(ctx, c, d, (S,), "repaired frame")
    with swr.Context(0) as ctx:
        oc, od = ctx.render_resolved(v, i, IDENT, W // S, H // S, DT, factor=S, depth_filter=MIN)
        assert ctx.render_timings()["frames"] == 2
        same_color(oc, RM.color(c, S), "render_resolved, repaired")
        same_depth(od, RM.depth(d, S, MIN), "render_resolved, repaired")


# ---- 8: destinations ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_pageable_and_pinned_destinations(swr):
    """A 4096x2560 target resolved by 2: the resolved image is 2048x1280, 10 MiB, so the staged (pageable) path crosses one 8 MiB chunk
    boundary."""
    S, w, h = 2, 2048, 1280
    assert w * h * 4 > (8 << 20)
    rng = np.random.default_rng(0xDE57)
    c = rng.integers(0, 256, (h * S, w * S, 4), dtype=np.uint8)
    d = rng.uniform(-1.0, 1.0, (h * S, w * S)).astype(np.float32)
    wc, wd = RM.color(c, S), RM.depth(d, S, MIN)
    hc, hd = swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)
    try:
        with swr.Context(0) as ctx:
            ctx.target_set(w * S, h * S)
            ctx.target_write(c, d)
            pc, pd = ctx.read_color_resolved(S), ctx.read_depth_resolved(S, MIN)
            ctx.read_color_resolved(S, out=hc)
            ctx.read_depth_resolved(S, MIN, out=hd)
            same_color(pc, wc, "pageable")
            same_depth(pd, wd, "pageable")
            same_color(hc.array, wc, "pinned")
            same_depth(hd.array, wd, "pinned")
    finally:
        hc.free()
        hd.free()


# ---- 9: render_resolved ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("S", [2, 4])
def test_render_resolved(swr, oracle, S):
    spec = soup_spec(swr, S, DT)
    c, d, _ = FM.expect(oracle, spec, cache=_CACHE)
    v, i, m = spec.vertices, spec.indices, spec.transform
    with swr.Context(0) as ctx:
        oc, od = ctx.render_resolved(v, i, m, w0, h0, DT, factor=S, depth_filter=MIN, scene_id=7)
        assert oc.shape == (h0, w0, 4) and od.shape == (h0, w0)
        same_color(oc, RM.color(c, S), "render_resolved")
        same_depth(od, RM.depth(d, S, MIN), "render_resolved")
        assert ctx.render_timings()["scene_cached"] == 0 and ctx.render_timings()["frames"] == 1
        oc2, od2 = ctx.render_resolved(v, i, m, w0, h0, DT, factor=S, depth_filter=SAMPLE0, scene_id=7)
        assert ctx.render_timings()["scene_cached"] == 1
        same_color(oc2, oc, "the cached scene")
        same_depth(od2, RM.depth(d, S, SAMPLE0), "the cached scene, sample 0")
        # depth only: NO_COLOR with color=None
        cn, dn = ctx.render_resolved(v, i, m, w0, h0, DT | NC, factor=S, depth_filter=MIN)
        assert cn is None
        same_depth(dn, RM.depth(d, S, MIN), "NO_COLOR")
        # a .vertices pass resolves
        pc, pd, _, code = oracle.render(v, i, m, w0 * S, h0 * S, oracle.TINV_PER_TRIANGLE, primitive_type=VERTICES)
        assert code == 0
        vc, vd = ctx.render_resolved(v, i, m, w0, h0, 0, primitive_type=VERTICES, factor=S, depth_filter=MIN)
        same_color(vc, RM.color(pc, S), ".vertices")
        same_depth(vd, RM.depth(pd, S, MIN), ".vertices")
        assert (vc[..., 3] > 0).any()
        # factor 1 is swr_render
        small = FM.FrameSpec(v, i, w0, h0, DT, transform=m)
        c1, d1, _ = FM.expect(oracle, small)
        r1 = ctx.render_resolved(v, i, m, w0, h0, DT, factor=1)
        same_color(r1[0], c1, "factor 1")
        same_depth(r1[1], d1, "factor 1")
        # swr_render on the same context still gives its own oracle frame
        rc, rd = ctx.render(v, i, m, w0, h0, DT)
        same_color(rc, c1, "swr_render afterwards")
        same_depth(rd, d1, "swr_render afterwards")
