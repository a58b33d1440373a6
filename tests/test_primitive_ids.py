"""Primitive IDs (SWR_FLAG_PRIMITIVE_IDS, swr_read_ids; include/swr.h): which triangle is visible at every pixel.

Expected IDs come from the unchanged oracle.  A de-indexed copy of the scene gives every vertex of triangle t the flat colour
(2 d_c + 1) / 255 per channel, d_c the c-th 7-bit digit of t (red: bits 0-6, green: 7-13, blue: 14-20); the oracle's colour image
of that copy, decoded as byte >> 1 per channel, is the winner's index (alpha 0: nothing kept there, SWR_ID_NONE).  Vertex transforms
are per vertex, so the copy has exactly the original geometry and the same winners.  The decode has a margin of one byte: the
colour of a pixel is c * w0 + c * w1 + c * w2 with weights inside [0, 1] that sum to 1 up to a few float32 ulps, so 255 times it is
2 d_c + 1 up to ~1e-4 — the truncating CPU-rules quantiser gives 2 d_c + 1 or 2 d_c, the rounding Metal store 2 d_c + 1, and both
decode to d_c.  (The extended fragment stage does not change which fragment wins; its frames take the IDs of the passthrough copy.)
One exception: under painter's order a sliver triangle whose weights are not finite at a pixel still wins it, with a colour of 0
whatever its code.  So the copy is drawn twice, the second time with every digit inverted (127 - d_c); a pixel whose two decodes
disagree is such a pixel, and there the GPU's ID only has to be live (under the z-test those fragments have a NaN depth and are
never kept, so both decodes give SWR_ID_NONE).
The same oracle supplies the colour and depth of every frame, so the flag is also shown not to change them.
"""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, NC, METAL, LOAD, IDS = 1, 2, 4, 16, 32
NONE = 0xFFFFFFFF
W, H = 640, 360
IDENT = np.eye(4, dtype=np.float32).T.reshape(16)


MASK21 = (1 << 21) - 1


def coded(vertices, indices, invert=False):
    """The de-indexed copy of a scene, every triangle in its colour code (invert: every digit inverted)."""
    i = np.asarray(indices, dtype=np.int64).reshape(-1)
    v = np.array(np.asarray(vertices, dtype=np.float32).reshape(-1, 8)[i], copy=True)
    t = np.repeat(np.arange(i.size // 3, dtype=np.int64), 3)
    if invert:
        t = t ^ MASK21
    for ch in range(3):
        v[:, 4 + ch] = ((2 * ((t >> (7 * ch)) & 127) + 1) / 255.0).astype(np.float32)
    return v, np.arange(i.size, dtype=np.int64)


def decode(c, invert=False):
    ids = (c[..., 2].astype(np.int64) >> 1) | ((c[..., 1].astype(np.int64) >> 1) << 7) | ((c[..., 0].astype(np.int64) >> 1) << 14)
    if invert:
        ids = ids ^ MASK21
    ids = ids.astype(np.uint32)
    ids[c[..., 3] == 0] = NONE
    assert np.isin(c[..., 3], (0, 255)).all()
    return ids


def oracle_frame(oracle, v, i, m, w, h, flags, shading=None):
    if flags & METAL:
        c, d, _, code = oracle.render_metal(v, i, m, w, h, flags & NC, shading=shading)
    else:
        c, d, _, code = oracle.render(v, i, m, w, h, (flags & (DT | NC)) | oracle.TINV_PER_TRIANGLE, shading=shading)
    assert code == 0
    return c, d


def expected(oracle, v, i, m, w, h, flags, shading=None):
    """(colour or None, depth, IDs) of one clear frame; IDs of pixels won by a fragment without a finite colour are LIVE."""
    c, d = oracle_frame(oracle, v, i, m, w, h, flags, shading)
    ids = []
    for inv in (False, True):
        cv, ci = coded(v, i, inv)
        cc, cd = oracle_frame(oracle, cv, ci, m, w, h, flags & ~NC)
        assert cd.tobytes() == d.tobytes()
        ids.append(decode(cc, inv))
    rid = np.where(ids[0] == ids[1], ids[0].astype(np.int64), LIVE)
    if flags & (DT | METAL):
        assert (rid != LIVE).all()
    return (None if flags & NC else c), d, rid


LIVE = -1     # (expected IDs) a pixel some fragment of the frame wins, whichever
ANY = -2      # (expected IDs) not checked


def same(ctx, flags, want, what=""):
    rc, rd, rid = want
    ctx.sync()
    ids = ctx.read_ids()
    d = ctx.read_depth()
    assert ((ids[rid == LIVE]) != NONE).all(), what
    bad = np.nonzero((ids != rid) & (rid >= 0))
    assert bad[0].size == 0, f"{what}: {bad[0].size} IDs differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): {ids[bad][0]} vs {rid[bad][0]}"
    bad = np.nonzero(d.view(np.uint32) != rd.view(np.uint32))
    assert bad[0].size == 0, f"{what}: {bad[0].size} depth values differ"
    if rc is not None:
        c = ctx.read_color()
        bad = np.nonzero((c != rc).any(axis=-1))
        assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ"
    return ids


def pretransform(vertices, m):
    """Vertex.apply in float32 without FMA (the composition identity of DESIGN.md §11 / §12)."""
    v = np.array(vertices, dtype=np.float32, copy=True).reshape(-1, 8)
    c = np.asarray(m, dtype=np.float32).reshape(4, 4)
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    r = c[0][None, :] * x
    r = r + c[1][None, :] * y
    r = r + c[2][None, :] * z
    r = r + c[3][None, :]
    v[:, 0:3] = r[:, 0:3] / r[:, 3:4]
    return v


def concat(vertices, indices, items):
    vs, ix, base = [], [], 0
    for first, count, m in items:
        vs.append(pretransform(vertices, m))
        ix.append(np.asarray(indices[first:first + count], dtype=np.int64) + base)
        base += vertices.shape[0]
    return np.concatenate(vs), np.concatenate(ix)


def soup(swr, ntri=3000, seed=0x1D5, w=W, h=H, r_ndc=0.12):
    return swr.scenes.random_soup(ntri, w, h, seed, r_ndc=r_ndc, margin=1.1)


def mesh(swr):
    S = swr.scenes
    xyz, rgb, idx = S.torus_mesh(48, 24, 0.6, 0.25)
    return S.pack_vertices(xyz, rgb), np.asarray(idx, dtype=np.int64).reshape(-1)


MODES = {"painter": 0, "ztest": DT, "depth_only": DT | NC, "painter_depth_only": NC, "metal": METAL, "metal_depth_only": METAL | NC}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("scene", ["soup", "mesh"])
def test_ids_of_one_frame(swr, oracle, mode, scene):
    flags = MODES[mode]
    if scene == "soup":
        s = soup(swr)
        v, i, m = s.vertices, s.indices, swr.scenes.app_transform(0.7, scale=1.3)
    else:
        v, i = mesh(swr)
        m = swr.scenes.app_transform(0.4, scale=1.6)
    want = expected(oracle, v, i, m, W, H, flags)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw(m, flags | IDS)
        ids = same(ctx, flags, want, f"{scene}, {mode}")
    assert (ids != NONE).sum() > 1000


@pytest.mark.parametrize("shader", [1, 2])
def test_ids_with_the_extended_fragment_stage(swr, oracle, shader):
    S = swr.scenes
    s = soup(swr, 2500, seed=0x5A)
    sh = S.random_shading(s.vertices.shape[0], 0x5A, shader)
    m = S.app_transform(0.3, scale=1.2)
    for flags in (DT, 0):
        want = expected(oracle, s.vertices, s.indices, m, W, H, flags, shading=sh)
        with swr.Context(0) as ctx:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.shading_set(sh)
            ctx.target_set(W, H)
            ctx.draw(m, flags | IDS)
            same(ctx, flags, want, f"shader {shader}, flags {flags}")


def test_scene_above_2_20_triangles(swr, oracle):
    """The PLAIN kernels (no winner table): IDs above 2^20 need the 21 bits of the code."""
    s = swr.scenes.random_soup((1 << 20) + 3000, 480, 270, 0xB16, r_ndc=0.01, margin=1.1)
    for flags in (DT, DT | NC, 0, METAL):
        want = expected(oracle, s.vertices, s.indices, s.transform, 480, 270, flags)
        with swr.Context(0) as ctx:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(480, 270)
            ctx.draw(s.transform, flags | IDS)
            ids = same(ctx, flags, want, f"2^20 + 3000 triangles, flags {flags}")
        assert (ids[ids != NONE] >= (1 << 20)).any()


def test_cfg4_full_size(swr, oracle):
    s = swr.scenes.cfg4_soup()
    for flags in (DT | NC, DT):
        want = expected(oracle, s.vertices, s.indices, s.transform, s.width, s.height, flags)
        with swr.Context(0) as ctx:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(s.width, s.height)
            ctx.draw(s.transform, flags)             # a frame without the flag first: the 32-bit keys
            ctx.draw(s.transform, flags | IDS)
            same(ctx, flags, want, f"cfg4, flags {flags}")


def test_special_depths_and_the_slow_resolve(swr, oracle):
    """Depth-only z-tested frames whose winners have +-0 (the resolve's slow path), and fragments with NaN / +inf depths (never
    kept: SWR_ID_NONE unless another fragment wins there)."""
    s = soup(swr, 3000, seed=0x2E0)
    v = s.vertices.copy()
    v[0::7, 2] = 0.0
    v[1::11, 2] = -0.0
    v[2::13, 2] = np.nan
    v[3::17, 2] = np.inf
    for flags in (DT | NC, DT, METAL | NC):
        want = expected(oracle, v, s.indices, s.transform, W, H, flags)
        with swr.Context(0) as ctx:
            ctx.scene_upload(v, s.indices)
            ctx.target_set(W, H)
            ctx.draw(s.transform, flags | IDS)
            same(ctx, flags, want, f"special depths, flags {flags}")


@pytest.mark.parametrize("flags", [DT | NC, DT, 0, METAL])
def test_load_chain_ids_of_the_last_frame(swr, oracle, flags):
    """A, then B as a load frame with IDs: B's triangle where B wins, SWR_ID_NONE where the loaded image is kept (the expected values
    from the clear frame of A || B, pre-transformed)."""
    S = swr.scenes
    a, b = soup(swr, 1500, seed=0xA), soup(swr, 1500, seed=0xB)
    m_a, m_b = S.app_transform(0.2, scale=1.2), S.app_transform(1.1, scale=1.4)
    v = np.concatenate([pretransform(a.vertices, m_a), pretransform(b.vertices, m_b)])
    i = np.concatenate([a.indices, b.indices + a.vertices.shape[0]])
    rc, rd, rid = expected(oracle, v, i, IDENT, W, H, flags)
    na = a.indices.size // 3
    # (painter's order: a pixel won by a fragment without a finite colour may be A's or B's — not checked)
    rid = np.where(rid == LIVE, ANY, np.where((rid != NONE) & (rid >= na), rid - na, NONE))
    with swr.Context(0) as ctx:
        ctx.target_set(W, H)
        ctx.scene_upload(a.vertices, a.indices)
        ctx.draw(m_a, flags | IDS)
        ctx.scene_upload(b.vertices, b.indices)
        ctx.draw(m_b, flags | LOAD | IDS)
        ids = same(ctx, flags, (rc, rd, rid), f"load chain, flags {flags}")
    assert (ids == NONE).sum() > 0 and (ids != NONE).sum() > 0


def check_list(swr, oracle, ctx, v0, i0, items, flags, what):
    v, i = concat(v0, i0, items)
    want = expected(oracle, v, i, IDENT, W, H, flags)
    ctx.draw_list(items, flags | IDS)
    ids = same(ctx, flags, want, what)
    k, j = swr.binding.list_ids_to_items(ids, items)
    live = ids != NONE
    counts = [c // 3 for _, c, _ in items]
    vbase = np.concatenate([[0], np.cumsum(counts)[:-1]])
    assert (k[live] >= 0).all() and (vbase[k[live]] + j[live] == ids[live]).all()
    assert (j[live] < np.asarray(counts)[k[live]]).all()
    return k, j


@pytest.mark.parametrize("flags", [DT | NC, DT, 0, METAL])
def test_draw_lists(swr, oracle, flags):
    S = swr.scenes
    s = soup(swr, 2400, seed=0xD1)
    n = s.indices.size
    m = S.app_transform(0.6, scale=1.3)
    identity_layout = [(0, 1200, m), (1200, 2400, m), (3600, n - 3600, m)]
    objects = [(3 * 300 * k, 3 * 300, S.app_transform(0.3 * k, scale=0.8 + 0.1 * k)) for k in range(8)]
    instanced = [(600, 3000, m), (0, 1800, S.app_transform(1.0, scale=1.1)), (600, 3000, S.app_transform(2.0, scale=0.9)),
                 (1500, 2100, m)]
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        check_list(swr, oracle, ctx, s.vertices, s.indices, identity_layout, flags, "identity layout")
        k, _ = check_list(swr, oracle, ctx, s.vertices, s.indices, objects, flags, "8 objects")
        assert len(set(k[k >= 0].tolist())) >= 4
        check_list(swr, oracle, ctx, s.vertices, s.indices, instanced, flags, "instanced, overlapping ranges")


def test_unwaited_burst_alternating_the_flag(swr, oracle):
    S = swr.scenes
    s = soup(swr, 2000, seed=0xB0)
    ms = [S.app_transform(0.17 * k, scale=1.0 + 0.05 * k) for k in range(9)]
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        for k, m in enumerate(ms):
            ctx.draw(m, DT | (IDS if k % 2 == 0 else 0))
        same(ctx, DT, expected(oracle, s.vertices, s.indices, ms[-1], W, H, DT), "last of a burst")
        for k, m in enumerate(ms[:4]):
            ctx.draw(m, DT | NC | (IDS if k % 2 else 0))
        same(ctx, DT | NC, expected(oracle, s.vertices, s.indices, ms[3], W, H, DT | NC), "last of a depth-only burst")


@pytest.mark.parametrize("bins", ["fixed", "exact"])
def test_bin_overflow_of_the_last_frame(swr, oracle, bins):
    S = swr.scenes
    w, h = 1280, 720
    if bins == "exact":
        s = S.random_soup(220, w, h, 77, r_ndc=1.4, flags=DT, margin=0.3)
    else:
        s = S.random_soup(20000, w, h, 555, r_ndc=0.01, flags=DT, margin=1.0)
        v = s.vertices.copy()
        v[:, 0] = 0.30 + (v[:, 0] * 0.5 + 0.5) * 0.07
        v[:, 1] = 0.10 + (v[:, 1] * 0.5 + 0.5) * 0.06
        s.vertices = np.ascontiguousarray(v)
    want = expected(oracle, s.vertices, s.indices, s.transform, w, h, DT)
    with swr.Context(0) as ctx:
        if bins == "exact":
            ctx.debug_set(swr.binding.DEBUG_BIN_MODE, swr.binding.BIN_MODE_EXACT)
        ctx.target_set(w, h)
        ctx.scene_upload(s.vertices, s.indices)
        ctx.draw(s.transform, DT | IDS)           # a fresh context: its bins overflow, the frame is redrawn with its flags
        same(ctx, DT, want, f"overflowed last frame ({bins} bins)")


def test_eight_bands_at_4k(swr, oracle):
    s = swr.scenes.cfg4_soup(200_000)
    for flags in (DT | NC, DT):
        want = expected(oracle, s.vertices, s.indices, s.transform, s.width, s.height, flags)
        with swr.Context(0, device_count=8) as ctx:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(s.width, s.height)
            ctx.draw(s.transform, flags | IDS)
            same(ctx, flags, want, f"8 bands, flags {flags}")


@pytest.mark.parametrize("flags", [DT, DT | NC, METAL])
def test_render_with_the_flag(swr, oracle, flags):
    s = soup(swr, 2000, seed=0x4E)
    rc, rd, rid = expected(oracle, s.vertices, s.indices, s.transform, W, H, flags)
    with swr.Context(0) as ctx:
        c, d = ctx.render(s.vertices, s.indices, s.transform, W, H, flags | IDS)
        assert d.tobytes() == rd.tobytes() and (rc is None or np.array_equal(c, rc))
        assert np.array_equal(ctx.read_ids(), rid.astype(np.uint32))


def test_frames_without_the_flag_are_unchanged(swr, oracle):
    """After ID frames a frame without the flag gives the same colour and depth as ever (depth-only: on the 32-bit depth keys,
    which the ID frames leave alone), and its IDs cannot be read."""
    s = swr.scenes.cfg4_soup(200_000)
    for flags in (DT | NC, DT):
        rc, rd, _ = expected(oracle, s.vertices, s.indices, s.transform, s.width, s.height, flags)
        with swr.Context(0) as ctx:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(s.width, s.height)
            for _ in range(3):
                ctx.draw(s.transform, flags | IDS)
            ctx.draw(s.transform, flags)
            ctx.sync()
            assert ctx.read_depth().tobytes() == rd.tobytes()
            if rc is not None:
                assert np.array_equal(ctx.read_color(), rc)
            with pytest.raises(swr.SwrError) as e:
                ctx.read_ids()
            assert e.value.code == -1


def test_errors(swr):
    s = soup(swr, 500, seed=0xE)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        for what in ("before any ID frame", "after a frame without the flag", "after swr_target_set", "after swr_target_write"):
            if what == "after a frame without the flag":
                ctx.draw(s.transform, DT | IDS)
                ctx.draw(s.transform, DT)
            elif what == "after swr_target_set":
                ctx.draw(s.transform, DT | IDS)
                ctx.sync()
                assert (ctx.read_ids() != NONE).any()
                ctx.target_set(W, H)
            elif what == "after swr_target_write":
                ctx.draw(s.transform, DT | IDS)
                ctx.target_write(None, np.zeros((H, W), np.float32))
            with pytest.raises(swr.SwrError) as e:
                ctx.read_ids()
            assert e.value.code == -1, what
        for prim in (1, 2):                          # .line, .vertices
            with pytest.raises(swr.SwrError) as e:
                ctx.draw(s.transform, IDS, primitive_type=prim)
            assert e.value.code == -5
    with swr.Context(0, device_count=2) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        with pytest.raises(swr.SwrError) as e:
            ctx.draw(s.transform, IDS, primitive_type=2)
        assert e.value.code == -5
