"""Face culling (SWR_FLAG_CULL_BACK / _CULL_FRONT / _FRONT_CCW; include/swr.h "Face culling").

Expected images come from the unchanged oracle run on the FILTERED scene: oracle.project gives every vertex's screen x / y before any
rounding; the test truncates them (CPU rules) or rounds half away from zero and truncates (Metal rules) as setup_triangle_r does,
computes the signed area A = (bx - ax)(cy - ay) - (cx - ax)(by - ay) in int64, drops the culled triangles from the index list with
their order kept, and renders the rest.  Triangles with a non-finite or out-of-limit vertex stay in the list: both sides skip them.
IDs: the filtered scene is drawn once more colour-coded (the helpers of tests/test_primitive_ids.py, copied) and the decoded
positions are mapped back through the kept-index array, so the GPU's IDs must be the ORIGINAL triangle numbers.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, NC, METAL, REAL_LINES, LOAD, IDS = 1, 2, 4, 8, 16, 32
CB, CF, CCW = 64, 128, 256
NONE = 0xFFFFFFFF
W, H = 640, 360
IDENT = np.eye(4, dtype=np.float32).T.reshape(16)
LIMIT = float(1 << 30)

CULLS = {"back": CB, "front": CF, "both": CB | CF}
WINDINGS = {"cw": 0, "ccw": CCW}
MODES = {"painter": 0, "ztest": DT, "ztest_nc": DT | NC, "metal": METAL, "metal_nc": METAL | NC}


# ---- the filter ------------------------------------------------------------------------------------------------------------------
def integer_vertices(oracle, v, m, w, h, flags):
    """(ix, iy, usable) per vertex: the integer vertices setup_triangle_r rasterises with, and whether setup keeps the vertex."""
    sx, sy, _ = oracle.project(v, m, w, h)
    x, y = sx.astype(np.float64), sy.astype(np.float64)
    if flags & METAL:      # round() half away from zero (exact in float64 for float32 inputs)
        with np.errstate(invalid="ignore"):
            x = np.sign(x) * np.floor(np.abs(x) + 0.5)
            y = np.sign(y) * np.floor(np.abs(y) + 0.5)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(x) < LIMIT) & (np.abs(y) < LIMIT)
        if flags & METAL:
            ok &= (x >= 0) & (y >= 0)
    ix = np.where(ok, np.trunc(np.where(ok, x, 0)), 0).astype(np.int64)
    iy = np.where(ok, np.trunc(np.where(ok, y, 0)), 0).astype(np.int64)
    return ix, iy, ok


def signed_areas(oracle, v, i, m, w, h, flags):
    """A of every triangle (0 where setup skips the triangle anyway)."""
    ix, iy, ok = integer_vertices(oracle, v, m, w, h, flags)
    t = np.asarray(i, dtype=np.int64).reshape(-1, 3)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    area = (ix[b] - ix[a]) * (iy[c] - iy[a]) - (ix[c] - ix[a]) * (iy[b] - iy[a])
    return np.where(ok[a] & ok[b] & ok[c], area, 0)


def kept_triangles(area, flags):
    """Indices of the triangles a frame with these flags draws."""
    front = area < 0 if flags & CCW else area > 0
    back = area > 0 if flags & CCW else area < 0
    drop = ((flags & CB) != 0) & back | ((flags & CF) != 0) & front
    return np.nonzero(~drop)[0]


def filtered(oracle, v, i, m, w, h, flags):
    """(index list of the kept triangles in their order, kept-triangle array)."""
    keep = kept_triangles(signed_areas(oracle, v, i, m, w, h, flags), flags)
    return np.asarray(i, dtype=np.int64).reshape(-1, 3)[keep].reshape(-1), keep


# ---- colour-coded IDs (copied from tests/test_primitive_ids.py) ------------------------------------------------------------------
MASK21 = (1 << 21) - 1
LIVE = -1     # (expected IDs) a pixel some fragment of the frame wins, whichever


def coded(vertices, indices, invert=False):
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


def oracle_frame(oracle, v, i, m, w, h, flags):
    if flags & METAL:
        c, d, _, code = oracle.render_metal(v, i, m, w, h, flags & NC)
    else:
        c, d, _, code = oracle.render(v, i, m, w, h, (flags & (DT | NC)) | oracle.TINV_PER_TRIANGLE)
    assert code == 0
    return c, d


def expected(oracle, v, i, m, w, h, flags, ids=False):
    """(colour or None, depth, IDs in the original numbering or None, kept triangles) of one clear frame with these flags."""
    fi, keep = filtered(oracle, v, i, m, w, h, flags)
    c, d = oracle_frame(oracle, v, fi, m, w, h, flags)
    rid = None
    if ids:
        dec = []
        for inv in (False, True):
            cv, ci = coded(v, fi, inv)
            cc, cd = oracle_frame(oracle, cv, ci, m, w, h, flags & ~NC)
            assert cd.tobytes() == d.tobytes()
            dec.append(decode(cc, inv))
        pos = np.where(dec[0] == dec[1], dec[0].astype(np.int64), LIVE)      # position in the filtered list
        rid = pos.copy()
        hit = (pos >= 0) & (pos != NONE)
        rid[hit] = keep[pos[hit]]
        if flags & (DT | METAL):
            assert (rid != LIVE).all()
    return (None if flags & NC else c), d, rid, keep


def same(ctx, flags, want, what=""):
    rc, rd, rid = want[:3]
    ctx.sync()
    d = ctx.read_depth()
    bad = np.nonzero(d.view(np.uint32) != rd.view(np.uint32))
    assert bad[0].size == 0, f"{what}: {bad[0].size} depth values differ"
    if rc is not None and not (flags & NC):
        c = ctx.read_color()
        bad = np.nonzero((c != rc).any(axis=-1))
        assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"
    if rid is not None:
        ids = ctx.read_ids()
        assert (ids[rid == LIVE] != NONE).all(), what
        bad = np.nonzero((ids != rid) & (rid >= 0))
        assert bad[0].size == 0, f"{what}: {bad[0].size} IDs differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): {ids[bad][0]} vs {rid[bad][0]}"
        return ids
    return None


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def soup(swr, ntri=3000, seed=0xC011, w=W, h=H, r_ndc=0.12):
    """Random triangles: about half of each winding."""
    return swr.scenes.random_soup(ntri, w, h, seed, r_ndc=r_ndc, margin=1.1)


def torus(swr):
    S = swr.scenes
    xyz, rgb, idx = S.torus_mesh(48, 24, 0.6, 0.25)
    return S.pack_vertices(xyz, rgb), np.asarray(idx, dtype=np.int64).reshape(-1)


def scene(swr, name):
    S = swr.scenes
    if name == "soup":
        s = soup(swr)
        return s.vertices, s.indices, S.app_transform(0.7, scale=1.3)
    if name == "degenerate":
        s = S.degenerate_mix(W, H)
        return s.vertices, s.indices, s.transform
    v, i = torus(swr)
    return v, i, S.app_transform(0.4, scale=1.6)


def mirrored(m, screen=False):
    """A mirroring matrix (det < 0): m after a mirror of the model's x, or (screen) followed by a mirror of the clip-space x, which
    mirrors the image: every triangle's winding as displayed flips."""
    c = np.array(np.asarray(m, dtype=np.float32).reshape(4, 4), copy=True)     # c[j] = column j
    if screen:
        c[:, 0] = -c[:, 0]
    else:
        c[0] = -c[0]
    return c.reshape(16)


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


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_the_filter_sees_both_windings(swr, oracle):
    """(the scenes exercise what they are meant to: both signs of A, and A == 0 triangles in degenerate_mix)"""
    for name in ("soup", "degenerate", "torus"):
        v, i, m = scene(swr, name)
        for flags in (0, METAL):
            a = signed_areas(oracle, v, i, m, W, H, flags)
            assert (a > 0).sum() > 20 and (a < 0).sum() > 20, (name, flags)
    v, i, m = scene(swr, "degenerate")
    assert (signed_areas(oracle, v, i, m, W, H, 0) == 0).sum() >= 30


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("winding", list(WINDINGS))
@pytest.mark.parametrize("cull", list(CULLS))
def test_every_mode_and_winding(swr, oracle, cull, winding, mode):
    flags = MODES[mode] | CULLS[cull] | WINDINGS[winding]
    with swr.Context(0) as ctx:
        ctx.target_set(W, H)
        for name in ("soup", "degenerate", "torus"):
            v, i, m = scene(swr, name)
            want = expected(oracle, v, i, m, W, H, flags)
            keep = want[3]
            assert keep.size < i.size // 3, f"{name}: nothing culled"
            ctx.scene_upload(v, i)
            ctx.draw(m, flags)
            same(ctx, flags, want, f"{name}, {cull}, {winding}, {mode}")


@pytest.mark.parametrize("mode", ["painter", "ztest"])
def test_degenerate_triangles_are_never_culled(swr, oracle, mode):
    """Under the CPU rules, A == 0 triangles (collinear after truncation) keep drawing with both cull bits set."""
    S = swr.scenes
    s = S.degenerate_mix(W, H)
    flags = MODES[mode] | CB | CF
    area = signed_areas(oracle, s.vertices, s.indices, s.transform, W, H, flags)
    want = expected(oracle, s.vertices, s.indices, s.transform, W, H, flags)
    assert np.array_equal(want[3], np.nonzero(area == 0)[0]) and want[3].size >= 30
    if mode == "painter":     # (under the z-test their NaN depths keep most of them out)
        clear_c, _ = oracle_frame(oracle, s.vertices, np.zeros(0, np.int64), s.transform, W, H, flags)
        assert not np.array_equal(want[0], clear_c), "the A == 0 triangles draw nothing: the test shows nothing"
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        ctx.draw(s.transform, flags)
        same(ctx, flags, want, f"degenerate_mix, both bits, {mode}")


def test_worked_example(swr, oracle):
    """NDC (-0.5,-0.5), (0.5,-0.5), (0,0.5): counter-clockwise as displayed, A = -W*H/4."""
    v = swr.scenes.pack_vertices(np.array([[-0.5, -0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.5, 0.5]], np.float32),
                                 np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32))
    i = np.arange(3, dtype=np.int64)
    ix, iy, _ = integer_vertices(oracle, v, IDENT, W, H, 0)
    assert ix.tolist() == [W // 4, 3 * W // 4, W // 2] and iy.tolist() == [3 * H // 4, 3 * H // 4, H // 4]
    assert signed_areas(oracle, v, i, IDENT, W, H, 0).tolist() == [-W * H // 4]
    drawn = oracle_frame(oracle, v, i, IDENT, W, H, DT)
    cleared = oracle_frame(oracle, v, i[:0], IDENT, W, H, DT)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        for flags, want in ((DT | CB, cleared), (DT | CB | CCW, drawn), (DT | CF, drawn), (DT | CF | CCW, cleared),
                            (DT | CB | CF, cleared), (DT, drawn)):
            ctx.draw(IDENT, flags)
            same(ctx, flags, (want[0], want[1], None), f"flags {flags}")
    assert not np.array_equal(drawn[0], cleared[0])


@pytest.mark.parametrize("setting", [("bin", 1), ("bin", 3), ("order", 0), ("order", -1)])
def test_debug_bin_modes_and_stream_orders(swr, oracle, setting):
    b = swr.binding
    key = b.DEBUG_BIN_MODE if setting[0] == "bin" else b.DEBUG_STREAM_ORDER
    v, i, m = scene(swr, "soup")
    vt, it, mt = scene(swr, "torus")
    with swr.Context(0) as ctx:
        ctx.debug_set(key, setting[1])
        ctx.target_set(W, H)
        for vv, ii, mm in ((v, i, m), (vt, it, mt)):
            ctx.scene_upload(vv, ii)
            for flags in (DT | CB, METAL | CF | CCW, NC | DT | CB | CCW, CB | CF):
                ctx.draw(mm, flags)
                same(ctx, flags, expected(oracle, vv, ii, mm, W, H, flags), f"{setting}, flags {flags}")


def test_scene_above_2_20_triangles(swr, oracle):
    s = swr.scenes.random_soup((1 << 20) + 3000, 480, 270, 0xC0B16, r_ndc=0.01, margin=1.1)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(480, 270)
        for flags in (DT | CB | IDS, METAL | CF):
            want = expected(oracle, s.vertices, s.indices, s.transform, 480, 270, flags, ids=bool(flags & IDS))
            ctx.draw(s.transform, flags)
            ids = same(ctx, flags, want, f"2^20 + 3000 triangles, flags {flags}")
            if ids is not None:
                assert (ids[ids != NONE] >= (1 << 20)).any()


@pytest.mark.parametrize("flags", [DT, DT | NC, 0, METAL])
def test_draw_list_with_a_mirrored_item(swr, oracle, flags):
    """Each item's facing comes from its own transform; the mirrored item's winding flips (no compensation).  Expected: the clear
    frame of the pre-transformed concatenation, filtered, IDs mapped back to the list's order numbers."""
    S = swr.scenes
    s = soup(swr, 2400, seed=0xD1)
    base = S.app_transform(0.6, scale=1.3)
    items = [(0, 2400, base), (2400, 2400, mirrored(S.app_transform(0.9, scale=1.1))), (4800, 2400, S.app_transform(1.7)),
             (600, 1200, mirrored(base, screen=True))]
    v, i = concat(s.vertices, s.indices, items)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        for cull in (CB, CF | CCW, CB | CF):
            fl = flags | cull | (IDS if not flags & NC else 0)
            want = expected(oracle, v, i, IDENT, W, H, fl, ids=bool(fl & IDS))
            ctx.draw_list(items, fl)
            same(ctx, fl, want, f"draw list, flags {fl}")
    # item 3 is item 0's triangles 200..599 in the mirrored image: (nearly) every one of them has the other winding
    a = signed_areas(oracle, v, i, IDENT, W, H, flags)
    a0, a3 = a[200:600], a[2400:2800]
    both = (a0 != 0) & (a3 != 0)
    assert both.sum() > 300 and (np.sign(a0[both]) == -np.sign(a3[both])).mean() > 0.95


@pytest.mark.parametrize("flags", [DT, 0, METAL | NC])
def test_load_chain_whose_middle_frame_culls(swr, oracle, flags):
    """A (clear), B (load, CULL_BACK), C (load): the clear frame of A || filtered B || C, each pre-transformed."""
    S = swr.scenes
    parts = [(soup(swr, 1200, seed=0xA), S.app_transform(0.2, scale=1.2)), (soup(swr, 1200, seed=0xB), S.app_transform(1.1, scale=1.4)),
             (soup(swr, 1200, seed=0xC), S.app_transform(2.1, scale=1.1))]
    vs, ix, base = [], [], 0
    for k, (p, m) in enumerate(parts):
        pv = pretransform(p.vertices, m)
        pi = p.indices
        if k == 1:
            pi, keep = filtered(oracle, pv, pi, IDENT, W, H, flags | CB)
            assert 0 < keep.size < p.indices.size // 3
        vs.append(pv)
        ix.append(pi + base)
        base += pv.shape[0]
    rc, rd = oracle_frame(oracle, np.concatenate(vs), np.concatenate(ix), IDENT, W, H, flags)
    with swr.Context(0) as ctx:
        ctx.target_set(W, H)
        for k, (p, m) in enumerate(parts):
            ctx.scene_upload(p.vertices, p.indices)
            ctx.draw(m, flags | (LOAD if k else 0) | (CB if k == 1 else 0))
        same(ctx, flags, ((None if flags & NC else rc), rd, None), f"load chain, flags {flags}")


@pytest.mark.parametrize("mode", ["painter", "ztest", "ztest_nc", "metal"])
@pytest.mark.parametrize("name", ["soup", "torus"])
def test_primitive_ids_keep_the_original_numbering(swr, oracle, mode, name):
    v, i, m = scene(swr, name)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        for cull in (CB, CF | CCW):
            flags = MODES[mode] | cull | IDS
            want = expected(oracle, v, i, m, W, H, flags, ids=True)
            ctx.draw(m, flags)
            ids = same(ctx, flags, want, f"{name}, {mode}, cull {cull}")
            live = ids[ids != NONE].astype(np.int64)
            assert live.size > 1000 and np.isin(live, want[3]).all()
            # positions among the survivors would differ from the original numbers somewhere
            assert (live != np.searchsorted(want[3], live)).any()


@pytest.mark.parametrize("flags", [DT, DT | NC, 0, METAL])
def test_render_one_shot_and_cached(swr, oracle, flags):
    s = soup(swr, 2000, seed=0x4E)
    t, ti, tm = scene(swr, "torus")
    with swr.Context(0) as ctx:
        ctx.debug_set(swr.binding.DEBUG_ONESHOT_MIN_TRIS, 64)         # (the one-shot stream built chunk by chunk, in index order)
        for v, i, m, sid in ((s.vertices, s.indices, s.transform, 0), (t, ti, tm, 0), (t, ti, tm, 7), (t, ti, tm, 7)):
            for cull in (CB, CF | CCW):
                rc, rd, _, _ = expected(oracle, v, i, m, W, H, flags | cull)
                c, d = ctx.render(v, i, m, W, H, flags | cull, scene_id=sid)
                assert d.tobytes() == rd.tobytes(), f"scene_id {sid}, flags {flags | cull}: depth"
                if not flags & NC:
                    assert np.array_equal(c, rc), f"scene_id {sid}, flags {flags | cull}: colour"
        assert ctx.render_timings()["scene_cached"] == 1


def test_four_bands_at_4k(swr, oracle):
    s = swr.scenes.cfg4_soup(200_000)
    with swr.Context(0, device_count=4) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(s.width, s.height)
        for flags in (DT | NC | CB, DT | CF | CCW | IDS, METAL | NC | CB):
            want = expected(oracle, s.vertices, s.indices, s.transform, s.width, s.height, flags, ids=bool(flags & IDS))
            ctx.draw(s.transform, flags)
            same(ctx, flags, want, f"4 bands, flags {flags}")


_OVERFLOW_WANT = {}


@pytest.mark.parametrize("lanes", ["lanes", "two-stream"])
@pytest.mark.parametrize("bins", ["fixed", "exact"])
def test_overflowed_first_frame_is_redrawn_with_its_cull_bits(swr, oracle, monkeypatch, bins, lanes):
    S = swr.scenes
    if lanes == "two-stream":
        monkeypatch.setenv("SWR_LANES", "0")
    w, h = 1280, 720
    if bins == "exact":
        s = S.random_soup(1000, w, h, 78, r_ndc=1.4, flags=DT, margin=0.3)
    else:
        s = S.random_soup(20000, w, h, 555, r_ndc=0.01, flags=DT, margin=1.0)
        v = s.vertices.copy()
        v[:, 0] = 0.30 + (v[:, 0] * 0.5 + 0.5) * 0.07
        v[:, 1] = 0.10 + (v[:, 1] * 0.5 + 0.5) * 0.06
        s.vertices = np.ascontiguousarray(v)
    flags = DT | CB | IDS
    if bins not in _OVERFLOW_WANT:
        _OVERFLOW_WANT[bins] = expected(oracle, s.vertices, s.indices, s.transform, w, h, flags, ids=True)
    want = _OVERFLOW_WANT[bins]
    ntri = s.indices.size // 3
    with swr.Context(0) as ctx:
        if bins == "exact":
            ctx.debug_set(swr.binding.DEBUG_BIN_MODE, swr.binding.BIN_MODE_EXACT)
        ctx.target_set(w, h)
        ctx.scene_upload(s.vertices, s.indices)
        ctx.draw(s.transform, flags)              # a fresh context: its bins overflow, the frame is redrawn with its flags
        same(ctx, flags, want, f"overflowed first frame ({bins} bins, {lanes})")
        pairs = ctx.timings()["tile_pairs"]
    # (the culled frame alone still needs more than the first capacity: 2 ntri + 65536 pairs, or 1024 per fixed tile region)
    assert pairs > (2 * ntri + 65536 if bins == "exact" else 4 * 1024), pairs


def test_unwaited_burst_alternating_cull_and_no_cull(swr, oracle):
    S = swr.scenes
    s = soup(swr, 2000, seed=0xB0)
    ms = [S.app_transform(0.17 * k, scale=1.0 + 0.05 * k) for k in range(9)]
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        for last in (8, 7):
            for k, m in enumerate(ms[:last + 1]):
                ctx.draw(m, DT | (CB if k % 2 == 0 else 0))
            fl = DT | (CB if last % 2 == 0 else 0)
            same(ctx, fl, expected(oracle, s.vertices, s.indices, ms[last], W, H, fl), f"last of a burst ({last})")
        for k, m in enumerate(ms[:4]):
            ctx.draw(m, DT | NC | (CF | CCW if k % 2 else 0))
        fl = DT | NC | CF | CCW
        same(ctx, fl, expected(oracle, s.vertices, s.indices, ms[3], W, H, fl), "last of a depth-only burst")


@pytest.mark.parametrize("prim", [1, 2])
def test_vertices_and_lines_ignore_the_bits(swr, prim):
    S = swr.scenes
    s = soup(swr, 1500, seed=0x11)
    m = S.app_transform(0.5, scale=1.2)
    extra = REAL_LINES if prim == 1 else 0
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices[: s.indices.size // 6 * 6])
        ctx.target_set(W, H)
        ctx.draw(m, DT | extra, primitive_type=prim)
        ctx.sync()
        c0, d0 = ctx.read_color(), ctx.read_depth()
        assert (c0 != c0[0, 0]).any()
        for bits in (CB, CF, CB | CF, CB | CCW, CF | CB | CCW):
            ctx.draw(m, DT | extra | bits, primitive_type=prim)
            ctx.sync()
            assert np.array_equal(ctx.read_color(), c0), bits
            assert ctx.read_depth().tobytes() == d0.tobytes(), bits


def test_tile_pairs(swr, oracle):
    s = soup(swr)
    m = swr.scenes.app_transform(0.7, scale=1.3)
    area = signed_areas(oracle, s.vertices, s.indices, m, W, H, 0)
    s.indices = np.ascontiguousarray(s.indices.reshape(-1, 3)[area != 0].reshape(-1))     # no triangle without a facing
    with swr.Context(0) as ctx:
        ctx.timing_enable(2)
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        ctx.draw(m, DT)
        ctx.sync()
        full = ctx.timings()
        ctx.draw(m, DT | CB)
        ctx.sync()
        back = ctx.timings()
        assert back["triangles"] == full["triangles"] == s.indices.size // 3
        assert 0 < back["tile_pairs"] < full["tile_pairs"]
        ctx.draw(m, DT | CB | CF)
        ctx.sync()
        none = ctx.timings()
        assert none["tile_pairs"] == 0 and none["triangles"] == s.indices.size // 3
        rc, rd = oracle_frame(oracle, s.vertices, s.indices[:0], m, W, H, DT)
        same(ctx, DT, (rc, rd, None), "every triangle culled: the cleared image")


def test_bad_flag_bits_still_refused(swr):
    s = soup(swr, 100, seed=0x12)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(W, H)
        ctx.draw(s.transform, DT | CB | CF | CCW)
        for bad in (1 << 9, CB | (1 << 9)):
            with pytest.raises(swr.SwrError) as e:
                ctx.draw(s.transform, DT | bad)
            assert e.value.code == -1
