"""The second trip of every capped grid and grid-stride loop (tests/grid_caps.py is the inventory; tests/test_grid_caps_table.py keeps
it honest).  Each case takes its size from grid_caps.SHAPES — the smallest that crosses the cap with the last workgroup partly filled —
compares bit for bit with a model, the oracle or a context that uploaded the model's result, and first asserts on the CPU, from the
model alone, that what lies beyond the first trip is observable.  One band everywhere: the caps are per band."""
import dataclasses
import os
import re

import numpy as np
import pytest

import grid_caps as G
import item_bounds_model as IBM
import kernel_matrix as K
import skin_dq_model as DQ
import skin_model as SM
import test_depth_clip as TDC
import test_skin_dq as TDQ

gpu = pytest.mark.gpu
DT, NC, METAL, LOAD, IDS = K.DT, K.NC, K.METAL, K.LOAD, K.IDS
REAL_LINES, CLIP = 8, 1024
TRI, LINE, VERTICES = 0, 1, 2
IDENT = K.IDENT
INDEX_RANGE = -3
DEBUG_STREAM_ORDER = 1
FIRST_TRIP = 4096 * 256


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(a.shape[0], a.shape[1])


def frame(ctx, flags, prim=TRI, m=IDENT):
    ctx.draw(m, flags, prim)
    ctx.sync()
    return ctx.read_color(), ctx.read_depth()


def same_frames(got, want, what):
    for g, w, name in zip(got, want, ("colour", "depth")):
        bad = np.nonzero(words(g) != words(w))
        assert bad[0].size == 0, f"{what}: {bad[0].size} {name} pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"


def quantised(rgb):
    """The byte a colour channel in [0, 1] is stored as: uint(c * 255.0f), truncated."""
    return (np.clip(np.asarray(rgb, np.float32), np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.uint32)


# ---- 1. skin: both kernels, without and with attributes ----------------------------------------------------------------------------
def pixel_grid(nv, w, h):
    """Vertex i at the centre of pixel (2 (i mod 512), i div 512), a random colour each."""
    i = np.arange(nv)
    px, py = 2 * (i % 512) + 0.5, i // 512 + 0.5
    assert py.max() < h and px.max() + 1 < w
    xyz = np.stack([px / w * 2.0 - 1.0, 1.0 - py / h * 2.0, np.full(nv, 0.5)], axis=-1)
    return K._pack(xyz, np.random.default_rng(0x5C1).uniform(0.02, 0.98, (nv, 3)))


def two_joints(kind, w):
    """The identity, and a translation of one pixel in x."""
    if kind == "matrices":
        return np.stack([SM.joint_matrix(), SM.joint_matrix(tx=2.0 / w)])
    return np.stack([DQ.IDENTITY, DQ.dq_joint((0, 0, 1), 0.0, (2.0 / w, 0.0, 0.0))])


def pose(kind, v, j, wt, table):
    return SM.pose_vertices(v, j, wt, table) if kind == "matrices" else DQ.pose_vertices(v, j, wt, table)


def pose_attrs(kind, a, j, wt, table):
    return SM.pose_attrs(a, j, wt, table) if kind == "matrices" else DQ.pose_attrs(a, j, wt, table)


def set_pose(ctx, kind, table):
    ctx.pose_set(table) if kind == "matrices" else ctx.pose_set_dq(table)


def pixels_of(oracle, v, w, h):
    sx, sy, _ = oracle.project(v, IDENT, w, h)
    return sx.astype(np.int64), sy.astype(np.int64)


@gpu
@pytest.mark.parametrize("kind", ["matrices", "dual_quaternions"])
def test_skin_vertex_frame(swr, oracle, kind):
    """k_skin_vertices<LDS, false> / k_skin_vertices_dq<false> on 262 144 + 257 vertices: a vertex frame in which every vertex owns a
    pixel, against a context that uploaded the model-posed vertices.  Two rigs: one influence of weight 1, and the same joint twice
    with 0.5 + 0.5."""
    s = G.SHAPES["skin"]
    nv, w, h = s["units"], s["width"], s["height"]
    cap = next(c for c in G.CAPS if c.shape == "skin" and c.kernel.startswith("k_skin_vertices" + ("<" if kind == "matrices" else "_dq")))
    first_trip = cap.threshold - 1
    v = pixel_grid(nv, w, h)
    table = two_joints(kind, w)
    idx = np.arange(nv, dtype=np.int64)
    tail = idx >= first_trip
    assert tail.sum() == 257
    j1 = np.zeros((nv, 4), np.uint32)
    j1[:, 0] = idx % 2
    w1 = np.zeros((nv, 4), np.float32)
    w1[:, 0] = 1.0
    j2, w2 = j1.copy(), w1.copy()
    j2[:, 1] = j2[:, 0]
    w2[:, 0:2] = 0.5
    bx, by = pixels_of(oracle, v, w, h)
    with swr.Context(0) as ctx, swr.Context(0) as ref:
        ctx.scene_upload(v, idx)
        ctx.target_set(w, h)
        ref.target_set(w, h)
        for name, (j, wt) in (("one influence", (j1, w1)), ("0.5 + 0.5", (j2, w2))):
            posed = pose(kind, v, j, wt, table)
            # from the model: beyond the first trip every vertex owns its pixel, half of them moved, neighbours differ in colour
            x, y = pixels_of(oracle, posed, w, h)
            owners = np.bincount(y * w + x, minlength=w * h)
            alone = owners[(y * w + x)[tail]] == 1
            moved = (x[tail] != bx[tail]) | (y[tail] != by[tail])
            print(f"{kind}, {name}: {alone.mean():.3f} of the tail own their pixel, {moved.mean():.3f} moved")
            assert alone.mean() >= 0.95 and moved.mean() >= 0.40 and (y[tail] >= first_trip // 512).all(), name
            q = quantised(posed[tail, 4:7])
            packed = (q[:, 0] << 16) | (q[:, 1] << 8) | q[:, 2]
            assert np.unique(packed).size == packed.size, "two colours of the tail's row quantise to one pixel value"
            ctx.scene_skin(j, wt)
            set_pose(ctx, kind, table)
            ref.scene_upload(posed, idx)
            got, want = frame(ctx, 0, VERTICES), frame(ref, 0, VERTICES)
            same_frames(got, want, f"{kind}, {name}")
            drawn = (words(want[0])[first_trip // 512:] != 0).sum()
            assert drawn >= 0.95 * 257, f"{drawn} of the tail's points are in the reference frame"


@gpu
@pytest.mark.parametrize("kind", ["matrices", "dual_quaternions"])
def test_skin_shaded_frame(swr, oracle, kind):
    """k_skin_vertices<LDS, true> / k_skin_vertices_dq<true>: a z-tested Phong frame of triangles whose corners all lie beyond the first
    trip (the first 262 144 vertices are filler), under 64 joints of small rotations, against a context that uploaded the model-posed
    vertices and normals, and against the oracle."""
    s = G.SHAPES["skin"]
    nv, w, h = s["units"], s["width"], s["height"]
    first_trip = nv - 257
    v = pixel_grid(nv, w, h)
    sv, si = TDQ.strip(257)
    v[first_trip:] = sv
    idx = si + first_trip
    assert idx.min() >= first_trip == 1024 * 256
    dq, j, wt = TDQ.random_rig(nv, 64, 0x64)
    table = dq if kind == "dual_quaternions" else DQ.matrices_of(dq)
    sh = swr.scenes.random_shading(nv, 0x77, 1)
    posed = pose(kind, v, j, wt, table)
    posed_sh = dataclasses.replace(sh, attrs=pose_attrs(kind, sh.attrs, j, wt, table))
    wc, wd = K.oracle_clear(oracle, posed, idx, IDENT, w, h, DT, shading=posed_sh)
    uc, _ = K.oracle_clear(oracle, v, idx, IDENT, w, h, DT, shading=sh)
    won = np.isfinite(wd)
    changed = won & (wc != uc).any(axis=-1)
    print(f"{kind}: {won.sum()} pixels won by triangles of the tail, {changed.sum()} of them coloured otherwise than unposed")
    assert won.sum() >= 1000 and changed.sum() >= 500
    sx, sy, _ = oracle.project(posed, IDENT, w, h)
    area = 0.5 * np.abs((sx[idx[1::3]] - sx[idx[0::3]]) * (sy[idx[2::3]] - sy[idx[0::3]])
                        - (sx[idx[2::3]] - sx[idx[0::3]]) * (sy[idx[1::3]] - sy[idx[0::3]]))
    assert area.size == 255 and (area >= 8).all(), "every triangle covers at least 8 pixels"
    M = swr.binding.Material.from_shading(sh)
    with swr.Context(0) as ctx, swr.Context(0) as ref:
        for c, vv, attrs in ((ctx, v, sh.attrs), (ref, posed, posed_sh.attrs)):
            c.scene_upload(vv, idx)
            c.target_set(w, h)
            c.material_set(M)
            c.scene_attributes(attrs)
        ctx.scene_skin(j, wt)
        set_pose(ctx, kind, table)
        got, want = frame(ctx, DT), frame(ref, DT)
        same_frames(got, want, f"{kind}, Phong")
        same_frames(got, (wc, wd), f"{kind}, Phong, the oracle")


# ---- 2. delta pack -------------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5A5A5A5


def delta_round(swr, w, h, y0):
    """A full delivery into a pageable image, then one pixel changed in the first tile of row y0 and one in the last tile.  Returns
    (stats, destination words, second image) of the second read; the destination's rows from y0 on hold a sentinel before it."""
    rng = np.random.default_rng(w * h)
    img = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)
    img[img == SENTINEL] ^= 1
    dst = np.zeros((h, w, 4), np.uint8)
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.target_write(img.view(np.uint8).reshape(h, w, 4), None)
        st = ctx.read_color_delta(dst)
        assert st.full == 1 and st.tiles_changed == st.tiles and np.array_equal(words(dst), img)
        img2 = img.copy()
        img2[y0, 0] ^= 0x80000001
        img2[h - 1, w - 1] ^= 0x80000001
        ctx.target_write(img2.view(np.uint8).reshape(h, w, 4), None)
        words(dst)[y0:] = SENTINEL          # (inside R every word is delivered again: none of these may survive)
        st = ctx.read_color_delta(dst)
    return st, words(dst), img2


@gpu
@pytest.mark.parametrize("path", ["words", "quads"])
def test_delta_pack_rectangle(swr, path):
    """k_delta_pack<false> (width % 4 != 0) and <true>: a rectangle of more than 4096 x 256 words / quads.  A rectangle that is the
    whole band is delivered by the plain copy, so this one leaves out the first tile row."""
    s = {"words": G.SHAPES["delta_words"], "quads": G.SHAPES["delta_quads"]}[path]
    w, h, y0 = s["width"], s["height"], s["y0"]
    per_row = w // 4 if path == "quads" else w
    assert s["units"] == per_row * (h - y0) > FIRST_TRIP and (w % 4 == 0) == (path == "quads")
    row2 = y0 + FIRST_TRIP // per_row            # the row of the rectangle's unit 4096 x 256: the second trip starts in it
    assert y0 < row2 < h - 1, "whole rows of the rectangle lie beyond the first trip, the changed last pixel among them"
    st, dst, img2 = delta_round(swr, w, h, y0)
    assert st.rect == (0, y0, w, h) and st.tiles_changed == 2 and st.full == 0 and st.bytes_copied == 4 * w * (h - y0)
    assert np.array_equal(dst[:row2], img2[:row2]), "rows of the first trip"
    bad = np.nonzero(dst[row2:] != img2[row2:])
    assert bad[0].size == 0, (f"{bad[0].size} words beyond unit {FIRST_TRIP} of the packed rectangle differ, first at "
                              f"(y,x)=({row2 + bad[0][0]},{bad[1][0]}): {dst[row2:][bad][0]:#x}")


@gpu
@pytest.mark.parametrize("w,h", [(1026, 1024), (2048, 2052)], ids=["words", "quads"])
def test_delta_whole_target(swr, w, h):
    """The changed tiles are the first and the last: R is the whole target (delivered by the plain copy, not by k_delta_pack)."""
    st, dst, img2 = delta_round(swr, w, h, 0)
    assert st.rect == (0, 0, w, h) and st.tiles_changed == 2 and st.full == 0
    per_row = w // 4 if w % 4 == 0 else w
    row2 = FIRST_TRIP // per_row
    assert np.array_equal(dst[:row2], img2[:row2]), "rows before unit 1 048 576"
    assert row2 < h and np.array_equal(dst[row2:], img2[row2:]), "rows whose first word lies beyond unit 1 048 576"


# ---- 3. k_clip_ids ---------------------------------------------------------------------------------------------------------------------
def clip_scene():
    """12 floor triangles with one corner behind the near plane and two in the distance (clipped into a quad: two fans each; they reach
    the bottom of the target), then 30 triangles in front of the near plane: every fan after the first has an order number other than
    its triangle's."""
    rng = np.random.default_rng(0xC11)
    tris = []
    for k in range(12):
        x = -0.55 + 0.1 * k
        tris.append([(x, -0.6, 0.2), (3 * x - 0.3, -0.55, rng.uniform(2.5, 4.0)), (3 * x + 0.3, -0.5, rng.uniform(2.5, 4.0))])
    for k in range(30):
        c = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-0.8, 0.8), rng.uniform(1.5, 5.0)])
        tris.append((c + rng.uniform(-0.5, 0.5, (3, 3)) * [1, 1, 0.3]).tolist())
    xyz = np.asarray(tris, np.float64).reshape(-1, 3)
    return K._pack(xyz, rng.uniform(0, 1, (xyz.shape[0], 3))), np.arange(xyz.shape[0], dtype=np.int64)


@gpu
def test_clip_ids_past_the_cap(swr, oracle):
    """A z-tested depth-clip frame with primitive IDs on 1280 x 832: k_clip_ids maps fan order numbers back to the triangles'
    numbers, rows 820 to 831 in its second trip."""
    s = G.SHAPES["band"]
    w, h, row = s["width"], s["height"], s["row"]
    assert s["units"] > FIRST_TRIP >= (row - 1) * w + 1 and row * w >= FIRST_TRIP
    v, i = clip_scene()
    m = TDC.metal_perspective(aspect=w / h)
    flags = DT | CLIP | IDS
    assert TDC.crosses(v, i, m)[:12].all() and not TDC.crosses(v, i, m)[12:].any()
    V, _, I, fmap, fans = TDC.restate(v, i, m)
    c, d = TDC.oracle_frame(oracle, V, I, w, h, flags)
    dec = []
    for inv in (False, True):
        cv, ci = TDC.coded(V, I, inv)
        dec.append(TDC.decode(TDC.oracle_frame(oracle, cv, ci, w, h, flags)[0], inv))
    assert np.array_equal(dec[0], dec[1])
    order = dec[0].astype(np.int64)
    hit = order != K.NONE
    rid = order.copy()
    rid[hit] = fmap[order[hit]]
    renamed = hit & (rid != order)
    below = np.zeros_like(hit)
    below[row:] = True
    crossing = np.unique(rid[renamed & below])
    print(f"{(renamed & below).sum()} pixels in rows >= {row} carry a renamed ID, of {crossing.size} triangles "
          f"({(crossing < 12).sum()} of them clipped)")
    assert (renamed & below).sum() >= 500 and (crossing < 12).sum() >= 2 and fmap.size > i.size // 3
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(w, h)
        ctx.draw(m, flags)
        TDC.same(ctx, flags, (c, d, rid), "clip IDs on 1280 x 832")


# ---- 4. vertex and line frames ----------------------------------------------------------------------------------------------------------
def point_scene(w, h, row):
    """3 000 short segments (6 000 vertices) all over the target, and 600 more (1 200 vertices) in rows >= row."""
    rng = np.random.default_rng(0xD07)
    n, low = 3000, 600
    a = np.stack([rng.uniform(-1.02, 1.02, n + low), rng.uniform(-1.02, 1.02, n + low), rng.uniform(0, 1, n + low)], axis=-1)
    a[n:, 1] = rng.uniform(-1.0, 1.0 - 2.0 * (row + 1) / h, low)
    b = a + np.stack([rng.uniform(-0.04, 0.04, n + low), rng.uniform(-0.04, 0.04, n + low), np.zeros(n + low)], axis=-1)
    b[n:, 1] = rng.uniform(-1.0, 1.0 - 2.0 * (row + 1) / h, low)
    xyz = np.stack([a, b], axis=1).reshape(-1, 3)
    return K._pack(xyz, rng.uniform(0.05, 1.0, (xyz.shape[0], 3))), np.arange(xyz.shape[0], dtype=np.int64)


def cover_scene():
    """Two triangles that cover the whole target."""
    xyz = np.array([[-1.5, -1.5, 0.4], [1.5, -1.5, 0.4], [-1.5, 1.5, 0.4], [1.5, 1.5, 0.6], [-1.5, 1.5, 0.6], [1.5, -1.5, 0.6]])
    return K._pack(xyz, np.full((6, 3), 0.7)), np.arange(6, dtype=np.int64)


_BAND = {}


def framebuffers():
    """The framebuffers a context rotates through (swr_api.hip: NFB = NSLOT = SWR_NSLOT)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "software-renderer_amd", "csrc", "swr_api.hip")).read()
    assert "static constexpr int NFB = NSLOT;" in src and "static constexpr int NSLOT = SWR_NSLOT;" in src
    return int(re.search(r"#define SWR_NSLOT (\d+)\b", src).group(1))


def band_expectation(oracle, prim, w, h):
    if prim not in _BAND:
        v, i = point_scene(w, h, G.SHAPES["band"]["row"])
        ptype, flags = {"vertices": (VERTICES, 0), "real_lines": (LINE, REAL_LINES), "line_stub": (LINE, 0)}[prim]
        c, d, _, code = oracle.render(v, i, IDENT, w, h, flags, primitive_type=ptype)
        assert code == 0
        _BAND[prim] = (v, i, ptype, flags, c, d)
    if "cover" not in _BAND:
        cv, ci = cover_scene()
        _BAND["cover"] = (cv, ci) + K.oracle_clear(oracle, cv, ci, IDENT, w, h, DT)
        _BAND["start"] = K.special_start(w, h, 0x57A)
    return _BAND[prim], _BAND["cover"], _BAND["start"]


@gpu
@pytest.mark.parametrize("action", ["clear", "load"])
@pytest.mark.parametrize("prim", ["vertices", "real_lines", "line_stub"])
def test_vertex_and_line_frames(swr, oracle, prim, action):
    """k_clear_band<LOAD> and k_points_resolve<LOAD> on 1280 x 832 against the oracle: a clear frame drawn over a frame that covered
    every pixel, and a load frame over a written image with special depths."""
    s = G.SHAPES["band"]
    w, h, row = s["width"], s["height"], s["row"]
    assert s["units"] > FIRST_TRIP and row * w >= FIRST_TRIP
    (v, i, ptype, flags, oc, od), (cv, ci, cc, cd), (c0, d0) = band_expectation(oracle, prim, w, h)
    landed = oc[..., 3] == 255
    print(f"{prim}: {landed[row:].sum()} pixels land in rows >= {row}")
    assert landed[row:].sum() >= (0 if prim == "line_stub" else 200) and (prim != "line_stub" or not landed.any())
    assert (~landed[row:]).sum() >= 1000
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        if action == "clear":
            assert (cc[row:, :, 3] == 255).all() and np.isfinite(cd[row:]).all(), "the earlier frame covers rows beyond the first trip"
            assert (words(cc)[row:] != words(oc)[row:]).sum() >= 1000
            ctx.scene_upload(cv, ci)
            for _ in range(framebuffers()):     # (consecutive frames go to consecutive framebuffers: the next frame's was covered)
                same_frames(frame(ctx, DT), (cc, cd), "the covering frame")
            ctx.scene_upload(v, i)
            same_frames(frame(ctx, flags, ptype), (oc, od), f"{prim}, clear frame")
        else:
            want = np.where(landed[..., None], oc, c0)
            assert (words(want)[row:] == words(c0)[row:]).sum() >= 1000, "loaded pixels stay where nothing landed"
            ctx.scene_upload(v, i)
            ctx.target_write(c0, d0)
            same_frames(frame(ctx, flags | LOAD, ptype), (want, d0), f"{prim}, load frame")


# ---- 5. k_validate_indices ---------------------------------------------------------------------------------------------------------------
def degenerate_scene(ntri, nv=3000):
    """ntri degenerate triangles (one vertex three times) over nv vertices right of the target."""
    rng = np.random.default_rng(ntri)
    xyz = np.stack([rng.uniform(4.0, 5.0, nv), rng.uniform(-1, 1, nv), rng.uniform(0, 1, nv)], axis=-1)
    return K._pack(xyz, rng.uniform(0, 1, (nv, 3))), np.repeat(rng.integers(0, nv, ntri), 3).astype(np.int64)


def refused(swr, call):
    with pytest.raises(swr.SwrError) as e:
        call()
    return e.value.code


@gpu
def test_validate_indices_upload(swr):
    """swr_scene_upload of 1 048 581 indices: one bad index at position 1 048 576 or at the end is reported; the good array is not."""
    n = G.SHAPES["validate"]["triangles"]
    v, good = degenerate_scene(n)
    assert good.size == G.SHAPES["validate"]["units"] == FIRST_TRIP + 5
    with swr.Context(0) as ctx:
        for at in (FIRST_TRIP, good.size - 1):
            assert at >= FIRST_TRIP, "the position is first read on the second trip"
            for value in (v.shape[0], -1):
                bad = good.copy()
                bad[at] = value
                assert refused(swr, lambda: ctx.scene_upload(v, bad)) == INDEX_RANGE, f"index {value} at position {at} was not reported"
                ctx.scene_upload(v, good)


@gpu
@pytest.mark.parametrize("shape", ["validate", "validate_oneshot"])
def test_validate_indices_one_shot(swr, shape):
    """swr_render without a scene identity checks the index array chunk by chunk (70 per cent, then the rest), one launch each.  With
    349 527 triangles no chunk reaches the cap; with 499 323 the first chunk alone holds 1 048 704 indices."""
    n = G.SHAPES[shape]["triangles"]
    v, good = degenerate_scene(n)
    chunk = 3 * G.oneshot_first_chunk(n)
    crosses = chunk > FIRST_TRIP
    assert crosses == (shape == "validate_oneshot") and (not crosses or G.SHAPES[shape]["units"] == chunk) and n >= 1 << 18
    with swr.Context(0) as ctx:
        for at in (FIRST_TRIP, good.size - 1, chunk - 1):
            assert not crosses or at >= FIRST_TRIP
            for value in (v.shape[0], -1):
                bad = good.copy()
                bad[at] = value
                assert refused(swr, lambda: ctx.render(v, bad, IDENT, 64, 32, 0)) == INDEX_RANGE, \
                    f"index {value} at position {at} was not reported"
                ctx.render(v, good, IDENT, 64, 32, 0)


# ---- 6. item bounds: two work units share a partial record --------------------------------------------------------------------------------
@gpu
def test_item_bounds_two_units_share_a_record(swr):
    """An item of 32 x ITEM_BOUNDS_CHUNK + 1 triangles in the caller's order: work unit 32 — the last triangle alone — folds into
    partial record 0 after (or before) unit 0.  That triangle holds the item's extremes of x, y and z and its only corner behind the eye."""
    s = G.SHAPES["item_bounds"]
    C, S, count = s["chunk"], s["slots"], s["units"]
    assert count == S * C + 1
    w, h = 200, 136
    n = 5 + count
    rng = np.random.default_rng(0x1B2)
    xyz = np.concatenate([rng.uniform(-0.5, 0.5, (3 * n, 2)), rng.uniform(-0.5, 0.5, (3 * n, 1))], axis=-1)
    # through w = z + 2 (x and y doubled): a corner behind the eye at the right edge and the farthest z, one at the left edge and the
    # nearest z, one at the bottom edge
    xyz[3 * (n - 1):] = [[-0.24, -0.235, -2.5], [-0.24, 0.24, -1.5], [0.0, -0.24, -1.5]]
    v, i = K._pack(xyz, rng.uniform(0, 1, (3 * n, 3))), np.arange(3 * n, dtype=np.int64)
    persp = np.zeros(16, np.float32)
    persp[0], persp[5], persp[10], persp[11], persp[15] = 2.0, 2.0, 1.0, 1.0, 2.0
    items = [(0, 15, K.affine_matrix()), (15, 3 * count, persp)]
    without = [(0, 15, K.affine_matrix()), (15, 3 * (count - 1), persp)]
    with swr.Context(0) as ctx:
        ctx.debug_set(DEBUG_STREAM_ORDER, 0)            # the caller's order: the item's unit u is its triangles [u C, (u + 1) C)
        ctx.scene_upload(v, i)
        ctx.target_set(w, h)
        for flags in (0, METAL):
            want = IBM.item_bounds(v, i, items, w, h, flags)
            short = IBM.item_bounds(v, i, without, w, h, flags)
            assert want["drawable"][1] == count and want["behind"][1] == 1 and short["behind"][1] == 0
            for field in ("x0", "x1", "y0", "y1", "zmin", "zmax"):
                assert want[field][1] != short[field][1], f"unit 32 does not move {field}"
            got = ctx.item_bounds(items, flags)
            for k in range(2):
                assert got[k].tobytes() == want[k].tobytes(), f"flags {flags}, item {k}: {got[k]} is not the model's {want[k]}"
