"""Depth queries (swr_query_depth; include/swr.h "Depth queries"): screen boxes tested against the depth image on the
device — passed[k] = the pixels of box k with z_k < depth.

Two expectations, neither of them the code under test, and equality is exact everywhere:
  (a) numpy over the depth image of frame_model.expect (the unchanged oracle) for z-tested frames, or over the image the test itself
      wrote with swr_target_write;
  (b) numpy over the library's own read_depth() of the same frame, which predates the call and is itself tested against the oracle.

The frames are drawn on the small target of kernel_matrix.TARGETS (328 x 200: neither dimension is a multiple of 64 or 32, so partial
tiles exist on both edges) unless a case says otherwise.  The dense scene is that of tests/test_count_ids.py: a constant-depth triangle
(tiles accepted or rejected whole from their minimum and maximum), a field of tiny triangles at z 0.05 to 0.9 (tiles that straddle z)
and cleared screen.  The NaN classes come from the special-values image.  The figures of CLASS_MIN were taken from the oracle's image
when the box sets were designed and are checked on the CPU by test_box_sets_are_not_vacuous."""
import ctypes
import os
import re

import numpy as np
import pytest

import frame_model as FM
import kernel_matrix as K

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_depth_query.hip")
DT, NC, METAL, LOAD, IDS, BLEND = FM.DT, FM.NC, FM.METAL, FM.LOAD, FM.IDS, FM.BLEND
IDENT = K.IDENT
W, H = K.TARGETS["small"]
LW, LH = K.TARGETS["large"]
BAD_ARG, HIP, UNSUPPORTED, NO_SCENE = -1, -4, -5, -6
INF, NAN = np.float32(np.inf), np.float32(np.nan)
DENORMAL = np.float32(1e-40)

# (box, tile) pairs per class of k_depth_boxes over the dense z-tested oracle image with dense_boxes plus the special image with
# special_boxes, at T = 32 (16, 8): rejected 321 (528, 975), accepted without NaN 681 (1 348, 2 737) of which partial 352 (600, 1 085),
# accepted whole with NaNs subtracted 177 (361, 734), scanned because they straddle z 2 275 (3 659, 6 365), scanned because partial
# with NaNs 86 (111, 186).  The far triangle's depth is 0.95 to an ulp either side, so the depths next to it split its tiles between
# the classes.  The bounds asserted are the issue's: at least 8 of each.
CLASS_MIN = 8
CLASSES = ("rejected", "accepted", "accepted_partial", "accepted_whole_minus_nan", "scanned_straddle", "scanned_partial_nan")


def tile_rows():
    """T, parsed from the constants of swr_depth_query.hip."""
    src = open(SRC).read()
    t = int(re.search(r"constexpr int DQ_TILE_ROWS_PRODUCT = (\d+);", src).group(1))
    assert t in (8, 16, 32)
    return t


def split_area():
    src = open(os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_internal.h")).read()
    return 1 << int(re.search(r"constexpr uint32_t DEPTH_QUERY_SPLIT_AREA = 1u << (\d+);", src).group(1))


def dense_scene(w=W, h=H, seed=0xC0):
    """tests/test_count_ids.py's dense scene (a copy): one far triangle over the right half, 14 000 triangles of about three pixels over
    the left 54 %, 24 det == 0 slivers, and empty screen around the far triangle."""
    rng = np.random.default_rng(seed)
    tiny = K._tris(rng, 14000, 0, 0, 0.54 * w, h, 1.7, 0.05, 0.9, w, h)
    bx, by = K._ndc(np.array([0.55, 0.93, 0.55]) * w, np.array([0.04, 0.5, 0.96]) * h, w, h)
    big = (np.stack([bx, by, np.full(3, 0.95)], axis=-1), rng.uniform(0, 1, (3, 3)))
    sl = K._slivers(rng, 24, w, h)
    v = K._pack(np.concatenate([big[0], tiny[0], sl[0]]), np.concatenate([big[1], tiny[1], sl[1]]))
    return v, np.arange(v.shape[0], dtype=np.int64)


FAR_PIXEL = (100, 250)          # (y, x) inside the far triangle


def z_values(far):
    far = np.float32(far)
    return [far, np.nextafter(far, np.float32(0)), np.nextafter(far, np.float32(2)), np.float32(0.5), np.float32(0.99),
            np.float32(-0.0), np.float32(0.0), -INF, INF, NAN, DENORMAL]


def as_boxes(rows):
    a = np.zeros(len(rows), dtype=[("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32), ("z", np.float32),
                                    ("reserved", np.int32, (3,))])
    for k, (x0, y0, x1, y1, z) in enumerate(rows):
        a[k] = (x0, y0, x1, y1, z, (0, 0, 0))
    return a


def grid_boxes(zs, w, h, bw, bh, sx, sy):
    """Overlapping boxes of bw x bh at a stride of sx x sy (clipped to the target), the depths taken in turn."""
    rows, k = [], 0
    for y in range(0, h, sy):
        for x in range(0, w, sx):
            rows.append((x, y, min(x + bw, w), min(y + bh, h), zs[k % len(zs)]))
            k += 1
    return rows


def dense_boxes(T, far):
    zs = z_values(far)
    rows = [(0, 0, W, H, z) for z in zs]                                                    # the whole target with every depth
    rows += [(x, y, x + 1, y + 1, z) for x, y in ((20, 30), (250, 100), (327, 0), (0, 199), (300, 150), (64, T), (63, T - 1))
             for z in (zs[0], zs[3])]                                                       # 1 x 1
    for d0 in (-1, 0, 1):                   # edges on, one before and one after multiples of 64 columns and of T rows
        for d1 in (-1, 0, 1):
            for z in (zs[0], zs[1], zs[2], zs[3], zs[4]):
                rows.append((64 + d0, T + d0, 256 + d1, 5 * T + d1, z))
                rows.append((128 + d1, 2 * T + d1, 320 + d0, H - T + d0, z))
            rows.append((192 + d0, 3 * T + d1, 192 + d0 + 64, 4 * T + d1, zs[3]))
            rows.append((d0 + 1, 6 * T + d0, 64 + d1, 6 * T + d0 + 1, zs[3]))
    rows += [(10, 20, 10, 90, zs[3]), (10, 20, 60, 20, zs[3]), (0, 0, 0, 0, zs[3]), (W, H, W, H, zs[3])]      # empty
    rows += rows[:6] + [(5, 5, 200, 150, zs[3]), (6, 6, 201, 151, zs[3]), (5, 5, 200, 150, zs[3])]           # duplicated and overlapping
    rows += grid_boxes(zs, W, H, 70, 35, 41, 23)
    return as_boxes(rows)


def special_image():
    """kernel_matrix.special_start (NaNs, +-0, +-inf and denormals among ordinary depths: every tile of it straddles every finite z) with
    two regions of its own: rows 64..95 x columns 128..255 all NaN, and rows 96..191 x columns 0..255 of depths 0.6 .. 0.9 with one NaN
    in fifty (tiles a z of 0.5 is in front of, NaNs to subtract)."""
    c, d = K.special_start(W, H, 0xD3)
    d = d.copy()
    rng = np.random.default_rng(0xD4)
    d[64:96, 128:256] = NAN
    clean = rng.uniform(0.6, 0.9, (96, 256)).astype(np.float32)
    clean[rng.uniform(size=clean.shape) < 0.02] = NAN
    d[96:192, 0:256] = clean
    d.setflags(write=False)
    return c, d


def stored_pixel(d):
    """(y, x) of special_image: a box is tested with this pixel's value, bit for bit — the first ordinary depth of row 40 from column 290."""
    x = next(x for x in range(290, W - 6) if 0.1 < d[40, x] < 0.9)
    return 40, x


def special_boxes(T, d):
    stored = d[stored_pixel(d)]
    zs = z_values(0.5) + [stored, np.float32(0.55), np.float32(0.75), np.float32(-1e-45)]
    rows = [(0, 0, W, H, z) for z in zs]
    rows += [(128, 64, 256, 96, z) for z in (zs[3], -INF, INF)] + [(130, 66, 250, 90, zs[3]), (100, 60, 280, 100, zs[3])]   # the all-NaN tiles
    rows += [(0, 96, 256, 192, z) for z in (np.float32(0.5), np.float32(0.55), np.float32(0.75), -INF)]      # the clean region, whole tiles
    rows += [(3, 97, 250, 190, np.float32(0.5)), (65, 96 + T + 1, 190, 192 - T - 1, np.float32(0.5)), (0, 100, 256, 101, np.float32(0.5))]
    y, x = stored_pixel(d)
    rows += [(x, y, x + 1, y + 1, stored), (x - 5, y - 5, x + 6, y + 6, stored), (x, y, x + 1, y + 1, np.nextafter(stored, -INF))]
    rows += grid_boxes(zs, W, H, 90, 50, 53, 31)
    return as_boxes(rows)


def expected(depth, boxes, rows=None):
    """passed[] of the header over a depth image; rows = (r0, r1): only these rows of the target are counted (one band)."""
    r0, r1 = rows if rows is not None else (0, depth.shape[0])
    out = np.zeros(boxes.size, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        for k, b in enumerate(boxes):
            out[k] = np.count_nonzero(b["z"] < depth[max(int(b["y0"]), r0):min(int(b["y1"]), r1), int(b["x0"]):int(b["x1"])])
    return out


def classify(depth, boxes, T):
    """Every (box, tile) pair classified as k_depth_boxes does: the figures of CLASSES."""
    h, w = depth.shape
    out = dict.fromkeys(CLASSES, 0)
    with np.errstate(invalid="ignore"):
        for b in boxes:
            x0, y0, x1, y1, z = int(b["x0"]), int(b["y0"]), int(b["x1"]), int(b["y1"]), b["z"]
            if x0 >= x1 or y0 >= y1 or np.isnan(z):
                continue
            for ty in range(y0 // T, (y1 + T - 1) // T):
                for tx in range(x0 // 64, (x1 + 63) // 64):
                    tile = depth[ty * T:ty * T + T, tx * 64:tx * 64 + 64]
                    real = tile[~np.isnan(tile)]
                    nan = tile.size - real.size
                    mn = real.min() if real.size else INF
                    mx = real.max() if real.size else -INF
                    ix = min(x1, tx * 64 + 64) - max(x0, tx * 64)
                    iy = min(y1, ty * T + T) - max(y0, ty * T)
                    whole = ix * iy == tile.size
                    if not z < mx:
                        out["rejected"] += 1
                    elif z < mn and nan == 0:
                        out["accepted"] += 1
                        out["accepted_partial"] += not whole
                    elif z < mn and whole:
                        out["accepted_whole_minus_nan"] += 1
                    elif z < mn:
                        out["scanned_partial_nan"] += 1
                    else:
                        out["scanned_straddle"] += 1
    return out


def check(ctx, depth, boxes, rows=None, what=""):
    got = ctx.query_depth(boxes)
    want = expected(depth, boxes, rows)
    assert got.dtype == np.uint32 and got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} counts differ, first at box {bad[0]} {boxes[bad[0]]}: {got[bad[0]]} vs {want[bad[0]]}"
    return got


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def cache():
    return {}


@pytest.fixture(scope="module")
def dense(oracle, cache):
    """The dense scene and its expected depth on the small target, per rule set (computed once, never modified)."""
    v, i = dense_scene()
    depth = {}
    for name, flags in (("ztest", DT), ("metal", METAL), ("depth_only", DT | NC), ("painter", 0)):
        depth[name] = FM.expect(oracle, FM.FrameSpec(v, i, W, H, flags, transform=IDENT, key="dense"), cache=cache)[1]
        depth[name].setflags(write=False)
    return v, i, depth


RULES = {"painter": 0, "ztest": DT, "metal": METAL, "depth_only": DT | NC}


def test_box_sets_are_not_vacuous(dense):
    _, _, depth = dense
    T = tile_rows()
    d = depth["ztest"]
    far = d[FAR_PIXEL]
    inside = d[FAR_PIXEL[0] - 10:FAR_PIXEL[0] + 10, FAR_PIXEL[1] - 30:FAR_PIXEL[1] + 20]
    assert (np.abs(inside - np.float32(0.95)) < 1e-6).all() and np.unique(inside).size > 1, "the far triangle: 0.95 to a few ulps"
    assert np.isposinf(depth["painter"]).all() and same_bits(depth["depth_only"], d)
    boxes = dense_boxes(T, far)
    sd = special_image()[1]
    sboxes = special_boxes(T, sd)
    for t in (8, 16, 32):           # (the box sets depend on T only through their edges: every candidate tile height is covered)
        got = classify(d, dense_boxes(t, far), t)
        for k, v in classify(sd, special_boxes(t, sd), t).items():
            got[k] += v
        for k in CLASSES:
            assert got[k] >= CLASS_MIN, (t, k, got)
    # the tiles that are all NaN, and a z equal to a stored value bit for bit
    assert np.isnan(sd[64:96, 128:256]).all() and (sboxes["z"].view(np.uint32) == sd[stored_pixel(sd)].view(np.uint32)).sum() >= 3
    for image, bx in ((d, boxes), (sd, sboxes)):
        want = expected(image, bx)
        area = ((bx["x1"] - bx["x0"]) * (bx["y1"] - bx["y0"])).astype(np.uint32)
        assert (want == 0).any() and ((want == area) & (area > 0)).any() and ((want > 0) & (want < area)).any()
    # z one ulp either side of the far triangle's depth gives different answers over the whole target
    whole = expected(d, boxes[:3])
    assert whole[1] > whole[0] > whole[2] and whole[1] - whole[0] == np.count_nonzero(d == far)


# ---- one frame per rule set ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rules", ["painter", "ztest", "metal", "depth_only"])
def test_rule_sets(swr, dense, rules):
    v, i, depth = dense
    T = tile_rows()
    boxes = dense_boxes(T, depth["ztest"][FAR_PIXEL])
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw(IDENT, RULES[rules])
        got = check(ctx, depth[rules], boxes, what=rules + " (a)")                          # (a); no read has come before
        image = ctx.read_depth()
        assert same_bits(image, depth[rules])
        assert np.array_equal(check(ctx, image, boxes, what=rules + " (b)"), got)           # (b)
        if rules == "painter":              # all +inf: the area for every z below +inf, 0 for +inf and NaN
            area = ((boxes["x1"] - boxes["x0"]) * (boxes["y1"] - boxes["y0"])).astype(np.uint32)
            assert np.array_equal(got, np.where(boxes["z"] < INF, area, 0))


@gpu
def test_small_queries_skip_the_summary(swr, dense):
    """Queries whose boxes together hold a small fraction of the band are scanned directly (k_depth_boxes<false, false>); the answers
    are those of the summary route."""
    v, i, depth = dense
    d = depth["ztest"]
    zs = z_values(d[FAR_PIXEL])
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw(IDENT, DT)
        for y, x in (FAR_PIXEL, (30, 20), (0, 327), (199, 0)):
            check(ctx, d, as_boxes([(x, y, x + 1, y + 1, z) for z in zs]), what=f"1 x 1 at {x},{y}")
        small = as_boxes([(60, 10, 70, 40, zs[3]), (200, 90, 270, 110, zs[0]), (200, 90, 270, 110, zs[1]), (0, 0, 0, 0, zs[3]),
                          (W - 2, H - 3, W, H, zs[3]), (63, 15, 65, 17, zs[3])])
        assert int(((small["x1"] - small["x0"]) * (small["y1"] - small["y0"])).sum()) * 16 < W * H
        check(ctx, d, small, what="a few small boxes")
        # the same boxes inside a query that takes the summary route
        both = np.concatenate([small, as_boxes([(0, 0, W, H, zs[3])])])
        assert np.array_equal(check(ctx, d, both)[:small.size], expected(d, small))


# ---- special values -----------------------------------------------------------------------------------------------------------
@gpu
def test_special_values_load_and_blend_frames(swr, oracle, dense, cache):
    v, i, _ = dense
    T = tile_rows()
    c0, d0 = special_image()
    boxes = special_boxes(T, d0)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.target_write(c0, d0)
        first = check(ctx, d0, boxes, what="the written image")                             # no frame drawn
        assert same_bits(ctx.read_depth(), d0)
        k = [n for n, b in enumerate(boxes) if tuple(b)[:4] == (128, 64, 256, 96)]
        assert len(k) == 3 and (first[k] == 0).all(), "tiles that are all NaN pass nothing, not even -inf"
        y, x = stored_pixel(d0)
        one = [n for n, b in enumerate(boxes) if tuple(b)[:4] == (x, y, x + 1, y + 1)]
        assert first[one].tolist() == [0, 1], "z == depth does not pass; one ulp nearer does"
        # a z-tested load frame on top
        want = FM.expect(oracle, FM.FrameSpec(v, i, W, H, DT | LOAD, transform=IDENT, key="dense"), start=(c0, d0), cache=cache)[1]
        ctx.draw(IDENT, DT | LOAD)
        second = check(ctx, want, boxes, what="load frame (a)")
        assert same_bits(ctx.read_depth(), want) and (second != first).any()
        # a blend frame leaves the depth where it was: the same answers
        ctx.draw(IDENT, BLEND | DT | LOAD)
        assert np.array_equal(check(ctx, want, boxes, what="after a blend frame"), second)
        assert same_bits(ctx.read_depth(), want)


# ---- bands --------------------------------------------------------------------------------------------------------------------
def band_boxes(T, far, bands):
    zs = z_values(far)
    rows = [(0, 0, W, H, z) for z in zs[:5]]
    for a, b in bands:
        if b > a:
            rows += [(5, max(a - 3, 0), 300, min(b + 3, H), zs[3]), (7, a + 1, 201, b - 1, zs[3]), (0, a, W, b, zs[0]), (0, a, W, b, zs[1]),
                     (100, max(a - 1, 0), 101, a + 1, zs[3]), (64, b - 1, 128, min(b + 1, H), zs[3])]
    rows += [(100, 0, 101, H, zs[3]), (0, H - 1, W, H, zs[3]), (0, 0, W, 1, zs[3]), (10, 20, 10, 90, zs[3])]
    return as_boxes(rows) if len(rows) else None


@gpu
def test_three_bands_on_one_device(swr, dense):
    v, i, depth = dense
    d = depth["ztest"]
    T = tile_rows()
    with swr.Context(0, device_count=3) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        rows = [(a, b) for _, a, b in ctx.bands()]
        assert len(rows) == 3 and all(b > a for a, b in rows)
        ctx.draw(IDENT, DT)
        check(ctx, d, band_boxes(T, d[FAR_PIXEL], rows), what="3 bands: borders")           # straddle band borders, miss whole bands
        check(ctx, d, dense_boxes(T, d[FAR_PIXEL]), what="3 bands: the dense box set")
        assert same_bits(ctx.read_depth(), d)
        only_first = as_boxes([(0, 0, W, rows[0][1], np.float32(0.5)), (3, 1, 9, 2, np.float32(0.5))])
        check(ctx, d, only_first, what="3 bands: boxes that miss two of them")


@gpu
def test_a_context_that_owns_one_band_of_the_target(swr, dense):
    v, i, depth = dense
    d = depth["ztest"]
    T = tile_rows()
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H, 32, 96)
        ctx.draw(IDENT, DT)
        assert same_bits(ctx.read_depth()[32:96], d[32:96])
        boxes = np.concatenate([band_boxes(T, d[FAR_PIXEL], [(32, 96)]), dense_boxes(T, d[FAR_PIXEL]),
                                as_boxes([(0, 0, W, 32, np.float32(0.5)), (0, 96, W, H, np.float32(0.5)), (5, 31, 300, 33, np.float32(0.5)),
                                          (5, 95, 300, 97, np.float32(0.5))])])
        got = check(ctx, d, boxes, rows=(32, 96), what="rows [32, 96)")
        assert got[-4:].tolist()[:2] == [0, 0] and got.max() == 64 * W
        with pytest.raises(swr.SwrError) as e:              # the boxes are still checked against the full target
            ctx.query_depth([(0, 0, W, H + 1, 0.5)])
        assert e.value.code == BAD_ARG


# ---- limits -------------------------------------------------------------------------------------------------------------------
@gpu
def test_65536_boxes_and_one_more(swr, dense):
    v, i, depth = dense
    d = depth["ztest"]
    zs = z_values(d[FAR_PIXEL])
    rng = np.random.default_rng(0xB0)
    n = swr.binding.DEPTH_QUERY_MAX
    x, y = rng.integers(0, W - 3, n), rng.integers(0, H - 2, n)
    boxes = np.zeros(n + 1, dtype=swr.binding.DEPTH_BOX_DTYPE)
    boxes["x0"], boxes["y0"], boxes["x1"], boxes["y1"] = np.append(x, 0), np.append(y, 0), np.append(x + 3, 1), np.append(y + 2, 1)
    boxes["z"] = np.array(zs, dtype=np.float32)[np.arange(n + 1) % len(zs)]
    L = swr.load_library()
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw(IDENT, DT)
        got = check(ctx, d, boxes[:n], what="65 536 boxes")
        assert (got == 0).any() and (got == 6).any() and ((got > 0) & (got < 6)).any()
        passed = np.full(n + 1, 0xA5A5A5A5, dtype=np.uint32)
        assert L.swr_query_depth(ctx._h, boxes.ctypes.data, n + 1, passed.ctypes.data) == UNSUPPORTED
        assert (passed == 0xA5A5A5A5).all()
        assert L.swr_query_depth(ctx._h, None, 0, None) == 0                    # n == 0 with NULL pointers
        assert ctx.query_depth(np.zeros((0, 5))).size == 0
        check(ctx, d, boxes[:100], what="after the refusal")


def large_image():
    """1280 x 720: depth falling from 0.8 to 0.2 left to right (a z of 0.5 straddles the tiles of a few columns and is accepted or
    rejected by the rest), a noisy block, a block of +inf, and a sprinkle of NaNs over the top left corner."""
    rng = np.random.default_rng(0x1A)
    d = np.broadcast_to(np.linspace(0.8, 0.2, LW, dtype=np.float32), (LH, LW)).copy()
    d[300:500, 100:500] = rng.uniform(0.0, 1.0, (200, 400)).astype(np.float32)
    d[520:700, 700:1100] = INF
    corner = d[0:100, 0:300]
    corner[rng.uniform(size=corner.shape) < 0.01] = NAN
    d.setflags(write=False)
    return d


@gpu
@pytest.mark.parametrize("bands", [1, 3])
def test_large_boxes_are_split(swr, bands):
    """The large target: whole-target boxes with a mid-range z (k_depth_boxes<true, true>: the tiles of a box of DEPTH_QUERY_SPLIT_AREA
    pixels or more are shared by many workgroups) next to 4096 small ones."""
    d = large_image()
    rng = np.random.default_rng(0x1B)
    x, y = rng.integers(0, LW - 40, 4096), rng.integers(0, LH - 30, 4096)
    rows = [(0, 0, LW, LH, np.float32(0.5))]
    rows += [(int(a), int(b), int(a + 1 + k % 40), int(b + 1 + k % 30), np.float32(0.1 + 0.8 * (k % 9) / 8)) for k, (a, b) in enumerate(zip(x, y))]
    rows += [(0, 0, LW, LH, np.float32(0.5)), (0, 0, LW, 250, np.float32(0.35)), (1, 1, LW - 1, LH - 1, NAN), (3, 5, LW - 7, LH - 9, np.float32(0.65)),
             (0, 0, LW, LH, INF), (0, 0, LW, LH, -INF), (100, 300, 500, 719, np.float32(0.5))]
    boxes = as_boxes(rows)
    area = (boxes["x1"] - boxes["x0"]).astype(np.int64) * (boxes["y1"] - boxes["y0"])
    assert (area // bands >= split_area()).sum() >= 5 and (area < split_area()).sum() >= 4096
    with swr.Context(0, device_count=bands if bands > 1 else 0) as ctx:
        ctx.target_set(LW, LH)
        ctx.target_write(None, d)
        got = check(ctx, d, boxes, what=f"{bands} band(s)")
        assert 0 < got[0] < LW * LH and got[0] == got[4097] and got[4099] == 0
        assert np.array_equal(ctx.query_depth(boxes), got)
        assert same_bits(ctx.read_depth(), d)


# ---- ordering and side effects --------------------------------------------------------------------------------------------
@gpu
def test_ordering_and_side_effects(swr, dense):
    v, i, depth = dense
    d = depth["ztest"]
    T = tile_rows()
    boxes = dense_boxes(T, d[FAR_PIXEL])
    want = expected(d, boxes)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        # right after swr_target_set: the cleared image
        area = ((boxes["x1"] - boxes["x0"]) * (boxes["y1"] - boxes["y0"])).astype(np.uint32)
        assert np.array_equal(ctx.query_depth(boxes), np.where(boxes["z"] < INF, area, 0))
        ctx.draw(IDENT, DT | IDS)
        a = ctx.query_depth(boxes)                                          # before any read
        b = ctx.query_depth(boxes)                                          # back to back
        assert np.array_equal(a, want) and np.array_equal(b, want)
        color, dep, ids = ctx.read_color(), ctx.read_depth(), ctx.read_ids()
        counts = ctx.count_ids()
        assert same_bits(dep, d)
        for read in (ctx.read_color, ctx.read_depth, ctx.read_ids, ctx.count_ids):
            assert np.array_equal(ctx.query_depth(boxes), want)
            read()
            assert np.array_equal(ctx.query_depth(boxes), want)
        # the images are untouched, and so is what the other reductions return
        assert np.array_equal(ctx.read_color(), color) and same_bits(ctx.read_depth(), dep) and np.array_equal(ctx.read_ids(), ids)
        again = ctx.count_ids()
        assert np.array_equal(again[0], counts[0]) and again[1] == counts[1]
        # ... and what a load frame starts from: a triangle in front of everything, drawn over the frame
        front = K._pack(np.array([[-0.9, -0.9, -0.5], [0.9, -0.8, -0.5], [0.0, 0.9, -0.5]]), np.full((3, 3), 0.25))
        ctx.scene_upload(front, np.arange(3, dtype=np.int64))
        ctx.draw(IDENT, DT | LOAD)
        d2 = ctx.read_depth()
        covered = d2 < 0
        assert covered.sum() > 1000 and same_bits(d2[~covered], d[~covered])
        check(ctx, d2, boxes, what="after a load frame (b)")
        # fewer boxes, then more again: the staging is sized and zeroed for every query
        check(ctx, d2, boxes[:3], what="fewer boxes")
        check(ctx, d2, np.concatenate([boxes, boxes]), what="more boxes")
        # swr_target_set again: cleared again
        ctx.target_set(W, H)
        assert ctx.query_depth([(0, 0, W, H, 0.5), (0, 0, W, H, np.inf), (0, 0, W, H, np.nan), (2, 3, 50, 70, -np.inf)]).tolist() == \
            [W * H, 0, 0, 48 * 67]


@gpu
def test_bin_overflow_of_the_last_frame(swr, oracle):
    """Forced as tests/test_count_ids.py forces it: a fresh context whose fixed-stride bins are too small for 20 000 triangles in a few
    tiles.  The query is the first call that waits: it repairs the frame and tests the repaired depth."""
    w, h = 1280, 720
    s = swr.scenes.random_soup(20000, w, h, 555, r_ndc=0.01, flags=DT, margin=1.0)
    v = s.vertices.copy()
    v[:, 0] = 0.30 + (v[:, 0] * 0.5 + 0.5) * 0.07
    v[:, 1] = 0.10 + (v[:, 1] * 0.5 + 0.5) * 0.06
    v = np.ascontiguousarray(v)
    want = FM.expect(oracle, FM.FrameSpec(v, s.indices, w, h, DT, transform=s.transform))[1]
    ys, xs = np.nonzero(np.isfinite(want))
    assert ys.size > 200            # (the 20 000 triangles lie on top of each other in about 45 x 22 pixels: 539 of them are covered)
    x0, y0, x1, y1 = int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1
    mid = np.float32(np.median(want[ys, xs]))
    boxes = as_boxes([(0, 0, w, h, mid), (x0, y0, x1, y1, mid), (x0, y0, x1, y1, np.float32(-1.0)), (x0 + 3, y0 + 2, x1 - 1, y1 - 5, mid),
                      (0, 0, w, h, np.float32(2.0))])
    wp = expected(want, boxes)
    assert 0 < wp[1] < (x1 - x0) * (y1 - y0) and wp[4] == w * h - ys.size
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, s.indices)
        ctx.draw(s.transform, DT)
        assert np.array_equal(ctx.query_depth(boxes), wp), "overflowed last frame"
        assert same_bits(ctx.read_depth(), want)


@gpu
def test_render_and_render_resolved(swr, dense):
    v, i, depth = dense
    d = depth["ztest"]
    T = tile_rows()
    boxes = dense_boxes(T, d[FAR_PIXEL])
    with swr.Context(0) as ctx:
        ctx.render(v, i, IDENT, W, H, DT)
        check(ctx, d, boxes, what="swr_render")
        # a resolved render leaves the depth at sample resolution: the boxes are in samples
        w, h = 164, 100
        ctx.render_resolved(v, i, IDENT, w, h, DT, factor=2)
        assert (ctx.width, ctx.height) == (2 * w, 2 * h) == (W, H)
        check(ctx, d, boxes, what="swr_render_resolved")
        with pytest.raises(swr.SwrError) as e:
            ctx.query_depth([(0, 0, 2 * w + 1, h, 0.5)])
        assert e.value.code == BAD_ARG


@gpu
def test_frame_loop_example_prints_the_skipped_objects(swr, capsys):
    """examples/frame_loop.py --objects N --occlusion: every copy's screen rectangle and nearest depth against the previous frame."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    fl.run(3, 128, None, depth_test=True, objects=5, occlusion=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("occlusion:")]
    assert len(lines) == 2          # every frame but the first is tested against its predecessor
    for ln in lines:
        m = re.match(r"occlusion: frame (\d+): (\d+) of (\d+) objects could be skipped \(pixels that pass per object: \[(.*)\]\)", ln)
        skipped, total = int(m.group(2)), int(m.group(3))
        per = [int(t) for t in m.group(4).split(",")]
        assert total == 5 and len(per) == 5 and skipped == sum(1 for p in per if p == 0) and max(per) > 0


# ---- errors -------------------------------------------------------------------------------------------------------------------
def code_of(swr, call):
    with pytest.raises(swr.SwrError) as e:
        call()
    return e.value.code, str(e.value)


@gpu
@pytest.mark.parametrize("device_count", [0, 2])
def test_errors(swr, dense, device_count):
    v, i, depth = dense
    d = depth["ztest"]
    T = tile_rows()
    good = dense_boxes(T, d[FAR_PIXEL])
    L = swr.load_library()
    with swr.Context(0, device_count=device_count) as ctx:
        assert code_of(swr, lambda: ctx.query_depth([(0, 0, 1, 1, 0.5)]))[0] == NO_SCENE         # no target
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw(IDENT, DT)
        want = expected(d, good)
        assert np.array_equal(ctx.query_depth(good), want)
        passed = np.full(good.size, 0xA5A5A5A5, dtype=np.uint32)
        assert L.swr_query_depth(ctx._h, None, good.size, passed.ctypes.data) == BAD_ARG
        assert L.swr_query_depth(ctx._h, good.ctypes.data, good.size, None) == BAD_ARG
        assert L.swr_query_depth(ctx._h, good.ctypes.data, -1, passed.ctypes.data) == BAD_ARG
        at = good.size // 2                         # a bad box in the middle of a good list: its index is in the message
        for rect in ((0, 0, W + 1, H), (0, 0, W, H + 1), (-1, 0, W, H), (0, -1, W, H), (9, 0, 8, H), (0, 9, W, 8), (W + 1, 0, W + 1, H)):
            bad = good.copy()
            bad[at] = (*rect, 0.5, (0, 0, 0))
            bad[at + 7] = (-3, 0, 1, 1, 0.5, (0, 0, 0))
            rc = L.swr_query_depth(ctx._h, bad.ctypes.data, bad.size, passed.ctypes.data)
            text = (L.swr_last_error(ctx._h) or b"").decode()
            assert rc == BAD_ARG and f"box {at}:" in text, (rect, text)
        for word in range(3):
            bad = good.copy()
            bad["reserved"][at + 1, word] = 1
            code, text = code_of(swr, lambda: ctx.query_depth(bad))
            assert code == BAD_ARG and f"box {at + 1}:" in text, text
        assert (passed == 0xA5A5A5A5).all(), "after an error nothing was written"
        # the context is still usable
        assert np.array_equal(ctx.query_depth(good), want)


@gpu
def test_failed_context_returns_its_sticky_error(swr, dense):
    v, i, _ = dense
    ctx = swr.Context(0, wait_budget_ms=300)
    try:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ctx.draw(IDENT, DT)
        ctx.sync()
        assert ctx.query_depth([(0, 0, W, H, 0.5)])[0] > 0
        ctx.debug_fault(swr.binding.FAULT_ENQUEUE)      # the next frame's raster share fails as if a launch had returned an error
        try:
            ctx.draw(IDENT, DT)
        except swr.SwrError as e:
            assert e.code == HIP
        assert code_of(swr, lambda: ctx.query_depth([(0, 0, W, H, 0.5)]))[0] == HIP
    finally:
        ctx.close()


# ---- the table: every kernel instantiation launched in swr_depth_query.hip has a GPU case above ------------------------------
GPU_CASES = {
    "k_depth_tiles": ("test_rule_sets", "test_special_values_load_and_blend_frames", "test_three_bands_on_one_device"),
    "k_depth_boxes<true,false>": ("test_rule_sets", "test_special_values_load_and_blend_frames", "test_65536_boxes_and_one_more"),
    "k_depth_boxes<false,false>": ("test_small_queries_skip_the_summary",),
    "k_depth_boxes<true,true>": ("test_large_boxes_are_split",),
}


def test_every_launched_kernel_has_a_gpu_case():
    src = open(SRC).read()
    body = src[src.index("void launch_depth_query("):].replace(" ", "")
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(k_depth_\w+(?:<[^>]*>)?)\)?,", body))
    assert launched, "launch_depth_query launches nothing"
    assert launched == set(re.findall(r"k_depth_boxes<[^>]*>|k_depth_tiles", body)), "an instantiation outside hipLaunchKernelGGL"
    assert set(re.findall(r"__global__[^;{]*?(k_depth_\w+)\(", src)) == {"k_depth_tiles", "k_depth_boxes"}
    missing = launched - set(GPU_CASES)
    assert not missing, f"no GPU case for {sorted(missing)}"
    for variant, tests in GPU_CASES.items():
        for name in tests:
            fn = globals().get(name)
            assert callable(fn) and any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), (variant, name)
