"""The part of the raster kernels that runs once per workgroup, whatever the tile holds: the 2-D grid that names the
tile, the decisions the host fills in at launch (row-split limit, spread, rows per workgroup and per wave), the frame-uniform words
read through the scalar path, the host words published at the end of the kernel, and the interior clear / resolve of k_raster_depth
(tile wholly inside the band and the image, width % 4 == 0, one workgroup per tile) beside the edge path.  Every image is compared
bit for bit with the oracle; the targets put every edge rule on a tile and every grid regime on a launch.

A grid of at most 320 tiles runs four workgroups per tile (vs_log = 2), and the interior path needs one per tile: every target up to
512 x 512 below, the 516- and 514-wide ones included, exercises the EDGE code only.  The interior path, beside edge tiles and alone,
is what the targets of more than 320 tiles at the end of the file are for (1344 x 544 = 21 x 17 tiles and its neighbours)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, NC, LOAD = 1, 2, 16
FRAMES = {"depth_only": DT | NC, "colour_depth": DT, "painter": 0}


def reference(oracle, s, flags):
    c, d, _, rc = oracle.render(s.vertices, s.indices, s.transform, s.width, s.height, flags | oracle.TINV_PER_TRIANGLE)
    assert rc == 0
    return c, d


def same(c, d, rc, rd, what, rows=None):
    r0, r1 = rows if rows else (0, rd.shape[0])
    if c is not None:
        bad = np.nonzero((c[r0:r1] != rc[r0:r1]).any(axis=-1))
        assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ, first at (y,x)=({bad[0][0] + r0},{bad[1][0]})"
    bad = np.nonzero(d[r0:r1].view(np.uint32) != rd[r0:r1].view(np.uint32))
    assert bad[0].size == 0, (f"{what}: {bad[0].size} depth values differ, first at (y,x)=({bad[0][0] + r0},{bad[1][0]}) "
                              f"got {d[bad[0][0] + r0, bad[1][0]]!r} want {rd[bad[0][0] + r0, bad[1][0]]!r}")


def whole_frame(ctx, oracle, s, flags, what):
    rc, rd = reference(oracle, s, flags)
    c, d = ctx.render(s.vertices, s.indices, s.transform, s.width, s.height, flags)
    same(None if flags & NC else c, d, rc, rd, what)
    return rd


def soup_for(swr, w, h, seed, flags):
    """A few hundred triangles on the small targets, 2 000 on the 512-wide ones, 3 000 of r = 0.05 above; margin 1.1: some straddle
    or leave the screen."""
    ntri = 300 if w * h <= 130 * 70 else (800 if w * h <= 260 * 97 else (2000 if w * h <= 516 * 512 else 3000))
    r = 0.3 if w * h <= 260 * 97 else (0.1 if w * h <= 516 * 512 else 0.05)
    return swr.scenes.random_soup(ntri, w, h, seed, r_ndc=r, flags=flags, margin=1.1)


def tiles_of(w, rows):
    return ((w + 63) // 64) * ((rows + 31) // 32)


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("w,h", [(1, 1), (63, 31), (64, 32), (65, 33), (127, 64), (130, 70), (260, 97), (512, 512)])
def test_targets_that_put_every_edge_rule_on_a_tile(gpu_ctx, oracle, swr, w, h, frame):
    """One tile cut on both sides, exactly one tile, one pixel more than a tile, a ragged last column with and without
    width % 4 == 0, a last tile row of one row, and a target with interior tiles."""
    flags = FRAMES[frame]
    whole_frame(gpu_ctx, oracle, soup_for(swr, w, h, 0x71E0 + w, flags), flags, f"{w}x{h} {frame}")


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("w", [512, 516, 514])
def test_interior_and_edge_tiles_in_one_frame(gpu_ctx, oracle, swr, w, frame):
    """512: every tile inside the image; 516: the same tiles and a ragged last column of four pixels, width % 4 == 0; 514:
    width % 4 != 0.  128 and 144 tiles: four workgroups per tile, so all three run the edge clear / resolve on 8-row slices (full
    tiles, a ragged column stored by 16-B groups, a ragged column stored pixel by pixel) — not the interior path
    (test_interior_path_beside_edge_tiles)."""
    assert tiles_of(w, 512) <= 320
    flags = FRAMES[frame]
    whole_frame(gpu_ctx, oracle, soup_for(swr, w, 512, 0x1E00 + w, flags), flags, f"{w}x512 {frame}")


@pytest.mark.parametrize("frame", ["depth_only", "colour_depth"])
@pytest.mark.parametrize("w,h,r0,r1", [(260, 97, 0, 70), (260, 97, 32, 97), (512, 512, 32, 96), (512, 512, 64, 200)])
def test_bands(swr, oracle, w, h, r0, r1, frame):
    """Bands through target_set: one that ends inside the image at a row that is no multiple of the tile, one that starts inside it
    and ends with its ragged last row, one made of full tiles only, and one whose last tile row is cut inside a tile (rows
    192-199 of 64-199).  All of at most 320 tiles: four workgroups per tile, the edge code (the interior path in a band:
    test_band_of_more_than_320_tiles).  Nothing is written outside the band.  (A band starts at a multiple of the tile height — swr_target_set
    refuses any other, test_a_band_starts_on_a_tile_row — so rows [5, 70) and [33, 97) are drawn as [0, 70) and [32, 97).)"""
    flags = FRAMES[frame]
    s = soup_for(swr, w, h, 0xBA2D + r0, flags)
    rc, rd = reference(oracle, s, flags)
    with swr.Context() as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h, r0, r1)
        ctx.draw(s.transform, flags)
        ctx.sync()
        d = np.full((h, w), 7.0, np.float32)
        ctx.read_depth(d)
        c = None
        if not flags & NC:
            c = np.full((h, w, 4), 9, np.uint8)
            ctx.read_color(c)
    same(c, d, rc, rd, f"{w}x{h} rows [{r0}, {r1}) {frame}", rows=(r0, r1))
    assert (d[:r0] == 7.0).all() and (d[r1:] == 7.0).all()
    assert c is None or ((c[:r0] == 9).all() and (c[r1:] == 9).all())


@pytest.mark.parametrize("r0,r1", [(5, 70), (33, 97)])
def test_a_band_starts_on_a_tile_row(swr, r0, r1):
    """The grid names a tile by its row in the band: a band that started inside a tile would have no such grid, and the API has none."""
    with swr.Context() as ctx:
        with pytest.raises(swr.SwrError, match="multiple of 32"):
            ctx.target_set(260, 97, r0, r1)


@pytest.mark.parametrize("frame", ["depth_only", "colour_depth"])
@pytest.mark.parametrize("w,h,ntri,r", [(512, 512, 2000, 0.1), (1344, 544, 3000, 0.05), (1344, 544, 3000, 0.3),
                                        (3072, 1056, 3000, 0.05), (3072, 1056, 300, 0.05)])
def test_the_three_grid_regimes(gpu_ctx, oracle, swr, w, h, ntri, r, frame):
    """128 tiles: four workgroups per tile.  357 tiles: the grid does not fill the chip — bins up to 192 entries split the rows
    (r = 0.05: every tile), fuller ones are cut into chunks of less than 64 entries (r = 0.3: about 210 entries per tile, on both
    sides of 192 and of 256).  1 584 tiles: chunks of 64, the row-split limit 128; with 300 triangles most tiles are below it and
    many are empty."""
    tiles = ((w + 63) // 64) * ((h + 31) // 32)
    assert tiles == {512: 128, 1344: 357, 3072: 1584}[w]
    flags = FRAMES[frame]
    s = swr.scenes.random_soup(ntri, w, h, 0x6E1D + ntri + w, r_ndc=r, flags=flags, margin=1.1)
    whole_frame(gpu_ctx, oracle, s, flags, f"{w}x{h} {ntri} triangles r={r} {frame}")


@pytest.mark.parametrize("w,h", [(130, 70), (512, 512), (1344, 544), (1348, 550), (1346, 544)])
def test_load_frame_on_the_depth_only_kernel(swr, oracle, w, h):
    """k_raster_depth<true>: its clear is the loaded image.  A second soup drawn over the first frame's image is the clear frame
    of the two soups together (a depth-only image is the per-pixel minimum, ties keep the first drawn).  130 x 70 and 512 x 512 run
    four workgroups per tile: the edge clear.  1344 x 544: every tile through the interior clear and resolve; 1348 x 550 and
    1346 x 544: interior tiles beside a ragged column and a cut row, and width % 4 != 0 (edge clear everywhere)."""
    assert (tiles_of(w, h) > 320) == (w > 512)
    S = swr.scenes
    a = soup_for(swr, w, h, 0x10AD, DT | NC)
    b = soup_for(swr, w, h, 0x20AD, DT | NC)
    both = S.Scene("both", w, h, np.concatenate([a.vertices, b.vertices]),
                   np.concatenate([a.indices, b.indices + a.vertices.shape[0]]), a.transform, DT | NC)
    _, rd = reference(oracle, both, DT | NC)
    with swr.Context() as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(a.vertices, a.indices)
        ctx.draw(a.transform, DT | NC)
        ctx.scene_upload(b.vertices, b.indices)
        ctx.draw(b.transform, DT | NC | LOAD)
        ctx.sync()
        d = ctx.read_depth()
    same(None, d, None, rd, f"{w}x{h} load frame")


@pytest.mark.parametrize("w,h", [(512, 512), (1344, 544), (1348, 550)])
def test_zero_depth_tile_beside_ordinary_ones(swr, oracle, w, h):
    """z = 0 for the triangles of one screen corner: those tiles are rastered again with the 64-bit keys, the others are not.  Three
    frames on one context: the redo count of a launch is handed over at the end of the kernel.  512 x 512: the redo behind the edge
    resolve (four workgroups per tile); 1344 x 544: behind the interior resolve; 1348 x 550: both in one frame."""
    s = soup_for(swr, w, h, 0x2E20, DT | NC)
    v = s.vertices.reshape(-1, 3, 8)
    corner = (v[:, :, 0] < -0.5).all(axis=1) & (v[:, :, 1] > 0.5).all(axis=1)
    assert corner.sum() > 20
    v[corner, :, 2] = 0.0
    _, rd = reference(oracle, s, DT | NC)
    assert (rd == 0).any() and (rd[h // 2:] != 0).all()
    with swr.Context() as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        for k in range(3):
            ctx.draw(s.transform, DT | NC)
            ctx.sync()
            same(None, ctx.read_depth(), None, rd, f"{w}x{h} zero-depth corner, frame {k}")


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("w,h", [(1348, 544), (1346, 544), (1344, 550), (1348, 550)])
def test_interior_path_beside_edge_tiles(gpu_ctx, oracle, swr, w, h, frame):
    """More than 320 tiles: one workgroup per tile, so a tile wholly inside the image takes the interior path of k_raster_depth where
    width % 4 == 0.  1348: 21 interior columns and a ragged column of four pixels; 1346: width % 4 != 0, no tile may take the
    interior path; 1344 x 550: a last tile row of six rows; 1348 x 550: both.  The colour frames run the same prologue."""
    assert tiles_of(w, h) > 320
    flags = FRAMES[frame]
    whole_frame(gpu_ctx, oracle, soup_for(swr, w, h, 0x1A7E + w + h, flags), flags, f"{w}x{h} {frame}")


@pytest.mark.parametrize("frame", ["depth_only", "colour_depth"])
@pytest.mark.parametrize("w,h,r0,r1", [(3072, 1056, 64, 320), (3072, 1056, 64, 310), (3076, 1056, 800, 1056)])
def test_band_of_more_than_320_tiles(swr, oracle, w, h, r0, r1, frame):
    """Bands of 8 x 48 (49) tiles, one workgroup per tile: interior tiles only; a last tile row cut to 22 rows; a ragged last column
    with width % 4 == 0 in a band that ends with the image.  Nothing is written outside the band."""
    assert tiles_of(w, r1 - r0) > 320
    flags = FRAMES[frame]
    s = soup_for(swr, w, h, 0xB16B + r1, flags)
    rc, rd = reference(oracle, s, flags)
    with swr.Context() as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h, r0, r1)
        ctx.draw(s.transform, flags)
        ctx.sync()
        d = np.full((h, w), 7.0, np.float32)
        ctx.read_depth(d)
        c = None
        if not flags & NC:
            c = np.full((h, w, 4), 9, np.uint8)
            ctx.read_color(c)
    same(c, d, rc, rd, f"{w}x{h} rows [{r0}, {r1}) {frame}", rows=(r0, r1))
    assert (d[:r0] == 7.0).all() and (d[r1:] == 7.0).all()
    assert c is None or ((c[:r0] == 9).all() and (c[r1:] == 9).all())
