"""The numpy model of the delta reads (tests/delta_model.py) on hand cases, and the classes of outcome the GPU cases of
tests/test_delta_read.py are drawn from.  CPU only."""
import numpy as np
import pytest

import delta_model as M


def image(w, h, seed=1):
    return np.random.default_rng(seed).integers(0, 2 ** 32, (h, w), dtype=np.uint32)


def flipped(prev, pts):
    cur = prev.copy()
    for x, y in pts:
        cur[y, x] ^= 0x80000000
    return cur


@pytest.mark.parametrize("pt,tile,rect", [
    ((63, 31), (0, 0), (0, 0, 64, 32)),             # the last word of the first tile
    ((64, 32), (1, 1), (64, 32, 128, 64)),          # the first word of its diagonal neighbour
    ((0, 0), (0, 0), (0, 0, 64, 32)),
    ((129, 69), (2, 2), (128, 64, 130, 70)),        # the last pixel of the ragged corner tile: 2 x 6 pixels
])
def test_one_word(pt, tile, rect):
    w, h = 130, 70
    prev = image(w, h)
    cur = flipped(prev, [pt])
    dst = prev.copy()
    d, out = M.delta(prev, cur, [(0, h)], dst)
    assert (d.tiles, d.tiles_changed, d.full) == (9, 1, 0)
    assert d.rect == rect and d.band_rects == [rect]
    assert d.flags[0][tile[1], tile[0]] and d.flags[0].sum() == 1
    assert d.rect_bytes == d.changed_pixels * 4 == (rect[2] - rect[0]) * (rect[3] - rect[1]) * 4
    assert np.array_equal(out, cur)


def test_no_change_and_every_tile():
    w, h = 130, 70
    prev = image(w, h)
    d, out = M.delta(prev, prev.copy(), [(0, h)], prev)
    assert (d.tiles_changed, d.rect, d.rect_bytes, d.changed_pixels, d.band_rects) == (0, (0, 0, 0, 0), 0, 0, [None])
    assert np.array_equal(out, prev)
    cur = ~prev
    d, out = M.delta(prev, cur, [(0, h)], prev)
    assert (d.tiles_changed, d.rect, d.rect_bytes, d.changed_pixels) == (9, (0, 0, w, h), w * h * 4, w * h)
    assert np.array_equal(out, cur)


def test_no_baseline_delivers_the_band_whole():
    w, h = 192, 128
    cur = image(w, h)
    dst = np.full((h, w), 0xA5A5A5A5, dtype=np.uint32)
    d, out = M.delta(None, cur, [(32, 96)], dst)
    assert (d.full, d.tiles, d.tiles_changed, d.rect, d.rect_bytes) == (1, 6, 6, (0, 32, w, 96), w * 64 * 4)
    assert np.array_equal(out[32:96], cur[32:96]) and (out[:32] == 0xA5A5A5A5).all() and (out[96:] == 0xA5A5A5A5).all()


def test_the_rectangle_is_a_bounding_box_and_nothing_outside_is_written():
    w, h = 192, 96
    prev = image(w, h)
    cur = flipped(prev, [(0, 0), (191, 95)])        # two opposite corners: R is everything, seven tiles inside it did not change
    dst = prev.copy()
    d, out = M.delta(prev, cur, [(0, h)], dst)
    assert d.tiles_changed == 2 and d.rect == (0, 0, w, h) and d.rect_bytes == w * h * 4 and d.changed_pixels == 2 * 64 * 32
    cur = flipped(prev, [(70, 5), (70, 95)])        # one column of tiles
    dst = prev.copy()
    dst[3, 3] ^= 0xFF                               # a wrong word outside R stays wrong
    d, out = M.delta(prev, cur, [(0, h)], dst)
    assert d.rect == (64, 0, 128, 96) and out[3, 3] == dst[3, 3] != cur[3, 3]
    assert M.outside(d, (h, w)).sum() == w * h - 64 * 96 and np.array_equal(out[:, 64:128], cur[:, 64:128])


def test_bands_have_rectangles_of_their_own():
    w, h = 192, 128
    bands = [(0, 32), (32, 64), (64, 128)]
    prev = image(w, h)
    cur = flipped(prev, [(0, 0), (191, 127)])
    d, out = M.delta(prev, cur, bands, prev)
    assert d.band_rects == [(0, 0, 64, 32), None, (128, 96, 192, 128)]
    assert d.rect == (0, 0, 192, 128) and d.rect_bytes == 2 * 64 * 32 * 4 and d.tiles == 12 and d.tiles_changed == 2
    assert np.array_equal(out, cur)


def test_bits_not_values():
    prev = np.array([[0.0, np.nan, 1.0, -0.0]], dtype=np.float32)
    same = prev.copy()
    assert M.delta(prev, same, [(0, 1)], prev)[0].tiles_changed == 0            # an identical NaN is no change
    zero = prev.copy(); zero[0, 0] = -0.0
    assert M.delta(prev, zero, [(0, 1)], prev)[0].tiles_changed == 1            # -0 against +0 is one
    nan = prev.copy(); nan.view(np.uint32)[0, 1] ^= 1
    assert np.isnan(nan[0, 1]) and M.delta(prev, nan, [(0, 1)], prev)[0].tiles_changed == 1      # another payload too


def test_bands_of():
    assert M.bands_of(128, 3) == [(0, 32), (32, 64), (64, 128)]
    assert M.bands_of(70, 1) == [(0, 70)]
    for h, n in ((200, 3), (33, 2), (4096, 8)):
        b = M.bands_of(h, n)
        assert b[0][0] == 0 and b[-1][1] == h and all(b[k][1] == b[k + 1][0] and b[k][0] % 32 == 0 for k in range(n - 1))


@pytest.mark.parametrize("shape", sorted(M.SHAPES))
def test_every_gpu_parameter_set_reaches_every_class_its_tiles_allow(shape):
    """zero, one, several but not all, all tiles changed, an R narrower than the band and an R of full width: every shape's change
    sets produce at least one case of each — of those its tile grid allows (a single tile can be neither 'several but not all' nor
    narrower than its band; delta_model.possible says which, from the grid alone)."""
    seen, can = M.classes(shape), M.possible(shape)
    assert {"zero", "one", "all", "full_width"} <= can
    for name in can:
        assert seen[name] >= 1, (shape, name, seen)
    for name in set(seen) - can:
        assert seen[name] == 0, (shape, name, seen)
    # the shapes with a grid reach all six
    if shape in ("3x3_tiles", "ragged", "three_bands", "band_of_target"):
        assert can == set(seen)
