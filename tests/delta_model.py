"""A numpy model of the delta reads, written from include/swr.h "Delta reads" (not from the library): what a delta read of an image
`cur`, against the baseline `prev` the device keeps, does to the caller's image, for a context whose bands own the rows `bands` of the
target.  Images are (H, W) arrays of 32-bit words (a colour image viewed as uint32, a depth image viewed as uint32: the compare is on
bits).  Shared by tests/test_delta_model.py (CPU) and tests/test_delta_read.py (GPU), together with the shapes and the change sets
the GPU cases run."""
from dataclasses import dataclass, field

import numpy as np

TILE_W, TILE_H = 64, 32


@dataclass
class Delta:
    tiles: int = 0
    tiles_changed: int = 0
    changed_pixels: int = 0                 # pixels of the changed tiles: 4 x this is the least a delivery copies
    rect: tuple = (0, 0, 0, 0)              # (x0, y0, x1, y1): the bounding box of the bands' R, all 0 when nothing changed
    rect_bytes: int = 0                     # the bytes of every band's R: the most a delivery copies
    full: int = 0
    band_rects: list = field(default_factory=list)      # per band: R as (x0, y0, x1, y1) or None
    flags: list = field(default_factory=list)           # per band: (tiles_y, tiles_x) bool


def as_words(image):
    """An (H, W) uint32 view of a (H, W, 4) uint8 colour image or a (H, W) float32 depth image (or uint32 words as they are)."""
    a = np.ascontiguousarray(image)
    if a.dtype == np.uint8:
        return a.view(np.uint32).reshape(a.shape[0], a.shape[1])
    return a.view(np.uint32)


def bands_of(height, n):
    """How a context of n bands splits a target: whole tile rows, as evenly as they go (swr_context_band_info is the authority on the
    device; the model only needs bands that start at multiples of TILE_H)."""
    rows = (height + TILE_H - 1) // TILE_H
    cuts = [min(height, ((rows * k) // n) * TILE_H) for k in range(n + 1)]
    cuts[-1] = height
    return [(cuts[k], cuts[k + 1]) for k in range(n)]


def delta(prev, cur, bands, dst):
    """The delta read of `cur` with the baseline `prev` (None: no baseline) on a context that owns the row ranges `bands`; `dst` is the
    caller's image before the call.  Returns (Delta, the caller's image after the call: dst with every band's R taken from cur)."""
    cur = as_words(cur)
    H, W = cur.shape
    out = as_words(dst).copy()
    d = Delta(full=1 if prev is None else 0)
    if prev is not None:
        prev = as_words(prev)
    box = None
    for r0, r1 in bands:
        assert r0 % TILE_H == 0 and 0 <= r0 <= r1 <= H
        tx_n, ty_n = (W + TILE_W - 1) // TILE_W, (r1 - r0 + TILE_H - 1) // TILE_H
        flags = np.zeros((ty_n, tx_n), dtype=bool)
        for ty in range(ty_n):
            for tx in range(tx_n):
                ys = slice(r0 + ty * TILE_H, min(r1, r0 + (ty + 1) * TILE_H))
                xs = slice(tx * TILE_W, min(W, (tx + 1) * TILE_W))
                flags[ty, tx] = prev is None or not np.array_equal(prev[ys, xs], cur[ys, xs])
                if flags[ty, tx]:
                    d.changed_pixels += (ys.stop - ys.start) * (xs.stop - xs.start)
        d.tiles += tx_n * ty_n
        d.tiles_changed += int(flags.sum())
        d.flags.append(flags)
        if not flags.any():
            d.band_rects.append(None)
            continue
        tys, txs = np.nonzero(flags)
        x0, x1 = int(txs.min()) * TILE_W, min(W, (int(txs.max()) + 1) * TILE_W)
        y0, y1 = r0 + int(tys.min()) * TILE_H, min(r1, r0 + (int(tys.max()) + 1) * TILE_H)
        d.band_rects.append((x0, y0, x1, y1))
        d.rect_bytes += (x1 - x0) * (y1 - y0) * 4
        out[y0:y1, x0:x1] = cur[y0:y1, x0:x1]
        box = (x0, y0, x1, y1) if box is None else (min(box[0], x0), min(box[1], y0), max(box[2], x1), max(box[3], y1))
    if box is not None:
        d.rect = box
    return d, out


def outside(d, shape):
    """The pixels no delivery may write: a bool (H, W) mask of everything outside every band's R."""
    m = np.ones(shape, dtype=bool)
    for r in d.band_rects:
        if r is not None:
            m[r[1]:r[3], r[0]:r[2]] = False
    return m


# ---- the shapes and change sets of the GPU cases ---------------------------------------------------------------------------------
# name -> (width, height, bands of the context, the rows [a, b) the context owns or None for the whole target)
SHAPES = {
    "one_tile": (64, 32, 1, None),
    "one_pixel": (1, 1, 1, None),
    "3x3_tiles": (192, 96, 1, None),
    "ragged": (130, 70, 1, None),                # width % 4 != 0: the dword path; partial right and bottom tiles
    "three_bands": (192, 128, 3, None),
    "band_of_target": (192, 128, 1, (32, 96)),
}


def owned(shape):
    """The row ranges the context of SHAPES[shape] owns."""
    w, h, n, rows = SHAPES[shape]
    return [rows] if rows else bands_of(h, n)


def change_sets(shape):
    """name -> the pixels (x, y) of the full target whose word a case flips, for SHAPES[shape].  The single words sit where a tile
    index can go wrong: the last word of the first tile (63, 31), the first word of the diagonal neighbour (64, 32), the origin, and
    the last pixel of the last (ragged, where the shape has one) tile — all relative to the first owned row; pixels the shape does
    not have are left out."""
    w, h, n, rows = SHAPES[shape]
    bands = owned(shape)
    ya, yb = bands[0][0], bands[-1][1]
    inside = lambda pts: [(x, y) for x, y in pts if 0 <= x < w and ya <= y < yb]
    sets = {
        "none": [],
        "origin": inside([(0, ya)]),
        "word_63_31": inside([(63, ya + 31)]),
        "word_64_32": inside([(64, ya + 32)]),
        "last_pixel": inside([(w - 1, yb - 1)]),
        "diagonal": inside([(63, ya + 31), (64, ya + 32)]),
        "column": inside([(70, ya + 5), (70, yb - 1)]),              # one column of tiles, top and bottom: R narrower than the band
        "row": inside([(3, ya + 40), (w - 1, ya + 41)]),             # one row of tiles, left and right: R of full width
        "all": [(x, y) for y in range(ya, yb, TILE_H) for x in range(0, w, TILE_W)],
    }
    return {k: v for k, v in sets.items() if v or k == "none"}


def classes(shape):
    """Which classes of outcome the change sets of a shape produce: the counts of cases with zero, one, several but not all and all
    tiles changed, with an R narrower than the band and with an R of full width."""
    w, h, n, rows = SHAPES[shape]
    bands = owned(shape)
    seen = dict(zero=0, one=0, several=0, all=0, narrower=0, full_width=0)
    rng = np.random.default_rng(7)
    prev = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)
    for name, pts in change_sets(shape).items():
        cur = prev.copy()
        for x, y in pts:
            cur[y, x] ^= 1
        d, _ = delta(prev, cur, bands, prev)
        seen["zero"] += d.tiles_changed == 0
        seen["one"] += d.tiles_changed == 1
        seen["several"] += 1 < d.tiles_changed < d.tiles
        seen["all"] += d.tiles_changed == d.tiles
        seen["narrower"] += any(r is not None and r[2] - r[0] < w for r in d.band_rects)
        seen["full_width"] += any(r is not None and r[2] - r[0] == w for r in d.band_rects)
    return seen


def possible(shape):
    """The classes a shape's tile grid allows at all: one tile can be neither 'several but not all' nor narrower than its band."""
    w, h, n, rows = SHAPES[shape]
    bands = owned(shape)
    tx = (w + TILE_W - 1) // TILE_W
    tiles = sum(tx * ((b - a + TILE_H - 1) // TILE_H) for a, b in bands)
    p = {"zero", "all", "full_width"}
    p.add("one")                    # (with one tile, 'one' is 'all')
    if tiles >= 3:
        p.add("several")
    if tx >= 2:
        p.add("narrower")
    return p
