"""The boundary of the item bounds (include/swr.h "Item bounds"): the symbol, the layout of swr_item_bound, the header's normative text
and the pure helper of the binding.  CPU only; the error codes that need a device are in tests/test_item_bounds.py."""
import ctypes
import os
import re

import numpy as np

import item_bounds_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
LAYOUT = [("x0", 0), ("y0", 4), ("x1", 8), ("y1", 12), ("zmin", 16), ("zmax", 20), ("drawable", 24), ("skipped", 28), ("behind", 32),
          ("reserved", 36)]


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def test_symbol_and_struct(swr):
    L = swr.load_library()
    B = swr.binding
    assert hasattr(L, "swr_item_bounds") and "swr_item_bounds" in B.ABI_SYMBOLS
    assert ctypes.sizeof(B.ItemBound) == 48 and B.ITEM_BOUND_DTYPE.itemsize == 48 and M.DTYPE.itemsize == 48
    assert [(f, getattr(B.ItemBound, f).offset) for f, _ in B.ItemBound._fields_] == LAYOUT
    assert [(f, B.ITEM_BOUND_DTYPE.fields[f][1]) for f in B.ITEM_BOUND_DTYPE.names] == LAYOUT
    assert [(f, M.DTYPE.fields[f][1]) for f in M.DTYPE.names] == LAYOUT
    assert B.ItemBound.reserved.size == 12 and B.ItemBound.zmin.size == 4
    assert L.swr_abi_version() == 6


def test_header_text():
    h = header()
    assert re.search(r"typedef struct swr_item_bound \{\s*int32_t\s+x0, y0, x1, y1;[^}]*float\s+zmin, zmax;[^}]*uint32_t drawable;[^}]*"
                     r"uint32_t skipped;[^}]*uint32_t behind;[^}]*uint32_t reserved\[3\];[^}]*\} swr_item_bound;", h)
    assert re.search(r"int\s+swr_item_bounds\(swr_context\*\s*\w*,\s*const swr_draw_item\*\s*\w*,\s*int32_t\s*\w*,\s*uint32_t\s*\w*,\s*"
                     r"swr_item_bound\*\s*\w*\);", h)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    assert h.index("---- Morph targets") < h.index("---- Item bounds") < h.index("---- Load frames")
    for text in ("the presence of the swr_item_bounds symbol is the feature test",
                 "r = c0 * x;   r = r + c1 * y;   r = r + c2 * z;   r = r + c3 * 1.0f;        ndc = r.xyz / r.w;",
                 "sx = (ndc.x * 0.5f + 0.5f) * W;   sy = (ndc.y * -0.5f + 0.5f) * H;   sz = ndc.z;",
                 "|v| < 2^30", "drawable + skipped == index_count / 3.", "x0 = min ix, x1 = max ix + 1, y0 = min iy, y1 = max iy + 1",
                 "a zero result is returned as +0 (m + 0.0f)", "zmin is the nearest VERTEX",
                 "subtracts a margin", "SWR_FLAG_DEPTH_CLIP\n *     returns SWR_ERR_UNSUPPORTED",
                 "After an error nothing was written", "does not count\n *     as a frame"):
        assert text in h, text


def test_depth_boxes_helper(swr):
    B = swr.binding
    b = np.zeros(3, dtype=B.ITEM_BOUND_DTYPE)
    b["x0"], b["y0"], b["x1"], b["y1"] = [1, 0, 7], [2, 0, 7], [30, 0, 7], [40, 0, 9]
    b["zmin"] = [0.5, np.inf, -0.25]
    rows = B.depth_boxes(b, 2.0 ** -10)
    assert rows.shape == (3, 5)
    assert rows[:, :4].tolist() == [[1, 2, 30, 40], [0, 0, 0, 0], [7, 7, 7, 9]]
    assert rows[0, 4] == float(np.float32(0.5) - np.float32(2.0 ** -10)) and rows[1, 4] == np.inf
    assert rows[2, 4] == float(np.float32(-0.25) - np.float32(2.0 ** -10))
    boxes = B.Context.depth_boxes(rows)                      # what Context.query_depth makes of them
    assert boxes.dtype == B.DEPTH_BOX_DTYPE and boxes["x1"].tolist() == [30, 0, 7] and boxes["z"][0] == np.float32(rows[0, 4])
    assert B.depth_boxes(np.zeros(0, dtype=B.ITEM_BOUND_DTYPE), 0.0).shape == (0, 5)
    assert np.array_equal(b.view(np.uint8), np.asarray(b).view(np.uint8)), "the helper leaves its input alone"


def test_null_context_is_refused(swr):
    L = swr.load_library()
    items = np.zeros(2, dtype=swr.binding.DRAW_ITEM_DTYPE)
    out = np.full(2 * 12, 0xA5A5A5A5, dtype=np.uint32)
    assert L.swr_item_bounds(None, items.ctypes.data, 2, 0, out.ctypes.data) == BAD_ARG
    assert L.swr_item_bounds(None, None, 0, 0, None) == BAD_ARG
    assert (out == 0xA5A5A5A5).all()
