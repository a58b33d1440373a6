"""The boundary of the depth queries (include/swr.h "Depth queries"): the symbol, the layout of swr_depth_box, the limit and the
header's normative text.  CPU only; the error codes that need a device are in tests/test_depth_query.py."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def test_symbol_and_struct(swr):
    L = swr.load_library()
    B = swr.binding
    assert hasattr(L, "swr_query_depth") and "swr_query_depth" in B.ABI_SYMBOLS
    assert ctypes.sizeof(B.DepthBox) == 32 and B.DEPTH_BOX_DTYPE.itemsize == 32
    assert [(f, getattr(B.DepthBox, f).offset) for f, _ in B.DepthBox._fields_] == [
        ("x0", 0), ("y0", 4), ("x1", 8), ("y1", 12), ("z", 16), ("reserved", 20)]
    assert [(f, B.DEPTH_BOX_DTYPE.fields[f][1]) for f in B.DEPTH_BOX_DTYPE.names] == [
        ("x0", 0), ("y0", 4), ("x1", 8), ("y1", 12), ("z", 16), ("reserved", 20)]
    assert B.DepthBox.reserved.size == 12 and B.DepthBox.z.size == 4
    assert B.DEPTH_QUERY_MAX == 1 << 16
    assert L.swr_abi_version() == 6


def test_header_text():
    h = header()
    assert re.search(r"typedef struct swr_depth_box \{\s*int32_t x0, y0, x1, y1;[^}]*float\s+z;[^}]*int32_t reserved\[3\];[^}]*\} swr_depth_box;", h)
    assert re.search(r"#define SWR_DEPTH_QUERY_MAX \(1 << 16\)", h)
    assert re.search(r"int\s+swr_query_depth\(swr_context\*\s*\w*,\s*const swr_depth_box\*\s*\w*,\s*int64_t\s*\w*,\s*uint32_t\*\s*\w*\);", h)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    assert h.index("---- Visibility counts") < h.index("---- Depth queries") < h.index("---- Load frames"), "next to 'Visibility counts'"
    for text in ("the presence of the swr_query_depth symbol is the feature test",
                 "a stored NaN is never passed; a NaN z passes nowhere; z == depth does not pass; -0 and +0 are equal",
                 "is passed by every finite z and by -inf; a stored -inf is never passed; denormals compare exactly",
                 "Every element of passed[0 .. n) is", "the message names the first offending box index",
                 "After an error nothing was written"):
        assert text in h, text


def test_boxes_from_rows(swr):
    B = swr.binding
    a = B.Context.depth_boxes([(1, 2, 3, 4, 0.5), (0, 0, 0, 0, float("nan"))])
    assert a.dtype == B.DEPTH_BOX_DTYPE and a.shape == (2,)
    assert a[0].tolist()[:5] == (1, 2, 3, 4, 0.5)[:5] and np.isnan(a["z"][1]) and not a["reserved"].any()
    assert B.Context.depth_boxes(a) is a or np.array_equal(B.Context.depth_boxes(a).view(np.uint8), a.view(np.uint8))
    assert B.Context.depth_boxes(np.zeros((0, 5))).size == 0


def test_null_context_is_refused(swr):
    L = swr.load_library()
    boxes = np.zeros(4, dtype=swr.binding.DEPTH_BOX_DTYPE)
    passed = np.zeros(4, dtype=np.uint32)
    assert L.swr_query_depth(None, boxes.ctypes.data, 4, passed.ctypes.data) == BAD_ARG
    assert L.swr_query_depth(None, None, 0, None) == BAD_ARG
