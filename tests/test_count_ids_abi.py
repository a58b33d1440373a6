"""The boundary of the visibility counts (include/swr.h "Visibility counts"): the symbol, the layout of swr_id_count, the two group
values and the header's normative text.  CPU only; the error codes need a device and are in tests/test_count_ids.py."""
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
    assert hasattr(L, "swr_count_ids") and "swr_count_ids" in B.ABI_SYMBOLS
    assert ctypes.sizeof(B.IdCount) == 32
    assert [(f, getattr(B.IdCount, f).offset) for f, _ in B.IdCount._fields_] == [
        ("group", 0), ("x0", 4), ("y0", 8), ("x1", 12), ("y1", 16), ("reserved", 20)]
    assert B.IdCount.reserved.size == 12
    assert (B.COUNT_PER_PRIMITIVE, B.COUNT_PER_ITEM) == (0, 1)
    assert L.swr_abi_version() == 6


def test_header_text():
    h = header()
    assert re.search(r"enum\s*\{\s*SWR_COUNT_PER_PRIMITIVE\s*=\s*0\s*,\s*SWR_COUNT_PER_ITEM\s*=\s*1\s*\}", h)
    assert re.search(r"typedef struct swr_id_count \{\s*int32_t group;[^}]*int32_t x0, y0, x1, y1;[^}]*int32_t reserved\[3\];[^}]*\} swr_id_count;", h)
    assert re.search(r"int\s+swr_count_ids\(swr_context\*\s*\w*,\s*const swr_id_count\*\s*\w*,\s*uint32_t\*\s*\w*,\s*int64_t\s*\w*,\s*uint32_t\*\s*\w*\);", h)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    assert h.index("---- Primitive IDs") < h.index("---- Visibility counts") < h.index("---- Load frames"), "next to 'Primitive IDs'"
    for text in ("counts[0] + ... + counts[n-1] + *none == (x1 - x0) * (y1 - y0)",
                 "a frame that was not a draw list counts as a list of one",
                 "the presence of the swr_count_ids symbol is the feature test"):
        assert text in h, text


def test_null_arguments_are_refused(swr):
    L = swr.load_library()
    q = swr.binding.IdCount(0, 0, 0, 1, 1, (ctypes.c_int32 * 3)(0, 0, 0))
    counts = np.zeros(4, dtype=np.uint32)
    none = ctypes.c_uint32(0)
    assert L.swr_count_ids(None, ctypes.byref(q), counts.ctypes.data, 4, ctypes.byref(none)) == BAD_ARG
    assert L.swr_count_ids(None, None, None, 0, None) == BAD_ARG
