"""CPU-only checks of the draw-list boundary (swr_draw_list, swr_draw_item): the header, the Python binding and the
library agree, with no ABI bump.  The GPU behaviour is tested in tests/test_draw_list.py."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_item_and_the_entry_point():
    text = open(os.path.join(ROOT, "include", "swr.h")).read()
    body = re.search(r"typedef struct swr_draw_item \{(.*?)\} swr_draw_item;", text, re.S)
    assert body, "swr_draw_item is not declared"
    fields = re.findall(r"^\s*(int64_t|float)\s+(\w+)(\[16\])?;", body.group(1), re.M)
    assert [(t, n, a) for t, n, a in fields] == [("int64_t", "first_index", ""), ("int64_t", "index_count", ""),
                                                ("float", "transform", "[16]")]
    assert re.search(r"#define SWR_DRAW_LIST_MAX 4096\b", text)
    assert re.search(r"\bint swr_draw_list\(swr_context\* ctx, const swr_draw_item\* items, int32_t item_count, uint32_t flags\);",
                     text)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", text)


def test_binding_item_is_80_bytes(swr):
    b = swr.binding
    assert ctypes.sizeof(b.DrawItem) == 80
    assert b.DRAW_ITEM_DTYPE.itemsize == 80
    assert b.DRAW_LIST_MAX == 4096
    assert [f for f, _ in b.DrawItem._fields_] == ["first_index", "index_count", "transform"]
    # tuples and the structured array give the same bytes
    m = np.arange(16, dtype=np.float32)
    a = swr.Context.draw_items([(3, 6, m), (0, 0, m.reshape(4, 4))])
    assert a.dtype == b.DRAW_ITEM_DTYPE and a.size == 2
    assert a[0]["first_index"] == 3 and a[0]["index_count"] == 6 and a[0]["transform"].tobytes() == m.tobytes()
    assert swr.Context.draw_items(a) is not None


def test_symbol_is_exported_and_listed(swr):
    swr.build()
    assert "swr_draw_list" in swr.binding.ABI_SYMBOLS
    lib = ctypes.CDLL(swr.library_path())
    assert hasattr(lib, "swr_draw_list")
    assert lib.swr_abi_version() == 6


def test_null_context_is_refused_without_a_device(swr):
    swr.build()
    lib = ctypes.CDLL(swr.library_path())
    lib.swr_draw_list.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32]
    lib.swr_draw_list.restype = ctypes.c_int
    assert lib.swr_draw_list(None, None, 0, 0) == -1
    item = swr.binding.DrawItem()
    assert lib.swr_draw_list(None, ctypes.addressof(item), 1, 0) == -1
