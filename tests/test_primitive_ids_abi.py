"""CPU-only checks of the primitive-ID boundary (SWR_FLAG_PRIMITIVE_IDS, SWR_ID_NONE, swr_read_ids): the header, the
Python binding and the library agree, with no ABI bump.  The GPU behaviour is tested in tests/test_primitive_ids.py."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_flag_the_sentinel_and_the_entry_point():
    text = open(os.path.join(ROOT, "include", "swr.h")).read()
    assert re.search(r"\bSWR_FLAG_PRIMITIVE_IDS\s*=\s*1u\s*<<\s*5\b", text)
    assert re.search(r"#define SWR_ID_NONE 0xFFFFFFFFu\b", text)
    assert re.search(r"\bint swr_read_ids\(swr_context\* ctx, uint32_t\* dst_full_image\);", text)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", text)


def test_binding_constants(swr):
    b = swr.binding
    assert b.FLAG_PRIMITIVE_IDS == 32 and b.ID_NONE == 0xFFFFFFFF
    assert "swr_read_ids" in b.ABI_SYMBOLS


def test_symbol_is_exported_and_abi_unchanged(swr):
    swr.build()
    lib = ctypes.CDLL(swr.library_path())
    assert hasattr(lib, "swr_read_ids")
    assert lib.swr_abi_version() == 6


def test_null_context_is_refused_without_a_device(swr):
    swr.build()
    lib = ctypes.CDLL(swr.library_path())
    lib.swr_read_ids.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.swr_read_ids.restype = ctypes.c_int
    buf = np.zeros(16, dtype=np.uint32)
    assert lib.swr_read_ids(None, buf.ctypes.data) == -1
    assert lib.swr_read_ids(None, None) == -1


def test_list_helper_recovers_items_and_triangles(swr):
    b = swr.binding
    m = np.eye(4, dtype=np.float32).reshape(16)
    items = [(0, 9, m), (30, 0, m), (3, 6, m), (0, 30, m)]       # 3, 0, 2 and 10 triangles: vbases 0, 3, 3, 5
    ids = np.array([[0, 2, 3, 4], [5, 14, b.ID_NONE, 7]], dtype=np.uint32)
    k, j = b.list_ids_to_items(ids, items)
    assert k.tolist() == [[0, 0, 2, 2], [3, 3, -1, 3]]
    assert j.tolist() == [[0, 2, 0, 1], [0, 9, -1, 2]]
