"""The boundary of the delta reads (include/swr.h "Delta reads"): the symbols, the layout of swr_delta_stats, the bits of
swr_delta_reset and the header's normative text.  CPU only; the error codes that need a device are in tests/test_delta_read.py."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
SYMBOLS = ("swr_read_color_delta", "swr_read_depth_delta", "swr_delta_reset", "swr_render_delta")


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def test_symbols_and_struct(swr):
    L = swr.load_library()
    B = swr.binding
    for name in SYMBOLS:
        assert hasattr(L, name) and name in B.ABI_SYMBOLS, name
    assert ctypes.sizeof(B.DeltaStats) == 48
    assert [(f, getattr(B.DeltaStats, f).offset) for f, _ in B.DeltaStats._fields_] == [
        ("x0", 0), ("y0", 4), ("x1", 8), ("y1", 12), ("tiles", 16), ("tiles_changed", 24), ("bytes_copied", 32), ("full", 40),
        ("reserved", 44)]
    assert B.DeltaStats.tiles.size == 8 and B.DeltaStats.full.size == 4
    assert (B.DELTA_COLOR, B.DELTA_DEPTH) == (1, 2)
    assert L.swr_abi_version() == 6
    assert (L.swr_tile_cols(), L.swr_tile_rows()) == (64, 32)      # the tiles of the delta reads are the library's tiles


def test_header_text():
    h = header()
    assert re.search(r"typedef struct swr_delta_stats \{\s*int32_t x0, y0, x1, y1;[^}]*int64_t tiles;[^}]*int64_t tiles_changed;[^}]*"
                     r"int64_t bytes_copied;[^}]*int32_t full;[^}]*int32_t reserved;[^}]*\} swr_delta_stats;\s*/\* 48 bytes \*/", h)
    assert re.search(r"enum \{ SWR_DELTA_COLOR = 1, SWR_DELTA_DEPTH = 2 \};", h)
    assert re.search(r"int\s+swr_read_color_delta\(swr_context\*\s*\w*,\s*void\*\s*\w*,\s*swr_delta_stats\*\s*\w*\);", h)
    assert re.search(r"int\s+swr_read_depth_delta\(swr_context\*\s*\w*,\s*float\*\s*\w*,\s*swr_delta_stats\*\s*\w*\);", h)
    assert re.search(r"int\s+swr_delta_reset\(swr_context\*\s*\w*,\s*uint32_t\s*\w*\);", h)
    assert re.search(r"int\s+swr_render_delta\(swr_context\*\s*\w*,\s*const swr_render_pass\*\s*\w*,\s*swr_delta_stats\s+\w*\[2\]\);", h)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    assert h.index("---- Depth queries") < h.index("---- Delta reads") < h.index("---- Load frames"), "next to 'Depth queries'"
    for text in ("the presence of the swr_read_color_delta symbol is the feature test",
                 "anchored at pixel (0, 0) of the full target",
                 "The pointer may\n *     differ from call to call; the content may not",
                 "compared as bits", "-0 against +0, are therefore changes; equal NaN bits are not",
                 "tiles_changed is the exact number of changed tiles",
                 "nothing outside is touched", "but never a pixel of an unchanged tile outside R; bytes_copied says what it did",
                 "byte for byte what swr_read_color / swr_read_depth would deliver",
                 "no framebuffer image is\n *     modified",
                 "The same target again keeps it",
                 "A group writes stats once, after every band succeeded",
                 "SWR_FLAG_LOAD returns SWR_ERR_UNSUPPORTED",
                 "After an error dst, stats and the baselines are untouched"):
        assert text in h, text


def test_null_context_is_refused(swr):
    L = swr.load_library()
    B = swr.binding
    img = np.zeros((4, 4), dtype=np.uint32)
    st = B.DeltaStats()
    ctypes.memset(ctypes.byref(st), 0x7F, 48)
    assert L.swr_read_color_delta(None, img.ctypes.data, ctypes.byref(st)) == BAD_ARG
    assert L.swr_read_depth_delta(None, img.ctypes.data, ctypes.byref(st)) == BAD_ARG
    assert L.swr_read_color_delta(None, None, None) == BAD_ARG
    assert L.swr_delta_reset(None, B.DELTA_COLOR) == BAD_ARG
    assert L.swr_render_delta(None, ctypes.byref(B.RenderPass()), None) == BAD_ARG
    assert bytes(st) == b"\x7f" * 48 and not img.any()
