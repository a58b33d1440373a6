"""The boundary of the supersampled resolve (include/swr.h "Supersampled resolve"): the three symbols, the layout of swr_resolve, the
header's normative text, and every error code the header names.  What needs no device runs on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, NC, LOAD = 1, 2, 16
BAD_ARG, HIP, UNSUPPORTED, NO_SCENE = -1, -4, -5, -6
IDENT = np.eye(4, dtype=np.float32).T.reshape(16)
SYMBOLS = ("swr_read_color_resolved", "swr_read_depth_resolved", "swr_render_resolved")
gpu = pytest.mark.gpu


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def resolve_of(swr, factor, depth_filter=0, reserved=(0, 0)):
    return swr.binding.Resolve(factor, depth_filter, (ctypes.c_int32 * 2)(*reserved))


def test_symbols_and_struct(swr):
    L = swr.load_library()
    B = swr.binding
    for s in SYMBOLS:
        assert hasattr(L, s) and s in B.ABI_SYMBOLS
    assert ctypes.sizeof(B.Resolve) == 16
    assert [f for f, _ in B.Resolve._fields_] == ["factor", "depth_filter", "reserved"]
    assert (B.RESOLVE_DEPTH_SAMPLE0, B.RESOLVE_DEPTH_MIN) == (0, 1)
    assert L.swr_abi_version() == 6


def test_header_text():
    h = header()
    assert re.search(r"enum\s*\{\s*SWR_RESOLVE_DEPTH_SAMPLE0\s*=\s*0\s*,\s*SWR_RESOLVE_DEPTH_MIN\s*=\s*1\s*\}", h)
    assert re.search(r"typedef struct swr_resolve \{\s*int32_t factor;[^}]*int32_t depth_filter;[^}]*int32_t reserved\[2\];[^}]*\} swr_resolve;", h)
    assert re.search(r"int\s+swr_read_color_resolved\(swr_context\*\s*\w*,\s*const swr_resolve\*\s*\w*,\s*void\*\s*\w+\);", h)
    assert re.search(r"int\s+swr_read_depth_resolved\(swr_context\*\s*\w*,\s*const swr_resolve\*\s*\w*,\s*float\*\s*\w+\);", h)
    assert re.search(r"int\s+swr_render_resolved\(swr_context\*\s*\w*,\s*const swr_render_pass\*\s*\w*,\s*const swr_resolve\*\s*\w*\);", h)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    for text in ("out = (Σ_{j<S} Σ_{i<S} src[S·y+j][S·x+i][c] + S·S/2) / (S·S), integer division",
                 "if (s < m || (m != m && s == s)) m = s",
                 "the resolved alpha is the coverage"):
        assert text in h, text


def test_null_arguments_are_refused(swr):
    L = swr.load_library()
    r = resolve_of(swr, 2)
    buf = np.zeros(16, dtype=np.uint8)
    rp = swr.binding.RenderPass()
    assert L.swr_read_color_resolved(None, ctypes.byref(r), buf.ctypes.data) == BAD_ARG
    assert L.swr_read_depth_resolved(None, ctypes.byref(r), buf.ctypes.data) == BAD_ARG
    assert L.swr_render_resolved(None, ctypes.byref(rp), ctypes.byref(r)) == BAD_ARG
    assert L.swr_read_color_resolved(None, None, None) == BAD_ARG


def code_of(swr, call):
    with pytest.raises(swr.SwrError) as e:
        call()
    return e.value.code


def small_scene():
    v = np.zeros((6, 8), dtype=np.float32)
    v[:, 0:3] = [(-0.8, -0.8, 0.3), (0.8, -0.7, 0.4), (0.0, 0.8, 0.5), (-0.5, 0.6, 0.2), (0.6, 0.5, 0.6), (0.1, -0.9, 0.7)]
    v[:, 4:7] = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]
    return v, np.arange(6, dtype=np.int64)


@gpu
@pytest.mark.parametrize("device_count", [0, 2])
def test_error_codes(swr, device_count):
    L = swr.load_library()
    v, i = small_scene()
    with swr.Context(0, device_count=device_count) as ctx:
        # before swr_target_set
        assert code_of(swr, lambda: ctx.read_color_resolved(2, out=np.zeros((4, 4, 4), np.uint8), resolve=resolve_of(swr, 2))) == NO_SCENE
        assert code_of(swr, lambda: ctx.read_depth_resolved(2, out=np.zeros((4, 4), np.float32), resolve=resolve_of(swr, 2))) == NO_SCENE
        ctx.scene_upload(v, i)
        ctx.target_set(64, 40)
        ctx.draw(IDENT, DT)
        c, d = np.zeros((40, 64, 4), np.uint8), np.zeros((40, 64), np.float32)
        # NULL arguments on a live context
        r = resolve_of(swr, 2)
        assert L.swr_read_color_resolved(ctx._h, None, c.ctypes.data) == BAD_ARG
        assert L.swr_read_color_resolved(ctx._h, ctypes.byref(r), None) == BAD_ARG
        assert L.swr_read_depth_resolved(ctx._h, None, d.ctypes.data) == BAD_ARG
        assert L.swr_read_depth_resolved(ctx._h, ctypes.byref(r), None) == BAD_ARG
        assert L.swr_render_resolved(ctx._h, None, ctypes.byref(r)) == BAD_ARG
        assert L.swr_render_resolved(ctx._h, ctypes.byref(swr.binding.RenderPass()), None) == BAD_ARG
        # the structure
        for bad in (resolve_of(swr, 0), resolve_of(swr, 3), resolve_of(swr, 8), resolve_of(swr, -2), resolve_of(swr, 2, 2),
                    resolve_of(swr, 2, -1), resolve_of(swr, 2, 0, (1, 0)), resolve_of(swr, 4, 1, (0, 9)), resolve_of(swr, 1, 5)):
            assert code_of(swr, lambda: ctx.read_color_resolved(0, out=c, resolve=bad)) == BAD_ARG
            assert code_of(swr, lambda: ctx.read_depth_resolved(0, out=d, resolve=bad)) == BAD_ARG
        for bad in ((3, 0), (0, 0), (2, 7)):
            assert code_of(swr, lambda: ctx.render_resolved(v, i, IDENT, 16, 8, DT, factor=bad[0], depth_filter=bad[1])) == BAD_ARG
        # W or H not a multiple of S
        ctx.target_set(66, 40)
        assert code_of(swr, lambda: ctx.read_color_resolved(4, out=c, resolve=resolve_of(swr, 4))) == BAD_ARG
        assert code_of(swr, lambda: ctx.read_depth_resolved(4, out=d, resolve=resolve_of(swr, 4))) == BAD_ARG
        ctx.read_color_resolved(2)
        ctx.target_set(64, 42)
        assert code_of(swr, lambda: ctx.read_depth_resolved(4, out=d, resolve=resolve_of(swr, 4, 1))) == BAD_ARG
        ctx.read_depth_resolved(2, 1)
        ctx.target_set(63, 41)
        assert code_of(swr, lambda: ctx.read_color_resolved(2, out=c, resolve=resolve_of(swr, 2))) == BAD_ARG
        ctx.read_color_resolved(1)
        # the load action has no meaning at another resolution
        c0, d0 = np.zeros((8, 16, 4), np.uint8), np.zeros((8, 16), np.float32)
        assert code_of(swr, lambda: ctx.render_resolved(v, i, IDENT, 16, 8, DT | LOAD, color=c0, depth=d0, factor=2)) == UNSUPPORTED
        assert code_of(swr, lambda: ctx.render_resolved(v, i, IDENT, 16, 8, DT | LOAD | NC, depth=d0, factor=4)) == UNSUPPORTED
        # ... and what swr_render refuses is refused alike: unknown flag bits, a NULL depth image
        assert code_of(swr, lambda: ctx.render_resolved(v, i, IDENT, 16, 8, 1 << 9, factor=2)) == BAD_ARG
        assert code_of(swr, lambda: ctx.render_resolved(v, i, IDENT, 16, 8, 1 << 13, factor=2)) == BAD_ARG
        ctx.render_resolved(v, i, IDENT, 16, 8, DT, factor=2)


@gpu
def test_failed_context_returns_its_sticky_error(swr):
    v, i = small_scene()
    ctx = swr.Context(0, wait_budget_ms=300)
    try:
        ctx.scene_upload(v, i)
        ctx.target_set(64, 40)
        ctx.draw(IDENT, DT)
        ctx.sync()
        ctx.debug_fault(swr.binding.FAULT_ENQUEUE)      # the next frame's raster share fails as if a launch had returned an error
        try:
            ctx.draw(IDENT, DT)
        except swr.SwrError as e:
            assert e.code == HIP
        assert code_of(swr, lambda: ctx.read_color_resolved(2)) == HIP
        assert code_of(swr, lambda: ctx.read_depth_resolved(2, 1)) == HIP
        assert code_of(swr, lambda: ctx.render_resolved(v, i, IDENT, 16, 8, DT, factor=2)) == HIP
    finally:
        ctx.close()
