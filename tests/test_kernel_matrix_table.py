"""The kernel matrix cannot rot (CPU): the rows of tests/kernel_matrix.py are exactly the kernels the dispatch can launch, and the
expectation helpers hold the identities include/swr.h states."""
import os
import re

import numpy as np
import pytest

import kernel_matrix as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_kernels.hip")


def _body(src, start, end):
    a = src.index(start)
    return src[a:src.index(end, a)]


def dispatch_kernels(src):
    """The kernels launch_raster_t<LOAD, IDS> (LOAD and IDS expanded to false / true, the SWR_ABLATION block skipped) and
    launch_bin (its SWR_BIN_GOL / SWR_BIN_GO2 calls expanded) can launch, template arguments as written."""
    raster = _body(src, "static bool launch_raster_t(", "\nbool launch_raster(")
    raster = re.sub(r"#ifdef SWR_ABLATION.*?#endif", "", raster, flags=re.S)
    out = set()
    for k in re.findall(r"SWR_LAUNCH\(\s*stop\s*,\s*\(?\s*(k_\w+<[^>]*>)", raster):
        for load in ("false", "true"):
            for ids in ("false", "true"):
                out.add(re.sub(r"\bIDS\b", ids, re.sub(r"\bLOAD\b", load, k)))
    binning = _body(src, "bool launch_bin(", "\nvoid launch_scan(")
    for macro, params, kernel in re.findall(r"#define (SWR_BIN_GO\w*)\(([^)]*)\)\s*SWR_LAUNCH\(\s*stop\s*,\s*\((k_bin<[^>]*>)\)",
                                            binning):
        names = [p.strip() for p in params.split(",")]
        for args in re.findall(re.escape(macro) + r"\(([^)]*)\);", binning):
            k = kernel
            for p, a in zip(names, [x.strip() for x in args.split(",")]):
                k = re.sub(r"\b%s\b" % p, a, k)
            out.add(k)
    return out


def test_rows_are_the_dispatch():
    with open(KERNELS) as f:
        src = f.read()
    found = dispatch_kernels(src)
    rows = [r.name for r in K.ROWS]
    assert len(rows) == len(set(rows))
    assert set(rows) == found, (f"in the dispatch without a row: {sorted(found - set(rows))}; "
                                f"rows the dispatch does not launch: {sorted(set(rows) - found)}")
    assert len([n for n in rows if n.startswith("k_bin<")]) == 16 and len(rows) == 62 + 16


def test_the_parser_sees_a_new_variant():
    with open(KERNELS) as f:
        src = f.read()
    fake = "SWR_LAUNCH(stop, (k_raster<true, 0, false, true, false, LOAD, IDS, true>), dim3(tiles), dim3(RASTER_THREADS), 0, s, a);"
    at = src.index("        else if (a.color) SWR_LAUNCH(stop, (k_raster<true, 0, false, true, false")
    grown = dispatch_kernels(src[:at] + "        " + fake + "\n" + src[at:])
    assert len(grown - dispatch_kernels(src)) == 4
    at = src.index("#undef SWR_BIN_GO2")
    grown = dispatch_kernels(src[:at] + "        SWR_BIN_GO2(true, true, 7);\n" + src[at:])
    assert grown - dispatch_kernels(src) == {"k_bin<256, true, true, 7>"}


def _dispatch_model(flags, shader, ntri, k32=True):
    """Which raster kernel launch_raster_t picks for a frame (the rows' frames are checked against this; the kernel trace of
    tests/test_kernel_matrix.py against the rows)."""
    L, I = K._b(flags & K.LOAD), K._b(flags & K.IDS)
    plain = ntri >= (1 << K.PRIM_BITS) + (0 if flags & K.LOAD else 1)
    color = not flags & K.NC
    ext = shader != 0 and color
    if flags & K.METAL:
        if ext:
            return f"k_raster_ext<true, true, {K._b(plain)}, {L}, {I}>"
        return f"k_raster<true, 0, true, {K._b(color)}, {K._b(color and plain)}, {L}, {I}>"
    z = K._b(flags & K.DT)
    if ext:
        return f"k_raster_ext<{z}, false, {K._b(plain)}, {L}, {I}>"
    if flags & K.DT and not color and not flags & K.IDS and k32:
        return f"k_raster_depth<{L}>"
    return f"k_raster<{z}, 0, false, {K._b(color)}, {K._b(color and plain)}, {L}, {I}>"


def test_every_row_frame_reaches_its_kernel():
    n = {"visible": 6000, "padded": K.PADDED_TRIANGLES}
    for r in K.ROWS:
        if r.name.startswith("k_bin<"):
            continue
        k32 = dict(r.hooks).get(K.DEBUG_DEPTH_KEYS32, 1) != 0
        for s in r.scenes:
            got = _dispatch_model(r.flags, r.shader, n[s], k32)
            assert got == r.name, (r.name, s, got)


# ---- the helpers against the header's identities ---------------------------------------------------------------------------------
def _soups(swr, w, h):
    S = swr.scenes
    a = S.random_soup(700, w, h, 0xA1, r_ndc=0.15, margin=1.1)
    b = S.random_soup(700, w, h, 0xB2, r_ndc=0.15, margin=1.1)
    vb = np.concatenate([a.vertices[:300].copy(), b.vertices])         # B starts with A's first 100 triangles: exact ties
    vb[:300, 4:7] = vb[:300, 4:7][::-1]
    return (a.vertices, a.indices, S.app_transform(0.3, scale=1.2)), (vb, np.arange(vb.shape[0], dtype=np.int64),
                                                                      S.app_transform(0.3, scale=1.2))


@pytest.mark.parametrize("flags", [K.DT, 0, K.METAL, K.DT | K.NC], ids=["ztest", "painter", "metal", "depth_only"])
def test_load_rule_composes_like_the_header_says(swr, oracle, flags):
    """The load rule over A's clear frame, then B, is the clear frame of A || B pre-transformed — colour, depth and IDs."""
    w, h = 320, 192
    (va, ia, ma), (vb, ib, mb) = _soups(swr, w, h)
    ea = K.expected_frame(oracle, va, ia, ma, w, h, flags)
    start = (np.zeros((h, w, 4), np.uint8) if ea.color is None else ea.color, ea.depth)
    eb = K.expected_frame(oracle, vb, ib, mb, w, h, flags | K.LOAD, start=start)
    v, i = K.concat(np.concatenate([va, vb]), np.concatenate([ia, ib + va.shape[0]]), [(0, ia.size + ib.size, ma)])
    both = K.expected_frame(oracle, v, i, K.IDENT, w, h, flags)
    assert eb.depth.tobytes() == both.depth.tobytes()
    if not flags & K.NC:
        assert np.array_equal(eb.color, both.color)
    na = ia.size // 3
    want = np.where(both.ids == K.LIVE, K.LIVE, np.where((both.ids != K.NONE) & (both.ids >= na), both.ids - na, K.NONE))
    check = (want != K.LIVE) & (eb.ids != K.LIVE)
    assert np.array_equal(eb.ids[check], want[check])
    assert (eb.ids[check] == K.NONE).sum() > 500 and (eb.ids[check] != K.NONE).sum() > 500
    if flags & (K.DT | K.METAL):
        ties = np.isin(both.ids, np.arange(100)) & (eb.ids == K.NONE)      # A's triangle kept on an exact tie with B's copy
        assert ties.sum() > 100


def test_load_rule_on_special_depths():
    d0 = np.array([[np.nan, -np.inf, 0.0, -0.0, 1e-45, -1e-45, np.inf, 0.5]], np.float32)
    db = np.array([[0.1, -1e30, -0.0, 0.0, 0.0, -1e-45, 1e30, 0.5]], np.float32)
    c0 = np.zeros((1, 8, 4), np.uint8)
    cb = np.full((1, 8, 4), 255, np.uint8)
    c, d = K.load_rule(c0, d0, cb, db, K.DT)
    assert d.view(np.uint32).tolist() == np.array([[np.nan, -np.inf, 0.0, -0.0, 0.0, -1e-45, 1e30, 0.5]],
                                                  np.float32).view(np.uint32).tolist()
    assert d.view(np.uint32)[0, 0] == d0.view(np.uint32)[0, 0]
    assert (c[0, :, 3] == [0, 0, 0, 0, 255, 0, 255, 0]).all()
    c, d = K.load_rule(c0, d0, cb, db, 0)
    assert d.tobytes() == d0.tobytes() and (c == 255).all()


def test_ids_above_2_20_decode(swr, oracle):
    """The coded copies of a scene of 2^20 + 1 triangles give the last triangle, number 2^20, where it is visible."""
    w, h = K.TARGETS["small"]
    vs = K.visible_set(w, h)
    v, i, first = K.padded(vs.vertices, vs.indices, vs.n_head, K.PADDED_TRIANGLES)
    last = (1 << K.PRIM_BITS)
    for flags in (K.DT, 0, K.METAL):
        rid = K.expected_ids(oracle, v, i, K.IDENT, w, h, flags)
        assert (rid == last).sum() > 500, flags
        assert (rid[(rid >= 0) & (rid != K.NONE)] >= first).any()
        ys, xs = np.nonzero(rid == last)
        # the last triangle (tests/kernel_matrix.py: visible_set) is the one nearest to the viewer: it owns the pixels around its
        # centroid under every rule
        cy, cx = int(round(np.mean(ys))), int(round(np.mean(xs)))
        assert rid[cy, cx] == last


def test_cull_filter_worked_example(swr, oracle):
    """include/swr.h: NDC (-0.5,-0.5), (0.5,-0.5), (0,0.5) is counter-clockwise as displayed, A = -W*H/4."""
    w, h = 640, 360
    v = swr.scenes.pack_vertices(np.array([[-0.5, -0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.5, 0.5]], np.float32),
                                 np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32))
    i = np.arange(3, dtype=np.int64)
    for rules in (0, K.METAL):
        area = K.signed_areas(oracle, v, i, K.IDENT, w, h, rules)
        assert area.tolist() == [-w * h // 4]
        for cull, kept in ((K.CB, 0), (K.CB | K.CCW, 1), (K.CF, 1), (K.CF | K.CCW, 0), (K.CB | K.CF, 0), (0, 1)):
            assert K.kept_triangles(area, cull).size == kept, cull
        mirrored = K.signed_areas(oracle, v, i, K.mirrored(K.IDENT), w, h, rules)
        assert mirrored.tolist() == [w * h // 4]
    # the integer vertices: truncated (CPU rules) or rounded half away from zero first (Metal rules); A == 0 is never culled
    px = np.array([[10.6, 10.2], [20.2, 10.2], [10.6, 20.7], [30.5, 40.5], [50.5, 40.5], [40.5, 40.5]])
    x, y = swr.scenes.pixel_to_ndc(px[:, 0], px[:, 1], w, h)
    v = swr.scenes.pack_vertices(np.stack([x, y, np.full(6, 0.5)], axis=-1).astype(np.float32), np.ones((6, 3), np.float32))
    i = np.arange(6, dtype=np.int64)
    assert K.signed_areas(oracle, v, i, K.IDENT, w, h, 0).tolist() == [100, 0]
    assert K.signed_areas(oracle, v, i, K.IDENT, w, h, K.METAL).tolist() == [99, 0]
    for cull in (K.CB, K.CF, K.CB | K.CF, K.CB | K.CCW, K.CF | K.CCW, K.CB | K.CF | K.CCW):
        assert 1 in K.kept_triangles(np.array([100, 0]), cull), cull
