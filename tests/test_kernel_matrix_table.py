"""The kernel matrix cannot rot (CPU): the rows of tests/kernel_matrix.py are exactly the kernels the dispatch can launch, and the
expectation helpers hold the identities include/swr.h states."""
import itertools
import os
import re

import numpy as np
import pytest

import kernel_matrix as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_kernels.hip")
RESOLVE = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_resolve.hip")


def _body(src, start, end):
    a = src.index(start)
    return src[a:src.index(end, a)]


def _code(src):
    """The source without the SWR_ABLATION block and without its comments."""
    return re.sub(r"//[^\n]*", "", re.sub(r"#ifdef SWR_ABLATION.*?#endif", "", src, flags=re.S))


def _block_end(text, at):
    """The index behind the brace that closes the one opened at text[at]."""
    depth = 0
    for i in range(at, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return i + 1
    raise ValueError("unbalanced braces")


def kernels_named(code):
    """Every kernel a piece of launch code names (k_name or k_name<...>), template arguments as written.  The lifter: in the generic
    lambda handed to with_bools, a template argument that is one of the lambda's `auto NAME` parameters is expanded to false and
    true, since with_bools instantiates the lambda's body for both."""
    lifted = []
    for m in re.finditer(r"\bwith_bools\(\s*\[[^\]]*\]\s*\(([^)]*)\)[^{;]*\{", code):
        lifted.append((m.end() - 1, _block_end(code, m.end() - 1), re.findall(r"\bauto\s+(\w+)", m.group(1))))
    out = set()
    for m in re.finditer(r"\bk_\w+\b(?:<[^<>;]*>)?", code):
        names = [n for a, b, ns in lifted if a <= m.start() < b for n in ns if re.search(r"\b%s\b" % n, m.group(0))]
        for values in itertools.product(("false", "true"), repeat=len(names)):
            k = m.group(0)
            for n, v in zip(names, values):
                k = re.sub(r"\b%s\b" % n, v, k)
            out.add(k)
    return out


def dispatch_kernels(src):
    """The kernels launch_raster_keys (the SWR_ABLATION block skipped) and launch_bin (with bin_kernel, which holds its k_bin
    template-id) can launch."""
    code = _code(src)
    return (kernels_named(_body(code, "static bool launch_raster_keys(", "\nbool launch_raster("))
            | kernels_named(_body(code, "static BinKernel bin_kernel(", "\n}\n"))
            | kernels_named(_body(code, "bool launch_bin(", "\nvoid launch_scan(")))


def blend_kernels(src):
    """The kernels launch_raster_blend can launch."""
    return kernels_named(_body(_code(src), "static bool launch_raster_blend(", "\nstatic bool launch_raster_keys("))


def canonical(name, src):
    """A template-id without the trailing arguments that repeat the defaults of the kernel's declaration (the rows write k_bin's
    LIST only where it is true)."""
    m = re.fullmatch(r"(k_\w+)<(.*)>", name)
    if not m:
        return name
    at = src.index("void %s(" % m.group(1))
    decl = src[src.rindex("template <", 0, at):at]
    params = [p.partition("=")[2].strip() or None for p in decl[len("template <"):decl.index(">")].split(",")]
    args = [a.strip() for a in m.group(2).split(",")]
    while args and len(args) <= len(params) and params[len(args) - 1] == args[-1]:
        args.pop()
    return "%s<%s>" % (m.group(1), ", ".join(args))


def resolve_kernels(src):
    """The kernels launch_resolve can launch: launch_resolve_sf<S, DF>'s launches with the S and DF of every call."""
    sf = _body(src, "void launch_resolve_sf(", "\n}  // namespace")
    templates = re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*(k_\w+<[^>]*>)", sf)
    calls = re.findall(r"launch_resolve_sf<\s*(\w+)\s*,\s*(\w+)\s*>\(", _body(src, "void launch_resolve(", "\n}  // namespace swr"))
    return {re.sub(r"\bDF\b", df, re.sub(r"\bS\b", S, k)) for S, df in calls for k in templates}


def test_blend_and_resolve_rows_are_the_dispatch():
    with open(KERNELS) as f:
        found = blend_kernels(f.read())
    rows = [r.name for r in K.BLEND_ROWS]
    assert len(rows) == len(set(rows)) == 7 and set(rows) == found, (sorted(found - set(rows)), sorted(set(rows) - found))
    with open(RESOLVE) as f:
        found = resolve_kernels(f.read())
    rows = [r.name for r in K.RESOLVE_ROWS]
    assert len(rows) == len(set(rows)) == 10 and set(rows) == found, (sorted(found - set(rows)), sorted(set(rows) - found))
    assert not set(r.name for r in K.ROWS) & (set(r.name for r in K.BLEND_ROWS) | set(rows))


def test_the_blend_and_resolve_parsers_see_a_new_variant():
    with open(KERNELS) as f:
        src = f.read()
    at = src.index("        return go(k_raster_blend<ZTEST, false, LOAD>);")
    grown = blend_kernels(src[:at] + "        if (f.nitems) return go(k_raster_blend<false, true, LOAD>);\n" + src[at:])
    assert grown - blend_kernels(src) == {"k_raster_blend<false, true, true>", "k_raster_blend<false, true, false>"}
    at = src.index("    return with_bools([&](auto ZTEST, auto LOAD) {\n        const auto go = [&](auto kernel) { return launch_on(stop, kernel, dim3(ntiles)")
    grown = blend_kernels(src[:at] + "    hipLaunchKernelGGL(k_blend_merge, dim3(ntiles), dim3(256), 0, s, a);\n" + src[at:])
    assert grown - blend_kernels(src) == {"k_blend_merge"}
    with open(RESOLVE) as f:
        src = f.read()
    at = src.index("    } else {\n        if (mn) launch_resolve_sf<4")
    grown = resolve_kernels(src[:at] + "    } else if (factor == 8) {\n        launch_resolve_sf<8, SWR_RESOLVE_DEPTH_MIN>(c, d, co, dz, w, npix, s);\n" + src[at:])
    assert grown - resolve_kernels(src) == {"k_resolve<8, SWR_RESOLVE_DEPTH_MIN, true, true>", "k_resolve<8, 0, true, false>",
                                            "k_resolve<8, SWR_RESOLVE_DEPTH_MIN, false, true>"}
    at = src.index("    else hipLaunchKernelGGL((k_resolve<S, DF, false, true>)")
    grown = resolve_kernels(src[:at] + "    else if (!w) hipLaunchKernelGGL((k_resolve<S, DF, false, false>), grid, block, 0, s, color);\n" + src[at:])
    assert len(grown - resolve_kernels(src)) == 4


def _blend_dispatch_model(flags, ntri):
    """Which kernels launch_raster_blend launches for a blend frame."""
    zt, mt = (True, True) if flags & K.METAL else ((True, False) if flags & K.DT else (False, False))
    return (["k_blend_order"] if ntri > 0 else []) + [f"k_raster_blend<{K._b(zt)}, {K._b(mt)}, {K._b(flags & K.LOAD)}>"]


def _resolve_dispatch_model(S, depth_filter, color, depth):
    """Which kernel launch_resolve launches for the images wanted (colour alone: the filter is not instantiated)."""
    df = {K.RESOLVE_SAMPLE0: "SWR_RESOLVE_DEPTH_SAMPLE0", K.RESOLVE_MIN: "SWR_RESOLVE_DEPTH_MIN"}[depth_filter]
    assert S in (2, 4) and (color or depth)
    if color and depth:
        return f"k_resolve<{S}, {df}, true, true>"
    return f"k_resolve<{S}, 0, true, false>" if color else f"k_resolve<{S}, {df}, false, true>"


def test_every_blend_and_resolve_row_reaches_its_kernel():
    for r in K.BLEND_ROWS:
        assert not r.flags & ~(K.DT | K.METAL | K.LOAD) and r.mode in (K.BLEND_OVER, K.BLEND_ADD) and 0 < r.opacity < 255
        assert r.name in _blend_dispatch_model(r.flags, 6000), r.name
    assert _blend_dispatch_model(0, 0) == ["k_raster_blend<false, false, false>"]
    seen = set()
    for r in K.RESOLVE_ROWS:
        assert _resolve_dispatch_model(r.S, r.depth_filter, r.color, r.depth) == r.name, r.name
        seen.add((r.S, r.depth_filter if r.depth else None, r.color, r.depth))
    assert len(seen) == 10


def test_rows_are_the_dispatch():
    with open(KERNELS) as f:
        src = f.read()
    found = {canonical(k, src) for k in dispatch_kernels(src)}
    rows = [r.name for r in K.ROWS]
    want = {canonical(n, src) for n in rows}
    assert len(rows) == len(set(rows)) == len(want) and len(found) == len(dispatch_kernels(src))
    assert want == found, (f"in the dispatch without a row: {sorted(found - want)}; "
                           f"rows the dispatch does not launch: {sorted(want - found)}")
    assert len([n for n in rows if n.startswith("k_bin<")]) == 16 and len(rows) == 62 + 16


def test_the_parser_sees_a_new_variant():
    with open(KERNELS) as f:
        src = f.read()
    fake = "if (c.color) return go(k_raster<true, 0, false, true, false, LOAD, IDS, true>);"
    at = src.index("        if (c.k32) return go(k_raster_depth<LOAD>);")
    grown = dispatch_kernels(src[:at] + "        " + fake + "\n" + src[at:])
    assert len(grown - dispatch_kernels(src)) == 4
    at = src.index("    return launch_on(stop, bin_kernel(")
    grown = dispatch_kernels(src[:at] + "    if (aff) return launch_on(stop, k_bin<256, true, true, 7>, dim3(f.plan.G), dim3(256), lds, s, b);\n"
                             + src[at:])
    assert grown - dispatch_kernels(src) == {"k_bin<256, true, true, 7>"}
    assert canonical("k_bin<256, true, true, 7>", src) == "k_bin<256, true, true, 7>"
    at = src.index("k_bin<256, MT, DEFER, AFF, LIST>; }")
    grown = dispatch_kernels(src[:at] + "k_bin<256, MT, DEFER, AFF, LIST, MT>; }" + src[at + len("k_bin<256, MT, DEFER, AFF, LIST>; }"):])
    assert len(grown - dispatch_kernels(src)) == 16


def _dispatch_model(flags, shader, ntri, k32=True):
    """Which raster kernel launch_raster_keys picks for a frame (the rows' frames are checked against this; the kernel trace of
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
