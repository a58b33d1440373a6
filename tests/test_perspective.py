"""Perspective-correct interpolation (SWR_FLAG_PERSPECTIVE; include/swr.h "Perspective-correct interpolation").

Expected colour comes from a NumPy model written here from the header's definition: the structure of oracle/swr_oracle_np.py's
render / render_metal (coverage, screen weights, z-test, quantisation; its fragment stage `_shaded` imported) with colour and the
varyings interpolated with the corrected weights p = (w0 q_a, w1 q_b, w2 q_c) / s, s = (u0 + u1) + u2, in float32, one rounding per
operation.  Depth and IDs must be bit for bit those of the same frame without the flag.  Depth-clip fans come from the clipper of
tests/test_depth_clip.py, whose polygons carry w.  Every test sets the flag, so a library without the feature fails all of them with
SWR_ERR_BAD_ARG.
"""
import dataclasses

import numpy as np
import pytest

from oracle.swr_oracle_np import _shaded, interpolate, quantise
from tests.test_depth_clip import clip_space, restate, straddling_soup

pytestmark = pytest.mark.gpu

DT, NC, METAL, REAL_LINES, LOAD, IDS = 1, 2, 4, 8, 16, 32
CB, CLIP, PERSP = 64, 1024, 2048
NONE = 0xFFFFFFFF
W, H = 320, 192
f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(16)
RULES = {"painter": 0, "ztest": DT, "metal": METAL}


# ---- the model -------------------------------------------------------------------------------------------------------------------
def persp(w0, w1, w2, rw):
    """The header's correction: screen weights -> the weights colour and varyings are interpolated with."""
    ra, rb, rc = (f32(x) for x in rw)
    if ra == rb and rb == rc:
        return w0, w1, w2
    qa, qb, qc = f32(1.0) / ra, f32(1.0) / rb, f32(1.0) / rc
    u0, u1, u2 = w0 * qa, w1 * qb, w2 * qc
    s = (u0 + u1) + u2
    rs = f32(1.0) / s
    return u0 * rs, u1 * rs, u2 * rs


def model(v, i, ms, w, h, flags, shading=None, start=None, rw=None, cull_back=False, correct=True):
    """(colour, depth) of a frame: v [nv, 8], i indices, ms one matrix or one per triangle, start = (colour, depth) of a load frame,
    rw [ntri, 3] the corners' w when they are not the transform's own (depth-clip fans)."""
    metal = bool(flags & METAL)
    ztest = bool(flags & (DT | METAL))
    color = np.zeros((h, w, 4), dtype=np.uint8) if start is None else np.array(start[0], copy=True)
    depth = np.full((h, w), np.inf, dtype=f32) if start is None else np.array(start[1], copy=True)
    V = np.asarray(v, dtype=f32).reshape(-1, 8)
    idx = np.asarray(i, dtype=np.int64).reshape(-1, 3)
    many = np.asarray(ms).size != 16
    A = None if shading is None or shading.shader == 0 else np.asarray(shading.attrs, dtype=f32).reshape(-1, 8)
    cache = {}
    with np.errstate(all="ignore"):
        for p, tri in enumerate(idx):
            m = ms[p] if many else ms
            if id(m) not in cache:
                cache[id(m)] = clip_space(V, m)
            r = cache[id(m)][tri]                                           # [3, 4]
            ws = r[:, 3] if rw is None else np.asarray(rw[p], dtype=f32)
            ndc = r[:, :3] / r[:, 3:4]
            sx = (ndc[:, 0] * f32(0.5) + f32(0.5)) * f32(w)
            sy = (ndc[:, 1] * f32(-0.5) + f32(0.5)) * f32(h)
            col = [V[k, 4:7] for k in tri]
            if metal:
                px = np.trunc(sx + np.copysign(f32(0.5), sx))
                py = np.trunc(sy + np.copysign(f32(0.5), sy))
                if not ((px >= 0) & (px < 2.0 ** 30) & (py >= 0) & (py < 2.0 ** 30)).all():
                    continue
                xs, ys = [int(q) for q in px], [int(q) for q in py]
            else:
                if not ((np.abs(sx) < f32(2.0 ** 30)) & (np.abs(sy) < f32(2.0 ** 30))).all():
                    continue
                xs, ys = [int(q) for q in sx], [int(q) for q in sy]
            if cull_back:
                area = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (xs[2] - xs[0]) * (ys[1] - ys[0])
                if area < 0:
                    continue
            sel_attr = None if A is None else [A[k] for k in tri]
            if metal:
                if min(xs) == 0 or min(ys) == 0:
                    continue
                (p1x, p2x, p3x), (p1y, p2y, p3y) = [f32(q) for q in xs], [f32(q) for q in ys]
                divider = (p1x - p3x) * (p2y - p3y) - (p2x - p3x) * (p1y - p3y)
                x0, x1, y0, y1 = min(xs), min(max(xs), w - 1), min(ys), min(max(ys), h - 1)
                if x0 > x1 or y0 > y1:
                    continue
                gx = (np.arange(x0, x1 + 1).astype(f32) + f32(0.5))[None, :]
                gy = (np.arange(y0, y1 + 1).astype(f32) + f32(0.5))[:, None]
                w0 = ((p2y - p3y) * (gx - p3x) + (p3x - p2x) * (gy - p3y)) / divider
                w1 = ((p3y - p1y) * (gx - p3x) + (p1x - p3x) * (gy - p3y)) / divider
                w2 = f32(1.0) - w0 - w1
                inside = (w0 >= 0) & (w0 <= 1) & (w1 >= 0) & (w1 <= 1) & (w2 >= 0) & (w2 <= 1)
                z = w0 * ndc[0, 2] + w1 * ndc[1, 2] + w2 * ndc[2, 2]
                sub = depth[y0:y1 + 1, x0:x1 + 1]
                win = inside & (z < sub)
                sub[win] = z[win]
                if flags & NC:
                    continue
                c0, c1, c2 = persp(w0, w1, w2, ws) if correct else (w0, w1, w2)
                rgb = [c0 * col[0][ch] + c1 * col[1][ch] + c2 * col[2][ch] for ch in range(3)]
                alpha = np.full(z.shape, f32(1.0), dtype=f32)
                if sel_attr is not None:
                    rgb, alpha = _shaded(shading, sel_attr, c0, c1, c2, rgb, True)
                un = lambda a: np.rint(np.fmin(np.fmax(a, f32(0)), f32(1)) * f32(255)).astype(np.uint8)
                px4 = np.stack([un(rgb[2]), un(rgb[1]), un(rgb[0]), un(alpha)], axis=-1)
                color[y0:y1 + 1, x0:x1 + 1][win] = px4[win]
                continue
            ints = list(zip(xs, ys))
            a, b, c = ints
            cf = (f32(c[0]) + f32(0.5), f32(c[1]) + f32(0.5))
            col0 = ((f32(a[0]) + f32(0.5)) - cf[0], (f32(a[1]) + f32(0.5)) - cf[1])
            col1 = ((f32(b[0]) + f32(0.5)) - cf[0], (f32(b[1]) + f32(0.5)) - cf[1])
            det = col0[0] * col1[1] - col1[0] * col0[1]
            T = ((col1[1] / det, -col1[0] / det), (-col0[1] / det, col0[0] / det))
            order = sorted(range(3), key=lambda k: sy[k])
            S = [ints[k] for k in order]
            for y in range(max(S[0][1], 0), min(S[2][1], h - 1) + 1):
                lx = interpolate([S[0], S[1], S[2]], y)
                rx = interpolate([S[0], S[2]], y)
                if lx > rx:
                    lx, rx = rx, lx
                x0, x1 = max(lx, 0), min(rx, w - 1)
                if x0 > x1:
                    continue
                gx = np.arange(x0, x1 + 1)
                dx = (gx.astype(f32) + f32(0.5)) - cf[0]
                dy = (f32(y) + f32(0.5)) - cf[1]
                w0 = T[0][0] * dx + T[0][1] * dy
                w1 = T[1][0] * dx + T[1][1] * dy
                w2 = f32(1.0) - w0 - w1
                sel = np.ones(gx.shape, dtype=bool)
                if ztest:
                    d = ndc[0, 2] * w0 + ndc[1, 2] * w1 + ndc[2, 2] * w2
                    sel = d < depth[y, x0:x1 + 1]
                    depth[y, x0:x1 + 1][sel] = d[sel]
                if flags & NC:
                    continue
                c0, c1, c2 = persp(w0, w1, w2, ws) if correct else (w0, w1, w2)
                rgb = [col[0][ch] * c0 + col[1][ch] * c1 + col[2][ch] * c2 for ch in range(3)]
                alpha = np.full(gx.shape, f32(1.0), dtype=f32)
                if sel_attr is not None:
                    rgb, alpha = _shaded(shading, sel_attr, c0, c1, c2, rgb, False)
                px = np.stack([quantise(rgb[2]), quantise(rgb[1]), quantise(rgb[0]), quantise(alpha)], axis=-1)
                color[y, x0:x1 + 1][sel] = px[sel]
    return color, depth


# ---- scenes and helpers ----------------------------------------------------------------------------------------------------------
def perspective(fy=1.2, aspect=W / H, near=0.5, far=6.0):
    """A [0, 1]-depth perspective looking down +z: w = z_eye."""
    a = far / (far - near)
    m = np.zeros((4, 4), dtype=np.float64)       # rows = output, columns = input
    m[0, 0], m[1, 1] = fy / aspect, fy
    m[2, 2], m[2, 3] = a, -near * a
    m[3, 2] = 1.0
    return np.ascontiguousarray(m.astype(f32).T).reshape(16)


def soup(n, seed, z_lo=1.0, z_hi=5.0, r=0.7):
    """Random triangles in front of the eye, with a few exact depth ties."""
    v, i = straddling_soup(n, seed, z_lo=z_lo, z_hi=z_hi, r=r)
    v[3:30:9] = v[0:27:9]                        # (some shared corners: exact ties)
    return v, i


def torus(swr):
    S = swr.scenes
    xyz, rgb, i = S.torus_mesh(48, 24, 0.6, 0.25)
    return S.pack_vertices(xyz, rgb), i, S.torus_attrs(48, 24)


def shading_for(swr, nv, shader, seed=0x51):
    if shader == 0:
        return None
    return swr.scenes.random_shading(nv, seed, shader, shininess_log2=3)


def frame(ctx, m, flags, items=None):
    if items is None:
        ctx.draw(m, flags)
    else:
        ctx.draw_list(items, flags)
    ctx.sync()
    c = None if flags & NC else ctx.read_color()
    d = ctx.read_depth()
    ids = ctx.read_ids() if flags & IDS else None
    return c, d, ids


def check(got, want_c, what, ref=None):
    """got = (colour, depth, ids) of the frame with the flag; want_c the model's colour; ref the same frame without the flag."""
    c, d, ids = got
    if want_c is not None:
        bad = np.nonzero((c != want_c).any(axis=-1))
        assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): " \
                                 f"{c[bad[0][0], bad[1][0]]} vs {want_c[bad[0][0], bad[1][0]]}"
    if ref is not None:
        assert d.tobytes() == ref[1].tobytes(), f"{what}: depth differs from the frame without the flag"
        if ids is not None:
            assert np.array_equal(ids, ref[2]), f"{what}: IDs differ from the frame without the flag"


def start_images(seed, w=W, h=H):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    d = rng.uniform(0.3, 1.2, (h, w)).astype(f32)
    d[::7, ::5] = np.inf
    return c, d


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------
# eye space (X, Y, Z) with w = Z: x_ndc = X / Z, y_ndc = Y / Z, z_ndc = 0.5
WZ = np.ascontiguousarray(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.5, 0], [0, 0, 1, 0]], dtype=f32).T).reshape(16)


def vtx(X, Y, Z, rgb):
    return [X, Y, Z, 0.0, *rgb, 0.0]


def test_known_answer_edge(swr):
    """a = (-0.5, -0.5) at w = 1 (red), b = (0.5, -0.5) at w = 3 (black), c = (0, 0.5) at w = 1 (black); 256 x 256.
    Screen: a = (64, 192), b = (192, 192), c = (128, 64).  Pixel (127, 191), centre (127.5, 191.5), lies next to the edge ab,
    halfway along it in screen space.  T() (cf = c + 0.5, det = -16384): w_a = 129/256 = 0.50390625, w_b = 125/256 = 0.48828125,
    w_c = 2/256 = 0.0078125 (all exact).  Affine red = 0.50390625 * 255 = 128.5 -> 128.  Perspective: u = (129/256, 125/768,
    2/256), s = 0.6744791..., p_a = 0.7471042 -> red = 190.51 -> 190."""
    v = np.array([vtx(-0.5, -0.5, 1.0, (1, 0, 0)), vtx(1.5, -1.5, 3.0, (0, 0, 0)), vtx(0.0, 0.5, 1.0, (0, 0, 0))], dtype=f32)
    i = np.arange(3, dtype=np.int64)
    # hand derivation of the weights at (127, 191): T() of a = (64, 192), b = (192, 192), c = (128, 64) (cf = c + 0.5)
    dx, dy = f32(127.5) - f32(128.5), f32(191.5) - f32(64.5)
    col0, col1 = (f32(-64.0), f32(128.0)), (f32(64.0), f32(128.0))
    det = col0[0] * col1[1] - col1[0] * col0[1]                 # -16384
    w0 = (col1[1] / det) * dx + (-col1[0] / det) * dy            # 0.5
    w1 = (-col0[1] / det) * dx + (col0[0] / det) * dy            # 0.49609375
    w2 = f32(1) - w0 - w1                                        # 0.00390625
    assert (w0, w1, w2) == (f32(0.50390625), f32(0.48828125), f32(0.0078125))
    p0 = persp(w0, w1, w2, (1.0, 3.0, 1.0))[0]
    assert int(p0 * f32(255)) == 190
    with swr.Context(0) as ctx:
        c_lin, _ = ctx.render(v, i, WZ, 256, 256, 0)
        c, d = ctx.render(v, i, WZ, 256, 256, PERSP)
        c_m, _ = ctx.render(v, i, WZ, 256, 256, METAL | PERSP)
    assert c_lin[191, 127, 2] == 128                             # (BGRA: red is byte 2)
    assert c[191, 127, 2] == 190
    assert c[191, 127, 3] == 255
    mc, _ = model(v, i, WZ, 256, 256, 0)
    assert np.array_equal(c, mc)
    mm, _ = model(v, i, WZ, 256, 256, METAL)
    assert np.array_equal(c_m, mm)


def test_known_answer_floor():
    """exercised below through the GPU; kept separate so that the hand derivation reads on its own:
    a floor y = -0.5 from Z = 1 (v = 0) to Z = 3 (v = 1), X in [-0.8, 0.8] (u 0 .. 1).  Screen row at y_ndc = -1/3 lies at Z = 1.5,
    so v = (1.5 - 1) / 2 = 0.25 there, where screen-affine interpolation gives 0.5."""
    Z = -0.5 / (-1.0 / 3.0)
    assert abs((Z - 1.0) / 2.0 - 0.25) < 1e-12


def floor_quad(z0=1.0, z1=3.0, y=-0.5, x=0.8):
    # colour: red = u (across), green = v (into the screen)
    v = np.array([vtx(-x, y, z0, (0, 0, 0)), vtx(x, y, z0, (1, 0, 0)), vtx(x, y, z1, (1, 1, 0)), vtx(-x, y, z1, (0, 1, 0))], dtype=f32)
    return v, np.array([0, 1, 2, 0, 2, 3], dtype=np.int64)


@pytest.mark.parametrize("rules", ["ztest", "metal"])
def test_known_answer_floor_gpu(swr, rules):
    v, i = floor_quad()
    n = 240                               # square, so that y_ndc = 1 - 2 (row + 0.5) / n
    flags = RULES[rules] | PERSP
    with swr.Context(0) as ctx:
        c, _ = ctx.render(v, i, WZ, n, n, flags)
        c_lin, _ = ctx.render(v, i, WZ, n, n, RULES[rules])
    row = 159                             # centre y_ndc = 1 - 2 * 159.5 / 240 = -0.329...: Z = 0.5 / 0.329 = 1.519, v = 0.2595
    y_ndc = 1.0 - 2.0 * (row + 0.5) / n
    v_exact = (-0.5 / y_ndc - 1.0) / 2.0
    g = int(c[row, n // 2, 1])
    assert abs(g - 255 * v_exact) <= 3, (g, 255 * v_exact)      # (pixel centres and truncated vertices: within 3 of 66.2)
    assert int(c_lin[row, n // 2, 1]) > 120                      # affine: about half way, 130
    mc, _ = model(v, i, WZ, n, n, RULES[rules])
    assert np.array_equal(c, mc)


# ---- 2. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("load", [False, True])
@pytest.mark.parametrize("shader", [0, 1, 2])
@pytest.mark.parametrize("rules", list(RULES))
def test_parity_soup(swr, oracle, rules, shader, load, ids):
    v, i = soup(300, 0x9E0 + shader)
    m = perspective()
    sh = shading_for(swr, v.shape[0], shader)
    flags = RULES[rules] | (LOAD if load else 0) | (IDS if ids else 0)
    start = start_images(0x5A + shader) if load else None
    want, want_d = model(v, i, m, W, H, flags, sh, start)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        if sh is not None:
            ctx.shading_set(sh)
        ctx.target_set(W, H)
        if load:
            ctx.target_write(*start)
        ref = frame(ctx, m, flags)
        if load:
            ctx.target_write(*start)
        got = frame(ctx, m, flags | PERSP)
    check(got, want, f"soup {rules} shader {shader} load {load} ids {ids}", ref)
    assert got[1].tobytes() == want_d.tobytes()                  # the model's depth is the oracle's
    # depth and IDs from the model as well (tests/frame_model.py: the C oracle's depth, colour-coded IDs), not only from the frame
    # the library draws without the flag
    import frame_model as FM
    FM.same(got, FM.expect(oracle, FM.FrameSpec(v, i, W, H, flags | PERSP, m, shading=sh), start), f"soup {rules} {shader} {load} {ids}: model")
    assert not np.array_equal(got[0], ref[0])                    # (the flag does something here)


@pytest.mark.parametrize("shader", [0, 1, 2])
@pytest.mark.parametrize("rules", list(RULES))
def test_parity_torus_app_transform(swr, oracle, rules, shader):
    v, i, attrs = torus(swr)
    m = swr.scenes.app_transform(0.7, scale=1.4)
    sh = None
    if shader:
        sh = dataclasses.replace(swr.scenes.random_shading(v.shape[0], 0x70, shader), attrs=attrs)
    flags = RULES[rules] | IDS
    want, _ = model(v, i, m, W, H, flags, sh)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        if sh is not None:
            ctx.shading_set(sh)
        ctx.target_set(W, H)
        ref = frame(ctx, m, flags)
        got = frame(ctx, m, flags | PERSP)
    check(got, want, f"torus {rules} shader {shader}", ref)
    import frame_model as FM
    FM.same(got, FM.expect(oracle, FM.FrameSpec(v, i, W, H, flags | PERSP, m, shading=sh)), f"torus {rules} shader {shader}: model")
    if rules != "painter":
        c_or, d_or, _, code = (oracle.render_metal(v, i, m, W, H, shading=sh) if rules == "metal" else
                               oracle.render(v, i, m, W, H, DT | oracle.TINV_PER_TRIANGLE, shading=sh))
        assert code == 0 and got[1].tobytes() == d_or.tobytes()


# ---- 3. identity properties ----------------------------------------------------------------------------------------------------
def rotation_scaled():
    a, s = 0.6, 0.7
    m = np.eye(4, dtype=np.float64)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = s * np.cos(a), -s * np.sin(a), s * np.sin(a), s * np.cos(a)
    m[2, 2] = 0.1
    m[0, 3] = 0.1
    return np.ascontiguousarray(m.astype(f32).T).reshape(16)


@pytest.mark.parametrize("rules", list(RULES))
def test_affine_transforms_unchanged(swr, rules):
    v, i = soup(400, 0xAF)
    v[:, 2] = v[:, 2] * f32(0.1)
    sh = shading_for(swr, v.shape[0], 2)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        for m in (IDENT, rotation_scaled()):
            for s in (None, sh):
                if s is not None:
                    ctx.shading_set(s)
                ref = frame(ctx, m, RULES[rules] | IDS)
                got = frame(ctx, m, RULES[rules] | IDS | PERSP)
                assert np.array_equal(got[0], ref[0]) and got[1].tobytes() == ref[1].tobytes() and np.array_equal(got[2], ref[2])


def test_no_color_vertices_and_lines_unchanged(swr):
    v, i = soup(300, 0xBC)
    m = perspective()
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        for flags in (DT | NC, METAL | NC):
            ref = frame(ctx, m, flags)
            got = frame(ctx, m, flags | PERSP)
            assert got[1].tobytes() == ref[1].tobytes()
        for prim, extra in ((2, 0), (1, 0), (1, REAL_LINES)):
            ctx.draw(m, DT | extra, prim); ctx.sync()
            rc, rd = ctx.read_color(), ctx.read_depth()
            ctx.draw(m, DT | extra | PERSP, prim); ctx.sync()
            assert np.array_equal(ctx.read_color(), rc) and ctx.read_depth().tobytes() == rd.tobytes(), (prim, extra)


# ---- 4. combinations ---------------------------------------------------------------------------------------------------------------
def test_draw_list_mixed_items(swr):
    v, i = soup(400, 0xD1)
    n = i.size
    pm, aff = perspective(), rotation_scaled()
    pm2 = np.array(pm, copy=True).reshape(4, 4)
    pm2[3, 0] = 0.4                      # (translated along x before the projection)
    pm2 = pm2.reshape(16)
    h = n // 2 // 3 * 3
    items = [(0, h, pm), (h, n - h, aff), (0, h, pm2), (h, n - h, pm)]     # instancing: each range under two matrices
    vi, ms = [], []
    t = np.asarray(i).reshape(-1, 3)
    for first, cnt, m in items:
        vi.append(t[first // 3:(first + cnt) // 3])
        ms += [m] * (cnt // 3)
    I = np.concatenate(vi).reshape(-1)
    sh = shading_for(swr, v.shape[0], 1)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        for flags, s in ((DT | IDS, None), (0 | IDS, None), (METAL | IDS, sh)):
            if s is not None:
                ctx.shading_set(s)
            want, _ = model(v, I, ms, W, H, flags, s)
            ref = frame(ctx, None, flags, items)
            got = frame(ctx, None, flags | PERSP, items)
            check(got, want, f"draw list {flags}", ref)
        # every item affine: bit for bit the frame without the flag
        aff_items = [(0, h, aff), (h, n - h, IDENT)]
        ref = frame(ctx, None, DT | IDS, aff_items)
        got = frame(ctx, None, DT | IDS | PERSP, aff_items)
        assert np.array_equal(got[0], ref[0]) and got[1].tobytes() == ref[1].tobytes()


@pytest.mark.parametrize("rules", ["ztest", "metal"])
def test_cull_back(swr, rules):
    v, i = soup(400, 0xCB)
    m = perspective()
    flags = RULES[rules] | IDS | CB
    want, _ = model(v, i, m, W, H, flags, cull_back=True)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ref = frame(ctx, m, flags)
        got = frame(ctx, m, flags | PERSP)
    check(got, want, f"cull back {rules}", ref)


def clip_model(v, i, m, flags, shading=None):
    attrs = shading.attrs if shading is not None else None
    V, A, I, fmap, fans = restate(v, i, m, attrs)
    rw = [(poly[0][3], poly[s][3], poly[s + 1][3]) for poly in fans for s in range(1, len(poly) - 1)]
    sh = None if shading is None else dataclasses.replace(shading, attrs=A)
    return model(V, I, IDENT, W, H, flags, sh, rw=rw)


@pytest.mark.parametrize("rules", list(RULES))
def test_depth_clip_fly_through(swr, rules):
    v, i = straddling_soup(600, 0xF1, z_lo=-1.5, z_hi=4.0, r=1.5)       # the eye inside a stretched soup
    m = perspective()
    sh = shading_for(swr, v.shape[0], 1)
    flags = RULES[rules] | IDS | CLIP
    for s in (None, sh):
        want, _ = clip_model(v, i, m, flags, s)
        with swr.Context(0) as ctx:
            ctx.scene_upload(v, i)
            if s is not None:
                ctx.shading_set(s)
            ctx.target_set(W, H)
            ref = frame(ctx, m, flags)
            got = frame(ctx, m, flags | PERSP)
        check(got, want, f"fly-through {rules} shaded {s is not None}", ref)


def test_depth_clip_textured_floor(swr):
    v, i = floor_quad(z0=-1.0, z1=5.0, x=0.15)         # (narrow: the Metal rules skip triangles reaching x < 0 on the screen)
    v[:, 4:7] = 1.0                                     # white: the colour is the texture's (unlit)
    uv = np.array([[0, 0], [4, 0], [4, 12], [0, 12]], dtype=f32)
    attrs = swr.scenes.pack_attrs(np.tile(np.array([[0, 1, 0]], dtype=f32), (4, 1)), uv)
    sh = dataclasses.replace(swr.scenes.random_shading(4, 0xF7, 2), attrs=attrs, texture=swr.scenes.checker_texture(64, 64, 3, 2),
                             ambient=1.0, diffuse=0.0, specular=0.0)
    m = perspective(near=0.2)
    for rules in ("ztest", "metal"):
        flags = RULES[rules] | CLIP
        want, _ = clip_model(v, i, m, flags, sh)
        with swr.Context(0) as ctx:
            ctx.scene_upload(v, i)
            ctx.shading_set(sh)
            ctx.target_set(W, H)
            ref = frame(ctx, m, flags)
            got = frame(ctx, m, flags | PERSP)
        check(got, want, f"textured floor {rules}", ref)
        assert not np.array_equal(got[0], ref[0])


def test_four_bands(swr):
    v, i = soup(800, 0x4B)
    m = perspective()
    want, _ = model(v, i, m, W, H, DT)
    with swr.Context(0, device_count=4) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        ref = frame(ctx, m, DT | IDS)
        got = frame(ctx, m, DT | IDS | PERSP)
    check(got, want, "4 bands", ref)


def test_render_with_and_without_scene_id(swr):
    v, i = soup(500, 0x5E)
    m = perspective()
    sh = shading_for(swr, v.shape[0], 2)
    want, want_d = model(v, i, m, W, H, DT, sh)
    with swr.Context(0) as ctx:
        for sid in (0, 7, 7):
            c, d = ctx.render(v, i, m, W, H, DT | PERSP, scene_id=sid, shading=sh)
            assert np.array_equal(c, want) and d.tobytes() == want_d.tobytes(), sid


def test_overflowed_frame_is_redrawn_with_the_flag(swr):
    S = swr.scenes
    w, h = 1280, 720
    s = S.random_soup(20000, w, h, 555, r_ndc=0.01, flags=DT, margin=1.0)
    v = s.vertices.copy()
    v[:, 0] = 0.30 + (v[:, 0] * 0.5 + 0.5) * 0.07
    v[:, 1] = 0.10 + (v[:, 1] * 0.5 + 0.5) * 0.06
    rng = np.random.default_rng(0x0F)
    zz = rng.uniform(1.0, 3.0, v.shape[0]).astype(f32)
    v[:, 0] = v[:, 0] * zz                      # eye space for w = Z: the same screen positions, varied w
    v[:, 1] = v[:, 1] * zz
    v[:, 2] = zz
    v = np.ascontiguousarray(v)
    want, _ = model(v, s.indices, WZ, w, h, DT)
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, s.indices)
        ctx.draw(WZ, DT | IDS | PERSP)           # a fresh context: its bins overflow, the frame is redrawn with its flags
        ctx.sync()
        got = (ctx.read_color(), ctx.read_depth(), ctx.read_ids())
        pairs = ctx.timings()["tile_pairs"]
        ref = frame(ctx, WZ, DT | IDS)
    assert pairs > 4 * 1024
    check(got, want, "overflowed first frame", ref)


def lifted(s, seed):
    """A screen-space soup given eye-space corners for WZ: the same NDC, w random in [1, 3]."""
    v = s.vertices.copy()
    zz = np.random.default_rng(seed).uniform(1.0, 3.0, v.shape[0]).astype(f32)
    v[:, 0], v[:, 1], v[:, 2] = v[:, 0] * zz, v[:, 1] * zz, zz
    return np.ascontiguousarray(v)


@pytest.mark.parametrize("flags,shader", [(DT, 0), (METAL, 0), (0, 0), (DT, 2)])
def test_dense_tile_more_winners_than_a_round(swr, flags, shader):
    """~1 000 entries and ~380 winners per 64 x 32 tile: more than the perspective records of one round (the per-thread path in the
    tiles beyond 4 096 entries is covered by the 2^20 test's PLAIN kernels)."""
    s = swr.scenes.random_soup(12000, 640, 64, 0x3A, r_ndc=0.05, flags=flags, margin=1.05)
    v = lifted(s, 0x3B)
    sh = shading_for(swr, v.shape[0], shader)
    want, _ = model(v, s.indices, WZ, 640, 64, flags, sh)
    with swr.Context(0) as ctx:
        c, d = ctx.render(v, s.indices, WZ, 640, 64, flags | PERSP, shading=sh)
        c0, d0 = ctx.render(v, s.indices, WZ, 640, 64, flags, shading=sh)
    check((c, d, None), want, f"dense tile {flags} {shader}", (c0, d0, None))


@pytest.mark.parametrize("flags,shader", [(DT, 0), (METAL, 1), (0, 2)])
def test_beyond_2_to_20_primitives(swr, flags, shader):
    """2^20 + 600 triangles: the colour kernels without the winner table (PLAIN).  The first 2^20 lie far outside the image."""
    far = (1 << 20)
    vis = swr.scenes.random_soup(600, W, H, 0x20, r_ndc=0.15, flags=flags, margin=1.05)
    vv = lifted(vis, 0x21)
    off = np.zeros((3 * far, 8), dtype=f32)
    off[:, 0] = 50.0
    off[:, 2] = 1.0
    v = np.ascontiguousarray(np.concatenate([off, vv]))
    i = np.arange(v.shape[0], dtype=np.int64)
    sh = shading_for(swr, v.shape[0], shader)
    sh_vis = None if sh is None else dataclasses.replace(sh, attrs=sh.attrs[3 * far:])
    want, _ = model(vv, np.arange(vv.shape[0]), WZ, W, H, flags, sh_vis)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        if sh is not None:
            ctx.shading_set(sh)
        ctx.target_set(W, H)
        ref = frame(ctx, WZ, flags | IDS)
        got = frame(ctx, WZ, flags | IDS | PERSP)
    check(got, want, f"2^20 + 600, {flags} {shader}", ref)
