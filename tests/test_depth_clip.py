"""Depth clipping (SWR_FLAG_DEPTH_CLIP; include/swr.h "Depth clipping").

Expected images come from the unchanged oracle run on the RESTATED scene: a clipper written here in numpy float32 (one rounding per
operation, no FMA) computes every vertex's clip-space position with vertex_shader's operation order, clips each triangle against
the near plane (z >= 0), then the far plane (w - z >= 0), fans the polygon and gives every fan vertex in NDC with its interpolated
colour and attributes.  That scene is drawn by the oracle with the identity transform and the other flags of the frame; IDs are
decoded from a colour-coded draw of it (the helpers of tests/test_cull.py) and mapped back through the fan-to-original map.
Every test sets the flag, so a library without the feature fails all of them with SWR_ERR_BAD_ARG.
"""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, NC, METAL, LOAD, IDS = 1, 2, 4, 16, 32
CB, CF, CCW = 64, 128, 256
CLIP = 1024
NONE = 0xFFFFFFFF
W, H = 320, 192
IDENT = np.eye(4, dtype=np.float32).T.reshape(16)
MODES = {"painter": 0, "ztest": DT, "ztest_nc": DT | NC, "metal": METAL, "metal_nc": METAL | NC}
f32 = np.float32


# ---- the clipper ------------------------------------------------------------------------------------------------------------------
def clip_space(v, m):
    """vertex_shader: r = c0 * x, + c1 * y, + c2 * z, + c3 * 1, one rounding each (float32 arrays)."""
    c = np.asarray(m, dtype=f32).reshape(4, 4)          # c[j] = column j
    p = np.asarray(v, dtype=f32).reshape(-1, 8)
    r = c[0][None, :] * p[:, 0:1]
    r = r + c[1][None, :] * p[:, 1:2]
    r = r + c[2][None, :] * p[:, 2:3]
    r = r + c[3][None, :] * f32(1.0)
    return r.astype(f32)


def _pass(poly, plane):
    d = (lambda q: q[2]) if plane == 0 else (lambda q: f32(q[3] - q[2]))
    out = []
    n = len(poly)
    for i in range(n):
        a, b = poly[i], poly[(i + 1) % n]
        da, db = d(a), d(b)
        if da >= 0:
            out.append(a)
        if (da > 0 and db < 0) or (da < 0 and db > 0):
            I, O, dI, dO = (a, b, da, db) if da > 0 else (b, a, db, da)
            t = f32(dI / f32(dI - dO))
            out.append((I + t * (O - I)).astype(f32))       # float32 array ops: one rounding each
    return out


def clip_triangle(corners):
    """corners: 3 float32[12] (x y z w r g b nx ny nz u v) -> polygon (list of float32[12]), empty when nothing is left."""
    if not all(np.isfinite(c[:4]).all() for c in corners):
        return []
    poly = _pass(list(corners), 0)
    if len(poly) < 3:
        return []
    poly = _pass(poly, 1)
    return poly if len(poly) >= 3 else []


def restate(v, i, m, attrs=None, order=None):
    """(vertices, attributes or None, index list, fan -> original map, the fans) of the restated scene.  `order`: the original
    numbers of the triangles (default 0 .. n-1); m may be one matrix, or one per triangle."""
    v = np.asarray(v, dtype=f32).reshape(-1, 8)
    t = np.asarray(i, dtype=np.int64).reshape(-1, 3)
    ms = [m] * len(t) if np.asarray(m).size == 16 else list(m)
    a = None if attrs is None else np.asarray(attrs, dtype=f32).reshape(-1, 8)
    rs = {}
    out_v, out_a, fmap, fans = [], [], [], []
    for p, tri in enumerate(t):
        key = id(ms[p])
        if key not in rs:
            rs[key] = clip_space(v, ms[p])
        r = rs[key]
        corners = []
        for k in tri:
            c = np.zeros(12, dtype=f32)
            c[0:4] = r[k]
            c[4:7] = v[k, 4:7]
            if a is not None:
                c[7:10] = a[k, 0:3]
                c[10] = a[k, 4]
                c[11] = a[k, 5]
            corners.append(c)
        poly = clip_triangle(corners)
        fans.append(poly)
        for s in range(1, len(poly) - 1):
            for q in (poly[0], poly[s], poly[s + 1]):
                vv = np.zeros(8, dtype=f32)
                with np.errstate(divide="ignore", invalid="ignore"):
                    vv[0:3] = q[0:3] / q[3]
                vv[4:7] = q[4:7]
                out_v.append(vv)
                aa = np.zeros(8, dtype=f32)
                aa[0:3] = q[7:10]
                aa[4], aa[5] = q[10], q[11]
                out_a.append(aa)
            fmap.append(p if order is None else order[p])
    nv = len(out_v)
    V = np.array(out_v, dtype=f32).reshape(-1, 8)
    A = None if a is None else np.array(out_a, dtype=f32).reshape(-1, 8)
    return V, A, np.arange(nv, dtype=np.int64), np.array(fmap, dtype=np.int64), fans


# ---- colour-coded IDs: tests/kernel_matrix.py's (shared with tests/frame_model.py) -----------------------------------------------
from kernel_matrix import LIVE, MASK21, coded, decode  # noqa: E402,F401


def oracle_frame(oracle, v, i, w, h, flags, shading=None, color=None, depth=None):
    if flags & METAL:
        c, d, _, code = oracle.render_metal(v, i, IDENT, w, h, flags & NC, color=color, depth=depth, shading=shading)
    else:
        c, d, _, code = oracle.render(v, i, IDENT, w, h, (flags & (DT | NC)) | oracle.TINV_PER_TRIANGLE, color=color, depth=depth,
                                      shading=shading)
    assert code == 0
    return c, d


def expected(oracle, v, i, m, flags, w=W, h=H, ids=False, shading=None, order=None, start=None):
    """(colour or None, depth, IDs or None, fan map) of the clip frame; start = (colour, depth) of a load frame."""
    attrs = shading.attrs if shading is not None else None
    V, A, I, fmap, _ = restate(v, i, m, attrs, order)
    sh = None
    if shading is not None:
        sh = dataclasses.replace(shading, attrs=A)
    col = dep = None
    if start is not None:
        col = None if start[0] is None else np.array(start[0], copy=True)
        dep = np.array(start[1], copy=True)
    c, d = oracle_frame(oracle, V, I, w, h, flags, sh, col, dep)
    rid = None
    if ids:
        dec = []
        for inv in (False, True):
            cv, ci = coded(V, I, inv)
            cc, cd = oracle_frame(oracle, cv, ci, w, h, flags & ~NC, None,
                                  None if start is None or start[0] is None else np.zeros_like(start[0]),
                                  None if start is None else np.array(start[1], copy=True))
            dec.append(decode(cc, inv))
        pos = np.where(dec[0] == dec[1], dec[0].astype(np.int64), LIVE)
        rid = pos.copy()
        hit = (pos >= 0) & (pos != NONE)
        rid[hit] = fmap[pos[hit]]
    return (None if flags & NC else c), d, rid, fmap


def same(ctx, flags, want, what=""):
    rc, rd, rid = want[:3]
    ctx.sync()
    d = ctx.read_depth()
    bad = np.nonzero(d.view(np.uint32) != rd.view(np.uint32))
    assert bad[0].size == 0, f"{what}: {bad[0].size} depth values differ"
    if rc is not None and not (flags & NC):
        c = ctx.read_color()
        bad = np.nonzero((c != rc).any(axis=-1))
        assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"
    if rid is not None:
        ids = ctx.read_ids()
        assert (ids[rid == LIVE] != NONE).all(), what
        bad = np.nonzero((ids != rid) & (rid >= 0))
        assert bad[0].size == 0, f"{what}: {bad[0].size} IDs differ, first {ids[bad][0]} vs {rid[bad][0]}"


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def metal_perspective(fy=1.2, aspect=W / H, near=0.5, far=6.0):
    """A Metal [0, 1]-depth perspective looking down +z: w = z_eye, z_clip = (z_eye - near) * far / (far - near)."""
    a = far / (far - near)
    m = np.zeros((4, 4), dtype=np.float64)       # rows = output, columns = input
    m[0, 0], m[1, 1] = fy / aspect, fy
    m[2, 2], m[2, 3] = a, -near * a
    m[3, 2] = 1.0
    return np.ascontiguousarray(m.astype(f32).T).reshape(16)


def straddling_soup(n, seed, z_lo=-1.0, z_hi=8.0, r=0.8):
    """Random triangles around centres spread from behind the eye to beyond the far plane."""
    rng = np.random.default_rng(seed)
    cen = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(z_lo, z_hi, n)], axis=1)
    xyz = (cen[:, None, :] + rng.uniform(-r, r, (n, 3, 3))).reshape(-1, 3).astype(f32)
    rgb = rng.uniform(0, 1, (3 * n, 3)).astype(f32)
    v = np.zeros((3 * n, 8), dtype=f32)
    v[:, 0:3], v[:, 4:7] = xyz, rgb
    xyz[:, 2][xyz[:, 2] == 0] = f32(0.25)          # (no clip-space z of exactly -0 / 0 from z_eye == near: keep it simple)
    v[:, 0:3] = xyz
    return v, np.arange(3 * n, dtype=np.int64)


def app_soup(swr, n, seed):
    """Triangles under the app's projection (w = z + 1 after the app's translation): centres on both sides of the near plane."""
    v, i = straddling_soup(n, seed, z_lo=-2.0, z_hi=1.5, r=0.6)
    return v, i, swr.scenes.app_transform(0.3, scale=1.0)


def draw(ctx, v, i, m, flags, shading=None):
    ctx.scene_upload(v, i)
    if shading is not None:
        ctx.shading_set(shading)
    ctx.target_set(W, H)
    ctx.draw(m, flags)


def crosses(v, i, m):
    r = clip_space(v, m)[np.asarray(i).reshape(-1, 3)]
    out = (r[..., 2] < 0) | (r[..., 3] - r[..., 2] < 0)
    return out.any(axis=1) & ~out.all(axis=1)


# ---- 1. in front: unchanged ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_in_front_unchanged(swr, mode):
    S = swr.scenes
    xyz, rgb, idx = S.torus_mesh(48, 24, 0.6, 0.25)
    scenes = [(S.pack_vertices(xyz, rgb), np.asarray(idx, dtype=np.int64), S.app_transform(0.4, scale=1.0))]
    s = S.cfg1_triangle()
    scenes.append((s.vertices, s.indices, s.transform))
    v, i = straddling_soup(2000, 0xF0, z_lo=1.5, z_hi=4.0, r=0.3)
    scenes.append((v, i, metal_perspective()))
    flags = MODES[mode]
    with swr.Context(0) as ctx:
        for v, i, m in scenes:
            r = clip_space(v, m)
            assert (r[:, 2] > 0).all() and (r[:, 3] - r[:, 2] > 0).all()
            draw(ctx, v, i, m, flags | IDS)
            ctx.sync()
            c0, d0, id0 = ctx.read_color(), ctx.read_depth(), ctx.read_ids()
            ctx.draw(m, flags | IDS | CLIP)
            ctx.sync()
            assert ctx.read_depth().tobytes() == d0.tobytes()
            assert (ctx.read_ids() == id0).all()
            if not flags & NC:
                assert (ctx.read_color() == c0).all()


# ---- 2. known answers ------------------------------------------------------------------------------------------------------------
def one(x0, x1, x2, rgb=((1, 0, 0), (0, 1, 0), (0, 0, 1))):
    v = np.zeros((3, 8), dtype=f32)
    v[:, 0:3] = np.array([x0, x1, x2], dtype=f32)
    v[:, 4:7] = np.array(rgb, dtype=f32)
    return v, np.arange(3, dtype=np.int64)


def test_known_answers(swr, oracle):
    m = metal_perspective()
    with swr.Context(0) as ctx:
        # one vertex behind the near plane (w > 0, z < 0): a quad of two sub-triangles
        v, i = one((-1.0, -0.8, 2.0), (1.0, -0.6, 2.5), (0.1, 0.9, 0.3))
        r = clip_space(v, m)
        assert r[2, 3] > 0 and r[2, 2] < 0
        _, _, _, fmap = want = expected(oracle, v, i, m, DT, ids=True)
        assert list(fmap) == [0, 0]
        draw(ctx, v, i, m, DT | IDS | CLIP)
        same(ctx, DT, want, "one vertex behind")
        c_clip = ctx.read_color()
        ctx.draw(m, DT)
        ctx.sync()
        assert (ctx.read_color() != c_clip).any(), "the frame without the flag must differ"
        # one vertex at w < 0: no mirrored artifact — pixels only where the clipped quad is
        v, i = one((-1.0, -0.8, 2.0), (1.0, -0.6, 2.5), (0.2, 0.5, -1.0))
        assert clip_space(v, m)[2, 3] < 0
        want = expected(oracle, v, i, m, 0, ids=True)
        draw(ctx, v, i, m, IDS | CLIP)
        same(ctx, 0, want, "w < 0")
        # crossing both planes: three sub-triangles
        v, i = one((-0.5, -0.3, 0.2), (0.6, -0.2, 9.0), (0.0, 0.6, 3.0))
        _, _, _, fmap = want = expected(oracle, v, i, m, DT, ids=True)
        assert len(fmap) == 3
        draw(ctx, v, i, m, DT | IDS | CLIP)
        same(ctx, DT, want, "both planes")
        # entirely behind / entirely beyond: nothing, IDs NONE
        for tri in [((-1, -1, -0.5), (1, -1, -0.6), (0, 1, -0.2)), ((-1, -1, 7.0), (1, -1, 8.0), (0, 1, 9.0))]:
            v, i = one(*tri)
            draw(ctx, v, i, m, DT | IDS | CLIP)
            ctx.sync()
            assert (ctx.read_ids() == NONE).all() and np.isposinf(ctx.read_depth()).all()
            assert (ctx.read_color()[..., 3] == 0).all()
        # a vertex exactly on the near plane: no duplicate vertex (the polygon stays a triangle ... or a quad, never 4 with a copy)
        v, i = one((-1.0, -0.8, 0.5), (1.0, -0.6, 2.5), (0.1, 0.9, 0.2))       # z_eye = near: z_clip == 0 exactly
        r = clip_space(v, m)
        assert r[0, 2] == 0
        _, _, _, _, fans = restate(v, i, m)
        pts = [tuple(q[:4]) for q in fans[0]]
        assert len(pts) == len(set(pts)) == 3
        want = expected(oracle, v, i, m, DT, ids=True)
        draw(ctx, v, i, m, DT | IDS | CLIP)
        same(ctx, DT, want, "vertex on the plane")


# ---- 3. random straddling soups ----------------------------------------------------------------------------------------------------
def with_ties(v, i):
    """Duplicate every 7th triangle (an exact tie across triangles; fans of duplicates share their diagonals too)."""
    t = np.asarray(i).reshape(-1, 3)
    dup = t[::7]
    return v, np.concatenate([t, dup]).reshape(-1)


@pytest.mark.parametrize("proj", ["app", "metal"])
@pytest.mark.parametrize("mode", list(MODES))
def test_random_straddling(swr, oracle, proj, mode):
    if proj == "app":
        v, i, m = app_soup(swr, 2000, 0xA11 + len(mode))
    else:
        v, i = straddling_soup(2000, 0xB22 + len(mode))
        m = metal_perspective()
    v, i = with_ties(v, i)
    assert crosses(v, i, m).sum() > 100
    flags = MODES[mode]
    want = expected(oracle, v, i, m, flags, ids=True)
    with swr.Context(0) as ctx:
        draw(ctx, v, i, m, flags | IDS | CLIP)
        same(ctx, flags, want, f"{proj} {mode}")


@pytest.mark.parametrize("shader", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
def test_random_straddling_shaded(swr, oracle, shader, mode):
    v, i = straddling_soup(2000, 0xC33 + shader)
    m = metal_perspective()
    sh = swr.scenes.random_shading(v.shape[0], 11 + shader, shader)
    flags = MODES[mode]
    want = expected(oracle, v, i, m, flags, ids=True, shading=sh)
    with swr.Context(0) as ctx:
        draw(ctx, v, i, m, flags | IDS | CLIP, shading=sh)
        same(ctx, flags, want, f"shader {shader} {mode}")


# ---- 4. shared edges -------------------------------------------------------------------------------------------------------------
def grid(n=24, z0=-0.5, z1=5.0):
    xs = np.linspace(-3, 3, n + 1, dtype=f32)
    zs = np.linspace(z0, z1, n + 1, dtype=f32)
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    xyz = np.stack([X, np.full_like(X, f32(-0.7)), Z], axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    v = np.zeros((xyz.shape[0], 8), dtype=f32)
    v[:, 0:3] = xyz
    v[:, 4:7] = rng.uniform(0, 1, (xyz.shape[0], 3))
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    t = np.stack([np.stack([a, a + n + 1, a + 1], 1), np.stack([a + 1, a + n + 1, a + n + 2], 1)], 1).reshape(-1)
    return v, t.astype(np.int64)


def test_shared_edges(swr, oracle):
    v, i = grid()
    m = metal_perspective()
    _, _, _, _, fans = restate(v, i, m)
    # adjacent triangles clip their shared edge to bit-identical vertices
    pts = {}
    for p, poly in enumerate(fans):
        for q in poly:
            if q[2] == 0:       # on the near plane: an intersection (or an input vertex exactly on it)
                pts.setdefault(tuple(np.round(q[:2].astype(np.float64), 4)), set()).add(q[:4].tobytes())
    assert pts and all(len(s) == 1 for s in pts.values())
    for flags in (0, DT):
        want = expected(oracle, v, i, m, flags, ids=True)
        with swr.Context(0) as ctx:
            draw(ctx, v, i, m, flags | IDS | CLIP)
            same(ctx, flags, want, f"grid {flags}")


# ---- 5. composition ----------------------------------------------------------------------------------------------------------------
def test_cull_per_sub_triangle(swr, oracle):
    v, i = straddling_soup(1500, 0xD44)
    m = metal_perspective()
    V, _, I, fmap, _ = restate(v, i, m)
    from test_cull import kept_triangles, signed_areas          # the culling filter, applied to the restated scene
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        for cull in (CB, CF, CB | CCW):
            flags = DT | cull
            keep = kept_triangles(signed_areas(oracle, V, I, IDENT, W, H, flags), flags)
            fi = I.reshape(-1, 3)[keep].reshape(-1)
            c, d = oracle_frame(oracle, V, fi, W, H, flags)
            ctx.draw(m, flags | CLIP)
            same(ctx, flags, (c, d, None), f"cull {cull}")


def ndc_scene(v, i, m):
    """The frame without the flag as a scene in NDC (every vertex r / w, no clipping), for the identity transform."""
    r = clip_space(v, m)
    out = np.array(np.asarray(v, dtype=f32).reshape(-1, 8), copy=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, 0:3] = r[:, 0:3] / r[:, 3:4]
    return out, np.asarray(i, dtype=np.int64)


def concat(*scenes):
    vs, is_, base = [], [], 0
    for v, i in scenes:
        vs.append(v)
        is_.append(np.asarray(i, dtype=np.int64) + base)
        base += v.shape[0]
    return np.concatenate(vs), np.concatenate(is_)


def test_load_chain_middle_clips(swr, oracle):
    """clear frame (no flag) -> load frame with the flag -> load frame without it: the oracle's frame of the three restated scenes
    concatenated (a load chain is the loop continued, include/swr.h "Load frames")."""
    v, i = straddling_soup(1200, 0xE55)
    m = metal_perspective()
    m2 = np.array(m, copy=True)
    m2[12] = f32(0.4)            # the second draw moves x
    sub = np.asarray(i).reshape(-1, 3)
    r = clip_space(v, m)[sub]
    inside = ((r[..., 2] >= 0) & (r[..., 3] - r[..., 2] >= 0)).all(axis=1)
    front = sub[inside].reshape(-1)                     # the first frame: only triangles entirely inside
    s1 = ndc_scene(v, front, m)
    s2 = restate(v, i, m2)[::2][:2]
    s3 = ndc_scene(v, i, m)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, front)
        ctx.target_set(W, H)
        ctx.draw(m, DT)
        same(ctx, DT, (*oracle_frame(oracle, *s1, W, H, DT), None), "first")
        ctx.scene_upload(v, i)
        ctx.draw(m2, DT | LOAD | CLIP)
        same(ctx, DT, (*oracle_frame(oracle, *concat(s1, s2), W, H, DT), None), "middle frame clips")
        ctx.draw(m, DT | LOAD)
        same(ctx, DT, (*oracle_frame(oracle, *concat(s1, s2, s3), W, H, DT), None), "last frame, no flag")


def test_draw_list_two_items(swr, oracle):
    v, i = straddling_soup(900, 0xF66)
    m = metal_perspective()
    mir = np.array(m, copy=True).reshape(4, 4)
    mir[0] = -mir[0]                 # mirrored model x
    mir = mir.reshape(16)
    n = i.size
    items = [(0, n // 2 // 3 * 3, m), (n // 2 // 3 * 3, n - n // 2 // 3 * 3, mir)]
    t = np.asarray(i).reshape(-1, 3)
    k0 = items[0][1] // 3
    ms = [m] * k0 + [mir] * (len(t) - k0)
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        for flags in (DT, 0):
            want = expected(oracle, v, i, ms, flags, ids=True)
            ctx.draw_list(items, flags | IDS | CLIP)
            same(ctx, flags, want, f"draw list {flags}")


def test_render_one_shot_and_scene_id(swr, oracle):
    v, i = straddling_soup(1000, 0x177)
    m = metal_perspective()
    want = expected(oracle, v, i, m, DT, ids=True)
    with swr.Context(0) as ctx:
        for sid in (0, 42, 42):
            c, d = ctx.render(v, i, m, W, H, DT | IDS | CLIP, scene_id=sid)
            assert (c == want[0]).all() and d.tobytes() == want[1].tobytes()
            ids = ctx.read_ids()
            assert ((ids == want[2]) | (want[2] < 0)).all()


@pytest.mark.parametrize("bands", [2, 4])
def test_multi_band(swr, oracle, bands):
    v, i = straddling_soup(1500, 0x288 + bands)
    m = metal_perspective()
    want = expected(oracle, v, i, m, DT, ids=True)
    with swr.Context(0, device_count=bands) as ctx:
        draw(ctx, v, i, m, DT | IDS | CLIP)
        same(ctx, DT, want, f"{bands} bands")


@pytest.mark.parametrize("key,value", [(1, 0), (1, -1), (3, 0), (3, 1), (3, 3)])
def test_debug_paths(swr, oracle, key, value):
    v, i = straddling_soup(1500, 0x399)
    m = metal_perspective()
    want = expected(oracle, v, i, m, DT, ids=True)
    with swr.Context(0) as ctx:
        ctx.debug_set(key, value)
        draw(ctx, v, i, m, DT | IDS | CLIP)
        same(ctx, DT, want, f"debug {key}={value}")


# ---- 6. capacity and overflow ------------------------------------------------------------------------------------------------------
def test_every_triangle_crosses(swr, oracle):
    """Maximal expansion: every triangle has one vertex behind the near plane -> two sub-triangles each, large ones; the first
    frame of a context (bins sized for the scene) and an un-waited burst that alternates clip and no-clip frames."""
    rng = np.random.default_rng(0x4AA)
    n = 3000
    xyz = np.empty((n, 3, 3), dtype=f32)
    xyz[:, 0:2, 0] = rng.uniform(-3, 3, (n, 2))
    xyz[:, 0:2, 1] = rng.uniform(-2, 2, (n, 2))
    xyz[:, 0:2, 2] = rng.uniform(0.8, 3.0, (n, 2))
    xyz[:, 2] = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.3, n)], 1)
    v = np.zeros((3 * n, 8), dtype=f32)
    v[:, 0:3] = xyz.reshape(-1, 3)
    v[:, 4:7] = rng.uniform(0, 1, (3 * n, 3))
    i = np.arange(3 * n, dtype=np.int64)
    m = metal_perspective()
    assert crosses(v, i, m).all()
    want = expected(oracle, v, i, m, DT, ids=True)
    plain, plain_d, _, _ = oracle.render(v, i, m, W, H, DT | oracle.TINV_PER_TRIANGLE)
    with swr.Context(0) as ctx:
        draw(ctx, v, i, m, DT | IDS | CLIP)
        same(ctx, DT, want, "first frame")
        c, d = np.zeros((H, W, 4), np.uint8), np.zeros((H, W), np.float32)
        for k in range(6):
            ctx.draw(m, DT | (CLIP if k % 2 == 0 else 0))
        ctx.present(c, d)
        ctx.present_wait()
        assert d.tobytes() == plain_d.tobytes()
        ctx.draw(m, DT | IDS | CLIP)
        same(ctx, DT, want, "after the burst")


# ---- 7. the 2^20 edge --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["below_to_above", "above_to_below"])
def test_2_20_edge(swr, oracle, case):
    """Submitted below 2^20 with a post-clip count above it, and the reverse: the clip frame equals the frame without the flag of
    the restated scene (built here in bulk: the crossing triangles are simple enough to clip in closed form)."""
    n = (1 << 20) - 64 if case == "below_to_above" else (1 << 20) + 4096
    rng = np.random.default_rng(7)
    # tiny triangles at z_eye in front; a block of them crosses the near plane with one vertex behind (two sub-triangles each)
    # (below_to_above), or lies entirely behind (above_to_below)
    cx, cy = rng.uniform(-2, 2, n).astype(f32), rng.uniform(-1.2, 1.2, n).astype(f32)
    z = rng.uniform(1.0, 4.0, n).astype(f32)
    xyz = np.empty((n, 3, 3), dtype=f32)
    xyz[:, 0] = np.stack([cx, cy, z], 1)
    xyz[:, 1] = np.stack([cx + f32(0.01), cy, z], 1)
    xyz[:, 2] = np.stack([cx, cy + f32(0.01), z], 1)
    k = 8192
    if case == "below_to_above":
        xyz[:k, 2, 2] = f32(-0.5)        # one corner behind: 2 sub-triangles each, 2^20 - 64 + 8192 > 2^20 after the clip
    else:
        xyz[:k, :, 2] = f32(-0.5)        # entirely behind: 2^20 + 4096 - 8192 < 2^20 after the clip
    v = np.zeros((3 * n, 8), dtype=f32)
    v[:, 0:3] = xyz.reshape(-1, 3)
    v[:, 4:7] = rng.uniform(0, 1, (3 * n, 3)).astype(f32)
    i = np.arange(3 * n, dtype=np.int64)
    m = metal_perspective()
    # the restated scene: the test clipper for the k crossing triangles, the plain divide for the others (all inside)
    r = clip_space(v, m).reshape(n, 3, 4)
    V0, _, _, fm0, _ = restate(v[:3 * k], np.arange(3 * k), m)
    q = np.zeros((n - k, 3, 8), dtype=f32)
    q[..., 0:3] = r[k:, :, 0:3] / r[k:, :, 3:4]
    q[..., 4:7] = v[3 * k:, 4:7].reshape(-1, 3, 3)
    fanv = [V0, q.reshape(-1, 8)]
    fmap = list(fm0) + list(range(k, n))
    V = np.concatenate(fanv)
    fmap = np.array(fmap)
    post = V.shape[0] // 3
    assert (n < (1 << 20)) != (post < (1 << 20))
    with swr.Context(0) as ctx:
        for extra in (0, LOAD):
            ctx.scene_upload(V, np.arange(V.shape[0], dtype=np.int64))
            ctx.target_set(W, H)
            if extra:                       # (waited for: the first frame of a new scene may overflow the bins and be redrawn)
                ctx.draw(IDENT, DT | IDS)
                ctx.sync()
            ctx.draw(IDENT, DT | IDS | extra)
            ctx.sync()
            c0, d0, id0 = ctx.read_color(), ctx.read_depth(), ctx.read_ids()
            ctx.scene_upload(v, i)
            ctx.target_set(W, H)
            if extra:
                ctx.draw(m, DT | IDS | CLIP)
                ctx.sync()
            ctx.draw(m, DT | IDS | CLIP | extra)
            ctx.sync()
            assert ctx.read_depth().tobytes() == d0.tobytes()
            assert (ctx.read_color() == c0).all()
            if not extra:                                    # the clear frame against the oracle on the restated scene as well
                rc, rd = oracle_frame(oracle, V, np.arange(V.shape[0], dtype=np.int64), W, H, DT)
                assert (c0 == rc).all() and d0.tobytes() == rd.tobytes()
            ids = ctx.read_ids()
            mapped = np.where(id0 == NONE, NONE, fmap[np.minimum(id0, fmap.size - 1)]).astype(np.uint32)
            assert (ids == mapped).all()


# ---- 8. edge cases ----------------------------------------------------------------------------------------------------------------
def test_edge_cases(swr, oracle):
    v, i = straddling_soup(800, 0x5BB)
    v[5, 0] = np.inf
    v[40, 1] = np.nan
    m = metal_perspective()
    want = expected(oracle, v, i, m, DT, ids=True)
    assert 1 not in set(want[3]) and 13 not in set(want[3])      # the triangles of the non-finite vertices are dropped
    with swr.Context(0) as ctx:
        draw(ctx, v, i, m, DT | IDS | CLIP)
        same(ctx, DT, want, "non-finite")
        pairs_clip = ctx.timings()
        # .vertices and .line frames ignore the bit
        for prim in (2, 1):
            ii = i if prim == 2 else i[: i.size // 2 * 2]
            ctx.scene_upload(v, ii)
            ctx.draw(m, DT, prim)
            ctx.sync()
            c0, d0 = ctx.read_color(), ctx.read_depth()
            ctx.draw(m, DT | CLIP, prim)
            ctx.sync()
            assert (ctx.read_color() == c0).all() and ctx.read_depth().tobytes() == d0.tobytes()
        # a frame without the flag after clip frames: the oracle's frame of the scene as it is
        ctx.scene_upload(v, i)
        ctx.draw(m, DT | CLIP)
        ctx.draw(m, DT)
        c, d, _, code = oracle.render(v, i, m, W, H, DT | oracle.TINV_PER_TRIANGLE)
        assert code == 0
        same(ctx, DT, (c, d, None), "no flag after clip frames")
    assert pairs_clip["triangles"] == i.size // 3


def test_tile_pairs_count_fans(swr):
    v, i = one((-1.0, -0.8, 2.0), (1.0, -0.6, 2.5), (0.1, 0.9, 0.3))
    m = metal_perspective()
    with swr.Context(0) as ctx:
        draw(ctx, v, i, m, DT)
        ctx.sync()
        plain = ctx.timings()
        ctx.draw(m, DT | CLIP)
        ctx.sync()
        t = ctx.timings()
        V, _, I, _, _ = restate(v, i, m)
        ctx.scene_upload(V, I)
        ctx.draw(IDENT, DT)
        ctx.sync()
        assert t["triangles"] == 1 and t["tile_pairs"] == ctx.timings()["tile_pairs"] != plain["tile_pairs"]


def test_fan_overflow_first_frame_and_dropped_burst(swr, oracle):
    """More crossing triangles than a fresh context's fan capacity: the first frame is redrawn silently; a presented, un-waited
    frame of a burst that overflowed is reported as SWR_ERR_FRAME_DROPPED (as for a bin overflow), and the next frames are right."""
    rng = np.random.default_rng(0x4AB)
    n = 3000
    xyz = np.empty((n, 3, 3), dtype=f32)
    xyz[:, 0:2, 0] = rng.uniform(-2, 2, (n, 2))
    xyz[:, 0:2, 1] = rng.uniform(-1.5, 1.5, (n, 2))
    xyz[:, 0:2, 2] = rng.uniform(0.8, 3.0, (n, 2))
    xyz[:, 2] = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.3, n)], 1)
    v = np.zeros((3 * n, 8), dtype=f32)
    v[:, 0:3] = xyz.reshape(-1, 3)
    v[:, 4:7] = rng.uniform(0, 1, (3 * n, 3))
    i = np.arange(3 * n, dtype=np.int64)
    m = metal_perspective()
    want = expected(oracle, v, i, m, DT)
    assert want[3].size > n + 2 * 1024                       # more fan triangles than n + 2 x the first capacity
    with swr.Context(0) as ctx:                              # one-shot: the overflowed frame is redrawn inside swr_render
        c, d = ctx.render(v, i, m, W, H, DT | CLIP)
        assert ctx.render_timings()["frames"] >= 2
        assert (c == want[0]).all() and d.tobytes() == want[1].tobytes()
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        c, d = np.zeros((H, W, 4), np.uint8), np.zeros((H, W), np.float32)
        ctx.draw(m, DT | CLIP)
        ctx.present(c, d)                                    # presented, not waited for: overflowed
        ctx.draw(m, DT)
        with pytest.raises(swr.SwrError) as e:
            ctx.sync()
        assert e.value.code == -8
        ctx.draw(m, DT | CLIP)
        same(ctx, DT, want, "after the drop")


def test_two_stream_scheduler(swr, oracle, monkeypatch):
    """SWR_LANES=0: the two-stream frame pipeline takes the pre-pass and the ID map as well."""
    monkeypatch.setenv("SWR_LANES", "0")
    v, i = straddling_soup(1500, 0x6CC)
    m = metal_perspective()
    want = expected(oracle, v, i, m, DT, ids=True)
    with swr.Context(0) as ctx:
        draw(ctx, v, i, m, DT | IDS | CLIP)
        for _ in range(6):                                   # a pipelined burst, then the last one checked
            ctx.draw(m, DT | IDS | CLIP)
        same(ctx, DT, want, "SWR_LANES=0")
