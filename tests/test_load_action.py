"""Load frames (SWR_FLAG_LOAD, include/swr.h "Load frames"): a frame drawn on top of the image already there.

Expected images come from the unchanged oracle.  The composition identity: scene A drawn with M_A, then scene B drawn with M_B as a
load frame, is bit for bit ONE clear frame of A || B drawn with the identity transform, every vertex pre-transformed by its own
matrix in the order of Vertex.apply (float32, no FMA), B's indices offset by A's vertex count.  Arbitrary starting images follow
the per-pixel rule: z-test keeps (cB, dB) where dB < d0, painter's order overwrites where B covers (alpha 255) and keeps d0.
"""
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, NC, METAL, REAL_LINES, LOAD = 1, 2, 4, 8, 16
TRI, LINE, VERTICES = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(c, d, rc, rd, what=""):
    if rc is not None:
        bad = np.nonzero((c != rc).any(axis=-1))
        assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"
    bad = np.nonzero(d.view(np.uint32) != rd.view(np.uint32))
    assert bad[0].size == 0, f"{what}: {bad[0].size} depth values differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"


def pretransform(vertices, m):
    """Vertex.apply in float32 without FMA: r = c0 x; r += c1 y; r += c2 z; r += c3; ndc = r.xyz / r.w."""
    v = np.array(vertices, dtype=np.float32, copy=True).reshape(-1, 8)
    c = np.asarray(m, dtype=np.float32).reshape(4, 4)          # column-major: c[k] = column k
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    r = c[0][None, :] * x
    r = r + c[1][None, :] * y
    r = r + c[2][None, :] * z
    r = r + c[3][None, :]
    v[:, 0:3] = r[:, 0:3] / r[:, 3:4]
    return v


def concat(parts):
    """[(vertices, indices, transform)] -> the pre-transformed A || B || ... and its indices."""
    vs, ix, base = [], [], 0
    for v, i, m in parts:
        vs.append(pretransform(v, m))
        ix.append(np.asarray(i, dtype=np.int64) + base)
        base += v.shape[0]
    return np.concatenate(vs), np.concatenate(ix)


def check_pretransform(oracle, v, m, w, h):
    """The harness's pre-transform projects to the same sx / sy / sz bits as projecting with M directly."""
    ident = np.eye(4, dtype=np.float32).T.reshape(16)
    a = oracle.project(v, m, w, h)
    b = oracle.project(pretransform(v, m), ident, w, h)
    for p, q in zip(a, b):
        assert p.tobytes() == q.tobytes()


def expected(oracle, parts, w, h, flags, shading=None):
    v, i = concat(parts)
    ident = np.eye(4, dtype=np.float32).T.reshape(16)
    if flags & METAL:
        c, d, _, code = oracle.render_metal(v, i, ident, w, h, flags & NC, shading=shading)
    else:
        c, d, _, code = oracle.render(v, i, ident, w, h, flags | oracle.TINV_PER_TRIANGLE, shading=shading)
    assert code == 0
    return c, d


def scenes_for_chain(swr, w, h):
    """Three scenes: A at M_A; B at M_A too, half of it A's own triangles with other colours (exact depth ties across
    frames: the earlier frame must keep them) and half new ones; C at another matrix."""
    S = swr.scenes
    a = S.random_soup(400, w, h, 0x10AD, r_ndc=0.15, margin=1.1)
    m_a = S.app_transform(0.3, scale=1.2)
    vb = a.vertices[:600].copy()
    vb[:, 4:7] = vb[::-1, 4:7]
    extra = S.random_soup(200, w, h, 0x20AD, r_ndc=0.2, margin=1.1)
    b_v = np.concatenate([vb, extra.vertices])
    b_i = np.arange(b_v.shape[0], dtype=np.int64)
    c = S.random_soup(300, w, h, 0x30AD, r_ndc=0.12, margin=1.1)
    m_c = S.app_transform(1.1, scale=1.5)
    return [(a.vertices, a.indices, m_a), (b_v, b_i, m_a), (c.vertices, c.indices, m_c)]


def shading_for(swr, parts, shader):
    if shader is None:
        return [None] * len(parts), None
    S = swr.scenes
    base = S.random_shading(sum(p[0].shape[0] for p in parts), 0x5A, shader)
    out, at = [], 0
    for v, _, _ in parts:
        out.append(dataclasses.replace(base, attrs=base.attrs[at:at + v.shape[0]]))
        at += v.shape[0]
    return out, base


MODES = {
    "painter": (0, None), "ztest": (DT, None), "depth_only": (DT | NC, None), "depth_only_64": (DT | NC, None),
    "metal": (METAL, None), "metal_depth": (METAL | NC, None), "phong": (DT, 1), "textured": (DT, 2),
    "painter_phong": (0, 1),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_resident_chain_equals_the_concatenation(swr, oracle, mode):
    """A at M_A, then B and C with SWR_FLAG_LOAD: after two frames and after three, bit for bit the clear frame of the
    concatenation (ties across frames: the earlier frame wins)."""
    flags, shader = MODES[mode]
    w, h = 640, 360
    parts = scenes_for_chain(swr, w, h)
    for v, _, m in parts:
        check_pretransform(oracle, v, m, w, h)
    shades, whole = shading_for(swr, parts, shader)
    with swr.Context(0) as ctx:
        if mode == "depth_only_64":
            ctx.debug_set(swr.binding.DEBUG_DEPTH_KEYS32, 0)
        ctx.target_set(w, h)
        for k, ((v, i, m), sh) in enumerate(zip(parts, shades)):
            ctx.scene_upload(v, i)
            if sh is not None:
                ctx.shading_set(sh)
            ctx.draw(m, flags | (LOAD if k else 0))
            if k == 0:
                continue
            ctx.sync()
            d = ctx.read_depth()
            c = None if flags & NC else ctx.read_color()
            rc, rd = expected(oracle, parts[:k + 1], w, h, flags,
                              shading=None if whole is None else dataclasses.replace(
                                  whole, attrs=whole.attrs[:sum(p[0].shape[0] for p in parts[:k + 1])]))
            same(c, d, None if flags & NC else rc, rd, f"{mode}: chain of {k + 1}")


def special_start(w, h, seed):
    """A starting image with NaN, +-0, -inf, +inf and denormals among ordinary depths in (0, 1)."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    specials = np.array([np.nan, 0.0, -0.0, -np.inf, np.inf, 1e-40, -1e-40, 1e-45, 0.5], dtype=np.float32)
    pick = rng.integers(0, specials.size, (h, w))
    mask = rng.uniform(size=(h, w)) < 0.3
    d[mask] = specials[pick[mask]]
    d.view(np.uint32)[5, 7] = 0x7FC01234            # a NaN with a payload: its bits survive
    c = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return c, d


def start_rule(c0, d0, cb, db, flags):
    """Per-pixel expectation of a load frame of B over (c0, d0), from B's own clear frame (cb, db)."""
    if flags & (DT | METAL):
        win = db < d0
        d = np.where(win, db, d0)
        c = None if cb is None else np.where(win[..., None], cb, c0)
    else:
        d = d0.copy()
        c = None if cb is None else np.where((cb[..., 3] == 255)[..., None], cb, c0)
    return c, d


@pytest.mark.parametrize("how", ["target_write", "render"])
@pytest.mark.parametrize("mode", ["ztest", "painter", "depth_only", "depth_only_64", "metal"])
def test_arbitrary_starting_image(swr, oracle, how, mode):
    flags = {"ztest": DT, "painter": 0, "depth_only": DT | NC, "depth_only_64": DT | NC, "metal": METAL}[mode]
    w, h = 520, 300                                 # (520: the ragged right edge of the last tile column)
    S = swr.scenes
    b = S.random_soup(1500, w, h, 0xB0B, r_ndc=0.1, margin=1.1)
    b.vertices[::53, 2] = 0.0                       # fragments at exactly +-0 against loaded zeros
    b.vertices[::71, 2] = -0.0
    c0, d0 = special_start(w, h, 99)
    if flags & METAL:
        cb, db, _, code = oracle.render_metal(b.vertices, b.indices, b.transform, w, h)
    else:
        cb, db, _, code = oracle.render(b.vertices, b.indices, b.transform, w, h, flags | oracle.TINV_PER_TRIANGLE)
    assert code == 0
    rc, rd = start_rule(c0, d0, None if flags & NC else cb, db, flags)
    with swr.Context(0) as ctx:
        if mode == "depth_only_64":
            ctx.debug_set(swr.binding.DEBUG_DEPTH_KEYS32, 0)
        if how == "target_write":
            ctx.scene_upload(b.vertices, b.indices)
            ctx.target_set(w, h)
            ctx.target_write(None if flags & NC else c0, d0)
            ctx.draw(b.transform, flags | LOAD)
            ctx.sync()
            d = ctx.read_depth()
            c = None if flags & NC else ctx.read_color()
        else:
            c, d = ctx.render(b.vertices, b.indices, b.transform, w, h, flags | LOAD,
                              color=None if flags & NC else c0.copy(), depth=d0.copy(), scene_id=7)
            # the same again with the scene cached: the images are inputs, not cached
            c, d = ctx.render(b.vertices, b.indices, b.transform, w, h, flags | LOAD,
                              color=None if flags & NC else c0.copy(), depth=d0.copy(), scene_id=7)
            assert ctx.render_timings()["scene_cached"] == 1
    same(c, d, rc, rd, f"{how} {mode}")


@pytest.mark.parametrize("flags", [0, DT, DT | NC, METAL])
def test_load_right_after_target_set_is_the_clear_frame(swr, oracle, flags):
    w, h = 400, 256
    s = swr.scenes.random_soup(800, w, h, 0xC1EA, r_ndc=0.1, margin=1.1)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(w, h)
        ctx.draw(s.transform, flags)
        ctx.sync()
        want_d = ctx.read_depth().copy()
        want_c = None if flags & NC else ctx.read_color().copy()
        ctx.target_set(w, h)                       # (same target: the images are the cleared ones again)
        ctx.draw(s.transform, flags | LOAD)
        ctx.sync()
        same(None if flags & NC else ctx.read_color(), ctx.read_depth(), want_c, want_d, "load after target_set")


def test_unwaited_burst_of_load_frames(swr, oracle):
    """The resident frame loop: one scene, a clear frame and eight load frames with nine transforms, none waited for (the draws
    return at once, frames of all four lanes overlap), every frame presented into its own host image, then one present_wait:
    image k is the chain's prefix of k + 1 frames."""
    w, h = 512, 256
    S = swr.scenes
    s = S.random_soup(2000, w, h, 0xF00, r_ndc=0.05, margin=1.0)
    ms = [S.app_transform(0.37 * k, scale=1.0 + 0.1 * k) for k in range(9)]
    parts = [(s.vertices, s.indices, m) for m in ms]
    imgs = [(swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)) for _ in parts]
    try:
        with swr.Context(0) as ctx:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(w, h)
            for k, m in enumerate(ms):
                ctx.draw(m, DT | (LOAD if k else 0))
                ctx.present(*imgs[k])
            ctx.present_wait()
        for k in range(len(parts)):
            rc, rd = expected(oracle, parts[:k + 1], w, h, DT)
            same(imgs[k][0].array, imgs[k][1].array, rc, rd, f"burst image {k}")
    finally:
        for a, b in imgs:
            a.free(); b.free()


def crowded_scene(swr, ntri=20000):
    """ntri small triangles inside two neighbouring tiles of a 1280x720 frame: far more entries than the initial tile region of
    the fixed-stride bins holds."""
    s = swr.scenes.random_soup(ntri, 1280, 720, 555, r_ndc=0.01, flags=DT, margin=1.0)
    v = s.vertices.copy()
    v[:, 0] = 0.30 + (v[:, 0] * 0.5 + 0.5) * 0.07
    v[:, 1] = 0.10 + (v[:, 1] * 0.5 + 0.5) * 0.06
    s.vertices = np.ascontiguousarray(v)
    return s


def big_scene(swr, ntri=220):
    """A few hundred near-full-screen triangles: far more (triangle,tile) pairs than the initial exact-bin capacity."""
    return swr.scenes.random_soup(ntri, 1280, 720, 77, r_ndc=1.4, flags=DT, margin=0.3)


@pytest.mark.parametrize("bins", ["fixed", "exact"])
def test_bin_overflow_inside_a_chain(swr, oracle, bins):
    """A load frame never builds silently on an overflowed frame: every presented image is right, or the burst is reported."""
    S = swr.scenes
    w, h = 1280, 720
    a = S.random_soup(500, w, h, 0xA11, r_ndc=0.1, margin=1.1)
    b = big_scene(swr) if bins == "exact" else crowded_scene(swr)
    c = S.random_soup(500, w, h, 0xC11, r_ndc=0.1, margin=1.1)
    m_c = S.app_transform(0.9, scale=1.3)
    parts = [(a.vertices, a.indices, a.transform), (b.vertices, b.indices, b.transform), (c.vertices, c.indices, m_c)]
    want = [expected(oracle, parts[:k + 1], w, h, DT) for k in range(3)]

    def ctx_for():
        ctx = swr.Context(0)
        if bins == "exact":
            ctx.debug_set(swr.binding.DEBUG_BIN_MODE, swr.binding.BIN_MODE_EXACT)
        ctx.target_set(w, h)
        return ctx

    # (1) the overflowing load frame is the last one: redrawn from the same starting image, silently right
    with ctx_for() as ctx:
        ctx.scene_upload(a.vertices, a.indices)
        ctx.draw(a.transform, DT)
        ctx.scene_upload(b.vertices, b.indices)
        ctx.draw(b.transform, DT | LOAD)
        hc, hd = swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)
        ctx.present(hc, hd)
        ctx.present_wait()
        same(hc.array, hd.array, *want[1], "overflowing last load frame, repaired")
        hc.free(); hd.free()
    # (2) an un-waited resident burst on ONE scene (A || B || C pre-transformed, drawn three times with LOAD): the first
    # frame's bins overflow, the frames after it loaded an empty image: reported, never silently wrong
    v, i = concat(parts)
    ident = np.eye(4, dtype=np.float32).T.reshape(16)
    with ctx_for() as ctx:
        ctx.scene_upload(v, i)
        imgs = [(swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)) for _ in range(3)]
        chain = [expected(oracle, [(v, i, ident)] * (k + 1), w, h, DT) for k in range(3)]
        for k in range(3):
            ctx.draw(ident, DT | (LOAD if k else 0))
            ctx.present(*imgs[k])
        reported = False
        try:
            ctx.present_wait()
        except swr.SwrError as e:
            assert e.code == -8
            reported = True
            ctx.present_wait()
        if not reported:
            for k in range(3):
                same(imgs[k][0].array, imgs[k][1].array, *chain[k], f"burst image {k}")
        else:
            # the last frame is never left silently wrong either: a redraw of the chain from a clear frame is right
            ctx.draw(ident, DT)
            ctx.draw(ident, DT | LOAD)
            ctx.sync()
            same(ctx.read_color(), ctx.read_depth(), *chain[1], "chain redrawn after the report")
        for x, y in imgs:
            x.free(); y.free()


@pytest.mark.parametrize("prim", ["vertices", "real_lines", "line_stub"])
def test_points_and_lines_keep_the_loaded_depth(swr, oracle, prim):
    w, h = 384, 256
    S = swr.scenes
    a = S.random_soup(600, w, h, 0xD0D, r_ndc=0.12, margin=1.1)
    b = S.random_soup(400, w, h, 0xE0E, r_ndc=0.3, margin=1.1)
    ptype, flags = {"vertices": (VERTICES, 0), "real_lines": (LINE, REAL_LINES), "line_stub": (LINE, 0)}[prim]
    bi = b.indices if ptype != LINE else b.indices[: (b.indices.size // 2) * 2]
    with swr.Context(0) as ctx:
        ctx.scene_upload(a.vertices, a.indices)
        ctx.target_set(w, h)
        ctx.draw(a.transform, DT)
        ctx.sync()
        c0, d0 = ctx.read_color().copy(), ctx.read_depth().copy()
        ctx.scene_upload(b.vertices, bi)
        ctx.draw(b.transform, flags | LOAD, ptype)
        ctx.sync()
        c, d = ctx.read_color(), ctx.read_depth()
    assert d.tobytes() == d0.tobytes(), "a .vertices / .line load frame must leave the depth image as loaded"
    cb, _, _, code = oracle.render(b.vertices, bi, b.transform, w, h, flags, primitive_type=ptype)
    assert code == 0
    want = np.where((cb[..., 3] == 255)[..., None], cb, c0)
    same(c, d, want, d0, prim)


def test_eight_bands_chain_of_two_at_cfg4_size(swr, oracle):
    """device_count = 8 (all on one GPU here): every band loads and writes its own image; cfg4 size, depth-only and colour."""
    S = swr.scenes
    s = S.cfg4_soup(200_000)
    m_b = S.app_transform(0.5, scale=1.0)
    parts = [(s.vertices, s.indices, s.transform), (s.vertices, s.indices, m_b)]
    rc, rd = expected(oracle, parts, s.width, s.height, DT)
    for flags in (DT | NC, DT):
        with swr.Context(0, device_count=8) as ctx:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(s.width, s.height)
            ctx.draw(s.transform, flags)
            ctx.draw(m_b, flags | LOAD)
            ctx.sync()
            d = ctx.read_depth()
            c = None if flags & NC else ctx.read_color()
        same(c, d, None if flags & NC else rc, rd, f"8 bands, flags {flags}")


@pytest.mark.parametrize("bins", ["fixed", "exact"])
def test_load_frame_on_an_unpresented_overflowed_frame_is_reported(swr, oracle, bins):
    """The case the chain rule exists for: a frame whose bins overflow is NOT presented (so it is never reported itself), and a
    load frame drawn on it is the last frame.  Without the rule that load frame would verify cleanly while holding its own
    triangles over an empty image; it must be reported (-8).  Then the chain redrawn from a clear frame is right."""
    if bins == "exact":
        # a few hundred near-full-screen triangles at 4K: far more (triangle,tile) pairs than the initial exact bins hold
        w, h = 3840, 2160
        s = swr.scenes.random_soup(220, w, h, 77, r_ndc=1.4, flags=DT, margin=0.3)
    else:
        w, h = 1280, 720
        s = crowded_scene(swr)
    if bins == "exact":
        m1 = np.array([0.2, 0, 0, 0, 0, 0.2, 0, 0, 0, 0, 1, 0, 0.1, -0.1, 0, 1], dtype=np.float32)       # shrunk: few pairs
    else:
        k, cx, cy = 25.0, 0.335, 0.13                                                                  # the crowded patch spread out
        m1 = np.array([k, 0, 0, 0, 0, k, 0, 0, 0, 0, 1, 0, -k * cx, -k * cy, 0, 1], dtype=np.float32)
    ident = np.eye(4, dtype=np.float32).T.reshape(16)
    parts = [(s.vertices, s.indices, ident), (s.vertices, s.indices, m1)]
    rc, rd = expected(oracle, parts, w, h, DT)
    for finish in ("present_wait", "sync"):
        with swr.Context(0) as ctx:
            if bins == "exact":
                ctx.debug_set(swr.binding.DEBUG_BIN_MODE, swr.binding.BIN_MODE_EXACT)
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(w, h)
            ctx.draw(ident, DT)                          # overflows its bins (a fresh context), never presented
            ctx.draw(m1, DT | LOAD)
            hc, hd = swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)
            if finish == "present_wait":
                ctx.present(hc, hd)
            with pytest.raises(swr.SwrError) as e:
                ctx.present_wait() if finish == "present_wait" else ctx.sync()
            assert e.value.code == -8
            ctx.present_wait()
            # a load frame on the reported image is reported as well
            ctx.draw(m1, DT | LOAD)
            with pytest.raises(swr.SwrError) as e:
                ctx.sync()
            assert e.value.code == -8
            # the chain redrawn from a clear frame (the bins have grown): right, silently
            ctx.draw(ident, DT)
            ctx.draw(m1, DT | LOAD)
            ctx.present(hc, hd)
            ctx.present_wait()
            same(hc.array, hd.array, rc, rd, f"{bins}: chain redrawn after the report")
            hc.free(); hd.free()
