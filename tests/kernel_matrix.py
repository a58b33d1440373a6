"""The kernel matrix: every raster and binning kernel instantiation the dispatch can launch, the frame that reaches it, and the
expected images of such frames, built on the unchanged oracle.  A plain helper module of tests/test_kernel_matrix.py,
tests/test_primitive_boundary.py and tests/test_kernel_matrix_table.py (not a conftest, not a test file).

The rows are named by their template arguments exactly as written in launch_raster_keys / bin_kernel
(software-renderer_amd/csrc/swr_kernels.hip), the parameters lifted by with_bools (ZTEST, PLAIN, LOAD, IDS; k_bin: all four, LIST
written only where it is true) filled in; tests/test_kernel_matrix_table.py parses the dispatch and
fails when a variant is added there without a row here.

Expectations (include/swr.h):
  clear frames     oracle.render / oracle.render_metal, extended fragment stage included;
  load frames      the per-pixel rule of "Load frames" over an arbitrary starting image (load_rule, load_ids);
  primitive IDs    colour-coded de-indexed copies drawn twice, the second time with every digit inverted (coded, decode,
                   expected_ids; the technique of tests/test_primitive_ids.py, good to 2^21 triangles);
  face culling     exact integer signed areas of the truncated (Metal: rounded, then truncated) vertices (signed_areas, filtered);
  draw lists       the pre-transformed concatenation drawn with the identity (pretransform, concat).
"""
from __future__ import annotations

import dataclasses

import numpy as np

DT, NC, METAL, LOAD, IDS = 1, 2, 4, 16, 32
CB, CF, CCW = 64, 128, 256
NONE = 0xFFFFFFFF
LIVE = -1                       # (expected IDs) a pixel some fragment wins, whichever: a painter's-order fragment without a finite colour
IDENT = np.eye(4, dtype=np.float32).T.reshape(16)
LIMIT = float(1 << 30)
MASK21 = (1 << 21) - 1
PRIM_BITS = 20                  # WTAB_PRIM_BITS: the winner table's keys hold primitive numbers below 2^20 (load frames: + 1)
TILE_W, TILE_H = 64, 32

# (swr_debug_set keys and values, include/swr.h)
DEBUG_BIN_MODE, DEBUG_DEPTH_KEYS32, DEBUG_RASTER_SORT = 3, 5, 6
BIN_MODE_EXACT, BIN_MODE_ATOMIC = 1, 3

# the two targets every raster row is drawn on: 6 x 7 tiles, ragged on both edges (four workgroups per tile, vs_log = 2), and
# 20 x 23 = 460 tiles (one workgroup per tile, vs_log = 0; triangles there cover more than BIN_BIG_TILES = 128 tiles)
TARGETS = {"small": (328, 200), "large": (1280, 720)}
PADDED_TRIANGLES = (1 << PRIM_BITS) + 1


# ---- the matrix table -----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Row:
    """One kernel instantiation and the frame that reaches it.

    name     the kernel as written in the dispatch, template arguments filled in
    flags    the frame's flags (LOAD / IDS included)
    shader   SWR_SHADER_* of the context's material (0: the reference's passthrough stage)
    scenes   "visible" (the visible set, below 2^20 primitives: winner table) and / or "padded" (2^20 + 1 primitives: PLAIN)
    hooks    swr_debug_set (key, value) pairs, set on a fresh context before the scene and the target
    sorts    (k_raster_depth) the SWR_DEBUG_RASTER_SORT values to draw it with, one fresh context each: the scene's 32-bit-key
             state is sticky (one frame with many redone tiles moves it to the 64-bit kernel for good)
    Binning rows: metal / defer / affine / draw_list say which k_bin the frame reaches; `defer` frames are drawn twice on the large
    target, the first frame meeting triangles that cover hundreds of tiles."""
    name: str
    flags: int
    shader: int = 0
    scenes: tuple = ("visible",)
    hooks: tuple = ()
    sorts: tuple = ()
    metal: bool = False
    defer: bool = False
    affine: bool = True
    draw_list: bool = False
    targets: tuple = ("small", "large")

    @property
    def load(self):
        return bool(self.flags & LOAD)

    @property
    def ids(self):
        return bool(self.flags & IDS)


def _b(x):
    return "true" if x else "false"


# one entry per instantiation launch_raster_keys can reach, LOAD and IDS left open, in dispatch order:
# (name, flags, shader, scenes, only without IDS, hooks)
_BOTH = ("visible", "padded")
_RASTER = [
    # Metal rules
    ("k_raster_ext<true, true, true, {L}, {I}>", METAL, 2, ("padded",), False, ()),
    ("k_raster_ext<true, true, false, {L}, {I}>", METAL, 1, ("visible",), False, ()),
    ("k_raster<true, 0, true, true, true, {L}, {I}>", METAL, 0, ("padded",), False, ()),
    ("k_raster<true, 0, true, true, false, {L}, {I}>", METAL, 0, ("visible",), False, ()),
    ("k_raster<true, 0, true, false, false, {L}, {I}>", METAL | NC, 0, _BOTH, False, ()),
    # CPU rules, extended fragment stage
    ("k_raster_ext<true, false, true, {L}, {I}>", DT, 1, ("padded",), False, ()),
    ("k_raster_ext<true, false, false, {L}, {I}>", DT, 2, ("visible",), False, ()),
    ("k_raster_ext<false, false, true, {L}, {I}>", 0, 2, ("padded",), False, ()),
    ("k_raster_ext<false, false, false, {L}, {I}>", 0, 1, ("visible",), False, ()),
    # CPU rules, z-test
    ("k_raster<true, 0, false, true, true, {L}, {I}>", DT, 0, ("padded",), False, ()),
    ("k_raster<true, 0, false, true, false, {L}, {I}>", DT, 0, ("visible",), False, ()),
    ("k_raster_depth<{L}>", DT | NC, 0, _BOTH, True, ()),
    ("k_raster<true, 0, false, false, false, {L}, {I}>", DT | NC, 0, _BOTH, False, ((DEBUG_DEPTH_KEYS32, 0),)),
    # CPU rules, painter's order
    ("k_raster<false, 0, false, true, true, {L}, {I}>", 0, 0, ("padded",), False, ()),
    ("k_raster<false, 0, false, true, false, {L}, {I}>", 0, 0, ("visible",), False, ()),
    ("k_raster<false, 0, false, false, false, {L}, {I}>", NC, 0, _BOTH, False, ()),
]


def raster_rows():
    rows = []
    for load in (False, True):
        for ids in (False, True):
            for name, flags, shader, scenes, no_ids, hooks in _RASTER:
                if ids and no_ids:
                    continue
                f = flags | (LOAD if load else 0) | (IDS if ids else 0)
                sorts = (0, 2) if name.startswith("k_raster_depth") else ()
                hk = () if ids else hooks          # (ID frames take the 64-bit keys by themselves)
                rows.append(Row(name.format(L=_b(load), I=_b(ids)), f, shader, scenes, hk, sorts))
    return rows


def bin_rows():
    """The 16 k_bin<256, MT, DEFER, AFF, LIST> instantiations of bin_kernel (LIST = false: draws, true: draw lists)."""
    rows = []
    k = 0
    for metal in (False, True):
        for defer in (False, True):
            for affine in (False, True):
                for dl in (False, True):
                    name = f"k_bin<256, {_b(metal)}, {_b(defer)}, {_b(affine)}" + (", true>" if dl else ">")
                    flags = METAL if metal else (DT if k % 4 < 2 else 0)
                    flags |= (IDS if dl or k % 3 == 0 else 0)
                    flags |= (CB, CF | CCW, 0, CB | CCW)[k % 4]          # (culls happen in k_bin's setup)
                    rows.append(Row(name, flags, metal=metal, defer=defer, affine=affine, draw_list=dl,
                                    targets=("large",) if defer else ("small", "large")))
                    k += 1
    return rows


# the other binning paths (four-kernel chain with exact-size bins, global-atomic fallback): not k_bin, but the same frames
PATH_ROWS = [
    Row("bin_mode=exact, draw", DT | IDS | CB, hooks=((DEBUG_BIN_MODE, BIN_MODE_EXACT),)),
    Row("bin_mode=exact, draw list", METAL | IDS | CF, hooks=((DEBUG_BIN_MODE, BIN_MODE_EXACT),), draw_list=True, metal=True),
    Row("bin_mode=atomic, draw", IDS | CF | CCW, hooks=((DEBUG_BIN_MODE, BIN_MODE_ATOMIC),), affine=False),
    Row("bin_mode=atomic, draw list", DT | NC | IDS | CB, hooks=((DEBUG_BIN_MODE, BIN_MODE_ATOMIC),), draw_list=True, affine=False),
]

ROWS = raster_rows() + bin_rows()


# ---- the blend and resolve kernels (separate lists: ROWS stays the 62 + 16 raster and binning instantiations) ----------------------
BLEND = 4096
BLEND_OVER, BLEND_ADD = 0, 1
RESOLVE_SAMPLE0, RESOLVE_MIN = 0, 1
DEBUG_STREAM_ORDER = 1


@dataclasses.dataclass(frozen=True)
class BlendRow:
    """k_raster_blend<ZT, MT, LOAD> as written in launch_raster_blend (ZTEST, LOAD filled in), or k_blend_order; the blend frame that
    reaches it: flags (DT / METAL / LOAD, without the BLEND bit) and the swr_blend state."""
    name: str
    flags: int
    mode: int
    opacity: int

    @property
    def load(self):
        return bool(self.flags & LOAD)


def blend_rows():
    rows, k = [], 0
    for zt, mt, flags in ((False, False, 0), (True, False, DT), (True, True, METAL)):
        for load in (False, True):
            rows.append(BlendRow(f"k_raster_blend<{_b(zt)}, {_b(mt)}, {_b(load)}>", flags | (LOAD if load else 0),
                                 (BLEND_OVER, BLEND_ADD)[k % 2], (128, 200, 77, 254, 1, 150)[k]))
            k += 1
    return rows + [BlendRow("k_blend_order", DT | LOAD, BLEND_OVER, 140)]


@dataclasses.dataclass(frozen=True)
class ResolveRow:
    """k_resolve<S, DF, COLOR, DEPTH> as written in launch_resolve_sf, S and DF as launch_resolve passes them; the read that reaches
    it: colour and depth in one launch is swr_render_resolved's gather, one image is swr_read_color_resolved / _depth_resolved."""
    name: str
    S: int
    depth_filter: int
    color: bool
    depth: bool


_FILTER_NAME = {RESOLVE_SAMPLE0: "SWR_RESOLVE_DEPTH_SAMPLE0", RESOLVE_MIN: "SWR_RESOLVE_DEPTH_MIN"}


def resolve_rows():
    rows = []
    for S in (2, 4):
        for filt in (RESOLVE_SAMPLE0, RESOLVE_MIN):
            rows.append(ResolveRow(f"k_resolve<{S}, {_FILTER_NAME[filt]}, true, true>", S, filt, True, True))
        rows.append(ResolveRow(f"k_resolve<{S}, 0, true, false>", S, RESOLVE_SAMPLE0, True, False))
        for filt in (RESOLVE_SAMPLE0, RESOLVE_MIN):
            rows.append(ResolveRow(f"k_resolve<{S}, {_FILTER_NAME[filt]}, false, true>", S, filt, False, True))
    return rows


BLEND_ROWS = blend_rows()
RESOLVE_ROWS = resolve_rows()


def full_name(name):
    """The name with the template defaults the demangler prints (k_bin's LIST = false)."""
    if name.startswith("k_bin<") and name.count(",") == 3:
        return name[:-1] + ", false>"
    return name


# ---- transforms, draw lists ----------------------------------------------------------------------------------------------------
def affine_matrix(angle=0.09, scale=0.93, tx=0.03, ty=-0.02):
    c, s = np.cos(angle) * scale, np.sin(angle) * scale
    return np.array([c, s, 0, 0, -s, c, 0, 0, 0, 0, 1, 0, tx, ty, 0, 1], dtype=np.float32)


def perspective_matrix(k=0.25):
    """w = 1 + k z: a real perspective divide (the last row is not (0, 0, 0, 1)) that keeps the scene on the screen."""
    m = np.eye(4, dtype=np.float32).T.reshape(16).copy()
    m[11] = k
    return m


def mirrored(m):
    """m after a mirror of the model's x (det < 0): the winding as displayed flips."""
    c = np.array(np.asarray(m, dtype=np.float32).reshape(4, 4), copy=True)
    c[0] = -c[0]
    return c.reshape(16)


def pretransform(vertices, m):
    """Vertex.apply in float32 without FMA: r = c0 x; r += c1 y; r += c2 z; r += c3; ndc = r.xyz / r.w."""
    v = np.array(vertices, dtype=np.float32, copy=True).reshape(-1, 8)
    c = np.asarray(m, dtype=np.float32).reshape(4, 4)
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    r = c[0][None, :] * x
    r = r + c[1][None, :] * y
    r = r + c[2][None, :] * z
    r = r + c[3][None, :]
    v[:, 0:3] = r[:, 0:3] / r[:, 3:4]
    return v


def concat(vertices, indices, items):
    """A draw list [(first_index, index_count, transform)] as one pre-transformed scene, drawn with the identity."""
    vs, ix, base = [], [], 0
    for first, count, m in items:
        vs.append(pretransform(vertices, m))
        ix.append(np.asarray(indices[first:first + count], dtype=np.int64) + base)
        base += vertices.shape[0]
    return np.concatenate(vs), np.concatenate(ix)


# ---- clear frames and the load rule ---------------------------------------------------------------------------------------------
def oracle_clear(oracle, v, i, m, w, h, flags, shading=None):
    """(colour or None, depth) of the oracle's clear frame (flags: DT / NC / METAL; the rest is ignored)."""
    if flags & METAL:
        c, d, _, code = oracle.render_metal(v, i, m, w, h, flags & NC, shading=shading)
    else:
        c, d, _, code = oracle.render(v, i, m, w, h, (flags & (DT | NC)) | oracle.TINV_PER_TRIANGLE, shading=shading)
    assert code == 0
    return (None if flags & NC else c), d


def special_start(w, h, seed):
    """A starting image with NaN (one with a payload), +-0, +-inf and +-denormals among ordinary depths in (0, 1)."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    specials = np.array([np.nan, 0.0, -0.0, -np.inf, np.inf, 1e-40, -1e-40, 1e-45, -1e-45, 0.5], dtype=np.float32)
    pick = rng.integers(0, specials.size, (h, w))
    mask = rng.uniform(size=(h, w)) < 0.3
    d[mask] = specials[pick[mask]]
    d.view(np.uint32)[5, 7] = 0x7FC01234            # a NaN with a payload: its bits survive
    c = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return c, d


def load_wins(d0, cb, db, flags, rid_b=None):
    """Where a load frame of B over the depth image d0 keeps B's fragment (B's own clear frame: cb, db, IDs rid_b).
    z-test (always under the Metal rules): strict '<' against the loaded depth — a loaded NaN or -inf is never replaced, -0 and +0
    compare equal; painter's order: every covered pixel (alpha 255; without colour: a pixel B's IDs cover)."""
    if flags & (DT | METAL):
        return db < d0
    if cb is not None:
        return cb[..., 3] == 255
    assert rid_b is not None
    return rid_b != NONE


def load_rule(c0, d0, cb, db, flags, rid_b=None):
    """(colour or None, depth) of a load frame of B over (c0, d0)."""
    win = load_wins(d0, cb, db, flags, rid_b)
    d = np.where(win, db, d0) if flags & (DT | METAL) else d0.copy()
    c = None if cb is None else np.where(win[..., None], cb, c0)
    return c, d


def load_ids(d0, cb, db, rid_b, flags):
    """IDs of a load frame of B: B's where B's fragment is kept, SWR_ID_NONE where the loaded image wins."""
    return np.where(load_wins(d0, cb, db, flags, rid_b), rid_b, np.int64(NONE))


# ---- primitive IDs ---------------------------------------------------------------------------------------------------------------
def coded(vertices, indices, invert=False):
    """The de-indexed copy of a scene, triangle t in the flat colour (2 d_c + 1) / 255 per channel, d_c its c-th 7-bit digit
    (invert: every digit inverted)."""
    i = np.asarray(indices, dtype=np.int64).reshape(-1)
    v = np.array(np.asarray(vertices, dtype=np.float32).reshape(-1, 8)[i], copy=True)
    t = np.repeat(np.arange(i.size // 3, dtype=np.int64), 3)
    if invert:
        t = t ^ MASK21
    for ch in range(3):
        v[:, 4 + ch] = ((2 * ((t >> (7 * ch)) & 127) + 1) / 255.0).astype(np.float32)
    return v, np.arange(i.size, dtype=np.int64)


def decode(c, invert=False):
    ids = (c[..., 2].astype(np.int64) >> 1) | ((c[..., 1].astype(np.int64) >> 1) << 7) | ((c[..., 0].astype(np.int64) >> 1) << 14)
    if invert:
        ids = ids ^ MASK21
    ids = ids.astype(np.uint32)
    ids[c[..., 3] == 0] = NONE
    assert np.isin(c[..., 3], (0, 255)).all()
    return ids


def expected_ids(oracle, v, i, m, w, h, flags, depth=None):
    """IDs of the clear frame (int64; LIVE where a fragment without a finite colour wins under painter's order).  depth: the
    frame's own depth image, which the coded copies must reproduce bit for bit."""
    dec = []
    for inv in (False, True):
        cv, ci = coded(v, i, inv)
        cc, cd = oracle_clear(oracle, cv, ci, m, w, h, flags & ~NC)
        if depth is not None:
            assert cd.tobytes() == depth.tobytes()
        dec.append(decode(cc, inv))
    rid = np.where(dec[0] == dec[1], dec[0].astype(np.int64), LIVE)
    if flags & (DT | METAL):
        assert (rid != LIVE).all()
    return rid


# ---- face culling ----------------------------------------------------------------------------------------------------------------
def signed_areas(oracle, v, i, m, w, h, flags):
    """A = (bx - ax)(cy - ay) - (cx - ax)(by - ay) of every triangle in int64, from the integer vertices setup rasterises with:
    truncated, or under the Metal rules rounded half away from zero first (0 where setup skips the triangle anyway)."""
    sx, sy, _ = oracle.project(v, m, w, h)
    x, y = sx.astype(np.float64), sy.astype(np.float64)
    with np.errstate(invalid="ignore"):
        if flags & METAL:
            x = np.sign(x) * np.floor(np.abs(x) + 0.5)
            y = np.sign(y) * np.floor(np.abs(y) + 0.5)
        ok = (np.abs(x) < LIMIT) & (np.abs(y) < LIMIT)
        if flags & METAL:
            ok &= (x >= 0) & (y >= 0)
    ix = np.where(ok, np.trunc(np.where(ok, x, 0)), 0).astype(np.int64)
    iy = np.where(ok, np.trunc(np.where(ok, y, 0)), 0).astype(np.int64)
    t = np.asarray(i, dtype=np.int64).reshape(-1, 3)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    area = (ix[b] - ix[a]) * (iy[c] - iy[a]) - (ix[c] - ix[a]) * (iy[b] - iy[a])
    return np.where(ok[a] & ok[b] & ok[c], area, 0)


def kept_triangles(area, flags):
    front = area < 0 if flags & CCW else area > 0
    back = area > 0 if flags & CCW else area < 0
    drop = ((flags & CB) != 0) & back | ((flags & CF) != 0) & front
    return np.nonzero(~drop)[0]


def filtered(oracle, v, i, m, w, h, flags):
    """(index list of the triangles a frame with these cull bits draws, in their order; their original numbers)."""
    keep = kept_triangles(signed_areas(oracle, v, i, m, w, h, flags), flags)
    return np.asarray(i, dtype=np.int64).reshape(-1, 3)[keep].reshape(-1), keep


# ---- one frame's expectation -----------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Expected:
    color: np.ndarray | None
    depth: np.ndarray
    ids: np.ndarray              # int64, original numbering; LIVE / NONE as above
    clear_ids: np.ndarray        # the IDs of the clear frame (before the load rule)
    kept: np.ndarray | None = None


def expected_frame(oracle, v, i, m, w, h, flags, shading=None, start=None, cache=None):
    """Colour, depth and IDs of one frame of the scene (v, i) drawn with m and these flags (cull bits, SWR_FLAG_LOAD over
    start = (c0, d0)).  cache: a dict shared by frames of the same scene and target — one clear frame per (rules, z-test, no
    colour, shader, cull bits), one coded ID pair per (rules, z-test, cull bits)."""
    cache = {} if cache is None else cache
    cull = flags & (CB | CF | CCW)
    key_c = ("clear", flags & (DT | NC | METAL), 0 if shading is None else shading.shader, cull)
    key_i = ("ids", flags & (DT | METAL), cull)
    if ("kept", flags & METAL, cull) not in cache:
        cache[("kept", flags & METAL, cull)] = filtered(oracle, v, i, m, w, h, flags) if cull else (i, None)
    fi, keep = cache[("kept", flags & METAL, cull)]
    if key_c not in cache:
        cache[key_c] = oracle_clear(oracle, v, fi, m, w, h, flags, shading)
    cb, db = cache[key_c]
    if key_i not in cache:
        pos = expected_ids(oracle, v, fi, m, w, h, flags & (DT | METAL), depth=None)
        if keep is not None:
            hit = (pos >= 0) & (pos != NONE)
            pos = pos.copy()
            pos[hit] = keep[pos[hit]]
        cache[key_i] = pos
    rid = cache[key_i]
    if not flags & LOAD:
        return Expected(cb, db, rid, rid, keep)
    c0, d0 = start
    c, d = load_rule(None if cb is None else c0, d0, cb, db, flags, rid)
    return Expected(c, d, load_ids(d0, cb, db, rid, flags), rid, keep)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class VisibleSet:
    vertices: np.ndarray     # float32 [nv, 8], de-indexed
    indices: np.ndarray
    n_head: int              # triangles before the filler position
    tied: np.ndarray         # [k, 2]: (earlier triangle, later duplicate with other colours)


def _ndc(px, py, w, h):
    return px / w * 2.0 - 1.0, 1.0 - py / h * 2.0


def _tris(rng, n, x0, y0, x1, y1, size, z0, z1, w, h):
    """n random triangles with their centres in the pixel box [x0, x1) x [y0, y1) and vertices within `size` pixels."""
    cx = rng.uniform(x0, x1, (n, 1))
    cy = rng.uniform(y0, y1, (n, 1))
    px = np.clip(cx + rng.uniform(-size, size, (n, 3)), x0 - size, x1 + size)
    py = np.clip(cy + rng.uniform(-size, size, (n, 3)), y0 - size, y1 + size)
    x, y = _ndc(px, py, w, h)
    z = rng.uniform(z0, z1, (n, 3))
    xyz = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    rgb = rng.uniform(-0.1, 1.1, (3 * n, 3))
    return xyz, rgb


def _slivers(rng, n, w, h):
    """Triangles whose truncated vertices are collinear (det == 0): horizontal, vertical and diagonal runs and single points."""
    out = []
    for k in range(n):
        x, y = rng.integers(4, w - 40), rng.integers(4, h - 40)
        kind = k % 4
        if kind == 0:
            p = [(x + 0.5, y + 0.5), (x + 20.5, y + 0.5), (x + 9.5, y + 0.25)]
        elif kind == 1:
            p = [(x + 0.25, y + 0.5), (x + 0.75, y + 30.5), (x + 0.5, y + 12.5)]
        elif kind == 2:
            p = [(x + 0.5, y + 0.5), (x + 20.5, y + 20.5), (x + 10.5, y + 10.5)]
        else:
            p = [(x + 0.5, y + 0.5), (x + 0.6, y + 0.4), (x + 0.7, y + 0.9)]
        p = np.asarray(p, dtype=np.float64)
        nx, ny = _ndc(p[:, 0], p[:, 1], w, h)
        z = rng.choice([0.3, -0.2, 0.0, 0.7], 3)
        out.append(np.stack([nx, ny, z], axis=-1))
    xyz = np.concatenate(out)
    return xyz, rng.uniform(-0.1, 1.1, (xyz.shape[0], 3))


def _pack(xyz, rgb):
    v = np.zeros((xyz.shape[0], 8), np.float32)
    v[:, 0:3] = xyz
    v[:, 4:7] = rgb
    return v


def visible_set(w, h, seed=0x3A7):
    """The visible set of the matrix on a w x h target (pixel boxes in the tiles of TILE_W x TILE_H), in index order:
    head: 3 triangles covering most of the screen (far: > 128 tiles each on the large target), 2 of the 4 triangles of a
          tile that holds only them and the big ones (row-split mode), half of 600 medium triangles anywhere else (straddling
          every edge), half of ~1 000 small ones in one tile (chunks, work stealing), half of 4 600 tiny ones in another (more
          than 4 096 entries: no winner table, the per-thread cold path), half of 24 det == 0 slivers;
    tail: duplicates of 64 head triangles with other colours (exact depth ties: the earlier index wins under the z-test, the
          later one under painter's order), 40 strictly nearer triangles, the other halves, and a last triangle nearer than all.
    The filler of the padded scene goes between head and tail: padded to 2^20 + 1 primitives, the tail ends at number 2^20."""
    rng = np.random.default_rng(seed)
    few = (1 * TILE_W + 4, 1 * TILE_H + 4, 2 * TILE_W - 4, 2 * TILE_H - 4)
    busy = (2 * TILE_W, 2 * TILE_H, 3 * TILE_W, 3 * TILE_H)
    crowded = (3 * TILE_W, 4 * TILE_H, 4 * TILE_W, 5 * TILE_H)
    # (inside the screen under every transform of the matrix, or the Metal rules would skip them; two clockwise as displayed, one
    # counter-clockwise, so that every cull setting keeps one)
    big_px = np.array([[[0.08, 0.08], [0.92, 0.15], [0.3, 0.92]],
                       [[0.92, 0.92], [0.85, 0.1], [0.1, 0.85]],
                       [[0.5, 0.08], [0.92, 0.6], [0.08, 0.7]]])
    bx, by = _ndc(big_px[..., 0] * w, big_px[..., 1] * h, w, h)
    big = (np.stack([bx, by, rng.uniform(0.92, 0.99, (3, 3))], axis=-1).reshape(-1, 3), rng.uniform(0, 1, (9, 3)))
    f = _tris(rng, 4, *few, 8, 0.1, 0.8, w, h)
    # medium triangles everywhere but near the sparse tile
    cand = _tris(rng, 1500, -0.05 * w, -0.05 * h, 1.05 * w, 1.05 * h, 14, 0.0, 1.0, w, h)
    cxy = cand[0].reshape(-1, 3, 3)[:, :, :2].mean(axis=1)
    fx0, fy0 = _ndc(few[0] - 40, few[1] - 40, w, h)
    fx1, fy1 = _ndc(few[2] + 40, few[3] + 40, w, h)
    away = ~((cxy[:, 0] > fx0) & (cxy[:, 0] < fx1) & (cxy[:, 1] < fy0) & (cxy[:, 1] > fy1))
    sel = np.nonzero(away)[0][:600]
    soup = (cand[0].reshape(-1, 3, 3)[sel].reshape(-1, 3), cand[1].reshape(-1, 3, 3)[sel].reshape(-1, 3))
    bz = _tris(rng, 1000, *busy, 6, 0.0, 1.0, w, h)
    cr = _tris(rng, 4600, *crowded, 2.5, 0.0, 1.0, w, h)
    sl = _slivers(rng, 24, w, h)
    near = _tris(rng, 40, 0, 0, w, h, 12, -0.6, -0.1, w, h)
    # the last primitive (number 2^20 in the padded scene): nearer than everything, away from the edges
    lx, ly = _ndc(np.array([0.55, 0.75, 0.6]) * w, np.array([0.55, 0.6, 0.8]) * h, w, h)
    last = (np.stack([lx, ly, np.full(3, -0.7)], axis=-1), rng.uniform(0, 1, (3, 3)))

    def part(g, a, b):
        return g[0][3 * a:3 * b], g[1][3 * a:3 * b]

    head = [big, part(f, 0, 2), part(soup, 0, 300), part(bz, 0, 500), part(cr, 0, 2300), part(sl, 0, 12)]
    hxyz = np.concatenate([g[0] for g in head])
    hrgb = np.concatenate([g[1] for g in head])
    n_head = hxyz.shape[0] // 3
    # duplicates: the 2 sparse-tile triangles, 50 medium ones, 12 of the busy tile
    orig = np.concatenate([[3, 4], 5 + rng.choice(300, 50, replace=False), 305 + rng.choice(500, 12, replace=False)])
    dxyz = hxyz.reshape(-1, 3, 3)[orig].reshape(-1, 3)
    drgb = 1.0 - hrgb.reshape(-1, 3, 3)[orig].reshape(-1, 3)[:, ::-1]
    tail = [(dxyz, drgb), near, part(soup, 300, 600), part(bz, 500, 1000), part(cr, 2300, 4600), part(sl, 12, 24), part(f, 2, 4), last]
    xyz = np.concatenate([hxyz] + [g[0] for g in tail])
    rgb = np.concatenate([hrgb] + [g[1] for g in tail])
    v = _pack(xyz, rgb)
    tied = np.stack([orig, n_head + np.arange(orig.size)], axis=1)
    return VisibleSet(v, np.arange(v.shape[0], dtype=np.int64), n_head, tied)


def filler_pool(n=64, seed=0xF11):
    """n finite triangles entirely off the screen (right, left, above, below), for padding scenes past 2^20 primitives."""
    rng = np.random.default_rng(seed)
    side = np.arange(n) % 4
    c = rng.uniform(1.3, 4.0, n)
    t = rng.uniform(-1.5, 1.5, n)
    cx = np.select([side == 0, side == 1], [c, -c], t)
    cy = np.select([side == 2, side == 3], [c, -c], t)
    xyz = np.empty((n, 3, 3))
    xyz[..., 0] = cx[:, None] + rng.uniform(-0.2, 0.2, (n, 3))
    xyz[..., 1] = cy[:, None] + rng.uniform(-0.2, 0.2, (n, 3))
    xyz[..., 2] = rng.uniform(0.0, 1.0, (n, 3))
    return _pack(xyz.reshape(-1, 3), rng.uniform(0, 1, (3 * n, 3)))


def padded(vertices, indices, n_head, total):
    """The scene padded with off-screen filler to `total` triangles, the filler after the first n_head triangles.
    Returns (vertices, indices, number of the first triangle after the filler)."""
    pool = filler_pool()
    nv = vertices.shape[0]
    i = np.asarray(indices, dtype=np.int64)
    nfill = total - i.size // 3
    assert nfill >= 0
    k = np.arange(nfill, dtype=np.int64) % (pool.shape[0] // 3)
    fill = (nv + 3 * k[:, None] + np.arange(3)[None, :]).reshape(-1)
    idx = np.concatenate([i[:3 * n_head], fill, i[3 * n_head:]])
    return np.concatenate([vertices, pool]), idx, n_head + nfill
