"""One expected image for any legal triangle frame: every combination of

    rules {painter, DEPTH_TEST, METAL_RULES} x NO_COLOR x LOAD x PRIMITIVE_IDS x cull {none, BACK, FRONT, BACK|FRONT} x FRONT_CCW
    x DEPTH_CLIP x PERSPECTIVE x shader {0, 1, 2} x {draw, draw list} x transform {affine, perspective}

(include/swr.h refuses none of them).  A plain helper module of tests/test_frame_model.py, tests/test_frame_sequences.py,
tests/test_gpu_fuzz.py and tests/test_perspective.py (not a conftest, not a test file).

No rasteriser is written here.  `expect` composes what the per-feature test files already use, following the header's own "bit for
bit the frame of ..." restatements, in this order:

  draw list    the triangles of the items in item order, each with its item's matrix (test_perspective.model takes one matrix per
               triangle); where no corrected weights are needed, the pre-transformed concatenation drawn with the identity
               (kernel_matrix.concat);
  DEPTH_CLIP   test_depth_clip.restate: the fans in NDC under the identity, the fan -> original map, the fan corners' w;
  culling      kernel_matrix.signed_areas / kept_triangles on the (post-clip) triangles; IDs keep the original numbers;
  pixels       the C oracle, whenever the frame needs no corrected weights (no PERSPECTIVE, or NO_COLOR, or only affine transforms:
               every w is exactly 1 then, fan vertices included); test_perspective.model otherwise, whose depth must be the C oracle's;
  IDs          colour-coded copies drawn twice by the C oracle (kernel_matrix.expected_ids), mapped back to the original numbers;
  LOAD         kernel_matrix.load_rule / load_ids over the starting image.  The C oracle always clears, so it cannot take a starting
               image; test_perspective.model can, and tests/test_frame_model.py checks that passing `start` down to it gives the
               same image as the load rule over its clear frame.  One clear frame thereby serves every load chain it appears in.

Blend frames (SWR_FLAG_BLEND; FrameSpec.blend = (mode, opacity)): every primitive of the frame, in order, is drawn ALONE by the
unchanged oracle as a clear frame under the frame's rule set, which gives its covered pixels, its source bytes and (z-test) its
fragment depths, and folded into the starting image with the header's integer formulas (blend_bytes, primitives, model; written
from the header text alone, moved here from tests/test_blend.py).  Over an unspecified starting colour a pixel becomes specified
only through a contributing fragment that replaces it: SWR_BLEND_OVER with opacity 255.  The starting depth is always specified,
so "contributing" is exact.

`resolved` applies tests/resolve_model.py to a model image: a resolved colour pixel is masked if any of its S x S samples is.

A colour load frame over an image whose colour is unspecified (after a NO_COLOR frame; `start[0] is None`) has a defined colour
only where its own fragments win: the colour comes back as a numpy masked array, the other pixels masked, and a chain keeps the
mask of what is still unspecified.  `same` compares an image the library produced with such an expectation.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import kernel_matrix as K
import resolve_model as RM
import test_depth_clip as DC
import test_perspective as TP

DT, NC, METAL, REAL_LINES, LOAD, IDS = 1, 2, 4, 8, 16, 32
CB, CF, CCW, CLIP, PERSP, BLEND = 64, 128, 256, 1024, 2048, 4096
OVER, ADD = 0, 1
NONE, LIVE = K.NONE, K.LIVE
IDENT = K.IDENT

# the factors of the space above and their values, in the order the covering array and the coverage conditions name them
FACTORS = {
    "rules": ("painter", "ztest", "metal"),
    "no_color": (0, 1),
    "load": (0, 1),
    "ids": (0, 1),
    "cull": ("none", "back", "front", "both"),
    "ccw": (0, 1),
    "clip": (0, 1),
    "persp": (0, 1),
    "shader": (0, 1, 2),
    "list": (0, 1),
    "transform": ("affine", "perspective"),
}
_RULES = {"painter": 0, "ztest": DT, "metal": METAL}
_CULL = {"none": 0, "back": CB, "front": CF, "both": CB | CF}


def flags_of(row):
    """The SWR_FLAG_* bits of a row {factor: value} (shader, list and transform are not flags)."""
    return (_RULES[row["rules"]] | (NC if row["no_color"] else 0) | (LOAD if row["load"] else 0) | (IDS if row["ids"] else 0)
            | _CULL[row["cull"]] | (CCW if row["ccw"] else 0) | (CLIP if row["clip"] else 0) | (PERSP if row["persp"] else 0))


def row_of(flags, shader, is_list, perspective):
    """The factor values of a triangle frame."""
    return {"rules": "metal" if flags & METAL else ("ztest" if flags & DT else "painter"), "no_color": int(bool(flags & NC)),
            "load": int(bool(flags & LOAD)), "ids": int(bool(flags & IDS)),
            "cull": {0: "none", CB: "back", CF: "front", CB | CF: "both"}[flags & (CB | CF)], "ccw": int(bool(flags & CCW)),
            "clip": int(bool(flags & CLIP)), "persp": int(bool(flags & PERSP)), "shader": int(shader), "list": int(bool(is_list)),
            "transform": "perspective" if perspective else "affine"}


def all_pairs_in(factors):
    """Every pair of values of two different factors of a factor table: {((factor a, value), (factor b, value))}, a before b."""
    names = list(factors)
    return {((a, x), (b, y)) for p, a in enumerate(names) for b in names[p + 1:] for x in factors[a] for y in factors[b]}


def pairs_in(row, factors):
    names = list(factors)
    return {((a, row[a]), (b, row[b])) for p, a in enumerate(names) for b in names[p + 1:]}


def greedy_array(factors):
    """A deterministic pairwise covering array over a factor table, greedy: each new row starts from an uncovered pair and gives every
    other factor the value that covers the most pairs still uncovered (ties: the first value)."""
    names = list(factors)
    todo = all_pairs_in(factors)
    rows = []
    while todo:
        (a, x), (b, y) = min(todo, key=repr)
        row = {a: x, b: y}
        for f in names:
            if f in row:
                continue
            def gain(v):
                return sum(1 for g, u in row.items() if (((f, v), (g, u)) if names.index(f) < names.index(g) else ((g, u), (f, v))) in todo)
            row[f] = max(factors[f], key=gain)
        row = {f: row[f] for f in names}
        rows.append(row)
        todo -= pairs_in(row, factors)
    return rows


def all_pairs():
    """Every pair of values of two different factors of FACTORS."""
    return all_pairs_in(FACTORS)


def pairs_of(row):
    return pairs_in(row, FACTORS)


def covering_array():
    """The pairwise covering array over FACTORS (greedy_array)."""
    return greedy_array(FACTORS)


# the blend frames' own space: the factors a blend frame combines with (include/swr.h "Alpha blending", Combinations), its mode and
# the opacities at and next to the identities and in the middle
BLEND_FACTORS = {
    "rules": FACTORS["rules"],
    "load": FACTORS["load"],
    "cull": FACTORS["cull"],
    "ccw": FACTORS["ccw"],
    "clip": FACTORS["clip"],
    "list": FACTORS["list"],
    "transform": FACTORS["transform"],
    "mode": ("over", "add"),
    "opacity": (0, 1, 128, 254, 255),
}
_MODE = {"over": OVER, "add": ADD}


def legal(row):
    """The header's combination rules for a row {factor: value}: a blend frame (a row with a "mode", or with a true "blend") has
    no_color = 0, ids = 0, persp = 0 and shader = 0 (factors a row does not have count as 0); every other row is legal."""
    if row.get("mode") is None and not row.get("blend"):
        return True
    return not (row.get("no_color", 0) or row.get("ids", 0) or row.get("persp", 0) or row.get("shader", 0))


def blend_flags_of(row):
    """The SWR_FLAG_* bits of a BLEND_FACTORS row without SWR_FLAG_BLEND itself, and its (mode, opacity)."""
    flags = (_RULES[row["rules"]] | (LOAD if row["load"] else 0) | _CULL[row["cull"]] | (CCW if row["ccw"] else 0)
             | (CLIP if row["clip"] else 0))
    return flags, (_MODE[row["mode"]], int(row["opacity"]))


def blend_covering_array():
    """greedy_array over BLEND_FACTORS: every row legal by construction."""
    return greedy_array(BLEND_FACTORS)


def is_affine(m):
    """w is exactly 1 for every finite vertex: the last row of the column-major matrix is (0, 0, 0, 1)."""
    m = np.asarray(m, dtype=np.float32).reshape(16)
    return bool(m[3] == 0 and m[7] == 0 and m[11] == 0 and m[15] == 1)


@dataclasses.dataclass
class FrameSpec:
    """One triangle frame.  transform: the matrix of a draw; items: [(first_index, index_count, transform)] of a draw list (then
    transform is ignored).  shading: a scenes.Shading or None (shader 0).  key: a hashable name of (scene, target, transform or items,
    shading) for `expect`'s cache; None: nothing of this frame is cached."""
    vertices: np.ndarray
    indices: np.ndarray
    width: int
    height: int
    flags: int
    transform: np.ndarray | None = None
    items: list | None = None
    shading: object = None
    key: object = None
    blend: tuple | None = None

    @property
    def shader(self):
        return 0 if self.shading is None else int(self.shading.shader)

    def matrices(self):
        return [self.transform] if self.items is None else [m for _, _, m in self.items]

    def row(self):
        return row_of(self.flags, self.shader, self.items is not None, not all(is_affine(m) for m in self.matrices()))


def _triangles(spec):
    """(index triples in draw order [n, 3], one matrix per triangle or the one matrix of a draw)."""
    t = np.asarray(spec.indices, dtype=np.int64).reshape(-1, 3)
    if spec.items is None:
        return t, spec.transform
    parts, ms = [np.zeros((0, 3), dtype=np.int64)], []
    for first, count, m in spec.items:
        parts.append(t[first // 3:(first + count) // 3])
        ms += [m] * (count // 3)
    return np.concatenate(parts), ms


def _geometry(spec):
    """The frame's triangles before culling, twice: `flat` = (vertices, index triples, matrix, attributes) for the C oracle, the
    signed areas and the coded IDs (the restated scene under the identity for clip frames and draw lists); `per` = (vertices, index
    triples, matrices, rw, attributes) for test_perspective.model; fmap: triangle -> original number (None: its own)."""
    v = np.asarray(spec.vertices, dtype=np.float32).reshape(-1, 8)
    attrs = None if spec.shading is None else spec.shading.attrs
    t, ms = _triangles(spec)
    if spec.flags & CLIP:
        V, A, I, fmap, fans = DC.restate(v, t.reshape(-1), ms if spec.items is None or len(ms) else IDENT, attrs)
        rw = np.array([(poly[0][3], poly[s][3], poly[s + 1][3]) for poly in fans for s in range(1, len(poly) - 1)],
                      dtype=np.float32).reshape(-1, 3)
        T = I.reshape(-1, 3)
        return (V, T, IDENT, A), (V, T, IDENT, rw, A), fmap
    if spec.items is None:
        return (v, t, ms, attrs), (v, t, ms, None, attrs), None
    if not spec.items:
        return (v, t, IDENT, attrs), (v, t, IDENT, None, attrs), None
    cv, ci = K.concat(v, np.asarray(spec.indices, dtype=np.int64).reshape(-1), spec.items)
    ca = None if attrs is None else np.concatenate([np.asarray(attrs, dtype=np.float32).reshape(-1, 8)] * len(spec.items))
    return (cv, ci.reshape(-1, 3), IDENT, ca), (v, t, ms, None, attrs), None


def _with_attrs(shading, attrs):
    return None if shading is None else dataclasses.replace(shading, attrs=attrs)


def clear_frame(oracle, spec, cache=None):
    """(colour or None, depth, IDs or None) of the frame without SWR_FLAG_LOAD.  IDs (int64, original numbers, LIVE / NONE as in
    kernel_matrix) are computed with the flag, and for a painter's-order NO_COLOR frame (the load rule reads its coverage there)."""
    flags, w, h = spec.flags, spec.width, spec.height
    cache = cache if cache is not None and spec.key is not None else {}
    rules, cull = flags & (DT | METAL), flags & (CB | CF | CCW)

    def memo(key, make):
        key = (spec.key,) + key
        if key not in cache:
            cache[key] = make()
        return cache[key]

    flat, per, fmap = memo(("geometry", flags & CLIP), lambda: _geometry(spec))
    fv, ft, fm, fa = flat

    def kept():
        if not cull or ft.shape[0] == 0:
            return None
        return K.kept_triangles(K.signed_areas(oracle, fv, ft.reshape(-1), fm, w, h, flags), flags)
    keep = memo(("kept", flags & CLIP, flags & METAL, cull), kept)
    sel = slice(None) if keep is None else keep
    fi = ft[sel].reshape(-1)

    use_model = bool(flags & PERSP) and not flags & NC and not all(is_affine(m) for m in spec.matrices())

    def pixels():
        c, d = K.oracle_clear(oracle, fv, fi, fm, w, h, flags, _with_attrs(spec.shading, fa))
        if use_model:
            pv, pt, pm, rw, pa = per
            ms = [pm[k] for k in (range(len(pm)) if keep is None else keep)] if isinstance(pm, list) else pm
            c, dm = TP.model(pv, pt[sel].reshape(-1), ms, w, h, rules, _with_attrs(spec.shading, pa),
                             rw=None if rw is None else rw[sel])
            assert dm.tobytes() == d.tobytes(), "the model's depth is not the C oracle's"
        return c, d
    cb, db = memo(("pixels", flags & CLIP, rules, flags & NC, cull, spec.shader if not flags & NC else 0, use_model), pixels)

    rid = None
    if flags & IDS or (flags & LOAD and flags & NC and not rules):
        def ids():
            pos = K.expected_ids(oracle, fv, fi, fm, w, h, rules, depth=db)
            orig = fmap if fmap is not None else None
            if keep is not None:
                orig = keep if orig is None else orig[keep]
            if orig is not None:
                hit = (pos >= 0) & (pos != NONE)
                pos = pos.copy()
                pos[hit] = orig[pos[hit]]
            return pos
        rid = memo(("ids", flags & CLIP, rules, cull), ids)
    return cb, db, rid


# ---- blend frames ------------------------------------------------------------------------------------------------------------------
def blend_bytes(s, d, A, mode):
    """The header's arithmetic, per channel, on integer arrays."""
    s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
    if mode == OVER:
        return (s * A + d * (255 - A) + 127) // 255
    return np.minimum(255, d + (s * A + 127) // 255)


def primitives(oracle, spec):
    """[(number, y0, x0, source colour BGRA with alpha 255 where covered, fragment depths or None)] of the frame's primitives in order
    (number: the triangle's place in the frame's stream, fans counted, before culling),
    after depth clipping (fans, in their original's place) and face culling; each drawn alone by the oracle, its images cut down to
    the rows and columns it covers (nothing else of them is looked at)."""
    flags, w, h = spec.flags, spec.width, spec.height
    (fv, ft, fm, _), _, _ = _geometry(spec)
    keep = np.arange(ft.shape[0])
    if flags & (CB | CF) and ft.shape[0]:
        keep = K.kept_triangles(K.signed_areas(oracle, fv, ft.reshape(-1), fm, w, h, flags), flags)
    out, tri = [], np.arange(3, dtype=np.int64)
    for p in keep:
        v3 = np.ascontiguousarray(fv[ft[p]])
        if flags & METAL:
            c, d = K.oracle_clear(oracle, v3, tri, fm, w, h, METAL)
        else:
            c, _ = K.oracle_clear(oracle, v3, tri, fm, w, h, 0)
            d = K.oracle_clear(oracle, v3, tri, fm, w, h, DT | NC)[1] if flags & DT else None
        cov = c[..., 3] == 255
        ys, xs = np.nonzero(cov.any(axis=1))[0], np.nonzero(cov.any(axis=0))[0]
        if ys.size == 0:
            continue
        y0, y1, x0, x1 = ys[0], ys[-1] + 1, xs[0], xs[-1] + 1
        out.append((int(p), int(y0), int(x0), c[y0:y1, x0:x1].copy(), None if d is None else d[y0:y1, x0:x1].copy()))
    return out


_PRIMS = {}


def _cached_primitives(oracle, spec, cache=None):
    """primitives(spec), kept by spec.key and the flags that change them (in `cache`, or in the module's own)."""
    cache = _PRIMS if cache is None else cache
    if spec.key is None:
        return primitives(oracle, spec)
    key = ("prims", spec.key, spec.flags & ~(LOAD | BLEND))
    if key not in cache:
        cache[key] = primitives(oracle, spec)
    return cache[key]


def _blend_fold(oracle, spec, mode, opacity, c, d0, unknown=None, cache=None):
    """Folds the frame's primitives into the colour image c (in place) against the starting depth d0; unknown (in place): the
    pixels whose colour is still unspecified."""
    for _, y0, x0, cs, ds in _cached_primitives(oracle, spec, cache):
        box = (slice(y0, y0 + cs.shape[0]), slice(x0, x0 + cs.shape[1]))
        hit = cs[..., 3] == 255
        if ds is not None:
            with np.errstate(invalid="ignore"):
                hit = hit & (ds < d0[box])                  # strict '<' against the STARTING depth; NaN and +inf never pass
        if hit.any():
            src = cs[hit].astype(np.int64)
            src[:, 3] = 255
            part = c[box]
            part[hit] = blend_bytes(src, part[hit], opacity, mode).astype(np.uint8)
            if unknown is not None and mode == OVER and opacity == 255:
                unknown[box][hit] = False                   # replaced: whatever was there does not show
    return c


def contributions(oracle, spec, start=None, cache=None):
    """What a blend frame's fragments do at every pixel, for the tests' own non-vacuity checks: (contributing fragments per pixel,
    covering fragments the starting depth rejects per pixel, the numbers of the primitives with a contributing fragment)."""
    h, w = spec.height, spec.width
    d0 = np.full((h, w), np.inf, dtype=np.float32) if start is None or not spec.flags & LOAD else start[1]
    prims = _cached_primitives(oracle, spec, cache)
    passed, rejected, who = np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64), []
    for p, y0, x0, cs, ds in prims:
        box = (slice(y0, y0 + cs.shape[0]), slice(x0, x0 + cs.shape[1]))
        cov = cs[..., 3] == 255
        hit = cov
        if ds is not None:
            with np.errstate(invalid="ignore"):
                hit = cov & (ds < d0[box])
        passed[box] += hit
        rejected[box] += cov & ~hit
        if hit.any():
            who.append(p)
    return passed, rejected, np.asarray(who, dtype=np.int64)


def model(oracle, spec, mode, opacity, start=None, cache=None):
    """(colour, depth) of the blend frame `spec` (flags without the BLEND bit) over `start` = (colour, depth), or over the cleared
    image.  The per-primitive images are cached by spec.key (in `cache`, or in the module's own): they do not depend on mode or
    opacity."""
    h, w = spec.height, spec.width
    if start is None or not spec.flags & LOAD:
        c, d0 = np.zeros((h, w, 4), dtype=np.uint8), np.full((h, w), np.inf, dtype=np.float32)
    else:
        c, d0 = np.array(start[0], copy=True), np.array(start[1], copy=True)
    return _blend_fold(oracle, spec, mode, opacity, c, d0, cache=cache), d0


def _expect_blend(oracle, spec, start, cache):
    assert not spec.flags & (NC | IDS | PERSP) and spec.shader == 0, "not a legal blend frame (include/swr.h, Combinations)"
    mode, opacity = spec.blend
    h, w = spec.height, spec.width
    if not spec.flags & LOAD or start is None:
        return (*model(oracle, spec, mode, opacity, None, cache), None)
    c0, d0 = start
    d0 = np.array(d0, copy=True)
    unknown = None
    if c0 is None:
        c, unknown = np.zeros((h, w, 4), dtype=np.uint8), np.ones((h, w), dtype=bool)
    elif isinstance(c0, np.ma.MaskedArray):
        c, unknown = np.array(c0.data, copy=True), np.ma.getmaskarray(c0)[..., 0].copy()
    else:
        c = np.array(c0, copy=True)
    _blend_fold(oracle, spec, mode, opacity, c, d0, unknown, cache)
    if unknown is not None and unknown.any():
        c = np.ma.masked_array(c, mask=np.repeat(unknown[..., None], 4, axis=-1))
    return c, d0, None


def resolved(image, S, depth_filter):
    """(colour or None, depth, None) of a model image (colour or None, depth, ...) through the S x S resolve of
    tests/resolve_model.py.  A resolved colour pixel is masked if any of its samples is; depth is never masked."""
    c, d = image[0], image[1]
    if S == 1:
        return c, d, None
    rc = None
    if c is not None:
        rc = RM.color(np.ascontiguousarray(np.ma.getdata(c)), S)
        if isinstance(c, np.ma.MaskedArray):
            m = np.ma.getmaskarray(c)[..., 0]
            h, w = m.shape
            any_masked = m.reshape(h // S, S, w // S, S).any(axis=(1, 3))
            if any_masked.any():
                rc = np.ma.masked_array(rc, mask=np.repeat(any_masked[..., None], 4, axis=-1))
    return rc, RM.depth(d, S, depth_filter), None


def expect(oracle, spec, start=None, cache=None):
    """(colour or None, depth, ids or None) of the frame `spec`; start = (colour or None, depth), the image a SWR_FLAG_LOAD frame is
    drawn over (None: the cleared image).  cache: a dict shared by the frames of a test (see FrameSpec.key).  A blend frame
    (spec.blend) gives (colour, the starting depth, None)."""
    if spec.blend is not None:
        return _expect_blend(oracle, spec, start, cache)
    cb, db, rid = clear_frame(oracle, spec, cache)
    flags = spec.flags
    if not flags & LOAD or start is None:
        return cb, db, (rid if flags & IDS else None)
    c0, d0 = start
    unknown = None                                       # pixels of the starting colour that are unspecified
    if cb is not None:
        if c0 is None:
            c0, unknown = np.zeros_like(cb), np.ones(db.shape, dtype=bool)
        elif isinstance(c0, np.ma.MaskedArray):
            c0, unknown = np.asarray(c0.data), np.ma.getmaskarray(c0)[..., 0]
    c, d = K.load_rule(c0 if cb is not None else None, d0, cb, db, flags, rid)
    if unknown is not None:
        unknown = unknown & ~K.load_wins(d0, cb, db, flags, rid)
        if unknown.any():
            c = np.ma.masked_array(c, mask=np.repeat(unknown[..., None], 4, axis=-1))
    ids = K.load_ids(d0, cb, db, rid, flags) if flags & IDS else None
    return c, d, ids


def same(got, want, what=""):
    """Compare (colour or None, depth or None, ids or None) of the library with an expectation, bit for bit; images the library did
    not give (None) are skipped, masked colour pixels are unspecified, LIVE IDs must be some triangle."""
    gc, gd, gi = got
    wc, wd, wi = want
    if gd is not None:
        bad = np.nonzero(gd.view(np.uint32) != wd.view(np.uint32))
        assert bad[0].size == 0, f"{what}: {bad[0].size} depth values differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): " \
                                 f"{gd[bad][0]!r} vs {wd[bad][0]!r}"
    if gc is not None and wc is not None:
        diff = (gc != np.asarray(np.ma.getdata(wc))).any(axis=-1)
        if isinstance(wc, np.ma.MaskedArray):
            diff &= ~np.ma.getmaskarray(wc)[..., 0]
        bad = np.nonzero(diff)
        assert bad[0].size == 0, f"{what}: {bad[0].size} colour pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): " \
                                 f"{gc[bad[0][0], bad[1][0]]} vs {np.ma.getdata(wc)[bad[0][0], bad[1][0]]}"
    if gi is not None:
        assert wi is not None, f"{what}: no expected IDs"
        live = wi == LIVE
        assert (gi[live] != NONE).all(), f"{what}: a pixel some fragment wins has no ID"
        bad = np.nonzero((gi.astype(np.int64) != wi) & ~live)
        assert bad[0].size == 0, f"{what}: {bad[0].size} IDs differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): " \
                                 f"{gi[bad][0]} vs {wi[bad][0]}"
