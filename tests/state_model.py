"""The context as include/swr.h describes it, in NumPy: what one swr_context holds between calls — the scene, its attributes, skin,
pose (matrices or dual quaternions), morph targets (dense or sparse: one morph state of two kinds) and weights, the material, the target, the last frame's image, whether its IDs
are readable, and the delta baselines — and what every observer must answer from that state.  Written from the header's lifetime
and completion paragraphs, not from swr_api.hip.  A plain helper module of tests/test_state_sequences.py (GPU) and
tests/test_state_model.py (CPU): not a conftest, not a test file.

Nothing is rasterised here.  The model composes the per-feature models the suite already has:

  shape      tests/morph_model.py or, for sparse targets, tests/morph_sparse_model.py (morph first), then tests/skin_model.py or
             tests/skin_dq_model.py (the pose in effect);
  frames     tests/frame_model.py `expect` over the shape's vertices and attributes ("every frame, read and query after the call is
             bit for bit that of a context on which swr_scene_upload was given the morphed-then-posed vertices"); a SWR_FLAG_LOAD
             frame starts from the model's own previous image;
  counts     np.bincount over the model's IDs inside the rectangle, per item through binding.list_ids_to_items;
  queries    tests/test_depth_query.py `expected` over the model's depth;
  bounds     tests/item_bounds_model.py over the shape's vertices;
  deltas     tests/delta_model.py over the baseline the model keeps per image kind;
  resolves   frame_model.resolved.

A call the header refuses raises `Refused(code)` and leaves the state as it was."""
from __future__ import annotations

import dataclasses
import hashlib

import numpy as np

import delta_model as DM
import frame_model as FM
import item_bounds_model as IB
import morph_model as MM
import morph_sparse_model as MS
import normals_model as NM
import rays_model as RM
import skin_dq_model as DQ
import skin_model as SM

BAD_ARG, UNSUPPORTED, NO_SCENE = -1, -5, -6
DT, NC, METAL, REAL_LINES, LOAD, IDS, CLIP = FM.DT, FM.NC, FM.METAL, FM.REAL_LINES, FM.LOAD, FM.IDS, FM.CLIP
COUNT_PER_PRIMITIVE, COUNT_PER_ITEM = 0, 1
DELTA_COLOR, DELTA_DEPTH = 1, 2
ID_NONE = 0xFFFFFFFF
TRI, LINE, VERTICES = 0, 1, 2
TILE_W, TILE_H = 64, 32
MORPH_MAX_TARGETS = 256                                     # SWR_MORPH_MAX_TARGETS
DENSE, SPARSE = "dense", "sparse"
UPLOADED, SMOOTH, FLAT, FLIP = NM.UPLOADED, NM.SMOOTH, NM.FLAT, NM.FLIP     # SWR_NORMALS_*
RAYS_MAX = RM.RAYS_MAX                                      # SWR_RAYS_MAX


class Refused(Exception):
    """A call include/swr.h says fails (without a sticky error): the code it returns."""

    def __init__(self, code, why=""):
        super().__init__(f"{code}: {why}")
        self.code = code


def digest(*arrays):
    """A short name of the content of some arrays (None: its own name)."""
    h = hashlib.sha1()
    for a in arrays:
        if a is None:
            h.update(b"none")
        else:
            a = np.ascontiguousarray(a)
            h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()[:16]


def items_key(items):
    return digest(*[np.concatenate([np.array([f, n], dtype=np.float64), np.asarray(m, dtype=np.float64).reshape(16)]) for f, n, m in items]) \
        if items else "empty"


@dataclasses.dataclass
class Last:
    """The last frame: what swr_count_ids measures its `n` against."""
    kind: int = TRI
    flags: int = 0
    prims: int = 0
    items: list | None = None       # the draw list, or None


class State:
    def __init__(self, oracle, cache=None, shapes=None, casts=None):
        self.oracle = oracle
        self.cache = {} if cache is None else cache         # frame_model's clear frames, by (shape id, ...)
        self.shapes = {} if shapes is None else shapes      # shape key -> (vertices, attrs or None)
        self.v = self.i = None
        self.scene = None                                   # digest of the uploaded arrays
        self.attrs = None
        self.skin = None                                    # (joint, weight, digest)
        self.pose_kind, self.pose, self.pose_id = None, None, None
        # one morph state of two kinds ("Sparse morph targets": the targets in effect are those of the last call of either entry)
        self.targets = None                                 # dense: (position deltas, normal deltas or None, digest);
        self.kind = None                                    # sparse: ([(indices, position deltas[, normal deltas])], normals?, digest)
        self.weights, self.weights_id = None, None
        self.normals = None                                 # "Computed normals": (SMOOTH | FLAT, flip) or None (as uploaded)
        self.flat = {}                                      # shape id -> the de-indexed scene a lit frame draws under FLAT
        self.casts = {} if casts is None else casts         # (positions, rays) -> hits (the model's answers are kept: a set is cast often)
        self.material = None                                # a scenes.Shading (its attrs are not looked at) or None
        self.size = None
        self.image = None                                   # (colour or None or masked, depth, IDs or None)
        self.cleared = False                                # right after swr_target_set: reads are not issued, queries see +inf
        self.ids_ok = False
        self.last = None
        self.baseline = {DELTA_COLOR: None, DELTA_DEPTH: None}

    # ---- the scene ----------------------------------------------------------------------------------------------------------------
    def upload(self, v, i):
        """A new scene discards attributes, skin, pose, targets, weights and the normals mode, and makes the IDs unreadable: they
        number the primitives of the scene that is gone (the colour and depth images and the target stay)."""
        self.v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 8)
        self.i = np.ascontiguousarray(i, dtype=np.int64).reshape(-1)
        self.scene = digest(self.v, self.i)
        self.attrs = self.skin = self.targets = self.kind = None
        self.pose_kind = self.pose = self.pose_id = None
        self.weights = self.weights_id = None
        self.normals = None
        self.ids_ok = False

    def _need_scene(self):
        if self.v is None:
            raise Refused(NO_SCENE, "no scene")

    def attributes(self, attrs):
        self._need_scene()
        a = np.ascontiguousarray(attrs, dtype=np.float32).reshape(-1, 8)
        if a.shape[0] != self.v.shape[0]:
            raise Refused(BAD_ARG, "attribute count")
        self.attrs = a

    def set_skin(self, joint, weight):
        """A new skin — and none — restores the bind pose; the weights stay."""
        self._need_scene()
        if joint is None:
            self.skin = None
        else:
            j = np.asarray(joint).reshape(-1, 4).astype(np.int64)
            w = np.asarray(weight, dtype=np.float32).reshape(-1, 4)
            if j.shape[0] != self.v.shape[0]:
                raise Refused(BAD_ARG, "skin count")
            self.skin = (j, w, digest(j, w))
        self.pose_kind = self.pose = self.pose_id = None

    def set_pose(self, kind, table):
        """kind "mat" (swr_pose_set, J x 16) or "dq" (swr_pose_set_dq, J x 8); table None: the bind pose, through either entry."""
        self._need_scene()
        if self.skin is None:
            raise Refused(BAD_ARG, "no skin")
        if table is None:
            self.pose_kind = self.pose = self.pose_id = None
            return
        t = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 16 if kind == "mat" else 8)
        if t.shape[0] <= int(self.skin[0].max()):
            raise Refused(BAD_ARG, "fewer joints than the skin uses")
        self.pose_kind, self.pose, self.pose_id = kind, t, digest(t)

    def set_targets(self, dp, dn=None):
        """swr_scene_morph.  New targets — and none — set every weight to 0; skin and pose stay.  None removes whichever kind is
        resident."""
        self._need_scene()
        if dp is None:
            self.targets = self.kind = None
        else:
            dp = np.ascontiguousarray(dp, dtype=np.float32)
            if dp.ndim != 3 or dp.shape[1] != self.v.shape[0]:
                raise Refused(BAD_ARG, "target vertex count")
            if dp.shape[0] > MORPH_MAX_TARGETS:
                raise Refused(UNSUPPORTED, "more than SWR_MORPH_MAX_TARGETS targets")
            dn = None if dn is None else np.ascontiguousarray(dn, dtype=np.float32)
            self.targets, self.kind = (dp, dn, digest(dp, dn)), DENSE
        self.weights = self.weights_id = None

    def set_targets_sparse(self, targets, vertex_count=None):
        """swr_scene_morph_sparse: targets is a list of (indices, position deltas[, normal deltas]) or None (which removes whichever
        kind is resident); vertex_count: what the caller says the scene has (default: what it has).  Every check is made before
        anything changes.  New targets set every weight to 0; skin and pose stay."""
        self._need_scene()
        if targets is None:
            self.targets = self.kind = None
            self.weights = self.weights_id = None
            return
        nv = self.v.shape[0]
        if (nv if vertex_count is None else vertex_count) != nv:
            raise Refused(BAD_ARG, "a vertex_count that does not match the scene")
        if len(targets) < 1:
            raise Refused(BAD_ARG, "target_count < 1")
        if len(targets) > MORPH_MAX_TARGETS:
            raise Refused(UNSUPPORTED, "more than SWR_MORPH_MAX_TARGETS targets")
        kept, normals = [], set()
        for k, t in enumerate(targets):
            idx = np.ascontiguousarray(t[0], dtype=np.int64).reshape(-1)
            dp = np.ascontiguousarray(t[1], dtype=np.float32).reshape(-1, 3)
            dn = np.ascontiguousarray(t[2], dtype=np.float32).reshape(-1, 3) if len(t) > 2 and t[2] is not None else None
            if idx.size > nv:
                raise Refused(BAD_ARG, f"target {k}: count > vertex_count")
            if idx.size == 0:
                kept.append((idx.astype(np.uint32), dp))    # (an empty target: its pointers are not looked at)
                continue
            if idx.min() < 0 or idx.max() >= nv:
                raise Refused(BAD_ARG, f"target {k}: an index >= vertex_count")
            if not (np.diff(idx) > 0).all():
                raise Refused(BAD_ARG, f"target {k}: indices not strictly ascending")
            assert dp.shape[0] == idx.size and (dn is None or dn.shape[0] == idx.size), "the binding refuses these itself"
            normals.add(dn is not None)
            kept.append((idx.astype(np.uint32), dp) if dn is None else (idx.astype(np.uint32), dp, dn))
        if len(normals) > 1:
            raise Refused(BAD_ARG, "normal deltas on some non-empty targets only")
        self.targets = (kept, normals == {True}, digest(*[x for t in kept for x in t]) + f"/{len(kept)}")
        self.kind = SPARSE
        self.weights = self.weights_id = None

    def target_count(self):
        return 0 if self.targets is None else len(self.targets[0]) if self.kind == SPARSE else self.targets[0].shape[0]

    def set_weights(self, w):
        """swr_morph_set serves both kinds: one weight per target, the same errors."""
        self._need_scene()
        if self.targets is None:
            raise Refused(BAD_ARG, "no targets")
        if w is None:
            self.weights = self.weights_id = None
            return
        w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
        if w.shape[0] != self.target_count():
            raise Refused(BAD_ARG, "weight count")
        if (w != np.float32(0)).any():
            self.weights, self.weights_id = w, digest(w)
        else:
            self.weights = self.weights_id = None           # (+0 and -0: bit for bit what the upload built)

    def morph_pose(self, weights, kind, table):
        """swr_morph_pose_set: set_weights, then set_pose (kind "mat": SWR_POSE_MATRICES, "dq": SWR_POSE_DUAL_QUATS), with every check
        of both halves made before either changes anything: a refusal leaves the weights and the pose as they were.  It needs
        targets (of either kind) and a skin."""
        self._need_scene()
        if kind not in ("mat", "dq"):
            raise Refused(BAD_ARG, "an unknown pose_kind")
        held = (self.weights, self.weights_id, self.pose_kind, self.pose, self.pose_id)
        try:
            self.set_weights(weights)
            self.set_pose(kind, table)
        except Refused:
            self.weights, self.weights_id, self.pose_kind, self.pose, self.pose_id = held
            raise

    def set_normals(self, mode, flags=0, reserved=(0, 0)):
        """swr_scene_normals (mode None: NULL, which means UPLOADED).  Every check is made before anything changes.  The mode follows
        the upload it belongs to; it is in effect only while the scene has attributes and is kept when it is set earlier.  It
        changes no image, no ID and no baseline: the last frame stays as it was drawn."""
        self._need_scene()
        if mode is None:
            mode, flags, reserved = UPLOADED, 0, (0, 0)
        if mode not in (UPLOADED, SMOOTH, FLAT):
            raise Refused(BAD_ARG, "an unknown mode")
        if flags & ~FLIP:
            raise Refused(BAD_ARG, "unknown flag bits")
        if any(reserved):
            raise Refused(BAD_ARG, "a non-zero reserved word")
        self.normals = None if mode == UPLOADED else (mode, bool(flags & FLIP))

    def mode(self):
        """The computed mode in effect — (SMOOTH | FLAT, flip) — or None: it needs attributes."""
        return self.normals if self.attrs is not None else None

    def set_material(self, shading):
        self.material = shading if shading is not None and shading.shader else None

    # ---- the shape the frames draw ------------------------------------------------------------------------------------------------
    def shape_key(self):
        morph = (self.kind, self.targets[2], self.weights_id) if self.weights is not None else None
        pose = (self.skin[2], self.pose_kind, self.pose_id) if self.pose is not None else None
        attrs = None if self.attrs is None else digest(self.attrs)
        return (self.scene, attrs, morph, pose) + ((self.mode(),) if self.mode() is not None else ())

    def morphed(self):
        """(vertices, attributes or None) under the weights, before the pose.  Sparse targets take the loop of "Sparse morph
        targets" — a vertex a target does not list is not touched by it, which the dense target with zero rows does not say — and
        move normals only when their non-empty targets carry normal deltas."""
        v, a = self.v, self.attrs
        if self.weights is not None and self.kind == SPARSE:
            lists, normals, _ = self.targets
            v = MS.morph_vertices(v, lists, self.weights)
            if a is not None and normals:
                a = MS.morph_attrs(a, lists, self.weights)
        elif self.weights is not None:
            dp, dn, _ = self.targets
            v = MM.morph_vertices(v, dp, self.weights)
            if a is not None:
                a = MM.morph_attrs(a, dn, self.weights)
        return v, a

    def shape(self):
        """(vertices, attributes or None, id) of the resident, indexed scene as it is now: morphed, then posed, then — under
        SWR_NORMALS_SMOOTH — with the n_i of the posed vertices for normals (normal deltas and the normal half of the pose are left
        out).  Under SWR_NORMALS_FLAT the attributes are the morphed-and-posed ones: what a lit frame draws is `drawn`."""
        key = self.shape_key()
        if key not in self.shapes:
            v, a = self.morphed()
            if self.pose is not None:
                P = SM if self.pose_kind == "mat" else DQ
                j, w, _ = self.skin
                v = P.pose_vertices(v, j, w, self.pose)
                if a is not None:
                    a = P.pose_attrs(a, j, w, self.pose)
            if self.mode() is not None and self.mode()[0] == SMOOTH:
                _, a, _ = NM.expected_scene(SMOOTH, v, self.attrs, self.i, self.mode()[1])
            self.shapes[key] = (np.ascontiguousarray(v), None if a is None else np.ascontiguousarray(a), len(self.shapes))
        return self.shapes[key]

    def drawn(self):
        """(vertices, attributes or None, indices, id) of what a frame that reads normals draws: the indexed scene, or, under
        SWR_NORMALS_FLAT, the de-indexed one — vertex 3p + k is corner k of triangle p and carries f_p.  Index positions are the
        same in both, so draw-list ranges, primitive IDs and counts carry over."""
        v, a, sid = self.shape()
        if self.mode() is None or self.mode()[0] != FLAT:
            return v, a, self.i, sid
        if sid not in self.flat:
            self.flat[sid] = NM.expected_scene(FLAT, v, self.attrs, self.i, self.mode()[1])
        return self.flat[sid] + (sid,)

    # ---- the target ---------------------------------------------------------------------------------------------------------------
    def target_set(self, w, h):
        """The image is the cleared one and its IDs are gone; a baseline is dropped only when the size changes."""
        if self.size != (w, h):
            self.baseline = {DELTA_COLOR: None, DELTA_DEPTH: None}
        self.size = (w, h)
        self.image = (np.zeros((h, w, 4), dtype=np.uint8), np.full((h, w), np.inf, dtype=np.float32), None)
        self.cleared = True
        self.ids_ok = False

    def target_write(self, color, depth):
        """Either image may be None: that image stays as it is (the cleared one right after swr_target_set)."""
        c = self.image[0] if color is None else np.array(color, copy=True)
        d = self.image[1] if depth is None else np.array(depth, copy=True)
        self.image = (c, d, None)
        self.cleared = False
        self.ids_ok = False

    def delta_reset(self, bits):
        if not bits or bits & ~(DELTA_COLOR | DELTA_DEPTH):
            raise Refused(BAD_ARG, "delta bits")
        for b in (DELTA_COLOR, DELTA_DEPTH):
            if bits & b:
                self.baseline[b] = None

    # ---- frames -------------------------------------------------------------------------------------------------------------------
    def frame(self, flags, transform=None, items=None, kind=TRI):
        """One frame (swr_draw, swr_draw_primitives, swr_draw_list) in the shape the scene has now; returns its model image."""
        self._need_scene()
        if self.size is None:
            raise Refused(NO_SCENE, "no target")
        w, h = self.size
        v, a, sid = self.shape()
        if kind == TRI:
            shading, idx = None, self.i
            if self.material is not None and not flags & NC:
                if a is None:
                    raise Refused(BAD_ARG, "a Phong material without attributes")
                v, a, idx, sid = self.drawn()               # (depth-only frames and the passthrough shader read no normals)
                shading = dataclasses.replace(self.material, attrs=a)
            tkey = digest(transform) if items is None else items_key(items)
            spec = FM.FrameSpec(v, idx, w, h, flags, transform, items, shading,
                                key=("state", sid, w, h, tkey, 0 if shading is None else shading.shader))
            start = None
            if flags & LOAD and not self.cleared:
                start = self.image[:2]
            c, d, ids = FM.expect(self.oracle, spec, start, self.cache)
            prims = self.i.size // 3 if items is None else int(sum(n // 3 for _, n, _ in items))
        else:
            assert not flags & (LOAD | IDS) and items is None
            c, d, _, code = self.oracle.render(v, self.i, transform, w, h, flags & REAL_LINES, primitive_type=kind)
            assert code == 0
            ids, prims = None, self.i.size // 3
        self.image = (c, d, ids)
        self.cleared = False
        self.ids_ok = bool(flags & IDS)
        self.last = Last(kind, flags, prims, None if items is None else list(items))
        return self.image

    def render(self, v, i, transform, w, h, flags, shading=None, start=None):
        """swr_render: the upload it performs (which discards skin, pose and targets), the pass's own fragment stage, its target,
        its starting image under SWR_FLAG_LOAD, one frame."""
        self.upload(v, i)
        if shading is not None:
            self.attributes(shading.attrs)
        self.set_material(shading)
        self.target_set(w, h)
        if flags & LOAD:
            self.target_write(None if flags & NC else start[0], start[1])
        return self.frame(flags, transform)

    # ---- observers: none of them changes anything but a delta read its own baseline ---------------------------------------------------
    def read(self):
        assert self.image is not None and not self.cleared, "the generator reads no image the header leaves unspecified"
        return self.image

    def read_ids(self):
        if not self.ids_ok:
            raise Refused(BAD_ARG, "no readable IDs")
        return self.image[2]

    def count(self, group, rect, n, items_to_ids):
        """(counts, none) over the rectangle (x0, y0, x1, y1); items_to_ids: binding.list_ids_to_items."""
        if not self.ids_ok:
            raise Refused(BAD_ARG, "no readable IDs")
        need = (1 if self.last.items is None else len(self.last.items)) if group == COUNT_PER_ITEM else self.last.prims
        if n != need:
            raise Refused(BAD_ARG, f"n is {n}, the last frame has {need}")
        x0, y0, x1, y1 = rect
        ids = self.image[2][y0:y1, x0:x1]
        assert not (ids == FM.LIVE).any(), "a counted frame must have determined IDs"
        none = int((ids == FM.NONE).sum())
        hit = ids[ids != FM.NONE]
        if group == COUNT_PER_ITEM:
            if self.last.items is None:
                counts = np.array([hit.size], dtype=np.uint32)
            else:
                k, _ = items_to_ids(hit.astype(np.uint32), self.last.items)
                counts = np.bincount(k, minlength=n).astype(np.uint32)
        else:
            counts = np.bincount(hit, minlength=n).astype(np.uint32)
        assert counts.size == n and int(counts.sum()) + none == (x1 - x0) * (y1 - y0)
        return counts, none

    def depth(self):
        return self.image[1]

    def bounds(self, items, flags=0):
        self._need_scene()
        if flags & CLIP:
            raise Refused(UNSUPPORTED, "SWR_FLAG_DEPTH_CLIP")
        v, _, _ = self.shape()
        return IB.item_bounds(v, self.i, items, self.size[0], self.size[1], flags)

    def cast(self, rays, n=None, flags=0):
        """swr_cast_rays: rays_model.cast over the triangles of the shape's vertices and the scene's indices.  It needs a scene
        only — no target, no frame — and changes nothing.  n: what the caller says the array holds (default: what it holds)."""
        self._need_scene()
        rays = np.ascontiguousarray(rays, dtype=RM.RAY_DTYPE).reshape(-1)
        n = rays.size if n is None else n
        if n < 0 or flags != 0:
            raise Refused(BAD_ARG, "n < 0 or flags != 0")
        if n > RAYS_MAX:
            raise Refused(UNSUPPORTED, "more than SWR_RAYS_MAX rays")
        for k, r in enumerate(rays[:n]):
            if RM.check_ray(r) is not None:
                raise Refused(BAD_ARG, f"ray {k}: {RM.check_ray(r)}")
        v, _, sid = self.shape()
        key = (self.scene, digest(v[:, 0:3]), digest(rays[:n].view(np.uint32)))
        if key not in self.casts:
            self.casts[key] = RM.cast(RM.triangles(v, self.i), rays[:n])
        return self.casts[key]

    def delta(self, bit, dst, bands):
        """(delta_model.Delta, dst after the call) of a delta read of the image kind `bit`; the baseline becomes the image."""
        img = self.image[0] if bit == DELTA_COLOR else self.image[1]
        assert img is not None and not isinstance(img, np.ma.MaskedArray), "no colour delta read over an unspecified colour"
        d, out = DM.delta(self.baseline[bit], img, bands, dst)
        self.baseline[bit] = np.array(DM.as_words(img), copy=True)
        return d, out

    def resolved(self, S, filt):
        return FM.resolved(self.read(), S, filt)


def fullest_tile(oracle, v, i, matrices, w, h):
    """The most (triangle, tile) pairs any 64 x 32 tile gets, counted by bounding boxes, for triangles [(index triples, matrix)]:
    test_frame_sequences.tile_load for vertices that are given (an upper bound of what binning puts there)."""
    load = np.zeros(((h + TILE_H - 1) // TILE_H + 1, (w + TILE_W - 1) // TILE_W + 1), dtype=np.int64)
    ty, tx = load.shape[0] - 1, load.shape[1] - 1
    for t, m in matrices:
        sx, sy, _ = oracle.project(v, m, w, h)
        x, y = sx[t].astype(np.float64), sy[t].astype(np.float64)
        ok = np.isfinite(x).all(axis=1) & np.isfinite(y).all(axis=1)
        x, y = x[ok], y[ok]
        x0 = np.clip(np.floor(x.min(axis=1) / TILE_W), 0, tx).astype(int)
        x1 = np.clip(np.floor(x.max(axis=1) / TILE_W) + 1, 0, tx).astype(int)
        y0 = np.clip(np.floor(y.min(axis=1) / TILE_H), 0, ty).astype(int)
        y1 = np.clip(np.floor(y.max(axis=1) / TILE_H) + 1, 0, ty).astype(int)
        for a, b, c, d in zip(x0, x1, y0, y1):
            load[c:d, a:b] += 1
    return int(load.max())
