"""On the CPU: what the sequences of tests/test_state_sequences.py cover, that they are not vacuous, and that its player has teeth
(DESIGN.md §17).  The generator is pure Python; the model runs on the C oracle; the player is run against `StandInContext`, an
implementation of the binding's Context on top of tests/state_model.py with a table of switchable defects of the kind the sequences
are about.  Both families of seeds are covered: 41-43 (dense targets) as they were, and 44-46 (sparse targets of partial unions,
swr_morph_pose_set, two attribute arrays) with their world, their enlarged pair table, their three scripted parts and ten defects of
their own.  Nothing here needs a GPU."""
import dataclasses
import hashlib
import re
import time
import types

import numpy as np
import pytest

import delta_model as DM
import frame_model as FM
import morph_model as MM
import morph_sparse_model as MS
import normals_model as NM
import rays_model as RY
import skin_dq_model as DQ
import state_model as ST
import test_depth_query as TD
import test_frame_sequences as FS
import test_state_sequences as SS
from frame_model import CLIP, IDS, LOAD, NC

S_OPS, O_OPS = SS.S_OPS, SS.O_OPS
ALL_SEEDS = SS.STATE_SEEDS + SS.SPARSE_SEEDS + SS.NORMALS_SEEDS
FAMILIES = {"dense": SS.STATE_SEEDS, "sparse": SS.SPARSE_SEEDS, "normals": SS.NORMALS_SEEDS}


# ---- a context on the CPU -------------------------------------------------------------------------------------------------------------
class SwrError(Exception):
    def __init__(self, code, message=""):
        super().__init__(f"swr error {code}: {message}")
        self.code = code


class HostImage:
    """binding.HostImage without page-locked memory."""

    def __init__(self, shape, dtype):
        self.array = np.zeros(shape, dtype=dtype)

    def free(self):
        self.array = None


DEFECTS = {
    "pose_lost_after_cut": "the pose is not re-applied after a draw list or swr_item_bounds cut a Morton-sorted stream",
    "weights_lost_on_pose_set": "swr_pose_set drops the morph weights",
    "dq_kept_after_matrix_pose": "a matrix pose after a dual-quaternion pose is read as dual quaternions",
    "pose_survives_upload_same_size": "an upload with the same vertex count keeps skin and pose",
    "normal_deltas_ignored_by_late_attrs": "normal deltas given before swr_scene_attributes never take effect",
    "baseline_kept_across_target_change": "the delta baseline of a target size survives a change to another size and back",
    "baseline_updated_by_plain_read": "swr_read_color / swr_read_depth move the delta baseline",
    "delta_writes_row_outside_R": "a delta read writes the first row of R across the whole width",
    "counts_from_frame_before_last": "swr_count_ids reduces the ID image of the frame before the last",
    "query_buffer_not_regrown": "a swr_query_depth with more boxes than any before answers only as many as the largest before",
    "overflow_repair_in_new_shape": "an overflowed last frame is redrawn in the shape a following swr_morph_set / swr_pose_set sets",
    "present_copies_late": "swr_present copies what the framebuffer holds at swr_present_wait",
}
# defects of the state the second family is about: caught on the scripted parts of seed 44
SPARSE_DEFECTS = {
    "prefill_skipped_after_dense": "sparse targets installed over active dense ones: vertices outside the union keep the dense morph",
    "prefill_skipped_between_sparse_sets": "a sparse set installed over an active one: vertices of the old union outside the new keep their morph",
    "uv_stale_after_replaced_attrs": "a second swr_scene_attributes under sparse normal deltas: every vertex keeps the first array's colour/uv quad",
    "normals_morphed_without_normal_deltas": "a set without normal deltas after one with them still reads the morphed normals of the set before",
    "sparse_played_as_dense": "sparse targets are morphed as dense targets with zero rows: a NaN weight reaches vertices its target does not list",
    "null_of_other_entry_keeps_targets": "NULL through the entry of the kind that is not resident removes nothing",
    "weights_survive_new_targets_of_other_kind": "targets of the other kind keep the weights of the targets they replace",
    "combined_call_takes_weights_before_pose_error": "swr_morph_pose_set takes the weights, then refuses the joints",
    "combined_call_ignores_pose_kind": "swr_morph_pose_set blends dual quaternions as the matrices of their rigid motions",
    "combined_call_repairs_overflow_in_new_shape": "an overflowed last frame is redrawn in the shape and pose a following swr_morph_pose_set sets",
}


# defects of the state the third family is about: caught on the scripted parts of seed 47
NORMALS_DEFECTS = {
    "mode_survives_upload": "swr_scene_upload keeps the normals mode of the scene that is gone",
    "mode_survives_render_upload": "the upload swr_render performs keeps the normals mode",
    "mode_dropped_by_new_skin": "swr_scene_skin with a new skin forgets the normals mode",
    "mode_dropped_by_targets_of_other_kind": "targets of the other kind forget the normals mode",
    "early_mode_forgotten_by_attrs": "a mode set before swr_scene_attributes is forgotten when they arrive",
    "other_flip_is_a_noop": "the same mode with the other SWR_NORMALS_FLIP is taken as the no-op repeat",
    "posted_frame_presented_with_new_normals": "a frame posted before swr_scene_normals is presented with the new normals",
    "overflow_repaired_with_new_normals": "an overflowed last frame is redrawn with the normals a following swr_scene_normals sets",
    "rebuild_leaves_uploaded_normals": "a stream rebuild (a draw list or swr_item_bounds cutting a sorted stream) under a mode leaves the uploaded normals",
    "normals_from_unposed_vertices": "the normals are computed from the morphed vertices, before the pose",
    "uploaded_comes_back_without_normal_deltas": "SWR_NORMALS_UPLOADED after a computed mode restores the normals without the morph's normal deltas",
    "rays_from_uploaded_vertices": "swr_cast_rays answers from the vertices as uploaded, not from the shape",
    "rays_from_previous_shape": "swr_cast_rays answers from the shape before the last state change",
    "rays_make_ids_unreadable": "swr_cast_rays makes the IDs of the last frame unreadable",
    "rays_move_a_delta_baseline": "swr_cast_rays moves the delta baselines to the current image",
}


class SpoiltState(ST.State):
    """tests/state_model.py with what a defect leaves behind in the morphed arrays.  `residue`: (name, fn) — fn rewrites the
    (vertices, attributes) between the morph and the pose while a weight is not zero (with every weight zero the stream is built
    from the base arrays, and nothing stale is read).  `as_dense`: sparse targets are morphed as dense ones with zero rows."""
    residue = None
    as_dense = False
    keep_mode = False       # (defect) an upload keeps the normals mode
    mode_off = False        # (defect) the stream holds the uploaded normals until the next rewrite
    unposed = False         # (defect) computed normals come from the vertices before the pose

    def upload(self, v, i):
        kept = self.normals if self.keep_mode else None
        super().upload(v, i)
        self.residue = None
        self.normals = kept

    def mode(self):
        return None if self.mode_off else super().mode()

    def _unposed(self):
        return self.unposed and self.mode() is not None and self.pose is not None

    def shape(self):
        if not self._unposed():
            return super().shape()
        key = self.shape_key() + ("normals of the unposed vertices",)
        if key not in self.shapes:
            v, a, _ = super().shape()
            if self.mode()[0] == ST.SMOOTH:
                a = NM.smooth_attrs(self.attrs, self.morphed()[0], self.i, self.mode()[1])
            self.shapes[key] = (v, a, len(self.shapes))
        return self.shapes[key]

    def drawn(self):
        v, a, i, sid = super().drawn()
        if self._unposed() and self.mode()[0] == ST.FLAT:
            a = np.array(a, copy=True)
            a[:, 0:3] = np.repeat(NM.face_vectors(self.morphed()[0], self.i, self.mode()[1]), 3, axis=0)
        return v, a, i, sid

    def shape_key(self):
        key = super().shape_key()
        if self.weights is None:
            return key
        return key + ((self.residue[0],) if self.residue is not None else ()) + (("as dense",) if self.as_dense and self.kind == ST.SPARSE else ())

    def morphed(self):
        v, a = super().morphed()
        if self.weights is None:
            return v, a
        if self.as_dense and self.kind == ST.SPARSE:
            lists, normals, _ = self.targets
            v = MM.morph_vertices(self.v, MS.dense(lists, self.v.shape[0]), self.weights)
            if self.attrs is not None and normals:
                a = MM.morph_attrs(self.attrs, MS.dense(lists, self.v.shape[0], which=2), self.weights)
        if self.residue is not None:
            v, a = self.residue[1](np.array(v, copy=True), None if a is None else np.array(a, copy=True))
        return v, a


class StandInContext:
    """The methods of binding.Context that test_state_sequences.play calls, answered by tests/state_model.py; `defect`: one of DEFECTS."""
    oracle = None
    defect = None

    def __init__(self, device=0, device_count=0, **kw):
        self.S = SpoiltState(self.oracle, SS._CACHE, SS._SHAPES)
        self.S.as_dense = self.defect == "sparse_played_as_dense"
        self.S.unposed = self.defect == "normals_from_unposed_vertices"
        self.before_v = None                        # the vertices of the shape before the last state change
        self.nbands = max(1, device_count)
        self.order = 1
        self.cuts = set()
        self.pending = []
        self.unwaited = False
        self.last_call = None
        self.prev_ids = None
        self.largest_query = 0
        self.kept = {}                              # (defect) baselines by target size
        self.width = self.height = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    def _run(self, fn, *a, **kw):
        try:
            return fn(*a, **kw)
        except ST.Refused as e:
            raise SwrError(e.code, str(e)) from None

    def _blocking(self):
        self.unwaited = False

    def _check(self, code):
        if code:
            raise SwrError(code)

    def debug_set(self, key, value):
        if key == SS.K.DEBUG_STREAM_ORDER:
            self.order = value

    # -- state ----------------------------------------------------------------------------------------------------------------------
    def scene_upload(self, v, i):
        self._blocking()
        S = self.S
        keep = (S.skin, S.pose_kind, S.pose, S.pose_id) if self.defect == "pose_survives_upload_same_size" and S.v is not None \
            and S.v.shape[0] == np.asarray(v).reshape(-1, 8).shape[0] else None
        S.keep_mode, S.mode_off, self.before_v = self.defect == "mode_survives_upload", False, None
        S.upload(v, i)
        S.keep_mode = False
        if keep:
            S.skin, S.pose_kind, S.pose, S.pose_id = keep
        self.cuts = set()

    def scene_attributes(self, attrs):
        self._blocking()
        S = self.S
        old = S.attrs
        self._run(S.attributes, attrs)
        S.mode_off = False
        if self.defect == "early_mode_forgotten_by_attrs" and old is None:
            S.normals = None
        if self.defect == "normal_deltas_ignored_by_late_attrs" and S.kind == ST.DENSE:
            dp = S.targets[0]
            S.targets = (dp, None, ST.digest(dp, None))
        elif self.defect == "normal_deltas_ignored_by_late_attrs" and S.kind == ST.SPARSE:
            S.targets = ([t[:2] for t in S.targets[0]], False, S.targets[2] + " without normals")
        if self.defect == "uv_stale_after_replaced_attrs" and old is not None and S.kind == ST.SPARSE and S.targets[1]:
            def stale(v, a):
                a[:, 4:8] = old[:, 4:8]
                return v, a
            S.residue = ("stale uv " + ST.digest(old), stale)

    def texture_upload(self, texture):
        self._blocking()

    def material_set(self, material):
        self.S.set_material(material)

    def scene_skin(self, joints, weights=None):
        self._overflow_defect(lambda: self._run(self.S.set_skin, joints, weights))
        if self.defect == "mode_dropped_by_new_skin" and joints is not None:
            self.S.normals = None

    # -- computed normals and ray casts ---------------------------------------------------------------------------------------------
    def _normals(self, mode, flags, reserved):
        S, d = self.S, self.defect
        was = S.normals

        def change():
            if d == "other_flip_is_a_noop" and was is not None and mode == was[0] and not flags & ~ST.FLIP and not any(reserved):
                return
            self._run(S.set_normals, mode, flags, reserved)
            if d == "uploaded_comes_back_without_normal_deltas" and was is not None and S.normals is None and S.targets is not None:
                if S.kind == ST.DENSE:
                    S.targets = (S.targets[0], None, ST.digest(S.targets[0], None))
                elif S.targets[1]:
                    S.targets = ([t[:2] for t in S.targets[0]], False, S.targets[2] + " without normals")
        posted = self.last_call if d == "posted_frame_presented_with_new_normals" and self.unwaited and self.pending else None
        self._overflow_defect(change, "overflow_repaired_with_new_normals")
        if posted is not None:                      # the last posted frame again, under the new normals, into what was presented
            flags_, transform, items, kind, (image, cleared) = posted
            held = (S.image, S.cleared)
            S.image, S.cleared = image, cleared
            again = S.frame(flags_, transform, items, kind)
            S.image, S.cleared = held
            self.pending[-1] = (again,) + self.pending[-1][1:]

    def scene_normals(self, mode, flip=False):
        self._normals(None if mode is None else SS.NORMALS[mode] if isinstance(mode, str) else int(mode), ST.FLIP if flip else 0, (0, 0))

    def raw_scene_normals(self, mode, flags, reserved):
        try:
            self._normals(mode, flags, reserved)
        except SwrError as e:
            return e.code
        return 0

    def cast_rays(self, rays, n=None, flags=0):
        S, d = self.S, self.defect
        v = None
        if d == "rays_from_uploaded_vertices":
            v = S.v
        elif d == "rays_from_previous_shape" and self.before_v is not None and S.v is not None and self.before_v.shape == S.v.shape:
            v = self.before_v
        if v is None:
            hits = self._run(S.cast, rays, n, flags)
        else:
            self._run(S.cast, rays, n, flags)       # (its refusals)
            hits = RY.cast(RY.triangles(v, S.i), rays)
        self._blocking()
        if d == "rays_make_ids_unreadable":
            S.ids_ok = False
        if d == "rays_move_a_delta_baseline" and S.image is not None:
            for bit, img in ((ST.DELTA_COLOR, S.image[0]), (ST.DELTA_DEPTH, S.image[1])):
                if img is not None and not isinstance(img, np.ma.MaskedArray):
                    S.baseline[bit] = np.array(DM.as_words(img), copy=True)
        return hits

    def raw_cast_rays(self, rays, n, flags):
        try:
            self.cast_rays(rays, n, flags)
        except SwrError as e:
            return e.code
        return 0

    def _pose(self, kind, table):
        S = self.S
        weights = (S.weights, S.weights_id)
        if self.defect == "dq_kept_after_matrix_pose" and kind == "mat" and table is not None and S.pose_kind == "dq":
            kind, table = "dq", np.ascontiguousarray(np.asarray(table, dtype=np.float32).reshape(-1, 16)[:, :8])
        self._run(S.set_pose, kind, table)
        if self.defect == "weights_lost_on_pose_set":
            S.weights = S.weights_id = None
        else:
            S.weights, S.weights_id = weights

    def pose_set(self, joints):
        self._overflow_defect(lambda: self._pose("mat", joints))

    def pose_set_dq(self, dq):
        self._overflow_defect(lambda: self._pose("dq", dq))

    def _install(self, entry, fn):
        """New targets — or none — through swr_scene_morph (entry "dense") or swr_scene_morph_sparse ("sparse")."""
        S, d = self.S, self.defect
        was, weights = S.kind, S.weights
        if d == "null_of_other_entry_keeps_targets" and was is not None and was != entry and S.targets is not None and fn is None:
            return
        old_v, old_a = S.morphed() if weights is not None else (None, None)
        had_normals = was == ST.SPARSE and S.targets[1]
        self._run(*(fn or ((S.set_targets, None) if entry == ST.DENSE else (S.set_targets_sparse, None))))
        S.residue = None
        if S.kind == ST.SPARSE and old_v is not None:
            outside = np.ones(S.v.shape[0], dtype=bool)
            outside[SS.union_of(S.targets[0])] = False
            if (d, was) in (("prefill_skipped_after_dense", ST.DENSE), ("prefill_skipped_between_sparse_sets", ST.SPARSE)):
                def stale(v, a):
                    v[outside] = old_v[outside]
                    return v, a
                S.residue = ("no pre-fill " + ST.digest(old_v), stale)
            if d == "normals_morphed_without_normal_deltas" and had_normals and not S.targets[1] and old_a is not None:
                def stale_normals(v, a):
                    if a is not None:
                        a[:, 0:3] = old_a[:, 0:3]
                    return v, a
                S.residue = ("stale normals " + ST.digest(old_a), stale_normals)
        if d == "mode_dropped_by_targets_of_other_kind" and was is not None and S.kind not in (None, was):
            S.normals = None
        if d == "weights_survive_new_targets_of_other_kind" and weights is not None and S.kind not in (None, was):
            w = np.zeros(S.target_count(), dtype=np.float32)
            n = min(w.size, weights.size)
            w[:n] = weights[:n]
            S.set_weights(w)

    def scene_morph(self, dp, dn=None):
        self._overflow_defect(lambda: self._install(ST.DENSE, None if dp is None else (self.S.set_targets, dp, dn)))

    def scene_morph_sparse(self, targets, vertex_count=None):
        self._overflow_defect(lambda: self._install(ST.SPARSE, None if targets is None else (self.S.set_targets_sparse, targets, vertex_count)))

    def morph_set(self, w):
        self._overflow_defect(lambda: self._run(self.S.set_weights, w))

    def morph_pose_set(self, weights, joints, dq=False, pose_kind=None):
        S, d = self.S, self.defect

        def change():
            kind, table = ("dq" if dq else "mat") if pose_kind is None else {0: "mat", 1: "dq"}.get(pose_kind, "neither"), joints
            if d == "combined_call_ignores_pose_kind" and kind == "dq" and table is not None:
                kind, table = "mat", DQ.matrices_of(table)
            if d == "combined_call_takes_weights_before_pose_error":
                self._run(S.set_weights, weights)
                self._run(S.set_pose, kind, table)
            else:
                self._run(S.morph_pose, weights, kind, table)
        self._overflow_defect(change, "combined_call_repairs_overflow_in_new_shape")

    def _overflow_defect(self, change, defect="overflow_repair_in_new_shape"):
        """A blocking change of shape: an overflowed last frame is repaired in the shape it was posted in — or, the defect, in the new one."""
        redo = None
        self.S.mode_off = False
        if self.defect == "rays_from_previous_shape":
            self.before_v = self.S.shape()[0] if self.S.v is not None else None
        if self.defect == defect and self.unwaited and self.last_call is not None:
            flags, transform, items, kind, start = self.last_call
            v, _, _ = self.S.shape()
            tris = self.S.i.reshape(-1, 3)
            ms = [(tris, transform)] if items is None else [(tris[f // 3:(f + n) // 3], m) for f, n, m in items]
            if ST.fullest_tile(self.oracle, v, self.S.i, ms, *self.S.size) > SS.FIRST_BIN_GUESS:
                redo = self.last_call
        change()
        self._blocking()
        if redo is not None:
            flags, transform, items, kind, (image, cleared) = redo
            self.S.image, self.S.cleared = image, cleared
            self.S.frame(flags, transform, items, kind)

    def target_set(self, w, h):
        self._blocking()
        S = self.S
        if self.defect == "baseline_kept_across_target_change" and S.size is not None:
            self.kept[S.size] = dict(S.baseline)
        S.target_set(w, h)
        if self.defect == "baseline_kept_across_target_change" and (w, h) in self.kept:
            S.baseline = dict(self.kept[(w, h)])
        self.width, self.height = w, h

    def target_write(self, c, d):
        self._blocking()
        self.S.target_write(c, d)

    def delta_reset(self, bits):
        self._run(self.S.delta_reset, bits)

    def bands(self):
        return [(0, a, b) for a, b in DM.bands_of(self.S.size[1], self.nbands)]

    # -- frames ---------------------------------------------------------------------------------------------------------------------
    def _cut(self, items):
        n = self.S.i.size // 3
        need = set()
        for f, c, _ in items:
            if c:
                need |= {x for x in (f // 3, (f + c) // 3) if 0 < x < n}
        if self.order == 1 and n > 1 and not need <= self.cuts:
            self.cuts |= need
            if self.defect == "rebuild_leaves_uploaded_normals":
                self.S.mode_off = True
            if self.defect == "pose_lost_after_cut":
                self.S.pose_kind = self.S.pose = self.S.pose_id = None

    def _frame(self, flags, transform, items, kind):
        S = self.S
        self.prev_ids = S.image[2] if S.image is not None else None
        self.last_call = (flags, transform, items, kind, (S.image, S.cleared))
        self._run(S.frame, flags, transform, items, kind)
        self.unwaited = True

    def draw(self, transform, flags=0, primitive_type=0):
        self._frame(flags, np.array(transform, dtype=np.float32, copy=True), None, primitive_type)

    def draw_list(self, items, flags=0):
        items = [(int(f), int(n), np.array(m, dtype=np.float32, copy=True)) for f, n, m in items]
        self._cut(items)
        self._frame(flags, None, items, 0)

    def render(self, v, i, transform, w, h, flags=0, shading=None, scene_id=0, color=None, depth=None):
        self._blocking()
        start = (color, depth) if flags & LOAD else None
        self.S.keep_mode, self.S.mode_off, self.before_v = self.defect == "mode_survives_render_upload", False, None
        try:
            c, d, _ = self._run(self.S.render, v, i, transform, w, h, flags, shading, start)
        finally:
            self.S.keep_mode = False
        self.cuts = set()
        self.width, self.height = w, h
        return (None if c is None else self._color(c)), d.copy()

    def render_delta(self, v, i, transform, w, h, color, depth, flags=0, shading=None, scene_id=0):
        if flags & LOAD:
            raise SwrError(ST.UNSUPPORTED, "swr_render_delta: SWR_FLAG_LOAD")
        self._blocking()
        baseline = dict(self.S.baseline) if self.S.size == (w, h) else None
        self._run(self.S.render, v, i, transform, w, h, flags, shading, None)
        if baseline is not None:
            self.S.baseline = baseline
        self.cuts = set()
        self.width, self.height = w, h
        none = types.SimpleNamespace(x0=0, y0=0, x1=0, y1=0, tiles=0, tiles_changed=0, bytes_copied=0, full=0, reserved=0)
        return (none if flags & NC else self.read_color_delta(color)), self.read_depth_delta(depth)

    # -- observers ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _color(c):
        if c is None:
            return None
        out = np.array(np.ma.getdata(c), copy=True)
        if isinstance(c, np.ma.MaskedArray):
            out[np.ma.getmaskarray(c)] = 0xCD           # (unspecified pixels)
        return out

    def present(self, ci, di):
        self.pending.append((self.S.image, ci, di))

    def present_wait(self):
        self._blocking()
        for image, ci, di in self.pending:
            c, d, _ = self.S.image if self.defect == "present_copies_late" else image
            if c is not None:
                ci.array[...] = self._color(c)
            di.array[...] = d
        self.pending = []

    def sync(self):
        self._blocking()

    def _moved_baseline(self, bit):
        if self.defect == "baseline_updated_by_plain_read":
            img = self.S.image[0] if bit == ST.DELTA_COLOR else self.S.image[1]
            if img is not None and not isinstance(img, np.ma.MaskedArray):
                self.S.baseline[bit] = np.array(DM.as_words(img), copy=True)

    def read_color(self, out=None):
        self._blocking()
        self._moved_baseline(ST.DELTA_COLOR)
        c = self.S.image[0]
        return np.full(self.S.image[1].shape + (4,), 0xCD, dtype=np.uint8) if c is None else self._color(c)

    def read_depth(self, out=None):
        self._blocking()
        self._moved_baseline(ST.DELTA_DEPTH)
        return self.S.image[1].copy()

    def read_ids(self, out=None):
        ids = self._run(self.S.read_ids)
        self._blocking()
        got = np.where(ids == FM.LIVE, 0, ids).astype(np.uint32)
        if out is not None:
            out[...] = got
        return got

    def read_color_resolved(self, S):
        self._blocking()
        return self._color(FM.resolved((self.S.image[0], self.S.image[1]), S, 0)[0])

    def read_depth_resolved(self, S, depth_filter=0):
        self._blocking()
        return FM.resolved((None, self.S.image[1]), S, depth_filter)[1]

    def count_ids(self, group=0, rect=None, n=None):
        S = self.S
        rect = rect if rect is not None else (0, 0) + S.size
        image = S.image
        if self.defect == "counts_from_frame_before_last" and self.prev_ids is not None and S.ids_ok and self.prev_ids.shape == image[2].shape:
            S.image = (image[0], image[1], self.prev_ids)
        try:
            counts, none = self._run(S.count, group, rect, n, SS_binding().list_ids_to_items)
        finally:
            S.image = image
        self._blocking()
        return counts, none

    def query_depth(self, boxes):
        self._blocking()
        got = TD.expected(self.S.depth(), boxes)
        if self.defect == "query_buffer_not_regrown" and self.largest_query and boxes.size > self.largest_query:
            got[self.largest_query:] = 0
        self.largest_query = max(self.largest_query, boxes.size)
        return got

    def item_bounds(self, items, flags=0):
        items = [(int(f), int(n), np.array(m, dtype=np.float32, copy=True)) for f, n, m in items]
        if flags & CLIP:
            raise SwrError(ST.UNSUPPORTED, "swr_item_bounds: SWR_FLAG_DEPTH_CLIP")
        self._blocking()
        self._cut(items)
        return self._run(self.S.bounds, items, flags)

    def _delta(self, bit, buf):
        self._blocking()
        arr = buf.array if hasattr(buf, "array") else buf
        d, out = self.S.delta(bit, arr, [b[1:] for b in self.bands()])
        words = arr.view(np.uint32).reshape(out.shape)
        words[...] = out
        if self.defect == "delta_writes_row_outside_R" and not d.full:
            for r in d.band_rects:
                if r is not None:
                    row = words[r[1]].copy()
                    words[r[1], :r[0]] = 0
                    words[r[1], r[2]:] = 0
                    if np.array_equal(row, words[r[1]]):
                        words[r[1], :r[0]] = 1
                        words[r[1], r[2]:] = 1
        w, h = self.S.size
        return types.SimpleNamespace(x0=d.rect[0], y0=d.rect[1], x1=d.rect[2], y1=d.rect[3], tiles=d.tiles, tiles_changed=d.tiles_changed,
                                     bytes_copied=w * h * 4 if d.full else d.rect_bytes, full=d.full, reserved=0)

    def read_color_delta(self, buf):
        return self._delta(ST.DELTA_COLOR, buf)

    def read_depth_delta(self, buf):
        return self._delta(ST.DELTA_DEPTH, buf)


def SS_binding():
    import swr_amd
    return swr_amd.binding


def stand_in(oracle, defect=None):
    """A namespace that looks like the swr_amd package to `play`."""
    B = SS_binding()
    ctx = type("Ctx", (StandInContext,), {"oracle": oracle, "defect": defect})
    material = types.SimpleNamespace(from_shading=staticmethod(lambda sh: sh))
    binding = types.SimpleNamespace(Material=material, list_ids_to_items=B.list_ids_to_items)
    return types.SimpleNamespace(Context=ctx, HostImage=HostImage, SwrError=SwrError, binding=binding)


# ---- 1. the generator -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sequences():
    return {seed: SS.sequence(seed) for seed in ALL_SEEDS}


_FRAME_FIELDS = ("n", "scene", "size", "shader", "kind", "flags", "via", "tf", "shape", "scene_id", "write", "overflow", "items")


def canonical(ops):
    def frame(f):
        # (the mode a frame is drawn under is named where there is one: the lists of seeds 41-46 are as they were)
        return tuple(getattr(f, k) for k in _FRAME_FIELDS) + ((f.normals,) if f.normals is not None else ())
    return repr([(o[0],) + tuple(frame(x) if isinstance(x, SS.Frame) else x for x in o[1:]) for o in ops])


# sha256 of the operation lists of seeds 41, 42, 43 (canonical() below), as the generator made them when these tests were written
DIGESTS = {41: "838ec2cec4393516e7282ea6e7c433e665994e7893c1037342b0865b07f90412",
           42: "f3c3c516e569a2bb5a8e4eeffd5086dccaa34d7047ca67dbdf74e39ec4152335",
           43: "dfdeabd678e2596996737cb011c8b5309bf2f6ab91285e03f22066cfbc466864"}
# ... and of seeds 44, 45, 46, the second family, as it made them when that family was added
DIGESTS.update({44: "a2820265d385933388d2817592c80587ae73bd4438014e5b068969a8ceb554f4", 45: "34527b3e093178e6a66e200adc166aa5926d33e2186ab714cd7527220fac2def", 46: "0c820b15fcd5c65d8eb65f4c90ce71051d136bbc45e5957decb0259e96c7376d"})


# ... and of seeds 47, 48, 49, the third family, as it made them when that family was added
DIGESTS.update({47: "db0379db7ea57fc8504d657742cb5598314cdd1917497c70ebd44c337c0df851", 48: "b33e5b267267bf74e0cbd852df53f62c8f446ce5847380b99b7b8ab3ac09fc79",
                49: "891576e8ada3053444182ffe79bd355cae618e15e58b77a3575e229a8cc05c7e"})


def test_sequences_are_reproducible_and_pinned(sequences):
    assert set(DIGESTS) == set(ALL_SEEDS) and not any(SS.sparse_family(s) for s in SS.STATE_SEEDS) and all(map(SS.sparse_family, SS.SPARSE_SEEDS))
    for seed, ops in sequences.items():
        assert canonical(ops) == canonical(SS.sequence(seed)), seed
        assert hashlib.sha256(canonical(ops).encode()).hexdigest() == DIGESTS[seed], seed
    for seeds in FAMILIES.values():
        assert len({SS.hooks_of(seed) for seed in seeds}) == 3
        assert [dict(SS.hooks_of(seed))[SS.K.DEBUG_STREAM_ORDER] for seed in seeds] == list(SS.STREAM_ORDERS) == [1, 0, -1]
    # neither the first nor the second family knows anything of the third: no swr_scene_normals, no swr_cast_rays, no hub
    for seed in SS.STATE_SEEDS + SS.SPARSE_SEEDS:
        assert not any(o[0] in ("normals", "rays") or o[:2] == ("upload", "hub") for o in sequences[seed]), seed
        assert all(o[1].normals is None for o in sequences[seed] if o[0] in ("frame", "render", "render_delta")), seed
    for seed in SS.NORMALS_SEEDS:
        assert SS.sparse_family(seed) and SS.normals_family(seed) and not SS.normals_family(seed - 3) and not SS.normals_family(200)
    # the first family knows nothing of the second: no sparse set, no combined call, one attribute array
    for seed in SS.STATE_SEEDS:
        assert not any(o[0] == "morph_pose" or o[:2] == ("attrs", "other") or (o[0] == "targets" and (isinstance(o[1], str) or len(o) > 2))
                       for o in sequences[seed]), seed


def test_the_operations_and_the_scenes(sequences):
    W = SS.world()
    assert {n: s.i.size // 3 for n, s in W.items()} == SS.SCENES3 and {n: x for n, x in SS.SCENES3.items() if n != "hub"} == SS.SCENES
    nv = {n: s.v.shape[0] for n, s in W.items()}
    assert nv == {"torus": 768, "small": 900, "big": 3900, "hub": 312} == SS.VERTICES and any(x % 64 for x in nv.values()) and not nv["torus"] % 64
    # the hub: shared vertices on a count that is no multiple of 64 (both soups share none), one vertex of 300 triangles, one of none
    hub = W["hub"]
    used = np.bincount(hub.i, minlength=312)
    assert nv["hub"] % 64 == 56 and used[NM.HUB] == 300 and used[NM.UNUSED] == 0 and (used[1:301] == 2).all() and np.isfinite(hub.v).all()
    for name in ("small", "big"):
        assert np.bincount(W[name].i, minlength=nv[name]).max() == 1, "the soups share no vertex"
    for name, s in W.items():
        for j, w in s.skins.values():
            assert int(j.max()) == SS.JOINTS[name] - 1
        assert s.targets[0][1] is not None and s.targets[0][0].shape[0] != s.targets[1][0].shape[0]
    for j, w in list(W["small"].skins.values()) + list(W["big"].skins.values()):
        assert (w < 0).any() and np.abs(w.sum(axis=1) - 1).max() > 0.01, "not normalised, and a negative weight"
    # the non-finite target of the torus only ever gets weight +-0
    assert not np.isfinite(W["torus"].targets[0][0][SS.MM.NONFINITE]).any()
    assert all(w[SS.MM.NONFINITE] == 0 for w in W["torus"].weights[0].values()) and np.signbit(W["torus"].weights[0][1][SS.MM.NONFINITE])
    # the sparse sets and the second attribute array of the second family
    big_ragged = 0
    for name, s in W.items():
        n, s0, s1 = nv[name], s.sparse["s0"], s.sparse["s1"]
        U0, U1 = SS.union_of(s0), SS.union_of(s1)
        for U in (U0, U1):
            assert 1 <= U.size <= n - 1, name
            big_ragged += U.size > 256 and U.size % 64 != 0
        assert set(U0) - set(U1) and set(U1) - set(U0) and set(U0) & set(U1), "the unions differ, neither contains the other"
        assert 0 in U0 and 0 not in U1 and n - 1 in U1 and n - 1 not in U0, "the first and the last vertex: each in one union only"
        assert all(len(t) == 3 for t in s0 if t[0].size) and all(len(t) == 2 for t in s1), "normal deltas in one set only"
        assert s0[SS.S0_EMPTY][0].size == 0 and not np.isfinite(s0[SS.S0_NONFINITE][1]).any() and s0[SS.S0_NONFINITE][0].size > 10
        assert all(w[SS.S0_NONFINITE] == 0 for w in s.weights["s0"].values()) and np.signbit(s.weights["s0"][1][SS.S0_NONFINITE])
        assert np.isnan(s.weights["s0"][1][SS.S0_EMPTY]), "an empty target at NaN: a zero ROW at NaN would poison every vertex"
        counts = [len(s0), len(s1), s.targets[0][0].shape[0], s.targets[1][0].shape[0]]
        assert len(set(counts)) == 4 and counts[:2] == [SS.S0_TARGETS, SS.S1_TARGETS], (name, counts)
        assert all(len(w) == 2 and all(x.shape == (len(s.sparse[k]),) for x in w.values()) for k, w in s.weights.items() if isinstance(k, str))
        for t in s0 + s1:                                   # what swr_scene_morph_sparse asks of a list
            assert t[0].dtype == np.uint32 and (np.diff(t[0].astype(np.int64)) > 0).all() and (t[0].size == 0 or t[0][-1] < n)
        # every finite delta moves something, and the sets are no dense targets in disguise
        assert all(np.abs(t[1]).max() > 0.01 for t in s0 + s1 if t[0].size and np.isfinite(t[1]).all())
        assert all(t[0].size < U.size for ts, U in ((s0, U0), (s1, U1)) for t in ts), "no target lists its set's whole union"
        assert s.attrs2.shape == s.attrs.shape and (s.attrs2[:, 0:3] != s.attrs[:, 0:3]).any(axis=1).all()
        assert (s.attrs2[:, 4:6] != s.attrs[:, 4:6]).any(axis=1).all() and np.array_equal(s.attrs2[:, [3, 6, 7]], s.attrs[:, [3, 6, 7]])
    assert big_ragged >= 1, "two workgroups and a partial last wave"
    xyz = W["torus"].v[:, 0:3]
    minus0 = {int(k) for k in np.argwhere((xyz == 0) & np.signbit(xyz))[:, 0]}
    assert minus0 == {k for k, _ in SS.NEGATIVE_ZERO["torus"]}
    for key in ("s0", "s1"):
        assert minus0 - set(SS.union_of(W["torus"].sparse[key])), f"a vertex outside the union of {key} has a -0 coordinate"
    for seed, ops in sequences.items():
        names = {o[0] for o in ops}
        if SS.sparse_family(seed):
            assert names >= {"morph_pose"} and {o[1] for o in ops if o[0] == "attrs"} == {True, "other"}, seed
            assert {o[1] for o in ops if o[0] == "targets"} >= {0, 1, "s0", "s1", None}, seed
            assert {SS.none_entry(o, 0) for o in ops if o[0] == "targets" and o[1] is None and len(o) > 2} == {"dense", "sparse"}, seed
            assert {o[1:] for o in ops if o[0] == "morph_pose"} >= {(0, "dq", 0), (1, "mat", 0), (0, "mat", 0)}, seed
            assert {(o[1] is None, o[3] is None) for o in ops if o[0] == "morph_pose"} >= {(False, False), (True, False), (False, True)}, seed
        assert names >= {"upload", "target", "attrs", "material", "skin", "pose", "targets", "weights", "write", "frame", "render", "render_delta",
                         "present", "wait", "read", "read_ids", "read_resolved", "count", "query", "bounds", "delta", "delta_reset", "feed",
                         "refused"}, seed
        assert {o[1] for o in ops if o[0] == "upload"} == set(SS.SCENES3 if SS.normals_family(seed) else SS.SCENES) and {o[1] for o in ops if o[0] == "target"} == {0, 1, 2}, seed
        assert {o[1] for o in ops if o[0] == "material"} == {0, 1, 2}, seed
        assert {o[1] for o in ops if o[0] == "pose"} == {"mat", "dq", "bind_mat", "bind_dq"}, seed
        assert {o[1] for o in ops if o[0] == "weights"} >= {0, 1, "zero"} or {o[1] for o in ops if o[0] == "weights"} >= {0, 1, None}, seed
        assert {o[2] for o in ops if o[0] == "delta"} == {"pinned", "pageable"} and len({o[1] for o in ops if o[0] == "delta_reset"}) >= 2, seed
        assert {o[2] for o in ops if o[0] == "count"} == {"all", "pixel", "empty", "straddle"}, seed
        frames = [o[1] for o in ops if o[0] == "frame"]
        assert {f.kind for f in frames} == {"tri", "points", "lines"} and {f.via for f in frames} == {"draw", "list"}, seed
        assert not any(f.flags & FM.BLEND for f in frames)
        bursts = [r for r in SS.runs(ops) if len(r) >= 2]
        assert len(bursts) >= 5 and max(len(r) for r in bursts) <= 7, seed
        # a query with more boxes than any before, behind smaller ones
        sizes = [o[1] for o in ops if o[0] == "query"]
        assert min(sizes) == 1 and 2 in sizes and max(sizes) <= 660 and sum(1 for k in range(1, len(sizes)) if sizes[k] > max(sizes[:k])) >= 2, seed
        # the model's share stays bounded, and so does the number of shapes
        assert len({(f.shape, f.size, f.via, f.tf, f.shader, f.flags & ~(IDS | LOAD)) for f in SS.checked_frames(ops) if f.needs_model()}) <= 12
        shapes = {SS.normal_shape(f.shape) for f in frames}
        # (the third family: the seven deformations of the hub more — 304 triangles each — and the primary scene under dense set 0)
        assert len({x for x in shapes if x[2] is not None or x[4] is not None}) <= (22 if SS.normals_family(seed) else 12), (seed, len(shapes))
    assert {o[1] for ops in sequences.values() for o in ops if o[0] == "delta_reset"} == {1, 2, 3}
    refusals = {o[1:] for ops in sequences.values() for o in ops if o[0] == "refused"}
    assert refusals >= {("count_no_ids", -1), ("count_item_no_ids", -1), ("read_ids_no_ids", -1), ("count_wrong_n", -1), ("pose_few_joints", -1),
                        ("pose_no_skin", -1), ("weights_wrong_count", -1), ("weights_no_targets", -1), ("bounds_clip", -5),
                        ("render_delta_load", -5)}
    for seed in SS.NORMALS_SEEDS:                           # every refusal of the third family in every one of its sequences
        mine = [o[1:] for o in sequences[seed] if o[0] == "refused"]
        assert set(mine) >= {("normals_bad_mode", -1), ("normals_bad_flags", -1), ("normals_reserved", -1), ("rays_too_many", -5), ("rays_flags", -1),
                             ("rays_nan", -1), ("rays_zero_dir", -1), ("rays_tmin_tmax", -1)}, seed
        assert {o[1:] for o in sequences[seed] if o[0] == "normals"} >= {(m, f) for m in ("smooth", "flat") for f in (False, True)} | {
            ("uploaded", False), (None, False)}, seed
        assert {o[1] for o in sequences[seed] if o[0] == "rays"} == set(SS.RAY_SETS), seed
    for seed in SS.SPARSE_SEEDS + SS.NORMALS_SEEDS:         # every refusal of the second family in every one of its sequences
        mine = [o[1:] for o in sequences[seed] if o[0] == "refused"]
        assert set(mine) >= {("morph_pose_wrong_count", -1), ("morph_pose_few_joints", -1), ("morph_pose_bad_kind", -1), ("morph_pose_no_skin", -1),
                             ("morph_pose_no_targets", -1), ("sparse_wrong_vertex_count", -1), ("sparse_descending", -1),
                             ("sparse_some_normals", -1), ("sparse_too_many", -5)}, seed
    rows = [f.row() for ops in sequences.values() for f in SS.checked_frames(ops)]
    for factor, values in FM.FACTORS.items():
        assert {r[factor] for r in rows} == set(values), factor


# ---- 2. the coverage conditions: none is a measurement -------------------------------------------------------------------------------
def test_the_tables_of_pairs():
    assert set(ILLEGAL := SS.ILLEGAL) and all(s in S_OPS and o in O_OPS and len(why) > 40 for (s, o), why in ILLEGAL.items())
    assert all(s in S_OPS and o in O_OPS and len(why) > 40 for (s, o), why in SS.UNSPECIFIED.items())
    assert not set(SS.ILLEGAL) & set(SS.UNSPECIFIED)
    assert len(S_OPS) == 21 and len(O_OPS) == 11
    assert sum(SS.legal(s, o) for s in S_OPS for o in O_OPS) == 21 * 11 - len(SS.ILLEGAL) - len(SS.UNSPECIFIED) == 198
    # the second family: six more state changes, none of which makes IDs unreadable or the image unspecified
    assert SS.S_OPS_SPARSE[:21] == S_OPS and len(SS.S_OPS_SPARSE) == 27 == len(set(SS.S_OPS_SPARSE))
    assert SS.s_ops(41) == S_OPS and SS.s_ops(44) == SS.s_ops(200) == SS.S_OPS_SPARSE
    assert sum(SS.legal(s, o) for s in SS.S_OPS_SPARSE for o in O_OPS) == 198 + 6 * 11
    # the third family: six more state changes and one observer; every new pair is legal, each by a sentence of the header
    N, R = SS.S_OPS_NORMALS, SS.O_OPS_NORMALS
    assert N[:27] == SS.S_OPS_SPARSE and len(N) == 33 == len(set(N)) and R[:11] == O_OPS and R[11:] == ("rays",)
    assert SS.s_ops(47) == SS.s_ops(49) == N and SS.o_ops(47) == R and SS.o_ops(44) == SS.o_ops(41) == SS.o_ops(200) == O_OPS
    new = {(s, o) for s in N for o in R} - {(s, o) for s in SS.S_OPS_SPARSE for o in O_OPS}
    assert set(SS.DECIDED) == new and len(new) == 6 * 11 + 33 and all(len(why) > 40 for why in SS.DECIDED.values())
    assert not new & (set(SS.ILLEGAL) | set(SS.UNSPECIFIED)) and sum(SS.legal(s, o) for s in N for o in R) == 264 + 99


def played_pairs(sequences):
    """(state change, first observer) with nothing between them but waits, material changes and refusals; (observer, observer) alike;
    (state change, refused call) for the refusals right behind a state change."""
    so, oo, refused = set(), set(), set()
    for ops in sequences.values():
        cl = SS.classes(ops)
        for (ka, sa, oa), (kb, sb, ob) in zip(cl, cl[1:]):
            so |= {(s, o) for s in sa for o in ob}
            oo |= {(a, b) for a in oa for b in ob}
        for k, s, _ in cl:
            for op in ops[k + 1:]:
                if op[0] == "refused":
                    refused |= {(x, op[1]) for x in s}
                elif op[0] not in SS.NEUTRAL:
                    break
    return so, oo, refused


def test_every_legal_pair_is_played_and_no_other(sequences):
    """Each family plays every legal pair over its own table across its own three seeds."""
    for family, seeds in FAMILIES.items():
        every_legal_pair({seed: sequences[seed] for seed in seeds}, SS.s_ops(seeds[0]), {"dense": 198, "sparse": 264, "normals": 363}[family],
                         SS.o_ops(seeds[0]))


def every_legal_pair(sequences, s_ops, n, O_OPS):
    so, oo, refused = played_pairs(sequences)
    want = {(s, o) for s in s_ops for o in O_OPS if SS.legal(s, o)}
    assert len(want) == n
    assert not want - so, sorted(want - so)
    assert not so & set(SS.ILLEGAL), sorted(so & set(SS.ILLEGAL))
    assert not so & set(SS.UNSPECIFIED), sorted(so & set(SS.UNSPECIFIED))
    assert oo >= {(a, b) for a in O_OPS for b in O_OPS}, sorted({(a, b) for a in O_OPS for b in O_OPS} - oo)
    call = {"count_prim": "count_no_ids", "count_item": "count_item_no_ids", "read_ids": "read_ids_no_ids"}
    missing = {(s, o) for (s, o) in SS.ILLEGAL if (s, call[o]) not in refused}
    assert not missing, sorted(missing)
    # what the header leaves open is played too, unchecked, right behind its state change
    open_pairs = set()
    for ops in sequences.values():
        cl = SS.classes(ops)
        for (ka, sa, oa), (kb, sb, ob) in zip(cl, cl[1:]):
            if "unchecked" in ob:
                open_pairs |= {(s, ops[kb][1]) for s in sa}
    assert open_pairs >= set(SS.UNSPECIFIED), sorted(set(SS.UNSPECIFIED) - open_pairs)


def part_of(ops, name):
    a = ops.index(("part", name))
    b = next(k for k in range(a + 1, len(ops) + 1) if k == len(ops) or ops[k][0] == "part")
    return ops[a + 1:b]


def test_the_six_rebuild_callers_and_the_bind_entries(sequences):
    for seed, ops in sequences.items():
        rebuild_callers(seed, part_of(ops, "rebuild tour"))
    rebuild_orders_and_binds(sequences)


def test_the_six_rebuild_callers_under_a_mode(sequences):
    """The same six, once under SMOOTH and once under FLAT with FLIP: the mode is set before the attributes, every frame behind a
    caller is a Phong frame drawn under the mode and read back, and swr_item_bounds and a ray cast follow."""
    for seed in SS.NORMALS_SEEDS:
        tour = part_of(sequences[seed], "rebuild tour under a mode")
        ups = [k for k, o in enumerate(tour) if o[0] == "upload"]
        assert len(ups) == 2 and ups[0] == 0
        modes = []
        for half in (tour[:ups[1]], tour[ups[1]:]):
            n = next(k for k, o in enumerate(half) if o[0] == "normals")
            mode = half[n][1:]
            assert n < half.index(("attrs", True)) and not any(o[0] in ("frame", "attrs") for o in half[:n]), "set before the attributes"
            modes.append(mode)
            callers = rebuild_callers(seed, half)
            a = half.index(("attrs", True))
            frames = [o[1] for o in half[a:] if o[0] == "frame"]
            assert len(frames) >= 8 and all(f.shader in (1, 2) and not f.flags & NC and f.normals == mode for f in frames), seed
            assert all(f.normals is None and f.shader == 0 for f in (o[1] for o in half[:a] if o[0] == "frame")), "no effect without attributes"
            for name, k in callers:                 # a frame, its read, then swr_item_bounds and / or a ray cast before the next change
                j = next(j for j in range(k + 1, len(half)) if half[j][0] == "frame")
                behind = [o[0] for o in half[j + 1:j + 4]]
                assert behind[0] == "read" and "rays" in behind, (seed, name, behind)
            assert sum(1 for o in half if o[0] == "bounds") >= 6 and sum(1 for o in half if o[0] == "rays") >= 9, seed
            assert any(o[0] == "frame" and o[1].via == "list" and o[1].normals is not None for o in half), "a draw list under the mode"
        assert modes == [("smooth", False), ("flat", True)], seed
    assert dict(SS.hooks_of(47))[SS.K.DEBUG_STREAM_ORDER] == 1, "the cuts of seed 47 are real: its stream is Morton-sorted"


def rebuild_callers(seed, tour):
    """[(caller, its index)] of the six callers of the stream rebuild in a tour, each with a frame read back behind it."""
    state = dict(pose=None, weights=None, attrs=False)
    callers = []
    first = next(k for k, op in enumerate(tour) if op[0] == "read")      # (the tour sets its pose and weights in front of that)
    for k, op in enumerate(tour):
        nontrivial = state["pose"] is not None and state["weights"] is not None
        if k < first:
            pass
        elif op[0] == "attrs" and state["weights"] is not None:
            callers.append(("attributes", k))
        elif op[0] == "skin" and nontrivial:
            callers.append(("skin", k))
        elif op[0] == "pose" and state["pose"] is None and op[1] in ("mat", "dq") and callers and callers[-1][0] == "skin":
            callers.append(("pose", k))
        elif op[0] == "targets" and state["pose"] is not None:
            callers.append(("targets", k))
        elif op[0] == "weights" and state["pose"] is not None and callers[-1][0] == "targets":
            callers.append(("weights", k))
        elif nontrivial and (op[0] == "bounds" or (op[0] == "frame" and op[1].via == "list")) and "cut" not in dict(callers):
            callers.append(("cut", k))
        if op[0] == "pose":
            state["pose"] = None if op[1].startswith("bind") else op[1]
        elif op[0] == "skin":
            state["pose"] = None
        elif op[0] == "targets":
            state["weights"] = None
        elif op[0] == "weights":
            state["weights"] = op[1]
    assert [c for c, _ in callers if c != "cut"] == ["attributes", "skin", "pose", "targets", "weights"], (seed, callers)
    assert "cut" in dict(callers), (seed, callers)
    for name, k in callers:
        later = [(j, o[1]) for j, o in enumerate(tour) if j > k and o[0] == "frame"]
        assert later and tour[later[0][0] + 1][0] == "read", (seed, name)
        assert any(f.shape[3] is not None and f.shape[5] is not None and tour[j + 1][0] == "read" for j, f in later), (seed, name)
    # the pose kind on each side of the skin
    kinds = [o[1] for o in tour if o[0] == "pose"]
    assert kinds[:2] == ["mat", "dq"]
    return callers


def rebuild_orders_and_binds(sequences):
    """A list or swr_item_bounds cuts the stream first, in both orders across the seeds; every bind entry undoes every pose kind."""
    assert {next(o[0] for o in part_of(ops, "rebuild tour") if o[0] == "bounds" or (o[0] == "frame" and o[1].via == "list"))
            for ops in sequences.values()} == {"bounds", "frame"}
    binds = set()
    for seed, ops in sequences.items():
        kind = None
        for op in ops:
            if op[0] == "pose":
                if op[1].startswith("bind"):
                    binds.add((op[1], kind))
                    kind = None
                else:
                    kind = op[1]
            elif op[0] in ("skin", "upload", "render", "render_delta"):
                kind = None
        assert binds >= {("bind_mat", "mat"), ("bind_mat", "dq"), ("bind_dq", "mat"), ("bind_dq", "dq")}, seed


NEW_PARTS = ["morph kinds", "refusals", "late and replaced attributes"]
NORMALS_PARTS = ["normals tour", "rebuild tour under a mode", "un-waited normals", "overflow normals", "mode lifetimes", "rays change nothing",
                 "normals and rays refusals"]


def test_the_scripted_parts(sequences):
    for family, seeds in FAMILIES.items():
        the_scripted_parts({seed: sequences[seed] for seed in seeds}, family != "dense", family == "normals")


def the_scripted_parts(sequences, sparse, third=False):
    firsts, hows = set(), set()
    for seed, ops in sequences.items():
        assert [o[1] for o in ops if o[0] == "part"] == ["rebuild tour", "pose kinds", "un-waited", "overflow", "lifetimes", "baselines",
                                                          "bounds feed"] + (NEW_PARTS if sparse else []) + (NORMALS_PARTS if third else []) + ["pairs", "random"]
        # un-waited: presented frames, a change of shape with no wait in front, a frame, the wait
        u = part_of(ops, "un-waited")
        k = next(j for j, o in enumerate(u) if o[0] in ("weights", "pose", "morph_pose") and u[j - 1][0] == "present" and u[j - 2][0] == "frame")
        assert (u[k][0] == "morph_pose") == sparse, seed
        hows.add(u[k][0] if u[k][0] == "weights" else u[k][1:] if sparse else u[k][1])
        before = [o[1] for o in u[:k] if o[0] == "frame"]
        assert len(before) >= 2 and "wait" not in [o[0] for o in u[k - 2 * len(before):k]]
        assert u[k + 1][0] in ("frame", "material") and SS.normal_shape(before[-1].shape) != SS.normal_shape(
            next(o[1] for o in u[k + 1:] if o[0] == "frame").shape)
        # overflow: each of the five first waiting calls directly behind the one frame, then a plain read
        ov = part_of(ops, "overflow")
        for j, o in enumerate(ov):
            if o[0] == "frame" and o[1].overflow:
                firsts.add(ov[j + 1][0])
                assert ov[j + 1][0] in ("count", "query", "delta", "bounds", "morph_pose" if sparse else "weights") and ov[j + 2][0] == "read", \
                    (seed, ov[j + 1:j + 3])
                if ov[j + 1][0] == "morph_pose":            # weights AND pose change behind the overflowed frame
                    f = ov[j][1]
                    assert ov[j + 1][1] != f.shape[5] and ov[j + 1][1:] == (1, "mat", 0) and f.shape[3] == ("mat", "crowd"), seed
        assert sum(1 for o in ops if o[0] == "frame" and o[1].overflow) == 5 + (3 if third else 0)
        # lifetimes
        lt = part_of(ops, "lifetimes")
        renders = [o[1] for o in lt if o[0] == "render"]
        assert len(renders) == 2 and renders[0].scene_id == renders[1].scene_id != 0 and renders[0].scene == renders[1].scene
        ups = [o[1] for o in lt if o[0] == "upload"]
        assert ups[-2] == renders[0].scene and ups[-1] != ups[-2]
        # baselines: every call that must keep a baseline lies between two delta reads
        bl = [o[0] for o in part_of(ops, "baselines")]
        a = bl.index("delta")
        b = bl.index("delta", a + 1)
        assert set(bl[a + 1:b]) >= {"frame", "query", "bounds", "count", "present", "wait", "read", "read_resolved"}
        w = bl.index("write")
        assert w > b and bl[w + 1] == "delta" and "delta_reset" in bl and bl.count("render_delta") == 3 and bl.count("target") >= 4
        if sparse:
            the_new_parts(seed, ops)
        if third:
            the_normals_parts(seed, ops)
    if sparse:      # the combined call as the blocking change: both halves, NULL joints, NULL weights
        assert firsts == {"count", "query", "delta", "bounds", "morph_pose"} and hows == {(0, "dq", 0), (0, "mat", None), (None, "mat", 0)}
    else:
        assert firsts == {"count", "query", "delta", "bounds", "weights"} and hows == {"weights", "mat", "dq"}


def the_new_parts(seed, ops):
    """'morph kinds', 'refusals' and 'late and replaced attributes' of the second family, step by step."""
    def steps(part, attrs=False):
        """[(the state changes since the last frame, the frame, read back?, the observers behind it)]; attrs: attribute uploads count
        (elsewhere a material brings them along when it needs them)"""
        out, changes = [], []
        for op in part:
            if op[0] == "frame":
                out.append([changes, op[1], False, []])
                changes = []
            elif op[0] == "read" and out and not changes:
                out[-1][2] = True
            elif op[0] in ("count", "query", "bounds", "delta") and out and not changes:
                out[-1][3].append(op[0])
            elif op[0] in ("targets", "weights", "morph_pose", "skin", "pose", "upload", "refused") or (attrs and op[0] == "attrs"):
                changes.append(op)
        return out

    assert SS.PRIMARY[(seed - 41) % 3] in ("torus", "big") and SS.SCENES[SS.PRIMARY[(seed - 41) % 3]] > SS.FIRST_BIN_GUESS, "it can crowd a tile"
    mk = steps(part_of(ops, "morph kinds"))
    assert all(read and f.scene == SS.PRIMARY[(seed - 41) % 3] and f.shape[3] in (("mat", 0), ("dq", 0), None) for _, f, read, _ in mk), seed
    none = ("refused", "weights_no_targets", -1)
    assert [c for c, _, _, _ in mk] == [
        [("targets", 0), ("weights", 0)],                                       # 1
        [("targets", "s0")],                                                    # 2
        [("weights", 0)],                                                       # 3
        [("morph_pose", 0, "dq", 0)], [("morph_pose", None, "dq", 0)], [("morph_pose", 0, "mat", None)], [("morph_pose", 0, "mat", 0)],
        [("targets", "s1")], [("weights", 0)],                                  # 4
        [("targets", 1)],                                                       # 5
        [("targets", "s0"), ("weights", 1)],                                    # 6
        [("targets", None, "dense"), none],                                     # 7
        [("targets", 0), ("weights", 0)], [("targets", None, "sparse"), none]], seed
    # the frame behind a new set is the base; the frame under weights is the set's
    assert [(f.shape[4], f.shape[5]) for _, f, _, _ in mk] == [(0, 0), ("s0", None), ("s0", 0), ("s0", 0), ("s0", None), ("s0", 0), ("s0", 0), ("s1", None), ("s1", 0), (1, None),
                                                               ("s0", 1), (None, None), (0, 0), (None, None)], seed
    assert {o for _, _, _, obs in mk for o in obs} == {"count", "query", "bounds", "delta"} and all(f.flags & IDS for _, f, _, _ in mk), seed
    rf = steps(part_of(ops, "refusals"))
    calls = [c[1] for ch, _, _, _ in rf for c in ch if c[0] == "refused"]
    assert calls == ["morph_pose_no_targets", "morph_pose_wrong_count", "morph_pose_few_joints", "morph_pose_bad_kind", "sparse_wrong_vertex_count",
                     "sparse_descending", "sparse_some_normals", "sparse_too_many", "morph_pose_no_skin"], seed
    assert all(read and ch[-1][0] == "refused" for ch, _, read, _ in rf), "a frame, read back, right behind every refusal"
    # late and replaced attributes: twice, the second time under a pose
    la = steps(part_of(ops, "late and replaced attributes"), attrs=True)
    assert len(la) == 8 and all(read and f.shader == 2 and not f.flags & NC for _, f, read, _ in la), seed
    for k, posed in enumerate((False, True)):
        a, b, c, d = la[4 * k:4 * k + 4]
        head = [o[:2] for o in a[0]]
        assert head[0] == ("upload", SS.PRIMARY[(seed - 41) % 3]) and head.index(("targets", "s0")) < head.index(("attrs", True)) < head.index(("weights", 0))
        assert (("pose", "mat") in head) == posed and all((f.shape[3] is not None) == posed for _, f, _, _ in (a, b, c, d)), seed
        assert b[0] == [("attrs", "other")] and b[1].shape[5] == 0 and (a[1].shape[1], b[1].shape[1]) == (True, "other"), seed
        assert c[0][0] == ("targets", "s1") and (c[1].shape[5] == 0) == posed and d[0] == [("targets", "s0"), ("weights", 0)], seed


def steps_of(part):
    """[[the state changes and refusals since the last frame, the frame, read back?, the observers behind it]] of a scripted part."""
    out, changes = [], []
    for op in part:
        if op[0] in ("frame", "render"):
            out.append([changes, op[1], op[0] == "render", []])
            changes = []
        elif op[0] == "read" and out and not changes:
            out[-1][2] = True
        elif op[0] in ("count", "query", "bounds", "delta", "rays", "read_ids", "present", "wait") and out and not changes:
            out[-1][3].append(op[0])
        elif op[0] in ("targets", "weights", "morph_pose", "skin", "pose", "upload", "refused", "attrs", "normals"):
            changes.append(op)
    return out


DEFORMATIONS = [[("pose", "bind_mat", 0)], [("targets", 0), ("weights", 0)], [("targets", "s0"), ("weights", 1)], [("targets", "s1"), ("weights", 0)],
                [("pose", "mat", 0)], [("pose", "dq", 0)], [("targets", "s0"), ("morph_pose", 0, "mat", 0)]]


def the_normals_parts(seed, ops):
    """The seven scripted parts of the third family, step by step."""
    primary = SS.PRIMARY[(seed - 41) % 3]
    lit = lambda f: f.shader in (1, 2) and not f.flags & (NC | LOAD)
    # normals tour: a mode before the attributes; every mode with and without FLIP, UPLOADED and NULL; seven deformations under each
    nt = steps_of(part_of(ops, "normals tour"))
    assert all(read and "rays" in obs and f.scene == "hub" for _, f, read, obs in nt), seed
    head, first = nt[0], nt[1]
    assert [o[:2] for o in head[0]][0] == ("upload", "hub") and head[0][-1] == ("normals", "smooth", False) and not any(o[0] == "attrs" for o in head[0])
    assert head[1].shader == 0 and head[1].normals is None, "a passthrough frame: the mode has no effect without attributes"
    assert first[0] == [("attrs", True)] and first[1].normals == ("smooth", False) and lit(first[1]), "in effect when they arrive"
    want, modes = [], [("smooth", False), ("smooth", True), ("flat", True), ("flat", False), None]
    for k, m in enumerate(modes):
        if k:
            want.append(([("normals",) + m] if m else [("normals", "uploaded", False)], m))
        want += [(d, m) for d in DEFORMATIONS]
    want += [([("normals", "flat", True)], ("flat", True)), ([("normals", None, False)], None), ([("pose", "dq", 0)], None),
             ([("normals", "smooth", True)], ("smooth", True)), ([("normals", "smooth", True)], ("smooth", True))]
    assert [(c, f.normals) for c, f, _, _ in nt[2:]] == want, seed
    assert all(lit(f) for _, f, _, _ in nt[1:]) and {obs.count("rays") for _, _, _, obs in nt} == {1}, seed
    assert {(f.shape[3], f.shape[4], f.shape[5]) for _, f, _, _ in nt} == {(("mat", 0), "s0", 0), (None, "s0", 0), (None, 0, 0), (None, "s0", 1), (None, "s1", 0),
                                                                           (("mat", 0), "s1", 0), (("dq", 0), "s1", 0), (("dq", 0), "s0", 0)}, seed
    # un-waited normals: a burst of lit frames, the blocking call with no wait in front, a lit frame, the wait
    u = [o for o in part_of(ops, "un-waited normals") if o[0] != "material"]      # (a material is no blocking call)
    behind = [j for j, o in enumerate(u) if o[0] in ("normals", "rays") and u[j - 1][0] == "present" and u[j - 2][0] == "frame"]
    assert [u[j][0] for j in behind] == ["normals", "rays"], seed
    for j in behind:
        before = [o[1] for o in u[j - 6:j] if o[0] == "frame"]
        assert len(before) == 3 and [o[0] for o in u[j - 6:j]] == ["frame", "present"] * 3 and all(lit(f) and f.normals[0] == "smooth" for f in before)
        after = [o for o in u[j + 1:j + 6] if o[0] != "material"]
        assert [o[0] for o in after[:4]] == ["frame", "present", "wait", "read"] and lit(after[0][1]), seed
        assert (after[0][1].normals != before[-1].normals) == (u[j][0] == "normals") and (u[j][0] == "rays" or u[j][1] == "flat"), seed
    # overflow normals: another mode, the same mode and flags, a ray cast — each right behind the overflowed frame, then the read
    ov = part_of(ops, "overflow normals")
    firsts = []
    for j, o in enumerate(ov):
        if o[0] == "frame" and o[1].overflow:
            f = o[1]
            assert lit(f) and f.normals[0] == "smooth" and f.shape[3] == ("mat", "crowd") and ov[j + 2] == ("read",), seed
            firsts.append("same" if ov[j + 1] == ("normals",) + f.normals else "other" if ov[j + 1][0] == "normals" else ov[j + 1])
    assert firsts == ["other", "same", ("rays", "one")], (seed, firsts)
    # mode lifetimes
    lt = steps_of(part_of(ops, "mode lifetimes"))
    assert all(read and (f.via == "render" or "rays" in obs) and (f.via == "render" or lit(f)) for _, f, read, obs in lt), seed
    got = [([o for o in c if o[0] in ("upload", "normals", "attrs", "skin", "targets")], f.via, f.normals) for c, f, _, _ in lt]
    assert [g for g in got if g[0] or g[1] == "render"][-13:] == [
        ([("upload", primary), ("attrs", True)], "draw", None),                                 # an upload of the same size discards the mode
        ([("normals", "smooth", False)], "draw", ("smooth", False)),
        ([("normals", "flat", True)], "draw", ("flat", True)),
        ([("upload", "hub"), ("attrs", True)], "draw", None),                                   # ... and one of another size
        ([("upload", primary), ("skin", 0), ("targets", "s0"), ("attrs", True), ("normals", "flat", False)], "draw", ("flat", False)),
        ([], "render", None), ([], "render", None),                                             # swr_render with a new scene identity; cached
        ([("skin", 0), ("targets", "s0"), ("normals", "smooth", True)], "draw", ("smooth", True)),
        ([("attrs", "other")], "draw", ("smooth", True)),                                       # kept across a second attribute array
        ([("skin", None)], "draw", ("smooth", True)),                                           # ... swr_scene_skin(NULL)
        ([("skin", 0)], "draw", ("smooth", True)),                                              # ... a new skin
        ([("targets", 0)], "draw", ("smooth", True)),                                           # ... targets of the other kind
        ([("targets", "s1")], "draw", ("smooth", True))][-13:], (seed, got)
    k = next(j for j, (c, f, _, _) in enumerate(lt) if f.via == "render")
    assert lt[k][1].scene_id == lt[k + 1][1].scene_id != 0 and lt[k + 2][1].via == "draw" and lt[k + 2][1].normals is None and lit(lt[k + 2][1]), \
        "the plain draw behind the cached render is un-moded"
    assert lt[0][1].normals == ("smooth", False) and lt[1][0][0] == ("upload", primary), seed
    # a draw list cuts the sorted stream under a mode with no pose and no weights in effect: the mode alone asks for the normals again
    assert any(f.via == "list" and f.normals == ("flat", True) and f.shape[2:] == (None, None, None, None) for _, f, _, _ in lt), seed
    # ... and so does swr_item_bounds under SMOOTH, with other boundaries, in front of a Phong frame that is read back
    ml = part_of(ops, "mode lifetimes")
    j = next(j for j, o in enumerate(ml) if o[:2] == ("bounds", "thirds"))
    f = next(o[1] for o in ml[j:] if o[0] == "frame")
    assert f.normals == ("smooth", False) and f.shape[2:] == (None, None, None, None) and lit(f) and ml.index(("normals", "flat", True)) > j, seed
    # rays change nothing
    rc = [o[0] for o in part_of(ops, "rays change nothing") if o[0] not in ("material", "skin", "targets", "weights", "upload", "attrs", "target")]
    text = " ".join(rc)
    assert "frame rays count rays read_ids" in text and text.count("delta pose frame rays delta") == 2, (seed, text)
    assert "frame rays frame read" in text and text.endswith("frame present rays wait read"), (seed, text)
    ds = [o[1] for o in part_of(ops, "rays change nothing") if o[0] == "delta"]
    assert ds == [1, 1, 2, 2], "two delta reads of each kind"
    loaded = [o for o in part_of(ops, "rays change nothing") if o[0] == "frame" and o[1].flags & LOAD]
    assert len(loaded) == 1 and lit(dataclasses.replace(loaded[0][1], flags=loaded[0][1].flags & ~LOAD)), seed
    # refusals: a frame, read back, and a ray cast behind each
    rf = steps_of(part_of(ops, "normals and rays refusals"))
    calls = [c[1] for ch, _, _, _ in rf for c in ch if c[0] == "refused"]
    assert calls == ["normals_bad_mode", "normals_bad_flags", "normals_reserved", "rays_too_many", "rays_flags", "rays_nan", "rays_zero_dir",
                     "rays_tmin_tmax"], seed
    assert all(read and "rays" in obs and lit(f) and f.normals == ("flat", True) for _, f, read, obs in rf), seed
    assert all(ch[-1][0] == "refused" for ch, _, _, _ in rf[1:]), seed
    # every mode with and without FLIP, and none, under a Phong frame whose image is compared
    seen = {f.normals for f in SS.checked_frames(ops) if f.kind == "tri" and f.shader in (1, 2) and not f.flags & NC}
    assert seen == {(m, f) for m in ("smooth", "flat") for f in (False, True)} | {None}, seed


# ---- 3. not vacuous: from the model, with the C oracle ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def played(oracle, sequences):
    """Every sequence played once on the stand-in without a defect (which also says that the model accepts them: a LIVE pixel under
    a count, a colour delta read over an unspecified colour or a shape mismatch would raise here), one and three bands in turn."""
    out = {}
    for seed, ops in sequences.items():
        t0 = time.perf_counter()
        out[seed] = SS.play(stand_in(oracle), oracle, ops, 3 if seed % 2 else 1)
        out[seed]["seconds"] = time.perf_counter() - t0
    return out


def test_the_sequences_are_not_vacuous(oracle, sequences, played):
    W = SS.world()
    by_id = {sid: v for v, a, sid in SS._SHAPES.values()}
    depth_of = {}
    for seed, st in played.items():
        assert st["checked"] >= 100 and st["refused"] >= 15, seed
        if SS.sparse_family(seed):
            the_new_parts_are_not_vacuous(oracle, seed, sequences[seed], st, by_id, depth_of)
        if SS.normals_family(seed):
            the_ray_casts_are_not_vacuous(seed, sequences[seed], st, by_id)
        # consecutive shapes differ in at least 1 % of the pixels of a frame (z-tested, 320 x 192, the scene's affine matrix)
        pairs = {(a, b, scene) for (a, scene), (b, scene_b) in zip(st["shapes"], st["shapes"][1:]) if a != b and scene == scene_b}
        assert len(pairs) >= 15, seed
        for a, b, scene in pairs:
            for sid in (a, b):
                if sid not in depth_of:
                    depth_of[sid] = SS.K.oracle_clear(oracle, by_id[sid], W[scene].i, W[scene].tf["aff"], 320, 192, FM.DT | NC)[1]
            if by_id[a].tobytes() == by_id[b].tobytes():
                continue                                    # (the same vertices with other attributes)
            differ = (depth_of[a].view(np.uint32) != depth_of[b].view(np.uint32)).mean()
            assert differ >= 0.01, (seed, a, b, differ)
        # counts: at least three primitives, and at least three items, seen by one count
        for group in (ST.COUNT_PER_PRIMITIVE, ST.COUNT_PER_ITEM):
            assert max(n for g, rect, n in st["counts"] if g == group) >= 3, (seed, group)
        assert {rect for g, rect, n in st["counts"]} == {"all", "pixel", "empty", "straddle"}
        # queries: boxes that pass nowhere, partly and wholly in every call on a drawn image (a cleared image passes wholly or not at all)
        # (the scripted calls of one and of two boxes cannot hold all three kinds)
        assert all(none and partly and wholly for none, partly, wholly, flat, n in st["queries"] if not flat and n >= 3), seed
        assert all(none and wholly for none, partly, wholly, flat, n in st["queries"] if n >= 3), seed
        assert sum(1 for q in st["queries"] if not q[3] and q[4] >= 3) >= 8 and {1, 2} <= {q[4] for q in st["queries"]}, seed
        # delta reads
        assert sum(1 for changed, tiles, full, narrow in st["deltas"] if 0 < changed < tiles) >= 5, seed
        assert any(changed == 0 for changed, *_ in st["deltas"]) and sum(full for _, _, full, _ in st["deltas"]) >= 4, seed
        assert sum(1 for changed, tiles, full, narrow in st["deltas"] if narrow and not full) >= 2, seed
        # bounds: an item partly off the target, an empty one, one behind the eye
        recs = np.concatenate(st["bounds"])
        assert ((recs["drawable"] > 0) & (recs["x1"] == 320)).any() and ((recs["drawable"] == 0) & (recs["skipped"] == 0)).any()
        assert (recs["behind"] > 0).any(), seed
    assert any(q[3] for st in played.values() for q in st["queries"]), "a query on the cleared image right after swr_target_set"


MORPH_KINDS_MIN = 0.01     # of the pixels of a 320 x 192 frame: what consecutive frames of "morph kinds" differ in, at the least


def the_new_parts_are_not_vacuous(oracle, seed, ops, st, by_id, depth_of):
    W = SS.world()
    scene = SS.PRIMARY[(seed - 41) % 3]
    D = W[scene]
    a, b = st["parts"]["morph kinds"], st["parts"]["refusals"]
    sids = [sid for (sid, sc), k in zip(st["shapes"], st["frame_ops"]) if a < k < b]
    assert len(sids) == 14 and all(sc == scene for (sid, sc), k in zip(st["shapes"], st["frame_ops"]) if a < k < b)

    def depth(sid):
        if sid not in depth_of:
            depth_of[sid] = SS.K.oracle_clear(oracle, by_id[sid], D.i, D.tf["aff"], 320, 192, FM.DT | NC)[1]
        return depth_of[sid]

    # every consecutive pair of checked frames of "morph kinds" differs (z-tested, 320 x 192, the scene's affine matrix)
    for x, y in zip(sids, sids[1:]):
        differ = (depth(x).view(np.uint32) != depth(y).view(np.uint32)).mean()
        assert differ >= MORPH_KINDS_MIN, (seed, x, y, differ)
    # every sparse set, without a pose: the frame differs from the base where triangles with a vertex of the union are visible —
    # before or after the morph — and nowhere else, and some of the scene is visible elsewhere
    tris = D.i.reshape(-1, 3)
    base = SS.K.expected_frame(oracle, D.v, D.i, D.tf["aff"], 320, 192, FM.DT | IDS)
    for key in ("s0", "s1"):
        U = SS.union_of(D.sparse[key])
        mine = np.isin(tris, U).any(axis=1)
        for wid, w in D.weights[key].items():
            mv = MS.morph_vertices(D.v, D.sparse[key], w)
            outside = np.setdiff1d(np.arange(D.v.shape[0]), U)
            assert mv[outside].tobytes() == D.v[outside].tobytes() and (mv[U, 0:3] != D.v[U, 0:3]).any(axis=1).all(), (seed, key, wid)
            got = SS.K.expected_frame(oracle, mv, D.i, D.tf["aff"], 320, 192, FM.DT | IDS)
            inside = np.zeros(base.ids.shape, dtype=bool)
            for ids in (base.ids, got.ids):
                hit = ids != FM.NONE
                inside[hit] |= mine[ids[hit]]
            changed = (got.depth.view(np.uint32) != base.depth.view(np.uint32)) | (got.ids != base.ids)
            assert changed[inside].sum() >= MORPH_KINDS_MIN * changed.size, (seed, key, wid, int(changed[inside].sum()))
            assert not changed[~inside].any(), (seed, key, wid, int(changed[~inside].sum()))
            assert (np.isfinite(base.depth) & ~inside).sum() >= MORPH_KINDS_MIN * changed.size, (seed, key, wid)
    # the textured frames of "late and replaced attributes" show the second array: its frame differs from the first array's
    a = st["parts"]["late and replaced attributes"]
    late = [sid for (sid, sc), k in zip(st["shapes"], st["frame_ops"]) if a < k < min(x for x in st["parts"].values() if x > a)]
    attrs = {sid: x for v, x, sid in SS._SHAPES.values()}
    assert len(late) == 8 and all(attrs[sid] is not None for sid in late)
    for k in (0, 4):
        one, two = attrs[late[k]], attrs[late[k + 1]]
        assert by_id[late[k]].tobytes() == by_id[late[k + 1]].tobytes() and (one[:, 4:6] != two[:, 4:6]).any(axis=1).all(), seed
        assert (one[:, 0:3] != two[:, 0:3]).any(axis=1).all(), seed
        # the set without normal deltas leaves the uploaded normals, the one with them moves every normal of its union
        U = SS.union_of(D.sparse["s0"])
        moved = (attrs[late[k + 3]][:, 0:3] != attrs[late[k + 2]][:, 0:3]).any(axis=1)
        assert moved[U].all(), seed


RAY_HITS_MIN, RAY_MISSES_MIN, RAY_CHANGES_MIN = 10, 5, 8      # of 65 rays


def the_ray_casts_are_not_vacuous(seed, ops, st, by_id):
    """Every cast of the 65 rays has at least 10 hits and at least 5 misses; a change of shape between two of them on one scene
    changes at least 8 hit records; the single ray hits in some shape and the casts are spread over every scene of the family."""
    casts = st["rays"]
    assert len(casts) >= 80 and [r[0] for r in casts] == [k for k, o in enumerate(ops) if o[0] == "rays"], seed
    many = [r for r in casts if r[1] == "many"]
    one = [r for r in casts if r[1] == "one"]
    assert len(many) >= 60 and len(one) >= 8 and all(r[4].size == 65 for r in many) and all(r[4].size == 1 for r in one), seed
    for k, name, scene, sid, hits in many:
        n = int((hits["primitive"] != RY.ID_NONE).sum())
        assert RAY_HITS_MIN <= n <= 65 - RAY_MISSES_MIN, (seed, k, scene, n)
        assert len(set(hits["primitive"][hits["primitive"] != RY.ID_NONE].tolist())) >= 8, "the hits are spread over the scene"
    assert any(r[4]["primitive"][0] != RY.ID_NONE for r in one), seed
    assert {r[2] for r in many} >= {SS.PRIMARY[(seed - 41) % 3], "hub"}, seed
    moved = 0
    for a, b in zip(many, many[1:]):
        if a[2] == b[2] and by_id[a[3]][:, 0:3].tobytes() != by_id[b[3]][:, 0:3].tobytes():
            differ = sum(a[4][j].tobytes() != b[4][j].tobytes() for j in range(65))
            assert differ >= RAY_CHANGES_MIN, (seed, a[0], b[0], differ)
            moved += 1
    assert moved >= 20, (seed, moved)
    # ... and the state changes that move no vertex leave every record as it was (the model's own answer, for the record)
    assert all(a[4].tobytes() == b[4].tobytes() for a, b in zip(many, many[1:])
               if a[2] == b[2] and by_id[a[3]][:, 0:3].tobytes() == by_id[b[3]][:, 0:3].tobytes())


# what the modes differ in, of the 61 440 pixels of a 320 x 192 Phong frame (z-tested, the scene's affine matrix) of each scene in the
# shape of base(): the model gives at least 3 122 differing colour pixels per pair (the torus, SMOOTH against FLAT, both with FLIP; the
# hub's least is 12 138, the soup's 30 890).  The floor is half of the least.
MODES_DIFFER_MIN = 1500


@pytest.mark.parametrize("scene", ["hub", "torus", "big"])
def test_the_modes_show(oracle, scene):
    """Frames under SMOOTH, FLAT, each with FLIP, and UPLOADED differ pairwise in colour and in nothing else: depth and IDs are
    identical.  A sequence that confused two of them would not pass by accident."""
    D = SS.world()[scene]
    M = ST.State(oracle)
    M.upload(D.v, D.i)
    M.attributes(D.attrs)
    M.set_material(D.shading[1])
    M.target_set(320, 192)
    M.set_skin(*D.skins[0]); M.set_pose("mat", D.mats[0])
    M.set_targets_sparse(D.sparse["s0"]); M.set_weights(D.weights["s0"][0])
    frames = {}
    for mode, flip in ((ST.UPLOADED, 0), (ST.SMOOTH, 0), (ST.SMOOTH, ST.FLIP), (ST.FLAT, 0), (ST.FLAT, ST.FLIP)):
        M.set_normals(mode, flip)
        c, d, ids = M.frame(FM.DT | IDS, D.tf["aff"])
        frames[(mode, flip)] = (np.array(np.ma.getdata(c), copy=True), d.copy(), ids.copy())
    keys = list(frames)
    # (the soup shares no vertex: its n_i is its triangle's f_p normalised, and the fragment stage normalises either per pixel.  It
    # is the primary scene of seed 48: in that seed's parts on the primary scene SMOOTH taken for FLAT would not show; it shows in its
    # parts on the hub — "normals tour" and the upload of another size in "mode lifetimes" — and in seeds 47 and 49, on the torus)
    alike = {((ST.SMOOTH, f), (ST.FLAT, f)) for f in (0, ST.FLIP)} if scene == "big" else set()
    least = min((int((frames[a][0] != frames[b][0]).any(axis=-1).sum()), a, b) for k, a in enumerate(keys) for b in keys[k + 1:] if (a, b) not in alike)
    print(f"{scene}: the least two modes differ in: {least}")
    assert least[0] >= MODES_DIFFER_MIN, least
    for key in keys[1:]:
        assert frames[key][1].tobytes() == frames[keys[0]][1].tobytes() and np.array_equal(frames[key][2], frames[keys[0]][2]), key
    # a passthrough frame and a depth-only frame are the same under every mode
    M.set_material(None)
    plain = [M.set_normals(mode, flip) or M.frame(FM.DT, D.tf["aff"]) for mode, flip in keys]
    assert all(np.array_equal(np.ma.getdata(p[0]), np.ma.getdata(plain[0][0])) and p[1].tobytes() == plain[0][1].tobytes() for p in plain)


def test_burst_frames_stay_below_the_bin_guess_and_the_overflow_frame_does_not(oracle, sequences):
    """A frame that is not the last of its un-waited run and overflowed its bins would be reported as dropped: every frame but the
    overflow frames stays below the first guess of a tile region in the shape it is drawn in, by the bounding boxes of the deformed
    vertices (tests/test_frame_model.py's bound).  The overflow frames exceed it."""
    seen = {}
    for ops in sequences.values():
        for op in ops:
            if op[0] not in ("frame", "render", "render_delta") or op[1].kind != "tri":
                continue
            f = op[1]
            key = (SS.normal_shape(f.shape), f.size, f.via == "list", f.tf, bool(f.flags & CLIP))
            if key not in seen:
                s = SS.spec_of(f, SS.shape_vertices(*key[0]))
                s.flags &= CLIP
                seen[key] = FS.tile_load(oracle, s)[0]
            if f.overflow:
                assert seen[key] > SS.FIRST_BIN_GUESS * 1.05 and SS.SCENES3[f.scene] > SS.FIRST_BIN_GUESS, (key, seen[key])
            elif f.scene == "hub":
                # 300 of its 304 triangles meet in one tile.  A tile region holds the frame's triangles, if they are fewer than the guess,
                # rounded up to 64 (first_cap_tile): a frame of fewer triangles than the guess cannot overflow it
                drawn = SS.SCENES3["hub"] if f.via != "list" else sum(n // 3 for _, n, _ in SS.items_of(f.scene, f.tf, f.items))
                assert seen[key] <= drawn < SS.FIRST_BIN_GUESS, (key, seen[key])
            else:
                assert seen[key] <= min(SS.SCENES3[f.scene], SS.FIRST_BIN_GUESS) * 0.9, (key, seen[key])
    assert sum(1 for k in seen if k[0][2] == ("mat", "crowd")) >= 2


# ---- 4. teeth ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tour():
    return SS.sequence(SS.STATE_SEEDS[0], steps=0, pairs=False)      # the scripted parts (stream order 1: the cuts are real)


@pytest.fixture(scope="module")
def sparse_tour():
    return SS.sequence(SS.SPARSE_SEEDS[0], steps=0, pairs=False)     # the scripted parts of the second family (stream order 1 too)


@pytest.fixture(scope="module")
def normals_tour():
    return SS.sequence(SS.NORMALS_SEEDS[0], steps=0, pairs=False)    # the scripted parts of the third family (stream order 1 too)


def test_the_scripted_tour_of_the_third_family_passes_on_the_stand_in(oracle, normals_tour):
    assert dict(SS.hooks_of(SS.NORMALS_SEEDS[0]))[SS.K.DEBUG_STREAM_ORDER] == 1
    for bands in (1, 3):
        st = SS.play(stand_in(oracle), oracle, normals_tour, bands)
        assert st["checked"] >= 35 + 14 + 9 + 8 + 100 and len(st["deltas"]) >= 20 + 6 + 4 and st["refused"] >= 15 + 9 + 2 + 8 and len(st["rays"]) >= 90


def test_the_scripted_tour_passes_on_the_stand_in(oracle, tour, sparse_tour):
    assert dict(SS.hooks_of(SS.STATE_SEEDS[0]))[SS.K.DEBUG_STREAM_ORDER] == 1 == dict(SS.hooks_of(SS.SPARSE_SEEDS[0]))[SS.K.DEBUG_STREAM_ORDER]
    for bands in (1, 3):
        st = SS.play(stand_in(oracle), oracle, tour, bands)
        assert st["checked"] >= 35 and len(st["deltas"]) >= 20 and st["refused"] >= 15
        st = SS.play(stand_in(oracle), oracle, sparse_tour, bands)
        assert st["checked"] >= 35 + 14 + 9 + 8 and len(st["deltas"]) >= 20 + 6 and st["refused"] >= 15 + 9 + 2


# which part of the tour must catch which defect (profiles/state_sequences/mutations.txt records the operation)
CAUGHT_IN = {
    "pose_lost_after_cut": "rebuild tour",
    "weights_lost_on_pose_set": "rebuild tour",
    "dq_kept_after_matrix_pose": "pose kinds",
    "pose_survives_upload_same_size": "lifetimes",
    "normal_deltas_ignored_by_late_attrs": "rebuild tour",
    "baseline_kept_across_target_change": "baselines",
    "baseline_updated_by_plain_read": "baselines",
    "delta_writes_row_outside_R": "baselines",
    "counts_from_frame_before_last": "baselines",
    "query_buffer_not_regrown": "baselines",
    "overflow_repair_in_new_shape": "overflow",
    "present_copies_late": "un-waited",
}
# ... and which part of the second family's tour (profiles/sparse_sequences/mutations.txt)
SPARSE_CAUGHT_IN = {
    "prefill_skipped_after_dense": "morph kinds",
    "prefill_skipped_between_sparse_sets": "morph kinds",
    "uv_stale_after_replaced_attrs": "late and replaced attributes",
    "normals_morphed_without_normal_deltas": "late and replaced attributes",
    "sparse_played_as_dense": "morph kinds",
    "null_of_other_entry_keeps_targets": "morph kinds",
    "weights_survive_new_targets_of_other_kind": "morph kinds",
    "combined_call_takes_weights_before_pose_error": "refusals",
    "combined_call_ignores_pose_kind": "morph kinds",
    "combined_call_repairs_overflow_in_new_shape": "overflow",
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_the_player_catches(oracle, tour, defect):
    assert set(CAUGHT_IN) == set(DEFECTS) and len(DEFECTS) >= 10
    with pytest.raises(AssertionError) as e:
        SS.play(stand_in(oracle, defect), oracle, tour, 1)
    k = int(re.match(r"op (\d+) ", str(e.value)).group(1))
    part = [o[1] for o in tour[:k] if o[0] == "part"][-1]
    print(f"{defect}: caught at op {k} {tour[k][0]} in '{part}': {str(e.value)[:150]}")
    assert part == CAUGHT_IN[defect], (defect, part, str(e.value)[:300])


REFUSES = {"rays_make_ids_unreadable"}      # the defects that show as a call the stand-in refuses where the model answers


def caught_at(oracle, ops, defect):
    """(the operation at which `play` fails on the stand-in with the defect, its part, the text): a comparison that fails — or, for
    the defects of REFUSES alone, a call the stand-in refuses.  Any other error of the stand-in is no catch: it propagates."""
    stats = {}
    with pytest.raises(SwrError if defect in REFUSES else AssertionError) as e:
        SS.play(stand_in(oracle, defect), oracle, ops, 1, stats)
    k = stats["op"]
    assert defect in REFUSES or int(re.match(r"op (\d+) ", str(e.value)).group(1)) == k
    return k, [o[1] for o in ops[:k] if o[0] == "part"][-1], str(e.value)


# ... and which part of the third family's tour (profiles/normals_sequences/mutations.txt)
NORMALS_CAUGHT_IN = {
    "mode_survives_upload": "mode lifetimes",
    "mode_survives_render_upload": "mode lifetimes",
    "mode_dropped_by_new_skin": "mode lifetimes",
    "mode_dropped_by_targets_of_other_kind": "mode lifetimes",
    "early_mode_forgotten_by_attrs": "normals tour",
    "other_flip_is_a_noop": "normals tour",
    "posted_frame_presented_with_new_normals": "un-waited normals",
    "overflow_repaired_with_new_normals": "overflow normals",
    "rebuild_leaves_uploaded_normals": "rebuild tour under a mode",
    "normals_from_unposed_vertices": "normals tour",
    "uploaded_comes_back_without_normal_deltas": "normals tour",
    "rays_from_uploaded_vertices": "normals tour",
    "rays_from_previous_shape": "normals tour",
    "rays_make_ids_unreadable": "rays change nothing",
    "rays_move_a_delta_baseline": "rays change nothing",
}


@pytest.mark.parametrize("defect", sorted(NORMALS_DEFECTS))
def test_the_player_catches_in_the_third_family(oracle, normals_tour, defect):
    """As in the second family: the named part catches the defect played alone, and the whole tour of seed 47 catches it no later."""
    assert set(NORMALS_CAUGHT_IN) == set(NORMALS_DEFECTS) and not set(NORMALS_DEFECTS) & (set(DEFECTS) | set(SPARSE_DEFECTS)) and len(NORMALS_DEFECTS) >= 15
    alone = SS.sequence(SS.NORMALS_SEEDS[0], steps=0, pairs=False, only=(NORMALS_CAUGHT_IN[defect],))
    assert [o[1] for o in alone if o[0] == "part"] == [NORMALS_CAUGHT_IN[defect]]
    SS.play(stand_in(oracle), oracle, alone, 1)
    k, part, text = caught_at(oracle, alone, defect)
    print(f"{defect}: '{part}' alone: caught at its op {k} {alone[k][:3]}, {k - alone.index(('part', part))} operations into the part: {text[:150]}")
    names = [o[1] for o in normals_tour if o[0] == "part"]
    k, first, text = caught_at(oracle, normals_tour, defect)
    print(f"{defect}: the whole tour: caught at op {k} {normals_tour[k][:3]} in '{first}': {text[:150]}")
    assert names.index(first) <= names.index(part), (defect, first, part)
    assert first in NORMALS_PARTS, "no part of the earlier families calls swr_scene_normals or swr_cast_rays"


@pytest.mark.parametrize("defect", sorted((set(DEFECTS) - {"overflow_repair_in_new_shape"}) | set(SPARSE_DEFECTS)))
def test_the_third_family_keeps_the_teeth_of_the_first_two(oracle, normals_tour, defect):
    """The parts the third family shares with the first two catch in it what they catch there."""
    names = [o[1] for o in normals_tour if o[0] == "part"]
    k, part, text = caught_at(oracle, normals_tour, defect)
    if defect in DEFECTS:
        assert part == CAUGHT_IN[defect], (defect, text[:300])
    else:
        assert names.index(part) <= names.index(SPARSE_CAUGHT_IN[defect]), (defect, part, text[:300])


@pytest.mark.parametrize("defect", sorted(SPARSE_DEFECTS))
def test_the_player_catches_in_the_second_family(oracle, sparse_tour, defect):
    """The named part catches the defect ON ITS OWN — played alone from the scene's non-trivial shape, so that no earlier part of the
    tour stands in for it — and the whole tour catches it no later."""
    assert set(SPARSE_CAUGHT_IN) == set(SPARSE_DEFECTS) and not set(SPARSE_DEFECTS) & set(DEFECTS) and len(SPARSE_DEFECTS) >= 10
    alone = SS.sequence(SS.SPARSE_SEEDS[0], steps=0, pairs=False, only=(SPARSE_CAUGHT_IN[defect],))
    assert [o[1] for o in alone if o[0] == "part"] == [SPARSE_CAUGHT_IN[defect]]
    SS.play(stand_in(oracle), oracle, alone, 1)
    k, part, text = caught_at(oracle, alone, defect)
    print(f"{defect}: '{part}' alone: caught at its op {k} {alone[k][0]}, {k - alone.index(('part', part))} operations into the part: {text[:150]}")
    names = [o[1] for o in sparse_tour if o[0] == "part"]
    k, first, text = caught_at(oracle, sparse_tour, defect)
    print(f"{defect}: the whole tour: caught at op {k} {sparse_tour[k][0]} in '{first}': {text[:150]}")
    assert names.index(first) <= names.index(part), (defect, first, part)


@pytest.mark.parametrize("defect", sorted(set(DEFECTS) - {"overflow_repair_in_new_shape"}))
def test_the_second_family_keeps_the_teeth_of_the_first(oracle, sparse_tour, defect):
    """The scripted parts the two families share catch in the second what they catch in the first (but for the overflowed frame behind
    swr_morph_set: the second family has swr_morph_pose_set there, and a defect of its own for it)."""
    k, part, text = caught_at(oracle, sparse_tour, defect)
    assert part == CAUGHT_IN[defect], (defect, text[:300])
