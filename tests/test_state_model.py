"""On the CPU: what the sequences of tests/test_state_sequences.py cover, that they are not vacuous, and that its player has teeth
(DESIGN.md §17).  The generator is pure Python; the model runs on the C oracle; the player is run against `StandInContext`, an
implementation of the binding's Context on top of tests/state_model.py with a table of switchable defects of the kind the sequences
are about.  Nothing here needs a GPU."""
import hashlib
import re
import time
import types

import numpy as np
import pytest

import delta_model as DM
import frame_model as FM
import state_model as ST
import test_depth_query as TD
import test_frame_sequences as FS
import test_state_sequences as SS
from frame_model import CLIP, IDS, LOAD, NC

S_OPS, O_OPS = SS.S_OPS, SS.O_OPS


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


class StandInContext:
    """The methods of binding.Context that test_state_sequences.play calls, answered by tests/state_model.py; `defect`: one of DEFECTS."""
    oracle = None
    defect = None

    def __init__(self, device=0, device_count=0, **kw):
        self.S = ST.State(self.oracle, SS._CACHE, SS._SHAPES)
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

    def debug_set(self, key, value):
        if key == SS.K.DEBUG_STREAM_ORDER:
            self.order = value

    # -- state ----------------------------------------------------------------------------------------------------------------------
    def scene_upload(self, v, i):
        self._blocking()
        S = self.S
        keep = (S.skin, S.pose_kind, S.pose, S.pose_id) if self.defect == "pose_survives_upload_same_size" and S.v is not None \
            and S.v.shape[0] == np.asarray(v).reshape(-1, 8).shape[0] else None
        S.upload(v, i)
        if keep:
            S.skin, S.pose_kind, S.pose, S.pose_id = keep
        self.cuts = set()

    def scene_attributes(self, attrs):
        self._blocking()
        self._run(self.S.attributes, attrs)
        if self.defect == "normal_deltas_ignored_by_late_attrs" and self.S.targets is not None:
            dp = self.S.targets[0]
            self.S.targets = (dp, None, ST.digest(dp, None))

    def texture_upload(self, texture):
        self._blocking()

    def material_set(self, material):
        self.S.set_material(material)

    def scene_skin(self, joints, weights=None):
        self._overflow_defect(lambda: self._run(self.S.set_skin, joints, weights))

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

    def scene_morph(self, dp, dn=None):
        self._overflow_defect(lambda: self._run(self.S.set_targets, dp, dn))

    def morph_set(self, w):
        self._overflow_defect(lambda: self._run(self.S.set_weights, w))

    def _overflow_defect(self, change):
        """A blocking change of shape: an overflowed last frame is repaired in the shape it was posted in — or, the defect, in the new one."""
        redo = None
        if self.defect == "overflow_repair_in_new_shape" and self.unwaited and self.last_call is not None:
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
        c, d, _ = self._run(self.S.render, v, i, transform, w, h, flags, shading, start)
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
    return {seed: SS.sequence(seed) for seed in SS.STATE_SEEDS}


_FRAME_FIELDS = ("n", "scene", "size", "shader", "kind", "flags", "via", "tf", "shape", "scene_id", "write", "overflow", "items")


def canonical(ops):
    def frame(f):
        return tuple(getattr(f, k) for k in _FRAME_FIELDS)
    return repr([(o[0],) + tuple(frame(x) if isinstance(x, SS.Frame) else x for x in o[1:]) for o in ops])


# sha256 of the operation lists of seeds 41, 42, 43 (canonical() below), as the generator made them when these tests were written
DIGESTS = {41: "838ec2cec4393516e7282ea6e7c433e665994e7893c1037342b0865b07f90412",
           42: "f3c3c516e569a2bb5a8e4eeffd5086dccaa34d7047ca67dbdf74e39ec4152335",
           43: "dfdeabd678e2596996737cb011c8b5309bf2f6ab91285e03f22066cfbc466864"}


def test_sequences_are_reproducible_and_pinned(sequences):
    assert set(DIGESTS) == set(SS.STATE_SEEDS)
    for seed, ops in sequences.items():
        assert canonical(ops) == canonical(SS.sequence(seed)), seed
        assert hashlib.sha256(canonical(ops).encode()).hexdigest() == DIGESTS[seed], seed
    assert len({SS.hooks_of(seed) for seed in sequences}) == 3
    assert {dict(SS.hooks_of(seed))[SS.K.DEBUG_STREAM_ORDER] for seed in sequences} == {1, 0, -1}


def test_the_operations_and_the_scenes(sequences):
    W = SS.world()
    assert {n: s.i.size // 3 for n, s in W.items()} == SS.SCENES
    nv = {n: s.v.shape[0] for n, s in W.items()}
    assert nv == {"torus": 768, "small": 900, "big": 3900} and any(x % 64 for x in nv.values()) and not nv["torus"] % 64
    for name, s in W.items():
        for j, w in s.skins.values():
            assert int(j.max()) == SS.JOINTS[name] - 1
        assert s.targets[0][1] is not None and s.targets[0][0].shape[0] != s.targets[1][0].shape[0]
    for j, w in list(W["small"].skins.values()) + list(W["big"].skins.values()):
        assert (w < 0).any() and np.abs(w.sum(axis=1) - 1).max() > 0.01, "not normalised, and a negative weight"
    # the non-finite target of the torus only ever gets weight +-0
    assert not np.isfinite(W["torus"].targets[0][0][SS.MM.NONFINITE]).any()
    assert all(w[SS.MM.NONFINITE] == 0 for w in W["torus"].weights[0].values()) and np.signbit(W["torus"].weights[0][1][SS.MM.NONFINITE])
    for seed, ops in sequences.items():
        names = {o[0] for o in ops}
        assert names >= {"upload", "target", "attrs", "material", "skin", "pose", "targets", "weights", "write", "frame", "render", "render_delta",
                         "present", "wait", "read", "read_ids", "read_resolved", "count", "query", "bounds", "delta", "delta_reset", "feed",
                         "refused"}, seed
        assert {o[1] for o in ops if o[0] == "upload"} == set(SS.SCENES) and {o[1] for o in ops if o[0] == "target"} == {0, 1, 2}, seed
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
        assert len({x for x in shapes if x[2] is not None or x[4] is not None}) <= 12, (seed, len(shapes))
    assert {o[1] for ops in sequences.values() for o in ops if o[0] == "delta_reset"} == {1, 2, 3}
    refusals = {o[1:] for ops in sequences.values() for o in ops if o[0] == "refused"}
    assert refusals >= {("count_no_ids", -1), ("count_item_no_ids", -1), ("read_ids_no_ids", -1), ("count_wrong_n", -1), ("pose_few_joints", -1),
                        ("pose_no_skin", -1), ("weights_wrong_count", -1), ("weights_no_targets", -1), ("bounds_clip", -5),
                        ("render_delta_load", -5)}
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
    so, oo, refused = played_pairs(sequences)
    want = {(s, o) for s in S_OPS for o in O_OPS if SS.legal(s, o)}
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
        tour = part_of(ops, "rebuild tour")
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
        # the pose kind on each side of the skin, and a list or swr_item_bounds in both orders across the seeds
        kinds = [o[1] for o in tour if o[0] == "pose"]
        assert kinds[:2] == ["mat", "dq"]
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


def test_the_scripted_parts(sequences):
    firsts, hows = set(), set()
    for seed, ops in sequences.items():
        assert [o[1] for o in ops if o[0] == "part"] == ["rebuild tour", "pose kinds", "un-waited", "overflow", "lifetimes", "baselines",
                                                          "bounds feed", "pairs", "random"]
        # un-waited: presented frames, a change of shape with no wait in front, a frame, the wait
        u = part_of(ops, "un-waited")
        k = next(j for j, o in enumerate(u) if o[0] in ("weights", "pose") and u[j - 1][0] == "present" and u[j - 2][0] == "frame")
        hows.add(u[k][0] if u[k][0] == "weights" else u[k][1])
        before = [o[1] for o in u[:k] if o[0] == "frame"]
        assert len(before) >= 2 and "wait" not in [o[0] for o in u[k - 2 * len(before):k]]
        assert u[k + 1][0] in ("frame", "material") and SS.normal_shape(before[-1].shape) != SS.normal_shape(
            next(o[1] for o in u[k + 1:] if o[0] == "frame").shape)
        # overflow: each of the five first waiting calls directly behind the one frame, then a plain read
        ov = part_of(ops, "overflow")
        for j, o in enumerate(ov):
            if o[0] == "frame" and o[1].overflow:
                firsts.add(ov[j + 1][0])
                assert ov[j + 1][0] in ("count", "query", "delta", "bounds", "weights") and ov[j + 2][0] == "read", (seed, ov[j + 1:j + 3])
        assert sum(1 for o in ops if o[0] == "frame" and o[1].overflow) == 5
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
    assert firsts == {"count", "query", "delta", "bounds", "weights"} and hows == {"weights", "mat", "dq"}


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
                assert seen[key] > SS.FIRST_BIN_GUESS * 1.05 and SS.SCENES[f.scene] > SS.FIRST_BIN_GUESS, (key, seen[key])
            else:
                assert seen[key] <= min(SS.SCENES[f.scene], SS.FIRST_BIN_GUESS) * 0.9, (key, seen[key])
    assert sum(1 for k in seen if k[0][2] == ("mat", "crowd")) >= 2


# ---- 4. teeth ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tour():
    return SS.sequence(SS.STATE_SEEDS[0], steps=0, pairs=False)      # the scripted parts (stream order 1: the cuts are real)


def test_the_scripted_tour_passes_on_the_stand_in(oracle, tour):
    assert dict(SS.hooks_of(SS.STATE_SEEDS[0]))[SS.K.DEBUG_STREAM_ORDER] == 1
    for bands in (1, 3):
        st = SS.play(stand_in(oracle), oracle, tour, bands)
        assert st["checked"] >= 35 and len(st["deltas"]) >= 20 and st["refused"] >= 15


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


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_the_player_catches(oracle, tour, defect):
    assert set(CAUGHT_IN) == set(DEFECTS) and len(DEFECTS) >= 10
    with pytest.raises(AssertionError) as e:
        SS.play(stand_in(oracle, defect), oracle, tour, 1)
    k = int(re.match(r"op (\d+) ", str(e.value)).group(1))
    part = [o[1] for o in tour[:k] if o[0] == "part"][-1]
    print(f"{defect}: caught at op {k} {tour[k][0]} in '{part}': {str(e.value)[:150]}")
    assert part == CAUGHT_IN[defect], (defect, part, str(e.value)[:300])
