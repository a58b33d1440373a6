"""Sequences that mix poses, morph targets of both kinds, computed normals, ray casts, queries and delta reads on ONE context
(include/swr.h).

tests/test_frame_sequences.py plays frames, draw lists, renders, presents, reads, uploads and target changes in orders; it calls none
of swr_count_ids, swr_query_depth, swr_read_*_delta, swr_render_delta, swr_delta_reset, swr_scene_skin, swr_pose_set, swr_pose_set_dq,
swr_scene_morph, swr_scene_morph_sparse, swr_morph_set, swr_morph_pose_set, swr_item_bounds, swr_scene_normals and swr_cast_rays.  Each
of those came with a suite of its own: one scene, one target, a fresh context per case.  This file plays them in orders, between frames of every kind, on one context.

Three families of seeds.  STATE_SEEDS (41, 42, 43) know dense targets, swr_morph_set and swr_pose_set*, and one attribute array; their
operation lists are pinned as they were before the second family existed.  SPARSE_SEEDS (44, 45, 46) play the same parts with the
sparse set "s0" resident instead of dense set 0 and swr_morph_pose_set as the blocking change behind the burst and the overflowed
frame, and three parts more: "morph kinds" (dense and sparse sets replace each other under active weights; both sparse unions are
partial, so what a set does not list must come from the base, whatever the set before left behind), "refusals" (every refusal of
swr_morph_pose_set and swr_scene_morph_sparse, a frame behind each) and "late and replaced attributes" (sparse normal deltas before
swr_scene_attributes, then a second attribute array, textured).  Their pair table has six state changes more (S_OPS_SPARSE).
NORMALS_SEEDS (47, 48, 49) play all of that, swr_scene_normals — a mode that persists on the scene — and swr_cast_rays — a blocking
observer of the resident stream — with a fourth scene (the hub of tests/normals_model.py: shared vertices, 312 of them) and seven parts
more, each from base() under a Phong material: "normals tour" (a mode before swr_scene_attributes, every mode with and without FLIP over
seven deformations, UPLOADED and NULL, the same mode twice), "rebuild tour under a mode" (the six callers of the stream rebuild under
SMOOTH and under FLAT with FLIP), "un-waited normals" and "overflow normals" (swr_scene_normals, its early return and swr_cast_rays as
the blocking call behind a burst and behind an overflowed frame), "mode lifetimes" (uploads and swr_render discard the mode; a second
attribute array, skins and targets of the other kind keep it), "rays change nothing" (a ray cast between an ID frame and its counts,
between delta reads, in front of a load frame and between swr_present and swr_present_wait) and "normals and rays refusals".  Their pair
table has six state changes and one observer more (S_OPS_NORMALS, O_OPS_NORMALS).  Hit records are compared as bytes.

(a) `sequence(seed, steps)` is a pure-Python, seeded generator of legal C-ABI calls.  Scripted parts make the coverage certain — a
    tour of the six callers of the stream rebuild, the pose kinds and both bind entries, a burst posted under one shape and a blocking
    change of shape behind it, an overflowed frame whose first waiting call is each of five calls in turn, the lifetimes (swr_render
    with a scene identity, uploads of the same and of another size), the delta baselines, item bounds feeding the queries and the
    counts — then every legal (state change, first observer) pair and every ordered pair of observers, dealt over the seeds, then
    `steps` random operations.  Calls the header refuses are played as ("refused", call, code).
(b) `play` makes the calls and compares every image, count, query result, bounds record, delta stat and destination image with
    tests/state_model.py, bit for bit.  A SWR_FLAG_LOAD frame starts from the model's own previous image, never from a read-back.
(c) tests/test_state_model.py asserts, without a GPU, what the sequences of the three families cover, that they are not vacuous, and — on
    a stand-in context with switchable defects — that `play` has teeth.

SWR_SEQUENCE_SEEDS=N adds N more sequences (seeds 200..) per scheduler and band count: a soak.  They belong to the second family,
whose operations include the first's; the third family is seeds 47-49 alone."""
import dataclasses
import functools
import os
import random
import time

import numpy as np
import pytest

import frame_model as FM
import kernel_matrix as K
import morph_model as MM
import morph_sparse_model as MS
import normals_model as NM
import rays_model as RY
import resolve_model as RM
import skin_dq_model as DQ
import skin_model as SM
import state_model as ST
import test_depth_query as TD
import test_frame_sequences as FS
import test_perspective as TP
from frame_model import CB, CCW, CF, CLIP, DT, IDS, LOAD, METAL, NC, PERSP, REAL_LINES  # noqa: F401

pytestmark = pytest.mark.gpu

STATE_SEEDS = (41, 42, 43)                          # the first family: dense targets, swr_morph_set and swr_pose_set* (pinned as they were)
SPARSE_SEEDS = (44, 45, 46)                         # the second family: both kinds of targets, swr_morph_pose_set, two attribute arrays
NORMALS_SEEDS = (47, 48, 49)                        # the third family: the second's operations, swr_scene_normals and swr_cast_rays
STEPS = 24
NORMALS_STEPS = STEPS                               # (measured: with the whole tail its slowest case stays under the bound)
SPARSE_STEPS = STEPS                                # (measured: the slowest case of the second family takes as long as the slowest of the first)
SIZES = FS.SIZES                                    # 320 x 192, 256 x 160, 192 x 96: 6, 5 and 3 tile rows
SCENES = {"torus": 1536, "small": 300, "big": 1300}  # triangles; 768, 900 and 3 900 vertices (900 and 3 900 are no multiples of 64)
# the third family has a scene more: the hub of tests/normals_model.py, 304 triangles on 312 vertices (no multiple of 64), one of them
# shared by 300 triangles, one by none — k_vertex_normals is one lane per vertex, the torus has 768 and both soups share no vertex
SCENES3 = dict(SCENES, hub=304)
VERTICES = {"torus": 768, "small": 900, "big": 3900, "hub": 312}
JOINTS = {"torus": 4, "small": 8, "big": 8, "hub": 8}
TARGETS = {"torus": (5, 2), "small": (3, 2), "big": (3, 2), "hub": (3, 2)}     # targets in target set 0 and 1
STREAM_ORDERS = (1, 0, -1)                          # SWR_DEBUG_STREAM_ORDER of seeds 41, 42, 43
PRIMARY = ("torus", "big", "torus")                 # the scene the scripted parts run on (it must be able to crowd a tile: > 1 024)
MODEL_BUDGET = 3200         # triangles a sequence may send through the NumPy perspective model (as in tests/test_frame_sequences.py)
IMAGES = 8                  # page-locked image pairs per target size: a burst presents at most 6 frames
FIRST_BIN_GUESS = 1024      # swr_api.hip first_cap_tile: a tile region holds min(triangles, 1 024) entries at first
BAD_ARG, UNSUPPORTED = ST.BAD_ARG, ST.UNSUPPORTED
COLOR, DEPTH = ST.DELTA_COLOR, ST.DELTA_DEPTH

# the state-changing operations and the observers the coverage conditions of tests/test_state_model.py are stated over
S_OPS = ("upload_same", "upload_other", "attrs", "skin_new", "skin_none", "pose_mat", "pose_dq", "bind", "targets_new", "targets_none",
         "weights", "weights_zero", "target_same", "target_other", "target_write", "delta_reset", "render", "frame_ids", "frame_noids",
         "frame_list", "frame_points")
# the second family adds: sparse targets; targets of one kind over resident targets of the other; NULL through the entry of the kind
# that is not resident; swr_morph_pose_set with both halves, and with a NULL half; an attribute array that replaces another
S_OPS_SPARSE = S_OPS + ("targets_sparse", "targets_swap_kind", "targets_none_other_entry", "morph_pose", "morph_pose_null_halves", "attrs_other")
O_OPS = ("read", "present", "count_prim", "count_item", "query", "bounds", "delta_color", "delta_depth", "resolved", "read_ids",
         "load_frame")
# the third family adds: each computed mode, the same mode with the other SWR_NORMALS_FLIP, UPLOADED, NULL and the no-op repeat of the
# mode and flags in effect; and one observer, swr_cast_rays
S_OPS_NORMALS = S_OPS_SPARSE + ("normals_smooth", "normals_flat", "normals_flip", "normals_uploaded", "normals_null", "normals_same")
O_OPS_NORMALS = O_OPS + ("rays",)
RAY_SETS = ("one", "many")                          # 1 ray, and 65: one lane into a second wave of k_rays_init / k_rays_finish
NEEDS_IDS = ("count_prim", "count_item", "read_ids")

# (state change, observer) pairs the header forbids, each with the sentence that does; the sequences play them as refusals
_NO_IDS = ("swr_read_ids: SWR_ERR_BAD_ARG when the last frame was drawn without the flag, or when swr_target_set / swr_target_write has "
           "been called since (swr_count_ids: the conditions under which swr_read_ids refuses)")
ILLEGAL = {(s, o): _NO_IDS for s in ("target_same", "target_other", "target_write", "frame_noids") for o in NEEDS_IDS}
ILLEGAL.update({(s, o): "swr_read_ids: SWR_ERR_BAD_ARG when ... swr_target_set, swr_target_write or swr_scene_upload has been called since (the IDs "
                "number the primitives of the scene the frame was drawn from: after a new upload, of whatever size, they name nothing)"
                for s in ("upload_same", "upload_other") for o in NEEDS_IDS})
ILLEGAL.update({("frame_points", o): "Triangles only: .vertices and .line frames with the flag fail with SWR_ERR_UNSUPPORTED (so their "
                "frames never have readable IDs)" for o in NEEDS_IDS})
# pairs the header leaves open: they are played as ("unchecked", observer) — the call must succeed and leave every later answer the
# model's; what it delivers is not looked at
_AFTER_TARGET = ("right after swr_target_set the header defines the image only as what a load frame starts from and what swr_query_depth "
                 "sees (the cleared image)")
UNSPECIFIED = {(s, o): _AFTER_TARGET for s in ("target_same", "target_other") for o in ("read", "present", "delta_color", "delta_depth", "resolved")}
UNSPECIFIED.update({("target_write", o): "swr_present copies 'the frame of the LAST swr_draw' and a resolved read 'the last frame's colour "
                    "image': swr_target_write is no frame" for o in ("present", "resolved")})


# the new pairs, decided from the header: none is illegal and none is open.  Each sentence is the one that decides its pairs.
DECIDED = {(s, "rays"): "Ray casts, Errors: SWR_ERR_NO_SCENE: no scene (no other state is named: swr_cast_rays needs neither a target nor a "
           "frame, so it is defined right after swr_target_set, swr_target_write and a frame of any kind)" for s in S_OPS_NORMALS}
DECIDED.update({(s, o): "Computed normals, What the mode is: Primitive IDs, painter's order and tie order are unchanged (and swr_read_ids "
                "names swr_target_set, swr_target_write and swr_scene_upload as what makes IDs unreadable: swr_scene_normals is not among them)"
                for s in S_OPS_NORMALS[len(S_OPS_SPARSE):] for o in NEEDS_IDS})
DECIDED.update({(s, o): "Computed normals, Ordering: a frame posted before the call never sees the new normals (the image, its reads, "
                "queries and delta reads are those of the frame as it was drawn; only the next frame draws the new normals)"
                for s in S_OPS_NORMALS[len(S_OPS_SPARSE):] for o in O_OPS if o not in NEEDS_IDS})


def legal(s, o):
    return (s, o) not in ILLEGAL and (s, o) not in UNSPECIFIED


def sparse_family(seed):
    """Seeds 41-43 are the first family; every other seed (44-46, and the soak seeds 200..) belongs to the second."""
    return seed not in STATE_SEEDS


def normals_family(seed):
    """Seeds 47-49: the third family.  It plays everything the second plays (sparse_family is true of it)."""
    return seed in NORMALS_SEEDS


def s_ops(seed):
    return S_OPS_NORMALS if normals_family(seed) else S_OPS_SPARSE if sparse_family(seed) else S_OPS


def o_ops(seed):
    return O_OPS_NORMALS if normals_family(seed) else O_OPS


def none_entry(op, n):
    """The entry a ("targets", None[, entry]) operation goes through — "dense": swr_scene_morph(NULL), "sparse":
    swr_scene_morph_sparse(NULL); without a named entry the n-th such operation of a sequence alternates, swr_scene_morph first."""
    return op[2] if len(op) > 2 else ("dense", "sparse")[n % 2]


def hooks_of(seed):
    return FS.HOOK_SETS[seed % len(FS.HOOK_SETS)] + ((K.DEBUG_STREAM_ORDER, STREAM_ORDERS[(seed - STATE_SEEDS[0]) % 3]),)


# ---- the generator (no NumPy, no GPU) ------------------------------------------------------------------------------------------------
@dataclasses.dataclass(eq=False)
class Frame:
    n: int                  # order number in the sequence
    scene: str
    size: int               # index into SIZES
    shader: int             # the context's material when the frame is drawn
    kind: str               # "tri" | "points" | "lines"
    flags: int
    via: str                # "draw" | "list" | "render" | "render_delta"
    tf: str                 # "aff" | "per"
    shape: tuple = None     # the generator's name of the shape: (scene, attrs, skin, pose, targets, weights)
    scene_id: int = 0       # (render)
    write: int = None       # (render with SWR_FLAG_LOAD) the seed of its starting image
    overflow: bool = False  # the one frame of a part that crowds a tile beyond the first bin guess
    items: str = "split"    # (list) the draw list, a name of items_of
    part: str = ""
    normals: tuple = None   # (the third family) the computed mode in effect when the frame is drawn: ("smooth" | "flat", flip) or None

    def row(self):
        return FM.row_of(self.flags, self.shader, self.via == "list", self.tf == "per")

    def needs_model(self):
        return self.kind == "tri" and bool(self.flags & PERSP) and not self.flags & NC and self.tf == "per"

    def deformed(self):
        return self.shape[3] is not None or self.shape[5] is not None


BLOCKING = ("wait", "read", "read_resolved", "read_ids", "sync", "upload", "target", "write", "render", "render_delta", "attrs", "skin", "pose",
            "targets", "weights", "morph_pose", "count", "query", "bounds", "delta", "feed", "refused", "normals", "rays")
NEUTRAL = ("hooks", "wait", "sync", "material", "part", "refused")     # (neither a state change nor an observer of the tables)


def sequence(seed, steps=None, pairs=True, only=None):
    """The operations of one sequence:
    ("hooks", pairs) ("part", name) ("upload", scene) ("target", size) ("attrs", True | "other") ("material", shader) ("skin", id | None)
    ("pose", "mat" | "dq" | "bind_mat" | "bind_dq", id) ("targets", id | "s0" | "s1" | None[, entry]) ("weights", id | "zero" | None)
    ("morph_pose", weights id | "zero" | None, "mat" | "dq", pose id | None) ("write", seed)
    ("frame", Frame) ("render", Frame) ("render_delta", Frame, buffer) ("present", image) ("wait",) ("sync",) ("read",) ("read_ids",)
    ("read_resolved", S, depth filter, which) ("count", group, rect name) ("query", boxes, seed) ("bounds", list name, flags)
    ("delta", kind bits, buffer) ("delta_reset", bits) ("feed",) ("refused", call, code); the third family:
    ("normals", "smooth" | "flat" | "uploaded" | None, flip) ("rays", "one" | "many").
    only: the names of the scripted parts to generate (each starts from the scene's non-trivial shape on its own), for the teeth of
    tests/test_state_model.py."""
    rng = random.Random(seed)
    ops = [("hooks", hooks_of(seed))]
    primary = PRIMARY[(seed - STATE_SEEDS[0]) % 3]
    sparse = sparse_family(seed)
    third = normals_family(seed)
    scenes = SCENES3 if third else SCENES
    if steps is None:
        steps = NORMALS_STEPS if third else SPARSE_STEPS if sparse else STEPS
    T0, T1 = ("s0", "s1") if sparse else (0, 1)             # the targets base() keeps resident, and the tour's second set
    st = dict(scene=None, attrs=False, skin=None, pose=None, targets=None, weights=None, size=None, shader=0, last=None, ids=False,
              countable=False, image=False, color=False, pending=0, count=0, budget=MODEL_BUDGET, paid=set(), boxes=0, dbuf=0, part="",
              normals=None)

    def emit(*op):
        ops.append(tuple(op))

    def part(name):
        wait()
        st["part"] = name
        emit("part", name)

    def shape():
        return (st["scene"], st["attrs"], st["skin"], st["pose"], st["targets"], st["weights"])

    # -- state changes ------------------------------------------------------------------------------------------------------------
    def wait():
        if st["pending"]:
            emit("wait")
            st["pending"] = 0

    def upload(scene):
        wait()
        emit("upload", scene)
        st.update(ids=False, countable=False)               # (the IDs numbered the primitives of the scene that is gone)
        st.update(scene=scene, attrs=False, skin=None, pose=None, targets=None, weights=None, normals=None)
        if st["shader"]:
            material(0)

    def target(size):
        wait()
        emit("target", size)
        st.update(size=size, last=None, ids=False, countable=False, image=False, color=False)

    def attrs(which=True):
        wait()
        emit("attrs", which)
        st["attrs"] = which

    def material(shader):
        if shader and not st["attrs"]:
            attrs()
        if shader != st["shader"]:
            emit("material", shader)
            st["shader"] = shader

    def skin(k):
        wait()
        emit("skin", k)
        st.update(skin=k, pose=None)

    def pose(kind, k=0):
        wait()
        assert st["skin"] is not None
        emit("pose", kind, k)
        st["pose"] = None if kind.startswith("bind") else (kind, k)

    def targets(k, entry=None):
        wait()
        emit("targets", k) if entry is None else emit("targets", k, entry)
        st.update(targets=k, weights=None)

    def weights(k):
        wait()
        assert st["targets"] is not None
        emit("weights", k)
        st["weights"] = None if k in ("zero", None) else k

    def morph_pose(w, kind, k):
        wait()
        assert st["targets"] is not None and st["skin"] is not None
        emit("morph_pose", w, kind, k)
        st["weights"] = None if w in ("zero", None) else w
        st["pose"] = None if k is None else (kind, k)

    def normals(mode, flip=False):
        """swr_scene_normals: blocking; "uploaded" and None (NULL) leave no mode."""
        wait()
        emit("normals", mode, bool(flip))
        st["normals"] = (mode, bool(flip)) if mode in ("smooth", "flat") else None

    def write():
        wait()
        emit("write", rng.randrange(1 << 16))
        st.update(last=None, ids=False, countable=False, image=True, color=True)

    def reset(bits):
        emit("delta_reset", bits)

    def base(scene=None, w=0):
        """The scene in its non-trivial shape: skin 0, matrix pose 0, targets 0 (the second family: the sparse set "s0") under weights
        `w` — only what differs is called.  Every part starts from here, which keeps the distinct shapes of a sequence few
        (tests/test_state_model.py counts them)."""
        if scene is not None and scene != st["scene"]:
            upload(scene)
        if st["skin"] != 0:
            skin(0)
        if st["pose"] != ("mat", 0):
            pose("mat", 0)
        if st["targets"] != T0:
            targets(T0)
        if st["weights"] != w:
            weights(w)

    # -- frames ---------------------------------------------------------------------------------------------------------------------
    def frame(kind="tri", force=None, via=None, ids=None, color=None, present_it=False, overflow=False, items="split"):
        """One frame with random factors (force: factor values that are given; ids / color: True forces the flag on / a specified
        colour).  Blend frames are left out: their model is per primitive, and seeds 31-33 of tests/test_frame_sequences.py have them."""
        row = {f: rng.choice(FM.FACTORS[f]) for f in FM.FACTORS}
        if row["clip"] and rng.random() < 0.6:
            row["clip"] = 0                                     # (the restated fans are the model's dearest part after the perspective)
        row.update(force or {})
        if ids is not None:
            row["ids"] = int(ids)
        if color:
            row["no_color"] = 0
        if row["ids"] and "rules" not in (force or {}):
            row["rules"] = rng.choice(("ztest", "metal"))       # (counted frames: the z-tested rule sets determine every ID)
        if overflow:
            row.update(clip=0, list=0, transform="affine", persp=0, cull="none", load=0)
        if row["shader"] and not st["attrs"] and st["pending"]:
            row["shader"] = 0                                   # (no blocking attribute upload inside a burst)
        tf = "per" if row["transform"] == "perspective" else "aff"
        flags = FM.flags_of(row)
        if kind == "tri" and flags & PERSP and not flags & NC and tf == "per":
            cost = scenes[st["scene"]] * (3 if row["clip"] else 1) * (2 if row["list"] else 1)
            key = (shape(), st["size"], row["list"], row["shader"], flags & (DT | METAL | CB | CF | CCW | CLIP))
            if key in st["paid"]:
                pass
            elif cost > st["budget"]:
                flags &= ~PERSP
            else:
                st["budget"] -= cost
                st["paid"].add(key)
        if kind == "tri":
            material(row["shader"])
            how = via or ("list" if row["list"] else "draw")
        else:
            flags = (flags & (CB | CF | CCW | CLIP | PERSP)) | (REAL_LINES if kind == "lines" and rng.random() < 0.7 else 0)
            how = "draw"
        f = Frame(st["count"], st["scene"], st["size"], st["shader"], kind, flags, how, tf, shape(), overflow=overflow, part=st["part"],
                  items=items, normals=st["normals"] if st["attrs"] else None)
        st["count"] += 1
        if how in ("render", "render_delta"):
            # swr_render uploads the scene itself (skin, pose, targets and weights are gone), sets its own target (the same size: a
            # delta baseline is kept) and the pass's own fragment stage
            wait()
            f.scene_id = rng.choice((0, 70 + list(scenes).index(f.scene)))
            f.shape = (st["scene"], bool(f.shader), None, None, None, None)
            f.normals = None                                # (the upload it performs discards the mode)
            if flags & LOAD:
                f.write = rng.randrange(1 << 16)
            if how == "render":
                emit("render", f)
            else:
                emit("render_delta", f, ("pinned", "pageable")[st["dbuf"] % 2])
                st["dbuf"] += 1
            st.update(attrs=bool(f.shader), skin=None, pose=None, targets=None, weights=None, normals=None)
        else:
            emit("frame", f)
        loaded_color = bool(flags & LOAD) and st["color"] if st["image"] else True
        st.update(last=f, ids=bool(flags & IDS) and kind == "tri", countable=bool(flags & IDS) and kind == "tri", image=True,
                  color=(not flags & NC and (loaded_color or not flags & LOAD)) if kind == "tri" else True)
        if present_it:
            present()
        return f

    def present():
        if st["last"] is not None and st["pending"] < IMAGES:
            emit("present", st["pending"])
            st["pending"] += 1

    def burst(length, head=None, force=None):
        wait()
        if head:
            frame(head, present_it=True)
        for k in range(length):
            frame(force=dict(force or {}, clip=0) if st["scene"] == "big" else force, present_it=True)

    # -- observers ------------------------------------------------------------------------------------------------------------------
    def read():
        emit("read")

    def count(group, rect=None):
        emit("count", group, rect or rng.choice(("all", "pixel", "empty", "straddle")))

    def query(n=None):
        given, n = n, n or rng.randint(3, 300)              # (three boxes make a call that passes nowhere, partly and wholly)
        if not given and 0 < st["boxes"] < 600 and rng.random() < 0.35:
            n = st["boxes"] + rng.randint(1, 60)            # more boxes than any call before: the buffers grow
        st["boxes"] = max(st["boxes"], n)
        emit("query", n, rng.randrange(1 << 16))

    def bounds(name=None, flags=None):
        emit("bounds", name or rng.choice(("split", "one", "thirds")), rng.choice((0, METAL, DT | IDS | LOAD)) if flags is None else flags)

    def delta(bits=None):
        bits = bits or rng.choice((COLOR, DEPTH, COLOR | DEPTH))
        if not st["color"]:
            bits &= ~COLOR
        if bits:
            emit("delta", bits, ("pinned", "pageable")[st["dbuf"] % 2])
            st["dbuf"] += 1

    def resolved():
        which = "depth" if not st["color"] else rng.choice(("color", "depth", "both"))
        emit("read_resolved", rng.choice((2, 4)), rng.choice((RM.SAMPLE0, RM.MIN)), which)

    def refused(call, code=BAD_ARG):
        emit("refused", call, code)

    def rays(name=None):
        emit("rays", name or ("many" if rng.random() < 0.8 else "one"))

    def observe(o):
        """The observer `o` of O_OPS, on the state as it is (its legality is the caller's business)."""
        if o == "read":
            read()
        elif o == "present":
            present()
            wait()
        elif o == "count_prim":
            count(ST.COUNT_PER_PRIMITIVE)
        elif o == "count_item":
            count(ST.COUNT_PER_ITEM)
        elif o == "query":
            query()
        elif o == "bounds":
            bounds()
        elif o == "delta_color":
            delta(COLOR)
        elif o == "delta_depth":
            delta(DEPTH)
        elif o == "resolved":
            resolved()
        elif o == "read_ids":
            emit("read_ids")
            st["pending"] = 0
        elif o == "load_frame":
            frame(force=dict(load=1, no_color=0, clip=0, **({} if st["attrs"] else {"shader": 0})), ids=rng.random() < 0.5)
        elif o == "rays":
            rays()
        else:
            raise AssertionError(o)

    def change(s):
        """The state change `s` of S_OPS from the scene's non-trivial shape."""
        if s == "upload_same":
            upload(st["scene"])
        elif s == "upload_other":
            others = [x for x in scenes if x != st["scene"]]
            upload(min(others, key=lambda x: (sum(1 for o in ops if o == ("upload", x)), rng.random())))
        elif s.startswith("normals_"):
            # a mode shows only with attributes; a change "of mode" starts from the other one, the rest from some mode in effect
            if not st["attrs"]:
                attrs()
            cur, flip = st["normals"], rng.random() < 0.5
            if s in ("normals_smooth", "normals_flat"):
                if cur is not None and cur[0] == s[8:]:
                    normals("flat" if s == "normals_smooth" else "smooth", cur[1])
                normals(s[8:], flip)
            else:
                if cur is None:
                    normals(rng.choice(("smooth", "flat")), flip)
                cur = st["normals"]
                if s == "normals_flip":
                    normals(cur[0], not cur[1])
                elif s == "normals_same":
                    normals(*cur)
                else:
                    normals("uploaded" if s == "normals_uploaded" else None)
        elif s == "attrs":
            if st["attrs"]:
                upload(st["scene"])
                base()
                frame(ids=True, color=True, force=dict(load=0, shader=0, list=0))
            attrs()
        elif s == "skin_new":
            skin(0)                                         # (the same influences again: a new skin all the same)
        elif s == "skin_none":
            skin(None)
        elif s == "pose_mat":
            pose("mat", 0)
        elif s == "pose_dq":
            pose("dq", 0)
        elif s == "bind":
            pose(rng.choice(("bind_mat", "bind_dq")))
        elif s == "targets_new":
            targets(0)                                      # (the same deltas again: new targets all the same)
        elif s == "targets_none":
            targets(None)
        elif s == "weights":
            weights(1 if st["weights"] == 0 else 0)
        elif s == "weights_zero":
            weights(rng.choice(("zero", None)))
        elif s == "targets_sparse":
            targets("s0")                                   # (the same lists again: new targets all the same)
        elif s == "targets_swap_kind":
            targets(0)                                      # dense targets over the resident sparse ones
        elif s == "targets_none_other_entry":
            targets(None, "dense" if isinstance(st["targets"], str) else "sparse")
        elif s == "morph_pose":
            if rng.random() < 0.5:
                morph_pose(1 if st["weights"] == 0 else 0, "mat", 0)
            else:
                morph_pose(0, "dq", 0)
        elif s == "morph_pose_null_halves":
            morph_pose(*rng.choice(((None, "mat", 0), (0, "mat", None), ("zero", "dq", None), (None, "dq", None))))
        elif s == "attrs_other":
            if not st["attrs"]:
                attrs()
            attrs("other" if st["attrs"] is True else True)
        elif s == "target_same":
            target(st["size"])
        elif s == "target_other":
            target(rng.choice([x for x in range(len(SIZES)) if x != st["size"]]))
        elif s == "target_write":
            write()
        elif s == "delta_reset":
            reset(rng.choice((COLOR, DEPTH, COLOR | DEPTH)))
        elif s == "render":
            frame(via="render", ids=True, color=True, force=dict(load=0, clip=0))
        elif s == "frame_ids":
            frame(ids=True, color=True, force=dict(list=0))
        elif s == "frame_noids":
            frame(ids=False, color=True)
        elif s == "frame_list":
            frame(ids=True, color=True, force=dict(list=1))
        elif s == "frame_points":
            frame(rng.choice(("points", "lines")))
        else:
            raise AssertionError(s)

    # -- the scripted parts ---------------------------------------------------------------------------------------------------------
    def checked(**kw):
        """A frame that shows something (both cull bits together draw nothing), read back."""
        kw["force"] = dict(kw.get("force") or {}, cull=rng.choice(("none", "back", "front")))
        f = frame(color=True, **kw)
        read()
        return f

    def rebuild_tour():
        """A pose and weights, then each of the six callers of the stream rebuild; a frame is drawn and read after every step, and a
        frame under a pose and weights follows every caller."""
        part("rebuild tour")
        upload(primary)
        target(0)
        skin(0); pose("mat", 0); targets(T0); weights(0)
        checked(ids=True, force=dict(load=0, shader=0, list=0, clip=0))
        attrs()                                             # 1: attributes arriving after the normal deltas
        checked(force=dict(load=0, shader=1, list=0, no_color=0, clip=0))
        skin(0 if sparse else 1)                            # 2: a new skin: the bind pose, the weights kept
        checked(force=dict(load=0, shader=2, list=0, clip=0))
        pose("dq", 0)                                       # 3: a pose of the other kind
        checked(force=dict(load=0, shader=1, list=0, clip=0))
        targets(T1)                                         # 4: new targets under a pose: every weight 0, the pose kept
        checked(force=dict(load=0, list=0, clip=0))
        weights(0)                                          # 5: new weights
        checked(force=dict(load=0, shader=rng.choice((1, 2)), list=0, clip=0))
        if seed % 2:                                        # 6: a draw list or swr_item_bounds cuts a Morton-sorted stream
            checked(ids=True, force=dict(load=0, list=1, clip=0))
            bounds("thirds", 0)
        else:
            bounds("split", 0)
            checked(ids=True, force=dict(load=0, list=1, clip=0))
        checked(force=dict(load=0, list=0, clip=0, shader=1))       # (a plain frame on the cut stream)
        bounds("thirds", METAL)                             # (other boundaries: the stream is cut again)
        checked(force=dict(load=0, list=0, clip=0))

    def pose_kinds():
        """mat -> dq -> mat -> bind through the dq entry -> dq -> bind through the matrix entry, then each kind undone through its own
        entry; a frame after each."""
        part("pose kinds")
        base(primary)
        for kind, k in (("mat", 0), ("dq", 0), ("mat", 0), ("bind_dq", 0), ("dq", 0), ("bind_mat", 0), ("mat", 0), ("bind_mat", 0), ("dq", 0),
                        ("bind_dq", 0)):
            pose(kind, k)
            checked(force=dict(load=0, clip=0))

    def unwaited():
        """A burst posted under shape A, then swr_morph_set or swr_pose_set* to shape B with no wait in front: the presented images
        are A's, the next frame is B's.  The second family: swr_morph_pose_set, with both halves, NULL joints or NULL weights."""
        part("un-waited")
        base(primary)
        how = ("weights", "pose_mat", "pose_dq")[(seed + 1) % 3]
        if sparse:
            how = ((0, "dq", 0), (0, "mat", None), (None, "mat", 0))[(seed + 1) % 3]
        if how == "pose_mat":
            pose("dq", 0)
        frame("points", present_it=True)                    # (.vertices and .line frames read the shape too)
        frame("lines", present_it=True)
        for k in range(rng.randint(2, 4)):
            frame(force=dict(clip=0), present_it=True)
        pending, st["pending"] = st["pending"], 0            # (no wait in front of the change of shape: it completes the burst itself)
        if sparse:
            morph_pose(*how)
        elif how == "weights":
            weights(1 if st["weights"] == 0 else 0)
        elif how == "pose_mat":
            pose("mat", 0)
        else:
            pose("dq", 0)
        st["pending"] = pending
        frame(color=True, force=dict(load=0, clip=0), present_it=True)
        wait()
        read()

    def overflow():
        """A pose that crowds one tile beyond the first bin guess, one frame, and the first call that waits: each of five in turn.  A
        target of another tile grid in front makes the context guess again."""
        part("overflow")
        mode = dict(hooks_of(seed)).get(K.DEBUG_BIN_MODE, 0)
        emit("hooks", ((K.DEBUG_BIN_MODE, 0),))             # the fixed-stride bins: the only ones a crowded tile overflows
        for k, first in enumerate(("count", "query", "delta", "bounds", "morph_pose" if sparse else "weights")):
            base(primary)
            target(1)
            target(0)
            if first == "delta":                            # (a baseline to differ from)
                frame(color=True, force=dict(load=0, clip=0))
                delta(COLOR | DEPTH)
            pose("mat", "crowd")
            frame(ids=True, color=True, overflow=True, force=dict(rules=("ztest", "metal")[k % 2]))
            if first == "count":
                count((ST.COUNT_PER_PRIMITIVE, ST.COUNT_PER_ITEM)[seed % 2], "all")
            elif first == "query":
                query(40)
            elif first == "delta":
                delta(COLOR | DEPTH)
            elif first == "bounds":
                bounds("split", 0)
            elif first == "morph_pose":
                morph_pose(1, "mat", 0)                     # weights and pose change: the read below is of the shape AND pose it was posted in
            else:
                weights(1 if st["weights"] == 0 else 0)     # the answer and the read below are those of the shape it was posted in
            read()
            pose("mat", 0)
            if st["weights"] != 0:
                weights(0)
        emit("hooks", ((K.DEBUG_BIN_MODE, mode),))          # the seed's own bins again

    def lifetimes():
        part("lifetimes")
        base(primary)
        checked(force=dict(load=0, clip=0))
        # swr_render with a scene identity of the same arrays, twice (the second is cached), then a plain draw: the bind shape, no skin
        sid = 90 + seed
        for _ in range(2):
            f = frame(via="render", color=True, force=dict(load=0, clip=0, shader=0))
            f.scene_id = sid
        checked(force=dict(load=0, list=0, clip=0, shader=0))
        refused("pose_no_skin")
        # an upload of the same size: undeformed, and what the context learned about the bins survives without the old pose
        base(primary)
        checked(force=dict(load=0, clip=0))
        upload(primary)
        checked(force=dict(load=0, clip=0, shader=0))
        refused("pose_no_skin")
        refused("weights_no_targets")
        # an upload of another size, then a new skin and pose
        upload("small")
        checked(force=dict(load=0, shader=0))
        skin(0)
        pose("dq", 0)
        checked(ids=True, force=dict(load=0, shader=0))
        refused("pose_few_joints")
        refused("weights_no_targets")
        targets(0)
        refused("weights_wrong_count")
        weights(0)
        checked(force=dict(load=0))
        weights("zero")
        skin(None)
        refused("pose_no_skin")
        checked(force=dict(load=0))

    def baselines():
        part("baselines")
        base(primary)
        target(0)
        frame(ids=True, color=True, force=dict(load=0, clip=0, list=0, rules="ztest"))
        delta(COLOR | DEPTH)                                 # full: no baseline yet
        small_change = dict(load=1, no_color=0, clip=0, list=0, rules="ztest", cull="none", shader=0, persp=0, transform="affine")
        pose("dq", 0)
        frame(ids=True, force=small_change)                  # a load frame in another pose: few tiles change
        query(70); bounds("split", 0); count(ST.COUNT_PER_PRIMITIVE, "straddle")
        present(); wait(); read(); resolved()
        delta(COLOR | DEPTH)                                 # 0 < tiles_changed < tiles
        few = dict(load=1, list=1, no_color=0, clip=0, cull="none", persp=0, shader=0, transform="affine")
        frame(force=dict(few, rules="painter"), items="few")    # sixty triangles in painter's order: a few colour tiles, no depth at all
        delta(COLOR | DEPTH)                                 # R narrower than the target; the depth image is not written
        frame(force=dict(few, rules="ztest"), items="few2")
        delta(COLOR | DEPTH)
        write()
        delta(COLOR | DEPTH)                                 # swr_target_write keeps the baseline: the written image against it
        refused("count_no_ids"); refused("read_ids_no_ids")
        frame(force=dict(few, rules="ztest"), items="few2")
        delta(COLOR | DEPTH)
        frame(color=True, force=dict(load=0, clip=0))
        delta(COLOR | DEPTH)
        target(0)                                            # the same target again: the baseline is kept
        frame(color=True, force=dict(load=0, clip=0, list=0, rules="ztest", shader=0, persp=0, cull="none", transform="affine"))
        delta(COLOR | DEPTH)
        target(2); target(0)                                 # another size and back: dropped
        frame(color=True, force=dict(load=0, clip=0, list=0, rules="ztest", shader=0, persp=0, cull="none", transform="affine"))
        delta(COLOR | DEPTH)                                 # full = 1
        reset((COLOR, DEPTH)[seed % 2])                      # only that kind starts over
        delta(COLOR | DEPTH)
        frame(color=True, force=dict(load=1, clip=0, list=0, rules="ztest", shader=0, persp=0, cull="none", transform="affine"))   # a static frame
        delta(COLOR | DEPTH)                                 # tiles_changed == 0, dst not written at all
        refused("render_delta_load", UNSUPPORTED)
        frame(via="render_delta", color=True, force=dict(load=0, clip=0, shader=0, list=0))
        frame(via="render_delta", force=dict(load=0, clip=0, shader=0, list=0, no_color=1, rules="ztest"))     # the colour baseline survives
        frame(via="render_delta", color=True, force=dict(load=0, clip=0, shader=0, list=0))

    def bounds_feed():
        """The swr_item_bounds of a posed draw list feed swr_query_depth and swr_count_ids per item."""
        part("bounds feed")
        base(primary)
        target(rng.choice((0, 1)))
        frame(ids=True, color=True, force=dict(load=0, list=1, clip=0, cull="none", rules=rng.choice(("ztest", "metal"))))
        emit("feed")
        query(1); query(2)                                  # (too few boxes to pass nowhere, partly and wholly: exempt from that)
        refused("bounds_clip", UNSUPPORTED)
        refused("count_wrong_n")
        read()

    def step_frame(observer=None, **force):
        """A checked frame with IDs behind a step of a scripted part of the second family, and one observer of it."""
        checked(ids=True, force=dict(dict(load=0, clip=0, list=0), **force))
        if observer == "count":
            count(ST.COUNT_PER_PRIMITIVE, "all")
        elif observer == "query":
            query(40)
        elif observer == "bounds":
            bounds("thirds", 0)
        elif observer == "delta":
            delta(COLOR | DEPTH)

    def morph_kinds():
        """Dense and sparse targets replace each other under a pose, every set with active weights when the next arrives: what the
        new set does not list must come out as the base, whatever the set before left in the morphed arrays.  Both sparse unions
        are partial and neither contains the other.  A frame is drawn and read after every step."""
        part("morph kinds")
        base(primary)
        target(0)
        reset(COLOR | DEPTH)                                # (the part's first delta read is a full one)
        targets(0); weights(0)                              # 1: dense set 0, active: every vertex of the morphed array is written
        step_frame("bounds")
        targets("s0")                                       # 2: sparse over active dense targets: every weight 0, the frame is the base
        step_frame("count")
        weights(0)                                          # 3: outside the union of "s0" nothing of the dense morph is left
        step_frame("query")
        morph_pose(0, "dq", 0)                              #    (the combined call: the other pose kind, NULL weights, NULL joints, and back)
        step_frame()
        morph_pose(None, "dq", 0)
        step_frame()
        morph_pose(0, "mat", None)
        step_frame()
        morph_pose(0, "mat", 0)
        step_frame()
        targets("s1")                                       # 4: another sparse set, another union, over the active "s0"
        step_frame("delta")
        weights(0)
        step_frame("bounds")
        targets(1)                                          # 5: dense set 1 over the active "s1"
        step_frame("count")
        targets("s0"); weights(1)                           # 6: back to "s0" (its empty target at NaN, its non-finite one at -0)
        step_frame("query")
        targets(None, "dense")                              # 7: swr_scene_morph(NULL) removes sparse targets ...
        refused("weights_no_targets")
        step_frame("delta")
        targets(0); weights(0)
        step_frame("bounds")
        targets(None, "sparse")                             #    ... and swr_scene_morph_sparse(NULL) dense ones
        refused("weights_no_targets")
        step_frame("delta")

    def refusals():
        """Every refusal of swr_morph_pose_set and swr_scene_morph_sparse the generator can reach, each followed by a frame: neither
        the weights nor the pose nor the targets have changed.  (The refused calls carry weights, joints and targets that would
        change the frame if they were taken.)"""
        part("refusals")
        base(primary)
        targets(None)
        refused("morph_pose_no_targets")
        step_frame()
        targets("s0"); weights(0)
        for call in ("morph_pose_wrong_count", "morph_pose_few_joints", "morph_pose_bad_kind", "sparse_wrong_vertex_count", "sparse_descending",
                     "sparse_some_normals"):
            refused(call)
            step_frame()
        refused("sparse_too_many", UNSUPPORTED)
        skin(None)
        refused("morph_pose_no_skin")
        step_frame()

    def late_attrs():
        """Sparse normal deltas before any attributes, the attributes, a second attribute array under active weights, then a set without
        normal deltas and the one with them again: without a pose, then under one.  The colour/uv quad of the morphed attributes
        comes from the base for touched and untouched vertices alike: the frames are textured."""
        part("late and replaced attributes")
        tex = dict(load=0, clip=0, list=0, shader=2, no_color=0)
        for posed in (False, True):
            upload(primary)                                 # (no attributes, no skin, no targets)
            if posed:
                skin(0); pose("mat", 0)
            targets("s0")                                   # 1: normal deltas before any attributes
            attrs()                                         # 2: they take effect when the attributes arrive
            weights(0)
            checked(force=tex)
            attrs("other")                                  # 3: other normals and other uv while the weights are active
            checked(force=tex)
            targets("s1")                                   # 4: no normal deltas: the normals are the uploaded ones
            if posed:
                weights(0)                                  #    (without a pose: a frame of the base — one deformed shape fewer)
            checked(force=tex)
            targets("s0")                                   #    normal deltas again
            weights(0)
            checked(force=tex)

    def pair_tour():
        """Every legal (state change, first observer) pair and every ordered pair of observers, dealt over the three seeds; every
        illegal pair as a refusal."""
        part("pairs")
        skew = int(third)       # (twelve observers are a multiple of three: without it a seed would meet the same four behind every change)
        todo = [(s, o) for s in s_ops(seed) for o in o_ops(seed)]
        mine = [p for k, p in enumerate(todo) if (k + skew * (k // len(o_ops(seed))) + seed) % 3 == 0] if seed in STATE_SEEDS + SPARSE_SEEDS + NORMALS_SEEDS \
            else rng.sample(todo, len(todo) // 3)
        rng.shuffle(mine)
        scene = primary
        for s, o in mine:
            base(scene)
            if st["size"] is None or s in ("target_same", "target_other") and rng.random() < 0.3:
                target(rng.randrange(len(SIZES)))
            # what the observer needs from the frame in front of the state change
            if s in ("upload_same", "upload_other") and o in ("count_prim", "count_item", "read_ids"):
                frame(ids=True, color=True, force=dict(list=0, clip=0, load=0))
            elif not s.startswith("frame") and s != "render":
                frame(ids=o in NEEDS_IDS or rng.random() < 0.5, color=True, force=dict(clip=0, load=0))
            change(s)
            if (s, o) in ILLEGAL:
                refused({"count_prim": "count_no_ids", "count_item": "count_item_no_ids", "read_ids": "read_ids_no_ids"}[o])
                continue
            if (s, o) in UNSPECIFIED:
                emit("unchecked", o)                        # (the call succeeds; what it delivers is not looked at)
                continue
            if o in NEEDS_IDS and not (st["ids"] if o == "read_ids" else st["countable"]):
                continue                                    # (a frame of that kind without IDs: the pair is met by another frame)
            if o in ("delta_color",) and not st["color"]:
                continue
            observe(o)
        # observers behind observers: a walk over every ordered pair
        base(scene)
        target(0)
        frame(ids=True, color=True, force=dict(load=0, list=1, clip=0, rules="ztest"))
        order = [(a, b) for a in o_ops(seed) for b in o_ops(seed)]
        mine = [p for k, p in enumerate(order) if (k + skew * (k // len(o_ops(seed))) + seed) % 3 == 0] if seed in STATE_SEEDS + SPARSE_SEEDS + NORMALS_SEEDS \
            else rng.sample(order, len(order) // 3)
        for a, b in mine:
            for o in (a, b):
                if o in NEEDS_IDS and not st["ids"]:
                    frame(ids=True, color=True, force=dict(load=0, list=rng.randrange(2), clip=0, rules="ztest"))
                if o == "load_frame":
                    frame(force=dict(load=1, no_color=0, clip=0), ids=True)
                else:
                    observe(o)
            wait()

    # -- the scripted parts of the third family: each starts from base() under a Phong material ------------------------------------------
    def lit(which="many", observer=None, **force):
        """A Phong frame that shows its normals (colour, no load; without the perspective model, whose budget is the pairs'), read
        back, and a ray cast behind it; observer "bounds": swr_item_bounds in front of it."""
        if observer == "bounds":                            # (in front: the frame is drawn from the stream it may have cut)
            bounds(rng.choice(("split", "one", "thirds")), 0)
        f = checked(force=dict(dict(load=0, clip=0, list=0, persp=0, no_color=0, shader=rng.choice((1, 2))), **force))
        rays(which)
        return f

    def normals_tour():
        """A mode before swr_scene_attributes (no effect on a passthrough frame; in effect when they arrive), then every mode with and
        without FLIP, and under each: the bind pose, dense weights on a set with normal deltas, sparse weights on "s0" (normal deltas)
        and "s1" (none), a matrix pose, a dual-quaternion pose and swr_morph_pose_set.  Then UPLOADED and NULL over the same
        deformations — normal deltas and posed normals are back — and the same mode and flags twice.  On the hub: shared vertices,
        312 of them."""
        part("normals tour")
        upload("hub")
        target(0)
        skin(0); pose("mat", 0); targets("s0"); weights(0)
        normals("smooth", False)                            # before any attributes: kept, and of no effect yet
        checked(ids=True, force=dict(load=0, shader=0, list=0, clip=0, persp=0))
        rays("many")
        attrs()                                             # it takes effect when they arrive
        lit()

        def deformations():
            pose("bind_mat", 0)                             # the bind pose (under the weights of "s0")
            lit()
            targets(0); weights(0)                          # dense weights, normal deltas
            lit("one")
            targets("s0"); weights(1)                       # sparse, normal deltas (the NaN weight on the empty target)
            lit()
            targets("s1"); weights(0)                       # sparse, none
            lit()
            pose("mat", 0)
            lit()
            pose("dq", 0)
            lit("one")
            targets("s0")
            morph_pose(0, "mat", 0)                         # the combined call: back in the shape of base()
            lit()

        for k, (mode, flip) in enumerate((("smooth", False), ("smooth", True), ("flat", True), ("flat", False))):
            if k:                                           # (the second and the fourth change FLIP alone)
                normals(mode, flip)
                lit()
            deformations()
        normals("uploaded")                                 # as a context that never set a mode
        lit()
        deformations()
        normals("flat", True)
        lit()
        normals(None)                                       # NULL means UPLOADED
        lit()
        pose("dq", 0)
        lit()
        for _ in range(2):                                  # the same mode and flags twice: the second changes nothing
            normals("smooth", True)
            lit()

    def rebuild_tour_moded():
        """The six callers of the stream rebuild once under SMOOTH and once under FLAT with FLIP — the mode set before the attributes
        — each observed by a Phong frame, swr_item_bounds and a ray cast; the draw list's items cut a sorted stream."""
        part("rebuild tour under a mode")
        for mode, flip in (("smooth", False), ("flat", True)):
            upload(primary)
            target(0)
            normals(mode, flip)
            skin(0); pose("mat", 0); targets(T0); weights(0)
            checked(ids=True, force=dict(load=0, shader=0, list=0, clip=0, persp=0))
            rays("many")
            attrs()                                         # 1: attributes arriving under a mode that was set earlier
            lit(observer="bounds")
            skin(0)                                         # 2
            lit(observer="bounds")
            pose("dq", 0)                                   # 3
            lit(observer="bounds")
            targets(T1)                                     # 4
            lit(observer="bounds")
            weights(0)                                      # 5
            lit(observer="bounds")
            if seed % 2:                                    # 6: a draw list or swr_item_bounds cuts a Morton-sorted stream
                lit(ids=1, list=1)
                bounds("thirds", 0)
            else:
                bounds("split", 0)
                lit(ids=1, list=1)
            lit(observer="bounds")                          # (a plain frame on the cut stream)
            bounds("thirds", METAL)                         # (other boundaries: the stream is cut again)
            lit()

    def unwaited_normals():
        """A burst posted under one mode and swr_scene_normals behind it with no wait in front: every presented image shows the old
        normals, the next frame the new ones.  Then the same burst with swr_cast_rays behind it."""
        part("un-waited normals")
        for behind in ("normals", "rays"):
            base(primary)
            material(1)
            normals("smooth", behind == "rays")
            for k in range(3):
                frame(force=dict(clip=0, load=0, shader=1 + k % 2, no_color=0, persp=0, cull=("none", "back", "front")[(seed + k) % 3]), present_it=True)
            pending, st["pending"] = st["pending"], 0        # (no wait in front: the call completes the burst itself)
            if behind == "normals":
                normals("flat", bool(seed % 2))
            else:
                rays("many")
            st["pending"] = pending
            frame(force=dict(load=0, clip=0, shader=1, no_color=0, persp=0, cull="none"), present_it=True)
            wait()
            read()
            rays("many")

    def overflow_normals():
        """The overflowed frame under SMOOTH, and the first call that waits: swr_scene_normals with another mode, swr_scene_normals with
        the same mode and flags (its early return lies behind the repair), swr_cast_rays.  The read shows the normals it was drawn with."""
        part("overflow normals")
        mode = dict(hooks_of(seed)).get(K.DEBUG_BIN_MODE, 0)
        emit("hooks", ((K.DEBUG_BIN_MODE, 0),))
        for k, first in enumerate(("other", "same", "rays")):
            base(primary)
            target(1)
            target(0)
            material(1)
            normals("smooth", k == 1)
            pose("mat", "crowd")
            frame(ids=True, overflow=True, force=dict(rules=("ztest", "metal")[k % 2], shader=1, no_color=0))
            if first == "other":
                normals("flat", False)
            elif first == "same":
                normals("smooth", True)
            else:
                rays("one")                                 # (the crowded shape is a sixth of the scene's size: the 65 mostly miss it)
            read()
            pose("mat", 0)
            lit()
        emit("hooks", ((K.DEBUG_BIN_MODE, mode),))

    def mode_lifetimes():
        """The mode against every other state change: discarded by an upload of the same and of another size and by swr_render with a
        new scene identity (the cached second render and the plain draw behind it are un-moded); kept across a second attribute
        array, swr_scene_skin (NULL and a new one) and targets of the other kind."""
        part("mode lifetimes")
        base(primary)
        material(1)
        normals("smooth", False)
        lit()
        upload(primary)                                     # the same size
        attrs()
        lit()
        normals("smooth", False)                            # two cuts of the sorted stream with no pose and no weights, where the mode
        lit()                                               # alone makes the rebuild compute again: swr_item_bounds under SMOOTH (both
        bounds("thirds", 0)                                 # of its kernels, over the adjacency) ...
        lit()
        normals("flat", True)
        lit()
        lit(ids=1, list=1)                                  # ... and a draw list, of other boundaries, under FLAT with FLIP
        lit()
        upload("hub")                                       # another size
        attrs()
        lit()
        base(primary)
        material(1)
        normals("flat", False)
        lit()
        for _ in range(2):                                  # swr_render with a scene identity, twice: the second is cached
            f = frame(via="render", color=True, force=dict(load=0, clip=0, shader=1, persp=0))
            f.scene_id = 190 + seed
        lit()                                               # (a plain draw behind them)
        base(primary)
        normals("smooth", True)
        lit()
        attrs("other")                                      # uv and colour of the new array, normals computed
        lit(shader=2)
        skin(None)
        lit()
        skin(0)                                             # a new skin: the bind pose
        lit()
        pose("mat", 0)
        lit()
        targets(0); weights(0)                              # dense targets over the sparse ones
        lit()
        targets("s1"); weights(0)                           # and sparse ones over them
        lit()

    def rays_change_nothing():
        """A ray cast between an ID frame and its count and swr_read_ids, between two delta reads of each kind (a frame of another
        pose in front of it: the second read reports that frame's tiles, not none), between a frame and its load frame, and between
        swr_present and swr_present_wait."""
        part("rays change nothing")
        base(primary)
        target(0)
        material(1)
        normals("smooth", False)
        plain = dict(load=0, clip=0, list=0, rules="ztest", shader=1, persp=0, no_color=0, cull="none", transform="affine")
        frame(ids=True, force=plain)
        rays("many")
        count(ST.COUNT_PER_PRIMITIVE, "all")
        rays("one")
        emit("read_ids")
        for bit in (COLOR, DEPTH):
            delta(bit)
            pose("dq", 0)
            frame(ids=True, force=plain)
            rays("many")
            delta(bit)                                      # 0 < tiles_changed: the baseline is the first read's
            pose("mat", 0)
        frame(force=plain)
        rays("many")
        frame(force=dict(plain, load=1, list=1), items="few")
        read()
        frame(force=plain)
        present()
        rays("many")
        wait()
        read()

    def refusals3():
        """Every refusal of swr_scene_normals and swr_cast_rays the generator can reach, a frame and a ray cast behind each."""
        part("normals and rays refusals")
        base(primary)
        material(1)
        normals("flat", True)
        lit()
        for call, code in (("normals_bad_mode", BAD_ARG), ("normals_bad_flags", BAD_ARG), ("normals_reserved", BAD_ARG),
                           ("rays_too_many", UNSUPPORTED), ("rays_flags", BAD_ARG), ("rays_nan", BAD_ARG), ("rays_zero_dir", BAD_ARG),
                           ("rays_tmin_tmax", BAD_ARG)):
            refused(call, code)
            lit()

    scripted = [rebuild_tour, pose_kinds, unwaited, overflow, lifetimes, baselines, bounds_feed]
    if sparse:
        scripted += [morph_kinds, refusals, late_attrs]
    if third:
        scripted += [normals_tour, rebuild_tour_moded, unwaited_normals, overflow_normals, mode_lifetimes, rays_change_nothing, refusals3]
    names = {"normals tour": normals_tour, "rebuild tour under a mode": rebuild_tour_moded, "un-waited normals": unwaited_normals,
             "overflow normals": overflow_normals, "mode lifetimes": mode_lifetimes, "rays change nothing": rays_change_nothing,
             "normals and rays refusals": refusals3}
    names |= {"rebuild tour": rebuild_tour, "pose kinds": pose_kinds, "un-waited": unwaited, "overflow": overflow, "lifetimes": lifetimes,
             "baselines": baselines, "bounds feed": bounds_feed, "morph kinds": morph_kinds, "refusals": refusals,
             "late and replaced attributes": late_attrs}
    if only is not None:
        scripted = [names[n] for n in only]
        target(0)
    for p in scripted:
        p()
    if pairs:
        pair_tour()

    # -- the rest is by chance --------------------------------------------------------------------------------------------------------
    if steps:
        part("random")
        base(primary)
        if st["size"] is None:
            target(0)
    for step in range(steps):
        base(primary)
        op = rng.choice(["burst"] * 5 + ["points"] + ["draw"] * 3 + ["observe"] * 6 + ["change"] * 5
                        + ["target", "upload", "render", "rdelta", "write"])
        if op == "burst":
            burst(rng.randint(2, 6))
            if rng.random() < 0.5:
                read()
            wait()
        elif op == "points":
            burst(rng.randint(2, 4), head=rng.choice(("points", "lines")))
            wait()
        elif op == "draw":
            frame(rng.choice(("tri",) * 8 + ("points", "lines")), force=dict(clip=0) if st["scene"] == "big" else None)
        elif op == "observe":
            o = rng.choice(o_ops(seed))
            if not st["image"] or (o in NEEDS_IDS and not st["countable"]) or (o == "present" and st["last"] is None) \
                    or (o == "resolved" and st["last"] is None):
                frame(ids=True, color=True, force=dict(clip=0))
            observe(o)
        elif op == "change":
            s = rng.choice(("pose_mat", "pose_dq", "bind", "weights", "weights_zero", "skin_new", "targets_new", "delta_reset")
                           + (S_OPS_SPARSE[len(S_OPS):] * 2 if sparse else ()) + (S_OPS_NORMALS[len(S_OPS_SPARSE):] * 2 if third else ()))
            change(s)
        elif op == "target":
            target(rng.randrange(len(SIZES)))
        elif op == "upload":
            upload(rng.choice(list(scenes)))
            frame(force=dict(clip=0))
        elif op == "render":
            frame(via="render", force=dict(clip=0))
        elif op == "rdelta":
            frame(via="render_delta", force=dict(clip=0, load=0))
        elif op == "write":
            if st["size"] is not None:
                write()
                frame(force=dict(load=1, clip=0))
    wait()
    return ops


# ---- what the operations are, for the coverage conditions (no NumPy, no GPU) -----------------------------------------------------
def classes(ops):
    """[(index, S_OPS names, O_OPS names)] of every operation that changes state or observes; a SWR_FLAG_LOAD frame does both."""
    out, nv, size = [], None, None
    kind, attrs, nones = None, None, 0                      # the kind of the resident targets, the resident attribute array
    verts = VERTICES
    mode = None                                             # the normals mode of the scene (in effect or not)
    for k, op in enumerate(ops):
        s, o = set(), set()
        name = op[0]
        if name == "upload":
            s.add("upload_same" if verts[op[1]] == nv else "upload_other")
            nv = verts[op[1]]
            kind = attrs = mode = None
        elif name == "attrs":
            s.add("attrs" if attrs in (None, op[1]) else "attrs_other")
            attrs = op[1]
        elif name == "skin":
            s.add("skin_none" if op[1] is None else "skin_new")
        elif name == "pose":
            s.add({"mat": "pose_mat", "dq": "pose_dq"}.get(op[1], "bind"))
        elif name == "targets":
            if op[1] is None:
                s.add("targets_none")
                if kind is not None and none_entry(op, nones) != kind:
                    s.add("targets_none_other_entry")
                nones += 1
                kind = None
            else:
                new = "sparse" if isinstance(op[1], str) else "dense"
                s.add("targets_sparse" if new == "sparse" else "targets_new")
                if kind is not None and kind != new:
                    s.add("targets_swap_kind")
                kind = new
        elif name == "weights":
            s.add("weights_zero" if op[1] in ("zero", None) else "weights")
        elif name == "morph_pose":
            s.add("morph_pose_null_halves" if op[1] is None or op[3] is None else "morph_pose")
        elif name == "target":
            s.add("target_same" if op[1] == size else "target_other")
            size = op[1]
        elif name == "write":
            s.add("target_write")
        elif name == "delta_reset":
            s.add("delta_reset")
        elif name in ("frame", "render", "render_delta"):
            f = op[1]
            if name != "frame":
                s.add("render")                             # (its own gather is part of the call: no observer of what came before)
                nv = verts[f.scene]
                kind, attrs, mode = None, (True if f.shader else None), None
            elif f.kind != "tri":
                s.add("frame_points")
            else:
                s.add("frame_ids" if f.flags & IDS else "frame_noids")
                if f.via == "list":
                    s.add("frame_list")
                if f.flags & LOAD and name == "frame":
                    o.add("load_frame")
        elif name == "read":
            o.add("read")
        elif name == "present":
            o.add("present")
        elif name == "count":
            o.add("count_item" if op[1] == ST.COUNT_PER_ITEM else "count_prim")
        elif name == "query":
            o.add("query")
        elif name == "bounds":
            o.add("bounds")
        elif name == "delta":
            o.update(x for x, b in (("delta_color", COLOR), ("delta_depth", DEPTH)) if op[1] & b)
        elif name == "read_resolved":
            o.add("resolved")
        elif name == "read_ids":
            o.add("read_ids")
        elif name == "feed":
            o.add("bounds")                                 # (its first call; the query and the counts behind it are not credited)
        elif name == "unchecked":
            o.add("unchecked")
        elif name == "normals":
            new = (op[1], op[2]) if op[1] in ("smooth", "flat") else None
            if new is None:
                s.add("normals_null" if op[1] is None else "normals_uploaded")
            elif new == mode:
                s.add("normals_same")
            else:
                s.add("normals_flip" if mode is not None and mode[0] == new[0] else "normals_" + new[0])
            mode = new
        elif name == "rays":
            o.add("rays")
        if s or o:
            out.append((k, s, o))
    return out


def checked_frames(ops):
    """Every triangle frame whose image is compared: presented, read back (plainly, resolved, by a delta read), or rendered."""
    out, last = [], None
    for op in ops:
        if op[0] == "frame":
            last = op[1]
        elif op[0] in ("render", "render_delta"):
            out.append(op[1])
            last = op[1]
        elif op[0] in ("present", "read", "read_resolved", "delta") and last is not None and last.kind == "tri" and last not in out:
            out.append(last)
        elif op[0] in ("target", "write"):
            last = None
    return out


def runs(ops):
    """The un-waited runs of a sequence: [[Frame]] — frames with nothing between them that completes earlier frames."""
    out, cur = [], []
    for op in ops:
        if op[0] == "frame":
            cur.append(op[1])
        elif op[0] in BLOCKING and cur:
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


# ---- the scenes, skins, poses, targets and matrices behind the names ---------------------------------------------------------------
@dataclasses.dataclass
class Scene:
    v: np.ndarray
    i: np.ndarray
    attrs: np.ndarray
    shading: dict           # shader -> scenes.Shading
    skins: dict             # id -> (joint, weight)
    mats: dict              # id -> J x 16 joint matrices ("crowd": every triangle in one tile of the 320 x 192 target)
    dqs: dict               # id -> J x 8 dual quaternions
    targets: dict           # id -> (position deltas, normal deltas)
    weights: dict           # target id -> {id: weights}
    tf: dict                # "aff", "aff2", "per", "per2"
    attrs2: np.ndarray = None   # a second attribute array: other normals, other uv
    sparse: dict = None     # "s0" | "s1" -> [(indices, position deltas[, normal deltas])]; their weights are in `weights`


CROWD = (160.0, 112.0)      # the middle of tile (2, 3) of the 320 x 192 target, in the second of three bands


def _crowd(m, scale, z):
    """J x 16: every joint the same matrix — a uniform scale about the origin, then a shift that puts the origin onto CROWD under the
    affine matrix m (column-major) at depth coordinate z."""
    w, h = SIZES[0]
    nx, ny = CROWD[0] / w * 2 - 1, 1 - CROWD[1] / h * 2
    A = np.array([[m[0], m[4]], [m[1], m[5]]], dtype=np.float64)
    t = np.linalg.solve(A, np.array([nx - m[12] - m[8] * z, ny - m[13] - m[9] * z]))
    return SM.joint_matrix(0.0, scale, float(t[0]), float(t[1]), z)


S0_TARGETS, S1_TARGETS = 4, 6                       # (neither is a number of dense targets of any scene)
S0_EMPTY, S0_NONFINITE = 2, 3                       # the empty target of "s0", and the one that only ever gets weight +-0


def union_of(targets):
    return MS.touched(targets)


def sparse_sets(v, seed, amp):
    """The sparse target sets of a scene and their weights.  "s0": four targets with normal deltas over the vertices [0, 25/64 nv) —
    two that together list every vertex of the range (the first vertex of the scene among them), an empty one, and one of
    non-finite deltas on every fifth.  "s1": six targets without normal deltas over [25/96 nv, nv), the last vertex of the scene
    among them.  Neither union contains the other, each leaves some of the scene out, and 768, 900 and 3 900 vertices give unions
    of 300 and 568, 351 and 666, 1 523 and 2 885: more than 256, no multiple of 64."""
    nv = v.shape[0]
    rng = np.random.default_rng(seed)
    U0, U1 = np.arange(0, nv * 25 // 64), np.arange(nv * 25 // 96, nv)

    def deltas(n, shift):
        return ((np.asarray(shift) + rng.uniform(-0.2, 0.2, (n, 3))) * amp).astype(np.float32)

    def target(idx, shift, normals):
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        t = (idx, deltas(idx.size, shift))
        return t + (rng.uniform(-0.5, 0.5, (idx.size, 3)).astype(np.float32),) if normals else t

    a = rng.uniform(size=U0.size) < 0.7
    a[0] = True
    b = ~a | (rng.uniform(size=U0.size) < 0.4)
    fifth = np.ascontiguousarray(U0[::5], dtype=np.uint32)
    bad = np.tile(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), (fifth.size, 1))
    s0 = [target(U0[a], (0.0, 1.0, 0.0), True), target(U0[b], (0.8, 0.0, 0.3), True),
          (np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.float32)), (fifth, bad, np.full((fifth.size, 3), np.nan, dtype=np.float32))]
    s1, seen = [], np.zeros(U1.size, dtype=bool)
    for k in range(S1_TARGETS - 1):
        m = rng.uniform(size=U1.size) < 0.4
        m[-1] = False
        seen |= m
        s1.append(target(U1[m], rng.uniform(-1.0, 1.0, 3), False))
    s1.append(target(U1[~seen], (-0.6, -0.7, 0.0), False))
    weights = {"s0": {0: np.array([0.8, -0.6, 2.0, 0.0], dtype=np.float32), 1: np.array([-0.5, 0.9, np.nan, -0.0], dtype=np.float32)},
               "s1": {0: rng.uniform(0.4, 1.0, S1_TARGETS).astype(np.float32), 1: (-rng.uniform(0.4, 1.0, S1_TARGETS)).astype(np.float32)}}
    return {"s0": s0, "s1": s1}, weights


def other_attrs(attrs, seed):
    """A second attribute array: other normals and other uv, the padding lanes as they are."""
    rng = np.random.default_rng(seed)
    a = np.array(attrs, dtype=np.float32, copy=True)
    a[:, 0:3] += rng.uniform(-0.4, 0.4, (a.shape[0], 3)).astype(np.float32)
    a[:, 4:6] = a[:, 4:6] * np.float32(1.7) + np.float32(0.13)
    return a


def hub_scene(S, tf):
    """The hub of tests/normals_model.py in the torus's space and under its matrices, with what the sequences need of a scene: two
    random skins of eight joints (as the soups'), two poses of each kind, dense target sets of 3 and 2 with normal deltas.  Its one
    NaN coordinate is made finite: non-finite positions under a mode belong to tests/test_normals.py.  Vertex 0 is shared by 300
    triangles, vertex 304 by none, and 312 vertices are four waves and 56 lanes."""
    v, i = NM.hub(S)
    v = np.array(v, copy=True)
    v[NM.NAN_VERTEX, 0] = np.float32(-0.95)
    nv = v.shape[0]
    attrs = NM.hub_attrs(S)
    rng = np.random.default_rng(0x4B0B)
    skins, mats, dqs, tg, wt = {}, {}, {}, {}, {}
    for sid in (0, 1):
        jj = rng.integers(0, 8, (nv, 4)).astype(np.uint32)
        jj[0, 0], jj[1, 1] = 7, 7
        ww = rng.dirichlet(np.ones(4), nv).astype(np.float32) * rng.uniform(0.93, 1.07, (nv, 1)).astype(np.float32)
        skins[sid] = (jj, ww.astype(np.float32))
    for pid in (0, 1):
        mats[pid] = np.stack([SM.joint_matrix(rng.uniform(-0.3, 0.3), rng.uniform(0.8, 1.05), rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15),
                                              rng.uniform(-0.1, 0.1)) for _ in range(8)])
        dqs[pid] = np.stack([DQ.dq_joint((rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0), rng.uniform(-0.4, 0.4),
                                         (rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1))) for _ in range(8)])
    for tid, nt in ((0, 3), (1, 2)):
        tg[tid] = ((rng.uniform(-0.15, 0.15, (nt, nv, 3)) * (rng.uniform(size=(nt, nv, 1)) < 0.6)).astype(np.float32),
                   rng.uniform(-0.5, 0.5, (nt, nv, 3)).astype(np.float32))
        wt[tid] = {0: rng.uniform(0.4, 1.0, nt).astype(np.float32), 1: (-rng.uniform(0.4, 1.0, nt)).astype(np.float32)}
    shading = {s: dataclasses.replace(S.random_shading(nv, 0x4B, s, shininess_log2=3), attrs=attrs) for s in (1, 2)}
    return Scene(v, i, attrs, shading, skins, mats, dqs, tg, wt, tf)


RAY_SEED = 0x5EED
# how far the xy face the odd-numbered rays are aimed at is enlarged.  1.1 leaves the torus, the hub and "small" between 33 and 56 hits
# of 65 in every shape the sequences cast on.  The 1 300-triangle soup swells under its sparse sets (deltas of 0.4) and random skins
# until it covers that face and more: 57 to 65 hits, too few misses.  At 1.5 it has 32 to 56.
RAY_SPREAD = {"torus": 1.1, "small": 1.1, "hub": 1.1, "big": 1.5}


@functools.lru_cache(maxsize=None)
def ray_set(scene, name):
    """The rays of a scene, built from its bind shape: 65 origins in front of the scene's box, on -z, at 3 * half-depth + 1 from its
    centre, jittered by 0.2 of the half-extents; the even-numbered rays are aimed at the centroid of a random triangle, the
    odd-numbered ones at a random point of the box's xy face enlarged by RAY_SPREAD; tmin 0, tmax 10.  "one" is the first of them."""
    s = world()[scene]
    tri = RY.triangles(s.v, s.i)
    pts = tri.reshape(-1, 3)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    c, e = (lo + hi) / 2, (hi - lo) / 2
    rng = np.random.default_rng(RAY_SEED)
    n = 65
    rays = np.zeros(n, dtype=RY.RAY_DTYPE)
    org = c + np.array([0, 0, -1.0]) * (e[2] * 3 + 1) + rng.uniform(-0.2, 0.2, (n, 3)) * e
    tgt = c + rng.uniform(-1, 1, (n, 3)) * e * np.array([RAY_SPREAD[scene], RAY_SPREAD[scene], 0.0])
    aimed = np.arange(n) % 2 == 0
    tgt[aimed] = tri[rng.integers(0, tri.shape[0], n)].mean(axis=1)[aimed]
    rays["origin"], rays["dir"], rays["tmin"], rays["tmax"] = org, tgt - org, 0, 10
    assert all(RY.check_ray(r) is None for r in rays)
    rays.setflags(write=False)
    return rays if name == "many" else rays[:1]


NEGATIVE_ZERO = {"torus": ((80, 2), (320, 2))}      # (vertex, coordinate): z = +0 as built; 80 is outside the union of "s1", 320 of "s0"


@functools.lru_cache(maxsize=None)
def world():
    """name -> Scene."""
    import swr_amd
    S = swr_amd.scenes
    fs_scenes, fs_mats = FS.world()
    out = {}
    # the torus of tests/skin_model.py and tests/morph_model.py, in its own space (x, y in +-0.75, z in +-0.2)
    v, i = MM.torus(S)
    v = np.array(v, copy=True)
    for k, c in NEGATIVE_ZERO["torus"]:
        assert v[k, c] == 0 and not np.signbit(v[k, c])
        v[k, c] = np.float32(-0.0)                           # (an unlisted -0 stays -0; an applied zero delta would make it +0)
    aff = FS.affine(0.0, 0.95, 0.95, 0.5, 0.0, 0.0, 0.5)
    per = FS.affine(0.0, 0.9, 0.9, 0.5, 0.0, 0.0, 0.5)
    per[11] = np.float32(0.35)                               # w = 1 + 0.35 z
    per2 = per.copy()
    per2[12] = np.float32(0.2)
    tf = {"aff": aff, "aff2": FS.affine(0.3, 0.6, 0.55, 0.4, -0.3, 0.1, 0.5), "per": per, "per2": per2}
    j, w = SM.bend_skin(v)
    d, nd = MM.targets(S, v), MM.normal_targets(v.shape[0])
    two = [MM.LIFT, MM.SHEAR]
    attrs = S.torus_attrs(48, 16)
    out["torus"] = Scene(
        v, i, attrs, {s: dataclasses.replace(S.random_shading(v.shape[0], 0x5A7, s, shininess_log2=3), attrs=attrs) for s in (1, 2)},
        {0: (j, w), 1: (j[:, [1, 0, 3, 2]].copy(), w[:, [1, 0, 3, 2]] * np.float32(0.9))},
        {0: SM.bend_pose(), 1: SM.bend_pose(-0.3, 0.8, -0.15), "crowd": np.stack([_crowd(aff, 0.16, 0.0)] * 4)},
        {0: DQ.twist_pose(), 1: DQ.twist_pose(1.2, (-0.05, 0.06, 0.0))},
        {0: (d, nd), 1: (np.ascontiguousarray(d[two]), np.ascontiguousarray(nd[two]))},
        {0: {0: MM.WEIGHTS_A, 1: MM.WEIGHTS_B}, 1: {0: np.array([0.25, -1.0], dtype=np.float32), 1: np.array([-0.4, 0.6], dtype=np.float32)}},
        tf)
    # the 300- and 1 300-triangle soups of tests/test_frame_sequences.py (eye space: x in +-2.5, y in +-1.8, z in 1 .. 5)
    for k, (name, src) in enumerate((("small", "small"), ("big", "big"))):
        v, i, sh = fs_scenes[src]
        nv = v.shape[0]
        rng = np.random.default_rng(0x51A7E + k)
        skins = {}
        for sid in (0, 1):
            jj = rng.integers(0, 8, (nv, 4)).astype(np.uint32)
            jj[0, 0], jj[1, 1] = 7, 7                          # (the largest joint index is used)
            ww = rng.dirichlet(np.ones(4), nv).astype(np.float32) * rng.uniform(0.93, 1.07, (nv, 1)).astype(np.float32)
            ww[:, 3] -= np.float32(0.05)                       # not normalised, and one weight negative at many vertices
            ww[5] = (1.2, -0.3, 0.0, 0.1)
            skins[sid] = (jj, ww.astype(np.float32))
        mats, dqs = {}, {}
        for pid in (0, 1):
            mats[pid] = np.stack([SM.joint_matrix(rng.uniform(-0.25, 0.25), rng.uniform(0.85, 1.1), rng.uniform(-0.3, 0.3),
                                                  rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2)) for _ in range(8)])
            dqs[pid] = np.stack([DQ.dq_joint((rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0), rng.uniform(-0.3, 0.3),
                                             (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2))) for _ in range(8)])
        mats["crowd"] = np.stack([_crowd(fs_mats["aff"], 0.12, 2.5)] * 8)
        tg, wt = {}, {}
        for tid, nt in ((0, 3), (1, 2)):
            tg[tid] = ((rng.uniform(-0.35, 0.35, (nt, nv, 3)) * (rng.uniform(size=(nt, nv, 1)) < 0.6)).astype(np.float32),
                       rng.uniform(-0.5, 0.5, (nt, nv, 3)).astype(np.float32))
            wt[tid] = {0: rng.uniform(0.4, 1.0, nt).astype(np.float32), 1: (-rng.uniform(0.4, 1.0, nt)).astype(np.float32)}
        out[name] = Scene(v, i, sh[1].attrs, {1: sh[1], 2: sh[2]}, skins, mats, dqs, tg, wt,
                          {n: fs_mats[n] for n in ("aff", "aff2", "per", "per2")})
    out["hub"] = hub_scene(S, tf)
    for k, (name, s) in enumerate(out.items()):
        s.attrs2 = other_attrs(s.attrs, 0xA77 + k)
        s.sparse, w = sparse_sets(s.v, 0x5BA65E + k, 0.15 if name == "torus" else 0.4)
        s.weights.update(w)
    for name, s in out.items():
        assert s.i.size // 3 == SCENES3[name] and s.v.shape[0] == VERTICES[name] and s.mats[0].shape[0] == JOINTS[name] and s.targets[0][0].shape[0] == TARGETS[name][0]
        assert np.array_equal(s.shading[1].attrs, s.shading[2].attrs)
    return out


def normal_shape(sig):
    """The deformation of a generator shape (scene, attrs, skin, pose, targets, weights): what does not move a vertex is left out."""
    scene, _, skin, pose, targets, weights = sig
    return (scene, skin if pose is not None else None, pose, targets if weights is not None else None, weights)


@functools.lru_cache(maxsize=None)
def shape_vertices(scene, skin, pose, targets, weights):
    """The vertices of normal_shape(sig), from the names alone: morph first, then the pose."""
    s = world()[scene]
    v = s.v
    if weights is not None and isinstance(targets, str):
        v = MS.morph_vertices(v, s.sparse[targets], s.weights[targets][weights])
    elif weights is not None:
        v = MM.morph_vertices(v, s.targets[targets][0], s.weights[targets][weights])
    if pose is not None:
        P, table = (SM, s.mats[pose[1]]) if pose[0] == "mat" else (DQ, s.dqs[pose[1]])
        v = P.pose_vertices(v, *s.skins[skin], table)
    return v


def items_of(scene, tf, name="split"):
    """The draw lists: "split" — two ranges that split the scene and an instance of its first triangles, under "per" one item affine
    (tests/test_frame_sequences.py); "thirds" — other boundaries, one item empty, one partly off the target, one behind the eye;
    "one" — the whole scene."""
    s = world()[scene]
    n = s.i.size
    a, b, c = ("aff", "aff2", "aff") if tf == "aff" else ("per", "aff", "per2")
    if name == "one":
        return [(0, n, s.tf[a])]
    if name in ("few", "few2"):                              # sixty triangles shrunk into a corner: a few tiles
        m = np.array(s.tf["aff"], copy=True)
        m[0::4] *= np.float32(0.2)
        m[1::4] *= np.float32(0.2)
        m[12] += np.float32(-0.7 if name == "few" else 0.35)
        m[13] += np.float32(0.6 if name == "few" else -0.55)
        if name == "few2":
            m[14] -= np.float32(0.3)                         # (nearer than what is there)
        return [(0, 3 * 60, m)]
    if name == "split":
        h = n // 2 // 3 * 3
        return [(0, h, s.tf[a]), (h, n - h, s.tf[b]), (0, 3 * 60, K.mirrored(s.tf[c]) if tf == "aff" else s.tf[c])]
    t = n // 3 // 3 * 3
    off = np.array(s.tf["aff"], copy=True)
    off[12] += np.float32(0.9)                               # partly off the target
    behind = np.array(s.tf["aff"], copy=True)
    behind[15] = np.float32(-1.0)                            # w = -1 at every corner
    return [(0, t, s.tf[a]), (t, 0, s.tf[b]), (t, t, off), (2 * t, n - 2 * t, s.tf[b]), (3 * 7, 3 * 40, behind)]


def rect_of(name, w, h):
    """The rectangles of the counts: the whole target, one pixel, an empty one, one that straddles the band cuts of three bands."""
    return {"all": (0, 0, w, h), "pixel": (w // 2, h // 2, w // 2 + 1, h // 2 + 1), "empty": (w // 3, h // 3, w // 3, h // 3 + 5),
            "straddle": (w // 5, h // 3 - 9, w - 7, 2 * h // 3 + 5)}[name]


def boxes_of(depth, n, seed):
    """n boxes for swr_query_depth with z values taken from the depth image: the first three are the whole target under +inf (passes
    nowhere), under the median of its finite depths (passes partly) and under -1e30 (passes wholly); the others are random
    rectangles, a few of them empty, under the minimum, the median or the maximum of their own pixels, or one of these moved by one
    float."""
    h, w = depth.shape
    rng = np.random.default_rng(seed)
    finite = depth[np.isfinite(depth)]
    med = np.float32(np.median(finite)) if finite.size else np.float32(0.5)
    rows = [(0, 0, w, h, np.inf), (0, 0, w, h, med), (0, 0, w, h, np.float32(-1e30))][:n]
    while len(rows) < n:
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        x1, y1 = int(rng.integers(x0, min(w, x0 + 90) + 1)), int(rng.integers(y0, min(h, y0 + 70) + 1))
        part = depth[y0:y1, x0:x1]
        part = part[np.isfinite(part)]
        if part.size == 0:
            z = np.float32(rng.uniform(0, 1))
        else:
            z = np.float32((part.min(), np.median(part), part.max())[int(rng.integers(0, 3))])
            z = (z, np.nextafter(z, np.float32(np.inf)), np.nextafter(z, np.float32(-np.inf)))[int(rng.integers(0, 3))]
        rows.append((x0, y0, x1, y1, z))
    return make_boxes(rows)


def make_boxes(rows):
    """A binding.DEPTH_BOX_DTYPE array of rows (x0, y0, x1, y1, z)."""
    import swr_amd
    a = np.zeros(len(rows), dtype=swr_amd.binding.DEPTH_BOX_DTYPE)
    for k, (x0, y0, x1, y1, z) in enumerate(rows):
        a[k]["x0"], a[k]["y0"], a[k]["x1"], a[k]["y1"], a[k]["z"] = x0, y0, x1, y1, z
    return a


def spec_of(f, v=None):
    """The FrameSpec of a frame of a sequence over the vertices v (None: the scene as uploaded), for tile loads."""
    s = world()[f.scene]
    w, h = SIZES[f.size]
    return FM.FrameSpec(s.v if v is None else v, s.i, w, h, f.flags, s.tf[f.tf], items_of(f.scene, f.tf, f.items) if f.via == "list" else None, None)


# ---- the player -----------------------------------------------------------------------------------------------------------------------
_CACHE, _SHAPES, _CASTS = {}, {}, {}    # frame_model's clear frames, the shapes and the model's ray hits, shared by every run of the module
NORMALS = {"uploaded": NM.UPLOADED, "smooth": NM.SMOOTH, "flat": NM.FLAT}


def play(swr, oracle, ops, bands, stats=None, model=None):
    """Plays `ops` on one context of `swr` and compares every answer with tests/state_model.py."""
    B = swr.binding
    W = world()
    pool, dsts = {}, {}
    stats = {} if stats is None else stats
    M = model if model is not None else ST.State(oracle, _CACHE, _SHAPES, _CASTS)
    clock = [0.0]

    def timed(fn, *a, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*a, **kw)
        finally:
            clock[0] += time.perf_counter() - t0

    def images(size):
        if size not in pool:
            w, h = SIZES[size]
            pool[size] = [(swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)) for _ in range(IMAGES)]
        return pool[size]

    def dst(size, bit, which):
        """The two destinations of the delta reads of one kind on one target size: a page-locked and a pageable image.  They hold
        the same bytes: the caller's promise is about the content, not the pointer."""
        if (size, bit) not in dsts:
            w, h = size
            shape, dtype = ((h, w, 4), np.uint8) if bit == COLOR else ((h, w), np.float32)
            pinned = swr.HostImage(shape, dtype)
            pinned.array.view(np.uint8)[...] = 0xA5
            dsts[(size, bit)] = {"pinned": pinned, "pageable": np.full(w * h * 4, 0xA5, dtype=np.uint8).view(dtype).reshape(shape)}
        return dsts[(size, bit)][which]

    def content(x):
        return x.array if hasattr(x, "array") else x

    def state():
        return f"scene {scene}, shape {M.shape()[2] if M.v is not None else None}, pose {M.pose_kind}, weights {cur['weights']}"

    def check_image(got, want, what):
        FM.same(got, want, f"{what} ({state()})")
        stats["checked"] = stats.get("checked", 0) + 1

    def check_delta(bit, buf, before, got_stats, what, full_bytes):
        d, out = timed(M.delta, bit, before, [b[1:] for b in ctx.bands()])
        kind = "colour" if bit == COLOR else "depth"
        after = ST.DM.as_words(content(buf))
        bad = np.nonzero(after != out)
        assert bad[0].size == 0, f"{what}: {kind} delta read: {bad[0].size} words of dst differ from the model, first at " \
                                 f"(y,x)=({bad[0][0]},{bad[1][0]}); R = {d.band_rects} ({state()})"
        g = got_stats
        assert (g.tiles, g.tiles_changed, g.full) == (d.tiles, d.tiles_changed, d.full), \
            f"{what}: {kind} delta stats tiles {g.tiles}/{d.tiles}, changed {g.tiles_changed}/{d.tiles_changed}, full {g.full}/{d.full} ({state()})"
        assert (g.x0, g.y0, g.x1, g.y1) == tuple(d.rect), f"{what}: {kind} delta rectangle {(g.x0, g.y0, g.x1, g.y1)}, model {d.rect} ({state()})"
        lo, hi = (full_bytes, full_bytes) if d.full else (4 * d.changed_pixels, d.rect_bytes)
        assert lo <= g.bytes_copied <= hi, f"{what}: {kind} delta bytes_copied {g.bytes_copied} outside [{lo}, {hi}] ({state()})"
        assert g.reserved == 0
        narrow = any(r is not None and r[2] - r[0] < M.size[0] for r in d.band_rects)
        stats["deltas"] = stats.get("deltas", []) + [(d.tiles_changed, d.tiles, d.full, narrow)]
        # the other destination gets the same bytes
        for other in dsts[(M.size, bit)].values():
            if other is not buf:
                content(other)[...] = content(buf)

    def check_refused(call, code, fn, what):
        got = 0
        try:
            fn()
        except swr.SwrError as e:
            got = e.code
        assert got == code, f"{what}: {call} returned {got}, not {code} ({state()})"
        stats["refused"] = stats.get("refused", 0) + 1

    def weights_of(wid):
        if wid is None:
            return None
        if wid == "zero":
            w = np.zeros(M.target_count(), dtype=np.float32)
            w[::2] = np.float32(-0.0)
            return w
        return D.weights[cur["targets"]][wid]

    def morph_pose_refused(call, code, w, table, dq, what):
        check_refused(call, code, lambda: ctx.morph_pose_set(w, table, dq=dq), what)
        with pytest.raises(ST.Refused):
            M.morph_pose(w, "dq" if dq else "mat", table)

    def sparse_refused(call, code, targets, what, vertex_count=None):
        check_refused(call, code, lambda: ctx.scene_morph_sparse(targets, vertex_count), what)
        with pytest.raises(ST.Refused):
            M.set_targets_sparse(targets, vertex_count)

    def raw_normals(mode, flags, reserved):
        """swr_scene_normals with any mode, flag and reserved words: the code it returns."""
        if hasattr(ctx, "raw_scene_normals"):                   # (the stand-in of tests/test_state_model.py)
            return ctx.raw_scene_normals(mode, flags, reserved)
        import ctypes
        return swr.load_library().swr_scene_normals(ctx._h, ctypes.byref(B.Normals(mode, flags, (ctypes.c_int32 * 2)(*reserved))))

    def raw_rays(rays, n, flags):
        """swr_cast_rays with any n and flags: (the code it returns, the hit records as it left them)."""
        hits = np.full(4 * max(len(rays), 1), 0xA5A5A5A5, dtype=np.uint32)
        if hasattr(ctx, "raw_cast_rays"):
            return ctx.raw_cast_rays(rays, n, flags), hits
        return swr.load_library().swr_cast_rays(ctx._h, rays.ctypes.data, n, flags, hits.ctypes.data), hits

    def check_rays(name, what):
        rays = ray_set(scene, name)
        got = ctx.cast_rays(rays)
        want = timed(M.cast, rays)
        bad = [j for j in range(rays.size) if got[j].tobytes() != want[j].tobytes()]
        assert not bad, f"{what}: {len(bad)} of {rays.size} hit records differ, first ray {bad[0]}: {got[bad[0]]} vs {want[bad[0]]} ({state()})"
        stats.setdefault("rays", []).append((k, name, scene, M.shape()[2], want))

    def normals_refused(call, code, mode, flags, reserved, what):
        check_refused(call, code, lambda: ctx._check(raw_normals(mode, flags, reserved)), what)
        with pytest.raises(ST.Refused):
            M.set_normals(mode, flags, reserved)

    def rays_refused(call, code, rays, what, n=None, flags=0):
        out = []
        check_refused(call, code, lambda: (out.append(raw_rays(rays, len(rays) if n is None else n, flags)), ctx._check(out[0][0])), what)
        assert (out[0][1] == 0xA5A5A5A5).all(), f"{what}: a refused swr_cast_rays wrote"
        with pytest.raises(ST.Refused):
            M.cast(rays, n, flags)

    cur = dict(weights=None, nones=0)
    scene = size = None
    try:
        with swr.Context(0, device_count=bands) as ctx:
            pending = []
            for k, op in enumerate(ops):
                name = op[0]
                stats["op"] = k
                what = f"op {k} {op[:1] + tuple(x for x in op[1:] if not isinstance(x, Frame))}"
                D = W[scene] if scene is not None else None
                if name == "hooks":
                    for key, value in op[1]:
                        ctx.debug_set(key, value)
                elif name == "part":
                    stats.setdefault("parts", {})[op[1]] = k
                elif name == "upload":
                    scene = op[1]
                    D = W[scene]
                    ctx.scene_upload(D.v, D.i)
                    M.upload(D.v, D.i)
                    cur["weights"] = None
                elif name == "target":
                    size = op[1]
                    ctx.target_set(*SIZES[size])
                    M.target_set(*SIZES[size])
                elif name == "attrs":
                    a = D.attrs if op[1] is True else D.attrs2
                    ctx.scene_attributes(a)
                    M.attributes(a)
                elif name == "material":
                    sh = D.shading[op[1]] if op[1] else None
                    if sh is not None and sh.texture is not None and cur.get("texture") is not sh.texture:
                        ctx.texture_upload(sh.texture)      # (blocking: once per texture, so that a material change completes no burst)
                        cur["texture"] = sh.texture
                    ctx.material_set(B.Material.from_shading(sh) if sh is not None else None)
                    M.set_material(sh)
                elif name == "skin":
                    jw = D.skins[op[1]] if op[1] is not None else (None, None)
                    ctx.scene_skin(*jw)
                    M.set_skin(*jw)
                elif name == "pose":
                    kind, pid = op[1], op[2]
                    if kind == "mat":
                        ctx.pose_set(D.mats[pid]); M.set_pose("mat", D.mats[pid])
                    elif kind == "dq":
                        ctx.pose_set_dq(D.dqs[pid]); M.set_pose("dq", D.dqs[pid])
                    elif kind == "bind_mat":
                        ctx.pose_set(None); M.set_pose("mat", None)
                    else:
                        ctx.pose_set_dq(None); M.set_pose("dq", None)
                elif name == "targets":
                    if op[1] is None:                       # NULL through either entry removes whichever kind is resident
                        if none_entry(op, cur["nones"]) == "dense":
                            ctx.scene_morph(None); M.set_targets(None)
                        else:
                            ctx.scene_morph_sparse(None); M.set_targets_sparse(None)
                        cur["nones"] += 1
                    elif isinstance(op[1], str):
                        ctx.scene_morph_sparse(D.sparse[op[1]])
                        M.set_targets_sparse(D.sparse[op[1]])
                    else:
                        ctx.scene_morph(*D.targets[op[1]])
                        M.set_targets(*D.targets[op[1]])
                    cur.update(targets=op[1], weights=None)
                elif name == "weights":
                    w = weights_of(op[1])
                    ctx.morph_set(w)
                    M.set_weights(w)
                    cur["weights"] = op[1]
                elif name == "morph_pose":
                    w, kind = weights_of(op[1]), op[2]
                    table = None if op[3] is None else (D.mats if kind == "mat" else D.dqs)[op[3]]
                    ctx.morph_pose_set(w, table, dq=kind == "dq")
                    M.morph_pose(w, kind, table)
                    cur["weights"] = op[1]
                elif name == "normals":
                    ctx.scene_normals(op[1], op[2])
                    M.set_normals(None if op[1] is None else NORMALS[op[1]], NM.FLIP if op[2] else 0)
                elif name == "rays":
                    check_rays(op[1], what)
                elif name == "write":
                    c, d = TP.start_images(op[1], *SIZES[size])
                    ctx.target_write(c, d)
                    M.target_write(c, d)
                elif name == "delta_reset":
                    ctx.delta_reset(op[1])
                    M.delta_reset(op[1])
                elif name == "frame":
                    f = op[1]
                    assert (f.scene, f.size) == (scene, size), what
                    if f.via == "list":
                        items = items_of(f.scene, f.tf, f.items)
                        ctx.draw_list(items, f.flags)
                        timed(M.frame, f.flags, None, items)
                    else:
                        prim = {"tri": 0, "lines": 1, "points": 2}[f.kind]
                        ctx.draw(D.tf[f.tf], f.flags, prim)
                        timed(M.frame, f.flags, D.tf[f.tf], None, prim)
                    stats.setdefault("shapes", []).append((M.shape()[2], scene))
                    stats.setdefault("frame_ops", []).append(k)
                elif name in ("render", "render_delta"):
                    f = op[1]
                    w, h = SIZES[f.size]
                    sh = D.shading[f.shader] if f.shader else None
                    start = TP.start_images(f.write, w, h) if f.flags & LOAD else None
                    if name == "render":
                        c, d = ctx.render(D.v, D.i, D.tf[f.tf], w, h, f.flags, shading=sh, scene_id=f.scene_id,
                                          color=None if f.flags & NC or start is None else start[0].copy(),
                                          depth=None if start is None else start[1].copy())
                        want = timed(M.render, D.v, D.i, D.tf[f.tf], w, h, f.flags, sh, start)
                        check_image((None if f.flags & NC else c, d, ctx.read_ids() if f.flags & IDS else None), want, what)
                    else:
                        bc, bd = dst((w, h), COLOR, op[2]), dst((w, h), DEPTH, op[2])
                        before = (content(bc).copy(), content(bd).copy())
                        sc, sd = ctx.render_delta(D.v, D.i, D.tf[f.tf], w, h, None if f.flags & NC else bc, bd, f.flags, shading=sh,
                                                  scene_id=f.scene_id)
                        timed(M.render, D.v, D.i, D.tf[f.tf], w, h, f.flags, sh, None)
                        if f.flags & NC:
                            assert (sc.tiles, sc.tiles_changed, sc.bytes_copied, sc.full) == (0, 0, 0, 0), f"{what}: colour stats under NO_COLOR"
                            assert np.array_equal(content(bc), before[0]), f"{what}: the colour destination was written under NO_COLOR"
                        else:
                            check_delta(COLOR, bc, before[0], sc, what, w * h * 4)
                        check_delta(DEPTH, bd, before[1], sd, what, w * h * 4)
                    cur["weights"] = None
                    cur["texture"] = sh.texture if sh is not None and sh.texture is not None else cur.get("texture")
                elif name == "present":
                    ci, di = images(size)[op[1]]
                    ctx.present(ci, di)
                    pending.append((op[1], size, M.image, k))
                elif name == "wait":
                    ctx.present_wait()
                    for slot, sz, want, at in pending:
                        ci, di = images(sz)[slot]
                        check_image((None if want[0] is None else ci.array.copy(), di.array.copy(), None), want,
                                    f"{what}: presented at op {at}")
                    pending = []
                elif name == "sync":
                    ctx.sync()
                elif name == "read":
                    want = M.read()
                    check_image((None if want[0] is None else ctx.read_color(), ctx.read_depth(), ctx.read_ids() if M.ids_ok else None),
                                want, what)
                elif name == "read_ids":
                    check_image((None, None, ctx.read_ids()), (None, None, M.read_ids()), what)
                elif name == "read_resolved":
                    S, filt, which = op[1:]
                    gc = ctx.read_color_resolved(S) if which in ("color", "both") and M.image[0] is not None else None
                    gd = ctx.read_depth_resolved(S, filt) if which in ("depth", "both") else None
                    check_image((gc, gd, None), timed(M.resolved, S, filt), what)
                elif name == "count":
                    group, rect = op[1], rect_of(op[2], *SIZES[size])
                    n = (1 if M.last.items is None else len(M.last.items)) if group == ST.COUNT_PER_ITEM else M.last.prims
                    counts, none = ctx.count_ids(group, rect, n)
                    wc, wn = timed(M.count, group, rect, n, B.list_ids_to_items)
                    assert none == wn and np.array_equal(counts, wc), \
                        f"{what}: {int((counts != wc).sum())} of {n} counts differ, none {none} vs {wn} ({state()})"
                    assert int(counts.sum()) + none == (rect[2] - rect[0]) * (rect[3] - rect[1]), f"{what}: the counts do not add up"
                    stats["counts"] = stats.get("counts", []) + [(group, op[2], int((wc != 0).sum()))]
                elif name == "query":
                    depth = M.depth()
                    boxes = boxes_of(depth, op[1], op[2])
                    got = ctx.query_depth(boxes)
                    want = timed(TD.expected, depth, boxes)
                    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {boxes.size} boxes differ, first " \
                                                      f"{int(np.nonzero(got != want)[0][0])} ({state()})"
                    area = (boxes["x1"] - boxes["x0"]) * (boxes["y1"] - boxes["y0"])
                    flat = M.cleared or not np.isfinite(depth).any()        # (nothing a box could pass partly)
                    stats["queries"] = stats.get("queries", []) + [(int((want[area > 0] == 0).sum()), int(((want > 0) & (want < area)).sum()),
                                                                    int(((want == area) & (area > 0)).sum()), flat, int(boxes.size))]
                elif name == "bounds":
                    items = items_of(scene, "aff" if op[1] != "split" else ("aff", "per")[k % 2], op[1])
                    got = ctx.item_bounds(items, op[2])
                    want = timed(M.bounds, items, op[2])
                    wrong = [j for j in range(len(items)) if got[j].tobytes() != want[j].tobytes()]
                    assert ST.IB.same(got, want), f"{what}: bounds records differ: {wrong} ({state()})"
                    stats["bounds"] = stats.get("bounds", []) + [want]
                elif name == "delta":
                    w, h = SIZES[size]
                    for bit, fn in ((COLOR, ctx.read_color_delta), (DEPTH, ctx.read_depth_delta)):
                        if op[1] & bit:
                            buf = dst((w, h), bit, op[2])
                            before = content(buf).copy()
                            check_delta(bit, buf, before, fn(buf), what, w * h * 4)
                elif name == "feed":
                    # the bounds of the posed list that was just drawn feed the depth query and the per-item counts
                    items = M.last.items
                    w, h = SIZES[size]
                    got = ctx.item_bounds(items, M.last.flags & METAL)
                    want = timed(M.bounds, items, M.last.flags & METAL)
                    assert ST.IB.same(got, want), f"{what}: bounds records differ ({state()})"
                    rows = [(b["x0"], b["y0"], b["x1"], b["y1"], np.nextafter(b["zmin"], np.float32(-np.inf))) for b in got]
                    boxes = make_boxes(rows)
                    passed = ctx.query_depth(boxes)
                    assert np.array_equal(passed, TD.expected(M.depth(), boxes)), f"{what}: query over the bounds ({state()})"
                    whole, none = ctx.count_ids(ST.COUNT_PER_ITEM, None, len(items))
                    ww, wn = M.count(ST.COUNT_PER_ITEM, (0, 0, w, h), len(items), B.list_ids_to_items)
                    assert none == wn and np.array_equal(whole, ww), f"{what}: counts per item ({state()})"
                    assert (whole > 0).sum() >= 2, f"{what}: fewer than two items are visible"
                    stats["counts"] = stats.get("counts", []) + [(ST.COUNT_PER_ITEM, "all", int((ww != 0).sum()))]
                    for j, b in enumerate(got):
                        own, _ = ctx.count_ids(ST.COUNT_PER_ITEM, (int(b["x0"]), int(b["y0"]), int(b["x1"]), int(b["y1"])), len(items))
                        assert own[j] == whole[j], f"{what}: item {j} shows {whole[j]} pixels, {own[j]} inside its own rectangle ({state()})"
                elif name == "unchecked":
                    # an order the header leaves open: the call succeeds, nothing of what it delivers is compared, and every later
                    # answer is still the model's (a delta read's baseline is dropped again: its content is as open as the image)
                    w, h = SIZES[size]
                    if op[1] == "read":
                        ctx.read_color(); ctx.read_depth()
                    elif op[1] == "present":
                        ctx.present(*images(size)[IMAGES - 1])
                        ctx.present_wait()
                        for slot, sz, want, at in pending:
                            ci, di = images(sz)[slot]
                            check_image((None if want[0] is None else ci.array.copy(), di.array.copy(), None), want, f"{what}: presented at op {at}")
                        pending = []
                    elif op[1] == "resolved":
                        ctx.read_color_resolved(2); ctx.read_depth_resolved(2, RM.MIN)
                    else:
                        bit = COLOR if op[1] == "delta_color" else DEPTH
                        (ctx.read_color_delta if bit == COLOR else ctx.read_depth_delta)(dst((w, h), bit, "pageable"))
                        ctx.delta_reset(bit)
                        M.delta_reset(bit)
                    stats["unchecked"] = stats.get("unchecked", 0) + 1
                elif name == "refused":
                    call, code = op[1], op[2]
                    w, h = SIZES[size]
                    if call in ("count_no_ids", "count_item_no_ids"):
                        group = ST.COUNT_PER_ITEM if "item" in call else ST.COUNT_PER_PRIMITIVE
                        # the n the last frame requires: only the unreadable IDs can be the reason
                        n = D.i.size // 3 if M.last is None else M.last.prims
                        if group:
                            n = 1 if M.last is None or M.last.items is None else len(M.last.items)
                        check_refused(call, code, lambda: ctx.count_ids(group, None, n), what)
                        with pytest.raises(ST.Refused):
                            M.count(group, (0, 0, w, h), n, B.list_ids_to_items)
                    elif call == "read_ids_no_ids":
                        out = np.full((h, w), 0xA5A5A5A5, dtype=np.uint32)
                        check_refused(call, code, lambda: ctx.read_ids(out), what)
                        assert (out == 0xA5A5A5A5).all(), f"{what}: a refused swr_read_ids wrote"
                        with pytest.raises(ST.Refused):
                            M.read_ids()
                    elif call == "count_wrong_n":
                        n = M.last.prims + 1
                        check_refused(call, code, lambda: ctx.count_ids(ST.COUNT_PER_PRIMITIVE, None, n), what)
                        with pytest.raises(ST.Refused):
                            M.count(ST.COUNT_PER_PRIMITIVE, (0, 0, w, h), n, B.list_ids_to_items)
                    elif call == "pose_few_joints":
                        few = D.mats[0][:JOINTS[scene] - 1]
                        check_refused(call, code, lambda: ctx.pose_set(few), what)
                        check_refused(call, code, lambda: ctx.pose_set_dq(D.dqs[0][:JOINTS[scene] - 1]), what)
                        with pytest.raises(ST.Refused):
                            M.set_pose("mat", few)
                    elif call == "pose_no_skin":
                        check_refused(call, code, lambda: ctx.pose_set(D.mats[0]), what)
                        check_refused(call, code, lambda: ctx.pose_set_dq(D.dqs[0]), what)
                        with pytest.raises(ST.Refused):
                            M.set_pose("mat", D.mats[0])
                    elif call == "weights_no_targets":
                        check_refused(call, code, lambda: ctx.morph_set(D.weights[0][0]), what)
                        with pytest.raises(ST.Refused):
                            M.set_weights(D.weights[0][0])
                    elif call == "weights_wrong_count":
                        wrong = np.ones(M.targets[0].shape[0] + 1, dtype=np.float32)
                        check_refused(call, code, lambda: ctx.morph_set(wrong), what)
                        with pytest.raises(ST.Refused):
                            M.set_weights(wrong)
                    elif call == "morph_pose_no_targets":
                        morph_pose_refused(call, code, None, D.mats[1], False, what)
                        morph_pose_refused(call, code, D.weights["s0"][1], D.dqs[1], True, what)
                    elif call == "morph_pose_no_skin":          # (weights that would be taken)
                        other = D.weights[cur["targets"]][1 if cur["weights"] == 0 else 0]
                        morph_pose_refused(call, code, other, D.mats[1], False, what)
                        morph_pose_refused(call, code, other, D.dqs[1], True, what)
                    elif call == "morph_pose_wrong_count":      # (a pose that would be taken; one weight too many, one too few)
                        morph_pose_refused(call, code, np.ones(M.target_count() + 1, dtype=np.float32), D.dqs[1], True, what)
                        morph_pose_refused(call, code, np.ones(M.target_count() - 1, dtype=np.float32), D.mats[1], False, what)
                    elif call == "morph_pose_few_joints":       # (weights that would be taken)
                        other = D.weights[cur["targets"]][1 if cur["weights"] == 0 else 0]
                        morph_pose_refused(call, code, other, D.mats[1][:JOINTS[scene] - 1], False, what)
                        morph_pose_refused(call, code, other, D.dqs[1][:JOINTS[scene] - 1], True, what)
                    elif call == "morph_pose_bad_kind":
                        other = D.weights[cur["targets"]][1 if cur["weights"] == 0 else 0]
                        for bad in (2, -1):
                            check_refused(call, code, lambda: ctx.morph_pose_set(other, D.mats[1], pose_kind=bad), what)
                        with pytest.raises(ST.Refused):
                            M.morph_pose(other, "neither", D.mats[1])
                    elif call == "sparse_wrong_vertex_count":
                        sparse_refused(call, code, D.sparse["s1"], what, D.v.shape[0] - 1)
                    elif call == "sparse_descending":
                        t = list(D.sparse["s1"])
                        idx = t[1][0].copy()
                        idx[[3, 4]] = idx[[4, 3]]
                        t[1] = (idx,) + t[1][1:]
                        sparse_refused(call, code, t, what)
                        idx = t[1][0].copy()
                        idx[3] = idx[4]                      # (not STRICTLY ascending)
                        t[1] = (idx,) + t[1][1:]
                        sparse_refused(call, code, t, what)
                        t[1] = D.sparse["s1"][1]
                        idx = t[2][0].copy()
                        idx[-1] = D.v.shape[0]              # (out of range)
                        t[2] = (idx,) + t[2][1:]
                        sparse_refused(call, code, t, what)
                    elif call == "sparse_some_normals":
                        t = list(D.sparse["s0"])
                        t[1] = t[1][:2]                     # (the empty target gives none either way: it does not count)
                        sparse_refused(call, code, t, what)
                    elif call == "sparse_too_many":
                        none = (np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.float32))
                        sparse_refused(call, code, [D.sparse["s1"][0]] + [none] * ST.MORPH_MAX_TARGETS, what)
                    elif call.startswith("normals_"):            # (each would change the next frame if it were taken)
                        other = NM.FLAT if M.normals is None or M.normals[0] == NM.SMOOTH else NM.SMOOTH
                        if call == "normals_bad_mode":
                            for bad in (3, -1):
                                normals_refused(call, code, bad, 0, (0, 0), what)
                        elif call == "normals_bad_flags":
                            for bad in (2, NM.FLIP | 1 << 31):
                                normals_refused(call, code, other, bad, (0, 0), what)
                        else:
                            for bad in ((1, 0), (0, -1)):
                                normals_refused(call, code, other, 0, bad, what)
                    elif call.startswith("rays_"):
                        rays = np.array(ray_set(scene, "many"))
                        if call == "rays_too_many":
                            rays_refused(call, code, np.resize(rays, ST.RAYS_MAX + 1), what)
                        elif call == "rays_flags":
                            for bad in (1, 1 << 31):
                                rays_refused(call, code, rays, what, flags=bad)
                        elif call == "rays_nan":
                            for field, j, bad in (("origin", 1, np.nan), ("dir", 2, np.inf), ("tmin", None, -np.inf), ("tmax", None, np.nan)):
                                r = rays.copy()
                                if j is None:
                                    r[field][64] = bad
                                else:
                                    r[field][64, j] = bad
                                rays_refused(call, code, r, what)
                        elif call == "rays_zero_dir":
                            r = rays.copy()
                            r["dir"][33] = (0.0, -0.0, 0.0)
                            rays_refused(call, code, r, what)
                        else:
                            r = rays.copy()
                            r["tmin"][0], r["tmax"][0] = 2.0, 1.0
                            rays_refused(call, code, r, what)
                    elif call == "bounds_clip":
                        check_refused(call, code, lambda: ctx.item_bounds(items_of(scene, "aff"), CLIP), what)
                        with pytest.raises(ST.Refused):
                            M.bounds(items_of(scene, "aff"), CLIP)
                    elif call == "render_delta_load":
                        bc, bd = dst((w, h), COLOR, "pageable"), dst((w, h), DEPTH, "pageable")
                        before = (bc.copy(), bd.copy())
                        check_refused(call, code, lambda: ctx.render_delta(D.v, D.i, D.tf["aff"], w, h, bc, bd, DT | LOAD), what)
                        assert np.array_equal(bc, before[0]) and bd.tobytes() == before[1].tobytes(), f"{what}: a refused swr_render_delta wrote"
                    else:
                        raise AssertionError(call)
                else:
                    raise AssertionError(op)
            ctx.present_wait()
            assert not pending
    finally:
        for lst in pool.values():
            for a, b in lst:
                a.free(); b.free()
        for d in dsts.values():
            d["pinned"].free()
    stats["model_s"] = stats.get("model_s", 0.0) + clock[0]
    return stats


# SWR_SEQUENCE_SEEDS=N adds N more sequences (seeds 200..; all of the second family) per scheduler and band count
_EXTRA = [200 + k for k in range(int(os.environ.get("SWR_SEQUENCE_SEEDS", "0")))]


@pytest.mark.parametrize("env", [{}, {"SWR_LANES": "0"}], ids=["lanes", "SWR_LANES=0"])
@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("seed", list(STATE_SEEDS + SPARSE_SEEDS + NORMALS_SEEDS) + _EXTRA)
def test_state_sequences(swr, oracle, monkeypatch, seed, bands, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t0 = time.perf_counter()
    stats = play(swr, oracle, sequence(seed), bands)
    print(f"seed {seed} bands {bands} {env}: {stats['checked']} images, {len(stats.get('counts', []))} counts, "
          f"{len(stats.get('queries', []))} queries, {len(stats.get('bounds', []))} bounds, {len(stats.get('deltas', []))} delta reads, "
          f"{len(stats.get('rays', []))} ray casts, {stats.get('refused', 0)} refusals checked, {time.perf_counter() - t0:.1f} s ({stats['model_s']:.1f} s in the model)")


# ---- the case the pairs found ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("order", ["larger first", "smaller first", "same size"])
def test_ids_are_unreadable_after_an_upload(swr, oracle, order, bands):
    """An ID frame, then swr_scene_upload, then swr_count_ids.  The IDs number the primitives of the scene that is gone.  Before the
    header named the upload among the refusals, the library measured n against the NEW scene: after a 1 536-triangle frame and an
    upload of 300 triangles it took n = 300, dropped every pixel with an ID >= 300 and returned counts whose sum with `none` was
    short of the rectangle's area, and it refused the last frame's own n = 1 536.  Now swr_count_ids and swr_read_ids return
    SWR_ERR_BAD_ARG for every n, write nothing, and the colour and depth images stay; the next ID frame is counted as ever."""
    B, W = swr.binding, world()
    first, second = {"larger first": ("torus", "small"), "smaller first": ("small", "torus"), "same size": ("torus", "torus")}[order]
    a, b = W[first], W[second]
    w, h = SIZES[0]
    M = ST.State(oracle, _CACHE, _SHAPES)

    def code_of(fn):
        try:
            fn()
        except swr.SwrError as e:
            return e.code
        return 0

    with swr.Context(0, device_count=bands) as ctx:
        ctx.target_set(w, h); M.target_set(w, h)
        ctx.scene_upload(a.v, a.i); M.upload(a.v, a.i)
        ctx.draw(a.tf["aff"], DT | IDS); want = M.frame(DT | IDS, a.tf["aff"])
        n = a.i.size // 3
        counts, none = ctx.count_ids(ST.COUNT_PER_PRIMITIVE, None, n)
        wc, wn = M.count(ST.COUNT_PER_PRIMITIVE, (0, 0, w, h), n, B.list_ids_to_items)
        assert none == wn and np.array_equal(counts, wc) and int(counts.sum()) + none == w * h and (counts > 0).sum() > 100
        ctx.scene_upload(b.v, b.i); M.upload(b.v, b.i)
        for m in sorted({a.i.size // 3, b.i.size // 3}):
            assert code_of(lambda: ctx.count_ids(ST.COUNT_PER_PRIMITIVE, None, m)) == BAD_ARG, f"{order}: n = {m} per primitive"
        assert code_of(lambda: ctx.count_ids(ST.COUNT_PER_ITEM, None, 1)) == BAD_ARG, f"{order}: per item"
        out = np.full((h, w), 0xA5A5A5A5, dtype=np.uint32)
        assert code_of(lambda: ctx.read_ids(out)) == BAD_ARG and (out == 0xA5A5A5A5).all(), f"{order}: swr_read_ids"
        with pytest.raises(ST.Refused):
            M.read_ids()
        FM.same((ctx.read_color(), ctx.read_depth(), None), want, f"{order}: the images stay")
        ctx.draw(b.tf["aff"], METAL | IDS); want = M.frame(METAL | IDS, b.tf["aff"])
        n = b.i.size // 3
        counts, none = ctx.count_ids(ST.COUNT_PER_PRIMITIVE, None, n)
        wc, wn = M.count(ST.COUNT_PER_PRIMITIVE, (0, 0, w, h), n, B.list_ids_to_items)
        assert none == wn and np.array_equal(counts, wc) and int(counts.sum()) + none == w * h and (counts > 0).sum() > 100
        FM.same((None, None, ctx.read_ids()), (None, None, want[2]), f"{order}: the next ID frame")
