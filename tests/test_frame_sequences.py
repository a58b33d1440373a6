"""Frame sequences that mix every frame flag on ONE context, and an all-pairs set of single frames (include/swr.h).

(a) `sequence(seed, steps)` is a pure-Python, seeded generator of legal C-ABI calls: draws, draw lists and one-shot renders with
    flags from the whole space of tests/frame_model.py, .vertices and .line frames between them, un-waited bursts of 2-9 frames
    with different flags, every frame presented into its own page-locked image, SWR_FLAG_LOAD chains, uploads of scenes of different
    and of equal sizes, target and material changes, a depth-clip frame that overflows the fan capacity in the middle of it all, a
    scene with depths <= 0 drawn early.  `play` makes the calls and compares every image the host gets to see, bit for bit, with
    frame_model.expect — a load frame's starting image is the model's own previous image, never a read-back.
(b) tests/test_frame_model.py asserts, without a GPU, what the sequences of SEEDS cover.
(c) `covering_rows`: a pairwise covering array over the same factors, each row ONE clear-or-load frame on a fresh context.

Like tests/test_gpu_stress.py::test_random_call_sequences (which stays as it is), whose flags end at DEPTH_TEST | NO_COLOR.
SWR_SEQUENCE_SEEDS=N adds N more sequences (seeds 100..) per scheduler: a soak.

(d) BLEND_SEEDS run the generator with `blend` switched on: SWR_FLAG_BLEND frames (draws, draw lists, one-shot renders) with
    swr_blend_set changes between them, inside the same bursts and load chains, and resolved reads (swr_read_*_resolved,
    swr_render_resolved) wherever a read is legal.  Switched off, the generator draws no random number it did not draw before:
    the sequences of SEEDS are the ones they always were (tests/test_frame_model.py holds their digest).
(e) `test_all_pairs_blend_frame`: frame_model.blend_covering_array, each row ONE blend frame on a fresh context, read back plainly
    and through k_resolve."""
import dataclasses
import functools
import os
import random
import time

import numpy as np
import pytest

import frame_model as FM
import kernel_matrix as K
import test_depth_clip as DC
import test_perspective as TP
import resolve_model as RM
from frame_model import BLEND, CB, CCW, CF, CLIP, DT, IDS, LOAD, METAL, NC, PERSP, REAL_LINES  # noqa: F401

pytestmark = pytest.mark.gpu

SEEDS = (21, 22, 23)
BLEND_SEEDS = (31, 32, 33)  # sequence(seed, blend=True)
STEPS = 70
SIZES = ((320, 192), (256, 160), (192, 96))
SCENES = {"small": 300, "big": 1300, "zero": 300, "straddle": 1300}      # triangles: big >= 4 x small, zero == small, straddle == big
# swr_debug_set hooks of a sequence, set on the fresh context (include/swr.h "Test hooks")
HOOK_SETS = ((),
             ((K.DEBUG_BIN_MODE, K.BIN_MODE_EXACT), (K.DEBUG_DEPTH_KEYS32, 0)),
             ((K.DEBUG_BIN_MODE, K.BIN_MODE_ATOMIC), (K.DEBUG_RASTER_SORT, 2)),
             ((K.DEBUG_RASTER_SORT, 0),))
MODEL_BUDGET = 16000        # triangles a sequence may send through the NumPy perspective model (about 0.2 - 1 s per 1 500)
# The blend model draws every primitive alone with the oracle, twice under the CPU rules' z-test (one colour and one depth frame):
# 0.25 - 0.3 ms a draw at 320x192 and 0.15 ms at 192x96 on the machine DESIGN.md §17 was measured on.  BLEND_BUDGET is in draws at
# 320x192 (about 4 s there): each distinct (scene, size, list, transform, rules, cull, clip) is paid once, whatever mode, opacity and
# load bit it is drawn with.  With it a sequence of BLEND_SEEDS spends no more time in the model than twice a sequence of SEEDS.
BLEND_BUDGET = 14000
BLEND_AREA = tuple(w * h / (320 * 192) for w, h in ((320, 192), (256, 160), (192, 96)))
OPACITIES = (0, 1, 128, 254, 255)
IMAGES = 10                 # page-locked image pairs per target size: a burst presents at most 9 frames, one more for its head
FIRST_FAN_CAPACITY = 1024   # swr_api.hip prepare_clip: a frame of n triangles has n + 2 * max(1024, n / 64) slots at first


def hooks_of(seed):
    return HOOK_SETS[seed % len(HOOK_SETS)]


# ---- the generator (no NumPy, no GPU) ------------------------------------------------------------------------------------------------
@dataclasses.dataclass(eq=False)
class Frame:
    n: int                  # order number in the sequence
    scene: str
    size: int               # index into SIZES
    shader: int             # the context's material when the frame is drawn
    kind: str               # "tri" | "points" | "lines"
    flags: int
    via: str                # "draw" | "list" | "render"
    tf: str                 # "aff" | "per"
    prev: object = None     # what a SWR_FLAG_LOAD frame is drawn over: a Frame, ("write", seed), or None (the cleared image)
    scene_id: int = 0       # (render)
    blend: object = None    # (mode, opacity) of the context when a SWR_FLAG_BLEND frame is drawn
    resolve: object = None  # (render) (S, depth filter): swr_render_resolved into SIZES[size] / S

    def row(self):
        return FM.row_of(self.flags, self.shader, self.via == "list", self.tf == "per")

    def needs_model(self):
        return self.kind == "tri" and bool(self.flags & PERSP) and not self.flags & NC and self.tf == "per"


BLOCKING = ("wait", "read", "read_resolved", "sync", "upload", "target", "write", "render", "hooks", "timing", "pipeline")


def sequence(seed, steps=STEPS, blend=False):
    """The operations of one sequence:
    ("hooks", pairs) ("upload", scene) ("target", size) ("shading", shader) ("write", seed) ("frame", Frame) ("render", Frame)
    ("present", image) ("wait",) ("read",) ("sync",) ("timing", level) ("pipeline", on);
    with blend: ("blend", mode, opacity) ("read_resolved", S, depth filter, "color" | "depth" | "both")."""
    rng = random.Random(seed)
    ops = [("hooks", hooks_of(seed))]
    st = dict(scene=None, size=None, shader=0, cur=None, last=None, shown=False, pending=0, count=0, budget=MODEL_BUDGET, paid=set(),
              blend=(FM.OVER, 255), bbudget=BLEND_BUDGET, bpaid=set())

    def blend_set(mode, opacity):
        if (mode, opacity) != st["blend"]:
            ops.append(("blend", mode, opacity))             # context state, like the material: no frame is completed by it
            st["blend"] = (mode, opacity)

    def read_resolved(S=None, filt=None, which=None, then_read=None):
        """A resolved read of the last frame (it completes everything, as a read does); about every second one is followed by a
        plain read, which must still see the full-size image."""
        f = st["last"]
        if f is None:
            return
        S = S or rng.choice((2, 4))
        filt = rng.choice((RM.SAMPLE0, RM.MIN)) if filt is None else filt
        which = which or rng.choice(("color", "depth", "both"))
        if f.flags & NC:
            which = "depth"                                  # (the resolved colour is as unspecified as swr_read_color's)
        ops.append(("read_resolved", S, filt, which))
        if rng.random() < 0.5 if then_read is None else then_read:
            ops.append(("read",))
        st["pending"] = 0
        ops.append(("wait",))

    def upload(scene):
        wait()
        ops.append(("upload", scene))
        st.update(scene=scene, last=None)
        if st["shader"]:                                     # (a new scene discards the vertex attributes)
            ops.append(("shading", st["shader"]))

    def target(size):
        wait()
        ops.append(("target", size))
        st.update(size=size, cur=None, last=None)

    def shading(shader):
        if shader != st["shader"]:
            ops.append(("shading", shader))
            st["shader"] = shader

    def wait():
        if st["pending"]:
            ops.append(("wait",))
            st["pending"] = 0

    def present():
        if st["last"] is not None and not st["shown"] and st["pending"] < IMAGES:
            ops.append(("present", st["pending"]))
            st["pending"] += 1
            st["shown"] = True

    def frame(kind="tri", clip_ok=True, force=None, via=None, blended=None, resolve=None):
        """One frame with random factors (force: factor values that are given).  blended: True / False, or None: by chance (only
        with `blend`, and never against a forced factor a blend frame cannot have); "tail": whatever it costs the model."""
        row = {f: rng.choice(FM.FACTORS[f]) for f in FM.FACTORS}
        row.update(force or {})
        if blend and kind == "tri" and blended is None:
            blended = rng.random() < 0.3 and not any((force or {}).get(k) for k in ("no_color", "ids", "persp", "shader"))
        if not clip_ok:
            row["clip"] = 0
        if st["scene"] == "straddle" and not row["clip"]:
            # un-clipped under the perspective matrix its slivers (w <= 0 at one corner) all cross the same tiles: more entries than
            # a tile region of the first guess holds, and a frame inside a burst that overflows its bins is dropped
            row["transform"] = "affine"
        tf = "per" if row["transform"] == "perspective" else "aff"
        if blended and kind == "tri":
            # include/swr.h "Alpha blending", Combinations: the generator steers the row the way it steers `clip` above
            row.update(no_color=0, ids=0, persp=0, shader=0)
            assert FM.legal(dict(row, blend=1))
            draws = (SCENES[st["scene"]] * (3 if row["clip"] else 1) + (60 if row["list"] else 0)) * (2 if row["rules"] == "ztest" else 1)
            bcost = draws * BLEND_AREA[st["size"]]
            key = (st["scene"], st["size"], row["list"], tf, row["rules"], row["cull"], row["ccw"], row["clip"])
            if key in st["bpaid"]:
                pass
            elif bcost > st["bbudget"] and blended != "tail":
                blended = False
            else:
                st["bbudget"] -= bcost
                st["bpaid"].add(key)
        blended = bool(blended) and kind == "tri"
        if blended and rng.random() < 0.6:
            blend_set(rng.choice((FM.OVER, FM.ADD)), rng.choice(OPACITIES))
        flags = FM.flags_of(row) | (BLEND if blended else 0)
        cost = SCENES[st["scene"]] * (3 if row["clip"] else 1) * (2 if row["list"] else 1)
        if kind == "tri" and flags & PERSP and not flags & NC and tf == "per":
            # the NumPy model's share of the run stays bounded: each distinct frame it has to draw is paid for once
            key = (st["scene"], st["size"], row["list"], row["shader"], flags & (DT | METAL | CB | CF | CCW | CLIP))
            if key in st["paid"]:
                pass
            elif cost > st["budget"]:
                flags &= ~PERSP
            else:
                st["budget"] -= cost
                st["paid"].add(key)
        if kind == "tri":
            shading(row["shader"])
            how = via or ("list" if row["list"] else "draw")
        else:                                                # .vertices / .line: the triangle-only bits are accepted and ignored
            flags = (flags & (CB | CF | CCW | CLIP | PERSP)) | (REAL_LINES if kind == "lines" and rng.random() < 0.7 else 0)
            how = "draw"
        f = Frame(st["count"], st["scene"], st["size"], st["shader"], kind, flags, how, tf, st["cur"] if flags & LOAD else None)
        if blended:
            f.blend = st["blend"]
        st["count"] += 1
        if how == "render":
            f.scene_id = rng.choice((0, 40 + list(SCENES).index(f.scene)))
            f.resolve = resolve
            if flags & LOAD:
                f.prev = ("write", rng.randrange(1 << 16))
            wait()
            ops.append(("render", f))
            # swr_render leaves its own scene, target and material on the context: set ours again
            ops.append(("upload", f.scene))
            ops.append(("target", f.size))
            if st["shader"]:
                ops.append(("shading", st["shader"]))
            st.update(cur=None, last=None)
            return f
        ops.append(("frame", f))
        st.update(cur=f, last=f, shown=False)
        return f

    def burst(length, head=None, tail_clip=False, force=None):
        """`length` triangle frames with no wait between them, each presented into its own image (head: a .vertices / .line frame
        in front).  On the straddling scene only the last frame may clip: a fan overflow is repaired for the last frame of a burst,
        an earlier one would be reported as dropped (include/swr.h SWR_ERR_FRAME_DROPPED)."""
        wait()
        if head:
            frame(head)
            present()
        for k in range(length):
            last = k == length - 1
            straddle = st["scene"] == "straddle"
            frame(clip_ok=(not straddle) or (last and tail_clip), force=dict(force or {}, **({"clip": 1, "load": 0} if last and tail_clip else {})),
                  blended="tail" if blend and last and tail_clip else None)
            present()
        if blend and tail_clip and st["last"].blend is not None:
            # the overflowed blend frame is redrawn by the read below: with the state it was posted with (swr_context::last_blend),
            # not with the one set meanwhile, chosen here so that the two give different images whatever the first one is
            mode, opacity = st["last"].blend
            blend_set(FM.ADD if mode == FM.OVER else FM.OVER, 200 if opacity < 128 else 30)
        if tail_clip or rng.random() < 0.5:
            ops.append(("read",))
            st["pending"] = 0                                # (a read completes everything: the presented images are there too)
            ops.append(("wait",))
        else:
            wait()

    def mixed_burst():
        """Blend and other frames next to each other, in both orders, with no wait: a depth-only frame (32-bit keys), an ID frame
        and a shaded one among them, the blend state changed in between."""
        wait()
        straddle = st["scene"] == "straddle"
        plain = (dict(rules="ztest", no_color=1, ids=0, load=0), None, dict(ids=1, no_color=0), None, dict(shader=rng.choice((1, 2)), no_color=0),
                 None, dict(load=1))
        for k, force in enumerate(plain):
            if force is None:
                blend_set(rng.choice((FM.OVER, FM.ADD)), OPACITIES[(seed + k) % len(OPACITIES)])
                frame(clip_ok=not straddle, blended=True, force=dict(list=k // 2 % 2))
            else:
                frame(clip_ok=not straddle, blended=False, force=force)
            present()
        ops.append(("read",))
        st["pending"] = 0
        ops.append(("wait",))

    def blend_chains():
        """Blend load frames over a colour frame of the key kernels, a depth-only frame (the colour there is unspecified), a
        swr_target_write image and another blend frame: three in a row each, one geometry for the model."""
        straddle = st["scene"] == "straddle"
        fixed = dict(rules=rng.choice(FM.FACTORS["rules"]), cull="none", ccw=0, clip=0, list=0, transform="affine")
        for start in ("colour", "depth_only", "write", "blend"):
            wait()
            if start == "write":
                s = rng.randrange(1 << 16)
                ops.append(("write", s))
                st.update(cur=("write", s), last=None)
            elif start == "blend":
                frame(clip_ok=not straddle, blended=True, force=dict(fixed, load=0))
                present()
            else:
                frame(clip_ok=not straddle, blended=False, force=dict(load=0, **(dict(no_color=1, rules=rng.choice(("ztest", "metal")))
                                                                                  if start == "depth_only" else dict(no_color=0))))
                present()
            for k in range(3):
                blend_set(FM.OVER if k == 0 and start == "depth_only" else rng.choice((FM.OVER, FM.ADD)),
                          (255, 128, 0)[k] if start == "depth_only" else rng.choice(OPACITIES))
                frame(blended=True, force=dict(fixed, load=1))
                present()
            ops.append(("read",))
            st["pending"] = 0
            ops.append(("wait",))

    def resolve_tour():
        """Resolved reads where single-frame tests never issue them: on a small target first and on the largest one right after
        the change (the resolve buffers grow), after a blend frame, a .vertices / .line frame and a depth-only frame, and in
        front of a load frame and a plain read (the full-size images are not modified)."""
        straddle = st["scene"] == "straddle"
        target(2)
        frame(clip_ok=not straddle, blended=False, force=dict(load=0, no_color=0))
        read_resolved(4, RM.MIN, "both", then_read=False)
        target(0)
        frame(clip_ok=not straddle, blended=True, force=dict(load=0))
        read_resolved(2, RM.SAMPLE0, "color", then_read=True)
        frame(rng.choice(("points", "lines")))
        read_resolved(2, RM.MIN, "depth", then_read=False)
        frame(clip_ok=not straddle, blended=False, force=dict(no_color=1, rules="ztest", ids=0))
        read_resolved(4, RM.SAMPLE0, "depth", then_read=False)
        frame(clip_ok=not straddle, blended=False, force=dict(load=0, no_color=0))
        read_resolved(rng.choice((2, 4)), rng.choice((RM.SAMPLE0, RM.MIN)), "both", then_read=False)
        frame(clip_ok=not straddle, force=dict(load=1, no_color=0))
        ops.append(("read",))
        ops.append(("wait",))

    scripted = {2: mixed_burst, 6: blend_chains, 10: mixed_burst, 40: blend_chains, 46: mixed_burst} if blend else {}

    # a scene with depths <= 0 first (the sticky move of a scene's depth-only frames to the 64-bit keys), then the scene of its size
    upload("zero")
    target(0)
    frame(force=dict(rules="ztest", no_color=1, load=0, ids=0, clip=0, list=0, transform="affine"))
    ops.append(("read",))
    upload("small")
    burst(5, force=dict(rules="ztest", no_color=1, ids=0))
    if blend:
        resolve_tour()
    at_overflow = rng.randrange(steps // 4, steps // 2)
    for step in range(steps):
        if step == at_overflow:
            # more crossing triangles than the first fan capacity, behind frames of other kinds
            upload("straddle")
            if blend and seed % 3 != 1:                      # (the blend model draws every fan triangle alone: on the smallest target)
                target(2)
            burst(rng.randint(3, 6), tail_clip=True)
            continue
        if step in scripted:
            scripted[step]()
            continue
        if step in (steps // 6, 4 * steps // 6, 5 * steps // 6):      # (every size and every scene comes up in every sequence)
            fresh = [x for x in range(len(SIZES)) if ("target", x) not in ops]
            if fresh:
                target(fresh[0])
            fresh = [x for x in SCENES if ("upload", x) not in ops]
            if fresh:
                upload(fresh[0])
        op = rng.choice(["burst"] * 5 + ["persp"] * 2 + ["draw"] * 3 + ["points", "present", "read", "read", "wait", "sync", "upload", "upload", "target",
                                                       "timing", "pipeline", "chain", "chain", "render", "render"]
                        + (["resolved"] * 4 + ["rrender"] * 2 if blend else []))
        if op == "resolved":
            read_resolved()
        elif op == "rrender":
            frame(via="render", clip_ok=st["scene"] != "straddle", force=dict(load=0), resolve=(rng.choice((2, 4)), rng.choice((RM.SAMPLE0, RM.MIN))))
        elif op == "burst":
            burst(rng.randint(2, 9))
        elif op == "persp" and st["scene"] != "straddle":
            # neighbouring lanes with different perspective tables: draws and draw lists of one rule set in turn, two distinct
            # frames for the model however long the burst
            wait()
            fixed = dict(persp=1, no_color=0, transform="perspective", clip=0, load=0, cull="none", ccw=0,
                         rules=rng.choice(FM.FACTORS["rules"]), shader=rng.choice(FM.FACTORS["shader"]))
            for k in range(rng.randint(5, 9)):
                frame(force=dict(fixed, list=k % 2))
                present()
            wait()
        elif op == "points":
            burst(rng.randint(4, 8), head=rng.choice(("points", "lines")))
        elif op == "draw":
            kind = rng.choice(("tri",) * 8 + ("points", "lines"))
            frame(kind, clip_ok=st["scene"] != "straddle")
        elif op == "present":
            present()
        elif op == "read" and st["last"] is not None:
            ops.append(("read",))
            st["pending"] = 0
            ops.append(("wait",))
        elif op == "wait":
            wait()
        elif op == "sync":
            ops.append(("sync",))
        elif op == "upload":
            fresh = [x for x in SCENES if ("upload", x) not in ops]          # (every scene and size comes up)
            upload(rng.choice(fresh or list(SCENES)))
        elif op == "target":
            fresh = [x for x in range(len(SIZES)) if ("target", x) not in ops]
            target(rng.choice(fresh or list(range(len(SIZES)))))
        elif op == "timing":
            ops.append(("timing", rng.randrange(3)))
        elif op == "pipeline":
            ops.append(("pipeline", rng.randrange(2)))
        elif op == "render":
            frame(via="render", clip_ok=st["scene"] != "straddle")
        elif op == "chain":
            # a load chain over target_write's image, over a clear frame, or over a frame of another kind (depth-only, then colour)
            wait()
            start = rng.choice(("write", "clear", "depth_only"))
            straddle = st["scene"] == "straddle"
            if start == "write":
                s = rng.randrange(1 << 16)
                ops.append(("write", s))
                st.update(cur=("write", s), last=None)
            elif start == "clear":
                frame(clip_ok=not straddle, force=dict(load=0))
                present()
            else:
                frame(clip_ok=not straddle, force=dict(load=0, no_color=1, rules=rng.choice(("ztest", "metal"))))
                present()
            for k in range(rng.randint(2, 4)):
                frame(clip_ok=not straddle, force=dict(load=1, **({"no_color": 0} if start == "depth_only" and k == 0 else {})))
                present()
            ops.append(("read",))
            st["pending"] = 0
            ops.append(("wait",))
    wait()
    return ops


def runs(ops):
    """The un-waited runs of a sequence: [[(Frame, checked)]] — frames with nothing between them that completes earlier frames
    (presents and material changes do not).  checked: the frame's image is compared (presented, or read back)."""
    out, cur = [], []
    for k, op in enumerate(ops):
        if op[0] == "frame":
            nxt = next((o for o in ops[k + 1:] if o[0] not in ("shading", "blend")), ("end",))
            cur.append((op[1], nxt[0] in ("present", "read", "read_resolved")))
        elif op[0] in BLOCKING and cur:
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def checked_frames(ops):
    """Every triangle frame whose image is compared (one-shot renders included)."""
    return [f for run in runs(ops) for f, chk in run if chk and f.kind == "tri"] + [op[1] for op in ops if op[0] == "render"]


# ---- the scenes, matrices and materials behind the names -----------------------------------------------------------------------------
def affine(angle=0.07, sx=0.36, sy=0.5, sz=0.22, tx=0.02, ty=-0.03, tz=-0.15):
    """Eye space (x in +-2.5, y in +-1.8, z in 1 .. 5) onto the screen with w = 1: z_ndc = sz * z + tz in (0, 1)."""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([c * sx, s * sx, 0, 0, -s * sy, c * sy, 0, 0, 0, 0, sz, 0, tx, ty, tz, 1], dtype=np.float32)


def straddling(n, seed):
    """n slivers, each with one corner in front of the eye, one behind the near plane and one beyond the far plane (under both
    transforms): a five-sided polygon, three fan triangles each."""
    rng = np.random.default_rng(seed)
    cen = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.4, 1.4, n)], axis=1)
    xyz = np.empty((n, 3, 3), dtype=np.float32)
    xyz[:, :, 0:2] = cen[:, None, :] + rng.uniform(-0.08, 0.08, (n, 3, 2))
    xyz[:, 0, 2] = rng.uniform(1.0, 3.0, n)
    xyz[:, 1, 2] = rng.uniform(-0.5, 0.2, n)
    xyz[:, 2, 2] = rng.uniform(7.0, 9.0, n)
    v = np.zeros((3 * n, 8), dtype=np.float32)
    v[:, 0:3] = xyz.reshape(-1, 3)
    v[:, 4:7] = rng.uniform(0, 1, (3 * n, 3))
    return v, np.arange(3 * n, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def world():
    """name -> (vertices, indices, {shader: Shading or None}); the matrices."""
    import swr_amd
    scenes = {}
    for k, (name, n) in enumerate(SCENES.items()):
        v, i = straddling(n, 0x57A + k) if name == "straddle" else TP.soup(n, 0x5E0 + k, r=0.15)
        if name == "zero":
            v[::7, 2] = np.float32(0.4)                      # z_ndc = 0.22 * 0.4 - 0.15 < 0 under the affine matrix
            v[::21, 2] = np.float32(0.15 / 0.22)             # (and a few close to zero)
        sh = {0: None}
        for shader in (1, 2):
            sh[shader] = swr_amd.scenes.random_shading(v.shape[0], 0x5AD + k, shader, shininess_log2=3)
        scenes[name] = (v, i, sh)
    per = TP.perspective()
    per2 = np.array(per, copy=True)
    per2[12] = np.float32(0.3)
    mats = {"aff": affine(), "aff2": affine(-0.1, 0.3, 0.42, 0.2, -0.1, 0.05, -0.1), "per": per, "per2": per2}
    return scenes, mats


def items_of(scene, tf):
    """The draw list of a scene: two ranges that split it and an instance of its first triangles; under "per" one item is affine."""
    scenes, mats = world()
    n = scenes[scene][1].size
    h = n // 2 // 3 * 3
    a, b, c = ("aff", "aff2", "aff") if tf == "aff" else ("per", "aff", "per2")
    return [(0, h, mats[a]), (h, n - h, mats[b]), (0, 3 * 60, K.mirrored(mats[c]) if tf == "aff" else mats[c])]


def tile_load(oracle, s):
    """The most (triangle, tile) pairs any 64 x 32 tile of the frame gets, counted by bounding boxes (an upper bound of what
    binning puts there): a frame inside an un-waited burst must stay below the first guess of a tile region, min(triangles, 1024)
    (swr_api.hip size_bins), or the library reports it as dropped."""
    (v, t, m, _), _, _ = FM._geometry(s)
    sx, sy, _ = oracle.project(v, m, s.width, s.height)
    x, y = sx[t].astype(np.float64), sy[t].astype(np.float64)
    ok = np.isfinite(x).all(axis=1) & np.isfinite(y).all(axis=1)
    x, y = x[ok], y[ok]
    tx, ty = (s.width + K.TILE_W - 1) // K.TILE_W, (s.height + K.TILE_H - 1) // K.TILE_H
    x0 = np.clip(np.floor(x.min(axis=1) / K.TILE_W), 0, tx).astype(int)
    x1 = np.clip(np.floor(x.max(axis=1) / K.TILE_W) + 1, 0, tx).astype(int)
    y0 = np.clip(np.floor(y.min(axis=1) / K.TILE_H), 0, ty).astype(int)
    y1 = np.clip(np.floor(y.max(axis=1) / K.TILE_H) + 1, 0, ty).astype(int)
    load = np.zeros((ty + 1, tx + 1), dtype=np.int64)
    for a, b, c, d in zip(x0, x1, y0, y1):
        load[c:d, a:b] += 1
    return int(load.max()), int(ok.sum())


def spec_of(f):
    scenes, mats = world()
    v, i, sh = scenes[f.scene]
    w, h = SIZES[f.size]
    shader = 0 if f.flags & NC else f.shader
    return FM.FrameSpec(v, i, w, h, f.flags & ~BLEND, mats[f.tf], items_of(f.scene, f.tf) if f.via == "list" else None, sh[shader],
                        key=(f.scene, f.size, f.via == "list", f.tf, shader), blend=f.blend if f.flags & BLEND else None)


_CLEAR = {}         # frame_model's clear frames, shared by every run of the module: a sequence is the same under every scheduler


def image_of(oracle, f, memo):
    """(colour or None, depth, ids or None): the model's image of a frame of a sequence."""
    if isinstance(f, tuple):
        w, h = f[2]
        return (*TP.start_images(f[1], w, h), None)
    if f.n not in memo:
        scenes, mats = world()
        w, h = SIZES[f.size]
        if f.kind == "tri":
            start = None
            if f.flags & LOAD and f.prev is not None:
                prev = (*f.prev, (w, h)) if isinstance(f.prev, tuple) else f.prev
                start = image_of(oracle, prev, memo)[:2]
            memo[f.n] = FM.expect(oracle, spec_of(f), start, _CLEAR)
        else:
            v, i, _ = scenes[f.scene]
            c, d, _, code = oracle.render(v, i, mats[f.tf], w, h, f.flags & REAL_LINES, primitive_type=2 if f.kind == "points" else 1)
            assert code == 0
            memo[f.n] = (c, d, None)
    return memo[f.n]


# ---- the player -----------------------------------------------------------------------------------------------------------------------
def play(swr, oracle, ops, bands, stats=None):
    scenes, mats = world()
    pool, memo = {}, {}
    stats = {} if stats is None else stats

    def images(size):
        if size not in pool:
            w, h = SIZES[size]
            pool[size] = [(swr.HostImage((h, w, 4), np.uint8), swr.HostImage((h, w), np.float32)) for _ in range(IMAGES)]
        return pool[size]

    def check(got, f, what):
        t0 = time.perf_counter()
        want = image_of(oracle, f, memo)
        stats["model_s"] = stats.get("model_s", 0.0) + time.perf_counter() - t0
        FM.same(got, want, f"{what}: frame {f.n} ({f.kind} {f.via} {f.tf} on {f.scene} {SIZES[f.size]}, shader {f.shader}, "
                           f"flags {f.flags:#x})")
        stats["checked"] = stats.get("checked", 0) + 1

    def check_resolved(got, f, S, filt, what):
        t0 = time.perf_counter()
        want = FM.resolved(image_of(oracle, f, memo), S, filt)
        stats["model_s"] = stats.get("model_s", 0.0) + time.perf_counter() - t0
        FM.same(got, want, f"{what}: frame {f.n} resolved by {S}, filter {filt} ({f.kind} {f.via} {f.tf} on {f.scene} {SIZES[f.size]}, "
                           f"shader {f.shader}, flags {f.flags:#x}, blend {f.blend})")
        stats["checked"] = stats.get("checked", 0) + 1

    try:
        with swr.Context(0, device_count=bands) as ctx:
            scene = size = None
            last, pending = None, []
            for k, op in enumerate(ops):
                what = f"op {k} {op[0]}"
                if op[0] == "hooks":
                    for key, value in op[1]:
                        ctx.debug_set(key, value)
                elif op[0] == "upload":
                    scene = op[1]
                    ctx.scene_upload(*scenes[scene][:2])
                    last = None
                elif op[0] == "target":
                    size = op[1]
                    ctx.target_set(*SIZES[size])
                    last = None
                elif op[0] == "shading":
                    ctx.shading_set(scenes[scene][2][op[1]])
                elif op[0] == "blend":
                    ctx.blend_set(op[1], op[2])
                elif op[0] == "write":
                    ctx.target_write(*TP.start_images(op[1], *SIZES[size]))
                    last = None
                elif op[0] == "frame":
                    f = op[1]
                    assert (f.scene, f.size) == (scene, size)
                    if f.via == "list":
                        ctx.draw_list(items_of(f.scene, f.tf), f.flags)
                    else:
                        ctx.draw(mats[f.tf], f.flags, {"tri": 0, "lines": 1, "points": 2}[f.kind])
                    last = f
                elif op[0] == "render":
                    f = op[1]
                    v, i, sh = scenes[f.scene]
                    w, h = SIZES[f.size]
                    if f.resolve is not None:
                        # swr_render_resolved: the destination is SIZES[size] / S, the frame (and its IDs) SIZES[size]
                        S, filt = f.resolve
                        c, d = ctx.render_resolved(v, i, mats[f.tf], w // S, h // S, f.flags, shading=sh[f.shader], scene_id=f.scene_id,
                                                   factor=S, depth_filter=filt)
                        check_resolved((c, d, None), f, S, filt, what)
                        if f.flags & IDS:
                            FM.same((None, None, ctx.read_ids()), image_of(oracle, f, memo), what + ": IDs at sample resolution")
                        last = None
                        continue
                    start = TP.start_images(f.prev[1], w, h) if f.flags & LOAD else (None, None)
                    c, d = ctx.render(v, i, mats[f.tf], w, h, f.flags, shading=sh[f.shader], scene_id=f.scene_id,
                                      color=None if f.flags & NC or start[0] is None else start[0].copy(),
                                      depth=None if start[1] is None else start[1].copy())
                    check((None if f.flags & NC else c, d, ctx.read_ids() if f.flags & IDS else None), f, what)
                    last = None
                elif op[0] == "present":
                    ci, di = images(size)[op[1]]
                    ctx.present(ci, di)
                    pending.append((op[1], size, last))
                elif op[0] == "wait":
                    ctx.present_wait()
                    for slot, sz, f in pending:
                        ci, di = images(sz)[slot]
                        check((None if f.flags & NC else ci.array.copy(), di.array.copy(), None), f, what + ": presented")
                    pending = []
                elif op[0] == "read":
                    f = last
                    ctx.sync()
                    check((None if f.flags & NC else ctx.read_color(), ctx.read_depth(),
                           ctx.read_ids() if f.flags & IDS and f.kind == "tri" else None), f, what)
                elif op[0] == "read_resolved":
                    # (no swr_sync in front: the call completes everything itself)
                    f, (S, filt, which) = last, op[1:]
                    gc = ctx.read_color_resolved(S) if which in ("color", "both") and not f.flags & NC else None
                    gd = ctx.read_depth_resolved(S, filt) if which in ("depth", "both") else None
                    check_resolved((gc, gd, None), f, S, filt, what)
                elif op[0] == "sync":
                    ctx.sync()
                elif op[0] == "timing":
                    ctx.timing_enable(op[1])
                elif op[0] == "pipeline":
                    ctx.pipeline_enable(bool(op[1]))
            ctx.present_wait()
            assert not pending
    finally:
        for lst in pool.values():
            for a, b in lst:
                a.free(); b.free()
    return stats


# SWR_SEQUENCE_SEEDS=N adds N more sequences (seeds 100..) per scheduler and band count
_EXTRA = [100 + k for k in range(int(os.environ.get("SWR_SEQUENCE_SEEDS", "0")))]


@pytest.mark.parametrize("env", [{}, {"SWR_LANES": "0"}], ids=["lanes", "SWR_LANES=0"])
@pytest.mark.parametrize("bands", [1, 3])
@pytest.mark.parametrize("seed", list(SEEDS) + list(BLEND_SEEDS) + _EXTRA)
def test_mixed_sequences(swr, oracle, monkeypatch, seed, bands, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t0 = time.perf_counter()
    stats = play(swr, oracle, sequence(seed, blend=seed in BLEND_SEEDS), bands)
    print(f"seed {seed} bands {bands} {env}: {stats['checked']} images checked, {time.perf_counter() - t0:.1f} s "
          f"({stats['model_s']:.1f} s in the model)")


# ---- (c) all-pairs single frames ----------------------------------------------------------------------------------------------------
def covering_rows():
    return FM.covering_array()


@functools.lru_cache(maxsize=None)
def pair_scene(target, clip):
    """The visible set of the kernel matrix for rows without depth clipping; a straddling soup for rows with it."""
    import swr_amd
    w, h = K.TARGETS[target]
    if clip:
        v, i = DC.straddling_soup(500, 0xA77, z_lo=-0.5, z_hi=7.0, r=0.5)
    else:
        vs = K.visible_set(w, h)
        v, i = vs.vertices, vs.indices
    sh = {0: None}
    for shader in (1, 2):
        sh[shader] = swr_amd.scenes.random_shading(v.shape[0], 0xA5, shader, shininess_log2=3)
    return v, i, sh


def pair_spec(row, target):
    w, h = K.TARGETS[target]
    v, i, sh = pair_scene(target, row["clip"])
    if row["clip"]:
        m = DC.metal_perspective(aspect=w / h) if row["transform"] == "perspective" else affine(sz=0.2, tz=-0.1)
        m2 = affine(-0.1, 0.3, 0.42, 0.2, -0.1, 0.05, -0.1)
    else:
        m = K.perspective_matrix() if row["transform"] == "perspective" else K.affine_matrix()
        m2 = K.affine_matrix(-0.05, 1.02, -0.02, 0.01)
    items = None
    if row["list"]:
        n = i.size // 3
        items = [(0, 3 * (n // 2), m), (3 * (n // 2), 3 * (n - n // 2), m2), (3 * (n // 5), 3 * 100, K.mirrored(m))]
    return FM.FrameSpec(v, i, w, h, FM.flags_of(row), m, items, sh[row["shader"]])


@pytest.mark.parametrize("target", ["small", "large"])
@pytest.mark.parametrize("k", range(len(FM.covering_array())))
def test_all_pairs_single_frame(swr, oracle, k, target):
    row = covering_rows()[k]
    s = pair_spec(row, target)
    start = K.special_start(s.width, s.height, 0x900 + k) if row["load"] else None
    want = FM.expect(oracle, s, start)
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        if s.shading is not None:
            ctx.shading_set(s.shading)
        ctx.target_set(s.width, s.height)
        if start is not None:
            ctx.target_write(*start)
        if s.items is not None:
            ctx.draw_list(s.items, s.flags)
        else:
            ctx.draw(s.transform, s.flags)
        ctx.sync()
        got = (None if s.flags & NC else ctx.read_color(), ctx.read_depth(), ctx.read_ids() if s.flags & IDS else None)
    FM.same(got, want, f"row {k} on {target}: {row}")


# ---- (e) all-pairs single blend frames ------------------------------------------------------------------------------------------------
def blend_pair_spec(row, target):
    """pair_spec's scenes and matrices for a row of frame_model.BLEND_FACTORS."""
    flags, state = FM.blend_flags_of(row)
    s = pair_spec(dict(row, no_color=0, ids=0, persp=0, shader=0), target)
    return dataclasses.replace(s, flags=flags, blend=state, key=("pairs", target, row["clip"], row["list"], row["transform"]))


@pytest.mark.parametrize("k", range(len(FM.blend_covering_array())))
def test_all_pairs_blend_frame(swr, oracle, k, target="small"):
    """One blend frame per row, on the small target only (the per-primitive model would take minutes on the large one), compared
    through a plain read and through swr_read_*_resolved with S = 2 (MIN for odd k, SAMPLE0 for even k)."""
    row = FM.blend_covering_array()[k]
    s = blend_pair_spec(row, target)
    start = K.special_start(s.width, s.height, 0xB00 + k) if row["load"] else None
    want = FM.expect(oracle, s, start, _CLEAR)
    filt = RM.MIN if k % 2 else RM.SAMPLE0
    with swr.Context(0) as ctx:
        ctx.scene_upload(s.vertices, s.indices)
        ctx.target_set(s.width, s.height)
        if start is not None:
            ctx.target_write(*start)
        ctx.blend_set(*s.blend)
        if s.items is not None:
            ctx.draw_list(s.items, s.flags | BLEND)
        else:
            ctx.draw(s.transform, s.flags | BLEND)
        ctx.sync()
        got = (ctx.read_color(), ctx.read_depth(), None)
        res = (ctx.read_color_resolved(2), ctx.read_depth_resolved(2, filt), None)
    FM.same(got, want, f"blend row {k} on {target}: {row}")
    FM.same(res, FM.resolved(want, 2, filt), f"blend row {k} on {target}, resolved by 2: {row}")
