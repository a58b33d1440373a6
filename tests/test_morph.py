"""Morph targets on the GPU (include/swr.h "Morph targets"): every frame after swr_morph_set is bit for bit the frame
of the model-morphed (then model-posed) vertices (tests/morph_model.py, tests/skin_model.py) — under the oracle, and on a second
context that uploaded them.  The scene is the torus of tests/morph_model.py (768 vertices, 1536 triangles, 24 groups, five targets)
on 320 x 192; tests/test_morph_model.py holds the floors that keep these cases from being vacuous.  No tolerance anywhere."""
import contextlib
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import kernel_matrix as K
import morph_model as MM
import skin_model as SM

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_morph.hip")
DT, NC, METAL, IDS = K.DT, K.NC, K.METAL, K.IDS
REAL_LINES, DEPTH_CLIP, PERSPECTIVE, BLEND = 8, 1024, 2048, 4096
LINE, VERTICES = 1, 2           # SWR_PRIMITIVE_*
W, H = MM.W, MM.H
IDENT = K.IDENT
BAD_ARG, HIP, UNSUPPORTED, NO_SCENE = -1, -4, -5, -6
RULE_SETS = {"ztest": DT | IDS, "painter": IDS, "metal": METAL | IDS, "depth_only": DT | NC}
WA, WB = MM.WEIGHTS_A, MM.WEIGHTS_B


@dataclasses.dataclass
class Case:
    v: np.ndarray
    i: np.ndarray
    d: np.ndarray           # (5, nv, 3) position deltas
    nd: np.ndarray          # (5, nv, 3) normal deltas
    vA: np.ndarray
    vB: np.ndarray
    joint: np.ndarray
    weight: np.ndarray
    P: np.ndarray           # two poses
    Q: np.ndarray


@pytest.fixture(scope="module")
def case(swr):
    v, i = MM.torus(swr.scenes)
    d = MM.targets(swr.scenes, v)
    j, w = SM.bend_skin(v)
    return Case(v, i, d, MM.normal_targets(v.shape[0]), MM.morph_vertices(v, d, WA), MM.morph_vertices(v, d, WB), j, w,
                SM.bend_pose(), SM.bend_pose(-0.3, 0.8, -0.15))


@contextlib.contextmanager
def resident(swr, v, i, targets=None, weights=None, **kw):
    with swr.Context(0, **kw) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        if targets is not None:
            ctx.scene_morph(*targets) if isinstance(targets, tuple) else ctx.scene_morph(targets)
        if weights is not None:
            ctx.morph_set(weights)
        yield ctx


def grab(ctx, flags, prim=0, m=IDENT, items=None):
    """One frame, read back: (depth, colour or None, IDs or None)."""
    if items is not None:
        ctx.draw_list(items, flags)
    else:
        ctx.draw(m, flags, prim)
    ctx.sync()
    return (ctx.read_depth(), None if flags & NC else ctx.read_color(), ctx.read_ids() if flags & IDS else None)


def same(a, b, what):
    for x, y, name in zip(a, b, ("depth", "colour", "IDs")):
        assert (x is None) == (y is None), what
        if x is not None:
            bad = np.nonzero(x.view(np.uint32).reshape(H, W) != y.view(np.uint32).reshape(H, W))
            assert bad[0].size == 0, f"{what}: {bad[0].size} {name} pixels differ, first at (y,x)=({bad[0][0]},{bad[1][0]})"


def differ(a, b):
    """Pixels in which two frames differ (depth bits, or colour)."""
    d = a[0].view(np.uint32) != b[0].view(np.uint32)
    if a[1] is not None:
        d = d | (a[1] != b[1]).any(axis=-1)
    return int(d.sum())


def against(want, got, flags, what):
    """A frame against K.Expected."""
    d, c, ids = got
    assert d.tobytes() == want.depth.tobytes(), f"{what}: depth"
    if not flags & NC:
        assert np.array_equal(c, want.color), f"{what}: colour"
    if flags & IDS:
        assert (ids[want.ids == K.LIVE] != K.NONE).all(), what
        assert not ((ids != want.ids) & (want.ids >= 0)).any(), f"{what}: IDs"


# ---- 1: the morphed frame is the oracle's frame of the morphed vertices, and that of a context that uploaded them -------------------
@gpu
@pytest.mark.parametrize("rules", sorted(RULE_SETS))
def test_morphed_frames_match_the_oracle_and_an_uploaded_context(swr, oracle, case, rules):
    """z-test, painter's order, the Metal rules with IDs, and (depth_only) the 32-bit depth kernel."""
    flags = RULE_SETS[rules]
    want = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, flags)
    with resident(swr, case.v, case.i, case.d) as ctx, resident(swr, case.vA, case.i) as ref:
        base = grab(ctx, flags)
        ctx.morph_set(WA)
        got = grab(ctx, flags)
        against(want, got, flags, rules)
        same(got, grab(ref, flags), rules)
        assert differ(base, got) > 10000, "the morph moves the image"
        if flags & IDS:
            hit = got[2] != K.NONE
            assert hit.sum() > 10000 and np.unique(got[2][hit]).size > 300


# ---- 2: sequences ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_weights_a_b_zero_and_null(swr, oracle, case):
    wa = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    wb = K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT)
    with resident(swr, case.v, case.i, case.d) as ctx:
        never = grab(ctx, DT)
        ctx.morph_set(WA)
        a = grab(ctx, DT)
        against(wa, a, DT, "weights A")
        ctx.morph_set(WB)
        b = grab(ctx, DT)
        against(wb, b, DT, "weights B")
        assert differ(a, b) > 5000
        ctx.morph_set(np.array([0.0, -0.0, 0.0, -0.0, 0.0], dtype=np.float32))
        same(grab(ctx, DT), never, "all weights zero")
        ctx.morph_set(WA)
        ctx.morph_set(None)
        same(grab(ctx, DT), never, "NULL weights")
        ctx.morph_set(None)
        same(grab(ctx, DT), never, "NULL weights twice")


@gpu
def test_a_zero_weight_skips_the_non_finite_target_and_a_tiny_one_does_not(swr, oracle, case):
    want = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    with resident(swr, case.v, case.i, case.d) as ctx:
        for zero in (0.0, -0.0):
            w = WA.copy()
            w[MM.NONFINITE] = zero
            ctx.morph_set(w)
            against(want, grab(ctx, DT), DT, f"the non-finite target at {zero}")
        w = WA.copy()
        w[MM.NONFINITE] = 1e-30
        ctx.morph_set(w)
        poisoned = MM.morph_vertices(case.v, case.d, w)
        assert not np.isfinite(poisoned[:, 0:3]).any()
        got = grab(ctx, DT)
        against(K.expected_frame(oracle, poisoned, case.i, IDENT, W, H, DT), got, DT, "the non-finite target at 1e-30")
        assert not np.isfinite(got[0]).any(), "every triangle has a non-finite corner: nothing is drawn"
        ctx.morph_set(WA)
        against(want, grab(ctx, DT), DT, "weights A again")


# ---- 3: morph first, then skin --------------------------------------------------------------------------------------------------------
@gpu
def test_morph_with_skin_in_both_call_orders(swr, oracle, case):
    def want(w, pose):
        return K.expected_frame(oracle, MM.morph_then_skin(case.v, case.d, w, case.joint, case.weight, pose), case.i, IDENT, W, H, DT | IDS)

    skin_then_morph = SM.pose_vertices(case.v, case.joint, case.weight, case.P)
    skin_then_morph = MM.morph_vertices(skin_then_morph, case.d, WA)
    wrong = K.expected_frame(oracle, skin_then_morph, case.i, IDENT, W, H, DT | IDS)
    wAP = want(WA, case.P)
    assert (wrong.depth.view(np.uint32) != wAP.depth.view(np.uint32)).sum() > 3000, "the order of morph and skin shows in the frame"
    for order in ("morph, pose", "pose, morph"):
        with resident(swr, case.v, case.i, case.d) as ctx:
            ctx.scene_skin(case.joint, case.weight)
            for step in order.split(", "):
                {"morph": lambda: ctx.morph_set(WA), "pose": lambda: ctx.pose_set(case.P)}[step]()
            against(wAP, grab(ctx, DT | IDS), DT | IDS, order)
            ctx.pose_set(case.Q)
            against(want(WA, case.Q), grab(ctx, DT | IDS), DT | IDS, order + ", a new pose")
            ctx.morph_set(WB)
            against(want(WB, case.Q), grab(ctx, DT | IDS), DT | IDS, order + ", new weights")
            ctx.morph_set(None)
            posed = SM.pose_vertices(case.v, case.joint, case.weight, case.Q)
            against(K.expected_frame(oracle, posed, case.i, IDENT, W, H, DT | IDS), grab(ctx, DT | IDS), DT | IDS, order + ", the pose alone")
            ctx.morph_set(WB)
            ctx.pose_set(None)
            against(K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT | IDS), grab(ctx, DT | IDS), DT | IDS, order + ", the morph alone")
    # targets given after the skin and the pose
    with resident(swr, case.v, case.i) as ctx:
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set(case.P)
        ctx.scene_morph(case.d)
        ctx.morph_set(WA)
        against(wAP, grab(ctx, DT | IDS), DT | IDS, "skin, pose, targets, weights")


@gpu
def test_new_targets_under_a_pose_and_removal(swr, oracle, case):
    posed = K.expected_frame(oracle, SM.pose_vertices(case.v, case.joint, case.weight, case.P), case.i, IDENT, W, H, DT)
    other = np.ascontiguousarray(case.d[[MM.LIFT, MM.SHEAR]])
    w2 = np.array([0.25, -1.0], dtype=np.float32)
    with resident(swr, case.v, case.i, case.d, WA) as ctx:
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set(case.P)
        ctx.scene_morph(other)
        against(posed, grab(ctx, DT), DT, "new targets: every weight 0, the pose kept")
        with pytest.raises(swr.SwrError):
            ctx.morph_set(WA)                   # two targets now
        ctx.morph_set(w2)
        v2 = MM.morph_then_skin(case.v, other, w2, case.joint, case.weight, case.P)
        against(K.expected_frame(oracle, v2, case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "the new targets")
        ctx.scene_morph(None)
        against(posed, grab(ctx, DT), DT, "the targets removed")
        with pytest.raises(swr.SwrError):
            ctx.morph_set(w2)
        ctx.pose_set(None)
        against(K.expected_frame(oracle, case.v, case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "the uploaded scene")


@gpu
def test_an_unwaited_frame_keeps_the_shape_it_was_posted_in(swr, oracle, case):
    wa = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    wb = K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT)
    hc, hd = swr.HostImage((H, W, 4), np.uint8), swr.HostImage((H, W), np.float32)
    try:
        with resident(swr, case.v, case.i, case.d, WA) as ctx:
            ctx.draw(IDENT, DT)
            ctx.present(hc, hd)
            ctx.morph_set(WB)
            ctx.draw(IDENT, DT)
            ctx.present_wait()
            against(wa, (hd.array, hc.array, None), DT, "the presented frame, weights A")
            against(wb, (ctx.read_depth(), ctx.read_color(), None), DT, "the next frame, weights B")
    finally:
        hc.free(); hd.free()


# ---- 4: three bands on one device: the group boxes follow the morph -----------------------------------------------------------------
@gpu
def test_three_bands_cull_with_the_morphed_boxes(swr, oracle, case):
    """The lift takes the torus out of the lowest band (tests/test_morph_model.py): with the upload's group boxes every band would cull
    by where the groups were."""
    def one(t, x):
        w = np.zeros(5, dtype=np.float32)
        w[t] = x
        return w

    with resident(swr, case.v, case.i, case.d, device_count=3) as ctx:
        assert [b[1:] for b in ctx.bands()] == [(0, 64), (64, 128), (128, 192)]
        never = grab(ctx, DT)
        for name, w in (("up", one(MM.LIFT, 1.0)), ("down", one(MM.LIFT, -1.0)), ("up and swollen", one(MM.LIFT, 1.0) + one(MM.SWELL, 1.0))):
            ctx.morph_set(w)
            want = K.expected_frame(oracle, MM.morph_vertices(case.v, case.d, w), case.i, IDENT, W, H, DT | IDS)
            assert (want.ids != K.NONE).sum() > 1000
            against(want, grab(ctx, DT | IDS), DT | IDS, name)
        ctx.morph_set(None)
        same(grab(ctx, DT), never, "all weights zero")


# ---- 5: a draw list over two ranges cuts the stream: the rebuilt stream is morphed again ------------------------------------------
@gpu
def test_a_draw_list_cuts_the_stream_and_new_weights_follow(swr, oracle, case):
    n1 = 3 * 500
    items = [(0, n1, K.affine_matrix(0.3, 0.6, -0.35, 0.1)), (n1, case.i.size - n1, K.affine_matrix(-0.2, 0.55, 0.4, -0.15))]
    with resident(swr, case.v, case.i, case.d, WA) as ctx:
        frames = []
        for name, morphed in (("weights A", case.vA), ("weights B", case.vB)):
            if morphed is case.vB:
                ctx.morph_set(WB)
            cv, ci = K.concat(morphed, case.i, items)
            want = K.expected_frame(oracle, cv, ci, IDENT, W, H, DT | IDS)
            assert np.unique(want.ids[want.ids != K.NONE] >= 500).size == 2, "both items are visible"
            frames.append(grab(ctx, DT | IDS, items=items))
            against(want, frames[-1], DT | IDS, name)
        assert differ(*frames) > 3000
        against(K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "a plain frame on the cut stream")


# ---- 6: attributes: the normals are morphed, in every order of the calls ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shader", [1, 2])
def test_phong_frames_with_morphed_normals(swr, oracle, case, shader):
    sh = swr.scenes.random_shading(case.v.shape[0], 0x51, shader)
    morphed_sh = dataclasses.replace(sh, attrs=MM.morph_attrs(sh.attrs, case.nd, WB))
    assert not np.array_equal(morphed_sh.attrs[:, 0:3], sh.attrs[:, 0:3]) and np.array_equal(morphed_sh.attrs[:, 3:], sh.attrs[:, 3:])
    wc, wd = K.oracle_clear(oracle, case.vB, case.i, IDENT, W, H, DT, shading=morphed_sh)
    uc, ud = K.oracle_clear(oracle, case.vB, case.i, IDENT, W, H, DT, shading=sh)
    assert (wc != uc).any(axis=-1).sum() > 3000, "morphed normals shade differently"
    M = swr.binding.Material.from_shading(sh)

    def check(ctx, c, d, what):
        gd, gc, _ = grab(ctx, DT)
        assert gd.tobytes() == d.tobytes() and np.array_equal(gc, c), what

    for order in ("attributes, targets, weights", "targets, attributes, weights", "targets, weights, attributes"):
        for nd, (c, d) in ((case.nd, (wc, wd)), (None, (uc, ud))):
            with resident(swr, case.v, case.i) as ctx:
                if sh.texture is not None:
                    ctx.texture_upload(sh.texture)
                ctx.material_set(M)
                for step in order.split(", "):
                    {"attributes": lambda: ctx.scene_attributes(sh.attrs), "targets": lambda: ctx.scene_morph(case.d, nd),
                     "weights": lambda: ctx.morph_set(WB)}[step]()
                check(ctx, c, d, order + (", normal deltas" if nd is not None else ", no normal deltas: the normals stay as uploaded"))
                if order.endswith("attributes") and nd is not None:
                    # zero weights restore the normals as well; and with a skin the pose reads the morphed normals
                    ctx.morph_set(None)
                    check(ctx, *K.oracle_clear(oracle, case.v, case.i, IDENT, W, H, DT, shading=sh), "zero weights with attributes")
                    ctx.morph_set(WB)
                    ctx.scene_skin(case.joint, case.weight)
                    ctx.pose_set(case.P)
                    both = dataclasses.replace(sh, attrs=SM.pose_attrs(morphed_sh.attrs, case.joint, case.weight, case.P))
                    vb = SM.pose_vertices(case.vB, case.joint, case.weight, case.P)
                    check(ctx, *K.oracle_clear(oracle, vb, case.i, IDENT, W, H, DT, shading=both), "morphed normals, posed")


# ---- 7: the other frame types and stream orders, against a context that uploaded the morphed vertices -----------------------------
@gpu
def test_points_and_real_lines_read_the_morphed_vertices(swr, case):
    with resident(swr, case.v, case.i, case.d) as ctx, resident(swr, case.vA, case.i) as ref:
        for name, flags, prim in (("vertices", DT, VERTICES), ("vertices painter", 0, VERTICES), ("lines", DT | REAL_LINES, LINE),
                                  ("lines painter", REAL_LINES, LINE)):
            base = grab(ctx, flags, prim)
            ctx.morph_set(WA)
            got = grab(ctx, flags, prim)
            same(got, grab(ref, flags, prim), name)
            assert differ(base, got) > 500, name
            ctx.morph_set(None)
            same(grab(ctx, flags, prim), base, name + ", all weights zero")
        # under a pose the chain's last array is the posed one
        ctx.scene_skin(case.joint, case.weight)
        ctx.morph_set(WA)
        ctx.pose_set(case.P)
        with resident(swr, MM.morph_then_skin(case.v, case.d, WA, case.joint, case.weight, case.P), case.i) as ref2:
            same(grab(ctx, DT, VERTICES), grab(ref2, DT, VERTICES), "vertices, morphed and posed")


@gpu
def test_clip_perspective_and_blend_frames(swr, case):
    m = swr.scenes.app_transform(1.0)
    with resident(swr, case.v, case.i, case.d, WA) as ctx, resident(swr, case.vA, case.i) as ref, resident(swr, case.v, case.i) as base:
        for name, flags in (("clip + perspective", DT | DEPTH_CLIP | PERSPECTIVE | IDS), ("clip", DEPTH_CLIP | IDS),
                            ("perspective, metal", METAL | PERSPECTIVE)):
            got = grab(ctx, flags, m=m)
            same(got, grab(ref, flags, m=m), name)
            assert differ(got, grab(base, flags, m=m)) > 3000, name
        for c in (ctx, ref):
            c.blend_set(swr.binding.BLEND_OVER, 160)
            c.draw(IDENT, DT)
        same(grab(ctx, BLEND | K.LOAD | DT, m=K.affine_matrix()), grab(ref, BLEND | K.LOAD | DT, m=K.affine_matrix()), "a blend frame over a frame")


@gpu
@pytest.mark.parametrize("order", [0, -1])
def test_stream_orders(swr, oracle, case, order):
    """SWR_DEBUG_STREAM_ORDER 0: the caller's order; -1: as for 2^24 primitives or more (slot == primitive, not reordered)."""
    want = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT | IDS)
    with swr.Context(0) as ctx:
        ctx.debug_set(swr.binding.DEBUG_STREAM_ORDER, order)
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        never = grab(ctx, DT | IDS)
        ctx.scene_morph(case.d)
        ctx.morph_set(WA)
        against(want, grab(ctx, DT | IDS), DT | IDS, f"order {order}")
        against(K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, IDS), grab(ctx, IDS), IDS, f"order {order}, painter")
        ctx.morph_set(None)
        same(grab(ctx, DT | IDS), never, "all weights zero")


# ---- 8: weights that crowd a few tiles are an ordinary overflow --------------------------------------------------------------------
@gpu
def test_weights_that_overflow_the_bins_are_repaired(swr, oracle):
    """Forced as tests/test_skin.py forces it with a pose: a fresh context, 20 000 triangles that one target collapses into a few tiles.
    The first read repairs the frame."""
    w, h = 1280, 720
    s = swr.scenes.random_soup(20000, w, h, 555, r_ndc=0.01, flags=DT, margin=1.0)
    v = s.vertices
    d = np.zeros((1, v.shape[0], 3), dtype=np.float32)
    d[0, :, 0] = v[:, 0] * np.float32(0.035 - 1.0) + np.float32(0.335)     # weight 1: x -> about 0.035 x + 0.335
    d[0, :, 1] = v[:, 1] * np.float32(0.03 - 1.0) + np.float32(0.13)
    morphed = MM.morph_vertices(v, d, [1.0])
    wc, wd = K.oracle_clear(oracle, morphed, s.indices, s.transform, w, h, DT)
    ys, xs = np.nonzero(np.isfinite(wd))
    assert 200 < ys.size < 64 * 32 * 4 and xs.max() - xs.min() < 128 and ys.max() - ys.min() < 64
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(v, s.indices)
        ctx.scene_morph(d)
        ctx.morph_set([1.0])
        ctx.draw(s.transform, DT)
        assert ctx.read_depth().tobytes() == wd.tobytes(), "overflowed last frame"
        assert np.array_equal(ctx.read_color(), wc)


# ---- 9: the shapes where the kernel itself can go wrong ------------------------------------------------------------------------------
def many_targets(nv, seed):
    """256 resident targets of small finite deltas, and weights for them."""
    rng = np.random.RandomState(seed)
    d = ((rng.random_sample((256, nv, 3)) - 0.5) * 0.02).astype(np.float32)
    w = ((rng.random_sample(256) - 0.5) * 2.0).astype(np.float32)
    w[w == 0] = 0.5
    return d, w


@gpu
@pytest.mark.parametrize("scene", ["one_triangle", "torus"])
def test_256_resident_targets_and_every_unroll_remainder(swr, case, scene):
    """Active counts 0, 1, 2, 3, an odd number beyond one unrolled batch, and all 256 — scattered over the 256 residents, the last
    one included — on 3 vertices (one lane of one wave) and on 768: against a context that uploaded the model's vertices, through a
    triangle frame with IDs and a .vertices frame (which reads the morphed array itself)."""
    if scene == "one_triangle":
        v = swr.scenes.pack_vertices(np.array([[-0.6, -0.5, 0.3], [0.7, -0.4, 0.5], [0.1, 0.8, 0.4]], dtype=np.float32),
                                     np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32))
        i = np.array([0, 1, 2], dtype=np.int64)
    else:
        v, i = case.v, case.i
    d, w_all = many_targets(v.shape[0], 0x256 + v.shape[0])
    with resident(swr, v, i, d) as ctx:
        base = grab(ctx, DT | IDS)
        seen = []
        for count in (0, 1, 2, 3, 7, 256):
            w = np.zeros(256, dtype=np.float32)
            pick = np.arange(256) if count == 256 else 255 - np.arange(count) * (256 // max(count, 1))     # (the last one included)
            assert np.unique(pick).size == count
            w[pick] = w_all[pick]
            ctx.morph_set(w)
            mv = MM.morph_vertices(v, d, w)
            with resident(swr, mv, i) as ref:
                got = grab(ctx, DT | IDS)
                same(got, grab(ref, DT | IDS), f"{count} of 256 active")
                same(grab(ctx, DT, VERTICES), grab(ref, DT, VERTICES), f"{count} of 256 active, .vertices")
            seen.append(got)
            if count:
                assert differ(base, got) > 0, count
            else:
                same(got, base, "none active")
        assert differ(seen[-1], seen[-2]) > 0


@gpu
def test_a_vertex_count_that_is_no_multiple_of_the_wave_or_the_block(swr, case):
    """773 vertices: three full blocks of 256 and a ragged wave of 5 lanes, whose vertices the last triangles use."""
    extra = swr.scenes.pack_vertices(np.array([[-0.9, -0.9, 0.2], [-0.6, -0.9, 0.2], [-0.9, -0.6, 0.2], [0.9, 0.9, 0.1], [0.6, 0.8, 0.1]], dtype=np.float32),
                                     np.full((5, 3), 0.5, dtype=np.float32))
    v = np.concatenate([case.v, extra])
    i = np.concatenate([case.i, np.array([768, 769, 770, 770, 771, 772], dtype=np.int64)])
    assert v.shape[0] == 773 and v.shape[0] % 64 != 0 and v.shape[0] % 256 != 0
    d = np.concatenate([case.d, np.zeros((5, 5, 3), dtype=np.float32)], axis=1)
    d[MM.SHEAR, 768:, 0] = 0.11                  # the ragged lanes move too
    d[MM.SWELL, 772, 1] = -0.3
    mv = MM.morph_vertices(v, d, WA)
    assert not np.array_equal(mv[768:, 0:3], v[768:, 0:3])
    with resident(swr, v, i, d, WA) as ctx, resident(swr, mv, i) as ref:
        same(grab(ctx, DT | IDS), grab(ref, DT | IDS), "773 vertices")
        same(grab(ctx, DT, VERTICES), grab(ref, DT, VERTICES), "773 vertices, .vertices")


# ---- 10: errors -----------------------------------------------------------------------------------------------------------------------
def code_of(swr, call):
    with pytest.raises(swr.SwrError) as e:
        call()
    return e.value.code, str(e.value)


@gpu
@pytest.mark.parametrize("device_count", [0, 2])
def test_errors(swr, oracle, case, device_count):
    L = swr.load_library()
    B = swr.binding
    nv = case.v.shape[0]
    d = np.ascontiguousarray(case.d)
    wa = np.ascontiguousarray(WA)
    want = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)

    def targets(**kw):
        f = dict(position_deltas=d.ctypes.data, normal_deltas=None, vertex_count=nv, target_count=5, reserved=0)
        f.update(kw)
        return ctypes.byref(B.MorphTargets(**f))

    def refused(ctx):
        assert L.swr_scene_morph(ctx._h, targets(vertex_count=nv - 1)) == BAD_ARG
        assert L.swr_scene_morph(ctx._h, targets(position_deltas=None)) == BAD_ARG
        assert L.swr_scene_morph(ctx._h, targets(target_count=0)) == BAD_ARG
        assert L.swr_scene_morph(ctx._h, targets(target_count=-3)) == BAD_ARG
        assert L.swr_scene_morph(ctx._h, targets(reserved=1)) == BAD_ARG
        assert L.swr_scene_morph(ctx._h, targets(target_count=257)) == UNSUPPORTED

    with swr.Context(0, device_count=device_count) as ctx:
        assert code_of(swr, lambda: ctx.scene_morph(case.d))[0] == NO_SCENE
        assert code_of(swr, lambda: ctx.morph_set(WA))[0] == NO_SCENE
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        code, text = code_of(swr, lambda: ctx.morph_set(WA))
        assert code == BAD_ARG and "swr_scene_morph" in text, text                      # no targets
        refused(ctx)
        assert code_of(swr, lambda: ctx.morph_set(WA))[0] == BAD_ARG                    # still none
        ctx.scene_morph(case.d)
        ctx.morph_set(WA)
        against(want, grab(ctx, DT), DT, "weights A")
        refused(ctx)
        assert L.swr_morph_set(ctx._h, wa.ctypes.data, 4) == BAD_ARG
        assert L.swr_morph_set(ctx._h, wa.ctypes.data, 6) == BAD_ARG
        assert L.swr_morph_set(ctx._h, wa.ctypes.data, 0) == BAD_ARG
        assert L.swr_morph_set(ctx._h, None, 5) == BAD_ARG
        assert L.swr_morph_set(ctx._h, None, -1) == BAD_ARG
        against(want, grab(ctx, DT), DT, "after the errors the scene, the targets and the weights are unchanged")
        ctx.morph_set(WB)
        against(K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "the targets are still there")
        # an upload drops targets and weights
        ctx.scene_upload(case.v, case.i)
        assert code_of(swr, lambda: ctx.morph_set(WA))[0] == BAD_ARG
        # ... and so does the upload a render performs
        ctx.scene_morph(case.d)
        ctx.morph_set(WA)
        c, dd = ctx.render(case.v, case.i, IDENT, W, H, DT)
        base = K.expected_frame(oracle, case.v, case.i, IDENT, W, H, DT)
        assert dd.tobytes() == base.depth.tobytes() and np.array_equal(c, base.color)
        assert code_of(swr, lambda: ctx.morph_set(WA))[0] == BAD_ARG


@gpu
def test_failed_context_returns_its_sticky_error(swr, case):
    ctx = swr.Context(0, wait_budget_ms=300)
    try:
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        ctx.scene_morph(case.d)
        ctx.morph_set(WA)
        ctx.debug_fault(swr.binding.FAULT_ENQUEUE)      # the next frame's raster share fails as if a launch had returned an error
        try:
            ctx.draw(IDENT, DT)
        except swr.SwrError as e:
            assert e.code == HIP
        assert code_of(swr, lambda: ctx.morph_set(WB))[0] == HIP
        assert code_of(swr, lambda: ctx.scene_morph(case.d))[0] == HIP
        assert code_of(swr, lambda: ctx.scene_morph(None))[0] == HIP
    finally:
        ctx.close()


@gpu
def test_the_example_morphs_its_torus(swr, oracle):
    """examples/frame_loop.py --morph: its frames are the oracle's frames of the model-morphed torus under the app's transform; with
    --skin as well, of the morphed-then-posed one."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    size, t0 = 128, 0.4
    for skin in (False, True):
        v, i, frames = fl.run_morph(2, size, None, True, time0=t0, skin=skin)
        deltas = fl.morph_targets(v)
        assert deltas.shape == (2, v.shape[0], 3) and all(np.abs(deltas[t]).max() > 0.01 for t in range(2))
        for k, (c, d) in enumerate(frames):
            t = t0 + k / 60.0
            w = fl.morph_weights(t)
            assert (np.asarray(w) != 0).all()
            mv = MM.morph_vertices(v, deltas, w)
            if skin:
                joint, weight = fl.bend_skin(v)
                mv = SM.pose_vertices(mv, joint, weight, fl.bend_pose(t))
            wc, wd = K.oracle_clear(oracle, mv, i, swr.scenes.app_transform(t), size, size, DT)
            assert d.tobytes() == wd.tobytes() and np.array_equal(c, wc), f"frame {k}, skin {skin}"
            assert (c[..., 3] == 255).sum() > 500
        assert not np.array_equal(frames[0][0], frames[1][0])


# ---- 11: every kernel swr_morph.hip launches has a GPU case above ---------------------------------------------------------------------
GPU_CASES = {
    "k_morph_vertices<false>": ("test_morphed_frames_match_the_oracle_and_an_uploaded_context", "test_256_resident_targets_and_every_unroll_remainder",
                                "test_a_vertex_count_that_is_no_multiple_of_the_wave_or_the_block", "test_three_bands_cull_with_the_morphed_boxes"),
    "k_morph_vertices<true>": ("test_phong_frames_with_morphed_normals",),
}


def test_every_launched_kernel_has_a_gpu_case():
    src = open(SRC).read()
    body = src[src.index("void launch_morph_vertices("):].replace(" ", "")
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(k_morph_\w+(?:<[^>]*>)?)\)?,", body))
    assert launched == {"k_morph_vertices<true>", "k_morph_vertices<false>"}, launched
    assert "if(attrs)hipLaunchKernelGGL((k_morph_vertices<true>)" in body, "NRM is lifted from the attributes"
    assert set(re.findall(r"__global__[^;{]*?(k_morph_\w+)\(", src)) == {"k_morph_vertices"}
    assert "gridDim" not in src, "one lane per vertex, no capped grid to stride over (else: a case with more vertices than one pass)"
    assert launched == set(GPU_CASES), f"no GPU case for {sorted(launched - set(GPU_CASES))}"
    for variant, tests in GPU_CASES.items():
        for name in tests:
            fn = globals().get(name)
            assert fn is not None, (variant, name)
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), f"{name} is not a GPU test"
