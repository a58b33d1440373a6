"""Sparse morph targets and swr_morph_pose_set on the GPU (include/swr.h "Sparse morph targets", "Weights and joints in one call",
DESIGN.md §28): every frame after the call is bit for bit the frame of the model-morphed (then model-posed) vertices
(tests/morph_sparse_model.py, tests/skin_model.py, tests/skin_dq_model.py) — under the oracle, and on a second context that uploaded
them.  The scene is the torus of tests/morph_model.py (768 vertices, 1536 triangles) with the seven sparse targets of
tests/morph_sparse_model.py on 320 x 192; tests/test_morph_sparse_model.py holds the floors that keep these cases from being vacuous.
No tolerance anywhere."""
import contextlib
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import kernel_matrix as K
import morph_model as MM
import morph_sparse_model as MS
import skin_dq_model as DQ
import skin_model as SM
from test_morph import against, code_of, differ, grab, same

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_morph_sparse.hip")
DT, NC, METAL, IDS = K.DT, K.NC, K.METAL, K.IDS
REAL_LINES = 8
LINE, VERTICES = 1, 2           # SWR_PRIMITIVE_*
W, H = MS.W, MS.H
IDENT = K.IDENT
BAD_ARG, HIP, UNSUPPORTED, NO_SCENE = -1, -4, -5, -6
RULE_SETS = {"ztest": DT | IDS, "painter": IDS, "metal": METAL | IDS, "depth_only": DT | NC}
WA, WB = MS.WEIGHTS_A, MS.WEIGHTS_B


@dataclasses.dataclass
class Case:
    v: np.ndarray
    i: np.ndarray
    T: list                 # the seven targets
    TN: list                # the same with normal deltas
    vA: np.ndarray
    vB: np.ndarray
    joint: np.ndarray
    weight: np.ndarray
    P: np.ndarray           # two matrix poses
    Q: np.ndarray
    D: np.ndarray           # a dual-quaternion pose


@pytest.fixture(scope="module")
def case(swr):
    v, i = MM.torus(swr.scenes)
    T = MS.rig(swr.scenes, v)
    j, w = SM.bend_skin(v)
    return Case(v, i, T, MS.rig(swr.scenes, v, normals=True), MS.morph_vertices(v, T, WA), MS.morph_vertices(v, T, WB), j, w,
                SM.bend_pose(), SM.bend_pose(-0.3, 0.8, -0.15), DQ.twist_pose())


@contextlib.contextmanager
def resident(swr, v, i, targets=None, weights=None, **kw):
    with swr.Context(0, **kw) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        if targets is not None:
            ctx.scene_morph_sparse(targets)
        if weights is not None:
            ctx.morph_set(weights)
        yield ctx


def want(oracle, case, w, flags=DT, T=None):
    return K.expected_frame(oracle, MS.morph_vertices(case.v, case.T if T is None else T, w), case.i, IDENT, W, H, flags)


# ---- 1: the morphed frame is the oracle's frame of the morphed vertices, and that of a context that uploaded them -------------------
@gpu
@pytest.mark.parametrize("rules", sorted(RULE_SETS))
def test_morphed_frames_match_the_oracle_and_an_uploaded_context(swr, oracle, case, rules):
    """z-test, painter's order, the Metal rules with IDs, and (depth_only) the 32-bit depth kernel."""
    flags = RULE_SETS[rules]
    with resident(swr, case.v, case.i, case.T) as ctx, resident(swr, case.vA, case.i) as ref:
        base = grab(ctx, flags)
        ctx.morph_set(WA)
        got = grab(ctx, flags)
        against(K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, flags), got, flags, rules)
        same(got, grab(ref, flags), rules)
        assert differ(base, got) > 10000, "the morph moves the image"


# ---- 2: weight sets by the lengths of the rows they leave active ---------------------------------------------------------------------
@gpu
def test_rows_of_every_active_length_then_zero_and_null(swr, oracle, case):
    """With the lift the rows hold 1, 2, 4 or 5 entries.  Active entries per row — the last vertex alone: 0 everywhere but one row (a
    touched vertex whose targets are all inactive comes out as the base bits); the swell: 0 or 1; A: 0 or 2; swell, shear and lift:
    1 or 3; B: up to 4 of 5 (the non-finite target at -0, the empty one at 2)."""
    sets = [("the last vertex", MS.one(MS.LAST)), ("swell", MS.one(MS.SWELL)), ("A", WA),
            ("swell, shear, lift", MS.one(MS.SWELL, 0.5) + MS.one(MS.SHEAR, -1.0) + MS.one(MS.LIFT, 0.25)), ("B", WB), ("the last vertex again", MS.one(MS.LAST))]
    with resident(swr, case.v, case.i, case.T) as ctx:
        never = grab(ctx, DT | IDS)
        frames = []
        for name, w in sets:
            ctx.morph_set(w)
            frames.append(grab(ctx, DT | IDS))
            against(want(oracle, case, w, DT | IDS), frames[-1], DT | IDS, name)
        assert 0 < differ(never, frames[0]) < 615 and differ(frames[0], frames[1]) > 10000 and differ(frames[2], frames[4]) > 5000
        same(frames[0], frames[5], "every touched vertex is rewritten from the base: nothing of B stays")
        ctx.morph_set(np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0], dtype=np.float32))
        same(grab(ctx, DT | IDS), never, "all weights zero")
        ctx.morph_set(WA)
        ctx.morph_set(None)
        same(grab(ctx, DT | IDS), never, "NULL weights")
        ctx.morph_set(None)
        same(grab(ctx, DT | IDS), never, "NULL weights twice")


@gpu
@pytest.mark.parametrize("scene", ["one_triangle", "torus"])
def test_256_targets_on_the_first_and_the_last_vertex(swr, case, scene):
    """256 resident targets that all list vertex 0 and vertex nv - 1 (rows of 256 entries, next to rows of none), with 0, 1, 3 and 256
    of them active, the last one included: against a context that uploaded the model's vertices, through a triangle frame with IDs
    and a .vertices frame (which reads the morphed array itself)."""
    if scene == "one_triangle":
        v = swr.scenes.pack_vertices(np.array([[-0.6, -0.5, 0.3], [0.7, -0.4, 0.5], [0.1, 0.8, 0.4]], dtype=np.float32),
                                     np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32))
        i = np.array([0, 1, 2], dtype=np.int64)
    else:
        v, i = case.v, case.i
    nv = v.shape[0]
    rng = np.random.RandomState(0x256 + nv)
    idx = np.array([0, nv - 1], dtype=np.uint32)
    T = [(idx, ((rng.random_sample((2, 3)) - 0.5) * 0.02).astype(np.float32)) for _ in range(256)]
    w_all = ((rng.random_sample(256) - 0.5) * 2.0).astype(np.float32)
    w_all[w_all == 0] = 0.5
    with resident(swr, v, i, T) as ctx:
        base = grab(ctx, DT | IDS)
        seen = []
        for count in (0, 1, 3, 256):
            w = np.zeros(256, dtype=np.float32)
            pick = np.arange(256) if count == 256 else 255 - np.arange(count) * (256 // max(count, 1))     # (the last one included)
            w[pick] = w_all[pick]
            ctx.morph_set(w)
            mv = MS.morph_vertices(v, T, w)
            assert (mv[1:-1] == v[1:-1]).all() and (count == 0) == np.array_equal(mv, v)
            with resident(swr, mv, i) as ref:
                got = grab(ctx, DT | IDS)
                same(got, grab(ref, DT | IDS), f"{count} of 256 active")
                same(grab(ctx, DT, VERTICES), grab(ref, DT, VERTICES), f"{count} of 256 active, .vertices")
            seen.append(got)
            if count == 0:
                same(got, base, "none active")
        assert differ(seen[-1], base) > 0 and differ(seen[-1], seen[-2]) > 0


# ---- 3: ragged shapes ----------------------------------------------------------------------------------------------------------------
@gpu
def test_773_vertices_and_the_461_vertex_union(swr, oracle, case):
    """773 vertices under a full-length target: three full blocks of 256 and a ragged wave of 5 lanes, whose vertices the last
    triangles use.  And the rig without the lift: 461 touched vertices, 7 waves and 13 lanes, in two blocks."""
    extra = swr.scenes.pack_vertices(np.array([[-0.9, -0.9, 0.2], [-0.6, -0.9, 0.2], [-0.9, -0.6, 0.2], [0.9, 0.9, 0.1], [0.6, 0.8, 0.1]], dtype=np.float32),
                                     np.full((5, 3), 0.5, dtype=np.float32))
    v = np.concatenate([case.v, extra])
    i = np.concatenate([case.i, np.array([768, 769, 770, 770, 771, 772], dtype=np.int64)])
    every = np.arange(773, dtype=np.uint32)
    shift = np.zeros((773, 3), dtype=np.float32)
    shift[:, 0] = 0.11
    T = [case.T[MS.SWELL], (every, shift), (np.array([772], dtype=np.uint32), np.array([[0, -0.3, 0]], dtype=np.float32))]
    w = np.array([0.75, 1.0, 1.0], dtype=np.float32)
    mv = MS.morph_vertices(v, T, w)
    assert v.shape[0] == 773 and not np.array_equal(mv[768:, 0:3], v[768:, 0:3])
    with resident(swr, v, i, T, w) as ctx, resident(swr, mv, i) as ref:
        same(grab(ctx, DT | IDS), grab(ref, DT | IDS), "773 vertices")
        same(grab(ctx, DT, VERTICES), grab(ref, DT, VERTICES), "773 vertices, .vertices")
    T6 = [t for k, t in enumerate(case.T) if k != MS.LIFT]
    w6 = np.delete(WB, MS.LIFT)
    assert MS.touched(T6).size == 461
    with resident(swr, case.v, case.i, T6, w6) as ctx:
        got = grab(ctx, DT | IDS)
        against(want(oracle, case, w6, DT | IDS, T=T6), got, DT | IDS, "461 touched vertices")
        with resident(swr, MS.morph_vertices(case.v, T6, w6), case.i) as ref:
            same(grab(ctx, DT, VERTICES), grab(ref, DT, VERTICES), "461 touched vertices, .vertices")


@gpu
def test_the_empty_target_and_the_all_empty_set(swr, oracle, case):
    none = (np.zeros(0, dtype=np.uint32), np.zeros((0, 3), dtype=np.float32))
    with resident(swr, case.v, case.i, case.T) as ctx:
        never = grab(ctx, DT)
        ctx.morph_set(MS.one(MS.EMPTY, 5.0))
        same(grab(ctx, DT), never, "the empty target alone, active")
        ctx.morph_set(MS.one(MS.EMPTY, np.nan) + MS.one(MS.SHEAR))
        against(want(oracle, case, MS.one(MS.SHEAR)), grab(ctx, DT), DT, "the empty target at NaN beside the shear")
        ctx.scene_morph_sparse([none, none, none])                 # nothing is touched: nothing is ever launched
        same(grab(ctx, DT), never, "an all-empty set: every weight 0")
        ctx.morph_set([1.0, np.nan, -2.0])
        same(grab(ctx, DT), never, "an all-empty set, active")
        with resident(swr, case.v, case.i) as ref:
            same(grab(ctx, DT, VERTICES), grab(ref, DT, VERTICES), "an all-empty set, .vertices: the pre-filled array is the base")
        ctx.morph_set(None)
        same(grab(ctx, DT), never, "an all-empty set, NULL weights")


@gpu
def test_a_zero_weight_skips_the_non_finite_target_and_a_tiny_one_poisons_its_vertices_only(swr, oracle, case):
    with resident(swr, case.v, case.i, case.T) as ctx:
        for zero in (0.0, -0.0):
            w = WA.copy()
            w[MS.NONFINITE] = zero
            ctx.morph_set(w)
            against(want(oracle, case, WA), grab(ctx, DT), DT, f"the non-finite target at {zero}")
        w = WA.copy()
        w[MS.NONFINITE] = 1e-30
        ctx.morph_set(w)
        poisoned = MS.morph_vertices(case.v, case.T, w)
        assert (~np.isfinite(poisoned[:, 0:3]).all(axis=1)).sum() == 154
        got = grab(ctx, DT)
        against(K.expected_frame(oracle, poisoned, case.i, IDENT, W, H, DT), got, DT, "the non-finite target at 1e-30")
        assert 1000 < np.isfinite(got[0]).sum() < np.isfinite(want(oracle, case, WA).depth).sum(), "only the triangles of listed vertices are gone"
        ctx.morph_set(WA)
        against(want(oracle, case, WA), grab(ctx, DT), DT, "weights A again")


@gpu
def test_negative_zero_stays_on_an_unlisted_vertex(swr):
    """The hand-made scene of tests/test_morph_sparse_model.py: a listed zero delta makes -0 into +0, an unlisted vertex keeps -0.
    The transform's z row is all -0 but for m[10] = 1, so that z = -0 reaches the depth of a .vertices frame as it is."""
    xyz = np.array([[0.25, 0.25, -0.0], [0.5, 0.25, -0.0], [0.25, 0.5, 0.5]], dtype=np.float32)
    v = swr.scenes.pack_vertices(xyz, np.eye(3, dtype=np.float32))
    i = np.array([0, 1, 2], dtype=np.int64)
    T = [(np.array([0, 2], dtype=np.uint32), np.array([[0, 0, 0], [0.25, 0, 0]], dtype=np.float32))]
    mv = MS.morph_vertices(v, T, [1.0])
    dense = MM.morph_vertices(v, MS.dense(T, 3), [1.0])
    assert mv[:, 2].view(np.uint32).tolist() == [0, 0x80000000, 0x3F000000] and dense[:, 2].view(np.uint32).tolist() == [0, 0, 0x3F000000]
    m = np.array(IDENT, dtype=np.float32).copy()
    m[[2, 6, 14]] = -0.0
    with resident(swr, v, i, T, [1.0]) as ctx, resident(swr, mv, i) as ref:
        for name, flags, prim in (("triangle", DT | IDS, 0), ("vertices", DT, VERTICES), ("vertices painter", 0, VERTICES)):
            same(grab(ctx, flags, prim, m=m), grab(ref, flags, prim, m=m), name)


# ---- 4: three bands on one device: the group boxes follow the morph -----------------------------------------------------------------
@gpu
def test_three_bands_cull_with_the_morphed_boxes(swr, oracle, case):
    """The lift takes the torus out of the lowest band (tests/test_morph_sparse_model.py): with stale group boxes every band would
    cull by where the groups were."""
    with resident(swr, case.v, case.i, case.T, device_count=3) as ctx:
        assert [b[1:] for b in ctx.bands()] == [(0, 64), (64, 128), (128, 192)]
        never = grab(ctx, DT)
        for name, w in (("up", MS.one(MS.LIFT, 1.0)), ("down", MS.one(MS.LIFT, -1.0)), ("up and swollen", MS.one(MS.LIFT, 1.0) + MS.one(MS.SWELL, 1.0))):
            ctx.morph_set(w)
            wf = want(oracle, case, w, DT | IDS)
            assert (wf.ids != K.NONE).sum() > 1000
            against(wf, grab(ctx, DT | IDS), DT | IDS, name)
        ctx.morph_set(None)
        same(grab(ctx, DT), never, "all weights zero")


# ---- 5: attributes: the normals are morphed, in every order of the calls ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shader", [1, 2])
def test_phong_frames_with_sparse_normal_deltas(swr, oracle, case, shader):
    sh = swr.scenes.random_shading(case.v.shape[0], 0x51, shader)
    morphed_sh = dataclasses.replace(sh, attrs=MS.morph_attrs(sh.attrs, case.TN, WB))
    assert not np.array_equal(morphed_sh.attrs[:, 0:3], sh.attrs[:, 0:3]) and np.array_equal(morphed_sh.attrs[:, 3:], sh.attrs[:, 3:])
    wc, wd = K.oracle_clear(oracle, case.vB, case.i, IDENT, W, H, DT, shading=morphed_sh)
    uc, ud = K.oracle_clear(oracle, case.vB, case.i, IDENT, W, H, DT, shading=sh)
    assert (wc != uc).any(axis=-1).sum() > 3000, "morphed normals shade differently"
    M = swr.binding.Material.from_shading(sh)

    def check(ctx, c, d, what):
        gd, gc, _ = grab(ctx, DT)
        assert gd.tobytes() == d.tobytes() and np.array_equal(gc, c), what

    for order in ("attributes, targets, weights", "targets, attributes, weights", "targets, weights, attributes"):
        for T, (c, d) in ((case.TN, (wc, wd)), (case.T, (uc, ud))):
            with resident(swr, case.v, case.i) as ctx:
                if sh.texture is not None:
                    ctx.texture_upload(sh.texture)
                ctx.material_set(M)
                for step in order.split(", "):
                    {"attributes": lambda: ctx.scene_attributes(sh.attrs), "targets": lambda: ctx.scene_morph_sparse(T),
                     "weights": lambda: ctx.morph_set(WB)}[step]()
                check(ctx, c, d, order + (", normal deltas" if T is case.TN else ", no normal deltas: the normals stay as uploaded"))
                if order.endswith("attributes") and T is case.TN:
                    # zero weights restore the normals as well; and with a skin the pose reads the morphed normals
                    ctx.morph_set(None)
                    check(ctx, *K.oracle_clear(oracle, case.v, case.i, IDENT, W, H, DT, shading=sh), "zero weights with attributes")
                    ctx.scene_skin(case.joint, case.weight)
                    ctx.morph_pose_set(WB, case.P)
                    both = dataclasses.replace(sh, attrs=SM.pose_attrs(morphed_sh.attrs, case.joint, case.weight, case.P))
                    vb = SM.pose_vertices(case.vB, case.joint, case.weight, case.P)
                    check(ctx, *K.oracle_clear(oracle, vb, case.i, IDENT, W, H, DT, shading=both), "morphed normals, posed, in one call")


# ---- 6: morph first, then skin; the combined call -------------------------------------------------------------------------------------
def posed(case, w, pose, dq=False):
    mv = MS.morph_vertices(case.v, case.T, w)
    return DQ.pose_vertices(mv, case.joint, case.weight, pose) if dq else SM.pose_vertices(mv, case.joint, case.weight, pose)


@gpu
@pytest.mark.parametrize("dq", [False, True])
def test_sparse_then_skin_in_both_call_orders(swr, oracle, case, dq):
    pose = case.D if dq else case.P

    def set_pose(ctx, p):
        ctx.pose_set_dq(p) if dq else ctx.pose_set(p)

    wAP = K.expected_frame(oracle, posed(case, WA, pose, dq), case.i, IDENT, W, H, DT | IDS)
    for order in ("morph, pose", "pose, morph"):
        with resident(swr, case.v, case.i, case.T) as ctx:
            ctx.scene_skin(case.joint, case.weight)
            for step in order.split(", "):
                {"morph": lambda: ctx.morph_set(WA), "pose": lambda: set_pose(ctx, pose)}[step]()
            against(wAP, grab(ctx, DT | IDS), DT | IDS, order)
            ctx.morph_set(WB)
            against(K.expected_frame(oracle, posed(case, WB, pose, dq), case.i, IDENT, W, H, DT | IDS), grab(ctx, DT | IDS), DT | IDS, order + ", new weights")
            ctx.morph_set(None)
            against(K.expected_frame(oracle, posed(case, np.zeros(7), pose, dq), case.i, IDENT, W, H, DT | IDS), grab(ctx, DT | IDS), DT | IDS,
                    order + ", the pose alone")
            ctx.morph_set(WB)
            set_pose(ctx, None)
            against(K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT | IDS), grab(ctx, DT | IDS), DT | IDS, order + ", the morph alone")
    # targets given after the skin and the pose
    with resident(swr, case.v, case.i) as ctx:
        ctx.scene_skin(case.joint, case.weight)
        set_pose(ctx, pose)
        ctx.scene_morph_sparse(case.T)
        ctx.morph_set(WA)
        against(wAP, grab(ctx, DT | IDS), DT | IDS, "skin, pose, targets, weights")


@gpu
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_the_combined_call_is_the_two_calls(swr, oracle, case, kind):
    """swr_morph_pose_set against swr_morph_set + swr_pose_set (and _dq) on a second context, on sparse and on dense targets; NULL
    halves; and after each half's errors neither the weights nor the pose have changed."""
    L = swr.load_library()
    T = case.T if kind == "sparse" else MS.dense(case.T[:5], 768)
    wa, wb = (WA, WB) if kind == "sparse" else (WA[:5], WB[:5])

    def install(ctx):
        ctx.scene_morph_sparse(T) if kind == "sparse" else ctx.scene_morph(T)
        ctx.scene_skin(case.joint, case.weight)

    with resident(swr, case.v, case.i) as one, resident(swr, case.v, case.i) as two:
        install(one); install(two)
        for name, w, pose, dq in (("A, P", wa, case.P, False), ("B, Q", wb, case.Q, False), ("A, D (dual quaternions)", wa, case.D, True),
                                  ("none, P", None, case.P, False), ("B, none", wb, None, False), ("none, none", None, None, True), ("B, D", wb, case.D, True)):
            one.morph_pose_set(w, pose, dq=dq)
            two.morph_set(w)
            two.pose_set_dq(pose) if dq else two.pose_set(pose)
            got = grab(one, DT | IDS)
            same(got, grab(two, DT | IDS), name)
            if kind == "sparse":
                mv = posed(case, np.zeros(7) if w is None else w, pose, dq) if pose is not None else MS.morph_vertices(case.v, T, np.zeros(7) if w is None else w)
                against(K.expected_frame(oracle, mv, case.i, IDENT, W, H, DT | IDS), got, DT | IDS, name)
        held = grab(one, DT | IDS)
        w = np.ascontiguousarray(wa)
        p = np.ascontiguousarray(case.P, dtype=np.float32).reshape(-1, 16)
        n, J = w.shape[0], p.shape[0]
        for args, code in (((w.ctypes.data, n - 1, p.ctypes.data, J, 0), BAD_ARG), ((None, n, p.ctypes.data, J, 0), BAD_ARG),
                           ((w.ctypes.data, n, p.ctypes.data, 1, 0), BAD_ARG), ((w.ctypes.data, n, None, J, 0), BAD_ARG),
                           ((w.ctypes.data, n, p.ctypes.data, -1, 0), BAD_ARG), ((w.ctypes.data, n, p.ctypes.data, 1025, 0), UNSUPPORTED),
                           ((w.ctypes.data, n, p.ctypes.data, J, 2), BAD_ARG), ((w.ctypes.data, n, p.ctypes.data, J, -1), BAD_ARG)):
            assert L.swr_morph_pose_set(one._h, *args) == code, args[1:]
        same(grab(one, DT | IDS), held, "after the errors the frame is the same")
        # ... and so is the state: a draw list that cuts the stream re-applies weights B and pose D
        n1 = 3 * 500
        items = [(0, n1, IDENT), (n1, case.i.size - n1, IDENT)]
        same((grab(one, DT, items=items)[0],), (held[0],), "the rebuilt stream holds weights B and pose D")
    # without targets, and without a skin
    with resident(swr, case.v, case.i) as ctx:
        assert code_of(swr, lambda: ctx.morph_pose_set(wa, case.P))[0] == BAD_ARG
        ctx.scene_morph_sparse(T) if kind == "sparse" else ctx.scene_morph(T)
        code, text = code_of(swr, lambda: ctx.morph_pose_set(wa, case.P))
        assert code == BAD_ARG and "swr_morph_pose_set needs swr_scene_skin" in text, text
        against(K.expected_frame(oracle, case.v, case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "the weights were not taken either")


@gpu
def test_unwaited_frames_keep_the_shape_they_were_posted_in(swr, oracle, case):
    """draw, present, call, draw — for swr_morph_set on sparse targets and for swr_morph_pose_set."""
    hc, hd = swr.HostImage((H, W, 4), np.uint8), swr.HostImage((H, W), np.float32)
    try:
        with resident(swr, case.v, case.i, case.T, WA) as ctx:
            ctx.scene_skin(case.joint, case.weight)
            ctx.draw(IDENT, DT)
            ctx.present(hc, hd)
            ctx.morph_set(WB)
            ctx.draw(IDENT, DT)
            ctx.present_wait()
            against(want(oracle, case, WA), (hd.array, hc.array, None), DT, "the presented frame, weights A")
            against(want(oracle, case, WB), (ctx.read_depth(), ctx.read_color(), None), DT, "the next frame, weights B")
            ctx.draw(IDENT, DT)
            ctx.present(hc, hd)
            ctx.morph_pose_set(WA, case.P)
            ctx.draw(IDENT, DT)
            ctx.present_wait()
            against(want(oracle, case, WB), (hd.array, hc.array, None), DT, "the presented frame, weights B")
            against(K.expected_frame(oracle, posed(case, WA, case.P), case.i, IDENT, W, H, DT), (ctx.read_depth(), ctx.read_color(), None), DT,
                    "the next frame, weights A in pose P")
    finally:
        hc.free(); hd.free()


# ---- 7: a draw list over two ranges cuts the stream: the rebuilt stream is morphed again ------------------------------------------
@gpu
def test_a_draw_list_cuts_the_stream_and_new_weights_follow(swr, oracle, case):
    n1 = 3 * 500
    items = [(0, n1, K.affine_matrix(0.3, 0.6, -0.35, 0.1)), (n1, case.i.size - n1, K.affine_matrix(-0.2, 0.55, 0.4, -0.15))]
    with resident(swr, case.v, case.i, case.T, WA) as ctx:
        frames = []
        for name, morphed in (("weights A", case.vA), ("weights B", case.vB)):
            if morphed is case.vB:
                ctx.morph_set(WB)
            cv, ci = K.concat(morphed, case.i, items)
            wf = K.expected_frame(oracle, cv, ci, IDENT, W, H, DT | IDS)
            frames.append(grab(ctx, DT | IDS, items=items))
            against(wf, frames[-1], DT | IDS, name)
        assert differ(*frames) > 3000
        against(K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "a plain frame on the cut stream")


# ---- 8: the other frame types read the morphed array ---------------------------------------------------------------------------------
@gpu
def test_points_and_real_lines_read_the_morphed_vertices(swr, case):
    with resident(swr, case.v, case.i, case.T) as ctx, resident(swr, case.vA, case.i) as ref:
        for name, flags, prim in (("vertices", DT, VERTICES), ("vertices painter", 0, VERTICES), ("lines", DT | REAL_LINES, LINE)):
            base = grab(ctx, flags, prim)
            ctx.morph_set(WA)
            got = grab(ctx, flags, prim)
            same(got, grab(ref, flags, prim), name)
            assert differ(base, got) > 200, name
            ctx.morph_set(None)
            same(grab(ctx, flags, prim), base, name + ", all weights zero")
        ctx.scene_skin(case.joint, case.weight)
        ctx.morph_pose_set(WA, case.P)
        with resident(swr, posed(case, WA, case.P), case.i) as ref2:
            same(grab(ctx, DT, VERTICES), grab(ref2, DT, VERTICES), "vertices, morphed and posed")


# ---- 9: dense and sparse targets replace each other on one context ------------------------------------------------------------------
@gpu
def test_dense_and_sparse_targets_replace_each_other(swr, oracle, case):
    d = MM.targets(swr.scenes, case.v)
    dA = K.expected_frame(oracle, MM.morph_vertices(case.v, d, MM.WEIGHTS_A), case.i, IDENT, W, H, DT)
    base = K.expected_frame(oracle, case.v, case.i, IDENT, W, H, DT)
    with resident(swr, case.v, case.i) as ctx:
        ctx.scene_morph(d)
        ctx.morph_set(MM.WEIGHTS_A)
        against(dA, grab(ctx, DT), DT, "dense")
        ctx.scene_morph_sparse(case.T)
        against(base, grab(ctx, DT), DT, "sparse over active dense targets: every weight 0")
        with pytest.raises(swr.SwrError):
            ctx.morph_set(MM.WEIGHTS_A)                 # seven targets now
        ctx.morph_set(WB)
        against(want(oracle, case, WB), grab(ctx, DT), DT, "sparse")
        ctx.scene_morph(d)
        against(base, grab(ctx, DT), DT, "dense over active sparse targets: every weight 0")
        ctx.morph_set(MM.WEIGHTS_A)
        against(dA, grab(ctx, DT), DT, "dense again")
        ctx.scene_morph_sparse(case.T)
        ctx.morph_set(WA)
        against(want(oracle, case, WA), grab(ctx, DT), DT, "sparse again")
        ctx.scene_morph(None)                           # either NULL removes whichever kind is resident
        against(base, grab(ctx, DT), DT, "sparse targets removed by swr_scene_morph(NULL)")
        assert code_of(swr, lambda: ctx.morph_set(WA))[0] == BAD_ARG
        ctx.scene_morph(d)
        ctx.morph_set(MM.WEIGHTS_A)
        ctx.scene_morph_sparse(None)
        against(base, grab(ctx, DT), DT, "dense targets removed by swr_scene_morph_sparse(NULL)")
        assert code_of(swr, lambda: ctx.morph_set(MM.WEIGHTS_A))[0] == BAD_ARG
    # A second pass with the rig without the lift.  Its union is 461 of the 768 vertices, so the 307 others come from the pre-fill
    # alone: above, the lift lists every vertex, and a pre-fill that is missing or stale changes nothing.  The set in front moves
    # every vertex each time (weights B lift the whole torus), dense or sparse.
    T6 = [t for k, t in enumerate(case.T) if k != MS.LIFT]
    w6a, w6b = np.delete(WA, MS.LIFT), np.delete(WB, MS.LIFT)
    outside = np.setdiff1d(np.arange(768), MS.touched(T6))
    dense_b = MM.morph_vertices(case.v, d, MM.WEIGHTS_B)
    assert outside.size == 307 and (dense_b[outside, 0:3] != case.v[outside, 0:3]).any(axis=1).all()
    assert (case.vB[outside, 0:3] != case.v[outside, 0:3]).any(axis=1).all()
    dB = K.expected_frame(oracle, dense_b, case.i, IDENT, W, H, DT)
    with resident(swr, case.v, case.i) as ctx:
        ctx.scene_morph(d)
        ctx.morph_set(MM.WEIGHTS_B)
        against(dB, grab(ctx, DT), DT, "dense, every vertex moved")
        ctx.scene_morph_sparse(T6)
        against(base, grab(ctx, DT), DT, "the partial union over active dense targets: every weight 0")
        ctx.morph_set(w6b)
        against(want(oracle, case, w6b, T=T6), grab(ctx, DT), DT, "the partial union: outside it nothing of the dense morph is left")
        ctx.scene_morph(d)
        ctx.morph_set(MM.WEIGHTS_B)
        against(dB, grab(ctx, DT), DT, "dense again")
        ctx.scene_morph_sparse(T6)
        ctx.morph_set(w6a)
        against(want(oracle, case, w6a, T=T6), grab(ctx, DT), DT, "the partial union again, other weights")
        ctx.scene_morph_sparse(case.T)                  # one sparse set after another, with another union
        ctx.morph_set(WB)
        against(want(oracle, case, WB), grab(ctx, DT), DT, "the seven targets: every vertex lifted")
        ctx.scene_morph_sparse(T6)
        against(base, grab(ctx, DT), DT, "the partial union over an active sparse set: every weight 0")
        ctx.morph_set(w6b)
        against(want(oracle, case, w6b, T=T6), grab(ctx, DT), DT, "the partial union: outside it nothing of the lift is left")


# ---- 10: errors -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("device_count", [0, 2])
def test_errors(swr, oracle, case, device_count):
    L = swr.load_library()
    B = swr.binding
    nv = case.v.shape[0]
    keep = [(np.ascontiguousarray(t[0]), np.ascontiguousarray(t[1]), np.ascontiguousarray(n[2])) for t, n in zip(case.T, case.TN)]
    bad_range = keep[MS.LIFT][0].copy(); bad_range[-1] = nv
    twice = keep[MS.LIFT][0].copy(); twice[5] = twice[4]
    down = keep[MS.LIFT][0].copy(); down[[7, 8]] = down[[8, 7]]

    def sparse(edit=None, normals=False, **kw):
        recs = (B.MorphSparseTarget * 7)()
        for k, (idx, dp, dn) in enumerate(keep):
            recs[k] = B.MorphSparseTarget(idx.ctypes.data if idx.size else None, dp.ctypes.data if idx.size else None,
                                          dn.ctypes.data if normals and idx.size else None, idx.size)
        if edit:
            edit(recs)
        f = dict(targets=recs, vertex_count=nv, target_count=7, reserved=0)
        f.update(kw)
        s = B.MorphSparse(**f)
        s._recs = recs
        return s

    def field(k, name, value):
        return lambda recs: setattr(recs[k], name, value)

    def refused(ctx):
        for s, code, words in ((sparse(vertex_count=nv - 1), BAD_ARG, None), (sparse(targets=None), BAD_ARG, None), (sparse(target_count=0), BAD_ARG, None),
                               (sparse(target_count=-3), BAD_ARG, None), (sparse(reserved=1), BAD_ARG, None), (sparse(target_count=257), UNSUPPORTED, None),
                               (sparse(field(0, "count", -1)), BAD_ARG, None), (sparse(field(MS.LIFT, "count", nv + 1)), BAD_ARG, None),
                               (sparse(field(1, "indices", None)), BAD_ARG, None), (sparse(field(1, "position_deltas", None)), BAD_ARG, None),
                               (sparse(field(MS.LIFT, "indices", bad_range.ctypes.data)), BAD_ARG, f"target 2, position {nv - 1}"),
                               (sparse(field(MS.LIFT, "indices", twice.ctypes.data)), BAD_ARG, "target 2, position 5"),
                               (sparse(field(MS.LIFT, "indices", down.ctypes.data)), BAD_ARG, "target 2, position 8"),
                               (sparse(field(MS.UNSWELL, "normal_deltas", None), normals=True), BAD_ARG, "target 4")):
            assert L.swr_scene_morph_sparse(ctx._h, ctypes.byref(s)) == code
            if words:
                with pytest.raises(swr.SwrError) as e:
                    ctx._check(code)
                assert words in str(e.value), str(e.value)

    with swr.Context(0, device_count=device_count) as ctx:
        assert code_of(swr, lambda: ctx.scene_morph_sparse(case.T))[0] == NO_SCENE
        assert code_of(swr, lambda: ctx.morph_pose_set(WA, case.P))[0] == NO_SCENE
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        code, text = code_of(swr, lambda: ctx.morph_set(WA))
        assert code == BAD_ARG and "swr_morph_set needs swr_scene_morph first" in text, text      # the message stays as it is
        refused(ctx)
        assert code_of(swr, lambda: ctx.morph_set(WA))[0] == BAD_ARG                              # still none
        ctx.scene_morph_sparse(case.T)
        ctx.morph_set(WA)
        against(want(oracle, case, WA), grab(ctx, DT), DT, "weights A")
        refused(ctx)
        wa = np.ascontiguousarray(WA)
        assert L.swr_morph_set(ctx._h, wa.ctypes.data, 6) == BAD_ARG
        assert L.swr_morph_set(ctx._h, wa.ctypes.data, 8) == BAD_ARG
        assert L.swr_morph_set(ctx._h, None, 7) == BAD_ARG
        against(want(oracle, case, WA), grab(ctx, DT), DT, "after the errors the scene, the targets and the weights are unchanged")
        ctx.morph_set(WB)
        against(want(oracle, case, WB), grab(ctx, DT), DT, "the targets are still there")
        # an upload drops targets and weights, and so does the upload a render performs
        ctx.scene_upload(case.v, case.i)
        assert code_of(swr, lambda: ctx.morph_set(WA))[0] == BAD_ARG
        ctx.scene_morph_sparse(case.T)
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
        ctx.scene_morph_sparse(case.T)
        ctx.scene_skin(case.joint, case.weight)
        ctx.morph_set(WA)
        ctx.debug_fault(swr.binding.FAULT_ENQUEUE)      # the next frame's raster share fails as if a launch had returned an error
        try:
            ctx.draw(IDENT, DT)
        except swr.SwrError as e:
            assert e.code == HIP
        assert code_of(swr, lambda: ctx.morph_set(WB))[0] == HIP
        assert code_of(swr, lambda: ctx.scene_morph_sparse(case.T))[0] == HIP
        assert code_of(swr, lambda: ctx.scene_morph_sparse(None))[0] == HIP
        assert code_of(swr, lambda: ctx.morph_pose_set(WB, case.P))[0] == HIP
    finally:
        ctx.close()


# ---- 11: the example ------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_example_morphs_its_torus_through_sparse_targets(swr, oracle):
    """examples/frame_loop.py --morph --sparse: the same frames as --morph — the oracle's frames of the model-morphed torus under the
    app's transform; with --skin as well (then through swr_morph_pose_set), of the morphed-then-posed one."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    size, t0 = 128, 0.4
    for skin in (False, True):
        v, i, frames = fl.run_morph(2, size, None, True, time0=t0, skin=skin, sparse=True)
        deltas = fl.morph_targets(v)
        T = swr.binding.sparse_targets(deltas)
        assert all(0 < t[0].size <= v.shape[0] for t in T) and T[1][0].size < v.shape[0], "each target is restricted to the vertices it moves"
        for k, (c, d) in enumerate(frames):
            t = t0 + k / 60.0
            w = fl.morph_weights(t)
            mv = MS.morph_vertices(v, T, w)         # (the sphere has -0 coordinates on vertices the twist drops: they stay -0)
            if skin:
                joint, weight = fl.bend_skin(v)
                mv = SM.pose_vertices(mv, joint, weight, fl.bend_pose(t))
            wc, wd = K.oracle_clear(oracle, mv, i, swr.scenes.app_transform(t), size, size, DT)
            assert d.tobytes() == wd.tobytes() and np.array_equal(c, wc), f"frame {k}, skin {skin}"
        assert not np.array_equal(frames[0][0], frames[1][0])


# ---- 12: every kernel swr_morph_sparse.hip launches has a GPU case above --------------------------------------------------------------
GPU_CASES = {
    "k_morph_sparse<false>": ("test_morphed_frames_match_the_oracle_and_an_uploaded_context", "test_rows_of_every_active_length_then_zero_and_null",
                              "test_256_targets_on_the_first_and_the_last_vertex", "test_773_vertices_and_the_461_vertex_union",
                              "test_three_bands_cull_with_the_morphed_boxes"),
    "k_morph_sparse<true>": ("test_phong_frames_with_sparse_normal_deltas",),
}


def test_every_launched_kernel_has_a_gpu_case():
    src = open(SRC).read()
    body = src[src.index("void launch_morph_sparse("):].replace(" ", "")
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(k_morph_\w+(?:<[^>]*>)?)\)?,", body))
    assert launched == {"k_morph_sparse<true>", "k_morph_sparse<false>"}, launched
    assert "if(a.attrs)hipLaunchKernelGGL((k_morph_sparse<true>)" in body, "NRM is lifted from the attributes"
    assert "if(a.touched_count<=0)return;" in body, "no touched vertex: no launch (a zero grid is a launch error)"
    assert set(re.findall(r"__global__[^;{]*?(k_morph_\w+)\(", src)) == {"k_morph_sparse"}
    assert "gridDim" not in src and "std::min" not in src, "one lane per touched vertex: no capped grid, no stride"
    assert launched == set(GPU_CASES), f"no GPU case for {sorted(launched - set(GPU_CASES))}"
    for variant, tests in GPU_CASES.items():
        for name in tests:
            fn = globals().get(name)
            assert fn is not None, (variant, name)
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), f"{name} is not a GPU test"
