"""Dual-quaternion skinning on the GPU (include/swr.h "Dual-quaternion skinning"): every frame after swr_pose_set_dq is
bit for bit the frame of the model-posed vertices (tests/skin_dq_model.py) — under the oracle, and on a second context that uploaded
them.  The scene is the torus of tests/skin_model.py (768 vertices, 1536 triangles, 24 groups) on 320 x 192 under the twisting pose of
tests/skin_dq_model.py; the kernel's edges use strips of 1 to 1 025 vertices.  tests/test_skin_dq_model.py holds the floors that keep
these cases from being vacuous.  No tolerance anywhere."""
import contextlib
import dataclasses
import os
import re

import numpy as np
import pytest

import item_bounds_model as IBM
import kernel_matrix as K
import morph_model as MM
import skin_dq_model as DQ
import skin_model as SM

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_skin_dq.hip")
DT, NC, METAL, IDS = K.DT, K.NC, K.METAL, K.IDS
REAL_LINES, DEPTH_CLIP, PERSPECTIVE, BLEND = 8, 1024, 2048, 4096
LINE, VERTICES = 1, 2           # SWR_PRIMITIVE_*
W, H = DQ.W, DQ.H
IDENT = K.IDENT
BAD_ARG, HIP, UNSUPPORTED, NO_SCENE = -1, -4, -5, -6
RULE_SETS = {"ztest": DT | IDS, "painter": IDS, "metal": METAL | IDS, "depth_only": DT | NC}


@dataclasses.dataclass
class Case:
    v: np.ndarray
    i: np.ndarray
    joint: np.ndarray
    weight: np.ndarray
    A: np.ndarray           # two dual-quaternion poses
    B: np.ndarray
    vA: np.ndarray
    vB: np.ndarray
    M: np.ndarray           # pose A's two motions as matrices (swr_pose_set)
    vM: np.ndarray


@pytest.fixture(scope="module")
def case(swr):
    v, i = SM.torus(swr.scenes)
    j, w = SM.bend_skin(v)
    A, B, M = DQ.twist_pose(), DQ.twist_pose(-1.4, (-0.1, 0.12, 0.0)), DQ.twist_matrices()
    return Case(v, i, j, w, A, B, DQ.pose_vertices(v, j, w, A), DQ.pose_vertices(v, j, w, B), M, SM.pose_vertices(v, j, w, M))


@contextlib.contextmanager
def resident(swr, v, i, skin=None, pose=None, **kw):
    with swr.Context(0, **kw) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        if skin is not None:
            ctx.scene_skin(*skin)
        if pose is not None:
            ctx.pose_set_dq(pose)
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


# ---- 1: the posed frame is the oracle's frame of the model-posed vertices, and that of a context that uploaded them ----------------
@gpu
@pytest.mark.parametrize("rules", sorted(RULE_SETS))
def test_posed_frames_match_the_oracle_and_an_uploaded_context(swr, oracle, case, rules):
    """z-test, painter's order, the Metal rules with IDs, and (depth_only) the 32-bit depth kernel."""
    flags = RULE_SETS[rules]
    want = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, flags)
    with resident(swr, case.v, case.i, (case.joint, case.weight)) as ctx, resident(swr, case.vA, case.i) as ref:
        bind = grab(ctx, flags)
        ctx.pose_set_dq(case.A)
        got = grab(ctx, flags)
        against(want, got, flags, rules)
        same(got, grab(ref, flags), rules)
        assert differ(bind, got) > 5000, "the pose moves the image"
        if flags & IDS:
            hit = got[2] != K.NONE
            assert hit.sum() > 10000 and np.unique(got[2][hit]).size > 300


# ---- 2: the kernel's edges: the last partial workgroup, the size of the table, both instantiations (every grid here is below the cap
# of 1024 workgroups — 1 025 vertices are 5 — so the grid stride is not among them: tests/test_grid_caps.py crosses it) --------------
def strip(n):
    """n vertices on a zigzag strip across the target, triangles (k, k + 1, k + 2); one vertex: one degenerate triangle."""
    k = np.arange(n, dtype=np.float64)
    xyz = np.stack([-0.8 + 1.6 * k / max(n - 1, 1), np.where(k % 2 == 0, -0.35, 0.35) + 0.1 * np.sin(k), 0.3 + 0.4 * k / max(n, 1)], axis=-1)
    rng = np.random.default_rng(n)
    v = K._pack(xyz, rng.uniform(0.1, 1, (n, 3)))
    t = np.arange(max(n - 2, 1), dtype=np.int64)
    idx = np.stack([t, np.minimum(t + 1, n - 1), np.minimum(t + 2, n - 1)], axis=-1).reshape(-1)
    return np.ascontiguousarray(v), idx


def random_rig(nv, joints, seed):
    """`joints` small rigid motions, every third negated; random influences with normalised weights; the last vertex references the
    highest joint with a weight that is not zero."""
    rng = np.random.default_rng(seed)
    dq = np.stack([DQ.dq_joint(rng.standard_normal(3), rng.uniform(-0.6, 0.6), rng.uniform(-0.08, 0.08, 3)) for _ in range(joints)])
    dq[2::3] = -dq[2::3]
    j = rng.integers(0, joints, (nv, 4)).astype(np.uint32)
    j[nv - 1, 3] = joints - 1
    w = rng.uniform(0.05, 1, (nv, 4)).astype(np.float32)
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    return dq, j, w


EDGES = [(1, 2), (255, 2), (256, 2), (257, 2), (1025, 2), (257, 1), (257, 64), (1025, 1024)]


@gpu
@pytest.mark.parametrize("nv,joints", EDGES)
def test_kernel_edges(swr, nv, joints):
    """Without attributes (k_skin_vertices_dq<false>), then with them under Phong and textured Phong (<true>): triangle and vertex
    frames against a context that uploaded the model's vertices and normals.  No case strides: the largest grid has 5 workgroups."""
    v, i = strip(nv)
    dq, j, w = random_rig(nv, joints, 1000 * joints + nv)
    posed = DQ.pose_vertices(v, j, w, dq)
    assert np.isfinite(posed).all() and not np.array_equal(posed[:, 0:3], v[:, 0:3]) and np.array_equal(posed[:, 3:], v[:, 3:])
    with resident(swr, v, i, (j, w), dq) as ctx, resident(swr, posed, i) as ref:
        for flags, prim in ((DT | IDS, 0), (0, VERTICES)):
            got = grab(ctx, flags, prim)
            same(got, grab(ref, flags, prim), f"{nv} vertices, {joints} joints, primitive {prim}")
            drawn = (got[1] != got[1][0, 0]).any(axis=-1).sum() if prim else np.isfinite(got[0]).sum()    # (points write no depth)
            assert nv < 3 or drawn >= (100 if prim else 1000), "something is drawn"
        # (one vertex draws nothing: the bounds of its one degenerate triangle show where the kernel put it)
        got, want = ctx.item_bounds([(0, i.size, IDENT)], 0), IBM.item_bounds(posed, i, [(0, i.size, IDENT)], W, H, 0)
        assert got[0].tobytes() == want[0].tobytes(), f"{got[0]} is not the model's {want[0]}"
        assert want[0].tobytes() != IBM.item_bounds(v, i, [(0, i.size, IDENT)], W, H, 0)[0].tobytes()
        for shader in (1, 2):
            sh = swr.scenes.random_shading(nv, 0x77, shader)
            for c, attrs in ((ctx, sh.attrs), (ref, DQ.pose_attrs(sh.attrs, j, w, dq))):
                if sh.texture is not None:
                    c.texture_upload(sh.texture)
                c.material_set(swr.binding.Material.from_shading(sh))
                c.scene_attributes(attrs)
            same(grab(ctx, DT), grab(ref, DT), f"{nv} vertices, {joints} joints, shader {shader}")


@gpu
@pytest.mark.parametrize("shader", [1, 2])
def test_phong_frames_with_posed_normals(swr, oracle, case, shader):
    """The torus under Phong and textured Phong against the oracle: the normals are rot(n), in every order of the calls."""
    sh = swr.scenes.random_shading(case.v.shape[0], 0x51, shader)
    posed_sh = dataclasses.replace(sh, attrs=DQ.pose_attrs(sh.attrs, case.joint, case.weight, case.A))
    assert not np.array_equal(posed_sh.attrs[:, 0:3], sh.attrs[:, 0:3]) and np.array_equal(posed_sh.attrs[:, 4:], sh.attrs[:, 4:])
    wc, wd = K.oracle_clear(oracle, case.vA, case.i, IDENT, W, H, DT, shading=posed_sh)
    uc, _ = K.oracle_clear(oracle, case.vA, case.i, IDENT, W, H, DT, shading=sh)
    assert (wc != uc).any(axis=-1).sum() > 3000, "posed normals shade differently"
    for order in ("attributes, skin, pose", "skin, pose, attributes"):
        with resident(swr, case.v, case.i) as ctx:
            if sh.texture is not None:
                ctx.texture_upload(sh.texture)
            ctx.material_set(swr.binding.Material.from_shading(sh))
            for step in order.split(", "):
                {"attributes": lambda: ctx.scene_attributes(sh.attrs), "skin": lambda: ctx.scene_skin(case.joint, case.weight),
                 "pose": lambda: ctx.pose_set_dq(case.A)}[step]()
            d, c, _ = grab(ctx, DT)
            assert d.tobytes() == wd.tobytes() and np.array_equal(c, wc), order


# ---- 3: what only dual quaternions have ----------------------------------------------------------------------------------------------
@gpu
def test_a_negated_joint_gives_the_identical_frame(swr, case):
    """q and -q are the same motion: joints 0 and 1 negated, and the influences moved onto the negated copies (joints 3 and 2)."""
    with resident(swr, case.v, case.i, (case.joint, case.weight), case.A) as ctx:
        want = grab(ctx, DT | IDS)
        neg = case.A.copy()
        neg[0:2] = -neg[0:2]
        ctx.pose_set_dq(neg)
        same(grab(ctx, DT | IDS), want, "joints 0 and 1 negated")
        swapped = case.joint.copy()
        swapped[:, 0], swapped[:, 1] = 3, 2
        ctx.scene_skin(swapped, case.weight)
        ctx.pose_set_dq(case.A)
        same(grab(ctx, DT | IDS), want, "the influences on the negated copies")
        assert np.isfinite(want[0]).sum() > 10000


@gpu
def test_a_zero_blend_drops_its_triangles_like_uploaded_nans(swr, oracle, case):
    w = case.weight.copy()
    w[100:140] = 0.0                                    # l == 0: NaN coordinates
    w[300, :] = [0.5, -0.5, 0, 0]
    j = case.joint.copy()
    j[300] = [0, 3, 0, 0]                               # identity and its negation: the signed weights cancel
    posed = DQ.pose_vertices(case.v, j, w, case.A)
    assert np.isnan(posed[100:140, 0:3]).all() and np.isnan(posed[300, 0:3]).all() and np.isfinite(posed[:100]).all()
    want = K.expected_frame(oracle, posed, case.i, IDENT, W, H, DT | IDS)
    whole = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT | IDS)
    assert (want.depth.view(np.uint32) != whole.depth.view(np.uint32)).sum() > 300, "the dropped triangles leave a hole"
    with resident(swr, case.v, case.i, (j, w), case.A) as ctx, resident(swr, posed, case.i) as ref:
        for flags in (DT | IDS, IDS, DT | NC):
            got = grab(ctx, flags)
            same(got, grab(ref, flags), f"flags {flags}")
        against(want, grab(ctx, DT | IDS), DT | IDS, "a zero blend")


@gpu
def test_the_two_modes_differ_on_the_same_joints(swr, oracle, case):
    """The twist through swr_pose_set (blended matrices, the pinched tube) and through swr_pose_set_dq, each against the oracle."""
    wq = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    wm = K.expected_frame(oracle, case.vM, case.i, IDENT, W, H, DT)
    with resident(swr, case.v, case.i, (case.joint, case.weight)) as ctx:
        ctx.pose_set(case.M)
        m = grab(ctx, DT)
        against(wm, m, DT, "matrices")
        ctx.pose_set_dq(case.A)
        q = grab(ctx, DT)
        against(wq, q, DT, "dual quaternions")
        assert differ(m, q) > 1000
        assert np.isfinite(q[0]).sum() > np.isfinite(m[0]).sum() + 2000, "the dual-quaternion twist keeps the tube's volume"


# ---- 4: sequences ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_pose_sequence_both_kinds_and_the_bind_pose(swr, oracle, case):
    wa = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    wb = K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT)
    wm = K.expected_frame(oracle, case.vM, case.i, IDENT, W, H, DT)
    with resident(swr, case.v, case.i, (case.joint, case.weight)) as ctx:
        never = grab(ctx, DT)
        ctx.pose_set_dq(case.A)
        a = grab(ctx, DT)
        against(wa, a, DT, "pose A")
        ctx.pose_set_dq(case.B)
        b = grab(ctx, DT)
        against(wb, b, DT, "pose B")
        assert differ(a, b) > 5000
        ctx.pose_set(case.M)
        against(wm, grab(ctx, DT), DT, "the matrix pose after a dual-quaternion one")
        ctx.pose_set_dq(case.A)
        against(wa, grab(ctx, DT), DT, "pose A after the matrix pose")
        ctx.pose_set(None)
        same(grab(ctx, DT), never, "swr_pose_set(NULL, 0) restores the bind pose")
        ctx.pose_set(case.M)
        ctx.pose_set_dq(None)
        same(grab(ctx, DT), never, "swr_pose_set_dq(NULL, 0) restores the bind pose")
        ctx.pose_set(case.M)
        against(wm, grab(ctx, DT), DT, "the matrix pose after the bind pose: the kind does not linger")
        # a new skin, and a removed one, restore the bind pose too
        ctx.pose_set_dq(case.A)
        ctx.scene_skin(case.joint, case.weight)
        same(grab(ctx, DT), never, "a new skin")
        ctx.pose_set_dq(case.B)
        ctx.scene_skin(None)
        same(grab(ctx, DT), never, "the skin removed")
        with pytest.raises(swr.SwrError):
            ctx.pose_set_dq(case.A)


@gpu
def test_morph_then_dual_quaternion_pose(swr, oracle, case):
    d = MM.targets(swr.scenes, case.v)
    nd = MM.normal_targets(case.v.shape[0])
    morphed = MM.morph_vertices(case.v, d, MM.WEIGHTS_A)
    posed = DQ.pose_vertices(morphed, case.joint, case.weight, case.A)
    assert not np.array_equal(posed[:, 0:3], case.vA[:, 0:3])
    want = K.expected_frame(oracle, posed, case.i, IDENT, W, H, DT | IDS)
    with resident(swr, case.v, case.i, (case.joint, case.weight)) as ctx:
        ctx.scene_morph(d, nd)
        ctx.morph_set(MM.WEIGHTS_A)
        ctx.pose_set_dq(case.A)
        against(want, grab(ctx, DT | IDS), DT | IDS, "morph, then pose")
        ctx.morph_set(None)
        against(K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "the weights removed: pose A alone")
        ctx.morph_set(MM.WEIGHTS_A)                     # (swr_morph_set re-applies the pose as a dual-quaternion pose)
        against(want, grab(ctx, DT | IDS), DT | IDS, "pose, then morph")
        # with attributes: the morphed normals are rotated
        sh = swr.scenes.random_shading(case.v.shape[0], 0x51, 1)
        ctx.material_set(swr.binding.Material.from_shading(sh))
        ctx.scene_attributes(sh.attrs)
        attrs = DQ.pose_attrs(MM.morph_attrs(sh.attrs, nd, MM.WEIGHTS_A), case.joint, case.weight, case.A)
        wc, wd = K.oracle_clear(oracle, posed, case.i, IDENT, W, H, DT, shading=dataclasses.replace(sh, attrs=attrs))
        dd, cc, _ = grab(ctx, DT)
        assert dd.tobytes() == wd.tobytes() and np.array_equal(cc, wc), "morphed normals, rotated"


@gpu
def test_an_unwaited_frame_keeps_the_pose_it_was_posted_in(swr, oracle, case):
    wa = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    wb = K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT)
    hc, hd = swr.HostImage((H, W, 4), np.uint8), swr.HostImage((H, W), np.float32)
    try:
        with resident(swr, case.v, case.i, (case.joint, case.weight), case.A) as ctx:
            ctx.draw(IDENT, DT)
            ctx.present(hc, hd)
            ctx.pose_set_dq(case.B)
            ctx.draw(IDENT, DT)
            ctx.present_wait()
            against(wa, (hd.array, hc.array, None), DT, "the presented frame, pose A")
            against(wb, (ctx.read_depth(), ctx.read_color(), None), DT, "the next frame, pose B")
    finally:
        hc.free(); hd.free()


@gpu
def test_three_bands_cull_with_the_posed_boxes(swr, oracle, case):
    """Poses that move the mesh from band to band: a group box left over from the pose before would cull what is now there."""
    skin = SM.rigid_skin(case.v.shape[0])
    with resident(swr, case.v, case.i, skin, device_count=3) as ctx:
        assert [b[1:] for b in ctx.bands()] == [(0, 64), (64, 128), (128, 192)]
        never = grab(ctx, DT)
        for name, q in (("up", DQ.UP), ("down", DQ.DOWN), ("up again", DQ.UP)):
            ctx.pose_set_dq(q)
            posed = DQ.pose_vertices(case.v, *skin, q)
            want = K.expected_frame(oracle, posed, case.i, IDENT, W, H, DT | IDS)
            assert (want.ids != K.NONE).sum() > 1000
            against(want, grab(ctx, DT | IDS), DT | IDS, name)
        ctx.pose_set_dq(None)
        same(grab(ctx, DT), never, "the bind pose")


@gpu
def test_a_draw_list_after_a_pose_rebuilds_a_posed_stream(swr, oracle, case):
    n1 = 3 * 500
    items = [(0, n1, K.affine_matrix(0.3, 0.6, -0.35, 0.1)), (n1, case.i.size - n1, K.affine_matrix(-0.2, 0.55, 0.4, -0.15))]
    with resident(swr, case.v, case.i, (case.joint, case.weight), case.A) as ctx:
        frames = []
        for name, posed in (("pose A", case.vA), ("pose B", case.vB)):
            if posed is case.vB:
                ctx.pose_set_dq(case.B)
            cv, ci = K.concat(posed, case.i, items)
            want = K.expected_frame(oracle, cv, ci, IDENT, W, H, DT | IDS)
            assert np.unique(want.ids[want.ids != K.NONE] >= 500).size == 2, "both items are visible"
            frames.append(grab(ctx, DT | IDS, items=items))
            against(want, frames[-1], DT | IDS, name)
        assert differ(*frames) > 3000
        against(K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "a plain frame on the cut stream")


# ---- 5: the other entry points ---------------------------------------------------------------------------------------------------------
@gpu
def test_item_bounds_after_the_pose(swr, case):
    n1 = 3 * 500
    items = [(0, n1, K.affine_matrix(0.3, 0.6, -0.35, 0.1)), (n1, case.i.size - n1, K.perspective_matrix()), (0, case.i.size, IDENT)]
    with resident(swr, case.v, case.i, (case.joint, case.weight), case.A) as ctx:
        for flags in (0, METAL):
            got = ctx.item_bounds(items, flags)
            want = IBM.item_bounds(case.vA, case.i, items, W, H, flags)
            unposed = IBM.item_bounds(case.v, case.i, items, W, H, flags)
            assert want.tobytes() != unposed.tobytes()
            for k in range(len(items)):
                assert got[k].tobytes() == want[k].tobytes(), f"flags {flags}, item {k}: {got[k]} is not the model's {want[k]}"


@gpu
def test_points_and_real_lines_read_the_posed_vertices(swr, case):
    with resident(swr, case.v, case.i, (case.joint, case.weight)) as ctx, resident(swr, case.vA, case.i) as ref:
        for name, flags, prim in (("vertices", DT, VERTICES), ("vertices painter", 0, VERTICES), ("lines", DT | REAL_LINES, LINE),
                                  ("lines painter", REAL_LINES, LINE)):
            bind = grab(ctx, flags, prim)
            ctx.pose_set_dq(case.A)
            got = grab(ctx, flags, prim)
            same(got, grab(ref, flags, prim), name)
            assert differ(bind, got) > 300, name
            ctx.pose_set_dq(None)
            same(grab(ctx, flags, prim), bind, name + ", the bind pose")


@gpu
def test_clip_perspective_and_blend_frames(swr, case):
    m = swr.scenes.app_transform(1.0)
    with resident(swr, case.v, case.i, (case.joint, case.weight), case.A) as ctx, resident(swr, case.vA, case.i) as ref, \
            resident(swr, case.v, case.i) as bind:
        for name, flags in (("clip + perspective", DT | DEPTH_CLIP | PERSPECTIVE | IDS), ("clip", DEPTH_CLIP | IDS),
                            ("perspective, metal", METAL | PERSPECTIVE)):
            got = grab(ctx, flags, m=m)
            same(got, grab(ref, flags, m=m), name)
            assert differ(got, grab(bind, flags, m=m)) > 3000, name
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
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set_dq(case.A)
        against(want, grab(ctx, DT | IDS), DT | IDS, f"order {order}")
        against(K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, IDS), grab(ctx, IDS), IDS, f"order {order}, painter")
        ctx.pose_set_dq(None)
        same(grab(ctx, DT | IDS), never, "the bind pose")


# ---- 6: errors, the example -----------------------------------------------------------------------------------------------------------
def code_of(swr, call):
    with pytest.raises(swr.SwrError) as e:
        call()
    return e.value.code, str(e.value)


@gpu
@pytest.mark.parametrize("device_count", [0, 2])
def test_errors(swr, oracle, case, device_count):
    L = swr.load_library()
    A = np.ascontiguousarray(case.A, dtype=np.float32)
    want = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    with swr.Context(0, device_count=device_count) as ctx:
        code, text = code_of(swr, lambda: ctx.pose_set_dq(case.A))
        assert code == NO_SCENE and "swr_pose_set_dq" in text, text
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        code, text = code_of(swr, lambda: ctx.pose_set_dq(case.A))
        assert code == BAD_ARG and "swr_pose_set_dq needs swr_scene_skin" in text, text         # no skin
        assert L.swr_pose_set_dq(ctx._h, None, 0) == BAD_ARG
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set_dq(case.A)
        against(want, grab(ctx, DT), DT, "pose A")
        assert L.swr_pose_set_dq(ctx._h, A.ctypes.data, -1) == BAD_ARG
        code, text = code_of(swr, lambda: ctx.pose_set_dq(case.A[:3]))
        assert code == BAD_ARG and "swr_pose_set_dq: 3 joints" in text and "joint index 3" in text, text
        assert L.swr_pose_set_dq(ctx._h, None, 4) == BAD_ARG
        assert L.swr_pose_set_dq(ctx._h, A.ctypes.data, 1025) == UNSUPPORTED
        assert L.swr_pose_set(ctx._h, A.ctypes.data, 3) == BAD_ARG
        against(want, grab(ctx, DT), DT, "after the errors the scene and the pose are unchanged")
        # an upload drops skin and pose, and so does the upload a render performs
        ctx.scene_upload(case.v, case.i)
        assert code_of(swr, lambda: ctx.pose_set_dq(case.A))[0] == BAD_ARG
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set_dq(case.A)
        c, d = ctx.render(case.v, case.i, IDENT, W, H, DT)
        bind = K.expected_frame(oracle, case.v, case.i, IDENT, W, H, DT)
        assert d.tobytes() == bind.depth.tobytes() and np.array_equal(c, bind.color)
        assert code_of(swr, lambda: ctx.pose_set_dq(case.A))[0] == BAD_ARG


@gpu
def test_failed_context_returns_its_sticky_error(swr, case):
    ctx = swr.Context(0, wait_budget_ms=300)
    try:
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set_dq(case.A)
        ctx.debug_fault(swr.binding.FAULT_ENQUEUE)      # the next frame's raster share fails as if a launch had returned an error
        try:
            ctx.draw(IDENT, DT)
        except swr.SwrError as e:
            assert e.code == HIP
        assert code_of(swr, lambda: ctx.pose_set_dq(case.B))[0] == HIP
        assert code_of(swr, lambda: ctx.pose_set_dq(None))[0] == HIP
    finally:
        ctx.close()


def load_example():
    import importlib.util
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    return fl


@gpu
def test_the_example_twists_its_torus(swr, oracle):
    """examples/frame_loop.py --skin --dq: its frames are the oracle's frames of the model-posed torus under the app's transform."""
    fl = load_example()
    size, t0 = 128, 0.4
    v, i, frames = fl.run_skin(2, size, None, True, time0=t0, dq=True)
    joint, weight = fl.bend_skin(v)
    for k, (c, d) in enumerate(frames):
        t = t0 + k / 60.0
        mats = fl.twist_pose(t)
        posed = DQ.pose_vertices(v, joint, weight, swr.binding.dual_quats(mats))
        wc, wd = K.oracle_clear(oracle, posed, i, swr.scenes.app_transform(t), size, size, DT)
        assert d.tobytes() == wd.tobytes() and np.array_equal(c, wc), f"frame {k}"
        assert (c[..., 3] == 255).sum() > 500
        linear = SM.pose_vertices(v, joint, weight, DQ.column_major(mats))
        lc, _ = K.oracle_clear(oracle, linear, i, swr.scenes.app_transform(t), size, size, DT)
        assert (lc != wc).any(axis=-1).sum() > 100, "the matrix pose of the same joints is another picture"
    assert not np.array_equal(frames[0][0], frames[1][0])
    # without dq the example is what it was
    _, _, plain = fl.run_skin(1, size, None, True, time0=t0)
    pc, pd = K.oracle_clear(oracle, SM.pose_vertices(v, joint, weight, fl.bend_pose(t0)), i, swr.scenes.app_transform(t0), size, size, DT)
    assert plain[0][1].tobytes() == pd.tobytes() and np.array_equal(plain[0][0], pc)


@gpu
def test_the_example_combines_dq_with_morph_and_with_bounds(swr, oracle):
    fl = load_example()
    size, t0 = 96, 0.3
    v, i, frames = fl.run_morph(1, size, None, True, time0=t0, skin=True, dq=True)
    joint, weight = fl.bend_skin(v)
    morphed = MM.morph_vertices(v, fl.morph_targets(v), fl.morph_weights(t0))
    posed = DQ.pose_vertices(morphed, joint, weight, swr.binding.dual_quats(fl.twist_pose(t0)))
    wc, wd = K.oracle_clear(oracle, posed, i, swr.scenes.app_transform(t0), size, size, DT)
    assert frames[0][1].tobytes() == wd.tobytes() and np.array_equal(frames[0][0], wc)
    _, _, res = fl.run(2, size, None, depth_test=True, time0=t0, objects=3, occlusion=True, bounds=True, skin=True, dq=True)
    _, _, lin = fl.run(2, size, None, depth_test=True, time0=t0, objects=3, occlusion=True, bounds=True, skin=True)
    assert len(res) == 2 and (res[1][0][..., 3] == 255).sum() > 200
    assert not np.array_equal(res[1][0], lin[1][0])


def test_dq_without_skin_is_an_argparse_error():
    import subprocess
    import sys
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "frame_loop.py"), "--dq"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 2 and "--dq is a mode of --skin" in run.stderr, run.stderr[-500:]


# ---- 7: every kernel launch_skin_vertices_dq launches has a GPU case above --------------------------------------------------------------
GPU_CASES = {
    "k_skin_vertices_dq<NRM.value> NRM=false": ("test_posed_frames_match_the_oracle_and_an_uploaded_context", "test_kernel_edges"),
    "k_skin_vertices_dq<NRM.value> NRM=true": ("test_phong_frames_with_posed_normals", "test_kernel_edges"),
}


def test_every_launched_kernel_has_a_gpu_case():
    src = open(SRC).read()
    body = src[src.index("void launch_skin_vertices_dq("):].replace(" ", "")
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(k_\w+(?:<[^>]*>)?)\)?,", body))
    assert launched == {"k_skin_vertices_dq<NRM.value>"}, launched
    assert "with_bools(" in body and "},attrs!=nullptr);" in body, "NRM is lifted from the attributes"
    assert set(re.findall(r"__global__[^;{]*?(k_\w+)\(", src)) == {"k_skin_vertices_dq"}
    assert re.search(r"template<boolNRM>__global__", src.replace(" ", "").replace("\n", "")), "NRM is the one template parameter"
    covered = {k.split(" ")[0] for k in GPU_CASES}
    assert launched == covered, f"no GPU case for {sorted(launched - covered)}"
    assert {k.split(" ")[1] for k in GPU_CASES} == {"NRM=false", "NRM=true"}
    for variant, tests in GPU_CASES.items():
        for name in tests:
            fn = globals().get(name)
            assert fn is not None, (variant, name)
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), f"{name} is not a GPU test"
