"""Skinned meshes on the GPU (include/swr.h "Skinned meshes"): every frame after swr_pose_set is bit for bit the
frame of the model-posed vertices (tests/skin_model.py) — under the oracle, and on a second context that uploaded them.  The scene
is the torus of tests/skin_model.py (768 vertices, 1536 triangles, 24 groups) on 320 x 192; tests/test_skin_model.py holds the
floors that keep these cases from being vacuous."""
import contextlib
import dataclasses
import os
import re

import numpy as np
import pytest

import item_bounds_model as IBM
import kernel_matrix as K
import skin_dq_model as DQ
import skin_model as SM
from test_skin_dq import EDGES, random_rig, strip

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_skin.hip")
DT, NC, METAL, IDS = K.DT, K.NC, K.METAL, K.IDS
REAL_LINES, DEPTH_CLIP, PERSPECTIVE, BLEND = 8, 1024, 2048, 4096
LINE, VERTICES = 1, 2           # SWR_PRIMITIVE_*
W, H = SM.W, SM.H
IDENT = K.IDENT
BAD_ARG, HIP, UNSUPPORTED, NO_SCENE = -1, -4, -5, -6
RULE_SETS = {"ztest": DT | IDS, "painter": IDS, "metal": METAL | IDS, "depth_only": DT | NC}


@dataclasses.dataclass
class Case:
    v: np.ndarray
    i: np.ndarray
    joint: np.ndarray
    weight: np.ndarray
    A: np.ndarray
    B: np.ndarray
    vA: np.ndarray
    vB: np.ndarray


@pytest.fixture(scope="module")
def case(swr):
    v, i = SM.torus(swr.scenes)
    j, w = SM.bend_skin(v)
    A, B = SM.bend_pose(), SM.bend_pose(-0.3, 0.8, -0.15)
    return Case(v, i, j, w, A, B, SM.pose_vertices(v, j, w, A), SM.pose_vertices(v, j, w, B))


@contextlib.contextmanager
def resident(swr, v, i, skin=None, pose=None, **kw):
    with swr.Context(0, **kw) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        if skin is not None:
            ctx.scene_skin(*skin)
        if pose is not None:
            ctx.pose_set(pose)
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


# ---- 1, 2: the posed frame is the oracle's frame of the posed vertices, and that of a context that uploaded them ------------------
@gpu
@pytest.mark.parametrize("rules", sorted(RULE_SETS))
def test_posed_frames_match_the_oracle_and_an_uploaded_context(swr, oracle, case, rules):
    flags = RULE_SETS[rules]
    want = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, flags)
    with resident(swr, case.v, case.i, (case.joint, case.weight)) as ctx, resident(swr, case.vA, case.i) as ref:
        bind = grab(ctx, flags)
        ctx.pose_set(case.A)
        got = grab(ctx, flags)
        against(want, got, flags, rules)
        same(got, grab(ref, flags), rules)
        assert differ(bind, got) > 10000, "the pose moves the image"
        if flags & IDS:
            hit = got[2] != K.NONE
            assert hit.sum() > 10000 and np.unique(got[2][hit]).size > 300


# ---- 2b: the kernel's edges: the last partial workgroup, the size of the table in LDS, both instantiations --------------------------
@gpu
@pytest.mark.parametrize("nv,joints", EDGES)
def test_kernel_edges(swr, nv, joints):
    """The strips and rigs of tests/test_skin_dq.py, their joints as matrices: without attributes (k_skin_vertices<LDS, false>), then
    with them under Phong and textured Phong (<LDS, true>), triangle and vertex frames against a context that uploaded the model's
    vertices and normals.  1 024 joints are 48 KB of dynamic LDS.  (Every grid here is below the cap of 1024 workgroups: the grid
    stride is crossed by tests/test_grid_caps.py.)"""
    v, i = strip(nv)
    dq, j, w = random_rig(nv, joints, 1000 * joints + nv)
    m = DQ.matrices_of(dq)
    assert m.shape == (joints, 16) and int(j.max()) == joints - 1
    posed = SM.pose_vertices(v, j, w, m)
    assert np.isfinite(posed).all() and not np.array_equal(posed[:, 0:3], v[:, 0:3]) and np.array_equal(posed[:, 3:], v[:, 3:])
    with resident(swr, v, i, (j, w), m) as ctx, resident(swr, posed, i) as ref:
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
            for c, attrs in ((ctx, sh.attrs), (ref, SM.pose_attrs(sh.attrs, j, w, m))):
                if sh.texture is not None:
                    c.texture_upload(sh.texture)
                c.material_set(swr.binding.Material.from_shading(sh))
                c.scene_attributes(attrs)
            same(grab(ctx, DT), grab(ref, DT), f"{nv} vertices, {joints} joints, shader {shader}")


# ---- 3: a rigid joint is the frame's transform ----------------------------------------------------------------------------------------
@gpu
def test_a_rigid_joint_equals_the_draw_transform(swr, case):
    M = K.affine_matrix()
    with resident(swr, case.v, case.i, SM.rigid_skin(case.v.shape[0]), M[None]) as ctx, resident(swr, case.v, case.i) as ref:
        for flags in (DT | IDS, IDS, METAL, DT | NC):
            a, b = grab(ctx, flags), grab(ref, flags, m=M)
            same(a, b, f"flags {flags}")
            assert np.isfinite(a[0]).sum() > 10000 or not flags & (DT | METAL)
        assert differ(grab(ctx, DT), grab(ref, DT)) > 5000


# ---- 4: sequences ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_pose_sequence_and_the_bind_pose(swr, oracle, case):
    wa = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    wb = K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT)
    with resident(swr, case.v, case.i, (case.joint, case.weight)) as ctx:
        never = grab(ctx, DT)
        ctx.pose_set(case.A)
        a = grab(ctx, DT)
        against(wa, a, DT, "pose A")
        ctx.pose_set(case.B)
        b = grab(ctx, DT)
        against(wb, b, DT, "pose B")
        assert differ(a, b) > 5000
        ctx.pose_set(None)
        same(grab(ctx, DT), never, "the bind pose again")
        # a new skin, and a removed one, restore the bind pose too
        ctx.pose_set(case.A)
        ctx.scene_skin(case.joint, case.weight)
        same(grab(ctx, DT), never, "a new skin")
        ctx.pose_set(case.B)
        ctx.scene_skin(None)
        same(grab(ctx, DT), never, "the skin removed")
        with pytest.raises(swr.SwrError):
            ctx.pose_set(case.A)


@gpu
def test_an_unwaited_frame_keeps_the_pose_it_was_posted_in(swr, oracle, case):
    wa = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    wb = K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT)
    hc, hd = swr.HostImage((H, W, 4), np.uint8), swr.HostImage((H, W), np.float32)
    try:
        with resident(swr, case.v, case.i, (case.joint, case.weight), case.A) as ctx:
            ctx.draw(IDENT, DT)
            ctx.present(hc, hd)
            ctx.pose_set(case.B)
            ctx.draw(IDENT, DT)
            ctx.present_wait()
            against(wa, (hd.array, hc.array, None), DT, "the presented frame, pose A")
            against(wb, (ctx.read_depth(), ctx.read_color(), None), DT, "the next frame, pose B")
    finally:
        hc.free(); hd.free()


# ---- 5: three bands on one device: the group boxes follow the pose --------------------------------------------------------------
@gpu
def test_three_bands_cull_with_the_posed_boxes(swr, oracle, case):
    skin = SM.rigid_skin(case.v.shape[0])
    with resident(swr, case.v, case.i, skin, device_count=3) as ctx:
        assert [b[1:] for b in ctx.bands()] == [(0, 64), (64, 128), (128, 192)]
        never = grab(ctx, DT)
        for name, m in (("up", SM.UP), ("down", SM.DOWN), ("up again", SM.UP)):
            ctx.pose_set(m[None])
            posed = SM.pose_vertices(case.v, *skin, m[None])
            want = K.expected_frame(oracle, posed, case.i, IDENT, W, H, DT | IDS)
            assert (want.ids != K.NONE).sum() > 1000
            against(want, grab(ctx, DT | IDS), DT | IDS, name)
        ctx.pose_set(None)
        same(grab(ctx, DT), never, "the bind pose")


# ---- 6: a draw list over two ranges cuts the stream: the rebuilt stream is posed again ---------------------------------------------
@gpu
def test_a_draw_list_after_a_pose_rebuilds_a_posed_stream(swr, oracle, case):
    n1 = 3 * 500
    items = [(0, n1, K.affine_matrix(0.3, 0.6, -0.35, 0.1)), (n1, case.i.size - n1, K.affine_matrix(-0.2, 0.55, 0.4, -0.15))]
    with resident(swr, case.v, case.i, (case.joint, case.weight), case.A) as ctx:
        frames = []
        for name, posed in (("pose A", case.vA), ("pose B", case.vB)):
            if posed is case.vB:
                ctx.pose_set(case.B)
            cv, ci = K.concat(posed, case.i, items)
            want = K.expected_frame(oracle, cv, ci, IDENT, W, H, DT | IDS)
            assert np.unique(want.ids[want.ids != K.NONE] >= 500).size == 2, "both items are visible"
            frames.append(grab(ctx, DT | IDS, items=items))
            against(want, frames[-1], DT | IDS, name)
        assert differ(*frames) > 3000
        against(K.expected_frame(oracle, case.vB, case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "a plain frame on the cut stream")


# ---- 7: attributes: the normals are posed, in every order of the calls -------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shader", [1, 2])
def test_phong_frames_with_posed_normals(swr, oracle, case, shader):
    sh = swr.scenes.random_shading(case.v.shape[0], 0x51, shader)
    posed_sh = dataclasses.replace(sh, attrs=SM.pose_attrs(sh.attrs, case.joint, case.weight, case.A))
    assert not np.array_equal(posed_sh.attrs[:, 0:3], sh.attrs[:, 0:3]) and np.array_equal(posed_sh.attrs[:, 4:], sh.attrs[:, 4:])
    wc, wd = K.oracle_clear(oracle, case.vA, case.i, IDENT, W, H, DT, shading=posed_sh)
    uc, _ = K.oracle_clear(oracle, case.vA, case.i, IDENT, W, H, DT, shading=sh)
    assert (wc != uc).any(axis=-1).sum() > 3000, "posed normals shade differently"
    skin = (case.joint, case.weight)
    M = swr.binding.Material.from_shading(sh)

    def check(ctx, what):
        d, c, _ = grab(ctx, DT)
        assert d.tobytes() == wd.tobytes() and np.array_equal(c, wc), what

    for order in ("attributes, skin, pose", "skin, attributes, pose", "skin, pose, attributes"):
        with resident(swr, case.v, case.i) as ctx:
            if sh.texture is not None:
                ctx.texture_upload(sh.texture)
            ctx.material_set(M)
            for step in order.split(", "):
                {"attributes": lambda: ctx.scene_attributes(sh.attrs), "skin": lambda: ctx.scene_skin(*skin),
                 "pose": lambda: ctx.pose_set(case.A)}[step]()
            check(ctx, order)
            if order.endswith("attributes"):
                # the bind pose restores the normals as well
                ctx.pose_set(None)
                bc, bd = K.oracle_clear(oracle, case.v, case.i, IDENT, W, H, DT, shading=sh)
                d, c, _ = grab(ctx, DT)
                assert d.tobytes() == bd.tobytes() and np.array_equal(c, bc), "the bind pose with attributes"


# ---- 8, 9, 10: the other frame types and stream orders, against a context that uploaded the posed vertices ----------------------
@gpu
def test_points_and_real_lines_read_the_posed_vertices(swr, case):
    with resident(swr, case.v, case.i, (case.joint, case.weight)) as ctx, resident(swr, case.vA, case.i) as ref:
        for name, flags, prim in (("vertices", DT, VERTICES), ("vertices painter", 0, VERTICES), ("lines", DT | REAL_LINES, LINE),
                                  ("lines painter", REAL_LINES, LINE)):
            bind = grab(ctx, flags, prim)
            ctx.pose_set(case.A)
            got = grab(ctx, flags, prim)
            same(got, grab(ref, flags, prim), name)
            assert differ(bind, got) > 500, name
            ctx.pose_set(None)
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
        ctx.pose_set(case.A)
        against(want, grab(ctx, DT | IDS), DT | IDS, f"order {order}")
        against(K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, IDS), grab(ctx, IDS), IDS, f"order {order}, painter")
        ctx.pose_set(None)
        same(grab(ctx, DT | IDS), never, "the bind pose")


# ---- 11: a pose that crowds a few tiles is an ordinary overflow -------------------------------------------------------------------
@gpu
def test_a_pose_that_overflows_the_bins_is_repaired(swr, oracle):
    """Forced as tests/test_depth_query.py forces it with vertices: a fresh context, 20 000 triangles that the pose collapses into
    a few tiles.  The first read repairs the frame."""
    w, h = 1280, 720
    s = swr.scenes.random_soup(20000, w, h, 555, r_ndc=0.01, flags=DT, margin=1.0)
    skin = SM.rigid_skin(s.vertices.shape[0])
    m = np.array([0.035, 0, 0, 0, 0, 0.03, 0, 0, 0, 0, 1, 0, 0.335, 0.13, 0, 1], dtype=np.float32)
    posed = SM.pose_vertices(s.vertices, *skin, m[None])
    wc, wd = K.oracle_clear(oracle, posed, s.indices, s.transform, w, h, DT)
    ys, xs = np.nonzero(np.isfinite(wd))
    assert 200 < ys.size < 64 * 32 * 4 and xs.max() - xs.min() < 128 and ys.max() - ys.min() < 64
    with swr.Context(0) as ctx:
        ctx.target_set(w, h)
        ctx.scene_upload(s.vertices, s.indices)
        ctx.scene_skin(*skin)
        ctx.pose_set(m[None])
        ctx.draw(s.transform, DT)
        assert ctx.read_depth().tobytes() == wd.tobytes(), "overflowed last frame"
        assert np.array_equal(ctx.read_color(), wc)


# ---- 12: errors ---------------------------------------------------------------------------------------------------------------------
def code_of(swr, call):
    with pytest.raises(swr.SwrError) as e:
        call()
    return e.value.code, str(e.value)


@gpu
@pytest.mark.parametrize("device_count", [0, 2])
def test_errors(swr, oracle, case, device_count):
    L = swr.load_library()
    nv = case.v.shape[0]
    sk = np.zeros(nv, dtype=swr.binding.SKIN_VERTEX_DTYPE)
    sk["joint"], sk["weight"] = case.joint, case.weight
    A = np.ascontiguousarray(case.A, dtype=np.float32)
    want = K.expected_frame(oracle, case.vA, case.i, IDENT, W, H, DT)
    with swr.Context(0, device_count=device_count) as ctx:
        assert code_of(swr, lambda: ctx.scene_skin(case.joint, case.weight))[0] == NO_SCENE
        assert code_of(swr, lambda: ctx.pose_set(case.A))[0] == NO_SCENE
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        assert code_of(swr, lambda: ctx.pose_set(case.A))[0] == BAD_ARG             # no skin
        assert L.swr_scene_skin(ctx._h, sk.ctypes.data, nv - 1) == BAD_ARG
        assert L.swr_scene_skin(ctx._h, None, nv) == BAD_ARG
        bad = sk.copy()
        bad["joint"][nv // 2, 2] = 1024
        assert L.swr_scene_skin(ctx._h, bad.ctypes.data, nv) == BAD_ARG
        ctx.scene_skin(sk)
        ctx.pose_set(case.A)
        against(want, grab(ctx, DT), DT, "pose A")
        assert L.swr_pose_set(ctx._h, A.ctypes.data, -1) == BAD_ARG
        code, text = code_of(swr, lambda: ctx.pose_set(case.A[:3]))
        assert code == BAD_ARG and "3 joints" in text and "joint index 3" in text, text
        assert L.swr_pose_set(ctx._h, None, 4) == BAD_ARG
        assert L.swr_pose_set(ctx._h, A.ctypes.data, 1025) == UNSUPPORTED
        assert L.swr_scene_skin(ctx._h, bad.ctypes.data, nv) == BAD_ARG
        against(want, grab(ctx, DT), DT, "after the errors the scene and the pose are unchanged")
        # an upload drops skin and pose
        ctx.scene_upload(case.v, case.i)
        assert code_of(swr, lambda: ctx.pose_set(case.A))[0] == BAD_ARG
        # ... and so does the upload a render performs
        ctx.scene_skin(sk)
        ctx.pose_set(case.A)
        c, d = ctx.render(case.v, case.i, IDENT, W, H, DT)
        bind = K.expected_frame(oracle, case.v, case.i, IDENT, W, H, DT)
        assert d.tobytes() == bind.depth.tobytes() and np.array_equal(c, bind.color)
        assert code_of(swr, lambda: ctx.pose_set(case.A))[0] == BAD_ARG


@gpu
def test_failed_context_returns_its_sticky_error(swr, case):
    ctx = swr.Context(0, wait_budget_ms=300)
    try:
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set(case.A)
        ctx.debug_fault(swr.binding.FAULT_ENQUEUE)      # the next frame's raster share fails as if a launch had returned an error
        try:
            ctx.draw(IDENT, DT)
        except swr.SwrError as e:
            assert e.code == HIP
        assert code_of(swr, lambda: ctx.pose_set(case.B))[0] == HIP
        assert code_of(swr, lambda: ctx.scene_skin(case.joint, case.weight))[0] == HIP
    finally:
        ctx.close()


@gpu
def test_the_example_bends_its_torus(swr, oracle):
    """examples/frame_loop.py --skin: its frames are the oracle's frames of the model-posed torus under the app's transform."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    size, t0 = 128, 0.4
    v, i, frames = fl.run_skin(2, size, None, True, time0=t0)
    joint, weight = fl.bend_skin(v)
    assert (weight[:, 0] > 0).any() and (weight[:, 1] > 0).any()
    for k, (c, d) in enumerate(frames):
        t = t0 + k / 60.0
        posed = SM.pose_vertices(v, joint, weight, fl.bend_pose(t))
        wc, wd = K.oracle_clear(oracle, posed, i, swr.scenes.app_transform(t), size, size, DT)
        assert d.tobytes() == wd.tobytes() and np.array_equal(c, wc), f"frame {k}"
        assert (c[..., 3] == 255).sum() > 500
    assert not np.array_equal(frames[0][0], frames[1][0])


# ---- 13: every kernel swr_skin.hip launches has a GPU case above ----------------------------------------------------------------------
GPU_CASES = {
    # (k_skin_vertices<TABLE_LDS, NRM>: TABLE_LDS is the build's choice, SWR_TUNE_SKIN_LDS)
    "k_skin_vertices<LDS.value,NRM.value> NRM=false": ("test_posed_frames_match_the_oracle_and_an_uploaded_context", "test_stream_orders",
                                                       "test_kernel_edges"),
    "k_skin_vertices<LDS.value,NRM.value> NRM=true": ("test_phong_frames_with_posed_normals", "test_kernel_edges"),
    "k_skin_stream<false>": ("test_posed_frames_match_the_oracle_and_an_uploaded_context", "test_three_bands_cull_with_the_posed_boxes"),
    "k_skin_stream<true>": ("test_phong_frames_with_posed_normals",),
}


def test_every_launched_kernel_has_a_gpu_case():
    src = open(SRC).read()
    body = src[src.index("void launch_skin_vertices("):].replace(" ", "")
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(k_skin_\w+(?:<[^>]*>)?)\)?,", body))
    assert launched == {"k_skin_vertices<LDS.value,NRM.value>", "k_skin_stream<true>", "k_skin_stream<false>"}, launched
    assert "with_bools(" in body and "},lds,attrs!=nullptr);" in body, "NRM is lifted from the attributes"
    assert set(re.findall(r"__global__[^;{]*?(k_skin_\w+)\(", src)) == {"k_skin_vertices", "k_skin_stream"}
    covered = {k.split(" ")[0] for k in GPU_CASES}
    assert launched == covered, f"no GPU case for {sorted(launched - covered)}"
    for variant, tests in GPU_CASES.items():
        for name in tests:
            fn = globals().get(name)
            assert fn is not None, (variant, name)
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), f"{name} is not a GPU test"
