"""Computed normals on the GPU (include/swr.h "Computed normals"): under a Phong material every frame after
swr_scene_normals is bit for bit the frame of the model's vertices and normals (tests/normals_model.py over tests/morph_sparse_model.py,
tests/skin_model.py and tests/skin_dq_model.py) — under the oracle, and on a second context that uploaded them: the same indices
with the n_i for SWR_NORMALS_SMOOTH, the de-indexed scene with the f_p for SWR_NORMALS_FLAT.  The scenes are the torus of
tests/morph_model.py (768 vertices, 1536 triangles) and the hub of tests/normals_model.py (312 vertices, 304 triangles) on 320 x 192;
tests/test_normals_model.py holds the floors that keep these cases from being vacuous.  No tolerance anywhere."""
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
import normals_model as NM
import skin_dq_model as DQ
import skin_model as SM
from test_morph import against, code_of, differ, grab, same

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_normals.hip")
DT, NC, METAL, IDS = K.DT, K.NC, K.METAL, K.IDS
VERTICES = 2                    # SWR_PRIMITIVE_VERTICES
W, H = NM.W, NM.H
IDENT = K.IDENT
BAD_ARG, HIP, UNSUPPORTED, NO_SCENE = -1, -4, -5, -6
SMOOTH, FLAT, UPLOADED = NM.SMOOTH, NM.FLAT, NM.UPLOADED
RULE_SETS = {"ztest": DT | IDS, "metal": METAL | IDS}
WA = MS.WEIGHTS_A
MODES = [(SMOOTH, False), (SMOOTH, True), (FLAT, False), (FLAT, True)]
MODE_IDS = ["smooth", "smooth-flip", "flat", "flat-flip"]


@dataclasses.dataclass
class Case:
    v: np.ndarray
    i: np.ndarray
    a: np.ndarray           # the torus's own normals and uv: what is uploaded
    sh: object              # the Phong material (its attrs are replaced per frame)
    T: list                 # the seven sparse targets, without normal deltas
    TN: list                # the same with normal deltas
    joint: np.ndarray
    weight: np.ndarray
    P: np.ndarray           # two matrix poses
    Q: np.ndarray
    D: np.ndarray           # a dual-quaternion pose
    shown: dict             # state -> the vertices the frame draws (the model's), computed once


@pytest.fixture(scope="module")
def case(swr):
    S = swr.scenes
    v, i = NM.torus(S)
    j, w = NM.torus_skin(v)
    T = NM.torus_rig(S, v)
    P, Q, D = SM.bend_pose(), SM.bend_pose(-0.3, 0.8, -0.15), DQ.twist_pose()
    mv = MS.morph_vertices(v, T, WA)
    shown = {"bind": v, "morphed": mv, "posed": SM.pose_vertices(v, j, w, P), "posed_dq": DQ.pose_vertices(v, j, w, D),
             "both": SM.pose_vertices(mv, j, w, P), "posed_q": SM.pose_vertices(v, j, w, Q)}
    return Case(v, i, NM.torus_uploaded_attrs(S), S.random_shading(768, 0x51, 1), T, NM.torus_rig(S, v, normals=True), j, w, P, Q, D, shown)


@contextlib.contextmanager
def resident(swr, v, i, attrs, sh, order=None, **kw):
    """A context with the scene, its attributes (None: none yet) and the material."""
    with swr.Context(0, **kw) as ctx:
        if order is not None:
            ctx.debug_set(swr.binding.DEBUG_STREAM_ORDER, order)
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        if attrs is not None:
            ctx.scene_attributes(attrs)
            ctx.material_set(swr.binding.Material.from_shading(sh))
        yield ctx


def apply(ctx, case, state):
    """Puts a context that holds the rig and the skin into `state`."""
    if state == "bind":
        ctx.morph_pose_set(None, None)
    elif state == "morphed":
        ctx.pose_set(None)
        ctx.morph_set(WA)
    elif state == "posed":
        ctx.morph_set(None)
        ctx.pose_set(case.P)
    elif state == "posed_dq":
        ctx.morph_set(None)
        ctx.pose_set_dq(case.D)
    else:
        ctx.morph_pose_set(WA, case.P)


def want(oracle, sh, scene, flags):
    v, a, i = scene
    return K.expected_frame(oracle, v, i, IDENT, W, H, flags, shading=dataclasses.replace(sh, attrs=a))


def check(swr, oracle, ctx, sh, scene, what, rules=("ztest",)):
    """The context's frames against the oracle's frames of `scene` and against a context that uploaded it."""
    v, a, i = scene
    with resident(swr, v, i, a, sh) as ref:
        for r in rules:
            flags = RULE_SETS[r]
            got = grab(ctx, flags)
            against(want(oracle, sh, scene, flags), got, flags, f"{what}, {r}")
            same(got, grab(ref, flags), f"{what}, {r}, against an uploaded context")
    return got


# ---- 1: both modes, with and without FLIP, on the torus in five states ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,flip", MODES, ids=MODE_IDS)
def test_the_torus_in_every_state(swr, oracle, case, mode, flip):
    """The bind pose; morphed only, by targets without normal deltas; posed only, by matrices and by dual quaternions; both, through
    swr_morph_pose_set.  The mode is set once and persists: every later call recomputes the normals."""
    with resident(swr, case.v, case.i, case.a, case.sh) as ctx:
        ctx.scene_morph_sparse(case.T)
        ctx.scene_skin(case.joint, case.weight)
        uploaded = grab(ctx, DT)
        ctx.scene_normals(mode, flip=flip)
        frames = {}
        for state in ("bind", "morphed", "posed", "posed_dq", "both"):
            apply(ctx, case, state)
            frames[state] = check(swr, oracle, ctx, case.sh, NM.expected_scene(mode, case.shown[state], case.a, case.i, flip), state, ("ztest", "metal"))
        assert uploaded[0].tobytes() != frames["posed"][0].tobytes() and differ(frames["bind"], frames["morphed"]) > 10000
        apply(ctx, case, "bind")
        assert (grab(ctx, DT)[1] != uploaded[1]).any(axis=-1).sum() > 10000, "computed normals shade differently from the uploaded ones"
        assert grab(ctx, DT)[0].tobytes() == uploaded[0].tobytes(), "normals never move a depth"


@gpu
def test_dense_targets_with_normal_deltas_have_no_effect_under_a_computed_mode(swr, oracle, case):
    """Normal deltas and the normal half of the skin are left out while a computed mode is in effect, and come back with UPLOADED."""
    dense, dense_n = MS.dense(case.TN[:5], 768), MS.dense(case.TN[:5], 768, which=2)
    w = WA[:5]
    mv = SM.pose_vertices(MM.morph_vertices(case.v, dense, w), case.joint, case.weight, case.P)
    with resident(swr, case.v, case.i, case.a, case.sh) as ctx:
        ctx.scene_morph(dense, dense_n)
        ctx.scene_skin(case.joint, case.weight)
        ctx.morph_pose_set(w, case.P)
        before = grab(ctx, DT)
        ctx.scene_normals(SMOOTH)
        check(swr, oracle, ctx, case.sh, NM.expected_scene(SMOOTH, mv, case.a, case.i), "dense targets with normal deltas, SMOOTH")
        ctx.scene_normals(FLAT)
        check(swr, oracle, ctx, case.sh, NM.expected_scene(FLAT, mv, case.a, case.i), "dense targets with normal deltas, FLAT")
        ctx.scene_normals(UPLOADED)
        same(grab(ctx, DT), before, "UPLOADED: the morphed and posed uploaded normals again")


# ---- 2: the hub scene --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,flip", MODES, ids=MODE_IDS)
def test_the_hub(swr, oracle, mode, flip):
    """A row of 300 next to rows of 0, 1 and 2, a triangle that names a vertex twice, a NaN corner, 312 vertices and 304 triangles:
    two workgroups each, the second partly filled."""
    S = swr.scenes
    v, i = NM.hub(S)
    a = NM.hub_attrs(S)
    sh = S.random_shading(NM.HUB_NV, 0x4B, 1)
    with resident(swr, v, i, a, sh) as ctx:
        uploaded = grab(ctx, DT)
        ctx.scene_normals(mode, flip=flip)
        got = check(swr, oracle, ctx, sh, NM.expected_scene(mode, v, a, i, flip), "the hub", ("ztest", "metal"))
        ctx.scene_normals(None)
        same(grab(ctx, DT), uploaded, "NULL restores the uploaded normals")
    assert np.isfinite(got[0]).sum() > 20000


# ---- 3: the slot order of the stream -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order", [1, 0, -1])
@pytest.mark.parametrize("mode", [SMOOTH, FLAT], ids=["smooth", "flat"])
def test_stream_orders(swr, oracle, case, mode, order):
    """SWR_DEBUG_STREAM_ORDER 1: Morton order; 0: the caller's order; -1: as for 2^24 primitives or more (slot == primitive)."""
    with resident(swr, case.v, case.i, case.a, case.sh, order=order) as ctx:
        ctx.scene_skin(case.joint, case.weight)
        ctx.scene_normals(mode)
        ctx.pose_set(case.P)
        scene = NM.expected_scene(mode, case.shown["posed"], case.a, case.i)
        against(want(oracle, case.sh, scene, DT | IDS), grab(ctx, DT | IDS), DT | IDS, f"order {order}")
        against(want(oracle, case.sh, scene, IDS), grab(ctx, IDS), IDS, f"order {order}, painter")


# ---- 4: the order of the calls ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", [SMOOTH, FLAT], ids=["smooth", "flat"])
def test_call_orders(swr, oracle, case, mode):
    posed = want(oracle, case.sh, NM.expected_scene(mode, case.shown["posed"], case.a, case.i), DT)
    posed_q = want(oracle, case.sh, NM.expected_scene(mode, case.shown["posed_q"], case.a, case.i), DT)
    # normals before attributes: kept, in effect when they arrive
    with resident(swr, case.v, case.i, None, case.sh) as ctx:
        ctx.scene_normals(mode)
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set(case.P)
        against(K.expected_frame(oracle, case.shown["posed"], case.i, IDENT, W, H, DT), grab(ctx, DT), DT, "no attributes yet: the passthrough frame")
        ctx.scene_attributes(case.a)
        ctx.material_set(swr.binding.Material.from_shading(case.sh))
        against(posed, grab(ctx, DT), DT, "normals, skin, pose, attributes")
    # normals after the skin and the pose
    with resident(swr, case.v, case.i, case.a, case.sh) as ctx:
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set(case.P)
        ctx.scene_normals(mode)
        against(posed, grab(ctx, DT), DT, "skin, pose, normals")
        # normals between two poses; and new targets, a new skin and new attributes keep the mode
        ctx.pose_set(case.Q)
        against(posed_q, grab(ctx, DT), DT, "pose, normals, pose")
        ctx.scene_morph_sparse(case.TN)
        ctx.morph_set(WA)
        ctx.pose_set(case.P)
        both = NM.expected_scene(mode, case.shown["both"], case.a, case.i)
        against(want(oracle, case.sh, both, DT), grab(ctx, DT), DT, "sparse targets with normal deltas under the mode")
        ctx.scene_attributes(case.a)
        against(want(oracle, case.sh, both, DT), grab(ctx, DT), DT, "new attributes under the mode")
        ctx.scene_skin(case.joint, case.weight)
        morphed = NM.expected_scene(mode, case.shown["morphed"], case.a, case.i)
        against(want(oracle, case.sh, morphed, DT), grab(ctx, DT), DT, "a new skin under the mode: the bind pose")
        # a draw list over two ranges cuts the stream: the rebuilt stream gets its normals again
        n1 = 3 * 500
        items = [(0, n1, K.affine_matrix(0.3, 0.6, -0.35, 0.1)), (n1, case.i.size - n1, K.affine_matrix(-0.2, 0.55, 0.4, -0.15))]
        mv, ma, mi = morphed
        cv, ci = K.concat(mv, mi, items)             # (the de-indexed scene has as many indices: the same ranges)
        ca = np.concatenate([ma, ma])
        got = grab(ctx, DT | IDS, items=items)
        against(K.expected_frame(oracle, cv, ci, IDENT, W, H, DT | IDS, shading=dataclasses.replace(case.sh, attrs=ca)), got, DT | IDS, "a draw list")
        against(want(oracle, case.sh, morphed, DT), grab(ctx, DT), DT, "a plain frame on the cut stream")


# ---- 5: UPLOADED and NULL restore the frame of a context that never set a mode -------------------------------------------------------
@gpu
def test_uploaded_and_null_restore_the_parents_frames(swr, oracle, case):
    """The uploaded normals come back morphed (with their normal deltas) and posed, bit for bit, from either computed mode."""
    def install(ctx):
        ctx.scene_morph_sparse(case.TN)
        ctx.scene_skin(case.joint, case.weight)

    with resident(swr, case.v, case.i, case.a, case.sh) as ctx, resident(swr, case.v, case.i, case.a, case.sh) as never:
        install(ctx); install(never)
        for name, act in (("bind", lambda c: None), ("morphed", lambda c: c.morph_set(WA)), ("morphed and posed", lambda c: c.pose_set(case.P)),
                          ("dual quaternions", lambda c: c.pose_set_dq(case.D)), ("posed", lambda c: c.morph_set(None))):
            act(never)
            ctx.scene_normals(SMOOTH, flip=True)
            act(ctx)
            computed = grab(ctx, DT | IDS)
            ctx.scene_normals(UPLOADED)
            held = grab(never, DT | IDS)
            same(grab(ctx, DT | IDS), held, f"{name}: UPLOADED after SMOOTH")
            assert differ(computed, held) > 10000, name
            ctx.scene_normals(FLAT)
            ctx.scene_normals(None)
            same(grab(ctx, DT | IDS), held, f"{name}: NULL after FLAT")
            ctx.scene_normals(None)
            same(grab(ctx, DT | IDS), held, f"{name}: NULL twice")
        ctx.pose_set(case.P)
        both = dataclasses.replace(case.sh, attrs=SM.pose_attrs(case.a, case.joint, case.weight, case.P))
        against(K.expected_frame(oracle, case.shown["posed"], case.i, IDENT, W, H, DT, shading=both), grab(ctx, DT), DT, "the oracle's posed uploaded normals")


# ---- 6: a new upload discards the mode ---------------------------------------------------------------------------------------------------
@gpu
def test_an_upload_discards_the_mode(swr, oracle, case):
    plain = want(oracle, case.sh, (case.v, case.a, case.i), DT)
    with resident(swr, case.v, case.i, case.a, case.sh) as ctx:
        ctx.scene_normals(SMOOTH)
        assert differ(grab(ctx, DT), (plain.depth, plain.color)) > 10000
        ctx.scene_upload(case.v, case.i)
        ctx.scene_attributes(case.a)
        against(plain, grab(ctx, DT), DT, "after swr_scene_upload")
        ctx.scene_normals(FLAT)
        c, d = ctx.render(case.v, case.i, IDENT, W, H, DT, shading=dataclasses.replace(case.sh, attrs=case.a))
        assert d.tobytes() == plain.depth.tobytes() and np.array_equal(c, plain.color), "the upload a swr_render performs"
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        ctx.scene_attributes(case.a)
        ctx.material_set(swr.binding.Material.from_shading(case.sh))
        against(plain, grab(ctx, DT), DT, "after the render's scene was replaced")
        # SMOOTH on the new scene builds the new scene's adjacency: the hub after the torus
        v, i = NM.hub(swr.scenes)
        a = NM.hub_attrs(swr.scenes)
        ctx.scene_upload(v, i)
        ctx.scene_attributes(a)
        ctx.scene_normals(SMOOTH, flip=True)
        against(want(oracle, case.sh, NM.expected_scene(SMOOTH, v, a, i, True), DT), grab(ctx, DT), DT, "the hub after the torus")


# ---- 7: two bands on one device ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", [SMOOTH, FLAT], ids=["smooth", "flat"])
def test_two_bands(swr, oracle, case, mode):
    with resident(swr, case.v, case.i, case.a, case.sh, device_count=2) as ctx:
        assert len(ctx.bands()) == 2
        ctx.scene_morph_sparse(case.T)
        ctx.scene_skin(case.joint, case.weight)
        ctx.scene_normals(mode, flip=True)
        for state in ("both", "morphed"):
            apply(ctx, case, state)
            scene = NM.expected_scene(mode, case.shown[state], case.a, case.i, True)
            against(want(oracle, case.sh, scene, DT | IDS), grab(ctx, DT | IDS), DT | IDS, state)
        ctx.scene_normals(None)
        never = dataclasses.replace(case.sh, attrs=case.a)
        against(K.expected_frame(oracle, case.shown["morphed"], case.i, IDENT, W, H, DT, shading=never), grab(ctx, DT), DT, "NULL on two bands")


# ---- 8: what never reads normals does not change -------------------------------------------------------------------------------------
@gpu
def test_item_bounds_depth_only_and_vertex_frames_are_unchanged(swr, case):
    items = [(0, 1500, IDENT), (1500, case.i.size - 1500, K.affine_matrix(0.3, 0.6, -0.35, 0.1))]
    with resident(swr, case.v, case.i, case.a, case.sh) as ctx:
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set(case.P)

        def look():
            return (ctx.item_bounds(items, DT).tobytes(), grab(ctx, DT | NC), grab(ctx, DT, VERTICES), grab(ctx, DT | IDS)[2])

        held = look()
        for mode, flip in MODES:
            ctx.scene_normals(mode, flip=flip)
            got = look()
            assert got[0] == held[0], "swr_item_bounds"
            same(got[1], held[1], "a depth-only frame")
            same(got[2], held[2], "a .vertices frame")
            assert np.array_equal(got[3], held[3]), "primitive IDs"
        ctx.material_set(None)
        passthrough = grab(ctx, DT)
        ctx.scene_normals(None)
        same(grab(ctx, DT), passthrough, "the passthrough shader")


# ---- 9: errors -------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("device_count", [0, 2])
def test_errors(swr, oracle, case, device_count):
    L = swr.load_library()
    B = swr.binding

    def call(ctx, mode, flags=0, r0=0, r1=0):
        return L.swr_scene_normals(ctx._h, ctypes.byref(B.Normals(mode, flags, (ctypes.c_int32 * 2)(r0, r1))))

    def refused(ctx):
        for args in ((3,), (-1,), (FLAT, 2), (SMOOTH, 0x80000001), (FLAT, 1, 1, 0), (SMOOTH, 0, 0, -1), (UPLOADED, 0, 7, 0)):
            assert call(ctx, *args) == BAD_ARG, args
        code, text = code_of(swr, lambda: ctx._check(call(ctx, 9)))
        assert code == BAD_ARG and "swr_scene_normals: unknown mode 9" in text, text
        assert L.swr_scene_normals(None, None) == BAD_ARG

    with swr.Context(0, device_count=device_count) as ctx:
        assert code_of(swr, lambda: ctx.scene_normals(SMOOTH))[0] == NO_SCENE
        assert code_of(swr, lambda: ctx.scene_normals(None))[0] == NO_SCENE
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        ctx.scene_attributes(case.a)
        ctx.material_set(B.Material.from_shading(case.sh))
        refused(ctx)
        against(want(oracle, case.sh, (case.v, case.a, case.i), DT), grab(ctx, DT), DT, "after the errors the normals are the uploaded ones")
        ctx.scene_normals("flat", flip=True)
        flat = want(oracle, case.sh, NM.expected_scene(FLAT, case.v, case.a, case.i, True), DT)
        against(flat, grab(ctx, DT), DT, "FLAT with FLIP")
        refused(ctx)
        against(flat, grab(ctx, DT), DT, "after the errors the mode and the scene are unchanged")
        ctx.scene_skin(case.joint, case.weight)
        ctx.pose_set(case.P)
        against(want(oracle, case.sh, NM.expected_scene(FLAT, case.shown["posed"], case.a, case.i, True), DT), grab(ctx, DT), DT, "the mode is still there")


@gpu
def test_failed_context_returns_its_sticky_error(swr, case):
    ctx = swr.Context(0, wait_budget_ms=300)
    try:
        ctx.scene_upload(case.v, case.i)
        ctx.target_set(W, H)
        ctx.scene_attributes(case.a)
        ctx.scene_normals(SMOOTH)
        ctx.debug_fault(swr.binding.FAULT_ENQUEUE)      # the next frame's raster share fails as if a launch had returned an error
        try:
            ctx.draw(IDENT, DT)
        except swr.SwrError as e:
            assert e.code == HIP
        assert code_of(swr, lambda: ctx.scene_normals(FLAT))[0] == HIP
        assert code_of(swr, lambda: ctx.scene_normals(None))[0] == HIP
        assert code_of(swr, lambda: ctx.scene_normals(7))[0] == HIP
    finally:
        ctx.close()


# ---- 10: the example -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["smooth", "flat"])
def test_the_example_computes_its_normals(swr, oracle, mode):
    """examples/frame_loop.py --morph --sparse --skin --auto-normals: the oracle's Phong frames of the morphed-then-posed torus with
    the model's normals, under the app's transform."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("frame_loop", os.path.join(ROOT, "examples", "frame_loop.py"))
    fl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fl)
    size, t0 = 128, 0.4
    v, i, frames = fl.run_morph(2, size, None, True, time0=t0, skin=True, sparse=True, auto_normals=mode)
    sh = fl.auto_normals_shading(v)
    T = swr.binding.sparse_targets(fl.morph_targets(v))
    joint, weight = fl.bend_skin(v)
    for k, (c, d) in enumerate(frames):
        t = t0 + k / 60.0
        mv = SM.pose_vertices(MS.morph_vertices(v, T, fl.morph_weights(t)), joint, weight, fl.bend_pose(t))
        ev, ea, ei = NM.expected_scene(NM.SMOOTH if mode == "smooth" else NM.FLAT, mv, sh.attrs, i)
        wc, wd = K.oracle_clear(oracle, ev, ei, swr.scenes.app_transform(t), size, size, DT, shading=dataclasses.replace(sh, attrs=ea))
        assert d.tobytes() == wd.tobytes() and np.array_equal(c, wc), f"frame {k}"
    assert not np.array_equal(frames[0][0], frames[1][0])


# ---- 11: every kernel swr_normals.hip launches has a GPU case above -------------------------------------------------------------------
GPU_CASES = {
    "k_face_normals<FLIP.value> FLIP=false": ("test_the_torus_in_every_state", "test_the_hub", "test_stream_orders", "test_call_orders"),
    "k_face_normals<FLIP.value> FLIP=true": ("test_the_torus_in_every_state", "test_the_hub", "test_two_bands"),
    "k_vertex_normals": ("test_the_torus_in_every_state", "test_the_hub", "test_an_upload_discards_the_mode"),
    "k_flat_normals<FLIP.value> FLIP=false": ("test_the_torus_in_every_state", "test_the_hub", "test_stream_orders", "test_call_orders"),
    "k_flat_normals<FLIP.value> FLIP=true": ("test_the_torus_in_every_state", "test_the_hub", "test_two_bands", "test_errors"),
}


def test_every_launched_kernel_has_a_gpu_case():
    src = open(SRC).read()
    code = re.sub(r"//[^\n]*", "", src)
    body = code[code.index("void launch_face_normals("):].replace(" ", "")
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(k_\w+(?:<[^>]*>)?)\)?,", body))
    assert launched == {"k_face_normals<FLIP.value>", "k_vertex_normals", "k_flat_normals<FLIP.value>"}, launched
    assert body.count("with_bools([&](autoFLIP)") == 2 and body.count("},flip);") == 2, "FLIP is lifted by with_bools"
    assert set(re.findall(r"__global__[^;{]*?(k_\w+)\(", code)) == {"k_face_normals", "k_vertex_normals", "k_flat_normals"}
    assert "gridDim" not in code and "std::min" not in code and "#define" not in code, "exact grids: no cap, no stride, no launch macro"
    assert body.count("if(ntri<=0)return;") == 2 and "if(nv<=0)return;" in body, "nothing to do: no launch (a zero grid is a launch error)"
    covered = {k.split(" ")[0] for k in GPU_CASES}
    assert launched == covered, f"no GPU case for {sorted(launched - covered)}"
    for variant, tests in GPU_CASES.items():
        for name in tests:
            fn = globals().get(name)
            assert fn is not None, (variant, name)
            assert any(m.name == "gpu" for m in getattr(fn, "pytestmark", [])), f"{name} is not a GPU test"
