"""The boundary of the dual-quaternion skinning (include/swr.h "Dual-quaternion skinning"): the symbol, the prototype, the section's
place and its normative text.  CPU only; the error codes that need a device are in tests/test_skin_dq.py."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
TITLE = "---- Dual-quaternion skinning (swr_pose_set_dq) — DESIGN.md §26"


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def section():
    h = header()
    return h[h.index(TITLE):h.index("---- Morph targets")]


def test_symbol(swr):
    L = swr.load_library()
    B = swr.binding
    assert hasattr(L, "swr_pose_set_dq") and "swr_pose_set_dq" in B.ABI_SYMBOLS
    assert B.ABI_SYMBOLS.count("swr_pose_set_dq") == 1
    assert L.swr_abi_version() == 6
    assert callable(B.dual_quats) and callable(B.Context.pose_set_dq)


def test_prototype_text():
    h = header()
    assert re.search(r"/\* joint_count x 8 floats: per joint the real quaternion \(x, y, z, w\), then the dual quaternion \(x, y, z, w\); "
                     r"w is the scalar part \*/\s*"
                     r"int\s+swr_pose_set_dq\(swr_context\*\s*ctx,\s*const float\*\s*dual_quats,\s*int32_t\s*joint_count\);", h)
    assert h.index("int swr_pose_set(") < h.index("int swr_pose_set_dq(") < h.index("int swr_scene_morph(")
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    assert h.count("#define SWR_SKIN_MAX_JOINTS") == 1, "the limit of the one pose state"


def test_section_place_and_text():
    h = header()
    assert h.count(TITLE) == 1
    assert h.index("---- Skinned meshes (swr_scene_skin, swr_pose_set) — DESIGN.md §23") < h.index("#define SWR_SKIN_MAX_JOINTS 1024") \
        < h.index(TITLE) < h.index("---- Morph targets (swr_scene_morph, swr_morph_set) — DESIGN.md §24"), "directly after 'Skinned meshes'"
    between = h[h.index("#define SWR_SKIN_MAX_JOINTS 1024"):h.index(TITLE)]
    assert between.split() == ["#define", "SWR_SKIN_MAX_JOINTS", "1024", "/*"], "nothing between the two sections"
    s = section()
    for text in ("No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_pose_set_dq symbol is the feature test",
                 "Nothing\n * existing changes",
                 "per joint the real quaternion (x, y, z, w), then the dual quaternion (x, y, z, w); w is\n *     the scalar part",
                 "It is the pose state of \"Skinned meshes\": the skin of swr_scene_skin, the limit SWR_SKIN_MAX_JOINTS, one pose in\n *     effect",
                 "The pose in effect is that of the last call of either kind",
                 "swr_pose_set_dq(ctx, NULL, 0) and swr_pose_set(ctx, NULL, 0) both restore the bind pose",
                 "Carried over from \"Skinned meshes\", by reference",
                 "a frame posted before the call never sees the new pose",
                 "a multi-device context poses every band",
                 "a new swr_scene_skin or swr_scene_upload discards the pose",
                 "morph first, then skin",
                 "its Errors paragraph, with swr_pose_set_dq in the messages",
                 "A failed context returns its sticky error",
                 "After an\n *     error the scene and the pose are unchanged",
                 "IEEE binary32, one rounding per operation, no FMA; sqrtf and / are correctly rounded",
                 "s_k = ((R_0.x*R_k.x + R_0.y*R_k.y) + R_0.z*R_k.z) + R_0.w*R_k.w",
                 "u_k = s_k < 0.0f ? -weight[k] : weight[k]",
                 "A NaN or zero s_k keeps the weight",
                 "B = u_0*Q_0;   B = B + u_1*Q_1;   B = B + u_2*Q_2;   B = B + u_3*Q_3",
                 "n = ((B.x*B.x + B.y*B.y) + B.z*B.z) + B.w*B.w over the real part;  l = sqrtf(n);  i = 1.0f / l;  C = B * i",
                 "The dual part is not made orthogonal to the real part",
                 "cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)",
                 "a = cross(q, x);   b = a + w*x;   c = cross(q, b);   rot(x) = x + 2.0f*c",
                 "e = cross(q, d);   t = 2.0f * ((w*d - dw*q) + e)",
                 "The posed position is rot(v) + t",
                 "are rot(n): no translation, no renormalisation",
                 "Colour, uv and the padding lanes never change",
                 "all four influences are always read",
                 "(l == 0) gives non-finite coordinates and the triangle is skipped exactly as an uploaded one",
                 "the payload of a NaN result is unspecified",
                 "does not normalise its input and does not check that it is a unit dual quaternion",
                 "A non-unit real\n *     part scales nothing",
                 "A joint with scale or shear cannot be expressed as a\n *     dual quaternion: use swr_pose_set for those",
                 "bit for bit that of a context on\n *     which swr_scene_upload"):
        assert text in s, text
    # by reference and not by copy: the section does not restate the ordering and error paragraphs of "Skinned meshes"
    assert "SWR_ERR_NO_SCENE" not in s and "an overflowed last frame is" not in s
    # "Skinned meshes" no longer lists the mode as missing
    skinned = h[h.index("---- Skinned meshes"):h.index(TITLE)]
    assert "Not covered: a pose that does not wait" in skinned and "dual-quaternion skinning, a partial" not in skinned


def test_null_context_is_refused(swr):
    L = swr.load_library()
    q = np.zeros(8, dtype=np.float32)
    assert L.swr_pose_set_dq(None, q.ctypes.data, 1) == BAD_ARG
    assert L.swr_pose_set_dq(None, None, 0) == BAD_ARG
