"""The boundary of the morph targets (include/swr.h "Morph targets"): the symbols, the layout of swr_morph_targets, the target limit
and the header's normative text.  CPU only; the error codes that need a device are in tests/test_morph.py."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
SYMBOLS = ("swr_scene_morph", "swr_morph_set")


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def test_symbols_and_struct(swr):
    L = swr.load_library()
    B = swr.binding
    for name in SYMBOLS:
        assert hasattr(L, name) and name in B.ABI_SYMBOLS, name
    assert ctypes.sizeof(B.MorphTargets) == 32
    assert [(f, getattr(B.MorphTargets, f).offset, getattr(B.MorphTargets, f).size) for f, _ in B.MorphTargets._fields_] == [
        ("position_deltas", 0, 8), ("normal_deltas", 8, 8), ("vertex_count", 16, 8), ("target_count", 24, 4), ("reserved", 28, 4)]
    assert B.MORPH_MAX_TARGETS == 256
    assert L.swr_abi_version() == 6
    assert callable(B.Context.scene_morph) and callable(B.Context.morph_set)


def test_header_text():
    h = header()
    assert re.search(r"typedef struct swr_morph_targets \{\s*const float\* position_deltas;[^}]*const float\* normal_deltas;[^}]*"
                     r"int64_t vertex_count;[^}]*int32_t target_count;[^}]*int32_t reserved;[^}]*\} swr_morph_targets;\s*/\* 32 bytes \*/", h)
    assert re.search(r"#define SWR_MORPH_MAX_TARGETS 256\b", h)
    assert re.search(r"int\s+swr_scene_morph\(swr_context\*\s*\w*,\s*const swr_morph_targets\*\s*\w*\);", h)
    assert re.search(r"int\s+swr_morph_set\(swr_context\*\s*\w*,\s*const float\*\s*\w*,\s*int32_t\s*\w*\);", h)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    assert h.index("---- Skinned meshes (swr_scene_skin, swr_pose_set)") \
        < h.index("---- Morph targets (swr_scene_morph, swr_morph_set) — DESIGN.md §24") < h.index("---- Load frames"), \
        "between 'Skinned meshes' and 'Load frames'"
    section = h[h.index("---- Morph targets"):h.index("---- Load frames")]
    flat = re.sub(r"\s*\n \*\s*", " ", section)         # the comment's lines joined
    for text in ("the presence of the swr_morph_set symbol is the feature test",
                 "IEEE binary32, one rounding per operation, no FMA",
                 "the base position is b, exactly as uploaded",
                 "Start with p = b.",
                 "Walk t in ascending order.",
                 "For every t with w[t] != 0.0f (float compare), p = p + w[t] * d[t][i], componentwise: the product is rounded, then the sum is rounded.",
                 "A target whose weight is +0 or -0 is skipped and its deltas are not read",
                 "a NaN or infinite delta in a zero-weight target changes nothing",
                 "A NaN weight compares unequal to 0 and is applied.",
                 "The skip is normative",
                 "Normals take the same loop with normal_deltas, only when the scene has attributes and normal_deltas was given",
                 "otherwise normals stay as uploaded",
                 "Normal deltas given before swr_scene_attributes arrives are kept and take effect when it does.",
                 "Colour, uv and the padding lanes never change.",
                 "Morph first, then skin",
                 "the position and normal that the \"Skinned meshes\" arithmetic reads are the morphed ones",
                 "Without a skin or a pose, the morphed vertices are the scene.",
                 "bit for bit that of a context on which swr_scene_upload (and swr_scene_attributes) was given the morphed-then-posed vertices",
                 "every entry point, flag, rule set, draw list and primitive type",
                 "Primitive IDs, painter's order and tie order keep the numbering of the index array",
                 "When all weights are zero, the scene is bit for bit what the upload built, or what the current pose alone built.",
                 "It copies the deltas: the caller's arrays are free on return.",
                 "New targets set every weight to 0; they keep the skin and the pose, which is re-applied to the unmorphed base.",
                 "targets == NULL removes the targets.",
                 "(the one a swr_render performs included) discards targets and weights",
                 "swr_morph_set persists until the next swr_morph_set, swr_scene_morph or swr_scene_upload.",
                 "swr_pose_set and swr_scene_skin keep the weights: the new pose is applied to the morphed vertices.",
                 "first complete and check everything drawn before, exactly as swr_pose_set does",
                 "an overflowed last frame is repaired in the shape it was drawn in",
                 "A multi-device context morphs every band.",
                 "SWR_ERR_NO_SCENE: no scene.",
                 "a NULL ctx; a vertex_count that does not match the scene; NULL position_deltas; target_count < 1; a non-zero reserved; "
                 "swr_morph_set without targets; weight_count not equal to the target count (except NULL with 0); NULL weights with a positive count.",
                 "SWR_ERR_UNSUPPORTED: target_count > SWR_MORPH_MAX_TARGETS.",
                 "SWR_ERR_NOMEM: the delta buffer cannot be allocated.",
                 "A failed context returns its sticky error.",
                 "After an error the scene, the targets and the weights are unchanged.",
                 "Not covered: sparse targets, morphing colours or uv, one call that sets weights and joints together",
                 "an un-waited morph, and the C++ and Swift mirrors"):
        assert text in flat, text
    skin = h[h.index("---- Skinned meshes"):h.index("---- Morph targets")]
    assert "morph targets" not in skin[skin.index("Not covered"):], "the skin's 'Not covered' line no longer names them"


def test_null_context_is_refused(swr):
    L = swr.load_library()
    B = swr.binding
    d = np.zeros((1, 4, 3), dtype=np.float32)
    w = np.zeros(1, dtype=np.float32)
    t = B.MorphTargets(d.ctypes.data, None, 4, 1, 0)
    assert L.swr_scene_morph(None, ctypes.byref(t)) == BAD_ARG
    assert L.swr_scene_morph(None, None) == BAD_ARG
    assert L.swr_morph_set(None, w.ctypes.data, 1) == BAD_ARG
    assert L.swr_morph_set(None, None, 0) == BAD_ARG
