"""The boundary of the sparse morph targets and of the combined call (include/swr.h "Sparse morph targets", "Weights and joints in one
call"): the symbols, the layouts of swr_morph_sparse_target and swr_morph_sparse, and the header's normative text.  CPU only; the
error codes that need a device are in tests/test_morph_sparse.py."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
SYMBOLS = ("swr_scene_morph_sparse", "swr_morph_pose_set")
TITLE = "---- Sparse morph targets (swr_scene_morph_sparse) — DESIGN.md §28"
TITLE2 = "---- Weights and joints in one call (swr_morph_pose_set) — DESIGN.md §28"


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def flat(section):
    return re.sub(r"\s*\n \*\s*", " ", section)         # the comment's lines joined


def test_symbols_and_structs(swr):
    L = swr.load_library()
    B = swr.binding
    for name in SYMBOLS:
        assert hasattr(L, name) and name in B.ABI_SYMBOLS, name
    assert ctypes.sizeof(B.MorphSparseTarget) == 32 and ctypes.sizeof(B.MorphSparse) == 24
    assert [(f, getattr(B.MorphSparseTarget, f).offset, getattr(B.MorphSparseTarget, f).size) for f, _ in B.MorphSparseTarget._fields_] == [
        ("indices", 0, 8), ("position_deltas", 8, 8), ("normal_deltas", 16, 8), ("count", 24, 8)]
    assert [(f, getattr(B.MorphSparse, f).offset, getattr(B.MorphSparse, f).size) for f, _ in B.MorphSparse._fields_] == [
        ("targets", 0, 8), ("vertex_count", 8, 8), ("target_count", 16, 4), ("reserved", 20, 4)]
    assert (B.POSE_MATRICES, B.POSE_DUAL_QUATS) == (0, 1) and B.MORPH_MAX_TARGETS == 256
    assert L.swr_abi_version() == 6
    assert callable(B.Context.scene_morph_sparse) and callable(B.Context.morph_pose_set) and callable(B.sparse_targets)


def test_header_text():
    h = header()
    assert re.search(r"typedef struct swr_morph_sparse_target \{\s*const uint32_t\* indices;[^}]*const float\*\s+position_deltas;[^}]*"
                     r"const float\*\s+normal_deltas;[^}]*int64_t\s+count;[^}]*\} swr_morph_sparse_target;\s*/\* 32 bytes \*/", h)
    assert re.search(r"typedef struct swr_morph_sparse \{\s*const swr_morph_sparse_target\* targets;[^}]*int64_t vertex_count;[^}]*"
                     r"int32_t target_count;[^}]*int32_t reserved;[^}]*\} swr_morph_sparse;\s*/\* 24 bytes \*/", h)
    assert re.search(r"enum \{ SWR_POSE_MATRICES = 0, SWR_POSE_DUAL_QUATS = 1 \};", h)
    assert re.search(r"int\s+swr_scene_morph_sparse\(swr_context\*\s*\w*,\s*const swr_morph_sparse\*\s*\w*\);", h)
    assert re.search(r"int\s+swr_morph_pose_set\(swr_context\*\s*\w*,\s*const float\*\s*\w*,\s*int32_t\s*\w*,\s*const float\*\s*\w*,\s*"
                     r"int32_t\s*\w*,\s*int32_t\s*\w*\);", h)
    assert h.index("int swr_morph_set(") < h.index("int swr_scene_morph_sparse(") < h.index("int swr_morph_pose_set(") < h.index("int swr_material_set(")
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    assert h.index("---- Morph targets") < h.index("---- Item bounds") < h.index(TITLE) < h.index(TITLE2) < h.index("---- Load frames")
    s = flat(h[h.index(TITLE):h.index(TITLE2)])
    for text in ("the presence of the swr_scene_morph_sparse symbol is the feature test",
                 "This section covers the \"sparse targets\" that the \"Not covered\" line of \"Morph targets\" names",
                 "The targets in effect are those of the last swr_scene_morph or swr_scene_morph_sparse.",
                 "Either call with NULL removes whichever kind is resident.",
                 "swr_morph_set serves both kinds: one weight per target, the same errors.",
                 "IEEE binary32, one rounding per operation, no FMA",
                 "start with p = b, the position as uploaded",
                 "Walk t in ascending order.",
                 "For every t with w[t] != 0.0f whose index list contains i at position j, p = p + w[t] * d_t[j], componentwise: "
                 "the product is rounded, then the sum.",
                 "A vertex a target does not list is not touched by that target.",
                 "This is not the dense target with a zero delta",
                 "an unlisted -0 coordinate stays -0 where an applied zero delta makes it +0",
                 "a NaN or infinite weight poisons only the listed vertices",
                 "A zero-weight target's deltas never enter the arithmetic; the device may still read them.",
                 "Normals take the same loop with normal_deltas",
                 "Either every target with count > 0 gives normal_deltas or none does.",
                 "Colour, uv and the padding lanes never change.",
                 "bit for bit that of a context that uploaded the morphed-then-posed vertices",
                 "Lifetime, Ordering and \"Order with the skin\" of \"Morph targets\" apply unchanged",
                 "new targets set every weight to 0 and keep skin and pose",
                 "an upload discards targets and weights",
                 "the arrays are copied and free on return",
                 "a multi-device context morphs every band",
                 "Errors, all checked before anything changes.",
                 "SWR_ERR_NO_SCENE: no scene.",
                 "a NULL ctx; a vertex_count that does not match the scene; a NULL targets array; target_count < 1; a non-zero reserved; "
                 "count < 0 or count > vertex_count; NULL indices or position_deltas with count > 0; an index >= vertex_count, or indices "
                 "not strictly ascending (the message names the target and the position); normal deltas on some non-empty targets only.",
                 "SWR_ERR_UNSUPPORTED: target_count > SWR_MORPH_MAX_TARGETS.",
                 "SWR_ERR_NOMEM: a device allocation fails.",
                 "A failed context returns its sticky error.",
                 "After an error the scene, the targets of either kind and the weights are unchanged."):
        assert text in s, text
    s2 = flat(h[h.index(TITLE2):h.index("---- Load frames")])
    for text in ("the presence of the swr_morph_pose_set symbol is the feature test",
                 "This section covers the \"one call that sets weights and joints together\"",
                 "The call is exactly swr_morph_set(weights, weight_count) followed by swr_pose_set (pose_kind SWR_POSE_MATRICES) or "
                 "swr_pose_set_dq (SWR_POSE_DUAL_QUATS) with joints, joint_count",
                 "Every argument of both halves is validated before anything changes: after an error neither the weights nor the pose have changed.",
                 "the skin and stream passes run once, and the call waits once",
                 "It needs targets (of either kind) and a skin.",
                 "NULL weights with 0 and NULL joints with 0 mean what they mean in the two calls.",
                 "SWR_ERR_BAD_ARG for an unknown pose_kind"):
        assert text in s2, text


def test_null_context_is_refused(swr):
    L = swr.load_library()
    B = swr.binding
    idx = np.arange(2, dtype=np.uint32)
    d = np.zeros((2, 3), dtype=np.float32)
    t = (B.MorphSparseTarget * 1)(B.MorphSparseTarget(idx.ctypes.data, d.ctypes.data, None, 2))
    s = B.MorphSparse(t, 4, 1, 0)
    w = np.zeros(1, dtype=np.float32)
    j = np.zeros(16, dtype=np.float32)
    assert L.swr_scene_morph_sparse(None, ctypes.byref(s)) == BAD_ARG
    assert L.swr_scene_morph_sparse(None, None) == BAD_ARG
    assert L.swr_morph_pose_set(None, w.ctypes.data, 1, j.ctypes.data, 1, 0) == BAD_ARG
    assert L.swr_morph_pose_set(None, None, 0, None, 0, 1) == BAD_ARG
