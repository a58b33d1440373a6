"""The boundary of the skinned meshes (include/swr.h "Skinned meshes"): the symbols, the layout of swr_skin_vertex, the joint limit
and the header's normative text.  CPU only; the error codes that need a device are in tests/test_skin.py."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
SYMBOLS = ("swr_scene_skin", "swr_pose_set")


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def test_symbols_and_struct(swr):
    L = swr.load_library()
    B = swr.binding
    for name in SYMBOLS:
        assert hasattr(L, name) and name in B.ABI_SYMBOLS, name
    assert ctypes.sizeof(B.SkinVertex) == 32
    assert [(f, getattr(B.SkinVertex, f).offset, getattr(B.SkinVertex, f).size) for f, _ in B.SkinVertex._fields_] == [
        ("joint", 0, 16), ("weight", 16, 16)]
    assert B.SKIN_VERTEX_DTYPE.itemsize == 32 and B.SKIN_VERTEX_DTYPE.fields["weight"][1] == 16
    assert B.SKIN_VERTEX_DTYPE["joint"].base == np.uint32 and B.SKIN_VERTEX_DTYPE["weight"].base == np.float32
    assert B.SKIN_MAX_JOINTS == 1024
    assert L.swr_abi_version() == 6


def test_header_text():
    h = header()
    assert re.search(r"typedef struct swr_skin_vertex \{\s*uint32_t joint\[4\];[^}]*float\s+weight\[4\];[^}]*\} swr_skin_vertex;\s*"
                     r"/\* 32 bytes, parallel to swr_vertex", h)
    assert re.search(r"#define SWR_SKIN_MAX_JOINTS 1024\b", h)
    assert re.search(r"int\s+swr_scene_skin\(swr_context\*\s*\w*,\s*const swr_skin_vertex\*\s*\w*,\s*int64_t\s*\w*\);", h)
    assert re.search(r"int\s+swr_pose_set\(swr_context\*\s*\w*,\s*const float\*\s*\w*\s*(/\*[^*]*\*/)?,\s*int32_t\s*\w*\);", h)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new flag bit"
    assert h.index("---- Delta reads") < h.index("---- Skinned meshes (swr_scene_skin, swr_pose_set) — DESIGN.md §23") \
        < h.index("---- Load frames"), "between 'Delta reads' and 'Load frames'"
    for text in ("the presence of the swr_pose_set symbol is the feature test",
                 "a new swr_scene_upload (the one a swr_render performs included) discards skin and pose",
                 "joints == NULL with joint_count == 0 restores the bind pose: the scene is bit for bit what the upload built",
                 "IEEE binary32, one rounding per operation, no FMA",
                 "r_k = c0.xyz * x;   r_k = r_k + c1.xyz * y;   r_k = r_k + c2.xyz * z;   r_k = r_k + c3.xyz * 1.0f;",
                 "acc = weight[0] * r_0;   acc = acc + weight[1] * r_1;   acc = acc + weight[2] * r_2;   acc = acc + weight[3] * r_3;",
                 "The fourth row of a joint matrix is ignored",
                 "no inverse transpose and no renormalisation",
                 "Colour and uv never\n *     change",
                 "all four influences are always read",
                 "bit for bit that of a context on which swr_scene_upload",
                 "Primitive IDs, painter's order and tie order keep the numbering of the index array",
                 "A frame posted before the call never sees the new pose",
                 "A multi-device context poses every band",
                 "joint_count <= the largest joint index the skin uses",
                 "SWR_ERR_UNSUPPORTED: joint_count > SWR_SKIN_MAX_JOINTS",
                 "After an error the\n *     scene and the pose are unchanged"):
        assert text in h, text


def test_null_context_is_refused(swr):
    L = swr.load_library()
    sk = np.zeros(4, dtype=swr.binding.SKIN_VERTEX_DTYPE)
    m = np.zeros(16, dtype=np.float32)
    assert L.swr_scene_skin(None, sk.ctypes.data, 4) == BAD_ARG
    assert L.swr_scene_skin(None, None, 0) == BAD_ARG
    assert L.swr_pose_set(None, m.ctypes.data, 1) == BAD_ARG
    assert L.swr_pose_set(None, None, 0) == BAD_ARG
