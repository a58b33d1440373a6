"""The boundary of the computed normals (include/swr.h "Computed normals"): the symbol, the layout of swr_normals, the enum values,
the binding's method, the header's normative text and the documents' sections.  CPU only; the error codes that need a device are in
tests/test_normals.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
TITLE = "---- Computed normals (swr_scene_normals) — DESIGN.md §29"


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def flat(section):
    return re.sub(r"\s*\n \*\s*", " ", section)         # the comment's lines joined


def test_symbol_struct_and_binding(swr):
    L = swr.load_library()
    B = swr.binding
    assert hasattr(L, "swr_scene_normals") and B.ABI_SYMBOLS.count("swr_scene_normals") == 1
    assert ctypes.sizeof(B.Normals) == 16
    assert [(f, getattr(B.Normals, f).offset, getattr(B.Normals, f).size) for f, _ in B.Normals._fields_] == [
        ("mode", 0, 4), ("flags", 4, 4), ("reserved", 8, 8)]
    assert (B.NORMALS_UPLOADED, B.NORMALS_SMOOTH, B.NORMALS_FLAT, B.NORMALS_FLIP) == (0, 1, 2, 1)
    assert B.NORMALS_MODES == {"uploaded": 0, "smooth": 1, "flat": 2}
    assert L.swr_abi_version() == 6
    assert callable(B.Context.scene_normals)
    assert L.swr_scene_normals(None, None) == BAD_ARG
    assert L.swr_scene_normals(None, ctypes.byref(B.Normals(1, 0, (ctypes.c_int32 * 2)(0, 0)))) == BAD_ARG


def test_the_library_exports_the_symbol(swr):
    swr.build()
    assert hasattr(ctypes.CDLL(swr.library_path()), "swr_scene_normals")
    api = read("software-renderer_amd", "csrc", "swr_api.hip")
    assert "sizeof(swr_normals) == 16" in api, "the layout is asserted where the library is compiled"


def test_header_text():
    h = read("include", "swr.h")
    assert re.search(r"enum \{ SWR_NORMALS_UPLOADED = 0, SWR_NORMALS_SMOOTH = 1, SWR_NORMALS_FLAT = 2 \};", h)
    assert re.search(r"enum \{ SWR_NORMALS_FLIP = 1u << 0 \};", h)
    assert re.search(r"typedef struct swr_normals \{\s*int32_t\s+mode;[^}]*uint32_t\s+flags;[^}]*int32_t\s+reserved\[2\];[^}]*\} swr_normals;\s*/\* 16 bytes \*/", h)
    assert re.search(r"int\s+swr_scene_normals\(swr_context\*\s*\w*,\s*const swr_normals\*\s*\w*\);\s*/\* NULL: SWR_NORMALS_UPLOADED \*/", h)
    assert h.index("int swr_morph_pose_set(") < h.index("int swr_scene_normals(") < h.index("int swr_material_set(")
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert h.index("---- Weights and joints in one call") < h.index(TITLE) < h.index("---- Load frames")
    s = flat(h[h.index(TITLE):h.index("---- Load frames")])
    for text in ("the presence of the swr_scene_normals symbol is the feature test",
                 "normals == NULL means SWR_NORMALS_UPLOADED",
                 "the morphed-then-posed xyz of indices[3p], indices[3p + 1] and indices[3p + 2]",
                 "p runs over 0 .. index_count / 3 - 1; trailing indices are ignored",
                 "The normals are in object space, like light_dir: the frame's transform is not involved.",
                 "IEEE binary32, one rounding per operation, no FMA",
                 "e1 = b - a and e2 = c - a",
                 "f_p = cross(e1, e2), with cross exactly as \"Dual-quaternion skinning\" defines it: two products and one subtraction per component",
                 "Under SWR_NORMALS_FLIP, f_p = cross(e2, e1).",
                 "All three corners of triangle p take the normal f_p.  It is not normalised: the fragment stage normalises per pixel.",
                 "This is what glTF prescribes for a mesh without normals.",
                 "For vertex i start with n = (+0, +0, +0).",
                 "Walk p in ascending order, and inside p the corners k = 0, 1, 2.",
                 "For every corner with indices[3p + k] == i, n = n + f_p, componentwise: a triangle that names i twice adds twice.",
                 "l = sqrtf((n.x*n.x + n.y*n.y) + n.z*n.z), with sqrtf and the divide correctly rounded",
                 "If l > 0.0f, n = n * (1.0f / l): one divide, three multiplies.",
                 "a vertex of no triangle stays (0, 0, 0)",
                 "a NaN l leaves n as the sum made it",
                 "Every corner that references i takes n.",
                 "The walk order is normative: it is what makes the sum bit-defined.",
                 "a non-finite position poisons the faces that use it and the vertices of those faces, and nothing else",
                 "Colour, uv, the padding lanes, positions, group boxes and the uploaded attribute array are never written.",
                 "morph normal_deltas and the normal half of either skinning mode have no effect on any frame",
                 "swr_scene_upload got the morphed-then-posed vertices and swr_scene_attributes got the same uv with the n_i above",
                 "it is that of the de-indexed scene: vertex 3p + k is corner k of triangle p, the indices are 0 .. 3 * ntri - 1, and each corner carries f_p",
                 "Primitive IDs, painter's order and tie order are unchanged.",
                 ".vertices and .line frames and the passthrough shader never read normals and do not change.",
                 "it may be set before or after swr_scene_attributes, swr_scene_skin and swr_scene_morph[_sparse]",
                 "It takes effect only while the scene has attributes: set earlier, it is kept and takes effect when swr_scene_attributes arrives",
                 "It persists across swr_pose_set, swr_pose_set_dq, swr_morph_set, swr_morph_pose_set, swr_scene_skin, swr_scene_morph and swr_scene_morph_sparse",
                 "the normals are recomputed whenever one of them rewrites the scene",
                 "SWR_NORMALS_UPLOADED (or NULL) restores the uploaded normals, morphed and posed as before",
                 "A new swr_scene_upload (the one a swr_render performs included) discards the mode.",
                 "everything drawn before is completed and checked first, the call is blocking",
                 "a multi-device context recomputes on every band",
                 "Errors, all checked before anything changes.",
                 "SWR_ERR_NO_SCENE: no scene.",
                 "SWR_ERR_BAD_ARG: a NULL ctx; an unknown mode; unknown flag bits; a non-zero reserved word.",
                 "SWR_ERR_UNSUPPORTED: SWR_NORMALS_SMOOTH on a scene with 2^32 or more indices.",
                 "SWR_ERR_NOMEM: a device allocation fails.",
                 "A failed context returns its sticky error.",
                 "After an error the mode and the scene are unchanged.",
                 "Not covered: angle-weighted normals, crease angles and smoothing groups, tangents, swr_render passes (which have no field for the mode), "
                 "an un-waited call, and the C++ and Swift mirrors."):
        assert text in s, text
    # the sections this one closes point to it
    skin = flat(h[h.index("---- Skinned meshes"):h.index("---- Dual-quaternion skinning")])
    morph = flat(h[h.index("---- Morph targets"):h.index("---- Item bounds")])
    assert "\"Computed normals\"" in skin[skin.index("Not covered"):] and "\"Computed normals\"" in morph[morph.index("Not covered"):]


def test_the_documents_have_their_sections():
    design, integration, readme = read("DESIGN.md"), read("INTEGRATION.md"), read("README.md")
    assert re.search(r"^## 29\. Computed normals", design, flags=re.M)
    section = design[design.index("## 29. Computed normals"):]
    for word in ("k_face_normals", "k_vertex_normals", "k_flat_normals", "adjacency", "profiles/normals/kernel.txt", "profiles/normals/bench_ab.txt",
                 "profiles/normals/vgprs.txt"):
        assert word in section, word
    assert re.search(r"^\*\*\(s\) ", integration, flags=re.M) and "swr_scene_normals" in integration[integration.index("**(s) "):]
    assert integration.index("**(r) ") < integration.index("**(s) ") < integration.index("## 5. ")
    assert "swr_scene_normals" in readme and "--auto-normals" in readme


def test_the_header_and_the_model_say_the_same_thing():
    """The operations the model spells are the header's: the same grouping of the squared length, the same compare, the same product."""
    model = read("tests", "normals_model.py")
    assert "(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]" in model
    assert "ok = l > np.float32(0.0)" in model and "np.float32(1.0) / l[ok]" in model and "n[ok] * inv[:, None]" in model
    assert "cross(e2, e1) if flip else cross(e1, e2)" in model
    assert "a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]" in model and "a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]" in model and "a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]" in model
    assert 'np.argsort(c, kind="stable")' in model, "ascending by corner number, duplicates kept"
