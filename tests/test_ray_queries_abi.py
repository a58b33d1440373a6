"""The boundary of the ray queries (include/swr.h "Ray queries"): the symbol, the layout of swr_ray_query, the flag values and
SWR_RAY_OCCLUDED, the section's place in the header and the normative sentences tests/ray_query_model.py rests on.  CPU only; the error
codes that need a device are in tests/test_ray_queries.py."""
import ctypes
import os
import re

import numpy as np

import ray_query_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
QUERY_LAYOUT = [("flags", 0), ("reserved", 4), ("first_primitive", 8), ("primitive_count", 16)]


def header():
    return open(os.path.join(ROOT, "include", "swr.h")).read()


def test_symbol_struct_and_constants(swr):
    L = swr.load_library()
    B = swr.binding
    assert hasattr(L, "swr_query_rays") and B.ABI_SYMBOLS.count("swr_query_rays") == 1
    assert hasattr(L, "swr_cast_rays") and "swr_cast_rays" in B.ABI_SYMBOLS
    assert B.RAY_QUERY_DTYPE.itemsize == 24
    assert [(f, B.RAY_QUERY_DTYPE.fields[f][1]) for f in B.RAY_QUERY_DTYPE.names] == QUERY_LAYOUT
    assert B.RAY_QUERY_DTYPE == M.QUERY_DTYPE
    assert [B.RAY_QUERY_DTYPE.fields[f][0] for f in B.RAY_QUERY_DTYPE.names] == [np.uint32, np.uint32, np.int64, np.int64]
    assert (B.RAYS_ANY_HIT, B.RAYS_CULL_BACK, B.RAYS_CULL_FRONT, B.RAYS_FRONT_CW) == (1, 2, 4, 8) == (M.ANY_HIT, M.CULL_BACK, M.CULL_FRONT, M.FRONT_CW)
    assert B.RAY_OCCLUDED == M.OCCLUDED == 0xFFFFFFFE and B.ID_NONE == M.ID_NONE == 0xFFFFFFFF
    assert B.RAYS_CULL == {None: 0, "none": 0, "back": 2, "front": 4, "both": 6}
    assert L.swr_query_rays.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert L.swr_abi_version() == 6
    assert callable(swr.Context.query_rays)


def test_header_declarations():
    h = header()
    assert re.search(r"enum \{ SWR_RAYS_ANY_HIT = 1u << 0, SWR_RAYS_CULL_BACK = 1u << 1, SWR_RAYS_CULL_FRONT = 1u << 2, "
                     r"SWR_RAYS_FRONT_CW = 1u << 3 \};", h)
    assert re.search(r"#define SWR_RAY_OCCLUDED 0xFFFFFFFEu\b", h) and re.search(r"#define SWR_ID_NONE 0xFFFFFFFFu\b", h)
    assert re.search(r"typedef struct swr_ray_query \{\s*uint32_t flags;[^;}]*\s*uint32_t reserved;[^;}]*\s*int64_t\s+first_primitive;[^;}]*"
                     r"\s*int64_t\s+primitive_count;[^;}]*\} swr_ray_query;\s*/\* 24 bytes \*/", h)
    assert re.search(r"int\s+swr_query_rays\(swr_context\*\s*\w*,\s*const swr_ray_query\*\s*\w*[^,]*,\s*const swr_ray\*\s*\w*,\s*int64_t\s*\w*,\s*"
                     r"swr_ray_hit\*\s*\w*\);", h)
    assert re.search(r"#define SWR_ABI_VERSION 6\b", h)
    assert not re.search(r"1u\s*<<\s*9\b", h) and not re.search(r"1u\s*<<\s*13\b", h), "no new draw-flag bit"
    # the section sits behind "Ray casts", its structs and SWR_RAYS_MAX, and in front of "Load frames"; the function behind swr_cast_rays
    assert h.index("---- Ray casts") < h.index("} swr_ray_hit;") < h.index("#define SWR_RAYS_MAX") < h.index("---- Ray queries")
    assert h.index("---- Ray queries") < h.index("} swr_ray_query;") < h.index("---- Load frames")
    at = h.index("int swr_cast_rays(")
    rest = h[h.index("\n", at) + 1:]
    assert re.match(r"(/\*[^\n]*\*/\n)?int swr_query_rays\(", rest), "declared directly after swr_cast_rays"
    # swr_cast_rays is as it was
    assert "int swr_cast_rays(swr_context* ctx, const swr_ray* rays, int64_t n, uint32_t flags /* 0 */, swr_ray_hit* hits);" in h


def test_header_text():
    h = header()
    section = h[h.index("---- Ray queries"):h.index("---- Load frames")]
    for text in ("the presence of the swr_query_rays symbol is the feature test",
                 "swr_cast_rays still refuses every non-zero flags",
                 "query == NULL means all defaults",
                 "flags 0, first_primitive 0, primitive_count -1",
                 "IEEE binary32, one rounding per operation, no FMA",
                 "steps 1 to 3",
                 "State, Ordering and Errors paragraphs hold with\n *     swr_query_rays in the messages; a refused ray is named by its index",
                 "n == 0 succeeds.  A scene without triangles answers every\n *     ray with a miss.",
                 "Only triangles p with first_primitive <= p < first_primitive + primitive_count are candidates",
                 "the range runs to index_count / 3",
                 "stay in the numbering of the whole index array, as for primitive\n *     IDs",
                 "An empty range is legal and answers every ray with a miss",
                 "For draw item k the range is first_index / 3,\n *     index_count / 3",
                 "det of step 3 decides",
                 "front-facing for the ray iff det > 0.0f",
                 "from the side cross(b - a, c - a) points to",
                 "a, b, c run counter-clockwise in a right-handed space",
                 "With SWR_RAYS_FRONT_CW front-facing is det < 0.0f",
                 "SWR_RAYS_CULL_BACK rejects the triangles that are not front-facing, SWR_RAYS_CULL_FRONT rejects the front-facing ones",
                 'directly after "Reject unless fabsf(det) > 0.0f", on the same det bits',
                 "Both bits reject everything",
                 'not the screen winding of "Face culling"',
                 "The hit record has no room for the facing: a caller\n *     learns it by culling",
                 'Step 4 of "Ray casts" over the triangles that survive range and cull',
                 "hits is bit for bit what swr_cast_rays writes",
                 "hits[k] is {SWR_RAY_OCCLUDED, 0, 0, 0} iff at least one surviving triangle is accepted by steps 1 to 3",
                 "the miss record {SWR_ID_NONE, 0, 0, 0}",
                 "Which triangle is never reported",
                 "a ray is occluded iff the nearest-mode answer\n *     of the same query is not a miss",
                 'hits[k].primitive != SWR_ID_NONE means "hit" in both modes',
                 "more than 2^32 - 2 primitives, so SWR_RAY_OCCLUDED is never a primitive number",
                 "unknown flag bits; a non-zero reserved; first_primitive < 0; primitive_count < -1; a range\n *     that ends beyond index_count / 3",
                 "after an error nothing was written",
                 "Not covered: more than one hit per ray; watertight edges; an un-waited call; and the C++ and Swift mirrors",
                 "it does not make the call cheaper on a reordered stream"):
        assert text in section, text
    # "Ray casts" keeps its sentences and points here
    casts = h[h.index("---- Ray casts"):h.index("---- Ray queries")]
    assert "Not covered: any-hit / occlusion-only rays" in casts and "Both facings are hit." in casts
    assert '"Ray queries" below covers the first three.' in casts
    # the limit the section cites is the one the upload enforces
    api = open(os.path.join(ROOT, "software-renderer_amd", "csrc", "swr_api.hip")).read()
    assert "if (index_count / 3 >= 0xFFFFFFFFll" in api and "more than 2^32-2 primitives" in api


def test_null_context_is_refused(swr):
    L = swr.load_library()
    B = swr.binding
    rays = np.zeros(2, dtype=B.RAY_DTYPE)
    rays["dir"] = (0, 0, 1)
    q = np.zeros(1, dtype=B.RAY_QUERY_DTYPE)
    q["flags"], q["primitive_count"] = B.RAYS_ANY_HIT, -1
    out = np.full(2 * 4, 0xA5A5A5A5, dtype=np.uint32)
    assert L.swr_query_rays(None, q.ctypes.data, rays.ctypes.data, 2, out.ctypes.data) == BAD_ARG
    assert L.swr_query_rays(None, None, rays.ctypes.data, 2, out.ctypes.data) == BAD_ARG
    assert L.swr_query_rays(None, None, None, 0, None) == BAD_ARG
    assert (out == 0xA5A5A5A5).all()
