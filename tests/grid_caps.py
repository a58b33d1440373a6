"""The capped grids: every launch site in software-renderer_amd/csrc/*.hip whose grid stops growing with its input — a std::min, an
`if (blocks > N)`, or a literal dim3(N) in front of a kernel that strides by its grid — and the one modulo fold (k_item_bounds' partial
records).  A kernel behind such a grid runs the body of its `for (i = ...; i < n; i += stride)` loop a second time only above
cap x block units, so a test below that size cannot tell a right stride from a wrong one.  A plain helper module of
tests/test_grid_caps.py (which imports SHAPES, so that the sizes drawn are the sizes checked here) and of
tests/test_grid_caps_table.py (which parses the launch wrappers and fails when a site has no entry, a threshold is stale, the named test
is missing, or its shape does not cross the threshold).  Not a conftest, not a test file.
"""
from __future__ import annotations

import dataclasses


@dataclasses.dataclass(frozen=True)
class Cap:
    """One capped launch site.

    kernel     the kernel's name, template arguments as they matter for the path (<...> is not parsed)
    file       the .hip file of the launch site, wrapper: the function that launches
    caps       every integer the cap can take at that site, as written (a ternary gives two); cap: the one in effect
    block      threads per workgroup
    unit       what one lane handles per trip (vertices / pixels / words / quads / indices / slots / ...)
    threshold  the first size with a second trip: cap * block + 1 (the fold: SLOTS * CHUNK + 1)
    test       node id of the GPU test that crosses it
    shape      key of SHAPES: SHAPES[shape]["units"] >= threshold
    evidence   (tests from before this table) a literal of the named test's module that fixes its size
    rule       how the threshold follows from the constants (below)
    """
    kernel: str
    file: str
    wrapper: str
    caps: tuple
    cap: int
    block: int
    unit: str
    threshold: int
    test: str
    shape: str
    evidence: str = ""
    rule: str = "cap"           # "cap": threshold = cap * block + 1; "fold": SLOTS * CHUNK + 1; "waves": COUNT_WAVES + 1


T = "tests/test_grid_caps.py::"


# ---- the shapes of tests/test_grid_caps.py, and the sizes tests from before it are known to reach -----------------------------------
def oneshot_first_chunk(ntri, cut=70):
    """Triangles in the first chunk of a one-shot upload (swr_api.hip, SWR_TUNE_ONESHOT_CUTS = {70, 100}: cut at 70 per cent, rounded up
    to a multiple of 64)."""
    return min(ntri, (ntri * cut // 100 + 63) // 64 * 64)


SKIN_NV = 262144 + 257
SKIN_W, SKIN_H = 1024, 520
BAND_W, BAND_H, BAND_ROW = 1280, 832, 820           # rows 820..831 lie past 4096 x 256 pixels
VALIDATE_TRIS = 349527                               # 1 048 581 indices
ONESHOT_TRIS = 499323                                # the first chunk of the one-shot upload alone holds 1 048 704 indices
ITEM_CHUNK, ITEM_SLOTS = 2048, 32
PADDED = (1 << 20) + 1

SHAPES = {
    "skin": dict(units=SKIN_NV, width=SKIN_W, height=SKIN_H),
    # a rectangle that is the whole band goes by the plain copy (band_read_delta), so the packed rectangles leave out the first tile row
    "delta_words": dict(units=1026 * (1056 - 32), width=1026, height=1056, y0=32),
    "delta_quads": dict(units=(2048 // 4) * (2084 - 32), width=2048, height=2084, y0=32),
    "band": dict(units=BAND_W * BAND_H, width=BAND_W, height=BAND_H, row=BAND_ROW),
    "validate": dict(units=3 * VALIDATE_TRIS, triangles=VALIDATE_TRIS),
    "validate_oneshot": dict(units=3 * oneshot_first_chunk(ONESHOT_TRIS), triangles=ONESHOT_TRIS),
    "item_bounds": dict(units=ITEM_SLOTS * ITEM_CHUNK + 1, chunk=ITEM_CHUNK, slots=ITEM_SLOTS),
    # tests from before this table
    "2^20+1 primitives": dict(units=PADDED),
    "2^20+4099 one-shot": dict(units=oneshot_first_chunk((1 << 20) + 4099)),
    "2^20+4096 clip": dict(units=((1 << 20) + 4096 + 255) // 256),
    "2^20 perspective": dict(units=(1 << 20) + 3),
    "cfg4 vertices": dict(units=3 * 200_000),
    "1.2 M list slots": dict(units=4 * 300_000),
    "cfg5 texture": dict(units=1024 * 1024),          # scenes.cfg5_textured: checker_texture(1024, 1024)
    "count segments": dict(units=6 * 200),             # 328 x 200: six row segments of 64 pixels per row
}

_PB = "tests/test_primitive_boundary.py::test_around_2_20_primitives[2^20+1]"

CAPS = [
    # ---- crossed for the first time by tests/test_grid_caps.py -----------------------------------------------------------------------
    Cap("k_skin_vertices<LDS, NRM>", "swr_skin.hip", "launch_skin_vertices", (1024, 65536), 1024, 256, "vertices", 262145,
        T + "test_skin_vertex_frame[matrices]", "skin"),
    Cap("k_skin_vertices_dq<NRM>", "swr_skin_dq.hip", "launch_skin_vertices_dq", (1024,), 1024, 256, "vertices", 262145,
        T + "test_skin_vertex_frame[dual_quaternions]", "skin"),
    Cap("k_delta_pack<false>", "swr_delta.hip", "launch_delta_pack", (4096,), 4096, 256, "words", 1048577,
        T + "test_delta_pack_rectangle[words]", "delta_words"),
    Cap("k_delta_pack<true>", "swr_delta.hip", "launch_delta_pack", (4096,), 4096, 256, "quads", 1048577,
        T + "test_delta_pack_rectangle[quads]", "delta_quads"),
    Cap("k_clip_ids", "swr_clip.hip", "launch_clip_ids", (4096,), 4096, 256, "pixels", 1048577, T + "test_clip_ids_past_the_cap", "band"),
    Cap("k_clear_band<LOAD>", "swr_kernels.hip", "launch_points_or_lines", (4096,), 4096, 256, "pixels", 1048577,
        T + "test_vertex_and_line_frames[line_stub-clear]", "band"),
    # (clear frames at 1920 x 1080 were crossed by tests/test_gpu_parity.py::test_vertices_primitive_points; the load instantiation was not)
    Cap("k_points_resolve<LOAD>", "swr_kernels.hip", "launch_points_or_lines", (4096,), 4096, 256, "pixels", 1048577,
        T + "test_vertex_and_line_frames[vertices-load]", "band"),
    Cap("k_validate_indices", "swr_kernels.hip", "launch_validate_indices", (4096,), 4096, 256, "indices", 1048577,
        T + "test_validate_indices_upload", "validate"),
    # the modulo fold: work unit u of an item combines into partial record u % ITEM_BOUNDS_SLOTS
    Cap("k_item_bounds<MT>", "swr_item_bounds.hip", "launch_item_bounds", (), 32, 2048, "triangles", 65537,
        T + "test_item_bounds_two_units_share_a_record", "item_bounds", rule="fold"),
    # ---- crossed by tests from before this table ---------------------------------------------------------------------------------------
    Cap("k_scene_bounds", "swr_upload.hip", "launch_build_stream", (128,), 128, 256, "vertices", 32769,
        "tests/test_load_action.py::test_eight_bands_chain_of_two_at_cfg4_size", "cfg4 vertices", "cfg4_soup(200_000)"),
    Cap("k_morton", "swr_upload.hip", "launch_build_stream", (2048,), 2048, 256, "triangles", 524289, _PB, "2^20+1 primitives",
        "K.padded(v0, i0, n_head, count)"),
    Cap("k_segment_keys", "swr_upload.hip", "launch_build_stream", (2048,), 2048, 256, "triangles", 524289, _PB, "2^20+1 primitives",
        "items = [(0, 3 * split, K.IDENT), (3 * split, 3 * (n - split), K.IDENT)]"),
    Cap("k_gather_stream", "swr_upload.hip", "launch_build_stream", (2048,), 2048, 256, "triangles", 524289, _PB, "2^20+1 primitives",
        "ctx.scene_upload(v, i)"),
    Cap("k_gather_stream", "swr_upload.hip", "launch_build_stream_range", (2048,), 2048, 256, "triangles", 524289,
        "tests/test_fragment_stage.py::test_gpu_colour_kernels_of_scenes_beyond_2_to_20_primitives", "2^20+4099 one-shot",
        "(1 << 20) + 4099"),
    Cap("k_gather_attrs", "swr_upload.hip", "launch_gather_attrs", (2048,), 2048, 256, "triangles", 524289, _PB, "2^20+1 primitives",
        '"textured_phong": (K.DT, 2)'),
    Cap("k_persp_fill", "swr_kernels.hip", "launch_persp_fill", (2048,), 2048, 256, "slots", 524289,
        "tests/test_perspective.py::test_beyond_2_to_20_primitives", "2^20 perspective", "far = (1 << 20)"),
    # (below its cap the grid is one workgroup per 64 row segments of 64 pixels, four waves each: a wave always strides.  The table keeps
    # the smallest size at which it does: one segment more than one workgroup's waves)
    # (four items over one range: from the second on, frame slot and stream slot differ)
    Cap("k_list_gather", "swr_kernels.hip", "launch_list_gather", (2048,), 2048, 256, "slots", 524289,
        "tests/test_draw_list.py::test_more_than_2_20_primitives", "1.2 M list slots", "random_soup(300_000, W, H, 0x2020"),
    Cap("k_texture_to_float", "swr_kernels.hip", "launch_texture_to_float", (2048,), 2048, 256, "texels", 524289,
        "tests/test_fragment_stage.py::test_gpu_cfg5_textured_full_size", "cfg5 texture", "swr.scenes.cfg5_textured()"),
    Cap("k_count_ids<PER_ITEM>", "swr_count.hip", "launch_count_ids", (512, 2048), 2048, 256, "segments", 5,
        "tests/test_count_ids.py::test_rule_sets_whole_target_both_groups", "count segments", 'W, H = K.TARGETS["small"]',
        rule="waves"),
]

# single-workgroup scans, launched with a literal dim3(1): every thread walks ceil(n / 1024) entries of its own, so the loop's second
# trip needs more than 1024 entries.  Not grid-strided (the table test's parser leaves them out), listed for the record.
SCANS = [
    Cap("k_clip_scan", "swr_clip.hip", "launch_clip_prep", (1,), 1, 1024, "count blocks", 1025,
        "tests/test_depth_clip.py::test_2_20_edge[above_to_below]", "2^20+4096 clip", "(1 << 20) + 4096"),
]
