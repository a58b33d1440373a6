"""ctypes binding of include/swr.h (plumbing for tests / bench; the product is the .so)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# SWR_LIBRARY: tools/ only — load another build of the same C-ABI (e.g. lib/libswr_hip_ablation.so of `make ablation`)
_LIB = os.environ.get("SWR_LIBRARY") or os.path.join(_PKG, "lib", "libswr_hip.so")

FLAG_DEPTH_TEST = 1
FLAG_NO_COLOR = 2
FLAG_METAL_RULES = 4
FLAG_REAL_LINES = 8      # .line primitives: the reference's DDA (Renderer.swift:405-419) instead of its empty stub (:289-293)
FLAG_LOAD = 16           # load action (ABI 6): the frame starts from the image already there instead of the clear (include/swr.h)
FLAG_PRIMITIVE_IDS = 32  # the frame also writes an ID image: which triangle is visible at every pixel (Context.read_ids)
FLAG_CULL_BACK = 64      # face culling: back-facing triangles are not drawn (include/swr.h "Face culling")
FLAG_CULL_FRONT = 128    # front-facing triangles are not drawn (with FLAG_CULL_BACK: every triangle with a facing)
FLAG_FRONT_CCW = 256     # front = counter-clockwise as displayed; without it clockwise (Metal's default winding)
FLAG_DEPTH_CLIP = 1024   # depth clipping: triangles clipped against the near (z >= 0) and far (z <= w) planes (include/swr.h "Depth clipping")
FLAG_PERSPECTIVE = 2048  # perspective-correct interpolation of colour and varyings (include/swr.h "Perspective-correct interpolation")
FLAG_BLEND = 4096        # alpha blending: every fragment is blended into the pixel in draw order (include/swr.h "Alpha blending")
BLEND_OVER, BLEND_ADD = 0, 1   # swr_blend.mode
RESOLVE_DEPTH_SAMPLE0, RESOLVE_DEPTH_MIN = 0, 1   # swr_resolve.depth_filter (include/swr.h "Supersampled resolve")
ID_NONE = 0xFFFFFFFF     # SWR_ID_NONE: a pixel where the frame keeps no fragment
COUNT_PER_PRIMITIVE, COUNT_PER_ITEM = 0, 1   # swr_id_count.group (include/swr.h "Visibility counts")

# every symbol include/swr.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "swr_abi_version", "swr_version", "swr_context_create", "swr_context_destroy", "swr_last_error",
    "swr_render", "swr_scene_upload", "swr_target_set", "swr_draw", "swr_draw_primitives", "swr_sync", "swr_read_color",
    "swr_read_depth", "swr_timing_enable", "swr_get_timings", "swr_timing_totals", "swr_timing_reset", "swr_pipeline_enable", "swr_tile_rows", "swr_tile_cols",
    "swr_band_rows", "swr_scene_attributes", "swr_material_set", "swr_texture_upload",
    "swr_timing_sample", "swr_context_bands", "swr_context_band_info", "swr_host_alloc", "swr_host_free",
    "swr_host_register", "swr_host_unregister", "swr_present", "swr_present_wait", "swr_device_count",
    "swr_render_timings", "swr_debug_fault", "swr_debug_set", "swr_target_write", "swr_draw_list", "swr_read_ids",
    "swr_blend_set", "swr_read_color_resolved", "swr_read_depth_resolved", "swr_render_resolved", "swr_count_ids",
    "swr_query_depth", "swr_read_color_delta", "swr_read_depth_delta", "swr_delta_reset", "swr_render_delta",
    "swr_scene_skin", "swr_pose_set", "swr_scene_morph", "swr_morph_set", "swr_item_bounds",
    "swr_pose_set_dq", "swr_scene_morph_sparse", "swr_morph_pose_set", "swr_scene_normals", "swr_cast_rays",
    "swr_query_rays",
]
# swr_debug_set keys (test hooks, include/swr.h)
DEBUG_STREAM_ORDER, DEBUG_CULL, DEBUG_BIN_MODE, DEBUG_ONESHOT_MIN_TRIS, DEBUG_DEPTH_KEYS32, DEBUG_RASTER_SORT = 1, 2, 3, 4, 5, 6
BIN_MODE_AUTO, BIN_MODE_EXACT, BIN_MODE_FIXED, BIN_MODE_ATOMIC = 0, 1, 2, 3


class SwrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"swr error {code}: {msg}")
        self.code = code


class RenderPass(ctypes.Structure):
    """swr_render_pass (include/swr.h) == RenderPass (Renderer.swift:191-200)."""
    _fields_ = [
        ("color", ctypes.c_void_p), ("depth", ctypes.c_void_p),
        ("width", ctypes.c_int64), ("height", ctypes.c_int64),
        ("color_bytes_per_row", ctypes.c_int64), ("depth_bytes_per_row", ctypes.c_int64),
        ("vertices", ctypes.c_void_p), ("vertex_count", ctypes.c_int64),
        ("indices", ctypes.c_void_p), ("index_count", ctypes.c_int64),
        ("primitive_type", ctypes.c_int32), ("flags", ctypes.c_uint32),
        ("transform", ctypes.c_float * 16),
        ("attributes", ctypes.c_void_p), ("material", ctypes.c_void_p), ("texture", ctypes.c_void_p),
        ("tex_width", ctypes.c_int32), ("tex_height", ctypes.c_int32),
        ("scene_id", ctypes.c_uint64),        # ABI 4: non-zero = "same arrays as the last pass with this id": no upload
    ]


class Material(ctypes.Structure):
    """swr_material (include/swr.h): the extended fragment stage."""
    _fields_ = [("shader", ctypes.c_int32), ("shininess_log2", ctypes.c_int32),
                ("light_dir", ctypes.c_float * 4), ("half_dir", ctypes.c_float * 4),
                ("ambient", ctypes.c_float), ("diffuse", ctypes.c_float), ("specular", ctypes.c_float),
                ("reserved", ctypes.c_float)]

    @classmethod
    def from_shading(cls, sh):
        return cls(int(sh.shader), int(sh.shininess_log2),
                   (ctypes.c_float * 4)(*[float(x) for x in sh.light_dir], 0.0),
                   (ctypes.c_float * 4)(*[float(x) for x in sh.half_dir], 0.0),
                   float(sh.ambient), float(sh.diffuse), float(sh.specular), 0.0)


class Blend(ctypes.Structure):
    """swr_blend (include/swr.h): the state of FLAG_BLEND frames."""
    _fields_ = [("mode", ctypes.c_int32), ("opacity", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


class Resolve(ctypes.Structure):
    """swr_resolve (include/swr.h): the factor S (1, 2 or 4 samples per axis) and the depth filter of a supersampled resolve."""
    _fields_ = [("factor", ctypes.c_int32), ("depth_filter", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


class IdCount(ctypes.Structure):
    """swr_id_count (include/swr.h): the group (COUNT_PER_PRIMITIVE / COUNT_PER_ITEM) and the half-open rectangle of a visibility count."""
    _fields_ = [("group", ctypes.c_int32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("x1", ctypes.c_int32), ("y1", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 3)]


class DepthBox(ctypes.Structure):
    """swr_depth_box (include/swr.h): the half-open rectangle of a depth query and the depth it is tested with."""
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("x1", ctypes.c_int32), ("y1", ctypes.c_int32), ("z", ctypes.c_float),
                ("reserved", ctypes.c_int32 * 3)]


DEPTH_QUERY_MAX = 1 << 16    # SWR_DEPTH_QUERY_MAX: boxes per swr_query_depth call
# swr_depth_box as a numpy record
DEPTH_BOX_DTYPE = np.dtype([("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32), ("z", np.float32),
                            ("reserved", np.int32, (3,))])


class ItemBound(ctypes.Structure):
    """swr_item_bound (include/swr.h "Item bounds"): where a draw item lands on the target, its depth range and its triangle counts."""
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("x1", ctypes.c_int32), ("y1", ctypes.c_int32),
                ("zmin", ctypes.c_float), ("zmax", ctypes.c_float),
                ("drawable", ctypes.c_uint32), ("skipped", ctypes.c_uint32), ("behind", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


# swr_item_bound as a numpy record (what Context.item_bounds returns)
ITEM_BOUND_DTYPE = np.dtype([("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32), ("zmin", np.float32),
                             ("zmax", np.float32), ("drawable", np.uint32), ("skipped", np.uint32), ("behind", np.uint32),
                             ("reserved", np.uint32, (3,))])


def depth_boxes(bounds, z_margin) -> np.ndarray:
    """The (n, 5) rows (x0, y0, x1, y1, zmin - z_margin) Context.query_depth takes, from the records of Context.item_bounds.  zmin is
    the nearest vertex: a fragment's depth can lie in front of it by rounding (include/swr.h "Item bounds"), so the caller chooses
    the margin.  The subtraction is made in float32, as the box's z is one.  Pure: no context, no device."""
    b = np.asarray(bounds)
    rows = np.zeros((b.size, 5), dtype=np.float64)
    for j, f in enumerate(("x0", "y0", "x1", "y1")):
        rows[:, j] = b[f].reshape(-1)
    rows[:, 4] = b["zmin"].reshape(-1).astype(np.float32) - np.float32(z_margin)
    return rows


class DeltaStats(ctypes.Structure):
    """swr_delta_stats (include/swr.h "Delta reads"): what a delta read did."""
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("x1", ctypes.c_int32), ("y1", ctypes.c_int32),
                ("tiles", ctypes.c_int64), ("tiles_changed", ctypes.c_int64), ("bytes_copied", ctypes.c_int64),
                ("full", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    @property
    def rect(self):
        """(x0, y0, x1, y1): the bounding box of everything written, pixels of the full target; all 0 when nothing was."""
        return (self.x0, self.y0, self.x1, self.y1)


DELTA_COLOR, DELTA_DEPTH = 1, 2     # SWR_DELTA_*: the bits of swr_delta_reset


class SkinVertex(ctypes.Structure):
    """swr_skin_vertex (include/swr.h "Skinned meshes"): the four joint influences of one vertex."""
    _fields_ = [("joint", ctypes.c_uint32 * 4), ("weight", ctypes.c_float * 4)]


SKIN_MAX_JOINTS = 1024       # SWR_SKIN_MAX_JOINTS: joints per pose
# swr_skin_vertex as a numpy record
SKIN_VERTEX_DTYPE = np.dtype([("joint", np.uint32, (4,)), ("weight", np.float32, (4,))])


def dual_quats(matrices) -> np.ndarray:
    """The (J, 8) float32 table swr_pose_set_dq takes, from (J, 4, 4) rigid matrices M (the mathematical matrices: rotation in
    M[j, :3, :3], translation in M[j, :3, 3]; a pose held column-major as swr_pose_set takes it is passed as
    P.reshape(-1, 4, 4).transpose(0, 2, 1)).  Computed in float64: the unit quaternion r = (x, y, z, w) of the rotation with w >= 0,
    the dual part 0.5 * (t, 0) * r, both rounded once to float32.  Scale and shear cannot be expressed: a matrix that has them gives
    the quaternion of whatever rotation the extraction reads out of it."""
    M = np.asarray(matrices, dtype=np.float64).reshape(-1, 4, 4)
    out = np.empty((M.shape[0], 8), dtype=np.float64)
    for j, m in enumerate(M):
        R, t = m[:3, :3], m[:3, 3]
        # the largest of the four squared components first: the extraction never divides by a small number
        tr = R[0, 0] + R[1, 1] + R[2, 2]
        c = np.array([1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2], 1 + tr])
        k = int(np.argmax(c))
        if k == 3:
            q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], c[3]])
        elif k == 0:
            q = np.array([c[0], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]])
        elif k == 1:
            q = np.array([R[0, 1] + R[1, 0], c[1], R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]])
        else:
            q = np.array([R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], c[2], R[1, 0] - R[0, 1]])
        q = q / np.sqrt((q * q).sum())
        if q[3] < 0:
            q = -q
        x, y, z, w = q
        out[j, 0:4] = q
        out[j, 4] = 0.5 * (t[0] * w + t[1] * z - t[2] * y)
        out[j, 5] = 0.5 * (-t[0] * z + t[1] * w + t[2] * x)
        out[j, 6] = 0.5 * (t[0] * y - t[1] * x + t[2] * w)
        out[j, 7] = -0.5 * (t[0] * x + t[1] * y + t[2] * z)
    return out.astype(np.float32)


class MorphTargets(ctypes.Structure):
    """swr_morph_targets (include/swr.h "Morph targets"): the deltas of target_count targets, target-major, packed float3."""
    _fields_ = [("position_deltas", ctypes.c_void_p), ("normal_deltas", ctypes.c_void_p), ("vertex_count", ctypes.c_int64),
                ("target_count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


MORPH_MAX_TARGETS = 256      # SWR_MORPH_MAX_TARGETS: targets per scene


class MorphSparseTarget(ctypes.Structure):
    """swr_morph_sparse_target (include/swr.h "Sparse morph targets"): the vertices one target moves, ascending, and their deltas."""
    _fields_ = [("indices", ctypes.c_void_p), ("position_deltas", ctypes.c_void_p), ("normal_deltas", ctypes.c_void_p),
                ("count", ctypes.c_int64)]


class MorphSparse(ctypes.Structure):
    """swr_morph_sparse: target_count sparse targets of a scene of vertex_count vertices."""
    _fields_ = [("targets", ctypes.POINTER(MorphSparseTarget)), ("vertex_count", ctypes.c_int64), ("target_count", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


POSE_MATRICES, POSE_DUAL_QUATS = 0, 1      # SWR_POSE_*: the pose_kind of swr_morph_pose_set


class Normals(ctypes.Structure):
    """swr_normals (include/swr.h "Computed normals"): where the resident scene's normals come from."""
    _fields_ = [("mode", ctypes.c_int32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_int32 * 2)]


NORMALS_UPLOADED, NORMALS_SMOOTH, NORMALS_FLAT = 0, 1, 2    # SWR_NORMALS_*: swr_normals.mode
NORMALS_FLIP = 1                                             # SWR_NORMALS_FLIP: swr_normals.flags
NORMALS_MODES = {"uploaded": NORMALS_UPLOADED, "smooth": NORMALS_SMOOTH, "flat": NORMALS_FLAT}

RAYS_MAX = 1 << 16           # SWR_RAYS_MAX: rays per swr_cast_rays call
# swr_ray and swr_ray_hit as numpy records (include/swr.h "Ray casts"): what Context.cast_rays takes and returns
RAY_DTYPE = np.dtype([("origin", np.float32, (3,)), ("tmin", np.float32), ("dir", np.float32, (3,)), ("tmax", np.float32)])
RAY_HIT_DTYPE = np.dtype([("primitive", np.uint32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])
# swr_ray_query (include/swr.h "Ray queries"): what Context.query_rays hands swr_query_rays
RAYS_ANY_HIT, RAYS_CULL_BACK, RAYS_CULL_FRONT, RAYS_FRONT_CW = 1, 2, 4, 8      # SWR_RAYS_*: swr_ray_query.flags
RAY_OCCLUDED = 0xFFFFFFFE    # SWR_RAY_OCCLUDED: hits[k].primitive of an occluded ray under RAYS_ANY_HIT
RAY_QUERY_DTYPE = np.dtype([("flags", np.uint32), ("reserved", np.uint32), ("first_primitive", np.int64), ("primitive_count", np.int64)])
RAYS_CULL = {None: 0, "none": 0, "back": RAYS_CULL_BACK, "front": RAYS_CULL_FRONT, "both": RAYS_CULL_BACK | RAYS_CULL_FRONT}


def pixel_ray(transform, W: int, H: int, x, y) -> np.ndarray:
    """The object-space ray(s) through the centre of pixel (x, y) of a W x H target drawn with `transform` (16 floats, column-major, as
    for draw): a RAY_DTYPE record, or an array of them when x and y are arrays.  The ray runs from NDC depth 0 (t = 0) to depth 1
    (t = 1): origin and origin + dir are the un-projected near and far points, tmin = 0, tmax = 1, and `dir` is not normalised.  The
    matrix is inverted on the host in float64; a singular one raises numpy.linalg.LinAlgError.  A projection without a far plane
    (depth 1 lies at infinity, like scenes.app_transform's) gives the direction towards it instead: the point of depth d is then
    origin + d / (1 - d) * dir, and tmax is the largest float."""
    m = np.asarray(transform, dtype=np.float64).reshape(4, 4).T       # (column-major in memory)
    inv = np.linalg.inv(m)
    xs, ys = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    nx = (xs + 0.5) / W * 2.0 - 1.0
    ny = 1.0 - (ys + 0.5) / H * 2.0
    one = np.ones_like(nx)
    near = np.stack([nx, ny, 0.0 * one, one], axis=-1) @ inv.T
    far = np.stack([nx, ny, one, one], axis=-1) @ inv.T
    origin = near[..., :3] / near[..., 3:]
    infinite = np.abs(far[..., 3:]) <= 1e-12 * np.abs(near[..., 3:])
    wf = np.where(infinite, 1.0, far[..., 3:])
    direction = np.where(infinite, far[..., :3] / near[..., 3:], far[..., :3] / wf - origin)
    rays = np.zeros(xs.shape, dtype=RAY_DTYPE)
    rays["origin"] = origin
    rays["dir"] = direction
    rays["tmin"] = 0.0
    rays["tmax"] = np.where(infinite[..., 0], np.finfo(np.float32).max, 1.0)
    return rays


def sparse_targets(dense_deltas, dense_normal_deltas=None) -> list:
    """Dense targets of shape (T, nv, 3) as the list Context.scene_morph_sparse takes: per target the indices of the vertices whose
    delta (or normal delta) is not all zero, ascending, and their rows.  A vertex that is dropped is one the sparse target does not
    touch: on it a -0 coordinate stays -0 and a non-finite weight has no effect, where the dense target with its zero row gives +0
    and NaN; everywhere else the two morph alike, bit for bit."""
    dp = np.ascontiguousarray(dense_deltas, dtype=np.float32)
    if dp.ndim != 3 or dp.shape[2] != 3:
        raise ValueError(f"dense_deltas of shape {dp.shape}, not (T, nv, 3)")
    dn = None
    if dense_normal_deltas is not None:
        dn = np.ascontiguousarray(dense_normal_deltas, dtype=np.float32)
        if dn.shape != dp.shape:
            raise ValueError(f"dense_normal_deltas of shape {dn.shape}, not {dp.shape}")
    out = []
    for t in range(dp.shape[0]):
        moved = np.any(dp[t] != 0, axis=1)
        if dn is not None:
            moved |= np.any(dn[t] != 0, axis=1)
        idx = np.flatnonzero(moved).astype(np.uint32)
        out.append((idx, dp[t][idx]) if dn is None else (idx, dp[t][idx], dn[t][idx]))
    return out


class Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("device_count", ctypes.c_uint32),
                ("wait_budget_ms", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class RenderTimes(ctypes.Structure):
    """swr_render_times: wall-clock phases of the last swr_render."""
    _fields_ = [("h2d_ms", ctypes.c_float), ("stream_build_ms", ctypes.c_float), ("draw_ms", ctypes.c_float),
                ("gather_ms", ctypes.c_float), ("total_ms", ctypes.c_float), ("scene_cached", ctypes.c_int32),
                ("frames", ctypes.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

FAULT_NONE, FAULT_LOST_EVENT, FAULT_ENQUEUE = 0, 1, 2


class DrawItem(ctypes.Structure):
    """swr_draw_item: indices [first_index, first_index + index_count) drawn with `transform` (16 floats, as Context.draw's)."""
    _fields_ = [("first_index", ctypes.c_int64), ("index_count", ctypes.c_int64), ("transform", ctypes.c_float * 16)]


DRAW_LIST_MAX = 4096

# structured-array form of a draw list (Context.draw_list accepts it as is)
DRAW_ITEM_DTYPE = np.dtype([("first_index", np.int64), ("index_count", np.int64), ("transform", np.float32, (16,))])


class Timings(ctypes.Structure):
    _fields_ = [("setup_bin_ms", ctypes.c_float), ("scan_ms", ctypes.c_float),
                ("scatter_ms", ctypes.c_float), ("raster_ms", ctypes.c_float),
                ("total_ms", ctypes.c_float), ("tile_pairs", ctypes.c_int64),
                ("tiles", ctypes.c_int64), ("triangles", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def library_path() -> str:
    return _LIB


def build(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of the in-tree library (cross-compiles without a GPU)."""
    srcs = [os.path.join(_PKG, "csrc", f) for f in os.listdir(os.path.join(_PKG, "csrc"))]
    srcs.append(os.path.join(_PKG, "..", "include", "swr.h"))
    stale = force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", _PKG, "-s", "lib/libswr_hip.so"])
    return _LIB


_lib = None


def load_library():
    """dlopen the product library; raises if it is not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise SwrError(-4, f"{_LIB} is not built; run `make -C software-renderer_amd` (hipcc, gfx950)")
    L = ctypes.CDLL(_LIB)
    vp, i64, i32, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32
    L.swr_abi_version.restype = ctypes.c_int
    L.swr_version.restype = ctypes.c_char_p
    L.swr_last_error.restype = ctypes.c_char_p
    L.swr_last_error.argtypes = [vp]
    L.swr_context_create.argtypes = [ctypes.POINTER(Config), ctypes.POINTER(vp)]
    L.swr_context_destroy.argtypes = [vp]
    L.swr_context_destroy.restype = None
    L.swr_render.argtypes = [vp, ctypes.POINTER(RenderPass)]
    L.swr_scene_upload.argtypes = [vp, vp, i64, vp, i64]
    L.swr_target_set.argtypes = [vp, i64, i64, i64, i64]
    L.swr_draw.argtypes = [vp, vp, u32]
    L.swr_draw_primitives.argtypes = [vp, vp, u32, i32]
    L.swr_draw_primitives.restype = ctypes.c_int
    L.swr_sync.argtypes = [vp]
    L.swr_read_color.argtypes = [vp, vp]
    L.swr_read_depth.argtypes = [vp, vp]
    L.swr_timing_enable.argtypes = [vp, ctypes.c_int]
    L.swr_get_timings.argtypes = [vp, ctypes.POINTER(Timings)]
    L.swr_timing_totals.argtypes = [vp, ctypes.POINTER(Timings), ctypes.POINTER(i64)]
    L.swr_timing_reset.argtypes = [vp]
    L.swr_timing_sample.argtypes = [vp, ctypes.c_int]
    L.swr_timing_sample.restype = ctypes.c_int
    L.swr_pipeline_enable.argtypes = [vp, ctypes.c_int]
    L.swr_pipeline_enable.restype = ctypes.c_int
    L.swr_band_rows.argtypes = [i64, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.swr_scene_attributes.argtypes = [vp, vp, i64]
    L.swr_material_set.argtypes = [vp, ctypes.POINTER(Material)]
    L.swr_texture_upload.argtypes = [vp, vp, i32, i32]
    L.swr_context_bands.argtypes = [vp]
    L.swr_context_band_info.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.swr_host_alloc.argtypes = [ctypes.c_size_t]
    L.swr_host_alloc.restype = vp
    L.swr_host_free.argtypes = [vp]
    L.swr_host_free.restype = None
    L.swr_host_register.argtypes = [vp, ctypes.c_size_t]
    L.swr_host_unregister.argtypes = [vp]
    try:
        L.swr_render_timings.argtypes = [vp, ctypes.POINTER(RenderTimes)]
        L.swr_render_timings.restype = ctypes.c_int
        L.swr_debug_fault.argtypes = [vp, ctypes.c_int]
        L.swr_debug_fault.restype = ctypes.c_int
        L.swr_debug_set.argtypes = [vp, ctypes.c_int, ctypes.c_int64]
        L.swr_debug_set.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # only an older A/B build loaded by tools/ may lack the ABI 4 entry points
            raise
    L.swr_present.argtypes = [vp, vp, vp]
    try:
        L.swr_draw_list.argtypes = [vp, vp, i32, u32]
        L.swr_draw_list.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack it)
            raise
    try:
        L.swr_read_ids.argtypes = [vp, vp]
        L.swr_read_ids.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack it)
            raise
    try:
        L.swr_blend_set.argtypes = [vp, ctypes.POINTER(Blend)]
        L.swr_blend_set.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack it)
            raise
    try:
        L.swr_read_color_resolved.argtypes = [vp, ctypes.POINTER(Resolve), vp]
        L.swr_read_depth_resolved.argtypes = [vp, ctypes.POINTER(Resolve), vp]
        L.swr_render_resolved.argtypes = [vp, ctypes.POINTER(RenderPass), ctypes.POINTER(Resolve)]
        for name in ("swr_read_color_resolved", "swr_read_depth_resolved", "swr_render_resolved"):
            getattr(L, name).restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack them)
            raise
    try:
        L.swr_count_ids.argtypes = [vp, ctypes.POINTER(IdCount), vp, i64, vp]
        L.swr_count_ids.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack it)
            raise
    try:
        L.swr_query_depth.argtypes = [vp, vp, i64, vp]
        L.swr_query_depth.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack it)
            raise
    try:
        L.swr_item_bounds.argtypes = [vp, vp, i32, u32, vp]
        L.swr_item_bounds.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack it)
            raise
    try:
        L.swr_read_color_delta.argtypes = [vp, vp, ctypes.POINTER(DeltaStats)]
        L.swr_read_depth_delta.argtypes = [vp, vp, ctypes.POINTER(DeltaStats)]
        L.swr_delta_reset.argtypes = [vp, ctypes.c_uint32]
        L.swr_render_delta.argtypes = [vp, ctypes.POINTER(RenderPass), ctypes.POINTER(DeltaStats)]
        for name in ("swr_read_color_delta", "swr_read_depth_delta", "swr_delta_reset", "swr_render_delta"):
            getattr(L, name).restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack them)
            raise
    try:
        L.swr_scene_skin.argtypes = [vp, vp, i64]
        L.swr_pose_set.argtypes = [vp, vp, i32]
        for name in ("swr_scene_skin", "swr_pose_set"):
            getattr(L, name).restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack them)
            raise
    try:
        L.swr_pose_set_dq.argtypes = [vp, vp, i32]
        L.swr_pose_set_dq.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack it)
            raise
    try:
        L.swr_scene_morph.argtypes = [vp, ctypes.POINTER(MorphTargets)]
        L.swr_morph_set.argtypes = [vp, vp, i32]
        for name in ("swr_scene_morph", "swr_morph_set"):
            getattr(L, name).restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack them)
            raise
    try:
        L.swr_scene_morph_sparse.argtypes = [vp, ctypes.POINTER(MorphSparse)]
        L.swr_morph_pose_set.argtypes = [vp, vp, i32, vp, i32, i32]
        for name in ("swr_scene_morph_sparse", "swr_morph_pose_set"):
            getattr(L, name).restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack them)
            raise
    try:
        L.swr_scene_normals.argtypes = [vp, ctypes.POINTER(Normals)]
        L.swr_scene_normals.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack it)
            raise
    try:
        L.swr_cast_rays.argtypes = [vp, vp, i64, u32, vp]
        L.swr_cast_rays.restype = ctypes.c_int
        L.swr_query_rays.argtypes = [vp, vp, vp, i64, vp]
        L.swr_query_rays.restype = ctypes.c_int
    except AttributeError:
        if not os.environ.get("SWR_LIBRARY"):      # (an older A/B build loaded by tools/ may lack it)
            raise
    L.swr_target_write.argtypes = [vp, vp, vp]
    L.swr_target_write.restype = ctypes.c_int
    L.swr_present_wait.argtypes = [vp]
    for name in ("swr_context_bands", "swr_context_band_info", "swr_host_register", "swr_host_unregister", "swr_present",
                 "swr_present_wait"):
        getattr(L, name).restype = ctypes.c_int
    for name in ("swr_scene_attributes", "swr_material_set", "swr_texture_upload"):
        getattr(L, name).restype = ctypes.c_int
    for name in ("swr_context_create", "swr_render", "swr_scene_upload", "swr_target_set", "swr_draw",
                 "swr_sync", "swr_read_color", "swr_read_depth", "swr_timing_enable", "swr_get_timings", "swr_timing_totals", "swr_timing_reset",
                 "swr_band_rows", "swr_tile_rows", "swr_tile_cols"):
        getattr(L, name).restype = ctypes.c_int
    _lib = L
    return L


def device_count() -> int:
    """Visible HIP devices (0 without a GPU / driver)."""
    L = load_library()
    L.swr_device_count.restype = ctypes.c_int
    return int(L.swr_device_count())


def tile_shape():
    L = load_library()
    return L.swr_tile_cols(), L.swr_tile_rows()


def band_rows(height: int, parts: int, part: int):
    L = load_library()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    rc = L.swr_band_rows(height, parts, part, ctypes.byref(a), ctypes.byref(b))
    if rc:
        raise SwrError(rc, "swr_band_rows: bad arguments")
    return a.value, b.value


# status codes of include/swr.h that the binding itself looks at
ERR_BAD_ARG, ERR_NO_SCENE = -1, -6


class HostImage:
    """A page-locked host image from swr_host_alloc (what a .storageModeShared MTLBuffer is to the reference,
    App.swift:59-60), viewed as a NumPy array; every GPU copies its band straight into it (swr_present)."""

    def __init__(self, shape, dtype):
        self._L = load_library()
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = self._L.swr_host_alloc(self.nbytes)
        if not self.ptr:
            raise SwrError(-7, f"swr_host_alloc({self.nbytes}) failed")
        buf = (ctypes.c_uint8 * self.nbytes).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=self.dtype).reshape(self.shape)
        self._busy = set()          # contexts with a present into this image in flight

    def free(self):
        if self.ptr and self._busy:
            raise SwrError(-1, "HostImage.free() while a swr_present into it is in flight: call present_wait() first")
        if self.ptr:
            self.array = None
            self._L.swr_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def host_register(a: np.ndarray):
    rc = load_library().swr_host_register(a.ctypes.data, a.nbytes)
    if rc:
        raise SwrError(rc, "swr_host_register failed")


def host_unregister(a: np.ndarray):
    load_library().swr_host_unregister(a.ctypes.data)


class Context:
    """swr_context: one per caller thread (GpuRenderer instance, App.swift:149); device_count > 1 = one context
    driving that many tile-row bands on as many GPUs as are visible."""

    def __init__(self, device: int = -1, device_count: int = 0, wait_budget_ms: int = 0):
        self._L = load_library()
        self._h = ctypes.c_void_p()
        self._present_refs = {}         # id -> destination of the presents in flight: kept alive until present_wait / close
        cfg = Config(device, device_count, wait_budget_ms, 0)
        rc = self._L.swr_context_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc:
            raise SwrError(rc, (self._L.swr_last_error(None) or b"").decode())
        self.width = self.height = 0
        self.row_begin = self.row_end = 0
        self._scene_prims = 0           # index_count / 3 of the resident scene
        self._scene_vertices = 0        # its vertex count
        self._last_list = None          # (primitives, items) of the last frame when it was a draw list (count_ids' default n)

    def close(self):
        if self._h:
            self._L.swr_context_destroy(self._h)      # (waits for, or abandons, every copy in flight)
            self._h = ctypes.c_void_p()
        self._release_presents()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _m_src = None

    def _check(self, rc: int):
        if rc:
            raise SwrError(rc, (self._L.swr_last_error(self._h) or b"").decode())

    # -- resident path -------------------------------------------------------------------
    def scene_upload(self, vertices: np.ndarray, indices: np.ndarray):
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 8)
        i = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        self._check(self._L.swr_scene_upload(self._h, v.ctypes.data, v.shape[0], i.ctypes.data, i.size))
        self._scene_prims = i.size // 3
        self._scene_vertices = v.shape[0]

    def scene_attributes(self, attrs: np.ndarray):
        a = np.ascontiguousarray(attrs, dtype=np.float32).reshape(-1, 8)
        self._check(self._L.swr_scene_attributes(self._h, a.ctypes.data, a.shape[0]))

    def scene_skin(self, joints: "np.ndarray | None", weights: "np.ndarray | None" = None):
        """swr_scene_skin: per vertex four joint indices (nv x 4, integers) and four weights (nv x 4, float32), or one
        SKIN_VERTEX_DTYPE record array as `joints`; None removes the skin and restores the bind pose."""
        if joints is None:
            self._check(self._L.swr_scene_skin(self._h, None, 0))
            return
        if weights is None:
            sk = np.ascontiguousarray(joints, dtype=SKIN_VERTEX_DTYPE).reshape(-1)
        else:
            j = np.asarray(joints).reshape(-1, 4)
            sk = np.zeros(j.shape[0], dtype=SKIN_VERTEX_DTYPE)
            sk["joint"] = j
            sk["weight"] = np.asarray(weights, dtype=np.float32).reshape(-1, 4)
        self._check(self._L.swr_scene_skin(self._h, sk.ctypes.data, sk.shape[0]))

    def pose_set(self, joints: "np.ndarray | None"):
        """swr_pose_set: the resident scene in the pose `joints` — joint_count x 16 floats, each matrix column-major like a frame's
        transform (a (J, 4, 4) array M with M[j] the mathematical matrix is passed as M.transpose(0, 2, 1)); None: the bind pose.
        Blocking: the pose is in effect when the call returns."""
        if joints is None:
            self._check(self._L.swr_pose_set(self._h, None, 0))
            return
        m = np.ascontiguousarray(joints, dtype=np.float32).reshape(-1, 16)
        self._check(self._L.swr_pose_set(self._h, m.ctypes.data, m.shape[0]))

    def pose_set_dq(self, dual_quats: "np.ndarray | None"):
        """swr_pose_set_dq: the resident scene in the pose `dual_quats` — a (J, 8) float32 array, per joint the real quaternion
        (x, y, z, w), then the dual quaternion (dual_quats() makes it from rigid matrices); None: the bind pose.  The joints are
        blended as dual quaternions, so a twisting limb keeps its volume.  Blocking: the pose is in effect when the call returns."""
        if dual_quats is None:
            self._check(self._L.swr_pose_set_dq(self._h, None, 0))
            return
        q = np.ascontiguousarray(dual_quats, dtype=np.float32).reshape(-1, 8)
        self._check(self._L.swr_pose_set_dq(self._h, q.ctypes.data, q.shape[0]))

    def scene_morph(self, position_deltas: "np.ndarray | None", normal_deltas: "np.ndarray | None" = None):
        """swr_scene_morph: the morph targets of the resident scene — position deltas of shape (T, nv, 3) and, optionally, normal
        deltas of the same shape; None removes the targets.  The deltas are copied; every weight is 0 afterwards."""
        if position_deltas is None:
            self._check(self._L.swr_scene_morph(self._h, None))
            return
        dp = np.ascontiguousarray(position_deltas, dtype=np.float32)
        if dp.ndim != 3 or dp.shape[2] != 3:
            raise ValueError(f"position_deltas of shape {dp.shape}, not (T, nv, 3)")
        dn = None
        if normal_deltas is not None:
            dn = np.ascontiguousarray(normal_deltas, dtype=np.float32)
            if dn.shape != dp.shape:
                raise ValueError(f"normal_deltas of shape {dn.shape}, not {dp.shape}")
        t = MorphTargets(dp.ctypes.data, dn.ctypes.data if dn is not None else None, dp.shape[1], dp.shape[0], 0)
        self._check(self._L.swr_scene_morph(self._h, ctypes.byref(t)))

    def morph_set(self, weights: "np.ndarray | None"):
        """swr_morph_set: the resident scene morphed by one weight per target (a target with weight 0 is skipped); None: every
        weight 0.  Blocking: the shape is in effect when the call returns."""
        if weights is None:
            self._check(self._L.swr_morph_set(self._h, None, 0))
            return
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        self._check(self._L.swr_morph_set(self._h, w.ctypes.data, w.shape[0]))

    def scene_morph_sparse(self, targets: "list | None", vertex_count: "int | None" = None):
        """swr_scene_morph_sparse: sparse morph targets of the resident scene — a list with, per target, (indices, position_deltas)
        or (indices, position_deltas, normal_deltas): the vertices the target moves, strictly ascending, and count x 3 deltas; an
        empty index array is an empty target.  None removes the targets, of either kind.  vertex_count: the scene's (default: that
        of the last scene_upload).  The arrays are copied; every weight is 0 afterwards; morph_set serves these targets too."""
        if targets is None:
            self._check(self._L.swr_scene_morph_sparse(self._h, None))
            return
        keep, recs = [], (MorphSparseTarget * max(1, len(targets)))()
        for k, t in enumerate(targets):
            idx = np.ascontiguousarray(t[0], dtype=np.uint32).reshape(-1)
            dp = np.ascontiguousarray(t[1], dtype=np.float32).reshape(-1, 3)
            dn = np.ascontiguousarray(t[2], dtype=np.float32).reshape(-1, 3) if len(t) > 2 and t[2] is not None else None
            if dp.shape[0] != idx.size or (dn is not None and dn.shape[0] != idx.size):
                raise ValueError(f"target {k}: {idx.size} indices, {dp.shape[0]} position deltas"
                                 + (f", {dn.shape[0]} normal deltas" if dn is not None else ""))
            keep.append((idx, dp, dn))
            recs[k] = MorphSparseTarget(idx.ctypes.data if idx.size else None, dp.ctypes.data if idx.size else None,
                                        dn.ctypes.data if dn is not None and idx.size else None, idx.size)
        nv = self._scene_vertices if vertex_count is None else int(vertex_count)
        s = MorphSparse(recs, nv, len(targets), 0)
        self._check(self._L.swr_scene_morph_sparse(self._h, ctypes.byref(s)))

    def morph_pose_set(self, weights: "np.ndarray | None", joints: "np.ndarray | None", dq: bool = False, pose_kind: "int | None" = None):
        """swr_morph_pose_set: morph_set(weights), then pose_set(joints) — dq: pose_set_dq(joints) — as one call: every argument of
        both is checked before anything changes, and the scene is rewritten once.  None means what it means in the two calls.
        pose_kind: the SWR_POSE_* value to pass as it is (default: the one `dq` names)."""
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        j = None if joints is None else np.ascontiguousarray(joints, dtype=np.float32).reshape(-1, 8 if dq else 16)
        self._check(self._L.swr_morph_pose_set(self._h, w.ctypes.data if w is not None else None, w.shape[0] if w is not None else 0,
                                               j.ctypes.data if j is not None else None, j.shape[0] if j is not None else 0,
                                               (POSE_DUAL_QUATS if dq else POSE_MATRICES) if pose_kind is None else int(pose_kind)))

    def scene_normals(self, mode: "int | str | None", flip: bool = False):
        """swr_scene_normals: the resident scene's normals as uploaded (NORMALS_UPLOADED, "uploaded"; None passes NULL), or computed on
        the device from the positions that are drawn — per vertex (NORMALS_SMOOTH, "smooth") or per triangle (NORMALS_FLAT, "flat");
        flip: the face vectors the other way round (SWR_NORMALS_FLIP)."""
        if mode is None:
            self._check(self._L.swr_scene_normals(self._h, None))
            return
        n = Normals(NORMALS_MODES[mode] if isinstance(mode, str) else int(mode), NORMALS_FLIP if flip else 0, (ctypes.c_int32 * 2)(0, 0))
        self._check(self._L.swr_scene_normals(self._h, ctypes.byref(n)))

    def material_set(self, material: "Material | None"):
        self._check(self._L.swr_material_set(self._h, ctypes.byref(material) if material is not None else None))

    def blend_set(self, mode: int = BLEND_OVER, opacity: int = 255, blend: "Blend | None" = None, default: bool = False):
        """swr_blend_set: the state of every later FLAG_BLEND frame (BLEND_OVER / BLEND_ADD, opacity 0..255); a ready-made Blend
        is passed as it is; default=True passes NULL (OVER, opacity 255)."""
        if default:
            self._check(self._L.swr_blend_set(self._h, None))
            return
        b = blend if blend is not None else Blend(int(mode), int(opacity), (ctypes.c_int32 * 2)(0, 0))
        self._check(self._L.swr_blend_set(self._h, ctypes.byref(b)))

    def texture_upload(self, texture: np.ndarray):
        t = np.ascontiguousarray(texture, dtype=np.uint8)
        assert t.ndim == 3 and t.shape[2] == 4
        self._check(self._L.swr_texture_upload(self._h, t.ctypes.data, t.shape[1], t.shape[0]))

    def shading_set(self, shading):
        """attributes + material + texture of a scenes.Shading (None: back to the reference's stage)."""
        if shading is None:
            self.material_set(None)
            return
        self.scene_attributes(shading.attrs)
        if shading.texture is not None:
            self.texture_upload(shading.texture)
        self.material_set(Material.from_shading(shading))

    def target_set(self, width: int, height: int, row_begin: int = 0, row_end: int | None = None):
        if row_end is None:
            row_end = height
        self._check(self._L.swr_target_set(self._h, width, height, row_begin, row_end))
        self.width, self.height, self.row_begin, self.row_end = width, height, row_begin, row_end

    def draw(self, transform: np.ndarray, flags: int = 0, primitive_type: int = 0):
        # the frame loop calls this thousands of times a second: keep the host side of a draw to one ctypes call
        # (converting the matrix costs more than the call; the same array object is not converted twice)
        # (a float32 C-contiguous array is passed by its own buffer, so the pointer of the same array object can be
        # re-used — in-place updates of that array are seen; anything else is converted on every call)
        if transform is not self._m_src:
            if (isinstance(transform, np.ndarray) and transform.dtype == np.float32 and transform.size == 16
                    and transform.flags.c_contiguous):
                self._m_src, self._m = transform, transform
            else:
                self._m_src, self._m = None, np.ascontiguousarray(transform, dtype=np.float32).reshape(16)
            self._m_ptr = self._m.ctypes.data
        rc = self._L.swr_draw_primitives(self._h, self._m_ptr, flags, primitive_type)
        if rc:
            self._check(rc)
        self._last_list = None

    @staticmethod
    def draw_items(items) -> np.ndarray:
        """A draw list as the structured array swr_draw_list reads (DRAW_ITEM_DTYPE, 80 bytes per item): from such an array
        itself, or from (first_index, index_count, transform) tuples."""
        if isinstance(items, np.ndarray) and items.dtype == DRAW_ITEM_DTYPE:
            return np.ascontiguousarray(items)
        items = list(items)
        a = np.zeros(len(items), dtype=DRAW_ITEM_DTYPE)
        for k, (first, count, transform) in enumerate(items):
            a[k]["first_index"] = first
            a[k]["index_count"] = count
            a[k]["transform"] = np.asarray(transform, dtype=np.float32).reshape(16)
        return a

    def draw_list(self, items, flags: int = 0):
        """swr_draw_list: one frame of several draws, each an index range with its own transform (include/swr.h).  `items`:
        (first_index, index_count, transform) tuples or a DRAW_ITEM_DTYPE array.  The list is copied by the call."""
        a = self.draw_items(items)
        self._check(self._L.swr_draw_list(self._h, a.ctypes.data if a.size else None, a.size, flags))
        self._last_list = (int((a["index_count"] // 3).sum()), int(a.size))

    def sync(self):
        self._check(self._L.swr_sync(self._h))

    def target_write(self, color=None, depth=None):
        """swr_target_write: the band's current image (what the next FLAG_LOAD frame starts from) := the rows of these full-size
        images (uint8 (height, width, 4) BGRA / float32 (height, width); a HostImage too); None keeps that image."""
        def ptr(a, dtype):
            if a is None:
                return None, None
            arr = a.array if hasattr(a, "array") else a
            if not (isinstance(arr, np.ndarray) and arr.dtype == dtype and arr.flags.c_contiguous):
                arr = np.ascontiguousarray(arr, dtype=dtype)
            if arr.size != self.width * self.height * (4 if dtype == np.uint8 else 1):
                raise ValueError("target_write: the image must have the target's full size")
            return arr.ctypes.data, arr
        cp, keep_c = ptr(color, np.uint8)
        dp, keep_d = ptr(depth, np.float32)
        self._check(self._L.swr_target_write(self._h, cp, dp))

    def bands(self):
        """[(device, row_begin, row_end)] of every band of the context."""
        out = []
        for k in range(self._L.swr_context_bands(self._h)):
            d, a, b = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
            self._check(self._L.swr_context_band_info(self._h, k, ctypes.byref(d), ctypes.byref(a), ctypes.byref(b)))
            out.append((d.value, a.value, b.value))
        return out

    def present(self, color=None, depth=None):
        """Enqueue the async copy of the last drawn frame into the caller's full-size images (NumPy arrays or
        HostImages; page-locked ones make the call non-blocking).  present_wait() makes the pixels visible."""
        def ptr(x):
            if x is None:
                return None
            return x.ptr if isinstance(x, HostImage) else x.ctypes.data
        # the C side writes into these later (DMA, or the helper thread's staged memcpy): keep them alive until the copies
        # have landed (a HostImage refuses to be freed meanwhile).  Registered before the call — a copy may be in flight the
        # moment it returns — and taken back if the call enqueued nothing; one entry per image however many frames present it.
        added = [x for x in (color, depth) if x is not None and id(x) not in self._present_refs]
        for x in added:
            self._present_refs[id(x)] = x
            if isinstance(x, HostImage):
                x._busy.add(id(self))
        rc = self._L.swr_present(self._h, ptr(color), ptr(depth))
        if rc:
            if rc in (ERR_BAD_ARG, ERR_NO_SCENE):          # refused before anything was enqueued
                for x in added:
                    del self._present_refs[id(x)]
                    if isinstance(x, HostImage):
                        x._busy.discard(id(self))
            self._check(rc)

    def _release_presents(self):
        for x in self._present_refs.values():
            if isinstance(x, HostImage):
                x._busy.discard(id(self))
        self._present_refs = {}

    def present_wait(self):
        try:
            self._check(self._L.swr_present_wait(self._h))
        finally:
            self._release_presents()

    def render_timings(self) -> dict:
        t = RenderTimes()
        self._check(self._L.swr_render_timings(self._h, ctypes.byref(t)))
        return t.as_dict()

    def debug_set(self, key: int, value: int):
        """Test hooks (swr_debug_set): force a code path for this context; results never depend on them."""
        self._check(self._L.swr_debug_set(self._h, int(key), ctypes.c_int64(int(value))))

    def debug_fault(self, fault: int):
        """Fault injection for the failure-path tests (FAULT_LOST_EVENT / FAULT_ENQUEUE)."""
        self._check(self._L.swr_debug_fault(self._h, int(fault)))

    def read_color(self, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        assert out.flags.c_contiguous and out.nbytes == self.width * self.height * 4
        self._check(self._L.swr_read_color(self._h, out.ctypes.data))
        return out

    def read_depth(self, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.zeros((self.height, self.width), dtype=np.float32)
        assert out.flags.c_contiguous and out.nbytes == self.width * self.height * 4
        self._check(self._L.swr_read_depth(self._h, out.ctypes.data))
        return out

    def read_ids(self, out: np.ndarray | None = None) -> np.ndarray:
        """swr_read_ids: the ID image of the last frame, drawn with FLAG_PRIMITIVE_IDS — (height, width) uint32, the triangle (draw
        lists: the position in the concatenation of the items) visible at every pixel, ID_NONE where the frame kept no fragment."""
        if out is None:
            out = np.zeros((self.height, self.width), dtype=np.uint32)
        assert out.flags.c_contiguous and out.nbytes == self.width * self.height * 4
        self._check(self._L.swr_read_ids(self._h, out.ctypes.data))
        return out

    def count_ids(self, group: int = COUNT_PER_PRIMITIVE, rect=None, n: int | None = None, query: "IdCount | None" = None):
        """swr_count_ids: the ID image of the last frame reduced on the device — (counts, none): counts[p] the pixels of the rectangle
        that show primitive p (COUNT_PER_PRIMITIVE) or counts[k] those that show a triangle of draw item k (COUNT_PER_ITEM; a frame
        that was no draw list is one item), uint32, and the number of pixels with ID_NONE.  `rect` = (x0, y0, x1, y1), half-open, in
        pixels of the full target; None: the whole target.  `n` defaults to what the context last drew.  A ready-made IdCount is
        passed as it is."""
        if query is None:
            x0, y0, x1, y1 = rect if rect is not None else (0, 0, self.width, self.height)
            query = IdCount(int(group), int(x0), int(y0), int(x1), int(y1), (ctypes.c_int32 * 3)(0, 0, 0))
        if n is None:
            prims, items = self._last_list if self._last_list is not None else (self._scene_prims, 1)
            n = items if query.group == COUNT_PER_ITEM else prims
        counts = np.zeros(max(int(n), 0), dtype=np.uint32)
        none = ctypes.c_uint32(0)
        self._check(self._L.swr_count_ids(self._h, ctypes.byref(query), counts.ctypes.data if counts.size else None, int(n),
                                          ctypes.byref(none)))
        return counts, int(none.value)

    @staticmethod
    def depth_boxes(boxes) -> np.ndarray:
        """A DEPTH_BOX_DTYPE array from an (n, 5) array of rows (x0, y0, x1, y1, z) — the rectangle's numbers must be integers — or a
        DEPTH_BOX_DTYPE array, which is passed as it is (reserved words included)."""
        if isinstance(boxes, np.ndarray) and boxes.dtype == DEPTH_BOX_DTYPE:
            return np.ascontiguousarray(boxes).reshape(-1)
        rows = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)
        a = np.zeros(rows.shape[0], dtype=DEPTH_BOX_DTYPE)
        for j, f in enumerate(("x0", "y0", "x1", "y1")):
            if not (rows[:, j] == np.rint(rows[:, j])).all():
                raise ValueError("depth_boxes: the rectangles are in whole pixels")
            a[f] = rows[:, j].astype(np.int32)
        a["z"] = rows[:, 4].astype(np.float32)
        return a

    def query_depth(self, boxes) -> np.ndarray:
        """swr_query_depth: uint32[n], for every box the number of its pixels where its z would pass the strict z-test against the
        depth image as it is now (z < depth).  `boxes`: an (n, 5) array of rows (x0, y0, x1, y1, z), the rectangle half-open and in
        pixels of the full target, or a DEPTH_BOX_DTYPE array."""
        a = self.depth_boxes(boxes)
        passed = np.zeros(a.size, dtype=np.uint32)
        self._check(self._L.swr_query_depth(self._h, a.ctypes.data if a.size else None, a.size, passed.ctypes.data if a.size else None))
        return passed

    def item_bounds(self, items, flags: int = 0) -> np.ndarray:
        """swr_item_bounds: an ITEM_BOUND_DTYPE array, for every item of `items` (as for draw_list) the rectangle it would land in on
        the target, the depth range of its vertices and its drawable / skipped / behind triangle counts, computed on the device from
        the resident scene as it is now (morphed and posed).  Only FLAG_METAL_RULES of `flags` changes the result."""
        a = self.draw_items(items)
        out = np.zeros(a.size, dtype=ITEM_BOUND_DTYPE)
        self._check(self._L.swr_item_bounds(self._h, a.ctypes.data if a.size else None, a.size, flags, out.ctypes.data if a.size else None))
        return out

    def cast_rays(self, rays) -> np.ndarray:
        """swr_cast_rays: a RAY_HIT_DTYPE array, for every ray its nearest hit on the resident triangles as they are now (morphed and
        posed), in object space; a miss has primitive == ID_NONE and t = u = v = 0.  `rays`: a RAY_DTYPE array (pixel_ray makes them),
        or an (n, 8) float array of rows (origin xyz, tmin, dir xyz, tmax)."""
        a = np.asarray(rays)
        if a.dtype != RAY_DTYPE:
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 8).view(RAY_DTYPE).reshape(-1)
        a = np.ascontiguousarray(a).reshape(-1)
        out = np.zeros(a.size, dtype=RAY_HIT_DTYPE)
        self._check(self._L.swr_cast_rays(self._h, a.ctypes.data if a.size else None, a.size, 0, out.ctypes.data if a.size else None))
        return out

    def query_rays(self, rays, any_hit: bool = False, cull: "str | None" = None, front_cw: bool = False, first_primitive: int = 0,
                   primitive_count: int = -1) -> np.ndarray:
        """swr_query_rays: cast_rays restricted to the primitives [first_primitive, first_primitive + primitive_count) (-1: to the end
        of the scene; for a draw item first_index // 3 and index_count // 3) and to one facing (`cull`: None, "back", "front" or
        "both"; front-facing means counter-clockwise seen from the ray's origin, clockwise with `front_cw`).  With `any_hit` the
        answer is one bit per ray: primitive == RAY_OCCLUDED when anything is hit, ID_NONE otherwise, and t = u = v = 0.  The
        defaults are cast_rays itself."""
        a = np.asarray(rays)
        if a.dtype != RAY_DTYPE:
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 8).view(RAY_DTYPE).reshape(-1)
        a = np.ascontiguousarray(a).reshape(-1)
        q = np.zeros(1, dtype=RAY_QUERY_DTYPE)
        q["flags"] = (RAYS_ANY_HIT if any_hit else 0) | RAYS_CULL[cull] | (RAYS_FRONT_CW if front_cw else 0)
        q["first_primitive"], q["primitive_count"] = first_primitive, primitive_count
        out = np.zeros(a.size, dtype=RAY_HIT_DTYPE)
        self._check(self._L.swr_query_rays(self._h, q.ctypes.data, a.ctypes.data if a.size else None, a.size,
                                           out.ctypes.data if a.size else None))
        return out

    @staticmethod
    def _dst_ptr(x):
        return x.ptr if isinstance(x, HostImage) else x.ctypes.data

    def _read_delta(self, fn, out) -> DeltaStats:
        arr = out.array if isinstance(out, HostImage) else out
        assert arr.flags.c_contiguous and arr.nbytes == self.width * self.height * 4
        st = DeltaStats()
        self._check(fn(self._h, self._dst_ptr(out), ctypes.byref(st)))
        return st

    def read_color_delta(self, out) -> DeltaStats:
        """swr_read_color_delta: `out` — a (height, width, 4) uint8 NumPy array or HostImage that still holds what the last
        read_color_delta delivered — becomes what read_color would deliver now; only the rectangle around the tiles that changed is
        written (the whole band the first time).  Returns what was done."""
        return self._read_delta(self._L.swr_read_color_delta, out)

    def read_depth_delta(self, out) -> DeltaStats:
        """swr_read_depth_delta: read_color_delta for the (height, width) float32 depth image; its baseline is its own."""
        return self._read_delta(self._L.swr_read_depth_delta, out)

    def delta_reset(self, images: int = DELTA_COLOR | DELTA_DEPTH):
        """swr_delta_reset: drop the baselines named by the DELTA_* bits; the next delta read of those kinds delivers the whole band."""
        self._check(self._L.swr_delta_reset(self._h, int(images)))

    def read_color_resolved(self, factor: int, out=None, resolve: "Resolve | None" = None) -> np.ndarray:
        """swr_read_color_resolved: the last frame's colour image through the factor x factor box filter, computed on the device —
        (height / factor, width / factor, 4) uint8; alpha is the coverage of the pixel.  `out`: a NumPy array or a HostImage of that
        size; rows outside the context's band(s) are left untouched.  A ready-made Resolve is passed as it is."""
        r = resolve if resolve is not None else Resolve(int(factor), RESOLVE_DEPTH_SAMPLE0, (ctypes.c_int32 * 2)(0, 0))
        f = max(1, int(r.factor))
        if out is None:
            out = np.zeros((self.height // f, self.width // f, 4), dtype=np.uint8)
        arr = out.array if isinstance(out, HostImage) else out
        assert arr.flags.c_contiguous and (arr.nbytes == (self.width // f) * (self.height // f) * 4 or (resolve is not None and out is not None))
        self._check(self._L.swr_read_color_resolved(self._h, ctypes.byref(r), self._dst_ptr(out)))
        return arr

    def read_depth_resolved(self, factor: int, depth_filter: int = RESOLVE_DEPTH_SAMPLE0, out=None,
                            resolve: "Resolve | None" = None) -> np.ndarray:
        """swr_read_depth_resolved: (height / factor, width / factor) float32 — sample (0,0) of every block (RESOLVE_DEPTH_SAMPLE0)
        or the block's minimum, NaNs losing (RESOLVE_DEPTH_MIN)."""
        r = resolve if resolve is not None else Resolve(int(factor), int(depth_filter), (ctypes.c_int32 * 2)(0, 0))
        f = max(1, int(r.factor))
        if out is None:
            out = np.zeros((self.height // f, self.width // f), dtype=np.float32)
        arr = out.array if isinstance(out, HostImage) else out
        assert arr.flags.c_contiguous and (arr.nbytes == (self.width // f) * (self.height // f) * 4 or (resolve is not None and out is not None))
        self._check(self._L.swr_read_depth_resolved(self._h, ctypes.byref(r), self._dst_ptr(out)))
        return arr

    def timing_enable(self, level=2):
        """0/False off, 1 = events around k_raster only, 2/True = around every stage."""
        level = 2 if level is True else (0 if level is False else int(level))
        self._check(self._L.swr_timing_enable(self._h, level))

    def timing_sample(self, every_nth: int):
        """Level-1 timing brackets only every n-th frame's k_raster."""
        self._check(self._L.swr_timing_sample(self._h, int(every_nth)))

    def timings(self) -> dict:
        t = Timings()
        self._check(self._L.swr_get_timings(self._h, ctypes.byref(t)))
        return t.as_dict()

    def timing_totals(self):
        """(sums dict, frames) over every frame since timing_reset()."""
        t, n = Timings(), ctypes.c_int64()
        self._check(self._L.swr_timing_totals(self._h, ctypes.byref(t), ctypes.byref(n)))
        return t.as_dict(), n.value

    def pipeline_enable(self, on: bool = True):
        """Overlap binning of the next frame with the raster of the previous one (default on)."""
        self._check(self._L.swr_pipeline_enable(self._h, 1 if on else 0))

    def timing_reset(self):
        self._check(self._L.swr_timing_reset(self._h))

    # -- one-shot path: Renderer.render(renderPass:) / GpuRenderer.render(renderPass:) -----
    def render(self, vertices, indices, transform, width, height, flags=0, primitive_type=0,
               color=None, depth=None, shading=None, scene_id=0):
        return self._render(None, vertices, indices, transform, width, height, flags, primitive_type, color, depth, shading, scene_id)

    def render_resolved(self, vertices, indices, transform, width, height, flags=0, primitive_type=0,
                        color=None, depth=None, shading=None, scene_id=0, factor=2, depth_filter=RESOLVE_DEPTH_SAMPLE0):
        """swr_render_resolved: Context.render with (width, height, color, depth) describing the DESTINATION; the frame is drawn at
        factor * width x factor * height and resolved on the device (include/swr.h "Supersampled resolve").  FLAG_LOAD is refused."""
        r = Resolve(int(factor), int(depth_filter), (ctypes.c_int32 * 2)(0, 0))
        return self._render(r, vertices, indices, transform, width, height, flags, primitive_type, color, depth, shading, scene_id)

    def render_delta(self, vertices, indices, transform, width, height, color, depth, flags=0, primitive_type=0,
                     shading=None, scene_id=0):
        """swr_render_delta: Context.render whose gather is the two delta reads.  `color` (None under FLAG_NO_COLOR) and `depth` — NumPy
        arrays or HostImages — still hold what the last render_delta into them delivered.  FLAG_LOAD is refused.  Returns
        (colour DeltaStats, depth DeltaStats)."""
        stats = (DeltaStats * 2)()
        self._render(None, vertices, indices, transform, width, height, flags, primitive_type, color, depth, shading, scene_id, delta=stats)
        return stats[0], stats[1]

    def _render(self, resolve, vertices, indices, transform, width, height, flags, primitive_type, color, depth, shading, scene_id,
                delta=None):
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 8)
        i = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        m = np.ascontiguousarray(transform, dtype=np.float32).reshape(16)
        if resolve is None and (flags & FLAG_LOAD) and (depth is None or (color is None and not (flags & FLAG_NO_COLOR))):
            raise ValueError("render with FLAG_LOAD: color / depth are the starting image and must be given")
        if delta is not None and (depth is None or (color is None and not (flags & FLAG_NO_COLOR))):
            raise ValueError("render_delta: color / depth hold what the last call delivered and must be given")
        if color is None and not (flags & FLAG_NO_COLOR):
            color = np.full((height, width, 4), 0xCD, dtype=np.uint8)
        if depth is None:
            depth = np.full((height, width), -123.0, dtype=np.float32)
        rp = RenderPass()
        rp.color = self._dst_ptr(color) if color is not None else None
        rp.depth = self._dst_ptr(depth)
        rp.width, rp.height = width, height
        rp.color_bytes_per_row = width * 4
        rp.depth_bytes_per_row = width * 4
        rp.vertices, rp.vertex_count = v.ctypes.data, v.shape[0]
        rp.indices, rp.index_count = i.ctypes.data, i.size
        rp.primitive_type, rp.flags = primitive_type, flags
        rp.scene_id = int(scene_id)
        rp.transform = (ctypes.c_float * 16)(*m.tolist())
        if shading is not None:
            a = np.ascontiguousarray(shading.attrs, dtype=np.float32).reshape(-1, 8)
            mat = Material.from_shading(shading)
            rp.attributes = a.ctypes.data
            rp.material = ctypes.addressof(mat)
            if shading.texture is not None:
                t = np.ascontiguousarray(shading.texture, dtype=np.uint8)
                rp.texture, rp.tex_width, rp.tex_height = t.ctypes.data, t.shape[1], t.shape[0]
        if delta is not None:
            self._check(self._L.swr_render_delta(self._h, ctypes.byref(rp), delta))
            S = 1
        elif resolve is None:
            self._check(self._L.swr_render(self._h, ctypes.byref(rp)))
            S = 1
        else:
            self._check(self._L.swr_render_resolved(self._h, ctypes.byref(rp), ctypes.byref(resolve)))
            S = int(resolve.factor)      # the target is the supersampled one: read_ids delivers S * width x S * height words
        self.width, self.height, self.row_begin, self.row_end = S * width, S * height, 0, S * height     # (swr_render sets the target: read_ids)
        self._scene_prims, self._last_list = i.size // 3, None
        self._scene_vertices = v.shape[0]
        return color, depth


def render(scene, extra_flags: int = 0, device: int = -1):
    """Convenience: one-shot render of a scenes.Scene; returns (color, depth)."""
    with Context(device) as ctx:
        return ctx.render(scene.vertices, scene.indices, scene.transform, scene.width, scene.height,
                          scene.flags | extra_flags, shading=scene.shading)


def list_ids_to_items(ids: np.ndarray, items) -> tuple[np.ndarray, np.ndarray]:
    """Map the ID image of a draw-list frame (Context.read_ids after Context.draw_list) to (item, triangle-in-item) arrays of the
    same shape: item k's j-th triangle has the ID vbase_k + j, vbase_k = the sum of index_count / 3 of the items before it (a
    search over the vbases).  Pixels with ID_NONE get -1 in both.  `items`: what was passed to draw_list."""
    a = Context.draw_items(items)
    counts = (a["index_count"] // 3).astype(np.int64)
    vbase = np.concatenate([[0], np.cumsum(counts)[:-1]]) if counts.size else np.zeros(0, np.int64)
    ids = np.asarray(ids)
    live = ids != ID_NONE
    v = ids.astype(np.int64)
    # the last item whose vbase is <= the ID and that has triangles (empty items share their vbase with the next one)
    nonempty = np.nonzero(counts > 0)[0]
    k = np.full(ids.shape, -1, dtype=np.int64)
    j = np.full(ids.shape, -1, dtype=np.int64)
    if nonempty.size:
        pos = np.searchsorted(vbase[nonempty], v[live], side="right") - 1
        kk = nonempty[np.clip(pos, 0, None)]
        k[live] = kk
        j[live] = v[live] - vbase[kk]
    return k, j
