"""The sizes of a target at which the library changes its path: include/swr.h accepts targets up to 65535 x 65535, and between the
largest target older tests draw on (7680 x 4320, 120 x 135 tiles) and that limit the code switches on a triangle's extent (16-bit
vertex deltas, the dense walk's 15-bit bound), on a coordinate's width (the 16-bit halves of a packed box) and on the number of tiles
(the LDS binning paths, the dynamic LDS above 64 KB, k_scan's tiles per thread).  A plain helper module of
tests/test_large_targets.py (which takes its targets and its scene from here, so that the sizes drawn are the sizes checked) and of
tests/test_target_sizes_table.py (which reads the constants out of the sources and fails when a threshold is retuned past a case, a
kernel with more than 64 KB of dynamic LDS is missing from prepare_device, or a row's case is gone).  Not a conftest, not a test file.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import kernel_matrix as K

TILE_W, TILE_H = K.TILE_W, K.TILE_H
MAX_DIM = 65535                                     # check_target_args, include/swr.h
LDS_DEFAULT = 65536                                 # dynamic LDS a kernel may ask for without hipFuncAttributeMaxDynamicSharedMemorySize

# name -> (width, height): the smallest targets that cross each threshold (tile grid in the comment)
TARGETS = {
    "WIDE": (65535, 96),                            # 1024 x 3
    "TALL": (96, 65535),                            # 2 x 2048
    "X16K": (16448, 64),                            # 257 x 2
    "EXACT": (65535, 544),                          # 1024 x 17 = 17 408
    "LDS_TOP": (65535, 1088),                       # 1024 x 34 = 34 816
    "ATOMIC": (65535, 1089),                        # 1024 x 35 = 35 840
}
RESOLVED = {"WIDE": (65532, 96), "TALL": (96, 65532)}      # divisible by 2 and by 4
SMALL_TRIANGLES = 2000
LONG_TRIANGLES = 14                                 # six thin ones, two pairs, the corner triangle, the sliver, two duplicates


def tiles(name_or_size):
    w, h = TARGETS[name_or_size] if isinstance(name_or_size, str) else name_or_size
    return ((w + TILE_W - 1) // TILE_W) * ((h + TILE_H - 1) // TILE_H)


@dataclasses.dataclass(frozen=True)
class Threshold:
    """One size at which the path changes.

    key        the row's name; tests/test_large_targets.py names the rows each case crosses (CROSSES)
    file, function   where the constant stands
    constant   the constant as written there (tests/test_target_sizes_table.py finds it in the function's text)
    unit       what is compared with it
    below, above     the largest size on the old side and the smallest on the new one, in `unit`
    case       node id of the GPU test that reaches `above` or beyond, at_least: the size it reaches
    mutation   the line of profiles/large_targets/mutations.txt that this case fails, or why there is no safe one
    """
    key: str
    file: str
    function: str
    constant: str
    unit: str
    below: int
    above: int
    case: str
    at_least: int
    mutation: str


T = "tests/test_large_targets.py::"
_API, _KRN = "swr_api.hip", "swr_kernels.hip"

ROWS = [
    Threshold("small_x", _KRN, "setup_triangle_r", "(int64_t)maxx - (int64_t)minx < 32768", "x extent of a triangle in pixels",
              32767, 32768, T + "test_frames[WIDE]", 65529, "small bound raised to 65536"),
    # (TILE_H lower than in x: the dense walk keeps C.y relative to the tile's first row in 16 bits, and a tile starts up to TILE_H - 1
    # rows above the triangle.  The bound was 32768 until this table's TALL case failed: Scene.pair)
    Threshold("small_y", _KRN, "setup_triangle_r", "(int64_t)s2y - (int64_t)s0y < 32768 - TILE_H", "y extent of a triangle in pixels",
              32735, 32736, T + "test_frames[TALL]", 65529, "small bound raised to 65536"),
    Threshold("dense_x", _KRN, "raster_tile", "maxx - minx >= 16384", "x extent of a GEOM_SMALL triangle in pixels",
              16383, 16384, T + "test_x16k", 16384, "`maxx - minx >= 16384` dropped from big"),
    Threshold("box_x", _KRN, "unpack_box", "b.x1 = r.x >> 16", "x1 of a packed box: the bits above the 15th",
              32767, 32768, T + "test_frames[WIDE]", 65534, "x1 masked to 15 bits in unpack_box"),
    Threshold("box_y", _KRN, "unpack_box", "b.y1 = r.y >> 16", "y1 of a packed box relative to its band: the bits above the 15th",
              32767, 32768, T + "test_frames[TALL]", 65534,
              "none built: y1 feeds the same unpack as x1 (one line); the x1 mutation stands for both"),
    Threshold("plan_lds", _KRN, "plan_binning", "p.lds_bytes <= 136 * 1024", "tiles of a band",
              34816, 34817, T + "test_tile_counts[ATOMIC-DT]", 35840, "none needed: test_tile_counts[LDS_TOP-*] and [ATOMIC-*] compare "
              "timings()['tiles'] and every image on both sides; a moved bound is caught by tests/test_target_sizes_table.py"),
    Threshold("plan_groups", _KRN, "plan_binning", "> 150 * 1024", "bytes: tiles * 4 + (groups per workgroup + 1) * 4",
              150 * 1024, 150 * 1024 + 1, "", 0,
              "not crossed: at 34 816 tiles it takes 3 584 groups of 64 per workgroup, 58.7 M triangles; no test draws that many"),
    Threshold("scan_per", _KRN, "k_scan", "(n + 1023) / 1024", "tiles of a band: tiles per thread of the one workgroup",
              1024, 1025, T + "test_tile_counts[ATOMIC-DT]", 35840, 
              "k_scan: `run` no longer advances (caught once; the build then faulted and is not to be built again)"),
    Threshold("bin_lds", _KRN, "launch_bin", "(size_t)((b.ntiles + 1) / 2) * 4 + (size_t)(b.per + 1) * 4 + 2 * (256 / 64) * 4 + 4",
              "bytes of dynamic LDS of k_bin", LDS_DEFAULT, LDS_DEFAULT + 1, T + "test_tile_counts[LDS_TOP-DT]", 69632,
              "none built: prepare_device without the k_bin rows is not shown to keep the frame's later kernels in range "
              "(profiles/large_targets/mutations.txt); tests/test_target_sizes_table.py drops them from a copy of the source instead"),
    Threshold("fill_lds", _KRN, "launch_fill", "f.plan.lds_bytes + 4 * 256", "bytes of dynamic LDS of k_fill_lds",
              LDS_DEFAULT, LDS_DEFAULT + 1, T + "test_tile_counts[EXACT-DT]", 17408 * 4 + 1024, 
              "none built: prepare_device without the k_fill_lds row, as for k_bin; dropped from a copy of the source instead"),
    Threshold("hist_lds", _KRN, "launch_setup_bin", "(h16 ? (size_t)((ntiles + 1) / 2) * 4 : f.plan.lds_bytes) + (size_t)(per + 1) * 4",
              "bytes of dynamic LDS of k_setup_hist", LDS_DEFAULT, LDS_DEFAULT + 1, T + "test_tile_counts[LDS_TOP-exact]", 69632,
              "none built: the same hipFuncSetAttribute call as the k_fill_lds row, two lines above it"),
]
BY_KEY = {r.key: r for r in ROWS}


# ---- the byte counts of the launches, restated (tests/test_target_sizes_table.py holds them against the expressions in the source) ---
BIN_G, BIN_THREADS = 256, 256                       # SWR_TUNE_BIN_G, plan_binning's threads


def groups_per_workgroup(ntri):
    g = max(1, min((ntri + BIN_THREADS - 1) // BIN_THREADS, BIN_G))
    return ((ntri + 63) // 64 + g - 1) // g


def lds_bytes(kernel, ntiles, ntri):
    per = groups_per_workgroup(ntri)
    if kernel == "k_bin":
        return (ntiles + 1) // 2 * 4 + (per + 1) * 4 + 2 * (256 // 64) * 4 + 4
    if kernel == "k_fill_lds":
        return ntiles * 4 + 4 * 256
    assert kernel == "k_setup_hist"
    return ((ntiles + 1) // 2 * 4 if per * 64 < 65536 else ntiles * 4) + (per + 1) * 4


# ---- the scene ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Scene:
    vertices: np.ndarray        # float32 [nv, 8], de-indexed
    indices: np.ndarray
    long: np.ndarray            # numbers of the triangles that run the length of the long axis
    pair: tuple                 # (triangle of extent E - 1, triangle of extent E), E = 32768 (X16K: 16384)
    pair2: tuple                # (extent E - TILE_H - 1, extent E - TILE_H): the bound of GEOM_SMALL in y
    corner: int                 # the triangle with a vertex in the last column and the last row
    tied: np.ndarray            # [k, 2]: (a long triangle, its duplicate with other colours)
    sliver: int                 # the long det == 0 triangle


def _long_pixels(L, S, E):
    """Corners (position along the long axis, position across it) in pixels of the long triangles of an L x S target: six thin ones of
    extent up to L - 6, two a few pixels thick across all of S, the pair of extent E - 1 and E, the corner triangle, the sliver."""
    m = min(S - 1, 95)                                                     # (on a thicker target they stay thin, spread below)
    thin = [
        [(3, 0.10 * m), (L - 3, 0.12 * m), (3, 0.17 * m)],
        [(L - 4, 0.30 * m), (5, 0.34 * m), (L - 4, 0.39 * m)],
        [(10, 0.20 * m), (L - 15, 0.72 * m), (10, 0.29 * m)],              # across every tile row (column) of the short axis
        [(2, 0.62 * m), (L - 5, 0.69 * m), (L - 5, 0.64 * m)],
        [(L // 2, 0.05 * m), (L - 8, 0.93 * m), (7, 0.90 * m)],            # a wide one: its rows are up to L pixels long
        [(40, 0.80 * m), (L // 3, 0.83 * m), (L - 40, 0.78 * m)],
    ]                                                                      # (three of one winding, three of the other)
    # (the far corner is the third: the dense walk keeps C.x relative to the tile in 16 bits, and the tiles at the near end are
    # E - 1 + 36 pixels from it)
    pair = [
        [(100, 0.42 * m), (100, 0.49 * m), (100 + E - 1, 0.45 * m)],
        [(200, 0.52 * m), (200, 0.59 * m), (200 + E, 0.55 * m)],
        [(300, 0.44 * m), (300, 0.51 * m), (300 + E - TILE_H - 1, 0.47 * m)],
        [(400, 0.54 * m), (400, 0.61 * m), (400 + E - TILE_H, 0.57 * m)],
    ]
    sliver = [[(50, 0.75 * m), (L - 60, 0.75 * m), (L // 2, 0.75 * m)]]
    # each group of a thicker target in a place of its own across it: the first and the last tile row (column) among them
    spread = [0.0, 1.0, 0.5, 0.25, 0.97, 0.75, 0.1, 0.6, 0.15, 0.65, 0.4]
    groups = thin + pair + sliver
    for g, f in zip(groups, spread):
        g[:] = [(a, c + np.floor(f * (S - 1 - m))) for a, c in g]
    # inside the last tile of a 65535-pixel axis, with edges along the last row and the last column
    corner = [[(L - 0.5, S - 0.5), (L - 30, S - 0.5), (L - 0.5, S - 30.5)]]
    return thin, pair, corner, sliver


def scene(name, seed=0x7A2):
    """The scene of a target: SMALL_TRIANGLES small triangles all over it, then the long ones among them (so that order numbers on
    both sides of them exist), duplicates of two of them with other colours at the end."""
    w, h = TARGETS[name] if name in TARGETS else name
    along_x = w >= h
    L, S = (w, h) if along_x else (h, w)
    E = 16384 if L < 32768 else 32768
    rng = np.random.default_rng(seed)
    thin, pair, corner, sliver = _long_pixels(L, S, E)
    groups = thin + pair + corner + sliver
    n_long = len(groups)
    p = np.asarray(groups, dtype=np.float64)                               # [n, 3, 2]
    centre = np.floor(p) + 0.5                                             # pixel centres: truncation gives the integer meant
    a, c = centre[..., 0], centre[..., 1]
    k_sliver = len(thin) + len(pair) + len(corner)
    c[k_sliver] = c[k_sliver, 0] + np.array([0.0, 0.0, -0.25])            # det == 0 after truncation
    px, py = (a, c) if along_x else (c, a)
    nx, ny = K._ndc(px, py, w, h)
    z = rng.uniform(0.25, 0.75, (n_long, 3))
    z[3] = (-0.2, 0.5, 0.6)                                                # crosses the near plane (SWR_FLAG_DEPTH_CLIP)
    lxyz = np.stack([nx, ny, z], axis=-1).reshape(-1, 3)
    lrgb = rng.uniform(0.0, 1.0, (3 * n_long, 3))
    half = SMALL_TRIANGLES // 2
    sxyz, srgb = K._tris(rng, SMALL_TRIANGLES, 0, 0, w, h, 7, 0.0, 1.0, w, h)
    first = half
    tied_of = np.array([0, 2])
    dxyz = lxyz.reshape(-1, 3, 3)[tied_of].reshape(-1, 3)
    drgb = 1.0 - lrgb.reshape(-1, 3, 3)[tied_of].reshape(-1, 3)[:, ::-1]
    xyz = np.concatenate([sxyz[:3 * half], lxyz, sxyz[3 * half:], dxyz])
    rgb = np.concatenate([srgb[:3 * half], lrgb, srgb[3 * half:], drgb])
    v = K._pack(xyz, rgb)
    n = v.shape[0] // 3
    k = len(thin)
    return Scene(v, np.arange(v.shape[0], dtype=np.int64), first + np.arange(k + 4), (first + k, first + k + 1),
                 (first + k + 2, first + k + 3), first + k + 4, np.stack([first + tied_of, n - 2 + np.arange(2)], axis=1), first + k + 5)


def extents(oracle, v, i, m, w, h):
    """(x extent, y extent) of every triangle's truncated screen vertices, as setup_triangle_r computes them (int64)."""
    sx, sy, _ = oracle.project(v, m, w, h)
    t = np.asarray(i, dtype=np.int64).reshape(-1, 3)
    ix, iy = np.trunc(sx.astype(np.float64)).astype(np.int64)[t], np.trunc(sy.astype(np.float64)).astype(np.int64)[t]
    return ix.max(axis=1) - ix.min(axis=1), iy.max(axis=1) - iy.min(axis=1)
