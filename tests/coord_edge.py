"""Screen coordinates up to the skip rule's limit: the scenes of tests/test_coord_edge.py and tests/test_coord_edge_model.py.  A plain
helper module like tests/kernel_matrix.py (not a conftest, not a test file).

The skip rule (include/swr.h) draws a primitive whose screen coordinates all satisfy |x|, |y| < 2^30 and skips every
other one.  The edge set mixes about 25 "far" triangles, with corners between 2^17 and the last float below 2^30 on every side of the
target, in index order into 200 ordinary small triangles, on two small targets with one power-of-two side each (on that axis +-2^30
itself is a screen coordinate some NDC float maps to) and ragged last tiles:

    wide  256 x 200        tall  200 x 256

The far classes (FarSet.cls, one letter per far triangle):
  a  one corner at the last reachable coordinate below +2^30 or the nearest above -2^30 (in x, in y, in both), the other two on the
     target: long slivers across it;
  b  three corners off the target near the limits on different sides, the target strictly inside, the depth a plane that crosses the
     small triangles' depths on the target;
  c  extents of 2^31 - 192 pixels on the power-of-two axis and the nearest reachable on the other, at once, in both windings (the second
     one 128 pixels shorter in y, so that a strip of the target between the two stays open under painter's order);
  d  the decades: wedges from a point on the target to two corners at +-2^17, 2^20, 2^24, 2^24 + 2 (the float after 2^24; 2^24 + 1 is
     the first integer a float cannot hold), 2^27 and 0.75 * 2^30 (drawn by the product, skipped by a limit of 2^29);
  e  skipped: a corner at exactly +2^30 and at exactly -2^30 (on the power-of-two axis), at the next reachable coordinate beyond, and near
     3e38; each a class b triangle but for that corner;
  f  covers no pixel: one whose bounding box meets the target while no span does, one whose box misses it;
  g  det == 0 after truncation with a 2^31-scale extent: a one-row span of NaN weights under the CPU rules, skipped under the Metal rules;
  h  an exact duplicate of the last class b triangle in other colours, later in index order.
The Metal variant keeps every far corner on the non-negative side (the Metal rules skip negative coordinates) and adds class
  z  a corner at exactly 0 (the ROI skip) and  n  a negative corner.
The perspective variant is for K.perspective_matrix(): slivers with one vertex whose w is a few float steps above 0, found by a seeded
scan, class  p  where the largest |screen coordinate| is in [2^29, 2^30) and class  q  where it is in [2^30, 2^31).

Everything is laid out in pixels and mapped to NDC by searching the float32 NDC values around the exact preimage for the one the
screen map (one rounding per operation) takes to the coordinate meant; tests/test_coord_edge_model.py checks the result through
oracle.project.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import kernel_matrix as K

TARGETS = {"wide": (256, 200), "tall": (200, 256)}
LIMIT = float(1 << 30)
BELOW = LIMIT - 64.0            # the last float below 2^30
N_SOUP = 200
F32 = np.float32


# ---- pixels -> NDC -----------------------------------------------------------------------------------------------------------------
def screen_of(n, size, flip):
    """The screen map of one NDC coordinate in float32, one rounding per operation (Renderer.swift:166-168)."""
    n = np.asarray(n, dtype=F32)
    with np.errstate(over="ignore"):
        return (n * F32(-0.5 if flip else 0.5) + F32(0.5)) * F32(size)


def ndc_for(p, size, flip, mode="inside"):
    """The NDC float32 whose screen coordinate is, among the floats around the exact preimage of p,
    inside: the farthest from 0 with |s| <= |p|;  beyond: the nearest to 0 with |s| >= |p|;  exact: p itself (asserted)."""
    n0 = F32((2.0 * p / size - 1.0) * (-1.0 if flip else 1.0))
    cand = [n0]
    for direction in (-np.inf, np.inf):
        n = n0
        for _ in range(24):
            n = np.nextafter(n, F32(direction))
            cand.append(n)
    cand = np.array(cand, dtype=F32)
    s = screen_of(cand, size, flip).astype(np.float64)
    if mode == "exact":
        hit = np.nonzero(s == p)[0]
        assert hit.size, f"{p} is not a screen coordinate of a {size}-pixel axis"
        return cand[hit[0]]
    same_side = (np.sign(s) == np.sign(p)) | (p == 0)
    ok = np.nonzero(same_side & ((np.abs(s) <= abs(p)) if mode == "inside" else (np.abs(s) >= abs(p))))[0]
    if ok.size == 0:                         # (near NDC 0 many floats share one screen coordinate: the nearest will do)
        return cand[np.argmin(np.abs(s - p))]
    return cand[ok[np.argmax(np.abs(s[ok]))] if mode == "inside" else ok[np.argmin(np.abs(s[ok]))]]


def _corner(c, w, h):
    """(px, py[, mode x, mode y]) -> NDC (x, y)."""
    px, py = c[0], c[1]
    mx = c[2] if len(c) > 2 else "inside"
    my = c[3] if len(c) > 3 else "inside"
    return ndc_for(px, w, False, mx), ndc_for(py, h, True, my)


def _plane(corners, w, h, z0, gx, gy):
    """Corner depths of the plane z0 + gx (x - w/2) / w + gy (y - h/2) / h: a depth that varies across the target needs corner depths
    of the order of the corners' distance."""
    return [z0 + gx * (c[0] - w / 2) / w + gy * (c[1] - h / 2) / h for c in corners]


@dataclasses.dataclass
class FarSet:
    vertices: np.ndarray      # float32 [3 n, 8], de-indexed
    indices: np.ndarray       # int64 [3 n]
    far: np.ndarray           # the numbers of the far triangles, ascending
    cls: str                  # their classes, one letter each
    twin: tuple               # (class b original, its class h duplicate) as triangle numbers, or ()

    def of(self, letters):
        """The numbers of the far triangles of these classes."""
        return self.far[[k for k, c in enumerate(self.cls) if c in letters]]

    @property
    def triangles(self):
        return self.indices.size // 3


# ---- the far triangles, in pixels ----------------------------------------------------------------------------------------------------
def _tilt(corners, w, h, degrees):
    """Depths of a plane through 0.5 at the target's centre that rises by 0.5 per target size in the direction `degrees` (x right,
    y down): triangles that cover the target get directions of their own, so that each is the nearest one somewhere."""
    t = np.radians(degrees)
    return _plane(corners, w, h, 0.5, 0.5 * np.cos(t), 0.5 * np.sin(t))


def _wedge(corners, w, h, g, qx, qy):
    """Depths of a wedge from corners[0] into the quadrant (qx, qy): 0.5 at its point, nearer by g per target size into the quadrant."""
    ax, ay = corners[0][0], corners[0][1]
    z0 = 0.5 + g * (qx * (ax - w / 2) / w + qy * (ay - h / 2) / h)
    return _plane(corners, w, h, z0, -g * qx, -g * qy)


def _far_cpu(w, h):
    """[(class, [(px, py[, mode x, mode y])] * 3, [z] * 3)] of the CPU-rules edge set, in index order.
    Under painter's order a triangle with the target strictly inside hides everything before it: the class b triangles come first,
    the duplicate (appended by _build right after them) wins that tie, and everything later leaves part of the target open."""
    B, L = BELOW, LIMIT
    pow_x = w == 256                           # the axis on which +-2^30 is reachable exactly
    out = []

    def add(cls, corners, z):
        out.append((cls, corners, _tilt(corners, w, h, z) if np.isscalar(z) else z))

    # b: the target strictly inside, three sides (the last one is duplicated)
    add("b", [(B, B), (-B, 0.45 * L), (0.4 * L, -B)], 90)
    add("b", [(-B, 0.55 * L), (B, 0.3 * L), (0.1 * L, -B)], 180)
    add("b", [(-B, -B), (B, -0.5 * L), (-0.5 * L, B)], 250)
    # c: the largest extents in x and y at once, both windings: below the diagonal y = x, and above y = x - 64
    add("c", [(-B, -B), (B, B), (-B, B)], 315)
    add("c", [(-B, -B), (B, B - 128.0), (B, -B)], 115)
    # d: the decades: wedges from a point on the target to two corners at +-M, the quadrants in turn
    mags = [2.0 ** 17, 2.0 ** 20, 2.0 ** 24, 2.0 ** 24 + 1, 2.0 ** 27, 0.75 * L, 0.75 * L]
    quad = [(1, 1), (-1, 1), (-1, -1), (1, -1)]
    for k, M in enumerate(mags):
        md = "beyond" if M == 2.0 ** 24 + 1 else "inside"
        qx, qy = quad[k % 4]
        f = 0.08 + 0.2 * (k // 4)                # (the corners of the target; a cross through its centre stays open)
        ax, ay = 0.5 * w + qx * f * w, 0.5 * h + qy * f * h
        c = [(ax, ay), (qx * M, -qy * 0.2 * M, md), (-qx * 0.3 * M, qy * M, "inside", md)]
        add("d", c, _wedge(c, w, h, 0.9 if k < 4 else 7.0, qx, qy))
    # a: one far corner, two on the target
    add("a", [(B, 0.30 * h), (0.10 * w, 0.30 * h), (0.12 * w, 0.47 * h)], [0.15, 0.12, 0.2])
    add("a", [(0.60 * w, -B), (0.50 * w, 0.90 * h), (0.72 * w, 0.84 * h)], [0.2, 0.1, 0.25])
    add("a", [(-B, B), (0.80 * w, 0.10 * h), (0.93 * w, 0.24 * h)], [0.1, 0.22, 0.16])
    # e: skipped; class b triangles but for one corner
    exact_p = (L, -0.5 * L, "exact") if pow_x else (0.4 * L, L, "inside", "exact")
    exact_m = (-L, 0.45 * L, "exact") if pow_x else (-0.5 * L, -L, "inside", "exact")
    add("e", [(-B, -B), exact_p, (-0.5 * L, B)] if pow_x else [(-B, -B), (B, -0.5 * L), exact_p], [0.01] * 3)
    add("e", [(B, B), exact_m, (0.4 * L, -B)] if pow_x else [(B, B), (-B, 0.45 * L), exact_m], [0.01] * 3)
    add("e", [(-B, 0.55 * L), (L + 64, 0.3 * L, "beyond"), (0.1 * L, -B)], [0.01] * 3)
    add("e", [(-B, -L - 64, "inside", "beyond"), (B, 0.3 * L), (0.1 * L, B)], [0.01] * 3)
    add("e", [(-B, -B), (3e38, -0.5 * L), (-0.5 * L, B)], [0.01] * 3)
    # f: no pixel.  The box of the first meets the target; the hypotenuse passes 2^26 pixels from it
    M = 2.0 ** 27
    add("f", [(-M, 0.5 * h), (0.5 * w, -M), (-M, -M)], [0.01] * 3)
    add("f", [(B, 2.0 * h), (B - 1e6, 3.0 * h), (w + 10.0, 2.5 * h)], [0.01] * 3)
    # g: collinear after truncation, one row across the target
    y = int(0.37 * h)
    add("g", [(-B, y + 0.25), (B, y + 0.5), (0.3 * L, y + 0.75)], [0.3, 0.4, 0.5])
    return out


def _far_metal(w, h):
    """The Metal variant: every coordinate positive, the target in the corner of the far triangles."""
    B, L = BELOW, LIMIT
    pow_x = w == 256
    out = []

    def add(cls, corners, z):
        out.append((cls, corners, _tilt(corners, w, h, z) if np.isscalar(z) else z))

    add("b", [(3.0, 1.0), (B, 6.0), (9.0, 0.8 * L)], 90)
    add("b", [(1.0, 2.0), (0.6 * L, 9.0), (4.0, 0.7 * L)], 180)
    add("b", [(2.0, 3.0), (B, 5.0), (7.0, B)], 30)
    add("c", [(1.0, 1.0), (B, B), (1.0, B)], 315)
    add("c", [(1.0, 1.0), (B, B - 128.0), (B, 1.0)], 135)
    mags = [2.0 ** 17, 2.0 ** 20, 2.0 ** 24, 2.0 ** 24 + 1, 2.0 ** 27, 0.75 * L]
    for k, M in enumerate(mags):
        md = "beyond" if M == 2.0 ** 24 + 1 else "inside"
        c = [(0.04 * w + 0.08 * w * k, 0.05 * h + 0.08 * h * k), (M, 0.3 * h + 0.1 * h * k, md), (0.2 * w + 0.1 * w * k, M, "inside", md)]
        z = _wedge(c, w, h, 0.4 * 1.6 ** k, 1, 1)
        if k % 2:
            c, z = [c[0], c[2], c[1]], [z[0], z[2], z[1]]
        add("d", c, z)
    add("a", [(B, 0.30 * h), (0.10 * w, 0.30 * h), (0.12 * w, 0.47 * h)], [0.15, 0.12, 0.2])
    add("a", [(0.60 * w, B), (0.50 * w, 0.10 * h), (0.72 * w, 0.16 * h)], [0.2, 0.1, 0.25])
    add("a", [(B, B), (0.30 * w, 0.55 * h), (0.43 * w, 0.52 * h)], [-6.0, -6.1, -5.9])    # (nearer than the wedges there)
    exact_p = (L, 5.0, "exact") if pow_x else (7.0, L, "inside", "exact")
    add("e", [(2.0, 3.0), exact_p, (7.0, B)] if pow_x else [(2.0, 3.0), (B, 5.0), exact_p], [0.01] * 3)
    add("e", [(2.0, 3.0), (L + 64, 5.0, "beyond"), (7.0, B)], [0.01] * 3)
    add("e", [(2.0, 3.0), (B, 5.0), (7.0, 3e38)], [0.01] * 3)
    add("z", [(0.25, 3.0), (B, 5.0), (7.0, B)], [0.01] * 3)           # rounds to 0: the ROI skip
    add("z", [(2.0, 0.0, "inside", "exact"), (B, 5.0), (7.0, B)], [0.01] * 3)
    add("n", [(-3.0, 3.0), (B, 5.0), (7.0, B)], [0.01] * 3)
    add("f", [(B, 2.0 * h), (B - 1e6, 3.0 * h), (w + 10.0, 2.5 * h)], [0.01] * 3)
    y = int(0.37 * h)
    add("g", [(1.0, y), (B, y), (0.3 * L, y)], [0.3, 0.4, 0.5])
    return out


# ---- the sets ----------------------------------------------------------------------------------------------------------------------
def _soup(rng, w, h, n=N_SOUP, z0=-0.5, z1=0.6):
    return K._tris(rng, n, 4, 4, w - 4, h - 4, 16, z0, z1, w, h)


def _mixed(soup, far, rng, twin_of=None):
    """The far triangles in index order among the soup's: one after every few small triangles, the duplicate (class h) of far triangle
    `twin_of` as the next far one after it."""
    sxyz, srgb = soup
    n_soup = sxyz.shape[0] // 3
    fx = [np.asarray(f[0], dtype=np.float64) for f in far]
    fc = [rng.uniform(0.0, 1.0, (3, 3)) for _ in far]
    cls = [f[1] for f in far]
    if twin_of is not None:                  # right after the original's class
        fx.insert(twin_of + 1, fx[twin_of].copy())
        fc.insert(twin_of + 1, 1.0 - fc[twin_of][:, ::-1])
        cls.insert(twin_of + 1, "h")
    nf = len(fx)
    step = max(1, (n_soup - 10) // nf)
    xyz, rgb, far_at, k = [], [], [], 0
    for t in range(n_soup):
        xyz.append(sxyz[3 * t:3 * t + 3])
        rgb.append(srgb[3 * t:3 * t + 3])
        if (t + 1) % step == 0 and k < nf:
            far_at.append(len(xyz))
            xyz.append(fx[k])
            rgb.append(fc[k])
            k += 1
    assert k == nf
    v = K._pack(np.concatenate(xyz), np.concatenate(rgb))
    far_at = np.asarray(far_at, dtype=np.int64)
    twin = () if twin_of is None else (int(far_at[twin_of]), int(far_at[twin_of + 1]))
    return FarSet(v, np.arange(v.shape[0], dtype=np.int64), far_at, "".join(cls), twin)


def _build(name, spec, seed):
    w, h = TARGETS[name]
    rng = np.random.default_rng(seed)
    far = []
    for cls, corners, z in spec:
        xy = np.array([_corner(c, w, h) for c in corners], dtype=np.float64)
        far.append((np.concatenate([xy, np.asarray(z, dtype=np.float64)[:, None]], axis=1), cls))
    last_b = max(k for k, f in enumerate(far) if f[1] == "b")
    return _mixed(_soup(rng, w, h), far, rng, twin_of=last_b)


_SETS = {}


def edge_set(name):
    """The CPU-rules edge set of a target ("wide" / "tall")."""
    if ("cpu", name) not in _SETS:
        _SETS[("cpu", name)] = _build(name, _far_cpu(*TARGETS[name]), 0xC0ED)
    return _SETS[("cpu", name)]


def metal_set(name):
    """The Metal variant."""
    if ("metal", name) not in _SETS:
        _SETS[("metal", name)] = _build(name, _far_metal(*TARGETS[name]), 0xC0EE)
    return _SETS[("metal", name)]


def rules_set(name, flags):
    return metal_set(name) if flags & K.METAL else edge_set(name)


def max_coordinate(oracle, v, i, m, w, h):
    """Per triangle: the largest |screen coordinate| of its corners through oracle.project (NaN if one is not a number)."""
    sx, sy, _ = oracle.project(v, m, w, h)
    t = np.asarray(i, dtype=np.int64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return np.maximum(np.abs(sx[t].astype(np.float64)).max(axis=1), np.abs(sy[t].astype(np.float64)).max(axis=1))


def perspective_set(oracle, name):
    """The perspective variant under K.perspective_matrix(): small triangles, and slivers with one vertex at w = 1 + z / 4 a few float
    steps above 0 (z just above -4), kept from a seeded scan where oracle.project puts their largest |coordinate| into [2^29, 2^30)
    (class p, 6 of them) or [2^30, 2^31) (class q, 4 of them)."""
    if ("persp", name) in _SETS:
        return _SETS[("persp", name)]
    w, h = TARGETS[name]
    m = K.perspective_matrix()
    rng = np.random.default_rng(0xC0EF)
    want = {"p": 6, "q": 4}
    far = []
    for _ in range(4000):
        if not any(want.values()):
            break
        z = F32(-4.0)
        for _ in range(int(rng.integers(1, 9))):
            z = np.nextafter(z, F32(0))
        apex = [rng.uniform(-1, 1), rng.uniform(-1, 1), float(z)]
        bx, by = rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8)
        tri = np.array([apex, [bx, by, rng.uniform(0.1, 0.9)], [bx + rng.uniform(0.1, 0.25), by + rng.uniform(-0.25, 0.25), rng.uniform(0.1, 0.9)]])
        big = max_coordinate(oracle, K._pack(tri, np.zeros((3, 3))), np.arange(3), m, w, h)[0]
        cls = "p" if 2.0 ** 29 <= big < LIMIT else ("q" if LIMIT <= big < 2.0 ** 31 else None)
        if cls and want[cls]:
            want[cls] -= 1
            far.append((tri, cls))
    assert not any(want.values()), "the scan did not find the perspective slivers"
    # (NDC after the divide is x / w with w in [1, 1.25] for the small triangles: they stay on the target)
    soup = _soup(rng, w, h)
    _SETS[("persp", name)] = _mixed(soup, far, rng)
    return _SETS[("persp", name)]


def padded(fs):
    """K.padded(edge set): 2^20 + 1 primitives, the filler after the first half, the last triangle number 2^20.
    Returns (vertices, indices, far numbers in the padded scene)."""
    n_head = fs.triangles // 2
    v, i, first = K.padded(fs.vertices, fs.indices, n_head, K.PADDED_TRIANGLES)
    far = np.where(fs.far < n_head, fs.far, fs.far + (first - n_head))
    return v, i, far


# ---- points and lines --------------------------------------------------------------------------------------------------------------
def point_scene(name):
    """Vertices for a .vertices frame: on the target, at the last coordinate inside the limit on each side (off the target: nothing
    lands), at the limit and beyond (skipped), at the decades, and pairs that truncate to the same pixel (the later index wins)."""
    w, h = TARGETS[name]
    rng = np.random.default_rng(0xC0F0)
    pts = [(x, y) for x, y in zip(rng.uniform(0, w, 300), rng.uniform(0, h, 300))]
    pts += [(10.25, 20.5), (10.75, 20.25), (w - 0.5, h - 0.5), (0.0, 0.0, "exact", "exact")]
    B, L = BELOW, LIMIT
    for M in (2.0 ** 17, 2.0 ** 20, 2.0 ** 24, 2.0 ** 27, 0.75 * L, B):
        pts += [(M, 0.5 * h), (-M, 0.5 * h), (0.5 * w, M), (0.5 * w, -M), (M, -M)]
    pts += [(L, 0.5 * h, "exact") if w == 256 else (0.5 * w, L, "inside", "exact"),
            (-L, 0.5 * h, "exact") if w == 256 else (0.5 * w, -L, "inside", "exact"),
            (L + 64, 0.5 * h, "beyond"), (0.5 * w, -L - 64, "inside", "beyond"), (3e38, 3.0)]
    xy = np.array([_corner(p, w, h) for p in pts], dtype=np.float64)
    xyz = np.concatenate([xy, rng.uniform(0, 1, (len(pts), 1))], axis=1)
    v = K._pack(xyz, rng.uniform(0, 1, (len(pts), 3)))
    return v, np.arange(len(pts), dtype=np.int64)


def line_scene(name):
    """Eight long lines of a real-line frame, (vertices, indices, what each is): the long axis is the power-of-two one.
      0  2^20 steps exactly, across the target                       drawn
      1  2^20 + 1 steps, across the target                           skipped
      2  starts beyond 2^24 (x += xStep is inexact there), 2^20      drawn (off the target: within 2^20 steps such a line cannot
         steps long                                                  reach it; lines 0, 6 and 7 accumulate inexactly across it)
      3  one endpoint at exactly 2^30                                skipped whole
      4  one endpoint at the last float below 2^30, 2^20 steps long  drawn (off the target: nothing lands)
      5  a short line on the target                                  drawn
      6  2^20 steps along the other axis                             drawn
      7  from -2^19 to 2^19 diagonally                               drawn"""
    w, h = TARGETS[name]
    pow_x = w == 256
    S = float(1 << 20)
    B, L = BELOW, LIMIT

    def along(a, b):
        """(long-axis coordinate, the other one) -> (px, py)"""
        return (a, b) if pow_x else (b, a)

    ex = ("exact",) if pow_x else ("inside", "exact")
    segs = [
        (along(-S + 100.0, 31.0) + ex, along(100.0, 90.0) + ex),
        (along(-S + 99.0, 41.0) + ex, along(100.0, 120.0) + ex),
        (along(2.0 ** 24 + 32.0, 150.0) + ex, along(2.0 ** 24 + 32.0 - S, 20.0) + ex),
        (along(L, 50.0) + ex, along(40.0, 60.0)),
        (along(B, 50.0) + ex, along(B - S, 60.0) + ex),
        ((5.5, 7.5), (0.8 * w, 0.7 * h)),
        ((along(77.0, -S / 2)[0], along(77.0, -S / 2)[1]), (along(99.0, S / 2)[0], along(99.0, S / 2)[1])),
        ((-S / 2, -S / 2 + 30), (S / 2, S / 2)),
    ]
    rng = np.random.default_rng(0xC0F1)
    xy = np.array([_corner(p, w, h) for s in segs for p in s], dtype=np.float64)
    xyz = np.concatenate([xy, rng.uniform(0, 1, (xy.shape[0], 1))], axis=1)
    v = K._pack(xyz, rng.uniform(0.1, 1, (xy.shape[0], 3)))
    return v, np.arange(xy.shape[0], dtype=np.int64)


# ---- expectations, cached per (set, target) -------------------------------------------------------------------------------------------
REAL_LINES = 8                  # SWR_FLAG_REAL_LINES
_CACHES = {}


def cache_of(fs, name, key="edge"):
    """The kernel_matrix.expected_frame cache of a set on a target (one clear frame per rule set, one coded ID pair per rule set)."""
    return _CACHES.setdefault((id(fs), name, key), {})


def frame(oracle, fs, name, flags, m=K.IDENT, start=None, shading=None, key="edge"):
    """kernel_matrix.expected_frame of a set on its target."""
    w, h = TARGETS[name]
    return K.expected_frame(oracle, fs.vertices, fs.indices, m, w, h, flags, shading, start, cache_of(fs, name, key))


def frame_ids(oracle, fs, name, flags, m=K.IDENT, key="edge"):
    return frame(oracle, fs, name, flags | K.IDS, m, key=key).ids


def shown(ids, n):
    """Pixels per triangle of an expected ID image."""
    ids = np.asarray(ids).reshape(-1)
    return np.bincount(ids[(ids >= 0) & (ids != K.NONE)], minlength=n)
