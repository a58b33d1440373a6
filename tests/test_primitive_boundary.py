"""Scenes of 2^20 - 1, 2^20 and 2^20 + 1 primitives: both thresholds of the winner table (tests/kernel_matrix.py for the helpers).

The winner table packs `primitive << 12 | bin position` into a key's low word, and a z-tested load frame packs primitive + 1: clear
frames take the PLAIN kernels above 2^20 primitives, load frames from 2^20 on.  The scene: about 150 visible triangles at the start,
off-screen filler, about 150 at the very end (bins far below 4 096 entries: the table is in use on the non-PLAIN side).  The last
three primitives are duplicates of triangles 0 and 1 with other colours (exact depth ties: they lose them under the z-test and win
them under painter's order) and a last triangle nearer than everything.  Every mode draws with IDs, as a clear frame and as a load
frame over a special starting image, reached three ways: a draw, a two-item draw list split inside the filler (IDs number the
concatenation), and a culled frame (the count is of submitted triangles; IDs keep the original numbering).
"""
import numpy as np
import pytest

import kernel_matrix as K

pytestmark = pytest.mark.gpu

W, H = 328, 200
COUNTS = [(1 << 20) - 1, 1 << 20, (1 << 20) + 1]
MODES = {"ztest": (K.DT, 0), "painter": (0, 0), "metal": (K.METAL, 0), "textured_phong": (K.DT, 2)}


def _px_tri(rng, n, z0, z1):
    """n clockwise-as-displayed or counter-clockwise triangles of 10-30 pixels inside the target, in NDC."""
    c = rng.uniform([20, 20], [W - 20, H - 20], (n, 1, 2))
    p = c + rng.uniform(-15, 15, (n, 3, 2))
    x, y = K._ndc(p[..., 0], p[..., 1], W, H)
    z = rng.uniform(z0, z1, (n, 3))
    return np.stack([x, y, z], axis=-1).reshape(-1, 3)


def boundary_scene():
    """(vertices, indices of the visible triangles, n_head): head = triangles 0 and 1 (near, clockwise as displayed) and 148
    others; tail = 147 others, the duplicates of 0 and 1, and the last triangle (nearest of all, clockwise as displayed)."""
    rng = np.random.default_rng(0xB0DA)

    def cw(px):          # pixel triples, clockwise as displayed (A > 0 with y down)
        x, y = K._ndc(np.asarray(px, float)[:, 0], np.asarray(px, float)[:, 1], W, H)
        return x, y

    t0 = cw([(40.5, 30.5), (120.5, 40.5), (60.5, 110.5)])
    t1 = cw([(200.5, 100.5), (300.5, 120.5), (230.5, 180.5)])
    tl = cw([(130.5, 60.5), (190.5, 70.5), (150.5, 150.5)])
    z01 = np.array([0.05, 0.07, 0.06])
    tri = lambda xy, z: np.stack([xy[0], xy[1], z], axis=-1)
    head = np.concatenate([tri(t0, z01), tri(t1, z01[::-1]), _px_tri(rng, 148, 0.2, 1.0)])
    tail = np.concatenate([_px_tri(rng, 147, 0.2, 1.0), tri(t0, z01), tri(t1, z01[::-1]), tri(tl, np.full(3, -0.5))])
    xyz = np.concatenate([head, tail])
    rgb = rng.uniform(-0.1, 1.1, (xyz.shape[0], 3))
    v = K._pack(xyz, rgb)
    return v, np.arange(v.shape[0], dtype=np.int64), 150


@pytest.mark.parametrize("count", COUNTS, ids=["2^20-1", "2^20", "2^20+1"])
def test_around_2_20_primitives(swr, oracle, count):
    v0, i0, n_head = boundary_scene()
    v, i, first = K.padded(v0, i0, n_head, count)
    n = i.size // 3
    assert n == count and first + 150 == n
    last, dup0, dup1 = n - 1, n - 3, n - 2
    c0, d0 = K.special_start(W, H, 0xB0D)
    area = K.signed_areas(oracle, v, i, K.IDENT, W, H, 0)
    assert (area[[0, 1, dup0, dup1, last]] > 0).all()
    cull = K.CB                                  # clockwise as displayed is front-facing by default: 0, 1 and the last are kept
    caches = {}
    with swr.Context(0) as ctx:
        ctx.scene_upload(v, i)
        ctx.target_set(W, H)
        split = first - 1000
        items = [(0, 3 * split, K.IDENT), (3 * split, 3 * (n - split), K.IDENT)]
        for mode, (base, shader) in MODES.items():
            sh = None if shader == 0 else swr.scenes.random_shading(v.shape[0], 0xB0D, shader)
            if sh is None:
                ctx.material_set(None)
            else:
                ctx.shading_set(sh)
            for load in (False, True):
                for way in ("draw", "list", "culled"):
                    flags = base | K.IDS | (K.LOAD if load else 0) | (cull if way == "culled" else 0)
                    cache = caches.setdefault(way == "culled", {})
                    want = K.expected_frame(oracle, v, i, K.IDENT, W, H, flags, sh, (c0, d0), cache)
                    what = f"{count} primitives, {mode}, {'load' if load else 'clear'} frame, {way}"
                    if way == "culled":
                        visible = np.r_[0:n_head, first:n]
                        assert np.isin([0, 1, dup0, dup1, last], want.kept).all(), what
                        assert 20 < np.setdiff1d(visible, want.kept).size < 200, what
                    if load:
                        ctx.target_write(c0, d0)
                    if way == "list":
                        ctx.draw_list(items, flags)
                    else:
                        ctx.draw(K.IDENT, flags)
                    ctx.sync()
                    ids = ctx.read_ids()
                    bad = np.nonzero((ids != want.ids) & (want.ids >= 0))
                    assert bad[0].size == 0, (f"{what}: {bad[0].size} IDs differ, first at (y,x)=({bad[0][0]},{bad[1][0]}): "
                                              f"{ids[bad][0]} vs {want.ids[bad][0]}")
                    assert (ids[want.ids == K.LIVE] != K.NONE).all(), what
                    assert ctx.read_depth().tobytes() == want.depth.tobytes(), what
                    assert np.array_equal(ctx.read_color(), want.color), what
                    # the last primitive wins where it is nearest (and, under painter's order, wherever it covers)
                    assert (ids == last).sum() > 1000, what
                    if base & (K.DT | K.METAL):
                        # the duplicates lose their exact ties to triangles 0 and 1
                        assert not np.isin(ids, [dup0, dup1]).any(), what
                        assert (ids == 0).sum() > 500 and (ids == 1).sum() > 500, what
                    else:
                        assert (ids == dup0).sum() > 500 and (ids == dup1).sum() > 500, what
                    assert (ids[ids != K.NONE] >= first).any() and (ids[ids != K.NONE] < n_head).any(), what
