"""CPU tests of tests/frame_model.py (no GPU): the one expectation equals the expectation every per-feature test file already
uses, the reductions include/swr.h promises hold, the golden fixtures reproduce through it, and the sequences and the covering array
of tests/test_frame_sequences.py meet their coverage conditions."""
import dataclasses
import glob
import hashlib
import os

import numpy as np
import pytest

import frame_model as FM
import kernel_matrix as K
import resolve_model as RM
import test_depth_clip as DC
import test_frame_sequences as FS
import test_perspective as TP
from frame_model import ADD, BLEND, CB, CCW, CF, CLIP, DT, IDS, LOAD, METAL, NC, OVER, PERSP

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 320, 192
RULES = (0, DT, METAL)


def spec(v, i, flags, m=None, items=None, shading=None, w=W, h=H):
    return FM.FrameSpec(v, i, w, h, flags, transform=m, items=items, shading=shading)


def eq(a, b):
    return (a is None and b is None) or (a.shape == b.shape and a.tobytes() == b.tobytes())


@pytest.fixture(scope="module")
def flat(swr):
    """A screen-space soup of both windings with exact ties, under an affine transform."""
    s = swr.scenes.random_soup(500, W, H, 0xF1A7, r_ndc=0.15, margin=1.1)
    v = s.vertices.copy()
    v[3:30:9] = v[0:27:9]
    return v, s.indices, K.affine_matrix()


# ---- 1. each single feature: the expectation of its own test file ------------------------------------------------------------------
@pytest.mark.parametrize("flags", [DT | CB, CF | CCW, METAL | CB | CCW, DT | NC | CF, DT | IDS, IDS, METAL | IDS | CB, DT | LOAD | IDS,
                                   LOAD, METAL | LOAD | IDS | CF, DT | NC | LOAD, NC | LOAD | IDS])
def test_equals_kernel_matrix_expected_frame(swr, oracle, flat, flags):
    """cull / load / IDs: kernel_matrix.expected_frame."""
    v, i, m = flat
    sh = swr.scenes.random_shading(v.shape[0], 5, 2) if flags & LOAD and not flags & NC else None
    start = K.special_start(W, H, 0x51) if flags & LOAD else None
    want = K.expected_frame(oracle, v, i, m, W, H, flags | IDS, sh, start)
    c, d, ids = FM.expect(oracle, spec(v, i, flags, m, shading=sh), start)
    assert eq(c, want.color) and eq(d, want.depth)
    assert (ids is None) == (not flags & IDS)
    if ids is not None:
        assert np.array_equal(ids, want.ids)
    if flags & (CB | CF):
        assert 0 < want.kept.size < i.size // 3


@pytest.mark.parametrize("flags", [DT | IDS, IDS | CB, METAL | IDS | CF | CCW, DT | LOAD | IDS])
def test_equals_kernel_matrix_draw_list(oracle, flat, flags):
    """draw lists: the pre-transformed concatenation drawn with the identity, as tests/test_kernel_matrix.py expects them."""
    v, i, m = flat
    n = i.size // 3
    items = [(0, 3 * (n // 2), m), (3 * (n // 2), 3 * (n - n // 2), K.affine_matrix(-0.2, 0.8, -0.1, 0.05)), (0, 3 * 40, K.mirrored(m))]
    start = K.special_start(W, H, 0x52) if flags & LOAD else None
    cv, ci = K.concat(v, i, items)
    want = K.expected_frame(oracle, cv, ci, K.IDENT, W, H, flags, None, start)
    c, d, ids = FM.expect(oracle, spec(v, i, flags, items=items), start)
    assert eq(c, want.color) and eq(d, want.depth) and np.array_equal(ids, want.ids)


@pytest.mark.parametrize("shader", [0, 2])
@pytest.mark.parametrize("mode", list(DC.MODES))
def test_equals_depth_clip_expected(swr, oracle, mode, shader):
    v, i = DC.straddling_soup(400, 0xC1)
    m = DC.metal_perspective()
    assert DC.crosses(v, i, m).sum() > 40
    sh = swr.scenes.random_shading(v.shape[0], 12, shader) if shader else None
    flags = DC.MODES[mode]
    wc, wd, wid, _ = DC.expected(oracle, v, i, m, flags, ids=True, shading=sh)
    c, d, ids = FM.expect(oracle, spec(v, i, flags | CLIP | IDS, m, shading=sh))
    assert eq(c, wc) and eq(d, wd) and np.array_equal(ids, wid)


def test_equals_depth_clip_cull_and_draw_list(oracle):
    """The compositions tests/test_depth_clip.py checks: culling per sub-triangle, a two-item list with a mirrored matrix."""
    v, i = DC.straddling_soup(400, 0xC2)
    m = DC.metal_perspective()
    V, _, I, fmap, _ = DC.restate(v, i, m)
    for cull in (CB, CF, CB | CCW):
        flags = DT | cull
        keep = K.kept_triangles(K.signed_areas(oracle, V, I, K.IDENT, W, H, flags), flags)
        wc, wd = DC.oracle_frame(oracle, V, I.reshape(-1, 3)[keep].reshape(-1), W, H, flags)
        c, d, _ = FM.expect(oracle, spec(v, i, flags | CLIP, m))
        assert eq(c, wc) and eq(d, wd) and 0 < keep.size < fmap.size
    mir = K.mirrored(m)
    n = i.size
    h = n // 2 // 3 * 3
    items = [(0, h, m), (h, n - h, mir)]
    ms = [m] * (h // 3) + [mir] * ((n - h) // 3)
    for flags in (DT, 0):
        wc, wd, wid, _ = DC.expected(oracle, v, i, ms, flags, ids=True)
        c, d, ids = FM.expect(oracle, spec(v, i, flags | CLIP | IDS, items=items))
        assert eq(c, wc) and eq(d, wd) and np.array_equal(ids, wid)


@pytest.mark.parametrize("shader", [0, 1])
@pytest.mark.parametrize("rules", RULES)
def test_equals_perspective_model(swr, oracle, rules, shader):
    v, i = TP.soup(250, 0x9E1)
    m = TP.perspective()
    sh = TP.shading_for(swr, v.shape[0], shader)
    start = TP.start_images(0x5B)
    wc, wd = TP.model(v, i, m, W, H, rules, sh)
    c, d, _ = FM.expect(oracle, spec(v, i, rules | PERSP, m, shading=sh))
    assert eq(c, wc) and eq(d, wd)
    lin, _, _ = FM.expect(oracle, spec(v, i, rules, m, shading=sh))
    assert not eq(lin, wc)
    # a load frame: the load rule over the model's clear frame is the model started from the image
    wc, wd = TP.model(v, i, m, W, H, rules, sh, start)
    c, d, _ = FM.expect(oracle, spec(v, i, rules | PERSP | LOAD, m, shading=sh), start)
    assert eq(c, wc) and eq(d, wd)


def test_equals_perspective_model_compositions(swr, oracle):
    """tests/test_perspective.py's own compositions: back-face culling, a mixed draw list, depth-clip fans."""
    v, i = TP.soup(250, 0xCB)
    m = TP.perspective()
    for rules in (DT, METAL):
        wc, wd = TP.model(v, i, m, W, H, rules, cull_back=True)
        c, d, _ = FM.expect(oracle, spec(v, i, rules | PERSP | CB, m))
        assert eq(c, wc) and eq(d, wd)
    aff = TP.rotation_scaled()
    n = i.size
    h = n // 2 // 3 * 3
    items = [(0, h, m), (h, n - h, aff), (0, h, m)]
    t = np.asarray(i).reshape(-1, 3)
    I = np.concatenate([t[:h // 3], t[h // 3:], t[:h // 3]]).reshape(-1)
    ms = [m] * (h // 3) + [aff] * ((n - h) // 3) + [m] * (h // 3)
    sh = TP.shading_for(swr, v.shape[0], 1)
    for flags, s in ((DT, None), (0, None), (METAL, sh)):
        wc, wd = TP.model(v, I, ms, W, H, flags, s)
        c, d, _ = FM.expect(oracle, spec(v, i, flags | PERSP, items=items, shading=s))
        assert eq(c, wc) and eq(d, wd)
    v, i = DC.straddling_soup(250, 0xF1, z_lo=-1.5, z_hi=4.0, r=1.5)
    for rules in RULES:
        wc, wd = TP.clip_model(v, i, m, rules, sh)
        c, d, _ = FM.expect(oracle, spec(v, i, rules | PERSP | CLIP, m, shading=sh))
        assert eq(c, wc) and eq(d, wd)


# ---- 2. the reductions the header promises -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules", RULES)
def test_reductions(swr, oracle, flat, rules):
    v, i, m = flat
    sh = swr.scenes.random_shading(v.shape[0], 6, 1)
    base = FM.expect(oracle, spec(v, i, rules | IDS, m, shading=sh))

    def same_as_base(got):
        return eq(got[0], base[0]) and eq(got[1], base[1]) and np.array_equal(got[2], base[2])
    # SWR_FLAG_PERSPECTIVE under an affine transform: the frame without it
    assert same_as_base(FM.expect(oracle, spec(v, i, rules | IDS | PERSP, m, shading=sh)))
    # SWR_FLAG_DEPTH_CLIP on a scene entirely inside both planes (the affine transform keeps z in (0, 1), w = 1): the frame without it
    r = DC.clip_space(v, m)
    assert (r[:, 2] > 0).all() and (r[:, 3] - r[:, 2] > 0).all()
    assert same_as_base(FM.expect(oracle, spec(v, i, rules | IDS | CLIP, m, shading=sh)))
    assert same_as_base(FM.expect(oracle, spec(v, i, rules | IDS | CLIP | PERSP, m, shading=sh)))
    # a one-item draw list: the draw
    assert same_as_base(FM.expect(oracle, spec(v, i, rules | IDS, items=[(0, i.size, m)], shading=sh)))
    # SWR_FLAG_CULL_BACK | SWR_FLAG_CULL_FRONT keeps exactly the A == 0 triangles
    area = K.signed_areas(oracle, v, i, m, W, H, rules)
    zero = np.nonzero(area == 0)[0]
    fi = np.asarray(i).reshape(-1, 3)[zero].reshape(-1)
    want = FM.expect(oracle, spec(v, fi, rules, m, shading=sh))
    for ccw in (0, CCW):
        got = FM.expect(oracle, spec(v, i, rules | CB | CF | ccw | IDS, m, shading=sh))
        assert eq(got[0], want[0]) and eq(got[1], want[1])
        assert np.isin(got[2][(got[2] != K.NONE) & (got[2] != K.LIVE)], zero).all()


@pytest.mark.parametrize("rules", RULES)
def test_uncorrected_model_is_the_c_oracle(oracle, rules):
    """tests/test_perspective.py's model with the screen weights left as they are: the C oracle's frame."""
    v, i = TP.soup(400, 0x9E2, r=0.15)
    m = TP.perspective()
    wc, wd = K.oracle_clear(oracle, v, i, m, W, H, rules)
    c, d = TP.model(v, i, m, W, H, rules, correct=False)
    assert eq(c, wc) and eq(d, wd)


def test_unspecified_colour_is_masked(oracle, flat):
    """A colour load frame over a depth-only frame: colour is defined where the frame's own fragments win, and a chain narrows
    what is still unspecified."""
    v, i, m = flat
    _, d0, _ = FM.expect(oracle, spec(v, i[:300], DT | NC, m))
    c1, d1, _ = FM.expect(oracle, spec(v, i[300:], DT | LOAD, m), (None, d0))
    own, dn, _ = FM.expect(oracle, spec(v, i[300:], DT, m))
    win = dn < d0
    assert isinstance(c1, np.ma.MaskedArray) and np.array_equal(np.ma.getmaskarray(c1)[..., 0], ~win)
    assert np.array_equal(np.ma.getdata(c1)[win], own[win]) and 0 < win.sum() < win.size
    c2, _, _ = FM.expect(oracle, spec(v, i[:300], LOAD, K.affine_matrix(0.3)), (c1, d1))
    cov = FM.expect(oracle, spec(v, i[:300], 0, K.affine_matrix(0.3)))[0][..., 3] == 255
    assert np.array_equal(np.ma.getmaskarray(c2)[..., 0], ~win & ~cov)
    FM.same((np.ma.getdata(c2).copy(), None, None), (c2, d1, None))
    wrong = np.ma.getdata(c2).copy()
    wrong[np.nonzero(win)[0][0], np.nonzero(win)[1][0], 0] ^= 1
    with pytest.raises(AssertionError):
        FM.same((wrong, None, None), (c2, d1, None))


# ---- 2b. blend frames and resolved reads, by the model alone --------------------------------------------------------------------------
BW, BH = 96, 64


@pytest.fixture(scope="module")
def small_soup(swr):
    s = swr.scenes.random_soup(90, BW, BH, 0xB1E, r_ndc=0.3, margin=1.1)
    v = s.vertices.copy()
    v[3:30:9] = v[0:27:9]
    return v, s.indices, K.affine_matrix()


def bspec(v, i, flags, blend, m=None, items=None):
    return FM.FrameSpec(v, i, BW, BH, flags, transform=m, items=items, blend=blend)


@pytest.mark.parametrize("rules", RULES)
def test_blend_expectation_has_the_header_properties(oracle, small_soup, rules):
    v, i, m = small_soup
    clear_d = np.full((BH, BW), np.inf, dtype=np.float32)
    starts = [None, K.special_start(BW, BH, 0xB2), K.special_start(BW, BH, 0xB3)]
    for start in starts:
        load = LOAD if start is not None else 0
        want_d = clear_d if start is None else start[1]
        # (b) opacity 0: the starting image, special starts included; the depth is the start's bit for bit
        for mode in (OVER, ADD):
            c, d, ids = FM.expect(oracle, bspec(v, i, rules | load, (mode, 0), m), start)
            assert ids is None and d.tobytes() == want_d.tobytes()
            assert np.array_equal(c, np.zeros((BH, BW, 4), np.uint8) if start is None else start[0])
        # (c) a draw list is the chain of its one-item frames
        items = [(0, 90, m), (60, 150, K.affine_matrix(0.3, 0.8)), (0, 0, m), (30, 120, K.mirrored(m))]
        for mode, opacity in ((OVER, 128), (ADD, 254)):
            lc, ld, _ = FM.expect(oracle, bspec(v, i, rules | load, (mode, opacity), items=items), start)
            cur = start
            for k, it in enumerate(items):
                fl = rules | (LOAD if cur is not None else 0)
                cc, cd, _ = FM.expect(oracle, bspec(v, i, fl, (mode, opacity), items=[it]), cur)
                cur = (cc, cd)
            assert np.array_equal(cur[0], lc) and cur[1].tobytes() == ld.tobytes() == want_d.tobytes()
            assert not np.array_equal(lc, np.zeros_like(lc) if start is None else start[0])
    # (a) OVER with opacity 255 and no z-test: the colour of the frame without the bit
    if not rules:
        for start in starts:
            load = LOAD if start is not None else 0
            c, d, _ = FM.expect(oracle, bspec(v, i, load, (OVER, 255), m), start)
            pc, _, _ = FM.expect(oracle, spec(v, i, load, m, w=BW, h=BH), start)
            assert np.array_equal(c, pc) and d.tobytes() == (clear_d if start is None else start[1]).tobytes()


@pytest.mark.parametrize("opacity", [255, 128])
@pytest.mark.parametrize("mode", [OVER, ADD])
def test_blend_over_an_unspecified_colour(oracle, small_soup, mode, opacity):
    """A blend load frame over a NO_COLOR frame: a pixel becomes specified only through a contributing OVER 255 fragment."""
    v, i, m = small_soup
    _, d0, _ = FM.expect(oracle, bspec(v, i[:120], DT | NC, None, m))
    glass = bspec(v, i[120:], DT | LOAD, (mode, opacity), K.affine_matrix(0.4, 0.9))
    c, d, _ = FM.expect(oracle, glass, (None, d0))
    assert d.tobytes() == d0.tobytes()
    # contributing: some fragment of the frame passes the strict test against the starting depth
    hit = np.zeros((BH, BW), dtype=bool)
    for _, y0, x0, cs, ds in FM.primitives(oracle, glass):
        with np.errstate(invalid="ignore"):
            hit[y0:y0 + cs.shape[0], x0:x0 + cs.shape[1]] |= (cs[..., 3] == 255) & (ds < d0[y0:y0 + cs.shape[0], x0:x0 + cs.shape[1]])
    assert 0 < hit.sum() < hit.size
    specified = hit if (mode, opacity) == (OVER, 255) else np.zeros_like(hit)
    assert isinstance(c, np.ma.MaskedArray) and np.array_equal(np.ma.getmaskarray(c)[..., 0], ~specified)
    if specified.any():     # ... and what is specified does not depend on what was there
        junk = K.special_start(BW, BH, 0xB4)[0]
        c2, _, _ = FM.expect(oracle, glass, (junk, d0))
        assert np.array_equal(np.ma.getdata(c)[specified], c2[specified])
    # a chain keeps the mask of what is still unspecified: an OVER 255 frame on top clears it where it contributes, and only there
    top = bspec(v, i[:60], LOAD, (OVER, 255), K.affine_matrix(-0.2, 0.7))
    c3, _, _ = FM.expect(oracle, top, (c, d))
    cov = FM.expect(oracle, spec(v, i[:60], 0, K.affine_matrix(-0.2, 0.7), w=BW, h=BH))[0][..., 3] == 255
    assert np.array_equal(np.ma.getmaskarray(c3)[..., 0], ~specified & ~cov) and cov.any()


def test_resolved_expectation_propagates_the_mask():
    rng = np.random.default_rng(0x2E5)
    c = rng.integers(0, 256, (16, 24, 4), dtype=np.uint8)
    d = K.special_start(24, 16, 0x2E6)[1]
    for filt in (RM.SAMPLE0, RM.MIN):
        rc, rd, ids = FM.resolved((c, d, None), 1, filt)
        assert rc is c and rd is d and ids is None
        for S in (2, 4):
            rc, rd, _ = FM.resolved((c, d, None), S, filt)
            assert not isinstance(rc, np.ma.MaskedArray) and np.array_equal(rc, RM.color(c, S))
            assert rd.tobytes() == RM.depth(d, S, filt).tobytes()
            mask = np.zeros((16, 24), dtype=bool)
            mask[5, 7] = mask[0, 0] = mask[15, 23] = True
            mask[8:12, 8:12] = True
            mc = np.ma.masked_array(c, mask=np.repeat(mask[..., None], 4, axis=-1))
            rc, rd2, _ = FM.resolved((mc, d, None), S, filt)
            want = np.zeros((16 // S, 24 // S), dtype=bool)
            for y, x in zip(*np.nonzero(mask)):
                want[y // S, x // S] = True
            assert np.array_equal(np.ma.getmaskarray(rc)[..., 0], want) and 0 < want.sum() < want.size
            assert np.array_equal(np.ma.getdata(rc)[~want], RM.color(c, S)[~want])
            assert not isinstance(rd2, np.ma.MaskedArray) and rd2.tobytes() == rd.tobytes()
            assert FM.resolved((None, d, None), S, filt)[0] is None


def test_blend_covering_array_covers_every_pair():
    rows = FM.blend_covering_array()
    assert rows == FM.blend_covering_array() and rows == FS.FM.blend_covering_array()
    seen = set()
    for r in rows:
        assert set(r) == set(FM.BLEND_FACTORS) and all(r[f] in FM.BLEND_FACTORS[f] for f in r) and FM.legal(r)
        seen |= FM.pairs_in(r, FM.BLEND_FACTORS)
        s = FS.blend_pair_spec(r, "small")
        flags, state = FM.blend_flags_of(r)
        assert s.flags == flags and s.blend == state and not flags & (NC | IDS | PERSP | BLEND) and s.shading is None
        assert (s.items is not None) == bool(r["list"])
    assert seen == FM.all_pairs_in(FM.BLEND_FACTORS)
    # the untouched space: FACTORS ends at persp / shader / list / transform as before, and its array has not moved
    assert FM.all_pairs_in(FM.FACTORS) == FM.all_pairs() and len(FM.covering_array()) <= 24
    assert not FM.legal(dict(mode="over", no_color=1)) and not FM.legal(dict(blend=1, shader=2)) and FM.legal(dict(no_color=1, ids=1))
    assert not FM.legal(dict(blend=1, ids=1)) and not FM.legal(dict(blend=1, persp=1))


# ---- 3. the golden fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(HERE, "golden", "*.npz")) +
                                        glob.glob(os.path.join(HERE, "golden", "shaded", "*.npz"))), ids=os.path.basename)
def test_golden_fixtures_reproduce(swr, oracle, path):
    g = np.load(path)
    sh = None
    if "attrs" in g.files:
        a, dd, s = (float(x) for x in g["ads"])
        sh = swr.scenes.Shading(g["attrs"], int(g["shader"]), int(g["shininess_log2"]), tuple(g["light_dir"]), tuple(g["half_dir"]),
                                a, dd, s, g["texture"] if "texture" in g.files else None)
    flags = int(g["flags"]) | (METAL if "metal" in g.files and int(g["metal"]) else 0)
    c, d, _ = FM.expect(oracle, FM.FrameSpec(g["vertices"], g["indices"], int(g["width"]), int(g["height"]), flags, g["transform"],
                                             shading=sh))
    assert eq(d, g["depth"])
    assert (c is None) == ("color" not in g.files)
    if c is not None:
        assert eq(c, g["color"])


# ---- 4. what the sequences of tests/test_frame_sequences.py cover (the generator needs no GPU) -----------------------------------------
@pytest.fixture(scope="module")
def sequences():
    return {seed: FS.sequence(seed) for seed in FS.SEEDS}


# sha256 of the operation lists of seeds 21, 22, 23 as the generator made them before it learnt `blend` (computed at that commit)
PARENT_DIGESTS = {21: "982105087b6f07e46616e208a9b0d1027b9f43ee389b4e22a03b4816727062b8",
                  22: "aed5803d0aa88a5f00b2165905844cc191b1522722ba45ca9ee40b1cb271b4bf",
                  23: "48436f6baa1320a1a7578c8f4388ecc2f337c93bd11b038712bc8bf99c59f57c"}
_FRAME_FIELDS = ("n", "scene", "size", "shader", "kind", "flags", "via", "tf", "prev", "scene_id")


def canonical(ops):
    def frame(f):
        return tuple(getattr(f, k).n if isinstance(getattr(f, k), FS.Frame) else getattr(f, k) for k in _FRAME_FIELDS)
    return repr([(o[0],) + tuple(frame(x) if isinstance(x, FS.Frame) else x for x in o[1:]) for o in ops])


@pytest.fixture(scope="module")
def blend_sequences():
    return {seed: FS.sequence(seed, blend=True) for seed in FS.BLEND_SEEDS}


def test_blend_sequences_cover_what_single_frames_cannot(blend_sequences):
    """What the checked frames and the resolved reads of BLEND_SEEDS include, over the three seeds together."""
    assert len({FS.hooks_of(seed) for seed in blend_sequences}) >= 3
    checked, all_runs, resolved, state_change, grown = [], [], [], 0, 0
    for seed, ops in blend_sequences.items():
        again = FS.sequence(seed, blend=True)
        assert canonical(ops) == canonical(again) and [o[1].blend for o in ops if o[0] == "frame"] == [o[1].blend for o in again if o[0] == "frame"]
        checked += FS.checked_frames(ops)
        all_runs += FS.runs(ops)
        last = last_checked = None
        frames_since_target, since_frame, largest = 0, [], 0
        for k, op in enumerate(ops):
            if op[0] == "frame":
                if last is not None and "blend" in since_frame and not set(since_frame) & set(FS.BLOCKING):
                    state_change += 1
                last, since_frame = op[1], []
                frames_since_target += 1
                continue
            since_frame.append(op[0])
            if op[0] == "target":
                frames_since_target = 0
            if op[0] in ("upload", "target", "write", "render"):
                last = None
            if op[0] == "read_resolved":
                S, filt, which = op[1:]
                assert last is not None and which in ("color", "depth", "both") and not (last.flags & NC and which != "depth")
                w, h = FS.SIZES[last.size]
                assert w % 4 == 0 and h % 4 == 0
                nxt = [o for o in ops[k + 1:k + 6] if o[0] not in ("wait", "shading", "blend")]
                plain_read = bool(nxt) and nxt[0][0] == "read"
                after = [o for o in nxt if o[0] != "read"]
                load_next = bool(after) and after[0][0] == "frame" and bool(after[0][1].flags & LOAD) and after[0][1].prev is last \
                    and any(f is after[0][1] and chk for run in FS.runs(ops) for f, chk in run)
                size = (w // S) * (h // S)
                if largest and size > largest and frames_since_target == 1:
                    grown += 1
                largest = max(largest, size)
                resolved.append((S, filt, which, last, plain_read, load_next))
    blends = [f for f in checked if f.flags & BLEND]
    assert all(f.kind == "tri" and f.blend is not None and FM.legal(dict(f.row(), blend=1)) and f.shader == 0 for f in blends)
    assert all(f.blend is None for f in checked if not f.flags & BLEND)
    assert {f.via for f in blends} == {"draw", "list", "render"}
    assert {f.blend[0] for f in blends} == {OVER, ADD}
    assert len({f.blend[1] for f in blends}) >= 4 and {0, 255} <= {f.blend[1] for f in blends}
    assert {f.row()["rules"] for f in blends} == set(FM.FACTORS["rules"])
    loads = [f for f in blends if f.flags & LOAD and f.prev is not None]
    is_frame = lambda p: isinstance(p, FS.Frame) and p.kind == "tri"      # noqa: E731
    assert any(is_frame(f.prev) and not f.prev.flags & (NC | BLEND) for f in loads), "over a colour frame of the key kernels"
    assert any(is_frame(f.prev) and f.prev.flags & NC for f in loads), "over a depth-only frame"
    assert any(isinstance(f.prev, tuple) for f in loads), "over a swr_target_write image"
    assert any(is_frame(f.prev) and f.prev.flags & BLEND for f in loads), "over another blend frame"
    assert any(is_frame(f.prev) and f.prev.flags & BLEND and f.prev.flags & LOAD and is_frame(f.prev.prev) and f.prev.prev.flags & BLEND
               for f in loads), "a chain of three blend frames"
    # blend and other frames next to each other, in both orders, inside un-waited runs of four or more; one such run with a
    # depth-only frame, an ID frame and a shaded one
    orders, rich = set(), 0
    for run in all_runs:
        if len(run) < 4 or not any(f.flags & BLEND for f, _ in run):
            continue
        for (a, ca), (b, cb) in zip(run, run[1:]):
            if a.kind == b.kind == "tri" and ca and cb and bool(a.flags & BLEND) != bool(b.flags & BLEND):
                orders.add(bool(a.flags & BLEND))
        tri = [f for f, _ in run if f.kind == "tri"]
        rich += (any(f.flags & (DT | NC | METAL | IDS | BLEND) == DT | NC for f in tri) and any(f.flags & IDS for f in tri)
                 and any(f.shader and not f.flags & NC for f in tri))
    assert orders == {False, True} and rich >= 1
    assert any(run[-1][0].scene == "straddle" and run[-1][0].flags & CLIP and run[-1][0].flags & BLEND and run[-1][1] and len(run) >= 3
               for run in all_runs), "a blend frame as the clip tail of the fan-overflow burst"
    assert state_change >= 1
    # ... and between the overflowing blend tail and the read that redraws it, in every seed: the redraw keeps the posted state
    for seed, ops in blend_sequences.items():
        k = next(k for k, o in enumerate(ops) if o[0] == "frame" and o[1].scene == "straddle" and o[1].flags & CLIP and o[1].flags & BLEND)
        after = [o for o in ops[k + 1:k + 5] if o[0] != "present"]
        assert after[0][0] == "blend" and after[0][1:] != ops[k][1].blend and after[1][0] == "read", seed
        assert (after[0][2] in (0, 255)) is False and after[0][1] != ops[k][1].blend[0]
    # resolved reads
    assert {r[0] for r in resolved} == {2, 4} and {r[1] for r in resolved} == {RM.SAMPLE0, RM.MIN}
    assert {r[2] for r in resolved} == {"color", "depth", "both"}
    assert any(r[3].flags & BLEND for r in resolved) and any(r[3].kind != "tri" for r in resolved)
    assert any(r[3].kind == "tri" and r[3].flags & NC for r in resolved)
    assert any(r[4] for r in resolved) and any(r[5] for r in resolved) and grown >= 1
    one_shots = [f for f in checked if f.via == "render" and f.resolve is not None]
    assert {f.resolve[0] for f in one_shots} == {2, 4} and not any(f.flags & LOAD for f in one_shots)


def test_old_seeds_generate_the_operations_they_always_did(sequences):
    assert set(PARENT_DIGESTS) == set(FS.SEEDS)
    for seed, ops in sequences.items():
        assert hashlib.sha256(canonical(ops).encode()).hexdigest() == PARENT_DIGESTS[seed], seed
        assert all(o[1].blend is None and o[1].resolve is None and not o[1].flags & BLEND for o in ops if o[0] in ("frame", "render"))
        assert not {o[0] for o in ops} & {"blend", "read_resolved"}


def test_sequences_are_reproducible_and_mixed(sequences):
    all_ops = [o for ops in sequences.values() for o in ops]
    for seed, ops in sequences.items():
        again = FS.sequence(seed)
        sig = lambda seq: [(o[0],) + tuple(dataclasses.astuple(x)[:8] if isinstance(x, FS.Frame) else x for x in o[1:]) for o in seq]
        assert sig(ops) == sig(again)
        assert {o[0] for o in ops} >= {"hooks", "upload", "target", "shading", "frame", "present", "wait", "read"}, seed
        assert {o[1] for o in ops if o[0] == "upload"} == set(FS.SCENES) and {o[1] for o in ops if o[0] == "target"} == {0, 1, 2}
        assert {o[1] for o in ops if o[0] == "shading"} == {0, 1, 2}
        frames = [o[1] for o in ops if o[0] == "frame"]
        assert {f.via for f in frames} == {"draw", "list"} and {f.kind for f in frames} > {"tri"}
        # bursts of different flags, every frame of them checked
        long_runs = [r for r in FS.runs(ops) if len(r) >= 5]
        assert len(long_runs) >= 5 and all(len({f.flags for f, _ in r}) > 1 for r in long_runs)
        # the scene with depths <= 0 is drawn first, depth-only and z-tested; ordinary depth-only frames of the scene of its size follow
        first = frames[0]
        assert first.scene == "zero" and first.flags & (DT | NC | METAL) == DT | NC
        assert sum(1 for f in frames if f.scene == "small" and f.flags & (DT | NC | METAL | IDS) == DT | NC) >= 5
        # the model's share stays bounded
        assert len({(f.scene, f.size, f.via, f.tf, f.shader, f.flags & ~(IDS | LOAD)) for f in FS.checked_frames(ops) if f.needs_model()}) <= 40
    assert {o[0] for o in all_ops} >= {"write", "render", "sync", "timing", "pipeline"}
    frames = [o[1] for o in all_ops if o[0] == "frame"]
    assert {f.kind for f in frames} == {"tri", "points", "lines"}
    assert {bool(f.flags & FM.REAL_LINES) for f in frames if f.kind == "lines"} == {False, True}
    assert {o[1].scene_id != 0 for o in all_ops if o[0] == "render"} == {False, True}
    # load chains over target_write's image, over a clear frame and over a frame of another kind (depth-only, then colour)
    loads = [f for f in frames if f.flags & LOAD and f.kind == "tri"]
    assert any(isinstance(f.prev, tuple) for f in loads)
    assert any(isinstance(f.prev, FS.Frame) and not f.prev.flags & (LOAD | NC) for f in loads)
    assert any(isinstance(f.prev, FS.Frame) and f.prev.flags & NC and not f.flags & NC for f in loads)
    assert len({FS.hooks_of(seed) for seed in sequences}) == len(sequences)


def test_scene_sizes_and_the_fan_overflow(sequences):
    scenes, mats = FS.world()
    n = {name: s[1].size // 3 for name, s in scenes.items()}
    assert n == FS.SCENES and n["big"] >= 4 * n["small"] and n["zero"] == n["small"] and n["straddle"] == n["big"]
    v, i, _ = scenes["zero"]
    assert (DC.clip_space(v, mats["aff"])[:, 2] <= 0).sum() > 50
    # the straddling scene: more fan triangles than the slots of a first depth-clip frame, under either transform
    v, i, _ = scenes["straddle"]
    for tf in ("aff", "per"):
        assert DC.restate(v, i, mats[tf])[3].size > n["straddle"] + 2 * FS.FIRST_FAN_CAPACITY
    for seed, ops in sequences.items():
        for run in FS.runs(ops):
            clips = [k for k, (f, _) in enumerate(run) if f.scene == "straddle" and f.flags & CLIP and f.kind == "tri"]
            assert all(k == len(run) - 1 for k in clips), "a depth-clip frame of the straddling scene that is not the last of its burst"
        tails = [run for run in FS.runs(ops) if run[-1][0].scene == "straddle" and run[-1][0].flags & CLIP]
        assert tails and len(tails[0]) >= 3 and tails[0][-1][1], seed
        k = ops.index(("frame", tails[0][0][0]))
        assert any(o[0] == "frame" for o in ops[:k]) and any(o[0] == "frame" for o in ops[k + 12:])       # frames of other kinds around it


def test_every_pair_of_factor_values_is_checked(sequences):
    """2(b), first condition: every pair of values of two different factors occurs in a frame whose image is compared."""
    seen = set()
    for ops in sequences.values():
        for f in FS.checked_frames(ops):
            seen |= FM.pairs_of(f.row())
    missing = FM.all_pairs() - seen
    assert not missing, sorted(missing)


BINARY = {"DEPTH_CLIP": lambda f: bool(f.flags & CLIP), "PERSPECTIVE": lambda f: bool(f.flags & PERSP),
          "PRIMITIVE_IDS": lambda f: bool(f.flags & IDS), "LOAD": lambda f: bool(f.flags & LOAD), "NO_COLOR": lambda f: bool(f.flags & NC),
          "draw list": lambda f: f.via == "list", "shader": lambda f: f.shader > 0}


@pytest.mark.parametrize("d", [1, 4])
@pytest.mark.parametrize("name", list(BINARY))
def test_ordered_pairs_inside_bursts(sequences, name, d):
    """2(b), second condition: (value in frame k, value in frame k + d) takes all four values inside un-waited bursts, frame k + d
    compared — d = 1: neighbouring lanes; d = 4 (NSLOT): the same lane's working set."""
    got = set()
    for ops in sequences.values():
        for run in FS.runs(ops):
            for k in range(len(run) - d):
                a, (b, checked) = run[k][0], run[k + d]
                if checked and a.kind == b.kind == "tri":
                    got.add((BINARY[name](a), BINARY[name](b)))
    assert len(got) == 4, (name, d, got)


def test_triangle_frames_behind_a_points_or_lines_frame(sequences):
    """2(b), third condition (the lanes' framebuffers): a .vertices or .line frame, then four or more triangle frames
    with no wait between them, all compared."""
    found = 0
    for seed, ops in sequences.items():
        for run in FS.runs(ops):
            for k, (f, _) in enumerate(run):
                if f.kind != "tri":
                    n = 0
                    for g, checked in run[k + 1:]:
                        if g.kind != "tri" or not checked:
                            break
                        n += 1
                    found += n >= 4
    assert found >= 1


def test_covering_array_covers_every_pair():
    rows = FS.covering_rows()
    assert rows == FM.covering_array() and len(rows) <= 24
    seen = set()
    for r in rows:
        assert set(r) == set(FM.FACTORS) and all(r[f] in FM.FACTORS[f] for f in r)
        assert FM.row_of(FM.flags_of(r), r["shader"], r["list"], r["transform"] == "perspective") == r
        seen |= FM.pairs_of(r)
    assert seen == FM.all_pairs()
    # the array as it was before its construction was shared with the blend space (sha256 of repr(rows), taken at that commit)
    assert len(rows) == 17 and hashlib.sha256(repr(rows).encode()).hexdigest() == "4f168030f9eb5bb1012980bc149e2983fed1f8d79cf5bfd8150395616a3c4fbe"
    for r in rows:                                      # the frames the rows turn into are the rows
        for target in ("small",):
            assert FS.pair_spec(r, target).row() == r


def test_no_frame_inside_a_burst_can_overflow_its_bins(oracle, sequences, blend_sequences):
    """Legal sequences: a presented frame that is not the last of its burst and overflows its bins would be reported as
    SWR_ERR_FRAME_DROPPED.  Every such frame stays below the first guess of a tile region by its bounding boxes."""
    seen = {}
    for ops in list(sequences.values()) + list(blend_sequences.values()):
        for run in FS.runs(ops):
            for f, _ in run[:-1] if run[-1][0].scene == "straddle" and run[-1][0].flags & CLIP else run:
                if f.kind != "tri":
                    continue
                key = (f.scene, f.size, f.via == "list", f.tf, bool(f.flags & CLIP))
                if key not in seen:
                    s = FS.spec_of(f)
                    s.flags &= CLIP
                    seen[key] = FS.tile_load(oracle, s)
                load, n = seen[key]
                assert load <= min(FS.SCENES[f.scene], 1024) * 0.9, (key, load, n)
