"""CPU tests of tests/frame_model.py (no GPU): the one expectation equals the expectation every per-feature test file already
uses, the reductions include/swr.h promises hold, the golden fixtures reproduce through it, and the sequences and the covering array
of tests/test_frame_sequences.py meet their coverage conditions."""
import dataclasses
import glob
import os

import numpy as np
import pytest

import frame_model as FM
import kernel_matrix as K
import test_depth_clip as DC
import test_frame_sequences as FS
import test_perspective as TP
from frame_model import CB, CCW, CF, CLIP, DT, IDS, LOAD, METAL, NC, PERSP

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
    for r in rows:                                      # the frames the rows turn into are the rows
        for target in ("small",):
            assert FS.pair_spec(r, target).row() == r


def test_no_frame_inside_a_burst_can_overflow_its_bins(oracle, sequences):
    """Legal sequences: a presented frame that is not the last of its burst and overflows its bins would be reported as
    SWR_ERR_FRAME_DROPPED.  Every such frame stays below the first guess of a tile region by its bounding boxes."""
    seen = {}
    for ops in sequences.values():
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
