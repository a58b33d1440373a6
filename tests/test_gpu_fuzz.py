"""Seeded random scenes against the oracle: image sizes (tile counts on both sides of the kernels' grid thresholds), triangle
counts and sizes (sparse / dense tiles, row-split and wide chunks, triangles for the deferred list), every rule set, colour
and depth-only, one context or bands, one-shot renders and frame loops.  40 cases in the suite;  SWR_FUZZ_CASES=400 for more.
Every case then draws one more frame of its scene with random newer flags (primitive IDs, culling, depth clipping, perspective
correction, the load action) against tests/frame_model.py; those random numbers come from a generator of their own, so the cases
above are the cases they always were."""
import os

import numpy as np
import pytest

import frame_model as FM

DT, NC, MR = 1, 2, 4


def newer_flags(rng2, ntri, w, h, flags, affine):
    """Random bits of the flags that came after this file.  The NumPy models bound two of them: depth clipping restates the scene
    triangle by triangle in Python (scenes up to 3 000 triangles), and perspective correction of a colour frame under a projective
    matrix goes through the per-row model (up to 600 triangles on up to 640 x 360 pixels); elsewhere the C oracle does the work."""
    extra = int(rng2.choice([0, FM.IDS])) | int(rng2.choice([0, FM.CB, FM.CF, FM.CB | FM.CF])) | int(rng2.choice([0, FM.CCW]))
    extra |= int(rng2.choice([0, FM.LOAD]))
    if ntri <= 3000 and rng2.integers(0, 2):
        extra |= FM.CLIP
    cheap = affine or flags & NC or (ntri * (3 if extra & FM.CLIP else 1) <= 600 and w * h <= 640 * 360)
    if cheap and rng2.integers(0, 2):
        extra |= FM.PERSP
    return extra


def one_case(swr, oracle, rng, case, rng2):
    S = swr.scenes
    w = int(rng.choice([64, 200, 255, 512, 640, 960, 1280, 1920]))
    h = int(rng.choice([32, 129, 256, 360, 540, 720, 1080]))
    kind = int(rng.integers(0, 5))
    if kind == 0:   ntri, r = int(rng.integers(1, 60)), float(rng.uniform(0.3, 1.6))         # few, large
    elif kind == 1: ntri, r = int(rng.integers(100, 700)), float(rng.uniform(0.2, 0.9))      # many large: deep tiles
    elif kind == 2: ntri, r = int(rng.integers(2000, 40000)), float(rng.uniform(0.005, 0.05))  # small
    elif kind == 3: ntri, r = int(rng.integers(300, 6000)), float(rng.uniform(0.05, 0.25))   # mid-size: 100-200 per tile
    else:           ntri, r = int(rng.integers(1, 3000)), float(rng.uniform(0.01, 1.0))
    # keep the oracle's work bounded (fragments ~ ntri * (r * w / 2)^2 / 2)
    while ntri * (r * w * 0.5) * (r * h * 0.5) * 0.5 > 1.5e8 and ntri > 1:
        ntri //= 2
    s = S.random_soup(ntri, w, h, 0xF000 + case, r_ndc=r, flags=DT, margin=float(rng.uniform(0.5, 1.2)), shared=bool(rng.integers(0, 2)))
    if kind == 4 and ntri > 40:                                    # a few tile-spanning triangles among the rest
        b = S.random_soup(int(rng.integers(1, 12)), w, h, 0xF800 + case, r_ndc=1.3, flags=DT, margin=0.7)
        s = S.Scene("mix", w, h, np.concatenate([b.vertices, s.vertices]),
                    np.concatenate([b.indices, s.indices + b.vertices.shape[0]]), s.transform, DT)
    flags = int(rng.choice([DT, DT | NC, 0, NC, MR, MR | NC]))
    m = S.app_transform(float(rng.uniform(0, 6.28))) if rng.integers(0, 3) == 0 else s.transform
    # the extended fragment stage (per-pixel Phong, textured) on a third of the colour frames
    sh = None
    if not (flags & NC) and rng.integers(0, 3) == 0:
        sh = S.random_shading(s.vertices.shape[0], 0xFA00 + case, int(rng.choice([S.SHADER_PHONG, S.SHADER_TEXTURED_PHONG])),
                              shininess_log2=int(rng.integers(0, 7)))
    if flags & MR:
        rc, rd, _, err = oracle.render_metal(s.vertices, s.indices, m, w, h, flags & NC, shading=sh)
    else:
        rc, rd, _, err = oracle.render(s.vertices, s.indices, m, w, h, flags | oracle.TINV_PER_TRIANGLE, shading=sh)
    assert err == 0
    bands = int(rng.choice([0, 0, 2, 3]))
    what = f"case {case}: {ntri} tris r={r:.3f} {w}x{h} flags={flags} bands={bands} kind={kind} shader={None if sh is None else sh.shader}"
    extra = newer_flags(rng2, ntri, w, h, flags, FM.is_affine(m))
    spec = FM.FrameSpec(s.vertices, s.indices, w, h, flags | extra, m, shading=sh)
    start = (None if flags & NC else rc, rd)                       # a load frame goes over the case's own frame
    want = FM.expect(oracle, spec, start)
    what2 = what + f" newer flags {extra:#x}"
    with swr.Context(0, device_count=bands) as ctx:
        if rng.integers(0, 2):
            sid = int(rng.choice([0, 17]))
            c, d = ctx.render(s.vertices, s.indices, m, w, h, flags, shading=sh, scene_id=sid)
            assert d.tobytes() == rd.tobytes(), what + " (render): depth"
            if not (flags & NC):
                assert np.array_equal(c, rc), what + " (render): colour"
            c, d = ctx.render(s.vertices, s.indices, m, w, h, flags | extra, shading=sh, scene_id=sid,
                              color=None if flags & NC else rc.copy(), depth=rd.copy())
            FM.same((None if flags & NC else c, d, ctx.read_ids() if extra & FM.IDS else None), want, what2 + " (render)")
        else:
            ctx.scene_upload(s.vertices, s.indices)
            ctx.target_set(w, h)
            if sh is not None:
                ctx.shading_set(sh)
            for frame in range(3):                                  # (frames 2 and 3: sort heuristics and the deferred list settle)
                ctx.draw(m, flags)
                ctx.sync()
                assert ctx.read_depth().tobytes() == rd.tobytes(), what + f" (frame {frame}): depth"
                if not (flags & NC):
                    assert np.array_equal(ctx.read_color(), rc), what + f" (frame {frame}): colour"
            ctx.draw(m, flags | extra)                              # (SWR_FLAG_LOAD: over the image of the frame just checked)
            ctx.sync()
            FM.same((None if flags & NC else ctx.read_color(), ctx.read_depth(), ctx.read_ids() if extra & FM.IDS else None), want,
                    what2 + " (resident)")


@pytest.mark.gpu
def test_seeded_random_scenes(swr, oracle):
    cases = int(os.environ.get("SWR_FUZZ_CASES", "40"))
    rng = np.random.default_rng(int(os.environ.get("SWR_FUZZ_SEED", "20261004")))
    rng2 = np.random.default_rng([0x6E77, int(os.environ.get("SWR_FUZZ_SEED", "20261004"))])
    for case in range(cases):
        one_case(swr, oracle, rng, case, rng2)
