#!/usr/bin/env python3
"""Headless version of the reference app's frame loop (renderer/App.swift:153-188).

Every frame the app builds `projection * Transform(scale 2, rotation(time), translation (0,0,1))`
(App.swift:169-183), hands the same sphere mesh to `renderer.render(renderPass:)` (App.swift:185)
and advances `time += 1/60` (App.swift:155-157).  Here the mesh stays resident on the MI355X
(swr_scene_upload once), each frame is one swr_draw, and frames are written as binary PPM.

    python examples/frame_loop.py --frames 4 --size 512 --out /tmp/frames [--obj mesh.obj] [--depth-test] [--objects N]
                                   [--cull back [--front-ccw]] [--ssaa {1,2,4}] [--ids] [--pick X,Y [--lit]] [--occlusion [--bounds]] [--delta] [--skin [--dq]] [--morph [--sparse]]
                                   [--auto-normals {smooth,flat}]

--objects N draws N copies of the mesh, each with its own model matrix (its own spin, its own place on screen), as ONE draw list
per frame (swr_draw_list: the mesh is uploaded once, every copy is an item over its whole index range).
--pick X,Y also writes every frame's ID image (SWR_FLAG_PRIMITIVE_IDS) and prints which copy of the mesh and which of its
triangles are visible at pixel (X, Y): mouse picking (use it with --objects N).
--pick X,Y --lit repeats the pick with rays (swr_query_rays): the pixel's ray is brought into every copy's object space and cast against
that copy's range of triangles only, the nearest copy is reported, and one occlusion ray from the picked point towards the light says
whether the point is lit or in the copy's own shadow.
--ids writes the ID image too and after the last frame prints how many triangles of it are visible and how many
pixels every copy covers, counted on the device (swr_count_ids: only the counts cross to the host, not the ID image).
--occlusion (with --objects N and --depth-test) tests every copy's screen rectangle and nearest depth against the depth image of the
previous frame before the next one is drawn, on the device (swr_query_depth: only one count per copy crosses to the host, not the
depth image), and prints how many copies could be skipped because nothing of them would pass the z-test.
--bounds (with --occlusion) takes every copy's rectangle and nearest depth from the device instead of projecting the vertices on the
host (swr_item_bounds: 48 bytes per copy cross, in the arithmetic the frame itself uses).  The posed and morphed vertices exist only on
the device, so --occlusion --bounds is what combines with --skin and --morph: the copies are then copies of the bending, breathing torus.
--delta runs the host-visible loop the way the app calls it — one swr_render per frame, the same mesh, a new transform, the same two host
images — through swr_render_delta: the device compares every frame with what the host images already hold, tile by tile, and only the
rectangle around the tiles that changed crosses to the host.  It prints the tiles that changed per frame.
--skin draws a torus that bends between two joints instead: the mesh and its per-vertex joint weights are uploaded once
(swr_scene_upload, swr_scene_skin), and every frame sets a new pose of two joint matrices (swr_pose_set) — the vertices are posed on
the device, nothing but 128 bytes of pose crosses per frame — and draws it with the app's transform.  --skin --dq adds a twist of the
two ends against each other and sets the pose as dual quaternions (swr_pose_set_dq, 64 bytes per frame): the joints are blended as rigid
motions, so the twisting tube keeps its volume where the blended matrices of swr_pose_set would pinch it.
--morph gives the mesh two procedural morph targets (blend shapes) — a swell along the direction from the mesh's centre and a twist
about z — uploaded once (swr_scene_morph), and every frame sets two new weights (swr_morph_set): the vertices are morphed on the
device, nothing but the weights crosses per frame.  With --skin the torus is morphed first and then posed, as glTF orders the two.
--morph --sparse uploads the same two targets as sparse ones (swr_scene_morph_sparse): each lists only the vertices it moves, and only
those are stored and rewritten on the device.  With --skin the weights and the pose are then set by one call (swr_morph_pose_set), which
rewrites the scene once per frame instead of twice.
--auto-normals smooth|flat (with --skin and / or --morph) lights the deforming mesh with a Phong material although it brings no
normals and its targets no normal deltas: the device computes them from the deformed positions after every pose and morph call
(swr_scene_normals), per vertex (smooth) or per triangle (flat).
--cull {none,back,front} [--front-ccw] turns on face culling (Metal's setCullMode / setFrontFacingWinding): triangles that face
away (back) or towards the viewer (front) are not drawn; front is clockwise as displayed unless --front-ccw.

--ssaa S (2 or 4) draws every frame at S*size x S*size and resolves it on the device with an S x S box filter
(swr_read_color_resolved / swr_read_depth_resolved): anti-aliased edges, alpha = the coverage of the pixel; only the size x size image
crosses to the host.  With --pick the ID image stays at sample resolution and X,Y address the size x size image.  Default 1: as before.

The demo mesh is a UV sphere standing in for ModelIO's `MDLMesh(sphereWithExtent: 0.4, segments: 13x13,
inwardNormals: true)` (App.swift:124) with colour = |normal| (App.swift:133).  `--obj` loads a
Wavefront OBJ instead (positions + optional normals; faces are fan-triangulated); `--ply` a Stanford PLY
(ascii or binary_little_endian; x y z, optional nx ny nz or red green blue; faces fan-triangulated) — the format
the Stanford bunny ships in.  Neither format is part of the reference (its only mesh is the ModelIO sphere).
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import swr_amd  # noqa: E402

S = swr_amd.scenes


def sphere_mesh(extent: float = 0.4, segments: int = 13):
    """UV sphere, `segments` x `segments`, colour = |normal|."""
    nu, nv = segments, segments
    r = extent / 2.0
    verts, cols, idx = [], [], []
    for j in range(nv + 1):
        phi = math.pi * j / nv
        for i in range(nu + 1):
            th = 2.0 * math.pi * i / nu
            n = (math.sin(phi) * math.cos(th), math.cos(phi), math.sin(phi) * math.sin(th))
            verts.append((r * n[0], r * n[1], r * n[2]))
            cols.append((abs(n[0]), abs(n[1]), abs(n[2])))
    for j in range(nv):
        for i in range(nu):
            a = j * (nu + 1) + i
            b = a + 1
            c = a + nu + 1
            d = c + 1
            idx += [a, c, b, b, c, d]
    return (S.pack_vertices(np.array(verts, dtype=np.float32), np.array(cols, dtype=np.float32)),
            np.array(idx, dtype=np.int64))


def load_obj(path: str):
    """Minimal Wavefront OBJ reader: v, vn, f (v, v/vt, v//vn, v/vt/vn; negative indices; n-gons)."""
    pos, nrm, out_v, out_c, idx = [], [], [], [], []
    cache = {}
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if t[0] == "v":
                pos.append(tuple(float(x) for x in t[1:4]))
            elif t[0] == "vn":
                nrm.append(tuple(float(x) for x in t[1:4]))
            elif t[0] == "f":
                face = []
                for tok in t[1:]:
                    parts = tok.split("/")
                    vi = int(parts[0])
                    vi = vi - 1 if vi > 0 else len(pos) + vi
                    ni = None
                    if len(parts) == 3 and parts[2]:
                        ni = int(parts[2])
                        ni = ni - 1 if ni > 0 else len(nrm) + ni
                    key = (vi, ni)
                    if key not in cache:
                        cache[key] = len(out_v)
                        out_v.append(pos[vi])
                        n = nrm[ni] if ni is not None else (0.577, 0.577, 0.577)
                        out_c.append(tuple(abs(x) for x in n))
                    face.append(cache[key])
                for k in range(1, len(face) - 1):
                    idx += [face[0], face[k], face[k + 1]]
    return (S.pack_vertices(np.array(out_v, dtype=np.float32), np.array(out_c, dtype=np.float32)),
            np.array(idx, dtype=np.int64))


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def load_ply(path: str):
    """Minimal Stanford PLY reader (ascii 1.0 / binary_little_endian 1.0): element vertex with x y z and optional
    nx ny nz (colour = |normal|, as the app does, App.swift:133) or red green blue (uchar 0..255 or float 0..1);
    element face with one list property (vertex_indices), fan-triangulated.  Other elements / properties are skipped."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:                          # EOF before end_header (readline returns b"" for ever)
                raise ValueError("PLY header without end_header")
            t = line.decode("ascii", "replace").split()
            if not t:
                continue
            if t[0] == "format":
                fmt = t[1]
            elif t[0] == "element":
                elements.append({"name": t[1], "count": int(t[2]), "props": []})
            elif t[0] == "property":
                if t[1] == "list":
                    elements[-1]["props"].append(("list", t[2], t[3], t[4]))
                else:
                    elements[-1]["props"].append(("scalar", t[1], t[2]))
            elif t[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError(f"unsupported PLY format {fmt}")
        verts, faces = None, []
        if fmt == "ascii":
            tokens = f.read().split()
            pos = 0
        for el in elements:
            scalars = [p for p in el["props"] if p[0] == "scalar"]
            lists = [p for p in el["props"] if p[0] == "list"]
            if el["name"] == "vertex" and not lists:
                names = [p[2] for p in scalars]
                if fmt == "ascii":
                    n = len(names) * el["count"]
                    arr = np.array(tokens[pos:pos + n], dtype=np.float64).reshape(el["count"], len(names))
                    pos += n
                    cols = {nm: arr[:, k] for k, nm in enumerate(names)}
                    isint = {p[2]: _PLY_TYPES[p[1]][0] in "iu" for p in scalars}
                else:
                    dt = np.dtype([(p[2], "<" + _PLY_TYPES[p[1]]) for p in scalars])
                    arr = np.frombuffer(f.read(dt.itemsize * el["count"]), dtype=dt)
                    cols = {nm: arr[nm].astype(np.float64) for nm in names}
                    isint = {p[2]: _PLY_TYPES[p[1]][0] in "iu" for p in scalars}
                xyz = np.stack([cols["x"], cols["y"], cols["z"]], -1).astype(np.float32)
                if all(k in cols for k in ("red", "green", "blue")):
                    rgb = np.stack([cols["red"], cols["green"], cols["blue"]], -1)
                    if isint["red"]:
                        rgb = rgb / 255.0
                elif all(k in cols for k in ("nx", "ny", "nz")):
                    rgb = np.abs(np.stack([cols["nx"], cols["ny"], cols["nz"]], -1))
                else:
                    rgb = np.full(xyz.shape, 0.577)
                verts = (xyz, rgb.astype(np.float32))
            else:                                   # faces (or anything else: parsed to stay in sync, kept only for "face")
                for _ in range(el["count"]):
                    row_lists = []
                    for p in el["props"]:
                        if p[0] == "scalar":
                            if fmt == "ascii":
                                pos += 1
                            else:
                                f.read(np.dtype(_PLY_TYPES[p[1]]).itemsize)
                        else:
                            if fmt == "ascii":
                                n = int(tokens[pos]); pos += 1
                                row_lists.append([int(x) for x in tokens[pos:pos + n]]); pos += n
                            else:
                                n = int(np.frombuffer(f.read(np.dtype(_PLY_TYPES[p[1]]).itemsize), dtype="<" + _PLY_TYPES[p[1]])[0])
                                dt = np.dtype("<" + _PLY_TYPES[p[2]])
                                row_lists.append(np.frombuffer(f.read(dt.itemsize * n), dtype=dt).astype(np.int64).tolist())
                    if el["name"] == "face" and row_lists:
                        face = row_lists[0]
                        for k in range(1, len(face) - 1):
                            faces += [face[0], face[k], face[k + 1]]
        if verts is None:
            raise ValueError("PLY file without a vertex element")
    return S.pack_vertices(verts[0], verts[1]), np.array(faces, dtype=np.int64)


def write_ply(path: str, vertices: np.ndarray, indices: np.ndarray, binary: bool = True):
    """Writes the mesh as PLY (x y z + float red green blue; triangles) — the inverse of load_ply, for round trips."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 8)
    tri = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    hdr = ("ply\nformat %s 1.0\ncomment written by examples/frame_loop.py\nelement vertex %d\nproperty float x\nproperty float y\n"
           "property float z\nproperty float red\nproperty float green\nproperty float blue\nelement face %d\n"
           "property list uchar int vertex_indices\nend_header\n") % ("binary_little_endian" if binary else "ascii", v.shape[0], tri.shape[0])
    with open(path, "wb") as f:
        f.write(hdr.encode("ascii"))
        if binary:
            f.write(np.ascontiguousarray(v[:, [0, 1, 2, 4, 5, 6]], dtype="<f4").tobytes())
            rec = np.zeros(tri.shape[0], dtype=[("n", "u1"), ("i", "<i4", 3)])
            rec["n"] = 3
            rec["i"] = tri
            f.write(rec.tobytes())
        else:
            for row in v[:, [0, 1, 2, 4, 5, 6]]:
                f.write((" ".join(repr(float(x)) for x in row) + "\n").encode("ascii"))
            for t in tri:
                f.write(("3 %d %d %d\n" % tuple(int(x) for x in t)).encode("ascii"))


def load_mesh(path: str):
    return load_ply(path) if path.lower().endswith(".ply") else load_obj(path)


def write_ppm(path: str, bgra: np.ndarray):
    h, w, _ = bgra.shape
    with open(path, "wb") as f:
        f.write(f"P6\n{w} {h}\n255\n".encode())
        f.write(np.ascontiguousarray(bgra[..., [2, 1, 0]]).tobytes())


def object_transforms(time: float, n: int):
    """The app's matrix for n copies of the mesh: copy j spins with its own phase and sits at its own place on an
    ceil(sqrt(n))-wide grid (a screen-space offset applied after the projection: x' = x + dx * w)."""
    g = max(1, math.ceil(math.sqrt(n)))
    out = []
    for j in range(n):
        m = S.app_transform(time + 0.37 * j, scale=2.0 / g).reshape(4, 4).copy()     # rows = columns (column-major)
        dx = (2.0 * (j % g) + 1.0) / g - 1.0
        dy = 1.0 - (2.0 * (j // g) + 1.0) / g
        m[:, 0] += np.float32(dx) * m[:, 3]
        m[:, 1] += np.float32(dy) * m[:, 3]
        out.append(np.ascontiguousarray(m.reshape(16), dtype=np.float32))
    return out


def object_boxes(vertices: np.ndarray, matrices, width: int, height: int) -> np.ndarray:
    """One swr_query_depth box per matrix: the screen rectangle of the transformed vertices, one pixel wider on every side and
    clipped to the target, and their nearest depth moved a little nearer (the projection here is not bit for bit the device's, and
    the box has to be conservative); rows (x0, y0, x1, y1, z) for Context.query_depth."""
    h = np.concatenate([vertices[:, :3].astype(np.float64), np.ones((vertices.shape[0], 1))], axis=1)
    rows = []
    for m in matrices:
        c = h @ np.asarray(m, dtype=np.float64).reshape(4, 4)       # (column-major: the rows of the reshape are the columns)
        ndc = c[:, :3] / c[:, 3:4]
        sx, sy = (ndc[:, 0] + 1.0) * 0.5 * width, (1.0 - (ndc[:, 1] + 1.0) * 0.5) * height
        x0, x1 = int(np.clip(math.floor(sx.min()) - 1, 0, width)), int(np.clip(math.ceil(sx.max()) + 2, 0, width))
        y0, y1 = int(np.clip(math.floor(sy.min()) - 1, 0, height)), int(np.clip(math.ceil(sy.max()) + 2, 0, height))
        z = float(ndc[:, 2].min())
        rows.append((x0, y0, max(x0, x1), max(y0, y1), z - 1e-5 * abs(z) - 1e-6))
    return np.array(rows, dtype=np.float64).reshape(-1, 5)


# --bounds: how far in front of an item's nearest vertex its box is tested.  swr_item_bounds gives the nearest VERTEX; a fragment's
# interpolated depth can lie in front of it by rounding (and, under the CPU rules, by extrapolation at span pixels outside the
# triangle), so the caller subtracts a margin of their own: generous here, the depths of the app's scene are of order 1.
BOUNDS_Z_MARGIN = 2.0 ** -12


def cull_flags(cull: str = "none", front_ccw: bool = False) -> int:
    """Face culling (Metal's setCullMode / setFrontFacingWinding): none / back / front, front = clockwise as displayed unless
    front_ccw."""
    b = swr_amd.binding
    return {"none": 0, "back": b.FLAG_CULL_BACK, "front": b.FLAG_CULL_FRONT}[cull] | (b.FLAG_FRONT_CCW if front_ccw else 0)


def view_flags(clip: bool = False, perspective: bool = False) -> int:
    """Depth clipping (Metal's MTLDepthClipMode.clip: a camera may move into the scene) and perspective-correct interpolation of
    colour and varyings (Metal's [[center_perspective]]): both off by default, as in the reference."""
    b = swr_amd.binding
    return (b.FLAG_DEPTH_CLIP if clip else 0) | (b.FLAG_PERSPECTIVE if perspective else 0)


def run(frames: int, size: int, out: str | None, obj: str | None = None, depth_test: bool = False,
        time0: float = 0.0, objects: int = 1, pick: tuple[int, int] | None = None, cull: str = "none", front_ccw: bool = False,
        clip: bool = False, perspective: bool = False, glass: int | None = None, ssaa: int = 1, ids: bool = False,
        occlusion: bool = False, bounds: bool = False, skin: bool = False, morph: bool = False, dq: bool = False, lit: bool = False):
    """Returns the list of (colour, depth) frames; writes PPMs when `out` is given.  objects > 1: that many copies of the
    mesh, one draw list per frame (the third element of every result is then the list of matrices).  pick = (x, y): every
    frame also writes its ID image (SWR_FLAG_PRIMITIVE_IDS) and prints which copy and which triangle are under that pixel.
    lit (with pick): the pick is repeated with rays through every copy's own range and transform, and one occlusion ray says whether
    the picked point is lit (pick_lit, swr_query_rays).
    ids: the ID image is written, and after the last frame its visibility counts are printed (swr_count_ids).
    occlusion: from the second frame on, every copy's screen rectangle and nearest depth are tested against the previous frame's depth
    image before the frame is drawn (swr_query_depth), and the number of copies nothing of which would pass is printed.
    bounds (with occlusion): the boxes come from the device (swr_item_bounds) instead of object_boxes; an item with a corner behind
    the eye is never counted as skippable.  skin / morph (with occlusion and bounds): the mesh is the torus of run_skin, morphed
    and / or posed anew every frame — its vertices exist only on the device, so only the device can say where a copy lands.
    dq (with skin): the pose is the twisting one of twist_pose, set as dual quaternions (swr_pose_set_dq).
    cull / front_ccw: face culling (cull_flags); clip / perspective: view_flags.
    glass = A (0..255): after the opaque frame a second, shifted and smaller instance of the mesh is drawn over it as a blend load
    frame (SWR_FLAG_BLEND | SWR_FLAG_LOAD, SWR_BLEND_OVER at opacity A): you see the first instance through it; the depth image stays
    the opaque frame's (not with --pick or --perspective).
    ssaa = S (2 or 4): the frames are drawn at S * size and resolved on the device to size x size (the depth is sample (0,0))."""
    if (skin or morph) and not (occlusion and bounds):
        raise ValueError("skin / morph in this loop need occlusion and bounds (run_skin and run_morph are the plain loops)")
    if bounds and clip:
        raise ValueError("swr_item_bounds does not take SWR_FLAG_DEPTH_CLIP")
    if skin or morph:
        xyz, rgb, indices = S.torus_mesh(96, 32, 0.3, 0.1)
        vertices = S.pack_vertices(xyz, rgb)
    else:
        vertices, indices = load_mesh(obj) if obj else sphere_mesh()
    flags = (S.FLAG_DEPTH_TEST if depth_test else 0) | (swr_amd.binding.FLAG_PRIMITIVE_IDS if pick or ids else 0) | cull_flags(cull, front_ccw)
    flags |= view_flags(clip, perspective)
    results = []
    with swr_amd.Context() as ctx:
        ctx.scene_upload(vertices, indices)            # RenderPass.vertices / .indices, App.swift:163
        if morph:
            ctx.scene_morph(morph_targets(vertices))
        if skin:
            ctx.scene_skin(*bend_skin(vertices))
        ctx.target_set(ssaa * size, ssaa * size)        # MetalView.Coordinator.width/height, App.swift:52-53 (times the samples per axis)
        time = time0
        for k in range(frames):
            if morph:
                ctx.morph_set(morph_weights(time))
            if skin and dq:
                ctx.pose_set_dq(swr_amd.binding.dual_quats(twist_pose(time)))
            elif skin:
                ctx.pose_set(bend_pose(time))
            if objects > 1:
                m = object_transforms(time, objects)
                items = [(0, indices.size, mj) for mj in m]
                if occlusion and k > 0:
                    # the occlusion query of this frame's copies against the depth the previous frame left on the device (samples, with --ssaa)
                    if bounds:
                        where = ctx.item_bounds(items, flags)       # the scene as it is now: morphed and posed
                        passed = ctx.query_depth(swr_amd.binding.depth_boxes(where, BOUNDS_Z_MARGIN))
                        passed[(where["behind"] != 0) & (passed == 0)] = 1      # (drawn mirrored through the eye: never culled on its bounds)
                    else:
                        passed = ctx.query_depth(object_boxes(vertices, m, ssaa * size, ssaa * size))
                    print(f"occlusion: frame {k}: {int((passed == 0).sum())} of {objects} objects could be skipped "
                          f"(pixels that pass per object: {passed.tolist()})")
                ctx.draw_list(items, flags)             # all copies in one frame
            else:
                m = S.app_transform(time)               # App.swift:169-183
                items = [(0, indices.size, m)]
                ctx.draw(m, flags)                      # renderer.render(renderPass:), App.swift:185
            if glass is not None:
                # the transparent pass: tested against the opaque scene's depth (with --depth-test), blended in draw order, no depth write
                g = S.app_transform(time + 0.8, scale=0.7).reshape(4, 4).copy()
                g[:, 0] += np.float32(0.25) * g[:, 3]
                ctx.blend_set(swr_amd.binding.BLEND_OVER, glass)
                ctx.draw(np.ascontiguousarray(g.reshape(16), dtype=np.float32),
                         flags | swr_amd.binding.FLAG_BLEND | swr_amd.binding.FLAG_LOAD)
            if ssaa > 1:
                color, depth = ctx.read_color_resolved(ssaa), ctx.read_depth_resolved(ssaa)
            else:
                color, depth = ctx.read_color(), ctx.read_depth()
            if pick:
                # mouse picking: the ID under the pixel, mapped to (copy, triangle of the mesh) over the list's item bases
                x, y = pick
                id_image = ctx.read_ids()[::ssaa, ::ssaa]     # (IDs are not resolved: sample (0,0) of the pixel, like the depth)
                obj_k, tri = swr_amd.binding.list_ids_to_items(id_image[y:y + 1, x:x + 1], items)
                if obj_k[0, 0] < 0:
                    print(f"frame {k}: pixel ({x}, {y}): nothing")
                else:
                    print(f"frame {k}: pixel ({x}, {y}): copy {obj_k[0, 0]}, triangle {tri[0, 0]}, depth {depth[y, x]:.6g}")
                if lit:
                    pick_lit(ctx, items, size, pick, k)     # the same pick through each copy's own rays, and whether the point is lit
            results.append((color, depth, m))
            if out:
                os.makedirs(out, exist_ok=True)
                write_ppm(os.path.join(out, f"frame_{k:04d}.ppm"), color)
            time += 1.0 / 60.0                          # App.swift:155-157
        if ids and frames > 0:
            # visibility of the last frame, reduced on the device: pixels per triangle and per copy (samples, with --ssaa)
            per_tri, none = ctx.count_ids(swr_amd.binding.COUNT_PER_PRIMITIVE)
            per_copy, _ = ctx.count_ids(swr_amd.binding.COUNT_PER_ITEM)
            print(f"last frame: {np.count_nonzero(per_tri)} of {per_tri.size} triangles visible, {none} of {(ssaa * size) ** 2} "
                  f"pixels empty, pixels per copy: {per_copy.tolist()}")
    return vertices, indices, results


def run_streamed(frames: int, size: int, obj: str | None = None, depth_test: bool = False, time0: float = 0.0,
                 device_count: int = 1, on_frame=None, cull: str = "none", front_ccw: bool = False, clip: bool = False,
                 perspective: bool = False):
    """The same loop the way a host that wants every frame should drive it: two page-locked
    image sets alternate; frame k is being copied to the host (swr_present, asynchronous, every band of a multi-GPU
    context into its rows of the ONE image) while frame k+1 is drawn; the host touches frame k only after
    swr_present_wait.  `on_frame(k, colour, depth)` sees the host images (valid until the next but one present).
    Returns the frames (copies)."""
    vertices, indices = load_mesh(obj) if obj else sphere_mesh()
    flags = (S.FLAG_DEPTH_TEST if depth_test else 0) | cull_flags(cull, front_ccw) | view_flags(clip, perspective)
    sets = [(swr_amd.HostImage((size, size, 4), np.uint8), swr_amd.HostImage((size, size), np.float32)) for _ in range(2)]
    results = []

    def deliver(k):
        c, d = sets[k & 1]
        if on_frame:
            on_frame(k, c.array, d.array)
        results.append((c.array.copy(), d.array.copy()))

    with swr_amd.Context(0, device_count=device_count) as ctx:
        ctx.scene_upload(vertices, indices)
        ctx.target_set(size, size)
        time = time0
        for k in range(frames):
            ctx.draw(S.app_transform(time), flags)
            ctx.present(*sets[k & 1])                   # returns at once
            if k >= 1:
                ctx.present_wait()                      # every enqueued copy has landed: frame k-1 (and k) are host-visible
                deliver(k - 1)
            time += 1.0 / 60.0
        ctx.present_wait()
        if frames:
            deliver(frames - 1)
    for c, d in sets:
        c.free(); d.free()
    return results


def run_delta(frames: int, size: int, obj: str | None = None, depth_test: bool = False, time0: float = 0.0,
              device_count: int = 1, out: str | None = None):
    """The host-visible loop through swr_render_delta: the mesh is cached on the device by its scene identity, every frame carries a
    new transform, and the two page-locked host images keep what the last frame delivered, so only the rectangle around the tiles
    that changed is copied.  Prints the tiles changed per frame; returns the frames (copies) and the (colour, depth) stats of each."""
    vertices, indices = load_mesh(obj) if obj else sphere_mesh()
    flags = S.FLAG_DEPTH_TEST if depth_test else 0
    color, depth = swr_amd.HostImage((size, size, 4), np.uint8), swr_amd.HostImage((size, size), np.float32)
    results, stats = [], []
    with swr_amd.Context(0, device_count=device_count) as ctx:
        time = time0
        for k in range(frames):
            sc, sd = ctx.render_delta(vertices, indices, S.app_transform(time), size, size, color, depth, flags, scene_id=1)
            print(f"delta: frame {k}: colour {sc.tiles_changed} of {sc.tiles} tiles changed, {sc.bytes_copied} bytes copied"
                  f"{' (full)' if sc.full else ''}; depth {sd.tiles_changed} of {sd.tiles} tiles, {sd.bytes_copied} bytes"
                  f"{' (full)' if sd.full else ''}")
            results.append((color.array.copy(), depth.array.copy()))
            stats.append((sc, sd))
            if out:
                os.makedirs(out, exist_ok=True)
                write_ppm(os.path.join(out, f"frame_{k:04d}.ppm"), color.array)
            time += 1.0 / 60.0
    color.free(); depth.free()
    return results, stats


def bend_skin(vertices: np.ndarray):
    """(joints, weights) of a mesh that bends along x between joint 0 (weight 1 - t) and joint 1 (weight t), t = x mapped to 0..1
    across the mesh; all four influences of swr_skin_vertex are given, the last two with weight 0."""
    x = vertices[:, 0]
    t = np.clip((x - x.min()) / max(float(x.max() - x.min()), 1e-30), 0.0, 1.0).astype(np.float32)
    joints = np.zeros((x.shape[0], 4), dtype=np.uint32)
    joints[:, 1] = 1
    weights = np.zeros((x.shape[0], 4), dtype=np.float32)
    weights[:, 0], weights[:, 1] = 1.0 - t, t
    return joints, weights


def bend_pose(time: float) -> np.ndarray:
    """Two joint matrices (column-major, like a frame's transform): the two ends of the mesh turn about z against each other."""
    def turn(angle, ty):
        c, s = math.cos(angle), math.sin(angle)
        return np.array([c, s, 0, 0, -s, c, 0, 0, 0, 0, 1, 0, 0, ty, 0, 1], dtype=np.float32)
    a = 0.6 * math.sin(2.0 * time)
    return np.stack([turn(a, 0.05 * math.sin(3.0 * time)), turn(-a, -0.05 * math.sin(3.0 * time))])


def twist_pose(time: float) -> np.ndarray:
    """Two rigid joints as (2, 4, 4) mathematical matrices: the bend of bend_pose, and under it a twist of the two ends against each
    other about x — the ring's tangent where the two joints blend.  Blended as matrices the tube would pinch there; blended as dual
    quaternions (binding.dual_quats, swr_pose_set_dq) it keeps its volume."""
    def joint(turn_z, twist_x, ty):
        c, s = math.cos(turn_z), math.sin(turn_z)
        ct, st = math.cos(twist_x), math.sin(twist_x)
        rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        rx = np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]])
        m = np.eye(4)
        m[:3, :3] = rz @ rx
        m[1, 3] = ty
        return m
    a, b = 0.6 * math.sin(2.0 * time), 1.3 * math.sin(1.5 * time + 0.9)
    return np.stack([joint(a, -b, 0.05 * math.sin(3.0 * time)), joint(-a, b, -0.05 * math.sin(3.0 * time))])


def auto_normals_shading(vertices: np.ndarray):
    """The shading of --auto-normals: a mesh that brings no normals (all zero, like its uv) under a Phong material.  The normals the
    frames read are computed on the device from the deformed positions (swr_scene_normals)."""
    light, half = S.light_rig()
    return S.Shading(np.zeros((vertices.shape[0], 8), dtype=np.float32), S.SHADER_PHONG, 4, light, half, 0.2, 0.7, 0.5, None)


def use_auto_normals(ctx, vertices: np.ndarray, mode: str | None):
    """mode "smooth" or "flat": attributes without normals, a Phong material, and normals computed per vertex or per triangle."""
    if mode:
        sh = auto_normals_shading(vertices)
        ctx.scene_attributes(sh.attrs)
        ctx.material_set(swr_amd.binding.Material.from_shading(sh))
        ctx.scene_normals(mode)


def pick_ray(ctx, transform, size: int, pick, frame: int):
    """--pick X,Y on a deforming mesh: the ray through the centre of that pixel, from depth 0 to depth 1 in object space
    (binding.pixel_ray), cast against the resident triangles as they are now (swr_cast_rays).  Prints the triangle, t and the hit point;
    returns the hit record."""
    ray = swr_amd.binding.pixel_ray(transform, size, size, pick[0], pick[1])
    hit = ctx.cast_rays(ray.reshape(1))[0]
    if hit["primitive"] == swr_amd.binding.ID_NONE:
        print(f"frame {frame}: pixel {pick}: no triangle on the ray")
    else:
        p = ray["origin"] + hit["t"] * ray["dir"]
        print(f"frame {frame}: pixel {pick}: triangle {hit['primitive']}, t {hit['t']:.6f}, u {hit['u']:.4f}, v {hit['v']:.4f}, "
              f"hit point ({p[0]:.5f}, {p[1]:.5f}, {p[2]:.5f})")
    return hit


def pick_lit(ctx, items, size: int, pick, frame: int):
    """--pick X,Y --lit: the pick through rays instead of the ID image, and one shadow ray.  For every item (first_index, index_count,
    transform) of the frame the pixel's ray is brought into that item's object space (binding.pixel_ray with the item's transform) and
    cast against that item's triangles only (swr_query_rays with the item's range of primitives); the item whose hit is nearest in
    depth wins.  Then one occlusion ray (any-hit) starts at the hit point, goes towards the light of S.light_rig() — the material's
    light_dir, in object space — with its tmin just off the surface, against the same item's triangles: the point is lit, or the copy
    shadows itself.  Prints the item, the triangle and the verdict; returns (item, hit record, lit) or None."""
    b = swr_amd.binding
    best = None
    for k, (first, count, transform) in enumerate(items):
        ray = b.pixel_ray(transform, size, size, pick[0], pick[1])
        hit = ctx.query_rays(ray.reshape(1), first_primitive=first // 3, primitive_count=count // 3)[0]
        if hit["primitive"] == b.ID_NONE:
            continue
        p = ray["origin"] + hit["t"] * ray["dir"]
        clip = np.asarray(transform, dtype=np.float64).reshape(4, 4).T @ np.append(p.astype(np.float64), 1.0)
        depth = clip[2] / clip[3]
        if best is None or depth < best[0]:
            best = (depth, k, hit, p)
    if best is None:
        print(f"frame {frame}: pixel {pick}: no triangle on the ray of any item")
        return None
    depth, k, hit, p = best
    first, count, _ = items[k]
    light, _ = S.light_rig()
    shadow = np.zeros(1, dtype=b.RAY_DTYPE)
    shadow["origin"], shadow["dir"] = p, light
    shadow["tmin"], shadow["tmax"] = 1e-4, np.finfo(np.float32).max
    occluded = ctx.query_rays(shadow, any_hit=True, first_primitive=first // 3, primitive_count=count // 3)[0]["primitive"] == b.RAY_OCCLUDED
    print(f"frame {frame}: pixel {pick}: item {k}, triangle {hit['primitive'] - first // 3} of it, depth {depth:.6f}: "
          f"{'shadowed' if occluded else 'lit'}")
    return k, hit, not occluded


def run_skin(frames: int, size: int, out: str | None = None, depth_test: bool = True, time0: float = 0.0, device_count: int = 1,
             dq: bool = False, auto_normals: str | None = None, pick=None):
    """The resident loop with a deforming mesh: a torus skinned to two joints, a new pose every frame (swr_pose_set), the app's
    transform.  dq: the pose is twist_pose, which also twists the torus, set as dual quaternions (swr_pose_set_dq).  auto_normals
    ("smooth" / "flat"): lit by a Phong material with normals recomputed on the device after every pose (swr_scene_normals).
    pick (x, y): the triangle and the point of the posed mesh on that pixel's ray, every frame (pick_ray).
    Returns the mesh and the (colour, depth) frames."""
    xyz, rgb, indices = S.torus_mesh(96, 32, 0.3, 0.1)
    vertices = S.pack_vertices(xyz, rgb)
    flags = S.FLAG_DEPTH_TEST if depth_test else 0
    results = []
    with swr_amd.Context(0, device_count=device_count) as ctx:
        ctx.scene_upload(vertices, indices)
        ctx.scene_skin(*bend_skin(vertices))
        use_auto_normals(ctx, vertices, auto_normals)
        ctx.target_set(size, size)
        time = time0
        for k in range(frames):
            if dq:
                ctx.pose_set_dq(swr_amd.binding.dual_quats(twist_pose(time)))
            else:
                ctx.pose_set(bend_pose(time))
            ctx.draw(S.app_transform(time), flags)
            if pick:
                pick_ray(ctx, S.app_transform(time), size, pick, k)
            results.append((ctx.read_color(), ctx.read_depth()))
            if out:
                os.makedirs(out, exist_ok=True)
                write_ppm(os.path.join(out, f"frame_{k:04d}.ppm"), results[-1][0])
            time += 1.0 / 60.0
    return vertices, indices, results


def morph_targets(vertices: np.ndarray) -> np.ndarray:
    """(2, nv, 3) position deltas of any mesh: a swell away from the mesh's centre by a quarter of each vertex' distance, and a twist
    about z that grows with height."""
    p = vertices[:, 0:3].astype(np.float32)
    centre = ((p.min(axis=0) + p.max(axis=0)) * np.float32(0.5)).astype(np.float32)
    r = p - centre
    d = np.zeros((2, p.shape[0], 3), dtype=np.float32)
    d[0] = r * np.float32(0.25)
    extent = max(float(np.abs(r[:, 2]).max()), 1e-30)
    angle = (r[:, 2] / np.float32(extent)) * np.float32(0.8)
    c, s = np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)
    d[1, :, 0] = (c * r[:, 0] - s * r[:, 1]) - r[:, 0]
    d[1, :, 1] = (s * r[:, 0] + c * r[:, 1]) - r[:, 1]
    return d


def morph_weights(time: float) -> np.ndarray:
    """The two weights at `time`: the mesh breathes and twists back and forth (never exactly 0: both targets stay active)."""
    return np.array([0.5 + 0.45 * math.sin(4.0 * time), 0.05 + math.sin(2.5 * time)], dtype=np.float32)


def run_morph(frames: int, size: int, out: str | None = None, depth_test: bool = True, time0: float = 0.0, skin: bool = False,
              device_count: int = 1, obj: str | None = None, dq: bool = False, sparse: bool = False, auto_normals: str | None = None,
              pick=None):
    """The resident loop with a mesh that changes its shape: two morph targets uploaded once (swr_scene_morph), new weights every
    frame (swr_morph_set), the app's transform.  skin: the torus of run_skin, morphed and then posed (swr_pose_set, or with dq
    swr_pose_set_dq and twist_pose) every frame.  sparse: the targets are uploaded as sparse ones, restricted to the vertices they
    move (swr_scene_morph_sparse), and with skin the weights and the pose are set by one call (swr_morph_pose_set).
    auto_normals ("smooth" / "flat"): lit by a Phong material with normals recomputed on the device after every change of shape
    (swr_scene_normals): the targets carry no normal deltas.  pick (x, y): the triangle and the point of the deformed mesh on that
    pixel's ray, every frame (pick_ray).  Returns the mesh and the (colour, depth) frames."""
    if skin:
        xyz, rgb, indices = S.torus_mesh(96, 32, 0.3, 0.1)
        vertices = S.pack_vertices(xyz, rgb)
    else:
        vertices, indices = load_mesh(obj) if obj else sphere_mesh()
    flags = S.FLAG_DEPTH_TEST if depth_test else 0
    results = []
    with swr_amd.Context(0, device_count=device_count) as ctx:
        ctx.scene_upload(vertices, indices)
        if sparse:
            ctx.scene_morph_sparse(swr_amd.binding.sparse_targets(morph_targets(vertices)))
        else:
            ctx.scene_morph(morph_targets(vertices))
        if skin:
            ctx.scene_skin(*bend_skin(vertices))
        use_auto_normals(ctx, vertices, auto_normals)
        ctx.target_set(size, size)
        time = time0
        for k in range(frames):
            pose = None if not skin else swr_amd.binding.dual_quats(twist_pose(time)) if dq else bend_pose(time)
            if sparse and skin:
                ctx.morph_pose_set(morph_weights(time), pose, dq=dq)     # one rewrite of the scene for both
            else:
                ctx.morph_set(morph_weights(time))
                if skin and dq:
                    ctx.pose_set_dq(pose)
                elif skin:
                    ctx.pose_set(pose)
            ctx.draw(S.app_transform(time), flags)
            if pick:
                pick_ray(ctx, S.app_transform(time), size, pick, k)
            results.append((ctx.read_color(), ctx.read_depth()))
            if out:
                os.makedirs(out, exist_ok=True)
                write_ppm(os.path.join(out, f"frame_{k:04d}.ppm"), results[-1][0])
            time += 1.0 / 60.0
    return vertices, indices, results


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)    # the app renders 512x512 (App.swift:52-53)
    ap.add_argument("--out", default=None)
    ap.add_argument("--obj", default=None, help="Wavefront OBJ mesh")
    ap.add_argument("--ply", default=None, help="Stanford PLY mesh (ascii or binary little endian)")
    ap.add_argument("--depth-test", action="store_true")
    ap.add_argument("--stream", action="store_true", help="asynchronous presents into two page-locked image sets")
    ap.add_argument("--gpus", type=int, default=1, help="bands / GPUs of the one context (with --stream)")
    ap.add_argument("--objects", type=int, default=1, help="copies of the mesh, each with its own matrix: one draw list per frame")
    ap.add_argument("--pick", default=None,
                    help="X,Y: print the copy and the triangle under that pixel every frame (primitive IDs); with --skin / --morph: the "
                         "triangle, t and the hit point of that pixel's ray on the deformed mesh (swr_cast_rays)")
    ap.add_argument("--lit", action="store_true",
                    help="with --pick X,Y: pick through rays as well — with --objects N through each copy's own range of triangles and "
                         "transform, reporting the nearest copy — and cast one occlusion ray from the picked point towards the light: "
                         "lit or shadowed (swr_query_rays)")
    ap.add_argument("--ids", action="store_true",
                    help="write the ID image and print the last frame's visibility counts: visible triangles, pixels per copy (swr_count_ids)")
    ap.add_argument("--occlusion", action="store_true",
                    help="with --objects N: test every copy's screen rectangle and nearest depth against the previous frame's depth "
                         "image on the device and print how many copies could be skipped (swr_query_depth)")
    ap.add_argument("--bounds", action="store_true",
                    help="with --occlusion: the copies' rectangles and nearest depths come from the device (swr_item_bounds), which "
                         "also allows --skin and --morph")
    ap.add_argument("--delta", action="store_true",
                    help="the host-visible loop through swr_render_delta: only the tiles that changed cross to the host; prints them per frame")
    ap.add_argument("--skin", action="store_true",
                    help="a torus bending between two joints: skinned once (swr_scene_skin), a new pose every frame (swr_pose_set)")
    ap.add_argument("--dq", action="store_true",
                    help="with --skin: the torus also twists, and the pose is set as dual quaternions (swr_pose_set_dq): the twist keeps "
                         "its volume where blended matrices would pinch it")
    ap.add_argument("--morph", action="store_true",
                    help="two procedural morph targets on the mesh (swr_scene_morph), new weights every frame (swr_morph_set); composes with --skin")
    ap.add_argument("--sparse", action="store_true",
                    help="with --morph: the targets list only the vertices they move (swr_scene_morph_sparse); with --skin as well, weights "
                         "and pose are set by one call (swr_morph_pose_set)")
    ap.add_argument("--auto-normals", choices=["smooth", "flat"], default=None,
                    help="with --skin and / or --morph: a Phong material whose normals are computed on the device from the deformed "
                         "positions, per vertex or per triangle (swr_scene_normals)")
    ap.add_argument("--cull", choices=["none", "back", "front"], default="none", help="face culling: which facing is not drawn")
    ap.add_argument("--front-ccw", action="store_true", help="front = counter-clockwise as displayed (default: clockwise)")
    ap.add_argument("--clip", action="store_true", help="depth clipping: triangles clipped against the near and far planes")
    ap.add_argument("--perspective", action="store_true", help="perspective-correct interpolation of colour and varyings")
    ap.add_argument("--glass", type=int, default=None, metavar="A",
                    help="draw a second instance over the mesh as a blend load frame with opacity A (0..255): alpha blending")
    ap.add_argument("--ssaa", type=int, choices=[1, 2, 4], default=1,
                    help="supersampling: draw at S x size and resolve S x S samples per pixel on the device")
    a = ap.parse_args()
    if a.dq and not a.skin:
        ap.error("--dq is a mode of --skin")
    if a.lit and (not a.pick or a.stream or a.delta or ((a.skin or a.morph) and not (a.occlusion and a.bounds))):
        ap.error("--lit needs --pick X,Y and is part of the plain loop (with or without --objects N)")
    if a.sparse and not a.morph:
        ap.error("--sparse is a mode of --morph")
    if a.ssaa != 1 and a.stream:
        ap.error("--ssaa is not part of the --stream loop (there is no asynchronous resolved present)")
    if a.glass is not None:
        if not 0 <= a.glass <= 255:
            ap.error("--glass: the opacity is 0..255")
        if a.pick or a.ids or a.perspective:
            ap.error("--glass does not combine with --pick, --ids or --perspective (blend frames write no IDs and interpolate screen-linearly)")
        if a.stream:
            ap.error("--glass is not part of the --stream loop")
    if a.bounds and not (a.occlusion and a.objects > 1):
        ap.error("--bounds needs --occlusion and --objects N")
    if a.bounds and a.clip:
        ap.error("--bounds does not combine with --clip (swr_item_bounds does not take SWR_FLAG_DEPTH_CLIP)")
    deforming_bounds = a.occlusion and a.bounds and (a.skin or a.morph)
    if a.auto_normals and (deforming_bounds or not (a.skin or a.morph)):
        ap.error("--auto-normals is a mode of the --skin and --morph loops")
    if a.sparse and deforming_bounds:
        ap.error("--sparse is part of the plain --morph loop, not of --occlusion --bounds")
    if deforming_bounds and (a.obj or a.ply or a.stream or a.delta or a.glass is not None):
        ap.error("--occlusion --bounds with --skin / --morph draws copies of the torus: not with --obj, --ply, --stream, --delta or --glass")
    if a.morph and not deforming_bounds:
        if a.stream or a.delta or a.ssaa != 1 or a.glass is not None or a.objects > 1 or a.ids or a.occlusion or (a.skin and (a.obj or a.ply)):
            ap.error("--morph is its own loop: only --frames, --size, --out, --depth-test, --gpus, --pick, --skin and (without --skin) --obj / --ply apply")
        _, idx, res = run_morph(a.frames, a.size, a.out, a.depth_test, skin=a.skin, device_count=a.gpus, obj=a.ply or a.obj, dq=a.dq, sparse=a.sparse,
                              auto_normals=a.auto_normals, pick=tuple(int(t) for t in a.pick.split(",")) if a.pick else None)
        print(f"{a.frames} morphed{' and posed' if a.skin else ''} frames, {idx.size // 3} triangles, "
              f"coverage per frame: {[round(float((c[..., 3] == 255).mean()), 4) for c, _ in res]}")
        sys.exit(0)
    if a.skin and not deforming_bounds:
        if a.stream or a.delta or a.ssaa != 1 or a.glass is not None or a.objects > 1 or a.ids or a.occlusion or a.obj or a.ply:
            ap.error("--skin is its own loop over its own mesh: only --frames, --size, --out, --depth-test, --gpus and --pick apply")
        _, idx, res = run_skin(a.frames, a.size, a.out, a.depth_test, device_count=a.gpus, dq=a.dq, auto_normals=a.auto_normals,
                               pick=tuple(int(t) for t in a.pick.split(",")) if a.pick else None)
        print(f"{a.frames} posed frames, {idx.size // 3} triangles, coverage per frame: {[round(float((c[..., 3] == 255).mean()), 4) for c, _ in res]}")
        sys.exit(0)
    if a.delta:
        if a.stream or a.ssaa != 1 or a.glass is not None or a.objects > 1 or a.pick or a.ids or a.occlusion:
            ap.error("--delta is the plain swr_render loop: not with --stream, --ssaa, --glass, --objects, --pick, --ids or --occlusion")
        res, _ = run_delta(a.frames, a.size, a.ply or a.obj, a.depth_test, device_count=a.gpus, out=a.out)
        print(f"{a.frames} frames through delta reads, coverage per frame: {[round(float((c[..., 3] == 255).mean()), 4) for c, _ in res]}")
        sys.exit(0)
    if a.stream:
        res = run_streamed(a.frames, a.size, a.ply or a.obj, a.depth_test, device_count=a.gpus, cull=a.cull, front_ccw=a.front_ccw,
                           clip=a.clip, perspective=a.perspective)
        print(f"{a.frames} frames streamed, coverage per frame: {[round(float((c[..., 3] == 255).mean()), 4) for c, _ in res]}")
        sys.exit(0)
    pick = tuple(int(t) for t in a.pick.split(",")) if a.pick else None
    _, idx, res = run(a.frames, a.size, a.out, a.ply or a.obj, a.depth_test, objects=a.objects, pick=pick, cull=a.cull,
                      front_ccw=a.front_ccw, clip=a.clip, perspective=a.perspective, glass=a.glass, ssaa=a.ssaa, ids=a.ids,
                      occlusion=a.occlusion, bounds=a.bounds, skin=deforming_bounds and a.skin, morph=deforming_bounds and a.morph,
                      dq=a.dq, lit=a.lit)
    cov = [(c[..., 3] == 255).mean() for c, _, _ in res]
    print(f"{a.frames} frames, {max(1, a.objects)} x {idx.size // 3} triangles, coverage per frame: {[round(float(x), 4) for x in cov]}")
