/*
 * swr.h — C-ABI of the MI355X-native triangle rasterizer (drop-in boundary).
 *
 * This header is the whole boundary: plain pointers and sizes, no C++ / torch / HIP
 * types.  Every entry point names the reference interface (file:line relative to
 * zhvrnkov/software-renderer) that it stands in for.  The shared library that exports
 * these symbols is `software-renderer_amd/lib/libswr_hip.so` (built from
 * `software-renderer_amd/csrc/` with hipcc for gfx950).  There is no CPU fallback inside
 * the library: every entry point that computes needs a HIP device and returns
 * SWR_ERR_HIP (with a message in swr_last_error) when there is none.
 *
 * Semantics are those of the reference's CPU renderer (renderer/Renderer.swift:204-287,
 * 467-494, 88-100, 116-129, 159-171) — see DESIGN.md §2 for the normative restatement.
 */
#ifndef SWR_H_
#define SWR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWR_ABI_VERSION 6

/* ---- status codes (the reference has no error channel: it fatalError()s / try!s,
 *      Renderer.swift:26,209,239,497; GpuRenderer.swift:20-31,37-38) ------------------ */
enum {
    SWR_OK = 0,
    SWR_ERR_BAD_ARG = -1,       /* null pointer, non-positive size, bad band */
    SWR_ERR_INDEX_COUNT = -2,   /* index_count % verticesCount != 0   (assert, Renderer.swift:209) */
    SWR_ERR_INDEX_RANGE = -3,   /* an index outside [0, vertex_count)  (Swift array trap, Renderer.swift:226) */
    SWR_ERR_HIP = -4,           /* HIP runtime error / no device */
    SWR_ERR_UNSUPPORTED = -5,   /* unknown primitive type, too many primitives / vertices */
    SWR_ERR_NO_SCENE = -6,      /* swr_draw before swr_scene_upload / swr_target_set */
    SWR_ERR_NOMEM = -7,
    SWR_ERR_FRAME_DROPPED = -8  /* a frame that was copied to the host (swr_present) in an un-waited burst had overflowed
                                   the (triangle,tile) bins and was rastered empty; the bins have been grown, redraw it.
                                   (The last frame of a burst is always repaired silently; frames never presented are
                                   never reported: nobody could see them.) */
};

/* ---- PrimitiveType (Renderer.swift:174-189).  Only .triangle is on the hot path. ---- */
enum {
    SWR_PRIMITIVE_TRIANGLE = 0,
    SWR_PRIMITIVE_LINE = 1,      /* reference draw(line:) is an empty stub, Renderer.swift:289-293 */
    SWR_PRIMITIVE_VERTICES = 2   /* Renderer.swift:295-302: point plotting */
};

/* ---- draw flags --------------------------------------------------------------------- */
enum {
    /* 0 = the CPU renderer exactly as written: painter's order (highest primitive index
     * covering a pixel wins), depth image stays +inf (z-test commented out,
     * Renderer.swift:257-261). */
    SWR_FLAG_DEPTH_TEST = 1u << 0, /* restore Renderer.swift:257-261: depth = za*w0+zb*w1+zc*w2,
                                      strict '<', first-drawn wins ties (also :344-348,
                                      Shaders.metal:158-165) */
    SWR_FLAG_NO_COLOR   = 1u << 1, /* depth-only pass: the colour image is neither cleared nor
                                      written (BASELINE config 4) */
    SWR_FLAG_METAL_RULES = 1u << 2, /* the Metal path's rules instead of the CPU renderer's:
                                      vertices snapped with round() (Shaders.metal:71), one thread per ROI
                                      pixel with inside = all(0 <= ws <= 1) (:133-153), z-test always on
                                      (:158-161), bgra8Unorm store (round to nearest), ROIs whose min-x or
                                      min-y is 0 skipped (GpuRenderer.swift:122-124); IEEE arithmetic (the
                                      reference's MTL_FAST_MATH build is not bit-reproducible) */
    SWR_FLAG_REAL_LINES = 1u << 3, /* OPT-IN, .line primitives only.  Default (flag clear) = the reference as written:
                                      draw(line:colorBuffer:depthBuffer:) has an empty body (Renderer.swift:289-293), a
                                      .line pass only clears.  With the flag every 2-index primitive is drawn with the
                                      reference's own DDA (draw(line:with:in:), Renderer.swift:405-419) between its two
                                      transformed endpoints, truncated like .vertices does (:298-299): steps =
                                      max(|dx|, |dy|), float x / y advanced by dx/steps, dy/steps, pixel
                                      (Int(x.rounded()), Int(y.rounded())) for steps iterations (the end point itself is
                                      not plotted), in the colour of the FIRST vertex, later primitives overwrite
                                      earlier ones, no z-test, depth stays +inf.  Lines longer than 2^20 steps or with a
                                      non-finite endpoint are skipped (the reference would trap / never finish) */
    SWR_FLAG_LOAD = 1u << 4,       /* LOAD ACTION (ABI 6; Metal's MTLLoadActionLoad): the frame is Renderer.render(renderPass:) WITHOUT the
                                      clear of Renderer.swift:205-206 — the same loop continues from the image already there (see
                                      "Load frames" below) */
    SWR_FLAG_PRIMITIVE_IDS = 1u << 5, /* the frame also writes an ID image: which triangle is visible at every pixel (Metal: a second
                                      colour attachment written with [[primitive_id]]); read it with swr_read_ids (see "Primitive
                                      IDs" below) */
    SWR_FLAG_CULL_BACK = 1u << 6,  /* face culling (Metal's setCullMode(.back)): back-facing triangles are not drawn (see "Face culling") */
    SWR_FLAG_CULL_FRONT = 1u << 7, /* front-facing triangles are not drawn; with SWR_FLAG_CULL_BACK every triangle with a facing is dropped */
    SWR_FLAG_FRONT_CCW = 1u << 8,  /* front = counter-clockwise as displayed (Metal's setFrontFacingWinding(.counterClockwise));
                                      without it front = clockwise as displayed (MTLWindingClockwise, Metal's default) */
    SWR_FLAG_DEPTH_CLIP = 1u << 10, /* clip every triangle against the near (z >= 0) and far (z <= w) planes before the divide, like
                                      Metal's default MTLDepthClipMode.clip (see "Depth clipping") */
    SWR_FLAG_PERSPECTIVE = 1u << 11, /* interpolate colour and varyings with perspective correction, like Metal's [[center_perspective]]
                                      and GL's smooth (see "Perspective-correct interpolation") */
    SWR_FLAG_BLEND = 1u << 12      /* every fragment is blended into the pixel, in draw order, instead of replacing it (Metal's
                                      isBlendingEnabled; see "Alpha blending"); the state is set with swr_blend_set */
};

/* ---- Alpha blending (SWR_FLAG_BLEND, swr_blend_set) — DESIGN.md §18 ----------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6): the presence of the swr_blend_set symbol is the feature test; an older library refuses the
 * flag bit with SWR_ERR_BAD_ARG.  Without the bit nothing changes.  (Bit 9 stays unused and refused.)
 * The blend state (swr_blend, below) persists on the context like the material: it applies to every later frame drawn with the bit,
 * on every band or device, swr_render included; a frame uses the state that was set when it was posted.
 *
 * Fragments and order.  A blend frame is Renderer.render(renderPass:) with one change: a fragment does not replace the pixel, it is
 * blended into it.
 *   Fragments: exactly those the same frame without the bit would generate — coverage of the active rule set (CPU scanline spans, or
 *     the Metal inside test), after face culling and depth clipping, the same skipped triangles.
 *   Order: fragments are taken per pixel in primitive order — index order, or for a draw list the order number (item order first);
 *     depth-clip fan triangles in fan order, in their original's place.
 *   Starting image: under SWR_FLAG_LOAD the image already there, exactly as for load frames ("Load frames" below); without it the
 *     cleared image, colour (0,0,0,0), depth +inf.
 * Depth.  The depth image is never written: after the frame it equals the starting depth image bit for bit, NaNs, -0 and +inf
 *   included.  With SWR_FLAG_DEPTH_TEST (always under SWR_FLAG_METAL_RULES) a fragment contributes iff d < depth[x,y] of the STARTING
 *   image, d the rule set's own depth expression; a NaN or +inf d never passes.  Without the z-test every fragment contributes.
 *   This is the standard transparent pass: test against the opaque scene, write no depth.
 * Arithmetic.  All integer and exact: no float blend, nothing drifts, opacity 0 and 255 are identities.
 *   Source bytes (sb, sg, sr) of a fragment: the bytes the frame without the bit would store for it if it won the pixel — same
 *     interpolation, clamp and quantiser as the rule set (trunc under the CPU rules, rint under the Metal rules); sa = 255.
 *   SWR_BLEND_OVER, A = opacity, d the pixel's current byte, per channel b, g, r, a:  d' = (s*A + d*(255 - A) + 127) / 255
 *     (integer division).
 *   SWR_BLEND_ADD:  d' = min(255, d + (s*A + 127) / 255).
 * Combinations.
 *   SWR_FLAG_NO_COLOR with the bit: SWR_ERR_BAD_ARG.
 *   SWR_FLAG_PRIMITIVE_IDS, SWR_FLAG_PERSPECTIVE, or a material whose shader is not SWR_SHADER_PASSTHROUGH: SWR_ERR_UNSUPPORTED.
 *   .vertices and .line frames accept the bit and ignore it, like the cull and clip bits.
 *   Cull, clip, load, depth test, Metal rules, draw lists (swr_draw_list), multi-band contexts and swr_render all combine with it.
 * Properties that follow.
 *   (a) OVER with opacity 255 and no z-test: the colour image is bit for bit that of the same frame without the bit (painter's order).
 *   (b) Opacity 0: the colour image equals the starting colour image.
 *   (c) A blend draw list is bit for bit the chain of its one-item blend frames, the first with the list's own load or clear start
 *       and the rest SWR_FLAG_LOAD — with the z-test too, because depth never changes.
 * Bin overflow: the load-frame rules apply unchanged.  An overflowed blend frame is rastered as "no triangles", so it shows the
 *   starting image; it is redrawn from the same starting image, or reported with SWR_ERR_FRAME_DROPPED. */
enum { SWR_BLEND_OVER = 0, SWR_BLEND_ADD = 1 };
typedef struct swr_blend {
    int32_t mode;        /* SWR_BLEND_* */
    int32_t opacity;     /* 0..255 */
    int32_t reserved[2]; /* 0 */
} swr_blend;             /* 16 bytes */

/* ---- Supersampled resolve (swr_read_color_resolved, swr_read_depth_resolved, swr_render_resolved) — DESIGN.md §19 ------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the three symbols is the feature test.  Nothing existing
 * changes.  Supersampling is Metal's storeAction = .multisampleResolve with sample-rate shading: the frame is drawn at S*w x S*h with
 * the same transform — every rule set, flag, blend frame, band and draw list as it is — and an S x S box filter, on the device,
 * brings it down to w x h.  Only the small image crosses to the host.
 *
 * W x H is the target set by swr_target_set; w = W / S, h = H / S (swr_resolve.factor = S).
 *   Colour.  For output pixel (x, y) and each channel c of b, g, r, a:
 *       out = (Σ_{j<S} Σ_{i<S} src[S·y+j][S·x+i][c] + S·S/2) / (S·S), integer division.
 *     Nothing is gamma-corrected.  A cleared pixel is (0,0,0,0) and a covered one has a = 255, so the resolved alpha is the coverage
 *     of the pixel (255 = every sample covered), usable for compositing the anti-aliased image over a background.
 *   Depth, SWR_RESOLVE_DEPTH_SAMPLE0.  The bits of src[S·y][S·x].
 *   Depth, SWR_RESOLVE_DEPTH_MIN.  Take m = sample (0,0), then the other samples in row-major order (j outer, i inner):
 *       if (s < m || (m != m && s == s)) m = s
 *     The result is the bits of m.  NaNs lose to any number; if all samples are NaN the first one's bits are kept, payload included;
 *     of equal zeros the first met is kept, so -0 and +0 survive as they are; +inf (the cleared depth) and denormals compare exactly.
 *   factor == 1.  The destination is byte for byte what swr_read_color / swr_read_depth deliver.
 *   Completion.  The calls complete everything first, like swr_read_*: an overflowed last frame is repaired before it is resolved, and
 *     the image resolved is that of the last frame.  The full-size images on the device are not modified: a following SWR_FLAG_LOAD
 *     frame, swr_read_color, swr_read_depth and swr_read_ids see them unchanged.  After a SWR_FLAG_NO_COLOR frame the resolved colour is
 *     as unspecified as swr_read_color's.
 *   Bands.  Each band resolves its own rows [row_begin, row_end) into rows [row_begin/S, row_end/S) of the caller's w x h image; rows
 *     outside the band(s) are left untouched.  row_begin is a multiple of the tile height (32) and row_end is either a multiple of 32
 *     or equal to H, so with H a multiple of S no sample block straddles two bands.  Multi-device contexts fan out like swr_read_*.
 *   Errors.  SWR_ERR_BAD_ARG: a NULL argument, a factor outside {1, 2, 4}, an unknown filter, a non-zero reserved word, or W or H not
 *     a multiple of S (or a band whose row_end is neither);  SWR_ERR_NO_SCENE: no target;  a failed context returns its sticky error,
 *     as elsewhere.
 * swr_render_resolved(ctx, pass, resolve) is swr_render with pass->width, pass->height, pass->color and pass->depth describing the
 *   DESTINATION, w x h: the frame is drawn at S·w x S·h with the pass's transform and flags, then resolved into the caller's images.
 *   scene_id caching works as in swr_render; swr_render_times.gather_ms covers the resolve plus the copy; frames is 2 after a
 *   repaired overflow.  SWR_FLAG_LOAD: SWR_ERR_UNSUPPORTED (the starting image would be at the wrong resolution).  SWR_FLAG_NO_COLOR:
 *   the colour is not resolved, and color may be NULL.  .vertices and .line passes resolve like any other.  With
 *   SWR_FLAG_PRIMITIVE_IDS the ID image stays at sample resolution: swr_read_ids delivers S·w x S·h words (IDs are not resolved). */
enum { SWR_RESOLVE_DEPTH_SAMPLE0 = 0, SWR_RESOLVE_DEPTH_MIN = 1 };
typedef struct swr_resolve {
    int32_t factor;        /* S: 1, 2 or 4 samples per axis */
    int32_t depth_filter;  /* SWR_RESOLVE_DEPTH_* (ignored by swr_read_color_resolved, but checked) */
    int32_t reserved[2];   /* 0 */
} swr_resolve;             /* 16 bytes */

/* ---- Face culling (SWR_FLAG_CULL_BACK / _CULL_FRONT / _FRONT_CCW) — DESIGN.md §14 ------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6): a library that accepts the bits has the feature; an older one refuses them with
 * SWR_ERR_BAD_ARG.
 *   Facing comes from the integer vertices the triangle is rasterised with — the truncated screen coordinates, or under
 *     SWR_FLAG_METAL_RULES the rounded-then-truncated ones — a, b, c in index order, pixel coordinates (x right, y down, row 0 at
 *     the top): A = (bx - ax) * (cy - ay) - (cx - ax) * (by - ay), exact.  A > 0: clockwise as displayed; A < 0: counter-clockwise.
 *     Example: NDC (-0.5,-0.5), (0.5,-0.5), (0,0.5) (counter-clockwise with y up) maps to pixels (W/4, 3H/4), (3W/4, 3H/4), (W/2, H/4):
 *     A = -W*H/4 < 0, counter-clockwise as displayed (the y flip of the screen map keeps the visual orientation).
 *   Front-facing: A > 0, or A < 0 with SWR_FLAG_FRONT_CCW; back-facing: the other sign.  A == 0 has no facing and is never culled
 *     (under the CPU rules such triangles draw as before; the Metal rules skip them anyway).  Triangles setup already skips stay
 *     skipped.
 *   Every triangle entry point: swr_draw, swr_draw_primitives(SWR_PRIMITIVE_TRIANGLE), swr_draw_list (each item's facing from its
 *     own transform: a mirroring matrix flips the winding, uncompensated, as in Metal and GL), swr_render.  .vertices and .line
 *     frames accept the bits and ignore them.
 *   A culled frame is bit for bit the frame without the bits of the same scene with the culled triangles removed from the index
 *     list, order kept — colour, depth and IDs, which keep the original numbering (triangle index p, draw-list order number).
 *   swr_timings.triangles still counts submitted triangles; tile_pairs only the pairs binned. */

/* ---- Depth clipping (SWR_FLAG_DEPTH_CLIP) — DESIGN.md §15 --------------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6): a library that accepts the bit has the feature; an older one refuses it with
 * SWR_ERR_BAD_ARG.  Without the bit nothing changes: every vertex goes from clip space straight to xyz / w.  (Bit 9 stays unused:
 * it is the bit earlier releases are tested to refuse as unknown.)
 *   Clip-space vertices r = (x, y, z, w): vertex_shader as setup computes it (draw lists: each item's own transform).
 *   Inside the near plane iff d_near = z >= 0, inside the far plane iff d_far = w - z >= 0 (binary32).  A triangle with a
 *     non-finite clip-space component is dropped (a documented deviation, like DESIGN.md §2.6).
 *   A triangle with all three vertices inside both planes is drawn exactly as without the bit.  Any other triangle is clipped
 *     against the near plane, then the far plane, each pass Sutherland-Hodgman over the edges (P_i, P_i+1) in vertex order,
 *     cyclic: P_i is emitted iff d(P_i) >= 0; an edge with one endpoint at d > 0 and the other at d < 0 adds the intersection,
 *     computed from the inside endpoint I towards the outside one O: t = d_I / (d_I - d_O), every carried component
 *     c = c_I + t * (c_O - c_I), one rounding per operation, no FMA.  A vertex at d == 0 is inside and never duplicated.
 *     Carried: x, y, z, w, the colour and (the extended fragment stage) normal and uv.  A polygon of fewer than 3 vertices is
 *     dropped.
 *   The polygon P_0 .. P_n-1 (n <= 5) becomes the fan (P_0, P_k, P_k+1), k = 1 .. n-2, in that order (winding kept).  Each
 *     sub-triangle is then a triangle of the scene in every respect (divide, screen map, truncation or the Metal snap, facing and
 *     culling, raster, z-test, fragment_shader); it takes the original triangle's place in the draw order, in fan order (painter's
 *     order: the later sub-triangle wins; the z-test: the earlier one wins an exact tie).
 *   IDs (SWR_FLAG_PRIMITIVE_IDS): every sub-triangle reports the original number (triangle index p, or draw-list order number).
 *   Restated: a clip frame is bit for bit the frame without the bit of the scene in which every triangle is replaced by its fan,
 *     every fan vertex given in NDC (x/w, y/w, z/w) with its interpolated colour and attributes, drawn with the identity transform
 *     and the same other flags — IDs mapped back to the original numbering.  The identity turns an NDC coordinate of -0 into +0:
 *     a clip-space z of exactly -0 is drawn with depth +0 under the bit.
 *   swr_draw, swr_draw_primitives(SWR_PRIMITIVE_TRIANGLE), swr_draw_list, swr_render.  .vertices and .line frames accept the bit
 *     and ignore it.  swr_timings.triangles counts submitted triangles; tile_pairs the pairs binned, fan triangles included.
 *   A frame with the bit may have at most SWR_DEPTH_CLIP_MAX_TRIANGLES submitted triangles (more: SWR_ERR_UNSUPPORTED). */
#define SWR_DEPTH_CLIP_MAX_TRIANGLES (1 << 24)

/* ---- Perspective-correct interpolation (SWR_FLAG_PERSPECTIVE) — DESIGN.md §16 ----------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6): a library that accepts the bit has the feature; an older one refuses it with
 * SWR_ERR_BAD_ARG.  Without the bit nothing changes.  With it only the weights colour and the varyings (the extended stage's normal
 * and uv) are interpolated with change: coverage, depth, the z-test, tie rules and IDs are bit for bit those of the frame without it.
 *   For a triangle with corners a, b, c in index order, rw_a, rw_b, rw_c is the clip-space w of each corner, as vertex_shader computes
 *     it in setup: the frame's transform (swr_draw, swr_draw_primitives(SWR_PRIMITIVE_TRIANGLE), swr_render); the item's own
 *     (swr_draw_list); under SWR_FLAG_DEPTH_CLIP the clipper's w of the fan vertex (an original vertex keeps its own, an intersection
 *     gets w_I + t * (w_O - w_I)).
 *   rw_a == rw_b == rw_c (float ==): the screen weights unchanged — the frame is bit for bit the frame without the bit.  This holds for
 *     every affine transform (w is exactly 1).
 *   Otherwise, once per triangle q_k = 1 / rw_k; per pixel, with the rule set's own screen weights (w0, w1, w2) (the
 *     divider formula under SWR_FLAG_METAL_RULES): u0 = w0 * q_a, u1 = w1 * q_b, u2 = w2 * q_c, s = (u0 + u1) + u2, rs = 1 / s,
 *     p0 = u0 * rs, p1 = u1 * rs, p2 = u2 * rs — IEEE binary32, one rounding per operation, no FMA, both divisions correctly
 *     rounded.  Colour, normal and uv are interpolated with (p0, p1, p2) in each rule set's expression order; the depth stays
 *     za*w0 + zb*w1 + zc*w2 (screen-linear, as in Metal and GL).
 *   No special cases: negative w, s == 0 and NaN weights follow IEEE arithmetic (the colour clamp maps NaN to 0); a corner with
 *     rw == 0 has non-finite screen coordinates and its triangle is skipped.
 *   SWR_FLAG_NO_COLOR, .vertices and .line frames accept the bit; it has no effect on them.  It combines with every other flag,
 *     multi-band contexts, draw lists and swr_render. */

/* ---- Primitive IDs (SWR_FLAG_PRIMITIVE_IDS) — DESIGN.md §13 --------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6): the presence of the swr_read_ids symbol is the feature test.
 * A frame drawn with the flag also writes one uint32_t per pixel, band-local and laid out like the depth image.
 *   The ID of a pixel is the order number of the primitive whose fragment the frame keeps there — the winner whose colour and depth
 *     the frame stores, under painter's order, the z-test and the Metal rules alike, with every fragment shader:
 *     swr_draw, swr_draw_primitives(SWR_PRIMITIVE_TRIANGLE), swr_render: the triangle index p (indices[3p .. 3p+2]);
 *     swr_draw_list: the triangle's position in the concatenation of the items — item k's j-th triangle is vbase_k + j, vbase_k the
 *       sum of index_count / 3 of the items before it.
 *   SWR_ID_NONE marks a pixel where the frame keeps no fragment: nothing covers it, its only fragments have a NaN or +inf depth
 *     under the z-test, or (SWR_FLAG_LOAD) the loaded image wins there.  IDs never come from earlier frames.
 *   Triangles only: .vertices and .line frames with the flag fail with SWR_ERR_UNSUPPORTED.
 *   The colour and depth images of a frame are bit for bit the same with and without the flag.
 * swr_read_ids(ctx, dst): like swr_read_depth — completes everything, then copies rows [row_begin, row_end) of each band into the
 *   caller's full-size image (width * height words).  SWR_ERR_BAD_ARG when the last frame was drawn without the flag, or when
 *   swr_target_set, swr_target_write or swr_scene_upload has been called since (the IDs number the primitives of the scene the frame
 *   was drawn from: after a new upload, of whatever size, they name nothing, and swr_count_ids would have no n that fits them; the
 *   colour and depth images stay).  An overflowed last frame is redrawn with its flags, IDs included. */
#define SWR_ID_NONE 0xFFFFFFFFu

/* ---- Visibility counts (swr_count_ids) — DESIGN.md §20 ---------------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_count_ids symbol is the feature test.  Nothing
 * existing changes.  The questions asked of an ID image are mostly reductions — which draws are visible at all and how many pixels
 * does each cover (Metal's visibilityResultMode = .counting), which triangles lie under a selection rectangle or under one pixel.
 * swr_count_ids answers them on the device, band by band; only the counts cross to the host.
 *
 * Let ids be exactly the W x H image swr_read_ids would deliver now, and R the half-open rectangle [x0, x1) x [y0, y1) of the query,
 * in pixels of the full target (0 <= x0 <= x1 <= W, 0 <= y0 <= y1 <= H; an empty rectangle is legal and gives zeros; 1 x 1 is picking).
 *   SWR_COUNT_PER_PRIMITIVE: counts[p] = the number of pixels of R with ids == p.  n must equal the last frame's primitive count:
 *     index_count / 3 of the uploaded scene (swr_draw, swr_draw_primitives, swr_render), or for swr_draw_list the total over the items.
 *     Culled triangles and depth-clip fans keep the original numbering, as in the ID image.
 *   SWR_COUNT_PER_ITEM: counts[k] = the number of pixels of R whose ID lies in [vbase_k, vbase_k + index_count_k / 3), vbase_k as
 *     under "Primitive IDs".  n must equal the last draw list's item_count; a frame that was not a draw list counts as a list of one
 *     item (n == 1).  An empty item counts 0.  item_count == 0 means n == 0, and counts may then be NULL.
 *   *none = the number of pixels of R equal to SWR_ID_NONE; none may be NULL.
 *   Always: counts[0] + ... + counts[n-1] + *none == (x1 - x0) * (y1 - y0).  Every element of counts[0 .. n) is written, zeros
 *     included.  Counts fit 32 bits (a target is at most 65535 x 65535).  All arithmetic is integer: the result is exact.
 *   Completion.  The call completes everything first, like swr_read_ids: an overflowed last frame is redrawn, IDs included, before it
 *     is counted.  The ID, colour and depth images on the device are not modified: a following swr_read_ids, SWR_FLAG_LOAD frame or
 *     second swr_count_ids sees them unchanged.
 *   Bands.  Each band counts the part of R that falls into its rows [row_begin, row_end); the library adds the bands' counts before
 *     it returns (a multi-device context: one array for the caller, written once, after every band succeeded).  A context that owns
 *     only a band of the target (swr_target_set with row_begin / row_end) counts the part of R in its rows; R itself is still checked
 *     against the full W x H.
 *   After swr_render (or swr_render_resolved) with SWR_FLAG_PRIMITIVE_IDS the rectangle is in pixels of the target that call set —
 *     sample resolution, S*w x S*h, after a resolved render.
 *   Errors.  SWR_ERR_BAD_ARG: a NULL ctx or q; a NULL counts with n > 0; an unknown group; a non-zero reserved word; a rectangle
 *     outside the target or inverted; an n that is not the required value (the message names it); the conditions under which
 *     swr_read_ids refuses (the last frame was drawn without SWR_FLAG_PRIMITIVE_IDS, or swr_target_set / swr_target_write /
 *     swr_scene_upload came after it).  SWR_ERR_NO_SCENE: no target.  A failed context returns its sticky error.  After an error nothing was written. */
enum { SWR_COUNT_PER_PRIMITIVE = 0, SWR_COUNT_PER_ITEM = 1 };
typedef struct swr_id_count {
    int32_t group;          /* SWR_COUNT_* */
    int32_t x0, y0, x1, y1; /* half-open rectangle [x0,x1) x [y0,y1), in pixels of the full W x H target */
    int32_t reserved[3];    /* 0 */
} swr_id_count;             /* 32 bytes */

/* ---- Depth queries (swr_query_depth) — DESIGN.md §21 -----------------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_query_depth symbol is the feature test.  Nothing
 * existing changes.  swr_count_ids tells which objects that were drawn are visible; swr_query_depth tells whether an object that was
 * not drawn, or is about to be, could be visible at all behind what the depth image already holds — the occlusion query of the
 * hardware APIs (a bounding box drawn with colour and depth writes off, the passing fragments counted), without the 33 MB depth image
 * of a 4K frame crossing to the host.  The caller supplies every object's screen rectangle and its nearest depth.
 *
 * Let depth be exactly the W x H image swr_read_depth would deliver now.  passed[k] = the number of pixels (x, y) of box k,
 * x0 <= x < x1 and y0 <= y < y1, with boxes[k].z < depth[y][x], compared as binary32 '<': the pixels where a fragment of depth z
 * would pass the strict z-test of SWR_FLAG_DEPTH_TEST.  What that rule fixes:
 *     a stored NaN is never passed; a NaN z passes nowhere; z == depth does not pass; -0 and +0 are equal; +inf, the cleared depth,
 *     is passed by every finite z and by -inf; a stored -inf is never passed; denormals compare exactly (nothing is flushed).
 *   Boxes.  0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H, in pixels of the full target; an empty rectangle is legal and gives 0.
 *     Boxes may overlap and repeat.  n == 0 is legal, and boxes and passed may then be NULL.  Every element of passed[0 .. n) is
 *     written.  At most SWR_DEPTH_QUERY_MAX boxes per call.
 *   Exactness.  The counts are integers and exact: they do not depend on how the device gets there (it keeps a minimum, a maximum
 *     and a NaN count per tile and reads only the pixels of tiles that straddle z).
 *   The depth image.  No SWR_FLAG_PRIMITIVE_IDS is needed: the depth image exists after every frame — +inf after a painter's-order
 *     frame, the starting depth after a blend frame, the written image after swr_target_write, the cleared image right after
 *     swr_target_set (every pixel +inf, whatever the buffers held before: that answer needs no device).  The call is legal in all
 *     of these.
 *   After swr_render (or swr_render_resolved) the rectangles are in pixels of the target that call set — sample resolution,
 *     S*w x S*h, after a resolved render.
 *   Completion.  The call completes everything first, like swr_read_depth: an overflowed last frame is repaired before it is tested.
 *     No image on the device is modified.
 *   Bands.  Each band counts the part of every box in its rows [row_begin, row_end); the library adds the bands and writes the
 *     caller's array once, after every band succeeded.  A context that owns only a band of the target (swr_target_set with
 *     row_begin / row_end) counts the part of every box in its rows; the boxes are still checked against the full W x H.
 *   Errors.  SWR_ERR_BAD_ARG: a NULL ctx; NULL boxes or passed with n > 0; n < 0; a non-zero reserved word; a rectangle inverted or
 *     outside the target (the message names the first offending box index).  SWR_ERR_UNSUPPORTED: n > SWR_DEPTH_QUERY_MAX.
 *     SWR_ERR_NO_SCENE: no target.  A failed context returns its sticky error.  After an error nothing was written. */
typedef struct swr_depth_box {
    int32_t x0, y0, x1, y1;   /* half-open rectangle [x0,x1) x [y0,y1), pixels of the full W x H target */
    float   z;                /* the depth the box is tested with (its nearest depth, chosen by the caller) */
    int32_t reserved[3];      /* 0 */
} swr_depth_box;              /* 32 bytes */
#define SWR_DEPTH_QUERY_MAX (1 << 16)

/* ---- Delta reads (swr_read_color_delta, swr_read_depth_delta, swr_render_delta) — DESIGN.md §22 -----------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_read_color_delta symbol is the feature test.  Nothing
 * existing changes.  A frame costs little on the device; what a caller waits for is the copy of two full images that mostly hold what
 * they held a frame ago.  A delta read compares the image with what the host already holds, tile by tile, on the device, and only
 * the changed part crosses.  Everything below is integer and exact.
 *   Tiles.  A tile is swr_tile_cols() x swr_tile_rows() pixels (64 x 32), anchored at pixel (0, 0) of the full target.  Bands start
 *     at multiples of 32 rows, so a band's tiles are tiles of the target.  The right and bottom tiles may be partial.
 *   Baseline.  Every band keeps one baseline image on the device per image kind (colour, depth): the image the last delta read of
 *     that kind delivered.  Baselines are allocated on first use.
 *   The caller's promise.  The band's rows of dst still hold what the previous delta read of that kind delivered.  The pointer may
 *     differ from call to call; the content may not.
 *   No baseline.  The band is delivered whole, exactly as swr_read_color / swr_read_depth deliver it: full = 1, and every tile counts
 *     as changed.
 *   With a baseline.  A tile is changed iff any of its 32-bit words differs from the baseline, compared as bits: a NaN with another
 *     payload, and -0 against +0, are therefore changes; equal NaN bits are not.  tiles_changed is the exact number of changed tiles.
 *     Let R be the bounding box of the band's changed tiles, clipped to the band and the width.  dst is written only inside R (a
 *     multi-device context: only inside each band's own R); nothing outside is touched.  An implementation may write less than R,
 *     but never a pixel of an unchanged tile outside R; bytes_copied says what it did.
 *   After the call.  Under the promise, the band's rows of dst are byte for byte what swr_read_color / swr_read_depth would deliver
 *     now, and the baseline is that image.
 *   Completion.  As swr_read_*: everything is completed first, an overflowed last frame is repaired, and no framebuffer image is
 *     modified.  After a SWR_FLAG_NO_COLOR frame the colour is as unspecified as swr_read_color's, but the baseline still tracks what
 *     was delivered.
 *   What drops a baseline.  swr_delta_reset; a swr_target_set that changes the width, the height or the rows; destroying the
 *     context.  The same target again keeps it (swr_render sets its target every frame).
 *   What keeps a baseline.  Frames, swr_target_write, swr_present, the other reads and the queries: none of them changes what the
 *     host holds.
 *   Bands.  Every band handles its own rows; the stats are summed and the rectangle is the bounding box of the bands' rectangles.  A
 *     context that owns rows [a, b) of a larger target handles only those rows.  A group writes stats once, after every band succeeded.
 *   swr_render_delta is swr_render whose gather is the two delta reads (the colour's is skipped under SWR_FLAG_NO_COLOR, and stats[0]
 *     is then all 0): pass->color and pass->depth carry the promise, swr_render_times.gather_ms covers the delta, scene_id caching
 *     works as in swr_render.  SWR_FLAG_LOAD returns SWR_ERR_UNSUPPORTED: its starting image is uploaded whole anyway.
 *   Errors.  SWR_ERR_BAD_ARG: a NULL ctx or dst; zero or unknown swr_delta_reset bits.  SWR_ERR_NO_SCENE: no target.  A failed context
 *     returns its sticky error.  After an error dst, stats and the baselines are untouched.
 *   Not covered: the ID image, an asynchronous present, and the C++ and Swift mirrors. */
typedef struct swr_delta_stats {
    int32_t x0, y0, x1, y1;   /* bounding box of everything written to dst, pixels of the full target; all 0 when nothing was */
    int64_t tiles;            /* tiles in the context's band(s) */
    int64_t tiles_changed;    /* tiles that differed from the baseline (== tiles on a full delivery) */
    int64_t bytes_copied;     /* bytes written to dst */
    int32_t full;             /* 1: there was no baseline, the whole band was delivered */
    int32_t reserved;         /* 0 on return */
} swr_delta_stats;            /* 48 bytes */
enum { SWR_DELTA_COLOR = 1, SWR_DELTA_DEPTH = 2 };

/* ---- Skinned meshes (swr_scene_skin, swr_pose_set) — DESIGN.md §23 ---------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_pose_set symbol is the feature test.  Nothing
 * existing changes.  The resident scene can deform without a new swr_scene_upload: every vertex carries four joint influences, and
 * swr_pose_set rewrites the positions (and normals) of the resident triangle stream on the device from a table of joint matrices.
 *   swr_scene_skin follows the swr_scene_upload it belongs to, like swr_scene_attributes, before or after it: vertex_count must
 *     match, and a new swr_scene_upload (the one a swr_render performs included) discards skin and pose.  skin == NULL with vertex_count == 0
 *     removes the skin and restores the bind pose.  A new skin restores the bind pose too.  The largest joint index is found once, here.
 *   swr_pose_set puts the scene into the pose.  The pose persists until the next swr_pose_set, swr_scene_skin or swr_scene_upload.
 *     joints == NULL with joint_count == 0 restores the bind pose: the scene is bit for bit what the upload built.
 *   Arithmetic (normative): IEEE binary32, one rounding per operation, no FMA.  For the vertex (x, y, z) and every influence
 *     k = 0..3, in this order, with c0..c3 the columns of joints[joint[k]] (16 floats, column-major like a frame's transform):
 *         r_k = c0.xyz * x;   r_k = r_k + c1.xyz * y;   r_k = r_k + c2.xyz * z;   r_k = r_k + c3.xyz * 1.0f;
 *     then   acc = weight[0] * r_0;   acc = acc + weight[1] * r_1;   acc = acc + weight[2] * r_2;   acc = acc + weight[3] * r_3;
 *     and the posed position is acc.  The fourth row of a joint matrix is ignored: joints are affine, the frame's own transform
 *     carries the perspective.  Normals (scenes with attributes only) take the same two steps without the c3 term, blended with
 *     the same weights: no inverse transpose and no renormalisation, the fragment stage normalises per pixel.  Colour and uv never
 *     change.  There are no special cases: all four influences are always read, zero, negative and non-finite weights follow IEEE
 *     (a -0 coordinate may come out as +0), and a triangle with a non-finite posed coordinate is skipped exactly as an uploaded one.
 *   What a pose is.  Every frame, read and query after swr_pose_set is bit for bit that of a context on which swr_scene_upload
 *     (and swr_scene_attributes) was given the posed vertices (and normals) with the same indices: every entry point, flag, rule
 *     set, draw list and primitive type.  Primitive IDs, painter's order and tie order keep the numbering of the index array.
 *   Ordering.  swr_pose_set and swr_scene_skin first complete and check everything drawn before (an overflowed last frame is
 *     repaired in the pose it was drawn in), then rewrite the scene, and return when the pose is in effect: blocking, like
 *     swr_scene_attributes.  A frame posted before the call never sees the new pose.  A multi-device context poses every band.
 *   Errors.  SWR_ERR_NO_SCENE: no scene.  SWR_ERR_BAD_ARG: a NULL ctx; a vertex_count that does not match the scene; skin == NULL
 *     with vertex_count > 0 on a scene that has vertices; a joint index >= SWR_SKIN_MAX_JOINTS; swr_pose_set without a skin;
 *     joint_count < 0; joint_count <= the largest joint index the skin uses; NULL joints with joint_count > 0.
 *     SWR_ERR_UNSUPPORTED: joint_count > SWR_SKIN_MAX_JOINTS.  A failed context returns its sticky error.  After an error the
 *     scene and the pose are unchanged.
 *   Not covered: a pose that does not wait (ordered by events), a partial vertex update from the host, and the C++ and Swift
 *     mirrors.  (Dual-quaternion skinning is the next section.  Normals that are right under scale or shear: "Computed normals".) */
typedef struct swr_skin_vertex {
    uint32_t joint[4];   /* indices into the pose; all four are always read */
    float    weight[4];  /* used as given: not normalised, not sorted, not skipped when 0 */
} swr_skin_vertex;       /* 32 bytes, parallel to swr_vertex: entry i belongs to vertex i */
#define SWR_SKIN_MAX_JOINTS 1024

/* ---- Dual-quaternion skinning (swr_pose_set_dq) — DESIGN.md §26 -------------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_pose_set_dq symbol is the feature test.  Nothing
 * existing changes.  swr_pose_set blends the four joint matrices, and that blend is not a rotation: a vertex weighted half and half
 * between a joint at rest and one twisted 180 degrees about the bone lands on the bone (the "candy wrapper").  swr_pose_set_dq
 * blends the joints as unit dual quaternions instead, so the blend stays a rigid motion.
 *   dual_quats is joint_count x 8 floats: per joint the real quaternion (x, y, z, w), then the dual quaternion (x, y, z, w); w is
 *     the scalar part.  For a rotation quaternion r and a translation t the dual part is 0.5 * (t, 0) * r.
 *   One pose state.  It is the pose state of "Skinned meshes": the skin of swr_scene_skin, the limit SWR_SKIN_MAX_JOINTS, one pose in
 *     effect.  The pose in effect is that of the last call of either kind, swr_pose_set or swr_pose_set_dq.
 *     swr_pose_set_dq(ctx, NULL, 0) and swr_pose_set(ctx, NULL, 0) both restore the bind pose, whichever kind is in effect.
 *   Carried over from "Skinned meshes", by reference: its Ordering paragraph (everything drawn before is completed and checked first,
 *     the call blocks, a frame posted before the call never sees the new pose, a multi-device context poses every band); its lifetime
 *     (a new swr_scene_skin or swr_scene_upload discards the pose); "Order with the skin" of "Morph targets" (morph first, then skin:
 *     v and n below are the morphed ones when weights are set); and its Errors paragraph, with swr_pose_set_dq in the messages and
 *     "NULL dual_quats with joint_count > 0" for the last SWR_ERR_BAD_ARG.  A failed context returns its sticky error.  After an
 *     error the scene and the pose are unchanged.
 *   Arithmetic (normative): IEEE binary32, one rounding per operation, no FMA; sqrtf and / are correctly rounded.  For the vertex v
 *     and every influence k = 0..3, Q_k = dual_quats[joint[k]], with R_k its first four and D_k its last four floats.
 *     Sign.  u_0 = weight[0].  For k = 1..3:  s_k = ((R_0.x*R_k.x + R_0.y*R_k.y) + R_0.z*R_k.z) + R_0.w*R_k.w;
 *         u_k = s_k < 0.0f ? -weight[k] : weight[k].  A NaN or zero s_k keeps the weight.  (q and -q are the same rotation; influence
 *         0 is the pivot.)
 *     Blend, per component of the eight:  B = u_0*Q_0;   B = B + u_1*Q_1;   B = B + u_2*Q_2;   B = B + u_3*Q_3.
 *     Normalise.  n = ((B.x*B.x + B.y*B.y) + B.z*B.z) + B.w*B.w over the real part;  l = sqrtf(n);  i = 1.0f / l;  C = B * i (eight
 *         multiplies).  The dual part is not made orthogonal to the real part: the translation below does not need it.
 *     Rotate a vector x, with q = C.real.xyz and w = C.real.w, where
 *         cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), two products and one subtraction each:
 *         a = cross(q, x);   b = a + w*x;   c = cross(q, b);   rot(x) = x + 2.0f*c.
 *     Translate.  With d = C.dual.xyz and dw = C.dual.w:  e = cross(q, d);   t = 2.0f * ((w*d - dw*q) + e).
 *     The posed position is rot(v) + t.  Normals (scenes with attributes only) are rot(n): no translation, no renormalisation.
 *     Colour, uv and the padding lanes never change.  There are no special cases: all four influences are always read; a zero blend
 *     (l == 0) gives non-finite coordinates and the triangle is skipped exactly as an uploaded one; a -0 coordinate may come out as
 *     +0; the payload of a NaN result is unspecified (nothing a frame shows depends on it).
 *   Input contract.  The call does not normalise its input and does not check that it is a unit dual quaternion.  A non-unit real
 *     part scales nothing: it only changes that joint's share of the blend.  A joint with scale or shear cannot be expressed as a
 *     dual quaternion: use swr_pose_set for those.
 *   What a pose is.  As in "Skinned meshes": every frame, read and query after swr_pose_set_dq is bit for bit that of a context on
 *     which swr_scene_upload (and swr_scene_attributes) was given the posed vertices (and normals) with the same indices.
 *   Not covered: a per-vertex choice of the mode, scale carried beside the dual quaternion, a pose that does not wait, converting
 *     matrices on the device, and the C++ and Swift mirrors. */

/* ---- Morph targets (swr_scene_morph, swr_morph_set) — DESIGN.md §24 ----------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_morph_set symbol is the feature test.  Nothing
 * existing changes.  The resident scene can change its shape without a new swr_scene_upload: swr_scene_morph gives it up to
 * SWR_MORPH_MAX_TARGETS morph targets (blend shapes), per-vertex deltas of position and, optionally, normal, and swr_morph_set
 * rewrites the resident triangle stream on the device from a weight per target.
 *   Arithmetic (normative): IEEE binary32, one rounding per operation, no FMA.  For vertex i the base position is b, exactly as
 *     uploaded, d[t][i] is the position delta of target t, and the weights are w[0 .. T).  Start with p = b.  Walk t in ascending
 *     order.  For every t with w[t] != 0.0f (float compare), p = p + w[t] * d[t][i], componentwise: the product is rounded, then the
 *     sum is rounded.  The morphed position is p.
 *     A target whose weight is +0 or -0 is skipped and its deltas are not read: a NaN or infinite delta in a zero-weight target
 *     changes nothing, and a -0 coordinate stays -0.  A NaN weight compares unequal to 0 and is applied.  The skip is normative: it
 *     makes a rig of 100 targets with 4 active cost 4, and it is bit-defined where x + 0 * d is not (-0 would become +0, 0 * inf NaN).
 *     Normals take the same loop with normal_deltas, only when the scene has attributes and normal_deltas was given; otherwise
 *     normals stay as uploaded.  Normal deltas given before swr_scene_attributes arrives are kept and take effect when it does.
 *     Colour, uv and the padding lanes never change.
 *   Order with the skin.  Morph first, then skin: the position and normal that the "Skinned meshes" arithmetic reads are the
 *     morphed ones.  Without a skin or a pose, the morphed vertices are the scene.
 *   What a morph is.  Every frame, read and query after the call is bit for bit that of a context on which swr_scene_upload (and
 *     swr_scene_attributes) was given the morphed-then-posed vertices (and normals) with the same indices: every entry point, flag,
 *     rule set, draw list and primitive type.  Primitive IDs, painter's order and tie order keep the numbering of the index array.
 *     When all weights are zero, the scene is bit for bit what the upload built, or what the current pose alone built.
 *   Lifetime.  swr_scene_morph follows the swr_scene_upload it belongs to, before or after swr_scene_attributes and swr_scene_skin.
 *     It copies the deltas: the caller's arrays are free on return.  New targets set every weight to 0; they keep the skin and the
 *     pose, which is re-applied to the unmorphed base.  targets == NULL removes the targets.  A new swr_scene_upload (the one a
 *     swr_render performs included) discards targets and weights.  swr_morph_set persists until the next swr_morph_set,
 *     swr_scene_morph or swr_scene_upload.  swr_pose_set and swr_scene_skin keep the weights: the new pose is applied to the
 *     morphed vertices.
 *   Ordering.  swr_scene_morph and swr_morph_set first complete and check everything drawn before, exactly as swr_pose_set does
 *     (an overflowed last frame is repaired in the shape it was drawn in), then rewrite the scene, and return when it is in effect:
 *     blocking.  A frame posted before the call never sees the new shape.  A multi-device context morphs every band.
 *   Errors.  SWR_ERR_NO_SCENE: no scene.  SWR_ERR_BAD_ARG: a NULL ctx; a vertex_count that does not match the scene; NULL
 *     position_deltas; target_count < 1; a non-zero reserved; swr_morph_set without targets; weight_count not equal to the target
 *     count (except NULL with 0); NULL weights with a positive count.  SWR_ERR_UNSUPPORTED: target_count > SWR_MORPH_MAX_TARGETS.
 *     SWR_ERR_NOMEM: the delta buffer cannot be allocated.  A failed context returns its sticky error.  After an error the scene,
 *     the targets and the weights are unchanged.
 *   Not covered: sparse targets, morphing colours or uv, one call that sets weights and joints together (today swr_morph_set
 *     followed by swr_pose_set runs the skin and stream passes twice), an un-waited morph, and the C++ and Swift mirrors.
 *     (Normals for targets without normal_deltas: "Computed normals".) */
#define SWR_MORPH_MAX_TARGETS 256
typedef struct swr_morph_targets {
    const float* position_deltas; /* target_count x vertex_count x 3 floats, target-major, tightly packed (glTF VEC3 accessors back to back) */
    const float* normal_deltas;   /* same shape, or NULL: normals do not morph */
    int64_t vertex_count;         /* must equal the resident scene's */
    int32_t target_count;         /* 1 .. SWR_MORPH_MAX_TARGETS */
    int32_t reserved;             /* 0 */
} swr_morph_targets;              /* 32 bytes */

/* ---- Item bounds (swr_item_bounds) — DESIGN.md §25 ---------------------------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_item_bounds symbol is the feature test.  Nothing
 * existing changes.  swr_query_depth and swr_count_ids take screen rectangles from the caller; since "Skinned meshes" and "Morph
 * targets" the vertices an object is drawn from exist only on the device.  swr_item_bounds says where every item of a draw list would
 * land and how near it is, in the arithmetic the frame itself uses; 48 bytes per item cross to the host.
 *   Input.  Item k is exactly what swr_draw_list would draw: the triangles indices[first_index, first_index + index_count) of the
 *     resident scene as it is now (morphed and posed), transformed by items[k].transform, on the target of swr_target_set.
 *   Per corner (normative): IEEE binary32, one rounding per operation, no FMA.  With c0..c3 the columns of the transform:
 *         r = c0 * x;   r = r + c1 * y;   r = r + c2 * z;   r = r + c3 * 1.0f;        ndc = r.xyz / r.w;
 *         sx = (ndc.x * 0.5f + 0.5f) * W;   sy = (ndc.y * -0.5f + 0.5f) * H;   sz = ndc.z;
 *     and under SWR_FLAG_METAL_RULES sx = roundf(sx), sy = roundf(sy) (half away from zero): what the frame's setup computes.
 *   Drawable.  A triangle is drawable iff all six of its sx, sy satisfy |v| < 2^30 and, under the Metal rules, v >= 0: the coordinate
 *     part of the frame's skip rule.  A triangle whose integer vertices are collinear counts as drawable, and so does one a frame
 *     would cull by its facing (the cull bits are ignored: the bounds cover both facings): the answer is conservative.
 *     drawable + skipped == index_count / 3.
 *   The rectangle.  With ix = (int)sx, iy = (int)sy (truncation, the integer vertices of "Face culling") over the corners of the
 *     drawable triangles: x0 = min ix, x1 = max ix + 1, y0 = min iy, y1 = max iy + 1, then each clamped, x into [0, W] and y into
 *     [0, H].  Every pixel the item covers lies inside it.  An item wholly off the target gives an empty rectangle (x0 == x1 or
 *     y0 == y1), which is legal input to swr_query_depth and swr_count_ids.  All 0 when drawable == 0.
 *   The depth range.  zmin and zmax are folded with s < m ? s : m and s > m ? s : m from +inf and -inf over all three sz of every
 *     drawable triangle, so a NaN sz is left out by the fold itself; a zero result is returned as +0 (m + 0.0f).  Minimum and maximum
 *     do not depend on the order: the result is bit-defined.
 *     zmin is the nearest VERTEX.  A fragment's depth za*w0 + zb*w1 + zc*w2 can leave [zmin, zmax] by rounding, and under the CPU
 *     rules also by extrapolation at span pixels outside the triangle: a caller who feeds zmin to swr_query_depth subtracts a margin
 *     of their own.
 *   behind counts the drawable triangles with a corner whose clip-space w (r.w) is not > 0.  Without SWR_FLAG_DEPTH_CLIP such a
 *     triangle is drawn mirrored through the eye: the caller should not cull an item on bounds with behind != 0.
 *   flags.  Every combination swr_draw_list accepts is accepted, and only SWR_FLAG_METAL_RULES changes the result.  SWR_FLAG_DEPTH_CLIP
 *     returns SWR_ERR_UNSUPPORTED: the rectangle of a clipped fan is not that of its triangle.  Unknown bits: SWR_ERR_BAD_ARG.
 *   Items.  Checked exactly as swr_draw_list checks them (SWR_ERR_INDEX_COUNT, SWR_ERR_BAD_ARG, SWR_ERR_UNSUPPORTED above
 *     SWR_DRAW_LIST_MAX items, SWR_ERR_NO_SCENE without a scene or a target).  Ranges may overlap and repeat.  item_count == 0 is legal,
 *     and items and out may then be NULL; NULL out with item_count > 0 is SWR_ERR_BAD_ARG.  An empty item gives drawable = skipped =
 *     behind = 0, the all-0 rectangle and zmin / zmax = +inf / -inf.  After an error nothing was written.
 *   Completion.  Blocking, like swr_query_depth: everything drawn before is completed and checked first (an overflowed last frame is
 *     repaired).  No image and no delta baseline is modified, what the next frame draws does not change, and the call does not count
 *     as a frame: swr_read_ids and swr_count_ids after it see the last frame as before.  On a scene uploaded in Morton order the call
 *     cuts the triangle stream at the items' boundaries, as the first swr_draw_list of these items would; that list then finds the
 *     cuts in place.
 *   Bands.  The result does not depend on rows.  A multi-device context computes on its first band (every band holds the whole scene)
 *     and writes the caller's array once; a context that owns rows [a, b) of a larger target answers for the full W x H.  After
 *     swr_render_resolved the target is the sample grid, and the rectangles are in samples.
 *   Not covered: SWR_FLAG_DEPTH_CLIP, a call that does not wait, the bounds of .vertices and .line passes, and the C++ and Swift
 *     mirrors. */
typedef struct swr_item_bound {
    int32_t  x0, y0, x1, y1;  /* half-open pixel rectangle in the full W x H target, clipped to it; all 0 when drawable == 0 */
    float    zmin, zmax;      /* over the corners' sz of drawable triangles; +inf / -inf when there is none */
    uint32_t drawable;        /* triangles of the item that setup would not skip for their coordinates */
    uint32_t skipped;         /* the others: drawable + skipped == index_count / 3 */
    uint32_t behind;          /* drawable triangles with a corner whose clip-space w is not > 0 */
    uint32_t reserved[3];     /* 0 on return */
} swr_item_bound;             /* 48 bytes */

/* ---- Sparse morph targets (swr_scene_morph_sparse) — DESIGN.md §28 -----------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_scene_morph_sparse symbol is the feature test.
 * Nothing existing changes.  This section covers the "sparse targets" that the "Not covered" line of "Morph targets" names: a target
 * lists only the vertices it moves, as a glTF sparse accessor does, and only those are stored on the device and rewritten by
 * swr_morph_set.
 *   One morph state.  The targets in effect are those of the last swr_scene_morph or swr_scene_morph_sparse.  Either call with
 *     NULL removes whichever kind is resident.  swr_morph_set serves both kinds: one weight per target, the same errors.
 *   Arithmetic (normative): IEEE binary32, one rounding per operation, no FMA.  For vertex i start with p = b, the position as
 *     uploaded.  Walk t in ascending order.  For every t with w[t] != 0.0f whose index list contains i at position j,
 *     p = p + w[t] * d_t[j], componentwise: the product is rounded, then the sum.
 *     A vertex a target does not list is not touched by that target.  This is not the dense target with a zero delta: an unlisted
 *     -0 coordinate stays -0 where an applied zero delta makes it +0, and a NaN or infinite weight poisons only the listed
 *     vertices.  A zero-weight target's deltas never enter the arithmetic; the device may still read them.
 *     Normals take the same loop with normal_deltas, under the conditions of "Morph targets" (the scene has attributes; deltas
 *     given before swr_scene_attributes take effect when it arrives).  Either every target with count > 0 gives normal_deltas or
 *     none does.  Colour, uv and the padding lanes never change.
 *   What a sparse morph is.  Every frame, read and query after the call is bit for bit that of a context that uploaded the
 *     morphed-then-posed vertices.
 *   Lifetime, Ordering and "Order with the skin" of "Morph targets" apply unchanged: new targets set every weight to 0 and keep
 *     skin and pose; an upload discards targets and weights; the call is blocking and first completes and checks everything drawn
 *     before; the arrays are copied and free on return; a multi-device context morphs every band.
 *   Errors, all checked before anything changes.  SWR_ERR_NO_SCENE: no scene.  SWR_ERR_BAD_ARG: a NULL ctx; a vertex_count that
 *     does not match the scene; a NULL targets array; target_count < 1; a non-zero reserved; count < 0 or count > vertex_count;
 *     NULL indices or position_deltas with count > 0; an index >= vertex_count, or indices not strictly ascending (the message
 *     names the target and the position); normal deltas on some non-empty targets only.  SWR_ERR_UNSUPPORTED: target_count >
 *     SWR_MORPH_MAX_TARGETS.  SWR_ERR_NOMEM: a device allocation fails.  A failed context returns its sticky error.  After an
 *     error the scene, the targets of either kind and the weights are unchanged.
 *   Not covered: morphing colours or uv, an un-waited morph, and the C++ and Swift mirrors. */
typedef struct swr_morph_sparse_target {
    const uint32_t* indices;          /* count vertex indices, strictly ascending, each < vertex_count */
    const float*    position_deltas;  /* count x 3 floats: entry j belongs to vertex indices[j] */
    const float*    normal_deltas;    /* count x 3 floats, or NULL */
    int64_t         count;            /* 0 .. vertex_count; 0 = an empty target, the pointers may be NULL */
} swr_morph_sparse_target;            /* 32 bytes */
typedef struct swr_morph_sparse {
    const swr_morph_sparse_target* targets;
    int64_t vertex_count;             /* must equal the resident scene's */
    int32_t target_count;             /* 1 .. SWR_MORPH_MAX_TARGETS */
    int32_t reserved;                 /* 0 */
} swr_morph_sparse;                   /* 24 bytes */

/* ---- Weights and joints in one call (swr_morph_pose_set) — DESIGN.md §28 -----------------------------------------------------------
 * No ABI bump and no flag bit: the presence of the swr_morph_pose_set symbol is the feature test.  This section covers the "one
 * call that sets weights and joints together" that the "Not covered" line of "Morph targets" names.
 *   The call is exactly swr_morph_set(weights, weight_count) followed by swr_pose_set (pose_kind SWR_POSE_MATRICES) or
 *     swr_pose_set_dq (SWR_POSE_DUAL_QUATS) with joints, joint_count, with two differences.  Every argument of both halves is
 *     validated before anything changes: after an error neither the weights nor the pose have changed.  And the scene is rewritten
 *     once: the skin and stream passes run once, and the call waits once.
 *   It needs targets (of either kind) and a skin.  NULL weights with 0 and NULL joints with 0 mean what they mean in the two calls.
 *   Errors: those of the two calls, under their conditions, and SWR_ERR_BAD_ARG for an unknown pose_kind. */
enum { SWR_POSE_MATRICES = 0, SWR_POSE_DUAL_QUATS = 1 };

/* ---- Computed normals (swr_scene_normals) — DESIGN.md §29 ---------------------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_scene_normals symbol is the feature test.  Nothing
 * existing changes.  The normals of the resident scene can be computed on the device from the positions that are drawn, instead of
 * being uploaded: a morph target without normal deltas, the matrix skin's blend "without inverse transpose" under scale or shear, and
 * a mesh that has no normals at all then light the surface as it is drawn.  normals == NULL means SWR_NORMALS_UPLOADED.
 *   Positions and triangles.  a, b and c are the positions the frame draws for triangle p: the morphed-then-posed xyz of
 *     indices[3p], indices[3p + 1] and indices[3p + 2].  p runs over 0 .. index_count / 3 - 1; trailing indices are ignored.  The
 *     normals are in object space, like light_dir: the frame's transform is not involved.
 *   Face vector (normative): IEEE binary32, one rounding per operation, no FMA.  e1 = b - a and e2 = c - a, componentwise.
 *     f_p = cross(e1, e2), with cross exactly as "Dual-quaternion skinning" defines it: two products and one subtraction per
 *     component.  Under SWR_NORMALS_FLIP, f_p = cross(e2, e1).
 *   SWR_NORMALS_FLAT.  All three corners of triangle p take the normal f_p.  It is not normalised: the fragment stage normalises per
 *     pixel.  This is what glTF prescribes for a mesh without normals.
 *   SWR_NORMALS_SMOOTH.  For vertex i start with n = (+0, +0, +0).  Walk p in ascending order, and inside p the corners k = 0, 1, 2.
 *     For every corner with indices[3p + k] == i, n = n + f_p, componentwise: a triangle that names i twice adds twice.  Then
 *     normalise:  l = sqrtf((n.x*n.x + n.y*n.y) + n.z*n.z), with sqrtf and the divide correctly rounded.  If l > 0.0f,
 *     n = n * (1.0f / l): one divide, three multiplies.  Otherwise n stays as it is: a vertex of no triangle stays (0, 0, 0), which
 *     the Phong stage treats as the zero vector, and a NaN l leaves n as the sum made it.  Every corner that references i takes n.
 *     The walk order is normative: it is what makes the sum bit-defined.  There are no other special cases: a non-finite position
 *     poisons the faces that use it and the vertices of those faces, and nothing else.
 *   What is replaced.  Only the normals the frames read.  Colour, uv, the padding lanes, positions, group boxes and the uploaded
 *     attribute array are never written.  While a computed mode is in effect, morph normal_deltas and the normal half of either
 *     skinning mode have no effect on any frame (the implementation may skip them).
 *   What the mode is.  Under SMOOTH every frame, read and query after the call is bit for bit that of a context on which
 *     swr_scene_upload got the morphed-then-posed vertices and swr_scene_attributes got the same uv with the n_i above.  Under FLAT
 *     it is that of the de-indexed scene: vertex 3p + k is corner k of triangle p, the indices are 0 .. 3 * ntri - 1, and each
 *     corner carries f_p.  Primitive IDs, painter's order and tie order are unchanged.  .vertices and .line frames and the
 *     passthrough shader never read normals and do not change.
 *   Lifetime.  The mode follows the swr_scene_upload it belongs to; it may be set before or after swr_scene_attributes,
 *     swr_scene_skin and swr_scene_morph[_sparse].  It takes effect only while the scene has attributes: set earlier, it is kept and
 *     takes effect when swr_scene_attributes arrives, as morph normal deltas do.  It persists across swr_pose_set, swr_pose_set_dq,
 *     swr_morph_set, swr_morph_pose_set, swr_scene_skin, swr_scene_morph and swr_scene_morph_sparse, and the normals are recomputed
 *     whenever one of them rewrites the scene.  SWR_NORMALS_UPLOADED (or NULL) restores the uploaded normals, morphed and posed as
 *     before: bit for bit what a context that never set a mode holds.  A new swr_scene_upload (the one a swr_render performs
 *     included) discards the mode.
 *   Ordering.  The Ordering paragraph of "Skinned meshes" applies: everything drawn before is completed and checked first, the call
 *     is blocking, a frame posted before the call never sees the new normals, and a multi-device context recomputes on every band.
 *   Errors, all checked before anything changes.  SWR_ERR_NO_SCENE: no scene.  SWR_ERR_BAD_ARG: a NULL ctx; an unknown mode; unknown
 *     flag bits; a non-zero reserved word.  SWR_ERR_UNSUPPORTED: SWR_NORMALS_SMOOTH on a scene with 2^32 or more indices.
 *     SWR_ERR_NOMEM: a device allocation fails.  A failed context returns its sticky error.  After an error the mode and the scene
 *     are unchanged.
 *   Cost.  SWR_NORMALS_SMOOTH builds a vertex-to-triangle adjacency once per scene, on the host, in the call (4 bytes per vertex and
 *     per index stay resident, beside 16 per triangle and per vertex); every later rewrite of the scene pays two more kernels.
 *     One lane sums one vertex's faces in order, so a vertex shared by thousands of triangles is slow.  SWR_NORMALS_FLAT needs
 *     neither and pays one kernel.
 *   Not covered: angle-weighted normals, crease angles and smoothing groups, tangents, swr_render passes (which have no field for
 *     the mode), an un-waited call, and the C++ and Swift mirrors. */
enum { SWR_NORMALS_UPLOADED = 0, SWR_NORMALS_SMOOTH = 1, SWR_NORMALS_FLAT = 2 };
enum { SWR_NORMALS_FLIP = 1u << 0 };
typedef struct swr_normals {
    int32_t  mode;        /* SWR_NORMALS_* */
    uint32_t flags;       /* SWR_NORMALS_FLIP or 0 */
    int32_t  reserved[2]; /* 0 */
} swr_normals;            /* 16 bytes */

/* ---- Ray casts (swr_cast_rays) — DESIGN.md §30 --------------------------------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_cast_rays symbol is the feature test.  Nothing
 * existing changes.  Once a scene is morphed and posed on the device, the vertices an object is drawn from exist only there.
 * swr_cast_rays answers "what does this line hit?" against them: hits[k] is the nearest accepted hit of rays[k], for n rays a call.
 *   Space.  Rays are in the space of the resident vertices: object space, the scene as it is now — morphed, posed, and with whatever
 *     swr_scene_upload gave.  No transform is applied: a caller with a draw item's transform brings the ray into that space itself.
 *   Which triangles.  Triangle p has the corners a, b, c = the positions of indices[3p], indices[3p + 1], indices[3p + 2], for
 *     p < index_count / 3, whatever the primitive type of later draws; trailing indices are ignored.
 *   Result.  hits[k].primitive is p in the numbering of the index array, as primitive IDs use it; t, u, v come from the arithmetic
 *     below.  The hit point is origin + t*dir, or equivalently (1-u-v)*a + u*b + v*c.  A miss is primitive = SWR_ID_NONE,
 *     t = u = v = 0.
 *   Arithmetic (normative): IEEE binary32, one rounding per operation, no FMA; / is correctly rounded.
 *     dot(x, y) = (x.x*y.x + x.y*y.y) + x.z*y.z;  cross exactly as "Dual-quaternion skinning" defines it: two products and one
 *     subtraction per component.  Per ray and triangle:
 *     1. Skip.  A triangle with a corner coordinate that is not finite is never hit (the frames skip it too).
 *     2. Box pre-test.  Start [nr, fr] = [tmin, tmax].  For each axis j = x, y, z:  lo = the smallest and hi = the largest of the
 *        three corners' coordinate j;  r = 1.0f / dir[j].
 *          If dir[j] == 0.0f or !(fabsf(r) <= FLT_MAX), the axis is parallel: the triangle is rejected unless
 *            lo <= origin[j] && origin[j] <= hi.
 *          Otherwise  t0 = (lo - origin[j]) * r;  t1 = (hi - origin[j]) * r;  near = t0 < t1 ? t0 : t1;  far = t0 < t1 ? t1 : t0;
 *            nr = near > nr ? near : nr;  fr = far < fr ? far : fr.
 *        After the three axes the triangle is rejected unless nr <= fr.  With finite inputs none of these values is a NaN: on an
 *        axis that is not parallel r is finite and not zero, so t0 and t1 are products of a finite number or an infinity (a
 *        difference that overflowed) with a finite non-zero number, never 0 * inf and never inf - inf.  The pre-test is normative:
 *        it may reject a triangle the next step would graze, and it is what lets an implementation cull whole groups exactly.
 *     3. Moeller-Trumbore.  e1 = b - a;  e2 = c - a;  pv = cross(dir, e2);  det = dot(e1, pv).  Reject unless fabsf(det) > 0.0f.
 *        inv = 1.0f / det;  tv = origin - a;  u = dot(tv, pv) * inv.  Reject unless u >= 0.0f && u <= 1.0f.
 *        qv = cross(tv, e1);  v = dot(dir, qv) * inv.  Reject unless v >= 0.0f && u + v <= 1.0f.
 *        t = dot(e2, qv) * inv + 0.0f (a zero comes out as +0).  Reject unless t >= tmin && t <= tmax.
 *        Both facings are hit.  A comparison with a NaN (an overflowed intermediate) rejects.
 *     4. Winner.  Of the accepted triangles the one with the smallest t wins; on equal t the smallest p.  This does not depend on any
 *        order of evaluation: the result is bit-defined.
 *   State.  The call changes nothing: the next frame, read and query are bit for bit what they would have been without it.
 *   Ordering.  Blocking, as swr_item_bounds: everything posted before is completed and checked first.  A multi-device context answers
 *     from its first band's copy of the scene (the scene is replicated).
 *   Errors, all checked before anything runs.  SWR_ERR_NO_SCENE: no scene.  SWR_ERR_BAD_ARG: a NULL ctx; n < 0; NULL rays or hits with
 *     n > 0; flags != 0; a ray with a float that is not finite; an all-zero direction; tmin > tmax — the message names the ray's index.
 *     SWR_ERR_UNSUPPORTED: n > SWR_RAYS_MAX.  SWR_ERR_NOMEM: an allocation fails.  A failed context returns its sticky error.
 *     n == 0 succeeds.  A scene without triangles answers every ray with a miss.
 *   Not covered: any-hit / occlusion-only rays; the facing of the hit and face culling; rays restricted to an index range or a draw
 *     item; more than one hit per ray; watertight edges (a ray that grazes an edge or a triangle's box can miss both neighbours, as
 *     with any Moeller-Trumbore test); an un-waited call; and the C++ and Swift mirrors.  "Ray queries" below covers the first three. */
typedef struct swr_ray {
    float origin[3]; float tmin;
    float dir[3];    float tmax;
} swr_ray;                /* 32 bytes */
typedef struct swr_ray_hit {
    uint32_t primitive;   /* SWR_ID_NONE: a miss */
    float t, u, v;
} swr_ray_hit;            /* 16 bytes */
#define SWR_RAYS_MAX (1 << 16)

/* ---- Ray queries (swr_query_rays) — DESIGN.md §31 -----------------------------------------------------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6) and no flag bit: the presence of the swr_query_rays symbol is the feature test.  Nothing
 * existing changes: swr_cast_rays still refuses every non-zero flags.  swr_query_rays is swr_cast_rays with three additions, chosen by
 * a swr_ray_query: occlusion rays (one bit per ray), a facing cull, and a range of primitives.  query == NULL means all defaults:
 * flags 0, first_primitive 0, primitive_count -1.
 *   Carried over from "Ray casts".  Its Space and Which triangles paragraphs, the numbering of p, and steps 1 to 3 with their
 *     arithmetic: IEEE binary32, one rounding per operation, no FMA.  Its State, Ordering and Errors paragraphs hold with
 *     swr_query_rays in the messages; a refused ray is named by its index.  n == 0 succeeds.  A scene without triangles answers every
 *     ray with a miss.
 *   Range.  Only triangles p with first_primitive <= p < first_primitive + primitive_count are candidates.  With primitive_count -1
 *     the range runs to index_count / 3.  p and hits[k].primitive stay in the numbering of the whole index array, as for primitive
 *     IDs.  An empty range is legal and answers every ray with a miss.  For draw item k the range is first_index / 3,
 *     index_count / 3.
 *   Facing.  det of step 3 decides.  Without SWR_RAYS_FRONT_CW a triangle is front-facing for the ray iff det > 0.0f: the ray arrives
 *     from the side cross(b - a, c - a) points to (the face vector of "Computed normals" without SWR_NORMALS_FLIP), and seen from the
 *     ray's origin a, b, c run counter-clockwise in a right-handed space.  With SWR_RAYS_FRONT_CW front-facing is det < 0.0f.
 *     SWR_RAYS_CULL_BACK rejects the triangles that are not front-facing, SWR_RAYS_CULL_FRONT rejects the front-facing ones.  The
 *     reject sits directly after "Reject unless fabsf(det) > 0.0f", on the same det bits.  Both bits reject everything, which is
 *     legal, as for frames.  This is the geometric winding in object space, not the screen winding of "Face culling": that one
 *     depends on the frame's transform and the y flip, this one on neither.  The hit record has no room for the facing: a caller
 *     learns it by culling.
 *   Nearest mode (no SWR_RAYS_ANY_HIT).  Step 4 of "Ray casts" over the triangles that survive range and cull.  With query == NULL,
 *     or with flags 0, first_primitive 0 and primitive_count -1, hits is bit for bit what swr_cast_rays writes.
 *   SWR_RAYS_ANY_HIT.  hits[k] is {SWR_RAY_OCCLUDED, 0, 0, 0} iff at least one surviving triangle is accepted by steps 1 to 3;
 *     otherwise it is the miss record {SWR_ID_NONE, 0, 0, 0}.  Which triangle is never reported: that is what keeps the answer
 *     independent of any order of evaluation, and therefore bit-defined.  Equivalently, a ray is occluded iff the nearest-mode answer
 *     of the same query is not a miss; hits[k].primitive != SWR_ID_NONE means "hit" in both modes.  swr_scene_upload refuses a scene
 *     of more than 2^32 - 2 primitives, so SWR_RAY_OCCLUDED is never a primitive number.
 *   Errors, added.  SWR_ERR_BAD_ARG: unknown flag bits; a non-zero reserved; first_primitive < 0; primitive_count < -1; a range
 *     that ends beyond index_count / 3.  All are checked before anything runs; after an error nothing was written.
 *   Not covered: more than one hit per ray; watertight edges; an un-waited call; and the C++ and Swift mirrors.  A range is filtered
 *     per triangle: it does not make the call cheaper on a reordered stream. */
enum { SWR_RAYS_ANY_HIT = 1u << 0, SWR_RAYS_CULL_BACK = 1u << 1, SWR_RAYS_CULL_FRONT = 1u << 2, SWR_RAYS_FRONT_CW = 1u << 3 };
#define SWR_RAY_OCCLUDED 0xFFFFFFFEu
typedef struct swr_ray_query {
    uint32_t flags;            /* SWR_RAYS_* */
    uint32_t reserved;         /* 0 */
    int64_t  first_primitive;  /* >= 0 */
    int64_t  primitive_count;  /* >= 0, or -1: to the end of the scene */
} swr_ray_query;               /* 24 bytes */

/* ---- Load frames (SWR_FLAG_LOAD, ABI 6) — DESIGN.md §11 ------------------------------------------------------------------
 * A load frame runs Renderer.render(renderPass:) without Renderer.swift:205-206: the same triangle (.vertices, .line) loop
 * continues from the image already there.
 *   z-test (SWR_FLAG_DEPTH_TEST; always under SWR_FLAG_METAL_RULES): a fragment is kept iff d < depth[x,y], depth[x,y] starting at
 *     the loaded value — strict '<', so on an equal depth the image that was there wins (first drawn wins, across frames).  A loaded
 *     NaN or -inf is never replaced; -0 and +0 compare equal (neither replaces the other); denormals compare exactly.
 *   painter's order (no z-test): covered pixels are overwritten, the others keep the loaded colour; the depth image stays exactly
 *     as loaded.
 *   SWR_FLAG_NO_COLOR: colour is neither read nor written (the band's colour image after such a frame is unspecified, as before);
 *     depth is loaded.  .vertices and real lines behave as above; a .line frame without SWR_FLAG_REAL_LINES leaves the image as it is.
 * Composition: the image of scene A drawn with M_A, then scene B drawn with M_B as a load frame, is bit for bit the clear frame of
 * A || B drawn with the identity, every vertex pre-transformed by its own matrix (Vertex.apply order, float32, no FMA), B's indices
 * offset by A's vertex count; chains of any length alike.
 * The starting image:
 *   resident path (swr_draw / swr_draw_primitives): the band's image of the last frame drawn on the context;
 *   right after swr_target_set: the cleared image (colour 0, depth +inf) — a load frame there IS the clear frame;
 *   swr_target_write: the images it wrote;
 *   swr_render: pass->color / pass->depth are the starting image (swr_target_write + the draw); with scene_id the scene is still
 *     cached, the images never are.
 * Bin overflow: a load frame never builds silently on an overflowed frame.  A frame whose bins overflowed is rastered empty; if it
 *   is the last frame it is redrawn from the SAME starting image.  A load frame whose starting image is such an empty frame (or a
 *   load frame built on one, any number of frames back) counts as dropped: reported with SWR_ERR_FRAME_DROPPED when it was
 *   presented or when it is the last frame of the burst (whose image the next load frame or swr_read_* would see), and every later
 *   load frame on top of it is reported too, until a clear frame, swr_target_set or swr_target_write replaces the image. */

/* ---- Vertex (Renderer.swift:154-157): two SIMD3<Float>, each padded to 16 B --------- */
typedef struct swr_vertex {
    float xyz[4];    /* x,y,z, lane 3 = padding (ignored) */
    float color[4];  /* r,g,b, lane 3 = padding (ignored) */
} swr_vertex;        /* 32 bytes */

/* ---- fragment-stage extensions (BASELINE configs 3 and 5) -------------------
 * The reference's fragment stage returns the interpolated vertex colour (Shaders.metal:116-121) and has
 * no normals, texture coordinates, lights or textures.  These additions sit behind the same
 * fragment_shader(VertexOut) hook: VertexOut gains `normal` and `uv` varyings, interpolated exactly like
 * `color` (screen-affine barycentric weights, Renderer.swift:266 / Shaders.metal:162), and the hook
 * evaluates a Blinn-Phong model per pixel.  Every operation is a single IEEE binary32 + - * / sqrt in a
 * fixed order, so the CPU oracle and the HIP kernels agree bit for bit; parity for these
 * modes is build-internal (there is nothing in the reference to compare with). */
typedef struct swr_vertex_attr {
    float normal[4]; /* nx,ny,nz (any length; normalised per pixel), lane 3 = padding */
    float uv[4];     /* u,v (repeat addressing), lanes 2,3 = padding */
} swr_vertex_attr;   /* 32 bytes, parallel to swr_vertex: attribute i belongs to vertex i */

enum {
    SWR_SHADER_PASSTHROUGH = 0,    /* float4(vin.color, 1)                      (Shaders.metal:116-121) */
    SWR_SHADER_PHONG = 1,          /* base = vin.color                          (BASELINE config 3)     */
    SWR_SHADER_TEXTURED_PHONG = 2  /* base = vin.color * bilinear(texture, uv)  (BASELINE config 5)     */
};

/* rgb = base * (ambient + diffuse * max(N.L, 0)) + specular * max(N.H, 0)^(2^shininess_log2),  a = 1,
 * N = vin.normal / |vin.normal| (zero vector when the length is 0).  light_dir and half_dir are given by
 * the caller in the space of the normals (object space: normals are passed through untransformed, like
 * colours, Shaders.metal:53); half_dir is the Blinn half vector of a distant light and viewer. */
typedef struct swr_material {
    int32_t shader;          /* SWR_SHADER_* */
    int32_t shininess_log2;  /* 0..16: the exponent is a power of two, evaluated by repeated squaring */
    float   light_dir[4];    /* unit vector towards the light, lane 3 ignored */
    float   half_dir[4];     /* unit half vector, lane 3 ignored */
    float   ambient, diffuse, specular, reserved;
} swr_material;              /* 56 bytes */

/* ---- RenderPass (Renderer.swift:191-200) + Image<T> (Renderer.swift:8-21) ------------
 * color: Pixel = {b,g,r,a} u8 (Renderer.swift:44-49); element (x,y) at color[y*width+x]
 * (App.swift:351-360: addressing uses width; bytesPerRow is stored but never read, so
 * the two *_bytes_per_row fields are carried for layout parity and ignored). */
typedef struct swr_render_pass {
    void*    color;                 /* width*height*4 bytes, BGRA8; may be NULL iff SWR_FLAG_NO_COLOR */
    float*   depth;                 /* width*height floats */
    int64_t  width;
    int64_t  height;
    int64_t  color_bytes_per_row;   /* ignored, see above */
    int64_t  depth_bytes_per_row;   /* ignored */
    const swr_vertex* vertices;
    int64_t  vertex_count;
    const int64_t* indices;         /* Swift Int (Renderer.swift:196) */
    int64_t  index_count;
    int32_t  primitive_type;        /* SWR_PRIMITIVE_* ; default .triangle (Renderer.swift:197) */
    uint32_t flags;                 /* SWR_FLAG_* */
    float    transform[16];         /* matrix_float4x4, column-major: column c = transform[4c..4c+3]
                                       (Renderer.swift:199) */
    /* extensions (all optional; NULL = the reference's passthrough fragment stage) */
    const swr_vertex_attr* attributes;  /* vertex_count entries */
    const swr_material*    material;
    const void*            texture;     /* tex_width*tex_height Pixels (b,g,r,a), row-major; SWR_SHADER_TEXTURED_PHONG */
    int32_t  tex_width, tex_height;
    /* Scene identity (ABI 4).  The reference's only caller draws the SAME mesh every display frame with a new transform
     * (App.swift:153-185) and its GpuRenderer keeps its device buffers across calls (GpuRenderer.swift:32-33,41-67).
     * 0 = no promise: vertices / indices / attributes / texture are uploaded and the device-side triangle stream is
     * rebuilt on every call (what ABI 3 did) — as a scene that lives for ONE frame: in index order (no Morton sort),
     * built behind the copy of the index array.  Non-zero = the caller promises that the CONTENT of `vertices`,
     * `indices`, `attributes` and `texture` (and their counts / sizes) equals that of the last swr_render on this
     * context that carried the same id: the upload is then skipped and the pass costs one resident frame plus the
     * gather.  A new id (or new counts) uploads.  transform, flags, primitive_type, material and the image pointers
     * may change freely between calls with the same id. */
    uint64_t scene_id;
} swr_render_pass;      /* 192 bytes */

typedef struct swr_config {
    int32_t  device;        /* HIP device ordinal (of the first device); -1 = current device */
    uint32_t device_count;  /* 0 or 1: one GPU.  N > 1: the context drives N tile-row bands of the framebuffer, band k
                               on device (device + k) % min(N, visible devices), one host thread and one set of HIP
                               streams per band, scene replicated, no collective.  With fewer
                               visible GPUs than N, several bands share a GPU (same code path). */
    uint32_t wait_budget_ms;/* Longest time any single wait inside the library may take (a helper thread polling for a
                               kernel's completion, a blocking call waiting for the streams): 0 = default (20 000 ms).
                               When it expires the context fails for good: the blocking call returns SWR_ERR_HIP with the
                               frame number and what was being waited for, every later call returns the same error at
                               once, swr_context_destroy still returns (it may leak what the GPU still owns).  The
                               reference has no counterpart: scheduleAndWait blocks forever (Metal+Extensions.swift:57-67). */
    uint32_t reserved;      /* 0 */
} swr_config;               /* 16 bytes */

/* Per-kernel device times of the last swr_draw / swr_render on this context, measured with
 * hipEvents recorded on the context's own stream (only filled when timing is enabled). */
typedef struct swr_timings {
    float setup_bin_ms;   /* vertex transform + triangle setup + tile binning (count/emit) */
    float scan_ms;        /* per-tile offsets */
    float scatter_ms;     /* bin fill */
    float raster_ms;      /* tile raster + resolve + framebuffer write (the dominant kernel) */
    float total_ms;       /* first kernel start -> last kernel end */
    int64_t tile_pairs;   /* (triangle,tile) pairs binned in the frame */
    int64_t tiles;        /* tiles in the band */
    int64_t triangles;    /* primitives submitted */
} swr_timings;

typedef struct swr_context swr_context;

/* Library / ABI identification; number of visible HIP devices (0 when there is none or no driver). */
int         swr_abi_version(void);
const char* swr_version(void);
int         swr_device_count(void);

/* GpuRenderer() / Renderer() default initialisers (App.swift:148-149) + MTLContext.shared
 * (Metal+Extensions.swift:5-45): device(s), streams, cached scratch buffers.  The reference's one synchronous
 * draw call (GpuRenderer.swift:35, caller App.swift:185) maps onto ONE context whatever the number of GPUs:
 * with cfg->device_count = N every entry point below fans out to N per-device sub-contexts. */
int  swr_context_create(const swr_config* cfg, swr_context** out);
void swr_context_destroy(swr_context* ctx);
/* Number of bands (sub-contexts) of the context, and where band `band` lives: its HIP device and the rows
 * [row_begin,row_end) it owns after swr_target_set.  Any out pointer may be NULL. */
int  swr_context_bands(const swr_context* ctx);
int  swr_context_band_info(const swr_context* ctx, int32_t band, int32_t* device, int64_t* row_begin, int64_t* row_end);

/* Last error text for this context (NULL ctx: last error of a failed swr_context_create).  Call it from the thread that
 * made the failing call; the text stays valid until that thread's next call on the context. */
const char* swr_last_error(const swr_context* ctx);

/* Wall-clock phases of the last swr_render on this context (host steady clock; the H2D / stream-build split inside the
 * upload comes from HIP events).  scene_cached = 1 when the pass carried the scene_id of the resident scene and nothing
 * was uploaded. */
typedef struct swr_render_times {
    float h2d_ms;           /* vertices / indices / attributes / texture: host -> device */
    float stream_build_ms;  /* index check, Morton order, de-indexed triangle stream, group boxes */
    float draw_ms;          /* target + one frame, until the raster has finished */
    float gather_ms;        /* swr_present + swr_present_wait: bands -> the caller's images */
    float total_ms;
    int32_t scene_cached;
    int32_t frames;         /* frames the call drew: 1, or 2 when a tile overflowed its bin region and the frame was redrawn (ABI 5;
                               was `reserved`) */
} swr_render_times;
int swr_render_timings(swr_context* ctx, swr_render_times* out);

/* Fault injection for the failure-path tests (tests/test_gpu_api.py, tests/host): the NEXT frame's raster share
 *   SWR_FAULT_LOST_EVENT   waits for a completion that never arrives (the wait budget must end it),
 *   SWR_FAULT_ENQUEUE      fails as if a HIP launch had returned an error.
 * Either way the context ends up failed (see swr_config.wait_budget_ms).  Never needed by a renderer. */
enum { SWR_FAULT_NONE = 0, SWR_FAULT_LOST_EVENT = 1, SWR_FAULT_ENQUEUE = 2 };
int swr_debug_fault(swr_context* ctx, int fault);

/* Test hooks (ABI 5; until round 4 these were environment variables read by the product's hot-path setup): force a code
 * path the library would otherwise choose by itself, for THIS context.  A hook takes effect at the next swr_scene_upload /
 * swr_target_set / swr_render (the stream order, the bin layout, the one-shot threshold) or at the next frame (the others);
 * results never depend on them — every parity test that sets one compares against the oracle.  Never needed by a renderer.
 *   SWR_DEBUG_STREAM_ORDER      1 (default) Morton-ordered triangle stream; 0 keep the caller's primitive order;
 *                               -1 behave as for scenes of >= 2^24 primitives (no reordering, slot == index)
 *   SWR_DEBUG_CULL              1 (default) per-band culling of 64-primitive groups; 0 off
 *   SWR_DEBUG_BIN_MODE          0 (default) fixed-stride bins (the single-launch k_bin) wherever they can hold the scene, exact-size
 *                               bins otherwise; 1 always exact-size bins (four-kernel chain); 2 = 0; 3 global-atomic binning fallback
 *   SWR_DEBUG_ONESHOT_MIN_TRIS  primitives from which a swr_render without a scene identity cuts its index copy in two
 *                               (default 2^18; minimum 64)
 *   SWR_DEBUG_DEPTH_KEYS32      1 (default) depth-only z-tested frames take 32-bit depth keys (k_raster_depth); 0 the 64-bit kernel
 *   SWR_DEBUG_RASTER_SORT       1 (default) such frames sort their bins inside the raster workgroups on small tile grids (thin
 *                               bands), by a k_sort_bins launch on large ones; 0 always the launch; 2 always inside the raster */
enum { SWR_DEBUG_STREAM_ORDER = 1, SWR_DEBUG_CULL = 2, SWR_DEBUG_BIN_MODE = 3, SWR_DEBUG_ONESHOT_MIN_TRIS = 4,
       SWR_DEBUG_DEPTH_KEYS32 = 5, SWR_DEBUG_RASTER_SORT = 6 };
int swr_debug_set(swr_context* ctx, int key, int64_t value);

/* Renderer.render(renderPass:) (Renderer.swift:204-230) and GpuRenderer.render(renderPass:)
 * (GpuRenderer.swift:35-90): caller-owned host memory in, colour + depth images filled on
 * return (synchronous, like scheduleAndWait, Metal+Extensions.swift:57-67). */
int swr_render(swr_context* ctx, const swr_render_pass* pass);

/* ---- resident path: what the app's frame loop does (App.swift:153-185) — same mesh every
 * frame, new transform — without re-uploading; inputs and outputs stay in HBM. ----------- */

/* RenderPass.vertices / .indices (Renderer.swift:195-196); replaces the per-frame
 * makeBuffer / setBytes uploads of GpuRenderer.swift:68-71,93-103.  Validates indices.
 * Also builds the device-side triangle stream once (primitives de-indexed and ordered by the Morton code
 * of their centroid, bounding boxes of 64-primitive groups) — invisible in the image:
 * painter's order and z-tie order always refer to the caller's index order. */
int swr_scene_upload(swr_context* ctx, const swr_vertex* vertices, int64_t vertex_count,
                     const int64_t* indices, int64_t index_count);

/* Fragment-stage extensions on the resident path.  swr_scene_attributes must follow the swr_scene_upload
 * it belongs to (vertex_count must match; a new swr_scene_upload discards the attributes).  The material
 * and the texture persist on the context until replaced; swr_material_set(ctx, NULL) restores the
 * reference's passthrough stage.  A draw with a Phong material but no attributes, or a textured material
 * but no texture, returns SWR_ERR_BAD_ARG. */
int swr_scene_attributes(swr_context* ctx, const swr_vertex_attr* attributes, int64_t vertex_count);
/* Skinned meshes (see "Skinned meshes" above): the per-vertex influences, and the pose the resident scene is put into. */
int swr_scene_skin(swr_context* ctx, const swr_skin_vertex* skin, int64_t vertex_count);
int swr_pose_set(swr_context* ctx, const float* joints /* joint_count x 16, column-major like transform */, int32_t joint_count);
/* joint_count x 8 floats: per joint the real quaternion (x, y, z, w), then the dual quaternion (x, y, z, w); w is the scalar part */
int swr_pose_set_dq(swr_context* ctx, const float* dual_quats, int32_t joint_count);
/* Morph targets (see "Morph targets" above): the targets of the resident scene, and the weights it is morphed by. */
int swr_scene_morph(swr_context* ctx, const swr_morph_targets* targets);                 /* NULL: remove the targets */
int swr_morph_set(swr_context* ctx, const float* weights, int32_t weight_count);         /* NULL, 0: every weight 0 */
/* sparse morph targets ("Sparse morph targets" above); weights and joints in one call ("Weights and joints in one call") */
int swr_scene_morph_sparse(swr_context* ctx, const swr_morph_sparse* targets);           /* NULL: remove the targets */
int swr_morph_pose_set(swr_context* ctx, const float* weights, int32_t weight_count,
                       const float* joints, int32_t joint_count, int32_t pose_kind);
/* computed normals ("Computed normals" above): where the resident scene's normals come from */
int swr_scene_normals(swr_context* ctx, const swr_normals* normals);                     /* NULL: SWR_NORMALS_UPLOADED */
int swr_material_set(swr_context* ctx, const swr_material* material);
int swr_texture_upload(swr_context* ctx, const void* bgra8, int32_t width, int32_t height);
/* The blend state of SWR_FLAG_BLEND frames (see "Alpha blending" above); NULL restores the default, SWR_BLEND_OVER with opacity 255.
 * An opacity outside 0..255, an unknown mode or a non-zero reserved word: SWR_ERR_BAD_ARG, and the state is unchanged.  Frames
 * already posted keep the state they were posted with. */
int swr_blend_set(swr_context* ctx, const swr_blend* blend);

/* colorBuffer / depthBuffer size (Renderer.swift:192-193).  row_begin/row_end select the
 * tile-row band [row_begin,row_end) of the framebuffer this context owns; pass
 * 0,height for the whole image.  row_begin must be a multiple of swr_tile_rows().  A multi-device
 * context cuts [row_begin,row_end) into device_count bands of whole tile rows (like swr_band_rows);
 * a band may be empty when there are more devices than tile rows. */
int swr_target_set(swr_context* ctx, int64_t width, int64_t height,
                   int64_t row_begin, int64_t row_end);

/* One frame: clear + all triangles (Renderer.swift:204-230) into the device-resident band(s).
 * Asynchronous: the call validates its arguments and posts the frame to the context's helper threads, which
 * enqueue it on the HIP streams; swr_sync(), swr_present_wait() or a swr_read_* completes it.  A HIP failure while
 * enqueueing is returned by the next of those blocking calls; on a multi-device context the same holds for an
 * error of the draw itself (no scene, bad index count, ...). */
int swr_draw(swr_context* ctx, const float transform[16], uint32_t flags);
/* Same with RenderPass.primitiveType (Renderer.swift:197, :210-219): .triangle = swr_draw;
 * .vertices plots every vertex reference as a point (Renderer.swift:295-302); .line clears only
 * (the reference's draw(line:) is an empty stub, Renderer.swift:289-293). */
int swr_draw_primitives(swr_context* ctx, const float transform[16], uint32_t flags, int32_t primitive_type);
int swr_sync(swr_context* ctx);
/* The band's current image (what the next SWR_FLAG_LOAD frame starts from) := rows [row_begin,row_end) of the caller's full-size
 * images, per band (a multi-device context: every band its own rows, like swr_present in the other direction).  Everything drawn
 * before is completed and checked first (like swr_sync; its error is returned and nothing is written).  Either pointer may be
 * NULL: that image stays as it is (the cleared one right after swr_target_set).  Page-locked sources go straight to the device,
 * others are staged.  (ABI 6) */
int swr_target_write(swr_context* ctx, const void* color_full_image, const float* depth_full_image);

/* ---- Draw lists: several draws with their own transforms in one frame — DESIGN.md §12 ----------------------------------------
 * No ABI bump (SWR_ABI_VERSION stays 6): nothing existing changes.  The presence of the swr_draw_list symbol is the feature test.
 * One draw item = a range of the uploaded index array drawn with its own transform. */
typedef struct swr_draw_item {
    int64_t first_index;   /* into the uploaded index array; multiple of 3 */
    int64_t index_count;   /* multiple of 3; 0 = an empty draw */
    float   transform[16]; /* column-major, exactly as swr_draw's */
} swr_draw_item;           /* 80 bytes */
#define SWR_DRAW_LIST_MAX 4096
/* One frame of `item_count` draws.  The frame is Renderer.render(renderPass:) over the concatenation of the items: item k contributes
 * the triangles indices[first_index_k, first_index_k + index_count_k), each transformed by transform_k; the primitive order is item
 * order first, then index order inside an item.  So under painter's order a later item covers an earlier one, and under the z-test
 * (strict '<') the earlier item wins a tie.  The image is bit for bit the clear frame (the load frame under SWR_FLAG_LOAD) of the
 * pre-transformed concatenation drawn with the identity, and bit for bit the chain of item_count frames of one item each, the first
 * a clear frame and the others SWR_FLAG_LOAD frames.
 *   Ranges may overlap, repeat and come in any order: one range drawn K times with K matrices is instancing.  item_count == 0 is a
 *     frame without triangles (it clears, or keeps the image under SWR_FLAG_LOAD).
 *   flags apply to the whole frame (SWR_FLAG_DEPTH_TEST, SWR_FLAG_NO_COLOR, SWR_FLAG_METAL_RULES, SWR_FLAG_LOAD); material, vertex
 *     attributes and texture are the context's, as for swr_draw.  Triangles only.
 *   Asynchronous like swr_draw; the list is copied, the caller may overwrite it as soon as the call returns.  A multi-device context
 *     draws the list on every band.  swr_timings.triangles counts the list's total; swr_present / swr_read_* / SWR_ERR_FRAME_DROPPED
 *     behave as for any other frame.
 * Errors: SWR_ERR_INDEX_COUNT — a first_index or index_count that is not a multiple of 3;  SWR_ERR_BAD_ARG — a range outside the
 *   uploaded index array, items == NULL with item_count > 0, item_count < 0;  SWR_ERR_UNSUPPORTED — item_count > SWR_DRAW_LIST_MAX,
 *   or 2^24 triangles or more in the list;  SWR_ERR_NO_SCENE — no scene or no target. */
int swr_draw_list(swr_context* ctx, const swr_draw_item* items, int32_t item_count, uint32_t flags);

/* ---- host-visible frames: the gather ("final image gathered with pinned hipMemcpyAsync") -------------------
 * The reference's images live in CPU/GPU-shared MTLBuffers (App.swift:59-60,80-101) and are complete on return
 * of render (scheduleAndWait, Metal+Extensions.swift:57-67).  Here every band is copied device -> host into its
 * rows of the caller's ONE full-size image; bands are disjoint, so there is nothing to merge.
 *
 * swr_host_alloc / swr_host_free: page-locked host memory every GPU can DMA into — allocate the colour and depth
 *   images with it (what makeBuffer(.storageModeShared) is to the reference).  swr_host_register /
 *   swr_host_unregister page-lock memory the caller already owns.  (Process-wide, no context needed.)
 *
 * swr_present(ctx, color_full, depth_full): enqueue the copy of the frame of the LAST swr_draw — rows
 *   [row_begin,row_end) of each band — into the caller's full-size images and return at once.  Per device: one
 *   hipMemcpyAsync per image, colour and depth in flight together on two copy streams, behind that frame's
 *   raster.  The device framebuffers are double-buffered: the next swr_draw renders into the other one, so the
 *   copy of frame N overlaps the raster of frame N+1.  Either pointer may be NULL (image not wanted; colour is
 *   skipped for SWR_FLAG_NO_COLOR frames).  A destination that is not page-locked still works: it is staged
 *   through pinned 8 MiB chunks by the context's helper thread (or, without helper threads, by the caller).
 * swr_present_wait(ctx): returns when every enqueued copy has landed: the pixels are host-visible.
 *
 * swr_read_color / swr_read_depth: swr_sync + the same copy of one image + wait (rows outside the band(s) are
 *   left untouched).  swr_render = upload + swr_draw + swr_present + swr_present_wait. */
void* swr_host_alloc(size_t bytes);
void  swr_host_free(void* p);
int   swr_host_register(void* p, size_t bytes);
int   swr_host_unregister(void* p);
int swr_present(swr_context* ctx, void* color_full_image, float* depth_full_image);
int swr_present_wait(swr_context* ctx);
int swr_read_color(swr_context* ctx, void* dst_full_image);
int swr_read_depth(swr_context* ctx, float* dst_full_image);
int swr_read_ids(swr_context* ctx, uint32_t* dst_full_image);   /* SWR_FLAG_PRIMITIVE_IDS frames (see "Primitive IDs" above) */
/* Visibility counts (see "Visibility counts" above): swr_sync + a reduction of the ID image on the device + the copy of the n + 1
 * counters + wait.  counts has n elements; none may be NULL. */
int swr_count_ids(swr_context* ctx, const swr_id_count* q, uint32_t* counts, int64_t n, uint32_t* none);
/* Depth queries (see "Depth queries" above): swr_sync + the copy of the n boxes + a reduction of the depth image on the device + the
 * copy of the n counts + wait.  boxes and passed have n elements. */
int swr_query_depth(swr_context* ctx, const swr_depth_box* boxes, int64_t n, uint32_t* passed);
/* Item bounds (see "Item bounds" above): swr_sync + the copy of the items + a reduction of the resident triangle stream on the device +
 * the copy of the item_count records + wait.  items and out have item_count elements. */
int swr_item_bounds(swr_context* ctx, const swr_draw_item* items, int32_t item_count, uint32_t flags, swr_item_bound* out);
/* the nearest hit of each of n rays on the resident triangles (see "Ray casts" above; blocking) */
int swr_cast_rays(swr_context* ctx, const swr_ray* rays, int64_t n, uint32_t flags /* 0 */, swr_ray_hit* hits);
/* swr_cast_rays with occlusion rays, a facing cull and a range of primitives (see "Ray queries" above; blocking) */
int swr_query_rays(swr_context* ctx, const swr_ray_query* query /* NULL: all defaults */, const swr_ray* rays, int64_t n, swr_ray_hit* hits);
/* Delta reads (see "Delta reads" above): swr_sync + the compare against the band's baseline on the device + the copy of the tile
 * flags + the copy of the changed rectangle + wait.  dst is the full W x H image, as for swr_read_*; stats may be NULL. */
int swr_read_color_delta(swr_context* ctx, void*  dst_full_image, swr_delta_stats* stats);
int swr_read_depth_delta(swr_context* ctx, float* dst_full_image, swr_delta_stats* stats);
int swr_delta_reset(swr_context* ctx, uint32_t images);     /* SWR_DELTA_* bits, non-zero, no others: the next delta read is full */
/* Supersampled resolve (see "Supersampled resolve" above): swr_sync + the S x S box filter on the device + the copy of the small
 * image + wait.  The destination has (W/S) x (H/S) elements; page-locked and pageable destinations both work, as for swr_read_*. */
int swr_read_color_resolved(swr_context* ctx, const swr_resolve* resolve, void*  dst);  /* (W/S) x (H/S) BGRA8 */
int swr_read_depth_resolved(swr_context* ctx, const swr_resolve* resolve, float* dst);  /* (W/S) x (H/S) floats */
/* swr_render at S·width x S·height, resolved into the pass's width x height images (both images in one launch per band). */
int swr_render_resolved(swr_context* ctx, const swr_render_pass* pass, const swr_resolve* resolve);
/* swr_render whose gather is the two delta reads into pass->color and pass->depth (see "Delta reads" above).  stats[0] is the colour's,
 * stats[1] the depth's; stats may be NULL. */
int swr_render_delta(swr_context* ctx, const swr_render_pass* pass, swr_delta_stats stats[2]);

/* Timing instrumentation: hipEvents on the context stream.  level 0 = off, 1 = two events around
 * the dominant kernel (k_raster) only, 2 = around every stage (each event costs a few us of
 * stream time, so level 2 perturbs the frame it measures). */
int swr_timing_enable(swr_context* ctx, int level);
/* Level 1 only: bracket the k_raster of every n-th frame instead of every frame (default 1).  An event pair on
 * the raster stream is a synchronisation point that costs a pipelined 4K frame about 15 us; sampling keeps the
 * measurement live inside a timed region without slowing every frame of it.  swr_timing_totals' frame count is
 * the number of frames actually bracketed. */
int swr_timing_sample(swr_context* ctx, int every_nth);
int swr_get_timings(swr_context* ctx, swr_timings* out);          /* the last frame */
/* Sums over every frame drawn since swr_timing_reset (events are kept in a ring, so a whole
 * timed region of frames is measured without a host sync per frame). */
int swr_timing_totals(swr_context* ctx, swr_timings* sum_out, int64_t* frames_out);
int swr_timing_reset(swr_context* ctx);

/* Frame pipelining (on by default): the binning kernels of the next swr_draw run on a second stream,
 * over a triple-buffered working set, while the previous frame is still being rasterised.  Results
 * are identical either way; 0 serialises the two stages on one stream (clean per-stage timings). */
int swr_pipeline_enable(swr_context* ctx, int enable);

/* Tile geometry the band boundaries must respect. */
int swr_tile_rows(void);
int swr_tile_cols(void);

/* Helper: split `height` rows into `parts` contiguous bands aligned to swr_tile_rows();
 * writes row_begin/row_end of band `part`.  Pure host arithmetic (no device needed). */
int swr_band_rows(int64_t height, int32_t parts, int32_t part,
                  int64_t* row_begin, int64_t* row_end);

#ifdef __cplusplus
}
#endif
#endif /* SWR_H_ */
