// swr_internal.h — structures shared between the HIP kernels (swr_kernels.hip) and the C-ABI
// host code (swr_api.hip).  Nothing here is part of the public boundary (include/swr.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "../../include/swr.h"

namespace swr {

// Screen-space tile owned by one workgroup of the raster kernel.  The per-pixel visibility
// key tile (8 B/pixel) lives in LDS: 64x32 -> 16 KiB, i.e. up to 8 workgroups per CU by LDS.
constexpr int TILE_W = 64;
constexpr int TILE_H = 32;
constexpr int RASTER_THREADS = 256;

// Per-triangle record written by the setup kernel and gathered by the raster kernel:
// 32 bytes = 2 x 16-byte loads.  B and C are stored relative to A as int16, which is exact for
// every GEOM_SMALL triangle (bbox extents < 2^15); the rare others keep their absolute
// coordinates in GeomFull.  T() is recomputed from the integer vertices where it is needed (same
// expressions -> same bits), so it does not travel through HBM.
struct GeomRec {
    int32_t ax, ay;                // truncated screen vertex A (Renderer.swift:251)
    int16_t dbx, dby;              // B - A
    int16_t dcx, dcy;              // C - A
    float za, zb, zc;              // NDC z of a,b,c (Renderer.swift:254-256)
    uint32_t flags;                // GEOM_* below
};
static_assert(sizeof(GeomRec) == 32, "GeomRec must be 32 bytes");

// Absolute integer vertices, written and read only for triangles without GEOM_SMALL.
struct GeomFull {
    int32_t ax, ay, bx, by, cx, cy, pad0, pad1;
};
static_assert(sizeof(GeomFull) == 32, "GeomFull must be 32 bytes");

enum : uint32_t {
    GEOM_VALID = 1u << 0,
    GEOM_SMALL = 1u << 1,          // bbox extents < 2^15 (in y: < 2^15 - TILE_H, setup_triangle_r): int16 deltas and 32-bit span arithmetic are exact
    GEOM_ORD_SHIFT = 2,            // 3 x 2 bits: which of a,b,c is S0,S1,S2 of the y-sorted list (:271)
    GEOM_ORIG_SHIFT = 8            // bits 8..31: the primitive's ORIGINAL index (scenes below 2^24 primitives;
                                   // larger scenes are not reordered, so slot == original index)
};
constexpr int64_t SORT_MAX_TRIS = 1ll << 24;

struct Target {
    int32_t width, height;         // full framebuffer
    int32_t row_begin, row_end;    // band owned by this context
    int32_t tiles_x, tiles_y;      // tiles in the band
};

// device-side frame counters (one 32-bit word each)
enum { CNT_PAIRS = 0, CNT_OVERFLOW = 1, CNT_BAD_INDEX = 2, CNT_WORDS = 8 };

// One item of a draw-list frame on the device (swr_draw_item, resolved by the host).  Item k draws the scene primitives
// [first, first + count) — in a segmented stream (swr_upload.hip) also the stream slots [first, first + count) — into the frame slots
// [vbase, vbase + count); its k_bin work units are [ubase, ubase + groups of 64 stream slots it touches).  The order number of
// primitive o of the item (GeomRec.flags, the visibility keys) is vbase + o - first.
struct ListItem {
    uint32_t first, count, vbase, ubase;
    float m[16];                   // column-major, as swr_draw's
};
static_assert(sizeof(ListItem) == 80, "ListItem must be 80 bytes");
constexpr int LIST_ITEM_BITS = 12;  // k_bin<.., LIST> packs (item, group of the item) into 32 bits: item < SWR_DRAW_LIST_MAX = 2^12
static_assert(SWR_DRAW_LIST_MAX <= (1 << LIST_ITEM_BITS), "item ids must fit the packed work unit");

// Depth clipping (SWR_FLAG_DEPTH_CLIP, swr_clip.hip): the per-frame pre-pass that turns the submitted triangles (n of them: the
// scene's, or a draw list's order numbers) into the frame's own stream of 3n slots — the post-clip triangles in NDC, slot = order
// number, the rest marked invalid — which the frame then bins and rasters with the identity transform.
struct ClipPrep {
    const float4* src_xyz;         // the scene's triangle stream (DeviceFrame::tri_xyz / tri_rgb / tri_nrm / inv / reordered)
    const float4* src_rgb;
    const float4* src_nrm;         // NULL: the scene has no attributes
    const uint32_t* src_inv;
    int32_t src_reordered;
    int64_t n;                     // submitted triangles
    int64_t bound;                 // frame slots: n + 2 x the fan capacity, at most 3n (0: not a clip frame)
    float m[16];                   // swr_draw's transform (draw lists: the items' own)
    const ListItem* items;         // draw lists: the frame's items on the device (else NULL)
    int32_t nitems;
    uint32_t* sums;                // [ceil(n / 256) + 1] fan triangles per pre-pass workgroup -> their exclusive offsets + the total
    float4* xyz; float4* rgb; float4* nrm;   // [3 * bound] the frame's stream (nrm NULL without attributes)
    uint32_t* map;                 // [bound] order number -> original number (the ID image)
    float4* box;                   // [2 * ceil(bound / 64)] box of every 64-slot group
    uint32_t* over;                // device-visible pinned word of the frame: the post-clip count if it exceeded `bound`, else 0
    float4* pq;                    // [bound] perspective frames (DeviceFrame::pq): (q_a, q_b, q_c, bypass) of every fan triangle, else NULL
    int32_t count_only;            // launch_bin: only the count and its scan (sums[ceil(n / 256)] = the post-clip count), no frame
};

// Geometry of the LDS binning path (see plan_binning in swr_kernels.hip).
struct BinPlan {
    bool use_lds;
    int threads;        // workgroup size of the two binning walks
    int G;              // workgroups = rows of the count matrix
    int chunk;          // primitives per workgroup
    size_t lds_bytes;   // tiles * 4
};
BinPlan plan_binning(int64_t ntri, int ntiles, bool force_atomic);
int live_groups_per_workgroup(int64_t ntri, int G);

// Everything one frame needs, all device pointers.  colour/depth are band-local: element
// (x, y) of the full image lives at [(y - row_begin) * width + x].
struct DeviceFrame {
    const swr_vertex* vertices;    // as uploaded (AoS)
    const int64_t* indices;
    // the triangle stream (swr_upload.hip): primitives in Morton order of their centroid, de-indexed
    const float4* tri_xyz;         // [ni] corner positions; w of corner 0 = original primitive index (bits)
    const uint32_t* inv;           // [ntri] sorted slot of original primitive o
    const float4* box64;           // [2 * ceil(ntri/64)] object-space min / max of each 64-slot group
    int32_t reordered;             // 1: slots are a permutation (original index in GeomRec.flags); 0: slot == index
    const float4* tri_rgb;         // [ni] colours per slot corner (48 B / triangle); lane 3 = v
    const float4* tri_nrm;         // [ni] (nx,ny,nz,u) per primitive corner (extended fragment stage)
    swr_material material;         // shader == SWR_SHADER_PASSTHROUGH: the reference's stage
    const float4* texels;          // texture of swr_texture_upload, converted to (r,g,b,a) floats
    int32_t tex_w, tex_h;
    int64_t vertex_count;
    int64_t index_count;           // (.vertices / .line passes: ntri = index_count / 3 is the triangle count only)
    int64_t ntri;
    GeomRec* geo;
    GeomFull* geo_full;
    uint32_t* tile_count;          // [tiles] (triangle,tile) pairs per tile
    uint32_t* tile_start;          // [tiles+1] exclusive scan of tile_count
    uint32_t* counters;            // [CNT_WORDS]
    uint32_t* host_counters;       // device-visible address of the pinned host copy
    uint32_t* host_max;            // pinned host word: entries of the frame's fullest bin (written by k_fill_lds; may be NULL)
    int32_t insort;                // 1: k_raster_depth sorts every bin itself (no k_sort_bins launch for this frame)
    int32_t k32;                   // 1: depth-only z-tested frames take the 32-bit depth keys (k_raster_depth)
    uint32_t* redo_dev;            // device word: tiles k_raster_depth had to raster again (sampled)
    uint32_t* host_redo;           // pinned host word that receives it: at the end of a launch's first workgroup, what was counted up to then
    int32_t defer_big;             // 1: the previous frame had triangles for the deferred list (k_bin<DEFER>)
    int32_t skip_sort;             // 1: no k_sort_bins for this frame (every bin of the previous frames fitted two chunks)
    uint32_t* tile_cursor;         // [tiles] running fill position (starts as tile_start)
    uint2* ranges;                 // [ntri] band-clipped pixel bbox (x0|x1<<16, y0|y1<<16, y band-relative)
    uint32_t* bins;                // [capacity] primitive ids grouped by tile (exact bins) / [tiles * cap_tile] (fixed-stride bins)
    // fixed-stride bins (k_bin, one launch): tile t owns bins[t * cap_tile, +fill[CNT_WORDS + t])
    int32_t fixed_bins;            // 1: this frame is binned by k_bin
    uint32_t cap_tile;             // entries per tile region
    uint32_t* fill;                // [CNT_WORDS counters][tiles] of this frame, zero when k_bin starts
    uint32_t* fill_next;           // the next frame's block (k_bin zeroes it)
    uint32_t* host_fill;           // pinned host word: the frame's largest fill (overflow test)
    uint4* biglist;                // [1024] triangles of the frame that cover too many tiles to be scattered by k_bin: k_sort_bins appends them per tile
    uint32_t* bin_matrix;          // [G][tiles] per-workgroup tile counts -> prefixes (LDS path)
    uint32_t* live;                // [G][1 + ceil(groups/G)] per binning workgroup: count + the stream groups that survived its cull
    int32_t live_parity;           // >= 0: cull the groups against the band; -1: every group is live
    BinPlan plan;
    uint32_t capacity;
    uint8_t* color;
    float* depth;
    const uint8_t* src_color;      // load frames (SWR_FLAG_LOAD): the framebuffer the frame starts from (never color / depth)
    const float* src_depth;
    uint32_t* ids;                 // SWR_FLAG_PRIMITIVE_IDS frames: the ID image, band-local like depth (else NULL)
    Target tg;
    float m[16];                   // column-major transform
    uint32_t flags;                // SWR_FLAG_*
    // draw-list frames (swr_draw_list): NULL for every other frame.  ntri is then the list's total V; geo / geo_full /
    // ranges / bins hold FRAME slots, and tri_rgb / tri_nrm / inv the frame's own per-slot copies (k_list_gather).
    const ListItem* items;         // [nitems] on the device
    int32_t nitems;
    int64_t units;                 // (item, 64-slot stream group) work units of k_bin<.., LIST>
    int32_t list_affine;           // every item's transform has the last row (0, 0, 0, 1): k_bin<.., AFF, LIST>
    // inv_out != NULL: the binning launch first gathers the frame's own per-slot tables (k_list_gather) from the scene's
    struct { const float4* rgb; const float4* nrm; float4* rgb_out; float4* nrm_out; uint32_t* inv_out; } gather;
    // depth-clip frames (SWR_FLAG_DEPTH_CLIP): clip.bound > 0; ntri = clip.bound, tri_xyz / tri_rgb / tri_nrm / box64 = the clip
    // stream, m = identity, not reordered, not a list (a clipped draw list is a plain frame over its clip stream)
    ClipPrep clip;
    int64_t order_space;           // > 0: the frame's order numbers lie below this (the PLAIN / winner-table switch); 0: ntri
    // SWR_FLAG_PERSPECTIVE colour frames through a non-affine transform: [ntri] per slot the raster sees, (q_a, q_b,
    // q_c, bypass) — filled in front of the binning (k_persp_fill; depth-clip frames: k_clip_emit); NULL: the screen weights
    float4* pq;
    // SWR_FLAG_BLEND frames: the blend state as it was when the frame was posted (launch_raster: k_raster_blend)
    swr_blend blend;
};

// with_bools(fn, b0, b1, ...) calls fn(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): runtime bools become template
// arguments.  fn is a generic lambda, `[&](auto LOAD, auto IDS) { ... k_x<LOAD, IDS> ... }`; its body is instantiated for all 2^N
// combinations, so every template-id it names with a lifted parameter exists for both values of it.
template <class F>
decltype(auto) with_bools(F&& fn) { return fn(); }
template <class F, class... Rest>
decltype(auto) with_bools(F&& fn, bool b0, Rest... rest) {
    return b0 ? with_bools([&](auto... c) -> decltype(auto) { return fn(std::true_type{}, c...); }, rest...)
              : with_bools([&](auto... c) -> decltype(auto) { return fn(std::false_type{}, c...); }, rest...);
}

#ifdef __HIPCC__   // (the host layer's stand-alone tests compile swr_api.hip against a fake runtime that has no kernels to launch)
// Launch with the completion of the kernel bound to `stop` when there is one (hipExtLaunchKernelGGL: the event is the kernel's own
// completion signal — no marker packet behind the kernel, which would cost the next kernel of the queue ~6.5 us).  Returns whether
// the kernel carries the event.
template <class Kernel, class... Args>
bool launch_on(hipEvent_t stop, Kernel k, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args&&... args) {
    if (stop) hipExtLaunchKernelGGL(k, grid, block, (uint32_t)lds, s, nullptr, stop, 0, std::forward<Args>(args)...);
    else hipLaunchKernelGGL(k, grid, block, (uint32_t)lds, s, std::forward<Args>(args)...);
    return stop != nullptr;
}
#endif

void launch_validate_indices(const int64_t* indices, int64_t count, int64_t vertex_count,
                             uint32_t* counters, hipStream_t s);
hipError_t prepare_device();      // per-device kernel attributes (after hipSetDevice)

// swr_upload.hip: the once-per-scene triangle stream
struct StreamBuild {
    const swr_vertex* vertices; int64_t nv;
    const int64_t* indices; int64_t ntri;
    bool sort;                     // false: identity order (scenes of 2^24 primitives or more, or SWR_SORT=0)
    uint32_t* scratch;             // 4 * ntri + 8 words
    void* sort_temp; size_t sort_temp_bytes;
    float4* tri_xyz; float4* tri_rgb; uint32_t* inv; float4* box64;
    const uint32_t* cuts;          // draw lists: [ncuts] sorted primitive indices the stream is cut at (sorted by (segment, Morton code))
    int ncuts;
};
size_t stream_sort_temp_bytes(int64_t ntri);
hipError_t launch_build_stream(const StreamBuild& b, hipStream_t s);
hipError_t launch_build_stream_range(const StreamBuild& b, int64_t t0, int64_t t1, hipStream_t s);   // index order, primitives [t0, t1)
void launch_gather_attrs(const swr_vertex_attr* attrs, int64_t nv, const int64_t* indices, int64_t ntri,
                         const float4* tri_xyz, float4* tri_nrm, float4* tri_rgb, hipStream_t s);
void launch_texture_to_float(const uint32_t* bgra, int64_t n, float4* out, hipStream_t s);
uint32_t fixed_cap_max(int64_t ntri, int ntiles);   // largest tile region k_bin can fill (0: the frame needs the exact-size path)
bool launch_bin(const DeviceFrame& f, hipStream_t s, hipEvent_t stop = nullptr);
void launch_setup_bin(const DeviceFrame& f, hipStream_t s);
void launch_scan(const DeviceFrame& f, hipStream_t s);
// stop != NULL: the event is bound to the (last) kernel launched, as its completion (launch_on); returns whether a kernel carries it
bool launch_fill(const DeviceFrame& f, hipStream_t s, hipEvent_t stop = nullptr);
bool launch_sort_bins(const DeviceFrame& f, hipStream_t s, hipEvent_t stop = nullptr);
bool launch_raster(const DeviceFrame& f, hipStream_t s, hipEvent_t stop = nullptr);
bool frame_uses_k32(const DeviceFrame& f);   // the frame's raster is k_raster_depth (32-bit depth keys, sorts its bins itself)
void launch_points_or_lines(const DeviceFrame& f, int primitive_type, hipStream_t s);

// swr_clip.hip: the clip pre-pass in front of a clip frame's binning (launch_bin / launch_setup_bin start with it) and the ID map
// behind its raster (launch_raster ends with it, carrying `stop`)
void launch_clip_prep(const DeviceFrame& f, hipStream_t s);
bool launch_clip_ids(const DeviceFrame& f, hipStream_t s, hipEvent_t stop);

// swr_resolve.hip: the S x S box filter of a supersampled band: `rows` source rows of `width` pixels (multiples of
// factor, 2 or 4) -> width / factor x rows / factor pixels; a NULL source image is not resolved
void launch_resolve(const void* color, const void* depth, void* color_out, void* depth_out, int width, int rows, int factor,
                    int depth_filter, hipStream_t s);

// swr_count.hip: visibility counts: the rectangle [x0, x1) x [y0, y1), band-local rows, of the band's ID image `ids`
// (`width` words per row) into counters[0 .. n], zeroed by the caller on the same stream — counters[n] counts SWR_ID_NONE; per_item:
// counters[k] the IDs of item k of `items` (n items; NULL: one item that holds every ID), else counters[p] the ID p
void launch_count_ids(const uint32_t* ids, int width, int x0, int x1, int y0, int y1, int per_item, const ListItem* items,
                      uint32_t* counters, int64_t n, hipStream_t s);

// swr_depth_query.hip: depth queries: passed[k] = the pixels of boxes[k] (full-target coordinates, already checked),
// clipped to the band's rows [row_begin, row_begin + rows), with boxes[k].z < depth — the band's depth image, `width` floats per row.
// Every passed[0 .. n) is written, by plain stores; nothing has to be zeroed.  `large` lists the nlarge boxes whose part in the band
// holds at least DEPTH_QUERY_SPLIT_AREA pixels (ascending box indices, duplicates of a box are separate entries): their tiles are
// split across workgroups.  total_area is the sum of the boxes' parts in the band, in pixels: a query far smaller than the band is
// scanned directly, without the tile summary.  `scratch` holds the summary: depth_query_scratch_bytes(width, rows) bytes.
// boxes, large, scratch and passed are device memory.
constexpr uint32_t DEPTH_QUERY_SPLIT_AREA = 1u << 17;
inline size_t depth_query_scratch_bytes(int width, int rows) {      // (16 bytes per tile of 64 columns x at least 8 rows)
    return (size_t)((width + 63) / 64) * (size_t)((rows + 7) / 8) * 16;
}
void launch_depth_query(const float* depth, int width, int rows, int row_begin, const swr_depth_box* boxes, int64_t n,
                        const uint32_t* large, int64_t nlarge, uint64_t total_area, void* scratch, uint32_t* passed, hipStream_t s);

// swr_delta.hip: delta reads.  launch_delta compares the band's image `cur` (`width` words per row, `rows` rows) with
// its baseline `base`, tile by tile (64 x 32, row-major, ceil(width / 64) per row): flags[t] = 1 where tile t differs in any bit, else
// 0 — every word of the table is written by a plain store, nothing has to be zeroed — and the changed tiles' words are stored into
// `base`.  have_base == 0: nothing is compared, every tile is stored and flagged (the copy of the band into a fresh baseline).
// direct: NULL, or the band's rows of a page-locked host image as the device sees them (hipHostGetDevicePointer): the changed tiles'
// words are stored there too.  launch_delta_pack gathers columns [x0, x1) of the band-local rows [y0, y1) of `src` into `out`, rows of
// x1 - x0 words.  cur, base, flags, src and out are device memory.
void launch_delta(const uint32_t* cur, uint32_t* base, int have_base, int width, int rows, uint32_t* flags, uint32_t* direct, hipStream_t s);
void launch_delta_pack(const uint32_t* src, int width, int x0, int x1, int y0, int y1, uint32_t* out, hipStream_t s);

// swr_skin.hip: skinned meshes.  launch_skin_vertices poses the nv vertices — posed[i] = the blend of include/swr.h
// "Skinned meshes" of vertices[i] with its colour copied, posed_nrm[i] = (the blended normal of attrs[i], 0) — from `joints`, the
// pose on the device: joint_count matrices of 16 floats, column-major.  attrs == NULL: the scene has no attributes and posed_nrm is
// not written.  Every joint index of `skin` is below joint_count (the host has checked it).
// launch_skin_stream rewrites the positions of the scene's triangle stream from a vertex array — the xyz lanes of tri_xyz[3s + k] =
// those of pos[pos_stride * index], in float4 units; the w lanes stay — and, nrm != NULL, the xyz lanes of tri_nrm[3s + k] from
// nrm[nrm_stride * index], and writes the box of every 64-slot group as k_box64 does.  The primitive of slot s is tri_xyz[3s].w when
// `reordered`, else s.  Given the posed arrays (strides 2 and 1) the stream is in the pose; given the scene's own vertices and
// attributes (strides 2 and 2) it is bit for bit the stream the upload built.  All pointers are device memory.
void launch_skin_vertices(const swr_vertex* vertices, const swr_vertex_attr* attrs, const swr_skin_vertex* skin, int64_t nv,
                          const float* joints, int32_t joint_count, swr_vertex* posed, float4* posed_nrm, hipStream_t s);
void launch_skin_stream(const float4* pos, int pos_stride, const float4* nrm, int nrm_stride, int64_t nv, const int64_t* indices,
                        int64_t ntri, int reordered, float4* tri_xyz, float4* tri_nrm, float4* box64, hipStream_t s);

// swr_morph.hip: morph targets.  The deltas live on the device as target-major planes of SWR_TUNE_MORPH_PAD ? 4 : 3
// floats per vertex (the swr_api.hip upload packs them so): dpos[(target * nv + i) * floats ..], and dnrm the same.  `list` holds the
// `active` targets whose weight is not zero, ascending, on the device.  launch_morph_vertices writes morphed[i] = vertices[i] with
// p = p + weight * dpos[target][i] applied per list entry in order (include/swr.h "Morph targets"), colour and padding lanes copied,
// and, attrs != NULL (then dnrm != NULL), morphed_attrs[i] = attrs[i] with the normal taken through the same loop over dnrm, uv
// copied.  Every target of the list is below the resident target count (the host built the list).  All pointers are device memory.
#ifndef SWR_TUNE_MORPH_PAD
#define SWR_TUNE_MORPH_PAD 0       // deltas as 12 bytes per vertex and target (0) or as padded float4 (1): DESIGN.md §24 has the measurement
#endif
struct MorphEntry { uint32_t target; float weight; };
void launch_morph_vertices(const swr_vertex* vertices, const swr_vertex_attr* attrs, int64_t nv, const float* dpos, const float* dnrm,
                           const MorphEntry* list, int32_t active, swr_vertex* morphed, swr_vertex_attr* morphed_attrs, hipStream_t s);

// swr_item_bounds.hip: item bounds.  records[k] = the swr_item_bound of items[k] (include/swr.h "Item bounds") over the
// stream slots [first, first + count) of tri_xyz — the item's triangles, the stream being cut at the item's boundaries — through the
// item's own matrix, on a width x height target; metal: the Metal rules.  Item k's work units are [ubase, ubase + ceil(count /
// ITEM_BOUNDS_CHUNK)), `units` in all (an empty item has none; vbase is not read).  The workgroups of an item fold into
// ITEM_BOUNDS_SLOTS partial records of 64 bytes in `scratch` (item_bounds_scratch_bytes(n) bytes), which the launch initialises itself
// and folds into records[k] at its end: nothing has to be zeroed.  tri_xyz, items, scratch and records are device memory.
// (vertices / indices: the vertex array in effect and the index array, read only by the SWR_TUNE_ITEM_BOUNDS = 1 A/B build, which
// gathers the item's triangles through them, first and count then being primitive numbers, instead of walking the stream)
#ifndef SWR_TUNE_ITEM_BOUNDS_CHUNK
#define SWR_TUNE_ITEM_BOUNDS_CHUNK 2048     // stream slots per work unit, a multiple of 256: DESIGN.md §25 has the measurement
#endif
constexpr int ITEM_BOUNDS_CHUNK = SWR_TUNE_ITEM_BOUNDS_CHUNK;
#ifndef SWR_TUNE_ITEM_BOUNDS_SLOTS
#define SWR_TUNE_ITEM_BOUNDS_SLOTS 32       // partial records per item the workgroups' atomics are spread over: DESIGN.md §25
#endif
constexpr int ITEM_BOUNDS_SLOTS = SWR_TUNE_ITEM_BOUNDS_SLOTS;
inline size_t item_bounds_scratch_bytes(int64_t n) { return (size_t)n * (size_t)ITEM_BOUNDS_SLOTS * 64; }
struct ItemBoundsArgs {
    const float4* tri_xyz;
    const swr_vertex* vertices;
    const int64_t* indices;
    const ListItem* items;
    int32_t n;
    int32_t width, height;
    int32_t metal;
    int64_t units;
    void* scratch;
    swr_item_bound* records;
};
inline int64_t item_bounds_units(uint32_t count) { return ((int64_t)count + ITEM_BOUNDS_CHUNK - 1) / ITEM_BOUNDS_CHUNK; }
void launch_item_bounds(const ItemBoundsArgs& a, hipStream_t s);

// swr_skin_dq.hip: dual-quaternion skinning.  launch_skin_vertices_dq is launch_skin_vertices with the blend of
// include/swr.h "Dual-quaternion skinning": the same arrays in, the same posed arrays out, launch_skin_stream follows it.  `dual_quats`
// is the pose on the device: joint_count x 8 floats, per joint the real quaternion (x, y, z, w), then the dual quaternion, 16-byte
// aligned.  Every joint index of `skin` is below joint_count (the host has checked it).
void launch_skin_vertices_dq(const swr_vertex* vertices, const swr_vertex_attr* attrs, const swr_skin_vertex* skin, int64_t nv,
                             const float* dual_quats, int32_t joint_count, swr_vertex* posed, float4* posed_nrm, hipStream_t s);

// swr_morph_sparse.hip: sparse morph targets.  The targets live on the device as vertex-major rows over the TOUCHED
// vertices, the union of the targets' index lists: touched[r] is the vertex of row r, ascending; row[r] .. row[r + 1] are its entries
// in dpos (and, in step, dnrm), sorted by target.  weights holds one weight per resident target (`targets` of them, at most
// SWR_MORPH_MAX_TARGETS).  launch_morph_sparse writes, for every touched vertex i, the xyz and padding lanes of morphed[i] = those of
// vertices[i] with p = p + weight * delta applied per row entry whose weight is not zero, in row order (include/swr.h "Sparse morph
// targets"), and, attrs != NULL (then dnrm != NULL), the normal and padding lanes of morphed_attrs[i] from attrs[i] through the same
// loop over dnrm.  Nothing else is written: the host pre-fills morphed and morphed_attrs with the base arrays, so the colour and uv
// lanes and every untouched vertex are already there.  touched_count >= 1; every entry's target is below `targets` and every touched
// vertex below the scene's vertex count (the host built the rows).  All pointers are device memory.
struct MorphSparseEntry { uint32_t target; float dx, dy, dz; };
static_assert(sizeof(MorphSparseEntry) == 16, "one 16-byte load per entry");
struct MorphSparseArgs {
    const swr_vertex* vertices;
    const swr_vertex_attr* attrs;
    const uint32_t* touched;           // [touched_count]
    const int64_t* row;                // [touched_count + 1]
    const MorphSparseEntry* dpos;      // [row[touched_count]]
    const MorphSparseEntry* dnrm;      // the same shape, or NULL
    const float* weights;              // [targets]
    int64_t touched_count;
    int32_t targets;
    swr_vertex* morphed;
    swr_vertex_attr* morphed_attrs;
};
void launch_morph_sparse(const MorphSparseArgs& a, hipStream_t s);

// swr_normals.hip: computed normals.  launch_face_normals writes face[p] = (f_p, 0) of include/swr.h "Computed
// normals" for the ntri triangles of `indices`, from the vertex array in effect — the pos, pos_stride pair launch_skin_stream takes;
// flip: SWR_NORMALS_FLIP.  launch_vertex_normals writes auto_nrm[i] = (n_i, 0) for the nv vertices: the faces of row i of the
// adjacency added in row order, then normalised.  adj_off[nv + 1] are the row bounds, adj_tri[adj_off[nv]] the triangle of every
// corner that names the vertex, ascending by corner number 3p + k, duplicates kept (the host built it: swr_scene_normals); every
// entry is below ntri.  launch_skin_stream, given auto_nrm with stride 1, then writes the stream.  launch_flat_normals writes the xyz
// lanes of tri_nrm[3s + k], k = 0..2, = f of the xyz lanes of tri_xyz[3s .. 3s + 2] for the ntri slots of the stream (after
// launch_skin_stream has written its positions); the w lanes stay.  All pointers are device memory.
void launch_face_normals(const float4* pos, int pos_stride, int64_t nv, const int64_t* indices, int64_t ntri, bool flip, float4* face,
                         hipStream_t s);
void launch_vertex_normals(const uint32_t* adj_off, const uint32_t* adj_tri, const float4* face, int64_t nv, float4* auto_nrm,
                           hipStream_t s);
void launch_flat_normals(const float4* tri_xyz, int64_t ntri, bool flip, float4* tri_nrm, hipStream_t s);

// swr_rays.hip: ray casts.  hits[k] = the swr_ray_hit of rays[k] (include/swr.h "Ray casts") over the ntri slots of
// tri_xyz, with box64 — the box of every 64-slot group, `groups` = ceil(ntri / 64) of them — as the cull.  The primitive of slot s is
// tri_xyz[3s].w when `reordered`, else s; inv[p] is then the slot of primitive p (not read otherwise).  One workgroup per (ray,
// chunk of RAYS_GROUPS_PER_WG groups) combines into keys[k], one 64-bit word per ray, which the launch initialises itself and decodes
// into hits[k] at its end: nothing has to be zeroed.  Every ray has been checked by the host.  ntri == 0: every ray misses.  All
// pointers are device memory.
// Ray queries (include/swr.h "Ray queries") ride on the same launch: `flags` are the query's SWR_RAYS_* bits and
// [p_begin, p_end) its range of primitives, 0 <= p_begin <= p_end <= ntri, resolved by the host.  ntri and groups stay those of the
// whole stream: the range is a predicate per triangle.  flags 0 with the range [0, ntri) is swr_cast_rays itself.
#ifndef SWR_TUNE_RAYS_GROUPS_PER_WG
#define SWR_TUNE_RAYS_GROUPS_PER_WG 1024    // group boxes per workgroup, a multiple of 256: DESIGN.md §30
#endif
constexpr int RAYS_GROUPS_PER_WG = SWR_TUNE_RAYS_GROUPS_PER_WG;
struct RaysArgs {
    const float4* tri_xyz;
    const float4* box64;
    const uint32_t* inv;
    int32_t reordered;
    int64_t ntri;
    int64_t groups;
    const swr_ray* rays;
    int64_t n;
    unsigned long long* keys;
    swr_ray_hit* hits;
    uint32_t flags;
    int64_t p_begin;
    int64_t p_end;
};
inline int64_t rays_chunks(int64_t groups) { return (groups + RAYS_GROUPS_PER_WG - 1) / RAYS_GROUPS_PER_WG; }
void launch_cast_rays(const RaysArgs& a, hipStream_t s);

}  // namespace swr
