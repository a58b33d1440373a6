// swr_rules.hip.h — the arithmetic rules that several kernels must agree on bit for bit, one definition each.
//
// Device code only: included by the .hip kernel files, never by the host layer (swr_api.hip).  A kernel that needs one of these rules
// includes it from here; a second spelling of a rule anywhere under csrc/ fails tests/test_shared_rules.py.
// The frame kernels of swr_kernels.hip must keep their machine code (tools/kernel_diff.py), and three places there move it under any
// form of the call, so they restate a rule in their own statement order and say so: setup_triangle_r the skip rule
// (screen_vertices_ok; it takes the map from screen_vertex), k_points and k_lines the map (they take the skip rule from here).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "swr_internal.h"
#include "swr_shaders.hip.h"

namespace swr {

// ---- vertex -> screen ------------------------------------------------------------------------------------------------------------
// 2^30: a triangle with a screen coordinate at or beyond it (or a non-finite one: Swift's Int(NaN) would trap) is skipped, the same
// skip rule as the oracle.  Below it the truncated coordinates' deltas stay below 2^31.
constexpr float COORD_LIMIT = 1073741824.0f;

struct ScreenVertex { float sx, sy, sz, w; };       // screen x, y in pixels (before truncation), NDC z, clip-space w

// Vertex.apply(transform:) (Renderer.swift:159-163) through the vertex_shader hook, then convertedToScreen (:165-171).
// MT = the Metal rules: vertex_pass snaps, pixels = round(uv * screen) (Shaders.metal:71), half away from zero like Metal's round().
// AFF = the transform's last row is (0, 0, 0, 1): w is exactly 1 for every finite vertex and x / 1 = x, so the divisions are skipped.
// Colours pass through vertex_shader untouched (Shaders.metal:53) and are not needed here.  (The statement order is setup_triangle_r's: both products after both sums.)
template <bool MT, bool AFF = false>
__device__ __forceinline__ ScreenVertex screen_vertex(float3 xyz, const float4x4& M, float fw, float fh) {
    const VertexOut vo = vertex_shader(xyz, make_float3(0, 0, 0), M);
    const float nx = AFF ? vo.pos.x : vo.pos.x / vo.pos.w;
    const float ny = AFF ? vo.pos.y : vo.pos.y / vo.pos.w;
    const float nz = AFF ? vo.pos.z : vo.pos.z / vo.pos.w;
    const float u = nx * 0.5f + 0.5f;
    const float v = ny * -0.5f + 0.5f;
    ScreenVertex s;
    s.sx = u * fw;
    s.sy = v * fh;
    s.sz = nz;
    s.w = vo.pos.w;
    if (MT) { s.sx = roundf(s.sx); s.sy = roundf(s.sy); }
    return s;
}

// The skip rule over the N vertices of a primitive: every coordinate inside the limit (false for NaN and infinities), and, under the
// Metal rules, none negative: uint2(pos.xy) (Shaders.metal:102-104) is undefined for a negative coordinate.
template <bool MT, int N>
__device__ __forceinline__ bool screen_vertices_ok(const float* sx, const float* sy) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; k++) ok = ok && (fabsf(sx[k]) < COORD_LIMIT) && (fabsf(sy[k]) < COORD_LIMIT);
    if (MT) {
#pragma unroll
        for (int k = 0; k < N; k++) ok = ok && (sx[k] >= 0.0f) && (sy[k] >= 0.0f);
    }
    return ok;
}

// ---- the monotone float <-> uint map ---------------------------------------------------------------------------------------------
// Negative floats reversed, positive ones offset: monotone for every non-NaN float, -0 below +0.  An integer min / max (in LDS, by
// atomics) over the mapped values is the float's, exactly and whatever the order: the visibility keys, the scene bounds of the upload,
// the depth range of item bounds.
__device__ __forceinline__ uint32_t orderable_depth(float d) {
    uint32_t u = __float_as_uint(d);
    return u ^ (uint32_t)(((int32_t)u >> 31) | 0x80000000);
}
__device__ __forceinline__ float depth_from_orderable(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    return __uint_as_float(u);
}

// ---- wave64 reductions -----------------------------------------------------------------------------------------------------------
// Butterfly over xor shuffles: after the six steps every lane holds the result of all 64.  Every lane of the wave must be active.
// Floats come in two forms that differ on NaN and are kept apart: wave_fmin / wave_fmax are fminf / fmaxf (a NaN operand is dropped);
// wave_min / wave_max on floats are the compare-and-select `other < mine ? other : mine` (a NaN never wins and never leaves).
template <class T, class F>
__device__ __forceinline__ T wave_reduce(T v, F f) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = f(v, (T)__shfl_xor(v, off));
    return v;
}
template <class T>      // int, uint32_t
__device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, [](T mine, T other) { return min(mine, other); }); }
template <class T>
__device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T mine, T other) { return max(mine, other); }); }
template <class T>
__device__ __forceinline__ T wave_add(T v) { return wave_reduce(v, [](T mine, T other) { return mine + other; }); }
__device__ __forceinline__ float wave_min(float v) { return wave_reduce(v, [](float mine, float other) { return other < mine ? other : mine; }); }
__device__ __forceinline__ float wave_max(float v) { return wave_reduce(v, [](float mine, float other) { return other > mine ? other : mine; }); }
__device__ __forceinline__ float wave_fmin(float v) { return wave_reduce(v, [](float mine, float other) { return fminf(mine, other); }); }
__device__ __forceinline__ float wave_fmax(float v) { return wave_reduce(v, [](float mine, float other) { return fmaxf(mine, other); }); }

// ---- the box of a 64-slot group --------------------------------------------------------------------------------------------------
// box64[2g], box64[2g + 1] = (min xyz, 0), (max xyz, 0) over the 192 corners of the slots [64g, 64g + 64): what the frame's cull test
// (group_culled_m) projects.  A coordinate that is not finite poisons the whole box with NaN, which the cull test reads as "cannot be
// culled".  One wave per group, one lane per slot: the lane folds its three corners, the wave reduces, lane 0 stores.
__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }
struct GroupBox { float lo[3], hi[3]; bool bad; };
__device__ __forceinline__ GroupBox box_start() { return GroupBox{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}, false}; }
__device__ __forceinline__ void box_fold(GroupBox& b, const float4& x) {       // one corner
    const float c[3] = {x.x, x.y, x.z};
#pragma unroll
    for (int j = 0; j < 3; j++) {
        b.bad = b.bad || !(fabsf(c[j]) < INFINITY);
        b.lo[j] = fminf(b.lo[j], c[j]);
        b.hi[j] = fmaxf(b.hi[j], c[j]);
    }
}
// the wave's box in every lane, poisoned if any lane met a coordinate that is not finite; returns whether it is
__device__ __forceinline__ bool box_reduce(GroupBox& b) {
    const bool any_bad = __ballot(b.bad) != 0ull;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float lo = wave_fmin(b.lo[j]), hi = wave_fmax(b.hi[j]);
        b.lo[j] = any_bad ? quiet_nan() : lo;
        b.hi[j] = any_bad ? quiet_nan() : hi;
    }
    return any_bad;
}
__device__ __forceinline__ void box_store(const GroupBox& b, float4* __restrict__ box /* &box64[2g] */) {
    box[0] = make_float4(b.lo[0], b.lo[1], b.lo[2], 0);
    box[1] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0);
}

// ---- the pixel quantiser ---------------------------------------------------------------------------------------------------------
// Pixel(float3:) -> .floats(b: z, g: y, r: x, a: 1) clamps to [0, 1], scales by 255 and truncates (Renderer.swift:116-128); the Metal
// path's bgra8Unorm store rounds to nearest even instead.
template <bool METAL>
__device__ __forceinline__ uint32_t quantize_channel(float f) {
    float u = fminf(fmaxf(f, 0.0f), 1.0f) * 255.0f;
    if (METAL) u = rintf(u);
    return (uint32_t)u;
}
// f = (r, g, b, a) -> the framebuffer's BGRA word: quantize_channel of each, in the statement order of the raster kernels' resolves
// (four clamps, four roundings, four conversions: any other order moves their instructions)
template <bool METAL>
__device__ __forceinline__ uint32_t quantize_bgra(float4 f) {
    float ub = fminf(fmaxf(f.z, 0.0f), 1.0f) * 255.0f, ug = fminf(fmaxf(f.y, 0.0f), 1.0f) * 255.0f;
    float ur = fminf(fmaxf(f.x, 0.0f), 1.0f) * 255.0f, ua = fminf(fmaxf(f.w, 0.0f), 1.0f) * 255.0f;
    if (METAL) { ub = rintf(ub); ug = rintf(ug); ur = rintf(ur); ua = rintf(ua); }
    return (uint32_t)ub | ((uint32_t)ug << 8) | ((uint32_t)ur << 16) | ((uint32_t)ua << 24);
}

// ---- the cross product -----------------------------------------------------------------------------------------------------------
// include/swr.h "Dual-quaternion skinning": two products and one subtraction per component, each rounded.  The rotation of the
// dual-quaternion skin and the face vector of the computed normals (swr_normals.hip).
struct Vec3 { float x, y, z; };
__device__ __forceinline__ Vec3 cross3(const Vec3 a, const Vec3 b) {
    Vec3 r;
    r.x = a.y * b.z - a.z * b.y;
    r.y = a.z * b.x - a.x * b.z;
    r.z = a.x * b.y - a.y * b.x;
    return r;
}

// ---- draw lists --------------------------------------------------------------------------------------------------
// The item of frame slot v (UNITS: of work unit v — k_bin<LIST>'s and k_item_bounds'): the last item whose vbase (ubase) is <= v.  Empty
// items share their base with the next item and are passed over; item 0 starts at 0.  (A binary search over <= SWR_DRAW_LIST_MAX items.)
template <bool UNITS>
__device__ __forceinline__ int list_find(const ListItem* __restrict__ items, int n, uint32_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t key = UNITS ? items[mid].ubase : items[mid].vbase;
        if (key <= v) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

}  // namespace swr
