// swr_item_bounds.hip — item bounds (include/swr.h "Item bounds").
//
// records[k] = the screen rectangle, the depth range and the three triangle counts of draw item k: a reduction over the item's
// triangles in the arithmetic of the frame's setup (screen_vertex and screen_vertices_ok of swr_rules.hip.h, as setup_triangle_r in
// swr_kernels.hip uses them, then truncation).  The host has cut the resident triangle stream at the items' boundaries, as a
// draw list does, so item k's triangles are the stream slots [first, first + count): 48 contiguous bytes per triangle, no index gather.
//
//   k_item_bounds_init    one lane per partial record (ITEM_BOUNDS_SLOTS per item, 64 bytes each): the fold's start — min from INT_MAX
//                         / +inf, max from INT_MIN / -inf, the counts 0 — by plain stores.
//   k_item_bounds<MT>     one workgroup per (item, chunk of ITEM_BOUNDS_CHUNK slots) work unit, laid out by the host like the work
//                         units of k_bin<LIST> (ListItem::ubase; the item of a unit by binary search, wave-uniform, its matrix in scalar
//                         registers).  A lane owns one triangle per pass of 256: three float4 loads, the per-corner arithmetic, a fold
//                         of the nine quantities in registers; then a wave64 reduction with shuffles, four waves through LDS, and ONE
//                         combine per workgroup into one of the item's partial records (its unit number modulo ITEM_BOUNDS_SLOTS):
//                         integer atomicMin / atomicMax for ix and iy, the same on orderable(sz) — the monotone float -> uint map of
//                         the visibility keys (orderable_depth, swr_rules.hip.h), so the depth's minimum and maximum are exact and
//                         order-free — and atomicAdd for the skipped and behind counts.  No float atomic.  (Atomics on one address
//                         serialise at 8 to 14 ns each: with one record per item they were 40 of the kernel's 50 us on a million
//                         triangles; 32 records on lines of their own take them off the critical path.)
//   k_item_bounds_finish  one lane per item: its partial records folded, the keys back to floats, + 0.0f (a zero comes out as +0),
//                         the rectangle made half-open and clamped to the target, all 0 for an item without a drawable triangle,
//                         drawable = count - skipped; the 48-byte record.
// The perspective divide is always made: x / 1 is exact, so an affine item gives the same bits as k_bin<AFF> does without it.
// Everything but the per-corner floats is integer; min and max do not depend on order: the result is bit-defined.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "swr_internal.h"
#include "swr_rules.hip.h"

namespace swr {

namespace {

#ifndef SWR_TUNE_ITEM_BOUNDS
#define SWR_TUNE_ITEM_BOUNDS (-1)           // -1 = the product: the walk of the cut stream, one pass per item; the A/B builds of DESIGN.md §25:
                                            // 1 = the index gather (first / count are primitive numbers, no cut: the corners come from
                                            // `vertices` through `indices`); 2 = instancing (consecutive items over one range share the
                                            // work units of the first: a workgroup walks its chunk once per matrix, from L2 after the first)
#endif

constexpr int IB_THREADS = 256;
constexpr int IB_WAVES = IB_THREADS / 64;
static_assert(ITEM_BOUNDS_CHUNK % IB_THREADS == 0, "a work unit is a whole number of passes");
static_assert(sizeof(swr_item_bound) == 48, "include/swr.h");

// a partial record: the minima and maxima of ix / iy (inclusive), zmin / zmax as orderable keys, the counts; 64 bytes, so that no two
// share the 64 bytes an atomic request covers
struct alignas(64) IbAccum {
    int32_t minx, miny, maxx, maxy;
    uint32_t zmin, zmax;
    uint32_t drawable, skipped, behind;     // (drawable: in registers and LDS only; the finish has it as count - skipped)
    uint32_t pad[7];
};
static_assert(sizeof(IbAccum) == 64, "item_bounds_scratch_bytes");

__device__ __forceinline__ IbAccum ib_start() {
    IbAccum a;
    a.minx = a.miny = INT32_MAX; a.maxx = a.maxy = INT32_MIN;
    a.zmin = orderable_depth(INFINITY); a.zmax = orderable_depth(-INFINITY);
    a.drawable = a.skipped = a.behind = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) a.pad[i] = 0;
    return a;
}

__global__ __launch_bounds__(IB_THREADS) void k_item_bounds_init(IbAccum* partial, uint32_t n /* items * ITEM_BOUNDS_SLOTS */) {
    const uint32_t k = blockIdx.x * IB_THREADS + threadIdx.x;
    if (k < n) partial[k] = ib_start();
}

template <bool MT>
__global__ __launch_bounds__(IB_THREADS) void k_item_bounds(ItemBoundsArgs a) {
    __shared__ IbAccum s_part[IB_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int k = __builtin_amdgcn_readfirstlane(list_find<true>(a.items, a.n, blockIdx.x));
    const uint32_t first = a.items[k].first, count = a.items[k].count;
    const uint32_t t0 = (blockIdx.x - a.items[k].ubase) * (uint32_t)ITEM_BOUNDS_CHUNK;   // < count: the host gave the item ceil(count / CHUNK) units
    const float fw = (float)a.width, fh = (float)a.height;
    int k_end = k + 1;          // (the instancing A/B: the items after k over the same range have no units of their own)
    if (SWR_TUNE_ITEM_BOUNDS == 2)
        while (k_end < a.n && a.items[k_end].first == first && a.items[k_end].count == count) k_end++;
    for (int kk = k; kk < k_end; kk++) {
        const float4* __restrict__ mc = reinterpret_cast<const float4*>(a.items[kk].m);
        const float4x4 M = {{mc[0], mc[1], mc[2], mc[3]}};

        int32_t minx = INT32_MAX, miny = INT32_MAX, maxx = INT32_MIN, maxy = INT32_MIN;
        float zmin = INFINITY, zmax = -INFINITY;
        uint32_t drawable = 0, skipped = 0, behind = 0;
#pragma unroll 2
        for (uint32_t p = 0; p < (uint32_t)ITEM_BOUNDS_CHUNK; p += IB_THREADS) {
            const uint32_t t = t0 + p + threadIdx.x;
            const bool in = t < count;
            // (a lane past the item's end reads the item's last triangle instead and is left out of the fold: no load is under a branch)
            const size_t s = (size_t)first + (size_t)std::min(t, count - 1u);
            float4 x[3];
            if (SWR_TUNE_ITEM_BOUNDS == 1) {
#pragma unroll
                for (int j = 0; j < 3; j++) x[j] = reinterpret_cast<const float4*>(a.vertices)[2 * (size_t)a.indices[3 * s + j]];
            } else {
#pragma unroll
                for (int j = 0; j < 3; j++) x[j] = a.tri_xyz[3 * s + j];
            }
            float sx[3], sy[3], sz[3];
            bool w_ok = true;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const ScreenVertex v = screen_vertex<MT>(make_float3(x[j].x, x[j].y, x[j].z), M, fw, fh);
                sx[j] = v.sx; sy[j] = v.sy; sz[j] = v.sz;
                w_ok = w_ok && (v.w > 0.0f);
            }
            const bool ok = screen_vertices_ok<MT, 3>(sx, sy);
            const bool d = in && ok;
            drawable += d ? 1u : 0u;
            skipped += (in && !ok) ? 1u : 0u;
            behind += (d && !w_ok) ? 1u : 0u;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int32_t ix = ok ? (int32_t)sx[j] : 0, iy = ok ? (int32_t)sy[j] : 0;
                minx = d ? std::min(minx, ix) : minx; maxx = d ? std::max(maxx, ix) : maxx;
                miny = d ? std::min(miny, iy) : miny; maxy = d ? std::max(maxy, iy) : maxy;
                zmin = (d && sz[j] < zmin) ? sz[j] : zmin;
                zmax = (d && sz[j] > zmax) ? sz[j] : zmax;
            }
        }
        minx = wave_min(minx); maxx = wave_max(maxx); miny = wave_min(miny); maxy = wave_max(maxy);
        zmin = wave_min(zmin); zmax = wave_max(zmax);
        drawable = wave_add(drawable); skipped = wave_add(skipped); behind = wave_add(behind);
        if (lane == 0) {
            IbAccum w = ib_start();
            w.minx = minx; w.miny = miny; w.maxx = maxx; w.maxy = maxy;
            w.zmin = orderable_depth(zmin); w.zmax = orderable_depth(zmax);
            w.drawable = drawable; w.skipped = skipped; w.behind = behind;
            s_part[wave] = w;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            IbAccum w = s_part[0];
            for (int i = 1; i < IB_WAVES; i++) {
                const IbAccum& q = s_part[i];
                w.minx = std::min(w.minx, q.minx); w.miny = std::min(w.miny, q.miny);
                w.maxx = std::max(w.maxx, q.maxx); w.maxy = std::max(w.maxy, q.maxy);
                w.zmin = std::min(w.zmin, q.zmin); w.zmax = std::max(w.zmax, q.zmax);
                w.drawable += q.drawable; w.skipped += q.skipped; w.behind += q.behind;
            }
            IbAccum* r = reinterpret_cast<IbAccum*>(a.scratch) + (size_t)kk * ITEM_BOUNDS_SLOTS + (blockIdx.x - a.items[k].ubase) % ITEM_BOUNDS_SLOTS;
            if (w.drawable) {       // (a workgroup without a drawable triangle holds the fold's start: nothing to combine)
                atomicMin(&r->minx, w.minx); atomicMax(&r->maxx, w.maxx);
                atomicMin(&r->miny, w.miny); atomicMax(&r->maxy, w.maxy);
                atomicMin(&r->zmin, w.zmin); atomicMax(&r->zmax, w.zmax);
            }
            if (w.skipped) atomicAdd(&r->skipped, w.skipped);
            if (w.behind) atomicAdd(&r->behind, w.behind);
        }
        if (SWR_TUNE_ITEM_BOUNDS == 2) __syncthreads();     // (s_part is written again for the next matrix)
    }
}

__global__ __launch_bounds__(IB_THREADS) void k_item_bounds_finish(const IbAccum* __restrict__ partial, const ListItem* __restrict__ items,
                                                                   int32_t n, int32_t width, int32_t height, swr_item_bound* records) {
    const int32_t k = (int32_t)(blockIdx.x * IB_THREADS + threadIdx.x);
    if (k >= n) return;
    IbAccum a = partial[(size_t)k * ITEM_BOUNDS_SLOTS];
    for (int i = 1; i < ITEM_BOUNDS_SLOTS; i++) {
        const IbAccum q = partial[(size_t)k * ITEM_BOUNDS_SLOTS + i];
        a.minx = std::min(a.minx, q.minx); a.miny = std::min(a.miny, q.miny);
        a.maxx = std::max(a.maxx, q.maxx); a.maxy = std::max(a.maxy, q.maxy);
        a.zmin = std::min(a.zmin, q.zmin); a.zmax = std::max(a.zmax, q.zmax);
        a.skipped += q.skipped; a.behind += q.behind;
    }
    swr_item_bound b;
    const uint32_t drawable = items[k].count - a.skipped;
    const bool any = drawable != 0;
    // (|ix| < 2^30: max + 1 does not overflow)
    b.x0 = any ? std::min(std::max(a.minx, 0), width) : 0;
    b.x1 = any ? std::min(std::max(a.maxx + 1, 0), width) : 0;
    b.y0 = any ? std::min(std::max(a.miny, 0), height) : 0;
    b.y1 = any ? std::min(std::max(a.maxy + 1, 0), height) : 0;
    b.zmin = depth_from_orderable(a.zmin) + 0.0f;
    b.zmax = depth_from_orderable(a.zmax) + 0.0f;
    b.drawable = drawable; b.skipped = a.skipped; b.behind = a.behind;
    b.reserved[0] = b.reserved[1] = b.reserved[2] = 0;
    records[k] = b;
}

}  // namespace

void launch_item_bounds(const ItemBoundsArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.n > SWR_DRAW_LIST_MAX) return;
    const dim3 per_item((uint32_t)(a.n + IB_THREADS - 1) / IB_THREADS), block(IB_THREADS);
    const uint32_t slots = (uint32_t)a.n * ITEM_BOUNDS_SLOTS;
    hipLaunchKernelGGL(k_item_bounds_init, dim3((slots + IB_THREADS - 1) / IB_THREADS), block, 0, s, (IbAccum*)a.scratch, slots);
    if (a.units > 0) {
        if (a.metal) hipLaunchKernelGGL((k_item_bounds<true>), dim3((uint32_t)a.units), block, 0, s, a);
        else hipLaunchKernelGGL((k_item_bounds<false>), dim3((uint32_t)a.units), block, 0, s, a);
    }
    hipLaunchKernelGGL(k_item_bounds_finish, per_item, block, 0, s, (const IbAccum*)a.scratch, a.items, a.n, a.width, a.height, a.records);
}

}  // namespace swr
