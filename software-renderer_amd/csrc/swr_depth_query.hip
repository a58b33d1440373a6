// swr_depth_query.hip — depth queries (include/swr.h "Depth queries").
//
// passed[k] = the number of pixels of box k with z_k < depth, the strict z-test of the raster.  Brute force costs the sum of the box
// areas (4096 object boxes over a 4K frame are gigabytes of reads), so a query runs in two steps on the context's raster stream:
//
//   k_depth_tiles reads the band's depth image once and writes one 16-byte record per tile of 64 columns x DQ_TILE_ROWS rows:
//     mn / mx, the minimum / maximum over the tile's non-NaN pixels (from +inf / -inf), and nan, the number of its NaN pixels.
//     One wave per tile, one dword load per lane and row (256 contiguous bytes per wave and row, all rows of the tile in flight
//     together), folded with explicit comparisons — d < m ? d : m skips a NaN by itself, nothing relies on what fminf does with
//     one — and reduced across the wave with shuffles.  A tile's pixel count follows from its position (the tiles of the right
//     and bottom edge are partial).  Tiles are band-local, so a band border is a tile border.
//   k_depth_boxes: one workgroup per box, its waves striding over the tiles the box touches.  With I the box's part of the tile:
//       !(z < mx)                              contributes 0   (all-NaN tiles, z = +inf and boxes behind everything included)
//       z < mn and nan == 0                    contributes |I|
//       z < mn and the tile is wholly inside   contributes the tile's pixel count minus nan
//       otherwise                              the pixels of I are read: a lane per column, the lanes add up z < d down the rows
//     so only tiles that straddle z are read: the occluders' silhouettes, and partial tiles that hold NaNs.  The accepted tiles
//     are added in a wave-uniform register, the scanned pixels per lane; one shuffle reduction per wave and four LDS words per
//     workgroup end in ONE plain store per box: no atomics, no memset.
//   A box whose part in the band holds DEPTH_QUERY_SPLIT_AREA pixels or more (a whole-target box with z in the middle of the
//     scene's range makes one workgroup scan most of a frame) is stored as 0 by its own workgroup and walked by DQ_SPLIT_BLOCKS
//     workgroups of a second launch, each adding its share with one integer atomic.  The host lists those boxes (it has every box in
//     hand when it checks them), so the second launch exists only when there is one.
//   A query whose boxes together hold less than 1 / DQ_SKIP_RATIO of the band does not pay the read of the whole band: it is scanned
//     directly (k_depth_boxes<false, false>, every tile treated as straddling).
// All arithmetic on the counts is integer and every comparison is the binary32 '<' of the definition: the result is exact, whichever
// route a tile takes.  T, the skip and the split were chosen by measurement (tools/depth_query_ab.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "swr_internal.h"
#include "swr_rules.hip.h"

namespace swr {

namespace {

#ifndef SWR_TUNE_DEPTH_QUERY
#define SWR_TUNE_DEPTH_QUERY (-1)           // -1 = the product; 0 = the plain scan of every box, no summary and no split (the A/B base);
                                            // 1 = the summary always (no skip); 2 = no split; 8, 16, 32 = the product with that tile height
#endif

constexpr int DQ_TILE_ROWS_PRODUCT = 32;    // T: divides 32 (chosen by measurement)
constexpr int DQ_TILE_ROWS = (SWR_TUNE_DEPTH_QUERY == 8 || SWR_TUNE_DEPTH_QUERY == 16 || SWR_TUNE_DEPTH_QUERY == 32)
                                 ? SWR_TUNE_DEPTH_QUERY : DQ_TILE_ROWS_PRODUCT;
constexpr int DQ_THREADS = 256;
constexpr int DQ_WAVES = DQ_THREADS / 64;
constexpr int DQ_SPLIT_BLOCKS = 64;         // workgroups that share a large box
constexpr uint64_t DQ_SKIP_RATIO = 16;      // the summary is skipped when total box area * DQ_SKIP_RATIO < the band's pixels
static_assert(32 % DQ_TILE_ROWS == 0 && DQ_TILE_ROWS >= 8, "band borders are tile borders; depth_query_scratch_bytes assumes T >= 8");

struct DepthTile {
    float mn, mx;               // over the non-NaN pixels; +inf / -inf when there is none
    uint32_t nan;               // NaN pixels
    uint32_t pad;
};
static_assert(sizeof(DepthTile) == 16, "depth_query_scratch_bytes");

struct DqArgs {
    const float* depth;         // the band's depth image, `width` floats per row
    int32_t width, rows;        // of the band
    int32_t row0;               // the band's first row in the target
    const swr_depth_box* boxes; // full-target coordinates
    const uint32_t* large;      // SPLIT: the boxes walked by this launch
    const DepthTile* tiles;     // SUMMARY: tiles_x * ceil(rows / T) records
    int32_t tiles_x;
    int32_t skip_large;         // !SPLIT: a large box is stored as 0 and left to the SPLIT launch
    uint32_t* passed;
};

__global__ __launch_bounds__(DQ_THREADS) void k_depth_tiles(const float* depth, int32_t width, int32_t rows, int32_t tiles_x, uint32_t ntiles,
                                                            DepthTile* out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * DQ_WAVES + (threadIdx.x >> 6);
    if (tile >= ntiles) return;                 // (wave-uniform)
    const int32_t ty = (int32_t)(tile / (uint32_t)tiles_x), tx = (int32_t)tile - ty * tiles_x;
    const int32_t x = tx * 64 + (int32_t)lane, y0 = ty * DQ_TILE_ROWS;
    const bool in_x = x < width;
    // (a lane or row outside the band reads the band's nearest pixel instead and is left out of the fold: no load is under a branch,
    // so all of them are in flight together)
    const float* p = depth + (size_t)std::min(x, width - 1);
    float d[DQ_TILE_ROWS];
#pragma unroll
    for (int r = 0; r < DQ_TILE_ROWS; r++) d[r] = p[(size_t)std::min(y0 + r, rows - 1) * (size_t)width];
    float mn = INFINITY, mx = -INFINITY;
    uint32_t nan = 0;
#pragma unroll
    for (int r = 0; r < DQ_TILE_ROWS; r++) {
        const bool in = in_x && y0 + r < rows;
        mn = in && d[r] < mn ? d[r] : mn;
        mx = in && d[r] > mx ? d[r] : mx;
        nan += in && d[r] != d[r] ? 1u : 0u;
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    nan = wave_add(nan);
    if (lane == 0) {
        DepthTile t;
        t.mn = mn; t.mx = mx; t.nan = nan; t.pad = 0;
        out[tile] = t;
    }
}

template <bool SUMMARY, bool SPLIT>
__global__ __launch_bounds__(DQ_THREADS) void k_depth_boxes(DqArgs a) {
    __shared__ uint32_t s_sum[DQ_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t k = SPLIT ? a.large[blockIdx.x / DQ_SPLIT_BLOCKS] : blockIdx.x;
    const swr_depth_box b = a.boxes[k];
    // the box's part in the band, band-local rows (the host has checked the box against the target; the clamps keep every read inside
    // the band whatever it holds)
    const int32_t x0 = std::max(b.x0, 0), x1 = std::min(b.x1, a.width);
    const int32_t y0 = std::max(b.y0 - a.row0, 0), y1 = std::min(b.y1 - a.row0, a.rows);
    const float z = b.z;
    const bool none = x0 >= x1 || y0 >= y1;
    const bool large = !none && (uint32_t)(x1 - x0) * (uint32_t)(y1 - y0) >= DEPTH_QUERY_SPLIT_AREA;
    if (SPLIT) {
        if (!large || z != z) return;           // (not listed by the host; a NaN z passes nowhere: the 0 is already there)
    } else if (none || z != z || (a.skip_large && large)) {
        if (threadIdx.x == 0) a.passed[k] = 0;
        return;
    }
    const int32_t tx0 = x0 >> 6, ntx = ((x1 + 63) >> 6) - tx0;
    const int32_t ty0 = y0 / DQ_TILE_ROWS, nty = (y1 + DQ_TILE_ROWS - 1) / DQ_TILE_ROWS - ty0;
    const uint32_t nt = (uint32_t)ntx * (uint32_t)nty;
    const uint32_t first = SPLIT ? (blockIdx.x % DQ_SPLIT_BLOCKS) * DQ_WAVES + wave : wave;
    const uint32_t stride = SPLIT ? DQ_SPLIT_BLOCKS * DQ_WAVES : DQ_WAVES;
    uint32_t acc = 0;           // wave-uniform: the tiles accepted from their record
    uint32_t cnt = 0;           // per lane: the pixels read
    for (uint32_t t = first; t < nt; t += stride) {             // (wave-uniform: every lane is active)
        const int32_t tyi = (int32_t)(t / (uint32_t)ntx), tx = tx0 + ((int32_t)t - tyi * ntx), ty = ty0 + tyi;
        const int32_t ix0 = std::max(x0, tx * 64), ix1 = std::min(x1, tx * 64 + 64);
        const int32_t iy0 = std::max(y0, ty * DQ_TILE_ROWS), iy1 = std::min(y1, ty * DQ_TILE_ROWS + DQ_TILE_ROWS);
        if (SUMMARY) {
            const DepthTile rec = a.tiles[(size_t)ty * (size_t)a.tiles_x + (size_t)tx];
            if (!(z < rec.mx)) continue;
            if (z < rec.mn) {
                if (rec.nan == 0) { acc += (uint32_t)(ix1 - ix0) * (uint32_t)(iy1 - iy0); continue; }
                const int32_t tw = std::min(64, a.width - tx * 64), th = std::min(DQ_TILE_ROWS, a.rows - ty * DQ_TILE_ROWS);
                if (ix1 - ix0 == tw && iy1 - iy0 == th) { acc += (uint32_t)(tw * th) - rec.nan; continue; }
            }
        }
        const int32_t x = tx * 64 + (int32_t)lane;
        if (x >= ix0 && x < ix1) {
            const float* p = a.depth + (size_t)iy0 * (size_t)a.width + (size_t)x;
#pragma unroll 4
            for (int32_t y = iy0; y < iy1; y++, p += a.width) cnt += z < *p ? 1u : 0u;
        }
    }
    cnt = wave_add(cnt);
    if (lane == 0) s_sum[wave] = cnt + acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < DQ_WAVES; w++) sum += s_sum[w];
        if (!SPLIT) a.passed[k] = sum;
        else if (sum) atomicAdd(&a.passed[k], sum);
    }
}

}  // namespace

void launch_depth_query(const float* depth, int width, int rows, int row_begin, const swr_depth_box* boxes, int64_t n,
                        const uint32_t* large, int64_t nlarge, uint64_t total_area, void* scratch, uint32_t* passed, hipStream_t s) {
    if (n <= 0 || n > SWR_DEPTH_QUERY_MAX || width <= 0 || rows <= 0) return;
    DqArgs a;
    a.depth = depth; a.width = width; a.rows = rows; a.row0 = row_begin;
    a.boxes = boxes; a.large = large; a.tiles = (const DepthTile*)scratch;
    a.tiles_x = (width + 63) / 64;
    a.passed = passed;
    const uint32_t ntiles = (uint32_t)a.tiles_x * (uint32_t)((rows + DQ_TILE_ROWS - 1) / DQ_TILE_ROWS);
    const bool summary = SWR_TUNE_DEPTH_QUERY != 0 &&
                         (SWR_TUNE_DEPTH_QUERY == 1 || total_area * DQ_SKIP_RATIO >= (uint64_t)width * (uint64_t)rows);
    const bool split = summary && SWR_TUNE_DEPTH_QUERY != 2 && nlarge > 0;
    a.skip_large = split ? 1 : 0;
    if (summary) {
        hipLaunchKernelGGL(k_depth_tiles, dim3((ntiles + DQ_WAVES - 1) / DQ_WAVES), dim3(DQ_THREADS), 0, s, depth, width, rows, a.tiles_x,
                           ntiles, (DepthTile*)scratch);
        hipLaunchKernelGGL((k_depth_boxes<true, false>), dim3((uint32_t)n), dim3(DQ_THREADS), 0, s, a);
    } else {
        hipLaunchKernelGGL((k_depth_boxes<false, false>), dim3((uint32_t)n), dim3(DQ_THREADS), 0, s, a);
    }
    if (split) hipLaunchKernelGGL((k_depth_boxes<true, true>), dim3((uint32_t)nlarge * DQ_SPLIT_BLOCKS), dim3(DQ_THREADS), 0, s, a);
}

}  // namespace swr
