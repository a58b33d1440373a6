// swr_delta.hip — delta reads (include/swr.h "Delta reads").
//
// Colour and depth are both one 32-bit word per pixel, so one kernel family serves both.
//
// k_delta_tiles compares a band's image with the band's baseline — the image the host already holds — tile by tile.  One wave per
// 64 x 32 tile, four waves per workgroup.  A wave reads its tile row by row, 256 contiguous bytes per row: with 16-byte accesses where
// width % 4 == 0 (16 lanes per row, four rows per access, eight accesses per image), with dword accesses otherwise (one row per
// access, 32 accesses: ragged widths are legal, and a row then starts at any word).  No load sits under a branch: lanes beyond the
// band's right or bottom edge are clamped into the band and left out of the fold.  The wave ORs cur ^ base over its words, one ballot
// says whether any lane saw a difference, and only then are the tile's current words stored into the baseline (and, DIRECT, into the
// caller's page-locked image, mapped into the device's address space): an unchanged tile costs its two reads and nothing else.  Every
// tile stores its own word of the flag table, changed or not: no atomics, and nothing to zero before.  HAVE_BASE = false is the first
// delivery: no compare, every tile is stored — the device-to-device copy of the band into a fresh baseline — and flagged.
//
// k_delta_pack gathers the rows of a rectangle of the band into contiguous memory, for one linear copy to the host: the way to a
// pageable destination.  For a page-locked one the DIRECT store won the measurement (0.05 against 0.13 ms on the app's
// scene at 4K, 0.33 against 0.62 ms on a half-changed frame): no second launch, no second wait, and only the changed tiles cross.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "swr_internal.h"

namespace swr {

namespace {

constexpr int DELTA_THREADS = 256;
constexpr int DELTA_WAVES = DELTA_THREADS / 64;

struct DeltaArgs {
    const uint32_t* cur;    // the band's image, `width` words per row
    uint32_t* base;         // the band's baseline, the same layout
    uint32_t* flags;        // [tiles_x * tiles_y]: 1 = the tile differed (or HAVE_BASE is false)
    uint32_t* direct;       // DIRECT: the band's rows of the caller's image (page-locked, mapped), the same layout
    int32_t width, rows;
    int32_t tiles_x, tiles;
};

template <bool HAVE_BASE, bool VEC, bool DIRECT>
__global__ __launch_bounds__(DELTA_THREADS) void k_delta_tiles(DeltaArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int tile = (int)(blockIdx.x * DELTA_WAVES + (threadIdx.x >> 6));
    if (tile >= a.tiles) return;                // (wave-uniform: a whole wave leaves, and nothing below waits for another wave)
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    if (VEC) {
        // lane = (row of four, quad of sixteen): 16 lanes x 16 bytes per tile row, four rows per access
        const int x = tx * TILE_W + (lane & 15) * 4, ysub = ty * TILE_H + (lane >> 4);
        const bool xin = x < a.width;           // (width % 4 == 0: a quad is inside or outside as a whole)
        const int xc = xin ? x : a.width - 4;
        if (!HAVE_BASE) {           // the first delivery: load and store row by row, nothing is kept
#pragma unroll
            for (int k = 0; k < TILE_H / 4; k++) {
                const int y = ysub + 4 * k;
                const size_t at = (size_t)(y < a.rows ? y : a.rows - 1) * (size_t)a.width + (size_t)xc;
                const uint4 c = *(const uint4*)(a.cur + at);
                if (xin && y < a.rows) *(uint4*)(a.base + at) = c;
            }
            if (lane == 0) a.flags[tile] = 1u;
            return;
        }
        uint4 cur[TILE_H / 4];
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < TILE_H / 4; k++) {
            const int y = ysub + 4 * k;
            const bool in = xin && y < a.rows;
            const size_t at = (size_t)(y < a.rows ? y : a.rows - 1) * (size_t)a.width + (size_t)xc;
            cur[k] = *(const uint4*)(a.cur + at);
            if (HAVE_BASE) {
                const uint4 b = *(const uint4*)(a.base + at);
                const uint32_t d = (cur[k].x ^ b.x) | (cur[k].y ^ b.y) | (cur[k].z ^ b.z) | (cur[k].w ^ b.w);
                acc |= in ? d : 0u;
            }
        }
        const bool changed = HAVE_BASE ? __ballot(acc != 0u) != 0ull : true;
        if (changed && xin) {
#pragma unroll
            for (int k = 0; k < TILE_H / 4; k++) {
                const int y = ysub + 4 * k;
                if (y < a.rows) {
                    const size_t at = (size_t)y * (size_t)a.width + (size_t)x;
                    *(uint4*)(a.base + at) = cur[k];
                    if (DIRECT) *(uint4*)(a.direct + at) = cur[k];
                }
            }
        }
        if (lane == 0) a.flags[tile] = changed ? 1u : 0u;
    } else {
        // lane = column: 64 lanes x 4 bytes per tile row, one row per access
        const int x = tx * TILE_W + lane, y0 = ty * TILE_H;
        const bool xin = x < a.width;
        const int xc = xin ? x : a.width - 1;
        if (!HAVE_BASE) {
#pragma unroll
            for (int k = 0; k < TILE_H; k++) {
                const int y = y0 + k;
                const size_t at = (size_t)(y < a.rows ? y : a.rows - 1) * (size_t)a.width + (size_t)xc;
                const uint32_t c = a.cur[at];
                if (xin && y < a.rows) a.base[at] = c;
            }
            if (lane == 0) a.flags[tile] = 1u;
            return;
        }
        uint32_t cur[TILE_H];
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < TILE_H; k++) {
            const int y = y0 + k;
            const bool in = xin && y < a.rows;
            const size_t at = (size_t)(y < a.rows ? y : a.rows - 1) * (size_t)a.width + (size_t)xc;
            cur[k] = a.cur[at];
            if (HAVE_BASE) {
                const uint32_t d = cur[k] ^ a.base[at];
                acc |= in ? d : 0u;
            }
        }
        const bool changed = HAVE_BASE ? __ballot(acc != 0u) != 0ull : true;
        if (changed && xin) {
#pragma unroll
            for (int k = 0; k < TILE_H; k++) {
                const int y = y0 + k;
                if (y < a.rows) {
                    const size_t at = (size_t)y * (size_t)a.width + (size_t)x;
                    a.base[at] = cur[k];
                    if (DIRECT) a.direct[at] = cur[k];
                }
            }
        }
        if (lane == 0) a.flags[tile] = changed ? 1u : 0u;
    }
}

struct PackArgs {
    const uint32_t* src;    // the band's image, `width` words per row
    uint32_t* out;          // rows of `w` words, contiguous
    int32_t width, x0, y0, w;
    uint32_t units;         // VEC: quads, else words, of the rectangle
};

// a grid-stride copy of the rectangle, one quad (VEC: width % 4 == 0, and x0 is a multiple of the tile width) or one word per lane
template <bool VEC>
__global__ __launch_bounds__(DELTA_THREADS) void k_delta_pack(PackArgs a) {
    const uint32_t per_row = VEC ? (uint32_t)a.w / 4u : (uint32_t)a.w;
    for (uint32_t i = blockIdx.x * DELTA_THREADS + threadIdx.x; i < a.units; i += gridDim.x * DELTA_THREADS) {
        const uint32_t r = i / per_row, q = i - r * per_row;
        if (VEC) {
            const size_t from = (size_t)(a.y0 + (int)r) * (size_t)a.width + (size_t)a.x0 + (size_t)q * 4u;
            *(uint4*)(a.out + (size_t)i * 4u) = *(const uint4*)(a.src + from);
        } else {
            a.out[i] = a.src[(size_t)(a.y0 + (int)r) * (size_t)a.width + (size_t)a.x0 + q];
        }
    }
}

template <bool HAVE_BASE, bool VEC>
void launch_tiles(const DeltaArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.tiles + DELTA_WAVES - 1) / DELTA_WAVES)), block(DELTA_THREADS);
    if constexpr (HAVE_BASE) {
        if (a.direct) { hipLaunchKernelGGL((k_delta_tiles<true, VEC, true>), grid, block, 0, s, a); return; }
    }
    hipLaunchKernelGGL((k_delta_tiles<HAVE_BASE, VEC, false>), grid, block, 0, s, a);      // (a first delivery goes by the plain copy)
}

}  // namespace

// Compare the band's image `cur` (`width` words per row, `rows` rows) with its baseline `base`, tile by tile: flags[t] = 1 where tile
// t (row-major, ceil(width / 64) per row) differs in any bit, else 0, and the changed tiles' words are stored into `base`.
// have_base == 0: nothing is compared, every tile is stored and flagged.  direct: NULL, or the band's rows of a page-locked host image
// as the device sees them; the changed tiles' words are stored there too.  All pointers but `direct` are device memory.
void launch_delta(const uint32_t* cur, uint32_t* base, int have_base, int width, int rows, uint32_t* flags, uint32_t* direct, hipStream_t s) {
    if (width <= 0 || rows <= 0) return;
    DeltaArgs a;
    a.cur = cur; a.base = base; a.flags = flags; a.direct = direct;
    a.width = width; a.rows = rows;
    a.tiles_x = (width + TILE_W - 1) / TILE_W;
    a.tiles = a.tiles_x * ((rows + TILE_H - 1) / TILE_H);
    // 16-byte accesses need rows that start at multiples of 16 bytes (hipMalloc aligns the images; a caller's image may start anywhere)
    const bool vec = width % 4 == 0 && ((uintptr_t)cur | (uintptr_t)base | (uintptr_t)direct) % 16 == 0;
    if (have_base) { if (vec) launch_tiles<true, true>(a, s); else launch_tiles<true, false>(a, s); }
    else           { if (vec) launch_tiles<false, true>(a, s); else launch_tiles<false, false>(a, s); }
}

// Gather columns [x0, x1) of the band-local rows [y0, y1) of `src` (`width` words per row) into `out`, rows of x1 - x0 words.
void launch_delta_pack(const uint32_t* src, int width, int x0, int x1, int y0, int y1, uint32_t* out, hipStream_t s) {
    if (x1 <= x0 || y1 <= y0) return;
    PackArgs a;
    a.src = src; a.out = out; a.width = width; a.x0 = x0; a.y0 = y0; a.w = x1 - x0;
    const bool vec = width % 4 == 0 && x0 % 4 == 0 && ((uintptr_t)src | (uintptr_t)out) % 16 == 0;
    const uint64_t units = (uint64_t)(y1 - y0) * (uint64_t)(vec ? a.w / 4 : a.w);
    a.units = (uint32_t)units;
    const unsigned blocks = (unsigned)std::min<uint64_t>((units + DELTA_THREADS - 1) / DELTA_THREADS, 4096u);
    if (vec) hipLaunchKernelGGL((k_delta_pack<true>), dim3(blocks), dim3(DELTA_THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_delta_pack<false>), dim3(blocks), dim3(DELTA_THREADS), 0, s, a);
}

}  // namespace swr
