// swr_resolve.hip — supersampled resolve (include/swr.h "Supersampled resolve").
//
// The frame was drawn at S*w x S*h; k_resolve brings a band of it down to w x (band rows / S) with an S x S box filter:
//
//   colour   per channel (sum of the S*S bytes + S*S/2) / (S*S), integer — the four channels of a pixel are summed two at a time in
//            the 16-bit halves of a word (b and r in one, g and a in the other): the largest sum, 16 * 255 + 8 = 4088, stays below
//            2^12, so a half never carries into its neighbour, and what the shift moves down from the upper half is masked away
//   depth    the bits of sample (0,0), or the sequential minimum of the header (NaNs lose, the first of equal zeros is kept)
//
// A streaming kernel: one lane per output pixel, consecutive lanes on consecutive output columns, so a wave reads S runs of
// 64 * S * 4 contiguous bytes per image (one dwordx2 / dwordx4 load per lane and source row) and stores one run of 256 bytes.
// No LDS, no atomics, no cross-lane step.  Colour and depth go through one launch when both are wanted.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swr_internal.h"

namespace swr {

namespace {

constexpr int RESOLVE_THREADS = 256;

template <int S> struct SampleRow;
template <> struct SampleRow<2> { using type = uint2; };
template <> struct SampleRow<4> { using type = uint4; };

template <int S> __device__ __forceinline__ void unpack(const typename SampleRow<S>::type& v, uint32_t (&px)[S]);
template <> __device__ __forceinline__ void unpack<2>(const uint2& v, uint32_t (&px)[2]) { px[0] = v.x; px[1] = v.y; }
template <> __device__ __forceinline__ void unpack<4>(const uint4& v, uint32_t (&px)[4]) { px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w; }

// w: output pixels per row; npix: output pixels of the band (w * output rows).  The source band has S * w pixels per row and
// S output-rows-many times as many rows; both images are band-local, like the framebuffers.
template <int S, int DEPTH_FILTER, bool COLOR, bool DEPTH>
__global__ __launch_bounds__(RESOLVE_THREADS) void k_resolve(const uint32_t* __restrict__ color, const uint32_t* __restrict__ depth,
                                                             uint32_t* __restrict__ color_out, uint32_t* __restrict__ depth_out,
                                                             uint32_t w, uint32_t npix) {
    using Row = typename SampleRow<S>::type;
    constexpr int SHIFT = S == 2 ? 2 : 4;                       // 2 * log2 S
    constexpr uint32_t ROUND = (uint32_t)(S * S / 2) * 0x00010001u;
    const uint32_t gid = blockIdx.x * RESOLVE_THREADS + threadIdx.x;
    if (gid >= npix) return;
    const uint32_t y = gid / w, x = gid - y * w;
    const size_t pitch = (size_t)w * S;                         // source pixels per row
    const size_t first = (size_t)y * S * pitch + (size_t)x * S; // sample (0,0): a multiple of S pixels, so the row loads are aligned
    if (COLOR) {
        uint32_t br = 0, ga = 0;
#pragma unroll
        for (int j = 0; j < S; j++) {
            const Row v = *reinterpret_cast<const Row*>(color + first + (size_t)j * pitch);
            uint32_t px[S];
            unpack<S>(v, px);
#pragma unroll
            for (int i = 0; i < S; i++) {
                br += px[i] & 0x00FF00FFu;
                ga += (px[i] >> 8) & 0x00FF00FFu;
            }
        }
        br = ((br + ROUND) >> SHIFT) & 0x00FF00FFu;
        ga = ((ga + ROUND) >> SHIFT) & 0x00FF00FFu;
        color_out[gid] = br | (ga << 8);
    }
    if (DEPTH) {
        if (DEPTH_FILTER == SWR_RESOLVE_DEPTH_SAMPLE0) {
            depth_out[gid] = depth[first];
        } else {
            uint32_t mb = 0;
#pragma unroll
            for (int j = 0; j < S; j++) {
                const Row v = *reinterpret_cast<const Row*>(depth + first + (size_t)j * pitch);
                uint32_t px[S];
                unpack<S>(v, px);
#pragma unroll
                for (int i = 0; i < S; i++) {
                    if (i == 0 && j == 0) { mb = px[0]; continue; }
                    // the header's rule, as written: ordered compares only, so NaN, -0 / +0 and denormals behave as stated there
                    const float s = __uint_as_float(px[i]), m = __uint_as_float(mb);
                    if (s < m || (m != m && s == s)) mb = px[i];
                }
            }
            depth_out[gid] = mb;
        }
    }
}

template <int S, int DF>
void launch_resolve_sf(const uint32_t* color, const uint32_t* depth, uint32_t* color_out, uint32_t* depth_out, uint32_t w, uint32_t npix,
                       hipStream_t s) {
    const dim3 grid((npix + RESOLVE_THREADS - 1) / RESOLVE_THREADS), block(RESOLVE_THREADS);
    if (color && depth) hipLaunchKernelGGL((k_resolve<S, DF, true, true>), grid, block, 0, s, color, depth, color_out, depth_out, w, npix);
    else if (color) hipLaunchKernelGGL((k_resolve<S, 0, true, false>), grid, block, 0, s, color, depth, color_out, depth_out, w, npix);
    else hipLaunchKernelGGL((k_resolve<S, DF, false, true>), grid, block, 0, s, color, depth, color_out, depth_out, w, npix);
}

}  // namespace

// Resolve a band of `rows` source rows of `width` pixels (both multiples of `factor`, 2 or 4) into width / factor x rows / factor
// pixels.  color / depth: the band's source images, NULL = that image is not wanted (at least one is).
void launch_resolve(const void* color, const void* depth, void* color_out, void* depth_out, int width, int rows, int factor,
                    int depth_filter, hipStream_t s) {
    const uint32_t w = (uint32_t)(width / factor), npix = w * (uint32_t)(rows / factor);
    if (!npix || (!color && !depth)) return;
    const uint32_t* c = (const uint32_t*)color;
    const uint32_t* d = (const uint32_t*)depth;
    uint32_t* co = (uint32_t*)color_out;
    uint32_t* dz = (uint32_t*)depth_out;
    const bool mn = depth_filter == SWR_RESOLVE_DEPTH_MIN;
    if (factor == 2) {
        if (mn) launch_resolve_sf<2, SWR_RESOLVE_DEPTH_MIN>(c, d, co, dz, w, npix, s);
        else launch_resolve_sf<2, SWR_RESOLVE_DEPTH_SAMPLE0>(c, d, co, dz, w, npix, s);
    } else {
        if (mn) launch_resolve_sf<4, SWR_RESOLVE_DEPTH_MIN>(c, d, co, dz, w, npix, s);
        else launch_resolve_sf<4, SWR_RESOLVE_DEPTH_SAMPLE0>(c, d, co, dz, w, npix, s);
    }
}

}  // namespace swr
