// swr_frame_policy.h — where a frame's bins are sorted and which depth keys it takes, as pure functions of plain values.
// Host only: included by swr_api.hip (enqueue_frame) and by tests/host/frame_policy_test.cpp, never by a kernel source.
#pragma once
#include <stdint.h>
#include "../../include/swr.h"

// Where k_sort_bins runs.  On the binning stream it is part of the chain that runs ahead of the raster; on
// the raster stream (right before k_raster) the binning stream is free one kernel earlier.  Alternating A/B on
// one box (tools/ab_sort_stream.py, tools/bt_bands.sh; untimed frames of cfg4, us per frame):
//   whole 4K frame (4 080 tiles): 112 vs 122 -> binning stream;  half / quarter / eighth bands: 83 / 59 / 41
//   vs 73 / 49 / 40 -> raster stream;  light frames (cfg2, 6 k triangles): 37 vs 43 -> binning stream.
// -DSWR_TUNE_SORT_STREAM=0/1 forces either.
#ifndef SWR_TUNE_SORT_STREAM
#define SWR_TUNE_SORT_STREAM (-1)     // 0 / 1: k_sort_bins always on the binning / raster stream (tuning builds)
#endif
#ifndef SWR_TUNE_SORT_SPARSE
#define SWR_TUNE_SORT_SPARSE 0        // 1: launch k_sort_bins on sparse frames too
#endif

namespace swr {

struct FramePolicy {
    bool skip_sort = false, defer_big = false, insort = false;   // DeviceFrame's (insort: by policy_insort)
    bool k32 = false;                     // the frame's candidate bit for the 32-bit depth keys, settled
    bool k32_give_up = false;             // the scene belongs on the 64-bit keys from here on (the caller clears swr_context::k32_ok)
    bool sort_on_raster_stream = false;   // k_sort_bins right before k_raster instead of behind the binning chain
};

// fullest: the pinned word that holds the fullest bin of the latest binned frame (0xFFFFFFFF after a new scene or target: nothing
// known yet); redo: the sampled count of tiles the 32-bit keys had to raster again; k32: the frame's candidate bit;
// two_streams: binning and raster are enqueued on different streams.
inline FramePolicy frame_policy(uint32_t fullest, uint32_t redo, int tiles, int64_t ntri, uint32_t flags, bool k32, bool two_streams) {
    FramePolicy p;
    constexpr int sort_stream_mode = SWR_TUNE_SORT_STREAM;
    p.sort_on_raster_stream = sort_stream_mode >= 0 ? sort_stream_mode == 1 : (two_streams && ntri >= 200000 && tiles < 3000);
    // Sparse frames need no k_sort_bins: when the fullest bin of the latest binned frame (a pinned word k_fill_lds overwrites every
    // frame) fits two chunks, every tile of THIS frame is expected to be walked by all four waves together (row-split mode), where the
    // order inside the bin does not matter — k_raster masks the class tags itself.  A wrong guess costs time, never pixels.
    // (cfg5: 0.321 -> 0.313 ms, the app's sphere 18.6 -> 17.1 us; -DSWR_TUNE_SORT_SPARSE=1 sorts always.)
    constexpr bool sort_sparse = SWR_TUNE_SORT_SPARSE != 0;
    p.skip_sort = !sort_sparse && sort_stream_mode < 0 && fullest <= 128u;
    // bit 31 of that word: the latest rastered frame met triangles that cover hundreds of tiles — this frame's k_bin puts them on
    // the deferred list and k_sort_bins appends them per tile (swr_kernels.hip, BIN_BIG_TILES); 0xFFFFFFFF = nothing known yet
    p.defer_big = fullest != 0xFFFFFFFFu && (fullest & 0x80000000u);
    // a blend frame orders its bins itself (k_blend_order strips the class tags): no k_sort_bins, so nothing is deferred to it
    if (flags & SWR_FLAG_BLEND) { p.skip_sort = true; p.defer_big = false; }
    // 32-bit depth keys: one tile in REDO_SAMPLE (8) reports when it had to be rastered again (~6x the time of a tile that did
    // not); from 2 % of the tiles on the 64-bit kernel is the cheaper one for this scene
    p.k32_give_up = k32 && (uint64_t)redo * 8u * 50u > (uint64_t)tiles;
    p.k32 = k32 && !p.k32_give_up;
    return p;
}

// ... and on a small grid (a thin band: the frame is bound by its kernel chain, not by the chip) a frame on the 32-bit keys (uses_k32:
// frame_uses_k32 of the frame once p.k32 is in it) sorts its bins inside the raster workgroups, in the LDS the narrow keys leave free: no
// k_sort_bins launch — unless the frame defers triangles that cover hundreds of tiles, which k_sort_bins appends to the bins.  On a grid
// that fills the chip the launch is the cheaper place for the sort (swr_kernels.hip, raster_tile; profiles/r04/insort_ab.txt).
// (swr_debug_set SWR_DEBUG_RASTER_SORT, dbg_insort: 0 never, 1 by grid size, 2 always)
inline void policy_insort(FramePolicy& p, int tiles, bool uses_k32, int dbg_insort) {
    const bool insort_grid = dbg_insort == 2 || (dbg_insort == 1 && tiles <= 1536);
    if (insort_grid && uses_k32 && !p.defer_big && !p.skip_sort && SWR_TUNE_SORT_STREAM < 0) { p.insort = true; p.skip_sort = true; }
}

}  // namespace swr
