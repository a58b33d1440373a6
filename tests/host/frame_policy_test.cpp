// The sort and depth-key policy of a frame (software-renderer_amd/csrc/swr_frame_policy.h: frame_policy, policy_insort) at the edges of
// its thresholds.  Pure functions of plain values: no HIP, no runtime, nothing but the header.  Every expected value below was read off
// the conditions as enqueue_frame had them before they moved into the header, not taken from a run of the functions.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/host/frame_policy_test.cpp -o frame_policy_test
#include <cstdio>
#include <initializer_list>

#include "../../software-renderer_amd/csrc/swr_frame_policy.h"

using swr::FramePolicy;
using swr::frame_policy;
using swr::policy_insort;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

// a frame nothing special is known about: a dense scene (fullest bin 1000), no redo, a 4K grid, one stream
static FramePolicy plain(uint32_t fullest, uint32_t flags = 0) { return frame_policy(fullest, 0, 4080, 100000, flags, false, false); }

static bool insort_fires(FramePolicy p, int tiles, bool uses_k32, int dbg) {
    const bool skipped = p.skip_sort;
    policy_insort(p, tiles, uses_k32, dbg);
    CHECK(p.skip_sort == (skipped || p.insort));      // a frame that sorts in the raster launches no k_sort_bins; nothing else changes it
    return p.insort;
}

int main() {
    // sparse frames: the fullest bin of the latest frame fits two chunks (128 entries)
    CHECK(plain(0).skip_sort && plain(128).skip_sort);
    CHECK(!plain(129).skip_sort && !plain(1000).skip_sort);
    CHECK(!plain(128).defer_big && !plain(129).defer_big);
    // nothing known yet: neither
    CHECK(!plain(0xFFFFFFFFu).skip_sort && !plain(0xFFFFFFFFu).defer_big);
    // bit 31: the latest frame met triangles that cover hundreds of tiles
    CHECK(plain(0x80000000u).defer_big && !plain(0x80000000u).skip_sort);
    CHECK(plain(0x80000005u).defer_big && plain(0xFFFFFFFEu).defer_big);
    CHECK(!plain(0x7FFFFFFFu).defer_big);
    // a blend frame orders its bins itself, whatever the word says
    for (const uint32_t fullest : {0u, 128u, 129u, 0x80000000u, 0x80000005u, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
        const FramePolicy p = plain(fullest, SWR_FLAG_BLEND);
        CHECK(p.skip_sort && !p.defer_big && !p.insort);
        const FramePolicy q = plain(fullest, SWR_FLAG_BLEND | SWR_FLAG_DEPTH_TEST | SWR_FLAG_LOAD);
        CHECK(q.skip_sort && !q.defer_big);
    }
    CHECK(!plain(1000, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR).skip_sort);      // (no other flag does)
    // the 32-bit keys are given up where redo * 8 * 50 > tiles
    {
        const FramePolicy a = frame_policy(1000, 1, 400, 100000, 0, true, false);       // 400 > 400: no
        CHECK(a.k32 && !a.k32_give_up);
        const FramePolicy b = frame_policy(1000, 2, 400, 100000, 0, true, false);       // 800 > 400
        CHECK(!b.k32 && b.k32_give_up);
        const FramePolicy c0 = frame_policy(1000, 0, 1, 100000, 0, true, false);        // 0 > 1: no
        CHECK(c0.k32 && !c0.k32_give_up);
        const FramePolicy c1 = frame_policy(1000, 1, 1, 100000, 0, true, false);        // 400 > 1
        CHECK(!c1.k32 && c1.k32_give_up);
        const FramePolicy big = frame_policy(1000, 0xFFFFFFFFu, 4080, 100000, 0, true, false);   // (64-bit product: no wrap)
        CHECK(!big.k32 && big.k32_give_up);
        // a frame that is no candidate neither takes the keys nor moves the scene's state
        const FramePolicy d = frame_policy(1000, 2, 400, 100000, 0, false, false);
        CHECK(!d.k32 && !d.k32_give_up);
        const FramePolicy e = frame_policy(1000, 0xFFFFFFFFu, 1, 100000, 0, false, false);
        CHECK(!e.k32 && !e.k32_give_up);
    }
    // the sort inside the raster workgroups: small grids, or always / never by the debug switch
    {
        const FramePolicy dense = plain(1000);
        CHECK(insort_fires(dense, 1536, true, 1) && !insort_fires(dense, 1537, true, 1));
        CHECK(insort_fires(dense, 1, true, 1));
        CHECK(!insort_fires(dense, 1, true, 0) && !insort_fires(dense, 1536, true, 0) && !insort_fires(dense, 100000, true, 0));
        CHECK(insort_fires(dense, 1, true, 2) && insort_fires(dense, 1537, true, 2) && insort_fires(dense, 100000, true, 2));
        // not without the 32-bit kernel, not with deferred triangles, not on a frame that launches no sort anyway
        CHECK(!insort_fires(dense, 1536, false, 1) && !insort_fires(dense, 1536, false, 2));
        CHECK(!insort_fires(plain(0x80000000u), 1536, true, 1) && !insort_fires(plain(0x80000000u), 1536, true, 2));
        CHECK(!insort_fires(plain(128), 1536, true, 1) && !insort_fires(plain(128), 1536, true, 2));
        CHECK(!insort_fires(plain(1000, SWR_FLAG_BLEND), 1536, true, 2));
        CHECK(insort_fires(plain(0xFFFFFFFFu), 1536, true, 1));      // (nothing known yet: the frame would launch a sort)
    }
    // k_sort_bins in front of the raster: only with two streams, from 200 000 triangles, below 3 000 tiles
    CHECK(frame_policy(1000, 0, 2999, 200000, 0, false, true).sort_on_raster_stream);
    CHECK(!frame_policy(1000, 0, 2999, 199999, 0, false, true).sort_on_raster_stream);
    CHECK(!frame_policy(1000, 0, 3000, 200000, 0, false, true).sort_on_raster_stream);
    CHECK(!frame_policy(1000, 0, 2999, 200000, 0, false, false).sort_on_raster_stream);
    CHECK(!frame_policy(1000, 0, 1, 1 << 24, 0, false, false).sort_on_raster_stream);
    CHECK(frame_policy(128, 0, 1, 1 << 24, SWR_FLAG_BLEND, true, true).sort_on_raster_stream);   // (decided by those three alone)
    if (failures) { std::printf("frame policy test: %d check(s) failed\n", failures); return 1; }
    std::printf("frame policy test: ok\n");
    return 0;
}
