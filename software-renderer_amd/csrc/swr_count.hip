// swr_count.hip — visibility counts (include/swr.h "Visibility counts").
//
// k_count_ids reduces a rectangle of a band's ID image to one counter per primitive (or per draw item) plus one for SWR_ID_NONE.
// A streaming kernel: a wave takes 64 consecutive pixels of one row (256 contiguous bytes, one dword load per lane — the rectangle's
// x0 is arbitrary, so nothing wider is assumed to be aligned), and the waves of the grid stride over the rectangle's row segments.
//
// The cost is the add per pixel, not the read: neighbouring pixels mostly share an ID, so the wave reduces before it touches memory.
// A segment that holds ONE ID (one ballot against the first lane's) is not added at all: ID and length are carried in two wave-uniform
// registers into the wave's next segment and added when the ID changes or the wave is done (a large triangle behind a scene would
// otherwise send every segment's add to one address).  A mixed segment is reduced by one of two forms:
//   the leader loop: the first lane still counting names its ID, the lanes that hold it ballot, the leader adds the popcount, they
//     all leave: one trip and one single-lane add per distinct ID;
//   run heads: a lane whose ID differs from its left neighbour's starts a run and adds its length, the distance to the next head in
//     the 64-bit ballot of heads or to the end of the segment: one pass, no loop; an ID that comes back later pays a second add.
// Chosen by measurement (SWR_TUNE_COUNT_REDUCE): per primitive the leader loop (fewer global atomics, about 10 % less
// per call), per item run heads (every head searches its item in its own lane; the leader loop searches one ID at a time: 5 to 8 x slower).
// Per primitive the counters are a global array of n + 1 words, zeroed by the caller on the same stream, added to with no-return
// integer atomics.  Per item the counters (at most SWR_DRAW_LIST_MAX + 1) and the items' vbase live in LDS (32 KB): the item of a
// group is looked up once, by the binary search list_find / swr_clip.hip use (the last item whose vbase is <= the ID: empty items share
// their base with the next one), the adds are LDS atomics, and a workgroup flushes only its non-zero counters, one global atomic each.
// All arithmetic is integer: the result is exact and does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "swr_internal.h"

namespace swr {

namespace {

#ifndef SWR_TUNE_COUNT_REDUCE
#define SWR_TUNE_COUNT_REDUCE (-1)          // the reduction of a mixed segment: -1 = leader loop per primitive, run heads per item
                                            // (the product); 0 = run heads for both, 1 = leader loop for both (A/B builds)
#endif

constexpr int COUNT_THREADS = 256;
constexpr int COUNT_WAVES = COUNT_THREADS / 64;
constexpr int COUNT_SEGS_PER_WAVE = 16;     // row segments a wave walks when the grid is not capped

struct CountArgs {
    const uint32_t* ids;        // the band's ID image, `pitch` words per row
    uint32_t pitch;
    uint32_t x0, w;             // columns [x0, x0 + w) of every row
    uint32_t y0;                // first band-local row
    uint32_t segs_per_row;      // ceil(w / 64)
    uint32_t nseg;              // rows * segs_per_row
    const ListItem* items;      // PER_ITEM: the last frame's items on the device; NULL: the frame was no draw list (one item, vbase 0)
    uint32_t* counters;         // [n + 1], the last one counts SWR_ID_NONE
    uint32_t n;                 // primitives, or PER_ITEM items (<= SWR_DRAW_LIST_MAX)
};

// one add for `len` pixels that hold `id`
template <bool PER_ITEM>
__device__ __forceinline__ void add_group(const CountArgs& a, uint32_t* s_cnt, const uint32_t* s_vbase, uint32_t id, uint32_t len) {
    if (PER_ITEM) {
        uint32_t slot = a.n;
        if (id != SWR_ID_NONE) {
            if (a.n == 0) return;               // (a list without items draws nothing: every pixel is SWR_ID_NONE)
            uint32_t lo = 0, hi = a.n - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (s_vbase[mid] <= id) lo = mid; else hi = mid - 1;
            }
            slot = lo;
        }
        atomicAdd(&s_cnt[slot], len);
    } else {
        if (id != SWR_ID_NONE && id >= a.n) return;     // (no frame writes such an ID; it is dropped, the counters end at n)
        atomicAdd(&a.counters[id == SWR_ID_NONE ? a.n : id], len);
    }
}

template <bool PER_ITEM>
__global__ __launch_bounds__(COUNT_THREADS) void k_count_ids(CountArgs a) {
    __shared__ uint32_t s_vbase[PER_ITEM ? SWR_DRAW_LIST_MAX : 1];
    __shared__ uint32_t s_cnt[PER_ITEM ? SWR_DRAW_LIST_MAX + 1 : 1];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (PER_ITEM) {
        for (uint32_t k = threadIdx.x; k <= a.n; k += COUNT_THREADS) {
            s_cnt[k] = 0;
            if (k < a.n) s_vbase[k] = a.items ? a.items[k].vbase : 0u;
        }
        __syncthreads();
    }
    constexpr bool LEADER_LOOP = SWR_TUNE_COUNT_REDUCE < 0 ? !PER_ITEM : SWR_TUNE_COUNT_REDUCE != 0;
    uint32_t carry_id = 0, carry_len = 0;       // wave-uniform: the one-ID segments seen since the last add
    for (uint32_t seg = blockIdx.x * COUNT_WAVES + wave; seg < a.nseg; seg += gridDim.x * COUNT_WAVES) {   // (wave-uniform: every lane is active)
        const uint32_t row = seg / a.segs_per_row, sx = (seg - row * a.segs_per_row) * 64u + lane;
        const bool valid = sx < a.w;            // (the valid lanes of a segment are lanes [0, count), count >= 1)
        uint32_t id = SWR_ID_NONE;
        if (valid) id = a.ids[(size_t)(a.y0 + row) * a.pitch + a.x0 + sx];
        const unsigned long long live = __ballot(valid);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)id);
        if (__ballot(valid && id != first) == 0ull) {       // one ID: carried, not added
            if (carry_len && carry_id != first) {
                if (lane == 0) add_group<PER_ITEM>(a, s_cnt, s_vbase, carry_id, carry_len);
                carry_len = 0;
            }
            carry_id = first;
            carry_len += (uint32_t)__popcll(live);
            continue;
        }
        if (LEADER_LOOP) {
            // every predicate is explicit and every ballot is taken with all 64 lanes active; only the add is under a lane condition
            unsigned long long todo = live;
            while (todo) {
                const uint32_t lead_lane = (uint32_t)__builtin_ctzll(todo);
                const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)id, (int)lead_lane);
                const unsigned long long same = __ballot(valid && id == lead);
                if (lane == lead_lane) add_group<PER_ITEM>(a, s_cnt, s_vbase, lead, (uint32_t)__popcll(same));
                todo &= ~same;
            }
        } else {
            const uint32_t left = __shfl_up(id, 1);
            const bool head = valid && (lane == 0 || id != left);
            const unsigned long long heads = __ballot(head);
            if (head) {
                const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
                const uint32_t end = above ? lane + 1 + (uint32_t)__builtin_ctzll(above) : (uint32_t)__popcll(live);
                add_group<PER_ITEM>(a, s_cnt, s_vbase, id, end - lane);
            }
        }
    }
    if (carry_len && lane == 0) add_group<PER_ITEM>(a, s_cnt, s_vbase, carry_id, carry_len);
    if (PER_ITEM) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k <= a.n; k += COUNT_THREADS) {
            const uint32_t v = s_cnt[k];
            if (v) atomicAdd(&a.counters[k], v);
        }
    }
}

}  // namespace

// Count the rectangle [x0, x1) x [y0, y1) — band-local rows — of the band's ID image `ids` (`width` words per row) into
// counters[0 .. n], which the caller has zeroed on the same stream: counters[n] counts SWR_ID_NONE; per_item: counters[k] the IDs of
// item k of `items` (n of them, at most SWR_DRAW_LIST_MAX; NULL: one item that holds every ID), else counters[p] the ID p.
void launch_count_ids(const uint32_t* ids, int width, int x0, int x1, int y0, int y1, int per_item, const ListItem* items,
                      uint32_t* counters, int64_t n, hipStream_t s) {
    if (x1 <= x0 || y1 <= y0 || (per_item && n > SWR_DRAW_LIST_MAX)) return;
    CountArgs a;
    a.ids = ids; a.pitch = (uint32_t)width;
    a.x0 = (uint32_t)x0; a.w = (uint32_t)(x1 - x0); a.y0 = (uint32_t)y0;
    a.segs_per_row = (a.w + 63u) / 64u;
    a.nseg = (uint32_t)(y1 - y0) * a.segs_per_row;
    a.items = items; a.counters = counters; a.n = (uint32_t)n;
    const uint32_t per_block = COUNT_WAVES * COUNT_SEGS_PER_WAVE;
    // (per item every workgroup ends with a pass over its LDS counters: fewer, longer-lived workgroups)
    const uint32_t blocks = std::min<uint32_t>((a.nseg + per_block - 1) / per_block, per_item ? 512u : 2048u);
    if (per_item) hipLaunchKernelGGL((k_count_ids<true>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_count_ids<false>), dim3(blocks), dim3(COUNT_THREADS), 0, s, a);
}

}  // namespace swr
