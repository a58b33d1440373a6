// The host side of the visibility counts (software-renderer_amd/csrc/swr_api.hip: band_count_ids, the group fan-out and sum,
// swr_count_ids) on the fake HIP runtime of tests/host/hip_stub, under the address and undefined-behaviour sanitizers.  The stand-in
// of swr::launch_count_ids (stub_launch.cpp) is a plain CPU loop over the header's definition run as a "kernel" of the fake stream.  The stand-in raster leaves the ID image at zero, so the loop ADDS a pattern of
// its own to what it reads: the ID of band-local pixel (x, y) is ids[y][x] + pattern(x, y).  The band's rows are read (a rectangle
// clipped wrongly is an out-of-bounds read the address sanitizer reports, or a wrong count), the counters are added to, never
// assigned (a buffer that was not zeroed shows), and counters[n] is written (a buffer sized too small is reported).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/count_host_test.cpp -lpthread
#include <algorithm>
#include <string>
#include <vector>

#include "host_test.h"

// what the header defines, over the pattern: per band, the band-local rows of the rectangle
static void expect(const Bands& b, const swr_id_count& q, uint32_t total, const std::vector<uint32_t>& vbase /* per item; empty: per primitive */,
                   bool list, std::vector<uint32_t>& counts, uint32_t& none) {
    none = 0;
    for (uint32_t& v : counts) v = 0;
    for (size_t k = 0; k < b.r0.size(); k++)
        for (int64_t y = std::max<int64_t>(q.y0, b.r0[k]); y < std::min<int64_t>(q.y1, b.r1[k]); y++)
            for (int x = q.x0; x < q.x1; x++) {
                const uint32_t id = count_pattern((uint32_t)x, (uint32_t)(y - b.r0[k]), total);
                if (id == SWR_ID_NONE) { none++; continue; }
                if (q.group == SWR_COUNT_PER_PRIMITIVE) { counts[id]++; continue; }
                size_t slot = 0;
                if (list) for (size_t i = 0; i < vbase.size(); i++) if (vbase[i] <= id) slot = i;
                counts[slot]++;
            }
}

static const uint32_t Z = SWR_FLAG_DEPTH_TEST | SWR_FLAG_PRIMITIVE_IDS;
static void ident(float* m) { for (int k = 0; k < 16; k++) m[k] = (k % 5 == 0) ? 1.0f : 0.0f; }

static void upload(swr_context* c, int prims) {
    std::vector<swr_vertex> verts((size_t)prims * 3);
    std::vector<int64_t> idx((size_t)prims * 3);
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (int64_t)i;
    CHECK(swr_scene_upload(c, verts.data(), (int64_t)verts.size(), idx.data(), (int64_t)idx.size()) == SWR_OK);
}

// one query against the expectation; both the sum rule and every element
static void query(swr_context* c, const Bands& b, swr_id_count q, uint32_t total, const std::vector<uint32_t>& vbase, bool list, int64_t n) {
    std::vector<uint32_t> want((size_t)n), got((size_t)n, 0xA5A5A5A5u);
    uint32_t want_none = 0, got_none = 0xA5A5A5A5u;
    expect(b, q, total, vbase, list, want, want_none);
    CHECK(swr_count_ids(c, &q, n ? got.data() : nullptr, n, &got_none) == SWR_OK);
    CHECK(got == want);
    CHECK(got_none == want_none);
    uint64_t sum = got_none;
    for (uint32_t v : got) sum += v;
    CHECK(sum == (uint64_t)(q.x1 - q.x0) * (uint64_t)(q.y1 - q.y0));
    CHECK(swr_count_ids(c, &q, n ? got.data() : nullptr, n, nullptr) == SWR_OK);      // none may be NULL; the same query again
    CHECK(got == want);
}

static void scenario(uint32_t devices) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int W = 100, H = 200;
    float m[16];
    ident(m);
    swr_id_count whole{SWR_COUNT_PER_PRIMITIVE, 0, 0, W, H, {0, 0, 0}};
    uint32_t cnt[8] = {};
    // before a target
    CHECK(swr_count_ids(c, &whole, cnt, 1, nullptr) == SWR_ERR_NO_SCENE);
    upload(c, 100);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    const Bands b = bands_of(c);
    CHECK((int)b.r0.size() == (devices > 1 ? (int)devices : 1));
    // right after swr_target_set no frame has written IDs
    std::vector<uint32_t> big(100);
    CHECK(swr_count_ids(c, &whole, big.data(), 100, nullptr) == SWR_ERR_BAD_ARG);
    CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_count_ids(c, &whole, big.data(), 100, nullptr) == SWR_ERR_BAD_ARG);     // drawn without the flag
    CHECK(swr_draw(c, m, Z) == SWR_OK);
    g_count_total = 100;
    const std::vector<uint32_t> none_v;
    // rectangles: the whole target, inside one band, across band borders, missing the last band(s), columns, one pixel, empty ones
    const int rects[][4] = {{0, 0, W, H}, {3, 70, 97, 100}, {1, 50, 66, 150}, {0, 0, W, 40}, {99, 0, 100, H}, {0, 199, W, 200},
                            {37, 64, 38, 65}, {37, 63, 38, 64}, {10, 20, 10, 90}, {10, 20, 60, 20}, {0, 0, 0, 0}, {W, H, W, H}};
    for (const auto& r : rects) {
        for (int group : {SWR_COUNT_PER_PRIMITIVE, SWR_COUNT_PER_ITEM}) {
            swr_id_count q{group, r[0], r[1], r[2], r[3], {0, 0, 0}};
            query(c, b, q, 100, none_v, false, group == SWR_COUNT_PER_ITEM ? 1 : 100);
        }
    }
    // a rectangle that misses every band launches nothing
    {
        const int before = g_count_launches.load();
        swr_id_count q{SWR_COUNT_PER_PRIMITIVE, 5, 7, 5, 90, {0, 0, 0}};
        query(c, b, q, 100, none_v, false, 100);
        CHECK(g_count_launches.load() == before);
        if (devices == 3) {             // rows of the first band only: one launch per query
            swr_id_count one{SWR_COUNT_PER_PRIMITIVE, 0, 0, W, (int)b.r1[0], {0, 0, 0}};
            uint32_t nn = 0;
            CHECK(swr_count_ids(c, &one, big.data(), 100, &nn) == SWR_OK);
            CHECK(g_count_launches.load() == before + 1);
        }
    }
    // every refusal of the header; nothing is written, and the context goes on working
    {
        std::vector<uint32_t> keep(100, 0xA5A5A5A5u);
        uint32_t nn = 0xA5A5A5A5u;
        CHECK(swr_count_ids(nullptr, &whole, keep.data(), 100, &nn) == SWR_ERR_BAD_ARG);
        CHECK(swr_count_ids(c, nullptr, keep.data(), 100, &nn) == SWR_ERR_BAD_ARG);
        CHECK(swr_count_ids(c, &whole, nullptr, 100, &nn) == SWR_ERR_BAD_ARG);
        swr_id_count q = whole;
        q.group = 2; CHECK(swr_count_ids(c, &q, keep.data(), 100, &nn) == SWR_ERR_BAD_ARG);
        q.group = -1; CHECK(swr_count_ids(c, &q, keep.data(), 100, &nn) == SWR_ERR_BAD_ARG);
        for (int k = 0; k < 3; k++) { q = whole; q.reserved[k] = 1; CHECK(swr_count_ids(c, &q, keep.data(), 100, &nn) == SWR_ERR_BAD_ARG); }
        const int bad[][4] = {{0, 0, W + 1, H}, {0, 0, W, H + 1}, {-1, 0, W, H}, {0, -1, W, H}, {50, 0, 49, H}, {0, 90, W, 89}, {W + 1, 0, W + 1, H}};
        for (const auto& r : bad) { q = whole; q.x0 = r[0]; q.y0 = r[1]; q.x1 = r[2]; q.y1 = r[3]; CHECK(swr_count_ids(c, &q, keep.data(), 100, &nn) == SWR_ERR_BAD_ARG); }
        for (int64_t n : {(int64_t)99, (int64_t)101, (int64_t)0, (int64_t)1, (int64_t)-1}) {
            CHECK(swr_count_ids(c, &whole, keep.data(), n, &nn) == SWR_ERR_BAD_ARG);
            if (n >= 0) CHECK(std::string(swr_last_error(c)).find("100 primitives") != std::string::npos);     // the message names the value
        }
        q = whole; q.group = SWR_COUNT_PER_ITEM;
        CHECK(swr_count_ids(c, &q, keep.data(), 2, &nn) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("1 draw items") != std::string::npos);
        CHECK(swr_count_ids(c, &q, keep.data(), 0, &nn) == SWR_ERR_BAD_ARG);
        bool untouched = nn == 0xA5A5A5A5u;
        for (uint32_t v : keep) untouched = untouched && v == 0xA5A5A5A5u;
        CHECK(untouched);
        query(c, b, whole, 100, none_v, false, 100);
    }
    // a draw list: per item with empty items in front, in the middle and at the end; per primitive over the list's total
    {
        swr_draw_item it[7] = {};
        const int64_t first[7] = {0, 30, 0, 60, 12, 0, 0}, count[7] = {0, 20, 0, 0, 40, 15, 0};     // (ranges overlap: 12..52 and 30..50)
        std::vector<uint32_t> vbase;
        uint32_t total = 0;
        for (int k = 0; k < 7; k++) {
            it[k].first_index = 3 * first[k]; it[k].index_count = 3 * count[k]; ident(it[k].transform);
            vbase.push_back(total); total += (uint32_t)count[k];
        }
        CHECK(swr_draw_list(c, it, 7, Z) == SWR_OK);
        g_count_total = total;
        for (const auto& r : rects) {
            swr_id_count q{SWR_COUNT_PER_ITEM, r[0], r[1], r[2], r[3], {0, 0, 0}};
            query(c, b, q, total, vbase, true, 7);
            q.group = SWR_COUNT_PER_PRIMITIVE;
            query(c, b, q, total, none_v, true, total);
        }
        swr_id_count q = whole; q.group = SWR_COUNT_PER_ITEM;
        std::vector<uint32_t> got(7);
        CHECK(swr_count_ids(c, &q, got.data(), 7, nullptr) == SWR_OK);
        CHECK(got[0] == 0 && got[2] == 0 && got[3] == 0 && got[6] == 0 && got[1] && got[4] && got[5]);
        CHECK(swr_count_ids(c, &q, got.data(), 6, nullptr) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("7 draw items") != std::string::npos);
        CHECK(swr_count_ids(c, &whole, got.data(), 100, nullptr) == SWR_ERR_BAD_ARG);      // (the scene's count is not the list's)
        CHECK(std::string(swr_last_error(c)).find("75 primitives") != std::string::npos);
        // a list without items: n == 0 in both groups, counts may be NULL
        CHECK(swr_draw_list(c, nullptr, 0, Z) == SWR_OK);
        g_count_total = 0;
        for (int group : {SWR_COUNT_PER_PRIMITIVE, SWR_COUNT_PER_ITEM}) {
            swr_id_count e{group, 2, 3, 71, 181, {0, 0, 0}};
            uint32_t nn = 0;
            CHECK(swr_count_ids(c, &e, nullptr, 0, &nn) == SWR_OK);
            CHECK(nn == 69u * 178u);
            CHECK(swr_count_ids(c, &e, got.data(), 1, &nn) == SWR_ERR_BAD_ARG);
        }
    }
    // the counters shrink, grow and start from zero: a smaller scene, then a much larger one, then the first again
    for (int prims : {10, 5000, 100}) {
        upload(c, prims);
        CHECK(swr_draw(c, m, Z) == SWR_OK);
        g_count_total = (uint32_t)prims;
        query(c, b, whole, (uint32_t)prims, none_v, false, prims);
        swr_id_count q{SWR_COUNT_PER_ITEM, 1, 1, W - 1, H - 1, {0, 0, 0}};
        query(c, b, q, (uint32_t)prims, none_v, false, 1);
        q.group = SWR_COUNT_PER_PRIMITIVE;
        query(c, b, q, (uint32_t)prims, none_v, false, prims);
    }
    // the images are the frame's: reading them and drawing on go on as before; swr_target_write / swr_target_set end the IDs' validity
    {
        std::vector<uint32_t> ids((size_t)W * H, 1u);
        CHECK(swr_read_ids(c, ids.data()) == SWR_OK);
        query(c, b, whole, 100, none_v, false, 100);
        std::vector<float> dep((size_t)W * H, 0.5f);
        CHECK(swr_target_write(c, nullptr, dep.data()) == SWR_OK);
        CHECK(swr_count_ids(c, &whole, big.data(), 100, nullptr) == SWR_ERR_BAD_ARG);
        CHECK(swr_draw(c, m, Z | SWR_FLAG_LOAD) == SWR_OK);
        query(c, b, whole, 100, none_v, false, 100);
        CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
        CHECK(swr_count_ids(c, &whole, big.data(), 100, nullptr) == SWR_ERR_BAD_ARG);
    }
    swr_context_destroy(c);
}

// a context that owns one band of a larger target counts the part of the rectangle in its rows
static void one_band_of_a_target() {
    swr_config cfg{0, 1, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    upload(c, 40);
    CHECK(swr_target_set(c, 80, 160, 32, 96) == SWR_OK);
    float m[16];
    ident(m);
    CHECK(swr_draw(c, m, Z) == SWR_OK);
    g_count_total = 40;
    const Bands b = bands_of(c);
    const std::vector<uint32_t> none_v;
    const int rects[][4] = {{0, 0, 80, 160}, {5, 40, 70, 90}, {5, 0, 70, 32}, {5, 96, 70, 160}, {79, 95, 80, 96}};
    for (const auto& r : rects) {
        // (the sum rule holds for the part the band owns: compare element by element only)
        swr_id_count q{SWR_COUNT_PER_PRIMITIVE, r[0], r[1], r[2], r[3], {0, 0, 0}};
        std::vector<uint32_t> want(40), got(40, 7u);
        uint32_t wn = 0, gn = 7u;
        expect(b, q, 40, none_v, false, want, wn);
        CHECK(swr_count_ids(c, &q, got.data(), 40, &gn) == SWR_OK);
        CHECK(got == want && gn == wn);
    }
    swr_id_count q{SWR_COUNT_PER_PRIMITIVE, 0, 0, 80, 161, {0, 0, 0}};
    uint32_t got[40];
    CHECK(swr_count_ids(c, &q, got, 40, nullptr) == SWR_ERR_BAD_ARG);
    swr_context_destroy(c);
}

// a failed context returns its sticky error
static void failed_context(uint32_t devices) {
    swr_config cfg{0, devices, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    upload(c, 100);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    float m[16];
    ident(m);
    CHECK(swr_draw(c, m, Z) == SWR_OK);
    CHECK(swr_sync(c) == SWR_OK);
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, Z);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    swr_id_count q{SWR_COUNT_PER_PRIMITIVE, 0, 0, 64, 64, {0, 0, 0}};
    std::vector<uint32_t> got(100);
    CHECK(swr_count_ids(c, &q, got.data(), 100, nullptr) == SWR_ERR_HIP);
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    scenario(1);
    scenario(3);
    one_band_of_a_target();
    failed_context(1);
    failed_context(2);
    return report("count host test");
}
