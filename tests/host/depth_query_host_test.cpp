// The host side of the depth queries (software-renderer_amd/csrc/swr_api.hip: band_query_depth, the group fan-out and sum,
// swr_query_depth) on the fake HIP runtime of tests/host/hip_stub, under the address and undefined-behaviour sanitizers.  The stand-in
// of swr::launch_depth_query (stub_launch.cpp) is a plain CPU loop over the header's definition run as a "kernel" of the fake stream.  The depth image is a pattern written with swr_target_write, so the
// loop reads the band's own rows (a box clipped wrongly is an out-of-bounds read the address sanitizer reports, or a wrong count).
// The loop also checks what the host hands it next to the boxes: the list of large boxes and the total area of the band's parts.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/depth_query_host_test.cpp -lpthread
#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "host_test.h"

// the depth of pixel (x, y) of the full target: ordinary depths, +inf, NaN and -inf
static float pattern(int x, int y) {
    const uint32_t v = ((uint32_t)x * 7u + (uint32_t)y * 13u + ((uint32_t)x >> 3) * ((uint32_t)y >> 2)) % 23u;
    if (v == 20u) return std::numeric_limits<float>::infinity();
    if (v == 21u) return std::numeric_limits<float>::quiet_NaN();
    if (v == 22u) return -std::numeric_limits<float>::infinity();
    return (float)v / 20.0f;
}

static swr_depth_box box(int x0, int y0, int x1, int y1, float z) { return swr_depth_box{x0, y0, x1, y1, z, {0, 0, 0}}; }

// what the header defines, over the pattern, for the rows the bands own
static std::vector<uint32_t> expect(const Bands& b, const std::vector<swr_depth_box>& boxes) {
    std::vector<uint32_t> want(boxes.size(), 0);
    for (size_t i = 0; i < boxes.size(); i++)
        for (size_t k = 0; k < b.r0.size(); k++)
            for (int64_t y = std::max<int64_t>(boxes[i].y0, b.r0[k]); y < std::min<int64_t>(boxes[i].y1, b.r1[k]); y++)
                for (int x = boxes[i].x0; x < boxes[i].x1; x++) want[i] += boxes[i].z < pattern(x, (int)y) ? 1u : 0u;
    return want;
}

static void query(swr_context* c, const Bands& b, const std::vector<swr_depth_box>& boxes) {
    const std::vector<uint32_t> want = expect(b, boxes);
    std::vector<uint32_t> got(boxes.size(), 0xA5A5A5A5u);
    CHECK(swr_query_depth(c, boxes.data(), (int64_t)boxes.size(), got.data()) == SWR_OK);
    CHECK(got == want);
    std::vector<uint32_t> again(boxes.size(), 0x5A5A5A5Au);
    CHECK(swr_query_depth(c, boxes.data(), (int64_t)boxes.size(), again.data()) == SWR_OK);       // the same query again
    CHECK(again == want);
}

static void write_pattern(swr_context* c, int W, int H) {
    std::vector<float> d((size_t)W * H);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) d[(size_t)y * W + x] = pattern(x, y);
    CHECK(swr_target_write(c, nullptr, d.data()) == SWR_OK);
}

static const float INF = std::numeric_limits<float>::infinity();
static const float QNAN = std::numeric_limits<float>::quiet_NaN();

static std::vector<swr_depth_box> box_set(int W, int H) {
    // the whole target at several depths, inside one band, across band borders, columns, one pixel, empty ones, repeats
    std::vector<swr_depth_box> v;
    for (float z : {0.5f, -1.0f, 2.0f, 0.0f, -0.0f, INF, -INF, QNAN, 0.25f}) v.push_back(box(0, 0, W, H, z));
    const int rects[][4] = {{3, 70, 97, 100}, {1, 50, 66, 150}, {0, 0, W, 40}, {W - 1, 0, W, H}, {0, H - 1, W, H}, {37, 64, 38, 65},
                            {37, 63, 38, 64}, {10, 20, 10, 90}, {10, 20, 60, 20}, {0, 0, 0, 0}, {W, H, W, H}, {3, 70, 97, 100}};
    for (const auto& r : rects)
        for (float z : {0.5f, 0.1f}) v.push_back(box(r[0], r[1], r[2], r[3], z));
    return v;
}

static void scenario(uint32_t devices, int W, int H) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    uint32_t out[4] = {7, 7, 7, 7};
    const swr_depth_box one = box(0, 0, 1, 1, 0.5f);
    CHECK(swr_query_depth(c, &one, 1, out) == SWR_ERR_NO_SCENE);         // before a target
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    const Bands b = bands_of(c);
    CHECK((int)b.r0.size() == (devices > 1 ? (int)devices : 1));
    write_pattern(c, W, H);
    const std::vector<swr_depth_box> boxes = box_set(W, H);
    query(c, b, boxes);
    // n == 0: legal with NULL pointers, launches nothing
    {
        const int before = g_query_launches.load();
        CHECK(swr_query_depth(c, nullptr, 0, nullptr) == SWR_OK);
        CHECK(swr_query_depth(c, boxes.data(), 0, out) == SWR_OK);
        CHECK(out[0] == 7);
        // boxes that miss every band's rows, or are empty, launch nothing and give zeros
        std::vector<swr_depth_box> miss = {box(5, 7, 5, 90, 0.5f), box(0, 0, W, 0, 0.5f)};
        query(c, b, miss);
        CHECK(g_query_launches.load() == before);
        if (devices == 3) {             // rows of the first band only: one launch per query
            std::vector<swr_depth_box> first = {box(0, 0, W, (int)b.r1[0], 0.5f)};
            std::vector<uint32_t> got(1);
            CHECK(swr_query_depth(c, first.data(), 1, got.data()) == SWR_OK);
            CHECK(g_query_launches.load() == before + 1);
            CHECK(got == expect(b, first));
        }
    }
    // the staging grows and shrinks and starts from zero: few boxes, many, few again; a band the small query misses holds zeros, not
    // what the large one left there
    {
        std::vector<swr_depth_box> many;
        for (int k = 0; k < 5000; k++) many.push_back(box(k % (W - 3), (k * 7) % (H - 2), k % (W - 3) + 3, (k * 7) % (H - 2) + 2, (float)(k % 21) / 20.0f));
        query(c, b, {box(0, 0, W, H, 0.5f)});
        query(c, b, many);
        query(c, b, {box(1, 1, W - 1, 9, 0.3f), box(0, 0, W, H, 0.5f)});
        query(c, b, {box(2, 2, 9, 9, 0.3f)});
        std::vector<swr_depth_box> max_n((size_t)SWR_DEPTH_QUERY_MAX, box(5, 5, 6, 7, 0.5f));
        query(c, b, max_n);
        query(c, b, boxes);
    }
    // every refusal of the header; nothing is written, and the context goes on working
    {
        std::vector<swr_depth_box> bad = boxes;
        std::vector<uint32_t> keep(bad.size() + 1, 0xA5A5A5A5u);
        const int64_t n = (int64_t)bad.size();
        const int launches = g_query_launches.load();           // a refused call touches no band: nothing is launched on any of them
        CHECK(swr_query_depth(nullptr, bad.data(), n, keep.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_query_depth(c, nullptr, n, keep.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_query_depth(c, bad.data(), n, nullptr) == SWR_ERR_BAD_ARG);
        CHECK(swr_query_depth(c, bad.data(), -1, keep.data()) == SWR_ERR_BAD_ARG);
        std::vector<swr_depth_box> too_many((size_t)SWR_DEPTH_QUERY_MAX + 1, box(0, 0, 1, 1, 0.5f));
        std::vector<uint32_t> big(too_many.size(), 0xA5A5A5A5u);
        CHECK(swr_query_depth(c, too_many.data(), (int64_t)too_many.size(), big.data()) == SWR_ERR_UNSUPPORTED);
        CHECK(big[0] == 0xA5A5A5A5u && big.back() == 0xA5A5A5A5u);
        const int wrong[][4] = {{0, 0, W + 1, H}, {0, 0, W, H + 1}, {-1, 0, W, H}, {0, -1, W, H}, {50, 0, 49, H}, {0, 90, W, 89}, {W + 1, 0, W + 1, H}};
        const size_t at = bad.size() / 2;           // a bad box in the middle of a good list: its index is in the message
        for (const auto& r : wrong) {
            bad = boxes; bad[at] = box(r[0], r[1], r[2], r[3], 0.5f); bad[at + 2] = box(-5, 0, 1, 1, 0.5f);
            CHECK(swr_query_depth(c, bad.data(), n, keep.data()) == SWR_ERR_BAD_ARG);
            CHECK(std::string(swr_last_error(c)).find("box " + std::to_string(at) + ":") != std::string::npos);
        }
        for (int k = 0; k < 3; k++) {
            bad = boxes; bad[at + 1].reserved[k] = 1;
            CHECK(swr_query_depth(c, bad.data(), n, keep.data()) == SWR_ERR_BAD_ARG);
            CHECK(std::string(swr_last_error(c)).find("box " + std::to_string(at + 1) + ":") != std::string::npos);
        }
        bool untouched = true;
        for (uint32_t v : keep) untouched = untouched && v == 0xA5A5A5A5u;
        CHECK(untouched);
        CHECK(g_query_launches.load() == launches);
        query(c, b, boxes);
    }
    // the images are the frame's: reading them and drawing on go on as before
    {
        std::vector<float> dep((size_t)W * H, 0.0f);
        CHECK(swr_read_depth(c, dep.data()) == SWR_OK);
        bool same = true;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const float p = pattern(x, y), d = dep[(size_t)y * W + x];
                same = same && memcmp(&p, &d, 4) == 0;
            }
        CHECK(same);
        query(c, b, boxes);
        // right after swr_target_set the depth is the cleared one: every pixel passes a finite z, none passes +inf or NaN
        CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
        const std::vector<swr_depth_box> q = {box(0, 0, W, H, 0.5f), box(0, 0, W, H, INF), box(0, 0, W, H, QNAN), box(3, 4, 30, 50, -INF)};
        std::vector<uint32_t> got(4, 7u);
        CHECK(swr_query_depth(c, q.data(), 4, got.data()) == SWR_OK);
        CHECK(got[0] == (uint32_t)(W * H) && got[1] == 0 && got[2] == 0 && got[3] == 27u * 46u);
    }
    swr_context_destroy(c);
}

// a context that owns one band of a larger target counts the part of every box in its rows
static void one_band_of_a_target() {
    swr_config cfg{0, 1, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int W = 80, H = 160;
    CHECK(swr_target_set(c, W, H, 32, 96) == SWR_OK);
    write_pattern(c, W, H);
    const Bands b = bands_of(c);
    CHECK(b.r0.size() == 1 && b.r0[0] == 32 && b.r1[0] == 96);
    query(c, b, {box(0, 0, W, H, 0.5f), box(5, 40, 70, 90, 0.5f), box(5, 0, 70, 32, 0.5f), box(5, 96, 70, 160, 0.5f), box(79, 95, 80, 96, -1.0f),
                 box(5, 31, 70, 33, -1.0f), box(5, 95, 70, 97, -1.0f)});
    const swr_depth_box outside = box(0, 0, W, H + 1, 0.5f);
    uint32_t got = 7;
    CHECK(swr_query_depth(c, &outside, 1, &got) == SWR_ERR_BAD_ARG);
    CHECK(got == 7);
    swr_context_destroy(c);
}

// a box of DEPTH_QUERY_SPLIT_AREA pixels or more in a band is listed as large, per band (the stand-in launch checks the list)
static void large_boxes(uint32_t devices) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int W = 1024, H = 600;
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    write_pattern(c, W, H);
    const Bands b = bands_of(c);
    query(c, b, {box(0, 0, 10, 10, 0.5f), box(0, 0, W, H, 0.5f), box(0, 0, W, 128, 0.5f), box(0, 0, W, 127, 0.5f), box(1, 1, W, H, QNAN),
                 box(0, 0, W, H, 0.5f), box(0, 100, 512, 400, 0.2f)});
    swr_context_destroy(c);
}

// a failed context returns its sticky error
static void failed_context(uint32_t devices) {
    swr_config cfg{0, devices, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    std::vector<swr_vertex> verts(300);
    std::vector<int64_t> idx(300);
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (int64_t)i;
    CHECK(swr_scene_upload(c, verts.data(), 300, idx.data(), 300) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    float m[16];
    for (int k = 0; k < 16; k++) m[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_sync(c) == SWR_OK);
    const swr_depth_box q = box(0, 0, 64, 64, 0.5f);
    uint32_t got = 7;
    CHECK(swr_query_depth(c, &q, 1, &got) == SWR_OK);
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, SWR_FLAG_DEPTH_TEST);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    got = 7;
    CHECK(swr_query_depth(c, &q, 1, &got) == SWR_ERR_HIP);
    CHECK(got == 7);
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    scenario(1, 100, 200);
    scenario(3, 100, 200);
    one_band_of_a_target();
    large_boxes(1);
    large_boxes(3);
    failed_context(1);
    failed_context(2);
    CHECK(g_launch_fails.load() == 0);
    return report("depth query host test");
}
