// The host side of the item bounds (software-renderer_amd/csrc/swr_api.hip: band_item_bounds, the cut, the group path,
// swr_item_bounds) on the fake HIP runtime of tests/host/hip_stub, under the address and undefined-behaviour sanitizers.  The stand-in
// of swr::launch_item_bounds (hip_stub/stub_launch.cpp) is a plain CPU loop over the stream slots of the items it is handed, run as a
// "kernel" of the fake stream; it also checks the work units and the ranges.  The fake upload builds no stream, so the scene is skinned and posed: the stand-in skin launch then writes the
// stream, slot s = primitive s, and the loop reads real corners (a range resolved wrongly is a wrong record, one past the stream an
// out-of-bounds read the address sanitizer reports).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ \
//       software-renderer_amd/csrc/swr_api.hip tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp \
//       tests/host/item_bounds_host_test.cpp -lpthread
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <string>
#include <unistd.h>
#include <vector>

#include "host_test.h"
#include "../../software-renderer_amd/csrc/swr_internal.h"

static const float INF = std::numeric_limits<float>::infinity();

// ---- the scene: skinned and posed, so that the fake stream holds the posed corners in index order -----------------------------------
static const int NV = 900, NTRI = 5000;     // more than two work units in one item
static std::string g_trace;

static int stream_builds() {                // launch_build_stream is the one "kernel" line of the trace after the upload: uploads + cuts
    std::ifstream in(g_trace);
    std::string line;
    int n = 0;
    while (std::getline(in, line)) n += line.rfind("kernel ", 0) == 0 ? 1 : 0;
    return n;
}

struct Posed { Scene s; std::vector<float> pose; std::vector<float> xyz; };     // xyz: the posed positions, 3 floats per vertex
static Posed make_posed() {
    Posed p;
    p.s = make_scene(NV, NTRI, 2);
    p.s.v[17].xyz[1] = std::numeric_limits<float>::quiet_NaN();             // its triangles are skipped, the others stay
    p.pose = make_pose(3, 0.02f);
    p.xyz.resize(3 * (size_t)NV);
    for (int i = 0; i < NV; i++) blend(p.s.v[i].xyz, p.s.sk[i], p.pose.data(), true, &p.xyz[3 * (size_t)i]);
    return p;
}

static void persp(float* m, float tag) {    // w = 0.5 + z: the scene's z in [0.1, 0.2] stays in front; shifted by `tag`
    tagm(m, 1.0f);
    m[12] = tag; m[11] = 1.0f; m[15] = 0.5f;
}

static swr_draw_item item(int64_t first_tri, int64_t tris, const float* m) {
    swr_draw_item it{};
    it.first_index = 3 * first_tri; it.index_count = 3 * tris;
    memcpy(it.transform, m, sizeof it.transform);
    return it;
}

static std::vector<swr_item_bound> expect(const Posed& p, const std::vector<swr_draw_item>& items, int W, int H, uint32_t flags) {
    std::vector<swr_item_bound> want;
    for (const swr_draw_item& it : items) {
        const int64_t* idx = p.s.idx.data() + it.first_index;
        want.push_back(fold(it.index_count / 3, [&](int64_t t, int j) { return &p.xyz[3 * (size_t)idx[3 * t + j]]; }, it.transform, W, H,
                            (flags & SWR_FLAG_METAL_RULES) != 0));
    }
    return want;
}

static void bounds(swr_context* c, const Posed& p, const std::vector<swr_draw_item>& items, int W, int H, uint32_t flags) {
    const std::vector<swr_item_bound> want = expect(p, items, W, H, flags);
    std::vector<swr_item_bound> got(items.size() + 1);
    memset(got.data(), 0x5A, got.size() * sizeof(swr_item_bound));
    const swr_item_bound guard = got.back();
    CHECK(swr_item_bounds(c, items.data(), (int32_t)items.size(), flags, got.data()) == SWR_OK);
    CHECK(memcmp(got.data(), want.data(), want.size() * sizeof(swr_item_bound)) == 0);
    CHECK(memcmp(&got.back(), &guard, sizeof guard) == 0);
}

static std::vector<swr_draw_item> item_set() {
    float a[16], b[16], far[16];
    tagm(a, 1.0f); persp(b, 0.1f); tagm(far, 1.0f); far[12] = 7.0f;             // far: wholly right of the target
    return {item(0, NTRI, a), item(0, 1, a), item(63, 65, b), item(100, 2048, b), item(100, 2049, a), item(7, 0, a), item(NTRI, 0, b),
            item(100, 2048, far), item(4999, 1, b), item(2000, 3000, a), item(100, 2048, b)};
}

static void upload(swr_context* c, const Posed& p) {
    CHECK(swr_scene_upload(c, p.s.v.data(), NV, p.s.idx.data(), 3 * NTRI) == SWR_OK);
    CHECK(swr_scene_skin(c, p.s.sk.data(), NV) == SWR_OK);
    CHECK(swr_pose_set(c, p.pose.data(), 3) == SWR_OK);
}

static void scenario(uint32_t devices, int W, int H) {
    const Posed p = make_posed();
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int bands = (int)std::max<uint32_t>(devices, 1);
    const std::vector<swr_draw_item> items = item_set();
    const int32_t n = (int32_t)items.size();
    std::vector<swr_item_bound> keep(items.size());
    memset(keep.data(), 0xA5, keep.size() * sizeof(swr_item_bound));
    const std::vector<swr_item_bound> untouched = keep;
    auto kept = [&] { return memcmp(keep.data(), untouched.data(), keep.size() * sizeof(swr_item_bound)) == 0; };
    // before a scene, and before a target
    CHECK(swr_item_bounds(c, items.data(), n, 0, keep.data()) == SWR_ERR_NO_SCENE);
    upload(c, p);
    CHECK(swr_item_bounds(c, items.data(), n, 0, keep.data()) == SWR_ERR_NO_SCENE);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    CHECK(swr_context_bands(c) == bands);
    // the cut: requested by the first call, on band 0 alone; the same list again and the list drawn find it in place (the other
    // bands of a group cut when they draw the list)
    {
        const int launches = g_bounds_launches.load(), builds = stream_builds();
        bounds(c, p, items, W, H, 0);
        CHECK(stream_builds() == builds + 1);
        CHECK(g_bounds_launches.load() == launches + 1);                     // band 0 alone launches
        bounds(c, p, items, W, H, SWR_FLAG_METAL_RULES);
        bounds(c, p, items, W, H, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR | SWR_FLAG_CULL_BACK | SWR_FLAG_PRIMITIVE_IDS | SWR_FLAG_LOAD);
        CHECK(swr_draw_list(c, items.data(), n, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        CHECK(swr_sync(c) == SWR_OK);
        bounds(c, p, items, W, H, 0);
        CHECK(stream_builds() == builds + bands);
        CHECK(g_bounds_launches.load() == launches + 4);
        // a new boundary is a new cut; the frame drawn before stays what it was
        std::vector<float> before((size_t)W * H), after((size_t)W * H);
        CHECK(swr_read_depth(c, before.data()) == SWR_OK);
        float m[16];
        tagm(m, 1.0f);
        bounds(c, p, {item(1234, 77, m)}, W, H, 0);
        CHECK(stream_builds() == builds + bands + 1);
        CHECK(swr_read_depth(c, after.data()) == SWR_OK);
        CHECK(before == after && all_eq(after, 1.0f));
    }
    // n == 0: legal with NULL pointers, launches nothing, writes nothing
    {
        const int launches = g_bounds_launches.load();
        CHECK(swr_item_bounds(c, nullptr, 0, 0, nullptr) == SWR_OK);
        CHECK(swr_item_bounds(c, items.data(), 0, SWR_FLAG_METAL_RULES, keep.data()) == SWR_OK);
        CHECK(kept() && g_bounds_launches.load() == launches);
    }
    // the staging grows, shrinks and starts from zero: 1 item, SWR_DRAW_LIST_MAX, 2
    {
        float m[16];
        tagm(m, 1.0f);
        bounds(c, p, {item(0, NTRI, m)}, W, H, 0);
        std::vector<swr_draw_item> many;
        for (int k = 0; k < SWR_DRAW_LIST_MAX; k++) many.push_back(item(100 + (k % 3) * 948, k % 5 == 4 ? 0 : 948 + (k % 2), m));
        bounds(c, p, many, W, H, 0);
        bounds(c, p, {item(63, 65, m), item(7, 0, m)}, W, H, SWR_FLAG_METAL_RULES);
        bounds(c, p, items, W, H, 0);
    }
    // every refusal of the header; nothing is written, and the context goes on working
    {
        float m[16];
        tagm(m, 1.0f);
        CHECK(swr_item_bounds(nullptr, items.data(), n, 0, keep.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_item_bounds(c, nullptr, n, 0, keep.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_item_bounds(c, items.data(), n, 0, nullptr) == SWR_ERR_BAD_ARG);
        CHECK(swr_item_bounds(c, items.data(), -1, 0, keep.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_item_bounds(c, items.data(), n, 1u << 9, keep.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_item_bounds(c, items.data(), n, 1u << 20, keep.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_item_bounds(c, items.data(), n, SWR_FLAG_DEPTH_CLIP, keep.data()) == SWR_ERR_UNSUPPORTED);
        CHECK(swr_item_bounds(c, items.data(), n, SWR_FLAG_DEPTH_CLIP | SWR_FLAG_DEPTH_TEST, keep.data()) == SWR_ERR_UNSUPPORTED);
        std::vector<swr_draw_item> bad = items;
        bad[3].first_index += 1;
        CHECK(swr_item_bounds(c, bad.data(), n, 0, keep.data()) == SWR_ERR_INDEX_COUNT);
        bad = items; bad[3].index_count -= 1;
        CHECK(swr_item_bounds(c, bad.data(), n, 0, keep.data()) == SWR_ERR_INDEX_COUNT);
        bad = items; bad[5] = item(NTRI, 1, m);
        CHECK(swr_item_bounds(c, bad.data(), n, 0, keep.data()) == SWR_ERR_BAD_ARG);
        bad = items; bad[5] = item(-1, 1, m);
        CHECK(swr_item_bounds(c, bad.data(), n, 0, keep.data()) == SWR_ERR_BAD_ARG);
        bad = items; bad[5] = item(0, -1, m);
        CHECK(swr_item_bounds(c, bad.data(), n, 0, keep.data()) == SWR_ERR_BAD_ARG);
        std::vector<swr_draw_item> too_many((size_t)SWR_DRAW_LIST_MAX + 1, item(0, 1, m));
        std::vector<swr_item_bound> big(too_many.size());
        memset(big.data(), 0xA5, big.size() * sizeof(swr_item_bound));
        CHECK(swr_item_bounds(c, too_many.data(), (int32_t)too_many.size(), 0, big.data()) == SWR_ERR_UNSUPPORTED);
        CHECK(memcmp(&big.front(), &untouched.front(), sizeof(swr_item_bound)) == 0 && memcmp(&big.back(), &untouched.front(), sizeof(swr_item_bound)) == 0);
        CHECK(kept());
        bounds(c, p, items, W, H, 0);
    }
    swr_context_destroy(c);
}

// a context that owns one band of a larger target answers for the full W x H
static void one_band_of_a_target() {
    const Posed p = make_posed();
    swr_config cfg{0, 1, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    upload(c, p);
    CHECK(swr_target_set(c, 80, 160, 32, 96) == SWR_OK);
    bounds(c, p, item_set(), 80, 160, 0);
    CHECK(swr_target_set(c, 80, 160, 96, 96) == SWR_OK);       // no rows at all
    bounds(c, p, item_set(), 80, 160, SWR_FLAG_METAL_RULES);
    swr_context_destroy(c);
}

// a failed context returns its sticky error and writes nothing
static void failed_context(uint32_t devices) {
    const Posed p = make_posed();
    swr_config cfg{0, devices, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    upload(c, p);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    float m[16];
    tagm(m, 1.0f);
    const swr_draw_item it = item(0, 300, m);
    swr_item_bound got;
    memset(&got, 0xA5, sizeof got);
    const swr_item_bound untouched = got;
    CHECK(swr_item_bounds(c, &it, 1, 0, &got) == SWR_OK);
    CHECK(got.drawable + got.skipped == 300);
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, SWR_FLAG_DEPTH_TEST);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    got = untouched;
    CHECK(swr_item_bounds(c, &it, 1, 0, &got) == SWR_ERR_HIP);
    CHECK(memcmp(&got, &untouched, sizeof got) == 0);
    swr_context_destroy(c);
}

int main() {
    char path[] = "/tmp/swr_item_bounds_trace_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) { std::printf("FAIL mkstemp\n"); return 1; }
    close(fd);
    g_trace = path;
    setenv("FAKE_HIP_TRACE", path, 1);      // (read once, by the fake runtime's first enqueue)
    fake_kernel_delay_us(0);
    scenario(1, 200, 136);
    scenario(3, 200, 136);
    one_band_of_a_target();
    failed_context(1);
    failed_context(2);
    CHECK(g_launch_fails.load() == 0);
    unlink(path);
    return report("item bounds host test");
}
