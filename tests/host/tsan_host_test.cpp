// Thread-sanitizer run of the C-ABI's HOST layer (software-renderer_amd/csrc/swr_api.hip: helper threads, host-paced
// stream ordering, the present / regrow / failure protocols) on a fake HIP runtime (tests/host/hip_stub/): streams are
// host threads, kernels are stand-ins that tag the framebuffer with the frame's transform[0].  No GPU, no pixels: what is
// checked is ORDER (every host image shows the frame it was presented for), the error protocol, and that TSan stays silent.
//   g++ -std=c++17 -O1 -g -fsanitize=thread -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/tsan_host_test.cpp -lpthread
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_test.h"

static bool no_pipeline = false;      // --no-pipeline: every context runs with swr_pipeline_enable(0), one stream

static const int W = 128, H = 96;
static std::vector<swr_vertex> verts(300);
static std::vector<int64_t> idx(300);
static bool all_eq(const float* d, float v, int r0 = 0, int r1 = H) {
    for (int i = r0 * W; i < r1 * W; i++) if (d[i] != v) return false;
    return true;
}

static void resident(uint32_t devices) {
    swr_config cfg{0, devices, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    if (no_pipeline) CHECK(swr_pipeline_enable(c, 0) == SWR_OK);
    CHECK(swr_scene_upload(c, verts.data(), 300, idx.data(), 300) == SWR_OK);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    float m[16];
    std::vector<float> d(W * H);
    // a long un-waited burst (crosses the working-set ring and the 64-deep raster ring), then one read
    for (int f = 1; f <= 300; f++) { tagm(m, (float)f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR) == SWR_OK); }
    CHECK(swr_read_depth(c, d.data()) == SWR_OK);
    CHECK(all_eq(d.data(), 300.0f));
    // draw + present into four page-locked images and a pageable one, no wait in between
    float* img[5];
    for (int k = 0; k < 4; k++) img[k] = (float*)swr_host_alloc(W * H * 4);
    std::vector<float> pageable(W * H);
    img[4] = pageable.data();
    for (int round = 0; round < 6; round++) {
        for (int k = 0; k < 5; k++) {
            tagm(m, (float)(1000 + 10 * round + k));
            CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR) == SWR_OK);
            CHECK(swr_present(c, nullptr, img[k]) == SWR_OK);
        }
        CHECK(swr_present_wait(c) == SWR_OK);
        for (int k = 0; k < 5; k++) CHECK(all_eq(img[k], (float)(1000 + 10 * round + k)));
    }
    // one frame at a time (the idle-inline path), timing on and off, pipelining off and on
    for (int f = 0; f < 20; f++) {
        if (f == 5) CHECK(swr_timing_enable(c, 2) == SWR_OK);
        if (f == 10) CHECK(swr_pipeline_enable(c, 0) == SWR_OK);
        if (f == 15) { CHECK(swr_pipeline_enable(c, no_pipeline ? 0 : 1) == SWR_OK); CHECK(swr_timing_enable(c, 0) == SWR_OK); }
        tagm(m, (float)(2000 + f));
        CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR) == SWR_OK);
        CHECK(swr_sync(c) == SWR_OK);
    }
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d.data(), 2019.0f));
    // a tile region overflows in the middle of a presented burst: the earlier frame is reported, the last one repaired
    swr::g_fake_fill.store(5000);
    tagm(m, 3001.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR) == SWR_OK); CHECK(swr_present(c, nullptr, img[0]) == SWR_OK);
    tagm(m, 3002.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR) == SWR_OK); CHECK(swr_present(c, nullptr, img[1]) == SWR_OK);
    CHECK(swr_present_wait(c) == SWR_ERR_FRAME_DROPPED);
    CHECK(swr_present_wait(c) == SWR_OK);
    CHECK(all_eq(img[1], 3002.0f));
    swr::g_fake_fill.store(7);
    // swr_render with a scene identity
    swr_render_pass rp{};
    rp.depth = img[2]; rp.width = W; rp.height = H; rp.vertices = verts.data(); rp.vertex_count = 300; rp.indices = idx.data(); rp.index_count = 300;
    rp.flags = SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR; rp.scene_id = 42;
    swr_render_times rt{};
    for (int f = 0; f < 4; f++) {
        tagm(rp.transform, (float)(4000 + f));
        CHECK(swr_render(c, &rp) == SWR_OK);
        CHECK(swr_render_timings(c, &rt) == SWR_OK && rt.scene_cached == (f > 0));
        CHECK(all_eq(img[2], (float)(4000 + f)));
    }
    // ... and without one: the one-shot upload builds the stream on the binning stream, chunk by chunk behind the index copy
    setenv("SWR_ONESHOT_MIN_TRIS", "64", 1);
    rp.scene_id = 0; rp.index_count = 300;
    for (int f = 0; f < 3; f++) {
        tagm(rp.transform, (float)(5000 + f));
        CHECK(swr_render(c, &rp) == SWR_OK);
        CHECK(swr_render_timings(c, &rt) == SWR_OK && rt.scene_cached == 0);
        CHECK(all_eq(img[2], (float)(5000 + f)));
    }
    unsetenv("SWR_ONESHOT_MIN_TRIS");
    // destroy with work in flight
    for (int f = 0; f < 40; f++) { tagm(m, 1.0f); swr_draw(c, m, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR); if (f % 3 == 0) swr_present(c, nullptr, img[3]); }
    swr_context_destroy(c);
    for (int k = 0; k < 4; k++) swr_host_free(img[k]);
}

static void failure(uint32_t devices, int fault) {
    swr_config cfg{0, devices, 150, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    CHECK(swr_scene_upload(c, verts.data(), 300, idx.data(), 300) == SWR_OK);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    float m[16];
    tagm(m, 1.0f);
    for (int f = 0; f < 6; f++) CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR) == SWR_OK);
    CHECK(swr_sync(c) == SWR_OK);
    CHECK(swr_debug_fault(c, fault) == SWR_OK);
    const auto t0 = std::chrono::steady_clock::now();
    for (int f = 0; f < 80; f++) swr_draw(c, m, SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR);      // beyond the 64-deep raster ring: must not hang
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    CHECK(s < 8.0);
    CHECK(strlen(swr_last_error(c)) > 10);
    CHECK(swr_sync(c) == SWR_ERR_HIP);                       // sticky
    std::vector<float> d(W * H);
    CHECK(swr_read_depth(c, d.data()) == SWR_ERR_HIP);
    swr_context_destroy(c);                                  // returns
}

// Every frame type the draw entry points size buffers and bins for — draw lists, depth-clip frames, perspective tables, ID images,
// load frames — on a 100-triangle scene and then a 3 000-triangle one on the same context: every lane buffer and the bins grow
// once, with plain frames still in flight in front of the draw that grows them.  The stand-in kernels touch both ends of every
// table they are handed (stub_launch.cpp), so a table sized or grown wrongly is a sanitizer report; the tags check the order.
static void frame_types(int bin_mode) {
    swr_config cfg{0, 0, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    if (no_pipeline) CHECK(swr_pipeline_enable(c, 0) == SWR_OK);
    CHECK(swr_debug_set(c, SWR_DEBUG_BIN_MODE, bin_mode) == SWR_OK);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    std::vector<float> d(W * H);
    std::vector<uint32_t> ids(W * H);
    float m[16], tag = 100.0f * (float)(bin_mode + 1);
    const uint32_t Z = SWR_FLAG_DEPTH_TEST;
    auto in_flight = [&] { tagm(m, 1.0f); for (int k = 0; k < 2; k++) CHECK(swr_draw(c, m, Z | SWR_FLAG_NO_COLOR) == SWR_OK); };
    auto shows = [&](float t) { CHECK(swr_read_depth(c, d.data()) == SWR_OK); CHECK(all_eq(d.data(), t)); };
    for (const int64_t ntri : {(int64_t)100, (int64_t)3000}) {
        std::vector<swr_vertex> v((size_t)ntri * 3);
        std::vector<swr_vertex_attr> a((size_t)ntri * 3, swr_vertex_attr{{0, 0, 1, 0}, {0.5f, 0.5f, 0, 0}});
        std::vector<int64_t> ix((size_t)ntri * 3);
        for (size_t i = 0; i < v.size(); i++) { ix[i] = (int64_t)i; v[i] = swr_vertex{{0.1f * (float)(i % 7), 0.2f, 0.5f, 0}, {1, 1, 1, 0}}; }
        CHECK(swr_material_set(c, nullptr) == SWR_OK);
        CHECK(swr_scene_upload(c, v.data(), (int64_t)v.size(), ix.data(), (int64_t)ix.size()) == SWR_OK);
        // three items whose frame slots are not their stream slots; the last one through a perspective matrix
        swr_draw_item it[3];
        const int64_t q = ntri / 4;
        const int64_t first[3] = {2 * q, 0, q + 1};
        for (int k = 0; k < 3; k++) { it[k].first_index = 3 * first[k]; it[k].index_count = 3 * (q - 1); tagm(it[k].transform, 0.0f); }
        it[2].transform[3] = 0.25f;
        auto list = [&](uint32_t flags) { it[0].transform[0] = ++tag; CHECK(swr_draw_list(c, it, 3, flags) == SWR_OK); };
        in_flight(); list(Z | SWR_FLAG_PERSPECTIVE); shows(tag);
        in_flight(); list(Z | SWR_FLAG_PERSPECTIVE | SWR_FLAG_DEPTH_CLIP); shows(tag);
        swr_material phong{};
        phong.shader = SWR_SHADER_PHONG; phong.shininess_log2 = 4; phong.light_dir[2] = phong.half_dir[2] = 1.0f; phong.diffuse = 1.0f;
        in_flight();
        CHECK(swr_scene_attributes(c, a.data(), (int64_t)a.size()) == SWR_OK);
        CHECK(swr_material_set(c, &phong) == SWR_OK);
        in_flight();
        tagm(m, ++tag); m[3] = 0.25f;
        CHECK(swr_draw(c, m, Z | SWR_FLAG_DEPTH_CLIP | SWR_FLAG_PERSPECTIVE) == SWR_OK); shows(tag);
        in_flight();
        tagm(m, ++tag);
        CHECK(swr_draw(c, m, Z | SWR_FLAG_PRIMITIVE_IDS) == SWR_OK);
        CHECK(swr_read_ids(c, ids.data()) == SWR_OK); shows(tag);
        in_flight(); list(Z | SWR_FLAG_LOAD); shows(tag);
    }
    // more crossing triangles than a clip frame has slots for: swr_sync grows the fans and redraws the frame
    in_flight();
    swr::g_fake_clip_over.store(100);
    tagm(m, ++tag); m[3] = 0.25f;
    CHECK(swr_draw(c, m, Z | SWR_FLAG_DEPTH_CLIP | SWR_FLAG_PERSPECTIVE) == SWR_OK);
    CHECK(swr_sync(c) == SWR_OK);
    CHECK(swr::g_fake_clip_over.load() == 0);
    shows(tag);
    // a tile region of a draw-list frame overflows: repaired the same way
    swr_draw_item one{0, 3 * 2000, {}};
    tagm(one.transform, ++tag);
    swr::g_fake_fill.store(5000); swr::g_fake_pairs.store(200000);     // (nothing in flight: every frame that runs now reports it)
    CHECK(swr_draw_list(c, &one, 1, Z) == SWR_OK);
    CHECK(swr_sync(c) == SWR_OK);
    shows(tag);
    swr::g_fake_fill.store(7); swr::g_fake_pairs.store(1000);
    swr_context_destroy(c);
}

// --no-failure: without the failure sections; --single: one device, stand-in kernels without delay, SWR_LANES as the environment
// has it (with FAKE_HIP_TRACE and --no-failure: a run whose sequence of runtime calls does not depend on timing)
int main(int argc, char** argv) {
    bool no_failure = false, single = false;
    for (int k = 1; k < argc; k++) {
        if (!strcmp(argv[k], "--no-failure")) no_failure = true;
        else if (!strcmp(argv[k], "--single")) single = true;
        else if (!strcmp(argv[k], "--no-pipeline")) no_pipeline = true;
        else { std::printf("unknown switch %s\n", argv[k]); return 2; }
    }
    for (int i = 0; i < 300; i++) { idx[i] = i; verts[i] = swr_vertex{{0.1f * (float)(i % 7), 0.2f, 0.5f, 0}, {1, 1, 1, 0}}; }
    const char* const env_lanes = getenv("SWR_LANES");
    const std::string keep = env_lanes ? env_lanes : "1";
    for (const char* lanes : {"1", "0"}) {       // frame lanes (the default) and the two-stream pipeline with its helper threads
        if (single && keep != lanes) continue;
        setenv("SWR_LANES", lanes, 1);
        for (int delay : {0, 15, 150}) {         // kernels that finish before / while / long after the host enqueues the next
            if (single && delay) continue;
            fake_kernel_delay_us(delay);
            resident(0);
            if (!single) resident(3);
        }
        fake_kernel_delay_us(single ? 0 : 15);
        for (int bin_mode : {0, 1}) frame_types(bin_mode);      // fixed-stride bins, exact-size bins
        for (int fault = 1; fault <= 2 && !no_failure; fault++) { failure(0, fault); failure(2, fault); }
    }
    return report("tsan host test");
}
