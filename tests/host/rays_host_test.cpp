// The host side of the ray casts (software-renderer_amd/csrc/swr_api.hip: check_rays, band_cast_rays, swr_cast_rays) on the fake HIP
// runtime of tests/host/hip_stub, under the address and undefined-behaviour sanitizers.  The stand-in of swr::launch_cast_rays is the
// launch set's (hip_stub/stub_launch.cpp): a CPU loop that reads every ray, every stream slot, every group box and, when the stream is
// reordered, every inv entry it is handed, writes every key word and every hit, and notes what it was handed and when.  Its hits echo
// the rays (hip_stub/stub_launch.h: ray_echo), so that the program sees the upload in front of the launch and the read-back behind it.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/rays_host_test.cpp -lpthread
#include <cmath>
#include <string>
#include <vector>

#include "host_test.h"

static std::vector<swr_ray> make_rays(size_t n, float salt) {
    std::vector<swr_ray> r(n);
    for (size_t k = 0; k < n; k++)
        r[k] = swr_ray{{0.25f * (float)(k % 13) + salt, -1.0f + 0.001f * (float)(k % 997), 2.0f}, 0.125f * (float)(k % 5),
                       {0.0f, (k % 2) ? 0.5f : -0.0f, -1.0f - (float)(k % 3)}, 10.0f + (float)(k % 7)};
    return r;
}

// one successful call: the hits are the stand-in's for exactly these rays, from one launch on the first band over the whole scene
static const RayNote* g_last = nullptr;
static RayNote g_last_note;
static void cast_ok(swr_context* c, const std::vector<swr_ray>& rays, int64_t ntri, const char* what) {
    std::vector<swr_ray_hit> hits(rays.size() + 1, swr_ray_hit{0xA5A5A5A5u, -7.0f, -7.0f, -7.0f});
    (void)take_ray_notes();
    const int rc = swr_cast_rays(c, rays.data(), (int64_t)rays.size(), 0, hits.data());
    const std::vector<RayNote> notes = take_ray_notes();
    if (rc != SWR_OK || notes.size() != 1 || !notes[0].ran) {
        std::printf("FAIL %s: rc %d (%s), %zu launches\n", what, rc, swr_last_error(c), notes.size()); fails++; g_last = nullptr; return;
    }
    g_last_note = notes[0]; g_last = &g_last_note;
    const swr::RaysArgs& a = notes[0].a;
    bool ok = a.n == (int64_t)rays.size() && a.ntri == ntri && (ntri == 0 || (a.tri_xyz && a.box64));
    for (size_t k = 0; ok && k < rays.size(); k++) {
        const swr_ray_hit e = ray_echo(rays[k], (int64_t)k, ntri);
        ok = memcmp(&hits[k], &e, sizeof e) == 0;
    }
    ok = ok && hits[rays.size()].primitive == 0xA5A5A5A5u;      // nothing behind the n-th hit is written
    if (!ok) { std::printf("FAIL %s: the hits are not the launch's\n", what); fails++; }
}

// every refusal: the code, the ray's index in the message, nothing launched, nothing written
static void refusals(swr_context* c, bool have_scene) {
    std::vector<swr_ray> rays = make_rays(5, 0.0f);
    std::vector<swr_ray_hit> hits(5, swr_ray_hit{0xA5A5A5A5u, -7.0f, -7.0f, -7.0f});
    const int launches = g_ray_launches.load();
    CHECK(swr_cast_rays(nullptr, rays.data(), 5, 0, hits.data()) == SWR_ERR_BAD_ARG);
    if (!have_scene) {
        CHECK(swr_cast_rays(c, rays.data(), 5, 0, hits.data()) == SWR_ERR_NO_SCENE);
        CHECK(swr_cast_rays(c, nullptr, 0, 0, nullptr) == SWR_ERR_NO_SCENE);
    } else {
        CHECK(swr_cast_rays(c, rays.data(), -1, 0, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_cast_rays(c, nullptr, 5, 0, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_cast_rays(c, rays.data(), 5, 0, nullptr) == SWR_ERR_BAD_ARG);
        CHECK(swr_cast_rays(c, rays.data(), 5, 1, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_cast_rays(c, rays.data(), 5, 0x80000000u, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_cast_rays(c, rays.data(), (int64_t)SWR_RAYS_MAX + 1, 0, hits.data()) == SWR_ERR_UNSUPPORTED);     // (refused before a ray is read)
        const float bad[3] = {NAN, INFINITY, -INFINITY};
        for (int word = 0; word < 8; word++)
            for (float b : bad) {
                std::vector<swr_ray> r = rays;
                reinterpret_cast<float*>(&r[3])[word] = b;
                CHECK(swr_cast_rays(c, r.data(), 5, 0, hits.data()) == SWR_ERR_BAD_ARG);
                CHECK(std::string(swr_last_error(c)).find("swr_cast_rays: ray 3:") != std::string::npos);
            }
        std::vector<swr_ray> r = rays;
        r[4].dir[0] = 0.0f; r[4].dir[1] = -0.0f; r[4].dir[2] = 0.0f;
        CHECK(swr_cast_rays(c, r.data(), 5, 0, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("swr_cast_rays: ray 4: the direction is zero") != std::string::npos);
        CHECK(swr_cast_rays(c, r.data(), 4, 0, hits.data()) == SWR_OK);                                             // (the first four are fine)
        for (int k = 0; k < 4; k++) hits[(size_t)k] = swr_ray_hit{0xA5A5A5A5u, -7.0f, -7.0f, -7.0f};
        (void)take_ray_notes();
        r = rays;
        r[0].tmin = 2.0f; r[0].tmax = 1.0f;
        CHECK(swr_cast_rays(c, r.data(), 5, 0, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("swr_cast_rays: ray 0: tmin") != std::string::npos);
        r[0].tmin = 1.0f;                                                                                           // tmin == tmax is legal
        CHECK(swr_cast_rays(c, r.data(), 1, 0, hits.data()) == SWR_OK);
        hits[0] = swr_ray_hit{0xA5A5A5A5u, -7.0f, -7.0f, -7.0f};
        (void)take_ray_notes();
        CHECK(g_ray_launches.load() == launches + 2);
    }
    if (!have_scene) CHECK(g_ray_launches.load() == launches);
    for (const swr_ray_hit& h : hits) CHECK(h.primitive == 0xA5A5A5A5u && h.t == -7.0f);
    expect_no_launch("refused ray casts");
}

static void scenario(uint32_t devices) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int B = (int)devices;
    const int nv = 300, ntri = 64 * 3 + 17;
    const Scene s = make_scene(nv, ntri, 2);
    const std::vector<float> A = make_pose(3, 0.25f), Bp = make_pose(4, -0.5f);
    float m[16];
    std::vector<float> d((size_t)64 * 192);
    refusals(c, false);
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    // no target is needed; n == 0 succeeds without a launch, whatever the pointers
    {
        const int launches = g_ray_launches.load();
        swr_ray_hit h{0xA5A5A5A5u, 0, 0, 0};
        CHECK(swr_cast_rays(c, nullptr, 0, 0, nullptr) == SWR_OK);
        CHECK(swr_cast_rays(c, make_rays(1, 0.0f).data(), 0, 0, &h) == SWR_OK && h.primitive == 0xA5A5A5A5u);
        CHECK(g_ray_launches.load() == launches);
    }
    cast_ok(c, make_rays(7, 0.5f), ntri, "a scene without a target");
    CHECK(swr_target_set(c, 64, 192, 0, 192) == SWR_OK);
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    CHECK(swr_pose_set(c, A.data(), 3) == SWR_OK);
    expect_stream(s, nullptr, nullptr, A.data(), false, B, "pose A");
    // every refusal leaves scene and pose: no stream launch, and the next cast reads the stream pose A wrote
    refusals(c, true);
    const int streams = g_stream_launches.load();
    cast_ok(c, make_rays(65, 1.0f), ntri, "65 rays in pose A");
    CHECK(g_last && g_last->streams_before == streams && g_stream_launches.load() == streams);     // after the pose's stream launches, and none of its own
    const swr::RaysArgs first = g_last ? g_last->a : swr::RaysArgs{};
    // regrowth: 1 ray, SWR_RAYS_MAX rays, 1 ray again — the large call's buffers are kept
    cast_ok(c, make_rays(1, 2.0f), ntri, "1 ray");
    cast_ok(c, make_rays((size_t)SWR_RAYS_MAX, 3.0f), ntri, "SWR_RAYS_MAX rays");
    const swr::RaysArgs big = g_last ? g_last->a : swr::RaysArgs{};
    cast_ok(c, make_rays(1, 4.0f), ntri, "1 ray after the largest call");
    CHECK(g_last && g_last->a.rays == big.rays && g_last->a.keys == big.keys && g_last->a.hits == big.hits);
    CHECK(g_last && g_last->a.tri_xyz == first.tri_xyz && g_last->a.box64 == first.box64);            // the resident stream, every time
    // behind an un-waited frame: the frame completes as it was posted; and behind an overflowed one, which is repaired first
    tagm(m, 3.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    cast_ok(c, make_rays(64, 5.0f), ntri, "behind an un-waited frame");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 3.0f));
    swr::g_fake_fill.store(5000);
    tagm(m, 4.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    cast_ok(c, make_rays(63, 6.0f), ntri, "behind an overflowed frame");
    swr::g_fake_fill.store(7);
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 4.0f));
    // behind a depth-clip frame and a draw list that cuts the stream: still the resident stream
    tagm(m, 5.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST | SWR_FLAG_DEPTH_CLIP) == SWR_OK);
    cast_ok(c, make_rays(3, 7.0f), ntri, "behind a depth-clip frame");
    CHECK(g_last && g_last->a.tri_xyz == first.tri_xyz && g_last->a.box64 == first.box64);
    {
        swr_draw_item items[2] = {{0, 3 * (int64_t)(ntri / 2), {}}, {3 * (int64_t)(ntri / 2), 3 * (int64_t)(ntri - ntri / 2), {}}};
        tagm(items[0].transform, 6.0f); tagm(items[1].transform, 6.0f);
        CHECK(swr_draw_list(c, items, 2, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        cast_ok(c, make_rays(3, 8.0f), ntri, "behind a draw list");
        CHECK(g_last && g_last->a.tri_xyz == first.tri_xyz && g_last->a.ntri == ntri);
        (void)take_records();       // (the cut restreams the scene in its pose)
    }
    // the call changes nothing: the next pose is the model's
    CHECK(swr_pose_set(c, Bp.data(), 4) == SWR_OK);
    expect_stream(s, nullptr, nullptr, Bp.data(), false, B, "pose B after the casts");
    cast_ok(c, make_rays(2, 9.0f), ntri, "pose B");
    // a scene without triangles: legal, every ray misses, nothing is launched over no groups (the stand-in is handed ntri 0)
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), 2) == SWR_OK);
    cast_ok(c, make_rays(4, 10.0f), 0, "a scene without triangles");
    CHECK(g_last && g_last->a.groups == 0);
    swr_context_destroy(c);
}

// a failed context returns its sticky error
static void failed_context(uint32_t devices) {
    swr_config cfg{0, devices, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const Scene s = make_scene(300, 100, 2);
    CHECK(swr_scene_upload(c, s.v.data(), 300, s.idx.data(), 300) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    float m[16];
    tagm(m, 1.0f);
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, SWR_FLAG_DEPTH_TEST);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    const int launches = g_ray_launches.load();
    std::vector<swr_ray> rays = make_rays(3, 0.0f);
    swr_ray_hit hits[3] = {{0xA5A5A5A5u, 0, 0, 0}, {0xA5A5A5A5u, 0, 0, 0}, {0xA5A5A5A5u, 0, 0, 0}};
    CHECK(swr_cast_rays(c, rays.data(), 3, 0, hits) == SWR_ERR_HIP);
    // (a group checks the call's arguments before its bands report, as every entry point that waits: fan in swr_api.hip)
    CHECK(swr_cast_rays(c, rays.data(), 3, 9, hits) == (devices == 1 ? SWR_ERR_HIP : SWR_ERR_BAD_ARG));
    CHECK(swr_cast_rays(c, nullptr, 0, 0, nullptr) == SWR_ERR_HIP);
    CHECK(g_ray_launches.load() == launches && hits[0].primitive == 0xA5A5A5A5u && hits[2].primitive == 0xA5A5A5A5u);
    (void)take_records();
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    scenario(1);
    scenario(3);
    failed_context(1);
    failed_context(2);
    CHECK(g_ray_launches.load() > 0);
    return report("rays host test");
}
