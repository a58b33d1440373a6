// The host side of the ray queries (software-renderer_amd/csrc/swr_api.hip: check_ray_query, band_cast_rays, swr_query_rays) on the fake
// HIP runtime of tests/host/hip_stub, under the address and undefined-behaviour sanitizers.  The stand-in of swr::launch_cast_rays is the
// launch set's (hip_stub/stub_launch.cpp), used as it is: it refuses a launch whose groups are not those of the whole stream, reads every
// element it is handed, answers with an echo of the rays and notes the RaysArgs it was given, which is what this program looks at.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/ray_queries_host_test.cpp -lpthread
#include <cmath>
#include <string>
#include <vector>

#include "host_test.h"

static const swr_ray_hit UNTOUCHED{0xA5A5A5A5u, -7.0f, -7.0f, -7.0f};

static std::vector<swr_ray> make_rays(size_t n, float salt) {
    std::vector<swr_ray> r(n);
    for (size_t k = 0; k < n; k++)
        r[k] = swr_ray{{0.25f * (float)(k % 13) + salt, -1.0f + 0.001f * (float)(k % 997), 2.0f}, 0.125f * (float)(k % 5),
                       {0.0f, (k % 2) ? 0.5f : -0.0f, -1.0f - (float)(k % 3)}, 10.0f + (float)(k % 7)};
    return r;
}

// one successful query: one launch, on the first band, that ran; the hits are the stand-in's for exactly these rays; the RaysArgs of
// the launch in `out`
static bool query_ok(swr_context* c, const swr_ray_query* q, const std::vector<swr_ray>& rays, int64_t ntri, swr::RaysArgs& out,
                     const char* what) {
    std::vector<swr_ray_hit> hits(rays.size() + 1, UNTOUCHED);
    (void)take_ray_notes();
    const int rc = swr_query_rays(c, q, rays.data(), (int64_t)rays.size(), hits.data());
    const std::vector<RayNote> notes = take_ray_notes();
    if (rc != SWR_OK || notes.size() != 1 || !notes[0].ran) {
        std::printf("FAIL %s: rc %d (%s), %zu launches\n", what, rc, swr_last_error(c), notes.size()); fails++; return false;
    }
    out = notes[0].a;
    bool ok = out.n == (int64_t)rays.size() && out.ntri == ntri && out.groups == (ntri + 63) / 64;
    for (size_t k = 0; ok && k < rays.size(); k++) {
        const swr_ray_hit e = ray_echo(rays[k], (int64_t)k, ntri);
        ok = memcmp(&hits[k], &e, sizeof e) == 0;
    }
    ok = ok && memcmp(&hits[rays.size()], &UNTOUCHED, sizeof UNTOUCHED) == 0;       // nothing behind the n-th hit is written
    if (!ok) { std::printf("FAIL %s: the hits or the sizes are not the launch's\n", what); fails++; }
    return ok;
}

// what a launch was handed beyond the stream: flags and the resolved range
static void expect_query(swr_context* c, const swr_ray_query* q, int64_t ntri, uint32_t flags, int64_t p_begin, int64_t p_end,
                         const char* what) {
    swr::RaysArgs a{};
    if (!query_ok(c, q, make_rays(5, 0.5f), ntri, a, what)) return;
    if (a.flags != flags || a.p_begin != p_begin || a.p_end != p_end) {
        std::printf("FAIL %s: flags 0x%x range [%lld, %lld), not 0x%x [%lld, %lld)\n", what, (unsigned)a.flags, (long long)a.p_begin,
                    (long long)a.p_end, (unsigned)flags, (long long)p_begin, (long long)p_end);
        fails++;
    }
}

// every new refusal, and those carried over: the code, swr_query_rays in the message, nothing launched, nothing written
static void refusals(swr_context* c, bool have_scene, int64_t ntri) {
    std::vector<swr_ray> rays = make_rays(5, 0.0f);
    std::vector<swr_ray_hit> hits(5, UNTOUCHED);
    const int launches = g_ray_launches.load();
    const swr_ray_query fine{SWR_RAYS_ANY_HIT | SWR_RAYS_CULL_BACK, 0, 0, -1};
    CHECK(swr_query_rays(nullptr, &fine, rays.data(), 5, hits.data()) == SWR_ERR_BAD_ARG);
    CHECK(swr_query_rays(nullptr, nullptr, nullptr, 0, nullptr) == SWR_ERR_BAD_ARG);
    if (!have_scene) {
        CHECK(swr_query_rays(c, &fine, rays.data(), 5, hits.data()) == SWR_ERR_NO_SCENE);
        CHECK(swr_query_rays(c, nullptr, nullptr, 0, nullptr) == SWR_ERR_NO_SCENE);
        CHECK(std::string(swr_last_error(c)).find("swr_query_rays") != std::string::npos);
    } else {
        const swr_ray_query bad[] = {
            {16u, 0, 0, -1}, {0x80000000u, 0, 0, -1}, {SWR_RAYS_ANY_HIT | 0x100u, 0, 0, -1},                // unknown flag bits
            {0, 1u, 0, -1}, {SWR_RAYS_ANY_HIT, 0x80000000u, 0, -1},                                         // reserved
            {0, 0, -1, -1}, {0, 0, -1, 0}, {0, 0, INT64_MIN, -1},                                           // first_primitive < 0
            {0, 0, 0, -2}, {0, 0, 0, INT64_MIN},                                                            // primitive_count < -1
            {0, 0, 0, ntri + 1}, {0, 0, ntri, 1}, {0, 0, 1, ntri}, {0, 0, ntri + 1, 0}, {0, 0, ntri + 1, -1},   // beyond the scene
            {0, 0, INT64_MAX, INT64_MAX}, {0, 0, 1, INT64_MAX}, {0, 0, INT64_MAX, -1},
        };
        for (const swr_ray_query& q : bad) {
            CHECK(swr_query_rays(c, &q, rays.data(), 5, hits.data()) == SWR_ERR_BAD_ARG);
            CHECK(std::string(swr_last_error(c)).find("swr_query_rays:") != std::string::npos);
            CHECK(swr_query_rays(c, &q, nullptr, 0, nullptr) == SWR_ERR_BAD_ARG);                           // (n == 0 does not excuse a bad query)
        }
        CHECK(swr_query_rays(c, &fine, rays.data(), -1, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_query_rays(c, &fine, nullptr, 5, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_query_rays(c, &fine, rays.data(), 5, nullptr) == SWR_ERR_BAD_ARG);
        CHECK(swr_query_rays(c, nullptr, rays.data(), (int64_t)SWR_RAYS_MAX + 1, hits.data()) == SWR_ERR_UNSUPPORTED);
        const float nonfinite[3] = {NAN, INFINITY, -INFINITY};
        for (int word = 0; word < 8; word++)
            for (float b : nonfinite) {
                std::vector<swr_ray> r = rays;
                reinterpret_cast<float*>(&r[3])[word] = b;
                CHECK(swr_query_rays(c, &fine, r.data(), 5, hits.data()) == SWR_ERR_BAD_ARG);
                CHECK(std::string(swr_last_error(c)).find("swr_query_rays: ray 3:") != std::string::npos);
            }
        std::vector<swr_ray> r = rays;
        r[4].dir[0] = 0.0f; r[4].dir[1] = -0.0f; r[4].dir[2] = 0.0f;
        CHECK(swr_query_rays(c, nullptr, r.data(), 5, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("swr_query_rays: ray 4: the direction is zero") != std::string::npos);
        r = rays;
        r[0].tmin = 2.0f; r[0].tmax = 1.0f;
        CHECK(swr_query_rays(c, &fine, r.data(), 5, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("swr_query_rays: ray 0: tmin") != std::string::npos);
        // swr_cast_rays keeps refusing what it refused
        CHECK(swr_cast_rays(c, rays.data(), 5, 1, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(swr_cast_rays(c, rays.data(), 5, 9, hits.data()) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("swr_cast_rays: unknown flags") != std::string::npos);
    }
    CHECK(g_ray_launches.load() == launches);
    for (const swr_ray_hit& h : hits) CHECK(memcmp(&h, &UNTOUCHED, sizeof h) == 0);
    expect_no_launch("refused ray queries");
}

static bool same_args(const swr::RaysArgs& a, const swr::RaysArgs& b) {
    return a.tri_xyz == b.tri_xyz && a.box64 == b.box64 && a.inv == b.inv && a.reordered == b.reordered && a.ntri == b.ntri &&
           a.groups == b.groups && a.rays == b.rays && a.n == b.n && a.keys == b.keys && a.hits == b.hits && a.flags == b.flags &&
           a.p_begin == b.p_begin && a.p_end == b.p_end;
}

static void scenario(uint32_t devices) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int nv = 300;
    const int64_t ntri = 64 * 3 + 17;
    const Scene s = make_scene(nv, (int)ntri, 2);
    float m[16];
    std::vector<float> d((size_t)64 * 192);
    refusals(c, false, ntri);
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    // n == 0 succeeds without a launch, whatever the pointers, with and without a query
    {
        const int launches = g_ray_launches.load();
        const swr_ray_query q{SWR_RAYS_ANY_HIT, 0, 3, 4};
        swr_ray_hit h = UNTOUCHED;
        CHECK(swr_query_rays(c, nullptr, nullptr, 0, nullptr) == SWR_OK);
        CHECK(swr_query_rays(c, &q, make_rays(1, 0.0f).data(), 0, &h) == SWR_OK && h.primitive == 0xA5A5A5A5u);
        CHECK(g_ray_launches.load() == launches);
    }
    refusals(c, true, ntri);
    // a pose, so that every band's resident stream is on record: one stream launch per band, each into the band's own arrays
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    const std::vector<float> pose = make_pose(3, 0.25f);
    CHECK(swr_pose_set(c, pose.data(), 3) == SWR_OK);
    const std::vector<Record> streams = take_records();
    CHECK(streams.size() == (size_t)devices);
    for (size_t i = 0; i < streams.size(); i++)
        for (size_t j = i + 1; j < streams.size(); j++) CHECK(streams[i].tri_xyz != streams[j].tri_xyz && streams[i].box != streams[j].box);
    // query == NULL and the all-defaults query hand the launch what swr_cast_rays hands it: one band's stream and that band's boxes.
    // (Which band cannot be seen from here: the bands stream on threads of their own, so the records carry no band order, and the
    // launch note carries no band.  That it is one band's pair, and the same pair in every later call, can.)
    {
        const std::vector<swr_ray> rays = make_rays(65, 1.0f);
        std::vector<swr_ray_hit> hits(65, UNTOUCHED);
        (void)take_ray_notes();
        CHECK(swr_cast_rays(c, rays.data(), 65, 0, hits.data()) == SWR_OK);
        const std::vector<RayNote> notes = take_ray_notes();
        CHECK(notes.size() == 1 && notes[0].ran);
        const swr::RaysArgs cast = notes.empty() ? swr::RaysArgs{} : notes[0].a;
        CHECK(cast.flags == 0 && cast.p_begin == 0 && cast.p_end == ntri && cast.ntri == ntri && cast.groups == (ntri + 63) / 64);
        int owners = 0;
        for (const Record& r : streams) owners += r.tri_xyz == cast.tri_xyz && r.box == cast.box64;
        CHECK(owners == 1);
        swr::RaysArgs a{};
        const swr_ray_query defaults{0, 0, 0, -1}, spelt{0, 0, 0, ntri};
        CHECK(query_ok(c, nullptr, rays, ntri, a, "query == NULL") && same_args(a, cast));
        CHECK(query_ok(c, &defaults, rays, ntri, a, "the all-defaults query") && same_args(a, cast));
        CHECK(query_ok(c, &spelt, rays, ntri, a, "the whole range, spelt out") && same_args(a, cast));
    }
    // flags and the range arrive as given, -1 resolved to the scene's triangle count; ntri and groups stay the whole stream's
    {
        const uint32_t all = SWR_RAYS_ANY_HIT | SWR_RAYS_CULL_BACK | SWR_RAYS_CULL_FRONT | SWR_RAYS_FRONT_CW;
        const swr_ray_query q1{SWR_RAYS_ANY_HIT, 0, 0, -1}, q2{SWR_RAYS_CULL_BACK, 0, 70, 5}, q3{SWR_RAYS_FRONT_CW | SWR_RAYS_CULL_FRONT, 0, 64, -1},
                            q4{all, 0, ntri - 1, 1}, q5{0, 0, 64, 64};
        expect_query(c, &q1, ntri, SWR_RAYS_ANY_HIT, 0, ntri, "any-hit");
        expect_query(c, &q2, ntri, SWR_RAYS_CULL_BACK, 70, 75, "a cull and a range inside a group");
        expect_query(c, &q3, ntri, SWR_RAYS_FRONT_CW | SWR_RAYS_CULL_FRONT, 64, ntri, "from a group's first slot to the end");
        expect_query(c, &q4, ntri, all, ntri - 1, ntri, "every flag, the last triangle");
        expect_query(c, &q5, ntri, 0, 64, 128, "one group");
        // an empty range is legal, at either end and in the middle: the launch sees begin == end
        const swr_ray_query e1{0, 0, 0, 0}, e2{SWR_RAYS_ANY_HIT, 0, ntri, 0}, e3{0, 0, ntri, -1}, e4{SWR_RAYS_CULL_BACK, 0, 100, 0};
        expect_query(c, &e1, ntri, 0, 0, 0, "an empty range at the start");
        expect_query(c, &e2, ntri, SWR_RAYS_ANY_HIT, ntri, ntri, "an empty range at the end");
        expect_query(c, &e3, ntri, 0, ntri, ntri, "from the end to the end");
        expect_query(c, &e4, ntri, SWR_RAYS_CULL_BACK, 100, 100, "an empty range in the middle");
    }
    // regrowth: SWR_RAYS_MAX rays, then one: the large call's buffers are kept
    {
        swr::RaysArgs big{}, one{};
        const swr_ray_query q{SWR_RAYS_ANY_HIT, 0, 0, -1};
        CHECK(query_ok(c, &q, make_rays((size_t)SWR_RAYS_MAX, 3.0f), ntri, big, "SWR_RAYS_MAX rays"));
        CHECK(query_ok(c, &q, make_rays(1, 4.0f), ntri, one, "1 ray after the largest call"));
        CHECK(one.rays == big.rays && one.keys == big.keys && one.hits == big.hits && one.tri_xyz == big.tri_xyz);
    }
    // behind an un-waited frame: the frame completes as it was posted; behind a draw list that cuts the stream: the resident stream
    CHECK(swr_target_set(c, 64, 192, 0, 192) == SWR_OK);
    {
        swr::RaysArgs before{}, a{};
        const swr_ray_query q{SWR_RAYS_CULL_FRONT, 0, 10, 100};
        CHECK(query_ok(c, &q, make_rays(3, 5.0f), ntri, before, "with a target"));
        tagm(m, 3.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        CHECK(query_ok(c, &q, make_rays(64, 5.0f), ntri, a, "behind an un-waited frame"));
        CHECK(a.tri_xyz == before.tri_xyz && a.box64 == before.box64 && a.p_begin == 10 && a.p_end == 110);
        CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 3.0f));
        swr_draw_item items[2] = {{0, 3 * (ntri / 2), {}}, {3 * (ntri / 2), 3 * (ntri - ntri / 2), {}}};
        tagm(items[0].transform, 6.0f); tagm(items[1].transform, 6.0f);
        CHECK(swr_draw_list(c, items, 2, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        const swr_ray_query item1{SWR_RAYS_ANY_HIT, 0, items[1].first_index / 3, items[1].index_count / 3};
        CHECK(query_ok(c, &item1, make_rays(3, 8.0f), ntri, a, "behind a draw list, the second item's range"));
        CHECK(a.tri_xyz == before.tri_xyz && a.ntri == ntri && a.p_begin == ntri / 2 && a.p_end == ntri && a.flags == SWR_RAYS_ANY_HIT);
        CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 6.0f));
        (void)take_records();       // (the cut restreams the scene)
    }
    // a scene without triangles: legal, only the empty range fits it
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), 2) == SWR_OK);
    {
        const swr_ray_query any{SWR_RAYS_ANY_HIT, 0, 0, -1}, beyond{0, 0, 0, 1};
        expect_query(c, &any, 0, SWR_RAYS_ANY_HIT, 0, 0, "a scene without triangles");
        std::vector<swr_ray> rays = make_rays(2, 0.0f);
        swr_ray_hit h[2] = {UNTOUCHED, UNTOUCHED};
        CHECK(swr_query_rays(c, &beyond, rays.data(), 2, h) == SWR_ERR_BAD_ARG && h[0].primitive == 0xA5A5A5A5u);
    }
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
    swr_ray_hit hits[3] = {UNTOUCHED, UNTOUCHED, UNTOUCHED};
    const swr_ray_query q{SWR_RAYS_ANY_HIT, 0, 0, -1}, bad{16u, 0, 0, -1};
    CHECK(swr_query_rays(c, &q, rays.data(), 3, hits) == SWR_ERR_HIP);
    CHECK(swr_query_rays(c, nullptr, rays.data(), 3, hits) == SWR_ERR_HIP);
    // (a group checks the call's arguments before its bands report, as every entry point that waits: fan in swr_api.hip)
    CHECK(swr_query_rays(c, &bad, rays.data(), 3, hits) == (devices == 1 ? SWR_ERR_HIP : SWR_ERR_BAD_ARG));
    CHECK(swr_query_rays(c, nullptr, nullptr, 0, nullptr) == SWR_ERR_HIP);
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
    return report("ray queries host test");
}
