// The host side of the morph targets (software-renderer_amd/csrc/swr_api.hip: single_scene_morph, single_morph_set, the upload of the
// deltas, enqueue_pose as the chain morph, skin, stream, and its callers in restream, single_scene_attributes, single_scene_skin and
// single_pose_set, the group fan-out) on the fake HIP runtime of tests/host/hip_stub, under the address and undefined-behaviour
// sanitizers.  The stand-ins of swr::launch_morph_vertices, swr::launch_skin_vertices and swr::launch_skin_stream (stub_launch.cpp) are
// plain CPU loops over the header's arithmetic run as "kernels" of the fake stream.  The fake stream build writes no stream, so the
// loops take slot s for primitive s; they read and write every element of every array they are given, at the sizes swr_internal.h
// states: an array the host layer sized too small, or the wrong array, is an out-of-bounds access the address sanitizer reports or a
// stream that differs from the model's.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/morph_host_test.cpp -lpthread
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host_test.h"

// target `poison` (if any) is NaN and infinities
static Targets make_targets(int count, int nv, bool nrm, float salt, int poison = -1) {
    Targets t;
    t.count = count; t.nrm = nrm;
    t.dp.resize((size_t)count * nv * 3);
    if (nrm) t.dn.resize(t.dp.size());
    for (int k = 0; k < count; k++)
        for (int i = 0; i < nv; i++)
            for (int c = 0; c < 3; c++) {
                const size_t at = ((size_t)k * nv + i) * 3 + c;
                const bool bad = k == poison;
                t.dp[at] = bad ? (c == 0 ? NAN : c == 1 ? INFINITY : -INFINITY) : salt + 0.001f * (float)((k * 31 + i * 7 + c * 3) % 113) - 0.05f;
                if (nrm) t.dn[at] = bad ? NAN : 0.01f * (float)((k * 13 + i * 5 + c) % 37) - salt;
            }
    return t;
}
static swr_morph_targets desc(const Targets& t, int64_t nv) {
    return swr_morph_targets{t.dp.data(), t.nrm ? t.dn.data() : nullptr, nv, t.count, 0};
}

static void scenario(uint32_t devices, int nv, int ntri) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int B = (int)devices;
    const int W = 64, H = 192;
    const Scene s = make_scene(nv, ntri, 5);
    const std::vector<float> A = make_pose(6, 0.25f), Bp = make_pose(9, -0.5f);
    const Targets T = make_targets(5, nv, true, 0.02f, 3);          // target 3 is not finite: only ever weight 0
    const Targets T2 = make_targets(3, nv, false, -0.01f);
    const float wA[5] = {0.75f, 1.0f, 0.0f, 0.0f, 0.0f}, wB[5] = {-0.5f, 0.25f, 0.5f, -0.0f, 0.375f};
    const float wZ[5] = {0.0f, -0.0f, 0.0f, -0.0f, 0.0f}, w3[3] = {0.0f, 2.0f, -1.0f};
    std::vector<float> d((size_t)W * H);
    float m[16];
    // before a scene, before targets
    { const swr_morph_targets t = desc(T, nv); CHECK(swr_scene_morph(c, &t) == SWR_ERR_NO_SCENE); }
    CHECK(swr_morph_set(c, wA, 5) == SWR_ERR_NO_SCENE);
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    CHECK(swr_morph_set(c, wA, 5) == SWR_ERR_BAD_ARG);
    CHECK(std::string(swr_last_error(c)).find("swr_scene_morph") != std::string::npos);
    CHECK(swr_morph_set(c, nullptr, 0) == SWR_ERR_BAD_ARG);
    CHECK(swr_scene_morph(c, nullptr) == SWR_OK);                    // nothing to remove
    // every refusal of swr_scene_morph
    auto refusals = [&] {
        swr_morph_targets t = desc(T, nv);
        CHECK(swr_scene_morph(nullptr, &t) == SWR_ERR_BAD_ARG);
        t = desc(T, nv); t.vertex_count = nv - 1; CHECK(swr_scene_morph(c, &t) == SWR_ERR_BAD_ARG);
        t = desc(T, nv); t.vertex_count = nv + 1; CHECK(swr_scene_morph(c, &t) == SWR_ERR_BAD_ARG);
        t = desc(T, nv); t.position_deltas = nullptr; CHECK(swr_scene_morph(c, &t) == SWR_ERR_BAD_ARG);
        t = desc(T, nv); t.target_count = 0; CHECK(swr_scene_morph(c, &t) == SWR_ERR_BAD_ARG);
        t = desc(T, nv); t.target_count = -1; CHECK(swr_scene_morph(c, &t) == SWR_ERR_BAD_ARG);
        t = desc(T, nv); t.reserved = 1; CHECK(swr_scene_morph(c, &t) == SWR_ERR_BAD_ARG);
        t = desc(T, nv); t.target_count = SWR_MORPH_MAX_TARGETS + 1; CHECK(swr_scene_morph(c, &t) == SWR_ERR_UNSUPPORTED);
    };
    refusals();
    CHECK(swr_morph_set(c, wA, 5) == SWR_ERR_BAD_ARG);              // still no targets
    expect_no_launch("refused targets");
    // the targets are copied: the caller's arrays are scribbled over and freed on return
    {
        Targets* tmp = new Targets(T);
        const swr_morph_targets t = desc(*tmp, nv);
        CHECK(swr_scene_morph(c, &t) == SWR_OK);
        std::fill(tmp->dp.begin(), tmp->dp.end(), 1.0e30f); std::fill(tmp->dn.begin(), tmp->dn.end(), -1.0e30f);
        delete tmp;
    }
    expect_no_launch("new targets on an unmorphed scene change nothing");
    CHECK(swr_morph_set(c, wA, 5) == SWR_OK);
    expect_stream(s, &T, wA, nullptr, false, B, "weights A");
    // every refusal of swr_morph_set, and of swr_scene_morph again: stream, targets and weights stay
    CHECK(swr_morph_set(nullptr, wA, 5) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_set(c, wB, 4) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_set(c, wB, 6) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_set(c, wB, 0) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_set(c, wB, -1) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_set(c, nullptr, 5) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_set(c, nullptr, -1) == SWR_ERR_BAD_ARG);
    refusals();
    expect_no_launch("refused weights");
    // weights behind an un-waited frame: the frame completes as it was posted
    tagm(m, 3.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_morph_set(c, wB, 5) == SWR_OK);
    expect_stream(s, &T, wB, nullptr, false, B, "weights B behind a frame");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 3.0f));
    // ... and an overflowed one is repaired by the call, before the stream changes
    swr::g_fake_fill.store(5000);
    tagm(m, 4.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_morph_set(c, wA, 5) == SWR_OK);
    swr::g_fake_fill.store(7);
    expect_stream(s, &T, wA, nullptr, false, B, "weights A behind an overflowed frame (the refusals left A in place before)");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 4.0f));
    // a pose under an active morph, then a morph under an active pose: morph first, then skin
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    expect_no_launch("a skin without a pose");
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_OK);
    expect_stream(s, &T, wA, A.data(), false, B, "pose A under weights A");
    CHECK(swr_morph_set(c, wB, 5) == SWR_OK);
    expect_stream(s, &T, wB, A.data(), false, B, "weights B under pose A");
    // attributes arrive: the normal deltas given earlier take effect, and the pose is applied to the morphed normals
    const int nrm_before = g_morph_nrm_launches.load();
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    expect_stream(s, &T, wB, A.data(), true, B, "attributes under weights B and pose A");
    CHECK(g_morph_nrm_launches.load() == nrm_before + B);
    // a draw list over two ranges cuts the stream (restream): morphed and posed again
    if (ntri >= 4) {
        swr_draw_item items[2] = {{0, 3 * (int64_t)(ntri / 2), {}}, {3 * (int64_t)(ntri / 2), 3 * (int64_t)(ntri - ntri / 2), {}}};
        tagm(items[0].transform, 5.0f); tagm(items[1].transform, 6.0f);
        CHECK(swr_draw_list(c, items, 2, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        CHECK(swr_sync(c) == SWR_OK);
        expect_stream(s, &T, wB, A.data(), true, B, "weights B and pose A after the stream was cut");
    }
    // all-zero weights, of either sign, and NULL restore the posed stream exactly; a second time there is nothing to do
    CHECK(swr_morph_set(c, wZ, 5) == SWR_OK);
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "zero weights: pose A alone");
    CHECK(swr_morph_set(c, nullptr, 0) == SWR_OK);
    CHECK(swr_morph_set(c, wZ, 5) == SWR_OK);
    expect_no_launch("zero weights twice");
    CHECK(swr_morph_set(c, wA, 5) == SWR_OK);
    expect_stream(s, &T, wA, A.data(), true, B, "weights A again");
    CHECK(swr_morph_set(c, nullptr, 0) == SWR_OK);
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "NULL weights: pose A alone");
    // a new pose and the bind pose keep the weights
    CHECK(swr_morph_set(c, wB, 5) == SWR_OK);
    expect_stream(s, &T, wB, A.data(), true, B, "weights B");
    CHECK(swr_pose_set(c, Bp.data(), 9) == SWR_OK);
    expect_stream(s, &T, wB, Bp.data(), true, B, "pose B keeps weights B");
    CHECK(swr_pose_set(c, nullptr, 0) == SWR_OK);
    expect_stream(s, &T, wB, nullptr, true, B, "the bind pose keeps weights B");
    CHECK(swr_morph_set(c, wZ, 5) == SWR_OK);
    expect_stream(s, nullptr, nullptr, nullptr, true, B, "zero weights: the uploaded stream");
    // new targets zero the weights and keep the pose; these have no normal deltas: the normals stay as uploaded (and are posed)
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_OK);
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "pose A");
    CHECK(swr_morph_set(c, wA, 5) == SWR_OK);
    expect_stream(s, &T, wA, A.data(), true, B, "weights A under pose A");
    { const swr_morph_targets t = desc(T2, nv); CHECK(swr_scene_morph(c, &t) == SWR_OK); }
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "new targets: every weight 0, pose A kept");
    CHECK(swr_morph_set(c, wA, 5) == SWR_ERR_BAD_ARG);              // three targets now
    CHECK(swr_morph_set(c, w3, 3) == SWR_OK);
    expect_stream(s, &T2, w3, A.data(), true, B, "three targets without normal deltas");
    // a new skin keeps the weights and drops the pose
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    expect_stream(s, &T2, w3, nullptr, true, B, "a new skin: the morph alone");
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_OK);
    expect_stream(s, &T2, w3, A.data(), true, B, "pose A again");
    // removal of the targets
    CHECK(swr_scene_morph(c, nullptr) == SWR_OK);
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "the targets removed: pose A alone");
    CHECK(swr_morph_set(c, w3, 3) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_set(c, nullptr, 0) == SWR_ERR_BAD_ARG);
    CHECK(swr_scene_morph(c, nullptr) == SWR_OK);
    expect_no_launch("removed twice");
    // targets from page-locked memory: one copy straight from the caller's array
    {
        float* pinned = nullptr;
        CHECK(hipHostMalloc((void**)&pinned, T.dp.size() * 4, 0) == hipSuccess);
        memcpy(pinned, T.dp.data(), T.dp.size() * 4);
        swr_morph_targets t = desc(T, nv);
        t.position_deltas = pinned; t.normal_deltas = nullptr;
        CHECK(swr_scene_morph(c, &t) == SWR_OK);
        memset(pinned, 0xFF, T.dp.size() * 4);
        CHECK(hipHostFree(pinned) == hipSuccess);
        Targets Tp = T; Tp.nrm = false;
        CHECK(swr_morph_set(c, wB, 5) == SWR_OK);
        expect_stream(s, &Tp, wB, A.data(), true, B, "page-locked deltas, no normal deltas");
    }
    // an upload drops everything
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_morph_set(c, wA, 5) == SWR_ERR_BAD_ARG);
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_ERR_BAD_ARG);
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    expect_no_launch("an upload drops targets and weights");
    // attributes first, then targets with normal deltas
    { const swr_morph_targets t = desc(T, nv); CHECK(swr_scene_morph(c, &t) == SWR_OK); }
    CHECK(swr_morph_set(c, wB, 5) == SWR_OK);
    expect_stream(s, &T, wB, nullptr, true, B, "attributes before the targets");
    swr_context_destroy(c);
}

// 256 targets over enough vertices that the deltas take several staging chunks: all active, then only the last
static void many_targets(uint32_t devices, int nv) {
    swr_config cfg{0, devices, 20000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const Scene s = make_scene(nv, 200, 2);
    const Targets T = make_targets(SWR_MORPH_MAX_TARGETS, nv, true, 0.0f);
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    { const swr_morph_targets t = desc(T, nv); CHECK(swr_scene_morph(c, &t) == SWR_OK); }
    std::vector<float> w(SWR_MORPH_MAX_TARGETS);
    for (int k = 0; k < SWR_MORPH_MAX_TARGETS; k++) w[k] = 0.01f * (float)(k % 17 + 1) * (k % 2 ? -1.0f : 1.0f);
    CHECK(swr_morph_set(c, w.data(), SWR_MORPH_MAX_TARGETS) == SWR_OK);
    expect_stream(s, &T, w.data(), nullptr, true, (int)devices, "256 targets, all active");
    std::fill(w.begin(), w.end(), 0.0f);
    w.back() = 1.5f;
    CHECK(swr_morph_set(c, w.data(), SWR_MORPH_MAX_TARGETS) == SWR_OK);
    expect_stream(s, &T, w.data(), nullptr, true, (int)devices, "256 targets, the last one active");
    swr_context_destroy(c);
}

// a failed context returns its sticky error
static void failed_context(uint32_t devices) {
    swr_config cfg{0, devices, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const Scene s = make_scene(300, 100, 2);
    const Targets T = make_targets(2, 300, false, 0.0f);
    const float w[2] = {1.0f, 0.5f};
    CHECK(swr_scene_upload(c, s.v.data(), 300, s.idx.data(), 300) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    const swr_morph_targets t = desc(T, 300);
    CHECK(swr_scene_morph(c, &t) == SWR_OK);
    float m[16];
    tagm(m, 1.0f);
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, SWR_FLAG_DEPTH_TEST);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    (void)take_records();
    CHECK(swr_morph_set(c, w, 2) == SWR_ERR_HIP);
    CHECK(swr_scene_morph(c, &t) == SWR_ERR_HIP);
    CHECK(swr_scene_morph(c, nullptr) == SWR_ERR_HIP);
    expect_no_launch("a failed context");
    swr_context_destroy(c);
}
int main() {
    fake_kernel_delay_us(0);
    scenario(1, 300, 200);
    scenario(3, 300, 200);
    scenario(1, 3, 1);              // one triangle: one ragged group
    scenario(3, 130, 129);          // 64 * 2 + 1 slots
    many_targets(1, 8200);          // 256 x 8200 x 12 bytes: three staging chunks per plane
    many_targets(3, 700);
    failed_context(1);
    failed_context(2);
    CHECK(g_morph_launches.load() > 0 && g_morph_nrm_launches.load() > 0 && g_vertex_launches.load() > 0);
    CHECK(g_stream_launches.load() > g_morph_launches.load());
    return report("morph host test");
}
