// The host side of the skinned meshes (software-renderer_amd/csrc/swr_api.hip: single_scene_skin, single_pose_set, enqueue_pose and
// its callers in restream and single_scene_attributes, the group fan-out) on the fake HIP runtime of tests/host/hip_stub, under the
// address and undefined-behaviour sanitizers.  The stand-ins of swr::launch_skin_vertices and swr::launch_skin_stream (stub_launch.cpp)
// are plain CPU loops over the header's arithmetic run as "kernels" of the fake stream.  The fake stream build writes no stream, so the
// loops take slot s for primitive s; they read and write every element of every array they are given, at the sizes swr_internal.h
// states: an array the host layer sized too small, or the wrong array, is an out-of-bounds access the address sanitizer reports or a
// stream that differs from the model's.  What is checked is the host side: which arrays it hands over, when, and what it refuses.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/skin_host_test.cpp -lpthread
#include <string>
#include <vector>

#include "host_test.h"

// the stream every band must hold: the positions (and normals) of the scene in `pose` (NULL: the bind pose); bands = the launches
// the call must have made
static void expect_stream(const Scene& s, const float* pose, bool nrm, int bands, const char* what) {
    expect_stream(s, nullptr, nullptr, pose, nrm, bands, what);
}

static void scenario(uint32_t devices, int nv, int ntri) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int B = (int)devices;
    const int W = 64, H = 192;
    const Scene s = make_scene(nv, ntri, 5);
    const std::vector<float> A = make_pose(6, 0.25f), Bp = make_pose(9, -0.5f);
    std::vector<float> d((size_t)W * H);
    float m[16];
    // before a scene, before a skin
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_ERR_NO_SCENE);
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_ERR_NO_SCENE);
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_ERR_BAD_ARG);
    CHECK(std::string(swr_last_error(c)).find("swr_scene_skin") != std::string::npos);
    CHECK(swr_pose_set(c, nullptr, 0) == SWR_ERR_BAD_ARG);
    // every refusal of swr_scene_skin
    CHECK(swr_scene_skin(nullptr, s.sk.data(), nv) == SWR_ERR_BAD_ARG);
    CHECK(swr_scene_skin(c, s.sk.data(), nv - 1) == SWR_ERR_BAD_ARG);
    CHECK(swr_scene_skin(c, s.sk.data(), nv + 1) == SWR_ERR_BAD_ARG);
    CHECK(swr_scene_skin(c, nullptr, nv) == SWR_ERR_BAD_ARG);
    { Scene bad = s; bad.sk[nv - 1].joint[3] = SWR_SKIN_MAX_JOINTS; CHECK(swr_scene_skin(c, bad.sk.data(), nv) == SWR_ERR_BAD_ARG);
      bad.sk[nv - 1].joint[3] = SWR_SKIN_MAX_JOINTS - 1; CHECK(swr_scene_skin(c, bad.sk.data(), nv) == SWR_OK);      // the limit itself
      std::vector<float> big = make_pose(SWR_SKIN_MAX_JOINTS, 0.0f);
      CHECK(swr_pose_set(c, big.data(), SWR_SKIN_MAX_JOINTS - 1) == SWR_ERR_BAD_ARG);
      CHECK(swr_pose_set(c, big.data(), SWR_SKIN_MAX_JOINTS + 1) == SWR_ERR_UNSUPPORTED);
      expect_no_launch("refused poses");
      CHECK(swr_pose_set(c, big.data(), SWR_SKIN_MAX_JOINTS) == SWR_OK);       // the largest table, read to its last float
      expect_stream(bad, big.data(), false, B, "1024 joints"); }
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);                        // a new skin: back to the bind pose
    expect_stream(s, nullptr, false, B, "a new skin restores the bind pose");
    // every refusal of swr_pose_set; the pose stays
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_OK);
    expect_stream(s, A.data(), false, B, "pose A");
    CHECK(swr_pose_set(nullptr, A.data(), 6) == SWR_ERR_BAD_ARG);
    CHECK(swr_pose_set(c, A.data(), -1) == SWR_ERR_BAD_ARG);
    CHECK(swr_pose_set(c, A.data(), 5) == SWR_ERR_BAD_ARG);
    { const std::string e = swr_last_error(c); CHECK(e.find("5 joints") != std::string::npos && e.find("joint index 5") != std::string::npos); }
    CHECK(swr_pose_set(c, A.data(), 0) == SWR_ERR_BAD_ARG);
    CHECK(swr_pose_set(c, nullptr, 6) == SWR_ERR_BAD_ARG);
    CHECK(swr_pose_set(c, A.data(), SWR_SKIN_MAX_JOINTS + 1) == SWR_ERR_UNSUPPORTED);
    expect_no_launch("refused poses");
    // a pose behind an un-waited frame: the frame completes as it was posted
    tagm(m, 3.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_pose_set(c, Bp.data(), 9) == SWR_OK);
    expect_stream(s, Bp.data(), false, B, "pose B behind a frame");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 3.0f));
    // ... and an overflowed one is repaired by the call, before the stream changes
    swr::g_fake_fill.store(5000);
    tagm(m, 4.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_OK);
    swr::g_fake_fill.store(7);
    expect_stream(s, A.data(), false, B, "pose A behind an overflowed frame");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 4.0f));
    // attributes while a pose is in effect: the normals are posed too; then a pose with normals; the bind pose restores both
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    expect_stream(s, A.data(), true, B, "attributes under pose A");
    CHECK(swr_pose_set(c, Bp.data(), 9) == SWR_OK);
    expect_stream(s, Bp.data(), true, B, "pose B with normals");
    // a draw list over two ranges cuts the stream (restream): posed again.  (The fake stream is never Morton-sorted, so the cut is
    // only made when the context says its stream is sorted: scenes of two primitives or more, by default.)
    if (ntri >= 4) {
        swr_draw_item items[2] = {{0, 3 * (int64_t)(ntri / 2), {}}, {3 * (int64_t)(ntri / 2), 3 * (int64_t)(ntri - ntri / 2), {}}};
        tagm(items[0].transform, 5.0f); tagm(items[1].transform, 6.0f);
        CHECK(swr_draw_list(c, items, 2, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        CHECK(swr_sync(c) == SWR_OK);
        expect_stream(s, Bp.data(), true, B, "pose B after the stream was cut");
    }
    CHECK(swr_pose_set(c, nullptr, 0) == SWR_OK);
    expect_stream(s, nullptr, true, B, "the bind pose");
    CHECK(swr_pose_set(c, nullptr, 0) == SWR_OK);                               // already there: nothing to do
    expect_no_launch("the bind pose twice");
    // removing the skin under a pose restores the bind pose; a pose is then refused
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_OK);
    expect_stream(s, A.data(), true, B, "pose A again");
    CHECK(swr_scene_skin(c, nullptr, 0) == SWR_OK);
    expect_stream(s, nullptr, true, B, "the skin removed");
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_ERR_BAD_ARG);
    // an upload drops skin and pose
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_OK);
    expect_stream(s, A.data(), true, B, "pose A before the upload");
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_ERR_BAD_ARG);
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    expect_no_launch("an upload drops the pose");
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);                        // attributes first, then the skin
    CHECK(swr_pose_set(c, Bp.data(), 9) == SWR_OK);
    expect_stream(s, Bp.data(), true, B, "attributes before the skin");
    swr_context_destroy(c);
}

// a failed context returns its sticky error
static void failed_context(uint32_t devices) {
    swr_config cfg{0, devices, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const Scene s = make_scene(300, 100, 2);
    const std::vector<float> A = make_pose(3, 0.0f);
    CHECK(swr_scene_upload(c, s.v.data(), 300, s.idx.data(), 300) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    CHECK(swr_scene_skin(c, s.sk.data(), 300) == SWR_OK);
    float m[16];
    tagm(m, 1.0f);
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, SWR_FLAG_DEPTH_TEST);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    (void)take_records();
    CHECK(swr_pose_set(c, A.data(), 3) == SWR_ERR_HIP);
    CHECK(swr_scene_skin(c, s.sk.data(), 300) == SWR_ERR_HIP);
    expect_no_launch("a failed context");
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    scenario(1, 300, 200);
    scenario(3, 300, 200);
    scenario(1, 3, 1);              // one triangle: one ragged group
    scenario(3, 130, 129);          // 64 * 2 + 1 slots
    failed_context(1);
    failed_context(2);
    CHECK(g_vertex_launches.load() > 0 && g_stream_launches.load() > g_vertex_launches.load());
    return report("skin host test");
}
