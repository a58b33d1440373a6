// The host side of the skinned meshes (software-renderer_amd/csrc/swr_api.hip: single_scene_skin, single_pose_set, enqueue_pose and
// its callers in restream and single_scene_attributes, the group fan-out) on the fake HIP runtime of tests/host/hip_stub, under the
// address and undefined-behaviour sanitizers.  The stand-in set of stub_launch.cpp has no skin launch: this program defines
// swr::launch_skin_vertices and swr::launch_skin_stream itself, as plain CPU loops over the header's arithmetic run as "kernels" of the
// fake stream.  The fake stream build writes no stream, so the loops take slot s for primitive s; they read and write every element of
// every array they are given, at the sizes swr_internal.h states: an array the host layer sized too small, or the wrong array, is an
// out-of-bounds access the address sanitizer reports or a stream that differs from the model's.  What is checked is the host side:
// which arrays it hands over, when, and what it refuses.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/skin_host_test.cpp -lpthread
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/swr.h"
#include <hip/hip_runtime.h>
#include "../../software-renderer_amd/csrc/swr_internal.h"

namespace swr { extern std::atomic<uint32_t> g_fake_fill; }
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// the header's arithmetic for one vector: translate = the c3 term (positions), else not (normals)
static void blend(const float* v, const swr_skin_vertex& sk, const float* joints, bool translate, float* out) {
    float acc[3] = {0, 0, 0};
    for (int k = 0; k < 4; k++) {
        const float* m = joints + 16 * (size_t)sk.joint[k];
        for (int c = 0; c < 3; c++) {
            float r = m[c] * v[0];
            r = r + m[4 + c] * v[1];
            r = r + m[8 + c] * v[2];
            if (translate) r = r + m[12 + c] * 1.0f;
            acc[c] = k == 0 ? sk.weight[k] * r : acc[c] + sk.weight[k] * r;
        }
    }
    memcpy(out, acc, sizeof acc);
}

// what the last stream launch of every band wrote, and how often each launch ran
struct Record { const float4* tri_xyz; const float4* tri_nrm; const float4* box; int64_t ntri; bool nrm; };
static std::mutex g_m;
static std::vector<Record> g_records;
static std::atomic<int> g_vertex_launches{0}, g_stream_launches{0};

#ifndef SKIN_HOST_NO_LAUNCH
namespace swr {
void launch_skin_vertices(const swr_vertex* vertices, const swr_vertex_attr* attrs, const swr_skin_vertex* skin, int64_t nv,
                          const float* joints, int32_t joint_count, swr_vertex* posed, float4* posed_nrm, hipStream_t s) {
    g_vertex_launches++;
    fake_enqueue(s, [=] {
        for (int64_t i = 0; i < nv; i++) {
            for (int k = 0; k < 4; k++) if ((int64_t)skin[i].joint[k] >= joint_count) { std::printf("FAIL joint %u of %d\n", skin[i].joint[k], joint_count); fails++; return; }
            posed[i] = vertices[i];
            blend(vertices[i].xyz, skin[i], joints, true, posed[i].xyz);
            if (attrs) { float n[3]; blend(attrs[i].normal, skin[i], joints, false, n); posed_nrm[i] = make_float4(n[0], n[1], n[2], 0.0f); }
        }
    }, nullptr, "k_skin_vertices", (size_t)nv);
}
void launch_skin_stream(const float4* pos, int pos_stride, const float4* nrm, int nrm_stride, int64_t nv, const int64_t* indices,
                        int64_t ntri, int reordered, float4* tri_xyz, float4* tri_nrm, float4* box64, hipStream_t s) {
    g_stream_launches++;
    fake_enqueue(s, [=] {
        (void)reordered;                    // (the fake upload builds no stream: slot s holds primitive s)
        for (int64_t g = 0; g < (ntri + 63) / 64; g++) {
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int64_t t = g * 64; t < std::min(ntri, g * 64 + 64); t++)
                for (int k = 0; k < 3; k++) {
                    const int64_t ix = indices[3 * t + k];
                    if (ix < 0 || ix >= nv) { std::printf("FAIL index\n"); fails++; return; }
                    const float4 x = pos[(size_t)pos_stride * ix];
                    float4& o = tri_xyz[3 * t + k];
                    o.x = x.x; o.y = x.y; o.z = x.z;
                    if (nrm) { const float4 n = nrm[(size_t)nrm_stride * ix]; float4& q = tri_nrm[3 * t + k]; q.x = n.x; q.y = n.y; q.z = n.z; }
                    const float c[3] = {x.x, x.y, x.z};
                    for (int j = 0; j < 3; j++) { lo[j] = std::min(lo[j], c[j]); hi[j] = std::max(hi[j], c[j]); }
                }
            box64[2 * g] = make_float4(lo[0], lo[1], lo[2], 0);
            box64[2 * g + 1] = make_float4(hi[0], hi[1], hi[2], 0);
        }
        std::lock_guard<std::mutex> lk(g_m);
        g_records.push_back(Record{tri_xyz, tri_nrm, box64, ntri, nrm != nullptr});
    }, nullptr, "k_skin_stream", (size_t)ntri);
}
}  // namespace swr
#endif

struct Scene {
    std::vector<swr_vertex> v;
    std::vector<swr_vertex_attr> a;
    std::vector<swr_skin_vertex> sk;
    std::vector<int64_t> idx;
};

static Scene make_scene(int nv, int ntri, uint32_t top_joint) {
    Scene s;
    s.v.resize(nv); s.a.resize(nv); s.sk.resize(nv); s.idx.resize(3 * (size_t)ntri);
    for (int i = 0; i < nv; i++) {
        s.v[i] = swr_vertex{{0.01f * i - 0.5f, 0.3f - 0.002f * i, 0.1f + 0.001f * i, 0}, {0.1f, 0.2f, 0.3f, 0}};
        s.a[i] = swr_vertex_attr{{0.5f, 0.01f * i, -0.25f, 0}, {0.1f * i, 0.2f, 0, 0}};
        s.sk[i] = swr_skin_vertex{{(uint32_t)(i % 3), (uint32_t)((i + 1) % 3), top_joint, 0}, {0.5f, 0.25f, 0.125f, 0.125f}};
    }
    for (size_t k = 0; k < s.idx.size(); k++) s.idx[k] = (int64_t)((k * 7 + k / 3) % (size_t)nv);
    return s;
}

static std::vector<float> make_pose(int joints, float salt) {
    std::vector<float> p(16 * (size_t)joints, 0.0f);
    for (int j = 0; j < joints; j++) {
        float* m = &p[16 * (size_t)j];
        m[0] = 1.0f + 0.1f * j + salt; m[5] = 0.9f - 0.05f * j; m[10] = 1.0f; m[15] = 1.0f;
        m[1] = 0.1f * salt; m[4] = -0.2f; m[12] = 0.01f * j; m[13] = salt; m[14] = -0.02f * j;
        m[3] = 77.0f; m[7] = -5.0f;         // the fourth row is ignored
    }
    return p;
}

// the stream every band must hold: the positions (and normals) of the scene in `pose` (NULL: the bind pose); bands = the launches
// the call must have made
static void expect_stream(const Scene& s, const float* pose, bool nrm, int bands, const char* what) {
    std::lock_guard<std::mutex> lk(g_m);
    if ((int)g_records.size() != bands) { std::printf("FAIL %s: %zu stream launches, not %d\n", what, g_records.size(), bands); fails++; g_records.clear(); return; }
    const int64_t ntri = (int64_t)s.idx.size() / 3;
    for (const Record& r : g_records) {
        bool ok = r.ntri == ntri && r.nrm == nrm;
        for (int64_t t = 0; ok && t < ntri; t++)
            for (int k = 0; k < 3; k++) {
                const int64_t ix = s.idx[3 * t + k];
                float p[3], n[3];
                if (pose) { blend(s.v[ix].xyz, s.sk[ix], pose, true, p); blend(s.a[ix].normal, s.sk[ix], pose, false, n); }
                else { memcpy(p, s.v[ix].xyz, 12); memcpy(n, s.a[ix].normal, 12); }
                ok = ok && memcmp(&r.tri_xyz[3 * t + k], p, 12) == 0 && (!nrm || memcmp(&r.tri_nrm[3 * t + k], n, 12) == 0);
            }
        if (!ok) { std::printf("FAIL %s: the stream is not the model's\n", what); fails++; }
    }
    g_records.clear();
}
static void expect_no_launch(const char* what) {
    std::lock_guard<std::mutex> lk(g_m);
    if (!g_records.empty()) { std::printf("FAIL %s: %zu unexpected stream launches\n", what, g_records.size()); fails++; g_records.clear(); }
}

static void tagm(float* m, float tag) { for (int k = 0; k < 16; k++) m[k] = (k % 5 == 0) ? 1.0f : 0.0f; m[0] = tag; }
static bool all_eq(const std::vector<float>& d, float v) { for (float x : d) if (x != v) return false; return true; }

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
    { std::lock_guard<std::mutex> lk(g_m); g_records.clear(); }
    CHECK(swr_pose_set(c, A.data(), 3) == SWR_ERR_HIP);
    CHECK(swr_scene_skin(c, s.sk.data(), 300) == SWR_ERR_HIP);
    expect_no_launch("a failed context");
    swr_context_destroy(c);
}

// -DSKIN_HOST_NO_LAUNCH: the program links without the skin launches, as the older stand-alone programs do, and a pose fails loudly
static void without_the_kernel() {
    swr_config cfg{0, 1, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const Scene s = make_scene(300, 100, 2);
    const std::vector<float> A = make_pose(3, 0.0f);
    CHECK(swr_scene_upload(c, s.v.data(), 300, s.idx.data(), 300) == SWR_OK);
    CHECK(swr_scene_skin(c, s.sk.data(), 300) == SWR_OK);
    CHECK(swr_pose_set(c, A.data(), 3) == SWR_ERR_HIP);
    CHECK(std::string(swr_last_error(c)).find("k_skin_vertices") != std::string::npos);
    CHECK(swr_sync(c) == SWR_OK);       // (not a failed context: only this call cannot be answered)
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
#ifdef SKIN_HOST_NO_LAUNCH
    without_the_kernel();
    std::printf(fails ? "skin host test: %d failures\n" : "skin host test: ok\n", fails);
    return fails ? 1 : 0;
#endif
    scenario(1, 300, 200);
    scenario(3, 300, 200);
    scenario(1, 3, 1);              // one triangle: one ragged group
    scenario(3, 130, 129);          // 64 * 2 + 1 slots
    failed_context(1);
    failed_context(2);
    CHECK(g_vertex_launches.load() > 0 && g_stream_launches.load() > g_vertex_launches.load());
    std::printf(fails ? "skin host test: %d failures\n" : "skin host test: ok\n", fails);
    return fails ? 1 : 0;
}
