// The host side of the dual-quaternion skinning (software-renderer_amd/csrc/swr_api.hip: single_pose_set as swr_pose_set_dq, the kind
// of the pose the context remembers, enqueue_pose and its callers in restream, single_scene_attributes, single_scene_morph,
// single_morph_set and single_scene_skin, the group fan-out) on the fake HIP runtime of tests/host/hip_stub, under the address and
// undefined-behaviour sanitizers.  The stand-in of swr::launch_skin_vertices_dq (hip_stub/stub_launch.cpp) is a plain CPU loop over the
// header's arithmetic (pose_dq of hip_stub/stub_launch.h, which the model below shares) run as a "kernel" of the fake stream.  It
// reads and writes every element of every array it is handed, at the sizes swr_internal.h states: a table sized for the other kind
// of pose (8 floats a joint against 16), or the wrong array, is an out-of-bounds access the address sanitizer reports or a stream that
// differs from the model's.  The other launches are the stand-ins of hip_stub, used as they are.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ \
//       software-renderer_amd/csrc/swr_api.hip tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp \
//       tests/host/skin_dq_host_test.cpp -lpthread
#include <atomic>
#include <cmath>
#include <string>
#include <vector>

#include "host_test.h"
#include "../../software-renderer_amd/csrc/swr_internal.h"

// ---- poses -----------------------------------------------------------------------------------------------------------------------
struct Pose { const float* data; bool dq; };
static const Pose BIND{nullptr, false};

// unit-ish dual quaternions: a turn about (1, 2, salt) by an angle that grows with j, a translation; every third joint negated
static std::vector<float> make_dq(int joints, float salt) {
    std::vector<float> p(8 * (size_t)joints);
    for (int j = 0; j < joints; j++) {
        const float ang = 0.3f * (float)(j % 19) + salt, ax[3] = {1.0f, 2.0f, salt};
        const float len = sqrtf(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), sn = sinf(0.5f * ang) / len, w = cosf(0.5f * ang);
        const float q[3] = {ax[0] * sn, ax[1] * sn, ax[2] * sn}, t[3] = {0.01f * (float)(j % 23), salt, -0.02f * (float)(j % 7)};
        float* o = &p[8 * (size_t)j];
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = w;
        o[4] = 0.5f * (t[0] * w + t[1] * q[2] - t[2] * q[1]);
        o[5] = 0.5f * (-t[0] * q[2] + t[1] * w + t[2] * q[0]);
        o[6] = 0.5f * (t[0] * q[1] - t[1] * q[0] + t[2] * w);
        o[7] = -0.5f * (t[0] * q[0] + t[1] * q[1] + t[2] * q[2]);
        if (j % 3 == 2) for (int c = 0; c < 8; c++) o[c] = -o[c];
    }
    return p;
}

static bool same3(const float* a, const float* b) {      // NaN compared as NaN
    for (int j = 0; j < 3; j++)
        if (memcmp(&a[j], &b[j], 4) != 0 && !(std::isnan(a[j]) && std::isnan(b[j]))) return false;
    return true;
}

// the stream every band must hold: the scene morphed by w over T (either NULL: unmorphed), then in `pose`; bands = the stream launches
// the call must have made
static void expect_dq_stream(const Scene& s, const Targets* T, const float* w, Pose pose, bool nrm, int bands, const char* what) {
    if (!pose.dq) { expect_stream(s, T, w, pose.data, nrm, bands, what); return; }
    const std::vector<Record> records = take_records();
    if ((int)records.size() != bands) { std::printf("FAIL %s: %zu stream launches, not %d\n", what, records.size(), bands); fails++; return; }
    const int64_t ntri = (int64_t)s.idx.size() / 3, nv = (int64_t)s.v.size();
    for (const Record& r : records) {
        bool ok = r.ntri == ntri && r.nrm == nrm;
        for (int64_t t = 0; ok && t < ntri; t++)
            for (int k = 0; k < 3; k++) {
                const int64_t ix = s.idx[3 * t + k];
                float p[3], n[3], q[3];
                memcpy(p, s.v[ix].xyz, 12); memcpy(n, s.a[ix].normal, 12);
                if (T && w) {
                    morph(p, T->dp.data(), w, T->count, nv, ix, p);
                    if (T->nrm) morph(n, T->dn.data(), w, T->count, nv, ix, n);
                }
                pose_dq(p, s.sk[ix], pose.data, true, q); memcpy(p, q, 12);
                pose_dq(n, s.sk[ix], pose.data, false, q); memcpy(n, q, 12);
                ok = ok && same3(&r.tri_xyz[3 * t + k].x, p) && (!nrm || same3(&r.tri_nrm[3 * t + k].x, n));
            }
        if (!ok) { std::printf("FAIL %s: the stream is not the model's (ntri %lld nrm %d)\n", what, (long long)r.ntri, (int)r.nrm); fails++; }
    }
}

// the model itself: the exact facts of the header's arithmetic
static void model_facts() {
    const swr_skin_vertex quarter{{0, 1, 0, 1}, {0.25f, 0.25f, 0.25f, 0.25f}}, solo{{0, 0, 0, 0}, {1.0f, 0.0f, 0.0f, 0.0f}};
    const float ident[16] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0};
    const float v[3] = {0.3f, -1.7f, 2.9f};
    float o[3];
    pose_dq(v, quarter, ident, true, o);
    CHECK(memcmp(o, v, 12) == 0);
    const float shift[8] = {0, 0, 0, 1, 0.25f, -0.5f, 1.0f, 0};
    pose_dq(v, solo, shift, true, o);
    CHECK(o[0] == v[0] + 0.5f && o[1] == v[1] - 1.0f && o[2] == v[2] + 2.0f);
    pose_dq(v, solo, shift, false, o);
    CHECK(memcmp(o, v, 12) == 0);
    const float half_z[8] = {0, 0, 1, 0, 0, 0, 0, 0};
    pose_dq(v, solo, half_z, true, o);
    CHECK(o[0] == -v[0] && o[1] == -v[1] && o[2] == v[2]);
    // identity and a half turn about x, half and half: a quarter turn, not the axis
    const float two[16] = {0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0};
    const swr_skin_vertex halves{{0, 1, 0, 0}, {0.5f, 0.5f, 0.0f, 0.0f}};
    const float y[3] = {0, 1, 0};
    pose_dq(y, halves, two, true, o);
    CHECK(std::fabs(o[0]) < 1e-6f && std::fabs(o[1]) < 1e-6f && std::fabs(o[2] - 1.0f) < 1e-6f);
    // a negated joint: no bit changes
    const std::vector<float> A = make_dq(4, 0.3f);
    std::vector<float> N = A;
    for (int c = 0; c < 8; c++) N[c] = -N[c];
    const swr_skin_vertex mix{{0, 1, 2, 3}, {0.4f, 0.3f, 0.2f, 0.1f}};
    float a[3], b[3];
    pose_dq(v, mix, A.data(), true, a); pose_dq(v, mix, N.data(), true, b);
    CHECK(memcmp(a, b, 12) == 0 && memcmp(a, v, 12) != 0);
    // all-zero weights: NaN
    const swr_skin_vertex zero{{0, 1, 2, 3}, {0, 0, 0, 0}};
    pose_dq(v, zero, A.data(), true, o);
    CHECK(std::isnan(o[0]) && std::isnan(o[1]) && std::isnan(o[2]));
}

static void scenario(uint32_t devices, int nv, int ntri) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int B = (int)devices;
    const int W = 64, H = 192;
    Scene s = make_scene(nv, ntri, 5);
    s.sk[0] = swr_skin_vertex{{0, 1, 2, 5}, {0.0f, 0.0f, 0.0f, 0.0f}};       // a zero blend: NaN in the stream, compared as NaN
    const std::vector<float> DA = make_dq(6, 0.25f), DB = make_dq(9, -0.5f), MA = make_pose(6, 0.25f), MB = make_pose(9, -0.5f);
    const Pose dA{DA.data(), true}, dB{DB.data(), true}, mA{MA.data(), false}, mB{MB.data(), false};
    Targets T;
    T.count = 3; T.nrm = true;
    T.dp.resize((size_t)3 * nv * 3); T.dn.resize(T.dp.size());
    for (size_t k = 0; k < T.dp.size(); k++) { T.dp[k] = 0.001f * (float)(k % 113) - 0.05f; T.dn[k] = 0.01f * (float)(k % 37) - 0.1f; }
    const swr_morph_targets td{T.dp.data(), T.dn.data(), nv, 3, 0};
    const float wA[3] = {0.75f, 0.0f, -0.5f}, wB[3] = {0.25f, 1.0f, 0.0f};
    std::vector<float> d((size_t)W * H);
    float m[16];
    // before a scene, before a skin
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_ERR_NO_SCENE);
    CHECK(std::string(swr_last_error(c)).find("swr_pose_set_dq") != std::string::npos);
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_ERR_BAD_ARG);
    { const std::string e = swr_last_error(c); CHECK(e.find("swr_pose_set_dq needs swr_scene_skin") != std::string::npos); }
    CHECK(swr_pose_set_dq(c, nullptr, 0) == SWR_ERR_BAD_ARG);
    // 1024 joints: the largest table, read to its last float; one fewer is refused
    { Scene top = s; top.sk[nv - 1].joint[3] = SWR_SKIN_MAX_JOINTS - 1; CHECK(swr_scene_skin(c, top.sk.data(), nv) == SWR_OK);
      const std::vector<float> big = make_dq(SWR_SKIN_MAX_JOINTS, 0.1f);
      CHECK(swr_pose_set_dq(c, big.data(), SWR_SKIN_MAX_JOINTS - 1) == SWR_ERR_BAD_ARG);
      CHECK(swr_pose_set_dq(c, big.data(), SWR_SKIN_MAX_JOINTS + 1) == SWR_ERR_UNSUPPORTED);
      expect_no_launch("refused poses");
      CHECK(swr_pose_set_dq(c, big.data(), SWR_SKIN_MAX_JOINTS) == SWR_OK);
      expect_dq_stream(top, nullptr, nullptr, Pose{big.data(), true}, false, B, "1024 joints"); }
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);                        // a new skin: back to the bind pose
    expect_dq_stream(s, nullptr, nullptr, BIND, false, B, "a new skin restores the bind pose");
    // every refusal; the pose and the stream stay
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, dA, false, B, "dual-quaternion pose A");
    CHECK(swr_pose_set_dq(nullptr, DA.data(), 6) == SWR_ERR_BAD_ARG);
    CHECK(swr_pose_set_dq(c, DA.data(), -1) == SWR_ERR_BAD_ARG);
    CHECK(swr_pose_set_dq(c, DA.data(), 5) == SWR_ERR_BAD_ARG);
    { const std::string e = swr_last_error(c);
      CHECK(e.find("swr_pose_set_dq: 5 joints") != std::string::npos && e.find("joint index 5") != std::string::npos); }
    CHECK(swr_pose_set_dq(c, DA.data(), 0) == SWR_ERR_BAD_ARG);
    CHECK(swr_pose_set_dq(c, nullptr, 6) == SWR_ERR_BAD_ARG);
    CHECK(std::string(swr_last_error(c)).find("without dual quaternions") != std::string::npos);
    CHECK(swr_pose_set_dq(c, DA.data(), SWR_SKIN_MAX_JOINTS + 1) == SWR_ERR_UNSUPPORTED);
    CHECK(swr_pose_set(c, MA.data(), 5) == SWR_ERR_BAD_ARG);                   // a refused matrix pose leaves the dual-quaternion one
    expect_no_launch("refused poses");
    // a restream right after the refusals: the pose in effect is still dual-quaternion pose A
    if (ntri >= 4) {
        swr_draw_item items[2] = {{0, 3 * (int64_t)(ntri / 2), {}}, {3 * (int64_t)(ntri / 2), 3 * (int64_t)(ntri - ntri / 2), {}}};
        tagm(items[0].transform, 5.0f); tagm(items[1].transform, 6.0f);
        CHECK(swr_draw_list(c, items, 2, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        CHECK(swr_sync(c) == SWR_OK);
        expect_dq_stream(s, nullptr, nullptr, dA, false, B, "pose A after the stream was cut (restream)");
    }
    // behind an un-waited frame: the frame completes as it was posted
    tagm(m, 3.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_pose_set_dq(c, DB.data(), 9) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, dB, false, B, "pose B behind a frame");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 3.0f));
    // ... and an overflowed one is repaired by the call, before the stream changes
    swr::g_fake_fill.store(5000);
    tagm(m, 4.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_OK);
    swr::g_fake_fill.store(7);
    expect_dq_stream(s, nullptr, nullptr, dA, false, B, "pose A behind an overflowed frame");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 4.0f));
    // attributes while the pose is in effect: the normals are rotated too
    const int nrm_before = g_dq_nrm_launches.load();
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, dA, true, B, "attributes under pose A");
    CHECK(g_dq_nrm_launches.load() == nrm_before + B);
    // morph targets arrive under the pose, weights are set, new targets zero them: the pose is re-applied as a dual-quaternion pose
    CHECK(swr_scene_morph(c, &td) == SWR_OK);
    expect_no_launch("new targets on an unmorphed scene change nothing");
    CHECK(swr_morph_set(c, wA, 3) == SWR_OK);
    expect_dq_stream(s, &T, wA, dA, true, B, "weights A under pose A");
    CHECK(swr_pose_set_dq(c, DB.data(), 9) == SWR_OK);
    expect_dq_stream(s, &T, wA, dB, true, B, "pose B keeps weights A");
    CHECK(swr_morph_set(c, wB, 3) == SWR_OK);
    expect_dq_stream(s, &T, wB, dB, true, B, "weights B under pose B");
    CHECK(swr_scene_morph(c, &td) == SWR_OK);                                  // (swr_scene_morph with weights set: every weight 0)
    expect_dq_stream(s, nullptr, nullptr, dB, true, B, "new targets: pose B alone");
    CHECK(swr_morph_set(c, wA, 3) == SWR_OK);
    expect_dq_stream(s, &T, wA, dB, true, B, "weights A again");
    CHECK(swr_morph_set(c, nullptr, 0) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, dB, true, B, "NULL weights: pose B alone");
    // matrix pose -> dual-quaternion pose -> matrix pose -> bind: the last call of either kind is the pose
    const int v_before = g_vertex_launches.load(), q_before = g_dq_launches.load();
    CHECK(swr_pose_set(c, MA.data(), 6) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, mA, true, B, "matrix pose A");
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, dA, true, B, "dual-quaternion pose A after a matrix pose");
    CHECK(swr_pose_set(c, MB.data(), 9) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, mB, true, B, "matrix pose B after a dual-quaternion pose");
    CHECK(g_vertex_launches.load() == v_before + 2 * B && g_dq_launches.load() == q_before + B);
    if (ntri >= 4) {                                                            // ... and a restream re-applies it as a matrix pose
        swr_draw_item items[2] = {{0, 3, {}}, {3, 3 * (int64_t)(ntri - 1), {}}};      // (another cut: the stream is built anew)
        tagm(items[0].transform, 7.0f); tagm(items[1].transform, 8.0f);
        CHECK(swr_draw_list(c, items, 2, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        CHECK(swr_sync(c) == SWR_OK);
        expect_dq_stream(s, nullptr, nullptr, mB, true, B, "matrix pose B after the stream was cut again");
    }
    CHECK(swr_pose_set(c, nullptr, 0) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, BIND, true, B, "the bind pose");
    // each NULL, 0 call after the other kind
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, dA, true, B, "pose A");
    CHECK(swr_pose_set(c, nullptr, 0) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, BIND, true, B, "swr_pose_set(NULL, 0) after a dual-quaternion pose");
    CHECK(swr_pose_set(c, MA.data(), 6) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, mA, true, B, "matrix pose A");
    CHECK(swr_pose_set_dq(c, nullptr, 0) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, BIND, true, B, "swr_pose_set_dq(NULL, 0) after a matrix pose");
    CHECK(swr_pose_set_dq(c, nullptr, 0) == SWR_OK);
    CHECK(swr_pose_set(c, nullptr, 0) == SWR_OK);
    expect_no_launch("the bind pose twice");
    // a matrix pose right after a bind restored from the other kind is a matrix pose (the kind does not linger)
    CHECK(swr_pose_set_dq(c, DB.data(), 9) == SWR_OK);
    (void)take_records();
    CHECK(swr_pose_set_dq(c, nullptr, 0) == SWR_OK);
    (void)take_records();
    CHECK(swr_pose_set(c, MB.data(), 9) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, mB, true, B, "matrix pose B after bind after a dual-quaternion pose");
    // a new skin drops the pose and its kind; a removed skin refuses the call
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, dA, true, B, "pose A again");
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, BIND, true, B, "a new skin");
    CHECK(swr_pose_set(c, MA.data(), 6) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, mA, true, B, "a matrix pose on the new skin");
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_OK);
    (void)take_records();
    CHECK(swr_scene_skin(c, nullptr, 0) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, BIND, true, B, "the skin removed");
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_ERR_BAD_ARG);
    // an upload drops skin, pose and kind
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, dA, true, B, "pose A before the upload");
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_pose_set_dq(c, DA.data(), 6) == SWR_ERR_BAD_ARG);
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    expect_no_launch("an upload drops the pose");
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    CHECK(swr_pose_set(c, MB.data(), 9) == SWR_OK);
    expect_dq_stream(s, nullptr, nullptr, mB, true, B, "a matrix pose on the new scene");
    swr_context_destroy(c);
}

// a failed context returns its sticky error
static void failed_context(uint32_t devices) {
    swr_config cfg{0, devices, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const Scene s = make_scene(300, 100, 2);
    const std::vector<float> A = make_dq(3, 0.0f);
    CHECK(swr_scene_upload(c, s.v.data(), 300, s.idx.data(), 300) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    CHECK(swr_scene_skin(c, s.sk.data(), 300) == SWR_OK);
    CHECK(swr_pose_set_dq(c, A.data(), 3) == SWR_OK);
    (void)take_records();
    float m[16];
    tagm(m, 1.0f);
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, SWR_FLAG_DEPTH_TEST);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    (void)take_records();
    CHECK(swr_pose_set_dq(c, A.data(), 3) == SWR_ERR_HIP);
    CHECK(swr_pose_set_dq(c, nullptr, 0) == SWR_ERR_HIP);
    expect_no_launch("a failed context");
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    model_facts();
    scenario(1, 300, 200);
    scenario(3, 300, 200);
    scenario(1, 3, 1);              // one triangle: one ragged group
    scenario(3, 3, 1);
    scenario(1, 130, 129);          // 64 * 2 + 1 slots
    scenario(3, 130, 129);
    failed_context(1);
    failed_context(2);
    CHECK(g_dq_launches.load() > 0 && g_dq_nrm_launches.load() > 0 && g_vertex_launches.load() > 0);
    CHECK(g_stream_launches.load() > g_dq_launches.load() + g_vertex_launches.load());
    return report("skin dq host test");
}
