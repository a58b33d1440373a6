// The host side of the computed normals (software-renderer_amd/csrc/swr_api.hip: single_scene_normals — the checks, the adjacency it
// builds by a counting sort, its upload — and the stage enqueue_pose gained between the vertex passes and the stream write, the group
// fan-out) on the fake HIP runtime of tests/host/hip_stub, under the address and undefined-behaviour sanitizers.  The stand-ins of
// swr::launch_face_normals, launch_vertex_normals and launch_flat_normals are the launch set's (hip_stub/stub_launch.cpp): CPU loops
// over the header's arithmetic that read and write every element of every array they are handed, at the sizes swr_internal.h states,
// and note when they were called relative to the other launches (hip_stub/stub_launch.h has the notes and the adjacency copy).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/normals_host_test.cpp -lpthread
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "host_test.h"

// ---- the model ------------------------------------------------------------------------------------------------------------------------
enum { UPLOADED = SWR_NORMALS_UPLOADED, SMOOTH = SWR_NORMALS_SMOOTH, FLAT = SWR_NORMALS_FLAT };

// the shape a scene is in: morphed by w over T (either NULL: not), then in `pose` (NULL: not; dq: dual quaternions)
struct Shape { const Targets* T; const float* w; const float* pose; bool dq; };

static std::vector<float> positions(const Scene& s, const Shape& sh) {
    const int64_t nv = (int64_t)s.v.size();
    std::vector<float> out((size_t)nv * 3);
    for (int64_t i = 0; i < nv; i++) {
        float p[3];
        memcpy(p, s.v[i].xyz, 12);
        if (sh.T && sh.w) morph(p, sh.T->dp.data(), sh.w, sh.T->count, nv, i, p);
        if (sh.pose) {
            float q[3];
            if (sh.dq) pose_dq(p, s.sk[i], sh.pose, true, q); else blend(p, s.sk[i], sh.pose, true, q);
            memcpy(p, q, 12);
        }
        memcpy(&out[3 * (size_t)i], p, 12);
    }
    return out;
}
static bool same3(const float* a, const float* b) {
    for (int j = 0; j < 3; j++) if (memcmp(a + j, b + j, 4) != 0 && !(std::isnan(a[j]) && std::isnan(b[j]))) return false;
    return true;
}
// "Computed normals" per corner of the index array, by the definition: for vertex i, every corner in ascending order that names it
static std::vector<float> corner_normals(const Scene& s, const std::vector<float>& pos, int mode, bool flip) {
    const int64_t ntri = (int64_t)s.idx.size() / 3, nv = (int64_t)s.v.size();
    std::vector<float> face((size_t)ntri * 3), out((size_t)ntri * 9);
    for (int64_t p = 0; p < ntri; p++)
        face_of(&pos[3 * (size_t)s.idx[3 * p]], &pos[3 * (size_t)s.idx[3 * p + 1]], &pos[3 * (size_t)s.idx[3 * p + 2]], flip, &face[3 * (size_t)p]);
    if (mode == FLAT) {
        for (int64_t e = 0; e < 3 * ntri; e++) memcpy(&out[3 * (size_t)e], &face[3 * (size_t)(e / 3)], 12);
        return out;
    }
    std::vector<float> n((size_t)nv * 3, 0.0f);
    for (int64_t e = 0; e < 3 * ntri; e++)
        for (int j = 0; j < 3; j++) n[3 * (size_t)s.idx[e] + j] = n[3 * (size_t)s.idx[e] + j] + face[3 * (size_t)(e / 3) + j];
    for (int64_t i = 0; i < nv; i++) normalise(&n[3 * (size_t)i]);
    for (int64_t e = 0; e < 3 * ntri; e++) memcpy(&out[3 * (size_t)e], &n[3 * (size_t)s.idx[e]], 12);
    return out;
}

// the stream every band must hold under a computed mode, and the launches that wrote it: one stream launch per band — with the
// normals under SMOOTH, without under FLAT, where the flat launch on the same stream arrays wrote them
static void expect_computed(const Scene& s, const Shape& sh, int mode, bool flip, int bands, const char* what) {
    const std::vector<Record> records = take_records();
    std::vector<FlatNote> flats;
    { std::lock_guard<std::mutex> lk(g_note_m); flats.swap(g_flat_notes); }
    if ((int)records.size() != bands || (int)flats.size() != (mode == FLAT ? bands : 0)) {
        std::printf("FAIL %s: %zu stream launches and %zu flat launches for %d bands\n", what, records.size(), flats.size(), bands); fails++; return;
    }
    const int64_t ntri = (int64_t)s.idx.size() / 3;
    const std::vector<float> pos = positions(s, sh), nrm = corner_normals(s, pos, mode, flip);
    for (const Record& r : records) {
        const float4* tri_nrm = r.tri_nrm;
        if (mode == FLAT) {
            tri_nrm = nullptr;
            for (const FlatNote& f : flats) if (f.tri_xyz == r.tri_xyz) tri_nrm = f.tri_nrm;
        }
        bool ok = r.ntri == ntri && r.nrm == (mode == SMOOTH) && tri_nrm != nullptr;
        for (int64_t e = 0; ok && e < 3 * ntri; e++)
            ok = same3(&r.tri_xyz[e].x, &pos[3 * (size_t)s.idx[e]]) && same3(&tri_nrm[e].x, &nrm[3 * (size_t)e]);
        if (!ok) { std::printf("FAIL %s: the stream is not the model's (mode %d flip %d)\n", what, mode, (int)flip); fails++; }
    }
}

static int set_mode(swr_context* c, int mode, bool flip = false) {
    const swr_normals n{mode, flip ? (uint32_t)SWR_NORMALS_FLIP : 0u, {0, 0}};
    return swr_scene_normals(c, &n);
}

// ---- the hub scene of tests/normals_model.py (the topology; the coordinates are this program's) ----------------------------------------
static Scene hub_scene() {
    const int nv = 312;
    Scene s = make_scene(nv, 0, 2);
    for (int j = 0; j < 300; j++) { s.idx.push_back(0); s.idx.push_back(1 + j); s.idx.push_back(1 + (j + 1) % 300); }
    const int64_t extra[12] = {301, 302, 303, 305, 305, 306, 307, 308, 309, 308, 310, 311};
    s.idx.insert(s.idx.end(), extra, extra + 12);
    for (int i = 0; i < nv; i++) s.v[i].xyz[2] = 0.1f + 0.003f * (float)((i * 37) % 101);       // (not coplanar)
    s.v[307].xyz[0] = NAN;
    return s;
}

static void check_hub_adjacency(const Scene& s) {
    std::vector<uint32_t> off, tri;
    { std::lock_guard<std::mutex> lk(g_note_m); off = g_adj_off; tri = g_adj_tri; }
    const size_t nv = s.v.size(), corners = s.idx.size();
    CHECK(off.size() == nv + 1 && tri.size() == corners && off[0] == 0 && off[nv] == corners);
    if (off.size() != nv + 1 || tri.size() != corners) return;
    size_t at = 0;
    bool ok = true;
    for (size_t i = 0; i < nv; i++) {                       // by the definition: the corners that name i, ascending
        ok = ok && off[i] == at;
        for (size_t e = 0; e < corners; e++)
            if ((size_t)s.idx[e] == i) { ok = ok && at < tri.size() && tri[at] == (uint32_t)(e / 3); at++; }
    }
    CHECK(ok && at == corners);
    CHECK(off[1] - off[0] == 300 && tri[0] == 0 && tri[299] == 299);                            // the hub: longer than a workgroup
    CHECK(off[2] - off[1] == 2 && tri[off[1]] == 0 && tri[off[1] + 1] == 299);                  // a ring vertex
    CHECK(off[302] - off[301] == 1 && off[305] - off[304] == 0);                                // the lone triangle; no triangle at all
    CHECK(off[306] - off[305] == 2 && tri[off[305]] == 301 && tri[off[305] + 1] == 301);        // named twice: kept twice
    CHECK(off[309] - off[308] == 2 && tri[off[308]] == 302 && tri[off[308] + 1] == 303);
}

// ---- scenarios --------------------------------------------------------------------------------------------------------------------------
// one band: which launches a call makes under each mode, and in which order
static void sequences() {
    swr_config cfg{0, 1, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int nv = 300, ntri = 200;
    const Scene s = make_scene(nv, ntri, 5);
    const std::vector<float> A = make_pose(6, 0.25f);
    std::vector<float> Q(8 * 6, 0.0f);
    for (int j = 0; j < 6; j++) { Q[8 * (size_t)j + 3] = 1.0f; Q[8 * (size_t)j + 4] = 0.01f * (float)j; }
    Targets T;                                              // two dense targets with normal deltas
    T.count = 2; T.nrm = true;
    T.dp.resize((size_t)2 * nv * 3); T.dn.resize(T.dp.size());
    for (size_t k = 0; k < T.dp.size(); k++) { T.dp[k] = 0.001f * (float)((k * 7) % 113) - 0.05f; T.dn[k] = 0.01f * (float)((k * 5) % 37); }
    std::vector<uint32_t> every((size_t)nv);
    for (int i = 0; i < nv; i++) every[(size_t)i] = (uint32_t)i;
    const swr_morph_sparse_target st[2] = {{every.data(), T.dp.data(), T.dn.data(), nv}, {every.data(), T.dp.data() + (size_t)nv * 3, T.dn.data() + (size_t)nv * 3, nv}};
    const swr_morph_sparse sparse{st, nv, 2, 0};
    const swr_morph_targets dense{T.dp.data(), T.dn.data(), nv, 2, 0};
    const float w[2] = {0.75f, -0.5f};
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    expect_no_launch("a scene without a mode, a morph or a pose");

    struct Step { const char* name; int morph; int pose; };     // morph: 0 none, 1 dense, 2 sparse; pose: 0 none, 1 matrices, 2 dual quaternions, 3 the combined call
    const Step steps[] = {{"no deformation", 0, 0}, {"dense morph", 1, 0}, {"sparse morph", 2, 0}, {"matrix pose", 0, 1},
                          {"dual-quaternion pose", 0, 2}, {"the combined call", 2, 3}, {"dense morph and dual quaternions", 1, 2}};
    for (int mode : {SMOOTH, FLAT, UPLOADED})
        for (const Step& st_ : steps) {
            // from the uploaded scene: no targets, the bind pose, no mode
            CHECK(swr_scene_morph(c, nullptr) == SWR_OK);
            CHECK(swr_pose_set(c, nullptr, 0) == SWR_OK);
            CHECK(swr_scene_normals(c, nullptr) == SWR_OK);
            (void)take_records();
            { std::lock_guard<std::mutex> lk(g_note_m); g_flat_notes.clear(); }
            if (st_.morph == 1) CHECK(swr_scene_morph(c, &dense) == SWR_OK);
            if (st_.morph == 2) CHECK(swr_scene_morph_sparse(c, &sparse) == SWR_OK);
            expect_no_launch("new targets");
            const bool flip = mode == FLAT;
            const int face0 = g_face_launches.load(), vn0 = g_vnrm_launches.load(), flat0 = g_flat_launches.load();
            CHECK(set_mode(c, mode, flip) == SWR_OK);
            const Shape bind{nullptr, nullptr, nullptr, false};
            if (mode == UPLOADED) expect_no_launch("UPLOADED on a context without a mode");
            else expect_computed(s, bind, mode, flip, 1, st_.name);
            CHECK(g_face_launches.load() == face0 + (mode == SMOOTH) && g_vnrm_launches.load() == vn0 + (mode == SMOOTH) && g_flat_launches.load() == flat0 + (mode == FLAT));
            // the deforming call
            const LaunchCounts before = launch_counts();
            const int mn0 = g_morph_nrm_launches.load() + g_sparse_nrm_launches.load(), dqn0 = g_dq_nrm_launches.load();
            const int face1 = g_face_launches.load(), vn1 = g_vnrm_launches.load(), flat1 = g_flat_launches.load();
            const bool dq = st_.pose == 2;
            if (st_.pose == 3) CHECK(swr_morph_pose_set(c, w, 2, A.data(), 6, SWR_POSE_MATRICES) == SWR_OK);
            else {
                if (st_.morph) CHECK(swr_morph_set(c, w, 2) == SWR_OK);
                if (st_.morph && st_.pose) (void)take_records();        // (two calls: the second one's stream is the one checked)
                if (st_.morph && st_.pose) { std::lock_guard<std::mutex> lk(g_note_m); g_flat_notes.clear(); }
                if (st_.pose == 1) CHECK(swr_pose_set(c, A.data(), 6) == SWR_OK);
                if (st_.pose == 2) CHECK(swr_pose_set_dq(c, Q.data(), 6) == SWR_OK);
            }
            const Shape shape{st_.morph ? &T : nullptr, st_.morph ? w : nullptr, st_.pose ? (dq ? Q.data() : A.data()) : nullptr, dq};
            const int calls = (st_.morph && st_.pose && st_.pose != 3) ? 2 : (st_.morph || st_.pose) ? 1 : 0;
            const LaunchCounts after = launch_counts();
            if (!calls) continue;
            CHECK(after.stream == before.stream + calls);
            CHECK(after.morph == before.morph + (st_.morph ? calls : 0) && after.skin == before.skin + (st_.pose ? 1 : 0));
            if (mode == UPLOADED) {
                // today's sequence exactly: the vertex passes carry the normals, one stream launch with them, nothing else
                if (dq) {
                    // (host_test.h's expect_stream poses with matrices: the dual-quaternion stream is checked through the model above)
                    const std::vector<Record> r = take_records();
                    CHECK(r.size() == 1 && r[0].nrm);
                } else expect_stream(s, st_.morph ? &T : nullptr, st_.morph ? w : nullptr, st_.pose ? A.data() : nullptr, true, 1, st_.name);
                CHECK(g_face_launches.load() == face1 && g_vnrm_launches.load() == vn1 && g_flat_launches.load() == flat1);
                CHECK(g_morph_nrm_launches.load() + g_sparse_nrm_launches.load() == mn0 + (st_.morph ? calls : 0));
                CHECK(g_dq_nrm_launches.load() == dqn0 + (dq ? 1 : 0));
                continue;
            }
            expect_computed(s, shape, mode, flip, 1, st_.name);
            // the NRM = false vertex passes: no morph and no dual-quaternion launch was handed normals
            CHECK(g_morph_nrm_launches.load() + g_sparse_nrm_launches.load() == mn0 && g_dq_nrm_launches.load() == dqn0);
            CHECK(g_face_launches.load() == face1 + (mode == SMOOTH ? calls : 0) && g_vnrm_launches.load() == vn1 + (mode == SMOOTH ? calls : 0));
            CHECK(g_flat_launches.load() == flat1 + (mode == FLAT ? calls : 0));
            // the order of the last call: vertex passes, then the normals, then the stream (SMOOTH); the stream, then the normals (FLAT)
            std::lock_guard<std::mutex> lk(g_note_m);
            if (mode == SMOOTH) {
                CHECK(g_face_at.stream == after.stream - 1 && g_face_at.skin == after.skin && g_face_at.morph == after.morph);
                CHECK(g_vnrm_after_faces == g_face_launches.load());
            } else {
                CHECK(g_flat_at.stream == after.stream && g_flat_at.skin == after.skin && g_flat_at.morph == after.morph);
            }
        }
    swr_context_destroy(c);
}

// the errors, the lifetime and the hub's adjacency, on 1 and 3 bands
static void scenario(uint32_t devices) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int B = (int)devices;
    const Scene s = hub_scene();
    const int nv = (int)s.v.size();
    const std::vector<float> A = make_pose(3, 0.25f), Bp = make_pose(4, -0.5f);
    const Shape bind{nullptr, nullptr, nullptr, false}, inA{nullptr, nullptr, A.data(), false}, inB{nullptr, nullptr, Bp.data(), false};
    float m[16];
    std::vector<float> d((size_t)64 * 192);
    // before a scene
    CHECK(set_mode(c, SMOOTH) == SWR_ERR_NO_SCENE);
    CHECK(swr_scene_normals(c, nullptr) == SWR_ERR_NO_SCENE);
    CHECK(swr_scene_normals(nullptr, nullptr) == SWR_ERR_BAD_ARG);
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_target_set(c, 64, 192, 0, 192) == SWR_OK);
    auto refusals = [&] {
        swr_normals n{SMOOTH, 0, {0, 0}};
        n.mode = 3; CHECK(swr_scene_normals(c, &n) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("swr_scene_normals: unknown mode 3") != std::string::npos);
        n.mode = -1; CHECK(swr_scene_normals(c, &n) == SWR_ERR_BAD_ARG);
        n.mode = FLAT; n.flags = 2; CHECK(swr_scene_normals(c, &n) == SWR_ERR_BAD_ARG);
        n.flags = 0x80000001u; CHECK(swr_scene_normals(c, &n) == SWR_ERR_BAD_ARG);
        n.flags = 1; n.reserved[0] = 1; CHECK(swr_scene_normals(c, &n) == SWR_ERR_BAD_ARG);
        n.reserved[0] = 0; n.reserved[1] = -1; CHECK(swr_scene_normals(c, &n) == SWR_ERR_BAD_ARG);
        n.mode = UPLOADED; n.flags = 0; CHECK(swr_scene_normals(c, &n) == SWR_ERR_BAD_ARG);        // (reserved still set)
        CHECK(swr_scene_normals(nullptr, &n) == SWR_ERR_BAD_ARG);
    };
    refusals();
    expect_no_launch("refused modes");
    // normals before attributes: kept, nothing to write yet; in effect when the attributes arrive
    const int vn0 = g_vnrm_launches.load();
    CHECK(set_mode(c, SMOOTH) == SWR_OK);
    expect_no_launch("a mode on a scene without attributes");
    CHECK(g_vnrm_launches.load() == vn0);
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    CHECK(swr_pose_set(c, A.data(), 3) == SWR_OK);
    expect_stream(s, nullptr, nullptr, A.data(), false, B, "a pose under a mode that is not in effect yet");
    CHECK(g_vnrm_launches.load() == vn0);
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    expect_computed(s, inA, SMOOTH, false, B, "the attributes arrive: SMOOTH in pose A");
    check_hub_adjacency(s);
    // every refusal leaves mode and scene: the next pose is still SMOOTH
    refusals();
    expect_no_launch("refused modes under SMOOTH");
    CHECK(set_mode(c, SMOOTH) == SWR_OK);
    expect_no_launch("the same mode again");
    CHECK(swr_pose_set(c, Bp.data(), 4) == SWR_OK);
    expect_computed(s, inB, SMOOTH, false, B, "normals between two poses");
    // the mode behind an un-waited frame: the frame completes as it was posted; and behind an overflowed one
    tagm(m, 3.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(set_mode(c, FLAT, true) == SWR_OK);
    expect_computed(s, inB, FLAT, true, B, "FLAT with FLIP behind a frame");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 3.0f));
    swr::g_fake_fill.store(5000);
    tagm(m, 4.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(set_mode(c, SMOOTH, true) == SWR_OK);
    swr::g_fake_fill.store(7);
    expect_computed(s, inB, SMOOTH, true, B, "SMOOTH with FLIP behind an overflowed frame");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 4.0f));
    check_hub_adjacency(s);
    // kept across the skin, the targets and the poses; new attributes are gathered, then replaced again
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);               // (a new skin restores the bind pose)
    expect_computed(s, bind, SMOOTH, true, B, "a new skin: the bind pose, still SMOOTH");
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    expect_computed(s, bind, SMOOTH, true, B, "new attributes under SMOOTH without a deformation");
    // a draw list over two ranges cuts the stream (restream): the rebuilt stream gets its normals again
    {
        const int64_t ntri = (int64_t)s.idx.size() / 3;
        swr_draw_item items[2] = {{0, 3 * (ntri / 2), {}}, {3 * (ntri / 2), 3 * (ntri - ntri / 2), {}}};
        tagm(items[0].transform, 5.0f); tagm(items[1].transform, 6.0f);
        CHECK(swr_draw_list(c, items, 2, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        CHECK(swr_sync(c) == SWR_OK);
        expect_computed(s, bind, SMOOTH, true, B, "after the stream was cut");
    }
    CHECK(swr_pose_set(c, A.data(), 3) == SWR_OK);
    expect_computed(s, inA, SMOOTH, true, B, "pose A after the new skin");
    // UPLOADED and NULL restore today's stream; a second time there is nothing to do
    CHECK(set_mode(c, UPLOADED) == SWR_OK);
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "UPLOADED: the uploaded normals, posed");
    CHECK(swr_scene_normals(c, nullptr) == SWR_OK);
    expect_no_launch("NULL after UPLOADED");
    CHECK(set_mode(c, FLAT) == SWR_OK);
    expect_computed(s, inA, FLAT, false, B, "FLAT in pose A");
    CHECK(swr_scene_normals(c, nullptr) == SWR_OK);
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "NULL: the uploaded normals, posed");
    // an upload drops the mode (and the adjacency: the next SMOOTH builds the new scene's)
    CHECK(set_mode(c, SMOOTH) == SWR_OK);
    (void)take_records();
    const Scene s2 = make_scene(130, 129, 2);
    CHECK(swr_scene_upload(c, s2.v.data(), 130, s2.idx.data(), (int64_t)s2.idx.size()) == SWR_OK);
    CHECK(swr_scene_attributes(c, s2.a.data(), 130) == SWR_OK);
    CHECK(swr_scene_skin(c, s2.sk.data(), 130) == SWR_OK);
    const int face0 = g_face_launches.load(), flat0 = g_flat_launches.load();
    CHECK(swr_pose_set(c, A.data(), 3) == SWR_OK);
    expect_stream(s2, nullptr, nullptr, A.data(), true, B, "an upload drops the mode");
    CHECK(g_face_launches.load() == face0 && g_flat_launches.load() == flat0);
    CHECK(set_mode(c, SMOOTH) == SWR_OK);
    expect_computed(s2, Shape{nullptr, nullptr, A.data(), false}, SMOOTH, false, B, "SMOOTH on the new scene: its own adjacency");
    { std::lock_guard<std::mutex> lk(g_note_m); CHECK(g_adj_off.size() == 131 && g_adj_tri.size() == 387); }
    // a scene without triangles and one without vertices: legal, nothing is launched
    CHECK(swr_scene_upload(c, s2.v.data(), 130, s2.idx.data(), 2) == SWR_OK);
    CHECK(swr_scene_attributes(c, s2.a.data(), 130) == SWR_OK);
    CHECK(set_mode(c, SMOOTH) == SWR_OK && set_mode(c, FLAT) == SWR_OK && set_mode(c, UPLOADED) == SWR_OK);
    CHECK(swr_scene_upload(c, nullptr, 0, nullptr, 0) == SWR_OK);
    CHECK(set_mode(c, SMOOTH) == SWR_OK && set_mode(c, FLAT) == SWR_OK);
    (void)take_records();
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
    CHECK(swr_scene_attributes(c, s.a.data(), 300) == SWR_OK);
    float m[16];
    tagm(m, 1.0f);
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, SWR_FLAG_DEPTH_TEST);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    (void)take_records();
    CHECK(set_mode(c, SMOOTH) == SWR_ERR_HIP);
    CHECK(set_mode(c, 7) == SWR_ERR_HIP);
    CHECK(swr_scene_normals(c, nullptr) == SWR_ERR_HIP);
    expect_no_launch("a failed context");
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    sequences();
    scenario(1);
    scenario(3);
    failed_context(1);
    failed_context(2);
    CHECK(g_face_launches.load() > 0 && g_vnrm_launches.load() > 0 && g_flat_launches.load() > 0 && g_flip_launches.load() > 0);
    return report("normals host test");
}
