// The host side of the sparse morph targets and of swr_morph_pose_set (software-renderer_amd/csrc/swr_api.hip:
// single_scene_morph_sparse — the checks, the rows it builds, their upload through the staging chunks, the pre-fill of the morphed
// arrays — enqueue_pose with sparse targets, single_morph_pose_set and the checks it shares with single_morph_set and single_pose_set,
// the group fan-out) on the fake HIP runtime of tests/host/hip_stub, under the address and undefined-behaviour sanitizers.  The
// stand-in of swr::launch_morph_sparse is the launch set's (hip_stub/stub_launch.cpp): a CPU loop over the header's arithmetic that
// checks the rows it is handed and reads and writes every element of every array, at the sizes swr_internal.h states.  Like the
// kernel it writes the position (and normal) quads of the touched vertices only: everything else of the morphed arrays is the host
// layer's pre-fill, which the skin stream launch then reads.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/morph_sparse_host_test.cpp -lpthread
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host_test.h"

// sparse targets as the caller holds them
struct Sparse {
    std::vector<std::vector<uint32_t>> idx;
    std::vector<std::vector<float>> dp, dn;
    bool nrm = false;
    std::vector<swr_morph_sparse_target> recs;
    swr_morph_sparse desc(int64_t nv) {
        recs.clear();
        for (size_t t = 0; t < idx.size(); t++)
            recs.push_back(swr_morph_sparse_target{idx[t].empty() ? nullptr : idx[t].data(), idx[t].empty() ? nullptr : dp[t].data(),
                                                   nrm && !idx[t].empty() ? dn[t].data() : nullptr, (int64_t)idx[t].size()});
        return swr_morph_sparse{recs.data(), nv, (int32_t)recs.size(), 0};
    }
    // the dense targets with zero rows where a target lists nothing: on these scenes (no -0 coordinate, finite weights, the non-finite
    // target only ever at weight 0) the header's dense loop gives the sparse loop's bits, so host_test.h's model serves
    Targets dense(int nv) const {
        Targets T;
        T.count = (int)idx.size(); T.nrm = nrm;
        T.dp.assign((size_t)T.count * nv * 3, 0.0f);
        if (nrm) T.dn.assign(T.dp.size(), 0.0f);
        for (size_t t = 0; t < idx.size(); t++)
            for (size_t j = 0; j < idx[t].size(); j++)
                for (int c = 0; c < 3; c++) {
                    T.dp[(t * nv + idx[t][j]) * 3 + c] = dp[t][3 * j + c];
                    if (nrm) T.dn[(t * nv + idx[t][j]) * 3 + c] = dn[t][3 * j + c];
                }
        return T;
    }
    size_t touched(int nv) const {
        std::vector<char> seen((size_t)nv, 0);
        for (const auto& l : idx) for (uint32_t i : l) seen[i] = 1;
        return (size_t)std::count(seen.begin(), seen.end(), 1);
    }
};

// six targets: the even vertices, every third, all of them, every fifth (NaN and infinities: only ever weight 0), none, the last one
static Sparse make_sparse(int nv, bool nrm, float salt) {
    Sparse s;
    s.nrm = nrm;
    s.idx.resize(6); s.dp.resize(6); s.dn.resize(6);
    for (int i = 0; i < nv; i++) {
        if (i % 2 == 0) s.idx[0].push_back((uint32_t)i);
        if (i % 3 == 0) s.idx[1].push_back((uint32_t)i);
        s.idx[2].push_back((uint32_t)i);
        if (i % 5 == 0) s.idx[3].push_back((uint32_t)i);
    }
    s.idx[5].push_back((uint32_t)(nv - 1));
    for (int t = 0; t < 6; t++)
        for (size_t j = 0; j < s.idx[t].size(); j++)
            for (int c = 0; c < 3; c++) {
                const bool bad = t == 3;
                s.dp[t].push_back(bad ? (c == 0 ? NAN : c == 1 ? INFINITY : -INFINITY) : salt + 0.001f * (float)((t * 31 + j * 7 + c * 3) % 113) - 0.05f);
                if (nrm) s.dn[t].push_back(bad ? NAN : 0.01f * (float)((t * 13 + j * 5 + c) % 37) - salt);
            }
    return s;
}

static void scenario(uint32_t devices, int nv, int ntri) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int B = (int)devices;
    const int W = 64, H = 192;
    const Scene s = make_scene(nv, ntri, 5);
    const std::vector<float> A = make_pose(6, 0.25f), Bp = make_pose(9, -0.5f);
    Sparse S = make_sparse(nv, true, 0.02f), S2 = make_sparse(nv, false, -0.01f);
    const Targets T = S.dense(nv), T2 = S2.dense(nv);
    const float wA[6] = {0.75f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f}, wB[6] = {-0.5f, 0.25f, 0.5f, -0.0f, 2.0f, 0.375f};
    const float wZ[6] = {0.0f, -0.0f, 0.0f, -0.0f, 0.0f, -0.0f}, wL[6] = {0, 0, 0, 0, 3.0f, 1.5f};
    std::vector<float> d((size_t)W * H);
    float m[16];
    // before a scene, before targets
    { const swr_morph_sparse t = S.desc(nv); CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_NO_SCENE); }
    CHECK(swr_morph_pose_set(c, wA, 6, A.data(), 6, SWR_POSE_MATRICES) == SWR_ERR_NO_SCENE);
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    CHECK(swr_morph_set(c, wA, 6) == SWR_ERR_BAD_ARG);
    CHECK(std::string(swr_last_error(c)).find("swr_morph_set needs swr_scene_morph first") != std::string::npos);
    CHECK(swr_scene_morph_sparse(c, nullptr) == SWR_OK);             // nothing to remove
    // every refusal of swr_scene_morph_sparse
    auto refusals = [&] {
        swr_morph_sparse t = S.desc(nv);
        auto fresh = [&] { t = S.desc(nv); };
        CHECK(swr_scene_morph_sparse(nullptr, &t) == SWR_ERR_BAD_ARG);
        fresh(); t.vertex_count = nv - 1; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); t.vertex_count = nv + 1; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); t.targets = nullptr; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); t.target_count = 0; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); t.target_count = -1; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); t.reserved = 1; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); t.target_count = SWR_MORPH_MAX_TARGETS + 1; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_UNSUPPORTED);
        fresh(); S.recs[0].count = -1; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); S.recs[2].count = nv + 1; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); S.recs[1].indices = nullptr; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); S.recs[1].position_deltas = nullptr; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        fresh(); S.recs[0].normal_deltas = nullptr; CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);      // normals on some only
        fresh();
        std::vector<uint32_t> ix = S.idx[2];
        S.recs[2].indices = ix.data();
        ix.back() = (uint32_t)nv;                                    // out of range
        CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("target 2, position " + std::to_string(nv - 1)) != std::string::npos);
        ix.back() = (uint32_t)(nv - 1);
        if (nv >= 3) {
            ix[1] = ix[0];                                           // not strictly ascending
            CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
            CHECK(std::string(swr_last_error(c)).find("target 2, position 1") != std::string::npos);
            ix[1] = 2; ix[2] = 1;                                    // descending
            CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_BAD_ARG);
            CHECK(std::string(swr_last_error(c)).find("target 2, position 2") != std::string::npos);
        }
    };
    refusals();
    CHECK(swr_morph_set(c, wA, 6) == SWR_ERR_BAD_ARG);              // still no targets
    expect_no_launch("refused targets");
    // the targets are copied: the caller's arrays are scribbled over and freed on return
    {
        Sparse* tmp = new Sparse(S);
        const swr_morph_sparse t = tmp->desc(nv);
        CHECK(swr_scene_morph_sparse(c, &t) == SWR_OK);
        for (auto& v : tmp->idx) std::fill(v.begin(), v.end(), 0xFFFFFFFFu);
        for (auto& v : tmp->dp) std::fill(v.begin(), v.end(), 1.0e30f);
        for (auto& v : tmp->dn) std::fill(v.begin(), v.end(), -1.0e30f);
        std::fill(tmp->recs.begin(), tmp->recs.end(), swr_morph_sparse_target{});
        delete tmp;
    }
    expect_no_launch("new targets on an unmorphed scene change nothing");
    const int before = g_sparse_launches.load();
    CHECK(swr_morph_set(c, wA, 6) == SWR_OK);
    expect_stream(s, &T, wA, nullptr, false, B, "weights A");
    CHECK(g_sparse_launches.load() == before + B && g_sparse_rows.load() == (int64_t)S.touched(nv));
    // every refusal again, and of swr_morph_set: stream, targets and weights stay
    CHECK(swr_morph_set(c, wB, 5) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_set(c, wB, 7) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_set(c, nullptr, 6) == SWR_ERR_BAD_ARG);
    refusals();
    expect_no_launch("refused weights");
    // weights behind an un-waited frame: the frame completes as it was posted
    tagm(m, 3.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_morph_set(c, wB, 6) == SWR_OK);
    expect_stream(s, &T, wB, nullptr, false, B, "weights B behind a frame (the refusals left the targets in place)");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 3.0f));
    // ... and an overflowed one is repaired by the call, before the stream changes
    swr::g_fake_fill.store(5000);
    tagm(m, 4.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    CHECK(swr_morph_set(c, wA, 6) == SWR_OK);
    swr::g_fake_fill.store(7);
    expect_stream(s, &T, wA, nullptr, false, B, "weights A behind an overflowed frame");
    CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 4.0f));
    // weights that reach only the empty target and the last vertex; every touched vertex is rewritten from the base
    CHECK(swr_morph_set(c, wL, 6) == SWR_OK);
    expect_stream(s, &T, wL, nullptr, false, B, "the empty target and the last vertex");
    CHECK(swr_morph_set(c, wA, 6) == SWR_OK);
    expect_stream(s, &T, wA, nullptr, false, B, "weights A after them: nothing stale");
    // a pose under an active sparse morph, then a morph under an active pose: morph first, then skin
    CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
    expect_no_launch("a skin without a pose");
    CHECK(swr_pose_set(c, A.data(), 6) == SWR_OK);
    expect_stream(s, &T, wA, A.data(), false, B, "pose A under weights A");
    CHECK(swr_morph_set(c, wB, 6) == SWR_OK);
    expect_stream(s, &T, wB, A.data(), false, B, "weights B under pose A");
    // attributes arrive: the pre-fill of the normals is made, the normal deltas given earlier take effect, the pose reads the result
    const int nrm_before = g_sparse_nrm_launches.load();
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    expect_stream(s, &T, wB, A.data(), true, B, "attributes under weights B and pose A");
    CHECK(g_sparse_nrm_launches.load() == nrm_before + B);
    // a draw list over two ranges cuts the stream (restream): morphed and posed again
    if (ntri >= 4) {
        swr_draw_item items[2] = {{0, 3 * (int64_t)(ntri / 2), {}}, {3 * (int64_t)(ntri / 2), 3 * (int64_t)(ntri - ntri / 2), {}}};
        tagm(items[0].transform, 5.0f); tagm(items[1].transform, 6.0f);
        CHECK(swr_draw_list(c, items, 2, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        CHECK(swr_sync(c) == SWR_OK);
        expect_stream(s, &T, wB, A.data(), true, B, "weights B and pose A after the stream was cut");
    }
    // new attributes replace the base normals: the pre-fill is redone
    {
        Scene s2 = s;
        for (auto& a : s2.a) { a.normal[0] = -a.normal[0]; a.normal[1] += 0.125f; }
        CHECK(swr_scene_attributes(c, s2.a.data(), nv) == SWR_OK);
        expect_stream(s2, &T, wB, A.data(), true, B, "new attributes under weights B and pose A");
        CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
        expect_stream(s, &T, wB, A.data(), true, B, "the first attributes again");
    }
    // all-zero weights, of either sign, and NULL restore the posed stream exactly; a second time there is nothing to do
    CHECK(swr_morph_set(c, wZ, 6) == SWR_OK);
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "zero weights: pose A alone");
    CHECK(swr_morph_set(c, nullptr, 0) == SWR_OK);
    CHECK(swr_morph_set(c, wZ, 6) == SWR_OK);
    expect_no_launch("zero weights twice");
    // swr_morph_pose_set against the two calls: the same stream, one skin and one stream launch per band
    {
        CHECK(swr_morph_set(c, wA, 6) == SWR_OK);
        CHECK(swr_pose_set(c, Bp.data(), 9) == SWR_OK);
        (void)take_records();
        const int v0 = g_vertex_launches.load(), s0 = g_stream_launches.load(), m0 = g_sparse_launches.load();
        CHECK(swr_morph_pose_set(c, wB, 6, A.data(), 6, SWR_POSE_MATRICES) == SWR_OK);
        CHECK(g_vertex_launches.load() == v0 + B && g_stream_launches.load() == s0 + B && g_sparse_launches.load() == m0 + B);
        expect_stream(s, &T, wB, A.data(), true, B, "weights B and pose A in one call");
        // each half's errors leave both halves' state
        CHECK(swr_morph_pose_set(c, wA, 5, Bp.data(), 9, SWR_POSE_MATRICES) == SWR_ERR_BAD_ARG);
        CHECK(std::string(swr_last_error(c)).find("swr_morph_pose_set: ") != std::string::npos);
        CHECK(swr_morph_pose_set(c, nullptr, 6, Bp.data(), 9, SWR_POSE_MATRICES) == SWR_ERR_BAD_ARG);
        CHECK(swr_morph_pose_set(c, wA, 6, Bp.data(), 3, SWR_POSE_MATRICES) == SWR_ERR_BAD_ARG);      // the skin uses joint 5
        CHECK(std::string(swr_last_error(c)).find("swr_morph_pose_set: ") != std::string::npos);
        CHECK(swr_morph_pose_set(c, wA, 6, nullptr, 9, SWR_POSE_MATRICES) == SWR_ERR_BAD_ARG);
        CHECK(swr_morph_pose_set(c, wA, 6, Bp.data(), -1, SWR_POSE_MATRICES) == SWR_ERR_BAD_ARG);
        CHECK(swr_morph_pose_set(c, wA, 6, Bp.data(), SWR_SKIN_MAX_JOINTS + 1, SWR_POSE_MATRICES) == SWR_ERR_UNSUPPORTED);
        CHECK(swr_morph_pose_set(c, wA, 6, Bp.data(), 9, 2) == SWR_ERR_BAD_ARG);
        CHECK(swr_morph_pose_set(c, wA, 6, Bp.data(), 9, -1) == SWR_ERR_BAD_ARG);
        CHECK(swr_morph_pose_set(nullptr, wA, 6, Bp.data(), 9, SWR_POSE_MATRICES) == SWR_ERR_BAD_ARG);
        expect_no_launch("refused combined calls");
        if (ntri >= 4) {            // (a restream re-applies what the context holds: still weights B and pose A)
            swr_draw_item items[2] = {{0, 3, {}}, {3, 3 * (int64_t)(ntri - 1), {}}};
            tagm(items[0].transform, 5.0f); tagm(items[1].transform, 6.0f);
            CHECK(swr_draw_list(c, items, 2, SWR_FLAG_DEPTH_TEST) == SWR_OK);
            CHECK(swr_sync(c) == SWR_OK);
            expect_stream(s, &T, wB, A.data(), true, B, "after the refusals the context still holds weights B and pose A");
        }
        // NULL halves mean what they mean in the two calls
        CHECK(swr_morph_pose_set(c, nullptr, 0, Bp.data(), 9, SWR_POSE_MATRICES) == SWR_OK);
        expect_stream(s, nullptr, nullptr, Bp.data(), true, B, "no weights, pose B");
        CHECK(swr_morph_pose_set(c, wA, 6, nullptr, 0, SWR_POSE_MATRICES) == SWR_OK);
        expect_stream(s, &T, wA, nullptr, true, B, "weights A, the bind pose");
        CHECK(swr_morph_pose_set(c, nullptr, 0, nullptr, 0, SWR_POSE_DUAL_QUATS) == SWR_OK);
        expect_stream(s, nullptr, nullptr, nullptr, true, B, "neither: the uploaded stream");
        CHECK(swr_morph_pose_set(c, nullptr, 0, nullptr, 0, SWR_POSE_MATRICES) == SWR_OK);
        expect_no_launch("neither, twice");
        // behind an un-waited frame
        tagm(m, 7.0f); CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
        CHECK(swr_morph_pose_set(c, wB, 6, A.data(), 6, SWR_POSE_MATRICES) == SWR_OK);
        expect_stream(s, &T, wB, A.data(), true, B, "the combined call behind a frame");
        CHECK(swr_read_depth(c, d.data()) == SWR_OK && all_eq(d, 7.0f));
    }
    // dense -> sparse -> dense -> removal on one context: new targets zero the weights and keep the pose
    { const swr_morph_targets t{T2.dp.data(), nullptr, nv, T2.count, 0}; CHECK(swr_scene_morph(c, &t) == SWR_OK); }
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "dense targets: every weight 0, pose A kept");
    CHECK(swr_morph_set(c, wB, 6) == SWR_OK);
    expect_stream(s, &T2, wB, A.data(), true, B, "the dense targets (no normal deltas)");
    { const swr_morph_sparse t = S2.desc(nv); CHECK(swr_scene_morph_sparse(c, &t) == SWR_OK); }
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "sparse targets over dense ones: every weight 0");
    CHECK(swr_morph_set(c, wA, 6) == SWR_OK);
    expect_stream(s, &T2, wA, A.data(), true, B, "sparse targets without normal deltas: the normals stay as uploaded (and are posed)");
    { const swr_morph_targets t{T.dp.data(), T.dn.data(), nv, T.count, 0}; CHECK(swr_scene_morph(c, &t) == SWR_OK); }
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "dense targets over sparse ones");
    {
        const int dense0 = g_morph_launches.load(), sparse0 = g_sparse_launches.load();
        CHECK(swr_morph_set(c, wA, 6) == SWR_OK);
        expect_stream(s, &T, wA, A.data(), true, B, "the dense targets with normal deltas");
        CHECK(g_morph_launches.load() == dense0 + B && g_sparse_launches.load() == sparse0);
    }
    { const swr_morph_sparse t = S.desc(nv); CHECK(swr_scene_morph_sparse(c, &t) == SWR_OK); }
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "sparse targets over active dense ones: every weight 0");
    CHECK(swr_morph_set(c, wB, 6) == SWR_OK);
    expect_stream(s, &T, wB, A.data(), true, B, "sparse again, attributes before the targets");
    CHECK(swr_scene_morph(c, nullptr) == SWR_OK);                   // the dense call's NULL removes sparse targets
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "the targets removed: pose A alone");
    CHECK(swr_morph_set(c, wA, 6) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_pose_set(c, wA, 6, A.data(), 6, SWR_POSE_MATRICES) == SWR_ERR_BAD_ARG);
    { const swr_morph_targets t{T2.dp.data(), nullptr, nv, T2.count, 0}; CHECK(swr_scene_morph(c, &t) == SWR_OK); }
    CHECK(swr_morph_set(c, wA, 6) == SWR_OK);
    (void)take_records();
    CHECK(swr_scene_morph_sparse(c, nullptr) == SWR_OK);            // ... and the sparse call's NULL removes dense ones
    expect_stream(s, nullptr, nullptr, A.data(), true, B, "dense targets removed by the sparse call");
    CHECK(swr_scene_morph_sparse(c, nullptr) == SWR_OK);
    expect_no_launch("removed twice");
    // page-locked sources
    {
        uint32_t* pi = nullptr; float* pd = nullptr;
        CHECK(hipHostMalloc((void**)&pi, S.idx[2].size() * 4, 0) == hipSuccess && hipHostMalloc((void**)&pd, S.dp[2].size() * 4, 0) == hipSuccess);
        memcpy(pi, S.idx[2].data(), S.idx[2].size() * 4); memcpy(pd, S.dp[2].data(), S.dp[2].size() * 4);
        swr_morph_sparse t = S2.desc(nv);
        Sparse Sp = S2;
        Sp.idx[2] = S.idx[2]; Sp.dp[2] = S.dp[2];
        S2.recs[2].indices = pi; S2.recs[2].position_deltas = pd;
        CHECK(swr_scene_morph_sparse(c, &t) == SWR_OK);
        memset(pi, 0xFF, S.idx[2].size() * 4); memset(pd, 0xFF, S.dp[2].size() * 4);
        CHECK(hipHostFree(pi) == hipSuccess && hipHostFree(pd) == hipSuccess);
        const Targets Tp = Sp.dense(nv);
        CHECK(swr_morph_set(c, wB, 6) == SWR_OK);
        expect_stream(s, &Tp, wB, A.data(), true, B, "page-locked arrays");
    }
    // an upload drops everything
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_morph_set(c, wA, 6) == SWR_ERR_BAD_ARG);
    CHECK(swr_morph_pose_set(c, wA, 6, A.data(), 6, SWR_POSE_MATRICES) == SWR_ERR_BAD_ARG);
    expect_no_launch("an upload drops targets and weights");
    // all-empty targets: legal, nothing is ever launched, the stream is the base's
    {
        Sparse E;
        E.idx.resize(3); E.dp.resize(3); E.dn.resize(3);
        const swr_morph_sparse t = E.desc(nv);
        const float w3[3] = {1.0f, NAN, -2.0f};
        const int before_e = g_sparse_launches.load();
        CHECK(swr_scene_morph_sparse(c, &t) == SWR_OK);
        CHECK(swr_morph_set(c, w3, 3) == SWR_OK);
        expect_stream(s, nullptr, nullptr, nullptr, false, B, "all-empty targets");
        CHECK(g_sparse_launches.load() == before_e);
        CHECK(swr_morph_set(c, nullptr, 0) == SWR_OK);
        expect_stream(s, nullptr, nullptr, nullptr, false, B, "all-empty targets, zero weights");
    }
    // the dual-quaternion half of the combined call
    {
        std::vector<float> Q(8 * 6, 0.0f);
        for (int j = 0; j < 6; j++) Q[8 * (size_t)j + 3] = 1.0f;    // identity rotations, no translation
        const swr_morph_sparse t = S2.desc(nv);
        CHECK(swr_scene_morph_sparse(c, &t) == SWR_OK);
        CHECK(swr_scene_skin(c, s.sk.data(), nv) == SWR_OK);
        (void)take_records();
        const int q0 = g_dq_launches.load();
        CHECK(swr_morph_pose_set(c, wA, 6, Q.data(), 6, SWR_POSE_DUAL_QUATS) == SWR_OK);
        CHECK(g_dq_launches.load() == q0 + B);
        CHECK((int)take_records().size() == B);
    }
    swr_context_destroy(c);
}

// 256 targets that each list every vertex: the entries take several staging chunks per table; all active, then only the last
static void many_entries(uint32_t devices, int nv) {
    swr_config cfg{0, devices, 20000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const Scene s = make_scene(nv, 200, 2);
    Sparse S;
    S.nrm = true;
    S.idx.resize(SWR_MORPH_MAX_TARGETS); S.dp.resize(SWR_MORPH_MAX_TARGETS); S.dn.resize(SWR_MORPH_MAX_TARGETS);
    for (int t = 0; t < SWR_MORPH_MAX_TARGETS; t++)
        for (int i = 0; i < nv; i++) {
            if (t % 2 && i % 7 == t % 7) continue;                   // (odd targets leave some vertices out)
            S.idx[t].push_back((uint32_t)i);
            for (int k = 0; k < 3; k++) {
                S.dp[t].push_back(0.001f * (float)((t * 31 + i * 7 + k * 3) % 113) - 0.05f);
                S.dn[t].push_back(0.01f * (float)((t * 13 + i * 5 + k) % 37));
            }
        }
    const Targets T = S.dense(nv);
    CHECK(swr_scene_upload(c, s.v.data(), nv, s.idx.data(), (int64_t)s.idx.size()) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    CHECK(swr_scene_attributes(c, s.a.data(), nv) == SWR_OK);
    { const swr_morph_sparse t = S.desc(nv); CHECK(swr_scene_morph_sparse(c, &t) == SWR_OK); }
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
    Sparse S = make_sparse(300, false, 0.0f);
    const float w[6] = {1.0f, 0.5f, 0, 0, 0, 0};
    const std::vector<float> A = make_pose(6, 0.25f);
    CHECK(swr_scene_upload(c, s.v.data(), 300, s.idx.data(), 300) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    CHECK(swr_scene_skin(c, s.sk.data(), 300) == SWR_OK);
    const swr_morph_sparse t = S.desc(300);
    CHECK(swr_scene_morph_sparse(c, &t) == SWR_OK);
    float m[16];
    tagm(m, 1.0f);
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, SWR_FLAG_DEPTH_TEST);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    (void)take_records();
    CHECK(swr_morph_set(c, w, 6) == SWR_ERR_HIP);
    CHECK(swr_scene_morph_sparse(c, &t) == SWR_ERR_HIP);
    CHECK(swr_scene_morph_sparse(c, nullptr) == SWR_ERR_HIP);
    CHECK(swr_morph_pose_set(c, w, 6, A.data(), 6, SWR_POSE_MATRICES) == SWR_ERR_HIP);
    CHECK(swr_morph_pose_set(c, w, 6, A.data(), 6, 7) == SWR_ERR_HIP);
    expect_no_launch("a failed context");
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    scenario(1, 300, 200);
    scenario(3, 300, 200);
    scenario(1, 3, 1);              // one triangle: one ragged group
    scenario(3, 130, 129);          // 64 * 2 + 1 slots
    many_entries(1, 4200);          // about 1.07 million entries of 16 bytes: three staging chunks per table
    many_entries(3, 700);
    failed_context(1);
    failed_context(2);
    CHECK(g_sparse_launches.load() > 0 && g_sparse_nrm_launches.load() > 0 && g_vertex_launches.load() > 0);
    return report("morph sparse host test");
}
