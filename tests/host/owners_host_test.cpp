// What a context owns goes with it (software-renderer_amd/csrc/swr_api.hip: DevBuf, HostBuf, Pinned, Event, Stream, the workers, and
// destroy_single, which frees nothing by hand), on the fake HIP runtime of tests/host/hip_stub under the address, undefined-behaviour
// and leak sanitizers.  The fake hipMalloc, hipHostMalloc, streams and events are heap objects, so an owner that is missing, or one
// whose destructor does nothing, is a leak the sanitizer reports at exit.  The program touches everything a context allocates lazily
// — once per kind of context — and destroys it; it asserts only that every call succeeds.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/owners_host_test.cpp -lpthread
#include <vector>

#include "host_test.h"

static const int NV = 30, NTRI = 12, W = 64;

static void persp(float* m, float tag) {    // w = 0.5 + z: not affine, the scene's z in [0.1, 0.2] stays in front
    tagm(m, tag);
    m[11] = 1.0f; m[15] = 0.5f;
}

static void everything(uint32_t devices, int H) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const Scene s = make_scene(NV, NTRI, 2);
    float m[16], pm[16];
    tagm(m, 2.0f); persp(pm, 3.0f);
    const uint32_t Z = SWR_FLAG_DEPTH_TEST;
    CHECK(swr_scene_upload(c, s.v.data(), NV, s.idx.data(), 3 * NTRI) == SWR_OK);
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    // attributes, a texture and the material that reads them
    CHECK(swr_scene_attributes(c, s.a.data(), NV) == SWR_OK);
    const std::vector<uint32_t> texels(8 * 4, 0xFF336699u);
    CHECK(swr_texture_upload(c, texels.data(), 8, 4) == SWR_OK);
    swr_material mat{};
    mat.shader = SWR_SHADER_TEXTURED_PHONG; mat.shininess_log2 = 3; mat.light_dir[2] = 1.0f; mat.half_dir[2] = 1.0f; mat.diffuse = 1.0f;
    CHECK(swr_material_set(c, &mat) == SWR_OK);
    CHECK(swr_draw(c, m, Z) == SWR_OK);
    // skin, a pose of matrices and one of dual quaternions
    CHECK(swr_scene_skin(c, s.sk.data(), NV) == SWR_OK);
    const std::vector<float> pose = make_pose(3, 0.02f);
    CHECK(swr_pose_set(c, pose.data(), 3) == SWR_OK);
    std::vector<float> dq(8 * 3, 0.0f);
    for (int j = 0; j < 3; j++) dq[8 * (size_t)j + 3] = 1.0f;
    CHECK(swr_pose_set_dq(c, dq.data(), 3) == SWR_OK);
    // morph targets with normals, uploaded twice (the second set replaces the first), in effect, then dropped
    {
        const std::vector<float> dp(2 * (size_t)NV * 3, 0.001f), dn(2 * (size_t)NV * 3, 0.01f);
        const swr_morph_targets t{dp.data(), dn.data(), NV, 2, 0};
        const float w[2] = {0.5f, 0.25f};
        CHECK(swr_scene_morph(c, &t) == SWR_OK);
        CHECK(swr_morph_set(c, w, 2) == SWR_OK);
        CHECK(swr_scene_morph(c, &t) == SWR_OK);
        CHECK(swr_morph_set(c, w, 2) == SWR_OK);
        CHECK(swr_draw(c, m, Z) == SWR_OK);
        CHECK(swr_scene_morph(c, nullptr) == SWR_OK);
    }
    // a draw list that cuts the stream: a colour frame with the material (the frame's own per-slot tables), perspective, clipped, IDs
    swr_draw_item items[2] = {};
    items[0].first_index = 3 * 5; items[0].index_count = 3 * 4; tagm(items[0].transform, 4.0f);
    items[1].first_index = 3 * 1; items[1].index_count = 3 * 3; persp(items[1].transform, 5.0f);
    CHECK(swr_draw_list(c, items, 2, Z) == SWR_OK);
    CHECK(swr_draw_list(c, items, 2, Z | SWR_FLAG_PERSPECTIVE) == SWR_OK);
    CHECK(swr_draw_list(c, items, 2, Z | SWR_FLAG_DEPTH_CLIP) == SWR_OK);
    CHECK(swr_draw_list(c, items, 2, Z | SWR_FLAG_PRIMITIVE_IDS) == SWR_OK);
    // a clip frame and a perspective frame of the scene
    CHECK(swr_draw(c, m, Z | SWR_FLAG_DEPTH_CLIP) == SWR_OK);
    CHECK(swr_draw(c, pm, Z | SWR_FLAG_PERSPECTIVE) == SWR_OK);
    CHECK(swr_sync(c) == SWR_OK);
    // a resolved read
    {
        std::vector<uint32_t> col((size_t)(W / 2) * (H / 2));
        std::vector<float> dep(col.size());
        const swr_resolve rs{2, SWR_RESOLVE_DEPTH_MIN, {0, 0}};
        CHECK(swr_read_color_resolved(c, &rs, col.data()) == SWR_OK);
        CHECK(swr_read_depth_resolved(c, &rs, dep.data()) == SWR_OK);
    }
    // an ID frame; a count, a depth query and item bounds
    {
        CHECK(swr_draw(c, m, Z | SWR_FLAG_PRIMITIVE_IDS) == SWR_OK);
        g_count_total = NTRI;
        const swr_id_count q{SWR_COUNT_PER_PRIMITIVE, 0, 0, W, H, {0, 0, 0}};
        std::vector<uint32_t> counts(NTRI);
        uint32_t none = 0;
        CHECK(swr_count_ids(c, &q, counts.data(), NTRI, &none) == SWR_OK);
        std::vector<uint32_t> ids((size_t)W * H);
        CHECK(swr_read_ids(c, ids.data()) == SWR_OK);
        const swr_depth_box box{1, 1, W - 1, H - 1, 0.5f, {0, 0, 0}};
        uint32_t passed = 0;
        CHECK(swr_query_depth(c, &box, 1, &passed) == SWR_OK);
        swr_item_bound rec[2];
        CHECK(swr_item_bounds(c, items, 2, 0, rec) == SWR_OK);
    }
    // both delta reads into a pageable image: the whole band through the stage chunks, then a changed frame, then an unchanged one
    {
        std::vector<uint32_t> col((size_t)W * H);
        std::vector<float> dep(col.size());
        for (float tag : {6.0f, 7.0f, 7.0f}) {
            float t[16];
            tagm(t, tag);
            CHECK(swr_draw(c, t, Z) == SWR_OK);
            swr_delta_stats st;
            CHECK(swr_read_color_delta(c, col.data(), &st) == SWR_OK);
            CHECK(swr_read_depth_delta(c, dep.data(), &st) == SWR_OK);
        }
        CHECK(swr_read_color(c, col.data()) == SWR_OK);
        CHECK(swr_target_write(c, col.data(), dep.data()) == SWR_OK);
    }
    // timing level 2, and the frame presented into pageable images
    {
        CHECK(swr_timing_enable(c, 2) == SWR_OK);
        CHECK(swr_draw(c, m, Z) == SWR_OK);
        std::vector<uint32_t> col((size_t)W * H);
        std::vector<float> dep(col.size());
        CHECK(swr_present(c, col.data(), dep.data()) == SWR_OK);
        CHECK(swr_present_wait(c) == SWR_OK);
        swr_timings t;
        int64_t frames = 0;
        CHECK(swr_get_timings(c, &t) == SWR_OK);
        CHECK(swr_timing_totals(c, &t, &frames) == SWR_OK);
        CHECK(swr_timing_enable(c, 0) == SWR_OK);
    }
    // swr_render: a scene for one frame (a new upload, built behind the copy of its index array), then a resident one
    {
        std::vector<uint32_t> col((size_t)W * H);
        std::vector<float> dep(col.size());
        swr_render_pass p{};
        p.color = col.data(); p.depth = dep.data(); p.width = W; p.height = H;
        p.vertices = s.v.data(); p.vertex_count = NV; p.indices = s.idx.data(); p.index_count = 3 * NTRI;
        p.primitive_type = SWR_PRIMITIVE_TRIANGLE; p.flags = Z;
        tagm(p.transform, 8.0f);
        p.attributes = s.a.data(); p.material = &mat; p.texture = texels.data(); p.tex_width = 8; p.tex_height = 4;
        CHECK(swr_debug_set(c, SWR_DEBUG_ONESHOT_MIN_TRIS, 0) == SWR_OK);
        CHECK(swr_render(c, &p) == SWR_OK);
        p.scene_id = 7;
        CHECK(swr_render(c, &p) == SWR_OK);
        CHECK(swr_render(c, &p) == SWR_OK);
    }
    swr_context_destroy(c);
}

// a context nobody used
static void untouched(uint32_t devices) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    untouched(1);
    untouched(3);
    everything(1, 32);
    everything(3, 32);      // (one tile row: the last band has it, the others are empty)
    everything(3, 96);
    return report("owners host test");
}
