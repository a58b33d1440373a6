// The host side of the supersampled resolve (software-renderer_amd/csrc/swr_api.hip: band_read_resolved, the generalised
// copy_band, the group fan-out, swr_render_resolved) on the fake HIP runtime of tests/host/hip_stub, under the address and
// undefined-behaviour sanitizers.  The stand-in of swr::launch_resolve (stub_launch.cpp) is a plain CPU loop over the header's
// formulas run as a "kernel" of the fake stream.  What is checked is the host layer's
// arithmetic: buffer sizes, band offsets, row pitch, destination rows, the pinned path and the staged path across an 8 MiB chunk.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/resolve_host_test.cpp -lpthread
#include <cstring>
#include <vector>

#include "host_test.h"

static void fill(std::vector<uint32_t>& c, std::vector<float>& d, uint32_t seed) {
    uint32_t x = seed;
    for (size_t i = 0; i < c.size(); i++) {
        x = x * 1664525u + 1013904223u;
        c[i] = x;
        d[i] = (float)((x >> 8) & 0xFFFF) / 65536.0f - (float)(i % 7);
    }
}

// one target: write it, read it resolved into pageable and page-locked destinations, compare with the loops above
static void scenario(uint32_t devices, int W, int H, int r0, int r1, int S, uint32_t seed) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    CHECK(swr_target_set(c, W, H, r0, r1) == SWR_OK);
    std::vector<uint32_t> col((size_t)W * H);
    std::vector<float> dep((size_t)W * H);
    fill(col, dep, seed);
    CHECK(swr_target_write(c, col.data(), dep.data()) == SWR_OK);
    const int w = W / S, h = H / S;
    const size_t n = (size_t)w * h;
    std::vector<uint32_t> want_c(n, 0xA5A5A5A5u), got_c(n, 0xA5A5A5A5u);
    std::vector<float> want_d(n, -77.0f), got_d(n, -77.0f);
    for (int y = r0 / S; y < r1 / S; y++)
        for (int x = 0; x < w; x++) {
            const size_t at = (size_t)y * S * W + (size_t)x * S;
            want_c[(size_t)y * w + x] = S == 1 ? col[at] : resolve_box(col.data() + at, W, S);
            want_d[(size_t)y * w + x] = S == 1 ? dep[at] : resolve_minimum(dep.data() + at, W, S);
        }
    swr_resolve rs{S, SWR_RESOLVE_DEPTH_MIN, {0, 0}};
    CHECK(swr_read_color_resolved(c, &rs, got_c.data()) == SWR_OK);
    CHECK(swr_read_depth_resolved(c, &rs, got_d.data()) == SWR_OK);
    CHECK(memcmp(got_c.data(), want_c.data(), n * 4) == 0);
    CHECK(memcmp(got_d.data(), want_d.data(), n * 4) == 0);
    uint32_t* pc = (uint32_t*)swr_host_alloc(n * 4);
    float* pd = (float*)swr_host_alloc(n * 4);
    for (size_t i = 0; i < n; i++) { pc[i] = 0xA5A5A5A5u; pd[i] = -77.0f; }
    CHECK(swr_read_color_resolved(c, &rs, pc) == SWR_OK);
    CHECK(swr_read_depth_resolved(c, &rs, pd) == SWR_OK);
    CHECK(memcmp(pc, want_c.data(), n * 4) == 0);
    CHECK(memcmp(pd, want_d.data(), n * 4) == 0);
    // the full-size images are untouched
    std::vector<uint32_t> back((size_t)W * H);
    CHECK(swr_read_color(c, back.data()) == SWR_OK);
    CHECK(memcmp(back.data() + (size_t)r0 * W, col.data() + (size_t)r0 * W, (size_t)(r1 - r0) * W * 4) == 0);
    // what is refused is refused before anything is touched
    swr_resolve bad{3, 0, {0, 0}};
    CHECK(swr_read_color_resolved(c, &bad, pc) == SWR_ERR_BAD_ARG);
    bad = swr_resolve{2, 0, {0, 1}};
    CHECK(swr_read_depth_resolved(c, &bad, pd) == SWR_ERR_BAD_ARG);
    CHECK(memcmp(pc, want_c.data(), n * 4) == 0);
    swr_host_free(pc);
    swr_host_free(pd);
    swr_context_destroy(c);
}

static void render_resolved(uint32_t devices) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    std::vector<swr_vertex> verts(300);
    std::vector<int64_t> idx(300);
    for (int i = 0; i < 300; i++) idx[i] = i;
    const int w = 48, h = 40;
    std::vector<uint32_t> col((size_t)w * h, 1u);
    std::vector<float> dep((size_t)w * h, -5.0f);
    swr_render_pass p{};
    p.color = col.data(); p.depth = dep.data(); p.width = w; p.height = h;
    p.vertices = verts.data(); p.vertex_count = 300; p.indices = idx.data(); p.index_count = 300;
    p.flags = SWR_FLAG_DEPTH_TEST;
    p.transform[0] = 9.0f; p.transform[5] = p.transform[10] = p.transform[15] = 1.0f;     // the stand-in raster tags every pixel with it
    swr_resolve rs{4, SWR_RESOLVE_DEPTH_MIN, {0, 0}};
    CHECK(swr_render_resolved(c, &p, &rs) == SWR_OK);
    bool ok = true;
    for (float v : dep) ok = ok && v == 9.0f;
    for (uint32_t v : col) ok = ok && v == 0x09090909u;
    CHECK(ok);
    swr_render_times t{};
    CHECK(swr_render_timings(c, &t) == SWR_OK && t.frames == 1);
    p.flags = SWR_FLAG_DEPTH_TEST | SWR_FLAG_LOAD;
    CHECK(swr_render_resolved(c, &p, &rs) == SWR_ERR_UNSUPPORTED);
    p.flags = SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR;
    p.color = nullptr;
    p.transform[0] = 4.0f;
    CHECK(swr_render_resolved(c, &p, &rs) == SWR_OK);
    ok = true;
    for (float v : dep) ok = ok && v == 4.0f;
    CHECK(ok);
    // swr_render afterwards, at its own size
    p.color = col.data(); p.flags = SWR_FLAG_DEPTH_TEST; p.transform[0] = 6.0f;
    CHECK(swr_render(c, &p) == SWR_OK);
    ok = true;
    for (float v : dep) ok = ok && v == 6.0f;
    CHECK(ok);
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    scenario(1, 4, 4, 0, 4, 4, 1);
    scenario(1, 72, 36, 0, 36, 2, 2);
    scenario(1, 200, 100, 0, 100, 4, 3);
    scenario(1, 200, 100, 0, 100, 1, 4);
    scenario(1, 80, 160, 32, 64, 2, 5);          // one band of a larger target: the other rows keep the sentinel
    scenario(1, 80, 160, 32, 64, 4, 6);
    scenario(2, 80, 200, 0, 200, 2, 7);          // bands whose last one ends inside a tile row
    scenario(3, 160, 400, 0, 400, 4, 8);
    scenario(1, 4096, 2560, 0, 2560, 2, 9);      // the resolved image is 10 MiB: the staged path crosses one 8 MiB chunk
    render_resolved(1);
    render_resolved(2);
    return report("resolve host test");
}
