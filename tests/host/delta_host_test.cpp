// The host side of the delta reads (software-renderer_amd/csrc/swr_api.hip: band_read_delta, the group fan-out and sum,
// swr_read_color_delta / swr_read_depth_delta / swr_delta_reset / swr_render_delta) on the fake HIP runtime of tests/host/hip_stub,
// under the address and undefined-behaviour sanitizers.  The stand-ins of swr::launch_delta and swr::launch_delta_pack
// (stub_launch.cpp) are plain CPU loops over the header's definition run as "kernels" of the fake stream.  The images are patterns written with swr_target_write, so the loops read the band's own rows, and a baseline, a flag table
// or a staging buffer sized too small is an out-of-bounds access the address sanitizer reports.  What is checked is the host side:
// the rectangle and the counts it derives from the flag table, the rows it moves into the caller's image, and what it leaves alone.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Itests/host/hip_stub -x c++ software-renderer_amd/csrc/swr_api.hip \
//       tests/host/hip_stub/stub_runtime.cpp tests/host/hip_stub/stub_launch.cpp tests/host/delta_host_test.cpp -lpthread
#include <algorithm>
#include <string>
#include <vector>

#include "host_test.h"

// (the library stores the changed tiles of a page-locked destination from the compare itself; built with -DSWR_TUNE_DELTA_DIRECT=0 it
// gathers the rectangle and copies it through the stage chunks, as it always does for a pageable destination)
#ifndef SWR_TUNE_DELTA_DIRECT
#define SWR_TUNE_DELTA_DIRECT_TEST 1
#else
#define SWR_TUNE_DELTA_DIRECT_TEST SWR_TUNE_DELTA_DIRECT
#endif

using Image = std::vector<uint32_t>;

// The header's definition: what a delta read with a baseline `prev` of the image `cur` writes into `dst`, and its stats.  direct_pinned:
// a band whose rows start the page-locked destination (the only address the fake runtime knows as page-locked) gets its changed tiles
// alone (the header allows less than R).
static swr_delta_stats model(const Image& prev, const Image& cur, int W, const Bands& b, Image& dst, bool have_base, bool direct_pinned) {
    swr_delta_stats t{};
    for (size_t k = 0; k < b.r0.size(); k++) {
        const int r0 = (int)b.r0[k], r1 = (int)b.r1[k], rows = r1 - r0;
        const bool direct = direct_pinned && r0 == 0;
        const int tx_n = (W + 63) / 64, ty_n = (rows + 31) / 32;
        int bx0 = W, bx1 = 0, by0 = r1, by1 = r0;
        int64_t changed = 0, px = 0;
        std::vector<char> flag((size_t)tx_n * ty_n, 0);
        for (int ty = 0; ty < ty_n; ty++)
            for (int tx = 0; tx < tx_n; tx++) {
                const int x0 = tx * 64, x1 = std::min(W, x0 + 64), y0 = r0 + ty * 32, y1 = std::min(r1, y0 + 32);
                bool diff = !have_base;
                for (int y = y0; y < y1 && !diff; y++)
                    diff = memcmp(&prev[(size_t)y * W + x0], &cur[(size_t)y * W + x0], (size_t)(x1 - x0) * 4) != 0;
                if (!diff) continue;
                flag[(size_t)ty * tx_n + tx] = 1;
                changed++; px += (int64_t)(x1 - x0) * (y1 - y0);
                bx0 = std::min(bx0, x0); bx1 = std::max(bx1, x1); by0 = std::min(by0, y0); by1 = std::max(by1, y1);
            }
        t.tiles += (int64_t)tx_n * ty_n;
        t.tiles_changed += changed;
        if (!changed) continue;
        int64_t bytes = (int64_t)(bx1 - bx0) * (by1 - by0) * 4;
        if (direct && have_base) {
            bytes = px * 4;
            for (int y = by0; y < by1; y++)
                for (int x = bx0; x < bx1; x++)
                    if (flag[(size_t)((y - r0) / 32) * tx_n + x / 64]) dst[(size_t)y * W + x] = cur[(size_t)y * W + x];
        } else {
            for (int y = by0; y < by1; y++) memcpy(&dst[(size_t)y * W + bx0], &cur[(size_t)y * W + bx0], (size_t)(bx1 - bx0) * 4);
        }
        if (!t.bytes_copied) { t.x0 = bx0; t.y0 = by0; t.x1 = bx1; t.y1 = by1; }
        else { t.x0 = std::min(t.x0, bx0); t.y0 = std::min(t.y0, by0); t.x1 = std::max(t.x1, bx1); t.y1 = std::max(t.y1, by1); }
        t.bytes_copied += bytes;
    }
    t.full = have_base ? 0 : (t.tiles ? 1 : 0);
    return t;
}

static bool same(const swr_delta_stats& a, const swr_delta_stats& b) { return memcmp(&a, &b, sizeof a) == 0; }

static uint32_t pattern(int x, int y, uint32_t salt) { return (uint32_t)x * 2654435761u + (uint32_t)y * 40503u + salt * 0x9E3779B9u; }

static Image make(int W, int H, uint32_t salt) {
    Image im((size_t)W * H);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) im[(size_t)y * W + x] = pattern(x, y, salt);
    return im;
}

// a destination: pageable, or page-locked (hipHostMalloc of the fake runtime)
struct Dst {
    uint32_t* p = nullptr;
    size_t n = 0;
    bool pinned = false;
    Dst(size_t words, bool pin) : n(words), pinned(pin) {
        if (pin) { CHECK(hipHostMalloc((void**)&p, words * 4, hipHostMallocDefault) == hipSuccess); }
        else p = new uint32_t[words];
        for (size_t i = 0; i < n; i++) p[i] = 0xA5A5A5A5u;
    }
    ~Dst() { if (pinned) hipHostFree(p); else delete[] p; }
};

struct Reader {
    swr_context* c;
    int img, W, H;
    Bands b;
    Image host;         // what the caller's image must hold
    Image cur;          // the image on the device
    bool have_base = false;
    Dst* dst;
    // write `next` to the device, plant wrong words at `plant` (pixels that must not be written), read, compare with the model
    void step(const Image& next, const std::vector<std::pair<int, int>>& plant = {}) {
        if (img == 0) CHECK(swr_target_write(c, next.data(), nullptr) == SWR_OK);
        else CHECK(swr_target_write(c, nullptr, (const float*)next.data()) == SWR_OK);
        const Image prev = cur;
        cur = next;
        const bool direct = SWR_TUNE_DELTA_DIRECT_TEST && dst->pinned;
        // (only words outside the bounding box of what will be written can be planted)
        Image scratch = host;
        const swr_delta_stats pre = model(prev, cur, W, b, scratch, have_base, direct);
        std::vector<std::pair<int, int>> planted;
        for (auto [x, y] : plant)
            if (!(pre.bytes_copied && x >= pre.x0 && x < pre.x1 && y >= pre.y0 && y < pre.y1) &&
                std::find(planted.begin(), planted.end(), std::make_pair(x, y)) == planted.end()) planted.push_back({x, y});
        for (auto [x, y] : planted) { dst->p[(size_t)y * W + x] ^= 0x00FF00FFu; host[(size_t)y * W + x] ^= 0x00FF00FFu; }
        const swr_delta_stats want = model(prev, cur, W, b, host, have_base, direct);
        swr_delta_stats got;
        memset(&got, 0x7F, sizeof got);
        const int rc = img == 0 ? swr_read_color_delta(c, dst->p, &got) : swr_read_depth_delta(c, (float*)dst->p, &got);
        CHECK(rc == SWR_OK);
        CHECK(same(got, want));
        if (!same(got, want))
            std::printf("  got  [%d,%d)x[%d,%d) tiles %lld changed %lld bytes %lld full %d\n  want [%d,%d)x[%d,%d) tiles %lld changed %lld bytes %lld full %d\n",
                        got.x0, got.x1, got.y0, got.y1, (long long)got.tiles, (long long)got.tiles_changed, (long long)got.bytes_copied, got.full,
                        want.x0, want.x1, want.y0, want.y1, (long long)want.tiles, (long long)want.tiles_changed, (long long)want.bytes_copied, want.full);
        CHECK(memcmp(dst->p, host.data(), host.size() * 4) == 0);
        have_base = true;
        // the planted words are the caller's breach of the promise: mend them, so that the next step starts from a kept promise
        for (auto [x, y] : planted) { dst->p[(size_t)y * W + x] ^= 0x00FF00FFu; host[(size_t)y * W + x] ^= 0x00FF00FFu; }
    }
};

static void poke(Image& im, int W, int x, int y) { im[(size_t)y * W + x] ^= 0x80000000u; }

// one context (or a group) on a target, or on rows [r0, r1) of it
static void scenario(uint32_t devices, int W, int H, int r0, int r1, int img, bool pinned) {
    swr_config cfg{0, devices, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    Dst dst((size_t)W * H, pinned);
    swr_delta_stats keep;
    memset(&keep, 0x7F, sizeof keep);
    const swr_delta_stats untouched = keep;
    CHECK(swr_read_color_delta(c, dst.p, &keep) == SWR_ERR_NO_SCENE);        // before a target
    CHECK(swr_read_depth_delta(c, (float*)dst.p, &keep) == SWR_ERR_NO_SCENE);
    CHECK(same(keep, untouched) && dst.p[0] == 0xA5A5A5A5u);
    CHECK(swr_target_set(c, W, H, r0, r1) == SWR_OK);
    Reader r{c, img, W, H, bands_of(c), Image(dst.p, dst.p + dst.n), make(W, H, 0), false, &dst};
    CHECK((int)r.b.r0.size() == (devices > 1 ? (int)devices : 1));
    const int ya = (int)r.b.r0[0], yb = (int)r.b.r1.back();     // the rows the context owns
    Image im = make(W, H, 1);
    r.step(im);                                     // the first read is full; rows outside the band(s) keep the sentinel
    r.step(im);                                     // nothing changed: nothing copied
    { const int before = g_packs.load(); r.step(im, {{0, ya}, {W - 1, yb - 1}}); CHECK(g_packs.load() == before); }
    poke(im, W, 0, ya); r.step(im, {{std::min(W - 1, 64), ya}, {0, std::min(yb - 1, ya + 32)}});      // the first tile alone
    poke(im, W, W - 1, yb - 1); r.step(im, {{0, ya}});                                              // the last pixel (a ragged tile)
    if (W > 64 && yb - ya > 32) {
        poke(im, W, 63, ya + 31); poke(im, W, 64, ya + 32); r.step(im, {{W - 1, ya}, {0, yb - 1}});   // two tiles across a corner
        poke(im, W, 70, ya + 5); poke(im, W, 70, yb - 1); r.step(im, {{0, ya + 3}, {W - 1, ya + 3}});   // a column of tiles: R is narrower than the band
        poke(im, W, 3, ya + 40); poke(im, W, W - 1, ya + 41); r.step(im, {{5, ya}, {5, yb - 1}});       // a row of tiles: full width, not all rows
    }
    im = make(W, H, 2); r.step(im);                 // every tile changed: the whole band, no gather
    // the other image kind has a baseline of its own: its first read is full, and this one's baseline stays
    {
        Dst other((size_t)W * H, pinned);
        swr_delta_stats st{};
        CHECK((img == 0 ? swr_read_depth_delta(c, (float*)other.p, &st) : swr_read_color_delta(c, other.p, &st)) == SWR_OK);
        CHECK(st.full == 1 && st.tiles_changed == st.tiles);
        CHECK((img == 0 ? swr_read_depth_delta(c, (float*)other.p, &st) : swr_read_color_delta(c, other.p, &st)) == SWR_OK);
        CHECK(st.full == 0 && st.tiles_changed == 0 && st.bytes_copied == 0);
        r.step(im);
    }
    // what keeps a baseline: the same target again, the other reads; what drops it: a reset of this kind, another target
    CHECK(swr_target_set(c, W, H, r0, r1) == SWR_OK);
    { Image full((size_t)W * H); CHECK(swr_read_color(c, full.data()) == SWR_OK); CHECK(swr_read_depth(c, (float*)full.data()) == SWR_OK); }
    poke(im, W, W / 2, ya + (yb - ya) / 2); r.step(im);
    CHECK(swr_delta_reset(c, img == 0 ? SWR_DELTA_DEPTH : SWR_DELTA_COLOR) == SWR_OK);      // (the other kind's)
    r.step(im);
    CHECK(swr_delta_reset(c, img == 0 ? SWR_DELTA_COLOR : SWR_DELTA_DEPTH) == SWR_OK);
    r.have_base = false; r.step(im);
    CHECK(swr_delta_reset(c, SWR_DELTA_COLOR | SWR_DELTA_DEPTH) == SWR_OK);
    r.have_base = false; r.step(im);
    // every refusal; nothing is written
    {
        const Image before(dst.p, dst.p + dst.n);
        CHECK(swr_read_color_delta(nullptr, dst.p, &keep) == SWR_ERR_BAD_ARG);
        CHECK(swr_read_depth_delta(nullptr, (float*)dst.p, &keep) == SWR_ERR_BAD_ARG);
        CHECK(swr_read_color_delta(c, nullptr, &keep) == SWR_ERR_BAD_ARG);
        CHECK(swr_read_depth_delta(c, nullptr, &keep) == SWR_ERR_BAD_ARG);
        CHECK(swr_delta_reset(nullptr, SWR_DELTA_COLOR) == SWR_ERR_BAD_ARG);
        CHECK(swr_delta_reset(c, 0) == SWR_ERR_BAD_ARG);
        CHECK(swr_delta_reset(c, 4) == SWR_ERR_BAD_ARG);
        CHECK(swr_delta_reset(c, SWR_DELTA_COLOR | 8u) == SWR_ERR_BAD_ARG);
        swr_render_pass p{};
        p.color = dst.p; p.depth = (float*)dst.p; p.width = W; p.height = H; p.flags = SWR_FLAG_LOAD;
        swr_delta_stats two[2];
        memset(two, 0x7F, sizeof two);
        CHECK(swr_render_delta(c, &p, two) == SWR_ERR_UNSUPPORTED);
        CHECK(swr_render_delta(nullptr, &p, two) == SWR_ERR_BAD_ARG && swr_render_delta(c, nullptr, two) == SWR_ERR_BAD_ARG);
        CHECK(same(two[0], untouched) && same(two[1], untouched));
        CHECK(same(keep, untouched) && memcmp(dst.p, before.data(), dst.n * 4) == 0);
        r.step(im);             // (and the baseline is still there: nothing changed)
        CHECK((img == 0 ? swr_read_color_delta(c, dst.p, nullptr) : swr_read_depth_delta(c, (float*)dst.p, nullptr)) == SWR_OK);   // stats may be NULL
    }
    // another target drops the baselines; the table and the baseline grow with it
    if (r0 == 0 && r1 == H) {
        const int W2 = W + 70, H2 = H + 40;
        CHECK(swr_target_set(c, W2, H2, 0, H2) == SWR_OK);
        Dst d2((size_t)W2 * H2, pinned);
        Reader r2{c, img, W2, H2, bands_of(c), Image(d2.p, d2.p + d2.n), make(W2, H2, 0), false, &d2};
        Image im2 = make(W2, H2, 5);
        r2.step(im2);
        poke(im2, W2, W2 - 1, 0); r2.step(im2);
        CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);      // back: dropped again
        r.have_base = false; r.b = bands_of(c); r.step(im);
    }
    swr_context_destroy(c);
}

// a changed rectangle larger than a stage chunk (8 MiB): the chunk border falls inside a row
static void large_rectangle(bool pinned) {
    swr_config cfg{0, 1, 5000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    const int W = 2200, H = 1100;
    CHECK(swr_target_set(c, W, H, 0, H) == SWR_OK);
    Dst dst((size_t)W * H, pinned);
    Reader r{c, 0, W, H, bands_of(c), Image(dst.p, dst.p + dst.n), make(W, H, 0), false, &dst};
    Image im = make(W, H, 1);
    r.step(im);
    poke(im, W, 100, 100); r.step(im);              // a small gather first: the staging grows with the next one
    Image next = make(W, H, 2);
    for (int y = 0; y < H; y++)
        for (int x = 2176; x < W; x++) next[(size_t)y * W + x] = im[(size_t)y * W + x];     // all but the last column of tiles
    const int before = g_packs.load();
    r.step(next, {{2176, 0}, {W - 1, H - 1}});
    CHECK(SWR_TUNE_DELTA_DIRECT_TEST && pinned ? g_packs.load() == before : g_packs.load() == before + 1);
    swr_context_destroy(c);
}

// a failed context returns its sticky error
static void failed_context(uint32_t devices) {
    swr_config cfg{0, devices, 2000, 0};
    swr_context* c = nullptr;
    CHECK(swr_context_create(&cfg, &c) == SWR_OK);
    std::vector<swr_vertex> verts(300);
    std::vector<int64_t> idx(300);
    for (size_t i = 0; i < idx.size(); i++) idx[i] = (int64_t)i;
    CHECK(swr_scene_upload(c, verts.data(), 300, idx.data(), 300) == SWR_OK);
    CHECK(swr_target_set(c, 64, 64, 0, 64) == SWR_OK);
    float m[16];
    for (int k = 0; k < 16; k++) m[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    CHECK(swr_draw(c, m, SWR_FLAG_DEPTH_TEST) == SWR_OK);
    Image dst(64 * 64, 0xA5A5A5A5u);
    swr_delta_stats st;
    CHECK(swr_read_depth_delta(c, (float*)dst.data(), &st) == SWR_OK && st.full == 1);      // (the delta read is the call that waits)
    CHECK(swr_debug_fault(c, SWR_FAULT_ENQUEUE) == SWR_OK);
    swr_draw(c, m, SWR_FLAG_DEPTH_TEST);
    CHECK(swr_sync(c) == SWR_ERR_HIP);
    const Image before = dst;
    memset(&st, 0x7F, sizeof st);
    const swr_delta_stats untouched = st;
    CHECK(swr_read_depth_delta(c, (float*)dst.data(), &st) == SWR_ERR_HIP);
    CHECK(swr_read_color_delta(c, dst.data(), &st) == SWR_ERR_HIP);
    CHECK(swr_delta_reset(c, SWR_DELTA_COLOR) == SWR_ERR_HIP);
    CHECK(same(st, untouched) && dst == before);
    swr_context_destroy(c);
}

int main() {
    fake_kernel_delay_us(0);
    for (int img = 0; img < 2; img++)
        for (int pinned = 0; pinned < 2; pinned++) {
            scenario(1, 200, 100, 0, 100, img, pinned != 0);
            scenario(3, 200, 200, 0, 200, img, pinned != 0);
        }
    scenario(1, 130, 70, 0, 70, 0, false);
    scenario(1, 64, 32, 0, 32, 1, true);
    scenario(1, 1, 1, 0, 1, 0, false);
    scenario(1, 192, 128, 32, 96, 0, false);         // a context that owns one band of a larger target
    scenario(1, 192, 128, 32, 96, 1, true);
    large_rectangle(false);
    large_rectangle(true);
    failed_context(1);
    failed_context(2);
    CHECK(g_compares.load() > 0 && g_packs.load() > 0);
    CHECK(SWR_TUNE_DELTA_DIRECT_TEST ? g_directs.load() > 0 : g_directs.load() == 0);
    return report("delta host test");
}
