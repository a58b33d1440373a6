// What the host test programs see of the stand-in launch set (stub_launch.cpp): the knobs they turn, how often each feature launch
// ran, what the last skin stream launches wrote, the failures a stand-in found on the fake stream's thread, and the arithmetic the
// stand-ins share with the programs' models.  Test infrastructure only.
#pragma once
#include <atomic>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../../include/swr.h"
#include <hip/hip_runtime.h>

namespace swr {
extern std::atomic<uint32_t> g_fake_fill;        // largest tile fill the fake k_bin reports (tests raise it to force a regrow)
extern std::atomic<uint32_t> g_fake_pairs;
extern std::atomic<uint32_t> g_fake_clip_over;   // != 0: the next clip frame's raster reports this many triangles beyond its slots, once
}
// primitives of the frame being counted: the fake ID image is ids[y][x] + count_pattern(x, y, g_count_total)
extern std::atomic<uint32_t> g_count_total;

// launches so far
extern std::atomic<int> g_count_launches, g_query_launches;
extern std::atomic<int> g_compares, g_directs, g_packs;                     // launch_delta, those with a direct destination, launch_delta_pack
extern std::atomic<int> g_vertex_launches, g_stream_launches;               // launch_skin_vertices, launch_skin_stream
extern std::atomic<int> g_morph_launches, g_morph_nrm_launches;             // launch_morph_vertices, those with normals
// what a stand-in found wrong in what it was handed (it runs on the fake stream's thread): a program adds this to its failures
extern std::atomic<int> g_launch_fails;

// what a stream launch wrote; take_records: the launches since the last call, the list cleared
struct Record { const float4* tri_xyz; const float4* tri_nrm; const float4* box; int64_t ntri; bool nrm; };
std::vector<Record> take_records();

// the ID the pattern gives band-local pixel (x, y): 0 .. total - 1, or SWR_ID_NONE
inline uint32_t count_pattern(uint32_t x, uint32_t y, uint32_t total) {
    const uint32_t v = (x * 7u + y * 13u + (x >> 3) * (y >> 2)) % (total + 1u);
    return v == total ? SWR_ID_NONE : v;
}

// "Supersampled resolve": the rounded mean of S x S colour samples per channel, the nearest of S x S depths
inline uint32_t resolve_box(const uint32_t* src, size_t pitch, int S) {
    uint32_t out = 0;
    for (int ch = 0; ch < 4; ch++) {
        uint32_t sum = 0;
        for (int j = 0; j < S; j++) for (int i = 0; i < S; i++) sum += (src[j * pitch + i] >> (8 * ch)) & 0xFFu;
        out |= ((sum + S * S / 2) / (S * S)) << (8 * ch);
    }
    return out;
}
inline float resolve_minimum(const float* src, size_t pitch, int S) {
    float m = src[0];
    for (int j = 0; j < S; j++) for (int i = 0; i < S; i++) { const float s = src[j * pitch + i]; if (s < m || (m != m && s == s)) m = s; }
    return m;
}

// "Skinned meshes", for one vector: translate = the c3 term (positions), else not (normals)
inline void blend(const float* v, const swr_skin_vertex& sk, const float* joints, bool translate, float* out) {
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
