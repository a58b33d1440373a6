// What the host test programs see of the stand-in launch set (stub_launch.cpp): the knobs they turn, how often each feature launch
// ran, what the last skin stream launches wrote, what the normals and ray launches noted about their arguments and their order, the
// failures a stand-in found on the fake stream's thread, and the arithmetic the stand-ins share with the programs' models.  Test
// infrastructure only.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../../software-renderer_amd/csrc/swr_internal.h"

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
extern std::atomic<int> g_bounds_launches;                                  // launch_item_bounds
extern std::atomic<int> g_dq_launches, g_dq_nrm_launches;                   // launch_skin_vertices_dq, those with normals
extern std::atomic<int> g_sparse_launches, g_sparse_nrm_launches;           // launch_morph_sparse, those with normals
extern std::atomic<int64_t> g_sparse_rows;                                  // touched vertices of the last launch_morph_sparse
extern std::atomic<int> g_face_launches, g_vnrm_launches, g_flat_launches;  // launch_face_normals, launch_vertex_normals, launch_flat_normals
extern std::atomic<int> g_flip_launches;                                    // face and flat launches with flip
extern std::atomic<int> g_ray_launches;                                     // launch_cast_rays
// what a stand-in found wrong in what it was handed (it runs on the fake stream's thread): a program adds this to its failures
extern std::atomic<int> g_launch_fails;

// what a stream launch wrote; take_records: the launches since the last call, the list cleared
struct Record { const float4* tri_xyz; const float4* tri_nrm; const float4* box; int64_t ntri; bool nrm; };
std::vector<Record> take_records();

// the stream write, either skin, either morph: launches so far
struct LaunchCounts { int stream, skin, morph; };
inline LaunchCounts launch_counts() {
    return LaunchCounts{g_stream_launches.load(), g_vertex_launches.load() + g_dq_launches.load(), g_morph_launches.load() + g_sparse_launches.load()};
}
// what the normals and ray launches note, under g_note_m
extern std::mutex g_note_m;
extern LaunchCounts g_face_at, g_flat_at;            // what had been launched when the last face / flat launch was made
extern int g_vnrm_after_faces;                       // face launches made when the last vertex-normal launch was made
struct FlatNote { const float4* tri_xyz; const float4* tri_nrm; };
extern std::vector<FlatNote> g_flat_notes;           // the flat launches since the last look
extern std::vector<uint32_t> g_adj_off, g_adj_tri;   // the adjacency the last vertex-normal launch was handed
struct RayNote {
    swr::RaysArgs a;
    int streams_before;         // stream launches made when the ray launch was made
    bool ran;
};
std::vector<RayNote> take_ray_notes();               // the ray launches since the last call, the list cleared

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

// "Dual-quaternion skinning", for one vertex: every operation its own float operation
inline void cross(const float* a, const float* b, float* r) {
    const float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
    r[0] = x; r[1] = y; r[2] = z;
}
inline void blend_dq(const swr_skin_vertex& sk, const float* dq, float* C) {
    const float* Q[4];
    for (int k = 0; k < 4; k++) Q[k] = dq + 8 * (size_t)sk.joint[k];
    float u[4] = {sk.weight[0], 0, 0, 0};
    for (int k = 1; k < 4; k++) {
        float s = Q[0][0] * Q[k][0] + Q[0][1] * Q[k][1];
        s = s + Q[0][2] * Q[k][2];
        s = s + Q[0][3] * Q[k][3];
        u[k] = s < 0.0f ? -sk.weight[k] : sk.weight[k];
    }
    float B[8];
    for (int c = 0; c < 8; c++) {
        float b = u[0] * Q[0][c];
        for (int k = 1; k < 4; k++) { const float p = u[k] * Q[k][c]; b = b + p; }
        B[c] = b;
    }
    float n = B[0] * B[0] + B[1] * B[1];
    n = n + B[2] * B[2];
    n = n + B[3] * B[3];
    const float l = sqrtf(n), i = 1.0f / l;
    for (int c = 0; c < 8; c++) C[c] = B[c] * i;
}
inline void rotate(const float* C, const float* x, float* out) {
    float a[3], b[3], c[3];
    cross(C, x, a);
    for (int j = 0; j < 3; j++) { const float p = C[3] * x[j]; b[j] = a[j] + p; }
    cross(C, b, c);
    for (int j = 0; j < 3; j++) { const float p = 2.0f * c[j]; out[j] = x[j] + p; }
}
inline void pose_dq(const float* v, const swr_skin_vertex& sk, const float* dq, bool translate, float* out) {
    float C[8], r[3], e[3];
    blend_dq(sk, dq, C);
    rotate(C, v, r);
    if (translate) {
        cross(C, C + 4, e);
        for (int j = 0; j < 3; j++) {
            const float wd = C[3] * C[4 + j], dq_ = C[7] * C[j];
            float t = wd - dq_;
            t = t + e[j];
            t = 2.0f * t;
            r[j] = r[j] + t;
        }
    }
    memcpy(out, r, sizeof r);
}

// "Computed normals": the face normal of a triangle, and the normalisation of a vertex normal
inline void face_of(const float* a, const float* b, const float* c, bool flip, float* f) {
    float e1[3], e2[3];
    for (int j = 0; j < 3; j++) { e1[j] = b[j] - a[j]; e2[j] = c[j] - a[j]; }
    if (flip) cross(e2, e1, f); else cross(e1, e2, f);
}
inline void normalise(float* n) {
    float q = n[0] * n[0] + n[1] * n[1];
    q = q + n[2] * n[2];
    const float l = sqrtf(q);
    if (l > 0.0f) { const float r = 1.0f / l; for (int j = 0; j < 3; j++) n[j] = n[j] * r; }
}

// what the ray stand-in answers for ray k: a function of the ray and of the scene's size
inline uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline swr_ray_hit ray_echo(const swr_ray& r, int64_t k, int64_t ntri) {
    return swr_ray_hit{(uint32_t)k ^ float_bits(r.origin[0]), r.tmin + r.dir[2], r.origin[1], (float)ntri + r.tmax};
}

// include/swr.h "Item bounds" over `count` triangles whose corner j of triangle t is corner(t, j) (three floats)
template <class Corner>
inline swr_item_bound fold(int64_t count, Corner corner, const float* m, int W, int H, bool metal) {
    swr_item_bound b{};
    b.zmin = INFINITY; b.zmax = -INFINITY;
    int64_t minx = INT64_MAX, miny = INT64_MAX, maxx = INT64_MIN, maxy = INT64_MIN;
    for (int64_t t = 0; t < count; t++) {
        float sx[3], sy[3], sz[3];
        bool ok = true, w_ok = true;
        for (int j = 0; j < 3; j++) {
            const float* p = corner(t, j);
            float r[4];
            for (int i = 0; i < 4; i++) { r[i] = m[i] * p[0]; r[i] = r[i] + m[4 + i] * p[1]; r[i] = r[i] + m[8 + i] * p[2]; r[i] = r[i] + m[12 + i] * 1.0f; }
            const float nx = r[0] / r[3], ny = r[1] / r[3];
            sx[j] = (nx * 0.5f + 0.5f) * (float)W; sy[j] = (ny * -0.5f + 0.5f) * (float)H; sz[j] = r[2] / r[3];
            if (metal) { sx[j] = roundf(sx[j]); sy[j] = roundf(sy[j]); }
            ok = ok && std::fabs(sx[j]) < 1073741824.0f && std::fabs(sy[j]) < 1073741824.0f && (!metal || (sx[j] >= 0.0f && sy[j] >= 0.0f));
            w_ok = w_ok && r[3] > 0.0f;
        }
        if (!ok) { b.skipped++; continue; }
        b.drawable++;
        if (!w_ok) b.behind++;
        for (int j = 0; j < 3; j++) {
            minx = std::min<int64_t>(minx, (int)sx[j]); maxx = std::max<int64_t>(maxx, (int)sx[j]);
            miny = std::min<int64_t>(miny, (int)sy[j]); maxy = std::max<int64_t>(maxy, (int)sy[j]);
            b.zmin = sz[j] < b.zmin ? sz[j] : b.zmin; b.zmax = sz[j] > b.zmax ? sz[j] : b.zmax;
        }
    }
    if (b.drawable) {
        b.x0 = (int32_t)std::clamp<int64_t>(minx, 0, W); b.x1 = (int32_t)std::clamp<int64_t>(maxx + 1, 0, W);
        b.y0 = (int32_t)std::clamp<int64_t>(miny, 0, H); b.y1 = (int32_t)std::clamp<int64_t>(maxy + 1, 0, H);
    }
    b.zmin = b.zmin + 0.0f; b.zmax = b.zmax + 0.0f;
    return b;
}
