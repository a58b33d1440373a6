// What the host test programs of this directory share: CHECK and the failure count, the program's verdict, and the helpers more than
// one of them uses.  The stand-in launches they all link, and what a program can observe of them, are in hip_stub/stub_launch.h.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/swr.h"
#include <hip/hip_runtime.h>
#include "hip_stub/stub_launch.h"

inline int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

// the last line of a program and its exit code; what the stand-ins found on the fake stream's thread counts too
inline int report(const char* name) {
    fails += g_launch_fails.load();
    if (fails) std::printf("%s: %d failures\n", name, fails);
    else std::printf("%s: ok\n", name);
    return fails ? 1 : 0;
}

// the rows [r0[k], r1[k]) band k of a context owns
struct Bands { std::vector<int64_t> r0, r1; };
inline Bands bands_of(swr_context* c) {
    Bands b;
    for (int k = 0; k < swr_context_bands(c); k++) {
        int64_t a = 0, e = 0;
        CHECK(swr_context_band_info(c, k, nullptr, &a, &e) == SWR_OK);
        b.r0.push_back(a); b.r1.push_back(e);
    }
    return b;
}

// the identity with `tag` in m[0]: the stand-in raster writes the tag into every pixel of the frame's depth image
inline void tagm(float* m, float tag) { for (int k = 0; k < 16; k++) m[k] = (k % 5 == 0) ? 1.0f : 0.0f; m[0] = tag; }
inline bool all_eq(const std::vector<float>& d, float v) { for (float x : d) if (x != v) return false; return true; }

struct Scene {
    std::vector<swr_vertex> v;
    std::vector<swr_vertex_attr> a;
    std::vector<swr_skin_vertex> sk;
    std::vector<int64_t> idx;
};

// (the coordinates wrap at primes, so that they stay small however many vertices there are)
inline Scene make_scene(int nv, int ntri, uint32_t top_joint) {
    Scene s;
    s.v.resize(nv); s.a.resize(nv); s.sk.resize(nv); s.idx.resize(3 * (size_t)ntri);
    for (int i = 0; i < nv; i++) {
        s.v[i] = swr_vertex{{0.01f * (i % 97) - 0.5f, 0.3f - 0.002f * (i % 89), 0.1f + 0.001f * (i % 101), 0}, {0.1f, 0.2f, 0.3f, 0}};
        s.a[i] = swr_vertex_attr{{0.5f, 0.01f * (i % 83), -0.25f, 0}, {0.1f * (i % 7), 0.2f, 0, 0}};
        s.sk[i] = swr_skin_vertex{{(uint32_t)(i % 3), (uint32_t)((i + 1) % 3), top_joint, 0}, {0.5f, 0.25f, 0.125f, 0.125f}};
    }
    for (size_t k = 0; k < s.idx.size(); k++) s.idx[k] = (int64_t)((k * 7 + k / 3) % (size_t)nv);
    return s;
}

inline std::vector<float> make_pose(int joints, float salt) {
    std::vector<float> p(16 * (size_t)joints, 0.0f);
    for (int j = 0; j < joints; j++) {
        float* m = &p[16 * (size_t)j];
        m[0] = 1.0f + 0.1f * j + salt; m[5] = 0.9f - 0.05f * j; m[10] = 1.0f; m[15] = 1.0f;
        m[1] = 0.1f * salt; m[4] = -0.2f; m[12] = 0.01f * j; m[13] = salt; m[14] = -0.02f * j;
        m[3] = 77.0f; m[7] = -5.0f;         // the fourth row is ignored
    }
    return p;
}

// morph targets as the caller holds them: packed float3, target-major
struct Targets { std::vector<float> dp, dn; int count; bool nrm; };

// "Morph targets", on the caller's packed arrays: p = b; for t ascending with w[t] != 0: p = p + w[t] * d[t][i]
inline void morph(const float* b, const float* deltas, const float* w, int targets, int64_t nv, int64_t i, float* out) {
    float p[3] = {b[0], b[1], b[2]};
    for (int t = 0; t < targets; t++) {
        if (!(w[t] != 0.0f)) continue;
        const float* d = deltas + ((size_t)t * (size_t)nv + (size_t)i) * 3;
        for (int c = 0; c < 3; c++) { const float m = w[t] * d[c]; p[c] = p[c] + m; }
    }
    memcpy(out, p, sizeof p);
}

// the stream every band must hold: the scene morphed by w over T (either NULL: unmorphed), then in `pose` (NULL: unposed); bands = the
// stream launches the call must have made
inline void expect_stream(const Scene& s, const Targets* T, const float* w, const float* pose, bool nrm, int bands, const char* what) {
    const std::vector<Record> records = take_records();
    if ((int)records.size() != bands) { std::printf("FAIL %s: %zu stream launches, not %d\n", what, records.size(), bands); fails++; return; }
    const int64_t ntri = (int64_t)s.idx.size() / 3, nv = (int64_t)s.v.size();
    for (const Record& r : records) {
        bool ok = r.ntri == ntri && r.nrm == nrm;
        for (int64_t t = 0; ok && t < ntri; t++)
            for (int k = 0; k < 3; k++) {
                const int64_t ix = s.idx[3 * t + k];
                float p[3], n[3];
                memcpy(p, s.v[ix].xyz, 12); memcpy(n, s.a[ix].normal, 12);
                if (T && w) {
                    morph(p, T->dp.data(), w, T->count, nv, ix, p);
                    if (T->nrm) morph(n, T->dn.data(), w, T->count, nv, ix, n);
                }
                if (pose) { float q[3]; blend(p, s.sk[ix], pose, true, q); memcpy(p, q, 12); blend(n, s.sk[ix], pose, false, q); memcpy(n, q, 12); }
                ok = ok && memcmp(&r.tri_xyz[3 * t + k], p, 12) == 0 && (!nrm || memcmp(&r.tri_nrm[3 * t + k], n, 12) == 0);
            }
        if (!ok) { std::printf("FAIL %s: the stream is not the model's (ntri %lld nrm %d)\n", what, (long long)r.ntri, (int)r.nrm); fails++; }
    }
}
inline void expect_no_launch(const char* what) {
    const std::vector<Record> records = take_records();
    if (!records.empty()) { std::printf("FAIL %s: %zu unexpected stream launches\n", what, records.size()); fails++; }
}
