// swr_morph.hip — morph targets (include/swr.h "Morph targets").
//
// Like a pose, a morph never touches a frame kernel: it rewrites what they read.  One launch per swr_morph_set:
//
// k_morph_vertices: one lane per vertex reads the vertex (and, NRM, its attribute record), walks the ACTIVE list — the targets whose
// weight is not zero, in ascending order, compacted by the host: a skipped target's deltas are never read — and applies per target
// and component one multiply and one add, each rounded (the build contracts nothing).  The list entry is the same for every lane:
// the loop counter is uniform, so the entries come through the scalar cache, not per lane.  The loads of MORPH_UNROLL targets are
// issued before the first is consumed: they are independent, only the adds chain.  It writes the morphed vertex array in swr_vertex
// layout (colour and padding lanes copied: k_points / k_lines read it in place of the scene's) and, NRM, the morphed attributes in
// swr_vertex_attr layout (uv copied), so that k_skin_vertices and k_skin_stream take them as they take the scene's own arrays.
//
// Deltas on the device: target-major planes, positions and normals in buffers of their own (a scene without attributes, or targets
// without normal deltas, then reads one dense plane per active target).  Per vertex and target 12 bytes, three dwords per lane
// (SWR_TUNE_MORPH_PAD 0), or a padded float4 (1): DESIGN.md §24 has the measurement.
// Compulsory bytes per vertex: 32 read, 32 written, 12 per active target; with normals each doubles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swr_internal.h"

namespace swr {

namespace {

constexpr int MORPH_THREADS = 256;
constexpr int MORPH_UNROLL = 4;
constexpr int DELTA_FLOATS = SWR_TUNE_MORPH_PAD ? 4 : 3;

struct MorphArgs {
    const float4* vtx;          // swr_vertex: (xyz, pad), (rgb, pad)
    const float4* attrs;        // swr_vertex_attr: (normal, pad), (uv, pad)
    const float* dpos;          // [target][vertex][DELTA_FLOATS]
    const float* dnrm;          // the same shape
    const MorphEntry* list;     // the active targets, ascending
    float4* out;                // like vtx
    float4* out_attrs;          // like attrs
    int64_t nv;
    int32_t active;
};

struct Delta { float x, y, z; };

__device__ __forceinline__ Delta load_delta(const float* plane, int64_t nv, uint32_t target, int64_t i) {
    const float* d = plane + ((int64_t)target * nv + i) * DELTA_FLOATS;
    Delta r;
    if (SWR_TUNE_MORPH_PAD) {
        const float4 q = *reinterpret_cast<const float4*>(d);
        r.x = q.x; r.y = q.y; r.z = q.z;
    } else {
        r.x = d[0]; r.y = d[1]; r.z = d[2];
    }
    return r;
}

// p = p + w * d, componentwise: the product is rounded, then the sum
__device__ __forceinline__ void apply(float4& p, float w, const Delta& d) {
    p.x = p.x + w * d.x;
    p.y = p.y + w * d.y;
    p.z = p.z + w * d.z;
}

template <bool NRM>
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_vertices(MorphArgs a) {
    const int64_t i = (int64_t)blockIdx.x * MORPH_THREADS + threadIdx.x;
    if (i >= a.nv) return;
    const MorphEntry* __restrict__ list = a.list;
    float4 p = a.vtx[2 * i];
    const float4 col = a.vtx[2 * i + 1];
    float4 n = make_float4(0, 0, 0, 0), uv = n;
    if (NRM) { n = a.attrs[2 * i]; uv = a.attrs[2 * i + 1]; }
    int k = 0;
    for (; k + MORPH_UNROLL <= a.active; k += MORPH_UNROLL) {
        MorphEntry e[MORPH_UNROLL];
        Delta dp[MORPH_UNROLL], dn[MORPH_UNROLL];
#pragma unroll
        for (int u = 0; u < MORPH_UNROLL; u++) {
            e[u] = list[k + u];
            dp[u] = load_delta(a.dpos, a.nv, e[u].target, i);
            if (NRM) dn[u] = load_delta(a.dnrm, a.nv, e[u].target, i);
        }
#pragma unroll
        for (int u = 0; u < MORPH_UNROLL; u++) {
            apply(p, e[u].weight, dp[u]);
            if (NRM) apply(n, e[u].weight, dn[u]);
        }
    }
    for (; k < a.active; k++) {
        const MorphEntry e = list[k];
        const Delta dp = load_delta(a.dpos, a.nv, e.target, i);
        apply(p, e.weight, dp);
        if (NRM) { const Delta dn = load_delta(a.dnrm, a.nv, e.target, i); apply(n, e.weight, dn); }
    }
    a.out[2 * i] = p;
    a.out[2 * i + 1] = col;
    if (NRM) { a.out_attrs[2 * i] = n; a.out_attrs[2 * i + 1] = uv; }
}

}  // namespace

void launch_morph_vertices(const swr_vertex* vertices, const swr_vertex_attr* attrs, int64_t nv, const float* dpos, const float* dnrm,
                           const MorphEntry* list, int32_t active, swr_vertex* morphed, swr_vertex_attr* morphed_attrs, hipStream_t s) {
    if (nv <= 0) return;
    MorphArgs a;
    a.vtx = reinterpret_cast<const float4*>(vertices); a.attrs = reinterpret_cast<const float4*>(attrs);
    a.dpos = dpos; a.dnrm = dnrm; a.list = list; a.active = active;
    a.out = reinterpret_cast<float4*>(morphed); a.out_attrs = reinterpret_cast<float4*>(morphed_attrs); a.nv = nv;
    // one lane per vertex, no stride: 2^32 vertices are 2^24 workgroups
    const dim3 grid((unsigned)((nv + MORPH_THREADS - 1) / MORPH_THREADS)), block(MORPH_THREADS);
    if (attrs) hipLaunchKernelGGL((k_morph_vertices<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_morph_vertices<false>), grid, block, 0, s, a);
}

}  // namespace swr
