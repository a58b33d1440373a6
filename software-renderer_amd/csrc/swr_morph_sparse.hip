// swr_morph_sparse.hip — sparse morph targets (include/swr.h "Sparse morph targets").
//
// A sparse target lists only the vertices it moves.  The host turns the targets into vertex-major rows over the touched vertices (the
// union of the index lists, swr_internal.h) and pre-fills the morphed arrays with the base, so one launch per swr_morph_set rewrites
// the touched vertices only:
//
// k_morph_sparse: one lane per TOUCHED vertex.  The workgroup first copies the weight table (at most SWR_MORPH_MAX_TARGETS floats, one
// per lane) into LDS.  A lane then reads its vertex number and its row bounds, the base position (and, NRM, the base normal), walks
// the row — one 16-byte load per entry (and, NRM, one more), the weight looked up in LDS by the entry's target, an entry whose weight
// is zero skipped by the float compare the header fixes — and applies per entry and component one multiply and one add, each rounded
// (the build contracts nothing), in row order: the host sorted every row by target.  It writes the position quad of morphed[i] (and,
// NRM, the normal quad of morphed_attrs[i]): the colour and uv quads are those of the pre-fill and never change.
// Rows are short (a vertex is listed by a few targets of a rig) and of different lengths within a wave; the entries of neighbouring
// rows are neighbours in memory, so a wave's first trip reads a contiguous run.
// Compulsory bytes per touched vertex: 4 + 8 of row table, 16 read, 16 written, 16 per entry; with normals the last three double.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swr_internal.h"

namespace swr {

namespace {

constexpr int MORPH_SPARSE_THREADS = 256;
static_assert(MORPH_SPARSE_THREADS >= SWR_MORPH_MAX_TARGETS, "one lane per weight fills the LDS table");

// p = p + w * d, componentwise: the product is rounded, then the sum
__device__ __forceinline__ void apply(float4& p, float w, const float4& e) {
    p.x = p.x + w * e.y;
    p.y = p.y + w * e.z;
    p.z = p.z + w * e.w;
}

template <bool NRM>
__global__ __launch_bounds__(MORPH_SPARSE_THREADS) void k_morph_sparse(MorphSparseArgs a) {
    __shared__ float w[SWR_MORPH_MAX_TARGETS];
    if ((int)threadIdx.x < a.targets) w[threadIdx.x] = a.weights[threadIdx.x];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * MORPH_SPARSE_THREADS + threadIdx.x;
    if (r >= a.touched_count) return;
    const int64_t i = a.touched[r];
    int64_t k = a.row[r];
    const int64_t end = a.row[r + 1];
    const float4* __restrict__ dpos = reinterpret_cast<const float4*>(a.dpos);      // (target bits, dx, dy, dz)
    const float4* __restrict__ dnrm = reinterpret_cast<const float4*>(a.dnrm);
    float4 p = reinterpret_cast<const float4*>(a.vertices)[2 * i];
    float4 n = make_float4(0, 0, 0, 0);
    if (NRM) n = reinterpret_cast<const float4*>(a.attrs)[2 * i];
    for (; k < end; k++) {
        const float4 e = dpos[k];
        float4 f = e;
        if (NRM) f = dnrm[k];
        const float wt = w[__float_as_uint(e.x)];
        if (wt != 0.0f) {
            apply(p, wt, e);
            if (NRM) apply(n, wt, f);
        }
    }
    reinterpret_cast<float4*>(a.morphed)[2 * i] = p;
    if (NRM) reinterpret_cast<float4*>(a.morphed_attrs)[2 * i] = n;
}

}  // namespace

void launch_morph_sparse(const MorphSparseArgs& a, hipStream_t s) {
    if (a.touched_count <= 0) return;      // (a zero grid is a launch error)
    // one lane per touched vertex, no stride: 2^32 vertices are 2^24 workgroups
    const dim3 grid((unsigned)((a.touched_count + MORPH_SPARSE_THREADS - 1) / MORPH_SPARSE_THREADS)), block(MORPH_SPARSE_THREADS);
    if (a.attrs) hipLaunchKernelGGL((k_morph_sparse<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_morph_sparse<false>), grid, block, 0, s, a);
}

}  // namespace swr
