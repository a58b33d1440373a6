// swr_normals.hip — computed normals (include/swr.h "Computed normals").
//
// The normals of the mesh as it is drawn, from the positions that are drawn.  Nothing here touches a frame kernel: the kernels write
// what the frames read, the normal lanes of tri_nrm.  Every operation is the header's, in the header's order, one rounding each (the
// build contracts nothing); sqrtf and the divide are correctly rounded (the build says so).
//
// SWR_NORMALS_SMOOTH, two launches in front of k_skin_stream (swr_skin.hip), which then writes the stream's normal lanes from
// auto_nrm exactly as it writes them from posed normals:
//   k_face_normals: one lane per triangle p of the index array.  Three int64 indices (a wave reads 1536 contiguous bytes), three
//   positions gathered from the final vertex array (the scene's, the morphed or the posed one: the pair k_skin_stream takes), the
//   two edges, one cross product, one 16-byte store face[p] = (f, 0).  Compulsory bytes per triangle: 24 + 48 gathered + 16.
//   k_vertex_normals: one lane per vertex i walks its row adj_tri[adj_off[i] .. adj_off[i + 1]) of the adjacency the host built
//   (ascending by corner, duplicates kept) and adds face[adj_tri[e]] in row order, one 16-byte gather per entry, then normalises and
//   stores auto_nrm[i] = (n, 0).  The sum is sequential in ONE lane: float addition is not associative and the header fixes the
//   order, so a row is never split over lanes; a hub of valence 1000 costs its lane 1000 dependent adds while the rest of its wave
//   idles.  Accepted: meshes have valence about six.  Compulsory bytes per vertex: 8 of row bounds + 16 stored, 4 + 16 per entry.
// SWR_NORMALS_FLAT, one launch behind k_skin_stream (which has written the positions):
//   k_flat_normals: one lane per stream slot reads the xyz lanes of the slot's three tri_xyz entries — already de-indexed, in corner
//   order, whatever the slot order is — computes f and stores it into the xyz lanes of the three tri_nrm entries.  The w lanes (u)
//   are not written.  No adjacency, no face array.  Compulsory bytes per slot: 48 read + 36 written.
// All three grids are exact, ceil(n / 256) workgroups of one lane per element: no stride, no cap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "swr_internal.h"
#include "swr_rules.hip.h"

namespace swr {

namespace {

constexpr int NORMALS_THREADS = 256;

// f = cross(b - a, c - a); FLIP: cross(c - a, b - a)
template <bool FLIP>
__device__ __forceinline__ Vec3 face_vector(const float4& a, const float4& b, const float4& c) {
    const Vec3 e1 = {b.x - a.x, b.y - a.y, b.z - a.z};
    const Vec3 e2 = {c.x - a.x, c.y - a.y, c.z - a.z};
    return FLIP ? cross3(e2, e1) : cross3(e1, e2);
}

struct FaceArgs {
    const float4* pos;          // the vertex array in effect, in float4 units of
    int32_t pos_stride;         // this stride per vertex
    const int64_t* indices;
    int64_t nv, ntri;
    float4* face;               // [ntri] (f, 0)
};

template <bool FLIP>
__global__ __launch_bounds__(NORMALS_THREADS) void k_face_normals(FaceArgs a) {
    const int64_t p = (int64_t)blockIdx.x * NORMALS_THREADS + threadIdx.x;
    if (p >= a.ntri) return;
    float4 x[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int64_t ix = a.indices[3 * p + k];
        const bool in = ix >= 0 && ix < a.nv;           // (always: the scene upload validated the indices)
        x[k] = make_float4(0, 0, 0, 0);
        if (in) x[k] = a.pos[(int64_t)a.pos_stride * ix];
    }
    const Vec3 f = face_vector<FLIP>(x[0], x[1], x[2]);
    a.face[p] = make_float4(f.x, f.y, f.z, 0.0f);
}

struct VertexArgs {
    const uint32_t* adj_off;    // [nv + 1]
    const uint32_t* adj_tri;    // [adj_off[nv]] triangles per vertex, ascending by corner, duplicates kept
    const float4* face;
    int64_t nv;
    float4* auto_nrm;           // [nv] (n, 0)
};

__global__ __launch_bounds__(NORMALS_THREADS) void k_vertex_normals(VertexArgs a) {
    const int64_t i = (int64_t)blockIdx.x * NORMALS_THREADS + threadIdx.x;
    if (i >= a.nv) return;
    const uint32_t end = a.adj_off[i + 1];
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    for (uint32_t e = a.adj_off[i]; e < end; e++) {
        const float4 f = a.face[a.adj_tri[e]];
        nx = nx + f.x;
        ny = ny + f.y;
        nz = nz + f.z;
    }
    const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (l > 0.0f) {                                     // (false for 0 and for NaN: n stays as it is)
        const float r = 1.0f / l;
        nx = nx * r;
        ny = ny * r;
        nz = nz * r;
    }
    a.auto_nrm[i] = make_float4(nx, ny, nz, 0.0f);
}

template <bool FLIP>
__global__ __launch_bounds__(NORMALS_THREADS) void k_flat_normals(const float4* __restrict__ tri_xyz, int64_t ntri, float4* __restrict__ tri_nrm) {
    const int64_t s = (int64_t)blockIdx.x * NORMALS_THREADS + threadIdx.x;
    if (s >= ntri) return;
    const Vec3 f = face_vector<FLIP>(tri_xyz[3 * s], tri_xyz[3 * s + 1], tri_xyz[3 * s + 2]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float* out = reinterpret_cast<float*>(tri_nrm + 3 * s + k);
        out[0] = f.x; out[1] = f.y; out[2] = f.z;
    }
}

inline dim3 exact_grid(int64_t n) { return dim3((unsigned)((n + NORMALS_THREADS - 1) / NORMALS_THREADS)); }

}  // namespace

void launch_face_normals(const float4* pos, int pos_stride, int64_t nv, const int64_t* indices, int64_t ntri, bool flip, float4* face,
                         hipStream_t s) {
    if (ntri <= 0) return;      // (a zero grid is a launch error)
    FaceArgs a;
    a.pos = pos; a.pos_stride = pos_stride; a.indices = indices; a.nv = nv; a.ntri = ntri; a.face = face;
    const dim3 grid = exact_grid(ntri), block(NORMALS_THREADS);
    with_bools([&](auto FLIP) { hipLaunchKernelGGL((k_face_normals<FLIP.value>), grid, block, 0, s, a); }, flip);
}

void launch_vertex_normals(const uint32_t* adj_off, const uint32_t* adj_tri, const float4* face, int64_t nv, float4* auto_nrm,
                           hipStream_t s) {
    if (nv <= 0) return;
    VertexArgs a;
    a.adj_off = adj_off; a.adj_tri = adj_tri; a.face = face; a.nv = nv; a.auto_nrm = auto_nrm;
    const dim3 grid = exact_grid(nv), block(NORMALS_THREADS);
    hipLaunchKernelGGL(k_vertex_normals, grid, block, 0, s, a);
}

void launch_flat_normals(const float4* tri_xyz, int64_t ntri, bool flip, float4* tri_nrm, hipStream_t s) {
    if (ntri <= 0) return;
    const dim3 grid = exact_grid(ntri), block(NORMALS_THREADS);
    with_bools([&](auto FLIP) { hipLaunchKernelGGL((k_flat_normals<FLIP.value>), grid, block, 0, s, tri_xyz, ntri, tri_nrm); }, flip);
}

}  // namespace swr
