// swr_skin.hip — skinned meshes (include/swr.h "Skinned meshes").
//
// A pose never touches a frame kernel: it rewrites what they read.  Two launches per pose:
//
// k_skin_vertices poses every vertex ONCE, not once per corner that references it (a closed mesh references a vertex about six
// times): one lane per vertex reads the vertex, its four influences and, with attributes, its normal, blends the four joint
// transforms in the header's order — plain multiplies and adds, one rounding each (the build contracts nothing) — and writes the
// posed vertex array (colour copied: k_points / k_lines read it in place of the scene's) and the posed normals.  The joint indices
// differ from lane to lane, so the pose table is a gather: TABLE_LDS keeps it in LDS as 12 floats per joint (the three rows that
// count; a workgroup packs it once and strides over the vertices), the other variant leaves the 64-byte matrices to L2.
//
// k_skin_stream writes the position lanes of the triangle stream (and the normal lanes of tri_nrm) from a vertex array, one lane
// per slot, and — the wave holds the 64 slots of one group — the group's box, with k_box64's operations in k_box64's order.  The w
// lanes (original index, u) and tri_rgb are not written.  Fed the posed arrays it puts the stream into the pose; fed the scene's
// own vertices and attributes it restores the stream the upload built, bit for bit.  Compulsory bytes per slot: 24 of indices, 4 of
// the original index, 36 (+ 36) stored; the 48 (+ 48) gathered come from an array a sixth of the stream's size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "swr_internal.h"
#include "swr_rules.hip.h"

#ifndef SWR_TUNE_SKIN_LDS
#define SWR_TUNE_SKIN_LDS 1        // the pose table in LDS (1) or left to L2 (0): DESIGN.md §23 has the measurement
#endif

namespace swr {

namespace {

constexpr int SKIN_THREADS = 256;

struct SkinArgs {
    const float4* vtx;          // swr_vertex: (xyz, pad), (rgb, pad)
    const float4* attrs;        // swr_vertex_attr: (normal, pad), (uv, pad)
    const swr_skin_vertex* skin;
    const float* joints;        // joint_count x 16, column-major
    float4* posed;              // like vtx
    float4* posed_nrm;          // [nv] (normal, 0)
    int64_t nv;
    int32_t joint_count;
};

struct Affine { float c0[3], c1[3], c2[3], c3[3]; };

template <bool TABLE_LDS>
__device__ __forceinline__ Affine load_joint(const float4* tab, const float4* joints4, uint32_t j) {
    Affine m;
    if (TABLE_LDS) {
        const float4 q0 = tab[3 * j], q1 = tab[3 * j + 1], q2 = tab[3 * j + 2];
        m.c0[0] = q0.x; m.c0[1] = q0.y; m.c0[2] = q0.z;
        m.c1[0] = q0.w; m.c1[1] = q1.x; m.c1[2] = q1.y;
        m.c2[0] = q1.z; m.c2[1] = q1.w; m.c2[2] = q2.x;
        m.c3[0] = q2.y; m.c3[1] = q2.z; m.c3[2] = q2.w;
    } else {
        const float4 a = joints4[4 * j], b = joints4[4 * j + 1], c = joints4[4 * j + 2], d = joints4[4 * j + 3];
        m.c0[0] = a.x; m.c0[1] = a.y; m.c0[2] = a.z;
        m.c1[0] = b.x; m.c1[1] = b.y; m.c1[2] = b.z;
        m.c2[0] = c.x; m.c2[1] = c.y; m.c2[2] = c.z;
        m.c3[0] = d.x; m.c3[1] = d.y; m.c3[2] = d.z;
    }
    return m;
}

template <bool TABLE_LDS, bool NRM>
__global__ __launch_bounds__(SKIN_THREADS) void k_skin_vertices(SkinArgs a) {
    extern __shared__ float4 tab[];
    if (TABLE_LDS) {
        float* t = reinterpret_cast<float*>(tab);
        for (int i = (int)threadIdx.x; i < 12 * a.joint_count; i += SKIN_THREADS) {
            const int j = i / 12, e = i - 12 * j;
            t[i] = a.joints[16 * j + 4 * (e / 3) + e % 3];
        }
        __syncthreads();
    }
    const float4* joints4 = reinterpret_cast<const float4*>(a.joints);
    const int64_t stride = (int64_t)gridDim.x * SKIN_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SKIN_THREADS + threadIdx.x; i < a.nv; i += stride) {
        const float4 p = a.vtx[2 * i], col = a.vtx[2 * i + 1];
        const uint4 jn = *reinterpret_cast<const uint4*>(a.skin[i].joint);
        const float4 wt = *reinterpret_cast<const float4*>(a.skin[i].weight);
        float4 n = make_float4(0, 0, 0, 0);
        if (NRM) n = a.attrs[2 * i];
        const uint32_t jk[4] = {jn.x, jn.y, jn.z, jn.w};
        const float wk[4] = {wt.x, wt.y, wt.z, wt.w};
        float acc[3], nacc[3];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const Affine m = load_joint<TABLE_LDS>(tab, joints4, jk[k]);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float r = m.c0[c] * p.x;            // vertex_shader's order: col0*x, + col1*y, + col2*z, + col3*1
                r = r + m.c1[c] * p.y;
                r = r + m.c2[c] * p.z;
                r = r + m.c3[c] * 1.0f;
                acc[c] = k == 0 ? wk[k] * r : acc[c] + wk[k] * r;
                if (NRM) {
                    float q = m.c0[c] * n.x;
                    q = q + m.c1[c] * n.y;
                    q = q + m.c2[c] * n.z;
                    nacc[c] = k == 0 ? wk[k] * q : nacc[c] + wk[k] * q;
                }
            }
        }
        a.posed[2 * i] = make_float4(acc[0], acc[1], acc[2], p.w);
        a.posed[2 * i + 1] = col;
        if (NRM) a.posed_nrm[i] = make_float4(nacc[0], nacc[1], nacc[2], 0.0f);
    }
}

struct StreamArgs {
    const float4* pos; const float4* nrm;   // the vertex arrays the stream is written from, in float4 units of
    int32_t pos_stride, nrm_stride;         // these strides per vertex
    const int64_t* indices;
    int64_t nv, ntri;
    int32_t reordered;
    float4* tri_xyz; float4* tri_nrm; float4* box64;
};

// one lane per slot; a wave is the 64-slot group blockIdx.x * 4 + wave
template <bool NRM>
__global__ __launch_bounds__(SKIN_THREADS) void k_skin_stream(StreamArgs a) {
    const int64_t s = (int64_t)blockIdx.x * SKIN_THREADS + threadIdx.x;
    const int64_t g = s >> 6;
    if (g >= (a.ntri + 63) / 64) return;        // (wave-uniform)
    GroupBox b = box_start();
    if (s < a.ntri) {
        const int64_t o = a.reordered ? (int64_t)__float_as_uint(a.tri_xyz[3 * s].w) : s;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int64_t ix = a.indices[3 * o + k];
            const bool in = ix >= 0 && ix < a.nv;       // (always: the scene upload validated the indices)
            float4 x = make_float4(0, 0, 0, 0);
            if (in) x = a.pos[(int64_t)a.pos_stride * ix];
            float* out = reinterpret_cast<float*>(a.tri_xyz + 3 * s + k);
            out[0] = x.x; out[1] = x.y; out[2] = x.z;
            if (NRM && in) {
                const float4 n = a.nrm[(int64_t)a.nrm_stride * ix];
                float* nout = reinterpret_cast<float*>(a.tri_nrm + 3 * s + k);
                nout[0] = n.x; nout[1] = n.y; nout[2] = n.z;
            }
            box_fold(b, x);
        }
    }
    box_reduce(b);
    if ((threadIdx.x & 63) == 0) box_store(b, a.box64 + 2 * g);
}

}  // namespace

void launch_skin_vertices(const swr_vertex* vertices, const swr_vertex_attr* attrs, const swr_skin_vertex* skin, int64_t nv,
                          const float* joints, int32_t joint_count, swr_vertex* posed, float4* posed_nrm, hipStream_t s) {
    if (nv <= 0) return;
    SkinArgs a;
    a.vtx = reinterpret_cast<const float4*>(vertices); a.attrs = reinterpret_cast<const float4*>(attrs); a.skin = skin;
    a.joints = joints; a.posed = reinterpret_cast<float4*>(posed); a.posed_nrm = posed_nrm;
    a.nv = nv; a.joint_count = joint_count;
    const bool lds = SWR_TUNE_SKIN_LDS != 0;
    // TABLE_LDS: every workgroup packs the table once, so few workgroups stride over many vertices
    const int64_t blocks = (nv + SKIN_THREADS - 1) / SKIN_THREADS;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, lds ? 1024 : 65536)), block(SKIN_THREADS);
    const size_t bytes = lds ? (size_t)joint_count * 48 : 0;
    with_bools([&](auto LDS, auto NRM) {
        hipLaunchKernelGGL((k_skin_vertices<LDS.value, NRM.value>), grid, block, (uint32_t)bytes, s, a);
    }, lds, attrs != nullptr);
}

void launch_skin_stream(const float4* pos, int pos_stride, const float4* nrm, int nrm_stride, int64_t nv, const int64_t* indices,
                        int64_t ntri, int reordered, float4* tri_xyz, float4* tri_nrm, float4* box64, hipStream_t s) {
    if (ntri <= 0) return;
    StreamArgs a;
    a.pos = pos; a.nrm = nrm; a.pos_stride = pos_stride; a.nrm_stride = nrm_stride;
    a.indices = indices; a.nv = nv; a.ntri = ntri; a.reordered = reordered;
    a.tri_xyz = tri_xyz; a.tri_nrm = tri_nrm; a.box64 = box64;
    const dim3 grid((unsigned)((ntri + SKIN_THREADS - 1) / SKIN_THREADS)), block(SKIN_THREADS);
    if (nrm && tri_nrm) hipLaunchKernelGGL((k_skin_stream<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_skin_stream<false>), grid, block, 0, s, a);
}

}  // namespace swr
