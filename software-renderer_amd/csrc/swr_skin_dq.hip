// swr_skin_dq.hip — dual-quaternion skinning (include/swr.h "Dual-quaternion skinning").
//
// k_skin_vertices_dq is k_skin_vertices (swr_skin.hip) with another blend: it reads the same arrays, writes the same posed arrays, and
// k_skin_stream follows it unchanged.  One lane poses one vertex once.  The pose is two float4 per joint — the real quaternion, then
// the dual quaternion, (x, y, z, w) each — and stays in LDS as it arrives, 32 bytes a joint (32 KB at SWR_SKIN_MAX_JOINTS): a
// workgroup copies it once and strides over the vertices.  Per vertex: the sign of influences 1..3 against influence 0, the blend of
// the eight components, one sqrtf and one divide (both correctly rounded: the build says so), three cross products for the position
// and two for the normal.  Every operation is the header's, in the header's order, one rounding each (the build contracts nothing).
// Compulsory bytes per vertex, as the matrix kernel's: 32 read + 32 of influences + 32 written, + 16 + 16 with normals.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "swr_internal.h"
#include "swr_rules.hip.h"

namespace swr {

namespace {

constexpr int SKIN_DQ_THREADS = 256;

struct SkinDqArgs {
    const float4* vtx;          // swr_vertex: (xyz, pad), (rgb, pad)
    const float4* attrs;        // swr_vertex_attr: (normal, pad), (uv, pad)
    const swr_skin_vertex* skin;
    const float4* dq;           // joint_count x (real, dual)
    float4* posed;              // like vtx
    float4* posed_nrm;          // [nv] (normal, 0)
    int64_t nv;
    int32_t joint_count;
};

// a = cross(q, x);  b = a + w*x;  c = cross(q, b);  rot(x) = x + 2*c
__device__ __forceinline__ Vec3 dq_rotate(const Vec3 q, const float w, const Vec3 x) {
    const Vec3 a = cross3(q, x);
    Vec3 b;
    b.x = a.x + w * x.x; b.y = a.y + w * x.y; b.z = a.z + w * x.z;
    const Vec3 c = cross3(q, b);
    Vec3 r;
    r.x = x.x + 2.0f * c.x; r.y = x.y + 2.0f * c.y; r.z = x.z + 2.0f * c.z;
    return r;
}

template <bool NRM>
__global__ __launch_bounds__(SKIN_DQ_THREADS) void k_skin_vertices_dq(SkinDqArgs a) {
    extern __shared__ float4 dq_tab[];
    for (int i = (int)threadIdx.x; i < 2 * a.joint_count; i += SKIN_DQ_THREADS) dq_tab[i] = a.dq[i];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * SKIN_DQ_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SKIN_DQ_THREADS + threadIdx.x; i < a.nv; i += stride) {
        const float4 p = a.vtx[2 * i], col = a.vtx[2 * i + 1];
        const uint4 jn = *reinterpret_cast<const uint4*>(a.skin[i].joint);
        const float4 wt = *reinterpret_cast<const float4*>(a.skin[i].weight);
        const uint32_t jk[4] = {jn.x, jn.y, jn.z, jn.w};
        const float wk[4] = {wt.x, wt.y, wt.z, wt.w};
        const float4 r0 = dq_tab[2 * jk[0]];
        float4 br, bd;                                  // the blend: real, dual
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float4 r = k == 0 ? r0 : dq_tab[2 * jk[k]], d = dq_tab[2 * jk[k] + 1];
            float u = wk[k];
            if (k > 0) {
                const float s = ((r0.x * r.x + r0.y * r.y) + r0.z * r.z) + r0.w * r.w;
                u = s < 0.0f ? -wk[k] : wk[k];          // (a NaN or zero s keeps the weight)
            }
            if (k == 0) {
                br = make_float4(u * r.x, u * r.y, u * r.z, u * r.w);
                bd = make_float4(u * d.x, u * d.y, u * d.z, u * d.w);
            } else {
                br.x = br.x + u * r.x; br.y = br.y + u * r.y; br.z = br.z + u * r.z; br.w = br.w + u * r.w;
                bd.x = bd.x + u * d.x; bd.y = bd.y + u * d.y; bd.z = bd.z + u * d.z; bd.w = bd.w + u * d.w;
            }
        }
        const float n2 = ((br.x * br.x + br.y * br.y) + br.z * br.z) + br.w * br.w;
        const float l = sqrtf(n2);
        const float inv = 1.0f / l;
        const Vec3 q = {br.x * inv, br.y * inv, br.z * inv};
        const float w = br.w * inv;
        const Vec3 d = {bd.x * inv, bd.y * inv, bd.z * inv};
        const float dw = bd.w * inv;
        const Vec3 v = {p.x, p.y, p.z};
        const Vec3 rv = dq_rotate(q, w, v);
        const Vec3 e = cross3(q, d);
        Vec3 t;                                         // t = 2 * ((w*d - dw*q) + e)
        t.x = 2.0f * ((w * d.x - dw * q.x) + e.x);
        t.y = 2.0f * ((w * d.y - dw * q.y) + e.y);
        t.z = 2.0f * ((w * d.z - dw * q.z) + e.z);
        a.posed[2 * i] = make_float4(rv.x + t.x, rv.y + t.y, rv.z + t.z, p.w);
        a.posed[2 * i + 1] = col;
        if (NRM) {
            const float4 n = a.attrs[2 * i];
            const Vec3 n3 = {n.x, n.y, n.z};
            const Vec3 rn = dq_rotate(q, w, n3);
            a.posed_nrm[i] = make_float4(rn.x, rn.y, rn.z, 0.0f);
        }
    }
}

}  // namespace

void launch_skin_vertices_dq(const swr_vertex* vertices, const swr_vertex_attr* attrs, const swr_skin_vertex* skin, int64_t nv,
                             const float* dual_quats, int32_t joint_count, swr_vertex* posed, float4* posed_nrm, hipStream_t s) {
    if (nv <= 0) return;
    SkinDqArgs a;
    a.vtx = reinterpret_cast<const float4*>(vertices); a.attrs = reinterpret_cast<const float4*>(attrs); a.skin = skin;
    a.dq = reinterpret_cast<const float4*>(dual_quats); a.posed = reinterpret_cast<float4*>(posed); a.posed_nrm = posed_nrm;
    a.nv = nv; a.joint_count = joint_count;
    // every workgroup copies the table once, so few workgroups stride over many vertices
    const int64_t blocks = (nv + SKIN_DQ_THREADS - 1) / SKIN_DQ_THREADS;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, 1024)), block(SKIN_DQ_THREADS);
    const size_t bytes = (size_t)joint_count * 32;
    with_bools([&](auto NRM) {
        hipLaunchKernelGGL((k_skin_vertices_dq<NRM.value>), grid, block, (uint32_t)bytes, s, a);
    }, attrs != nullptr);
}

}  // namespace swr
