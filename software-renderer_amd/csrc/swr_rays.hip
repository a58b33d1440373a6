// swr_rays.hip — ray casts (include/swr.h "Ray casts").
//
// hits[k] = the nearest accepted hit of rays[k] on the resident triangle stream: 48 contiguous bytes per triangle (tri_xyz), and the
// object-space box of every 64-slot group (box64) as a one-level bounding hierarchy.  The box pre-test of the header is monotone in
// the box (rounded subtraction and rounded multiplication by a fixed r are monotone) and a triangle's box lies inside its group's,
// so "pre-test the group's box, then run steps 1-3 on its 64 slots" accepts exactly the triangles brute force accepts.
//
//   k_rays_init     one lane per ray: its key word = all ones (no hit), by a plain store.
//   k_rays<CULL>    one workgroup per (chunk of RAYS_GROUPS_PER_WG groups, ray), the ray in scalar registers.  Pass 1: a lane tests
//                   one group box per trip of 256; a poisoned box (NaN: a corner of the group is not finite) always passes; the
//                   survivors are compacted by ballot into an LDS queue (one LDS atomic per wave and trip).  Pass 2: one wave per
//                   queued group, one lane per slot: three float4 loads, steps 1-3, the 64-bit key (orderable(t) << 32) | p kept as
//                   a running minimum per lane.  Then a wave64 reduction of the key by shuffles, four waves through LDS, and ONE
//                   64-bit atomicMin per workgroup into the ray's key word — none when the workgroup accepted nothing.
//                   orderable_depth (swr_rules.hip.h) is monotone and t carries no -0 (the header's + 0.0f), so the minimum of
//                   the keys is the smallest t and, on equal t, the smallest p: order-free, hence bit-defined.  No float atomic.
//   k_rays_finish   one lane per ray: the winner decoded, its slot found (inv when the stream is reordered), u and v computed again
//                   with the same operations, the 16-byte record written by one vector store.
//
// Ray queries (include/swr.h "Ray queries") ride on the same launch, chosen by RaysArgs::flags and [p_begin, p_end):
//   k_rays<CULL, true>      nearest mode with a range or a facing cull: pass 2 also tests, per lane, the primitive against the range
//                           and the sign of the det that step 3 computed against the cull bits.  <CULL, false> is swr_cast_rays: it
//                           reads none of the three fields.
//   k_rays_any<FILTER>      SWR_RAYS_ANY_HIT: the same grid and pass 1.  On entry one lane reads the ray's key word once (a relaxed
//                           agent-scope atomic load) and the workgroup leaves, uniformly, if another workgroup has already found the
//                           ray occluded.  In pass 2 a wave stops at the first trip whose ballot of hits is not zero and raises a
//                           flag in LDS, which the other waves read once per trip; no barrier inside that loop, one behind it.  One
//                           lane publishes by an atomicMin of 0 on the key word: the word is all ones or it is not, and that is the
//                           whole answer — an OR over the triangles, whatever the order, the timing and the placement.
//   k_rays_finish<true>     the any-hit decode: {SWR_RAY_OCCLUDED, 0, 0, 0} or the miss; nothing is recomputed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>
#include <cmath>

#include "swr_internal.h"
#include "swr_rules.hip.h"

namespace swr {

namespace {

#ifndef SWR_TUNE_RAYS_CULL
#define SWR_TUNE_RAYS_CULL 1                // 1 = the product: the group boxes are tested first; 0 = brute force, every group is entered
                                            // (the A/B build of DESIGN.md §30)
#endif

constexpr int RAYS_THREADS = 256;
constexpr int RAYS_WAVES = RAYS_THREADS / 64;
static_assert(RAYS_GROUPS_PER_WG % RAYS_THREADS == 0, "pass 1 is a whole number of trips");
static_assert(sizeof(swr_ray) == 32 && sizeof(swr_ray_hit) == 16, "include/swr.h");
constexpr unsigned long long RAYS_NO_HIT = ~0ull;

// the header's dot and cross: no FMA (-ffp-contract=off), the association as written
__device__ __forceinline__ float ray_dot(const float3& x, const float3& y) { return (x.x * y.x + x.y * y.y) + x.z * y.z; }
__device__ __forceinline__ float3 ray_cross(const float3& a, const float3& b) {
    return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ float3 ray_sub(const float3& a, const float3& b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }

// a ray as the kernels hold it: the header's record and, per axis, r = 1 / dir and whether the axis is parallel
struct RayRegs {
    float o[3], d[3], r[3];
    bool par[3];
    float tmin, tmax;
};
__device__ __forceinline__ RayRegs ray_regs(const swr_ray& q) {
    RayRegs R;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        R.o[j] = q.origin[j]; R.d[j] = q.dir[j];
        R.r[j] = 1.0f / q.dir[j];
        R.par[j] = q.dir[j] == 0.0f || !(fabsf(R.r[j]) <= FLT_MAX);
    }
    R.tmin = q.tmin; R.tmax = q.tmax;
    return R;
}

// step 2 of the header on the box [lo, hi]: the same operations for a triangle's box and for a group's
__device__ __forceinline__ bool ray_box(const RayRegs& R, const float lo[3], const float hi[3]) {
    float nr = R.tmin, fr = R.tmax;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float t0 = (lo[j] - R.o[j]) * R.r[j], t1 = (hi[j] - R.o[j]) * R.r[j];
        const float near = t0 < t1 ? t0 : t1, far = t0 < t1 ? t1 : t0;
        const bool inside = lo[j] <= R.o[j] && R.o[j] <= hi[j];
        ok = ok && (!R.par[j] || inside);
        nr = (!R.par[j] && near > nr) ? near : nr;
        fr = (!R.par[j] && far < fr) ? far : fr;
    }
    return ok && nr <= fr;
}

// steps 1-3 on one triangle: whether it is accepted, and t, u, v and the det of step 3
__device__ __forceinline__ bool ray_triangle(const RayRegs& R, const float4& xa, const float4& xb, const float4& xc, float& t, float& u,
                                             float& v, float& det) {
    const float ca[3] = {xa.x, xa.y, xa.z}, cb[3] = {xb.x, xb.y, xb.z}, cc[3] = {xc.x, xc.y, xc.z};
    bool finite = true;
    float lo[3], hi[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        finite = finite && fabsf(ca[j]) < INFINITY && fabsf(cb[j]) < INFINITY && fabsf(cc[j]) < INFINITY;
        lo[j] = fminf(fminf(ca[j], cb[j]), cc[j]);
        hi[j] = fmaxf(fmaxf(ca[j], cb[j]), cc[j]);
    }
    const bool box = ray_box(R, lo, hi);
    const float3 a = make_float3(xa.x, xa.y, xa.z), b = make_float3(xb.x, xb.y, xb.z), c = make_float3(xc.x, xc.y, xc.z);
    const float3 o = make_float3(R.o[0], R.o[1], R.o[2]), d = make_float3(R.d[0], R.d[1], R.d[2]);
    const float3 e1 = ray_sub(b, a), e2 = ray_sub(c, a);
    const float3 pv = ray_cross(d, e2);
    det = ray_dot(e1, pv);
    const float inv = 1.0f / det;
    const float3 tv = ray_sub(o, a);
    u = ray_dot(tv, pv) * inv;
    const float3 qv = ray_cross(tv, e1);
    v = ray_dot(d, qv) * inv;
    t = ray_dot(e2, qv) * inv + 0.0f;
    return finite && box && fabsf(det) > 0.0f && u >= 0.0f && u <= 1.0f && v >= 0.0f && u + v <= 1.0f && t >= R.tmin && t <= R.tmax;
}

__device__ __forceinline__ bool ray_triangle(const RayRegs& R, const float4& xa, const float4& xb, const float4& xc, float& t, float& u,
                                             float& v) {
    float det;
    return ray_triangle(R, xa, xb, xc, t, u, v, det);
}

// "Ray queries": whether primitive p, whose step 3 gave det, survives the query's range and facing cull.  det is not zero and not a
// NaN wherever the answer is used (step 3 has rejected the triangle otherwise).
__device__ __forceinline__ bool ray_query_keeps(const RaysArgs& a, uint32_t p, float det) {
    const bool front = (a.flags & SWR_RAYS_FRONT_CW) ? det < 0.0f : det > 0.0f;
    const bool culled = front ? (a.flags & SWR_RAYS_CULL_FRONT) != 0 : (a.flags & SWR_RAYS_CULL_BACK) != 0;
    return (int64_t)p >= a.p_begin && (int64_t)p < a.p_end && !culled;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(k, off);
        k = other < k ? other : k;
    }
    return k;
}

__device__ __forceinline__ uint32_t ray_of_block() { return blockIdx.z * gridDim.y + blockIdx.y; }

__global__ __launch_bounds__(RAYS_THREADS) void k_rays_init(unsigned long long* keys, uint32_t n) {
    const uint32_t k = blockIdx.x * RAYS_THREADS + threadIdx.x;
    if (k < n) keys[k] = RAYS_NO_HIT;
}

template <bool CULL, bool FILTER>
__global__ __launch_bounds__(RAYS_THREADS) void k_rays(RaysArgs a) {
    __shared__ uint32_t s_queue[RAYS_GROUPS_PER_WG];
    __shared__ uint32_t s_count;
    __shared__ unsigned long long s_key[RAYS_WAVES];
    const uint32_t ray = ray_of_block();
    if (ray >= (uint32_t)a.n) return;           // (uniform: the second z-plane of an odd ray count)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const RayRegs R = ray_regs(a.rays[ray]);
    const int64_t g0 = (int64_t)blockIdx.x * RAYS_GROUPS_PER_WG;        // < groups: the grid has ceil(groups / RAYS_GROUPS_PER_WG) chunks
    const uint32_t in_chunk = (uint32_t)(a.groups - g0 < RAYS_GROUPS_PER_WG ? a.groups - g0 : RAYS_GROUPS_PER_WG);
    uint32_t queued;
    if (CULL) {
        if (threadIdx.x == 0) s_count = 0;
        __syncthreads();
        for (uint32_t i = 0; i < (uint32_t)RAYS_GROUPS_PER_WG; i += RAYS_THREADS) {
            if (i >= in_chunk) break;           // (uniform)
            const uint32_t gi = i + threadIdx.x;
            const bool in = gi < in_chunk;
            // (a lane past the chunk's end reads the chunk's last box instead and is left out: no load is under a branch)
            const size_t g = (size_t)g0 + (in ? gi : in_chunk - 1u);
            const float4 bl = a.box64[2 * g], bh = a.box64[2 * g + 1];
            const float lo[3] = {bl.x, bl.y, bl.z}, hi[3] = {bh.x, bh.y, bh.z};
            const bool pass = in && (!(bl.x == bl.x) || ray_box(R, lo, hi));       // (box_reduce poisons every lane of the box at once)
            const unsigned long long m = __ballot(pass);
            uint32_t base = 0;
            if (lane == 0 && m) base = atomicAdd(&s_count, (uint32_t)__popcll(m));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            if (pass) s_queue[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = gi;
        }
        __syncthreads();
        queued = s_count;
    } else {
        queued = in_chunk;
    }
    unsigned long long best = RAYS_NO_HIT;
    for (uint32_t q = wave; q < queued; q += RAYS_WAVES) {
        const int64_t g = g0 + (CULL ? s_queue[q] : q);
        const int64_t s = g * 64 + lane;
        const bool in = s < a.ntri;
        const size_t sl = (size_t)(in ? s : a.ntri - 1);       // (ntri >= 1: a scene without triangles has no groups and no launch)
        const float4 xa = a.tri_xyz[3 * sl], xb = a.tri_xyz[3 * sl + 1], xc = a.tri_xyz[3 * sl + 2];
        float t, u, v, det;
        bool hit = ray_triangle(R, xa, xb, xc, t, u, v, det) && in;
        const uint32_t p = a.reordered ? __float_as_uint(xa.w) : (uint32_t)sl;
        if (FILTER) hit = hit && ray_query_keeps(a, p, det);
        const unsigned long long key = ((unsigned long long)orderable_depth(t) << 32) | p;
        best = (hit && key < best) ? key : best;
    }
    best = wave_min_u64(best);
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long k = s_key[0];
        for (int i = 1; i < RAYS_WAVES; i++) k = s_key[i] < k ? s_key[i] : k;
        if (k != RAYS_NO_HIT) atomicMin(&a.keys[ray], k);
    }
}

// SWR_RAYS_ANY_HIT: is any triangle of the chunk accepted?  The ray's key word drops from all ones to 0 when one is; nothing else of
// it is ever read, so which workgroup, wave or lane found the triangle cannot show in the result.
template <bool FILTER>
__global__ __launch_bounds__(RAYS_THREADS) void k_rays_any(RaysArgs a) {
    __shared__ uint32_t s_queue[RAYS_GROUPS_PER_WG];
    __shared__ uint32_t s_count;
    __shared__ uint32_t s_done;         // the ray is occluded: on entry by another workgroup's word, in pass 2 by a wave of this one
    const uint32_t ray = ray_of_block();
    if (ray >= (uint32_t)a.n) return;           // (uniform: the second z-plane of an odd ray count)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (threadIdx.x == 0) {
        s_count = 0;
        // one look at what the other workgroups of this ray have published so far: a stale all-ones costs time, never the answer
        s_done = __hip_atomic_load(&a.keys[ray], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != RAYS_NO_HIT;
    }
    __syncthreads();
    if (s_done) return;                         // (uniform: one LDS word, read by every lane behind the barrier; it is written again
                                                // only in pass 2, behind the barrier that closes pass 1)
    const RayRegs R = ray_regs(a.rays[ray]);
    const int64_t g0 = (int64_t)blockIdx.x * RAYS_GROUPS_PER_WG;
    const uint32_t in_chunk = (uint32_t)(a.groups - g0 < RAYS_GROUPS_PER_WG ? a.groups - g0 : RAYS_GROUPS_PER_WG);
    // pass 1 as in k_rays, line for line (a shared function costs k_rays the schedule DESIGN.md §30 measured: §31)
    for (uint32_t i = 0; i < (uint32_t)RAYS_GROUPS_PER_WG; i += RAYS_THREADS) {
        if (i >= in_chunk) break;           // (uniform)
        const uint32_t gi = i + threadIdx.x;
        const bool in = gi < in_chunk;
        const size_t g = (size_t)g0 + (in ? gi : in_chunk - 1u);
        const float4 bl = a.box64[2 * g], bh = a.box64[2 * g + 1];
        const float lo[3] = {bl.x, bl.y, bl.z}, hi[3] = {bh.x, bh.y, bh.z};
        const bool pass = in && (!(bl.x == bl.x) || ray_box(R, lo, hi));
        const unsigned long long m = __ballot(pass);
        uint32_t base = 0;
        if (lane == 0 && m) base = atomicAdd(&s_count, (uint32_t)__popcll(m));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (pass) s_queue[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = gi;
    }
    __syncthreads();
    const uint32_t queued = s_count;
    for (uint32_t q = wave; q < queued; q += RAYS_WAVES) {
        // (one read per trip; every lane of the wave reads the same word, so the wave leaves as one)
        if (__hip_atomic_load(&s_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
        const int64_t s = (g0 + s_queue[q]) * 64 + lane;
        const bool in = s < a.ntri;
        const size_t sl = (size_t)(in ? s : a.ntri - 1);
        const float4 xa = a.tri_xyz[3 * sl], xb = a.tri_xyz[3 * sl + 1], xc = a.tri_xyz[3 * sl + 2];
        float t, u, v, det;
        bool hit = ray_triangle(R, xa, xb, xc, t, u, v, det) && in;
        if (FILTER) hit = hit && ray_query_keeps(a, a.reordered ? __float_as_uint(xa.w) : (uint32_t)sl, det);
        if (__ballot(hit)) {
            if (lane == 0) __hip_atomic_store(&s_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            break;
        }
    }
    __syncthreads();                            // (every wave arrives: the loop has no other way out)
    if (threadIdx.x == 0 && s_done) atomicMin(&a.keys[ray], 0ull);
}

template <bool ANY>
__global__ __launch_bounds__(RAYS_THREADS) void k_rays_finish(RaysArgs a) {
    const uint32_t k = blockIdx.x * RAYS_THREADS + threadIdx.x;
    if (k >= (uint32_t)a.n) return;
    const unsigned long long key = a.keys[k];
    uint4 out = make_uint4(SWR_ID_NONE, 0u, 0u, 0u);
    if (ANY) {
        if (key != RAYS_NO_HIT) out.x = SWR_RAY_OCCLUDED;
    } else if (key != RAYS_NO_HIT) {
        const uint32_t p = (uint32_t)key;       // (< ntri: the w lane of a reordered stream's corner 0, or the slot itself)
        const size_t s = a.reordered ? a.inv[p] : p;
        const RayRegs R = ray_regs(a.rays[k]);
        float t, u, v;
        ray_triangle(R, a.tri_xyz[3 * s], a.tri_xyz[3 * s + 1], a.tri_xyz[3 * s + 2], t, u, v);
        // (t of the key, bit for bit the t computed here: orderable_depth is a bijection)
        out = make_uint4(p, __float_as_uint(depth_from_orderable((uint32_t)(key >> 32))), __float_as_uint(u), __float_as_uint(v));
    }
    reinterpret_cast<uint4*>(a.hits)[k] = out;
}

}  // namespace

void launch_cast_rays(const RaysArgs& a, hipStream_t s) {
    if (a.n <= 0 || a.n > SWR_RAYS_MAX) return;
    const dim3 per_ray((uint32_t)(a.n + RAYS_THREADS - 1) / RAYS_THREADS), block(RAYS_THREADS);
    hipLaunchKernelGGL(k_rays_init, per_ray, block, 0, s, a.keys, (uint32_t)a.n);
    const bool any = (a.flags & SWR_RAYS_ANY_HIT) != 0;
    // a query that is not swr_cast_rays itself: a facing cull, or a range that leaves a primitive out
    const bool filter = (a.flags & (SWR_RAYS_CULL_BACK | SWR_RAYS_CULL_FRONT)) != 0 || a.p_begin > 0 || a.p_end < a.ntri;
    if (a.groups > 0 && a.p_begin < a.p_end) {      // (an empty range: every ray misses, as over no groups)
        // one workgroup per (chunk, ray); the rays split over y and z so that SWR_RAYS_MAX of them fit the 65 535 of a grid's y
        const uint32_t planes = ((uint32_t)a.n + 65534u) / 65535u;
        const dim3 grid((uint32_t)rays_chunks(a.groups), ((uint32_t)a.n + planes - 1u) / planes, planes);
        if (any) {
            if (filter) hipLaunchKernelGGL((k_rays_any<true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((k_rays_any<false>), grid, block, 0, s, a);
        } else if (filter) {
            hipLaunchKernelGGL((k_rays<true, true>), grid, block, 0, s, a);
        } else if (SWR_TUNE_RAYS_CULL) {
            hipLaunchKernelGGL((k_rays<true, false>), grid, block, 0, s, a);
        } else {
            hipLaunchKernelGGL((k_rays<false, false>), grid, block, 0, s, a);
        }
    }
    if (any) hipLaunchKernelGGL((k_rays_finish<true>), per_ray, block, 0, s, a);
    else hipLaunchKernelGGL((k_rays_finish<false>), per_ray, block, 0, s, a);
}

}  // namespace swr
