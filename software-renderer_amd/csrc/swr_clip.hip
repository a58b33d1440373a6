// swr_clip.hip — depth clipping (SWR_FLAG_DEPTH_CLIP, include/swr.h "Depth clipping").
//
// A clip frame is drawn as the frame without the flag of another scene: every submitted triangle replaced by its fan of
// clipped sub-triangles, every fan vertex given in NDC, the identity transform.  That scene is built per frame, on the
// frame's own stream, into the working set of its lane:
//
//   k_clip_count   one thread per submitted triangle (index order, or order number of a draw list): the clip-space vertices
//                  through vertex_shader, the clip, the number of fan triangles (0 .. 3)
//   k_clip_scan    the per-workgroup sums of those counts -> exclusive offsets (one workgroup), the post-clip count behind them
//   k_clip_emit    the same clip again; fan triangle s of p goes to frame slot base[p] + s: its NDC corners (tri_xyz), colours
//                  (tri_rgb) and attributes (tri_nrm) — the layout of the scene's triangle stream, in index order — and the
//                  original number map[slot] = p.  Slots from the post-clip count up to the frame's n + 2F are invalid.
//   k_clip_box     the box of every 64-slot group of that stream (the band culling of the binning kernels)
//   ... the frame's binning and raster, unchanged, over the n + 2F slots with the identity transform ...
//   k_clip_ids     (SWR_FLAG_PRIMITIVE_IDS) the ID image: order number -> original number
//
// Every arithmetic operation below is one IEEE binary32 rounding (the build contracts nothing, -ffp-contract=off; the
// _rn intrinsics say it again), so the test suite's numpy clipper restates it bit for bit.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <algorithm>

#include "swr_internal.h"
#include "swr_rules.hip.h"
#include "swr_shaders.hip.h"

namespace swr {

namespace {

// One vertex of the clip polygon: x, y, z, w, r, g, b, nx, ny, nz, u, v.
constexpr int NC = 12;
constexpr int MAXV = 5;          // a triangle clipped by two planes has at most five vertices

struct Poly {
    float c[MAXV][NC];
    int n;
};

__device__ __forceinline__ float plane_d(const float* v, int plane) {
    return plane == 0 ? v[2] : __fsub_rn(v[3], v[2]);      // near: z >= 0;  far: w - z >= 0
}

// Sutherland-Hodgman against one plane.  A vertex with d >= 0 is kept; an edge with one endpoint strictly inside and the
// other strictly outside adds the intersection, computed from the inside endpoint towards the outside one (shared edges of
// two triangles give bit-identical vertices).
__device__ __forceinline__ void clip_pass(const Poly& in, Poly& out, int plane) {
    out.n = 0;
    for (int i = 0; i < in.n; i++) {
        const int j = i + 1 == in.n ? 0 : i + 1;
        const float di = plane_d(in.c[i], plane), dj = plane_d(in.c[j], plane);
        if (di >= 0.0f) {
            for (int k = 0; k < NC; k++) out.c[out.n][k] = in.c[i][k];
            out.n++;
        }
        if ((di > 0.0f && dj < 0.0f) || (di < 0.0f && dj > 0.0f)) {
            const float* I = di > 0.0f ? in.c[i] : in.c[j];
            const float* O = di > 0.0f ? in.c[j] : in.c[i];
            const float dI = di > 0.0f ? di : dj, dO = di > 0.0f ? dj : di;
            const float t = __fdiv_rn(dI, __fsub_rn(dI, dO));
            for (int k = 0; k < NC; k++) out.c[out.n][k] = __fadd_rn(I[k], __fmul_rn(t, __fsub_rn(O[k], I[k])));
            out.n++;
        }
    }
}

// The submitted triangle v of the frame: its stream slot and transform.
struct Source {
    int64_t slot;
    float4x4 m;
};

__device__ __forceinline__ Source source_of(const ClipPrep& p, int64_t v) {
    Source s;
    int64_t prim = v;
    const float* m = p.m;
    if (p.items) {
        // the item that holds order number v: the last one whose vbase is <= v (an empty item shares its vbase with the next)
        int lo = 0, hi = p.nitems - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.items[mid].vbase <= (uint32_t)v) lo = mid; else hi = mid - 1;
        }
        const ListItem& it = p.items[lo];
        prim = (int64_t)it.first + (v - (int64_t)it.vbase);
        m = it.m;
    }
    s.slot = p.src_reordered ? (int64_t)p.src_inv[prim] : prim;
    for (int c = 0; c < 4; c++) s.m.columns[c] = make_float4(m[4 * c + 0], m[4 * c + 1], m[4 * c + 2], m[4 * c + 3]);
    return s;
}

// The three corners of submitted triangle v in clip space (x y z w r g b nx ny nz u v), in registers (constant indices only), and
// how they lie: ok = every clip-space component finite and not all three beyond one plane; inside = all three inside both.
__device__ __forceinline__ void load_corners(const ClipPrep& p, int64_t v, float (&c)[3][NC], bool& ok, bool& inside) {
    const Source src = source_of(p, v);
    bool finite = true, below = true, beyond = true;
    inside = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float4 x = p.src_xyz[3 * src.slot + k];
        const float4 rgb = p.src_rgb[3 * src.slot + k];
        const float4 nrm = p.src_nrm ? p.src_nrm[3 * src.slot + k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const VertexOut vo = vertex_shader(make_float3(x.x, x.y, x.z), make_float3(rgb.x, rgb.y, rgb.z), src.m);
        c[k][0] = vo.pos.x; c[k][1] = vo.pos.y; c[k][2] = vo.pos.z; c[k][3] = vo.pos.w;
        c[k][4] = vo.color.x; c[k][5] = vo.color.y; c[k][6] = vo.color.z;
        c[k][7] = nrm.x; c[k][8] = nrm.y; c[k][9] = nrm.z; c[k][10] = nrm.w; c[k][11] = rgb.w;
#pragma unroll
        for (int j = 0; j < 4; j++) finite = finite && fabsf(c[k][j]) < INFINITY;
        const float dn = c[k][2], df = __fsub_rn(c[k][3], c[k][2]);
        inside = inside && dn >= 0.0f && df >= 0.0f;
        below = below && dn < 0.0f;
        beyond = beyond && df < 0.0f;
    }
    ok = finite && !below && !beyond;
}

// The clip polygon of a triangle that crosses a plane (n = 0: nothing left).  Only these triangles touch the polygon arrays,
// which live in private memory (dynamically indexed).
__device__ __noinline__ void clip_crossing(const float (&c)[3][NC], Poly& out) {
    Poly a, b;
    a.n = 3;
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < NC; j++) a.c[k][j] = c[k][j];
    clip_pass(a, b, 0);
    if (b.n < 3) { out.n = 0; return; }
    clip_pass(b, out, 1);
    if (out.n < 3) out.n = 0;
}

__device__ __forceinline__ uint32_t fan_count(int n) { return n >= 3 ? (uint32_t)(n - 2) : 0u; }

constexpr int CLIP_THREADS = 256;

// exclusive scan of one value per thread over the workgroup (CLIP_THREADS), in LDS; *total = the workgroup's sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* lds, uint32_t* total) {
    const int t = threadIdx.x;
    lds[t] = x;
    __syncthreads();
    for (int off = 1; off < CLIP_THREADS; off <<= 1) {
        const uint32_t y = t >= off ? lds[t - off] : 0u;
        __syncthreads();
        lds[t] += y;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    *total = lds[CLIP_THREADS - 1];
    __syncthreads();
    return incl - x;
}

__global__ __launch_bounds__(CLIP_THREADS) void k_clip_count(ClipPrep p) {
    __shared__ uint32_t lds[CLIP_THREADS];
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t cnt = 0;
    if (v < p.n) {
        float c[3][NC];
        bool ok, inside;
        load_corners(p, v, c, ok, inside);
        if (ok && inside) cnt = 1;
        else if (ok) {
            Poly q;
            clip_crossing(c, q);
            cnt = fan_count(q.n);
        }
    }
    uint32_t total;
    (void)block_excl_scan(cnt, lds, &total);
    if (threadIdx.x == 0) p.sums[blockIdx.x] = total;
}

// sums[0 .. nb) -> exclusive offsets, sums[nb] = the post-clip count (one workgroup of 1024 threads, chunks of ceil(nb / 1024))
__global__ __launch_bounds__(1024) void k_clip_scan(uint32_t* __restrict__ sums, int64_t nb) {
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (nb + 1023) / 1024;
    const int64_t b0 = std::min<int64_t>(nb, t * per), b1 = std::min<int64_t>(nb, b0 + per);
    uint32_t acc = 0;
    for (int64_t b = b0; b < b1; b++) acc += sums[b];
    part[t] = acc;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint32_t y = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += y;
        __syncthreads();
    }
    uint32_t run = part[t] - acc;
    for (int64_t b = b0; b < b1; b++) {
        const uint32_t x = sums[b];
        sums[b] = run;
        run += x;
    }
    if (t == 1023) sums[nb] = part[1023];
}

// The NDC corner of Renderer.swift:161-162 / Shaders.metal:68 (the divide as setup does it), its colour and attributes.
__device__ __forceinline__ void put_corner(const ClipPrep& p, int64_t at, const float* c) {
    p.xyz[at] = make_float4(__fdiv_rn(c[0], c[3]), __fdiv_rn(c[1], c[3]), __fdiv_rn(c[2], c[3]), 1.0f);
    p.rgb[at] = make_float4(c[4], c[5], c[6], c[11]);
    if (p.nrm) p.nrm[at] = make_float4(c[7], c[8], c[9], c[10]);
}

// The perspective table entry of a frame slot (SWR_FLAG_PERSPECTIVE, k_persp_fill): the clip-space w of its three corners — an
// original vertex's own, an intersection's w_I + t (w_O - w_I) — as (q_a, q_b, q_c, bypass).
__device__ __forceinline__ void put_persp(const ClipPrep& p, int64_t slot, float wa, float wb, float wc) {
    const bool bypass = wa == wb && wb == wc;
    p.pq[slot] = make_float4(__fdiv_rn(1.0f, wa), __fdiv_rn(1.0f, wb), __fdiv_rn(1.0f, wc), bypass ? 1.0f : 0.0f);
}

// Fan triangle s of triangle v at slot (= order number) base + s.  A post-clip count above the frame's slots (more crossing
// triangles than the fan capacity) leaves every slot invalid — the frame is rastered empty — and reports the count to the host
// (ClipPrep::over), which grows the capacity and redraws, as for a bin overflow.
__global__ __launch_bounds__(CLIP_THREADS) void k_clip_emit(ClipPrep p) {
    __shared__ uint32_t lds[CLIP_THREADS];
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nb = (p.n + CLIP_THREADS - 1) / CLIP_THREADS;
    const int64_t total = p.sums[nb];
    const bool over = total > p.bound;
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.over) *p.over = over ? (uint32_t)total : 0u;
    // slots beyond the post-clip count: one NaN corner makes setup skip the slot
    const float nan = quiet_nan();
    for (int64_t s = (over ? 0 : total) + v; s < p.bound; s += (int64_t)gridDim.x * blockDim.x) p.xyz[3 * s] = make_float4(nan, nan, nan, 1.0f);
    float c[3][NC];
    bool ok = false, inside = false;
    if (v < p.n) load_corners(p, v, c, ok, inside);
    Poly q;
    q.n = 0;
    uint32_t cnt = 0;
    if (ok && inside) cnt = 1;
    else if (ok) {
        clip_crossing(c, q);
        cnt = fan_count(q.n);
    }
    uint32_t wg_total;
    const int64_t base = (int64_t)p.sums[blockIdx.x] + block_excl_scan(cnt, lds, &wg_total);     // the order number of fan triangle 0
    if (!cnt || over) return;
    if (inside) {                     // the triangle as it is, straight from registers
#pragma unroll
        for (int k = 0; k < 3; k++) put_corner(p, 3 * base + k, c[k]);
        p.map[base] = (uint32_t)v;
        if (p.pq) put_persp(p, base, c[0][3], c[1][3], c[2][3]);
        return;
    }
    for (uint32_t s = 0; s < cnt; s++) {
        const int64_t slot = base + s;
        put_corner(p, 3 * slot + 0, q.c[0]);          // the fan (P0, Pk, Pk+1)
        put_corner(p, 3 * slot + 1, q.c[s + 1]);
        put_corner(p, 3 * slot + 2, q.c[s + 2]);
        p.map[slot] = (uint32_t)v;
        if (p.pq) put_persp(p, slot, q.c[0][3], q.c[s + 1][3], q.c[s + 2][3]);
    }
}

// One wave per 64-slot group: the box of its slots below the post-clip count (NaN if a coordinate is not finite: never
// culled); a group with none gets a box far right of every band, so the binning kernels skip it without reading it.
__global__ __launch_bounds__(256) void k_clip_box(ClipPrep p) {
    const int64_t groups = (p.bound + 63) / 64;
    const int64_t g = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (g >= groups) return;
    int64_t total = p.sums[(p.n + CLIP_THREADS - 1) / CLIP_THREADS];
    if (total > p.bound) total = 0;                  // (an overflowed frame: every slot invalid)
    const int64_t s = g * 64 + (threadIdx.x & 63);
    GroupBox b = box_start();
    if (s < total) {
        for (int k = 0; k < 3; k++) box_fold(b, p.xyz[3 * s + k]);
    }
    const bool poisoned = box_reduce(b);
    if ((threadIdx.x & 63) == 0) {
        if (!poisoned && g * 64 >= total) {      // NDC x = 4: 1.5 widths right of the image
            b.lo[0] = b.hi[0] = 4.0f; b.lo[1] = b.hi[1] = 0.0f; b.lo[2] = b.hi[2] = 0.5f;
        }
        box_store(b, p.box + 2 * g);
    }
}

__global__ __launch_bounds__(256) void k_clip_ids(uint32_t* __restrict__ ids, int64_t npix, const uint32_t* __restrict__ map, int64_t bound) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
        const uint32_t id = ids[i];
        if (id != SWR_ID_NONE) ids[i] = (int64_t)id < bound ? map[id] : SWR_ID_NONE;
    }
}

}  // namespace

void launch_clip_prep(const DeviceFrame& f, hipStream_t s) {
    const ClipPrep& p = f.clip;
    if (p.bound <= 0 || p.n <= 0) return;
    const int64_t nb = (p.n + CLIP_THREADS - 1) / CLIP_THREADS;
    hipLaunchKernelGGL(k_clip_count, dim3((unsigned)nb), dim3(CLIP_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_clip_scan, dim3(1), dim3(1024), 0, s, p.sums, nb);
    if (p.count_only) return;
    hipLaunchKernelGGL(k_clip_emit, dim3((unsigned)nb), dim3(CLIP_THREADS), 0, s, p);
    const int64_t groups = (p.bound + 63) / 64;
    hipLaunchKernelGGL(k_clip_box, dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, s, p);
}

bool launch_clip_ids(const DeviceFrame& f, hipStream_t s, hipEvent_t stop) {
    const int64_t npix = (int64_t)f.tg.width * (int64_t)(f.tg.row_end - f.tg.row_begin);
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (npix + 255) / 256));
    return launch_on(stop, k_clip_ids, dim3(blocks), dim3(256), 0, s, f.ids, npix, (const uint32_t*)f.clip.map, f.clip.bound);
}

}  // namespace swr
