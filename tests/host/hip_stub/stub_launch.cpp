// Stand-ins for every kernel launch wrapper of swr_internal.h on the fake HIP runtime: the one set every host test program links.
// The frame launches (swr_kernels.hip / swr_upload.hip) enqueue host lambdas that leave what the host layer looks at afterwards
// (pair totals, largest fill, a frame tag in the framebuffer) and touch both ends of every table their DeviceFrame names, at the sizes
// swr_internal.h gives.  The feature launches (resolve, visibility counts, depth queries, delta reads, skin, morph, item bounds,
// dual-quaternion skin, sparse morph, computed normals, ray casts) are plain CPU loops over the header's arithmetic that read and write
// every element of every array they are handed; the sparse morph checks its rows, the normals launches note when they were called
// relative to the others, and the ray launch answers with an echo of its rays.  Either way a buffer the host layer sized too small is
// an out-of-bounds access the address sanitizer reports.  stub_launch.h holds what the programs observe.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "stub_launch.h"

std::atomic<uint32_t> g_count_total{0};
std::atomic<int> g_count_launches{0}, g_query_launches{0}, g_compares{0}, g_directs{0}, g_packs{0};
std::atomic<int> g_vertex_launches{0}, g_stream_launches{0}, g_morph_launches{0}, g_morph_nrm_launches{0};
std::atomic<int> g_bounds_launches{0}, g_dq_launches{0}, g_dq_nrm_launches{0};
std::atomic<int> g_sparse_launches{0}, g_sparse_nrm_launches{0};
std::atomic<int64_t> g_sparse_rows{0};
std::atomic<int> g_face_launches{0}, g_vnrm_launches{0}, g_flat_launches{0}, g_flip_launches{0}, g_ray_launches{0};
std::atomic<int> g_launch_fails{0};

std::mutex g_note_m;
LaunchCounts g_face_at{}, g_flat_at{};
int g_vnrm_after_faces = 0;
std::vector<FlatNote> g_flat_notes;
std::vector<uint32_t> g_adj_off, g_adj_tri;
static std::vector<RayNote> g_ray_notes;
std::vector<RayNote> take_ray_notes() {
    std::lock_guard<std::mutex> lk(g_note_m);
    std::vector<RayNote> out;
    out.swap(g_ray_notes);
    return out;
}
static std::atomic<uint32_t> g_sink{0};     // what the ray launch's reads add up to (so that no read is optimised away)

static std::mutex g_records_m;
static std::vector<Record> g_records;
std::vector<Record> take_records() {
    std::lock_guard<std::mutex> lk(g_records_m);
    std::vector<Record> r;
    r.swap(g_records);
    return r;
}

namespace swr {
std::atomic<uint32_t> g_fake_fill{7};        // largest tile fill the fake k_bin reports (tests raise it to force a regrow)
std::atomic<uint32_t> g_fake_pairs{1000};
std::atomic<uint32_t> g_fake_clip_over{0};   // != 0: the next clip frame's raster reports this many triangles beyond its slots, once

namespace {
// first and last element of a table: written (tables the kernels fill) or read (tables they are given)
template <class T> void ends(T* p, int64_t n) { if (p && n > 0) { p[0] = T{}; p[n - 1] = T{}; } }
template <class T> void ends(const T* p, int64_t n) {
    if (!p || n <= 0) return;
    const volatile unsigned char* b = (const volatile unsigned char*)p;
    (void)b[0]; (void)b[(size_t)n * sizeof(T) - 1];
}
// what the binning launch of a frame (clip pre-pass, list gather, perspective table, binning) may write
void touch_binning(const DeviceFrame& f) {
    const int64_t tiles = (int64_t)f.tg.tiles_x * f.tg.tiles_y;
    const ClipPrep& p = f.clip;
    if (p.bound > 0) {
        ends(p.items, p.nitems);
        ends(p.xyz, 3 * p.bound); ends(p.rgb, 3 * p.bound); ends(p.nrm, 3 * p.bound);
        ends(p.map, p.bound); ends(p.box, 2 * ((p.bound + 63) / 64)); ends(p.sums, (p.n + 255) / 256 + 1);
        ends(p.pq, p.bound);
    }
    ends(f.items, f.nitems);
    ends(f.gather.inv_out, f.ntri); ends(f.gather.rgb_out, 3 * f.ntri); ends(f.gather.nrm_out, 3 * f.ntri);
    ends(f.pq, f.ntri);
    ends(f.geo, f.ntri); ends(f.geo_full, f.ntri); ends(f.ranges, f.ntri);
    ends(f.bins, f.fixed_bins ? tiles * (int64_t)f.cap_tile : (int64_t)f.capacity);
    if (f.fixed_bins) ends(f.fill, CNT_WORDS + tiles);
    else if (f.plan.use_lds) ends(f.bin_matrix, (int64_t)f.plan.G * tiles);
}
// the tag of a frame: transform[0] of swr_draw, of a draw list's first item, of what a clip frame was submitted with
float frame_tag(const DeviceFrame& f) {
    if (f.clip.bound > 0) return (f.clip.items && f.clip.nitems > 0) ? f.clip.items[0].m[0] : f.clip.m[0];
    return (f.items && f.nitems > 0) ? f.items[0].m[0] : f.m[0];
}
}  // namespace

int live_groups_per_workgroup(int64_t ntri, int G) { return (int)(((ntri + 63) / 64 + G - 1) / (G > 0 ? G : 1)); }
BinPlan plan_binning(int64_t ntri, int ntiles, bool force_atomic) {
    BinPlan p{};
    p.use_lds = !force_atomic; p.threads = 256; p.G = (int)std::max<int64_t>(1, std::min<int64_t>(256, (ntri + 255) / 256));
    p.chunk = (int)((ntri + p.G - 1) / p.G); p.lds_bytes = (size_t)ntiles * 4;
    return p;
}
uint32_t fixed_cap_max(int64_t ntri, int ntiles) { return (ntri <= 0 || ntiles <= 0) ? 0u : 61440u; }
hipError_t prepare_device() { return hipSuccess; }
size_t stream_sort_temp_bytes(int64_t) { return 64; }

void launch_validate_indices(const int64_t* idx, int64_t n, int64_t nv, uint32_t* counters, hipStream_t s) {
    fake_enqueue(s, [=] { for (int64_t i = 0; i < n; i++) if (idx[i] < 0 || idx[i] >= nv) counters[CNT_BAD_INDEX] = 1u; });
}
hipError_t launch_build_stream(const StreamBuild&, hipStream_t s) { fake_enqueue(s, nullptr); return hipSuccess; }
hipError_t launch_build_stream_range(const StreamBuild&, int64_t, int64_t, hipStream_t s) { fake_enqueue(s, nullptr); return hipSuccess; }
void launch_gather_attrs(const swr_vertex_attr*, int64_t, const int64_t*, int64_t, const float4*, float4*, float4*, hipStream_t s) { fake_enqueue(s, nullptr); }
void launch_texture_to_float(const uint32_t*, int64_t, float4*, hipStream_t s) { fake_enqueue(s, nullptr); }

bool launch_bin(const DeviceFrame& f, hipStream_t s, hipEvent_t stop) {
    const DeviceFrame ff = f;
    fake_enqueue(s, [ff] {
        const int ntiles = ff.tg.tiles_x * ff.tg.tiles_y;
        touch_binning(ff);
        memset(ff.fill_next, 0, (size_t)(CNT_WORDS + ntiles) * 4);
        ff.fill[CNT_PAIRS] = g_fake_pairs.load();
        ff.fill[3] = g_fake_fill.load();                    // CNT_MAXFILL
    }, stop, "k_bin", (size_t)ff.plan.G);
    return stop != nullptr;
}
void launch_setup_bin(const DeviceFrame& f, hipStream_t s) {
    const DeviceFrame ff = f;
    fake_enqueue(s, [ff] { touch_binning(ff); }, nullptr, "k_setup", (size_t)ff.plan.G);
}
void launch_scan(const DeviceFrame&, hipStream_t) {}
bool launch_fill(const DeviceFrame& f, hipStream_t s, hipEvent_t stop) {
    const DeviceFrame ff = f;
    fake_enqueue(s, [ff] { ff.counters[CNT_PAIRS] = g_fake_pairs.load(); *ff.host_counters = g_fake_pairs.load(); if (ff.host_max) __atomic_store_n(ff.host_max, g_fake_fill.load(), __ATOMIC_RELAXED); }, stop, "k_fill", (size_t)ff.plan.G);
    return stop != nullptr;
}
bool launch_sort_bins(const DeviceFrame& f, hipStream_t s, hipEvent_t stop) {
    if (f.skip_sort) return false;
    fake_enqueue(s, nullptr, stop, "k_sort_bins");
    return stop != nullptr;
}
bool frame_uses_k32(const DeviceFrame& f) {
    return f.k32 && (f.flags & SWR_FLAG_DEPTH_TEST) && (f.flags & SWR_FLAG_NO_COLOR) && !(f.flags & SWR_FLAG_METAL_RULES);
}
bool launch_raster(const DeviceFrame& f, hipStream_t s, hipEvent_t stop) {
    const DeviceFrame ff = f;
    if (ff.tg.tiles_x * ff.tg.tiles_y == 0) return false;
    fake_enqueue(s, [ff] {
        bool overflow;
        if (ff.fixed_bins) {
            *ff.host_counters = ff.fill[CNT_PAIRS]; *ff.host_fill = ff.fill[3]; if (ff.host_max) __atomic_store_n(ff.host_max, ff.fill[3], __ATOMIC_RELAXED);
            overflow = ff.fill[3] > ff.cap_tile;
        } else overflow = ff.counters[CNT_PAIRS] > ff.capacity;
        if (ff.clip.bound > 0) {
            const uint32_t over = g_fake_clip_over.exchange(0);
            if (over) { *ff.clip.over = (uint32_t)ff.clip.bound + over; overflow = true; }
        }
        // the "image": every pixel of the band carries the frame's tag; an overflowed frame is rastered empty
        const size_t n = (size_t)ff.tg.width * (size_t)(ff.tg.row_end - ff.tg.row_begin);
        const float tag = overflow ? -1.0f : frame_tag(ff);
        for (size_t i = 0; i < n; i++) ff.depth[i] = tag;
        if (ff.color && !(ff.flags & SWR_FLAG_NO_COLOR)) memset(ff.color, (int)tag & 0xFF, n * 4);
        ends(ff.ids, (int64_t)n);
    }, stop, "k_raster", (size_t)ff.ntri);
    return stop != nullptr;
}
void launch_points_or_lines(const DeviceFrame& f, int, hipStream_t s) {
    const DeviceFrame ff = f;
    fake_enqueue(s, [ff] {
        const size_t n = (size_t)ff.tg.width * (size_t)(ff.tg.row_end - ff.tg.row_begin);
        for (size_t i = 0; i < n; i++) ff.depth[i] = ff.m[0];
    }, nullptr, "k_points_or_lines");
}

// ---- the feature launches ------------------------------------------------------------------------------------------------------

void launch_resolve(const void* color, const void* depth, void* color_out, void* depth_out, int width, int rows, int factor,
                    int depth_filter, hipStream_t s) {
    fake_enqueue(s, [=] {
        const int S = factor, w = width / S, h = rows / S;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t at = (size_t)y * S * width + (size_t)x * S;
                if (color) ((uint32_t*)color_out)[(size_t)y * w + x] = resolve_box((const uint32_t*)color + at, width, S);
                if (depth) ((float*)depth_out)[(size_t)y * w + x] = depth_filter == SWR_RESOLVE_DEPTH_MIN ? resolve_minimum((const float*)depth + at, width, S)
                                                                                                              : ((const float*)depth)[at];
            }
    }, nullptr, "k_resolve");
}

// The stand-in raster leaves the ID image at zero, so the loop ADDS a pattern of its own to what it reads.  The band's rows are read,
// the counters are added to, never assigned (a buffer that was not zeroed shows), and counters[n] is written.
void launch_count_ids(const uint32_t* ids, int width, int x0, int x1, int y0, int y1, int per_item, const ListItem* items,
                      uint32_t* counters, int64_t n, hipStream_t s) {
    g_count_launches++;
    fake_enqueue(s, [=] {
        const uint32_t total = g_count_total.load();
        for (int y = y0; y < y1; y++)
            for (int x = x0; x < x1; x++) {
                uint32_t id = ids[(size_t)y * width + x] + count_pattern((uint32_t)x, (uint32_t)y, total);
                int64_t slot = n;
                if (id != SWR_ID_NONE) {
                    if (!per_item) slot = id;
                    else if (!items) slot = 0;
                    else { slot = 0; for (int64_t k = 0; k < n; k++) if (items[k].vbase <= id) slot = k; }
                }
                counters[slot] += 1;
            }
    }, nullptr, "k_count_ids");
}

// (the loop also checks what the host hands it next to the boxes: the list of large boxes and the total area of the band's parts)
void launch_depth_query(const float* depth, int width, int rows, int row_begin, const swr_depth_box* boxes, int64_t n,
                        const uint32_t* large, int64_t nlarge, uint64_t total_area, void* scratch, uint32_t* passed, hipStream_t s) {
    g_query_launches++;
    fake_enqueue(s, [=] {
        uint64_t area = 0;
        int64_t seen_large = 0;
        memset(scratch, 0x5A, depth_query_scratch_bytes(width, rows));      // (a summary sized too small is reported)
        for (int64_t k = 0; k < n; k++) {
            const swr_depth_box b = boxes[k];
            const int y0 = std::max(b.y0, row_begin) - row_begin, y1 = std::min(b.y1, row_begin + rows) - row_begin;
            uint32_t cnt = 0;
            for (int y = y0; y < y1; y++)
                for (int x = b.x0; x < b.x1; x++) cnt += b.z < depth[(size_t)y * width + x] ? 1u : 0u;
            passed[k] = cnt;
            const uint64_t part = (y1 > y0 && b.x1 > b.x0) ? (uint64_t)(y1 - y0) * (uint64_t)(b.x1 - b.x0) : 0;
            area += part;
            if (part >= swr::DEPTH_QUERY_SPLIT_AREA) {
                if (seen_large >= nlarge || large[seen_large] != (uint32_t)k) g_launch_fails++;
                seen_large++;
            }
        }
        if (area != total_area || seen_large != nlarge) g_launch_fails++;
    }, nullptr, "k_depth_boxes");
}

void launch_delta(const uint32_t* cur, uint32_t* base, int have_base, int width, int rows, uint32_t* flags, uint32_t* direct, hipStream_t s) {
    g_compares++;
    if (direct) g_directs++;
    fake_enqueue(s, [=] {
        const int tx_n = (width + 63) / 64, ty_n = (rows + 31) / 32;
        for (int ty = 0; ty < ty_n; ty++)
            for (int tx = 0; tx < tx_n; tx++) {
                const int x0 = tx * 64, x1 = std::min(width, x0 + 64), y0 = ty * 32, y1 = std::min(rows, y0 + 32);
                bool changed = !have_base;
                for (int y = y0; y < y1 && !changed; y++)
                    changed = memcmp(cur + (size_t)y * width + x0, base + (size_t)y * width + x0, (size_t)(x1 - x0) * 4) != 0;
                flags[(size_t)ty * tx_n + tx] = changed ? 1u : 0u;
                if (!changed) continue;
                for (int y = y0; y < y1; y++) {
                    memcpy(base + (size_t)y * width + x0, cur + (size_t)y * width + x0, (size_t)(x1 - x0) * 4);
                    if (direct) memcpy(direct + (size_t)y * width + x0, cur + (size_t)y * width + x0, (size_t)(x1 - x0) * 4);
                }
            }
    }, nullptr, "k_delta_tiles");
}
void launch_delta_pack(const uint32_t* src, int width, int x0, int x1, int y0, int y1, uint32_t* out, hipStream_t s) {
    g_packs++;
    fake_enqueue(s, [=] {
        for (int y = y0; y < y1; y++) memcpy(out + (size_t)(y - y0) * (x1 - x0), src + (size_t)y * width + x0, (size_t)(x1 - x0) * 4);
    }, nullptr, "k_delta_pack");
}

void launch_morph_vertices(const swr_vertex* vertices, const swr_vertex_attr* attrs, int64_t nv, const float* dpos, const float* dnrm,
                           const MorphEntry* list, int32_t active, swr_vertex* morphed, swr_vertex_attr* morphed_attrs, hipStream_t s) {
    g_morph_launches++;
    if (attrs) g_morph_nrm_launches++;
    fake_enqueue(s, [=] {
        const size_t F = SWR_TUNE_MORPH_PAD ? 4 : 3;
        if (active < 1 || active > SWR_MORPH_MAX_TARGETS) { std::printf("FAIL %d active targets\n", active); g_launch_fails++; return; }
        for (int k = 0; k < active; k++)
            if (list[k].weight == 0.0f || (k && list[k].target <= list[k - 1].target) || list[k].target >= SWR_MORPH_MAX_TARGETS) {
                std::printf("FAIL active list entry %d: target %u weight %g\n", k, list[k].target, list[k].weight); g_launch_fails++; return;
            }
        for (int64_t i = 0; i < nv; i++) {
            morphed[i] = vertices[i];
            if (attrs) morphed_attrs[i] = attrs[i];
            for (int k = 0; k < active; k++) {
                const float w = list[k].weight;
                const float* d = dpos + ((size_t)list[k].target * (size_t)nv + (size_t)i) * F;
                for (int c = 0; c < 3; c++) { const float m = w * d[c]; morphed[i].xyz[c] = morphed[i].xyz[c] + m; }
                if (attrs) {
                    const float* e = dnrm + ((size_t)list[k].target * (size_t)nv + (size_t)i) * F;
                    for (int c = 0; c < 3; c++) { const float m = w * e[c]; morphed_attrs[i].normal[c] = morphed_attrs[i].normal[c] + m; }
                }
            }
        }
    }, nullptr, "k_morph_vertices", (size_t)nv);
}
void launch_skin_vertices(const swr_vertex* vertices, const swr_vertex_attr* attrs, const swr_skin_vertex* skin, int64_t nv,
                          const float* joints, int32_t joint_count, swr_vertex* posed, float4* posed_nrm, hipStream_t s) {
    g_vertex_launches++;
    fake_enqueue(s, [=] {
        for (int64_t i = 0; i < nv; i++) {
            for (int k = 0; k < 4; k++) if ((int64_t)skin[i].joint[k] >= joint_count) { std::printf("FAIL joint %u of %d\n", skin[i].joint[k], joint_count); g_launch_fails++; return; }
            posed[i] = vertices[i];
            blend(vertices[i].xyz, skin[i], joints, true, posed[i].xyz);
            if (attrs) { float n[3]; blend(attrs[i].normal, skin[i], joints, false, n); posed_nrm[i] = make_float4(n[0], n[1], n[2], 0.0f); }
        }
    }, nullptr, "k_skin_vertices", (size_t)nv);
}
void launch_skin_stream(const float4* pos, int pos_stride, const float4* nrm, int nrm_stride, int64_t nv, const int64_t* indices,
                        int64_t ntri, int reordered, float4* tri_xyz, float4* tri_nrm, float4* box64, hipStream_t s) {
    g_stream_launches++;
    fake_enqueue(s, [=] {
        (void)reordered;                    // (the fake upload builds no stream: slot s holds primitive s)
        for (int64_t g = 0; g < (ntri + 63) / 64; g++) {
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int64_t t = g * 64; t < std::min(ntri, g * 64 + 64); t++)
                for (int k = 0; k < 3; k++) {
                    const int64_t ix = indices[3 * t + k];
                    if (ix < 0 || ix >= nv) { std::printf("FAIL index\n"); g_launch_fails++; return; }
                    const float4 x = pos[(size_t)pos_stride * ix];
                    float4& o = tri_xyz[3 * t + k];
                    o.x = x.x; o.y = x.y; o.z = x.z;
                    if (nrm) { const float4 n = nrm[(size_t)nrm_stride * ix]; float4& q = tri_nrm[3 * t + k]; q.x = n.x; q.y = n.y; q.z = n.z; }
                    const float c[3] = {x.x, x.y, x.z};
                    for (int j = 0; j < 3; j++) { lo[j] = std::min(lo[j], c[j]); hi[j] = std::max(hi[j], c[j]); }
                }
            box64[2 * g] = make_float4(lo[0], lo[1], lo[2], 0);
            box64[2 * g + 1] = make_float4(hi[0], hi[1], hi[2], 0);
        }
        std::lock_guard<std::mutex> lk(g_records_m);
        g_records.push_back(Record{tri_xyz, tri_nrm, box64, ntri, nrm != nullptr});
    }, nullptr, "k_skin_stream", (size_t)ntri);
}

// (also checks what the host resolved: the work units and the ranges)
void launch_item_bounds(const ItemBoundsArgs& a, hipStream_t s) {
    g_bounds_launches++;
    fake_enqueue(s, [a] {
        int64_t units = 0;
        memset(a.scratch, 0x5A, item_bounds_scratch_bytes(a.n));            // (partial records sized too small are reported)
        for (int32_t k = 0; k < a.n; k++) {
            const ListItem& it = a.items[k];
            if (it.ubase != (uint32_t)units) { std::printf("FAIL item %d: ubase %u, not %lld\n", (int)k, it.ubase, (long long)units); g_launch_fails++; }
            units += item_bounds_units(it.count);
            memset(&a.records[k], 0xA5, sizeof(swr_item_bound));             // (every word of every record is the launch's to write)
            const float4* tri = a.tri_xyz + 3 * (size_t)it.first;
            a.records[k] = fold((int64_t)it.count, [tri](int64_t t, int j) { return &tri[3 * t + j].x; }, it.m, a.width, a.height, a.metal != 0);
        }
        if (units != a.units) { std::printf("FAIL %lld units handed, the items have %lld\n", (long long)a.units, (long long)units); g_launch_fails++; }
        if (a.n < 1 || a.n > SWR_DRAW_LIST_MAX || !a.vertices || !a.indices) g_launch_fails++;
    }, nullptr, "k_item_bounds", (size_t)a.units);
}

// (also checks the table it is handed: its alignment, its size, the joint range of the skin)
void launch_skin_vertices_dq(const swr_vertex* vertices, const swr_vertex_attr* attrs, const swr_skin_vertex* skin, int64_t nv,
                             const float* dual_quats, int32_t joint_count, swr_vertex* posed, float4* posed_nrm, hipStream_t s) {
    g_dq_launches++;
    if (attrs) g_dq_nrm_launches++;
    fake_enqueue(s, [=] {
        if (joint_count < 1 || joint_count > SWR_SKIN_MAX_JOINTS || ((uintptr_t)dual_quats & 15)) { std::printf("FAIL table of %d joints\n", joint_count); g_launch_fails++; return; }
        float sum = 0.0f;
        for (int64_t k = 0; k < 8 * (int64_t)joint_count; k++) sum += dual_quats[k];       // (the whole table is the launch's to read)
        if (sum == 12345.678f) g_launch_fails++;
        for (int64_t i = 0; i < nv; i++) {
            for (int k = 0; k < 4; k++) if ((int64_t)skin[i].joint[k] >= joint_count) { std::printf("FAIL joint %u of %d\n", skin[i].joint[k], joint_count); g_launch_fails++; return; }
            posed[i] = vertices[i];
            pose_dq(vertices[i].xyz, skin[i], dual_quats, true, posed[i].xyz);
            if (attrs) { float n[3]; pose_dq(attrs[i].normal, skin[i], dual_quats, false, n); posed_nrm[i] = make_float4(n[0], n[1], n[2], 0.0f); }
        }
    }, nullptr, "k_skin_vertices_dq", (size_t)nv);
}

// (also checks the rows it is handed; like the kernel it writes the position and normal quads of the touched vertices only:
// everything else of the morphed arrays is the host layer's pre-fill)
void launch_morph_sparse(const MorphSparseArgs& a, hipStream_t s) {
    g_sparse_launches++;
    if (a.attrs) g_sparse_nrm_launches++;
    g_sparse_rows.store(a.touched_count);
    const MorphSparseArgs b = a;
    fake_enqueue(s, [b] {
        auto bad = [](const char* what, long long x) { std::printf("FAIL sparse launch: %s %lld\n", what, x); g_launch_fails++; };
        if (b.touched_count < 1) return bad("touched_count", b.touched_count);
        if (b.targets < 1 || b.targets > SWR_MORPH_MAX_TARGETS) return bad("targets", b.targets);
        if (b.row[0] != 0) return bad("row[0]", b.row[0]);
        if ((b.attrs != nullptr) != (b.dnrm != nullptr) || (b.attrs != nullptr) != (b.morphed_attrs != nullptr)) return bad("normal arrays", 0);
        float sum = 0.0f;
        for (int t = 0; t < b.targets; t++) sum += b.weights[t] == b.weights[t] ? b.weights[t] : 0.0f;     // (the whole table is read)
        if (sum == 12345.678f) g_launch_fails++;
        for (int64_t r = 0; r < b.touched_count; r++) {
            const int64_t i = b.touched[r];
            if (r && b.touched[r] <= b.touched[r - 1]) return bad("touched not ascending at row", r);
            if (b.row[r + 1] <= b.row[r]) return bad("an empty or negative row", r);
            float p[4], n[4] = {0, 0, 0, 0};
            memcpy(p, b.vertices[i].xyz, 16);
            if (b.attrs) memcpy(n, b.attrs[i].normal, 16);
            for (int64_t k = b.row[r]; k < b.row[r + 1]; k++) {
                const MorphSparseEntry e = b.dpos[k];
                if (e.target >= (uint32_t)b.targets || (k > b.row[r] && e.target <= b.dpos[k - 1].target)) return bad("row not sorted by target at entry", k);
                if (b.dnrm && b.dnrm[k].target != e.target) return bad("normal entry of another target at", k);
                const float w = b.weights[e.target];
                if (!(w != 0.0f)) continue;
                const float d[3] = {e.dx, e.dy, e.dz};
                for (int c = 0; c < 3; c++) { const float m = w * d[c]; p[c] = p[c] + m; }
                if (b.dnrm) {
                    const float f[3] = {b.dnrm[k].dx, b.dnrm[k].dy, b.dnrm[k].dz};
                    for (int c = 0; c < 3; c++) { const float m = w * f[c]; n[c] = n[c] + m; }
                }
            }
            memcpy(b.morphed[i].xyz, p, 16);
            if (b.attrs) memcpy(b.morphed_attrs[i].normal, n, 16);
        }
    }, nullptr, "k_morph_sparse", (size_t)b.touched_count);
}

// (the normals launches note what had been launched when they were made, and the adjacency and the stream arrays they were handed)
void launch_face_normals(const float4* pos, int pos_stride, int64_t nv, const int64_t* indices, int64_t ntri, bool flip, float4* face,
                         hipStream_t s) {
    if (ntri <= 0) return;          // (as the launches themselves: a zero grid is a launch error)
    { std::lock_guard<std::mutex> lk(g_note_m); g_face_at = launch_counts(); }
    g_face_launches++;
    if (flip) g_flip_launches++;
    fake_enqueue(s, [=] {
        if (pos_stride != 2 || ntri < 1) { std::printf("FAIL face launch: stride %d, %lld triangles\n", pos_stride, (long long)ntri); g_launch_fails++; return; }
        for (int64_t p = 0; p < ntri; p++) {
            const float4* x[3];
            for (int k = 0; k < 3; k++) {
                const int64_t ix = indices[3 * p + k];
                if (ix < 0 || ix >= nv) { std::printf("FAIL face launch: index\n"); g_launch_fails++; return; }
                x[k] = pos + (size_t)pos_stride * ix;
            }
            float f[3];
            face_of(&x[0]->x, &x[1]->x, &x[2]->x, flip, f);
            face[p] = make_float4(f[0], f[1], f[2], 0.0f);
        }
    }, nullptr, "k_face_normals", (size_t)ntri);
}
void launch_vertex_normals(const uint32_t* adj_off, const uint32_t* adj_tri, const float4* face, int64_t nv, float4* auto_nrm, hipStream_t s) {
    if (nv <= 0) return;
    { std::lock_guard<std::mutex> lk(g_note_m); g_vnrm_after_faces = g_face_launches.load(); }
    g_vnrm_launches++;
    fake_enqueue(s, [=] {
        if (adj_off[0] != 0) { std::printf("FAIL vertex normals: adj_off[0] = %u\n", adj_off[0]); g_launch_fails++; return; }
        for (int64_t i = 0; i < nv; i++) {
            if (adj_off[i + 1] < adj_off[i]) { std::printf("FAIL vertex normals: row %lld\n", (long long)i); g_launch_fails++; return; }
            float n[3] = {0.0f, 0.0f, 0.0f};
            for (uint32_t e = adj_off[i]; e < adj_off[i + 1]; e++) {
                const float4 f = face[adj_tri[e]];
                n[0] = n[0] + f.x; n[1] = n[1] + f.y; n[2] = n[2] + f.z;
            }
            normalise(n);
            auto_nrm[i] = make_float4(n[0], n[1], n[2], 0.0f);
        }
        std::lock_guard<std::mutex> lk(g_note_m);
        g_adj_off.assign(adj_off, adj_off + nv + 1);
        g_adj_tri.assign(adj_tri, adj_tri + adj_off[nv]);
    }, nullptr, "k_vertex_normals", (size_t)nv);
}
void launch_flat_normals(const float4* tri_xyz, int64_t ntri, bool flip, float4* tri_nrm, hipStream_t s) {
    if (ntri <= 0) return;
    { std::lock_guard<std::mutex> lk(g_note_m); g_flat_at = launch_counts(); }
    g_flat_launches++;
    if (flip) g_flip_launches++;
    fake_enqueue(s, [=] {
        for (int64_t t = 0; t < ntri; t++) {
            float f[3];
            face_of(&tri_xyz[3 * t].x, &tri_xyz[3 * t + 1].x, &tri_xyz[3 * t + 2].x, flip, f);
            for (int k = 0; k < 3; k++) { float4& q = tri_nrm[3 * t + k]; q.x = f[0]; q.y = f[1]; q.z = f[2]; }
        }
        std::lock_guard<std::mutex> lk(g_note_m);
        g_flat_notes.push_back(FlatNote{tri_xyz, tri_nrm});
    }, nullptr, "k_flat_normals", (size_t)ntri);
}

// (reads every ray, every stream slot, every group box and, when the stream is reordered, every inv entry it is handed, writes every
// key word and every hit, and notes what it was handed and when; its hits echo the rays)
void launch_cast_rays(const RaysArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    g_ray_launches++;
    size_t at;
    {
        std::lock_guard<std::mutex> lk(g_note_m);
        at = g_ray_notes.size();
        g_ray_notes.push_back(RayNote{a, g_stream_launches.load(), false});
    }
    const RaysArgs b = a;
    fake_enqueue(s, [b, at] {
        if (b.n > SWR_RAYS_MAX || b.groups != (b.ntri + 63) / 64 || !b.rays || !b.keys || !b.hits) {
            std::printf("FAIL ray launch: n %lld ntri %lld groups %lld\n", (long long)b.n, (long long)b.ntri, (long long)b.groups); g_launch_fails++; return;
        }
        uint32_t sum = 0;
        for (int64_t e = 0; e < 3 * b.ntri; e++) sum += float_bits(b.tri_xyz[e].x) + float_bits(b.tri_xyz[e].w);
        for (int64_t g = 0; g < 2 * b.groups; g++) sum += float_bits(b.box64[g].x) + float_bits(b.box64[g].z);
        if (b.reordered) for (int64_t p = 0; p < b.ntri; p++) sum += b.inv[p];
        g_sink += sum;
        for (int64_t k = 0; k < b.n; k++) {
            const swr_ray r = b.rays[k];
            const float f[8] = {r.origin[0], r.origin[1], r.origin[2], r.tmin, r.dir[0], r.dir[1], r.dir[2], r.tmax};
            for (float x : f) if (!std::isfinite(x)) { std::printf("FAIL ray launch: ray %lld is not finite\n", (long long)k); g_launch_fails++; return; }
            b.keys[k] = ~0ull;
            b.hits[k] = ray_echo(r, k, b.ntri);
        }
        std::lock_guard<std::mutex> lk(g_note_m);
        if (at < g_ray_notes.size()) g_ray_notes[at].ran = true;
    }, nullptr, "k_rays", (size_t)b.n);
}
}  // namespace swr
