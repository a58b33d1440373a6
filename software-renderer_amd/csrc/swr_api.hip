// swr_api.hip — the C-ABI of include/swr.h over the gfx950 kernels (swr_kernels.hip).
//
// Stands in for GpuRenderer.render(renderPass:) (renderer/GpuRenderer.swift:35-141): where the
// reference allocates shared MTLBuffers, encodes one compute dispatch per triangle and blocks
// twice per frame in scheduleAndWait, this context keeps scene, records, bins and the
// framebuffer band resident in HBM and enqueues five kernels on two HIP streams per frame.
//
// One swr_context is either
//   * a single-device context: one GPU, one tile-row band of the framebuffer, or
//   * a group (swr_config.device_count = N > 1): N single-device sub-contexts, sub-context k owning band k of the
//     group's target on device (first + k) % devices, each driven by its own host thread.  Every entry point fans
//     out; the scene is replicated; there is no collective — each device copies its band straight into its rows
//     of the caller's one host image (swr_present / swr_read_*: hipMemcpyAsync on the device's copy streams).
//
// There is no CPU fallback: without a HIP device every computing entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <iterator>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "swr_internal.h"
#include "swr_frame_policy.h"

using namespace swr;

namespace {
thread_local std::string g_create_error;
// true on a context's own helper threads (bin_worker / ras_worker): an error there cannot be written into the context's
// error string — the caller may be reading it (swr_last_error) — and is fatal for the context anyway
thread_local bool tl_helper_thread = false;

// ---- owners: what the HIP runtime hands out is held by a member that gives it back in its destructor.  A context frees nothing by
// hand: deleting it frees what it owns, in reverse order of declaration (see swr_context).  Aliases of a handle stay raw.
// device memory, grown by ensure()
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { (void)reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~DevBuf() { (void)reset(); }
    hipError_t reset() { const hipError_t e = p ? hipFree(p) : hipSuccess; p = nullptr; bytes = 0; return e; }
};
// page-locked host words one band keeps for itself (what a query's answer or a flag table is copied into), grown by ensure_host()
struct HostBuf {
    uint32_t* p = nullptr;
    size_t words = 0;
    HostBuf() = default;
    HostBuf(HostBuf&& o) noexcept : p(o.p), words(o.words) { o.p = nullptr; o.words = 0; }
    HostBuf& operator=(HostBuf&& o) noexcept { if (this != &o) { (void)reset(); p = o.p; words = o.words; o.p = nullptr; o.words = 0; } return *this; }
    ~HostBuf() { (void)reset(); }
    hipError_t reset() { const hipError_t e = p ? hipHostFree(p) : hipSuccess; p = nullptr; words = 0; return e; }
};
// a page-locked allocation of a fixed size (the per-frame words, the stage chunks, a lane's item table); reads as the pointer
template <class T>
struct Pinned {
    T* p = nullptr;
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned() { (void)reset(); }
    operator T*() const { return p; }
    hipError_t alloc(size_t bytes, unsigned flags) { return hipHostMalloc((void**)&p, bytes, flags); }
    hipError_t reset() { const hipError_t e = p ? hipHostFree(p) : hipSuccess; p = nullptr; return e; }
};
// an event and a stream; each reads as its raw handle, so the HIP calls take them as they are
struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (h) (void)hipEventDestroy(h); }
    operator hipEvent_t() const { return h; }
    hipError_t create() { return hipEventCreate(&h); }
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&h, flags); }
};
struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (h) (void)hipStreamDestroy(h); }
    operator hipStream_t() const { return h; }
    hipError_t create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
};

#ifndef SWR_TUNE_HELPER_SPIN
#define SWR_TUNE_HELPER_SPIN 4000     // pause loops an idle Worker spins before it sleeps
#endif
// One host thread per sub-context of a group: HIP calls of different devices are enqueued in parallel and the
// caller's thread pays a few microseconds per fan-out instead of N x (nine HIP calls).  Jobs run in FIFO order;
// asynchronous posts (swr_draw, swr_present) return at once and a failure is kept until the next blocking call.
struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv_job, cv_idle;
    std::deque<std::function<int()>> q;
    bool busy = false, quit = false;
    int sticky_rc = 0;

    void start(int device, bool helper = false) {
        th = std::thread([this, device, helper] {
            tl_helper_thread = helper;
            (void)hipSetDevice(device);
            std::unique_lock<std::mutex> lk(m);
            for (;;) {
                if (q.empty()) {
                    // spin briefly before sleeping: frames arrive every few tens of microseconds
                    lk.unlock();
                    for (int spin = 0; spin < SWR_TUNE_HELPER_SPIN; spin++) {
                        __builtin_ia32_pause();
                        if (pending.load(std::memory_order_acquire)) break;
                    }
                    lk.lock();
                    cv_job.wait(lk, [this] { return quit || !q.empty(); });
                }
                if (q.empty() && quit) return;
                std::function<int()> job = std::move(q.front());
                q.pop_front();
                pending.store(!q.empty(), std::memory_order_release);
                busy = true;
                lk.unlock();
                const int rc = job();
                lk.lock();
                busy = false;
                if (rc && !sticky_rc) sticky_rc = rc;
                if (q.empty()) cv_idle.notify_all();
            }
        });
    }
    void post(std::function<int()> job) {
        {
            std::lock_guard<std::mutex> lk(m);
            q.push_back(std::move(job));
            pending.store(true, std::memory_order_release);
        }
        cv_job.notify_one();
    }
    // wait until every posted job has run; returns (and clears) the first failure since the last drain
    int drain() {
        std::unique_lock<std::mutex> lk(m);
        cv_idle.wait(lk, [this] { return q.empty() && !busy; });
        const int rc = sticky_rc;
        sticky_rc = 0;
        return rc;
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(m);
            quit = true;
        }
        cv_job.notify_one();
        if (th.joinable()) th.join();
    }
    ~Worker() { stop(); }       // (jobs still queued run first: a caller that wants their result drains before)
    std::atomic<bool> pending{false};
};
}  // namespace

static_assert(sizeof(swr_render_pass) == 192 && sizeof(swr_material) == 56 && sizeof(swr_vertex_attr) == 32 &&
              sizeof(swr_vertex) == 32 && sizeof(swr_config) == 16 && sizeof(swr_render_times) == 28 && sizeof(swr_blend) == 16 &&
              sizeof(swr_resolve) == 16 && sizeof(swr_id_count) == 32 && sizeof(swr_depth_box) == 32 && sizeof(swr_delta_stats) == 48 &&
              sizeof(swr_skin_vertex) == 32 && sizeof(swr_morph_targets) == 32 && sizeof(swr_item_bound) == 48 &&
              sizeof(swr_morph_sparse_target) == 32 && sizeof(swr_morph_sparse) == 24 && sizeof(swr_normals) == 16,
              "include/swr.h layouts (mirrored by the ctypes / Swift bindings)");

struct swr_context {
    int device = 0;
#ifndef SWR_NSLOT
#define SWR_NSLOT 4   // working sets = frame lanes = frames in flight: 3 -> 4 lanes: worst band of 8 16.2 -> 13.5 us, of 2 35.8 -> 33.7, the whole frame the same; 5: slower everywhere (more streams than hardware queues), profiles/r04/lanes_probe.txt
#endif
    static constexpr int NSLOT = SWR_NSLOT;
    // ---- ORDER OF FREEING.  Members are destroyed in reverse order of declaration, and every owner below (DevBuf, HostBuf, Pinned,
    // Event) is declared after these streams: deleting the context frees buffers, pinned words and events first, then the lane, binning
    // and copy streams, and `stream` last — the order destroy_single kept by hand.  A new owner goes below this block.
    Stream stream;
    Stream copy_stream[2];              // colour, depth: both images in flight together
    Stream bin_stream_own;
    Stream lane_stream[NSLOT];          // frame lanes (below)
    std::string err;                    // written and read on the caller's thread only (swr_last_error)

    // ---- failure state: a HIP error while a helper thread enqueues, or a wait that outlives the budget, fails the
    // context for good.  `failed` is what every spin loop, every later call and the destructor look at; the text is
    // written once under the mutex (by whichever thread failed) and copied into `err` by the caller's thread.
    std::atomic<int> failed{0};
    std::mutex err_m;
    std::string failed_msg;
    uint32_t wait_budget_ms = 20000;
    std::atomic<int> inject{0};         // swr_debug_fault: consumed by the next frame's raster share
    // swr_debug_set (test hooks; the defaults are what a renderer gets)
    int dbg_stream_order = 1;           // 1 Morton-ordered stream, 0 caller's order, -1 as for >= 2^24 primitives
    int dbg_cull = 1;                   // per-band culling of 64-primitive groups
    int dbg_bin_mode = 0;               // 0 auto (fixed-stride bins where they can hold the scene), 1 exact-size bins, 2 = 0, 3 global-atomic fallback
    int64_t dbg_oneshot_min_tris = (int64_t)1 << 18;
    bool dbg_k32 = true;                // depth-only z-tested frames on 32-bit depth keys
    int dbg_insort = 1;                 // ... which sort their bins inside the raster workgroups: 0 never, 1 on small grids, 2 always
    // scene identity of swr_render (swr_render_pass.scene_id): what is resident
    uint64_t scene_id = 0;
    int64_t scene_nv = -1, scene_ni = -1;
    bool scene_attrs = false;
    const void* scene_tex = nullptr; int32_t scene_tw = 0, scene_th = 0;
    swr_render_times rt{};              // phases of the last swr_render
    float up_h2d_ms = 0.0f, up_build_ms = 0.0f;   // of the last swr_scene_upload (HIP events)
    Event up_ev[3];

    // ---- group (device_count > 1): the sub-contexts (owned: destroy_single) and their host threads.  Of what follows a group uses
    // tg / has_target alone: the full target its bands share ----
    std::vector<swr_context*> kids;
    std::vector<std::unique_ptr<Worker>> workers;
    int band = 0;                       // a sub-context: which band of its group it is

    // scene (RenderPass.vertices / .indices)
    DevBuf vertices, indices, tri_rgb;
    // the triangle stream built at upload (swr_upload.hip)
    DevBuf tri_xyz, inv, box64, stream_scratch, sort_temp;
    bool reordered = false;
    int64_t nv = 0, ni = 0;
    bool has_scene = false;
    // extended fragment stage (swr_scene_attributes / swr_material_set / swr_texture_upload)
    DevBuf attrs, tri_nrm, texture, texture_bytes;   // texture: float4 texels; texture_bytes: upload staging
    bool has_attrs = false;
    swr_material material{};            // shader 0 = the reference's passthrough stage
    swr_blend blend{SWR_BLEND_OVER, 255, {0, 0}};   // swr_blend_set: the state of SWR_FLAG_BLEND frames
    int32_t tex_w = 0, tex_h = 0;
    // skinned meshes (swr_scene_skin / swr_pose_set): the influences; the pose in effect, on the host (restream and
    // swr_scene_attributes rebuild the stream from the bind pose and pose it again) and on the device; the posed vertices (what
    // .vertices and line frames read while a pose is in effect) and normals k_skin_vertices writes
    DevBuf skin, pose_dev, posed, posed_nrm;
    bool has_skin = false;
    int64_t skin_max_joint = -1;        // the largest joint index of the skin (-1: a scene without vertices)
    bool pose_active = false;           // the stream is in `pose` (else: as the upload built it)
    std::vector<float> pose;            // joint_count x 16, or (pose_dq) joint_count x 8
    bool pose_dq = false;               // the pose in effect is a swr_pose_set_dq one: dual quaternions, not matrices
    // morph targets (swr_scene_morph / swr_morph_set): the deltas as swr_internal.h lays them out; the weights on the
    // host (restream and swr_scene_attributes re-apply them) and their non-zero entries as the list the kernel walks, on the host and
    // on the device; the morphed vertices (what the skin, .vertices and line frames read while a weight is not zero) and attributes
    DevBuf morph_dpos, morph_dnrm, morph_list_dev, morphed, morphed_attrs;
    int32_t morph_targets = 0;          // 0: no targets
    bool morph_has_nrm = false;         // normal deltas were given (they take effect once the scene has attributes)
    bool morph_active = false;          // some weight is not zero
    std::vector<float> morph_w;         // morph_targets weights
    std::vector<MorphEntry> morph_list;
    // sparse morph targets (swr_scene_morph_sparse): the other kind of resident targets.  The rows over the touched
    // vertices as swr_internal.h lays them out (entries of positions in morph_dpos, of normals in morph_dnrm) and the weight table on
    // the device.  While they are resident `morphed` (and, with normal deltas and attributes, `morphed_attrs`) hold the base arrays
    // wherever no target reaches: the pre-fill of single_scene_morph_sparse and single_scene_attributes
    DevBuf morph_touched, morph_row, morph_w_dev;
    bool morph_sparse = false;          // the resident targets are sparse ones
    int64_t morph_touched_count = 0;    // rows (0: every target is empty, nothing is ever launched)
    // computed normals (swr_scene_normals): the mode and flags of the scene (in effect while it has attributes); the
    // adjacency swr_scene_normals(SMOOTH) builds once per scene, as swr_internal.h lays it out; the face vectors and the vertex
    // normals the two SMOOTH kernels write
    int32_t normals_mode = SWR_NORMALS_UPLOADED;
    uint32_t normals_flags = 0;
    bool adj_built = false;             // adj_off / adj_tri hold the adjacency of the resident scene
    DevBuf adj_off, adj_tri, face, auto_nrm;

    // target band (RenderPass.colorBuffer / .depthBuffer), double-buffered in HBM: swr_present copies the frame just
    // drawn to the host while the next swr_draw renders into the other buffer
    Target tg{};
    bool has_target = false;
    // (one per lane: with frame lanes — below — every frame in flight renders into its own buffer; the two-stream pipeline uses two)
    static constexpr int NFB = NSLOT;
    static_assert(NFB >= 2, "double-buffered at least");
    DevBuf color[NFB], depth[NFB];
    // SWR_FLAG_PRIMITIVE_IDS: the ID image of each framebuffer, sized by the first ID frame on a target (a context
    // that never asks pays no memory); ids_valid = the last frame wrote one (cleared by swr_target_set / swr_target_write / swr_scene_upload)
    DevBuf ids[NFB];
    bool ids_valid = false;
    // supersampled resolve: the band's resolved colour and depth images, (W/S) x (band rows/S), sized by the first
    // resolved read (k_resolve writes them, copy_band carries them to the host; the framebuffers themselves are only read)
    DevBuf rs_color, rs_depth;
    // visibility counts: the n + 1 counters of a query on the device (zeroed before every query, k_count_ids adds) and
    // the band's own page-locked copy of them, both sized by the largest query so far
    DevBuf count_dev;
    HostBuf count_host;
    // depth queries: the n boxes, the list of the large ones and the n counts of a query, in this order, on the device and
    // in the band's own page-locked staging (words), both sized by the largest query so far; the tile summary k_depth_tiles writes
    DevBuf query_dev, query_tiles;
    HostBuf query_host;
    const uint32_t* query_passed = nullptr;     // the counts of the last query inside query_host
    // item bounds: the n items and the n records of a call, in this order, on the device and in the band's own
    // page-locked staging, both sized by the largest call so far; the partial records k_item_bounds folds into
    DevBuf bounds_dev, bounds_scratch;
    HostBuf bounds_host;
    const swr_item_bound* bounds_out = nullptr; // the records of the last call inside bounds_host
    // ray casts: the n rays, the n key words k_rays combines into and the n hits of a call on the device, and the
    // band's own page-locked staging (the rays, then the hits), all sized by the largest call so far
    DevBuf rays_dev, rays_keys, rays_hits;
    HostBuf rays_host;
    const swr_ray_hit* rays_out = nullptr;      // the hits of the last call inside rays_host
    // delta reads: per image kind (0 colour, 1 depth) the band's baseline — the image the last delta read delivered —
    // and whether it holds one; the tile flags k_delta_tiles writes, on the device and in the band's own page-locked copy; the rows of
    // a changed rectangle gathered for one linear copy; what the band's last delta read did (a group adds the bands up)
    DevBuf delta_base[2], delta_flags, delta_pack;
    bool delta_valid[2] = {false, false};
    HostBuf delta_host;
    swr_delta_stats delta_stats{};
    int fb_cur = 0;                    // the next swr_draw renders into this buffer
    int fb_last = 0;                    // the buffer of the last swr_draw (what swr_present / swr_read_* copy)
    hipStream_t last_stream = nullptr;  // the stream that carries the last frame's raster (swr_present records frame_done behind it)
    Event frame_done[NFB];               // raster stream -> copy streams, per framebuffer
    Event copy_done[NFB][2];             // [fb][image]: the raster into fb waits for these
    bool copy_recorded[NFB][2] = {};
    // ---- load frames (SWR_FLAG_LOAD): a frame that starts from the band's current image instead of the clear
    bool src_clear = true;              // the current image is the cleared one (swr_target_set): a load frame is then a clear frame
    int load_src = 0;                   // the framebuffer the last frame loaded from (its overflow redraw reads it again)
    Event src_ready;                    // frame lanes: the source frame's raster, waited for by the load frame's raster
    Event read_done[NFB];               // frame lanes: the raster of the load frame that read framebuffer fb; writers of fb wait for it
    bool read_recorded[NFB] = {};
    // pinned staging for destinations that are not page-locked (two 8 MiB chunks per image, D2H / memcpy pipelined)
    static constexpr size_t STAGE_BYTES = 8u << 20;
    Pinned<uint8_t> stage[2][2];
    Event stage_ev[2][2];
    // the last swr_present (for the redo of a frame whose pair list overflowed)
    void* present_color = nullptr;
    float* present_depth = nullptr;
    bool present_pending = false;

    // Per-frame working set, multi-buffered: the binning kernels of frame N+1 run on `bin_stream`
    // while k_raster of frame N runs on `stream` (HBM-bound vs LDS/VALU-bound: they overlap well).
    struct Slot {
        DevBuf geo, geo_full, ranges, bins, bin_matrix;
        DevBuf biglist;        // fixed-stride bins: the frame's deferred large triangles (k_bin -> k_sort_bins)
        DevBuf live;           // per binning workgroup: count + surviving stream-group ids (k_setup_hist -> k_fill_lds)
        DevBuf tilebuf;        // [CNT_WORDS counters][tiles tile_count][tiles+1 tile_start][tiles cursor]
        Event bin_done;                    // two-stream: the binning chain's completion; lanes: polled by the injected lost event only
        // draw-list frames: the item table (pinned staging -> device, on the frame's own stream, before its binning)
        // and the frame's per-slot colours / attributes / original-index table (k_list_gather)
        DevBuf items, lrgb, lnrm, linv;
        // depth-clip frames: the frame's clip stream (n + 2F slots) and the pre-pass's tables (swr_clip.hip)
        DevBuf cxyz, crgb, cnrm, cmap, cbox, csums;
        // perspective frames: the frame's per-slot (q_a, q_b, q_c, bypass) table (k_persp_fill / k_clip_emit)
        DevBuf pq;
        Pinned<ListItem> items_host;        // pinned; rewritten only after items_copied (its last copy) has completed
        size_t items_cap = 0;
        Event items_copied;
        bool items_recorded = false;
        uint64_t items_frame = 0;           // the frame whose copy items_copied follows
    } slot[NSLOT];
    hipStream_t bin_stream = nullptr;   // the stream binning is enqueued on (== stream when pipelining is off); every scheduler: sched_of reads it
    Event up_chunk_ev;                  // one-shot upload: index chunk k resident / its stream built
    uint64_t frame_no = 0;
    uint64_t synced_upto = 0;           // every frame below this has completed (full stream sync seen by the caller)
    int last_slot = 0;
    uint32_t capacity = 0;              // exact bins: (triangle,tile) pairs every slot's `bins` holds
    // ---- FRAME LANES (round 4; the default whenever frames may overlap).  The binning and the raster of ONE frame go back to
    // back onto ONE stream — kernels of a queue follow each other without a gap, and nothing else orders them: no event, no
    // wait packet, no completion signal, no helper thread that polls — and consecutive frames onto NSLOT different streams.
    // Everything a frame writes belongs to its lane: the working set (slot = lane), its two fill blocks (k_bin of the lane's
    // n-th frame zeroes the block of its (n + 1)-th, last read by a raster that is earlier on the same stream) and its
    // framebuffer (fb advances with every draw; the buffer a frame writes was last written NSLOT frames earlier — same lane).
    // Frames of different lanes overlap freely on the chip.  What the two-stream pipeline of rounds 1-3 paid per frame — a
    // 5 us gap behind every kernel that carries a completion signal, the polls of two helper threads — is gone: cfg4 76 -> 67 us
    // per frame, and a thin band (1/8 of the frame: bound by its kernel chain, not by the chip) 24.5 -> 15.9 us
    // (profiles/r04/lanes_probe.txt).  SWR_LANES=0 keeps the two-stream pipeline.
    bool lanes_ok = false;
    DevBuf lanefill[NSLOT][2];
    bool lanefill_dirty[NSLOT][2] = {};
    // pacing of an un-waited burst: every PACE_EVERY-th frame leaves a marker behind its raster; a draw waits for the marker of
    // 3 * PACE_EVERY frames ago (the per-frame pinned words are a ring of PAIR_RING frames)
    static constexpr int PACE_EVERY = 24;
    Event pace_ev[4];
    uint64_t pace_frame[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    uint32_t cap_tile = 0;              // entries per tile region
    bool fixed_mode = false;            // frames are binned by k_bin (else: exact-size bins, four kernels)
    bool fixed_allowed = true;          // false once a tile of this scene / target needed more than the fixed path can give
    size_t bins_entries = 0;            // entries every slot's `bins` holds

    // Pinned, device-mapped words.  h_pairs[f % PAIR_RING] receives the (triangle,tile) pair total of frame f from
    // the binning kernels (no D2H copy, no host sync per frame); a whole burst of un-waited frames can be checked
    // for bin overflow afterwards.  h_misc is the upload's index-check word.
    // (Fixed-stride bins: words [PAIR_RING + 1, 2 PAIR_RING + 1) receive the LARGEST tile fill of frame f — the overflow
    // test there is per tile region.)
    static constexpr int PAIR_RING = 256;
    Pinned<uint32_t> h_pairs;
    uint32_t* h_pairs_dev = nullptr;
    bool frame_presented[PAIR_RING] = {};   // was frame f copied to the host (swr_present)?  Only then can an overflow be seen
    bool frame_load[PAIR_RING] = {};        // did frame f start from the image of frame f - 1 (a load frame)?
    bool src_bad = false;                   // the image of frame frames_checked - 1 is wrong: an overflow left it empty, or it loaded one
    Pinned<uint32_t> h_misc;
    // Depth-only z-tested frames: 32-bit depth keys (k_raster_depth) until the scene shows that too many of its tiles have
    // to be rastered again with the 64-bit keys (depths that are not > +0: a 2-D scene at z = 0, geometry in front of the
    // near plane); word 2 PAIR_RING + 1 of h_pairs receives the sampled count of such tiles, one launch late.
    bool k32_ok = true;                 // reset by a scene of another size / another tile grid
    int64_t sized_ntri = -1;            // what size_bins last sized the bins for
    int sized_tiles = -1;
    DevBuf redo_cnt;                    // the device counter behind that word
    uint64_t frames_checked = 0;        // frames [frames_checked, frame_no) have not had their pair total looked at
    // (every scheduler keeps these three in step — mark_posted — so that a swr_pipeline_enable toggle finds them where the other expects)
    std::atomic<uint64_t> bin_enqueued{0};      // frames whose binning (incl. the bin_done record) is on the binning stream
    std::atomic<uint64_t> ras_enqueued{0};      // frames whose raster (incl. the ras_done record) is on the raster stream
    uint64_t posted = 0;                        // frames handed over: to the helper or run inline (two-stream), enqueued whole or abandoned (lanes)
    // ---- THE TWO-STREAM PIPELINE (rounds 1-3: SWR_LANES=0) and its one-stream case (swr_pipeline_enable(0)): what only they use.  The
    // lanes touch none of it, except that every scheduler drains the helpers (flush_raster, sync_copies: they may hold a present's copies).
    struct TwoStream {
#ifndef SWR_RAS_EVERY
#define SWR_RAS_EVERY 1   // every n-th k_raster carries a completion event (see RAS_EVERY)
#endif
        // A kernel that carries a completion signal (ras_done) costs the NEXT kernel of its queue ~5 us
        // (profiles/r02/c_kernel_trace_pipelined.txt).  The binning of frame N needs "k_raster(N - NSLOT) has finished"; it
        // waits for the first event-carrying raster at or after that frame instead (same queue, in order), so only every
        // RAS_EVERY-th raster needs one, at the price of RAS_EVERY - 1 extra working sets.  Measured (NSLOT / RAS_EVERY = 3 / 1,
        // 4 / 2, 6 / 4; profiles/r02/ras_every_ab.txt): cfg4 0.0977 / 0.0993 / 0.0981 ms, 1/8 band 29.2 / 27.7 / 27.0 us — the
        // gap on the raster queue is filled by the binning queue's kernels (the frame is bound by the sum of the work), so
        // the default stays 3 / 1.
        static constexpr int RAS_EVERY = SWR_RAS_EVERY;
        static_assert(RAS_EVERY >= 1 && NSLOT > RAS_EVERY, "the event-carrying raster must be older than the frame being binned");
        // Fixed-stride bins (k_bin: ONE binning launch per frame): tile t owns bins[t * cap_tile, (t + 1) * cap_tile).  The
        // per-tile fill counters live in NFILL = NSLOT + 1 rotating blocks (frame % NFILL) while the working sets rotate by NSLOT:
        // k_bin of frame N zeroes the block of frame N + 1, which was last read by the raster of frame N - NSLOT — the raster
        // whose completion lets the binning of frame N start.
        static constexpr int NFILL = NSLOT + 1;      // k_bin(N) zeroes the fill block of frame N + 1: its last reader must be the raster of frame N - NSLOT
        DevBuf fillbuf[NFILL];              // [CNT_WORDS counters][tiles fills]
        bool fill_dirty[NFILL] = {};        // block was used and nothing has zeroed it since (then the frame memsets it first)
        // Two host threads per context: every frame is ~9 HIP calls (3.5 us each); the binning stream's share (slot wait,
        // three or four launches, event record) is enqueued by `bin_worker` while the caller's thread enqueues the raster
        // stream's share (event wait, launches, event record) of the PREVIOUS frame — a thin band or a small scene is
        // bound by the host's enqueue rate, not by the GPU.
        std::unique_ptr<Worker> bin_worker;
        // ... and a third one for the raster stream's share, for a different reason: a cross-stream hipStreamWaitEvent in
        // front of a kernel costs that kernel ~10 us after its predecessor on the queue has ended, even when the event
        // completed long before (profiles/r02/gaps_pipelined_before.txt) — a wait that is never enqueued costs nothing.
        // `ras_worker` polls hipEventQuery(bin_done) of the frame and only then enqueues k_raster, with no wait in front
        // (and `bin_worker` does the same with ras_done before it re-uses a working set).  swr_draw / swr_present only post.
        // SWR_EVENT_WAITS=1: the caller's thread enqueues the raster share behind event waits (round-2 first half).
        std::unique_ptr<Worker> ras_worker;
        // bin_done / ras_done are bound to the kernels they follow (hipExtLaunchKernelGGL's stop event) instead of being
        // recorded behind them: a marker packet between two kernels of a queue costs the second one ~6.5 us.  SWR_BIND_EVENTS=0: record.
        bool bind_events = true;
        // One frame at a time (an interactive app: swr_draw, swr_sync / swr_present_wait, idle, ...) does not need the
        // helpers: when every earlier frame is known to be complete, the frame is enqueued by the caller's thread itself,
        // ordered by event waits on the streams — the helpers may be asleep by then, and waking two threads costs more than
        // the two wait packets (draw -> sync of cfg4 after 5 ms of idle: 205 -> 180 us; cfg2 94 -> 70 us,
        // profiles/r02/cold_latency.txt).  Frames drawn while others are in flight go through the helpers.  SWR_INLINE_IDLE=0: never.
        bool inline_idle = true;
        std::atomic<int> bin_error{0};
        static constexpr int RAS_RING = 64;          // frames whose raster share may be waiting for ras_worker; swr_draw blocks beyond that
        struct RasJob { DeviceFrame f; hipEvent_t ev3 = nullptr, ev4 = nullptr; int si = 0; bool sort_here = false; int fb = 0; bool paced = false; } ras_job[RAS_RING];
        // per working set: the completion of the event-carrying k_raster that read it, and the frame whose k_raster it tracks (none yet)
        struct RasDone { Event ev; uint64_t frame = ~0ull; } ras_done[NSLOT];
    } ts;
    // ---- draw lists (swr_draw_list)
    bool stream_sorted = false;         // the stream is Morton-sorted: a list's ranges must be runs of slots (cut the stream at them)
    std::vector<uint32_t> cuts;         // primitive indices the stream is cut at now (sorted; empty: one segment, as uploaded)
    DevBuf cuts_dev;
    // (clip_fan and clip_total are not in the record: they are how the context sizes a clip frame — check_frames grows the fan — not what was drawn)
    int64_t clip_fan = 0;               // fan capacity F: a clip frame of n triangles has n + 2F slots (each crossing triangle adds <= 2)
    int64_t clip_total = -1;            // the post-clip count of the last clip frame when the host had to know it (else -1)
    Pinned<uint32_t> h_clip;            // pinned, device-mapped: [PAIR_RING] per frame, the post-clip count of a clip frame whose fans
    uint32_t* h_clip_dev = nullptr;     // overflowed its slots (0: none); [PAIR_RING] the post-clip count the host asked for
    int64_t list_plan_max = 0;          // largest binning size (work units * 64) of a list since the upload (fixed-bin limits)
    // The last draw: what its frame is built from (make_frame, make_list_frame, make_clip_frame) and what its redo after an overflow
    // (check_frames) needs again.  The draw entry points fill it (begin_draw .. end_draw; prepare_clip sets clip_n); everything else reads.
    struct DrawRecord {
        float m[16]{};
        uint32_t flags = 0;
        swr_blend blend{SWR_BLEND_OVER, 255, {0, 0}};   // the blend state the frame was posted with (a redo draws with it again)
        int prim = SWR_PRIMITIVE_TRIANGLE;
        bool is_list = false;               // a draw list (swr_draw_list) of
        std::vector<ListItem> list;         // these items (kept while it is the last draw: the redo stages them again),
        int64_t list_tris = 0, list_units = 0;   // its total and its k_bin work units
        bool list_affine = false, list_identity = false;   // identity: frame slot == stream slot and order number == original index for every item
        bool clip = false; int64_t clip_n = 0;   // a depth-clip frame (SWR_FLAG_DEPTH_CLIP) of clip_n submitted triangles
        bool persp = false;                 // perspective-correct colour (SWR_FLAG_PERSPECTIVE, triangles through a non-affine transform): its slot's pq table is filled and read
    } last_draw;
    bool draw_pending = false;

    // timing: a ring of hipEvent sets recorded on the context stream around each kernel, so a
    // whole timed region of frames can be measured without a host sync per frame
    static constexpr int RING = 64;
    int timing = 0;            // 0 off, 1 = events around k_raster only, 2 = around every stage
    int timing_every = 1;      // level 1: bracket only every n-th frame's k_raster (swr_timing_sample)
    Event ev[RING][5];
    int ev_level[RING]{};
    uint64_t seq = 0;          // frames enqueued with timing on
    uint64_t harvested = 0;    // frames whose events have been read
    swr_timings last{};
    double sum_ms[5]{};
    int64_t sum_frames = 0;

    // SWR_HOST_PROFILE=1: wall time of the host side of a frame, split by HIP call group, printed at destroy
    bool hp_on = false;
    double hp_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t hp_frames = 0;
    std::chrono::steady_clock::time_point hp_last, hp_last_r;    // hp_last_r: the raster share's own clock (it may run on ras_worker)
    void hp_lap_on(std::chrono::steady_clock::time_point& last, int k) {
        if (!hp_on) return;
        const auto now = std::chrono::steady_clock::now();
        hp_t[k] += std::chrono::duration<double, std::micro>(now - last).count();
        last = now;
    }
    void hp_begin() { if (hp_on) hp_last = std::chrono::steady_clock::now(); }
    void hp_lap(int k) { hp_lap_on(hp_last, k); }
    void hp_begin_r() { if (hp_on) hp_last_r = std::chrono::steady_clock::now(); }
    void hp_lap_r(int k) { hp_lap_on(hp_last_r, k); }
};

namespace {

// The context has failed for good (first failure wins).  Callable from any thread.
int fatal_msg(swr_context* c, int code, const char* text) {
    std::lock_guard<std::mutex> lk(c->err_m);
    if (!c->failed.load(std::memory_order_relaxed)) {
        c->failed_msg = text;
        c->failed.store(code, std::memory_order_release);
    }
    return code;
}

int fail(swr_context* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (!c) g_create_error = buf;
    else if (tl_helper_thread) return fatal_msg(c, code, buf);    // never touch c->err from a helper (the caller may be reading it)
    else c->err = buf;
    return code;
}

int fatal(swr_context* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return fatal_msg(c, code, buf);
}

// Caller's thread: has the context failed?  Then its text becomes the last error and every entry point returns the code.
int sticky(swr_context* c) {
    const int f = c->failed.load(std::memory_order_acquire);
    if (f) {
        std::lock_guard<std::mutex> lk(c->err_m);
        c->err = c->failed_msg;
    }
    return f;
}

// `rc` of a failed wait — or, when the context has failed for good meanwhile, that failure
inline int or_sticky(swr_context* c, int rc) { const int f = sticky(c); return f ? f : rc; }

// The bands of c: the sub-contexts of a group, or the context itself.  Band 0 answers for the scene every band holds.
inline bool is_group(const swr_context* c) { return !c->kids.empty(); }
inline size_t band_count(const swr_context* c) { return is_group(c) ? c->kids.size() : 1; }
template <class C> inline C* band(C* c, size_t k) { return is_group(c) ? c->kids[k] : c; }

// Bounded waiting: spin, then yield, never beyond the context's budget; gives up at once when the context has failed.
struct Deadline {
    std::chrono::steady_clock::time_point end;
    unsigned spins = 0;
    explicit Deadline(const swr_context* c) : end(std::chrono::steady_clock::now() + std::chrono::milliseconds(c->wait_budget_ms)) {}
    // false: the budget is used up
    bool pause() {
        if (++spins < 2000) { for (int i = 0; i < 8; i++) __builtin_ia32_pause(); return true; }
        std::this_thread::yield();
        return (spins & 63u) != 0 || std::chrono::steady_clock::now() < end;
    }
};

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ctx, SWR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

int ensure(swr_context* c, DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return SWR_OK;
    HIP_TRY(c, b.reset());
    // grow geometrically so a slowly growing scene does not reallocate every frame
    size_t want = bytes + bytes / 8;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(c, SWR_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    b.bytes = want;
    return SWR_OK;
}

int ensure_host(swr_context* c, HostBuf& b, size_t words) {
    if (b.words >= words) return SWR_OK;
    HIP_TRY(c, b.reset());
    const size_t want = words + words / 8;
    HIP_TRY(c, hipHostMalloc((void**)&b.p, want * 4, hipHostMallocDefault));
    b.words = want;
    return SWR_OK;
}

int ensure_bins(swr_context* c, size_t entries) {
    if (entries <= c->bins_entries) return SWR_OK;
    int rc;
    for (auto& sl : c->slot)
        if ((rc = ensure(c, sl.bins, entries * 4))) return rc;
    c->bins_entries = entries;
    return SWR_OK;
}

int ensure_capacity(swr_context* c, uint32_t cap) {
    if (cap <= c->capacity) return SWR_OK;
    const int rc = ensure_bins(c, cap);
    if (rc) return rc;
    c->capacity = cap;
    return SWR_OK;
}

int flush_raster(swr_context* c, uint64_t upto_frame_count);
int enqueue_raster_shares(swr_context* c, uint64_t upto_frame_count);

// hipEventQuery until the event has completed (host-paced ordering: see swr_context::ras_worker) — or the context has
// failed, or the wait budget is used up: then the context fails with what was being waited for.
int poll_event(swr_context* c, hipEvent_t ev, const char* what, uint64_t frame, bool never = false) {
    Deadline d(c);
    for (;;) {
        if (const int f = c->failed.load(std::memory_order_acquire)) return f;
        const hipError_t e = never ? hipErrorNotReady : hipEventQuery(ev);
        if (e == hipSuccess) return SWR_OK;
        if (e != hipErrorNotReady) return fatal(c, SWR_ERR_HIP, "hipEventQuery(%s of frame %llu) failed: %s", what, (unsigned long long)frame, hipGetErrorString(e));
        if (!never) (void)hipGetLastError();                  // hipErrorNotReady is sticky in hipGetLastError
        if (!d.pause())
            return fatal(c, SWR_ERR_HIP, "frame %llu: %s did not complete within %u ms (device %d); the context has failed",
                         (unsigned long long)frame, what, c->wait_budget_ms, c->device);
    }
}

// hipStreamSynchronize with the same bound (hipStreamQuery polls)
int wait_stream(swr_context* c, hipStream_t s, const char* what) {
    Deadline d(c);
    for (;;) {
        if (const int f = c->failed.load(std::memory_order_acquire)) return f;
        const hipError_t e = hipStreamQuery(s);
        if (e == hipSuccess) return SWR_OK;
        if (e != hipErrorNotReady) return fatal(c, SWR_ERR_HIP, "hipStreamQuery(%s) failed: %s", what, hipGetErrorString(e));
        (void)hipGetLastError();
        if (!d.pause())
            return fatal(c, SWR_ERR_HIP, "the %s did not drain within %u ms (device %d, %llu frames drawn); the context has failed",
                         what, c->wait_budget_ms, c->device, (unsigned long long)c->frame_no);
    }
}

// wait until an atomic frame counter has passed `g` (the other helper's progress)
int wait_counter(swr_context* c, const std::atomic<uint64_t>& ctr, uint64_t g, const char* what) {
    Deadline d(c);
    while (ctr.load(std::memory_order_acquire) <= g) {
        if (const int f = c->failed.load(std::memory_order_acquire)) return f;
        if (!d.pause())
            return fatal(c, SWR_ERR_HIP, "frame %llu: %s was not enqueued within %u ms; the context has failed", (unsigned long long)g, what, c->wait_budget_ms);
    }
    return SWR_OK;
}

// The three schedulers of a frame.  OneStream: binning and raster on `stream` (swr_pipeline_enable(0), SWR_PIPELINE=0).  Lanes: whenever
// frames may overlap at all (pipelining on), a frame's binning and raster go onto its lane (swr_context::lane_stream).  TwoStream
// (SWR_LANES=0, or a lane stream could not be created): binning on `bin_stream`, raster on `stream` (swr_context::TwoStream).
enum class Sched { OneStream, TwoStream, Lanes };
inline Sched sched_of(const swr_context* c) { return c->bin_stream == c->stream ? Sched::OneStream : c->lanes_ok ? Sched::Lanes : Sched::TwoStream; }
using TS = swr_context::TwoStream;

int sync_streams(swr_context* c) {
    int rc = flush_raster(c, c->frame_no);      // everything drawn so far is on the streams
    if (!rc) rc = wait_stream(c, c->bin_stream, "binning stream");
    if (!rc) rc = wait_stream(c, c->stream, "raster stream");
    if (c->lanes_ok)
        for (hipStream_t ls : c->lane_stream)
            if (!rc && ls) rc = wait_stream(c, ls, "frame lane");
    if (rc) return or_sticky(c, rc);
    c->synced_upto = c->posted;      // NOT frame_no: enqueue_frame may sync after it has numbered the frame it is about to post
    for (bool& r : c->read_recorded) r = false;     // every load frame's read of its source has completed: nothing to wait for
    return SWR_OK;
}

int sync_copies(swr_context* c) {
    int rc = SWR_OK;
    if (c->ts.ras_worker) rc = c->ts.ras_worker->drain();    // posted swr_present copies
    if (!rc) rc = wait_stream(c, c->copy_stream[0], "colour copy stream");
    if (!rc) rc = wait_stream(c, c->copy_stream[1], "depth copy stream");
    if (rc) return or_sticky(c, rc);
    return SWR_OK;
}

inline int tiles_of(const Target& t) { return t.tiles_x * t.tiles_y; }
inline uint32_t& pair_word(swr_context* c, uint64_t frame) { return c->h_pairs[frame % swr_context::PAIR_RING]; }
inline uint32_t& fill_word(swr_context* c, uint64_t frame) { return c->h_pairs[swr_context::PAIR_RING + 1 + frame % swr_context::PAIR_RING]; }

// ---- growing what every lane owns ---------------------------------------------------------------------------------------------
// A table of (working-set buffer, bytes a frame needs): if any lane's buffer is smaller, every stream is drained once and every
// lane's buffer grown.  Each size is written once, in the table; an entry that applies only under a condition is not added.
struct LaneSizes {
    struct Entry { DevBuf swr_context::Slot::* buf; size_t bytes; } e[12];
    int n = 0;
    void add(DevBuf swr_context::Slot::* buf, size_t bytes) { e[n].buf = buf; e[n].bytes = bytes; n++; }
};
int grow_lanes(swr_context* c, const LaneSizes& t) {
    bool grow = false;
    for (auto& sl : c->slot)
        for (int k = 0; k < t.n; k++) grow = grow || (sl.*t.e[k].buf).bytes < t.e[k].bytes;
    if (!grow) return SWR_OK;
    int rc = sync_streams(c);
    if (rc) return rc;
    for (auto& sl : c->slot)
        for (int k = 0; k < t.n; k++)
            if ((rc = ensure(c, sl.*t.e[k].buf, t.e[k].bytes))) return rc;
    return SWR_OK;
}

// ---- the first guess of the bins ------------------------------------------------------------------------------------------------
// Fixed-stride bins, entries per tile region for `tris` triangles on `tiles` tiles, at most `cmax`.  A primitive enters a tile's
// region at most once, so a region of `tris` entries can never overflow: small frames get that; large ones six times the mean load
// of a tile, at least 1024 entries (a fuller tile makes the host grow the regions and redraw once).
inline uint32_t first_cap_tile(int64_t tris, int tiles, uint32_t cmax) {
    const uint64_t want = std::max<uint64_t>(std::max<uint64_t>(64, (uint64_t)(6 * tris / tiles)), (uint64_t)std::min<int64_t>(tris, 1024));
    return (uint32_t)std::min<uint64_t>((want + 63) & ~63ull, cmax);
}
// Exact-size bins: (triangle,tile) pairs for `tris` triangles
inline uint32_t first_capacity(int64_t tris) { return (uint32_t)std::min<uint64_t>((uint64_t)tris * 2 + 65536, 0xFFFFFFF0ull); }

// The bins must be able to take a frame of `tris` triangles whose binning size is `plan` (a draw list: its k_bin work units * 64; a
// clip frame: its slots), sized by the first guess as size_bins sizes them for the scene: they only grow, with every stream idle.
// A frame beyond what k_bin can hold (a workgroup's share of the work below the cursor limit) moves the context to the exact-size
// bins, as a scene that needs more than a region would.
int fit_bins(swr_context* c, int64_t tris, int64_t plan) {
    int rc;
    const int tiles = tiles_of(c->tg);
    if (c->fixed_mode && tris > 0) {
        if (fixed_cap_max(plan, tiles) < c->cap_tile) {
            if ((rc = sync_streams(c))) return rc;
            c->fixed_mode = false;
            c->fixed_allowed = false;
        } else {
            // (capped for the scene's own frames too: a region survives into them, and their cursors must stay below 2^16)
            const uint32_t want = first_cap_tile(tris, tiles, fixed_cap_max(std::max<int64_t>(c->ni / 3, plan), tiles));
            if (want > c->cap_tile) {
                if ((rc = sync_streams(c))) return rc;
                if ((rc = ensure_bins(c, (size_t)tiles * want))) return rc;
                c->cap_tile = want;
            }
        }
    }
    if (!c->fixed_mode && tris > 0 && first_capacity(tris) > c->capacity) {
        if ((rc = sync_streams(c))) return rc;
        if ((rc = ensure_capacity(c, first_capacity(tris)))) return rc;
    }
    // (the fixed-bin limits of check_frames and of later frames cover this frame's binning size too)
    c->list_plan_max = std::max<int64_t>(c->list_plan_max, plan);
    return SWR_OK;
}

// Size the bins for the scene / target pair (both known; every stream idle).  Fixed-stride bins where k_bin can be used:
// a first guess of six times the mean load per tile (the host grows it when a frame overflows), exact bins otherwise.
int size_bins(swr_context* c) {
    if (!c->has_scene || !c->has_target) return SWR_OK;
    const int tiles = tiles_of(c->tg);
    const int64_t ntri = c->ni / 3;
    {   // the redo counter of the 32-bit depth keys starts from zero (swr_context::k32_ok is reset by the callers)
        int rc0 = ensure(c, c->redo_cnt, 16);
        if (rc0) return rc0;
        HIP_TRY(c, hipMemsetAsync(c->redo_cnt.p, 0, 16, c->stream));
        if ((rc0 = wait_stream(c, c->stream, "raster stream (redo counter)"))) return or_sticky(c, rc0);
        c->h_pairs[2 * swr_context::PAIR_RING + 1] = 0u;
        c->sized_ntri = ntri; c->sized_tiles = tiles;
    }

    // Bands of large scenes (what one GPU of N renders) took round 2's chain of three short binning kernels in round 3: the one
    // long k_bin shared the chip with the band's raster worse.  With the perspective divide gone for affine transforms (k_bin
    // <.., AFF>) and no k_sort_bins launch on thin depth-only bands (the raster sorts its own bins) it is the other way round:
    // worst band of N = 2 / 4 / 8 on one GPU 47.1 / 29.3 / 24.5 us per frame against 52.8 / 35.7 / 26.3 with the chain
    // (profiles/r04/band_binmode_ab.txt) — k_bin everywhere.  Colour frames: N = 2 / 4 equal, N = 8 32.9 (chain) vs 36.4.
    // swr_debug_set(SWR_DEBUG_BIN_MODE, 1) forces the chain.
    const bool no_fixed = c->dbg_bin_mode == 1 || c->dbg_bin_mode == 3;
    const uint32_t cmax = (c->fixed_allowed && !no_fixed) ? fixed_cap_max(ntri, tiles) : 0u;
    int rc;
    if (cmax) {
        const uint32_t want = first_cap_tile(ntri, tiles, cmax);
        if (!c->fixed_mode || c->cap_tile < want || c->cap_tile > cmax) c->cap_tile = want;   // a grown region survives a new transform
        if ((rc = ensure_bins(c, (size_t)tiles * c->cap_tile))) return rc;
        const size_t fb = (size_t)(CNT_WORDS + tiles) * 4;
        for (int k = 0; k < TS::NFILL; k++) {
            if ((rc = ensure(c, c->ts.fillbuf[k], fb))) return rc;
            HIP_TRY(c, hipMemsetAsync(c->ts.fillbuf[k].p, 0, c->ts.fillbuf[k].bytes, c->stream));
            c->ts.fill_dirty[k] = false;
        }
        for (int l = 0; l < swr_context::NSLOT; l++)
            for (int k = 0; k < 2; k++) {
                if ((rc = ensure(c, c->lanefill[l][k], fb))) return rc;
                HIP_TRY(c, hipMemsetAsync(c->lanefill[l][k].p, 0, c->lanefill[l][k].bytes, c->stream));
                c->lanefill_dirty[l][k] = false;
            }
        if ((rc = wait_stream(c, c->stream, "raster stream (fill counters)"))) return or_sticky(c, rc);
        c->fixed_mode = true;
        return SWR_OK;
    }
    c->fixed_mode = false;
    return ensure_capacity(c, first_capacity(ntri));
}

#ifndef SWR_TUNE_IDLE_BIN_G
#define SWR_TUNE_IDLE_BIN_G 512
#endif
// The binning geometry of a frame of `ntri` triangles.  A frame over a stream of its own (own_stream: a draw list, whose binning
// size is its work units * 64, or a clip frame) is planned by that `size` under the fixed-stride bins and takes the global-atomic
// chain under the exact-size ones (its tables need no per-G sizing).
// An idle context (every earlier frame complete: a single frame, or the first of a burst) bins with twice the workgroups, idle_G
// (an eighth of the frame's 64-primitive groups) at most SWR_TUNE_IDLE_BIN_G: with nothing else on the chip k_bin is a chain of round
// trips at one wave per SIMD, and two waves per SIMD overlap them; beside a raster the extra waves only take issue slots from it
// (round 2's sweeps), so frames posted while others are in flight keep one workgroup per CU.
BinPlan plan_frame(const swr_context* c, int64_t ntri, int64_t size, int64_t idle_G, bool own_stream) {
    const int tiles = tiles_of(c->tg);
    const bool fixed = c->fixed_mode && ntri > 0;
    BinPlan p = !own_stream ? plan_binning(ntri, tiles, c->dbg_bin_mode == 3) : fixed ? plan_binning(size, tiles, false) : plan_binning(ntri, tiles, true);
    if (fixed && c->synced_upto == c->posted)
        p.G = (int)std::max<int64_t>(1, std::min<int64_t>(SWR_TUNE_IDLE_BIN_G, std::max<int64_t>(p.G, idle_G)));
    return p;
}

// The frame of draw `d` on working set si, as a plain frame over the scene's stream (a list or clip frame is made of it below).
DeviceFrame make_frame(swr_context* c, int si, uint64_t frame, const swr_context::DrawRecord& d) {
    swr_context::Slot& sl = c->slot[si];
    DeviceFrame f{};
    // (k_points / k_lines: the last array of the chain morph, skin)
    f.vertices = (const swr_vertex*)(c->pose_active ? c->posed.p : c->morph_active ? c->morphed.p : c->vertices.p);
    f.indices = (const int64_t*)c->indices.p;
    f.tri_rgb = (const float4*)c->tri_rgb.p;
    f.tri_xyz = (const float4*)c->tri_xyz.p;
    f.inv = (const uint32_t*)c->inv.p;
    f.box64 = (const float4*)c->box64.p;
    f.reordered = c->reordered ? 1 : 0;
    f.tri_nrm = (const float4*)c->tri_nrm.p;
    f.material = c->material;
    f.texels = (const float4*)c->texture.p;
    f.tex_w = c->tex_w; f.tex_h = c->tex_h;
    f.vertex_count = c->nv;
    f.index_count = c->ni;
    f.ntri = c->ni / 3;
    f.geo = (GeomRec*)sl.geo.p;
    f.geo_full = (GeomFull*)sl.geo_full.p;
    uint32_t* tb = (uint32_t*)sl.tilebuf.p;
    f.counters = tb;
    f.host_counters = c->h_pairs_dev + (frame % swr_context::PAIR_RING);   // word CNT_PAIRS (= 0) of this frame
    f.host_max = c->h_pairs_dev + swr_context::PAIR_RING;                  // one word, overwritten by every frame
    f.skip_sort = 0;
    f.defer_big = 0;
    f.redo_dev = (uint32_t*)c->redo_cnt.p;
    f.host_redo = c->h_pairs_dev + 2 * swr_context::PAIR_RING + 1;
    // (ID frames take the 64-bit keys, whose key carries the winner: they neither use nor move the scene's 32-bit-key state)
    f.k32 = (c->k32_ok && c->dbg_k32 && f.redo_dev && !(d.flags & SWR_FLAG_PRIMITIVE_IDS)) ? 1 : 0;
    f.tile_count = tb + CNT_WORDS;
    f.tile_start = tb + CNT_WORDS + tiles_of(c->tg);
    f.tile_cursor = tb + CNT_WORDS + 2 * tiles_of(c->tg) + 1;
    f.ranges = (uint2*)sl.ranges.p;
    f.plan = plan_frame(c, f.ntri, f.ntri, ((f.ntri + 63) / 64 + 7) / 8, false);
    f.bin_matrix = (uint32_t*)sl.bin_matrix.p;
    f.live = (uint32_t*)sl.live.p;
    // Groups of the stream whose projected box misses this context's band (or the framebuffer) are skipped by
    // k_setup_hist; the test costs one lane-pass per workgroup, so it is always on (SWR_DEBUG_CULL = 0 switches it off).
    f.live_parity = c->dbg_cull != 0 ? 0 : -1;
    f.bins = (uint32_t*)sl.bins.p;
    f.capacity = c->capacity;
    f.fixed_bins = (c->fixed_mode && f.ntri > 0) ? 1 : 0;
    f.cap_tile = c->cap_tile;
    if (sched_of(c) == Sched::Lanes) {       // the lane's two blocks alternate: this frame's, and the one its k_bin zeroes for the lane's next frame
        const int par = (int)((frame / (uint64_t)swr_context::NSLOT) & 1u);
        f.fill = (uint32_t*)c->lanefill[si][par].p;
        f.fill_next = (uint32_t*)c->lanefill[si][par ^ 1].p;
    } else {
        f.fill = (uint32_t*)c->ts.fillbuf[frame % TS::NFILL].p;
        f.fill_next = (uint32_t*)c->ts.fillbuf[(frame + 1) % TS::NFILL].p;
    }
    f.host_fill = c->h_pairs_dev + swr_context::PAIR_RING + 1 + (frame % swr_context::PAIR_RING);
    f.biglist = (uint4*)sl.biglist.p;
    f.color = (uint8_t*)c->color[c->fb_cur].p;
    f.depth = (float*)c->depth[c->fb_cur].p;
    const bool load = (d.flags & SWR_FLAG_LOAD) != 0;
    f.src_color = load ? (const uint8_t*)c->color[c->load_src].p : nullptr;
    f.src_depth = load ? (const float*)c->depth[c->load_src].p : nullptr;
    f.ids = (d.flags & SWR_FLAG_PRIMITIVE_IDS) ? (uint32_t*)c->ids[c->fb_cur].p : nullptr;
    f.tg = c->tg;
    memcpy(f.m, d.m, sizeof f.m);
    f.flags = d.flags;
    f.pq = d.persp ? (float4*)sl.pq.p : nullptr;
    f.blend = d.blend;
    return f;
}

// ---- draw-list frames ----------------------------------------------------------------------------------------------
// The frame of the last draw list: V = the list's total primitives, binned by k_bin<.., LIST> over (item, stream group) work units
// (fixed-stride bins) or by k_list_setup + k_scan + k_fill (exact-size bins).  Unless every item's frame slots are its stream slots,
// the raster reads the frame's own copies of the per-slot tables (k_list_gather).
void make_list_frame(swr_context* c, int si, const swr_context::DrawRecord& d, DeviceFrame& f) {
    swr_context::Slot& sl = c->slot[si];
    f.ntri = d.list_tris;
    f.items = (const ListItem*)sl.items.p;
    f.nitems = (int32_t)d.list.size();
    f.units = d.list_units;
    f.list_affine = d.list_affine ? 1 : 0;
    f.fixed_bins = (c->fixed_mode && f.ntri > 0) ? 1 : 0;
    f.plan = plan_frame(c, f.ntri, f.units * 64, (f.units + 7) / 8, true);
    if (!d.list_identity && f.ntri > 0) {
        f.reordered = 1;                    // keys carry order numbers; inv maps them to frame slots
        f.inv = (const uint32_t*)sl.linv.p;
        f.gather.rgb = (const float4*)c->tri_rgb.p; f.gather.nrm = (const float4*)c->tri_nrm.p;
        f.gather.inv_out = (uint32_t*)sl.linv.p;
        // (sized by swr_draw_list for the flags and material of the list; a material set after it is not the list's)
        const size_t need = (size_t)f.ntri * 48;
        if (!(f.flags & SWR_FLAG_NO_COLOR) && sl.lrgb.bytes >= need) {
            f.tri_rgb = f.gather.rgb_out = (float4*)sl.lrgb.p;
            if (c->material.shader != SWR_SHADER_PASSTHROUGH && sl.lnrm.bytes >= need) f.tri_nrm = f.gather.nrm_out = (float4*)sl.lnrm.p;
        }
    }
}

// the slots of a clip frame: n + 2F, at most 3n (each triangle gives at most three)
inline int64_t clip_slots(const swr_context* c) { const int64_t n = c->last_draw.clip_n; return std::min<int64_t>(3 * n, n + 2 * c->clip_fan); }

// ---- depth-clip frames ----------------------------------------------------------------------------------------------
// The frame over the clip stream of its lane: n + 2F slots (n submitted triangles, of the scene or of the draw list), the identity
// transform, slot = order number.  The pre-pass (launch_clip_prep) reads the scene's stream with the frame's transform(s) — a draw
// list's items from the device copy staged for the frame — and the frame itself is binned like a scene of n + 2F primitives.
void make_clip_frame(swr_context* c, int si, uint64_t frame, const swr_context::DrawRecord& d, DeviceFrame& f) {
    swr_context::Slot& sl = c->slot[si];
    ClipPrep& p = f.clip;
    p.src_xyz = (const float4*)c->tri_xyz.p;
    p.src_rgb = (const float4*)c->tri_rgb.p;
    p.src_nrm = c->has_attrs ? (const float4*)c->tri_nrm.p : nullptr;
    p.src_inv = (const uint32_t*)c->inv.p;
    p.src_reordered = c->reordered ? 1 : 0;
    p.n = d.clip_n;
    p.bound = clip_slots(c);
    p.over = c->h_clip_dev + (frame % swr_context::PAIR_RING);
    memcpy(p.m, f.m, sizeof p.m);
    p.items = d.is_list ? f.items : nullptr;
    p.nitems = d.is_list ? f.nitems : 0;
    p.sums = (uint32_t*)sl.csums.p;
    p.xyz = (float4*)sl.cxyz.p; p.rgb = (float4*)sl.crgb.p;
    p.nrm = p.src_nrm ? (float4*)sl.cnrm.p : nullptr;
    p.map = (uint32_t*)sl.cmap.p; p.box = (float4*)sl.cbox.p;
    p.pq = f.pq;                        // (k_clip_emit fills the perspective table of the clip stream's slots)
    // the frame itself: a plain (not a list) frame over the clip stream
    f.items = nullptr; f.nitems = 0; f.units = 0; f.list_affine = 0;
    f.gather = {};
    f.tri_xyz = p.xyz; f.tri_rgb = p.rgb; f.tri_nrm = p.nrm; f.box64 = p.box;
    f.inv = nullptr; f.reordered = 0;
    for (int k = 0; k < 16; k++) f.m[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    f.ntri = p.bound;
    // order numbers are dense over the post-clip count: below the slot count, or below the count itself when the host needed it
    f.order_space = c->clip_total >= 0 ? std::max<int64_t>(c->clip_total, 1) : std::max<int64_t>(p.bound, 1);
    // (32-bit depth keys: the clip frame's zero depths on the near plane are its own; they do not move the scene's state)
    f.redo_dev = nullptr; f.k32 = 0;
    f.fixed_bins = (c->fixed_mode && f.ntri > 0) ? 1 : 0;
    // (the idle raise rounds DOWN here, as it always has: it differs from the scene frame's between 131 073 and 262 080 slots)
    f.plan = plan_frame(c, f.ntri, f.ntri, (f.ntri + 63) / 64 / 8, true);
}

// ---- perspective-correct interpolation ----------------------------------------------------------------------------
// Does a frame with these flags read a perspective table?  SWR_FLAG_PERSPECTIVE on a colour frame of triangles whose transform (every
// item's, for a draw list) is not affine: under an affine map every w is exactly 1, and the screen weights are what the flag gives.
inline bool persp_frame(uint32_t flags, int32_t primitive_type, bool affine) {
    return (flags & SWR_FLAG_PERSPECTIVE) && !(flags & SWR_FLAG_NO_COLOR) && primitive_type == SWR_PRIMITIVE_TRIANGLE && !affine;
}
inline bool affine_transform(const float m[16]) { return m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f; }

// Every lane's perspective table for a frame of `slots` slots (grown with every stream idle).
int ensure_persp(swr_context* c, int64_t slots) {
    LaneSizes t;
    t.add(&swr_context::Slot::pq, (size_t)std::max<int64_t>(slots, 1) * 16);
    return grow_lanes(c, t);
}

// A depth-clip frame of n submitted triangles: the lane buffers for n + 2F slots and bins that can take them (every stream idle when
// anything grows), as swr_draw_list sizes them for a list of n + 2F triangles; the post-clip count first when the PLAIN switch needs it.
int prepare_clip(swr_context* c, int64_t n, uint32_t flags, const float* m) {
    if (n > (int64_t)SWR_DEPTH_CLIP_MAX_TRIANGLES)
        return fail(c, SWR_ERR_UNSUPPORTED, "SWR_FLAG_DEPTH_CLIP: %lld triangles (at most %d)", (long long)n, SWR_DEPTH_CLIP_MAX_TRIANGLES);
    if (n != c->last_draw.clip_n || c->clip_fan <= 0) c->clip_fan = std::max<int64_t>(1024, n / 64);   // (grown by check_frames on overflow)
    c->last_draw.clip_n = n;
    int rc;
    const size_t V = (size_t)std::max<int64_t>(clip_slots(c), 1);
    const size_t S = (size_t)(n + 255) / 256 + 1;            // the pre-pass's workgroup sums + the total
    using Slot = swr_context::Slot;
    LaneSizes t;
    t.add(&Slot::geo, V * sizeof(GeomRec)); t.add(&Slot::geo_full, V * sizeof(GeomFull)); t.add(&Slot::ranges, V * sizeof(uint2));
    t.add(&Slot::cxyz, V * 48); t.add(&Slot::crgb, V * 48);
    if (c->has_attrs && c->tri_nrm.p) t.add(&Slot::cnrm, V * 48);
    t.add(&Slot::cmap, V * 4); t.add(&Slot::cbox, (V + 63) / 64 * 32); t.add(&Slot::csums, S * 4);
    if ((rc = grow_lanes(c, t))) return rc;
    // (no submitted triangle: no slot, nothing to bin; the binning size is a whole number of 64-slot groups)
    if ((rc = fit_bins(c, clip_slots(c), ((int64_t)V + 63) / 64 * 64))) return rc;
    // The PLAIN / winner-table switch of the raster is judged on the post-clip count.  Below the threshold with all n + 2F slots
    // it needs nothing; otherwise the host counts first (every stream idle, the count kernels alone, one wait): a scene of about
    // 2^20 triangles or more, and only when its slot count reaches the threshold.
    c->clip_total = -1;
    const int64_t thr = ((int64_t)1 << 20) + ((flags & SWR_FLAG_LOAD) ? 0 : 1);
    if (n > 0 && (int64_t)V >= thr) {
        if ((rc = sync_streams(c))) return rc;
        // (m == NULL, a draw list: its items reach the device with the frame (stage_list), so its count is not known here: the bound holds)
        if (m) {
            DeviceFrame f{};
            f.vertices = (const swr_vertex*)c->vertices.p;
            f.tri_xyz = (const float4*)c->tri_xyz.p;
            f.tri_rgb = (const float4*)c->tri_rgb.p;
            f.tri_nrm = (const float4*)c->tri_nrm.p;
            f.inv = (const uint32_t*)c->inv.p;
            f.reordered = c->reordered ? 1 : 0;
            f.tg = c->tg;
            memcpy(f.m, m, sizeof f.m);
            make_clip_frame(c, 0, c->frame_no, c->last_draw, f);
            f.clip.count_only = 1;
            launch_bin(f, c->stream, nullptr);
            const int64_t nb = (n + 255) / 256;
            HIP_TRY(c, hipMemcpyAsync(&c->h_clip[swr_context::PAIR_RING], f.clip.sums + nb, 4, hipMemcpyDeviceToHost, c->stream));
            if ((rc = wait_stream(c, c->stream, "the depth-clip count"))) return or_sticky(c, rc);
            c->clip_total = (int64_t)c->h_clip[swr_context::PAIR_RING];
        }
    }
    return SWR_OK;
}

// What the binning share of a draw-list frame enqueues in front of its binning, on the frame's stream (captured by value: in the
// two-stream pipeline a helper thread enqueues it later).
struct ListPrep {
    bool on = false;
    void* dev = nullptr; const void* host = nullptr; size_t bytes = 0;
    hipEvent_t copied = nullptr;
};

// The item table into the slot's pinned staging.  The staging is rewritten only once the copy that last read it has completed: in the
// two-stream pipeline that copy is enqueued by the binning helper, so its binning share has to be on the stream first.
int stage_list(swr_context* c, int si, uint64_t frame, ListPrep& lp) {
    swr_context::Slot& sl = c->slot[si];
    int rc;
    if (!sl.items_copied) HIP_TRY(c, sl.items_copied.create(hipEventDisableTiming));
    if (sl.items_recorded && sl.items_frame < frame) {      // (a frame number posted again after a failed post: it never copied)
        if (sched_of(c) != Sched::Lanes && (rc = wait_counter(c, c->bin_enqueued, sl.items_frame, "the binning share of an earlier draw list"))) return rc;
        if ((rc = poll_event(c, sl.items_copied, "the copy of an earlier frame's draw list", sl.items_frame))) return rc;
        sl.items_recorded = false;
    }
    const size_t n = c->last_draw.list.size();
    if (sl.items_cap < n) {
        sl.items_cap = 0;
        HIP_TRY(c, sl.items_host.reset());
        const size_t want = std::max<size_t>(64, n);
        HIP_TRY(c, sl.items_host.alloc(want * sizeof(ListItem), hipHostMallocDefault));
        sl.items_cap = want;
    }
    if (n) memcpy(sl.items_host, c->last_draw.list.data(), n * sizeof(ListItem));
    sl.items_recorded = true;
    sl.items_frame = frame;
    lp.on = true;
    lp.dev = sl.items.p; lp.host = sl.items_host; lp.bytes = n * sizeof(ListItem);
    lp.copied = sl.items_copied;
    return SWR_OK;
}

int enqueue_list_prep(swr_context* c, const ListPrep& lp, hipStream_t s) {
    if (!lp.on) return SWR_OK;
    if (lp.bytes) HIP_TRY(c, hipMemcpyAsync(lp.dev, lp.host, lp.bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipEventRecord(lp.copied, s));
    return SWR_OK;
}

// read the events of every completed-but-unread frame (caller has synchronised the stream)
void harvest(swr_context* c) {
    for (; c->harvested < c->seq; c->harvested++) {
        const Event* ev = c->ev[c->harvested % swr_context::RING];
        float ms[5] = {0, 0, 0, 0, 0};
        if (c->ev_level[c->harvested % swr_context::RING] >= 2) {
            hipEventElapsedTime(&ms[0], ev[0], ev[1]);
            hipEventElapsedTime(&ms[1], ev[1], ev[2]);
            hipEventElapsedTime(&ms[2], ev[2], ev[3]);
            hipEventElapsedTime(&ms[4], ev[0], ev[4]);
        }
        hipEventElapsedTime(&ms[3], ev[3], ev[4]);
        c->last.setup_bin_ms = ms[0]; c->last.scan_ms = ms[1]; c->last.scatter_ms = ms[2];
        c->last.raster_ms = ms[3]; c->last.total_ms = ms[4];
        for (int i = 0; i < 5; i++) c->sum_ms[i] += ms[i];
        c->sum_frames++;
    }
}

// the raster (or point / clear pass) about to write framebuffer `fb` must not overtake a copy still reading it
int wait_for_copies_of(swr_context* c, int fb, hipStream_t s) {
    for (int img = 0; img < 2; img++)
        if (c->copy_recorded[fb][img]) HIP_TRY(c, hipStreamWaitEvent(s, c->copy_done[fb][img], 0));
    // ... nor a load frame of another lane still reading it as its source
    if (c->read_recorded[fb]) HIP_TRY(c, hipStreamWaitEvent(s, c->read_done[fb], 0));
    return SWR_OK;
}

// What a frame's binning chain needs besides the frame (by value: in the two-stream pipeline a helper thread enqueues it later).
struct BinChain {
    // global-atomic fallback: counters must start at zero.  Empty scene: no binning kernel runs at all, so the tile table
    // (counts, starts, counters) is simply zeroed.
    bool zero_tables = false;
    size_t zero_bytes = 0;
    bool fill_memset = false;           // fixed-stride bins: the frame's fill block is dirty (the k_bin before it took another path)
    ListPrep lp;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;    // timing level 2
};

// The binning chain of frame `f` (working set si) onto stream s: zero what must be zero, the draw list's items, then k_bin — ONE
// launch: cull, setup, histogram, region reservation, fill — or setup / scan / fill.  `stop` is bound to the chain's last kernel
// (see swr_context::bind_events); *bound = a kernel carries it.  Where k_sort_bins goes and what orders the chain against other
// streams is the scheduler's business.
int enqueue_binning(swr_context* c, const DeviceFrame& f, int si, hipStream_t s, const BinChain& b, hipEvent_t stop, bool* bound) {
    if (b.zero_tables) HIP_TRY(c, hipMemsetAsync(c->slot[si].tilebuf.p, 0, b.zero_bytes, s));
    if (b.fill_memset) HIP_TRY(c, hipMemsetAsync(f.fill, 0, (size_t)(CNT_WORDS + tiles_of(f.tg)) * 4, s));
    { const int rl = enqueue_list_prep(c, b.lp, s); if (rl) return rl; }
    if (b.e0) HIP_TRY(c, hipEventRecord(b.e0, s));
    if (f.fixed_bins) {
        *bound = launch_bin(f, s, stop);
        if (b.e1) HIP_TRY(c, hipEventRecord(b.e1, s));
        if (b.e2) HIP_TRY(c, hipEventRecord(b.e2, s));
    } else {
        launch_setup_bin(f, s);
        if (b.e1) HIP_TRY(c, hipEventRecord(b.e1, s));
        launch_scan(f, s);
        if (b.e2) HIP_TRY(c, hipEventRecord(b.e2, s));
        *bound = launch_fill(f, s, stop);
    }
    return SWR_OK;
}

// The one epilogue of a frame that went onto the streams whole, or was abandoned: every frame below `upto` counts as posted, binned and
// rastered.  A path that left a counter behind would hang wait_counter in the other scheduler after a swr_pipeline_enable toggle.  (Only
// the two-stream frame advances them share by share.)  Sequentially consistent stores: the strongest order any of these sites used.
void mark_posted(swr_context* c, uint64_t upto) { c->posted = upto; c->bin_enqueued.store(upto); c->ras_enqueued.store(upto); }

// An empty band (a group with more sub-contexts than tile rows hands these out): nothing to bin, raster or copy
int enqueue_empty_frame(swr_context* c) {
    if (const int rc = flush_raster(c, c->frame_no)) return rc;
    fill_word(c, c->frame_no) = 0;
    c->frame_load[c->frame_no % swr_context::PAIR_RING] = false;     // (no pixels: nothing it could load wrongly)
    pair_word(c, c->frame_no++) = 0;
    mark_posted(c, c->frame_no);
    c->draw_pending = true;
    return SWR_OK;
}

// .vertices / .line: three small kernels on the raster stream with every stream idle, no binning; the pair counter reads 0
int enqueue_points_frame(swr_context* c, const swr_context::DrawRecord& d) {
    int rc = sync_streams(c); if (rc) return rc;
    const bool lanes = sched_of(c) == Sched::Lanes, load = (d.flags & SWR_FLAG_LOAD) != 0;
    const uint64_t frame = c->frame_no++;
    DeviceFrame f = make_frame(c, 0, frame, d);
    pair_word(c, frame) = 0; fill_word(c, frame) = 0;
    c->frame_load[frame % swr_context::PAIR_RING] = load;
    if ((rc = wait_for_copies_of(c, c->fb_cur, c->stream))) return rc;
    launch_points_or_lines(f, d.prim, c->stream);
    if (load && lanes) {
        HIP_TRY(c, hipEventRecord(c->read_done[c->load_src], c->stream));
        c->read_recorded[c->load_src] = true;
    }
    HIP_TRY(c, hipGetLastError());
    mark_posted(c, c->frame_no);
    c->draw_pending = true;
    c->last_stream = c->stream;
    if (lanes) c->fb_cur = (c->fb_last + 1) % swr_context::NFB;
    return SWR_OK;
}

// *ev = the set of timing events of the frame about to be posted (swr_timing_enable), NULL when it is not timed
int claim_timing_events(swr_context* c, const Event** ev) {
    *ev = nullptr;
    if (c->timing < 2 && !(c->timing == 1 && (c->frame_no % (uint64_t)c->timing_every) == 0)) return SWR_OK;
    if (c->seq - c->harvested >= (uint64_t)swr_context::RING) { int rc = sync_streams(c); if (rc) return rc; harvest(c); }   // ring full: drain it
    *ev = c->ev[c->seq % swr_context::RING];
    c->ev_level[c->seq++ % swr_context::RING] = c->timing;
    return SWR_OK;
}

// frame_policy (swr_frame_policy.h) on the context's pinned words, into the frame; returns whether k_sort_bins goes onto the raster stream
bool settle_policy(swr_context* c, Sched sched, DeviceFrame& f) {
    const int tiles = tiles_of(c->tg);
    // (words the GPU overwrites while frames are in flight: read them as what they are, relaxed atomics)
    const uint32_t fullest = __atomic_load_n(&c->h_pairs[swr_context::PAIR_RING], __ATOMIC_RELAXED);
    const uint32_t redo = __atomic_load_n(&c->h_pairs[2 * swr_context::PAIR_RING + 1], __ATOMIC_RELAXED);
    FramePolicy p = frame_policy(fullest, redo, tiles, f.ntri, f.flags, f.k32 != 0, sched == Sched::TwoStream);
    if (p.k32_give_up) c->k32_ok = false;
    f.k32 = p.k32 ? 1 : 0;
    policy_insort(p, tiles, frame_uses_k32(f), c->dbg_insort);
    f.skip_sort = p.skip_sort ? 1 : 0; f.defer_big = p.defer_big ? 1 : 0; f.insort = p.insort ? 1 : 0;
    return p.sort_on_raster_stream;
}

// Fixed-stride bins: the frame's fill block must be zero when k_bin starts (the k_bin before it did that, unless that frame took
// another path); k_bin leaves it dirty and zeroes the next frame's.  Returns whether the frame has to memset its block first.
bool claim_fill_block(swr_context* c, Sched sched, int si, uint64_t frame) {
    const int k = sched == Sched::Lanes ? (int)((frame / (uint64_t)swr_context::NSLOT) & 1u) : (int)(frame % TS::NFILL);
    bool* dirty = sched == Sched::Lanes ? c->lanefill_dirty[si] : c->ts.fill_dirty;
    const bool was = dirty[k];
    dirty[k] = true;
    dirty[sched == Sched::Lanes ? k ^ 1 : (k + 1) % TS::NFILL] = false;
    return was;
}

// ---- FRAME LANES: the whole frame, binning and raster, back to back on the lane's stream (see swr_context::lane_stream) ----------
// nothing was enqueued for the frame: the context has failed (fatal) or the call reports
int abandon_frame(swr_context* c, uint64_t frame, int rc) { mark_posted(c, frame + 1); return rc; }
// an un-waited burst is paced by markers: at most ~4 * PACE_EVERY frames in flight
int pace_burst(swr_context* c, uint64_t frame) {
    constexpr uint64_t E = swr_context::PACE_EVERY;
    if (frame % E != 0 || frame < 3 * E) return SWR_OK;
    const uint64_t old = frame - 3 * E;
    const int ko = (int)((frame / E + 1) % 4);          // the marker of `old`: (k - 3) mod 4
    if (c->pace_frame[ko] != old || old < c->synced_upto) return SWR_OK;
    return poll_event(c, c->pace_ev[ko], "an earlier frame of the burst", old);
}

// what the frame puts on its lane S: the binning chain, k_sort_bins, the raster, and the markers behind it
int enqueue_lane_chain(swr_context* c, const DeviceFrame& f, int si, uint64_t frame, hipStream_t S, const BinChain& bc, const Event* ev, bool src_wait) {
    bool bound;
    { const int rb = enqueue_binning(c, f, si, S, bc, nullptr, &bound); if (rb) return rb; }
    if (!f.skip_sort) launch_sort_bins(f, S, nullptr);
    if (src_wait) HIP_TRY(c, hipStreamWaitEvent(S, c->src_ready, 0));
    if (ev) HIP_TRY(c, hipEventRecord(ev[3], S));
    launch_raster(f, S, nullptr);
    if (ev) HIP_TRY(c, hipEventRecord(ev[4], S));
    if (f.flags & SWR_FLAG_LOAD) {
        HIP_TRY(c, hipEventRecord(c->read_done[c->load_src], S));
        c->read_recorded[c->load_src] = true;
    }
    if (frame % (uint64_t)swr_context::PACE_EVERY == 0) {
        const int k = (int)((frame / (uint64_t)swr_context::PACE_EVERY) % 4);
        HIP_TRY(c, hipEventRecord(c->pace_ev[k], S));
        c->pace_frame[k] = frame;
    }
    HIP_TRY(c, hipGetLastError());
    return SWR_OK;
}

int enqueue_lane_frame(swr_context* c, const DeviceFrame& f, int si, uint64_t frame, const BinChain& bc, const Event* ev) {
    hipStream_t S = c->lane_stream[si];
    const int inj = c->inject.exchange(0, std::memory_order_relaxed);      // swr_debug_fault
    if (inj == SWR_FAULT_ENQUEUE) return abandon_frame(c, frame, fatal(c, SWR_ERR_HIP, "frame %llu: injected enqueue failure (swr_debug_fault)", (unsigned long long)frame));
    int rc = inj != SWR_FAULT_LOST_EVENT ? SWR_OK : poll_event(c, c->slot[si].bin_done, "the lane's previous frame (injected: a completion that never arrives)", frame, true);
    if (!rc) rc = pace_burst(c, frame);
    if (!rc) rc = wait_for_copies_of(c, c->fb_cur, S);
    if (rc) return abandon_frame(c, frame, rc);
    // a load frame: its raster starts after the raster of the frame it loads (the previous one, on another lane); its binning
    // still overlaps that raster
    const bool src_wait = (f.flags & SWR_FLAG_LOAD) && c->last_stream && c->last_stream != S;
    if (src_wait && hipEventRecord(c->src_ready, c->last_stream) != hipSuccess)
        return abandon_frame(c, frame, fatal(c, SWR_ERR_HIP, "frame %llu: recording the source frame's completion failed", (unsigned long long)frame));
    if ((rc = enqueue_lane_chain(c, f, si, frame, S, bc, ev, src_wait)))
        return abandon_frame(c, frame, fatal(c, rc, "enqueueing frame %llu failed: %s", (unsigned long long)frame, c->err.c_str()));
    c->draw_pending = true;
    mark_posted(c, frame + 1);
    c->last_stream = S;
    c->fb_cur = (c->fb_last + 1) % swr_context::NFB;      // the next frame (another lane) renders into its own buffer
    return SWR_OK;
}

// ---- THE TWO-STREAM PIPELINE, and one stream (swr_context::TwoStream) -------------------------------------------------------------
// What the binning stream's share of a frame needs, by value: a helper thread may enqueue it later.
struct BinShare {
    DeviceFrame f; BinChain bc; uint64_t frame; int si;
    hipStream_t sb;                     // the binning stream
    bool two_streams, sort_on_raster_stream, slot_wait, paced;
};

// The binning stream's share of frame b.frame (caller's thread or bin_worker).
int bin_share(swr_context* c, const BinShare& b) {
    swr_context::Slot& sl = c->slot[b.si];
    if (b.slot_wait) {
        // the first event-carrying raster at or after that frame (RAS_EVERY); its event must have been bound /
        // recorded (by ras_worker or the caller's thread) before it is polled / waited for
        const uint64_t prev = b.frame - (uint64_t)swr_context::NSLOT;
        const uint64_t ef = prev + (uint64_t)(TS::RAS_EVERY - 1) - prev % (uint64_t)TS::RAS_EVERY;
        { const int rc = wait_counter(c, c->ras_enqueued, ef, "the raster of an earlier frame"); if (rc) return rc; }
        const TS::RasDone& rd = c->ts.ras_done[ef % (uint64_t)swr_context::NSLOT];
        if (rd.frame == ef) {
            if (b.paced) { const int rc = poll_event(c, rd.ev, "k_raster (its working set is needed again)", ef); if (rc) return rc; }
            else HIP_TRY(c, hipStreamWaitEvent(b.sb, rd.ev, 0));
        }
    }
    // bin_done = the completion of the chain's last kernel itself (bound at launch) where there is one
    hipEvent_t stop = (b.two_streams && c->ts.bind_events) ? sl.bin_done.h : nullptr;
    bool bound;
    { const int rb = enqueue_binning(c, b.f, b.si, b.sb, b.bc, (b.sort_on_raster_stream || b.f.skip_sort) ? stop : nullptr, &bound); if (rb) return rb; }
    if (!b.sort_on_raster_stream && !b.f.skip_sort) bound = launch_sort_bins(b.f, b.sb, stop);
    if (b.two_streams && !bound) HIP_TRY(c, hipEventRecord(sl.bin_done, b.sb));
    HIP_TRY(c, hipGetLastError());
    return SWR_OK;
}

// bin_share as the helpers' job: ANY failure fails the context, and bin_enqueued still advances (the raster share waits on it)
int bin_job(swr_context* c, const BinShare& b) {
    int rc = c->failed.load(std::memory_order_acquire);
    if (!rc) rc = bin_share(c, b);
    if (rc) {
        fatal(c, rc, "enqueueing the binning of frame %llu failed: %s", (unsigned long long)b.frame, tl_helper_thread ? "(helper thread)" : c->err.c_str());
        c->ts.bin_error.store(rc, std::memory_order_relaxed);
    }
    c->bin_enqueued.store(b.frame + 1, std::memory_order_release);
    return rc;
}

// Binning onto bin_stream, raster onto `stream` (one stream: the same), each share enqueued by a helper thread or by the caller's own.
int enqueue_two_stream_frame(swr_context* c, Sched sched, const DeviceFrame& f, int si, uint64_t frame, const BinChain& bc, const Event* ev,
                             bool sort_on_raster_stream) {
    TS& ts = c->ts;
    const bool two = sched == Sched::TwoStream;
    c->last_stream = c->stream;
    // this slot's buffers are free again once the raster of NSLOT frames ago has read them (a full sync since then
    // settles it: every non-pipelined path syncs first)
    const bool slot_wait = two && frame >= (uint64_t)swr_context::NSLOT && frame - (uint64_t)swr_context::NSLOT >= c->synced_upto;
    // helpers or the caller's own thread?  (idle context: every earlier frame is complete)
    const bool streaming = two && (ts.bin_worker || ts.ras_worker) && !(ts.inline_idle && c->synced_upto == c->posted);
    const bool paced = streaming && ts.ras_worker;      // cross-stream order by host polls instead of event waits
    if (frame >= (uint64_t)TS::RAS_RING) {
        const int rc = wait_counter(c, c->ras_enqueued, frame - (uint64_t)TS::RAS_RING, "the raster share of an earlier frame");
        if (rc) { c->frame_no = frame; return or_sticky(c, rc); }     // nothing was posted for this frame
    }
    TS::RasJob& rj = ts.ras_job[frame % TS::RAS_RING];
    rj.f = f; rj.ev3 = ev ? ev[3].h : nullptr; rj.ev4 = ev ? ev[4].h : nullptr; rj.si = si; rj.sort_here = sort_on_raster_stream;
    rj.fb = c->fb_cur; rj.paced = paced;
    c->draw_pending = true;   // the pair total lands in the frame's pinned word (written by the scan)
    c->posted = frame + 1;
    const BinShare share{f, bc, frame, si, c->bin_stream, two, sort_on_raster_stream, slot_wait, paced};
    if (!streaming) {
        { int rc = bin_share(c, share); if (rc) return rc; }
        c->bin_enqueued.store(frame + 1, std::memory_order_release);
        c->hp_lap(2);
        return flush_raster(c, frame + 1);
    }
    // two helpers: one enqueues this frame's binning while the other enqueues the previous frame's raster.  One
    // helper (sub-contexts of a group: the group's per-device thread is this thread): the binning share runs here.
    if (ts.bin_worker) ts.bin_worker->post([c, share]() -> int { return bin_job(c, share); });
    else (void)bin_job(c, share);            // a failure is picked up by the raster share (bin_error) and by the next blocking call
    c->hp_lap(2);
    if (ts.ras_worker) {
        ts.ras_worker->post([c, frame]() -> int { return enqueue_raster_shares(c, frame + 1); });
        return SWR_OK;
    }
    return flush_raster(c, frame);            // frames < frame; this one follows with the next draw / sync / present
}

// (exact-size bins only: never on the single-launch path) the count matrix of the LDS binning walk, for every lane
int ensure_bin_matrix(swr_context* c) {
    const BinPlan plan = plan_binning(c->ni / 3, tiles_of(c->tg), c->dbg_bin_mode == 3);
    if (!plan.use_lds || c->fixed_mode) return SWR_OK;
    LaneSizes t;
    t.add(&swr_context::Slot::bin_matrix, (size_t)plan.G * (size_t)tiles_of(c->tg) * 4);
    return grow_lanes(c, t);
}

// Post the frame of the last draw (c->last_draw: swr_draw / swr_draw_list through end_draw, or its redo after an overflow).
int enqueue_frame(swr_context* c) {
    if (const int f = sticky(c)) return f;      // a failed context posts nothing more
    c->hp_begin();
    const swr_context::DrawRecord& d = c->last_draw;
    int rc = ensure_bin_matrix(c);
    if (rc) return rc;
    c->fb_last = c->fb_cur;
    if (tiles_of(c->tg) == 0) return enqueue_empty_frame(c);
    if (d.prim != SWR_PRIMITIVE_TRIANGLE) return enqueue_points_frame(c, d);
    const Sched sched = sched_of(c);
    const uint64_t frame = c->frame_no++;
    c->frame_presented[frame % swr_context::PAIR_RING] = false;
    c->frame_load[frame % swr_context::PAIR_RING] = (d.flags & SWR_FLAG_LOAD) != 0;
    const int si = c->last_slot = (int)(frame % swr_context::NSLOT);
    DeviceFrame f = make_frame(c, si, frame, d);
    BinChain bc;
    if (d.is_list) {
        make_list_frame(c, si, d, f);
        if ((rc = stage_list(c, si, frame, bc.lp))) { c->frame_no = frame; return rc; }
    }
    c->h_clip[frame % swr_context::PAIR_RING] = 0u;
    if (d.clip) make_clip_frame(c, si, frame, d, f);
    const Event* ev = nullptr;
    if ((rc = claim_timing_events(c, &ev))) return rc;
    c->hp_lap(0);
    const bool sort_on_raster_stream = settle_policy(c, sched, f);
    if (f.ntri <= 0) { if ((rc = sync_streams(c))) return rc; pair_word(c, frame) = 0; }
    if (!f.fixed_bins) fill_word(c, frame) = 0;
    else bc.fill_memset = claim_fill_block(c, sched, si, frame);
    bc.zero_tables = !f.fixed_bins && (!f.plan.use_lds || f.ntri <= 0);
    bc.zero_bytes = (size_t)(CNT_WORDS + 3 * tiles_of(c->tg) + 1) * 4;
    if (ev && c->timing >= 2) { bc.e0 = ev[0]; bc.e1 = ev[1]; bc.e2 = ev[2]; }
    if (sched == Sched::Lanes) return enqueue_lane_frame(c, f, si, frame, bc, ev);
    return enqueue_two_stream_frame(c, sched, f, si, frame, bc, ev, sort_on_raster_stream);
}

// Every frame below `upto` has its raster share on the raster stream when this returns.
int flush_raster(swr_context* c, uint64_t upto) {
    if (c->ts.ras_worker) {                                  // every posted share (and present) has been enqueued
        const int rc = c->ts.ras_worker->drain();
        if (rc) return rc;
    }
    return enqueue_raster_shares(c, std::min(upto, c->posted));   // frames of the one-stream path (never posted)
}

// The raster stream's share of frame g (caller's thread or ras_worker).
int raster_share(swr_context* c, uint64_t g) {
    { const int rc = wait_counter(c, c->bin_enqueued, g, "the binning share"); if (rc) return rc; }
    if (c->ts.bin_error.load(std::memory_order_relaxed)) {
        const int rc = c->ts.bin_error.exchange(0);
        return rc ? rc : SWR_ERR_HIP;          // the text was recorded by the thread that failed
    }
    TS::RasJob& rj = c->ts.ras_job[g % TS::RAS_RING];
    swr_context::Slot& sl = c->slot[rj.si];
    TS::RasDone& rd = c->ts.ras_done[rj.si];
    hipStream_t sr = c->stream;
    const bool two = sched_of(c) != Sched::OneStream;      // (never Lanes: a lane frame has no raster share)
    const int inj = c->inject.exchange(0, std::memory_order_relaxed);      // swr_debug_fault
    if (inj == SWR_FAULT_ENQUEUE) return fatal(c, SWR_ERR_HIP, "frame %llu: injected enqueue failure (swr_debug_fault)", (unsigned long long)g);
    c->hp_begin_r();
    if ((two && rj.paced) || inj == SWR_FAULT_LOST_EVENT) {
        const int rc = poll_event(c, sl.bin_done, "the binning (k_bin / k_sort_bins)", g, inj == SWR_FAULT_LOST_EVENT);
        if (rc) return rc;
    } else if (two) HIP_TRY(c, hipStreamWaitEvent(sr, sl.bin_done, 0));
    c->hp_lap_r(3);
    { int rc = wait_for_copies_of(c, rj.fb, sr); if (rc) return rc; }
    if (rj.sort_here) launch_sort_bins(rj.f, sr);
    if (rj.ev3) HIP_TRY(c, hipEventRecord(rj.ev3, sr));
    const bool carries = two && g % (uint64_t)TS::RAS_EVERY == (uint64_t)(TS::RAS_EVERY - 1);
    const bool bound = launch_raster(rj.f, sr, (carries && c->ts.bind_events) ? rd.ev.h : nullptr);
    if (rj.ev4) HIP_TRY(c, hipEventRecord(rj.ev4, sr));
    c->hp_lap_r(4);
    if (carries) { if (!bound) HIP_TRY(c, hipEventRecord(rd.ev, sr)); rd.frame = g; }
    c->hp_lap_r(5);
    c->hp_frames++;
    HIP_TRY(c, hipGetLastError());
    return SWR_OK;
}

// The raster shares of every frame below `upto` that have not been enqueued yet.  ANY failure fails the context and
// still advances ras_enqueued: the binning helper (slot wait), swr_draw (back-pressure) and the destructor wait on it.
int enqueue_raster_shares(swr_context* c, uint64_t upto) {
    for (;;) {
        const uint64_t g = c->ras_enqueued.load(std::memory_order_relaxed);
        if (g >= upto) return SWR_OK;
        int rc = c->failed.load(std::memory_order_acquire);
        if (!rc) rc = raster_share(c, g);
        if (rc) {
            // (no-op when the cause has been recorded already: a helper's HIP_TRY, an expired wait)
            fatal(c, rc, "enqueueing the raster of frame %llu failed: %s", (unsigned long long)g, tl_helper_thread ? "(helper thread)" : c->err.c_str());
            c->ras_enqueued.store(std::max(upto, g + 1), std::memory_order_release);
            return rc;
        }
        c->ras_enqueued.store(g + 1, std::memory_order_release);
    }
}

// Is `p` page-locked memory HIP knows (hipHostMalloc / hipHostRegister)?  Then hipMemcpyAsync into it is a true
// asynchronous DMA; anything else would be staged by the runtime and block the caller.
bool is_pinned(const void* p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // unknown pointer = plain pageable memory: not an error
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

int ensure_stage(swr_context* c, int img) {
    for (int k = 0; k < 2; k++) {
        if (!c->stage[img][k]) HIP_TRY(c, c->stage[img][k].alloc(swr_context::STAGE_BYTES, hipHostMallocDefault));
        if (!c->stage_ev[img][k]) HIP_TRY(c, c->stage_ev[img][k].create(hipEventDisableTiming));
    }
    return SWR_OK;
}

// The band's image `img` (0 colour, 1 depth, 2 IDs) in framebuffer `fb`
inline const void* fb_image(const swr_context* c, int fb, int img) {
    return img == 0 ? c->color[fb].p : img == 1 ? c->depth[fb].p : c->ids[fb].p;
}

// Enqueue the copy of a band-local device image `src_band` — rows of `row` bytes: a framebuffer image of `fb` (fb_image), or the
// band's resolved image computed from it — into rows [r0, r1) of the caller's host image (rows of the same pitch: for a framebuffer
// image the band's [row_begin, row_end) of the full-size image), on copy stream `img` (0 the colour's, 1 the depth's: the ID image
// rides on the depth's, through its staging), behind frame_done[fb].
// Page-locked destination: ONE hipMemcpyAsync straight into the caller's rows (returns at once).  Pageable
// destination: pipelined through two pinned 8 MiB chunks (D2H of chunk k+1 overlaps the memcpy of chunk k; blocks).
int copy_band(swr_context* c, int fb, int img, const void* src_band, size_t row, int64_t r0, int64_t r1, void* dst_full, uint64_t frame) {
    const size_t bytes = (size_t)(r1 - r0) * row;
    if (!bytes) return SWR_OK;
    uint8_t* dst = (uint8_t*)dst_full + (size_t)r0 * row;
    const uint8_t* src = (const uint8_t*)src_band;
    hipStream_t s = c->copy_stream[img];
    HIP_TRY(c, hipStreamWaitEvent(s, c->frame_done[fb], 0));
    if (is_pinned(dst)) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    } else {
        int rc = ensure_stage(c, img);
        if (rc) return rc;
        const size_t CH = swr_context::STAGE_BYTES;
        const size_t n = (bytes + CH - 1) / CH;
        for (size_t k = 0; k <= n; k++) {
            if (k < n) {
                const size_t len = std::min(CH, bytes - k * CH);
                HIP_TRY(c, hipMemcpyAsync(c->stage[img][k & 1], src + k * CH, len, hipMemcpyDeviceToHost, s));
                HIP_TRY(c, hipEventRecord(c->stage_ev[img][k & 1], s));
            }
            if (k > 0) {
                const size_t j = k - 1, len = std::min(CH, bytes - j * CH);
                { const int rcw = poll_event(c, c->stage_ev[img][j & 1], "a staged copy to the host", frame); if (rcw) return rcw; }
                memcpy(dst + j * CH, c->stage[img][j & 1], len);
            }
        }
    }
    HIP_TRY(c, hipEventRecord(c->copy_done[fb][img], s));
    c->copy_recorded[fb][img] = true;
    return SWR_OK;
}

// ---- single-device implementations of the entry points ----------------------------------------------------------
int check_frames(swr_context* c);
int enqueue_present(swr_context* c, void* color_full, float* depth_full);
int prefill_sparse(swr_context* c, bool positions, bool attrs);

// Skinned meshes and morph targets.  Enqueue on c->stream (every stream idle) what puts the triangle stream —
// positions, the normals when with_nrm, the group boxes — into the context's shape: the morph (of sparse or of dense targets, whichever
// kind is resident) when a weight is not zero, then the pose
// reading the morphed arrays, then the stream from whichever array is last.  With neither, back to what the upload built, bit for bit.
int enqueue_pose(swr_context* c, bool with_nrm) {
    const int64_t ntri = c->ni / 3;
    int rc;
    // computed normals take effect while the scene has attributes: the vertex passes then leave the normals out
    // (their NRM = false variants), and the normals come from the positions that are last, between the vertex passes and the stream
    const int32_t computed = with_nrm ? c->normals_mode : SWR_NORMALS_UPLOADED;
    const bool flip = (c->normals_flags & SWR_NORMALS_FLIP) != 0;
    const bool vnrm = with_nrm && computed == SWR_NORMALS_UPLOADED;     // the vertex passes carry the uploaded normals along
    const swr_vertex* v = (const swr_vertex*)c->vertices.p;
    const swr_vertex_attr* at = vnrm ? (const swr_vertex_attr*)c->attrs.p : nullptr;
    if (c->morph_active && c->morph_sparse) {
        // sparse targets: the touched vertices are rewritten from the base; everywhere else the morphed arrays hold the pre-fill
        const bool mnrm = vnrm && c->morph_has_nrm;
        if (c->morph_touched_count > 0) {
            HIP_TRY(c, hipMemcpyAsync(c->morph_w_dev.p, c->morph_w.data(), c->morph_w.size() * 4, hipMemcpyHostToDevice, c->stream));
            MorphSparseArgs a{};
            a.vertices = v; a.attrs = mnrm ? at : nullptr;
            a.touched = (const uint32_t*)c->morph_touched.p; a.row = (const int64_t*)c->morph_row.p;
            a.dpos = (const MorphSparseEntry*)c->morph_dpos.p; a.dnrm = mnrm ? (const MorphSparseEntry*)c->morph_dnrm.p : nullptr;
            a.weights = (const float*)c->morph_w_dev.p; a.touched_count = c->morph_touched_count; a.targets = c->morph_targets;
            a.morphed = (swr_vertex*)c->morphed.p; a.morphed_attrs = mnrm ? (swr_vertex_attr*)c->morphed_attrs.p : nullptr;
            launch_morph_sparse(a, c->stream);
        }
        v = (const swr_vertex*)c->morphed.p;
        if (mnrm) at = (const swr_vertex_attr*)c->morphed_attrs.p;
    } else if (c->morph_active) {
        const bool mnrm = vnrm && c->morph_has_nrm;             // (else the normals stay as uploaded)
        c->morph_list.clear();
        for (int32_t t = 0; t < c->morph_targets; t++)
            if (c->morph_w[t] != 0.0f) c->morph_list.push_back(MorphEntry{(uint32_t)t, c->morph_w[t]});
        if ((rc = ensure(c, c->morphed, (size_t)c->nv * sizeof(swr_vertex)))) return rc;
        if (mnrm && (rc = ensure(c, c->morphed_attrs, (size_t)c->nv * sizeof(swr_vertex_attr)))) return rc;
        if ((rc = ensure(c, c->morph_list_dev, c->morph_list.size() * sizeof(MorphEntry)))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->morph_list_dev.p, c->morph_list.data(), c->morph_list.size() * sizeof(MorphEntry),
                                  hipMemcpyHostToDevice, c->stream));
        launch_morph_vertices(v, mnrm ? at : nullptr, c->nv, (const float*)c->morph_dpos.p, (const float*)c->morph_dnrm.p,
                              (const MorphEntry*)c->morph_list_dev.p, (int32_t)c->morph_list.size(), (swr_vertex*)c->morphed.p,
                              (swr_vertex_attr*)c->morphed_attrs.p, c->stream);
        v = (const swr_vertex*)c->morphed.p;
        if (mnrm) at = (const swr_vertex_attr*)c->morphed_attrs.p;
    }
    if (c->pose_active) {
        if ((rc = ensure(c, c->posed, (size_t)c->nv * sizeof(swr_vertex)))) return rc;
        if (vnrm && (rc = ensure(c, c->posed_nrm, (size_t)c->nv * 16))) return rc;
        if ((rc = ensure(c, c->pose_dev, c->pose.size() * 4))) return rc;
        if (!c->pose.empty())
            HIP_TRY(c, hipMemcpyAsync(c->pose_dev.p, c->pose.data(), c->pose.size() * 4, hipMemcpyHostToDevice, c->stream));
        if (c->pose_dq)
            launch_skin_vertices_dq(v, at, (const swr_skin_vertex*)c->skin.p, c->nv, (const float*)c->pose_dev.p,
                                    (int32_t)(c->pose.size() / 8), (swr_vertex*)c->posed.p, (float4*)c->posed_nrm.p, c->stream);
        else
            launch_skin_vertices(v, at, (const swr_skin_vertex*)c->skin.p, c->nv, (const float*)c->pose_dev.p,
                                 (int32_t)(c->pose.size() / 16), (swr_vertex*)c->posed.p, (float4*)c->posed_nrm.p, c->stream);
        v = (const swr_vertex*)c->posed.p;
    }
    if (computed != SWR_NORMALS_UPLOADED) {
        // `v` is the vertex array the frame draws: the scene's, the morphed or the posed one
        if (computed == SWR_NORMALS_SMOOTH) {
            if ((rc = ensure(c, c->face, (size_t)ntri * 16))) return rc;
            if ((rc = ensure(c, c->auto_nrm, (size_t)c->nv * 16))) return rc;
            launch_face_normals((const float4*)v, 2, c->nv, (const int64_t*)c->indices.p, ntri, flip, (float4*)c->face.p, c->stream);
            launch_vertex_normals((const uint32_t*)c->adj_off.p, (const uint32_t*)c->adj_tri.p, (const float4*)c->face.p, c->nv,
                                  (float4*)c->auto_nrm.p, c->stream);
            launch_skin_stream((const float4*)v, 2, (const float4*)c->auto_nrm.p, 1, c->nv, (const int64_t*)c->indices.p, ntri,
                               c->reordered ? 1 : 0, (float4*)c->tri_xyz.p, (float4*)c->tri_nrm.p, (float4*)c->box64.p, c->stream);
        } else {
            launch_skin_stream((const float4*)v, 2, nullptr, 1, c->nv, (const int64_t*)c->indices.p, ntri, c->reordered ? 1 : 0,
                               (float4*)c->tri_xyz.p, nullptr, (float4*)c->box64.p, c->stream);
            launch_flat_normals((const float4*)c->tri_xyz.p, ntri, flip, (float4*)c->tri_nrm.p, c->stream);
        }
    } else if (c->pose_active) {
        launch_skin_stream((const float4*)c->posed.p, 2, with_nrm ? (const float4*)c->posed_nrm.p : nullptr, 1, c->nv,
                           (const int64_t*)c->indices.p, ntri, c->reordered ? 1 : 0, (float4*)c->tri_xyz.p,
                           with_nrm ? (float4*)c->tri_nrm.p : nullptr, (float4*)c->box64.p, c->stream);
    } else {
        launch_skin_stream((const float4*)v, 2, (const float4*)at, 2, c->nv,
                           (const int64_t*)c->indices.p, ntri, c->reordered ? 1 : 0, (float4*)c->tri_xyz.p,
                           with_nrm ? (float4*)c->tri_nrm.p : nullptr, (float4*)c->box64.p, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    return SWR_OK;
}

// swr_scene_morph(NULL), a new scene: no targets of either kind, no weights; the delta planes and the rows go back to the device
void drop_morph(swr_context* c) {
    (void)c->morph_dpos.reset();
    (void)c->morph_dnrm.reset();
    (void)c->morph_touched.reset();
    (void)c->morph_row.reset();
    c->morph_sparse = false;
    c->morph_touched_count = 0;
    c->morph_targets = 0;
    c->morph_has_nrm = false;
    c->morph_active = false;
    c->morph_w.clear();
}

#ifndef SWR_TUNE_ONESHOT_CUTS
#define SWR_TUNE_ONESHOT_CUTS {70, 100}   // single_scene_upload: where a one-shot scene's index array is cut, per cent of the primitives
#endif
// oneshot: the scene is uploaded for ONE frame (swr_render without a scene identity, the reference's calling pattern):
// the triangle stream keeps index order — the Morton sort costs more than it saves a single frame (cfg4: build 0.49 ->
// 0.23 ms, the frame 0.154 -> 0.177 ms) — and it is built chunk by chunk behind the copy of the index array.
int single_scene_upload(swr_context* c, const swr_vertex* vertices, int64_t vertex_count,
                        const int64_t* indices, int64_t index_count, bool oneshot = false) {
    if (const int f = sticky(c)) return f;
    if (vertex_count < 0 || index_count < 0 || (index_count > 0 && (!indices || !vertices)))
        return fail(c, SWR_ERR_BAD_ARG, "swr_scene_upload: bad vertex/index arguments");
    if (index_count / 3 >= 0xFFFFFFFFll || vertex_count > 0xFFFFFFFFll)
        return fail(c, SWR_ERR_UNSUPPORTED, "more than 2^32-2 primitives or 2^32 vertices");
    HIP_TRY(c, hipSetDevice(c->device));
    { int rcs = check_frames(c); if (rcs) return rcs; }     // (an overflowed frame presented just before is repaired / reported first)
    c->has_scene = false;
    c->has_attrs = false;
    c->has_skin = false; c->skin_max_joint = -1;     // (a new scene has neither skin nor pose)
    c->pose_active = false; c->pose_dq = false; c->pose.clear();
    drop_morph(c);                                   // (nor morph targets)
    c->normals_mode = SWR_NORMALS_UPLOADED; c->normals_flags = 0; c->adj_built = false;   // (nor a normals mode: the adjacency is the old indices')
    c->draw_pending = false;
    c->last_draw.is_list = false;
    c->ids_valid = false;            // the IDs number the primitives of the scene that is going: swr_count_ids has no n for them any more
    c->cuts.clear();                 // a new stream is one segment
    c->list_plan_max = 0;
    c->present_pending = false;
    int rc;
    if ((rc = ensure(c, c->vertices, (size_t)vertex_count * sizeof(swr_vertex)))) return rc;
    if ((rc = ensure(c, c->indices, (size_t)index_count * 8))) return rc;
    if ((rc = ensure(c, c->tri_rgb, (size_t)index_count * 16))) return rc;
    const int64_t ntri = index_count / 3;
    // SWR_DEBUG_STREAM_ORDER 0: keep index order (the original index still travels in GeomRec.flags);
    // -1: behave as for a scene of 2^24 primitives or more (no reordering, slot == index) — test hook
    const int sort_mode = c->dbg_stream_order;
    const bool reorder = sort_mode == 1 && !oneshot && ntri > 1 && ntri < SORT_MAX_TRIS;
    const size_t sort_bytes = reorder ? stream_sort_temp_bytes(ntri) : 0;
    if ((rc = ensure(c, c->tri_xyz, (size_t)index_count * 16))) return rc;
    if ((rc = ensure(c, c->inv, (size_t)ntri * 4))) return rc;
    if ((rc = ensure(c, c->box64, (size_t)((ntri + 63) / 64) * 32))) return rc;
    if ((rc = ensure(c, c->stream_scratch, ((size_t)ntri * 4 + 8) * 4))) return rc;
    if ((rc = ensure(c, c->sort_temp, sort_bytes))) return rc;
    for (auto& sl : c->slot) {
        if ((rc = ensure(c, sl.geo, (size_t)(index_count / 3) * sizeof(GeomRec)))) return rc;
        if ((rc = ensure(c, sl.geo_full, (size_t)(index_count / 3) * sizeof(GeomFull)))) return rc;
        if ((rc = ensure(c, sl.ranges, (size_t)(index_count / 3) * sizeof(uint2)))) return rc;
        if ((rc = ensure(c, sl.biglist, (size_t)1024 * 16))) return rc;
        if ((rc = ensure(c, sl.live, (size_t)((index_count / 3 + 63) / 64 + 2 * 1024 + 2) * 4))) return rc;   // [G <= 1024][1 + per]
        if ((rc = ensure(c, sl.tilebuf, (size_t)(CNT_WORDS + 3 * std::max(1, tiles_of(c->tg)) + 1) * 4))) return rc;
    }
    for (Event& e : c->up_ev) if (!e) HIP_TRY(c, e.create());
    HIP_TRY(c, hipEventRecord(c->up_ev[0], c->stream));
    if (vertex_count)
        HIP_TRY(c, hipMemcpyAsync(c->vertices.p, vertices, (size_t)vertex_count * sizeof(swr_vertex),
                                  hipMemcpyHostToDevice, c->stream));
    StreamBuild b{};
    b.vertices = (const swr_vertex*)c->vertices.p; b.nv = vertex_count;
    b.indices = (const int64_t*)c->indices.p; b.ntri = ntri;
    b.sort = reorder;
    b.scratch = (uint32_t*)c->stream_scratch.p;
    b.sort_temp = c->sort_temp.p; b.sort_temp_bytes = sort_bytes;
    b.tri_xyz = (float4*)c->tri_xyz.p; b.tri_rgb = (float4*)c->tri_rgb.p;
    b.inv = (uint32_t*)c->inv.p; b.box64 = (float4*)c->box64.p;
    uint32_t* const bad = (uint32_t*)c->slot[0].tilebuf.p;     // CNT_BAD_INDEX lives in the first slot's counter words
    HIP_TRY(c, hipMemsetAsync(bad, 0, CNT_WORDS * 4, c->stream));
    // One-shot scenes with an index array worth cutting up (>= 4 MiB): the index check and the stream of chunk k run on
    // the binning stream while chunk k+1 is on the link (a copy from pageable memory returns when its bytes are staged)
    hipStream_t side = c->bin_stream_own.h;      // (a stream of its own, or none)
    const int64_t chunk_min = c->dbg_oneshot_min_tris;                   // (SWR_DEBUG_ONESHOT_MIN_TRIS: chunk small scenes too)
    const bool chunked = oneshot && side && sort_mode != -1 && ntri >= chunk_min && ntri < SORT_MAX_TRIS;
    if (chunked) {
        // two chunks, the second one small: every extra copy call from pageable memory costs the link ~30 us, the last
        // chunk's build is the tail (cfg4, whole call: {100} 3.10 ms, {70,100} 3.06, {50,82,100} 3.07, four quarters 3.12)
        constexpr int cuts[] = SWR_TUNE_ONESHOT_CUTS;          // per cent of the primitives
        if (!c->up_chunk_ev) HIP_TRY(c, c->up_chunk_ev.create(hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->up_chunk_ev, c->stream));           // (vertices resident, counter words zero)
        HIP_TRY(c, hipStreamWaitEvent(side, c->up_chunk_ev, 0));
        int64_t t0 = 0;
        for (const int cut : cuts) {
            const int64_t t1 = cut >= 100 ? ntri : std::min(ntri, (ntri * cut / 100 + 63) / 64 * 64);
            if (t1 <= t0) continue;
            HIP_TRY(c, hipMemcpyAsync((int64_t*)c->indices.p + 3 * t0, indices + 3 * t0, (size_t)(t1 - t0) * 24, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipEventRecord(c->up_chunk_ev, c->stream));
            HIP_TRY(c, hipStreamWaitEvent(side, c->up_chunk_ev, 0));
            launch_validate_indices((const int64_t*)c->indices.p + 3 * t0, 3 * (t1 - t0), vertex_count, bad, side);
            HIP_TRY(c, launch_build_stream_range(b, t0, t1, side));
            t0 = t1;
        }
        HIP_TRY(c, hipEventRecord(c->up_ev[1], c->stream));
        HIP_TRY(c, hipEventRecord(c->up_chunk_ev, side));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->up_chunk_ev, 0));
        c->reordered = true;                                          // (identity order; the original index travels in GeomRec.flags)
        c->stream_sorted = false;
    } else {
        if (index_count)
            HIP_TRY(c, hipMemcpyAsync(c->indices.p, indices, (size_t)index_count * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->up_ev[1], c->stream));
        // index range check (Swift array subscript would trap, Renderer.swift:226)
        launch_validate_indices((const int64_t*)c->indices.p, index_count, vertex_count, bad, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, launch_build_stream(b, c->stream));
        c->reordered = ntri > 0 && ntri < SORT_MAX_TRIS && sort_mode != -1;   // original index travels in GeomRec.flags
        c->stream_sorted = reorder;
    }
    HIP_TRY(c, hipMemcpyAsync(c->h_misc, c->slot[0].tilebuf.p, CNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->up_ev[2], c->stream));
    if ((rc = wait_stream(c, c->stream, "scene upload"))) return or_sticky(c, rc);
    (void)hipEventElapsedTime(&c->up_h2d_ms, c->up_ev[0], c->up_ev[1]);
    (void)hipEventElapsedTime(&c->up_build_ms, c->up_ev[1], c->up_ev[2]);
    if (c->h_misc[CNT_BAD_INDEX])
        return fail(c, SWR_ERR_INDEX_RANGE, "an index is outside [0, %lld)", (long long)vertex_count);
    c->nv = vertex_count;
    c->ni = index_count;
    c->has_scene = true;
    c->h_pairs[swr_context::PAIR_RING] = 0xFFFFFFFFu;       // fullest bin of the new scene: unknown (sort)
    // What earlier frames taught the context about this (primitive count, tile grid) pair survives the upload — the regions a
    // crowded tile made the host grow, a scene that needed exact bins, a scene whose depth frames belong on the 64-bit keys: the
    // reference's calling pattern uploads the SAME mesh on every call (GpuRenderer.swift:41-71), and re-learning it would cost
    // every such call a second frame.  A different primitive count starts from the first guess again.
    if (index_count / 3 != c->sized_ntri) {
        c->fixed_allowed = true;
        c->fixed_mode = false;                              // (re-sized below or at swr_target_set)
        c->k32_ok = true;
    }
    if (!c->has_target) return ensure_capacity(c, first_capacity(index_count / 3));
    return size_bins(c);
}

int single_scene_attributes(swr_context* c, const swr_vertex_attr* attributes, int64_t vertex_count) {
    if (const int f = sticky(c)) return f;
    if (!c->has_scene) return fail(c, SWR_ERR_NO_SCENE, "swr_scene_attributes needs swr_scene_upload first");
    if (vertex_count != c->nv || (vertex_count > 0 && !attributes))
        return fail(c, SWR_ERR_BAD_ARG, "swr_scene_attributes: %lld attributes for %lld vertices",
                    (long long)vertex_count, (long long)c->nv);
    HIP_TRY(c, hipSetDevice(c->device));
    { int rcs = sync_streams(c); if (rcs) return rcs; }
    int rc;
    if ((rc = ensure(c, c->attrs, (size_t)vertex_count * sizeof(swr_vertex_attr)))) return rc;
    if ((rc = ensure(c, c->tri_nrm, (size_t)c->ni * 16))) return rc;
    if (vertex_count)
        HIP_TRY(c, hipMemcpyAsync(c->attrs.p, attributes, (size_t)vertex_count * sizeof(swr_vertex_attr),
                                  hipMemcpyHostToDevice, c->stream));
    launch_gather_attrs((const swr_vertex_attr*)c->attrs.p, vertex_count, (const int64_t*)c->indices.p, c->ni / 3,
                        (const float4*)c->tri_xyz.p, (float4*)c->tri_nrm.p, (float4*)c->tri_rgb.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    if ((rc = prefill_sparse(c, false, true))) return rc;       // (sparse normal deltas given earlier take effect on these attributes)
    // (the gather wrote the uploaded normals: morph and pose them, or, under a computed mode given earlier, replace them)
    if ((c->pose_active || c->morph_active || c->normals_mode != SWR_NORMALS_UPLOADED) && (rc = enqueue_pose(c, true))) return rc;
    if ((rc = wait_stream(c, c->stream, "attribute upload"))) return or_sticky(c, rc);
    c->has_attrs = true;
    return SWR_OK;
}

// swr_scene_skin: the influences of the resident scene's vertices (skin == NULL: none).  The stream goes back to the bind pose.
int single_scene_skin(swr_context* c, const swr_skin_vertex* skin, int64_t vertex_count) {
    if (const int f = sticky(c)) return f;
    if (!c->has_scene) return fail(c, SWR_ERR_NO_SCENE, "swr_scene_skin needs swr_scene_upload first");
    if (skin ? vertex_count != c->nv : vertex_count != 0)
        return fail(c, SWR_ERR_BAD_ARG, "swr_scene_skin: %lld influences%s for %lld vertices", (long long)vertex_count,
                    skin ? "" : " without a skin", (long long)c->nv);
    int64_t maxj = -1;
    for (int64_t i = 0; skin && i < vertex_count; i++)
        for (int k = 0; k < 4; k++) maxj = std::max<int64_t>(maxj, skin[i].joint[k]);
    if (maxj >= SWR_SKIN_MAX_JOINTS)
        return fail(c, SWR_ERR_BAD_ARG, "swr_scene_skin: joint index %lld (at most %d)", (long long)maxj, SWR_SKIN_MAX_JOINTS - 1);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = check_frames(c))) return rc;      // (every stream idle; an overflowed last frame redrawn in the pose it was drawn in)
    if (skin) {
        if ((rc = ensure(c, c->skin, (size_t)vertex_count * sizeof(swr_skin_vertex)))) return rc;
        if (vertex_count)
            HIP_TRY(c, hipMemcpyAsync(c->skin.p, skin, (size_t)vertex_count * sizeof(swr_skin_vertex), hipMemcpyHostToDevice, c->stream));
    }
    if (c->pose_active) {
        c->pose_active = false;
        c->pose_dq = false;
        c->pose.clear();
        if ((rc = enqueue_pose(c, c->has_attrs))) return rc;
    }
    if ((rc = wait_stream(c, c->stream, "skin upload"))) return or_sticky(c, rc);
    c->has_skin = skin != nullptr;
    c->skin_max_joint = maxj;
    return SWR_OK;
}

// swr_pose_set, swr_pose_set_dq (dq): the resident scene in the pose `joints` (NULL with joint_count 0: the bind pose), in effect when
// the call returns.  One pose state: the pose in effect is that of the last call of either kind, joint_count x 16 floats of matrices
// or, dq, joint_count x 8 floats of dual quaternions.
// (check_pose / take_pose: the checks and the host state of the call, shared with swr_morph_pose_set, whose name `fn` is then)
int check_pose(swr_context* c, const char* fn, const float* joints, int32_t joint_count, bool dq) {
    if (!c->has_scene) return fail(c, SWR_ERR_NO_SCENE, "%s needs swr_scene_upload first", fn);
    if (!c->has_skin) return fail(c, SWR_ERR_BAD_ARG, "%s needs swr_scene_skin first", fn);
    if (joint_count < 0) return fail(c, SWR_ERR_BAD_ARG, "%s: joint_count %d", fn, joint_count);
    if (joint_count > SWR_SKIN_MAX_JOINTS)
        return fail(c, SWR_ERR_UNSUPPORTED, "%s: %d joints (at most %d)", fn, joint_count, SWR_SKIN_MAX_JOINTS);
    if (!joints && joint_count > 0)
        return fail(c, SWR_ERR_BAD_ARG, "%s: %d joints without %s", fn, joint_count, dq ? "dual quaternions" : "matrices");
    if (joints && (int64_t)joint_count <= c->skin_max_joint)
        return fail(c, SWR_ERR_BAD_ARG, "%s: %d joints, but the skin uses joint index %lld", fn, joint_count,
                    (long long)c->skin_max_joint);
    return SWR_OK;
}
// the pose becomes the context's; whether the stream has to be rewritten for it
bool take_pose(swr_context* c, const float* joints, int32_t joint_count, bool dq) {
    const bool bind = !joints;
    if (bind && !c->pose_active) return false;
    c->pose_active = !bind;
    c->pose_dq = !bind && dq;
    if (bind) c->pose.clear(); else c->pose.assign(joints, joints + (size_t)joint_count * (dq ? 8 : 16));
    return true;
}
int single_pose_set(swr_context* c, const float* joints, int32_t joint_count, bool dq) {
    if (const int f = sticky(c)) return f;
    int rc;
    if ((rc = check_pose(c, dq ? "swr_pose_set_dq" : "swr_pose_set", joints, joint_count, dq))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = check_frames(c))) return rc;      // (every stream idle; an overflowed last frame redrawn in the pose it was drawn in)
    if (!take_pose(c, joints, joint_count, dq)) return SWR_OK;
    if ((rc = enqueue_pose(c, c->has_attrs))) return rc;
    if ((rc = wait_stream(c, c->stream, "pose"))) return or_sticky(c, rc);
    return SWR_OK;
}

// One plane of deltas — target_count x nv x 3 floats of the caller's — into `dst` in the device layout, on c->stream (idle).  Packed
// layout from page-locked memory: one copy straight from the caller's array.  Else through the pinned staging chunks of image 0, two
// in flight, the host writing (and, SWR_TUNE_MORPH_PAD, padding) chunk k+1 while chunk k is on the link: no second full host copy.
// `chunks` counts the chunks staged since the stream was last idle (the two planes of one call share the staging).
int upload_deltas(swr_context* c, void* dst, const float* src, size_t count /* target_count * nv */, size_t& chunks) {
    if (!count) return SWR_OK;
    if (!SWR_TUNE_MORPH_PAD && is_pinned(src)) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, count * 12, hipMemcpyHostToDevice, c->stream));
        return SWR_OK;
    }
    int rc = ensure_stage(c, 0);
    if (rc) return rc;
    constexpr size_t F = SWR_TUNE_MORPH_PAD ? 4 : 3;
    const size_t per = swr_context::STAGE_BYTES / (F * 4);        // vectors per chunk
    for (size_t at = 0; at < count; at += per) {
        const size_t n = std::min(per, count - at), k = chunks++;
        if (k >= 2 && (rc = poll_event(c, c->stage_ev[0][k & 1], "a staged copy of morph deltas", c->frame_no))) return rc;
        float* st = (float*)c->stage[0][k & 1].p;
        if (SWR_TUNE_MORPH_PAD)
            for (size_t i = 0; i < n; i++) {
                st[4 * i] = src[3 * (at + i)]; st[4 * i + 1] = src[3 * (at + i) + 1]; st[4 * i + 2] = src[3 * (at + i) + 2]; st[4 * i + 3] = 0.0f;
            }
        else memcpy(st, src + 3 * at, n * 12);
        HIP_TRY(c, hipMemcpyAsync((uint8_t*)dst + at * F * 4, st, n * F * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->stage_ev[0][k & 1], c->stream));
    }
    return SWR_OK;
}

// A table of the sparse targets (entries, touched vertices, rows: built on the host, so never page-locked) into `dst` on c->stream,
// through the same staging chunks under the same rule: `chunks` counts the chunks staged since the stream was last idle, the tables
// of one call share it, and a chunk is written again only once the copy that last read it has ended.
int upload_staged(swr_context* c, void* dst, const void* src, size_t bytes, size_t& chunks) {
    if (!bytes) return SWR_OK;
    int rc = ensure_stage(c, 0);
    if (rc) return rc;
    const size_t per = swr_context::STAGE_BYTES;
    for (size_t at = 0; at < bytes; at += per) {
        const size_t n = std::min(per, bytes - at), k = chunks++;
        if (k >= 2 && (rc = poll_event(c, c->stage_ev[0][k & 1], "a staged copy of sparse morph targets", c->frame_no))) return rc;
        memcpy(c->stage[0][k & 1].p, (const uint8_t*)src + at, n);
        HIP_TRY(c, hipMemcpyAsync((uint8_t*)dst + at, c->stage[0][k & 1].p, n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->stage_ev[0][k & 1], c->stream));
    }
    return SWR_OK;
}

// swr_scene_morph: the morph targets of the resident scene (targets == NULL: none).  Every weight is 0 afterwards; skin and pose stay.
int single_scene_morph(swr_context* c, const swr_morph_targets* t) {
    if (const int f = sticky(c)) return f;
    if (!c->has_scene) return fail(c, SWR_ERR_NO_SCENE, "swr_scene_morph needs swr_scene_upload first");
    if (t) {
        if (t->vertex_count != c->nv)
            return fail(c, SWR_ERR_BAD_ARG, "swr_scene_morph: targets of %lld vertices for %lld vertices", (long long)t->vertex_count, (long long)c->nv);
        if (!t->position_deltas) return fail(c, SWR_ERR_BAD_ARG, "swr_scene_morph: position_deltas is NULL");
        if (t->target_count < 1) return fail(c, SWR_ERR_BAD_ARG, "swr_scene_morph: target_count %d", t->target_count);
        if (t->reserved != 0) return fail(c, SWR_ERR_BAD_ARG, "swr_scene_morph: reserved must be 0");
        if (t->target_count > SWR_MORPH_MAX_TARGETS)
            return fail(c, SWR_ERR_UNSUPPORTED, "swr_scene_morph: %d targets (at most %d)", t->target_count, SWR_MORPH_MAX_TARGETS);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = check_frames(c))) return rc;      // (every stream idle; an overflowed last frame redrawn in the shape it was drawn in)
    DevBuf dpos, dnrm;                          // the new planes: the old ones stay until these are filled (a failure frees them)
    if (t) {
        const size_t count = (size_t)t->target_count * (size_t)c->nv;
        const size_t bytes = std::max<size_t>(16, count * (SWR_TUNE_MORPH_PAD ? 16 : 12));
        for (DevBuf* b : {&dpos, &dnrm}) {
            if (b == &dnrm && !t->normal_deltas) break;
            const hipError_t e = hipMalloc(&b->p, bytes);
            if (e != hipSuccess) {
                b->p = nullptr;
                return fail(c, SWR_ERR_NOMEM, "swr_scene_morph: hipMalloc(%zu) for the deltas failed: %s", bytes, hipGetErrorString(e));
            }
            b->bytes = bytes;
        }
        size_t chunks = 0;
        if ((rc = upload_deltas(c, dpos.p, t->position_deltas, count, chunks))) return rc;
        if (t->normal_deltas && (rc = upload_deltas(c, dnrm.p, t->normal_deltas, count, chunks))) return rc;
        if ((rc = wait_stream(c, c->stream, "morph target upload"))) return or_sticky(c, rc);
    }
    const bool was_active = c->morph_active;
    drop_morph(c);
    if (t) {
        c->morph_dpos = std::move(dpos); c->morph_dnrm = std::move(dnrm);
        c->morph_targets = t->target_count;
        c->morph_has_nrm = t->normal_deltas != nullptr;
        c->morph_w.assign((size_t)t->target_count, 0.0f);
    }
    if (was_active) {                           // every weight is 0 now: the unmorphed scene, in the pose it has
        if ((rc = enqueue_pose(c, c->has_attrs))) return rc;
        if ((rc = wait_stream(c, c->stream, "morph targets"))) return or_sticky(c, rc);
    }
    return SWR_OK;
}

// hipMemcpyDeviceToDevice (the fake runtime the host test programs compile this file against names only the two host directions)
constexpr hipMemcpyKind COPY_ON_DEVICE = (hipMemcpyKind)3;
#ifdef __HIPCC__
static_assert(COPY_ON_DEVICE == hipMemcpyDeviceToDevice, "the copy kind of prefill_sparse");
#endif

// Sparse targets: the morphed arrays start as copies of the base arrays, made on the device, so that k_morph_sparse
// has the touched vertices to write and nothing else.  positions: when the targets are installed; attrs: then too, and again when
// swr_scene_attributes replaces the base attributes (only where normal deltas were given).  On c->stream.
int prefill_sparse(swr_context* c, bool positions, bool attrs) {
    if (!c->morph_sparse || c->nv == 0) return SWR_OK;
    int rc;
    if (positions) {
        if ((rc = ensure(c, c->morphed, (size_t)c->nv * sizeof(swr_vertex)))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->morphed.p, c->vertices.p, (size_t)c->nv * sizeof(swr_vertex), COPY_ON_DEVICE, c->stream));
    }
    if (attrs && c->morph_has_nrm) {
        if ((rc = ensure(c, c->morphed_attrs, (size_t)c->nv * sizeof(swr_vertex_attr)))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->morphed_attrs.p, c->attrs.p, (size_t)c->nv * sizeof(swr_vertex_attr), COPY_ON_DEVICE, c->stream));
    }
    return SWR_OK;
}

// a device buffer of its own for new targets: the resident ones stay until the new are filled (a failure frees what it got)
int alloc_targets(swr_context* c, DevBuf& b, size_t bytes) {
    bytes = std::max<size_t>(16, bytes);
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(c, SWR_ERR_NOMEM, "swr_scene_morph_sparse: hipMalloc(%zu) for the targets failed: %s", bytes, hipGetErrorString(e));
    }
    b.bytes = bytes;
    return SWR_OK;
}

// swr_scene_morph_sparse: sparse morph targets of the resident scene (targets == NULL: none, of either kind).  Every weight is 0
// afterwards; skin and pose stay.  The rows are built here, on the host, by a counting sort over the vertices: O(vertices + entries).
int single_scene_morph_sparse(swr_context* c, const swr_morph_sparse* t) {
    if (!t) return single_scene_morph(c, nullptr);
    const char* fn = "swr_scene_morph_sparse";
    if (const int f = sticky(c)) return f;
    if (!c->has_scene) return fail(c, SWR_ERR_NO_SCENE, "%s needs swr_scene_upload first", fn);
    if (t->vertex_count != c->nv)
        return fail(c, SWR_ERR_BAD_ARG, "%s: targets of %lld vertices for %lld vertices", fn, (long long)t->vertex_count, (long long)c->nv);
    if (t->target_count < 1) return fail(c, SWR_ERR_BAD_ARG, "%s: target_count %d", fn, t->target_count);
    if (t->reserved != 0) return fail(c, SWR_ERR_BAD_ARG, "%s: reserved must be 0", fn);
    if (t->target_count > SWR_MORPH_MAX_TARGETS)
        return fail(c, SWR_ERR_UNSUPPORTED, "%s: %d targets (at most %d)", fn, t->target_count, SWR_MORPH_MAX_TARGETS);
    if (!t->targets) return fail(c, SWR_ERR_BAD_ARG, "%s: targets is NULL", fn);
    const int32_t T = t->target_count;
    const int64_t nv = c->nv;
    int64_t entries = 0;
    int with_nrm = -1;                          // of the non-empty targets: -1 none seen yet, else whether they give normal deltas
    for (int32_t k = 0; k < T; k++) {
        const swr_morph_sparse_target& g = t->targets[k];
        if (g.count < 0 || g.count > nv) return fail(c, SWR_ERR_BAD_ARG, "%s: target %d lists %lld of %lld vertices", fn, k, (long long)g.count, (long long)nv);
        if (g.count == 0) continue;
        if (!g.indices || !g.position_deltas) return fail(c, SWR_ERR_BAD_ARG, "%s: target %d: %s is NULL", fn, k, g.indices ? "position_deltas" : "indices");
        for (int64_t j = 0; j < g.count; j++) {
            if (g.indices[j] >= (uint64_t)nv)
                return fail(c, SWR_ERR_BAD_ARG, "%s: target %d, position %lld: index %u of %lld vertices", fn, k, (long long)j, g.indices[j], (long long)nv);
            if (j && g.indices[j] <= g.indices[j - 1])
                return fail(c, SWR_ERR_BAD_ARG, "%s: target %d, position %lld: index %u after %u is not ascending", fn, k, (long long)j,
                            g.indices[j], g.indices[j - 1]);
        }
        const int has = g.normal_deltas ? 1 : 0;
        if (with_nrm >= 0 && with_nrm != has) return fail(c, SWR_ERR_BAD_ARG, "%s: target %d: normal deltas on some targets only", fn, k);
        with_nrm = has;
        entries += g.count;
    }
    const bool nrm = with_nrm == 1;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = check_frames(c))) return rc;      // (every stream idle; an overflowed last frame redrawn in the shape it was drawn in)
    // the rows: how many targets list each vertex -> the touched vertices, ascending, and their offsets -> the entries, target by
    // target in ascending order, each appended to its vertex's row: every row comes out sorted by target
    std::vector<uint32_t> slot((size_t)nv, 0);  // per vertex: its count, then its row
    for (int32_t k = 0; k < T; k++)
        for (int64_t j = 0; j < t->targets[k].count; j++) slot[t->targets[k].indices[j]]++;
    std::vector<uint32_t> touched;
    std::vector<int64_t> row(1, 0);
    for (int64_t i = 0; i < nv; i++)
        if (slot[(size_t)i]) {
            row.push_back(row.back() + slot[(size_t)i]);
            slot[(size_t)i] = (uint32_t)touched.size();
            touched.push_back((uint32_t)i);
        }
    std::vector<int64_t> cursor(row.begin(), row.end() - 1);
    std::vector<MorphSparseEntry> ep((size_t)entries), en(nrm ? (size_t)entries : 0);
    for (int32_t k = 0; k < T; k++) {
        const swr_morph_sparse_target& g = t->targets[k];
        for (int64_t j = 0; j < g.count; j++) {
            const size_t at = (size_t)cursor[slot[g.indices[j]]]++;
            ep[at] = MorphSparseEntry{(uint32_t)k, g.position_deltas[3 * j], g.position_deltas[3 * j + 1], g.position_deltas[3 * j + 2]};
            if (nrm) en[at] = MorphSparseEntry{(uint32_t)k, g.normal_deltas[3 * j], g.normal_deltas[3 * j + 1], g.normal_deltas[3 * j + 2]};
        }
    }
    DevBuf dpos, dnrm, dtouched, drow, dw, dmorphed, dattrs;
    if ((rc = alloc_targets(c, dpos, ep.size() * sizeof(MorphSparseEntry)))) return rc;
    if (nrm && (rc = alloc_targets(c, dnrm, en.size() * sizeof(MorphSparseEntry)))) return rc;
    if ((rc = alloc_targets(c, dtouched, touched.size() * 4))) return rc;
    if ((rc = alloc_targets(c, drow, row.size() * 8))) return rc;
    if (!c->morph_w_dev.p && (rc = alloc_targets(c, dw, SWR_MORPH_MAX_TARGETS * 4))) return rc;
    // (the morphed arrays are kept across targets; where they have to grow, the new ones are allocated before anything changes too)
    if (c->morphed.bytes < (size_t)nv * sizeof(swr_vertex) && (rc = alloc_targets(c, dmorphed, (size_t)nv * sizeof(swr_vertex)))) return rc;
    if (nrm && c->morphed_attrs.bytes < (size_t)nv * sizeof(swr_vertex_attr) &&
        (rc = alloc_targets(c, dattrs, (size_t)nv * sizeof(swr_vertex_attr)))) return rc;
    size_t chunks = 0;
    if ((rc = upload_staged(c, dpos.p, ep.data(), ep.size() * sizeof(MorphSparseEntry), chunks))) return rc;
    if ((rc = upload_staged(c, dnrm.p, en.data(), en.size() * sizeof(MorphSparseEntry), chunks))) return rc;
    if ((rc = upload_staged(c, dtouched.p, touched.data(), touched.size() * 4, chunks))) return rc;
    if ((rc = upload_staged(c, drow.p, row.data(), row.size() * 8, chunks))) return rc;
    if ((rc = wait_stream(c, c->stream, "sparse morph target upload"))) return or_sticky(c, rc);
    const bool was_active = c->morph_active;
    drop_morph(c);
    c->morph_dpos = std::move(dpos); c->morph_dnrm = std::move(dnrm);
    c->morph_touched = std::move(dtouched); c->morph_row = std::move(drow);
    if (dw.p) c->morph_w_dev = std::move(dw);
    if (dmorphed.p) c->morphed = std::move(dmorphed);
    if (dattrs.p) c->morphed_attrs = std::move(dattrs);
    c->morph_sparse = true;
    c->morph_touched_count = (int64_t)touched.size();
    c->morph_targets = T;
    c->morph_has_nrm = nrm;
    c->morph_w.assign((size_t)T, 0.0f);
    if ((rc = prefill_sparse(c, true, c->has_attrs))) return rc;
    // (was_active: every weight is 0 now: the unmorphed scene, in the pose it has)
    if (was_active && (rc = enqueue_pose(c, c->has_attrs))) return rc;
    if ((rc = wait_stream(c, c->stream, "sparse morph targets"))) return or_sticky(c, rc);
    return SWR_OK;
}

// swr_morph_set: the resident scene under `weights` (NULL with weight_count 0: every weight 0), in effect when the call returns.
// (check_weights / take_weights: the checks and the host state of the call, shared with swr_morph_pose_set, whose name `fn` is then)
int check_weights(swr_context* c, const char* fn, const float* weights, int32_t weight_count) {
    if (!c->has_scene) return fail(c, SWR_ERR_NO_SCENE, "%s needs swr_scene_upload first", fn);
    if (!c->morph_targets) return fail(c, SWR_ERR_BAD_ARG, "%s needs swr_scene_morph first", fn);
    if (weights ? weight_count != c->morph_targets : weight_count != 0)
        return fail(c, SWR_ERR_BAD_ARG, "%s: %d weights%s for %d targets", fn, weight_count, weights ? "" : " without an array",
                    c->morph_targets);
    return SWR_OK;
}
// the weights become the context's; whether the stream has to be rewritten for them
bool take_weights(swr_context* c, const float* weights, int32_t weight_count) {
    bool any = false;
    for (int32_t k = 0; weights && k < weight_count; k++) any = any || weights[k] != 0.0f;
    if (weights) c->morph_w.assign(weights, weights + weight_count); else c->morph_w.assign((size_t)c->morph_targets, 0.0f);
    if (!any && !c->morph_active) return false;
    c->morph_active = any;
    return true;
}
int single_morph_set(swr_context* c, const float* weights, int32_t weight_count) {
    if (const int f = sticky(c)) return f;
    int rc;
    if ((rc = check_weights(c, "swr_morph_set", weights, weight_count))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = check_frames(c))) return rc;      // (every stream idle; an overflowed last frame redrawn in the shape it was drawn in)
    if (!take_weights(c, weights, weight_count)) return SWR_OK;
    if ((rc = enqueue_pose(c, c->has_attrs))) return rc;
    if ((rc = wait_stream(c, c->stream, "morph"))) return or_sticky(c, rc);
    return SWR_OK;
}

// swr_morph_pose_set: swr_morph_set, then swr_pose_set (pose_kind SWR_POSE_MATRICES) or swr_pose_set_dq (SWR_POSE_DUAL_QUATS), with
// every check of both made before either half changes anything, and one rewrite of the scene: one check_frames, one enqueue_pose,
// one wait.
int single_morph_pose_set(swr_context* c, const float* weights, int32_t weight_count, const float* joints, int32_t joint_count,
                          int32_t pose_kind) {
    const char* fn = "swr_morph_pose_set";
    if (const int f = sticky(c)) return f;
    if (pose_kind != SWR_POSE_MATRICES && pose_kind != SWR_POSE_DUAL_QUATS) return fail(c, SWR_ERR_BAD_ARG, "%s: unknown pose_kind %d", fn, pose_kind);
    const bool dq = pose_kind == SWR_POSE_DUAL_QUATS;
    int rc;
    if ((rc = check_weights(c, fn, weights, weight_count))) return rc;
    if ((rc = check_pose(c, fn, joints, joint_count, dq))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = check_frames(c))) return rc;      // (every stream idle; an overflowed last frame redrawn in the shape and pose it was drawn in)
    const bool morphed = take_weights(c, weights, weight_count), posed = take_pose(c, joints, joint_count, dq);
    if (!morphed && !posed) return SWR_OK;
    if ((rc = enqueue_pose(c, c->has_attrs))) return rc;
    if ((rc = wait_stream(c, c->stream, "morph and pose"))) return or_sticky(c, rc);
    return SWR_OK;
}

// swr_scene_normals: where the resident scene's normals come from (n == NULL: as uploaded), in effect when the call returns — once
// the scene has attributes.  SWR_NORMALS_SMOOTH needs the adjacency: built here, once per scene, on the host, by a counting sort of
// the corners by vertex that keeps corner order — O(vertices + corners) — from the index array as the device holds it.  Everything
// that can fail is done before the mode changes: the new buffers are the context's only then.
int single_scene_normals(swr_context* c, const swr_normals* n) {
    const char* fn = "swr_scene_normals";
    if (const int f = sticky(c)) return f;
    if (!c->has_scene) return fail(c, SWR_ERR_NO_SCENE, "%s needs swr_scene_upload first", fn);
    const int32_t mode = n ? n->mode : SWR_NORMALS_UPLOADED;
    const uint32_t flags = n ? n->flags : 0;
    if (mode != SWR_NORMALS_UPLOADED && mode != SWR_NORMALS_SMOOTH && mode != SWR_NORMALS_FLAT)
        return fail(c, SWR_ERR_BAD_ARG, "%s: unknown mode %d", fn, mode);
    if (flags & ~(uint32_t)SWR_NORMALS_FLIP) return fail(c, SWR_ERR_BAD_ARG, "%s: unknown flags 0x%x", fn, flags);
    if (n && (n->reserved[0] != 0 || n->reserved[1] != 0)) return fail(c, SWR_ERR_BAD_ARG, "%s: reserved must be 0", fn);
    if (mode == SWR_NORMALS_SMOOTH && c->ni >= ((int64_t)1 << 32))
        return fail(c, SWR_ERR_UNSUPPORTED, "%s: smooth normals of %lld indices (fewer than 2^32)", fn, (long long)c->ni);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = check_frames(c))) return rc;      // (every stream idle; an overflowed last frame redrawn with the normals it was drawn with)
    if (mode == c->normals_mode && flags == c->normals_flags) return SWR_OK;
    auto alloc = [&](DevBuf& b, size_t bytes) {         // a buffer of its own: the context's stay until nothing can fail any more
        bytes = std::max<size_t>(16, bytes);
        const hipError_t e = hipMalloc(&b.p, bytes);
        if (e != hipSuccess) {
            b.p = nullptr;
            return fail(c, SWR_ERR_NOMEM, "%s: hipMalloc(%zu) failed: %s", fn, bytes, hipGetErrorString(e));
        }
        b.bytes = bytes;
        return (int)SWR_OK;
    };
    DevBuf doff, dtri, dface, dnrm;
    if (mode == SWR_NORMALS_SMOOTH) {
        const size_t nv = (size_t)c->nv, corners = (size_t)(c->ni / 3) * 3;     // (trailing indices belong to no triangle)
        if (c->face.bytes < (corners / 3) * 16 && (rc = alloc(dface, (corners / 3) * 16))) return rc;
        if (c->auto_nrm.bytes < nv * 16 && (rc = alloc(dnrm, nv * 16))) return rc;
        if (!c->adj_built) {
            std::vector<int64_t> idx(corners);
            if (corners) HIP_TRY(c, hipMemcpyAsync(idx.data(), c->indices.p, corners * 8, hipMemcpyDeviceToHost, c->stream));
            if ((rc = wait_stream(c, c->stream, "index download"))) return or_sticky(c, rc);
            std::vector<uint32_t> off(nv + 1, 0), tri(corners);
            for (size_t e = 0; e < corners; e++) {
                if (idx[e] < 0 || (uint64_t)idx[e] >= (uint64_t)nv)     // (never: the upload validated the indices)
                    return fail(c, SWR_ERR_INDEX_RANGE, "%s: index %lld of %zu vertices", fn, (long long)idx[e], nv);
                off[(size_t)idx[e] + 1]++;
            }
            for (size_t i = 0; i < nv; i++) off[i + 1] += off[i];
            std::vector<uint32_t> cursor(off.begin(), off.end() - 1);
            for (size_t e = 0; e < corners; e++) tri[cursor[(size_t)idx[e]]++] = (uint32_t)(e / 3);
            if ((rc = alloc(doff, off.size() * 4))) return rc;
            if ((rc = alloc(dtri, tri.size() * 4))) return rc;
            size_t chunks = 0;
            if ((rc = upload_staged(c, doff.p, off.data(), off.size() * 4, chunks))) return rc;
            if ((rc = upload_staged(c, dtri.p, tri.data(), tri.size() * 4, chunks))) return rc;
            if ((rc = wait_stream(c, c->stream, "adjacency upload"))) return or_sticky(c, rc);
        }
    }
    if (doff.p) { c->adj_off = std::move(doff); c->adj_tri = std::move(dtri); c->adj_built = true; }
    if (dface.p) c->face = std::move(dface);
    if (dnrm.p) c->auto_nrm = std::move(dnrm);
    c->normals_mode = mode;
    c->normals_flags = flags;
    if (!c->has_attrs) return SWR_OK;           // (kept: it takes effect when swr_scene_attributes arrives)
    if ((rc = enqueue_pose(c, true))) return rc;
    if ((rc = wait_stream(c, c->stream, "normals"))) return or_sticky(c, rc);
    return SWR_OK;
}

int single_material_set(swr_context* c, const swr_material* m) {
    if (!m) { c->material = swr_material{}; return SWR_OK; }
    if (m->shader != SWR_SHADER_PASSTHROUGH && m->shader != SWR_SHADER_PHONG && m->shader != SWR_SHADER_TEXTURED_PHONG)
        return fail(c, SWR_ERR_UNSUPPORTED, "unknown shader %d", m->shader);
    if (m->shininess_log2 < 0 || m->shininess_log2 > 16)
        return fail(c, SWR_ERR_BAD_ARG, "shininess_log2 %d outside [0,16]", m->shininess_log2);
    c->material = *m;      // read at the next swr_draw (by value into the kernel arguments)
    return SWR_OK;
}

int single_blend_set(swr_context* c, const swr_blend* b) {
    if (!b) { c->blend = swr_blend{SWR_BLEND_OVER, 255, {0, 0}}; return SWR_OK; }
    if (b->mode != SWR_BLEND_OVER && b->mode != SWR_BLEND_ADD) return fail(c, SWR_ERR_BAD_ARG, "swr_blend_set: unknown mode %d", b->mode);
    if (b->opacity < 0 || b->opacity > 255) return fail(c, SWR_ERR_BAD_ARG, "swr_blend_set: opacity %d outside [0,255]", b->opacity);
    if (b->reserved[0] != 0 || b->reserved[1] != 0) return fail(c, SWR_ERR_BAD_ARG, "swr_blend_set: reserved words must be 0");
    c->blend = *b;          // copied into the next frames as they are posted (end_draw)
    return SWR_OK;
}

int single_texture_upload(swr_context* c, const void* bgra8, int32_t width, int32_t height) {
    if (const int f = sticky(c)) return f;
    if (!bgra8 || width <= 0 || height <= 0 || width > 16384 || height > 16384)
        return fail(c, SWR_ERR_BAD_ARG, "swr_texture_upload: bad texture %dx%d", width, height);
    HIP_TRY(c, hipSetDevice(c->device));
    { int rcs = sync_streams(c); if (rcs) return rcs; }
    int rc;
    const size_t n = (size_t)width * (size_t)height;
    if ((rc = ensure(c, c->texture_bytes, n * 4))) return rc;
    if ((rc = ensure(c, c->texture, n * 16))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->texture_bytes.p, bgra8, n * 4, hipMemcpyHostToDevice, c->stream));
    launch_texture_to_float((const uint32_t*)c->texture_bytes.p, (int64_t)n, (float4*)c->texture.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    if ((rc = wait_stream(c, c->stream, "texture upload"))) return or_sticky(c, rc);
    c->tex_w = width; c->tex_h = height;
    return SWR_OK;
}

int check_target_args(swr_context* c, int64_t width, int64_t height, int64_t row_begin, int64_t row_end) {
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535)
        return fail(c, SWR_ERR_BAD_ARG, "bad framebuffer size %lldx%lld", (long long)width, (long long)height);
    if (row_begin < 0 || row_end > height || row_begin > row_end || (row_begin % TILE_H) != 0)
        return fail(c, SWR_ERR_BAD_ARG, "bad band [%lld,%lld): row_begin must be a multiple of %d",
                    (long long)row_begin, (long long)row_end, TILE_H);
    return SWR_OK;
}

// swr_target_set on one band: rows [row_begin, row_end) of the target the entry point has checked
int single_target_set(swr_context* c, int64_t width, int64_t height, int64_t row_begin, int64_t row_end) {
    if (const int f = sticky(c)) return f;
    int rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->src_clear = true;        // the band images are the cleared ones again (what the next load frame starts from)
    c->ids_valid = false;       // (and no frame on them has written IDs)
    if (c->has_target && c->tg.width == width && c->tg.height == height && c->tg.row_begin == row_begin && c->tg.row_end == row_end)
        return SWR_OK;          // the same target again (swr_render every frame): nothing to resize, nothing to wait for
    if ((rc = check_frames(c)) || (rc = sync_copies(c))) return rc;      // (an overflowed frame presented just before is repaired / reported first)
    c->draw_pending = false;
    c->present_pending = false;
    Target t;
    t.width = (int32_t)width; t.height = (int32_t)height;
    t.row_begin = (int32_t)row_begin; t.row_end = (int32_t)row_end;
    t.tiles_x = (int32_t)((width + TILE_W - 1) / TILE_W);
    t.tiles_y = (int32_t)((row_end - row_begin + TILE_H - 1) / TILE_H);
    const size_t px = (size_t)width * (size_t)(row_end - row_begin);
    for (int fb = 0; fb < swr_context::NFB; fb++) {
        if ((rc = ensure(c, c->color[fb], px * 4))) return rc;
        if ((rc = ensure(c, c->depth[fb], px * 4))) return rc;
        c->copy_recorded[fb][0] = c->copy_recorded[fb][1] = false;
        c->read_recorded[fb] = false;
    }
    c->fb_cur = c->fb_last = 0;
    c->delta_valid[0] = c->delta_valid[1] = false;          // another target: the host holds nothing of it (delta reads start over)
    for (auto& sl : c->slot)
        if ((rc = ensure(c, sl.tilebuf, (size_t)(CNT_WORDS + 3 * std::max(1, tiles_of(t)) + 1) * 4))) return rc;
    c->tg = t;
    c->has_target = true;
    c->h_pairs[swr_context::PAIR_RING] = 0xFFFFFFFFu;       // fullest bin on the new target: unknown (sort)
    if (tiles_of(t) != c->sized_tiles) {                    // (see single_scene_upload)
        c->fixed_allowed = true;
        c->fixed_mode = false;
        c->k32_ok = true;
    }
    return size_bins(c);
}

int check_draw_args(swr_context* c, uint32_t flags, int32_t primitive_type) {
    if (primitive_type != SWR_PRIMITIVE_TRIANGLE && primitive_type != SWR_PRIMITIVE_LINE &&
        primitive_type != SWR_PRIMITIVE_VERTICES)
        return fail(c, SWR_ERR_UNSUPPORTED, "unknown primitive type %d", primitive_type);
    if (flags & ~(uint32_t)(SWR_FLAG_DEPTH_TEST | SWR_FLAG_NO_COLOR | SWR_FLAG_METAL_RULES | SWR_FLAG_REAL_LINES | SWR_FLAG_LOAD |
                            SWR_FLAG_PRIMITIVE_IDS | SWR_FLAG_CULL_BACK | SWR_FLAG_CULL_FRONT | SWR_FLAG_FRONT_CCW |
                            SWR_FLAG_DEPTH_CLIP | SWR_FLAG_PERSPECTIVE | SWR_FLAG_BLEND))
        return fail(c, SWR_ERR_BAD_ARG, "unknown flag bits 0x%x", flags);
    if ((flags & SWR_FLAG_REAL_LINES) && primitive_type != SWR_PRIMITIVE_LINE)
        return fail(c, SWR_ERR_BAD_ARG, "SWR_FLAG_REAL_LINES only applies to .line primitives");
    if ((flags & SWR_FLAG_PRIMITIVE_IDS) && primitive_type != SWR_PRIMITIVE_TRIANGLE)
        return fail(c, SWR_ERR_UNSUPPORTED, "SWR_FLAG_PRIMITIVE_IDS: triangles only");
    // alpha blending: triangles only (.vertices and .line frames accept the bit and ignore it)
    if ((flags & SWR_FLAG_BLEND) && primitive_type == SWR_PRIMITIVE_TRIANGLE) {
        if (flags & SWR_FLAG_NO_COLOR) return fail(c, SWR_ERR_BAD_ARG, "SWR_FLAG_BLEND blends colour: not with SWR_FLAG_NO_COLOR");
        if (flags & (SWR_FLAG_PRIMITIVE_IDS | SWR_FLAG_PERSPECTIVE))
            return fail(c, SWR_ERR_UNSUPPORTED, "SWR_FLAG_BLEND does not combine with SWR_FLAG_PRIMITIVE_IDS or SWR_FLAG_PERSPECTIVE");
    }
    return SWR_OK;
}

// An ID frame (SWR_FLAG_PRIMITIVE_IDS) needs the ID image of every framebuffer at the target's size: allocated by the first one on a
// target (swr_target_set waits for the frames before a resize, so no frame in flight uses a buffer that grows here)
int ensure_ids(swr_context* c, uint32_t flags) {
    if (!(flags & SWR_FLAG_PRIMITIVE_IDS)) return SWR_OK;
    const size_t bytes = (size_t)c->tg.width * (size_t)(c->tg.row_end - c->tg.row_begin) * 4;
    for (DevBuf& b : c->ids) {
        const int rc = ensure(c, b, bytes);
        if (rc) return rc;
    }
    return SWR_OK;
}

// What swr_draw and swr_draw_list do alike once their arguments are in order.  Before the frame: the material has what it needs, the
// ring of per-frame words has room, the ID images are there.
int begin_draw(swr_context* c, uint32_t flags, int32_t primitive_type) {
    if (primitive_type == SWR_PRIMITIVE_TRIANGLE && (flags & SWR_FLAG_BLEND) && c->material.shader != SWR_SHADER_PASSTHROUGH)
        return fail(c, SWR_ERR_UNSUPPORTED, "SWR_FLAG_BLEND needs the passthrough fragment stage (swr_material_set(ctx, NULL))");
    if (primitive_type == SWR_PRIMITIVE_TRIANGLE && !(flags & SWR_FLAG_NO_COLOR) &&
        c->material.shader != SWR_SHADER_PASSTHROUGH) {
        if (!c->has_attrs)
            return fail(c, SWR_ERR_BAD_ARG, "the material needs vertex attributes (swr_scene_attributes)");
        if (c->material.shader == SWR_SHADER_TEXTURED_PHONG && c->tex_w <= 0)
            return fail(c, SWR_ERR_BAD_ARG, "the material needs a texture (swr_texture_upload)");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->frame_no - c->frames_checked >= (uint64_t)swr_context::PAIR_RING - 2) {
        // the ring of per-frame pair totals is about to wrap over frames nobody has looked at: look now (before
        // the new transform or list replaces the one a redo of the last frame would need)
        const int rc = check_frames(c);
        if (rc) return rc;
    }
    return ensure_ids(c, flags);
}

// ... and the frame itself: where a load frame reads and writes, what a redo of the frame needs, the enqueue.
int end_draw(swr_context* c, uint32_t flags, int32_t primitive_type, bool list, bool persp) {
    if (flags & SWR_FLAG_LOAD) {
        if (c->src_clear) {
            flags &= ~(uint32_t)SWR_FLAG_LOAD;      // loading the cleared image IS the clear frame
        } else {
            // the frame reads the last frame's buffer and writes another one (the pipelined paths reuse a buffer when nothing copies it)
            c->load_src = c->fb_last;
            if (c->fb_cur == c->load_src) c->fb_cur = (c->load_src + 1) % swr_context::NFB;
        }
    }
    c->src_clear = false;
    c->ids_valid = (flags & SWR_FLAG_PRIMITIVE_IDS) != 0;
    swr_context::DrawRecord& d = c->last_draw;
    d.flags = flags; d.blend = c->blend; d.prim = primitive_type;
    d.is_list = list; d.clip = (flags & SWR_FLAG_DEPTH_CLIP) != 0; d.persp = persp;
    return enqueue_frame(c);
}

int single_draw(swr_context* c, const float transform[16], uint32_t flags, int32_t primitive_type) {
    int rc = check_draw_args(c, flags, primitive_type);
    if (rc) return rc;
    {
        const int per = primitive_type == SWR_PRIMITIVE_LINE ? 2 : 3;          // verticesCount, Renderer.swift:179-188
        if (c->has_scene && c->ni % per != 0)                                  // assert, Renderer.swift:209
            return fail(c, SWR_ERR_INDEX_COUNT, "index_count %lld is not a multiple of %d", (long long)c->ni, per);
    }
    if (!c->has_scene || !c->has_target)
        return fail(c, SWR_ERR_NO_SCENE, "swr_draw needs swr_scene_upload and swr_target_set first");
    if ((rc = begin_draw(c, flags, primitive_type))) return rc;
    // depth clipping: triangles only (.vertices and .line frames accept the bit and ignore it)
    if (primitive_type != SWR_PRIMITIVE_TRIANGLE) flags &= ~(uint32_t)(SWR_FLAG_DEPTH_CLIP | SWR_FLAG_BLEND);
    if ((flags & SWR_FLAG_DEPTH_CLIP) && (rc = prepare_clip(c, c->ni / 3, flags, transform))) return rc;
    const bool persp = persp_frame(flags, primitive_type, affine_transform(transform));
    if (persp && (rc = ensure_persp(c, (flags & SWR_FLAG_DEPTH_CLIP) ? clip_slots(c) : c->ni / 3))) return rc;
    memcpy(c->last_draw.m, transform, sizeof c->last_draw.m);
    return end_draw(c, flags, primitive_type, false, persp);
}

// ---- swr_draw_list ----------------------------------------------------------------------------------------------
// The argument checks of a list on a band or a group alike: against c's target and the scene every band holds; *tris = the list's total.
int check_list_args(swr_context* c, const swr_draw_item* items, int32_t n, uint32_t flags, int64_t* tris) {
    const swr_context* scene = band(c, 0);
    const int64_t ni = scene->ni;
    int rc = check_draw_args(c, flags, SWR_PRIMITIVE_TRIANGLE);
    if (rc) return rc;
    if (n < 0) return fail(c, SWR_ERR_BAD_ARG, "swr_draw_list: item_count %d", (int)n);
    if (n > SWR_DRAW_LIST_MAX) return fail(c, SWR_ERR_UNSUPPORTED, "swr_draw_list: %d items (at most %d)", (int)n, SWR_DRAW_LIST_MAX);
    if (n > 0 && !items) return fail(c, SWR_ERR_BAD_ARG, "swr_draw_list: items is NULL");
    for (int32_t k = 0; k < n; k++)
        if (items[k].first_index % 3 != 0 || items[k].index_count % 3 != 0)
            return fail(c, SWR_ERR_INDEX_COUNT, "swr_draw_list: item %d: first_index %lld / index_count %lld not a multiple of 3", (int)k,
                        (long long)items[k].first_index, (long long)items[k].index_count);
    if (!scene->has_scene || !c->has_target) return fail(c, SWR_ERR_NO_SCENE, "swr_draw_list needs swr_scene_upload and swr_target_set first");
    int64_t total = 0;
    for (int32_t k = 0; k < n; k++) {
        const int64_t a = items[k].first_index, cnt = items[k].index_count;
        if (a < 0 || cnt < 0 || a > ni || cnt > ni - a)
            return fail(c, SWR_ERR_BAD_ARG, "swr_draw_list: item %d: indices [%lld, %lld + %lld) outside the %lld uploaded", (int)k,
                        (long long)a, (long long)a, (long long)cnt, (long long)ni);
        total += cnt / 3;
        if (total >= SORT_MAX_TRIS)
            return fail(c, SWR_ERR_UNSUPPORTED, "swr_draw_list: 2^24 triangles or more in one list (the width of the order number)");
    }
    *tris = total;
    return SWR_OK;
}

// Rebuild the stream cut at `cuts` (every stream idle): sorted by (segment, Morton code), so that every segment is a run of slots.
int restream(swr_context* c, const std::vector<uint32_t>& cuts) {
    int rc;
    const int64_t ntri = c->ni / 3;
    if ((rc = ensure(c, c->cuts_dev, std::max<size_t>(1, cuts.size()) * 4))) return rc;
    if (!cuts.empty()) HIP_TRY(c, hipMemcpyAsync(c->cuts_dev.p, cuts.data(), cuts.size() * 4, hipMemcpyHostToDevice, c->stream));
    StreamBuild b{};
    b.vertices = (const swr_vertex*)c->vertices.p; b.nv = c->nv;
    b.indices = (const int64_t*)c->indices.p; b.ntri = ntri;
    b.sort = true;
    b.scratch = (uint32_t*)c->stream_scratch.p;
    b.sort_temp = c->sort_temp.p; b.sort_temp_bytes = c->sort_temp.bytes;
    b.tri_xyz = (float4*)c->tri_xyz.p; b.tri_rgb = (float4*)c->tri_rgb.p;
    b.inv = (uint32_t*)c->inv.p; b.box64 = (float4*)c->box64.p;
    b.cuts = (const uint32_t*)c->cuts_dev.p; b.ncuts = (int)cuts.size();
    HIP_TRY(c, launch_build_stream(b, c->stream));
    if (c->has_attrs)
        launch_gather_attrs((const swr_vertex_attr*)c->attrs.p, c->nv, (const int64_t*)c->indices.p, ntri,
                            (const float4*)c->tri_xyz.p, (float4*)c->tri_nrm.p, (float4*)c->tri_rgb.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    // (the rebuild gathered the uploaded scene: morph and pose it again, and compute its normals again)
    if ((c->pose_active || c->morph_active || (c->has_attrs && c->normals_mode != SWR_NORMALS_UPLOADED)) &&
        (rc = enqueue_pose(c, c->has_attrs))) return rc;
    if ((rc = wait_stream(c, c->stream, "stream rebuild (draw list)"))) return or_sticky(c, rc);
    c->cuts = cuts;
    return SWR_OK;
}

// A Morton-sorted stream scatters an index range over the whole stream: cut it at every boundary of `need` (primitive indices, any
// order) first — once per new set of boundaries: the cuts made for earlier lists stay while they are few.
int cut_stream(swr_context* c, std::vector<uint32_t>& need) {
    if (!c->stream_sorted || need.empty()) return SWR_OK;
    std::sort(need.begin(), need.end());
    need.erase(std::unique(need.begin(), need.end()), need.end());
    if (std::includes(c->cuts.begin(), c->cuts.end(), need.begin(), need.end())) return SWR_OK;
    std::vector<uint32_t> cuts;
    std::set_union(c->cuts.begin(), c->cuts.end(), need.begin(), need.end(), std::back_inserter(cuts));
    if (cuts.size() > (size_t)2 * SWR_DRAW_LIST_MAX) cuts = need;
    int rc;
    if ((rc = check_frames(c))) return rc;           // (every stream idle; an overflowed last frame redrawn on the old stream)
    return restream(c, cuts);
}

// swr_draw_list on one band: a list check_list_args has passed, of `tris` triangles
int single_draw_list(swr_context* c, const swr_draw_item* items, int32_t n, uint32_t flags, int64_t tris) {
    if (const int f = sticky(c)) return f;
    int rc;
    if ((rc = begin_draw(c, flags, SWR_PRIMITIVE_TRIANGLE))) return rc;
    // the items, resolved: primitive ranges, frame bases, work units
    std::vector<ListItem> list((size_t)n);
    std::vector<uint32_t> need;             // the cuts the stream needs
    const int64_t ntri = c->ni / 3;
    int64_t vbase = 0, units = 0;
    bool affine = true, identity = true;
    for (int32_t k = 0; k < n; k++) {
        ListItem& it = list[(size_t)k];
        it.first = (uint32_t)(items[k].first_index / 3);
        it.count = (uint32_t)(items[k].index_count / 3);
        it.vbase = (uint32_t)vbase;
        it.ubase = (uint32_t)units;
        memcpy(it.m, items[k].transform, sizeof it.m);
        if (it.count) {
            units += (int64_t)((it.first + it.count - 1) >> 6) - (int64_t)(it.first >> 6) + 1;
            affine = affine && affine_transform(it.m);
            identity = identity && it.first == it.vbase;
            if (it.first > 0) need.push_back(it.first);
            if ((int64_t)it.first + it.count < ntri) need.push_back(it.first + it.count);
        }
        vbase += it.count;
    }
    if ((rc = cut_stream(c, need))) return rc;
    // per-slot buffers for V frame slots (grown with every stream idle); the frame's own per-slot tables only where the raster reads them
    {
        using Slot = swr_context::Slot;
        const size_t V = (size_t)std::max<int64_t>(tris, 1);
        const bool color = !(flags & SWR_FLAG_NO_COLOR);
        LaneSizes t;
        t.add(&Slot::geo, V * sizeof(GeomRec)); t.add(&Slot::geo_full, V * sizeof(GeomFull)); t.add(&Slot::ranges, V * sizeof(uint2));
        t.add(&Slot::items, std::max<size_t>(1, (size_t)n) * sizeof(ListItem));
        if (!identity) t.add(&Slot::linv, V * 4);
        if (!identity && color) t.add(&Slot::lrgb, V * 48);
        if (!identity && color && c->material.shader != SWR_SHADER_PASSTHROUGH) t.add(&Slot::lnrm, V * 48);
        if ((rc = grow_lanes(c, t))) return rc;
    }
    if ((rc = fit_bins(c, tris, units * 64))) return rc;
    if ((flags & SWR_FLAG_DEPTH_CLIP) && (rc = prepare_clip(c, tris, flags, nullptr))) return rc;
    const bool persp = persp_frame(flags, SWR_PRIMITIVE_TRIANGLE, affine);
    if (persp && (rc = ensure_persp(c, (flags & SWR_FLAG_DEPTH_CLIP) ? clip_slots(c) : tris))) return rc;
    c->last_draw.list.swap(list);
    c->last_draw.list_tris = tris; c->last_draw.list_units = units;
    c->last_draw.list_affine = affine; c->last_draw.list_identity = identity;
    return end_draw(c, flags, SWR_PRIMITIVE_TRIANGLE, true, persp);
}

// swr_present of the frame in fb_last: both images in flight together, each on its own copy stream
int enqueue_present(swr_context* c, void* color_full, float* depth_full) {
    const int fb = c->fb_last;
    if (tiles_of(c->tg) == 0) return SWR_OK;
    const bool want_color = color_full && !(c->last_draw.flags & SWR_FLAG_NO_COLOR);
    const uint64_t frame = c->frame_no ? c->frame_no - 1 : 0;      // the frame being presented (for messages)
    hipStream_t fs = c->last_stream ? c->last_stream : c->stream;        // the stream that carries the frame's raster
    auto copies = [c, fb, want_color, color_full, depth_full, frame, fs]() -> int {
        int rc;
        HIP_TRY(c, hipEventRecord(c->frame_done[fb], fs));
        const size_t row = (size_t)c->tg.width * 4;
        if (want_color && (rc = copy_band(c, fb, 0, fb_image(c, fb, 0), row, c->tg.row_begin, c->tg.row_end, color_full, frame))) return rc;
        if (depth_full && (rc = copy_band(c, fb, 1, fb_image(c, fb, 1), row, c->tg.row_begin, c->tg.row_end, depth_full, frame))) return rc;
        return SWR_OK;
    };
    // frame lanes: the frame is on its stream already, and the next draw went (or goes) to another buffer anyway
    const bool lanes = sched_of(c) == Sched::Lanes;
    if (!lanes && c->ts.ras_worker) c->ts.ras_worker->post(copies);   // behind the frame's raster share, in order
    else {
        int rc = flush_raster(c, c->frame_no);        // the frame being presented must be on the raster stream
        if (rc || (rc = copies())) return rc;
    }
    if (!lanes) c->fb_cur = fb == 0 ? 1 : 0;     // the next frame renders into the other framebuffer while this one is being copied
    if (c->frame_no) c->frame_presented[(c->frame_no - 1) % swr_context::PAIR_RING] = true;
    return SWR_OK;
}

int single_present(swr_context* c, void* color_full, float* depth_full) {
    if (const int f = sticky(c)) return f;
    if (!c->has_target) return fail(c, SWR_ERR_NO_SCENE, "swr_present needs swr_target_set and a swr_draw first");
    if (!color_full && !depth_full) return fail(c, SWR_ERR_BAD_ARG, "swr_present: both image pointers are NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    c->present_color = color_full;
    c->present_depth = depth_full;
    c->present_pending = true;
    return enqueue_present(c, color_full, depth_full);
}

// Look at the pair totals of every frame since the last look.  The LAST frame is repaired here (bins grown, frame
// redrawn and, if it had been presented, copied again); an earlier frame of an un-waited burst that overflowed was
// rastered empty — the bins are grown and SWR_ERR_FRAME_DROPPED is returned once everything else is in order.
int check_frames(swr_context* c) {
    bool dropped = false;
    uint64_t dropped_frame = 0;
    uint32_t dropped_pairs = 0;
    auto finish = [&]() -> int {
        harvest(c);
        if (dropped)
            return fail(c, SWR_ERR_FRAME_DROPPED, "frame %llu of an un-waited burst overflowed the bin capacity (%u entries) and "
                        "was rastered empty; the bins have been grown — redraw it", (unsigned long long)dropped_frame, dropped_pairs);
        return SWR_OK;
    };
    // what a frame needed against what the bins give: exact bins count (triangle,tile) pairs, fixed-stride bins the
    // entries of the fullest tile region
    auto used = [&](uint64_t f) { return c->fixed_mode ? fill_word(c, f) : pair_word(c, f); };
    auto limit = [&]() { return c->fixed_mode ? c->cap_tile : c->capacity; };
    // a depth-clip frame whose fan triangles overflowed its slots was rastered empty too: its word holds the post-clip count
    auto clip_over = [&](uint64_t f) { return (uint64_t)c->h_clip[f % swr_context::PAIR_RING]; };
    for (int attempt = 0; attempt < 8; attempt++) {
        int rc;
        if ((rc = sync_streams(c))) return rc;
        if (!c->draw_pending || c->frame_no == 0) { c->frames_checked = c->frame_no; return finish(); }
        const uint64_t L = c->frame_no - 1;
        const uint32_t pairs = used(L);
        uint32_t need = pairs;
        uint32_t total_pairs = pair_word(c, L);               // (for the switch to exact bins)
        bool bad_prev = c->src_bad;                            // the image of frame f - 1 is wrong
        uint64_t clip_need = clip_over(L);
        for (uint64_t f = c->frames_checked; f < L; f++) {
            const uint32_t pf = used(f);
            if (pf > limit()) { need = std::max(need, pf); total_pairs = std::max(total_pairs, pair_word(c, f)); }
            clip_need = std::max(clip_need, clip_over(f));
            // an earlier frame that overflowed was rastered empty — and a load frame built on such an image is as wrong: that matters
            // only if it was copied to the host
            const bool bad = pf > limit() || clip_over(f) != 0 || (c->frame_load[f % swr_context::PAIR_RING] && bad_prev);
            if (bad && c->frame_presented[f % swr_context::PAIR_RING]) {
                if (!dropped || pf > dropped_pairs) { dropped_frame = f; dropped_pairs = pf; }
                dropped = true;
            }
            bad_prev = bad;
        }
        c->frames_checked = L;
        c->src_bad = bad_prev;
        const uint32_t old_limit = limit();
        if (need > old_limit) {
            if ((rc = sync_copies(c))) return rc;
            if (c->fixed_mode) {
                const uint32_t cmax = fixed_cap_max(std::max<int64_t>(c->ni / 3, c->list_plan_max), tiles_of(c->tg));
                if (need > cmax) {
                    // a tile needs more than a fixed region can hold: exact-size bins (four binning kernels) from here on
                    c->fixed_mode = false;
                    c->fixed_allowed = false;
                    const uint64_t want = (uint64_t)total_pairs + total_pairs / 4 + 1024;
                    if (want > 0xFFFFFFF0ull) return fail(c, SWR_ERR_UNSUPPORTED, "too many (triangle,tile) pairs: %u", total_pairs);
                    if ((rc = ensure_capacity(c, (uint32_t)want))) return rc;
                } else {
                    const uint64_t want = std::min<uint64_t>(cmax, (((uint64_t)need + need / 4 + 64) + 63) & ~63ull);
                    if ((rc = ensure_bins(c, (size_t)tiles_of(c->tg) * (size_t)want))) return rc;
                    c->cap_tile = (uint32_t)want;
                }
            } else {
                const uint64_t want = (uint64_t)need + need / 4 + 1024;
                if (want > 0xFFFFFFF0ull) return fail(c, SWR_ERR_UNSUPPORTED, "too many (triangle,tile) pairs: %u", need);
                if ((rc = ensure_capacity(c, (uint32_t)want))) return rc;
            }
        }
        if (clip_need) {
            // more crossing triangles than the fan capacity: grow it (every stream is idle), the redraw below takes the new slots
            if ((rc = sync_copies(c))) return rc;
            const int64_t extra = (int64_t)clip_need - c->last_draw.clip_n;
            c->clip_fan = std::max<int64_t>(2 * c->clip_fan, (extra + 1) / 2 + extra / 8 + 64);
            if (c->last_draw.clip && (rc = prepare_clip(c, c->last_draw.clip_n, c->last_draw.flags, nullptr))) return rc;
            if (c->last_draw.clip && c->last_draw.persp && (rc = ensure_persp(c, clip_slots(c)))) return rc;
        }
        if (c->frame_load[L % swr_context::PAIR_RING] && c->src_bad) {
            // the last frame loaded a wrong image: a redraw cannot repair it — reported (whether it was copied or not: it is what the
            // next load frame, swr_present or swr_read_* would see), and so is every load frame built on it until an image is replaced
            c->draw_pending = false;
            c->present_pending = false;
            c->frames_checked = c->frame_no;
            harvest(c);
            return fail(c, SWR_ERR_FRAME_DROPPED, "frame %llu is a load frame whose starting image was rastered empty by a bin overflow "
                        "(the bins have been grown) — redraw the chain from a clear frame, swr_target_set or swr_target_write",
                        (unsigned long long)L);
        }
        if (pairs <= old_limit && !clip_over(L)) {
            c->draw_pending = false;
            c->src_bad = false;
            c->present_pending = false;        // the last frame is verified: a later repair must not copy into a stale destination
            c->frames_checked = c->frame_no;
            c->last.tile_pairs = pair_word(c, L);
            c->last.tiles = tiles_of(c->tg);
            c->last.triangles = c->last_draw.is_list ? c->last_draw.list_tris : c->ni / 3;
            return finish();
        }
        // the last frame overflowed: redraw it into the same framebuffer, copy it again
        c->h_clip[L % swr_context::PAIR_RING] = 0u;          // (its fan overflow is repaired by the redraw)
        const bool was_presented = c->present_pending && c->frame_presented[L % swr_context::PAIR_RING];
        c->fb_cur = c->fb_last;
        if ((rc = enqueue_frame(c))) return rc;
        if (was_presented && (rc = enqueue_present(c, c->present_color, c->present_depth))) return rc;
    }
    return fail(c, SWR_ERR_HIP, "pair list kept overflowing");
}

// swr_target_write: rows [row_begin, row_end) of the caller's images become the band's current image (what the next load frame
// starts from).  Everything drawn before is finished and checked first; NULL keeps that image (the cleared one after swr_target_set).
int single_target_write(swr_context* c, const void* color_full, const float* depth_full) {
    if (const int f = sticky(c)) return f;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = check_frames(c)) || (rc = sync_copies(c))) return rc;
    const size_t px = (size_t)c->tg.width * (size_t)(c->tg.row_end - c->tg.row_begin);
    const int fb = c->fb_last;
    if (px) {
        const size_t off = (size_t)c->tg.row_begin * (size_t)c->tg.width;
        // (pageable sources are staged by the runtime; page-locked ones go straight over the link)
        if (c->src_clear && (!color_full || !depth_full)) {
            // an image not given keeps the cleared state: the clear of a .line pass (the reference's empty stub), Renderer.swift:205-206
            DeviceFrame f{};
            f.color = (uint8_t*)c->color[fb].p;
            f.depth = (float*)c->depth[fb].p;
            f.tg = c->tg;
            launch_points_or_lines(f, SWR_PRIMITIVE_LINE, c->stream);
            HIP_TRY(c, hipGetLastError());
        }
        if (color_full) HIP_TRY(c, hipMemcpyAsync(c->color[fb].p, (const uint32_t*)color_full + off, px * 4, hipMemcpyHostToDevice, c->stream));
        if (depth_full) HIP_TRY(c, hipMemcpyAsync(c->depth[fb].p, depth_full + off, px * 4, hipMemcpyHostToDevice, c->stream));
        if ((rc = wait_stream(c, c->stream, "image upload"))) return or_sticky(c, rc);
    }
    c->src_clear = false;
    c->src_bad = false;
    c->ids_valid = false;       // the image is the caller's now: no frame's IDs describe it
    return SWR_OK;
}

int single_sync(swr_context* c) {
    if (const int f = sticky(c)) return f;
    HIP_TRY(c, hipSetDevice(c->device));
    return check_frames(c);
}

int single_present_wait(swr_context* c) {
    if (const int f = sticky(c)) return f;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = check_frames(c);
    if (rc) return rc;
    if ((rc = sync_copies(c))) return rc;
    c->present_pending = false;
    return SWR_OK;
}

// img: 0 colour, 1 depth, 2 the ID image (swr_read_ids)
int single_read(swr_context* c, int img, void* dst) {
    if (const int f = sticky(c)) return f;
    if (!c->has_target) return fail(c, SWR_ERR_NO_SCENE, "swr_read_* needs swr_target_set first");
    if (img == 2 && !c->ids_valid)
        return fail(c, SWR_ERR_BAD_ARG, "swr_read_ids: the last frame was drawn without SWR_FLAG_PRIMITIVE_IDS, or swr_target_set / "
                    "swr_target_write / swr_scene_upload came after it");
    int rc = single_sync(c);
    if (rc) return rc;
    if (tiles_of(c->tg) == 0) return SWR_OK;
    const int fb = c->fb_last;
    HIP_TRY(c, hipEventRecord(c->frame_done[fb], c->stream));
    const int cs = img == 2 ? 1 : img;      // the ID image goes on the depth image's copy stream
    if ((rc = copy_band(c, fb, cs, fb_image(c, fb, img), (size_t)c->tg.width * 4, c->tg.row_begin, c->tg.row_end, dst,
                        c->frame_no ? c->frame_no - 1 : 0))) return rc;
    if ((rc = wait_stream(c, c->copy_stream[cs], "copy stream"))) return or_sticky(c, rc);
    return SWR_OK;
}

// Every query below comes in two parts.  check_X: what the call may be handed, against c->tg — a band's own target or the full one a
// group keeps, so it holds for either kind of context and runs once, before any band is touched.  band_X: one band's work — sticky,
// the state only a band has (ids_valid, the last draw), the launches, the wait — which leaves the band's answer in its own staging for
// the entry point to gather over the bands of c.

// what a swr_resolve may hold (swr_render_resolved checks it before it has a target)
int check_resolve_args(swr_context* c, const swr_resolve& rs) {
    if (rs.factor != 1 && rs.factor != 2 && rs.factor != 4)
        return fail(c, SWR_ERR_BAD_ARG, "swr_resolve: factor %d is not 1, 2 or 4", rs.factor);
    if (rs.depth_filter != SWR_RESOLVE_DEPTH_SAMPLE0 && rs.depth_filter != SWR_RESOLVE_DEPTH_MIN)
        return fail(c, SWR_ERR_BAD_ARG, "swr_resolve: unknown depth filter %d", rs.depth_filter);
    if (rs.reserved[0] || rs.reserved[1]) return fail(c, SWR_ERR_BAD_ARG, "swr_resolve: reserved words must be 0");
    return SWR_OK;
}

int check_resolve(swr_context* c, const swr_resolve& rs) {
    const int rc = check_resolve_args(c, rs);
    if (rc) return rc;
    if (!c->has_target) return fail(c, SWR_ERR_NO_SCENE, "swr_read_*_resolved needs swr_target_set first");
    const Target& t = c->tg;
    if (t.width % rs.factor || t.height % rs.factor)
        return fail(c, SWR_ERR_BAD_ARG, "supersampled resolve: the target %dx%d is not a multiple of the factor %d", t.width, t.height, rs.factor);
    // (row_begin is a multiple of the tile height; a row_end that is one too, or the height, passes: whole sample blocks per band)
    if (t.row_end % rs.factor)
        return fail(c, SWR_ERR_BAD_ARG, "supersampled resolve: the band's row_end %d is not a multiple of the factor %d", t.row_end, rs.factor);
    return SWR_OK;
}

// swr_read_color_resolved / swr_read_depth_resolved (one image) and the gather of swr_render_resolved (both, one launch): the last
// frame's band, resolved by rs.factor, into rows [row_begin / S, row_end / S) of the caller's (W/S) x (H/S) images.  NULL: not wanted.
int band_read_resolved(swr_context* c, swr_resolve rs, void* color_dst, float* depth_dst) {
    if (const int f = sticky(c)) return f;
    int rc;
    if (rs.factor == 1) {       // one sample per pixel: the plain read
        if (color_dst && (rc = single_read(c, 0, color_dst))) return rc;
        return depth_dst ? single_read(c, 1, depth_dst) : SWR_OK;
    }
    if ((rc = single_sync(c))) return rc;       // (an overflowed last frame is repaired here)
    if (tiles_of(c->tg) == 0) return SWR_OK;
    const int S = rs.factor, fb = c->fb_last;
    // (row_begin is a multiple of the tile height and row_end one too or the height, itself a multiple of S: whole sample blocks)
    const int rows = c->tg.row_end - c->tg.row_begin;
    const size_t row = (size_t)(c->tg.width / S) * 4, bytes = row * (size_t)(rows / S);
    if (color_dst && (rc = ensure(c, c->rs_color, bytes))) return rc;
    if (depth_dst && (rc = ensure(c, c->rs_depth, bytes))) return rc;
    launch_resolve(color_dst ? c->color[fb].p : nullptr, depth_dst ? c->depth[fb].p : nullptr, c->rs_color.p, c->rs_depth.p,
                   c->tg.width, rows, S, rs.depth_filter, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->frame_done[fb], c->stream));
    const uint64_t frame = c->frame_no ? c->frame_no - 1 : 0;
    const int64_t r0 = c->tg.row_begin / S, r1 = c->tg.row_end / S;
    if (color_dst && (rc = copy_band(c, fb, 0, c->rs_color.p, row, r0, r1, color_dst, frame))) return rc;
    if (depth_dst && (rc = copy_band(c, fb, 1, c->rs_depth.p, row, r0, r1, depth_dst, frame))) return rc;
    if (color_dst && (rc = wait_stream(c, c->copy_stream[0], "colour copy stream"))) return or_sticky(c, rc);
    if (depth_dst && (rc = wait_stream(c, c->copy_stream[1], "depth copy stream"))) return or_sticky(c, rc);
    return SWR_OK;
}

// what a swr_id_count may hold, and its rectangle against the full target
int check_count(swr_context* c, const swr_id_count& q, const uint32_t* counts, int64_t n) {
    if (q.group != SWR_COUNT_PER_PRIMITIVE && q.group != SWR_COUNT_PER_ITEM)
        return fail(c, SWR_ERR_BAD_ARG, "swr_count_ids: unknown group %d", q.group);
    if (q.reserved[0] || q.reserved[1] || q.reserved[2]) return fail(c, SWR_ERR_BAD_ARG, "swr_count_ids: reserved words must be 0");
    if (n < 0 || (n > 0 && !counts)) return fail(c, SWR_ERR_BAD_ARG, "swr_count_ids: counts is NULL or n is negative (n = %lld)", (long long)n);
    if (!c->has_target) return fail(c, SWR_ERR_NO_SCENE, "swr_count_ids needs swr_target_set first");
    const Target& t = c->tg;
    if (q.x0 < 0 || q.y0 < 0 || q.x0 > q.x1 || q.y0 > q.y1 || q.x1 > t.width || q.y1 > t.height)
        return fail(c, SWR_ERR_BAD_ARG, "swr_count_ids: the rectangle [%d,%d) x [%d,%d) is inverted or outside the target %dx%d",
                    q.x0, q.x1, q.y0, q.y1, t.width, t.height);
    return SWR_OK;
}

// swr_count_ids on one band: the part of the rectangle in the band's rows, counted into c->count_host.p[0 .. n] (word n: SWR_ID_NONE).
// A band the rectangle misses, or one without tiles, launches nothing and leaves zeros there.
int band_count_ids(swr_context* c, swr_id_count q, int64_t n) {
    if (const int f = sticky(c)) return f;
    int rc;
    if (!c->ids_valid)
        return fail(c, SWR_ERR_BAD_ARG, "swr_count_ids: the last frame was drawn without SWR_FLAG_PRIMITIVE_IDS, or swr_target_set / "
                    "swr_target_write / swr_scene_upload came after it");
    const bool per_item = q.group == SWR_COUNT_PER_ITEM;
    const int64_t need = per_item ? (c->last_draw.is_list ? (int64_t)c->last_draw.list.size() : 1) : (c->last_draw.is_list ? c->last_draw.list_tris : c->ni / 3);
    if (n != need)
        return fail(c, SWR_ERR_BAD_ARG, "swr_count_ids: n is %lld, but the last frame has %lld %s", (long long)n, (long long)need,
                    per_item ? "draw items" : "primitives");
    if ((rc = single_sync(c))) return rc;       // (an overflowed last frame is repaired here)
    const size_t words = (size_t)n + 1;
    if ((rc = ensure_host(c, c->count_host, words))) return rc;
    memset(c->count_host.p, 0, words * 4);
    const int y0 = std::max<int>(q.y0, c->tg.row_begin), y1 = std::min<int>(q.y1, c->tg.row_end);
    if (tiles_of(c->tg) == 0 || y0 >= y1 || q.x0 >= q.x1) return SWR_OK;
    if ((rc = ensure(c, c->count_dev, words * 4))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->count_dev.p, 0, words * 4, c->stream));
    const ListItem* items = (per_item && c->last_draw.is_list) ? (const ListItem*)c->slot[c->last_slot].items.p : nullptr;
    launch_count_ids((const uint32_t*)c->ids[c->fb_last].p, c->tg.width, q.x0, q.x1, y0 - c->tg.row_begin, y1 - c->tg.row_begin,
                     per_item ? 1 : 0, items, (uint32_t*)c->count_dev.p, n, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->count_host.p, c->count_dev.p, words * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c, c->stream, "raster stream (visibility counts)"))) return or_sticky(c, rc);
    return SWR_OK;
}

// what swr_query_depth may be handed, and every box against the full target
int check_query(swr_context* c, const swr_depth_box* boxes, int64_t n, const uint32_t* passed) {
    if (n < 0 || (n > 0 && (!boxes || !passed)))
        return fail(c, SWR_ERR_BAD_ARG, "swr_query_depth: boxes or passed is NULL, or n is negative (n = %lld)", (long long)n);
    if (n > SWR_DEPTH_QUERY_MAX)
        return fail(c, SWR_ERR_UNSUPPORTED, "swr_query_depth: %lld boxes, at most %d per call", (long long)n, SWR_DEPTH_QUERY_MAX);
    if (!c->has_target) return fail(c, SWR_ERR_NO_SCENE, "swr_query_depth needs swr_target_set first");
    const Target& t = c->tg;
    for (int64_t k = 0; k < n; k++) {
        const swr_depth_box& b = boxes[k];
        if (b.reserved[0] || b.reserved[1] || b.reserved[2])
            return fail(c, SWR_ERR_BAD_ARG, "swr_query_depth: box %lld: reserved words must be 0", (long long)k);
        if (b.x0 < 0 || b.y0 < 0 || b.x0 > b.x1 || b.y0 > b.y1 || b.x1 > t.width || b.y1 > t.height)
            return fail(c, SWR_ERR_BAD_ARG, "swr_query_depth: box %lld: the rectangle [%d,%d) x [%d,%d) is inverted or outside the target %dx%d",
                        (long long)k, b.x0, b.x1, b.y0, b.y1, t.width, t.height);
    }
    return SWR_OK;
}

// swr_query_depth on one band: the part of every box in the band's rows, tested against the band's depth image — the buffer
// single_read copies for swr_read_depth — into c->query_passed[0 .. n).  A band no box touches, or one without tiles, launches nothing
// and leaves zeros there.
int band_query_depth(swr_context* c, const swr_depth_box* boxes, int64_t n) {
    if (const int f = sticky(c)) return f;
    int rc;
    if ((rc = single_sync(c))) return rc;       // (an overflowed last frame is repaired here)
    c->query_passed = nullptr;
    if (n == 0) return SWR_OK;
    const size_t nn = (size_t)n, words = nn * 8 + nn + nn;      // boxes | large | passed
    if ((rc = ensure_host(c, c->query_host, words))) return rc;
    uint32_t* large = c->query_host.p + nn * 8;
    uint32_t* out = c->query_host.p + nn * 9;
    memcpy(c->query_host.p, boxes, nn * 32);
    memset(out, 0, nn * 4);
    c->query_passed = out;
    // the boxes' parts in this band: their total area, and the ones large enough to be split across workgroups
    uint64_t total_area = 0;
    size_t nlarge = 0;
    for (size_t k = 0; k < nn; k++) {
        const swr_depth_box& b = boxes[k];
        const int64_t h = (int64_t)std::min<int>(b.y1, c->tg.row_end) - (int64_t)std::max<int>(b.y0, c->tg.row_begin);
        if (h <= 0 || b.x1 <= b.x0) continue;
        const uint64_t area = (uint64_t)h * (uint64_t)(b.x1 - b.x0);
        total_area += area;
        if (area >= DEPTH_QUERY_SPLIT_AREA) large[nlarge++] = (uint32_t)k;
        // right after swr_target_set the image is the cleared one, whatever the buffers hold (the clear itself waits for the first
        // frame): every pixel is +inf, and the answer needs no device
        if (c->src_clear && b.z < std::numeric_limits<float>::infinity()) out[k] = (uint32_t)area;
    }
    if (tiles_of(c->tg) == 0 || total_area == 0 || c->src_clear) return SWR_OK;
    if ((rc = ensure(c, c->query_dev, words * 4))) return rc;
    if ((rc = ensure(c, c->query_tiles, depth_query_scratch_bytes(c->tg.width, c->tg.row_end - c->tg.row_begin)))) return rc;
    uint32_t* dev = (uint32_t*)c->query_dev.p;
    HIP_TRY(c, hipMemcpyAsync(dev, c->query_host.p, (nn * 8 + nlarge) * 4, hipMemcpyHostToDevice, c->stream));
    launch_depth_query((const float*)c->depth[c->fb_last].p, c->tg.width, c->tg.row_end - c->tg.row_begin, c->tg.row_begin,
                       (const swr_depth_box*)dev, n, dev + nn * 8, (int64_t)nlarge, total_area, c->query_tiles.p, dev + nn * 9, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, dev + nn * 9, nn * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c, c->stream, "raster stream (depth query)"))) return or_sticky(c, rc);
    return SWR_OK;
}

#ifndef SWR_TUNE_ITEM_BOUNDS
#define SWR_TUNE_ITEM_BOUNDS (-1)   // -1 = the product: k_item_bounds walks the stream, cut at the items' boundaries, one pass per item;
                                    // the A/B builds of DESIGN.md §25: 1 = it gathers the items' triangles through the index array
                                    // instead and the stream is not cut; 2 = instancing: an item over the range of the item before it
                                    // gets no work units, the workgroups of the first apply every matrix of the run
#endif

// what swr_item_bounds may be handed: swr_draw_list's own checks, then what the call adds to them
int check_bounds(swr_context* c, const swr_draw_item* items, int32_t n, uint32_t flags, const swr_item_bound* out) {
    int64_t tris = 0;
    const int rc = check_list_args(c, items, n, flags, &tris);
    if (rc) return rc;
    if (flags & SWR_FLAG_DEPTH_CLIP)
        return fail(c, SWR_ERR_UNSUPPORTED, "swr_item_bounds: SWR_FLAG_DEPTH_CLIP (the rectangle of a clipped fan is not its triangle's)");
    if (n > 0 && !out) return fail(c, SWR_ERR_BAD_ARG, "swr_item_bounds: out is NULL");
    return SWR_OK;
}

// swr_item_bounds on one band (a group: its first): the n records into c->bounds_out[0 .. n), inside the band's page-locked staging.
// The items are resolved and the stream is cut as single_draw_list does, so the same list drawn afterwards finds its cuts in place.
int band_item_bounds(swr_context* c, const swr_draw_item* items, int32_t n, uint32_t flags) {
    if (const int f = sticky(c)) return f;
    int rc;
    if ((rc = single_sync(c))) return rc;       // (an overflowed last frame is repaired here)
    c->bounds_out = nullptr;
    if (n == 0) return SWR_OK;
    const size_t nn = (size_t)n, item_words = sizeof(ListItem) / 4, rec_words = sizeof(swr_item_bound) / 4;
    const size_t words = nn * (item_words + rec_words);         // items | records
    if ((rc = ensure_host(c, c->bounds_host, words))) return rc;
    ListItem* list = (ListItem*)c->bounds_host.p;
    swr_item_bound* rec = (swr_item_bound*)(c->bounds_host.p + nn * item_words);
    memset(rec, 0, nn * sizeof(swr_item_bound));
    std::vector<uint32_t> need;             // the cuts the stream needs
    const int64_t ntri = c->ni / 3;
    int64_t units = 0;
    for (size_t k = 0; k < nn; k++) {
        ListItem& it = list[k];
        it.first = (uint32_t)(items[k].first_index / 3);
        it.count = (uint32_t)(items[k].index_count / 3);
        it.vbase = 0;
        it.ubase = (uint32_t)units;
        memcpy(it.m, items[k].transform, sizeof it.m);
        const bool follows = SWR_TUNE_ITEM_BOUNDS == 2 && k > 0 && it.first == list[k - 1].first && it.count == list[k - 1].count;
        if (!follows) units += item_bounds_units(it.count);
        if (it.count && it.first > 0) need.push_back(it.first);
        if (it.count && (int64_t)it.first + it.count < ntri) need.push_back(it.first + it.count);
    }
    if (SWR_TUNE_ITEM_BOUNDS != 1 && (rc = cut_stream(c, need))) return rc;
    if ((rc = ensure(c, c->bounds_dev, words * 4))) return rc;
    if ((rc = ensure(c, c->bounds_scratch, item_bounds_scratch_bytes(n)))) return rc;
    uint32_t* dev = (uint32_t*)c->bounds_dev.p;
    HIP_TRY(c, hipMemcpyAsync(dev, list, nn * sizeof(ListItem), hipMemcpyHostToDevice, c->stream));
    ItemBoundsArgs a{};
    a.tri_xyz = (const float4*)c->tri_xyz.p;
    a.vertices = (const swr_vertex*)(c->pose_active ? c->posed.p : c->morph_active ? c->morphed.p : c->vertices.p);
    a.indices = (const int64_t*)c->indices.p;
    a.items = (const ListItem*)dev;
    a.n = n;
    a.width = c->tg.width; a.height = c->tg.height;
    a.metal = (flags & SWR_FLAG_METAL_RULES) ? 1 : 0;
    a.units = units;
    a.scratch = c->bounds_scratch.p;
    a.records = (swr_item_bound*)(dev + nn * item_words);
    launch_item_bounds(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(rec, a.records, nn * sizeof(swr_item_bound), hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c, c->stream, "raster stream (item bounds)"))) return or_sticky(c, rc);
    c->bounds_out = rec;
    return SWR_OK;
}

// what swr_cast_rays and swr_query_rays (`fn`, with flags 0) may be handed (include/swr.h "Ray casts"): on a band or a group alike,
// against the scene every band holds
int check_rays(swr_context* c, const char* fn, const swr_ray* rays, int64_t n, uint32_t flags, const swr_ray_hit* hits) {
    if (!band(c, 0)->has_scene) return fail(c, SWR_ERR_NO_SCENE, "%s needs swr_scene_upload first", fn);
    if (n < 0) return fail(c, SWR_ERR_BAD_ARG, "%s: n %lld", fn, (long long)n);
    if (flags != 0) return fail(c, SWR_ERR_BAD_ARG, "%s: unknown flags 0x%x", fn, (unsigned)flags);
    if (n > SWR_RAYS_MAX) return fail(c, SWR_ERR_UNSUPPORTED, "%s: %lld rays (at most %d)", fn, (long long)n, SWR_RAYS_MAX);
    if (n > 0 && !rays) return fail(c, SWR_ERR_BAD_ARG, "%s: rays is NULL", fn);
    if (n > 0 && !hits) return fail(c, SWR_ERR_BAD_ARG, "%s: hits is NULL", fn);
    for (int64_t k = 0; k < n; k++) {
        const swr_ray& r = rays[k];
        const float f[8] = {r.origin[0], r.origin[1], r.origin[2], r.tmin, r.dir[0], r.dir[1], r.dir[2], r.tmax};
        for (int j = 0; j < 8; j++)
            if (!std::isfinite(f[j])) return fail(c, SWR_ERR_BAD_ARG, "%s: ray %lld: float %d is not finite", fn, (long long)k, j);
        if (r.dir[0] == 0.0f && r.dir[1] == 0.0f && r.dir[2] == 0.0f)
            return fail(c, SWR_ERR_BAD_ARG, "%s: ray %lld: the direction is zero", fn, (long long)k);
        if (r.tmin > r.tmax) return fail(c, SWR_ERR_BAD_ARG, "%s: ray %lld: tmin %g > tmax %g", fn, (long long)k, r.tmin, r.tmax);
    }
    return SWR_OK;
}

// the query swr_cast_rays is, resolved over ntri primitives: every primitive, both facings, the nearest hit
inline swr_ray_query default_ray_query(int64_t ntri) { return swr_ray_query{0, 0, 0, ntri}; }

// what swr_query_rays may be handed as its query (include/swr.h "Ray queries"), the scene being there: `q` = the query with its
// defaults filled in and primitive_count resolved, which is what band_cast_rays takes.  query == NULL: the defaults.
int check_ray_query(swr_context* c, const swr_ray_query* query, swr_ray_query& q) {
    const char* fn = "swr_query_rays";
    const int64_t ntri = band(c, 0)->ni / 3;
    q = default_ray_query(ntri);
    if (!query) return SWR_OK;
    const uint32_t known = SWR_RAYS_ANY_HIT | SWR_RAYS_CULL_BACK | SWR_RAYS_CULL_FRONT | SWR_RAYS_FRONT_CW;
    if (query->flags & ~known) return fail(c, SWR_ERR_BAD_ARG, "%s: unknown flags 0x%x", fn, (unsigned)query->flags);
    if (query->reserved != 0) return fail(c, SWR_ERR_BAD_ARG, "%s: reserved is 0x%x, not 0", fn, (unsigned)query->reserved);
    if (query->first_primitive < 0) return fail(c, SWR_ERR_BAD_ARG, "%s: first_primitive %lld", fn, (long long)query->first_primitive);
    if (query->primitive_count < -1) return fail(c, SWR_ERR_BAD_ARG, "%s: primitive_count %lld", fn, (long long)query->primitive_count);
    // (first <= ntri first: the sum below then cannot overflow)
    if (query->first_primitive > ntri || (query->primitive_count >= 0 && query->primitive_count > ntri - query->first_primitive))
        return fail(c, SWR_ERR_BAD_ARG, "%s: primitives %lld + %lld end beyond the scene's %lld", fn, (long long)query->first_primitive,
                    (long long)query->primitive_count, (long long)ntri);
    q.flags = query->flags;
    q.first_primitive = query->first_primitive;
    q.primitive_count = query->primitive_count < 0 ? ntri - query->first_primitive : query->primitive_count;
    return SWR_OK;
}

// swr_cast_rays / swr_query_rays on one band (a group: its first): the n hits into c->rays_out[0 .. n), inside the band's page-locked
// staging.  `q` is a checked query (check_ray_query).  The stream read is the resident one as it is now — cut by an earlier draw list
// or not, never a frame's clip stream — and nothing of the context but the call's own buffers is written.
int band_cast_rays(swr_context* c, const swr_ray_query& q, const swr_ray* rays, int64_t n) {
    if (const int f = sticky(c)) return f;
    int rc;
    if ((rc = single_sync(c))) return rc;       // (an overflowed last frame is repaired here)
    c->rays_out = nullptr;
    if (n == 0) return SWR_OK;
    const size_t nn = (size_t)n, ray_words = sizeof(swr_ray) / 4, hit_words = sizeof(swr_ray_hit) / 4;
    if ((rc = ensure_host(c, c->rays_host, nn * (ray_words + hit_words)))) return rc;       // rays | hits
    swr_ray* in = (swr_ray*)c->rays_host.p;
    swr_ray_hit* out = (swr_ray_hit*)(c->rays_host.p + nn * ray_words);
    memcpy(in, rays, nn * sizeof(swr_ray));
    memset(out, 0, nn * sizeof(swr_ray_hit));
    if ((rc = ensure(c, c->rays_dev, nn * sizeof(swr_ray)))) return rc;
    if ((rc = ensure(c, c->rays_keys, nn * 8))) return rc;
    if ((rc = ensure(c, c->rays_hits, nn * sizeof(swr_ray_hit)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->rays_dev.p, in, nn * sizeof(swr_ray), hipMemcpyHostToDevice, c->stream));
    RaysArgs a{};
    a.tri_xyz = (const float4*)c->tri_xyz.p;
    a.box64 = (const float4*)c->box64.p;
    a.inv = (const uint32_t*)c->inv.p;
    a.reordered = c->reordered ? 1 : 0;
    a.ntri = c->ni / 3;
    a.groups = (a.ntri + 63) / 64;
    a.rays = (const swr_ray*)c->rays_dev.p;
    a.n = n;
    a.keys = (unsigned long long*)c->rays_keys.p;
    a.hits = (swr_ray_hit*)c->rays_hits.p;
    a.flags = q.flags;
    a.p_begin = q.first_primitive;
    a.p_end = q.first_primitive + q.primitive_count;
    launch_cast_rays(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, a.hits, nn * sizeof(swr_ray_hit), hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c, c->stream, "raster stream (ray casts)"))) return or_sticky(c, rc);
    c->rays_out = out;
    return SWR_OK;
}

#ifndef SWR_TUNE_DELTA_DIRECT
#define SWR_TUNE_DELTA_DIRECT 1    // how the changed part reaches a page-locked destination, chosen by measurement:
                                    // 1 = k_delta_tiles stores the changed tiles straight into the caller's image through its
                                    // device address (the product: 0.05 against 0.13 ms on the app's scene at 4K); 0 = R gathered
                                    // on the device, one linear copy into page-locked staging, rows copied by the host — what a
                                    // pageable destination always takes (A/B builds)
#endif

// swr_read_color_delta / swr_read_depth_delta on one band (img: 0 colour, 1 depth): the band's rows of `dst`, which hold what the last
// delta read of this kind delivered, become what single_read would deliver now; only the bounding box of the tiles that differ from
// the band's baseline is written.  What was done is left in c->delta_stats.
int check_delta(swr_context* c, const void* dst) {
    if (!dst) return fail(c, SWR_ERR_BAD_ARG, "swr_read_*_delta: the destination is NULL");
    if (!c->has_target) return fail(c, SWR_ERR_NO_SCENE, "swr_read_*_delta needs swr_target_set first");
    return SWR_OK;
}

int band_read_delta(swr_context* c, int img, void* dst) {
    if (const int f = sticky(c)) return f;
    int rc = single_sync(c);        // (an overflowed last frame is repaired here)
    if (rc) return rc;
    swr_delta_stats st{};
    c->delta_stats = st;
    const int tiles = tiles_of(c->tg);
    if (tiles == 0) return SWR_OK;
    const int W = c->tg.width, rows = c->tg.row_end - c->tg.row_begin, fb = c->fb_last;
    const size_t row = (size_t)W * 4, bytes = row * (size_t)rows;
    DevBuf& base = c->delta_base[img];
    if (base.bytes < bytes) c->delta_valid[img] = false;        // (never: a target of another size has dropped the baseline already)
    if ((rc = ensure(c, base, bytes))) return rc;
    if ((rc = ensure(c, c->delta_flags, (size_t)tiles * 4))) return rc;
    if ((rc = ensure_host(c, c->delta_host, (size_t)tiles))) return rc;
    const uint32_t* cur = (const uint32_t*)fb_image(c, fb, img);
    uint8_t* band_dst = (uint8_t*)dst + (size_t)c->tg.row_begin * row;
    const uint64_t frame = c->frame_no ? c->frame_no - 1 : 0;
    st.tiles = tiles;
    // the whole band, as single_read delivers it (no baseline, or every tile row and column changed)
    auto whole_band = [&]() -> int {
        HIP_TRY(c, hipEventRecord(c->frame_done[fb], c->stream));
        int rcw = copy_band(c, fb, img, cur, row, c->tg.row_begin, c->tg.row_end, dst, frame);
        if (rcw) return rcw;
        if ((rcw = wait_stream(c, c->copy_stream[img], "copy stream (delta read)"))) return or_sticky(c, rcw);
        st.x0 = 0; st.y0 = c->tg.row_begin; st.x1 = W; st.y1 = c->tg.row_end;
        st.bytes_copied = (int64_t)bytes;
        return SWR_OK;
    };
    if (!c->delta_valid[img]) {
        launch_delta(cur, (uint32_t*)base.p, 0, W, rows, (uint32_t*)c->delta_flags.p, nullptr, c->stream);
        HIP_TRY(c, hipGetLastError());
        if ((rc = whole_band())) return rc;
        if ((rc = wait_stream(c, c->stream, "raster stream (delta read)"))) return or_sticky(c, rc);
        c->delta_valid[img] = true;
        st.tiles_changed = tiles;
        st.full = 1;
        c->delta_stats = st;
        return SWR_OK;
    }
    uint32_t* direct = nullptr;
    if (SWR_TUNE_DELTA_DIRECT && is_pinned(band_dst)) {
        if (hipHostGetDevicePointer((void**)&direct, band_dst, 0) != hipSuccess) { (void)hipGetLastError(); direct = nullptr; }
    }
    launch_delta(cur, (uint32_t*)base.p, 1, W, rows, (uint32_t*)c->delta_flags.p, direct, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->delta_host.p, c->delta_flags.p, (size_t)tiles * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c, c->stream, "raster stream (delta read)"))) return or_sticky(c, rc);
    // the changed tiles: their number, their bounding box in tiles, and the pixels they hold
    int tx0 = c->tg.tiles_x, tx1 = -1, ty0 = c->tg.tiles_y, ty1 = -1;
    int64_t changed = 0, changed_px = 0;
    for (int ty = 0; ty < c->tg.tiles_y; ty++)
        for (int tx = 0; tx < c->tg.tiles_x; tx++) {
            if (!c->delta_host.p[(size_t)ty * c->tg.tiles_x + tx]) continue;
            changed++;
            changed_px += (int64_t)(std::min(W, (tx + 1) * TILE_W) - tx * TILE_W) * (std::min(rows, (ty + 1) * TILE_H) - ty * TILE_H);
            tx0 = std::min(tx0, tx); tx1 = std::max(tx1, tx);
            ty0 = std::min(ty0, ty); ty1 = std::max(ty1, ty);
        }
    st.tiles_changed = changed;
    if (changed == 0) { c->delta_stats = st; return SWR_OK; }
    // R, in columns and band-local rows
    const int x0 = tx0 * TILE_W, x1 = std::min(W, (tx1 + 1) * TILE_W), y0 = ty0 * TILE_H, y1 = std::min(rows, (ty1 + 1) * TILE_H);
    if (direct) {       // (the kernel has stored the changed tiles already)
        st.x0 = x0; st.x1 = x1; st.y0 = c->tg.row_begin + y0; st.y1 = c->tg.row_begin + y1;
        st.bytes_copied = changed_px * 4;
    } else if (x0 == 0 && x1 == W && y0 == 0 && y1 == rows) {
        if ((rc = whole_band())) return rc;
    } else {
        // R's rows gathered on the device, moved through the page-locked stage chunks, and copied row by row into the caller's image
        const size_t rrow = (size_t)(x1 - x0) * 4, rbytes = rrow * (size_t)(y1 - y0);
        if ((rc = ensure(c, c->delta_pack, rbytes)) || (rc = ensure_stage(c, img))) return rc;
        launch_delta_pack(cur, W, x0, x1, y0, y1, (uint32_t*)c->delta_pack.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        const uint8_t* src = (const uint8_t*)c->delta_pack.p;
        const size_t CH = swr_context::STAGE_BYTES, n = (rbytes + CH - 1) / CH;
        for (size_t k = 0; k <= n; k++) {
            if (k < n) {
                HIP_TRY(c, hipMemcpyAsync(c->stage[img][k & 1], src + k * CH, std::min(CH, rbytes - k * CH), hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, hipEventRecord(c->stage_ev[img][k & 1], c->stream));
            }
            if (k > 0) {
                const size_t j = k - 1;
                if ((rc = poll_event(c, c->stage_ev[img][j & 1], "a staged copy to the host (delta read)", frame))) return rc;
                const uint8_t* from = c->stage[img][j & 1];
                for (size_t off = j * CH, left = std::min(CH, rbytes - j * CH); left;) {       // (a chunk may start and end inside a row)
                    const size_t r = off / rrow, col = off - r * rrow, len = std::min(left, rrow - col);
                    memcpy(band_dst + ((size_t)y0 + r) * row + (size_t)x0 * 4 + col, from, len);
                    off += len; left -= len; from += len;
                }
            }
        }
        st.x0 = x0; st.x1 = x1; st.y0 = c->tg.row_begin + y0; st.y1 = c->tg.row_begin + y1;
        st.bytes_copied = (int64_t)rbytes;
    }
    c->delta_stats = st;
    return SWR_OK;
}

// Stop the helpers, wait (bounded) for the streams, delete the context: what it owns frees itself (see "ORDER OF FREEING").  A context
// whose streams do not drain is leaked whole instead — no HIP free or destroy call is made while the GPU may still use its memory.
void destroy_single(swr_context* c) {
    hipSetDevice(c->device);
    // helper jobs are bounded (every wait in them is) and give up at once on a failed context: the drains return
    for (std::unique_ptr<Worker>* w : {&c->ts.ras_worker, &c->ts.bin_worker})
        if (*w) { (*w)->drain(); w->reset(); }
    // bounded too: a GPU that never finishes must not hang the destructor (what it still owns is then leaked)
    c->wait_budget_ms = std::min<uint32_t>(c->wait_budget_ms, 5000u);
    auto drain = [c](hipStream_t st) {           // (looks at the stream, not at the failed flag: the GPU may be fine)
        if (!st) return true;
        Deadline d(c);
        for (;;) {
            const hipError_t e = hipStreamQuery(st);
            if (e == hipSuccess) return true;
            if (e != hipErrorNotReady) return false;
            (void)hipGetLastError();
            if (!d.pause()) return false;
        }
    };
    bool drained = drain(c->bin_stream) && drain(c->stream) && drain(c->copy_stream[0]) && drain(c->copy_stream[1]);
    for (hipStream_t ls : c->lane_stream) drained = drained && drain(ls);
    if (!drained) {
        fprintf(stderr, "[swr] context on device %d destroyed in a failed state (%s); device memory it may still be using is not freed\n",
                c->device, c->failed_msg.c_str());
        return;         // (the context object goes with it: a few KB of host memory beside everything the device holds)
    }
    if (c->hp_on && c->hp_frames)
        fprintf(stderr, "[swr host profile] device %d, %llu frames, us/frame: prepare %.2f | wait(slot) %.2f | binning launches %.2f | "
                        "event record+wait %.2f | raster-stream launches %.2f | record(ras_done) %.2f\n", c->device,
                (unsigned long long)c->hp_frames, c->hp_t[0] / c->hp_frames, c->hp_t[1] / c->hp_frames, c->hp_t[2] / c->hp_frames,
                c->hp_t[3] / c->hp_frames, c->hp_t[4] / c->hp_frames, c->hp_t[5] / c->hp_frames);
    delete c;
}

// helpers: 2 = a binning and a raster helper (a single-device context), 1 = the raster helper only — the thread that
// calls swr_draw enqueues the binning itself (sub-contexts of a group: that thread is the group's per-device worker, so
// a device has ONE thread that polls for completions, not two), 0 = none.
int create_single(int dev, swr_context** out, int helpers, uint32_t wait_budget_ms) {
    std::unique_ptr<swr_context> c(new swr_context());      // (a failure below frees what was created so far; nothing is enqueued yet)
    c->device = dev;
    if (wait_budget_ms) c->wait_budget_ms = wait_budget_ms;
    c->hp_on = getenv("SWR_HOST_PROFILE") && atoi(getenv("SWR_HOST_PROFILE")) == 1;
    hipError_t e;
    if ((e = hipSetDevice(dev)) != hipSuccess || (e = prepare_device()) != hipSuccess ||
        (e = c->stream.create()) != hipSuccess || (e = c->copy_stream[0].create()) != hipSuccess ||
        (e = c->copy_stream[1].create()) != hipSuccess ||
        (e = c->h_pairs.alloc((2 * swr_context::PAIR_RING + 2) * 4, hipHostMallocMapped)) != hipSuccess ||
        (e = hipHostGetDevicePointer((void**)&c->h_pairs_dev, c->h_pairs, 0)) != hipSuccess ||
        (e = c->h_misc.alloc(CNT_WORDS * 4, hipHostMallocDefault)) != hipSuccess ||
        (e = c->h_clip.alloc((swr_context::PAIR_RING + 1) * 4, hipHostMallocMapped)) != hipSuccess ||
        (e = hipHostGetDevicePointer((void**)&c->h_clip_dev, c->h_clip, 0)) != hipSuccess)
        return fail(nullptr, SWR_ERR_HIP, "context init on device %d failed: %s", dev, hipGetErrorString(e));
    memset(c->h_pairs, 0, (2 * swr_context::PAIR_RING + 2) * 4);
    c->h_pairs[swr_context::PAIR_RING] = 0xFFFFFFFFu;     // fullest bin: unknown
    memset(c->h_misc, 0, CNT_WORDS * 4);
    memset(c->h_clip, 0, (swr_context::PAIR_RING + 1) * 4);
    {
        // SWR_PIPELINE=0: binning and raster share one stream (no overlap of consecutive frames)
        const char* pl = getenv("SWR_PIPELINE");
        if (pl && pl[0] == '0') c->bin_stream = c->stream;
        else {
            // a plain second stream: stream priorities (binning highest or lowest) were measured to make
            // no difference to how the two queues share the CUs on this platform
            c->bin_stream = c->bin_stream_own.create() == hipSuccess ? c->bin_stream_own.h : c->stream.h;
            // SWR_HOST_THREADS=1: enqueue everything from the caller's thread (no helper)
            const char* ht = getenv("SWR_HOST_THREADS");
            if (ht && ht[0] == '1') helpers = 0;
            { const char* be = getenv("SWR_BIND_EVENTS"); c->ts.bind_events = !(be && be[0] == '0'); }
            { const char* ii = getenv("SWR_INLINE_IDLE"); c->ts.inline_idle = !(ii && ii[0] == '0'); }
            const char* ew = getenv("SWR_EVENT_WAITS");     // =1: no raster helper; the caller's thread orders the streams by event waits
            if (c->bin_stream_own && helpers >= 2) { c->ts.bin_worker.reset(new Worker()); c->ts.bin_worker->start(dev, true); }
            if (c->bin_stream_own && helpers >= 1 && !(ew && ew[0] == '1')) { c->ts.ras_worker.reset(new Worker()); c->ts.ras_worker->start(dev, true); }
        }
        for (int k = 0; k < swr_context::NSLOT; k++) {
            c->slot[k].bin_done.create(hipEventDisableTiming);
            c->ts.ras_done[k].ev.create(hipEventDisableTiming);
        }
        for (int i = 0; i < swr_context::NFB; i++) {
            c->frame_done[i].create(hipEventDisableTiming);
            for (int j = 0; j < 2; j++) c->copy_done[i][j].create(hipEventDisableTiming);
            c->read_done[i].create(hipEventDisableTiming);
        }
        c->src_ready.create(hipEventDisableTiming);
        // frame lanes (swr_context::lane_stream): one stream per working set.  SWR_LANES=0: the two-stream pipeline of rounds 1-3
        {
            const char* ln = getenv("SWR_LANES");
            c->lanes_ok = c->bin_stream_own && !(ln && ln[0] == '0');
            for (int l = 0; l < swr_context::NSLOT && c->lanes_ok; l++)
                if (c->lane_stream[l].create() != hipSuccess) c->lanes_ok = false;
            for (Event& e : c->pace_ev) e.create(hipEventDisableTiming);
        }
    }
    for (int r = 0; r < swr_context::RING; r++)
        for (int i = 0; i < 5; i++) c->ev[r][i].create();
    *out = c.release();
    return SWR_OK;
}

// ---- group fan-out -----------------------------------------------------------------------------------------------

// run fn(kid) on every sub-context's own thread and wait; the first failure (and its text) becomes the group's
template <class F>
int group_run(swr_context* g, F fn) {
    const size_t n = g->kids.size();
    for (size_t k = 0; k < n; k++) {
        swr_context* kid = g->kids[k];
        g->workers[k]->post([kid, fn] { return fn(kid); });
    }
    int first = SWR_OK;
    for (size_t k = 0; k < n; k++) {
        const int rc = g->workers[k]->drain();
        if (rc && !first) {
            first = rc;
            g->err = "device " + std::to_string(g->kids[k]->device) + " (band " + std::to_string(k) + "): " + g->kids[k]->err;
        }
    }
    return first;
}

// An entry point that waits: fn on every band of c — a group's on their own threads — and the wait for all of them.  Every such entry
// point has one shape: its NULL checks, sticky(c), the call's checks against c (check_X: once, before a band is touched), fan(c, the
// band's work), then one gather over the bands of c, which writes the caller's arrays only after every band succeeded.
template <class F>
int fan(swr_context* c, F fn) { return is_group(c) ? group_run(c, fn) : fn(c); }

// fire and forget (swr_draw / swr_present on a group): errors surface at the next group_run
template <class F>
void group_post(swr_context* g, F fn) {
    for (size_t k = 0; k < g->kids.size(); k++) {
        swr_context* kid = g->kids[k];
        g->workers[k]->post([kid, fn] { return fn(kid); });
    }
}

// tile-row band k of n inside [row_begin, row_end) (row_begin is tile-aligned)
void sub_band(int64_t row_begin, int64_t row_end, int n, int k, int64_t* r0, int64_t* r1) {
    const int64_t trows = (row_end - row_begin + TILE_H - 1) / TILE_H;
    *r0 = std::min<int64_t>(row_begin + trows * k / n * TILE_H, row_end);
    *r1 = std::min<int64_t>(row_begin + trows * (k + 1) / n * TILE_H, row_end);
}

}  // namespace

extern "C" {

int swr_abi_version(void) { return SWR_ABI_VERSION; }
const char* swr_version(void) { return "swr-hip gfx950 0.5 (tile 64x32, wave64 LDS visibility keys: 32-bit depth keys + winner table, span ring, one-launch binning, frame lanes, multi-device bands, load action)"; }
int swr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
int swr_tile_rows(void) { return TILE_H; }
int swr_tile_cols(void) { return TILE_W; }

const char* swr_last_error(const swr_context* ctx) {
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int swr_band_rows(int64_t height, int32_t parts, int32_t part, int64_t* row_begin, int64_t* row_end) {
    if (height <= 0 || parts <= 0 || part < 0 || part >= parts || !row_begin || !row_end)
        return SWR_ERR_BAD_ARG;
    sub_band(0, height, parts, part, row_begin, row_end);
    return SWR_OK;
}

int swr_context_create(const swr_config* cfg, swr_context** out) {
    if (!out) return fail(nullptr, SWR_ERR_BAD_ARG, "swr_context_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, SWR_ERR_HIP, "no HIP device (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    int dev = cfg ? cfg->device : -1;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) return fail(nullptr, SWR_ERR_BAD_ARG, "device %d out of range (%d devices)", dev, ndev);
    const uint32_t n = cfg ? cfg->device_count : 0;
    if (n > 64) return fail(nullptr, SWR_ERR_BAD_ARG, "device_count %u > 64", n);
    const uint32_t budget = cfg ? cfg->wait_budget_ms : 0u;
    if (n <= 1) return create_single(dev, out, 2, budget);
    // group: sub-context k on device (dev + k) % min(n, visible devices) — with fewer GPUs than bands several bands
    // share a GPU (same code path; how a 1-GPU box tests the 8-band layout)
    swr_context* g = new swr_context();
    g->device = dev;
    if (budget) g->wait_budget_ms = budget;
    const int span = std::min<int>((int)n, ndev);
    for (uint32_t k = 0; k < n; k++) {
        swr_context* kid = nullptr;
        int rc = create_single((dev + (int)(k % (uint32_t)span)) % ndev, &kid, 1, budget);
        if (rc) {
            for (swr_context* x : g->kids) destroy_single(x);
            delete g;
            return rc;
        }
        kid->band = (int)k;
        g->kids.push_back(kid);
    }
    for (uint32_t k = 0; k < n; k++) {
        g->workers.emplace_back(new Worker());
        g->workers[k]->start(g->kids[k]->device);
    }
    *out = g;
    return SWR_OK;
}

void swr_context_destroy(swr_context* c) {
    if (!c) return;
    if (is_group(c)) {
        for (auto& w : c->workers) w->drain();
        c->workers.clear();
        for (swr_context* kid : c->kids) destroy_single(kid);
        delete c;
        return;
    }
    destroy_single(c);
}

int swr_context_bands(const swr_context* c) { return c ? (int)band_count(c) : 0; }

int swr_context_band_info(const swr_context* c, int32_t band, int32_t* device, int64_t* row_begin, int64_t* row_end) {
    if (!c || band < 0 || band >= swr_context_bands(c)) return SWR_ERR_BAD_ARG;
    const swr_context* k = ::band(c, (size_t)band);
    if (device) *device = k->device;
    if (row_begin) *row_begin = k->has_target ? k->tg.row_begin : 0;
    if (row_end) *row_end = k->has_target ? k->tg.row_end : 0;
    return SWR_OK;
}

int swr_scene_upload(swr_context* c, const swr_vertex* vertices, int64_t vertex_count,
                     const int64_t* indices, int64_t index_count) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // the resident scene changes: a later swr_render must not take it for its own
    // (a group replicates the scene: every device reads the caller's arrays itself, over its own PCIe link)
    return fan(c, [=](swr_context* k) { return single_scene_upload(k, vertices, vertex_count, indices, index_count); });
}

int swr_scene_attributes(swr_context* c, const swr_vertex_attr* attributes, int64_t vertex_count) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // the resident scene changes: a later swr_render must not take it for its own
    return fan(c, [=](swr_context* k) { return single_scene_attributes(k, attributes, vertex_count); });
}

int swr_scene_skin(swr_context* c, const swr_skin_vertex* skin, int64_t vertex_count) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // the resident scene changes: a later swr_render must not take it for its own
    return fan(c, [=](swr_context* k) { return single_scene_skin(k, skin, vertex_count); });
}

int swr_pose_set(swr_context* c, const float* joints, int32_t joint_count) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // (the same)
    return fan(c, [=](swr_context* k) { return single_pose_set(k, joints, joint_count, false); });
}

int swr_pose_set_dq(swr_context* c, const float* dual_quats, int32_t joint_count) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // (the same)
    return fan(c, [=](swr_context* k) { return single_pose_set(k, dual_quats, joint_count, true); });
}

int swr_scene_morph(swr_context* c, const swr_morph_targets* targets) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // the resident scene changes: a later swr_render must not take it for its own
    return fan(c, [=](swr_context* k) { return single_scene_morph(k, targets); });
}

int swr_morph_set(swr_context* c, const float* weights, int32_t weight_count) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // (the same)
    return fan(c, [=](swr_context* k) { return single_morph_set(k, weights, weight_count); });
}

int swr_scene_morph_sparse(swr_context* c, const swr_morph_sparse* targets) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // (the same)
    return fan(c, [=](swr_context* k) { return single_scene_morph_sparse(k, targets); });
}

int swr_morph_pose_set(swr_context* c, const float* weights, int32_t weight_count, const float* joints, int32_t joint_count,
                       int32_t pose_kind) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // (the same)
    return fan(c, [=](swr_context* k) { return single_morph_pose_set(k, weights, weight_count, joints, joint_count, pose_kind); });
}

int swr_scene_normals(swr_context* c, const swr_normals* normals) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // (the same)
    return fan(c, [=](swr_context* k) { return single_scene_normals(k, normals); });
}

int swr_material_set(swr_context* c, const swr_material* m) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (is_group(c)) {
        const bool has = m != nullptr;
        const swr_material copy = has ? *m : swr_material{};
        return group_run(c, [=](swr_context* k) { return single_material_set(k, has ? &copy : nullptr); });
    }
    return single_material_set(c, m);
}

int swr_blend_set(swr_context* c, const swr_blend* b) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (is_group(c)) {
        // (validated on the group first: a rejected state reaches no band)
        int rc = single_blend_set(c, b);
        if (rc) return rc;
        const swr_blend copy = c->blend;
        return group_run(c, [=](swr_context* k) { return single_blend_set(k, &copy); });
    }
    return single_blend_set(c, b);
}

int swr_texture_upload(swr_context* c, const void* bgra8, int32_t width, int32_t height) {
    if (!c) return SWR_ERR_BAD_ARG;
    c->scene_id = 0;      // the resident scene changes: a later swr_render must not take it for its own
    return fan(c, [=](swr_context* k) { return single_texture_upload(k, bgra8, width, height); });
}

int swr_target_set(swr_context* c, int64_t width, int64_t height, int64_t row_begin, int64_t row_end) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (const int f = sticky(c)) return f;
    int rc = check_target_args(c, width, height, row_begin, row_end);
    if (rc) return rc;
    const int n = (int)band_count(c);       // (one band: its rows are the target's)
    rc = fan(c, [=](swr_context* k) {
        int64_t r0, r1;
        sub_band(row_begin, row_end, n, k->band, &r0, &r1);
        return single_target_set(k, width, height, r0, r1);
    });
    if (rc) return rc;
    if (is_group(c)) {      // the full target, for the checks of the calls that follow
        c->tg = Target{(int32_t)width, (int32_t)height, (int32_t)row_begin, (int32_t)row_end, 0, 0};
        c->has_target = true;
    }
    return SWR_OK;
}

int swr_draw_primitives(swr_context* c, const float transform[16], uint32_t flags, int32_t primitive_type) {
    if (!c || !transform) return SWR_ERR_BAD_ARG;
    if (!is_group(c)) return single_draw(c, transform, flags, primitive_type);
    int rc = check_draw_args(c, flags, primitive_type);
    if (rc) return rc;
    std::array<float, 16> m;
    memcpy(m.data(), transform, sizeof(float) * 16);
    group_post(c, [=](swr_context* k) { return single_draw(k, m.data(), flags, primitive_type); });
    return SWR_OK;      // asynchronous, like the single-device draw: a failure is reported by the next blocking call
}

int swr_draw(swr_context* c, const float transform[16], uint32_t flags) {
    return swr_draw_primitives(c, transform, flags, SWR_PRIMITIVE_TRIANGLE);
}

int swr_draw_list(swr_context* c, const swr_draw_item* items, int32_t item_count, uint32_t flags) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (const int f = sticky(c)) return f;
    int64_t tris = 0;
    const int rc = check_list_args(c, items, item_count, flags, &tris);
    if (rc) return rc;
    if (!is_group(c)) return single_draw_list(c, items, item_count, flags, tris);
    // asynchronous, like swr_draw: the bands draw their own copy of the list
    auto list = std::make_shared<std::vector<swr_draw_item>>(items, items + item_count);
    group_post(c, [=](swr_context* k) { return single_draw_list(k, list->data(), item_count, flags, tris); });
    return SWR_OK;
}

int swr_target_write(swr_context* c, const void* color_full, const float* depth_full) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (const int f = sticky(c)) return f;
    if (!c->has_target) return fail(c, SWR_ERR_NO_SCENE, "swr_target_write needs swr_target_set first");
    return fan(c, [=](swr_context* k) { return single_target_write(k, color_full, depth_full); });
}

int swr_sync(swr_context* c) {
    if (!c) return SWR_ERR_BAD_ARG;
    return fan(c, [](swr_context* k) { return single_sync(k); });
}

int swr_present(swr_context* c, void* color_full, float* depth_full) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (!is_group(c)) return single_present(c, color_full, depth_full);
    if (!color_full && !depth_full) return fail(c, SWR_ERR_BAD_ARG, "swr_present: both image pointers are NULL");
    group_post(c, [=](swr_context* k) { return single_present(k, color_full, depth_full); });
    return SWR_OK;
}

int swr_present_wait(swr_context* c) {
    if (!c) return SWR_ERR_BAD_ARG;
    return fan(c, [](swr_context* k) { return single_present_wait(k); });
}

int swr_read_color(swr_context* c, void* dst) {
    if (!c || !dst) return SWR_ERR_BAD_ARG;
    return fan(c, [=](swr_context* k) { return single_read(k, 0, dst); });
}

int swr_read_depth(swr_context* c, float* dst) {
    if (!c || !dst) return SWR_ERR_BAD_ARG;
    return fan(c, [=](swr_context* k) { return single_read(k, 1, dst); });
}

int swr_read_ids(swr_context* c, uint32_t* dst) {
    if (!c || !dst) return SWR_ERR_BAD_ARG;
    return fan(c, [=](swr_context* k) { return single_read(k, 2, dst); });
}

int swr_count_ids(swr_context* c, const swr_id_count* query, uint32_t* counts, int64_t n, uint32_t* none) {
    if (!c || !query) return SWR_ERR_BAD_ARG;
    const swr_id_count q = *query;
    if (const int f = sticky(c)) return f;
    int rc = check_count(c, q, counts, n);
    if (rc) return rc;
    if ((rc = fan(c, [=](swr_context* k) { return band_count_ids(k, q, n); }))) return rc;
    if (n) memset(counts, 0, (size_t)n * 4);
    uint32_t nn = 0;
    for (size_t b = 0; b < band_count(c); b++) {
        const uint32_t* part = band(c, b)->count_host.p;
        for (int64_t i = 0; i < n; i++) counts[i] += part[i];
        nn += part[n];
    }
    if (none) *none = nn;
    return SWR_OK;
}

int swr_query_depth(swr_context* c, const swr_depth_box* boxes, int64_t n, uint32_t* passed) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (const int f = sticky(c)) return f;
    int rc = check_query(c, boxes, n, passed);
    if (rc) return rc;
    if ((rc = fan(c, [=](swr_context* k) { return band_query_depth(k, boxes, n); }))) return rc;
    if (n) memset(passed, 0, (size_t)n * 4);
    for (size_t b = 0; b < band_count(c); b++)
        for (int64_t i = 0; i < n; i++) passed[i] += band(c, b)->query_passed[i];
    return SWR_OK;
}

int swr_item_bounds(swr_context* c, const swr_draw_item* items, int32_t item_count, uint32_t flags, swr_item_bound* out) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (const int f = sticky(c)) return f;
    int rc = check_bounds(c, items, item_count, flags, out);
    if (rc) return rc;
    // the result does not depend on rows and every band holds the whole scene: the first band answers for the full target, the
    // others finish what they have in flight
    swr_context* first = band(c, 0);
    if ((rc = fan(c, [=](swr_context* k) { return k == first ? band_item_bounds(k, items, item_count, flags) : single_sync(k); }))) return rc;
    if (item_count) memcpy(out, first->bounds_out, (size_t)item_count * sizeof(swr_item_bound));
    return SWR_OK;
}

int swr_cast_rays(swr_context* c, const swr_ray* rays, int64_t n, uint32_t flags, swr_ray_hit* hits) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (const int f = sticky(c)) return f;
    int rc = check_rays(c, "swr_cast_rays", rays, n, flags, hits);
    if (rc) return rc;
    // every band holds the whole scene: the first band answers, the others finish what they have in flight
    swr_context* first = band(c, 0);
    const swr_ray_query q = default_ray_query(first->ni / 3);
    if ((rc = fan(c, [=](swr_context* k) { return k == first ? band_cast_rays(k, q, rays, n) : single_sync(k); }))) return rc;
    if (n) memcpy(hits, first->rays_out, (size_t)n * sizeof(swr_ray_hit));
    return SWR_OK;
}

int swr_query_rays(swr_context* c, const swr_ray_query* query, const swr_ray* rays, int64_t n, swr_ray_hit* hits) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (const int f = sticky(c)) return f;
    int rc = check_rays(c, "swr_query_rays", rays, n, 0, hits);
    if (rc) return rc;
    swr_ray_query q;
    if ((rc = check_ray_query(c, query, q))) return rc;
    // as swr_cast_rays: the first band answers, the others finish what they have in flight
    swr_context* first = band(c, 0);
    if ((rc = fan(c, [=](swr_context* k) { return k == first ? band_cast_rays(k, q, rays, n) : single_sync(k); }))) return rc;
    if (n) memcpy(hits, first->rays_out, (size_t)n * sizeof(swr_ray_hit));
    return SWR_OK;
}

// one band's stats added to a total: sums, and the bounding box of the rectangles
static void delta_add(swr_delta_stats& t, const swr_delta_stats& k, bool first) {
    if (k.bytes_copied) {
        if (!t.bytes_copied) { t.x0 = k.x0; t.y0 = k.y0; t.x1 = k.x1; t.y1 = k.y1; }
        else { t.x0 = std::min(t.x0, k.x0); t.y0 = std::min(t.y0, k.y0); t.x1 = std::max(t.x1, k.x1); t.y1 = std::max(t.y1, k.y1); }
    }
    t.tiles += k.tiles; t.tiles_changed += k.tiles_changed; t.bytes_copied += k.bytes_copied;
    if (k.tiles) t.full = first ? k.full : (t.full & k.full);       // (the bands' baselines come and go together)
}

// swr_read_color_delta / swr_read_depth_delta and the gather of swr_render_delta; `out` (never NULL) is written after every band succeeded
static int read_delta(swr_context* c, int img, void* dst, swr_delta_stats* out) {
    if (const int f = sticky(c)) return f;
    int rc = check_delta(c, dst);
    if (rc) return rc;
    if ((rc = fan(c, [=](swr_context* k) { return band_read_delta(k, img, dst); }))) return rc;
    swr_delta_stats t{};
    bool first = true;
    for (size_t b = 0; b < band_count(c); b++) {
        const swr_delta_stats& part = band(c, b)->delta_stats;
        delta_add(t, part, first);
        if (part.tiles) first = false;
    }
    *out = t;
    return SWR_OK;
}

int swr_read_color_delta(swr_context* c, void* dst, swr_delta_stats* stats) {
    if (!c) return SWR_ERR_BAD_ARG;
    swr_delta_stats st;
    const int rc = read_delta(c, 0, dst, &st);
    if (!rc && stats) *stats = st;
    return rc;
}

int swr_read_depth_delta(swr_context* c, float* dst, swr_delta_stats* stats) {
    if (!c) return SWR_ERR_BAD_ARG;
    swr_delta_stats st;
    const int rc = read_delta(c, 1, dst, &st);
    if (!rc && stats) *stats = st;
    return rc;
}

int swr_delta_reset(swr_context* c, uint32_t images) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (const int f = sticky(c)) return f;
    if (!images || (images & ~(uint32_t)(SWR_DELTA_COLOR | SWR_DELTA_DEPTH)))
        return fail(c, SWR_ERR_BAD_ARG, "swr_delta_reset: images 0x%x is zero or holds unknown bits", images);
    auto reset = [=](swr_context* k) {
        if (const int f = sticky(k)) return f;
        if (images & SWR_DELTA_COLOR) k->delta_valid[0] = false;
        if (images & SWR_DELTA_DEPTH) k->delta_valid[1] = false;
        return (int)SWR_OK;
    };
    return fan(c, reset);
}

// the resolved read of one or both images (NULL: not wanted); every band writes its own rows of the caller's images: nothing to gather
static int read_resolved(swr_context* c, const swr_resolve* resolve, void* color_dst, float* depth_dst) {
    const swr_resolve rs = *resolve;
    if (const int f = sticky(c)) return f;
    const int rc = check_resolve(c, rs);
    if (rc) return rc;
    return fan(c, [=](swr_context* k) { return band_read_resolved(k, rs, color_dst, depth_dst); });
}

int swr_read_color_resolved(swr_context* c, const swr_resolve* resolve, void* dst) {
    if (!c || !resolve || !dst) return SWR_ERR_BAD_ARG;
    return read_resolved(c, resolve, dst, nullptr);
}

int swr_read_depth_resolved(swr_context* c, const swr_resolve* resolve, float* dst) {
    if (!c || !resolve || !dst) return SWR_ERR_BAD_ARG;
    return read_resolved(c, resolve, nullptr, dst);
}

// ---- page-locked host images ---------------------------------------------------------------------------------------
void* swr_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

void swr_host_free(void* p) {
    Pinned<void> owner;         // (freed as the owner goes)
    owner.p = p;
}

int swr_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return SWR_ERR_BAD_ARG;
    if (hipHostRegister(p, bytes, hipHostRegisterPortable) != hipSuccess) {
        (void)hipGetLastError();
        return fail(nullptr, SWR_ERR_HIP, "hipHostRegister(%p, %zu) failed", p, bytes);
    }
    return SWR_OK;
}

int swr_host_unregister(void* p) {
    if (!p) return SWR_ERR_BAD_ARG;
    if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return SWR_ERR_HIP; }
    return SWR_OK;
}

// ---- instrumentation -------------------------------------------------------------------------------------------------
int swr_timing_enable(swr_context* c, int enable) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (is_group(c)) return group_run(c, [=](swr_context* k) { return swr_timing_enable(k, enable); });
    int rc = swr_sync(c);
    if (rc) return rc;
    c->timing = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return SWR_OK;
}

int swr_timing_sample(swr_context* c, int every_nth) {
    if (!c || every_nth < 1) return SWR_ERR_BAD_ARG;
    if (is_group(c)) return group_run(c, [=](swr_context* k) { return swr_timing_sample(k, every_nth); });
    int rc = swr_sync(c);
    if (rc) return rc;
    c->timing_every = every_nth;
    return SWR_OK;
}

int swr_pipeline_enable(swr_context* c, int enable) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (is_group(c)) return group_run(c, [=](swr_context* k) { return swr_pipeline_enable(k, enable); });
    int rc = swr_sync(c);
    if (rc) return rc;
    c->bin_stream = (enable && c->bin_stream_own) ? c->bin_stream_own : c->stream;
    return SWR_OK;
}

// A group reports the slowest band per stage (the frame is done when the last band is) and the sums of the counts.
static void merge_timings(swr_timings* acc, const swr_timings& t, bool first) {
    if (first) { *acc = t; return; }
    acc->setup_bin_ms = std::max(acc->setup_bin_ms, t.setup_bin_ms);
    acc->scan_ms = std::max(acc->scan_ms, t.scan_ms);
    acc->scatter_ms = std::max(acc->scatter_ms, t.scatter_ms);
    acc->raster_ms = std::max(acc->raster_ms, t.raster_ms);
    acc->total_ms = std::max(acc->total_ms, t.total_ms);
    acc->tile_pairs += t.tile_pairs;
    acc->tiles += t.tiles;
}

int swr_timing_totals(swr_context* c, swr_timings* sum, int64_t* frames) {
    if (!c || !sum || !frames) return SWR_ERR_BAD_ARG;
    const int rc = swr_sync(c);
    if (rc) return rc;
    for (size_t b = 0; b < band_count(c); b++) {
        const swr_context* k = band(c, b);
        swr_timings t = k->last;
        t.setup_bin_ms = (float)k->sum_ms[0]; t.scan_ms = (float)k->sum_ms[1];
        t.scatter_ms = (float)k->sum_ms[2]; t.raster_ms = (float)k->sum_ms[3];
        t.total_ms = (float)k->sum_ms[4];
        merge_timings(sum, t, b == 0);
    }
    *frames = band(c, 0)->sum_frames;
    return SWR_OK;
}

int swr_timing_reset(swr_context* c) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (is_group(c)) return group_run(c, [](swr_context* k) { return swr_timing_reset(k); });
    int rc = swr_sync(c);
    if (rc) return rc;
    for (double& v : c->sum_ms) v = 0.0;
    c->sum_frames = 0;
    return SWR_OK;
}

int swr_get_timings(swr_context* c, swr_timings* out) {
    if (!c || !out) return SWR_ERR_BAD_ARG;
    const int rc = swr_sync(c);
    if (rc) return rc;
    for (size_t b = 0; b < band_count(c); b++) merge_timings(out, band(c, b)->last, b == 0);
    return SWR_OK;
}

// swr_render (resolve == NULL, delta false), swr_render_resolved and swr_render_delta (delta_stats: NULL or where the two stats go)
// share this body: only the target's size and the gather differ.
static int render_pass(swr_context* c, const swr_render_pass* p, const swr_resolve* resolve, bool delta = false, swr_delta_stats* delta_stats = nullptr) {
    if (p->primitive_type != SWR_PRIMITIVE_TRIANGLE && p->primitive_type != SWR_PRIMITIVE_LINE &&
        p->primitive_type != SWR_PRIMITIVE_VERTICES)
        return fail(c, SWR_ERR_UNSUPPORTED, "unknown primitive type %d", p->primitive_type);
    if (p->index_count >= 0 && p->index_count % (p->primitive_type == SWR_PRIMITIVE_LINE ? 2 : 3) != 0)   // Renderer.swift:209
        return fail(c, SWR_ERR_INDEX_COUNT, "index_count %lld is not a multiple of %d", (long long)p->index_count,
                    p->primitive_type == SWR_PRIMITIVE_LINE ? 2 : 3);
    if (!p->depth || (!(p->flags & SWR_FLAG_NO_COLOR) && !p->color))
        return fail(c, SWR_ERR_BAD_ARG, "swr_render: colour/depth image pointer is NULL");
    int rc;
    const int64_t S = resolve ? resolve->factor : 1;             // the frame is drawn at S * width x S * height
    if (resolve) {
        if ((rc = check_resolve_args(c, *resolve))) return rc;
        if (p->flags & SWR_FLAG_LOAD)
            return fail(c, SWR_ERR_UNSUPPORTED, "swr_render_resolved: SWR_FLAG_LOAD is not supported (the starting image would be at the wrong resolution)");
    }
    if (delta && (p->flags & SWR_FLAG_LOAD))
        return fail(c, SWR_ERR_UNSUPPORTED, "swr_render_delta: SWR_FLAG_LOAD is not supported (its starting image is uploaded whole anyway)");
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<float, std::milli>(b - a).count(); };
    const auto t0 = clk::now();
    // Scene identity: the caller's promise that the arrays hold what they held at the last call with this id — the
    // resident copy (and the triangle stream built from it) is then used as it is, like the reference's GpuRenderer
    // keeps its MTLBuffers across calls (GpuRenderer.swift:32-33,41-67) for the app's one mesh (App.swift:153-185).
    const bool cached = p->scene_id != 0 && p->scene_id == c->scene_id && p->vertex_count == c->scene_nv &&
                        p->index_count == c->scene_ni && (p->attributes != nullptr) == c->scene_attrs &&
                        (p->texture == nullptr ? c->scene_tex == nullptr
                                               : (c->scene_tex != nullptr && p->tex_width == c->scene_tw && p->tex_height == c->scene_th));
    c->rt = swr_render_times{};
    c->rt.scene_cached = cached ? 1 : 0;
    if (!cached) {
        c->scene_id = 0;
        // no identity = the scene lives for this frame only: uploaded in index order, built behind the copy
        const bool oneshot = p->scene_id == 0;
        if ((rc = fan(c, [=](swr_context* k) { return single_scene_upload(k, p->vertices, p->vertex_count, p->indices, p->index_count, oneshot); }))) return rc;
        if (p->attributes && (rc = swr_scene_attributes(c, p->attributes, p->vertex_count))) return rc;
        if (p->texture && (rc = swr_texture_upload(c, p->texture, p->tex_width, p->tex_height))) return rc;
        c->scene_id = p->scene_id; c->scene_nv = p->vertex_count; c->scene_ni = p->index_count;
        c->scene_attrs = p->attributes != nullptr;
        c->scene_tex = p->texture; c->scene_tw = p->tex_width; c->scene_th = p->tex_height;
        // the split inside the upload: HIP events of (the slowest band of) the upload itself
        float h2d = band(c, 0)->up_h2d_ms;
        for (size_t b = 1; b < band_count(c); b++) h2d = std::max(h2d, band(c, b)->up_h2d_ms);
        c->rt.h2d_ms = h2d;
        c->rt.stream_build_ms = ms(t0, clk::now()) - h2d;       // index check, sort, gather, attribute / texture passes, allocation
    }
    const auto t1 = clk::now();
    // the pass carries its own fragment stage: NULL material = the reference's passthrough
    if ((rc = swr_material_set(c, p->material))) return rc;
    if ((rc = swr_target_set(c, S * p->width, S * p->height, 0, S * p->height))) return rc;
    // a load frame: the caller's images are its starting image (inputs now, never cached)
    if ((p->flags & SWR_FLAG_LOAD) &&
        (rc = swr_target_write(c, (p->flags & SWR_FLAG_NO_COLOR) ? nullptr : p->color, p->depth))) return rc;
    const swr_context* kf = band(c, 0);
    const uint64_t frames0 = kf->frame_no;
    if ((rc = swr_draw_primitives(c, p->transform, p->flags, p->primitive_type))) return rc;
    if (resolve) {
        // the gather of a supersampled pass: the frame itself (an overflow is repaired), then both images resolved in one launch per
        // band and the small images copied
        if ((rc = swr_sync(c))) return rc;
        const auto t2 = clk::now();
        if ((rc = read_resolved(c, resolve, (p->flags & SWR_FLAG_NO_COLOR) ? nullptr : p->color, p->depth))) return rc;
        const auto t3 = clk::now();
        c->rt.draw_ms = ms(t1, t2);
        c->rt.frames = (int32_t)(kf->frame_no - frames0);
        c->rt.gather_ms = ms(t2, t3);
        c->rt.total_ms = ms(t0, t3);
        return SWR_OK;
    }
    if (delta) {
        // the gather of a delta pass: the frame itself (an overflow is repaired), then the changed part of each image
        if ((rc = swr_sync(c))) return rc;
        const auto t2 = clk::now();
        swr_delta_stats st[2] = {};
        if (!(p->flags & SWR_FLAG_NO_COLOR) && (rc = read_delta(c, 0, p->color, &st[0]))) return rc;
        if ((rc = read_delta(c, 1, p->depth, &st[1]))) return rc;
        const auto t3 = clk::now();
        if (delta_stats) { delta_stats[0] = st[0]; delta_stats[1] = st[1]; }
        c->rt.draw_ms = ms(t1, t2);
        c->rt.frames = (int32_t)(kf->frame_no - frames0);
        c->rt.gather_ms = ms(t2, t3);
        c->rt.total_ms = ms(t0, t3);
        return SWR_OK;
    }
    // colour and depth leave every device together (two copy streams each); synchronous on return like
    // scheduleAndWait (Metal+Extensions.swift:57-67)
    if ((rc = swr_present(c, (p->flags & SWR_FLAG_NO_COLOR) ? nullptr : p->color, p->depth))) return rc;
    if ((rc = swr_sync(c))) return rc;                           // (the frame itself; repairs an overflow before the copy is waited for)
    const auto t2 = clk::now();
    if ((rc = swr_present_wait(c))) return rc;
    const auto t3 = clk::now();
    c->rt.draw_ms = ms(t1, t2);
    c->rt.frames = (int32_t)(kf->frame_no - frames0);            // 1, or 2 when the bins had to grow and the frame was redrawn
    c->rt.gather_ms = ms(t2, t3);
    c->rt.total_ms = ms(t0, t3);
    return SWR_OK;
}

int swr_render(swr_context* c, const swr_render_pass* p) {
    if (!c || !p) return SWR_ERR_BAD_ARG;
    return render_pass(c, p, nullptr);
}

int swr_render_resolved(swr_context* c, const swr_render_pass* p, const swr_resolve* resolve) {
    if (!c || !p || !resolve) return SWR_ERR_BAD_ARG;
    return render_pass(c, p, resolve);
}

int swr_render_delta(swr_context* c, const swr_render_pass* p, swr_delta_stats stats[2]) {
    if (!c || !p) return SWR_ERR_BAD_ARG;
    return render_pass(c, p, nullptr, true, stats);
}

int swr_render_timings(swr_context* c, swr_render_times* out) {
    if (!c || !out) return SWR_ERR_BAD_ARG;
    *out = c->rt;
    return SWR_OK;
}

int swr_debug_set(swr_context* c, int key, int64_t value) {
    if (!c) return SWR_ERR_BAD_ARG;
    if (is_group(c)) {
        int rc = SWR_OK;
        for (swr_context* k : c->kids) { const int r = swr_debug_set(k, key, value); if (r && !rc) { rc = r; c->err = k->err; } }
        return rc;
    }
    switch (key) {
        case SWR_DEBUG_STREAM_ORDER:
            if (value < -1 || value > 1) break;
            c->dbg_stream_order = (int)value; return SWR_OK;
        case SWR_DEBUG_CULL:
            if (value < 0 || value > 1) break;
            c->dbg_cull = (int)value; return SWR_OK;
        case SWR_DEBUG_BIN_MODE: {
            if (value < 0 || value > 3) break;
            c->dbg_bin_mode = (int)value;
            // the layout of the bins follows the mode: size them again for what is resident (streams idle first)
            if (c->has_scene && c->has_target) {
                int rc = swr_sync(c);
                if (rc) return rc;
                c->fixed_allowed = true; c->fixed_mode = false;
                return size_bins(c);
            }
            return SWR_OK;
        }
        case SWR_DEBUG_ONESHOT_MIN_TRIS:
            if (value < 0) break;
            c->dbg_oneshot_min_tris = std::max<int64_t>(64, value); return SWR_OK;
        case SWR_DEBUG_DEPTH_KEYS32:
            if (value < 0 || value > 1) break;
            c->dbg_k32 = value != 0; return SWR_OK;
        case SWR_DEBUG_RASTER_SORT:
            if (value < 0 || value > 2) break;
            c->dbg_insort = (int)value; return SWR_OK;
        default:
            return fail(c, SWR_ERR_BAD_ARG, "swr_debug_set: unknown key %d", key);
    }
    return fail(c, SWR_ERR_BAD_ARG, "swr_debug_set: value %lld out of range for key %d", (long long)value, key);
}

int swr_debug_fault(swr_context* c, int fault) {
    if (!c || fault < SWR_FAULT_NONE || fault > SWR_FAULT_ENQUEUE) return SWR_ERR_BAD_ARG;
    if (is_group(c)) { for (swr_context* k : c->kids) k->inject.store(fault); return SWR_OK; }
    c->inject.store(fault);
    return SWR_OK;
}

}  // extern "C"
