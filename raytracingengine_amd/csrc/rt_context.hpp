// rt_context.hpp — the C-ABI objects (rt_context, rt_scene) and the helpers the C-ABI
// translation units share (rt_capi.cpp: single device; rt_capi_queries.cpp: the batch queries;
// rt_multi.cpp: RCCL multi-GPU frames).
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <string>
#include <utility>
#include <vector>

#include "rt_capi.h"
#include "rt_internal.hpp"
#include "rt_row_plan.hpp"

namespace rtamd {

// Sets the calling thread's rt_last_error() message and returns st.
rt_status fail(rt_status st, const std::string& msg);
rt_status hip_fail(hipError_t e, const char* what);

#define RT_HIP(call)                                    \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return rtamd::hip_fail(e_, #call); \
    } while (0)

// Returns a failed rt_status of `call` to the caller (its message is already set).
#define RT_TRY(call)                    \
    do {                                \
        rt_status s_ = (call);          \
        if (s_ != RT_OK) return s_;     \
    } while (0)

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&ptr, need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
};

// Restores the caller's current device on scope exit.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace rtamd

struct rt_comm;

struct rt_context {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    size_t lds_limit = 0;
    rtamd::DeviceBuffer out64, out32, ldr, tm_in, tm_out, dbg, rays;
    rtamd::DeviceBuffer counters;  // 2 x u64
    rtamd::DeviceBuffer wf, wf_ctl;  // breadth-first TraceRay arena + its control block
    // The arena and the counters are one per context: a render that uses them waits for the
    // previous one that did, on whatever stream it ran (scratch_wait / scratch_done).
    hipEvent_t scratch_event = nullptr;
    bool scratch_used = false;
    hipStream_t scratch_stream = nullptr;  // the stream of the latest scratch user
    // the packet kernel's fix-up list (TraceParams.fix_list) and its control words, one per
    // context like the counters (ordered across streams by scratch_wait / scratch_done)
    rtamd::DeviceBuffer fix_list, fix_ctl;
    int fix_parity = 0;  // which of the two counts of fix_ctl the next fix-variant launch uses
    // the adaptive frames' list of unfinished pixels (AdaptiveArgs.list) and its count, scratch
    // of the context like the fix-up list; adapt_listing: the latest adaptive call used them
    rtamd::DeviceBuffer adapt_list, adapt_ctl;
    bool adapt_listing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events;
    double timed_ms = 0.0;
    uint64_t launches = 0;
    // packet-kernel frames enqueued {with, without} each thing the rt_debug_* entry of the same
    // name reports (rt_capi.cpp count_packet_frames)
    enum PkCounter {
        kCntConeTable,     // a camera-cone table
        kCntShadowTable,   // a shadow-cull table
        kCntTileClass,     // tile class words
        kCntPlaneClear,    // class words that carry shadow-plane keep masks
        kCntTileSplit,     // fix-up variant frames: the split launch / its single launch
        kCntTileShadowed,  // ... with / without a launch over a list of shadowed-plane tiles
        kPkCounters
    };
    uint64_t pk_frames[kPkCounters][2] = {};
    // rt_render_multi: RCCL communicators over the devices of the last context list this
    // context led (rt_multi.cpp); destroyed with the context
    std::vector<rt_context*> group_ctxs;
    std::vector<rt_comm*> group_comms;
    // the contexts whose cached group includes this one (released when this one is destroyed)
    std::vector<rt_context*> group_roots;
};

struct rt_scene {
    rt_context* ctx = nullptr;
    rtamd::DeviceBuffer buf;
    int32_t ns = 0, np = 0, nt = 0, nl = 0;
    size_t off_sph = 0, off_sph_mat = 0, off_pl = 0, off_pl_mat = 0, off_tri = 0, off_tri_mat = 0,
           off_lt = 0;
    bool any_transparent = false;
    double max_specular = 0.0;  // NaN-aware: stored as +inf when a NaN specular exists
    bool has_area = false;
    rt_area_light area{};
    size_t off_bvh = 0, off_bvh_tri = 0;  // triangle BVH, when bvh_nodes > 0
    int32_t bvh_nodes = 0;
    size_t off_sperm = 0, off_sbnd = 0;   // sphere chunks, when ns >= kSphChunkMin
    size_t off_box = 0;                   // planes-only chain table (rt_box.hip), when np > 0
    int32_t box_n[4] = {0, 0, 0, 0};
    // Packet-kernel LDS images, one per camera position this scene was rendered from more than
    // once (the image depends on the spheres, planes, point lights and camera position only).  An
    // entry is written once, by packet_image_kernel on the stream of the render that created
    // it; renders on other streams wait for its event until it has completed.  Never rewritten
    // or freed before the scene, so a launch in flight never sees it change.
    struct PkImage {
        double cam[3];
        rtamd::DeviceBuffer buf;
        hipEvent_t ready = nullptr;
        hipStream_t stream = nullptr;
        bool done = false;
        // Costliest-first tile order of the packet kernel for this camera (rt_packet_host.cpp
        // tile_order): the wave durations one launch records, then the order built from them,
        // for launches of the same shape (grid, rows) — state 1 recorded, 2 ordered.  One entry
        // per launch shape (up to kMaxTileOrders), each written once and never rewritten, so a
        // launch of one shape in flight on any stream never sees another shape's table.
        struct TileOrder {
            uint32_t key[8] = {};  // gx gy waves width height rows row0 row_block|row_stride
            int state = 0;
            rtamd::DeviceBuffer cost, keys, order;
            hipEvent_t recorded = nullptr, built = nullptr;
            // pinned host word the order kernel fills: 0 not yet, 1 narrow (keep the default
            // order, no table), 2 dispatch by the table
            uint32_t* verdict = nullptr;
        };
        std::vector<TileOrder> ords;
        int last_ord = -1;  // the entry of the latest launch (rt_debug_tile_order)
        // Camera-cone mask tables of this camera (rt_cone_table.hpp), one per launch shape and
        // camera-ray constants (cone_table_key: the focal length is the render call's; up to
        // kMaxConeTabs, later shapes or focal lengths go without): written once by
        // packet_cone_table_kernel on the stream of the render that created it, never rewritten;
        // renders on other streams wait for `ready` until it has completed.  Dropped with the
        // image entry.  The buffer also holds the shadow-cull words formed from the cone masks
        // (rt_shadow_table.hpp) and whatever else the key's contents word names: the layout is
        // rt_tile_table.hpp's.
        struct ConeTab {
            static constexpr size_t kKeyWords = 20;
            uint32_t key[kKeyWords] = {};
            rtamd::DeviceBuffer buf;
            hipEvent_t ready = nullptr;
            hipStream_t stream = nullptr;
            bool done = false;
            // with tile lists (the key says so): two pinned host words the launch that forms the
            // table fills with the lists' counts (tile_list_counts_encode; 0: not formed yet)
            unsigned long long* counts = nullptr;
        };
        std::vector<ConeTab> tabs;
    };
    mutable std::vector<PkImage> pk_images;
    mutable std::vector<std::array<double, 3>> pk_seen;  // cameras rendered once, no image yet
    // Cameras without an image: a ring of kPkPubSlots publish slots (rt_packet_host.cpp, in-launch
    // image hand-off), each launch tagged with its own epoch; zeroed once at allocation.
    mutable rtamd::DeviceBuffer pk_pub;
    // Frame batches with cameras that have no cached image (a moving camera): one small launch
    // forms every frame's image into a ring entry of kPkBatchRing × kPkMaxBatch images before
    // the batch launch, which copies them like cached ones; an entry is reused only after the
    // batch that read it (its event) has completed.
    static constexpr int kPkBatchRing = 4;
    mutable rtamd::DeviceBuffer pk_batch;
    mutable hipEvent_t pk_batch_done[kPkBatchRing] = {nullptr, nullptr, nullptr, nullptr};
    mutable bool pk_batch_used[kPkBatchRing] = {false, false, false, false};
    mutable int pk_batch_next = 0;
    // ... and the cone tables of those frames, one buffer per ring entry (the table's size is
    // the launch shape's, so an entry grows on demand, after the batch that last read it)
    mutable rtamd::DeviceBuffer pk_batch_tab[kPkBatchRing];
};

namespace rtamd {

// The three frame outputs, in the order of every {hdr64, hdr32, ldr} pointer triple: the RT_OUT_*
// bit, the bytes of a pixel and the context buffer a host framebuffer is staged in.
struct FrameOutput {
    int bit;
    size_t px_bytes;
    DeviceBuffer rt_context::*buf;
};
constexpr FrameOutput kFrameOutputs[3] = {{RT_OUT_HDR64, 3 * sizeof(double), &rt_context::out64},
                                          {RT_OUT_HDR32, 3 * sizeof(float), &rt_context::out32},
                                          {RT_OUT_LDR, 3, &rt_context::ldr}};

// Host framebuffers of npx pixels through those buffers: grow() the requested ones (host pointer
// not NULL), hand their device pointers to the render, download() enqueues the copies back on
// ctx->stream.  The caller holds a DeviceGuard and synchronizes.
struct FrameStage {
    rt_context* ctx;
    void* host[3];
    size_t npx;
    FrameStage(rt_context* c, void* h64, void* h32, void* hldr, size_t n)
        : ctx(c), host{h64, h32, hldr}, npx(n) {}
    rt_status grow() const {
        for (int k = 0; k < 3; ++k)
            if (host[k]) RT_HIP((ctx->*kFrameOutputs[k].buf).ensure(npx * kFrameOutputs[k].px_bytes));
        return RT_OK;
    }
    void* dev(int k) const { return host[k] ? (ctx->*kFrameOutputs[k].buf).ptr : nullptr; }
    double* d64() const { return static_cast<double*>(dev(0)); }
    float* d32() const { return static_cast<float*>(dev(1)); }
    uint8_t* dldr() const { return static_cast<uint8_t*>(dev(2)); }
    rt_status download() const {
        for (int k = 0; k < 3; ++k)
            if (host[k])
                RT_HIP(hipMemcpyAsync(host[k], dev(k), npx * kFrameOutputs[k].px_bytes,
                                      hipMemcpyDeviceToHost, ctx->stream));
        return RT_OK;
    }
};

// *opts, or the defaults for NULL.
inline rt_render_opts resolved(const rt_render_opts* opts) {
    rt_render_opts o;
    if (opts) o = *opts;
    else rt_render_opts_default(&o);
    return o;
}

rt_status validate_camera(const rt_camera* cam);
// The row set of o against a camera's height.  suffix: empty, or " passed to NAME" for the
// entries whose messages end in their name.
rt_status check_row_set(const rt_render_opts& o, uint32_t height, const std::string& suffix);
// The row set of o (checked) as the kernels read it: p.row0 / row_block / row_stride / rows.
void set_row_set(const rt_render_opts& o, uint32_t height, TraceParams& p);
// Enqueues one render (plus the counting pass with RT_FLAG_COUNT_RAYS) on ctx's stream into
// device outputs in the packed row order of opts.  The caller holds a DeviceGuard.
rt_status enqueue_render(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                         const rt_render_opts* opts, double* d64, float* d32, uint8_t* dldr);
// The same for a batch of nframes cameras (same width / height / focal / aa_samples): frame f
// writes its rows f·stride·width pixels into each output, stride = frame_rows (0: the rows the
// render produces; larger pads every frame, as the row-split gather's send buffers are laid out).
// Packet-kernel scenes render up to kPkMaxBatch frames per launch (blockIdx.z = frame), other
// scenes one launch per frame.
rt_status enqueue_frames(rt_context* ctx, const rt_scene* sc, const rt_camera* cams, int nframes,
                         const rt_render_opts* opts, double* d64, float* d32, uint8_t* dldr,
                         uint32_t frame_rows = 0);
rt_status check_batch(const rt_camera* cams, int nframes);
// The launch parameters of a render or a query (rt_capi_queries.cpp) of `sc` from `cam` with opts
// (NULL: the defaults), after checking all three: p, the TraceRay shape the scene can produce
// (path: kPathDirect / kPathChain / kPathTree), whether the scene's records fit the context's LDS
// budget and their bytes, and the rows the row set of opts selects.
rt_status build_params(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                       const rt_render_opts* opts_in, TraceParams& p, int& path, bool& lds,
                       size_t& lds_bytes, uint32_t& rows);
// rt_packet_host.cpp, for enqueue_frames before a packet launch.  One frame: p.pk_image from the
// scene's cache of camera images, a setup launch on a camera's second sighting, or a publish
// slot (p.pk_pub); a batch: p.fr[f] for every frame and *batch_ring = the ring entry its formed
// images took, or -1.  Both set p.tile_order / p.tile_cost and *rec, the tile-order entry whose
// recording launch the caller marks complete.  *split: the batch's split launch (tiles == 0: none).
rt_status packet_image(rt_context* ctx, const rt_scene* sc, TraceParams& p, int flags,
                       rt_scene::PkImage::TileOrder** rec);
rt_status packet_batch_images(rt_context* ctx, const rt_scene* sc, const rt_camera* cams,
                              int nframes, TraceParams& p, int flags,
                              rt_scene::PkImage::TileOrder** rec, int* batch_ring,
                              PkSplit* split);
// The breadth-first TraceRay arena, the ray counters and the fix-up list are one per context:
// renders that use them are ordered across streams.  scratch_wait orders work on ctx->stream
// after the last such render (any stream), scratch_done marks ctx->stream's work so far as the
// latest such user.
rt_status scratch_wait(rt_context* ctx);
rt_status scratch_done(rt_context* ctx);
// The list of an adaptive call over px pixels (rt_capi_queries.cpp): grows ctx->adapt_list as
// fixup_buffers grows its list and zeroes the count on ctx->stream.  The caller has made
// scratch_wait and makes scratch_done after its launches.
rt_status adaptive_buffers(rt_context* ctx, size_t px, AdaptiveArgs& a);
// The two ray counters [trace, shadow]: zeroed on ctx->stream; read into c, either enqueued on
// ctx->stream (c is valid once the stream has been synchronized) or with a blocking copy.
rt_status counters_zero(rt_context* ctx);
rt_status counters_read(rt_context* ctx, unsigned long long c[2], bool on_stream);
// RT_FLAG_TIME_KERNEL (flags without it: nothing happens): timing_begin takes an event pair (a
// recycled one, or a new one) and records its first event on ctx->stream, timing_end records the
// second and queues the pair; harvest_events adds the elapsed time of the completed pairs (all:
// waits for every one) to the context totals and recycles them.
using EventPair = std::pair<hipEvent_t, hipEvent_t>;
rt_status timing_begin(rt_context* ctx, int flags, EventPair& ev);
rt_status timing_end(rt_context* ctx, int flags, const EventPair& ev);
rt_status harvest_events(rt_context* ctx, bool all);
// rt_multi.cpp: releases the communicators rt_render_multi cached in ctx.
void release_group(rt_context* ctx);
// rt_multi.cpp: releases ctx's own group and every group that includes ctx (context teardown).
void leave_groups(rt_context* ctx);

}  // namespace rtamd
