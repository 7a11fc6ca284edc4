// rt_capi.cpp — implementation of include/rt_capi.h on HIP (gfx950): contexts, scenes, render,
// G-buffer, statistics and the rt_debug_* entries (the batch queries: rt_capi_queries.cpp).
//
// The context owns a device, a stream and growable device staging buffers; a scene is one
// HBM allocation of packed records (rt_internal.hpp).  No exception crosses the C boundary.
#include "rt_capi.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "rt_context.hpp"
#include "rt_internal.hpp"
#include "rt_wavefront.hpp"

#pragma clang fp contract(off)

using namespace rtamd;

namespace rtamd {

thread_local std::string g_last_error;

rt_status fail(rt_status st, const std::string& msg) {
    g_last_error = msg;
    return st;
}

rt_status hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP,
                std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace rtamd

namespace rtamd {

void pack_material(const rt_material& m, double* o) {
    o[0] = m.color[0];
    o[1] = m.color[1];
    o[2] = m.color[2];
    o[3] = m.shininess;
    o[4] = m.specular;
    o[5] = m.transparency;
    o[6] = m.refractive_index;
    o[7] = 0.0;
}

// Vec3::normalize (Math.h:31-37) on the host (used for the triangle normal, Shape.h:222-227).
void normalize3(const double* a, double* o) {
    const double len = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (len <= 1e-12) {
        o[0] = o[1] = o[2] = 0.0;
        return;
    }
    o[0] = a[0] / len;
    o[1] = a[1] / len;
    o[2] = a[2] / len;
}

rt_status harvest_events(rt_context* ctx, bool all) {
    size_t keep_from = 0;
    for (size_t i = 0; i < ctx->pending.size(); ++i) {
        auto& ev = ctx->pending[i];
        if (!all && hipEventQuery(ev.second) != hipSuccess) {
            keep_from = i;
            break;
        }
        RT_HIP(hipEventSynchronize(ev.second));
        float ms = 0.f;
        RT_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
        ctx->timed_ms += ms;
        ctx->launches += 1;
        ctx->free_events.push_back(ev);
        keep_from = i + 1;
    }
    ctx->pending.erase(ctx->pending.begin(), ctx->pending.begin() + keep_from);
    return RT_OK;
}

rt_status timing_begin(rt_context* ctx, int flags, EventPair& ev) {
    if (!(flags & RT_FLAG_TIME_KERNEL)) return RT_OK;
    if (ctx->pending.size() >= 1024) RT_TRY(harvest_events(ctx, false));
    if (!ctx->free_events.empty()) {
        ev = ctx->free_events.back();
        ctx->free_events.pop_back();
    } else {
        RT_HIP(hipEventCreate(&ev.first));
        RT_HIP(hipEventCreate(&ev.second));
    }
    RT_HIP(hipEventRecord(ev.first, ctx->stream));
    return RT_OK;
}

rt_status timing_end(rt_context* ctx, int flags, const EventPair& ev) {
    if (!(flags & RT_FLAG_TIME_KERNEL)) return RT_OK;
    RT_HIP(hipEventRecord(ev.second, ctx->stream));
    ctx->pending.push_back(ev);
    return RT_OK;
}

rt_status counters_zero(rt_context* ctx) {
    RT_HIP(hipMemsetAsync(ctx->counters.ptr, 0, 2 * sizeof(unsigned long long), ctx->stream));
    return RT_OK;
}

rt_status counters_read(rt_context* ctx, unsigned long long c[2], bool on_stream) {
    const size_t bytes = 2 * sizeof(unsigned long long);
    if (on_stream)
        RT_HIP(hipMemcpyAsync(c, ctx->counters.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    else
        RT_HIP(hipMemcpy(c, ctx->counters.ptr, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status check_row_set(const rt_render_opts& o, uint32_t height, const std::string& suffix) {
    const uint32_t r1 = o.row_end ? o.row_end : height;
    if (r1 > height || o.row_begin >= r1)
        return fail(RT_ERR_INVALID_ARG, "row range [" + std::to_string(o.row_begin) + "," +
                                            std::to_string(r1) + ") invalid for height " +
                                            std::to_string(height) + suffix);
    if (o.row_cycle > 1 && o.row_block == 0)
        return fail(RT_ERR_INVALID_ARG, suffix.empty() ? "row_cycle > 1 needs row_block >= 1"
                                                       : "row_cycle > 1 without row_block >= 1" + suffix);
    return RT_OK;
}

void set_row_set(const rt_render_opts& o, uint32_t height, TraceParams& p) {
    p.row0 = o.row_begin;
    if (o.row_cycle > 1) {
        p.row_block = o.row_block;
        p.row_stride = static_cast<uint32_t>(o.row_block) * o.row_cycle;
    }
    p.rows = rendered_rows(o, height);
}

rt_status validate_camera(const rt_camera* cam) {
    if (!cam) return fail(RT_ERR_INVALID_ARG, "camera is NULL");
    if (cam->width == 0 || cam->height == 0)
        return fail(RT_ERR_INVALID_ARG, "camera width/height must be > 0");
    if (cam->aa_samples < 0) return fail(RT_ERR_INVALID_ARG, "aa_samples must be >= 0");
    if (static_cast<uint64_t>(cam->width) * cam->height > (1ull << 31))
        return fail(RT_ERR_UNSUPPORTED, "image larger than 2^31 pixels");
    return RT_OK;
}

rt_status build_params(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                       const rt_render_opts* opts_in, TraceParams& p, int& path, bool& lds,
                       size_t& lds_bytes, uint32_t& rows) {
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "context is NULL");
    if (!sc) return fail(RT_ERR_INVALID_ARG, "scene is NULL");
    if (sc->ctx != ctx) return fail(RT_ERR_INVALID_ARG, "scene belongs to another context");
    RT_TRY(validate_camera(cam));
    const rt_render_opts opts = resolved(opts_in);
    RT_TRY(check_row_set(opts, cam->height, ""));
    if (opts.tonemap < RT_TONEMAP_NONE || opts.tonemap >= RT_TONEMAP_COUNT)
        return fail(RT_ERR_INVALID_ARG, "tonemap operator out of range");

    const double* base = static_cast<const double*>(sc->buf.ptr);
    std::memset(&p, 0, sizeof p);
    p.sph = base + sc->off_sph;
    p.sph_mat = base + sc->off_sph_mat;
    p.pl = base + sc->off_pl;
    p.pl_mat = base + sc->off_pl_mat;
    p.tri = base + sc->off_tri;
    p.tri_mat = base + sc->off_tri_mat;
    if (sc->bvh_nodes > 0 && !(opts.flags & RT_FLAG_NO_BVH)) {
        p.bvh = base + sc->off_bvh;
        p.bvh_tri = reinterpret_cast<const int32_t*>(base + sc->off_bvh_tri);
    }
    p.lt = base + sc->off_lt;
    if (sc->np > 0) {
        p.box = base + sc->off_box;
        for (int k = 0; k < 4; ++k) p.box_n[k] = sc->box_n[k];
    }
    if (sc->ns >= kSphChunkMin) {
        p.sph_bnd = base + sc->off_sbnd;
        p.sph_perm = reinterpret_cast<const int32_t*>(base + sc->off_sperm);
    }
    p.ns = sc->ns;
    p.np = sc->np;
    p.nt = sc->nt;
    p.nl = sc->nl;
    if (sc->has_area && sc->area.samples > 0) {
        const rt_area_light& a = sc->area;  // samples = k * k (rt_scene_set_area_light)
        const int k = static_cast<int>(std::lround(std::sqrt(static_cast<double>(a.samples))));
        const double li = a.intensity / static_cast<double>(a.samples);
        for (int i = 0; i < 3; ++i) {
            p.al_corner[i] = a.corner[i];
            p.al_u[i] = a.edge_u[i];
            p.al_v[i] = a.edge_v[i];
            p.al_E[i] = a.color[i] * li;
        }
        p.al_samples = a.samples;
        p.al_k = k;
    }
    for (int i = 0; i < 3; ++i) p.cam_pos[i] = cam->position[i];
    p.focal = cam->focal;
    p.width = cam->width;
    p.height = cam->height;
    const CameraConsts cc = camera_consts(cam->width, cam->height, cam->position[2], cam->focal);
    p.half_w = cc.half_w;
    p.half_h = cc.half_h;
    p.cam_dz = cc.dz;
    p.cam_dz2 = cc.dz2;
    p.aa = cam->aa_samples;
    p.max_rec = opts.max_recursion;
    p.bias = opts.bias;
    p.seed = opts.seed;
    set_row_set(opts, cam->height, p);
    rows = p.rows;
    p.tonemap = opts.tonemap;

    // Which TraceRay shape can this scene produce?  (Scene.h:175-195)
    if (sc->any_transparent) path = kPathTree;
    else if (!(sc->max_specular <= opts.bias) && opts.max_recursion >= 1) path = kPathChain;
    else path = kPathDirect;
    if (path != kPathDirect && opts.max_recursion > kMaxDepth)
        return fail(RT_ERR_UNSUPPORTED, "max_recursion > " + std::to_string(kMaxDepth) +
                                            " with reflective/transparent materials");
    lds_bytes = sizeof(double) * (static_cast<size_t>(kSphStride) * sc->ns +
                                  static_cast<size_t>(kPlStride) * sc->np +
                                  static_cast<size_t>(kLtStride) * sc->nl);
    lds = lds_bytes <= ctx->lds_limit;
    return RT_OK;
}

rt_status scratch_wait(rt_context* ctx) {
    // the latest user on this same stream is ordered before us already
    if (ctx->scratch_used && ctx->scratch_stream != ctx->stream)
        RT_HIP(hipStreamWaitEvent(ctx->stream, ctx->scratch_event, 0));
    return RT_OK;
}

rt_status scratch_done(rt_context* ctx) {
    RT_HIP(hipEventRecord(ctx->scratch_event, ctx->stream));
    ctx->scratch_used = true;
    ctx->scratch_stream = ctx->stream;
    return RT_OK;
}

// The packet kernel's fix-up buffers for a launch of `px` output pixels (rt_internal.hpp
// TraceParams.fix_list): the list grows on demand; the two counts are zeroed once, then each
// fix-up launch zeroes the one the next launch uses (ctx->fix_parity alternates).
rt_status fixup_buffers(rt_context* ctx, size_t px, TraceParams& p) {
    if (px >= (size_t(1) << 32)) return fail(RT_ERR_UNSUPPORTED, "fix-up list above 2^32 pixels");
    if (!ctx->fix_ctl.ptr) {
        RT_HIP(ctx->fix_ctl.ensure(2 * sizeof(uint32_t)));
        RT_HIP(hipMemsetAsync(ctx->fix_ctl.ptr, 0, 2 * sizeof(uint32_t), ctx->stream));
    }
    if (ctx->fix_list.bytes < px * sizeof(uint32_t)) {
        // the list may still be read by a fix-up launch on any stream the context used; every
        // user of the list is a scratch user, so the context's last scratch event covers them
        // all (not hipDeviceSynchronize: it would also wait on an RCCL gather of a dead peer
        // and on other contexts' work)
        if (ctx->scratch_used) RT_HIP(hipEventSynchronize(ctx->scratch_event));
        RT_HIP(ctx->fix_list.ensure(px * sizeof(uint32_t)));
    }
    p.fix_list = static_cast<uint32_t*>(ctx->fix_list.ptr);
    p.fix_ctl = static_cast<uint32_t*>(ctx->fix_ctl.ptr) + ctx->fix_parity;
    p.fix_next = static_cast<uint32_t*>(ctx->fix_ctl.ptr) + (1 - ctx->fix_parity);
    return RT_OK;
}

rt_status adaptive_buffers(rt_context* ctx, size_t px, AdaptiveArgs& a) {
    if (px >= (size_t(1) << 32)) return fail(RT_ERR_UNSUPPORTED, "adaptive list above 2^32 pixels");
    RT_HIP(ctx->adapt_ctl.ensure(sizeof(uint32_t)));
    if (ctx->adapt_list.bytes < px * sizeof(uint32_t)) {
        // as fixup_buffers: the list's users are scratch users, the last scratch event covers them
        if (ctx->scratch_used) RT_HIP(hipEventSynchronize(ctx->scratch_event));
        RT_HIP(ctx->adapt_list.ensure(px * sizeof(uint32_t)));
    }
    RT_HIP(hipMemsetAsync(ctx->adapt_ctl.ptr, 0, sizeof(uint32_t), ctx->stream));
    a.list = static_cast<uint32_t*>(ctx->adapt_list.ptr);
    a.list_count = static_cast<uint32_t*>(ctx->adapt_ctl.ptr);
    return RT_OK;
}

rt_status check_batch(const rt_camera* cams, int nframes) {
    if (!cams || nframes < 1) return fail(RT_ERR_INVALID_ARG, "frame batch: no cameras");
    for (int f = 0; f < nframes; ++f) {
        RT_TRY(validate_camera(cams + f));
        if (cams[f].width != cams[0].width || cams[f].height != cams[0].height ||
            cams[f].aa_samples != cams[0].aa_samples ||
            std::memcmp(&cams[f].focal, &cams[0].focal, sizeof(double)) != 0)
            return fail(RT_ERR_INVALID_ARG, "frame batch: every camera must have the first's "
                                            "width, height, focal and aa_samples");
    }
    return RT_OK;
}

rt_status enqueue_render(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                         const rt_render_opts* opts, double* d64, float* d32, uint8_t* dldr) {
    return enqueue_frames(ctx, sc, cam, 1, opts, d64, d32, dldr);
}

// The rt_debug_* frame counters of one packet launch: what each of its frames was handed (its
// table pointers; one frame: the launch's own) and, for the fix-up variant, how it is launched.
static void count_packet_frames(rt_context* ctx, const TraceParams& p, int nframes, bool fixup,
                                const PkSplit& split) {
    auto count = [&](rt_context::PkCounter c, bool with, uint64_t n) {
        ctx->pk_frames[c][with ? 0 : 1] += n;
    };
    for (int f = 0; f < nframes; ++f) {
        const bool cone = (nframes > 1 ? p.fr_tab[f] : p.cone_tab) != nullptr;
        const bool shadow = (nframes > 1 ? p.fr_stab[f] : p.shadow_tab) != nullptr;
        const bool cls = (nframes > 1 ? p.fr_ctab[f] : p.class_tab) != nullptr;
        count(rt_context::kCntConeTable, cone, 1);
        count(rt_context::kCntShadowTable, shadow, 1);
        count(rt_context::kCntTileClass, cls, 1);
        count(rt_context::kCntPlaneClear, cls && p.plane_masks, 1);
    }
    if (!fixup) return;
    count(rt_context::kCntTileSplit, split.tiles != 0, static_cast<uint64_t>(nframes));
    count(rt_context::kCntTileShadowed, split.tiles && split.sh_n, static_cast<uint64_t>(nframes));
}

// Which kernel serves a frame (or frame batch) of a scene, decided once per enqueue_frames call,
// and what its launch needs beside the TraceParams.
struct FrameRoute {
    // kPacket: scenes without secondary rays whose LDS image fits (rt_packet.hip).  kBox:
    // reflection chains of scenes made of planes and up to kBoxMaxSpheres spheres, the
    // scalar-cache chain kernel (rt_box.hip).  kLeanGeneric: the generic kernels without triangle
    // / area-light code, for scenes that use neither.  kGeneric: everything else.
    enum Kernel { kPacket, kBox, kLeanGeneric, kGeneric } kernel;
    bool sample_parallel;
    // the breadth-first TraceRay serves the image launch when its roots fit the arena
    // (enqueue_wavefront): refraction trees, and reflection chains under RTAMD_WF_CHAIN=1
    bool arena;
    // kPacket: the fix-up variant (undecided shadow rays re-rendered per pixel after the launch).
    // Known once the frames' images are placed: packet_uses_fixup reads p.tile_cost / p.nframes.
    bool fixup = false;
    int path;
    bool lds;
    size_t lds_bytes;
    bool any_specular;
};

static FrameRoute choose_route(const TraceParams& p, int path, int flags, const rt_scene* sc,
                               const rt_context* ctx, bool lds, size_t lds_bytes) {
    FrameRoute r;
    r.path = path;
    r.lds = lds;
    r.lds_bytes = lds_bytes;
    r.any_specular = sc->max_specular > 0.0;
    r.sample_parallel = !(flags & RT_FLAG_NO_SAMPLE_PARALLEL);
    const bool specialised = !(flags & RT_FLAG_GENERIC_KERNEL);
    const char* wf_chain = std::getenv("RTAMD_WF_CHAIN");
    r.arena = specialised && (path == kPathTree ||
                              (path == kPathChain && wf_chain && std::atoi(wf_chain) == 1));
    // RTAMD_BOX_SPH=0 keeps scenes with spheres on the generic chain kernel (A/B runs)
    static const bool box_sph = [] {
        const char* e = std::getenv("RTAMD_BOX_SPH");
        return !(e && std::atoi(e) == 0);
    }();
    const bool lean = p.nt == 0 && p.al_samples == 0;
    if (specialised && path == kPathDirect && p.ns <= packet_max_spheres() &&
        packet_lds_bytes(p.ns, p.np, p.nl) <= ctx->lds_limit)
        r.kernel = FrameRoute::kPacket;
    else if (specialised && path == kPathChain && lean &&
             (p.ns == 0 ? p.np > 0 : (box_sph && p.ns <= kBoxMaxSpheres)))
        r.kernel = FrameRoute::kBox;
    else
        r.kernel = lean ? FrameRoute::kLeanGeneric : FrameRoute::kGeneric;
    return r;
}

// The image launch (split: the packet batch's tile lists) or the counting launch of a route.
static hipError_t launch(const FrameRoute& r, const TraceParams& q, bool count, hipStream_t stream,
                         const PkSplit* split) {
    switch (r.kernel) {
    case FrameRoute::kPacket:
        return launch_packet_direct(q, count, r.any_specular, stream, count ? nullptr : split);
    case FrameRoute::kBox: return launch_box_chain(q, count, r.sample_parallel, stream);
    case FrameRoute::kLeanGeneric:
        return lean::launch_trace(q, r.path, count, r.lds, r.lds_bytes, stream, r.sample_parallel);
    default: return launch_trace(q, r.path, count, r.lds, r.lds_bytes, stream, r.sample_parallel);
    }
}

// Scenes with refraction trees take the breadth-first TraceRay when the roots fit the arena
// budget (RTAMD_WF_MB, default 4096 MiB); trees that overflow it are re-rendered per pixel.
// Reflection chains stay per pixel: measured 2-3x faster there (coherent, no stack), while
// the glass tree renders 4.6x faster breadth-first.  RTAMD_WF_CHAIN=1 forces chains too.
// *enqueued: whether the breadth-first launch went onto the stream (else the caller launches).
static rt_status enqueue_wavefront(rt_context* ctx, const TraceParams& p, const FrameRoute& r,
                                   bool* enqueued) {
    *enqueued = false;
    if (!r.arena) return RT_OK;
    const size_t n0 = static_cast<size_t>(p.rows) * p.width *
                      static_cast<size_t>(p.aa > 0 ? p.aa : 0);
    const char* env = std::getenv("RTAMD_WF_MB");
    const size_t budget = (env && std::atoll(env) > 0 ? static_cast<size_t>(std::atoll(env))
                                                      : size_t(4096)) << 20;
    // the deferred-direct queue is laid out only when that pass runs (refraction trees)
    const bool defer = r.path == kPathTree && wf_defer_selected();
    const size_t root_bytes = wf_arena_bytes(n0, n0, defer);
    if (n0 >= (size_t(1) << 30) || root_bytes > budget) return RT_OK;
    // ~100 B per non-root node (+16 B of queue when deferred)
    size_t extra = (budget - root_bytes) / (defer ? 116 : 100);
    extra = std::min(extra, std::max<size_t>(n0, 1) * 64);
    extra = std::min(extra, (size_t(1) << 31) - 1 - n0);
    const size_t cap = n0 + extra;
    RT_HIP(ctx->wf.ensure(wf_arena_bytes(n0, cap, defer)));
    RT_HIP(ctx->wf_ctl.ensure(sizeof(WfCtl)));
    const WfArena A = wf_arena_layout(ctx->wf.ptr, n0, cap, static_cast<WfCtl*>(ctx->wf_ctl.ptr),
                                      defer);
    // (an arena route is never the packet kernel's; the box kernel's scenes are lean ones)
    RT_HIP(r.kernel == FrameRoute::kGeneric
               ? launch_wavefront(p, r.path, A, r.lds, r.lds_bytes, ctx->stream)
               : lean::launch_wavefront(p, r.path, A, r.lds, r.lds_bytes, ctx->stream));
    *enqueued = true;
    return RT_OK;
}

rt_status enqueue_frames(rt_context* ctx, const rt_scene* sc, const rt_camera* cams, int nframes,
                         const rt_render_opts* opts, double* d64, float* d32, uint8_t* dldr,
                         uint32_t frame_rows) {
    TraceParams p;
    int path;
    bool lds;
    size_t lds_bytes;
    uint32_t rows;
    if (nframes != 1) RT_TRY(check_batch(cams, nframes));
    RT_TRY(build_params(ctx, sc, cams, opts, p, path, lds, lds_bytes, rows));
    p.out64 = d64;
    p.out32 = d32;
    p.ldr = dldr;
    const int flags = opts ? opts->flags : 0;
    if (!dldr) p.tonemap = RT_TONEMAP_NONE;
    if (dldr && p.tonemap == RT_TONEMAP_NONE) p.ldr = nullptr;
    FrameRoute route = choose_route(p, path, flags, sc, ctx, lds, lds_bytes);
    const bool packet = route.kernel == FrameRoute::kPacket;
    if (frame_rows && frame_rows < rows)
        return fail(RT_ERR_INVALID_ARG, "frame batch: frame stride below the rendered rows");
    const size_t frame_px = static_cast<size_t>(frame_rows ? frame_rows : rows) * p.width;
    if (nframes > 1 && (!packet || nframes > kPkMaxBatch)) {
        // one launch per frame (other kernels), or per kPkMaxBatch frames
        const int step = packet ? kPkMaxBatch : 1;
        for (int f0 = 0; f0 < nframes; f0 += step) {
            const size_t off = 3 * frame_px * static_cast<size_t>(f0);
            RT_TRY(enqueue_frames(ctx, sc, cams + f0, std::min(step, nframes - f0), opts,
                                  d64 ? d64 + off : nullptr, d32 ? d32 + off : nullptr,
                                  dldr ? dldr + off : nullptr, frame_rows));
        }
        return RT_OK;
    }
    bool scratch = (flags & RT_FLAG_COUNT_RAYS) || route.arena;

    EventPair ev{nullptr, nullptr};
    RT_TRY(timing_begin(ctx, flags, ev));
    rt_scene::PkImage::TileOrder* rec = nullptr;  // set: this launch records wave durations
    int batch_ring = -1;  // the ring entry of this batch's formed images, if any
    PkSplit pk_split{0u, 0u, 0u};  // the batch's tile lists, if every frame has them
    if (packet && nframes > 1) {
        // a frame batch: frame f's camera and image source, all formed before the launch by at
        // most one small launch (packet_batch_images)
        p.nframes = static_cast<uint32_t>(nframes);
        p.frame_px = frame_px;
        RT_TRY(packet_batch_images(ctx, sc, cams, nframes, p, flags, &rec, &batch_ring, &pk_split));
    } else if (packet) {
        RT_TRY(packet_image(ctx, sc, p, flags, &rec));
    }
    // the fix-up variant uses the context's fix-up list: ordered across streams like the counters
    route.fixup = packet && packet_uses_fixup(p, false, route.any_specular);
    if (route.fixup) {
        RT_TRY(fixup_buffers(ctx, nframes > 1 ? static_cast<size_t>(nframes) * frame_px
                                              : static_cast<size_t>(rows) * p.width, p));
        scratch = true;
    }
    if (scratch) RT_TRY(scratch_wait(ctx));
    // The fix-up variant's split launch (rt_packet.hip launch_packet_split): every frame of the
    // batch has its tile lists (packet_batch_images formed none under a tile order), and the two
    // launches go onto the render's stream one after the other
    if (!route.fixup || p.tile_order) pk_split.tiles = 0;
    if (packet) count_packet_frames(ctx, p, nframes, route.fixup, pk_split);
    bool wavefront;
    RT_TRY(enqueue_wavefront(ctx, p, route, &wavefront));
    if (!wavefront) RT_HIP(launch(route, p, false, ctx->stream, &pk_split));
    if (route.fixup) {
        const hipError_t fe = launch_packet_fixup(p, ctx->stream);
        if (fe != hipSuccess) {
            // the packet launch appended to the list and no fix-up launch zeroes the next count:
            // reset both, or a later fix-variant launch would append at a stale base past its list
            (void)hipMemsetAsync(ctx->fix_ctl.ptr, 0, 2 * sizeof(uint32_t), ctx->stream);
            return hip_fail(fe, "launch_packet_fixup");
        }
        ctx->fix_parity ^= 1;  // the next fix-variant launch appends to the count just zeroed
    }
    if (rec) RT_HIP(hipEventRecord(rec->recorded, ctx->stream));
    RT_TRY(timing_end(ctx, flags, ev));
    if (flags & RT_FLAG_COUNT_RAYS) {
        // Counting variant: same trace with wave-reduced atomics, outputs discarded.
        TraceParams pc = p;
        pc.out64 = nullptr;
        pc.out32 = nullptr;
        pc.ldr = nullptr;
        pc.counters = static_cast<unsigned long long*>(ctx->counters.ptr);
        pc.tile_cost = nullptr;  // the durations are the image launch's
        RT_HIP(launch(route, pc, true, ctx->stream, nullptr));
    }
    if (batch_ring >= 0) {  // the entry is free again once these launches have completed
        RT_HIP(hipEventRecord(sc->pk_batch_done[batch_ring], ctx->stream));
        sc->pk_batch_used[batch_ring] = true;
    }
    return scratch ? scratch_done(ctx) : RT_OK;
}

// ---- G-buffer (rt_gbuffer.hip) ------------------------------------------------------------
constexpr size_t kGbBytes[5] = {8, 4, 24, 8, 12};  // per pixel, in RT_GB_* bit order

rt_status check_gbuffer_args(int outputs, const rt_gbuffer_out* out) {
    if (outputs == 0) return fail(RT_ERR_INVALID_ARG, "G-buffer: no output requested");
    if (outputs & ~RT_GB_ALL) return fail(RT_ERR_INVALID_ARG, "G-buffer: unknown output bit");
    if (!out) return fail(RT_ERR_INVALID_ARG, "G-buffer: the output record is NULL");
    const void* ptr[5] = {out->depth, out->depth_norm, out->normal, out->prim, out->albedo};
    for (int k = 0; k < 5; ++k)
        if ((outputs & (1 << k)) && !ptr[k])
            return fail(RT_ERR_INVALID_ARG, "G-buffer: a requested output's pointer is NULL");
    return RT_OK;
}

// Enqueues the G-buffer pass of nframes cameras on ctx's stream into device outputs (checked by
// the caller, which holds a DeviceGuard); at most kPkMaxBatch frames per launch.
rt_status enqueue_gbuffer(rt_context* ctx, const rt_scene* sc, const rt_camera* cams, int nframes,
                          const rt_render_opts* opts_in, int outputs, const rt_gbuffer_out& out) {
    RT_TRY(check_batch(cams, nframes));
    rt_render_opts opts = resolved(opts_in);
    // not read here: whatever the caller left in them must neither fail nor steer the pass
    opts.max_recursion = 1;
    opts.tonemap = RT_TONEMAP_NONE;
    opts.flags &= RT_FLAG_GENERIC_KERNEL | RT_FLAG_NO_BVH | RT_FLAG_TIME_KERNEL;
    TraceParams p;
    int path;
    bool lds;
    size_t lds_bytes;
    uint32_t rows;
    RT_TRY(build_params(ctx, sc, cams, &opts, p, path, lds, lds_bytes, rows));
    const bool packet = !(opts.flags & RT_FLAG_GENERIC_KERNEL) &&
                        gbuffer_packet_fits(p, ctx->lds_limit);
    if (packet) p.nl = 0;  // the packet image is laid out without light records
    p.frame_px = static_cast<uint64_t>(rows) * p.width;
    GbOut g;

    EventPair ev{nullptr, nullptr};
    RT_TRY(timing_begin(ctx, opts.flags, ev));
    for (int f0 = 0; f0 < nframes; f0 += kPkMaxBatch) {
        const int n = std::min(kPkMaxBatch, nframes - f0);
        p.nframes = static_cast<uint32_t>(n);
        for (int f = 0; f < n; ++f) {
            for (int i = 0; i < 3; ++i) p.fr[f].cam[i] = cams[f0 + f].position[i];
            g.planes[f][0] = cams[f0 + f].near_plane;
            g.planes[f][1] = cams[f0 + f].far_plane;
        }
        const size_t off = static_cast<size_t>(f0) * p.frame_px;  // pixels
        auto at = [&](void* base, int bit, size_t elems) -> char* {
            return (outputs & bit) ? static_cast<char*>(base) + off * elems : nullptr;
        };
        g.depth = reinterpret_cast<double*>(at(out.depth, RT_GB_DEPTH, kGbBytes[0]));
        g.depth_norm = reinterpret_cast<float*>(at(out.depth_norm, RT_GB_DEPTH_NORM, kGbBytes[1]));
        g.normal = reinterpret_cast<double*>(at(out.normal, RT_GB_NORMAL, kGbBytes[2]));
        g.prim = reinterpret_cast<int32_t*>(at(out.prim, RT_GB_PRIM, kGbBytes[3]));
        g.albedo = reinterpret_cast<float*>(at(out.albedo, RT_GB_ALBEDO, kGbBytes[4]));
        RT_HIP(launch_gbuffer(p, g, packet, 0, ctx->stream));
    }
    return timing_end(ctx, opts.flags, ev);
}

}  // namespace rtamd

extern "C" {

const char* rt_last_error(void) { return g_last_error.c_str(); }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void rt_render_opts_default(rt_render_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->max_recursion = 10;         // Scene.h:24
    o->tonemap = RT_TONEMAP_ACES;  // RaytracingEngine.cpp:301 tonemap()
    o->bias = 1e-3;                // Scene.h:291
    o->seed = 0x5EEDull;
}

rt_status rt_context_create(int device, rt_context** out) {
    if (!out) return fail(RT_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(RT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n)
        return fail(RT_ERR_NO_DEVICE, "device " + std::to_string(device) + " not in [0," +
                                          std::to_string(n) + ")");
    hipDeviceProp_t prop;
    RT_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RT_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName +
                                          ", this build targets gfx950 only");
    DeviceGuard g(device);
    rt_context* ctx = new (std::nothrow) rt_context();
    if (!ctx) return fail(RT_ERR_OOM, "host allocation failed");
    ctx->device = device;
    // stay at <= 40 KiB of staged scene per 256-thread workgroup so >= 4 workgroups fit a CU
    ctx->lds_limit = 40 * 1024;
    hipError_t e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = ctx->counters.ensure(2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(ctx->counters.ptr, 0, 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->scratch_event, hipEventDisableTiming);
    if (e != hipSuccess) {
        rt_context_destroy(ctx);
        return hip_fail(e, "rt_context_create");
    }
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return RT_OK;
}

rt_status rt_context_destroy(rt_context* ctx) {
    if (!ctx) return RT_OK;
    DeviceGuard g(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto* v : {&ctx->pending, &ctx->free_events})
        for (auto& ev : *v) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
    if (ctx->scratch_event) {
        (void)hipEventSynchronize(ctx->scratch_event);
        (void)hipEventDestroy(ctx->scratch_event);
    }
    leave_groups(ctx);  // communicators of any group this context is in go first
    for (DeviceBuffer* b : {&ctx->out64, &ctx->out32, &ctx->ldr, &ctx->tm_in, &ctx->tm_out,
                            &ctx->dbg, &ctx->rays, &ctx->counters, &ctx->wf, &ctx->wf_ctl,
                            &ctx->fix_list, &ctx->fix_ctl, &ctx->adapt_list, &ctx->adapt_ctl})
        b->release();
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    return RT_OK;
}

rt_status rt_context_set_stream(rt_context* ctx, void* hip_stream) {
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "context is NULL");
    ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return RT_OK;
}

rt_status rt_context_synchronize(rt_context* ctx) {
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "context is NULL");
    DeviceGuard g(ctx->device);
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

rt_status rt_scene_create(rt_context* ctx, const rt_scene_desc* d, rt_scene** out) {
    if (!ctx || !d || !out) return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_scene_create");
    *out = nullptr;
    if (d->n_spheres < 0 || d->n_planes < 0 || d->n_triangles < 0 || d->n_lights < 0)
        return fail(RT_ERR_INVALID_ARG, "negative primitive count");
    if ((d->n_spheres && !d->spheres) || (d->n_planes && !d->planes) ||
        (d->n_triangles && !d->triangles) || (d->n_lights && !d->lights))
        return fail(RT_ERR_INVALID_ARG, "primitive count > 0 with NULL array");
    DeviceGuard g(ctx->device);

    rt_scene* sc = new (std::nothrow) rt_scene();
    if (!sc) return fail(RT_ERR_OOM, "host allocation failed");
    sc->ctx = ctx;
    sc->ns = d->n_spheres;
    sc->np = d->n_planes;
    sc->nt = d->n_triangles;
    sc->nl = d->n_lights;
    size_t off = 0;
    auto take = [&off](size_t n) {
        size_t o = off;
        off += (n + 1) & ~size_t(1);  // keep every array 16-byte aligned
        return o;
    };
    sc->off_sph = take(size_t(kSphStride) * sc->ns);
    sc->off_pl = take(size_t(kPlStride) * sc->np);
    sc->off_tri = take(size_t(kTriStride) * sc->nt);
    sc->off_lt = take(size_t(kLtStride) * sc->nl);
    // one material table [spheres | planes | triangles]: a hit's material is one integer
    // offset away (no pointer select, so global loads instead of flat ones)
    sc->off_sph_mat = take(size_t(kMatStride) * (size_t(sc->ns) + sc->np + sc->nt));
    sc->off_pl_mat = sc->off_sph_mat + size_t(kMatStride) * sc->ns;
    sc->off_tri_mat = sc->off_pl_mat + size_t(kMatStride) * sc->np;
    std::vector<double> h(off + 2, 0.0);

    bool transparent = false;
    double max_spec = 0.0;
    auto note = [&](const rt_material& m) {
        if (!(m.transparency <= 0.0)) transparent = true;
        if (std::isnan(m.specular)) max_spec = INFINITY;
        else if (m.specular > max_spec) max_spec = m.specular;
    };
    for (int i = 0; i < sc->ns; ++i) {
        const rt_sphere& s = d->spheres[i];
        double* o = &h[sc->off_sph + size_t(kSphStride) * i];
        o[0] = s.center[0];
        o[1] = s.center[1];
        o[2] = s.center[2];
        o[3] = s.radius * s.radius;  // Shape.h:77
        pack_material(s.material, &h[sc->off_sph_mat + size_t(kMatStride) * i]);
        note(s.material);
    }
    for (int i = 0; i < sc->np; ++i) {
        const rt_plane& pl = d->planes[i];
        double* o = &h[sc->off_pl + size_t(kPlStride) * i];
        for (int k = 0; k < 3; ++k) {
            o[k] = pl.point[k];
            o[3 + k] = pl.normal[k];
        }
        pack_material(pl.material, &h[sc->off_pl_mat + size_t(kMatStride) * i]);
        note(pl.material);
    }
    for (int i = 0; i < sc->nt; ++i) {
        const rt_triangle& t = d->triangles[i];
        double* o = &h[sc->off_tri + size_t(kTriStride) * i];
        double a0[3], a1[3], a2[3], e1u[3], e2u[3], n[3];
        for (int k = 0; k < 3; ++k) {
            a0[k] = t.v0[k] + t.translation[k];  // tv0() Shape.h:198
            a1[k] = t.v1[k] + t.translation[k];
            a2[k] = t.v2[k] + t.translation[k];
            e1u[k] = t.v1[k] - t.v0[k];          // untranslated edges for the normal
            e2u[k] = t.v2[k] - t.v0[k];
        }
        const double c[3] = {e1u[1] * e2u[2] - e1u[2] * e2u[1], e1u[2] * e2u[0] - e1u[0] * e2u[2],
                             e1u[0] * e2u[1] - e1u[1] * e2u[0]};
        normalize3(c, n);
        for (int k = 0; k < 3; ++k) {
            o[k] = a0[k];
            o[3 + k] = a1[k] - a0[k];  // edge1 = tv1() - a0
            o[6 + k] = a2[k] - a0[k];  // edge2 = tv2() - a0
            o[9 + k] = n[k];
        }
        pack_material(t.material, &h[sc->off_tri_mat + size_t(kMatStride) * i]);
        note(t.material);
    }
    for (int i = 0; i < sc->nl; ++i) {
        const rt_light& l = d->lights[i];
        double* o = &h[sc->off_lt + size_t(kLtStride) * i];
        for (int k = 0; k < 3; ++k) {
            o[k] = l.position[k];
            o[3 + k] = l.color[k] * l.intensity;  // Scene.h:110 emitted
        }
    }
    sc->any_transparent = transparent;
    sc->max_specular = max_spec;

    // triangle BVH (rt_bvh.cpp) appended to the same allocation: nodes, then the leaf-order
    // triangle ids packed two per double slot
    if (sc->nt >= kBvhMinTris) {
        std::vector<double> nodes;
        std::vector<int32_t> order;
        build_triangle_bvh(&h[sc->off_tri], sc->nt, nodes, order);
        sc->off_bvh = h.size();
        sc->off_bvh_tri = sc->off_bvh + nodes.size();
        h.resize(sc->off_bvh_tri + (order.size() + 1) / 2 + 2, 0.0);
        std::memcpy(&h[sc->off_bvh], nodes.data(), nodes.size() * sizeof(double));
        std::memcpy(&h[sc->off_bvh_tri], order.data(), order.size() * sizeof(int32_t));
        sc->bvh_nodes = static_cast<int32_t>(nodes.size() / kBvhNodeStride);
    }

    // spatial sphere chunks of the packet kernel's culls: permutation (packed two per double
    // slot) and one bounding sphere per chunk
    if (sc->ns >= kSphChunkMin) {
        std::vector<int32_t> perm;
        std::vector<double> bnd;
        build_sphere_chunks(&h[sc->off_sph], sc->ns, perm, bnd);
        sc->off_sbnd = (h.size() + 1) & ~size_t(1);
        sc->off_sperm = sc->off_sbnd + bnd.size();
        h.resize(sc->off_sperm + (perm.size() + 1) / 2 + 2, 0.0);
        std::memcpy(&h[sc->off_sbnd], bnd.data(), bnd.size() * sizeof(double));
        std::memcpy(&h[sc->off_sperm], perm.data(), perm.size() * sizeof(int32_t));
    }

    // planes-only chain table (rt_box.hip): the planes grouped by the axis of their normal —
    // exactly ±e_x, ±e_y, ±e_z (two zero components, the third ±1), then the rest — each group
    // in scene order, with the plane's material, a flag for normals whose normalize() returns
    // them unchanged (|n| rounds to 1: sqrt of the reference's dot, correctly rounded as on the
    // device) and the scene index for closest-hit ties
    if (sc->np > 0) {
        std::vector<int> grp(sc->np);
        for (int i = 0; i < sc->np; ++i) {
            const double* q = &h[sc->off_pl + size_t(kPlStride) * i];
            const double* n = q + 3;
            grp[i] = 3;
            const bool bounded = std::fabs(q[0]) <= 0x1p1000 && std::fabs(q[1]) <= 0x1p1000 &&
                                 std::fabs(q[2]) <= 0x1p1000;  // p − o stays finite (rt_box.hip)
            for (int k = 0; k < 3 && bounded; ++k)
                if (std::fabs(n[k]) == 1.0 && n[(k + 1) % 3] == 0.0 && n[(k + 2) % 3] == 0.0)
                    grp[i] = k;
        }
        sc->off_box = (h.size() + 1) & ~size_t(1);
        h.resize(sc->off_box + size_t(kBoxRec) * sc->np + 2, 0.0);
        size_t r = 0;
        for (int g = 0; g < 4; ++g) {
            for (int i = 0; i < sc->np; ++i) {
                if (grp[i] != g) continue;
                const double* pl = &h[sc->off_pl + size_t(kPlStride) * i];
                double* o = &h[sc->off_box + size_t(kBoxRec) * r++];
                for (int k = 0; k < 6; ++k) o[k] = pl[k];
                o[6] = g < 3 ? pl[g] : 0.0;
                const double nn = pl[3] * pl[3] + pl[4] * pl[4] + pl[5] * pl[5];
                o[7] = std::sqrt(nn) == 1.0 ? 1.0 : 0.0;
                for (int k = 0; k < kMatStride - 1; ++k)
                    o[8 + k] = h[sc->off_pl_mat + size_t(kMatStride) * i + k];
                const int32_t idx[2] = {i, 0};
                std::memcpy(&o[15], idx, sizeof idx);
                ++sc->box_n[g];
            }
        }
    }

    hipError_t e = sc->buf.ensure(h.size() * sizeof(double));
    if (e == hipSuccess)
        e = hipMemcpyAsync(sc->buf.ptr, h.data(), h.size() * sizeof(double),
                           hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        sc->buf.release();
        delete sc;
        return hip_fail(e, "rt_scene_create upload");
    }
    *out = sc;
    return RT_OK;
}

rt_status rt_scene_destroy(rt_scene* sc) {
    if (!sc) return RT_OK;
    DeviceGuard g(sc->ctx->device);
    // Launches that read the scene or its packet images may be in flight on any stream the
    // context used (rt_context_set_stream switches it; pipelined frames use several), not only
    // the current one: wait for the whole device before freeing.
    (void)hipDeviceSynchronize();
    sc->buf.release();
    sc->pk_pub.release();
    sc->pk_batch.release();
    for (auto& e : sc->pk_batch_done)
        if (e) (void)hipEventDestroy(e);
    for (auto& im : sc->pk_images) {
        im.buf.release();
        if (im.ready) (void)hipEventDestroy(im.ready);
        for (auto& o : im.ords) {
            o.cost.release();
            o.keys.release();
            o.order.release();
            if (o.recorded) (void)hipEventDestroy(o.recorded);
            if (o.built) (void)hipEventDestroy(o.built);
            if (o.verdict) (void)hipHostFree(o.verdict);
        }
        for (auto& t : im.tabs) {
            t.buf.release();
            if (t.ready) (void)hipEventDestroy(t.ready);
            if (t.counts) (void)hipHostFree(t.counts);
        }
    }
    for (auto& b : sc->pk_batch_tab) b.release();
    delete sc;
    return RT_OK;
}

rt_status rt_scene_set_area_light(rt_scene* sc, const rt_area_light* light) {
    if (!sc) return fail(RT_ERR_INVALID_ARG, "scene is NULL");
    if (!light) {
        sc->has_area = false;
        return RT_OK;
    }
    if (light->samples <= 0) return fail(RT_ERR_INVALID_ARG, "area light needs samples > 0");
    const int k = static_cast<int>(std::lround(std::sqrt(static_cast<double>(light->samples))));
    if (k * k != light->samples)
        return fail(RT_ERR_INVALID_ARG, "area light samples must be a perfect square");
    sc->area = *light;
    sc->has_area = true;
    return RT_OK;
}

rt_status rt_render_device(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                           const rt_render_opts* opts, void* d64, void* d32, void* dldr) {
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "context is NULL");
    DeviceGuard g(ctx->device);
    return enqueue_render(ctx, sc, cam, opts, static_cast<double*>(d64), static_cast<float*>(d32),
                   static_cast<uint8_t*>(dldr));
}

rt_status rt_render_batch(rt_context* ctx, const rt_scene* sc, const rt_camera* cams,
                          int nframes, const rt_render_opts* opts, void* d64, void* d32,
                          void* dldr) {
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "context is NULL");
    RT_TRY(check_batch(cams, nframes));
    DeviceGuard g(ctx->device);
    return enqueue_frames(ctx, sc, cams, nframes, opts, static_cast<double*>(d64),
                          static_cast<float*>(d32), static_cast<uint8_t*>(dldr));
}

rt_status rt_gbuffer_device(rt_context* ctx, const rt_scene* sc, const rt_camera* cams,
                            int nframes, const rt_render_opts* opts, int outputs,
                            const struct rt_gbuffer* d_out) {
    RT_TRY(check_gbuffer_args(outputs, d_out));
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "context is NULL");
    DeviceGuard g(ctx->device);
    return enqueue_gbuffer(ctx, sc, cams, nframes, opts, outputs, *d_out);
}

rt_status rt_gbuffer(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                     const rt_render_opts* opts, int outputs, const struct rt_gbuffer* h_out) {
    RT_TRY(check_gbuffer_args(outputs, h_out));
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "context is NULL");
    RT_TRY(validate_camera(cam));
    DeviceGuard g(ctx->device);
    const rt_render_opts o = resolved(opts);
    const size_t npx = static_cast<size_t>(rendered_rows(o, cam->height)) * cam->width;
    // one staging allocation, every requested output at a 256-byte boundary
    void* const host[5] = {h_out->depth, h_out->depth_norm, h_out->normal, h_out->prim,
                           h_out->albedo};
    size_t off[5], total = 0;
    for (int k = 0; k < 5; ++k) {
        off[k] = total;
        if (outputs & (1 << k)) total += (npx * kGbBytes[k] + 255) / 256 * 256;
    }
    RT_HIP(ctx->out64.ensure(total));
    char* base = static_cast<char*>(ctx->out64.ptr);
    rt_gbuffer_out d{base + off[0], base + off[1], base + off[2], base + off[3], base + off[4]};
    RT_TRY(enqueue_gbuffer(ctx, sc, cam, 1, &o, outputs, d));
    for (int k = 0; k < 5; ++k)
        if (outputs & (1 << k))
            RT_HIP(hipMemcpyAsync(host[k], base + off[k], npx * kGbBytes[k], hipMemcpyDeviceToHost,
                                  ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

rt_status rt_render(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                    const rt_render_opts* opts, double* h64, float* h32, uint8_t* hldr,
                    rt_stats* stats) {
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "context is NULL");
    RT_TRY(validate_camera(cam));
    DeviceGuard g(ctx->device);
    rt_render_opts o = resolved(opts);
    if (stats) o.flags |= RT_FLAG_COUNT_RAYS;
    const FrameStage fs(ctx, h64, h32, hldr,
                        static_cast<size_t>(rendered_rows(o, cam->height)) * cam->width);
    RT_TRY(fs.grow());
    if (stats) {
        RT_TRY(scratch_wait(ctx));  // the counters: after any counting render on another stream
        RT_TRY(counters_zero(ctx));
    }
    RT_TRY(enqueue_render(ctx, sc, cam, &o, fs.d64(), fs.d32(), fs.dldr()));
    RT_TRY(fs.download());
    unsigned long long c[2] = {0, 0};
    if (stats) {
        // the read-back is the counters' last use: a counting render queued on another stream
        // waits for it (scratch_event), not only for the counting launch
        RT_TRY(counters_read(ctx, c, true));
        RT_TRY(scratch_done(ctx));
    }
    RT_HIP(hipStreamSynchronize(ctx->stream));
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->trace_rays = c[0];
        stats->shadow_rays = c[1];
        if (o.flags & RT_FLAG_TIME_KERNEL) {
            RT_TRY(harvest_events(ctx, true));
            stats->kernel_ms = ctx->timed_ms;
            stats->launches = ctx->launches;
        }
    }
    return RT_OK;
}

rt_status rt_stats_read(rt_context* ctx, rt_stats* out) {
    if (!ctx || !out) return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_stats_read");
    DeviceGuard g(ctx->device);
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_TRY(harvest_events(ctx, true));
    unsigned long long c[2] = {0, 0};
    RT_TRY(counters_read(ctx, c, false));
    out->trace_rays = c[0];
    out->shadow_rays = c[1];
    out->kernel_ms = ctx->timed_ms;
    out->launches = ctx->launches;
    return RT_OK;
}

rt_status rt_stats_reset(rt_context* ctx) {
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "context is NULL");
    DeviceGuard g(ctx->device);
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_TRY(harvest_events(ctx, true));
    ctx->timed_ms = 0.0;
    ctx->launches = 0;
    RT_HIP(hipMemset(ctx->counters.ptr, 0, 2 * sizeof(unsigned long long)));
    return RT_OK;
}

rt_status rt_debug_f64_ops(rt_context* ctx, const double* x, const double* y, size_t n,
                           double* out) {
    if (!ctx || !x || !y || !out) return fail(RT_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard g(ctx->device);
    RT_HIP(ctx->dbg.ensure(n * 7 * sizeof(double)));
    double* dx = static_cast<double*>(ctx->dbg.ptr);
    double* dy = dx + n;
    double* dout = dy + n;
    RT_HIP(hipMemcpyAsync(dx, x, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(hipMemcpyAsync(dy, y, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(launch_debug_f64(dx, dy, n, dout, ctx->stream));
    RT_HIP(hipMemcpyAsync(out, dout, 5 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

rt_status rt_debug_tile_order(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                              uint32_t* order, uint32_t* cost, size_t capacity, uint32_t* tiles,
                              uint32_t* waves, int* state) {
    if (!ctx || !sc || !cam || !tiles || !waves || !state)
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_debug_tile_order");
    *tiles = *waves = 0;
    *state = 0;
    DeviceGuard g(ctx->device);
    RT_HIP(hipDeviceSynchronize());
    for (const auto& im : sc->pk_images) {
        if (std::memcmp(im.cam, cam->position, sizeof im.cam) != 0) continue;
        if (im.last_ord < 0) return RT_OK;
        const auto& o = im.ords[static_cast<size_t>(im.last_ord)];
        *state = o.state;
        if (o.state == 0) return RT_OK;
        *tiles = o.key[0] * o.key[1];
        *waves = o.key[2];
        if (order && o.state == 2) {
            if (capacity < *tiles) return fail(RT_ERR_INVALID_ARG, "order capacity too small");
            RT_HIP(hipMemcpy(order, o.order.ptr, sizeof(uint32_t) * *tiles, hipMemcpyDeviceToHost));
        }
        if (cost) {
            if (capacity < size_t(*tiles) * *waves)
                return fail(RT_ERR_INVALID_ARG, "cost capacity too small");
            RT_HIP(hipMemcpy(cost, o.cost.ptr, sizeof(uint32_t) * *tiles * *waves,
                             hipMemcpyDeviceToHost));
        }
        return RT_OK;
    }
    return RT_OK;
}

static rt_status debug_counter(rt_context* ctx, rt_context::PkCounter c, uint64_t* with,
                               uint64_t* without, const char* entry) {
    if (!ctx || !with || !without)
        return fail(RT_ERR_INVALID_ARG, std::string("NULL argument to ") + entry);
    *with = ctx->pk_frames[c][0];
    *without = ctx->pk_frames[c][1];
    return RT_OK;
}

rt_status rt_debug_cone_table(rt_context* ctx, uint64_t* with_table, uint64_t* without_table) {
    return debug_counter(ctx, rt_context::kCntConeTable, with_table, without_table, __func__);
}

rt_status rt_debug_shadow_table(rt_context* ctx, uint64_t* with_table, uint64_t* without_table) {
    return debug_counter(ctx, rt_context::kCntShadowTable, with_table, without_table, __func__);
}

rt_status rt_debug_tile_class(rt_context* ctx, uint64_t* with_words, uint64_t* without_words) {
    return debug_counter(ctx, rt_context::kCntTileClass, with_words, without_words, __func__);
}

rt_status rt_debug_plane_clear(rt_context* ctx, uint64_t* with_masks, uint64_t* without_masks) {
    return debug_counter(ctx, rt_context::kCntPlaneClear, with_masks, without_masks, __func__);
}

rt_status rt_debug_tile_split(rt_context* ctx, uint64_t* split, uint64_t* single) {
    return debug_counter(ctx, rt_context::kCntTileSplit, split, single, __func__);
}

rt_status rt_debug_tile_shadowed(rt_context* ctx, uint64_t* with, uint64_t* without) {
    return debug_counter(ctx, rt_context::kCntTileShadowed, with, without, __func__);
}

rt_status rt_debug_fixup_count(rt_context* ctx, uint32_t* pixels) {
    if (!ctx || !pixels) return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_debug_fixup_count");
    *pixels = 0;
    if (!ctx->fix_ctl.ptr) return RT_OK;
    DeviceGuard g(ctx->device);
    RT_HIP(hipStreamSynchronize(ctx->stream));
    // the count the last fix-variant launch appended to: its fix-up launch zeroed the other one
    RT_HIP(hipMemcpy(pixels, static_cast<const uint32_t*>(ctx->fix_ctl.ptr) + (1 - ctx->fix_parity),
                     sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status rt_debug_adaptive_listed(rt_context* ctx, uint32_t* pixels) {
    if (!ctx || !pixels)
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_debug_adaptive_listed");
    *pixels = 0;
    if (!ctx->adapt_listing) return RT_OK;
    DeviceGuard g(ctx->device);
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_HIP(hipMemcpy(pixels, ctx->adapt_ctl.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

rt_status rt_debug_vec_ops(rt_context* ctx, const double* v, size_t n, double* out) {
    if (!ctx || !v || !out) return fail(RT_ERR_INVALID_ARG, "NULL argument");
    DeviceGuard g(ctx->device);
    RT_HIP(ctx->dbg.ensure(n * 19 * sizeof(double)));
    double* dv = static_cast<double*>(ctx->dbg.ptr);
    double* dout = dv + 3 * n;
    RT_HIP(hipMemcpyAsync(dv, v, 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(launch_debug_vec(dv, n, dout, ctx->stream));
    RT_HIP(hipMemcpyAsync(out, dout, 16 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

}  // extern "C"
