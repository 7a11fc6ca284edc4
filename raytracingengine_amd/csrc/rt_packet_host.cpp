// rt_packet_host.cpp — the host half of the packet path: per scene, the cache of camera images
// (rt_scene::PkImage), the publish slots of cameras without one, the costliest-first tile
// orders and a frame batch's image sources.  enqueue_frames (rt_capi.cpp) calls packet_image
// or packet_batch_images before a packet launch; the rest is local to this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "rt_context.hpp"
#include "rt_internal.hpp"
#include "rt_shadow_table.hpp"

#pragma clang fp contract(off)

namespace rtamd {
namespace {

// The packet kernel's LDS image for this scene and camera (p.pk_image): looked up by camera
// position and formed by one setup launch the SECOND time a camera is rendered, then copied by
// every workgroup instead of being recomputed per workgroup.  A camera seen once (a moving
// camera) takes the in-kernel prologue and costs no setup launch; the last kMaxPkSeen such
// positions are remembered.  Past kMaxPkImages cached cameras the kernel forms it in LDS.
constexpr size_t kMaxPkImages = 16;
constexpr size_t kMaxPkSeen = 16;
// Launch shapes (grid, row set) with their own costliest-first tile order per cached camera.
constexpr size_t kMaxTileOrders = 8;
// A camera without a cached image gets a publish slot instead: the launch's first workgroup
// forms the image and hands it to the later ones through {epoch, word} granules
// (rt_packet_kernel.hpp).  Slots rotate so that launches in flight on other streams keep
// theirs; a slot overwritten by a
// later launch only fails its tags (the workgroup then forms the image itself).  Images above
// kPkPubMaxWords 32-bit words (4 KiB, about 32 spheres) are formed per workgroup: reading twice
// their size in granules costs as much as forming them (moving camera, MI355X: C2's 1.9 KiB
// image 54.1 -> 50.8 us; C3's 14.3 KiB 555 -> 555 us; C5's 6.5 KiB 522 -> 530 us).
constexpr size_t kPkPubSlots = 32;
constexpr size_t kPkPubMaxWords = 1024;
// Epochs are unique across the process (not per scene): a slot whose memory held another
// scene's granules (a freed and re-allocated buffer) can never match a later launch's tags.
std::atomic<uint32_t> g_pk_epoch{0};
rt_status packet_publish_slot(rt_context* ctx, const rt_scene* sc, TraceParams& p) {
    const size_t words = packet_lds_bytes(p.ns, p.np, p.nl) / 4;
    // RTAMD_PK_PUB=0: every workgroup forms it (A/B runs; read once)
    static const bool off = packet_switch_off("RTAMD_PK_PUB");
    if (off || words > kPkPubMaxWords) return RT_OK;
    const size_t slot = kPkPubMaxWords * sizeof(unsigned long long);
    if (!sc->pk_pub.ptr) {
        // zeroed (epoch 0 is never used) and complete before any stream's launch reads it
        RT_HIP(sc->pk_pub.ensure(kPkPubSlots * slot));
        RT_HIP(hipMemsetAsync(sc->pk_pub.ptr, 0, kPkPubSlots * slot, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));
    }
    uint32_t ep = ++g_pk_epoch;
    if (ep == 0) ep = ++g_pk_epoch;
    p.pk_epoch = ep;
    // the first resident round: 256 CUs x 10 workgroups of 128 threads (20 waves per CU)
    static const long first_env = [] {
        const char* e = std::getenv("RTAMD_PK_PUB_FIRST");
        return e ? std::atol(e) : -1L;
    }();
    int cus = 0;
    RT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    p.pk_pub_first = first_env >= 0 ? static_cast<uint32_t>(first_env)
                                    : static_cast<uint32_t>(cus > 0 ? cus : 256) * 10u;
    p.pk_pub = reinterpret_cast<unsigned long long*>(static_cast<char*>(sc->pk_pub.ptr) +
                                                     (ep % kPkPubSlots) * slot);
    return RT_OK;
}
// Costliest tiles first (rt_packet.hip packet_order_kernel): the launch that creates a camera's
// packet image also records every wave's duration; the next launch of the same shape sorts the
// tiles by them (one small kernel, once) and every later one dispatches the costliest tiles
// first, so the cheapest fill the partly idle end of the launch.  The order only permutes which
// workgroup renders which tile: every pixel is computed by the same instructions, so images do
// not change (RT_FLAG_NO_TILE_ORDER: the default order, for A/B runs and the tests).  `*rec`
// receives the entry whose recording launch enqueue_render marks complete.
// existing_only: use an order already built for this shape, never record or build one (frame
// batches with several cameras: their launch neither pays the recording nor waits on a build).
rt_status tile_order(rt_context* ctx, rt_scene::PkImage& im, TraceParams& p, int flags,
                     rt_scene::PkImage::TileOrder** rec, bool existing_only = false) {
    *rec = nullptr;
    if (flags & RT_FLAG_NO_TILE_ORDER) return RT_OK;
    uint32_t gx, gy, waves;
    packet_grid(p, gx, gy, waves);
    const uint32_t key[8] = {gx, gy, waves, p.width, p.height, p.rows, p.row0,
                             (p.row_block << 16) ^ p.row_stride};
    const uint32_t tiles = gx * gy;
    size_t idx = 0;
    while (idx < im.ords.size() && std::memcmp(im.ords[idx].key, key, sizeof key) != 0) ++idx;
    if (existing_only && (idx == im.ords.size() || im.ords[idx].state != 2)) return RT_OK;
    if (idx == im.ords.size()) {  // a new launch shape: record this launch
        if (im.ords.size() >= kMaxTileOrders) return RT_OK;  // the default order
        if (im.ords.capacity() < kMaxTileOrders) im.ords.reserve(kMaxTileOrders);
        im.ords.emplace_back();
        auto& o = im.ords.back();
        im.last_ord = static_cast<int>(idx);
        hipError_t e = o.cost.ensure(sizeof(uint32_t) * tiles * waves);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&o.recorded, hipEventDisableTiming);
        if (e != hipSuccess) {
            o.cost.release();
            im.ords.pop_back();
            im.last_ord = -1;
            return hip_fail(e, "tile order");
        }
        std::memcpy(o.key, key, sizeof key);
        o.state = 1;
        p.tile_cost = static_cast<uint32_t*>(o.cost.ptr);
        *rec = &o;
        return RT_OK;
    }
    auto& o = im.ords[idx];
    im.last_ord = static_cast<int>(idx);
    if (o.state == 1) {  // build the order (after the recording launch, on whatever stream)
        RT_HIP(o.keys.ensure(sizeof(uint32_t) * tiles));
        RT_HIP(o.order.ensure(sizeof(uint32_t) * tiles));
        if (!o.built) RT_HIP(hipEventCreateWithFlags(&o.built, hipEventDisableTiming));
        if (!o.verdict) RT_HIP(hipHostMalloc(reinterpret_cast<void**>(&o.verdict), sizeof(uint32_t)));
        __atomic_store_n(o.verdict, 0u, __ATOMIC_RELAXED);
        RT_HIP(hipStreamWaitEvent(ctx->stream, o.recorded, 0));
        RT_HIP(launch_packet_order(static_cast<const uint32_t*>(o.cost.ptr), gx, gy, waves,
                                   static_cast<uint32_t*>(o.keys.ptr),
                                   static_cast<uint32_t*>(o.order.ptr), o.verdict, ctx->stream));
        RT_HIP(hipEventRecord(o.built, ctx->stream));
        o.state = 2;
    } else {
        // a narrow cost distribution keeps the default order: no table at all (the verdict is
        // only ever read as "narrow" once the order kernel has written it)
        if (__atomic_load_n(o.verdict, __ATOMIC_RELAXED) == 1u) return RT_OK;
        RT_HIP(hipStreamWaitEvent(ctx->stream, o.built, 0));  // built on another stream
    }
    p.tile_order = static_cast<const uint32_t*>(o.order.ptr);
    return RT_OK;
}

// A launch whose camera has no image entry yet (a moving camera): an order built earlier for the
// same launch shape under another camera of the scene, if any — an order only permutes which
// workgroup renders which tile, and nearby cameras share their costly tiles.
rt_status scene_tile_order(rt_context* ctx, const rt_scene* sc, TraceParams& p, int flags,
                           rt_scene::PkImage::TileOrder** rec) {
    for (auto& im : sc->pk_images) {
        const rt_status st = tile_order(ctx, im, p, flags, rec, true);
        if (st != RT_OK || p.tile_order) return st;
    }
    return RT_OK;
}

// The cached image of this camera position, or null; a render on another stream than the one
// that formed it waits for the entry's event until it has completed.
rt_status packet_image_cached(rt_context* ctx, const rt_scene* sc, const double* cam,
                              rt_scene::PkImage** out) {
    *out = nullptr;
    for (auto& im : sc->pk_images) {
        if (std::memcmp(im.cam, cam, sizeof im.cam) != 0) continue;
        if (!im.done && im.stream != ctx->stream) {
            const hipError_t q = hipEventQuery(im.ready);
            if (q == hipSuccess) im.done = true;
            else if (q == hipErrorNotReady) RT_HIP(hipStreamWaitEvent(ctx->stream, im.ready, 0));
            else return hip_fail(q, "hipEventQuery");
        }
        *out = &im;
        return RT_OK;
    }
    return RT_OK;
}

// A camera without a cached image: true when it was seen before (the last kMaxPkSeen first
// sightings) and the cache has room, i.e. it should get a cache entry now (removed from the seen
// list); otherwise it is remembered as seen once.
bool packet_second_sighting(const rt_scene* sc, const double* cam) {
    auto& seen = sc->pk_seen;
    auto it = std::find_if(seen.begin(), seen.end(), [&](const std::array<double, 3>& c) {
        return std::memcmp(c.data(), cam, 3 * sizeof(double)) == 0;
    });
    if (it == seen.end()) {
        if (seen.size() >= kMaxPkSeen) seen.erase(seen.begin());
        seen.push_back({cam[0], cam[1], cam[2]});
        return false;
    }
    if (sc->pk_images.size() >= kMaxPkImages) return false;
    seen.erase(it);
    return true;
}

// A new cache entry for this camera (its buffer allocated, its event created; the caller
// enqueues the launch that forms the image and records `ready` after it on ctx->stream).
rt_status packet_image_entry(rt_context* ctx, const rt_scene* sc, const double* cam,
                             const TraceParams& p, rt_scene::PkImage** out) {
    *out = nullptr;
    // never reallocated: a frame batch holds entries of earlier frames while adding one
    if (sc->pk_images.capacity() < kMaxPkImages) sc->pk_images.reserve(kMaxPkImages);
    sc->pk_images.emplace_back();
    rt_scene::PkImage& im = sc->pk_images.back();
    std::memcpy(im.cam, cam, sizeof im.cam);
    im.stream = ctx->stream;
    hipError_t e = im.buf.ensure(packet_lds_bytes(p.ns, p.np, p.nl));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&im.ready, hipEventDisableTiming);
    if (e != hipSuccess) {
        im.buf.release();
        if (im.ready) (void)hipEventDestroy(im.ready);
        sc->pk_images.pop_back();
        return hip_fail(e, "packet image entry");
    }
    *out = &im;
    return RT_OK;
}

// Tile tables (rt_tile_table.hpp says what one holds and where; the kernel's pointers into one
// are TraceParams.cone_tab / shadow_tab / class_tab and fr_tab / fr_stab / fr_ctab).  A table
// belongs to a camera, its ray constants, a launch shape and its contents (cone_table_key): a
// cached camera keeps up to kMaxConeTabs of them next to its image (later shapes or focal lengths
// go without), each formed once by a small launch on the stream that first needs it and guarded
// by an event for the others; a batch frame without a cached image gets one in the batch's ring
// entry, formed by one launch per batch.  A one-frame launch of a camera seen for the first time
// (the publish-slot path) gets none: a setup launch per frame costs more than the frame saves.
// What a launch's tables hold, and which sections reach the kernel, is tables_wanted's answer:
// the scene, the launch and the RTAMD_PK_* switches (each read per launch, 0 = off) decide, and
// a table formed with other contents is one of its own in the cache.
//   RTAMD_PK_CONE_TAB      the cone pointer (the words are still formed: the others need them)
//   RTAMD_PK_SHADOW_TAB    the shadow words and their pointer; they depend on the render call's
//                          bias, so a table that holds them is keyed by it
//   RTAMD_PK_TILE_CLASS    the class words (only with both of the above)
//   RTAMD_PK_PLANE_CLEAR   their shadow-plane keep masks (else all ones: every plane classified)
//   RTAMD_PK_TILE_SPLIT    the lists, for the frame batches that take the fix-up variant
//   RTAMD_PK_TILE_SHADOWED the shadowed-plane mark and the third list
// A cache entry's table with lists also has two pinned host words that receive the lists' counts
// once the table is formed (TileListCounts), which size the split launch's grids; a batch with a
// ring frame (a camera seen for the first time) forms no lists and stays one launch, as does the
// batch whose launch forms a table.
constexpr size_t kMaxConeTabs = 8;
// The ring's table memory per entry (kPkBatchRing entries), counted in cone words: a 32-frame
// 1080p batch takes 8.3 MB (259 KB a frame), a 4K frame 1 MB; frames past the cap go without a
// table.  The class words count too (as much again: 16.6 MB for the 32-frame batch, still under
// the cap).  The shadow words come on top (nl times as much, 8.3 MB for a 32-frame C2 batch).
constexpr size_t kConeRingBytes = size_t(16) << 20;

struct TabsWanted {
    bool cone, shadow;  // which of the cone and shadow pointers the kernel gets
    TileTabContents c;  // what the launch's tables hold (the class pointer: c.has_class())
    bool any() const { return cone || shadow; }
};
TabsWanted tables_wanted(const rt_scene* sc, const TraceParams& p) {
    TabsWanted w{false, false, {0, 0, 0}};
    if (!packet_reads_cone_table(p, sc->max_specular > 0.0)) return w;
    auto on = [](const char* name) { return !packet_switch_off(name); };
    w.cone = on("RTAMD_PK_CONE_TAB");
    w.shadow = packet_shadow_table_lights(p) > 0 && on("RTAMD_PK_SHADOW_TAB");
    w.c.shadow_nl = w.shadow ? packet_shadow_table_lights(p) : 0;
    if (w.cone && w.shadow && on("RTAMD_PK_TILE_CLASS"))
        w.c.class_words = on("RTAMD_PK_PLANE_CLEAR") ? 2 : 1;
    // the tile lists serve frame batches that take the fix-up variant, and only those
    if (w.c.has_class() && p.nframes >= 1 &&
        packet_uses_fixup(p, false, sc->max_specular > 0.0) && packet_split_wanted(p))
        w.c.lists = on("RTAMD_PK_TILE_SHADOWED") ? 2 : 1;
    return w;
}

// p's launch shape as a table's layout
TileTabLayout table_layout(const TraceParams& p, const TileTabContents& c) {
    uint32_t gx, gy, waves;
    packet_grid(p, gx, gy, waves);
    return TileTabLayout{static_cast<size_t>(gx) * gy * waves, static_cast<size_t>(gx) * gy, c};
}

// A table's key: everything its words depend on besides the scene and the camera position (the
// cache entry's) — the launch shape (tile_order's fields, the row plan's block and stride as
// words of their own: a collision here would be wrong masks, not another permutation), the
// camera-ray constants dz = (cam.z + focal) − cam.z, W/2 and H/2 bit for bit (the focal length
// is the render call's, not the scene's, so one position may be rendered at several), the
// contents, and for a table with shadow words the render call's bias bit for bit: the words formed
// at one bias are wrong masks at a larger one.
constexpr size_t kConeKeyWords = rt_scene::PkImage::ConeTab::kKeyWords;
void cone_table_key(const TraceParams& p, double dz, const TileTabContents& c,
                    uint32_t (&key)[kConeKeyWords]) {
    uint32_t gx, gy, waves;
    packet_grid(p, gx, gy, waves);
    const uint32_t k[9] = {gx, gy, waves, p.width, p.height, p.rows, p.row0, p.row_block,
                           p.row_stride};
    const double d[3] = {dz, p.half_w, p.half_h};
    std::memset(key, 0, sizeof key);
    std::memcpy(key, k, sizeof k);
    std::memcpy(key + 9, d, sizeof d);
    static_assert(sizeof k + sizeof d + sizeof(uint32_t) + sizeof(double) <=
                      sizeof(uint32_t) * kConeKeyWords, "cone table key");
    // (lights and planes are the scene's, like the spheres: not part of the key)
    key[15] = c.key_word();
    if (c.has_shadow()) std::memcpy(key + 16, &p.bias, sizeof p.bias);
}

// The cached camera's table for p's launch shape: *tab = the existing one (this stream ordered
// after the launch that formed it), or a new entry whose table the caller forms (*fresh) and
// whose event it records; null when the camera's table list is full.
rt_status cone_table_entry(rt_context* ctx, rt_scene::PkImage& im, const TraceParams& p,
                           double dz, const TileTabContents& c,
                           rt_scene::PkImage::ConeTab** tab, bool* fresh) {
    *tab = nullptr;
    *fresh = false;
    uint32_t key[kConeKeyWords];
    cone_table_key(p, dz, c, key);
    for (auto& t : im.tabs) {
        if (std::memcmp(t.key, key, sizeof key) != 0) continue;
        if (!t.done && t.stream != ctx->stream) {
            const hipError_t q = hipEventQuery(t.ready);
            if (q == hipSuccess) t.done = true;
            else if (q == hipErrorNotReady) RT_HIP(hipStreamWaitEvent(ctx->stream, t.ready, 0));
            else return hip_fail(q, "hipEventQuery");
        }
        *tab = &t;
        return RT_OK;
    }
    if (im.tabs.size() >= kMaxConeTabs) return RT_OK;
    // never reallocated: a batch holds entries of earlier frames while adding one
    if (im.tabs.capacity() < kMaxConeTabs) im.tabs.reserve(kMaxConeTabs);
    im.tabs.emplace_back();
    auto& t = im.tabs.back();
    std::memcpy(t.key, key, sizeof key);
    t.stream = ctx->stream;
    hipError_t e = t.buf.ensure(table_layout(p, c).bytes());
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t.ready, hipEventDisableTiming);
    if (e == hipSuccess && c.has_lists()) {
        // (the two words of tile_list_counts_encode)
        e = hipHostMalloc(reinterpret_cast<void**>(&t.counts), 2 * sizeof(unsigned long long));
        if (e == hipSuccess) __atomic_store_n(t.counts, 0ull, __ATOMIC_RELAXED);
        if (e == hipSuccess) __atomic_store_n(t.counts + 1, 0ull, __ATOMIC_RELAXED);
    }
    if (e != hipSuccess) {
        t.buf.release();
        if (t.ready) (void)hipEventDestroy(t.ready);
        im.tabs.pop_back();
        return hip_fail(e, "cone table entry");
    }
    *tab = &t;
    *fresh = true;
    return RT_OK;
}

void cone_table_drop(rt_scene::PkImage& im) {  // the entry cone_table_entry just added
    auto& t = im.tabs.back();
    t.buf.release();
    if (t.ready) (void)hipEventDestroy(t.ready);
    if (t.counts) (void)hipHostFree(t.counts);
    im.tabs.pop_back();
}

// The kernel's three pointers into a table at `words` (null: none is handed over).
void hand_table(const TabsWanted& want, const TileTabLayout& L, const unsigned long long* words,
                const unsigned long long** cone, const unsigned long long** shadow,
                const unsigned long long** cls) {
    *cone = words && want.cone ? words + L.cone(0) : nullptr;
    *shadow = words && want.shadow ? words + L.shadow(0, 0) : nullptr;
    *cls = words && want.c.has_class() ? words + L.cls(0) : nullptr;
}

// One-frame launches with an image entry (p.pk_image set, formed earlier on the stream).
rt_status cone_table_single(rt_context* ctx, const rt_scene* sc, rt_scene::PkImage& im,
                            TraceParams& p) {
    const TabsWanted want = tables_wanted(sc, p);  // (no lists: p.nframes == 0)
    if (!want.any()) return RT_OK;
    rt_scene::PkImage::ConeTab* t = nullptr;
    bool fresh = false;
    const rt_status st = cone_table_entry(ctx, im, p, p.cam_dz, want.c, &t, &fresh);
    if (st != RT_OK || !t) return st;
    if (fresh) {
        PkConeJobs jobs;
        std::memset(&jobs, 0, sizeof jobs);
        jobs.dst[0] = static_cast<unsigned long long*>(t->buf.ptr);
        jobs.frame[0] = -1;
        jobs.n = 1;
        jobs.contents = want.c;
        hipError_t e = launch_packet_cone_tables(p, jobs, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(t->ready, ctx->stream);
        if (e != hipSuccess) {
            cone_table_drop(im);
            return hip_fail(e, "cone table setup");
        }
    }
    hand_table(want, table_layout(p, want.c), static_cast<const unsigned long long*>(t->buf.ptr),
               &p.cone_tab, &p.shadow_tab, &p.class_tab);
    p.plane_masks = want.c.forms_keep() ? 1u : 0u;
    return RT_OK;
}

}  // namespace

// One-frame launches: the cached image; on a camera's second sighting a one-workgroup setup
// launch forms its cache entry; on a first sighting a publish slot.
rt_status packet_image(rt_context* ctx, const rt_scene* sc, TraceParams& p, int flags,
                       rt_scene::PkImage::TileOrder** rec) {
    *rec = nullptr;
    rt_scene::PkImage* found = nullptr;
    rt_status st = packet_image_cached(ctx, sc, p.cam_pos, &found);
    if (st != RT_OK) return st;
    if (found) {
        p.pk_image = static_cast<const double*>(found->buf.ptr);
        st = tile_order(ctx, *found, p, flags, rec);
        return st != RT_OK ? st : cone_table_single(ctx, sc, *found, p);
    }
    if (!packet_second_sighting(sc, p.cam_pos)) {
        const rt_status st2 = packet_publish_slot(ctx, sc, p);
        return st2 != RT_OK ? st2 : scene_tile_order(ctx, sc, p, flags, rec);
    }
    rt_scene::PkImage* im = nullptr;
    st = packet_image_entry(ctx, sc, p.cam_pos, p, &im);
    if (st != RT_OK) return st;
    hipError_t e = launch_packet_image(p, static_cast<double*>(im->buf.ptr), ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(im->ready, ctx->stream);
    if (e != hipSuccess) {
        im->buf.release();
        (void)hipEventDestroy(im->ready);
        sc->pk_images.pop_back();
        return hip_fail(e, "packet image setup");
    }
    p.pk_image = static_cast<const double*>(im->buf.ptr);
    st = tile_order(ctx, *im, p, flags, rec);
    return st != RT_OK ? st : cone_table_single(ctx, sc, *im, p);
}

// A frame batch's image sources (p.fr[f].img for every frame, before the batch launch): a
// cached image, or one formed by ONE small launch for every frame that has none — into a new
// cache entry when the camera was seen before (so a revisited position costs no launch of its
// own), else into the batch's ring slot (an entry of kPkBatchRing, reused once the launches that
// read it have completed).  Frames with the camera of an earlier frame of the batch share its
// image.  The tile order: frame 0's, recorded / built only when every frame has frame 0's
// camera (a static camera), otherwise only an order built earlier for the shape.
rt_status packet_batch_images(rt_context* ctx, const rt_scene* sc, const rt_camera* cams,
                              int nframes, TraceParams& p, int flags,
                              rt_scene::PkImage::TileOrder** rec, int* batch_ring,
                              PkSplit* split) {
    *rec = nullptr;
    *batch_ring = -1;
    *split = PkSplit{0u, 0u, 0u, 0u};
    enum Kind { kCached, kPromote, kRing, kDup };
    Kind kind[kPkMaxBatch];
    int dup_of[kPkMaxBatch];
    rt_scene::PkImage* ent[kPkMaxBatch] = {};
    bool same_cam = true;
    bool any_ring = false;
    const size_t cache_before = sc->pk_images.size();
    // Every error exit after the first promotion drops the entries this call created (newest
    // last): an entry that never received its image, with a `ready` event never recorded, would
    // be taken as a formed image by every later render from that camera position.
    struct Rollback {
        const rt_scene* sc;
        size_t keep;
        bool armed = true;
        ~Rollback() {
            if (!armed) return;
            while (sc->pk_images.size() > keep) {
                auto& im = sc->pk_images.back();
                im.buf.release();
                if (im.ready) (void)hipEventDestroy(im.ready);
                sc->pk_images.pop_back();
            }
        }
    } rollback{sc, cache_before};
    for (int f = 0; f < nframes; ++f) {
        PkFrame& F = p.fr[f];
        for (int i = 0; i < 3; ++i) F.cam[i] = cams[f].position[i];
        // (width, height and focal are the batch's: rt_render_batch checked them)
        const CameraConsts cc = camera_consts(p.width, p.height, F.cam[2], p.focal);
        p.fr_dz[f][0] = cc.dz;
        p.fr_dz[f][1] = cc.dz2;
        F.img = nullptr;
        F.pub = nullptr;
        F.epoch = 0;
        F._pad = 0;
        if (std::memcmp(F.cam, p.fr[0].cam, sizeof F.cam) != 0) same_cam = false;
        int g = 0;
        while (g < f && std::memcmp(p.fr[g].cam, F.cam, sizeof F.cam) != 0) ++g;
        if (g < f) {
            kind[f] = kDup;
            dup_of[f] = g;
            continue;
        }
        rt_status st = packet_image_cached(ctx, sc, F.cam, &ent[f]);
        if (st != RT_OK) return st;
        if (ent[f]) {
            kind[f] = kCached;
            F.img = static_cast<const double*>(ent[f]->buf.ptr);
            continue;
        }
        if (packet_second_sighting(sc, F.cam)) {
            st = packet_image_entry(ctx, sc, F.cam, p, &ent[f]);
            if (st != RT_OK) return st;
            kind[f] = kPromote;
            F.img = static_cast<const double*>(ent[f]->buf.ptr);
            continue;
        }
        kind[f] = kRing;
        any_ring = true;
    }
    const size_t img_doubles = ((packet_lds_bytes(p.ns, p.np, p.nl) + 255) & ~size_t(255)) /
                               sizeof(double);
    double* ring = nullptr;
    if (any_ring) {
        const size_t entry = img_doubles * sizeof(double) * kPkMaxBatch;
        RT_HIP(sc->pk_batch.ensure(entry * rt_scene::kPkBatchRing));
        const int r = sc->pk_batch_next;
        sc->pk_batch_next = (r + 1) % rt_scene::kPkBatchRing;
        if (!sc->pk_batch_done[r])
            RT_HIP(hipEventCreateWithFlags(&sc->pk_batch_done[r], hipEventDisableTiming));
        if (sc->pk_batch_used[r])  // the batch that last read this entry, on any stream
            RT_HIP(hipStreamWaitEvent(ctx->stream, sc->pk_batch_done[r], 0));
        ring = reinterpret_cast<double*>(static_cast<char*>(sc->pk_batch.ptr) +
                                         static_cast<size_t>(r) * entry);
        *batch_ring = r;
    }
    PkImageJobs jobs;
    std::memset(&jobs, 0, sizeof jobs);
    for (int f = 0; f < nframes; ++f) {
        PkFrame& F = p.fr[f];
        if (kind[f] == kRing) F.img = ring + static_cast<size_t>(f) * img_doubles;
        if (kind[f] == kDup) F.img = p.fr[dup_of[f]].img;
        if (kind[f] == kRing || kind[f] == kPromote) {
            jobs.dst[jobs.n] = const_cast<double*>(F.img);
            jobs.frame[jobs.n] = f;
            ++jobs.n;
        }
    }
    hipError_t e = launch_packet_image_batch(p, jobs, ctx->stream);
    for (int f = 0; f < nframes && e == hipSuccess; ++f)
        if (kind[f] == kPromote) e = hipEventRecord(ent[f]->ready, ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "packet batch images");  // the rollback drops them
    rollback.armed = false;  // every promoted entry now has its image and its recorded event
    const rt_status ost = kind[0] == kCached ? tile_order(ctx, *ent[0], p, flags, rec, !same_cam)
                                             : scene_tile_order(ctx, sc, p, flags, rec);
    TabsWanted want = tables_wanted(sc, p);
    if (ost != RT_OK || !want.any()) return ost;
    // A batch with a first-seen camera (a moving camera) forms no lists and stays one launch: the
    // host cannot know its counts before the launch, both grids would have to cover every tile,
    // and the surplus workgroups cost more than the split saves (moving_camera −10 %,
    // profiles/tile_split_ab.txt)
    if (any_ring) want.c.lists = 0;
    // The frames' cone tables, after their images on the stream: a cached or promoted camera's
    // from (or into) its entry, a ring frame's into the ring entry's table buffer up to its
    // cap, a duplicate's shared; every table that does not exist yet by ONE launch.
    const TileTabLayout L = table_layout(p, want.c);
    const uint32_t tiles = static_cast<uint32_t>(L.tiles);
    const size_t tab_bytes = (L.bytes() + 255) & ~size_t(255);
    // (the cap counts the cone words and the class words; the others come on top)
    const size_t cone_bytes =
        (sizeof(unsigned long long) * L.capped_words() + 255) & ~size_t(255);
    char* ring_tab = nullptr;
    size_t ring_room = 0;
    if (any_ring) {
        size_t n_ring = 0;
        for (int f = 0; f < nframes; ++f) n_ring += kind[f] == kRing;
        const size_t fit = std::min(n_ring, kConeRingBytes / cone_bytes);
        auto& buf = sc->pk_batch_tab[*batch_ring];
        if (fit > 0 && buf.bytes < fit * tab_bytes) {
            // the stream already waits for the batch that last read this ring entry; freeing
            // its table buffer needs that batch complete on the host's side too
            if (sc->pk_batch_used[*batch_ring])
                RT_HIP(hipEventSynchronize(sc->pk_batch_done[*batch_ring]));
            RT_HIP(buf.ensure(fit * tab_bytes));
        }
        ring_tab = static_cast<char*>(buf.ptr);
        ring_room = fit;
    }
    PkConeJobs cj;
    std::memset(&cj, 0, sizeof cj);
    cj.contents = want.c;
    PkListCounts lc;
    std::memset(&lc, 0, sizeof lc);
    // a frame's list counts where the host has them (a cache entry's table formed earlier); a
    // table formed by this call's launch has none yet, and its batch stays one launch
    TileListCounts most{0u, 0u, 0u};
    bool all_lists = want.c.has_lists();
    auto count_frame = [&](const unsigned long long* host) {
        const unsigned long long v[2] = {host ? __atomic_load_n(host, __ATOMIC_RELAXED) : 0ull,
                                         host ? __atomic_load_n(host + 1, __ATOMIC_RELAXED) : 0ull};
        TileListCounts n;
        if (!tile_list_counts_decode(v, &n)) all_lists = false;
        else most = TileListCounts{std::max(most.uniform, n.uniform),
                                   std::max(most.general, n.general),
                                   std::max(most.shadowed, n.shadowed)};
    };
    p.plane_masks = want.c.forms_keep() ? 1u : 0u;
    // the kernel's pointers of a frame whose table is (or will be) at `words`
    auto hand = [&](int f, const unsigned long long* words) {
        hand_table(want, L, words, &p.fr_tab[f], &p.fr_stab[f], &p.fr_ctab[f]);
    };
    rt_scene::PkImage* made[kPkMaxBatch];  // entries that got a fresh table (newest last)
    rt_scene::PkImage::ConeTab* made_tab[kPkMaxBatch];
    int n_made = 0;
    rt_status st = RT_OK;
    for (int f = 0; f < nframes && st == RT_OK; ++f) {
        hand(f, nullptr);
        unsigned long long* dst = nullptr;
        if (kind[f] == kDup) {
            p.fr_tab[f] = p.fr_tab[dup_of[f]];
            p.fr_stab[f] = p.fr_stab[dup_of[f]];
            p.fr_ctab[f] = p.fr_ctab[dup_of[f]];
            continue;
        }
        if (kind[f] == kRing) {
            if (ring_room == 0) all_lists = false;
            if (ring_room == 0) continue;  // past the cap: the wave forms its own mask
            --ring_room;
            dst = reinterpret_cast<unsigned long long*>(ring_tab);
            ring_tab += tab_bytes;
        } else {
            rt_scene::PkImage::ConeTab* t = nullptr;
            bool fresh = false;
            st = cone_table_entry(ctx, *ent[f], p, p.fr_dz[f][0], want.c, &t, &fresh);
            if (st != RT_OK || !t) all_lists = false;
            if (st != RT_OK || !t) continue;
            hand(f, static_cast<const unsigned long long*>(t->buf.ptr));
            if (!fresh) count_frame(t->counts);
            if (!fresh) continue;
            lc.host[cj.n] = t->counts;
            made[n_made] = ent[f];
            made_tab[n_made] = t;
            ++n_made;
            dst = static_cast<unsigned long long*>(t->buf.ptr);
        }
        hand(f, dst);
        count_frame(nullptr);  // formed by this call's launch: not known yet
        cj.dst[cj.n] = dst;
        cj.frame[cj.n] = f;
        ++cj.n;
    }
    if (st == RT_OK) {
        hipError_t ce = launch_packet_cone_tables(p, cj, ctx->stream, &lc);
        for (int i = 0; i < n_made && ce == hipSuccess; ++i)
            ce = hipEventRecord(made_tab[i]->ready, ctx->stream);
        if (ce != hipSuccess) st = hip_fail(ce, "packet batch cone tables");
    }
    if (st != RT_OK)  // a table never formed must not be found by a later render
        for (int i = n_made - 1; i >= 0; --i) cone_table_drop(*made[i]);
    if (st == RT_OK && all_lists) {  // every frame has its lists: the split launch
        *split = PkSplit{tiles, most.uniform, most.general,
                         want.c.forms_mark() ? most.shadowed : 0u};
    }
    return st;
}

}  // namespace rtamd
