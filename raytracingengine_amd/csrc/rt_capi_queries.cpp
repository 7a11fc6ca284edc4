// rt_capi_queries.cpp — the batch query entries of include/rt_capi.h: rays, points or a camera in,
// one answer array or a record of selectable outputs back.  Every query is written once, as an
// enqueue_X on device pointers; its _device entry is checks -> params -> enqueue_X, its host entry
// checks -> params -> stage -> enqueue_X -> download through the context's staging buffer
// (ctx->rays, laid out by rt_stage.hpp).  Host entries synchronise the context's stream before
// they return; _device entries neither synchronise nor allocate.
#include "rt_capi.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rt_context.hpp"
#include "rt_internal.hpp"
#include "rt_stage.hpp"

#pragma clang fp contract(off)

using namespace rtamd;

namespace {

// ---- staging ---------------------------------------------------------------------------------
// One output of a record of selectable outputs (rt_direct_light_out, rt_scatter_out,
// rt_closest_out), in the record's bit order: what check_outputs, the staging and the conversion
// to the kernels' record know about it.
template <class Rec>
struct OutField {
    int bit;
    size_t bytes;  // per ray
    void* Rec::*member;
};

// The items of one host entry in ctx->rays: declare them, upload(), take the device pointers,
// enqueue, finish().
class Stage {
public:
    explicit Stage(rt_context* ctx) : ctx_(ctx) {}
    int in(const void* host, size_t bytes) { return plan_.input(host, bytes); }
    int out(void* host, size_t bytes, size_t align = 8) { return plan_.output(host, bytes, align); }
    int inout(void* host, size_t bytes, bool read, size_t align = 8) {
        return plan_.inout(host, bytes, read, align);
    }
    // The requested outputs of `host` for n rays; the first one's item (the others follow).
    template <class Rec, size_t N>
    int outs(const OutField<Rec> (&tab)[N], int outputs, const Rec& host, size_t n) {
        const int first = plan_.count;
        for (const auto& f : tab) {
            const bool on = outputs & f.bit;
            out(on ? host.*f.member : nullptr, on ? n * f.bytes : 0, f.bytes % 8 ? 1 : 8);
        }
        return first;
    }
    // Lays the items out, grows ctx->rays to their total and enqueues the inputs' copies.
    rt_status upload() {
        RT_HIP(ctx_->rays.ensure(plan_.layout()));
        for (int i = 0; i < plan_.count; ++i)
            if (const StageItem& it = plan_.item[i]; it.src && it.bytes)
                RT_HIP(hipMemcpyAsync(at(i), it.src, it.bytes, hipMemcpyHostToDevice,
                                      ctx_->stream));
        return RT_OK;
    }
    // The device array of item i; null for an item without bytes (an output not requested).
    void* at(int i) const {
        const StageItem& it = plan_.item[i];
        return it.bytes ? static_cast<char*>(ctx_->rays.ptr) + it.offset : nullptr;
    }
    // The device record of the outputs declared by outs() at `first`.
    template <class Rec, size_t N>
    Rec outs_at(const OutField<Rec> (&tab)[N], int first) const {
        Rec d{};
        for (size_t k = 0; k < N; ++k) d.*tab[k].member = at(first + static_cast<int>(k));
        return d;
    }
    // Enqueues the outputs' copies to the host.
    rt_status download() {
        for (int i = 0; i < plan_.count; ++i)
            if (const StageItem& it = plan_.item[i]; it.dst && it.bytes)
                RT_HIP(hipMemcpyAsync(it.dst, at(i), it.bytes, hipMemcpyDeviceToHost,
                                      ctx_->stream));
        return RT_OK;
    }
    rt_status sync() {
        RT_HIP(hipStreamSynchronize(ctx_->stream));
        return RT_OK;
    }
    rt_status finish() {
        RT_TRY(download());
        return sync();
    }

private:
    rt_context* ctx_;
    StagePlan plan_;
};

// ---- records of selectable outputs -----------------------------------------------------------
using DlRec = rt_direct_light_out;
using ScRec = rt_scatter_out;
using ChRec = rt_closest_out;
constexpr OutField<DlRec> kDlOut[] = {{RT_DL_RADIANCE, 24, &DlRec::radiance},
                                      {RT_DL_DIFFUSE, 24, &DlRec::diffuse},
                                      {RT_DL_SPECULAR, 24, &DlRec::specular}};
constexpr OutField<ScRec> kScOut[] = {{RT_SC_VALUE, 24, &ScRec::value},
                                      {RT_SC_REFRACT, 48, &ScRec::refract_rays},
                                      {RT_SC_REFLECT, 48, &ScRec::reflect_rays},
                                      {RT_SC_WEIGHTS, 16, &ScRec::weights},
                                      {RT_SC_FLAGS, 1, &ScRec::flags}};
constexpr OutField<ChRec> kChOut[] = {{RT_CH_T, 8, &ChRec::t},
                                      {RT_CH_PRIM, 8, &ChRec::prim},
                                      {RT_CH_NORMAL, 24, &ChRec::normal},
                                      {RT_CH_POINT, 24, &ChRec::point},
                                      {RT_CH_MATERIAL, 56, &ChRec::material}};
constexpr size_t kRayBytes = 6 * sizeof(double);  // {o, d}; a point of the light queries: {p, n}

// The argument checks of the entries with an output record, made before anything touches a
// device; `entry` ends every message.  inputs_ok: no input pointer is NULL, or n == 0;
// materials_ok: n_materials is n or 1, or n == 0 (for the entry that takes materials).
template <class Rec, size_t N>
rt_status check_outputs(const OutField<Rec> (&tab)[N], int outputs, const Rec* out, bool inputs_ok,
                        const rt_context* ctx, const char* entry, bool materials_ok = true) {
    const std::string name(entry);
    int all = 0;
    for (const auto& f : tab) all |= f.bit;
    if (outputs == 0) return fail(RT_ERR_INVALID_ARG, "no output requested from " + name);
    if (outputs & ~all) return fail(RT_ERR_INVALID_ARG, "unknown output bit passed to " + name);
    if (!out) return fail(RT_ERR_INVALID_ARG, "NULL output record passed to " + name);
    for (const auto& f : tab)
        if ((outputs & f.bit) && !(out->*f.member))
            return fail(RT_ERR_INVALID_ARG, "NULL pointer of a requested output passed to " + name);
    if (!inputs_ok) return fail(RT_ERR_INVALID_ARG, "NULL argument to " + name);
    if (!materials_ok) return fail(RT_ERR_INVALID_ARG, "n_materials must be n or 1 in " + name);
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "NULL context passed to " + name);
    return RT_OK;
}

// `o` with the pointers of the outputs that were not requested set to null: they are never read
// further and never handed to a kernel.
template <class Rec, size_t N>
Rec requested(const OutField<Rec> (&tab)[N], int outputs, Rec o) {
    for (const auto& f : tab)
        if (!(outputs & f.bit)) o.*f.member = nullptr;
    return o;
}

// ---- launch parameters -----------------------------------------------------------------------
// The members of opts a query reads; whatever else the caller left there neither fails nor
// steers it.
enum : unsigned {
    kReadNoBvh = 1,      // flags & RT_FLAG_NO_BVH
    kReadBias = 2,       // bias
    kReadRecursion = 4,  // the sign of max_recursion: 0 is "at the recursion limit"
    kReadAll = 8,        // everything but the row range (rt_trace_rays)
    kReadSeed = 16,      // seed (the keyed entries: the area light's draws)
};

struct QueryParams {
    TraceParams p;
    int path;     // which TraceRay shape the scene can produce (build_params)
    bool opaque;  // no material is transparent, so the kernels' occlusion_opaque variant serves
                  // the scene; RTAMD_TX_OPAQUE=0 (read per call) sends it through the march alone
};

// build_params for a query: its scene and opts part, with a 1x1 camera.  Fails on a NULL or
// foreign scene.
rt_status query_params(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                       unsigned which, QueryParams& q) {
    rt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.width = cam.height = 1;
    cam.aa_samples = 1;
    rt_render_opts o;
    rt_render_opts_default(&o);
    if (opts && (which & kReadAll)) o = *opts;
    if (opts && (which & kReadNoBvh)) o.flags = opts->flags & RT_FLAG_NO_BVH;
    if (opts && (which & kReadBias)) o.bias = opts->bias;
    if (opts && (which & kReadSeed)) o.seed = opts->seed;
    o.row_begin = o.row_end = 0;
    bool lds;
    size_t lds_bytes;
    uint32_t rows;
    RT_TRY(build_params(ctx, sc, &cam, &o, q.p, q.path, lds, lds_bytes, rows));
    if (which & kReadRecursion) q.p.max_rec = (opts && opts->max_recursion <= 0) ? 0 : 1;
    const char* e = std::getenv("RTAMD_TX_OPAQUE");
    q.opaque = !sc->any_transparent && !(e && std::atoi(e) == 0);
    return RT_OK;
}

void copy_row_set(const rt_render_opts& from, rt_render_opts& o) {
    o.seed = from.seed;
    o.row_begin = from.row_begin;
    o.row_end = from.row_end;
    o.row_block = from.row_block;
    o.row_cycle = from.row_cycle;
}

// ---- the keys of the area light's draws (the _keyed entries) -----------------------------------
// What an entry of a per-level query does about the keys.  An un-keyed entry has none: nothing is
// checked or staged, opts->seed is not read and the launch gets a null pointer.
struct EntryKeys {
    bool keyed;
    rt_area_keys k{nullptr, 0, 0};  // *keys, or {NULL, 0, 0} for NULL
    AreaKeyArgs dk{};

    // Checked before anything touches a device.
    rt_status check(const rt_area_keys* keys, const char* entry) {
        if (!keyed) return RT_OK;
        if (keys) k = *keys;
        if (k.depth > 63)  // the streams of neighbouring samples would collide
            return fail(RT_ERR_INVALID_ARG, "keys->depth " + std::to_string(k.depth) +
                                                " above 63 passed to " + entry);
        if (k.sample > 0x00FFFFFFu)  // the stream is 32 bits
            return fail(RT_ERR_INVALID_ARG, "keys->sample " + std::to_string(k.sample) +
                                                " above 0x00FFFFFF passed to " + entry);
        return RT_OK;
    }
    // The members of opts the query reads: `base`, and the seed of the draws.
    unsigned reads(unsigned base) const { return base | (keyed ? kReadSeed : 0u); }
    // The pixel keys as one more staged input of a host entry, when given.
    int stage(Stage& s, size_t n) const {
        return s.in(k.pixel, k.pixel ? n * sizeof(uint64_t) : 0);
    }
    // The kernels' record with the pixel keys at d_pixel (device memory, or NULL).
    const AreaKeyArgs* device(const void* d_pixel) {
        dk = AreaKeyArgs{static_cast<const unsigned long long*>(d_pixel), k.sample, k.depth};
        return keyed ? &dk : nullptr;
    }
};

constexpr unsigned kReadLevel = kReadNoBvh | kReadBias;  // what every per-level query reads

const double* f64(const void* p) { return static_cast<const double*>(p); }
double* f64(void* p) { return static_cast<double*>(p); }

// ---- the queries, each on device pointers ------------------------------------------------------
rt_status enqueue_trace_rays(rt_context* ctx, const QueryParams& q, bool count, const void* rays,
                             size_t n, void* rgb) {
    RT_HIP(launch_trace_rays(q.p, q.path, count, f64(rays), n, f64(rgb), ctx->stream));
    return RT_OK;
}

rt_status enqueue_intersect(rt_context* ctx, const QueryParams& q, const void* rays, size_t n,
                            void* hits) {
    RT_HIP(launch_intersect_rays(q.p, f64(rays), n, f64(hits), ctx->stream));
    return RT_OK;
}

rt_status enqueue_occluded(rt_context* ctx, const QueryParams& q, const void* rays,
                           const void* max_dist, size_t n, void* occluded) {
    RT_HIP(launch_occluded_rays(q.p, f64(rays), f64(max_dist), n, static_cast<uint8_t*>(occluded),
                                ctx->stream));
    return RT_OK;
}

rt_status enqueue_transmittance(rt_context* ctx, const QueryParams& q, const void* rays,
                                const void* max_dist, size_t n, void* T) {
    RT_HIP(launch_transmittance_rays(q.p, q.opaque, f64(rays), f64(max_dist), n, f64(T),
                                     ctx->stream));
    return RT_OK;
}

// keys (here and in the three queries below): the _keyed entries', or nullptr for the un-keyed
// ones; which kernel answers is the launch's matter (rt_internal.hpp).
rt_status enqueue_light_transmittance(rt_context* ctx, const QueryParams& q, const void* points,
                                      size_t n, void* T, const AreaKeyArgs* keys) {
    RT_HIP(launch_light_transmittance(q.p, q.opaque, f64(points), keys, n, f64(T), ctx->stream));
    return RT_OK;
}

// Columns of the light-transmittance table: the point lights, and for a keyed query the area
// light's samples after them.
size_t light_columns(const QueryParams& q, bool keyed) {
    return static_cast<size_t>(q.p.nl) + (keyed ? static_cast<size_t>(q.p.al_samples) : 0);
}

DlOut dl_out(const rt_direct_light_out& o) {
    return DlOut{f64(o.radiance), f64(o.diffuse), f64(o.specular)};
}

static_assert(sizeof(rt_material) == 7 * sizeof(double), "rt_material is not seven packed doubles");

// materials: n device records, or with shared_material one host record for all points, read now
// and passed in the kernel arguments (rt_capi.h).
rt_status enqueue_direct_light(rt_context* ctx, const QueryParams& q, const void* points,
                               const void* materials, const void* shared_material, size_t n,
                               const rt_direct_light_out& out, const AreaKeyArgs* keys) {
    DlMaterial s{};
    if (shared_material) std::memcpy(s.v, shared_material, sizeof(rt_material));
    RT_HIP(launch_direct_light_points(q.p, q.opaque, f64(points),
                                      shared_material ? nullptr : f64(materials), s, keys, n,
                                      dl_out(out), ctx->stream));
    return RT_OK;
}

rt_status enqueue_direct_light_rays(rt_context* ctx, const QueryParams& q, const void* rays,
                                    size_t n, const rt_direct_light_out& out,
                                    const AreaKeyArgs* keys) {
    RT_HIP(launch_direct_light_rays(q.p, q.opaque, f64(rays), keys, n, dl_out(out), ctx->stream));
    return RT_OK;
}

rt_status enqueue_scatter(rt_context* ctx, const QueryParams& q, const void* rays, size_t n,
                          const rt_scatter_out& o, const AreaKeyArgs* keys) {
    const ScOut out{f64(o.value), f64(o.refract_rays), f64(o.reflect_rays), f64(o.weights),
                    static_cast<uint8_t*>(o.flags)};
    RT_HIP(launch_scatter_rays(q.p, q.opaque, f64(rays), keys, n, out, ctx->stream));
    return RT_OK;
}

rt_status enqueue_closest(rt_context* ctx, const QueryParams& q, const void* rays, size_t n,
                          const rt_closest_out& o) {
    const ChOut out{f64(o.t), static_cast<int32_t*>(o.prim), f64(o.normal), f64(o.point),
                    f64(o.material)};
    RT_HIP(launch_closest_rays(q.p, f64(rays), n, out, ctx->stream));
    return RT_OK;
}

rt_status enqueue_camera_rays(rt_context* ctx, const TraceParams& p, int sample, void* rays) {
    RT_HIP(launch_camera_rays(p, sample, f64(rays), ctx->stream));
    return RT_OK;
}

rt_status enqueue_accumulate(rt_context* ctx, const QueryParams& q, int s0, int s1, void* sum) {
    RT_HIP(launch_accumulate_samples(q.p, q.path, s0, s1, f64(sum), ctx->stream));
    return RT_OK;
}

rt_status enqueue_resolve(rt_context* ctx, const void* sum, size_t n, int samples, int tonemap,
                          void* hdr64, void* hdr32, void* ldr) {
    RT_HIP(launch_resolve(f64(sum), n, samples, tonemap, f64(hdr64), static_cast<float*>(hdr32),
                          static_cast<uint8_t*>(ldr), ctx->stream));
    return RT_OK;
}

// RTAMD_ADAPT_LIST=0 (read per call) keeps every pixel in the tile kernel; otherwise the call
// uses the context's list, scratch like the fix-up list (scratch_wait / scratch_done).
rt_status enqueue_adaptive(rt_context* ctx, const QueryParams& q, const rt_adaptive_rule& rule,
                           int fresh, int sample_end, void* sum, void* moments, void* count) {
    AdaptiveArgs a{};
    a.tolerance = rule.tolerance;
    a.lum_floor = rule.lum_floor;
    a.min_samples = rule.min_samples;
    a.sample_end = sample_end;
    a.fresh = fresh != 0;
    a.sum = f64(sum);
    a.moments = f64(moments);
    a.count = static_cast<int32_t*>(count);
    const char* e = std::getenv("RTAMD_ADAPT_LIST");
    const bool listing = !(e && std::atoi(e) == 0);
    if (listing) {
        RT_TRY(scratch_wait(ctx));
        RT_TRY(adaptive_buffers(ctx, static_cast<size_t>(q.p.rows) * q.p.width, a));
    }
    ctx->adapt_listing = listing;
    RT_HIP(launch_accumulate_adaptive(q.p, q.path, a, ctx->stream));
    return listing ? scratch_done(ctx) : RT_OK;
}

rt_status enqueue_resolve_counts(rt_context* ctx, const void* sum, const void* count, size_t n,
                                 int tonemap, void* hdr64, void* hdr32, void* ldr) {
    RT_HIP(launch_resolve_counts(f64(sum), static_cast<const int32_t*>(count), n, tonemap,
                                 f64(hdr64), static_cast<float*>(hdr32),
                                 static_cast<uint8_t*>(ldr), ctx->stream));
    return RT_OK;
}

// ---- argument checks and parameters of the camera entries -------------------------------------
// The argument checks of the two camera-ray entries and the camera part of build_params: no scene
// is involved, and of opts only the row set and the seed are read.
rt_status camera_rays_params(const rt_context* ctx, const rt_camera* cam,
                             const rt_render_opts* opts, int sample, const void* out,
                             const char* entry, TraceParams& p) {
    const std::string name(entry);
    if (!ctx || !cam || !out) return fail(RT_ERR_INVALID_ARG, "NULL argument to " + name);
    if (cam->width == 0 || cam->height == 0)
        return fail(RT_ERR_INVALID_ARG, "zero camera width or height passed to " + name);
    if (static_cast<uint64_t>(cam->width) * cam->height > (1ull << 31))
        return fail(RT_ERR_UNSUPPORTED, "image larger than 2^31 pixels passed to " + name);
    if (sample < 0 || sample >= std::max(1, cam->aa_samples))
        return fail(RT_ERR_INVALID_ARG, "sample " + std::to_string(sample) +
                                            " outside [0, max(1, aa_samples)) passed to " + name);
    rt_render_opts o;
    rt_render_opts_default(&o);
    if (opts) copy_row_set(*opts, o);
    RT_TRY(check_row_set(o, cam->height, " passed to " + name));
    std::memset(&p, 0, sizeof p);
    for (int i = 0; i < 3; ++i) p.cam_pos[i] = cam->position[i];
    p.focal = cam->focal;
    p.width = cam->width;
    p.height = cam->height;
    p.aa = cam->aa_samples;
    p.seed = o.seed;
    set_row_set(o, cam->height, p);
    return RT_OK;
}

// What the entries that continue a sum (accumulate, adaptive) do after their own argument checks:
// the row set, checked before the context or the scene is dereferenced, then build_params with
// the members of opts the call reads: the kernel selection (path) and the RT_ERR_UNSUPPORTED of
// rt_trace_rays for the scene and opts.  name: the entry's, ends every message.
rt_status sum_params(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                     const rt_render_opts* opts, const std::string& name, QueryParams& q) {
    rt_render_opts o;
    rt_render_opts_default(&o);
    if (opts) {
        copy_row_set(*opts, o);
        o.max_recursion = opts->max_recursion;
        o.bias = opts->bias;
        o.flags = opts->flags & RT_FLAG_NO_BVH;
    }
    o.tonemap = RT_TONEMAP_NONE;
    RT_TRY(check_row_set(o, cam->height, " passed to " + name));
    bool lds;
    size_t lds_bytes;
    uint32_t rows;
    const rt_status st = build_params(ctx, sc, cam, &o, q.p, q.path, lds, lds_bytes, rows);
    if (st != RT_OK) return fail(st, std::string(rt_last_error()) + ", passed to " + name);
    return RT_OK;
}

// The argument checks of the two accumulate entries, made before the context or the scene is
// dereferenced, then sum_params.
rt_status accumulate_params(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                            const rt_render_opts* opts, int s0, int s1, const void* sum,
                            const char* entry, QueryParams& q) {
    const std::string name(entry);
    if (!ctx || !sc || !cam || !sum) return fail(RT_ERR_INVALID_ARG, "NULL argument to " + name);
    if (cam->width == 0 || cam->height == 0)
        return fail(RT_ERR_INVALID_ARG, "zero camera width or height passed to " + name);
    if (s0 < 0 || s0 >= s1 || s1 > std::max(1, cam->aa_samples))
        return fail(RT_ERR_INVALID_ARG, "sample range [" + std::to_string(s0) + "," +
                                            std::to_string(s1) +
                                            ") empty or outside [0, max(1, aa_samples)] passed to " +
                                            name);
    return sum_params(ctx, sc, cam, opts, name, q);
}

// The argument checks of the two adaptive entries, in the same place, then sum_params.
rt_status adaptive_params(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                          const rt_render_opts* opts, const rt_adaptive_rule* rule, int sample_end,
                          const void* sum, const void* moments, const void* count,
                          const char* entry, QueryParams& q) {
    const std::string name(entry);
    if (!ctx || !sc || !cam || !rule || !sum || !moments || !count)
        return fail(RT_ERR_INVALID_ARG, "NULL argument to " + name);
    if (cam->width == 0 || cam->height == 0)
        return fail(RT_ERR_INVALID_ARG, "zero camera width or height passed to " + name);
    if (sample_end < 1 || sample_end > std::max(1, cam->aa_samples))
        return fail(RT_ERR_INVALID_ARG, "sample_end " + std::to_string(sample_end) +
                                            " outside [1, max(1, aa_samples)] passed to " + name);
    if (rule->min_samples < 2)
        return fail(RT_ERR_INVALID_ARG, "rule->min_samples " + std::to_string(rule->min_samples) +
                                            " < 2 passed to " + name);
    if (!(rule->tolerance >= 0.0))
        return fail(RT_ERR_INVALID_ARG, "rule->tolerance negative or NaN passed to " + name);
    if (!(rule->lum_floor > 0.0))
        return fail(RT_ERR_INVALID_ARG, "rule->lum_floor not above 0 passed to " + name);
    return sum_params(ctx, sc, cam, opts, name, q);
}

// The checks of the resolve entries, before the context is dereferenced.  count_missing: the
// entry divides by per-pixel counts (samples is then 1) and was given none.
rt_status check_resolve_args(const rt_context* ctx, const void* sum, size_t n, int samples,
                             int tonemap, const void* hdr64, const void* hdr32, const void* ldr,
                             const char* entry, bool count_missing = false) {
    const std::string name(entry);
    if (samples < 1)
        return fail(RT_ERR_INVALID_ARG, "samples " + std::to_string(samples) + " < 1 passed to " + name);
    if (tonemap < RT_TONEMAP_NONE || tonemap > RT_TONEMAP_COUNT)
        return fail(RT_ERR_INVALID_ARG, "unknown tonemap operator passed to " + name);
    if (!hdr64 && !hdr32 && !ldr) return fail(RT_ERR_INVALID_ARG, "no output passed to " + name);
    if (ldr && tonemap == RT_TONEMAP_NONE)
        return fail(RT_ERR_INVALID_ARG, "bytes requested with RT_TONEMAP_NONE from " + name);
    if (!sum && n > 0) return fail(RT_ERR_INVALID_ARG, "NULL sum passed to " + name);
    if (count_missing && n > 0) return fail(RT_ERR_INVALID_ARG, "NULL count passed to " + name);
    if (!ctx) return fail(RT_ERR_INVALID_ARG, "NULL context passed to " + name);
    return RT_OK;
}

// ---- the four per-level queries: each form once ------------------------------------------------
// keyed: the call came through the _keyed entry; `entry` is the called entry's name and ends
// every message.  The light query builds its parameters before the n == 0 return (a NULL or
// foreign scene fails it even then); with no columns nothing is written and there is no output
// to point to: a NULL one is accepted.  The others return RT_OK for n == 0 before the scene or a
// device is touched; with n_materials == 1 the material is a host record, for both forms.
rt_status light_transmittance_device(rt_context* ctx, const rt_scene* sc,
                                     const rt_render_opts* opts, const void* d_points, size_t n,
                                     void* d_T, const rt_area_keys* keys, bool keyed,
                                     const char* entry) {
    EntryKeys K{keyed};
    RT_TRY(K.check(keys, entry));
    const std::string null_arg = std::string("NULL argument to ") + entry;
    if (!ctx || (n && !d_points)) return fail(RT_ERR_INVALID_ARG, null_arg);
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, K.reads(kReadLevel), q));
    if (n == 0 || light_columns(q, K.keyed) == 0) return RT_OK;
    if (!d_T) return fail(RT_ERR_INVALID_ARG, null_arg);
    return enqueue_light_transmittance(ctx, q, d_points, n, d_T, K.device(K.k.pixel));
}

rt_status light_transmittance_host(rt_context* ctx, const rt_scene* sc,
                                   const rt_render_opts* opts, const double* points, size_t n,
                                   double* T_out, const rt_area_keys* keys, bool keyed,
                                   const char* entry) {
    EntryKeys K{keyed};
    RT_TRY(K.check(keys, entry));
    const std::string null_arg = std::string("NULL argument to ") + entry;
    if (!ctx || (n && !points)) return fail(RT_ERR_INVALID_ARG, null_arg);
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, K.reads(kReadLevel), q));
    const size_t cols = light_columns(q, K.keyed);
    if (n == 0 || cols == 0) return RT_OK;
    if (!T_out) return fail(RT_ERR_INVALID_ARG, null_arg);
    Stage s(ctx);
    const int i_pts = s.in(points, n * kRayBytes), i_key = K.stage(s, n),
              i_out = s.out(T_out, n * cols * sizeof(double));
    RT_TRY(s.upload());
    RT_TRY(enqueue_light_transmittance(ctx, q, s.at(i_pts), n, s.at(i_out),
                                       K.device(s.at(i_key))));
    return s.finish();
}

rt_status direct_light_device(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                              const void* d_points, const void* d_materials, size_t n_materials,
                              size_t n, int outputs, const rt_direct_light_out* d_out,
                              const rt_area_keys* keys, bool keyed, const char* entry) {
    EntryKeys K{keyed};
    RT_TRY(K.check(keys, entry));
    RT_TRY(check_outputs(kDlOut, outputs, d_out, !n || (d_points && d_materials), ctx, entry,
                         !n || n_materials == n || n_materials == 1));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, K.reads(kReadLevel), q));
    return enqueue_direct_light(ctx, q, d_points, d_materials,
                                n_materials == 1 ? d_materials : nullptr, n,
                                requested(kDlOut, outputs, *d_out), K.device(K.k.pixel));
}

rt_status direct_light_host(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                            const double* points, const rt_material* materials,
                            size_t n_materials, size_t n, int outputs,
                            const rt_direct_light_out* out, const rt_area_keys* keys, bool keyed,
                            const char* entry) {
    EntryKeys K{keyed};
    RT_TRY(K.check(keys, entry));
    RT_TRY(check_outputs(kDlOut, outputs, out, !n || (points && materials), ctx, entry,
                         !n || n_materials == n || n_materials == 1));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, K.reads(kReadLevel), q));
    const bool shared = n_materials == 1;
    Stage s(ctx);
    const int i_pts = s.in(points, n * 9 * sizeof(double)),
              i_mat = s.in(materials, shared ? 0 : n * sizeof(rt_material)),
              i_key = K.stage(s, n), i_out = s.outs(kDlOut, outputs, *out, n);
    RT_TRY(s.upload());
    RT_TRY(enqueue_direct_light(ctx, q, s.at(i_pts), s.at(i_mat), shared ? materials : nullptr, n,
                                s.outs_at(kDlOut, i_out), K.device(s.at(i_key))));
    return s.finish();
}

rt_status direct_light_rays_device(rt_context* ctx, const rt_scene* sc,
                                   const rt_render_opts* opts, const void* d_rays, size_t n,
                                   int outputs, const rt_direct_light_out* d_out,
                                   const rt_area_keys* keys, bool keyed, const char* entry) {
    EntryKeys K{keyed};
    RT_TRY(K.check(keys, entry));
    RT_TRY(check_outputs(kDlOut, outputs, d_out, !n || d_rays, ctx, entry));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, K.reads(kReadLevel), q));
    return enqueue_direct_light_rays(ctx, q, d_rays, n, requested(kDlOut, outputs, *d_out),
                                     K.device(K.k.pixel));
}

rt_status direct_light_rays_host(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                                 const double* rays, size_t n, int outputs,
                                 const rt_direct_light_out* out, const rt_area_keys* keys,
                                 bool keyed, const char* entry) {
    EntryKeys K{keyed};
    RT_TRY(K.check(keys, entry));
    RT_TRY(check_outputs(kDlOut, outputs, out, !n || rays, ctx, entry));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, K.reads(kReadLevel), q));
    Stage s(ctx);
    const int i_rays = s.in(rays, n * kRayBytes), i_key = K.stage(s, n),
              i_out = s.outs(kDlOut, outputs, *out, n);
    RT_TRY(s.upload());
    RT_TRY(enqueue_direct_light_rays(ctx, q, s.at(i_rays), n, s.outs_at(kDlOut, i_out),
                                     K.device(s.at(i_key))));
    return s.finish();
}

rt_status scatter_rays_device(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                              const void* d_rays, size_t n, int outputs,
                              const rt_scatter_out* d_out, const rt_area_keys* keys, bool keyed,
                              const char* entry) {
    EntryKeys K{keyed};
    RT_TRY(K.check(keys, entry));
    RT_TRY(check_outputs(kScOut, outputs, d_out, !n || d_rays, ctx, entry));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, K.reads(kReadLevel | kReadRecursion), q));
    return enqueue_scatter(ctx, q, d_rays, n, requested(kScOut, outputs, *d_out),
                           K.device(K.k.pixel));
}

rt_status scatter_rays_host(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                            const double* rays, size_t n, int outputs, const rt_scatter_out* out,
                            const rt_area_keys* keys, bool keyed, const char* entry) {
    EntryKeys K{keyed};
    RT_TRY(K.check(keys, entry));
    RT_TRY(check_outputs(kScOut, outputs, out, !n || rays, ctx, entry));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, K.reads(kReadLevel | kReadRecursion), q));
    Stage s(ctx);
    const int i_rays = s.in(rays, n * kRayBytes), i_key = K.stage(s, n),
              i_out = s.outs(kScOut, outputs, *out, n);
    RT_TRY(s.upload());
    RT_TRY(enqueue_scatter(ctx, q, s.at(i_rays), n, s.outs_at(kScOut, i_out),
                           K.device(s.at(i_key))));
    return s.finish();
}

}  // namespace

extern "C" {

// ---- TraceRay and IntersectClosest (rt_trace.hip) ---------------------------------------------
// These, the any-hit and the transmittance entries build their parameters before the n == 0
// return: a NULL or foreign scene fails them even then.
rt_status rt_trace_rays_device(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                               const void* d_rays, size_t n, void* d_rgb) {
    if (!ctx || (n && (!d_rays || !d_rgb)))
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_trace_rays_device");
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, kReadAll, q));
    return n ? enqueue_trace_rays(ctx, q, false, d_rays, n, d_rgb) : RT_OK;
}

rt_status rt_trace_rays(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                        const double* rays, size_t n, double* rgb, rt_stats* stats) {
    if (!ctx || (n && (!rays || !rgb)))
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_trace_rays");
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, kReadAll, q));
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return RT_OK;
    Stage s(ctx);
    const int i_rays = s.in(rays, n * kRayBytes), i_rgb = s.out(rgb, n * 3 * sizeof(double));
    RT_TRY(s.upload());
    RT_TRY(enqueue_trace_rays(ctx, q, false, s.at(i_rays), n, s.at(i_rgb)));
    RT_TRY(s.download());
    unsigned long long c[2] = {0, 0};
    if (stats) {  // the counting pass: the same trace with wave-reduced atomics
        q.p.counters = static_cast<unsigned long long*>(ctx->counters.ptr);
        RT_TRY(scratch_wait(ctx));
        RT_TRY(counters_zero(ctx));
        RT_TRY(enqueue_trace_rays(ctx, q, true, s.at(i_rays), n, s.at(i_rgb)));
        RT_TRY(counters_read(ctx, c, true));
        RT_TRY(scratch_done(ctx));  // the counters' last user is this read-back
    }
    RT_TRY(s.sync());
    if (stats) {
        stats->trace_rays = c[0];
        stats->shadow_rays = c[1];
    }
    return RT_OK;
}

rt_status rt_intersect_rays(rt_context* ctx, const rt_scene* sc, const double* rays, size_t n,
                            double* hits) {
    if (!ctx || (n && (!rays || !hits)))
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_intersect_rays");
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, nullptr, 0, q));
    if (n == 0) return RT_OK;
    Stage s(ctx);
    const int i_rays = s.in(rays, n * kRayBytes), i_hits = s.out(hits, n * 9 * sizeof(double));
    RT_TRY(s.upload());
    RT_TRY(enqueue_intersect(ctx, q, s.at(i_rays), n, s.at(i_hits)));
    return s.finish();
}

// ---- any hit (rt_anyhit.hip) -------------------------------------------------------------------
rt_status rt_occluded_rays_device(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                                  const void* d_rays, const void* d_max_dist, size_t n,
                                  void* d_occluded) {
    if (!ctx || (n && (!d_rays || !d_max_dist || !d_occluded)))
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_occluded_rays_device");
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, kReadNoBvh, q));
    return n ? enqueue_occluded(ctx, q, d_rays, d_max_dist, n, d_occluded) : RT_OK;
}

rt_status rt_occluded_rays(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                           const double* rays, const double* max_dist, size_t n,
                           uint8_t* occluded_out) {
    if (!ctx || (n && (!rays || !max_dist || !occluded_out)))
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_occluded_rays");
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, kReadNoBvh, q));
    if (n == 0) return RT_OK;
    Stage s(ctx);
    const int i_rays = s.in(rays, n * kRayBytes), i_dist = s.in(max_dist, n * sizeof(double)),
              i_out = s.out(occluded_out, n, 1);
    RT_TRY(s.upload());
    RT_TRY(enqueue_occluded(ctx, q, s.at(i_rays), s.at(i_dist), n, s.at(i_out)));
    return s.finish();
}

// ---- transmittance (rt_transmit.hip) -----------------------------------------------------------
rt_status rt_transmittance_rays_device(rt_context* ctx, const rt_scene* sc,
                                       const rt_render_opts* opts, const void* d_rays,
                                       const void* d_max_dist, size_t n, void* d_T) {
    if (!ctx || (n && (!d_rays || !d_max_dist || !d_T)))
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_transmittance_rays_device");
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, kReadNoBvh | kReadBias, q));
    return n ? enqueue_transmittance(ctx, q, d_rays, d_max_dist, n, d_T) : RT_OK;
}

rt_status rt_transmittance_rays(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                                const double* rays, const double* max_dist, size_t n,
                                double* T_out) {
    if (!ctx || (n && (!rays || !max_dist || !T_out)))
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_transmittance_rays");
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, kReadNoBvh | kReadBias, q));
    if (n == 0) return RT_OK;
    Stage s(ctx);
    const int i_rays = s.in(rays, n * kRayBytes), i_dist = s.in(max_dist, n * sizeof(double)),
              i_out = s.out(T_out, n * sizeof(double));
    RT_TRY(s.upload());
    RT_TRY(enqueue_transmittance(ctx, q, s.at(i_rays), s.at(i_dist), n, s.at(i_out)));
    return s.finish();
}

// ---- the per-level queries (rt_transmit.hip, rt_direct.hip, rt_scatter.hip) -------------------
// Sixteen entries over the eight implementations above: {host, _device} x {un-keyed, _keyed}.
rt_status rt_light_transmittance_device(rt_context* ctx, const rt_scene* sc,
                                        const rt_render_opts* opts, const void* d_points, size_t n,
                                        void* d_T) {
    return light_transmittance_device(ctx, sc, opts, d_points, n, d_T, nullptr, false,
                                      "rt_light_transmittance_device");
}

rt_status rt_light_transmittance(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                                 const double* points, size_t n, double* T_out) {
    return light_transmittance_host(ctx, sc, opts, points, n, T_out, nullptr, false,
                                    "rt_light_transmittance");
}

rt_status rt_light_transmittance_keyed_device(rt_context* ctx, const rt_scene* sc,
                                              const rt_render_opts* opts, const void* d_points,
                                              size_t n, void* d_T, const rt_area_keys* keys) {
    return light_transmittance_device(ctx, sc, opts, d_points, n, d_T, keys, true,
                                      "rt_light_transmittance_keyed_device");
}

rt_status rt_light_transmittance_keyed(rt_context* ctx, const rt_scene* sc,
                                       const rt_render_opts* opts, const double* points, size_t n,
                                       double* T_out, const rt_area_keys* keys) {
    return light_transmittance_host(ctx, sc, opts, points, n, T_out, keys, true,
                                    "rt_light_transmittance_keyed");
}

rt_status rt_direct_light_device(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                                 const void* d_points, const void* d_materials, size_t n_materials,
                                 size_t n, int outputs, const struct rt_direct_light_out* d_out) {
    return direct_light_device(ctx, sc, opts, d_points, d_materials, n_materials, n, outputs,
                               d_out, nullptr, false, "rt_direct_light_device");
}

rt_status rt_direct_light(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                          const double* points, const rt_material* materials, size_t n_materials,
                          size_t n, int outputs, const struct rt_direct_light_out* out) {
    return direct_light_host(ctx, sc, opts, points, materials, n_materials, n, outputs, out,
                             nullptr, false, "rt_direct_light");
}

rt_status rt_direct_light_keyed_device(rt_context* ctx, const rt_scene* sc,
                                       const rt_render_opts* opts, const void* d_points,
                                       const void* d_materials, size_t n_materials, size_t n,
                                       int outputs, const struct rt_direct_light_out* d_out,
                                       const rt_area_keys* keys) {
    return direct_light_device(ctx, sc, opts, d_points, d_materials, n_materials, n, outputs,
                               d_out, keys, true, "rt_direct_light_keyed_device");
}

rt_status rt_direct_light_keyed(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                                const double* points, const rt_material* materials,
                                size_t n_materials, size_t n, int outputs,
                                const struct rt_direct_light_out* out, const rt_area_keys* keys) {
    return direct_light_host(ctx, sc, opts, points, materials, n_materials, n, outputs, out, keys,
                             true, "rt_direct_light_keyed");
}

rt_status rt_direct_light_rays_device(rt_context* ctx, const rt_scene* sc,
                                      const rt_render_opts* opts, const void* d_rays, size_t n,
                                      int outputs, const struct rt_direct_light_out* d_out) {
    return direct_light_rays_device(ctx, sc, opts, d_rays, n, outputs, d_out, nullptr, false,
                                    "rt_direct_light_rays_device");
}

rt_status rt_direct_light_rays(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                               const double* rays, size_t n, int outputs,
                               const struct rt_direct_light_out* out) {
    return direct_light_rays_host(ctx, sc, opts, rays, n, outputs, out, nullptr, false,
                                  "rt_direct_light_rays");
}

rt_status rt_direct_light_rays_keyed_device(rt_context* ctx, const rt_scene* sc,
                                            const rt_render_opts* opts, const void* d_rays,
                                            size_t n, int outputs,
                                            const struct rt_direct_light_out* d_out,
                                            const rt_area_keys* keys) {
    return direct_light_rays_device(ctx, sc, opts, d_rays, n, outputs, d_out, keys, true,
                                    "rt_direct_light_rays_keyed_device");
}

rt_status rt_direct_light_rays_keyed(rt_context* ctx, const rt_scene* sc,
                                     const rt_render_opts* opts, const double* rays, size_t n,
                                     int outputs, const struct rt_direct_light_out* out,
                                     const rt_area_keys* keys) {
    return direct_light_rays_host(ctx, sc, opts, rays, n, outputs, out, keys, true,
                                  "rt_direct_light_rays_keyed");
}

rt_status rt_scatter_rays_device(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                                 const void* d_rays, size_t n, int outputs,
                                 const struct rt_scatter_out* d_out) {
    return scatter_rays_device(ctx, sc, opts, d_rays, n, outputs, d_out, nullptr, false,
                               "rt_scatter_rays_device");
}

rt_status rt_scatter_rays(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                          const double* rays, size_t n, int outputs,
                          const struct rt_scatter_out* out) {
    return scatter_rays_host(ctx, sc, opts, rays, n, outputs, out, nullptr, false,
                             "rt_scatter_rays");
}

rt_status rt_scatter_rays_keyed_device(rt_context* ctx, const rt_scene* sc,
                                       const rt_render_opts* opts, const void* d_rays, size_t n,
                                       int outputs, const struct rt_scatter_out* d_out,
                                       const rt_area_keys* keys) {
    return scatter_rays_device(ctx, sc, opts, d_rays, n, outputs, d_out, keys, true,
                               "rt_scatter_rays_keyed_device");
}

rt_status rt_scatter_rays_keyed(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                                const double* rays, size_t n, int outputs,
                                const struct rt_scatter_out* out, const rt_area_keys* keys) {
    return scatter_rays_host(ctx, sc, opts, rays, n, outputs, out, keys, true,
                             "rt_scatter_rays_keyed");
}

// ---- closest hit with selectable outputs (rt_closest.hip) --------------------------------------
rt_status rt_closest_rays_device(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                                 const void* d_rays, size_t n, int outputs,
                                 const struct rt_closest_out* d_out) {
    RT_TRY(check_outputs(kChOut, outputs, d_out, !n || d_rays, ctx, "rt_closest_rays_device"));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, kReadNoBvh, q));
    return enqueue_closest(ctx, q, d_rays, n, requested(kChOut, outputs, *d_out));
}

rt_status rt_closest_rays(rt_context* ctx, const rt_scene* sc, const rt_render_opts* opts,
                          const double* rays, size_t n, int outputs,
                          const struct rt_closest_out* out) {
    RT_TRY(check_outputs(kChOut, outputs, out, !n || rays, ctx, "rt_closest_rays"));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    QueryParams q;
    RT_TRY(query_params(ctx, sc, opts, kReadNoBvh, q));
    Stage s(ctx);
    const int i_rays = s.in(rays, n * kRayBytes), i_out = s.outs(kChOut, outputs, *out, n);
    RT_TRY(s.upload());
    RT_TRY(enqueue_closest(ctx, q, s.at(i_rays), n, s.outs_at(kChOut, i_out)));
    return s.finish();
}

// ---- camera rays (rt_camera_rays.hip) ----------------------------------------------------------
rt_status rt_camera_rays_device(rt_context* ctx, const rt_camera* cam, const rt_render_opts* opts,
                                int sample, void* d_rays) {
    TraceParams p;
    RT_TRY(camera_rays_params(ctx, cam, opts, sample, d_rays, "rt_camera_rays_device", p));
    DeviceGuard g(ctx->device);
    return enqueue_camera_rays(ctx, p, sample, d_rays);
}

rt_status rt_camera_rays(rt_context* ctx, const rt_camera* cam, const rt_render_opts* opts,
                         int sample, double* rays_out) {
    TraceParams p;
    RT_TRY(camera_rays_params(ctx, cam, opts, sample, rays_out, "rt_camera_rays", p));
    DeviceGuard g(ctx->device);
    Stage s(ctx);
    const int i_out = s.out(rays_out, static_cast<size_t>(p.rows) * p.width * 6 * sizeof(double));
    RT_TRY(s.upload());
    RT_TRY(enqueue_camera_rays(ctx, p, sample, s.at(i_out)));
    return s.finish();
}

// ---- progressive frames (rt_accumulate.hip) ----------------------------------------------------
// The host twins stage in the buffers they share with render (out64, out32, tm_in, tm_out).
rt_status rt_accumulate_samples_device(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                                       const rt_render_opts* opts, int sample_begin,
                                       int sample_end, void* d_sum) {
    QueryParams q;
    RT_TRY(accumulate_params(ctx, sc, cam, opts, sample_begin, sample_end, d_sum,
                             "rt_accumulate_samples_device", q));
    DeviceGuard g(ctx->device);
    return enqueue_accumulate(ctx, q, sample_begin, sample_end, d_sum);
}

rt_status rt_accumulate_samples(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                                const rt_render_opts* opts, int sample_begin, int sample_end,
                                double* sum) {
    QueryParams q;
    RT_TRY(accumulate_params(ctx, sc, cam, opts, sample_begin, sample_end, sum,
                             "rt_accumulate_samples", q));
    DeviceGuard g(ctx->device);
    const size_t bytes = static_cast<size_t>(q.p.rows) * q.p.width * 3 * sizeof(double);
    RT_HIP(ctx->out64.ensure(bytes));
    if (sample_begin > 0)  // the sum so far; with sample_begin == 0 nothing of it is read
        RT_HIP(hipMemcpyAsync(ctx->out64.ptr, sum, bytes, hipMemcpyHostToDevice, ctx->stream));
    RT_TRY(enqueue_accumulate(ctx, q, sample_begin, sample_end, ctx->out64.ptr));
    RT_HIP(hipMemcpyAsync(sum, ctx->out64.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

rt_status rt_resolve_device(rt_context* ctx, const void* d_sum, size_t n, int samples, int tonemap,
                            void* d_hdr64, void* d_hdr32, void* d_ldr) {
    RT_TRY(check_resolve_args(ctx, d_sum, n, samples, tonemap, d_hdr64, d_hdr32, d_ldr,
                              "rt_resolve_device"));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    return enqueue_resolve(ctx, d_sum, n, samples, tonemap, d_hdr64, d_hdr32, d_ldr);
}

rt_status rt_resolve(rt_context* ctx, const double* sum, size_t n, int samples, int tonemap,
                     double* hdr64, float* hdr32, uint8_t* ldr) {
    RT_TRY(check_resolve_args(ctx, sum, n, samples, tonemap, hdr64, hdr32, ldr, "rt_resolve"));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    const size_t planes = tonemap == RT_TONEMAP_COUNT ? RT_TONEMAP_COUNT : 1;
    // the two HDR outputs as a frame's; the bytes (every operator's plane under RT_TONEMAP_COUNT)
    // in rt_tonemap's buffer
    const FrameStage fs(ctx, hdr64, hdr32, nullptr, n);
    RT_TRY(fs.grow());
    RT_HIP(ctx->tm_in.ensure(n * 3 * sizeof(double)));
    if (ldr) RT_HIP(ctx->tm_out.ensure(planes * n * 3));
    RT_HIP(hipMemcpyAsync(ctx->tm_in.ptr, sum, n * 3 * sizeof(double), hipMemcpyHostToDevice,
                          ctx->stream));
    RT_TRY(enqueue_resolve(ctx, ctx->tm_in.ptr, n, samples, tonemap, fs.dev(0), fs.dev(1),
                           ldr ? ctx->tm_out.ptr : nullptr));
    RT_TRY(fs.download());
    if (ldr)
        RT_HIP(hipMemcpyAsync(ldr, ctx->tm_out.ptr, planes * n * 3, hipMemcpyDeviceToHost,
                              ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

// ---- adaptive progressive frames (rt_adaptive.hip) ---------------------------------------------
rt_status rt_accumulate_adaptive_device(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                                        const rt_render_opts* opts, const rt_adaptive_rule* rule,
                                        int fresh, int sample_end, void* d_sum, void* d_moments,
                                        void* d_count) {
    QueryParams q;
    RT_TRY(adaptive_params(ctx, sc, cam, opts, rule, sample_end, d_sum, d_moments, d_count,
                           "rt_accumulate_adaptive_device", q));
    DeviceGuard g(ctx->device);
    return enqueue_adaptive(ctx, q, *rule, fresh, sample_end, d_sum, d_moments, d_count);
}

rt_status rt_accumulate_adaptive(rt_context* ctx, const rt_scene* sc, const rt_camera* cam,
                                 const rt_render_opts* opts, const rt_adaptive_rule* rule,
                                 int fresh, int sample_end, double* sum, double* moments,
                                 int32_t* count) {
    QueryParams q;
    RT_TRY(adaptive_params(ctx, sc, cam, opts, rule, sample_end, sum, moments, count,
                           "rt_accumulate_adaptive", q));
    DeviceGuard g(ctx->device);
    const size_t px = static_cast<size_t>(q.p.rows) * q.p.width;
    Stage s(ctx);  // the state so far goes up unless the call is fresh; all of it comes back
    const int i_sum = s.inout(sum, px * 3 * sizeof(double), !fresh),
              i_mom = s.inout(moments, px * 2 * sizeof(double), !fresh),
              i_cnt = s.inout(count, px * sizeof(int32_t), !fresh, sizeof(int32_t));
    RT_TRY(s.upload());
    RT_TRY(enqueue_adaptive(ctx, q, *rule, fresh, sample_end, s.at(i_sum), s.at(i_mom),
                            s.at(i_cnt)));
    return s.finish();
}

rt_status rt_resolve_counts_device(rt_context* ctx, const void* d_sum, const void* d_count,
                                   size_t n, int tonemap, void* d_hdr64, void* d_hdr32,
                                   void* d_ldr) {
    RT_TRY(check_resolve_args(ctx, d_sum, n, 1, tonemap, d_hdr64, d_hdr32, d_ldr,
                              "rt_resolve_counts_device", !d_count));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    return enqueue_resolve_counts(ctx, d_sum, d_count, n, tonemap, d_hdr64, d_hdr32, d_ldr);
}

rt_status rt_resolve_counts(rt_context* ctx, const double* sum, const int32_t* count, size_t n,
                            int tonemap, double* hdr64, float* hdr32, uint8_t* ldr) {
    RT_TRY(check_resolve_args(ctx, sum, n, 1, tonemap, hdr64, hdr32, ldr, "rt_resolve_counts",
                              !count));
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    const size_t planes = tonemap == RT_TONEMAP_COUNT ? RT_TONEMAP_COUNT : 1;
    Stage s(ctx);  // the counts (4 B each) after the arrays of doubles, before the floats and bytes
    const int i_sum = s.in(sum, n * 3 * sizeof(double)),
              i_64 = s.out(hdr64, hdr64 ? n * 3 * sizeof(double) : 0),
              i_32 = s.out(hdr32, hdr32 ? n * 3 * sizeof(float) : 0, sizeof(float)),
              i_cnt = s.in(count, n * sizeof(int32_t)),
              i_ldr = s.out(ldr, ldr ? planes * n * 3 : 0, 1);
    RT_TRY(s.upload());
    RT_TRY(enqueue_resolve_counts(ctx, s.at(i_sum), s.at(i_cnt), n, tonemap, s.at(i_64),
                                  s.at(i_32), s.at(i_ldr)));
    return s.finish();
}

rt_status rt_tonemap(rt_context* ctx, const double* hdr, size_t n, int op, uint8_t* out) {
    if (!ctx || (!hdr && n) || (!out && n))
        return fail(RT_ERR_INVALID_ARG, "NULL argument to rt_tonemap");
    if (op < 0 || op > RT_TONEMAP_COUNT) return fail(RT_ERR_INVALID_ARG, "tonemap op out of range");
    if (n == 0) return RT_OK;
    DeviceGuard g(ctx->device);
    const size_t planes = op == RT_TONEMAP_COUNT ? RT_TONEMAP_COUNT : 1;
    RT_HIP(ctx->tm_in.ensure(n * 3 * sizeof(double)));
    RT_HIP(ctx->tm_out.ensure(planes * n * 3));
    RT_HIP(hipMemcpyAsync(ctx->tm_in.ptr, hdr, n * 3 * sizeof(double), hipMemcpyHostToDevice,
                          ctx->stream));
    RT_HIP(launch_tonemap(static_cast<const double*>(ctx->tm_in.ptr), n, op,
                          static_cast<uint8_t*>(ctx->tm_out.ptr), ctx->stream));
    RT_HIP(hipMemcpyAsync(out, ctx->tm_out.ptr, planes * n * 3, hipMemcpyDeviceToHost,
                          ctx->stream));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

}  // extern "C"
