/*
 * rt_capi.h — C-ABI of the MI355X (gfx950) renderer that replaces the CPU hot path of
 * Sorax5/RaytracingEngine.  Plain C types only: pointers, sizes, PODs.  No exceptions cross
 * this boundary; every entry point returns an rt_status and the message of the last failure
 * on the calling thread is available from rt_last_error().
 *
 * Reference interface each entry point replaces (paths relative to /root/reference/RaytracingEngine):
 *
 *   rt_render / rt_render_device   std::vector<Vec3> Scene::RenderImage() const      Scene.h:311-328
 *                                  (per pixel: GeneratePixelAt Scene.h:283-304 → TraceRay Scene.h:131-198
 *                                   → IntersectClosest Scene.h:218-257, directLightning Scene.h:79-129,
 *                                   computeTransmittance Scene.h:35-77, backgroundColor Scene.h:30-33)
 *   rt_occluded_rays[_device]      bool Scene::IntersectAnyBefore(ray, maxDist) const   Scene.h:259-276
 *                                  (per shape: Sphere::Intersect Shape.h:72-98, Plane::Intersect
 *                                   Shape.h:149-159, Triangle::Intersect Shape.h:202-220)
 *   rt_transmittance_rays[_device] double Scene::computeTransmittance(ray, maxDist, bias) const   Scene.h:35-77
 *                                  (private there; each step an IntersectClosest Scene.h:218-257)
 *   rt_light_transmittance[_device] the shadow rays of Scene::directLightning   Scene.h:81, 86-104
 *   rt_direct_light[_device]       Vec3 Scene::directLightning(hit, viewDir, normalIn, bias) const   Scene.h:79-129
 *                                  (private there; over the point lights, for n surface points)
 *   rt_direct_light_rays[_device]  the localLight of Scene::TraceRay   Scene.h:136-147, 168
 *                                  (IntersectClosest, the normal flip, then directLightning)
 *   rt_scatter_rays[_device]       one level of Scene::TraceRay   Scene.h:131-198
 *                                  (what the level adds, and the child rays of Scene.h:178-180 and
 *                                   190-191 with their weights, before they are traced)
 *   rt_light_transmittance_keyed[_device], rt_direct_light_keyed[_device],
 *   rt_direct_light_rays_keyed[_device], rt_scatter_rays_keyed[_device]
 *                                  build-defined: the four entries above with the build-defined area
 *                                  light's samples appended to directLightning's loop (after
 *                                  Scene.h:86-124), their random draws under keys the caller supplies
 *   rt_camera_rays[_device]        Rayon Camera::getRay(x, y, AA) const   Math.h:99-121
 *                                  (for every pixel of a frame, with the jitter of one AA sample)
 *   rt_closest_rays[_device]       std::optional<HitInfo> Scene::IntersectClosest(ray) const
 *                                  Scene.h:218-257 (and HitInfo::material, Shape.h:28-38)
 *   rt_trace_rays[_device]         Vec3 Scene::TraceRay(ray, 0, bias) const   Scene.h:131-198
 *   rt_accumulate_samples[_device] the sample loop of Scene::GeneratePixelAt   Scene.h:283-304
 *                                  (Scene.h:289-297, for a range of its AA samples, into a resident sum)
 *   rt_resolve[_device]            GeneratePixelAt's division by the sample count   Scene.h:298-300,
 *                                  then tonemap()/toColor() as rt_tonemap
 *   rt_accumulate_adaptive[_device] that loop left per pixel where a stop rule on the pixel's samples
 *                                  says so (no counterpart: the reference takes every sample)
 *   rt_resolve_counts[_device]     the division by each pixel's own count, zero samples included
 *                                  Scene.h:298-303
 *   rt_tonemap                     tonemap() RaytracingEngine.cpp:165-174 and the operators of
 *                                  tonemapAll() RaytracingEngine.cpp:176-214, each followed by
 *                                  toColor() RaytracingEngine.cpp:113-121
 *   rt_scene_create                the scene state Scene::AddSphere/AddPlane/AddLight/AddTriangle/
 *                                  AddModel accumulate (Scene.h:208-212)
 *   rt_camera                      Camera (Math.h:85-122); antiAliasingAmount Math.h:94
 *
 * The C++20 drop-in headers under raytracingengine_amd/api/ (Math.h, Shape.h, Light.h, Scene.h,
 * Image.h) are the reference-shaped API above this ABI; see INTEGRATION.md.
 *
 * Numerics: all geometry and shading is IEEE binary64 evaluated in the reference's operation
 * order without FMA contraction, so images are bit-identical to the reference except where the
 * reference calls libm pow/log (Blinn-Phong, Fresnel, Reinhard-Jodie), which may differ by an ulp.
 */
#ifndef RT_CAPI_H
#define RT_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_VERSION 1

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = 1, /* null pointer, zero size, inconsistent counts, bad row range   */
    RT_ERR_HIP = 2,         /* a HIP runtime call failed (message names the call)           */
    RT_ERR_OOM = 3,         /* device allocation failed                                     */
    RT_ERR_UNSUPPORTED = 4, /* a request outside what this build implements                 */
    RT_ERR_NO_DEVICE = 5,   /* no gfx950 device at the requested ordinal                    */
    RT_ERR_RCCL = 6         /* an RCCL call failed (message names the call)                 */
} rt_status;

/* Material (Shape.h:13-19).  Defaults in the reference: shininess 128, specular 0,
 * transparency 0, refractive_index 1. */
typedef struct rt_material {
    double color[3];
    double shininess;
    double specular;
    double transparency;
    double refractive_index;
} rt_material;

/* Sphere (Shape.h:59-133): centre = Transform.position, radius. */
typedef struct rt_sphere {
    double center[3];
    double radius;
    rt_material material;
} rt_sphere;

/* Plane (Shape.h:135-186).  `normal` is the normal as the Plane object stores it, i.e.
 * already passed through Vec3::normalize() by the constructor (Shape.h:141-142). */
typedef struct rt_plane {
    double point[3];
    double normal[3];
    rt_material material;
} rt_plane;

/* Triangle (Shape.h:188-246): untranslated vertices plus Transform.position, which the
 * reference adds to every vertex on each query (tv0/tv1/tv2, Shape.h:198-200).  A Model
 * (Shape.h:248-307) is flattened into triangles that carry the model's material and
 * translation.  Order in rt_scene_desc.triangles: the scene's standalone triangles in
 * AddTriangle order, then every model's triangles in AddModel order and index order — the
 * closest-hit order of Scene::IntersectClosest (Scene.h:243-254). */
typedef struct rt_triangle {
    double v0[3];
    double v1[3];
    double v2[3];
    double translation[3];
    rt_material material;
} rt_triangle;

/* Point light (Light.h:6-15). */
typedef struct rt_light {
    double position[3];
    double color[3];
    double intensity;
} rt_light;

typedef struct rt_scene_desc {
    const rt_sphere* spheres;
    int32_t n_spheres;
    const rt_plane* planes;
    int32_t n_planes;
    const rt_triangle* triangles;
    int32_t n_triangles;
    const rt_light* lights;
    int32_t n_lights;
} rt_scene_desc;

/* Camera (Math.h:85-122).  aa_samples = Camera::antiAliasingAmount (reference default 32).
 * near/far: the trace does not read them (as in the reference); the G-buffer's normalised
 * depth does (HitInfo::normalizedDistance, Shape.h:40-42). */
typedef struct rt_camera {
    double position[3];
    double focal;
    uint32_t width;
    uint32_t height;
    int32_t aa_samples;
    int32_t _pad0;
    double near_plane;
    double far_plane;
} rt_camera;

/* Tonemap operators (RaytracingEngine.cpp:123-174), in tonemapAll()'s output order. */
typedef enum rt_tonemap_op {
    RT_TONEMAP_NONE = -1,                    /* no LDR output                               */
    RT_TONEMAP_SIMPLE = 0,                   /* simple()                       :123-131     */
    RT_TONEMAP_REINHARD = 1,                 /* reinhardSimple()               :133-135     */
    RT_TONEMAP_REINHARD_EXTENDED = 2,        /* reinhardExtended(c, 5.0)       :137-141,193 */
    RT_TONEMAP_REINHARD_EXTENDED_LUMINANCE = 3, /* reinhardExtendedLuminance(c, 5.0) :143-148,195 */
    RT_TONEMAP_REINHARD_JODIE = 4,           /* reinhardJodie(c, 0.18)         :150-154     */
    RT_TONEMAP_UNCHARTED2 = 5,               /* uncharted2()                   :156-163     */
    RT_TONEMAP_ACES = 6,                     /* aces_approx() == tonemap()     :89-98,165   */
    RT_TONEMAP_COUNT = 7
} rt_tonemap_op;

/* Soft-shadow extension (BASELINE config 5).  The reference has point lights only
 * (Light.h); an area light is a build-defined extension with no reference semantics. */
typedef struct rt_area_light {
    double corner[3];    /* one corner of the parallelogram emitter                        */
    double edge_u[3];    /* first edge vector                                              */
    double edge_v[3];    /* second edge vector                                             */
    double color[3];
    double intensity;    /* total intensity, split evenly over the samples                 */
    int32_t samples;     /* stratified samples per shading point (sqrt must be integral)   */
    int32_t _pad0;
} rt_area_light;

typedef struct rt_render_opts {
    int32_t max_recursion;   /* Scene::maxRecursion, reference value 10 (Scene.h:24)        */
    int32_t tonemap;         /* rt_tonemap_op applied to the LDR output, if requested       */
    double bias;             /* GeneratePixelAt's bias, reference value 1e-3 (Scene.h:291)  */
    uint64_t seed;           /* key of the counter-based AA jitter RNG (samples 1..N-1)     */
    uint32_t row_begin;      /* render rows [row_begin, row_end) only (row tiles for        */
    uint32_t row_end;        /*  multi-GPU); row_end == 0 means the full image height       */
    int32_t flags;           /* RT_FLAG_* bits                                              */
    /* Block-cyclic row sets (load-balanced multi-GPU frames).  With row_cycle > 1 the call
     * renders the blocks of row_block rows starting at row_begin + k*row_cycle*row_block
     * (k = 0, 1, ...), clipped to row_end, packed one after another in the outputs: rank r of
     * n passes row_begin = r*row_block, row_cycle = n.  0 / 1: the contiguous range above. */
    uint16_t row_block;
    uint16_t row_cycle;
} rt_render_opts;

#define RT_FLAG_COUNT_RAYS 0x1   /* also run the ray-counting pass (fills rt_stats counts)   */
#define RT_FLAG_TIME_KERNEL 0x2  /* bracket each render launch with HIP events              */
#define RT_FLAG_GENERIC_KERNEL 0x4 /* ablation: bypass the packet-culled kernel              */
#define RT_FLAG_NO_BVH 0x8         /* ablation: test every triangle (no triangle BVH)          */
#define RT_FLAG_PIPELINE 0x10      /* rt_render_gather: gather + assembly on the communicator's
                                      own stream, overlapping the next frame's render (two
                                      frame slots); rt_comm_synchronize waits for the frame   */
#define RT_FLAG_NO_TILE_ORDER 0x20 /* ablation: the packet kernel's default tile order instead
                                      of costliest tiles first (the image is the same)        */
#define RT_FLAG_NO_SAMPLE_PARALLEL 0x40 /* ablation: multi-sample planes-only chains loop over
                                      the samples per thread instead of one thread per sample
                                      (the image is the same)                                 */

/* Fills opts with the reference defaults: max_recursion 10, bias 1e-3, tonemap ACES,
 * full image, seed 0x5EED, no flags. */
void rt_render_opts_default(rt_render_opts* opts);

typedef struct rt_stats {
    uint64_t trace_rays;   /* TraceRay invocations that reach IntersectClosest              */
    uint64_t shadow_rays;  /* computeTransmittance invocations                              */
    double kernel_ms;      /* summed HIP-event time of render launches (RT_FLAG_TIME_KERNEL)*/
    uint64_t launches;     /* render launches timed into kernel_ms                          */
} rt_stats;

typedef struct rt_context rt_context;
typedef struct rt_scene rt_scene;

/* Thread-local message of the most recent failure ("" if none). */
const char* rt_last_error(void);

/* The build record of this library (no reference counterpart): a static JSON object with the
 * sha256 of the sources, headers and flags it was compiled from ("source_sha256"), the target
 * ("arch") and the compiler ("hipcc"), so that a run can check which sources its binary holds
 * (raytracingengine_amd/build.py source_digest). */
const char* rt_build_info(void);

/* Number of visible HIP devices (0 when none). */
int rt_device_count(void);

/* A context owns one HIP device, one stream and growable device buffers.  One context per
 * host thread; calls on a context are not thread-safe. */
rt_status rt_context_create(int device, rt_context** out);
rt_status rt_context_destroy(rt_context* ctx);
/* Make the context launch on an externally owned hipStream_t (NULL = its own stream). */
rt_status rt_context_set_stream(rt_context* ctx, void* hip_stream);
rt_status rt_context_synchronize(rt_context* ctx);

/* Upload a scene to the context's device (done once; the render then reads it from HBM). */
rt_status rt_scene_create(rt_context* ctx, const rt_scene_desc* desc, rt_scene** out);
rt_status rt_scene_destroy(rt_scene* scene);
/* Attach (or with NULL, detach) a build-defined area light to an uploaded scene. */
rt_status rt_scene_set_area_light(rt_scene* scene, const rt_area_light* light);

/* Synchronous host-buffer render: Scene::RenderImage().  Any of the three outputs may be
 * NULL.  hdr64_out: rows*width*3 doubles, row-major, idx = (y-row_begin)*W + x, RGB (the
 * reference's std::vector<Vec3> layout).  hdr32_out: the same as float.  ldr_out:
 * rows*width*3 bytes of opts->tonemap followed by toColor().  stats may be NULL. */
rt_status rt_render(rt_context* ctx, const rt_scene* scene, const rt_camera* cam,
                    const rt_render_opts* opts, double* hdr64_out, float* hdr32_out,
                    uint8_t* ldr_out, rt_stats* stats);

/* One frame on n contexts (one per GPU, each with its own copy of the scene: scenes[i] belongs to
 * ctxs[i]), returned in the caller's host buffers — Scene::RenderImage (Scene.h:311-328) over the
 * GPUs of a node from one process.  Context i renders the block-cyclic row set i of n
 * (opts->row_block rows per block, default 16; the row range and row_cycle of opts must be left
 * at the whole image).  Contexts on distinct GPUs: the RCCL path — communicators over their
 * devices (ncclCommInitAll, created on first use and cached in ctxs[0] until the list changes),
 * rt_render_gather_all into ctxs[0]'s device, one device-to-host copy per output.  Contexts that
 * share a GPU (RCCL allows one rank per GPU): the same through rt_comm_create_local (the gather
 * as device copies); RTAMD_MULTI_HOST=1 copies each context's rows straight to their host rows.
 * Stats, when requested, are summed over the contexts (kernel_ms: the slowest GPU's render). */
rt_status rt_render_multi(rt_context* const* ctxs, rt_scene* const* scenes, int n,
                          const rt_camera* cam, const rt_render_opts* opts, double* hdr64_out,
                          float* hdr32_out, uint8_t* rgb8_out, rt_stats* stats);

/* ---- Row-tiled frames over the GPUs of a node with ONE RCCL gather ----------
 * Replaces the pixel loop of Scene::RenderImage (Scene.h:318-325) split by rows: rank r of n
 * renders the block-cyclic row set r (blocks of opts->row_block rows, default 16, starting at
 * row r*block and every n*block rows after it), one ncclGather per requested output moves every
 * rank's rows (padded to the largest rank's) to rank 0 over xGMI, and rank 0 writes them into
 * image row order in its device framebuffers.  Everything is enqueued on the communicator's
 * context stream; no host synchronisation. */
#define RT_COMM_ID_BYTES 128    /* == NCCL_UNIQUE_ID_BYTES                                   */
#define RT_OUT_HDR64 0x1        /* float64 Vec3 framebuffer (24 B/px)                        */
#define RT_OUT_HDR32 0x2        /* float32 framebuffer (12 B/px)                             */
#define RT_OUT_LDR 0x4          /* tonemapped bytes of opts->tonemap (3 B/px)                */

typedef struct rt_comm rt_comm;

typedef struct rt_gather_timing {
    double render_ms;    /* summed over the timed frames (RT_FLAG_TIME_KERNEL), this rank   */
    double gather_ms;    /* the ncclGather(s), from the end of this rank's render           */
    double assemble_ms;  /* rank 0: the gathered rows written into image order              */
    uint64_t frames;     /* frames timed                                                    */
    uint32_t rows;       /* rows this rank renders per frame                                */
    uint32_t max_rows;   /* rows every rank sends (the largest rank's)                      */
} rt_gather_timing;

/* ncclGetUniqueId: called on one process, the bytes handed to every rank (any transport). */
rt_status rt_comm_unique_id(uint8_t* id /* RT_COMM_ID_BYTES */);
/* One rank of an n-rank communicator on ctx's device (non-blocking ncclCommInitRankConfig): one
 * process per GPU.  Destroy communicators before their contexts.  Failure detection (SURVEY §5;
 * the reference has no communicator): every wait on the communicator — its initialisation, the
 * issue of each gather, rt_comm_synchronize, rt_comm_set_root_weight — polls
 * ncclCommGetAsyncError with a deadline (rt_comm_create: RTAMD_COMM_TIMEOUT_MS, default 300000;
 * 0 = none).  On an asynchronous RCCL error or at the deadline the communicator is aborted
 * (ncclCommAbort: its kernels in flight return) and the call fails with RT_ERR_RCCL; every later
 * call on it fails the same way (destroy it and create a new one).  A rank whose peers never
 * join therefore gets RT_ERR_RCCL from rt_comm_create instead of blocking for ever. */
rt_status rt_comm_create(rt_context* ctx, int nranks, int rank, const uint8_t* id, rt_comm** out);
/* rt_comm_create with its deadline in milliseconds (0 = wait without a deadline). */
rt_status rt_comm_create_ex(rt_context* ctx, int nranks, int rank, const uint8_t* id,
                            long timeout_ms, rt_comm** out);
/* The deadline of the communicator's later waits (milliseconds, 0 = none). */
rt_status rt_comm_set_timeout(rt_comm* comm, long timeout_ms);
/* n communicators, one per context, over n DISTINCT devices from one process (ncclCommInitAll);
 * comms_out[i] is rank i on ctxs[i]. */
rt_status rt_comm_create_all(rt_context* const* ctxs, int n, rt_comm** comms_out);
/* n communicators over n contexts of ONE process that may share a GPU (RCCL allows one rank per
 * GPU): the same multi-rank frame — row plan, padded send buffers, rank 0's receive layout and
 * assembly, the pipelined slots — with the gather done as device-to-device copies of every
 * rank's packed rows into rank 0's receive buffer (what ncclGather delivers).  Driven only by
 * rt_render_gather_all; rt_render_multi uses it for contexts that share a device. */
rt_status rt_comm_create_local(rt_context* const* ctxs, int n, rt_comm** comms_out);
rt_status rt_comm_destroy(rt_comm* comm);
rt_status rt_comm_info(const rt_comm* comm, int* nranks, int* rank);
/* Weighted row split (every rank of the communicator sets the same weight before its next frame;
 * default 1).  Collective on an rt_comm_create communicator with n > 1: the ranks check that
 * they agree (one all-reduce) and all return RT_ERR_INVALID_ARG, weight unchanged, if not.
 * rt_render_gather_all[_batch] checks that its communicators carry one weight.  The frame's blocks are dealt over weight + n − 1 row sets, rank 0 renders `weight`
 * of them and every other rank one — rank 0's rows never cross a link, so when the peers' gathers
 * are link-bound it takes a larger share.  With weight > 1 the gather is a group of P2P sends of
 * equal counts (ncclSend / ncclRecv) into rank 0's receive buffer, where rank 0 renders its own
 * row sets in place; rank-local outputs of rank 0 hold its row sets one after another (each
 * nframes*max_rows*W*3 elements).  rt_gather_timing.rows is a rank's total. */
rt_status rt_comm_set_root_weight(rt_comm* comm, int weight);
/* Collective: every rank calls it with the same camera, opts and outputs (RT_OUT_* bits).  The
 * scene belongs to the communicator's context.  On rank 0 the d_* are whole-frame device
 * framebuffers (W*H*3 elements, image order) for every requested output; elsewhere ignored.
 * opts->flags RT_FLAG_TIME_KERNEL records the frame's render / gather / assembly times. */
rt_status rt_render_gather(rt_comm* comm, const rt_scene* scene, const rt_camera* cam,
                           const rt_render_opts* opts, int outputs, void* d_hdr64,
                           void* d_hdr32, void* d_ldr);
/* The same from one process for every rank of an rt_comm_create_all (one ncclGroup) or of an
 * rt_comm_create_local.  With n == 1 the rank renders straight into the framebuffers. */
rt_status rt_render_gather_all(rt_comm* const* comms, rt_scene* const* scenes, int n,
                               const rt_camera* cam, const rt_render_opts* opts, int outputs,
                               void* d_hdr64, void* d_hdr32, void* d_ldr);
/* A batch of nframes frames (see rt_render_batch: one camera per frame, same width / height /
 * focal / aa_samples) in one call: this rank renders its rows of every frame in one launch,
 * frame after frame at a stride of max_rows rows (the largest rank's row count), then ONE
 * ncclGather per gathered output moves the whole batch, and rank 0 assembles every frame (one
 * launch).  On rank 0 the d_* hold nframes whole frames back to back (frame f at f*W*H*3
 * elements).  rank_* (any may be NULL) receive outputs that are rendered but NOT gathered: this
 * rank's rows of every frame, packed, frame f at f*max_rows*W*3 elements (max_rows =
 * rt_gather_timing.max_rows; a rank with fewer rows leaves the rest of each frame's stride
 * unwritten; buffers of nframes*max_rows*W*3 elements) — e.g. the float64 HDR framebuffer kept
 * where it was rendered while the tonemapped bytes are gathered.  An output is either gathered
 * (in `outputs`) or rank-local, not both.  rt_render_gather = nframes 1, no rank_*. */
rt_status rt_render_gather_batch(rt_comm* comm, const rt_scene* scene, const rt_camera* cams,
                                 int nframes, const rt_render_opts* opts, int outputs,
                                 void* d_hdr64, void* d_hdr32, void* d_ldr, void* rank_hdr64,
                                 void* rank_hdr32, void* rank_ldr);
/* rt_render_gather_all for a batch of frames (the layouts of rt_render_gather_batch). */
rt_status rt_render_gather_all_batch(rt_comm* const* comms, rt_scene* const* scenes, int n,
                                     const rt_camera* cams, int nframes,
                                     const rt_render_opts* opts, int outputs, void* d_hdr64,
                                     void* d_hdr32, void* d_ldr);
/* Waits for every frame enqueued on the communicator (render, gather, assembly); on an
 * rt_comm_create communicator with n > 1 it polls the streams and ncclCommGetAsyncError and
 * aborts the communicator on an RCCL error or at its deadline (RT_ERR_RCCL). */
rt_status rt_comm_synchronize(rt_comm* comm);
/* Summed frame timings since the last reset (waits for the timed frames to finish). */
rt_status rt_comm_timing(rt_comm* comm, rt_gather_timing* out, int reset);

/* Asynchronous render into DEVICE buffers on the context's stream (inputs and outputs stay
 * resident in HBM).  Same layouts as rt_render; pointers are device pointers or NULL. */
rt_status rt_render_device(rt_context* ctx, const rt_scene* scene, const rt_camera* cam,
                           const rt_render_opts* opts, void* d_hdr64, void* d_hdr32,
                           void* d_ldr);
/* A batch of frames: Scene::RenderImage (Scene.h:311-328) once per camera of cams[0..nframes)
 * — views of one scene from several positions (an animation's frames, a camera path) — into
 * device buffers holding the frames back to back (frame f at f*rows*W*3 elements of each
 * output).  Every camera must have cams[0]'s width, height, focal and aa_samples; the position
 * may differ.  Scenes the packet kernel renders (no secondary rays) take up to 32 frames per
 * launch (one grid plane per frame), so the launch's ramp and drain are paid once per batch;
 * other scenes take one launch per frame.  Each frame is the frame rt_render_device gives. */
rt_status rt_render_batch(rt_context* ctx, const rt_scene* scene, const rt_camera* cams,
                          int nframes, const rt_render_opts* opts, void* d_hdr64,
                          void* d_hdr32, void* d_ldr);

/* ---- Full-frame G-buffer ---------------------------------------------------------------------
 * Per pixel, the HitInfo of the camera ray: what was hit, how far away, with which normal and
 * base colour — Scene::CalculatePixelDepth(x, y, false) (Scene.h:278-281) and
 * HitInfo::normalizedDistance(camera) (Shape.h:40-42) for every pixel of a frame in one launch.
 *
 * Pixel value: pixel (x, y) holds IntersectClosest(camera.getRay(x, y, false)); the ray is the
 *   unjittered one and aa_samples is ignored.
 * Bit-exactness: depth, normal and prim carry the same bits rt_intersect_rays returns for that
 *   ray.  normal is the unflipped HitInfo::normal: the plane's stored normal, the triangle's, or
 *   unit(p - C) for a sphere.  A triangle's index is its index into rt_scene_desc.triangles; a
 *   sphere's is the scene's index (also for scenes of more than 64 spheres, which the renderer
 *   holds in a spatial order of its own).
 * depth_norm: (t - near_plane) / (far_plane - near_plane) evaluated in double in that order, then
 *   rounded to float.  near_plane == far_plane follows IEEE; there is no special case.
 * Miss: prim = {0, -1}, depth = depth_norm = +inf, normal = albedo = 0.
 * Layouts follow rt_render_device: row-major and rows-local (idx = (y - row_begin)*W + x, one
 *   element group per pixel as listed below); row_begin / row_end and the block-cyclic row_block
 *   / row_cycle of opts are honoured.  Frame f of a batch sits f*rows*W pixels into each output;
 *   every camera must have cams[0]'s width, height, focal and aa_samples (rt_render_batch's rule).
 * RT_ERR_INVALID_ARG: outputs == 0, an unknown bit in outputs, or a requested output whose
 *   pointer is NULL (pointers of outputs that are not requested are ignored).
 * Of opts only the row set and the flags RT_FLAG_GENERIC_KERNEL, RT_FLAG_NO_BVH and
 *   RT_FLAG_TIME_KERNEL are read; max_recursion, bias, seed and tonemap are not (primary
 *   visibility does not depend on them, nor on the materials: every scene type is served). */
#define RT_GB_DEPTH      0x01  /* double   [px]    HitInfo::distance                          */
#define RT_GB_DEPTH_NORM 0x02  /* float    [px]    (float)HitInfo::normalizedDistance(camera) */
#define RT_GB_NORMAL     0x04  /* double   [px][3] HitInfo::normal                            */
#define RT_GB_PRIM       0x08  /* int32_t  [px][2] {type, index}, as rt_intersect_rays        */
#define RT_GB_ALBEDO     0x10  /* float    [px][3] (float)HitInfo::material.color             */
#define RT_GB_ALL        0x1f

/* The output pointers.  The identifier rt_gbuffer alone names the host entry point below (C has
 * one name space for functions and typedefs), so the record is `struct rt_gbuffer`, or
 * rt_gbuffer_out for short. */
struct rt_gbuffer {
    void* depth;
    void* depth_norm;
    void* normal;
    void* prim;
    void* albedo;
};
typedef struct rt_gbuffer rt_gbuffer_out;

/* Device pointers, asynchronous on the context's stream. */
rt_status rt_gbuffer_device(rt_context* ctx, const rt_scene* scene, const rt_camera* cams,
                            int nframes, const rt_render_opts* opts, int outputs,
                            const struct rt_gbuffer* d_out);
/* Host pointers, synchronous, one frame. */
rt_status rt_gbuffer(rt_context* ctx, const rt_scene* scene, const rt_camera* cam,
                     const rt_render_opts* opts, int outputs, const struct rt_gbuffer* h_out);

/* ---- Serving frame queue -------------------------------------------------------------------
 * Consecutive Scene::RenderImage() frames (Scene.h:311-328) into device framebuffers with
 * `depth` frames in flight on as many HIP streams of the context's device (depth 1..8), so that
 * one frame's launch tail can overlap the next frame's start.  Measured on MI355X with the C2
 * 1080p frame at the sustained clock it does not pay (45.4 µs per frame on one stream; 48.3 /
 * 47.3 / 46.1 µs at depth 2 / 3 / 4: concurrent frames contend for the same CUs); it serves
 * applications that submit frames from one thread without managing streams.  Frames are
 * independent; each submit returns a ticket, and
 * rt_queue_wait(ticket) returns once that frame's outputs are written.  The caller keeps the
 * framebuffers of frames in flight untouched (e.g. `depth` sets of them, used round-robin). */
typedef struct rt_queue rt_queue;
rt_status rt_queue_create(rt_context* ctx, int depth, rt_queue** out);
rt_status rt_queue_destroy(rt_queue* queue);
/* rt_render_device on the queue's next stream; *ticket (may be NULL) numbers the frame. */
rt_status rt_queue_submit(rt_queue* queue, const rt_scene* scene, const rt_camera* cam,
                          const rt_render_opts* opts, void* d_hdr64, void* d_hdr32, void* d_ldr,
                          uint64_t* ticket);
rt_status rt_queue_wait(rt_queue* queue, uint64_t ticket);
/* Waits for every submitted frame (and folds RT_FLAG_TIME_KERNEL timings into rt_stats). */
rt_status rt_queue_synchronize(rt_queue* queue);

/* Ray counts (and, with RT_FLAG_TIME_KERNEL, accumulated kernel time) since the last reset. */
rt_status rt_stats_read(rt_context* ctx, rt_stats* out);
rt_status rt_stats_reset(rt_context* ctx);

/* Batch Scene::TraceRay (Scene.h:131-198) at recursion depth 0 for n arbitrary host rays
 * {ox,oy,oz,dx,dy,dz}: the per-sample body of GenerateAntiAliasing (Scene.h:306-309).
 * rgb_out: n*3 doubles.  opts->max_recursion/bias/seed apply; the area-light RNG is keyed by
 * the ray's index.  stats may be NULL. */
rt_status rt_trace_rays(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                        const double* rays, size_t n, double* rgb_out, rt_stats* stats);

/* Batch Scene::IntersectClosest (Scene.h:218-257) for n host rays.  hits_out: n*9 doubles
 * {type, index, distance, normal.xyz, hitPoint.xyz}; type 0 = miss (index -1), 1 sphere,
 * 2 plane, 3 triangle (index into rt_scene_desc.triangles). */
rt_status rt_intersect_rays(rt_context* ctx, const rt_scene* scene, const double* rays,
                            size_t n, double* hits_out);

/* Batch Scene::IntersectAnyBefore (Scene.h:259-276) for n host rays {ox,oy,oz,dx,dy,dz} and n
 * distances: occluded_out[i] is 1 when some primitive's Intersect(ray i) returns a t with
 * t > 0.0 && t < max_dist[i], else 0 — the reference's `within`, each t in binary64 in the
 * reference's operation order, so there is no tolerance.  A Model counts through its flattened
 * triangles (its Intersect reports their smallest t).  max_dist NaN or <= 0 gives 0, +inf means
 * any hit with t > 0; a plane met at exactly t == 0 does not count (and does not hide an
 * occluder further along, as a closest hit compared with max_dist would); an empty scene gives
 * 0.  Lights, materials and the area light are not read.  opts may be NULL; only
 * RT_FLAG_NO_BVH is read.  n == 0 returns RT_OK. */
rt_status rt_occluded_rays(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                           const double* rays, const double* max_dist, size_t n,
                           uint8_t* occluded_out);
/* The same on device pointers (d_rays: n*6 doubles, d_max_dist: n doubles, d_occluded: n
 * bytes), asynchronous on the context's stream. */
rt_status rt_occluded_rays_device(rt_context* ctx, const rt_scene* scene,
                                  const rt_render_opts* opts, const void* d_rays,
                                  const void* d_max_dist, size_t n, void* d_occluded);

/* Batch Scene::computeTransmittance (Scene.h:35-77) for n host rays {ox,oy,oz,dx,dy,dz} and n
 * distances: T_out[i] in [0,1] is the value computeTransmittance(ray i, max_dist[i], opts->bias)
 * returns — a closest-hit march of at most 64 steps that multiplies the transparencies of what it
 * crosses before max_dist, each clamped to [0,1] (Scene.h:68).  Every t is binary64 in the
 * reference's operation order and ties go to the lowest scene index, as IntersectClosest decides
 * them, so there is no tolerance.  Materials are read for `transparency` only; lights and the
 * area light are not read.
 *   - max_dist NaN or <= 0 gives 1.0 (the loop is never entered); an empty scene gives 1.0.
 *   - max_dist +inf marches until a miss, until T <= 1e-4, or until the 64-step counter runs out:
 *     what lies beyond the 64th step is not seen.
 *   - A hit at t <= 0 moves the origin by bias, one at t <= bias by t + bias; neither is counted.
 *     A counted hit needs traveled + t < max_dist (not t < max_dist, and glass is not opaque:
 *     this is not rt_occluded_rays).
 *   - The direction is not normalised: t, traveled, bias and max_dist are all in units of its
 *     length, as in the reference.
 * Of opts only bias and RT_FLAG_NO_BVH are read — whatever else the caller left there neither
 * fails nor steers the call; opts == NULL gives the defaults (bias 1e-3).  n == 0 returns RT_OK.
 * Synchronous. */
rt_status rt_transmittance_rays(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                                const double* rays, const double* max_dist, size_t n,
                                double* T_out);
/* The same on device pointers (d_rays: n*6 doubles, d_max_dist: n doubles, d_T: n doubles),
 * asynchronous on the context's stream; no host memory is touched. */
rt_status rt_transmittance_rays_device(rt_context* ctx, const rt_scene* scene,
                                       const rt_render_opts* opts, const void* d_rays,
                                       const void* d_max_dist, size_t n, void* d_T);

/* The shadow rays of Scene::directLightning (Scene.h:86-104) from n surface points to every
 * point light of the scene.  points: n*6 doubles {p.xyz, normal.xyz}; T_out: n*n_lights doubles,
 * [i*n_lights + l].  For point i = {p, n_in} and light l, in this order (Scene.h:81, 87-104):
 *   1. normal = n_in.normalize() (Vec3::normalize: a length <= 1e-12 gives the zero vector);
 *   2. v = light.position - p;
 *   3. dist = v.length(); the answer is 0.0 if dist <= 0;
 *   4. L = v / dist;
 *   5. the answer is 0.0 if max(0, normal·L) <= 0;
 *   6. the answer is 0.0 if dist <= bias;
 *   7. otherwise it is computeTransmittance({p + normal*bias, L}, dist - bias, bias).
 * The three zeros are the reference's `continue`s: that light adds nothing at that point.  The
 * raw T is returned; dropping T <= bias (Scene.h:105) is the shader's decision, not the query's.
 * The caller passes the normal facing the viewer, as TraceRay flips it (Scene.h:146).  This entry
 * serves the point lights; rt_light_transmittance_keyed serves the build-defined area light as
 * well.  A scene without lights returns RT_OK and writes nothing.  opts as for rt_transmittance_rays.  Synchronous. */
rt_status rt_light_transmittance(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                                 const double* points, size_t n, double* T_out);
/* The same on device pointers (d_points: n*6 doubles, d_T: n*n_lights doubles), asynchronous on
 * the context's stream; no host memory is touched. */
rt_status rt_light_transmittance_device(rt_context* ctx, const rt_scene* scene,
                                        const rt_render_opts* opts, const void* d_points, size_t n,
                                        void* d_T);

/* Batch Scene::directLightning (Scene.h:79-129) for n surface points the caller supplies.
 * points: n*9 doubles {p.xyz, normal.xyz, view.xyz}.  `normal` faces the viewer, as TraceRay flips
 * it (Scene.h:146), and is normalised by the query (Scene.h:81, Vec3::normalize: a length <= 1e-12
 * gives the zero vector); `view` is viewDir (Scene.h:147) and is used as given, not normalised.
 * materials: n_materials == n gives every point its own rt_material, n_materials == 1 one
 * material shared by all points; any other count is RT_ERR_INVALID_ARG.
 * Per point, over the scene's point lights in scene order (Scene.h:86-124):
 *   1. v = light.position - p; dist = v.length(); the light is skipped if dist <= 0 (Scene.h:89);
 *   2. L = v / dist; ndl = max(0, normal·L); skipped if ndl <= 0 (Scene.h:93) or dist <= bias
 *      (Scene.h:98);
 *   3. T = computeTransmittance({p + normal*bias, L}, dist - bias, bias); dropped if T <= bias
 *      (Scene.h:105);
 *   4. contribution = (emitted * (1.0 / (dist*dist))) * ndl with emitted = color * intensity;
 *      diffuse += contribution * T (Scene.h:110-113);
 *   5. only if material.transparency <= 0 and material.specular > 0: H = (L + view).normalize(),
 *      NdotH = max(0, normal·H), and if NdotH > 0
 *      specular += ((emitted * (1.0 / (dist*dist))) * pow(NdotH, shininess)) * T (Scene.h:115-123).
 * Outputs, each n*3 doubles, chosen by the bits of `outputs`:
 *   RT_DL_DIFFUSE / RT_DL_SPECULAR  the two accumulators after the last light;
 *   RT_DL_RADIANCE                  color * diffuse + specular * material.specular (Scene.h:126-128),
 *                                   directLightning's return value.
 * Every operation is binary64 in the reference's order, so diffuse has no tolerance; where pow is
 * reached, specular and radiance are within 1e-12 * max(1, |value|) of libm's.
 * This entry reads the scene's point lights; rt_direct_light_keyed reads the build-defined area
 * light as well.  A scene without lights writes zeros: the outputs have a fixed shape.
 * Of opts only bias and RT_FLAG_NO_BVH are read; opts == NULL gives the defaults (bias 1e-3).
 * RT_ERR_INVALID_ARG: outputs == 0, an unknown bit in outputs, out NULL or a requested output's
 * pointer NULL (pointers of outputs not requested are ignored), NULL inputs with n > 0.
 * n == 0 returns RT_OK.  Synchronous. */
#define RT_DL_RADIANCE 0x1  /* double [n][3]  directLightning's return value               */
#define RT_DL_DIFFUSE  0x2  /* double [n][3]  diffuseAccumulation  (Scene.h:83, 113)        */
#define RT_DL_SPECULAR 0x4  /* double [n][3]  specularAccumlation  (Scene.h:84, 121)        */
#define RT_DL_ALL      0x7
struct rt_direct_light_out {
    void* radiance;
    void* diffuse;
    void* specular;
};
rt_status rt_direct_light(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                          const double* points, const rt_material* materials, size_t n_materials,
                          size_t n, int outputs, const struct rt_direct_light_out* out);
/* The same on device pointers (d_points: n*9 doubles, d_materials: n_materials*7 doubles, the
 * members of d_out: n*3 doubles each), asynchronous on the context's stream.  With
 * n_materials == n no host memory is touched; with n_materials == 1 d_materials is a HOST
 * pointer to the one shared material, which travels in the kernel arguments. */
rt_status rt_direct_light_device(rt_context* ctx, const rt_scene* scene,
                                 const rt_render_opts* opts, const void* d_points,
                                 const void* d_materials, size_t n_materials, size_t n,
                                 int outputs, const struct rt_direct_light_out* d_out);

/* The same shading at the first hit of n rays {ox,oy,oz,dx,dy,dz}: what TraceRay calls localLight
 * (Scene.h:168) at recursion depth 0.  Per ray: IntersectClosest (Scene.h:218-257), hitPoint =
 * o + d*t, incoming = d.normalize(), normal = hit.normal flipped against incoming
 * (Scene.h:145-146), viewDir = -incoming, the hit primitive's material, then directLightning as
 * above.  Every scene type is served: mirrors and glass too, whose child rays are simply not
 * traced.  A ray that hits nothing writes +0.0 to every requested output; what was hit is
 * rt_intersect_rays' or the G-buffer's answer.  outputs, out, opts and the errors as for
 * rt_direct_light.  Synchronous. */
rt_status rt_direct_light_rays(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                               const double* rays, size_t n, int outputs,
                               const struct rt_direct_light_out* out);
/* The same on device pointers (d_rays: n*6 doubles), asynchronous on the context's stream; no
 * host memory is touched. */
rt_status rt_direct_light_rays_device(rt_context* ctx, const rt_scene* scene,
                                      const rt_render_opts* opts, const void* d_rays, size_t n,
                                      int outputs, const struct rt_direct_light_out* d_out);

/* Batch scatter: one level of Scene::TraceRay (Scene.h:131-198) for n rays {ox,oy,oz,dx,dy,dz},
 * before its children are traced.  With it TraceRay is composable from this interface:
 *   TraceRay(ray, 0) == value(ray) + TraceRay(refraction child, 1) * fw
 *                                  + TraceRay(reflection child, 1) * rw
 * summed in that order (Scene.h:172, 182, 193); an absent child adds nothing.  The query never
 * recurses.  Per ray:
 *   Miss (IntersectClosest, Scene.h:218-257, finds nothing): value = backgroundColor(ray)
 *     (Scene.h:30-33, 137-139), the flags byte is 0, both child rays and both weights are +0.0.
 *   Hit: hitPoint = o + d*t; incoming, frontFace, the flipped normal, viewDir and cosTheta as in
 *     Scene.h:144-148; transparency = clamp(material.transparency, 0, 1) (Scene.h:166);
 *     localLight = directLightning(hit, viewDir, normal, bias) as rt_direct_light_rays forms it,
 *     over the scene's point lights only; value = (0,0,0) + localLight * (1 - transparency) if
 *     transparency < 1, else (0,0,0) (Scene.h:169-173).
 *   Refraction, only if transparency > 0: eta = frontFace ? 1/etaT : etaT/1, refractDir =
 *     incoming.refract(normal, eta); if refractDir.length() > bias the ray is
 *     {hitPoint + dir * (bias * 1e2), dir} with dir = refractDir.normalize(), and
 *     fw = transparency * (1 - fresnel), fresnel = f0 + (1 - f0) * pow(1 - cosTheta, 5),
 *     f0 = pow((etaT - 1) / (etaT + 1), 2) (Scene.h:26-28, 161-164, 175-183).  Otherwise (total
 *     internal reflection, or a refraction direction no longer than bias) there is no refraction
 *     ray and fresnel becomes exactly 1.0 (Scene.h:185).
 *   Reflection: rw = transparency > 0 ? fresnel : material.specular; the ray is present if
 *     rw > bias: {hitPoint + dir * bias, dir} with dir = incoming.reflect(normal).normalize()
 *     (Scene.h:189-191).
 *   An absent child: its six doubles and its weight are +0.0, so the outputs have a fixed shape
 *     and repeated calls return the same bytes.  Callers select live children by the flags; an
 *     absent child is not to be traced (0 * NaN is NaN).
 * Recursion limit: opts->max_recursion <= 0 treats every ray as one at the limit
 * (Scene.h:132-134): value = backgroundColor(ray), nothing is intersected, flags 0, no children —
 * how a caller ends a composition.  Any max_recursion > 0, the default included, gives the level
 * above.
 * Of opts only max_recursion (its sign), bias and RT_FLAG_NO_BVH are read; opts == NULL gives the
 * defaults.  This entry does not read the build-defined area light, even when attached to the
 * scene (the rule of rt_direct_light and rt_light_transmittance): rt_scatter_rays_keyed, which
 * takes the pixel and sample keys its random numbers need, does.
 * Numerics: child rays, flags and a miss's value carry no tolerance.  A hit's value carries none
 * where directLightning does not reach pow, else it is within 1e-12 * max(1, |value|) of libm's.
 * rw of an opaque material is material.specular bit for bit; fw and rw of a transparent material
 * pass through the Fresnel pow and are held to the same 1e-12 bar; under total internal
 * reflection rw is exactly 1.0.
 * RT_ERR_INVALID_ARG: outputs == 0, an unknown bit in outputs, out NULL or a requested output's
 * pointer NULL (pointers of outputs not requested are ignored), NULL rays with n > 0, a NULL
 * context or scene.  n == 0 returns RT_OK.  Host pointers, synchronous. */
#define RT_SC_VALUE    0x01  /* double  [n][3]  what this level adds before its children        */
#define RT_SC_REFRACT  0x02  /* double  [n][6]  refraction ray {o, d}      (Scene.h:178-180)     */
#define RT_SC_REFLECT  0x04  /* double  [n][6]  reflection ray {o, d}      (Scene.h:190-191)     */
#define RT_SC_WEIGHTS  0x08  /* double  [n][2]  {fw, rw}: transparency*(1-fresnel), reflectiveness */
#define RT_SC_FLAGS    0x10  /* uint8_t [n]     bit 0 hit, bit 1 refraction ray, bit 2 reflection ray */
#define RT_SC_ALL      0x1f
struct rt_scatter_out {
    void* value;
    void* refract_rays;
    void* reflect_rays;
    void* weights;
    void* flags;
};
rt_status rt_scatter_rays(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                          const double* rays, size_t n, int outputs,
                          const struct rt_scatter_out* out);
/* The same on device pointers (d_rays: n*6 doubles; the members of d_out sized as above),
 * asynchronous on the context's stream; no host memory is touched. */
rt_status rt_scatter_rays_device(rt_context* ctx, const rt_scene* scene,
                                 const rt_render_opts* opts, const void* d_rays, size_t n,
                                 int outputs, const struct rt_scatter_out* d_out);

/* The keys of the build-defined area light's draws for a batch of rays or points: what the four
 * _keyed queries below take next to their sibling's arguments.  The render kernels draw the
 * point of area sample s of a hit from two uniform numbers of the counter RNG under the key
 * (opts->seed, pixel, stream, 2s | 2s + 1); a frame uses pixel = y_image*W + x and the AA sample
 * index, rt_trace_rays pixel = the ray's index and sample 0, both the recursion depth of the hit. */
typedef struct rt_area_keys {
    const void* pixel;  /* n uint64 keys, or NULL: element i draws with pixel = i (rt_trace_rays' rule).
                           Host pointer in the host entries, device pointer in the _device entries. */
    uint32_t sample;    /* AA sample index s     } stream = 0x10000 + (s << 6) + depth,          */
    uint32_t depth;     /* recursion depth 0..63 } as the render kernels form it                 */
} rt_area_keys;

/* The direct-light, shadow and scatter queries with the build-defined area light served
 * (rt_scene_set_area_light; BASELINE config 5).  Each entry has its sibling's arguments, outputs,
 * numerics and errors, plus `keys`; its _device twin is asynchronous on the context's stream as
 * the sibling's.  The struct itself is always host memory and is read before the call returns;
 * keys == NULL means {NULL, 0, 0}.  RT_ERR_INVALID_ARG in addition to the sibling's: depth > 63
 * (the streams of neighbouring samples would collide), sample > 0x00FFFFFF (the stream is a
 * uint32).  Of opts the entries read what the sibling reads, and seed.
 *
 * The area samples are appended to directLightning's loop after the point lights, in sample
 * order s = 0 .. samples-1, into the same diffuse and specular accumulators.  With
 * k = sqrt(samples), r1 = u01(seed, pixel, stream, 2s), r2 = u01(seed, pixel, stream, 2s + 1):
 *   fu = ((double)(s % k) + r1) / k;  fv = ((double)(s / k) + r2) / k;
 *   light point = (corner + edge_u*fu) + edge_v*fv;
 *   emitted     = color * (intensity / samples);
 * then steps 1-5 of rt_direct_light with that point and that emitted value.
 *
 *   rt_direct_light_keyed, rt_direct_light_rays_keyed: RT_DL_DIFFUSE / RT_DL_SPECULAR are the
 *     accumulators after the last area sample, RT_DL_RADIANCE their combination as before.
 *   rt_scatter_rays_keyed: value is formed from that localLight.  Child rays, weights and flags
 *     do not depend on the keys; a terminal level (max_recursion <= 0) is the sky, as before.
 *     TraceRay of an area-light scene composes as in rt_scatter_rays, each level asked with
 *     depth = its recursion level and the pixel keys of the rays its rays descend from.
 *   rt_light_transmittance_keyed: T_out is n * (n_lights + samples) doubles.  Columns
 *     0 .. n_lights-1 are rt_light_transmittance's; column n_lights + s is the same seven steps with
 *     the light point of sample s in place of light.position.  The mean of the last `samples`
 *     columns is the point's soft visibility.  With no column at all nothing is written.
 *
 * A scene without an area light: every keyed entry returns its sibling's bytes; the keys are
 * validated but otherwise unused, and the light transmittance has n_lights columns. */
rt_status rt_light_transmittance_keyed(rt_context* ctx, const rt_scene* scene,
                                       const rt_render_opts* opts, const double* points, size_t n,
                                       double* T_out, const rt_area_keys* keys);
rt_status rt_light_transmittance_keyed_device(rt_context* ctx, const rt_scene* scene,
                                              const rt_render_opts* opts, const void* d_points,
                                              size_t n, void* d_T, const rt_area_keys* keys);
rt_status rt_direct_light_keyed(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                                const double* points, const rt_material* materials,
                                size_t n_materials, size_t n, int outputs,
                                const struct rt_direct_light_out* out, const rt_area_keys* keys);
rt_status rt_direct_light_keyed_device(rt_context* ctx, const rt_scene* scene,
                                       const rt_render_opts* opts, const void* d_points,
                                       const void* d_materials, size_t n_materials, size_t n,
                                       int outputs, const struct rt_direct_light_out* d_out,
                                       const rt_area_keys* keys);
rt_status rt_direct_light_rays_keyed(rt_context* ctx, const rt_scene* scene,
                                     const rt_render_opts* opts, const double* rays, size_t n,
                                     int outputs, const struct rt_direct_light_out* out,
                                     const rt_area_keys* keys);
rt_status rt_direct_light_rays_keyed_device(rt_context* ctx, const rt_scene* scene,
                                            const rt_render_opts* opts, const void* d_rays,
                                            size_t n, int outputs,
                                            const struct rt_direct_light_out* d_out,
                                            const rt_area_keys* keys);
rt_status rt_scatter_rays_keyed(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                                const double* rays, size_t n, int outputs,
                                const struct rt_scatter_out* out, const rt_area_keys* keys);
rt_status rt_scatter_rays_keyed_device(rt_context* ctx, const rt_scene* scene,
                                       const rt_render_opts* opts, const void* d_rays, size_t n,
                                       int outputs, const struct rt_scatter_out* d_out,
                                       const rt_area_keys* keys);

/* Camera rays: Camera::getRay(x, y, sample > 0 && aa_samples > 1) (Math.h:99-121) for every
 * pixel of the row set of opts — the primary rays the render kernels trace for AA sample
 * `sample` of a frame of this camera, seed and row set.  No scene is involved.
 * rays_out: rows*W*6 doubles {ox,oy,oz,dx,dy,dz}, row-major and rows-local like rt_render_device's
 * and rt_gbuffer_device's pixels: ray (x, y) sits at idx = (y_local*W + x); row_begin / row_end
 * and the block-cyclic row_block / row_cycle of opts are honoured.  o is the camera position, d a
 * unit vector.
 * Jitter: sample 0 is never jittered (GeneratePixelAt, Scene.h:289-292: `aa > 0 && aaCount > 1`).
 * Samples > 0 add the two uniform numbers of the build-defined counter RNG under the key
 * (opts->seed, y_image*W + x, sample, 0 | 1) to the screen x and y, the render kernels' own
 * draw.  So RenderImage is expressible from this interface:
 *   render(x, y) == (TraceRay(ray of sample 0) + ... + TraceRay(ray of sample N-1)) / N
 * summed in that order (Scene.h:289-300); for a scene with an area light, whose random numbers are
 * keyed by the pixel and the sample, from the _keyed queries above under those keys.
 * Of opts only the row set and seed are read; opts == NULL gives the defaults.
 * RT_ERR_INVALID_ARG: a NULL context, camera or output, zero width or height, a row set outside
 * the image, sample < 0 or sample >= max(1, aa_samples).  RT_ERR_UNSUPPORTED: more than 2^31
 * pixels.  Host pointer, synchronous. */
rt_status rt_camera_rays(rt_context* ctx, const rt_camera* cam, const rt_render_opts* opts,
                         int sample, double* rays_out);
/* The same into a device pointer (rows*W*6 doubles), asynchronous on the context's stream; no
 * host memory is touched. */
rt_status rt_camera_rays_device(rt_context* ctx, const rt_camera* cam, const rt_render_opts* opts,
                                int sample, void* d_rays);

/* Batch Scene::IntersectClosest (Scene.h:218-257) for n rays {ox,oy,oz,dx,dy,dz} with selectable
 * structure-of-arrays outputs: what rt_intersect_rays answers in nine interleaved doubles per
 * ray, plus the hit primitive's material (HitInfo::material), each in a plane of its own, and
 * only those requested are computed and written.
 * Bit-exactness: t, normal, point and prim carry the bits rt_intersect_rays returns for the same
 *   ray (ties go to the first primitive in the reference's order of spheres, planes, triangles;
 *   the comparison is the strict '<' of Scene.h:226-254).  normal is the unflipped
 *   HitInfo::normal.  A triangle's index is its index into rt_scene_desc.triangles; a sphere's is
 *   the scene's index (also for scenes of more than 64 spheres, which the renderer holds in a
 *   spatial order of its own).  material is the seven doubles of the primitive's rt_material in
 *   member order, as uploaded — what rt_direct_light accepts per point.
 * Miss: t = +inf and prim = {0, -1} (the G-buffer's rule), normal = point = material = +0.0.
 * Of opts only RT_FLAG_NO_BVH is read; opts == NULL gives the defaults.  Lights and the area
 * light are not read.
 * RT_ERR_INVALID_ARG: outputs == 0, an unknown bit in outputs, out NULL or a requested output's
 * pointer NULL (pointers of outputs not requested are ignored), NULL rays with n > 0, a NULL
 * context or scene.  n == 0 returns RT_OK.  Host pointers, synchronous. */
#define RT_CH_T        0x01  /* double  [n]     HitInfo::distance                                */
#define RT_CH_PRIM     0x02  /* int32_t [n][2]  {type, index}, as rt_intersect_rays / RT_GB_PRIM */
#define RT_CH_NORMAL   0x04  /* double  [n][3]  HitInfo::normal, unflipped                       */
#define RT_CH_POINT    0x08  /* double  [n][3]  HitInfo::hitPoint = o + d*t                      */
#define RT_CH_MATERIAL 0x10  /* double  [n][7]  HitInfo::material as rt_material                 */
#define RT_CH_ALL      0x1f
struct rt_closest_out {
    void* t;
    void* prim;
    void* normal;
    void* point;
    void* material;
};
rt_status rt_closest_rays(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                          const double* rays, size_t n, int outputs,
                          const struct rt_closest_out* out);
/* The same on device pointers (d_rays: n*6 doubles; the members of d_out sized as above),
 * asynchronous on the context's stream; no host memory is touched. */
rt_status rt_closest_rays_device(rt_context* ctx, const rt_scene* scene,
                                 const rt_render_opts* opts, const void* d_rays, size_t n,
                                 int outputs, const struct rt_closest_out* d_out);

/* rt_trace_rays on device pointers: d_rays n*6 doubles, d_rgb n*3 doubles, asynchronous on the
 * context's stream.  No staging copy is made, no host memory is touched and no stats are taken
 * (ray counting stays with the host entry).  The kernel is the one rt_trace_rays selects for the
 * scene and opts, so the bytes are the host entry's; the same members of opts apply
 * (max_recursion, bias, seed, RT_FLAG_NO_BVH), and RT_ERR_UNSUPPORTED for a max_recursion above
 * the kernels' limit with reflective or transparent materials.  RT_ERR_INVALID_ARG: a NULL
 * context or scene, a NULL pointer with n > 0.  n == 0 returns RT_OK. */
rt_status rt_trace_rays_device(rt_context* ctx, const rt_scene* scene, const rt_render_opts* opts,
                               const void* d_rays, size_t n, void* d_rgb);

/* Progressive frames: Scene::GeneratePixelAt (Scene.h:283-304) cut at any AA sample.  For every
 * pixel px of the row set of opts:
 *   sum[px] = (sample_begin == 0 ? +0.0 : sum[px]);
 *   for s in [sample_begin, sample_end):
 *       sum[px] = sum[px] + TraceRay(camera ray of sample s at px, 0, bias)
 * the loop of Scene.h:289-297 in its order, so that
 *   rt_render_device == rt_resolve_device(rt_accumulate_samples_device(0, N), N),  N = aa_samples,
 * bit for bit wherever the frame equals its samples' TraceRay summed in order (rt_camera_rays
 * above), and the frame can be cut after any sample: a preview after the first, refinement while
 * the camera rests, 28 samples added to 4 that exist.
 * d_sum: rows*W*3 doubles, row-major and rows-local like rt_render_device's hdr64.
 * Which rays: the ray of sample s is rt_camera_rays' ray, Camera::getRay(x, y, s > 0 &&
 *   aa_samples > 1): sample 0 is never jittered, samples above 0 only when aa_samples > 1, and the
 *   RNG key is the image pixel y_image*W + x (with opts->seed and s).
 * Which TraceRay: the device function rt_trace_rays selects for the scene and opts (no secondary
 *   ray, reflection chain or refraction tree), with its RT_ERR_UNSUPPORTED for a max_recursion
 *   above the kernels' limit with reflective or transparent materials.
 * Area light: with an area light attached its random numbers are keyed by (pixel, s), as the
 *   render kernels key them — not by a ray's index, as rt_trace_rays keys them — so the frame of
 *   an area-light scene is reproduced too.
 * The sum: with sample_begin == 0 the previous contents of d_sum are not read (no memset is
 *   needed, NaN garbage is harmless); with sample_begin > 0 they are.  The fold is sequential:
 *   only continuing ONE sum is bit-exact.  Adding two separately accumulated ranges,
 *   accumulate(0, k) + accumulate'(k, N), rounds in another order than the reference and is not
 *   its frame.
 * Of opts the call reads max_recursion, bias, seed, the row set (row_begin / row_end / row_block /
 *   row_cycle) and RT_FLAG_NO_BVH; tonemap and the other flags are ignored.  opts == NULL gives
 *   the defaults.  The packet, box and breadth-first render kernels are not used: one thread per
 *   pixel runs the generic TraceRay.
 * RT_ERR_INVALID_ARG: sample_begin < 0, sample_begin >= sample_end, sample_end > max(1,
 *   aa_samples), a NULL context, scene, camera or sum, zero width or height, a row set outside the
 *   image.  Asynchronous on the context's stream; no host memory is touched. */
rt_status rt_accumulate_samples_device(rt_context* ctx, const rt_scene* scene,
                                       const rt_camera* cam, const rt_render_opts* opts,
                                       int sample_begin, int sample_end, void* d_sum);
/* The same on a host sum (in and out: read only when sample_begin > 0), synchronous. */
rt_status rt_accumulate_samples(rt_context* ctx, const rt_scene* scene, const rt_camera* cam,
                                const rt_render_opts* opts, int sample_begin, int sample_end,
                                double* sum);

/* Resolve a sum, or any FP64 radiance buffer, on the device: per pixel v = sum / (double)samples
 * (GeneratePixelAt's division, Scene.h:298-300, the render kernels' own), then what a render
 * writes: d_hdr64 (v, n*3 doubles), d_hdr32 ((float)v, n*3 floats) and d_ldr (toColor(op(v))).
 * Any output may be NULL, not all of them.  d_hdr64 may be d_sum itself.
 * tonemap in [0, RT_TONEMAP_COUNT): n*3 bytes; RT_TONEMAP_COUNT: seven planes in tonemapAll()
 * order, 7*n*3 bytes, as rt_tonemap; RT_TONEMAP_NONE only with d_ldr NULL.
 * Device tonemap: rt_resolve_device(ctx, d_hdr, n, 1, op, NULL, NULL, d_ldr) is rt_tonemap on
 * device pointers — the division by 1.0 is exact — with rt_tonemap's bytes.
 * RT_ERR_INVALID_ARG: samples < 1, an unknown tonemap, every output NULL, d_ldr with
 * RT_TONEMAP_NONE, a NULL sum with n_pixels > 0, a NULL context.  n_pixels == 0 returns RT_OK.
 * Asynchronous on the context's stream; no host memory is touched. */
rt_status rt_resolve_device(rt_context* ctx, const void* d_sum, size_t n_pixels, int samples,
                            int tonemap, void* d_hdr64, void* d_hdr32, void* d_ldr);
/* The same on host pointers, synchronous. */
rt_status rt_resolve(rt_context* ctx, const double* sum, size_t n_pixels, int samples, int tonemap,
                     double* hdr64, float* hdr32, uint8_t* ldr);

/* Adaptive progressive frames: the sum of rt_accumulate_samples continued per pixel only while a
 * stop rule on the pixel's own samples asks for more.  State per pixel of the row set of opts,
 * rows-local like d_sum above: d_sum 3 doubles, d_moments 2 doubles {m1, m2}, d_count one int32.
 * fresh != 0: none of the three is read (no memset is needed) and n, sum, m1, m2 start at
 * 0 / +0.0.  For every pixel px:
 *
 *   n = count[px]
 *   while n < sample_end:
 *       if n >= min_samples and converged(n, m1, m2): break
 *       c   = TraceRay(camera ray of sample n at px, 0, bias)   -- exactly rt_accumulate_samples' ray, key and TraceRay
 *       sum = sum + c                                           -- GeneratePixelAt's fold, Scene.h:289-297
 *       L   = (c.x*0.2126 + c.y*0.7152) + c.z*0.0722            -- luminance, Vec3::dot order
 *       m1  = m1 + L;  m2 = m2 + L*L;  n = n + 1
 *   count[px] = n
 *
 *   converged(n, m1, m2):            -- IEEE binary64, one rounding per operation, no FMA, no sqrt, no libm
 *       nd = (double)n;  mean = m1 / nd
 *       var  = (m2 - m1*mean) / (nd - 1.0)
 *       err2 = var / nd                                   -- squared standard error of the mean luminance
 *       ref  = mean > lum_floor ? mean : lum_floor
 *       lim  = tolerance * ref
 *       return err2 <= lim*lim                            -- false for NaN: such a pixel runs to sample_end
 *
 * The rule is re-examined before every sample, so count[px] is a function of the pixel's sample
 * sequence alone: it does not depend on how calls cut the range (sample_end = 3, then 5, then 8
 * on one state is sample_end = 8, in all three arrays, bit for bit; a pixel the rule stopped
 * stays stopped), on the launch shape, or on which kernel traced the pixel.  sum[px] is
 * rt_accumulate_samples(0, count[px])[px] bit for bit; with min_samples >= sample_end the rule
 * never fires, sum is rt_accumulate_samples(0, sample_end) and every count is sample_end.  A
 * pixel that takes no sample in a call that is not fresh is not written.
 * Kernels: one thread per pixel in 8x8 tiles while at least half of a wave's pixels want samples;
 * the rest is appended to a device-side list in the context and finished 64 listed pixels to a
 * wave.  RTAMD_ADAPT_LIST=0 in the environment, read per call, keeps every pixel in the tile
 * kernel; the three arrays are the same bits.
 * Of opts the call reads what rt_accumulate_samples_device reads, the row set included.
 * RT_ERR_INVALID_ARG, before anything is dereferenced or a device is touched: a NULL context,
 *   scene, camera, rule or array; zero width or height; sample_end < 1 or > max(1, aa_samples);
 *   min_samples < 2; tolerance negative or NaN; lum_floor not > 0; a row set outside the image.
 * RT_ERR_UNSUPPORTED: as rt_accumulate_samples_device; a row set above 2^32 pixels.
 * Asynchronous on the context's stream; no host memory is touched. */
typedef struct rt_adaptive_rule {
    double tolerance;     /* relative standard error of the mean luminance to stop at, >= 0 */
    double lum_floor;     /* the mean luminance below which the error is absolute, > 0 */
    int32_t min_samples;  /* samples every pixel takes before the rule is examined, >= 2 */
    int32_t _pad0;
} rt_adaptive_rule;
rt_status rt_accumulate_adaptive_device(rt_context* ctx, const rt_scene* scene,
                                        const rt_camera* cam, const rt_render_opts* opts,
                                        const rt_adaptive_rule* rule, int fresh, int sample_end,
                                        void* d_sum, void* d_moments, void* d_count);
/* The same on host arrays (in and out: read unless fresh), synchronous. */
rt_status rt_accumulate_adaptive(rt_context* ctx, const rt_scene* scene, const rt_camera* cam,
                                 const rt_render_opts* opts, const rt_adaptive_rule* rule,
                                 int fresh, int sample_end, double* sum, double* moments,
                                 int32_t* count);

/* rt_resolve_device with each pixel's own count as the divisor: v = sum / (double)count, and
 * {0,0,0} for a pixel whose count is 0 (GeneratePixelAt, Scene.h:298-303: its sum is not read);
 * then what rt_resolve_device writes.  The argument checks are rt_resolve_device's, plus a NULL
 * count with n_pixels > 0. */
rt_status rt_resolve_counts_device(rt_context* ctx, const void* d_sum, const void* d_count,
                                   size_t n_pixels, int tonemap, void* d_hdr64, void* d_hdr32,
                                   void* d_ldr);
/* The same on host pointers, synchronous. */
rt_status rt_resolve_counts(rt_context* ctx, const double* sum, const int32_t* count,
                            size_t n_pixels, int tonemap, double* hdr64, float* hdr32,
                            uint8_t* ldr);

/* Device tonemap of host FP64 radiance: op in [0, RT_TONEMAP_COUNT) writes n*3 bytes;
 * op == RT_TONEMAP_COUNT writes all seven operators, tonemapAll() order, 7*n*3 bytes. */
rt_status rt_tonemap(rt_context* ctx, const double* hdr, size_t n_pixels, int op,
                     uint8_t* ldr_out);

/* Test hook: evaluates x/y, sqrt(x), pow(x,y), log(x) and the Blinn-Phong pow of the trace
 * kernels (rt_device.hpp pow_bp) on the device for n inputs so the parity suite can pin device
 * libm against the host's.  out: 5*n doubles. */
rt_status rt_debug_f64_ops(rt_context* ctx, const double* x, const double* y, size_t n,
                           double* out);

/* Test hook: per 3-vector v (3*n doubles), the normalize / light-vector results of the fast
 * sqrt/division cores next to the compiler's exact lowering, so the parity suite can pin them bit
 * for bit.  out: 16*n doubles (layout in rt_trace.hip, debug_vec_kernel). */
rt_status rt_debug_vec_ops(rt_context* ctx, const double* v, size_t n, double* out);

/* Test hook: rank 0's assembly step alone (gathered [n][max_rows][row_bytes] host buffer ->
 * image-order [height][row_bytes] host buffer) for row plans the 1-GPU test box cannot run. */
rt_status rt_debug_assemble_rows(rt_context* ctx, const void* gathered, size_t row_bytes,
                                 uint32_t height, uint32_t block, uint32_t n, uint32_t max_rows,
                                 void* image);

/* Test hook: the packet kernel's costliest-first tile order of `scene` seen from cam->position
 * (rt_packet_host.cpp tile_order): *tiles / *waves receive the launch shape (0 when the camera has no
 * order state), `order` (capacity `tiles`) the dispatch order once built, `cost` (capacity
 * tiles*waves) the recorded wave durations (100 MHz ticks); either may be NULL. */
rt_status rt_debug_tile_order(rt_context* ctx, const rt_scene* scene, const rt_camera* cam,
                              uint32_t* order, uint32_t* cost, size_t capacity, uint32_t* tiles,
                              uint32_t* waves, int* state);

/* Test hook (read-only): the packet-kernel frames this context has enqueued so far that read
 * their camera-cone candidate masks from a per-tile table (*with_table) and those whose waves
 * formed their own (*without_table).  RTAMD_PK_CONE_TAB=0 in the environment, read per launch,
 * turns the tables off. */
rt_status rt_debug_cone_table(rt_context* ctx, uint64_t* with_table, uint64_t* without_table);

/* Test hook (read-only): the same count for the shadow-cull masks — frames enqueued with a
 * per-tile, per-light shadow table (*with_table; a tile without a word still forms its own mask)
 * and without one (*without_table).  RTAMD_PK_SHADOW_TAB=0 in the environment, read per launch,
 * turns the shadow tables off, independently of RTAMD_PK_CONE_TAB. */
rt_status rt_debug_shadow_table(rt_context* ctx, uint64_t* with_table, uint64_t* without_table);

/* Test hook (read-only): the same count for the tile class words — frames enqueued with a class
 * word per tile next to their cone and shadow tables (*with_words: the fix-up variant of the
 * packet kernel renders the tiles that see one plane or only sky on its uniform path) and
 * without (*without_words).  They exist only where both tables are formed and passed;
 * RTAMD_PK_TILE_CLASS=0 in the environment, read per launch, turns them off. */
rt_status rt_debug_tile_class(rt_context* ctx, uint64_t* with_words, uint64_t* without_words);

/* Test hook (read-only): the same count for the shadow-plane keep masks — frames enqueued with
 * class words whose per-light masks were formed (*with_masks: the uniform path leaves the planes
 * a mask drops out of its shadow classification) and frames without class words or with all-ones
 * masks (*without_masks).  RTAMD_PK_PLANE_CLEAR=0 in the environment, read per launch, forms
 * all-ones masks. */
rt_status rt_debug_plane_clear(rt_context* ctx, uint64_t* with_masks, uint64_t* without_masks);

/* Test hook (read-only): frames enqueued through the fix-up variant of the packet kernel as a
 * split launch (*split: the uniform tiles in a kernel of their own over the frame's tile list,
 * the general workgroups over theirs) and as its single launch (*single).  A batch is split when
 * every frame has tile lists next to its class words and no tile order applies;
 * RTAMD_PK_TILE_SPLIT=0 in the environment, read per launch, keeps the single launch. */
rt_status rt_debug_tile_split(rt_context* ctx, uint64_t* split, uint64_t* single);

/* Test hook (read-only): frames enqueued through the fix-up variant of the packet kernel with a
 * launch over the frame's list of shadowed-plane tiles (*with: tiles that see one plane and whose
 * shadow rays can meet a sphere, rendered by the uniform kernel's second form between the split
 * launch's two kernels) and without one (*without: the single launch, a split launch whose tables
 * were formed without that list, or a batch none of whose frames has such a tile).
 * RTAMD_PK_TILE_SHADOWED=0 in the environment, read per launch, forms no such list. */
rt_status rt_debug_tile_shadowed(rt_context* ctx, uint64_t* with, uint64_t* without);

/* Test hook (read-only, waits for the context's stream): the pixels the context's last launch of
 * the packet kernel's fix-up variant queued for its fix-up launch (0 before the first one). */
rt_status rt_debug_fixup_count(rt_context* ctx, uint32_t* pixels);

/* Test hook (read-only, waits for the context's stream): the pixels the context's latest adaptive
 * call appended to its list for the list kernel (0 before the first one and with
 * RTAMD_ADAPT_LIST=0). */
rt_status rt_debug_adaptive_listed(rt_context* ctx, uint32_t* pixels);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* RT_CAPI_H */
