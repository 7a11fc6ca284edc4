// rt_internal.hpp — what the C-ABI layer (rt_capi.cpp) and the kernels (rt_trace.hip) share.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstdlib>
#include <vector>

#include "rt_tile_table.hpp"

namespace rtamd {

// Device scene records (doubles per record).  Layout in HBM is one allocation, record arrays
// back to back; the per-ray geometry arrays (sphere/plane/light) are staged into LDS.
constexpr int kSphStride = 4;   // cx cy cz r²            (r² = radius*radius, as Shape.h:77)
constexpr int kPlStride = 8;    // px py pz nx ny nz - -  (normal as stored, Shape.h:142)
constexpr int kTriStride = 12;  // a0(3) e1(3) e2(3) n(3) (translated v0 and edges, Shape.h:204-206;
                                //                         untranslated normal, Shape.h:222-227)
constexpr int kLtStride = 8;    // px py pz Ex Ey Ez - -  (E = color*intensity, Scene.h:110)
constexpr int kMatStride = 8;   // r g b shininess specular transparency ior -
// Planes-only chain kernel (rt_box.hip): one record per plane, in axis-group order —
// p xyz | n xyz | p[k] (k = the group's axis) | 1 when |n| rounds to exactly 1 |
// material (kMatStride - 1 doubles: r g b shininess specular transparency ior) | scene index (int)
constexpr int kBoxRec = 16;
constexpr int kBoxMaxSpheres = 64;  // reflection chains with spheres take rt_box.hip up to this

constexpr int kBvhNodeStride = 8;  // triangle BVH node: lo xyz, hi xyz, {first, count}
constexpr int kBvhMinTris = 32;    // scenes with fewer triangles test them all (no BVH)
constexpr int kBvhStack = 64;      // traversal stack entries (build depth <= 48)
constexpr int kMaxDepth = 16;   // deepest recursion the CHAIN/TREE kernels keep a stack for
// Generic kernels: 256-thread workgroups of 8×32 pixels, so each wave is an 8×8 tile — the
// rays of a square tile stay together down a reflection chain longer than those of a 64-pixel
// row (C1 0.52 → 0.49 ms, mirror -2 %, mesh -4 %; 16×4 waves: C1 0.50 ms).
constexpr int kTileW = 8;       // pixels per workgroup row
constexpr int kTileH = 32;      // rows per workgroup (256 threads: 4 waves of 8×8)

enum PathKind : int {
    kPathDirect = 0,  // no material can spawn a secondary ray: primary + shadow rays only
    kPathChain = 1,   // opaque, some specular > bias: linear reflection chain (≤ maxRecursion)
    kPathTree = 2     // some transparency > 0: refraction + reflection binary tree
};

// Packet kernel frame batches (rt_render_batch): frames of one scene and launch shape, one per
// blockIdx.z, each with its own camera position and the camera-dependent packet-image source.
constexpr int kPkMaxBatch = 32;
struct PkFrame {
    double cam[3];
    const double* img;         // cached LDS image of this camera, or null
    unsigned long long* pub;   // else: the in-launch hand-off slot, or null (form per workgroup)
    uint32_t epoch;
    uint32_t _pad;
};

struct TraceParams {
    // scene (device pointers into the scene allocation)
    const double* sph;
    const double* sph_mat;
    const double* pl;
    const double* pl_mat;
    const double* tri;
    const double* tri_mat;
    const double* lt;
    int32_t ns, np, nt, nl;
    // build-defined area light (samples == 0: none)
    double al_corner[3];
    double al_u[3];
    double al_v[3];
    double al_E[3];        // color * (intensity / samples)
    int32_t al_samples;
    int32_t al_k;          // sqrt(samples)
    // camera
    double cam_pos[3];
    double focal;
    uint32_t width, height;
    int32_t aa;
    int32_t max_rec;
    double bias;
    uint64_t seed;
    // tile
    uint32_t row0, rows;
    uint32_t row_block, row_stride;  // block-cyclic rows (row_block 0: contiguous from row0)
    // outputs (device; any may be null)
    double* out64;
    float* out32;
    uint8_t* ldr;
    int32_t tonemap;
    int32_t _pad;
    unsigned long long* counters;  // [trace, shadow] — only written by the counting variant
    const uint8_t* redo;  // generic kernels: when set, only pixels with a flagged sample run
    const double* bvh;       // triangle BVH nodes (rt_bvh.cpp), or null: test every triangle
    const int32_t* bvh_tri;  // triangle ids in leaf order
    const double* pk_image;  // packet kernel: LDS image of this scene + camera, or null
    // packet kernel, camera without a cached image: the slot the launch's first workgroup
    // publishes its image to ({epoch, word} granules, one per 32-bit image word), or null
    unsigned long long* pk_pub;
    uint32_t pk_epoch;       // this launch's tag (never 0)
    uint32_t pk_pub_first;   // workgroups below this linear index form the image themselves
    // packet kernel, ns >= kSphChunkMin: spatial sphere order and chunk bounds (build_sphere_chunks)
    const int32_t* sph_perm;
    const double* sph_bnd;
    // generic kernels with `redo`: 0 here means no sample overflowed, every workgroup leaves
    const uint32_t* redo_any;
    // packet kernel: the tile each workgroup renders, by dispatch position (costliest first,
    // packet_order_kernel), or null for the default bottom-up order; and, when set, where each
    // wave records its duration (per tile and wave) for the next order
    const uint32_t* tile_order;
    uint32_t* tile_cost;
    // planes-only chain kernel: the box table (kBoxRec doubles per plane) and its group sizes —
    // normal ±e_x, ±e_y, ±e_z, any other
    const double* box;
    int32_t box_n[4];
    // packet kernel, fix-up variants (kFeatFix): undecided shadow rays are not marched; the
    // pixel's output index (frame · frame_px + row-local pixel) is appended to fix_list and
    // packet_fixup_kernel renders it with the exact per-pixel path.  fix_ctl: the list's count
    // for this launch; fix_next: the count the context's NEXT fix-variant launch appends to (the
    // two alternate launch by launch; the fix-up launch zeroes fix_next — nothing reads it until
    // that next launch, ordered after this one — so no completion atomic is needed)
    uint32_t* fix_list;
    uint32_t* fix_ctl;
    uint32_t* fix_next;
    // packet kernel frame batch: nframes > 0 replaces cam_pos / pk_image / pk_pub / pk_epoch
    // by fr[blockIdx.z]; frame z writes its outputs frame_px pixels after frame z - 1's
    uint32_t nframes;
    // host only (rt_debug_plane_clear): the class words handed to this launch carry real
    // shadow-plane keep masks (shadow_plane_keep), not all ones
    uint32_t plane_masks;
    uint64_t frame_px;
    PkFrame fr[kPkMaxBatch];
    // camera-ray terms that are constant over a frame, formed once on the host (camera_consts)
    // and read with scalar loads by the packet kernel: width / 2, height / 2,
    // dz = (cam.z + focal) − cam.z and dz · dz; fr_dz[f] = {dz, dz · dz} of a batch's frame f
    // (after fr[], whose records keep their size: the kernels that do not read these fields
    // see the layout they were tuned with)
    double half_w, half_h, cam_dz, cam_dz2;
    double fr_dz[kPkMaxBatch][2];
    // packet kernel, single-sample variants of up to 64 spheres: the camera-cone candidate mask
    // of every wave tile (rt_cone_table.hpp), one 64-bit word per tile at
    // (tby · gx + tbx) · waves + wave, formed by packet_cone_table_kernel before the launch; null:
    // the wave forms its own.  fr_tab[f]: frame f's of a batch (after fr_dz, as fr_dz after fr[]).
    // These three pointer sets point into one tile table each: rt_tile_table.hpp has its layout
    const unsigned long long* cone_tab;
    const unsigned long long* fr_tab[kPkMaxBatch];
    // the same variants: the shadow-cull candidate masks of every wave tile (rt_shadow_table.hpp),
    // nl 64-bit words per tile at ((tby · gx + tbx) · waves + wave) · nl + light; a word of all
    // ones or a null pointer: the wave forms its own mask (origin_ball + cull_capsule).
    // fr_stab[f]: frame f's
    const unsigned long long* shadow_tab;
    const unsigned long long* fr_stab[kPkMaxBatch];
    // the fix-up variant of those: the class word of every wave tile (tile_class_word,
    // rt_shadow_table.hpp), one per tile at (tby · gx + tbx) · waves + wave — 0: the general
    // path, else the tile sees only sky or only one plane and casts no shadow ray a sphere can
    // meet (pk_uniform_tile).  The class is the
    // word's bits 0-7; bits 8 + 8·l … 15 + 8·l hold light l's shadow-plane keep mask
    // (shadow_plane_keep; all ones: every plane is classified), on general tiles too, so readers
    // test tile_class_of(word).  Null: no tile is classified.  fr_ctab[f]: frame f's
    const unsigned long long* class_tab;
    const unsigned long long* fr_ctab[kPkMaxBatch];
};
// The fix-up variant's split launch of a frame batch (packet_uniform_kernel and
// packet_direct_kernel's kFeatSplit twin, rt_packet.hip): every frame's class words are followed
// by its tile lists (rt_tile_table.hpp, TileTabLayout::Lists); tiles == 0: no lists, one
// launch as before.  uni_n and gen_n: the uniform tiles and general workgroups the two launches
// cover per frame — the largest count of the batch's frames where the host knows them, every
// tile or workgroup where it does not.  sh_n: the same for the shadowed-plane tiles
// (packet_uniform_kernel<true>, between the two; 0 where the tables were formed without that
// list).  Host only: TraceParams keeps its size and layout.
struct PkSplit {
    uint32_t tiles;
    uint32_t uni_n, gen_n;
    uint32_t sh_n;
};
// the runtime passes at most 4 KiB of kernel arguments (packet_image_batch_kernel and
// packet_cone_table_kernel take a job list of kPkMaxBatch pointers and ints next to it)
static_assert(sizeof(TraceParams) + 12 * kPkMaxBatch + 32 <= 4096, "kernel arguments above 4 KiB");

// Camera::getRay's frame constants (Math.h:99-121): the single IEEE double operations of the
// device expression, in its order, so a kernel that reads them computes the bits it computed
// itself — sx = x − W/2, sy = H/2 − y, d = (sx − cam.x, sy − cam.y, dz), |d|² = (…) + dz·dz.
struct CameraConsts {
    double half_w, half_h, dz, dz2;
};
inline CameraConsts camera_consts(uint32_t width, uint32_t height, double cam_z, double focal) {
    CameraConsts c;
    c.half_w = static_cast<double>(width) / 2.0;
    c.half_h = static_cast<double>(height) / 2.0;
    c.dz = (cam_z + focal) - cam_z;  // not focal: the sum is rounded first
    c.dz2 = c.dz * c.dz;
    return c;
}

// Host: the spatial sphere chunks of the packet kernel's culls (rt_bvh.cpp): perm[sorted] =
// original index, bounds = one bounding sphere (cx cy cz R) per 64 sorted spheres.
constexpr int kSphChunkMin = 65;  // scenes with fewer spheres have a single chunk (no order)
void build_sphere_chunks(const double* sph, int ns, std::vector<int32_t>& perm,
                         std::vector<double>& bounds);

// Host: builds the triangle BVH over the uploaded triangle records (kTriStride doubles each).
void build_triangle_bvh(const double* tri, int nt, std::vector<double>& nodes,
                        std::vector<int32_t>& order);

// Doubles of the scene image the generic kernels stage into LDS (spheres, planes, lights).
__host__ __device__ inline size_t scene_doubles(const TraceParams& p) {
    return static_cast<size_t>(kSphStride) * p.ns + static_cast<size_t>(kPlStride) * p.np +
           static_cast<size_t>(kLtStride) * p.nl;
}

// sample_parallel: multi-sample frames (2 ≤ aa ≤ kAaParallelMax) of the direct and chain paths
// trace one sample per thread (rt_trace.hip), the same image as the per-thread sample loop
constexpr int kAaParallelMax = 128;
hipError_t launch_trace(const TraceParams& p, int path, bool count, bool lds, size_t lds_bytes,
                        hipStream_t stream, bool sample_parallel = false);
namespace lean {  // rt_trace_lean.hip: the same kernels for scenes without triangles / area light
hipError_t launch_trace(const TraceParams& p, int path, bool count, bool lds, size_t lds_bytes,
                        hipStream_t stream, bool sample_parallel = false);
}
hipError_t launch_box_chain(const TraceParams& p, bool count, bool sample_parallel,
                            hipStream_t stream);
hipError_t launch_packet_direct(const TraceParams& p, bool count, bool any_specular,
                                hipStream_t stream, const PkSplit* split = nullptr);
size_t packet_lds_bytes(int ns, int np, int nl);
hipError_t launch_packet_image(const TraceParams& p, double* img, hipStream_t stream);
// Whether launch_packet_direct takes a fix-up variant for p (then p.fix_list / p.fix_ctl must be
// set, with room for every output pixel of the launch), and the fix-up launch that follows it.
bool packet_uses_fixup(const TraceParams& p, bool count, bool any_specular);
hipError_t launch_packet_fixup(const TraceParams& p, hipStream_t stream);
// The images a frame batch forms before its launch: job j forms frame frame[j]'s image
// (camera p.fr[frame[j]].cam) at dst[j] — a cache entry of the scene or a slot of its ring.
struct PkImageJobs {
    double* dst[kPkMaxBatch];
    int32_t frame[kPkMaxBatch];
    int32_t n;
};
hipError_t launch_packet_image_batch(const TraceParams& p, const PkImageJobs& jobs,
                                     hipStream_t stream);
// The tile tables (rt_tile_table.hpp) one launch forms: job j writes the table of frame frame[j]
// (-1: the one-frame launch's camera, p.cam_pos / p.pk_image) to dst[j], reading the frame's
// packet image, formed earlier on the stream; every job's table holds `contents`.
struct PkConeJobs {
    unsigned long long* dst[kPkMaxBatch];
    int32_t frame[kPkMaxBatch];
    int32_t n;
    TileTabContents contents;
};
// host[j], when set, points at the two pinned host words that receive job j's list counts once
// the table is formed (tile_list_counts_encode)
struct PkListCounts {
    unsigned long long* host[kPkMaxBatch];
};
hipError_t launch_packet_cone_tables(const TraceParams& p, const PkConeJobs& jobs,
                                     hipStream_t stream, const PkListCounts* counts = nullptr);
// An RTAMD_PK_* switch as set now (-1: unset), and whether it is set to 0 — "off"; read per
// launch: the tests flip the switches between launches.
inline int packet_switch(const char* name) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : -1;
}
inline bool packet_switch_off(const char* name) { return packet_switch(name) == 0; }
// Whether a launch of p may take the split launch at all (RTAMD_PK_TILE_SPLIT, read per launch,
// a tile grid whose columns and rows a list entry can name, one wave row per workgroup and no
// tile order: an order names dispatch positions, a list tiles), and the two launches
// themselves: launch_packet_direct takes them when split->tiles is set.
bool packet_split_wanted(const TraceParams& p);
// Whether p's launch is served by a variant that reads a cone table.
bool packet_reads_cone_table(const TraceParams& p, bool any_specular);
// Lights per tile of the shadow table such a launch's scene gets (0: none, rt_shadow_table.hpp).
int packet_shadow_table_lights(const TraceParams& p);
// The packet kernel's launch shape for p (grid of workgroups, waves per workgroup), and the
// costliest-first tile order built from the wave durations a launch of that shape recorded.
void packet_grid(const TraceParams& p, uint32_t& gx, uint32_t& gy, uint32_t& waves);
hipError_t launch_packet_order(const uint32_t* cost, uint32_t gx, uint32_t gy, uint32_t waves,
                               uint32_t* keys, uint32_t* order, uint32_t* verdict,
                               hipStream_t stream);
int packet_max_spheres();
// G-buffer pass (rt_gbuffer.hip): per pixel, IntersectClosest of the unjittered camera ray.
// Device outputs, any may be null; rows-local like TraceParams.out64, frame f (p.fr[f].cam,
// p.nframes >= 1) at f * p.frame_px pixels of each.
struct GbOut {
    double* depth;      // [px]    HitInfo::distance, +inf on a miss
    float* depth_norm;  // [px]    (float)((t - near) / (far - near)) of the frame's camera
    double* normal;     // [px][3] geometric normal, as rt_intersect_rays
    int32_t* prim;      // [px][2] {type, index}
    float* albedo;      // [px][3] (float)material.color
    double planes[kPkMaxBatch][2];  // frame f's camera {near_plane, far_plane}
};
// Whether the packet kernel serves p (its LDS image without light records fits lds_limit).
bool gbuffer_packet_fits(const TraceParams& p, size_t lds_limit);
// packet: gbuffer_packet_kernel (p.nl must be 0: the image is laid out without lights), else
// gbuffer_generic_kernel.  tile_w: 8 (8×8 px per wave) or 16 (16×4), 0: the default.
hipError_t launch_gbuffer(const TraceParams& p, const GbOut& g, bool packet, int tile_w,
                          hipStream_t stream);
hipError_t launch_trace_rays(const TraceParams& p, int path, bool count, const double* rays,
                             size_t n, double* out, hipStream_t stream);
hipError_t launch_intersect_rays(const TraceParams& p, const double* rays, size_t n, double* out,
                                 hipStream_t stream);
// Any-hit query (rt_anyhit.hip): per ray, 1 iff a primitive lies at 0 < t < max_dist[i].
hipError_t launch_occluded_rays(const TraceParams& p, const double* rays, const double* max_dist,
                                size_t n, uint8_t* out, hipStream_t stream);
// The keys of the build-defined area light's draws, for the per-level queries below.  Each
// launch takes `keys`: null is the un-keyed kernel (point lights only); with keys, and only for
// p.al_samples > 0, the keyed_ kernel, which serves the area light's samples after the point
// lights.  keys->pixel: n device keys, or null (element i draws with pixel = i); the draws are
// keyed (p.seed, pixel, 0x10000 + (sample << 6) + depth, 2s | 2s + 1) as direct_terms keys them.
struct AreaKeyArgs {
    const unsigned long long* pixel;
    uint32_t sample;
    uint32_t depth;
};
// Transmittance queries (rt_transmit.hip): per ray, computeTransmittance(ray, max_dist[i], p.bias);
// per point {p, normal} and point light l, directLightning's shadow ray, out[i * p.nl + l] — with
// keys served, nl + al_samples columns per point, the samples after the lights.
// opaque: the scene has no transparent material (the variant that asks occlusion_opaque first).
hipError_t launch_transmittance_rays(const TraceParams& p, bool opaque, const double* rays,
                                     const double* max_dist, size_t n, double* out,
                                     hipStream_t stream);
hipError_t launch_light_transmittance(const TraceParams& p, bool opaque, const double* points,
                                      const AreaKeyArgs* keys, size_t n, double* out,
                                      hipStream_t stream);
// Direct-lighting queries (rt_direct.hip): directLightning (Scene.h:79-129) over the scene's
// lights, per point {p, normal, view} with a material of rt_material's layout (materials: one per
// point, or null: `shared` for all of them), and per ray at its closest hit with the hit
// primitive's material (a miss writes zeros).  Each output is [n][3] doubles, or null: not written.
struct DlOut {
    double* radiance;  // color * diffuse + specular * material.specular (Scene.h:126-128)
    double* diffuse;   // diffuseAccumulation
    double* specular;  // specularAccumlation
};
struct DlMaterial {
    double v[8];  // r g b shininess specular transparency ior -
};
hipError_t launch_direct_light_points(const TraceParams& p, bool opaque, const double* points,
                                      const double* materials, const DlMaterial& shared,
                                      const AreaKeyArgs* keys, size_t n, const DlOut& out,
                                      hipStream_t stream);
hipError_t launch_direct_light_rays(const TraceParams& p, bool opaque, const double* rays,
                                    const AreaKeyArgs* keys, size_t n, const DlOut& out,
                                    hipStream_t stream);
// Scatter query (rt_scatter.hip): one TraceRay level (Scene.h:131-198) per ray, before its
// children are traced — shade_hit's Node written out.  p.max_rec <= 0: every ray is at the
// recursion limit (sky, no intersection).  keys are served only with out.value set.  A null
// output is not written; at least one is set.
struct ScOut {
    double* value;         // [n][3] sky on a miss, else localLight * (1 - transparency)
    double* refract_rays;  // [n][6] {o, d}, zeros where absent
    double* reflect_rays;  // [n][6] {o, d}, zeros where absent
    double* weights;       // [n][2] {fw, rw}, zero where the child is absent
    uint8_t* flags;        // [n]    bit 0 hit, bit 1 refraction ray, bit 2 reflection ray
};
hipError_t launch_scatter_rays(const TraceParams& p, bool opaque, const double* rays,
                               const AreaKeyArgs* keys, size_t n, const ScOut& out,
                               hipStream_t stream);
// Camera rays (rt_camera_rays.hip): Camera::getRay(x, y, sample > 0 && p.aa > 1) for every pixel
// of p's row set, {o, d} per pixel at its rows-local index; the jitter key is the render
// kernels' (p.seed, y_image * W + x, sample).  out: p.rows * p.width * 6 doubles.
hipError_t launch_camera_rays(const TraceParams& p, int sample, double* out, hipStream_t stream);
// Closest-hit query (rt_closest.hip): IntersectClosest per ray, each output a plane of its own.
// A null output is not written; at least one is set.  A miss: t = +inf, prim = {0, -1}, +0.0
// elsewhere.
struct ChOut {
    double* t;         // [n]    HitInfo::distance
    int32_t* prim;     // [n][2] {type, index}
    double* normal;    // [n][3] geometric normal, as rt_intersect_rays
    double* point;     // [n][3] o + d * t
    double* material;  // [n][7] the hit primitive's material, rt_material's member order
};
hipError_t launch_closest_rays(const TraceParams& p, const double* rays, size_t n, const ChOut& out,
                               hipStream_t stream);
// Progressive frames (rt_accumulate.hip).  launch_accumulate_samples: for every pixel of p's row
// set, sum = (s0 == 0 ? +0.0 : sum) + TraceRay(camera ray of sample s) for s in [s0, s1) in
// order, with the render kernels' keys (pix = y_image * W + x, s) for the jitter and the area
// light; sum: p.rows * p.width * 3 doubles, rows-local.  launch_resolve: per pixel sum / samples,
// written as doubles, floats and tonemapped bytes (op in [0, 7), or 7: seven planes in
// tonemapAll() order; op is read only with ldr set); a null output is not written.
hipError_t launch_accumulate_samples(const TraceParams& p, int path, int s0, int s1, double* sum,
                                     hipStream_t stream);
hipError_t launch_resolve(const double* sum, size_t n, int samples, int op, double* out64,
                          float* out32, uint8_t* ldr, hipStream_t stream);
// Adaptive progressive frames (rt_adaptive.hip).  The rule of rt_accumulate_adaptive_device
// (rt_capi.h) over the pixels of p's row set, on the rows-local state sum (3 doubles a pixel),
// moments (2) and count (int32): each pixel continues from its count while the rule wants a
// sample, up to sample_end.  fresh: the state is not read.  list / list_count: a list of
// p.rows * p.width row-local pixel indices and its count, zero before the launch — the tile
// kernel appends the pixels its waves leave unfinished, the list kernel (launched after it)
// finishes them; list == null: the tile kernel finishes every pixel, one launch.
struct AdaptiveArgs {
    double tolerance, lum_floor;
    int32_t min_samples, sample_end, fresh;
    double* sum;
    double* moments;
    int32_t* count;
    uint32_t* list;
    uint32_t* list_count;
};
hipError_t launch_accumulate_adaptive(const TraceParams& p, int path, const AdaptiveArgs& a,
                                      hipStream_t stream);
// launch_resolve with each pixel's own count as the divisor; a count of 0: the pixel is {0,0,0}.
hipError_t launch_resolve_counts(const double* sum, const int32_t* count, size_t n, int op,
                                 double* out64, float* out32, uint8_t* ldr, hipStream_t stream);
hipError_t launch_tonemap(const double* hdr, size_t n, int op, uint8_t* out, hipStream_t stream);
hipError_t launch_debug_f64(const double* x, const double* y, size_t n, double* out,
                            hipStream_t stream);
hipError_t launch_debug_vec(const double* v, size_t n, double* out, hipStream_t stream);

}  // namespace rtamd
