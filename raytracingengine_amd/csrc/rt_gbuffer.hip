// rt_gbuffer.hip — the full-frame G-buffer pass: per pixel the camera ray's HitInfo, i.e.
// Scene::CalculatePixelDepth(x, y, false) (Scene.h:278-281) = IntersectClosest(camera.getRay(x, y,
// false)), written out as depth (HitInfo::distance), normalised depth (HitInfo::normalizedDistance,
// Shape.h:40-42), geometric normal, primitive {type, index} and base colour.
//
// Primary visibility does not depend on materials, so the packet machinery of
// rt_packet_device.hpp (the camera-constant LDS image, cull_cone, closest_camera) serves every
// scene type here — chains and trees too — without its light records, shadow code or tonemap:
//
//  * gbuffer_packet_kernel<MAXC, TRIS, TW>: one wave = one TW × 64/TW pixel tile, for scenes
//    inside the packet limits (≤ packet_max_spheres() spheres, image within the LDS limit).
//  * gbuffer_generic_kernel: one thread per pixel over closest() / normal_of() of
//    rt_trace_common.hpp, for every other scene and for RT_FLAG_GENERIC_KERNEL (the in-tree A/B
//    partner of the packet kernel).
//
// Both produce the bits rt_intersect_rays returns for the same ray: the same roots, plane
// quotients and triangle tests in the reference's order (the packet kernel only skips candidates
// that provably cannot win, rt_packet_device.hpp), the same hit point cam + d·t and unit(p − C).
#include "rt_packet_device.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// Waves per SIMD the packet variants are compiled for: the no-triangle ≤ 64-sphere variant is a
// strict subset of packet_direct_kernel<1, 0, …> (6: at most 80 VGPRs + AGPRs), the triangle
// variants keep the shaded kernel's budget.
constexpr int gb_waves(int MAXC, bool TRIS) {
    return TRIS ? RT_PACKET_TRIS_WAVES : (MAXC == 1 ? RT_PACKET_SMALL_WAVES : RT_PACKET_AA1_WAVES);
}

// The requested stores of one pixel (o: its rows-local index in the batch).  Null pointers are
// wave-uniform kernel arguments: scalar branches.
__device__ __forceinline__ void gb_store(const GbOut& G, int frame, size_t o, bool hit, double t,
                                         d3 n, int kind, int idx, const double* mat) {
    if (G.depth) G.depth[o] = hit ? t : INFINITY;
    if (G.depth_norm) {
        // HitInfo::normalizedDistance (Shape.h:41), in double, then rounded to float
        const double near_plane = G.planes[frame][0], far_plane = G.planes[frame][1];
        const double dn = (t - near_plane) / (far_plane - near_plane);
        G.depth_norm[o] = hit ? static_cast<float>(dn) : INFINITY;
    }
    if (G.normal) {
        G.normal[3 * o + 0] = hit ? n.x : 0.0;
        G.normal[3 * o + 1] = hit ? n.y : 0.0;
        G.normal[3 * o + 2] = hit ? n.z : 0.0;
    }
    if (G.prim) reinterpret_cast<int2*>(G.prim)[o] = make_int2(hit ? kind : 0, hit ? idx : -1);
    if (G.albedo) {
        G.albedo[3 * o + 0] = hit ? static_cast<float>(mat[0]) : 0.0f;
        G.albedo[3 * o + 1] = hit ? static_cast<float>(mat[1]) : 0.0f;
        G.albedo[3 * o + 2] = hit ? static_cast<float>(mat[2]) : 0.0f;
    }
}

// Workgroup: kWgWavesX waves in x, blockDim.x / (64 · kWgWavesX) in y (1 or 2, by the size of the
// LDS image like the shaded kernel); grid z = the frame of the batch.
template <int MAXC, bool TRIS, int TW>
__global__ __launch_bounds__(256, gb_waves(MAXC, TRIS)) void gbuffer_packet_kernel(TraceParams P,
                                                                                   GbOut G) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int TH = 64 / TW;
    constexpr int FEAT = TRIS ? kFeatTris : 0;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int ns = P.ns, np = P.np, nl = P.nl, nb = pk_chunk_bounds(ns), nsb = ns + nb;
    // (the image layout: pk_build_image, rt_packet_device.hpp, is the format's definition)
    double* s_sph = smem;
    double* s_pl = s_sph + kPkSph * nsb;
    double* s_pln = s_pl + kPlStride * np + kLtStride * nl;
    const int32_t* s_orig = reinterpret_cast<const int32_t*>(s_pln + 4 * np);
    const double* camp = P.fr[blockIdx.z].cam;
    const uint64_t frame_off = static_cast<uint64_t>(blockIdx.z) * P.frame_px;
    const d3 cam = mk(camp[0], camp[1], camp[2]);
    pk_build_image(P, camp, smem, tid, nthreads);
    __syncthreads();

    PacketScene S;
    S.sph = s_sph;
    S.pl = s_pl;
    S.lt = nullptr;
    S.tri = P.tri;
    S.mat = P.sph_mat;
    S.bvh = P.bvh;
    S.bvh_tri = P.bvh_tri;
    S.ns = ns;
    S.np = np;
    S.nt = P.nt;
    S.nl = nl;
    S.nb = nb;
    S.orig = nb ? s_orig : nullptr;
    S.wstk = nullptr;
    if constexpr (TRIS)  // after the image: kPkStack ints per wave
        S.wstk = reinterpret_cast<int*>(smem + pk_image_bytes(ns, np, nl) / 8) + kPkStack * (tid >> 6);
    const int nchunks = (ns + 63) / 64;

    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t x = blockIdx.x * (TW * kWgWavesX) + (wave % kWgWavesX) * TW + (lane % TW);
    const uint32_t yl = blockIdx.y * (TH * (nthreads / (64 * kWgWavesX))) +
                        (wave / kWgWavesX) * TH + (lane / TW);
    const bool valid = x < P.width && yl < P.rows;
    // lanes past the image edge trace a clamped in-image ray: they take part in the cone's
    // reductions (a superset bound is still conservative) and write nothing
    const uint32_t xc = x < P.width ? x : P.width - 1;
    const uint32_t y = image_row(P, yl < P.rows ? yl : P.rows - 1);
    // Camera::getRay(x, y, false) (Math.h:99-121): sample 0 is never jittered
    const d3 d = camera_dir(P, cam, xc, y, 0, 0);
    // camera cone: axis = the tile's centre-lane direction, half-angle from the wave minimum of
    // the per-lane cosines (packet_direct_kernel's bound)
    const d3 axis = lane_d3(d, (TH / 2) * TW + TW / 2);
    const double cos_min = static_cast<double>(wave_red<0>(static_cast<float>(dot(d, axis)))) - 1e-7;
    const bool ok = isfinite(cos_min) && cos_min > 0.0;
    const Masks<MAXC> M = ok ? cull_cone<MAXC>(S, axis, cos_min) : all_candidates<MAXC>(ns);
    PkHit h;
    h.t = 0.0;
    h.prim = 0;
    const bool hit = valid && closest_camera<MAXC, FEAT>(S, M, nchunks, cam, d, h);
    if (!valid) return;
    d3 n = mk(0.0, 0.0, 0.0);
    int kind = 0, idx = -1;
    const double* mat = S.mat;
    if (hit) {
        n = pk_normal(S, h, cam + d * h.t);
        mat = pk_material<MAXC>(S, h);
        if (h.prim < ns) {
            kind = 1;
            idx = h.prim;
            if constexpr (MAXC > 1) idx = s_orig[h.prim];  // chunk order -> the scene's index
        } else if (h.prim < ns + np) {
            kind = 2;
            idx = h.prim - ns;
        } else {
            kind = 3;
            idx = h.prim - ns - np;
        }
    }
    gb_store(G, blockIdx.z, frame_off + static_cast<size_t>(yl) * P.width + x, hit, h.t, n, kind, idx, mat);
}

// One thread per pixel, a wave = 64 consecutive pixels of a row (each 8-byte output goes out as
// 512 contiguous bytes per wave instruction).
constexpr int kGbGenW = 64, kGbGenH = 4;
__global__ __launch_bounds__(kGbGenW * kGbGenH) void gbuffer_generic_kernel(TraceParams P,
                                                                            GbOut G) {
    const uint32_t x = blockIdx.x * kGbGenW + threadIdx.x;
    const uint32_t yl = blockIdx.y * kGbGenH + threadIdx.y;
    if (x >= P.width || yl >= P.rows) return;
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);  // the records in HBM, no staging
    const double* camp = P.fr[blockIdx.z].cam;
    const d3 cam = mk(camp[0], camp[1], camp[2]);
    const d3 d = camera_dir(P, cam, x, image_row(P, yl), 0, 0);
    Hit h;
    const bool hit = closest(S, cam, d, h);
    d3 n = mk(0.0, 0.0, 0.0);
    const double* mat = S.sph_mat;
    if (hit) {
        n = normal_of(S, h, cam + d * h.t);
        mat = material_of(S, h);
    }
    const size_t o = static_cast<uint64_t>(blockIdx.z) * P.frame_px +
                     static_cast<size_t>(yl) * P.width + x;
    gb_store(G, blockIdx.z, o, hit, h.t, n, h.kind, h.idx, mat);
}

// The packet image without light records (the launcher's callers set p.nl = 0).
bool gbuffer_packet_fits(const TraceParams& p, size_t lds_limit) {
    return p.ns <= packet_max_spheres() && pk_image_bytes(p.ns, p.np, 0) <= lds_limit;
}

// Default tile of the packet kernel: 8×8 or 16×4 pixels per wave (the store-shape A/B of
// DESIGN.md §4; RTAMD_GB_TILE=8|16 overrides it for A/B runs).
#ifndef RT_GB_TILE_W
#define RT_GB_TILE_W 16
#endif

template <int MAXC, bool TRIS, int TW>
static void launch_gb_packet(const TraceParams& p, const GbOut& g, hipStream_t stream) {
    size_t lds = pk_image_bytes(p.ns, p.np, p.nl);
    const unsigned wgy = pk_wgy(lds);
    const dim3 block(64 * kWgWavesX * wgy);
    if constexpr (TRIS) lds += sizeof(int) * kPkStack * (block.x / 64);
    constexpr unsigned TH = 64 / TW;
    const dim3 grid((p.width + TW * kWgWavesX - 1) / (TW * kWgWavesX),
                    (p.rows + TH * wgy - 1) / (TH * wgy), p.nframes);
    hipLaunchKernelGGL((gbuffer_packet_kernel<MAXC, TRIS, TW>), grid, block, lds, stream, p, g);
}

template <int MAXC, bool TRIS>
static void launch_gb_tile(const TraceParams& p, const GbOut& g, int tile_w, hipStream_t stream) {
    if (tile_w == 8) launch_gb_packet<MAXC, TRIS, 8>(p, g, stream);
    else launch_gb_packet<MAXC, TRIS, 16>(p, g, stream);
}

template <int MAXC>
static void launch_gb_maxc(const TraceParams& p, const GbOut& g, int tile_w, hipStream_t stream) {
    if (p.nt > 0) launch_gb_tile<MAXC, true>(p, g, tile_w, stream);
    else launch_gb_tile<MAXC, false>(p, g, tile_w, stream);
}

hipError_t launch_gbuffer(const TraceParams& p, const GbOut& g, bool packet, int tile_w,
                          hipStream_t stream) {
    if (p.nframes < 1 || p.nframes > static_cast<uint32_t>(kPkMaxBatch) || p.width == 0 ||
        p.rows == 0)
        return hipErrorInvalidValue;
    if (!packet) {
        const dim3 block(kGbGenW, kGbGenH);
        const dim3 grid((p.width + kGbGenW - 1) / kGbGenW, (p.rows + kGbGenH - 1) / kGbGenH,
                        p.nframes);
        hipLaunchKernelGGL(gbuffer_generic_kernel, grid, block, 0, stream, p, g);
        return hipGetLastError();
    }
    if (p.nl != 0) return hipErrorInvalidValue;
    if (tile_w == 0) {
        const char* e = std::getenv("RTAMD_GB_TILE");  // read per launch (A/B runs switch it)
        tile_w = e ? std::atoi(e) : RT_GB_TILE_W;
    }
    if (tile_w != 8 && tile_w != 16) return hipErrorInvalidValue;
    const int chunks = (p.ns + 63) / 64;
    if (chunks <= 1) launch_gb_maxc<1>(p, g, tile_w, stream);
    else if (chunks <= 4) launch_gb_maxc<4>(p, g, tile_w, stream);
    else launch_gb_maxc<16>(p, g, tile_w, stream);
    return hipGetLastError();
}

}  // namespace rtamd
