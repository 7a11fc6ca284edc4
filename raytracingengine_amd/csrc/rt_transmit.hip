// rt_transmit.hip — the batch transmittance queries for gfx950 (MI355X):
// Scene::computeTransmittance (Scene.h:35-77) for n arbitrary rays, and the shadow rays of
// Scene::directLightning (Scene.h:86-104) from n surface points to every point light.
//
// Both kernels run the march of the render kernels, transmittance (rt_trace_common.hpp): closest
// hits over closest's sphere and plane loops (trip counts ns and np for the whole wave, so the
// records arrive through the scalar cache) and the triangle BVH or, without one, the plain
// triangle loop; every t in binary64 in the reference's operation order, ties to the lowest scene
// index, materials read for the transparency only.  A lane that has left the march is masked off
// and the wave leaves it once no lane is marching.
// OPAQUE (no material of the scene is transparent, so T is 0 or 1 and the first counted hit
// decides it): occlusion_opaque classifies the lane first and only the lanes it leaves undecided
// (-1: triangles, roots near a threshold, values out of range) march — light_term's pair.
// Lights are read by the light body only: the point lights, and with AREA (rt_query_out.hpp, the
// keyed_ kernel) the build-defined area light's samples after them.
#include "rt_query_out.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// One thread per ray: 7 doubles in (the ray and its max_dist), one double out.
template <bool OPAQUE>
__global__ __launch_bounds__(256) void transmittance_rays_kernel(TraceParams P,
                                                                 const double* __restrict__ rays,
                                                                 const double* __restrict__ max_dist,
                                                                 size_t n, double* __restrict__ out) {
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + 6 * i;
    out[i] = transmit_ray<OPAQUE>(S, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), max_dist[i],
                                  P.bias);
}

// One thread per point {p, normal}: 6 doubles in, nl + al doubles out at [i][c] — the point lights
// in scene order, then (AREA) the area samples in stratum order.  The light loop's trip count is
// nl for the whole wave (the records through the scalar cache).
template <bool AREA, bool OPAQUE>
__device__ __forceinline__ void light_points_body(const TraceParams& P, const double* points,
                                                  const AreaKeyArgs& keys, size_t n, double* out) {
    SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    if constexpr (!AREA) S.al = 0;
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* q = points + 6 * i;
    const d3 p = mk(q[0], q[1], q[2]);
    const d3 normal = unit(mk(q[3], q[4], q[5]));  // Scene.h:81
    const double bias = P.bias;
    double* w = out + (static_cast<size_t>(S.nl) + static_cast<size_t>(S.al)) * i;
    for (int l = 0; l < S.nl; ++l) {
        const double* lt = S.lt + kLtStride * l;
        w[l] = shadow_T<OPAQUE>(S, p, normal, mk(lt[0], lt[1], lt[2]), bias);
    }
    if constexpr (AREA) {
        const uint64_t pix = pixel_key(keys, i);
        const uint32_t stream = area_stream(keys.sample, static_cast<int>(keys.depth));
        for (int s = 0; s < S.al; ++s)
            w[S.nl + s] = shadow_T<OPAQUE>(S, p, normal, area_point(P, pix, stream, s), bias);
    }
}

template <bool OPAQUE>
__global__ __launch_bounds__(256) void light_transmittance_kernel(TraceParams P,
                                                                  const double* __restrict__ points,
                                                                  size_t n, double* __restrict__ out) {
    light_points_body<false, OPAQUE>(P, points, AreaKeyArgs{}, n, out);
}

template <bool OPAQUE>
__global__ __launch_bounds__(256) void keyed_shadow_points_kernel(TraceParams P,
                                                                  const double* __restrict__ points,
                                                                  AreaKeyArgs keys, size_t n,
                                                                  double* __restrict__ out) {
    light_points_body<true, OPAQUE>(P, points, keys, n, out);
}

hipError_t launch_transmittance_rays(const TraceParams& p, bool opaque, const double* rays,
                                     const double* max_dist, size_t n, double* out,
                                     hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    if (opaque)
        hipLaunchKernelGGL(transmittance_rays_kernel<true>, grid, block, 0, stream, p, rays,
                           max_dist, n, out);
    else
        hipLaunchKernelGGL(transmittance_rays_kernel<false>, grid, block, 0, stream, p, rays,
                           max_dist, n, out);
    return hipGetLastError();
}

namespace {

template <bool OPAQUE>
void launch_light_points(const TraceParams& p, const double* points, const AreaKeyArgs* keys,
                         size_t n, double* out, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    if (keys)
        hipLaunchKernelGGL(keyed_shadow_points_kernel<OPAQUE>, grid, block, 0, stream, p, points,
                           *keys, n, out);
    else
        hipLaunchKernelGGL(light_transmittance_kernel<OPAQUE>, grid, block, 0, stream, p, points,
                           n, out);
}

}  // namespace

// keys: served only for a scene with an area light attached; null, or no area light: the
// un-keyed kernel, which has nothing to write without a point light.
hipError_t launch_light_transmittance(const TraceParams& p, bool opaque, const double* points,
                                      const AreaKeyArgs* keys, size_t n, double* out,
                                      hipStream_t stream) {
    if (p.al_samples <= 0) keys = nullptr;
    if (n == 0 || (!keys && p.nl == 0)) return hipSuccess;
    if (opaque)
        launch_light_points<true>(p, points, keys, n, out, stream);
    else
        launch_light_points<false>(p, points, keys, n, out, stream);
    return hipGetLastError();
}

}  // namespace rtamd
