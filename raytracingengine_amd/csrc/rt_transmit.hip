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
// Lights are read by the light kernel only; the area light by neither (keyed_shadow_points_kernel,
// rt_area_queries.hip, answers for its samples).
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

// One thread per point {p, normal}: 6 doubles in, nl doubles out at [i][l].  The light loop's
// trip count is nl for the whole wave (the records through the scalar cache); the three skips are
// directLightning's `continue`s (Scene.h:89, 92, 95) and answer 0.0.
template <bool OPAQUE>
__global__ __launch_bounds__(256) void light_transmittance_kernel(TraceParams P,
                                                                  const double* __restrict__ points,
                                                                  size_t n, double* __restrict__ out) {
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* q = points + 6 * i;
    const d3 p = mk(q[0], q[1], q[2]);
    const d3 normal = unit(mk(q[3], q[4], q[5]));  // Scene.h:81
    const double bias = P.bias;
    double* w = out + static_cast<size_t>(S.nl) * i;
    for (int l = 0; l < S.nl; ++l) {
        const double* lt = S.lt + kLtStride * l;
        double dist, inv_d2;
        d3 L;
        light_dir(mk(lt[0], lt[1], lt[2]) - p, dist, L, inv_d2);
        double T = 0.0;
        if (!(dist <= 0.0) && !(smax(0.0, dot(normal, L)) <= 0.0) && !(dist <= bias))
            T = transmit_ray<OPAQUE>(S, p + normal * bias, L, dist - bias, bias);
        w[l] = T;
    }
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

hipError_t launch_light_transmittance(const TraceParams& p, bool opaque, const double* points,
                                      size_t n, double* out, hipStream_t stream) {
    if (n == 0 || p.nl == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    if (opaque)
        hipLaunchKernelGGL(light_transmittance_kernel<true>, grid, block, 0, stream, p, points, n,
                           out);
    else
        hipLaunchKernelGGL(light_transmittance_kernel<false>, grid, block, 0, stream, p, points,
                           n, out);
    return hipGetLastError();
}

}  // namespace rtamd
