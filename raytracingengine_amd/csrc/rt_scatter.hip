// rt_scatter.hip — the batch scatter query for gfx950 (MI355X): one level of Scene::TraceRay
// (Scene.h:131-198) for n caller-supplied rays, "before its children are traced": what the level
// adds (the sky on a miss, localLight * (1 - transparency) on a hit), the refraction and the
// reflection ray it would trace next, their weights and which of them exist.
//
// The body is closest + shade_hit (rt_trace_common.hpp), the render kernels' own TraceRay step,
// and sky for a miss and for a ray at the recursion limit; the kernel only writes the Node out.
// Nothing of Scene.h is restated here, so the bits are the renderer's.  TREE (some material of
// the scene is transparent) selects what it selects in the render kernels: the Fresnel /
// refraction code, and with TREE == false occlusion_opaque before each shadow march.  DIRECT and
// CHILDREN are shade_hit's: without RT_SC_VALUE the light loop is not compiled in, without any of
// the child outputs (rays, weights, flags) the child-ray code is not.
// AREA (rt_query_out.hpp): keyed_scatter_kernel passes the caller's keys through, so direct_terms'
// own sample loop runs; DIRECT is always on there (a launch without the value does not depend on
// the keys).  The un-keyed kernel's SceneView says the scene has no area light, so that loop, and
// its second inlined light_term, is not compiled into it at all.
#include "rt_query_out.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// One thread per ray {o, d}.  P.max_rec <= 0: the ray is at the recursion limit (Scene.h:132-134),
// nothing is intersected.
template <bool AREA, bool TREE, bool DIRECT, bool CHILDREN>
__device__ __forceinline__ void scatter_body(const TraceParams& P, const double* rays,
                                             const AreaKeyArgs& keys, size_t n, const ScOut& out) {
    SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    if constexpr (!AREA) S.al = 0;
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + 6 * i;
    const d3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    Hit h;
    if (P.max_rec <= 0 || !closest(S, o, d, h)) {
        sc_store_node<CHILDREN>(out, i, sky_node(d));
        return;
    }
    Counts cnt{0, 0};
    const Node nd = shade_hit<TREE, false, DIRECT, CHILDREN>(
        S, P, o, d, h, AREA ? pixel_key(keys, i) : 0, AREA ? keys.sample : 0,
        AREA ? static_cast<int>(keys.depth) : 0, cnt);
    sc_store_node<CHILDREN>(out, i, nd);
}

template <bool TREE, bool DIRECT, bool CHILDREN>
__global__ __launch_bounds__(256) void scatter_rays_kernel(TraceParams P,
                                                           const double* __restrict__ rays, size_t n,
                                                           ScOut out) {
    scatter_body<false, TREE, DIRECT, CHILDREN>(P, rays, AreaKeyArgs{}, n, out);
}

template <bool TREE, bool CHILDREN>
__global__ __launch_bounds__(256) void keyed_scatter_kernel(TraceParams P,
                                                            const double* __restrict__ rays,
                                                            AreaKeyArgs keys, size_t n, ScOut out) {
    scatter_body<true, TREE, true, CHILDREN>(P, rays, keys, n, out);
}

// keys: null launches the un-keyed kernel; they are only given with direct.
template <bool TREE>
static void launch_scatter(const TraceParams& p, bool direct, bool children, const double* rays,
                           const AreaKeyArgs* keys, size_t n, const ScOut& out,
                           hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    if (keys && children)
        hipLaunchKernelGGL((keyed_scatter_kernel<TREE, true>), grid, block, 0, stream, p, rays,
                           *keys, n, out);
    else if (keys)
        hipLaunchKernelGGL((keyed_scatter_kernel<TREE, false>), grid, block, 0, stream, p, rays,
                           *keys, n, out);
    else if (direct && children)
        hipLaunchKernelGGL((scatter_rays_kernel<TREE, true, true>), grid, block, 0, stream, p, rays,
                           n, out);
    else if (direct)
        hipLaunchKernelGGL((scatter_rays_kernel<TREE, true, false>), grid, block, 0, stream, p, rays,
                           n, out);
    else
        hipLaunchKernelGGL((scatter_rays_kernel<TREE, false, true>), grid, block, 0, stream, p, rays,
                           n, out);
}

// direct: out.value is wanted; children: any of the child rays, the weights or the flags is.
// At least one of them holds (the entries reject outputs == 0).  keys: served only for a scene
// with an area light attached and with the value wanted (the child outputs do not depend on
// them); otherwise, and for null, the un-keyed kernel.
hipError_t launch_scatter_rays(const TraceParams& p, bool opaque, const double* rays,
                               const AreaKeyArgs* keys, size_t n, const ScOut& out,
                               hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const bool direct = out.value != nullptr;
    const bool children = out.refract_rays || out.reflect_rays || out.weights || out.flags;
    if (!direct && !children) return hipErrorInvalidValue;
    if (p.al_samples <= 0 || !direct) keys = nullptr;
    if (opaque)
        launch_scatter<false>(p, direct, children, rays, keys, n, out, stream);
    else
        launch_scatter<true>(p, direct, children, rays, keys, n, out, stream);
    return hipGetLastError();
}

}  // namespace rtamd
