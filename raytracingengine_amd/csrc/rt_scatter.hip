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
// The build-defined area light is not read (keyed_scatter_kernel, rt_area_queries.hip, reads it
// under keys the caller supplies): the kernel's SceneView says the scene has none
// (S.al = 0, a constant there), so direct()'s sample loop, and its second inlined light_term, is
// not compiled into these kernels at all.
#include "rt_query_out.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// One thread per ray {o, d}.  P.max_rec <= 0: the ray is at the recursion limit (Scene.h:132-134),
// nothing is intersected.
template <bool TREE, bool DIRECT, bool CHILDREN>
__global__ __launch_bounds__(256) void scatter_rays_kernel(TraceParams P,
                                                           const double* __restrict__ rays, size_t n,
                                                           ScOut out) {
    SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    S.al = 0;  // no area light: this entry takes no pixel and sample keys for its draws
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + 6 * i;
    const d3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    Hit h;
    if (P.max_rec <= 0 || !closest(S, o, d, h)) {
        Node nd;
        nd.hit = false;
        nd.refl = false;
        nd.refr = false;
        nd.value = sky(d);
        sc_store_node<CHILDREN>(out, i, nd);
        return;
    }
    Counts cnt{0, 0};
    const Node nd = shade_hit<TREE, false, DIRECT, CHILDREN>(S, P, o, d, h, 0, 0, 0, cnt);
    sc_store_node<CHILDREN>(out, i, nd);
}

template <bool TREE>
static void launch_scatter(const TraceParams& p, bool direct, bool children, const double* rays,
                           size_t n, const ScOut& out, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    if (direct && children)
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
// At least one of them holds (the entries reject outputs == 0).
hipError_t launch_scatter_rays(const TraceParams& p, bool opaque, const double* rays, size_t n,
                               const ScOut& out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const bool direct = out.value != nullptr;
    const bool children = out.refract_rays || out.reflect_rays || out.weights || out.flags;
    if (!direct && !children) return hipErrorInvalidValue;
    if (opaque)
        launch_scatter<false>(p, direct, children, rays, n, out, stream);
    else
        launch_scatter<true>(p, direct, children, rays, n, out, stream);
    return hipGetLastError();
}

}  // namespace rtamd
