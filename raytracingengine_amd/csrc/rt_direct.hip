// rt_direct.hip — the batch direct-lighting queries for gfx950 (MI355X):
// Scene::directLightning (Scene.h:79-129) for n caller-supplied surface points, and for the first
// hit of n rays (the localLight of TraceRay, Scene.h:136-147, 168, at recursion depth 0).
//
// Both bodies run direct_terms (rt_trace_common.hpp), the render kernels' light loop with the two
// accumulators still apart: light_term once per point light in scene order (trip count nl for the
// whole wave, so the light records arrive through the scalar cache) — light_dir, the three
// `continue`s, the shadow ray's march (transmittance), the T <= bias drop, the diffuse term and
// the gated Blinn-Phong term.  The rays body finds its hit with closest and forms hit point,
// normal and view as shade_hit does.  Nothing of that is restated here, so the bits are the
// renderer's.  OPAQUE (no material of the scene is transparent): light_term asks
// occlusion_opaque before the march, as the render kernels of such scenes do.
// AREA (rt_query_out.hpp): the keyed_ kernels append the build-defined area light's samples, the
// un-keyed ones read the point lights only.
#include "rt_query_out.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// One thread per point {p, normal, view}: 9 doubles in, and with SHARED == false the point's own
// material (7 doubles, rt_material's layout) — eight 16-byte loads, the two records read up front.
// SHARED: one material for all points, in the kernel arguments, so it stays in scalar registers.
template <bool AREA, bool OPAQUE, bool SHARED>
__device__ __forceinline__ void direct_points_body(const TraceParams& P, const double* points,
                                                   const double* materials,
                                                   const DlMaterial& shared,
                                                   const AreaKeyArgs& keys, size_t n,
                                                   const DlOut& out) {
    SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    if constexpr (!AREA) S.al = 0;
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* q = points + 9 * i;
    const d2u q0 = load2(q), q1 = load2(q + 2), q2 = load2(q + 4), q3 = load2(q + 6);
    const double q8 = q[8];
    double m[8];
    if constexpr (SHARED) {
        for (int k = 0; k < 7; ++k) m[k] = shared.v[k];
    } else {
        const double* r = materials + 7 * i;
        const d2u m0 = load2(r), m1 = load2(r + 2), m2 = load2(r + 4);
        m[0] = m0.x;
        m[1] = m0.y;
        m[2] = m1.x;
        m[3] = m1.y;
        m[4] = m2.x;
        m[5] = m2.y;
        m[6] = r[6];
    }
    Counts cnt{0, 0};
    d3 diff, spec;
    direct_terms<false, OPAQUE>(S, P, mk(q0.x, q0.y, q1.x), mk(q3.x, q3.y, q8), mk(q1.y, q2.x, q2.y),
                                m, AREA ? pixel_key(keys, i) : 0, AREA ? keys.sample : 0,
                                AREA ? static_cast<int>(keys.depth) : 0, cnt, diff, spec);
    store_outputs(out, i, mk(m[0], m[1], m[2]), m[4], diff, spec);
}

// One thread per ray {o, d}: IntersectClosest, then hit point, flipped normal and view as
// shade_hit forms them (hp = o + d·t, inc = unit(d), n = ±gn by dot(gn, inc) < 0, view = −inc),
// the hit primitive's material read from the scene's table at each use.  A miss writes zeros.
template <bool AREA, bool OPAQUE>
__device__ __forceinline__ void direct_rays_body(const TraceParams& P, const double* rays,
                                                 const AreaKeyArgs& keys, size_t n,
                                                 const DlOut& out) {
    SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    if constexpr (!AREA) S.al = 0;
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + 6 * i;
    const d3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    Hit h;
    if (!closest(S, o, d, h)) {
        const d3 z = mk(0.0, 0.0, 0.0);
        store3(out.radiance, i, z);
        store3(out.diffuse, i, z);
        store3(out.specular, i, z);
        return;
    }
    const d3 hp = o + d * h.t;  // Rayon::pointAtDistance
    const d3 gn = normal_of(S, h, hp);
    const double* m = material_of(S, h);
    const d3 inc = unit(d);
    const bool front = dot(gn, inc) < 0.0;
    const d3 nrm = front ? gn : -gn;
    Counts cnt{0, 0};
    d3 diff, spec;
    direct_terms<false, OPAQUE>(S, P, hp, -inc, nrm, m, AREA ? pixel_key(keys, i) : 0,
                                AREA ? keys.sample : 0, AREA ? static_cast<int>(keys.depth) : 0,
                                cnt, diff, spec);
    store_outputs(out, i, mk(m[0], m[1], m[2]), m[4], diff, spec);
}

template <bool OPAQUE, bool SHARED>
__global__ __launch_bounds__(256) void direct_light_points_kernel(
    TraceParams P, const double* __restrict__ points, const double* __restrict__ materials,
    DlMaterial shared, size_t n, DlOut out) {
    direct_points_body<false, OPAQUE, SHARED>(P, points, materials, shared, AreaKeyArgs{}, n, out);
}

template <bool OPAQUE, bool SHARED>
__global__ __launch_bounds__(256) void keyed_direct_points_kernel(
    TraceParams P, const double* __restrict__ points, const double* __restrict__ materials,
    DlMaterial shared, AreaKeyArgs keys, size_t n, DlOut out) {
    direct_points_body<true, OPAQUE, SHARED>(P, points, materials, shared, keys, n, out);
}

template <bool OPAQUE>
__global__ __launch_bounds__(256) void direct_light_rays_kernel(TraceParams P,
                                                                const double* __restrict__ rays,
                                                                size_t n, DlOut out) {
    direct_rays_body<false, OPAQUE>(P, rays, AreaKeyArgs{}, n, out);
}

template <bool OPAQUE>
__global__ __launch_bounds__(256) void keyed_direct_rays_kernel(TraceParams P,
                                                                const double* __restrict__ rays,
                                                                AreaKeyArgs keys, size_t n,
                                                                DlOut out) {
    direct_rays_body<true, OPAQUE>(P, rays, keys, n, out);
}

namespace {

// keys: null launches the un-keyed kernel.
template <bool OPAQUE, bool SHARED>
void launch_points(const TraceParams& p, const double* points, const double* materials,
                   const DlMaterial& shared, const AreaKeyArgs* keys, size_t n, const DlOut& out,
                   hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    if (keys)
        hipLaunchKernelGGL((keyed_direct_points_kernel<OPAQUE, SHARED>), grid, block, 0, stream, p,
                           points, materials, shared, *keys, n, out);
    else
        hipLaunchKernelGGL((direct_light_points_kernel<OPAQUE, SHARED>), grid, block, 0, stream, p,
                           points, materials, shared, n, out);
}

template <bool OPAQUE>
void launch_rays(const TraceParams& p, const double* rays, const AreaKeyArgs* keys, size_t n,
                 const DlOut& out, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    if (keys)
        hipLaunchKernelGGL(keyed_direct_rays_kernel<OPAQUE>, grid, block, 0, stream, p, rays, *keys,
                           n, out);
    else
        hipLaunchKernelGGL(direct_light_rays_kernel<OPAQUE>, grid, block, 0, stream, p, rays, n,
                           out);
}

}  // namespace

// keys (both launches): served only for a scene with an area light attached; null, or no area
// light: the un-keyed kernel.
hipError_t launch_direct_light_points(const TraceParams& p, bool opaque, const double* points,
                                      const double* materials, const DlMaterial& shared,
                                      const AreaKeyArgs* keys, size_t n, const DlOut& out,
                                      hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (p.al_samples <= 0) keys = nullptr;
    if (materials) {
        if (opaque)
            launch_points<true, false>(p, points, materials, shared, keys, n, out, stream);
        else
            launch_points<false, false>(p, points, materials, shared, keys, n, out, stream);
    } else {
        if (opaque)
            launch_points<true, true>(p, points, materials, shared, keys, n, out, stream);
        else
            launch_points<false, true>(p, points, materials, shared, keys, n, out, stream);
    }
    return hipGetLastError();
}

hipError_t launch_direct_light_rays(const TraceParams& p, bool opaque, const double* rays,
                                    const AreaKeyArgs* keys, size_t n, const DlOut& out,
                                    hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (p.al_samples <= 0) keys = nullptr;
    if (opaque)
        launch_rays<true>(p, rays, keys, n, out, stream);
    else
        launch_rays<false>(p, rays, keys, n, out, stream);
    return hipGetLastError();
}

}  // namespace rtamd
