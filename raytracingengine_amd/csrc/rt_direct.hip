// rt_direct.hip — the batch direct-lighting queries for gfx950 (MI355X):
// Scene::directLightning (Scene.h:79-129) for n caller-supplied surface points, and for the first
// hit of n rays (the localLight of TraceRay, Scene.h:136-147, 168, at recursion depth 0).
//
// Both kernels run light_term (rt_trace_common.hpp), the light loop's body of the render kernels,
// once per point light in scene order (trip count nl for the whole wave, so the light records
// arrive through the scalar cache): light_dir, the three `continue`s, the shadow ray's march
// (transmittance), the T <= bias drop, the diffuse term and the gated Blinn-Phong term, the two
// accumulators kept apart until the end.  The rays kernel finds its hit with closest and forms hit
// point, normal and view as shade_hit does.  Nothing of that is restated here, so the bits are the
// renderer's.  OPAQUE (no material of the scene is transparent): light_term asks
// occlusion_opaque before the march, as the render kernels of such scenes do.
// Only the point lights are read; the build-defined area light is read by the keyed twins of
// these kernels (rt_area_queries.hip).
#include "rt_query_out.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// directLightning's loop over the point lights for one point; m: {r g b shininess specular
// transparency ...}, read by light_term at its uses.
template <bool OPAQUE>
__device__ __forceinline__ void light_loop(const SceneView& S, d3 p, d3 n_in, d3 view,
                                           const double* m, double bias, d3& diff, d3& spec) {
    const d3 n = unit(n_in);  // Scene.h:81
    Counts cnt{0, 0};
    diff = mk(0.0, 0.0, 0.0);
    spec = mk(0.0, 0.0, 0.0);
    for (int l = 0; l < S.nl; ++l) {
        const double* lt = S.lt + kLtStride * l;
        light_term<false, OPAQUE>(S, p, n, view, m, mk(lt[0], lt[1], lt[2]),
                                  mk(lt[3], lt[4], lt[5]), bias, diff, spec, cnt);
    }
}

// One thread per point {p, normal, view}: 9 doubles in, and with SHARED == false the point's own
// material (7 doubles, rt_material's layout) — eight 16-byte loads, the two records read up front.
// SHARED: one material for all points, in the kernel arguments, so it stays in scalar registers.
template <bool OPAQUE, bool SHARED>
__global__ __launch_bounds__(256) void direct_light_points_kernel(
    TraceParams P, const double* __restrict__ points, const double* __restrict__ materials,
    DlMaterial shared, size_t n, DlOut out) {
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
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
    d3 diff, spec;
    light_loop<OPAQUE>(S, mk(q0.x, q0.y, q1.x), mk(q1.y, q2.x, q2.y), mk(q3.x, q3.y, q8), m, P.bias,
                       diff, spec);
    store_outputs(out, i, mk(m[0], m[1], m[2]), m[4], diff, spec);
}

// One thread per ray {o, d}: IntersectClosest, then hit point, flipped normal and view as
// shade_hit forms them (hp = o + d·t, inc = unit(d), n = ±gn by dot(gn, inc) < 0, view = −inc),
// the hit primitive's material read from the scene's table at each use.  A miss writes zeros.
template <bool OPAQUE>
__global__ __launch_bounds__(256) void direct_light_rays_kernel(TraceParams P,
                                                                const double* __restrict__ rays,
                                                                size_t n, DlOut out) {
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
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
    d3 diff, spec;
    light_loop<OPAQUE>(S, hp, nrm, -inc, m, P.bias, diff, spec);
    store_outputs(out, i, mk(m[0], m[1], m[2]), m[4], diff, spec);
}

hipError_t launch_direct_light_points(const TraceParams& p, bool opaque, const double* points,
                                      const double* materials, const DlMaterial& shared, size_t n,
                                      const DlOut& out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    if (materials) {
        if (opaque)
            hipLaunchKernelGGL((direct_light_points_kernel<true, false>), grid, block, 0, stream, p,
                               points, materials, shared, n, out);
        else
            hipLaunchKernelGGL((direct_light_points_kernel<false, false>), grid, block, 0, stream, p,
                               points, materials, shared, n, out);
    } else {
        if (opaque)
            hipLaunchKernelGGL((direct_light_points_kernel<true, true>), grid, block, 0, stream, p,
                               points, materials, shared, n, out);
        else
            hipLaunchKernelGGL((direct_light_points_kernel<false, true>), grid, block, 0, stream, p,
                               points, materials, shared, n, out);
    }
    return hipGetLastError();
}

hipError_t launch_direct_light_rays(const TraceParams& p, bool opaque, const double* rays, size_t n,
                                    const DlOut& out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    if (opaque)
        hipLaunchKernelGGL(direct_light_rays_kernel<true>, grid, block, 0, stream, p, rays, n, out);
    else
        hipLaunchKernelGGL(direct_light_rays_kernel<false>, grid, block, 0, stream, p, rays, n, out);
    return hipGetLastError();
}

}  // namespace rtamd
