// rt_area_queries.hip — the keyed twins of the per-level batch queries for gfx950 (MI355X): the
// scatter, direct-light and light-transmittance queries with the build-defined area light served.
// The area light's sample points are random draws keyed by (seed, pixel, stream, 2s | 2s + 1) with
// stream = 0x10000 + (sample << 6) + depth (direct(), rt_trace_common.hpp); here the caller hands
// the keys in: one 64-bit pixel key per element (or none: element i draws with pixel = i, the
// rule of rt_trace_rays), the sample and the depth for the whole batch.
//
// One thread per element, 256-thread workgroups, the scene read through stage_scene<false> as
// the un-keyed kernels do.  The pixel key is one 8-byte load per lane; whether there are keys at
// all is a kernel argument, so that test is a scalar branch.  sample, depth and the seed travel
// in the kernel arguments and stay scalar.
//
// keyed_scatter_kernel is closest + shade_hit with the keys passed through: direct()'s own sample
// loop runs, nothing is restated.  The direct-light kernels return the two accumulators apart,
// which direct() folds in its last line, so they run the loop of area_terms below: direct()'s
// sample loop restated over the shared light_term.  The two must stay the same text, operation
// for operation; tests/test_gpu_area_queries.py holds them to each other bit for bit.
// keyed_shadow_points_kernel walks the same sample points with rt_light_transmittance's seven
// steps.
//
// The launches are only taken for a scene with an area light attached and, for the scatter,
// with the value requested: everything else is the un-keyed kernels' (rt_capi_queries.cpp).
#include "rt_query_out.hpp"

#pragma clang fp contract(off)

namespace rtamd {

namespace {

__device__ __forceinline__ uint64_t pixel_key(const AreaKeyArgs& k, size_t i) {
    return k.pixel ? static_cast<uint64_t>(k.pixel[i]) : static_cast<uint64_t>(i);
}

__device__ __forceinline__ uint32_t area_stream(const AreaKeyArgs& k) {
    return 0x10000u + (k.sample << 6) + static_cast<uint32_t>(k.depth);
}

// The point of area sample s: the draws and the stratum of direct()'s sample loop
// (rt_trace_common.hpp), the same operations in the same order.
__device__ __forceinline__ d3 area_point(const TraceParams& P, uint64_t pix, uint32_t stream,
                                         int s) {
    const double k = static_cast<double>(P.al_k);
    const d3 corner = mk(P.al_corner[0], P.al_corner[1], P.al_corner[2]);
    const d3 eu = mk(P.al_u[0], P.al_u[1], P.al_u[2]);
    const d3 ev = mk(P.al_v[0], P.al_v[1], P.al_v[2]);
    const double r1 = u01(P.seed, pix, stream, 2u * static_cast<uint32_t>(s));
    const double r2 = u01(P.seed, pix, stream, 2u * static_cast<uint32_t>(s) + 1u);
    const double fu = (static_cast<double>(s % P.al_k) + r1) / k;
    const double fv = (static_cast<double>(s / P.al_k) + r2) / k;
    return (corner + eu * fu) + ev * fv;
}

// directLightning's light loop with the area samples appended: direct() (rt_trace_common.hpp) up
// to, not including, its last line — the two accumulators stay apart.  The sample loop restates
// the one under `if (S.al > 0)` there; a change there is a change here.
template <bool OPAQUE>
__device__ __forceinline__ void area_terms(const SceneView& S, const TraceParams& P, d3 p, d3 n_in,
                                           d3 view, const double* m, uint64_t pix,
                                           const AreaKeyArgs& keys, d3& diff, d3& spec) {
    const double bias = P.bias;
    const d3 n = unit(n_in);  // Scene.h:81
    Counts cnt{0, 0};
    diff = mk(0.0, 0.0, 0.0);
    spec = mk(0.0, 0.0, 0.0);
    for (int l = 0; l < S.nl; ++l) {
        const double* lt = S.lt + kLtStride * l;
        light_term<false, OPAQUE>(S, p, n, view, m, mk(lt[0], lt[1], lt[2]),
                                  mk(lt[3], lt[4], lt[5]), bias, diff, spec, cnt);
    }
    const uint32_t stream = area_stream(keys);
    const d3 E = mk(P.al_E[0], P.al_E[1], P.al_E[2]);
    for (int s = 0; s < S.al; ++s)
        light_term<false, OPAQUE>(S, p, n, view, m, area_point(P, pix, stream, s), E, bias, diff,
                                  spec, cnt);
}

}  // namespace

// One thread per ray {o, d}: rt_scatter.hip's kernel with the area light left on.  DIRECT is
// always on here (a launch without the value does not depend on the keys).
template <bool TREE, bool CHILDREN>
__global__ __launch_bounds__(256) void keyed_scatter_kernel(TraceParams P,
                                                            const double* __restrict__ rays,
                                                            AreaKeyArgs keys, size_t n, ScOut out) {
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
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
    const Node nd =
        shade_hit<TREE, false, true, CHILDREN>(S, P, o, d, h, pixel_key(keys, i), keys.sample,
                                               static_cast<int>(keys.depth), cnt);
    sc_store_node<CHILDREN>(out, i, nd);
}

// One thread per point {p, normal, view}: rt_direct.hip's points kernel, its loads and its
// SHARED material, with area_terms for the light loop.
template <bool OPAQUE, bool SHARED>
__global__ __launch_bounds__(256) void keyed_direct_points_kernel(
    TraceParams P, const double* __restrict__ points, const double* __restrict__ materials,
    DlMaterial shared, AreaKeyArgs keys, size_t n, DlOut out) {
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
    area_terms<OPAQUE>(S, P, mk(q0.x, q0.y, q1.x), mk(q1.y, q2.x, q2.y), mk(q3.x, q3.y, q8), m,
                       pixel_key(keys, i), keys, diff, spec);
    store_outputs(out, i, mk(m[0], m[1], m[2]), m[4], diff, spec);
}

// One thread per ray {o, d}: rt_direct.hip's rays kernel (hit point, flipped normal and view as
// shade_hit forms them) with area_terms for the light loop.  A miss writes zeros.
template <bool OPAQUE>
__global__ __launch_bounds__(256) void keyed_direct_rays_kernel(TraceParams P,
                                                                const double* __restrict__ rays,
                                                                AreaKeyArgs keys, size_t n,
                                                                DlOut out) {
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
    area_terms<OPAQUE>(S, P, hp, nrm, -inc, m, pixel_key(keys, i), keys, diff, spec);
    store_outputs(out, i, mk(m[0], m[1], m[2]), m[4], diff, spec);
}

// The seven steps of rt_light_transmittance (rt_capi.h) from point p to the light point lpos.
template <bool OPAQUE>
__device__ __forceinline__ double shadow_T(const SceneView& S, d3 p, d3 normal, d3 lpos,
                                           double bias) {
    double dist, inv_d2;
    d3 L;
    light_dir(lpos - p, dist, L, inv_d2);
    if (!(dist <= 0.0) && !(smax(0.0, dot(normal, L)) <= 0.0) && !(dist <= bias))
        return transmit_ray<OPAQUE>(S, p + normal * bias, L, dist - bias, bias);
    return 0.0;
}

// One thread per point {p, normal}: 6 doubles and the key in, nl + al doubles out at [i][c] —
// the point lights in scene order, then the area samples in stratum order.
template <bool OPAQUE>
__global__ __launch_bounds__(256) void keyed_shadow_points_kernel(TraceParams P,
                                                                  const double* __restrict__ points,
                                                                  AreaKeyArgs keys, size_t n,
                                                                  double* __restrict__ out) {
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
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
    const uint64_t pix = pixel_key(keys, i);
    const uint32_t stream = area_stream(keys);
    for (int s = 0; s < S.al; ++s)
        w[S.nl + s] = shadow_T<OPAQUE>(S, p, normal, area_point(P, pix, stream, s), bias);
}

namespace {

dim3 grid_of(size_t n) { return dim3(static_cast<unsigned>((n + 255) / 256)); }

}  // namespace

hipError_t launch_keyed_scatter(const TraceParams& p, bool opaque, const double* rays,
                                const AreaKeyArgs& keys, size_t n, const ScOut& out,
                                hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!out.value || p.al_samples <= 0) return hipErrorInvalidValue;
    const bool children = out.refract_rays || out.reflect_rays || out.weights || out.flags;
    const dim3 grid = grid_of(n), block(256);
    const AreaKeyArgs& k = keys;
    if (opaque && children)
        hipLaunchKernelGGL((keyed_scatter_kernel<false, true>), grid, block, 0, stream, p, rays, k,
                           n, out);
    else if (opaque)
        hipLaunchKernelGGL((keyed_scatter_kernel<false, false>), grid, block, 0, stream, p, rays, k,
                           n, out);
    else if (children)
        hipLaunchKernelGGL((keyed_scatter_kernel<true, true>), grid, block, 0, stream, p, rays, k,
                           n, out);
    else
        hipLaunchKernelGGL((keyed_scatter_kernel<true, false>), grid, block, 0, stream, p, rays, k,
                           n, out);
    return hipGetLastError();
}

hipError_t launch_keyed_direct_points(const TraceParams& p, bool opaque, const double* points,
                                      const double* materials, const DlMaterial& shared,
                                      const AreaKeyArgs& keys, size_t n, const DlOut& out,
                                      hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (p.al_samples <= 0) return hipErrorInvalidValue;
    const dim3 grid = grid_of(n), block(256);
    const AreaKeyArgs& k = keys;
    if (materials) {
        if (opaque)
            hipLaunchKernelGGL((keyed_direct_points_kernel<true, false>), grid, block, 0, stream, p,
                               points, materials, shared, k, n, out);
        else
            hipLaunchKernelGGL((keyed_direct_points_kernel<false, false>), grid, block, 0, stream,
                               p, points, materials, shared, k, n, out);
    } else {
        if (opaque)
            hipLaunchKernelGGL((keyed_direct_points_kernel<true, true>), grid, block, 0, stream, p,
                               points, materials, shared, k, n, out);
        else
            hipLaunchKernelGGL((keyed_direct_points_kernel<false, true>), grid, block, 0, stream, p,
                               points, materials, shared, k, n, out);
    }
    return hipGetLastError();
}

hipError_t launch_keyed_direct_rays(const TraceParams& p, bool opaque, const double* rays,
                                    const AreaKeyArgs& keys, size_t n, const DlOut& out,
                                    hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (p.al_samples <= 0) return hipErrorInvalidValue;
    const dim3 grid = grid_of(n), block(256);
    const AreaKeyArgs& k = keys;
    if (opaque)
        hipLaunchKernelGGL(keyed_direct_rays_kernel<true>, grid, block, 0, stream, p, rays, k, n,
                           out);
    else
        hipLaunchKernelGGL(keyed_direct_rays_kernel<false>, grid, block, 0, stream, p, rays, k, n,
                           out);
    return hipGetLastError();
}

hipError_t launch_keyed_shadow_points(const TraceParams& p, bool opaque, const double* points,
                                      const AreaKeyArgs& keys, size_t n, double* out,
                                      hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (p.al_samples <= 0) return hipErrorInvalidValue;
    const dim3 grid = grid_of(n), block(256);
    const AreaKeyArgs& k = keys;
    if (opaque)
        hipLaunchKernelGGL(keyed_shadow_points_kernel<true>, grid, block, 0, stream, p, points, k,
                           n, out);
    else
        hipLaunchKernelGGL(keyed_shadow_points_kernel<false>, grid, block, 0, stream, p, points, k,
                           n, out);
    return hipGetLastError();
}

}  // namespace rtamd
