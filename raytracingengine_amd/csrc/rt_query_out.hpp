// rt_query_out.hpp — what the per-level batch queries (rt_transmit.hip, rt_direct.hip,
// rt_scatter.hip), un-keyed and keyed, share besides the shading of rt_trace_common.hpp: the
// 16-byte record loads, the pixel key of an element, computeTransmittance with its fast path, the
// shadow ray of one light point, and the stores of the output records (DlOut, ScOut).  Plain
// vector stores, one thread per element.
//
// Each query's kernel body is written once, with a bool AREA: false is the un-keyed kernel, whose
// SceneView says the scene has no area light (S.al = 0, a constant there, so no sample loop is
// compiled in) and which ignores the keys; true serves the area light's samples under the
// caller's keys — one 64-bit pixel key per element (or none: element i draws with pixel = i, the
// rule of rt_trace_rays), the sample and the depth for the whole batch.  Whether there are pixel
// keys is a kernel argument, so that test is a scalar branch; sample, depth and the seed travel
// in the kernel arguments and stay scalar.
#pragma once

#include "rt_trace_common.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// Two doubles at 8-byte alignment: the records of a point (72 B) and of a material (56 B) keep
// every second thread off a 16-byte boundary, and a 16-byte global load needs none.
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));

__device__ __forceinline__ d2u load2(const double* p) { return *reinterpret_cast<const d2u*>(p); }

__device__ __forceinline__ uint64_t pixel_key(const AreaKeyArgs& k, size_t i) {
    return k.pixel ? static_cast<uint64_t>(k.pixel[i]) : static_cast<uint64_t>(i);
}

// computeTransmittance(ray {o, d}, max_dist, bias).  A max_dist that is NaN or <= 0 never enters
// the march's loop (traveled = 0 < max_dist is false): 1.0, asked before the classification,
// whose margins are formed from max_dist.
template <bool OPAQUE>
__device__ __forceinline__ double transmit_ray(const SceneView& S, d3 o, d3 d, double max_dist,
                                               double bias) {
    if (!(max_dist > 0.0)) return 1.0;
    if constexpr (OPAQUE) {
        const int occ = occlusion_opaque(S, o, d, max_dist, bias);
        if (occ >= 0) return static_cast<double>(occ);
    }
    return transmittance(S, o, d, max_dist, bias);
}

// The seven steps of rt_light_transmittance (rt_capi.h) from point p to the light point lpos; the
// three skips are directLightning's `continue`s (Scene.h:89, 92, 95) and answer 0.0.
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

__device__ __forceinline__ void store3(double* base, size_t i, d3 v) {
    if (!base) return;
    double* w = base + 3 * i;
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
}

// color * diffuseAccumulation + specularAccumlation * material.specular (Scene.h:126-128), the
// last line of `direct`.
__device__ __forceinline__ void store_outputs(const DlOut& out, size_t i, d3 color, double specular,
                                              d3 diff, d3 spec) {
    store3(out.radiance, i, hmul(color, diff) + spec * specular);
    store3(out.diffuse, i, diff);
    store3(out.specular, i, spec);
}

// A child ray {o, d}, or six +0.0 where the level has none: 48 B per ray, 8-byte aligned.
__device__ __forceinline__ void sc_store_ray(double* base, size_t i, bool present, d3 o, d3 d) {
    if (!base) return;
    double* w = base + 6 * i;
    w[0] = present ? o.x : 0.0;
    w[1] = present ? o.y : 0.0;
    w[2] = present ? o.z : 0.0;
    w[3] = present ? d.x : 0.0;
    w[4] = present ? d.y : 0.0;
    w[5] = present ? d.z : 0.0;
}

// Every requested output of ray i from its Node; an absent child is zeros, as is its weight.
template <bool CHILDREN>
__device__ __forceinline__ void sc_store_node(const ScOut& out, size_t i, const Node& nd) {
    store3(out.value, i, nd.value);
    if constexpr (CHILDREN) {
        sc_store_ray(out.refract_rays, i, nd.refr, nd.fo, nd.fd);
        sc_store_ray(out.reflect_rays, i, nd.refl, nd.ro, nd.rd);
        if (out.weights) {
            out.weights[2 * i + 0] = nd.refr ? nd.fw : 0.0;
            out.weights[2 * i + 1] = nd.refl ? nd.rw : 0.0;
        }
        if (out.flags)
            out.flags[i] = static_cast<uint8_t>((nd.hit ? 1 : 0) | (nd.refr ? 2 : 0) | (nd.refl ? 4 : 0));
    }
}

// The Node of a ray that hit nothing, or stands at the recursion limit: the sky, no children.
__device__ __forceinline__ Node sky_node(d3 d) {
    Node nd;
    nd.hit = false;
    nd.refl = false;
    nd.refr = false;
    nd.value = sky(d);
    return nd;
}

}  // namespace rtamd
