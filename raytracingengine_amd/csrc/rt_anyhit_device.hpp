// rt_anyhit_device.hpp — device building blocks of the any-hit (occlusion) query:
// Scene::IntersectAnyBefore (Scene.h:259-276) for one ray per lane.
//
// The answer is an OR over the primitives of `Intersect(ray)` returning a t with
// t > 0.0 && t < maxDist, so visiting order is free and a lane is finished at its first such t.
// Each t is the value closest_t / tri_hit_v (rt_trace_common.hpp) compute: IEEE binary64 in the
// reference's operation order, no FMA contraction (Sphere::Intersect Shape.h:72-98,
// Plane::Intersect Shape.h:149-159, Triangle::Intersect Shape.h:202-220).
#pragma once

#include "rt_trace_common.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// IntersectAnyBefore's `within` (Scene.h:264).
__device__ __forceinline__ bool any_within(double t, double max_dist) {
    return t > 0.0 && t < max_dist;
}

// Sphere::Intersect with closest_t's hoisted a, 2a and 4a: the same roots, the same selection
// (near root, the far one when the near one is below 1e-6, none when both are).
__device__ __forceinline__ bool any_sphere_t(const double* s, d3 o, d3 d, double two_a,
                                             double four_a, double& t) {
    const d3 oc = o - mk(s[0], s[1], s[2]);
    const double b = 2.0 * dot(oc, d);
    const double c = dot(oc, oc) - s[3];
    const double disc = b * b - four_a * c;
    if (disc < 0.0) return false;
    const double sq = sqrt(disc);
    double t0 = (-b - sq) / two_a;
    double t1 = (-b + sq) / two_a;
    if (t0 > t1) {
        const double tmp = t0;
        t0 = t1;
        t1 = tmp;
    }
    t = t0;
    if (t < 1e-6) {
        t = t1;
        if (t < 1e-6) return false;
    }
    return true;
}

// Plane::Intersect: t >= 0 is a hit there, and t == 0 then fails `within`.
__device__ __forceinline__ bool any_plane_t(const double* p, d3 o, d3 d, double& t) {
    const d3 n = mk(p[3], p[4], p[5]);
    const double denom = dot(n, d);
    if (!(fabs(denom) > 1e-6)) return false;
    const d3 p0l0 = mk(p[0], p[1], p[2]) - o;
    t = dot(p0l0, n) / denom;
    return t >= 0.0;
}

// The triangles' part over the BVH, for one lane: true at the first triangle with t < max_dist
// (every triangle t is > 1e-6, so t > 0 holds).  A node is visited only when bvh_box accepts it
// and its entry bound does not exceed max_dist by the 1e-9 margin the closest-hit traversal
// (bvh_triangles) keeps against its best t, so a triangle whose t is below max_dist by a
// rounding of the box arithmetic is never skipped.
__device__ __forceinline__ bool any_bvh_triangles(const double* tri, const double* bvh,
                                                  const int32_t* order, d3 o, d3 d,
                                                  double max_dist) {
    const d3 inv = mk(d.x != 0.0 ? 1.0 / d.x : 0.0, d.y != 0.0 ? 1.0 / d.y : 0.0,
                      d.z != 0.0 ? 1.0 / d.z : 0.0);
    const double lim = max_dist * (1.0 + 1e-9);
    int stk[kBvhStack];
    int sp = 0;
    double tn;
    if (bvh_box(bvh, o, d, inv, tn) && !(tn > lim)) stk[sp++] = 0;
    while (sp > 0) {
        const double* nd = bvh + kBvhNodeStride * stk[--sp];
        const int first = __double2loint(nd[6]), count = __double2hiint(nd[6]);
        if (count > 0) {
            for (int j = first; j < first + count; ++j) {
                double t;
                if (tri_hit(tri, order[j], o, d, t) && t < max_dist) return true;
            }
            continue;
        }
        double t0, t1;
        const bool h0 = bvh_box(bvh + kBvhNodeStride * first, o, d, inv, t0) && !(t0 > lim);
        const bool h1 = bvh_box(bvh + kBvhNodeStride * (first + 1), o, d, inv, t1) && !(t1 > lim);
        if (h0 && h1) {  // nearer child on top: the likelier early exit
            const bool near0 = !(t1 < t0);
            stk[sp++] = near0 ? first + 1 : first;
            stk[sp++] = near0 ? first : first + 1;
        } else if (h0) {
            stk[sp++] = first;
        } else if (h1) {
            stk[sp++] = first + 1;
        }
    }
    return false;
}

}  // namespace rtamd
