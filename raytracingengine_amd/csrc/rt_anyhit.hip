// rt_anyhit.hip — the batch occlusion query for gfx950 (MI355X): Scene::IntersectAnyBefore
// (Scene.h:259-276) for n arbitrary rays, one thread per ray, one byte out per ray.
//
// 1 iff some primitive's Intersect(ray) returns a t with t > 0.0 && t < maxDist, each t in the
// reference's binary64 operation order (rt_anyhit_device.hpp).  Spheres, then planes, in loops
// whose trip counts are the same for the whole wave, so the records arrive through the scalar
// cache; each lane keeps a `done` flag and the wave leaves a loop once no lane is undecided.
// Triangles: a per-lane any-hit BVH traversal for the lanes still undecided, or the plain loop
// when the scene has no BVH (fewer than kBvhMinTris triangles, or RT_FLAG_NO_BVH).
// Lights, materials and the area light are not read.  Traffic per ray: 7 doubles in (the ray and
// its maxDist, 56 B), one byte out.
#include "rt_anyhit_device.hpp"

#pragma clang fp contract(off)

namespace rtamd {

__global__ __launch_bounds__(256) void occluded_rays_kernel(TraceParams P,
                                                            const double* __restrict__ rays,
                                                            const double* __restrict__ max_dist,
                                                            size_t n, uint8_t* __restrict__ out) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    d3 o = mk(0.0, 0.0, 0.0), d = mk(0.0, 0.0, 0.0);
    double md = 0.0;
    if (valid) {
        const double* r = rays + 6 * i;
        o = mk(r[0], r[1], r[2]);
        d = mk(r[3], r[4], r[5]);
        md = max_dist[i];
    }
    // maxDist NaN or <= 0: `within` holds for no t, the answer is 0 before any traversal
    bool done = !valid || !(md > 0.0);
    bool occ = false;
    const double a = dot(d, d);     // Shape.h:75, hoisted as in closest_t
    const double two_a = 2.0 * a;   // Shape.h:85-86 denominator
    const double four_a = 4.0 * a;  // Shape.h:79: (4.0 * a) * c
    for (int k = 0; k < P.ns; ++k) {
        if (__ballot(!done) == 0ull) break;
        double t;
        const bool h = any_sphere_t(P.sph + kSphStride * k, o, d, two_a, four_a, t) &&
                       any_within(t, md);
        if (h && !done) {
            occ = true;
            done = true;
        }
    }
    for (int k = 0; k < P.np; ++k) {
        if (__ballot(!done) == 0ull) break;
        double t;
        const bool h = any_plane_t(P.pl + kPlStride * k, o, d, t) && any_within(t, md);
        if (h && !done) {
            occ = true;
            done = true;
        }
    }
    if (P.bvh) {
        // lanes decided by a sphere or a plane skip the traversal
        if (!done) occ = any_bvh_triangles(P.tri, P.bvh, P.bvh_tri, o, d, md);
    } else {
        for (int k = 0; k < P.nt; ++k) {
            if (__ballot(!done) == 0ull) break;
            double t;
            const bool h = tri_hit(P.tri, k, o, d, t) && t < md;  // t > 1e-6 already
            if (h && !done) {
                occ = true;
                done = true;
            }
        }
    }
    if (valid) out[i] = occ ? uint8_t(1) : uint8_t(0);
}

hipError_t launch_occluded_rays(const TraceParams& p, const double* rays, const double* max_dist,
                                size_t n, uint8_t* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(occluded_rays_kernel, dim3(static_cast<unsigned>((n + 255) / 256)),
                       dim3(256), 0, stream, p, rays, max_dist, n, out);
    return hipGetLastError();
}

}  // namespace rtamd
