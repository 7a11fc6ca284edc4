// rt_closest.hip — the batch closest-hit query with selectable outputs for gfx950 (MI355X):
// Scene::IntersectClosest (Scene.h:218-257) for n caller-supplied rays, each requested output a
// structure-of-arrays plane: distance, primitive {type, index}, geometric normal, hit point and
// the hit primitive's material.
//
// The body is closest, normal_of and material_of (rt_trace_common.hpp), what intersect_rays_kernel
// (rt_trace.hip) runs: ties, the strict '<' and every root are theirs, so t, normal, point and
// prim carry the bits rt_intersect_rays returns for the same ray.  FULL selects whether anything
// beyond t and prim is wanted: without it normal_of, the hit point and the material read are not
// compiled in (the split of scatter's DIRECT / CHILDREN).
// The scene is read through stage_scene<false>: the records stay in HBM, as in
// intersect_rays_kernel, whose global_view is the same set of pointers.
// The triangle BVH's traversal stack (kBvhStack node indices per ray) is the one thing these
// kernels hold differently: in LDS (BvhStackLds), not in private memory, so they have no private
// segment at all.  The traversal, its order and its ties are bvh_triangles' own.
#include "rt_trace_common.hpp"

#pragma clang fp contract(off)

namespace rtamd {

__device__ __forceinline__ void ch_store3(double* base, size_t i, bool hit, d3 v) {
    if (!base) return;
    double* w = base + 3 * i;
    w[0] = hit ? v.x : 0.0;
    w[1] = hit ? v.y : 0.0;
    w[2] = hit ? v.z : 0.0;
}

constexpr unsigned kChBvhThreads = 64;  // workgroup of the launches whose scene has a triangle BVH

// One thread per ray {o, d}.  A miss: t = +inf, prim = {0, -1}, +0.0 elsewhere (the G-buffer's
// rule).  Null output pointers are wave-uniform kernel arguments: scalar branches.
template <bool FULL>
__global__ __launch_bounds__(256) void closest_rays_kernel(TraceParams P,
                                                           const double* __restrict__ rays, size_t n,
                                                           ChOut out) {
    extern __shared__ int ch_stack[];  // kBvhStack entries per thread when P.bvh is set, else none
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rays + 6 * i;
    const d3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    Hit h;
    const bool hit = closest(S, o, d, h, BvhStackLds{ch_stack + threadIdx.x, static_cast<int>(blockDim.x)});
    if (out.t) out.t[i] = hit ? h.t : INFINITY;
    if (out.prim) reinterpret_cast<int2*>(out.prim)[i] = make_int2(hit ? h.kind : 0, hit ? h.idx : -1);
    if constexpr (FULL) {
        d3 p = mk(0.0, 0.0, 0.0), nn = mk(0.0, 0.0, 0.0);
        double m[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (hit) {
            p = o + d * h.t;
            nn = normal_of(S, h, p);
            if (out.material) {  // rt_material's seven members head the kMatStride record
                const double* mat = material_of(S, h);
                for (int k = 0; k < 7; ++k) m[k] = mat[k];
            }
        }
        ch_store3(out.normal, i, hit, nn);
        ch_store3(out.point, i, hit, p);
        if (out.material) {
            double* w = out.material + 7 * i;
            for (int k = 0; k < 7; ++k) w[k] = m[k];
        }
    }
}

// At least one output is set (the entries reject outputs == 0).
hipError_t launch_closest_rays(const TraceParams& p, const double* rays, size_t n, const ChOut& out,
                               hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const bool lean = out.t || out.prim;
    const bool full = out.normal || out.point || out.material;
    if (!lean && !full) return hipErrorInvalidValue;
    // scenes with a triangle BVH: one wave per workgroup and its 16 KiB of traversal stacks in
    // LDS; every other scene: 256 threads, no LDS
    const unsigned threads = p.bvh ? kChBvhThreads : 256;
    const size_t lds = p.bvh ? sizeof(int) * kBvhStack * kChBvhThreads : 0;
    const dim3 grid(static_cast<unsigned>((n + threads - 1) / threads)), block(threads);
    if (full)
        hipLaunchKernelGGL(closest_rays_kernel<true>, grid, block, lds, stream, p, rays, n, out);
    else
        hipLaunchKernelGGL(closest_rays_kernel<false>, grid, block, lds, stream, p, rays, n, out);
    return hipGetLastError();
}

}  // namespace rtamd
