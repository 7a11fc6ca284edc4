// rt_accumulate.hip — progressive frames for gfx950 (MI355X): GeneratePixelAt (Scene.h:283-304)
// cut at any AA sample.  accumulate_samples_kernel adds the samples [s0, s1) of every pixel of a
// launch's row set to a resident float64 sum, in the reference's order of the loop
// (Scene.h:289-297); resolve_kernel divides a sum by its sample count (Scene.h:298-300) and writes
// what store_pixel writes: the float64 and float32 pixels and the tonemapped bytes.
//
// Nothing of the renderer is restated here.  The ray of sample s is camera_dir's with the render
// kernels' key (pix = y_image * W + x, s, the launch's seed), TraceRay is trace_direct /
// trace_chain / trace_tree (rt_trace_common.hpp) over the scene in HBM — the functions and the
// SceneView trace_rays_kernel (rt_trace.hip) runs — and (pix, s) is also what they key the area
// light's random numbers by, as trace_kernel does.  So
//   resolve(accumulate(0, N), N) == rt_render_device's frame
// wherever the frame equals (Σ_s TraceRay(camera ray of sample s)) / N, and the composition's
// per-sample traffic (48 B of ray and 24 B of colour written and read back, a 24 B sum read and
// written by the add) stays in registers: the sum is read once (not at all when s0 == 0) and
// written once per launch.
#include "rt_trace_common.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// One thread per pixel of the row set, a wave an 8×8 tile like trace_kernel's (the rays of a
// square tile stay together down a reflection chain).  Compiled for 2 waves per SIMD, the budget
// of the generic trace kernels.
template <int PATH>
__global__ __launch_bounds__(kTileW * kTileH, 2) void accumulate_samples_kernel(
    TraceParams P, int s0, int s1, double* __restrict__ sum) {
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    const uint32_t x = blockIdx.x * kTileW + threadIdx.x;
    const uint32_t yl = blockIdx.y * kTileH + threadIdx.y;
    if (x >= P.width || yl >= P.rows) return;
    const uint32_t y = image_row(P, yl);
    const uint64_t pix = static_cast<uint64_t>(y) * P.width + x;
    const d3 cam = mk(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    double* w = sum + 3 * (static_cast<size_t>(yl) * P.width + x);
    // s0 == 0 starts GeneratePixelAt's +0.0 accumulator: what the buffer held is not read
    d3 acc = mk(0.0, 0.0, 0.0);
    if (s0 > 0) acc = mk(w[0], w[1], w[2]);  // uniform
    Counts cnt{0u, 0u};
    for (int s = s0; s < s1; ++s) {
        const d3 dir = camera_dir(P, cam, x, y, pix, s);
        d3 c;
        if constexpr (PATH == kPathDirect)
            c = trace_direct<false>(S, P, cam, dir, pix, static_cast<uint32_t>(s), cnt);
        else if constexpr (PATH == kPathChain)
            c = trace_chain<false>(S, P, cam, dir, pix, static_cast<uint32_t>(s), cnt);
        else
            c = trace_tree<false>(S, P, cam, dir, pix, static_cast<uint32_t>(s), cnt);
        acc = acc + c;
    }
    w[0] = acc.x;
    w[1] = acc.y;
    w[2] = acc.z;
}

hipError_t launch_accumulate_samples(const TraceParams& p, int path, int s0, int s1, double* sum,
                                     hipStream_t stream) {
    if (p.width == 0 || p.rows == 0 || s0 < 0 || s0 >= s1 || !sum) return hipErrorInvalidValue;
    const dim3 block(kTileW, kTileH);
    const dim3 grid((p.width + kTileW - 1) / kTileW, (p.rows + kTileH - 1) / kTileH);
    if (path == kPathDirect)
        hipLaunchKernelGGL(accumulate_samples_kernel<kPathDirect>, grid, block, 0, stream, p, s0, s1, sum);
    else if (path == kPathChain)
        hipLaunchKernelGGL(accumulate_samples_kernel<kPathChain>, grid, block, 0, stream, p, s0, s1, sum);
    else
        hipLaunchKernelGGL(accumulate_samples_kernel<kPathTree>, grid, block, 0, stream, p, s0, s1, sum);
    return hipGetLastError();
}

// One thread per pixel: v = sum / samples, the division trace_kernel makes before store_pixel
// (sdiv), then the requested outputs.  The bytes are tonemap_kernel's (rt_trace.hip): tonemap_op +
// to_color, reinhard_byte for operator 1; op == 7 writes the seven operators' planes in
// tonemapAll() order.  op < 0: no bytes (ldr is null).  out64 may be the sum itself (a thread reads
// its pixel before it writes it).
__global__ __launch_bounds__(256) void resolve_kernel(const double* sum, size_t n,
                                                      double samples, int op,
                                                      double* out64,
                                                      float* __restrict__ out32,
                                                      uint8_t* __restrict__ ldr) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const d3 c = sdiv(mk(sum[3 * i], sum[3 * i + 1], sum[3 * i + 2]), samples);
    resolve_store(c, i, n, op, out64, out32, ldr);
}

hipError_t launch_resolve(const double* sum, size_t n, int samples, int op, double* out64,
                          float* out32, uint8_t* ldr, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!sum || samples < 1 || (!out64 && !out32 && !ldr) || (ldr && (op < 0 || op > 7)))
        return hipErrorInvalidValue;
    const unsigned blocks = static_cast<unsigned>((n + 255) / 256);
    hipLaunchKernelGGL(resolve_kernel, dim3(blocks), dim3(256), 0, stream, sum, n,
                       static_cast<double>(samples), op, out64, out32, ldr);
    return hipGetLastError();
}

}  // namespace rtamd
