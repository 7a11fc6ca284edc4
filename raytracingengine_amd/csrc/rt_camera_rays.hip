// rt_camera_rays.hip — the renderer's own primary rays for gfx950 (MI355X), written out:
// Camera::getRay(x, y, sample > 0 && aa_samples > 1) (Math.h:99-121) for every pixel of a
// launch's row set, {o, d} per pixel, rows-local like the frame (idx = y_local * W + x).
//
// The direction is camera_dir (rt_trace_common.hpp), the function the render kernels call, with
// the key they pass it: pix = y_image * W + x, the sample's index, and the seed of the launch.
// Nothing of Math.h is restated here, so the rays are the frame's, sample by sample.  No scene is
// read.
#include "rt_trace_common.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// One thread per pixel, x fastest: a wave is 64 consecutive pixels of a row and stores 64 · 48
// contiguous bytes (six 8-byte stores per lane at a 48-byte lane stride).
constexpr int kCrW = 64, kCrH = 4;
__global__ __launch_bounds__(kCrW * kCrH) void camera_rays_kernel(TraceParams P, int sample,
                                                                  double* __restrict__ out) {
    const uint32_t x = blockIdx.x * kCrW + threadIdx.x;
    const uint32_t yl = blockIdx.y * kCrH + threadIdx.y;
    if (x >= P.width || yl >= P.rows) return;
    const uint32_t y = image_row(P, yl);
    const d3 cam = mk(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    const uint64_t pix = static_cast<uint64_t>(y) * P.width + x;
    const d3 d = camera_dir(P, cam, x, y, pix, sample);
    double* w = out + 6 * (static_cast<size_t>(yl) * P.width + x);
    w[0] = cam.x;
    w[1] = cam.y;
    w[2] = cam.z;
    w[3] = d.x;
    w[4] = d.y;
    w[5] = d.z;
}

hipError_t launch_camera_rays(const TraceParams& p, int sample, double* out, hipStream_t stream) {
    if (p.width == 0 || p.rows == 0 || sample < 0) return hipErrorInvalidValue;
    const dim3 block(kCrW, kCrH);
    const dim3 grid((p.width + kCrW - 1) / kCrW, (p.rows + kCrH - 1) / kCrH);
    hipLaunchKernelGGL(camera_rays_kernel, grid, block, 0, stream, p, sample, out);
    return hipGetLastError();
}

}  // namespace rtamd
