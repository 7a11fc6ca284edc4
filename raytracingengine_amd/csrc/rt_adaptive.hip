// rt_adaptive.hip — adaptive progressive frames for gfx950 (MI355X): rt_accumulate.hip's sum,
// continued per pixel only while a stop rule on the pixel's own samples asks for more, and a
// resolve that divides each pixel by its own count.
//
// The rule (include/rt_capi.h, rt_accumulate_adaptive_device) is written once: adaptive_wants /
// adaptive_converged decide, adaptive_sample is the loop body — accumulate_samples_kernel's ray,
// key and TraceRay (rt_trace_common.hpp), GeneratePixelAt's fold (Scene.h:289-297) and the two
// luminance moments.  It is re-examined before every sample, so a pixel's count, sum and moments
// depend on its sample sequence alone: not on how calls cut the range, on the launch shape, or on
// which of the two kernels below traced a sample.
//
// adaptive_tile_kernel runs one thread per pixel, a wave an 8x8 tile, while at least half of the
// wave's pixels still want samples; what is left is appended to a device-side list (one atomic
// per wave) and adaptive_list_kernel finishes it 64 listed pixels to a wave.  Without a list
// (RTAMD_ADAPT_LIST=0) the tile kernel runs every pixel to its end.
#include "rt_trace_common.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// IEEE binary64, one rounding per operation; false for a NaN anywhere.
__device__ __forceinline__ bool adaptive_converged(const AdaptiveArgs& A, int n, double m1,
                                                   double m2) {
    const double nd = static_cast<double>(n);
    const double mean = m1 / nd;
    const double var = (m2 - m1 * mean) / (nd - 1.0);
    const double err2 = var / nd;  // squared standard error of the mean luminance
    const double ref = mean > A.lum_floor ? mean : A.lum_floor;
    const double lim = A.tolerance * ref;
    return err2 <= lim * lim;
}

// A pixel's state without its sum (which only a pixel that takes a sample reads).
struct AdaptiveMoments {
    double m1, m2;
    int n;
};

// The head of the rule's loop: whether the pixel takes sample n.
__device__ __forceinline__ bool adaptive_wants(const AdaptiveArgs& A, const AdaptiveMoments& m) {
    if (m.n >= A.sample_end) return false;
    return !(m.n >= A.min_samples && adaptive_converged(A, m.n, m.m1, m.m2));
}

// The body of the rule's loop: sample m.n of image pixel (x, y).
template <int PATH>
__device__ __forceinline__ void adaptive_sample(const SceneView& S, const TraceParams& P, d3 cam,
                                                uint32_t x, uint32_t y, uint64_t pix, d3& sum,
                                                AdaptiveMoments& m, Counts& cnt) {
    const d3 dir = camera_dir(P, cam, x, y, pix, m.n);
    const uint32_t s = static_cast<uint32_t>(m.n);
    d3 c;
    if constexpr (PATH == kPathDirect) c = trace_direct<false>(S, P, cam, dir, pix, s, cnt);
    else if constexpr (PATH == kPathChain) c = trace_chain<false>(S, P, cam, dir, pix, s, cnt);
    else c = trace_tree<false>(S, P, cam, dir, pix, s, cnt);
    sum = sum + c;
    const double L = luminance(c);
    m.m1 = m.m1 + L;
    m.m2 = m.m2 + L * L;
    m.n = m.n + 1;
}

// The state of row-local pixel o.  fresh: nothing is read, the rule starts at +0.0 / 0.
__device__ __forceinline__ AdaptiveMoments adaptive_load(const AdaptiveArgs& A, size_t o) {
    if (A.fresh) return AdaptiveMoments{0.0, 0.0, 0};
    return AdaptiveMoments{A.moments[2 * o], A.moments[2 * o + 1], A.count[o]};
}
__device__ __forceinline__ d3 adaptive_load_sum(const AdaptiveArgs& A, size_t o) {
    if (A.fresh) return mk(0.0, 0.0, 0.0);
    return mk(A.sum[3 * o], A.sum[3 * o + 1], A.sum[3 * o + 2]);
}
__device__ __forceinline__ void adaptive_store(const AdaptiveArgs& A, size_t o, d3 sum,
                                               const AdaptiveMoments& m) {
    A.sum[3 * o + 0] = sum.x;
    A.sum[3 * o + 1] = sum.y;
    A.sum[3 * o + 2] = sum.z;
    A.moments[2 * o + 0] = m.m1;
    A.moments[2 * o + 1] = m.m2;
    A.count[o] = m.n;
}

// One thread per pixel of the row set, accumulate_samples_kernel's launch shape.  The wave samples
// in place while at least half of its pixels want a sample (in a fresh call: every pixel up to
// min_samples, then until half have stopped); the pixels that still want one are then appended
// to A.list.  A pixel that took no sample is not written (a fresh call writes every pixel).
template <int PATH>
__global__ __launch_bounds__(kTileW * kTileH, 2) void adaptive_tile_kernel(TraceParams P,
                                                                           AdaptiveArgs A) {
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    const uint32_t x = blockIdx.x * kTileW + threadIdx.x;
    const uint32_t yl = blockIdx.y * kTileH + threadIdx.y;
    const bool valid = x < P.width && yl < P.rows;
    const uint32_t y = image_row(P, valid ? yl : 0u);
    const uint64_t pix = static_cast<uint64_t>(y) * P.width + x;
    const size_t o = static_cast<size_t>(yl) * P.width + x;
    const d3 cam = mk(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    AdaptiveMoments m{0.0, 0.0, 0};
    d3 sum = mk(0.0, 0.0, 0.0);
    bool active = false;
    if (valid) {
        m = adaptive_load(A, o);
        active = adaptive_wants(A, m);
        if (active) sum = adaptive_load_sum(A, o);
    }
    const bool touched = active || (valid && A.fresh);
    const int keep = __builtin_popcountll(__ballot(valid));
    Counts cnt{0u, 0u};
    uint64_t live = __ballot(active);
    while (live && !(A.list && 2 * __builtin_popcountll(live) < keep)) {
        if (active) {
            adaptive_sample<PATH>(S, P, cam, x, y, pix, sum, m, cnt);
            active = adaptive_wants(A, m);
        }
        live = __ballot(active);
    }
    if (touched) adaptive_store(A, o, sum, m);
    if (live) {  // only with a list: the wave-aggregated append of rt_packet_epilogue.hpp
        const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int first = __builtin_ctzll(live);
        uint32_t base = 0;
        if (lane == static_cast<uint32_t>(first))
            base = atomicAdd(A.list_count, static_cast<uint32_t>(__builtin_popcountll(live)));
        base = __shfl(base, first, 64);
        if (active)
            A.list[base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(live >> 32),
                                                    __builtin_amdgcn_mbcnt_lo(
                                                        static_cast<uint32_t>(live), 0u))] =
                static_cast<uint32_t>(o);
    }
}

// The listed pixels, one lane each, run to the end of the rule's loop: a persistent grid over the
// device-side count, as packet_fixup_kernel's — the count is read from device memory, waves past
// the list return before anything else, and the host never learns the count.  A workgroup is one
// wave, so the hardware hands out the list 64 entries at a time as waves retire.
constexpr int kAdaptListThreads = 64;
constexpr int kAdaptListBlocks = 8192;
template <int PATH>
__global__ __launch_bounds__(kAdaptListThreads, 2) void adaptive_list_kernel(TraceParams P,
                                                                             AdaptiveArgs A) {
    const uint32_t n = *A.list_count;  // the tile launch before this one on the stream appended
    if (blockIdx.x * kAdaptListThreads >= n) return;
    const SceneView S = stage_scene<false>(P, nullptr, 0, 0);
    const d3 cam = mk(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    Counts cnt{0u, 0u};
    for (uint32_t i = blockIdx.x * kAdaptListThreads + threadIdx.x; i < n;
         i += gridDim.x * kAdaptListThreads) {
        const uint32_t o = A.list[i];  // row-local pixel (the launch's pixels are < 2^32)
        const uint32_t yl = o / P.width;
        const uint32_t x = o - yl * P.width;
        const uint32_t y = image_row(P, yl);
        const uint64_t pix = static_cast<uint64_t>(y) * P.width + x;
        // the tile kernel stored the state of every pixel it listed, a fresh call's included
        AdaptiveMoments m{A.moments[2 * static_cast<size_t>(o)],
                          A.moments[2 * static_cast<size_t>(o) + 1], A.count[o]};
        d3 sum = mk(A.sum[3 * static_cast<size_t>(o)], A.sum[3 * static_cast<size_t>(o) + 1],
                    A.sum[3 * static_cast<size_t>(o) + 2]);
        while (adaptive_wants(A, m)) adaptive_sample<PATH>(S, P, cam, x, y, pix, sum, m, cnt);
        adaptive_store(A, o, sum, m);
    }
}

hipError_t launch_accumulate_adaptive(const TraceParams& p, int path, const AdaptiveArgs& a,
                                      hipStream_t stream) {
    if (p.width == 0 || p.rows == 0 || a.sample_end < 1 || a.min_samples < 2 || !a.sum ||
        !a.moments || !a.count || (a.list && !a.list_count))
        return hipErrorInvalidValue;
    const dim3 block(kTileW, kTileH);
    const dim3 grid((p.width + kTileW - 1) / kTileW, (p.rows + kTileH - 1) / kTileH);
    const dim3 lblock(kAdaptListThreads), lgrid(kAdaptListBlocks);
    auto launch = [&](auto tile, auto list) {
        hipLaunchKernelGGL(tile, grid, block, 0, stream, p, a);
        if (a.list) hipLaunchKernelGGL(list, lgrid, lblock, 0, stream, p, a);
    };
    if (path == kPathDirect)
        launch(adaptive_tile_kernel<kPathDirect>, adaptive_list_kernel<kPathDirect>);
    else if (path == kPathChain)
        launch(adaptive_tile_kernel<kPathChain>, adaptive_list_kernel<kPathChain>);
    else
        launch(adaptive_tile_kernel<kPathTree>, adaptive_list_kernel<kPathTree>);
    return hipGetLastError();
}

// resolve_kernel with the pixel's own divisor: v = sum / (double)count, {0, 0, 0} for a pixel
// without a sample (GeneratePixelAt, Scene.h:298-303: its sum is not read), then resolve_store.
__global__ __launch_bounds__(256) void resolve_counts_kernel(const double* sum,
                                                             const int32_t* __restrict__ count,
                                                             size_t n, int op, double* out64,
                                                             float* __restrict__ out32,
                                                             uint8_t* __restrict__ ldr) {
    const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t k = count[i];
    d3 c = mk(0.0, 0.0, 0.0);
    if (k > 0) c = sdiv(mk(sum[3 * i], sum[3 * i + 1], sum[3 * i + 2]), static_cast<double>(k));
    resolve_store(c, i, n, op, out64, out32, ldr);
}

hipError_t launch_resolve_counts(const double* sum, const int32_t* count, size_t n, int op,
                                 double* out64, float* out32, uint8_t* ldr, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!sum || !count || (!out64 && !out32 && !ldr) || (ldr && (op < 0 || op > 7)))
        return hipErrorInvalidValue;
    const unsigned blocks = static_cast<unsigned>((n + 255) / 256);
    hipLaunchKernelGGL(resolve_counts_kernel, dim3(blocks), dim3(256), 0, stream, sum, count, n, op,
                       out64, out32, ldr);
    return hipGetLastError();
}

}  // namespace rtamd
