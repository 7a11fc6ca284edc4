// rt_packet.hip — the packet kernel's translation unit (rt_packet_kernel.hpp), the only one
// scheduled for ILP: every variant of packet_direct_kernel but the area light's
// (rt_packet_area.hip) with the dispatch that picks one, and the auxiliary kernels of the
// packet path with their launchers — the camera image (one, or a batch's), the fix-up of
// queued pixels and the costliest-first tile order.
#include "rt_cone_table.hpp"
#include "rt_packet_kernel.hpp"
#include "rt_shadow_table.hpp"

#pragma clang fp contract(off)

namespace rtamd {

#ifdef RT_PACKET_PROBE
// tools/isa/probe.sh: one instantiation only (register / ISA studies of a single variant)
template __global__ void packet_direct_kernel<RT_PACKET_PROBE>(TraceParams);
#else
size_t packet_lds_bytes(int ns, int np, int nl) { return pk_image_bytes(ns, np, nl); }

__global__ __launch_bounds__(256) void packet_image_kernel(TraceParams P, double* img) {
    pk_build_image(P, P.cam_pos, img, static_cast<int>(threadIdx.x), 256);
}

hipError_t launch_packet_image(const TraceParams& p, double* img, hipStream_t stream) {
    hipLaunchKernelGGL(packet_image_kernel, dim3(1), dim3(256), 0, stream, p, img);
    return hipGetLastError();
}

// The images of a frame batch's uncached cameras, one workgroup per job (pk_build_image: the
// same words a workgroup of the batch launch would form for itself), each written where the
// host put it: a new cache entry (a camera seen before) or the batch's ring slot.
__global__ __launch_bounds__(256) void packet_image_batch_kernel(TraceParams P, PkImageJobs J) {
    const int f = J.frame[blockIdx.x];
    pk_build_image(P, P.fr[f].cam, J.dst[blockIdx.x], static_cast<int>(threadIdx.x), 256);
}

hipError_t launch_packet_image_batch(const TraceParams& p, const PkImageJobs& jobs,
                                     hipStream_t stream) {
    if (jobs.n <= 0) return hipSuccess;
    if (jobs.n > kPkMaxBatch) return hipErrorInvalidValue;
    for (int j = 0; j < jobs.n; ++j)
        if (!jobs.dst[j] || jobs.frame[j] < 0 || jobs.frame[j] >= static_cast<int>(p.nframes))
            return hipErrorInvalidValue;
    hipLaunchKernelGGL(packet_image_batch_kernel, dim3(static_cast<unsigned>(jobs.n)),
                       dim3(256), 0, stream, p, jobs);
    return hipGetLastError();
}

// The tile tables (rt_tile_table.hpp: the sections, their order and what each is formed from) of
// a launch's wave tiles, one lane per tile and one grid row per job: a one-frame launch's camera,
// or every frame of a batch that has no cached table, so a batch of new cameras pays one launch.
// The per-sphere terms are the packet image's (cone_terms), formed earlier on the stream.  The
// lane writes the sections J.contents names, in their order, and returns after the last.
// Tables are indexed by tile — (tby · gx + tbx) · waves + wave — not by dispatch position: the
// tile order permutes dispatch, not tiles.  With lists the lanes take the tiles from the last one
// down, and a wavefront is one run of list positions (tile_list_run, rt_shadow_table.hpp, is the
// same run in plain C++ and shares the helpers that decide): compacted with three ballots
// (uniform tiles, shadowed tiles, listed workgroups' first lanes) and given its place in each
// list by one atomic add per wavefront on the counts packet_list_zero_kernel zeroed before.
// The kernel waits more than it issues (dependent FP64 chains, one lane per tile), so it is
// built for 5 waves per SIMD (96 VGPRs, 104 B of scratch; by itself it compiles to 3): the
// measured times are in DESIGN §4 and profiles/shadow_table_pmc.txt.
constexpr int kConeThreads = 256;
__global__ __launch_bounds__(kConeThreads, 5) void packet_cone_table_kernel(TraceParams P,
                                                                         PkConeJobs J, uint32_t gx,
                                                                         uint32_t gy,
                                                                         uint32_t waves) {
    __shared__ float s_terms[64 * 8];
    __shared__ double s_ctr[64 * 3];  // the sphere centres, for the shadow words
    const int f = J.frame[blockIdx.y];
    const double* camp = f < 0 ? P.cam_pos : P.fr[f].cam;
    const double* img = f < 0 ? P.pk_image : P.fr[f].img;
    const double dz = f < 0 ? P.cam_dz : P.fr_dz[f][0];
    const int ns = P.ns < 64 ? P.ns : 64;  // (the launcher checked P.ns <= 64)
    for (int i = threadIdx.x; i < 8 * ns; i += kConeThreads)
        s_terms[i] = reinterpret_cast<const float*>(img + kPkSph * (i >> 3) + 4)[i & 7];
    const TileTabContents C = J.contents;
    if (C.has_shadow())
        for (int i = threadIdx.x; i < 3 * ns; i += kConeThreads)
            s_ctr[i] = img[kPkSph * (i / 3) + i % 3];
    __syncthreads();
    const uint32_t pos = blockIdx.x * kConeThreads + threadIdx.x;
    if (pos >= gx * gy * waves) return;
    // (every tile has one lane; with lists the lanes take the tiles from the last one down)
    const uint32_t t = C.has_lists() ? tile_list_tile(pos, gx * gy * waves) : pos;
    const uint32_t wave = t % waves, wg = t / waves, tbx = wg % gx, tby = wg / gx;
    const uint32_t x0 = tbx * (kPkW * kWgWavesX) + (wave % kWgWavesX) * kPkW;
    const uint32_t yl0 = tby * (kPkH * (waves / kWgWavesX)) + (wave / kWgWavesX) * kPkH;
    const ConeRowPlan rp{P.row0, P.rows, P.row_block, P.row_stride};
    const ConeRect q = cone_tile_rect(x0, yl0, P.width, rp);
    const ConeBound B = cone_tile_bound(q, P.half_w, P.half_h, camp[0], camp[1], dz);
    const uint64_t cone = cone_tile_mask(B, s_terms, 8, ns);
    const TileTabLayout L{static_cast<size_t>(gx) * gy * waves, static_cast<size_t>(gx) * gy, C};
    unsigned long long* tab = J.dst[blockIdx.y];
    tab[L.cone(t)] = cone;
    if (!C.has_shadow()) return;
    // (the launcher checked shadow_nl == P.nl <= kShadowTabLights, P.np <= 2 and ns <= 63: no
    // chunk bounds, so the image's planes follow its ns sphere records)
    unsigned long long* sw = tab + L.shadow(t, 0);
    // (two planes at most: scenes of three or more take the plane-culling variant, no table)
    ShadowBound<2> SB;
    SB.n = 0;
    SB.ok = false;
    if (cone == 0)
        SB = shadow_tile_bound<2>(q, P.half_w, P.half_h, camp, dz, img + kPkSph * ns, P.np, P.bias);
    // (each light's shadow-plane keep mask too when the class words carry them, shadow_plane_keep:
    // it rides in the class word, tile_class_pack; else all ones, nothing is taken as proven)
    unsigned long long any = 0, keep = 0;
    for (int l = 0; l < C.shadow_nl; ++l) {
        sw[l] = shadow_tile_word(SB, P.lt + kLtStride * l, P.bias, s_ctr, 3, s_terms + 7, 8, ns);
        any |= sw[l];
        const unsigned k = C.forms_keep()
                               ? shadow_plane_keep<2>(SB, P.lt + kLtStride * l, img + kPkSph * ns,
                                                      P.np, camp, P.bias)
                               : kPlaneKeepAll;
        keep |= static_cast<unsigned long long>(k) << (8 + 8 * l);
    }
    if (!C.has_class()) return;
    // the tile's class word (tile_class_word), after every tile's shadow words; s_pln of the
    // image follows its planes and lights (pk_build_image).  The OR of the tile's shadow words
    // stands for them (zero iff every one is; the launcher checked shadow_nl <= kShadowTabLights)
    const double* pln = img + kPkSph * ns + kPlStride * P.np + kLtStride * P.nl;
    // (with the third list: the shadowed-plane mark too, tile_shadowed_mark.  `any` stands for
    // the words here as well: a real word has no bit 63, so their OR is all ones iff one is)
    const unsigned long long mark =
        C.forms_mark() ? tile_shadowed_mark(cone, SB, &any, 1, pln, P.np) : 0ull;
    const unsigned long long cw = tile_class_word(cone, SB, &any, 1, pln, P.np) | keep | mark;
    tab[L.cls(t)] = cw;
    if (!C.has_lists()) return;
    // the tile lists: the active lanes of this wavefront are a run's first lanes (lane 0 among
    // them), and a workgroup's tiles are `waves` adjacent lanes
    // (the counts word's halves: TileListCounts)
    uint32_t* n_ug = reinterpret_cast<uint32_t*>(tab + L.list_counts());
    unsigned long long* uni = tab + L.uniform(0);
    uint32_t* gen = reinterpret_cast<uint32_t*>(tab + L.general_base());
    const uint32_t lane = threadIdx.x & 63u;
    const bool is_uni = tile_list_uniform(cw), is_sh = tile_list_shadowed(cw);
    const uint64_t bu = __ballot(is_uni), bs = __ballot(is_sh), bg = __ballot(!is_uni && !is_sh);
    const bool lead = (lane & (waves - 1u)) == 0 && tile_list_wg_listed(bg, lane, waves);
    const uint64_t bl = __ballot(lead);
    uint32_t base_u = 0, base_g = 0, base_s = 0;
    if (lane == 0) {
        if (bu) base_u = atomicAdd(n_ug, static_cast<uint32_t>(__builtin_popcountll(bu)));
        if (bl) base_g = atomicAdd(n_ug + 1, static_cast<uint32_t>(__builtin_popcountll(bl)));
        if (bs)
            base_s = atomicAdd(reinterpret_cast<uint32_t*>(tab + L.shadowed_count()),
                               static_cast<uint32_t>(__builtin_popcountll(bs)));
    }
    base_u = __shfl(base_u, 0, 64);
    base_g = __shfl(base_g, 0, 64);
    base_s = __shfl(base_s, 0, 64);
    const uint64_t below = (1ull << lane) - 1ull;
    if (is_uni) uni[base_u + __builtin_popcountll(bu & below)] = tile_list_entry(cw, x0, yl0);
    if (is_sh)
        uni[TileTabLayout::shadowed_slot(base_s + __builtin_popcountll(bs & below),
                                         static_cast<uint32_t>(L.tiles))] =
            tile_shadowed_entry(cw, x0, yl0);
    if (lead) gen[base_g + __builtin_popcountll(bl & below)] = wg;
}

// The list counts of a table launch's jobs: zeroed before it, and handed to the host after it
// (tile_list_counts_encode, into two pinned words) where the table has a cache entry.
__global__ __launch_bounds__(64) void packet_list_zero_kernel(PkConeJobs J, TileTabLayout L) {
    if (static_cast<int>(threadIdx.x) >= J.n) return;
    J.dst[threadIdx.x][L.list_counts()] = 0ull;
    J.dst[threadIdx.x][L.shadowed_count()] = 0ull;
}
__global__ __launch_bounds__(64) void packet_list_counts_kernel(PkConeJobs J, PkListCounts C,
                                                                TileTabLayout L) {
    if (static_cast<int>(threadIdx.x) >= J.n || !C.host[threadIdx.x]) return;
    unsigned long long w[2];
    tile_list_counts_encode(tile_list_counts(J.dst[threadIdx.x][L.list_counts()],
                                             J.dst[threadIdx.x][L.shadowed_count()]), w);
    __hip_atomic_store(C.host[threadIdx.x], w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(C.host[threadIdx.x] + 1, w[1], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_packet_cone_tables(const TraceParams& p, const PkConeJobs& jobs,
                                     hipStream_t stream, const PkListCounts* counts) {
    if (jobs.n <= 0) return hipSuccess;
    if (jobs.n > kPkMaxBatch || p.ns > 64 || p.width == 0 || p.rows == 0)
        return hipErrorInvalidValue;
    const TileTabContents C = jobs.contents;
    if (!C.valid() || (C.has_shadow() && C.shadow_nl != packet_shadow_table_lights(p)))
        return hipErrorInvalidValue;
    for (int j = 0; j < jobs.n; ++j) {
        const int f = jobs.frame[j];
        if (!jobs.dst[j] || f < -1 || f >= static_cast<int>(p.nframes) ||
            !(f < 0 ? p.pk_image : p.fr[f].img))
            return hipErrorInvalidValue;
    }
    uint32_t gx, gy, waves;
    packet_grid(p, gx, gy, waves);
    const uint32_t tiles = gx * gy * waves;
    const TileTabLayout L{tiles, static_cast<size_t>(gx) * gy, C};
    if (C.has_lists()) {
        // (a list entry names a tile by 12-bit column and row: packet_split_wanted)
        if (gx * kWgWavesX > kListMaxCoord || gy * (waves / kWgWavesX) > kListMaxCoord)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(packet_list_zero_kernel, dim3(1), dim3(64), 0, stream, jobs, L);
    }
    hipLaunchKernelGGL(packet_cone_table_kernel,
                       dim3((tiles + kConeThreads - 1) / kConeThreads,
                            static_cast<unsigned>(jobs.n)),
                       dim3(kConeThreads), 0, stream, p, jobs, gx, gy, waves);
    if (C.has_lists() && counts)
        hipLaunchKernelGGL(packet_list_counts_kernel, dim3(1), dim3(64), 0, stream, jobs, *counts,
                           L);
    return hipGetLastError();
}

// The pixels a fix-up variant queued (TraceParams.fix_list: output index frame · frame_px + row-
// local pixel): GeneratePixelAt (Scene.h:283-304) with one sample through the per-pixel path —
// generic closest hit over every primitive, occlusion_opaque and the exact computeTransmittance
// march (rt_trace_common.hpp trace_direct) — the same image bits as the packet kernel, stored
// like it.  A persistent grid over the device-side count; it zeroes the count the next
// fix-variant launch uses (the two alternate, no memset on the stream), and workgroups past
// the list return before staging.  The scene records are staged into LDS when
// they fit.  Its cost is per wave, ~2 300 VALU + 1 100 SALU (~45k cycles) each: one wave per
// 64 queued pixels is the fastest arrangement — 16, 8 or 4 pixels per wave (more waves per SIMD)
// took 75 / 152 / 334 µs against 26 µs per 32-frame C2 batch, lanes of a group sharing one
// pixel's sphere loops 42 µs, a per-ray capsule mask for the marches no change
// (profiles/r05_ab_fixup.txt).
constexpr int kFixThreads = 256;
constexpr int kFixBlocks = 256;
template <bool LDS>
__global__ __launch_bounds__(kFixThreads) void packet_fixup_kernel(TraceParams P) {
    extern __shared__ double smem[];
    const uint32_t n = *P.fix_ctl;  // the packet launch before this one on the stream appended
    // the count the context's next fix-variant launch appends to: zeroed here, where nothing
    // reads it (the launch before this one's fix-up read it, and the next packet launch is
    // ordered after this one) — round 6: replaces 256 same-address completion atomics and
    // fences (the launch's floor, profiles/r06_fixup_ab.txt)
    if (blockIdx.x == 0 && threadIdx.x == 0) *P.fix_next = 0u;
    // workgroups past the list skip the scene staging (uniform per workgroup)
    if (blockIdx.x * kFixThreads >= n) return;
    // the fix-up variants' scenes: spheres, planes and point lights, no specular material, so
    // no triangle, BVH, area-light or pow code is compiled in (229 -> 167 VGPRs, 288 -> 40 B of
    // scratch: 27.5 -> 26 µs per 32-frame batch)
    SceneView S = stage_scene<LDS>(P, smem, threadIdx.x, kFixThreads);
    S.nt = 0;
    S.al = 0;
    S.spec = false;
    S.tri = S.tri_mat = S.bvh = nullptr;
    S.bvh_tri = nullptr;
    Counts cnt{0u, 0u};
    // (list entries are 32-bit output indices: the launch's pixels are < 2^32, fixup_buffers)
    const uint32_t fpx = P.nframes ? static_cast<uint32_t>(P.frame_px) : 0u;
    for (uint32_t i = blockIdx.x * kFixThreads + threadIdx.x; i < n; i += gridDim.x * kFixThreads) {
        const uint32_t o = P.fix_list[i];
        const uint32_t z = fpx ? o / fpx : 0u;
        const uint32_t pl = o - z * fpx;
        const uint32_t yl = pl / P.width;
        const uint32_t x = pl - yl * P.width;
        const double* cp = P.nframes ? P.fr[z].cam : P.cam_pos;
        const d3 cam = mk(cp[0], cp[1], cp[2]);
        const uint32_t y = image_row(P, yl);
        const uint64_t pix = static_cast<uint64_t>(y) * P.width + x;
        const d3 d = camera_dir(P, cam, x, y, pix, 0);
        d3 acc = mk(0.0, 0.0, 0.0);
        acc = acc + trace_direct<false>(S, P, cam, d, pix, 0u, cnt);  // one sample (AA = 1)
        store_pixel(P, static_cast<size_t>(o), acc);
    }
}

hipError_t launch_packet_fixup(const TraceParams& p, hipStream_t stream) {
    if (!p.fix_list || !p.fix_ctl || !p.fix_next) return hipErrorInvalidValue;
    if (p.nt != 0 || p.al_samples != 0) return hipErrorInvalidValue;  // the lean scene view
    const size_t lds = sizeof(double) * scene_doubles(p);
    if (lds <= 32 * 1024)
        hipLaunchKernelGGL(packet_fixup_kernel<true>, dim3(kFixBlocks), dim3(kFixThreads), lds,
                           stream, p);
    else
        hipLaunchKernelGGL(packet_fixup_kernel<false>, dim3(kFixBlocks), dim3(kFixThreads), 0,
                           stream, p);
    return hipGetLastError();
}

int packet_max_spheres() { return 16 * 64; }

void packet_grid(const TraceParams& p, uint32_t& gx, uint32_t& gy, uint32_t& waves) {
    const size_t lds = pk_image_bytes(p.ns, p.np, p.nl);
    const uint32_t wgy = pk_wgy(lds);
    gx = (p.width + kPkW * kWgWavesX - 1) / (kPkW * kWgWavesX);
    gy = (p.rows + kPkH * wgy - 1) / (kPkH * wgy);
    waves = kWgWavesX * wgy;
}

// Costliest tiles first: the tile order of the next launches from the wave durations one launch
// recorded (tile_cost, `waves` per tile).  One workgroup: a tile's cost is its slowest wave's
// (a workgroup holds its slots until then), binned into 16 levels of the largest cost; the bins
// are dispatched costliest first, and inside a bin the tiles keep the default (bottom-up) order,
// so tiles of similar cost stay spatially together (a fully cost-sorted order was 3.6 % slower on
// C2, whose tiles cost nearly the same).  Every key is read once and kept (`keys`), so the
// output is a permutation of the tiles even if another launch rewrites the costs meanwhile.
constexpr int kOrderBins = 16;
__global__ __launch_bounds__(1024) void packet_order_kernel(const uint32_t* cost, uint32_t gx,
                                                            uint32_t gy, uint32_t waves,
                                                            uint32_t* keys, uint32_t* order,
                                                            uint32_t* verdict) {
    __shared__ uint32_t s_max, s_cnt[kOrderBins];
    const uint32_t tid = threadIdx.x, tiles = gx * gy;
    if (tid == 0) s_max = 0;
    if (tid < kOrderBins) s_cnt[tid] = 0;
    __syncthreads();
    uint32_t m = 0;
    for (uint32_t i = tid; i < tiles; i += blockDim.x) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < waves; ++w) c = max(c, cost[i * waves + w]);
        keys[i] = c;
        m = max(m, c);
    }
    atomicMax(&s_max, m);
    __syncthreads();
    const uint64_t top = static_cast<uint64_t>(s_max) + 1;
    for (uint32_t i = tid; i < tiles; i += blockDim.x) {
        const uint64_t bin = static_cast<uint64_t>(keys[i]) * kOrderBins / top;  // < kOrderBins
        const uint32_t key = kOrderBins - 1 - static_cast<uint32_t>(bin);        // 0: costliest
        keys[i] = key;
        atomicAdd(&s_cnt[key], 1u);
    }
    __syncthreads();
    if (tid >= 64) return;
    // Narrow distributions keep the default order: when the median tile costs at least a
    // quarter of the costliest (C2: ~0.4), costliest-first was slower (C2 +3 %, MI355X); wide
    // ones (C3-C5: a few tiles at 10-35x the median) gain 4-10 %.
    uint32_t acc = 0;
    int median_bin = 0;  // cost bin (0 cheapest) holding the median tile
    for (int b = kOrderBins - 1; b >= 0; --b) {  // keys from cheapest (kOrderBins - 1) up
        acc += s_cnt[b];
        if (2 * acc >= tiles) {
            median_bin = kOrderBins - 1 - b;
            break;
        }
    }
    const bool narrow = median_bin >= kOrderBins / 4;
    // for the host (pinned memory): 1 = narrow, launches keep the default order without even
    // reading the table (its per-workgroup load cost C2 3 %); 2 = dispatch by the table
    if (tid == 0 && verdict) __hip_atomic_store(verdict, narrow ? 1u : 2u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_SYSTEM);
    // one wave scatters the tiles in default dispatch order (bottom-up rows), stably per bin:
    // lane b < kOrderBins holds bin b's cursor
    uint32_t cur = 0;
    for (int b = 0; b < kOrderBins; ++b)
        if (static_cast<int>(tid) > b) cur += s_cnt[b];
    if (narrow) {
        for (uint32_t lin = tid; lin < tiles; lin += 64) order[lin] = (gy - 1 - lin / gx) * gx + lin % gx;
        return;
    }
    const uint64_t below = (1ull << tid) - 1ull;
    for (uint32_t c0 = 0; c0 < tiles; c0 += 64) {
        const uint32_t lin = c0 + tid;
        const bool ok = lin < tiles;
        uint32_t tile = 0, key = kOrderBins;
        if (ok) {
            tile = (gy - 1 - lin / gx) * gx + lin % gx;
            key = keys[tile];
        }
        for (int b = 0; b < kOrderBins; ++b) {
            const uint64_t mk_ = __ballot(key == static_cast<uint32_t>(b));
            if (!mk_) continue;  // uniform
            const uint32_t base = __builtin_amdgcn_readlane(cur, b);
            if (key == static_cast<uint32_t>(b))
                order[base + __builtin_popcountll(mk_ & below)] = tile;
            if (static_cast<int>(tid) == b) cur += __builtin_popcountll(mk_);
        }
    }
}

hipError_t launch_packet_order(const uint32_t* cost, uint32_t gx, uint32_t gy, uint32_t waves,
                               uint32_t* keys, uint32_t* order, uint32_t* verdict,
                               hipStream_t stream) {
    hipLaunchKernelGGL(packet_order_kernel, dim3(1), dim3(1024), 0, stream, cost, gx, gy, waves,
                       keys, order, verdict);
    return hipGetLastError();
}

template <int MAXC>
static void launch_packet_maxc(const TraceParams& p, bool count, size_t lds, int feat,
                               hipStream_t stream) {
    // compiled feature sets: lean (the BASELINE C2-C4 shape), lean + plane culls (C3), lean +
    // area light (C5, rt_packet_area.hip), triangles / models only (no Blinn-Phong, area light
    // or Reinhard-Jodie), and everything
    if (feat == kFeatFix) launch_packet_variant<1, kFeatFix>(p, count, lds, stream);
    else if (feat == 0) launch_packet_variant<MAXC, 0>(p, count, lds, stream);
    else if (feat == kFeatPlanes) launch_packet_variant<MAXC, kFeatPlanes>(p, count, lds, stream);
    else if (feat == kFeatTris) launch_packet_variant<MAXC, kFeatTris>(p, count, lds, stream);
    else launch_packet_variant<MAXC, kFeatAll>(p, count, lds, stream);
}

static int packet_features(const TraceParams& p, bool any_specular) {
    int feat = 0;
    if (any_specular) feat |= kFeatSpec;
    if (p.al_samples > 0) feat |= kFeatArea;
    if (p.nt > 0) feat |= kFeatTris;
    if (p.ldr && p.tonemap == 4) feat |= kFeatJodie;
    // the plane cull has its own lean variant; combined with other features the general one
    if (p.np >= 3 && feat == 0) feat = kFeatPlanes;
    return feat;
}

// The variants that read a cone table (packet_direct_kernel's kTab): single sample, up to 64
// spheres, no feature — the marching one and its fix-up twin (C2's two).  The counting pass and
// a launch that records tile costs take the general variant, which forms its own masks.
bool packet_reads_cone_table(const TraceParams& p, bool any_specular) {
    return p.aa == 1 && !p.tile_cost && p.ns >= 1 && p.ns <= 64 && p.max_rec > 0 &&
           packet_features(p, any_specular) == 0;
}

int packet_shadow_table_lights(const TraceParams& p) {
    // (np <= 2 is what the variants that read a table render: packet_features)
    return p.np <= 2 ? shadow_table_lights(p.ns, p.np, p.nl, p.al_samples > 0) : 0;
}

// The fix-up variant serves the single-sample, ≤ 64-sphere, no-feature launches (C2) of frame
// batches that neither count rays nor record tile costs, when the launch is large enough to pay
// for its fix-up launch: that launch costs ~25 µs whatever it holds (one wave's serial generic
// pixel), the march-free packet kernel saves ~1 ns per pixel (C2: 37.8 → 35.7 µs per 1080p
// frame), so the break-even is ~25 M pixels per launch — kPkFixMinPixels (≈ 15 1080p frames)
// leaves a margin: a 32-frame batch takes it, an 8-frame one or one rank's rows of a 4- or
// 8-rank split keep the marching variant (profiles/r05_ab_fixup.txt).  RTAMD_PK_FIX=0: the
// marching variant everywhere, =1: the fix-up variant for every eligible batch (tests, A/B).
constexpr uint64_t kPkFixMinPixels = 32ull << 20;
bool packet_uses_fixup(const TraceParams& p, bool count, bool any_specular) {
    const int mode = packet_switch("RTAMD_PK_FIX");
    if (mode == 0) return false;
    const bool eligible = !count && p.aa == 1 && !p.tile_cost && p.nframes >= 1 &&
                          (p.ns + 63) / 64 <= 1 && packet_features(p, any_specular) == 0;
    const uint64_t px = static_cast<uint64_t>(p.nframes) * p.rows * p.width;
    return eligible && (mode == 1 || px >= kPkFixMinPixels);
}

// The uniform tiles of the fix-up variant's split launch (PkSplit; the general workgroups take
// packet_direct_kernel<1, kFeatFix | kFeatSplit, false, false, WGY>), one wave per entry of the frame's list of uniform
// tiles: the entry is the tile's class word with the tile's column and row (rt_shadow_table.hpp),
// one scalar load.  The wave forms packet_direct_kernel's kLean camera ray for its lane's pixel
// (clamped into the image as there), calls pk_uniform_tile and ends in the shared epilogue (rt_packet_epilogue.hpp): the calls the
// general kernel's uniform branch makes, with the same arguments, so the bits are its bits.  No
// LDS, no barrier, no table pointer beyond the frame's class words.  Grid: (waves of the largest
// list over kUniWaves, 1, frames); waves past the frame's count return at once.
#ifndef RT_PACKET_UNI_THREADS
#define RT_PACKET_UNI_THREADS 256
#endif
#ifndef RT_PACKET_UNI_WAVES
#define RT_PACKET_UNI_WAVES 8
#endif
// SPH = true: the same kernel over the frame's list of shadowed-plane tiles (tile_shadowed_mark,
// rt_shadow_table.hpp; entries of the same format, TileTabLayout::Lists), which also hands
// pk_uniform_tile the tile's shadow words — P.fr_stab of the frame at the tile the entry's column
// and row name, nl words — for the sphere block of the shadow classification.
constexpr int kUniThreads = RT_PACKET_UNI_THREADS;
template <bool SPH>
__global__ __launch_bounds__(kUniThreads, RT_PACKET_UNI_WAVES) void packet_uniform_kernel(TraceParams P, uint32_t tiles) {
    constexpr int FEAT = kFeatFix;
    const PkFrame& F = P.fr[blockIdx.z];  // (split launches are frame batches: P.nframes >= 1)
    // (one wave row per workgroup, packet_split_wanted: tiles / kWgWavesX workgroups)
    const pk_culp ctab = (pk_culp)P.fr_ctab[blockIdx.z];
    const TileTabLayout::Lists L{tiles, tiles / kWgWavesX};
    const pk_culp hdr = ctab + L.after_cls();
    const uint32_t i = blockIdx.x * (kUniThreads / 64) +
                       __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(threadIdx.x) >> 6);
    const TileListCounts n = tile_list_counts(SPH ? 0ull : hdr[L.counts()],
                                              SPH ? hdr[L.shadowed_count()] : 0ull);
    if (i >= (SPH ? n.shadowed : n.uniform)) return;
    const unsigned long long e = hdr[SPH ? L.shadowed(i) : L.uniform(i)];
    const unsigned long long cls = e & kListWordMask;
    const uint32_t col = static_cast<uint32_t>(e >> kListColShift) & kListCoordMask;
    const uint32_t row = static_cast<uint32_t>(e >> kListRowShift) & kListCoordMask;
    const d3 cam = mk(F.cam[0], F.cam[1], F.cam[2]);
    const double cam_dz = P.fr_dz[blockIdx.z][0], cam_dz2 = P.fr_dz[blockIdx.z][1];
    const uint64_t frame_off = static_cast<uint64_t>(blockIdx.z) * P.frame_px;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t x = col * kPkW + (lane % kPkW), yl = row * kPkH + (lane / kPkW);
    // lanes past the image edge trace a clamped in-image ray and write nothing
    const uint32_t xc = x < P.width ? x : P.width - 1;
    const uint32_t y = image_row(P, yl < P.rows ? yl : P.rows - 1);
    const double sx = static_cast<double>(xc) - P.half_w;
    const double sy = P.half_h - static_cast<double>(y);
    const d3 dv = mk(sx - cam.x, sy - cam.y, cam_dz);
    const d3 d = unit_sq(dv, dv.x * dv.x + dv.y * dv.y + cam_dz2);
    bool fix = false;
    PacketScene S;  // (not read: the records come through the scalar cache)
    S.lt = nullptr;
    d3 col3;
    if constexpr (SPH) {
        // the tile's index in the frame's tables: row · (tile columns) + column
        const uint32_t cols = (P.width + kPkW * kWgWavesX - 1) / (kPkW * kWgWavesX) * kWgWavesX;
        const unsigned long long* stab =
            P.fr_stab[blockIdx.z] + static_cast<size_t>(row * cols + col) * P.nl;
        col3 = pk_uniform_tile<1, FEAT, true>(S, P, F.img, cls, cam, d, P.ns, P.np, P.nl, P.bias,
                                              fix, stab);
    } else {
        col3 = pk_uniform_tile<1, FEAT>(S, P, F.img, cls, cam, d, P.ns, P.np, P.nl, P.bias, fix);
    }
    const d3 acc = mk(0.0, 0.0, 0.0) + col3;  // the sample loop's one addition
    constexpr int samples = 1;
    const uint32_t lane_e = lane, x_e = x, yl_e = yl;
#include "rt_packet_epilogue.hpp"
}

// RTAMD_PK_TILE_SPLIT=0 (read per launch): the fix-up variant's single launch, no lists formed
// (a table formed that way is one of its own).
bool packet_split_wanted(const TraceParams& p) {
    if (packet_switch_off("RTAMD_PK_TILE_SPLIT")) return false;
    uint32_t gx, gy, waves;
    packet_grid(p, gx, gy, waves);
    // (one wave row per workgroup: a scene with class words has at most 63 spheres, an image far
    // below the size at which workgroups take two rows)
    return !p.tile_order && waves == kWgWavesX && gx * kWgWavesX <= kListMaxCoord &&
           gy <= kListMaxCoord;
}

// The fix-up variant's split launch (s.tiles: every frame's class words are followed by
// its tile lists): packet_uniform_kernel over the uniform tiles and packet_direct_kernel's
// kFeatSplit twin over the general workgroups, one after the other on the stream, with
// packet_uniform_kernel<true> over the shadowed-plane tiles between them where the tables list
// those (s.sh_n).  They touch disjoint pixels and append to one fix-up list with atomics.  (The
// uniform launch forked onto a second stream measured the same: profiles/tile_split_ab.txt.)
static void launch_packet_split(const TraceParams& p, const PkSplit& s, size_t lds,
                                hipStream_t stream) {
    // (one wave row per workgroup: packet_split_wanted)
    const dim3 block(64 * kWgWavesX);
    const dim3 ggrid(s.gen_n, 1u, p.nframes);
    const dim3 ugrid((s.uni_n + kUniThreads / 64 - 1) / (kUniThreads / 64), 1u, p.nframes);
    const dim3 sgrid((s.sh_n + kUniThreads / 64 - 1) / (kUniThreads / 64), 1u, p.nframes);
    // (RT_PACKET_SPLIT_GENERAL_FIRST: the other order, for A/B builds)
#ifdef RT_PACKET_SPLIT_GENERAL_FIRST
    if (s.gen_n)
        hipLaunchKernelGGL((packet_direct_kernel<1, kFeatFix | kFeatSplit, false, false, 1>),
                           ggrid, block, lds, stream, p);
#endif
    if (s.uni_n)
        hipLaunchKernelGGL(packet_uniform_kernel<false>, ugrid, dim3(kUniThreads), 0, stream, p,
                           s.tiles);
    // (a table without the third list has a count of 0 for it: no launch)
    if (s.sh_n)
        hipLaunchKernelGGL(packet_uniform_kernel<true>, sgrid, dim3(kUniThreads), 0, stream, p,
                           s.tiles);
#ifndef RT_PACKET_SPLIT_GENERAL_FIRST
    if (s.gen_n)
        hipLaunchKernelGGL((packet_direct_kernel<1, kFeatFix | kFeatSplit, false, false, 1>),
                           ggrid, block, lds, stream, p);
#endif
}

hipError_t launch_packet_direct(const TraceParams& p, bool count, bool any_specular,
                                hipStream_t stream, const PkSplit* split) {
    const size_t lds = packet_lds_bytes(p.ns, p.np, p.nl);
    const int chunks = (p.ns + 63) / 64;
    int feat = packet_features(p, any_specular);
    if (packet_uses_fixup(p, count, any_specular)) {
        if (!p.fix_list || !p.fix_ctl || !p.fix_next) return hipErrorInvalidValue;
        feat = kFeatFix;
        // (the host sets split->tiles only for a frame batch whose frames all have lists, which
        // packet_split_wanted allowed: no tile order, one wave row per workgroup)
        if (split && split->tiles) {
            launch_packet_split(p, *split, lds, stream);
            return hipGetLastError();
        }
    }
    // the area-light variants live in rt_packet_area.hip (compiled with the default scheduler)
    if (feat == kFeatArea) return launch_packet_area(p, count, lds, chunks, stream);
    if (chunks <= 1) launch_packet_maxc<1>(p, count, lds, feat, stream);
    else if (chunks <= 4) launch_packet_maxc<4>(p, count, lds, feat, stream);
    else launch_packet_maxc<16>(p, count, lds, feat, stream);
    return hipGetLastError();
}
#endif  // RT_PACKET_PROBE

}  // namespace rtamd
