// rt_packet_device.hpp — the packet machinery shared by the shaded packet kernel
// (rt_packet_kernel.hpp) and the G-buffer kernel (rt_gbuffer.hip): the tunables, the LDS image
// of a scene seen from one camera, the packet culls and the closest-hit search.
//
// The packet-culled FP64 trace kernel serves scenes whose materials spawn no secondary rays
// (every BASELINE synthetic config C2–C5): camera ray + shadow rays per pixel.
//
// Same per-ray arithmetic as the generic kernel (rt_trace_common.hpp), so results stay
// bit-identical to the reference; what changes is WHICH primitives a ray is tested against
// and which divisions are skipped because their outcome is already decided:
//
//  * One wave = an 8×8 pixel tile.  Before each closest-hit search the wave bounds its rays —
//    a direction cone around the camera for camera rays, a capsule from the ball of shadow-ray
//    origins to the light for shadow rays — and each lane tests one sphere against that bound
//    (ballot → a 64-bit candidate mask per 64 spheres, held in SGPRs).  The bounds are reduced
//    across the wave in FP32 with directed rounding (DPP row steps + readlane), so they only
//    ever grow.
//  * The per-sphere test is conservative with a 1e-4 relative radius margin: a sphere outside
//    the bound has, for every ray of the packet, an exact discriminant < 0 by far more than
//    FP64 rounding can flip, so it can never be hit.  Spheres whose |oc|/r exceeds 1e5 (where
//    that argument would need a larger margin) are always kept.  Candidates are visited in
//    ascending index order, so strict-'<' tie-breaking (Shape.h:36) is unchanged.
//  * Camera rays share their origin: oc = cam − C, c = oc·oc − r² (Shape.h:73-77) and each
//    plane's (p − cam)·n (Shape.h:152-153) are the same doubles for every camera ray and are
//    formed once per workgroup into LDS.
//  * A candidate's root (or plane t) is only divided out when it can still win: if
//    numerator > best·denominator·(1+2⁻⁴⁰) the rounded quotient is provably ≥ best and the
//    strict '<' would reject it anyway.  The far root is only formed when the near root is
//    below the 1e-6 epsilon (t0 ≤ t1 holds exactly for 2a > 0, so the reference's swap never
//    fires).
//  * Shadow-ray marches (computeTransmittance, Scene.h:35-77) only move the origin along the
//    segment towards the light, so one capsule mask serves the whole march.
#pragma once

#include <cstdlib>

#include "rt_trace_common.hpp"

#pragma clang fp contract(off)

namespace rtamd {

constexpr int kPkW = 8;             // pixels per wave, x
constexpr int kPkH = 8;             // pixels per wave, y
#ifndef RT_PK_WAVES_X
#define RT_PK_WAVES_X 2
#endif
constexpr int kWgWavesX = RT_PK_WAVES_X;  // waves per workgroup, x
// Waves per workgroup in y (the WGY template parameter): 1 (128 threads, 16×8 px) while ten
// workgroups' LDS images fit the CU's 160 KiB — 20 waves, the 5-waves/SIMD budget — else 2
// (256 threads, 16×16 px: five images, still 20 waves).  Smaller workgroups wait less for their
// slowest wave (C3 -3 %, C5 -2 %); with C4's 27 KiB image they would halve the occupancy.
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr unsigned pk_wgy(size_t lds) { return 10 * lds <= kLdsPerCu ? 1u : 2u; }
constexpr double kCullRel = 1e-4;   // relative inflation of every culling radius
constexpr double kFarRatio = 1e5;   // |oc|/r beyond which a sphere is never culled
constexpr double kNoWin = 1.0 + 0x1.0p-40;  // "quotient provably >= best" factor
// Point-light shadow packets with more candidate spheres than this are split in two (pk_light);
// variants with more than 64 spheres only (MAXC > 1).
#ifndef RT_SHADOW_SPLIT
#define RT_SHADOW_SPLIT 1
#endif
#ifndef RT_SHADOW_SPLIT_MIN
#define RT_SHADOW_SPLIT_MIN 16
#endif
constexpr bool kShadowSplit = RT_SHADOW_SPLIT != 0;
constexpr int kShadowSplitMin = RT_SHADOW_SPLIT_MIN;

// Feature bits of a kernel variant: code for a feature the scene does not use is not compiled
// in, which is what keeps the FP64 register budget (and so the occupancy) down.
constexpr int kFeatSpec = 1;    // some opaque material has specular > 0: Blinn-Phong pow
constexpr int kFeatArea = 2;    // build-defined area light
constexpr int kFeatTris = 4;    // triangles / models
constexpr int kFeatJodie = 8;   // Reinhard-Jodie fused tonemap (log/pow)
constexpr int kFeatPlanes = 16; // ≥ 3 planes: shadow packets also cull planes (cull_capsule)
constexpr int kFeatAll = 31;
// with kFeatArea only: no planes and no point lights (C5: spheres lit by the area light), so the
// plane and point-light code compiles away; the single-sample instantiation then runs at 6
// waves/SIMD (80 VGPRs): C5 508 -> 490 us at 5 waves, -> 482 us at 6 (MI355X)
constexpr int kFeatNoPL = 32;
// Fix-up variant (with no other feature; single sample, ≤ 64 spheres: C2): a lane whose shadow
// ray the classifier leaves undecided does not march (computeTransmittance's exact loop is not
// compiled in, which takes the variant from 80 VGPRs + 44 B/lane of spills at 6 waves/SIMD to 64
// VGPRs + 12 B at 8); its pixel is queued instead and packet_fixup_kernel renders it with the
// exact per-pixel path after the launch (0.08 % of C2's shadow rays are undecided).
constexpr int kFeatFix = 128;
#ifndef RT_PACKET_FIX_WAVES
#define RT_PACKET_FIX_WAVES 8
#endif
// kFeatFix | kFeatSplit: the fix-up variant over a frame's list of general workgroups, without
// its uniform path (packet_direct_kernel, rt_packet_kernel.hpp); its waves per SIMD
constexpr int kFeatSplit = 256;
#ifndef RT_PACKET_GENERAL_WAVES
#define RT_PACKET_GENERAL_WAVES RT_PACKET_FIX_WAVES
#endif

// Waves per SIMD of the single-sample variant for <= 64 spheres, point lights and no other
// feature (C2): 6 with its light records read through the scalar cache (80 VGPRs, 48 B/lane of
// scratch): C2 48.1 -> 46.7 us against 5 waves (95 VGPRs + 20 B, lights from LDS), MI355X
constexpr int kPkStack = 64;       // wave-coherent BVH walk: node stack entries per wave (depth ≤ 48)
#ifndef RT_PACKET_SMALL_WAVES
#define RT_PACKET_SMALL_WAVES 6
#endif
// Waves per SIMD of the single-sample area-only variant (C5: spheres lit by the area light)
#ifndef RT_PACKET_AREA_WAVES
#define RT_PACKET_AREA_WAVES 6
#endif
// Waves per SIMD the lean variants are compiled for (4 = at most 128 VGPRs).
#ifndef RT_PACKET_LEAN_WAVES
#define RT_PACKET_LEAN_WAVES 4
#endif
// ... the triangle-only variants (BVH traversal; models without specular materials)
#ifndef RT_PACKET_TRIS_WAVES
#define RT_PACKET_TRIS_WAVES 4
#endif
// ... and the single-sample variants without Blinn-Phong / triangles (5 = at most 96 VGPRs)
#ifndef RT_PACKET_AA1_WAVES
#define RT_PACKET_AA1_WAVES 5
#endif

// This lane's index in the wave, formed where it is used: an opaque (volatile) mbcnt pair the
// compiler cannot hoist and keep live — it spilled the hoisted lane·80 LDS offset of the culls
// in the C2 variant.  C2 46.9 → 46.5 µs per launch, interleaved 3 rounds
// against threadIdx.x & 63 (profiles/r04_ab_c2_march_save_opaque_lane.txt).
__device__ __forceinline__ int cull_lane() {
    int l;
    __asm__ volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// (wave reductions, lane broadcasts: rt_trace_common.hpp)

// A sphere of the packet image (LDS): kPkSph doubles — cx cy cz r², the camera-cone terms as 8
// floats (cone_terms: vx vy vz q | rr dv slack r, r = the culling radius rounded up), the
// camera-ray constant c = oc·oc − r² with oc = cam − C (Shape.h:73,77; the candidates form oc
// again, the same three subtractions), 8 B of padding.  The lane-parallel culls read record `lane` with ds_read_b128: at an 80-B stride the
// 16 lanes of every ds_read_b128 lane group start on distinct 16-B slots of the 256-B bank row
// (20·lane mod 64 distinct), where the former 32-B records (plus a separate radius array) gave
// 2- and 4-way bank conflicts (C3: 1.84 conflict cycles per LDS cycle).
constexpr int kPkSph = 10;

struct PacketScene {
    const double* sph;   // LDS: sphere records (kPkSph doubles, above)
    const double* pl;    // LDS: planes (px py pz nx ny nz (p−cam)·n −)
    const double* lt;    // LDS: point lights
    const double* tri;   // HBM
    const double* mat;   // HBM: material table [spheres | planes | triangles]
    const double* bvh;   // HBM: triangle BVH, or null
    const int32_t* bvh_tri;
    // scenes with >= kSphChunkMin spheres: spheres are in spatial-chunk order (sph, rad, cone,
    // pre), chunk c's bounding sphere is pseudo-sphere ns + c of sph / rad / cone (nb of them),
    // and orig[i] is sorted sphere i's index in the scene (material table, closest-hit ties)
    const int32_t* orig;
    int ns, np, nt, nl, nb;
    int* wstk;  // LDS: this wave's node stack of the wave-coherent BVH walk (kFeatTris variants)
};

// Closest hit of the packet kernel: t and the primitive's index in the material table order
// [spheres | planes | triangles] (one register instead of a kind and a per-kind index).
struct PkHit {
    double t;
    int prim;
};

// Candidate masks: MAXC chunks of 64 spheres.  m[c] is wave-uniform (a ballot result).
template <int MAXC>
struct Masks {
    uint64_t m[MAXC];
    uint64_t pm;  // shadow packets: planes 0..63 that may block (bit set), the rest are clear
};

template <int MAXC>
__device__ __forceinline__ Masks<MAXC> all_candidates(int ns) {
    Masks<MAXC> M;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int left = ns - 64 * c;
        M.m[c] = left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
    }
    M.pm = ~0ull;
    return M;
}

// ------------------------------------------------------------------ packet culling (FP32)
// The culls only decide which spheres a packet may skip, so they run in FP32 (half the FP64
// issue cost, cheap sqrt) with every rounding error covered by explicit slack: each test keeps a
// sphere unless the FP32 value clears the exact bound by more than kF32Slack times the
// magnitudes involved (≥ 5× the worst-case FP32 error of the expression, derived per test
// below).  Differences of scene coordinates are taken in FP64 first, so large coordinates do not
// cost relative precision; NaN/inf anywhere keeps the sphere (every comparison is negated).
constexpr float kF32Slack = 2e-5f;
constexpr float kF32Up = 1.0f + 1e-6f;  // rounds a positive FP32 conversion up

__device__ __forceinline__ float f32_up(double v) { return static_cast<float>(v) * kF32Up; }
__device__ __forceinline__ float dot3f(float ax, float ay, float az, float bx, float by, float bz) {
    return ax * bx + ay * by + az * bz;
}
// v_sqrt_f32 without the compiler's correct-rounding fix-up (≤ 1 ulp, 1.2e-7 relative): every
// FP32 square root of the culls and classifications carries a margin of ≥ 5e-7 for it.
__device__ __forceinline__ float sqrt_f32(float x) { return __builtin_amdgcn_sqrtf(x); }

// Camera-ray packet: origin `o` shared, directions within the cone (axis, cos_min), cos_min > 0.
// Sphere (C, r) is kept iff angle(C−o, axis) ≤ θ + β, sin β = r'/|C−o| (r' = inflated r),
// evaluated without divisions as  (C−o)·axis ≥ cosθ·√(|C−o|²−r'²) − sinθ·r'.
// Error bound (d = |C−o|): |C−o|² and the dot product carry < 5e-7·d² and 3e-7·d; spheres with
// d ≤ 1.01·r' are kept outright, so |C−o|²−r'² ≥ 0.0199·r'² and its square root is off by at
// most 2.5e-6·d; total < 3e-6·d against a slack of 2e-5·d.
// The cone test's per-sphere terms depend on the camera only (every camera ray starts there),
// so each workgroup forms them once into LDS (8 floats per sphere: vx vy vz q | rr dv slack r),
// with q = NaN for spheres that are always kept; the same FP32 expressions, so the same masks.
__device__ __forceinline__ void cone_terms(const double* s, double radius, d3 o, float* out) {
    const float r = f32_up(radius);
    const float vx = static_cast<float>(s[0] - o.x), vy = static_cast<float>(s[1] - o.y),
                vz = static_cast<float>(s[2] - o.z);
    const float dv2 = dot3f(vx, vy, vz, vx, vy, vz);
    const float rr = r * (1.0f + static_cast<float>(kCullRel));
    const float dv = sqrt_f32(dv2);
    const bool always = !(dv > 1.01f * rr) || !(dv <= static_cast<float>(kFarRatio) * r);
    out[0] = vx;
    out[1] = vy;
    out[2] = vz;
    out[3] = always ? __builtin_nanf("") : sqrt_f32(dv2 - rr * rr);  // |C−o|·cos β
    out[4] = rr;
    out[5] = dv;
    out[6] = kF32Slack * dv;
    out[7] = r;  // the capsule test's radius
}

template <int MAXC>
__device__ __forceinline__ Masks<MAXC> cull_cone(const PacketScene& S, d3 axis, double cos_min) {
    Masks<MAXC> M;
    const int lane = cull_lane();
    const float cs = static_cast<float>(cos_min) * (1.0f - 1e-6f);  // rounded down (cs > 0)
    const float sn = sqrt_f32(fmaxf(0.0f, 1.0f - cs * cs)) * (1.0f + 1e-5f);  // rounded up
    const float ax = static_cast<float>(axis.x), ay = static_cast<float>(axis.y),
                az = static_cast<float>(axis.z);
    auto test = [&](int k) {
        const float4* c4 = reinterpret_cast<const float4*>(S.sph + kPkSph * k + 4);
        const float4 a = c4[0];
        const float4 b = c4[1];
        const float q = a.w, rr = b.x, dv = b.y, slack = b.z;
        // θ + β ≥ π, or the axis is outside the cone around C−o (NaN q: always kept)
        return !(q > -cs * dv + slack) ||
               !(dot3f(a.x, a.y, a.z, ax, ay, az) < cs * q - sn * rr - slack);
    };
    uint64_t live = ~0ull;  // chunks whose bounding sphere the cone may meet
    if constexpr (MAXC > 1)
        if (S.nb > 0) live = __ballot(lane < S.nb && test(S.ns + lane));
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        M.m[c] = 0ull;
        if (!((live >> c) & 1ull)) continue;  // uniform: no sphere of the chunk is in the cone
        const int k = c * 64 + lane;
        M.m[c] = __ballot(k < S.ns && test(k));
    }
    M.pm = ~0ull;
    return M;
}

// Shadow packet: origins inside ball (c, R), every ray aims at a light inside ball (L, RL).
// The segments [so, lpos] lie in the capsule of radius max(R, RL) around [c, L]; the traced
// rays do not quite follow them: directLightning takes the direction from the hit point P
// (L = (lpos − P)/dist) but starts the ray at so = P + n·bias, so the point at parameter t is
// so + (t/dist)·(lpos − so) + (t/dist)·n·bias, within bias·|n| of its segment for every
// t ≤ maxDist = dist − bias.  The capsule radius carries that bias (a sphere grazed by the
// ray but not by the segment is kept).  The squared distance
// from C to the segment carries < 1.5e-6·(|C−c|² + |L−c|²) of FP32 error (any of the three
// branches, including a branch chosen wrongly next to a boundary where they meet
// continuously), against a slack of 2e-5·(|C−c|² + |L−c|²).  The middle branch multiplies by
// v_rcp_f32(|L−c|²) (1 ulp: relative error ≤ 2^-23) instead of dividing (a full IEEE FP32
// division is 12 VALU in the per-lane branch): that adds ≤ 1.2e-7·(v·s)²/|s|² ≤ 1.2e-7·|C−c|²
// to the subtracted term, so the bound is < 1.7e-6·(|C−c|² + |L−c|²), still 12× inside the
// slack.  v_rcp_f32 flushes denormals: a denormal |s|² gives inf and an inf or NaN distance,
// which keeps the sphere; |s|² > 2^120, whose reciprocal would underflow to 0 and lose the
// subtracted term, culls nothing (`huge`).
template <int MAXC, int FEAT>
__device__ __forceinline__ Masks<MAXC> cull_capsule(const PacketScene& S, d3 c, float R, d3 L,
                                                    double RL, double bias) {
    Masks<MAXC> M;
    const int lane = cull_lane();
    const float sx = static_cast<float>(L.x - c.x), sy = static_cast<float>(L.y - c.y),
                sz = static_cast<float>(L.z - c.z);
    const float sl2 = dot3f(sx, sy, sz, sx, sy, sz);
    const float inv_sl2 = __builtin_amdgcn_rcpf(sl2);  // wave-uniform; only read when sl2 > 0
    const bool huge = !(sl2 <= 0x1p120f);              // (or NaN) no usable reciprocal: keep all
    const float Rc = fmaxf(R, f32_up(RL)) + f32_up(fabs(bias)) * 1.001f;  // |n| ≤ 1 + 2ε
    auto test = [&](int k) {
        const double2* s2 = reinterpret_cast<const double2*>(S.sph + kPkSph * k);
        const double2 sxy = s2[0], szr = s2[1];  // cx cy | cz r² (two ds_read_b128)
        const float r = reinterpret_cast<const float4*>(s2 + 2)[1].w;  // f32_up(radius)
        const float vx = static_cast<float>(sxy.x - c.x), vy = static_cast<float>(sxy.y - c.y),
                    vz = static_cast<float>(szr.x - c.z);
        const float vs = dot3f(vx, vy, vz, sx, sy, sz);
        const float vv = dot3f(vx, vy, vz, vx, vy, vz);
        float d2;
        if (!(vs > 0.0f) || !(sl2 > 0.0f)) {
            d2 = vv;
        } else if (!(vs < sl2)) {
            const float wx = vx - sx, wy = vy - sy, wz = vz - sz;
            d2 = dot3f(wx, wy, wz, wx, wy, wz);
        } else {
            d2 = vv - (vs * vs) * inv_sl2;  // a rounding and the reciprocal's ulp: ≪ slack
        }
        const float lim = (r + Rc) * (1.0f + static_cast<float>(kCullRel));
        const float far = static_cast<float>(kFarRatio) * r - Rc;
        return !(d2 > lim * lim + kF32Slack * (vv + sl2)) || !(far > 0.0f) ||
               !(vv <= far * far) || huge;
    };
    uint64_t live = ~0ull;  // chunks whose bounding sphere the capsule may meet
    if constexpr (MAXC > 1)
        if (S.nb > 0) live = __ballot(lane < S.nb && test(S.ns + lane));
#pragma unroll
    for (int ch = 0; ch < MAXC; ++ch) {
        M.m[ch] = 0ull;
        if (!((live >> ch) & 1ull)) continue;  // uniform: the capsule misses the whole chunk
        const int k = ch * 64 + lane;
        M.m[ch] = __ballot(k < S.ns && test(k));
    }
    // Planes (feature kFeatPlanes, scenes with three or more, where one lane-parallel test costs
    // less than the per-lane plane tests it saves): a plane with the capsule strictly on one
    // side — the origin ball and the light ball on the same side by their radii, the rays' bias
    // offset and 1e-8 of the magnitudes (FP64 rounding, and pk_occlusion's 1e-9 relative
    // "beyond the light" margin) — meets no ray of the packet within [0, maxDist], so
    // pk_occlusion would classify it clear for every lane.  |n|₁ bounds |n|₂.  The exact march
    // (pk_transmittance) still tests every plane.
    M.pm = ~0ull;
    if constexpr ((FEAT & kFeatPlanes) != 0) {
        if (S.np <= 64) {
            bool keep = true;
            if (lane < S.np) {
                const double* q = S.pl + kPlStride * lane;
                const d3 pn = mk(q[3], q[4], q[5]);
                const d3 p0 = mk(q[0], q[1], q[2]);
                const d3 vc = c - p0, vl = L - p0;
                const double nn = fabs(pn.x) + fabs(pn.y) + fabs(pn.z);
                const double sc = dot(vc, pn), sl = dot(vl, pn);
                const double mag = (fabs(vc.x) + fabs(vc.y) + fabs(vc.z) + fabs(vl.x) +
                                    fabs(vl.y) + fabs(vl.z) + static_cast<double>(R) + RL) * nn;
                const double off = fabs(bias) * 1.01 * nn + 1e-8 * mag;
                const double mc = static_cast<double>(R) * 1.001 * nn + off;
                const double ml = RL * 1.001 * nn + off;
                keep = !((sc > mc && sl > ml) || (sc < -mc && sl < -ml));
            }
            M.pm = __ballot(keep);
        }
    }
    return M;
}

// The running closest hit takes candidate i at t when the reference's in-order loop with strict
// '<' (Shape.h:36) would end on it: t < best, or — when the spheres are in spatial-chunk order
// (ORD, orig[] = scene indices) — t == best with a lower scene index.
template <bool ORD>
__device__ __forceinline__ void take_closest(double t, int i, const int32_t* orig, bool& found,
                                             double& best, int& prim) {
    bool take = !found || t < best;
    if constexpr (ORD) take = take || (t == best && orig[i] < orig[prim]);
    if (take) {
        found = true;
        best = t;
        prim = i;
    }
}

// Root selection of Sphere::Intersect (Shape.h:84-97) folded into the running closest.
// Requires two_a > 0 (then t0 ≤ t1 exactly); divisions are skipped when the candidate
// provably cannot be strictly closer than `best`.
template <bool ORD>
__device__ __forceinline__ void sphere_roots(double b, double disc, double two_a, int i,
                                             const int32_t* orig, bool& found, double& best,
                                             int& prim) {
    if (disc < 0.0) return;
    const double sq = sqrt(disc);
    const double n0 = -b - sq;
    if (found && n0 > (best * two_a) * kNoWin) return;  // t1 >= t0 > best (strictly)
    double t = n0 / two_a;
    if (t < 1e-6) {
        t = (-b + sq) / two_a;
        if (t < 1e-6) return;
    }
    take_closest<ORD>(t, i, orig, found, best, prim);
}

// sphere_roots through the sqrt/division cores (rt_device.hpp), r2a = rcp_refined(two_a) with
// two_a in [2^-100, 2^100].  A finite disc ≥ 2^-767 keeps b, √disc and both numerators finite;
// a numerator |n| ≥ 2^-900 divides exactly, and a smaller one gives |t| < 2^-790 both exactly
// and through the core, so the 1e-6 test (the only use of such a root) decides alike.  Other
// discriminants take the literal path.  t0 ≤ t1 as in sphere_roots.
template <bool ORD>
__device__ __forceinline__ void sphere_roots_core(double b, double disc, double two_a, double r2a,
                                                  int i, const int32_t* orig, bool& found,
                                                  double& best, int& prim) {
    if (disc < 0.0) return;
    double t;
    if (disc >= 0x1p-767 && disc <= 0x1.fffffffffffffp+1023) {
        const double sq = sqrt_core(disc);
        t = div_core(-b - sq, two_a, r2a);
        if (t < 1e-6) {
            t = div_core(-b + sq, two_a, r2a);
            if (t < 1e-6) return;
        }
    } else {
        const double sq = sqrt(disc);
        t = (-b - sq) / two_a;
        if (t < 1e-6) {
            t = (-b + sq) / two_a;
            if (t < 1e-6) return;
        }
    }
    take_closest<ORD>(t, i, orig, found, best, prim);
}

// The reference's literal root selection, for degenerate directions (2a not > 0).
template <bool ORD>
__device__ __forceinline__ void sphere_roots_literal(double b, double disc, double two_a, int i,
                                                     const int32_t* orig, bool& found,
                                                     double& best, int& prim) {
    if (disc < 0.0) return;
    const double sq = sqrt(disc);
    double t0 = (-b - sq) / two_a;
    double t1 = (-b + sq) / two_a;
    if (t0 > t1) {
        const double tmp = t0;
        t0 = t1;
        t1 = tmp;
    }
    double t = t0;
    if (t < 1e-6) {
        t = t1;
        if (t < 1e-6) return;
    }
    take_closest<ORD>(t, i, orig, found, best, prim);
}

// Plane::Intersect (Shape.h:149-159) given num = (p − o)·n and denom = n·d.
__device__ __forceinline__ void plane_t(double num, double denom, int p, bool& found,
                                        double& best, int& prim) {
    if (!(fabs(denom) > 1e-6)) return;
    if (found && best >= 0x1p-900) {  // skip the division when t = num/denom is provably >= best
        const double lim = (best * denom) * kNoWin;  // (a normal product: |denom| > 1e-6)
        if (denom > 0.0 ? num > lim : num < lim) return;
    }
    const double t = num / denom;
    if (t >= 0.0 && (!found || t < best)) {
        found = true;
        best = t;
        prim = p;
    }
}

// plane_t through the division core for a camera-ray plane whose numerator passed the
// prologue's test (2^-900 ≤ |num| ≤ 2^400, |n|₁ ≤ 2^90): with 1e-6 < |denom| ≤ 2^91 every
// operand is inside div_core's range, so t has the bits of num / denom.
__device__ __forceinline__ void plane_t_core(double num, double denom, int p, bool& found,
                                             double& best, int& prim) {
    if (!(fabs(denom) > 1e-6)) return;
    // opposite signs: t = num/denom is negative and nonzero (|num| ≥ 2^-900), so the
    // reference's t >= 0 rejects it — a whole wave looking away from the plane skips the division
    if ((num < 0.0) != (denom < 0.0)) return;
    const double t = div_core(num, denom, rcp_refined(denom));
    if (t >= 0.0 && (!found || t < best)) {
        found = true;
        best = t;
        prim = p;
    }
}

// The triangles' part of IntersectClosest over the BVH, walked once per WAVE (the packet
// kernel's rays of an 8x8 tile, or the lanes of a shadow march, go through the same nodes):
// the node stack is wave-uniform in LDS, node boxes, leaf triangle ids and triangle records
// are read through the scalar cache (wave-uniform addresses: SGPRs, no per-lane loads), and
// each lane tests the popped node's box against its own current best (the per-lane walk's
// test, bvh_triangles in rt_trace_common.hpp, with the same 1e-9 margin), so a lane only tests
// the triangles of leaves its ray reaches and is not closer than.  A lane may see nodes its
// own walk would not visit (another lane hit them); every triangle it tests in a leaf is a real
// intersection test, so it still returns exactly the (t, index) minimum among the triangles
// the reference tests (the leaf of the winning triangle is always entered: every ancestor box
// contains the hit, and no box whose entry exceeds the winner's t is needed).  Children are
// pushed nearer-first along the node's split axis by the lanes' majority direction.
typedef const __attribute__((address_space(4))) int32_t* pk_cip;
typedef const __attribute__((address_space(4))) double* pk_cdp;
typedef const __attribute__((address_space(4))) unsigned long long* pk_culp;
__device__ __forceinline__ void bvh_wave(const PacketScene& S, d3 o, d3 d, bool& found,
                                         double& best, int& kind, int& idx) {
    const d3 inv = mk(d.x != 0.0 ? 1.0 / d.x : 0.0, d.y != 0.0 ? 1.0 / d.y : 0.0,
                      d.z != 0.0 ? 1.0 / d.z : 0.0);
    const pk_cdp bvh = (pk_cdp)S.bvh;
    const pk_cdp tri = (pk_cdp)S.tri;
    const pk_cip ord = (pk_cip)S.bvh_tri;
    int* stk = S.wstk;
    bool tf = false;
    double tb = 0.0;
    int ti = 0;
    int sp = 0;
    stk[sp++] = 0;  // every active lane writes the same value
    while (sp > 0) {
        const int node = __builtin_amdgcn_readfirstlane(stk[--sp]);
        const pk_cdp nd = bvh + kBvhNodeStride * node;
        const double bound = tf ? (found ? fmin(tb, best) : tb) : (found ? best : INFINITY);
        double tn;
        const bool in = bvh_box_v(mk(nd[0], nd[1], nd[2]), mk(nd[3], nd[4], nd[5]), o, d, inv, tn) &&
                        !(tn > bound * (1.0 + 1e-9));
        if (__ballot(in) == 0) continue;  // uniform
        const double w = nd[6];
        const int first = __double2loint(w), count = __double2hiint(w);
        if (count > 0) {
            if (in) {
                for (int j = first; j < first + count; ++j) {
                    const int i = ord[j];
                    const pk_cdp q = tri + kTriStride * i;
                    double t;
                    if (tri_hit_v(mk(q[0], q[1], q[2]), mk(q[3], q[4], q[5]), mk(q[6], q[7], q[8]),
                                  o, d, t) &&
                        (!tf || t < tb || (t == tb && i < ti))) {
                        tf = true;
                        tb = t;
                        ti = i;
                    }
                }
            }
            continue;
        }
        const int axis = __double2loint(nd[7]);
        const double da = axis == 0 ? d.x : (axis == 1 ? d.y : d.z);
        const int pos = __builtin_popcountll(__ballot(in && da > 0.0));
        const int neg = __builtin_popcountll(__ballot(in && da < 0.0));
        const bool low_first = pos >= neg;  // the lower child is nearer for rays going up
        stk[sp++] = low_first ? first + 1 : first;
        stk[sp++] = low_first ? first : first + 1;
    }
    if (tf && (!found || tb < best)) {
        found = true;
        best = tb;
        kind = 3;
        idx = ti;
    }
}

template <int FEAT>
__device__ __forceinline__ void triangles(const PacketScene& S, d3 o, d3 d, bool& found,
                                          double& best, int& prim) {
    if (!(FEAT & kFeatTris)) return;
    const int base = S.ns + S.np;
    if (S.bvh) {
        int kind = 0, ti = -1;
        bvh_wave(S, o, d, found, best, kind, ti);
        if (kind == 3) prim = base + ti;
        return;
    }
    for (int i = 0; i < S.nt; ++i) {
        double t;
        if (tri_hit(S.tri, i, o, d, t) && (!found || t < best)) {
            found = true;
            best = t;
            prim = base + i;
        }
    }
}

// The candidate spheres of a camera ray (origin = the camera): closest_camera's sphere part.
template <int MAXC>
__device__ __forceinline__ void camera_spheres(const PacketScene& S, const Masks<MAXC>& M,
                                               int nchunks, d3 o, d3 d, bool& found, double& best,
                                               int& prim) {
    const double a = dot(d, d);
    const double two_a = 2.0 * a, four_a = 4.0 * a;
    const bool regular = two_a > 0.0;
    const bool core = two_a >= 0x1p-100 && two_a <= 0x1p100;  // camera rays are unit vectors
    if (__ballot(!core) == 0) {  // uniform: the whole wave divides through the shared reciprocal
        const double r2a = rcp_refined(two_a);
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (c >= nchunks) break;
            uint64_t m = M.m[c];
            while (m) {
                const int i = c * 64 + __builtin_ctzll(m);
                m &= m - 1;
                const double* q = S.sph + kPkSph * i;
                const double b = 2.0 * dot(o - mk(q[0], q[1], q[2]), d);  // oc = cam − C
                const double disc = b * b - four_a * q[8];
                sphere_roots_core<(MAXC > 1)>(b, disc, two_a, r2a, i, S.orig, found, best, prim);
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (c >= nchunks) break;
            uint64_t m = M.m[c];
            while (m) {
                const int i = c * 64 + __builtin_ctzll(m);
                m &= m - 1;
                const double* q = S.sph + kPkSph * i;
                const double b = 2.0 * dot(o - mk(q[0], q[1], q[2]), d);  // oc = cam − C
                const double disc = b * b - four_a * q[8];
                if (regular) sphere_roots<(MAXC > 1)>(b, disc, two_a, i, S.orig, found, best, prim);
                else sphere_roots_literal<(MAXC > 1)>(b, disc, two_a, i, S.orig, found, best, prim);
            }
        }
    }
}

// IntersectClosest for a camera ray (origin = the camera) over the candidate spheres.
template <int MAXC, int FEAT>
__device__ __forceinline__ bool closest_camera(const PacketScene& S, const Masks<MAXC>& M,
                                               int nchunks, d3 o, d3 d, PkHit& h) {
    bool found = false;
    double best = 0.0;
    int prim = -1;
    // Up to 64 spheres (one mask word): a wave whose cone holds no sphere (uniform, an SGPR
    // compare) goes straight to the planes, which do not read the quadratic's `a`.  The compiler
    // branches around the reciprocal by itself but leaves a = d·d, 2a, 4a and the range compares
    // (9 VALU) in front of its test.  With more chunks a similar branch cost C3/C4 2 %; the
    // area-light variants are left alone (kLean in packet_direct_kernel).
    if (MAXC > 1 || (FEAT & kFeatArea) != 0 || M.m[0] != 0)
        camera_spheres<MAXC>(S, M, nchunks, o, d, found, best, prim);
    for (int i = 0; i < S.np; ++i) {
        const double* p = S.pl + kPlStride * i;
        const double denom = dot(mk(p[3], p[4], p[5]), d);
        if (p[7] != 0.0) plane_t_core(p[6], denom, S.ns + i, found, best, prim);  // uniform
        else plane_t(p[6], denom, S.ns + i, found, best, prim);
    }
    triangles<FEAT>(S, o, d, found, best, prim);
    h.t = best;
    h.prim = prim;
    return found;
}

// IntersectClosest for an arbitrary ray over the candidate spheres.
template <int MAXC, int FEAT>
__device__ __forceinline__ bool closest_masked(const PacketScene& S, const Masks<MAXC>& M,
                                               int nchunks, d3 o, d3 d, PkHit& h) {
    bool found = false;
    double best = 0.0;
    int prim = -1;
    const double a = dot(d, d);
    const double two_a = 2.0 * a, four_a = 4.0 * a;
    const bool regular = two_a > 0.0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        if (c >= nchunks) break;
        uint64_t m = M.m[c];
        while (m) {
            const int i = c * 64 + __builtin_ctzll(m);
            m &= m - 1;
            const double* s = S.sph + kPkSph * i;
            const d3 oc = o - mk(s[0], s[1], s[2]);
            const double b = 2.0 * dot(oc, d);
            const double cc = dot(oc, oc) - s[3];
            const double disc = b * b - four_a * cc;
            if (regular) sphere_roots<(MAXC > 1)>(b, disc, two_a, i, S.orig, found, best, prim);
            else sphere_roots_literal<(MAXC > 1)>(b, disc, two_a, i, S.orig, found, best, prim);
        }
    }
    for (int i = 0; i < S.np; ++i) {
        const double* p = S.pl + kPlStride * i;
        const d3 n = mk(p[3], p[4], p[5]);
        plane_t(dot(mk(p[0], p[1], p[2]) - o, n), dot(n, d), S.ns + i, found, best, prim);
    }
    triangles<FEAT>(S, o, d, found, best, prim);
    h.t = best;
    h.prim = prim;
    return found;
}

template <int MAXC>
__device__ __forceinline__ const double* pk_material(const PacketScene& S, const PkHit& h) {
    // the table is [spheres | planes | triangles] in scene order; spheres in chunk order (MAXC
    // > 1: > 64 spheres) map back to it
    int m = h.prim;
    if constexpr (MAXC > 1) m = h.prim < S.ns ? S.orig[h.prim] : h.prim;
    return S.mat + kMatStride * m;
}

__device__ __forceinline__ d3 pk_normal(const PacketScene& S, const PkHit& h, d3 p) {
    if (h.prim < S.ns) {
        const double* s = S.sph + kPkSph * h.prim;
        return unit(p - mk(s[0], s[1], s[2]));
    }
    if (h.prim < S.ns + S.np) {
        const double* q = S.pl + kPlStride * (h.prim - S.ns);
        return mk(q[3], q[4], q[5]);
    }
    const double* q = S.tri + kTriStride * (h.prim - S.ns - S.np);
    return mk(q[9], q[10], q[11]);
}

// The packet kernel's LDS image of a scene seen from one camera (layout below, 16-byte
// aligned arrays): spheres, camera-cone terms, culling radii, camera-ray sphere constants,
// planes with their camera numerators, point lights, camera-ray plane normals.  Formed by each
// workgroup into LDS, or once per (scene, camera) into HBM by packet_image_kernel and copied.
// With >= kSphChunkMin spheres the spheres are in spatial-chunk order, each chunk's bounding
// sphere follows them as a pseudo-sphere in the sphere / cone / radius arrays, and the scene
// index of every sorted sphere closes the image.
__host__ __device__ inline int pk_chunk_bounds(int ns) { return ns >= kSphChunkMin ? (ns + 63) / 64 : 0; }
__host__ __device__ inline size_t pk_image_bytes(int ns, int np, int nl) {
    const size_t nsb = static_cast<size_t>(ns) + pk_chunk_bounds(ns);
    const size_t b = sizeof(double) * (static_cast<size_t>(kPkSph) * nsb +
                                       static_cast<size_t>(kPlStride + 4) * np +
                                       static_cast<size_t>(kLtStride) * nl) +
                     (pk_chunk_bounds(ns) ? sizeof(int32_t) * ns : 0);
    return (b + 15) / 16 * 16;
}

// pk_build_image is the format's definition: the five array pointers below are the layout, and
// pk_image_bytes its size.  The kernels that read an image (packet_direct_kernel,
// gbuffer_packet_kernel) spell the same five lines out again: taken from one shared function
// (struct by value or by reference, one accessor per array) the same addresses come out of the
// default scheduler in another instruction order — the products kPlStride·np and kLtStride·nl
// are no longer shared with their other uses in the caller — and the kernels' assembly changes.
__device__ __forceinline__ void pk_build_image(const TraceParams& P, const double* camp,
                                               double* img, int tid, int nthreads) {
    const int ns = P.ns, np = P.np, nl = P.nl, nb = pk_chunk_bounds(ns), nsb = ns + nb;
    double* s_sph = img;                                          // 80·nsb bytes
    double* s_pl = s_sph + kPkSph * nsb;
    double* s_lt = s_pl + kPlStride * np;
    double* s_pln = s_lt + kLtStride * nl;                        // 4·np doubles
    int32_t* s_orig = reinterpret_cast<int32_t*>(s_pln + 4 * np);  // nb > 0 only
    const d3 cam = mk(camp[0], camp[1], camp[2]);
    const int32_t* perm = nb ? P.sph_perm : nullptr;
    for (int i = tid; i < nb; i += nthreads) {  // chunk bounds as pseudo-spheres ns + c
        const double* q = P.sph_bnd + 4 * i;
        double* o = s_sph + kPkSph * (ns + i);
        o[0] = q[0];
        o[1] = q[1];
        o[2] = q[2];
        o[3] = q[3] * q[3];
        o[8] = 0.0;
        o[9] = 0.0;
        cone_terms(o, q[3], cam, reinterpret_cast<float*>(o + 4));
    }
    for (int i = tid; i < ns; i += nthreads) {
        const int si = perm ? perm[i] : i;
        if (perm) s_orig[i] = si;
        const double* s = P.sph + kSphStride * si;
        double* o = s_sph + kPkSph * i;
        o[0] = s[0];
        o[1] = s[1];
        o[2] = s[2];
        o[3] = s[3];
        o[9] = 0.0;
        // culling radius (only ever used with a margin, rounded up to FP32 in cone_terms)
        cone_terms(s, sqrt(s[3]), cam, reinterpret_cast<float*>(o + 4));
        // camera-ray constant of Sphere::Intersect (Shape.h:73,77)
        const d3 oc = cam - mk(s[0], s[1], s[2]);
        o[8] = dot(oc, oc) - s[3];
    }
    for (int i = tid; i < np; i += nthreads) {
        const double* p = P.pl + kPlStride * i;
        double* o = s_pl + kPlStride * i;
        for (int k = 0; k < 6; ++k) o[k] = p[k];
        // camera-ray numerator of Plane::Intersect (Shape.h:152-153)
        o[6] = dot(mk(p[0], p[1], p[2]) - cam, mk(p[3], p[4], p[5]));
        // 1 when camera rays may divide it through the core (plane_t_core)
        const double n1 = fabs(p[3]) + fabs(p[4]) + fabs(p[5]);
        o[7] = fabs(o[6]) >= 0x1p-900 && fabs(o[6]) <= 0x1p400 && n1 <= 0x1p90 ? 1.0 : 0.0;
        // Shading normal of a camera-ray hit on this plane (Scene.h:147-154 then directLightning's
        // normalize, Scene.h:81).  A hit has t = num/denom ≥ 0 with 2^-900 ≤ |num| (no underflow
        // to ±0) and |denom| > 1e-6, so sign(denom) = sign(num); with |n|₁ ≤ 2 both n·d and the
        // reference's n·normalize(d) are within 5ε·|n|₁ ≪ 1e-6 of the exact n·d, so frontFace
        // (n·normalize(d) < 0) is num < 0 for every camera ray that hits the plane, and the
        // normal is unit(num < 0 ? n : −n): the same for the whole frame.
        const d3 pn = mk(p[3], p[4], p[5]);
        const d3 un = unit(o[6] < 0.0 ? pn : -pn);
        double* q = s_pln + 4 * i;
        q[0] = un.x;
        q[1] = un.y;
        q[2] = un.z;
        q[3] = o[7] != 0.0 && n1 <= 2.0 ? 1.0 : 0.0;
    }
    for (int i = tid; i < kLtStride * nl; i += nthreads) s_lt[i] = P.lt[i];

}

}  // namespace rtamd
