// rt_shadow_table.hpp — the shadow-cull candidate mask of one wave tile and one point light,
// formed outside the packet kernel (rt_packet.hip packet_cone_table_kernel, the same lane per tile
// that forms the tile's camera-cone mask) and read by pk_light (rt_packet_kernel.hpp) with one
// scalar load instead of origin_ball + cull_capsule in every casting wave.
//
// Plain C++: no device builtin, so a host program can call every function here
// (tests/test_shadow_table_host.py builds one and checks the words against FP64 intersections of
// the oracle's shadow rays).  Contraction: the library and the host test are both built with
// -ffp-contract=off (build.py's HIP_FLAGS cover every translation unit, whatever the place of a
// `#pragma clang fp contract` relative to this header), so the device forms the host's words;
// nothing here relies on that — an FMA's rounding is far inside every slack below.
//
// Which tiles get a word.  pk_light's mask is formed from the wave's hit points; a conservative
// one follows from the scene, the camera and the tile alone when the tile can only see planes:
// its camera-cone mask (rt_cone_table.hpp) is empty, so no camera ray of the tile meets a sphere
// and every shadow origin lies on a plane.  Every ray of the tile is unit(v) for a v of the
// rectangle spanned by the four corner vectors in the plane z = dz (rt_cone_table.hpp's header).
//
// Classification.  Plane i (point p, normal n, num = (p − cam)·n as the packet image holds it) is
// met by the ray along v at t·|v| = num / (n·v): g(v) = (n·v)/num is 1/t of the unnormalised ray
// and linear in v, so its sign and any linear comparison of two planes' g over the rectangle are
// decided at the four corners.
//   never hit:  (n·v)·sign(num) ≤ 0 at every corner, as computed.  The exact value is then
//               ≤ 1e-15·Σ|n_k v_k| over the rectangle and the kernel's n·d ≤ 2e-15·|n|₁ on the
//               hit side, under plane_t's acceptance |n·d| > 1e-6 (|n|₁ ≤ 2 is required below);
//               on the other side t < 0, and |num| ≥ 2^-900 keeps it from rounding to −0.
//   always hit: (n·v)·sign(num) > 1e-12·Σ|n_k v_k| at every corner, and
//               min_corner |n·v| / max_corner |v| ≥ 2e-6: n·v is linear and of one sign, |v| is
//               convex, so every ray of the tile has |n·d| ≥ 2e-6 exactly and > 1e-6 as the kernel
//               computes it — plane_t accepts the plane for every ray, with t > 0.
//   anything else (a horizon inside the tile, |num| outside [2^-200, 2^200], |n|₁ > 2 or
//   < 2^-20, a non-finite value): no word for the tile.
// Hidden planes.  An always-hit plane j is left out when some always-hit plane i has
// g_i ≥ g_j·(1 + 1e-9) at every corner: then t_i ≤ t_j/(1 + 1e-9) for every ray, the kernel's
// quotients (each within 1e-9 relative of exact, below) keep t_i < t_j, and plane_t's strict
// t < best never ends on j.  Planes the margin cannot order are both kept.  Without this rule a
// wall's patch "below the floor" keeps five times the candidates.
//
// The ball of a kept plane.  The tile's hit points on it are the central projection of the
// rectangle onto the plane — a projective map that sends the rectangle (on one side of the
// plane's horizon: always hit) to the convex hull of the four projected corners
// h_k = cam + v_k·(num / n·v_k).  The ball around their mean c with R = max |h_k − c| holds that
// hull (R through an FP32 square root rounded up).  Rounding budget: with |n|₁ ≤ 2 and |n·d| ≥ 2e-6 the kernel's denominator carries
// ≤ 5e-16·2 / 2e-6 = 5e-10 relative error, so its hit point cam + d·t is within 6e-10·|h − cam|
// of the exact one, and so are the h_k formed here; R takes 1e-8·(|cam|₁ + |c|₁ + R) for both
// (8× their sum), is rounded up to FP32 by the (1 + 1e-5) origin_ball applies, and gains
// |bias|·1.001 for so = hp + n·bias with |n| ≤ 1 + 2ε (the oriented unit normal).
//
// The word is the OR over the kept planes of shadow_keeps — cull_capsule's sphere test
// (rt_packet_device.hpp) at (c, R, light, RL = 0, bias) with the same FP32 expressions, slack,
// `huge`, `far` and NaN rules; 1.0f / sl2 stands for v_rcp_f32 (within an ulp, inside the slack;
// a denormal sl2 gives a large or infinite quotient, and then an inf or NaN distance keeps the
// sphere).  A real word never has a bit ≥ ns set, so all-ones (ns ≤ 63) says "no word": the
// wave forms its own mask.  Tables are built for at most kShadowTabLights point lights,
// kShadowTabPlanes planes and 63 spheres, and never with an area light.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_cone_table.hpp"
#include "rt_tile_table.hpp"

#if defined(__clang__)
#define RT_ST_UNROLL _Pragma("unroll")
#else
#define RT_ST_UNROLL
#endif

namespace rtamd {

// (kShadowTabLights, the lights a table has words for: rt_tile_table.hpp)
constexpr int kShadowTabPlanes = 8;
constexpr unsigned long long kShadowNoWord = ~0ull;
// The tile class (tile_class_word, below): the relative margin of its plane ordering, and its
// words — 0: the general path; 1: every ray of the tile misses everything; 2 + i: every ray's
// closest hit is plane i, and no shadow ray of the tile can meet a sphere.
constexpr double kClassMargin = 1e-6;
constexpr unsigned long long kTileGeneral = 0ull, kTileSky = 1ull, kTilePlane0 = 2ull;

// Lights per tile a scene's table holds (0: no shadow table for this scene).
RT_CT_HD inline int shadow_table_lights(int ns, int np, int nl, bool area_light) {
    return (!area_light && ns >= 1 && ns <= 63 && np >= 1 && np <= kShadowTabPlanes && nl >= 1 &&
            nl <= kShadowTabLights)
               ? nl
               : 0;
}

struct ShadowBall {
    double c[3];
    float R;     // holds every shadow origin of the tile on its plane (bias included)
    int plane;   // the kept plane's index in `planes`
    bool lead;   // ahead of every other always-hit plane by kClassMargin (tile_class_word)
};
template <int kMaxPlanes = kShadowTabPlanes>
struct ShadowBound {
    ShadowBall ball[kMaxPlanes];
    int n;    // kept planes
    bool ok;  // false: no word for the tile
};

// The tile's origin balls.  planes: np records of 8 doubles px py pz nx ny nz num flag (the
// packet image's: num = (p − cam)·n, flag ≠ 0 when 2^-900 ≤ |num| ≤ 2^400 and |n|₁ ≤ 2^90).
// kCorners = 4 and kHideCorners = 4 are the bound; other values exist for the host test's
// mutants only, as kBiasInR = false does.  kMaxPlanes: the caller's cap on np (the table kernel's
// is 2 — scenes of three planes or more take the plane-culling variant, which reads no table —
// so its loops unroll and its arrays stay in registers).  Divisions are kept to the four
// t_k = num / n·v_k of a kept plane: the classification compares n·v, the hidden-plane rule
// cross-multiplies.
template <int kMaxPlanes = kShadowTabPlanes, int kCorners = 4, int kHideCorners = 4,
          bool kBiasInR = true>
RT_CT_HD inline ShadowBound<kMaxPlanes> shadow_tile_bound(const ConeRect& q, double half_w,
                                                          double half_h, const double* cam,
                                                          double dz, const double* planes, int np,
                                                          double bias) {
    ShadowBound<kMaxPlanes> B;
    B.n = 0;
    B.ok = false;
    if (np < 1 || np > kMaxPlanes) return B;
    double v[4][3], vl2_max = 0.0;
    for (int k = 0; k < 4; ++k) {  // the kernel's expression (cone_tile_bound)
        v[k][0] = (static_cast<double>((k & 1) ? q.x_hi : q.x_lo) - half_w) - cam[0];
        v[k][1] = (half_h - static_cast<double>((k & 2) ? q.y_hi : q.y_lo)) - cam[1];
        v[k][2] = dz;
        const double l2 = v[k][0] * v[k][0] + v[k][1] * v[k][1] + dz * dz;
        if (!(l2 > 0.0) || !isfinite(l2)) return B;
        if (l2 > vl2_max) vl2_max = l2;
    }
    if (!(dz != 0.0) || !isfinite(dz) || !isfinite(bias)) return B;
    const double cam1 = fabs(cam[0]) + fabs(cam[1]) + fabs(cam[2]);
    if (!isfinite(cam1)) return B;
    // e[i][k] = (n_i·v_k)·sign(num_i), > 0 on the hit side; g_i(v_k) = e[i][k] / an[i]
    double e[kMaxPlanes][4], an[kMaxPlanes];
    bool hit[kMaxPlanes];
    RT_ST_UNROLL
    for (int i = 0; i < kMaxPlanes; ++i) {
        if (i >= np) break;
        const double* p = planes + 8 * i;
        const double num = p[6];
        const double n1 = fabs(p[3]) + fabs(p[4]) + fabs(p[5]);
        if (!(p[7] != 0.0) || !(n1 <= 2.0) || !(n1 >= 0x1p-20) || !(num != 0.0) || !isfinite(num))
            return B;
        // (the cross-multiplied products of the hidden-plane rule stay finite and normal)
        if (!(fabs(num) <= 0x1p200) || !(fabs(num) >= 0x1p-200)) return B;
        an[i] = fabs(num);
        int n_hit = 0, n_miss = 0;
        double e_min = INFINITY;
        for (int k = 0; k < 4; ++k) {
            const double a = p[3] * v[k][0], b = p[4] * v[k][1], c = p[5] * v[k][2];
            const double ek = num > 0.0 ? (a + b) + c : -((a + b) + c);
            const double mag = (fabs(a) + fabs(b)) + fabs(c);
            if (!isfinite(ek) || !(fabs(ek) <= 0x1p200)) return B;
            if (ek > 1e-12 * mag) ++n_hit;
            else if (ek <= 0.0) ++n_miss;
            if (fabs(ek) < e_min) e_min = fabs(ek);
            e[i][k] = ek;
        }
        if (n_miss == 4) {
            hit[i] = false;
        } else if (n_hit == 4 && e_min * e_min >= 4e-12 * vl2_max) {  // |n·v| ≥ 2e-6·|v|
            hit[i] = true;
        } else {
            return B;
        }
    }
    RT_ST_UNROLL
    for (int j = 0; j < kMaxPlanes; ++j) {
        if (j >= np) break;
        if (!hit[j]) continue;
        bool hidden = false;
    RT_ST_UNROLL
        for (int i = 0; i < kMaxPlanes; ++i) {
            if (i >= np || hidden) break;
            if (i == j || !hit[i]) continue;
            // g_i ≥ g_j·(1 + 1e-9), all four factors positive and ≤ 2^200; a product under the
            // normal range orders nothing
            int ahead = 0;
            for (int k = 0; k < kHideCorners; ++k) {
                const double lhs = e[i][k] * an[j], rhs = e[j][k] * an[i];
                ahead += lhs >= rhs * (1.0 + 1e-9) && rhs >= 0x1p-900;
            }
            hidden = ahead == kHideCorners;
        }
        if (hidden) continue;
        ShadowBall& S = B.ball[B.n];
        S.plane = j;
        // the tile class's own ordering test (tile_class_word): g_j ≥ g_i·(1 + kClassMargin) at
        // every corner, for every other always-hit plane i, decided by j itself
        S.lead = true;
    RT_ST_UNROLL
        for (int i = 0; i < kMaxPlanes; ++i) {
            if (i >= np) break;
            if (i == j || !hit[i]) continue;
            int ahead = 0;
            for (int k = 0; k < kHideCorners; ++k) {
                const double lhs = e[j][k] * an[i], rhs = e[i][k] * an[j];
                ahead += lhs >= rhs * (1.0 + kClassMargin) && rhs >= 0x1p-900;
            }
            S.lead = S.lead && ahead == kHideCorners;
        }
        double h[4][3];
        S.c[0] = S.c[1] = S.c[2] = 0.0;
        // t_k = num / n·v_k through ONE division: an · Π_{m≠k} e_m / Π e_m (each factor in
        // (0, 2^200], the products normal or the tile has no word; a few ulps, inside the 1e-8)
        const double e01 = e[j][0] * e[j][1], e23 = e[j][2] * e[j][3];
        const double scale = an[j] / (e01 * e23);
        if (!(e01 * e23 >= 0x1p-900) || !isfinite(scale)) return B;
        const double tk[4] = {scale * (e[j][1] * e23), scale * (e[j][0] * e23),
                              scale * (e01 * e[j][3]), scale * (e01 * e[j][2])};
        for (int k = 0; k < kCorners; ++k) {
            const double t = tk[k];
            for (int a = 0; a < 3; ++a) {
                h[k][a] = cam[a] + v[k][a] * t;
                S.c[a] += h[k][a] / kCorners;
            }
        }
        double r2 = 0.0;
        for (int k = 0; k < kCorners; ++k) {
            const double dx = h[k][0] - S.c[0], dy = h[k][1] - S.c[1], dz_ = h[k][2] - S.c[2];
            const double d2 = dx * dx + dy * dy + dz_ * dz_;
            if (d2 > r2) r2 = d2;
        }
        // (an FP32 square root rounded up: R is only ever an upper bound)
        const double R = static_cast<double>(sqrtf(static_cast<float>(r2) * (1.0f + 1e-6f)) *
                                             (1.0f + 1e-6f));
        const double c1 = fabs(S.c[0]) + fabs(S.c[1]) + fabs(S.c[2]);
        const double Rm = R + 1e-8 * ((cam1 + c1) + R);
        if (!isfinite(Rm) || !isfinite(c1)) return B;
        S.R = static_cast<float>(Rm) * (1.0f + 1e-5f);
        if (kBiasInR) S.R += static_cast<float>(fabs(bias)) * (1.0f + 1e-6f) * 1.001f;
        if (!isfinite(S.R)) return B;
        ++B.n;
    }
    B.ok = true;
    return B;
}

// cull_capsule's sphere test for RL = 0: origins in the ball (c, R), rays towards L.  The
// segment's terms are formed once for a ball and a light (as cull_capsule forms them once for a
// wave), then each sphere — centre s, culling radius r (cone_terms' float 7) — is tested.
struct ShadowSeg {
    float sx, sy, sz, sl2, inv_sl2, Rc;
    bool huge;
};
RT_CT_HD inline ShadowSeg shadow_seg(const double* c, float R, const double* L, double bias) {
    ShadowSeg G;
    G.sx = static_cast<float>(L[0] - c[0]);
    G.sy = static_cast<float>(L[1] - c[1]);
    G.sz = static_cast<float>(L[2] - c[2]);
    G.sl2 = G.sx * G.sx + G.sy * G.sy + G.sz * G.sz;
    G.inv_sl2 = 1.0f / G.sl2;  // only read when sl2 > 0
    G.huge = !(G.sl2 <= 0x1p120f);
    G.Rc = (R > 0.0f ? R : 0.0f) + static_cast<float>(fabs(bias)) * (1.0f + 1e-6f) * 1.001f;
    return G;
}
RT_CT_HD inline bool shadow_seg_keeps(const ShadowSeg& G, const double* c, const double* s,
                                      float r) {
    const float vx = static_cast<float>(s[0] - c[0]), vy = static_cast<float>(s[1] - c[1]),
                vz = static_cast<float>(s[2] - c[2]);
    const float vs = vx * G.sx + vy * G.sy + vz * G.sz;
    const float vv = vx * vx + vy * vy + vz * vz;
    float d2;
    if (!(vs > 0.0f) || !(G.sl2 > 0.0f)) {
        d2 = vv;
    } else if (!(vs < G.sl2)) {
        const float wx = vx - G.sx, wy = vy - G.sy, wz = vz - G.sz;
        d2 = wx * wx + wy * wy + wz * wz;
    } else {
        d2 = vv - (vs * vs) * G.inv_sl2;
    }
    const float lim = (r + G.Rc) * (1.0f + 1e-4f);
    const float far = 1e5f * r - G.Rc;
    return !(d2 > lim * lim + 2e-5f * (vv + G.sl2)) || !(far > 0.0f) || !(vv <= far * far) ||
           G.huge;
}
RT_CT_HD inline bool shadow_keeps(const double* c, float R, const double* L, double bias,
                                  const double* s, float r) {
    return shadow_seg_keeps(shadow_seg(c, R, L, bias), c, s, r);
}

// The tile's word for a light at L over spheres [0, ns), ns ≤ 63: sphere i's centre is
// sph + sph_stride · i (doubles) and its culling radius rad[rad_stride · i] (floats).
template <int kMaxPlanes>
RT_CT_HD inline unsigned long long shadow_tile_word(const ShadowBound<kMaxPlanes>& B,
                                                    const double* L, double bias,
                                                    const double* sph, int sph_stride,
                                                    const float* rad, int rad_stride, int ns) {
    if (!B.ok || ns > 63) return kShadowNoWord;
    unsigned long long m = 0;
    RT_ST_UNROLL
    for (int b = 0; b < kMaxPlanes; ++b) {
        if (b >= B.n) break;
        const ShadowSeg G = shadow_seg(B.ball[b].c, B.ball[b].R, L, bias);
        for (int i = 0; i < ns; ++i)
            if (shadow_seg_keeps(G, B.ball[b].c, sph + static_cast<long>(sph_stride) * i,
                                 rad[static_cast<long>(rad_stride) * i]))
                m |= 1ull << i;
    }
    return m;
}

// The tile's class word (packet_direct_kernel's uniform path, rt_packet_kernel.hpp).  A tile is
// *uniform* when its cone mask is empty (no camera ray meets a sphere), shadow_tile_bound decided
// every plane (ok) and kept at most one, every light's shadow word is 0 (no shadow ray of the tile
// can meet a sphere: a word is a superset of the spheres any of them meets), nl ≤
// kShadowTabLights, and — with a kept plane — the packet image holds that plane's oriented unit
// normal (pln[4i + 3] ≠ 0: s_pln of pk_build_image) and the plane leads.
//
// What the class claims.  Sky (no kept plane): every plane is "never hit", so plane_t /
// plane_t_core reject each for every ray of the tile and IntersectClosest misses.  Plane i: it is
// "always hit" (t > 0, |n·d| > 1e-6 as the kernel computes it), every other plane is never hit
// or an always-hit plane j with g_i ≥ g_j·(1 + kClassMargin) at the four corners.  g_i − (1 + m)·g_j
// is linear in v, so the inequality holds exactly over the rectangle up to the corners' rounding:
// each e[·][k] = n·v_k carries ≤ 3ε·Σ|n_a v_a| ≤ 3ε·2√3·|v| of error against |n·v| ≥ 2e-6·|v|,
// 6e-10 relative, twice (i and j); the kernel's t = num / (n·d) has the image's own num (the one
// read here) and a denominator within 5ε·|n|₁ ≤ 1.1e-15 of the exact n·v/|v| (three products,
// two sums, d's components within 2ε), 5.5e-10 relative at |n·d| ≥ 2e-6, twice; the products and
// the quotients add 4ε.  Together < 2.4e-9, so with m = 1e-6 (430× that; the shadow words' 1e-9
// rule is left as it is — a plane it hides wrongly costs candidates there, a wrong t here) the
// kernel's computed t_i < t_j for every ray, and its in-order loop with strict '<' (plane_t's
// no-win skip needs t ≥ best·(1 − 2^-40)) ends on plane i with the bits of num_i / (n_i·d).
// The margin only costs tiles within 1e-6 of two planes' line of intersection, which straddle it.
//
// kClassPlanes and kIndexOff exist for the host test's mutants only (the class taken on two kept
// planes, without the ordering; the kept plane's index off by one).
template <int kMaxPlanes, int kClassPlanes = 1, int kIndexOff = 0>
RT_CT_HD inline unsigned long long tile_class_word(unsigned long long cone,
                                                   const ShadowBound<kMaxPlanes>& B,
                                                   const unsigned long long* words, int nl,
                                                   const double* pln, int np) {
    if (cone != 0 || !B.ok || B.n > kClassPlanes || nl < 1 || nl > kShadowTabLights)
        return kTileGeneral;
    for (int l = 0; l < nl; ++l)
        if (words[l] != 0) return kTileGeneral;
    if (B.n == 0) return kTileSky;
    const int i = B.ball[0].plane;
    if (kClassPlanes == 1 && !B.ball[0].lead) return kTileGeneral;
    if (i < 0 || i >= np || !(pln[4 * i + 3] != 0.0)) return kTileGeneral;
    return kTilePlane0 + static_cast<unsigned long long>((i + kIndexOff) % np);
}

// The shadowed-plane mark (packet_uniform_kernel<true>, rt_packet.hip).  A tile is *shadowed-plane
// i* when it meets every condition of class "plane i" but "every light's shadow word is 0": its
// cone mask is empty, the bound is ok and kept exactly plane i, which leads and has its oriented
// unit normal in the image, 1 ≤ nl ≤ kShadowTabLights, every light has a word and some word is not
// 0.  The geometric claims and their proof are tile_class_word's (every camera ray of the tile
// ends on plane i with the bits of num_i / (n_i·d)); each word is a superset of the spheres a
// shadow ray of the tile towards its light can meet (shadow_tile_word).  The tile's class byte
// stays kTileGeneral — the single launch renders it on its general path and counts it general —
// and the mark rides in bits the class byte and the keep masks leave free: bit 40, with the
// plane's index in bits 41-43.  Only the table word carries it: a list entry has the tile's
// column there (tile_shadowed_entry writes the plane's class into the class byte instead).
// kNoWordOk and kIndexOff exist for the host test's mutants only (the mark taken on a tile with a
// cone mask or a light without a word; the plane's index off by one).
constexpr unsigned long long kTileShadowedBit = 1ull << 40;
constexpr int kTileShadowedPlaneShift = 41;
template <int kMaxPlanes, bool kNoWordOk = false, int kIndexOff = 0>
RT_CT_HD inline unsigned long long tile_shadowed_mark(unsigned long long cone,
                                                      const ShadowBound<kMaxPlanes>& B,
                                                      const unsigned long long* words, int nl,
                                                      const double* pln, int np) {
    if ((cone != 0 && !kNoWordOk) || !B.ok || B.n != 1 || nl < 1 || nl > kShadowTabLights)
        return 0ull;
    bool some = false;
    for (int l = 0; l < nl; ++l) {
        if (words[l] == kShadowNoWord && !kNoWordOk) return 0ull;
        some = some || words[l] != 0;
    }
    if (!some || !B.ball[0].lead) return 0ull;
    const int i = B.ball[0].plane;
    if (i < 0 || i >= np || i >= 8 || !(pln[4 * i + 3] != 0.0)) return 0ull;
    return kTileShadowedBit |
           (static_cast<unsigned long long>((i + kIndexOff) % np) << kTileShadowedPlaneShift);
}

// The planes a tile's shadow rays towards the light at L must still classify: bit i stands for
// plane i of `planes`, kPlaneKeepAll says nothing is proven.  The class word carries one such
// mask per light next to the class (tile_class_pack), and pk_uniform_tile (rt_packet_kernel.hpp)
// leaves a dropped plane out of its shadow classification.
//
// What the kernel computes.  A casting lane (`need`) has its hit point hp on the ball's plane,
// within the ball; so = hp + n·bias with the plane's oriented unit normal n; D = unit(L − hp),
// dist = |L − hp| > bias, max_dist = dist − bias.  For plane i (point p, stored normal q, N = |q|,
// u = q/N) it forms dn = q·D and nm = (p − so)·q, A = nm·sign(dn), B = |dn|, and leaves the
// plane at a `continue` — neither `blocked` nor `undecided` — when |dn| ≤ 1e-6, when
// A < −1e-300·B, or when A ≥ max_dist·B·(1 + 1e-9).  A plane that always leaves this way can be
// left out: no bit of T, of `fix` or of the pixel depends on it.  Below, s(x) = (x − p)·u is the
// signed distance from plane i, m = margin·scale, and
//   scale = |cam|₁ + |c|₁ + |L|₁ + |p|₁ + R + |bias|
// for the ball (c, R), which bounds every coordinate and every distance that appears (hp and so
// lie in the ball, dist ≤ |L|₁ + |c|₁ + R); 2^-200 ≤ scale ≤ 2^200 or the plane is kept, and
// 2^-20 ≤ |q|₁ ≤ 2 holds for every plane of a bound that is ok (shadow_tile_bound).
//
// The ball's own plane is dropped when bias ≥ 1e-7·scale.  `need` has n·D > 0 and q = ±N·n up to
// rounding, so dn has the sign of ±1 or |dn| ≤ 1e-6 (the first exit).  Otherwise
// nm = (p − hp)·q − bias·(n·q) = ∓bias·N + e, A = −bias·N ± e: hp is within 6e-10·|hp − cam| of
// the plane (the rounding budget of the ball, above) and the dot product adds 4ε·(|p|₁ + |so|₁),
// so |e| ≤ 1e-8·scale·N, a tenth of bias·N.  A ≤ −0.9e-7·scale·N < −1e-300·B: the second exit.
// A bias that is negative or small against the scene's coordinates keeps the plane.
//
// Another plane i is dropped when L and the ball lie strictly on one side of it:
//   s(L) and s(c) have one sign,  |s(c)| − R ≥ 1e-6·scale,  |s(L)| − 2·|bias| ≥ 1e-6·scale.
// Take s(c) > 0 (the other sign mirrors q, which leaves A and B as they are).  Every so has
// s(so) ≥ m, so nm = −s(so)·N within 4ε·scale·N: negative, |nm| ≥ m·N·(1 − 1e-9).  dn carries
// ≤ 5ε·|q|₁ ≤ 2.3e-15 of error, so beyond the first exit its sign is exact.  dn > 0: A = nm < 0,
// the second exit.  dn < 0: the ray descends, s(so + t·D) = s(so) − t·B/N, and its end
// so + max_dist·D = L + bias·(n − D) has s ≥ s(L) − 2·|bias| ≥ m.  Hence
// s(so)·N − max_dist·B ≥ m·N, and with max_dist·B/N ≤ dist + |bias| ≤ 2·scale
//   A / (max_dist·B) ≥ 1 + m/(2·scale) = 1 + 5e-7
// against the third exit's 1e-9 and the relative errors of the computed A (1e-9: 4ε·scale·N
// over m·N), B (2.3e-9: 2.3e-15 over 1e-6) and the products (4ε): 125× their sum.  The 2·|bias|
// is needed: the ray ends bias·(n − D) off L, which can lie across the plane when n leans over
// it and the light is closer to the plane than that.
// The distances formed here carry ≤ 8ε·scale, ≪ m.  Any comparison that fails — a NaN, an
// infinity, a scale out of range — keeps the plane.
//
// kSideOfBall = false exists for the host test's mutant only (the light's side alone decides).
constexpr unsigned kPlaneKeepAll = 0xffu;
template <int kMaxPlanes, bool kSideOfBall = true>
RT_CT_HD inline unsigned shadow_plane_keep(const ShadowBound<kMaxPlanes>& B, const double* L,
                                           const double* planes, int np, const double* cam,
                                           double bias) {
    if (!B.ok || np < 1 || np > kMaxPlanes || np > 8) return kPlaneKeepAll;
    const double ab = fabs(bias);
    const double base = ((fabs(cam[0]) + fabs(cam[1])) + fabs(cam[2])) +
                        ((fabs(L[0]) + fabs(L[1])) + fabs(L[2])) + ab;
    unsigned keep = 0;
    RT_ST_UNROLL
    for (int i = 0; i < kMaxPlanes; ++i) {
        if (i >= np) break;
        const double* p = planes + 8 * i;
        const double N = sqrt((p[3] * p[3] + p[4] * p[4]) + p[5] * p[5]);
        const double p1 = (fabs(p[0]) + fabs(p[1])) + fabs(p[2]);
        // N·s(L)
        const double sL = ((L[0] - p[0]) * p[3] + (L[1] - p[1]) * p[4]) + (L[2] - p[2]) * p[5];
        bool drop = N >= 0x1p-21 && N <= 2.0;
        RT_ST_UNROLL
        for (int b = 0; b < kMaxPlanes; ++b) {
            if (b >= B.n) break;
            const ShadowBall& S = B.ball[b];
            const double R = static_cast<double>(S.R);
            const double scale =
                (base + p1) + (((fabs(S.c[0]) + fabs(S.c[1])) + fabs(S.c[2])) + R);
            if (!(scale >= 0x1p-200 && scale <= 0x1p200)) drop = false;
            if (S.plane == i) {
                if (!(bias >= 1e-7 * scale)) drop = false;
                continue;
            }
            const double m = 1e-6 * scale * N;
            const double sc =
                ((S.c[0] - p[0]) * p[3] + (S.c[1] - p[1]) * p[4]) + (S.c[2] - p[2]) * p[5];
            if (!((sL > 0.0 && sc > 0.0) || (sL < 0.0 && sc < 0.0)) && kSideOfBall) drop = false;
            if (!(fabs(sc) - R * N >= m) && kSideOfBall) drop = false;
            if (!(fabs(sL) - 2.0 * ab * N >= m)) drop = false;
        }
        if (!drop) keep |= 1u << i;
    }
    return keep;
}

// The class word as the table holds it: the class in bits 0-7 (tile_class_of), light l's keep
// mask in bits 8 + 8·l … 15 + 8·l (np ≤ 8, nl ≤ kShadowTabLights).  Every tile carries its
// masks, the general ones too, so a reader tests the class field, never the word.
constexpr unsigned long long kTileClassBits = 0xffull;
RT_CT_HD inline unsigned long long tile_class_of(unsigned long long word) {
    return word & kTileClassBits;
}
RT_CT_HD inline unsigned long long tile_class_pack(unsigned long long cls, const unsigned* keep,
                                                   int nl) {
    unsigned long long w = cls & kTileClassBits;
    for (int l = 0; l < nl && l < kShadowTabLights; ++l)
        w |= static_cast<unsigned long long>(keep[l] & kPlaneKeepAll) << (8 + 8 * l);
    return w;
}
RT_CT_HD inline unsigned tile_plane_keep(unsigned long long word, int l) {
    return static_cast<unsigned>(word >> (8 + 8 * l)) & kPlaneKeepAll;
}

// The tile lists of a frame (packet_uniform_kernel and the split launch of packet_direct_kernel,
// rt_packet_kernel.hpp): formed from the class words by the lane that forms them, where
// rt_tile_table.hpp says.  A tile is *uniform* when its class is not kTileGeneral, and *shadowed*
// when it is general and carries the shadowed-plane mark (tile_shadowed_mark: only a table with the
// third list forms marks); a workgroup is listed when at least one of its tiles is neither.  Every
// tile is therefore rendered exactly once: by a list kernel when it is uniform or shadowed, else by
// its wave of the listed workgroup (whose other waves return).
// A uniform entry is the tile's class word (bits 0-39: the class and up to four keep masks) with
// the tile's column and row in 8-pixel units above it (12 bits each), so the kernel that reads
// the list needs no second lookup and no division.
// The table kernel works on runs of 64 consecutive list positions (one wavefront): position i
// stands for tile T − 1 − i, so the lists come out roughly bottom-up, the order the general
// kernel's default dispatch has.  `waves` (2 or 4) divides 64 and T, so the tiles of a workgroup
// are `waves` adjacent, aligned lanes of one run.  The order of the runs in a list is whatever
// the runs' atomic adds make it; a list's order only permutes which workgroup renders which tile.
constexpr int kListColShift = 40, kListRowShift = 52;
constexpr unsigned long long kListWordMask = (1ull << kListColShift) - 1ull;
constexpr uint32_t kListCoordMask = 0xfffu;
constexpr uint32_t kListMaxCoord = kListCoordMask + 1u;  // tile columns and rows a list can name
RT_CT_HD inline uint32_t tile_list_tile(uint32_t pos, uint32_t tiles) { return tiles - 1u - pos; }
RT_CT_HD inline bool tile_list_uniform(unsigned long long word) {
    return tile_class_of(word) != kTileGeneral;
}
template <int kIndexOff = 0>
RT_CT_HD inline unsigned long long tile_list_entry(unsigned long long word, uint32_t x0,
                                                   uint32_t yl0) {
    return (word & kListWordMask) |
           (static_cast<unsigned long long>((x0 / 8u + kIndexOff) & kListCoordMask) << kListColShift) |
           (static_cast<unsigned long long>((yl0 / 8u) & kListCoordMask) << kListRowShift);
}
// Whether the workgroup of run lane `lane` is listed, from the run's mask of general tiles.
template <bool kDropMixed = false>
RT_CT_HD inline bool tile_list_wg_listed(uint64_t general, unsigned lane, unsigned waves) {
    const uint64_t group = (waves >= 64u ? ~0ull : (1ull << waves) - 1ull);
    const uint64_t g = (general >> (lane & ~(waves - 1u))) & group;
    return kDropMixed ? g == group : g != 0;
}
// A shadowed tile of a table word (a general class byte with the mark), and its list entry: the
// uniform entry the tile would have with class "plane i" — the keep masks as formed, the class
// byte written from the mark's plane index, column and row above them.
RT_CT_HD inline bool tile_list_shadowed(unsigned long long word) {
    return tile_class_of(word) == kTileGeneral && (word & kTileShadowedBit) != 0;
}
RT_CT_HD inline unsigned long long tile_shadowed_entry(unsigned long long word, uint32_t x0,
                                                       uint32_t yl0) {
    const unsigned long long cls = kTilePlane0 + ((word >> kTileShadowedPlaneShift) & 7ull);
    return tile_list_entry((word & ~kTileClassBits) | cls, x0, yl0);
}
// One run of up to 64 list positions from `pos0` on, as one wavefront of the table kernel forms
// it: words[] are the frame's class words by tile.  Three masks over the run's lanes (the kernel's
// three ballots) — uniform, shadowed and general tiles.  n_sh is the third list's switch: null
// for a table without it, where no tile counts as shadowed.  The run's uniform entries go to
// uni[*n_uni …], its shadowed entries to uni[shadowed_slot(*n_sh …)] downwards and its listed
// workgroups to gen[*n_gen …] (the kernel takes the three bases with one atomic add each).
// origin gives a tile's pixel origin.  The template parameters exist for the host tests' mutants
// only: an entry's column off by one, a workgroup listed only when all of its tiles are general,
// and a workgroup with a shadowed and a general wave not listed.
template <int kIndexOff = 0, bool kDropMixed = false, bool kDropShadowedMixed = false,
          class Origin>
inline void tile_list_run(const unsigned long long* words, uint32_t tiles, uint32_t waves,
                          uint32_t pos0, Origin origin, unsigned long long* uni, uint32_t* n_uni,
                          uint32_t* gen, uint32_t* n_gen, uint32_t* n_sh = nullptr) {
    uint64_t uniform = 0, shadowed = 0, general = 0;
    for (uint32_t l = 0; l < 64 && pos0 + l < tiles; ++l) {
        const unsigned long long w = words[tile_list_tile(pos0 + l, tiles)];
        if (tile_list_uniform(w)) uniform |= 1ull << l;
        else if (n_sh && tile_list_shadowed(w)) shadowed |= 1ull << l;
        else general |= 1ull << l;
    }
    for (uint32_t l = 0; l < 64 && pos0 + l < tiles; ++l) {
        const uint32_t t = tile_list_tile(pos0 + l, tiles);
        uint32_t x0, yl0;
        origin(t, x0, yl0);
        if ((uniform >> l) & 1ull) uni[(*n_uni)++] = tile_list_entry<kIndexOff>(words[t], x0, yl0);
        if ((shadowed >> l) & 1ull)
            uni[TileTabLayout::shadowed_slot((*n_sh)++, tiles)] =
                tile_shadowed_entry(words[t], x0, yl0);
        if ((l & (waves - 1u)) == 0 && tile_list_wg_listed<kDropMixed>(general, l, waves) &&
            !(kDropShadowedMixed && tile_list_wg_listed(shadowed, l, waves)))
            gen[(*n_gen)++] = t / waves;
    }
}

}  // namespace rtamd
