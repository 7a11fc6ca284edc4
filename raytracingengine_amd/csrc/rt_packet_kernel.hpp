// rt_packet_kernel.hpp — the shaded packet kernel: the shadow-ray and shading code over the
// packet machinery of rt_packet_device.hpp, packet_direct_kernel and the launch templates that
// pick its workgroup shape.  Included by the two translation units that instantiate it:
// rt_packet.hip (every variant but the area light's, scheduled for ILP) and rt_packet_area.hip
// (the area-light variants, default scheduling).
#pragma once

#include "rt_packet_device.hpp"
#include "rt_shadow_table.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// computeTransmittance (Scene.h:35-77) over the candidate spheres of the shadow packet.
template <int MAXC, int FEAT>
__device__ __forceinline__ double pk_transmittance(const PacketScene& S, const Masks<MAXC>& M,
                                                   int nchunks, d3 o, d3 d, double max_dist,
                                                   double bias) {
    double T = 1.0, traveled = 0.0;
    int safety = 64;
    while (safety-- > 0 && T > 1e-4 && traveled < max_dist) {
        PkHit h;
        if (!closest_masked<MAXC, FEAT>(S, M, nchunks, o, d, h)) break;
        const double t = h.t;
        if (t <= 0.0) {
            o = o + d * bias;
            traveled += bias;
            continue;
        }
        if (t <= bias) {
            o = (o + d * t) + d * bias;
            traveled += t + bias;
            continue;
        }
        if (traveled + t >= max_dist) break;
        T *= sclamp(pk_material<MAXC>(S, h)[5], 0.0, 1.0);
        o = (o + d * t) + d * bias;
        traveled += t + bias;
    }
    return sclamp(T, 0.0, 1.0);
}

// Occlusion test for an all-opaque scene (the only kind this kernel renders: any material with
// transparency > 0 goes to the tree kernel), where computeTransmittance (Scene.h:35-77) can only
// return 1 (clear) or 0 (blocked): its first closest hit t* decides — t* in (bias, maxDist)
// blocks, t* >= maxDist or no hit is clear, t* <= bias starts the march over near hits.  Each
// candidate is classified with a FP32 square root and one shared FP64 reciprocal instead of the
// reference's sqrt and division, with an explicit error bound Δ on every root; any root within
// Δ of a threshold (1e-6, bias, maxDist), any near hit, or any value out of the fast ranges makes
// the lane undecided, and undecided lanes run the exact march.  Returns 0 clear, 1 blocked,
// 2 undecided.  The discriminant (and with it hit/miss) is the reference's FP64 expression.
template <int MAXC, int FEAT, bool SPH>
__device__ __forceinline__ int pk_occlusion_t(const PacketScene& S, const Masks<MAXC>& M,
                                            int nchunks, d3 o, d3 d, double max_dist,
                                            double bias) {
    if constexpr ((FEAT & kFeatTris) != 0) return 2;
    bool blocked = false, undecided = false;
    // Up to 64 spheres (one mask word): a packet with no sphere candidate (uniform, an SGPR
    // compare; most of C2's, at 0.44 candidates per shadow ray) goes straight to the planes.
    // `a` and the range test on 2a serve the sphere classification only — its roots divide by
    // 2a; the plane classification below never reads them — so the early "undecided" for 2a
    // outside [2^-100, 2^100] is kept whenever the mask is not empty and skipped with the rest
    // (8 VALU per light) when it is.  SPH = false is that case as a copy of its own (pk_occlusion
    // below): one body with the branch inside spilled 8 B more per lane in C2's fix-up variant.
    if constexpr (SPH) {
        const double a = dot(d, d);
        const double two_a = 2.0 * a, four_a = 4.0 * a;
        if (!(two_a >= 0x1p-100 && two_a <= 0x1p100)) return 2;
        const double inv2a = rcp_refined(two_a);  // within 1 ulp of 1/2a: far inside the Δ margin
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
                if (disc < 0.0) continue;  // miss, exactly as the reference decides it
                if (!(disc == 0.0 || (disc > 1e-30 && disc < 1e30))) {
                    undecided = true;
                    continue;
                }
                // |sq − fl(√disc)| ≤ 5e-7·√disc (FP32 conversion + sqrt_f32), so both roots are
                // within Δ = 2e-6·(|b| + sq)/2a of the reference's fl(fl(−b ∓ sq)/2a) (2× margin)
                const double sq = static_cast<double>(sqrt_f32(static_cast<float>(disc)));
                const double delta = 2e-6 * (fabs(b) + sq) * inv2a;
                double t = (-b - sq) * inv2a;
                if (!(t >= 1e-6 + delta)) {
                    if (!(t < 1e-6 - delta)) {
                        undecided = true;
                        continue;
                    }
                    t = (-b + sq) * inv2a;
                    if (t < 1e-6 - delta) continue;  // both roots behind: no hit
                    if (!(t >= 1e-6 + delta)) {
                        undecided = true;
                        continue;
                    }
                }
                if (t >= max_dist + delta) continue;              // beyond the light
                if (t > bias + delta && t < max_dist - delta) blocked = true;
                else undecided = true;                            // near hit or on a boundary
            }
        }
    }
    for (int i = 0; i < S.np; ++i) {
        if (i < 64 && ((M.pm >> i) & 1ull) == 0) continue;  // clear for the whole packet (uniform)
        // Plane::Intersect (Shape.h:149-159): t = num / denom, decided without the division:
        // with A = num·sign(denom), B = |denom|, t lies on the side of x that A lies of x·B
        // (1e-9 relative margin ≫ the FP64 rounding of the quotient and the product)
        const double* p = S.pl + kPlStride * i;
        const d3 n = mk(p[3], p[4], p[5]);
        const double denom = dot(n, d);
        if (!(fabs(denom) > 1e-6)) continue;
        const double num = dot(mk(p[0], p[1], p[2]) - o, n);
        const double A = denom > 0.0 ? num : -num, B = fabs(denom);
        if (A < -1e-300 * B) continue;                        // t < 0 (no underflow to −0)
        if (A >= max_dist * B * (1.0 + 1e-9)) continue;       // beyond the light
        if (A > bias * B * (1.0 + 1e-9) && A < max_dist * B * (1.0 - 1e-9)) blocked = true;
        else undecided = true;
    }
    return undecided ? 2 : (blocked ? 1 : 0);
}

template <int MAXC, int FEAT>
__device__ __forceinline__ int pk_occlusion(const PacketScene& S, const Masks<MAXC>& M,
                                            int nchunks, d3 o, d3 d, double max_dist,
                                            double bias) {
    if constexpr (MAXC == 1 && (FEAT & kFeatArea) == 0)
        if (M.m[0] == 0)
            return pk_occlusion_t<MAXC, FEAT, false>(S, M, nchunks, o, d, max_dist, bias);
    return pk_occlusion_t<MAXC, FEAT, true>(S, M, nchunks, o, d, max_dist, bias);
}

// Shadow-packet candidates: the origins `so` of the lanes in `casting_lanes` lie in a ball around
// the first such lane's origin (exact), radius = the wave maximum of the distances in FP32
// rounded up; every segment ends in the light's ball (lcenter, lrad); non-finite origins or
// radius keep every sphere.
struct OriginBall {
    d3 c;
    float R;
    bool ok;  // wave-uniform: some lane casts, every origin finite, R finite
};
__device__ __forceinline__ OriginBall origin_ball(bool casting_lane, d3 so) {
    OriginBall B;
    const uint64_t casting = __ballot(casting_lane);
    B.c = mk(0.0, 0.0, 0.0);
    B.R = 0.0f;
    B.ok = false;
    if (!casting) return B;
    const bool bad = casting_lane && !(isfinite(so.x) && isfinite(so.y) && isfinite(so.z));
    B.c = lane_d3(so, __builtin_ctzll(casting));
    float r_lane = 0.0f;
    if (casting_lane) {  // |so − c| in FP32, rounded up (FP64 differences, 5e-7 rel. error)
        const float dx = static_cast<float>(so.x - B.c.x), dy = static_cast<float>(so.y - B.c.y),
                    dz = static_cast<float>(so.z - B.c.z);
        r_lane = sqrt_f32(dot3f(dx, dy, dz, dx, dy, dz)) * (1.0f + 1e-5f);
    }
    B.R = wave_red<1>(r_lane);
    B.ok = !__ballot(bad) && isfinite(B.R);
    return B;
}

template <int MAXC, int FEAT>
__device__ __forceinline__ Masks<MAXC> shadow_masks(const PacketScene& S, bool casting_lane, d3 so,
                                                    d3 lcenter, double lrad, double bias) {
    const OriginBall B = origin_ball(casting_lane, so);
    return B.ok ? cull_capsule<MAXC, FEAT>(S, B.c, B.R, lcenter, lrad, bias)
                : all_candidates<MAXC>(S.ns);
}

// One light of directLightning (Scene.h:86-124) for the whole wave: every lane calls it
// (uniform control flow for the packet reductions); `active` lanes shade.
// TAB (packet_direct_kernel's kTab variants): `stab`, when set, points at this tile's and this
// light's word of the frame's shadow table (rt_shadow_table.hpp) — a superset of the spheres any
// shadow ray of the tile can meet, formed from the scene, the camera and the tile alone.  Masks
// only shrink by provable misses, so a superset mask leaves every lane's classification as it
// is.  The other instantiations compile to the code they had.
template <int MAXC, int FEAT, bool COUNT, bool TAB = false>
__device__ __forceinline__ void pk_light(const PacketScene& S, bool active, d3 P, d3 n, d3 view,
                                         const PkHit& h, d3 lpos, d3 E, d3 lcenter, double lrad,
                                         double bias, int nchunks, d3& diff, d3& spec,
                                         Counts& cnt, const Masks<MAXC>* pre = nullptr,
                                         bool* fix = nullptr,
                                         const unsigned long long* stab = nullptr) {
    double dist = 0.0, inv_d2 = 0.0;
    d3 L = mk(0.0, 0.0, 0.0);
    if (active) light_dir(lpos - P, dist, L, inv_d2);  // skipped by waves with no hit lane
    const bool reach = active && !(dist <= 0.0);
    if (!reach) L = mk(0.0, 0.0, 0.0);
    const double ndl = smax(0.0, dot(n, L));
    const bool need = reach && !(ndl <= 0.0) && !(dist <= bias);
    const d3 so = P + n * bias;
    const uint64_t casting = __ballot(need);
    if (!casting) return;  // no lane casts this shadow ray (uniform)
    // every lane stays in the code below until the march mask is formed (wave reductions);
    // lanes that cast no ray only take part in them
    int occ = 0;
    Masks<MAXC> M;
    bool tabled = false;
    if constexpr (TAB) {
        if (stab) {  // uniform: one scalar load; all ones: the tile has no word
            const unsigned long long w = *(pk_culp)stab;
            if (w != ~0ull) {
                M.m[0] = w;
                M.pm = ~0ull;
                tabled = true;
            }
        }
    }
    if (pre) {
        M = *pre;
        if (need) occ = pk_occlusion<MAXC, FEAT>(S, M, nchunks, so, L, dist - bias, bias);
    } else if (TAB && tabled) {
        if (need) occ = pk_occlusion<MAXC, FEAT>(S, M, nchunks, so, L, dist - bias, bias);
    } else {
        const OriginBall B = origin_ball(need, so);
        M = B.ok ? cull_capsule<MAXC, FEAT>(S, B.c, B.R, lcenter, lrad, bias)
                 : all_candidates<MAXC>(S.ns);
        bool split = false;
        if constexpr (kShadowSplit && MAXC > 1) {
            // A wide packet (origins straddling a depth edge: a sphere in front of a wall) gets a
            // fat capsule that keeps much of the scene, and every lane then classifies every
            // candidate: these waves run 10-35x the median and set the tail of a launch.  Such
            // a packet is split in two — the lanes within R/2 of the ball's centre and the rest —
            // each with its own ball and capsule (ANDed with the shared mask), and each group
            // walks only its own candidates.  Masks only shrink by provable misses, so every
            // lane's classification is unchanged.  The groups' capsules skip the plane cull
            // (they keep the shared one's plane mask: C3 -0.7 %).  8-rank row splits: slowest
            // rank C4 0.30 → 0.20 ms, C3 0.11 → 0.09 ms (with the march mask below); one whole
            // frame: C4 -1 %, C3 +1.2 %, C2/C5 ±0.5 % (tools/gpu_ab.sh, 3 interleaved rounds).
            int cand = 0;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) cand += __builtin_popcountll(M.m[c]);
            split = B.ok && cand > kShadowSplitMin;  // uniform
            if (split) {
                float r_lane = 0.0f;
                if (need) {
                    const float dx = static_cast<float>(so.x - B.c.x),
                                dy = static_cast<float>(so.y - B.c.y),
                                dz = static_cast<float>(so.z - B.c.z);
                    r_lane = sqrt_f32(dot3f(dx, dy, dz, dx, dy, dz));
                }
                const bool near = r_lane <= 0.5f * B.R;
                Masks<MAXC> Mn = M, Mf = M;
                const OriginBall Bn = origin_ball(need && near, so);
                const OriginBall Bf = origin_ball(need && !near, so);
                if (Bn.ok) {
                    const Masks<MAXC> t =
                        cull_capsule<MAXC, (FEAT & ~kFeatPlanes)>(S, Bn.c, Bn.R, lcenter, lrad, bias);
#pragma unroll
                    for (int c = 0; c < MAXC; ++c) Mn.m[c] &= t.m[c];
                    Mn.pm &= t.pm;
                }
                if (Bf.ok) {
                    const Masks<MAXC> t =
                        cull_capsule<MAXC, (FEAT & ~kFeatPlanes)>(S, Bf.c, Bf.R, lcenter, lrad, bias);
#pragma unroll
                    for (int c = 0; c < MAXC; ++c) Mf.m[c] &= t.m[c];
                    Mf.pm &= t.pm;
                }
#pragma unroll 1
                for (int g = 0; g < 2; ++g) {  // uniform: one group after the other
                    Masks<MAXC> Mg;
#pragma unroll
                    for (int c = 0; c < MAXC; ++c) Mg.m[c] = g == 0 ? Mn.m[c] : Mf.m[c];
                    Mg.pm = g == 0 ? Mn.pm : Mf.pm;
                    if (need && near == (g == 0))
                        occ = pk_occlusion<MAXC, FEAT>(S, Mg, nchunks, so, L, dist - bias, bias);
                }
            }
        }
        if (!split && need) occ = pk_occlusion<MAXC, FEAT>(S, M, nchunks, so, L, dist - bias, bias);
    }
    // The exact march (computeTransmittance) for the undecided lanes: a handful of lanes whose
    // shadow ray starts on or next to a surface, marching up to 64 closest-hit steps.  Over the
    // whole packet's mask such a march visits every candidate of a wide capsule at every step
    // (the slowest waves of C3 spend > 90 % of their time here), so it gets a capsule of its
    // own around the marching lanes' origins: every origin of the march lies on the segment
    // from its shadow-ray origin towards the light, inside that capsule, so the mask still
    // holds every sphere the march can hit.  C3's slowest waves 240 → 85 µs; its 8-rank
    // row split went from 1.37-1.45× the mean rank to 1.02-1.04× (profiles/r02_*).
    const bool undecided = need && occ == 2;
    double T = occ == 1 ? 0.0 : 1.0;
    if constexpr ((FEAT & kFeatFix) != 0) {
        // no march here: the pixel is queued for packet_fixup_kernel (its output is rewritten)
        if (undecided) *fix = true;
    } else if (__ballot(undecided)) {  // uniform
        Masks<MAXC> Mu = M;
        const OriginBall Bu = origin_ball(undecided, so);
        if (Bu.ok) {
            const Masks<MAXC> t = cull_capsule<MAXC, FEAT>(S, Bu.c, Bu.R, lcenter, lrad, bias);
#pragma unroll
            for (int c = 0; c < MAXC; ++c) Mu.m[c] &= t.m[c];
            Mu.pm &= t.pm;
        }
        if (undecided) T = pk_transmittance<MAXC, FEAT>(S, Mu, nchunks, so, L, dist - bias, bias);
    }
    if (!need) return;
    if (COUNT) cnt.shadow++;
    if (T <= bias) return;
    diff = diff + ((E * inv_d2) * ndl) * T;
    if constexpr ((FEAT & kFeatSpec) != 0) {
        const double* m = pk_material<MAXC>(S, h);
        if (m[5] <= 0.0 && m[4] > 0.0) {
            const d3 H = unit(L + view);
            const double ndh = smax(0.0, dot(n, H));
            if (ndh > 0.0) {
                const double sf = pow_bp(ndh, m[3]);
                spec = spec + ((E * inv_d2) * sf) * T;
            }
        }
    }
}

// Point light l's position and E = colour·intensity.  With <= 64 spheres (MAXC == 1) the record
// is read through the scalar cache: wave-uniform, so SGPRs instead of VGPRs, which is what lets
// C2's variant run at 6 waves/SIMD (RT_PACKET_SMALL_WAVES).  More spheres keep the LDS copy
// (C3 +1.2 % through the scalar cache: the chunk masks need those SGPRs).
template <int MAXC>
__device__ __forceinline__ void pk_light_record(const PacketScene& S, const TraceParams& P, int l,
                                                d3& L, d3& E) {
    if constexpr (MAXC == 1) {
        const pk_cdp q = (pk_cdp)P.lt + kLtStride * l;
        L = mk(q[0], q[1], q[2]);
        E = mk(q[3], q[4], q[5]);
    } else {
        const double* q = S.lt + kLtStride * l;
        L = mk(q[0], q[1], q[2]);
        E = mk(q[3], q[4], q[5]);
    }
}

// A uniform tile of the fix-up variant (class c = tile_class_of(cls) ≠ 0: tile_class_word,
// rt_shadow_table.hpp): every camera ray of the wave misses everything (kTileSky) or ends on the
// one plane k = c − kTilePlane0, and no shadow ray of the tile can meet a sphere.  The wave's
// scene is then that plane's record, oriented normal and material row, the np ≤ 2 plane records
// of the shadow classification and the light records: wave-uniform, read from the global packet
// image `img` (pk_build_image's layout, no chunk bounds: ns ≤ 63) and the scene through the
// scalar cache — no LDS image, no sphere, no mask, no divergence bookkeeping.  Every lane is
// active, the lanes past the image edge included (clamped rays of the tile's rectangle: the
// class holds for them; the epilogue stores and queues nothing for them).  Returns the pixel's
// colour with the bits of the general path, whose operations these are, in its order:
// closest_camera's plane loop ends on plane k with t = num / n·d formed with found = false
// (the class's ordering argument), the normal is s_pln's, pk_light runs with active = true and a
// table word of 0 (pk_occlusion_t<1, FEAT, false>: the plane loop over every plane, M.pm all
// ones), and the shading is the kernel's own.
// `cls` is the table's whole word: the class in its low byte and, per light, the planes the
// tile's shadow rays must still classify (shadow_plane_keep, rt_shadow_table.hpp: a plane it
// drops leaves the classification at a `continue` for every casting lane of the tile, so leaving
// it out changes neither `blocked` nor `undecided`).  A light whose mask is 0 — most of C2's:
// the kept plane lies behind its own shadow origins, the other one beyond the light — runs no
// classification and loads no `oth` record; all ones classifies every plane as before.
// SPH (packet_uniform_kernel<true>: a shadowed-plane tile, tile_shadowed_mark): the camera ray's
// claims are the same, but a shadow ray can meet a sphere.  `stab` points at the tile's shadow
// words, one per light (one scalar load each); a non-zero word first runs the sphere block of
// pk_occlusion_t<1, FEAT, true> over the word's bits — what pk_light runs on the general path with
// that word as its mask: the range test on 2a, rcp_refined and the per-sphere discriminant, roots
// and thresholds, the same expressions in the same order — with the sphere records read from the
// global image through the scalar cache (the loop is wave-uniform; the LDS image holds these
// values).  A 2a out of range returns "undecided" there before any plane is classified: here it
// sets `undecided` and skips both blocks, which leaves T = 1 and queues the pixel, as there.
// A zero word for a light is pk_occlusion_t<1, FEAT, false>: the code of the other form.
template <int MAXC, int FEAT, bool SPH = false>
__device__ __forceinline__ d3 pk_uniform_tile(const PacketScene& S, const TraceParams& P,
                                              const double* img, unsigned long long cls, d3 cam,
                                              d3 d, int ns, int np, int nl, double bias,
                                              bool& fix,
                                              const unsigned long long* stab = nullptr) {
    if (tile_class_of(cls) == kTileSky) return sky(d);
    const int k = static_cast<int>(tile_class_of(cls) - kTilePlane0);
    const pk_cdp pl = (pk_cdp)img + kPkSph * ns;
    const pk_cdp rec = pl + kPlStride * k;
    const pk_cdp on = pl + kPlStride * np + kLtStride * nl + 4 * k;
    const pk_cdp m = (pk_cdp)P.sph_mat + kMatStride * (ns + k);
    // The shadow classification's planes: the kept one and, with two planes, the other (np ≤ 2
    // where a class word exists: packet_shadow_table_lights).  Each plane sets `blocked` or
    // `undecided` by itself, so their order does not matter.
    const pk_cdp oth = pl + kPlStride * (np > 1 ? 1 - k : k);
    const d3 pp = mk(rec[0], rec[1], rec[2]), pn = mk(rec[3], rec[4], rec[5]);
    const double num = rec[6], core = rec[7];
    const d3 n = mk(on[0], on[1], on[2]);
    bool found = false;
    double t = 0.0;
    int prim = -1;
    const double denom = dot(pn, d);
    if (core != 0.0) plane_t_core(num, denom, ns + k, found, t, prim);  // uniform
    else plane_t(num, denom, ns + k, found, t, prim);
    const d3 hp = cam + d * t;
    d3 diff = mk(0.0, 0.0, 0.0);
    const d3 spec = mk(0.0, 0.0, 0.0);  // (no Blinn-Phong in this variant)
    for (int l = 0; l < nl; ++l) {
        d3 lpos, E;
        pk_light_record<MAXC>(S, P, l, lpos, E);
        // pk_light, active
        double dist = 0.0, inv_d2 = 0.0;
        d3 L = mk(0.0, 0.0, 0.0);
        light_dir(lpos - hp, dist, L, inv_d2);
        const bool reach = !(dist <= 0.0);
        if (!reach) L = mk(0.0, 0.0, 0.0);
        const double ndl = smax(0.0, dot(n, L));
        const bool need = reach && !(ndl <= 0.0) && !(dist <= bias);
        const d3 so = hp + n * bias;
        if (!__ballot(need)) continue;  // no lane casts this shadow ray (uniform)
        // pk_occlusion_t<1, FEAT, false>'s plane classification, every plane the tile's mask
        // for this light keeps (uniform: scalar branches)
        bool blocked = false, undecided = false;
        const unsigned keep = tile_plane_keep(cls, l);
        bool planes = true;  // (SPH: false for a lane whose 2a is out of range)
        if constexpr (SPH) {
            // pk_occlusion_t<1, FEAT, true>'s sphere block over this light's word (uniform)
            const unsigned long long w = *(pk_culp)(stab + l);
            if (w != 0 && need) {
                const double max_dist = dist - bias;
                const double a = dot(L, L);
                const double two_a = 2.0 * a, four_a = 4.0 * a;
                if (!(two_a >= 0x1p-100 && two_a <= 0x1p100)) {
                    undecided = true;
                    planes = false;
                } else {
                    const double inv2a = rcp_refined(two_a);
                    uint64_t m = w;
                    while (m) {
                        const int i = __builtin_ctzll(m);
                        m &= m - 1;
                        const pk_cdp s = (pk_cdp)img + kPkSph * i;
                        const d3 oc = so - mk(s[0], s[1], s[2]);
                        const double b = 2.0 * dot(oc, L);
                        const double cc = dot(oc, oc) - s[3];
                        const double disc = b * b - four_a * cc;
                        if (disc < 0.0) continue;
                        if (!(disc == 0.0 || (disc > 1e-30 && disc < 1e30))) {
                            undecided = true;
                            continue;
                        }
                        const double sq = static_cast<double>(sqrt_f32(static_cast<float>(disc)));
                        const double delta = 2e-6 * (fabs(b) + sq) * inv2a;
                        double ts = (-b - sq) * inv2a;
                        if (!(ts >= 1e-6 + delta)) {
                            if (!(ts < 1e-6 - delta)) {
                                undecided = true;
                                continue;
                            }
                            ts = (-b + sq) * inv2a;
                            if (ts < 1e-6 - delta) continue;
                            if (!(ts >= 1e-6 + delta)) {
                                undecided = true;
                                continue;
                            }
                        }
                        if (ts >= max_dist + delta) continue;
                        if (ts > bias + delta && ts < max_dist - delta) blocked = true;
                        else undecided = true;
                    }
                }
            }
        }
        if (keep != 0 && need && planes) {
            const double max_dist = dist - bias;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (i >= np) break;
                if (((keep >> (i == 0 ? k : 1 - k)) & 1u) == 0) continue;
                const d3 qp = i == 0 ? pp : mk(oth[0], oth[1], oth[2]);
                const d3 qn = i == 0 ? pn : mk(oth[3], oth[4], oth[5]);
                const double dn = dot(qn, L);
                if (!(fabs(dn) > 1e-6)) continue;
                const double nm = dot(qp - so, qn);
                const double A = dn > 0.0 ? nm : -nm, B = fabs(dn);
                if (A < -1e-300 * B) continue;
                if (A >= max_dist * B * (1.0 + 1e-9)) continue;
                if (A > bias * B * (1.0 + 1e-9) && A < max_dist * B * (1.0 - 1e-9)) blocked = true;
                else undecided = true;
            }
        }
        const double T = (!undecided && blocked) ? 0.0 : 1.0;
        // no march here: the pixel is queued for packet_fixup_kernel (its output is rewritten)
        if (undecided) fix = true;
        if (!need) continue;
        if (T <= bias) continue;
        diff = diff + ((E * inv_d2) * ndl) * T;
    }
    const d3 local = hmul(mk(m[0], m[1], m[2]), diff) + spec * m[4];
    const double tr = sclamp(m[5], 0.0, 1.0);
    d3 fin = mk(0.0, 0.0, 0.0);
    if (tr < 1.0) fin = fin + local * (1.0 - tr);
    return fin;
}

// Waves per SIMD of a variant (its register budget).
constexpr int pk_waves(int MAXC, int FEAT, bool COUNT, bool MULTI) {
    return (FEAT == (kFeatFix | kFeatSplit) && MAXC == 1 && !MULTI && !COUNT)
               ? RT_PACKET_GENERAL_WAVES
         : (FEAT == kFeatFix && MAXC == 1 && !MULTI && !COUNT) ? RT_PACKET_FIX_WAVES
         : (FEAT == 0 && MAXC == 1 && !MULTI && !COUNT) ? RT_PACKET_SMALL_WAVES
         : (FEAT == (kFeatArea | kFeatNoPL) && !MULTI && !COUNT) ? RT_PACKET_AREA_WAVES
         : FEAT == kFeatTris ? RT_PACKET_TRIS_WAVES
         : (((FEAT == 0 || (FEAT & ~kFeatNoPL) == kFeatArea || FEAT == kFeatPlanes) && MAXC <= 4)
                ? (MULTI ? (FEAT == 0 ? RT_PACKET_LEAN_WAVES : 1) : RT_PACKET_AA1_WAVES)
                : 1);
}
// FEAT_ = kFeatFix | kFeatSplit is the fix-up variant's split launch (rt_packet.hip
// launch_packet_split): the launch is a row of workgroups per frame, workgroup blockIdx.x renders
// the blockIdx.x-th entry of the frame's list of general workgroups (rt_shadow_table.hpp, after
// the frame's class words) and returns at once past the list's count; a wave whose tile is
// uniform takes part in the staging and its barrier and returns — packet_uniform_kernel renders
// that tile — so pk_uniform_tile is not compiled into this launch.  The bit is taken off FEAT,
// so the body reads as it did and every other instantiation keeps its name and its code.
template <int MAXC, int FEAT_, bool COUNT, bool MULTI, int WGY>  // MULTI = false: one sample (AA = 1)
__global__ __launch_bounds__(64 * kWgWavesX * WGY, pk_waves(MAXC, FEAT_, COUNT, MULTI)) void packet_direct_kernel(TraceParams P) {
    constexpr int FEAT = FEAT_ & ~kFeatSplit;
    constexpr bool SPLIT = (FEAT_ & kFeatSplit) != 0;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x;
    constexpr bool kNoPL = (FEAT & kFeatNoPL) != 0;  // the launcher checked P.np == P.nl == 0
    // The tile this workgroup renders.  Results do not depend on the order; the tail of the
    // launch does.  Default: rows bottom-up (scenes lit from above put the shadow-ray work on
    // the floor and little on the sky / back wall, so the cheap top rows fill the partly idle
    // end: C3 -9 %, C5 -1 %, C2/C4 within ±1 %; centre-out and edges-in orders measured worse).
    // With a tile order (costliest first, from the wave durations of an earlier launch of this
    // scene, camera and shape: packet_order_kernel) the cheapest tiles fill the end instead.
    const uint32_t lin = blockIdx.y * gridDim.x + blockIdx.x;  // dispatch position
    uint32_t tbx = blockIdx.x, tby = gridDim.y - 1 - blockIdx.y;
    // the tile grid's workgroups per row (tables are indexed by tile, not by dispatch position)
    // (the split launch's grid is not the tile grid: the launch shape's, packet_grid)
    const uint32_t gxw = SPLIT ? (P.width + kPkW * kWgWavesX - 1) / (kPkW * kWgWavesX) : gridDim.x;
    if constexpr (!SPLIT) {
        if (P.tile_order) {
            const uint32_t t = P.tile_order[lin];
            tbx = t % gridDim.x;
            tby = t / gridDim.x;
        }
    }
    // the recording launch (the general variant, rt_packet_host.cpp tile_order): each wave's start
    uint64_t t_start = 0;
    if constexpr (MULTI)
        if (P.tile_cost) t_start = __builtin_amdgcn_s_memrealtime();
    const int ns = P.ns, np = kNoPL ? 0 : P.np, nl = kNoPL ? 0 : P.nl, nb = pk_chunk_bounds(ns),
              nsb = ns + nb;
    // (the image layout: pk_build_image, rt_packet_device.hpp, is the format's definition)
    double* s_sph = smem;                                         // 80·nsb bytes
    double* s_pl = s_sph + kPkSph * nsb;
    double* s_lt = s_pl + kPlStride * np;
    double* s_pln = s_lt + kLtStride * nl;                        // 4·np doubles
    const int32_t* s_orig = reinterpret_cast<const int32_t*>(s_pln + 4 * np);
    // The frame: one per launch, or frame blockIdx.z of a batch (rt_render_batch) with its own
    // camera and image source (scalar loads from the kernel arguments).
    const double* camp = P.cam_pos;
    const double* pk_img = P.pk_image;
    unsigned long long* pk_pub = P.pk_pub;
    uint32_t pk_epoch = P.pk_epoch;
    uint64_t frame_off = 0;
    // The variants of up to 64 spheres without an area light (C2's) read the camera ray's frame
    // constants from the host; closest_camera and pk_occlusion skip empty sphere masks for the
    // same variants.  The others stay as they are: C5's runs at the edge of its register budget
    // (the plane-only copy of pk_occlusion alone put 8 B more per lane into scratch), and the
    // variants of more than 64 spheres lost time with such branches before.
    constexpr bool kLean = MAXC == 1 && (FEAT & kFeatArea) == 0;
    // The single-sample variants of that kind without another feature (C2's two) read their
    // camera-cone mask from the frame's table when it has one (rt_cone_table.hpp): a
    // wave-uniform run-time test of the pointer, so the variants keep their names.
    constexpr bool kTab = kLean && !MULTI && !COUNT && (FEAT == 0 || FEAT == kFeatFix);
    const unsigned long long* cone_tab = kTab ? P.cone_tab : nullptr;
    const unsigned long long* shadow_tab = kTab ? P.shadow_tab : nullptr;
    // The fix-up variant of those also reads the tiles' class words (pk_uniform_tile).  The
    // marching variant does not: its undecided lanes march over the LDS image, so it would have
    // to keep the staging, and it stays on the general path as it is.
    constexpr bool kUni = kTab && FEAT == kFeatFix && !SPLIT;
    const unsigned long long* class_tab = (kUni || SPLIT) ? P.class_tab : nullptr;
    double cam_dz = P.cam_dz, cam_dz2 = P.cam_dz2;
    if (P.nframes) {
        const PkFrame& F = P.fr[blockIdx.z];
        camp = F.cam;
        cam_dz = P.fr_dz[blockIdx.z][0];
        cam_dz2 = P.fr_dz[blockIdx.z][1];
        pk_img = F.img;
        pk_pub = F.pub;
        pk_epoch = F.epoch;
        frame_off = static_cast<uint64_t>(blockIdx.z) * P.frame_px;
        if constexpr (kTab) {
            cone_tab = P.fr_tab[blockIdx.z];
            shadow_tab = P.fr_stab[blockIdx.z];
        }
        if constexpr (kUni || SPLIT) class_tab = P.fr_ctab[blockIdx.z];
    }
    if constexpr (SPLIT) {
        // this workgroup's entry of the frame's general list (the launcher checked that every
        // frame has class words and lists); past the count: nothing to render (uniform)
        const uint32_t split_wgs = gxw * ((P.rows + kPkH * WGY - 1) / (kPkH * WGY));
        const TileTabLayout::Lists L{split_wgs * (kWgWavesX * WGY), split_wgs};
        const pk_culp hdr = (pk_culp)class_tab + L.after_cls();
        if (lin >= tile_list_counts(hdr[L.counts()], 0ull).general) return;
        const uint32_t t = ((pk_cip)(hdr + L.general_base()))[lin];
        tbx = t % gxw;
        tby = t / gxw;
    }
    const d3 cam = mk(camp[0], camp[1], camp[2]);
    constexpr int kThreads = 64 * kWgWavesX * WGY;
    // This wave's class word (class field 0: the general path; the bits above it are the
    // lights' shadow-plane keep masks) and whether the workgroup stages the image:
    // every wave reads the adjacent words of all the workgroup's waves (one scalar load) and
    // forms the same test, so the barrier count stays uniform; a workgroup of uniform waves
    // reads no LDS afterwards (pk_uniform_tile, the epilogue) and skips the copy and its barrier.
    unsigned long long cls = kTileGeneral;
    bool staged = true;
    if constexpr (kUni) {
        if (class_tab && pk_img && P.max_rec > 0) {
            const pk_culp cw =
                (pk_culp)class_tab + (tby * gxw + tbx) * (kWgWavesX * WGY);
            const uint32_t w = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(tid >> 6));
            bool all = true;
#pragma unroll
            for (uint32_t i = 0; i < kWgWavesX * WGY; ++i) {
                const unsigned long long c = cw[i];
                all = all && tile_class_of(c) != kTileGeneral;
                if (i == w) cls = c;
            }
            staged = !all;
        }
    }
    if constexpr (SPLIT) {
        // a listed workgroup has a general wave, so it stages; this wave's own word says
        // whether it goes on after the barrier
        const uint32_t w = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(tid >> 6));
        cls = ((pk_culp)class_tab)[(tby * gxw + tbx) * (kWgWavesX * WGY) + w];
    }
    if (pk_img && staged) {  // the image of this scene and camera, formed once (packet_image_kernel)
        const float4* src = reinterpret_cast<const float4*>(pk_img);
        float4* dst = reinterpret_cast<float4*>(smem);
        const int nv = static_cast<int>(pk_image_bytes(ns, np, nl) / 16);
        for (int i = tid; i < nv; i += kThreads) dst[i] = src[i];
        __syncthreads();
        if constexpr (SPLIT)
            // packet_uniform_kernel's tile: uniform, or marked shadowed-plane (a table formed
            // without the third list carries no mark)
            if (tile_class_of(cls) != kTileGeneral || (cls & kTileShadowedBit) != 0) return;
    } else if (pk_img) {
        // (a workgroup of uniform tiles: no image in LDS)
    } else if (pk_pub) {
        // A camera without a cached image: the launch's first workgroup forms the image and
        // publishes it as {epoch, word} granules (8-byte agent-scope atomic stores, written
        // through to memory: the tag travels with its word, so no flag and no fence).  The
        // workgroups of the first resident round (linear index < pk_pub_first) form their own
        // and never read the slot, so no XCD's L2 holds a line of it from before the publish;
        // a later workgroup reads the granules with relaxed agent-scope 8-byte atomic loads
        // (each {epoch, word} read whole, as written) and copies them when every tag is this
        // launch's epoch.  A granule with this epoch can only hold this launch's word, so a
        // stale or half-published slot just means "form it".
        uint32_t* dst = reinterpret_cast<uint32_t*>(smem);
        const int nw = static_cast<int>(pk_image_bytes(ns, np, nl) / 4);  // a multiple of 4
        const uint32_t ep = pk_epoch;
        const uint32_t wg = lin;  // in its frame: a batch's frames dispatch one after another
        bool have = false;
        if (wg >= P.pk_pub_first) {
            int ok = 1;
            for (int i = tid; i < nw / 2; i += kThreads) {
                const unsigned long long gx = __hip_atomic_load(
                    pk_pub + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long gy = __hip_atomic_load(
                    pk_pub + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok &= static_cast<uint32_t>(gx >> 32) == ep && static_cast<uint32_t>(gy >> 32) == ep;
                dst[2 * i] = static_cast<uint32_t>(gx);
                dst[2 * i + 1] = static_cast<uint32_t>(gy);
            }
            have = __syncthreads_and(ok) != 0;
        }
        if (!have) {
            pk_build_image(P, camp, smem, tid, kThreads);
            __syncthreads();
            if (wg == 0) {
                const unsigned long long tag = static_cast<unsigned long long>(ep) << 32;
                for (int i = tid; i < nw; i += kThreads)
                    __hip_atomic_store(pk_pub + i, tag | dst[i], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    } else {
        pk_build_image(P, camp, smem, tid, kThreads);
        __syncthreads();
    }

    PacketScene S;
    S.sph = s_sph;
    S.pl = s_pl;
    S.lt = s_lt;
    S.tri = P.tri;
    S.mat = P.sph_mat;
    S.bvh = P.bvh;
    S.bvh_tri = P.bvh_tri;
    S.ns = ns;
    S.np = np;
    S.nt = P.nt;
    S.nl = nl;
    S.nb = nb;
    S.orig = nb ? s_orig : nullptr;
    S.wstk = nullptr;
    if constexpr ((FEAT & kFeatTris) != 0)  // after the image: 64 ints per wave
        S.wstk = reinterpret_cast<int*>(smem + pk_image_bytes(ns, np, nl) / 8) +
                 kPkStack * (tid >> 6);
    const int nchunks = (ns + 63) / 64;

    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t x = tbx * (kPkW * kWgWavesX) + (wave % kWgWavesX) * kPkW + (lane % kPkW);
    const uint32_t yl = tby * (kPkH * WGY) + (wave / kWgWavesX) * kPkH + (lane / kPkW);
    const bool valid = x < P.width && yl < P.rows;
    // lanes past the image edge trace a clamped in-image ray: they take part in the packet
    // reductions (a superset bound is still conservative) and write nothing.
    const uint32_t xc = x < P.width ? x : P.width - 1;
    const uint32_t y = image_row(P, yl < P.rows ? yl : P.rows - 1);
    const uint64_t pix = static_cast<uint64_t>(y) * P.width + xc;
    const double bias = P.bias;
    d3 al_c = mk(0.0, 0.0, 0.0);
    double al_r = 0.0;
    if constexpr ((FEAT & kFeatArea) != 0) {
        const d3 eu = mk(P.al_u[0], P.al_u[1], P.al_u[2]);
        const d3 ev = mk(P.al_v[0], P.al_v[1], P.al_v[2]);
        al_c = (mk(P.al_corner[0], P.al_corner[1], P.al_corner[2]) + eu * 0.5) + ev * 0.5;
        al_r = (0.5 * (length(eu) + length(ev))) * (1.0 + kCullRel);
    }
    Counts cnt{0u, 0u};
    bool fix = false;  // kFeatFix: an undecided shadow ray, the pixel goes to the fix-up

    d3 acc = mk(0.0, 0.0, 0.0);
    int samples = 0;
    const int nsamples = MULTI ? P.aa : 1;
    for (int s = 0; s < nsamples; ++s) {
        // Camera::getRay (Math.h:99-121).  W/2, H/2, dz = (cam.z + focal) − cam.z and dz·dz are
        // the same for every pixel of the frame: the host forms them (camera_consts, the same
        // IEEE operations) and they arrive as scalar loads.  FP64 has no scalar ALU here: formed
        // in the kernel, every lane of every wave converts, halves, adds and squares them.
        // The other variants keep camera_dir's expression (the same bits): kLean.
        d3 d;
        if constexpr (kLean) {
            double sx = static_cast<double>(xc) - P.half_w;
            double sy = P.half_h - static_cast<double>(y);
            // Single sample: the reference adds jx = jy = 0.0.  sx and sy are differences of
            // finite values, and x − x is +0, never −0, so v + 0.0 == v bit for bit: no adds.
            if constexpr (MULTI) {
                double jx = 0.0, jy = 0.0;
                if (s > 0 && P.aa > 1) {
                    jx = u01(P.seed, pix, static_cast<uint32_t>(s), 0u);
                    jy = u01(P.seed, pix, static_cast<uint32_t>(s), 1u);
                }
                sx += jx;
                sy += jy;
            }
            const d3 dv = mk(sx - cam.x, sy - cam.y, cam_dz);
            d = unit_sq(dv, dv.x * dv.x + dv.y * dv.y + cam_dz2);
        } else {
            d = camera_dir(P, cam, xc, y, pix, s);
        }

        d3 col;
        if (P.max_rec <= 0) {
            col = sky(d);  // TraceRay at depth >= maxRecursion (Scene.h:132-134)
        } else if (kUni && tile_class_of(cls) != kTileGeneral) {
            // uniform (cls is only set with max_rec > 0)
            if constexpr (kUni)
                col = pk_uniform_tile<MAXC, FEAT>(S, P, pk_img, cls, cam, d, ns, np, nl, bias, fix);
        } else {
            if (COUNT && valid) cnt.trace++;
            // (a lambda: the variants without a table compile to the code they had)
            const Masks<MAXC> M = [&] {
                if constexpr (kTab) {
                    if (cone_tab) {  // uniform: this tile's mask, one scalar load
                        Masks<MAXC> T;
                        const uint32_t w =
                            __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave));
                        T.m[0] = ((pk_culp)cone_tab)[(tby * gxw + tbx) * (kWgWavesX * WGY) + w];
                        T.pm = ~0ull;
                        return T;
                    }
                }
                // camera cone: axis = the tile's centre-lane direction (exact copy), half-angle
                // from the wave minimum of the per-lane cosines in FP32 (|cos| ≤ 1 + 2ε, so the
                // conversion is off by ≤ 6e-8, inside the 1e-7 taken off)
                const d3 axis = lane_d3(d, (kPkH / 2) * kPkW + kPkW / 2);
                const double cos_min =
                    static_cast<double>(wave_red<0>(static_cast<float>(dot(d, axis)))) - 1e-7;
                const bool ok = isfinite(cos_min) && cos_min > 0.0;  // cones narrower than 90°
                return ok ? cull_cone<MAXC>(S, axis, cos_min) : all_candidates<MAXC>(ns);
            }();
            PkHit h;
            h.t = 0.0;
            h.prim = 0;
            const bool hit = valid && closest_camera<MAXC, FEAT>(S, M, nchunks, cam, d, h);
            // shading inputs (Scene.h:147-154); misses carry harmless placeholders
            const d3 hp = cam + d * h.t;
            // `view` is only read by the Blinn-Phong term.
            d3 view = mk(0.0, 0.0, 0.0);
            d3 inc = mk(0.0, 0.0, 0.0);
            if constexpr ((FEAT & kFeatSpec) != 0) {
                inc = unit(d);
                view = -inc;
            }
            // planes: the frame-constant oriented normal of the prologue (s_pln); misses: unused
            d3 n = mk(0.0, 1.0, 0.0);
            bool known = !hit;
            if (hit && h.prim >= ns && h.prim < ns + np) {
                const double* q = s_pln + 4 * (h.prim - ns);
                if (q[3] != 0.0) {
                    n = mk(q[0], q[1], q[2]);
                    known = true;
                }
            }
            if (!known) {
                const d3 gn = pk_normal(S, h, hp);
                // frontFace = n·normalize(d) < 0 (Scene.h:148-150).  d is a unit vector (or
                // zero), so normalize(d) = d/l·(1+δ) with l = 1 ± 4ε and |δ| ≤ ε; both dot
                // products are within 5ε·S of their exact values, S = Σ|n_i·d_i| — when
                // |n·d| > 1e-14·S they have the same sign, and the second normalize (3
                // divisions) is only needed otherwise.
                bool front;
                if constexpr ((FEAT & kFeatSpec) != 0) {
                    front = dot(gn, inc) < 0.0;
                } else {
                    const double nd = dot(gn, d);
                    const double sabs = fabs(gn.x * d.x) + fabs(gn.y * d.y) + fabs(gn.z * d.z);
                    if (fabs(nd) > 1e-14 * sabs && sabs > 1e-200) front = nd < 0.0;
                    else front = dot(gn, unit(d)) < 0.0;
                }
                const d3 n0 = front ? gn : -gn;
                n = unit(n0);  // directLightning's own normalize (Scene.h:81)
            }
            d3 diff = mk(0.0, 0.0, 0.0), spec = mk(0.0, 0.0, 0.0);
            // The shading point and normal stay in registers across both light loops.  Parking
            // them in LDS (6 doubles per lane) in the ≤ 64-sphere variants cut the spills (C5
            // 116 → 44 B/lane, C2 44 → 12) but the reloads cost more: C5 414 → 434 µs, C2
            // 38.3 → 38.9 µs per frame (profiles/r04_ab_park.txt, r04_park_traffic.json).
            if constexpr (kTab) {
                // this tile's shadow-table words, one per light (a uniform address)
                const unsigned long long* stab = nullptr;
                if (shadow_tab) {
                    const uint32_t w =
                        __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave));
                    stab = shadow_tab + static_cast<size_t>(
                               (tby * gxw + tbx) * (kWgWavesX * WGY) + w) * nl;
                }
                for (int l = 0; l < nl; ++l) {
                    d3 L, E;
                    pk_light_record<MAXC>(S, P, l, L, E);
                    pk_light<MAXC, FEAT, COUNT, true>(S, hit, hp, n, view, h, L, E, L, 0.0, bias,
                                                      nchunks, diff, spec, cnt, nullptr, &fix,
                                                      stab ? stab + l : nullptr);
                }
            } else {
                for (int l = 0; l < nl; ++l) {
                    d3 L, E;
                    pk_light_record<MAXC>(S, P, l, L, E);
                    pk_light<MAXC, FEAT, COUNT>(S, hit, hp, n, view, h, L, E, L, 0.0, bias,
                                                nchunks, diff, spec, cnt, nullptr, &fix);
                }
            }
            if constexpr ((FEAT & kFeatArea) != 0) {
                if (P.al_samples > 0) {
                    const uint32_t stream = 0x10000u + (static_cast<uint32_t>(s) << 6);
                    const double k = static_cast<double>(P.al_k);
                    const d3 corner = mk(P.al_corner[0], P.al_corner[1], P.al_corner[2]);
                    const d3 eu = mk(P.al_u[0], P.al_u[1], P.al_u[2]);
                    const d3 ev = mk(P.al_v[0], P.al_v[1], P.al_v[2]);
                    const d3 E = mk(P.al_E[0], P.al_E[1], P.al_E[2]);
                    // one packet cull for all samples: every sample's casting lanes are hit
                    // lanes with this origin, and every sample point is in (al_c, al_r)
                    const OriginBall B = origin_ball(hit, hp + n * bias);
                    const Masks<MAXC> Ma = B.ok ? cull_capsule<MAXC, FEAT>(S, B.c, B.R, al_c, al_r, bias)
                                                : all_candidates<MAXC>(ns);
                    // When that leaves many candidates (a wide light seen past many spheres),
                    // each sample gets its own capsule: sample q lies in stratum cell
                    // (q mod k, q div k), a parallelogram of half-diagonal ≤ (|u|+|v|)/2k
                    // around the cell centre (plus an absolute term for the rounding of the
                    // sample and centre positions); its mask is ANDed with the shared one.
                    int cand = 0;
#pragma unroll
                    for (int c = 0; c < MAXC; ++c) cand += __builtin_popcountll(Ma.m[c]);
                    const bool per_cell = B.ok && cand > 4;
                    const double cell_r =
                        ((0.5 * (length(eu) + length(ev))) / k) * (1.0 + kCullRel) +
                        1e-12 * (fabs(corner.x) + fabs(corner.y) + fabs(corner.z) + fabs(eu.x) +
                                 fabs(eu.y) + fabs(eu.z) + fabs(ev.x) + fabs(ev.y) + fabs(ev.z));
                    // the stratum coordinates x / k as div_core with k's refined reciprocal (the
                    // correctly rounded quotient, rt_device.hpp: 0 ≤ x < k + 1, k ≤ 2^31)
                    const double rk = rcp_refined(k);
                    for (int q = 0; q < P.al_samples; ++q) {
                        const double r1 = u01(P.seed, pix, stream, 2u * static_cast<uint32_t>(q));
                        const double r2 =
                            u01(P.seed, pix, stream, 2u * static_cast<uint32_t>(q) + 1u);
                        const double fu = div_core(static_cast<double>(q % P.al_k) + r1, k, rk);
                        const double fv = div_core(static_cast<double>(q / P.al_k) + r2, k, rk);
                        const d3 lpos = (corner + eu * fu) + ev * fv;
                        Masks<MAXC> Mq = Ma;
                        if (per_cell) {  // uniform
                            const double cu = div_core(static_cast<double>(q % P.al_k) + 0.5, k, rk);
                            const double cv = div_core(static_cast<double>(q / P.al_k) + 0.5, k, rk);
                            const Masks<MAXC> Mc = cull_capsule<MAXC, FEAT>(
                                S, B.c, B.R, (corner + eu * cu) + ev * cv, cell_r, bias);
#pragma unroll
                            for (int c = 0; c < MAXC; ++c) Mq.m[c] &= Mc.m[c];
                            Mq.pm &= Mc.pm;
                        }
                        pk_light<MAXC, FEAT, COUNT>(S, hit, hp, n, view, h, lpos, E, al_c, al_r,
                                                    bias, nchunks, diff, spec, cnt, &Mq);
                    }
                }
            }
            if (hit) {
                const double* m = pk_material<MAXC>(S, h);
                const d3 local = hmul(mk(m[0], m[1], m[2]), diff) + spec * m[4];
                const double tr = sclamp(m[5], 0.0, 1.0);
                d3 fin = mk(0.0, 0.0, 0.0);
                if (tr < 1.0) fin = fin + local * (1.0 - tr);
                col = fin;
            } else {
                col = sky(d);
            }
        }
        acc = acc + col;
        samples += 1;
    }
    // The pixel again, from the lane id (mbcnt) and the workgroup's tile (scalars): keeping x /
    // yl live across the trace cost the single-sample variants a spilled dword per lane, whose
    // scratch write-back was most of C2's HBM traffic beyond the framebuffer (12 MB per frame).
    const uint32_t lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t wave_e = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave));
    const uint32_t x_e = tbx * (kPkW * kWgWavesX) + (wave_e % kWgWavesX) * kPkW + (lane_e % kPkW);
    const uint32_t yl_e = tby * (kPkH * WGY) + (wave_e / kWgWavesX) * kPkH + (lane_e / kPkW);
#include "rt_packet_epilogue.hpp"
    if constexpr (COUNT) {
        uint32_t t = cnt.trace, sh = cnt.shadow;
        for (int off = 32; off > 0; off >>= 1) {
            t += __shfl_xor(t, off, 64);
            sh += __shfl_xor(sh, off, 64);
        }
        if (lane == 0) {
            atomicAdd(P.counters + 0, static_cast<unsigned long long>(t));
            atomicAdd(P.counters + 1, static_cast<unsigned long long>(sh));
        }
    }
    if constexpr (MULTI) {
        // this wave's duration (100 MHz wall clock), per tile (a batch records its first frame)
        if (P.tile_cost && lane == 0 && blockIdx.z == 0) {
            const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
            P.tile_cost[(tby * gridDim.x + tbx) * (kWgWavesX * WGY) + wave] =
                static_cast<uint32_t>(t_end - t_start);
        }
    }
}

template <int MAXC, int FEAT, int WGY>
static void launch_packet_shape(const TraceParams& p, bool count, size_t lds, hipStream_t stream) {
    const dim3 block(64 * kWgWavesX * WGY);
    const dim3 grid((p.width + kPkW * kWgWavesX - 1) / (kPkW * kWgWavesX),
                    (p.rows + kPkH * WGY - 1) / (kPkH * WGY), p.nframes ? p.nframes : 1u);
    // the single-sample variant keeps no accumulator live across the trace (AA = 1, the
    // reference default for a preview and the bench's configuration); counting passes use the
    // general one
    // (a launch that records its wave durations for the tile order takes the general variant:
    // the single-sample one carries no recording code)
    if constexpr ((FEAT & kFeatTris) != 0) lds += sizeof(int) * kPkStack * (block.x / 64);
    if (count) hipLaunchKernelGGL((packet_direct_kernel<MAXC, FEAT, true, true, WGY>), grid, block, lds, stream, p);
    else if (p.aa == 1 && !p.tile_cost) hipLaunchKernelGGL((packet_direct_kernel<MAXC, FEAT, false, false, WGY>), grid, block, lds, stream, p);
    else hipLaunchKernelGGL((packet_direct_kernel<MAXC, FEAT, false, true, WGY>), grid, block, lds, stream, p);
}

template <int MAXC, int FEAT>
static void launch_packet_variant(const TraceParams& p, bool count, size_t lds, hipStream_t stream) {
    if (pk_wgy(lds) == 1) launch_packet_shape<MAXC, FEAT, 1>(p, count, lds, stream);
    else launch_packet_shape<MAXC, FEAT, 2>(p, count, lds, stream);
}

// rt_packet_area.hip, called by launch_packet_direct (rt_packet.hip) for feat == kFeatArea
hipError_t launch_packet_area(const TraceParams& p, bool count, size_t lds, int chunks,
                              hipStream_t stream);

}  // namespace rtamd
