// walk_main.cpp — stand-alone host check of the three triangle-BVH traversals against the ordered
// loop over all triangles, built and run by tests/test_bvh_walk_host.py with the real builder
// (csrc/rt_bvh.cpp) and the C oracle's Triangle::Intersect (oracle/rt_oracle.c).  The traversals
// are device code; they are restated here line for line, each under a comment naming its source,
// and the GPU tests (tests/test_gpu_mesh_packet.py, tests/test_gpu_ray_queries.py) bind the
// shipped code to the same answers.  This program checks the design's claims at a volume no GPU
// test of a few seconds reaches.
//
//   walk_main prop SEED CASES [--mutate M] [FILE...]
//       CASES random meshes of 32..2000 triangles, and every FILE (a crafted mesh with its camera
//       and lights, tests/mesh_sets.py hex_scene): packets of 64 rays from one origin through an
//       8x8 pixel tile, packets of unrelated rays, packets with a random subset of active lanes,
//       packets with a hit to beat, and the shadow rays of a tile's hits.  Every walk must return
//       exactly the (t, index) of the ordered loop with the strict '<' merge; the any-hit walk
//       the loop's answer for distances at, just below and just above the closest t.
//   walk_main depth PKSTACK FILE
//       FILE's mesh and two random ones: the tree's depth is <= 48, the largest stack pointer of
//       any walk is <= depth + 1 and below kBvhStack and PKSTACK (kPkStack, which a host program
//       cannot include: the test reads it from csrc/rt_packet_device.hpp), and the camera's
//       d.x == 0 column reaches the deepest leaf the tree has.
//   M: notie (the wave walk without its 'i < ti' rule), nomargin (it prunes at tn > bound, without
//      the 1e-9), nowiden (node boxes rebuilt without the builder's widening): each must make the
//      program fail — the checks are not vacuous.
// Exit status 0 only when every property holds.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_internal.hpp"
#include "rt_oracle.h"

using namespace rtamd;

static_assert(kBvhStack >= 48 + 2, "a tree of depth 48 takes 49 stack entries");

enum Mutation { kNone, kNoTie, kNoMargin, kNoWiden };
static Mutation g_mut = kNone;

struct Rng {
    uint64_t s;
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double u(double lo, double hi) { return lo + (hi - lo) * ((next() >> 11) * 0x1p-53); }
    uint32_t below(uint32_t n) { return static_cast<uint32_t>(next() % n); }
};

struct V3 {
    double x, y, z;
};

struct Mesh {
    std::vector<o_triangle> tris;
    std::vector<double> nodes;
    std::vector<int32_t> order;
    int depth = 0;

    void node(int n, int& first, int& count, int& axis) const {
        int32_t fc[2], ax[2];
        std::memcpy(fc, &nodes[size_t(kBvhNodeStride) * n + 6], sizeof fc);
        std::memcpy(ax, &nodes[size_t(kBvhNodeStride) * n + 7], sizeof ax);
        first = fc[0];
        count = fc[1];
        axis = ax[0];
    }
    int depth_of(int n) const {
        int first, count, axis;
        node(n, first, count, axis);
        return count > 0 ? 0 : 1 + std::max(depth_of(first), depth_of(first + 1));
    }
    // kNoWiden: every node's box becomes the exact bounds of its triangles' vertices
    void tighten(int n, double* lo, double* hi) {
        int first, count, axis;
        node(n, first, count, axis);
        for (int k = 0; k < 3; ++k) {
            lo[k] = INFINITY;
            hi[k] = -INFINITY;
        }
        if (count > 0) {
            for (int j = first; j < first + count; ++j) {
                const o_triangle& t = tris[size_t(order[size_t(j)])];
                for (int k = 0; k < 3; ++k) {
                    // the vertices the builder sees (rt_bvh.cpp build_triangle_bvh)
                    const double a0 = t.v0[k] + t.t[k];
                    const double e1 = (t.v1[k] + t.t[k]) - a0, e2 = (t.v2[k] + t.t[k]) - a0;
                    for (double v : {a0, a0 + e1, a0 + e2}) {
                        lo[k] = std::min(lo[k], v);
                        hi[k] = std::max(hi[k], v);
                    }
                }
            }
        } else {
            for (int c = 0; c < 2; ++c) {
                double l[3], h[3];
                tighten(first + c, l, h);
                for (int k = 0; k < 3; ++k) {
                    lo[k] = std::min(lo[k], l[k]);
                    hi[k] = std::max(hi[k], h[k]);
                }
            }
        }
        for (int k = 0; k < 3; ++k) {
            nodes[size_t(kBvhNodeStride) * n + k] = lo[k];
            nodes[size_t(kBvhNodeStride) * n + 3 + k] = hi[k];
        }
    }
    void build() {
        // kTriStride records as rt_capi.cpp packs them: a0, e1, e2 (the normal is not read here)
        std::vector<double> rec(size_t(kTriStride) * tris.size(), 0.0);
        for (size_t i = 0; i < tris.size(); ++i) {
            const o_triangle& t = tris[i];
            double* q = &rec[size_t(kTriStride) * i];
            for (int k = 0; k < 3; ++k) {
                q[k] = t.v0[k] + t.t[k];
                q[3 + k] = (t.v1[k] + t.t[k]) - q[k];
                q[6 + k] = (t.v2[k] + t.t[k]) - q[k];
            }
        }
        build_triangle_bvh(rec.data(), static_cast<int>(tris.size()), nodes, order);
        depth = depth_of(0);
        if (g_mut == kNoWiden) {
            double lo[3], hi[3];
            tighten(0, lo, hi);
        }
    }
};

struct Ray {
    double v[6];
    V3 o() const { return {v[0], v[1], v[2]}; }
    V3 d() const { return {v[3], v[4], v[5]}; }
};

static bool tri_hit(const Mesh& M, int i, const Ray& r, double& t) {
    return oracle_triangle_intersect(r.v, &M.tris[size_t(i)], &t) != 0;
}

// The triangles' part of IntersectClosest as the reference runs it (Scene.h:243-254) and as
// closest_stk (csrc/rt_trace_common.hpp) runs it without a BVH: index order, strict '<'.
static void loop_triangles(const Mesh& M, const Ray& r, bool& found, double& best, int& idx) {
    for (int i = 0; i < static_cast<int>(M.tris.size()); ++i) {
        double t;
        if (tri_hit(M, i, r, t) && (!found || t < best)) {
            found = true;
            best = t;
            idx = i;
        }
    }
}

// csrc/rt_trace_common.hpp bvh_box_v
static bool bvh_box_v(const double* nd, V3 o, V3 d, V3 inv, double& tn) {
    double lo = -INFINITY, hi = INFINITY;
    const double oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, ii[3] = {inv.x, inv.y, inv.z};
    for (int k = 0; k < 3; ++k) {
        if (dd[k] != 0.0) {
            double t0 = (nd[k] - oo[k]) * ii[k], t1 = (nd[3 + k] - oo[k]) * ii[k];
            if (t0 > t1) {
                const double x = t0;
                t0 = t1;
                t1 = x;
            }
            lo = std::fmax(lo, t0);  // fmax/fmin drop a NaN operand
            hi = std::fmin(hi, t1);
        } else if (oo[k] < nd[k] || oo[k] > nd[3 + k]) {
            return false;
        }
    }
    tn = lo;
    return !(hi < 0.0) && !(lo > hi + 1e-12 * std::fabs(hi));
}

static V3 inverse(V3 d) {  // the first statement of all three walks
    return {d.x != 0.0 ? 1.0 / d.x : 0.0, d.y != 0.0 ? 1.0 / d.y : 0.0,
            d.z != 0.0 ? 1.0 / d.z : 0.0};
}

struct Tally {
    uint64_t rays = 0, packets = 0, hits = 0;
    uint64_t bad_lane = 0, bad_wave = 0, bad_any = 0;
    int max_sp = 0, deepest_leaf = -1;
    void add(const Tally& t) {
        rays += t.rays;
        packets += t.packets;
        hits += t.hits;
        bad_lane += t.bad_lane;
        bad_wave += t.bad_wave;
        bad_any += t.bad_any;
        max_sp = std::max(max_sp, t.max_sp);
        deepest_leaf = std::max(deepest_leaf, t.deepest_leaf);
    }
};

// csrc/rt_trace_common.hpp bvh_triangles (the per-lane walk; kind is 3 where idx is set)
static void bvh_triangles(const Mesh& M, const Ray& r, bool& found, double& best, int& idx,
                          Tally& T) {
    const double* bvh = M.nodes.data();
    const V3 o = r.o(), d = r.d(), inv = inverse(d);
    bool tf = false;
    double tb = 0.0;
    int ti = 0;
    std::vector<int> stk(size_t(M.depth) + 8);
    int sp = 0;
    double tn;
    if (bvh_box_v(bvh, o, d, inv, tn)) stk[size_t(sp++)] = 0;
    while (sp > 0) {
        T.max_sp = std::max(T.max_sp, sp);
        const int n = stk[size_t(--sp)];
        int first, count, axis;
        M.node(n, first, count, axis);
        if (count > 0) {
            for (int j = first; j < first + count; ++j) {
                const int i = M.order[size_t(j)];
                double t;
                if (tri_hit(M, i, r, t) && (!tf || t < tb || (t == tb && i < ti))) {
                    tf = true;
                    tb = t;
                    ti = i;
                }
            }
            continue;
        }
        const double bound = tf ? (found ? std::fmin(tb, best) : tb) : (found ? best : INFINITY);
        const double lim = bound * (1.0 + 1e-9);
        double t0, t1;
        const bool h0 = bvh_box_v(bvh + kBvhNodeStride * first, o, d, inv, t0) && !(t0 > lim);
        const bool h1 = bvh_box_v(bvh + kBvhNodeStride * (first + 1), o, d, inv, t1) && !(t1 > lim);
        if (h0 && h1) {  // nearer child on top
            const bool near0 = !(t1 < t0);
            stk[size_t(sp++)] = near0 ? first + 1 : first;
            stk[size_t(sp++)] = near0 ? first : first + 1;
        } else if (h0) {
            stk[size_t(sp++)] = first;
        } else if (h1) {
            stk[size_t(sp++)] = first + 1;
        }
        T.max_sp = std::max(T.max_sp, sp);
    }
    if (tf && (!found || tb < best)) {
        found = true;
        best = tb;
        idx = ti;
    }
}

// csrc/rt_anyhit_device.hpp any_bvh_triangles
static bool any_bvh_triangles(const Mesh& M, const Ray& r, double max_dist, Tally& T) {
    const double* bvh = M.nodes.data();
    const V3 o = r.o(), d = r.d(), inv = inverse(d);
    const double lim = max_dist * (1.0 + 1e-9);
    std::vector<int> stk(size_t(M.depth) + 8);
    int sp = 0;
    double tn;
    if (bvh_box_v(bvh, o, d, inv, tn) && !(tn > lim)) stk[size_t(sp++)] = 0;
    while (sp > 0) {
        T.max_sp = std::max(T.max_sp, sp);
        int first, count, axis;
        M.node(stk[size_t(--sp)], first, count, axis);
        if (count > 0) {
            for (int j = first; j < first + count; ++j) {
                double t;
                if (tri_hit(M, M.order[size_t(j)], r, t) && t < max_dist) return true;
            }
            continue;
        }
        double t0, t1;
        const bool h0 = bvh_box_v(bvh + kBvhNodeStride * first, o, d, inv, t0) && !(t0 > lim);
        const bool h1 = bvh_box_v(bvh + kBvhNodeStride * (first + 1), o, d, inv, t1) && !(t1 > lim);
        if (h0 && h1) {
            const bool near0 = !(t1 < t0);
            stk[size_t(sp++)] = near0 ? first + 1 : first;
            stk[size_t(sp++)] = near0 ? first : first + 1;
        } else if (h0) {
            stk[size_t(sp++)] = first;
        } else if (h1) {
            stk[size_t(sp++)] = first + 1;
        }
        T.max_sp = std::max(T.max_sp, sp);
    }
    return false;
}
// IntersectAnyBefore's triangles, in index order (csrc/rt_anyhit_device.hpp: t < max_dist)
static bool any_loop(const Mesh& M, const Ray& r, double max_dist) {
    for (int i = 0; i < static_cast<int>(M.tris.size()); ++i) {
        double t;
        if (tri_hit(M, i, r, t) && t < max_dist) return true;
    }
    return false;
}

// csrc/rt_packet_device.hpp bvh_wave over 64 emulated lanes: one node stack for the wave, a
// ballot over the active lanes' box tests, children ordered by the active lanes' majority
// direction along the split axis.  `active` is the exec mask: an inactive lane neither votes nor
// changes.  leaf_depth[l], when set: the deepest leaf lane l tested triangles in.
struct Lane {
    Ray r;
    bool found;
    double best;
    int idx;
};
static void bvh_wave(const Mesh& M, Lane* L, uint64_t active, Tally& T, int* leaf_depth) {
    const double* bvh = M.nodes.data();
    V3 inv[64];
    bool tf[64];
    double tb[64];
    int ti[64];
    for (int l = 0; l < 64; ++l) {
        inv[l] = inverse(L[l].r.d());
        tf[l] = false;
        tb[l] = 0.0;
        ti[l] = 0;
    }
    std::vector<int> stk(size_t(M.depth) + 8), dep(size_t(M.depth) + 8);
    int sp = 0;
    dep[size_t(sp)] = 0;
    stk[size_t(sp++)] = 0;
    while (sp > 0) {
        T.max_sp = std::max(T.max_sp, sp);
        const int depth = dep[size_t(sp - 1)];
        const int node = stk[size_t(--sp)];  // readfirstlane: the stack is uniform
        const double* nd = bvh + kBvhNodeStride * node;
        bool in[64];
        uint64_t ballot = 0;
        for (int l = 0; l < 64; ++l) {
            in[l] = false;
            if (!(active >> l & 1)) continue;
            const double bound = tf[l] ? (L[l].found ? std::fmin(tb[l], L[l].best) : tb[l])
                                       : (L[l].found ? L[l].best : INFINITY);
            double tn;
            const double lim = g_mut == kNoMargin ? bound : bound * (1.0 + 1e-9);
            in[l] = bvh_box_v(nd, L[l].r.o(), L[l].r.d(), inv[l], tn) && !(tn > lim);
            if (in[l]) ballot |= 1ull << l;
        }
        if (ballot == 0) continue;
        int first, count, axis;
        M.node(node, first, count, axis);
        if (count > 0) {
            for (int l = 0; l < 64; ++l) {
                if (!in[l]) continue;
                if (leaf_depth) leaf_depth[l] = std::max(leaf_depth[l], depth);
                for (int j = first; j < first + count; ++j) {
                    const int i = M.order[size_t(j)];
                    double t;
                    if (tri_hit(M, i, L[l].r, t) &&
                        (!tf[l] || t < tb[l] || (g_mut != kNoTie && t == tb[l] && i < ti[l]))) {
                        tf[l] = true;
                        tb[l] = t;
                        ti[l] = i;
                    }
                }
            }
            continue;
        }
        int pos = 0, neg = 0;
        for (int l = 0; l < 64; ++l) {
            const double da = L[l].r.v[3 + axis];
            pos += in[l] && da > 0.0;
            neg += in[l] && da < 0.0;
        }
        const bool low_first = pos >= neg;  // the lower child is nearer for rays going up
        dep[size_t(sp)] = depth + 1;
        stk[size_t(sp++)] = low_first ? first + 1 : first;
        dep[size_t(sp)] = depth + 1;
        stk[size_t(sp++)] = low_first ? first : first + 1;
        T.max_sp = std::max(T.max_sp, sp);
    }
    for (int l = 0; l < 64; ++l) {
        if (!(active >> l & 1)) continue;
        if (tf[l] && (!L[l].found || tb[l] < L[l].best)) {
            L[l].found = true;
            L[l].best = tb[l];
            L[l].idx = ti[l];
        }
    }
}

// One packet: rays, the lanes' hit to beat (found / best), the exec mask.  Every active lane of
// the wave walk and every ray's own walk against the loop; the any-hit walk at, below and above
// the loop's closest triangle t.
static void check_packet(const Mesh& M, const Ray* rays, const bool* found0, const double* best0,
                         uint64_t active, Tally& T, int* leaf_depth = nullptr) {
    Lane L[64];
    for (int l = 0; l < 64; ++l) L[l] = {rays[l], found0[l], best0[l], -1};
    bvh_wave(M, L, active, T, leaf_depth);
    ++T.packets;
    for (int l = 0; l < 64; ++l) {
        if (!(active >> l & 1)) {  // untouched
            T.bad_wave += !(L[l].found == found0[l] && L[l].idx == -1 &&
                            std::memcmp(&L[l].best, &best0[l], 8) == 0);
            continue;
        }
        ++T.rays;
        bool f = found0[l];
        double b = best0[l];
        int i = -1;
        loop_triangles(M, rays[l], f, b, i);
        T.hits += i >= 0;
        T.bad_wave += !(L[l].found == f && L[l].idx == i && (!f || L[l].best == b));
        bool f2 = found0[l];
        double b2 = best0[l];
        int i2 = -1;
        bvh_triangles(M, rays[l], f2, b2, i2, T);
        T.bad_lane += !(f2 == f && i2 == i && (!f || b2 == b));
        // the any-hit walk around the closest triangle t (without a hit to beat)
        bool fa = false;
        double ta = 0.0;
        int ia = -1;
        if (found0[l]) loop_triangles(M, rays[l], fa, ta, ia);
        else fa = f, ta = b, ia = i;
        const double md[4] = {fa ? ta : 1.0, fa ? std::nextafter(ta, 0.0) : 0x1p-40,
                              fa ? std::nextafter(ta, INFINITY) : 0x1p40, INFINITY};
        for (double m : md) T.bad_any += any_bvh_triangles(M, rays[l], m, T) != any_loop(M, rays[l], m);
    }
}

static void no_hit(bool* f, double* b) {
    for (int l = 0; l < 64; ++l) {
        f[l] = false;
        b[l] = 0.0;
    }
}

// A hit to beat per lane: the loop's own t (a tie the triangle must lose), its neighbours, a
// random factor of it, or anything.
static void hits_to_beat(const Mesh& M, const Ray* rays, Rng& R, bool* f, double* b) {
    for (int l = 0; l < 64; ++l) {
        bool ff = false;
        double t = 0.0;
        int i = -1;
        loop_triangles(M, rays[l], ff, t, i);
        const uint32_t k = R.below(6);
        f[l] = k != 5;
        if (!ff) t = R.u(0.0, 20.0);
        b[l] = k == 0 ? t : k == 1 ? std::nextafter(t, 0.0) : k == 2 ? std::nextafter(t, INFINITY)
             : k == 3 ? t * R.u(0.5, 1.5) : R.u(0.0, 30.0);
        if (k == 5) b[l] = 0.0;
    }
}

static uint64_t random_mask(Rng& R) {
    const uint32_t k = R.below(4);
    uint64_t m = R.next();
    if (k == 1) m &= R.next();
    if (k == 2) m = 1ull << R.below(64);
    if (k == 3) m |= R.next();
    return m ? m : 1ull;
}

static void tile_rays(const o_camera& cam, uint32_t x0, uint32_t y0, Ray* rays) {
    for (uint32_t l = 0; l < 64; ++l) {  // lanes past the image are clamped into it, as the kernel's
        const uint32_t x = std::min(x0 + l % 8, cam.width - 1), y = std::min(y0 + l / 8, cam.height - 1);
        oracle_get_ray(&cam, x, y, 0, 0, 0, rays[l].v);
    }
}

// ------------------------------------------------------------------ random meshes
static void random_mesh(Rng& R, Mesh& M) {
    const int nt = static_cast<int>(32.0 * std::pow(2000.0 / 32.0, R.u(0.0, 1.0)));
    const double size = std::pow(2.0, R.u(-4.0, 1.0));
    const uint32_t kind = R.below(4);  // 0 soup, 1 on a lattice (shared vertices: ties), 2 flat, 3 duplicates
    M.tris.assign(size_t(nt), o_triangle{});
    for (int i = 0; i < nt; ++i) {
        o_triangle& t = M.tris[size_t(i)];
        if (kind == 3 && i > 0 && R.below(4) == 0) {
            t = M.tris[R.below(uint32_t(i))];
            continue;
        }
        double c[3];
        for (int k = 0; k < 3; ++k) c[k] = R.u(-4.0, 4.0);
        for (int k = 0; k < 3; ++k) {
            t.v0[k] = c[k] + R.u(-size, size);
            t.v1[k] = c[k] + R.u(-size, size);
            t.v2[k] = c[k] + R.u(-size, size);
            if (kind == 1) {
                t.v0[k] = std::floor(t.v0[k] * 2.0) / 2.0;
                t.v1[k] = std::floor(t.v1[k] * 2.0) / 2.0 + (k == i % 3 ? 0.5 : 0.0);
                t.v2[k] = std::floor(t.v2[k] * 2.0) / 2.0 + (k == (i + 1) % 3 ? 0.5 : 0.0);
            }
        }
        if (kind == 2) t.v0[1] = t.v1[1] = t.v2[1] = i % 3 == 0 ? 0.0 : 0.5;
        if (R.below(8) == 0)
            for (int k = 0; k < 3; ++k) t.t[k] = R.u(-1.0, 1.0);
    }
    M.build();
}

static void point_on(const Mesh& M, Rng& R, double* p) {
    const o_triangle& t = M.tris[R.below(uint32_t(M.tris.size()))];
    const uint32_t k = R.below(8);
    double a = R.u(0.0, 1.0), b = R.u(0.0, 1.0);
    if (a + b > 1.0) a = 1.0 - a, b = 1.0 - b;
    if (k == 0) a = 0.0, b = 0.0;  // a vertex, an edge
    if (k == 1) a = 1.0, b = 0.0;
    if (k == 2) b = 0.0;
    if (k == 3) a = 0.5, b = 0.5;
    for (int j = 0; j < 3; ++j)
        p[j] = t.v0[j] + t.t[j] + a * (t.v1[j] - t.v0[j]) + b * (t.v2[j] - t.v0[j]);
}

static void random_case(uint64_t seed, int packets, Tally& T) {
    Rng R{seed};
    Mesh M;
    random_mesh(R, M);
    Ray rays[64];
    bool f[64];
    double b[64];
    for (int p = 0; p < packets; ++p) {
        const uint32_t kind = R.below(4);
        if (kind == 0) {  // one origin through an 8x8 pixel tile
            o_camera cam{};
            cam.width = 64;
            cam.height = 48;
            cam.aa_samples = 1;
            for (int k = 0; k < 3; ++k) cam.position[k] = R.below(2) ? std::floor(R.u(-8, 8)) : R.u(-8, 8);
            cam.position[2] = -std::fabs(cam.position[2]) - R.u(0.0, 4.0);
            cam.focal = std::pow(2.0, R.u(3.0, 8.0));
            tile_rays(cam, 8 * R.below(8), 8 * R.below(6), rays);
        } else if (kind == 3) {
            // d[k] == 0 through a vertex, the origin's coordinate k within two units in the last
            // place of the vertex's: bvh_box_v compares it with the box's faces exactly, so only
            // the builder's widening keeps a leaf whose extreme vertex this is
            for (int l = 0; l < 64; ++l) {
                const o_triangle& t = M.tris[R.below(uint32_t(M.tris.size()))];
                const double* vs[3] = {t.v0, t.v1, t.v2};
                const double* v = vs[R.below(3)];
                const int k = static_cast<int>(R.below(3));
                const double s = R.u(0.5, 6.0);
                for (int j = 0; j < 3; ++j) {
                    const double dj = j == k ? 0.0 : R.u(-1.0, 1.0);
                    rays[l].v[3 + j] = dj;
                    rays[l].v[j] = (v[j] + t.t[j]) - dj * s;
                }
                for (int n = static_cast<int>(R.below(5)) - 2; n != 0; n += n < 0 ? 1 : -1)
                    rays[l].v[k] = std::nextafter(rays[l].v[k], n < 0 ? -INFINITY : INFINITY);
            }
        } else {  // unrelated rays, aimed at points of triangles (vertices and edges among them)
            double o[3], p3[3];
            for (int l = 0; l < 64; ++l) {
                if (l == 0 || kind == 2)
                    for (int k = 0; k < 3; ++k) o[k] = R.below(4) ? R.u(-8.0, 8.0) : std::floor(R.u(-6, 6)) / 2.0;
                point_on(M, R, p3);
                const double s = std::pow(2.0, R.u(-3.0, 3.0));
                for (int k = 0; k < 3; ++k) {
                    rays[l].v[k] = o[k];
                    rays[l].v[3 + k] = (p3[k] - o[k]) * s;
                }
                if (R.below(16) == 0) rays[l].v[3 + R.below(3)] = 0.0;
            }
        }
        const uint32_t how = R.below(4);
        if (how & 1) hits_to_beat(M, rays, R, f, b);
        else no_hit(f, b);
        check_packet(M, rays, f, b, (how & 2) ? random_mask(R) : ~0ull, T);
    }
}

// ------------------------------------------------------------------ crafted meshes
struct Crafted {
    Mesh M;
    o_camera cam{};
    std::vector<V3> lights;
};

static bool read_crafted(const char* path, Crafted& C) {
    FILE* fh = std::fopen(path, "r");
    if (!fh) return false;
    char tok[64];
    auto num = [&](double& v) {
        if (std::fscanf(fh, "%63s", tok) != 1) return false;
        v = std::strtod(tok, nullptr);
        return true;
    };
    double nt = 0.0, w = 0.0, h = 0.0, nl = 0.0, v = 0.0;
    bool ok = num(nt) && num(w) && num(h) && num(C.cam.position[0]) && num(C.cam.position[1]) &&
              num(C.cam.position[2]) && num(C.cam.focal) && num(nl);
    C.cam.width = static_cast<uint32_t>(w);
    C.cam.height = static_cast<uint32_t>(h);
    C.cam.aa_samples = 1;
    C.M.tris.assign(ok ? size_t(nt) : 0, o_triangle{});
    for (o_triangle& t : C.M.tris)
        for (int k = 0; k < 12 && ok; ++k) {
            ok = num(v);
            (k < 3 ? t.v0 : k < 6 ? t.v1 : k < 9 ? t.v2 : t.t)[k % 3] = v;
        }
    for (int l = 0; ok && l < static_cast<int>(nl); ++l) {
        V3 p{};
        ok = num(p.x) && num(p.y) && num(p.z);
        C.lights.push_back(p);
    }
    std::fclose(fh);
    if (ok) C.M.build();
    return ok;
}

// Every tile of the crafted frame: its camera rays (whole wave, a random exec mask, hits to
// beat), then per light the shadow rays of the lanes that hit — directLightning's, Scene.h:86-124:
// origin P + n·bias, direction unit(light − P), the lanes without a shadow ray inactive.
static void crafted_frame(const Crafted& C, uint64_t seed, Tally& T, int* column_leaf) {
    Rng R{seed};
    const o_scene sc{nullptr, 0, nullptr, 0, C.M.tris.data(), static_cast<int32_t>(C.M.tris.size()),
                     nullptr, 0};
    Ray rays[64], sh[64];
    bool f[64];
    double b[64];
    for (uint32_t y0 = 0; y0 < C.cam.height; y0 += 8)
        for (uint32_t x0 = 0; x0 < C.cam.width; x0 += 8) {
            tile_rays(C.cam, x0, y0, rays);
            int leaf[64];
            std::fill(leaf, leaf + 64, -1);
            no_hit(f, b);
            check_packet(C.M, rays, f, b, ~0ull, T, leaf);
            for (int l = 0; l < 64; ++l)
                if (rays[l].v[3] == 0.0 && column_leaf) *column_leaf = std::max(*column_leaf, leaf[l]);
            check_packet(C.M, rays, f, b, random_mask(R), T);
            hits_to_beat(C.M, rays, R, f, b);
            check_packet(C.M, rays, f, b, ~0ull, T);
            check_packet(C.M, rays, f, b, random_mask(R), T);
            for (const V3& lp : C.lights) {
                uint64_t casting = 0;
                for (int l = 0; l < 64; ++l) {
                    double o7[7];
                    int32_t index;
                    sh[l] = rays[l];
                    if (!oracle_closest(&sc, rays[l].v, o7, &index)) continue;
                    double n[3] = {o7[1], o7[2], o7[3]};
                    if (n[0] * rays[l].v[3] + n[1] * rays[l].v[4] + n[2] * rays[l].v[5] >= 0.0)
                        for (double& c : n) c = -c;
                    const double v[3] = {lp.x - o7[4], lp.y - o7[5], lp.z - o7[6]};
                    const double dist = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                    if (!(dist > 1e-3) || !(n[0] * v[0] + n[1] * v[1] + n[2] * v[2] > 0.0)) continue;
                    for (int k = 0; k < 3; ++k) {
                        sh[l].v[k] = o7[4 + k] + n[k] * 1e-3;
                        sh[l].v[3 + k] = v[k] / dist;
                    }
                    casting |= 1ull << l;
                }
                if (!casting) continue;
                no_hit(f, b);
                check_packet(C.M, sh, f, b, casting, T);
            }
        }
}

static int report(const char* what, const Tally& T, int extra_bad) {
    std::printf("%s rays %" PRIu64 " packets %" PRIu64 " hits %" PRIu64 " bad_wave %" PRIu64
                " bad_lane %" PRIu64 " bad_any %" PRIu64 " max_sp %d\n",
                what, T.rays, T.packets, T.hits, T.bad_wave, T.bad_lane, T.bad_any, T.max_sp);
    return (T.bad_wave || T.bad_lane || T.bad_any || extra_bad) ? 1 : 0;
}

int main(int argc, char** argv) {
    std::vector<std::string> args;
    for (int i = 1; i < argc; ++i) {
        if (std::string(argv[i]) == "--mutate" && i + 1 < argc) {
            const std::string m = argv[++i];
            g_mut = m == "notie" ? kNoTie : m == "nomargin" ? kNoMargin : m == "nowiden" ? kNoWiden : kNone;
            if (g_mut == kNone) return 2;
        } else {
            args.push_back(argv[i]);
        }
    }
    if (args.size() >= 3 && args[0] == "prop") {
        const uint64_t seed = std::strtoull(args[1].c_str(), nullptr, 10);
        const int cases = std::atoi(args[2].c_str());
        Tally all;
        int unread = 0;
        for (size_t a = 3; a < args.size(); ++a) {
            Crafted C;
            if (!read_crafted(args[a].c_str(), C)) {
                std::fprintf(stderr, "cannot read %s\n", args[a].c_str());
                ++unread;
                continue;
            }
            Tally T;
            crafted_frame(C, seed + a, T, nullptr);
            std::printf("file %s triangles %zu depth %d bad %" PRIu64 "\n", args[a].c_str(),
                        C.M.tris.size(), C.M.depth, T.bad_wave + T.bad_lane + T.bad_any);
            all.add(T);
        }
#pragma omp parallel for schedule(dynamic)
        for (int c = 0; c < cases; ++c) {
            Tally T;
            random_case(seed * 1000003ull + uint64_t(c), 12, T);
#pragma omp critical
            all.add(T);
        }
        return report("prop", all, unread);
    }
    if (args.size() == 3 && args[0] == "depth") {
        const int pkstack = std::atoi(args[1].c_str());
        Crafted C;
        if (!read_crafted(args[2].c_str(), C)) return 2;
        int bad = 0, column_leaf = -1;
        Tally T;
        crafted_frame(C, 1, T, &column_leaf);
        // the deepest leaf of the tree: a leaf at depth C.M.depth
        std::printf("crafted depth %d max_sp %d column_leaf %d kBvhStack %d kPkStack %d\n", C.M.depth,
                    T.max_sp, column_leaf, kBvhStack, pkstack);
        bad += !(C.M.depth <= 48 && T.max_sp <= C.M.depth + 1 && T.max_sp <= kBvhStack &&
                 T.max_sp <= pkstack && column_leaf == C.M.depth);
        for (int c = 0; c < 2; ++c) {
            Tally R;
            Rng rng{uint64_t(77 + c)};
            Mesh M;
            random_mesh(rng, M);
            random_case(uint64_t(77 + c), 40, R);  // the same mesh: the same seed
            std::printf("random%d triangles %zu depth %d max_sp %d\n", c, M.tris.size(), M.depth,
                        R.max_sp);
            bad += !(M.depth <= 48 && R.max_sp <= M.depth + 1 && R.max_sp <= kBvhStack &&
                     R.max_sp <= pkstack);
            T.add(R);
        }
        return report("depth", T, bad);
    }
    std::fprintf(stderr, "usage: walk_main prop SEED CASES [--mutate M] [FILE...] | depth PKSTACK FILE\n");
    return 2;
}
