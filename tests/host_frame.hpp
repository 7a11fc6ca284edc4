// host_frame.hpp — what the stand-alone host check programs of the tile table share
// (shadow_table/, tile_class/, plane_clear/, tile_lists/, tile_shadowed/; each has its own
// properties and main): the random frames, the frame file, the table kernel's inputs as
// pk_build_image forms them, the oracle's shadow rays and the class word of a tile.
//
// The frame file (tests/host_programs.py write_frame_file): width height cam(3) focal bias ns np
// nl, then cx cy cz r per sphere, px py pz nx ny nz per plane, x y z per light (hex floats).
#pragma once

#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_cone_table.hpp"
#include "rt_shadow_table.hpp"
#include "rt_oracle.h"

using namespace rtamd;

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
    double lu(double lo, double hi) { return std::exp(u(std::log(lo), std::log(hi))); }
    uint32_t below(uint32_t n) { return static_cast<uint32_t>(next() % n); }
};

struct Frame {
    o_camera cam;
    ConeRowPlan rp;
    double bias;
    std::vector<o_sphere> sph;
    std::vector<o_plane> pl;
    std::vector<o_light> lt;
    // the table kernel's inputs, as pk_build_image forms them
    std::vector<float> terms;    // 8 per sphere (cone_sphere_terms)
    std::vector<double> centre;  // 3 per sphere
    std::vector<double> planes;  // 8 per plane: p n num flag
    void prepare() {
        const size_t ns = sph.size();
        terms.assign(8 * ns, 0.0f);
        centre.assign(3 * ns, 0.0);
        for (size_t i = 0; i < ns; ++i) {
            const double s[4] = {sph[i].center[0], sph[i].center[1], sph[i].center[2],
                                 sph[i].radius * sph[i].radius};
            cone_sphere_terms(s, cam.position, &terms[8 * i]);
            for (int k = 0; k < 3; ++k) centre[3 * i + k] = s[k];
        }
        planes.assign(8 * pl.size(), 0.0);
        for (size_t i = 0; i < pl.size(); ++i) {
            double* o = &planes[8 * i];
            for (int k = 0; k < 3; ++k) o[k] = pl[i].point[k], o[3 + k] = pl[i].normal[k];
            o[6] = ((o[0] - cam.position[0]) * o[3] + (o[1] - cam.position[1]) * o[4]) +
                   (o[2] - cam.position[2]) * o[5];
            const double n1 = std::fabs(o[3]) + std::fabs(o[4]) + std::fabs(o[5]);
            o[7] = std::fabs(o[6]) >= 0x1p-900 && std::fabs(o[6]) <= 0x1p400 && n1 <= 0x1p90 ? 1.0
                                                                                           : 0.0;
        }
    }
    o_scene scene() const {
        o_scene sc{};
        sc.spheres = sph.data();
        sc.n_spheres = static_cast<int32_t>(sph.size());
        sc.planes = pl.data();
        sc.n_planes = static_cast<int32_t>(pl.size());
        sc.lights = lt.data();
        sc.n_lights = static_cast<int32_t>(lt.size());
        return sc;
    }
};

inline double cam_dz(const o_camera& c) { return (c.position[2] + c.focal) - c.position[2]; }

// the camera-cone mask of the tile at (x0, yl0), as the table kernel forms it
inline uint64_t tile_cone_mask(const Frame& F, uint32_t x0, uint32_t yl0) {
    const ConeRect q = cone_tile_rect(x0, yl0, F.cam.width, F.rp);
    const ConeBound CB = cone_tile_bound(q, static_cast<double>(F.cam.width) / 2.0,
                                         static_cast<double>(F.cam.height) / 2.0,
                                         F.cam.position[0], F.cam.position[1], cam_dz(F.cam));
    return cone_tile_mask(CB, F.terms.data(), 8, static_cast<int>(F.sph.size()));
}

// the pixel lane (lx, ly) of the tile traces (clamped into the image, as the kernel clamps)
inline void lane_pixel(const Frame& F, uint32_t x0, uint32_t yl0, uint32_t lx, uint32_t ly,
                       uint32_t& x, uint32_t& y, bool& valid) {
    const uint32_t xx = x0 + lx, yl = yl0 + ly;
    valid = xx < F.cam.width && yl < F.rp.rows;
    x = xx < F.cam.width ? xx : F.cam.width - 1;
    y = cone_image_row(F.rp, yl < F.rp.rows ? yl : F.rp.rows - 1);
}

inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The pixel's shadow rays as the oracle forms them (closest, trace, direct, light_term of
// rt_oracle.c): type = oracle_closest's, so[] the origin, and per light the direction, maxDist and
// whether the ray is cast.
struct Shadow {
    int type;
    double so[3];
    double L[kShadowTabLights][3], max_dist[kShadowTabLights];
    bool cast[kShadowTabLights];
};
inline void pixel_shadow(const Frame& F, const o_scene& sc, uint32_t x, uint32_t y, Shadow& S) {
    double ray[6], out[7];
    int32_t index = -1;
    oracle_get_ray(&F.cam, x, y, 0, 0, 0, ray);
    S.type = oracle_closest(&sc, ray, out, &index);
    for (size_t l = 0; l < F.lt.size(); ++l) S.cast[l] = false;
    if (!S.type) return;
    const double dl = std::sqrt(dot3(ray + 3, ray + 3));
    const double inc[3] = {ray[3] / dl, ray[4] / dl, ray[5] / dl};
    double n[3] = {out[1], out[2], out[3]};
    if (!(dot3(n, inc) < 0.0))
        for (int k = 0; k < 3; ++k) n[k] = -n[k];
    const double nl = std::sqrt(dot3(n, n));
    for (int k = 0; k < 3; ++k) n[k] /= nl;
    const double* P = out + 4;
    for (int k = 0; k < 3; ++k) S.so[k] = P[k] + n[k] * F.bias;
    for (size_t l = 0; l < F.lt.size(); ++l) {
        const double v[3] = {F.lt[l].position[0] - P[0], F.lt[l].position[1] - P[1],
                             F.lt[l].position[2] - P[2]};
        const double dist = std::sqrt(dot3(v, v));
        if (dist <= 0.0) continue;
        for (int k = 0; k < 3; ++k) S.L[l][k] = v[k] / dist;
        const double ndl = dot3(n, S.L[l]);
        if (!(ndl > 0.0) || dist <= F.bias) continue;
        S.cast[l] = true;
        S.max_dist[l] = dist - F.bias;
    }
}

// a root of |o + t d − C|² = r² in [1e-6, max_dist] (FP64, both roots)
inline bool shadow_ray_meets(const double* o, const double* d, double max_dist, const o_sphere& s) {
    const double oc[3] = {o[0] - s.center[0], o[1] - s.center[1], o[2] - s.center[2]};
    const double a = dot3(d, d), b = 2.0 * dot3(oc, d), c = dot3(oc, oc) - s.radius * s.radius;
    const double disc = b * b - 4.0 * a * c;
    if (disc < 0.0) return false;
    const double sq = std::sqrt(disc);
    const double t0 = (-b - sq) / (2.0 * a), t1 = (-b + sq) / (2.0 * a);
    return (t0 >= 1e-6 && t0 <= max_dist) || (t1 >= 1e-6 && t1 <= max_dist);
}

inline void set_rows(Frame& F, uint32_t begin, uint32_t block, uint32_t cycle) {
    const uint32_t H = F.cam.height;
    F.rp.row0 = begin;
    F.rp.row_block = 0;
    F.rp.row_stride = 0;
    if (cycle > 1 && block > 0) {
        F.rp.row_block = block;
        F.rp.row_stride = block * cycle;
        uint32_t rows = 0;
        for (uint32_t b = begin; b < H; b += block * cycle) rows += block < H - b ? block : H - b;
        F.rp.rows = rows;
    } else {
        F.rp.rows = H - begin;
    }
}

// The plane point a camera ray through screen position (px, py) sees first (planes only), with
// the plane's normal turned towards the camera; false: the ray meets no plane.
inline bool plane_point(const Frame& F, double px, double py, double* P, double* n, double* t_out) {
    const double v[3] = {px - F.cam.width / 2.0 - F.cam.position[0],
                         F.cam.height / 2.0 - py - F.cam.position[1], cam_dz(F.cam)};
    double best = INFINITY;
    int bi = -1;
    for (size_t i = 0; i < F.pl.size(); ++i) {
        const double den = dot3(F.pl[i].normal, v);
        const double w[3] = {F.pl[i].point[0] - F.cam.position[0],
                             F.pl[i].point[1] - F.cam.position[1],
                             F.pl[i].point[2] - F.cam.position[2]};
        const double t = dot3(w, F.pl[i].normal) / den;
        if (std::fabs(den) > 1e-9 && t > 0.0 && t < best) best = t, bi = static_cast<int>(i);
    }
    if (bi < 0) return false;
    const double nl = std::sqrt(dot3(F.pl[bi].normal, F.pl[bi].normal));
    const double sgn = dot3(F.pl[bi].normal, v) < 0.0 ? 1.0 : -1.0;
    for (int k = 0; k < 3; ++k) {
        P[k] = F.cam.position[k] + best * v[k];
        n[k] = sgn * F.pl[bi].normal[k] / nl;
    }
    *t_out = best * std::sqrt(dot3(v, v));
    return true;
}

inline o_plane mk_plane(const double* p, const double* n) {
    o_plane q{};
    for (int k = 0; k < 3; ++k) q.point[k] = p[k], q.normal[k] = n[k];
    return q;
}

// A wall facing the camera, a long focal length (small tiles), a bias larger than a tile's patch,
// a light within 2·bias of the wall off to one side and spheres floating about bias above the
// wall between the frame and the light, out of sight: the shadow rays run nearly parallel to the
// wall at height bias, where only the bias allowance keeps the spheres.
inline Frame bias_frame(Rng& R) {
    Frame F{};
    F.cam.width = 9 + 8 * R.below(6) + 1 + R.below(7);
    F.cam.height = 9 + 8 * R.below(4) + 1 + R.below(7);
    F.cam.aa_samples = 1;
    F.cam.far_plane = 200.0;
    F.cam.position[0] = R.u(-3.0, 3.0);
    F.cam.position[1] = R.u(-3.0, 3.0);
    F.cam.position[2] = -25.0;
    F.cam.focal = R.u(2.0, 6.0) * F.cam.width;
    set_rows(F, 0, 0, 1);
    F.bias = R.u(3.0, 6.0);
    const double wp[3] = {0.0, 0.0, 10.0}, wn[3] = {0.0, 0.0, -1.0};
    F.pl.push_back(mk_plane(wp, wn));
    // the wall patch the frame sees is about ±35·W/(2·focal) wide: the light off to one side
    const double half = 35.0 * F.cam.width / (2.0 * F.cam.focal);
    o_light l{};
    l.position[0] = F.cam.position[0] + R.u(2.5, 4.0) * half;
    l.position[1] = F.cam.position[1] + R.u(-0.3, 0.3) * half;
    l.position[2] = 10.0 - R.u(1.0, 1.9) * F.bias;
    l.intensity = 100.0;
    F.lt.push_back(l);
    const int ns = 3 + static_cast<int>(R.below(6));
    for (int i = 0; i < ns; ++i) {
        o_sphere s{};
        s.radius = R.u(0.1, 0.3) * F.bias;
        s.center[0] = F.cam.position[0] + R.u(1.3, 1.6) * half + s.radius;
        s.center[1] = F.cam.position[1] + R.u(-0.8, 0.8) * half;
        s.center[2] = 10.0 - R.u(1.0, 1.4) * F.bias;
        F.sph.push_back(s);
    }
    F.prepare();
    return F;
}

inline Frame random_frame(Rng& R) {
    if (R.below(8) == 0) return bias_frame(R);
    Frame F{};
    uint32_t W, H;
    do W = 9 + R.below(80); while (W % 8 == 0);
    do H = 9 + R.below(60); while (H % 8 == 0);
    F.cam.width = W;
    F.cam.height = H;
    F.cam.aa_samples = 1;
    F.cam.near_plane = 0.0;
    F.cam.far_plane = 200.0;
    // off-axis cameras: the screen stays at the world origin's x and y (Camera::getRay)
    const double off = R.below(3) == 0 ? 0.0 : R.u(0.0, 1.5) * W;
    F.cam.position[0] = R.u(-off, off);
    F.cam.position[1] = R.u(-off, off);
    F.cam.position[2] = R.u(-40.0, 40.0);
    // (a tile's cone at a focal length of a few pixels holds most of the scene, and a tile whose
    // cone holds a sphere has no entry: two frames in three have a longer one)
    F.cam.focal = R.below(3) == 0 ? R.lu(0.05, 100.0) : R.lu(8.0, 100.0);
    switch (R.below(4)) {
        case 0: set_rows(F, 0, 0, 1); break;
        case 1: set_rows(F, 1, 2, 2); break;
        case 2: set_rows(F, 0, 3, 3); break;
        default: set_rows(F, 0, 8, 2); break;
    }
    F.bias = R.below(4) == 0 ? R.lu(1e-6, 0.05) : 1e-3;
    const double* c = F.cam.position;
    // planes: a floor below the camera, a back wall in front, then nearly parallel twins, tilted
    // side walls and a ceiling; normals as stored (either orientation, lengths 0.5 .. 1.1)
    const int np = 1 + static_cast<int>(R.below(5));
    const double scale = R.lu(3.0, 40.0);
    auto tilt = [&](double* n, double amount) {
        for (int k = 0; k < 3; ++k) n[k] += R.u(-amount, amount);
        const double f = R.u(0.5, 1.1) / std::sqrt(dot3(n, n)) * (R.below(2) ? 1.0 : -1.0);
        for (int k = 0; k < 3; ++k) n[k] *= f;
    };
    const bool wall_first = R.below(2) == 0;
    for (int i = 0; i < np; ++i) {
        double p[3] = {c[0], c[1], c[2]}, n[3] = {0.0, 0.0, 0.0};
        const int kind = i == 0 ? (wall_first ? 1 : 0) : i == 1 ? (wall_first ? 0 : 1) : i;
        const double amount = R.below(3) == 0 ? R.u(0.0, 0.5) : 0.0;
        if (kind == 0) {  // floor
            p[1] -= scale * R.u(0.3, 1.5);
            n[1] = 1.0;
            tilt(n, amount);
        } else if (kind == 1) {  // back wall
            p[2] += scale * R.u(1.0, 4.0);
            n[2] = -1.0;
            tilt(n, amount);
        } else if (kind == 2) {  // a nearly parallel twin of an earlier plane, just behind it
            const o_plane& q = F.pl[R.below(static_cast<uint32_t>(F.pl.size()))];
            const double w[3] = {q.point[0] - c[0], q.point[1] - c[1], q.point[2] - c[2]};
            const double side = dot3(w, q.normal) > 0.0 ? 1.0 : -1.0;  // away from the camera
            const double nl = std::sqrt(dot3(q.normal, q.normal));
            const double gap = R.below(2) ? R.lu(1e-9, 1e-3) * scale : R.u(0.01, 0.3) * scale;
            for (int k = 0; k < 3; ++k) {
                p[k] = q.point[k] + side * gap * q.normal[k] / nl;
                n[k] = q.normal[k] + R.u(-1.0, 1.0) * (R.below(2) ? 1e-3 : 1e-9);
            }
        } else if (kind == 3) {  // side wall
            const double sx = R.below(2) ? 1.0 : -1.0;
            p[0] += sx * scale * R.u(0.5, 3.0);
            n[0] = -sx;
            tilt(n, R.u(0.0, 0.6));
        } else {  // ceiling
            p[1] += scale * R.u(0.5, 3.0);
            n[1] = -1.0;
            tilt(n, amount);
        }
        F.pl.push_back(mk_plane(p, n));
    }
    // spheres sitting on, within bias of, and floating above the planes' visible parts
    const int ns = F.cam.focal < 8.0 ? 1 + static_cast<int>(R.below(3))
                                     : 3 + static_cast<int>(R.below(10));
    for (int i = 0; i < ns; ++i) {
        double P[3], n[3], t = 0.0;
        bool ok = false;
        for (int tries = 0; tries < 20 && !ok; ++tries)
            ok = plane_point(F, R.u(0.0, W), R.u(0.0, H), P, n, &t);
        o_sphere s{};
        if (!ok) {  // no plane in sight: somewhere behind the camera
            for (int k = 0; k < 3; ++k) s.center[k] = c[k] + R.u(-1.0, 1.0) * scale;
            s.center[2] = c[2] - scale;
            s.radius = 0.1 * scale;
        } else {
            const double v0 = std::sqrt(cam_dz(F.cam) * cam_dz(F.cam) + 1.0);
            const double pix = std::fmin(t / v0, 0.05 * t);  // a pixel's width there, about
            s.radius = pix * R.u(0.5, 3.0);
            double gap = 0.0;
            switch (R.below(4)) {
                case 0: gap = 0.0; break;
                case 1: gap = R.u(0.0, 1.0) * F.bias; break;
                default: gap = s.radius * R.u(0.2, 6.0); break;
            }
            for (int k = 0; k < 3; ++k) s.center[k] = P[k] + n[k] * (s.radius + gap);
        }
        F.sph.push_back(s);
    }
    const int nl = 1 + static_cast<int>(R.below(4));
    for (int i = 0; i < nl; ++i) {
        o_light l{};
        l.intensity = 100.0;
        double P[3], n[3], t = 0.0;
        bool ok = false;
        for (int tries = 0; tries < 20 && !ok; ++tries)
            ok = plane_point(F, R.u(-0.5 * W, 1.5 * W), R.u(-0.5 * H, 1.5 * H), P, n, &t);
        const uint32_t kind = R.below(6);
        if (!ok) {
            for (int k = 0; k < 3; ++k) l.position[k] = c[k] + R.u(-1.0, 1.0) * scale;
        } else if (kind == 0) {  // within 2·bias of a plane
            for (int k = 0; k < 3; ++k) l.position[k] = P[k] + n[k] * R.u(0.2, 2.0) * F.bias;
        } else if (kind == 1) {  // behind the plane
            for (int k = 0; k < 3; ++k) l.position[k] = P[k] - n[k] * R.u(0.05, 1.0) * scale;
        } else if (kind <= 3 && !F.sph.empty()) {  // just past a sphere, seen from the plane
            const o_sphere& s = F.sph[R.below(static_cast<uint32_t>(F.sph.size()))];
            for (int k = 0; k < 3; ++k)
                l.position[k] = s.center[k] + n[k] * s.radius * R.u(1.5, 8.0) +
                                R.u(-1.0, 1.0) * s.radius;
        } else {  // above the plane
            for (int k = 0; k < 3; ++k)
                l.position[k] = P[k] + n[k] * R.u(0.05, 1.5) * scale + R.u(-0.2, 0.2) * scale;
        }
        F.lt.push_back(l);
    }
    F.prepare();
    return F;
}

// One frame from a frame file; 0, or the exit status of a file that cannot be used.
inline int read_frame(const char* path, Frame& F) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) return 4;
    unsigned W = 0, H = 0, ns = 0, np = 0, nl = 0;
    if (std::fscanf(f, "%u %u %la %la %la %la %la %u %u %u", &W, &H, &F.cam.position[0],
                    &F.cam.position[1], &F.cam.position[2], &F.cam.focal, &F.bias, &ns, &np,
                    &nl) != 10)
        return 4;
    if (W == 0 || H == 0 || ns < 1 || ns > 63 || np < 1 || np > unsigned(kShadowTabPlanes) ||
        nl < 1 || nl > unsigned(kShadowTabLights))
        return 4;
    F.cam.width = W;
    F.cam.height = H;
    F.cam.aa_samples = 1;
    F.sph.resize(ns);
    F.pl.resize(np);
    F.lt.resize(nl);
    for (auto& s : F.sph)
        if (std::fscanf(f, "%la %la %la %la", &s.center[0], &s.center[1], &s.center[2],
                        &s.radius) != 4)
            return 4;
    for (auto& p : F.pl)
        if (std::fscanf(f, "%la %la %la %la %la %la", &p.point[0], &p.point[1], &p.point[2],
                        &p.normal[0], &p.normal[1], &p.normal[2]) != 6)
            return 4;
    for (auto& l : F.lt)
        if (std::fscanf(f, "%la %la %la", &l.position[0], &l.position[1], &l.position[2]) != 3)
            return 4;
    std::fclose(f);
    set_rows(F, 0, 0, 1);
    F.prepare();
    return 0;
}

// s_pln's fourth word per plane, as pk_build_image forms it: the core flag and |n|₁ ≤ 2
inline std::vector<double> plane_flags(const Frame& F) {
    const size_t np = F.pl.size();
    std::vector<double> pln(4 * np, 0.0);
    for (size_t i = 0; i < np; ++i) {
        const double* o = &F.planes[8 * i];
        const double n1 = std::fabs(o[3]) + std::fabs(o[4]) + std::fabs(o[5]);
        pln[4 * i + 3] = o[7] != 0.0 && n1 <= 2.0 ? 1.0 : 0.0;
    }
    return pln;
}

// (class_main's mutants: the class taken on two kept planes, hidden and leading decided on one
// corner, the kept plane's index off by one)

enum ClassMutant { kClsNone, kClsTwo, kClsHide, kClsIndex };

// the class word of the tile at (x0, yl0), as the table kernel forms it; *all_zero: the tile has
// an entry and every light's shadow word is 0; *single: the word the tile would get if they were
inline unsigned long long class_word(const Frame& F, uint32_t x0, uint32_t yl0, ClassMutant mut,
                                     bool* all_zero, unsigned long long* single) {
    const int ns = static_cast<int>(F.sph.size()), np = static_cast<int>(F.pl.size());
    const int nl = static_cast<int>(F.lt.size());
    const double hw = static_cast<double>(F.cam.width) / 2.0,
                 hh = static_cast<double>(F.cam.height) / 2.0, dz = cam_dz(F.cam);
    const ConeRect q = cone_tile_rect(x0, yl0, F.cam.width, F.rp);
    const uint64_t cone = tile_cone_mask(F, x0, yl0);
    ShadowBound<> B;
    B.n = 0;
    B.ok = false;
    if (cone == 0) {
        if (mut == kClsHide)
            B = shadow_tile_bound<kShadowTabPlanes, 4, 1, true>(q, hw, hh, F.cam.position, dz,
                                                                F.planes.data(), np, F.bias);
        else
            B = shadow_tile_bound(q, hw, hh, F.cam.position, dz, F.planes.data(), np, F.bias);
    }
    unsigned long long words[kShadowTabLights];
    *all_zero = true;
    for (int l = 0; l < nl; ++l) {
        words[l] = shadow_tile_word(B, F.lt[l].position, F.bias, F.centre.data(), 3,
                                    F.terms.data() + 7, 8, ns);
        *all_zero = *all_zero && words[l] == 0;
    }
    const std::vector<double> pln = plane_flags(F);
    const unsigned long long none[kShadowTabLights] = {0, 0, 0, 0};
    auto word = [&](const unsigned long long* w) {
        switch (mut) {
            case kClsTwo:
                return tile_class_word<kShadowTabPlanes, 2, 0>(cone, B, w, nl, pln.data(), np);
            case kClsIndex:
                return tile_class_word<kShadowTabPlanes, 1, 1>(cone, B, w, nl, pln.data(), np);
            default: return tile_class_word<kShadowTabPlanes>(cone, B, w, nl, pln.data(), np);
        }
    };
    *single = word(none);
    return word(words);
}
