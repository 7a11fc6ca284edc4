// rt_cone_table.hpp — the camera-cone candidate mask of one wave tile, formed outside the packet
// kernel (rt_packet.hip packet_cone_table_kernel, one lane per tile) and read by the kernel with
// one scalar load instead of being reduced by every wave (rt_packet_kernel.hpp).  The mask is a
// function of the scene, the camera, the launch's row plan and the tile only.
//
// Plain C++: no device builtin, so a host program can call every function here
// (tests/test_cone_table_host.py builds one and checks the masks against FP64 intersections).
//
// The bound.  Every camera ray of the tile is d = unit(v), v = (x − W/2 − cam.x,
// H/2 − y − cam.y, dz) (Camera::getRay, Math.h:99-121) for an integer pixel (x, y) of the tile's
// clamped pixel rectangle [x_lo, x_hi] × [y_lo, y_hi]; lanes past the image edge trace clamped
// in-image rays, which the clamped rectangle holds, and a block-cyclic row plan whose block is
// not a multiple of 8 gives rows inside the bounding interval of the tile's first and last row
// (image_row is increasing), a superset.  Rounding to nearest is monotone, so every ray's v.x
// lies between the rounded v.x of x_lo and of x_hi, formed here by the same FP64 expression, and
// v.y likewise: every v is a point of the rectangle R spanned by the four corner vectors in the
// plane z = dz, exactly.  For dz ≠ 0 and an axis a, the points p of that plane with
// angle(p, a) ≤ θ form, for θ < 90°, the section of a convex cone by the plane: a convex set.
// So the angle to the axis is quasi-convex on the plane and its maximum over R is taken at a
// corner: cos angle(v, a) ≥ the minimum c of the four corner cosines, for any axis, as long as
// c > 0.  The axis is the unit vector of R's centre.
//
// Rounding budget.  c is formed in FP64 (each corner cosine within 1e-15 of its exact value:
// two normalisations and a dot product of unit vectors), a ray's own direction is the FP64
// normalisation of v (within 4e-16 of the exact unit vector), and c goes through the same FP32
// conversion the kernel's wave minimum goes through (|c| ≤ 1 + 2ε, off by ≤ 6e-8).  The same
// 1e-7 is taken off as in the kernel: 6e-8 for the conversion, and the 4e-8 left over cover the
// FP64 terms 10^7 times.  cone_keeps is cull_cone's test (rt_packet_device.hpp) with its cs
// rounded down, sn rounded up and 2e-5·|C − o| of slack; the axis is rounded to FP32 like the
// kernel's.  The per-sphere terms are cone_terms' (read from the packet image on the device; a
// host caller forms them with cone_sphere_terms, whose sqrtf differs from v_sqrt_f32 by ≤ 1 ulp,
// inside the slack).  dz == 0, a non-finite value or c ≤ 0: no bound, every sphere is kept.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_CT_HD __host__ __device__
#else
#define RT_CT_HD
#endif

namespace rtamd {

struct ConeRowPlan {  // TraceParams' row plan
    uint32_t row0, rows, row_block, row_stride;
};
RT_CT_HD inline uint32_t cone_image_row(const ConeRowPlan& r, uint32_t yl) {
    if (r.row_block == 0) return r.row0 + yl;
    return r.row0 + (yl / r.row_block) * r.row_stride + yl % r.row_block;
}

// The clamped pixel rectangle of the wave tile whose first pixel is (x0, first local row yl0).
struct ConeRect {
    uint32_t x_lo, x_hi, y_lo, y_hi;
};
RT_CT_HD inline ConeRect cone_tile_rect(uint32_t x0, uint32_t yl0, uint32_t width,
                                        const ConeRowPlan& r) {
    ConeRect q;
    q.x_lo = x0 < width ? x0 : width - 1;
    q.x_hi = x0 + 7 < width ? x0 + 7 : width - 1;
    q.y_lo = cone_image_row(r, yl0 < r.rows ? yl0 : r.rows - 1);
    q.y_hi = cone_image_row(r, yl0 + 7 < r.rows ? yl0 + 7 : r.rows - 1);
    return q;
}

struct ConeBound {
    float ax, ay, az;  // the axis, rounded to FP32
    float cs, sn;      // cos θ rounded down, sin θ rounded up (cull_cone)
    bool ok;           // false: no bound, keep every sphere
};

// half_w, half_h, dz: camera_consts (rt_internal.hpp); cam_x, cam_y: the camera position.
RT_CT_HD inline ConeBound cone_tile_bound(const ConeRect& q, double half_w, double half_h,
                                          double cam_x, double cam_y, double dz) {
    ConeBound B;
    B.ax = B.ay = B.az = B.cs = B.sn = 0.0f;
    B.ok = false;
    // the kernel's expression: sx = x − W/2, sy = H/2 − y, v = (sx − cam.x, sy − cam.y, dz)
    const double vx0 = (static_cast<double>(q.x_lo) - half_w) - cam_x;
    const double vx1 = (static_cast<double>(q.x_hi) - half_w) - cam_x;
    const double vy0 = (half_h - static_cast<double>(q.y_lo)) - cam_y;
    const double vy1 = (half_h - static_cast<double>(q.y_hi)) - cam_y;
    if (!(dz != 0.0) || !isfinite(dz) || !isfinite(vx0) || !isfinite(vx1) || !isfinite(vy0) ||
        !isfinite(vy1))
        return B;
    const double cx = 0.5 * vx0 + 0.5 * vx1, cy = 0.5 * vy0 + 0.5 * vy1;
    const double cl = sqrt(cx * cx + cy * cy + dz * dz);
    if (!(cl > 0.0) || !isfinite(cl)) return B;
    const double ax = cx / cl, ay = cy / cl, az = dz / cl;
    double c = 2.0;
    for (int k = 0; k < 4; ++k) {
        const double vx = (k & 1) ? vx1 : vx0, vy = (k & 2) ? vy1 : vy0;
        const double l = sqrt(vx * vx + vy * vy + dz * dz);
        if (!(l > 0.0) || !isfinite(l)) return B;
        const double ck = (vx / l) * ax + (vy / l) * ay + (dz / l) * az;
        if (ck < c) c = ck;  // (finite: l is finite and positive)
    }
    const double cos_min = static_cast<double>(static_cast<float>(c)) - 1e-7;
    if (!(isfinite(cos_min) && cos_min > 0.0)) return B;  // cones narrower than 90° only
    B.cs = static_cast<float>(cos_min) * (1.0f - 1e-6f);
    const float s2 = 1.0f - B.cs * B.cs;
    B.sn = sqrtf(s2 > 0.0f ? s2 : 0.0f) * (1.0f + 1e-5f);
    B.ax = static_cast<float>(ax);
    B.ay = static_cast<float>(ay);
    B.az = static_cast<float>(az);
    B.ok = true;
    return B;
}

// cull_cone's per-sphere test over cone_terms' eight floats t = vx vy vz q | rr dv slack r.
RT_CT_HD inline bool cone_keeps(const ConeBound& B, const float* t) {
    const float q = t[3], rr = t[4], dv = t[5], slack = t[6];
    return !(q > -B.cs * dv + slack) ||
           !(t[0] * B.ax + t[1] * B.ay + t[2] * B.az < B.cs * q - B.sn * rr - slack);
}

// cone_terms (rt_packet_device.hpp) for a host caller: s = cx cy cz r², o = the camera.
RT_CT_HD inline void cone_sphere_terms(const double* s, const double* o, float* out) {
    const float r = static_cast<float>(sqrt(s[3])) * (1.0f + 1e-6f);
    const float vx = static_cast<float>(s[0] - o[0]), vy = static_cast<float>(s[1] - o[1]),
                vz = static_cast<float>(s[2] - o[2]);
    const float dv2 = vx * vx + vy * vy + vz * vz;
    const float rr = r * (1.0f + static_cast<float>(1e-4));
    const float dv = sqrtf(dv2);
    const bool always = !(dv > 1.01f * rr) || !(dv <= static_cast<float>(1e5) * r);
    out[0] = vx;
    out[1] = vy;
    out[2] = vz;
    out[3] = always ? nanf("") : sqrtf(dv2 - rr * rr);
    out[4] = rr;
    out[5] = dv;
    out[6] = 2e-5f * dv;
    out[7] = r;
}

// The tile's mask over spheres [0, ns), ns ≤ 64: `terms` + stride_floats · i are sphere i's
// eight floats.
RT_CT_HD inline uint64_t cone_tile_mask(const ConeBound& B, const float* terms,
                                        int stride_floats, int ns) {
    const uint64_t all = ns >= 64 ? ~0ull : ((1ull << ns) - 1ull);
    if (!B.ok) return all;
    uint64_t m = 0;
    for (int i = 0; i < ns && i < 64; ++i)
        if (cone_keeps(B, terms + static_cast<long>(stride_floats) * i)) m |= 1ull << i;
    return m;
}

}  // namespace rtamd
