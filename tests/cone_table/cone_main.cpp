// cone_main.cpp — stand-alone host check of the camera-cone mask table (csrc/rt_cone_table.hpp),
// built and run by tests/test_cone_table_host.py against the C oracle (oracle/rt_oracle.c).
//
//   cone_main prop SEED CASES   random cameras, frames, row plans and spheres: for every tile and
//                               every pixel of it, a sphere the oracle's FP64 intersection hits
//                               (root >= 1e-6) must have its bit in the tile's mask
//   cone_main frame FILE        total popcount over one frame of the table's masks and of the
//                               per-wave cull restated (lane (4,4) axis, per-pixel minimum);
//                               FILE: width height cam(3) focal, then cx cy cz r per sphere
// Exit status 0 only when every property holds.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_cone_table.hpp"
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
    uint32_t below(uint32_t n) { return static_cast<uint32_t>(next() % n); }
};

struct Frame {
    o_camera cam;
    ConeRowPlan rp;
    std::vector<o_sphere> sph;
};

static double cam_dz(const o_camera& c) { return (c.position[2] + c.focal) - c.position[2]; }

// the table's mask of the tile at (x0, yl0)
static uint64_t table_mask(const Frame& F, uint32_t x0, uint32_t yl0) {
    const int ns = static_cast<int>(F.sph.size());
    std::vector<float> terms(8 * static_cast<size_t>(ns));
    for (int i = 0; i < ns; ++i) {
        const double s[4] = {F.sph[i].center[0], F.sph[i].center[1], F.sph[i].center[2],
                             F.sph[i].radius * F.sph[i].radius};
        cone_sphere_terms(s, F.cam.position, &terms[8 * static_cast<size_t>(i)]);
    }
    const ConeBound B = cone_tile_bound(cone_tile_rect(x0, yl0, F.cam.width, F.rp),
                                        static_cast<double>(F.cam.width) / 2.0,
                                        static_cast<double>(F.cam.height) / 2.0,
                                        F.cam.position[0], F.cam.position[1], cam_dz(F.cam));
    return cone_tile_mask(B, terms.data(), 8, ns);
}

// the pixel lane (lx, ly) of the tile traces (clamped into the image, as the kernel clamps)
static void lane_pixel(const Frame& F, uint32_t x0, uint32_t yl0, uint32_t lx, uint32_t ly,
                       uint32_t& x, uint32_t& y, bool& valid) {
    const uint32_t xx = x0 + lx, yl = yl0 + ly;
    valid = xx < F.cam.width && yl < F.rp.rows;
    x = xx < F.cam.width ? xx : F.cam.width - 1;
    y = cone_image_row(F.rp, yl < F.rp.rows ? yl : F.rp.rows - 1);
}

// today's per-wave cull restated: axis = lane (4,4)'s direction, cosine = the FP32 minimum over
// the 64 lanes less 1e-7, then cull_cone's test
static uint64_t wave_mask(const Frame& F, uint32_t x0, uint32_t yl0) {
    const int ns = static_cast<int>(F.sph.size());
    const uint64_t all = ns >= 64 ? ~0ull : ((1ull << ns) - 1ull);
    double ray[6], ax[6];
    uint32_t x, y;
    bool valid;
    lane_pixel(F, x0, yl0, 4, 4, x, y, valid);
    oracle_get_ray(&F.cam, x, y, 0, 0, 0, ax);
    float cmin = INFINITY;
    for (uint32_t l = 0; l < 64; ++l) {
        lane_pixel(F, x0, yl0, l % 8, l / 8, x, y, valid);
        oracle_get_ray(&F.cam, x, y, 0, 0, 0, ray);
        const float c = static_cast<float>(ray[3] * ax[3] + ray[4] * ax[4] + ray[5] * ax[5]);
        if (!(c >= cmin)) cmin = c;
    }
    const double cos_min = static_cast<double>(cmin) - 1e-7;
    if (!(std::isfinite(cos_min) && cos_min > 0.0)) return all;
    ConeBound B;
    B.cs = static_cast<float>(cos_min) * (1.0f - 1e-6f);
    const float s2 = 1.0f - B.cs * B.cs;
    B.sn = sqrtf(s2 > 0.0f ? s2 : 0.0f) * (1.0f + 1e-5f);
    B.ax = static_cast<float>(ax[3]);
    B.ay = static_cast<float>(ax[4]);
    B.az = static_cast<float>(ax[5]);
    B.ok = true;
    uint64_t m = 0;
    for (int i = 0; i < ns; ++i) {
        const double s[4] = {F.sph[i].center[0], F.sph[i].center[1], F.sph[i].center[2],
                             F.sph[i].radius * F.sph[i].radius};
        float t[8];
        cone_sphere_terms(s, F.cam.position, t);
        if (cone_keeps(B, t)) m |= 1ull << i;
    }
    return m;
}

static void set_rows(Frame& F, uint32_t begin, uint32_t block, uint32_t cycle) {
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

static Frame random_frame(Rng& R) {
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
    F.cam.focal = std::exp(R.u(std::log(0.05), std::log(100.0)));
    switch (R.below(4)) {
        case 0: set_rows(F, 0, 0, 1); break;
        case 1: set_rows(F, 1, 2, 2); break;
        case 2: set_rows(F, 0, 3, 3); break;
        default: set_rows(F, 0, 8, 2); break;
    }
    const int ns = 3 + static_cast<int>(R.below(10));
    for (int i = 0; i < ns; ++i) {
        // aim at a point of the screen, on a pixel, a tile corner or anywhere
        double px = R.u(-2.0, W + 2.0), py = R.u(-2.0, H + 2.0);
        const uint32_t snap = R.below(4);
        if (snap == 0) px = std::floor(px), py = std::floor(py);
        if (snap == 1) px = 8.0 * std::floor(px / 8.0) - 0.5, py = 8.0 * std::floor(py / 8.0) - 0.5;
        const double v[3] = {px - W / 2.0 - F.cam.position[0], H / 2.0 - py - F.cam.position[1],
                             F.cam.focal};
        const double vl = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        double t = std::exp(R.u(std::log(0.5), std::log(500.0))), r, sign = 1.0;
        const double pixel = t / vl;  // a pixel's width at distance t, about
        switch (R.below(8)) {
            case 0: r = pixel * R.u(0.05, 0.5); break;                  // sub-pixel
            case 1: case 2: r = pixel * R.u(1.0, 12.0); break;          // a few pixels
            case 3: r = t * R.u(0.3, 0.95); break;                      // screen-filling
            case 4: r = t * R.u(0.05, 0.5); sign = -1.0; break;         // behind the camera
            case 5: r = t * R.u(1.05, 30.0); break;                     // around the camera
            case 6: r = R.u(0.01, 1.0); t = r * std::pow(10.0, R.u(5.0, 7.0)); break;  // far
            default: r = t / R.u(1.0005, 1.2); break;                   // camera next to it
        }
        o_sphere s{};
        for (int k = 0; k < 3; ++k) s.center[k] = F.cam.position[k] + sign * t * v[k] / vl;
        s.radius = r;
        F.sph.push_back(s);
    }
    return F;
}

static int run_prop(uint64_t seed, int cases) {
    Rng R{seed};
    uint64_t tiles = 0, partial = 0, hits = 0, missed = 0, pixels = 0;
    for (int c = 0; c < cases; ++c) {
        const Frame F = random_frame(R);
        const int ns = static_cast<int>(F.sph.size());
        const uint64_t all = (1ull << ns) - 1ull;
        // the launch's wave tiles: 16-pixel workgroup columns of two waves, padded rows
        const uint32_t gx = (F.cam.width + 15) / 16, gy = (F.rp.rows + 7) / 8;
        for (uint32_t ty = 0; ty < gy; ++ty)
            for (uint32_t tx = 0; tx < 2 * gx; ++tx) {
                const uint32_t x0 = 8 * tx, yl0 = 8 * ty;
                const uint64_t m = table_mask(F, x0, yl0);
                ++tiles;
                if (m != 0 && m != all) ++partial;
                for (uint32_t l = 0; l < 64; ++l) {
                    uint32_t x, y;
                    bool valid;
                    lane_pixel(F, x0, yl0, l % 8, l / 8, x, y, valid);
                    double ray[6];
                    oracle_get_ray(&F.cam, x, y, 0, 0, 0, ray);
                    ++pixels;
                    for (int i = 0; i < ns; ++i) {
                        double t = 0.0;
                        if (!oracle_sphere_intersect(ray, &F.sph[i], &t) || !(t >= 1e-6)) continue;
                        ++hits;
                        if (!((m >> i) & 1ull)) {
                            if (missed++ < 10)
                                std::fprintf(stderr,
                                             "case %d: %ux%u tile (%u,%u) pixel (%u,%u) hits sphere "
                                             "%d at t=%.17g, bit clear (mask %016" PRIx64 ")\n",
                                             c, F.cam.width, F.cam.height, x0, yl0, x, y, i, t, m);
                        }
                    }
                }
            }
    }
    std::printf("prop cases %d tiles %" PRIu64 " partial %" PRIu64 " pixels %" PRIu64
                " hits %" PRIu64 " missed %" PRIu64 "\n",
                cases, tiles, partial, pixels, hits, missed);
    if (missed) return 1;
    if (hits < 10000) return 2;
    if (partial * 10 < tiles) return 3;
    return 0;
}

static int run_frame(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) return 4;
    Frame F{};
    unsigned W = 0, H = 0;
    if (std::fscanf(f, "%u %u %la %la %la %la", &W, &H, &F.cam.position[0], &F.cam.position[1],
                    &F.cam.position[2], &F.cam.focal) != 6)
        return 4;
    F.cam.width = W;
    F.cam.height = H;
    F.cam.aa_samples = 1;
    o_sphere s{};
    while (std::fscanf(f, "%la %la %la %la", &s.center[0], &s.center[1], &s.center[2],
                       &s.radius) == 4)
        F.sph.push_back(s);
    std::fclose(f);
    if (F.sph.empty() || F.sph.size() > 64 || W == 0 || H == 0) return 4;
    set_rows(F, 0, 0, 1);
    uint64_t tab = 0, wave = 0, tiles = 0, superset_breaks = 0;
    for (uint32_t yl0 = 0; yl0 < H; yl0 += 8)
        for (uint32_t x0 = 0; x0 < W; x0 += 8) {
            const uint64_t a = table_mask(F, x0, yl0), b = wave_mask(F, x0, yl0);
            tab += static_cast<uint64_t>(__builtin_popcountll(a));
            wave += static_cast<uint64_t>(__builtin_popcountll(b));
            superset_breaks += (a & ~b) != 0;
            ++tiles;
        }
    std::printf("frame tiles %" PRIu64 " table_popcount %" PRIu64 " wave_popcount %" PRIu64
                " tiles_where_table_keeps_more %" PRIu64 "\n",
                tiles, tab, wave, superset_breaks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && argv[1][0] == 'p')
        return run_prop(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]));
    if (argc == 3 && argv[1][0] == 'f') return run_frame(argv[2]);
    std::fprintf(stderr, "usage: cone_main prop SEED CASES | cone_main frame FILE\n");
    return 64;
}
