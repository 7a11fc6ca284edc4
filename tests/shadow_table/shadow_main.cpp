// shadow_main.cpp — stand-alone host check of the shadow-cull mask table
// (csrc/rt_shadow_table.hpp), built and run by tests/test_shadow_table_host.py against the C
// oracle (oracle/rt_oracle.c).
//
//   shadow_main prop SEED CASES [MUTANT]
//       random cameras, frames, row plans, planes, spheres and lights.  For every tile with an
//       entry, every pixel of it and every light: the oracle's closest hit, the shadow ray as the
//       oracle's direct lighting forms it, and its FP64 intersection with every sphere; a sphere
//       with a root in [1e-6, maxDist] must have its bit in the tile's word, and a pixel whose
//       oracle hit is a sphere must not lie in a tile with an entry (both count as `missed`).
//       MUTANT: none (default), corner (the ball from one corner instead of four), nobias (no
//       bias allowance at all), nobias_r (only R's bias term dropped: see run_prop), hide (a plane
//       hidden on the strength of one corner).
//   shadow_main frame FILE
//       one frame of a real scene: tiles, entries and the total popcount of the table's words
//       against a per-tile emulation of origin_ball + cull_capsule on the same tiles.
//       FILE: width height cam(3) focal bias ns np nl, then cx cy cz r per sphere, px py pz nx ny
//       nz per plane, x y z per light (hex floats).
// Exit status 0 only when every property holds (mutants: always 0, the caller reads `missed`).
#include "../host_frame.hpp"

enum Mutant { kNone, kCorner, kNoBias, kNoBiasR, kHide };

// the table's words of the tile at (x0, yl0), one per light; false: the tile has no entry
static bool table_words(const Frame& F, uint32_t x0, uint32_t yl0, Mutant mut, uint64_t* words) {
    const int ns = static_cast<int>(F.sph.size()), np = static_cast<int>(F.pl.size());
    const double hw = static_cast<double>(F.cam.width) / 2.0,
                 hh = static_cast<double>(F.cam.height) / 2.0, dz = cam_dz(F.cam);
    const ConeRect q = cone_tile_rect(x0, yl0, F.cam.width, F.rp);
    const uint64_t cone = tile_cone_mask(F, x0, yl0);
    ShadowBound<> B;
    B.n = 0;
    B.ok = false;
    if (cone == 0) {
        const double* pl = F.planes.data();
        switch (mut) {
            case kCorner: B = shadow_tile_bound<kShadowTabPlanes, 1, 4, true>(q, hw, hh, F.cam.position, dz, pl, np, F.bias); break;
            case kNoBias:
            case kNoBiasR: B = shadow_tile_bound<kShadowTabPlanes, 4, 4, false>(q, hw, hh, F.cam.position, dz, pl, np, F.bias); break;
            case kHide: B = shadow_tile_bound<kShadowTabPlanes, 4, 1, true>(q, hw, hh, F.cam.position, dz, pl, np, F.bias); break;
            default: B = shadow_tile_bound(q, hw, hh, F.cam.position, dz, pl, np, F.bias); break;
        }
    }
    bool entry = true;
    for (size_t l = 0; l < F.lt.size(); ++l) {
        words[l] = shadow_tile_word(B, F.lt[l].position, mut == kNoBias ? 0.0 : F.bias,
                                    F.centre.data(), 3, F.terms.data() + 7, 8, ns);
        entry = entry && words[l] != kShadowNoWord;
    }
    return entry;
}

// One frame's tiles: the properties and the counts.
struct Tally {
    uint64_t tiles = 0, entries = 0, partial = 0, pixels = 0, hits = 0, missed = 0;
    uint64_t table_pop = 0, wave_pop = 0, cone_blocked = 0;
};
static void check_frame(const Frame& F, Mutant mut, bool emulate, int tag, Tally& T) {
    const o_scene sc = F.scene();
    const int ns = static_cast<int>(F.sph.size());
    const size_t nl = F.lt.size();
    const uint64_t all = (1ull << ns) - 1ull;
    // the launch's wave tiles: 16-pixel workgroup columns of two waves, padded rows
    const uint32_t gx = (F.cam.width + 15) / 16, gy = (F.rp.rows + 7) / 8;
    std::vector<Shadow> lanes(64);
    for (uint32_t ty = 0; ty < gy; ++ty)
        for (uint32_t tx = 0; tx < 2 * gx; ++tx) {
            const uint32_t x0 = 8 * tx, yl0 = 8 * ty;
            uint64_t words[kShadowTabLights];
            ++T.tiles;
            if (!table_words(F, x0, yl0, mut, words)) {
                T.cone_blocked += tile_cone_mask(F, x0, yl0) != 0;
                continue;
            }
            ++T.entries;
            bool part = false;
            for (size_t l = 0; l < nl; ++l) {
                part = part || (words[l] != 0 && words[l] != all);
                T.table_pop += static_cast<uint64_t>(__builtin_popcountll(words[l]));
            }
            T.partial += part;
            bool valid[64];
            for (uint32_t l = 0; l < 64; ++l) {
                uint32_t x, y;
                lane_pixel(F, x0, yl0, l % 8, l / 8, x, y, valid[l]);
                pixel_shadow(F, sc, x, y, lanes[l]);
                ++T.pixels;
                if (lanes[l].type == 1) {  // a sphere seen from a tile with an entry
                    if (T.missed++ < 10)
                        std::fprintf(stderr, "case %d: tile (%u,%u) pixel (%u,%u) sees a sphere\n",
                                     tag, x0, yl0, x, y);
                    continue;
                }
                for (size_t k = 0; k < nl; ++k) {
                    if (!lanes[l].cast[k]) continue;
                    for (int i = 0; i < ns; ++i) {
                        if (!shadow_ray_meets(lanes[l].so, lanes[l].L[k], lanes[l].max_dist[k],
                                              F.sph[i]))
                            continue;
                        ++T.hits;
                        if ((words[k] >> i) & 1ull) continue;
                        if (T.missed++ < 10)
                            std::fprintf(stderr,
                                         "case %d: %ux%u tile (%u,%u) pixel (%u,%u) light %zu: "
                                         "sphere %d shadows it, bit clear (word %016" PRIx64 ")\n",
                                         tag, F.cam.width, F.cam.height, x0, yl0, x, y, k, i,
                                         words[k]);
                    }
                }
            }
            if (!emulate) continue;
            // origin_ball + cull_capsule of this wave restated: the ball around the first casting
            // lane's origin, R the FP32 maximum of the distances rounded up
            for (size_t k = 0; k < nl; ++k) {
                int first = -1;
                float Rw = 0.0f;
                for (int l = 0; l < 64; ++l) {
                    if (!valid[l] || !lanes[l].cast[k]) continue;
                    if (first < 0) first = l;
                    const float dx = static_cast<float>(lanes[l].so[0] - lanes[first].so[0]),
                                dy = static_cast<float>(lanes[l].so[1] - lanes[first].so[1]),
                                dz = static_cast<float>(lanes[l].so[2] - lanes[first].so[2]);
                    const float r = sqrtf(dx * dx + dy * dy + dz * dz) * (1.0f + 1e-5f);
                    if (r > Rw) Rw = r;
                }
                if (first < 0) continue;
                for (int i = 0; i < ns; ++i)
                    T.wave_pop += shadow_keeps(lanes[first].so, Rw, F.lt[k].position, F.bias,
                                               &F.centre[3 * static_cast<size_t>(i)],
                                               F.terms[8 * static_cast<size_t>(i) + 7]);
            }
        }
}

// `nobias_r` drops only the |bias|·1.001 added to R.  It is reported, not asserted: the ball is
// around the hit points, the ray from so = hp + n·bias runs along (lpos − hp), so it stays within
// bias·|n| of the segment [hp, lpos], which the capsule test's own bias allowance already covers;
// `nobias` drops both allowances and must miss.
static int run_prop(uint64_t seed, int cases, Mutant mut) {
    Rng R{seed};
    Tally T;
    for (int c = 0; c < cases; ++c) {
        const Frame F = random_frame(R);
        check_frame(F, mut, false, c, T);
    }
    std::printf("prop cases %d tiles %" PRIu64 " entries %" PRIu64 " partial %" PRIu64
                " pixels %" PRIu64 " hits %" PRIu64 " missed %" PRIu64 " cone_blocked %" PRIu64 "\n",
                cases, T.tiles, T.entries, T.partial, T.pixels, T.hits, T.missed, T.cone_blocked);
    if (mut != kNone) return 0;
    if (T.missed) return 1;
    if (T.hits < 10000) return 2;
    if (2 * T.entries < T.tiles) return 3;
    if (10 * T.partial < T.entries) return 5;
    return 0;
}

static int run_frame(const char* path) {
    Frame F{};
    if (const int r = read_frame(path, F)) return r;
    Tally T;
    check_frame(F, kNone, true, 0, T);
    std::printf("frame tiles %" PRIu64 " entries %" PRIu64 " table_popcount %" PRIu64
                " wave_popcount %" PRIu64 " hits %" PRIu64 " missed %" PRIu64 "\n",
                T.tiles, T.entries, T.table_pop, T.wave_pop, T.hits, T.missed);
    return T.missed ? 1 : 0;
}

int main(int argc, char** argv) {
    if ((argc == 4 || argc == 5) && argv[1][0] == 'p') {
        Mutant mut = kNone;
        if (argc == 5) {
            if (!std::strcmp(argv[4], "corner")) mut = kCorner;
            else if (!std::strcmp(argv[4], "nobias")) mut = kNoBias;
            else if (!std::strcmp(argv[4], "nobias_r")) mut = kNoBiasR;
            else if (!std::strcmp(argv[4], "hide")) mut = kHide;
            else if (std::strcmp(argv[4], "none")) return 64;
        }
        return run_prop(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]), mut);
    }
    if (argc == 3 && argv[1][0] == 'f') return run_frame(argv[2]);
    std::fprintf(stderr,
                 "usage: shadow_main prop SEED CASES [none|corner|nobias|nobias_r|hide] | "
                 "shadow_main frame FILE\n");
    return 64;
}
