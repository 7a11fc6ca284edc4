// class_main.cpp — stand-alone host check of the tile class words (tile_class_word,
// csrc/rt_shadow_table.hpp), built and run by tests/test_tile_class_host.py against the C oracle
// (oracle/rt_oracle.c).  The random frames, the frame file, the oracle's shadow rays and the class
// word itself (class_word) are tests/host_frame.hpp's.
//
//   class_main prop SEED CASES [MUTANT]
//       For every tile that meets the class's geometric conditions (empty cone mask, at most one
//       kept plane that leads, a valid oriented normal: `single`) and every lane pixel of it
//       (clamped into the image as the kernel clamps): oracle_closest returns the class's plane,
//       or a miss for a sky tile.  For every uniform tile (those whose shadow words are all zero
//       as well: the class word) no shadow ray the oracle casts from it has a sphere root in
//       [1e-6, maxDist].  Anything else counts as a violation.  MUTANT: none (default), two (the
//       class taken on two kept planes), hide (hidden and leading decided on one corner), index
//       (the kept plane's index off by one).
//   class_main frame FILE
//       one frame of a real scene (shadow_main's file format): tiles, uniform tiles, workgroups
//       (two waves side by side) whose tiles are all uniform, and the violations.
// Exit status 0 only when every property holds (mutants: always 0, the caller reads
// `violations`).
#include "../host_frame.hpp"

struct ClassTally {
    uint64_t tiles = 0, single = 0, uniform = 0, sky = 0, zero_words = 0, workgroups = 0,
             uniform_wgs = 0;
    uint64_t pixels = 0, rays = 0, violations = 0;
};

static void check_class_frame(const Frame& F, ClassMutant mut, int tag, ClassTally& T) {
    const o_scene sc = F.scene();
    const int ns = static_cast<int>(F.sph.size());
    const size_t nl = F.lt.size();
    // the launch's wave tiles: 16-pixel workgroup columns of two waves, padded rows
    const uint32_t gx = (F.cam.width + 15) / 16, gy = (F.rp.rows + 7) / 8;
    Shadow S;
    for (uint32_t ty = 0; ty < gy; ++ty)
        for (uint32_t wx = 0; wx < gx; ++wx) {
            ++T.workgroups;
            int uni = 0;
            for (uint32_t w = 0; w < 2; ++w) {
                const uint32_t x0 = 8 * (2 * wx + w), yl0 = 8 * ty;
                ++T.tiles;
                bool zero = false;
                unsigned long long geo = kTileGeneral;
                const unsigned long long cls = class_word(F, x0, yl0, mut, &zero, &geo);
                T.zero_words += zero;
                if (geo == kTileGeneral) continue;
                ++T.single;
                T.sky += geo == kTileSky;
                uni += cls != kTileGeneral;
                T.uniform += cls != kTileGeneral;
                for (uint32_t l = 0; l < 64; ++l) {
                    uint32_t x, y;
                    bool valid;
                    lane_pixel(F, x0, yl0, l % 8, l / 8, x, y, valid);
                    double ray[6], out[7];
                    int32_t index = -1;
                    oracle_get_ray(&F.cam, x, y, 0, 0, 0, ray);
                    const int type = oracle_closest(&sc, ray, out, &index);
                    ++T.pixels;
                    const bool same = geo == kTileSky
                                          ? type == 0
                                          : type == 2 && static_cast<unsigned long long>(index) ==
                                                             geo - kTilePlane0;
                    if (!same) {
                        if (T.violations++ < 10)
                            std::fprintf(stderr,
                                         "case %d: %ux%u tile (%u,%u) class %llu pixel (%u,%u): "
                                         "oracle type %d index %d\n",
                                         tag, F.cam.width, F.cam.height, x0, yl0, geo, x, y, type,
                                         index);
                        continue;
                    }
                    if (type == 0 || cls == kTileGeneral) continue;
                    pixel_shadow(F, sc, x, y, S);
                    for (size_t k = 0; k < nl; ++k) {
                        if (!S.cast[k]) continue;
                        ++T.rays;
                        for (int i = 0; i < ns; ++i) {
                            if (!shadow_ray_meets(S.so, S.L[k], S.max_dist[k], F.sph[i])) continue;
                            if (T.violations++ < 10)
                                std::fprintf(stderr,
                                             "case %d: tile (%u,%u) pixel (%u,%u) light %zu: "
                                             "sphere %d shadows a uniform tile\n",
                                             tag, x0, yl0, x, y, k, i);
                        }
                    }
                }
            }
            T.uniform_wgs += uni == 2;
        }
}

static void print_tally(const char* what, int cases, const ClassTally& T) {
    std::printf("%s cases %d tiles %" PRIu64 " single %" PRIu64 " uniform %" PRIu64 " sky %" PRIu64
                " zero_words %" PRIu64 " workgroups %" PRIu64 " uniform_wgs %" PRIu64
                " pixels %" PRIu64 " rays %" PRIu64 " violations %" PRIu64 "\n",
                what, cases, T.tiles, T.single, T.uniform, T.sky, T.zero_words, T.workgroups, T.uniform_wgs,
                T.pixels, T.rays, T.violations);
}

static int run_class_prop(uint64_t seed, int cases, ClassMutant mut) {
    Rng R{seed};
    ClassTally T;
    for (int c = 0; c < cases; ++c) {
        const Frame F = random_frame(R);
        check_class_frame(F, mut, c, T);
    }
    print_tally("prop", cases, T);
    if (mut != kClsNone) return 0;
    return T.violations ? 1 : 0;
}

static int run_class_frame(const char* path) {
    Frame F{};
    if (const int r = read_frame(path, F)) return r;
    ClassTally T;
    check_class_frame(F, kClsNone, 0, T);
    print_tally("frame", 1, T);
    return T.violations ? 1 : 0;
}

int main(int argc, char** argv) {
    if ((argc == 4 || argc == 5) && !std::strcmp(argv[1], "prop")) {
        ClassMutant mut = kClsNone;
        if (argc == 5) {
            if (!std::strcmp(argv[4], "two")) mut = kClsTwo;
            else if (!std::strcmp(argv[4], "hide")) mut = kClsHide;
            else if (!std::strcmp(argv[4], "index")) mut = kClsIndex;
            else if (std::strcmp(argv[4], "none")) return 64;
        }
        return run_class_prop(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]), mut);
    }
    if (argc == 3 && !std::strcmp(argv[1], "frame")) return run_class_frame(argv[2]);
    std::fprintf(stderr,
                 "usage: class_main prop SEED CASES [none|two|hide|index] | class_main frame "
                 "FILE\n");
    return 64;
}
