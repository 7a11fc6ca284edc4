// class_main.cpp — stand-alone host check of the tile class words (tile_class_word,
// csrc/rt_shadow_table.hpp), built and run by tests/test_tile_class_host.py against the C oracle
// (oracle/rt_oracle.c).  The random frames, the frame file and the oracle's shadow rays are
// tests/shadow_table/shadow_main.cpp's, included below with its main renamed.
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
//   class_main shadow ...
//       shadow_main's own command line.
// Exit status 0 only when every property holds (mutants: always 0, the caller reads
// `violations`).
#define main shadow_table_main
#include "../shadow_table/shadow_main.cpp"
#undef main

enum ClassMutant { kClsNone, kClsTwo, kClsHide, kClsIndex };

// the class word of the tile at (x0, yl0), as the table kernel forms it; *all_zero: the tile has
// an entry and every light's shadow word is 0; *single: the word the tile would get if they were
static unsigned long long class_word(const Frame& F, uint32_t x0, uint32_t yl0, ClassMutant mut,
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
    // s_pln's fourth word, as pk_build_image forms it: the core flag and |n|₁ ≤ 2
    std::vector<double> pln(4 * static_cast<size_t>(np), 0.0);
    for (int i = 0; i < np; ++i) {
        const double* o = &F.planes[8 * static_cast<size_t>(i)];
        const double n1 = std::fabs(o[3]) + std::fabs(o[4]) + std::fabs(o[5]);
        pln[4 * static_cast<size_t>(i) + 3] = o[7] != 0.0 && n1 <= 2.0 ? 1.0 : 0.0;
    }
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
    // (shadow_main's reader, through a frame file)
    std::FILE* f = std::fopen(path, "r");
    if (!f) return 4;
    Frame F{};
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
    ClassTally T;
    check_class_frame(F, kClsNone, 0, T);
    print_tally("frame", 1, T);
    return T.violations ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "shadow")) return shadow_table_main(argc - 1, argv + 1);
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
                 "usage: class_main prop SEED CASES [none|two|hide|index] | class_main frame FILE "
                 "| class_main shadow ...\n");
    return 64;
}
