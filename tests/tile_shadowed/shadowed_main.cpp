// shadowed_main.cpp — stand-alone host check of the shadowed-plane tiles (tile_shadowed_mark,
// tile_shadowed_entry and tile_list_run, csrc/rt_shadow_table.hpp: the rule and the three lists
// the table kernel's wavefronts follow), built and run by tests/test_tile_shadowed_host.py against
// the C oracle.  The random frames, the frame file and the oracle's shadow rays are
// tests/host_frame.hpp's.
//
//   shadowed_main prop SEED CASES [MUTANT]
//       For every frame: the table word of every tile as the table kernel forms it (class, keep
//       masks, shadowed mark), then the three lists, run by run.
//       - every lane pixel of a shadowed tile (clamped as the kernel clamps): oracle_closest
//         returns the plane the tile's list entry names;
//       - every shadow ray the oracle casts from such a pixel: every sphere it meets with a root
//         in [1e-6, maxDist] is in that light's shadow word;
//       - every tile is in exactly one of the uniform list, the shadowed list and a general wave
//         of a listed workgroup; nothing is listed twice; the counts are the class words';
//       - a workgroup is listed if and only if it has a tile that is neither uniform nor shadowed;
//       - every entry decodes to its tile, its plane and its keep masks.
//       MUTANT: none (default), noword (the shadowed class taken when a light has no word: a tile
//       that sees a sphere), index (the entry's plane index off by one), mixed (a workgroup with
//       a shadowed wave and a general wave is not listed).
//   shadowed_main frame FILE
//       the same on one frame of a real scene (shadow_main's file format).
//   shadowed_main census FILE
//       the frame's tiles by kind, the shadowed tiles by sphere candidates over all lights, and
//       the general workgroups with and without the shadowed list (profiles/
//       tile_shadowed_census.txt).
// Exit status 0 only when every property holds (mutants: always 0, the caller reads
// `violations`).
#include "../host_frame.hpp"

enum ShMutant { kShNone, kShNoWord, kShIndex, kShMixed };

// One tile's table entry as packet_cone_table_kernel forms it: the cone mask, the bound (only
// with an empty cone mask), the shadow words, the keep masks, the class and the shadowed mark.
struct TileWord {
    unsigned long long word;                   // class | keep masks | mark
    unsigned long long sw[kShadowTabLights];   // the shadow words
    unsigned keep[kShadowTabLights];           // the keep masks, formed here
    int plane;                                 // the bound's one kept plane (−1: none or several)
};
static TileWord table_word(const Frame& F, uint32_t x0, uint32_t yl0, ShMutant mut) {
    const int ns = static_cast<int>(F.sph.size()), np = static_cast<int>(F.pl.size());
    const int nl = static_cast<int>(F.lt.size());
    const double hw = static_cast<double>(F.cam.width) / 2.0,
                 hh = static_cast<double>(F.cam.height) / 2.0, dz = cam_dz(F.cam);
    const ConeRect q = cone_tile_rect(x0, yl0, F.cam.width, F.rp);
    const uint64_t cone = tile_cone_mask(F, x0, yl0);
    ShadowBound<> B, Bm;
    B.n = 0;
    B.ok = false;
    if (cone == 0)
        B = shadow_tile_bound(q, hw, hh, F.cam.position, dz, F.planes.data(), np, F.bias);
    Bm = B;  // (the noword mutant's: a bound for a tile that has no word)
    if (mut == kShNoWord && cone != 0)
        Bm = shadow_tile_bound(q, hw, hh, F.cam.position, dz, F.planes.data(), np, F.bias);
    TileWord W;
    for (int l = 0; l < kShadowTabLights; ++l) W.sw[l] = 0, W.keep[l] = 0;
    for (int l = 0; l < nl; ++l) {
        W.sw[l] = shadow_tile_word(B, F.lt[l].position, F.bias, F.centre.data(), 3,
                                   F.terms.data() + 7, 8, ns);
        W.keep[l] = shadow_plane_keep(B, F.lt[l].position, F.planes.data(), np, F.cam.position,
                                      F.bias);
    }
    const std::vector<double> pln = plane_flags(F);
    const unsigned long long cls =
        tile_class_word<kShadowTabPlanes>(cone, B, W.sw, nl, pln.data(), np);
    unsigned long long mark;
    if (mut == kShNoWord)
        mark = tile_shadowed_mark<kShadowTabPlanes, true>(cone, Bm, W.sw, nl, pln.data(), np);
    else if (mut == kShIndex)
        mark = tile_shadowed_mark<kShadowTabPlanes, false, 1>(cone, B, W.sw, nl, pln.data(), np);
    else
        mark = tile_shadowed_mark<kShadowTabPlanes>(cone, B, W.sw, nl, pln.data(), np);
    W.word = tile_class_pack(cls, W.keep, nl) | mark;
    W.plane = B.ok && B.n == 1 ? B.ball[0].plane : -1;
    return W;
}

struct ShTally {
    uint64_t tiles = 0, workgroups = 0, uniform = 0, shadowed = 0, listed = 0, general_wgs = 0,
             mixed = 0, cand1 = 0, cand2 = 0, cand3 = 0, pixels = 0, rays = 0, violations = 0;
};

static void check_shadowed_frame(const Frame& F, ShMutant mut, int tag, bool rays, ShTally& T) {
    const o_scene sc = F.scene();
    const int ns = static_cast<int>(F.sph.size());
    const size_t nl = F.lt.size();
    const uint32_t waves = 2;  // two waves side by side per workgroup
    const uint32_t gx = (F.cam.width + 15) / 16, gy = (F.rp.rows + 7) / 8;
    const uint32_t wgs = gx * gy, tiles = wgs * waves;
    auto origin = [&](uint32_t t, uint32_t& x0, uint32_t& yl0) {
        const uint32_t wg = t / waves, w = t % waves;
        x0 = 8 * (2 * (wg % gx) + w);
        yl0 = 8 * (wg / gx);
    };
    auto bad = [&](const char* what, uint32_t a) {
        if (T.violations++ < 10)
            std::fprintf(stderr, "case %d: %ux%u rows %u: %s %u\n", tag, F.cam.width, F.cam.height,
                         F.rp.rows, what, a);
    };
    std::vector<TileWord> tw(tiles);
    std::vector<unsigned long long> words(tiles);
    for (uint32_t t = 0; t < tiles; ++t) {
        uint32_t x0, yl0;
        origin(t, x0, yl0);
        tw[t] = table_word(F, x0, yl0, mut);
        words[t] = tw[t].word;
    }
    // the table's layout: the uniform entries from the front of the T words, the shadowed
    // entries from their end
    std::vector<unsigned long long> uni(tiles);
    std::vector<uint32_t> gen(wgs);
    uint32_t n_uni = 0, n_sh = 0, n_gen = 0;
    for (uint32_t pos0 = 0; pos0 < tiles; pos0 += 64) {
        if (mut == kShMixed)
            tile_list_run<0, false, true>(words.data(), tiles, waves, pos0, origin, uni.data(),
                                          &n_uni, gen.data(), &n_gen, &n_sh);
        else
            tile_list_run(words.data(), tiles, waves, pos0, origin, uni.data(), &n_uni,
                          gen.data(), &n_gen, &n_sh);
    }
    uint32_t want_uni = 0, want_sh = 0;
    for (uint32_t t = 0; t < tiles; ++t) {
        want_uni += tile_list_uniform(words[t]);
        want_sh += tile_list_shadowed(words[t]);
        if (tile_list_uniform(words[t]) && tile_list_shadowed(words[t])) bad("two kinds", t);
    }
    if (n_uni != want_uni) bad("uniform count", n_uni);
    if (n_sh != want_sh) bad("shadowed count", n_sh);
    if (static_cast<uint64_t>(n_uni) + n_sh > tiles || n_gen > wgs) {
        bad("count past the list", n_uni + n_sh);
        return;
    }
    std::vector<int> covered(tiles, 0), listed(wgs, 0);
    auto decode = [&](unsigned long long e, uint32_t& t) {
        const uint32_t col = static_cast<uint32_t>(e >> kListColShift) & kListCoordMask;
        const uint32_t row = static_cast<uint32_t>(e >> kListRowShift) & kListCoordMask;
        if (col >= 2 * gx || row >= gy) {
            bad("entry outside the grid, column", col);
            return false;
        }
        t = (row * gx + col / 2) * waves + col % 2;
        return true;
    };
    for (uint32_t i = 0; i < n_uni; ++i) {
        uint32_t t;
        if (!decode(uni[i], t)) continue;
        if (!tile_list_uniform(words[t])) bad("other tile in the uniform list", t);
        if ((uni[i] & kListWordMask) != (words[t] & kListWordMask))
            bad("uniform entry with another word", t);
        ++covered[t];
    }
    Shadow S;
    for (uint32_t i = 0; i < n_sh; ++i) {
        const unsigned long long e = uni[TileTabLayout::shadowed_slot(i, tiles)];
        uint32_t t;
        if (!decode(e, t)) continue;
        ++covered[t];
        if (!tile_list_shadowed(words[t])) {
            bad("other tile in the shadowed list", t);
            continue;
        }
        const TileWord& W = tw[t];
        // the entry's class byte is the plane's class, its keep masks the table's
        const unsigned long long c = tile_class_of(e);
        const int k = static_cast<int>(c) - static_cast<int>(kTilePlane0);
        if (c < kTilePlane0 || k >= static_cast<int>(F.pl.size())) {
            bad("shadowed entry without a plane", t);
            continue;
        }
        if (mut != kShNoWord && k != W.plane) bad("shadowed entry names another plane", t);
        for (size_t l = 0; l < nl; ++l)
            if (tile_plane_keep(e, static_cast<int>(l)) != (W.keep[l] & kPlaneKeepAll))
                bad("shadowed entry with other keep masks", t);
        int cand = 0;
        for (size_t l = 0; l < nl; ++l)
            if (W.sw[l] != kShadowNoWord) cand += __builtin_popcountll(W.sw[l]);
        T.cand1 += cand == 1;
        T.cand2 += cand == 2;
        T.cand3 += cand >= 3;
        if (!rays) continue;
        uint32_t x0, yl0;
        origin(t, x0, yl0);
        for (uint32_t l = 0; l < 64; ++l) {
            uint32_t x, y;
            bool valid;
            lane_pixel(F, x0, yl0, l % 8, l / 8, x, y, valid);
            double ray[6], out[7];
            int32_t index = -1;
            oracle_get_ray(&F.cam, x, y, 0, 0, 0, ray);
            const int type = oracle_closest(&sc, ray, out, &index);
            ++T.pixels;
            if (!(type == 2 && index == k)) {
                if (T.violations++ < 10)
                    std::fprintf(stderr,
                                 "case %d: %ux%u tile (%u,%u) shadowed plane %d pixel (%u,%u): "
                                 "oracle type %d index %d\n",
                                 tag, F.cam.width, F.cam.height, x0, yl0, k, x, y, type, index);
                continue;
            }
            pixel_shadow(F, sc, x, y, S);
            for (size_t m = 0; m < nl; ++m) {
                if (!S.cast[m]) continue;
                ++T.rays;
                for (int i2 = 0; i2 < ns; ++i2) {
                    if (!shadow_ray_meets(S.so, S.L[m], S.max_dist[m], F.sph[i2])) continue;
                    if ((W.sw[m] >> i2) & 1ull) continue;
                    if (T.violations++ < 10)
                        std::fprintf(stderr,
                                     "case %d: tile (%u,%u) pixel (%u,%u) light %zu: sphere %d "
                                     "is not in the word\n",
                                     tag, x0, yl0, x, y, m, i2);
                }
            }
        }
    }
    auto general = [&](uint32_t t) {
        return !tile_list_uniform(words[t]) && !tile_list_shadowed(words[t]);
    };
    for (uint32_t i = 0; i < n_gen; ++i) {
        if (gen[i] >= wgs) {
            bad("workgroup outside the grid", gen[i]);
            continue;
        }
        ++listed[gen[i]];
        for (uint32_t w = 0; w < waves; ++w)
            if (general(gen[i] * waves + w)) ++covered[gen[i] * waves + w];
    }
    for (uint32_t t = 0; t < tiles; ++t)
        if (covered[t] != 1) bad(covered[t] ? "tile rendered twice" : "tile not rendered", t);
    for (uint32_t g = 0; g < wgs; ++g) {
        int gen_w = 0, sh_w = 0, nonuni = 0;
        for (uint32_t w = 0; w < waves; ++w) {
            gen_w += general(g * waves + w);
            sh_w += tile_list_shadowed(words[g * waves + w]);
            nonuni += !tile_list_uniform(words[g * waves + w]);
        }
        if (listed[g] != (gen_w ? 1 : 0)) bad("workgroup listed wrongly", g);
        T.mixed += gen_w > 0 && sh_w > 0;
        T.general_wgs += nonuni > 0;
    }
    T.tiles += tiles;
    T.workgroups += wgs;
    T.uniform += n_uni;
    T.shadowed += n_sh;
    T.listed += n_gen;
}

static void print_shadowed(const char* what, int cases, const ShTally& T) {
    std::printf("%s cases %d tiles %" PRIu64 " workgroups %" PRIu64 " uniform %" PRIu64
                " shadowed %" PRIu64 " listed %" PRIu64 " general_wgs %" PRIu64 " mixed %" PRIu64
                " cand1 %" PRIu64 " cand2 %" PRIu64 " cand3 %" PRIu64 " pixels %" PRIu64
                " rays %" PRIu64 " violations %" PRIu64 "\n",
                what, cases, T.tiles, T.workgroups, T.uniform, T.shadowed, T.listed, T.general_wgs,
                T.mixed, T.cand1, T.cand2, T.cand3, T.pixels, T.rays, T.violations);
}

static int run_shadowed_prop(uint64_t seed, int cases, ShMutant mut) {
    Rng R{seed};
    ShTally T;
    for (int c = 0; c < cases; ++c) {
        const Frame F = random_frame(R);
        check_shadowed_frame(F, mut, c, true, T);
    }
    print_shadowed("prop", cases, T);
    if (mut != kShNone) return 0;
    return T.violations ? 1 : 0;
}

static int run_shadowed_frame(const char* path, bool census) {
    Frame F{};
    if (const int r = read_frame(path, F)) return r;
    ShTally T;
    check_shadowed_frame(F, kShNone, 0, !census, T);
    if (!census) {
        print_shadowed("frame", 1, T);
        return T.violations ? 1 : 0;
    }
    std::printf("tiles                                             %" PRIu64 "\n", T.tiles);
    std::printf("uniform (sky or one plane, every shadow word 0)   %" PRIu64 "\n", T.uniform);
    std::printf("shadowed (one leading plane, some word != 0)      %" PRIu64 "\n", T.shadowed);
    std::printf("  with 1 / 2 / 3+ sphere candidates over all lights  %" PRIu64 " / %" PRIu64
                " / %" PRIu64 "\n", T.cand1, T.cand2, T.cand3);
    std::printf("everything else                                   %" PRIu64 "\n",
                T.tiles - T.uniform - T.shadowed);
    std::printf("workgroups                                        %" PRIu64 "\n", T.workgroups);
    std::printf("general workgroups without the shadowed list      %" PRIu64 "\n", T.general_wgs);
    std::printf("general workgroups with it (listed)               %" PRIu64 "\n", T.listed);
    std::printf("  of which with a shadowed wave too               %" PRIu64 "\n", T.mixed);
    return T.violations ? 1 : 0;
}

int main(int argc, char** argv) {
    if ((argc == 4 || argc == 5) && !std::strcmp(argv[1], "prop")) {
        ShMutant mut = kShNone;
        if (argc == 5) {
            if (!std::strcmp(argv[4], "noword")) mut = kShNoWord;
            else if (!std::strcmp(argv[4], "index")) mut = kShIndex;
            else if (!std::strcmp(argv[4], "mixed")) mut = kShMixed;
            else if (std::strcmp(argv[4], "none")) return 64;
        }
        return run_shadowed_prop(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]), mut);
    }
    if (argc == 3 && !std::strcmp(argv[1], "frame")) return run_shadowed_frame(argv[2], false);
    if (argc == 3 && !std::strcmp(argv[1], "census")) return run_shadowed_frame(argv[2], true);
    std::fprintf(stderr, "usage: shadowed_main prop SEED CASES [none|noword|index|mixed] | "
                         "shadowed_main frame FILE | shadowed_main census FILE\n");
    return 64;
}
