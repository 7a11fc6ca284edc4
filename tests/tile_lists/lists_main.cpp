// lists_main.cpp — stand-alone host check of the tile lists (tile_list_run and its helpers,
// csrc/rt_shadow_table.hpp: the function the table kernel's wavefronts follow), built and run by
// tests/test_tile_lists_host.py.  The random frames, the frame file and the class words are
// tests/host_frame.hpp's.
//
//   lists_main prop SEED CASES [MUTANT]
//       For every frame: the class word of every tile, then the two lists, run by run.  Every
//       tile must be in exactly one of the uniform list (an entry that decodes to the tile and
//       carries its class word) and a listed workgroup's general waves; the uniform count must
//       be the number of class words that are not general; no tile and no workgroup may be
//       listed twice; a workgroup must be listed if and only if it has a general wave.
//       MUTANT: none (default), index (an entry's column off by one), mixed (a workgroup with a
//       uniform wave is not listed).
//   lists_main frame FILE
//       the same on one frame of a real scene (shadow_main's file format).
// Exit status 0 only when every property holds (mutants: always 0, the caller reads
// `violations`).
#include "../host_frame.hpp"

enum ListMutant { kLstNone, kLstIndex, kLstMixed };

struct ListTally {
    uint64_t tiles = 0, workgroups = 0, uniform = 0, listed = 0, mixed = 0, violations = 0;
};

static void check_lists_frame(const Frame& F, ListMutant mut, int tag, ListTally& T) {
    const uint32_t waves = 2;  // two waves side by side per workgroup
    const uint32_t gx = (F.cam.width + 15) / 16, gy = (F.rp.rows + 7) / 8;
    const uint32_t wgs = gx * gy, tiles = wgs * waves;
    auto origin = [&](uint32_t t, uint32_t& x0, uint32_t& yl0) {
        const uint32_t wg = t / waves, w = t % waves;
        x0 = 8 * (2 * (wg % gx) + w);
        yl0 = 8 * (wg / gx);
    };
    std::vector<unsigned long long> words(tiles);
    for (uint32_t t = 0; t < tiles; ++t) {
        uint32_t x0, yl0;
        origin(t, x0, yl0);
        bool zero = false;
        unsigned long long geo = kTileGeneral;
        words[t] = class_word(F, x0, yl0, kClsNone, &zero, &geo);
    }
    // (the table's layout: room for every tile and every workgroup)
    std::vector<unsigned long long> uni(tiles);
    std::vector<uint32_t> gen(wgs);
    uint32_t n_uni = 0, n_gen = 0;
    for (uint32_t pos0 = 0; pos0 < tiles; pos0 += 64) {  // (two lists: no shadowed count)
        if (mut == kLstIndex)
            tile_list_run<1, false>(words.data(), tiles, waves, pos0, origin, uni.data(), &n_uni,
                                    gen.data(), &n_gen);
        else if (mut == kLstMixed)
            tile_list_run<0, true>(words.data(), tiles, waves, pos0, origin, uni.data(), &n_uni,
                                   gen.data(), &n_gen);
        else
            tile_list_run(words.data(), tiles, waves, pos0, origin, uni.data(), &n_uni, gen.data(),
                          &n_gen);
    }
    auto bad = [&](const char* what, uint32_t a) {
        if (T.violations++ < 10)
            std::fprintf(stderr, "case %d: %ux%u rows %u: %s %u\n", tag, F.cam.width, F.cam.height,
                         F.rp.rows, what, a);
    };
    std::vector<int> covered(tiles, 0), listed(wgs, 0);
    uint32_t want_uni = 0;
    for (uint32_t t = 0; t < tiles; ++t) want_uni += tile_list_uniform(words[t]);
    if (n_uni != want_uni) bad("uniform count", n_uni);
    if (n_uni > tiles || n_gen > wgs) {
        bad("count past the list", n_uni);
        return;
    }
    for (uint32_t i = 0; i < n_uni; ++i) {
        const unsigned long long e = uni[i];
        const uint32_t col = static_cast<uint32_t>(e >> kListColShift) & kListCoordMask;
        const uint32_t row = static_cast<uint32_t>(e >> kListRowShift) & kListCoordMask;
        if (col >= 2 * gx || row >= gy) {
            bad("entry outside the grid, column", col);
            continue;
        }
        const uint32_t t = (row * gx + col / 2) * waves + col % 2;
        if (!tile_list_uniform(words[t])) bad("general tile in the uniform list", t);
        if ((e & kListWordMask) != (words[t] & kListWordMask)) bad("entry with another word", t);
        ++covered[t];
    }
    for (uint32_t i = 0; i < n_gen; ++i) {
        if (gen[i] >= wgs) {
            bad("workgroup outside the grid", gen[i]);
            continue;
        }
        ++listed[gen[i]];
        for (uint32_t w = 0; w < waves; ++w)
            if (!tile_list_uniform(words[gen[i] * waves + w])) ++covered[gen[i] * waves + w];
    }
    for (uint32_t t = 0; t < tiles; ++t)
        if (covered[t] != 1) bad(covered[t] ? "tile rendered twice" : "tile not rendered", t);
    for (uint32_t g = 0; g < wgs; ++g) {
        int general = 0;
        for (uint32_t w = 0; w < waves; ++w) general += !tile_list_uniform(words[g * waves + w]);
        if (listed[g] != (general ? 1 : 0)) bad("workgroup listed wrongly", g);
        T.mixed += general > 0 && general < static_cast<int>(waves);
    }
    T.tiles += tiles;
    T.workgroups += wgs;
    T.uniform += n_uni;
    T.listed += n_gen;
}

static void print_lists(const char* what, int cases, const ListTally& T) {
    std::printf("%s cases %d tiles %" PRIu64 " workgroups %" PRIu64 " uniform %" PRIu64
                " listed %" PRIu64 " mixed %" PRIu64 " violations %" PRIu64 "\n",
                what, cases, T.tiles, T.workgroups, T.uniform, T.listed, T.mixed, T.violations);
}

static int run_lists_prop(uint64_t seed, int cases, ListMutant mut) {
    Rng R{seed};
    ListTally T;
    for (int c = 0; c < cases; ++c) {
        const Frame F = random_frame(R);
        check_lists_frame(F, mut, c, T);
    }
    print_lists("prop", cases, T);
    if (mut != kLstNone) return 0;
    return T.violations ? 1 : 0;
}

static int run_lists_frame(const char* path) {
    Frame F{};
    if (const int r = read_frame(path, F)) return r;
    ListTally T;
    check_lists_frame(F, kLstNone, 0, T);
    print_lists("frame", 1, T);
    return T.violations ? 1 : 0;
}

int main(int argc, char** argv) {
    if ((argc == 4 || argc == 5) && !std::strcmp(argv[1], "prop")) {
        ListMutant mut = kLstNone;
        if (argc == 5) {
            if (!std::strcmp(argv[4], "index")) mut = kLstIndex;
            else if (!std::strcmp(argv[4], "mixed")) mut = kLstMixed;
            else if (std::strcmp(argv[4], "none")) return 64;
        }
        return run_lists_prop(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]), mut);
    }
    if (argc == 3 && !std::strcmp(argv[1], "frame")) return run_lists_frame(argv[2]);
    std::fprintf(stderr, "usage: lists_main prop SEED CASES [none|index|mixed] | lists_main frame FILE\n");
    return 64;
}
