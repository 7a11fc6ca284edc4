// table_main.cpp — stand-alone host check of the tile table's description
// (csrc/rt_tile_table.hpp), built and run by tests/test_tile_table_host.py.  The offsets below are
// written out as literals from the documented layout — T cone words, T·nl shadow words, T class
// words, 1 counts word, T uniform / shadowed words, (W+1)/2 general words, 1 shadowed-count word —
// and not recomputed.
//
//   table_main
//       prints `checks N failed M`; exit status 0 only when M is 0.
#include <cstdint>
#include <cstdio>
#include <set>

#include "rt_tile_table.hpp"

using namespace rtamd;

static int g_checks = 0, g_failed = 0;
static void expect(const char* what, unsigned long long got, unsigned long long want) {
    ++g_checks;
    if (got == want) return;
    ++g_failed;
    std::fprintf(stderr, "%s: %llu, expected %llu\n", what, got, want);
}

int main() {
    {  // T = 8 tiles in W = 4 workgroups, two lights, three lists
        const TileTabLayout L{8, 4, TileTabContents{2, 2, 2}};
        expect("8/4/2 valid", L.c.valid(), 1);
        expect("8/4/2 cone(0)", L.cone(0), 0);
        expect("8/4/2 cone(7)", L.cone(7), 7);
        expect("8/4/2 shadow(0,0)", L.shadow(0, 0), 8);
        expect("8/4/2 shadow(0,1)", L.shadow(0, 1), 9);
        expect("8/4/2 shadow(7,1)", L.shadow(7, 1), 23);
        expect("8/4/2 cls(0)", L.cls(0), 24);
        expect("8/4/2 cls(7)", L.cls(7), 31);
        expect("8/4/2 list_counts", L.list_counts(), 32);
        expect("8/4/2 uniform(0)", L.uniform(0), 33);
        expect("8/4/2 uniform(7)", L.uniform(7), 40);
        expect("8/4/2 shadowed(0)", L.shadowed(0), 40);
        expect("8/4/2 shadowed(7)", L.shadowed(7), 33);
        expect("8/4/2 general_base", L.general_base(), 41);
        expect("8/4/2 shadowed_count", L.shadowed_count(), 43);
        expect("8/4/2 words", L.words(), 44);
        expect("8/4/2 bytes", L.bytes(), 352);
        // the same lists as a kernel reaches them from the class words
        const TileTabLayout::Lists K = L.lists();
        expect("8/4/2 after_cls", L.cls(0) + K.after_cls(), 32);
        expect("8/4/2 from cls: general", L.cls(0) + K.after_cls() + K.general_base(), 41);
        expect("8/4/2 from cls: shadowed(0)", L.cls(0) + K.after_cls() + K.shadowed(0), 40);
        expect("8/4/2 from cls: count", L.cls(0) + K.after_cls() + K.shadowed_count(), 43);
    }
    {  // T = 6 tiles in W = 3 workgroups (an odd count: the general words round up), one light
        const TileTabLayout L{6, 3, TileTabContents{1, 2, 2}};
        expect("6/3/1 cls(0)", L.cls(0), 12);
        expect("6/3/1 list_counts", L.list_counts(), 18);
        expect("6/3/1 uniform(0)", L.uniform(0), 19);
        expect("6/3/1 general_base", L.general_base(), 25);
        expect("6/3/1 shadowed_count", L.shadowed_count(), 27);
        expect("6/3/1 words", L.words(), 28);
    }
    {  // tables that end early
        expect("cone only", (TileTabLayout{8, 4, TileTabContents{0, 0, 0}}).words(), 8);
        expect("no class", (TileTabLayout{8, 4, TileTabContents{2, 0, 0}}).words(), 24);
        expect("no lists", (TileTabLayout{8, 4, TileTabContents{2, 1, 0}}).words(), 32);
        expect("no lists, nl 3", (TileTabLayout{6, 3, TileTabContents{3, 2, 0}}).words(), 30);
        expect("two lists", (TileTabLayout{8, 4, TileTabContents{2, 2, 1}}).words(), 44);
    }
    // the closure rules, and a key word per valid contents
    expect("lists without class words", (TileTabContents{2, 0, 1}).valid(), 0);
    expect("class words without shadow words", (TileTabContents{0, 1, 0}).valid(), 0);
    expect("lists without anything", (TileTabContents{0, 0, 2}).valid(), 0);
    expect("too many lights", (TileTabContents{kShadowTabLights + 1, 0, 0}).valid(), 0);
    expect("a fourth list", (TileTabContents{1, 1, 3}).valid(), 0);
    std::set<uint32_t> keys;
    unsigned n_valid = 0;
    for (int nl = -1; nl <= kShadowTabLights + 1; ++nl)
        for (int cls = -1; cls <= 3; ++cls)
            for (int lists = -1; lists <= 3; ++lists) {
                const TileTabContents c{nl, cls, lists};
                if (!c.valid()) continue;
                ++n_valid;
                keys.insert(c.key_word());
            }
    // nl = 0 alone, and for nl = 1..4: no class words, or 2 kinds × (no, two, three lists)
    expect("valid contents", n_valid, 1 + 4 * (1 + 2 * 3));
    expect("distinct key words", keys.size(), n_valid);
    // the counts: table words → host words → counts, and "not yet"
    {
        const TileListCounts n = tile_list_counts(0x0000002a00000007ull, 0x5ull);
        expect("uniform", n.uniform, 7);
        expect("general", n.general, 42);
        expect("shadowed", n.shadowed, 5);
        unsigned long long host[2] = {0, 0};
        TileListCounts back{99, 99, 99};
        expect("not yet", tile_list_counts_decode(host, &back), 0);
        tile_list_counts_encode(n, host);
        expect("host word 0", host[0], 0x0000002b00000008ull);
        expect("host word 1", host[1], 6);
        expect("decoded", tile_list_counts_decode(host, &back), 1);
        expect("uniform back", back.uniform, 7);
        expect("general back", back.general, 42);
        expect("shadowed back", back.shadowed, 5);
        const unsigned long long half[2] = {host[0], 0};  // the second store not seen yet
        expect("half stored", tile_list_counts_decode(half, &back), 0);
        // empty lists are counts of 0, not "not yet"
        tile_list_counts_encode(TileListCounts{0, 0, 0}, host);
        expect("zero counts decode", tile_list_counts_decode(host, &back), 1);
        expect("zero uniform", back.uniform, 0);
    }
    std::printf("checks %d failed %d\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
