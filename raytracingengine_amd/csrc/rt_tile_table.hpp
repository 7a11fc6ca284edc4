// rt_tile_table.hpp — the per-camera tile table of the packet path's table-reading variants (C2's
// two): what one holds (TileTabContents), where each section lies (TileTabLayout) and how the
// lists' counts travel to the host (TileListCounts).  Every reader and writer of a table — the
// kernel that forms it and the launchers (rt_packet.hip), the kernels that render from it
// (rt_packet_kernel.hpp, packet_uniform_kernel), the cache and the ring (rt_packet_host.cpp) and
// the host tests — takes its offsets from here.
//
// The table.  One buffer of 64-bit words per camera, ray constants and launch shape, formed by one
// launch of packet_cone_table_kernel (one lane per wave tile) and never rewritten.  For T tiles in
// W workgroups of T / W waves, tile t = (tby · gx + tbx) · waves + wave, and nl shadow words per
// tile:
//   T words       cone: the tile's camera-cone candidate mask (rt_cone_table.hpp)
//   T · nl words  shadow: per tile and light, the shadow-cull candidate mask formed from the cone
//                 mask (rt_shadow_table.hpp); they depend on the render call's bias
//   T words       class: the tile's class (tile_class_word) in bits 0-7, light l's shadow-plane
//                 keep mask (shadow_plane_keep; all ones when not formed) in bits 8 + 8·l and up,
//                 the shadowed-plane mark (tile_shadowed_mark) above them when it is formed
//   1 word        list counts: uniform tiles in the low half, listed workgroups in the high half
//   T words       the uniform tiles' entries from the front (tile_list_entry) and the
//                 shadowed-plane tiles' from the end downwards (tile_shadowed_entry): a tile is in
//                 one list at most, so the two never meet
//   (W+1)/2 words the listed (general) workgroups, one 32-bit index tby · gx + tbx each
//   1 word        the count of shadowed-plane tiles
// A table ends after any section its contents leave out: cone words alone, cone and shadow words,
// those and class words, or everything.  Each later section is formed from the earlier ones by the
// same lane, which is what TileTabContents::valid() says; a table formed with other contents is
// another table (key_word() is part of its cache key).  The kernels that render hold a pointer to
// a section (TraceParams.cone_tab / shadow_tab / class_tab and the per-frame fr_*), null where the
// launch is not to read it; the lists are reached through the class pointer (Lists).
//
// Plain C++, like rt_cone_table.hpp: host test programs call it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_cone_table.hpp"

namespace rtamd {

// Point lights a table holds shadow words for, at most (the class word has a keep mask for each).
constexpr int kShadowTabLights = 4;

struct TileTabContents {
    int32_t shadow_nl;    // shadow words per tile, 0 .. kShadowTabLights
    int32_t class_words;  // 0: none, 1: with all-ones keep masks, 2: with the keep masks formed
    int32_t lists;        // 0: none, 1: uniform and general, 2: with the shadowed mark and list
    RT_CT_HD bool valid() const {
        if (shadow_nl < 0 || shadow_nl > kShadowTabLights) return false;
        if (class_words < 0 || class_words > 2 || lists < 0 || lists > 2) return false;
        // class words are formed from the shadow words, lists from the class words
        return (class_words == 0 || shadow_nl > 0) && (lists == 0 || class_words != 0);
    }
    RT_CT_HD bool has_shadow() const { return shadow_nl > 0; }
    RT_CT_HD bool has_class() const { return class_words != 0; }
    RT_CT_HD bool forms_keep() const { return class_words == 2; }
    RT_CT_HD bool has_lists() const { return lists != 0; }
    RT_CT_HD bool forms_mark() const { return lists == 2; }
    // one word that tells any two valid contents apart
    RT_CT_HD uint32_t key_word() const {
        return static_cast<uint32_t>(shadow_nl) | static_cast<uint32_t>(class_words) << 8 |
               static_cast<uint32_t>(lists) << 16;
    }
};

// Word offsets from the table's base.
struct TileTabLayout {
    size_t tiles, wgs;
    TileTabContents c;
    // The lists by themselves: word offsets from the counts word, which lies after_cls() words
    // after the class word of tile 0.  The kernels that read the lists hold the frame's class
    // pointer and the tile count, and nothing here depends on the sections before.
    struct Lists {
        uint32_t tiles, wgs;
        RT_CT_HD size_t after_cls() const { return tiles; }
        RT_CT_HD size_t counts() const { return 0; }
        RT_CT_HD size_t uniform(uint32_t i) const { return 1u + i; }
        RT_CT_HD size_t shadowed(uint32_t j) const { return uniform(shadowed_slot(j, tiles)); }
        RT_CT_HD size_t general_base() const { return size_t(1) + tiles; }  // a 32-bit array
        RT_CT_HD size_t shadowed_count() const {
            return 1 + static_cast<size_t>(tiles) + (static_cast<size_t>(wgs) + 1) / 2;
        }
        RT_CT_HD size_t end() const { return shadowed_count() + 1; }
    };
    // shadowed entry j's index in the array of uniform entries
    RT_CT_HD static uint32_t shadowed_slot(uint32_t j, uint32_t tiles) { return tiles - 1u - j; }

    RT_CT_HD size_t cone(size_t t) const { return t; }
    RT_CT_HD size_t shadow(size_t t, int l) const {
        return tiles + t * static_cast<size_t>(c.shadow_nl) + static_cast<size_t>(l);
    }
    RT_CT_HD size_t cls(size_t t) const {
        return tiles * (1 + static_cast<size_t>(c.shadow_nl)) + t;
    }
    RT_CT_HD Lists lists() const {
        return Lists{static_cast<uint32_t>(tiles), static_cast<uint32_t>(wgs)};
    }
    RT_CT_HD size_t list_counts() const { return cls(0) + lists().after_cls(); }
    RT_CT_HD size_t uniform(uint32_t i) const { return list_counts() + lists().uniform(i); }
    RT_CT_HD size_t shadowed(uint32_t j) const { return list_counts() + lists().shadowed(j); }
    RT_CT_HD size_t general_base() const { return list_counts() + lists().general_base(); }
    RT_CT_HD size_t shadowed_count() const { return list_counts() + lists().shadowed_count(); }
    RT_CT_HD size_t words() const {
        if (c.has_lists()) return list_counts() + lists().end();
        return c.has_class() ? cls(tiles) : shadow(tiles, 0);
    }
    RT_CT_HD size_t bytes() const { return sizeof(unsigned long long) * words(); }
    // the words the batch ring's cap counts: cone and class words (the others come on top)
    RT_CT_HD size_t capped_words() const { return tiles * (c.has_class() ? 2 : 1); }
};

// A table's three list counts.  In the table: the counts word (uniform low, general high; the
// table kernel's wavefronts add to its halves) and the shadowed count's word.  For the host: two
// pinned words of the same shape with every count plus one, so that 0 says "not formed yet".
struct TileListCounts {
    uint32_t uniform, general, shadowed;
};
RT_CT_HD inline TileListCounts tile_list_counts(unsigned long long counts_word,
                                                unsigned long long shadowed_word) {
    return TileListCounts{static_cast<uint32_t>(counts_word),
                          static_cast<uint32_t>(counts_word >> 32),
                          static_cast<uint32_t>(shadowed_word)};
}
RT_CT_HD inline void tile_list_counts_encode(const TileListCounts& n, unsigned long long* host) {
    host[0] = ((static_cast<unsigned long long>(n.general) + 1ull) << 32) |
              (static_cast<unsigned long long>(n.uniform) + 1ull);
    host[1] = static_cast<unsigned long long>(n.shadowed) + 1ull;
}
// false: not yet (a word still 0: the launch that forms the table has not stored it)
RT_CT_HD inline bool tile_list_counts_decode(const unsigned long long* host, TileListCounts* n) {
    const TileListCounts v = tile_list_counts(host[0], host[1]);
    if (!v.uniform || !v.general || !v.shadowed) return false;
    *n = TileListCounts{v.uniform - 1u, v.general - 1u, v.shadowed - 1u};
    return true;
}

}  // namespace rtamd
