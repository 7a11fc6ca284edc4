// stage_main — the staging layout rule (csrc/rt_stage.hpp) on its own, for
// tests/test_stage_host.py.  Includes that header only.
//
//   stage_main [MUTANT]
//       Declares the items of every host batch query as its entry does, for n in {0, 1, 63, 64,
//       65, 257}, every output mask of the three output records (7 + 31 + 31) and 0, 1 and 3
//       lights, lays them out and checks, per case:
//         total      the total is the entry's formula (the bytes the entry asked for before the
//                    layout rule was written down);
//         overlap    no two items with bytes overlap, and every one ends within the total;
//         aligned    an item whose size is a multiple of 8 sits at a multiple of 8;
//         extent     an output that was not requested has no bytes: the sizes sum to the total;
//         order      offsets do not decrease in declaration order among the 8-aligned items and
//                    among the byte-aligned ones, and every byte-aligned item lies after them.
//       MUTANT: none (default), short (an item one byte into its predecessor), bytes (the
//       byte-sized items placed before the others).
//       Prints "cases C violations V total T overlap O aligned A extent E order R".
// Exit status 0 only when every property holds (mutants: always 0, the caller reads the counts).
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "rt_stage.hpp"

using rtamd::StageItem;
using rtamd::StagePlan;

namespace {

int g_mutant = 0;  // 0 none, 1 short, 2 bytes
long g_cases = 0, g_total = 0, g_overlap = 0, g_aligned = 0, g_extent = 0, g_order = 0;

// Lays `plan` out and checks it against the entry's formula.
void check(StagePlan& plan, size_t want_total) {
    const size_t total = g_mutant == 1   ? plan.layout<true, false>()
                         : g_mutant == 2 ? plan.layout<false, true>()
                                         : plan.layout();
    ++g_cases;
    if (total != want_total || plan.total != total) ++g_total;
    size_t sum = 0, wide_end = 0, last_wide = 0, last_narrow = 0;
    bool overlap = false, aligned = true, order = true;
    for (int i = 0; i < plan.count; ++i) {
        const StageItem& a = plan.item[i];
        sum += a.bytes;
        if (a.bytes && a.offset + a.bytes > total) overlap = true;
        for (int j = 0; j < i; ++j) {
            const StageItem& b = plan.item[j];
            if (a.bytes && b.bytes && a.offset < b.offset + b.bytes &&
                b.offset < a.offset + a.bytes)
                overlap = true;
        }
        if (a.bytes && a.bytes % 8 == 0 && a.offset % 8 != 0) aligned = false;
        size_t& last = a.align >= 8 ? last_wide : last_narrow;
        if (a.offset < last) order = false;
        last = a.offset;
        if (a.align >= 8 && a.offset + a.bytes > wide_end) wide_end = a.offset + a.bytes;
    }
    for (int i = 0; i < plan.count; ++i)
        if (plan.item[i].align < 8 && plan.item[i].bytes && plan.item[i].offset < wide_end)
            order = false;
    g_overlap += overlap;
    g_aligned += !aligned;
    g_extent += sum != total;
    g_order += !order;
}

// The inputs, then the outputs of `mask` of a record whose outputs take bytes[k] per item: the
// total is in_doubles * n * 8 plus n * bytes[k] over the requested bits.
void record_case(size_t n, std::initializer_list<size_t> inputs, size_t in_doubles,
                 const size_t* bytes, int fields, int mask) {
    static char host[8];
    StagePlan plan;
    for (size_t b : inputs) plan.input(host, b);
    size_t want = in_doubles * n * 8;
    for (int k = 0; k < fields; ++k) {
        const bool on = mask & (1 << k);
        plan.output(host, on ? n * bytes[k] : 0, bytes[k] % 8 ? 1 : 8);
        if (on) want += n * bytes[k];
    }
    check(plan, want);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "short")) g_mutant = 1;
    else if (argc > 1 && !std::strcmp(argv[1], "bytes")) g_mutant = 2;
    else if (argc > 1 && std::strcmp(argv[1], "none")) return 2;
    static char host[8];
    const size_t kDl[3] = {24, 24, 24}, kSc[5] = {24, 48, 48, 16, 1}, kCh[5] = {8, 8, 24, 24, 56};
    for (size_t n : {size_t(0), size_t(1), size_t(63), size_t(64), size_t(65), size_t(257)}) {
        {  // rt_trace_rays: 9n doubles
            StagePlan p;
            p.input(host, n * 48);
            p.output(host, n * 24);
            check(p, 9 * n * 8);
        }
        {  // rt_intersect_rays: 15n doubles
            StagePlan p;
            p.input(host, n * 48);
            p.output(host, n * 72);
            check(p, 15 * n * 8);
        }
        {  // rt_occluded_rays: 7n doubles and n bytes
            StagePlan p;
            p.input(host, n * 48);
            p.input(host, n * 8);
            p.output(host, n, 1);
            check(p, 7 * n * 8 + n);
        }
        {  // rt_transmittance_rays: 8n doubles
            StagePlan p;
            p.input(host, n * 48);
            p.input(host, n * 8);
            p.output(host, n * 8);
            check(p, 8 * n * 8);
        }
        for (size_t nl : {size_t(0), size_t(1), size_t(3)}) {  // rt_light_transmittance
            StagePlan p;
            p.input(host, n * 48);
            p.output(host, n * nl * 8);
            check(p, (6 + nl) * n * 8);
        }
        for (int mask = 1; mask < 8; ++mask) {
            // rt_direct_light with n materials and with one shared material: (16 or 9 + 3k)n
            // doubles, k outputs; rt_direct_light_rays: (6 + 3k)n
            record_case(n, {n * 72, n * 56}, 16, kDl, 3, mask);
            record_case(n, {n * 72, 0}, 9, kDl, 3, mask);
            record_case(n, {n * 48}, 6, kDl, 3, mask);
        }
        for (int mask = 1; mask < 32; ++mask) {
            record_case(n, {n * 48}, 6, kSc, 5, mask);  // rt_scatter_rays
            record_case(n, {n * 48}, 6, kCh, 5, mask);  // rt_closest_rays
        }
        {  // rt_camera_rays: rows * W = n pixels, 6 doubles each
            StagePlan p;
            p.output(host, n * 48);
            check(p, n * 6 * 8);
        }
    }
    const long violations = g_total + g_overlap + g_aligned + g_extent + g_order;
    std::printf("cases %ld violations %ld total %ld overlap %ld aligned %ld extent %ld order %ld\n",
                g_cases, violations, g_total, g_overlap, g_aligned, g_extent, g_order);
    return g_mutant || violations == 0 ? 0 : 1;
}
