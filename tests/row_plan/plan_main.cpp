// plan_main — the row plan of multi-GPU frames (csrc/rt_row_plan.hpp) on its own, for
// tests/test_row_plan_host.py.  Includes that header only.
//
//   plan_main [MUTANT]
//       For every case (n ranks, row_block, image height H, root weight w) plans every rank and
//       prints
//         case N BLOCK H W
//         rank R rows ROWS max_rows M block B slots V
//         slot S rows ROWS recv OFFSET BYTES ranges A:B A:B ...     (one line per slot of R)
//       recv: where the slot of a batch of kFrames frames of kWidth pixels and kBpp bytes per
//       pixel sits in rank 0's receive buffer, and its bytes.  It checks, per case:
//         cover      every image row belongs to exactly one slot of one rank;
//         maxrows    every rank reports the same max_rows, the maximum of the slots' rows, and a
//                    rank's rows are the sum of its slots';
//         overlap    no slot's extent in the receive layout overlaps another's, and every one
//                    ends within the buffer (Plan::recv_bytes).
//       MUTANT: none (default), slot (rank r >= 1 placed one slot too far).
//       Last line: "cases C violations V cover X maxrows Y overlap Z".
// Exit status 0 only when every property holds (mutants: always 0, the caller reads the counts).
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "rt_row_plan.hpp"

using rtamd::Plan;
using rtamd::RowBlocks;

namespace {

constexpr uint32_t kWidth = 7;
constexpr int kFrames = 3;
constexpr size_t kBpp = 24;

bool g_mutant = false;
long g_cases = 0, g_cover = 0, g_maxrows = 0, g_overlap = 0;

void run_case(int n, uint32_t block, uint32_t H, int weight) {
    rt_render_opts base;
    std::memset(&base, 0, sizeof base);
    base.row_block = static_cast<uint16_t>(block);
    std::printf("case %d %u %u %d\n", n, block, H, weight);
    std::vector<int> owners(H, 0);
    std::vector<std::pair<size_t, size_t>> extents;
    bool maxrows = true, overlap = false;
    uint32_t max_rows = 0, seen_max = 0;
    size_t recv_bytes = 0;
    for (int r = 0; r < n; ++r) {
        Plan pl;
        const bool ok = g_mutant ? rtamd::make_plan<true>(H, base, n, r, weight, pl)
                                 : rtamd::make_plan(H, base, n, r, weight, pl);
        if (!ok) {
            std::printf("rank %d refused\n", r);
            maxrows = false;
            continue;
        }
        std::printf("rank %d rows %u max_rows %u block %u slots %d\n", r, pl.rows, pl.max_rows,
                    pl.block, pl.slots);
        if (r == 0) max_rows = pl.max_rows;
        if (r == 0) recv_bytes = pl.recv_bytes(kWidth, kFrames, kBpp);
        if (pl.max_rows != max_rows) maxrows = false;
        uint32_t sum = 0;
        for (int j = 0; j < pl.nslots; ++j) {
            const int s = pl.first_slot + j;
            const size_t at = pl.recv_offset(s, kWidth, kFrames, kBpp);
            const size_t bytes = pl.send_bytes(kWidth, kFrames, kBpp);
            std::printf("slot %d rows %u recv %zu %zu ranges", s, pl.slot_rows[j], at, bytes);
            const rt_render_opts o = pl.slot(j);
            uint32_t rows = 0;
            for (RowBlocks b(o, H); !b.done(); b.next()) {
                std::printf(" %llu:%llu", static_cast<unsigned long long>(b.y),
                            static_cast<unsigned long long>(b.y + b.rows()));
                for (uint64_t y = b.y; y < b.y + b.rows(); ++y) ++owners[y];
                if (b.packed != rows) maxrows = false;  // packed rows follow one another
                rows += b.rows();
            }
            std::printf("\n");
            if (rows != pl.slot_rows[j] || rows != rtamd::rendered_rows(o, H)) maxrows = false;
            sum += rows;
            if (rows > seen_max) seen_max = rows;
            if (at + bytes > recv_bytes) overlap = true;
            for (const auto& e : extents)
                if (at < e.first + e.second && e.first < at + bytes) overlap = true;
            extents.emplace_back(at, bytes);
        }
        if (sum != pl.rows) maxrows = false;
    }
    if (seen_max != max_rows) maxrows = false;
    bool cover = true;
    for (int c : owners) cover = cover && c == 1;
    ++g_cases;
    g_cover += !cover;
    g_maxrows += !maxrows;
    g_overlap += overlap;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "slot")) g_mutant = true;
    else if (argc > 1 && std::strcmp(argv[1], "none")) return 2;
    // the (n, block, H) of tests/test_gpu_rccl.py test_assemble_rows_matches_row_planner: among
    // them ranks whose first block starts past H, (8, 16, 100) and (16, 16, 64)
    const uint32_t kAssemble[8][3] = {{2, 16, 1080}, {8, 16, 4320}, {8, 16, 100}, {3, 7, 136},
                                      {4, 16, 37},   {8, 54, 4320}, {5, 1, 23},   {16, 16, 64}};
    for (const auto& c : kAssemble) run_case(static_cast<int>(c[0]), c[1], c[2], 1);
    run_case(1, 16, 37, 1);   // one rank: the whole frame, whatever the block ...
    run_case(1, 0, 1080, 1);
    run_case(1, 8, 100, 3);   // ... and the weight
    run_case(3, 0, 136, 1);   // no row_block: the default block
    for (int n : {2, 3, 8})
        for (int w : {1, 2, 3, 16}) {
            run_case(n, 8, 100, w);
            run_case(n, 16, 1080, w);
        }
    const long violations = g_cover + g_maxrows + g_overlap;
    std::printf("cases %ld violations %ld cover %ld maxrows %ld overlap %ld\n", g_cases,
                violations, g_cover, g_maxrows, g_overlap);
    return g_mutant || violations == 0 ? 0 : 1;
}
