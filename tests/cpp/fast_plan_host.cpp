// Stand-alone host program over openmavis_amd/csrc/fast_plan.h (no HIP, no device).  Each input line is a pyramid,
// "w0 h0 w1 h1 ...": the program plans its FAST cells and the prefilter's slot table as omv_orb_create does and prints
//   geom <cells> <fast_rs> <table entries>
//   cell <the 16 ints of struct Cell>                   one per cell
//   slots <n> lo hi lo hi ...                           the cell's run of the table: its rounds and the spare one
// and after the last pyramid "bop" with describe's 4 x 64 Toeplitz operands in hex.  Built with
// -fsanitize=address,undefined by tests/test_fast_plan_cpu.py, which compares the lines with its own restatement.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../openmavis_amd/csrc/fast_plan.h"

int main() {
    using namespace omv_fast_plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::vector<Cell> cells;
        int w, h, max_rw = 0;
        for (int l = 0; in >> w >> h; ++l) fast_level_cells(l, w, h, cells);
        for (const Cell &c : cells) max_rw = std::max(max_rw, c.x1 - c.x0);
        const int fast_rs = fast_row_stride(max_rw);
        std::vector<FastSlot> table;
        plan_fast_slots(cells, fast_rs, table);
        std::printf("geom %zu %d %zu\n", cells.size(), fast_rs, table.size());
        for (const Cell &c : cells) {
            std::printf("cell %d %d %d %d %d %d %d %d %u %d %u %d %d %d %d %d\n", c.level, c.y0, c.y1, c.x0, c.x1, c.o, c.nd,
                        c.rpi, c.mnd, c.ndet, c.mdw, c.jq0, c.npr, c.np, c.slot_off, c.nband);
            const int n = c.np > 0 ? (c.np + kSlotRound - 1) / kSlotRound * kSlotRound + kSlotRound : 0;
            if ((size_t)c.slot_off + (size_t)std::max(n, kSlotRound) > table.size()) return 2;   // a wave's loads stay inside
            std::printf("slots %d", n);
            for (int i = 0; i < n; ++i) std::printf(" %u %u", table[c.slot_off + i].lo, table[c.slot_off + i].hi);
            std::printf("\n");
        }
    }
    uint64_t bop[4 * 64];
    describe_bop_table(bop);
    std::printf("bop");
    for (uint64_t v : bop) std::printf(" %llx", (unsigned long long)v);
    std::printf("\n");
    return 0;
}
