// The host plan of the extraction kernels' bookkeeping (orb_extract.hip): the FAST cells of a level with the constants
// K2 reads instead of deriving, the prefilter's slot table, and describe's Toeplitz operands.  Nothing here needs the HIP
// runtime: hipcc compiles this text into the product, the host compiler into tests/cpp/fast_plan_host.cpp
// (tests/test_fast_plan_cpu.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>

namespace omv_fast_plan {

constexpr int kEdge = 19;     // EDGE_THRESHOLD
constexpr int kMinB = kEdge - 3;

struct Cell {
    int level, y0, y1, x0, x1;   // region rows [y0,y1), cols [x0,x1) in level coordinates
    // What K2 derives from the rectangle alone, host-computed (fast_cell_constants) and read with the rectangle by
    // one scalar load; every wave of every image recomputed them, three integer divisions included.  The dword path's
    // values hold for a dword-aligned level base and pitch, where the region's misalignment is o = x0 & 3 (the
    // kernel tests the alignment at run time; its byte path has o = 0 and uses ndet and mdw only).
    int o, nd, rpi;              // dwords of a staged row (x1 - x0 + o + 3) >> 2, rows per 64-lane band 64 / nd
    uint32_t mnd;                // lane / nd = lane * mnd >> 16 (lane < 64)
    int ndet;                    // detection window pixels (x1 - x0 - 6) * (y1 - y0 - 6), 0 when empty
    uint32_t mdw;                // i / dw = i * mdw >> 20
    int jq0, npr, np;            // first LDS dword of the window, dword pairs per row, pairs (prefilter slots) of the window
    int slot_off;                // the cell's first entry in the slot table (plan_fast_slots)
    int nband;                   // whole bands of rpi rows in the region: (y1 - y0) / rpi
};
static_assert(sizeof(Cell) == 64, "Cell: one 64-byte scalar load");

// A FAST cell with the constants K2 reads instead of deriving (struct Cell): the same integer expressions the
// kernel used to evaluate per wave.
inline Cell fast_cell_constants(int level, int y0, int y1, int x0, int x1) {
    Cell c{};
    c.level = level, c.y0 = y0, c.y1 = y1, c.x0 = x0, c.x1 = x1;
    const int rw = x1 - x0, rh = y1 - y0, dw = rw - 6, dh = rh - 6;
    c.o = x0 & 3;
    c.nd = (rw + c.o + 3) >> 2;
    c.rpi = c.nd > 0 ? 64 / c.nd : 0;
    c.nband = c.rpi > 0 ? rh / c.rpi : 0;
    c.mnd = c.nd > 0 ? (1u << 16) / (uint32_t)c.nd + 1u : 0u;   // exact while lane * nd < 2^16
    c.ndet = (dw > 0 && dh > 0) ? dw * dh : 0;
    c.mdw = dw > 0 ? (1u << 20) / (uint32_t)dw + 1u : 0u;
    c.jq0 = (c.o + 3) >> 2;
    const int jq1 = (c.o + rw - 4) >> 2, nqr = jq1 - c.jq0 + 1;
    c.npr = (nqr + 1) >> 1;
    c.np = c.ndet > 0 ? c.npr * dh : 0;
    return c;
}

// The FAST cells of a level of w x h pixels (ComputeKeyPointsOctTree, ORBextractor.cc:718-742), appended row-major.
inline void fast_level_cells(int level, int w, int h, std::vector<Cell> &cells) {
    const int maxBX = w - kEdge + 3, maxBY = h - kEdge + 3;
    const float width = (float)(maxBX - kMinB), height = (float)(maxBY - kMinB);
    const int nCols = (int)(width / 35.f), nRows = (int)(height / 35.f);
    // a level too small for one 35-px cell has no cells: the reference's loops over 0 rows / 0 columns do not
    // run (its cell size, a float division by zero, is then never used) and the level yields no keypoint
    if (nCols < 1 || nRows < 1) return;
    const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
    for (int i = 0; i < nRows; ++i) {
        const float iniY = (float)(kMinB + i * hCell);
        float maxY = iniY + hCell + 6;
        if (iniY >= maxBY - 3) continue;
        if (maxY > maxBY) maxY = (float)maxBY;
        for (int j = 0; j < nCols; ++j) {
            const float iniX = (float)(kMinB + j * wCell);
            float maxX = iniX + wCell + 6;
            if (iniX >= maxBX - 6) continue;
            if (maxX > maxBX) maxX = (float)maxBX;
            cells.push_back(fast_cell_constants(level, (int)iniY, (int)maxY, (int)iniX, (int)maxX));
        }
    }
}

// K2's LDS row stride in bytes: an odd dword count (rows spread over the LDS banks) -- 13 dwords when every cell row
// plus its misalignment fits, else 17, else 0: per cell, 4 nd.
inline int fast_row_stride(int max_rw) { return max_rw + 3 <= 52 ? 52 : max_rw + 3 <= 68 ? 68 : 0; }

// One prefilter slot of the dword path: lane tp of a cell tests the 8 pixels of the LDS dword pair (j, j + 1) of a
// window row.  Everything the slot needs is a function of the cell's shape and tp, so the kernel loads it instead of
// deriving it every round:
//   lo  bits 0..15 the candidate entry of the pair's column 0, (r << 7) + q0; bits 16..23 the mask of its columns
//       inside the detection window [3, rw - 4] (bit k = column q0 + k)
//   hi  the LDS byte offset of dword j - 3 rsw: the pair's upper compass neighbour, the lowest address the slot reads
// with r = 3 + tp / npr, jq = jq0 + 2 (tp % npr), q0 = 4 jq - o, j = r rsw + jq (rsw: dwords of an LDS row).
struct FastSlot {
    uint32_t lo, hi;
};
constexpr int kSlotRound = 64;   // slots of a prefilter round (one per lane)

inline FastSlot fast_slot(const Cell &c, int rsw, int tp) {
    const int rw = c.x1 - c.x0;
    const int r = 3 + tp / c.npr, jq = c.jq0 + 2 * (tp % c.npr);
    const int q0 = 4 * jq - c.o;
    uint32_t mask = 0;
    for (int k = 0; k < 8; ++k)
        if (q0 + k >= 3 && q0 + k <= rw - 4) mask |= 1u << k;
    return FastSlot{(uint32_t)((r << 7) + q0) | (mask << 16), (uint32_t)(4 * ((r - 3) * rsw + jq))};
}

// The slot table of a set of cells staged with row stride fast_rs (fast_row_stride): cells of equal (rw, rh, o) share
// their entries (nd and the stride follow from them), every cell's run is padded to whole rounds, and one round more
// (a round loads the next one without asking whether it exists), with slots that test its first pair and keep no
// column, and Cell::slot_off is set.  The table is never empty and a cell without a window points at entry 0, so
// that a wave may load its first round before it knows whether it has one.
inline void plan_fast_slots(std::vector<Cell> &cells, int fast_rs, std::vector<FastSlot> &table) {
    table.clear();
    std::map<std::tuple<int, int, int>, int> seen;
    for (Cell &c : cells) {
        c.slot_off = 0;
        if (c.np <= 0) continue;
        const int rw = c.x1 - c.x0, rh = c.y1 - c.y0;
        const auto key = std::make_tuple(rw, rh, c.o);
        const auto it = seen.find(key);
        if (it != seen.end()) {
            c.slot_off = it->second;
            continue;
        }
        c.slot_off = (int)table.size();
        seen.emplace(key, c.slot_off);
        const int rsw = fast_rs > 0 ? fast_rs >> 2 : c.nd;
        const int padded = (c.np + kSlotRound - 1) / kSlotRound * kSlotRound + kSlotRound;
        const FastSlot first = fast_slot(c, rsw, 0);
        for (int tp = 0; tp < padded; ++tp)
            table.push_back(tp < c.np ? fast_slot(c, rsw, tp) : FastSlot{0u, first.hi});
    }
    if (table.empty()) table.assign(kSlotRound, FastSlot{0u, 0u});
}

// describe's horizontal 7-tap sums as an i8 MFMA: the banded Toeplitz operand B[k][c'] = g[k - c' - po] of lane l
// (k = 8 (l >> 4) + j in byte j, c' = l & 15) for a patch whose column 0 is raw byte po, g = [18, 34, 48, 56, 48, 34, 18]:
// entry [po][lane], po = 0 .. 3.
inline void describe_bop_table(uint64_t out[4 * 64]) {
    const int g[7] = {18, 34, 48, 56, 48, 34, 18};
    for (int po = 0; po < 4; ++po)
        for (int lane = 0; lane < 64; ++lane) {
            uint64_t w = 0;
            for (int j = 0; j < 8; ++j) {
                const int tap = 8 * (lane >> 4) + j - (lane & 15) - po;
                if (tap >= 0 && tap < 7) w |= (uint64_t)g[tap] << (8 * j);
            }
            out[po * 64 + lane] = w;
        }
}

}  // namespace omv_fast_plan
