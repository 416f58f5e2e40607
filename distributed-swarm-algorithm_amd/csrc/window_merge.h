// The streaming nine-way merge over an agent's 3 x 3 cell window (physics.hip k_physics_sensed describes
// it), as a function over "candidate (j, q)": storage index j at cell-sorted position q, visited in ascending
// j -- the agent itself included, the caller's predicate decides the rest.  A window is up to nine runs of
// sorted_idx, one per cell, each ascending (the binning's sort is stable): nine cursors, ends and head
// indices in registers, the smallest head taken each turn; no list, no capacity, no fallback.
// k_physics_sensed and window_separation (physics.hip) keep their own written-out copies of these
// statements: their machine code is what S1's and U1-S's figures were measured on, and
// window_separation through this function compiles k_physics_loop_sensed to 1 141 instructions for 1 169
// (the candidate's position is loaded after the next head, not before).  New walkers go through this one.
// window_cell is the window's "which of the nine cells are in the grid" for code that reads a per-cell array
// (protocol.hip hear_window).  The merge below and protocol.hip k_task_conflicts keep the same arithmetic
// written out: through window_cell, in any form tried, k_task_conflicts compiles to other instructions (757
// against 708-915), and its machine code is what U1-T's figures were measured on.
#pragma once

#include "swarm_common.h"

namespace swarm {

constexpr int32_t kMergeEnd = 0x7fffffff;  // no head: the run is exhausted (n < 2^31 - 1)

// Cell k (0 .. 8, row by row) of the 3 x 3 window around cell (cx, cy): whether it is in the grid, and its
// index there (0 outside, so that a byte or an offset of it can be loaded ahead of the test).
struct WindowCell {
    bool in;
    int64_t at;
};
__device__ __forceinline__ WindowCell window_cell(const Grid &g, int64_t cx, int64_t cy, int k) {
    const int64_t yy = cy + (k / 3) - 1, xx = cx + (k % 3) - 1;
    const bool in = yy >= 0 && yy < g.ncy && xx >= 0 && xx < g.ncx;
    return {in, in ? yy * g.ncx + xx : 0};
}

template <class Visit>
__device__ __forceinline__ void window_merge(double px, double py, const Grid &g,
                                             const int32_t *__restrict__ sorted_idx,
                                             const uint32_t *__restrict__ off, Visit &&visit) {
    const int64_t cx = cell_coord(px, g.xmin, g.inv_cell, g.ncx);
    const int64_t cy = cell_coord(py, g.ymin, g.inv_cell, g.ncy);
    uint32_t cur[9], end[9];
    int32_t head[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int64_t yy = cy + (k / 3) - 1, xx = cx + (k % 3) - 1;
        const bool in = yy >= 0 && yy < g.ncy && xx >= 0 && xx < g.ncx;
        const int64_t c = in ? yy * g.ncx + xx : 0;
        cur[k] = in ? off[c] : 0u;
        end[k] = in ? off[c + 1] : 0u;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) head[k] = cur[k] < end[k] ? sorted_idx[cur[k]] : kMergeEnd;
    for (;;) {
        int32_t j = head[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) j = head[k] < j ? head[k] : j;
        if (j == kMergeEnd) break;
        uint32_t q = 0, e = 0;  // the run that holds j (indices are distinct: exactly one)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const bool hit = head[k] == j;
            q = hit ? cur[k] : q;
            e = hit ? end[k] : e;
        }
        const uint32_t qn = q + 1;
        const int32_t hn = qn < e ? sorted_idx[qn] : kMergeEnd;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const bool hit = head[k] == j;
            cur[k] = hit ? qn : cur[k];
            head[k] = hit ? hn : head[k];
        }
        visit(j, q);
    }
}

}  // namespace swarm
