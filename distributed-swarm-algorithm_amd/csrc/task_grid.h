// A task board's cell grid (contract U1-B): which tasks an agent has to look at so that its claim
// evaluation keeps the bits of a walk over the whole board.  Pure host arithmetic, no HIP includes, so that a
// plain host program or a test can drive it (tests/task_grid/task_grid_main.cpp).  Built once per board, on the
// host, with plain loops: every cell's tasks in ascending task index, no atomics, the same lists on every run.
//
// Why the 3 x 3 window suffices.  The claim evaluation (protocol.hip, k_tick_radio_board) skips task (tx, ty)
// for an agent at (px, py) unless  fl(fl(dx * dx) + fl(dy * dy)) <= 25  with dx = fl(px - tx): the far pre-test,
// exact, and a skipped task is neither claimed nor counted in the guard band.
//   1. Passing it means dx * dx <= 25 (1 + 2^-52), so |dx| <= 5 (1 + 2^-52), and the real difference is within
//      a relative 2^-53 of dx: |px - tx| <= 5 (1 + 2^-51) < 5 (1 + 1e-9) <= cell.  Likewise for y.
//   2. task_cell_coord (cell_coord's arithmetic, swarm_common.h) is monotone non-decreasing in v, clamps
//      included, and two reals less than one cell apart differ by at most one in floor((v - vmin) / cell); the
//      roundings of the subtraction and of the product with inv_cell move either operand by a relative 2^-52,
//      far inside the 1e-9 margin.  The clamp to [0, nc - 1] never widens a difference.
//   3. So |cell(px) - cell(tx)| <= 1 on both axes for every task that can pass the pre-test -- also for an agent
//      outside the tasks' box, which the clamps put in an edge cell.  The window may only ever offer a superset;
//      every offered task goes through the pre-test itself.
// An agent further than kTaskOutside beyond the box on some axis passes the pre-test for no task (every task is
// inside the box, so |dx| > 5.9): task_window_empty lets it skip the window.  A NaN coordinate fails the four
// comparisons, falls in cell 0 of its axis and fails every pre-test there by itself.
#pragma once

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "grid_shape.h"

namespace swarm {

constexpr int64_t kMaxBoardTasks = int64_t(1) << 24;
constexpr double kTaskCell = 5.0 * (1.0 + 1e-9);  // the narrowest cell (shape_grid grows it to fit the cell cap)
constexpr double kTaskOutside = 6.0;

enum TaskCellsStatus {
    kTaskCellsOk = 0,
    kTaskCellsNonFinite,  // a task position is NaN or infinite
    kTaskCellsExtent,     // the tasks' box has no finite extent (shape_grid refuses it)
    kTaskCellsMemory,     // the host ran out of memory for the lists
};

struct TaskCells {
    Grid g{};                        // covers the tasks' bounding box
    int64_t T = 0, longest = 0;      // tasks, and the longest cell list
    std::vector<uint32_t> cell_off;  // ncx * ncy + 1: cell c's tasks are idx[cell_off[c] .. cell_off[c + 1])
    std::vector<int32_t> idx;        // task indices, ascending within a cell
};

// cell_coord's arithmetic (swarm_common.h) for the host.
static inline int64_t task_cell_coord(double v, double vmin, double inv_cell, int64_t nc) {
    const double f = std::floor((v - vmin) * inv_cell);
    if (!(f >= 0.0)) return 0;  // also catches NaN
    if (f >= double(nc - 1)) return nc - 1;
    return int64_t(f);
}

// No task of a board whose box is g's can pass the far pre-test for an agent at (px, py).
static inline bool task_window_empty(const Grid &g, double px, double py) {
    return px < g.xmin - kTaskOutside || px > g.xmax + kTaskOutside || py < g.ymin - kTaskOutside ||
           py > g.ymax + kTaskOutside;
}

// The grid and cell lists of the T tasks tpos[2 k .. 2 k + 1] = (x, y), T <= 2^24.  On any status but
// kTaskCellsOk *out holds no list.
static inline TaskCellsStatus build_task_cells(int64_t T, const double *tpos, TaskCells *out) {
    *out = TaskCells{};
    out->T = T;
    for (int64_t q = 0; q < 2 * T; ++q)
        if (!std::isfinite(tpos[q])) return kTaskCellsNonFinite;
    Grid g{};
    if (T == 0) {  // one empty cell
        g.cell = g.inv_cell = 1.0;
        g.ncx = g.ncy = 1;
        out->g = g;
        try {
            out->cell_off.assign(2, 0u);
        } catch (const std::bad_alloc &) {
            return kTaskCellsMemory;
        }
        return kTaskCellsOk;
    }
    g.xmin = g.xmax = tpos[0];
    g.ymin = g.ymax = tpos[1];
    for (int64_t k = 1; k < T; ++k) {
        const double x = tpos[2 * k], y = tpos[2 * k + 1];
        g.xmin = x < g.xmin ? x : g.xmin, g.xmax = x > g.xmax ? x : g.xmax;
        g.ymin = y < g.ymin ? y : g.ymin, g.ymax = y > g.ymax ? y : g.ymax;
    }
    if (!shape_grid(&g, kTaskCell, 4 * T + 1024)) return kTaskCellsExtent;
    const int64_t cells = g.ncx * g.ncy;
    std::vector<uint32_t> cur;
    try {
        out->cell_off.assign(size_t(cells) + 1, 0u);
        out->idx.assign(size_t(T), 0);
        cur.assign(size_t(cells), 0u);
    } catch (const std::bad_alloc &) {
        *out = TaskCells{};
        out->T = T;
        return kTaskCellsMemory;
    }
    auto cell_of = [&](int64_t k) {
        return task_cell_coord(tpos[2 * k + 1], g.ymin, g.inv_cell, g.ncy) * g.ncx +
               task_cell_coord(tpos[2 * k], g.xmin, g.inv_cell, g.ncx);
    };
    uint32_t *off = out->cell_off.data();
    for (int64_t k = 0; k < T; ++k) ++off[cell_of(k) + 1];
    int64_t longest = 0;
    for (int64_t c = 0; c < cells; ++c) {
        longest = int64_t(off[c + 1]) > longest ? int64_t(off[c + 1]) : longest;
        off[c + 1] += off[c];
    }
    for (int64_t c = 0; c < cells; ++c) cur[size_t(c)] = off[c];
    for (int64_t k = 0; k < T; ++k) out->idx[cur[size_t(cell_of(k))]++] = int32_t(k);  // task by task: ascending
    out->g = g;
    out->longest = longest;
    return kTaskCellsOk;
}

// The tasks the window around (px, py) offers, in window order (cell by cell, row by row): what the kernel
// visits.  For tests and tools.
static inline void task_window(const TaskCells &tc, double px, double py, std::vector<int32_t> *offered) {
    offered->clear();
    if (tc.T == 0 || task_window_empty(tc.g, px, py)) return;
    const Grid &g = tc.g;
    const int64_t cx = task_cell_coord(px, g.xmin, g.inv_cell, g.ncx);
    const int64_t cy = task_cell_coord(py, g.ymin, g.inv_cell, g.ncy);
    for (int k = 0; k < 9; ++k) {
        const int64_t yy = cy + (k / 3) - 1, xx = cx + (k % 3) - 1;
        if (yy < 0 || yy >= g.ncy || xx < 0 || xx >= g.ncx) continue;
        const int64_t c = yy * g.ncx + xx;
        for (uint32_t q = tc.cell_off[size_t(c)]; q < tc.cell_off[size_t(c) + 1]; ++q) offered->push_back(tc.idx[q]);
    }
}

}  // namespace swarm
