// Drives csrc/grid_shape.h on the host (no HIP): shape_grid must refuse a box without a finite extent and
// must END for every other box, with at most max_cells cells of at least the requested side.  Built and
// run by tests/test_grid_shape.py (g++ -I<csrc>); prints one line per case, exit status = failed cases.
#include <cstdint>
#include <cstdio>

#include "grid_shape.h"

using swarm::Grid;
using swarm::shape_grid;

static int failed = 0;

static void fail(const char *name, const char *what) {
    std::printf("FAIL %s: %s\n", name, what);
    ++failed;
}

static Grid box(double x0, double y0, double x1, double y1) {
    Grid g{};
    g.xmin = x0; g.ymin = y0; g.xmax = x1; g.ymax = y1;
    g.ncx = g.ncy = -7;  // a refusal leaves the shape alone
    return g;
}

static void refused(const char *name, Grid g, double cell, int64_t max_cells) {
    if (shape_grid(&g, cell, max_cells)) return fail(name, "accepted a box without a finite extent");
    if (g.ncx != -7 || g.ncy != -7) return fail(name, "a refusal wrote the shape");
    std::printf("ok %s refused\n", name);
}

// want_nc > 0: the grid must be want_nc x want_nc cells of side within [cell_lo, cell_hi]
static void accepted(const char *name, Grid g, double cell, int64_t max_cells, int64_t want_nc = 0,
                     double cell_lo = 0, double cell_hi = 0) {
    if (!shape_grid(&g, cell, max_cells)) return fail(name, "refused");
    std::printf("ok %s ncx=%lld ncy=%lld cell=%.17g\n", name, (long long)g.ncx, (long long)g.ncy, g.cell);
    if (g.ncx < 1 || g.ncy < 1) return fail(name, "empty grid");
    if (double(g.ncx) * double(g.ncy) > double(max_cells)) return fail(name, "more than max_cells cells");
    if (!(g.cell >= cell)) return fail(name, "cells smaller than requested");
    if (!(g.inv_cell == 1.0 / g.cell)) return fail(name, "inv_cell");
    // the last cell of each axis holds the box's far edge
    if (!(double(g.ncx) * g.cell > g.xmax - g.xmin && double(g.ncy) * g.cell > g.ymax - g.ymin))
        return fail(name, "the grid does not cover the box");
    if (want_nc && (g.ncx != want_nc || g.ncy != want_nc)) return fail(name, "unexpected cell count");
    if (want_nc && !(g.cell >= cell_lo && g.cell <= cell_hi)) return fail(name, "unexpected cell side");
}

int main() {
    const double inf = HUGE_VAL;
    // finite corners, extent inf: the parent's loop never ended on these
    refused("x_pm1e308", box(-1e308, 0, 1e308, 0), 1.0, 1032);
    refused("y_pm1e308", box(0, -1e308, 0, 1e308), 1.0, 1032);
    refused("both_pm1e308", box(-1e308, -1e308, 1e308, 1e308), 1e-300, 1032);
    refused("dbl_max", box(-1.7976931348623157e308, 0, 1.7976931348623157e308, 1), 1e300, 1032);
    refused("inf_corner", box(0, 0, inf, 1), 1.0, 1032);
    refused("nan_corner", box(0, 0, std::nan(""), 1), 1.0, 1032);
    // large but finite: must end
    accepted("extent_1e300", box(0, 0, 1e300, 1e300), 1.0, 1032);
    accepted("extent_1e300_x_only", box(-5e299, 3, 5e299, 3), 1.0, 1032);
    accepted("cell_1e-300_extent_1e308", box(0, 0, 1e308, 1e308), 1e-300, 1032);
    accepted("extent_largest_finite", box(-8.9e307, 0, 8.9e307, 0), 1e-300, 1032);
    accepted("cell_largest_double", box(0, 0, 10, 10), 1.7976931348623157e308, 1032, 1, 1.7e308, inf);
    accepted("cell_overflows_while_growing", box(0, 0, 1.7e308, 1.7e308), 1e308, 1);
    // zero extent: one cell of the requested side
    accepted("zero_extent", box(3.5, 2.25, 3.5, 2.25), 1.0 + 1e-9, 1824, 1, 1.0 + 1e-9, 1.0 + 1e-9);
    // 64 agents over 1e4 x 1e4 with radius 1: the cap 4 * 64 + 1024 = 1280 grows the cells to 2^8.5 ~ 362
    accepted("sparse_64_agents", box(0, 0, 1e4, 1e4), 1.0 * (1.0 + 1e-9), 4 * 64 + 1024, 28, 362.0, 362.1);
    // nothing to grow: cells of the requested side
    accepted("dense", box(0, 0, 28.0, 28.0), 1.0, 4 * 2000 + 1024, 29, 1.0, 1.0);
    accepted("one_row", box(0, 7, 100, 7), 1.0, 4 * 300 + 1024);
    std::printf("%d failed\n", failed);
    return failed;
}
