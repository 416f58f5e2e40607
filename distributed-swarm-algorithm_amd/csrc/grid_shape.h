// The shape of a uniform grid of cells over a bounding box: pure host arithmetic, no HIP includes, so that a
// plain host program can drive it (tests/grid_shape/grid_shape_main.cpp proves that it ends).
#pragma once

#include <cmath>
#include <cstdint>

namespace swarm {

// A uniform grid of cells over a bounding box (binning.h bins agents into one).
struct Grid {
    double xmin, ymin, xmax, ymax;
    double cell, inv_cell;
    int64_t ncx, ncy;
};

// Cells of side >= `cell` over g's bounding box (enlarged until the grid has at most max_cells).  False, with
// g's shape untouched, when the box's extent is not finite: finite corners whose difference overflows a
// double (-1e308 and +1e308) give inf / c, and once c has grown to inf as well, inf / inf = NaN fails every
// comparison -- the loop below would never end.  With a finite extent it ends: c grows by sqrt(2) a turn,
// and from c > extent on (c = inf included: extent / inf = 0) the grid is 1 x 1.
static inline bool shape_grid(Grid *g, double cell, int64_t max_cells) {
    const double ex = g->xmax - g->xmin, ey = g->ymax - g->ymin;
    if (!(std::isfinite(ex) && std::isfinite(ey))) return false;
    if (max_cells < 1) max_cells = 1;  // a 1 x 1 grid is always reached
    double c = cell > 0 ? cell : 1.0;
    for (;;) {
        const double fx = std::floor(ex / c) + 1.0;
        const double fy = std::floor(ey / c) + 1.0;
        if (fx * fy <= double(max_cells)) {
            g->ncx = int64_t(fx);
            g->ncy = int64_t(fy);
            break;
        }
        c *= 1.4142135623730951;
    }
    g->cell = c;
    g->inv_cell = 1.0 / c;
    return true;
}

constexpr const char *kExtentError =
    "the positions' bounding box has no finite extent (max - min overflows a double)";

}  // namespace swarm
