// An obstacle field's cell lists (contract O1): which obstacles an agent in a given grid cell has to
// visit so that its obstacle forces keep the flat list's bits.  Pure host arithmetic, no HIP includes, so that
// a plain host program can drive it (tests/obstacle_cells/obstacle_cells_main.cpp).  Built once per field, on
// the host, with plain loops: the lists are filled in ascending obstacle index, no atomics, hence the same
// lists on every run.
//
// Why the lists suffice.  The flat loop (physics.hip, obstacle_forces) skips obstacle (ox, oy, r) for an agent
// at (px, py) unless  s2 <= rr * rr * (1 + 1e-12)  with rr = 5.0 + r and s2 = fl(fl(ex * ex) + fl(ey * ey)),
// ex = fl(px - ox); a skipped obstacle adds no term, not even +0.0.  An obstacle with rr <= 0 ("dead",
// r <= -5) has sqrt(s2) - r >= 5 for every agent, so its term is skipped by the loop's d < 5.0 and it is in
// no list.  For a live one let h = fl(rr * (1 + 1e-9)):
//   1. A term applies only if |px - ox| < h in real numbers.  Passing the pre-test with finite operands means
//      ex * ex <= s2 (1 + 2^-52) <= rr^2 (1 + 1e-12)(1 + 2^-51), so |ex| <= rr (1 + 1e-12), and the real
//      difference is within a relative 2^-53 of ex: |px - ox| <= rr (1 + 2e-12) < rr (1 + 1e-9)(1 - 2^-52)
//      <= h.  The margin 1e-9 is far above the roundings of s2, the root, the subtraction and h itself.
//      The same holds for y.
//   2. A double px >= ox - h (real) satisfies px >= fl(ox - h), because rounding is monotone and px is a
//      double; likewise px <= fl(ox + h).
//   3. cell_coord (swarm_common.h; obs_cell_coord below is its arithmetic, statement for statement) is
//      monotone non-decreasing in v, its clamps included: v -> fl(v - vmin) -> fl(. * inv_cell), inv_cell >= 0
//      -> floor -> clamp to [0, nc - 1] are all monotone.
//   4. So cell(fl(ox - h)) <= cell(px) <= cell(fl(ox + h)) on both axes for every agent the obstacle can act
//      on -- also for an agent outside the grid's box, which the clamps put in an edge cell of every
//      footprint that reaches it.  The obstacle is listed in exactly those cells.
// An agent with a NaN coordinate falls in cell 0 of that axis; whatever it visits there is skipped by the
// flat statements themselves (NaN fails d < 5.0), as in the flat loop.
#pragma once

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "grid_shape.h"

namespace swarm {

constexpr int64_t kMaxObsPairs = int64_t(1) << 26;  // (cell, obstacle) pairs of one field, at most

enum ObsCellsStatus {
    kObsCellsOk = 0,
    kObsCellsNonFinite,  // an obstacle entry is NaN or infinite
    kObsCellsExtent,     // the footprints' box has no finite extent (shape_grid refuses it)
    kObsCellsPairs,      // more than kMaxObsPairs pairs: counted by arithmetic, nothing allocated
    kObsCellsMemory,     // the host ran out of memory for the lists
};

struct ObsCells {
    Grid g{};                        // covers the bounding box of the live footprints
    int64_t m = 0, live = 0;         // obstacles, and those with 5.0 + r > 0
    int64_t pairs = 0, longest = 0;  // all lists together, and the longest one
    std::vector<uint32_t> cell_off;  // ncx * ncy + 1: cell c's list is idx[cell_off[c] .. cell_off[c + 1])
    std::vector<int32_t> idx;        // obstacle indices, ascending within a cell
};

// cell_coord's arithmetic (swarm_common.h) for the host.
static inline int64_t obs_cell_coord(double v, double vmin, double inv_cell, int64_t nc) {
    const double f = std::floor((v - vmin) * inv_cell);
    if (!(f >= 0.0)) return 0;  // also catches NaN
    if (f >= double(nc - 1)) return nc - 1;
    return int64_t(f);
}

// The half side h of obstacle o's footprint; false for a dead obstacle.
static inline bool obs_half_side(const double *o, double *h) {
    const double rr = 5.0 + o[2];  // the flat loop's own expression
    if (!(rr > 0)) return false;
    *h = rr * (1.0 + 1e-9);
    return true;
}

struct ObsCellRange {
    int64_t x0, x1, y0, y1;
};

// The cells of a live obstacle's footprint [fl(ox - h), fl(ox + h)] x [fl(oy - h), fl(oy + h)] on grid g.
static inline ObsCellRange obs_cell_range(const Grid &g, const double *o, double h) {
    return {obs_cell_coord(o[0] - h, g.xmin, g.inv_cell, g.ncx), obs_cell_coord(o[0] + h, g.xmin, g.inv_cell, g.ncx),
            obs_cell_coord(o[1] - h, g.ymin, g.inv_cell, g.ncy), obs_cell_coord(o[1] + h, g.ymin, g.inv_cell, g.ncy)};
}

// The grid's start side (shape_grid grows it until the grid fits its cell cap), from the mean half side of the
// live footprints.  Rule 1: twice the half side of an r = 0 obstacle, whatever the radii -- an agent's list then
// holds the obstacles within about 10 units of where they can act, also when the radii are large, and obstacles
// far larger than that cost pairs (memory, bounded by kMaxObsPairs) instead of lengthening every agent's walk.
// Rule 0: twice the mean half side (the cells grow with the radii; A/B builds; DESIGN 4j has both measured).
#ifndef SWARM_OBS_START_RULE
#define SWARM_OBS_START_RULE 1
#endif
static inline double obs_start_side(double mean_h) {
    return SWARM_OBS_START_RULE == 0 ? 2.0 * mean_h : 2.0 * (5.0 * (1.0 + 1e-9));
}

// The field of the m obstacles obs[3 o .. 3 o + 2] = (x, y, r), m < 2^31.  On any status but kObsCellsOk *out
// holds no list (its vectors are left empty).
static inline ObsCellsStatus build_obstacle_cells(int64_t m, const double *obs, ObsCells *out) {
    *out = ObsCells{};
    out->m = m;
    for (int64_t q = 0; q < 3 * m; ++q)
        if (!std::isfinite(obs[q])) return kObsCellsNonFinite;
    Grid g{};
    int64_t live = 0;
    double hsum = 0.0;
    for (int64_t o = 0; o < m; ++o) {
        double h;
        if (!obs_half_side(obs + 3 * o, &h)) continue;
        const double x0 = obs[3 * o] - h, x1 = obs[3 * o] + h, y0 = obs[3 * o + 1] - h, y1 = obs[3 * o + 1] + h;
        if (live == 0) {
            g.xmin = x0, g.xmax = x1, g.ymin = y0, g.ymax = y1;
        } else {
            g.xmin = x0 < g.xmin ? x0 : g.xmin, g.xmax = x1 > g.xmax ? x1 : g.xmax;
            g.ymin = y0 < g.ymin ? y0 : g.ymin, g.ymax = y1 > g.ymax ? y1 : g.ymax;
        }
        hsum += h;
        ++live;
    }
    out->live = live;
    if (live == 0) {  // one empty cell
        g.cell = g.inv_cell = 1.0;
        g.ncx = g.ncy = 1;
        out->g = g;
        out->cell_off.assign(2, 0u);
        return kObsCellsOk;
    }
    if (!shape_grid(&g, obs_start_side(hsum / double(live)), 4 * live + 1024)) return kObsCellsExtent;
    // the pair count, by arithmetic alone: a footprint's cell range is a product
    int64_t pairs = 0;
    for (int64_t o = 0; o < m; ++o) {
        double h;
        if (!obs_half_side(obs + 3 * o, &h)) continue;
        const ObsCellRange c = obs_cell_range(g, obs + 3 * o, h);
        pairs += (c.x1 - c.x0 + 1) * (c.y1 - c.y0 + 1);  // <= 4 m + 1024 each: no overflow before the test
        if (pairs > kMaxObsPairs) return kObsCellsPairs;
    }
    const int64_t cells = g.ncx * g.ncy;
    try {
        out->cell_off.assign(size_t(cells) + 1, 0u);
        out->idx.assign(size_t(pairs), 0);
    } catch (const std::bad_alloc &) {
        *out = ObsCells{};
        out->m = m;
        return kObsCellsMemory;
    }
    uint32_t *off = out->cell_off.data();
    for (int64_t o = 0; o < m; ++o) {  // per-cell counts, at off[c + 1]
        double h;
        if (!obs_half_side(obs + 3 * o, &h)) continue;
        const ObsCellRange c = obs_cell_range(g, obs + 3 * o, h);
        for (int64_t y = c.y0; y <= c.y1; ++y)
            for (int64_t x = c.x0; x <= c.x1; ++x) ++off[y * g.ncx + x + 1];
    }
    int64_t longest = 0;
    for (int64_t c = 0; c < cells; ++c) {  // offsets
        longest = int64_t(off[c + 1]) > longest ? int64_t(off[c + 1]) : longest;
        off[c + 1] += off[c];
    }
    std::vector<uint32_t> cur;
    try {
        cur.assign(out->cell_off.begin(), out->cell_off.end() - 1);
    } catch (const std::bad_alloc &) {
        *out = ObsCells{};
        out->m = m;
        return kObsCellsMemory;
    }
    for (int64_t o = 0; o < m; ++o) {  // the fill, obstacle by obstacle: every list ascending
        double h;
        if (!obs_half_side(obs + 3 * o, &h)) continue;
        const ObsCellRange c = obs_cell_range(g, obs + 3 * o, h);
        for (int64_t y = c.y0; y <= c.y1; ++y)
            for (int64_t x = c.x0; x <= c.x1; ++x) out->idx[cur[y * g.ncx + x]++] = int32_t(o);
    }
    out->g = g;
    out->pairs = pairs;
    out->longest = longest;
    return kObsCellsOk;
}

}  // namespace swarm
