// Moving obstacle fields (contract O2): the host arithmetic of a call -- the contract's advance, the
// call's grid and the capacity of the device builder's pair buffers.  Pure host arithmetic, no HIP includes, so
// that a plain host program can drive it (tests/obstacle_motion/obstacle_motion_main.cpp).  The lists
// themselves are built on the device, every tick (obstacle_field.hip); nothing here decides a bit of a result:
// cell_coord clamps, so any grid gives the flat list's bits (obstacle_cells.h, step 4) -- the grid and the
// capacity decide list lengths and memory only.
#pragma once

#include <cmath>
#include <cstdint>

#include "obstacle_cells.h"

namespace swarm {

enum ObsMotionStatus {
    kObsMotionOk = 0,
    kObsMotionNonFinite,  // a velocity (or a list entry) is NaN or infinite
    kObsMotionExtent,     // the box of the call's footprints has no finite extent
    kObsMotionPairs,      // the capacity bound exceeds kMaxObsPairs
};

// The contract's advance of one coordinate: the product and the sum rounded separately (-ffp-contract=off).
static inline double obs_advance(double x, double v, double dt) {
    const double d = v * dt;
    return x + d;
}

static inline bool obs_velocities_finite(int64_t m, const double *vel) {
    for (int64_t q = 0; q < 2 * m; ++q)
        if (!std::isfinite(vel[q])) return false;
    return true;
}

// The grid swarm_obstacle_field_create chooses for a list (build_obstacle_cells' shaping, statement for
// statement: the box of the live footprints through shape_grid with obs_start_side and the 4 live + 1024 cap).
static inline ObsMotionStatus obs_static_grid(int64_t m, const double *obs, Grid *out, int64_t *live_out) {
    for (int64_t q = 0; q < 3 * m; ++q)
        if (!std::isfinite(obs[q])) return kObsMotionNonFinite;
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
    *live_out = live;
    if (live == 0) {  // one empty cell
        g.cell = g.inv_cell = 1.0;
        g.ncx = g.ncy = 1;
        *out = g;
        return kObsMotionOk;
    }
    if (!shape_grid(&g, obs_start_side(hsum / double(live)), 4 * live + 1024)) return kObsMotionExtent;
    *out = g;
    return kObsMotionOk;
}

// One axis of a moving footprint over a call: [lo, hi] holds fl(x_k - h) and fl(x_k + h) for every position
// x_k, k = 0 .. ticks, of the contract's advance from x with the step d = fl(v * dt).
//   The x_k are monotone in k: x_{k+1} = fl(x_k + d) with the same d, and rounding is monotone, so d >= 0 gives
//   x_{k+1} >= x_k and d <= 0 the reverse.  Each step's rounding error is at most half an ulp of its result,
//   at most 2^-53 M with M = max(|x|, |x + ticks d|) + |d| an upper bound on every |x_k| up to the errors
//   themselves; after k <= ticks steps |x_k - (x + k d)| <= ticks 2^-53 M (1 + ticks 2^-53).  The pad below is
//   four times that plus four ulps of the corner, which also covers the roundings of x + ticks d, of the corner
//   itself and of fl(x_k -+ h).  (ticks < 2^31, so ticks 2^-51 < 2^-20.)
// A non-finite lo or hi (an overflow on the way) is left for the caller's extent check.
static inline void obs_axis_span(double x, double v, double h, double dt, int32_t ticks, double *lo, double *hi) {
    const double d = v * dt, xe = x + double(ticks) * d;
    const double a = x < xe ? x : xe, b = x < xe ? xe : x;
    const double big = (std::fabs(a) > std::fabs(b) ? std::fabs(a) : std::fabs(b)) + std::fabs(d) + h;
    const double pad = big * ((double(ticks) + 4.0) * 0x1p-51);
    *lo = a - h - pad;
    *hi = b + h + pad;
}

// The call's grid: the box of the live footprints at entry and wherever the velocities put them in `ticks`
// advances, through shape_grid as obs_static_grid does.  Correctness never depends on this box.
static inline ObsMotionStatus obs_call_grid(int64_t m, const double *obs, const double *vel, double dt, int32_t ticks,
                                            Grid *out, int64_t *live_out) {
    Grid g{};
    int64_t live = 0;
    double hsum = 0.0;
    bool finite = true;
    for (int64_t o = 0; o < m; ++o) {
        double h, x0, x1, y0, y1;
        if (!obs_half_side(obs + 3 * o, &h)) continue;
        obs_axis_span(obs[3 * o], vel ? vel[2 * o] : 0.0, h, dt, ticks, &x0, &x1);
        obs_axis_span(obs[3 * o + 1], vel ? vel[2 * o + 1] : 0.0, h, dt, ticks, &y0, &y1);
        finite = finite && std::isfinite(x0) && std::isfinite(x1) && std::isfinite(y0) && std::isfinite(y1);
        if (live == 0) {
            g.xmin = x0, g.xmax = x1, g.ymin = y0, g.ymax = y1;
        } else {
            g.xmin = x0 < g.xmin ? x0 : g.xmin, g.xmax = x1 > g.xmax ? x1 : g.xmax;
            g.ymin = y0 < g.ymin ? y0 : g.ymin, g.ymax = y1 > g.ymax ? y1 : g.ymax;
        }
        hsum += h;
        ++live;
    }
    *live_out = live;
    if (live == 0) {
        g.cell = g.inv_cell = 1.0;
        g.ncx = g.ncy = 1;
        *out = g;
        return kObsMotionOk;
    }
    if (!finite) return kObsMotionExtent;
    if (!shape_grid(&g, obs_start_side(hsum / double(live)), 4 * live + 1024)) return kObsMotionExtent;
    *out = g;
    return kObsMotionOk;
}

// ---- the pair capacity: a bound from the radii and the grid alone, wherever the obstacles are ----
//
// Per axis a footprint [a, b], a = fl(ox - h) <= b = fl(ox + h), covers  cell(b) - cell(a) + 1  cells with
// cell(v) = clamp(floor(u(v)), 0, nc - 1), u(v) = fl(fl(v - vmin) * inv) (obs_cell_coord).  Claim: that is at
// most  min(nc, floor(fl(2 h * inv)) + 3)  whenever the grid is "fine" (obs_grid_fine: (|vmin| + (nc + 2) c)
// inv <= 2^40 on that axis); on any other grid the bound is nc, which the clamps give.
//   (i) No clamp bites (0 <= u(a), u(b) < nc).  Then a, b are in [vmin, vmin + nc c (1 + 2^-50)], so every
//   magnitude below is at most M = |vmin| + (nc + 1) c, and M inv <= 2^40.  b - a <= 2 h + 2^-52 M (two
//   roundings of at most half an ulp each).  fl(b - vmin) - fl(a - vmin) <= (b - a) + 2^-52 M, and multiplying
//   by inv and rounding adds at most 2^-52 (nc + 1) more: u(b) - u(a) <= 2 h inv + 2^-50 M inv <= w + 2^-10 with
//   w = 2 h inv.  floor(u(b)) - floor(u(a)) <= floor(u(b) - u(a)) + 1, so the count is at most
//   floor(w + 2^-10) + 2 <= floor(w) + 3.  2 h is exact, and rounding is monotone: an integer k <= w is a double
//   (w < 2^53, else the bound exceeds nc), so fl(w) >= k and floor(fl(w)) >= floor(w).
//   (ii) u(a) < 0: a < vmin and cell(a) = 0 = cell(vmin), u(vmin) = 0; the count is that of [vmin, b], no wider.
//   (iii) u(b) >= nc: cell(b) = nc - 1.  If u(a) >= nc - 1 the count is 1.  Else let b1 be the largest double in
//   [a, b] with u(b1) < nc; its successor has u >= nc and lies within 2^-52 M of b1, so u(b1) >= nc - 2^-10 >
//   nc - 1 and cell(b1) = nc - 1 = cell(b): the count is that of [a, b1], no wider, and (i) applies to it.
// The issue's experiment (4e7 draws) never saw more than floor(w) + 2; the proof pays one more cell for the
// 2^-10 of rounding slack.
static inline bool obs_grid_fine(double vmin, double cell, double inv_cell, int64_t nc) {
    return (std::fabs(vmin) + (double(nc) + 2.0) * cell) * inv_cell <= 0x1p40;
}

static inline int64_t obs_axis_bound(double h, double vmin, double cell, double inv_cell, int64_t nc) {
    if (!obs_grid_fine(vmin, cell, inv_cell, nc)) return nc;
    const double w = std::floor(2.0 * h * inv_cell) + 3.0;
    return w < double(nc) ? int64_t(w) : nc;  // (NaN cannot occur: h and inv_cell are finite)
}

// The capacity for list `obs` (only the radii are read) on grid g: the sum of the per-obstacle products.
// kObsMotionPairs beyond kMaxObsPairs (each product is at most ncx * ncy <= 2^33 + 1024: no overflow before
// the test).
static inline ObsMotionStatus obs_pair_capacity(int64_t m, const double *obs, const Grid &g, int64_t *cap) {
    int64_t sum = 0;
    for (int64_t o = 0; o < m; ++o) {
        double h;
        if (!obs_half_side(obs + 3 * o, &h)) continue;
        sum += obs_axis_bound(h, g.xmin, g.cell, g.inv_cell, g.ncx) * obs_axis_bound(h, g.ymin, g.cell, g.inv_cell, g.ncy);
        if (sum > kMaxObsPairs) return kObsMotionPairs;
    }
    *cap = sum;
    return kObsMotionOk;
}

// A call's whole host side: velocities checked, the call's grid, the capacity on it.  Nothing is allocated.
struct ObsCallPlan {
    Grid g{};
    int64_t live = 0, capacity = 0;
};
static inline ObsMotionStatus plan_obstacle_call(int64_t m, const double *obs, const double *vel, double dt,
                                                 int32_t ticks, ObsCallPlan *out) {
    *out = ObsCallPlan{};
    if (vel && !obs_velocities_finite(m, vel)) return kObsMotionNonFinite;
    for (int64_t q = 0; q < 3 * m; ++q)
        if (!std::isfinite(obs[q])) return kObsMotionNonFinite;
    ObsMotionStatus st = obs_call_grid(m, obs, vel, dt, ticks, &out->g, &out->live);
    if (st != kObsMotionOk) return st;
    return obs_pair_capacity(m, obs, out->g, &out->capacity);
}

}  // namespace swarm
