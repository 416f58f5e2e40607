// Moving task boards (contract U1-M): the host arithmetic of a call -- the contract's advance, a
// task's per-axis span over the call, the box of all spans and the call's grid on it.  Pure arithmetic, no HIP
// includes, so that a plain host program can drive it (tests/task_motion/task_motion_main.cpp); task_board.hip
// compiles the same functions for the device (SWARM_HD), so the span-box reduction there and task_span_box here
// give the same four doubles.  The lists themselves are built on the device, every tick (task_board.hip).
//
// Unlike a moving obstacle field (obstacle_motion.h), a result bit rests on this box: an agent more than
// kTaskOutside beyond the box on some axis skips its task window (task_window_empty, task_grid.h), which is right
// only while every task is inside the box.  So the box must hold every position Q_k, k = 0 .. ticks, of every task.
//
// The proof, per axis.  x_0 = x, x_{k+1} = fl(x_k + d) with d = fl(v * dt) the same at every step (task_advance).
//   1. Monotone.  Rounding is monotone, so d >= 0 gives x_{k+1} = fl(x_k + d) >= fl(x_k) = x_k, and d <= 0 the
//      reverse: every x_k lies between x_0 and x_ticks.  Only x_ticks needs a bound.
//   2. Drift.  Let M = max(|x|, |x + ticks d|) + |d|.  While |x_k| <= 2 M, one step's rounding error is at most
//      half an ulp of its result, at most 2^-53 * 2 M = 2^-52 M.  By induction e_k = |x_k - (x + k d)| <=
//      k 2^-52 M: the exact x + k d lies between x and x + ticks d, so |x + k d| <= M - |d| and |x_k| <= M + e_k
//      <= M (1 + ticks 2^-52) < 2 M (ticks < 2^31), which keeps the premise.  So e_ticks <= ticks 2^-52 M.
//   3. The computed corner.  xe = fl(x + fl(ticks * d)) differs from x + ticks d by two roundings.  The product:
//      |ticks d| <= |x| + |x + ticks d| <= 2 M (x and x + ticks d may have opposite signs), so its rounding is at
//      most 2^-53 * 2 M = 2^-52 M.  The sum: its result has magnitude at most M (1 + 2^-52), so its rounding is at
//      most 2^-52 M as well.  Together |xe - (x + ticks d)| <= 2^-51 M.  `big` below is fl(max(|a|, |b|) + |d|) >=
//      M (1 - 2^-50), where a, b are x and xe in order (|xe| is within 2^-51 M of |x + ticks d|).
//   4. The pad.  Needed: e_ticks + |xe - (x + ticks d)| <= (ticks + 2) 2^-52 M, plus the rounding of a - pad and
//      b + pad themselves, at most an ulp of a value of magnitude <= 2 M: 2^-51 M.  Together (ticks + 4) 2^-52 M.
//      Had: pad = fl(big * fl((ticks + 4) * 2^-51)) >= (ticks + 4) 2^-51 M (1 - 2^-49) = (2 ticks + 8) 2^-52 M
//      (1 - 2^-49): twice that, but for a factor 1 - 2^-49.  So lo = fl(a - pad) <= x_k <= fl(b + pad) = hi for
//      k = 0 .. ticks.
// The driver checks the claim by iterating the advance: random and adversarial draws (|x| = 1e9, v dt below one
// ulp of x, opposite signs, ticks = 1 and 10^6).  A non-finite lo or hi (an overflow on the way) makes the call's
// box non-finite, and the call is refused.
#pragma once

#include <cmath>
#include <cstdint>

#include "task_grid.h"

#if defined(__HIPCC__)
#define SWARM_HD __host__ __device__
#else
#define SWARM_HD
#endif

namespace swarm {

enum TaskMotionStatus {
    kTaskMotionOk = 0,
    kTaskMotionNonFinite,  // a velocity or a position is NaN or infinite
    kTaskMotionExtent,     // a span overflows, or the box of all spans has no finite extent
};

// The contract's advance of one coordinate: the product and the sum rounded separately (-ffp-contract=off), as
// obs_advance does.
SWARM_HD static inline double task_advance(double x, double v, double dt) {
    const double d = v * dt;
    return x + d;
}

// One axis of a task over a call: [lo, hi] holds x_k for k = 0 .. ticks (the proof above): obs_axis_span's
// argument with h = 0, restated.
SWARM_HD static inline void task_axis_span(double x, double v, double dt, int32_t ticks, double *lo, double *hi) {
    const double d = v * dt, xe = x + double(ticks) * d;
    const double a = x < xe ? x : xe, b = x < xe ? xe : x;
    const double fa = a < 0 ? -a : a, fb = b < 0 ? -b : b, fd = d < 0 ? -d : d;
    const double big = (fa > fb ? fa : fb) + fd;
    const double pad = big * ((double(ticks) + 4.0) * 0x1p-51);
    *lo = a - pad;
    *hi = b + pad;
}

SWARM_HD static inline bool task_finite(double v) { return v - v == 0.0; }  // false for NaN and the infinities

// A box folded over spans: (xmin, ymin, xmax, ymax); a non-finite span end makes xmax +inf, whatever the order
// of the fold (a NaN would vanish in a comparison).
struct TaskBox {
    double xmin, ymin, xmax, ymax;
};
constexpr double kBoxEmptyLo = 1.7976931348623157e308, kBoxEmptyHi = -1.7976931348623157e308;

SWARM_HD static inline void task_box_add(TaskBox *b, double x, double y, double vx, double vy, double dt,
                                         int32_t ticks) {
    double x0, x1, y0, y1;
    task_axis_span(x, vx, dt, ticks, &x0, &x1);
    task_axis_span(y, vy, dt, ticks, &y0, &y1);
    if (!(task_finite(x0) && task_finite(x1) && task_finite(y0) && task_finite(y1))) {
        b->xmax = HUGE_VAL;
        return;
    }
    b->xmin = x0 < b->xmin ? x0 : b->xmin, b->xmax = x1 > b->xmax ? x1 : b->xmax;
    b->ymin = y0 < b->ymin ? y0 : b->ymin, b->ymax = y1 > b->ymax ? y1 : b->ymax;
}

// The box of the T tasks' spans over `ticks` advances (vel NULL: all zero).  T == 0: the empty box.
static inline TaskBox task_span_box(int64_t T, const double *pos, const double *vel, double dt, int32_t ticks) {
    TaskBox b{kBoxEmptyLo, kBoxEmptyLo, kBoxEmptyHi, kBoxEmptyHi};
    for (int64_t k = 0; k < T; ++k)
        task_box_add(&b, pos[2 * k], pos[2 * k + 1], vel ? vel[2 * k] : 0.0, vel ? vel[2 * k + 1] : 0.0, dt, ticks);
    return b;
}

static inline bool task_velocities_finite(int64_t T, const double *vel) {
    for (int64_t q = 0; q < 2 * T; ++q)
        if (!std::isfinite(vel[q])) return false;
    return true;
}

// The call's grid from the box of all spans: build_task_cells' shaping (kTaskCell, at most 4 T + 1024 cells).
// kTaskMotionExtent, *out untouched: a box that is not finite or whose extent is not.  T == 0: one empty cell.
static inline TaskMotionStatus task_grid_of_box(int64_t T, const TaskBox &box, Grid *out) {
    Grid g{};
    if (T == 0) {
        g.cell = g.inv_cell = 1.0;
        g.ncx = g.ncy = 1;
        *out = g;
        return kTaskMotionOk;
    }
    if (!(std::isfinite(box.xmin) && std::isfinite(box.ymin) && std::isfinite(box.xmax) && std::isfinite(box.ymax)))
        return kTaskMotionExtent;
    g.xmin = box.xmin, g.ymin = box.ymin, g.xmax = box.xmax, g.ymax = box.ymax;
    if (!shape_grid(&g, kTaskCell, 4 * T + 1024)) return kTaskMotionExtent;
    *out = g;
    return kTaskMotionOk;
}

// A call's whole host side: the velocities and positions checked, the box, the grid.  Nothing is written to
// *out on any status but kTaskMotionOk.
static inline TaskMotionStatus task_call_grid(int64_t T, const double *pos, const double *vel, double dt,
                                              int32_t ticks, Grid *out) {
    if (vel && !task_velocities_finite(T, vel)) return kTaskMotionNonFinite;
    for (int64_t q = 0; q < 2 * T; ++q)
        if (!std::isfinite(pos[q])) return kTaskMotionNonFinite;
    return task_grid_of_box(T, task_span_box(T, pos, vel, dt, ticks), out);
}

// The grid swarm_board_create chooses for a list (build_task_cells' shaping, statement for statement: the
// tasks' own box through shape_grid), without the lists.
static inline TaskMotionStatus task_static_grid(int64_t T, const double *pos, Grid *out) {
    for (int64_t q = 0; q < 2 * T; ++q)
        if (!std::isfinite(pos[q])) return kTaskMotionNonFinite;
    TaskBox b{kBoxEmptyLo, kBoxEmptyLo, kBoxEmptyHi, kBoxEmptyHi};
    for (int64_t k = 0; k < T; ++k) {
        const double x = pos[2 * k], y = pos[2 * k + 1];
        b.xmin = x < b.xmin ? x : b.xmin, b.xmax = x > b.xmax ? x : b.xmax;
        b.ymin = y < b.ymin ? y : b.ymin, b.ymax = y > b.ymax ? y : b.ymax;
    }
    return task_grid_of_box(T, b, out);
}

}  // namespace swarm
