// The host arithmetic of moving obstacle fields (contract O2), driven on the CPU: csrc/obstacle_motion.h
// through a plain host program (g++ -ffp-contract=off, the library's flag).  For every accepted case the program
// iterates the contract's advance exactly, tick by tick, and checks on the call's grid that
//   - the counted pairs (obstacle_cells.h's footprint ranges) never exceed the capacity bound;
//   - no obstacle's per-axis cell range exceeds its per-axis bound -- at its position, and with the position
//     snapped to every cell boundary its footprint's corners are next to, and one ulp either side;
//   - the call's box contains every footprint of every tick.
// The same per-axis check runs on the grid a static field of the tick's list would get (refresh's grid).
// Refusals (non-finite velocity, non-finite extent, more than 2^26 pairs by the bound) are checked to come back
// with the plan untouched: nothing was allocated (the header allocates nothing at all).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "obstacle_motion.h"

using namespace swarm;

static int g_failed = 0;

static void fail(const char *name, const char *what, long long a = 0, long long b = 0) {
    printf("FAIL %s: %s (%lld, %lld)\n", name, what, a, b);
    ++g_failed;
}

// cells of [fl(x - h), fl(x + h)] on one axis
static int64_t axis_cells(double x, double h, double vmin, double inv, int64_t nc) {
    return obs_cell_coord(x + h, vmin, inv, nc) - obs_cell_coord(x - h, vmin, inv, nc) + 1;
}

// the per-axis bound at x and at x snapped so that a footprint corner sits on a cell boundary, +- one ulp
static bool axis_ok(double x, double h, double vmin, double cell, double inv, int64_t nc) {
    const int64_t bound = obs_axis_bound(h, vmin, cell, inv, nc);
    if (axis_cells(x, h, vmin, inv, nc) > bound) return false;
    for (int side = -1; side <= 1; side += 2) {
        const double corner = x + side * h;
        const double kf = std::floor((corner - vmin) * inv);
        for (int dk = 0; dk <= 1; ++dk) {
            const double edge = vmin + (kf + dk) * cell;  // a cell boundary next to the corner
            const double xs = edge - side * h;            // the centre that puts the corner there
            if (!std::isfinite(xs)) continue;
            const double tries[3] = {std::nextafter(xs, -HUGE_VAL), xs, std::nextafter(xs, HUGE_VAL)};
            for (double t : tries)
                if (axis_cells(t, h, vmin, inv, nc) > bound) return false;
        }
    }
    return true;
}

static bool axes_ok(const char *name, const Grid &g, const std::vector<double> &obs, int64_t m) {
    for (int64_t o = 0; o < m; ++o) {
        double h;
        if (!obs_half_side(&obs[3 * o], &h)) continue;
        if (!axis_ok(obs[3 * o], h, g.xmin, g.cell, g.inv_cell, g.ncx) ||
            !axis_ok(obs[3 * o + 1], h, g.ymin, g.cell, g.inv_cell, g.ncy)) {
            fail(name, "an axis range exceeds its bound", o);
            return false;
        }
    }
    return true;
}

static void run_case(const char *name, std::vector<double> obs, const std::vector<double> &vel, double dt, int32_t ticks) {
    const int64_t m = int64_t(obs.size() / 3);
    ObsCallPlan plan;
    const ObsMotionStatus st = plan_obstacle_call(m, obs.data(), vel.empty() ? nullptr : vel.data(), dt, ticks, &plan);
    if (st != kObsMotionOk) {
        fail(name, "refused", st);
        return;
    }
    const Grid &g = plan.g;
    int64_t max_pairs = 0, moved_out = 0;
    Grid entry{};
    int64_t entry_live = 0;
    obs_static_grid(m, obs.data(), &entry, &entry_live);
    for (int32_t k = 0; k <= ticks; ++k) {
        int64_t pairs = 0;
        for (int64_t o = 0; o < m; ++o) {
            double h;
            if (!obs_half_side(&obs[3 * o], &h)) continue;
            const ObsCellRange c = obs_cell_range(g, &obs[3 * o], h);
            pairs += (c.x1 - c.x0 + 1) * (c.y1 - c.y0 + 1);
            const double x0 = obs[3 * o] - h, x1 = obs[3 * o] + h, y0 = obs[3 * o + 1] - h, y1 = obs[3 * o + 1] + h;
            if (!(x0 >= g.xmin && x1 <= g.xmax && y0 >= g.ymin && y1 <= g.ymax))
                return fail(name, "a footprint left the call's box at tick", k, o);
            if (k == ticks && entry_live && !(x1 >= entry.xmin && x0 <= entry.xmax && y1 >= entry.ymin && y0 <= entry.ymax))
                ++moved_out;
        }
        if (pairs > plan.capacity) return fail(name, "the counted pairs exceed the capacity", pairs, plan.capacity);
        max_pairs = pairs > max_pairs ? pairs : max_pairs;
        if (!axes_ok(name, g, obs, m)) return;
        // refresh's grid for the list of this tick, and the capacity on it
        Grid sg{};
        int64_t live = 0, cap = 0;
        if (obs_static_grid(m, obs.data(), &sg, &live) != kObsMotionOk) return fail(name, "static grid refused", k);
        if (!axes_ok(name, sg, obs, m)) return;
        if (obs_pair_capacity(m, obs.data(), sg, &cap) == kObsMotionOk) {
            int64_t sp = 0;
            for (int64_t o = 0; o < m; ++o) {
                double h;
                if (!obs_half_side(&obs[3 * o], &h)) continue;
                const ObsCellRange c = obs_cell_range(sg, &obs[3 * o], h);
                sp += (c.x1 - c.x0 + 1) * (c.y1 - c.y0 + 1);
            }
            if (sp > cap) return fail(name, "the static grid's pairs exceed its capacity", sp, cap);
        }
        if (k < ticks)
            for (int64_t o = 0; o < m; ++o) {  // the contract's advance, exactly
                obs[3 * o] = obs_advance(obs[3 * o], vel.empty() ? 0.0 : vel[2 * o], dt);
                obs[3 * o + 1] = obs_advance(obs[3 * o + 1], vel.empty() ? 0.0 : vel[2 * o + 1], dt);
            }
    }
    printf("ok %s m=%lld live=%lld ticks=%d ncx=%lld ncy=%lld capacity=%lld max_pairs=%lld left_entry_box=%lld\n", name,
           (long long)m, (long long)plan.live, int(ticks), (long long)g.ncx, (long long)g.ncy, (long long)plan.capacity,
           (long long)max_pairs, (long long)moved_out);
}

static void refused(const char *name, const std::vector<double> &obs, const std::vector<double> &vel, double dt,
                    int32_t ticks, ObsMotionStatus want) {
    ObsCallPlan plan;
    plan.capacity = -7;
    const ObsMotionStatus st =
        plan_obstacle_call(int64_t(obs.size() / 3), obs.data(), vel.empty() ? nullptr : vel.data(), dt, ticks, &plan);
    if (st != want) return fail(name, "wrong status", st, want);
    if (plan.capacity != 0) return fail(name, "a refused plan holds a capacity", plan.capacity);
    printf("ok %s refused status=%d\n", name, int(st));
}

int main() {
    std::mt19937_64 rng(20260);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    auto random_list = [&](int64_t m, double span, double shift, double rlo, double rhi) {
        std::vector<double> o(size_t(m) * 3);
        for (int64_t q = 0; q < m; ++q) o[3 * q] = shift + uni(0, span), o[3 * q + 1] = shift + uni(0, span), o[3 * q + 2] = uni(rlo, rhi);
        return o;
    };
    auto random_vel = [&](int64_t m, double vmax) {
        std::vector<double> v(size_t(m) * 2);
        for (double &x : v) x = uni(-vmax, vmax);
        return v;
    };
    run_case("random_300", random_list(300, 200, 0, 0.2, 2), random_vel(300, 8), 0.1, 40);
    run_case("random_1025", random_list(1025, 600, -300, 0.2, 2), random_vel(1025, 8), 0.1, 25);
    run_case("m1", random_list(1, 1, 0, 1, 1), random_vel(1, 8), 0.1, 30);
    run_case("m0", {}, {}, 0.1, 10);
    run_case("radii", random_list(200, 500, 0, -6, 300), random_vel(200, 8), 0.1, 20);
    run_case("near_1e9", random_list(100, 300, 1e9, 0.2, 2), random_vel(100, 8), 0.1, 30);
    run_case("near_minus_1e9", random_list(100, 300, -1e9, -6, 30), random_vel(100, 8), 0.1, 30);
    {
        std::vector<double> o(90), v(60);
        for (int q = 0; q < 30; ++q) o[3 * q] = 7.0 * q, o[3 * q + 1] = 3.0, o[3 * q + 2] = 1.0, v[2 * q] = 6.0, v[2 * q + 1] = 0.0;
        run_case("one_line", o, v, 0.1, 30);
        for (int q = 0; q < 30; ++q) v[2 * q] = 0.0, v[2 * q + 1] = -4.0;
        run_case("one_line_across", o, v, 0.1, 30);
    }
    run_case("velocity_zero", random_list(300, 200, 0, 0.2, 2), std::vector<double>(600, 0.0), 0.1, 30);
    run_case("velocity_null", random_list(300, 200, 0, 0.2, 2), {}, 0.1, 30);
    {
        std::vector<double> o = random_list(64, 100, 0, 0.2, 2), v(128);
        for (int q = 0; q < 64; ++q) v[2 * q] = (q & 1 ? 400.0 : -400.0), v[2 * q + 1] = (q & 2 ? 300.0 : -300.0);
        run_case("all_leave_the_entry_box", o, v, 0.1, 50);
    }
    run_case("all_dead", {0, 0, -5, 3, 3, -6, 9, 9, -100}, {1, 1, 2, 2, 3, 3}, 0.1, 10);
    run_case("negative_dt", random_list(50, 100, 0, 0.2, 2), random_vel(50, 8), -0.25, 20);
    run_case("many_ticks", random_list(20, 100, 0, 0.2, 2), random_vel(20, 8), 0.1, 2000);

    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = HUGE_VAL;
    refused("nan_velocity", {0, 0, 1, 5, 5, 1}, {0, nan, 0, 0}, 0.1, 5, kObsMotionNonFinite);
    refused("inf_velocity", {0, 0, 1, 5, 5, 1}, {0, 0, -inf, 0}, 0.1, 5, kObsMotionNonFinite);
    refused("nan_entry", {0, nan, 1}, {0, 0}, 0.1, 5, kObsMotionNonFinite);
    refused("extent_overflows", {0, 0, 1, 5, 5, 1}, {1e308, 0, -1e308, 0}, 10.0, 5, kObsMotionExtent);
    refused("product_overflows", {0, 0, 1}, {1e308, 0}, 1e10, 5, kObsMotionExtent);
    {
        // 40 000 obstacles of r = 200 over [0, 1000]^2: 44 x 44 cells each by the bound -- above 2^26
        std::vector<double> o = random_list(40000, 1000, 0, 200, 200);
        refused("bound_over_2_26", o, {}, 0.1, 5, kObsMotionPairs);
    }
    printf("%d failed\n", g_failed);
    return g_failed != 0;
}
