// The host arithmetic of moving task boards (contract U1-M), driven on the CPU: csrc/task_motion.h
// through a plain host program (g++ -ffp-contract=off, the library's flag).  For every accepted case the program
// iterates the contract's advance exactly, tick by tick, and checks that
//   - every position Q_k, k = 0 .. ticks, of every task lies inside its per-axis span, inside the box of all
//     spans and inside the call's grid's box (a result bit rests on it: task_window_empty skips by that box);
//   - the advance is the two separately rounded operations of the contract, bit for bit;
//   - the call's grid has at most 4 T + 1024 cells of side at least kTaskCell.
// Refusals (a non-finite velocity, a span that overflows, a box with no finite extent) are checked to come back
// with the grid untouched.
//
// With arguments `box FILE`: FILE holds T (int64), ticks (int64), dt (double), then T x 2 positions and T x 2
// velocities; the program prints task_span_box's four doubles as hex floats (a GPU test compares the device's
// reduction with them).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "task_motion.h"

using namespace swarm;

static int g_failed = 0;

static void fail(const char *name, const char *what, long long a = 0, long long b = 0) {
    printf("FAIL %s: %s (%lld, %lld)\n", name, what, a, b);
    ++g_failed;
}

static uint64_t bits(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

// the contract's advance restated with volatile temporaries: no contraction whatever the flags
static double advance_ref(double x, double v, double dt) {
    volatile double d = v * dt;
    volatile double r = x + d;
    return r;
}

static void run_case(const char *name, std::vector<double> pos, const std::vector<double> &vel, double dt, int32_t ticks) {
    const int64_t T = int64_t(pos.size() / 2);
    const double *v = vel.empty() ? nullptr : vel.data();
    Grid g{};
    const TaskMotionStatus st = task_call_grid(T, pos.data(), v, dt, ticks, &g);
    if (st != kTaskMotionOk) return fail(name, "refused", st);
    if (g.ncx * g.ncy > 4 * T + 1024 || g.ncx < 1 || g.ncy < 1 || !(g.cell >= kTaskCell || T == 0))
        return fail(name, "the grid's shape", g.ncx, g.ncy);
    const TaskBox box = task_span_box(T, pos.data(), v, dt, ticks);
    std::vector<double> lo(size_t(T) * 2), hi(size_t(T) * 2);
    for (int64_t q = 0; q < 2 * T; ++q) task_axis_span(pos[q], v ? v[q] : 0.0, dt, ticks, &lo[q], &hi[q]);
    int64_t left_entry = 0;
    Grid entry{};
    task_static_grid(T, pos.data(), &entry);
    for (int32_t k = 0; k <= ticks; ++k) {
        for (int64_t t = 0; t < T; ++t) {
            const double x = pos[2 * t], y = pos[2 * t + 1];
            if (!(x >= lo[2 * t] && x <= hi[2 * t] && y >= lo[2 * t + 1] && y <= hi[2 * t + 1]))
                return fail(name, "a task left its span at tick", k, t);
            if (!(x >= box.xmin && x <= box.xmax && y >= box.ymin && y <= box.ymax))
                return fail(name, "a task left the box at tick", k, t);
            if (!(x >= g.xmin && x <= g.xmax && y >= g.ymin && y <= g.ymax))
                return fail(name, "a task left the call's grid's box at tick", k, t);
            if (task_window_empty(g, x, y)) return fail(name, "the window of a task's own position is empty", k, t);
            if (k == ticks && !(x >= entry.xmin && x <= entry.xmax && y >= entry.ymin && y <= entry.ymax)) ++left_entry;
        }
        if (k < ticks)
            for (int64_t q = 0; q < 2 * T; ++q) {
                const double nx = task_advance(pos[q], v ? v[q] : 0.0, dt);
                if (bits(nx) != bits(advance_ref(pos[q], v ? v[q] : 0.0, dt))) return fail(name, "the advance's bits", k, q);
                pos[q] = nx;
            }
    }
    printf("ok %s T=%lld ticks=%d ncx=%lld ncy=%lld cell=%.17g left_entry_box=%lld\n", name, (long long)T, int(ticks),
           (long long)g.ncx, (long long)g.ncy, g.cell, (long long)left_entry);
}

static void refused(const char *name, const std::vector<double> &pos, const std::vector<double> &vel, double dt,
                    int32_t ticks, TaskMotionStatus want) {
    Grid g{};
    g.ncx = -7;
    const TaskMotionStatus st =
        task_call_grid(int64_t(pos.size() / 2), pos.data(), vel.empty() ? nullptr : vel.data(), dt, ticks, &g);
    if (st != want) return fail(name, "wrong status", st, want);
    if (g.ncx != -7) return fail(name, "a refused call wrote its grid", g.ncx);
    printf("ok %s refused status=%d\n", name, int(st));
}

static int print_box(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    int64_t hdr[2];
    double dt;
    if (fread(hdr, 8, 2, f) != 2 || fread(&dt, 8, 1, f) != 1) return 2;
    const size_t T = size_t(hdr[0]);
    std::vector<double> pos(T * 2), vel(T * 2);
    if (fread(pos.data(), 8, T * 2, f) != T * 2 || fread(vel.data(), 8, T * 2, f) != T * 2) return 2;
    fclose(f);
    const TaskBox b = task_span_box(int64_t(T), pos.data(), vel.data(), dt, int32_t(hdr[1]));
    printf("%a %a %a %a\n", b.xmin, b.ymin, b.xmax, b.ymax);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "box")) return print_box(argv[2]);
    std::mt19937_64 rng(20261);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    auto random_pos = [&](int64_t T, double span, double shift) {
        std::vector<double> p(size_t(T) * 2);
        for (double &x : p) x = shift + uni(0, span);
        return p;
    };
    auto random_vel = [&](int64_t T, double vmax) {
        std::vector<double> v(size_t(T) * 2);
        for (double &x : v) x = uni(-vmax, vmax);
        return v;
    };
    run_case("random_300", random_pos(300, 200, 0), random_vel(300, 3), 0.1, 120);
    run_case("random_5000", random_pos(5000, 600, -300), random_vel(5000, 8), 0.1, 40);
    run_case("t1", random_pos(1, 1, 0), random_vel(1, 3), 0.1, 30);
    run_case("t0", {}, {}, 0.1, 10);
    run_case("velocity_null", random_pos(300, 200, 0), {}, 0.1, 30);
    run_case("velocity_zero", random_pos(300, 200, 0), std::vector<double>(600, 0.0), 0.1, 30);
    run_case("negative_dt", random_pos(50, 100, 0), random_vel(50, 8), -0.25, 20);
    run_case("ticks_1", random_pos(200, 100, 0), random_vel(200, 50), 0.1, 1);
    run_case("ticks_0", random_pos(200, 100, 0), random_vel(200, 50), 0.1, 0);
    // adversarial: |x| = 1e9 with steps of every size against it, both signs of x and of v
    {
        std::vector<double> p, v;
        const double steps[] = {1e-9, 5.9e-8, 1.2e-7, 1e-7, 3e-7, 1e-3, 0.3, 7.0};  // ulp(1e9) = 1.19e-7
        for (double sx : {1e9, -1e9})
            for (double d : steps)
                for (double sv : {1.0, -1.0}) {
                    p.push_back(sx), p.push_back(-sx);
                    v.push_back(sv * d * 10.0), v.push_back(-sv * d * 10.0);
                }
        run_case("near_1e9_ticks_1", p, v, 0.1, 1);
        run_case("near_1e9_ticks_1000", p, v, 0.1, 1000);
        run_case("near_1e9_ticks_1e6", p, v, 0.1, 1000000);
    }
    // opposite signs: tasks that cross zero, and pairs that fly apart
    {
        std::vector<double> p, v;
        for (int q = 0; q < 16; ++q) {
            p.push_back(q & 1 ? 3.0 : -3.0), p.push_back(q & 2 ? 1e-300 : -1e-300);
            v.push_back(q & 1 ? -uni(0, 9) : uni(0, 9)), v.push_back(q & 4 ? 400.0 : -400.0);
        }
        run_case("opposite_signs", p, v, 0.1, 500);
        run_case("opposite_signs_ticks_1e6", p, v, 0.1, 1000000);
    }
    for (int rep = 0; rep < 40; ++rep) {  // random draws of every scale
        const double shift = std::ldexp(uni(-1, 1), int(uni(-20, 40))), vmax = std::ldexp(1.0, int(uni(-30, 20)));
        char name[64];
        snprintf(name, sizeof name, "scales_%d", rep);
        run_case(name, random_pos(40, std::ldexp(1.0, int(uni(-10, 20))), shift), random_vel(40, vmax), 0.1,
                 int32_t(uni(1, 3000)));
    }
    {
        std::vector<double> p = random_pos(64, 100, 0), v(128);
        for (int q = 0; q < 64; ++q) v[2 * q] = (q & 1 ? 400.0 : -400.0), v[2 * q + 1] = (q & 2 ? 300.0 : -300.0);
        run_case("all_leave_the_entry_box", p, v, 0.1, 50);
    }

    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = HUGE_VAL;
    refused("nan_velocity", {0, 0, 5, 5}, {0, nan, 0, 0}, 0.1, 5, kTaskMotionNonFinite);
    refused("inf_velocity", {0, 0, 5, 5}, {0, 0, -inf, 0}, 0.1, 5, kTaskMotionNonFinite);
    refused("nan_position", {0, nan}, {0, 0}, 0.1, 5, kTaskMotionNonFinite);
    refused("extent_overflows", {0, 0, 5, 5}, {1e307, 0, -1e307, 0}, 10.0, 5, kTaskMotionExtent);
    refused("span_overflows", {0, 0}, {1e308, 0}, 1e10, 5, kTaskMotionExtent);
    refused("static_extent_overflows", {-1e308, 0, 1e308, 0}, {}, 0.1, 5, kTaskMotionExtent);
    printf("%d failed\n", g_failed);
    return g_failed != 0;
}
