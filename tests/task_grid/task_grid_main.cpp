// Drives csrc/task_grid.h on the host (tests/test_update_loop_board.py compiles and runs it): for every case the
// cell lists are checked -- every task in exactly one cell, the cell its own coordinates give, every list
// ascending -- and, for probe points on a lattice over and around the box, at random, at every cell border and
// one ulp either side of it, and outside the box by less and by more than 5, every task that passes the claim
// evaluation's far pre-test dx * dx + dy * dy <= 25 (brute force over the whole board) must be among the tasks
// the 3 x 3 window offers.  Prints one line per case and "N failed" at the end.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "task_grid.h"

using namespace swarm;

static int failed = 0;

static bool check_probe(const TaskCells &tc, const std::vector<double> &t, double px, double py, long *near) {
    std::vector<int32_t> offered;
    task_window(tc, px, py, &offered);
    std::set<int32_t> in(offered.begin(), offered.end());
    if (in.size() != offered.size()) return false;  // a task offered twice
    for (int64_t k = 0; k < tc.T; ++k) {
        const double dx = px - t[2 * k], dy = py - t[2 * k + 1];
        if (dx * dx + dy * dy <= 25.0) {
            ++*near;
            if (!in.count(int32_t(k))) return false;
        }
    }
    return true;
}

static void run_case(const std::string &name, const std::vector<double> &t) {
    const int64_t T = int64_t(t.size() / 2);
    TaskCells tc;
    const TaskCellsStatus st = build_task_cells(T, t.data(), &tc);
    if (st != kTaskCellsOk) {
        printf("ok %s refused status=%d lists_empty=%d\n", name.c_str(), int(st), int(tc.idx.empty() && tc.cell_off.empty()));
        return;
    }
    const Grid &g = tc.g;
    bool ok = int64_t(tc.cell_off.size()) == g.ncx * g.ncy + 1 && int64_t(tc.idx.size()) == T &&
              tc.cell_off.back() == uint32_t(T) && (T == 0 || g.cell >= kTaskCell) && g.ncx * g.ncy <= 4 * T + 1024;
    std::vector<int> seen(size_t(T), 0);
    for (int64_t c = 0; ok && c < g.ncx * g.ncy; ++c)
        for (uint32_t q = tc.cell_off[c]; q < tc.cell_off[c + 1]; ++q) {
            const int32_t k = tc.idx[q];
            ok = ok && k >= 0 && k < T && !seen[k]++ && (q == tc.cell_off[c] || tc.idx[q - 1] < k) &&
                 task_cell_coord(t[2 * k + 1], g.ymin, g.inv_cell, g.ncy) * g.ncx +
                         task_cell_coord(t[2 * k], g.xmin, g.inv_cell, g.ncx) == c;
        }
    long probes = 0, near = 0;
    auto probe = [&](double x, double y) {
        ++probes;
        if (!check_probe(tc, t, x, y, &near)) ok = false;
    };
    if (T) {
        std::mt19937_64 rng(7);
        const double w = g.xmax - g.xmin, h = g.ymax - g.ymin;
        std::uniform_real_distribution<double> ux(g.xmin - 8.0, g.xmax + 8.0), uy(g.ymin - 8.0, g.ymax + 8.0);
        for (int q = 0; q < 400; ++q) probe(ux(rng), uy(rng));
        for (int a = 0; a <= 12; ++a)
            for (int b = 0; b <= 12; ++b) probe(g.xmin - 6.5 + (w + 13.0) * a / 12.0, g.ymin - 6.5 + (h + 13.0) * b / 12.0);
        // around every task: the rim of its reach on both axes and the diagonals, one ulp either side
        for (int64_t k = 0; k < T && k < 64; ++k)
            for (int a = -1; a <= 1; ++a)
                for (int b = -1; b <= 1; ++b) {
                    const double s = a && b ? 5.0 * 0.7071067811865476 : 5.0;
                    const double x = t[2 * k] + a * s, y = t[2 * k + 1] + b * s;
                    probe(x, y);
                    probe(std::nextafter(x, 1e300), std::nextafter(y, -1e300));
                    probe(std::nextafter(x, -1e300), std::nextafter(y, 1e300));
                }
        // the cell borders (of the first 40 columns and rows), at and one ulp beside them
        for (int64_t cx = 0; cx <= g.ncx && cx < 40; ++cx)
            for (int64_t cy = 0; cy <= g.ncy && cy < 40; ++cy) {
                const double x = g.xmin + cx * g.cell, y = g.ymin + cy * g.cell;
                probe(x, y);
                probe(std::nextafter(x, -1e300), std::nextafter(y, -1e300));
                probe(std::nextafter(x, 1e300), std::nextafter(y, 1e300));
            }
        // outside the box on all eight sides: by less than 5, by 5, by more than 5 and far away
        for (double d : {0.5, 4.999, 5.0, 5.5, 6.5, 1.0e6})
            for (int a = -1; a <= 1; ++a)
                for (int b = -1; b <= 1; ++b)
                    if (a || b)
                        probe(a < 0 ? g.xmin - d : a > 0 ? g.xmax + d : g.xmin + 0.5 * w,
                              b < 0 ? g.ymin - d : b > 0 ? g.ymax + d : g.ymin + 0.5 * h);
        std::vector<int32_t> off;
        task_window(tc, g.xmax + 6.5, g.ymin, &off);
        ok = ok && off.empty();  // more than kTaskOutside beyond the box: nothing is offered
        task_window(tc, std::nan(""), g.ymin, &off);  // a NaN coordinate: cell 0 of that axis, no crash
    }
    if (!ok) ++failed;
    printf("%s %s T=%lld ncx=%lld ncy=%lld cell=%.17g longest=%lld probes=%ld near=%ld\n", ok ? "ok" : "FAILED",
           name.c_str(), (long long)T, (long long)g.ncx, (long long)g.ncy, g.cell, (long long)tc.longest, probes, near);
}

int main() {
    std::mt19937_64 rng(11);
    auto uniform = [&](int T, double x0, double x1, double y0, double y1) {
        std::uniform_real_distribution<double> ux(x0, x1), uy(y0, y1);
        std::vector<double> t;
        for (int k = 0; k < T; ++k) {
            t.push_back(ux(rng));
            t.push_back(uy(rng));
        }
        return t;
    };
    run_case("t0", {});
    run_case("one_task", {3.0, -2.0});
    {
        std::vector<double> t;
        for (int k = 0; k < 50; ++k) t.insert(t.end(), {7.25, 7.25});
        run_case("co_located", t);
    }
    {
        std::vector<double> t;
        for (int k = 0; k < 60; ++k) t.insert(t.end(), {1.7 * k, 4.0});
        run_case("one_line_x", t);
        for (size_t k = 0; k < t.size(); k += 2) std::swap(t[k], t[k + 1]);
        run_case("one_line_y", t);
    }
    {
        // tasks exactly on cell borders: x = xmin + c * cell as the grid itself computes it
        std::vector<double> t = {0.0, 0.0, 40.0, 40.0};
        for (int c = 1; c < 8; ++c) t.insert(t.end(), {c * kTaskCell, c * kTaskCell});
        for (int c = 1; c < 8; ++c) t.insert(t.end(), {std::nextafter(c * kTaskCell, 0.0), 20.0});
        run_case("on_cell_borders", t);
    }
    run_case("scattered_300", uniform(300, 0.0, 35.0, 0.0, 35.0));
    run_case("scattered_5000", uniform(5000, -182.5, 217.5, -182.5, 217.5));
    run_case("wide_cells_grown", uniform(40, -1.0e5, 1.0e5, -1.0e5, 1.0e5));  // 4 T + 1024 cells: the cells grow
    run_case("near_1e9", uniform(80, 1.0e9, 1.0e9 + 60.0, -1.0e9, -1.0e9 + 60.0));
    run_case("nan_x", {1.0, 2.0, std::nan(""), 0.0});
    run_case("inf_y", {1.0, HUGE_VAL});
    run_case("extent_overflows", {-1.0e308, 0.0, 1.0e308, 0.0});
    printf("%d failed\n", failed);
    return failed != 0;
}
