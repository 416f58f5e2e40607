// Drives csrc/obstacle_cells.h on the host (no HIP): the cell lists of an obstacle field (contract O1) must be
// ascending without duplicates, hold exactly the footprints' cell ranges, and for every probe position hold
// every obstacle that passes the flat obstacle loop's pre-test there.  Built and run by
// tests/test_obstacle_cells.py (g++ -I<csrc>); prints one line per case, exit status = failed cases.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "obstacle_cells.h"

using namespace swarm;

static int failed = 0;

static void fail(const std::string &name, const std::string &what) {
    std::printf("FAIL %s: %s\n", name.c_str(), what.c_str());
    ++failed;
}

// a small generator of its own, so that the cases are the same everywhere
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uni() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return double(rng_state >> 11) * 0x1p-53;
}
static double uni(double a, double b) { return a + (b - a) * uni(); }

typedef std::vector<double> Obs;
static void add(Obs &o, double x, double y, double r) {
    o.push_back(x), o.push_back(y), o.push_back(r);
}
static Obs scatter(int64_t m, double lo, double hi, double r0, double r1, double shift = 0.0) {
    Obs o;
    for (int64_t k = 0; k < m; ++k) add(o, shift + uni(lo, hi), shift + uni(lo, hi), uni(r0, r1));
    return o;
}

// the flat loop's pre-test (physics.hip obstacle_forces), its own expressions: true = not skipped
static bool passes_pretest(const double *o, double px, double py) {
    const double ex = px - o[0], ey = py - o[1];
    const double s2 = ex * ex + ey * ey;
    const double rr = 5.0 + o[2];
    return !(s2 > rr * rr * (1.0 + 1e-12));
}
// ... and whether the loop then applies a term
static bool applies_term(const double *o, double px, double py) {
    const double ex = px - o[0], ey = py - o[1];
    double d = std::sqrt(ex * ex + ey * ey) - o[2];
    if (d <= 0.001) d = 0.001;
    return d < 5.0;
}

struct Probes {
    std::vector<double> x, y;
    void at(double px, double py) { x.push_back(px), y.push_back(py); }
};

static void three(std::vector<double> &v, double c) {
    v.push_back(std::nextafter(c, -HUGE_VAL)), v.push_back(c), v.push_back(std::nextafter(c, HUGE_VAL));
}

// a lattice, random probes, every cell boundary and one ulp either side (at most 48 boundaries an axis, spread
// evenly, the first and the last always), outside the box on all eight sides and 1e6 away, and around the first
// 64 live obstacles at the rim of their reach (where the pre-test turns), on the axes and the diagonals
static Probes make_probes(const ObsCells &oc, const Obs &obs) {
    const Grid &g = oc.g;
    const double x0 = g.xmin, y0 = g.ymin, x1 = x0 + double(g.ncx) * g.cell, y1 = y0 + double(g.ncy) * g.cell;
    const double wx = x1 - x0, wy = y1 - y0;
    Probes p;
    for (int a = 0; a <= 32; ++a)
        for (int b = 0; b <= 32; ++b) p.at(x0 - 0.1 * wx + 1.2 * wx * a / 32.0, y0 - 0.1 * wy + 1.2 * wy * b / 32.0);
    for (int k = 0; k < 3000; ++k) p.at(uni(x0 - 8, x1 + 8), uni(y0 - 8, y1 + 8));
    std::vector<double> bx, by;
    const int64_t sx = std::max<int64_t>(1, g.ncx / 47), sy = std::max<int64_t>(1, g.ncy / 47);
    for (int64_t k = 0; k < g.ncx; k += sx) three(bx, x0 + double(k) * g.cell);
    for (int64_t k = 0; k < g.ncy; k += sy) three(by, y0 + double(k) * g.cell);
    three(bx, x1), three(by, y1);
    for (double x : bx) {
        for (double y : by) p.at(x, y);
        for (int k = 0; k < 6; ++k) p.at(x, uni(y0, y1));
    }
    for (double y : by)
        for (int k = 0; k < 6; ++k) p.at(uni(x0, x1), y);
    int seen = 0;
    for (size_t o = 0; 3 * o < obs.size() && seen < 64; ++o) {
        const double rr = 5.0 + obs[3 * o + 2];
        if (!(rr > 0)) continue;
        ++seen;
        const double rim[] = {rr * (1.0 - 1e-13), rr, rr * (1.0 + 4e-13), rr * (1.0 + 1e-11)};
        for (double d : rim)
            for (int a = -1; a <= 1; ++a)
                for (int b = -1; b <= 1; ++b) {
                    if (!a && !b) continue;
                    const double s = (a && b) ? d * 0.70710678118654752 : d;
                    p.at(obs[3 * o] + a * s, obs[3 * o + 1] + b * s);
                }
        p.at(obs[3 * o], obs[3 * o + 1]);
    }
    const double far[] = {1.0, 1e6};
    const double g_xmax = g.xmax, g_ymax = g.ymax;
    for (double d : far)
        for (int sxn = -1; sxn <= 1; ++sxn)
            for (int syn = -1; syn <= 1; ++syn) {
                if (!sxn && !syn) continue;
                const double mx = 0.5 * (x0 + g_xmax), my = 0.5 * (y0 + g_ymax);
                p.at(sxn < 0 ? x0 - d : sxn > 0 ? g_xmax + d : mx, syn < 0 ? y0 - d : syn > 0 ? g_ymax + d : my);
                // just outside: still within reach of an obstacle at the rim
                if (d == 1.0)
                    p.at(sxn < 0 ? std::nextafter(x0, -HUGE_VAL) : sxn > 0 ? std::nextafter(g_xmax, HUGE_VAL) : mx,
                         syn < 0 ? std::nextafter(y0, -HUGE_VAL) : syn > 0 ? std::nextafter(g_ymax, HUGE_VAL) : my);
            }
    return p;
}

static void accepted(const std::string &name, const Obs &obs, int64_t want_live = -1) {
    const int64_t m = int64_t(obs.size() / 3);
    ObsCells oc;
    const ObsCellsStatus st = build_obstacle_cells(m, obs.data(), &oc);
    if (st != kObsCellsOk) return fail(name, "refused with status " + std::to_string(int(st)));
    const Grid &g = oc.g;
    const int64_t cells = g.ncx * g.ncy;
    if (want_live >= 0 && oc.live != want_live) return fail(name, "live = " + std::to_string(oc.live));
    if (g.ncx < 1 || g.ncy < 1 || cells > 4 * oc.live + 1024) return fail(name, "grid shape");
    if (int64_t(oc.cell_off.size()) != cells + 1 || oc.cell_off[0] != 0) return fail(name, "cell_off size");
    if (int64_t(oc.idx.size()) != oc.pairs || int64_t(oc.cell_off[cells]) != oc.pairs) return fail(name, "pairs");
    // every list ascending, no duplicates, indices of live obstacles
    int64_t longest = 0;
    for (int64_t c = 0; c < cells; ++c) {
        if (oc.cell_off[c] > oc.cell_off[c + 1]) return fail(name, "cell_off not monotone");
        longest = std::max<int64_t>(longest, oc.cell_off[c + 1] - oc.cell_off[c]);
        for (uint32_t q = oc.cell_off[c]; q < oc.cell_off[c + 1]; ++q) {
            if (oc.idx[q] < 0 || oc.idx[q] >= m) return fail(name, "index out of range");
            if (!(5.0 + obs[3 * size_t(oc.idx[q]) + 2] > 0)) return fail(name, "a dead obstacle is listed");
            if (q > oc.cell_off[c] && oc.idx[q] <= oc.idx[q - 1]) return fail(name, "a list is not ascending");
        }
    }
    if (longest != oc.longest) return fail(name, "longest");
    // the pair count is the sum of the footprints' cell ranges, and each footprint cell lists its obstacle
    int64_t want_pairs = 0, live = 0;
    for (int64_t o = 0; o < m; ++o) {
        const double r = obs[3 * o + 2], rr = 5.0 + r;
        if (!(rr > 0)) continue;
        ++live;
        const double h = rr * (1.0 + 1e-9);
        const int64_t cx0 = obs_cell_coord(obs[3 * o] - h, g.xmin, g.inv_cell, g.ncx);
        const int64_t cx1 = obs_cell_coord(obs[3 * o] + h, g.xmin, g.inv_cell, g.ncx);
        const int64_t cy0 = obs_cell_coord(obs[3 * o + 1] - h, g.ymin, g.inv_cell, g.ncy);
        const int64_t cy1 = obs_cell_coord(obs[3 * o + 1] + h, g.ymin, g.inv_cell, g.ncy);
        if (cx1 < cx0 || cy1 < cy0) return fail(name, "an empty footprint");
        want_pairs += (cx1 - cx0 + 1) * (cy1 - cy0 + 1);
    }
    if (live != oc.live) return fail(name, "live count");
    if (want_pairs != oc.pairs) return fail(name, "pairs != sum of the footprints' cell ranges");
    // covering: every obstacle that passes the flat pre-test at a probe is in the list of the probe's cell.  (A
    // dead obstacle, r <= -5, passes the pre-test within |5 + r| of its centre and is in no list by the
    // footprint rule: for it the flat loop's own d < 5.0 must be false, so that it adds no term either way.)
    const Probes p = make_probes(oc, obs);
    int64_t hits = 0;
    for (size_t k = 0; k < p.x.size(); ++k) {
        const int64_t c = obs_cell_coord(p.y[k], g.ymin, g.inv_cell, g.ncy) * g.ncx +
                          obs_cell_coord(p.x[k], g.xmin, g.inv_cell, g.ncx);
        const int32_t *b = oc.idx.data() + oc.cell_off[c], *e = oc.idx.data() + oc.cell_off[c + 1];
        for (int64_t o = 0; o < m; ++o) {
            if (!passes_pretest(obs.data() + 3 * o, p.x[k], p.y[k])) continue;
            if (!(5.0 + obs[3 * o + 2] > 0)) {
                if (applies_term(obs.data() + 3 * o, p.x[k], p.y[k])) return fail(name, "a dead obstacle acts");
                continue;
            }
            ++hits;
            if (!std::binary_search(b, e, int32_t(o))) {
                char what[200];
                std::snprintf(what, sizeof(what), "obstacle %lld (%.17g, %.17g, %.17g) missing at probe (%.17g, %.17g)",
                              (long long)o, obs[3 * o], obs[3 * o + 1], obs[3 * o + 2], p.x[k], p.y[k]);
                return fail(name, what);
            }
        }
    }
    std::printf("ok %s m=%lld live=%lld ncx=%lld ncy=%lld cell=%.17g pairs=%lld longest=%lld probes=%zu hits=%lld\n",
                name.c_str(), (long long)m, (long long)oc.live, (long long)g.ncx, (long long)g.ncy, g.cell,
                (long long)oc.pairs, (long long)oc.longest, p.x.size(), (long long)hits);
}

static bool holds_nothing(const ObsCells &oc) {
    return oc.cell_off.capacity() == 0 && oc.idx.capacity() == 0 && oc.pairs == 0;
}

static void refused(const std::string &name, const Obs &obs, ObsCellsStatus want) {
    ObsCells oc;
    oc.idx.assign(3, 1);  // a refusal leaves no list behind, whatever was there
    const ObsCellsStatus st = build_obstacle_cells(int64_t(obs.size() / 3), obs.data(), &oc);
    if (st != want) return fail(name, "status " + std::to_string(int(st)) + ", want " + std::to_string(int(want)));
    if (!holds_nothing(oc)) return fail(name, "a refusal left a list");
    std::printf("ok %s refused status=%d\n", name.c_str(), int(st));
}

int main() {
    // sizes
    accepted("m0", Obs{}, 0);
    {
        Obs o;
        add(o, 3.0, 4.0, 1.0);
        accepted("m1", o, 1);
    }
    accepted("m7", scatter(7, -10, 50, 0.2, 2), 7);
    accepted("m1025", scatter(1025, -10, 50, 0.2, 2), 1025);
    // radii: zero, negative, exactly dead, dead
    {
        Obs o = scatter(12, 0, 40, 0.2, 2);
        add(o, 10, 10, 0.0), add(o, 20, 12, -1.0), add(o, 30, 14, -5.0), add(o, 16, 30, -7.0);
        add(o, 22, 22, std::nextafter(-5.0, 0.0));  // the smallest live footprint
        accepted("radii", o, 15);
    }
    {
        Obs o;
        add(o, 1, 2, -5.0), add(o, 3, 4, -7.0), add(o, -2, 0, -1e6);
        accepted("all_dead", o, 0);
    }
    {
        Obs o = scatter(40, 0, 60, 0.2, 2);
        add(o, 31.0, 29.0, 300.0);
        accepted("r300_among_small", o, 41);
    }
    {
        Obs o = scatter(20, 0, 30, 0.2, 2);
        for (int k = 0; k < 5; ++k) add(o, 12.5, 7.25, 1.5);
        for (int k = 0; k < 3; ++k) add(o, o[0], o[1], o[2]);
        accepted("duplicates", o, 28);
    }
    {
        Obs h, v, pt;
        for (int k = 0; k < 30; ++k) add(h, 3.0 * k, 7.0, 0.5 + 0.05 * k), add(v, -4.0, 2.5 * k, 1.0);
        for (int k = 0; k < 9; ++k) add(pt, 5.0, 5.0, 1.0);
        accepted("one_line_x", h, 30);
        accepted("one_line_y", v, 30);
        accepted("one_point", pt, 9);
    }
    accepted("near_1e9", scatter(50, -10, 50, 0.2, 2, 1e9), 50);
    accepted("near_minus_1e9", scatter(50, -10, 50, 0.2, 2, -1e9), 50);
    {
        Obs o = scatter(30, 0, 40, 0.2, 2);
        add(o, 1e7, -1e7, 1.0);  // one far outlier: sparse cells
        accepted("outlier", o, 31);
    }
    // refusals
    {
        Obs o = scatter(9, 0, 40, 0.2, 2);
        Obs a = o, b = o, c = o, d = o;
        a[3 * 4] = std::nan(""), b[3 * 2 + 1] = HUGE_VAL, c[3 * 7 + 2] = -HUGE_VAL, d[3 * 8 + 2] = std::nan("");
        refused("nan_x", a, kObsCellsNonFinite);
        refused("inf_y", b, kObsCellsNonFinite);
        refused("minus_inf_r", c, kObsCellsNonFinite);  // dead, and refused all the same
        refused("nan_r", d, kObsCellsNonFinite);
    }
    {
        Obs o;
        add(o, -1e308, 0, 1), add(o, 1e308, 0, 1);
        refused("extent_overflows_x", o, kObsCellsExtent);
        Obs q;
        add(q, 0, -1.7e308, 1), add(q, 0, 1.7e308, 1e300);
        refused("extent_overflows_y", q, kObsCellsExtent);
    }
    {
        // more than 2^26 pairs: 200 000 small obstacles over an arena of 1 400, 224 of them with r = 1e6 -- the
        // cell cap makes ~890 x 890 cells over the huge ones' box, and each huge one reaches them all
        Obs o = scatter(200000, 0, 1400, 0.2, 2);
        for (int k = 0; k < 224; ++k) o[3 * size_t(k * 890) + 2] = 1e6;
        refused("too_many_pairs", o, kObsCellsPairs);
    }
    {
        // 70 000 obstacles that all reach every cell: refused by the count (judged by the test itself)
        const Obs o = scatter(70000, 0, 1400, 1e6, 1e6);
        ObsCells oc;
        const ObsCellsStatus st = build_obstacle_cells(70000, o.data(), &oc);
        std::printf("case huge_70000 status=%d lists_empty=%d ncx=%lld ncy=%lld pairs=%lld\n", int(st),
                    int(oc.cell_off.capacity() == 0 && oc.idx.capacity() == 0), (long long)oc.g.ncx,
                    (long long)oc.g.ncy, (long long)oc.pairs);
    }
    std::printf("%d failed\n", failed);
    return failed;
}
