// The host schedule of task lifetimes (contract U1-A), driven on the CPU: csrc/task_life.h through a
// plain host program.  It checks the presence predicate at the edges of a window, the list of closing ticks and
// the retire rule, windows with open == close, ticks next to INT64_MAX (no overflow: the predicate compares, it
// never subtracts) and the validity checks.  One "ok NAME" line per case, "N failed" last.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "task_life.h"

using namespace swarm;

static int g_failed = 0;

static void check(const char *name, bool ok) {
    printf("%s %s\n", ok ? "ok" : "FAIL", name);
    g_failed += !ok;
}

int main() {
    const int64_t M = kLifeForever;
    // the edges of one window
    check("edge_before_open", !task_present(10, 20, 9));
    check("edge_at_open", task_present(10, 20, 10));
    check("edge_last_tick", task_present(10, 20, 19));
    check("edge_at_close", !task_present(10, 20, 20));
    check("edge_after_close", !task_present(10, 20, 21));
    check("open_equals_close_never_present", !task_present(7, 7, 6) && !task_present(7, 7, 7) && !task_present(7, 7, 8));
    check("zero_zero_never_present", !task_present(0, 0, 0));
    check("all_open_window", task_present(0, M, 0) && task_present(0, M, 1) && task_present(0, M, M - 1));
    // next to INT64_MAX
    check("forever_absent_at_max", !task_present(0, M, M));
    check("near_max_open", !task_present(M - 1, M, M - 2) && task_present(M - 1, M, M - 1));
    check("near_max_close", task_present(M - 3, M - 1, M - 2) && !task_present(M - 3, M - 1, M - 1));
    check("max_max_never_present", !task_present(M, M, M) && !task_present(M, M, M - 1));
    // the closing ticks and the retire rule
    {
        const int64_t open[] = {0, 5, 5, 9, 3, 0, M - 2}, close[] = {M, 9, 7, 9, 7, 0, M - 1};
        const std::vector<int64_t> c = task_close_ticks(7, close);
        const std::vector<int64_t> want = {0, 7, 9, M - 1};
        check("close_ticks_sorted_unique_without_forever", c == want);
        bool ok = true;
        for (int64_t t = 0; t < 12; ++t) ok &= task_tick_retires(c, false, t) == (t == 0 || t == 7 || t == 9);
        check("retire_ticks", ok);
        check("retire_near_max", task_tick_retires(c, false, M - 1) && !task_tick_retires(c, false, M - 2) &&
                                     !task_tick_retires(c, false, M));
        check("retire_when_fresh", task_tick_retires(c, true, 3) && task_tick_retires({}, true, 3));
        check("retire_never_without_closes", !task_tick_retires({}, false, 0) && !task_tick_retires({}, false, M));
        check("count_present", task_count_present(7, open, close, 6) == 4 && task_count_present(7, open, close, 8) == 2 &&
                                   task_count_present(7, open, close, 9) == 1 && task_count_present(0, open, close, 3) == 0);
        check("empty_board", task_close_ticks(0, close).empty());
    }
    // a retiring tick is exactly a tick at which some task stops being present (windows of at least one tick)
    {
        std::mt19937_64 rng(7);
        bool ok = true;
        for (int rep = 0; rep < 200; ++rep) {
            const int64_t T = int64_t(rng() % 40);
            std::vector<int64_t> open(size_t(T) + 1), close(size_t(T) + 1);
            for (int64_t k = 0; k < T; ++k) {
                open[size_t(k)] = int64_t(rng() % 50);
                close[size_t(k)] = rng() % 5 == 0 ? M : open[size_t(k)] + 1 + int64_t(rng() % 30);
            }
            const std::vector<int64_t> c = task_close_ticks(T, close.data());
            for (int64_t t = 1; t < 90; ++t) {
                bool stops = false;
                for (int64_t k = 0; k < T; ++k)
                    stops |= task_present(open[size_t(k)], close[size_t(k)], t - 1) &&
                             !task_present(open[size_t(k)], close[size_t(k)], t);
                ok &= stops == task_tick_retires(c, false, t);
            }
        }
        check("retire_iff_a_task_stops_being_present_random", ok);
    }
    // validity
    {
        int64_t bad = -1;
        const int64_t o1[] = {0, 4, 2}, c1[] = {M, 4, 9};
        check("valid_windows", task_life_check(3, o1, c1, &bad) == kTaskLifeOk && bad == -1);
        const int64_t o2[] = {0, 5, 2}, c2[] = {M, 4, 9};
        check("refuses_open_after_close", task_life_check(3, o2, c2, &bad) == kTaskLifeOrder && bad == 1);
        const int64_t o3[] = {0, 1, -1}, c3[] = {M, 4, 9};
        check("refuses_negative_open", task_life_check(3, o3, c3, &bad) == kTaskLifeNegative && bad == 2);
        const int64_t o4[] = {0}, c4[] = {INT64_MIN};
        check("refuses_negative_close", task_life_check(1, o4, c4, nullptr) == kTaskLifeNegative);
        check("valid_empty", task_life_check(0, o4, c4, nullptr) == kTaskLifeOk);
        const int64_t o5[] = {M}, c5[] = {M};
        check("valid_max_max", task_life_check(1, o5, c5, nullptr) == kTaskLifeOk);
    }
    printf("%d failed\n", g_failed);
    return g_failed != 0;
}
