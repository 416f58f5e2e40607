// The host side of placing tasks into the slots of closed ones (contract U1-P), driven on the CPU:
// csrc/task_place.h through a plain host program, together with task_life.h's presence predicate (the quiet rule is
// "absent at ticks last and last - 1").  It checks the eligibility predicate at the edges, windows next to
// INT64_MAX (no overflow: it compares, it never subtracts), open == close, the per-request validity check and the
// request it names, duplicates, and the close-tick list update against a recomputation on random sequences.
// One "ok NAME" line per case, "N failed" last.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "task_life.h"
#include "task_place.h"

using namespace swarm;

static int g_failed = 0;

static void check(const char *name, bool ok) {
    printf("%s %s\n", ok ? "ok" : "FAIL", name);
    g_failed += !ok;
}

// The rule as the contract words it: absent at `last` and at `last - 1` (last >= 1 here, so last - 1 is a tick).
static bool quiet(int64_t open, int64_t close, int64_t last) {
    return !task_present(open, close, last) && !task_present(open, close, last - 1);
}

int main() {
    const int64_t M = kLifeForever;
    // a window [10, 20) against the last tick run: the close is heard at 20, its conflict at 21
    check("eligible_closed_at_last_minus_2", place_eligible(10, 20, 22));
    check("eligible_closed_at_last_minus_1", place_eligible(10, 20, 21));
    check("busy_closed_at_last", !place_eligible(10, 20, 20));
    check("busy_last_tick_of_the_window", !place_eligible(10, 20, 19));
    check("busy_open_at_last", !place_eligible(10, 20, 10));
    check("eligible_opens_after_last", place_eligible(10, 20, 9) && place_eligible(10, 20, 0));
    check("busy_one_tick_window_at_last", !place_eligible(7, 8, 7) && !place_eligible(7, 8, 8) && place_eligible(7, 8, 9));
    check("open_equals_close_always_eligible",
          place_eligible(7, 7, 6) && place_eligible(7, 7, 7) && place_eligible(7, 7, 8) && place_eligible(0, 0, 0) &&
              place_eligible(M, M, M) && place_eligible(M, M, 0));
    check("forever_is_never_eligible_once_open", !place_eligible(0, M, 0) && !place_eligible(0, M, M - 1) &&
                                                     !place_eligible(0, M, M) && place_eligible(5, M, 4));
    check("near_max_close", !place_eligible(M - 3, M - 1, M - 1) && place_eligible(M - 3, M - 1, M) &&
                                !place_eligible(M - 3, M - 1, M - 2));
    check("near_max_open", place_eligible(M, M, M - 1) && place_eligible(M - 1, M, M - 2) &&
                               !place_eligible(M - 1, M, M - 1));
    check("last_zero", place_eligible(1, 5, 0) && !place_eligible(0, 5, 0) && place_eligible(0, 0, 0));
    {  // the predicate is the contract's wording, on every small window and on windows next to INT64_MAX
        bool ok = true;
        for (int64_t o = 0; o < 12; ++o)
            for (int64_t c = o; c < 14; ++c)
                for (int64_t last = 1; last < 16; ++last) ok &= place_eligible(o, c, last) == quiet(o, c, last);
        for (int64_t o = M - 6; o > 0 && o <= M - 1; ++o)
            for (int64_t c = o; c > 0 && c <= M - 1; ++c)
                for (int64_t last = M - 7; last > 0 && last <= M - 1; ++last)
                    ok &= place_eligible(o, c, last) == quiet(o, c, last);
        check("eligible_iff_absent_at_last_and_the_tick_before", ok);
    }
    // one request: the first reason that applies, in the header's order
    {
        const int64_t T = 8, last = 30;
        auto one = [&](int64_t idx, int64_t oo, int64_t oc, double x, double vx, int req, int64_t o, int64_t c) {
            return place_check_one(T, last, idx, oo, oc, x, 1.0, vx, 0.0, req, o, c);
        };
        check("request_ok", one(3, 5, 29, 1.0, 0.0, -1, 31, 31) == kPlaceOk && one(0, 0, 0, 1.0, 0.0, 31, 40, M) == kPlaceOk &&
                                one(7, 31, 35, -2.0, 3.0, 0, M, M) == kPlaceOk);
        check("request_index", one(-1, 0, 0, 1.0, 0.0, 0, 31, 40) == kPlaceIndex && one(8, 0, 0, 1.0, 0.0, 0, 31, 40) == kPlaceIndex);
        check("request_busy", one(3, 5, 30, 1.0, 0.0, 0, 31, 40) == kPlaceBusy && one(3, 5, M, 1.0, 0.0, 0, 31, 40) == kPlaceBusy &&
                                  one(3, 30, 40, 1.0, 0.0, 0, 31, 40) == kPlaceBusy);
        check("request_negative", one(3, 0, 0, 1.0, 0.0, 0, -1, 40) == kPlaceNegative && one(3, 0, 0, 1.0, 0.0, 0, 31, -5) == kPlaceNegative);
        check("request_early", one(3, 0, 0, 1.0, 0.0, 0, 30, 40) == kPlaceEarly && one(3, 0, 0, 1.0, 0.0, 0, 0, 40) == kPlaceEarly);
        check("request_order", one(3, 0, 0, 1.0, 0.0, 0, 41, 40) == kPlaceOrder && one(3, 0, 0, 1.0, 0.0, 0, M, M - 1) == kPlaceOrder);
        check("request_non_finite", one(3, 0, 0, NAN, 0.0, 0, 31, 40) == kPlaceNonFinite && one(3, 0, 0, 1.0, INFINITY, 0, 31, 40) == kPlaceNonFinite &&
                                        one(3, 0, 0, -INFINITY, 0.0, 0, 31, 40) == kPlaceNonFinite);
        check("request_req", one(3, 0, 0, 1.0, 0.0, -2, 31, 40) == kPlaceReq && one(3, 0, 0, 1.0, 0.0, 32, 31, 40) == kPlaceReq);
    }
    {  // the list: the first bad request is named; NULL velocities are zero
        const int64_t T = 6, last = 9;
        const int32_t idx[] = {4, 1, 0, 5};
        const int64_t oo[] = {0, 2, 3, 0}, oc[] = {0, 8, 9, 0};  // the third slot closed at `last`: busy
        const double pos[] = {1, 1, 2, 2, 3, 3, 4, 4}, vel[] = {0, 0, 0, 0, 0, 0, NAN, 0};
        const int8_t req[] = {-1, 0, 1, 2};
        const int64_t o[] = {10, 12, 10, 10}, c[] = {10, M, 20, 11};
        int64_t bad = -7;
        check("list_names_the_first_bad_request", place_check(T, last, 4, idx, oo, oc, pos, vel, req, o, c, &bad) == kPlaceBusy && bad == 2);
        const int64_t oc2[] = {0, 8, 8, 0};
        bad = -7;
        check("list_then_the_next", place_check(T, last, 4, idx, oo, oc2, pos, vel, req, o, c, &bad) == kPlaceNonFinite && bad == 3);
        bad = -7;
        check("list_ok_with_null_velocities", place_check(T, last, 4, idx, oo, oc2, pos, nullptr, req, o, c, &bad) == kPlaceOk && bad == -7 &&
                                                  place_check(T, last, 4, idx, oo, oc2, pos, nullptr, req, o, c, nullptr) == kPlaceOk);
        check("list_empty", place_check(T, last, 0, idx, oo, oc, pos, vel, req, o, c, &bad) == kPlaceOk);
    }
    {  // duplicates
        const int32_t a[] = {5, 3, 9, 0}, b[] = {5, 3, 9, 3}, c[] = {2, 2}, d[] = {7, 1, 7, 1};
        int32_t dup = -1;
        check("no_duplicate", !place_has_duplicate(4, a, &dup) && dup == -1 && !place_has_duplicate(0, a, &dup) &&
                                  !place_has_duplicate(1, a, nullptr));
        check("duplicate_found", place_has_duplicate(4, b, &dup) && dup == 3 && place_has_duplicate(2, c, &dup) && dup == 2 &&
                                     place_has_duplicate(4, d, &dup) && dup == 1 && place_has_duplicate(4, b, nullptr));
    }
    {  // the close list by hand
        std::vector<int64_t> cl = {3, 7, 9, 15, M - 1};
        const int64_t add[] = {12, M, 9, 40, 12, 8};  // 8 <= last is no tick to come (a window [8, 8) placed early)
        place_update_closes(&cl, 8, 6, add);
        check("closes_by_hand", cl == std::vector<int64_t>({9, 12, 15, 40, M - 1}));
        std::vector<int64_t> none;
        place_update_closes(&none, 0, 0, add);
        check("closes_empty", none.empty());
        place_update_closes(&cl, M - 1, 0, add);
        check("closes_all_dropped", cl.empty());
    }
    {  // the close list on random sequences: after every place it is the recomputation's list -- every tick > last
       // that was in the list or is a new close -- and it covers every close tick to come of the board's windows
        std::mt19937_64 rng(11);
        bool ok = true, covers = true;
        for (int rep = 0; rep < 60; ++rep) {
            const int64_t T = 1 + int64_t(rng() % 24);
            std::vector<int64_t> open(size_t(T), 0), close(size_t(T), 0);
            std::vector<int64_t> cl = task_close_ticks(T, close.data());
            std::set<int64_t> model(cl.begin(), cl.end());
            int64_t last = 0;
            for (int step = 0; step < 40; ++step) {
                last += 1 + int64_t(rng() % 5);
                std::vector<int64_t> add;
                for (int64_t k = 0; k < T; ++k)
                    if (place_eligible(open[size_t(k)], close[size_t(k)], last) && rng() % 3 == 0) {
                        open[size_t(k)] = last + 1 + int64_t(rng() % 3);
                        close[size_t(k)] = rng() % 9 == 0 ? M : open[size_t(k)] + int64_t(rng() % 12);
                        add.push_back(close[size_t(k)]);
                    }
                place_update_closes(&cl, last, int64_t(add.size()), add.data());
                for (auto it = model.begin(); it != model.end();) it = *it <= last ? model.erase(it) : ++it;
                for (int64_t c : add)
                    if (c != M && c > last) model.insert(c);
                ok &= cl == std::vector<int64_t>(model.begin(), model.end());
                for (int64_t k = 0; k < T; ++k)
                    if (close[size_t(k)] != M && close[size_t(k)] > last && open[size_t(k)] != close[size_t(k)])
                        covers &= task_tick_retires(cl, false, close[size_t(k)]);
            }
        }
        check("closes_random_sequences_equal_the_recomputation", ok);
        check("closes_cover_every_close_to_come", covers);
    }
    check("reasons_have_text", place_reason(kPlaceBusy)[0] != 0 && place_reason(kPlaceReq)[0] != 0);
    printf("%d failed\n", g_failed);
    return g_failed != 0;
}
