// The host schedule of agent lifetimes (contract U1-J), driven on the CPU: csrc/agent_life.h through a
// plain host program.  It checks the window predicate and the set-time rule at their edges, the sorted event list
// (deaths before boots on one tick, empty windows and the defaults without events) and the per-tick segments of a
// call: events on its first and last tick, none at or before t0 or beyond the call, and a random cross-check
// against the definition.  One "ok NAME" line per case, "N failed" last.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "agent_life.h"

using namespace swarm;

static int g_failed = 0;

static void check(const char *name, bool ok) {
    printf("%s %s\n", ok ? "ok" : "FAIL", name);
    g_failed += !ok;
}

int main() {
    const int64_t M = kAgentForever;
    // the window predicate
    check("up_edges", !agent_up(10, 20, 9) && agent_up(10, 20, 10) && agent_up(10, 20, 19) && !agent_up(10, 20, 20));
    check("up_defaults", agent_up(0, M, 0) && agent_up(0, M, M - 1) && !agent_up(0, M, M));
    check("up_empty_window", !agent_up(7, 7, 6) && !agent_up(7, 7, 7) && !agent_up(7, 7, 8) && !agent_up(9, 3, 5));
    // the set-time rule: down iff not up at T
    {
        bool ok = true;
        for (int64_t T = 0; T < 30; ++T) ok &= agent_down_when_set(10, 20, T) == !agent_up(10, 20, T);
        ok &= !agent_down_when_set(0, M, 0) && !agent_down_when_set(0, M, M - 1);
        ok &= agent_down_when_set(5, 5, 4) && agent_down_when_set(5, 5, 5) && agent_down_when_set(5, 5, 6);
        ok &= agent_down_when_set(11, M, 10) && !agent_down_when_set(10, M, 10) && agent_down_when_set(0, 10, 10) &&
              !agent_down_when_set(0, 11, 10);
        check("set_time_rule", ok);
    }
    // validity
    {
        int64_t bad = -1;
        const int64_t b1[] = {0, 5, kAgentBootMax - 1}, d1[] = {M, 3, 0};
        check("valid_windows", agent_life_check(3, b1, d1, &bad) == kAgentLifeOk && bad == -1);
        const int64_t b2[] = {0, -1, 2}, d2[] = {M, M, M};
        check("refuses_negative_boot", agent_life_check(3, b2, d2, &bad) == kAgentLifeBoot && bad == 1);
        const int64_t b3[] = {0, 1, kAgentBootMax}, d3[] = {M, M, M};
        check("refuses_boot_at_2_31", agent_life_check(3, b3, d3, &bad) == kAgentLifeBoot && bad == 2);
        const int64_t b4[] = {0}, d4[] = {-2};
        check("refuses_negative_death", agent_life_check(1, b4, d4, nullptr) == kAgentLifeDeath);
        check("valid_empty", agent_life_check(0, b4, d4, nullptr) == kAgentLifeOk);
    }
    // the event list
    {
        const int64_t boot[] = {0, 0, 0}, death[] = {M, M, M};
        const auto ev = agent_life_events(3, boot, death);
        check("defaults_have_no_events", ev.empty());
        const AgentSchedule s = agent_life_schedule(ev, 0, 100);
        check("empty_schedule", s.empty() && !s.has_events(0) && !s.has_events(99) && s.count(5) == 0 && s.deaths(5) == 0);
        check("empty_swarm", agent_life_events(0, boot, death).empty());
    }
    {
        // row 0 restarts at 5; row 1 dies at 5; row 2 boots at 5 and dies at 9; row 3: boot == death; row 4: boot after
        // death; row 5 boots at tick 0 (never an event) and dies at 7
        const int64_t boot[] = {5, 0, 5, 6, 9, 0}, death[] = {M, 5, 9, 6, 3, 7};
        const auto ev = agent_life_events(6, boot, death);
        bool ok = ev.size() == 5;
        const int64_t ticks[] = {5, 5, 5, 7, 9};
        const uint32_t entries[] = {agent_entry(1, kAgentDies), agent_entry(0, kAgentBoots), agent_entry(2, kAgentBoots),
                                    agent_entry(5, kAgentDies), agent_entry(2, kAgentDies)};
        for (size_t q = 0; ok && q < 5; ++q) ok = ev[q].tick == ticks[q] && ev[q].entry == entries[q];
        check("death_sorts_before_boot_on_one_tick", ok);
        bool none = true;
        for (const AgentEvent &e : ev) none &= agent_entry_row(e.entry) != 3 && agent_entry_row(e.entry) != 4;
        check("boot_equals_death_never_fires", none);
        check("entry_round_trip", agent_entry_row(agent_entry(0x7FFFFFFE, kAgentBoots)) == 0x7FFFFFFE &&
                                      agent_entry_kind(agent_entry(0x7FFFFFFE, kAgentBoots)) == kAgentBoots &&
                                      agent_entry_kind(agent_entry(3, kAgentDies)) == kAgentDies);
        // a call over ticks 5 .. 9: events on its first and on its last tick
        {
            const AgentSchedule s = agent_life_schedule(ev, 4, 5);
            check("events_at_first_and_last_tick", !s.empty() && s.first == 0 && s.count(0) == 3 && s.deaths(0) == 1 &&
                                                       !s.has_events(1) && s.count(2) == 1 && s.deaths(2) == 1 &&
                                                       !s.has_events(3) && s.count(4) == 1 && s.seg[5] == 5);
        }
        // a call that starts at tick 5: the events at 5 have fired (or were the set-time rule's) and do not fire again
        {
            const AgentSchedule s = agent_life_schedule(ev, 5, 2);
            check("events_at_or_before_t0_do_not_fire", !s.empty() && s.first == 3 && !s.has_events(0) && s.count(1) == 1 &&
                                                            s.seg[2] == 1);
        }
        // a call that ends at tick 8: the death at 9 is beyond it
        {
            const AgentSchedule s = agent_life_schedule(ev, 7, 1);
            check("events_beyond_the_call_do_not_fire", s.empty());
            const AgentSchedule u = agent_life_schedule(ev, 9, 50);
            check("a_call_after_every_event", u.empty());
            check("a_call_of_no_ticks", agent_life_schedule(ev, 0, 0).empty());
        }
        // chunks see every event once
        {
            size_t total = 0;
            for (int64_t t0 = 0; t0 < 12; t0 += 3) {
                const AgentSchedule s = agent_life_schedule(ev, t0, 3);
                total += s.empty() ? 0 : s.seg[3];
            }
            check("chunks_fire_every_event_once", total == ev.size());
        }
    }
    // next to INT64_MAX: no overflow in the call's last tick
    {
        const int64_t boot[] = {3}, death[] = {M - 1};
        const auto ev = agent_life_events(1, boot, death);
        const AgentSchedule s = agent_life_schedule(ev, M - 2, 1);
        check("near_max_death", ev.size() == 2 && !s.empty() && s.first == 1 && s.count(0) == 1 && s.deaths(0) == 1);
        check("near_max_no_overflow", agent_life_schedule(ev, M - 1, 5).empty());
    }
    // random windows against the definition
    {
        std::mt19937_64 rng(11);
        bool ok = true;
        for (int rep = 0; rep < 200 && ok; ++rep) {
            const int64_t n = int64_t(rng() % 50);
            std::vector<int64_t> boot(size_t(n) + 1), death(size_t(n) + 1);
            for (int64_t i = 0; i < n; ++i) {
                boot[size_t(i)] = rng() % 3 ? int64_t(rng() % 30) : 0;
                death[size_t(i)] = rng() % 3 ? int64_t(rng() % 40) : M;
            }
            const auto ev = agent_life_events(n, boot.data(), death.data());
            const int64_t t0 = int64_t(rng() % 20), ticks = 1 + int64_t(rng() % 25);
            const AgentSchedule s = agent_life_schedule(ev, t0, ticks);
            for (int64_t k = 0; k < ticks && ok; ++k) {
                const int64_t t = t0 + 1 + k;
                std::vector<uint32_t> want;
                for (int64_t i = 0; i < n; ++i)
                    if (boot[size_t(i)] < death[size_t(i)] && death[size_t(i)] == t) want.push_back(agent_entry(i, kAgentDies));
                const size_t nd = want.size();
                for (int64_t i = 0; i < n; ++i)
                    if (boot[size_t(i)] < death[size_t(i)] && boot[size_t(i)] == t) want.push_back(agent_entry(i, kAgentBoots));
                ok &= s.count(k) == want.size() && s.deaths(k) == nd && s.has_events(k) == !want.empty();
                for (size_t q = 0; ok && q < want.size(); ++q) ok = ev[s.first + s.seg[size_t(k)] + q].entry == want[q];
            }
        }
        check("segments_equal_the_definition_random", ok);
    }
    printf("%d failed\n", g_failed);
    return g_failed != 0;
}
