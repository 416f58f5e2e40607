// Agent lifetimes (contract U1-J): the host schedule of a swarm whose agents boot and die during a
// run.  Pure arithmetic, no HIP includes, so that a plain host program can drive it (tests/agent_life/
// agent_life_main.cpp); agent_life.hip owns the handle and the event kernel.
//
// Agent i carries one window [boot[i], death[i]) of absolute ticks and is up at tick t iff boot[i] <= t < death[i]:
// two comparisons, no subtraction, so ticks up to INT64_MAX cannot overflow.  The defaults boot = 0 and
// death = kAgentForever mean "as it is, forever" and schedule nothing.  An agent whose window is empty
// (boot >= death) is never up and has no events.  At the start of tick t the agents with death == t die, then the
// agents with boot == t boot (a boot of an agent that is up is a restart).  Tick 0 is never run, so an event
// at tick 0 never fires; the set-time rule covers it.  The events of all agents are sorted once, when the windows
// are set: (tick, deaths before boots, row).  A call over the ticks t0+1 .. t0+ticks then finds its events by two
// binary searches and its per-tick segments in one pass over those events alone.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#ifndef SWARM_HD  // (the event kernel decodes the entries with the functions below)
#if defined(__HIPCC__)
#define SWARM_HD __host__ __device__
#else
#define SWARM_HD
#endif
#endif

namespace swarm {

constexpr int64_t kAgentForever = INT64_MAX;
constexpr int64_t kAgentBootMax = int64_t(1) << 31;  // a boot tick is 0 (the default) .. 2^31 - 1: tick_off = 1 - boot

enum AgentEventKind : uint32_t { kAgentDies = 0, kAgentBoots = 1 };

static inline bool agent_up(int64_t boot, int64_t death, int64_t t) { return boot <= t && t < death; }

// The set-time rule: with T the last tick run, an agent that is not up at T loses its alive flag; the others keep
// the flag they have.
static inline bool agent_down_when_set(int64_t boot, int64_t death, int64_t T) { return boot > T || death <= T; }

enum AgentLifeStatus {
    kAgentLifeOk = 0,
    kAgentLifeBoot,   // a boot tick outside [0, 2^31)
    kAgentLifeDeath,  // a death tick below zero
};

// The validity of n windows; *bad (may be NULL) is the first row refused.
static inline AgentLifeStatus agent_life_check(int64_t n, const int64_t *boot, const int64_t *death, int64_t *bad) {
    for (int64_t i = 0; i < n; ++i) {
        const AgentLifeStatus st = boot[i] < 0 || boot[i] >= kAgentBootMax ? kAgentLifeBoot
                                   : death[i] < 0                          ? kAgentLifeDeath
                                                                           : kAgentLifeOk;
        if (st != kAgentLifeOk) {
            if (bad) *bad = i;
            return st;
        }
    }
    return kAgentLifeOk;
}

struct AgentEvent {
    int64_t tick;
    uint32_t entry;  // the agent's storage row, bit 31: the kind (n < 2^31)
};

static inline uint32_t agent_entry(int64_t row, AgentEventKind kind) { return uint32_t(row) | (uint32_t(kind) << 31); }
SWARM_HD static inline int64_t agent_entry_row(uint32_t e) { return int64_t(e & 0x7FFFFFFFu); }
SWARM_HD static inline AgentEventKind agent_entry_kind(uint32_t e) { return AgentEventKind(e >> 31); }

// Every event of the n windows, sorted by (tick, kind, row): deaths before boots on one tick.
static inline std::vector<AgentEvent> agent_life_events(int64_t n, const int64_t *boot, const int64_t *death) {
    std::vector<AgentEvent> ev;
    for (int64_t i = 0; i < n; ++i) {
        if (boot[i] >= death[i]) continue;  // never up: no events
        if (boot[i] > 0) ev.push_back({boot[i], agent_entry(i, kAgentBoots)});
        if (death[i] != kAgentForever) ev.push_back({death[i], agent_entry(i, kAgentDies)});  // (death > boot >= 0)
    }
    std::sort(ev.begin(), ev.end(), [](const AgentEvent &a, const AgentEvent &b) {
        if (a.tick != b.tick) return a.tick < b.tick;
        const uint32_t ka = a.entry >> 31, kb = b.entry >> 31;
        if (ka != kb) return ka < kb;
        return a.entry < b.entry;
    });
    return ev;
}

// The events of one call: [first, first + seg[ticks]) of the sorted list, tick t0 + 1 + k owning the entries
// [first + seg[k], first + seg[k + 1]), its deaths first (died[k] of them).
struct AgentSchedule {
    size_t first = 0;
    std::vector<uint32_t> seg;   // ticks + 1 offsets; empty when the call has no event
    std::vector<uint32_t> died;  // per tick, the deaths among its events
    bool empty() const { return seg.empty(); }
    bool has_events(int64_t k) const { return !seg.empty() && seg[size_t(k) + 1] > seg[size_t(k)]; }
    uint32_t count(int64_t k) const { return seg.empty() ? 0u : seg[size_t(k) + 1] - seg[size_t(k)]; }
    uint32_t deaths(int64_t k) const { return seg.empty() ? 0u : died[size_t(k)]; }
};

static inline AgentSchedule agent_life_schedule(const std::vector<AgentEvent> &ev, int64_t t0, int64_t ticks) {
    AgentSchedule s;
    if (ticks <= 0 || ev.empty()) return s;
    // the last tick of the call, without overflow
    const int64_t last = t0 > kAgentForever - ticks ? kAgentForever : t0 + ticks;
    auto by_tick = [](const AgentEvent &a, int64_t t) { return a.tick <= t; };
    const auto lo = std::lower_bound(ev.begin(), ev.end(), t0, by_tick);  // the first event after t0
    const auto hi = std::lower_bound(lo, ev.end(), last, by_tick);        // the first event after `last`
    if (lo == hi) return s;
    s.first = size_t(lo - ev.begin());
    s.seg.assign(size_t(ticks) + 1, 0u);
    s.died.assign(size_t(ticks), 0u);
    for (auto it = lo; it != hi; ++it) {
        const size_t k = size_t(it->tick - t0 - 1);
        ++s.seg[k + 1];
        s.died[k] += agent_entry_kind(it->entry) == kAgentDies;
    }
    for (size_t k = 0; k < size_t(ticks); ++k) s.seg[k + 1] += s.seg[k];
    return s;
}

}  // namespace swarm
