// Task lifetimes (contract U1-A): the host schedule of a board whose tasks open and close during a
// run.  Pure arithmetic, no HIP includes, so that a plain host program can drive it (tests/task_life/
// task_life_main.cpp); task_board.hip compiles the presence predicate for the device as well (SWARM_HD).
//
// Task k carries one window [open[k], close[k]) of absolute ticks and is present at tick t iff
// open[k] <= t < close[k]: two comparisons, no subtraction, so ticks up to INT64_MAX cannot overflow.
// close == kLifeForever never closes; open == close is a task that is never present.  A tick *retires* -- the
// status entries of absent tasks leave every row at its start -- iff some close[k] equals it, or it is the first
// tick run after the lifetimes were set or changed.  The host knows that schedule, so the retire kernel is
// launched on those ticks alone, with no host wait.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#ifndef SWARM_HD
#if defined(__HIPCC__)
#define SWARM_HD __host__ __device__
#else
#define SWARM_HD
#endif
#endif

namespace swarm {

constexpr int64_t kLifeForever = INT64_MAX;

SWARM_HD static inline bool task_present(int64_t open, int64_t close, int64_t t) { return open <= t && t < close; }

enum TaskLifeStatus {
    kTaskLifeOk = 0,
    kTaskLifeNegative,  // an open or close tick below zero
    kTaskLifeOrder,     // open > close
};

// The validity of T windows; *bad (may be NULL) is the first task refused.
static inline TaskLifeStatus task_life_check(int64_t T, const int64_t *open, const int64_t *close, int64_t *bad) {
    for (int64_t k = 0; k < T; ++k) {
        const TaskLifeStatus st = open[k] < 0 || close[k] < 0 ? kTaskLifeNegative
                                  : open[k] > close[k]        ? kTaskLifeOrder
                                                              : kTaskLifeOk;
        if (st != kTaskLifeOk) {
            if (bad) *bad = k;
            return st;
        }
    }
    return kTaskLifeOk;
}

// The ticks at which some task closes, ascending, each once (kLifeForever is no tick of a run).
static inline std::vector<int64_t> task_close_ticks(int64_t T, const int64_t *close) {
    std::vector<int64_t> out;
    for (int64_t k = 0; k < T; ++k)
        if (close[k] != kLifeForever) out.push_back(close[k]);
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return out;
}

// Does tick t retire?  `closes`: task_close_ticks' list; fresh: the lifetimes were set or changed and no tick has
// run since.
static inline bool task_tick_retires(const std::vector<int64_t> &closes, bool fresh, int64_t t) {
    return fresh || std::binary_search(closes.begin(), closes.end(), t);
}

// How many of the T tasks are present at tick t.
static inline int64_t task_count_present(int64_t T, const int64_t *open, const int64_t *close, int64_t t) {
    int64_t c = 0;
    for (int64_t k = 0; k < T; ++k) c += task_present(open[k], close[k], t);
    return c;
}

}  // namespace swarm
