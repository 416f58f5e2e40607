// Placing tasks into the slots of closed ones (contract U1-P): the host side's arithmetic.  Standard
// headers only, so that a plain host program can drive it (tests/task_place/task_place_main.cpp).
//
// `last` is the last tick a loop ran on the board.  Slot k may take a new task iff it was absent, under its current
// window [open, close), at ticks last and last - 1 (the quiet rule): the last claim about it was heard at `close`
// at the latest, the conflict that claim caused at close + 1 <= last, so nothing in flight names the slot.  With
// open <= close that is one of
//     close < last          (closed, and the tick after the close has run: close <= last - 1)
//     open > last           (not open yet)
//     open == close         (never present)
// -- comparisons only, no subtraction, so windows next to INT64_MAX and last == 0 cannot overflow.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <iterator>
#include <vector>

namespace swarm {

static inline bool place_eligible(int64_t open, int64_t close, int64_t last) {
    return close < last || open > last || open == close;
}

enum PlaceStatus {
    kPlaceOk = 0,
    kPlaceIndex,       // a slot outside [0, T)
    kPlaceDuplicate,   // a slot listed twice
    kPlaceBusy,        // a slot that is not eligible
    kPlaceNegative,    // a negative open or close tick
    kPlaceEarly,       // a window that opens at or before `last`
    kPlaceOrder,       // open > close
    kPlaceNonFinite,   // a position or velocity that is not finite
    kPlaceReq,         // a requirement outside [-1, 31]
};

// One request against the slot's current window (old_open, old_close: read only when idx is a slot of the board).
static inline PlaceStatus place_check_one(int64_t T, int64_t last, int64_t idx, int64_t old_open, int64_t old_close,
                                          double x, double y, double vx, double vy, int req, int64_t open,
                                          int64_t close) {
    if (idx < 0 || idx >= T) return kPlaceIndex;
    if (!place_eligible(old_open, old_close, last)) return kPlaceBusy;
    if (open < 0 || close < 0) return kPlaceNegative;
    if (open <= last) return kPlaceEarly;
    if (open > close) return kPlaceOrder;
    if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(vx) && std::isfinite(vy))) return kPlaceNonFinite;
    if (req < -1 || req > 31) return kPlaceReq;
    return kPlaceOk;
}

// The m requests in order; *bad (may be NULL) is the first request refused.  vel may be NULL (zero).  The old
// windows are per request, gathered by the caller; those of a request whose idx is no slot are not looked at.
static inline PlaceStatus place_check(int64_t T, int64_t last, int64_t m, const int32_t *idx, const int64_t *old_open,
                                      const int64_t *old_close, const double *pos, const double *vel,
                                      const int8_t *req, const int64_t *open, const int64_t *close, int64_t *bad) {
    for (int64_t j = 0; j < m; ++j) {
        const PlaceStatus st = place_check_one(T, last, idx[j], old_open[j], old_close[j], pos[2 * j], pos[2 * j + 1],
                                               vel ? vel[2 * j] : 0.0, vel ? vel[2 * j + 1] : 0.0, int(req[j]),
                                               open[j], close[j]);
        if (st != kPlaceOk) {
            if (bad) *bad = j;
            return st;
        }
    }
    return kPlaceOk;
}

// Is a slot listed twice?  O(m log m) on a sorted copy; *dup (may be NULL) is the least slot listed twice.
static inline bool place_has_duplicate(int64_t m, const int32_t *idx, int32_t *dup) {
    std::vector<int32_t> s(idx, idx + m);
    std::sort(s.begin(), s.end());
    const auto it = std::adjacent_find(s.begin(), s.end());
    if (it == s.end()) return false;
    if (dup) *dup = *it;
    return true;
}

// The board's list of retiring ticks after a place: the entries <= last leave (those ticks have run), the m new
// close ticks join (INT64_MAX is no tick of a run); ascending, each once.  An old entry whose slot was re-placed
// may stay: a retire that removes nothing writes nothing.  O(m log m + |closes|).
static inline void place_update_closes(std::vector<int64_t> *closes, int64_t last, int64_t m, const int64_t *close) {
    std::vector<int64_t> add;
    for (int64_t j = 0; j < m; ++j)
        if (close[j] != INT64_MAX && close[j] > last) add.push_back(close[j]);
    std::sort(add.begin(), add.end());
    std::vector<int64_t> out;
    out.reserve(closes->size() + add.size());
    const auto from = std::upper_bound(closes->begin(), closes->end(), last);
    std::merge(from, closes->end(), add.begin(), add.end(), std::back_inserter(out));
    out.erase(std::unique(out.begin(), out.end()), out.end());
    closes->swap(out);
}

static inline const char *place_reason(PlaceStatus st) {
    switch (st) {
    case kPlaceOk: return "ok";
    case kPlaceIndex: return "names a slot outside [0, T)";
    case kPlaceDuplicate: return "names a slot listed twice";
    case kPlaceBusy: return "names a slot that is not free (its task was present at one of the last two ticks)";
    case kPlaceNegative: return "has a negative open or close tick";
    case kPlaceEarly: return "opens at or before the last tick run";
    case kPlaceOrder: return "opens after it closes";
    case kPlaceNonFinite: return "has a position or velocity that is not finite";
    default: return "has a treq outside [-1, 31]";
    }
}

}  // namespace swarm
