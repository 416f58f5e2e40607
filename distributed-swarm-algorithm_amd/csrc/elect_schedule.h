// The round schedule of an election (elect.hip's host loop): which rounds a launch covers, which leader
// buffer it reads and writes, how far the launches run ahead of the counts the host has read, and which
// buffer holds the final state.  Integer bookkeeping over the history of per-round change counts, nothing
// of the device: standard headers only, so that a plain g++ program (tests/elect_schedule/) drives it
// against a model of the leader buffers.
//
// Rounds and launches.  Round t's change count lands in counter slot t.  Launch i (1-based) reads leader
// buffer (i-1)&1 and writes i&1; its stamps, their value and their clears follow i as well.  Until pair
// rounds start a launch is a round (i = t).  With a two-hop index (pair_ok), once the last read round
// changed fewer than pair_below agents, ONE single round marks two-hop rows (PF_MARK) and every launch
// behind it covers two rounds (PF_PAIR) -- a single one only where one round is left before max_rounds.
// lend[i] is the last round of launch i (lend[0] = 0).  A sparse launch is guarded by the total of
// lend[i-2], which launch i-1 published: zero means converged, the launch is a no-op.
//
// Batches.  The host enqueues a batch of rounds, then the read-back of rounds (read_upto, tread], tread
// being `look` rounds before the batch's end so that the device still runs while the host reads and decides
// (rounds launched past convergence are guarded no-ops), waits for it, and sizes the next batch from the
// counts.  The newest launched round stays less than ring / 2 rounds ahead of read_upto: a round recycles the
// counter slot ring / 2 rounds ahead of it.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace swarm {

enum RoundKind { RK_DENSE = 0, RK_DENSE_MARK = 1, RK_SPARSE = 2 };

// Kind of frontier round t: the first dense_rounds rounds dense (nearly every agent changes;
// measured best at 9 for 10M agents with the 16-bit columns: 24.15 vs 24.23 ms at 8), the last of
// them marking, then sparse.
inline RoundKind plan_round(int t, int dense_rounds) {
    if (t < dense_rounds) return RK_DENSE;
    if (t == dense_rounds) return RK_DENSE_MARK;
    return RK_SPARSE;
}

// Whether sparse launch t clears the buffer it marks into first (parity t+1, last read by launch t-1):
// every 256 launches, per parity, so no stamp outlives the 510 launches after which its value recurs
// (take_stamps).
inline bool clear_due(int t) { return t > 2 && ((t - 1) & 255) < 2; }

// The interleaved -> agent-order switch point of the stamp layout for an n-agent swarm: marks are dealt
// over the chunks while a round changes at least this many agents (balance), in agent order below
// (locality of the few gathers).  il_min_changes >= 0 overrides (SWARM_IL_MIN_CHANGES).
inline int64_t il_min_for(int64_t n, int il_min_changes) {
    return il_min_changes >= 0 ? il_min_changes : std::max<int64_t>(1, int64_t(8e-4 * double(n)));
}

// Rounds in the next batch of an election loop (launched before the host reads their counts):
// double up to max_batch, but no more than ~1.5x the rounds a linear extrapolation of the last
// 32 per-round change counts leaves before zero -- rounds launched past convergence are wasted
// no-op launches (~8 us each at 10M agents; 164 of them at C3, 106 at C2 with pure doubling).
// doubling_only (SWARM_BATCH_DOUBLING=1): plain doubling (A/B aid).
inline int next_round_batch(const int64_t *hist, size_t nh, int batch, int max_batch, bool doubling_only) {
    int b = batch * 2 < max_batch ? batch * 2 : max_batch;
    constexpr size_t k = 32;
    if (nh >= k && !doubling_only) {
        const double slope = double(hist[nh - k] - hist[nh - 1]) / double(k - 1);
        if (slope > 0) {
            // rounds left on the linear trend, + 25 % and 4 rounds of margin: an overshoot costs one
            // no-op launch per round (~6 µs), an undershoot one more host round trip
            const double rem = 1.25 * double(hist[nh - 1]) / slope + 4.0;
            const int p = rem < 8.0 ? 8 : (rem > double(max_batch) ? max_batch : int(rem + 0.5));
            if (p < b) b = p;
        }
    }
    return b;
}

// The switch to pair rounds happens at a batch's first sparse launch: a batch that is about to cross
// pair_below ends where the linear trend of the last 32 rounds crosses it (8 rounds at the least), and
// within a quarter above it (the curve is flat and noisy there at 10M agents: 20 changes per round of
// slope) batches are 16 rounds, so that the pairs do not start a long batch late.
inline int pair_switch_batch(const int64_t *hist, size_t nh, int batch, int max_batch, double pair_below) {
    if (nh < 32 || double(hist[nh - 1]) < pair_below) return batch;
    const double slope = double(hist[nh - 32] - hist[nh - 1]) / 31.0;
    if (slope > 0) {
        const double rem = 1.1 * (double(hist[nh - 1]) - pair_below) / slope + 2.0;
        batch = std::min(batch, rem < 8.0 ? 8 : rem > double(max_batch) ? max_batch : int(rem));
    }
    if (double(hist[nh - 1]) < 1.25 * pair_below) batch = std::min(batch, 16);
    return batch;
}

// The one-workgroup tail (opt-in) takes over once the last read round's risers x 4 fit its list; batches are
// short once that is near (risers x 4 within 8 lists), so that the switch is not a long batch late.
inline int near_tail_batch(int64_t last_changes, int batch, int tail_cap) {
    return (tail_cap > 0 && last_changes * 4 <= 8 * int64_t(tail_cap)) ? std::min(batch, 8) : batch;
}

enum PairForm { PF_SINGLE = 0, PF_MARK = 1, PF_PAIR = 2 };

struct ScheduleParams {
    int max_rounds = 1;
    int dense_rounds = 0;        // frontier mode: rounds 1..dense_rounds are dense sweeps
    int look = 0;                // look-ahead rounds (0 when the rounds are timed or logged)
    bool frontier = false;       // FRONTIER mode (DENSE: every round a dense sweep)
    bool pair_ok = false;        // pair rounds allowed (two-hop index, int32 CSR, default levers, no tail)
    double pair_below = 0.0;     // ... once the last read round changed fewer agents than this
    int tail_cap = 0;            // > 0: the one-workgroup tail's list capacity
    bool tail_ok = false;        // ... and the call can hand over to it (undirected, int32 CSR, not timed)
    int max_batch = 256;         // rounds a read-back holds (kMaxBatch)
    int ring = 512;              // rounds of counter slots (kRing)
    bool skip_copy = false;      // the leader buffers do not start as copies of ids (rounds 1 and 2 dense)
    bool doubling_only = false;  // SWARM_BATCH_DOUBLING=1
    int64_t il_min = 1;          // il_min_for(n, ...)
};

// The bounds of a batch: rounds [t, tend] are launched (none when t > tend: only a read is left) and the
// counts of rounds (read_upto, tread] are read.  read_first: tread is already launched, so its read-back is
// enqueued in front of the batch's launches; otherwise behind the launch that covers tread.
struct BatchPlan {
    int t, tend, tread;
    bool read_first;
};

struct LaunchPlan {
    int t;              // first round of the launch
    int rounds;         // 1, or 2 for PF_PAIR
    RoundKind kind;
    PairForm form;
    int lc;             // this launch's number: reads leader buffer (lc-1)&1, writes lc&1
    int guard_round;    // lend[lc-2], whose total launch lc-1 published; 0: not guarded (lc <= 2)
    bool rd_il, wr_il;  // stamp layout of the marks it reads / writes: interleaved, else agent order
    bool totals_behind; // the batch's read-back is enqueued behind this launch
};

struct ScheduleEnd {
    int last;            // rounds_exec: the first round that changed nothing, or max_rounds
    bool converged;
    bool copy_b1;        // the final state is in leader buffer 1 only: copy it to buffer 0 (leader)
};

class ElectSchedule {
public:
    explicit ElectSchedule(const ScheduleParams &p) : p_(p), lend_(1, 0) {}

    bool running() const { return read_upto_ < p_.max_rounds && found_ < 0; }

    BatchPlan begin_batch() {
        b_.t = launched_ + 1;
        b_.tend = std::min(p_.max_rounds, launched_ + batch_);
        // at least one round is read (the first batches are shorter than the look-ahead)
        b_.tread = b_.tend == p_.max_rounds ? b_.tend : std::max(read_upto_ + 1, b_.tend - p_.look);
        b_.read_first = b_.tread <= launched_;
        next_ = b_.t;
        last_end_ = launched_;
        return b_;
    }

    // The next launch of the batch begin_batch() opened; false (and the batch's rounds count as launched)
    // when there is none.  A batch's last pair may end one round past tend.
    bool next_launch(LaunchPlan *l) {
        if (next_ > b_.tend) {
            launched_ = std::max(launched_, last_end_);
            return false;
        }
        const int r = next_;
        l->t = r;
        l->rounds = 1;
        l->kind = kind_of(r);
        l->form = PF_SINGLE;
        l->lc = lc_ + 1;
        l->guard_round = lc_ >= 2 ? lend_[lc_ - 1] : 0;
        l->rd_il = rd_il_;
        l->wr_il = hist_.empty() || hist_.back() >= p_.il_min;
        if (p_.frontier) rd_il_ = l->wr_il;
        if (p_.pair_ok && l->kind == RK_SPARSE) {
            if (!pair_mode_ && !hist_.empty() && double(hist_.back()) < p_.pair_below) {
                l->form = PF_MARK;
                pair_mode_ = true;
            } else if (pair_mode_ && r + 1 <= p_.max_rounds) {
                l->form = PF_PAIR;
                l->rounds = 2;
                ++pair_launches_;
            }
        }
        ++lc_;
        last_end_ = r + l->rounds - 1;
        lend_.push_back(last_end_);
        next_ = last_end_ + 1;
        l->totals_behind = b_.tread >= r && b_.tread <= last_end_;
        return true;
    }

    // The change counts of rounds (read_upto, upto] as read back: chg[i * stride] is round read_upto + 1 + i.
    // Returns how many of them count (up to and with the first round that changed nothing).
    int take_counts(const unsigned long long *chg, size_t stride, int upto) {
        int taken = 0;
        for (int r = read_upto_ + 1; r <= upto; ++r) {
            const int64_t c = int64_t(chg[size_t(taken) * stride]);
            hist_.push_back(c);
            ++taken;
            if (c == 0) {
                found_ = r;
                break;
            }
        }
        read_upto_ = upto;
        return taken;
    }

    // After a batch's counts: the size of the next one.  A batch with its look-ahead spans at most max_batch
    // rounds (pair rounds: two rounds of room for the pair that ends past its batch).
    void size_next_batch() {
        batch_ = next_round_batch(hist_.data(), hist_.size(), batch_, p_.max_batch - p_.look - (p_.pair_ok ? 2 : 0),
                                  p_.doubling_only);
        if (p_.pair_ok && !pair_mode_)
            batch_ = pair_switch_batch(hist_.data(), hist_.size(), batch_, p_.max_batch, p_.pair_below);
        if (!hist_.empty()) batch_ = near_tail_batch(hist_.back(), batch_, p_.tail_cap);
        // The newest round of the batch stays less than ring / 2 rounds ahead of read_upto: round t recycles the
        // counter slot of round t - ring / 2, read by then with a round to spare.  A batch of pairs ends one
        // round past its end when it is odd (before the switch-over: when the switch falls that way).
        const int room = p_.ring / 2 - 1 - (launched_ - read_upto_);
        while (batch_ > 1 && batch_ + ((p_.pair_ok && (!pair_mode_ || (batch_ & 1))) ? 1 : 0) > room) --batch_;
    }

    // Whether the one-workgroup tail is tried from round launched + 1 (the caller drains the launched rounds
    // first and asks tail_start_ok() again).
    bool tail_due() const {
        return p_.tail_cap > 0 && p_.tail_ok && found_ < 0 && p_.frontier && !hist_.empty() && hist_.back() > 0 &&
               hist_.back() * 4 <= p_.tail_cap && hist_.back() < tail_retry_below_ && launched_ < p_.max_rounds &&
               kind_of(launched_ + 1) == RK_SPARSE;
    }
    bool tail_start_ok() const { return found_ < 0 && launched_ < p_.max_rounds; }
    // the tail did not start (its list did not fit): retry once the changes halve
    void tail_not_started() { tail_retry_below_ = std::max<int64_t>(1, hist_.back() / 2); }
    // The tail ran rounds launched + 1 .. last, a launch's worth of buffer swaps each, and left its hand-back
    // marks in agent order; the caller reads their counts next.
    void adopt_tail(int last) {
        launched_ = last;
        while (lc_ < launched_) lend_.push_back(++lc_);  // (no pair rounds with the tail: a launch per round)
        rd_il_ = false;
        batch_ = 8;
    }

    // The newest buffer is lc & 1 (lc launches were issued).  After a launch whose rounds all changed nothing
    // both buffers hold the final state (dense and frontier alike).  A pair launch whose first round changed
    // something and whose second nothing leaves it in the buffer it wrote only; the launch behind it (not
    // guarded: its guard word is an earlier, non-zero round's) rewrites the other one.  Without the initial
    // copies a run that ends with round 1 has written buffer 1 only, zero changes or not.
    ScheduleEnd end() const {
        ScheduleEnd e;
        e.converged = found_ > 0;
        e.last = e.converged ? found_ : p_.max_rounds;
        bool newest_only = !e.converged;
        int lfin = lc_;  // the launch that wrote the final state
        if (e.converged) {
            lfin = int(std::lower_bound(lend_.begin(), lend_.end(), found_) - lend_.begin());
            newest_only = lfin == lc_ && lfin >= 1 && lend_[lfin - 1] + 1 != found_;
        }
        e.copy_b1 = (newest_only && (lfin & 1)) || (p_.skip_copy && e.last == 1);
        return e;
    }

    int launched() const { return launched_; }
    int read_upto() const { return read_upto_; }
    int found() const { return found_; }
    int batch() const { return batch_; }
    int launches() const { return lc_; }
    int launch_end(int i) const { return lend_[i]; }
    bool pair_mode() const { return pair_mode_; }
    bool reads_interleaved() const { return rd_il_; }  // the layout of the marks the next sparse launch reads
    int64_t pair_launches() const { return pair_launches_; }
    RoundKind kind_of(int t) const { return p_.frontier ? plan_round(t, p_.dense_rounds) : RK_DENSE; }
    const ScheduleParams &params() const { return p_; }

private:
    ScheduleParams p_;
    int found_ = -1, batch_ = 8, launched_ = 0, read_upto_ = 0;
    int lc_ = 0;                  // launches issued
    std::vector<int> lend_;       // lend_[i]: the last round of launch i
    std::vector<int64_t> hist_;   // per-round change counts read so far
    bool pair_mode_ = false;
    int64_t pair_launches_ = 0;
    bool rd_il_ = true;           // the marks the next sparse launch reads are interleaved
    int64_t tail_retry_below_ = INT64_MAX;
    BatchPlan b_{1, 0, 0, false};
    int next_ = 1, last_end_ = 0;
};

}  // namespace swarm
