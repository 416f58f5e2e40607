// Drives csrc/elect_schedule.h's ElectSchedule the way elect.hip's host loop does (run_batch, tail_rounds,
// finish) over synthetic change histories c[1..], and checks every launch against a small model of the two
// leader buffers.  The model knows only the rules of elect.hip's header comment and of the final copy:
//   launch i covers rounds (lend[i-1], lend[i]], reads buffer (i-1)&1 and writes i&1;
//   a buffer "holds the state after round k"; states from R-1 on are equal, R the first round with c[R] == 0;
//   a dense launch of round t is a no-op iff t > 1 and c[t-1] == 0, and writes every entry of its output;
//   a sparse launch is a no-op iff its guard round g > 0 and c[g] == 0; one that runs needs the state after
//   lend[i-1] in its input and the state after lend[i-2] in its output, and leaves the state after lend[i].
// It never asks the header's end() what to expect: it applies end()'s copy to the model and looks at buffer 0.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "elect_schedule.h"

using namespace swarm;

namespace {

constexpr int kNever = INT_MAX;
constexpr int kMaxBatch = 256, kRing = 512;
constexpr int64_t kIlMin = 800;  // il_min_for(1e6, -1)

enum Shape { LINEAR, GEOMETRIC, FLAT_TAIL, N_SHAPES };
const char *kShapeName[] = {"linear", "geometric", "flat_tail"};

// c[r] > 0 for r < R, 0 from R on; R == kNever: a history that never reaches zero
struct History {
    Shape shape;
    int R;
    int64_t at(int r) const {
        if (r >= R) return 0;
        const int span = R == kNever ? 400 : R;
        int64_t v = 0;
        if (shape == LINEAR) v = int64_t(100000.0 * double(span - r) / double(span));
        if (shape == GEOMETRIC) {
            double x = 100000.0;
            const double q = span > 40 ? 0.97 : 0.6;
            for (int i = 1; i < r && x > 0.5; ++i) x *= q;
            v = int64_t(x);
        }
        if (shape == FLAT_TAIL) {  // a steep start, then a long flat noisy tail of a few changes per round
            const int64_t noise = 3 + int64_t((uint32_t(r) * 2654435761u) >> 29);
            v = r < span / 4 ? 100000 / r : noise;
        }
        return v > 0 ? v : 1;
    }
};

struct TailScript {  // the adopted one-workgroup tail: rounds it runs before it hands back, refusals before it starts
    int cap = 0, run = 0, refusals = 0;
};

struct Counts {
    long cases = 0, failed = 0, launches = 0;
    long end_pair_first = 0, end_pair_second = 0, cut_pair_odd = 0, cut_pair_even = 0;
    long mark_first_sparse = 0, mark_via_trend = 0, mark_never = 0, tail_adopted = 0, tail_back = 0, tail_refused = 0;
    long copy_b1 = 0, max_ahead = 0;
} g_n;

struct Launch {
    int t, rounds, lc, guard, batch;
    RoundKind kind;
    PairForm form;
};

struct Checker {
    const History &h;
    const ScheduleParams &p;
    std::string err;
    int hold[2];  // buffer b holds the state after round hold[b]; -1: never written
    std::vector<int> lend{0};
    std::vector<Launch> ls;
    int marks = 0;

    Checker(const History &h_, const ScheduleParams &p_) : h(h_), p(p_) {
        hold[0] = hold[1] = p.skip_copy ? -1 : 0;
    }
    void fail(const std::string &m) {
        if (err.empty()) err = m;
    }
    bool eq(int a, int b) const { return a >= 0 && b >= 0 && (a == b || (a >= h.R - 1 && b >= h.R - 1)); }
    RoundKind want_kind(int t) const {
        if (!p.frontier || t < p.dense_rounds) return RK_DENSE;
        return t == p.dense_rounds ? RK_DENSE_MARK : RK_SPARSE;
    }
    // assertions 1-3 for one launch, then its effect on the model's buffers
    void launch(const Launch &l) {
        const int i = int(lend.size());
        const int a = lend[i - 1], b = l.t + l.rounds - 1;
        if (l.lc != i) fail("lc is not the launch's number");
        if (l.t != a + 1) fail("gap or overlap in the rounds covered");
        if (l.rounds != 1 && l.rounds != 2) fail("a launch covers one or two rounds");
        if (b > p.max_rounds) fail("a launch runs past max_rounds");
        if (l.kind != want_kind(l.t)) fail("round kind");
        if ((l.rounds == 2) != (l.form == PF_PAIR)) fail("two rounds iff PF_PAIR");
        if (l.form != PF_SINGLE && (l.kind != RK_SPARSE || !p.pair_ok)) fail("pair forms on sparse rounds of pair_ok only");
        if (l.form == PF_PAIR && marks != 1) fail("PF_PAIR without exactly one PF_MARK before it");
        if (l.form == PF_MARK) {
            if (++marks != 1) fail("a second PF_MARK");
            // the switch is decided from the counts read, which change between batches only: it falls on the
            // batch's first launch, or behind the dense launches that open the batch
            for (size_t k = ls.size(); k-- > 0 && ls[k].batch == l.batch;)
                if (ls[k].kind == RK_SPARSE) fail("PF_MARK behind a sparse launch of its batch");
        }
        if (marks == 1 && l.form == PF_SINGLE && l.kind == RK_SPARSE && b < p.max_rounds)
            fail("a single round inside pair mode with two rounds left");
        const int g = i >= 3 ? lend[i - 2] : 0;
        if (l.guard != g) fail("guard_round is not lend[i-2]");
        if (g > 0 && ls[i - 2].t != g + 1) fail("no earlier launch publishes the guard round's total");
        const int in = (i - 1) & 1, out = i & 1;
        if (l.kind != RK_SPARSE) {
            if (!(b > 1 && h.at(b - 1) == 0)) {
                const int src = (i == 1 && p.skip_copy) ? 0 : hold[in];  // round 1 reads ids without the copies
                if (!eq(src, a)) fail("a dense launch reads a stale buffer");
                hold[out] = b;
            }
        } else if (!(g > 0 && h.at(g) == 0)) {
            if (!eq(hold[in], a)) fail("a sparse launch's input does not hold the state after lend[i-1]");
            if (!eq(hold[out], i >= 2 ? lend[i - 2] : 0)) fail("a sparse launch's output does not hold the state after lend[i-2]");
            hold[out] = b;
        }
        lend.push_back(b);
        ls.push_back(l);
        ++g_n.launches;
    }
};

// One election over history h: the loop of elect_impl with the device replaced by h.
void run_case(const History &h, const ScheduleParams &p, const TailScript &ts, const std::string &name) {
    Checker ck(h, p);
    ElectSchedule sc(p);
    std::vector<unsigned long long> buf(kMaxBatch);
    int issued = 0, batch_no = 0, refusals = ts.refusals;
    bool trend = false, adopted = false, back = false;
    std::vector<int64_t> read;  // the counts the host has taken, as the schedule sees them
    // assertion 4: a read-back of rounds (from, upto]
    auto enqueue = [&](int from, int upto) {
        if (upto > issued) ck.fail("totals enqueued for a round that is not launched");
        if (upto <= from || upto - from > kMaxBatch) ck.fail("a read covers 1..kMaxBatch rounds");
        for (int r = from + 1; r <= upto; ++r) buf[size_t(r - from - 1)] = (unsigned long long)h.at(r);
    };
    auto take = [&](int upto) {
        const int r0 = sc.read_upto() + 1, n = sc.take_counts(buf.data(), 1, upto);
        for (int r = r0; r < r0 + n; ++r) read.push_back(h.at(r));
        if (sc.read_upto() != upto) ck.fail("read_upto after a read");
    };
    int guard_loops = 0;
    while (sc.running() && ck.err.empty()) {
        if (++guard_loops > 5000) {
            ck.fail("the loop does not end");
            break;
        }
        const BatchPlan bp = sc.begin_batch();
        const int from = sc.read_upto();
        int reads = 0;
        ++batch_no;
        if (bp.t != issued + 1) ck.fail("a batch does not start behind the last launched round");
        if (bp.tread <= from || bp.tread > p.max_rounds) ck.fail("tread out of range");
        if (bp.read_first) enqueue(from, bp.tread), ++reads;
        LaunchPlan l;
        while (sc.next_launch(&l)) {
            ck.launch({l.t, l.rounds, l.lc, l.guard_round, batch_no, l.kind, l.form});
            issued = l.t + l.rounds - 1;
            if (issued - from >= p.ring / 2) ck.fail("a launch kRing/2 or more rounds ahead of read_upto");
            g_n.max_ahead = std::max<long>(g_n.max_ahead, issued - from);
            if (l.totals_behind) enqueue(from, bp.tread), ++reads;
            if (l.form == PF_MARK) (trend ? g_n.mark_via_trend : g_n.mark_first_sparse) += 1;
        }
        if (sc.launched() != issued) ck.fail("launched() is not the last round launched");
        if (reads != 1) ck.fail("the host waits for a read-back that was not enqueued exactly once");
        take(bp.tread);
        sc.size_next_batch();
        if (sc.batch() < 1 || sc.batch() + p.look + (p.pair_ok ? 2 : 0) > kMaxBatch) ck.fail("batch size");
        // the pair switch-over's trend cap engaged: the batch is shorter than plain batch sizing makes it
        if (p.pair_ok && !sc.pair_mode() && read.size() >= 32 && double(read.back()) >= p.pair_below) trend = true;
        if (sc.tail_due()) {
            if (sc.launched() > sc.read_upto()) enqueue(sc.read_upto(), sc.launched()), take(sc.launched());
            if (!sc.tail_start_ok()) continue;
            if (refusals-- > 0) {
                sc.tail_not_started();
                ++g_n.tail_refused;
                continue;
            }
            const int t0 = sc.launched() + 1;
            int last = std::min(std::min(p.max_rounds, t0 + 199), t0 + ts.run - 1);
            if (h.R >= t0) last = std::min(last, h.R);  // the tail stops at the first round that changes nothing
            for (int r = t0; r <= last; ++r) {
                const int i = int(ck.lend.size());
                ck.launch({r, 1, i, i >= 3 ? ck.lend[i - 2] : 0, -1, RK_SPARSE, PF_SINGLE});
            }
            issued = last;
            sc.adopt_tail(last);
            adopted = true;
            if (sc.launches() != int(ck.lend.size()) - 1) ck.fail("launch count after the tail");
            enqueue(sc.read_upto(), last), take(last);
            if (sc.running() && sc.launched() < p.max_rounds) back = true;
        }
    }
    // assertion 5: the end-of-run decision applied to the model
    const ScheduleEnd e = sc.end();
    if (e.copy_b1) ck.hold[0] = ck.hold[1], ++g_n.copy_b1;
    const int want_last = std::min(h.R, p.max_rounds);
    if (e.last != want_last) ck.fail("rounds_exec");
    if (e.converged != (h.R <= p.max_rounds)) ck.fail("converged");
    if (!ck.eq(ck.hold[0], want_last)) ck.fail("leader does not hold the final state");
    if (ck.err.empty()) {
        const Launch *fin = nullptr;
        for (const Launch &l : ck.ls)
            if (l.t <= want_last && want_last < l.t + l.rounds) fin = &l;
        if (e.converged && fin && fin->form == PF_PAIR) (want_last == fin->t ? g_n.end_pair_first : g_n.end_pair_second) += 1;
        if (!e.converged && sc.pair_mode()) (sc.launches() & 1 ? g_n.cut_pair_odd : g_n.cut_pair_even) += 1;
        if (p.pair_ok && !sc.pair_mode()) ++g_n.mark_never;
        g_n.tail_adopted += adopted;
        g_n.tail_back += back;
    }
    ++g_n.cases;
    if (!ck.err.empty()) {
        if (++g_n.failed <= 20) printf("FAIL %s: %s\n", name.c_str(), ck.err.c_str());
    }
}

std::string name_of(const History &h, const ScheduleParams &p, int pair_case, const TailScript &ts) {
    char b[256];
    snprintf(b, sizeof b, "%s R=%d max=%d dense=%d look=%d %s skip=%d pairs=%d below=%.0f tail=%d/%d/%d",
             kShapeName[h.shape], h.R, p.max_rounds, p.dense_rounds, p.look, p.frontier ? "frontier" : "dense",
             int(p.skip_copy), pair_case, p.pair_below, ts.cap, ts.run, ts.refusals);
    return b;
}

void family(const History &h, const std::vector<int> &max_rounds) {
    for (int mr : max_rounds)
        for (int dense : {0, 1, 2, 9, 10})
            for (int look : {0, 1, 8, 64})
                for (int frontier : {0, 1})
                    for (int skip : {0, 1})
                        for (int pc = 0; pc < (frontier ? 4 : 1); ++pc) {
                            if (mr < 1 || (skip && frontier && dense < 2)) continue;
                            ScheduleParams p;
                            p.max_rounds = mr;
                            p.dense_rounds = dense;
                            p.look = look;
                            p.frontier = frontier;
                            p.skip_copy = skip;
                            p.max_batch = kMaxBatch;
                            p.ring = kRing;
                            p.il_min = kIlMin;
                            // pairs: not allowed; from the first sparse round; from the middle of the run (long
                            // decays get there through the trend cap); allowed but never reached
                            p.pair_ok = pc > 0;
                            const int mid = h.R == kNever ? 200 : std::max(1, h.R / 2);
                            p.pair_below = pc == 1 ? 1e18 : pc == 2 ? double(h.at(mid)) + 0.5 : 0.0;
                            run_case(h, p, TailScript{}, name_of(h, p, pc, TailScript{}));
                        }
}

// the opt-in tail: a hand-over, the rounds it runs, the hand-back to frontier rounds (or the end inside it)
void tail_family(const History &h, const std::vector<int> &max_rounds) {
    for (int mr : max_rounds)
        for (int dense : {0, 2, 9})
            for (int look : {0, 8})
                for (int cap : {16, 2048})
                    for (int run : {1, 3, 200})
                        for (int refusals : {0, 1}) {
                            if (mr < 1) continue;
                            ScheduleParams p;
                            p.max_rounds = mr;
                            p.dense_rounds = dense;
                            p.look = look;
                            p.frontier = true;
                            p.tail_cap = cap;
                            p.tail_ok = true;
                            p.max_batch = kMaxBatch;
                            p.ring = kRing;
                            p.il_min = kIlMin;
                            const TailScript ts{cap, run, refusals};
                            run_case(h, p, ts, name_of(h, p, 0, ts));
                        }
}

}  // namespace

int main() {
    std::vector<int> short_r, long_r = {255, 256, 257, 258, 259, 260, 510, 511, 512, 513, 514, 515, 516, 1100};
    for (int r = 1; r <= 12; ++r) short_r.push_back(r);
    for (int s = 0; s < N_SHAPES; ++s) {
        for (int R : short_r) {
            std::vector<int> mr;
            for (int m = 1; m <= R + 3; ++m) mr.push_back(m);
            family(History{Shape(s), R}, mr);
            tail_family(History{Shape(s), R}, {R, R + 3});
        }
        for (int R : long_r) {
            family(History{Shape(s), R}, {R - 1, R, R + 1, 257});
            tail_family(History{Shape(s), R}, {R - 1, R + 1, 257});
        }
        // a history that never reaches zero: every run is cut by max_rounds
        family(History{Shape(s), kNever}, {1, 2, 3, 10, 11, 12, 257, 600, 601});
        tail_family(History{Shape(s), kNever}, {257, 600});
    }
    printf("cases %ld launches %ld\n", g_n.cases, g_n.launches);
    printf("ended_on_pair_first_round %ld\nended_on_pair_second_round %ld\n", g_n.end_pair_first, g_n.end_pair_second);
    printf("cut_in_pair_mode_odd_launches %ld\ncut_in_pair_mode_even_launches %ld\n", g_n.cut_pair_odd, g_n.cut_pair_even);
    printf("pair_switch_on_first_sparse_batch %ld\npair_switch_through_trend_cap %ld\npair_switch_never %ld\n",
           g_n.mark_first_sparse, g_n.mark_via_trend, g_n.mark_never);
    printf("tail_adopted %ld\ntail_handed_back %ld\ntail_refused_first %ld\nfinal_copy_from_buffer_1 %ld\n",
           g_n.tail_adopted, g_n.tail_back, g_n.tail_refused, g_n.copy_b1);
    printf("max_rounds_ahead_of_read_upto %ld\n", g_n.max_ahead);
    printf("%ld failed\n", g_n.failed);
    return g_n.failed ? 1 : 0;
}
