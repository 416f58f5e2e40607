// Timer FSM / protocol ticks on gfx950.
//
// The reference runs every agent's update_loop at 10 Hz (agent.py:66-80): each tick it handles
// inbound packets and then _process_logic -- the failure detector / election timer
// _check_election_timeout (217-241) and the leader's _send_heartbeat (283-289).  Here the whole
// swarm ticks at once under contract T1 (tools/gen_golden.py ref_fsm, pinned against the real
// handlers): one launch per tick, one thread per agent, which
//   receives  the packets its CSR neighbours sent during the previous tick, in CSR order, as the
//             handlers process them (_handle_election_acclaim 263-275 + _handle_coordinator
//             277-281, _handle_heartbeat 243-261; the bully heartbeat only when the agent's own
//             tick % 10 == 0, 288);
//   ticks     its election timer: FOLLOWER silent for > timeout -> ELECTION_WAIT with a jitter
//             delay (a counter-based hash of (seed, id, tick), so every run draws the same);
//             ELECTION_WAIT past its delay -> LEADER + ELECTION_ACCLAIM + COORDINATOR;
//   sends     into its outbox byte (tick-parity double buffer): bit 0 ACCLAIM+COORDINATOR,
//             bit 1 HEARTBEAT -- exact, see swarm_oracle.c orc_protocol.
// Push mode (the hearers CSR given), one launch per tick:
//   k_tick   receive + timers, its workgroups in two roles: the receive role lists each 4 096-agent
//            chunk's receivers (mail bit set: 1 bit per agent, set by last tick's senders) in LDS
//            and serves them one per thread -- its one sender directly, or its CSR row in order
//            (col / outbox loads in chunks of kRecv, all in flight) when it has several -- then
//            their timers; the sweep role streams every other agent's timers (kSweepV agents per
//            thread); sends are listed in the workgroup's own segment (no global atomics),
//            per-tick counters; then each workgroup mails the hearers of the senders it listed
//            (64-bit atomicOr into the next tick's words, combined per word, all hearer loads in
//            flight).  The words rotate over three buffers: tick t reads buf(t), mails into
//            buf(t+1) and clears buf(t+2).
// (Rounds 2-3 ran k_compact + k_receive + k_sweep + k_mail, round 4 first k_tick + k_mail: the
// boundaries and the list round trips per tick.)
// A quiet agent costs ~9 B (its 8-byte record -- state, alive, leader-position flag, tick phase and its
// timer as a tick of the run -- and its outbox byte) plus its mail bit; only receivers pay for their
// rows.  Storm ticks: when a workgroup's senders exceed pull_frac x the agents of its share (a timeout wave: thousands of ACCLAIMs at once), it skips the mail atomics
// and the next tick pulls instead -- every alive agent walks its own row, as pull mode does.  Same results: an agent
// without a sender in its row hears nothing either way.  Pull mode (no hearers CSR): one fused
// launch in which every agent walks its row -- the cross-check.  Both are latency-bound gathers, no
// arithmetic worth the name.
// Agents killed at a kill tick (every alive LEADER then) stop receiving and sending.
//
// swarm_update_loop (contract U1, agent.py:67-81) runs the same ticks, each followed by the physics step of
// that tick (physics.hip k_physics_loop, on the run's records); the tick kernels are the same and read the
// heartbeat positions from the lagged one of the loop's two position buffers.  swarm_update_loop_sensed
// (U1-S) senses every tick's separation neighbours from the tick's snapshot (k_physics_loop_sensed), and a
// refused tick makes the call restore every caller array on the device (k_restore_refused: all or nothing).
// swarm_update_loop_radio (U1-R) is the sensed loop without a message graph: k_tick_radio is k_tick_pull's
// agent with the row walk replaced by the receive over its 3 x 3 cell window of the same binning (hear_window).
// swarm_update_loop_tasks (U1-T) is the radio loop with _process_tasks and the two task handlers run every tick:
// k_radio_outbox<true>, k_task_conflicts and k_tick_radio_tasks in place of the two radio kernels (TaskState).
// swarm_update_loop_channel (U1-L) is either of the two over a lossy channel: the three kernels that hear are
// templates on the channel (link_loss.h), k_*<NoLoss> what the loss-free loops launch, k_*<Lossy> what it adds.
// The four tick kernels (k_tick_pull, k_tick, k_tick_radio, k_tick_radio_tasks) differ in how an agent receives;
// what follows the receive is one function (settle_agent), and the two window kernels share the receive too.
// swarm_update_loop_board (U1-B) is U1-T / U1-L on a board of up to 2^24 tasks with sparse per-agent state:
// k_radio_outbox<true>, k_board_conflicts and k_tick_radio_board (BoardState), the same receive and settle_agent.
// The host loop of every entry point is run_ticks, a sequence of stages that each own their scratch:
// check_run_args, Counters (TickSums: a run's per-tick counters, also the task and link counts), pack_records,
// PushState / RadioState / TaskState / launch_tick_pull (the receive launch by mode), EntrySnapshot (sensed),
// TickClocks (A/B aid), tick_physics, read_back (one host wait).  Agent lifetimes (U1-J, agent_life.hip): a handle found
// from fsm->alive; on a tick with events one launch over that tick's events, right after the leader kill.
#include <cmath>
#include <cstring>

#include "fsm_records.h"
#include "link_loss.h"
#include "task_grid.h"
#include "tick_segments.h"
#include "utility.h"
#include "window_merge.h"

namespace swarm {
namespace {

constexpr uint8_t kAcclaim = 1, kHeartbeat = 2;
constexpr uint8_t kClaim = 4, kConflict = 8;  // U1-T's sender bytes: the outbox bits and these two
constexpr int kRecv = 8;  // CSR entries loaded per receive chunk (pull mode, hearer walks)
// k_tick's row walks (75 VGPRs, 6 waves per SIMD; 4 entries per chunk: 63 VGPRs, 8 waves, but
// 0.135 against 0.128 ms per tick -- the walks' chunks one after the other cost more than the
// occupancy gains; SWARM_RECV_TICK: A/B builds)
#ifndef SWARM_RECV_TICK
#define SWARM_RECV_TICK 8
#endif
constexpr int kRecvTick = SWARM_RECV_TICK;
constexpr uint8_t ST_F = SWARM_FOLLOWER, ST_W = SWARM_ELECTION_WAIT, ST_L = SWARM_LEADER;

__device__ __forceinline__ double jitter_u(uint64_t seed, int32_t id, int64_t t) {
    uint64_t x = seed ^ (uint64_t(uint32_t(id)) * 0x9E3779B97F4A7C15ull) ^ (uint64_t(t) * 0xD1B54A32D192ED03ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    return double(x >> 11) * (1.0 / 9007199254740992.0);
}

// The run's per-agent records (uint2 flag word + timer tick, LRec leader + leader position): fsm_records.h.
struct Fsm {
    uint2 *rec;  // (flag word, timer tick)
    LRec *lrec;
    double *last_hb, *wait_start, *delay;  // the caller's (kH64 timers; written when a wait starts)
    int64_t t0, t_end;                     // the run's ticks: t0 + 1 .. t_end
    double dt;
};

__device__ __forceinline__ void set_lpos(const Fsm &f, int64_t i, float x, float y) {
    *reinterpret_cast<float2 *>(&f.lrec[i].x) = make_float2(x, y);
}

// The first tick t in [lo, t_end] with double(t) * dt - ws > d, relative to t0; 0 when there is none
// (dt > 0: the test is monotone in t).  Tried first at the estimate floor((ws + d) / dt) + 1, clamped to
// [lo, t_end] (right but for rounding: then one test each side), bisection only when that is off.
__host__ __device__ __forceinline__ int32_t wait_exit(int64_t lo, int64_t t_end, int64_t t0, double dt, double ws,
                                                      double d) {
    auto go = [&](int64_t t) { return double(t) * dt - ws > d; };
    if (lo > t_end || !go(t_end)) return 0;
    int64_t hi = t_end;  // go(hi)
    const double g = std::floor((ws + d) / dt) + 1.0;
    if (g == g) {
        const int64_t c = g <= double(lo) ? lo : g >= double(t_end) ? t_end : int64_t(g);
        if (go(c)) {
            if (c == lo || !go(c - 1)) return int32_t(c - t0);
            hi = c - 1;
        } else {
            lo = c + 1;  // c < t_end: go(t_end) holds
        }
    }
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (go(mid)) hi = mid;
        else lo = mid + 1;
    }
    return int32_t(lo - t0);
}

__global__ __launch_bounds__(kBlock) void k_kill_leaders(int64_t n, uint2 *__restrict__ rec) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
        const uint32_t w = rec[i].x;
        if (fw_alive(w) && fw_state(w) == ST_L) rec[i].x = w & ~0xFF00u;
    }
}

// The C-ABI's fields -> records (once per run).
__global__ __launch_bounds__(kBlock) void k_pack_fsm(int64_t n, const uint8_t *__restrict__ state,
                                                    const uint8_t *__restrict__ alive,
                                                    const uint8_t *__restrict__ hl,
                                                    const int32_t *__restrict__ tick_off,
                                                    const int32_t *__restrict__ leader,
                                                    const float2 *__restrict__ lpos, Fsm f) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
        const int32_t ph = ((tick_off[i] % 10) + 10) % 10;
        const uint8_t st = state[i];
        uint32_t bits = hl[i] ? kHL : 0u;
        int32_t y = 0;
        if (st == ST_F) {  // last_hb as a tick of the run, if one represents it exactly
            const double lhb = f.last_hb[i];
            const double k = f.dt != 0.0 ? std::nearbyint(lhb / f.dt) : 0.0;
            const bool ok = f.dt != 0.0 && std::fabs(k) < 9.0e15 && k * f.dt == lhb &&
                            k - double(f.t0) > -2147483647.0 && k - double(f.t0) < 2147483647.0;
            if (ok) y = int32_t(int64_t(k) - f.t0);
            else bits |= kH64;
        } else if (st == ST_W) {
            if (f.dt > 0.0) y = wait_exit(f.t0 + 1, f.t_end, f.t0, f.dt, f.wait_start[i], f.delay[i]);
            else bits |= kH64;
        }
        f.rec[i] = make_uint2(fw_make(st, alive[i], bits, ph), uint32_t(y));
        const float2 q = lpos[i];
        f.lrec[i] = LRec{q.x, q.y, leader[i], 0};
    }
}

// Records -> the C-ABI's fields (once per run).
__global__ __launch_bounds__(kBlock) void k_unpack_fsm(int64_t n, uint8_t *__restrict__ state,
                                                      uint8_t *__restrict__ alive, uint8_t *__restrict__ hl,
                                                      int32_t *__restrict__ leader, float2 *__restrict__ lpos,
                                                      Fsm f) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
        const uint2 r = f.rec[i];
        state[i] = fw_state(r.x);
        alive[i] = fw_alive(r.x);
        hl[i] = (fw_bits(r.x) & kHL) ? 1 : 0;
        if (fw_bits(r.x) & kDirty) f.last_hb[i] = double(f.t0 + int32_t(r.y)) * f.dt;
        const LRec q = f.lrec[i];
        leader[i] = q.leader;
        lpos[i] = make_float2(q.x, q.y);
    }
}

// Handlers for everything agent (me) hears in CSR row [b, e) (see the header).  The row in
// chunks of kRecv: all column loads, then all outbox loads in flight, then the handlers in CSR
// order on registers; sender IDs only for neighbours that sent something.
struct Heard {
    uint8_t st, ob;
    bool live, lead_set;
    int32_t lead, hb_from;  // hb_from: the last accepted heartbeat's sender (its position -> leader_pos)
};

// What one sender's packets of a tick do to the receiver (s: sender ID, j: its index), in the
// order it sent them: ACCLAIM then COORDINATOR, then HEARTBEAT.
__device__ __forceinline__ void hear(Heard &h, uint8_t o, int32_t s, int32_t j, int32_t me, bool hb_tick) {
    if (o & kAcclaim) {
        if (s < me && (h.st == ST_L || h.st == ST_W) && hb_tick) h.ob |= kHeartbeat;  // bully back
        h.lead = s;  // (higher sender: follow) then COORDINATOR: unconditional takeover
        h.lead_set = true;
        h.st = ST_F;
        h.live = true;
    }
    if (o & kHeartbeat) {
        if (h.st == ST_L && s < me) {
            if (hb_tick) h.ob |= kHeartbeat;
        } else {
            h.st = ST_F;  // yield (LEADER) / stop waiting (ELECTION_WAIT) / stay FOLLOWER
            h.lead = s;
            h.lead_set = true;
            h.live = true;
            h.hb_from = j;
        }
    }
}

template <int R>
__device__ __forceinline__ void receive_row(int32_t b, int32_t e, const int32_t *__restrict__ col,
                                            const uint8_t *__restrict__ ob_in, const int32_t *__restrict__ ids,
                                            int32_t me, bool hb_tick, Heard &h) {
    for (int32_t k0 = b; k0 < e; k0 += R) {
        int32_t jj[R];
        uint8_t oo[R];
#pragma unroll
        for (int u = 0; u < R; ++u) jj[u] = k0 + u < e ? col[k0 + u] : -1;
        uint8_t any = 0;
#pragma unroll
        for (int u = 0; u < R; ++u) {
            oo[u] = jj[u] >= 0 ? ob_in[jj[u]] : uint8_t(0);
            any |= oo[u];
        }
        if (!any) continue;
        int32_t ss[R];  // the senders' IDs, all loads in flight
#pragma unroll
        for (int u = 0; u < R; ++u) ss[u] = oo[u] ? ids[jj[u]] : 0;
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const uint8_t o = oo[u] & (kAcclaim | kHeartbeat);
            if (o) hear(h, o, ss[u], jj[u], me, hb_tick);
        }
    }
}

// A liveness proof sets last_hb = now: the timer becomes this tick; the heartbeat's leader position (state
// / leader: caller).
__device__ __forceinline__ void apply_heard(int64_t i, const Heard &h, int64_t t, const double2 *__restrict__ pos,
                                            const Fsm &f, uint32_t &bits, int32_t &y) {
    if (h.live) {
        y = int32_t(t - f.t0);
        bits = (bits & ~kH64) | kDirty;
    }
    if (h.hb_from >= 0) {
        const double2 q = pos[h.hb_from];
        set_lpos(f, i, float(q.x), float(q.y));
        bits |= kHL;
    }
}

// _check_election_timeout (217-241) and the leader's heartbeat (283-289) for agent i in state
// st; `heard`: it got a liveness proof this tick (its timer is now).  Returns the sends.
__device__ __forceinline__ uint8_t timers(int64_t i, uint8_t &st, bool heard, int32_t &lead, bool &lead_set,
                                          int64_t t, double now, double timeout, double jitter, uint64_t seed,
                                          const int32_t *__restrict__ ids, int32_t phase, const Fsm &f,
                                          uint32_t &bits, int32_t &y) {
    uint8_t ob = 0;
    if (st == ST_F && !heard) {
        const double last_hb = (bits & kH64) ? f.last_hb[i] : double(f.t0 + y) * f.dt;
        if (now - last_hb > timeout) {
            if (bits & kDirty) f.last_hb[i] = last_hb;
            st = ST_W;
            const double d = 0.0 + jitter * jitter_u(seed, ids[i], t);
            f.wait_start[i] = now;
            f.delay[i] = d;
            lead = -1;
            lead_set = true;
            bits &= ~(kHL | kDirty);
            set_lpos(f, i, 0.f, 0.f);
            if (f.dt > 0.0) {
                y = wait_exit(t + 1, f.t_end, f.t0, f.dt, now, d);
                bits &= ~kH64;
            } else {
                bits |= kH64;
            }
        }
    }
    if (st == ST_W) {
        const bool done = (bits & kH64) ? now - f.wait_start[i] > f.delay[i] : (y != 0 && t - f.t0 >= int64_t(y));
        if (done) {
            st = ST_L;
            lead = ids[i];
            lead_set = true;
            ob |= kAcclaim;
        }
    }
    if (st == ST_L && ((t + phase) % 10) == 0) ob |= kHeartbeat;
    return ob;
}

// Per-tick counters: wave reduce, one LDS atomic per wave, one global atomic per workgroup into
// one of kShards copies (blockIdx-interleaved; k_sum_counts adds them up).  A single copy made
// every workgroup's 4 atomics queue on the same 4 addresses: ~50 us per tick at 4 096
// workgroups, ~470 us at one agent per thread (measured).
constexpr int kShards = 64;
constexpr int kTraffic = 8;  // traffic counters (swarm_protocol_run_ex), sharded like the tick counts

// Per-workgroup traffic counts into one of kShards copies (one atomic per nonzero value).
__device__ __forceinline__ void add_traffic(unsigned long long *tr, int k, unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (tr && (threadIdx.x & 63) == 0 && v) atomicAdd(&tr[(blockIdx.x & (kShards - 1)) * kTraffic + k], v);
}

__device__ __forceinline__ void add_counts(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned *s_cnt,
                                           unsigned long long *counts) {
    counts += 4 * (blockIdx.x & (kShards - 1));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c0 += __shfl_xor(c0, off, 64);
        c1 += __shfl_xor(c1, off, 64);
        c2 += __shfl_xor(c2, off, 64);
        c3 += __shfl_xor(c3, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (c0) atomicAdd(&s_cnt[0], c0);
        if (c1) atomicAdd(&s_cnt[1], c1);
        if (c2) atomicAdd(&s_cnt[2], c2);
        if (c3) atomicAdd(&s_cnt[3], c3);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// counts[t][shard][c] -> out[t][c]
__global__ __launch_bounds__(kBlock) void k_sum_counts(int64_t ticks, const unsigned long long *__restrict__ part,
                                                      unsigned long long *__restrict__ out) {
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < ticks * 4; q += int64_t(gridDim.x) * kBlock) {
        const int64_t t = q / 4, c = q % 4;
        unsigned long long sum = 0;
        for (int sh = 0; sh < kShards; ++sh) sum += part[(t * kShards + sh) * 4 + c];
        out[q] = sum;
    }
}

struct TickCounts {
    unsigned lead = 0, wait = 0, acc = 0, hb = 0;
    unsigned single = 0, multi = 0, edges = 0;  // one thread's, one tick: < 2^32 (32-bit: VGPRs)
};

// The end of every tick kernel's alive agent i, after what it heard (h; r0: its record at the start of the
// tick, bits / y: after the receive): its timers, its record (written when it changed), its leader, the
// tick's four counts.  Returns its sends; the outbox write is the caller's.
__device__ __forceinline__ uint8_t settle_agent(int64_t i, Heard &h, uint2 r0, uint32_t bits, int32_t y, int64_t t,
                                                double now, double timeout, double jitter, uint64_t seed,
                                                const int32_t *__restrict__ ids, const Fsm &f, TickCounts &c) {
    const int32_t ph = fw_phase(r0.x);
    const uint8_t ob = uint8_t(h.ob | timers(i, h.st, h.live, h.lead, h.lead_set, t, now, timeout, jitter, seed, ids,
                                             ph, f, bits, y));
    const uint32_t fw1 = fw_make(h.st, 1, bits, ph);
    if (fw1 != r0.x || uint32_t(y) != r0.y) f.rec[i] = make_uint2(fw1, uint32_t(y));
    if (h.lead_set) f.lrec[i].leader = h.lead;
    c.lead += h.st == ST_L;
    c.wait += h.st == ST_W;
    c.acc += (ob & kAcclaim) != 0;
    c.hb += (ob & kHeartbeat) != 0;
    return ob;
}

// ---------------------------------------------------------------- pull mode: one fused launch
__global__ __launch_bounds__(kBlock) void k_tick_pull(int64_t n, int64_t t, const int32_t *__restrict__ ids,
                                                     const double2 *__restrict__ pos, const int32_t *__restrict__ rp,
                                                     const int32_t *__restrict__ col, Fsm f,
                                                     const uint8_t *__restrict__ ob_in, uint8_t *__restrict__ ob_out,
                                                     double dt, double timeout, double jitter, uint64_t seed,
                                                     unsigned long long *__restrict__ counts) {
    __shared__ unsigned s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const double now = double(t) * dt;
    TickCounts c;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
        const uint2 r = f.rec[i];
        if (!fw_alive(r.x)) {
            ob_out[i] = 0;
            continue;
        }
        uint32_t bits = fw_bits(r.x);
        int32_t y = int32_t(r.y);
        Heard h{fw_state(r.x), 0, false, false, 0, -1};
        receive_row<kRecv>(rp[i], rp[i + 1], col, ob_in, ids, ids[i], ((t + fw_phase(r.x)) % 10) == 0, h);
        apply_heard(i, h, t, pos, f, bits, y);
        ob_out[i] = settle_agent(i, h, r, bits, y, t, now, timeout, jitter, seed, ids, f, c);
    }
    add_counts(c.lead, c.wait, c.acc, c.hb, s_cnt, counts);
}

// ---------------------------------------------------------------- push mode

// Mail for the hearers of sender i: one bit per agent (one atomicOr per distinct 64-agent word).
// The atomic returns the word's previous bits: a hearer whose bit was clear gets from[r] = i (its
// only sender so far); one whose bit was already set gets its `multi` bit (several senders: it
// walks its row).  (Plain byte marks were tried: the scan of 1-byte marks dirtied by scattered
// byte stores costs 5x the 64-bit bitmap's, more than the atomics save.)
struct Mail {
    unsigned long long *bits, *multi;
    int32_t *from;
};

// Up to kFlush word runs of one sender at once: every returning atomic in flight before the first
// result is used (one after the other, a sender's ~3 words cost ~3 atomic round trips).
constexpr int kFlush = 4;

__device__ __forceinline__ void mail_flush(const Mail &m, const int32_t *pw, const unsigned long long *pb, int np,
                                           int32_t sender) {
    unsigned long long old[kFlush];
#pragma unroll
    for (int j = 0; j < kFlush; ++j) old[j] = j < np ? atomicOr(&m.bits[pw[j]], pb[j]) : 0ull;
#pragma unroll
    for (int j = 0; j < kFlush; ++j) {
        if (j >= np) break;
        const unsigned long long dup = old[j] & pb[j];
        if (dup) atomicOr(&m.multi[pw[j]], dup);
        unsigned long long fresh = pb[j] & ~old[j];
        while (fresh) {
            const int q = __ffsll((long long)fresh) - 1;
            fresh &= fresh - 1;
            m.from[int64_t(pw[j]) * 64 + q] = sender;
        }
    }
}

__device__ __forceinline__ void mail_hearers(int32_t b, int32_t e, const int32_t *__restrict__ tcol, const Mail &m,
                                             int32_t sender) {
    int32_t w = -1, pw[kFlush];
    unsigned long long bits = 0, pb[kFlush];
    int np = 0;
    for (int32_t k0 = b; k0 < e; k0 += kRecv) {
        int32_t rr[kRecv];  // all hearer loads of the chunk in flight
#pragma unroll
        for (int u = 0; u < kRecv; ++u) rr[u] = k0 + u < e ? tcol[k0 + u] : -1;
#pragma unroll
        for (int u = 0; u < kRecv; ++u) {
            const int32_t r = rr[u];
            if (r < 0) continue;
            if ((r >> 6) != w) {
                if (bits) {
                    if (np == kFlush) {
                        mail_flush(m, pw, pb, np, sender);
                        np = 0;
                    }
                    pw[np] = w;
                    pb[np++] = bits;
                }
                w = r >> 6;
                bits = 0;
            }
            bits |= 1ull << (r & 63);
        }
    }
    if (bits) {
        if (np == kFlush) {
            mail_flush(m, pw, pb, np, sender);
            np = 0;
        }
        pw[np] = w;
        pb[np++] = bits;
    }
    if (np) mail_flush(m, pw, pb, np, sender);
}

// Resumed run: mail for the receivers of tick t0's sends.
__global__ __launch_bounds__(kBlock) void k_mail_from_outbox(int64_t n, const uint8_t *__restrict__ ob,
                                                            const int32_t *__restrict__ trp,
                                                            const int32_t *__restrict__ tcol, Mail m) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock)
        if (ob[i]) mail_hearers(trp[i], trp[i + 1], tcol, m, int32_t(i));
}

// One launch per tick for receive + timers (push mode), its workgroups in two roles that run side
// by side: the receivers' short dependent chains overlap the sweep's streaming instead of following
// it.  (A single role -- each sweep wave serving its own receivers -- held every wave for its
// receivers' chains: 0.170 vs 0.152 ms per tick with separate kernels.)
//   sweep    (workgroups g_recv ..): kSweepV consecutive agents per thread, their byte fields
//            (outbox) as one 32-bit word, their flag words as one 16-byte load, their timers (last_hb) and
//            their 64-agent mail word loaded up front; agents with a mail bit are left to the
//            receive role, the others tick their timers.
//   receive  (workgroups 0 .. g_recv - 1; all of them on a pulled tick): chunks of 4 096 agents;
//            the chunk's receivers (mail bit set; on a pulled tick every agent) are listed in LDS
//            and served one per thread -- its one sender directly (from[]), or its CSR row in
//            order when it has several (multi bit) or the tick is pulled -- then its timers run on
//            the result.
// Senders of both roles are listed in the workgroup's own segment, then mailed by it.
// (kSweepV, kRecvChunk: tick_segments.h, with the arithmetic of the grid and the segment capacities.)
static_assert(kTickBlock == kBlock, "tick_segments.h sizes the segments for kBlock threads");

// Sender segments of k_tick's workgroups (each mails its own): the g_recv receive-role ones first
// (rcap entries each: their chunks' agents), then the sweep-role ones (scap each: their agents, or
// their chunks' on a pulled tick, when every workgroup receives).  Sized by tick_shape (tick_segments.h).
struct Segs {
    int32_t *base;
    int64_t rcap, scap;
    int g_recv;
    __device__ __forceinline__ int32_t *of(int b) const {
        return b < g_recv ? base + int64_t(b) * rcap : base + int64_t(g_recv) * rcap + int64_t(b - g_recv) * scap;
    }
};

// Exclusive prefix over the workgroup of c (0 <= c < 2^B) and the total (every thread gets it).
template <int B>
__device__ __forceinline__ int block_excl_scan(int c, int &total, int *s_wave) {
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    int ex = 0, tot = 0;
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const unsigned long long m = __ballot((c >> b) & 1);
        ex += int(__builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u))) << b;
        tot += __popcll(m) << b;
    }
    if (lane == 0) s_wave[wid] = tot;
    __syncthreads();
    int off = 0, all = 0;
#pragma unroll
    for (int q = 0; q < kBlock / kWave; ++q) {
        off += q < wid ? s_wave[q] : 0;
        all += s_wave[q];
    }
    __syncthreads();  // s_wave read by all
    total = all;
    return off + ex;
}

// k_tick's own mail: once a workgroup's agents are done it mails the hearers of the senders it
// listed, into tick t+1's words; the words are rotated over three buffers (tick t reads buf(t),
// mails into buf(t+1) and clears buf(t+2), read in tick t-1 and next mailed in tick t+1) and the
// single-sender slots over two, so no workgroup of tick t touches what another one still reads.
// Storms are decided per workgroup: more senders than frac x the agents of its share -> it mails
// nothing and flags tick t+1 as pulled.  (Round 4's separate k_mail launch after k_tick, deciding
// on the tick's total senders: 0.128 against 0.123 ms per tick, same box.)
struct NextMail {
    Mail next;                       // tick t+1's words and single-sender slots
    unsigned long long *clear;       // buf(t+2), n_clear words
    int64_t n_clear;
    unsigned *pull_next, *pull_clear;
    double frac;                     // < 0: never a storm
    const int32_t *trp, *tcol;       // who hears each agent
    int64_t clk_t0;                  // SWARM_TICK_CLOCKS: the run's first tick
};

// k_tick's agent: settle_agent, its outbox byte written when it differs from the slot's (prev: tick t-2's),
// its sends listed.
__device__ __forceinline__ void finish_agent(int64_t i, Heard &h, uint2 r0, uint32_t bits, int32_t y, uint8_t prev,
                                             int64_t t, double now, double timeout, double jitter, uint64_t seed,
                                             const int32_t *__restrict__ ids, const Fsm &f,
                                             uint8_t *__restrict__ ob_out, int32_t *seg, int *s_ns, TickCounts &c) {
    const uint8_t ob = settle_agent(i, h, r0, bits, y, t, now, timeout, jitter, seed, ids, f, c);
    if (ob != prev) ob_out[i] = ob;
    if (ob) seg[atomicAdd(s_ns, 1)] = int32_t(i);  // this workgroup's sender segment (LDS counter)
}

// k_tick at >= 7 waves per SIMD (72 VGPRs, a few spilled): 0.1111 ms per tick against 0.1142 at 6 (79 VGPRs)
// and 0.1194 at the compiler's 5 (82), 0.129 at 8 (64 VGPRs, 26 spilled); 6 row entries per chunk at 7
// waves 0.1110-0.1116, 4 entries 0.1181 at 7 / 0.1156 at 8 (same box; SWARM_TICK_WAVES=0: the compiler's
// choice, A/B aid)
#ifndef SWARM_TICK_WAVES
#define SWARM_TICK_WAVES 7
#endif
// Experiment aid (A/B builds with -DSWARM_TICK_CLOCKS=1): per tick and workgroup, the 100 MHz wall clock
// at its start, after its role's work (all threads: add_counts' barrier), after its storm decision and at
// its end, plus its sender count; written to SWARM_TICK_CLOCKS_FILE after the run.
#ifndef SWARM_TICK_CLOCKS
#define SWARM_TICK_CLOCKS 0
#endif
#if SWARM_TICK_CLOCKS
__device__ unsigned long long *g_tick_clk;
#define TICK_CLK(slot, v)                                                                        \
    do {                                                                                          \
        if (threadIdx.x == 0 && g_tick_clk)                                                       \
            g_tick_clk[((t - 1 - clk_t0) * int64_t(gridDim.x) + blockIdx.x) * 5 + (slot)] = (v);  \
    } while (0)
#else
#define TICK_CLK(slot, v) \
    do {                  \
    } while (0)
#endif
#if SWARM_TICK_WAVES
#define SWARM_TICK_BOUNDS __launch_bounds__(kBlock, SWARM_TICK_WAVES)
#else
#define SWARM_TICK_BOUNDS __launch_bounds__(kBlock)
#endif
__global__ SWARM_TICK_BOUNDS void k_tick(int64_t n, int64_t t, const int32_t *__restrict__ ids,
                                                const double2 *__restrict__ pos, const int32_t *__restrict__ rp,
                                                const int32_t *__restrict__ col,
                                                Fsm f, Mail mail, const uint8_t *__restrict__ ob_in,
                                                uint8_t *__restrict__ ob_out, const unsigned *__restrict__ pull,
                                                Segs segs, double dt, double timeout,
                                                double jitter, uint64_t seed, unsigned long long *__restrict__ counts,
                                                int vec, unsigned long long *__restrict__ tr, NextMail im, int xg) {
    __shared__ unsigned s_cnt[4];
    __shared__ int s_ns;
    __shared__ int s_wave[kBlock / kWave];
    __shared__ uint32_t s_list[kRecvChunk];  // receive role: the chunk's receivers (agent | multi bit 31)
    static_assert(kRecvChunk % kBlock == 0 && kRecvChunk / kBlock <= 16, "receive slice: <= 16 bits of a word");
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_ns = 0;
#if SWARM_TICK_CLOCKS
    const int64_t clk_t0 = im.clk_t0;
#endif
    TICK_CLK(0, wall_clock64());
    __syncthreads();
#ifndef SWARM_SWEEP_FIRST  // A/B aid: the sweep role's workgroups dispatched before the receive role's
#define SWARM_SWEEP_FIRST 0
#endif
    // the workgroup's place in the role order (receive role first)
    const int lb = SWARM_SWEEP_FIRST ? (int(blockIdx.x) < int(gridDim.x) - segs.g_recv
                                            ? int(blockIdx.x) + segs.g_recv
                                            : int(blockIdx.x) - (int(gridDim.x) - segs.g_recv))
                                     : int(blockIdx.x);
    int32_t *seg = segs.of(lb);
    const int g_recv = segs.g_recv;
    // receive-role workgroups first: dispatched first, all their chains in flight at once (every
    // R-th workgroup instead, the roles side by side: 0.151 vs 0.138 ms per tick)
    const bool recv_role = lb < g_recv;
    const int rank = recv_role ? lb : lb - g_recv;
    const double now = double(t) * dt;
    const bool pulled = *pull != 0;
    TickCounts c;
    int64_t span = 0;  // agents of this workgroup's share (the storm rule)
    if (pulled || recv_role) {
        // ---- receive role
        // a pulled tick: every workgroup, 1 024-agent units (every agent walks its row: 4x the units,
        // a quarter of the row walks one after the other per thread)
        const int64_t nrole = pulled ? int64_t(gridDim.x) : int64_t(g_recv);
        const int kPerT = pulled ? kRecvChunk / 4 / kBlock : kRecvChunk / kBlock;  // agents per thread
        const int64_t unit = int64_t(kPerT) * kBlock;
        const int64_t nchunks = (n + unit - 1) / unit;
        // xg > 0: groups of xg chunks (4 xg units on a pulled tick) dealt round robin to the 8 XCDs
        // (workgroup r runs on XCD r % 8 under round-robin dispatch), so a receiver's neighbours -- in the
        // chunks around its own -- are mostly fetched into the L2 of the XCD that serves it
        const int64_t me = pulled ? int64_t(lb) : int64_t(rank);
        const int64_t gsz = pulled ? 4 * int64_t(xg) : int64_t(xg);
        const int64_t nl = nrole / 8, xcd = me % 8, l = me / 8;
        for (int64_t q = xg ? l : me;; q += xg ? nl : nrole) {
            int64_t ck = q;
            if (xg) {
                const int64_t gi = xcd + 8 * (q / gsz);
                if (gi * gsz >= nchunks) break;
                ck = gi * gsz + q % gsz;
                if (ck >= nchunks) continue;
            } else if (ck >= nchunks) {
                break;
            }
            span += unit;
            // thread: kPerT agents, a slice of mail word (ck * unit + threadIdx.x * kPerT) / 64
            const int64_t a0 = ck * unit + int64_t(threadIdx.x) * kPerT;
            unsigned b16 = 0, m16 = 0;
            if (a0 < n) {
                const unsigned valid = n - a0 >= kPerT ? (1u << kPerT) - 1u : ((1u << (n - a0)) - 1u);
                if (pulled) {
                    b16 = valid;  // every agent (the dead ones clear their outbox)
                    m16 = valid;
                } else {
                    const int64_t w = a0 >> 6;
                    const int sh = int(a0 & 63);
                    b16 = unsigned(mail.bits[w] >> sh) & valid;
                    if (b16) m16 = unsigned(mail.multi[w] >> sh) & b16;
                }
            }
            int total;
            int pos_ = block_excl_scan<5>(__popc(b16), total, s_wave);
            while (b16) {
                const int q = __ffs(b16) - 1;
                b16 &= b16 - 1;
                s_list[pos_++] = uint32_t(a0 + q) | (((m16 >> q) & 1u) ? 0x80000000u : 0u);
            }
            __syncthreads();
            for (int q = threadIdx.x; q < total; q += kBlock) {
                const uint32_t entry = s_list[q];
                const int64_t i = int32_t(entry & 0x7FFFFFFFu);
                const bool multi = (entry & 0x80000000u) != 0;
                // the receiver's fields and its single sender, all loads at once (no load behind the
                // alive test), then the sender's outbox, ID and position at once
                const uint8_t prev = ob_out[i];
                const uint2 r = f.rec[i];
                const int32_t me = ids[i];
                const int32_t j = multi ? 0 : mail.from[i];
                if (!fw_alive(r.x)) {
                    if (prev) ob_out[i] = 0;
                    continue;
                }
                Heard h{fw_state(r.x), 0, false, false, 0, -1};
                uint32_t bits = fw_bits(r.x);
                int32_t y = int32_t(r.y);
                const bool hb_tick = ((t + fw_phase(r.x)) % 10) == 0;
                if (multi) {  // several senders (or a pull): the row, in CSR order
                    const int32_t b = rp[i], e = rp[i + 1];
                    receive_row<kRecvTick>(b, e, col, ob_in, ids, me, hb_tick, h);
                    ++c.multi;
                    c.edges += unsigned(e - b);
                    apply_heard(i, h, t, pos, f, bits, y);
                } else {  // exactly one sender: no row walk
                    const uint8_t o = ob_in[j] & (kAcclaim | kHeartbeat);
                    const int32_t sid = ids[j];
                    const double2 sp = pos[j];  // used when its heartbeat is accepted (hb_from = j)
                    if (o) hear(h, o, sid, j, me, hb_tick);
                    ++c.single;
                    if (h.live) {
                        y = int32_t(t - f.t0);
                        bits = (bits & ~kH64) | kDirty;
                    }
                    if (h.hb_from >= 0) {
                        set_lpos(f, i, float(sp.x), float(sp.y));
                        bits |= kHL;
                    }
                }
                finish_agent(i, h, r, bits, y, prev, t, now, timeout, jitter, seed, ids, f, ob_out, seg, &s_ns, c);
            }
            __syncthreads();  // the list is reused
        }
    } else {
        // ---- sweep role
        const int64_t ngroups = (n + kSweepV - 1) / kSweepV;
        const int64_t stride = int64_t(int(gridDim.x) - g_recv) * kBlock;
        {  // the workgroup's groups (uniform)
            const int64_t g0 = int64_t(rank) * kBlock;
            span = g0 < ngroups ? ((ngroups - g0 + stride - 1) / stride) * kBlock * kSweepV : 0;
        }
        for (int64_t gi = int64_t(rank) * kBlock + threadIdx.x; gi < ngroups; gi += stride) {
            const int64_t i0 = gi * kSweepV;
            const bool full = vec && i0 + kSweepV <= n;
            uint2 rv[kSweepV];
            uint8_t pv[kSweepV];
            const unsigned mine = unsigned(mail.bits[i0 >> 6] >> (i0 & 63)) & ((1u << kSweepV) - 1u);
            if (full) {  // vec: the host checked the outbox's alignment; i0 is a multiple of 4 (records: scratch)
#pragma unroll
                for (int q = 0; q < kSweepV / 2; ++q) {
                    const uint4 r2 = *reinterpret_cast<const uint4 *>(f.rec + i0 + 2 * q);
                    rv[2 * q] = make_uint2(r2.x, r2.y);
                    rv[2 * q + 1] = make_uint2(r2.z, r2.w);
                }
#pragma unroll
                for (int q = 0; q < kSweepV / 4; ++q) {
                    const uint32_t wp = *reinterpret_cast<const uint32_t *>(ob_out + i0 + 4 * q);
#pragma unroll
                    for (int v = 0; v < 4; ++v) pv[4 * q + v] = uint8_t(wp >> (8 * v));
                }
            } else {
#pragma unroll
                for (int v = 0; v < kSweepV; ++v) {
                    const int64_t i = i0 + v < n ? i0 + v : n - 1;
                    rv[v] = i0 + v < n ? f.rec[i] : make_uint2(0u, 0u);  // past n: not alive
                    pv[v] = ob_out[i];
                }
            }
#pragma unroll
            for (int v = 0; v < kSweepV; ++v) {
                const int64_t i = i0 + v;
                if ((mine >> v) & 1u) continue;  // a receiver: the receive role's
                const uint8_t prev = pv[v];      // this slot's byte from tick t-2
                if (!fw_alive(rv[v].x)) {
                    if (i < n && prev) ob_out[i] = 0;
                    continue;
                }
                Heard h{fw_state(rv[v].x), 0, false, false, 0, -1};
                finish_agent(i, h, rv[v], fw_bits(rv[v].x), int32_t(rv[v].y), prev, t, now, timeout, jitter, seed,
                             ids, f, ob_out, seg, &s_ns, c);
            }
        }
    }
    if (tr) {
        add_traffic(tr, pulled ? 5 : 0, pulled ? 0ull : c.single);
        add_traffic(tr, pulled ? 6 : 1, c.multi);
        add_traffic(tr, 2, c.edges);
        if (pulled && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&tr[7], 1ull);  // pulled ticks
    }
    add_counts(c.lead, c.wait, c.acc, c.hb, s_cnt, counts);  // (ends with a barrier: s_ns is final)
    TICK_CLK(1, wall_clock64());
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < im.n_clear; q += int64_t(gridDim.x) * kBlock)
        if (im.clear[q]) im.clear[q] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) *im.pull_clear = 0;
    const int ns = s_ns;
    TICK_CLK(4, (unsigned long long)ns | ((unsigned long long)recv_role << 40) | ((unsigned long long)pulled << 41));
    TICK_CLK(2, wall_clock64());
    if (im.frac >= 0.0 && double(ns) > im.frac * double(span)) {
        if (threadIdx.x == 0) *im.pull_next = 1u;
        TICK_CLK(3, wall_clock64());
        return;
    }
    // the segment was written by this workgroup's threads before add_counts' barrier
    unsigned long long c_edges = 0;
    for (int q = threadIdx.x; q < ns; q += kBlock) {
        const int32_t i = seg[q];
        const int32_t b = im.trp[i], e = im.trp[i + 1];
        mail_hearers(b, e, im.tcol, im.next, i);
        c_edges += uint64_t(e - b);
    }
    if (tr) {
        add_traffic(tr, 3, threadIdx.x < unsigned(ns) ? uint64_t((ns - int(threadIdx.x) + kBlock - 1) / kBlock) : 0ull);
        add_traffic(tr, 4, c_edges);
    }
#if SWARM_TICK_CLOCKS
    __syncthreads();
#endif
    TICK_CLK(3, wall_clock64());
}

// traffic shards -> out[kTraffic]
__global__ void k_sum_traffic(const unsigned long long *__restrict__ tr, unsigned long long *__restrict__ out) {
    if (threadIdx.x < kTraffic) {
        unsigned long long v = 0;
        for (int sh = 0; sh < kShards; ++sh) v += tr[sh * kTraffic + threadIdx.x];
        out[threadIdx.x] = v;
    }
}

// ---------------------------------------------------------------- coupled update loop (contract U1)
// The physics half of swarm_update_loop: the positions double-buffered over the caller's two arrays (cur =
// P_{t-1}, lag = P_{t-2} at the start of tick t; the tick's heartbeats read lag, its physics step reads cur
// and writes lag, then the roles swap), the rest k_physics_loop's arguments.
struct LoopArgs {
    double *pos, *pos_prev;
    double *vel, *target;
    uint8_t *has_target;
    int64_t m;
    const double *obstacles;
    const int32_t *sense_rp, *sense_col;
    double max_speed;
    double *trace;  // frames x n x 2, or NULL
    int32_t trace_every;
    int64_t *n_singular;  // host, may be NULL
    double sense_radius;  // > 0: contract U1-S, every tick senses its neighbours (sense_rp / sense_col unused)
    int64_t *refused_tick;  // U1-S; host, may be NULL
    double radio_radius;    // > 0: contract U1-R, every tick senses who hears whom as well (no message graph)
};

// dst <- src (bytes) when a tick of the sensed loop was refused (st[0] != 0), else nothing: the entry
// snapshot of one caller array put back, on the device, so that the call needs no host wait to decide.
__global__ __launch_bounds__(kBlock) void k_restore_refused(const unsigned long long *__restrict__ st,
                                                           uint8_t *__restrict__ dst,
                                                           const uint8_t *__restrict__ src, size_t bytes) {
    if (st[0] == 0) return;
    const size_t stride = size_t(gridDim.x) * kBlock, first = size_t(blockIdx.x) * kBlock + threadIdx.x;
    size_t done = 0;
    if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 7) == 0) {
        const size_t words = bytes / 8;
        unsigned long long *d = reinterpret_cast<unsigned long long *>(dst);
        const unsigned long long *q = reinterpret_cast<const unsigned long long *>(src);
        for (size_t w = first; w < words; w += stride) d[w] = q[w];
        done = words * 8;
    }
    for (size_t b = done + first; b < bytes; b += stride) dst[b] = src[b];
}

// a <-> b, element-wise (an odd number of ticks leaves the newest positions in the caller's pos_prev)
__global__ __launch_bounds__(kBlock) void k_swap_positions(int64_t n, double2 *__restrict__ a, double2 *__restrict__ b) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
        const double2 p = a[i], q = b[i];
        a[i] = q;
        b[i] = p;
    }
}

// ---------------------------------------------------------------- radio update loop (contract U1-R)
// The tick's receive without a message graph: alive agent i hears j != i iff dx * dx + dy * dy <= r2 on the
// tick's snapshot (swarm_build_rgg's rule), the heard senders' packets handled in ascending storage index (a
// swarm_build_rgg row's order).  The snapshot's binning and cell-sorted copy are the sensed loop's
// (loop_sense_tick); next to them a cell-sorted copy of the inbound outbox (1 byte per agent: a candidate
// costs a streamed byte, not a gather) and one byte per cell, set when the cell holds a sender.
struct Radio {
    Grid g;
    double r2;                         // radio_radius squared
    const int32_t *sorted;             // the tick's binning (LoopSense)
    const uint32_t *off;
    const double2 *psort;
    uint8_t *ob_sorted;                // ob_sorted[q] = ob_in[sorted[q]]
    uint8_t *cell_send;                // [ncx * ncy], cleared per tick
    const unsigned long long *st;      // the call's verdict word: != 0, a tick was refused
};

// The outbox pass of both window loops.  U1-R (kTasks false): `in` is the inbound outbox, one cell plane.
// U1-T: `in` is the inbound sender bytes (TaskTick::sb_in, below) -- the outbox bits plus kClaim / kConflict,
// "the sender claimed", "the sender sent a conflict" -- and a cell plane for each of the three kinds of sender.
template <bool kTasks>
__global__ __launch_bounds__(kBlock) void k_radio_outbox(int64_t n, const uint8_t *__restrict__ in, Radio w,
                                                        uint8_t *__restrict__ cell_claim,
                                                        uint8_t *__restrict__ cell_conf) {
    if (w.st[0] != 0) return;
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < n; q += int64_t(gridDim.x) * kBlock) {
        const uint8_t o = kTasks ? in[w.sorted[q]] : in[w.sorted[q]] & (kAcclaim | kHeartbeat);
        const uint8_t fsm = o & (kAcclaim | kHeartbeat);
        const bool cl = kTasks && (o & kClaim) != 0, cf = kTasks && (o & kConflict) != 0;
        w.ob_sorted[q] = o;
        if (o) {  // (every writer of a cell's byte stores the same 1)
            const double2 p = w.psort[q];
            const int64_t cx = cell_coord(p.x, w.g.xmin, w.g.inv_cell, w.g.ncx);
            const int64_t cy = cell_coord(p.y, w.g.ymin, w.g.inv_cell, w.g.ncy);
            const int64_t c = cy * w.g.ncx + cx;
            if (fsm) w.cell_send[c] = 1;
            if (cl) cell_claim[c] = 1;
            if (cf) cell_conf[c] = 1;
        }
    }
}

// The window receive of both window loops: everything alive agent i (at p, storage index i) hears on the
// tick's snapshot, the Rc predicate on the cell-sorted copy, the heard senders handed to `sender(o, sid, j)`
// -- sorted outbox byte, ID, storage index -- in ascending storage index; ids[j] is gathered only for a
// candidate that sent and is in range.  `flag(cell)`: whether the receiver listens to anything cell `cell`
// holds (a cell plane's byte, or several OR-ed); `rel`: the bits of a sorted outbox byte it listens to.
// Three ways through, all exact:
//   skip    a receiver whose nine cells hold no such sender hears nothing;
//   few     otherwise it scans the outbox bytes of the flagged cells only and keeps the heard senders' indices
//           in a sorted register list of kHeardFast entries -- heartbeats come every tenth own tick from
//           leaders only, so a window mostly holds one or two senders -- and handles them in ascending index;
//   merge   when more senders are heard than the list holds, or more than kHeardCells of the nine cells hold
//           senders (an election storm, a dense block), the window is walked by the nine-way merge of
//           window_merge.h, every candidate in ascending index.
// (The merge for every receiver with a flagged cell: 0.92 ms per tick at 10M agents against 0.64 in this form;
// the list alone, a crowded window scanned first and merged after: 0.69.  DESIGN 4h.)
constexpr int kHeardFast = 4;
constexpr int kHeardCells = 4;  // more window cells than this hold senders: no scan, the merge at once
template <class Flag, class Sender>
__device__ __forceinline__ void hear_window(double2 p, int64_t i, const Radio &w, uint8_t rel,
                                            const int32_t *__restrict__ ids, Flag &&flag, Sender &&sender) {
    const int64_t cx = cell_coord(p.x, w.g.xmin, w.g.inv_cell, w.g.ncx);
    const int64_t cy = cell_coord(p.y, w.g.ymin, w.g.inv_cell, w.g.ncy);
    unsigned cells = 0;  // bit k: window cell k holds a sender this receiver listens to (the bytes loaded at once)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const WindowCell c = window_cell(w.g, cx, cy, k);
        // (loaded ahead of the test: as `c.in && flag(c.at)` the nine loads wait for one another, and
        // update_loop_radio takes 4.02 ms per tick for 3.98 at 10M agents)
        const uint8_t fl = flag(c.at);
        cells |= c.in && fl ? 1u << k : 0u;
    }
    if (!cells) return;
    // senders all around (an election storm): the list would overflow, merge at once
    const bool crowded = __popc(cells) > kHeardCells;
    // the heard senders of the flagged cells, the kHeardFast lowest indices kept in ascending order (an
    // insertion network on registers); one more than fit: the window is merged instead
    int32_t sj[kHeardFast];
    uint8_t so[kHeardFast];
#pragma unroll
    for (int u = 0; u < kHeardFast; ++u) {
        sj[u] = kMergeEnd;
        so[u] = 0;
    }
    bool more = crowded;
    for (int k = 0; k < 9 && !crowded; ++k) {
        if (!((cells >> k) & 1u)) continue;
        const int64_t c = window_cell(w.g, cx, cy, k).at;
        for (uint32_t q = w.off[c], e = w.off[c + 1]; q < e; ++q) {
            uint8_t o = w.ob_sorted[q] & rel;
            if (!o) continue;
            int32_t j = w.sorted[q];
            const double2 s = w.psort[q];
            const double ex = p.x - s.x, ey = p.y - s.y;
            if (j == int32_t(i) || !(ex * ex + ey * ey <= w.r2)) continue;
#pragma unroll
            for (int u = 0; u < kHeardFast; ++u) {
                const bool lower = j < sj[u];
                const int32_t tj = sj[u];
                const uint8_t to = so[u];
                sj[u] = lower ? j : tj;
                so[u] = lower ? o : to;
                j = lower ? tj : j;
                o = lower ? to : o;
            }
            more |= j != kMergeEnd;  // an index fell off the end of the list
        }
    }
    if (!more) {
        int32_t ss[kHeardFast];  // the senders' IDs, all loads in flight
#pragma unroll
        for (int u = 0; u < kHeardFast; ++u) ss[u] = sj[u] != kMergeEnd ? ids[sj[u]] : 0;
#pragma unroll
        for (int u = 0; u < kHeardFast; ++u)
            if (sj[u] != kMergeEnd) sender(so[u], ss[u], sj[u]);
    } else {
        window_merge(p.x, p.y, w.g, w.sorted, w.off, [&](int32_t j, uint32_t q) {
            const uint8_t o = w.ob_sorted[q] & rel;
            if (!o || j == int32_t(i)) return;
            const double2 s = w.psort[q];
            const double ex = p.x - s.x, ey = p.y - s.y;
            if (ex * ex + ey * ey <= w.r2) sender(o, ids[j], j);
        });
    }
}

// k_tick_pull's agent over the window: threads in cell-sorted order (a wave's lanes share their windows and
// the nine sender bytes; the records are gathered by storage index), the row walk replaced by hear_window.
// Returns at once when a tick of the call was refused (the caller restores every array).  Over a lossy channel
// hear_window's `sender` judges the link first, counts it, and returns when it is dropped.
template <class Ch>
__global__ __launch_bounds__(kBlock) void k_tick_radio(int64_t n, int64_t t, const int32_t *__restrict__ ids,
                                                      const double2 *__restrict__ pos, Fsm f, Radio w,
                                                      uint8_t *__restrict__ ob_out, double dt, double timeout,
                                                      double jitter, uint64_t seed,
                                                      unsigned long long *__restrict__ counts, Ch ch) {
    __shared__ unsigned s_cnt[4], s_lcnt[Ch::kLossy ? 4 : 1];
    if (w.st[0] != 0) return;  // uniform over the grid: written by an earlier kernel of the stream
    if (threadIdx.x < 4) {
        s_cnt[threadIdx.x] = 0;
        if constexpr (Ch::kLossy) s_lcnt[threadIdx.x] = 0;
    }
    __syncthreads();
    const double now = double(t) * dt;
    TickCounts c;
    unsigned links = 0, lost = 0;
    for (int64_t q0 = int64_t(blockIdx.x) * kBlock + threadIdx.x; q0 < n; q0 += int64_t(gridDim.x) * kBlock) {
        const int64_t i = w.sorted[q0];
        const uint2 r = f.rec[i];
        if (!fw_alive(r.x)) {
            ob_out[i] = 0;
            continue;
        }
        const double2 p = w.psort[q0];
        const int32_t me = ids[i];
        const bool hb_tick = ((t + fw_phase(r.x)) % 10) == 0;
        uint32_t bits = fw_bits(r.x);
        int32_t y = int32_t(r.y);
        Heard h{fw_state(r.x), 0, false, false, 0, -1};
        // (0xFF, not the two outbox bits: the pass wrote the byte masked, the `&` folds away)
        hear_window(p, i, w, 0xFF, ids, [&](int64_t cell) { return w.cell_send[cell]; },
                    [&](uint8_t o, int32_t sid, int32_t j) {
                        if constexpr (Ch::kLossy) {
                            const bool drop = ch.dropped(t, sid, me);
                            ++links;  // every sender of this window sent an election packet
                            lost += drop;
                            if (drop) return;
                        }
                        hear(h, o, sid, j, me, hb_tick);
                    });
        apply_heard(i, h, t, pos, f, bits, y);
        ob_out[i] = settle_agent(i, h, r, bits, y, t, now, timeout, jitter, seed, ids, f, c);
    }
    add_counts(c.lead, c.wait, c.acc, c.hb, s_cnt, counts);
    if constexpr (Ch::kLossy) add_counts(links, lost, 0u, 0u, s_lcnt, ch.cnt);
}

// ---------------------------------------------------------------- task update loop (contract U1-T)
// U1-R's tick with _process_tasks and the two task handlers (agent.py:292-336), DESIGN 4i.  Per agent: a
// 2-bit status per task (two 64-bit words), its claim table (a dense row of T winners and f32 utilities), and
// by tick parity the set of tasks it claimed and the set it sent a TASK_CONFLICT on.  Three launches per tick,
// the receive and the agent's end shared with U1-R's kernels (hear_window, settle_agent):
//   k_radio_outbox<true>  the outbox pass with two more bits in the cell-sorted byte -- the sender claimed, the
//                         sender sent a conflict -- and a cell byte for each of the three kinds of sender; it
//                         gathers one scratch byte per agent (TaskTick::sb_in), which the tick kernel wrote;
//   k_task_conflicts      the tick's TASK_CONFLICT delivery, before the receive: it writes only the status,
//                         which only the logic step reads, so it commutes with the rest of the receive; and one
//                         bit per (sender, task) is its whole outbox, because the last conflict a leader sent on
//                         a task names the winner its table holds at the end of that tick's receive -- read
//                         here from the sender's row, which no thread of this launch writes;
//   k_tick_radio_tasks    k_tick_radio's agent with the claims of each heard sender handled right after its
//                         election packets (LEADERs only, on both of hear_window's paths), then the timers, then
//                         the claim evaluation of the tasks still OPEN against the board staged in LDS.
// A receiver that is not LEADER at the start of the tick never handles a claim (hear() only ever leaves
// FOLLOWER behind), so it ignores the claim bits and the claim cells (hear_window's `rel` and `flag`): a
// claimer costs the followers around it nothing.
constexpr int kMaxTasks = 64;
constexpr double kClaimThr = 20.0, kHysteresis = 5.0, kUScale = 100.0;
// An OPEN task further than this (squared) is never claimed and never in the guard band: d2 > 25 gives
// sqrt(d2) >= 5 (IEEE sqrt is monotone and sqrt(25) = 5 exactly), so U <= fl(100 / 6) < 17 -- the same d2 the
// utility would take the root of (fp-contract off), so the skip is exact, NaN included (!(NaN <= 25): no
// claim, no guard, as utility() and guard_flag() give).
constexpr double kClaimFar2 = 25.0;

struct TaskTick {
    int32_t T;
    unsigned long long tmask;  // bits 0 .. T-1: a bit past the board in a caller's word is never an index
    const double2 *tpos;
    const int8_t *treq;
    const uint32_t *caps;
    unsigned long long *status_lo, *status_hi;
    const unsigned long long *claim_in, *conflict_in;  // tick t-1's sets
    unsigned long long *claim_out, *conflict_out;      // tick t's
    int32_t *tab_winner;
    float *tab_util;
    uint8_t *cell_claim, *cell_conf;  // as Radio::cell_send: the cell holds a claimer / a conflict sender
    unsigned long long *cnt;          // the tick's kShards x 4: claims sent, handled, conflicts sent, guard pairs
    // The sender bytes (scratch, by tick parity like the outbox): the outbox bits plus kClaim / kConflict when the
    // agent's claim / conflict word of that tick is not empty.  A quiet agent then costs a byte each way instead
    // of its four 64-bit words: the outbox pass gathers this byte alone, and the tick kernel rewrites a word only
    // when it, or the word of two ticks ago in the same slot, holds something.
    const uint8_t *sb_in;  // tick t-1's
    uint8_t *sb_out;       // in: tick t-2's, out: tick t's
};

// The sender bytes of both parities from the caller's outbox and words (once per call).
__global__ __launch_bounds__(kBlock) void k_task_sender_bytes(int64_t n2, const uint8_t *__restrict__ ob,
                                                             const unsigned long long *__restrict__ claim,
                                                             const unsigned long long *__restrict__ conflict,
                                                             unsigned long long tmask, uint8_t *__restrict__ sb) {
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < n2; q += int64_t(gridDim.x) * kBlock)
        sb[q] = uint8_t((ob[q] & (kAcclaim | kHeartbeat)) | ((claim[q] & tmask) ? kClaim : 0) |
                        ((conflict[q] & tmask) ? kConflict : 0));
}

// _handle_task_conflict (327-336) for every alive agent, over the conflict senders it hears, in ascending
// storage index; within a sender ascending task (one message per task is all that matters: the last).  Over a
// lossy channel a conflict sender in range is heard only over a link that tick t keeps -- the verdict the tick
// kernel reaches for the same (t, sender, receiver); the sender's ID is gathered for that alone.  Only then is
// the tick an argument, k_task_conflicts<Lossy, int64_t>: an unused one would move the loss-free kernel's
// argument loads if it came second, and in any later place the lossy kernel is allocated other registers.
template <class Ch, class... Tick>
__global__ __launch_bounds__(kBlock) void k_task_conflicts(int64_t n, Tick... t, const int32_t *__restrict__ ids,
                                                          const uint2 *__restrict__ rec, Radio w, TaskTick k,
                                                          Ch ch) {
    if (w.st[0] != 0) return;
    for (int64_t q0 = int64_t(blockIdx.x) * kBlock + threadIdx.x; q0 < n; q0 += int64_t(gridDim.x) * kBlock) {
        const double2 p = w.psort[q0];
        const int64_t cx = cell_coord(p.x, w.g.xmin, w.g.inv_cell, w.g.ncx);
        const int64_t cy = cell_coord(p.y, w.g.ymin, w.g.inv_cell, w.g.ncy);
        uint8_t any = 0;  // the nine bytes loaded at once
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const int64_t yy = cy + (c / 3) - 1, xx = cx + (c % 3) - 1;
            const bool in = yy >= 0 && yy < w.g.ncy && xx >= 0 && xx < w.g.ncx;
            const uint8_t fl = k.cell_conf[in ? yy * w.g.ncx + xx : 0];
            any |= in ? fl : uint8_t(0);
        }
        if (!any) continue;
        const int64_t i = w.sorted[q0];
        if (!fw_alive(rec[i].x)) continue;
        const int32_t me = ids[i];
        const unsigned long long lo0 = k.status_lo[i], hi0 = k.status_hi[i];
        unsigned long long lo = lo0, hi = hi0;
        window_merge(p.x, p.y, w.g, w.sorted, w.off, [&](int32_t j, uint32_t q) {
            if (!(w.ob_sorted[q] & kConflict) || j == int32_t(i)) return;
            const double2 s = w.psort[q];
            const double ex = p.x - s.x, ey = p.y - s.y;
            if (!(ex * ex + ey * ey <= w.r2)) return;
            if constexpr (Ch::kLossy)
                if (ch.dropped(t..., ids[j], me)) return;
            unsigned long long m = k.conflict_in[j] & k.tmask;
            const int32_t *row = k.tab_winner + int64_t(j) * k.T;
            while (m) {
                const int a = __ffsll((long long)m) - 1;
                m &= m - 1;
                const unsigned long long bit = 1ull << a;
                hi |= bit;  // ASSIGNED (3) for the winner, LOCKED (2) for everyone else
                lo = row[a] == me ? lo | bit : lo & ~bit;
            }
        });
        if (lo != lo0) k.status_lo[i] = lo;
        if (hi != hi0) k.status_hi[i] = hi;
    }
}

// _handle_task_claim (304-325) at a LEADER, for the claims sender j (ID sid) sent during tick t-1: its
// utilities recomputed from the position it claimed at (the lagged buffer) -- the same function of the same
// operands as its own evaluation, bit for bit -- and rounded to the '!f' payload.
struct ClaimRx {
    const unsigned long long *claim_in;
    const double2 *lag;
    const uint32_t *caps;
    int32_t *tw;  // the receiver's table row
    float *tu;
    const double *tx, *ty;  // the board (LDS)
    const int8_t *rq;
    unsigned long long conf;  // tasks it sent a conflict on during this tick
    unsigned handled, sent;
    unsigned long long tmask;
};

__device__ __forceinline__ void hear_claims(ClaimRx &c, int32_t j, int32_t sid) {
    unsigned long long m = c.claim_in[j] & c.tmask;
    if (!m) return;
    const double2 a = c.lag[j];
    const uint32_t cp = c.caps[j];
    while (m) {
        const int t = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float u = float(utility(a.x, a.y, cp, c.tx[t], c.ty[t], c.rq[t], kUScale));
        const int32_t hw = c.tw[t];
        const float hu = c.tu[t];
        ++c.handled;
        if (hw < 0 || double(u) > double(hu) + kHysteresis) {
            c.tw[t] = sid;
            c.tu[t] = u;
            c.conf |= 1ull << t;
            ++c.sent;
        } else if (hw != sid) {  // re-affirm the held winner
            c.conf |= 1ull << t;
            ++c.sent;
        }
    }
}

// The tasks that can be within reach of any lane of the wave (bit k: task k), for all 64 lanes at once: the
// wave's bounding box by shuffles, then lane k judges task k against it.  The box is reduced in f32 (half the
// shuffles) and widened by what the rounding to f32 can have lost, sx >= |x| 2^-24 for every x of the wave.  A
// task is left out only when it lies more than kWaveFar + sx beyond the box on some axis: then for every lane
// tx - x >= tx - xmax > 5.5, so fl(x - tx) < -5.4, its dx * dx > 29 and the far pre-test would skip the task
// anyway -- the mask never changes a result.  Lanes without an agent and non-finite agents pass NaN: fminf /
// fmaxf ignore them, and a NaN agent fails every pre-test by itself.  A wave of NaNs, or one with an agent
// beyond f32's range, keeps every task (the comparisons are false).
constexpr double kWaveFar = 5.5;
constexpr double kNaN = __builtin_nan("");
static_assert(kWave == 64 && kMaxTasks <= kWave, "one lane per task");
__device__ __forceinline__ unsigned long long wave_tasks(double2 p, int T, const double *s_tx, const double *s_ty) {
    float x0 = float(p.x), x1 = x0, y0 = float(p.y), y1 = y0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        x0 = fminf(x0, __shfl_xor(x0, off, 64));
        x1 = fmaxf(x1, __shfl_xor(x1, off, 64));
        y0 = fminf(y0, __shfl_xor(y0, off, 64));
        y1 = fmaxf(y1, __shfl_xor(y1, off, 64));
    }
    const int l = threadIdx.x & (kWave - 1);
    bool keep = false;
    if (l < T) {
        const double tx = s_tx[l], ty = s_ty[l];
        const double fx = kWaveFar + fmax(fabs(double(x0)), fabs(double(x1))) * 0x1p-23;
        const double fy = kWaveFar + fmax(fabs(double(y0)), fabs(double(y1))) * 0x1p-23;
        keep = !(tx - double(x1) > fx || double(x0) - tx > fx || ty - double(y1) > fy || double(y0) - ty > fy);
    }
    return __ballot(keep);
}

// At >= 4 waves per SIMD (128 VGPRs, none spilled): leg (a) of tools/bench_loop_tasks.py 4.28-4.30 ms per tick
// against 4.44-4.46 at the compiler's 3 (138 VGPRs), same session; 5 waves would need scratch (38 VGPRs spilled).
// Over a lossy channel the link is judged before the sender's election packets and claims are handled.
template <class Ch>
__global__ __launch_bounds__(kBlock, 4) void k_tick_radio_tasks(int64_t n, int64_t t, const int32_t *__restrict__ ids,
                                                            const double2 *__restrict__ pos, Fsm f, Radio w,
                                                            uint8_t *__restrict__ ob_out, double dt, double timeout,
                                                            double jitter, uint64_t seed,
                                                            unsigned long long *__restrict__ counts, TaskTick k,
                                                            Ch ch) {
    __shared__ unsigned s_cnt[4], s_tcnt[4], s_lcnt[Ch::kLossy ? 4 : 1];
    __shared__ double s_tx[kMaxTasks], s_ty[kMaxTasks];
    __shared__ int8_t s_rq[kMaxTasks];
    if (w.st[0] != 0) return;  // uniform over the grid: written by an earlier kernel of the stream
    if (threadIdx.x < 4) {
        s_cnt[threadIdx.x] = s_tcnt[threadIdx.x] = 0;
        if constexpr (Ch::kLossy) s_lcnt[threadIdx.x] = 0;
    }
    if (int(threadIdx.x) < k.T) {
        const double2 q = k.tpos[threadIdx.x];
        s_tx[threadIdx.x] = q.x;
        s_ty[threadIdx.x] = q.y;
        s_rq[threadIdx.x] = k.treq[threadIdx.x];
    }
    __syncthreads();
    const double now = double(t) * dt;
    TickCounts c;
    unsigned c_claim = 0, c_guard = 0, links = 0, lost = 0;
    ClaimRx cr{k.claim_in, pos, k.caps, nullptr, nullptr, s_tx, s_ty, s_rq, 0ull, 0u, 0u, k.tmask};
    // (the trip count is uniform over the workgroup: every wave enters wave_tasks with all its lanes)
    for (int64_t base = int64_t(blockIdx.x) * kBlock; base < n; base += int64_t(gridDim.x) * kBlock) {
        const int64_t q0 = base + threadIdx.x;
        const bool valid = q0 < n;
        const double2 p = valid ? w.psort[q0] : make_double2(kNaN, kNaN);
        const unsigned long long reach = wave_tasks(p, k.T, s_tx, s_ty);
        if (!valid) continue;
        const int64_t i = w.sorted[q0];
        const uint2 r = f.rec[i];
        const uint32_t fw = r.x;
        const uint8_t old = k.sb_out[i];  // what this slot's words hold (tick t-2's sends)
        if (!fw_alive(fw)) {
            ob_out[i] = 0;
            if (old & kClaim) k.claim_out[i] = 0;
            if (old & kConflict) k.conflict_out[i] = 0;
            if (old) k.sb_out[i] = 0;
            continue;
        }
        const int32_t me = ids[i];
        const uint8_t st0 = fw_state(fw);
        const bool hb_tick = ((t + fw_phase(fw)) % 10) == 0;
        uint32_t bits = fw_bits(fw);
        int32_t y = int32_t(r.y);
        Heard h{st0, 0, false, false, 0, -1};
        // only a LEADER's walk looks at claims (see the header)
        const bool lead0 = st0 == ST_L;
        const uint8_t rel = uint8_t(kAcclaim | kHeartbeat | (lead0 ? kClaim : 0));
        cr.tw = k.tab_winner + i * k.T;
        cr.tu = k.tab_util + i * k.T;
        cr.conf = 0;
        hear_window(
            p, i, w, rel, ids,
            [&](int64_t cell) { return uint8_t(w.cell_send[cell] | (lead0 ? k.cell_claim[cell] : uint8_t(0))); },
            [&](uint8_t o, int32_t sid, int32_t j) {
                if constexpr (Ch::kLossy) {
                    // (a claim-only sender is no election link; it is dropped all the same)
                    const bool drop = ch.dropped(t, sid, me);
                    const unsigned el = (o & (kAcclaim | kHeartbeat)) != 0;
                    links += el;
                    lost += el & unsigned(drop);
                    if (drop) return;
                }
                hear(h, o, sid, j, me, hb_tick);
                if ((o & kClaim) && h.st == ST_L) hear_claims(cr, j, sid);
            });
        apply_heard(i, h, t, pos, f, bits, y);
        const uint8_t ob = settle_agent(i, h, r, bits, y, t, now, timeout, jitter, seed, ids, f, c);
        ob_out[i] = ob;
        // _process_tasks (292-302): the tasks still OPEN after this tick's conflicts, at the tick's snapshot;
        // the status is read only when a task is near the wave at all
        unsigned long long claims = 0;
        if (reach) {
            const unsigned long long lo = k.status_lo[i];
            unsigned long long open = ~(lo | k.status_hi[i]) & reach;
            const uint32_t cp = k.caps[i];
            while (open) {
                const int a = __ffsll((long long)open) - 1;
                open &= open - 1;
                const double dx = p.x - s_tx[a], dy = p.y - s_ty[a];
                if (!(dx * dx + dy * dy <= kClaimFar2)) continue;
                const double U = utility(p.x, p.y, cp, s_tx[a], s_ty[a], s_rq[a], kUScale);
                c_guard += guard_flag(U, kClaimThr);
                if (U > kClaimThr) claims |= 1ull << a;
            }
            if (claims) k.status_lo[i] = lo | claims;  // TENTATIVE
        }
        if (claims || (old & kClaim)) k.claim_out[i] = claims;
        if (cr.conf || (old & kConflict)) k.conflict_out[i] = cr.conf;
        const uint8_t sent = uint8_t(ob | (claims ? kClaim : 0) | (cr.conf ? kConflict : 0));
        if (sent != old) k.sb_out[i] = sent;
        c_claim += unsigned(__popcll(claims));
    }
    add_counts(c.lead, c.wait, c.acc, c.hb, s_cnt, counts);
    add_counts(c_claim, cr.handled, cr.sent, c_guard, s_tcnt, k.cnt);
    if constexpr (Ch::kLossy) add_counts(links, lost, 0u, 0u, s_lcnt, ch.cnt);
}

// ---------------------------------------------------------------- board update loop (contract U1-B)
// U1-T on a board of up to 2^24 tasks, DESIGN 4m: the same three launches per tick, the per-agent task state in
// sparse rows in global memory instead of bit words and dense tables.  A row is ascending by task with its
// empty slots (-1) behind the last entry, so it has one form whatever order its entries arrived in; a thread
// searches and inserts in its own rows in place and only reads the rows of the senders it hears.
//   status        Ks slots, task << 2 | code (OPEN is never stored);
//   table         Kt slots in three arrays, task / winner / f32 utility;
//   claim / conflict rows by tick parity, Ks / Kt slots of task indices -- written on demand like U1-T's words: a
//                 row is touched only when it, or the row of two ticks ago in the same slot, holds something.
// The board itself is a cell grid over the tasks (task_grid.h): an agent evaluates the tasks of the 3 x 3 task
// cells around it -- three runs of the cell-sorted copy, a row of three cells is contiguous -- against the same
// far pre-test, utility() and guard_flag() as k_tick_radio_tasks; an agent whose three runs are empty reads
// nothing of its status row.  An agent that needs one slot more than a row has sets the call's verdict words
// (st[0] = 1 + tick as a too-dense tick does, st[1] = kind << 32 | agent) and skips the insert: no thread writes
// past a row, every later kernel of the call returns at once, and the caller's arrays are restored.
constexpr int kRowLinear = 4;  // rows of at most this many entries are scanned, longer ones bisected

struct BoardGrid {
    const uint32_t *off;  // ncx * ncy + 1
    const double2 *sxy;   // the tasks' positions in cell-sorted order
    const int2 *sir;      // (task index, treq) in the same order
    double xmin, ymin, xmax, ymax, inv_cell;
    int64_t ncx, ncy;
};

struct BoardTick {
    int32_t Ks, Kt;
    int32_t k;  // the tick of the call, from 0 (the verdict word's)
    const double2 *tpos;  // by task index: the claim handler's
    const int8_t *treq;
    BoardGrid tg;
    const uint32_t *caps;
    int32_t *status;
    int32_t *tab_task, *tab_winner;
    float *tab_util;
    const int32_t *claim_in, *conflict_in;  // tick t-1's rows
    int32_t *claim_out, *conflict_out;      // tick t's
    uint8_t *cell_claim, *cell_conf;        // as TaskTick's
    unsigned long long *cnt;
    const uint8_t *sb_in;  // the sender bytes, as TaskTick's
    uint8_t *sb_out;
    unsigned long long *st;  // the call's verdict words
};

// How many of a row's K slots are taken (the first empty one).
__device__ __forceinline__ int row_count(const int32_t *row, int K) {
    int lo = 0, hi = K;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] >= 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The first of a row's cnt entries whose task (entry >> sh) is not below `task`; cnt when there is none.
__device__ __forceinline__ int row_lower(const int32_t *row, int cnt, int32_t task, int sh) {
    if (cnt <= kRowLinear) {
        int q = 0;
        while (q < cnt && (row[q] >> sh) < task) ++q;
        return q;
    }
    int lo = 0, hi = cnt;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((row[mid] >> sh) < task) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <class V>
__device__ __forceinline__ void row_open(V *row, int cnt, int at) {  // entries [at, cnt) one slot up
    for (int m = cnt; m > at; --m) row[m] = row[m - 1];
}

// `task` into a row of task indices kept as a set (the claim and conflict rows; cnt < K by construction, and
// never a write past the row).
__device__ __forceinline__ void row_set_insert(int32_t *row, int K, int &cnt, int32_t task) {
    const int q = row_lower(row, cnt, task, 0);
    if ((q < cnt && row[q] == task) || cnt >= K) return;
    row_open(row, cnt, q);
    row[q] = task;
    ++cnt;
}

// A status row's entry for `task` set to `code`, inserted when the task was OPEN; false: the row is full.
__device__ __forceinline__ bool status_upsert(int32_t *row, int K, int &cnt, int32_t task, int32_t code) {
    const int q = row_lower(row, cnt, task, 2);
    const int32_t e = (task << 2) | code;
    if (q < cnt && (row[q] >> 2) == task) {
        if (row[q] != e) row[q] = e;
        return true;
    }
    if (cnt >= K) return false;
    row_open(row, cnt, q);
    row[q] = e;
    ++cnt;
    return true;
}

__device__ __forceinline__ void row_clear(int32_t *row, int K) {
    for (int q = 0; q < K && row[q] >= 0; ++q) row[q] = -1;
}

// (every overflowing thread of a tick stores the same st[0]; st[1] is one 64-bit store, any of them may stay)
__device__ __forceinline__ void board_overflow(unsigned long long *st, int32_t k, int kind, int64_t agent) {
    st[1] = (static_cast<unsigned long long>(kind) << 32) | static_cast<unsigned long long>(uint32_t(agent));
    st[0] = 1ull + unsigned(k);
}

// The entry check of one sparse array of `total` slots in rows of K: every slot -1 or a task in [0, T) (with a
// code in 1..3 where sh == 2), every row strictly ascending with the empties last.  bad[0] != 0: it is not.
__global__ __launch_bounds__(kBlock) void k_board_check_rows(int64_t total, int K, int sh, int32_t T,
                                                            const int32_t *__restrict__ a,
                                                            unsigned long long *__restrict__ bad) {
    bool wrong = false;
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < total; q += int64_t(gridDim.x) * kBlock) {
        const int32_t e = a[q];
        if (e == -1) continue;
        if (e < 0 || (e >> sh) >= T || (sh && (e & 3) == 0)) {
            wrong = true;
        } else if (q % K) {
            const int32_t prev = a[q - 1];
            wrong |= prev < 0 || (prev >> sh) >= (e >> sh);
        }
    }
    if (wrong) bad[0] = 1;
}

// The sender bytes of both parities from the caller's outbox and rows (once per call): a row holds something
// iff its first slot does.
__global__ __launch_bounds__(kBlock) void k_board_sender_bytes(int64_t n2, const uint8_t *__restrict__ ob,
                                                              const int32_t *__restrict__ claim, int Ks,
                                                              const int32_t *__restrict__ conflict, int Kt,
                                                              uint8_t *__restrict__ sb) {
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < n2; q += int64_t(gridDim.x) * kBlock)
        sb[q] = uint8_t((ob[q] & (kAcclaim | kHeartbeat)) | (claim[q * Ks] >= 0 ? kClaim : 0) |
                        (conflict[q * Kt] >= 0 ? kConflict : 0));
}

// k_task_conflicts' walk over sparse rows: for every task of a heard sender's conflict row the winner is looked
// up in the sender's table row (no entry: -1, everyone LOCKED) and the receiver's status row upserted; the last
// conflict in walk order decides.  No thread of this launch writes a table or a conflict row.
// The lifetime policy (contract U1-A.3) stands beside the channel policy: on a board with lifetimes a
// conflict about a task absent at this tick writes nothing (agent.py:332, 335: `if task_id in self.tasks`); the
// tick's presence bytes come from the key pass of the board's lists (task_board.hip).
struct NoLife {
    static constexpr bool kLife = false;
};
struct Lifetimes {
    static constexpr bool kLife = true;
    const uint8_t *present;  // by task index, this tick
    __device__ bool absent(int32_t task) const { return present[task] == 0; }
};
// Both policies as one kernel argument: an empty policy takes no room (empty bases), so the NoLife kernels keep
// the argument layout they had with the channel alone.
template <class Ch, class Lf>
struct BoardPolicy : Ch, Lf {};

template <class Ch, class Lf>
__global__ __launch_bounds__(kBlock) void k_board_conflicts(int64_t n, int64_t t, const int32_t *__restrict__ ids,
                                                           const uint2 *__restrict__ rec, Radio w, BoardTick k,
                                                           BoardPolicy<Ch, Lf> pl) {
    if (w.st[0] != 0) return;
    for (int64_t q0 = int64_t(blockIdx.x) * kBlock + threadIdx.x; q0 < n; q0 += int64_t(gridDim.x) * kBlock) {
        const double2 p = w.psort[q0];
        const int64_t cx = cell_coord(p.x, w.g.xmin, w.g.inv_cell, w.g.ncx);
        const int64_t cy = cell_coord(p.y, w.g.ymin, w.g.inv_cell, w.g.ncy);
        uint8_t any = 0;  // the nine bytes loaded at once
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const WindowCell wc = window_cell(w.g, cx, cy, c);
            const uint8_t fl = k.cell_conf[wc.at];
            any |= wc.in ? fl : uint8_t(0);
        }
        if (!any) continue;
        const int64_t i = w.sorted[q0];
        if (!fw_alive(rec[i].x)) continue;
        const int32_t me = ids[i];
        int32_t *srow = k.status + i * k.Ks;
        int ns = -1;  // the status row's entries, counted when the first conflict arrives
        bool over = false;
        window_merge(p.x, p.y, w.g, w.sorted, w.off, [&](int32_t j, uint32_t q) {
            if (!(w.ob_sorted[q] & kConflict) || j == int32_t(i)) return;
            const double2 s = w.psort[q];
            const double ex = p.x - s.x, ey = p.y - s.y;
            if (!(ex * ex + ey * ey <= w.r2)) return;
            if constexpr (Ch::kLossy)
                if (pl.dropped(t, ids[j], me)) return;
            const int32_t *crow = k.conflict_in + int64_t(j) * k.Kt;
            const int32_t *tt = k.tab_task + int64_t(j) * k.Kt;
            const int32_t *tw = k.tab_winner + int64_t(j) * k.Kt;
            if (crow[0] < 0) return;
            const int nt = row_count(tt, k.Kt);
            if (ns < 0) ns = row_count(srow, k.Ks);
            for (int c = 0; c < k.Kt; ++c) {
                const int32_t a = crow[c];
                if (a < 0) break;
                if constexpr (Lf::kLife)
                    if (pl.absent(a)) continue;
                const int at = row_lower(tt, nt, a, 0);
                const int32_t win = at < nt && tt[at] == a ? tw[at] : -1;
                // ASSIGNED (3) for the winner, LOCKED (2) for everyone else
                over |= !status_upsert(srow, k.Ks, ns, a, win == me ? 3 : 2);
            }
        });
        if (over) board_overflow(k.st, k.k, SWARM_BOARD_STATUS, i);
    }
}

// hear_claims over sparse rows: the claims of sender j's row against the receiver's sorted table row, the `>
// held + 5.0` rule and the re-affirmation as there; the tasks it sends a conflict on go into its conflict row.
struct BoardRx {
    const double2 *lag;
    int32_t *tt, *tw;  // the receiver's table row
    float *tu;
    int32_t *cfrow;    // its conflict row of this tick (cleared by the caller)
    int nt, ncf;       // their entries; nt < 0: not counted yet
    unsigned handled, sent;
    bool over;
};

__device__ __forceinline__ void hear_claims_board(BoardRx &c, const BoardTick &k, int32_t j, int32_t sid) {
    const int32_t *crow = k.claim_in + int64_t(j) * k.Ks;
    if (crow[0] < 0) return;
    const double2 a = c.lag[j];
    const uint32_t cp = k.caps[j];
    if (c.nt < 0) c.nt = row_count(c.tt, k.Kt);
    for (int q = 0; q < k.Ks; ++q) {
        const int32_t task = crow[q];
        if (task < 0) break;
        const double2 tp = k.tpos[task];
        const float u = float(utility(a.x, a.y, cp, tp.x, tp.y, k.treq[task], kUScale));
        ++c.handled;
        const int at = row_lower(c.tt, c.nt, task, 0);
        const bool have = at < c.nt && c.tt[at] == task;
        const int32_t hw = have ? c.tw[at] : -1;
        const float hu = have ? c.tu[at] : 0.f;
        if (hw < 0 || double(u) > double(hu) + kHysteresis) {
            if (!have) {
                if (c.nt >= k.Kt) {
                    c.over = true;
                    continue;
                }
                row_open(c.tt, c.nt, at);
                row_open(c.tw, c.nt, at);
                row_open(c.tu, c.nt, at);
                c.tt[at] = task;
                ++c.nt;
            }
            c.tw[at] = sid;
            c.tu[at] = u;
        } else if (hw == sid) {
            continue;
        }  // else: re-affirm the held winner
        ++c.sent;
        row_set_insert(c.cfrow, k.Kt, c.ncf, task);
    }
}

// k_tick_radio_tasks' agent on a board (see the header of this section).  Over a lossy channel the link is
// judged before the sender's election packets and claims are handled.
template <class Ch>
__global__ __launch_bounds__(kBlock) void k_tick_radio_board(int64_t n, int64_t t, const int32_t *__restrict__ ids,
                                                            const double2 *__restrict__ pos, Fsm f, Radio w,
                                                            uint8_t *__restrict__ ob_out, double dt, double timeout,
                                                            double jitter, uint64_t seed,
                                                            unsigned long long *__restrict__ counts, BoardTick k,
                                                            Ch ch) {
    __shared__ unsigned s_cnt[4], s_tcnt[4], s_lcnt[Ch::kLossy ? 4 : 1];
    if (w.st[0] != 0) return;  // uniform over the grid: written by an earlier kernel of the stream
    if (threadIdx.x < 4) {
        s_cnt[threadIdx.x] = s_tcnt[threadIdx.x] = 0;
        if constexpr (Ch::kLossy) s_lcnt[threadIdx.x] = 0;
    }
    __syncthreads();
    const double now = double(t) * dt;
    TickCounts c;
    unsigned c_claim = 0, c_guard = 0, links = 0, lost = 0;
    BoardRx rx{pos, nullptr, nullptr, nullptr, nullptr, -1, 0, 0u, 0u, false};
    for (int64_t q0 = int64_t(blockIdx.x) * kBlock + threadIdx.x; q0 < n; q0 += int64_t(gridDim.x) * kBlock) {
        const double2 p = w.psort[q0];
        const int64_t i = w.sorted[q0];
        const uint2 r = f.rec[i];
        const uint32_t fw = r.x;
        const uint8_t old = k.sb_out[i];  // what this slot's rows hold (tick t-2's sends)
        int32_t *clrow = k.claim_out + i * k.Ks, *cfrow = k.conflict_out + i * k.Kt;
        if (old & kClaim) row_clear(clrow, k.Ks);
        if (old & kConflict) row_clear(cfrow, k.Kt);
        if (!fw_alive(fw)) {
            ob_out[i] = 0;
            if (old) k.sb_out[i] = 0;
            continue;
        }
        const int32_t me = ids[i];
        const uint8_t st0 = fw_state(fw);
        const bool hb_tick = ((t + fw_phase(fw)) % 10) == 0;
        uint32_t bits = fw_bits(fw);
        int32_t y = int32_t(r.y);
        Heard h{st0, 0, false, false, 0, -1};
        // only a LEADER's walk looks at claims (k_tick_radio_tasks' header)
        const bool lead0 = st0 == ST_L;
        const uint8_t rel = uint8_t(kAcclaim | kHeartbeat | (lead0 ? kClaim : 0));
        rx.tt = k.tab_task + i * k.Kt;
        rx.tw = k.tab_winner + i * k.Kt;
        rx.tu = k.tab_util + i * k.Kt;
        rx.cfrow = cfrow;
        rx.nt = -1;
        rx.ncf = 0;
        rx.over = false;
        hear_window(
            p, i, w, rel, ids,
            [&](int64_t cell) { return uint8_t(w.cell_send[cell] | (lead0 ? k.cell_claim[cell] : uint8_t(0))); },
            [&](uint8_t o, int32_t sid, int32_t j) {
                if constexpr (Ch::kLossy) {
                    // (a claim-only sender is no election link; it is dropped all the same)
                    const bool drop = ch.dropped(t, sid, me);
                    const unsigned el = (o & (kAcclaim | kHeartbeat)) != 0;
                    links += el;
                    lost += el & unsigned(drop);
                    if (drop) return;
                }
                hear(h, o, sid, j, me, hb_tick);
                if ((o & kClaim) && h.st == ST_L) hear_claims_board(rx, k, j, sid);
            });
        apply_heard(i, h, t, pos, f, bits, y);
        const uint8_t ob = settle_agent(i, h, r, bits, y, t, now, timeout, jitter, seed, ids, f, c);
        ob_out[i] = ob;
        // _process_tasks (292-302): the tasks still OPEN after this tick's conflicts, at the tick's snapshot,
        // of the three runs of task cells around the agent
        int ncl = 0;
        bool over_s = false;
        const BoardGrid &tg = k.tg;
        const bool outside = p.x < tg.xmin - kTaskOutside || p.x > tg.xmax + kTaskOutside ||
                             p.y < tg.ymin - kTaskOutside || p.y > tg.ymax + kTaskOutside;
        if (!outside) {
            const int64_t tcx = cell_coord(p.x, tg.xmin, tg.inv_cell, tg.ncx);
            const int64_t tcy = cell_coord(p.y, tg.ymin, tg.inv_cell, tg.ncy);
            const int64_t x0 = tcx > 0 ? tcx - 1 : 0, x1 = tcx + 1 < tg.ncx ? tcx + 1 : tg.ncx - 1;
            uint32_t rb[3], re[3];  // the offsets loaded at once
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int64_t yy = tcy + d - 1;
                const bool in = yy >= 0 && yy < tg.ncy;
                const int64_t row0 = in ? yy * tg.ncx : 0;
                const uint32_t b = tg.off[row0 + x0], e = tg.off[row0 + x1 + 1];
                rb[d] = in ? b : 0u;
                re[d] = in ? e : 0u;
            }
            int32_t *srow = k.status + i * k.Ks;
            int ns = -1;  // the status row's entries, counted when the first task passes the pre-test
            uint32_t cp = 0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                for (uint32_t q = rb[d]; q < re[d]; ++q) {
                    const double2 tp = tg.sxy[q];
                    const double dx = p.x - tp.x, dy = p.y - tp.y;
                    if (!(dx * dx + dy * dy <= kClaimFar2)) continue;
                    const int2 ir = tg.sir[q];
                    if (ns < 0) {
                        ns = row_count(srow, k.Ks);
                        cp = k.caps[i];
                    }
                    const int at = row_lower(srow, ns, ir.x, 2);
                    if (at < ns && (srow[at] >> 2) == ir.x) continue;  // not OPEN
                    const double U = utility(p.x, p.y, cp, tp.x, tp.y, ir.y, kUScale);
                    c_guard += guard_flag(U, kClaimThr);
                    if (!(U > kClaimThr)) continue;
                    if (ns >= k.Ks) {
                        over_s = true;
                        continue;
                    }
                    row_open(srow, ns, at);
                    srow[at] = (ir.x << 2) | 1;  // TENTATIVE
                    ++ns;
                    row_set_insert(clrow, k.Ks, ncl, ir.x);
                    ++c_claim;
                }
            }
        }
        if (over_s) board_overflow(k.st, k.k, SWARM_BOARD_STATUS, i);
        if (rx.over) board_overflow(k.st, k.k, SWARM_BOARD_TABLE, i);
        const uint8_t sent = uint8_t(ob | (ncl ? kClaim : 0) | (rx.ncf ? kConflict : 0));
        if (sent != old) k.sb_out[i] = sent;
    }
    add_counts(c.lead, c.wait, c.acc, c.hb, s_cnt, counts);
    add_counts(c_claim, rx.handled, rx.sent, c_guard, s_tcnt, k.cnt);
    if constexpr (Ch::kLossy) add_counts(links, lost, 0u, 0u, s_lcnt, ch.cnt);
}

// ---------------------------------------------------------------- the host loop, in stages
// One run's arguments, as the entry points fill them (`loop`: swarm_update_loop*, each tick then followed
// by its physics step; `pos` is not used then, the heartbeats read the lagged buffer).
struct TickRun {
    swarm_ctx *ctx;
    int64_t n;
    const int32_t *ids;
    const double *pos;
    const int32_t *row_ptr, *col, *hear_row_ptr, *hear_col, *tick_off;
    const swarm_fsm *fsm;
    int64_t t0;
    int32_t ticks;
    double dt, timeout, jitter;
    uint64_t seed;
    const int64_t *kill_ticks;
    int32_t n_kill;
    double pull_frac;
    int64_t *counts, *traffic;
    const LoopArgs *loop;
    void *stream;
    const swarm_tasks *tasks = nullptr;  // U1-T (T > 0: swarm_update_loop_tasks), with its two host outputs
    int64_t *task_counts = nullptr, *n_guard = nullptr;
    const swarm_channel *ch = nullptr;  // U1-L (loss > 0: swarm_update_loop_channel's lossy kernels)
    int64_t *link_counts = nullptr;
    const swarm_board *board = nullptr;  // U1-B (T > 0: swarm_update_loop_board), with its state and overflow info
    const swarm_board_state *bstate = nullptr;
    swarm_board_overflow *overflow = nullptr;
    swarm_board *mboard = nullptr;  // U1-M: `board` again when it moves (its lists advance after every tick)
    bool tasked() const { return tasks && tasks->T > 0; }
    bool boarded() const { return board && board->T > 0; }
    bool lossy() const { return ch && ch->loss > 0.0; }
    bool sensed() const { return loop && loop->sense_radius > 0.0; }
    bool radio() const { return loop && loop->radio_radius > 0.0; }
    bool push() const { return hear_row_ptr != nullptr; }
};

// What one tick's receive launch needs, whatever the mode: the heartbeats' positions (the loops: the lagged
// buffer), tick t-1's sends and tick t's, the tick's kShards x 4 partial counters.
struct Tick {
    int64_t t;
    const double2 *pos;
    const uint8_t *ob_in;
    uint8_t *ob_out;
    unsigned long long *cnt;
};

int env_int(const char *name) {
    const char *e = getenv(name);
    return e ? atoi(e) : 0;
}

int check_run_args(const TickRun &r) {
    const swarm_fsm *fsm = r.fsm;
    SW_ARG(r.ctx != nullptr && fsm != nullptr, "NULL argument");
    SW_ARG(r.n >= 0 && r.n < (int64_t(1) << 31) && r.ticks >= 0 && r.t0 >= 0 && r.n_kill >= 0, "sizes out of range");
    SW_ARG(r.n_kill == 0 || r.kill_ticks != nullptr, "kill_ticks is NULL");
    SW_ARG(std::isfinite(r.dt) && r.timeout >= 0.0 && r.jitter >= 0.0, "dt / timeout / jitter out of range");
    SW_ARG(r.hear_row_ptr != nullptr || r.hear_col == nullptr, "hear_col without hear_row_ptr");
    SW_ARG(r.n == 0 || (r.ids && r.pos && (r.row_ptr || r.radio()) && r.tick_off && fsm->state && fsm->leader &&
                        fsm->last_hb && fsm->wait_start && fsm->delay && fsm->leader_pos && fsm->has_leader_pos &&
                        fsm->alive && fsm->outbox),
           "NULL agent array");
    SW_ARG(!std::isnan(r.pull_frac), "pull_frac is NaN");
    return SWARM_OK;
}

// Four counters per tick of the run in one scratch slot: per tick kShards x 4 partial counters (add_counts),
// cleared, then per tick their 4 sums (k_sum_counts), then `extra` bytes of the owner's.
struct TickSums {
    unsigned long long *part = nullptr, *sums = nullptr;
    int64_t t0 = 0, ticks = 0;

    int begin(const TickRun &r, Slot slot, hipStream_t s, size_t extra = 0) {
        t0 = r.t0;
        ticks = r.ticks;
        const size_t part_bytes = size_t(ticks) * kShards * 4 * 8;
        SW_ALLOC(part, r.ctx, slot, part_bytes + bytes() + extra);
        sums = part + size_t(ticks) * kShards * 4;
        SW_HIP(hipMemsetAsync(part, 0, part_bytes, s));
        return SWARM_OK;
    }
    unsigned long long *at(int64_t t) const { return part + size_t(t - t0 - 1) * kShards * 4; }  // tick t's partials
    size_t bytes() const { return size_t(ticks) * 4 * 8; }                                       // of the sums
    int sum_into(unsigned long long *host_dst, hipStream_t s) const {
        hipLaunchKernelGGL(k_sum_counts, dim3(grid_for(ticks * 4, kBlock, 256)), dim3(kBlock), 0, s, ticks, part, sums);
        SW_LAUNCHED();
        SW_HIP(hipMemcpyAsync(host_dst, sums, bytes(), hipMemcpyDeviceToHost, s));
        return SWARM_OK;
    }
};

// The run's counters in one scratch buffer (S_TMP0), laid out once.
struct Counters {
    TickSums tick;                  // lead, wait, acclaims, heartbeats
    unsigned long long *tr_shards;  // kShards x kTraffic traffic counters, NULL when no traffic is asked for
    unsigned long long *tr_sums;    // their kTraffic sums (k_sum_traffic)
    unsigned long long *sing;       // the loop's singular count: the last 64 bytes of the buffer
    int lay(const TickRun &r, hipStream_t s) {
        const size_t tr_bytes = size_t(kShards) * kTraffic * 8;
        if (const int rc = tick.begin(r, S_TMP0, s, tr_bytes + kTraffic * 8 + 64)) return rc;
        unsigned long long *shards = tick.sums + tick.ticks * 4;
        tr_shards = r.traffic ? shards : nullptr;
        tr_sums = shards + size_t(kShards) * kTraffic;
        sing = tr_sums + kTraffic;
        if (tr_shards) SW_HIP(hipMemsetAsync(tr_shards, 0, tr_bytes, s));
        if (r.loop) SW_HIP(hipMemsetAsync(sing, 0, 8, s));
        return SWARM_OK;
    }
};

// The sweep role's grid, and every per-agent kernel's of the run: 2 560 workgroups at most, with half as many
// in the receive role (10M agents, one-launch ticks, two boxes: 0.1208-0.1212 ms per tick against
// 0.1232-0.1234 for 2 048 + 1 280, 0.122 for 1 536 + 1 280, 2 560 + 1 536 and 3 072 + 1 280; the two-launch
// form had 2 048 + 1 280 at 0.128, 4 096 + 2 048 at 0.131; SWARM_FSM_SWEEP_WGS overrides, A/B aid)
unsigned sweep_grid(int64_t n) {
    static const int sweep_env = env_int("SWARM_FSM_SWEEP_WGS");
    return grid_for(n, kBlock, sweep_env > 0 ? unsigned(sweep_env) : 2560u);
}

// The run's records (flag word + timer tick, leader + leader position; unpacked into the caller's arrays at
// the end of the run), the LRecs on a 16-byte boundary; *vec: the sweep may load words (the outbox 16-byte
// aligned -- the tick's half is checked per launch; the records are scratch).
int pack_records(const TickRun &r, unsigned grid, Fsm *f, int *vec, hipStream_t s) {
    const swarm_fsm *fsm = r.fsm;
    uint8_t *recs;
    SW_ALLOC(recs, r.ctx, S_FSM_FLAGS, size_t(r.n) * 24 + 16);
    *f = Fsm{reinterpret_cast<uint2 *>(recs), reinterpret_cast<LRec *>(recs + lrec_offset(r.n)), fsm->last_hb,
             fsm->wait_start, fsm->delay, r.t0, r.t0 + r.ticks, r.dt};
    auto a16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    *vec = a16(fsm->outbox) && a16(recs);
    SW_ARG((reinterpret_cast<uintptr_t>(fsm->leader_pos) & 7) == 0, "leader_pos is not 8-byte aligned");
    hipLaunchKernelGGL(k_pack_fsm, dim3(grid), dim3(kBlock), 0, s, r.n, fsm->state, fsm->alive, fsm->has_leader_pos,
                       r.tick_off, fsm->leader, reinterpret_cast<const float2 *>(fsm->leader_pos), *f);
    SW_LAUNCHED();
    return SWARM_OK;
}

// Push mode: the mail words (three buffers rotated by tick, NextMail), the single-sender slots (two, by tick
// parity), the pull flags (by tick, after the words) and k_tick's sender segments.
struct PushState {
    static constexpr int nbuf = 3;
    int64_t n = 0, n_words = 0;
    unsigned long long *mw = nullptr;  // buffer b: mail bits at mw + 2b n_words, multi bits after them
    int32_t *from_base = nullptr;
    unsigned *pullf = nullptr;         // [nbuf] by tick: the tick pulls
    TickShape shape{};                 // k_tick's grid (both roles), the XCD-grouped order, the segments' capacities
    Segs segs{};

    Mail mail_of(int64_t tick) const {  // the mail a tick receives
        Mail m{};
        m.bits = mw + size_t(tick % nbuf) * 2 * size_t(n_words);
        m.multi = m.bits + n_words;
        m.from = from_base + size_t(tick & 1) * size_t(n);
        return m;
    }

    // Scratch, everything cleared, and the mail for tick t0 + 1 from tick t0's sends (a resumed run).
    int begin(const TickRun &r, unsigned grid, hipStream_t s) {
        static const int recv_env = env_int("SWARM_FSM_RECV_WGS"), xg_env = env_int("SWARM_TICK_XCD_GROUP");
        n = r.n;
        n_words = (n + 63) / 64;
        shape = tick_shape(n, grid, recv_env, xg_env);
        SW_ALLOC(mw, r.ctx, S_FSM_MAIL, size_t(n_words) * 48 + 64);
        SW_ALLOC(from_base, r.ctx, S_FSM_FROM, size_t(n) * 8);
        segs = Segs{nullptr, shape.rcap, shape.scap, shape.g_recv};
        SW_ALLOC(segs.base, r.ctx, S_FSM_SEND, size_t(shape.seg_total) * 4);
        pullf = reinterpret_cast<unsigned *>(mw + 6 * n_words);
        SW_HIP(hipMemsetAsync(mw, 0, size_t(n_words) * 48 + 64, s));
        hipLaunchKernelGGL(k_mail_from_outbox, dim3(grid), dim3(kBlock), 0, s, n,
                           r.fsm->outbox + size_t(r.t0 & 1) * size_t(n), r.hear_row_ptr, r.hear_col,
                           mail_of(r.t0 + 1));
        SW_LAUNCHED();
        return SWARM_OK;
    }

    // Tick k.t: receives buf(t), mails into buf(t+1), clears buf(t+2).
    int launch(const TickRun &r, const Fsm &f, const Tick &k, int vec, unsigned long long *tr, hipStream_t s) const {
        const int64_t t = k.t;
        const NextMail im{mail_of(t + 1), mail_of(t + 2).bits, 2 * n_words, pullf + (t + 1) % nbuf,
                          pullf + (t + 2) % nbuf, r.pull_frac < 0.0 ? -1.0 : r.pull_frac, r.hear_row_ptr,
                          r.hear_col, r.t0};
        hipLaunchKernelGGL(k_tick, dim3(shape.tgrid), dim3(kBlock), 0, s, n, t, r.ids, k.pos, r.row_ptr, r.col, f,
                           mail_of(t), k.ob_in, k.ob_out, pullf + t % nbuf, segs, r.dt, r.timeout, r.jitter, r.seed,
                           k.cnt, int(vec && (reinterpret_cast<uintptr_t>(k.ob_out) & 3) == 0), tr, im, shape.xg);
        SW_LAUNCHED();
        return SWARM_OK;
    }
};

// Radio mode (U1-R): no mail bitmap, no sender segments -- the receivers find their senders in their windows
// of the tick's binning (LoopSense), through a cell-sorted copy of the outbox and a byte per cell.
struct RadioState {
    Radio rw{};
    size_t cells = 0;

    // planes: bytes per cell (U1-T keeps one for each kind of sender, TaskState)
    int begin(const TickRun &r, const LoopSense &ls, int planes = 1) {
        rw.g = ls.g;
        rw.r2 = r.loop->radio_radius * r.loop->radio_radius;
        rw.st = ls.st;
        cells = size_t(ls.g.ncx * ls.g.ncy);
        SW_ALLOC(rw.ob_sorted, r.ctx, S_RADIO_OUTBOX, size_t(r.n));
        SW_ALLOC(rw.cell_send, r.ctx, S_RADIO_CELLS, cells * size_t(planes));
        return SWARM_OK;
    }

    // the tick's binning: rebuilt by loop_sense_tick before every tick's launches
    void bind(const LoopSense &ls) {
        rw.sorted = ls.sorted;
        rw.off = ls.off;
        rw.psort = ls.psort;
    }

    // ch: NoLoss{}, or the tick's Lossy
    template <class Ch>
    int launch(const TickRun &r, const Fsm &f, const Tick &k, Ch ch, hipStream_t s) const {
        const dim3 grid(grid_for(r.n, kBlock, 8192));
        SW_HIP(hipMemsetAsync(rw.cell_send, 0, cells, s));
        hipLaunchKernelGGL(k_radio_outbox<false>, grid, dim3(kBlock), 0, s, r.n, k.ob_in, rw, (uint8_t *)nullptr,
                           (uint8_t *)nullptr);
        SW_LAUNCHED();
        hipLaunchKernelGGL(k_tick_radio<Ch>, grid, dim3(kBlock), 0, s, r.n, k.t, r.ids, k.pos, f, rw, k.ob_out, r.dt,
                           r.timeout, r.jitter, r.seed, k.cnt, ch);
        SW_LAUNCHED();
        return SWARM_OK;
    }
};

// Task mode (U1-T): RadioState's scratch with three bytes per cell, the per-tick task counters (claims sent,
// handled, conflicts sent, guard pairs) and the tick's three launches.
struct TaskState {
    TickSums cnt;
    uint8_t *sb = nullptr;  // the sender bytes, 2n by tick parity (TaskTick)
    unsigned long long tmask = 0;

    int begin(const TickRun &r, hipStream_t s) {
        const swarm_tasks &b = *r.tasks;
        if (const int rc = cnt.begin(r, S_TASK_COUNTS, s)) return rc;
        SW_ALLOC(sb, r.ctx, S_TASK_SENDERS, size_t(r.n) * 2);
        tmask = b.T >= 64 ? ~0ull : (1ull << b.T) - 1ull;
        hipLaunchKernelGGL(k_task_sender_bytes, dim3(grid_for(2 * r.n, kBlock, 8192)), dim3(kBlock), 0, s, 2 * r.n,
                           r.fsm->outbox, reinterpret_cast<const unsigned long long *>(b.claim_out),
                           reinterpret_cast<const unsigned long long *>(b.conflict_out), tmask, sb);
        SW_LAUNCHED();
        return SWARM_OK;
    }

    // rs: bound to the tick's binning; ch: NoLoss{}, or the tick's Lossy
    template <class Ch>
    int launch(const TickRun &r, const Fsm &f, const Tick &k, const RadioState &rs, Ch ch, hipStream_t s) const {
        const dim3 grid(grid_for(r.n, kBlock, 8192));
        const swarm_tasks &b = *r.tasks;
        const size_t un = size_t(r.n), in = size_t((k.t - 1) & 1) * un, out = size_t(k.t & 1) * un;
        auto u64 = [](uint64_t *p) { return reinterpret_cast<unsigned long long *>(p); };
        const TaskTick tk{b.T,
                          tmask,
                          reinterpret_cast<const double2 *>(b.tpos),
                          b.treq,
                          b.caps,
                          u64(b.status_lo),
                          u64(b.status_hi),
                          u64(b.claim_out) + in,
                          u64(b.conflict_out) + in,
                          u64(b.claim_out) + out,
                          u64(b.conflict_out) + out,
                          b.tab_winner,
                          b.tab_util,
                          rs.rw.cell_send + rs.cells,
                          rs.rw.cell_send + 2 * rs.cells,
                          cnt.at(k.t),
                          sb + in,
                          sb + out};
        SW_HIP(hipMemsetAsync(rs.rw.cell_send, 0, 3 * rs.cells, s));
        hipLaunchKernelGGL(k_radio_outbox<true>, grid, dim3(kBlock), 0, s, r.n, tk.sb_in, rs.rw, tk.cell_claim,
                           tk.cell_conf);
        SW_LAUNCHED();
        if constexpr (Ch::kLossy)
            hipLaunchKernelGGL((k_task_conflicts<Ch, int64_t>), grid, dim3(kBlock), 0, s, r.n, k.t, r.ids, f.rec,
                               rs.rw, tk, ch);
        else
            hipLaunchKernelGGL(k_task_conflicts<Ch>, grid, dim3(kBlock), 0, s, r.n, r.ids, f.rec, rs.rw, tk, ch);
        SW_LAUNCHED();
        hipLaunchKernelGGL(k_tick_radio_tasks<Ch>, grid, dim3(kBlock), 0, s, r.n, k.t, r.ids, k.pos, f, rs.rw,
                           k.ob_out, r.dt, r.timeout, r.jitter, r.seed, k.cnt, tk, ch);
        SW_LAUNCHED();
        return SWARM_OK;
    }
};

// Board mode (U1-B): TaskState's scratch and counters, the entry check of the caller's sparse rows and the
// tick's three launches over them.
struct BoardState {
    TickSums cnt;
    uint8_t *sb = nullptr;  // the sender bytes, 2n by tick parity (BoardTick)

    // The entry check, queued before the call's entry wait (loop_sense_begin's): its verdict is on the host when
    // that wait ends, before anything is written.
    static int check_entry(const TickRun &r, hipStream_t s) {
        const swarm_board &b = *r.board;
        const swarm_board_state &q = *r.bstate;
        const int64_t n = r.n;
        SW_HIP(hipMemsetAsync(b.verdict, 0, 8, s));
        const struct {
            const int32_t *a;
            int64_t rows;
            int K, sh;
        } arr[4] = {{q.status, n, q.Ks, 2}, {q.tab_task, n, q.Kt, 0}, {q.claim_out, 2 * n, q.Ks, 0},
                    {q.conflict_out, 2 * n, q.Kt, 0}};
        for (const auto &a : arr) {
            hipLaunchKernelGGL(k_board_check_rows, dim3(grid_for(a.rows * a.K, kBlock, 8192)), dim3(kBlock), 0, s,
                               a.rows * a.K, a.K, a.sh, int32_t(b.T), a.a, b.verdict);
            SW_LAUNCHED();
        }
        b.verdict_host[0] = 1;  // (overwritten by the copy: a wait that never came reads as a refusal)
        SW_HIP(hipMemcpyAsync(b.verdict_host, b.verdict, 8, hipMemcpyDeviceToHost, s));
        return SWARM_OK;
    }
    static int entry_verdict(const TickRun &r) {
        SW_ARG(r.board->verdict_host[0] == 0,
               "a sparse task row holds an entry that is no task of the board, a status code outside 1..3, or is "
               "not strictly ascending with its empty slots last");
        return SWARM_OK;
    }

    int begin(const TickRun &r, hipStream_t s) {
        const swarm_board_state &q = *r.bstate;
        if (const int rc = cnt.begin(r, S_TASK_COUNTS, s)) return rc;
        SW_ALLOC(sb, r.ctx, S_TASK_SENDERS, size_t(r.n) * 2);
        hipLaunchKernelGGL(k_board_sender_bytes, dim3(grid_for(2 * r.n, kBlock, 8192)), dim3(kBlock), 0, s, 2 * r.n,
                           r.fsm->outbox, q.claim_out, q.Ks, q.conflict_out, q.Kt, sb);
        SW_LAUNCHED();
        return SWARM_OK;
    }

    // rs: bound to the tick's binning; st: the call's verdict words; ch: NoLoss{}, or the tick's Lossy
    template <class Ch>
    int launch(const TickRun &r, const Fsm &f, const Tick &k, const RadioState &rs, unsigned long long *st, Ch ch,
               hipStream_t s) const {
        const dim3 grid(grid_for(r.n, kBlock, 8192));
        const swarm_board &b = *r.board;
        const swarm_board_state &q = *r.bstate;
        const size_t un = size_t(r.n), in = size_t((k.t - 1) & 1) * un, out = size_t(k.t & 1) * un;
        const size_t ks = size_t(q.Ks), kt = size_t(q.Kt);
        // (U1-M) a moving board: the tick's lists on the call's grid, the claim handler's positions one advance behind
        const Grid &tg = b.moving ? b.call_g : b.g;
        const BoardTick bt{q.Ks,
                           q.Kt,
                           int32_t(k.t - r.t0 - 1),
                           reinterpret_cast<const double2 *>(b.moving ? b.lag : b.tpos),
                           b.treq,
                           BoardGrid{b.moving ? b.dyn_off : b.cell_off, reinterpret_cast<const double2 *>(b.sxy),
                                     reinterpret_cast<const int2 *>(b.sir), tg.xmin, tg.ymin, tg.xmax, tg.ymax,
                                     tg.inv_cell, tg.ncx, tg.ncy},
                           q.caps,
                           q.status,
                           q.tab_task,
                           q.tab_winner,
                           q.tab_util,
                           q.claim_out + in * ks,
                           q.conflict_out + in * kt,
                           q.claim_out + out * ks,
                           q.conflict_out + out * kt,
                           rs.rw.cell_send + rs.cells,
                           rs.rw.cell_send + 2 * rs.cells,
                           cnt.at(k.t),
                           sb + in,
                           sb + out,
                           st};
        SW_HIP(hipMemsetAsync(rs.rw.cell_send, 0, 3 * rs.cells, s));
        hipLaunchKernelGGL(k_radio_outbox<true>, grid, dim3(kBlock), 0, s, r.n, bt.sb_in, rs.rw, bt.cell_claim,
                           bt.cell_conf);
        SW_LAUNCHED();
        // (contract U1-A) a board with lifetimes: conflicts about the tasks absent this tick write nothing
        if (b.alive())
            hipLaunchKernelGGL((k_board_conflicts<Ch, Lifetimes>), grid, dim3(kBlock), 0, s, r.n, k.t, r.ids, f.rec,
                               rs.rw, bt, BoardPolicy<Ch, Lifetimes>{ch, Lifetimes{b.present}});
        else
            hipLaunchKernelGGL((k_board_conflicts<Ch, NoLife>), grid, dim3(kBlock), 0, s, r.n, k.t, r.ids, f.rec,
                               rs.rw, bt, BoardPolicy<Ch, NoLife>{ch, NoLife{}});
        SW_LAUNCHED();
        hipLaunchKernelGGL(k_tick_radio_board<Ch>, grid, dim3(kBlock), 0, s, r.n, k.t, r.ids, k.pos, f, rs.rw,
                           k.ob_out, r.dt, r.timeout, r.jitter, r.seed, k.cnt, bt, ch);
        SW_LAUNCHED();
        return SWARM_OK;
    }
};

int launch_tick_pull(const TickRun &r, unsigned grid, const Fsm &f, const Tick &k, hipStream_t s) {
    hipLaunchKernelGGL(k_tick_pull, dim3(grid), dim3(kBlock), 0, s, r.n, k.t, r.ids, k.pos, r.row_ptr, r.col, f,
                       k.ob_in, k.ob_out, r.dt, r.timeout, r.jitter, r.seed, k.cnt);
    SW_LAUNCHED();
    return SWARM_OK;
}

// The sensed loops (U1-S, U1-R): the caller's arrays as they are at entry, put back on the device if a tick
// is refused -- the ticks after a refused one are already queued and run on the records, so the call is all
// or nothing, and it needs no host wait to decide.
struct EntrySnapshot {
    struct Kept {
        void *p;
        size_t bytes, at;
    } kept[24];
    int nkept = 0;
    uint8_t *snap = nullptr;

    // booted_tick_off: the tick offsets of a call with agent events (contract U1-J: a boot writes them), else NULL
    int take(const TickRun &r, hipStream_t s, int32_t *booted_tick_off = nullptr) {
        const LoopArgs *loop = r.loop;
        const swarm_fsm *fsm = r.fsm;
        const size_t un = size_t(r.n);
        const Kept all[14] = {{loop->pos, un * 16, 0},       {loop->pos_prev, un * 16, 0},  {loop->vel, un * 16, 0},
                              {loop->target, un * 16, 0},    {fsm->last_hb, un * 8, 0},     {fsm->wait_start, un * 8, 0},
                              {fsm->delay, un * 8, 0},       {fsm->leader_pos, un * 8, 0},  {fsm->leader, un * 4, 0},
                              {fsm->outbox, un * 2, 0},      {loop->has_target, un, 0},     {fsm->state, un, 0},
                              {fsm->alive, un, 0},           {fsm->has_leader_pos, un, 0}};
        nkept = 0;
        for (int q = 0; q < 14; ++q) kept[nkept++] = all[q];
        if (booted_tick_off) kept[nkept++] = Kept{booted_tick_off, un * 4, 0};
        if (r.tasked()) {  // U1-T: every task array as well
            const swarm_tasks &b = *r.tasks;
            const size_t row = un * size_t(b.T) * 4;
            const Kept more[6] = {{b.status_lo, un * 8, 0},     {b.status_hi, un * 8, 0}, {b.claim_out, un * 16, 0},
                                  {b.conflict_out, un * 16, 0}, {b.tab_winner, row, 0},   {b.tab_util, row, 0}};
            for (int q = 0; q < 6; ++q) kept[nkept++] = more[q];
        }
        if (r.boarded()) {  // U1-B: the six sparse arrays
            const swarm_board_state &b = *r.bstate;
            const size_t srow = un * size_t(b.Ks) * 4, trow = un * size_t(b.Kt) * 4;
            const Kept more[6] = {{b.status, srow, 0},     {b.tab_task, trow, 0},      {b.tab_winner, trow, 0},
                                  {b.tab_util, trow, 0},   {b.claim_out, 2 * srow, 0}, {b.conflict_out, 2 * trow, 0}};
            for (int q = 0; q < 6; ++q) kept[nkept++] = more[q];
        }
        size_t total = 0;
        for (int q = 0; q < nkept; ++q) {
            kept[q].at = total;
            total += (kept[q].bytes + 15) & ~size_t(15);
        }
        SW_ALLOC(snap, r.ctx, S_LOOP_SNAP, total);
        for (int q = 0; q < nkept; ++q)
            SW_HIP(hipMemcpyAsync(snap + kept[q].at, kept[q].p, kept[q].bytes, hipMemcpyDeviceToDevice, s));
        return SWARM_OK;
    }

    // st[0] != 0: every caller array back to its entry bytes (the unpack before it included), on the device.
    int restore_if_refused(const unsigned long long *st, hipStream_t s) const {
        for (int q = 0; q < nkept; ++q) {
            const Kept &k = kept[q];
            hipLaunchKernelGGL(k_restore_refused, dim3(grid_for(int64_t(k.bytes / 8 + 1), kBlock, 4096)),
                               dim3(kBlock), 0, s, st, static_cast<uint8_t *>(k.p), snap + k.at, k.bytes);
            SW_LAUNCHED();
        }
        return SWARM_OK;
    }
};

// The A/B aid of -DSWARM_TICK_CLOCKS=1 (k_tick's TICK_CLK): the device buffer before the ticks, its records
// to SWARM_TICK_CLOCKS_FILE after them (header: ticks, workgroups, receive-role workgroups).  Empty otherwise.
struct TickClocks {
#if SWARM_TICK_CLOCKS
    unsigned long long *buf = nullptr;
    const char *file = nullptr;
    size_t words = 0;

    int begin(const TickRun &r, const PushState &ps, hipStream_t s) {
        file = getenv("SWARM_TICK_CLOCKS_FILE");
        words = size_t(r.ticks) * ps.shape.tgrid * 5;
        if (r.push() && file) {
            SW_HIP(hipMalloc(&buf, words * 8));
            SW_HIP(hipMemsetAsync(buf, 0, words * 8, s));
        }
        SW_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_tick_clk), &buf, sizeof(buf), 0, hipMemcpyHostToDevice, s));
        return SWARM_OK;
    }

    int end(const TickRun &r, const PushState &ps, hipStream_t s) {
        if (!buf) return SWARM_OK;
        std::vector<unsigned long long> hc(words);
        SW_HIP(hipMemcpyAsync(hc.data(), buf, words * 8, hipMemcpyDeviceToHost, s));
        SW_HIP(hipStreamSynchronize(s));
        SW_HIP(hipFree(buf));
        if (FILE *fp = fopen(file, "wb")) {
            const long long hdr[3] = {r.ticks, (long long)ps.shape.tgrid, ps.shape.g_recv};
            fwrite(hdr, 8, 3, fp);
            fwrite(hc.data(), 8, hc.size(), fp);
            fclose(fp);
        }
        return SWARM_OK;
    }
#else
    int begin(const TickRun &, const PushState &, hipStream_t) { return SWARM_OK; }
    int end(const TickRun &, const PushState &, hipStream_t) { return SWARM_OK; }
#endif
};

// The tick's physics: P_{t-1} (cur) -> P_t over the lagged buffer, then the roles swap; the trace frame.
int tick_physics(const TickRun &r, const Fsm &f, const LoopSense &ls, int64_t t, double **cur, double **lag,
                 unsigned long long *sing, hipStream_t s) {
    const LoopArgs *loop = r.loop;
    // `obstacles` that is a live field's own list: the sensed loops take the field's path (contract O1)
    const swarm_obstacle_field *fld = r.sensed() ? find_obstacle_field(r.ctx, loop->m, loop->obstacles) : nullptr;
    if (fld && fld->moving) {  // contract O2: the lists of O_{t-1} built on the device, then every obstacle advances
        swarm_obstacle_field *mov = find_moving_field(r.ctx, loop->m, loop->obstacles);
        ObsFieldView view;
        int rm;
        if ((rm = moving_field_tick(mov, ls.st, int32_t(t - r.t0 - 1), &view, s))) return rm;
        if ((rm = launch_physics_loop_sensed_field(r.n, r.ids, f.rec, f.lrec, *lag, loop->vel, loop->target,
                                                   loop->has_target, view, ls, r.dt, loop->max_speed, sing, s)))
            return rm;
        if ((rm = moving_field_advance(mov, ls.st, r.dt, s))) return rm;
    }
    const int rc = fld && fld->moving ? SWARM_OK
                   : fld        ? launch_physics_loop_sensed_field(r.n, r.ids, f.rec, f.lrec, *lag, loop->vel, loop->target,
                                                                 loop->has_target, obstacle_field_view(*fld), ls, r.dt,
                                                                 loop->max_speed, sing, s)
                   : r.sensed() ? launch_physics_loop_sensed(r.n, r.ids, f.rec, f.lrec, *lag, loop->vel, loop->target,
                                                           loop->has_target, loop->m, loop->obstacles, ls, r.dt,
                                                           loop->max_speed, sing, s)
                              : launch_physics_loop(r.n, r.ids, f.rec, f.lrec, *cur, *lag, loop->vel, loop->target,
                                                    loop->has_target, loop->m, loop->obstacles, loop->sense_rp,
                                                    loop->sense_col, r.dt, loop->max_speed, sing, s);
    if (rc) return rc;
    std::swap(*cur, *lag);
    const int64_t k = t - r.t0;
    if (loop->trace_every > 0 && k % loop->trace_every == 0)
        SW_HIP(hipMemcpyAsync(loop->trace + size_t(k / loop->trace_every - 1) * size_t(r.n) * 2, *cur,
                              size_t(r.n) * 16, hipMemcpyDeviceToDevice, s));
    return SWARM_OK;
}

// The run's results: the traffic sums, (sensed) the verdict words, the loop's singular count and the counts
// come back through pinned memory -- [0..3] verdict, [4] singular, [8..15] traffic, [16..] counts -- in the
// run's one final host wait (none when nothing is asked for).  A refused tick (`snap` restores the caller's
// arrays) withholds the counts and the singular count and sets refused_tick.
int read_back(const TickRun &r, const Counters &c, const LoopSense *ls, const EntrySnapshot &snap,
              const TickSums &tasks, const TickSums &links, swarm_obstacle_field *mov, hipStream_t s) {
    const bool want_sing = r.loop && r.loop->n_singular;
    const bool want_tasks = (r.tasked() || r.boarded()) && (r.task_counts || r.n_guard);
    const bool want_links = r.lossy() && r.link_counts;
    if (r.traffic) {  // (pull-mode runs: every tick walks every row -- the receivers are all agents)
        hipLaunchKernelGGL(k_sum_traffic, dim3(1), dim3(kWave), 0, s, c.tr_shards, c.tr_sums);
        SW_LAUNCHED();
    }
    if (ls)
        if (const int rc = snap.restore_if_refused(ls->st, s)) return rc;
    if (ls && mov)  // (contract O2) the list is the field's own array: back to its entry bits as well
        if (const int rc = moving_field_restore_if_refused(mov, ls->st, s)) return rc;
    if (ls && r.boarded() && r.mboard)  // (contract U1-M) the board's two lists likewise
        if (const int rc = moving_board_restore_if_refused(r.mboard, ls->st, s)) return rc;
    if (!(r.traffic || ls || want_sing || r.counts || want_tasks || want_links)) return SWARM_OK;
    // the sums that are asked for, one after the other from [16]: counts, task counts, link counts
    const size_t words = size_t(r.ticks) * 4, cnt_bytes = r.counts ? words * 8 : 0;
    unsigned long long *h = static_cast<unsigned long long *>(
        pinned(r.ctx, 128 + cnt_bytes + (size_t(want_tasks) + size_t(want_links)) * words * 8));
    if (!h) return SWARM_ERR_OOM;
    unsigned long long *ht = h + 16 + cnt_bytes / 8, *hl = ht + (want_tasks ? words : 0);
    int rc;
    if (want_links && (rc = links.sum_into(hl, s))) return rc;
    if (want_tasks && (rc = tasks.sum_into(ht, s))) return rc;
    if (r.traffic) SW_HIP(hipMemcpyAsync(h + 8, c.tr_sums, kTraffic * 8, hipMemcpyDeviceToHost, s));
    if (ls) SW_HIP(hipMemcpyAsync(h, ls->st, 32, hipMemcpyDeviceToHost, s));
    h[5] = 0;
    if (ls && mov && (rc = moving_field_error(mov, h + 5, s))) return rc;
    if (want_sing) SW_HIP(hipMemcpyAsync(h + 4, c.sing, 8, hipMemcpyDeviceToHost, s));
    if (r.counts && (rc = c.tick.sum_into(h + 16, s))) return rc;
    SW_HIP(hipStreamSynchronize(s));
    if (r.traffic) for (int q = 0; q < kTraffic; ++q) r.traffic[q] = int64_t(h[8 + q]);
    if (ls && h[0]) {
        const int64_t tick = r.t0 + int64_t(h[0]);
        if (r.loop->refused_tick) *r.loop->refused_tick = tick;
        if (h[5]) return moving_field_overflowed();
        if (h[1]) {  // U1-B: a sparse row overflowed (st[1] = kind << 32 | agent)
            const int kind = int(h[1] >> 32);
            const long long agent = static_cast<long long>(h[1] & 0xFFFFFFFFull);
            if (r.overflow) *r.overflow = swarm_board_overflow{kind, 0, agent};
            set_error("agent %lld (storage index) needs more than its %d %s slots at tick %lld (nothing of the call "
                      "is kept; repeat it with larger rows)",
                      agent, kind == SWARM_BOARD_STATUS ? r.bstate->Ks : r.bstate->Kt,
                      kind == SWARM_BOARD_STATUS ? "status" : "table", static_cast<long long>(tick));
            return SWARM_ERR_RANGE;
        }
        return loop_sense_refusal(h, "agents too dense to sense at tick %lld (nothing of the call is kept)",
                                  static_cast<long long>(tick));
    }
    if (want_sing) *r.loop->n_singular = int64_t(h[4]);
    if (r.counts) memcpy(r.counts, h + 16, cnt_bytes);
    if (want_tasks) {
        int64_t guard = 0;
        for (int64_t q = 0; q < r.ticks; ++q) {
            if (r.task_counts) for (int c = 0; c < 3; ++c) r.task_counts[3 * q + c] = int64_t(ht[4 * q + c]);
            guard += int64_t(ht[4 * q + 3]);
        }
        if (r.n_guard) *r.n_guard = guard;
    }
    if (want_links)
        for (int64_t q = 0; q < r.ticks; ++q)
            for (int c = 0; c < 2; ++c) r.link_counts[2 * q + c] = int64_t(hl[4 * q + c]);
    return SWARM_OK;
}

// The ticks t0+1 .. t0+ticks of every entry point below.
int run_ticks(const TickRun &r) {
    int rc;
    if ((rc = check_run_args(r))) return rc;
    if (r.traffic) for (int q = 0; q < kTraffic; ++q) r.traffic[q] = 0;
    if (r.task_counts) for (int64_t q = 0; q < int64_t(r.ticks) * 3; ++q) r.task_counts[q] = 0;
    if (r.n_guard) *r.n_guard = 0;
    if (r.lossy() && r.link_counts) for (int64_t q = 0; q < int64_t(r.ticks) * 2; ++q) r.link_counts[q] = 0;
    if (r.n == 0 || r.ticks == 0) {
        if (r.counts) for (int64_t q = 0; q < int64_t(r.ticks) * 4; ++q) r.counts[q] = 0;
        return SWARM_OK;
    }
    hipStream_t s = static_cast<hipStream_t>(r.stream);
    const LoopArgs *loop = r.loop;
    const bool sensed = r.sensed(), radio = r.radio(), push = r.push(), tasked = r.tasked(), boarded = r.boarded();
    // (contract U1-J) agent lifetimes attached to this alive array: the call's events, found on the host
    swarm_agent_life *life = find_agent_life(r.ctx, r.n, r.fsm->alive);
    AgentSchedule events;
    if (life) {
        SW_ARG(r.tick_off == life->tick_off, "tick_off is not the array the agent lifetimes were created with");
        if ((rc = agent_life_begin(life, r.t0, r.ticks, &events, s))) return rc;
    }
    // U1-S / U1-R: the call's grid (the loop's one host wait before its end; non-finite positions are refused
    // here; U1-R: cells wide enough for the radio window too -- one binning per tick serves both halves)
    LoopSense ls{};
    EntrySnapshot snap;
    // (contract O2) a moving field's list comes to the host with that wait; its grid and capacity are refused
    // before anything is written, and the field keeps its entry list for a refused tick
    swarm_obstacle_field *mov = sensed ? find_moving_field(r.ctx, loop->m, loop->obstacles) : nullptr;
    if (sensed) {
        if (mov && (rc = moving_field_fetch(mov, s))) return rc;
        if (boarded && (rc = BoardState::check_entry(r, s))) return rc;
        // (contract U1-M) the box of the tasks' spans over the call comes to the host with that wait as well
        if (boarded && r.mboard && (rc = moving_board_box(r.mboard, r.dt, r.ticks, s))) return rc;
        if ((rc = loop_sense_begin(r.ctx, r.n, loop->pos, loop->sense_radius, r.ticks, r.dt, loop->max_speed, &ls, s,
                                   radio ? loop->radio_radius : 0.0)))
            return rc;
        if (boarded && (rc = BoardState::entry_verdict(r))) return rc;
        if (boarded && r.mboard && (rc = moving_board_begin(r.mboard, s))) return rc;
        if (mov && (rc = moving_field_begin(mov, r.ticks, r.dt, true, s))) return rc;
        if ((rc = snap.take(r, s, events.empty() ? nullptr : life->tick_off))) return rc;
    }
    Counters cnt;
    if ((rc = cnt.lay(r, s))) return rc;
    const unsigned grid = sweep_grid(r.n);
    Fsm f;
    int vec;
    if ((rc = pack_records(r, grid, &f, &vec, s))) return rc;
    PushState ps;
    RadioState rs;
    TaskState ts;
    BoardState bs;
    TickSums links;  // a lossy run (U1-L): per tick the election links and those of them that were dropped
    TickClocks clk;
    if (push && (rc = ps.begin(r, grid, s))) return rc;
    if ((rc = clk.begin(r, ps, s))) return rc;
    if (radio && (rc = rs.begin(r, ls, tasked || boarded ? 3 : 1))) return rc;
    if (tasked && (rc = ts.begin(r, s))) return rc;
    if (boarded && (rc = bs.begin(r, s))) return rc;
    const bool lossy = radio && r.lossy();
    if (lossy && (rc = links.begin(r, S_LINK_COUNTS, s))) return rc;
    AgentEventArrays ev{};
    if (!events.empty()) {
        auto u64 = [](uint64_t *p) { return reinterpret_cast<unsigned long long *>(p); };
        ev.n = r.n;
        ev.rec = f.rec;
        ev.lrec = f.lrec;
        ev.last_hb = f.last_hb;
        ev.wait_start = f.wait_start;
        ev.delay = f.delay;
        ev.tick_off = life->tick_off;
        ev.outbox = r.fsm->outbox;
        if (loop) {
            ev.vel = reinterpret_cast<double2 *>(loop->vel);
            ev.target = reinterpret_cast<double2 *>(loop->target);
            ev.has_target = loop->has_target;
        }
        if (tasked) {
            const swarm_tasks &b = *r.tasks;
            ev.sb = ts.sb;
            ev.T = b.T;
            ev.status_lo = u64(b.status_lo);
            ev.status_hi = u64(b.status_hi);
            ev.claim_out = u64(b.claim_out);
            ev.conflict_out = u64(b.conflict_out);
            ev.tab_winner = b.tab_winner;
            ev.tab_util = b.tab_util;
        }
        if (boarded) {
            const swarm_board_state &q = *r.bstate;
            ev.sb = bs.sb;
            ev.Ks = q.Ks;
            ev.Kt = q.Kt;
            ev.b_status = q.status;
            ev.b_tab_task = q.tab_task;
            ev.b_tab_winner = q.tab_winner;
            ev.b_tab_util = q.tab_util;
            ev.b_claim_out = q.claim_out;
            ev.b_conflict_out = q.conflict_out;
        }
        ev.t0 = r.t0;
        ev.dt = r.dt;
    }
    double *cur = loop ? loop->pos : nullptr, *lag = loop ? loop->pos_prev : nullptr;  // P_{t-1}, P_{t-2}
    for (int64_t t = r.t0 + 1; t <= r.t0 + r.ticks; ++t) {
        // (a heartbeat sent during tick t-1 carries its sender's position of then: the loops' lagged buffer)
        const Tick k{t, reinterpret_cast<const double2 *>(loop ? lag : r.pos),
                     r.fsm->outbox + size_t((t - 1) & 1) * size_t(r.n), r.fsm->outbox + size_t(t & 1) * size_t(r.n),
                     cnt.tick.at(t)};
        if (std::find(r.kill_ticks, r.kill_ticks + r.n_kill, t) != r.kill_ticks + r.n_kill) {
            hipLaunchKernelGGL(k_kill_leaders, dim3(grid), dim3(kBlock), 0, s, r.n, f.rec);
            SW_LAUNCHED();
        }
        // (contract U1-J) a tick with agent events: its deaths, then its boots, over that tick's events alone
        if (events.has_events(t - r.t0 - 1) && (rc = launch_agent_events(life, events, t, ev, s))) return rc;
        // bin the snapshot P_{t-1}, judge its window work, sort a copy of it by cell (the call's grid reaches
        // far beyond the agents: offsets by search)
        if (sensed && (rc = loop_sense_tick(r.ctx, r.n, cur, int32_t(t - r.t0 - 1), &ls, s, true))) return rc;
        if (radio) rs.bind(ls);
        // (contract U1-M) the cell lists of Q_{t-1} before the tick's launches, the advance after them
        if (boarded && r.mboard && (rc = moving_board_tick(r.mboard, t, s))) return rc;
        // (contract U1-A) a retiring tick: the status entries of the tasks absent at t leave their rows first
        if (boarded && r.mboard && moving_board_retires(r.mboard, r.t0, t) &&
            (rc = moving_board_retire(r.mboard, ls.st, r.n, r.bstate->Ks, r.bstate->status, s)))
            return rc;
        auto window_tick = [&](auto ch) {
            return boarded  ? bs.launch(r, f, k, rs, ls.st, ch, s)
                   : tasked ? ts.launch(r, f, k, rs, ch, s)
                            : rs.launch(r, f, k, ch, s);
        };
        rc = lossy   ? window_tick(Lossy{r.ch->loss, r.ch->seed, links.at(t)})
             : radio ? window_tick(NoLoss{})
             : push  ? ps.launch(r, f, k, vec, cnt.tr_shards, s)
                     : launch_tick_pull(r, grid, f, k, s);
        if (rc) return rc;
        if (boarded && r.mboard && (rc = moving_board_advance(r.mboard, ls.st, r.dt, s))) return rc;
        if (loop && (rc = tick_physics(r, f, ls, t, &cur, &lag, cnt.sing, s))) return rc;
    }
    if (loop && cur != loop->pos) {  // an odd number of ticks: pos <- P_end, pos_prev <- P_{end-1}
        hipLaunchKernelGGL(k_swap_positions, dim3(grid_for(r.n, kBlock, 8192)), dim3(kBlock), 0, s, r.n,
                           reinterpret_cast<double2 *>(loop->pos), reinterpret_cast<double2 *>(loop->pos_prev));
        SW_LAUNCHED();
    }
    if ((rc = clk.end(r, ps, s))) return rc;
    hipLaunchKernelGGL(k_unpack_fsm, dim3(grid), dim3(kBlock), 0, s, r.n, r.fsm->state, r.fsm->alive,
                       r.fsm->has_leader_pos, r.fsm->leader, reinterpret_cast<float2 *>(r.fsm->leader_pos), f);
    SW_LAUNCHED();
    return read_back(r, cnt, sensed ? &ls : nullptr, snap, boarded ? bs.cnt : ts.cnt, links, mov, s);
}

// The three loop entry points' own arguments (run_ticks checks the rest): U1 takes a sensor CSR and n < 2^31,
// U1-S and U1-R sense (kMergeEnd = 2^31 - 1 is no agent: n < 2^31 - 1), U1-R hears by radius as well.
enum LoopKind { kLoopCsr, kLoopSensed, kLoopRadio };

int check_loop_args(LoopKind kind, swarm_ctx *ctx, int64_t n, int32_t ticks, double dt, const LoopArgs &a) {
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(n >= 0 && n < (int64_t(1) << 31) - (kind == kLoopCsr ? 0 : 1) && a.m >= 0 && ticks >= 0,
           "sizes out of range");
    if (kind == kLoopRadio)
        SW_ARG(a.radio_radius > 0 && std::isfinite(a.radio_radius), "radio_radius must be positive and finite");
    if (kind != kLoopCsr)
        SW_ARG(a.sense_radius > 0 && std::isfinite(a.sense_radius), "sense_radius must be positive and finite");
    SW_ARG(std::isfinite(dt) && std::isfinite(a.max_speed), "dt / max_speed must be finite");
    SW_ARG(n == 0 || (a.pos && a.pos_prev && a.vel && a.target && a.has_target && (kind != kLoopCsr || a.sense_rp)),
           "NULL agent array");
    SW_ARG(a.m == 0 || a.obstacles != nullptr, "obstacles is NULL");
    SW_ARG(a.trace_every >= 0, "trace_every must not be negative");
    SW_ARG(n == 0 || a.trace_every == 0 || ticks / a.trace_every == 0 || a.trace != nullptr, "trace is NULL");
    if (n > 0) {  // the two position buffers are both read and written by every tick: no shared element
        const uintptr_t p = reinterpret_cast<uintptr_t>(a.pos), q = reinterpret_cast<uintptr_t>(a.pos_prev);
        SW_ARG((p > q ? p - q : q - p) >= uintptr_t(n) * 16, "pos and pos_prev must not overlap");
        SW_ARG((p & 15) == 0 && (q & 15) == 0, "pos / pos_prev are not 16-byte aligned");
    }
    return SWARM_OK;
}

// swarm_update_loop_tasks' own argument: the board and the task arrays (T == 0: none is looked at).  The
// required capabilities are read back from the device (T <= 64 bytes, one host wait) so that a bad one is
// refused before anything is written.
int check_tasks(swarm_ctx *ctx, int64_t n, const swarm_tasks *b, void *stream) {
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(b != nullptr, "tasks is NULL");
    SW_ARG(b->T >= 0 && b->T <= kMaxTasks, "T must be in [0, 64]");
    if (b->T == 0) return SWARM_OK;
    SW_ARG(b->tpos && b->treq, "NULL task array");
    SW_ARG(n <= 0 || (b->caps && b->status_lo && b->status_hi && b->claim_out && b->conflict_out && b->tab_winner &&
                      b->tab_util),
           "NULL task array");
    auto al = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; };
    SW_ARG(al(b->tpos, 16), "tpos is not 16-byte aligned");
    SW_ARG(n <= 0 || (al(b->status_lo, 8) && al(b->status_hi, 8) && al(b->claim_out, 8) && al(b->conflict_out, 8)),
           "a task word array is not 8-byte aligned");
    int8_t rq[kMaxTasks];
    hipStream_t s = static_cast<hipStream_t>(stream);
    SW_HIP(hipMemcpyAsync(rq, b->treq, size_t(b->T), hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < b->T; ++k) SW_ARG(!bad_req(rq[k]), "a treq outside [-1, 31]");
    return SWARM_OK;
}

// swarm_update_loop_board's own arguments: the handle and the sparse state (T == 0: no array is looked at).  The
// rows' contents are checked on the device (BoardState::check_entry).
int check_board(swarm_ctx *ctx, int64_t n, const swarm_board *b, const swarm_board_state *q) {
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(b != nullptr, "board is NULL");
    SW_ARG(q != nullptr, "state is NULL");
    SW_ARG(q->Ks >= 1 && q->Ks <= 4096 && q->Kt >= 1 && q->Kt <= 4096, "status / table slots must be in [1, 4096]");
    SW_ARG(live_board(ctx, b), "the board is not a live board of this ctx");
    if (b->T == 0) return SWARM_OK;
    SW_ARG(n <= 0 || (q->caps && q->status && q->tab_task && q->tab_winner && q->tab_util && q->claim_out &&
                      q->conflict_out),
           "NULL task array");
    return SWARM_OK;
}

// swarm_update_loop_channel's own argument (NULL: the ideal channel).
int check_channel(const swarm_channel *ch) {
    SW_ARG(ch == nullptr || (ch->loss >= 0.0 && ch->loss <= 1.0), "loss must be in [0, 1]");
    return SWARM_OK;
}

// A loop entry point: its checks, its outputs' resting values, the run.
int run_loop(LoopKind kind, const TickRun &r) {
    if (const int rc = check_loop_args(kind, r.ctx, r.n, r.ticks, r.dt, *r.loop)) return rc;
    SW_ARG(kind != kLoopCsr || !find_moving_field(r.ctx, r.loop->m, r.loop->obstacles),
           "a moving obstacle field needs a sensed loop (a fixed-graph loop would read it as a frozen list)");
    if (r.loop->n_singular) *r.loop->n_singular = 0;
    if (r.loop->refused_tick) *r.loop->refused_tick = -1;
    return run_ticks(r);
}

}  // namespace
}  // namespace swarm

extern "C" {

int swarm_protocol_run(swarm_ctx *ctx, int64_t n, const int32_t *ids, const double *pos, const int32_t *row_ptr,
                       const int32_t *col, const int32_t *hear_row_ptr, const int32_t *hear_col,
                       const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks,
                       double dt, double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                       int32_t n_kill, int64_t *counts, void *stream) {
    return swarm::run_ticks({ctx, n, ids, pos, row_ptr, col, hear_row_ptr, hear_col, tick_off, fsm, t0, ticks, dt,
                             timeout, jitter, seed, kill_ticks, n_kill, -1.0, counts, nullptr, nullptr, stream});
}

int swarm_protocol_run_ex(swarm_ctx *ctx, int64_t n, const int32_t *ids, const double *pos, const int32_t *row_ptr,
                          const int32_t *col, const int32_t *hear_row_ptr, const int32_t *hear_col,
                          const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks,
                          double dt, double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                          int32_t n_kill, double pull_frac, int64_t *counts, int64_t *traffic, void *stream) {
    return swarm::run_ticks({ctx, n, ids, pos, row_ptr, col, hear_row_ptr, hear_col, tick_off, fsm, t0, ticks, dt,
                             timeout, jitter, seed, kill_ticks, n_kill, pull_frac, counts, traffic, nullptr, stream});
}

int swarm_update_loop(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                      const int32_t *row_ptr, const int32_t *col, const int32_t *hear_row_ptr,
                      const int32_t *hear_col, const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0,
                      int32_t ticks, double dt, double timeout, double jitter, uint64_t seed,
                      const int64_t *kill_ticks, int32_t n_kill, double pull_frac, double *vel, double *target,
                      uint8_t *has_target, int64_t m, const double *obstacles, const int32_t *sense_row_ptr,
                      const int32_t *sense_col, double max_speed, double *trace, int32_t trace_every,
                      int64_t *counts, int64_t *n_singular, void *stream) {
    using namespace swarm;
    const LoopArgs loop{pos, pos_prev, vel, target, has_target, m, obstacles, sense_row_ptr, sense_col, max_speed,
                        trace, trace_every, n_singular, 0.0, nullptr};
    return run_loop(kLoopCsr, {ctx, n, ids, pos, row_ptr, col, hear_row_ptr, hear_col, tick_off, fsm, t0, ticks, dt,
                               timeout, jitter, seed, kill_ticks, n_kill, pull_frac, counts, nullptr, &loop, stream});
}

int swarm_update_loop_sensed(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                             const int32_t *row_ptr, const int32_t *col, const int32_t *hear_row_ptr,
                             const int32_t *hear_col, const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0,
                             int32_t ticks, double dt, double timeout, double jitter, uint64_t seed,
                             const int64_t *kill_ticks, int32_t n_kill, double pull_frac, double *vel,
                             double *target, uint8_t *has_target, int64_t m, const double *obstacles,
                             double sense_radius, double max_speed, double *trace, int32_t trace_every,
                             int64_t *counts, int64_t *n_singular, int64_t *refused_tick, void *stream) {
    using namespace swarm;
    const LoopArgs loop{pos, pos_prev, vel, target, has_target, m, obstacles, nullptr, nullptr, max_speed,
                        trace, trace_every, n_singular, sense_radius, refused_tick};
    return run_loop(kLoopSensed, {ctx, n, ids, pos, row_ptr, col, hear_row_ptr, hear_col, tick_off, fsm, t0, ticks,
                                  dt, timeout, jitter, seed, kill_ticks, n_kill, pull_frac, counts, nullptr, &loop,
                                  stream});
}

int swarm_update_loop_radio(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                            const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks, double dt,
                            double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                            int32_t n_kill, double *vel, double *target, uint8_t *has_target, int64_t m,
                            const double *obstacles, double radio_radius, double sense_radius, double max_speed,
                            double *trace, int32_t trace_every, int64_t *counts, int64_t *n_singular,
                            int64_t *refused_tick, void *stream) {
    using namespace swarm;
    const LoopArgs loop{pos, pos_prev, vel, target, has_target, m, obstacles, nullptr, nullptr, max_speed,
                        trace, trace_every, n_singular, sense_radius, refused_tick, radio_radius};
    return run_loop(kLoopRadio, {ctx, n, ids, pos, nullptr, nullptr, nullptr, nullptr, tick_off, fsm, t0, ticks, dt,
                                 timeout, jitter, seed, kill_ticks, n_kill, -1.0, counts, nullptr, &loop, stream});
}

int swarm_update_loop_tasks(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                            const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks, double dt,
                            double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                            int32_t n_kill, double *vel, double *target, uint8_t *has_target, int64_t m,
                            const double *obstacles, double radio_radius, double sense_radius, double max_speed,
                            double *trace, int32_t trace_every, int64_t *counts, int64_t *n_singular,
                            int64_t *refused_tick, const swarm_tasks *tasks, int64_t *task_counts,
                            int64_t *n_guard, void *stream) {
    using namespace swarm;
    if (const int rc = check_tasks(ctx, n, tasks, stream)) return rc;
    const LoopArgs loop{pos, pos_prev, vel, target, has_target, m, obstacles, nullptr, nullptr, max_speed,
                        trace, trace_every, n_singular, sense_radius, refused_tick, radio_radius};
    return run_loop(kLoopRadio, {ctx, n, ids, pos, nullptr, nullptr, nullptr, nullptr, tick_off, fsm, t0, ticks, dt,
                                 timeout, jitter, seed, kill_ticks, n_kill, -1.0, counts, nullptr, &loop, stream,
                                 tasks, task_counts, n_guard});
}

int swarm_update_loop_channel(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                              const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks, double dt,
                              double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                              int32_t n_kill, double *vel, double *target, uint8_t *has_target, int64_t m,
                              const double *obstacles, double radio_radius, double sense_radius, double max_speed,
                              double *trace, int32_t trace_every, int64_t *counts, int64_t *n_singular,
                              int64_t *refused_tick, const swarm_tasks *tasks, int64_t *task_counts,
                              int64_t *n_guard, void *stream, const swarm_channel *ch, int64_t *link_counts) {
    using namespace swarm;
    if (const int rc = check_channel(ch)) return rc;
    if (tasks)
        if (const int rc = check_tasks(ctx, n, tasks, stream)) return rc;
    const LoopArgs loop{pos, pos_prev, vel, target, has_target, m, obstacles, nullptr, nullptr, max_speed,
                        trace, trace_every, n_singular, sense_radius, refused_tick, radio_radius};
    return run_loop(kLoopRadio, {ctx, n, ids, pos, nullptr, nullptr, nullptr, nullptr, tick_off, fsm, t0, ticks, dt,
                                 timeout, jitter, seed, kill_ticks, n_kill, -1.0, counts, nullptr, &loop, stream,
                                 tasks, task_counts, n_guard, ch, link_counts});
}

// swarm_update_loop_board (mboard NULL) and swarm_update_loop_board_moving (mboard == board).
static int board_loop(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                      const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks, double dt,
                      double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks, int32_t n_kill,
                      double *vel, double *target, uint8_t *has_target, int64_t m, const double *obstacles,
                      double radio_radius, double sense_radius, double max_speed, double *trace,
                      int32_t trace_every, int64_t *counts, int64_t *n_singular, int64_t *refused_tick,
                      const swarm_board *board, swarm_board *mboard, const swarm_board_state *state,
                      int64_t *task_counts, int64_t *n_guard, void *stream, const swarm_channel *ch,
                      int64_t *link_counts, swarm_board_overflow *overflow) {
    using namespace swarm;
    if (overflow) *overflow = swarm_board_overflow{SWARM_BOARD_FITS, 0, -1};
    if (const int rc = check_channel(ch)) return rc;
    if (const int rc = check_board(ctx, n, board, state)) return rc;
    SW_ARG(board->moving == (mboard != nullptr),
           mboard ? "the board does not move (swarm_update_loop_board takes it)"
                  : "a moving board needs swarm_update_loop_board_moving (this loop would read it as a frozen board)");
    // (contract U1-P.7) a board that has been placed on runs on from its own last tick: the new windows were
    // checked against it
    SW_ARG(!(mboard && mboard->placed_on && n > 0 && ticks > 0) || t0 == mboard->last_tick,
           "tasks have been placed on this board: the call must start at the tick after the last one run on it");
    const LoopArgs loop{pos, pos_prev, vel, target, has_target, m, obstacles, nullptr, nullptr, max_speed,
                        trace, trace_every, n_singular, sense_radius, refused_tick, radio_radius};
    TickRun r{ctx, n, ids, pos, nullptr, nullptr, nullptr, nullptr, tick_off, fsm, t0, ticks, dt,
              timeout, jitter, seed, kill_ticks, n_kill, -1.0, counts, nullptr, &loop, stream,
              nullptr, task_counts, n_guard, ch, link_counts};
    r.board = board;
    r.mboard = mboard;
    r.bstate = state;
    r.overflow = overflow;
    const int rc = run_loop(kLoopRadio, r);
    // (contract U1-A.7) the first tick of a call that ran has retired: a refused call keeps nothing, that too
    // (contract U1-P) ... and the board remembers the last tick run on it
    if (rc == SWARM_OK && mboard && n > 0 && ticks > 0 && r.boarded()) {
        mboard->life_fresh = false;
        mboard->last_tick = t0 + ticks;
    }
    return rc;
}

int swarm_update_loop_board(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                            const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks, double dt,
                            double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                            int32_t n_kill, double *vel, double *target, uint8_t *has_target, int64_t m,
                            const double *obstacles, double radio_radius, double sense_radius, double max_speed,
                            double *trace, int32_t trace_every, int64_t *counts, int64_t *n_singular,
                            int64_t *refused_tick, const swarm_board *board, const swarm_board_state *state,
                            int64_t *task_counts, int64_t *n_guard, void *stream, const swarm_channel *ch,
                            int64_t *link_counts, swarm_board_overflow *overflow) {
    return board_loop(ctx, n, ids, pos, pos_prev, tick_off, fsm, t0, ticks, dt, timeout, jitter, seed, kill_ticks,
                      n_kill, vel, target, has_target, m, obstacles, radio_radius, sense_radius, max_speed, trace,
                      trace_every, counts, n_singular, refused_tick, board, nullptr, state, task_counts, n_guard,
                      stream, ch, link_counts, overflow);
}

int swarm_update_loop_board_moving(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                                   const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks,
                                   double dt, double timeout, double jitter, uint64_t seed,
                                   const int64_t *kill_ticks, int32_t n_kill, double *vel, double *target,
                                   uint8_t *has_target, int64_t m, const double *obstacles, double radio_radius,
                                   double sense_radius, double max_speed, double *trace, int32_t trace_every,
                                   int64_t *counts, int64_t *n_singular, int64_t *refused_tick, swarm_board *board,
                                   const swarm_board_state *state, int64_t *task_counts, int64_t *n_guard,
                                   void *stream, const swarm_channel *ch, int64_t *link_counts,
                                   swarm_board_overflow *overflow) {
    return board_loop(ctx, n, ids, pos, pos_prev, tick_off, fsm, t0, ticks, dt, timeout, jitter, seed, kill_ticks,
                      n_kill, vel, target, has_target, m, obstacles, radio_radius, sense_radius, max_speed, trace,
                      trace_every, counts, n_singular, refused_tick, board, board, state, task_counts, n_guard, stream,
                      ch, link_counts, overflow);
}

int swarm_link_dropped(uint64_t seed, int64_t t, int32_t sid, int32_t rid, double loss) {
    return swarm::link_dropped(seed, t, sid, rid, loss) ? 1 : 0;
}

}  // extern "C"
