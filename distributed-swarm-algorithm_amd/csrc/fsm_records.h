// The per-agent records of a protocol run (protocol.hip packs the C-ABI's separate arrays into them at the
// start of a run and unpacks them at its end), shared with the coupled loop's physics step (physics.hip
// k_physics_loop), which reads an agent's state, alive flag and last-heard leader position from them.
#pragma once

#include "swarm_common.h"

namespace swarm {

// An agent's per-tick fields for the run, in one 8-byte record: a receiver touches one line for them
// instead of four, and the sweep streams 8 B per agent instead of 15.
//   x: the flag word -- byte 0 state, byte 1 alive, byte 2 bits (kHL: has_leader_pos, kH64, kDirty),
//      byte 3 tick phase = tick_off mod 10 in [0, 9] ((t + tick_off) % 10 == 0 iff (t + phase) % 10 == 0
//      for every tick t >= 0);
//   y: the agent's timer as a tick of the run (relative to t0), exact because the reference's clock is
//      t * dt: FOLLOWER -- the tick its last_heartbeat_time was set at (last_hb == double(t0 + y) * dt,
//      the timeout test evaluated on that value, as _check_election_timeout does, agent.py:223);
//      ELECTION_WAIT -- the first tick t at which now - election_wait_start > election_delay holds
//      (agent.py:234; found once, when the wait starts: the test is monotone in t for dt > 0), 0 = never.
//   kH64: the timer is in the caller's f64 arrays instead (a value no tick of the run represents, or
//      dt <= 0): the test reads them, as before.  kDirty: last_hb changed in the run; the unpack writes
//      double(t0 + y) * dt (a FOLLOWER entering ELECTION_WAIT writes it at once).
// Leader and leader position are write-only during a protocol run: one 16-byte record per agent (LRec), one
// line per heartbeat receiver instead of two.  (The coupled loop's physics step reads the position.)
constexpr uint32_t kHL = 1, kH64 = 2, kDirty = 4;
__host__ __device__ __forceinline__ uint8_t fw_state(uint32_t w) { return uint8_t(w); }
__host__ __device__ __forceinline__ uint8_t fw_alive(uint32_t w) { return uint8_t(w >> 8); }
__host__ __device__ __forceinline__ uint32_t fw_bits(uint32_t w) { return (w >> 16) & 0xFFu; }
__host__ __device__ __forceinline__ int32_t fw_phase(uint32_t w) { return int32_t(w >> 24); }
__host__ __device__ __forceinline__ uint32_t fw_make(uint8_t st, uint8_t al, uint32_t bits, int32_t ph) {
    return uint32_t(st) | (uint32_t(al) << 8) | (bits << 16) | (uint32_t(ph) << 24);
}

struct alignas(16) LRec {
    float x, y;      // leader_pos
    int32_t leader;  // leader
    int32_t pad;
};

// The records of n agents in one scratch buffer: the 8-byte records first, the LRecs after them at the
// next 16-byte boundary (n * 8 is only 8-byte aligned for odd n).
inline size_t lrec_offset(int64_t n) { return (size_t(n) * 8 + 15) & ~size_t(15); }
inline size_t fsm_records_bytes(int64_t n) { return lrec_offset(n) + size_t(n) * 16; }

// One physics step of the coupled update loop (contract U1; physics.hip): every alive agent steps from the
// snapshot pos_in to pos_out with its own record's state and last-heard leader position; dead agents'
// positions are copied through.  Queued on `s`; zero distances are added to *singular (device).
int launch_physics_loop(int64_t n, const int32_t *ids, const uint2 *rec, const LRec *lrec, const double *pos_in,
                        double *pos_out, double *vel, double *target, uint8_t *has_target, int64_t m,
                        const double *obstacles, const int32_t *row_ptr, const int32_t *col, double dt,
                        double max_speed, unsigned long long *singular, hipStream_t s);

// The sensed loop (contract U1-S; physics.hip): the separation neighbours of every tick are sensed from that
// tick's snapshot.  One LoopSense per call: the call's grid, the tick's binning and the device's verdict.
struct LoopSense {
    Grid g;                   // one grid for the call: the entry bounding box grown by the run's reach
    double r2;                // sense_radius squared
    double2 *psort;           // the tick's snapshot in cell-sorted order
    int32_t *sorted;          // the tick's binning: storage indices cell by cell, and the cells' offsets
    uint32_t *off;
    unsigned long long *st;   // device: [0] 0, or 1 + the call's first tick (from 0) refused for its window
                              // work; [2], [3] that tick's candidate pairs (a double's bits), largest window
};
// The call's grid from the bounding box of `pos` (one host wait; non-finite positions: SWARM_ERR_ARG with
// nothing written) and the verdict words cleared.  min_cell > 0: cells at least that wide (the radio loop
// reads a second window, of that radius, on the same grid).
int loop_sense_begin(swarm_ctx *ctx, int64_t n, const double *pos, double sense_radius, int32_t ticks, double dt,
                     double max_speed, LoopSense *ls, hipStream_t s, double min_cell = 0.0);
// Tick k of the call (from 0), queued on `s`: the snapshot binned, its window work judged on the device
// against swarm_build_rgg's limits, the cell-sorted copy of the snapshot.  offsets_by_search: the cells'
// offsets by search (bin_agents' sparse_grid) -- the loops' grid reaches far beyond the agents, by the run's
// reach on every side; swarm_physics_run_sensed keeps the dense form its figures were measured on.
int loop_sense_tick(swarm_ctx *ctx, int64_t n, const double *pos_in, int32_t k, LoopSense *ls, hipStream_t s,
                    bool offsets_by_search);
// The error of a call whose verdict words h (st read back) report a refused tick: the caller's wording
// (printf-style: "too dense ... at tick / step ..."), then the window figures; returns SWARM_ERR_RANGE.
int loop_sense_refusal(const unsigned long long *h, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// launch_physics_loop with the row of a sensor CSR replaced by the agent's 3 x 3 cell window of
// loop_sense_tick's binning (the snapshot is read through ls.psort); does nothing once a tick was refused.
int launch_physics_loop_sensed(int64_t n, const int32_t *ids, const uint2 *rec, const LRec *lrec, double *pos_out,
                               double *vel, double *target, uint8_t *has_target, int64_t m,
                               const double *obstacles, const LoopSense &ls, double dt, double max_speed,
                               unsigned long long *singular, hipStream_t s);

// What a kernel reads of an obstacle field (contract O1; swarm_obstacle_field in swarm_common.h): the grid's
// origin and shape, the cells' offsets and the cell lists as packed (x, y, r) triples.
struct ObsFieldView {
    const uint32_t *off;  // ncx * ncy + 1
    const double *tri;    // 3 doubles per listed obstacle
    double xmin, ymin, inv_cell;
    int64_t ncx, ncy;
};
inline ObsFieldView obstacle_field_view(const swarm_obstacle_field &f) {
    return {f.cell_off, f.tri, f.g.xmin, f.g.ymin, f.g.inv_cell, f.g.ncx, f.g.ncy};
}
// launch_physics_loop_sensed with the flat obstacle list replaced by the agent's cell list of a field: the
// same bits (contract O1), no LDS and no barriers.
int launch_physics_loop_sensed_field(int64_t n, const int32_t *ids, const uint2 *rec, const LRec *lrec,
                                     double *pos_out, double *vel, double *target, uint8_t *has_target,
                                     const ObsFieldView &field, const LoopSense &ls, double dt, double max_speed,
                                     unsigned long long *singular, hipStream_t s);

// Moving fields (contract O2; obstacle_field.hip).  A sensed entry point given a moving field's list:
//   moving_field_fetch   before the call's entry wait: the current list queued to the host;
//   moving_field_begin   after that wait, before anything is written: the call's grid and capacity
//                        (SWARM_ERR_ARG / SWARM_ERR_RANGE: nothing written), the buffers, the entry list kept;
//   moving_field_tick    per tick, before the physics kernel: the cell lists of the list as it stands, built on
//                        the device with no host wait; *view reads them.  A tick whose pairs exceed the capacity
//                        sets the field's error word and the stop word st[0] = 1 + k (the run is refused);
//   moving_field_advance per tick, after the physics kernel: every obstacle advances once, unless st[0] is set;
//   moving_field_restore_if_refused  (loops) the list back to its entry bits when st[0] is set;
//   moving_field_error   the error word queued into *h_word (pinned) for the call's final wait, and
//   moving_field_overflowed  its verdict: SWARM_ERR_RANGE with the error text.
// find_moving_field: find_obstacle_field for a field that moves (NULL for a static one or a flat list).
swarm_obstacle_field *find_moving_field(swarm_ctx *ctx, int64_t m, const double *obstacles);
int moving_field_fetch(swarm_obstacle_field *f, hipStream_t s);
int moving_field_begin(swarm_obstacle_field *f, int32_t ticks, double dt, bool keep_entry, hipStream_t s);
int moving_field_tick(swarm_obstacle_field *f, unsigned long long *st, int32_t k, ObsFieldView *view, hipStream_t s);
int moving_field_advance(swarm_obstacle_field *f, const unsigned long long *st, double dt, hipStream_t s);
int moving_field_restore_if_refused(swarm_obstacle_field *f, const unsigned long long *st, hipStream_t s);
int moving_field_error(swarm_obstacle_field *f, unsigned long long *h_word, hipStream_t s);
int moving_field_overflowed();

// Agent lifetimes (contract U1-J; agent_life.hip).  What the event kernel writes: the run's records and
// the caller's arrays, as run_ticks holds them.  A group of arrays the run does not have is NULL (vel: no loop;
// sb: no task loop) or has a width of zero (T: the 64-task board; Ks / Kt: the sparse board).
struct AgentEventArrays {
    int64_t n;
    uint2 *rec;
    LRec *lrec;
    double *last_hb, *wait_start, *delay;
    int32_t *tick_off;
    uint8_t *outbox;  // 2n, by tick parity
    double2 *vel, *target;
    uint8_t *has_target;
    uint8_t *sb;  // 2n sender bytes of a task loop, by tick parity
    int32_t T;
    unsigned long long *status_lo, *status_hi, *claim_out, *conflict_out;  // claim / conflict: 2n
    int32_t *tab_winner;
    float *tab_util;
    int32_t Ks, Kt;
    int32_t *b_status, *b_tab_task, *b_tab_winner;
    float *b_tab_util;
    int32_t *b_claim_out, *b_conflict_out;  // 2n rows each
    int64_t t0;
    double dt;
};
// agent_life_begin  a call over the ticks t0+1 .. t0+ticks: its schedule (host only), and -- when it has events --
//                   the handle's event list on the device (uploaded once per change of the windows, queued on s);
// launch_agent_events  tick t's segment, one launch over its events alone (the caller asks sched.has_events first).
int agent_life_begin(swarm_agent_life *h, int64_t t0, int32_t ticks, AgentSchedule *sched, hipStream_t s);
int launch_agent_events(const swarm_agent_life *h, const AgentSchedule &sched, int64_t t, const AgentEventArrays &a,
                        hipStream_t s);

}  // namespace swarm
