// Shared host/device plumbing for libswarm.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/swarm.h"
#include "grid_shape.h"  // struct Grid (here so that headers without hipCUB can hold one) and its shaping
#include "agent_life.h"  // AgentEvent, AgentSchedule (host-only arithmetic)

namespace swarm {

constexpr int kBlock = 256;   // threads per workgroup: 4 waves of 64
constexpr int kWave = 64;
constexpr int kElectCounters = 4;  // per-round election counters (elect.hip C_CHG..C_GHOST)

void set_error(const char *fmt, ...);

// Scratch slots owned by a ctx; each grows on demand (never shrinks until destroy).
enum Slot {
    S_LEADER_B = 0,   // election: second leader buffer (dense)
    S_ACT,            // election: per-agent append stamp (frontier)
    S_LIST,           // election: change lists, both round parities (frontier)
    S_CHANGES,        // election: per-round change counters (device)
    S_ESTATS,         // election: per-round active/edge counters (device)
    S_KEYS_IN,        // binning: cell keys
    S_KEYS_OUT,
    S_VALS_IN,        // binning: agent indices
    S_VALS_OUT,
    S_CELL_START,
    S_CELL_END,
    S_CUB_TMP,        // hipcub temporary storage
    S_BBOX,           // bounding box (device)
    S_ASTATS,         // allocation counters (device)
    S_DEG,            // graph builder: degrees
    S_TILEMAX,        // dense allocation: per (task, agent tile) max claim
    S_ORDER,          // dense allocation: agents in ascending ID order
    S_TMP0,
    S_TMP1,
    S_AUC_OFF,        // auction: candidate-list offsets (int64, n + 1)
    S_AUC_K,          // auction: candidate tasks
    S_AUC_V,          // auction: candidate values (f32)
    S_AUC_OUT,        // auction: dropped-out flags
    S_AUC_KEY,        // auction: per-task bid keys (u64)
    S_AUC_LIST,       // auction: bidder lists, targets, keys, counters, per-round log
    S_FSM_MAIL,       // protocol: mail bitmap (1 bit per agent) + list counters
    S_FSM_LIST,       // protocol: receivers of the current tick
    S_FSM_FROM,       // protocol: each receiver's sender when it has exactly one
    S_FSM_SEND,       // protocol: per-workgroup sender segments + counts
    S_DEFER,          // allocation: guard-band tasks deferred to the libm pass (list + per-task flags)
    S_FPAIRS,         // allocation: the deferred tasks' guard-band pairs (device -> host)
    S_OVR,            // allocation: host libm decisions for those pairs (host -> device)
    S_ENC_FLAGS,      // codec: tile ticket + per-tile look-back words (kept across calls, tagged by epoch)
    S_CHECK,          // election: the 16-bit column check's verdict word
    S_FSM_FLAGS,      // protocol: per-agent records of a run (flag word + timer tick; leader + leader position)
    S_SENSE_POS,      // sensed physics: the second position buffer of the run's double buffering
    S_SENSE_SORTED,   // sensed physics: the step's positions in cell-sorted order
    S_SENSE_STATE,    // sensed physics: stop word, singular count and the refused step's window figures
    S_LOOP_SNAP,      // sensed update loop: the caller's arrays as they were at entry (restored on a refusal)
    S_RADIO_OUTBOX,   // radio update loop: the tick's inbound outbox bytes in cell-sorted order
    S_RADIO_CELLS,    // radio update loop: one byte per grid cell, set when the cell holds a sender
    S_TASK_COUNTS,    // task update loop: the per-tick task counters (sharded) and their sums
    S_TASK_SENDERS,   // task update loop: one byte per agent and tick parity, what it sent (outbox + task bits)
    S_LINK_COUNTS,    // lossy update loops: the per-tick link counters (sharded) and their sums
    S_REORDER_BITS,   // reorder: the entry checks' verdict word and the permutation check's bitmap (1 bit per row)
    S_REORDER_INV,    // reorder: the inverse of a permutation (n int32)
    S_REORDER_DEG,    // reorder: the relabelled rows' degrees (n + 1 int32); the plan's moved-row counter
    S_REORDER_POS,    // reorder: the positions in input order (n x 2 f64)
    S_REORDER_ORDER,  // reorder: the cell order of the input positions (n int32)
    S_CENSUS,         // task census: the verdict word, the holder cursor and one packed best-entry key per task
    S_NUM
};

}  // namespace swarm

namespace swarm {
// Sharded auction state kept between swarm_auction_begin and the per-round calls (pointers into
// this ctx's scratch slots; see auction.hip).
struct AucPersist {
    int64_t n = 0, t = 0, npairs = 0;
    float eps = 0.f;
    const int32_t *ids = nullptr;
    int64_t *off = nullptr;
    int32_t *ck = nullptr;
    float *cv = nullptr;
    uint32_t *sorted_ids = nullptr;
    int32_t *order = nullptr;
    uint8_t *out = nullptr;
    unsigned long long *ring = nullptr;
    bool ready = false;
};
}  // namespace swarm

// An obstacle field (contract O1; obstacle_field.hip builds it, physics.hip reads it).  Everything it points to
// is owned by the field until swarm_obstacle_field_destroy (or its ctx's destroy).
struct swarm_obstacle_field {
    int64_t m = 0;
    double *obs = nullptr;         // device: the field's own copy of the list, m x 3 (the key of find_obstacle_field)
    uint32_t *cell_off = nullptr;  // device: ncx * ncy + 1
    double *tri = nullptr;         // device: the cell lists as packed (x, y, r) triples, in list order
    swarm::Grid g{};
    std::vector<uint32_t> cell_off_host;
    std::vector<int32_t> idx_host;  // the cell lists as obstacle indices (swarm_obstacle_field_read)
    // A moving field (contract O2; obstacle_field.hip): `obs` is the current list, in/out; the members
    // above describe the creation list (or the last refresh).  The buffers below grow on demand, `obs` never moves.
    int64_t live = 0;                 // the live obstacles of the list the host lists above describe
    bool moving = false;
    double *vel = nullptr;            // device: m x 2
    double *entry = nullptr;          // device: the list as it was at a loop's entry (restored on a refused tick)
    std::vector<double> vel_host;     // the velocities, checked finite (the call's box is planned from them)
    std::vector<double> list_host;    // the list as fetched at a call's entry
    swarm::Grid call_g{};             // the call's grid
    int64_t capacity = 0;             // pairs the call's buffers hold (obstacle_motion.h, obs_pair_capacity)
    unsigned long long *start = nullptr;  // device: m + 1 pair counts, then their exclusive sums
    uint32_t *keys[2] = {};           // device: the pairs' cell keys, emitted and sorted
    int32_t *vals[2] = {};            // device: the pairs' obstacle indices, emitted and sorted
    uint32_t *dyn_off = nullptr;      // device: the tick's cell offsets
    double *dyn_tri = nullptr;        // device: the tick's lists as packed triples
    void *cub_tmp = nullptr;          // device: hipCUB's temporary storage
    unsigned long long *err = nullptr;  // device: [0] set when a tick's pairs exceeded the capacity
    size_t cap_pairs = 0, cap_cells = 0, cap_tmp = 0;  // what the buffers above hold
};

// A task board (contract U1-B; task_board.hip builds it, protocol.hip reads it).  Everything it points to is
// owned by the board until swarm_board_destroy (or its ctx's destroy).
struct swarm_board {
    int64_t T = 0;
    double *tpos = nullptr;        // device: the caller's positions, T x 2 (by task index: the claim handler's)
    int8_t *treq = nullptr;        // device: T
    uint32_t *cell_off = nullptr;  // device: ncx * ncy + 1
    double *sxy = nullptr;         // device: the tasks' positions in cell-sorted order, T x 2
    int32_t *sir = nullptr;        // device: (task index, treq) in cell-sorted order, T x 2
    unsigned long long *verdict = nullptr;       // device: the entry check's word
    unsigned long long *verdict_host = nullptr;  // pinned: its copy, read after the call's entry wait
    swarm::Grid g{};
    int64_t longest = 0;
    std::vector<uint32_t> cell_off_host;
    std::vector<int32_t> idx_host;
    // A moving board (contract U1-M; task_board.hip): `tpos` is the current list `cur`, in/out; `sxy`
    // and `sir` are rewritten by every tick's device build; the members above describe the creation list (or the
    // last refresh).  The key and value buffers are T long; dyn_off and cub_tmp grow on demand.
    bool moving = false;
    double *lag = nullptr;            // device: T x 2, the list one advance behind `cur` (the claim handler's)
    double *vel = nullptr;            // device: T x 2
    double *entry = nullptr;          // device: cur then lag as they were at a loop's entry (a refused tick)
    double *box = nullptr;            // device: the span-box reduction's partials, then its four doubles
    uint32_t *keys[2] = {};           // device: the tasks' cell keys, by task and sorted
    int32_t *vals[2] = {};            // device: the task indices, by task and sorted
    uint32_t *dyn_off = nullptr;      // device: the tick's cell offsets
    void *cub_tmp = nullptr;          // device: hipCUB's temporary storage
    size_t cap_cells = 0, cap_tmp = 0;  // what the two buffers above hold
    swarm::Grid call_g{};             // the call's grid
    // Lifetimes (contract U1-A; task_life.h): one window of absolute ticks per task, on a moving board
    // only.  `present` is rewritten by every tick's key pass; the host keeps the schedule of retiring ticks.
    int64_t *life_open = nullptr, *life_close = nullptr;  // device: T each; NULL: every task always present
    uint8_t *present = nullptr;                           // device: T, the tick's presence by task index
    std::vector<int64_t> close_ticks;                     // the closing ticks, ascending, each once
    bool life_fresh = false;  // set or changed, and no call has run since: the next call's first tick retires
    bool alive() const { return life_open != nullptr; }
    // Placing (contract U1-P; task_place.h): the last tick a loop ran on the board, the requests'
    // staging buffer, the mask of the slots a place has just written (all zero between places) and the purge pass's
    // per-wave counts.
    int64_t last_tick = -1;       // -1: no loop call has run on this board
    bool placed_on = false;       // a place has succeeded: the next call must start at last_tick + 1
    void *place_buf = nullptr;    // device: one place's requests and the old windows of their slots
    uint8_t *placed = nullptr;    // device: T
    void *purge_part = nullptr;   // device: one count per wave of the purge pass
    size_t cap_place = 0, cap_part = 0;
};

// Agent lifetimes (contract U1-J; agent_life.h has the schedule, agent_life.hip the handle and the event
// kernel).  The handle is found by the loops from the alive array they are given anyway; it owns the sorted event
// list and its device copy, nothing else.
struct swarm_agent_life {
    int64_t n = 0;
    uint8_t *alive = nullptr;     // device: the caller's alive flags (the key of find_agent_life)
    int32_t *tick_off = nullptr;  // device: the caller's tick offsets, written at a boot
    std::vector<int64_t> boot, death;     // the windows, by storage row
    std::vector<swarm::AgentEvent> events;  // every event, sorted (agent_life_events)
    std::vector<uint32_t> entries_host;   // the events' entries in that order, as uploaded
    uint32_t *entries = nullptr;          // device: their copy (hipMalloc, grown on demand)
    size_t cap_entries = 0;
    bool uploaded = false;  // `entries` holds entries_host
    bool dead = false;      // destroyed: the emptied struct rests on the ctx's life_graves for a while
};

struct swarm_ctx {
    std::vector<swarm_obstacle_field *> fields;  // the live obstacle fields created on this ctx
    std::vector<swarm_board *> boards;           // the live task boards created on this ctx
    std::vector<swarm_agent_life *> lives;       // the live agent-lifetime handles created on this ctx
    std::vector<swarm_agent_life *> life_graves;  // the handles destroyed last (emptied structs, as board_graves)
    // The boards destroyed last (their memory freed, the structs kept): a new board cannot take the address of a
    // handle that has just died, so a stale handle is told from a live board whatever the allocator does.
    std::vector<swarm_board *> board_graves;
    swarm::AucPersist auc;         // sharded auction between begin and the round calls
    int device = 0;
    void *slot[swarm::S_NUM] = {};
    size_t cap[swarm::S_NUM] = {};
    void *host_pinned = nullptr;   // small pinned staging buffer for scalar/array readback
    size_t host_cap = 0;
    void *host_mapped = nullptr;   // coherent mapped host buffer the device writes (election read-back)
    void *mapped_dev = nullptr;
    size_t mapped_cap = 0;
    int64_t step_rows = 0;         // frontier stepper: owned rows / agents (rows + ghosts)
    int64_t step_all = 0;
    int64_t step_lo = 0;           // frontier stepper: the owned rows are [step_lo, step_lo + step_rows)
    const int16_t *step_c16 = nullptr;  // frontier stepper: 16-bit columns of the shard graph, or NULL
    bool step_c16_esc = false;          // step_c16 holds escapes (read through the int32 columns)
    bool step_c16_checked = false;      // step_c16 passed the column check against the stepped graph
    std::vector<const int16_t *> esc_built;  // column buffers swarm_graph_compact_escaped last wrote
    struct C16Built {                        // column buffers swarm_graph_compact last wrote (all deltas fit)
        const int16_t *c16;
        const void *rp;
        const int32_t *col;
        int64_t n, e_total;
    };
    std::vector<C16Built> c16_built;
    struct PairsBuilt {                      // two-hop indexes swarm_graph_pairs_fill last wrote (pairs.hip)
        const int32_t *rp2;
        const int16_t *col2;
        const int32_t *rp, *col;
        int64_t n;
    };
    std::vector<PairsBuilt> pairs_built;
    int step_rd_agent = 0;         // frontier stepper: the marks the next round reads are in agent order
    int step_wr_agent = 0;         // ... and the next round writes its marks in agent order (the tail)
    int step_cleared_for = 0;      // frontier stepper: the round whose stamp clear the round before it has done
    hipStream_t side = nullptr;    // a second stream for work that overlaps the caller's (side_stream)
    hipEvent_t side_ev[2] = {};    // fork / join events
    void *enc_flags = nullptr;     // codec one-pass encode: the S_ENC_FLAGS buffer last zeroed ...
    size_t enc_cap = 0;            // ... and its size
    uint32_t enc_epoch = 0;        // ... the epoch tag of the last call (look-back words carry it)
    unsigned long long fold_epoch = 0;  // allocation: the last epoch k_fold_stats wrote to mapped memory
};

namespace swarm {

int comm_allreduce_max_u64(swarm_comm *comm, unsigned long long *buf, size_t count, hipStream_t s);
int comm_allgather_u64(swarm_comm *comm, const unsigned long long *send, size_t count, unsigned long long *recv,
                       hipStream_t s);
int comm_rank(const swarm_comm *comm, int *rank, int *nranks);

// Returns a device buffer of at least `bytes` for `s` (nullptr + error on failure: the ctx
// belongs to another device -> scratch_code() SWARM_ERR_ARG, else SWARM_ERR_OOM).
void *scratch(swarm_ctx *ctx, Slot s, size_t bytes);
int scratch_code();
bool ctx_on_current_device(const swarm_ctx *ctx);
void *pinned(swarm_ctx *ctx, size_t bytes);
// The ctx's side stream and a fork / join event pair (created on first use, on the ctx's device):
// record fork on the caller's stream, wait for it on *side, launch there, record join on *side,
// wait for join on the caller's stream.
int side_stream(swarm_ctx *ctx, hipStream_t *side, hipEvent_t *fork, hipEvent_t *join);
void *mapped(swarm_ctx *ctx, size_t bytes, void **dev);
// Host wait for a device-written word of mapped memory to equal v (a spin: a waiting host thread stays
// on its core, where a stream / event synchronisation may yield it -- and the next call's launches then
// start from a cold core); hipStreamQuery every 256 spins reports a failed stream, and a stream that
// finished without the write is an error.
int wait_mapped_word(const unsigned long long *w, unsigned long long v, hipStream_t s, const char *what);

// The live field of ctx whose own list `obstacles` is (exactly its pointer, with its m), or NULL: any other
// pointer is a flat list.  The key is memory the library owns until the field is destroyed, so no allocator can
// hand it to somebody else while the field lives.
inline const swarm_obstacle_field *find_obstacle_field(const swarm_ctx *ctx, int64_t m, const double *obstacles) {
    if (obstacles)
        for (const swarm_obstacle_field *f : ctx->fields)
            if (f->obs == obstacles && f->m == m) return f;
    return nullptr;
}
// Frees a field's memory (the caller has taken it off its ctx's list and made sure the device is done with it).
void free_obstacle_field(swarm_obstacle_field *f);
// The same for a task board (task_board.hip); live_board: `b` is a live board of ctx.
void free_board(swarm_board *b);
inline bool live_board(const swarm_ctx *ctx, const swarm_board *b) {
    for (const swarm_board *q : ctx->boards)
        if (q == b) return true;
    return false;
}
// The live lifetime handle of ctx whose alive array `alive` is (with its n), or NULL (agent_life.hip frees them).
inline swarm_agent_life *find_agent_life(const swarm_ctx *ctx, int64_t n, const uint8_t *alive) {
    if (alive)
        for (swarm_agent_life *h : ctx->lives)
            if (!h->dead && h->alive == alive && h->n == n) return h;
    return nullptr;
}
void free_agent_life(swarm_agent_life *h);
// A moving board's call (contract U1-M; task_board.hip), in the order a loop uses them: the span-box reduction
// queued before the call's entry wait (its four doubles land in verdict_host[1..4]); after the wait the call's
// grid, the buffers and the entry snapshot (SWARM_ERR_ARG before anything is written: a box without a finite
// extent); per tick the cell lists of `cur` on that grid, then -- after the tick's kernels -- lag <- cur and the
// advance, nothing once the stop word is set; at the end both lists back to their entry bytes if it is.
int moving_board_box(swarm_board *b, double dt, int32_t ticks, hipStream_t s);
int moving_board_begin(swarm_board *b, hipStream_t s);
int moving_board_tick(swarm_board *b, int64_t t, hipStream_t s);
// (contract U1-A) does tick t of a call that starts after tick t0 retire; the retire pass over n status rows of Ks
// slots (after moving_board_tick(t): it reads the tick's presence bytes); a call that ran is no longer the first.
bool moving_board_retires(const swarm_board *b, int64_t t0, int64_t t);
int moving_board_retire(const swarm_board *b, const unsigned long long *st, int64_t n, int32_t Ks, int32_t *status,
                        hipStream_t s);
int moving_board_advance(swarm_board *b, const unsigned long long *st, double dt, hipStream_t s);
int moving_board_restore_if_refused(swarm_board *b, const unsigned long long *st, hipStream_t s);

}  // namespace swarm

#define SW_HIP(call)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            swarm::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call,                \
                             hipGetErrorString(e_));                                     \
            return SWARM_ERR_HIP;                                                        \
        }                                                                                \
    } while (0)

#define SW_ARG(cond, msg)                                                                \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            swarm::set_error("invalid argument: %s", msg);                               \
            return SWARM_ERR_ARG;                                                        \
        }                                                                                \
    } while (0)

#define SW_ALLOC(ptr, ctx, slot, bytes)                                                  \
    do {                                                                                 \
        (ptr) = static_cast<std::remove_reference_t<decltype(ptr)>>(swarm::scratch((ctx), (slot), (bytes)));      \
        if (!(ptr)) return swarm::scratch_code();                                        \
    } while (0)

// Launch-error check after a kernel launch.
#define SW_LAUNCHED() SW_HIP(hipGetLastError())

namespace swarm {

// The election's entry points for comm.hip (the RCCL round loop), defined in elect.hip: one stepper round, the
// ghost update of both borders, the device per-round totals (kElectCounters each) of rounds t0..t1, the check
// of the stepper's 16-bit columns, the stamp layout's switch point for an n-agent swarm (elect_schedule.h,
// il_min_for) and whether stepper round t is a dense sweep.
int frontier_round_stepper(swarm_ctx *ctx, int t, const int32_t *rp, const int32_t *col, int32_t *L0,
                           int32_t *L1, hipStream_t s);
int frontier_ghosts_both(swarm_ctx *ctx, int t, const int32_t *rp, const int32_t *col, int64_t b_lo, int64_t n_lo,
                         const int32_t *in_lo, int64_t b_hi, int64_t n_hi, const int32_t *in_hi, int32_t *L0,
                         int32_t *L1, hipStream_t s);
int frontier_round_totals(swarm_ctx *ctx, int t0, int t1, unsigned long long *dtot, hipStream_t s);
int frontier_check_compact(swarm_ctx *ctx, const int32_t *rp, const int32_t *col, hipStream_t s);
int64_t frontier_il_min(int64_t n);
bool frontier_round_dense(int t);

// SWARM_BATCH_DOUBLING=1: the election loops' batches double plainly (next_round_batch's A/B aid)
inline bool batch_doubling_only() {
    static const bool on = [] {
        const char *e = getenv("SWARM_BATCH_DOUBLING");
        return e && e[0] == '1';
    }();
    return on;
}

// Grid for a grid-stride kernel over `work` items with `per_block` items per block pass.
inline unsigned grid_for(int64_t work, int64_t per_block, unsigned cap = 8192) {
    int64_t g = (work + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return static_cast<unsigned>(g);
}

// The cell of coordinate v on one axis of a Grid (binning.h bins by it; here so that a kernel that only reads
// a binning needs no hipCUB).
__device__ __forceinline__ int64_t cell_coord(double v, double vmin, double inv_cell, int64_t nc) {
    double f = floor((v - vmin) * inv_cell);
    if (!(f >= 0.0)) return 0;            // also catches NaN
    if (f >= double(nc - 1)) return nc - 1;
    return int64_t(f);
}

}  // namespace swarm
