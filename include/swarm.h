/*
 * swarm.h -- C-ABI of libswarm.so, the MI355X (gfx950) swarm-step library.
 *
 * The reference has no FFI: its boundary is the Python module `agent` whose handlers are
 * called once per message (agent.py:197-214 dispatch).  These entry points replace the
 * *batched* form of those handlers -- one call runs a whole synchronous round (or all rounds
 * to convergence) for every agent at once.  Python binds them with ctypes
 * (distributed-swarm-algorithm_amd/swarm_amd/_lib.py; INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (HBM), borrowed: the library never frees them.
 *     Positions are interleaved float64 pairs (x0, y0, x1, y1, ...), i.e. agent.py:47
 *     `self.position` / task['pos'].
 *   - Agents are addressed by storage index i in [0, n); ids[i] (int32, >= 0, distinct) is
 *     the protocol ID (agent.py:26 `agent_id`).  The storage order is the caller's choice; the
 *     batched Python layer stores agents in spatial (grid-cell) order for locality.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Work is
 *     stream-ordered; the documented host sync points are the host-pointer outputs
 *     (rounds_exec, changes_per_round, stats, n_edges).
 *   - Return 0 (SWARM_OK) on success, > 0 for a soft condition, < 0 on error;
 *     swarm_last_error() returns the calling thread's last message.
 *   - Scratch memory is owned by a swarm_ctx (grows on demand, freed by swarm_ctx_destroy).
 *     A ctx is bound to the device that was current when it was created; one ctx per thread.
 */
#ifndef SWARM_H
#define SWARM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWARM_OK 0
#define SWARM_NOT_CONVERGED 1  /* max_rounds reached without a zero-change round */
#define SWARM_ERR_ARG (-1)     /* invalid argument (sizes, NULL pointers, ranges) */
#define SWARM_ERR_HIP (-2)     /* HIP runtime error (message has the hipError string) */
#define SWARM_ERR_OOM (-3)     /* scratch allocation failed */
#define SWARM_ERR_RANGE (-4)   /* a size exceeds the index type (e.g. >= 2^31 edges) */
#define SWARM_ERR_STALE (-5)   /* swarm_allocate_indexed: positions moved since swarm_cell_index */

/* Agent states as stored in the uint8 state array (agent.py:19-22 AgentState values). */
#define SWARM_FOLLOWER 1
#define SWARM_ELECTION_WAIT 2
#define SWARM_LEADER 3

/* Election execution strategies.  Both are exact: identical leaders, states, rounds_exec
 * and per-round change counts. */
#define SWARM_ELECT_DENSE 0    /* every agent gathers every round (Jacobi sweep) */
#define SWARM_ELECT_FRONTIER 1 /* dense sweeps while many agents change, then only the agents
                                  marked by last round's risers gather (sparse rounds) */
#define SWARM_ELECT_TIMED 0x100 /* OR into mode: time every kernel with HIP events (stats) */
#define SWARM_ELECT_TRUST_C16 0x200 /* OR into mode (swarm_elect_compact*): the caller vouches that col16 was
                                       written by swarm_graph_compact on this ctx from the same row_ptr / col
                                       and n, and that none of the three changed since; the 16-bit column
                                       check and the edge-count read-back are then skipped (no host wait
                                       before the first round).  Without such a record on the ctx the call
                                       checks the columns as usual. */

/* Allocation execution strategies (all exact). */
#define SWARM_ALLOC_AUTO 0
#define SWARM_ALLOC_BINNED 1   /* cell-list candidates within the claim radius */
#define SWARM_ALLOC_DENSE 2    /* every agent x every task, ID-ordered tiles */

typedef struct swarm_ctx swarm_ctx;

/* A uniform cell grid over agent positions (swarm_cell_index). */
typedef struct swarm_grid {
    double xmin, ymin, xmax, ymax;  /* bounding box of the indexed positions */
    double cell, inv_cell;          /* cell side (>= the requested one if the grid was capped) */
    int64_t ncx, ncy;               /* cells per row, rows */
} swarm_grid;

typedef struct swarm_alloc_stats {
    int64_t n_claims;        /* TASK_CLAIM messages the round produced (agent.py:302) */
    int64_t n_conflicts;     /* TASK_CONFLICT messages the resolver emitted (agent.py:322,325) */
    int64_t n_flagged;       /* claims/decisions inside the libm guard band */
    int64_t n_candidates;    /* agent x task pairs evaluated exactly in fp64 */
    int64_t n_overflow;      /* tasks whose claims exceeded the on-chip list (slow exact path) */
    int64_t mode_used;       /* SWARM_ALLOC_BINNED or SWARM_ALLOC_DENSE */
    int64_t n_resolved;      /* tasks with a guard-band pair, decided with the host's libm pow */
} swarm_alloc_stats;

typedef struct swarm_elect_stats {
    int64_t rounds_launched; /* rounds issued (>= rounds_exec; extra ones are no-ops); a pair launch issues two */
    int64_t active_total;    /* agents gathered (DENSE: all; SPARSE: marked), rounds 1..rounds_exec */
    int64_t edges_total;     /* CSR edges visited, summed over rounds 1..rounds_exec */
    int64_t changes_total;   /* leader changes, summed over rounds */
    double gather_ms;        /* SWARM_ELECT_TIMED: device time of every launched round kernel */
    double apply_ms;         /* always 0 (one kernel per round); kept for layout stability */
    int64_t gather_launches; /* kernel launches behind gather_ms (all launched rounds; a pair launch is one) */
    int64_t dense_rounds;    /* rounds executed as a full DENSE sweep */
    double bytes_total;      /* algorithmic HBM bytes of rounds 1..rounds_exec */
    double sparse_ms;        /* SWARM_ELECT_TIMED: device time of every launched sparse round */
    int64_t sparse_launches; /* SWARM_ELECT_TIMED: sparse kernel launches (incl. no-ops; a pair launch is one) */
    double sparse_bytes;     /* algorithmic HBM bytes of the executed sparse rounds */
    int64_t pair_launches;   /* launches that ran two rounds each (swarm_elect_pairs); 0 elsewhere */
} swarm_elect_stats;

const char *swarm_last_error(void);
/* "swarm-mi355x <version> (gfx950) src=<16 hex>": the hex digits are the sha256 prefix of the
 * sources the library was built from (csrc/Makefile HASHED), so a stale build is detectable. */
const char *swarm_version(void);

int swarm_ctx_create(swarm_ctx **out);
int swarm_ctx_destroy(swarm_ctx *ctx);

/*
 * Leader election to convergence (contract E2).
 * Replaces: SwarmAgent._handle_election_acclaim (agent.py:263-275) and
 * SwarmAgent._handle_heartbeat (agent.py:243-261) applied by every agent to every
 * neighbour's re-advertised leader each round, starting from the state
 * _check_election_timeout leaves after a win (agent.py:234-241: LEADER, leader_id = id).
 *   round t:  leader[v] <- max(leader[v], max_{u in N(v)} leader[u])   (synchronous)
 *   stop after the first round with zero changes; rounds_exec counts that round.
 *   state[v] = SWARM_LEADER iff leader[v] == ids[v], else SWARM_FOLLOWER.
 * row_ptr/col: CSR of N(v) (who v hears) over storage indices; FRONTIER mode requires it
 * symmetric (a riser marks the agents in its own row) -- use swarm_elect_directed otherwise.
 * leader (device, n): output.  changes_per_round (host, capacity max_rounds, may
 * be NULL): per-round change counts for rounds 1..rounds_exec.  stats (host) may be NULL.
 * Returns SWARM_NOT_CONVERGED if max_rounds rounds all changed something.
 */
int swarm_elect(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col,
                const int32_t *ids, int32_t *leader, uint8_t *state, int32_t max_rounds,
                int32_t mode, int32_t *rounds_exec, int64_t *changes_per_round,
                swarm_elect_stats *stats, void *stream);

/* Same for a directed neighbour graph (agent.py:59-65: update_sensors' per-agent neighbour
 * lists need not be symmetric).  hear_row_ptr/hear_col (device) is the transpose of
 * row_ptr/col -- for each agent, the agents that hear it -- through which FRONTIER rounds mark
 * the agents a riser can change next round.  hear_row_ptr[n] must equal row_ptr[n]
 * (SWARM_ERR_ARG otherwise).  DENSE mode ignores it. */
int swarm_elect_directed(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col,
                         const int32_t *hear_row_ptr, const int32_t *hear_col, const int32_t *ids,
                         int32_t *leader, uint8_t *state, int32_t max_rounds, int32_t mode,
                         int32_t *rounds_exec, int64_t *changes_per_round, swarm_elect_stats *stats,
                         void *stream);

/* Compact (16-bit) columns of a symmetric int32 CSR for the elections (an MI355X layout, no reference
 * counterpart): col16[k] = col[k] - (v & ~63) for every edge k of row v, i.e. each neighbour as a
 * delta from its row's 64-agent base.  In a spatial storage order (swarm_cell_order) a neighbour lies
 * within about one grid row of its agent, so the deltas fit and every column read moves half the
 * bytes.  col16 (device, row_ptr[n] int16, caller-allocated).  Returns SWARM_ERR_RANGE (col16
 * unusable) when a delta does not fit in 16 bits.  Rebuild it whenever the graph changes. */
int swarm_graph_compact(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col, int16_t *col16,
                        void *stream);

/* swarm_graph_compact that never refuses: a delta outside [-32767, 32767] is stored as -32768 (an escape)
 * and the elections read that neighbour from the int32 columns (col must stay alive beside col16).  For
 * shard graphs, whose ghost rows sit in blocks away from the owned rows: the frontier stepper
 * takes these columns through swarm_frontier_set_compact_escaped / swarm_shard.col16_escaped.
 * *n_escaped (host): the escaped edges.  < 2^30 edges. */
int swarm_graph_compact_escaped(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col,
                                int16_t *col16, int64_t *n_escaped, void *stream);

/* swarm_elect reading the graph's compact columns (swarm_graph_compact of the same row_ptr/col -- never
 * swarm_graph_compact_escaped's, which only the frontier stepper reads; col16 NULL: same as swarm_elect).  Same results, same stats.  With col16 it takes graphs of up to
 * 2^31 - 2^20 edges (the 16-bit columns' 32-bit byte offsets), so a 1.6e9-edge swarm (C5's 100M agents
 * on one GPU) runs on 32-bit row offsets; without, < 2^30 edges as swarm_elect. */
int swarm_elect_compact(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col, const int16_t *col16,
                        const int32_t *ids, int32_t *leader, uint8_t *state, int32_t max_rounds, int32_t mode,
                        int32_t *rounds_exec, int64_t *changes_per_round, swarm_elect_stats *stats, void *stream);

/* The two-hop index of a symmetric int32 CSR, for swarm_elect_pairs (an MI355X layout, no reference
 * counterpart).  Row v of (rp2, col2) holds v's CSR row first, in CSR order, then every agent at exactly two
 * hops: no duplicates, never v itself; col2 holds 16-bit deltas from the row's 64-agent base (v & ~63), as
 * swarm_graph_compact's columns.  Built on the device in two calls, once per graph version -- outside a
 * steady-state step, as the 16-bit columns and the allocation's cell index are:
 *   swarm_graph_pairs_count  counts[v] (device, n int32) = row v's length;
 *   the caller forms rp2 (device, n + 1 int32) = the exclusive prefix sums of counts, allocates col2
 *   (device, rp2[n] int16), and
 *   swarm_graph_pairs_fill   writes the rows.
 * Either call returns SWARM_ERR_RANGE, and the caller then simply elects without pair rounds, when an agent
 * within two hops lies more than 32767 slots from its row's base (expected for 100M agents on one GPU), when a
 * row is longer than max_row (hub rows: a pair launch walks a riser's row with 4 or 8 lanes), or when the index
 * has 2^31 - 2^20 entries or more.  At 10M agents of degree 16 the index has ~0.5 G entries (~1 GB).  The ctx
 * remembers the index it filled; rebuild it whenever the graph changes.  0 < n < 2^30.  Both synchronise. */
int swarm_graph_pairs_count(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col, int32_t max_row,
                            int32_t *counts, void *stream);
int swarm_graph_pairs_fill(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col, const int32_t *rp2,
                           int16_t *col2, void *stream);

/* swarm_elect_compact whose FRONTIER tail runs two synchronous rounds per kernel launch (same election, same
 * results, same per-round change counts; replaces the same handlers as swarm_elect, agent.py:243-275).  Once a
 * round has changed fewer than SWARM_PAIR_BELOW agents (default: 16 384, eight per resident workgroup), each launch gathers every listed
 * agent's two-hop row from the one buffer that holds L_t and writes L_{t+2}: max over N[v] is round t+1's value,
 * max over the whole row round t+2's ("pair rounds").  rp2 / col2 must be the index this ctx
 * filled from these row_ptr / col (SWARM_ERR_ARG otherwise); col16 as swarm_elect_compact's.  A single round is
 * launched where only one is left before max_rounds.  stats->pair_launches counts the two-round launches;
 * rounds_launched keeps counting rounds.  DENSE mode, SWARM_TAIL_WG and SWARM_ROUND_LOG run without pairs. */
int swarm_elect_pairs(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col, const int16_t *col16,
                      const int32_t *rp2, const int16_t *col2, const int32_t *ids, int32_t *leader, uint8_t *state,
                      int32_t max_rounds, int32_t mode, int32_t *rounds_exec, int64_t *changes_per_round,
                      swarm_elect_stats *stats, void *stream);

/* Same with int64 row offsets: graphs with >= 2^30 edges or agents (the int32-CSR entry points
 * address with 32-bit byte offsets and reject them with SWARM_ERR_ARG; swarm_elect_compact with
 * 16-bit columns reaches 2^31 - 2^20 edges). */
int swarm_elect_i64(swarm_ctx *ctx, int64_t n, const int64_t *row_ptr, const int32_t *col,
                    const int32_t *ids, int32_t *leader, uint8_t *state, int32_t max_rounds,
                    int32_t mode, int32_t *rounds_exec, int64_t *changes_per_round,
                    swarm_elect_stats *stats, void *stream);

/* swarm_elect_compact with int64 row offsets (graphs of >= 2^30 edges; the 16-bit columns are
 * built by swarm_graph_compact from the int32 row offsets, which hold up to 2^31 - 1 edges).
 * Replaces the same election as swarm_elect_i64 (agent.py:263-275); col16 = NULL is swarm_elect_i64. */
int swarm_elect_compact_i64(swarm_ctx *ctx, int64_t n, const int64_t *row_ptr, const int32_t *col,
                            const int16_t *col16, const int32_t *ids, int32_t *leader, uint8_t *state,
                            int32_t max_rounds, int32_t mode, int32_t *rounds_exec, int64_t *changes_per_round,
                            swarm_elect_stats *stats, void *stream);

/* One synchronous E2 round, dense, no convergence loop (building block for sharded runs):
 * leader_out[v] = max(leader_in[v], max_{u in N(v)} leader_in[u]) for v in [0, n_rows);
 * leader_in may hold n_rows + ghosts entries (col indexes it).  *changed (device int64) is
 * incremented by the number of rows whose value rose. */
int swarm_elect_round(swarm_ctx *ctx, int64_t n_rows, const int32_t *row_ptr,
                      const int32_t *col, const int32_t *leader_in, int32_t *leader_out,
                      int64_t *changed, void *stream);

/*
 * Frontier stepper for sharded (multi-GPU) elections: the same exact rounds as
 * swarm_elect(FRONTIER) but driven one round at a time, so a caller can exchange halo values
 * between rounds (swarm_amd/dist.py does it over RCCL).  Local storage = n_rows owned agents
 * followed by ghosts (copies of other shards' boundary agents), n_all in total; the CSR has
 * n_all rows (ghost rows list their local neighbours) and col indexes [0, n_all).
 * Leaders are double-buffered by round parity: round t reads leader[(t-1)&1] and writes
 * leader[t&1], so after round t the current state is leader[t&1] (leader0 / leader1, both
 * n_all, owned by the caller).
 *   begin:   leader0 = leader1 = init; round 1 is a full dense sweep.
 *   step:    round t over the owned rows (dense or sparse, decided on the device from round
 *            t-1's changes + ghost rises; no convergence guard: a shard with no local change
 *            can still receive ghost changes).  Owned changes are counted per round.
 *   ghosts:  after the halo exchange of round t, incoming[i] is the round-t leader of ghost
 *            begin+i; rises are written to both buffers and their local neighbours marked for
 *            round t+1.
 *   changes: per-round owned change counts of rounds t0..t1 (t1 - t0 < 256); host sync.
 *            Read at least every 256 rounds (counter slots are recycled).
 * One stepper per ctx; swarm_elect() on the same ctx resets it.
 */
int swarm_frontier_begin(swarm_ctx *ctx, int64_t n_rows, int64_t n_all, const int32_t *init,
                         int32_t *leader0, int32_t *leader1, void *stream);
/* swarm_frontier_begin with the owned rows at [own_begin, own_begin + n_own) (ghost rows on both
 * sides); swarm_frontier_set_compact: the shard graph's 16-bit columns for the following steps
 * (swarm_graph_compact; NULL: the int32 columns), reset by every begin. */
int swarm_frontier_begin_range(swarm_ctx *ctx, int64_t own_begin, int64_t n_own, int64_t n_all, const int32_t *init,
                               int32_t *leader0, int32_t *leader1, void *stream);
int swarm_frontier_set_compact(swarm_ctx *ctx, const int16_t *col16);
/* The same for swarm_graph_compact_escaped's columns (escaped neighbours read from the step's col). */
int swarm_frontier_set_compact_escaped(swarm_ctx *ctx, const int16_t *col16);
int swarm_frontier_step(swarm_ctx *ctx, int32_t t, const int32_t *row_ptr, const int32_t *col,
                        int32_t *leader0, int32_t *leader1, void *stream);
int swarm_frontier_ghosts(swarm_ctx *ctx, int32_t t, int64_t begin, int64_t count,
                          const int32_t *incoming, const int32_t *row_ptr, const int32_t *col,
                          int32_t *leader0, int32_t *leader1, void *stream);
int swarm_frontier_changes(swarm_ctx *ctx, int32_t t0, int32_t t1, int64_t *out, void *stream);

/*
 * Multi-GPU election: the sharded round loop on the device stream.  Each round:
 * the frontier round over every shard row; after every halo_depth-th round the owned rows each
 * peer keeps as ghosts are packed and sent to it, and the ghosts are received from it (RCCL
 * ncclSend/ncclRecv to EVERY peer in one group), and the received ghost leaders applied
 * (swarm_frontier_ghosts semantics); every batch of rounds one ncclAllReduce(sum) of the
 * per-round owned change counts decides convergence.  Same results as swarm_elect(FRONTIER) on
 * the union graph, for any partition of the agents over the ranks (strips: 2 peers; ID ranges of
 * Morton IDs: a compact region with up to 8; random IDs: every rank).  RCCL is taken from the
 * process at run time (the instance torch loaded); swarm_comm_available() says whether it was found.
 * Replaces: the reference's transport stub (agent.py:188-194) -- it has no multi-process path.
 */
typedef struct swarm_comm swarm_comm;

/* One rank's shard.  Rows: [ghosts of the peers below this rank | owned | ghosts of the peers above]:
 * the ghosts received from peers[j] are the ghost_count[j] rows that follow those of peers[j-1], the
 * peers ranked below this rank filling [0, own_begin) and the peers above [own_begin + n_rows, n_all)
 * (checked).  The ghosts must contain every agent within halo_depth hops of an owned agent, with
 * every edge among the shard's rows in the CSR (swarm_amd/dist.py: every agent within
 * halo_depth radio radii of the owner's region).  A peer appears once even if the halo is empty in
 * one direction; a peer with nothing either way may be left out. */
typedef struct swarm_shard {
    int64_t n_rows;               /* owned agents: rows [own_begin, own_begin + n_rows) */
    int64_t n_all;                /* owned + ghost agents */
    const int32_t *row_ptr;       /* CSR over all n_all rows (ghost rows list their local neighbours) */
    const int32_t *col;
    const int32_t *init;          /* initial leaders = IDs of all n_all agents */
    int64_t own_begin;            /* first owned row */
    int32_t halo_depth;           /* k >= 1 (0 = 1): all n_all rows are stepped, the halo is exchanged
                                     after every k-th round only (owned rows stay exact: a wrong value
                                     starts at the halo's outer edge and moves one hop per round) */
    int32_t n_peers;              /* ranks this shard exchanges with (0 = none) */
    const int32_t *peers;         /* host [n_peers]: their ranks, ascending, none equal to this rank */
    const int64_t *send_count;    /* host [n_peers]: owned rows sent to each peer */
    const int64_t *send_rows;     /* device [sum send_count]: those shard rows, peer after peer */
    const int64_t *ghost_count;   /* host [n_peers]: ghost rows received from each peer */
    const int16_t *col16;         /* swarm_graph_compact of row_ptr / col, or NULL (int32 columns) */
    int32_t col16_escaped;        /* col16 is swarm_graph_compact_escaped's (escapes read from col) */
} swarm_shard;

int swarm_comm_available(void);
int swarm_comm_unique_id(void *out128);
int swarm_comm_create(swarm_comm **out, int nranks, int rank, const void *id128);
int swarm_comm_destroy(swarm_comm *comm);
/* Transport kinds.  SWARM_COMM_RCCL: the calls above (one rank per GPU, RCCL over xGMI).
 * SWARM_COMM_SHM: processes of ONE host, any GPUs (several may share one): the same sharded C loops
 * (swarm_elect_sharded, swarm_auction_sharded) with every exchange staged through a POSIX shared-memory
 * segment and a process-shared barrier (synchronous per op; SWARM_SHM_MB mailbox MiB per rank and
 * parity, default 16; SWARM_SHM_TIMEOUT_S, default 120, before a barrier gives up).  Rank 0 makes the
 * id (swarm_comm_unique_id_kind), every rank passes the same 128 bytes to swarm_comm_create_kind. */
#define SWARM_COMM_RCCL 0
#define SWARM_COMM_SHM 1
int swarm_comm_unique_id_kind(int kind, void *out128);
int swarm_comm_create_kind(swarm_comm **out, int kind, int nranks, int rank, const void *id128);
int swarm_comm_kind(const swarm_comm *comm);
/* leader0 / leader1: n_all each; after rounds_exec rounds the state is leader[rounds_exec&1].
 * changes_per_round (host, capacity max_rounds): GLOBAL per-round change counts. */
int swarm_elect_sharded(swarm_ctx *ctx, swarm_comm *comm, const swarm_shard *shard,
                        int32_t *leader0, int32_t *leader1, int32_t max_rounds,
                        int32_t *rounds_exec, int64_t *changes_per_round, void *stream);
/* swarm_elect_sharded with this rank's own per-round figures (each optional, host, capacity max_rounds):
 * local_counts[3 (r-1) + {0,1,2}] = round r's owned changes, rows gathered and edges gathered on this rank
 * (a dense round: n_all rows and -1 = every edge of the shard graph); round_ms[r-1] = the device time from
 * the start of round r to the start of round r+1 on this rank (one HIP event per round; the per-round cost
 * model of DESIGN §6 is fitted from them).
 * comm may be NULL for a shard without peers (one rank: the shard graph stepped alone). */
int swarm_elect_sharded_ex(swarm_ctx *ctx, swarm_comm *comm, const swarm_shard *shard,
                           int32_t *leader0, int32_t *leader1, int32_t max_rounds,
                           int32_t *rounds_exec, int64_t *changes_per_round, int64_t *local_counts,
                           float *round_ms, void *stream);

/*
 * Task allocation round (contract A-H).
 * Replaces: SwarmAgent._process_tasks + _calculate_utility (agent.py:292-302, 338-347) run by
 * every agent over every OPEN task, then SwarmAgent._handle_task_claim (agent.py:304-325) at
 * the resolver for every claim in ascending sender-ID order, then the winner notification
 * _handle_task_conflict (agent.py:327-336).
 *   U(a,k) = (u_scale / (1 + sqrt(dx*dx + dy*dy))) * has_cap   (fp64, no FMA contraction)
 *   claim iff U > claim_thr; claim value x = f32(U) (round to nearest even)
 *   per task, claims in ascending agent ID: the first claim wins if the task has no current
 *   winner, otherwise a claim replaces the winner iff x > util + hysteresis (fp64).
 *   Guard band: the reference squares with libm pow(|d|, 2.0), which can
 *   differ from d*d by an ulp.  Every task with a pair whose decision or f32 value such an ulp
 *   could change (stats->n_flagged pairs) is deferred; those pairs are decided on the HOST with
 *   this process's libm pow, exactly as agent.py:297/302/340 compute them, and the task is then
 *   resolved once with them (stats->n_resolved tasks; one extra host round trip when > 0).  The
 *   outputs are therefore the reference's on this host's libm, not only the x*x arithmetic's.
 * apos (n*2 f64), acaps (n u32: bit k = capability k), tpos (t*2 f64), treq (t i8: -1 none).
 * winner/util (device, t): in = current claim table (-1 = no claim; util fp64), out = final.
 * won (device, n, may be NULL): out, tasks won per agent.  id_to_index (device, may be NULL,
 * length id_span): storage index of each ID, used to credit `won` for a pre-existing winner
 * that keeps its task.  nclaim/nmsg (device, t, may be NULL): claims and TASK_CONFLICT
 * messages per task.  stats (host, may be NULL).
 */
int swarm_allocate(swarm_ctx *ctx, int64_t n, const int32_t *ids, const double *apos,
                   const uint32_t *acaps, int64_t t, const double *tpos, const int8_t *treq,
                   double claim_thr, double hysteresis, double u_scale, int32_t mode,
                   int32_t *winner, double *util, int32_t *won, const int32_t *id_to_index,
                   int64_t id_span, int64_t *nclaim, int64_t *nmsg, swarm_alloc_stats *stats,
                   void *stream);

/*
 * The same round (BINNED) over agents stored in cell order -- swarm_cell_order's layout, the
 * spatial layout of swarm_amd.Swarm -- without a binning pass: a task's claim window is the
 * grid rows it covers, each a contiguous range of storage indices.  The index comes from
 * swarm_cell_index over the same positions.  Every call verifies on the device that each agent
 * still lies in its cell's range; if not (positions moved since the index was built) it returns
 * SWARM_ERR_STALE and the outputs are undefined -- rebuild the index, or call swarm_allocate.
 * Claim radius (u_scale / claim_thr - 1) must span at most 16 grid rows (SWARM_ERR_ARG).
 */


/* grid (host) and cell_off (device, ncells + 1): agents of cell c = cy * ncx + cx are storage
 * indices [cell_off[c], cell_off[c + 1]).  cell_off == NULL: fill grid and *ncells only.
 * SWARM_ERR_ARG if pos is not in cell order.  Synchronises the stream. */
int swarm_cell_index(swarm_ctx *ctx, int64_t n, const double *pos, double cell, swarm_grid *grid,
                     uint32_t *cell_off, int64_t cell_off_capacity, int64_t *ncells, void *stream);

int swarm_allocate_indexed(swarm_ctx *ctx, int64_t n, const int32_t *ids, const double *apos,
                           const uint32_t *acaps, const swarm_grid *grid, const uint32_t *cell_off,
                           int64_t t, const double *tpos, const int8_t *treq, double claim_thr,
                           double hysteresis, double u_scale, int32_t *winner, double *util,
                           int32_t *won, const int32_t *id_to_index, int64_t id_span,
                           int64_t *nclaim, int64_t *nmsg, swarm_alloc_stats *stats, void *stream);

/* swarm_allocate_indexed with flags (same results):
 *   SWARM_ALLOC_TRUST_INDEX   the caller vouches that apos are the positions swarm_cell_index indexed
 *                             (unchanged since): no device staleness check (never SWARM_ERR_STALE)
 *   SWARM_ALLOC_FRESH_CLAIMS  no claim table: winner / util are outputs only, initialised on the
 *                             device to -1 / 0.0 (what an empty agent.py task_claims table means) */
#define SWARM_ALLOC_TRUST_INDEX 1
#define SWARM_ALLOC_FRESH_CLAIMS 2
int swarm_allocate_indexed_ex(swarm_ctx *ctx, int64_t n, const int32_t *ids, const double *apos,
                              const uint32_t *acaps, const swarm_grid *grid, const uint32_t *cell_off,
                              int64_t t, const double *tpos, const int8_t *treq, double claim_thr,
                              double hysteresis, double u_scale, int32_t flags, int32_t *winner, double *util,
                              int32_t *won, const int32_t *id_to_index, int64_t id_span,
                              int64_t *nclaim, int64_t *nmsg, swarm_alloc_stats *stats, void *stream);

/*
 * Exact fp64 utility for m (agent, task) pairs (agent.py:338-347), GPU arithmetic.
 * out (device, m f64).  Used by parity tests and by callers that need costs, not claims.
 */
int swarm_utility(swarm_ctx *ctx, int64_t m, const double *apos, const uint32_t *acaps,
                  const double *tpos, const int8_t *treq, double u_scale, double *out,
                  void *stream);

/*
 * Radius graph builder (synthetic/sensor input side of the round):
 * edge i~j (i != j) iff dx*dx + dy*dy <= radius*radius (fp64).  Rows ascending.
 * Call with col == NULL to get row_ptr (device, n+1) and *n_edges (host); then again with col
 * (device, capacity col_capacity) to fill.  SWARM_ERR_RANGE (before any row is built) when the
 * cell occupancies say the build would scan more than 2^36 candidate pairs in all or more than
 * 2^20 in one agent's 3 x 3 cell window (co-located agents), or the graph has >= 2^31 edges.
 * SWARM_ERR_ARG (nothing written) for a position that is NaN or infinite, and for finite positions whose
 * bounding box has no finite extent (max - min overflows a double); so does every call that grids positions
 * (swarm_cell_order, swarm_cell_index, the sensed physics and loop, the auction) for such a box.
 */
int swarm_build_rgg(swarm_ctx *ctx, int64_t n, const double *pos, double radius,
                    int32_t *row_ptr, int32_t *col, int64_t col_capacity, int64_t *n_edges,
                    void *stream);

/*
 * Spatial storage order: perm (device, n) such that agents perm[0], perm[1], ... are
 * grouped by row-major grid cell of side `cell` (stable within a cell).  SWARM_ERR_ARG for a position
 * that is NaN or infinite.
 */
int swarm_cell_order(swarm_ctx *ctx, int64_t n, const double *pos, double cell,
                     int32_t *perm, void *stream);

/*
 * Auction allocation (BASELINE config C4) -- the north star's "auction
 * price update": no reference counterpart (the reference allocates by greedy claims and leader
 * hysteresis, swarm_allocate above), parity against the build's CPU restatement
 * (oracle/swarm_oracle.c orc_auction).  One task per agent and one agent per task over the
 * admissible pairs U > claim_thr (agent.py:297), value x = f32(U) (the claim payload,
 * agent.py:302).  Jacobi Bertsekas auction: each round every unassigned, active agent bids on
 * its best task (net = x - price[k], ties -> lowest task index) the price price + (best -
 * second) + eps, where the opt-out option (net 0) competes as a second best; an agent whose
 * best net is <= 0 drops out for good.  Each task takes its highest bid, ties -> lowest agent
 * ID; its previous owner becomes unassigned.  rounds_exec = rounds that had bidders (the auction
 * stops at the first round without one).
 * owner (device, t): storage index of the task's agent or -1; price (device, t, f32);
 * assigned (device, n): task index or -1.  bidders_per_round (host, capacity max_rounds, may be
 * NULL).  Returns SWARM_NOT_CONVERGED if max_rounds rounds all had bidders.
 */
typedef struct swarm_auction_stats {
    int64_t n_pairs;         /* admissible (agent, task) pairs */
    int64_t n_flagged;       /* pairs inside the libm guard band (see swarm_allocate) */
    int64_t rounds_launched; /* rounds issued (>= rounds_exec + 1) */
    int64_t tail_rounds;     /* rounds run by the single-workgroup tail kernel */
    int64_t bids_total;      /* agent-rounds with a bidder, summed over rounds */
} swarm_auction_stats;

int swarm_auction(swarm_ctx *ctx, int64_t n, const int32_t *ids, const double *apos, const uint32_t *acaps,
                  int64_t t, const double *tpos, const int8_t *treq, double claim_thr, double u_scale, float eps,
                  int32_t max_rounds, int32_t *owner, float *price, int32_t *assigned, int32_t *rounds_exec,
                  int64_t *bidders_per_round, swarm_auction_stats *stats, void *stream);

/*
 * Sharded auction (BASELINE config C4 on several GPUs): agents partitioned over
 * ranks, tasks replicated on every rank.  Round r: this rank's unassigned, active agents bid
 * into keys (t task keys, packed as in swarm_auction, + one bidder-count word per rank: t + world
 * u64, zero on the first call), the keys are MAX-all-reduced over ranks, and every rank resolves
 * every task identically.  owner_id holds the owning agent's ID (-1 none; replicated), price is
 * replicated, assigned (n, this rank's agents) the task index or -1.  Results equal
 * swarm_auction over the union of all ranks' agents (rounds, bidder counts, prices, owners).
 *   swarm_auction_begin    candidate lists of this rank's agents; initialises owner_id, price,
 *                          assigned; keeps its state in ctx until the next begin (no other
 *                          libswarm call on this ctx in between)
 *   swarm_auction_bid      round r's bids -> keys (then the caller all-reduces keys with MAX)
 *   swarm_auction_resolve  round r's resolution from the reduced keys; log[r] = the round's global
 *                          bidder count (device int64, indexed by round); zeroes keys again
 *   swarm_auction_sharded  the whole loop on the device stream with an RCCL all-reduce per round
 *                          (comm from swarm_comm_create); returns as swarm_auction
 */
int swarm_auction_begin(swarm_ctx *ctx, int64_t n, const int32_t *ids, const double *apos, const uint32_t *acaps,
                        int64_t t, const double *tpos, const int8_t *treq, double claim_thr, double u_scale, float eps,
                        int32_t *owner_id, float *price, int32_t *assigned, swarm_auction_stats *stats,
                        void *stream);
int swarm_auction_bid(swarm_ctx *ctx, int64_t r, int32_t rank, int32_t world, uint64_t *keys, const float *price,
                      int32_t *assigned, void *stream);
int swarm_auction_resolve(swarm_ctx *ctx, int64_t r, int32_t world, uint64_t *keys, int32_t *owner_id, float *price,
                          int32_t *assigned, int64_t *log, void *stream);
int swarm_auction_sharded(swarm_ctx *ctx, swarm_comm *comm, int64_t n, const int32_t *ids, const double *apos,
                          const uint32_t *acaps, int64_t t, const double *tpos, const int8_t *treq, double claim_thr,
                          double u_scale, float eps, int32_t max_rounds, int32_t *owner_id, float *price,
                          int32_t *assigned, int32_t *rounds_exec, int64_t *bidders_per_round,
                          swarm_auction_stats *stats, void *stream);

/*
 * Physics / formation step: SwarmAgent._update_physics (agent.py:94-181)
 * for every agent, as one synchronous step (contract P1): all agents read the step-start
 * positions pos_in (n x 2 f64) and write pos_out (must differ).  A FOLLOWER (state) with
 * leader_index >= 0 (storage index of its leader, -1 none) targets its V-formation slot behind
 * the f32-rounded leader position (the '!ff' heartbeat payload); target (n x 2 f64) /
 * has_target (n u8) are in/out (agent.py:53 self.target, None = 0).  obstacles: m x 3 f64
 * (x, y, radius), shared by every agent, applied in order; row_ptr/col: each agent's sensed
 * neighbours, applied in CSR order.  vel (n x 2 f64): out for every moving agent.  Agents
 * without a target keep position and velocity (agent.py:113-114).  Arithmetic: fp64, the
 * reference's order of operations, squares as x*x (the reference uses libm pow; <= 1 ulp per
 * square).  n_singular (host, may be NULL): zero distances to an obstacle centre or a
 * neighbour (the reference raises ZeroDivisionError there).
 */
int swarm_physics_step(swarm_ctx *ctx, int64_t n, const int32_t *ids, const uint8_t *state,
                       const int32_t *leader_index, const double *pos_in, double *pos_out, double *vel,
                       double *target, uint8_t *has_target, int64_t m, const double *obstacles,
                       const int32_t *row_ptr, const int32_t *col, double dt, double max_speed,
                       int64_t *n_singular, void *stream);

/*
 * `steps` physics steps whose neighbours are sensed from the moving positions (contract S1): the
 * reference's simulator refreshes every agent's neighbour list (update_sensors) before each tick, so
 * separation (agent.py:148-160) acts on where the neighbours are, not where they were.  Per step, with
 * P the positions at its start: agent i senses j != i iff dx*dx + dy*dy <= sense_radius^2 (fp64, the
 * products rounded separately: swarm_build_rgg's rule) and applies the sensed neighbours in ascending
 * storage index; everything else is swarm_physics_step.  The state after s steps is bit-identical to s
 * repetitions of swarm_build_rgg(P, sense_radius) + swarm_physics_step on that graph, without a graph
 * in memory.  pos (n x 2 f64) is in/out and holds the result for any step count (the second buffer is
 * the ctx's).  steps_done / n_singular (host, may be NULL): steps run; zero distances over all steps.
 * SWARM_ERR_ARG (nothing written): steps < 0, sense_radius not positive and finite, non-finite dt /
 * max_speed, non-finite positions at entry.  SWARM_ERR_RANGE: at the start of step *steps_done the
 * agents' 3 x 3 cell windows exceeded swarm_build_rgg's work limits (2^36 candidate pairs, 2^20 in one
 * window); pos holds the state after *steps_done steps and no window was scanned for that step or a
 * later one.  A singular step leaves non-finite positions; such an agent senses nobody and is sensed
 * by nobody in later steps.  Two host waits per call (the entry bounding box, the final verdict).
 * n == 0: nothing to do, *steps_done = steps; steps == 0: *steps_done = 0 and the arrays are neither
 * read nor checked.  Any other error (SWARM_ERR_HIP, SWARM_ERR_OOM) at step k > 0 ends the run there:
 * *steps_done = k (or the refused step, if earlier), pos holds the state after those steps.
 */
int swarm_physics_run_sensed(swarm_ctx *ctx, int64_t n, const int32_t *ids, const uint8_t *state,
                             const int32_t *leader_index, double *pos, double *vel, double *target,
                             uint8_t *has_target, int64_t m, const double *obstacles,
                             double sense_radius, int32_t steps, double dt, double max_speed,
                             int32_t *steps_done, int64_t *n_singular, void *stream);

/*
 * Batched wire codec: the reference's transport framing, agent.py:184-214,
 * for m messages at once.  Big-endian '!BBI' header (type, sender, tick) + payload by type:
 * 1 HEARTBEAT '!ff' (a, b = leader x, y), 2 ELECTION_ACCLAIM '!B' (the sender ID), 3 COORDINATOR
 * (none), 4 TASK_CLAIM '!If' (task, a = utility), 5 TASK_CONFLICT '!IB' (task, winner).
 * wide != 0 widens every u8 ID field to u32 ('!BII' header, '!I' acclaim, '!II' conflict), an
 * extension for swarms with IDs > 255 that the reference cannot frame.
 *
 * encode (device arrays of m; integer fields int64 so out-of-range values are representable):
 * status[i] = 0 ok, 1 struct.error (an integer field out of range), 2 OverflowError (a finite
 * value beyond f32), 3 unknown type -- payload checked before header, as the reference packs
 * them; an errored message takes no bytes.  offsets (device, m+1) = packet offsets into out,
 * offsets[m] = *total_bytes (host).  out == NULL: sizing call (status/offsets/total only);
 * otherwise cap must be >= the total (SWARM_ERR_RANGE: *total_bytes is the size needed, status and
 * offsets are filled, nothing at or past out + cap is written).  out may have any alignment (a view
 * into a larger buffer): the 16-byte stores are aligned on the address, not on the offset.  The
 * field arrays, offsets and status need only their natural alignment.  Synchronises the stream
 * (total_bytes).  One pass: tiles of 2 048 messages take their byte offsets from the lower
 * tiles' published counts (a ticket counter and look-back words in the ctx), so encode calls on one
 * ctx must not overlap (SWARM_ERR_HIP if they did and a look-back gave up).
 */
int swarm_codec_encode(swarm_ctx *ctx, int64_t m, const int64_t *type, const int64_t *sender, const int64_t *tick,
                       const double *a, const double *b, const int64_t *task, const int64_t *winner, int32_t wide,
                       uint8_t *out, int64_t cap, int64_t *offsets, int8_t *status, int64_t *total_bytes,
                       void *stream);

/*
 * decode: packet i is buf[offsets[i] .. offsets[i+1]) (device).  status: 0 handled, 1 dropped
 * (shorter than the header, agent.py:198-199), 2 unknown type (ignored, no handler), 3 the
 * handler's unpack raises struct.error (TASK_CLAIM payload != 8 bytes, TASK_CONFLICT != 5 (8
 * wide)), 4 offsets outside [0, buf_len] or decreasing (packet not read).  Fields not carried by
 * the type are 0; a HEARTBEAT carries a position (has_pos = 1,
 * a/b as f32) only when its payload is exactly 8 bytes (agent.py:256-258).  TASK_CLAIM
 * utility -> a; a signalling NaN arrives quiet, payload kept, as the handlers' Python floats do.
 * buf may have any alignment (a buffer that is not 16-byte aligned is parsed from global memory, not
 * staged).  Asynchronous on stream.
 */
int swarm_codec_decode(swarm_ctx *ctx, int64_t m, const uint8_t *buf, int64_t buf_len, const int64_t *offsets,
                       int32_t wide,
                       int8_t *status, int64_t *type, int64_t *sender, int64_t *tick, float *a, float *b,
                       int64_t *task, int64_t *winner, uint8_t *has_pos, void *stream);

/*
 * Timer FSM / protocol ticks: every agent's update_loop tick
 * (agent.py:66-80) at once -- inbound ELECTION_ACCLAIM / COORDINATOR / HEARTBEAT handling
 * (243-281) from the CSR neighbours' previous-tick sends, then _check_election_timeout
 * (217-241) and the leader's _send_heartbeat (283-289) -- for ticks t0+1 .. t0+ticks under
 * contract T1 (tools/gen_golden.py ref_fsm): clock = t * dt; agent i's own tick counter is
 * t + tick_off[i] (heartbeats when it is a multiple of 10); the election jitter is
 * jitter * u(seed, id, t) with u the splitmix64 hash of tools/gen_golden.py jitter_u.
 * fsm: device state, in/out (n each unless noted): state (SWARM_*), leader (ID, -1 = None),
 * last_hb / wait_start / delay (f64 seconds: last_heartbeat_time, election_wait_start,
 * election_delay), leader_pos (n x 2 f32, the '!ff' heartbeat payload; (0, 0) when None),
 * has_leader_pos, alive, outbox (2n bytes, tick-parity double buffer: the bytes at parity
 * (t0 & 1) are the tick-t0 sends; bit 0 ACCLAIM+COORDINATOR, bit 1 HEARTBEAT).
 * row_ptr/col: whom each agent hears (its receive order); hear_row_ptr/hear_col: the transpose
 * (who hears each agent; the same arrays for a symmetric graph), or NULL: with it only agents
 * something was sent to walk their row each tick (push marks), without it every agent does.
 * kill_ticks (host, n_kill): at the start of each such tick every alive LEADER dies.
 * counts (host, ticks x 4, may be NULL): per tick, alive LEADERs, alive ELECTION_WAITs, ACCLAIM
 * senders, HEARTBEAT senders.  Synchronises the stream when counts != NULL.
 */
typedef struct {
    uint8_t *state;
    int32_t *leader;
    double *last_hb;
    double *wait_start;
    double *delay;
    float *leader_pos;
    uint8_t *has_leader_pos;
    uint8_t *alive;
    uint8_t *outbox;
} swarm_fsm;

int swarm_protocol_run(swarm_ctx *ctx, int64_t n, const int32_t *ids, const double *pos, const int32_t *row_ptr,
                       const int32_t *col, const int32_t *hear_row_ptr, const int32_t *hear_col,
                       const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks,
                       double dt, double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                       int32_t n_kill, int64_t *counts, void *stream);

/* swarm_protocol_run with storm ticks pulled and the traffic counted (same results):
 * pull_frac (push mode): when the senders of a tick's workgroup (its share of the agents: a grid-stride
 *   set of 4-agent groups, or of 4 096-agent chunks) exceed pull_frac x its agents, the next tick's
 *   receivers walk their own rows instead of being mailed (a timeout wave makes most agents send at
 *   once: mailing every hearer costs more than every agent pulling); < 0: never.
 * traffic (host, 8 int64, may be NULL; synchronises): summed over the run -- [0] receivers served by
 *   their single sender, [1] receivers that walked their row (several senders), [2] row edges walked
 *   (those and pulled ticks), [3] senders mailed, [4] hearer edges mailed, [5] 0, [6] agents that
 *   walked their row in pulled ticks, [7] pulled ticks.  Pull mode (hear_row_ptr NULL) counts nothing. */
int swarm_protocol_run_ex(swarm_ctx *ctx, int64_t n, const int32_t *ids, const double *pos, const int32_t *row_ptr,
                          const int32_t *col, const int32_t *hear_row_ptr, const int32_t *hear_col,
                          const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks,
                          double dt, double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                          int32_t n_kill, double pull_frac, int64_t *counts, int64_t *traffic, void *stream);

/*
 * The coupled update loop (agent.py:67-81: each tick _process_logic, then _update_physics), for the
 * whole swarm, ticks t0+1 .. t0+ticks in one call (contract U1).  dt is both the FSM's clock step and
 * the physics step (the reference's period).  With P_k the positions after the physics of tick k, tick t:
 *   kills, receive, logic   swarm_protocol_run_ex's tick (same arguments, same meaning), except that a
 *             HEARTBEAT received at tick t carries the f32-rounded position its sender had when it sent
 *             it during tick t-1, P_{t-2} (the payload is packed inside _process_logic, before that
 *             tick's physics);
 *   physics   every alive agent senses its row of sense_row_ptr / sense_col (CSR order, dead agents
 *             included as bodies at rest) and the m obstacles at the snapshot P_{t-1} and runs
 *             swarm_physics_step's arithmetic with its own FSM state as the tick's logic left it: a
 *             FOLLOWER with has_leader_pos retargets the V slot behind its own leader_pos (stored in
 *             target / has_target); any other agent keeps the target it had (an ELECTION_WAIT agent
 *             and a new LEADER keep chasing their last slot); without a target it keeps position and
 *             velocity.  Dead agents run neither half: position, velocity and target stay frozen.
 * pos / pos_prev (n x 2 f64, 16-byte aligned, not overlapping): in, P_{t0} and P_{t0-1} (what the
 * heartbeats in flight at t0 carry; a copy of pos for a fresh run); out, P_{t0+ticks} and
 * P_{t0+ticks-1}, for either parity of ticks -- so a run split into chunks is the same run.  vel /
 * target / has_target / obstacles / max_speed: as swarm_physics_step.  trace (device, frames x n x 2
 * f64, frames = ticks / trace_every; ignored when trace_every == 0): frame f = P_{t0+(f+1) trace_every}.
 * counts (host, ticks x 4, may be NULL) as swarm_protocol_run; n_singular (host, may be NULL) as
 * swarm_physics_step, summed over the ticks.  The FSM's records are packed once and unpacked once; no
 * host wait inside the loop, one at the end when counts or n_singular is given.  n == 0 or ticks == 0:
 * nothing is read or written (counts zeroed, *n_singular = 0).  Arguments are checked before anything is
 * launched (SWARM_ERR_ARG).  The neighbour lists are fixed for the call; swarm_update_loop_sensed senses
 * them anew every tick.
 */
int swarm_update_loop(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                      const int32_t *row_ptr, const int32_t *col, const int32_t *hear_row_ptr,
                      const int32_t *hear_col, const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0,
                      int32_t ticks, double dt, double timeout, double jitter, uint64_t seed,
                      const int64_t *kill_ticks, int32_t n_kill, double pull_frac, double *vel, double *target,
                      uint8_t *has_target, int64_t m, const double *obstacles, const int32_t *sense_row_ptr,
                      const int32_t *sense_col, double max_speed, double *trace, int32_t trace_every,
                      int64_t *counts, int64_t *n_singular, void *stream);

/*
 * swarm_update_loop with the separation neighbours sensed from the moving positions (contract U1-S; the
 * reference's simulator calls update_sensors before every tick).  Tick t, with S = P_{t-1} the snapshot its
 * physics reads: every alive agent i senses each j != i with dx*dx + dy*dy <= sense_radius^2 (fp64, the
 * products rounded separately: swarm_build_rgg's rule), dead agents and agents without a target included as
 * bodies at rest, and applies the sensed neighbours in ascending storage index; everything else -- kills,
 * receive, logic, the heartbeats' P_{t-2}, retargeting, frozen dead agents, the arithmetic, pos / pos_prev,
 * trace, counts, n_singular -- is swarm_update_loop's, argument for argument.  The message graph (row_ptr /
 * col and the hearers) is fixed for the call and not touched.  The state after the call is bit-identical to
 * `ticks` repetitions of swarm_build_rgg(pos, sense_radius) + swarm_update_loop(ticks = 1) on that graph,
 * with no graph in memory.  An agent left non-finite by a singular tick senses nobody and is sensed by nobody.
 * SWARM_ERR_ARG (nothing written): a NULL ctx, sense_radius not positive and finite, non-finite dt /
 * max_speed, negative ticks, overlapping or misaligned pos / pos_prev, non-finite positions at entry.
 * All or nothing: when, at the start of some tick, the agents' 3 x 3 cell windows exceed swarm_build_rgg's
 * work limits (2^36 candidate pairs, 2^20 in one window; judged on the device), the call returns
 * SWARM_ERR_RANGE with *refused_tick (host, may be NULL; -1 otherwise) the absolute tick, and pos, pos_prev,
 * vel, target, has_target, every array of fsm (both outbox halves) and counts hold exactly what they held at
 * entry; no window of that tick or a later one was scanned.  To keep the progress up to a dense tick, run the
 * loop in chunks.  Two host waits per call: the entry bounding box and the final verdict; none in the loop.
 * The ctx keeps 114 bytes per agent for the entry state, next to the binning's scratch and the 16 bytes per
 * agent of the cell-sorted snapshot.  n == 0 or ticks == 0: as swarm_update_loop.
 */
int swarm_update_loop_sensed(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                             const int32_t *row_ptr, const int32_t *col, const int32_t *hear_row_ptr,
                             const int32_t *hear_col, const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0,
                             int32_t ticks, double dt, double timeout, double jitter, uint64_t seed,
                             const int64_t *kill_ticks, int32_t n_kill, double pull_frac, double *vel,
                             double *target, uint8_t *has_target, int64_t m, const double *obstacles,
                             double sense_radius, double max_speed, double *trace, int32_t trace_every,
                             int64_t *counts, int64_t *n_singular, int64_t *refused_tick, void *stream);

/*
 * swarm_update_loop_sensed with the radio neighbours re-sensed as well (contract U1-R): there is no message
 * graph.  Tick t, with S = P_{t-1} the snapshot its sensors read: alive agent i hears agent j != i iff
 * dx*dx + dy*dy <= radio_radius^2 on S (fp64, the products rounded separately, radio_radius^2 computed once:
 * swarm_build_rgg's rule) and receives what each heard j sent during tick t-1 in ascending storage index (a
 * swarm_build_rgg row's order; the handlers are order-dependent: a follower's leader and leader_pos are the
 * last heartbeat's in that order).  A heartbeat still carries its sender's f32-rounded P_{t-2}: who hears is
 * judged on P_{t-1}, what is heard was packed a tick earlier.  Dead agents neither send nor receive and are
 * still sensed as bodies at rest; an agent left non-finite by a singular tick hears nobody and is heard by
 * nobody.  Everything else -- kills, timers, the sensed physics at sense_radius, pos / pos_prev, trace,
 * counts, n_singular -- is swarm_update_loop_sensed's, argument for argument.  The state after the call is
 * bit-identical to `ticks` repetitions of swarm_build_rgg(pos, radio_radius) as the message graph +
 * swarm_update_loop_sensed(ticks = 1, sense_radius) (finite positions: swarm_build_rgg refuses a NaN), with
 * no graph in memory; calls chain with swarm_update_loop / swarm_update_loop_sensed through fsm, t0 and
 * pos_prev.
 * SWARM_ERR_ARG (nothing written): either radius not positive and finite, and whatever
 * swarm_update_loop_sensed refuses.  All or nothing as swarm_update_loop_sensed: both windows are read on one
 * grid per call, of cells max(radio_radius, min(sense_radius, 2)) wide, and its window work is judged on the
 * device at the start of every tick; a refused tick returns SWARM_ERR_RANGE with *refused_tick set and every
 * caller array as it was at entry.  Two host waits per call: the entry bounding box and the final verdict.
 * The ctx keeps, next to swarm_update_loop_sensed's scratch, one byte per agent (the cell-sorted outbox) and
 * one per grid cell (the cells that hold a sender).  n == 0 or ticks == 0: as swarm_update_loop.
 */
int swarm_update_loop_radio(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                            const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks, double dt,
                            double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                            int32_t n_kill, double *vel, double *target, uint8_t *has_target, int64_t m,
                            const double *obstacles, double radio_radius, double sense_radius, double max_speed,
                            double *trace, int32_t trace_every, int64_t *counts, int64_t *n_singular,
                            int64_t *refused_tick, void *stream);

/*
 * swarm_update_loop_radio with _process_logic's third step, _process_tasks, and the two task handlers
 * (agent.py:292-336) run every tick (contract U1-T).  A board of T <= 64 tasks is shared by all
 * agents (every agent's `tasks` dict holds all T).  Tick t, with U1-R's snapshot and walk:
 *   receive   alive agent i walks its heard senders j in ascending storage index; for each j it handles j's
 *             packets of tick t-1 as swarm_update_loop_radio does and then j's TASK_CLAIMs, which count only
 *             if i is LEADER at that moment (after j's election packets, before sender j+1's).  A claim on
 *             task k with utility u (f32; computed from the position its sender claimed at, P_{t-2}) takes
 *             i's table entry when that is empty or u > held + 5.0 (the f32 values widened to fp64) and sends a
 *             TASK_CONFLICT naming the claimer; otherwise, when the held winner is another agent, it sends one
 *             naming the held winner.  j's TASK_CONFLICTs set i's status of the task to ASSIGNED when the
 *             winner is i's ID, else LOCKED, whatever i's state and whoever j is; the last conflict on a task
 *             in walk order wins.
 *   logic     after the timers and the heartbeat, every task still OPEN with U(P_{t-1}[i], caps[i], task) >
 *             20.0 (fp64, swarm_allocate's arithmetic) becomes TENTATIVE and is claimed.  No status returns to
 *             OPEN.  Dead agents neither claim, arbitrate nor change status; what they sent before dying still
 *             arrives.  A table survives its owner losing leadership.
 * swarm_tasks, everything on the device, the per-agent arrays in/out so that a run split into chunks is the
 * same run with claims and conflicts in flight across the boundary:
 *   T, tpos (T x 2 f64), treq (T i8: -1 none, else a capability bit 0..31), caps (n u32): as swarm_allocate;
 *   status_lo / status_hi (n u64 each): bit k of the two words is task k's 2-bit status -- 0 OPEN,
 *             1 TENTATIVE, 2 LOCKED, 3 ASSIGNED;
 *   claim_out / conflict_out (2n u64 each, by tick parity as the outbox): bit k of word (t & 1) n + i -- agent
 *             i claimed task k during tick t / sent at least one TASK_CONFLICT on it (the message names the
 *             winner its table held at the end of that tick's receive);
 *   tab_winner (n x T i32, -1 empty) / tab_util (n x T f32): every agent's task_claims.
 * The dense table costs 8 T bytes per agent, and the ctx keeps the same again (plus 48 bytes per agent for the
 * other task words) in the entry snapshot, and 2 bytes per agent of scratch; a sparse table and T > 64 are
 * out of scope.
 * task_counts (host, ticks x 3, may be NULL): per tick, TASK_CLAIMs sent, claims handled by a LEADER,
 * TASK_CONFLICT messages sent.  n_guard (host, may be NULL): evaluated (agent, OPEN task) pairs of the run whose
 * utility lies where libm pow arithmetic for the squares could have decided differently (swarm_allocate's
 * guard band around 20.0); the loop has no host wait, so nothing is deferred -- the caller learns whether
 * the run may differ from the reference's.
 * SWARM_ERR_ARG (nothing written): tasks NULL, T outside [0, 64], a treq outside [-1, 31] (read back from the
 * device before anything is launched), a NULL array with T > 0, and whatever swarm_update_loop_radio refuses.
 * The all-or-nothing refusal of a too-dense tick restores every task array as well and withholds task_counts
 * and n_guard.  T == 0: swarm_update_loop_radio, task_counts zeroed, *n_guard = 0, no task array touched.
 */
typedef struct {
    int32_t T;
    const double *tpos;
    const int8_t *treq;
    const uint32_t *caps;
    uint64_t *status_lo;
    uint64_t *status_hi;
    uint64_t *claim_out;
    uint64_t *conflict_out;
    int32_t *tab_winner;
    float *tab_util;
} swarm_tasks;

int swarm_update_loop_tasks(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                            const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks, double dt,
                            double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                            int32_t n_kill, double *vel, double *target, uint8_t *has_target, int64_t m,
                            const double *obstacles, double radio_radius, double sense_radius, double max_speed,
                            double *trace, int32_t trace_every, int64_t *counts, int64_t *n_singular,
                            int64_t *refused_tick, const swarm_tasks *tasks, int64_t *task_counts,
                            int64_t *n_guard, void *stream);

/*
 * swarm_update_loop_radio / swarm_update_loop_tasks over a lossy channel (contract U1-L).  Inside
 * radio_radius the ideal channel delivers every packet; here, at absolute tick t (t0 + 1 .. t0 + ticks), the
 * link from in-range sender j (ID sid) to alive receiver i (ID rid), j != i, is dropped iff
 *     u(ch->seed, t, sid, rid) < ch->loss,
 * and a dropped link delivers nothing of what j sent during tick t-1 to i: not its ACCLAIM + COORDINATOR pair,
 * not its HEARTBEAT (no liveness proof, no leader position, no bully-back), not its TASK_CLAIMs, not its
 * TASK_CONFLICTs.  Every other step is swarm_update_loop_radio's / swarm_update_loop_tasks': the walk order,
 * the lagged positions, timers, the claim evaluation, kills, the refusal of a too-dense tick.  j -> i and
 * i -> j are decided independently.  The draw, in uint64_t arithmetic mod 2^64:
 *     fin(x): x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9; x = (x ^ (x >> 27)) * 0x94D049BB133111EB; x ^ (x >> 31)
 *     a = fin(seed ^ (u64(u32(sid)) * 0x9E3779B97F4A7C15) ^ (u64(t) * 0xD1B54A32D192ED03))
 *     b = fin(a ^ (u64(u32(rid)) * 0x9E3779B97F4A7C15));  u = double(b >> 11) * 2^-53
 * It is keyed on IDs, not storage indices, and on the absolute tick: the decisions depend neither on the layout
 * nor on how a run is cut into calls, and there is no per-agent state.  The granularity is the link and the
 * tick, not the packet: the receive fuses a sender's ACCLAIM with the COORDINATOR that follows it, and the task
 * tick relies on the election handlers only ever leaving FOLLOWER behind.
 * Arguments: swarm_update_loop_tasks', then ch and link_counts.  tasks == NULL or tasks->T == 0: the radio loop
 * (task_counts zeroed, *n_guard = 0).  ch == NULL or ch->loss == 0.0: swarm_update_loop_radio's /
 * swarm_update_loop_tasks' own kernels and bits, and link_counts is NOT written (those kernels do not count
 * links).  link_counts (host, ticks x 2, may be NULL), written when ch->loss > 0: per tick [0] the election
 * links -- ordered pairs of an alive receiver and an in-range sender j != i whose tick t-1 sends include an
 * ACCLAIM or a HEARTBEAT -- and [1] how many of those were dropped.  Claim-only and conflict-only senders are
 * not counted; they are dropped by the same rule.  A refused tick withholds link_counts (zeros).
 * SWARM_ERR_ARG (nothing written): ch->loss NaN, < 0 or > 1, and whatever the two loops refuse.
 * swarm_link_dropped: the rule on the host, 1 when the link is dropped, else 0 (needs no device).
 */
typedef struct {
    double loss;
    uint64_t seed;
} swarm_channel;

int swarm_update_loop_channel(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                              const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks, double dt,
                              double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                              int32_t n_kill, double *vel, double *target, uint8_t *has_target, int64_t m,
                              const double *obstacles, double radio_radius, double sense_radius, double max_speed,
                              double *trace, int32_t trace_every, int64_t *counts, int64_t *n_singular,
                              int64_t *refused_tick, const swarm_tasks *tasks, int64_t *task_counts,
                              int64_t *n_guard, void *stream, const swarm_channel *ch, int64_t *link_counts);

int swarm_link_dropped(uint64_t seed, int64_t t, int32_t sid, int32_t rid, double loss);

/*
 * Obstacle fields (contract O1): the sensed physics visits only the obstacles in reach.
 * A field is built once from a list of m obstacles (x, y, r) and is read-only afterwards.  It owns a device
 * copy of the list and, over a uniform grid that covers the obstacles' footprints, for every cell the
 * obstacles that can act on an agent in that cell, stored as packed (x, y, r) triples in list order.  An
 * obstacle acts only within 5 + r of its centre; it is listed in every cell its square of half side
 * (5 + r)(1 + 1e-9) touches, so an agent that visits its own cell's list, in list order, evaluates every term
 * the flat list's loop evaluates, in the same order: every output of a call given the field is bit-identical to
 * the same call given the same m obstacles as a flat list (the loop's far-obstacle test skips the others
 * without adding anything).  An obstacle with r <= -5 never acts and is in no list.
 *
 * Selection: no signature changes.  Pass m = the field's m and obstacles = the field's own list (the device
 * pointer swarm_obstacle_field_obstacles stores in *obstacles; every function here returns a status) to any
 * entry point that takes `m, obstacles`.  swarm_physics_run_sensed, swarm_update_loop_sensed,
 * swarm_update_loop_radio and swarm_update_loop_tasks recognise exactly that pointer with that m, on the ctx the
 * field was created on, and take the field's path: no LDS staging, no barriers, nothing done for an agent that
 * does not move.  Any other pointer (a copy of the list, an offset into it, another m) is a flat list and takes
 * the flat path.  swarm_physics_step and swarm_update_loop (fixed graphs) read the pointer as the flat list it
 * also is: the same bits by the contract.  The key is memory the library owns until the field is destroyed.
 *
 * swarm_obstacle_field_create: obstacles (device, m x 3 f64, may be NULL when m == 0) is copied; the lists are
 * built on the host, so the call waits for the stream once.  *info (may be NULL) describes the field.
 * SWARM_ERR_ARG, nothing created: a NULL ctx or out, m outside [0, 2^31), a NaN or infinite entry, footprints
 * whose bounding box has no finite extent.  SWARM_ERR_RANGE, nothing created: more than 2^26 (cell, obstacle)
 * pairs -- counted by arithmetic before any list is allocated, so that a few huge obstacles among many small
 * ones cannot fill memory.  The grid has at most 4 live + 1024 cells of side >= 10 (1 + 1e-9), whatever the radii:
 * obstacles whose reach spans very many such cells are what the pair limit refuses -- give those as a flat list.
 * swarm_obstacle_field_read (for tests and tools): cell_off_host (ncx * ncy + 1 u32) and idx_host (pairs i32,
 * the lists as obstacle indices, ascending in every cell; cell c = cy * ncx + cx holds
 * idx[cell_off[c] .. cell_off[c + 1])); either may be NULL.
 * swarm_obstacle_field_destroy waits for the device, then frees the field; swarm_ctx_destroy frees the fields
 * still alive.  A field must not be used after either.
 */
typedef struct swarm_obstacle_field swarm_obstacle_field;

typedef struct {
    int64_t m;       /* obstacles in the list */
    int64_t live;    /* those with 5 + r > 0 */
    int64_t ncx;     /* the grid: ncx x ncy cells of side `cell` from (xmin, ymin) */
    int64_t ncy;
    double cell;
    double xmin;
    double ymin;
    int64_t pairs;   /* (cell, obstacle) pairs: the length of all lists together */
    int64_t longest; /* the longest cell list */
} swarm_obstacle_field_info;

int swarm_obstacle_field_create(swarm_ctx *ctx, int64_t m, const double *obstacles, swarm_obstacle_field **out,
                                swarm_obstacle_field_info *info, void *stream);
int swarm_obstacle_field_obstacles(const swarm_obstacle_field *field, const double **obstacles);
int swarm_obstacle_field_read(const swarm_obstacle_field *field, uint32_t *cell_off_host, int32_t *idx_host);
int swarm_obstacle_field_destroy(swarm_ctx *ctx, swarm_obstacle_field *field);

/*
 * Moving obstacles (contract O2): fields rebuilt on the device every tick.
 * A moving field is a field (O1) whose list has one velocity (vx, vy) per obstacle; radii do not change.  The
 * field owns the current list O (m x 3 f64; its device pointer is still the field's key and never changes) and
 * the velocities (m x 2 f64).  For every sensed entry point given the field's pointer and m, with dt the call's
 * own dt:
 *   Reading.    The physics of tick t (step k) reads the agents' snapshot P_{t-1} and the list as it stands
 *               then, O_{t-1}.
 *   Advancing.  After that physics every obstacle advances once: x <- fl(x + fl(vx * dt)), y likewise; the
 *               product and the sum are rounded separately, r is untouched.  Live and dead (r <= -5) alike.
 *   In/out.     The list is in/out like pos: a run cut into chunks is the same run, and velocities may be
 *               changed between calls.
 *   Equivalence.  Every caller array, count, n_singular and the list itself after `ticks` ticks are
 *               bit-identical to `ticks` repetitions of: the same entry point with ticks = 1 and the current
 *               list as a flat list; then the advance above done by the caller.  (A moving field's tick is an
 *               O1 field of O_{t-1}, and O1 gives the flat list's bits on any grid.)
 *   Refusals.   A refused, too-dense tick of a loop (SWARM_ERR_RANGE, all or nothing) leaves the list as it was
 *               at entry, like every other array.  A refused swarm_physics_run_sensed step leaves it advanced
 *               exactly steps_done times, as pos is.  (A call with n == 0 or ticks == 0 runs no tick and
 *               advances nothing.)
 * The moving path is taken by swarm_physics_run_sensed, swarm_update_loop_sensed, _radio, _tasks and _channel.
 * swarm_physics_step and swarm_update_loop (fixed graphs) given a moving field's pointer return SWARM_ERR_ARG
 * with nothing written (they would read it as a frozen list); a static field there stays as it was.
 *
 * Per tick the cell lists are built on the call's stream with no host wait: per obstacle the live test, the
 * half side and the footprint's cell range (the static builder's arithmetic); an exclusive sum; the (cell,
 * obstacle) pairs written in ascending obstacle index; a stable radix sort by cell; the offsets by search; the
 * triples gathered from the current list -- no atomics, every cell's list ascending, the static builder's lists.
 * The grid is chosen once per call on the host, over the live footprints at entry and wherever the velocities
 * put them in `ticks` advances (the list is copied to the host within the call's existing entry wait); results
 * never depend on it.  The pair buffers are sized by a bound from the radii and the grid alone (per axis at most
 * min(nc, floor(2 h / cell) + 3) cells, h = (5 + r)(1 + 1e-9); csrc/obstacle_motion.h has the proof).
 * SWARM_ERR_ARG, nothing written: footprints whose box over the call has no finite extent.  SWARM_ERR_RANGE,
 * nothing written: a bound above 2^26 pairs, or a grid of more than 2^31 cells -- at create_moving on the
 * creation grid, at every call on the call's grid.  The device never writes past the capacity: a tick whose
 * pairs exceeded it would refuse the run at that tick (SWARM_ERR_RANGE), as a too-dense tick does.
 *
 * swarm_obstacle_field_create_moving: swarm_obstacle_field_create plus velocities (device, m x 2 f64; NULL: all
 * zero).  SWARM_ERR_ARG: a non-finite velocity, and whatever the static create refuses.
 * swarm_obstacle_field_obstacles returns the pointer of the current list: reading it after a call is how the
 * positions come back.
 * swarm_obstacle_field_set_velocities (waits for the stream): SWARM_ERR_ARG on a static field or a non-finite
 * entry, nothing changed.
 * swarm_obstacle_field_refresh (for tests and tools; waits): rebuilds the cell lists with the device builder for
 * the list as it stands, on the grid swarm_obstacle_field_create would choose for that list, and fills *info;
 * swarm_obstacle_field_read then returns those lists.  On a static field it only fills *info.
 */
int swarm_obstacle_field_create_moving(swarm_ctx *ctx, int64_t m, const double *obstacles, const double *velocities,
                                       swarm_obstacle_field **out, swarm_obstacle_field_info *info, void *stream);
int swarm_obstacle_field_set_velocities(swarm_ctx *ctx, swarm_obstacle_field *field, const double *velocities,
                                        void *stream);
int swarm_obstacle_field_refresh(swarm_ctx *ctx, swarm_obstacle_field *field, swarm_obstacle_field_info *info,
                                 void *stream);

/*
 * The task loop on boards of any size (contract U1-B): swarm_update_loop_tasks / _channel word for
 * word -- the receive, the two task handlers, the claim evaluation, the lossy channel, kills, the refusal of a
 * too-dense tick -- with 0 <= T <= 2^24 tasks and every agent's task state stored sparsely.  The 64-task loop
 * above is untouched and stays the faster one for the boards it takes.
 *
 * The board is a handle.  swarm_board_create copies tpos (device, T x 2 f64) and treq (device, T i8) and builds,
 * on the host (one wait for the stream), a grid over the tasks' bounding box with cells at least 5 (1 + 1e-9)
 * wide (at most 4 T + 1024 cells) and per cell its tasks in ascending index.  A task is claimed only within
 * distance 4 and evaluated only when dx * dx + dy * dy <= 25, so an agent looks at the tasks of the 3 x 3 task
 * cells around it and at no others; the grid only ever offers a superset, every offered task takes the loop's own
 * pre-test.  SWARM_ERR_ARG, nothing created: a NULL ctx or out, T outside [0, 2^24] (refused before the device is
 * touched), a NULL array with T > 0, a non-finite position, a box without a finite extent, a treq outside
 * [-1, 31].  swarm_board_info fills *info; swarm_board_read (for tests and tools) copies the cells' offsets
 * (ncx * ncy + 1 u32) and the cell-sorted task indices (T i32), either may be NULL.  swarm_board_destroy waits for
 * the device, then frees the board; swarm_ctx_destroy frees the boards still alive.
 *
 * swarm_board_state: every agent's task state, on the device, in/out, sparse and canonical -- the final bytes do
 * not depend on the order in which a kernel met the tasks, so a run cut into chunks equals the single run bit for
 * bit.  Ks status slots and Kt table slots per agent, each in [1, 4096], chosen by the caller:
 *   status        (n x Ks i32)  entries task << 2 | code, code 1 TENTATIVE, 2 LOCKED, 3 ASSIGNED (OPEN is never
 *                 stored), strictly ascending by task, the empty slots -1 behind the last entry;
 *   tab_task / tab_winner / tab_util  (n x Kt; i32, i32, f32)  the agent's task_claims ascending by task; an empty
 *                 slot has task -1, winner -1, utility 0.  A table survives its owner losing leadership;
 *   claim_out     (2 x n x Ks i32) / conflict_out (2 x n x Kt i32), by tick parity like the outbox: row
 *                 ((t & 1) n + i) holds the tasks agent i claimed / sent at least one TASK_CONFLICT on during tick
 *                 t, ascending, -1 behind the last.  The capacities suffice by construction: a claim takes a status
 *                 slot on the tick it is sent, a conflict names an entry of its sender's table;
 *   caps          (n u32) as swarm_allocate.
 * The winner a conflict names is read from its sender's table as it stood at the end of the previous tick; a
 * conflict on a task that table has no entry for (it can only come from a caller's arrays) reads as winner -1:
 * everyone LOCKED.
 *
 * Overflow is a refusal.  An agent that needs a (Ks + 1)-th status or a (Kt + 1)-th table entry during tick t
 * makes the call all or nothing, exactly as a too-dense tick does: SWARM_ERR_RANGE, *refused_tick = t, every
 * caller array back to its entry bytes (these six included), the counts withheld; no thread writes past a row.
 * *overflow (may be NULL) names the kind -- SWARM_BOARD_STATUS or SWARM_BOARD_TABLE, SWARM_BOARD_FITS otherwise
 * -- and one agent (storage index) that overflowed; when several do in that tick, any of them.  Both counts only
 * grow, so the refused tick is the first one at whose end the exact run holds more than the capacity.
 *
 * Entry checks, SWARM_ERR_ARG with nothing written: one device pass before any kernel indexes with a caller's
 * value -- every entry -1 or a task in [0, T), every status code in 1..3, every row strictly ascending with the
 * empties last (its verdict comes back with the entry bounding box's wait); a capacity outside [1, 4096]; a NULL
 * ctx, board, state or array; a board of another ctx; and whatever swarm_update_loop_channel refuses.
 * T == 0: swarm_update_loop_radio / its lossy form, task_counts zeroed, *n_guard = 0, no state array touched.
 * Arguments: swarm_update_loop_channel's with (board, state) in place of tasks, then overflow.  ch == NULL or
 * ch->loss == 0: the ideal channel, link_counts not written.
 */
typedef struct swarm_board swarm_board;

typedef struct {
    int64_t T;       /* tasks */
    int64_t ncx;     /* the grid: ncx x ncy cells of side `cell` from (xmin, ymin) */
    int64_t ncy;
    double cell;
    double xmin;
    double ymin;
    int64_t longest; /* the longest cell list */
} swarm_board_desc;

typedef struct {
    int32_t Ks;
    int32_t Kt;
    const uint32_t *caps;
    int32_t *status;
    int32_t *tab_task;
    int32_t *tab_winner;
    float *tab_util;
    int32_t *claim_out;
    int32_t *conflict_out;
} swarm_board_state;

#define SWARM_BOARD_FITS 0
#define SWARM_BOARD_STATUS 1
#define SWARM_BOARD_TABLE 2

typedef struct {
    int32_t kind;    /* SWARM_BOARD_* */
    int32_t pad;
    int64_t agent;   /* storage index, -1 when nothing overflowed */
} swarm_board_overflow;

int swarm_board_create(swarm_ctx *ctx, int64_t T, const double *tpos, const int8_t *treq, swarm_board **out,
                       swarm_board_desc *info, void *stream);
int swarm_board_info(const swarm_board *board, swarm_board_desc *info);
int swarm_board_read(const swarm_board *board, uint32_t *cell_off_host, int32_t *idx_host);
int swarm_board_destroy(swarm_ctx *ctx, swarm_board *board);

int swarm_update_loop_board(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                            const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks, double dt,
                            double timeout, double jitter, uint64_t seed, const int64_t *kill_ticks,
                            int32_t n_kill, double *vel, double *target, uint8_t *has_target, int64_t m,
                            const double *obstacles, double radio_radius, double sense_radius, double max_speed,
                            double *trace, int32_t trace_every, int64_t *counts, int64_t *n_singular,
                            int64_t *refused_tick, const swarm_board *board, const swarm_board_state *state,
                            int64_t *task_counts, int64_t *n_guard, void *stream, const swarm_channel *ch,
                            int64_t *link_counts, swarm_board_overflow *overflow);

/*
 * Moving tasks (contract U1-M): the board's cell grid rebuilt on the device every tick.
 * A moving board is a board (U1-B) with one velocity (vx, vy) per task.  It owns two position lists by task
 * index, `cur` and `lag` (T x 2 f64 each), and the velocities (T x 2 f64).  With Q_0 the creation positions:
 *   Reading.    Tick t of a call runs U1-B (U1-L when lossy) word for word with cur = Q_{t-1}: the grid, the far
 *               pre-test, the utility, the guard flag and the claim evaluation.  The claims of tick t-1 are heard
 *               with lag = Q_{t-2}: the handler recomputes the utility a claim was sent with.
 *   Advancing.  After the tick's kernels lag[k] = cur[k], then cur[k] = fl(cur[k] + fl(v[k] * dt)) per
 *               coordinate, the product and the sum rounded separately.
 *   In/out.     At creation lag = cur.  Both lists persist across calls: a run cut into chunks is the single run
 *               bit for bit.  swarm_board_set_velocities changes neither list.
 *   Refusals.   A refused tick (a status or table overflow, a too-dense tick: SWARM_ERR_RANGE, all or nothing)
 *               leaves both lists at their entry bytes, like the sparse rows.  A call with n == 0, T == 0 or
 *               ticks == 0 runs no tick and advances nothing.
 * Per tick the cell-sorted copy is built on the call's stream with no host wait: the tasks' cell keys on the
 * call's grid, a stable radix sort of (key, task index), the offsets by search, one gather of the (x, y) and
 * (index, treq) rows -- no atomics, every cell's tasks in ascending index, the host builder's lists.  The call's
 * grid covers the box of every task's span over `ticks` advances (csrc/task_motion.h has the proof that every
 * position of the call lies inside; an agent more than 6 beyond the box skips its task window), reduced on the
 * device and read with the call's existing entry wait.  SWARM_ERR_ARG, nothing written: a span that overflows or
 * a box without a finite extent.
 *
 * swarm_board_create_moving: swarm_board_create plus velocities (device, T x 2 f64; NULL: all zero).
 * SWARM_ERR_ARG, nothing created: a non-finite velocity, and whatever swarm_board_create refuses.
 * swarm_board_set_velocities (waits for the stream; NULL: all zero): SWARM_ERR_ARG on a static board or a
 * non-finite entry, nothing changed.
 * swarm_board_positions: the device pointers of cur and lag (a static board: its positions, twice); reading them
 * after a call is how the positions come back.
 * swarm_board_refresh (for tests and tools; waits): rebuilds the cell lists with the device builder for the
 * current list, on the grid swarm_board_create would choose for it, and fills *info; swarm_board_read then returns
 * those lists.  On a static board it only fills *info.
 * swarm_board_call_box (for tests and tools; waits): the device's span-box reduction for a call of `ticks` ticks
 * of dt, box_host = (xmin, ymin, xmax, ymax); xmax = +inf when a span is not finite.
 * swarm_update_loop_board_moving: swarm_update_loop_board's arguments with a moving board (SWARM_ERR_ARG for a
 * static one).  swarm_update_loop_board is unchanged for static boards and refuses a moving board with
 * SWARM_ERR_ARG, nothing written.
 */
int swarm_board_create_moving(swarm_ctx *ctx, int64_t T, const double *tpos, const int8_t *treq,
                              const double *velocities, swarm_board **out, swarm_board_desc *info, void *stream);
int swarm_board_set_velocities(swarm_ctx *ctx, swarm_board *board, const double *velocities, void *stream);
int swarm_board_positions(const swarm_board *board, const double **cur, const double **lag);
int swarm_board_refresh(swarm_ctx *ctx, swarm_board *board, swarm_board_desc *info, void *stream);
int swarm_board_call_box(swarm_ctx *ctx, swarm_board *board, double dt, int32_t ticks, double *box_host,
                         void *stream);
int swarm_update_loop_board_moving(swarm_ctx *ctx, int64_t n, const int32_t *ids, double *pos, double *pos_prev,
                                   const int32_t *tick_off, const swarm_fsm *fsm, int64_t t0, int32_t ticks,
                                   double dt, double timeout, double jitter, uint64_t seed,
                                   const int64_t *kill_ticks, int32_t n_kill, double *vel, double *target,
                                   uint8_t *has_target, int64_t m, const double *obstacles, double radio_radius,
                                   double sense_radius, double max_speed, double *trace, int32_t trace_every,
                                   int64_t *counts, int64_t *n_singular, int64_t *refused_tick, swarm_board *board,
                                   const swarm_board_state *state, int64_t *task_counts, int64_t *n_guard,
                                   void *stream, const swarm_channel *ch, int64_t *link_counts,
                                   swarm_board_overflow *overflow);

/*
 * Task lifetimes (contract U1-A): a board whose tasks open and close during a run.
 * A moving board may carry one window of absolute ticks per task -- the ticks a lossy channel hashes --
 * open_tick and close_tick (T i64 each).  Task k is present at tick t iff open[k] <= t < close[k]; INT64_MAX
 * never closes; open == close is never present.  A board without lifetimes is the board as it was.
 *   Handlers.   Before tick t every agent deletes tasks[k] for each k that stops being present and sets
 *               tasks[k] = OPEN for each k that becomes present; then the tick runs U1-B (U1-L, U1-M) word for word.
 *   Offering.   Only present tasks reach the claim evaluation and the guard-band count: an absent task is in no
 *               cell's run of the tick's lists.
 *   Conflicts.  A TASK_CONFLICT about a task absent at the receiving tick writes nothing.
 *   Claims.     A TASK_CLAIM about a task absent at the hearing tick is arbitrated as ever: the table entry is
 *               made and the conflict sent (nobody acts on it).  Table entries are never removed by a close.
 *   Positions.  cur / lag advance for absent tasks too.
 *   Retiring.   Tick t retires if some close[k] == t, or if it is the first tick of the first call after the
 *               lifetimes were set or changed: at its start every status entry of an absent task leaves its row,
 *               which is canonical again.  claim_out / conflict_out are message records and keep theirs.  A
 *               tick's removals precede its inserts, so a row overflows iff its end-of-tick count exceeds Ks.
 *   Refusals.   A refused call restores rows and positions as before; no call writes the lifetimes.  A run cut
 *               into chunks is the single run bit for bit, and all windows (0, INT64_MAX) give the bits of the
 *               board without lifetimes.
 * swarm_board_set_lifetimes (waits for the stream): open_tick / close_tick are device or host arrays, copied;
 * NULL / NULL removes the lifetimes.  SWARM_ERR_ARG, nothing changed: a NULL ctx or board, only one array, a board
 * of another ctx or a dead one, a static board, a negative tick, open > close.
 * swarm_board_lifetimes: the device pointers of the board's copies (NULL, NULL: none).
 * swarm_update_loop_board_moving is the entry point; swarm_update_loop_board refuses the board as any moving one.
 */
int swarm_board_set_lifetimes(swarm_ctx *ctx, swarm_board *board, const int64_t *open_tick, const int64_t *close_tick,
                              void *stream);
int swarm_board_lifetimes(const swarm_board *board, const int64_t **open_tick, const int64_t **close_tick);

/*
 * Placing tasks into the slots of closed ones (contract U1-P): a board of T slots serves an unbounded
 * stream of tasks with at most T alive at once -- the reference's `tasks` dict taking a new key.  Between calls, on
 * a moving board with lifetimes.  `last` is the last tick of the last successful swarm_update_loop_board_moving
 * call on the board (swarm_board_last_tick; -1: none yet).
 *   1 Eligibility (the quiet rule).  Slot k may be placed iff it was absent, under its current window, at ticks
 *     last and last - 1: close[k] <= last - 1, or open[k] > last, or open[k] == close[k].  The last claim about k
 *     was then heard at `close` at the latest and the conflict it caused at close + 1 <= last: no message in
 *     flight names k, and claim_out / conflict_out need no purge.
 *   2 Writes, per listed slot: cur[k] = lag[k] = the new position, treq[k], vel[k] (NULL: zero), open[k], close[k].
 *     The new window needs open >= last + 1 and open <= close.
 *   3 Purge.  Unless SWARM_PLACE_KEEP_TABLES is given, every claim-table entry about a placed slot leaves its row,
 *     at every agent, dead ones included; tab_task / tab_winner / tab_util move together and the row stays
 *     ascending with the empties (-1, -1, 0) last.  An entry outside [0, T) is kept.  With the flag the tables stay
 *     -- the reference re-adding the same task id: the old winner's hysteresis applies to the new life.  Status
 *     rows need nothing: the close retired them, and conflicts about an absent task write nothing.
 *   4 Equivalence.  A run that places with purge equals, slot for slot, the U1-A run over a board with one index per
 *     life: the statuses, tables and positions of the lives in slots, and every tick's counts.
 *   5 Schedule.  The new close ticks join the board's retiring ticks; entries <= last are dropped.  Host work is
 *     O(m log m + the number of closing ticks), never O(T).
 *   6 Refusals, SWARM_ERR_ARG with nothing changed on host or device: a NULL ctx, board or state; an unknown flag;
 *     n outside [0, 2^31); m < 0, or a NULL array (vel apart) with m > 0; state capacities outside [1, 4096]; a
 *     NULL table array when the purge would read it; a board of another ctx or a dead one; a static board or one
 *     without lifetimes; lifetimes set with no tick run since (the retire they owe has not happened); m > T; and,
 *     after the call's one host wait, the first request that names a slot outside [0, T), a slot that is not
 *     eligible, a negative tick, a window that opens at or before `last` or after it closes, a non-finite position
 *     or velocity, a treq outside [-1, 31]; a slot listed twice.  m == 0 is SWARM_OK and touches nothing.
 *   7 On a board that has been placed on, swarm_update_loop_board_moving refuses a call with n > 0 and ticks > 0
 *     whose t0 is not `last` (SWARM_ERR_ARG, nothing written).  Boards never placed on behave as before.
 *   8 A run cut into chunks with the same places between the same ticks is the same run bit for bit; a loop call
 *     refused after a place restores rows and positions to what they were after the place.
 * swarm_board_place: n agents' tables in `state` (only Ks, Kt and the three table arrays are read); m requests:
 * idx (m i32), tpos (m x 2 f64), treq (m i8), vel (m x 2 f64 or NULL), open_tick / close_tick (m i64), each a
 * device or a host array, copied.  The slots' current windows are fetched by a gather of m entries; after one host
 * wait the scatter and the purge (one pass over n x Kt task words; a row that loses nothing is only read) are
 * queued on the stream, and a second wait returns *purged (may be NULL), the number of table entries removed.
 */
#define SWARM_PLACE_KEEP_TABLES 1u
int swarm_board_place(swarm_ctx *ctx, swarm_board *board, int64_t n, const swarm_board_state *state, int64_t m,
                      const int32_t *idx, const double *tpos, const int8_t *treq, const double *vel,
                      const int64_t *open_tick, const int64_t *close_tick, uint32_t flags, int64_t *purged,
                      void *stream);
int swarm_board_last_tick(const swarm_board *board, int64_t *last_tick);

/*
 * Restoring the spatial storage order of a moved swarm (contract R1).  No reference counterpart: the
 * reference keeps its agents in a Python list.  Three calls: the order (swarm_resort_plan), the per-agent arrays
 * moved into it (swarm_permute_rows), the neighbour graph renamed to it (swarm_graph_relabel).  Every value that
 * indexes memory is checked on the device before it is used, and SWARM_ERR_ARG means that nothing was written.
 *
 * swarm_permute_rows: dst row k = src row from[k], for each of `count` arrays of n rows of row_bytes bytes
 * (device), in one pass: the rows of 1, 2, 4, 8 or 16 bytes whose src and dst are aligned to their width share one
 * launch, any other row is copied by ceil(row_bytes / 16) lanes (16, 4 or 1 bytes per lane, by what base and width
 * allow).  `from` (device, n) must be a permutation of [0, n): one bitmap pass (a 64-bit atomic OR per row), its
 * verdict read with one host wait, before any dst byte is written.  SWARM_ERR_ARG: a NULL ctx / from / arrays /
 * src / dst, n outside [0, 2^31), count outside [0, 64], a row_bytes outside [1, 16384] (a task board row of 4096
 * slots), a dst that overlaps a src, another dst or `from` (host pointer ranges; a src may be given twice), a
 * `from` that names a row outside [0, n) or a row twice.  All of these but the last are refused before the device
 * is touched.  n == 0 and count == 0 are no-ops.
 */
typedef struct swarm_rows {
    const void *src;
    void *dst;
    int64_t row_bytes;
} swarm_rows;

int swarm_permute_rows(swarm_ctx *ctx, int64_t n, const int32_t *from, int32_t count, const swarm_rows *arrays,
                       void *stream);

/*
 * The CSR (row_ptr, col) in a new numbering: out row k = in row from[k], every column c replaced by to[c] (to =
 * the inverse of from), the order inside a row kept.  row_ptr_out (device, n + 1) and col_out (device, row_ptr[n])
 * are the caller's.  Checked before anything is written, with one host wait: `from` as swarm_permute_rows checks
 * it, row_ptr starting at 0 and never decreasing, every column in [0, n) (the columns index `to`); row_ptr[n] is
 * taken as the length of col.  SWARM_ERR_ARG for any of these, for a NULL pointer (col and col_out may be NULL for
 * a graph without edges), n outside [0, 2^31 - 1) and an output that overlaps an input or the other output.
 */
int swarm_graph_relabel(swarm_ctx *ctx, int64_t n, const int32_t *from, const int32_t *row_ptr, const int32_t *col,
                        int32_t *row_ptr_out, int32_t *col_out, void *stream);

/*
 * The canonical order of contract R1 for agents stored as pos (device, n x 2 f64, storage order) with perm[k] the
 * input index of storage row k: perm_out (device, n) is what swarm_cell_order gives for the positions in input
 * order with `cell` -- agents of one cell in ascending INPUT index, whatever their storage order was -- and
 * from[k] (device, n) is the current storage row of the agent that belongs in row k; *moved (host) counts the rows
 * with from[k] != k.  Waits for the stream.  SWARM_ERR_ARG, nothing written: what swarm_cell_order refuses (a
 * position that is NaN or infinite, a box without a finite extent), a perm that is not a permutation of [0, n)
 * (the bitmap pass above), a NULL pointer, an output that overlaps an input or the other output.
 */
int swarm_resort_plan(swarm_ctx *ctx, int64_t n, const double *pos, const int32_t *perm, double cell, int32_t *from,
                      int32_t *perm_out, int64_t *moved, void *stream);

/*
 * Task census (contract U1-C): the per-task outcome of a task board, reduced on the device.  No
 * reference counterpart: the reference keeps every agent's tasks in its own dict.  Read-only: nothing of the board,
 * the state or the agents is written.
 *
 * Agent i (storage index) is counted iff mask == NULL or mask[i] != 0 (mask: device, n bytes).  For every task k in
 * [0, T), the ten arrays of swarm_census (device, T long each, all written by every successful call):
 *   tentative / locked / assigned  (i32)  counted agents whose status of k is TENTATIVE / LOCKED / ASSIGNED;
 *   tables                (i32)  counted agents whose claim table has an entry for k;
 *   holder_lo / holder_hi (i32)  the lowest / highest agent ID (ids[i], not i) among the ASSIGNED holders; -1, -1
 *                                when there is none;
 *   winner_lo / winner_hi (i32)  the lowest / highest winner ID the counted table entries name (they agree iff the
 *                                two are equal); -1, -1 without an entry;
 *   best_winner / best_util (i32, f32)  the counted table entry with the highest utility, among equal utilities the
 *                                lowest winner ID; -1, +0.0f without an entry.
 * Utilities compare by the order-preserving integer image of their f32 bits (b < 0 ? ~b : b | 2^31), which defines
 * the result for any bytes; the lows are minima of the IDs as unsigned words, the highs maxima as signed ones (the
 * library's IDs are never negative, so both are the plain order).  Every output is a commutative integer
 * reduction: the census is bit-exact, whatever the storage order and the kernel's schedule.
 *
 * holders (device, cap pairs of i32, 8-byte aligned; NULL with cap == 0): every (task, agent ID) pair with a
 * counted ASSIGNED status, in any order, through a wave-aggregated cursor; never more than cap pairs are written.
 * *n_holders (host, may be NULL) is the exact total, sum(assigned), which may exceed cap: the first
 * min(cap, total) slots then hold true pairs, and a second call with cap >= total returns them all.
 *
 * swarm_board_census: the sparse board of swarm_update_loop_board (static or moving).  Of `state` only Ks, Kt,
 * status, tab_task, tab_winner and tab_util are read.  swarm_tasks_census: the 64-task board of
 * swarm_update_loop_tasks, from the two status words and the dense n x T tables; an entry is a tab_winner >= 0,
 * status bits at or above T are no tasks and are ignored.  Both wait for the stream once, at the end.
 *
 * SWARM_ERR_ARG before the device is touched: a NULL ctx, board, state, out or array (ids and the state arrays may
 * be NULL when n == 0); a board that is no live board of ctx; Ks or Kt outside [1, 4096]; T outside [0, 64] for the
 * 64-task form; n outside [0, 2^31); cap < 0; holders NULL with cap > 0, or misaligned.
 * SWARM_ERR_ARG from the device (swarm_board_census): rows that are not canonical, by the rule of
 * swarm_update_loop_board's entry pass -- every status / tab_task entry -1 or a task in [0, T), every status code
 * in 1..3, every row strictly ascending with the empties last.  The check is folded into the census pass: every
 * entry is range-checked by the thread that loaded it before it indexes anything.  After this refusal the ten
 * arrays and holders are unspecified; nothing outside them has been written.
 * T == 0: success, nothing launched, *n_holders = 0.  n == 0: success, the arrays hold their empty values.
 * Scratch: 8 T + 64 bytes of the ctx (a packed (utility image, ~winner) key per task).
 */
typedef struct {
    int32_t *tentative;
    int32_t *locked;
    int32_t *assigned;
    int32_t *tables;
    int32_t *holder_lo;
    int32_t *holder_hi;
    int32_t *winner_lo;
    int32_t *winner_hi;
    int32_t *best_winner;
    float *best_util;
} swarm_census;

int swarm_board_census(swarm_ctx *ctx, int64_t n, const int32_t *ids, const swarm_board *board,
                       const swarm_board_state *state, const uint8_t *mask, const swarm_census *out, int32_t *holders,
                       int64_t cap, int64_t *n_holders, void *stream);
int swarm_tasks_census(swarm_ctx *ctx, int64_t n, const int32_t *ids, int32_t T, const uint64_t *status_lo,
                       const uint64_t *status_hi, const int32_t *tab_winner, const float *tab_util,
                       const uint8_t *mask, const swarm_census *out, int32_t *holders, int64_t cap,
                       int64_t *n_holders, void *stream);

/*
 * Agent lifetimes (contract U1-J): agents that boot and die during a run.  The reference runs one
 * process per agent (agent.py:349-358); a process that starts late is a fresh SwarmAgent.__init__ (agent.py:25-54),
 * one that stops simply stops, one that restarts is both.
 *
 * Agent i (storage index) carries one window of absolute ticks and is up at tick t iff boot[i] <= t < death[i].
 * The defaults boot = 0 and death = INT64_MAX mean "as it is, forever": with them every loop gives the bits it
 * gives without a handle.  An agent with boot >= death is never up and has no events.
 *
 * swarm_agent_life_create attaches the windows (host arrays, n each, copied) to the swarm whose alive flags
 * (device, n bytes: the array every loop is given as fsm->alive) and tick offsets (device, n int32: the loops'
 * tick_off) are named; it touches no device memory.  Every protocol run and update loop of this ctx that is given
 * this alive array then runs the events below; it must be given this tick_off as well (SWARM_ERR_ARG otherwise).
 * One handle per alive array.  The two device arrays must outlive the handle.
 *
 * swarm_agent_life_set replaces the windows and applies the set-time rule, with last_tick the last tick run:
 * agents with boot > last_tick or death <= last_tick get alive = 0, all others keep the flag they have (an agent
 * killed at a kill tick stays dead), nothing else is written.  It waits for the stream.  A second window for an
 * agent that has died gives a rebirth.
 *
 * At the start of tick t of a call, after the leader kill of a kill tick: first the deaths, then the boots.
 *   death (death[i] == t)  alive = 0 and nothing else, exactly what a kill-tick victim is: what it sent during
 *          t - 1 is still heard at t, its position stays and stays a separation neighbour.
 *   boot  (boot[i] == t)   a fresh SwarmAgent constructed at the clock of tick t - 1: alive, FOLLOWER, leader -1,
 *          no leader position, last_hb = (t - 1) dt, wait_start = delay = 0, its own tick counter 1 at tick t
 *          (tick_off[i] = 1 - t), velocity 0, no target, both outbox halves empty; in the task loops an empty
 *          status row (every task OPEN to it again), an empty claim table and no claim or conflict in flight, the
 *          sparse rows in the empty encoding (-1 slots, utilities +0.0f).  Position, ID and capabilities stay.  It
 *          receives at tick t what the up agents in range sent during t - 1.  A boot of an agent that is up is a
 *          restart.
 *          (swarm_protocol_run / _ex are not given velocity, target and has_target and leave them alone.)
 * Every absolute tick runs once, so a run cut into calls is the single run bit for bit.  A refused call (a tick too
 * dense to sense, a board overflow) writes nothing, tick_off included, and the repeated call fires the same events.
 * A tick without events launches nothing; on a tick with events one kernel runs over that tick's events alone.
 *
 * swarm_agent_life_events: events (host, ticks x 2) = per tick of the call t0 + 1 .. t0 + ticks the agents that
 * boot and the agents that die, from the schedule alone (host only).
 * swarm_agent_life_destroy: the handle is dead (NULL: nothing happens); the loops run as without it.  Handles
 * still alive are freed with their ctx.
 *
 * SWARM_ERR_ARG before anything is written, without a device: a NULL ctx, out, handle or array (the arrays may be
 * NULL when n == 0); n outside [0, 2^31), or not the handle's; a handle that is dead or no handle of ctx; a boot
 * tick outside [0, 2^31); a negative death tick or last_tick; an alive array that already has a handle.
 */
typedef struct swarm_agent_life swarm_agent_life;

int swarm_agent_life_create(swarm_ctx *ctx, int64_t n, const int64_t *boot, const int64_t *death, uint8_t *alive,
                            int32_t *tick_off, swarm_agent_life **out);
int swarm_agent_life_set(swarm_ctx *ctx, swarm_agent_life *life, int64_t n, const int64_t *boot, const int64_t *death,
                         int64_t last_tick, void *stream);
int swarm_agent_life_events(swarm_ctx *ctx, const swarm_agent_life *life, int64_t t0, int32_t ticks, int64_t *events);
int swarm_agent_life_destroy(swarm_ctx *ctx, swarm_agent_life *life);

#ifdef __cplusplus
}
#endif

#endif /* SWARM_H */
