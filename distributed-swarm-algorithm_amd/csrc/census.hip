// Task census (contract U1-C): the per-task outcome of a task board, reduced on the device.  Read-only
// over the board: a transpose from agent-major rows to per-task records, every field a commutative integer
// reduction, so the result is bit-exact whatever the storage order and the schedule.
//
// Plan.  A workgroup takes a contiguous range of agents (the storage order is spatial: its agents see the same few
// tasks), reads their rows coalesced -- a wave covers whole consecutive rows, 16 bytes per lane where the row width
// allows -- and aggregates in LDS: the sparse form in an open-addressed table keyed by task, the 64-task form in 64
// records outright.  At the end it flushes one global atomic per distinct (task, field) that it touched.  A task
// that finds no table slot within kProbes probes goes to the global records directly: slower, still exact.  The
// canonical-row check of the sparse form is folded into the same read: every entry is range-checked by the thread
// that loaded it before it indexes anything, and the order check only feeds the verdict word.
#include "swarm_common.h"

namespace swarm {
namespace {

constexpr int kSlotBits = 9;
constexpr int kSlots = 1 << kSlotBits;  // LDS table slots of the sparse form: 44 bytes each, 22 KB per workgroup
                                        // (256: 1.15 ms, 512: 0.78 ms, 1024: 0.99 ms per call at 10M agents)
constexpr int kProbes = 8;              // linear probes before a task goes to the global records
constexpr int kStage = 512;             // holder pairs a workgroup stages in LDS before its one cursor add (4 KB)
constexpr int kMaxSlots = 4096;         // swarm_board_state's row capacity
constexpr int64_t kMaxBlocks = 4096;
constexpr int64_t kMinAgents = 128;         // agents per workgroup at least ...
constexpr int64_t kMaxAgents = 1 << 19;     // ... and at most: a workgroup's slots (x 4096) index with 32 bits
constexpr uint32_t kNoId = 0xFFFFFFFFu;     // the unsigned-min start value: reads as -1

// The order-preserving integer image of an f32's bits, and its inverse.
__device__ __forceinline__ uint32_t util_image(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ uint32_t util_bits(uint32_t o) { return (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o; }
__device__ __forceinline__ unsigned long long best_key(uint32_t winner, uint32_t ubits) {
    return (static_cast<unsigned long long>(util_image(ubits)) << 32) | uint32_t(~winner);
}

// The global records (swarm_census, the two minima as the unsigned words they are reduced as) and the scratch.
struct Records {
    uint32_t *cnt[4];  // tentative, locked, assigned (status code - 1), tables
    uint32_t *hlo;
    int32_t *hhi;
    uint32_t *wlo;
    int32_t *whi;
    unsigned long long *key;     // scratch: per task the highest (utility image, ~winner)
    unsigned long long *bad;     // scratch: the verdict word
    unsigned long long *cursor;  // scratch: the holder pairs' cursor / total
    int2 *pairs;                 // the caller's holder buffer, or NULL
    long long cap;
};

// A workgroup's records in LDS, by table slot (sparse form) or by task (64-task form).
template <int S>
struct Local {
    int32_t task[S];
    uint32_t cnt[4][S];
    uint32_t hlo[S];
    int32_t hhi[S];
    uint32_t wlo[S];
    int32_t whi[S];
    unsigned long long best[S];
    unsigned long long total;  // ASSIGNED entries counted when no pair buffer was given
};

// A workgroup's holder pairs on their way to the caller's buffer: n counts every pair offered, the first kStage of
// them are staged here and leave with one add to the global cursor, the others go there wave by wave.
struct Stage {
    int2 pair[kStage];
    unsigned n;
    unsigned long long base;
};

template <int S>
__device__ __forceinline__ void local_clear(Local<S> &t) {
    for (int s = threadIdx.x; s < S; s += kBlock) {
        t.task[s] = -1;
        for (int c = 0; c < 4; ++c) t.cnt[c][s] = 0;
        t.hlo[s] = t.wlo[s] = kNoId;
        t.hhi[s] = t.whi[s] = -1;
        t.best[s] = 0;
    }
    if (threadIdx.x == 0) t.total = 0;
    __syncthreads();
}

// Slot s of the workgroup's records into the global record of `task` (checked by whoever stored it).
template <int S>
__device__ __forceinline__ void local_flush(const Local<S> &t, int s, int32_t task, const Records &o) {
    for (int c = 0; c < 4; ++c)
        if (t.cnt[c][s]) atomicAdd(o.cnt[c] + task, t.cnt[c][s]);
    if (t.cnt[2][s]) {
        atomicMin(o.hlo + task, t.hlo[s]);
        atomicMax(o.hhi + task, t.hhi[s]);
    }
    if (t.cnt[3][s]) {
        atomicMin(o.wlo + task, t.wlo[s]);
        atomicMax(o.whi + task, t.whi[s]);
        atomicMax(o.key + task, t.best[s]);
    }
}

// The table slot of `task` (claimed if new), or -1 when kProbes probes found neither it nor a free slot.
__device__ __forceinline__ uint32_t table_home(int32_t task) {
    return (uint32_t(task) * 2654435761u) >> (32 - kSlotBits);
}
__device__ __forceinline__ int table_slot(Local<kSlots> &t, int32_t task) {
    const uint32_t h = table_home(task);
    for (int p = 0; p < kProbes; ++p) {
        const int s = int((h + p) & (kSlots - 1));
        int32_t k = __hip_atomic_load(&t.task[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == -1) k = atomicCAS(&t.task[s], -1, task);
        if (k == -1 || k == task) return s;
    }
    return -1;
}

// `count` agents with status `code` of a task / one ASSIGNED holder / one table entry into slot s of the workgroup's
// records, or (s < 0) into the global ones.
template <int S>
__device__ __forceinline__ void add_count(Local<S> &t, int s, int32_t task, int code, uint32_t count,
                                          const Records &o) {
    if (s >= 0)
        atomicAdd(&t.cnt[code - 1][s], count);
    else
        atomicAdd(o.cnt[code - 1] + task, count);
}

template <int S>
__device__ __forceinline__ void add_holder(Local<S> &t, int s, int32_t task, int32_t id, const Records &o) {
    if (s >= 0) {
        atomicMin(&t.hlo[s], uint32_t(id));
        atomicMax(&t.hhi[s], id);
    } else {
        atomicMin(o.hlo + task, uint32_t(id));
        atomicMax(o.hhi + task, id);
    }
}

template <int S>
__device__ __forceinline__ void add_entry(Local<S> &t, int s, int32_t task, int32_t winner, uint32_t ubits,
                                          const Records &o) {
    const unsigned long long key = best_key(uint32_t(winner), ubits);
    if (s >= 0) {
        atomicAdd(&t.cnt[3][s], 1u);
        atomicMin(&t.wlo[s], uint32_t(winner));
        atomicMax(&t.whi[s], winner);
        atomicMax(&t.best[s], key);
    } else {
        atomicAdd(o.cnt[3] + task, 1u);
        atomicMin(o.wlo + task, uint32_t(winner));
        atomicMax(o.whi + task, winner);
        atomicMax(o.key + task, key);
    }
}

// The (task, ID) pair of every lane with `on` on its way to the caller's buffer, through wave-aggregated cursors:
// one LDS add per wave into the workgroup's stage, and for the pairs the stage has no room for one add per wave to
// the global cursor (one word takes about 90 returning adds per microsecond, chip-wide: a wave-level global cursor
// alone cost 15 ms at 700 000 pairs).  Without a buffer the wave's count goes to the workgroup's total.  Every lane
// of the wave calls it (convergent).
__device__ __forceinline__ void append_holders(bool on, int32_t task, int32_t id, const Records &o, Stage &st,
                                               unsigned long long *total) {
    const unsigned long long m = __ballot(on);
    if (m == 0) return;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int first = __ffsll(static_cast<long long>(m)) - 1;
    if (!o.pairs) {
        if (lane == first) atomicAdd(total, static_cast<unsigned long long>(__popcll(m)));
        return;
    }
    unsigned at = 0;
    if (lane == first) at = atomicAdd(&st.n, unsigned(__popcll(m)));
    at = __shfl(at, first) + unsigned(__popcll(m & ((1ull << lane) - 1ull)));
    const bool spill = on && at >= unsigned(kStage);
    if (on && !spill) st.pair[at] = make_int2(task, id);
    const unsigned long long m2 = __ballot(spill);
    if (m2 == 0) return;
    const int first2 = __ffsll(static_cast<long long>(m2)) - 1;
    unsigned long long base = 0;
    if (lane == first2) base = atomicAdd(o.cursor, static_cast<unsigned long long>(__popcll(m2)));
    base = __shfl(base, first2) + static_cast<unsigned long long>(__popcll(m2 & ((1ull << lane) - 1ull)));
    if (spill && base < static_cast<unsigned long long>(o.cap)) o.pairs[base] = make_int2(task, id);
}

// The staged pairs into the caller's buffer, after the workgroup's last append (all threads; pairs != NULL).
__device__ __forceinline__ void flush_holders(Stage &st, const Records &o) {
    const unsigned count = st.n < unsigned(kStage) ? st.n : unsigned(kStage);
    if (threadIdx.x == 0 && count) st.base = atomicAdd(o.cursor, static_cast<unsigned long long>(count));
    __syncthreads();
    for (unsigned i = threadIdx.x; i < count; i += kBlock) {
        const unsigned long long at = st.base + i;
        if (at < static_cast<unsigned long long>(o.cap)) o.pairs[at] = st.pair[i];
    }
}

template <int V>
struct Vec;
template <>
struct Vec<1> {
    int32_t e[1];
    __device__ __forceinline__ void load(const int32_t *p) { e[0] = p[0]; }
};
template <>
struct Vec<4> {
    int32_t e[4];
    __device__ __forceinline__ void load(const int32_t *p) {
        const int4 v = *reinterpret_cast<const int4 *>(p);
        e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
    }
};

struct BoardArgs {
    int64_t n;
    int64_t per;  // agents per workgroup
    int32_t T;
    int Ks, Kt;
    const int32_t *ids;
    const uint8_t *mask;
    const int32_t *status;
    const int32_t *tab_task;
    const int32_t *tab_winner;
    const uint32_t *tab_util;
    Records o;
};

// One sparse array of a workgroup's agents [a0, a0 + len / K): the statuses (kStatus: entries task << 2 | code) or
// the table's tasks.  V entries per lane, V | K, so that a lane's entries lie in one row.  Returns the verdict.
template <int V, bool kStatus>
__device__ __forceinline__ bool walk_rows(const BoardArgs &a, Local<kSlots> &t, Stage &st,
                                          const int32_t *__restrict__ rows, int K, int64_t a0, uint32_t len) {
    constexpr int sh = kStatus ? 2 : 0;
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int64_t s0 = a0 * K;
    const int ksh = (K & (K - 1)) == 0 ? __ffs(K) - 1 : -1;
    bool wrong = false;
    Vec<V> next;  // the trip after this one's entries, loaded before this trip's LDS round trips
    for (int j = 0; j < V; ++j) next.e[j] = -1;
    if (threadIdx.x * V < len) next.load(rows + s0 + threadIdx.x * V);
    for (uint32_t base = 0; base < len; base += uint32_t(kBlock) * V) {  // the same trips for the whole workgroup
        const uint32_t r = base + threadIdx.x * V;
        const bool in = r < len;
        const Vec<V> v = next;
        for (int j = 0; j < V; ++j) next.e[j] = -1;
        if (r + uint32_t(kBlock) * V < len) next.load(rows + s0 + r + uint32_t(kBlock) * V);
        const uint32_t row = ksh >= 0 ? r >> ksh : r / uint32_t(K);
        const uint32_t at = r - row * uint32_t(K);  // the first entry's place in its row
        int32_t prev = __shfl_up(v.e[V - 1], 1);
        if (lane == 0 && in && at) prev = rows[s0 + r - 1];
        const int64_t agent = a0 + row;
        bool ok[V], any = false;
        for (int j = 0; j < V; ++j) {
            const int32_t e = v.e[j];
            ok[j] = false;
            if (e != -1) {
                if (e < 0 || (e >> sh) >= a.T || (kStatus && (e & 3) == 0)) {
                    wrong = true;
                } else {
                    ok[j] = true;
                    if (at + j) wrong |= prev < 0 || (prev >> sh) >= (e >> sh);
                }
            }
            any |= ok[j];
            prev = e;
        }
        const bool counted = any && (!a.mask || a.mask[agent] != 0);
        int32_t id = 0;
        if (kStatus) {
            bool holds = false;
            for (int j = 0; j < V; ++j) holds |= ok[j] && (v.e[j] & 3) == 3;
            if (counted && holds) id = a.ids[agent];
        }
        // the lane's V home slots read together (and a table entry's winner and utility): one LDS round trip where
        // the tasks are already there, which they are after a workgroup's first few trips
        int32_t home[V], winner[V];
        uint32_t ubits[V];
        for (int j = 0; j < V; ++j) {
            home[j] = -1, winner[j] = -1, ubits[j] = 0;
            if (counted && ok[j]) {
                home[j] = __hip_atomic_load(&t.task[table_home(v.e[j] >> sh)], __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_WORKGROUP);
                if (!kStatus) winner[j] = a.tab_winner[s0 + r + j], ubits[j] = a.tab_util[s0 + r + j];
            }
        }
        for (int j = 0; j < V; ++j) {
            const bool use = counted && ok[j];
            const int32_t e = v.e[j], task = e >> sh;  // task in [0, T) where `use`
            const int code = e & 3;
            if (!kStatus) {
                if (use) add_entry(t, home[j] == task ? int(table_home(task)) : table_slot(t, task), task, winner[j],
                                   ubits[j], a.o);
                continue;
            }
            const bool holds = use && code == 3;
            if (use) {
                const int s = home[j] == task ? int(table_home(task)) : table_slot(t, task);
                add_count(t, s, task, code, 1u, a.o);
                if (holds) add_holder(t, s, task, id, a.o);
            }
            append_holders(holds, task, id, a.o, st, &t.total);
        }
    }
    return wrong;
}

template <int VS, int VT>
__global__ __launch_bounds__(kBlock) void k_census_board(const BoardArgs a) {
    __shared__ Local<kSlots> t;
    __shared__ Stage st;
    if (threadIdx.x == 0) st.n = 0;
    local_clear(t);
    const int64_t a0 = int64_t(blockIdx.x) * a.per;
    const int64_t a1 = a0 + a.per < a.n ? a0 + a.per : a.n;
    bool wrong = false;
    if (a0 < a1) {
        wrong |= walk_rows<VS, true>(a, t, st, a.status, a.Ks, a0, uint32_t((a1 - a0) * a.Ks));
        wrong |= walk_rows<VT, false>(a, t, st, a.tab_task, a.Kt, a0, uint32_t((a1 - a0) * a.Kt));
    }
    if (wrong) *a.o.bad = 1;
    __syncthreads();
    for (int s = threadIdx.x; s < kSlots; s += kBlock)
        if (t.task[s] >= 0) local_flush(t, s, t.task[s], a.o);
    if (threadIdx.x == 0 && t.total) atomicAdd(a.o.cursor, t.total);
    if (a.o.pairs) flush_holders(st, a.o);
}

struct TasksArgs {
    int64_t n;
    int64_t per;
    int32_t T;
    const int32_t *ids;
    const uint8_t *mask;
    const unsigned long long *status_lo;
    const unsigned long long *status_hi;
    const int32_t *tab_winner;
    const uint32_t *tab_util;
    Records o;
};

// The 64-task board: the counts from the two status words by ballot and popcount (lane k keeps task k's), the dense
// table scanned for winners >= 0 and its utilities read only there.
template <int V>
__global__ __launch_bounds__(kBlock) void k_census_tasks(const TasksArgs a) {
    __shared__ Local<kWave> t;
    __shared__ Stage st;
    if (threadIdx.x == 0) st.n = 0;
    local_clear(t);
    const int lane = int(threadIdx.x) & (kWave - 1);
    const int T = a.T;
    const int64_t a0 = int64_t(blockIdx.x) * a.per;
    const int64_t a1 = a0 + a.per < a.n ? a0 + a.per : a.n;
    const unsigned long long live = T >= 64 ? ~0ull : (1ull << T) - 1ull;  // bits at or above T are no tasks
    uint32_t c1 = 0, c2 = 0, c3 = 0;
    for (int64_t base = a0; base < a1; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        unsigned long long lo = 0, hi = 0;
        if (i < a1 && (!a.mask || a.mask[i] != 0)) lo = a.status_lo[i] & live, hi = a.status_hi[i] & live;
        const int32_t id = (lo & hi) ? a.ids[i] : 0;
        for (int k = 0; k < T; ++k) {
            const unsigned long long b1 = __ballot((lo >> k) & 1), b2 = __ballot((hi >> k) & 1);
            if (lane == k) c1 += __popcll(b1 & ~b2), c2 += __popcll(~b1 & b2), c3 += __popcll(b1 & b2);
            if (b1 & b2) {  // the same for the whole wave
                const bool on = ((lo & hi) >> k) & 1;
                if (on) {
                    atomicMin(&t.hlo[k], uint32_t(id));
                    atomicMax(&t.hhi[k], id);
                }
                append_holders(on, k, id, a.o, st, &t.total);
            }
        }
    }
    if (c1) atomicAdd(&t.cnt[0][lane], c1);
    if (c2) atomicAdd(&t.cnt[1][lane], c2);
    if (c3) atomicAdd(&t.cnt[2][lane], c3);
    if (a0 < a1) {
        const int64_t s0 = a0 * T;
        const uint32_t len = uint32_t((a1 - a0) * T);
        for (uint32_t base = 0; base < len; base += uint32_t(kBlock) * V) {
            const uint32_t r = base + threadIdx.x * V;
            if (r >= len) break;
            Vec<V> w;
            w.load(a.tab_winner + s0 + r);
            bool any = false;
            for (int j = 0; j < V; ++j) any |= w.e[j] >= 0;
            if (!any) continue;
            const uint32_t row = r / uint32_t(T);
            if (a.mask && a.mask[a0 + row] == 0) continue;
            for (int j = 0; j < V; ++j)
                if (w.e[j] >= 0) {
                    const int task = int(r - row * uint32_t(T)) + j;  // V | T: the lane's entries lie in one row
                    add_entry(t, task, task, w.e[j], a.tab_util[s0 + r + j], a.o);
                }
        }
    }
    __syncthreads();
    if (int(threadIdx.x) < T) local_flush(t, threadIdx.x, int32_t(threadIdx.x), a.o);
    if (threadIdx.x == 0 && t.total) atomicAdd(a.o.cursor, t.total);
    if (a.o.pairs) flush_holders(st, a.o);
}

// The records' start values -- zero counts, unsigned-min / signed-max identities that read as -1 -- and the scratch.
__global__ __launch_bounds__(kBlock) void k_census_init(int64_t T, const Records o) {
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < T; k += int64_t(gridDim.x) * kBlock) {
        for (int c = 0; c < 4; ++c) o.cnt[c][k] = 0;
        o.hlo[k] = o.wlo[k] = kNoId;
        o.hhi[k] = o.whi[k] = -1;
        o.key[k] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *o.bad = 0, *o.cursor = 0;
}

// best_winner / best_util from the packed keys; a task without a counted entry reads (-1, +0.0f).
__global__ __launch_bounds__(kBlock) void k_census_best(int64_t T, const Records o, int32_t *__restrict__ best_winner,
                                                       uint32_t *__restrict__ best_util) {
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < T; k += int64_t(gridDim.x) * kBlock) {
        const bool has = o.cnt[3][k] != 0;
        const unsigned long long key = o.key[k];
        best_winner[k] = has ? int32_t(~uint32_t(key)) : -1;
        best_util[k] = has ? util_bits(uint32_t(key >> 32)) : 0u;
    }
}

bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// What both forms refuse before the device is touched (after their own NULL checks of ctx and out).
int check_common(const int32_t *ids, int64_t n, const swarm_census *out, const int32_t *holders, int64_t cap) {
    SW_ARG(n >= 0 && n < (int64_t(1) << 31), "n must be in [0, 2^31)");
    SW_ARG(out->tentative && out->locked && out->assigned && out->tables && out->holder_lo && out->holder_hi &&
               out->winner_lo && out->winner_hi && out->best_winner && out->best_util,
           "NULL census array");
    SW_ARG(n == 0 || ids != nullptr, "ids is NULL");
    SW_ARG(cap >= 0, "cap must not be negative");
    SW_ARG(cap == 0 || holders != nullptr, "holders is NULL with cap > 0");
    SW_ARG(reinterpret_cast<uintptr_t>(holders) % 8 == 0, "holders is not aligned to a pair");
    return SWARM_OK;
}

struct Call {
    Records o{};
    unsigned long long *host = nullptr;  // pinned: verdict, total
    int64_t per = 0;
    unsigned blocks = 0;
};

// The scratch, the records' start values and the workgroups' share of the agents.
int begin(swarm_ctx *ctx, int64_t n, int64_t T, const swarm_census *out, int32_t *holders, int64_t cap, Call *c,
          hipStream_t s) {
    unsigned long long *buf;
    SW_ALLOC(buf, ctx, S_CENSUS, 64 + size_t(T) * 8);
    c->host = static_cast<unsigned long long *>(pinned(ctx, 64));
    if (!c->host) return SWARM_ERR_OOM;
    Records &o = c->o;
    o.cnt[0] = reinterpret_cast<uint32_t *>(out->tentative);
    o.cnt[1] = reinterpret_cast<uint32_t *>(out->locked);
    o.cnt[2] = reinterpret_cast<uint32_t *>(out->assigned);
    o.cnt[3] = reinterpret_cast<uint32_t *>(out->tables);
    o.hlo = reinterpret_cast<uint32_t *>(out->holder_lo);
    o.hhi = out->holder_hi;
    o.wlo = reinterpret_cast<uint32_t *>(out->winner_lo);
    o.whi = out->winner_hi;
    o.bad = buf;
    o.cursor = buf + 1;
    o.key = buf + 8;
    o.pairs = cap > 0 ? reinterpret_cast<int2 *>(holders) : nullptr;
    o.cap = cap;
    hipLaunchKernelGGL(k_census_init, dim3(grid_for(T, kBlock, 8192)), dim3(kBlock), 0, s, T, o);
    SW_LAUNCHED();
    int64_t per = (n + kMaxBlocks - 1) / kMaxBlocks;
    per = per < kMinAgents ? kMinAgents : per;  // (n < 2^31: never above kMaxAgents)
    static_assert((int64_t(1) << 31) / kMaxBlocks <= kMaxAgents, "a workgroup's slots must index with 32 bits");
    c->per = per;
    c->blocks = unsigned((n + per - 1) / per);
    return SWARM_OK;
}

// best_*, then the one host wait: the verdict and the pairs' total.
int finish(const Call &c, int64_t T, const swarm_census *out, int64_t *n_holders, const char *who, hipStream_t s) {
    hipLaunchKernelGGL(k_census_best, dim3(grid_for(T, kBlock, 8192)), dim3(kBlock), 0, s, T, c.o, out->best_winner,
                       reinterpret_cast<uint32_t *>(out->best_util));
    SW_LAUNCHED();
    c.host[0] = 1;  // (overwritten by the copy: a wait that never came reads as a refusal)
    SW_HIP(hipMemcpyAsync(c.host, c.o.bad, 16, hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    if (c.host[0] != 0) {
        set_error("invalid argument: %s: a sparse task row holds an entry that is no task of the board, a status code "
                  "outside 1..3, or is not strictly ascending with its empty slots last",
                  who);
        return SWARM_ERR_ARG;
    }
    if (n_holders) *n_holders = int64_t(c.host[1]);
    return SWARM_OK;
}

}  // namespace
}  // namespace swarm

extern "C" {

int swarm_board_census(swarm_ctx *ctx, int64_t n, const int32_t *ids, const swarm_board *board,
                       const swarm_board_state *state, const uint8_t *mask, const swarm_census *out, int32_t *holders,
                       int64_t cap, int64_t *n_holders, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(board != nullptr, "board is NULL");
    SW_ARG(state != nullptr, "state is NULL");
    SW_ARG(out != nullptr, "out is NULL");
    SW_ARG(state->Ks >= 1 && state->Ks <= kMaxSlots && state->Kt >= 1 && state->Kt <= kMaxSlots,
           "status and table slots must be in [1, 4096]");
    if (const int rc = check_common(ids, n, out, holders, cap)) return rc;
    SW_ARG(n == 0 || (state->status && state->tab_task && state->tab_winner && state->tab_util),
           "NULL board state array");
    SW_ARG(live_board(ctx, board), "board is not a live board of this ctx");
    if (n_holders) *n_holders = 0;
    const int64_t T = board->T;
    if (T == 0) return SWARM_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Call c;
    if (const int rc = begin(ctx, n, T, out, holders, cap, &c, s)) return rc;
    if (n > 0) {
        BoardArgs a{};
        a.n = n, a.per = c.per, a.T = int32_t(T), a.Ks = state->Ks, a.Kt = state->Kt, a.ids = ids, a.mask = mask;
        a.status = state->status, a.tab_task = state->tab_task, a.tab_winner = state->tab_winner;
        a.tab_util = reinterpret_cast<const uint32_t *>(state->tab_util);
        a.o = c.o;
        const bool vs = state->Ks % 4 == 0 && aligned16(state->status);
        const bool vt = state->Kt % 4 == 0 && aligned16(state->tab_task);
        const dim3 grid(c.blocks), block(kBlock);
        void (*kernel)(const BoardArgs) = vs ? (vt ? k_census_board<4, 4> : k_census_board<4, 1>)
                                             : (vt ? k_census_board<1, 4> : k_census_board<1, 1>);
        hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
        SW_LAUNCHED();
    }
    return finish(c, T, out, n_holders, "swarm_board_census", s);
}

int swarm_tasks_census(swarm_ctx *ctx, int64_t n, const int32_t *ids, int32_t T, const uint64_t *status_lo,
                       const uint64_t *status_hi, const int32_t *tab_winner, const float *tab_util,
                       const uint8_t *mask, const swarm_census *out, int32_t *holders, int64_t cap,
                       int64_t *n_holders, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(out != nullptr, "out is NULL");
    SW_ARG(T >= 0 && T <= 64, "T must be in [0, 64]");
    if (const int rc = check_common(ids, n, out, holders, cap)) return rc;
    SW_ARG(n == 0 || T == 0 || (status_lo && status_hi && tab_winner && tab_util), "NULL task state array");
    if (n_holders) *n_holders = 0;
    if (T == 0) return SWARM_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Call c;
    if (const int rc = begin(ctx, n, T, out, holders, cap, &c, s)) return rc;
    if (n > 0) {
        TasksArgs a{};
        a.n = n, a.per = c.per, a.T = T, a.ids = ids, a.mask = mask;
        a.status_lo = reinterpret_cast<const unsigned long long *>(status_lo);
        a.status_hi = reinterpret_cast<const unsigned long long *>(status_hi);
        a.tab_winner = tab_winner, a.tab_util = reinterpret_cast<const uint32_t *>(tab_util);
        a.o = c.o;
        const dim3 grid(c.blocks), block(kBlock);
        if (T % 4 == 0 && aligned16(tab_winner))
            hipLaunchKernelGGL(k_census_tasks<4>, grid, block, 0, s, a);
        else
            hipLaunchKernelGGL(k_census_tasks<1>, grid, block, 0, s, a);
        SW_LAUNCHED();
    }
    return finish(c, T, out, n_holders, "swarm_tasks_census", s);
}

}  // extern "C"
