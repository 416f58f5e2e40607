// Agent lifetimes (contract U1-J): agents that boot and die during a run.
//
// The reference runs one process per agent (agent.py:349-358): one that starts late is a fresh
// SwarmAgent.__init__ (agent.py:25-54), one that stops simply stops, one that restarts is both.  Here every agent
// carries a window [boot, death) of absolute ticks (agent_life.h).  The handle keeps the sorted events of all
// windows on the host and a copy of their entries on the device; a loop call finds its slice of them by two
// binary searches, and on a tick with events run_ticks queues one launch of k_agent_events over that tick's
// segment, right after the leader kill: the work is proportional to the events, there is no sweep over the
// agents and no host wait.  A tick without events launches nothing.
//   death  alive = 0 in the agent's record, nothing else: what a kill_ticks victim is (what it sent during t-1 is
//          still in the outbox half tick t reads, its position is copied through by the physics step).
//   boot   a fresh SwarmAgent constructed at the clock of tick t-1: FOLLOWER, alive, leader -1, no leader
//          position, last_heartbeat_time (t-1) dt, wait_start = delay = 0, tick counter 1 at tick t
//          (tick_off = 1 - t), velocity 0, no target, both outbox halves empty, and on a task board an empty
//          status row (every task OPEN again), an empty claim table and no claim or conflict in flight.
//          Position, ID and capabilities stay: the robot stands where it stood.
// An agent has at most one event per tick (its window is not empty), so the events of a tick are independent.
// One group of G lanes serves an event: its first lane writes the scalars, all of them clear the rows, each lane
// every G-th slot (coalesced; a slot is rewritten only when it holds something).  G is 1 without task rows, 8 for
// rows of up to 16 slots and a whole wave for wider ones.
#include <new>

#include "fsm_records.h"

namespace swarm {
namespace {

constexpr uint8_t ST_F = SWARM_FOLLOWER;

template <class V>
__device__ __forceinline__ void clear_slots(V *row, int K, int sub, int G, V empty) {
    for (int q = sub; q < K; q += G)
        if (row[q] != empty) row[q] = empty;
}

// f32 slots by their bits (a NaN left by a caller compares unequal to itself, and -0.0f equal to +0.0f)
__device__ __forceinline__ void clear_floats(float *row, int K, int sub, int G) {
    uint32_t *w = reinterpret_cast<uint32_t *>(row);
    for (int q = sub; q < K; q += G)
        if (w[q] != 0u) w[q] = 0u;
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_agent_events(const uint32_t *__restrict__ ev, int64_t count, int64_t t,
                                                         AgentEventArrays a) {
    const int sub = int(threadIdx.x) & (G - 1);
    const int64_t group = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / G;
    const int64_t ngroups = int64_t(gridDim.x) * (kBlock / G);
    const size_t un = size_t(a.n);
    for (int64_t e = group; e < count; e += ngroups) {
        const uint32_t w = ev[e];
        const int64_t i = agent_entry_row(w);
        if (i >= a.n) continue;  // (the host checked every row against n: never taken)
        if (agent_entry_kind(w) == kAgentDies) {
            if (sub == 0) a.rec[i].x &= ~0xFF00u;
            continue;
        }
        if (sub == 0) {
            // the timer as a tick of the run (fsm_records.h): last_hb = double(t - 1) * dt, written by the unpack
            // (kDirty); dt == 0: the f64 arrays hold the timers (kH64)
            const int32_t ph = int32_t((((1 - t) % 10) + 10) % 10);
            const uint32_t bits = a.dt != 0.0 ? kDirty : kH64;
            if (a.dt == 0.0) a.last_hb[i] = double(t - 1) * a.dt;
            a.rec[i] = make_uint2(fw_make(ST_F, 1, bits, ph), uint32_t(int32_t(t - 1 - a.t0)));
            a.lrec[i] = LRec{0.f, 0.f, -1, 0};
            a.wait_start[i] = 0.0;
            a.delay[i] = 0.0;
            a.tick_off[i] = int32_t(1 - t);
            a.outbox[i] = 0;
            a.outbox[un + i] = 0;
            if (a.vel) {
                a.vel[i] = make_double2(0.0, 0.0);
                a.target[i] = make_double2(0.0, 0.0);
                a.has_target[i] = 0;
            }
            if (a.sb) {
                a.sb[i] = 0;
                a.sb[un + i] = 0;
            }
            if (a.T > 0) {
                a.status_lo[i] = 0;
                a.status_hi[i] = 0;
                a.claim_out[i] = 0;
                a.claim_out[un + i] = 0;
                a.conflict_out[i] = 0;
                a.conflict_out[un + i] = 0;
            }
        }
        if (a.T > 0) {
            clear_slots(a.tab_winner + size_t(i) * a.T, a.T, sub, G, int32_t(-1));
            clear_floats(a.tab_util + size_t(i) * a.T, a.T, sub, G);
        }
        if (a.Ks > 0) {  // the sparse board: set_task_board's empty rows
            const size_t ks = size_t(a.Ks), kt = size_t(a.Kt), r = size_t(i);
            clear_slots(a.b_status + r * ks, a.Ks, sub, G, int32_t(-1));
            clear_slots(a.b_claim_out + r * ks, a.Ks, sub, G, int32_t(-1));
            clear_slots(a.b_claim_out + (un + r) * ks, a.Ks, sub, G, int32_t(-1));
            clear_slots(a.b_tab_task + r * kt, a.Kt, sub, G, int32_t(-1));
            clear_slots(a.b_tab_winner + r * kt, a.Kt, sub, G, int32_t(-1));
            clear_floats(a.b_tab_util + r * kt, a.Kt, sub, G);
            clear_slots(a.b_conflict_out + r * kt, a.Kt, sub, G, int32_t(-1));
            clear_slots(a.b_conflict_out + (un + r) * kt, a.Kt, sub, G, int32_t(-1));
        }
    }
}

// The set-time rule on the device: alive = 0 for the listed rows.
__global__ __launch_bounds__(kBlock) void k_agents_down(const uint32_t *__restrict__ rows, int64_t count, int64_t n,
                                                        uint8_t *__restrict__ alive) {
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < count; q += int64_t(gridDim.x) * kBlock)
        if (int64_t(rows[q]) < n) alive[rows[q]] = 0;
}

bool known_life(const swarm_ctx *ctx, const swarm_agent_life *h) {
    for (const swarm_agent_life *q : ctx->lives)
        if (q == h) return true;
    return false;
}

// The handles destroyed last are kept, emptied, on the ctx (the oldest of them deleted): a new handle cannot take
// the address of one that has just died, so a stale handle is told from a live one whatever the allocator does.
constexpr size_t kLifeGraves = 16;

// The windows' checks (nothing is written before they pass).
int check_windows(int64_t n, const int64_t *boot, const int64_t *death) {
    int64_t bad = -1;
    switch (agent_life_check(n, boot, death, &bad)) {
    case kAgentLifeOk:
        return SWARM_OK;
    case kAgentLifeBoot:
        set_error("invalid argument: agent %lld (storage index) boots at tick %lld, outside [0, 2^31)",
                  static_cast<long long>(bad), static_cast<long long>(boot[bad]));
        return SWARM_ERR_ARG;
    default:
        set_error("invalid argument: agent %lld (storage index) dies at a negative tick", static_cast<long long>(bad));
        return SWARM_ERR_ARG;
    }
}

bool same_windows(const swarm_agent_life *h, const int64_t *boot, const int64_t *death) {
    return h->boot.size() == size_t(h->n) && std::equal(h->boot.begin(), h->boot.end(), boot) &&
           std::equal(h->death.begin(), h->death.end(), death);
}

void take_windows(swarm_agent_life *h, const int64_t *boot, const int64_t *death) {
    h->boot.assign(boot, boot + h->n);
    h->death.assign(death, death + h->n);
    h->events = agent_life_events(h->n, boot, death);
    h->entries_host.resize(h->events.size());
    for (size_t q = 0; q < h->events.size(); ++q) h->entries_host[q] = h->events[q].entry;
    h->uploaded = false;
}

}  // namespace

void free_agent_life(swarm_agent_life *h) {
    if (h->entries) (void)hipFree(h->entries);
    delete h;
}

int agent_life_begin(swarm_agent_life *h, int64_t t0, int32_t ticks, AgentSchedule *sched, hipStream_t s) {
    *sched = agent_life_schedule(h->events, t0, ticks);
    if (sched->empty() || h->uploaded) return SWARM_OK;
    const size_t cnt = h->entries_host.size();
    if (h->cap_entries < cnt) {
        // (the old list may still be read by queued work)
        if (h->entries) {
            SW_HIP(hipDeviceSynchronize());
            (void)hipFree(h->entries);
            h->entries = nullptr;
            h->cap_entries = 0;
        }
        SW_HIP(hipMalloc(&h->entries, cnt * sizeof(uint32_t)));
        h->cap_entries = cnt;
    }
    SW_HIP(hipMemcpyAsync(h->entries, h->entries_host.data(), cnt * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    h->uploaded = true;
    return SWARM_OK;
}

int launch_agent_events(const swarm_agent_life *h, const AgentSchedule &sched, int64_t t, const AgentEventArrays &a,
                        hipStream_t s) {
    const int64_t k = t - a.t0 - 1;
    const int64_t count = sched.count(k);
    if (count == 0) return SWARM_OK;
    const uint32_t *ev = h->entries + sched.first + sched.seg[size_t(k)];
    const int width = std::max(int(a.T), std::max(int(a.Ks), int(a.Kt)));
    if (width == 0) {
        hipLaunchKernelGGL(k_agent_events<1>, dim3(grid_for(count, kBlock, 8192)), dim3(kBlock), 0, s, ev, count, t, a);
    } else if (width <= 16) {
        hipLaunchKernelGGL(k_agent_events<8>, dim3(grid_for(count, kBlock / 8, 8192)), dim3(kBlock), 0, s, ev, count, t,
                           a);
    } else {
        hipLaunchKernelGGL(k_agent_events<kWave>, dim3(grid_for(count, kBlock / kWave, 16384)), dim3(kBlock), 0, s, ev,
                           count, t, a);
    }
    SW_LAUNCHED();
    return SWARM_OK;
}

}  // namespace swarm

extern "C" {

int swarm_agent_life_create(swarm_ctx *ctx, int64_t n, const int64_t *boot, const int64_t *death, uint8_t *alive,
                            int32_t *tick_off, swarm_agent_life **out) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && out != nullptr, "ctx or out is NULL");
    *out = nullptr;
    SW_ARG(n >= 0 && n < (int64_t(1) << 31), "n out of range");
    SW_ARG(n == 0 || (boot && death && alive && tick_off), "NULL agent array");
    if (const int rc = check_windows(n, boot, death)) return rc;
    SW_ARG(!find_agent_life(ctx, n, alive), "this alive array already has agent lifetimes (destroy them first)");
    swarm_agent_life *h = new (std::nothrow) swarm_agent_life();
    if (!h) {
        set_error("out of host memory");
        return SWARM_ERR_OOM;
    }
    h->n = n;
    h->alive = alive;
    h->tick_off = tick_off;
    take_windows(h, boot, death);
    ctx->lives.push_back(h);
    *out = h;
    return SWARM_OK;
}

int swarm_agent_life_set(swarm_ctx *ctx, swarm_agent_life *life, int64_t n, const int64_t *boot, const int64_t *death,
                         int64_t last_tick, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && life != nullptr, "ctx or life is NULL");
    SW_ARG(known_life(ctx, life), "the handle is no live agent-lifetime handle of this ctx");
    SW_ARG(n == life->n, "n is not the handle's");
    SW_ARG(n == 0 || (boot && death), "NULL agent array");
    SW_ARG(last_tick >= 0, "last_tick must not be negative");
    if (const int rc = check_windows(n, boot, death)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the set-time rule: the rows that are not up at last_tick, uploaded through the handle's own list buffer
    std::vector<uint32_t> down;
    for (int64_t i = 0; i < n; ++i)
        if (agent_down_when_set(boot[i], death[i], last_tick)) down.push_back(uint32_t(i));
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    // queued work on any stream may still read the old list, and the next loop may upload the new one on another
    SW_HIP(hipDeviceSynchronize());
    if (!down.empty()) {
        uint32_t *d = nullptr;
        SW_HIP(hipMalloc(&d, down.size() * sizeof(uint32_t)));  // (a failure here has written nothing)
        hipError_t e = hipMemcpyAsync(d, down.data(), down.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_agents_down, dim3(grid_for(int64_t(down.size()), kBlock, 4096)), dim3(kBlock), 0, s, d,
                               int64_t(down.size()), n, life->alive);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(d);
        SW_HIP(e);
    }
    // the windows last, once the rule has gone through; windows that are the handle's own (a create followed by a
    // set of the same arrays) keep their sorted events
    if (!same_windows(life, boot, death)) take_windows(life, boot, death);
    return SWARM_OK;
}

int swarm_agent_life_events(swarm_ctx *ctx, const swarm_agent_life *life, int64_t t0, int32_t ticks, int64_t *events) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && life != nullptr, "ctx or life is NULL");
    SW_ARG(known_life(ctx, life), "the handle is no live agent-lifetime handle of this ctx");
    SW_ARG(t0 >= 0 && ticks >= 0, "t0 / ticks must not be negative");
    SW_ARG(ticks == 0 || events != nullptr, "events is NULL");
    const AgentSchedule sched = agent_life_schedule(life->events, t0, ticks);
    for (int64_t k = 0; k < ticks; ++k) {
        events[2 * k] = int64_t(sched.count(k)) - int64_t(sched.deaths(k));
        events[2 * k + 1] = int64_t(sched.deaths(k));
    }
    return SWARM_OK;
}

int swarm_agent_life_destroy(swarm_ctx *ctx, swarm_agent_life *life) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    if (!life) return SWARM_OK;
    SW_ARG(known_life(ctx, life), "the handle is no live agent-lifetime handle of this ctx");
    if (life->entries) {
        (void)hipDeviceSynchronize();  // the list may still be read by queued work
        (void)hipFree(life->entries);
    }
    life->entries = nullptr;
    life->cap_entries = 0;
    life->uploaded = false;
    life->dead = true;
    life->alive = nullptr;
    life->tick_off = nullptr;
    std::vector<int64_t>().swap(life->boot);
    std::vector<int64_t>().swap(life->death);
    std::vector<AgentEvent>().swap(life->events);
    std::vector<uint32_t>().swap(life->entries_host);
    ctx->lives.erase(std::find(ctx->lives.begin(), ctx->lives.end(), life));
    auto &g = ctx->life_graves;
    try {
        g.push_back(life);
    } catch (const std::bad_alloc &) {
        delete life;
        return SWARM_OK;
    }
    if (g.size() > kLifeGraves) {
        delete g.front();
        g.erase(g.begin());
    }
    return SWARM_OK;
}

}  // extern "C"
