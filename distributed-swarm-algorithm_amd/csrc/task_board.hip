// Task boards (contract U1-B): the host side.  The grid and the cell lists are built by task_grid.h
// from a host copy of the caller's board -- once per board, one host wait, not the hot path -- and uploaded as
// a cell-sorted copy of (x, y, treq, index); protocol.hip's board kernels read them.  A moving board (contract
// U1-M) rebuilds that copy on the device before every tick, with no host wait (below).
#include <cmath>
#include <cstring>
#include <new>

#include "binning.h"
#include "swarm_common.h"
#include "task_grid.h"
#include "task_life.h"
#include "task_motion.h"
#include "task_place.h"
#include "utility.h"

namespace swarm {

namespace {

// Frees everything a board owns; the struct itself stays, an empty board.
void release_board(swarm_board *b) {
    void *const dev[] = {b->tpos,    b->treq,    b->cell_off, b->sxy,     b->sir,     b->verdict, b->lag,    b->vel,
                         b->entry,   b->box,     b->keys[0],  b->keys[1], b->vals[0], b->vals[1], b->dyn_off, b->cub_tmp,
                         b->life_open, b->life_close, b->present, b->place_buf, b->placed, b->purge_part};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    if (b->verdict_host) (void)hipHostFree(b->verdict_host);
    *b = swarm_board();
}

constexpr size_t kBoardGraves = 16;

// A destroyed board: what it owned is freed, the struct is kept on the ctx's list of the last few that died (the
// oldest of them deleted), so that its address is not handed to the next board.
void bury_board(swarm_ctx *ctx, swarm_board *b) {
    release_board(b);
    auto &g = ctx->board_graves;
    try {
        g.push_back(b);
    } catch (const std::bad_alloc &) {
        delete b;
        return;
    }
    if (g.size() > kBoardGraves) {
        delete g.front();
        g.erase(g.begin());
    }
}

}  // namespace

void free_board(swarm_board *b) {
    if (!b) return;
    release_board(b);
    delete b;
}

namespace {

// The rest of swarm_board_create once the lists are built: on any error the caller frees b.
int upload_board(swarm_board *b, const std::vector<double> &h_pos, const std::vector<int8_t> &h_req,
                 const TaskCells &tc, hipStream_t s) {
    const size_t T = size_t(tc.T);
    std::vector<double> sxy;
    std::vector<int32_t> sir;
    try {
        sxy.resize(T * 2);
        sir.resize(T * 2);
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for %zu cell-sorted tasks", T);
        return SWARM_ERR_OOM;
    }
    for (size_t q = 0; q < T; ++q) {
        const size_t k = size_t(tc.idx[q]);
        sxy[2 * q] = h_pos[2 * k], sxy[2 * q + 1] = h_pos[2 * k + 1];
        sir[2 * q] = int32_t(k), sir[2 * q + 1] = int32_t(h_req[k]);
    }
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->tpos), (T ? T : 1) * 16));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->treq), T ? T : 1));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->cell_off), tc.cell_off.size() * 4));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->sxy), (T ? T : 1) * 16));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->sir), (T ? T : 1) * 8));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->verdict), 64));
    SW_HIP(hipHostMalloc(reinterpret_cast<void **>(&b->verdict_host), 64, hipHostMallocDefault));
    SW_HIP(hipMemcpyAsync(b->cell_off, tc.cell_off.data(), tc.cell_off.size() * 4, hipMemcpyHostToDevice, s));
    if (T) {
        SW_HIP(hipMemcpyAsync(b->tpos, h_pos.data(), T * 16, hipMemcpyHostToDevice, s));
        SW_HIP(hipMemcpyAsync(b->treq, h_req.data(), T, hipMemcpyHostToDevice, s));
        SW_HIP(hipMemcpyAsync(b->sxy, sxy.data(), T * 16, hipMemcpyHostToDevice, s));
        SW_HIP(hipMemcpyAsync(b->sir, sir.data(), T * 8, hipMemcpyHostToDevice, s));
    }
    SW_HIP(hipStreamSynchronize(s));  // the host vectors above end with this call
    return SWARM_OK;
}

swarm_board_desc describe(const swarm_board &b) {
    return swarm_board_desc{b.T, b.g.ncx, b.g.ncy, b.g.cell, b.g.xmin, b.g.ymin, b.longest};
}

// ---- moving boards (contract U1-M): the cell-sorted copy built on the device, every tick ----
//
// The builder is build_task_cells on the device: the tasks' cell keys on the call's grid (binning.h's k_cell_keys:
// cell_coord's arithmetic, which task_cell_coord restates), a stable radix sort of (key, task index) -- a cell's
// tasks keep ascending task index, the host builder's list -- the offsets by search, and one gather that writes
// the 16-byte (x, y) rows and the 8-byte (index, treq) rows in sorted order.  No atomics: the same lists on every
// run.  Every index that addresses memory comes from the sort's values, 0 .. T - 1 by construction (the gather
// checks it all the same).

constexpr unsigned kBoxParts = 1024;  // workgroups of the span-box reduction, at most

// The box of every task's span over the call (task_motion.h, the same functions): per workgroup four doubles.
__global__ __launch_bounds__(kBlock) void k_task_span_box(int64_t T, const double2 *__restrict__ cur,
                                                         const double2 *__restrict__ vel, double dt, int32_t ticks,
                                                         double *__restrict__ part) {
    TaskBox b{kBoxEmptyLo, kBoxEmptyLo, kBoxEmptyHi, kBoxEmptyHi};
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < T; k += int64_t(gridDim.x) * kBlock) {
        const double2 p = cur[k], v = vel[k];
        task_box_add(&b, p.x, p.y, v.x, v.y, dt, ticks);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        b.xmin = fmin(b.xmin, __shfl_xor(b.xmin, off, 64));
        b.ymin = fmin(b.ymin, __shfl_xor(b.ymin, off, 64));
        b.xmax = fmax(b.xmax, __shfl_xor(b.xmax, off, 64));
        b.ymax = fmax(b.ymax, __shfl_xor(b.ymax, off, 64));
    }
    __shared__ double s[4][kBlock / kWave];
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s[0][wid] = b.xmin; s[1][wid] = b.ymin; s[2][wid] = b.xmax; s[3][wid] = b.ymax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / kWave; ++w) {
            s[0][0] = fmin(s[0][0], s[0][w]); s[1][0] = fmin(s[1][0], s[1][w]);
            s[2][0] = fmax(s[2][0], s[2][w]); s[3][0] = fmax(s[3][0], s[3][w]);
        }
        part[4 * blockIdx.x + 0] = s[0][0]; part[4 * blockIdx.x + 1] = s[1][0];
        part[4 * blockIdx.x + 2] = s[2][0]; part[4 * blockIdx.x + 3] = s[3][0];
    }
}

// The cell-sorted copy: row q is task svals[q].  Loads gather, stores are coalesced 16- and 8-byte rows.
__global__ __launch_bounds__(kBlock) void k_task_gather(int64_t T, const int32_t *__restrict__ svals,
                                                       const double2 *__restrict__ cur,
                                                       const int8_t *__restrict__ treq, double2 *__restrict__ sxy,
                                                       int2 *__restrict__ sir) {
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < T; q += int64_t(gridDim.x) * kBlock) {
        const int32_t k = svals[q];
        if (k < 0 || k >= T) continue;
        sxy[q] = cur[k];
        sir[q] = make_int2(k, int(treq[k]));
    }
}

// The contract's advance, one pass: lag <- cur, cur <- fl(cur + fl(v * dt)) per coordinate (-ffp-contract=off:
// two roundings).  Nothing once the run's stop word is set.
__global__ __launch_bounds__(kBlock) void k_task_advance(const unsigned long long *__restrict__ st, int64_t T,
                                                        double2 *__restrict__ cur, double2 *__restrict__ lag,
                                                        const double2 *__restrict__ vel, double dt) {
    if (st[0] != 0) return;  // uniform over the grid: written by an earlier kernel of the stream
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < T; k += int64_t(gridDim.x) * kBlock) {
        const double2 p = cur[k], v = vel[k];
        lag[k] = p;
        cur[k] = make_double2(task_advance(p.x, v.x, dt), task_advance(p.y, v.y, dt));
    }
}

// Both lists back to their entry bytes when a tick of the loop was refused (obstacle_field.hip's k_obs_restore).
__global__ __launch_bounds__(kBlock) void k_task_restore(const unsigned long long *__restrict__ st, int64_t T,
                                                        double2 *__restrict__ cur, double2 *__restrict__ lag,
                                                        const double2 *__restrict__ entry) {
    if (st[0] == 0) return;
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < T; k += int64_t(gridDim.x) * kBlock) {
        cur[k] = entry[k];
        lag[k] = entry[T + k];
    }
}

// ---- lifetimes (contract U1-A) ----
//
// k_cell_keys with the presence predicate (task_life.h): a task absent at tick t takes the key `ncells`, one past
// the last cell, so the stable sort puts it behind every cell's run and the offsets search -- off[ncells] is the
// first sorted position whose key is >= ncells -- leaves it in no run: the tick's kernels are never offered it.
// The same pass writes the tick's presence bytes, which the retire pass and the conflict walk read.
__global__ __launch_bounds__(kBlock) void k_cell_keys_life(const double2 *__restrict__ pos, int64_t T, Grid g,
                                                          const int64_t *__restrict__ open,
                                                          const int64_t *__restrict__ close, int64_t t,
                                                          uint32_t *__restrict__ keys, int32_t *__restrict__ vals,
                                                          uint8_t *__restrict__ present) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < T; i += int64_t(gridDim.x) * kBlock) {
        const double2 p = pos[i];
        const int64_t cx = cell_coord(p.x, g.xmin, g.inv_cell, g.ncx);
        const int64_t cy = cell_coord(p.y, g.ymin, g.inv_cell, g.ncy);
        const bool in = task_present(open[i], close[i], t);
        keys[i] = uint32_t(in ? cy * g.ncx + cx : g.ncx * g.ncy);
        vals[i] = int32_t(i);
        present[i] = uint8_t(in);
    }
}

// The retire pass (contract U1-A.7): the status entries whose task is absent this tick leave their rows, the
// entries behind them move down, the freed slots become -1 -- a canonical row again.  2^lg lanes share a row (the
// least power of two that holds Ks, 64 at most), so a wave takes 64 >> lg rows at once and its loads are
// consecutive 4-byte words; a longer row is walked in chunks of 64 and left at the first chunk that is not full
// (the fillers are behind the entries).  The ranks come from one ballot per chunk.  In place: a chunk's stores go
// to slots at or below the slots it has loaded, all loaded before the ballot that ranks them.  A lane stores only
// where the slot's value changes, so a row that loses nothing is not written.  Nothing once the stop word is set.
// Rows of at most 64 slots -- one chunk -- are taken kRetireTurn groups a turn, every group's loads issued before
// the first ballot: with one 256-byte load in flight per wave the pass ran at 29 % of the copy rate.
constexpr int kRetireTurn = 4;

__global__ __launch_bounds__(kBlock) void k_board_retire(const unsigned long long *__restrict__ st, int64_t n,
                                                        int32_t Ks, int32_t lg, int32_t T,
                                                        const uint8_t *__restrict__ present,
                                                        int32_t *__restrict__ status) {
    if (st[0] != 0) return;  // uniform over the grid: written by an earlier kernel of the stream
    const int L = 1 << lg, lane = threadIdx.x & (kWave - 1), sub = lane >> lg, lig = lane & (L - 1);
    const int64_t per = kWave >> lg;  // rows per wave
    const int64_t wave = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6, nwaves = int64_t(gridDim.x) * (kBlock >> 6);
    const uint64_t gm = lg == 6 ? ~0ull : ((1ull << L) - 1) << (sub * L);  // the lanes of this lane's row
    const uint64_t below = gm & ((1ull << lane) - 1);
    if (Ks <= kWave) {  // one chunk per row: kRetireTurn row groups a turn, all of them loaded before the first is ranked
        const int64_t step = nwaves * per;
        for (int64_t r0 = wave * per; r0 < n; r0 += kRetireTurn * step) {  // (uniform over the wave)
            int32_t e[kRetireTurn];
            bool keep[kRetireTurn];
#pragma unroll
            for (int u = 0; u < kRetireTurn; ++u) {
                const int64_t row = r0 + u * step + sub;
                e[u] = row < n && lig < Ks ? status[row * Ks + lig] : -1;
            }
#pragma unroll
            for (int u = 0; u < kRetireTurn; ++u) keep[u] = e[u] >= 0 && (e[u] >> 2) < T && present[e[u] >> 2] != 0;
#pragma unroll
            for (int u = 0; u < kRetireTurn; ++u) {
                const uint64_t mk = __ballot(keep[u]), mv = __ballot(e[u] >= 0);
                if (mk == mv) continue;  // (uniform) no row of the group loses anything
                const int at = __popcll(mk & below), kept = __popcll(mk & gm), seen = __popcll(mv & gm);
                const int64_t base = (r0 + u * step + sub) * Ks;  // (a lane that stores holds an entry: its row exists)
                if (keep[u] && at != lig) status[base + at] = e[u];
                if (lig >= kept && lig < seen) status[base + lig] = -1;
            }
        }
        return;
    }
    for (int64_t r0 = wave * per; r0 < n; r0 += nwaves * per) {  // (uniform over the wave)
        const int64_t row = r0 + sub;
        const bool live = row < n;
        int32_t *rp = status + (live ? row : 0) * Ks;
        int kept = 0, seen = 0;
        for (int c = 0; c < Ks; c += L) {
            const int idx = c + lig;
            const int32_t e = live && idx < Ks ? rp[idx] : -1;
            const bool valid = e >= 0;
            const bool keep = valid && (e >> 2) < T && present[e >> 2] != 0;
            const uint64_t mk = __ballot(keep), mv = __ballot(valid);
            const int at = kept + __popcll(mk & below);
            if (keep && at != idx) rp[at] = e;
            kept += __popcll(mk & gm);
            const int nv = __popcll(mv & gm);
            seen += nv;
            if (lg == 6 && nv < kWave) break;  // one row per wave: uniform
        }
        for (int q = kept + lig; q < seen; q += L) rp[q] = -1;
    }
}

// ---- placing (contract U1-P) ----
//
// One place's requests in the board's staging buffer, m of each: 16-byte sections first, so that every section is
// aligned to its element.
struct PlaceReq {
    double2 *pos, *vel;
    int64_t *open, *close, *old_open, *old_close;
    int32_t *idx;
    int8_t *req;
};
constexpr size_t kPlaceBytes = 16 + 16 + 8 + 8 + 8 + 8 + 4 + 1;  // per request

PlaceReq place_sections(void *buf, size_t m) {
    char *p = static_cast<char *>(buf);
    PlaceReq r;
    r.pos = reinterpret_cast<double2 *>(p), r.vel = reinterpret_cast<double2 *>(p + 16 * m);
    r.open = reinterpret_cast<int64_t *>(p + 32 * m), r.close = reinterpret_cast<int64_t *>(p + 40 * m);
    r.old_open = reinterpret_cast<int64_t *>(p + 48 * m), r.old_close = reinterpret_cast<int64_t *>(p + 56 * m);
    r.idx = reinterpret_cast<int32_t *>(p + 64 * m), r.req = reinterpret_cast<int8_t *>(p + 68 * m);
    return r;
}

// The current windows of the m listed slots, for the host's eligibility check: m entries, not T.  A request that
// names no slot reads nothing (the host refuses it by its index alone).
__global__ __launch_bounds__(kBlock) void k_board_place_fetch(int64_t m, int64_t T, PlaceReq r,
                                                             const int64_t *__restrict__ open,
                                                             const int64_t *__restrict__ close) {
    for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < m; j += int64_t(gridDim.x) * kBlock) {
        const int32_t k = r.idx[j];
        const bool in = k >= 0 && k < T;
        r.old_open[j] = in ? open[k] : 0;
        r.old_close[j] = in ? close[k] : 0;
    }
}

// The scatter of m checked requests (no slot twice): cur = lag = the new position, the requirement, the velocity,
// the window; placed[k] = 1 for the purge pass (NULL: the tables are kept).
__global__ __launch_bounds__(kBlock) void k_board_place(int64_t m, int64_t T, PlaceReq r, double2 *__restrict__ cur,
                                                       double2 *__restrict__ lag, double2 *__restrict__ vel,
                                                       int8_t *__restrict__ treq, int64_t *__restrict__ open,
                                                       int64_t *__restrict__ close, uint8_t *__restrict__ placed) {
    for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < m; j += int64_t(gridDim.x) * kBlock) {
        const int32_t k = r.idx[j];
        if (k < 0 || k >= T) continue;  // (refused on the host before this launch)
        cur[k] = lag[k] = r.pos[j];
        vel[k] = r.vel[j];
        treq[k] = r.req[j];
        open[k] = r.open[j];
        close[k] = r.close[j];
        if (placed) placed[k] = 1;
    }
}

// The purge pass (contract U1-P.3): every claim-table entry about a placed slot leaves its row, the entries behind
// it move down, the freed slots become (-1, -1, 0) -- a canonical row again.  k_board_retire's scheme over the
// table's task words: 2^lg lanes per row, consecutive 4-byte loads, one ballot per 64 slots ranks the keepers, rows
// of at most 64 slots kRetireTurn groups a turn with every load issued before the first ballot, longer rows in
// chunks of 64 and left at the first chunk that is not full.  A row that loses nothing reads its task words only
// and writes nothing; the winner and utility words are read, and moved with their task, only from the first chunk
// that loses an entry on.  In place: a chunk's stores go to slots at or below the slots it has loaded.  An entry
// outside [0, T) is kept (the loop's entry check owns that verdict).  part[wave]: the entries the wave removed.
__global__ __launch_bounds__(kBlock) void k_board_purge(int64_t n, int32_t Kt, int32_t lg, int32_t T,
                                                       const uint8_t *__restrict__ placed, int32_t *tab_task,
                                                       int32_t *tab_winner, int32_t *tab_util,
                                                       unsigned long long *__restrict__ part) {
    const int L = 1 << lg, lane = threadIdx.x & (kWave - 1), sub = lane >> lg, lig = lane & (L - 1);
    const int64_t per = kWave >> lg;  // rows per wave
    const int64_t wave = (int64_t(blockIdx.x) * kBlock + threadIdx.x) >> 6, nwaves = int64_t(gridDim.x) * (kBlock >> 6);
    const uint64_t gm = lg == 6 ? ~0ull : ((1ull << L) - 1) << (sub * L);  // the lanes of this lane's row
    const uint64_t below = gm & ((1ull << lane) - 1);
    unsigned long long removed = 0;  // (counted by the first lane of each row)
    if (Kt <= kWave) {
        const int64_t step = nwaves * per;
        for (int64_t r0 = wave * per; r0 < n; r0 += kRetireTurn * step) {  // (uniform over the wave)
            int32_t e[kRetireTurn];
            bool keep[kRetireTurn];
#pragma unroll
            for (int u = 0; u < kRetireTurn; ++u) {
                const int64_t row = r0 + u * step + sub;
                e[u] = row < n && lig < Kt ? tab_task[row * Kt + lig] : -1;
            }
#pragma unroll
            for (int u = 0; u < kRetireTurn; ++u) keep[u] = e[u] >= 0 && !(e[u] < T && placed[e[u]] != 0);
            uint64_t mk[kRetireTurn], mv[kRetireTurn];
#pragma unroll
            for (int u = 0; u < kRetireTurn; ++u) mk[u] = __ballot(keep[u]), mv[u] = __ballot(e[u] >= 0);
#pragma unroll
            for (int u = 0; u < kRetireTurn; ++u) {  // (no ballot below: the rows of a group part ways here)
                if (mk[u] == mv[u]) continue;  // (uniform) no row of the group loses anything
                const int at = __popcll(mk[u] & below), kept = __popcll(mk[u] & gm), seen = __popcll(mv[u] & gm);
                if (kept != seen) {  // this lane's row loses an entry (seen > 0: the row exists)
                    const int64_t base = (r0 + u * step + sub) * Kt;
                    int32_t w = -1, f = 0;
                    if (e[u] >= 0) w = tab_winner[base + lig], f = tab_util[base + lig];
                    if (keep[u] && at != lig)
                        tab_task[base + at] = e[u], tab_winner[base + at] = w, tab_util[base + at] = f;
                    if (lig >= kept && lig < seen)
                        tab_task[base + lig] = -1, tab_winner[base + lig] = -1, tab_util[base + lig] = 0;
                    if (lig == 0) removed += unsigned(seen - kept);
                }
            }
        }
    } else {  // lg == 6: one row per wave
        for (int64_t row = wave; row < n; row += nwaves) {  // (uniform over the wave)
            const int64_t base = row * Kt;
            int kept = 0, seen = 0;
            for (int c = 0; c < Kt; c += kWave) {
                const int idx = c + lane;
                const int32_t e = idx < Kt ? tab_task[base + idx] : -1;
                const bool valid = e >= 0;
                const bool keep = valid && !(e < T && placed[e] != 0);
                const uint64_t mk = __ballot(keep), mv = __ballot(valid);
                const int at = kept + __popcll(mk & below);
                kept += __popcll(mk);
                const int nv = __popcll(mv);
                seen += nv;
                if (kept != seen) {  // (uniform) an entry has left at or before this chunk: the three words move
                    int32_t w = -1, f = 0;
                    if (valid) w = tab_winner[base + idx], f = tab_util[base + idx];
                    if (keep && at != idx) tab_task[base + at] = e, tab_winner[base + at] = w, tab_util[base + at] = f;
                }
                if (nv < kWave) break;  // (uniform) the fillers are behind the entries
            }
            for (int q = kept + lane; q < seen; q += kWave) tab_task[base + q] = -1, tab_winner[base + q] = -1, tab_util[base + q] = 0;
            if (lane == 0) removed += unsigned(seen - kept);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) removed += __shfl_xor(removed, off, 64);
    if (lane == 0) part[wave] = removed;
}

// Behind the purge: the mask back to zero (m stores, not T) and the waves' counts summed into out[0] by the first
// workgroup.
__global__ __launch_bounds__(kBlock) void k_board_place_done(int64_t m, int64_t T, const int32_t *__restrict__ idx,
                                                            uint8_t *__restrict__ placed, int64_t nparts,
                                                            const unsigned long long *__restrict__ part,
                                                            unsigned long long *__restrict__ out) {
    for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < m; j += int64_t(gridDim.x) * kBlock) {
        const int32_t k = idx[j];
        if (k >= 0 && k < T) placed[k] = 0;
    }
    if (blockIdx.x != 0) return;
    unsigned long long sum = 0;
    for (int64_t q = threadIdx.x; q < nparts; q += kBlock) sum += part[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    __shared__ unsigned long long s[kBlock / kWave];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = s[0] + s[1] + s[2] + s[3];
}

int sort_end_bit(int64_t ncells) {
    int b = 1;
    while (b < 32 && (int64_t(1) << b) < ncells) ++b;
    return b;
}

// p <- a device buffer of at least `bytes`, *have its size: grown by a new allocation (hipFree waits for the
// device: no queued work reads the old one).
int grow(void **p, size_t *have, size_t bytes) {
    if (*p && *have >= bytes) return SWARM_OK;
    bytes = bytes < 64 ? 64 : bytes;
    if (*p) SW_HIP(hipFree(*p));
    *p = nullptr, *have = 0;
    if (hipMalloc(p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        set_error("out of device memory for %zu bytes of a moving task board", bytes);
        return SWARM_ERR_OOM;
    }
    *have = bytes;
    return SWARM_OK;
}

// The board's buffers for a grid of `ncells` cells.
int size_buffers(swarm_board *b, int64_t ncells, hipStream_t s) {
    size_t off_bytes = b->cap_cells * 4;
    void *off = b->dyn_off;
    int rc = grow(&off, &off_bytes, (size_t(ncells) + 1) * 4);
    b->dyn_off = static_cast<uint32_t *>(off), b->cap_cells = off_bytes / 4;
    if (rc) return rc;
    size_t sort_bytes = 0;
    if (b->T)
        SW_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, b->keys[0], b->keys[1], b->vals[0], b->vals[1],
                                                  int(b->T), 0, sort_end_bit(ncells + 1), s));
    return grow(&b->cub_tmp, &b->cap_tmp, sort_bytes);
}

// The cell-sorted copy of `cur` on grid g, queued on s (size_buffers has run for g's cell count).  tick (NULL:
// every task): the tick whose present tasks the lists hold, on a board with lifetimes (contract U1-A) -- the sort
// then covers the key of the absent, `ncells`.
int build_lists(swarm_board *b, const Grid &g, const int64_t *tick, hipStream_t s) {
    const int64_t T = b->T, ncells = g.ncx * g.ncy;
    const bool life = tick && b->alive();
    if (T) {
        if (life)
            hipLaunchKernelGGL(k_cell_keys_life, dim3(grid_for(T, kBlock, 8192)), dim3(kBlock), 0, s,
                               reinterpret_cast<const double2 *>(b->tpos), T, g, b->life_open, b->life_close, *tick,
                               b->keys[0], b->vals[0], b->present);
        else
            hipLaunchKernelGGL(k_cell_keys, dim3(grid_for(T, kBlock, 8192)), dim3(kBlock), 0, s,
                               reinterpret_cast<const double2 *>(b->tpos), T, g, b->keys[0], b->vals[0]);
        SW_LAUNCHED();
        size_t tmp = b->cap_tmp;
        SW_HIP(hipcub::DeviceRadixSort::SortPairs(b->cub_tmp, tmp, b->keys[0], b->keys[1], b->vals[0], b->vals[1],
                                                  int(T), 0, sort_end_bit(ncells + (life ? 1 : 0)), s));
    }
    hipLaunchKernelGGL(k_cell_offsets_search, dim3(grid_for(ncells + 1, kBlock, 8192)), dim3(kBlock), 0, s, b->keys[1],
                       T, ncells, b->dyn_off);
    SW_LAUNCHED();
    if (T) {
        hipLaunchKernelGGL(k_task_gather, dim3(grid_for(T, kBlock, 8192)), dim3(kBlock), 0, s, T, b->vals[1],
                           reinterpret_cast<const double2 *>(b->tpos), b->treq, reinterpret_cast<double2 *>(b->sxy),
                           reinterpret_cast<int2 *>(b->sir));
        SW_LAUNCHED();
    }
    return SWARM_OK;
}

int motion_error(TaskMotionStatus st) {
    switch (st) {
    case kTaskMotionOk:
        return SWARM_OK;
    case kTaskMotionNonFinite:
        set_error("invalid argument: a task position or velocity is not finite");
        return SWARM_ERR_ARG;
    default:
        set_error("invalid argument: the moving tasks' positions have no finite extent over the call");
        return SWARM_ERR_ARG;
    }
}

// The device velocities (NULL: zero) to the host, refused unless finite.
int fetch_velocities(int64_t T, const double *velocities, std::vector<double> *out, hipStream_t s) {
    try {
        out->assign(size_t(T) * 2, 0.0);
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for %lld velocities", static_cast<long long>(T));
        return SWARM_ERR_OOM;
    }
    if (T && velocities) {
        SW_HIP(hipMemcpyAsync(out->data(), velocities, size_t(T) * 16, hipMemcpyDeviceToHost, s));
        SW_HIP(hipStreamSynchronize(s));
    }
    SW_ARG(task_velocities_finite(T, out->data()), "a velocity is not finite");
    return SWARM_OK;
}

// What a moving board owns beyond a static one (on any error the caller frees b).
int make_moving(swarm_board *b, const std::vector<double> &h_vel, hipStream_t s) {
    const size_t T = size_t(b->T), rows = T ? T : 1;
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->lag), rows * 16));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->vel), rows * 16));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->entry), rows * 32));
    SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->box), (size_t(kBoxParts) + 1) * 32));
    for (int q = 0; q < 2; ++q) {
        SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->keys[q]), rows * 4));
        SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->vals[q]), rows * 4));
    }
    if (T) {
        SW_HIP(hipMemcpyAsync(b->lag, b->tpos, T * 16, hipMemcpyDeviceToDevice, s));  // at creation lag = cur
        SW_HIP(hipMemcpyAsync(b->vel, h_vel.data(), T * 16, hipMemcpyHostToDevice, s));
    }
    SW_HIP(hipStreamSynchronize(s));
    b->moving = true;
    b->call_g = b->g;
    return size_buffers(b, b->g.ncx * b->g.ncy, s);
}

// The span-box reduction of the list as it stands, its four doubles at b->box + 4 kBoxParts.
int launch_span_box(swarm_board *b, double dt, int32_t ticks, hipStream_t s) {
    const unsigned np = grid_for(b->T, kBlock, kBoxParts);
    hipLaunchKernelGGL(k_task_span_box, dim3(np), dim3(kBlock), 0, s, b->T, reinterpret_cast<const double2 *>(b->tpos),
                       reinterpret_cast<const double2 *>(b->vel), dt, ticks, b->box);
    SW_LAUNCHED();
    hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(64), 0, s, b->box, int(np), b->box + 4 * size_t(kBoxParts));
    SW_LAUNCHED();
    return SWARM_OK;
}

}  // namespace

int moving_board_box(swarm_board *b, double dt, int32_t ticks, hipStream_t s) {
    if (const int rc = launch_span_box(b, dt, ticks, s)) return rc;
    double *h = reinterpret_cast<double *>(b->verdict_host + 1);
    h[2] = HUGE_VAL;  // (overwritten by the copy: a wait that never came reads as a refusal)
    SW_HIP(hipMemcpyAsync(h, b->box + 4 * size_t(kBoxParts), 32, hipMemcpyDeviceToHost, s));
    return SWARM_OK;
}

int moving_board_begin(swarm_board *b, hipStream_t s) {
    const double *h = reinterpret_cast<const double *>(b->verdict_host + 1);
    Grid g{};
    int rc;
    if ((rc = motion_error(task_grid_of_box(b->T, TaskBox{h[0], h[1], h[2], h[3]}, &g)))) return rc;
    if ((rc = size_buffers(b, g.ncx * g.ncy, s))) return rc;
    b->call_g = g;
    const size_t T = size_t(b->T);
    SW_HIP(hipMemcpyAsync(b->entry, b->tpos, T * 16, hipMemcpyDeviceToDevice, s));
    SW_HIP(hipMemcpyAsync(b->entry + 2 * T, b->lag, T * 16, hipMemcpyDeviceToDevice, s));
    return SWARM_OK;
}

int moving_board_tick(swarm_board *b, int64_t t, hipStream_t s) { return build_lists(b, b->call_g, &t, s); }

bool moving_board_retires(const swarm_board *b, int64_t t0, int64_t t) {
    return b->alive() && task_tick_retires(b->close_ticks, b->life_fresh && t == t0 + 1, t);
}

int moving_board_retire(const swarm_board *b, const unsigned long long *st, int64_t n, int32_t Ks, int32_t *status,
                        hipStream_t s) {
    int lg = 0;
    while (lg < 6 && (1 << lg) < Ks) ++lg;
    int64_t waves = (n + (kWave >> lg) - 1) / (kWave >> lg);
    if (Ks <= kWave) waves = (waves + kRetireTurn - 1) / kRetireTurn;
    hipLaunchKernelGGL(k_board_retire, dim3(grid_for(waves * kWave, kBlock, 16384)), dim3(kBlock), 0, s, st, n, Ks, lg,
                       int32_t(b->T), b->present, status);
    SW_LAUNCHED();
    return SWARM_OK;
}

int moving_board_advance(swarm_board *b, const unsigned long long *st, double dt, hipStream_t s) {
    hipLaunchKernelGGL(k_task_advance, dim3(grid_for(b->T, kBlock, 4096)), dim3(kBlock), 0, s, st, b->T,
                       reinterpret_cast<double2 *>(b->tpos), reinterpret_cast<double2 *>(b->lag),
                       reinterpret_cast<const double2 *>(b->vel), dt);
    SW_LAUNCHED();
    return SWARM_OK;
}

int moving_board_restore_if_refused(swarm_board *b, const unsigned long long *st, hipStream_t s) {
    hipLaunchKernelGGL(k_task_restore, dim3(grid_for(b->T, kBlock, 4096)), dim3(kBlock), 0, s, st, b->T,
                       reinterpret_cast<double2 *>(b->tpos), reinterpret_cast<double2 *>(b->lag),
                       reinterpret_cast<const double2 *>(b->entry));
    SW_LAUNCHED();
    return SWARM_OK;
}

}  // namespace swarm

// swarm_board_create (moving false) and swarm_board_create_moving.
static int create_board(swarm_ctx *ctx, int64_t T, const double *tpos, const int8_t *treq, bool moving,
                        const double *velocities, swarm_board **out, swarm_board_desc *info, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && out != nullptr, "ctx or out is NULL");
    SW_ARG(T >= 0 && T <= kMaxBoardTasks, "T must be in [0, 2^24]");
    SW_ARG(T == 0 || (tpos != nullptr && treq != nullptr), "NULL task array");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<double> h_pos;
    std::vector<int8_t> h_req;
    TaskCells tc;
    try {
        h_pos.resize(size_t(T) * 2);
        h_req.resize(size_t(T));
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for a board of %lld tasks", static_cast<long long>(T));
        return SWARM_ERR_OOM;
    }
    if (T) {
        SW_HIP(hipMemcpyAsync(h_pos.data(), tpos, size_t(T) * 16, hipMemcpyDeviceToHost, s));
        SW_HIP(hipMemcpyAsync(h_req.data(), treq, size_t(T), hipMemcpyDeviceToHost, s));
        SW_HIP(hipStreamSynchronize(s));
    }
    for (int64_t k = 0; k < T; ++k) SW_ARG(!bad_req(h_req[size_t(k)]), "a treq outside [-1, 31]");
    switch (build_task_cells(T, h_pos.data(), &tc)) {
    case kTaskCellsOk:
        break;
    case kTaskCellsNonFinite:
        SW_ARG(false, "task positions must be finite");
    case kTaskCellsExtent:
        set_error("invalid argument: %s", kExtentError);
        return SWARM_ERR_ARG;
    default:
        set_error("out of host memory for the board's cell lists");
        return SWARM_ERR_OOM;
    }
    std::vector<double> h_vel;
    if (moving)  // its own refusal, before anything is created
        if (const int rc = fetch_velocities(T, velocities, &h_vel, s)) return rc;
    swarm_board *b = new (std::nothrow) swarm_board();
    if (!b) {
        set_error("out of host memory");
        return SWARM_ERR_OOM;
    }
    b->T = T;
    b->g = tc.g;
    b->longest = tc.longest;
    int rc = upload_board(b, h_pos, h_req, tc, s);
    if (!rc && moving) rc = make_moving(b, h_vel, s);
    if (rc) {
        free_board(b);
        return rc;
    }
    b->cell_off_host = std::move(tc.cell_off);
    b->idx_host = std::move(tc.idx);
    try {
        ctx->boards.push_back(b);
    } catch (const std::bad_alloc &) {
        free_board(b);
        set_error("out of host memory");
        return SWARM_ERR_OOM;
    }
    if (info) *info = describe(*b);
    *out = b;
    return SWARM_OK;
}

extern "C" {

int swarm_board_create(swarm_ctx *ctx, int64_t T, const double *tpos, const int8_t *treq, swarm_board **out,
                       swarm_board_desc *info, void *stream) {
    return create_board(ctx, T, tpos, treq, false, nullptr, out, info, stream);
}

int swarm_board_create_moving(swarm_ctx *ctx, int64_t T, const double *tpos, const int8_t *treq,
                              const double *velocities, swarm_board **out, swarm_board_desc *info, void *stream) {
    return create_board(ctx, T, tpos, treq, true, velocities, out, info, stream);
}

int swarm_board_set_velocities(swarm_ctx *ctx, swarm_board *board, const double *velocities, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && board != nullptr, "ctx or board is NULL");
    SW_ARG(live_board(ctx, board), "the board is not a live board of this ctx");
    SW_ARG(board->moving, "the board does not move (swarm_board_create_moving makes one that does)");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<double> h_vel;
    if (const int rc = fetch_velocities(board->T, velocities, &h_vel, s)) return rc;
    if (board->T) {
        SW_HIP(hipMemcpyAsync(board->vel, h_vel.data(), size_t(board->T) * 16, hipMemcpyHostToDevice, s));
        SW_HIP(hipStreamSynchronize(s));
    }
    return SWARM_OK;
}

int swarm_board_set_lifetimes(swarm_ctx *ctx, swarm_board *board, const int64_t *open_tick, const int64_t *close_tick,
                              void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && board != nullptr, "ctx or board is NULL");
    SW_ARG((open_tick == nullptr) == (close_tick == nullptr), "open_tick and close_tick: both arrays, or both NULL");
    SW_ARG(live_board(ctx, board), "the board is not a live board of this ctx");
    SW_ARG(board->moving, "lifetimes need a moving board (swarm_board_create_moving; NULL velocities: at rest)");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    swarm_board *b = board;
    if (!open_tick) {  // no lifetimes: the board as it was made
        SW_HIP(hipDeviceSynchronize());  // queued work may still read them
        void *const dev[] = {b->life_open, b->life_close, b->present};
        for (void *p : dev)
            if (p) SW_HIP(hipFree(p));
        b->life_open = b->life_close = nullptr;
        b->present = nullptr;
        b->close_ticks.clear();
        b->life_fresh = false;
        return SWARM_OK;
    }
    const size_t T = size_t(b->T), rows = T ? T : 1;
    std::vector<int64_t> h_open, h_close, closes;
    try {
        h_open.resize(rows);
        h_close.resize(rows);
        if (T) {  // (device or host arrays)
            SW_HIP(hipMemcpyAsync(h_open.data(), open_tick, T * 8, hipMemcpyDefault, s));
            SW_HIP(hipMemcpyAsync(h_close.data(), close_tick, T * 8, hipMemcpyDefault, s));
            SW_HIP(hipStreamSynchronize(s));
        }
        int64_t bad = -1;
        switch (task_life_check(b->T, h_open.data(), h_close.data(), &bad)) {
        case kTaskLifeOk:
            break;
        case kTaskLifeNegative:
            set_error("invalid argument: task %lld has a negative open or close tick", static_cast<long long>(bad));
            return SWARM_ERR_ARG;
        default:
            set_error("invalid argument: task %lld opens after it closes", static_cast<long long>(bad));
            return SWARM_ERR_ARG;
        }
        closes = task_close_ticks(b->T, h_close.data());
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for %zu lifetimes", T);
        return SWARM_ERR_OOM;
    }
    if (!b->life_open) {  // all three or none: a failure leaves the board without lifetimes
        int64_t *o = nullptr, *c = nullptr;
        uint8_t *p = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&o), rows * 8) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&c), rows * 8) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&p), rows) != hipSuccess) {
            (void)hipGetLastError();
            if (o) (void)hipFree(o);
            if (c) (void)hipFree(c);
            set_error("out of device memory for %zu lifetimes", T);
            return SWARM_ERR_OOM;
        }
        b->life_open = o, b->life_close = c, b->present = p;
    }
    if (T) {
        SW_HIP(hipMemcpyAsync(b->life_open, h_open.data(), T * 8, hipMemcpyHostToDevice, s));
        SW_HIP(hipMemcpyAsync(b->life_close, h_close.data(), T * 8, hipMemcpyHostToDevice, s));
        SW_HIP(hipStreamSynchronize(s));
    }
    b->close_ticks = std::move(closes);
    b->life_fresh = true;
    return SWARM_OK;
}

int swarm_board_lifetimes(const swarm_board *board, const int64_t **open_tick, const int64_t **close_tick) {
    using namespace swarm;
    SW_ARG(board != nullptr && open_tick != nullptr && close_tick != nullptr, "board, open_tick or close_tick is NULL");
    *open_tick = board->life_open;
    *close_tick = board->life_close;
    return SWARM_OK;
}

int swarm_board_last_tick(const swarm_board *board, int64_t *last_tick) {
    using namespace swarm;
    SW_ARG(board != nullptr && last_tick != nullptr, "board or last_tick is NULL");
    *last_tick = board->last_tick;
    return SWARM_OK;
}

int swarm_board_place(swarm_ctx *ctx, swarm_board *board, int64_t n, const swarm_board_state *state, int64_t m,
                      const int32_t *idx, const double *tpos, const int8_t *treq, const double *vel,
                      const int64_t *open_tick, const int64_t *close_tick, uint32_t flags, int64_t *purged,
                      void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && board != nullptr && state != nullptr, "ctx, board or state is NULL");
    SW_ARG((flags & ~uint32_t(SWARM_PLACE_KEEP_TABLES)) == 0, "unknown flag");
    SW_ARG(n >= 0 && n < (int64_t(1) << 31), "n must be in [0, 2^31)");
    SW_ARG(m >= 0, "m must not be negative");
    SW_ARG(m == 0 || (idx && tpos && treq && open_tick && close_tick), "NULL request array");
    SW_ARG(state->Ks >= 1 && state->Ks <= 4096 && state->Kt >= 1 && state->Kt <= 4096,
           "status / table slots must be in [1, 4096]");
    SW_ARG(live_board(ctx, board), "the board is not a live board of this ctx");
    swarm_board *b = board;
    SW_ARG(b->moving && b->alive(), "placing needs a moving board with lifetimes (swarm_board_set_lifetimes)");
    SW_ARG(!b->life_fresh && b->last_tick >= 0,
           "the lifetimes were set and no tick has run since: the retire they owe has not happened");
    const bool purge = !(flags & SWARM_PLACE_KEEP_TABLES) && n > 0;
    SW_ARG(!purge || (state->tab_task && state->tab_winner && state->tab_util), "NULL table array");
    SW_ARG(m <= b->T, "more requests than slots: a slot is listed twice");
    if (purged) *purged = 0;
    if (m == 0) return SWARM_OK;
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t um = size_t(m);
    const int64_t T = b->T, last = b->last_tick;
    // the requests into the staging buffer (host or device arrays), the slots' current windows behind them
    if (const int rc = grow(&b->place_buf, &b->cap_place, um * kPlaceBytes)) return rc;
    const PlaceReq r = place_sections(b->place_buf, um);
    SW_HIP(hipMemcpyAsync(r.idx, idx, um * 4, hipMemcpyDefault, s));
    SW_HIP(hipMemcpyAsync(r.pos, tpos, um * 16, hipMemcpyDefault, s));
    SW_HIP(hipMemcpyAsync(r.req, treq, um, hipMemcpyDefault, s));
    SW_HIP(hipMemcpyAsync(r.open, open_tick, um * 8, hipMemcpyDefault, s));
    SW_HIP(hipMemcpyAsync(r.close, close_tick, um * 8, hipMemcpyDefault, s));
    if (vel)
        SW_HIP(hipMemcpyAsync(r.vel, vel, um * 16, hipMemcpyDefault, s));
    else
        SW_HIP(hipMemsetAsync(r.vel, 0, um * 16, s));
    hipLaunchKernelGGL(k_board_place_fetch, dim3(grid_for(m, kBlock, 4096)), dim3(kBlock), 0, s, m, T, r, b->life_open,
                       b->life_close);
    SW_LAUNCHED();
    std::vector<char> host;
    std::vector<int64_t> closes;
    try {
        host.resize(um * kPlaceBytes);
        SW_HIP(hipMemcpyAsync(host.data(), b->place_buf, host.size(), hipMemcpyDeviceToHost, s));
        SW_HIP(hipStreamSynchronize(s));  // the one wait before anything is written
        const PlaceReq h = place_sections(host.data(), um);
        int64_t bad = -1;
        PlaceStatus st = place_check(T, last, m, h.idx, h.old_open, h.old_close, reinterpret_cast<double *>(h.pos),
                                     reinterpret_cast<double *>(h.vel), h.req, h.open, h.close, &bad);
        int32_t dup = -1;
        if (st == kPlaceOk && place_has_duplicate(m, h.idx, &dup)) {
            set_error("invalid argument: slot %d is listed twice", int(dup));
            return SWARM_ERR_ARG;
        }
        if (st != kPlaceOk) {
            set_error("invalid argument: request %lld (slot %d) %s", static_cast<long long>(bad), int(h.idx[bad]),
                      place_reason(st));
            return SWARM_ERR_ARG;
        }
        closes = b->close_ticks;
        place_update_closes(&closes, last, m, h.close);
    } catch (const std::bad_alloc &) {
        set_error("out of host memory for %zu placed tasks", um);
        return SWARM_ERR_OOM;
    }
    int64_t nparts = 0;
    int lg = 0;
    unsigned pgrid = 1;
    if (purge) {  // the buffers first: an allocation that fails leaves the board as it was
        while (lg < 6 && (1 << lg) < state->Kt) ++lg;
        int64_t waves = (n + (kWave >> lg) - 1) / (kWave >> lg);
        if (state->Kt <= kWave) waves = (waves + kRetireTurn - 1) / kRetireTurn;
        pgrid = grid_for(waves * kWave, kBlock, 16384);
        nparts = int64_t(pgrid) * (kBlock / kWave);
        if (const int rc = grow(&b->purge_part, &b->cap_part, size_t(nparts) * 8)) return rc;
        if (!b->placed) {
            SW_HIP(hipMalloc(reinterpret_cast<void **>(&b->placed), size_t(T)));
            SW_HIP(hipMemsetAsync(b->placed, 0, size_t(T), s));
        }
    }
    hipLaunchKernelGGL(k_board_place, dim3(grid_for(m, kBlock, 4096)), dim3(kBlock), 0, s, m, T, r,
                       reinterpret_cast<double2 *>(b->tpos), reinterpret_cast<double2 *>(b->lag),
                       reinterpret_cast<double2 *>(b->vel), b->treq, b->life_open, b->life_close,
                       purge ? b->placed : nullptr);
    SW_LAUNCHED();
    b->close_ticks.swap(closes);
    b->placed_on = true;
    if (purge) {
        hipLaunchKernelGGL(k_board_purge, dim3(pgrid), dim3(kBlock), 0, s, n, state->Kt, lg, int32_t(T), b->placed,
                           state->tab_task, state->tab_winner, reinterpret_cast<int32_t *>(state->tab_util),
                           static_cast<unsigned long long *>(b->purge_part));
        SW_LAUNCHED();
        hipLaunchKernelGGL(k_board_place_done, dim3(grid_for(m, kBlock, 4096)), dim3(kBlock), 0, s, m, T, r.idx,
                           b->placed, nparts, static_cast<const unsigned long long *>(b->purge_part), b->verdict + 5);
        SW_LAUNCHED();
        SW_HIP(hipMemcpyAsync(b->verdict_host + 5, b->verdict + 5, 8, hipMemcpyDeviceToHost, s));
    }
    SW_HIP(hipStreamSynchronize(s));  // the staging buffer and *purged end with this call
    if (purge && purged) *purged = int64_t(b->verdict_host[5]);
    return SWARM_OK;
}

int swarm_board_positions(const swarm_board *board, const double **cur, const double **lag) {
    using namespace swarm;
    SW_ARG(board != nullptr && cur != nullptr && lag != nullptr, "board, cur or lag is NULL");
    *cur = board->tpos;
    *lag = board->moving ? board->lag : board->tpos;
    return SWARM_OK;
}

int swarm_board_call_box(swarm_ctx *ctx, swarm_board *board, double dt, int32_t ticks, double *box_host,
                         void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && board != nullptr && box_host != nullptr, "ctx, board or box_host is NULL");
    SW_ARG(live_board(ctx, board), "the board is not a live board of this ctx");
    SW_ARG(board->moving, "the board does not move (swarm_board_create_moving makes one that does)");
    SW_ARG(ticks >= 0 && std::isfinite(dt), "ticks or dt out of range");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = moving_board_box(board, dt, ticks, s)) return rc;
    SW_HIP(hipStreamSynchronize(s));
    memcpy(box_host, board->verdict_host + 1, 32);
    return SWARM_OK;
}

int swarm_board_refresh(swarm_ctx *ctx, swarm_board *board, swarm_board_desc *info, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr && board != nullptr, "ctx or board is NULL");
    SW_ARG(live_board(ctx, board), "the board is not a live board of this ctx");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    swarm_board *b = board;
    if (b->moving) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        const size_t T = size_t(b->T);
        std::vector<double> h_pos;
        std::vector<uint32_t> off;
        std::vector<int32_t> idx;
        Grid g{};
        int rc;
        try {
            h_pos.resize(T * 2);
            idx.resize(T);
            if (T) {
                SW_HIP(hipMemcpyAsync(h_pos.data(), b->tpos, T * 16, hipMemcpyDeviceToHost, s));
                SW_HIP(hipStreamSynchronize(s));
            }
            if ((rc = motion_error(task_static_grid(b->T, h_pos.data(), &g)))) return rc;
            const int64_t ncells = g.ncx * g.ncy;
            off.resize(size_t(ncells) + 1);
            if ((rc = size_buffers(b, ncells, s))) return rc;
            if ((rc = build_lists(b, g, nullptr, s))) return rc;
            SW_HIP(hipMemcpyAsync(off.data(), b->dyn_off, off.size() * 4, hipMemcpyDeviceToHost, s));
            if (T) SW_HIP(hipMemcpyAsync(idx.data(), b->vals[1], T * 4, hipMemcpyDeviceToHost, s));
            SW_HIP(hipStreamSynchronize(s));
        } catch (const std::bad_alloc &) {
            set_error("out of host memory for the board's cell lists");
            return SWARM_ERR_OOM;
        }
        int64_t longest = 0;
        for (size_t c = 0; c + 1 < off.size(); ++c)
            longest = int64_t(off[c + 1] - off[c]) > longest ? int64_t(off[c + 1] - off[c]) : longest;
        b->g = g;
        b->longest = longest;
        b->cell_off_host = std::move(off);
        b->idx_host = std::move(idx);
    }
    if (info) *info = describe(*b);
    return SWARM_OK;
}

int swarm_board_info(const swarm_board *board, swarm_board_desc *info) {
    using namespace swarm;
    SW_ARG(board != nullptr && info != nullptr, "board or info is NULL");
    *info = describe(*board);
    return SWARM_OK;
}

int swarm_board_read(const swarm_board *board, uint32_t *cell_off_host, int32_t *idx_host) {
    using namespace swarm;
    SW_ARG(board != nullptr, "board is NULL");
    if (cell_off_host) memcpy(cell_off_host, board->cell_off_host.data(), board->cell_off_host.size() * 4);
    if (idx_host && !board->idx_host.empty()) memcpy(idx_host, board->idx_host.data(), board->idx_host.size() * 4);
    return SWARM_OK;
}

int swarm_board_destroy(swarm_ctx *ctx, swarm_board *board) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    if (!board) return SWARM_OK;
    auto &v = ctx->boards;
    auto it = v.begin();
    while (it != v.end() && *it != board) ++it;
    SW_ARG(it != v.end(), "the board is not a live board of this ctx");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    SW_HIP(hipDeviceSynchronize());  // queued work may still read the board
    v.erase(it);
    bury_board(ctx, board);
    return SWARM_OK;
}

}  // extern "C"
