// Uniform-grid binning of agents (cell-list), shared by the RGG builder, the spatial storage
// order and the binned allocation.  Agents are bucketed by row-major cell key with a hipCUB
// radix sort; cell_off[c] is the first sorted position of cell c (exclusive prefix), so the
// agents of cells [c0, c1] of one grid row are the contiguous range [cell_off[c0],
// cell_off[c1 + 1]).
#pragma once

#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <cmath>
#include <cstring>

#include "swarm_common.h"

namespace swarm {

// fmin / fmax return the other operand for a NaN, so a NaN position leaves no trace in the box: the sensed
// physics and loop rely on that (an agent a singular step left NaN is absent from every later step's grid).
// kNanIsInf: a NaN coordinate counts as +inf instead, for the callers that refuse every non-finite position.
template <bool kNanIsInf>
static __global__ __launch_bounds__(kBlock) void k_bbox_partial(const double2 *__restrict__ pos,
                                                               int64_t n, double *__restrict__ part) {
    double mnx = DBL_MAX, mny = DBL_MAX, mxx = -DBL_MAX, mxy = -DBL_MAX;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
        const double2 p = pos[i];
        if (kNanIsInf && (p.x != p.x || p.y != p.y)) mxx = HUGE_VAL;
        mnx = fmin(mnx, p.x); mny = fmin(mny, p.y);
        mxx = fmax(mxx, p.x); mxy = fmax(mxy, p.y);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mnx = fmin(mnx, __shfl_xor(mnx, off, 64));
        mny = fmin(mny, __shfl_xor(mny, off, 64));
        mxx = fmax(mxx, __shfl_xor(mxx, off, 64));
        mxy = fmax(mxy, __shfl_xor(mxy, off, 64));
    }
    __shared__ double s[4][kBlock / kWave];
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s[0][wid] = mnx; s[1][wid] = mny; s[2][wid] = mxx; s[3][wid] = mxy; }
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

// One wave folds the per-block partials.
static __global__ void k_bbox_final(const double *__restrict__ part, int nparts, double *__restrict__ out) {
    double b0 = DBL_MAX, b1 = DBL_MAX, b2 = -DBL_MAX, b3 = -DBL_MAX;
    for (int i = threadIdx.x; i < nparts; i += kWave) {
        b0 = fmin(b0, part[4 * i + 0]); b1 = fmin(b1, part[4 * i + 1]);
        b2 = fmax(b2, part[4 * i + 2]); b3 = fmax(b3, part[4 * i + 3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        b0 = fmin(b0, __shfl_xor(b0, off, 64)); b1 = fmin(b1, __shfl_xor(b1, off, 64));
        b2 = fmax(b2, __shfl_xor(b2, off, 64)); b3 = fmax(b3, __shfl_xor(b3, off, 64));
    }
    if (threadIdx.x == 0) { out[0] = b0; out[1] = b1; out[2] = b2; out[3] = b3; }
}

static __global__ __launch_bounds__(kBlock) void k_cell_keys(const double2 *__restrict__ pos, int64_t n,
                                                            Grid g, uint32_t *__restrict__ keys,
                                                            int32_t *__restrict__ vals) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += int64_t(gridDim.x) * kBlock) {
        const double2 p = pos[i];
        const int64_t cx = cell_coord(p.x, g.xmin, g.inv_cell, g.ncx);
        const int64_t cy = cell_coord(p.y, g.ymin, g.inv_cell, g.ncy);
        keys[i] = uint32_t(cy * g.ncx + cx);
        vals[i] = int32_t(i);
    }
}

// cell_off[c] = #agents with key < c, for c in [0, ncells]
static __global__ __launch_bounds__(kBlock) void k_cell_offsets(const uint32_t *__restrict__ skeys, int64_t n,
                                                               int64_t ncells, uint32_t *__restrict__ off) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i <= n; i += int64_t(gridDim.x) * kBlock) {
        const int64_t lo = (i == 0) ? 0 : int64_t(skeys[i - 1]) + 1;
        const int64_t hi = (i == n) ? ncells : int64_t(skeys[i]);
        for (int64_t c = lo; c <= hi; ++c) off[c] = uint32_t(i);
    }
}

// The same offsets by search, one thread per cell: cell_off[c] = the first sorted position whose key is
// >= c.  k_cell_offsets has the thread at a key boundary fill every empty cell up to the next key, one store
// after the other: right when most cells are occupied, but a grid grown far beyond the agents (the sensed
// update loop's: the entry box plus the run's reach, 100 units a side for 200 ticks) leaves the first and
// the last thread ~1e5 cells of margin each (1.4 of 4.8 ms per tick at 10M agents).
static __global__ __launch_bounds__(kBlock) void k_cell_offsets_search(const uint32_t *__restrict__ skeys,
                                                                      int64_t n, int64_t ncells,
                                                                      uint32_t *__restrict__ off) {
    for (int64_t c = int64_t(blockIdx.x) * kBlock + threadIdx.x; c <= ncells; c += int64_t(gridDim.x) * kBlock) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (int64_t(skeys[mid]) < c) lo = mid + 1;
            else hi = mid;
        }
        off[c] = uint32_t(lo);
    }
}

// shape_grid (grid_shape.h) for a library entry point: a box without a finite extent is SWARM_ERR_ARG.
static inline int shape_grid_checked(Grid *g, double cell, int64_t max_cells) {
    if (!shape_grid(g, cell, max_cells)) {
        set_error("invalid argument: %s", kExtentError);
        return SWARM_ERR_ARG;
    }
    return SWARM_OK;
}

// Bounding box of n positions -> host Grid with cells of side >= `cell` (enlarged if the grid
// would exceed max_cells).  One host sync (the grid shape sizes the launch).  SWARM_ERR_ARG for an
// infinite position -- and for a NaN one with refuse_nan (k_bbox_partial) -- and for a box whose extent is
// not finite.
static inline int make_grid(swarm_ctx *ctx, int64_t n, const double *pos, double cell, int64_t max_cells,
                            Grid *g, hipStream_t s, bool refuse_nan = false) {
    const unsigned np = grid_for(n, kBlock, 1024);
    double *part;
    SW_ALLOC(part, ctx, S_BBOX, size_t(np) * 4 * 8 + 64);
    double *fin = part + size_t(np) * 4;
    if (refuse_nan)
        hipLaunchKernelGGL(k_bbox_partial<true>, dim3(np), dim3(kBlock), 0, s,
                           reinterpret_cast<const double2 *>(pos), n, part);
    else
        hipLaunchKernelGGL(k_bbox_partial<false>, dim3(np), dim3(kBlock), 0, s,
                           reinterpret_cast<const double2 *>(pos), n, part);
    SW_LAUNCHED();
    hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(64), 0, s, part, int(np), fin);
    SW_LAUNCHED();
    double *hb = static_cast<double *>(pinned(ctx, 64));
    if (!hb) return SWARM_ERR_OOM;
    SW_HIP(hipMemcpyAsync(hb, fin, 32, hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    if (!(std::isfinite(hb[0]) && std::isfinite(hb[1]) && std::isfinite(hb[2]) && std::isfinite(hb[3]))) {
        set_error("positions must be finite");
        return SWARM_ERR_ARG;
    }
    g->xmin = hb[0]; g->ymin = hb[1]; g->xmax = hb[2]; g->ymax = hb[3];
    return shape_grid_checked(g, cell, max_cells);
}

// Sort agents by cell.  On return *sorted_idx (device, n) lists agent indices cell by cell
// (ascending index within a cell: the radix sort is stable) and *cell_off (device,
// ncells + 1) is the exclusive prefix.  sparse_grid: the offsets by search (k_cell_offsets_search), for a grid
// with wide empty margins.
static inline int bin_agents(swarm_ctx *ctx, int64_t n, const double *pos, const Grid &g,
                             int32_t **sorted_idx, uint32_t **cell_off, hipStream_t s, bool sparse_grid = false) {
    const int64_t ncells = g.ncx * g.ncy;
    uint32_t *kin, *kout, *off;
    int32_t *vin, *vout;
    SW_ALLOC(kin, ctx, S_KEYS_IN, size_t(n) * 4);
    SW_ALLOC(kout, ctx, S_KEYS_OUT, size_t(n) * 4);
    SW_ALLOC(vin, ctx, S_VALS_IN, size_t(n) * 4);
    SW_ALLOC(vout, ctx, S_VALS_OUT, size_t(n) * 4);
    SW_ALLOC(off, ctx, S_CELL_START, size_t(ncells + 1) * 4);
    hipLaunchKernelGGL(k_cell_keys, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s,
                       reinterpret_cast<const double2 *>(pos), n, g, kin, vin);
    SW_LAUNCHED();
    int end_bit = 1;
    while (end_bit < 32 && (int64_t(1) << end_bit) < ncells) ++end_bit;
    size_t tmp_bytes = 0;
    SW_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, kin, kout, vin, vout, int(n), 0, end_bit, s));
    void *tmp;
    SW_ALLOC(tmp, ctx, S_CUB_TMP, tmp_bytes);
    SW_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, kin, kout, vin, vout, int(n), 0, end_bit, s));
    if (sparse_grid)
        hipLaunchKernelGGL(k_cell_offsets_search, dim3(grid_for(ncells + 1, kBlock, 8192)), dim3(kBlock), 0, s, kout,
                           n, ncells, off);
    else
        hipLaunchKernelGGL(k_cell_offsets, dim3(grid_for(n + 1, kBlock, 8192)), dim3(kBlock), 0, s, kout, n,
                           ncells, off);
    SW_LAUNCHED();
    *sorted_idx = vout;
    *cell_off = off;
    return SWARM_OK;
}

// Work a kernel that scans every agent's 3 x 3 cell window will do, from the cell occupancies alone:
// W = sum over agents of their window's occupancy (a double: a bound, not a count) and the longest
// serial scan is the largest window (max_win).
static __global__ __launch_bounds__(kBlock) void k_window_work(const uint32_t *__restrict__ off, Grid g,
                                                              double *__restrict__ out,
                                                              unsigned long long *__restrict__ max_win) {
    double w = 0.0;
    unsigned long long mx = 0;
    const int64_t ncells = g.ncx * g.ncy;
    for (int64_t c = int64_t(blockIdx.x) * kBlock + threadIdx.x; c < ncells; c += int64_t(gridDim.x) * kBlock) {
        const uint32_t occ = off[c + 1] - off[c];
        if (occ == 0) continue;
        const int64_t cx = c % g.ncx, cy = c / g.ncx;
        const int64_t x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < g.ncx ? cx + 1 : g.ncx - 1;
        unsigned long long win = 0;
        for (int64_t yy = (cy > 0 ? cy - 1 : 0); yy <= cy + 1 && yy < g.ncy; ++yy)
            win += off[yy * g.ncx + x1 + 1] - off[yy * g.ncx + x0];
        w += double(occ) * double(win);
        mx = win > mx ? win : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        w += __shfl_xor(w, o, 64);
        const unsigned long long m = __shfl_xor(mx, o, 64);
        mx = m > mx ? m : mx;
    }
    // one atomic pair per workgroup: every wave of the grid adding to the same two words serialised
    // them (0.7 ms at 2M cells)
    __shared__ double s_w[kBlock / kWave];
    __shared__ unsigned long long s_mx[kBlock / kWave];
    if ((threadIdx.x & 63) == 0) {
        s_w[threadIdx.x >> 6] = w;
        s_mx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBlock / kWave; ++k) {
            w += s_w[k];
            mx = s_mx[k] > mx ? s_mx[k] : mx;
        }
        if (w > 0.0) {
            atomicAdd(out, w);
            atomicMax(max_win, mx);
        }
    }
}

// Bounds on a window-scanning kernel's work (one thread per agent): a radius graph over co-located
// agents (a million agents in one cell) would make swarm_build_rgg run for hours on the device.  A
// deg-16 RGG has windows of ~45 agents: W ~ 45 n (100M agents: 4.5e9), far below these.
constexpr double kMaxScanPairs = 68719476736.0;          // 2^36 candidate checks in all
constexpr unsigned long long kMaxWindow = 1ull << 20;    // candidates one thread scans

__host__ __device__ inline bool window_work_exceeded(double pairs, unsigned long long max_window) {
    return pairs > kMaxScanPairs || max_window > kMaxWindow;
}

inline void set_window_work_error(const char *what, double pairs, unsigned long long max_window) {
    set_error("%s: %.3g candidate pairs to scan (limit %.3g), the largest 3x3-cell "
              "window holds %llu agents (limit %llu) -- co-located agents?",
              what, pairs, kMaxScanPairs, max_window, kMaxWindow);
}

// k_window_work of the binned agents, stream-ordered: (*acc)[0] = W (double), (*acc)[1] = max_win (u64).
static inline int launch_window_work(swarm_ctx *ctx, const uint32_t *off, const Grid &g, hipStream_t s,
                                     double **acc_out) {
    double *acc;
    SW_ALLOC(acc, ctx, S_CELL_END, 64);
    SW_HIP(hipMemsetAsync(acc, 0, 16, s));
    hipLaunchKernelGGL(k_window_work, dim3(grid_for(g.ncx * g.ncy, kBlock, 8192)), dim3(kBlock), 0, s, off, g, acc,
                       reinterpret_cast<unsigned long long *>(acc + 1));
    SW_LAUNCHED();
    *acc_out = acc;
    return SWARM_OK;
}

// The same, read back and judged on the host (one host sync): SWARM_ERR_RANGE beyond the limits.
static inline int check_window_work(swarm_ctx *ctx, const uint32_t *off, const Grid &g, hipStream_t s,
                                    unsigned long long *max_window) {
    double *acc;
    const int rc = launch_window_work(ctx, off, g, s, &acc);
    if (rc) return rc;
    double *h = static_cast<double *>(pinned(ctx, 64));
    if (!h) return SWARM_ERR_OOM;
    SW_HIP(hipMemcpyAsync(h, acc, 16, hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    unsigned long long m;
    memcpy(&m, h + 1, 8);
    *max_window = m;
    if (window_work_exceeded(h[0], m)) {
        set_window_work_error("radius graph too dense to build", h[0], m);
        return SWARM_ERR_RANGE;
    }
    return SWARM_OK;
}

}  // namespace swarm
