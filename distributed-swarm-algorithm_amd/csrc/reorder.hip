// Restoring the spatial storage order of a moved swarm (contract R1): the canonical order of the
// current positions (swarm_resort_plan), a row permutation of any number of per-agent arrays in one pass
// (swarm_permute_rows) and the neighbour graph in the new numbering (swarm_graph_relabel).
// Not reference code: the reference keeps its agents in a Python list and has no storage order.
#include <hipcub/hipcub.hpp>

#include <cmath>

#include "swarm_common.h"

namespace swarm {
namespace {

constexpr int kMaxArrays = 64;      // arrays one swarm_permute_rows call takes
constexpr int64_t kMaxRowBytes = 16384;  // a board row of 4096 slots
constexpr int kBatch = 16;          // narrow arrays whose gathers one thread keeps in flight (16 x 16 B = 64 VGPRs)

// verdict bits of the entry checks
constexpr unsigned kBadRange = 1, kBadDup = 2, kBadRowPtr = 4, kBadCol = 8;

// The narrow arrays of a call, by value in the kernel arguments (8 + 64 x 24 = 1544 bytes).
struct RowSet {
    int32_t count;
    int32_t pad;
    swarm_rows a[kMaxArrays];
};

__device__ __forceinline__ void fold_verdict(unsigned out, unsigned *bad) {
    if (__ballot(out != 0)) {  // one atomic per wave that found something
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) out |= __shfl_xor(out, off, 64);
        if ((threadIdx.x & 63) == 0) atomicOr(bad, out);
    }
}

// `from` is a permutation of [0, n): every value in range and no bit of the (zeroed) bitmap set twice.
__global__ __launch_bounds__(kBlock) void k_perm_check(const int32_t *__restrict__ from, int64_t n,
                                                      unsigned long long *__restrict__ bits,
                                                      unsigned *__restrict__ bad) {
    unsigned out = 0;
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < n; k += int64_t(gridDim.x) * kBlock) {
        const int64_t f = from[k];
        if (f < 0 || f >= n) {
            out |= kBadRange;
        } else {
            const unsigned long long m = 1ull << (f & 63);
            if (atomicOr(&bits[f >> 6], m) & m) out |= kBadDup;
        }
    }
    fold_verdict(out, bad);
}

// row_ptr starts at 0 and never decreases: every row slice then lies inside [0, row_ptr[n]).
__global__ __launch_bounds__(kBlock) void k_rowptr_check(const int32_t *__restrict__ rp, int64_t n,
                                                        unsigned *__restrict__ bad) {
    unsigned out = 0;
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < n; k += int64_t(gridDim.x) * kBlock) {
        if (rp[k] > rp[k + 1]) out |= kBadRowPtr;
        if (k == 0 && rp[0] != 0) out |= kBadRowPtr;
    }
    fold_verdict(out, bad);
}

// Every column names a row in [0, n).  A wave takes a task of 64 rows -- one contiguous edge slice, as
// elect.hip's k_check_col16 walks them -- and reads it 8 columns per lane per pass.  A slice outside
// [0, row_ptr[n]] (a row_ptr k_rowptr_check refuses as well) is not read.
__global__ __launch_bounds__(kBlock) void k_col_check(const int32_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                     int64_t n, unsigned *__restrict__ bad) {
    constexpr int kU = 8;
    const int lane = threadIdx.x & 63;
    const int64_t ntask = (n + 63) / 64;
    const int32_t total = rp[n];
    unsigned out = 0;
    for (int64_t task = int64_t(blockIdx.x) * (kBlock / kWave) + (threadIdx.x >> 6); task < ntask;
         task += int64_t(gridDim.x) * (kBlock / kWave)) {
        const int64_t base = task * 64;
        const int32_t b = rp[base], e = rp[base + 64 < n ? base + 64 : n];
        if (b < 0 || b > e || e > total) {
            out |= kBadRowPtr;
            continue;
        }
        for (int64_t k0 = b; k0 < e; k0 += 64 * kU) {
            int32_t c[kU];
#pragma unroll
            for (int j = 0; j < kU; ++j) {
                const int64_t k = k0 + j * 64 + lane;
                c[j] = k < e ? col[k] : 0;
            }
#pragma unroll
            for (int j = 0; j < kU; ++j) out |= (c[j] < 0 || c[j] >= n) ? kBadCol : 0u;
        }
    }
    fold_verdict(out, bad);
}

__device__ __forceinline__ uint4 load_row(const void *src, int64_t r, int w) {
    uint4 v = {0u, 0u, 0u, 0u};
    switch (w) {
    case 1: v.x = static_cast<const uint8_t *>(src)[r]; break;
    case 2: v.x = static_cast<const uint16_t *>(src)[r]; break;
    case 4: v.x = static_cast<const uint32_t *>(src)[r]; break;
    case 8: {
        const uint2 t = static_cast<const uint2 *>(src)[r];
        v.x = t.x;
        v.y = t.y;
        break;
    }
    default: v = static_cast<const uint4 *>(src)[r];
    }
    return v;
}

__device__ __forceinline__ void store_row(void *dst, int64_t r, int w, const uint4 &v) {
    switch (w) {
    case 1: static_cast<uint8_t *>(dst)[r] = uint8_t(v.x); break;
    case 2: static_cast<uint16_t *>(dst)[r] = uint16_t(v.x); break;
    case 4: static_cast<uint32_t *>(dst)[r] = v.x; break;
    case 8: static_cast<uint2 *>(dst)[r] = make_uint2(v.x, v.y); break;
    default: static_cast<uint4 *>(dst)[r] = v;
    }
}

// Rows of 1, 2, 4, 8 or 16 bytes, every narrow array of the call in one launch: thread k reads from[k] once
// (coalesced), issues the gather loads of up to kBatch arrays -- they are latency-bound, so they all go out before
// the first of them is waited for -- and then does that batch's coalesced stores.  The widths are uniform over the
// launch: every branch on them is a scalar one.
__global__ __launch_bounds__(kBlock) void k_permute_narrow(const RowSet set, const int32_t *__restrict__ from,
                                                          int64_t n) {
    const int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= n) return;
    const int64_t f = from[k];
    for (int b = 0; b < set.count; b += kBatch) {
        uint4 v[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j)
            if (b + j < set.count) v[j] = load_row(set.a[b + j].src, f, int(set.a[b + j].row_bytes));
#pragma unroll
        for (int j = 0; j < kBatch; ++j)
            if (b + j < set.count) store_row(set.a[b + j].dst, k, int(set.a[b + j].row_bytes), v[j]);
    }
}

// A wide row: its `upr` units of sizeof(U) bytes go to consecutive lanes, so a row is read and written in whole
// lines; four units per thread are loaded before the first is stored.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename U>
__global__ __launch_bounds__(kBlock) void k_permute_wide(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                        const int32_t *__restrict__ from, int64_t n, int64_t row_bytes,
                                                        int64_t upr) {
    constexpr int kU = 4;
    const int64_t total = n * upr, stride = int64_t(gridDim.x) * kBlock;
    for (int64_t t0 = int64_t(blockIdx.x) * kBlock + threadIdx.x; t0 < total; t0 += kU * stride) {
        U v[kU];
        int64_t at[kU];
#pragma unroll
        for (int j = 0; j < kU; ++j) {
            const int64_t t = t0 + j * stride;
            at[j] = -1;
            v[j] = U(0);
            if (t < total) {
                const int64_t row = t / upr, u = t - row * upr;
                at[j] = row * row_bytes + u * int64_t(sizeof(U));
                v[j] = *reinterpret_cast<const U *>(src + int64_t(from[row]) * row_bytes + u * int64_t(sizeof(U)));
            }
        }
#pragma unroll
        for (int j = 0; j < kU; ++j)
            if (at[j] >= 0) *reinterpret_cast<U *>(dst + at[j]) = v[j];
    }
}

// to[from[k]] = k
__global__ __launch_bounds__(kBlock) void k_invert(const int32_t *__restrict__ from, int64_t n,
                                                  int32_t *__restrict__ to) {
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < n; k += int64_t(gridDim.x) * kBlock)
        to[from[k]] = int32_t(k);
}

// deg[k] = the length of row from[k]; deg[n] = 0 (the scan's last entry is then the edge count)
__global__ __launch_bounds__(kBlock) void k_degrees(const int32_t *__restrict__ from,
                                                   const int32_t *__restrict__ rp, int64_t n,
                                                   int32_t *__restrict__ deg) {
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k <= n; k += int64_t(gridDim.x) * kBlock) {
        int32_t d = 0;
        if (k < n) {
            const int64_t f = from[k];
            d = rp[f + 1] - rp[f];
        }
        deg[k] = d;
    }
}

// The column pass, edge-parallel: a workgroup of one wave takes 64 output rows, whose edges are one contiguous
// slice of col_out; lane l keeps row l's output and source offsets in LDS, and every edge of the slice finds its
// row by a search over those 65 offsets (empty rows are skipped by it), so a row of 300 neighbours is copied by all
// the lanes and the stores are coalesced.  Four edges per lane: their columns are loaded, then their new names,
// then they are stored.
__global__ __launch_bounds__(kWave) void k_relabel_cols(const int32_t *__restrict__ from,
                                                       const int32_t *__restrict__ rp,
                                                       const int32_t *__restrict__ col,
                                                       const int32_t *__restrict__ rpo,
                                                       const int32_t *__restrict__ to, int32_t *__restrict__ colo,
                                                       int64_t n) {
    constexpr int kU = 4;
    __shared__ int32_t s_out[kWave + 1], s_src[kWave];
    const int lane = threadIdx.x;
    const int64_t ntask = (n + 63) / 64;
    for (int64_t task = blockIdx.x; task < ntask; task += gridDim.x) {
        const int64_t base = task * 64, r = base + lane;
        const int32_t oe = rpo[base + 64 < n ? base + 64 : n];
        s_out[lane] = r < n ? rpo[r] : oe;
        s_src[lane] = r < n ? rp[from[r]] : 0;
        if (lane == 0) s_out[kWave] = oe;
        __syncthreads();
        const int32_t ob = s_out[0];
        for (int64_t k0 = ob; k0 < oe; k0 += 64 * kU) {
            int32_t c[kU];
#pragma unroll
            for (int j = 0; j < kU; ++j) {
                const int64_t k = k0 + j * 64 + lane;
                c[j] = -1;
                if (k < oe) {
                    int lo = 0, hi = kWave - 1;  // the last row whose first edge is at or before k
#pragma unroll
                    for (int step = 0; step < 6; ++step) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (int64_t(s_out[mid]) <= k) lo = mid;
                        else hi = mid - 1;
                    }
                    c[j] = col[int64_t(s_src[lo]) + (k - s_out[lo])];
                }
            }
#pragma unroll
            for (int j = 0; j < kU; ++j)
                if (c[j] >= 0) c[j] = to[c[j]];
#pragma unroll
            for (int j = 0; j < kU; ++j) {
                const int64_t k = k0 + j * 64 + lane;
                if (k < oe) colo[k] = c[j];
            }
        }
        __syncthreads();
    }
}

// pin[perm[k]] = pos[k] and inv[perm[k]] = k: the positions in input order, and where each input agent is stored
__global__ __launch_bounds__(kBlock) void k_to_input(const double2 *__restrict__ pos,
                                                    const int32_t *__restrict__ perm, int64_t n,
                                                    double2 *__restrict__ pin, int32_t *__restrict__ inv) {
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < n; k += int64_t(gridDim.x) * kBlock) {
        const int64_t i = perm[k];
        pin[i] = pos[k];
        inv[i] = int32_t(k);
    }
}

// from[k] = inv[order[k]] (the old storage index of the agent the new row k holds); *moved += rows that change
__global__ __launch_bounds__(kBlock) void k_compose(const int32_t *__restrict__ order,
                                                   const int32_t *__restrict__ inv, int64_t n,
                                                   int32_t *__restrict__ from, int32_t *__restrict__ perm_out,
                                                   unsigned long long *__restrict__ moved) {
    unsigned long long mine = 0;
    for (int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x; k < n; k += int64_t(gridDim.x) * kBlock) {
        const int32_t i = order[k];
        const int32_t f = inv[i];
        from[k] = f;
        perm_out[k] = i;
        mine += f != int32_t(k) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(moved, mine);
}

bool overlap(const void *a, int64_t an, const void *b, int64_t bn) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return an > 0 && bn > 0 && a0 < b0 + uintptr_t(bn) && b0 < a0 + uintptr_t(an);
}

bool aligned(const void *p, int64_t to) { return reinterpret_cast<uintptr_t>(p) % uintptr_t(to) == 0; }

// Enqueues the permutation check of `from` into the ctx's bitmap and verdict word (both zeroed first); *d_bad is
// the verdict word, for further checks of the same call to fold into.
int enqueue_perm_check(swarm_ctx *ctx, const int32_t *from, int64_t n, unsigned **d_bad, hipStream_t s) {
    const size_t words = size_t((n + 63) / 64);
    unsigned long long *buf;
    SW_ALLOC(buf, ctx, S_REORDER_BITS, 64 + words * 8);
    SW_HIP(hipMemsetAsync(buf, 0, 64 + words * 8, s));
    *d_bad = reinterpret_cast<unsigned *>(buf);
    hipLaunchKernelGGL(k_perm_check, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, from, n, buf + 8, *d_bad);
    SW_LAUNCHED();
    return SWARM_OK;
}

// The one host wait of a call's entry checks: the verdict word (and row_ptr[n] when rp_end is given).
int read_verdict(swarm_ctx *ctx, const unsigned *d_bad, const int32_t *rp_end, unsigned *verdict, int32_t *e_total,
                 hipStream_t s) {
    unsigned *h = static_cast<unsigned *>(pinned(ctx, 64));
    if (!h) return SWARM_ERR_OOM;
    SW_HIP(hipMemcpyAsync(h, d_bad, 4, hipMemcpyDeviceToHost, s));
    if (rp_end) SW_HIP(hipMemcpyAsync(h + 1, rp_end, 4, hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    *verdict = h[0];
    if (rp_end) *e_total = int32_t(h[1]);
    return SWARM_OK;
}

int perm_verdict(unsigned v, const char *who, const char *what) {
    if (v & kBadRange) {
        set_error("invalid argument: %s: %s names a row outside [0, n)", who, what);
        return SWARM_ERR_ARG;
    }
    if (v & kBadDup) {
        set_error("invalid argument: %s: %s names a row twice (not a permutation)", who, what);
        return SWARM_ERR_ARG;
    }
    return SWARM_OK;
}

}  // namespace
}  // namespace swarm

extern "C" {

int swarm_permute_rows(swarm_ctx *ctx, int64_t n, const int32_t *from, int32_t count, const swarm_rows *arrays,
                       void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(n >= 0 && n < (int64_t(1) << 31), "n must be in [0, 2^31)");
    SW_ARG(count >= 0 && count <= kMaxArrays, "count must be in [0, 64]");
    SW_ARG(count == 0 || arrays != nullptr, "arrays is NULL");
    for (int32_t i = 0; i < count; ++i)
        SW_ARG(arrays[i].row_bytes >= 1 && arrays[i].row_bytes <= kMaxRowBytes, "row_bytes must be in [1, 16384]");
    if (n == 0) return SWARM_OK;
    SW_ARG(from != nullptr, "from is NULL");
    SW_ARG(aligned(from, 4), "from is not aligned");
    for (int32_t i = 0; i < count; ++i) SW_ARG(arrays[i].src && arrays[i].dst, "NULL src / dst");
    for (int32_t i = 0; i < count; ++i) {
        const int64_t bytes = n * arrays[i].row_bytes;
        SW_ARG(!overlap(arrays[i].dst, bytes, from, n * 4), "a dst overlaps from");
        for (int32_t j = 0; j < count; ++j) {
            const int64_t other = n * arrays[j].row_bytes;
            SW_ARG(!overlap(arrays[i].dst, bytes, arrays[j].src, other), "a dst overlaps a src");
            SW_ARG(j == i || !overlap(arrays[i].dst, bytes, arrays[j].dst, other), "a dst overlaps another dst");
        }
    }
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned *d_bad, verdict = 0;
    int rc = enqueue_perm_check(ctx, from, n, &d_bad, s);
    if (rc) return rc;
    if ((rc = read_verdict(ctx, d_bad, nullptr, &verdict, nullptr, s))) return rc;
    if ((rc = perm_verdict(verdict, "swarm_permute_rows", "from"))) return rc;

    RowSet set{};
    for (int32_t i = 0; i < count; ++i) {
        const swarm_rows &a = arrays[i];
        const int64_t w = a.row_bytes;
        if ((w == 1 || w == 2 || w == 4 || w == 8 || w == 16) && aligned(a.src, w) && aligned(a.dst, w)) {
            set.a[set.count++] = a;
            continue;
        }
        const uint8_t *src = static_cast<const uint8_t *>(a.src);
        uint8_t *dst = static_cast<uint8_t *>(a.dst);
        const int64_t unit = (w % 16 == 0 && aligned(src, 16) && aligned(dst, 16)) ? 16
                             : (w % 4 == 0 && aligned(src, 4) && aligned(dst, 4))  ? 4
                                                                                   : 1;
        const int64_t upr = w / unit;
        const dim3 grid(grid_for(n * upr, int64_t(kBlock) * 4, 16384));
        if (unit == 16)
            hipLaunchKernelGGL(k_permute_wide<u32x4>, grid, dim3(kBlock), 0, s, src, dst, from, n, w, upr);
        else if (unit == 4)
            hipLaunchKernelGGL(k_permute_wide<uint32_t>, grid, dim3(kBlock), 0, s, src, dst, from, n, w, upr);
        else
            hipLaunchKernelGGL(k_permute_wide<uint8_t>, grid, dim3(kBlock), 0, s, src, dst, from, n, w, upr);
        SW_LAUNCHED();
    }
    if (set.count) {
        hipLaunchKernelGGL(k_permute_narrow, dim3(unsigned((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, set, from,
                           n);
        SW_LAUNCHED();
    }
    return SWARM_OK;
}

int swarm_graph_relabel(swarm_ctx *ctx, int64_t n, const int32_t *from, const int32_t *row_ptr, const int32_t *col,
                        int32_t *row_ptr_out, int32_t *col_out, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(n >= 0 && n < (int64_t(1) << 31) - 1, "n must be in [0, 2^31 - 1)");
    SW_ARG(row_ptr != nullptr && row_ptr_out != nullptr, "row_ptr / row_ptr_out is NULL");
    SW_ARG(n == 0 || from != nullptr, "from is NULL");
    const int64_t rpb = (n + 1) * 4;
    SW_ARG(!overlap(row_ptr_out, rpb, row_ptr, rpb) && !overlap(row_ptr_out, rpb, from, n * 4),
           "row_ptr_out overlaps an input");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {
        SW_HIP(hipMemsetAsync(row_ptr_out, 0, 4, s));
        return SWARM_OK;
    }
    unsigned *d_bad, verdict = 0;
    int32_t e_total = 0;
    int rc = enqueue_perm_check(ctx, from, n, &d_bad, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rowptr_check, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, row_ptr, n, d_bad);
    SW_LAUNCHED();
    if (col != nullptr) {
        hipLaunchKernelGGL(k_col_check, dim3(grid_for((n + 63) / 64, kBlock / kWave, 4096)), dim3(kBlock), 0, s,
                           row_ptr, col, n, d_bad);
        SW_LAUNCHED();
    }
    if ((rc = read_verdict(ctx, d_bad, row_ptr + n, &verdict, &e_total, s))) return rc;
    if ((rc = perm_verdict(verdict, "swarm_graph_relabel", "from"))) return rc;
    if (verdict & kBadRowPtr) {
        set_error("invalid argument: swarm_graph_relabel: row_ptr must start at 0 and never decrease");
        return SWARM_ERR_ARG;
    }
    if (verdict & kBadCol) {
        set_error("invalid argument: swarm_graph_relabel: a column names a row outside [0, n)");
        return SWARM_ERR_ARG;
    }
    SW_ARG(e_total == 0 || (col != nullptr && col_out != nullptr), "col / col_out is NULL");
    const int64_t cb = int64_t(e_total) * 4;
    SW_ARG(!overlap(col_out, cb, col, cb) && !overlap(col_out, cb, row_ptr, rpb) && !overlap(col_out, cb, from, n * 4) &&
               !overlap(col_out, cb, row_ptr_out, rpb) && !overlap(row_ptr_out, rpb, col, cb),
           "an output overlaps an input or the other output");

    int32_t *to, *deg;
    SW_ALLOC(to, ctx, S_REORDER_INV, size_t(n) * 4);
    SW_ALLOC(deg, ctx, S_REORDER_DEG, size_t(n + 1) * 4);
    const dim3 grid(grid_for(n + 1, kBlock, 8192));
    hipLaunchKernelGGL(k_invert, grid, dim3(kBlock), 0, s, from, n, to);
    SW_LAUNCHED();
    hipLaunchKernelGGL(k_degrees, grid, dim3(kBlock), 0, s, from, row_ptr, n, deg);
    SW_LAUNCHED();
    size_t tmp_bytes = 0;
    SW_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, deg, row_ptr_out, int(n + 1), s));
    void *tmp;
    SW_ALLOC(tmp, ctx, S_CUB_TMP, tmp_bytes);
    SW_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, deg, row_ptr_out, int(n + 1), s));
    if (e_total > 0) {
        hipLaunchKernelGGL(k_relabel_cols, dim3(grid_for((n + 63) / 64, 1, 65536)), dim3(kWave), 0, s, from, row_ptr,
                           col, row_ptr_out, to, col_out, n);
        SW_LAUNCHED();
    }
    return SWARM_OK;
}

int swarm_resort_plan(swarm_ctx *ctx, int64_t n, const double *pos, const int32_t *perm, double cell, int32_t *from,
                      int32_t *perm_out, int64_t *moved, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(n >= 0 && n < (int64_t(1) << 31), "n must be in [0, 2^31)");
    SW_ARG(cell > 0 && std::isfinite(cell), "cell must be positive and finite");
    SW_ARG(moved != nullptr, "moved is NULL");
    if (n == 0) {
        *moved = 0;
        return SWARM_OK;
    }
    SW_ARG(pos && perm && from && perm_out, "NULL array");
    SW_ARG(!overlap(from, n * 4, perm, n * 4) && !overlap(perm_out, n * 4, perm, n * 4) &&
               !overlap(from, n * 4, perm_out, n * 4) && !overlap(from, n * 4, pos, n * 16) &&
               !overlap(perm_out, n * 4, pos, n * 16),
           "an output overlaps an input or the other output");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned *d_bad, verdict = 0;
    int rc = enqueue_perm_check(ctx, perm, n, &d_bad, s);
    if (rc) return rc;
    if ((rc = read_verdict(ctx, d_bad, nullptr, &verdict, nullptr, s))) return rc;
    if ((rc = perm_verdict(verdict, "swarm_resort_plan", "perm"))) return rc;

    double2 *pin;
    int32_t *inv, *order;
    unsigned long long *d_moved;
    SW_ALLOC(pin, ctx, S_REORDER_POS, size_t(n) * 16);
    SW_ALLOC(inv, ctx, S_REORDER_INV, size_t(n) * 4);
    SW_ALLOC(order, ctx, S_REORDER_ORDER, size_t(n) * 4);
    SW_ALLOC(d_moved, ctx, S_REORDER_DEG, 64);
    const dim3 grid(grid_for(n, kBlock, 8192));
    hipLaunchKernelGGL(k_to_input, grid, dim3(kBlock), 0, s, reinterpret_cast<const double2 *>(pos), perm, n, pin, inv);
    SW_LAUNCHED();
    // the order a fresh swarm of these input positions gets: swarm_cell_order itself (its non-finite check included)
    if ((rc = swarm_cell_order(ctx, n, reinterpret_cast<const double *>(pin), cell, order, s))) return rc;
    SW_HIP(hipMemsetAsync(d_moved, 0, 8, s));
    hipLaunchKernelGGL(k_compose, grid, dim3(kBlock), 0, s, order, inv, n, from, perm_out, d_moved);
    SW_LAUNCHED();
    unsigned long long *h = static_cast<unsigned long long *>(pinned(ctx, 64));
    if (!h) return SWARM_ERR_OOM;
    SW_HIP(hipMemcpyAsync(h, d_moved, 8, hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    *moved = int64_t(h[0]);
    return SWARM_OK;
}

}  // extern "C"
