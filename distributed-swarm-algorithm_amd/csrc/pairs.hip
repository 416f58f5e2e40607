// The two-hop index of a symmetric int32 CSR, for the election's pair rounds (elect.hip, gather_listed_pair).
//
// An MI355X layout with no reference counterpart: row v of (rp2, col2) holds v's CSR row first, in CSR order,
// then every agent at exactly two hops, each once and never v itself; columns are 16-bit deltas from the row's
// 64-agent base (v & ~63), as swarm_graph_compact's.  Built once per graph version, outside a steady-state
// step, in two passes over the same kernel: count (row lengths; the caller turns them into offsets) and fill.
//
// One wave per agent.  Every agent of the row lies within 32767 slots of the base or the build is refused, so
// the wave keeps one bit per slot of that window in LDS (65 536 bits, 8 KiB): v and its neighbours are set
// first, then each neighbour's row is walked 64 columns per step, and a column whose bit was still clear (one
// LDS atomic OR) is new.  New columns are placed by a ballot prefix.  Lanes that hold the same agent in one
// step are told apart by the atomic: exactly one of them sees the bit clear.
#include <algorithm>

#include "swarm_common.h"

namespace swarm {
namespace {

constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kWindowWords = 65536 / 32;
constexpr unsigned PB_RANGE = 1u;  // a column outside the graph, or more than 32767 slots from its row's base
constexpr unsigned PB_ROW = 2u;    // a row longer than the cap

// FILL = false: counts[v] = the row's length.  FILL = true: the row written at rp2[v] (never past rp2[v + 1]).
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_pairs(const int32_t *__restrict__ rp, const int32_t *__restrict__ col,
                                                  int64_t n, int32_t max_row, int32_t *__restrict__ counts,
                                                  const int32_t *__restrict__ rp2, int16_t *__restrict__ col2,
                                                  unsigned *__restrict__ bad) {
    __shared__ __attribute__((aligned(16))) uint32_t s_bits[kWavesPerBlock][kWindowWords];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t *bits = s_bits[wid];
    uint4 *bits4 = reinterpret_cast<uint4 *>(bits);
    unsigned out = 0;
    for (int64_t v = int64_t(blockIdx.x) * kWavesPerBlock + wid; v < n; v += int64_t(gridDim.x) * kWavesPerBlock) {
        // a refused build stops early (a 100M-agent swarm's deltas do not fit: no pass over all of it)
        if (__hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & PB_RANGE) break;
        for (int i = lane; i < kWindowWords / 4; i += kWave) bits4[i] = make_uint4(0, 0, 0, 0);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const int32_t base = int32_t(v) & ~63;
        const int32_t b = rp[v], e = rp[v + 1];
        const int32_t o = FILL ? rp2[v] : 0, oe = FILL ? rp2[v + 1] : 0;
        // a column's window slot, or -1: slots are 1 .. 65535 (delta + 32768), v's own is 32768 + (v & 63)
        auto window_slot = [&](int32_t w) {
            const int32_t d = w - base;
            return (w >= 0 && w < n && d >= -32767 && d <= 32767) ? d + 32768 : -1;
        };
        if (lane == 0) atomicOr(&bits[(32768 + int(v & 63)) >> 5], 1u << ((32768 + int(v & 63)) & 31));
        for (int32_t k = b + lane; k < e; k += kWave) {  // the neighbours: set, and written in CSR order
            const int32_t sl = window_slot(col[k]);
            if (sl < 0) {
                out |= PB_RANGE;
                continue;
            }
            atomicOr(&bits[sl >> 5], 1u << (sl & 31));
            if (FILL && o + (k - b) < oe) col2[o + (k - b)] = int16_t(sl - 32768);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        int32_t len = e - b;  // wave-uniform
        for (int32_t i = b; i < e; ++i) {
            const int32_t u = col[i];  // one address for the wave
            if (u < 0 || u >= n) continue;  // (flagged above)
            const int32_t ub = rp[u], ue = rp[u + 1];
            for (int32_t k0 = ub; k0 < ue; k0 += kWave) {
                const int32_t k = k0 + lane;
                bool fresh = false;
                int32_t sl = -1;
                if (k < ue) {
                    sl = window_slot(col[k]);
                    if (sl < 0)
                        out |= PB_RANGE;
                    else
                        fresh = !((atomicOr(&bits[sl >> 5], 1u << (sl & 31)) >> (sl & 31)) & 1u);
                }
                const unsigned long long m = __ballot(fresh);
                if (FILL && fresh) {
                    const int32_t pos = o + len + int32_t(__builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32),
                                                          __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u)));
                    if (pos < oe) col2[pos] = int16_t(sl - 32768);
                }
                len += __popcll(m);
            }
        }
        if (len > max_row) out |= PB_ROW;
        if (!FILL && lane == 0) counts[v] = len;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (out) atomicOr(bad, out);
}

int pairs_entry(swarm_ctx *ctx, int64_t n, const int32_t *rp, const int32_t *col, hipStream_t s, int32_t *e_total) {
    SW_ARG(ctx != nullptr, "ctx is NULL");
    if (!ctx_on_current_device(ctx)) return SWARM_ERR_ARG;
    SW_ARG(n > 0 && n < (int64_t(1) << 30), "n out of range (0 < n < 2^30)");
    SW_ARG(rp != nullptr, "row_ptr is NULL");
    SW_HIP(hipMemcpyAsync(e_total, rp + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    SW_ARG(*e_total >= 0, "row_ptr[n] < 0");
    SW_ARG(*e_total == 0 || col != nullptr, "col is NULL but the graph has edges");
    return SWARM_OK;
}

int pairs_verdict(unsigned bad) {
    if (bad & PB_RANGE) {
        set_error("two-hop index: an agent within two hops lies more than 32767 storage slots from its row's "
                  "64-agent base (or a column is outside the graph): run without pair rounds");
        return SWARM_ERR_RANGE;
    }
    if (bad & PB_ROW) {
        set_error("two-hop index: a row is longer than max_row (a hub): run without pair rounds");
        return SWARM_ERR_RANGE;
    }
    return SWARM_OK;
}

void pairs_forget(swarm_ctx *ctx, const void *rp2, const void *col2) {
    auto &v = ctx->pairs_built;
    v.erase(std::remove_if(v.begin(), v.end(),
                           [&](const swarm_ctx::PairsBuilt &p) { return p.rp2 == rp2 || p.col2 == col2; }),
            v.end());
}

}  // namespace
}  // namespace swarm

extern "C" {

int swarm_graph_pairs_count(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col, int32_t max_row,
                            int32_t *counts, void *stream) {
    using namespace swarm;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t e_total = 0;
    if (int rc = pairs_entry(ctx, n, row_ptr, col, s, &e_total)) return rc;
    SW_ARG(counts != nullptr, "counts is NULL");
    SW_ARG(max_row >= 1, "max_row < 1");
    unsigned *bad;
    SW_ALLOC(bad, ctx, S_TMP1, sizeof(unsigned));
    SW_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_pairs<false>, dim3(grid_for(n, kWavesPerBlock, 8192)), dim3(kBlock), 0, s, row_ptr, col, n,
                       max_row, counts, nullptr, nullptr, bad);
    SW_LAUNCHED();
    unsigned hbad = 0;
    SW_HIP(hipMemcpyAsync(&hbad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    return pairs_verdict(hbad);
}

int swarm_graph_pairs_fill(swarm_ctx *ctx, int64_t n, const int32_t *row_ptr, const int32_t *col, const int32_t *rp2,
                           int16_t *col2, void *stream) {
    using namespace swarm;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t e_total = 0;
    if (int rc = pairs_entry(ctx, n, row_ptr, col, s, &e_total)) return rc;
    SW_ARG(rp2 != nullptr, "rp2 is NULL");
    pairs_forget(ctx, rp2, col2);
    int32_t ends[2] = {0, 0};  // rp2[0], rp2[n]
    SW_HIP(hipMemcpyAsync(&ends[0], rp2, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SW_HIP(hipMemcpyAsync(&ends[1], rp2 + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    SW_ARG(ends[0] == 0 && ends[1] >= e_total, "rp2 is not the offsets of swarm_graph_pairs_count's row lengths");
    if (int64_t(ends[1]) >= (int64_t(1) << 31) - (int64_t(1) << 20)) {
        set_error("two-hop index: 2^31 - 2^20 entries or more (32-bit byte offsets): run without pair rounds");
        return SWARM_ERR_RANGE;
    }
    SW_ARG(ends[1] == 0 || col2 != nullptr, "col2 is NULL");
    unsigned *bad;
    SW_ALLOC(bad, ctx, S_TMP1, sizeof(unsigned));
    SW_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_pairs<true>, dim3(grid_for(n, kWavesPerBlock, 8192)), dim3(kBlock), 0, s, row_ptr, col, n,
                       INT32_MAX, nullptr, rp2, col2, bad);
    SW_LAUNCHED();
    unsigned hbad = 0;
    SW_HIP(hipMemcpyAsync(&hbad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    SW_HIP(hipStreamSynchronize(s));
    if (int rc = pairs_verdict(hbad)) return rc;
    ctx->pairs_built.push_back({rp2, col2, row_ptr, col, n});
    return SWARM_OK;
}

}  // extern "C"
