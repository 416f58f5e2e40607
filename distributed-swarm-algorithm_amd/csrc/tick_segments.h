// The shape of k_tick's launch (protocol.hip) and of its sender segments: pure host arithmetic, no HIP
// includes, so that a plain host program can drive it (tests/tick_segments/tick_segments_main.cpp deals
// k_tick's units to its workgroups and proves that no segment overflows).
#pragma once

#include <algorithm>
#include <cstdint>

namespace swarm {

constexpr int kTickBlock = 256;  // threads per workgroup of k_tick (kBlock)
#ifndef SWARM_SWEEP_V            // A/B aid: agents per sweep thread (4 or 8)
#define SWARM_SWEEP_V 4
#endif
constexpr int kSweepV = SWARM_SWEEP_V;
static_assert(kSweepV == 4 || kSweepV == 8, "sweep: 4 or 8 agents per thread");
constexpr int kRecvChunk = 4096;  // agents per receive-role pass (64 mail words, 16 agents per thread;
                                  // 2 048: 0.144 vs 0.138 ms per tick)

// k_tick's grid and the capacities of its workgroups' sender segments (entries: agent indices).  A workgroup
// lists at most the agents it is dealt: the g_recv receive-role workgroups their 4 096-agent chunks (rcap
// each), the sweep-role ones their kSweepV-agent groups, or -- on a pulled tick, when every workgroup
// receives -- their 1 024-agent units (scap each).
struct TickShape {
    int g_recv;      // receive-role workgroups (the first of the grid)
    unsigned tgrid;  // both roles: g_recv + the sweep grid
    int xg;          // chunks per group of the XCD-grouped order, 0 = plain grid stride
    int64_t rcap, scap;
    int64_t seg_total;  // g_recv * rcap + sweep grid * scap
};

// n agents, `grid` sweep-role workgroups; recv_wgs > 0 overrides the receive role's share (SWARM_FSM_RECV_WGS),
// xcd_group > 0 asks for the XCD-grouped chunk order (SWARM_TICK_XCD_GROUP).
static inline TickShape tick_shape(int64_t n, unsigned grid, int recv_wgs, int xcd_group) {
    TickShape t{};
    // the receive role: a workgroup per 4 096-agent chunk, at most half the sweep grid (10M agents: 1 280 of
    // 2 442 chunks' workgroups; two-launch form, sweep grid 2 048: 1 280 -> 0.1279 ms per tick, 1 536 ->
    // 0.1281, 2 048 -> 0.1298, 1 024 -> 0.1303; sweep grid 4 096: 2 048 -> 0.138, 512 -> 0.160, 256 -> 0.214)
    const int64_t ngroups = (n + kSweepV - 1) / kSweepV;
    const int64_t nchunks = (n + kRecvChunk - 1) / kRecvChunk;
    t.g_recv = int(std::max<int64_t>(
        1, std::min<int64_t>(nchunks, recv_wgs > 0 ? recv_wgs : std::max<int64_t>(1, int64_t(grid) / 2))));
    t.tgrid = grid + unsigned(t.g_recv);
    // the grouped order only when both role grids split evenly over the 8 XCDs
    t.xg = (xcd_group > 0 && t.g_recv % 8 == 0 && t.tgrid % 8 == 0) ? xcd_group : 0;
    // a grid-stride share of kSweepV-agent groups, or of 4 096-agent chunks
    t.rcap = (nchunks + t.g_recv - 1) / t.g_recv * kRecvChunk;
    const int64_t sweep_threads = int64_t(grid) * kTickBlock;
    t.scap = std::max((ngroups + sweep_threads - 1) / sweep_threads * kTickBlock * kSweepV,
                      (nchunks + t.tgrid - 1) / t.tgrid * kRecvChunk);
    if (t.xg) {  // the grouped order may deal a workgroup more chunks than the grid stride: its segment holds them
        auto most = [](int64_t nch, int64_t g, int64_t nrole) {  // max chunks of one workgroup
            const int64_t ngr = (nch + g - 1) / g;
            int64_t worst = 0;
            for (int64_t x = 0; x < 8; ++x) {
                const int64_t full = ngr > x ? (ngr - 1 - x) / 8 + 1 : 0;  // groups of XCD x
                int64_t cx = full * g;
                if (full && (x + 8 * (full - 1)) == ngr - 1) cx -= ngr * g - nch;  // its last group is partial
                worst = std::max(worst, (cx + nrole / 8 - 1) / (nrole / 8));
            }
            return worst;
        };
        t.rcap = std::max(t.rcap, most(nchunks, t.xg, t.g_recv) * kRecvChunk);
        const int64_t unit = kRecvChunk / 4, nunits = (n + unit - 1) / unit;
        t.scap = std::max(t.scap, most(nunits, 4 * int64_t(t.xg), t.tgrid) * unit);
        t.rcap = std::max(t.rcap, t.scap);  // a pulled tick: the receive-role workgroups too
    }
    t.seg_total = int64_t(t.g_recv) * t.rcap + int64_t(grid) * t.scap;
    return t;
}

}  // namespace swarm
