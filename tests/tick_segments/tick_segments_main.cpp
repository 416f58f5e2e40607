// Drives csrc/tick_segments.h on the host (no HIP): a workgroup of k_tick (protocol.hip) lists the senders
// among the agents it is dealt in its own segment, so tick_shape's capacities must hold whatever one
// workgroup can be dealt, and the segments must not overlap.  The dealing is restated here on its own, from
// the kernel's description rather than its loops:
//   receive role  workgroups 0 .. g_recv - 1 share the 4 096-agent chunks;
//   sweep role    the other `grid` workgroups share the kSweepV-agent groups, a group per thread and pass;
//   pulled tick   all g_recv + grid workgroups share 1 024-agent units instead.
// Units are shared by plain stride (unit u to workgroup u % nrole), or in the XCD-grouped order: groups of
// gsz consecutive units go round robin to the 8 XCDs, and an XCD's units, in order, round robin to its
// nrole / 8 workgroups (workgroup w runs on XCD w % 8).
// Built and run by tests/test_tick_segments.py (g++ -I<csrc>); exit status = failed cases.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tick_segments.h"

using swarm::kRecvChunk;
using swarm::kSweepV;
using swarm::kTickBlock;
using swarm::TickShape;

static int failed = 0, cases = 0, grouped = 0;

// Agents dealt to each of nrole workgroups from units of `unit` agents; gsz > 0: the XCD-grouped order.
// Returns false when a unit is dealt twice or not at all.
static bool deal_units(int64_t n, int64_t unit, int64_t nrole, int64_t gsz, std::vector<int64_t> &dealt) {
    const int64_t nunits = (n + unit - 1) / unit;
    std::vector<int> seen(size_t(nunits), 0);
    dealt.assign(size_t(nrole), 0);
    auto give = [&](int64_t u, int64_t w) {
        ++seen[size_t(u)];
        dealt[size_t(w)] += std::min(unit, n - u * unit);
    };
    if (!gsz) {
        for (int64_t u = 0; u < nunits; ++u) give(u, u % nrole);
    } else {
        const int64_t per_xcd = nrole / 8;
        for (int64_t x = 0; x < 8; ++x) {
            int64_t slot = 0;  // the XCD's units in order, the missing ones of a last partial group included
            for (int64_t g = x; g * gsz < nunits; g += 8)
                for (int64_t k = 0; k < gsz; ++k, ++slot)
                    if (g * gsz + k < nunits) give(g * gsz + k, x + 8 * (slot % per_xcd));
        }
    }
    for (int c : seen)
        if (c != 1) return false;
    return true;
}

static void check(int64_t n, unsigned grid, int recv_wgs, int xcd_group) {
    const TickShape t = swarm::tick_shape(n, grid, recv_wgs, xcd_group);
    ++cases;
    grouped += t.xg != 0;
    char name[96];
    std::snprintf(name, sizeof(name), "n=%lld grid=%u recv=%d xg=%d", (long long)n, grid, recv_wgs, xcd_group);
    auto fail = [&](const char *what, int64_t w, int64_t got, int64_t cap) {
        std::printf("FAIL %s: %s (workgroup %lld: %lld agents, capacity %lld)\n", name, what, (long long)w,
                    (long long)got, (long long)cap);
        ++failed;
    };
    if (t.g_recv < 1 || t.tgrid != grid + unsigned(t.g_recv)) return fail("grid", 0, t.g_recv, t.tgrid);
    if (t.xg && (t.g_recv % 8 || t.tgrid % 8)) return fail("grouped order on an uneven grid", 0, t.g_recv, t.tgrid);
    // segment b: [at(b), at(b) + cap(b)), the receive-role ones first; in order, so disjoint iff none runs
    // past the start of the next and the last ends within the total
    auto cap = [&](int64_t b) { return b < t.g_recv ? t.rcap : t.scap; };
    auto at = [&](int64_t b) {
        return b < t.g_recv ? b * t.rcap : int64_t(t.g_recv) * t.rcap + (b - t.g_recv) * t.scap;
    };
    for (int64_t b = 0; b < int64_t(t.tgrid); ++b) {
        const int64_t next = b + 1 < int64_t(t.tgrid) ? at(b + 1) : t.seg_total;
        if (cap(b) < 0 || at(b) + cap(b) > next) return fail("segments overlap", b, at(b) + cap(b), next);
    }
    std::vector<int64_t> dealt;
    // a tick that is not pulled: the receive role's chunks ...
    if (!deal_units(n, kRecvChunk, t.g_recv, t.xg, dealt))
        return fail("receive role: chunks not dealt once", 0, 0, 0);
    for (int64_t w = 0; w < t.g_recv; ++w)
        if (dealt[size_t(w)] > t.rcap) return fail("receive role", w, dealt[size_t(w)], t.rcap);
    // ... and the sweep role's groups: pass p gives workgroup r the groups (p * grid + r) * 256 .. + 255
    const int64_t ngroups = (n + kSweepV - 1) / kSweepV;
    int64_t swept = 0;
    for (int64_t r = 0; r < int64_t(grid); ++r) {
        int64_t mine = 0;
        for (int64_t g0 = r * kTickBlock; g0 < ngroups; g0 += int64_t(grid) * kTickBlock)
            mine += std::min(n, (g0 + kTickBlock) * kSweepV) - g0 * kSweepV;
        if (mine > t.scap) return fail("sweep role", t.g_recv + r, mine, t.scap);
        swept += mine;
    }
    if (swept != n) return fail("sweep role: agents not dealt once", 0, swept, n);
    // a pulled tick: every workgroup, 1 024-agent units, groups of 4 xg units
    if (!deal_units(n, kRecvChunk / 4, t.tgrid, 4 * int64_t(t.xg), dealt))
        return fail("pulled tick: units not dealt once", 0, 0, 0);
    for (int64_t w = 0; w < int64_t(t.tgrid); ++w)
        if (dealt[size_t(w)] > cap(w)) return fail("pulled tick", w, dealt[size_t(w)], cap(w));
}

int main() {
    for (int xg : {0, 1, 2, 3, 5}) {
        std::vector<int64_t> ns = {1, 3, 4095, 4096, 4097, 32767, 1000003};
        if (xg) {
            ns.push_back(32768 * int64_t(xg) - 1);
            ns.push_back(32768 * int64_t(xg) + 1);
        }
        for (int64_t n : ns)
            for (unsigned grid : {1u, 8u, 16u, 2560u})
                for (int recv : {0, 1, 8, 1280}) check(n, grid, recv, xg);
    }
    std::printf("%d cases, %d in the grouped order\n%d failed\n", cases, grouped, failed);
    return failed;
}
