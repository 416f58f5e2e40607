// The lossy channel of the radio and task update loops (contract U1-L): whether the link from
// sender `sid` to receiver `rid` is dropped at absolute tick t.  A pure function of (seed, t, sid, rid) on
// agent IDs, not storage indices: no per-agent state, the same verdict in every layout, in every kernel of
// the tick and on the host (swarm_link_dropped), and a chunked run is the same run.  Two rounds of
// jitter_u's finaliser (splitmix64's), the sender and the tick mixed in first, then the receiver, so that
// j -> i and i -> j are decided independently.
#pragma once
#include <cstdint>

namespace swarm {

__host__ __device__ __forceinline__ uint64_t link_fin(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// The link's uniform draw in [0, 1): 53 bits.
__host__ __device__ __forceinline__ double link_u(uint64_t seed, int64_t t, int32_t sid, int32_t rid) {
    const uint64_t a = link_fin(seed ^ (uint64_t(uint32_t(sid)) * 0x9E3779B97F4A7C15ull) ^
                                (uint64_t(t) * 0xD1B54A32D192ED03ull));
    const uint64_t b = link_fin(a ^ (uint64_t(uint32_t(rid)) * 0x9E3779B97F4A7C15ull));
    return double(b >> 11) * (1.0 / 9007199254740992.0);
}

// loss == 0 drops nothing, loss == 1 everything (u < 1 always).
__host__ __device__ __forceinline__ bool link_dropped(uint64_t seed, int64_t t, int32_t sid, int32_t rid,
                                                      double loss) {
    return link_u(seed, t, sid, rid) < loss;
}

// The channel as the window kernels of protocol.hip take it: their last parameter, its type their template
// parameter.  The link j -> i of tick t is dropped iff dropped(t, ids[j], ids[i]), and a dropped link delivers
// nothing of j's tick t-1 sends.  NoLoss is empty and what `if constexpr (Ch::kLossy)` guards is not compiled
// for it, so k_*<NoLoss> has the instructions of a kernel written without a channel (kernel-argument offsets
// aside; tools/asm_compare.py).  The tick stays the kernels' own argument, not a field of Lossy: the lossy
// instantiations depend on that for their registers.
struct NoLoss {
    static constexpr bool kLossy = false;
};
struct Lossy {
    static constexpr bool kLossy = true;
    double loss;
    uint64_t seed;
    // the tick's kShards x 4 link counters: [0] the election links (alive receiver, in-range sender with an
    // ACCLAIM or a HEARTBEAT), [1] those of them that were dropped
    unsigned long long *cnt;
    __device__ bool dropped(int64_t t, int32_t sid, int32_t rid) const {
        return link_dropped(seed, t, sid, rid, loss);
    }
};

}  // namespace swarm
