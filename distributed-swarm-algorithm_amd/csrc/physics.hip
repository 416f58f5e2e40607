// Physics / formation step on gfx950.
//
// Replaces SwarmAgent._update_physics (agent.py:94-181) run by every agent of the swarm, as one
// synchronous step (contract P1, tools/gen_golden.py): every agent reads the step-start snapshot
// of all positions (pos_in) and writes its new position to pos_out (double-buffered), so the
// result does not depend on the order agents are updated in.
//   formation  a FOLLOWER with a leader targets its V slot behind the leader's position as the
//              heartbeat carries it ('!ff': f32-rounded, agent.py:256-258, 283-289):
//              x - 2 id, y + 2 id (even id) / y - 2 id (odd id)  (agent.py:96-111)
//   forces     attraction to the target beyond 0.5 (118-125); obstacle repulsion, obstacles in
//              list order (128-146); neighbour separation within 2.0, neighbours in CSR order
//              (149-160) -- sums in the reference's order, so the result is bit-exact against
//              the CPU restatement's x*x arithmetic (the reference squares with libm pow: <= 1
//              ulp per square, checked with a tolerance against its fixtures)
//   update     speed clamp to max_speed (169-174), Euler step (177-178).
// One thread per agent (fp64 VALU + the neighbour gathers; the snapshot of the neighbourhood is
// the HBM traffic: 16 B per edge + 80 B per agent); obstacles staged in LDS per workgroup.
// A zero distance to an obstacle centre or a neighbour makes the reference raise
// ZeroDivisionError; here it yields non-finite values and is counted (n_singular).
//
// swarm_physics_run_sensed runs several such steps and senses each step's neighbours from that
// step's positions (contract S1; the reference's simulator refreshes the neighbour lists before
// every tick): per step the agents are binned and one fused kernel reads the 3 x 3 cell windows
// directly -- no degree pass, no scan, no CSR in memory.
#include <cmath>

#include <cstdarg>

#include "binning.h"
#include "fsm_records.h"
#include "window_merge.h"

namespace swarm {
namespace {

constexpr int kObsLds = 1024;  // obstacles staged in LDS per pass (3 doubles each)
#ifndef SWARM_PHYS_NB
#define SWARM_PHYS_NB 6
#endif
constexpr int kNb = SWARM_PHYS_NB;  // neighbour positions in flight per thread (6: 0.869-0.879 ms, 4: 0.898, 8: 0.92; r5 physics_nb_ab.log)

// Correctly rounded f64 division and square root, written out as LLVM expands them for gfx950 but
// without their range steps (div_scale / div_fmas scaling / div_fixup; the ldexp pre-scale and class
// test of sqrt), which are the identity when every operand and result is normal and far from the
// exponent limits -- in_range() below, checked by the caller, who falls back to '/' and sqrt()
// otherwise.  Same instructions on the same operands: the same bits.  (Round 5: the separation
// terms' three divisions and square root were ~60 % of k_physics' fp64 instructions; two divisions
// by the same norm share its refined reciprocal.)
#ifndef SWARM_PHYS_LIBM
#define SWARM_PHYS_LIBM 0  // 1: the library '/' and sqrt() everywhere (A/B builds)
#endif
__device__ __forceinline__ bool in_range(double x) {
    const double a = fabs(x);
    return a >= 0x1p-500 && a <= 0x1p500;  // (false for 0, denormals, inf, NaN)
}
__device__ __forceinline__ double rcp_refined(double den) {  // v_rcp_f64 + two Newton steps
    double r = __builtin_amdgcn_rcp(den);
    double e = __builtin_fma(-den, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-den, r, 1.0);
    return __builtin_fma(r, e, r);
}
__device__ __forceinline__ double div_by(double num, double den, double r) {  // num / den, r = rcp_refined(den)
    const double q = num * r;
    const double rem = __builtin_fma(-den, q, num);
    return __builtin_fma(rem, r, q);
}
__device__ __forceinline__ double sqrt_core(double x) {  // v_rsq_f64 + Newton steps on (g, h)
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}

// The pieces of one agent's step as functions.  separation_term is shared by k_physics (neighbours from
// a CSR) and k_physics_sensed (neighbours from the step's own cell windows): the same code, hence the same
// bits.  The others restate k_physics' statements for k_physics_sensed (see the note at k_physics).

// Formation (agent.py:96-111): a FOLLOWER with a leader retargets its V slot behind the leader's
// f32-rounded position.  Returns whether the agent has a target (moves); t = that target.
__device__ __forceinline__ bool formation_target(int64_t i, const int32_t *__restrict__ ids,
                                                 const uint8_t *__restrict__ state,
                                                 const int32_t *__restrict__ leader,
                                                 const double2 *__restrict__ pin, double2 *__restrict__ tgt,
                                                 uint8_t *__restrict__ has_t, double2 &t) {
    t = tgt[i];
    bool has = has_t[i] != 0;
    const int32_t L = leader[i];
    if (state[i] == SWARM_FOLLOWER && L >= 0) {
        const double2 lp = pin[L];
        const double lx = double(float(lp.x)), ly = double(float(lp.y));
        const double rank = double(ids[i]);
        const double xo = -2.0 * rank;
        const double yo = (ids[i] % 2 == 0) ? 2.0 * rank : -2.0 * rank;
        t = make_double2(lx + xo, ly + yo);
        tgt[i] = t;
        if (!has) has_t[i] = 1;
        has = true;
    }
    return has;
}

// Obstacle repulsion (agent.py:128-146), obstacles in list order: every workgroup stages them through
// LDS (all lanes join the barriers, moving or not).
__device__ __forceinline__ void obstacle_forces(double *s_obs, int64_t m, const double *__restrict__ obs, bool moving,
                                                double px, double py, double &frx, double &fry,
                                                unsigned long long &sing) {
    for (int64_t o0 = 0; o0 < m; o0 += kObsLds) {
        const int64_t cnt = (m - o0 < kObsLds) ? m - o0 : kObsLds;
        __syncthreads();
        for (int64_t q = threadIdx.x; q < 3 * cnt; q += kBlock) s_obs[q] = obs[3 * o0 + q];
        __syncthreads();
        if (moving)
            for (int64_t o = 0; o < cnt; ++o) {
                const double ox = s_obs[3 * o], oy = s_obs[3 * o + 1], r = s_obs[3 * o + 2];
                const double ex = px - ox, ey = py - oy;
                const double s2 = ex * ex + ey * ey;
                // far obstacles (most): sqrt(s2) - r >= 5 for certain, so the exact test below could
                // not apply the force -- skip its square root (the margin 1e-12 is far above the
                // roundings of s2, the square root and the subtraction; NaN falls through)
                const double rr = 5.0 + r;
                if (s2 > rr * rr * (1.0 + 1e-12)) continue;
                double d = sqrt(s2) - r;
                if (d <= 0.001) d = 0.001;
                if (d < 5.0) {
                    const double mag = 50.0 * (1.0 / d - 1.0 / 5.0) / (d * d);
                    const double nrm = sqrt(s2);
                    sing += nrm == 0.0;
                    frx += (ex / nrm) * mag;
                    fry += (ey / nrm) * mag;
                }
            }
    }
}

// One neighbour's separation term (agent.py:149-160) from the offset (ex, ey) to it and
// s2 = ex * ex + ey * ey: added to the running sums when the neighbour is within the 2.0 personal
// space.  The sums travel by value: with reference parameters the compiler arranged k_physics' unrolled
// row loop differently (20 more instructions, 1.4 % slower); this form compiles it as before the lift.
struct SepAcc {
    double x, y;              // separation force so far
    unsigned long long sing;  // zero distances so far
};
__device__ __forceinline__ SepAcc separation_term(double ex, double ey, double s2, SepAcc acc) {
    if (!SWARM_PHYS_LIBM && in_range(ex) && in_range(ey) && in_range(s2)) {
        // both offsets nonzero and normal: the norm is in [2^-500, 2^251), d * d in
        // [1e-6, 4), every quotient normal -- the range steps are the identity
        const double nrm = sqrt_core(s2);
        if (nrm < 2.0) {
            const double d = nrm <= 0.001 ? 0.001 : nrm;
            const double dd = d * d;
            const double mag = div_by(20.0, dd, rcp_refined(dd));
            const double rn = rcp_refined(nrm);
            acc.x += div_by(ex, nrm, rn) * mag;
            acc.y += div_by(ey, nrm, rn) * mag;
        }
        return acc;
    }
    double d = sqrt(s2);
    if (d < 2.0) {
        if (d <= 0.001) d = 0.001;
        const double mag = 20.0 / (d * d);
        const double nrm = sqrt(s2);
        acc.sing += nrm == 0.0;
        acc.x += (ex / nrm) * mag;
        acc.y += (ey / nrm) * mag;
    }
    return acc;
}

// Attraction to the target beyond 0.5 (agent.py:118-125).
__device__ __forceinline__ void attraction(double px, double py, double2 t, double &fax, double &fay) {
    const double gx = t.x - px, gy = t.y - py;
    if (sqrt(gx * gx + gy * gy) > 0.5) {
        fax = 1.0 * gx;
        fay = 1.0 * gy;
    }
}

// The three forces summed, the speed clamp (agent.py:169-174) and the Euler step (177-178).
__device__ __forceinline__ void integrate(int64_t i, double px, double py, double fax, double fay, double frx,
                                          double fry, double fsx, double fsy, double dt, double max_speed,
                                          double2 *__restrict__ vel, double2 *__restrict__ pout) {
    const double f0 = fax + frx + fsx, f1 = fay + fry + fsy;
    const double vmag = sqrt(f0 * f0 + f1 * f1);
    double2 v;
    if (vmag > max_speed) {
        const double scale = max_speed / vmag;
        v = make_double2(f0 * scale, f1 * scale);
    } else {
        v = make_double2(f0, f1);
    }
    vel[i] = v;
    pout[i] = make_double2(px + v.x * dt, py + v.y * dt);
}

__device__ __forceinline__ void count_singular(unsigned long long sing, unsigned long long *__restrict__ singular) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sing += __shfl_xor(sing, off, 64);
    if ((threadIdx.x & 63) == 0 && sing) atomicAdd(singular, sing);
}

// k_physics keeps its body written out and shares only the separation term: routed through the helpers
// above (formation_target, obstacle_forces, attraction, integrate) the compiler laid its blocks out
// differently and the f1 step measured 1-2 % slower; in this form its machine code is what it was.  (Its row
// walk and k_physics_loop's as one function returning a SepAcc: 1 680 / 1 682 instructions for 1 681 / 1 683,
// not the same streams -- both keep the walk written out.)
__global__ __launch_bounds__(kBlock, 8) void k_physics(int64_t n, const int32_t *__restrict__ ids,
                                                   const uint8_t *__restrict__ state,
                                                   const int32_t *__restrict__ leader,
                                                   const double2 *__restrict__ pin, double2 *__restrict__ pout,
                                                   double2 *__restrict__ vel, double2 *__restrict__ tgt,
                                                   uint8_t *__restrict__ has_t, int64_t m,
                                                   const double *__restrict__ obs, const int32_t *__restrict__ rp,
                                                   const int32_t *__restrict__ col, double dt, double max_speed,
                                                   unsigned long long *__restrict__ singular) {
    __shared__ double s_obs[kObsLds * 3];
    unsigned long long sing = 0;
    for (int64_t base = int64_t(blockIdx.x) * kBlock; base < n; base += int64_t(gridDim.x) * kBlock) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < n;
        double px = 0, py = 0, frx = 0.0, fry = 0.0;
        bool moving = false;
        double2 t = make_double2(0, 0);
        if (valid) {
            const double2 p = pin[i];
            px = p.x;
            py = p.y;
            t = tgt[i];
            bool has = has_t[i] != 0;
            const int32_t L = leader[i];
            if (state[i] == SWARM_FOLLOWER && L >= 0) {
                const double2 lp = pin[L];
                const double lx = double(float(lp.x)), ly = double(float(lp.y));
                const double rank = double(ids[i]);
                const double xo = -2.0 * rank;
                const double yo = (ids[i] % 2 == 0) ? 2.0 * rank : -2.0 * rank;
                t = make_double2(lx + xo, ly + yo);
                tgt[i] = t;
                if (!has) has_t[i] = 1;
                has = true;
            }
            moving = has;
        }
        // obstacles: every workgroup stages them through LDS (all lanes join the barriers)
        for (int64_t o0 = 0; o0 < m; o0 += kObsLds) {
            const int64_t cnt = (m - o0 < kObsLds) ? m - o0 : kObsLds;
            __syncthreads();
            for (int64_t q = threadIdx.x; q < 3 * cnt; q += kBlock) s_obs[q] = obs[3 * o0 + q];
            __syncthreads();
            if (moving)
                for (int64_t o = 0; o < cnt; ++o) {
                    const double ox = s_obs[3 * o], oy = s_obs[3 * o + 1], r = s_obs[3 * o + 2];
                    const double ex = px - ox, ey = py - oy;
                    const double s2 = ex * ex + ey * ey;
                    // far obstacles (most): sqrt(s2) - r >= 5 for certain, so the exact test below could
                    // not apply the force -- skip its square root (the margin 1e-12 is far above the
                    // roundings of s2, the square root and the subtraction; NaN falls through)
                    const double rr = 5.0 + r;
                    if (s2 > rr * rr * (1.0 + 1e-12)) continue;
                    double d = sqrt(s2) - r;
                    if (d <= 0.001) d = 0.001;
                    if (d < 5.0) {
                        const double mag = 50.0 * (1.0 / d - 1.0 / 5.0) / (d * d);
                        const double nrm = sqrt(s2);
                        sing += nrm == 0.0;
                        frx += (ex / nrm) * mag;
                        fry += (ey / nrm) * mag;
                    }
                }
        }
        if (!moving) {  // keeps its position (in the output buffer too: synchronous step)
            if (valid) pout[i] = make_double2(px, py);
            continue;
        }
        double fax = 0.0, fay = 0.0;
        const double gx = t.x - px, gy = t.y - py;
        if (sqrt(gx * gx + gy * gy) > 0.5) {
            fax = 1.0 * gx;
            fay = 1.0 * gy;
        }
        double fsx = 0.0, fsy = 0.0;
        // the row in chunks of kNb: all column loads, then all position gathers in flight, then
        // the separation terms summed in CSR order (the reference's order: bit-exact)
        for (int32_t k0 = rp[i], e = rp[i + 1]; k0 < e; k0 += kNb) {
            int32_t jj[kNb];
#pragma unroll
            for (int u = 0; u < kNb; ++u) jj[u] = k0 + u < e ? col[k0 + u] : -1;
            double2 qq[kNb];
#pragma unroll
            for (int u = 0; u < kNb; ++u) qq[u] = jj[u] >= 0 ? pin[jj[u]] : make_double2(0.0, 0.0);
#pragma unroll
            for (int u = 0; u < kNb; ++u) {
                if (jj[u] < 0) continue;
                const double ex = px - qq[u].x, ey = py - qq[u].y;
                const SepAcc r = separation_term(ex, ey, ex * ex + ey * ey, SepAcc{fsx, fsy, sing});
                fsx = r.x;
                fsy = r.y;
                sing = r.sing;
            }
        }
        const double f0 = fax + frx + fsx, f1 = fay + fry + fsy;
        const double vmag = sqrt(f0 * f0 + f1 * f1);
        double2 v;
        if (vmag > max_speed) {
            const double scale = max_speed / vmag;
            v = make_double2(f0 * scale, f1 * scale);
        } else {
            v = make_double2(f0, f1);
        }
        vel[i] = v;
        pout[i] = make_double2(px + v.x * dt, py + v.y * dt);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sing += __shfl_xor(sing, off, 64);
    if ((threadIdx.x & 63) == 0 && sing) atomicAdd(singular, sing);
}

// ---- the coupled update loop's step (contract U1): _update_physics with the agent's own FSM state ----
//
// k_physics for a tick of swarm_update_loop, run after the tick's FSM kernel on the run's records
// (fsm_records.h) instead of state / leader_index arrays: an alive FOLLOWER whose record has kHL targets the
// V slot behind its OWN last-heard leader position (LRec: the '!ff' payload as the heartbeat delivered it,
// up to ten ticks old, from whichever neighbour it accepted last) -- no gather of a leader's row; any other
// alive agent (ELECTION_WAIT, a new LEADER, a FOLLOWER that has not heard a position) keeps the target it
// had.  A dead agent's position is copied through and nothing else of it is written.  The forces are the
// helpers' above in k_physics' order, the neighbour row walked as k_physics walks it: the same bits.

// Formation for agent i from its records.  Returns whether the agent moves; t = its target.
__device__ __forceinline__ bool formation_target_loop(int64_t i, const int32_t *__restrict__ ids, uint32_t fw,
                                                      const LRec *__restrict__ lrec, double2 *__restrict__ tgt,
                                                      uint8_t *__restrict__ has_t, double2 &t) {
    if (!fw_alive(fw)) return false;
    t = tgt[i];
    bool has = has_t[i] != 0;
    if (fw_state(fw) == SWARM_FOLLOWER && (fw_bits(fw) & kHL)) {
        const float2 lp = *reinterpret_cast<const float2 *>(&lrec[i].x);
        const double lx = double(lp.x), ly = double(lp.y);
        const double rank = double(ids[i]);
        const double xo = -2.0 * rank;
        const double yo = (ids[i] % 2 == 0) ? 2.0 * rank : -2.0 * rank;
        t = make_double2(lx + xo, ly + yo);
        tgt[i] = t;
        if (!has) has_t[i] = 1;
        has = true;
    }
    return has;
}

__global__ __launch_bounds__(kBlock, 8) void k_physics_loop(
    int64_t n, const int32_t *__restrict__ ids, const uint2 *__restrict__ rec, const LRec *__restrict__ lrec,
    const double2 *__restrict__ pin, double2 *__restrict__ pout, double2 *__restrict__ vel,
    double2 *__restrict__ tgt, uint8_t *__restrict__ has_t, int64_t m, const double *__restrict__ obs,
    const int32_t *__restrict__ rp, const int32_t *__restrict__ col, double dt, double max_speed,
    unsigned long long *__restrict__ singular) {
    __shared__ double s_obs[kObsLds * 3];
    unsigned long long sing = 0;
    for (int64_t base = int64_t(blockIdx.x) * kBlock; base < n; base += int64_t(gridDim.x) * kBlock) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < n;
        double px = 0, py = 0, frx = 0.0, fry = 0.0;
        bool moving = false;
        double2 t = make_double2(0, 0);
        if (valid) {
            const double2 p = pin[i];
            px = p.x;
            py = p.y;
            moving = formation_target_loop(i, ids, rec[i].x, lrec, tgt, has_t, t);
        }
        obstacle_forces(s_obs, m, obs, moving, px, py, frx, fry, sing);
        if (!moving) {  // dead or without a target: its position in the output buffer too
            if (valid) pout[i] = make_double2(px, py);
            continue;
        }
        double fax = 0.0, fay = 0.0;
        attraction(px, py, t, fax, fay);
        double fsx = 0.0, fsy = 0.0;
        // the row in chunks of kNb, as k_physics: column loads, position gathers in flight, terms in CSR order
        for (int32_t k0 = rp[i], e = rp[i + 1]; k0 < e; k0 += kNb) {
            int32_t jj[kNb];
#pragma unroll
            for (int u = 0; u < kNb; ++u) jj[u] = k0 + u < e ? col[k0 + u] : -1;
            double2 qq[kNb];
#pragma unroll
            for (int u = 0; u < kNb; ++u) qq[u] = jj[u] >= 0 ? pin[jj[u]] : make_double2(0.0, 0.0);
#pragma unroll
            for (int u = 0; u < kNb; ++u) {
                if (jj[u] < 0) continue;
                const double ex = px - qq[u].x, ey = py - qq[u].y;
                const SepAcc r = separation_term(ex, ey, ex * ex + ey * ey, SepAcc{fsx, fsy, sing});
                fsx = r.x;
                fsy = r.y;
                sing = r.sing;
            }
        }
        integrate(i, px, py, fax, fay, frx, fry, fsx, fsy, dt, max_speed, vel, pout);
    }
    count_singular(sing, singular);
}

// ---- sensed step (contract S1): the neighbours of a step are sensed from that step's positions ----
//
// k_physics with the CSR replaced by the agent's 3 x 3 cell window of the step's binning (binning.h):
// agent i senses j != i iff dx * dx + dy * dy <= r2 (swarm_build_rgg's rule) and applies the sensed
// neighbours in ascending storage index (a swarm_build_rgg row's order).  A window is up to nine runs
// of sorted_idx, one per cell, each ascending (the sort is stable): a streaming nine-way merge -- nine
// cursors and nine head indices in registers, the smallest head taken each turn -- visits the
// candidates in ascending index with no list, no capacity and no fallback.  Threads are mapped in
// cell-sorted order over a cell-sorted copy of the positions (psort[q] = pin[sorted_idx[q]]), so a
// wave's lanes walk the same windows and a candidate's position is read at its cursor, next to its
// index, not gathered.  Cells of side >= min(R, 2) (1 + 1e-9) suffice: a neighbour farther than 2.0
// adds no term.  A non-finite agent sits in an edge cell (cell_coord), fails every <= and so senses
// nobody and is sensed by nobody.  st[0] != 0 (a step refused for its window work): the step only
// copies the positions through.  (kMergeEnd, window_merge.h: the head of an exhausted run.)

__global__ __launch_bounds__(kBlock) void k_sorted_positions(const double2 *__restrict__ pin, int64_t n,
                                                            const int32_t *__restrict__ sorted_idx,
                                                            double2 *__restrict__ psort) {
    for (int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x; q < n; q += int64_t(gridDim.x) * kBlock)
        psort[q] = pin[sorted_idx[q]];
}

// st[0]: 0, or 1 + the first step whose window work exceeds swarm_build_rgg's limits (every later step
// is then a no-op); st[2], st[3]: that step's candidate pairs (a double's bits) and largest window.
__global__ void k_sense_verdict(const double *__restrict__ acc, unsigned long long *__restrict__ st, int32_t step) {
    if (st[0] != 0) return;
    const unsigned long long *u = reinterpret_cast<const unsigned long long *>(acc);
    if (window_work_exceeded(acc[0], u[1])) {
        st[2] = u[0];
        st[3] = u[1];
        st[0] = 1ull + unsigned(step);
    }
}

__global__ __launch_bounds__(kBlock) void k_physics_sensed(
    int64_t n, const int32_t *__restrict__ ids, const uint8_t *__restrict__ state, const int32_t *__restrict__ leader,
    const double2 *__restrict__ pin, double2 *__restrict__ pout, double2 *__restrict__ vel, double2 *__restrict__ tgt,
    uint8_t *__restrict__ has_t, int64_t m, const double *__restrict__ obs, Grid g, double r2,
    const int32_t *__restrict__ sorted_idx, const uint32_t *__restrict__ off, const double2 *__restrict__ psort,
    double dt, double max_speed, unsigned long long *__restrict__ st) {
    __shared__ double s_obs[kObsLds * 3];
    const bool stopped = st[0] != 0;  // uniform over the grid: written by an earlier kernel of the stream
    unsigned long long sing = 0;
    for (int64_t base = int64_t(blockIdx.x) * kBlock; base < n; base += int64_t(gridDim.x) * kBlock) {
        const int64_t q0 = base + threadIdx.x;
        const bool valid = q0 < n;
        if (stopped) {
            if (valid) pout[q0] = pin[q0];
            continue;
        }
        int64_t i = 0;
        double px = 0, py = 0, frx = 0.0, fry = 0.0;
        bool moving = false;
        double2 t = make_double2(0, 0);
        if (valid) {
            i = sorted_idx[q0];
            const double2 p = psort[q0];
            px = p.x;
            py = p.y;
            moving = formation_target(i, ids, state, leader, pin, tgt, has_t, t);
        }
        obstacle_forces(s_obs, m, obs, moving, px, py, frx, fry, sing);
        if (!moving) {
            if (valid) pout[i] = make_double2(px, py);
            continue;
        }
        // the nine cells of the window: cursor, end and head index of each run (an absent cell: empty)
        const int64_t cx = cell_coord(px, g.xmin, g.inv_cell, g.ncx);
        const int64_t cy = cell_coord(py, g.ymin, g.inv_cell, g.ncy);
        uint32_t cur[9], end[9];
        int32_t head[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int64_t yy = cy + (k / 3) - 1, xx = cx + (k % 3) - 1;
            const bool in = yy >= 0 && yy < g.ncy && xx >= 0 && xx < g.ncx;
            const int64_t c = in ? yy * g.ncx + xx : 0;
            cur[k] = in ? off[c] : 0u;
            end[k] = in ? off[c + 1] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) head[k] = cur[k] < end[k] ? sorted_idx[cur[k]] : kMergeEnd;
        double fax = 0.0, fay = 0.0;
        attraction(px, py, t, fax, fay);
        double fsx = 0.0, fsy = 0.0;
        for (;;) {
            int32_t j = head[0];
#pragma unroll
            for (int k = 1; k < 9; ++k) j = head[k] < j ? head[k] : j;
            if (j == kMergeEnd) break;
            uint32_t q = 0, e = 0;  // the run that holds j (indices are distinct: exactly one)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const bool hit = head[k] == j;
                q = hit ? cur[k] : q;
                e = hit ? end[k] : e;
            }
            const double2 o = psort[q];
            const uint32_t qn = q + 1;
            const int32_t hn = qn < e ? sorted_idx[qn] : kMergeEnd;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const bool hit = head[k] == j;
                cur[k] = hit ? qn : cur[k];
                head[k] = hit ? hn : head[k];
            }
            if (j == int32_t(i)) continue;
            const double ex = px - o.x, ey = py - o.y;
            const double s2 = ex * ex + ey * ey;
            if (s2 <= r2) {
                const SepAcc r = separation_term(ex, ey, s2, SepAcc{fsx, fsy, sing});
                fsx = r.x;
                fsy = r.y;
                sing = r.sing;
            }
        }
        integrate(i, px, py, fax, fay, frx, fry, fsx, fsy, dt, max_speed, vel, pout);
    }
    count_singular(sing, st + 1);
}

// ---- the sensed loop's step (contract U1-S): k_physics_loop's agent, k_physics_sensed's neighbours ----
//
// k_physics_sensed's nine-way merge as a function: the separation force on agent i at (px, py) from its
// 3 x 3 cell window, the sensed neighbours (s2 <= r2) applied in ascending storage index.  The same
// statements on the same operands, hence the same bits.  (k_physics_sensed keeps its body written out:
// routed through this function, whole or split into the window's opening and its merge, the compiler
// scheduled it differently -- 1 155 / 1 160 instructions for 1 165 -- and S1's figures were measured on
// the form it has.  This function through window_merge (window_merge.h) with a visiting lambda was compiled
// too: k_physics_loop_sensed 1 141 instructions for 1 169, so it keeps the statements as well.)
__device__ __forceinline__ SepAcc window_separation(int64_t i, double px, double py, const Grid &g, double r2,
                                                    const int32_t *__restrict__ sorted_idx,
                                                    const uint32_t *__restrict__ off,
                                                    const double2 *__restrict__ psort, unsigned long long sing) {
    const int64_t cx = cell_coord(px, g.xmin, g.inv_cell, g.ncx);
    const int64_t cy = cell_coord(py, g.ymin, g.inv_cell, g.ncy);
    uint32_t cur[9], end[9];
    int32_t head[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int64_t yy = cy + (k / 3) - 1, xx = cx + (k % 3) - 1;
        const bool in = yy >= 0 && yy < g.ncy && xx >= 0 && xx < g.ncx;
        const int64_t c = in ? yy * g.ncx + xx : 0;
        cur[k] = in ? off[c] : 0u;
        end[k] = in ? off[c + 1] : 0u;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) head[k] = cur[k] < end[k] ? sorted_idx[cur[k]] : kMergeEnd;
    double fsx = 0.0, fsy = 0.0;
    for (;;) {
        int32_t j = head[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) j = head[k] < j ? head[k] : j;
        if (j == kMergeEnd) break;
        uint32_t q = 0, e = 0;  // the run that holds j (indices are distinct: exactly one)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const bool hit = head[k] == j;
            q = hit ? cur[k] : q;
            e = hit ? end[k] : e;
        }
        const double2 o = psort[q];
        const uint32_t qn = q + 1;
        const int32_t hn = qn < e ? sorted_idx[qn] : kMergeEnd;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const bool hit = head[k] == j;
            cur[k] = hit ? qn : cur[k];
            head[k] = hit ? hn : head[k];
        }
        if (j == int32_t(i)) continue;
        const double ex = px - o.x, ey = py - o.y;
        const double s2 = ex * ex + ey * ey;
        if (s2 <= r2) {
            const SepAcc r = separation_term(ex, ey, s2, SepAcc{fsx, fsy, sing});
            fsx = r.x;
            fsy = r.y;
            sing = r.sing;
        }
    }
    return SepAcc{fsx, fsy, sing};
}

// A tick's physics of swarm_update_loop_sensed, after the tick's FSM kernel: k_physics_sensed's thread
// mapping (cell-sorted order over the cell-sorted copy of the snapshot) with the agent's state taken from
// the run's records as k_physics_loop takes it -- the flag word of the 8-byte record, a follower's leader
// position from its own LRec.  A dead agent's position is copied through and nothing else of it is written;
// it is still binned, so the others sense it as a body at rest.  st[0] != 0 (a tick refused for its window
// work): nothing is read or written -- the call is all or nothing and its caller restores the state.
// Occupancy: the obstacles' 24 KiB of LDS admit six workgroups a CU, six waves a SIMD, which 80 VGPRs would
// fill; the merge's 27 cursor registers and the fp64 temporaries take 93, and bounded to six waves
// (__launch_bounds__(kBlock, 6)) the compiler spills ten registers to 44 bytes of scratch a lane -- so, as
// k_physics_sensed, no occupancy bound: 93 VGPRs, five waves a SIMD, no scratch (the bounded form
// was compiled, not timed).
__global__ __launch_bounds__(kBlock) void k_physics_loop_sensed(
    int64_t n, const int32_t *__restrict__ ids, const uint2 *__restrict__ rec, const LRec *__restrict__ lrec,
    double2 *__restrict__ pout, double2 *__restrict__ vel, double2 *__restrict__ tgt, uint8_t *__restrict__ has_t,
    int64_t m, const double *__restrict__ obs, Grid g, double r2, const int32_t *__restrict__ sorted_idx,
    const uint32_t *__restrict__ off, const double2 *__restrict__ psort, double dt, double max_speed,
    const unsigned long long *__restrict__ st, unsigned long long *__restrict__ singular) {
    __shared__ double s_obs[kObsLds * 3];
    if (st[0] != 0) return;  // uniform over the grid: written by an earlier kernel of the stream
    unsigned long long sing = 0;
    for (int64_t base = int64_t(blockIdx.x) * kBlock; base < n; base += int64_t(gridDim.x) * kBlock) {
        const int64_t q0 = base + threadIdx.x;
        const bool valid = q0 < n;
        int64_t i = 0;
        double px = 0, py = 0, frx = 0.0, fry = 0.0;
        bool moving = false;
        double2 t = make_double2(0, 0);
        if (valid) {
            i = sorted_idx[q0];
            const double2 p = psort[q0];
            px = p.x;
            py = p.y;
            moving = formation_target_loop(i, ids, rec[i].x, lrec, tgt, has_t, t);
        }
        obstacle_forces(s_obs, m, obs, moving, px, py, frx, fry, sing);
        if (!moving) {  // dead or without a target: its position in the output buffer too
            if (valid) pout[i] = make_double2(px, py);
            continue;
        }
        double fax = 0.0, fay = 0.0;
        attraction(px, py, t, fax, fay);
        const SepAcc sep = window_separation(i, px, py, g, r2, sorted_idx, off, psort, sing);
        sing = sep.sing;
        integrate(i, px, py, fax, fay, frx, fry, sep.x, sep.y, dt, max_speed, vel, pout);
    }
    count_singular(sing, singular);
}

// ---- obstacle fields (contract O1): a moving agent visits only the obstacles in its reach ----
//
// The field forms of k_physics_sensed and k_physics_loop_sensed: obstacle_forces(s_obs, ...) replaced by the
// agent's own cell of the field's grid, two offset loads and a walk over that cell's (x, y, r) triples, read at
// the cursor with no index indirection.  obstacle_term is the flat loop's body, statement for statement, and a
// cell's triples are in list order; an obstacle that is not in the agent's cell list fails the flat loop's
// pre-test for that agent (obstacle_cells.h has the proof), where it adds nothing, not even +0.0 -- so frx, fry
// and the singular count keep the flat list's bits.  No s_obs, no LDS, no barriers, and an agent that does not
// move reads nothing of the field.  Threads are in cell-sorted order and a field's cells are at least 10 units
// wide (obstacle_cells.h, obs_start_side), against sensing cells of 1 or 2: the lanes of a wave mostly walk the
// same one or two lists, so a load serves many lanes.
// Bounds: cell_coord clamps both coordinates into [0, nc - 1] (NaN: 0), so c is in [0, ncx * ncy - 1];
// off has ncx * ncy + 1 entries, ascending, the last one the number of triples (< 2^32): every q read is a
// triple of the buffer.
#ifndef SWARM_OBS_DEPTH
#define SWARM_OBS_DEPTH 2
#endif
constexpr int kObsDepth = SWARM_OBS_DEPTH;  // triples in flight per thread

__device__ __forceinline__ void obstacle_term(double ox, double oy, double r, double px, double py, double &frx,
                                              double &fry, unsigned long long &sing) {
    const double ex = px - ox, ey = py - oy;
    const double s2 = ex * ex + ey * ey;
    const double rr = 5.0 + r;
    if (s2 > rr * rr * (1.0 + 1e-12)) return;  // the flat loop's pre-test (its `continue`)
    double d = sqrt(s2) - r;
    if (d <= 0.001) d = 0.001;
    if (d < 5.0) {
        const double mag = 50.0 * (1.0 / d - 1.0 / 5.0) / (d * d);
        const double nrm = sqrt(s2);
        sing += nrm == 0.0;
        frx += (ex / nrm) * mag;
        fry += (ey / nrm) * mag;
    }
}

__device__ __forceinline__ void field_forces(const ObsFieldView &f, double px, double py, double &frx, double &fry,
                                             unsigned long long &sing) {
    const int64_t cx = cell_coord(px, f.xmin, f.inv_cell, f.ncx);
    const int64_t cy = cell_coord(py, f.ymin, f.inv_cell, f.ncy);
    const int64_t c = cy * f.ncx + cx;
    const uint32_t e = f.off[c + 1];
    for (uint32_t q = f.off[c]; q < e; q += kObsDepth) {
        double t[kObsDepth][3];
#pragma unroll
        for (int u = 0; u < kObsDepth; ++u) {
            const bool in = e - q > uint32_t(u);
            const double *p = f.tri + 3 * size_t(in ? q + u : q);
            t[u][0] = p[0], t[u][1] = p[1], t[u][2] = p[2];
        }
#pragma unroll
        for (int u = 0; u < kObsDepth; ++u)
            if (e - q > uint32_t(u)) obstacle_term(t[u][0], t[u][1], t[u][2], px, py, frx, fry, sing);
    }
}

__global__ __launch_bounds__(kBlock) void k_physics_sensed_field(
    int64_t n, const int32_t *__restrict__ ids, const uint8_t *__restrict__ state, const int32_t *__restrict__ leader,
    const double2 *__restrict__ pin, double2 *__restrict__ pout, double2 *__restrict__ vel, double2 *__restrict__ tgt,
    uint8_t *__restrict__ has_t, ObsFieldView field, Grid g, double r2, const int32_t *__restrict__ sorted_idx,
    const uint32_t *__restrict__ off, const double2 *__restrict__ psort, double dt, double max_speed,
    unsigned long long *__restrict__ st) {
    const bool stopped = st[0] != 0;  // uniform over the grid: written by an earlier kernel of the stream
    unsigned long long sing = 0;
    for (int64_t q0 = int64_t(blockIdx.x) * kBlock + threadIdx.x; q0 < n; q0 += int64_t(gridDim.x) * kBlock) {
        if (stopped) {
            pout[q0] = pin[q0];
            continue;
        }
        const int64_t i = sorted_idx[q0];
        const double2 p = psort[q0];
        const double px = p.x, py = p.y;
        double2 t;
        if (!formation_target(i, ids, state, leader, pin, tgt, has_t, t)) {
            pout[i] = make_double2(px, py);
            continue;
        }
        double frx = 0.0, fry = 0.0;
        field_forces(field, px, py, frx, fry, sing);
        double fax = 0.0, fay = 0.0;
        attraction(px, py, t, fax, fay);
        const SepAcc sep = window_separation(i, px, py, g, r2, sorted_idx, off, psort, sing);
        sing = sep.sing;
        integrate(i, px, py, fax, fay, frx, fry, sep.x, sep.y, dt, max_speed, vel, pout);
    }
    count_singular(sing, st + 1);
}

__global__ __launch_bounds__(kBlock) void k_physics_loop_sensed_field(
    int64_t n, const int32_t *__restrict__ ids, const uint2 *__restrict__ rec, const LRec *__restrict__ lrec,
    double2 *__restrict__ pout, double2 *__restrict__ vel, double2 *__restrict__ tgt, uint8_t *__restrict__ has_t,
    ObsFieldView field, Grid g, double r2, const int32_t *__restrict__ sorted_idx, const uint32_t *__restrict__ off,
    const double2 *__restrict__ psort, double dt, double max_speed, const unsigned long long *__restrict__ st,
    unsigned long long *__restrict__ singular) {
    if (st[0] != 0) return;  // uniform over the grid: written by an earlier kernel of the stream
    unsigned long long sing = 0;
    for (int64_t q0 = int64_t(blockIdx.x) * kBlock + threadIdx.x; q0 < n; q0 += int64_t(gridDim.x) * kBlock) {
        const int64_t i = sorted_idx[q0];
        const double2 p = psort[q0];
        const double px = p.x, py = p.y;
        double2 t;
        if (!formation_target_loop(i, ids, rec[i].x, lrec, tgt, has_t, t)) {
            pout[i] = make_double2(px, py);  // dead or without a target: its position in the output buffer too
            continue;
        }
        double frx = 0.0, fry = 0.0;
        field_forces(field, px, py, frx, fry, sing);
        double fax = 0.0, fay = 0.0;
        attraction(px, py, t, fax, fay);
        const SepAcc sep = window_separation(i, px, py, g, r2, sorted_idx, off, psort, sing);
        sing = sep.sing;
        integrate(i, px, py, fax, fay, frx, fry, sep.x, sep.y, dt, max_speed, vel, pout);
    }
    count_singular(sing, singular);
}

}  // namespace

int launch_physics_loop_sensed_field(int64_t n, const int32_t *ids, const uint2 *rec, const LRec *lrec,
                                     double *pos_out, double *vel, double *target, uint8_t *has_target,
                                     const ObsFieldView &field, const LoopSense &ls, double dt, double max_speed,
                                     unsigned long long *singular, hipStream_t s) {
    hipLaunchKernelGGL(k_physics_loop_sensed_field, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, n, ids, rec,
                       lrec, reinterpret_cast<double2 *>(pos_out), reinterpret_cast<double2 *>(vel),
                       reinterpret_cast<double2 *>(target), has_target, field, ls.g, ls.r2, ls.sorted, ls.off, ls.psort,
                       dt, max_speed, ls.st, singular);
    SW_LAUNCHED();
    return SWARM_OK;
}

int launch_physics_loop(int64_t n, const int32_t *ids, const uint2 *rec, const LRec *lrec, const double *pos_in,
                        double *pos_out, double *vel, double *target, uint8_t *has_target, int64_t m,
                        const double *obstacles, const int32_t *row_ptr, const int32_t *col, double dt,
                        double max_speed, unsigned long long *singular, hipStream_t s) {
    hipLaunchKernelGGL(k_physics_loop, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, n, ids, rec, lrec,
                       reinterpret_cast<const double2 *>(pos_in), reinterpret_cast<double2 *>(pos_out),
                       reinterpret_cast<double2 *>(vel), reinterpret_cast<double2 *>(target), has_target, m,
                       obstacles, row_ptr, col, dt, max_speed, singular);
    SW_LAUNCHED();
    return SWARM_OK;
}

// The grid of a call that moves its agents for `steps` steps: no agent moves more than |max_speed * dt| a
// step, so the entry bounding box grown by the run's reach holds every finite position of every step
// (cell_coord clamps the rest to an edge cell, which keeps two agents within R in adjacent cells).  One host
// wait; non-finite positions are refused here, before anything is written.
// min_cell: a second window read on the same grid (the radio loop's, of radius min_cell) needs its cells at
// least that wide; the sensing predicate, not the cell, decides who is sensed, so wider cells only add
// candidates.
static int make_run_grid(swarm_ctx *ctx, int64_t n, const double *pos, double sense_radius, int32_t steps,
                         double dt, double max_speed, Grid *g, hipStream_t s, double min_cell) {
    const double need = sense_radius < 2.0 ? sense_radius : 2.0;
    const double cell = (need > min_cell ? need : min_cell) * (1.0 + 1e-9);
    const int64_t cap4 = 4 * n + 1024, max_cells = cap4 < (int64_t(1) << 31) ? cap4 : (int64_t(1) << 31);
    const int rc = make_grid(ctx, n, pos, cell, max_cells, g, s);
    if (rc) return rc;
    double reach = double(steps) * std::fabs(max_speed * dt);
    if (!(reach < 1e12)) reach = 1e12;  // any box is exact; beyond it the agents share the edge cells
    g->xmin -= reach;
    g->ymin -= reach;
    g->xmax += reach;
    g->ymax += reach;
    return shape_grid_checked(g, cell, max_cells);  // the grown box's extent is checked again
}

int loop_sense_begin(swarm_ctx *ctx, int64_t n, const double *pos, double sense_radius, int32_t ticks, double dt,
                     double max_speed, LoopSense *ls, hipStream_t s, double min_cell) {
    const int rc = make_run_grid(ctx, n, pos, sense_radius, ticks, dt, max_speed, &ls->g, s, min_cell);
    if (rc) return rc;
    ls->r2 = sense_radius * sense_radius;
    ls->sorted = nullptr;
    ls->off = nullptr;
    SW_ALLOC(ls->psort, ctx, S_SENSE_SORTED, size_t(n) * 16);
    SW_ALLOC(ls->st, ctx, S_SENSE_STATE, 64);
    SW_HIP(hipMemsetAsync(ls->st, 0, 32, s));
    return SWARM_OK;
}

int loop_sense_tick(swarm_ctx *ctx, int64_t n, const double *pos_in, int32_t k, LoopSense *ls, hipStream_t s,
                    bool offsets_by_search) {
    double *acc;
    int rc;
    if ((rc = bin_agents(ctx, n, pos_in, ls->g, &ls->sorted, &ls->off, s, offsets_by_search))) return rc;
    // the window work against swarm_build_rgg's limits, judged on the device: a refused tick sets the stop word
    if ((rc = launch_window_work(ctx, ls->off, ls->g, s, &acc))) return rc;
    hipLaunchKernelGGL(k_sense_verdict, dim3(1), dim3(1), 0, s, acc, ls->st, k);
    SW_LAUNCHED();
    hipLaunchKernelGGL(k_sorted_positions, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s,
                       reinterpret_cast<const double2 *>(pos_in), n, ls->sorted, ls->psort);
    SW_LAUNCHED();
    return SWARM_OK;
}

int loop_sense_refusal(const unsigned long long *h, const char *fmt, ...) {
    double pairs;
    memcpy(&pairs, h + 2, 8);
    char what[112];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(what, sizeof(what), fmt, ap);
    va_end(ap);
    set_window_work_error(what, pairs, h[3]);
    return SWARM_ERR_RANGE;
}

int launch_physics_loop_sensed(int64_t n, const int32_t *ids, const uint2 *rec, const LRec *lrec, double *pos_out,
                               double *vel, double *target, uint8_t *has_target, int64_t m,
                               const double *obstacles, const LoopSense &ls, double dt, double max_speed,
                               unsigned long long *singular, hipStream_t s) {
    hipLaunchKernelGGL(k_physics_loop_sensed, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, n, ids, rec, lrec,
                       reinterpret_cast<double2 *>(pos_out), reinterpret_cast<double2 *>(vel),
                       reinterpret_cast<double2 *>(target), has_target, m, obstacles, ls.g, ls.r2, ls.sorted, ls.off,
                       ls.psort, dt, max_speed, ls.st, singular);
    SW_LAUNCHED();
    return SWARM_OK;
}

}  // namespace swarm

extern "C" {

int swarm_physics_step(swarm_ctx *ctx, int64_t n, const int32_t *ids, const uint8_t *state,
                       const int32_t *leader_index, const double *pos_in, double *pos_out, double *vel,
                       double *target, uint8_t *has_target, int64_t m, const double *obstacles,
                       const int32_t *row_ptr, const int32_t *col, double dt, double max_speed,
                       int64_t *n_singular, void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(n >= 0 && n < (int64_t(1) << 31) && m >= 0, "sizes out of range");
    SW_ARG(std::isfinite(dt) && std::isfinite(max_speed), "dt / max_speed must be finite");
    SW_ARG(n == 0 || (ids && state && leader_index && pos_in && pos_out && vel && target && has_target && row_ptr),
           "NULL agent array");
    SW_ARG(m == 0 || obstacles != nullptr, "obstacles is NULL");
    SW_ARG(pos_in != pos_out || n == 0, "pos_in and pos_out must differ (synchronous step)");
    SW_ARG(!find_moving_field(ctx, m, obstacles),
           "a moving obstacle field needs a sensed entry point (a fixed-graph step would read it as a frozen list)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_singular) *n_singular = 0;
    if (n == 0) return SWARM_OK;
    unsigned long long *d_sing;
    SW_ALLOC(d_sing, ctx, S_TMP0, 64);
    SW_HIP(hipMemsetAsync(d_sing, 0, 8, s));
    hipLaunchKernelGGL(k_physics, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, n, ids, state, leader_index,
                       reinterpret_cast<const double2 *>(pos_in), reinterpret_cast<double2 *>(pos_out),
                       reinterpret_cast<double2 *>(vel), reinterpret_cast<double2 *>(target), has_target, m, obstacles,
                       row_ptr, col, dt, max_speed, d_sing);
    SW_LAUNCHED();
    if (n_singular) {
        unsigned long long *h = static_cast<unsigned long long *>(pinned(ctx, 64));
        if (!h) return SWARM_ERR_OOM;
        SW_HIP(hipMemcpyAsync(h, d_sing, 8, hipMemcpyDeviceToHost, s));
        SW_HIP(hipStreamSynchronize(s));
        *n_singular = int64_t(*h);
    }
    return SWARM_OK;
}

int swarm_physics_run_sensed(swarm_ctx *ctx, int64_t n, const int32_t *ids, const uint8_t *state,
                             const int32_t *leader_index, double *pos, double *vel, double *target,
                             uint8_t *has_target, int64_t m, const double *obstacles, double sense_radius,
                             int32_t steps, double dt, double max_speed, int32_t *steps_done, int64_t *n_singular,
                             void *stream) {
    using namespace swarm;
    SW_ARG(ctx != nullptr, "ctx is NULL");
    SW_ARG(n >= 0 && n < (int64_t(1) << 31) - 1 && m >= 0, "sizes out of range");
    SW_ARG(steps >= 0, "steps must not be negative");
    SW_ARG(sense_radius > 0 && std::isfinite(sense_radius), "sense_radius must be positive and finite");
    SW_ARG(std::isfinite(dt) && std::isfinite(max_speed), "dt / max_speed must be finite");
    SW_ARG(n == 0 || (ids && state && leader_index && pos && vel && target && has_target), "NULL agent array");
    SW_ARG(m == 0 || obstacles != nullptr, "obstacles is NULL");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0 || steps == 0) {
        if (steps_done) *steps_done = n == 0 ? steps : 0;
        if (n_singular) *n_singular = 0;
        return SWARM_OK;
    }
    // One grid for the whole call (loop_sense_begin).  Host wait 1 of 2; non-finite positions are refused here,
    // before anything is written.
    // (contract O2) a moving field's list comes to the host with that wait; its grid and capacity are refused
    // before anything is written as well
    swarm_obstacle_field *mov = find_moving_field(ctx, m, obstacles);
    LoopSense ls{};
    int rc;
    if (mov && (rc = moving_field_fetch(mov, s))) return rc;
    if ((rc = loop_sense_begin(ctx, n, pos, sense_radius, steps, dt, max_speed, &ls, s))) return rc;
    if (mov && (rc = moving_field_begin(mov, steps, dt, false, s))) return rc;
    double2 *other;
    SW_ALLOC(other, ctx, S_SENSE_POS, size_t(n) * 16);
    unsigned long long *h = static_cast<unsigned long long *>(pinned(ctx, 64));
    if (!h) return SWARM_ERR_OOM;
    double2 *buf[2] = {reinterpret_cast<double2 *>(pos), other};
    // `obstacles` that is a live field's own list: the field's path (contract O1: the same bits)
    const swarm_obstacle_field *fld = find_obstacle_field(ctx, m, obstacles);
    // a refused step sets the stop word (ls.st[0]): it and every later step only copy the positions through
    auto queue_step = [&](int32_t k) -> int {
        const double2 *pin = buf[k & 1];
        const int rc = loop_sense_tick(ctx, n, reinterpret_cast<const double *>(pin), k, &ls, s, false);
        if (rc) return rc;
        if (mov) {  // the lists of O_{k}, the field's kernel on them, then every obstacle advances once
            ObsFieldView view;
            int rm;
            if ((rm = moving_field_tick(mov, ls.st, k, &view, s))) return rm;
            hipLaunchKernelGGL(k_physics_sensed_field, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, n, ids,
                               state, leader_index, pin, buf[(k + 1) & 1], reinterpret_cast<double2 *>(vel),
                               reinterpret_cast<double2 *>(target), has_target, view, ls.g, ls.r2, ls.sorted, ls.off,
                               ls.psort, dt, max_speed, ls.st);
            SW_LAUNCHED();
            return moving_field_advance(mov, ls.st, dt, s);
        }
        if (fld)
            hipLaunchKernelGGL(k_physics_sensed_field, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, n, ids,
                               state, leader_index, pin, buf[(k + 1) & 1], reinterpret_cast<double2 *>(vel),
                               reinterpret_cast<double2 *>(target), has_target, obstacle_field_view(*fld), ls.g, ls.r2,
                               ls.sorted, ls.off, ls.psort, dt, max_speed, ls.st);
        else
            hipLaunchKernelGGL(k_physics_sensed, dim3(grid_for(n, kBlock, 8192)), dim3(kBlock), 0, s, n, ids, state,
                               leader_index, pin, buf[(k + 1) & 1], reinterpret_cast<double2 *>(vel),
                               reinterpret_cast<double2 *>(target), has_target, m, obstacles, ls.g, ls.r2, ls.sorted,
                               ls.off, ls.psort, dt, max_speed, ls.st);
        SW_LAUNCHED();
        return SWARM_OK;
    };
    // a step that could not be queued (scratch, a launch error) ends the run after the steps before it:
    // its fused kernel did not run, so the state after `queued` steps is whole, and it is reported as
    // any other result before the step's error is returned
    int32_t queued = 0;
    for (rc = SWARM_OK; queued < steps; ++queued)
        if ((rc = queue_step(queued))) break;
    if (queued & 1) SW_HIP(hipMemcpyAsync(pos, other, size_t(n) * 16, hipMemcpyDeviceToDevice, s));
    SW_HIP(hipMemcpyAsync(h, ls.st, 32, hipMemcpyDeviceToHost, s));
    h[5] = 0;
    if (mov) (void)moving_field_error(mov, h + 5, s);
    SW_HIP(hipStreamSynchronize(s));  // host wait 2 of 2
    const int32_t done = h[0] ? int32_t(h[0] - 1) : queued;
    if (steps_done) *steps_done = done;
    if (n_singular) *n_singular = int64_t(h[1]);
    if (rc) return rc;
    if (h[5]) return moving_field_overflowed();
    if (h[0])
        return loop_sense_refusal(h, "agents too dense to sense at step %d (%d steps done)", int(done), int(done));
    return SWARM_OK;
}

}  // extern "C"
