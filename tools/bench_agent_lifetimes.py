#!/usr/bin/env python3
"""ms per tick of agent lifetimes (contract U1-J) at C3, on bench_task_lifetimes.py's setup: the C3
swarm, Rc = Rs = 1.0, kills at 80 / 150, 30 % of the agents with a target.  bench.py is left alone.  For every loop
asked for (radio: update_loop_radio; board: update_loop_board with C3's 10 000 tasks at rest on 16 / 16 slots) the
legs take turns run by run, after one warm-up run each, min - median - max of the timed runs:

  a  the loop without lifetimes;
  b  default windows set, so no event in the call (must end in a's state: the call adds no launch, and b - a should
     lie within the spread of a's own runs);
  c  steady churn: 1 % of the agents restarting every 10 ticks (each group once; their alive flags are put back
     after the set-time rule, so they are up when they boot) and a burst of 10 % dying on one tick;
  d  the per-tick workaround c replaces: one loop call per stretch between event ticks, with torch edits of alive,
     state, leader, tick_off, the timers, vel, target, the outbox halves and the board rows from Python in between
     (must end in c's state).

--events-only runs leg c alone, once after a warm-up, for a kernel-trace run of its own (k_agent_events' time per
event tick comes from that trace, not from this script).

Usage:  python tools/bench_agent_lifetimes.py [--agents N] [--loops radio,board] [--ticks K] [--reps R]
                                              [--label NAME] [--out FILE] [--events-only]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOREVER = np.iinfo(np.int64).max


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--deg", type=float, default=16.0)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--radio-radius", type=float, default=1.0)
    ap.add_argument("--sense-radius", type=float, default=1.0)
    ap.add_argument("--tasks", type=int, default=10_000)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loops", default="radio,board")
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--events-only", action="store_true")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r37_agent_lifetimes", "agent_lifetimes.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=a.tasks)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev)
    n, ticks, rc, rs, T = sw.n, a.ticks, a.radio_radius, a.sense_radius, a.tasks
    g = np.random.default_rng(a.seed + 3)  # (bench_loop_tasks.py's draws, in its order)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    pos0 = sw.pos.clone()
    kills = (80, 150)
    kw = dict(obstacles=obs, kill_ticks=kills, seed=5)
    # the churn: group q (1 % of the agents) restarts at tick 10 (q + 1); 10 % of the others die at the burst tick
    gl = np.random.default_rng(a.seed + 41)
    who = gl.permutation(n)
    per, groups = max(n // 100, 1), ticks // 10
    boot, death = np.zeros(n, np.int64), np.full(n, FOREVER)
    for q in range(groups):
        boot[who[q * per:(q + 1) * per]] = 10 * (q + 1)
    burst = ticks // 2 + 5
    death[who[groups * per:groups * per + n // 10]] = burst
    event_ticks = sorted(set([10 * (q + 1) for q in range(groups)] + [burst]))
    perm = sw.perm.cpu().numpy().astype(np.int64)
    boot_s, death_s = torch.as_tensor(boot[perm], device=dev), torch.as_tensor(death[perm], device=dev)

    def reset(loop, windows):
        sw.pos.copy_(pos0)
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        if loop == "board":
            sw.set_task_board(d["tx"], d["ty"], d["treq"], status_slots=a.slots, table_slots=a.slots)
        if windows is not None:
            sw.set_agent_lifetimes(*windows)
            sw.fsm["alive"].fill_(1)  # restarts: up when they boot
        torch.cuda.synchronize()

    def run(loop, k):
        if loop == "board":
            return sw.update_loop_board(k, rc, rs, **kw)
        return sw.update_loop_radio(k, rc, rs, **kw)

    def edit(t):
        f, m = sw.fsm, sw.n
        dies = torch.nonzero(death_s == t)[:, 0]
        boots = torch.nonzero(boot_s == t)[:, 0]
        if dies.numel():
            f["alive"][dies] = 0
        if not boots.numel():
            return
        f["alive"][boots] = 1
        sw.state[boots] = 1
        sw.leader[boots] = -1
        f["leader_pos"][boots] = 0.0
        f["has_leader_pos"][boots] = 0
        f["last_hb"][boots] = float(t - 1) * 0.1
        f["wait_start"][boots] = 0.0
        f["delay"][boots] = 0.0
        sw.tick_off[boots] = 1 - t
        sw.vel[boots] = 0.0
        sw.target[boots] = 0.0
        sw.has_target[boots] = 0
        for half in (boots, boots + m):
            f["outbox"][half] = 0
        if hasattr(sw, "board"):
            b = sw.board
            for k in ("status", "tab_task", "tab_winner"):
                b[k][boots] = -1
            b["tab_util"][boots] = 0.0
            for half in (boots, boots + m):
                b["claim_out"][half] = -1
                b["conflict_out"][half] = -1

    def workaround(loop):
        t = 0
        for e in event_ticks + [ticks + 1]:
            if e - 1 > t:
                run(loop, e - 1 - t)
                t = e - 1
            if e <= ticks:
                edit(e)
        return None

    def checksum():
        out = [float(sw.pos[:, 0].sum()), float(sw.pos[:, 1].sum()), int(sw.leader.long().sum()),
               int(sw.fsm["alive"].sum()), int(sw.tick_off.long().sum())]
        if hasattr(sw, "board"):
            out.append(int(sw.board["status"].long().sum()))
        return out

    res = {"agents": n, "ticks": ticks, "kill_ticks": list(kills), "radio_radius": rc, "sense_radius": rs,
           "libswarm": _lib.version(), "label": a.label, "event_ticks": event_ticks,
           "events": {"restarts_per_event_tick": per, "deaths_at_the_burst": int((death == burst).sum())},
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; the legs take "
                   "turns run by run; min - median - max of the timed runs"}
    legs = {"a_no_lifetimes": None, "b_default_windows": (0, None), "c_churn": (boot, death), "d_workaround": None}
    names = ["c_churn"] if a.events_only else [k for k in legs if k[0] in a.legs.split(",")]
    for loop in a.loops.split(","):
        if hasattr(sw, "board") and loop != "board":
            sw.board["finalizer"]()
            del sw.board
        times, sums = {k: [] for k in names}, {}
        for rep in range((1 if a.events_only else a.reps) + 1):
            for k in names:
                reset(loop, legs[k])
                t0 = time.perf_counter()
                if k == "d_workaround":
                    workaround(loop)
                else:
                    r = run(loop, ticks)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / ticks
                print(f"[bench_agent_lifetimes] {loop} {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick",
                      file=sys.stderr, flush=True)
                if rep:
                    times[k].append(ms)
                sums[k] = checksum()
                if k == "c_churn":
                    res[loop + "_agent_events_total"] = [int(v) for v in r["agent_events"].sum(0)]
        res[loop + "_ms_per_tick"] = {k: [min(v), float(np.median(v)), max(v)] for k, v in times.items() if v}
        res[loop + "_checksums"] = sums
        if "a_no_lifetimes" in sums and "b_default_windows" in sums:
            assert sums["a_no_lifetimes"] == sums["b_default_windows"], ("legs a and b ended differently", sums)
        if "c_churn" in sums and "d_workaround" in sums:
            assert sums["c_churn"] == sums["d_workaround"], ("legs c and d ended differently", sums)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    old = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            old = json.load(fh)
    old[a.label] = res
    with open(a.out, "w") as fh:
        json.dump(old, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
