#!/usr/bin/env python3
"""Measure the radio and task update loops over a lossy channel (contract U1-L: Swarm.update_loop_radio /
Swarm.update_loop_tasks with loss=) on tools/bench_loop_tasks.py's setup: the C3 swarm, 200 ticks, kills at
80 / 150, Rc = Rs = 1.0, a board of 64 tasks spread over the arena.  bench.py is not involved.

Legs (ms per tick, wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs, the
legs taking turns run by run so that drift hits them alike): both loops at every --loss value; loss 0 goes
through the loss-free kernels.  Loss changes the workload -- more timeouts, more elections, more storm ticks --
so the lossy legs are not comparable tick for tick with the loss-free ones: every leg reports its elections
(ACCLAIMs sent over the run), its leaders at the end and its link_counts totals next to its time.
Results are merged into --out under --label.

Usage:  python tools/bench_loop_lossy.py [--agents N] [--loss 0,0.01,0.1,0.3] [--loops radio,tasks] [--label NAME]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--deg", type=float, default=16.0)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--radio-radius", type=float, default=1.0)
    ap.add_argument("--sense-radius", type=float, default=1.0)
    ap.add_argument("--tasks", type=int, default=64)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--loss-seed", type=int, default=11)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loss", default="0,0.01,0.1,0.3")
    ap.add_argument("--loops", default="radio,tasks")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_lossy_links", "update_loop_lossy.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    losses = [float(v) for v in a.loss.split(",")]
    loops = [k for k in ("radio", "tasks") if k in a.loops.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=1)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev)
    n, ticks, rc, rs, T = sw.n, a.ticks, a.radio_radius, a.sense_radius, a.tasks
    print(f"[bench_loop_lossy] {a.label}: n={n} Rc={rc} Rs={rs} T={T} loss={losses} loops={loops}", file=sys.stderr,
          flush=True)
    g = np.random.default_rng(a.seed + 3)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    board = (g.uniform(0, side, T), g.uniform(0, side, T))
    pos0 = sw.pos.clone()
    kills = (80, 150)

    def reset(tasks):
        sw.pos.copy_(pos0)
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        if tasks:
            sw.set_tasks(*board)
        torch.cuda.synchronize()

    kw = dict(obstacles=obs, kill_ticks=kills, seed=5)
    legs = [(lp, p) for lp in loops for p in losses]
    name = lambda lp, p: f"update_loop_{lp}_loss_{p:g}"  # noqa: E731
    res = {"agents": n, "ticks": ticks, "kill_ticks": list(kills), "radio_radius": rc, "sense_radius": rs, "tasks": T,
           "loss_seed": a.loss_seed, "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; the legs "
                   "take turns run by run"}
    times = {name(*k): [] for k in legs}
    for rep in range(a.reps + 1):  # the first round is the warm-up
        for lp, p in legs:
            reset(lp == "tasks")
            run = sw.update_loop_tasks if lp == "tasks" else sw.update_loop_radio
            t0 = time.perf_counter()
            r = run(ticks, rc, rs, loss=p, loss_seed=a.loss_seed, **kw)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / ticks
            k = name(lp, p)
            print(f"[bench_loop_lossy] {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick", file=sys.stderr,
                  flush=True)
            if rep:
                times[k].append(ms)
            info = {"elections_acclaims_sent": int(r["counts"][:, 2].sum()), "heartbeats_sent": int(r["counts"][:, 3].sum()),
                    "leaders_at_the_end": int(r["counts"][-1, 0]), "waiting_at_the_end": int(r["counts"][-1, 1])}
            if "link_counts" in r:
                info["election_links"], info["election_links_dropped"] = (int(v) for v in r["link_counts"].sum(0))
            if "task_counts" in r:
                tc = r["task_counts"]
                info.update(claims_sent=int(tc[:, 0].sum()), claims_handled_by_a_leader=int(tc[:, 1].sum()),
                            conflicts_sent=int(tc[:, 2].sum()))
            res[k + "_run"] = info
    res.update(times)
    res["median_ms_per_tick"] = {k: float(np.median(v)) for k, v in times.items()}
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out[a.label] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({a.label: res}))


if __name__ == "__main__":
    main()
