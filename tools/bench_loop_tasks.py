#!/usr/bin/env python3
"""Measure the update loop that claims and resolves tasks every tick (Swarm.update_loop_tasks, contract U1-T)
on tools/bench_loop_radio.py's setup: the C3 swarm, 200 ticks, kills at 80 / 150, Rc = Rs = 1.0.  bench.py is
not involved.

Legs (ms per tick, wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs, the
legs taking turns run by run so that drift hits them alike):
  a  update_loop_tasks with a board of 64 tasks spread uniformly over the arena (no required capability);
  b  update_loop_tasks with every one of the 64 tasks out of everyone's reach: the per-agent task words are
     streamed, nothing is claimed;
  c  update_loop_radio: what a and b are reported against, in the same session;
  d  update_loop_radio, update_loop_sensed, update_loop and protocol_run: the loops around this one
     (update_loop_radio shares its window receive, all of them the agent's end of a tick);
  e  protocol_run without a hearers graph (mode "pull": k_tick_pull, which no other leg runs).
Against another commit: run it once on this tree and once with --pkg pointing at that commit's built package,
under different --label, in alternating processes, and compare.
Results are merged into --out under --label.

Usage:  python tools/bench_loop_tasks.py [--agents N] [--legs a,b,c,d,e] [--label NAME] [--pkg DIR] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_loop_tasks", "update_loop_tasks.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    legs = [k for k in "abcde" if k in a.legs.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=1)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev).build_graph(1.0)
    n, e, ticks, rc, rs, T = sw.n, sw.n_edges, a.ticks, a.radio_radius, a.sense_radius, a.tasks
    graph0 = (sw.row_ptr, sw.col)
    print(f"[bench_loop_tasks] {a.label}: n={n} E={e} Rc={rc} Rs={rs} T={T} legs={legs}", file=sys.stderr, flush=True)
    g = np.random.default_rng(a.seed + 3)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    boards = {"a": (g.uniform(0, side, T), g.uniform(0, side, T)),
              "b": (np.full(T, -1.0e6), np.linspace(-1.0e6, 1.0e6, T))}
    pos0 = sw.pos.clone()
    kills = (80, 150)

    def reset(board=None):
        """The same start for every run: positions, message graph, FSM, velocity, 30 % of the agents with a
        target, and a fresh board where the leg has one."""
        sw.pos.copy_(pos0)
        sw.row_ptr, sw.col = graph0
        sw._hear = None
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        if board is not None:
            sw.set_tasks(*boards[board])
        torch.cuda.synchronize()

    kw = dict(obstacles=obs, kill_ticks=kills, seed=5)
    runs = {
        "a_update_loop_tasks_board_in_the_arena": lambda: sw.update_loop_tasks(ticks, rc, rs, **kw),
        "b_update_loop_tasks_board_out_of_reach": lambda: sw.update_loop_tasks(ticks, rc, rs, **kw),
        "c_update_loop_radio": lambda: sw.update_loop_radio(ticks, rc, rs, **kw),
        "d_update_loop_radio": lambda: sw.update_loop_radio(ticks, rc, rs, **kw),
        "d_update_loop_sensed": lambda: sw.update_loop_sensed(ticks, rs, **kw),
        "d_update_loop": lambda: sw.update_loop(ticks, **kw),
        "d_protocol_run": lambda: sw.protocol_run(ticks, kill_ticks=kills, seed=5),
        "e_protocol_run_pull": lambda: sw.protocol_run(ticks, kill_ticks=kills, seed=5, mode="pull"),
    }
    names = [k for k in runs if k[0] in legs]
    res = {"agents": n, "edges": e, "ticks": ticks, "kill_ticks": list(kills), "radio_radius": rc,
           "sense_radius": rs, "tasks": T, "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; "
                   "the legs take turns run by run"}
    times = {k: [] for k in names}
    sums, leaders = {}, {}
    for rep in range(a.reps + 1):  # the first round is the warm-up
        for k in names:
            reset(k[0] if k[0] in boards else None)
            t0 = time.perf_counter()
            r = runs[k]()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / ticks
            print(f"[bench_loop_tasks] {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick",
                  file=sys.stderr, flush=True)
            if rep:
                times[k].append(ms)
            sums[k] = [float(sw.pos[:, 0].sum()), float(sw.pos[:, 1].sum())]
            leaders[k] = int(sw.leader.to(torch.int64).sum())
            if isinstance(r, dict) and "task_counts" in r:
                tc = r["task_counts"]
                st = sw.task_status()
                res[k + "_tasks"] = {"claims_sent": int(tc[:, 0].sum()), "claims_handled_by_a_leader": int(tc[:, 1].sum()),
                                     "conflicts_sent": int(tc[:, 2].sum()), "guard_pairs": int(r["guard"]),
                                     "claims_sent_at_tick_1": int(tc[0, 0]),
                                     "statuses_at_the_end": torch.bincount(st.flatten().long(), minlength=4).tolist()}
    res.update(times)
    res["pos_checksum"], res["leader_checksum"] = sums, leaders
    kb, kc = "b_update_loop_tasks_board_out_of_reach", "c_update_loop_radio"
    if kb in sums and kc in sums:  # an idle board is the radio loop
        assert sums[kb] == sums[kc] and leaders[kb] == leaders[kc], ("legs b and c ended differently", sums, leaders)
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
