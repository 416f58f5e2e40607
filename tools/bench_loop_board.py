#!/usr/bin/env python3
"""Measure the task loop on boards of any size (Swarm.update_loop_board, contract U1-B) on
tools/bench_loop_tasks.py's setup: the C3 swarm, 200 ticks, kills at 80 / 150, Rc = Rs = 1.0.  bench.py is not
involved.

Legs (ms per tick, wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs, the legs
taking turns run by run so that drift hits them alike):
  a  update_loop_board with bench_loop_tasks.py's board of 64 tasks over the arena, and update_loop_tasks on the
     same board (a_update_loop_tasks): the price of the sparse rows where both loops apply;
  b  update_loop_board with C3's own 10 000 tasks (gen.tasks), --slots status / table slots per agent, doubled
     until the run is not refused; the peak slot use per agent is reported;
  c  update_loop_radio: what a and b are reported over, in the same session;
  d  update_loop_tasks, update_loop_radio, update_loop_sensed, update_loop and protocol_run: the existing loops,
     whose kernels this loop leaves alone.  Against the parent commit: run the tool once on this tree and once
     with --pkg pointing at that commit's built package, under different --label, in alternating processes.
Results are merged into --out under --label.

Usage:  python tools/bench_loop_board.py [--agents N] [--legs a,b,c,d] [--label NAME] [--pkg DIR] [--out FILE]
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
    ap.add_argument("--tasks", type=int, default=10_000)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_task_board", "update_loop_board.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    legs = [k for k in "abcd" if k in a.legs.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=a.tasks)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev).build_graph(1.0)
    n, e, ticks, rc, rs = sw.n, sw.n_edges, a.ticks, a.radio_radius, a.sense_radius
    graph0 = (sw.row_ptr, sw.col)
    print(f"[bench_loop_board] {a.label}: n={n} E={e} Rc={rc} Rs={rs} T={a.tasks} legs={legs}", file=sys.stderr,
          flush=True)
    g = np.random.default_rng(a.seed + 3)  # (bench_loop_tasks.py's draws, in its order)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    board64 = (g.uniform(0, side, 64), g.uniform(0, side, 64))
    board_c3 = (d["tx"], d["ty"], d["treq"])
    slots = {"a": [a.slots, a.slots], "b": [a.slots, a.slots]}
    pos0 = sw.pos.clone()
    kills = (80, 150)

    def reset(name):
        """The same start for every run: positions, message graph, FSM, velocity, 30 % of the agents with a
        target, and a fresh board where the leg has one."""
        sw.pos.copy_(pos0)
        sw.row_ptr, sw.col = graph0
        sw._hear = None
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        if name == "a_update_loop_board_64_tasks":
            sw.set_task_board(*board64, status_slots=slots["a"][0], table_slots=slots["a"][1])
        elif name == "b_update_loop_board_c3_tasks":
            sw.set_task_board(*board_c3, status_slots=slots["b"][0], table_slots=slots["b"][1])
        elif name.endswith("update_loop_tasks"):
            sw.set_tasks(*board64)
        torch.cuda.synchronize()

    kw = dict(obstacles=obs, kill_ticks=kills, seed=5)

    def board_run(leg):
        """update_loop_board, its rows doubled and the run repeated from the same start while it is refused."""
        def go():
            name = [k for k in runs if k[0] == leg and "board" in k][0]
            while True:
                try:
                    return sw.update_loop_board(ticks, rc, rs, **kw)
                except _lib.SwarmError as err:
                    if err.code != _lib.ERR_RANGE or sw.last_board_overflow is None:
                        raise
                    kind = sw.last_board_overflow[0]
                    slots[leg][0 if kind == "status" else 1] *= 2
                    print(f"[bench_loop_board] {name}: {kind} rows full at tick {sw.last_refused_tick}, now "
                          f"{slots[leg]}", file=sys.stderr, flush=True)
                    reset(name)
        return go

    runs = {
        "a_update_loop_board_64_tasks": board_run("a"),
        "a_update_loop_tasks": lambda: sw.update_loop_tasks(ticks, rc, rs, **kw),
        "b_update_loop_board_c3_tasks": board_run("b"),
        "c_update_loop_radio": lambda: sw.update_loop_radio(ticks, rc, rs, **kw),
        "d_update_loop_tasks": lambda: sw.update_loop_tasks(ticks, rc, rs, **kw),
        "d_update_loop_radio": lambda: sw.update_loop_radio(ticks, rc, rs, **kw),
        "d_update_loop_sensed": lambda: sw.update_loop_sensed(ticks, rs, **kw),
        "d_update_loop": lambda: sw.update_loop(ticks, **kw),
        "d_protocol_run": lambda: sw.protocol_run(ticks, kill_ticks=kills, seed=5),
    }
    names = [k for k in runs if k[0] in legs and (hasattr(sw, "update_loop_board") or "board" not in k)]
    res = {"agents": n, "edges": e, "ticks": ticks, "kill_ticks": list(kills), "radio_radius": rc,
           "sense_radius": rs, "tasks_leg_b": a.tasks, "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; "
                   "the legs take turns run by run"}
    times = {k: [] for k in names}
    sums, leaders = {}, {}
    for rep in range(a.reps + 1):  # the first round is the warm-up (and finds the rows that fit)
        for k in names:
            reset(k)
            t0 = time.perf_counter()
            r = runs[k]()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / ticks
            print(f"[bench_loop_board] {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick",
                  file=sys.stderr, flush=True)
            if rep:
                times[k].append(ms)
            sums[k] = [float(sw.pos[:, 0].sum()), float(sw.pos[:, 1].sum())]
            leaders[k] = int(sw.leader.to(torch.int64).sum())
            if isinstance(r, dict) and "task_counts" in r:
                tc = r["task_counts"]
                res[k + "_tasks"] = {"claims_sent": int(tc[:, 0].sum()), "claims_handled_by_a_leader": int(tc[:, 1].sum()),
                                     "conflicts_sent": int(tc[:, 2].sum()), "guard_pairs": int(r["guard"])}
                if "board" in k:
                    b = sw.board
                    res[k + "_tasks"].update(
                        status_slots=b["Ks"], table_slots=b["Kt"],
                        peak_status_entries_per_agent=int((b["status"] >= 0).sum(1).max()),
                        peak_table_entries_per_agent=int((b["tab_task"] >= 0).sum(1).max()),
                        agents_with_a_status=int((b["status"][:, 0] >= 0).sum()),
                        agents_with_a_table=int((b["tab_task"][:, 0] >= 0).sum()),
                        board_state_bytes_per_agent=12 * b["Ks"] + 20 * b["Kt"], grid=b["info"])
    res.update(times)
    res["pos_checksum"], res["leader_checksum"] = sums, leaders
    ka, kt = "a_update_loop_board_64_tasks", "a_update_loop_tasks"
    if ka in sums and kt in sums:  # one board, two storage layouts: the same run
        assert sums[ka] == sums[kt] and leaders[ka] == leaders[kt], ("leg a's two loops ended differently", sums)
        assert res[ka + "_tasks"]["claims_sent"] == res[kt + "_tasks"]["claims_sent"]
    kc = "c_update_loop_radio"
    if kc in times:
        med = lambda v: float(np.median(v))  # noqa: E731
        res["ms_per_tick_over_the_radio_loop"] = {k: med(times[k]) - med(times[kc]) for k in names if k[0] in "ab"}
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
