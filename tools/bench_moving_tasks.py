#!/usr/bin/env python3
"""Measure moving task boards (Swarm.set_task_board(..., velocities=), contract U1-M) on tools/bench_loop_board.py's
setup: the C3 swarm, 200 ticks, kills at 80 / 150, Rc = Rs = 1.0, C3's own 10 000 tasks.  bench.py is not involved.

Legs (ms per tick, wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs, the legs
taking turns run by run so that drift hits them alike; reported as min - median - max):
  a  the static board (update_loop_board as it was);
  b  a moving board at zero velocities: b - a is what the device rebuild and the advance cost per tick (the results
     are the static board's, bit for bit -- the position checksums are compared);
  c  the same 10 000 tasks drifting at up to --speed units/s;
  d  the workaround a moving board replaces: update_loop_board(1) and a new board handle per tick from Python, the
     positions advanced by numpy.  It computes something else: a claim is heard with the next tick's positions;
  e  --big-tasks moving tasks, uniform over a square --big-spread times the arena's side around it (over the arena
     alone a million tasks put hundreds within reach of every agent, and the rows, not the board, are measured).
Rows are doubled and the run repeated from the same start while a board run is refused.  Results are merged into
--out under --label.

Usage:  python tools/bench_moving_tasks.py [--agents N] [--legs a,b,c,d,e] [--tasks T] [--big-tasks T] [--big-spread S]
            [--speed V] [--slots K] [--reps R] [--label NAME] [--pkg DIR] [--out FILE]
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
    ap.add_argument("--big-tasks", type=int, default=1_000_000)
    ap.add_argument("--big-spread", type=float, default=10.0)
    ap.add_argument("--speed", type=float, default=3.0)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c,d,e")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_moving_tasks", "moving_tasks.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    legs = [k for k in "abcde" if k in a.legs.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=a.tasks)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev).build_graph(1.0)
    n, ticks, rc, rs, dt = sw.n, a.ticks, a.radio_radius, a.sense_radius, 0.1
    graph0 = (sw.row_ptr, sw.col)
    print(f"[bench_moving_tasks] {a.label}: n={n} Rc={rc} Rs={rs} T={a.tasks} legs={legs}", file=sys.stderr, flush=True)
    g = np.random.default_rng(a.seed + 3)  # (bench_loop_tasks.py's draws, in its order)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    g.uniform(0, side, 64), g.uniform(0, side, 64)  # (bench_loop_board.py's 64-task board: not used here)
    vel = g.uniform(-a.speed, a.speed, (a.tasks, 2))
    lo, hi = side * (1.0 - a.big_spread) / 2.0, side * (1.0 + a.big_spread) / 2.0
    big = (g.uniform(lo, hi, a.big_tasks), g.uniform(lo, hi, a.big_tasks),
           g.integers(-1, 3, a.big_tasks).astype(np.int8), g.uniform(-a.speed, a.speed, (a.big_tasks, 2)))
    c3 = (d["tx"], d["ty"], d["treq"])
    boards = {"a_static_board": (c3, None), "b_moving_board_zero_velocities": (c3, np.zeros_like(vel)),
              "c_moving_board": (c3, vel), "d_one_tick_calls_and_a_new_handle_per_tick": (c3, None),
              "e_moving_board_big": (big[:3], big[3])}
    slots = {k: [a.slots, a.slots] for k in boards}
    pos0 = sw.pos.clone()
    kills = (80, 150)
    kw = dict(obstacles=obs, kill_ticks=kills, seed=5)

    def reset(name):
        sw.pos.copy_(pos0)
        sw.row_ptr, sw.col = graph0
        sw._hear = None
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        (tx, ty, rq), v = boards[name]
        sw.set_task_board(tx, ty, rq, status_slots=slots[name][0], table_slots=slots[name][1], velocities=v)
        torch.cuda.synchronize()

    def one_call():
        return sw.update_loop_board(ticks, rc, rs, **kw)

    def per_tick_handles():
        """Leg d: the rows carried from handle to handle, the positions advanced on the host."""
        name = "d_one_tick_calls_and_a_new_handle_per_tick"
        (tx, ty, rq), _ = boards[name]
        import ctypes
        q = np.stack([tx, ty], 1).astype(np.float64)
        lib, ctx, first = _lib.lib(), sw.board["ctx"], sw.board["handle"]
        rq_dev = torch.as_tensor(np.asarray(rq, np.int8), device=dev)
        tc, guard = [], 0
        try:
            for _ in range(ticks):
                r = sw.update_loop_board(1, rc, rs, **kw)
                tc.append(r["task_counts"])
                guard += r["guard"]
                q = q + vel * dt
                handle, tpos = ctypes.c_void_p(), torch.as_tensor(q, device=dev)
                _lib.check(lib.swarm_board_create(ctx, len(q), _lib.ptr(tpos), _lib.ptr(rq_dev), ctypes.byref(handle),
                                                  None, _lib.stream()))
                old, sw.board["handle"] = sw.board["handle"], handle
                if old is not first:  # (the first one is set_task_board's, and its finalizer's)
                    _lib.check(lib.swarm_board_destroy(ctx, old))
        finally:
            last, sw.board["handle"] = sw.board["handle"], first
            if last is not first:
                lib.swarm_board_destroy(ctx, last)
        return dict(task_counts=np.concatenate(tc), guard=guard)

    def refusing(name, run):
        def go():
            while True:
                try:
                    return run()
                except _lib.SwarmError as err:
                    if err.code != _lib.ERR_RANGE or sw.last_board_overflow is None:
                        raise
                    kind = sw.last_board_overflow[0]
                    slots[name][0 if kind == "status" else 1] *= 2
                    print(f"[bench_moving_tasks] {name}: {kind} rows full at tick {sw.last_refused_tick}, now "
                          f"{slots[name]}", file=sys.stderr, flush=True)
                    reset(name)
        return go

    runs = {k: refusing(k, per_tick_handles if k[0] == "d" else one_call) for k in boards}
    names = [k for k in runs if k[0] in legs]
    res = {"agents": n, "ticks": ticks, "kill_ticks": list(kills), "radio_radius": rc, "sense_radius": rs,
           "tasks": a.tasks, "tasks_leg_e": a.big_tasks, "spread_leg_e": a.big_spread, "speed": a.speed, "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; the legs take "
                   "turns run by run; min - median - max of the timed runs",
           "leg_d_note": "computes something else: a claim is heard with the positions of the tick after it was sent"}
    times = {k: [] for k in names}
    sums = {}
    for rep in range(a.reps + 1):  # the first round is the warm-up (and finds the rows that fit)
        for k in names:
            reset(k)
            t0 = time.perf_counter()
            r = runs[k]()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / ticks
            print(f"[bench_moving_tasks] {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick", file=sys.stderr,
                  flush=True)
            if rep:
                times[k].append(ms)
            sums[k] = [float(sw.pos[:, 0].sum()), float(sw.pos[:, 1].sum())]
            tc, b = r["task_counts"], sw.board
            res[k + "_tasks"] = {"claims_sent": int(tc[:, 0].sum()), "claims_handled_by_a_leader": int(tc[:, 1].sum()),
                                 "conflicts_sent": int(tc[:, 2].sum()), "guard_pairs": int(r["guard"]),
                                 "status_slots": b["Ks"], "table_slots": b["Kt"],
                                 "peak_status_entries_per_agent": int((b["status"] >= 0).sum(1).max()),
                                 "peak_table_entries_per_agent": int((b["tab_task"] >= 0).sum(1).max())}
    res["ms_per_tick"] = {k: [min(v), float(np.median(v)), max(v)] for k, v in times.items() if v}
    res["pos_checksum"] = sums
    ka, kb = "a_static_board", "b_moving_board_zero_velocities"
    if ka in sums and kb in sums:
        assert sums[ka] == sums[kb], ("legs a and b ended differently", sums)
        assert res[ka + "_tasks"] == res[kb + "_tasks"]
        if times[ka]:
            res["rebuild_and_advance_ms_per_tick"] = float(np.median(times[kb]) - np.median(times[ka]))
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
