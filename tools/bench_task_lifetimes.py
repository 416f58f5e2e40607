#!/usr/bin/env python3
"""Measure task lifetimes (Swarm.set_task_board(..., open_tick=, close_tick=), contract U1-A) on
tools/bench_moving_tasks.py's setup: the C3 swarm, 200 ticks, kills at 80 / 150, Rc = Rs = 1.0, C3's own 10 000
tasks on a moving board at rest.  bench.py is not involved.

Legs (ms per tick, wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs, the legs
taking turns run by run so that drift hits them alike; reported as min - median - max):
  a  the moving board at rest, without lifetimes (as it was);
  b  the same board with all-open lifetimes (0, INT64_MAX): a's bits (the checksums and the task figures are
     compared); b - a is what the presence predicate in the key pass and in the conflict walk costs per tick;
  c  every task open from tick 0, closing at a multiple of 10 drawn from 10 .. 2 x ticks: one tick in ten retires;
  d  closing ticks drawn from 1 .. 2 x ticks: every tick retires.  (d - c) x ticks / (retiring ticks of d - of c)
     is an estimate of the retire pass per retiring tick -- the two legs lose their tasks at the same rate; its byte
     floor is n x Ks x 4 bytes read once;
  e  --long-ticks ticks in calls of --ticks: windows of --window ticks opening evenly over the run, against the same
     tasks without lifetimes at the same slots (no row doubling in this leg: a refusal is the result);
  f  the workaround lifetimes replace: a new board of the present tasks per tick from Python and one-tick calls,
     which also loses every status and table at every tick; --f-ticks ticks, its time only.
Rows are doubled and the run repeated from the same start while a board run of legs a-d is refused.  Results are
merged into --out under --label.

Usage:  python tools/bench_task_lifetimes.py [--agents N] [--legs a,b,c,d,e,f] [--tasks T] [--slots K] [--reps R]
            [--long-ticks L] [--window W] [--f-ticks F] [--label NAME] [--pkg DIR] [--out FILE]
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
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long-ticks", type=int, default=600)
    ap.add_argument("--window", type=int, default=40)
    ap.add_argument("--f-ticks", type=int, default=10)
    ap.add_argument("--legs", default="a,b,c,d,e,f")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_task_lifetimes", "task_lifetimes.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    legs = [k for k in "abcdef" if k in a.legs.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=a.tasks)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev).build_graph(1.0)
    n, ticks, rc, rs, T = sw.n, a.ticks, a.radio_radius, a.sense_radius, a.tasks
    graph0 = (sw.row_ptr, sw.col)
    print(f"[bench_task_lifetimes] {a.label}: n={n} Rc={rc} Rs={rs} T={T} legs={legs}", file=sys.stderr, flush=True)
    g = np.random.default_rng(a.seed + 3)  # (bench_loop_tasks.py's draws, in its order)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    gl = np.random.default_rng(a.seed + 29)
    c3 = (d["tx"], d["ty"], d["treq"])
    rest = np.zeros((T, 2))
    zero = np.zeros(T, np.int64)
    every = gl.integers(1, 2 * ticks + 1, T).astype(np.int64)
    tenth = (10 * gl.integers(1, 2 * ticks // 10 + 1, T)).astype(np.int64)
    long_open = (np.arange(T, dtype=np.int64) * max(a.long_ticks - a.window, 1)) // max(T, 1)
    life = {"a_moving_board_at_rest": None, "b_all_open_lifetimes": (zero, np.full(T, FOREVER)),
            "c_closes_on_one_tick_in_ten": (zero, tenth), "d_closes_on_every_tick": (zero, every)}
    slots = {k: [a.slots, a.slots] for k in life}
    pos0 = sw.pos.clone()
    kills = (80, 150)
    kw = dict(obstacles=obs, kill_ticks=kills, seed=5)

    def reset(windows, ks, kt, board=True):
        sw.pos.copy_(pos0)
        sw.row_ptr, sw.col = graph0
        sw._hear = None
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        if board:
            lo, hi = windows if windows is not None else (None, None)
            sw.set_task_board(*c3, status_slots=ks, table_slots=kt, velocities=rest, open_tick=lo, close_tick=hi)
        torch.cuda.synchronize()

    def refusing(name):
        while True:
            try:
                return sw.update_loop_board(ticks, rc, rs, **kw)
            except _lib.SwarmError as err:
                if err.code != _lib.ERR_RANGE or sw.last_board_overflow is None:
                    raise
                kind = sw.last_board_overflow[0]
                slots[name][0 if kind == "status" else 1] *= 2
                print(f"[bench_task_lifetimes] {name}: {kind} rows full at tick {sw.last_refused_tick}, now "
                      f"{slots[name]}", file=sys.stderr, flush=True)
                reset(life[name], *slots[name])

    def figures(tc, guard):
        b = sw.board
        return {"claims_sent": int(tc[:, 0].sum()), "claims_handled_by_a_leader": int(tc[:, 1].sum()),
                "conflicts_sent": int(tc[:, 2].sum()), "guard_pairs": int(guard), "status_slots": b["Ks"],
                "table_slots": b["Kt"], "peak_status_entries_per_agent": int((b["status"] >= 0).sum(1).max()),
                "status_entries": int((b["status"] >= 0).sum()),
                "peak_table_entries_per_agent": int((b["tab_task"] >= 0).sum(1).max())}

    names = [k for k in life if k[0] in legs]
    res = {"agents": n, "ticks": ticks, "kill_ticks": list(kills), "radio_radius": rc, "sense_radius": rs, "tasks": T,
           "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; the legs take "
                   "turns run by run; min - median - max of the timed runs"}
    times = {k: [] for k in names}
    sums = {}
    for rep in range(a.reps + 1):  # the first round is the warm-up (and finds the rows that fit)
        for k in names:
            reset(life[k], *slots[k])
            t0 = time.perf_counter()
            r = refusing(k)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / ticks
            print(f"[bench_task_lifetimes] {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick", file=sys.stderr,
                  flush=True)
            if rep:
                times[k].append(ms)
            sums[k] = [float(sw.pos[:, 0].sum()), float(sw.pos[:, 1].sum())]
            res[k + "_tasks"] = figures(r["task_counts"], r["guard"])
            if life[k] is not None:
                hi = life[k][1]
                res[k + "_tasks"]["retiring_ticks"] = int(np.unique(hi[hi <= ticks]).size) + 1  # (+ the first tick)
                res[k + "_tasks"]["tasks_present_at_the_end"] = int(sw.board_present(ticks).sum())
    res["ms_per_tick"] = {k: [min(v), float(np.median(v)), max(v)] for k, v in times.items() if v}
    res["pos_checksum"] = sums
    med = {k[0]: float(np.median(v)) for k, v in times.items() if v}
    ka, kb = "a_moving_board_at_rest", "b_all_open_lifetimes"
    if ka in sums and kb in sums:
        assert sums[ka] == sums[kb], ("legs a and b ended differently", sums)
        fa, fb = dict(res[ka + "_tasks"]), dict(res[kb + "_tasks"])
        for key in ("retiring_ticks", "tasks_present_at_the_end"):
            fb.pop(key)
        assert fa == fb, (fa, fb)
        if "a" in med:
            res["all_open_lifetimes_ms_per_tick"] = med["b"] - med["a"]
    if "c" in med and "d" in med:
        rc_, rd_ = (res[k + "_tasks"]["retiring_ticks"]
                    for k in ("c_closes_on_one_tick_in_ten", "d_closes_on_every_tick"))
        res["retire_pass_ms_per_retiring_tick_estimate"] = (med["d"] - med["c"]) * ticks / (rd_ - rc_)
        res["retire_pass_byte_floor_bytes"] = int(n) * slots["d_closes_on_every_tick"][0] * 4

    if "e" in legs:  # a long run at --slots: with windows, and the same tasks always present
        windows = (long_open, long_open + a.window)
        out = {}
        for name, w in (("with_lifetimes", windows), ("without_lifetimes", None)):
            reset(w, a.slots, a.slots)
            done, t0, tc = 0, time.perf_counter(), []
            try:
                while done < a.long_ticks:
                    r = sw.update_loop_board(min(ticks, a.long_ticks - done), rc, rs, **kw)
                    tc.append(r["task_counts"])
                    done = sw.fsm_tick
                refused = None
            except _lib.SwarmError as err:
                if err.code != _lib.ERR_RANGE or sw.last_board_overflow is None:
                    raise
                refused = [sw.last_board_overflow[0], int(sw.last_refused_tick)]
            torch.cuda.synchronize()
            out[name] = {"ticks_run": int(sw.fsm_tick), "refused": refused, "seconds": time.perf_counter() - t0,
                         **(figures(np.concatenate(tc), 0) if tc else {})}
            print(f"[bench_task_lifetimes] e {name}: {out[name]}", file=sys.stderr, flush=True)
        res["e_long_run"] = {"ticks": a.long_ticks, "window": a.window, "slots": a.slots, **out}

    if "f" in legs:  # a new board per tick from Python: every status and table is lost at every tick
        lo, hi = zero, every
        reset(None, a.slots, a.slots, board=False)
        ft, fs = [], a.slots
        for t in range(1, a.f_ticks + 1):
            t0 = time.perf_counter()
            here = (lo <= t) & (t < hi)
            while True:  # (rows that one tick of a fresh board overflows are doubled, inside the tick's time)
                sw.set_task_board(c3[0][here], c3[1][here], c3[2][here], status_slots=fs, table_slots=fs)
                try:
                    sw.update_loop_board(1, rc, rs, obstacles=obs, seed=5)
                    break
                except _lib.SwarmError as err:
                    if err.code != _lib.ERR_RANGE or sw.last_board_overflow is None:
                        raise
                    fs *= 2
            torch.cuda.synchronize()
            ft.append((time.perf_counter() - t0) * 1e3)
        ft = ft[1:]  # (the first tick warms up)
        res["f_new_board_per_tick_ms_per_tick"] = [min(ft), float(np.median(ft)), max(ft)]
        res["f_slots"] = fs
        print(f"[bench_task_lifetimes] f: {res['f_new_board_per_tick_ms_per_tick']}", file=sys.stderr, flush=True)

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
