#!/usr/bin/env python3
"""Measure a stream of tasks through a board of fixed size (Swarm.place_board_tasks, contract U1-P) on
tools/bench_task_lifetimes.py's setup: the C3 swarm, Rc = Rs = 1.0, kills at 80 / 150, tasks at rest.  bench.py is
not involved.

The stream: --tasks slots, every life --window - 1 ticks long, a quarter of the slots closing just before every
--every-th tick, so that a place every --every ticks re-fills them (a slot is absent for the two ticks the quiet
rule asks for: about 95 % of the slots hold a present task at any tick); new positions uniform over the arena, the
requirements drawn from C3's.  Legs (ms per tick over --ticks ticks in calls of --every, wall clock ended on a
synchronise; one warm-up run per leg, then --reps timed runs, the legs taking turns run by run; min - median - max):
  a  streamed through the slots: update_loop_board(every), place_board_tasks, ...; the place calls are also timed
     on their own (each ends on the library's second wait);
  b  the same lives on a virtual board with one index per life, all windows known in advance (the recommendation
     before U1-P), in the same calls of --every ticks;
  c  a new board of the present tasks per batch from Python (loses every status and table at every batch).
a and b must send, handle and resolve the same number of claims on every tick (contract U1-P.4).  Rows are doubled
and the leg repeated from the start while a run is refused.  The board's device bytes are reported by the formula of
its arrays.  Results are merged into --out under --label.

Usage:  python tools/bench_task_stream.py [--agents N] [--legs a,b,c] [--tasks T] [--ticks K] [--every E]
            [--window W] [--slots S] [--reps R] [--label NAME] [--pkg DIR] [--out FILE]
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
# cur, lag, vel (16 each), the entry snapshot (32), sxy (16), sir (8), open, close (8 each), treq, present (1 each),
# the sort's keys and values twice (4 x 4)
BOARD_BYTES_PER_INDEX = 3 * 16 + 32 + 16 + 8 + 2 * 8 + 2 + 4 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--deg", type=float, default=16.0)
    ap.add_argument("--ticks", type=int, default=600)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--window", type=int, default=40)
    ap.add_argument("--radio-radius", type=float, default=1.0)
    ap.add_argument("--sense-radius", type=float, default=1.0)
    ap.add_argument("--tasks", type=int, default=10_000)
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_task_stream", "task_stream.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    legs = [k for k in "abc" if k in a.legs.split(",")]
    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=a.tasks)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev).build_graph(1.0)
    n, ticks, every, rc, rs, T = sw.n, a.ticks, a.every, a.radio_radius, a.sense_radius, a.tasks
    assert ticks % every == 0 and a.window % every == 0 and a.window >= 2 * every
    phases = a.window // every
    graph0 = (sw.row_ptr, sw.col)
    print(f"[bench_task_stream] {a.label}: n={n} T={T} ticks={ticks} every={every} legs={legs}", file=sys.stderr,
          flush=True)
    g = np.random.default_rng(a.seed + 3)  # (bench_loop_tasks.py's draws, in its order)
    side = float(sw.pos[:, 0].max())
    obs = np.stack([g.uniform(0, side, 16), g.uniform(0, side, 16), g.uniform(0.2, 1.5, 16)], 1)
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    pos0 = sw.pos.clone()
    kills = (80, 150)
    kw = dict(obstacles=obs, kill_ticks=kills, seed=5)

    # the stream: slot k closes just before the ticks every * (j * phases + k % phases + 1) and is placed after them
    gs = np.random.default_rng(a.seed + 33)
    init = dict(x=np.asarray(d["tx"], np.float64), y=np.asarray(d["ty"], np.float64), req=np.asarray(d["treq"]),
                open=np.zeros(T, np.int64), close=(every * (np.arange(T) % phases + 1) - 1).astype(np.int64))
    places = []  # (last, slots, x, y, req, open, close)
    close = init["close"].copy()
    for last in range(every, ticks, every):
        k = np.flatnonzero(close == last - 1)
        m = len(k)
        close[k] = last + a.window - 1
        places.append((last, k, gs.uniform(0, side, m), gs.uniform(0, side, m), gs.choice(init["req"], m),
                       np.full(m, last + 1, np.int64), close[k].copy()))
    lives = T + sum(len(p[1]) for p in places)
    vb = {key: np.concatenate([init[key]] + [p[i] for p in places])
          for key, i in (("x", 2), ("y", 3), ("req", 4), ("open", 5), ("close", 6))}
    slots = {k: [a.slots, a.slots] for k in "abc"}

    def reset():
        sw.pos.copy_(pos0)
        sw.row_ptr, sw.col = graph0
        sw._hear = None
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        torch.cuda.synchronize()

    def board(b, ks, kt):
        sw.set_task_board(b["x"], b["y"], b["req"], status_slots=ks, table_slots=kt, open_tick=b["open"],
                          close_tick=b["close"])

    def leg(name):
        """One run of a leg from the start -> (ms per tick, per-tick task counts, place times in ms, purged)."""
        ks, kt = slots[name]
        reset()
        if name != "c":
            board(init if name == "a" else vb, ks, kt)
        torch.cuda.synchronize()
        t0, tc, pt, purged = time.perf_counter(), [], [], 0
        for call in range(ticks // every):
            if name == "c":  # a new board of the tasks present over the batch
                lo = call * every + 1
                here = (vb["open"] <= lo) & (lo < vb["close"])
                sw.set_task_board(vb["x"][here], vb["y"][here], vb["req"][here], status_slots=ks, table_slots=kt)
            tc.append(sw.update_loop_board(every, rc, rs, **kw)["task_counts"])
            if name == "a" and call < len(places):
                _, k, x, y, req, lo, hi = places[call]
                p0 = time.perf_counter()
                purged += sw.place_board_tasks(k, x, y, req, open_tick=lo, close_tick=hi)["purged"]
                pt.append((time.perf_counter() - p0) * 1e3)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / ticks, np.concatenate(tc), pt, purged

    def refusing(name):
        while True:
            try:
                return leg(name)
            except _lib.SwarmError as err:
                if err.code != _lib.ERR_RANGE or sw.last_board_overflow is None:
                    raise
                kind = sw.last_board_overflow[0]
                slots[name][0 if kind == "status" else 1] *= 2
                print(f"[bench_task_stream] {name}: {kind} rows full at tick {sw.last_refused_tick}, now "
                      f"{slots[name]}", file=sys.stderr, flush=True)

    names = {"a": "a_streamed_through_slots", "b": "b_virtual_board_one_index_per_life", "c": "c_new_board_per_batch"}
    res = {"agents": n, "ticks": ticks, "place_every": every, "window": a.window - 1, "slots_on_the_board": T,
           "lives": int(lives), "kill_ticks": list(kills), "radio_radius": rc, "sense_radius": rs,
           "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; the legs take "
                   "turns run by run; min - median - max of the timed runs"}
    times, counts, place_ms = {k: [] for k in legs}, {}, []
    for rep in range(a.reps + 1):  # the first round is the warm-up (and finds the rows that fit)
        for k in legs:
            ms, tc, pt, purged = refusing(k)
            print(f"[bench_task_stream] {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick", file=sys.stderr,
                  flush=True)
            counts[k] = tc
            if rep:
                times[k].append(ms)
                place_ms += pt
            b = sw.board
            res[names[k]] = {"status_slots": b["Ks"], "table_slots": b["Kt"], "claims_sent": int(tc[:, 0].sum()),
                             "claims_handled_by_a_leader": int(tc[:, 1].sum()), "conflicts_sent": int(tc[:, 2].sum()),
                             "peak_table_entries_per_agent": int((b["tab_task"] >= 0).sum(1).max()),
                             "table_entries": int((b["tab_task"] >= 0).sum()),
                             "board_indices": int(b["T"]), "board_device_bytes": int(b["T"]) * BOARD_BYTES_PER_INDEX,
                             "state_bytes_per_agent": 12 * b["Ks"] + 20 * b["Kt"]}
            if k == "a":
                res[names[k]]["table_entries_purged"] = int(purged)
    res["ms_per_tick"] = {names[k]: [min(v), float(np.median(v)), max(v)] for k, v in times.items() if v}
    if place_ms:
        res["place_call_ms"] = [min(place_ms), float(np.median(place_ms)), max(place_ms)]
        res["place_call_requests"] = int(len(places[0][1]))
        res["purge_pass_byte_floor_bytes"] = int(n) * slots["a"][1] * 4
    if "a" in counts and "b" in counts:
        assert np.array_equal(counts["a"], counts["b"]), "legs a and b counted differently"
        res["a_equals_b_on_every_ticks_counts"] = True

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
