#!/usr/bin/env python3
"""Generate tests/golden/loop_stream_board_n200.npz: REAL reference agents served an unbounded stream of tasks, every
arrival under a FRESH dict key (build container only).  The loop is tools/gen_golden_loop_tasks.py's ref_loop_tasks
with its before_tick hook, as tools/gen_golden_task_lifetimes.py uses it: before tick t the hook does, at every
agent, `del a.tasks[key]` for every life that stops being present and `a.tasks[key] = {...}` for every life that
becomes present.  Contract U1-P says that a board of SLOTS indices whose closed slots are re-placed
computes the same run; so next to the reference's run over one key per life the fixture records the *slot map*: the
arrivals are placed every PLACE_EVERY ticks into the lowest slots the quiet rule allows (absent at the last tick run
and at the one before), an arrival that finds no slot waits for the next place.  The schedule is drawn before the
run (it depends on windows only), so the reference never sees a slot: its task ids are the life numbers.

Lives 0 .. SLOTS - 1 are the board's first tenants (life k in slot k; the later ones of them never present, spare
slots); lives from SLOTS on arrive by place.  A few lives move (contract U1-M).

Only data is written: loop_board_n200's keys over the lives, plus per life its slot, the tick of its place, its
window, velocity and the run's figures (stream_counts).  tests/golden/index.json is not touched.

Usage:  python tools/gen_golden_task_stream.py [--task-seed S]   (with a seed: figures only, nothing written)
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402
import gen_golden_loop as ggl  # noqa: E402
import gen_golden_loop_board as ggb  # noqa: E402
import gen_golden_loop_tasks as ggt  # noqa: E402

NAME, SLOTS, FIRST_TENANTS, ARRIVALS, PLACE_EVERY, V_MAX, MAX_BYTES = "loop_stream_board_n200", 120, 70, 560, 3, 3.0, 400000
SEEDS = tuple(range(5150, 5190))  # tried in order: the first that meets CONDITIONS is the fixture's
COUNT_KEYS = ("lives", "placed", "waited", "most_lives_in_a_slot", "reuses", "stale_reuses", "stale_entries",
              "other_winner", "other_winner_within_hysteresis", "handled", "guard")
CONDITIONS = "all four statuses at the end; a slot that holds at least three lives; a reuse that finds a stale table " \
             "entry about its slot; a life won by another agent than the stale entry's winner, at a leader that held " \
             "that entry -- one of them with a utility the old entry's hysteresis would have refused; an arrival " \
             "that waited for a slot; no evaluated pair inside the guard band"


FOREVER = np.iinfo(np.int64).max


class Tasks(dict):
    def __missing__(self, key):  # (read-outs only: nothing is inserted)
        return {"status": "OPEN"}


def eligible(lo, hi, last):
    return (hi < last) | (lo > last) | (lo == hi)


def schedule(seed, first_tick, ticks):
    """The stream, from windows alone: per life its slot, place tick (-1: a first tenant), window, and whether it
    waited.  Arrivals that find no slot before the run ends never become lives."""
    rng = np.random.default_rng(seed)
    lo, hi = np.zeros(SLOTS, np.int64), np.zeros(SLOTS, np.int64)
    lo[:FIRST_TENANTS] = first_tick
    hi[:FIRST_TENANTS] = first_tick + rng.integers(12, 41, FIRST_TENANTS)
    hi[:FIRST_TENANTS][rng.uniform(size=FIRST_TENANTS) < 0.2] = FOREVER  # some never close: their slots stay taken
    life = dict(slot=list(range(SLOTS)), place=[-1] * SLOTS, open=lo.tolist(), close=hi.tolist(),
                waited=[False] * SLOTS)
    want = np.sort(rng.integers(first_tick + 1, ticks - 14, ARRIVALS))
    burst = rng.choice(ARRIVALS, 90, replace=False)  # a crowd at one tick: more than the free slots
    want[burst] = first_tick + (ticks - first_tick) // 2
    want = np.sort(want)
    length = rng.integers(12, 41, ARRIVALS)
    delay = rng.choice([0, 0, 0, 1, 2], ARRIVALS)
    forever = rng.uniform(size=ARRIVALS) < 0.04
    queue, nxt, left = [], 0, set()
    holds = np.ones(SLOTS, np.int64)
    holds[FIRST_TENANTS:] = 0
    for last in range(first_tick + 1, ticks, PLACE_EVERY):
        while nxt < ARRIVALS and want[nxt] <= last + 1:
            queue.append(nxt)
            nxt += 1
        free = np.flatnonzero(eligible(lo, hi, last))
        for k, a in zip(free, queue):
            o = last + 1 + int(delay[a])
            lo[k], hi[k] = o, FOREVER if forever[a] else o + int(length[a])
            holds[k] += 1
            life["slot"].append(int(k)), life["place"].append(last), life["open"].append(o)
            life["close"].append(int(hi[k])), life["waited"].append(a in left)
        queue = queue[len(free):]
        left.update(queue)  # no slot at this place: they wait for the next
    out = {k: np.asarray(v) for k, v in life.items()}
    out["most"] = int(holds.max())
    return out


def run(mod, seed):
    c = ggt.TASK_CASES["loop_tasks_n200"]
    inp = ggl.make_loop_inputs(c)
    inp["sense_radius"] = np.float64(c["sense_radius"])
    inp["radio_radius"] = np.float64(ggt.RADIO_RADIUS)
    dt, ticks = float(inp["dt"]), int(inp["ticks"])
    life = schedule(seed, ggt.TASK_TICK, ticks)
    NL = len(life["slot"])
    lo, hi, place = life["open"].astype(np.int64), life["close"].astype(np.int64), life["place"]
    prev = np.full(NL, -1, np.int64)  # the life a placed life takes its slot from
    tenant = {}
    for i in np.argsort(place, kind="stable"):
        prev[i] = tenant.get(int(life["slot"][i]), -1)
        tenant[int(life["slot"][i])] = int(i)
    real = lo != hi
    q, held = {}, {}
    stale = []  # (new life, agent, the old entry's winner, its utility)

    def entry(board, k):
        e = {"status": "OPEN", "pos": (float(q["x"][k]), float(q["y"][k]))}
        if board["task_req"][k] >= 0:
            e["required_cap"] = ggt.CAP_NAMES[board["task_req"][k]]
        return e

    def hook(t, agents, board, trng):
        first = not q
        if first:
            # most arrivals appear near the task their slot held before (within ~1): the leaders that arbitrated
            # the old life then hear about the new one -- the case a stale table entry can spoil
            for k in np.argsort(place, kind="stable"):
                near = trng.uniform() < 0.6
                jx, jy = trng.normal(0.0, 0.7, 2)
                if place[k] >= 0 and prev[k] >= 0 and real[prev[k]] and near:
                    board["task_x"][k] = board["task_x"][prev[k]] + jx
                    board["task_y"][k] = board["task_y"][prev[k]] + jy
            moving = trng.uniform(size=NL) < 0.1
            q["vx"] = np.where(moving, trng.uniform(-V_MAX, V_MAX, NL), 0.0)
            q["vy"] = np.where(moving, trng.uniform(-V_MAX, V_MAX, NL), 0.0)
            q["x"], q["y"] = board["task_x"].copy(), board["task_y"].copy()
            held["agents"] = agents
            for a in agents:
                a.tasks = Tasks(a.tasks)
        else:
            q["x"] = q["x"] + q["vx"] * dt
            q["y"] = q["y"] + q["vy"] * dt
        now = np.flatnonzero(place == t - 1)  # placed after the tick before: this tick reads the placed position
        q["x"][now], q["y"][now] = board["task_x"][now], board["task_y"][now]
        for k in now:
            if prev[k] >= 0 and real[prev[k]]:
                for i, a in enumerate(agents):
                    c = a.task_claims.get(int(prev[k]))
                    if c is not None:
                        stale.append((int(k), i, int(c["winner"]), float(c["utility"])))
        was = np.ones(NL, bool) if first else (lo <= t - 1) & (t - 1 < hi)
        here = (lo <= t) & (t < hi)
        for a in agents:
            for k in np.flatnonzero(was & ~here):
                del a.tasks[int(k)]
            for k in np.flatnonzero(here & ~was):
                a.tasks[int(k)] = entry(board, int(k))
            for k in np.flatnonzero(here & ((q["vx"] != 0.0) | (q["vy"] != 0.0))):
                a.tasks[int(k)]["pos"] = (float(q["x"][k]), float(q["y"][k]))

    out, s = ggt.ref_loop_tasks(mod, inp, seed, n_tasks=NL, before_tick=hook)
    agents = held["agents"]
    other = within = 0
    for k, i, w, u in stale:
        c = agents[i].task_claims.get(k)
        if c is not None and c["winner"] != w:
            other += 1
            within += c["utility"] <= u + 5.0
    reuses = int(real[prev[prev >= 0]].sum())
    n = dict(lives=int(real.sum()), placed=int((place >= 0).sum()), waited=int(life["waited"].sum()),
             most_lives_in_a_slot=life["most"], reuses=reuses, stale_reuses=len({k for k, _, _, _ in stale}),
             stale_entries=len(stale), other_winner=other, other_winner_within_hysteresis=int(within),
             handled=int(s["handled"]), guard=int(s["guard"]))
    present = sorted(set(out["status_out"].ravel().tolist()))
    ok = present == [0, 1, 2, 3] and n["most_lives_in_a_slot"] >= 3 and n["stale_reuses"] >= 1 and other >= 1 and \
        within >= 1 and n["waited"] >= 1 and n["guard"] == 0
    return inp, out, s, life, q, n, present, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task-seed", type=int, default=None, help="try one seed (nothing is written)")
    args = ap.parse_args()
    mod = gg.load_reference()
    for seed in SEEDS if args.task_seed is None else (args.task_seed,):
        t0 = time.time()
        inp, out, s, life, q, n, present, ok = run(mod, seed)
        print(NAME, "task seed", seed, "| statuses", present, n, "claims sent", s["sent"], "statuses at one agent <=",
              int((out["status_out"] != 0).sum(1).max()), "table entries <=",
              int((out["tab_winner_out"] >= 0).sum(1).max()), "%.1fs" % (time.time() - t0),
              "conditions", "met" if ok else "MISSED", flush=True)
        if ok:
            break
    if args.task_seed is not None:
        return
    assert ok, CONDITIONS
    dt = float(inp["dt"])
    arrays = dict(inp)
    arrays.update(out)
    for k in ("claim_out", "conflict_out"):  # the 64-bit words cannot hold this board
        del arrays[k]
    arrays.update(claim_idx=ggb.index_rows(s["claim_sets"]), conflict_idx=ggb.index_rows(s["conflict_sets"]),
                  task_vx=q["vx"], task_vy=q["vy"], task_x_end=q["x"] + q["vx"] * dt, task_y_end=q["y"] + q["vy"] * dt,
                  slots=np.int64(SLOTS), life_slot=life["slot"].astype(np.int32),
                  life_place=life["place"].astype(np.int64), open_tick=life["open"].astype(np.int64),
                  close_tick=life["close"].astype(np.int64), task_seed=np.int64(seed),
                  stream_counts=np.array([n[k] for k in COUNT_KEYS], np.int64))
    path = os.path.join(gg.OUT, NAME + ".npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < MAX_BYTES, os.path.getsize(path)
    print("   wrote", os.path.relpath(path, gg.ROOT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
