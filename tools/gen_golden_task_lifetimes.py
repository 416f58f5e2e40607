#!/usr/bin/env python3
"""Generate tests/golden/loop_lifetime_board_n200.npz: REAL reference agents on a board of 300 tasks that OPEN and
CLOSE during the run (build container only).  The loop is tools/gen_golden_loop_tasks.py's ref_loop_tasks with its
before_tick hook, as tools/gen_golden_moving_tasks.py uses it.  Contract U1-A: task k is present at
tick t iff open[k] <= t < close[k]; before tick t the hook does, at every agent, `del a.tasks[k]` for every k that
stops being present and `a.tasks[k] = {'status': 'OPEN', ...}` for every k that becomes present -- the reference's
`tasks` is a dict its simulator fills and empties from outside (agent.py:41-44), _process_tasks walks whatever is
in it (292-302), _handle_task_conflict guards its writes with `if task_id in self.tasks` (332, 335) and
_handle_task_claim has no such guard (304-325).  A few tasks also move (contract U1-M: tick t reads Q_{t-1}, every
task advances, present or not).

Each agent's `tasks` is a dict subclass whose only addition is __missing__: the harness's observers and its final
read-out index a.tasks[k] for every k, and an absent task reads as OPEN there; `in`, iteration, `del` and item
assignment -- all the reference uses -- are dict's own.

Only data is written: loop_board_n200's keys, plus open_tick / close_tick, task_vx / task_vy, the positions after
the last tick and the run's figures (life_counts).  tests/golden/index.json is not touched.

Usage:  python tools/gen_golden_task_lifetimes.py [--task-seed S]   (with a seed: figures only, nothing written)
"""
from __future__ import annotations

import argparse
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402
import gen_golden_loop as ggl  # noqa: E402
import gen_golden_loop_board as ggb  # noqa: E402
import gen_golden_loop_tasks as ggt  # noqa: E402

NAME, N_TASKS, TASK_SEED, V_MAX, MAX_BYTES = "loop_lifetime_board_n200", 300, 4242, 3.0, 790802
FOREVER = np.iinfo(np.int64).max
COUNT_KEYS = ("handled", "deleted", "handled_at_close", "dropped", "opened", "closed", "guard")
CONDITIONS = "all four statuses at the end; leader-handled claims >= 100; status entries deleted by closes >= 20; " \
             "a claim handled by a leader on the tick its task closed; a conflict dropped at a receiver for " \
             "absence; no evaluated pair inside the guard band"


class Tasks(dict):
    def __missing__(self, key):  # (read-outs only: nothing is inserted)
        return {"status": "OPEN"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task-seed", type=int, default=None, help="try another task seed (nothing is written)")
    args = ap.parse_args()
    mod = gg.load_reference()
    c = ggt.TASK_CASES["loop_tasks_n200"]
    seed = TASK_SEED if args.task_seed is None else args.task_seed
    t0 = time.time()
    inp = ggl.make_loop_inputs(c)
    inp["sense_radius"] = np.float64(c["sense_radius"])
    inp["radio_radius"] = np.float64(ggt.RADIO_RADIUS)
    dt, ticks = float(inp["dt"]), int(inp["ticks"])
    q = {}
    n = dict(deleted=0, handled_at_close=0, dropped=0, opened=0, closed=0)
    now = [0]

    def entry(board, k):
        e = {"status": "OPEN", "pos": (float(q["x"][k]), float(q["y"][k]))}
        if board["task_req"][k] >= 0:
            e["required_cap"] = ggt.CAP_NAMES[board["task_req"][k]]
        return e

    def life(t, agents, board, trng):
        now[0] = t
        first = not q
        if first:  # the hand-out tick: windows, then velocities, drawn after the board; this tick reads Q_0
            span = ticks - ggt.TASK_TICK
            q["open"] = (ggt.TASK_TICK + trng.integers(0, max(span - 30, 1), N_TASKS)).astype(np.int64)
            q["open"][trng.uniform(size=N_TASKS) < 0.25] = ggt.TASK_TICK  # a quarter is there from the hand-out
            q["close"] = q["open"] + trng.integers(12, 60, N_TASKS)
            q["close"][trng.uniform(size=N_TASKS) < 0.2] = FOREVER  # some never close
            moving = trng.uniform(size=N_TASKS) < 0.1  # a few move
            q["vx"] = np.where(moving, trng.uniform(-V_MAX, V_MAX, N_TASKS), 0.0)
            q["vy"] = np.where(moving, trng.uniform(-V_MAX, V_MAX, N_TASKS), 0.0)
            q["x"], q["y"] = board["task_x"].copy(), board["task_y"].copy()
            for a in agents:
                a.tasks = Tasks(a.tasks)

                def conflict(sender, payload, a=a, seen=a._handle_task_conflict):
                    k = mod.struct.unpack("!II" if len(payload) == 8 else "!IB", payload)[0]
                    if k not in a.tasks:
                        n["dropped"] += 1
                    seen(sender, payload)
                a._handle_task_conflict = conflict

                def claim(sender, payload, a=a, seen=a._handle_task_claim):
                    k = struct.unpack("!If", payload)[0]
                    if a.state == mod.AgentState.LEADER and q["close"][k] == now[0]:
                        n["handled_at_close"] += 1
                    seen(sender, payload)
                a._handle_task_claim = claim
        else:
            q["x"] = q["x"] + q["vx"] * dt
            q["y"] = q["y"] + q["vy"] * dt
        was = np.ones(N_TASKS, bool) if first else (q["open"] <= t - 1) & (t - 1 < q["close"])
        here = (q["open"] <= t) & (t < q["close"])
        n["opened"] += 0 if first else int((here & ~was).sum())
        n["closed"] += 0 if first else int((was & ~here).sum())
        for a in agents:
            for k in np.flatnonzero(was & ~here):
                if not first:
                    n["deleted"] += a.tasks[int(k)]["status"] != "OPEN"
                del a.tasks[int(k)]
            for k in np.flatnonzero(here & ~was):
                a.tasks[int(k)] = entry(board, int(k))
            for k in np.flatnonzero(here & ((q["vx"] != 0.0) | (q["vy"] != 0.0))):
                a.tasks[int(k)]["pos"] = (float(q["x"][k]), float(q["y"][k]))

    out, s = ggt.ref_loop_tasks(mod, inp, seed, n_tasks=N_TASKS, before_tick=life)
    present = sorted(set(out["status_out"].ravel().tolist()))
    n.update(handled=int(s["handled"]), guard=int(s["guard"]))
    print(NAME, "task seed", seed, "| statuses", present, "leader-handled claims", s["handled"],
          "status entries deleted", n["deleted"], "claims handled at the close tick", n["handled_at_close"],
          "conflicts dropped for absence", n["dropped"], "opens", n["opened"], "closes", n["closed"], "claims sent", s["sent"], "guard", s["guard"],
          "statuses at one agent <=", int((out["status_out"] != 0).sum(1).max()), "table entries <=",
          int((out["tab_winner_out"] >= 0).sum(1).max()), "%.1fs" % (time.time() - t0), flush=True)
    ok = present == [0, 1, 2, 3] and s["handled"] >= 100 and n["deleted"] >= 20 and n["handled_at_close"] >= 1 and \
        n["dropped"] >= 1 and s["guard"] == 0
    if args.task_seed is not None:
        print("   conditions", "met" if ok else "MISSED")
        return
    assert ok, CONDITIONS
    arrays = dict(inp)
    arrays.update(out)
    for k in ("claim_out", "conflict_out"):  # the 64-bit words cannot hold a board of 300
        del arrays[k]
    arrays.update(claim_idx=ggb.index_rows(s["claim_sets"]), conflict_idx=ggb.index_rows(s["conflict_sets"]),
                  task_vx=q["vx"], task_vy=q["vy"], task_x_end=q["x"] + q["vx"] * dt, task_y_end=q["y"] + q["vy"] * dt,
                  open_tick=q["open"], close_tick=q["close"],
                  life_counts=np.array([n[k] for k in COUNT_KEYS], np.int64))
    path = os.path.join(gg.OUT, NAME + ".npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < MAX_BYTES, os.path.getsize(path)
    print("   wrote", os.path.relpath(path, gg.ROOT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
