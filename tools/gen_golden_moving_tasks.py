#!/usr/bin/env python3
"""Generate tests/golden/loop_moving_board_n200.npz: REAL reference agents on a board of 300 MOVING tasks (build
container only).  The loop is tools/gen_golden_loop_tasks.py's ref_loop_tasks, as tools/gen_golden_loop_board.py
drives it, with one addition: every task has a velocity, and before every tick from the hand-out on each agent's
tasks[k]['pos'] is set to Q_{t-1} -- the reference reads task['pos'] afresh every time _process_tasks runs
(agent.py:292-302, 338-347), so a simulator that moves its targets between ticks is inside its model.  Contract
U1-M: Q_0 is the board at the hand-out (tick 45 reads Q_0), Q_k = fl(Q_{k-1} + fl(v * dt)) per
coordinate, the product and the sum rounded separately (numpy float64: no fused multiply-add).

Only data is written: loop_board_n200's keys, plus task_vx / task_vy and the positions after the last tick
(task_x_end / task_y_end).  tests/golden/index.json is not touched.

Usage:  python tools/gen_golden_moving_tasks.py [--task-seed S]   (with a seed: figures only, nothing written)
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

NAME, N_TASKS, TASK_SEED, V_MAX, MAX_BYTES = "loop_moving_board_n200", 300, 4242, 3.0, 790802
CONDITIONS = "all four statuses at the end; leader-handled claims >= 100; hysteresis replacements >= 2; " \
             "re-affirmations >= 5; no evaluated pair inside the guard band"


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
    dt = float(inp["dt"])
    q = {}

    def move(t, agents, board, trng):
        if not q:  # the hand-out tick: the velocities, drawn after the board; this tick reads Q_0
            q["vx"], q["vy"] = trng.uniform(-V_MAX, V_MAX, N_TASKS), trng.uniform(-V_MAX, V_MAX, N_TASKS)
            q["x"], q["y"] = board["task_x"].copy(), board["task_y"].copy()
            return
        q["x"] = q["x"] + q["vx"] * dt
        q["y"] = q["y"] + q["vy"] * dt
        for a in agents:
            for k in range(N_TASKS):
                a.tasks[k]["pos"] = (float(q["x"][k]), float(q["y"][k]))

    out, s = ggt.ref_loop_tasks(mod, inp, seed, n_tasks=N_TASKS, before_tick=move)
    present = sorted(set(out["status_out"].ravel().tolist()))
    print(NAME, "task seed", seed, "| statuses", present, "leader-handled claims", s["handled"], "replacements",
          s["replaced"], "re-affirmations", s["reaffirmed"], "overwritten statuses", s["overwritten"], "claims sent",
          s["sent"], "guard", s["guard"], "statuses at one agent <=", int((out["status_out"] != 0).sum(1).max()),
          "table entries <=", int((out["tab_winner_out"] >= 0).sum(1).max()), "%.1fs" % (time.time() - t0), flush=True)
    ok = present == [0, 1, 2, 3] and s["handled"] >= 100 and s["replaced"] >= 2 and s["reaffirmed"] >= 5 and \
        s["guard"] == 0
    if args.task_seed is not None:
        print("   conditions", "met" if ok else "MISSED")
        return
    assert ok, CONDITIONS
    arrays = dict(inp)
    arrays.update(out)
    for k in ("claim_out", "conflict_out"):  # the 64-bit words cannot hold a board of 300
        del arrays[k]
    arrays.update(claim_idx=ggb.index_rows(s["claim_sets"]), conflict_idx=ggb.index_rows(s["conflict_sets"]),
                  task_vx=q["vx"], task_vy=q["vy"], task_x_end=q["x"] + q["vx"] * dt, task_y_end=q["y"] + q["vy"] * dt)
    path = os.path.join(gg.OUT, NAME + ".npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < MAX_BYTES, os.path.getsize(path)
    print("   wrote", os.path.relpath(path, gg.ROOT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
