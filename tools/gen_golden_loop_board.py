#!/usr/bin/env python3
"""Generate tests/golden/loop_board_n200.npz: REAL reference agents on a board of 300 tasks (build container
only).  The loop is tools/gen_golden_loop_tasks.py's ref_loop_tasks, unchanged but for the board's size:
loop_tasks_n200's agents, kills and radii, 300 tasks handed to every agent at tick 45 over the bounding box of
the positions at that moment.  Contract U1-B is U1-T on such a board.

Only data is written: loop_tasks_n200's input keys, the board, the final statuses (n x 300 codes), every agent's
task_claims as dense tables, the per-tick task counts, and the claim and conflict sets of the last two ticks as
index lists -- claim_idx / conflict_idx, rows of (tick parity, agent, task) in ascending order; the 64-bit words
of the 64-task fixtures cannot hold them.  tests/golden/index.json is not touched.

The tool asserts, over the tasks with index 64 and above only, what the fixture must exercise (CONDITIONS), and
that the file stays below the largest fixture committed so far.  Task seeds were tried until the conditions
held; TASK_SEED records the one in use.

Usage:  python tools/gen_golden_loop_board.py [--task-seed S]   (with a seed: figures only, nothing written)
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
import gen_golden_loop_tasks as ggt  # noqa: E402

NAME, N_TASKS, FROM, TASK_SEED, MAX_BYTES = "loop_board_n200", 300, 64, 4242, 790802
CONDITIONS = "over tasks >= 64: all four statuses at the end; leader-handled claims >= 20; hysteresis " \
             "replacements >= 2; re-affirmations >= 5; statuses overwritten by a later conflict >= 2; no " \
             "evaluated pair inside the guard band"


def index_rows(sets):
    """[parity][agent] -> set of tasks, as int32 rows (parity, agent, task) in ascending order."""
    rows = [(h, i, k) for h in (0, 1) for i, s in enumerate(sets[h]) for k in sorted(s)]
    return np.asarray(rows, np.int32).reshape(-1, 3)


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
    out, s = ggt.ref_loop_tasks(mod, inp, seed, n_tasks=N_TASKS, stat_from=FROM)
    hi = out["status_out"][:, FROM:]
    present = sorted(set(hi.ravel().tolist()))
    print(NAME, "task seed", seed, "| tasks >= 64: statuses", present, "leader-handled claims", s["handled"],
          "replacements", s["replaced"], "re-affirmations", s["reaffirmed"], "overwritten statuses", s["overwritten"],
          "claims no leader handled", s["unheard"], "tasks touched", int((hi != 0).any(0).sum()),
          "smallest |U - 20| %.2g" % s["min_gap"], "guard", s["guard"], "| all tasks: claims sent", s["sent"],
          "handled", int(out["task_counts"][:, 1].sum()), "conflicts", int(out["task_counts"][:, 2].sum()),
          "statuses at one agent <=", int((out["status_out"] != 0).sum(1).max()), "table entries <=",
          int((out["tab_winner_out"] >= 0).sum(1).max()), "%.1fs" % (time.time() - t0), flush=True)
    ok = (present == [0, 1, 2, 3] and s["handled"] >= 20 and s["replaced"] >= 2 and s["reaffirmed"] >= 5 and
          s["overwritten"] >= 2 and s["guard"] == 0)
    if args.task_seed is not None:
        print("   conditions", "met" if ok else "MISSED")
        return
    assert ok, CONDITIONS
    arrays = dict(inp)
    arrays.update(out)
    for k in ("claim_out", "conflict_out"):  # the 64-bit words cannot hold a board of 300
        del arrays[k]
    arrays.update(claim_idx=index_rows(s["claim_sets"]), conflict_idx=index_rows(s["conflict_sets"]))
    path = os.path.join(gg.OUT, NAME + ".npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < MAX_BYTES, os.path.getsize(path)
    print("   wrote", os.path.relpath(path, gg.ROOT), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
