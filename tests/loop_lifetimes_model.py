"""CPU model of task lifetimes (contract U1-A) -- TESTS ONLY.

A thin driver over the unchanged loop_tasks_model / loop_lossy_model, one tick at a time through start=, as
test_moving_tasks._drive drives a moving board.  Task k is present at tick t iff open[k] <= t < close[k].
  - Before tick t the absent tasks' task_x / task_y are NaN: the model's far test `d2 <= 36` is then false for
    them, so they are offered neither to the claim evaluation nor to the guard-band count.
  - Before and after every tick the absent tasks' status columns are set to OPEN.  Before: `del self.tasks[k]` at
    the tick a task closes (the entries a retiring tick removes).  After: the model's conflict delivery knows no
    lifetimes and writes the status of a task the receiver no longer has.  Fact 1 of DESIGN 4i says that conflict
    delivery writes only statuses and commutes with the rest of the receive -- claims are arbitrated from the
    tables alone -- and an absent task is not evaluated afterwards, so nothing in the tick reads those columns:
    zeroing them equals ignoring the conflicts about them (agent.py:332, 335).
  - Claims are untouched: a TASK_CLAIM about a task that has closed since it was sent is arbitrated from its
    payload, the table entry made and the conflict sent (agent.py:304-325 has no guard).  Tables are never purged.
  - Positions advance for every task, absent or not (cur = Q_{t-1} read by tick t, lag one behind).
"""
import numpy as np

import loop_board_model as lbm
import loop_lossy_model
import loop_tasks_model

FOREVER = np.iinfo(np.int64).max


def present(open_tick, close_tick, t):
    return (np.asarray(open_tick, np.int64) <= t) & (t < np.asarray(close_tick, np.int64))


def drive(oracle_mod, q, Q0, V, open_tick, close_tick, ticks, *, first=0, loss=None, loss_seed=0, use_pow=False,
          start=None):
    """The model over case q (the order of its arrays): `first` ticks in one piece (before the hand-out), then
    `ticks` ticks one at a time with the board at Q_0, Q_1, ... and the tasks present at each tick (start: a result
    of this function: goes on from it, with the windows given now).  -> test_moving_tasks._drive's dict; its acc
    also counts `deleted` (status entries removed at the tick their task closed or was found absent) and `dropped`
    ((agent, task) statuses written by conflicts about absent tasks, and ignored)."""
    dt = float(q["dt"])
    run = (lambda g, k, st: loop_tasks_model.run(oracle_mod, g, k, start=st, use_pow=use_pow)) if loss is None else \
        (lambda g, k, st: loop_lossy_model.run(oracle_mod, g, k, start=st, use_pow=use_pow, loss=loss,
                                               loss_seed=loss_seed))
    acc = dict(counts=[], task_counts=[], link_counts=[], peaks=[], singular=0, guard=0, deleted=0, dropped=0) \
        if start is None else {k: (list(v) if isinstance(v, list) else v) for k, v in start["acc"].items()}
    o = None if start is None else start["o"]
    cur = np.array(Q0, np.float64) if start is None else start["cur"]
    lag = cur.copy() if start is None else start["lag"]
    V = np.zeros_like(cur) if V is None else np.asarray(V, np.float64)

    def note(o):
        acc["counts"].append(o["counts"])
        acc["task_counts"].append(o["task_counts"])
        if loss is not None:
            acc["link_counts"].append(o["link_counts"])
        acc["singular"] += o["singular"]
        acc["guard"] += o["guard"]
    if first:
        o = run(q, first, o)
        note(o)
    g = dict(q)
    for _ in range(ticks):
        t = (0 if o is None else int(o["tick"])) + 1
        gone = ~present(open_tick, close_tick, t)
        if o is not None and o.get("tasks"):
            st = o["tasks"]["status"]
            acc["deleted"] += int((st[:, gone] != 0).sum())
            st[:, gone] = 0
        g["task_x"], g["task_y"] = np.where(gone, np.nan, cur[:, 0]), np.where(gone, np.nan, cur[:, 1])
        o = run(g, 1, o)
        st = o["tasks"]["status"]
        assert st is o["status"]
        acc["dropped"] += int((st[:, gone] != 0).sum())
        st[:, gone] = 0
        note(o)
        acc["peaks"].append(lbm.peak_slots(o))
        lag, cur = cur, cur + V * dt
    return dict(o=o, acc=acc, cur=cur, lag=lag)
