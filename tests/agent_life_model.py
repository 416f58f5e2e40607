"""CPU model of agent lifetimes on the radio and task loops (contract U1-J) -- TESTS ONLY.

A thin driver over the unchanged loop_radio_model.run(..., start=) -- or, with a board (task_x in g) or a lossy
channel (loss=), over loop_lossy_model.run(..., start=), the model of the task loop and of the channel -- one tick
at a time, in the style of loop_lifetimes_model.py: before tick t it applies to the model's state dict the edits
the contract names -- the agents with death == t lose their alive flag and nothing else; the agents with boot == t
become a fresh SwarmAgent constructed at the clock of tick t - 1 (FOLLOWER, leader -1, no leader position,
last_hb = (t - 1) dt, wait_start = delay = 0, tick_off = 1 - t, velocity 0, no target, both outbox halves empty;
on a board every status OPEN, an empty claim table, no claim or conflict of either of the last two ticks in
flight) at the position they stand at.  oracle/ is untouched.  The rows' order is the order of the arrays: run it
over the storage order to predict the GPU.
"""
import numpy as np

import loop_lossy_model
import loop_radio_model
from loop_model import F
from loop_tasks_model import fresh_tasks

FOREVER = np.iinfo(np.int64).max


def up(boot, death, t):
    return (np.asarray(boot) <= t) & (t < np.asarray(death))


def fresh(oracle, g):
    """The state dict of a run that has not started: loop_radio_model.run's start= form at tick 0."""
    ids = np.asarray(g["ids"], np.int32)
    n = len(ids)
    z = np.zeros(n + 1, np.int64)
    fsm = oracle.protocol(ids, g["x"], g["y"], z, np.zeros(0, np.int32), g["tick_off"], 0, last_hb=g["last_hb0"])
    fsm.pop("counts")
    fsm.update({k: np.array(v) for k, v in g.get("fsm0", {}).items()})
    x, y = np.array(g["x"], np.float64), np.array(g["y"], np.float64)
    return dict(tick=0, fsm=fsm, tasks=fresh_tasks(n, len(np.asarray(g.get("task_x", ())))), x=x, y=y,
                px=x.copy(), py=y.copy(), vx=np.zeros(n), vy=np.zeros(n),
                tx=np.array(g["tx"], np.float64), ty=np.array(g["ty"], np.float64),
                has_t=np.array(g["has_t"], np.uint8), tick_off=np.array(g["tick_off"], np.int32))


def set_time(o, boot, death):
    """The set-time rule at the last tick run: whoever is not up loses its alive flag, nothing else is written."""
    o["fsm"]["alive"][~up(boot, death, o["tick"])] = 0
    return o


def events(o, t, boot, death, dt):
    """The start of tick t: deaths, then boots, on the state dict; returns (booted, died)."""
    boot, death = np.asarray(boot), np.asarray(death)
    live = boot < death
    dies, boots = live & (death == t), live & (boot == t)
    f = o["fsm"]
    n = len(boot)
    f["alive"][dies] = 0
    f["alive"][boots] = 1
    f["state"][boots] = F
    f["leader"][boots] = -1
    f["lpos"][boots] = 0.0
    f["has_lpos"][boots] = 0
    f["last_hb"][boots] = float(t - 1) * dt
    f["wait_start"][boots] = 0.0
    f["delay"][boots] = 0.0
    f["outbox"][:n][boots] = 0
    f["outbox"][n:][boots] = 0
    o["tick_off"][boots] = 1 - t
    for k in ("vx", "vy", "tx", "ty", "has_t"):
        o[k][boots] = 0
    tk = o.get("tasks")
    if tk is not None:
        tk["status"][boots] = 0  # OPEN
        tk["tab_winner"][boots] = -1
        tk["tab_util"][boots] = 0.0
        for i in np.flatnonzero(boots):
            for k in ("claims", "conflicts", "claims_prev", "conflicts_prev"):
                tk[k][i] = []
    return int(boots.sum()), int(dies.sum())


def drive(oracle, g, boot, death, ticks, *, start=None, on_tick=None, loss=None, loss_seed=0, **kw):
    """Ticks t0+1 .. t0+ticks with the windows (boot, death); start: what this function returned (or fresh());
    on_tick(t, o): called after every tick with the state dict.  -> the state dict, with counts (ticks x 4),
    agent_events (ticks x 2) and tick_off; with a board or loss= also task_counts (ticks x 3), link_counts
    (ticks x 2) and guard."""
    o = fresh(oracle, g) if start is None else start
    dt = float(g["dt"])
    general = loss is not None or len(np.asarray(g.get("task_x", ()))) > 0
    counts, ev, singular, tcounts, lcounts, guard = [], [], 0, [], [], 0
    for _ in range(int(ticks)):
        t = int(o["tick"]) + 1
        tick_off = o["tick_off"]
        ev.append(events(o, t, boot, death, dt))
        if general:
            o = loop_lossy_model.run(oracle, dict(g, tick_off=tick_off), 1, start=o, loss=loss or 0.0,
                                     loss_seed=loss_seed, **kw)
            tcounts.append(o["task_counts"])
            lcounts.append(o["link_counts"])
            guard += o["guard"]
        else:
            o = loop_radio_model.run(oracle, dict(g, tick_off=tick_off), 1, start=o, **kw)
        o["tick_off"] = tick_off
        counts.append(o["counts"])
        singular += o["singular"]
        if on_tick:
            on_tick(t, o)
    o["counts"] = np.concatenate(counts) if counts else np.zeros((0, 4), np.int64)
    o["agent_events"] = np.array(ev, np.int64).reshape(-1, 2)
    o["singular"] = singular
    if general:
        o["task_counts"] = np.concatenate(tcounts) if tcounts else np.zeros((0, 3), np.int64)
        o["link_counts"] = np.concatenate(lcounts) if lcounts else np.zeros((0, 2), np.int64)
        o["guard"] = guard
    return o
