"""CPU model of the radio update loop (contract U1-R) -- TESTS ONLY.

loop_sensed_model.run's per-tick composition (oracle.protocol over P_{t-2}, then oracle.physics on the agents
and their leader-position phantoms, the sensor CSR rebuilt from P_{t-1} at the sensing radius) with the
message CSR rebuilt as well, at the top of every tick, from that tick's P_{t-1} at the radio radius: agent i
hears j != i iff dx*dx + dy*dy <= Rc*Rc (fp64, the products rounded separately), rows in ascending index
(loop_sensed_model.sense_csr: the same rule at another radius).  oracle.protocol delivers a row's packets in
row order and takes a heartbeat's position from the arrays it is given, P_{t-2}: who hears is judged on
P_{t-1}, what is heard was packed a tick earlier.  The rows' order is the order of the arrays: run it over the
storage order to predict the GPU.
reradio=False keeps the message graph of the input for the whole run: U1-S, the absence of the feature;
with resense=False as well the sensors are that graph's rows too: U1 (update_loop with its default sensors),
so that a run chained over the three loops can be modelled chunk by chunk (start=).
use_pow as loop_model.run: True equals real SwarmAgent objects bit for bit (tests/golden/loop_radio_*.npz,
tools/gen_golden_loop_radio.py), False is the GPU's x*x arithmetic.
"""
import numpy as np

from loop_model import FSM_KEYS, F, L
from loop_sensed_model import sense_csr


def run(oracle, g, ticks=None, *, radio_radius=None, radius=None, use_pow=False, reradio=True, resense=True,
        timeout=3.0, jitter=0.2, start=None):
    """Ticks 1 .. ticks of U1-R from a fixture-style input dict g (loop_sensed_model.run's keys plus
    radio_radius; row_ptr / col are read only with reradio=False) -> loop_sensed_model.run's dict, plus
    max_heard, the longest radio row of the run.  start: a dict this function
    returned after t0 = start["tick"] ticks -- the run goes on from there with ticks t0+1 .. t0+ticks."""
    assert reradio or "row_ptr" in g, "reradio=False needs the input's message graph"
    ids = np.asarray(g["ids"], np.int32)
    n = len(ids)
    ticks = int(g["ticks"]) if ticks is None else int(ticks)
    if resense:
        radius = float(g["sense_radius"]) if radius is None else float(radius)
    if reradio:
        rc = float(g["radio_radius"]) if radio_radius is None else float(radio_radius)
    dt, ms, seed = float(g["dt"]), float(g["max_speed"]), int(g["seed"])
    if reradio:
        rp, col = np.zeros(n + 1, np.int64), np.zeros(0, np.int32)
    else:
        rp, col = np.asarray(g["row_ptr"], np.int64), np.asarray(g["col"], np.int32)
    t0 = 0
    if start is None:
        x, y = np.array(g["x"], np.float64), np.array(g["y"], np.float64)
        px, py = x.copy(), y.copy()
        vx, vy = np.zeros(n), np.zeros(n)
        tx, ty = np.array(g["tx"], np.float64), np.array(g["ty"], np.float64)
        has_t = np.array(g["has_t"], np.uint8)
        fsm = dict(last_hb=np.array(g["last_hb0"], np.float64))
        fsm.update({k: np.array(v) for k, v in g.get("fsm0", {}).items()})  # oracle.protocol's state keywords
    else:
        t0 = int(start["tick"])
        x, y, px, py, vx, vy, tx, ty = (np.array(start[k], np.float64) for k in
                                        ("x", "y", "px", "py", "vx", "vy", "tx", "ty"))
        has_t = np.array(start["has_t"], np.uint8)
        fsm = {k: np.array(v) for k, v in start["fsm"].items()}  # the outbox halves included
    counts = np.zeros((ticks, 4), np.int64)
    singular, max_row, max_heard = 0, 0, 0
    ids2 = np.concatenate([ids, ids])
    lead_rows = np.arange(n, 2 * n, dtype=np.int32)
    z = np.zeros(n)
    for t in range(t0 + 1, t0 + ticks + 1):
        if reradio:  # who hears whom at this tick: the radius graph of P_{t-1}
            rp, col = sense_csr(oracle, x, y, rc)
            max_heard = max(max_heard, int(np.diff(rp).max()) if n else 0)
        o = oracle.protocol(ids, px, py, rp, col, g["tick_off"], 1, t0=t - 1, dt=dt, timeout=timeout,
                            jitter=jitter, seed=seed, kill_ticks=g["kill_ticks"], **fsm)
        counts[t - t0 - 1] = o.pop("counts")[0]
        fsm = o
        alive = fsm["alive"] != 0
        follows = alive & (fsm["state"] == F) & (fsm["has_lpos"] != 0)
        lp = fsm["lpos"].astype(np.float64)
        srp, scol = sense_csr(oracle, x, y, radius) if resense else (rp, col)
        max_row = max(max_row, int(np.diff(srp).max()) if n else 0)
        ph = oracle.physics(
            ids2, np.concatenate([fsm["state"], np.full(n, L, np.uint8)]),
            np.concatenate([np.where(follows, lead_rows, -1).astype(np.int32), np.full(n, -1, np.int32)]),
            np.concatenate([x, lp[:, 0]]), np.concatenate([y, lp[:, 1]]), np.concatenate([vx, z]),
            np.concatenate([vy, z]), np.concatenate([tx, z]), np.concatenate([ty, z]),
            np.concatenate([np.where(alive, has_t, 0).astype(np.uint8), np.zeros(n, np.uint8)]),
            g["obs"], np.concatenate([srp, np.full(n, srp[-1], np.int64)]), scol, dt=dt, max_speed=ms, steps=1,
            use_pow=use_pow)
        singular += ph["singular"]
        px, py = x, y
        x, y, vx, vy, tx, ty = (ph[k][:n].copy() for k in ("x", "y", "vx", "vy", "tx", "ty"))
        has_t = np.where(alive, ph["has_t"][:n], has_t).astype(np.uint8)
    out = {k: fsm[k] for k in FSM_KEYS} if "state" in fsm else {}
    out.update(fsm=fsm, x=x, y=y, vx=vx, vy=vy, tx=tx, ty=ty, has_t=has_t, counts=counts, singular=singular,
               px=px, py=py, max_row=max_row, max_heard=max_heard, tick=t0 + ticks)
    return out
