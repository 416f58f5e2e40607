"""CPU model of the coupled update loop (contract U1) -- TESTS ONLY.

It composes the existing oracle per tick, so it needs nothing new under oracle/:
  * oracle.protocol(ticks=1, t0=t-1) over the positions the tick's heartbeats carry, P_{t-2} (a HEARTBEAT
    received at tick t was packed during tick t-1, before that tick's physics);
  * oracle.physics(steps=1) on 2n rows: the n agents at P_{t-1}, then n phantoms at leader_pos[i] widened to
    f64 (float(double(f32)) is the identity, so the phantom reproduces the '!ff' payload exactly), LEADERs
    without a target and with empty rows.  leader[i] = n + i for an alive FOLLOWER with has_lpos, else -1;
    dead agents have has_t masked to 0 for the call (they do not move) and restored afterwards.
Driven with use_pow=True it equals real SwarmAgent objects bit for bit (tests/golden/loop_*.npz,
tools/gen_golden_loop.py); with use_pow=False it is the GPU's x*x arithmetic.
"""
import numpy as np

F, W, L = 1, 2, 3
FSM_KEYS = ("state", "leader", "last_hb", "wait_start", "delay", "lpos", "has_lpos", "alive")
# the thirteen per-agent arrays of a loop_* fixture (key + "_out"), position / velocity / target as x, y pairs
OUT_KEYS = FSM_KEYS + ("x", "y", "vx", "vy", "tx", "ty", "has_t")


def run(oracle, g, ticks=None, *, use_pow=False, hb_lagged=True, timeout=3.0, jitter=0.2):
    """Ticks 1 .. ticks of U1 from a fixture-style input dict g (ids, x, y, row_ptr, col, tick_off,
    last_hb0, tx, ty, has_t, obs, kill_ticks, seed, dt, max_speed; optional sense_row_ptr / sense_col:
    the sensor CSR when it is not the message graph) -> dict of OUT_KEYS, counts (ticks x 4) and
    singular.  hb_lagged=False is the easy mistake: heartbeats reading the current positions P_{t-1}."""
    ids = np.asarray(g["ids"], np.int32)
    n = len(ids)
    ticks = int(g["ticks"]) if ticks is None else int(ticks)
    rp, col = np.asarray(g["row_ptr"], np.int64), np.asarray(g["col"], np.int32)
    srp = np.asarray(g.get("sense_row_ptr", rp), np.int64)
    scol = np.asarray(g.get("sense_col", col), np.int32)
    dt, ms, seed = float(g["dt"]), float(g["max_speed"]), int(g["seed"])
    x, y = np.array(g["x"], np.float64), np.array(g["y"], np.float64)
    px, py = x.copy(), y.copy()  # P_{t-2}; a fresh run's heartbeats in flight: none, so P_0 serves
    vx, vy = np.zeros(n), np.zeros(n)
    tx, ty = np.array(g["tx"], np.float64), np.array(g["ty"], np.float64)
    has_t = np.array(g["has_t"], np.uint8)
    fsm = dict(last_hb=np.array(g["last_hb0"], np.float64))
    counts = np.zeros((ticks, 4), np.int64)
    singular = 0
    ids2 = np.concatenate([ids, ids])
    rp2 = np.concatenate([srp, np.full(n, srp[-1], np.int64)])
    lead_rows = np.arange(n, 2 * n, dtype=np.int32)
    for t in range(1, ticks + 1):
        hx, hy = (px, py) if hb_lagged else (x, y)
        o = oracle.protocol(ids, hx, hy, rp, col, g["tick_off"], 1, t0=t - 1, dt=dt, timeout=timeout,
                            jitter=jitter, seed=seed, kill_ticks=g["kill_ticks"], **fsm)
        counts[t - 1] = o.pop("counts")[0]
        fsm = o
        alive = fsm["alive"] != 0
        follows = alive & (fsm["state"] == F) & (fsm["has_lpos"] != 0)
        lp = fsm["lpos"].astype(np.float64)
        z = np.zeros(n)
        ph = oracle.physics(
            ids2, np.concatenate([fsm["state"], np.full(n, L, np.uint8)]),
            np.concatenate([np.where(follows, lead_rows, -1).astype(np.int32), np.full(n, -1, np.int32)]),
            np.concatenate([x, lp[:, 0]]), np.concatenate([y, lp[:, 1]]), np.concatenate([vx, z]),
            np.concatenate([vy, z]), np.concatenate([tx, z]), np.concatenate([ty, z]),
            np.concatenate([np.where(alive, has_t, 0).astype(np.uint8), np.zeros(n, np.uint8)]),
            g["obs"], rp2, scol, dt=dt, max_speed=ms, steps=1, use_pow=use_pow)
        singular += ph["singular"]
        px, py = x, y
        x, y, vx, vy, tx, ty = (ph[k][:n].copy() for k in ("x", "y", "vx", "vy", "tx", "ty"))
        has_t = np.where(alive, ph["has_t"][:n], has_t).astype(np.uint8)
    out = {k: fsm[k] for k in FSM_KEYS} if ticks else {}
    out.update(x=x, y=y, vx=vx, vy=vy, tx=tx, ty=ty, has_t=has_t, counts=counts, singular=singular,
               px=px, py=py)
    return out
