"""CPU model of the sensed update loop (contract U1-S) -- TESTS ONLY.

loop_model.run's per-tick composition (oracle.protocol over P_{t-2}, then oracle.physics on the agents and
their leader-position phantoms) with the sensor CSR rebuilt, every tick, from the positions that tick's
physics reads, P_{t-1}: agent i senses j != i iff dx*dx + dy*dy <= R*R (fp64, the products rounded
separately), rows in ascending index, dead agents and agents without a target included.  The rows' order is
the order of the arrays it is given: run it over the storage order to predict the GPU.
  n <= 2 048   the rule brute-forced in numpy (elementwise, the same bits; any coordinates, and a non-finite
               agent fails every <=: it senses nobody and is sensed by nobody)
  larger n     oracle.rgg_csr, which indexes its cells from floor(x / r) >= 0: the coordinates must stay
               >= 0 over the run
resense=False keeps the graph of the tick-0 positions for the whole run: U1 with sensors = that graph, the
absence of the feature.  use_pow as loop_model.run: True equals real SwarmAgent objects bit for bit
(tests/golden/loop_sensed_*.npz, tools/gen_golden_loop_sensed.py), False is the GPU's x*x arithmetic.
"""
import numpy as np

from loop_model import FSM_KEYS, F, L

BRUTE_MAX = 2048


def sense_csr(oracle, x, y, radius):
    """(row_ptr int64, col int32) of the agents within `radius` of each other, rows in ascending index."""
    n = len(x)
    if n <= BRUTE_MAX:
        with np.errstate(invalid="ignore"):
            dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
            near = dx * dx + dy * dy <= radius * radius
        near[np.arange(n), np.arange(n)] = False
        rows, cols = np.nonzero(near)  # row-major: each row's columns ascend
        rp = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
        return rp, cols.astype(np.int32)
    assert np.isfinite(x).all() and np.isfinite(y).all() and x.min() >= 0.0 and y.min() >= 0.0, \
        "oracle.rgg_csr needs finite coordinates >= 0"
    rp, col = oracle.rgg_csr(x, y, radius)
    return np.asarray(rp, np.int64), np.asarray(col, np.int32)


def run(oracle, g, ticks=None, *, radius=None, use_pow=False, resense=True, timeout=3.0, jitter=0.2):
    """Ticks 1 .. ticks of U1-S from a fixture-style input dict g (loop_model.run's keys; sense_radius unless
    `radius` is given; optional fsm0: FSM arrays the run starts from instead of a fresh agent's) -> dict of
    loop_model.OUT_KEYS, counts (ticks x 4), singular, px / py (P_{end-1}) and max_row, the longest sensed
    row of the run."""
    ids = np.asarray(g["ids"], np.int32)
    n = len(ids)
    ticks = int(g["ticks"]) if ticks is None else int(ticks)
    radius = float(g["sense_radius"]) if radius is None else float(radius)
    rp, col = np.asarray(g["row_ptr"], np.int64), np.asarray(g["col"], np.int32)
    dt, ms, seed = float(g["dt"]), float(g["max_speed"]), int(g["seed"])
    x, y = np.array(g["x"], np.float64), np.array(g["y"], np.float64)
    px, py = x.copy(), y.copy()
    vx, vy = np.zeros(n), np.zeros(n)
    tx, ty = np.array(g["tx"], np.float64), np.array(g["ty"], np.float64)
    has_t = np.array(g["has_t"], np.uint8)
    fsm = dict(last_hb=np.array(g["last_hb0"], np.float64))
    fsm.update({k: np.array(v) for k, v in g.get("fsm0", {}).items()})  # oracle.protocol's state keywords
    counts = np.zeros((ticks, 4), np.int64)
    singular, max_row = 0, 0
    ids2 = np.concatenate([ids, ids])
    lead_rows = np.arange(n, 2 * n, dtype=np.int32)
    z = np.zeros(n)
    srp = scol = None
    for t in range(1, ticks + 1):
        o = oracle.protocol(ids, px, py, rp, col, g["tick_off"], 1, t0=t - 1, dt=dt, timeout=timeout,
                            jitter=jitter, seed=seed, kill_ticks=g["kill_ticks"], **fsm)
        counts[t - 1] = o.pop("counts")[0]
        fsm = o
        alive = fsm["alive"] != 0
        follows = alive & (fsm["state"] == F) & (fsm["has_lpos"] != 0)
        lp = fsm["lpos"].astype(np.float64)
        if resense or srp is None:
            srp, scol = sense_csr(oracle, x, y, radius)
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
    out = {k: fsm[k] for k in FSM_KEYS} if ticks else {}
    out.update(x=x, y=y, vx=vx, vy=vy, tx=tx, ty=ty, has_t=has_t, counts=counts, singular=singular,
               px=px, py=py, max_row=max_row)
    return out
