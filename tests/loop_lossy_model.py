"""CPU model of the radio and task update loops over a lossy channel (contract U1-L) -- TESTS ONLY.

loop_tasks_model.run's per-tick composition (which is loop_radio_model.run's when there is no board) with one
step added: after the radio CSR of the tick's snapshot is built, row i loses every j whose link j -> i is
dropped at that tick,
    dropped(loss_seed, t, ids[j], ids[i], loss)  iff  u(loss_seed, t, ids[j], ids[i]) < loss,
with t the absolute tick.  Everything that is received -- oracle.protocol's election packets and heartbeats,
the TASK_CLAIMs and the TASK_CONFLICTs -- is received over the filtered rows, so a dropped link delivers
nothing of its sender's tick t-1 sends.  The sensing CSR at sense_radius is not filtered: loss is the radio's,
not the sensors'.  link_counts come from the unfiltered rows: per tick the ordered pairs of an alive receiver
(after the tick's kills) and an in-range sender whose inbound outbox byte holds ACCLAIM or HEARTBEAT, and how
many of those pairs were dropped.  u() is the draw of csrc/link_loss.h, restated in numpy.
With loss = 0 the run is loop_tasks_model.run's / loop_radio_model.run's.  use_pow as there: True equals real
SwarmAgent objects bit for bit (tests/golden/loop_lossy_*.npz, tools/gen_golden_loop_lossy.py), False is the
GPU's x*x arithmetic.  The rows' order is the order of the arrays: run it over the storage order to predict
the GPU (the verdicts are keyed on IDs, so they do not change with the order).
"""
import numpy as np

from loop_model import FSM_KEYS, F, L
from loop_sensed_model import sense_csr
from loop_tasks_model import ASSIGNED, CLAIM_THR, FAR, HYSTERESIS, LOCKED, OPEN, TENTATIVE, fresh_tasks, \
    guard_flag, utility

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
K_ID, K_T = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD1B54A32D192ED03)
K1, K2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def _fin(x):
    x = (x ^ (x >> np.uint64(30))) * K1
    x = (x ^ (x >> np.uint64(27))) * K2
    return x ^ (x >> np.uint64(31))


def u(seed, t, sid, rid):
    """The link's uniform draw in [0, 1) (csrc/link_loss.h link_u), vectorised: t, sid, rid broadcast."""
    with np.errstate(over="ignore"):
        seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
        t = np.asarray(t, np.int64).astype(np.uint64)
        s = np.asarray(sid, np.int32).astype(np.uint32).astype(np.uint64)
        r = np.asarray(rid, np.int32).astype(np.uint32).astype(np.uint64)
        a = _fin(seed ^ (s * K_ID) ^ (t * K_T))
        b = _fin(a ^ (r * K_ID))
    return (b >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def dropped(seed, t, sid, rid, loss):
    return u(seed, t, sid, rid) < float(loss)


def lossy_rows(rp, col, ids, t, loss, loss_seed, alive, ob_in):
    """Row i of (rp, col) without the senders whose link to i is dropped at tick t, and the tick's link counts
    (election links of alive receivers, those dropped) from the unfiltered rows."""
    n = len(ids)
    col = np.asarray(col, np.int64)
    rows = np.repeat(np.arange(n), np.diff(rp))
    drop = dropped(loss_seed, t, ids[col], ids[rows], loss) if len(col) else np.zeros(0, bool)
    link = alive[rows] & ((ob_in[col] & 3) != 0)
    keep = ~drop
    rp2 = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=rp2[1:])
    return rp2, col[keep].astype(np.int32), (int(link.sum()), int((link & drop).sum()))


def run(oracle, g, ticks=None, *, loss=None, loss_seed=None, radio_radius=None, radius=None, use_pow=False,
        timeout=3.0, jitter=0.2, start=None, task_tick=None):
    """Ticks 1 .. ticks of U1-L from a fixture-style input dict g: loop_tasks_model.run's keys (the task keys
    may be missing: no board, the radio loop) plus loss and loss_seed -> loop_tasks_model.run's dict plus
    link_counts (ticks x 2).  start: a dict this function returned, as there."""
    ids = np.asarray(g["ids"], np.int32)
    n = len(ids)
    ticks = int(g["ticks"]) if ticks is None else int(ticks)
    radius = float(g["sense_radius"]) if radius is None else float(radius)
    rc = float(g["radio_radius"]) if radio_radius is None else float(radio_radius)
    loss = float(g["loss"]) if loss is None else float(loss)
    loss_seed = int(g["loss_seed"]) if loss_seed is None else int(loss_seed)
    dt, ms, seed = float(g["dt"]), float(g["max_speed"]), int(g["seed"])
    tkx, tky = np.asarray(g.get("task_x", ()), np.float64), np.asarray(g.get("task_y", ()), np.float64)
    T = len(tkx)
    trq = np.asarray(g["task_req"], np.int64) if T else np.zeros(0, np.int64)
    caps = np.asarray(g["caps"], np.uint32) if T else np.zeros(n, np.uint32)
    task_tick = int(g.get("task_tick", 1)) if task_tick is None else int(task_tick)
    kills = set(int(k) for k in np.asarray(g["kill_ticks"]).ravel())
    t0 = 0
    if start is None:
        x, y = np.array(g["x"], np.float64), np.array(g["y"], np.float64)
        px, py = x.copy(), y.copy()
        vx, vy = np.zeros(n), np.zeros(n)
        tx, ty = np.array(g["tx"], np.float64), np.array(g["ty"], np.float64)
        has_t = np.array(g["has_t"], np.uint8)
        fsm = dict(last_hb=np.array(g["last_hb0"], np.float64))
        fsm.update({k: np.array(v) for k, v in g.get("fsm0", {}).items()})
        tk = fresh_tasks(n, T)
    else:
        t0 = int(start["tick"])
        x, y, px, py, vx, vy, tx, ty = (np.array(start[k], np.float64) for k in
                                        ("x", "y", "px", "py", "vx", "vy", "tx", "ty"))
        has_t = np.array(start["has_t"], np.uint8)
        fsm = {k: np.array(v) for k, v in start["fsm"].items()}
        tk = start.get("tasks") or fresh_tasks(n, T)
        tk = {k: (v.copy() if isinstance(v, np.ndarray) else [list(q) for q in v]) for k, v in tk.items()}
    status, tabw, tabu = tk["status"], tk["tab_winner"], tk["tab_util"]
    claims_prev, conf_prev = tk["claims"], tk["conflicts"]
    claims_pp, conf_pp = tk["claims_prev"], tk["conflicts_prev"]
    counts = np.zeros((ticks, 4), np.int64)
    tcounts = np.zeros((ticks, 3), np.int64)
    lcounts = np.zeros((ticks, 2), np.int64)
    singular, max_row, max_heard, guard = 0, 0, 0, 0
    ids2 = np.concatenate([ids, ids])
    lead_rows = np.arange(n, 2 * n, dtype=np.int32)
    z = np.zeros(n)
    for t in range(t0 + 1, t0 + ticks + 1):
        rp, col = sense_csr(oracle, x, y, rc)
        max_heard = max(max_heard, int(np.diff(rp).max()) if n else 0)
        state0 = fsm["state"] if "state" in fsm else np.full(n, F, np.uint8)
        alive0 = (fsm["alive"] != 0) if "alive" in fsm else np.ones(n, bool)
        alive_now = alive0 & ~((state0 == L) & (t in kills))
        ob_in = fsm["outbox"][((t - 1) & 1) * n:((t - 1) & 1) * n + n] if "outbox" in fsm else np.zeros(n, np.uint8)
        # ---- the channel: the one step this model adds
        rp, col, lcounts[t - t0 - 1] = lossy_rows(rp, col, ids, t, loss, loss_seed, alive_now, ob_in)
        # ---- the task handlers of the receive, on the state before the tick's protocol step
        claims_cur = [[] for _ in range(n)]
        conf_cur = [[] for _ in range(n)]
        task_sender = np.array([bool(claims_prev[j]) or bool(conf_prev[j]) for j in range(n)], bool)
        if task_sender.any() and len(col):
            hot = task_sender[col]
            rows = np.repeat(np.arange(n), np.diff(rp))[hot]
            for i in np.unique(rows):
                if not alive_now[i]:
                    continue
                me, leader = int(ids[i]), state0[i] == L
                for j in col[rp[i]:rp[i + 1]]:
                    o, s = int(ob_in[j]), int(ids[j])
                    for k, wn in conf_prev[j]:
                        status[i, k] = ASSIGNED if wn == me else LOCKED
                    if leader and ((o & 1) or ((o & 2) and s > me)):
                        leader = False
                    if not leader:
                        continue
                    for k, uu in claims_prev[j]:
                        tcounts[t - t0 - 1, 1] += 1
                        if tabw[i, k] < 0 or float(uu) > float(tabu[i, k]) + HYSTERESIS:
                            tabw[i, k], tabu[i, k] = s, uu
                            conf_cur[i].append((k, s))
                        elif tabw[i, k] != s:
                            conf_cur[i].append((k, int(tabw[i, k])))
        # ---- the election handlers, timers and heartbeat
        o = oracle.protocol(ids, px, py, rp, col, g["tick_off"], 1, t0=t - 1, dt=dt, timeout=timeout,
                            jitter=jitter, seed=seed, kill_ticks=g["kill_ticks"], **fsm)
        counts[t - t0 - 1] = o.pop("counts")[0]
        fsm = o
        alive = fsm["alive"] != 0
        assert (alive == alive_now).all()
        # ---- _process_tasks at the tick's snapshot P_{t-1}
        if T and t >= task_tick:
            with np.errstate(invalid="ignore"):
                near = (x[:, None] - tkx[None, :]) ** 2 + (y[:, None] - tky[None, :]) ** 2 <= FAR
            for i, k in zip(*np.nonzero(near & (status == OPEN) & alive[:, None])):
                uu = utility(float(x[i]), float(y[i]), caps[i], float(tkx[k]), float(tky[k]), int(trq[k]), use_pow)
                guard += guard_flag(uu)
                if uu > CLAIM_THR:
                    status[i, k] = TENTATIVE
                    claims_cur[i].append((int(k), np.float32(uu)))
        tcounts[t - t0 - 1, 0] = sum(len(c) for c in claims_cur)
        tcounts[t - t0 - 1, 2] = sum(len(c) for c in conf_cur)
        claims_pp, conf_pp, claims_prev, conf_prev = claims_prev, conf_prev, claims_cur, conf_cur
        # ---- physics (the sensors are not lossy)
        follows = alive & (fsm["state"] == F) & (fsm["has_lpos"] != 0)
        lp = fsm["lpos"].astype(np.float64)
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
    end = t0 + ticks
    claim_out, conflict_out = np.zeros((2, n), np.uint64), np.zeros((2, n), np.uint64)
    for tick, cl, cf in ((end - 1, claims_pp, conf_pp), (end, claims_prev, conf_prev)):
        for i in range(n):
            for k, _ in cl[i]:
                claim_out[tick & 1, i] |= np.uint64(1) << np.uint64(k)
            for k, _ in cf[i]:
                conflict_out[tick & 1, i] |= np.uint64(1) << np.uint64(k)
    out = {k: fsm[k] for k in FSM_KEYS} if "state" in fsm else {}
    out.update(fsm=fsm, x=x, y=y, vx=vx, vy=vy, tx=tx, ty=ty, has_t=has_t, counts=counts, singular=singular,
               px=px, py=py, max_row=max_row, max_heard=max_heard, tick=end, status=status, tab_winner=tabw,
               tab_util=tabu, claim_out=claim_out, conflict_out=conflict_out, task_counts=tcounts, guard=guard,
               link_counts=lcounts,
               tasks=dict(status=status, tab_winner=tabw, tab_util=tabu, claims=claims_prev, conflicts=conf_prev,
                          claims_prev=claims_pp, conflicts_prev=conf_pp))
    return out
