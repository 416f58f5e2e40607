"""CPU model of the task update loop (contract U1-T) -- TESTS ONLY.

loop_radio_model.run's per-tick composition (the radio CSR of P_{t-1}, oracle.protocol over P_{t-2}, then
oracle.physics with the sensor CSR of P_{t-1}) with the reference's task handlers restated in Python around
the protocol tick, over explicit messages -- every TASK_CLAIM as (task, f32 utility), every TASK_CONFLICT as
(task, winner) in the order it was sent -- so that it owes nothing to the two facts the kernels rely on (the
conflict delivery commuting with the receive, one bit per conflict):
  receive   alive agent i (after the tick's kills) walks its radio row in ascending index and handles each
            sender's TASK_CONFLICTs of tick t-1 (_handle_task_conflict, agent.py:327-336) and, while it is
            LEADER, its TASK_CLAIMs (_handle_task_claim, 304-325).  The election handlers only ever leave
            FOLLOWER behind, so i is LEADER at sender j's claims iff it was LEADER at the start of the tick and
            no sender up to and including j made it yield: one with ACCLAIM + COORDINATOR (unconditional
            takeover, 277-281), or with a HEARTBEAT and a higher ID (249-251).  The FSM itself is
            oracle.protocol's, as in loop_radio_model.
  logic     every alive agent's OPEN tasks with U(P_{t-1}[i]) > 20.0 become TENTATIVE and are claimed
            (_process_tasks, 292-302; _calculate_utility, 338-347).
use_pow=True squares with libm pow, as the reference's `**2` does, and equals real SwarmAgent objects bit for
bit (tests/golden/loop_tasks_*.npz, tools/gen_golden_loop_tasks.py); False is the GPU's x*x arithmetic.  The
rows' order is the order of the arrays: run it over the storage order to predict the GPU.  The board is handed
out at the start of tick g["task_tick"] (default 1): before it the run is loop_radio_model's.
"""
import math

import numpy as np

from loop_model import FSM_KEYS, F, L
from loop_sensed_model import sense_csr

OPEN, TENTATIVE, LOCKED, ASSIGNED = 0, 1, 2, 3
CLAIM_THR, HYSTERESIS, U_SCALE, FAR = 20.0, 5.0, 100.0, 36.0


def guard_flag(u, thr=CLAIM_THR):
    """csrc/utility.h guard_flag."""
    if u == 0.0 or u != u:
        return False
    if abs(u - thr) <= max(abs(thr), abs(u)) * 2.0 ** -49:
        return True
    if u > thr:
        e = abs(u) * 2.0 ** -50
        return bool(np.float32(u - e) != np.float32(u + e))
    return False


def utility(ax, ay, caps, tx, ty, rq, use_pow):
    """_calculate_utility (338-347); float ** 2 is libm pow, as in the reference."""
    dx, dy = ax - tx, ay - ty
    d = math.sqrt(dx ** 2 + dy ** 2) if use_pow else math.sqrt(dx * dx + dy * dy)
    has = 1.0 if rq < 0 or (rq < 32 and (int(caps) >> rq) & 1) else 0.0
    return (U_SCALE / (1.0 + d)) * has


def fresh_tasks(n, T):
    return dict(status=np.zeros((n, T), np.uint8), tab_winner=np.full((n, T), -1, np.int32),
                tab_util=np.zeros((n, T), np.float32), claims=[[] for _ in range(n)],
                conflicts=[[] for _ in range(n)], claims_prev=[[] for _ in range(n)],
                conflicts_prev=[[] for _ in range(n)])


def run(oracle, g, ticks=None, *, radio_radius=None, radius=None, use_pow=False, timeout=3.0, jitter=0.2,
        start=None, task_tick=None):
    """Ticks 1 .. ticks of U1-T from a fixture-style input dict g (loop_radio_model.run's keys plus task_x,
    task_y, task_req, caps, task_tick) -> loop_radio_model.run's dict plus status (n x T), tab_winner,
    tab_util, claim_out / conflict_out (2 x n uint64 by tick parity: the last two ticks' sets), task_counts
    (ticks x 3), guard, and `tasks`, the state a later chunk goes on from (start=)."""
    ids = np.asarray(g["ids"], np.int32)
    n = len(ids)
    ticks = int(g["ticks"]) if ticks is None else int(ticks)
    radius = float(g["sense_radius"]) if radius is None else float(radius)
    rc = float(g["radio_radius"]) if radio_radius is None else float(radio_radius)
    dt, ms, seed = float(g["dt"]), float(g["max_speed"]), int(g["seed"])
    tkx, tky = np.asarray(g["task_x"], np.float64), np.asarray(g["task_y"], np.float64)
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
    claims_prev, conf_prev = tk["claims"], tk["conflicts"]  # what tick t0 sent
    claims_pp, conf_pp = tk["claims_prev"], tk["conflicts_prev"]  # tick t0 - 1 (kept for the parity arrays)
    counts = np.zeros((ticks, 4), np.int64)
    tcounts = np.zeros((ticks, 3), np.int64)
    singular, max_row, max_heard, guard = 0, 0, 0, 0
    ids2 = np.concatenate([ids, ids])
    lead_rows = np.arange(n, 2 * n, dtype=np.int32)
    z = np.zeros(n)
    for t in range(t0 + 1, t0 + ticks + 1):
        rp, col = sense_csr(oracle, x, y, rc)
        max_heard = max(max_heard, int(np.diff(rp).max()) if n else 0)
        # ---- the task handlers of the receive, on the state before the tick's protocol step
        state0 = fsm["state"] if "state" in fsm else np.full(n, F, np.uint8)
        alive0 = (fsm["alive"] != 0) if "alive" in fsm else np.ones(n, bool)
        alive_now = alive0 & ~((state0 == L) & (t in kills))
        ob_in = fsm["outbox"][((t - 1) & 1) * n:((t - 1) & 1) * n + n] if "outbox" in fsm else np.zeros(n, np.uint8)
        claims_cur = [[] for _ in range(n)]
        conf_cur = [[] for _ in range(n)]
        task_sender = np.array([bool(claims_prev[j]) or bool(conf_prev[j]) for j in range(n)])
        if task_sender.any():
            hot = task_sender[col]
            rows = np.repeat(np.arange(n), np.diff(rp))[hot]
            for i in np.unique(rows):
                if not alive_now[i]:
                    continue
                me, leader = int(ids[i]), state0[i] == L
                for j in col[rp[i]:rp[i + 1]]:
                    o, s = int(ob_in[j]), int(ids[j])
                    for k, wn in conf_prev[j]:  # (anywhere among j's packets: they write only the status)
                        status[i, k] = ASSIGNED if wn == me else LOCKED
                    if leader and ((o & 1) or ((o & 2) and s > me)):
                        leader = False  # j's election packets made it yield: its claims come after them
                    if not leader:
                        continue
                    for k, u in claims_prev[j]:
                        tcounts[t - t0 - 1, 1] += 1
                        if tabw[i, k] < 0 or float(u) > float(tabu[i, k]) + HYSTERESIS:
                            tabw[i, k], tabu[i, k] = s, u
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
                u = utility(float(x[i]), float(y[i]), caps[i], float(tkx[k]), float(tky[k]), int(trq[k]), use_pow)
                guard += guard_flag(u)
                if u > CLAIM_THR:
                    status[i, k] = TENTATIVE
                    claims_cur[i].append((int(k), np.float32(u)))
        tcounts[t - t0 - 1, 0] = sum(len(c) for c in claims_cur)
        tcounts[t - t0 - 1, 2] = sum(len(c) for c in conf_cur)
        claims_pp, conf_pp, claims_prev, conf_prev = claims_prev, conf_prev, claims_cur, conf_cur
        # ---- physics
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
               tasks=dict(status=status, tab_winner=tabw, tab_util=tabu, claims=claims_prev, conflicts=conf_prev,
                          claims_prev=claims_pp, conflicts_prev=conf_pp))
    return out
