#!/usr/bin/env python3
"""Generate tests/golden/loop_tasks_*.npz by driving REAL reference agents through the radio update loop with
a task board handed to every agent at a stored tick (build container only; the helpers are
tools/gen_golden.py's, tools/gen_golden_loop.py's and tools/gen_golden_loop_sensed.py's, none of them changed:
the loop below is a loop of its own, so the existing fixtures stay byte-identical).

Contract U1-T: gen_golden_loop.ref_loop's lock-step loop with U1-R's delivery (every tick the
packets of tick t-1 from the agents within radio_radius in the snapshot at the start of the tick, ascending
index, each sender's packets in the order it sent them) and all five message types dispatched -- TASK_CLAIM and
TASK_CONFLICT through on_message_received, or through the handlers directly on the wide path ('!IB' -> '!II').
At the start of tick task_tick every agent, dead ones included, gets the same board: 24 tasks drawn uniformly
over the bounding box of the positions at that moment (P_{task_tick-1}), each requiring none or one of three
capability names; every agent holds each name with p = 0.5.  From then on _process_logic's third step claims.
Only data is written: loop_radio_*'s keys, the board (task_x, task_y, task_req as an index into cap_names or
-1, caps as a bit mask over cap_names, task_tick), the final statuses, every agent's task_claims as dense
tables, the claim and conflict sets of the last two ticks by tick parity, and the per-tick task counts (claims
sent, claims handled by a LEADER, TASK_CONFLICT messages sent).  tests/golden/index.json is not touched.

The tool asserts what each fixture must exercise and prints the figures (see CONDITIONS).

Usage:  python tools/gen_golden_loop_tasks.py [--only NAME ...]
"""
from __future__ import annotations

import argparse
import math
import os
import struct
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402
import gen_golden_loop as ggl  # noqa: E402
import gen_golden_loop_sensed as ggs  # noqa: E402

RADIO_RADIUS, TASK_TICK, N_TASKS = 2.5, 45, 24
CAP_NAMES = ("extinguisher", "sonar", "camera")
TASK_CASES = {
    # loop_n200's inputs and kills (u8 IDs)
    "loop_tasks_n200": dict(ggl.LOOP_CASES["loop_n200"], sense_radius=2.5, task_seed=9113),
    # IDs > 255: the wide codec path
    "loop_tasks_wide_n400": dict(ggl.LOOP_CASES["loop_wide_n400"], sense_radius=2.5, task_seed=9113),
    # a sensing radius below the personal space and below the radio radius
    "loop_tasks_r12_n250": dict(ggl.LOOP_CASES["loop_n250"], sense_radius=1.2, task_seed=9113),
}
CONDITIONS = "all four statuses at the end; leader-handled claims >= 20; hysteresis replacements >= 2; " \
             "re-affirmations >= 5; statuses overwritten by a later conflict >= 2; claims no leader handled >= 20; " \
             "no evaluated pair inside the guard band"


def guard_flag(u, thr=20.0):
    """csrc/utility.h guard_flag."""
    if u == 0.0:
        return False
    if abs(u - thr) <= max(abs(thr), abs(u)) * 2.0 ** -49:
        return True
    if u > thr:
        e = abs(u) * 2.0 ** -50
        return np.float32(u - e) != np.float32(u + e)
    return False


def ref_loop_tasks(mod, inp, task_seed, n_tasks=N_TASKS, stat_from=0, before_tick=None):
    """n_tasks: the board's size (tools/gen_golden_loop_board.py hands out more than the 64 the words below can
    hold: they then carry the tasks below 64 only, and stat["claim_sets"] / stat["conflict_sets"] the last two
    ticks' sets as index lists).  stat_from: the observers' figures count tasks with this index and above.
    before_tick(t, agents, board, trng): called at the start of every tick from the hand-out on, after the board is
    handed out (tools/gen_golden_moving_tasks.py moves the tasks with it)."""
    N_TASKS = n_tasks
    n = len(inp["ids"])
    ids = inp["ids"]
    wide = int(ids.max()) > 255
    mod.struct = gg._FsmWide(struct) if wide else struct
    clock, cur = [0.0], [0, 0]
    seed, dt = int(inp["seed"]), float(inp["dt"])
    ticks = int(inp["ticks"])
    mod.time = types.SimpleNamespace(time=lambda: clock[0], sleep=gg._noop)
    mod.random = types.SimpleNamespace(uniform=lambda a, b: a + (b - a) * gg.jitter_u(seed, cur[0], cur[1]))
    trng = np.random.default_rng(task_seed)
    caps = np.zeros(n, np.uint32)
    for b in range(len(CAP_NAMES)):
        caps |= (trng.uniform(size=n) < 0.5).astype(np.uint32) << np.uint32(b)
    agents = [mod.SwarmAgent(int(ids[i]), n, capabilities=[c for b, c in enumerate(CAP_NAMES) if caps[i] >> b & 1])
              for i in range(n)]
    out_prev = [[] for _ in range(n)]
    out_cur = [[] for _ in range(n)]
    stat = dict(handled=0, replaced=0, reaffirmed=0, overwritten=0, sent=0, min_gap=math.inf, guard=0)
    claim_heard = {}  # (sender id, task, its tick) -> leaders that handled it
    task_of = {}  # id(an agent's task dict) -> its index
    L, W = mod.AgentState.LEADER, mod.AgentState.ELECTION_WAIT
    tcounts = np.zeros((ticks, 3), np.int64)
    now_t = [0]
    for i, a in enumerate(agents):
        a.position = [float(inp["x"][i]), float(inp["y"][i])]
        a.last_heartbeat_time = float(inp["last_hb0"][i])
        a.max_speed = float(inp["max_speed"])
        if inp["has_t"][i]:
            a.set_target(float(inp["tx"][i]), float(inp["ty"][i]))

        def send(mt, payload=b"", a=a, i=i):  # the payload as packed at send time
            out_cur[i].append(a._pack_header(mt) + payload)
            if mt == 4:
                tcounts[now_t[0] - 1, 0] += 1
            if mt == 5:
                tcounts[now_t[0] - 1, 2] += 1
        a._send_msg = send

        # observers around the real handlers (they decide nothing)
        def claim(sender, payload, a=a, real=a._handle_task_claim):
            k, u = struct.unpack("!If", payload)
            if a.state == L:
                tcounts[now_t[0] - 1, 1] += 1
                stat["handled"] += k >= stat_from
                claim_heard[(sender, k, now_t[0] - 1)] += 1
                held = a.task_claims.get(k)
                if held and u > held["utility"] + 5.0:
                    stat["replaced"] += k >= stat_from
                elif held and held["winner"] != sender:
                    stat["reaffirmed"] += k >= stat_from
            real(sender, payload)
        a._handle_task_claim = claim

        def conflict(sender, payload, a=a, real=a._handle_task_conflict):
            k, _ = mod.struct.unpack("!IB", payload)
            before = a.tasks[k]["status"]
            real(sender, payload)
            if before in ("LOCKED", "ASSIGNED") and a.tasks[k]["status"] != before:
                stat["overwritten"] += k >= stat_from
        a._handle_task_conflict = conflict

        def util(task, a=a, real=a._calculate_utility):
            u = real(task)
            if task_of.get(id(task), 0) >= stat_from:
                stat["min_gap"] = min(stat["min_gap"], abs(u - 20.0))
                stat["guard"] += guard_flag(u)
            return u
        a._calculate_utility = util
    obstacles = [tuple(float(v) for v in o) for o in inp["obs"]]
    alive = np.ones(n, bool)
    kills = set(int(k) for k in inp["kill_ticks"])
    counts = np.zeros((ticks, 4), np.int64)
    heard = ggs.sensed_rows(RADIO_RADIUS)
    sensed = ggs.sensed_rows(float(inp["sense_radius"]))
    board = None
    last_two = [None, None]  # out_cur of ticks end-1 and end
    for t in range(1, ticks + 1):
        clock[0] = t * dt
        now_t[0] = t
        if t in kills:
            for i, a in enumerate(agents):
                if alive[i] and a.state == L:
                    alive[i] = False
        if t == TASK_TICK:
            px = np.array([a.position[0] for a in agents])
            py = np.array([a.position[1] for a in agents])
            tx = trng.uniform(px.min(), px.max(), N_TASKS)
            ty = trng.uniform(py.min(), py.max(), N_TASKS)
            req = trng.integers(-1, len(CAP_NAMES), N_TASKS).astype(np.int8)
            board = dict(task_x=tx, task_y=ty, task_req=req)
            for a in agents:
                a.tasks = {}
                for k in range(N_TASKS):
                    a.tasks[k] = {"status": "OPEN", "pos": (float(tx[k]), float(ty[k]))}
                    task_of[id(a.tasks[k])] = k
                    if req[k] >= 0:
                        a.tasks[k]["required_cap"] = CAP_NAMES[req[k]]
        if before_tick is not None and board is not None:
            before_tick(t, agents, board, trng)
        hears = heard([(a.position[0], a.position[1]) for a in agents])
        for i, a in enumerate(agents):
            if not alive[i]:
                continue
            a.tick = t + int(inp["tick_off"][i])
            for j in hears[i]:
                for pkt in out_prev[j]:
                    if wide:  # on_message_received slices a 6-byte header: dispatch as it does
                        mt, snd, _ = struct.unpack("!BII", pkt[:9])
                        pl = pkt[9:]
                        {1: lambda: a._handle_heartbeat(snd, pl), 2: lambda: a._handle_election_acclaim(snd),
                         3: lambda: a._handle_coordinator(snd), 4: lambda: a._handle_task_claim(snd, pl),
                         5: lambda: a._handle_task_conflict(snd, pl)}[mt]()
                    else:
                        a.on_message_received(pkt)
        for i, a in enumerate(agents):
            if not alive[i]:
                continue
            cur[0], cur[1] = int(ids[i]), t
            a.tick = t + int(inp["tick_off"][i])
            a._process_logic()
        snap = [(a.position[0], a.position[1]) for a in agents]
        rows = sensed(snap)
        for i, a in enumerate(agents):
            if alive[i]:
                a.update_sensors(obstacles, [(int(ids[j]), snap[j][0], snap[j][1]) for j in rows[i]])
        for i, a in enumerate(agents):
            if alive[i]:
                a._update_physics(dt)
        hdr = 9 if wide else 6
        for i, a in enumerate(agents):
            types_sent = {pk[0] for pk in out_cur[i]}
            counts[t - 1, 2] += 2 in types_sent
            counts[t - 1, 3] += 1 in types_sent
            for pk in out_cur[i]:
                if pk[0] == 4:
                    claim_heard[(int(ids[i]), struct.unpack("!If", pk[hdr:])[0], t)] = 0
            if alive[i]:
                counts[t - 1, 0] += a.state == L
                counts[t - 1, 1] += a.state == W
        last_two = [last_two[1], out_cur]
        out_prev, out_cur = out_cur, [[] for _ in range(n)]
    conf_fmt = "!II" if wide else "!IB"
    hdr = 9 if wide else 6
    claim_out = np.zeros((2, n), np.uint64)
    conflict_out = np.zeros((2, n), np.uint64)
    stat["claim_sets"] = [[set() for _ in range(n)] for _ in range(2)]
    stat["conflict_sets"] = [[set() for _ in range(n)] for _ in range(2)]
    for tk, sent in ((ticks - 1, last_two[0]), (ticks, last_two[1])):
        for i in range(n):
            for pk in sent[i]:
                if pk[0] == 4:
                    k = struct.unpack("!If", pk[hdr:])[0]
                    stat["claim_sets"][tk & 1][i].add(k)
                    if k < 64:
                        claim_out[tk & 1, i] |= np.uint64(1) << np.uint64(k)
                if pk[0] == 5:
                    k = struct.unpack(conf_fmt, pk[hdr:])[0]
                    stat["conflict_sets"][tk & 1][i].add(k)
                    if k < 64:
                        conflict_out[tk & 1, i] |= np.uint64(1) << np.uint64(k)
    mod.struct, mod.time, mod.random = struct, time, __import__("random")
    status = np.array([[gg.STATUS_CODE[a.tasks[k]["status"]] for k in range(N_TASKS)] for a in agents], np.uint8)
    tabw = np.full((n, N_TASKS), -1, np.int32)
    tabu = np.zeros((n, N_TASKS), np.float32)
    for i, a in enumerate(agents):
        for k, c in a.task_claims.items():
            tabw[i, k] = c["winner"]
            tabu[i, k] = c["utility"]  # an unpacked '!f': exactly an f32
            assert float(tabu[i, k]) == c["utility"]
    stat["sent"] = int(tcounts[:, 0].sum())
    stat["unheard"] = sum(1 for (_, k, _), v in claim_heard.items() if v == 0 and k >= stat_from)
    assert len(claim_heard) == stat["sent"]
    out = dict(
        state_out=np.array([a.state.value for a in agents], np.uint8),
        leader_out=np.array([-1 if a.leader_id is None else a.leader_id for a in agents], np.int32),
        last_hb_out=np.array([a.last_heartbeat_time for a in agents], np.float64),
        wait_start_out=np.array([a.election_wait_start for a in agents], np.float64),
        delay_out=np.array([a.election_delay for a in agents], np.float64),
        has_lpos_out=np.array([a.leader_pos is not None for a in agents], np.uint8),
        lpos_out=np.array([a.leader_pos if a.leader_pos is not None else (0.0, 0.0) for a in agents],
                          np.float32).reshape(n, 2),
        alive_out=alive.astype(np.uint8),
        x_out=np.array([a.position[0] for a in agents]), y_out=np.array([a.position[1] for a in agents]),
        vx_out=np.array([a.velocity[0] for a in agents]), vy_out=np.array([a.velocity[1] for a in agents]),
        has_t_out=np.array([a.target is not None for a in agents], np.uint8),
        tx_out=np.array([a.target[0] if a.target else 0.0 for a in agents]),
        ty_out=np.array([a.target[1] if a.target else 0.0 for a in agents]),
        counts=counts, caps=caps, task_tick=np.int64(TASK_TICK), status_out=status, tab_winner_out=tabw,
        tab_util_out=tabu, claim_out=claim_out, conflict_out=conflict_out, task_counts=tcounts, **board)
    return out, stat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--task-seed", type=int, default=None, help="try another task seed (nothing is written)")
    args = ap.parse_args()
    mod = gg.load_reference()
    for name, c in TASK_CASES.items():
        if args.only is not None and name not in args.only:
            continue
        t0 = time.time()
        inp = ggl.make_loop_inputs(c)
        inp["sense_radius"] = np.float64(c["sense_radius"])
        inp["radio_radius"] = np.float64(RADIO_RADIUS)
        out, s = ref_loop_tasks(mod, inp, c["task_seed"] if args.task_seed is None else args.task_seed)
        present = sorted(set(out["status_out"].ravel().tolist()))
        print(name, "statuses", present, "leader-handled claims", s["handled"], "replacements", s["replaced"],
              "re-affirmations", s["reaffirmed"], "overwritten statuses", s["overwritten"], "claims sent", s["sent"],
              "claims no leader handled", s["unheard"], "conflicts sent", int(out["task_counts"][:, 2].sum()),
              "TENTATIVE at end", int((out["status_out"] == 1).sum()), "smallest |U - 20| %.2g" % s["min_gap"],
              "guard", s["guard"], "%.1fs" % (time.time() - t0), flush=True)
        ok = (present == [0, 1, 2, 3] and s["handled"] >= 20 and s["replaced"] >= 2 and s["reaffirmed"] >= 5 and
              s["overwritten"] >= 2 and s["unheard"] >= 20 and s["guard"] == 0)
        if args.task_seed is not None:
            print("   conditions", "met" if ok else "MISSED")
            continue
        assert ok, CONDITIONS
        arrays = dict(inp)
        arrays.update(out)
        np.savez_compressed(os.path.join(gg.OUT, name + ".npz"), **arrays)


if __name__ == "__main__":
    main()
