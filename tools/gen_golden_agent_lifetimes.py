#!/usr/bin/env python3
"""Generate tests/golden/agent_life_*.npz by driving REAL reference agents that are constructed anew and stopped
during the radio update loop, with and without a task board (contract U1-J; build container only; the
helpers are tools/gen_golden_loop.py's, gen_golden_loop_sensed.py's and gen_golden_loop_tasks.py's).

gen_golden_loop.ref_loop's lock-step loop with the radio loop's delivery (the previous tick's packets from the
agents within radio_radius of the receiver in the snapshot at the start of the tick, ascending index) and sensing,
and one window [boot, death) of absolute ticks per agent.  Before tick t, after the leader kill:
  death == t   the agent is no longer ticked and nothing is delivered to it; what it sent during t - 1 is still
               delivered to the others; its body stays a separation neighbour;
  boot == t    a new SwarmAgent(id, n, capabilities) takes the old object's place, constructed with the clock at
               (t - 1) dt, at the position the old one stood at, its tick counter 1 at tick t; what the old object
               sent during t - 1 is dropped with it; once the board is handed out, the new object gets a `tasks`
               dict of its own with every task OPEN, and its task_claims are empty as __init__ leaves them.
Agents with boot > 0 are down from the start, except the agents of `restart`, which run from tick 0 and are up when
they boot (the caller puts their alive flags back after the set-time rule).  The board case is
gen_golden_loop_tasks.py's: capabilities and 24 tasks drawn from a task seed, handed to every agent at tick 45,
message types 4 and 5 dispatched.  The windows are drawn before the run; the leaders that die, the high IDs that
start late and (board) the holders of an ASSIGNED task that restart are picked from shorter runs, so that the
reference run alone shows what the asserts below ask of every fixture.  Only data is written: the inputs
(loop_radio_* / loop_tasks_*'s keys plus boot / death / restart), every final per-agent array, tick_off as the run
left it, the per-tick counts and the per-tick events.

Usage:  python tools/gen_golden_agent_lifetimes.py [--only NAME ...]
"""
from __future__ import annotations

import argparse
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
import gen_golden_loop_tasks as ggt  # noqa: E402

FOREVER = np.iinfo(np.int64).max
RADIO_RADIUS = 2.5
TICKS = 120
CASES = {
    "agent_life_radio_n200": dict(ggl.LOOP_CASES["loop_n200"], sense_radius=2.5, ticks=TICKS, kill_ticks=[]),
    "agent_life_board_n200": dict(ggl.LOOP_CASES["loop_n200"], sense_radius=2.5, ticks=TICKS, kill_ticks=[],
                                  task_seed=4242),
    "agent_life_wide_n400": dict(ggl.LOOP_CASES["loop_wide_n400"], sense_radius=2.5, ticks=TICKS, kill_ticks=[]),
}


def ref_loop_life(mod, inp, boot, death, sensed, heard, trace=None, restart=None, task_seed=None):
    """ref_loop with windows.  trace(t, agents, alive): called after every tick.  task_seed: the board case."""
    n = len(inp["ids"])
    ids = inp["ids"]
    wide = int(ids.max()) > 255
    mod.struct = gg._FsmWide(struct) if wide else struct
    clock, cur, now_t = [0.0], [0, 0], [0]
    seed, dt = int(inp["seed"]), float(inp["dt"])
    mod.time = types.SimpleNamespace(time=lambda: clock[0], sleep=gg._noop)
    mod.random = types.SimpleNamespace(uniform=lambda a, b: a + (b - a) * gg.jitter_u(seed, cur[0], cur[1]))
    out_prev = [[] for _ in range(n)]
    out_cur = [[] for _ in range(n)]
    box = {"cur": out_cur}
    ticks = int(inp["ticks"])
    tcounts = np.zeros((ticks, 3), np.int64)
    L, W = mod.AgentState.LEADER, mod.AgentState.ELECTION_WAIT
    booted = np.zeros(n, bool)
    stat = dict(claims_by_booted=0)
    caps, names, trng = np.zeros(n, np.uint32), ggt.CAP_NAMES, None
    if task_seed is not None:
        trng = np.random.default_rng(task_seed)
        for b in range(len(names)):
            caps |= (trng.uniform(size=n) < 0.5).astype(np.uint32) << np.uint32(b)

    def make(i):
        if task_seed is None:
            return mod.SwarmAgent(int(ids[i]), n)
        return mod.SwarmAgent(int(ids[i]), n, capabilities=[c for b, c in enumerate(names) if caps[i] >> b & 1])

    def wire(a, i):
        def send(mt, payload=b"", a=a, i=i):  # the payload as packed at send time
            box["cur"][i].append(a._pack_header(mt) + payload)
            if mt == 4:
                tcounts[now_t[0] - 1, 0] += 1
                stat["claims_by_booted"] += bool(booted[i])
            if mt == 5:
                tcounts[now_t[0] - 1, 2] += 1
        a._send_msg = send
        a.max_speed = float(inp["max_speed"])

        def claim(sender, payload, a=a, real=a._handle_task_claim):  # an observer: it decides nothing
            if a.state == L:
                tcounts[now_t[0] - 1, 1] += 1
            real(sender, payload)
        a._handle_task_claim = claim

    def hand_out(a, board):
        a.tasks = {}
        for k in range(len(board["task_x"])):
            a.tasks[k] = {"status": "OPEN", "pos": (float(board["task_x"][k]), float(board["task_y"][k]))}
            if board["task_req"][k] >= 0:
                a.tasks[k]["required_cap"] = names[board["task_req"][k]]
    agents = [make(i) for i in range(n)]
    for i, a in enumerate(agents):
        a.position = [float(inp["x"][i]), float(inp["y"][i])]
        a.last_heartbeat_time = float(inp["last_hb0"][i])
        if inp["has_t"][i]:
            a.set_target(float(inp["tx"][i]), float(inp["ty"][i]))
        wire(a, i)
    tick_off = np.array(inp["tick_off"], np.int64)
    obstacles = [tuple(float(v) for v in o) for o in inp["obs"]]
    live = boot < death
    alive = ~((boot > 0) | (death <= 0))  # the set-time rule at tick 0
    if restart is not None:
        alive |= restart
    kills = set(int(k) for k in inp["kill_ticks"])
    counts = np.zeros((ticks, 4), np.int64)
    events = np.zeros((ticks, 2), np.int64)
    board = None
    last_two = [None, None]
    for t in range(1, ticks + 1):
        now_t[0] = t
        if t in kills:
            clock[0] = t * dt
            for i, a in enumerate(agents):
                if alive[i] and a.state == L:
                    alive[i] = False
        if task_seed is not None and t == ggt.TASK_TICK:
            px = np.array([a.position[0] for a in agents])
            py = np.array([a.position[1] for a in agents])
            tx = trng.uniform(px.min(), px.max(), ggt.N_TASKS)
            ty = trng.uniform(py.min(), py.max(), ggt.N_TASKS)
            req = trng.integers(-1, len(names), ggt.N_TASKS).astype(np.int8)
            board = dict(task_x=tx, task_y=ty, task_req=req)
            for a in agents:
                hand_out(a, board)
        for i in np.flatnonzero(live & (death == t)):
            alive[i] = False
            events[t - 1, 1] += 1
        clock[0] = (t - 1) * dt  # a booted agent is constructed at the clock of the tick before
        for i in np.flatnonzero(live & (boot == t)):
            old = agents[i]
            a = make(i)
            a.position = [old.position[0], old.position[1]]
            wire(a, i)
            if board is not None:
                hand_out(a, board)
            agents[i] = a
            out_prev[i] = []
            tick_off[i] = 1 - t
            alive[i] = True
            booted[i] = True
            events[t - 1, 0] += 1
        clock[0] = t * dt
        hears = heard([(a.position[0], a.position[1]) for a in agents])
        for i, a in enumerate(agents):
            if not alive[i]:
                continue
            a.tick = t + int(tick_off[i])
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
            a.tick = t + int(tick_off[i])
            a._process_logic()
        snap = [(a.position[0], a.position[1]) for a in agents]
        rows = sensed(snap)
        for i, a in enumerate(agents):
            if alive[i]:
                a.update_sensors(obstacles, [(int(ids[j]), snap[j][0], snap[j][1]) for j in rows[i]])
        for i, a in enumerate(agents):
            if alive[i]:
                a._update_physics(dt)
        for i, a in enumerate(agents):
            types_sent = {pk[0] for pk in out_cur[i]}
            counts[t - 1, 2] += 2 in types_sent
            counts[t - 1, 3] += 1 in types_sent
            if alive[i]:
                counts[t - 1, 0] += a.state == L
                counts[t - 1, 1] += a.state == W
        if trace:
            trace(t, agents, alive)
        last_two = [last_two[1], out_cur]
        out_prev, out_cur = out_cur, [[] for _ in range(n)]
        box["cur"] = out_cur
    mod.struct, mod.time, mod.random = struct, time, __import__("random")
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
        tick_off_out=tick_off.astype(np.int32), counts=counts, agent_events=events)
    if board is not None:
        T = ggt.N_TASKS
        hdr = 9 if wide else 6
        conf_fmt = "!II" if wide else "!IB"
        claim_out, conflict_out = np.zeros((2, n), np.uint64), np.zeros((2, n), np.uint64)
        for tk, sent in ((ticks - 1, last_two[0]), (ticks, last_two[1])):
            for i in range(n):
                for pk in sent[i]:
                    if pk[0] == 4:
                        claim_out[tk & 1, i] |= np.uint64(1) << np.uint64(struct.unpack("!If", pk[hdr:])[0])
                    if pk[0] == 5:
                        conflict_out[tk & 1, i] |= np.uint64(1) << np.uint64(struct.unpack(conf_fmt, pk[hdr:])[0])
        tabw, tabu = np.full((n, T), -1, np.int32), np.zeros((n, T), np.float32)
        for i, a in enumerate(agents):
            for k, c in a.task_claims.items():
                tabw[i, k], tabu[i, k] = c["winner"], c["utility"]
                assert float(tabu[i, k]) == c["utility"]
        out.update(caps=caps, task_tick=np.int64(ggt.TASK_TICK), task_counts=tcounts, claim_out=claim_out,
                   conflict_out=conflict_out, tab_winner_out=tabw, tab_util_out=tabu,
                   status_out=np.array([[gg.STATUS_CODE[a.tasks[k]["status"]] for k in range(T)] for a in agents],
                                       np.uint8), **board)
    out["_stat"] = stat
    return out


def draw_windows(mod, inp, sensed, heard, seed, task_seed=None):
    """The windows of a fixture, from a first run without any: two standing leaders die at ticks 50 and 51 (the
    second on the tick a late agent boots), the twelve highest IDs start late (they time out and take over before
    the end), random late starters and deaths, a boot at tick 1 and at the last tick.  Board case: five agents that
    hold an ASSIGNED task at tick 70 of a run with these windows restart at tick 71."""
    n, ticks = len(inp["ids"]), int(inp["ticks"])
    L = mod.AgentState.LEADER
    leaders = {}

    def trace(t, agents, alive):
        if t == 49:
            leaders["at49"] = [i for i, a in enumerate(agents) if alive[i] and a.state == L]
    none = np.zeros(n, np.int64), np.full(n, FOREVER)
    ref_loop_life(mod, dict(inp, ticks=np.int64(49)), *none, sensed, heard, trace, task_seed=task_seed)
    rng = np.random.default_rng(seed)
    boot, death = np.zeros(n, np.int64), np.full(n, FOREVER)
    by_id = np.argsort(inp["ids"])
    high = [int(i) for i in by_id[-12:]]
    lead = [i for i in leaders["at49"] if i not in high][:2]
    assert len(lead) == 2, "the case has fewer than two leaders at tick 49"
    rest = np.array([i for i in rng.permutation(n) if i not in high and i not in lead])
    k = n // 10
    boot[rest[:k]] = rng.integers(2, ticks, k)
    death[rest[k:2 * k]] = rng.integers(2, ticks, k)
    boot[high] = [20, 30, 40, 51] * 3
    death[lead[0]], death[lead[1]] = 50, 51
    boot[rest[0]], boot[rest[1]] = 1, ticks
    death[rest[k]] = int(boot[rest[2]])  # a death and a boot of different agents on one tick
    restart = np.zeros(n, bool)
    if task_seed is not None:
        held = {}

        def trace70(t, agents, alive):
            if t == 70:
                held["at70"] = [i for i, a in enumerate(agents) if alive[i] and boot[i] == 0 and death[i] == FOREVER
                                and any(v["status"] == "ASSIGNED" for v in a.tasks.values())]
        ref_loop_life(mod, dict(inp, ticks=np.int64(70)), boot, death, sensed, heard, trace70, task_seed=task_seed)
        again = held["at70"][:5]
        assert len(again) == 5, "fewer than five free agents hold an ASSIGNED task at tick 70"
        boot[again] = 71
        restart[again] = True
    return boot, death, lead, high, restart


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    mod = gg.load_reference()
    for name, c in CASES.items():
        if args.only is not None and name not in args.only:
            continue
        t0 = time.time()
        task_seed = c.get("task_seed")
        inp = ggl.make_loop_inputs(c)
        inp["sense_radius"] = np.float64(c["sense_radius"])
        inp["radio_radius"] = np.float64(RADIO_RADIUS)
        sensed, heard = ggs.sensed_rows(float(c["sense_radius"])), ggs.sensed_rows(RADIO_RADIUS)
        boot, death, lead, high, restart = draw_windows(mod, inp, sensed, heard, c["seed"] + 17, task_seed)
        hist = {}

        def trace(t, agents, alive):
            hist[t] = (np.array([a.state.value for a in agents]), alive.copy(),
                       np.array([-1 if a.leader_id is None else a.leader_id for a in agents]),
                       [any(v["status"] == "ASSIGNED" for v in a.tasks.values()) for a in agents]
                       if task_seed is not None and t >= ggt.TASK_TICK else None)
        out = ref_loop_life(mod, inp, boot, death, sensed, heard, trace, restart=restart, task_seed=task_seed)
        stat = out.pop("_stat")
        ids, ticks = inp["ids"], int(inp["ticks"])
        st, al = out["state_out"], out["alive_out"].astype(bool)
        late = (boot > 0) & (death > ticks)
        # what every fixture must contain, in the reference's run alone
        took_over = [i for i in np.flatnonzero(late & al & (st == 3))
                     if any((hist[t][0][j] == 3) and hist[t][1][j] and ids[j] < ids[i] and hist[t + 1][2][j] == ids[i]
                            and hist[t + 1][1][j] for t in range(int(boot[i]), ticks) for j in range(len(ids)))]
        assert took_over, "no booted agent ends LEADER after taking over from a living lower leader"
        assert (late & al & (st == 1) & (out["has_lpos_out"] == 1)).any(), "no booted FOLLOWER with a leader position"
        dying = np.flatnonzero((death <= ticks) & (boot < death))
        assert any(hist[int(death[i]) - 1][0][i] != 3 and hist[int(death[i]) - 1][1][i] for i in dying if death[i] > 1), \
            "no non-leader death"
        for i in lead:
            assert hist[int(death[i]) - 1][0][i] == 3 and hist[int(death[i]) - 1][1][i], "a picked leader was none"
        orphans = [j for i in lead for j in np.flatnonzero(hist[int(death[i])][2] == ids[i])]
        assert any(hist[t][0][j] == 2 for j in orphans for t in range(52, ticks + 1)), \
            "no timeout re-election after a leader's death"
        ev = out["agent_events"]
        assert ev[0, 0] >= 1 and ev[-1, 0] >= 1 and ((ev[:, 0] >= 1) & (ev[:, 1] >= 1)).any()
        if task_seed is not None:
            again = np.flatnonzero(restart)
            assert all(hist[70][3][i] and hist[70][1][i] for i in again), "a restarting agent held no ASSIGNED task"
            assert stat["claims_by_booted"] >= 1, "no booted agent claims a task"
            assert out["task_counts"][:, 1].sum() >= 20 and (out["status_out"] == 3).any()
        arrays = dict(inp)
        arrays.update(out)
        arrays.update(boot=boot, death=death, restart=restart.astype(np.uint8))
        path = os.path.join(gg.OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20)
        print(name, "booted", int(ev[:, 0].sum()), "died", int(ev[:, 1].sum()), "took over", len(took_over),
              "leaders at the end", int(out["counts"][-1, 0]), "dead", int((~al).sum()),
              "claims by booted agents", stat["claims_by_booted"], "bytes", os.path.getsize(path),
              "%.1fs" % (time.time() - t0))


if __name__ == "__main__":
    main()
