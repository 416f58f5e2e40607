#!/usr/bin/env python3
"""Generate tests/golden/loop_lossy_*.npz by driving REAL reference agents through the task update loop over a
lossy channel (build container only; the helpers are tools/gen_golden.py's, tools/gen_golden_loop.py's and
tools/gen_golden_loop_sensed.py's, none of them changed, and the loop below is a loop of its own, so the
existing fixtures stay byte-identical).

Contract U1-L: tools/gen_golden_loop_tasks.py's lock-step loop with one line added to the
delivery -- `if dropped(loss_seed, t, sender ID, receiver ID, loss): continue` inside `for j in hears[i]`, so a
dropped link delivers none of the packets j sent during tick t-1.  The draw u() is restated here on Python
integers (csrc/link_loss.h is the definition; tests/loop_lossy_model.py restates it in numpy).
Only data is written: loop_tasks_*'s keys plus loss, loss_seed and link_counts (ticks x 2: per tick the ordered
pairs of an alive receiver and an in-range sender whose tick t-1 packets include an ACCLAIM or a HEARTBEAT,
and how many of those pairs were dropped).  tests/golden/index.json is not touched.

The tool asserts what each fixture must exercise (see CONDITIONS) and prints the figures.  Seeds are tried in
order from the case's first_seed until all hold; the seeds tried are printed, and recorded in DESIGN.md 4k.

Usage:  python tools/gen_golden_loop_lossy.py [--only NAME ...] [--tries N]
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
from gen_golden_loop_tasks import CAP_NAMES, N_TASKS, RADIO_RADIUS, TASK_TICK, guard_flag  # noqa: E402

LOSSY_CASES = {
    # loop_n200's inputs (u8 IDs), the kill at tick 90
    "loop_lossy_n200": dict(ggl.LOOP_CASES["loop_n200"], ticks=120, sense_radius=2.5, task_seed=9113, loss=0.3,
                            first_seed=1, need="all"),
    # IDs > 255: the wide codec path, the kill at tick 70
    "loop_lossy_wide_n400": dict(ggl.LOOP_CASES["loop_wide_n400"], ticks=120, sense_radius=2.5, task_seed=9113,
                                 loss=0.1, first_seed=1, need="all"),
    # nothing is ever delivered: every agent elects itself, every claim stays TENTATIVE
    "loop_lossy_p1_n200": dict(ggl.LOOP_CASES["loop_n200"], ticks=60, sense_radius=2.5, task_seed=9113, loss=1.0,
                               first_seed=1, need="p1"),
}
CONDITIONS = {
    "all": "a follower that times out and re-elects while in range of an alive leader >= 1; a tick with two "
           "alive LEADERs in range of each other >= 1; a claim in range of a LEADER that the LEADER does not "
           "handle because the link was dropped >= 1; a conflict dropped at its claimer but heard by a "
           "bystander >= 1; all four statuses at the end; no evaluated pair inside the guard band",
    "p1": "every link dropped; no claim handled, no conflict sent; statuses OPEN and TENTATIVE only; every alive "
          "agent LEADER of itself at the end; no evaluated pair inside the guard band",
}
M64 = (1 << 64) - 1


def _fin(x):
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def link_u(seed, t, sid, rid):
    """csrc/link_loss.h link_u on Python integers."""
    a = _fin((seed ^ ((sid & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) ^ (t * 0xD1B54A32D192ED03)) & M64)
    b = _fin((a ^ ((rid & 0xFFFFFFFF) * 0x9E3779B97F4A7C15)) & M64)
    return float(b >> 11) * 2.0 ** -53


def dropped(seed, t, sid, rid, loss):
    return link_u(seed, t, sid, rid) < loss


def ref_loop_lossy(mod, inp, task_seed, loss, loss_seed):
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
    stat = dict(handled=0, sent=0, min_gap=math.inf, guard=0, reelect_in_range=0, two_leaders=0, claim_lost=0,
                conflict_split=0, links=0, dropped=0)
    L, W, FOL = mod.AgentState.LEADER, mod.AgentState.ELECTION_WAIT, mod.AgentState.FOLLOWER
    tcounts = np.zeros((ticks, 3), np.int64)
    lcounts = np.zeros((ticks, 2), np.int64)
    now_t = [0]
    hdr = 9 if wide else 6
    conf_fmt = "!II" if wide else "!IB"
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

        def claim(sender, payload, a=a, real=a._handle_task_claim):  # an observer: it decides nothing
            if a.state == L:
                tcounts[now_t[0] - 1, 1] += 1
                stat["handled"] += 1
            real(sender, payload)
        a._handle_task_claim = claim

        def util(task, a=a, real=a._calculate_utility):
            u = real(task)
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
                    if req[k] >= 0:
                        a.tasks[k]["required_cap"] = CAP_NAMES[req[k]]
        hears = heard([(a.position[0], a.position[1]) for a in agents])
        lead0 = [alive[i] and a.state == L for i, a in enumerate(agents)]
        stat["two_leaders"] += any(lead0[i] and any(lead0[j] for j in hears[i]) for i in range(n))
        fol0 = [a.state == FOL for a in agents]
        # a conflict dropped at the agent it names, kept at someone else in range of its sender
        for j in range(n):
            for pk in out_prev[j]:
                if pk[0] == 5:
                    w = mod.struct.unpack(conf_fmt, pk[hdr:])[1]
                    rx = [i for i in range(n) if alive[i] and j in hears[i]]
                    lost_at_winner = any(int(ids[i]) == w and dropped(loss_seed, t, int(ids[j]), w, loss) for i in rx)
                    kept_elsewhere = any(int(ids[i]) != w and not dropped(loss_seed, t, int(ids[j]), int(ids[i]), loss)
                                         for i in rx)
                    stat["conflict_split"] += lost_at_winner and kept_elsewhere
        for i, a in enumerate(agents):
            if not alive[i]:
                continue
            a.tick = t + int(inp["tick_off"][i])
            for j in hears[i]:
                election = any(pk[0] in (1, 2, 3) for pk in out_prev[j])
                lcounts[t - 1, 0] += election
                if dropped(loss_seed, t, int(ids[j]), int(ids[i]), loss):
                    lcounts[t - 1, 1] += election
                    stat["claim_lost"] += a.state == L and any(pk[0] == 4 for pk in out_prev[j])
                    continue
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
            was_follower = a.state == FOL and fol0[i]
            a._process_logic()
            if was_follower and a.state != FOL:  # timed out, although a leader it could hear was alive
                stat["reelect_in_range"] += any(lead0[j] for j in hears[i])
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
        last_two = [last_two[1], out_cur]
        out_prev, out_cur = out_cur, [[] for _ in range(n)]
    claim_out = np.zeros((2, n), np.uint64)
    conflict_out = np.zeros((2, n), np.uint64)
    for tk, sent in ((ticks - 1, last_two[0]), (ticks, last_two[1])):
        for i in range(n):
            for pk in sent[i]:
                if pk[0] == 4:
                    claim_out[tk & 1, i] |= np.uint64(1) << np.uint64(struct.unpack("!If", pk[hdr:])[0])
                if pk[0] == 5:
                    conflict_out[tk & 1, i] |= np.uint64(1) << np.uint64(struct.unpack(conf_fmt, pk[hdr:])[0])
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
    stat["links"], stat["dropped"] = int(lcounts[:, 0].sum()), int(lcounts[:, 1].sum())
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
        tab_util_out=tabu, claim_out=claim_out, conflict_out=conflict_out, task_counts=tcounts,
        link_counts=lcounts, loss=np.float64(loss), loss_seed=np.uint64(loss_seed), **board)
    return out, stat


def conditions_met(need, out, s):
    present = sorted(set(out["status_out"].ravel().tolist()))
    if need == "p1":
        al = out["alive_out"] != 0
        return (s["links"] == s["dropped"] > 0 and s["handled"] == 0 and int(out["task_counts"][:, 2].sum()) == 0 and
                present == [0, 1] and s["guard"] == 0 and (out["state_out"][al] == 3).all() and
                (out["leader_out"][al] == out["ids"][al]).all())
    return (s["reelect_in_range"] >= 1 and s["two_leaders"] >= 1 and s["claim_lost"] >= 1 and
            s["conflict_split"] >= 1 and present == [0, 1, 2, 3] and s["guard"] == 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--tries", type=int, default=20, help="loss seeds tried per case, from its first_seed")
    args = ap.parse_args()
    mod = gg.load_reference()
    for name, c in LOSSY_CASES.items():
        if args.only is not None and name not in args.only:
            continue
        inp = ggl.make_loop_inputs(c)
        inp["sense_radius"] = np.float64(c["sense_radius"])
        inp["radio_radius"] = np.float64(RADIO_RADIUS)
        for loss_seed in range(c["first_seed"], c["first_seed"] + args.tries):
            t0 = time.time()
            out, s = ref_loop_lossy(mod, inp, c["task_seed"], c["loss"], loss_seed)
            out["ids"] = inp["ids"]
            ok = conditions_met(c["need"], out, s)
            print(name, "loss_seed", loss_seed, "statuses", sorted(set(out["status_out"].ravel().tolist())),
                  "links", s["links"], "dropped", s["dropped"], "re-elections in range of a leader",
                  s["reelect_in_range"], "ticks with two leaders in range", s["two_leaders"],
                  "claims lost at a leader", s["claim_lost"], "conflicts lost at the winner, kept elsewhere",
                  s["conflict_split"], "claims sent", s["sent"], "handled", s["handled"], "conflicts sent",
                  int(out["task_counts"][:, 2].sum()), "smallest |U - 20| %.2g" % s["min_gap"], "guard", s["guard"],
                  "met" if ok else "MISSED", "%.1fs" % (time.time() - t0), flush=True)
            if ok:
                break
        assert ok, CONDITIONS[c["need"]]
        arrays = dict(inp)
        arrays.update(out)
        np.savez_compressed(os.path.join(gg.OUT, name + ".npz"), **arrays)


if __name__ == "__main__":
    main()
