#!/usr/bin/env python3
"""Generate tests/golden/loop_*.npz by driving REAL reference agents through the coupled update loop
(build container only; the helpers are tools/gen_golden.py's, whose case tables are left alone).

Contract U1: tools/gen_golden.py ref_fsm's lock-step loop -- clock t * dt, kills, every alive
agent receives what its CSR neighbours sent during the previous tick (packets framed by _pack_header, the
'!ff' heartbeat payload packed when it was sent), then _process_logic -- with SwarmAgent.set_target at the
start and, after the tick's logic, the tick's physics: a snapshot of all positions, update_sensors(obstacles,
the agent's CSR row in CSR order from the snapshot, dead agents included) and _update_physics(dt) for every
alive agent.  Only data is written: the inputs, every final per-agent array and the per-tick counts, with
the case's parameters inside the file.  tests/golden/index.json is not touched.

Usage:  python tools/gen_golden_loop.py [--only NAME ...]
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

LOOP_CASES = {
    # u8 IDs, two kills
    "loop_n200": dict(n=200, side=15.0, ticks=260, kill_ticks=(90, 180), seed=71),
    # u8 IDs, one kill
    "loop_n250": dict(n=250, side=17.0, ticks=220, kill_ticks=(100,), seed=72),
    # IDs > 255: the wide codec path
    "loop_wide_n400": dict(n=400, side=21.5, ticks=200, kill_ticks=(70, 140), seed=73, id_scale=5),
}
RADIUS, DT, MAX_SPEED, N_OBS = 2.5, 0.1, 5.0, 6


def make_loop_inputs(c):
    n, side, rng = c["n"], c["side"], np.random.default_rng(c["seed"])
    x = rng.uniform(10.0, 10.0 + side, n)
    y = rng.uniform(10.0, 10.0 + side, n)
    sc = c.get("id_scale", 1)
    ids = (rng.permutation(n) * sc + rng.integers(0, sc, n)).astype(np.int32)
    row_ptr, col = gg.gen.rgg_csr(x, y, RADIUS)
    off = rng.integers(0, 40, n).astype(np.int32)
    has_t = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    tx = np.where(has_t, rng.uniform(0.0, 3.0 * side, n), 0.0)
    ty = np.where(has_t, rng.uniform(0.0, 3.0 * side, n), 0.0)
    obs = np.stack([rng.uniform(10.0, 10.0 + side, N_OBS), rng.uniform(10.0, 10.0 + side, N_OBS),
                    rng.uniform(0.2, 1.0, N_OBS)], 1)
    return dict(ids=ids, x=x, y=y, row_ptr=np.asarray(row_ptr, np.int64), col=np.asarray(col, np.int32),
                tick_off=off, last_hb0=-(off * DT), tx=tx, ty=ty, has_t=has_t, obs=obs,
                ticks=np.int64(c["ticks"]), kill_ticks=np.asarray(c["kill_ticks"], np.int64),
                seed=np.uint64(c["seed"] * 7919), dt=np.float64(DT), max_speed=np.float64(MAX_SPEED),
                radius=np.float64(RADIUS))


def ref_loop(mod, inp, sensed=None, heard=None):
    """sensed: None -- every tick's sensors are the agent's CSR row (U1); or a function of the tick's
    snapshot returning every agent's sensed indices (U1-S, tools/gen_golden_loop_sensed.py).
    heard: None -- every tick's packets come along the agent's CSR row; or a function of the snapshot at the
    start of the tick (before the receive phase) returning every agent's heard indices in ascending order,
    dead agents included (U1-R, tools/gen_golden_loop_radio.py): the delivery loop iterates those."""
    n = len(inp["ids"])
    ids, rp, col = inp["ids"], inp["row_ptr"], inp["col"]
    wide = int(ids.max()) > 255
    mod.struct = gg._FsmWide(struct) if wide else struct
    clock, cur = [0.0], [0, 0]
    seed, dt = int(inp["seed"]), float(inp["dt"])
    mod.time = types.SimpleNamespace(time=lambda: clock[0], sleep=gg._noop)
    mod.random = types.SimpleNamespace(uniform=lambda a, b: a + (b - a) * gg.jitter_u(seed, cur[0], cur[1]))
    agents = [mod.SwarmAgent(int(ids[i]), n) for i in range(n)]
    out_prev = [[] for _ in range(n)]
    out_cur = [[] for _ in range(n)]
    for i, a in enumerate(agents):
        a.position = [float(inp["x"][i]), float(inp["y"][i])]
        a.last_heartbeat_time = float(inp["last_hb0"][i])
        a.max_speed = float(inp["max_speed"])
        if inp["has_t"][i]:
            a.set_target(float(inp["tx"][i]), float(inp["ty"][i]))

        def send(mt, payload=b"", a=a, i=i):  # the payload as packed at send time
            out_cur[i].append(a._pack_header(mt) + payload)
        a._send_msg = send
    obstacles = [tuple(float(v) for v in o) for o in inp["obs"]]
    alive = np.ones(n, bool)
    kills = set(int(k) for k in inp["kill_ticks"])
    L, W = mod.AgentState.LEADER, mod.AgentState.ELECTION_WAIT
    counts = np.zeros((int(inp["ticks"]), 4), np.int64)
    for t in range(1, int(inp["ticks"]) + 1):
        clock[0] = t * dt
        if t in kills:
            for i, a in enumerate(agents):
                if alive[i] and a.state == L:
                    alive[i] = False
        hears = heard([(a.position[0], a.position[1]) for a in agents]) if heard else None
        for i, a in enumerate(agents):
            if not alive[i]:
                continue
            a.tick = t + int(inp["tick_off"][i])
            for j in (hears[i] if heard else col[rp[i]:rp[i + 1]]):
                for pkt in out_prev[j]:
                    if wide:  # on_message_received slices a 6-byte header: dispatch as it does
                        mt, snd, _ = struct.unpack("!BII", pkt[:9])
                        pl = pkt[9:]
                        {1: lambda: a._handle_heartbeat(snd, pl), 2: lambda: a._handle_election_acclaim(snd),
                         3: lambda: a._handle_coordinator(snd)}[mt]()
                    else:
                        a.on_message_received(pkt)
        for i, a in enumerate(agents):
            if not alive[i]:
                continue
            cur[0], cur[1] = int(ids[i]), t
            a.tick = t + int(inp["tick_off"][i])
            a._process_logic()
        snap = [(a.position[0], a.position[1]) for a in agents]
        rows = sensed(snap) if sensed else None
        for i, a in enumerate(agents):
            if alive[i]:
                a.update_sensors(obstacles, [(int(ids[j]), snap[j][0], snap[j][1])
                                             for j in (rows[i] if sensed else col[rp[i]:rp[i + 1]])])
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
        out_prev, out_cur = out_cur, [[] for _ in range(n)]
    mod.struct, mod.time, mod.random = struct, time, __import__("random")
    return dict(
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
        counts=counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    mod = gg.load_reference()
    for name, c in LOOP_CASES.items():
        if args.only is not None and name not in args.only:
            continue
        t0 = time.time()
        inp = make_loop_inputs(c)
        out = ref_loop(mod, inp)
        arrays = dict(inp)
        arrays.update(out)
        np.savez_compressed(os.path.join(gg.OUT, name + ".npz"), **arrays)
        fol = (out["state_out"] == 1) & (out["has_lpos_out"] == 1) & (out["alive_out"] == 1)
        moved = (out["x_out"] != inp["x"]) | (out["y_out"] != inp["y"])
        print(name, "degree %.1f" % (len(inp["col"]) / c["n"]), "followers with leader_pos", int(fol.sum()),
              "dead", int((out["alive_out"] == 0).sum()), "moved", int(moved.sum()),
              "leaders per 20 ticks", out["counts"][::20, 0].tolist(), "%.1fs" % (time.time() - t0))


if __name__ == "__main__":
    main()
