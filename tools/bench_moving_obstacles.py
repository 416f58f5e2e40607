#!/usr/bin/env python3
"""Measure update_loop_radio over moving obstacles (contract O2) on tools/bench_obstacle_field.py's
setup: the C3 swarm, 30 % of the agents with a target, Rc = Rs = 1.0.  bench.py is not involved.

For every m of --m (obstacles uniform over the arena, r in U(0.2, 2), fixed seed), --ticks ticks per run, four legs:
  s  the static field of the list (contract O1: built once on the host);
  z  a moving field with zero velocities: the device builder runs every tick, nothing moves -- must end on s's
     position and leader checksums; z - s is the builder's cost;
  v  a moving field with speeds in U(0, --speed), directions uniform;
  p  what a caller had to do before moving fields: per tick update_loop_radio(1, obstacles=obstacle_field(list_t))
     from Python, the list advanced on the host by the contract's arithmetic -- must end on v's checksums.
ms per tick, wall clock ended on a synchronise; per leg one warm-up run, then --reps timed runs, the legs taking
turns run by run.  Results are merged into --out under --label.

Usage:  python tools/bench_moving_obstacles.py [--agents N] [--m 1024,16384,1000000] [--legs s,z,v,p] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=10_000_000)
    ap.add_argument("--deg", type=float, default=16.0)
    ap.add_argument("--m", default="1024,16384,1000000")
    ap.add_argument("--speed", type=float, default=5.0)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--radio-radius", type=float, default=1.0)
    ap.add_argument("--sense-radius", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="s,z,v,p")
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "distributed-swarm-algorithm_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_moving_obstacles", "moving_obstacles.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    from swarm_amd import _lib, gen
    from swarm_amd.swarm import Swarm

    dev = torch.device("cuda", 0)
    d = gen.swarm_inputs(a.agents, a.seed, deg=a.deg, t=1)
    sw = Swarm(d["ids"], d["x"], d["y"], d["caps"], device=dev)
    n, rc, rs, ticks, dt = sw.n, a.radio_radius, a.sense_radius, a.ticks, 0.1
    g = np.random.default_rng(a.seed + 3)
    side = float(sw.pos[:, 0].max())
    off = (np.arange(n, dtype=np.int64) * 7919 % 40).astype(np.int32)
    has_t = torch.as_tensor(g.uniform(size=n) < 0.3, device=dev)
    tgt = torch.as_tensor(g.uniform(0, side, (n, 2)), device=dev)
    pos0 = sw.pos.clone()
    legs = [k for k in ("s", "z", "v", "p") if k in a.legs.split(",")]
    print(f"[bench_moving_obstacles] {a.label}: n={n} side={side:.1f} Rc={rc} Rs={rs} m={a.m} legs={legs}",
          file=sys.stderr, flush=True)

    def reset():
        """The same start for every run: positions, FSM, velocity, 30 % of the agents with a target."""
        sw.pos.copy_(pos0)
        sw.protocol_reset(tick_off=off, last_hb=-(off * 0.1))
        sw.vel = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        sw.target = torch.where(has_t[:, None], tgt, torch.zeros_like(tgt)).contiguous()
        sw.has_target = has_t.to(torch.uint8).contiguous()
        torch.cuda.synchronize()

    res = {"agents": n, "arena_side": side, "radio_radius": rc, "sense_radius": rs, "ticks": ticks,
           "libswarm": _lib.version(),
           "unit": "ms per tick, wall clock ended on a synchronise, after one warm-up run of the leg; the legs of "
                   "an m take turns run by run", "m": {}}
    for m in [int(v) for v in a.m.split(",") if v]:
        q = np.random.default_rng(a.seed + 11 + m)
        obs = np.stack([q.uniform(0, side, m), q.uniform(0, side, m), q.uniform(0.2, 2.0, m)], 1)
        ang, spd = q.uniform(0, 2 * np.pi, m), q.uniform(0, a.speed, m)
        vel = np.stack([spd * np.cos(ang), spd * np.sin(ang)], 1)
        step = vel * np.float64(dt)
        times = {k: [] for k in legs}
        sums, leaders, sing, info = {}, {}, {}, {}
        for rep in range(a.reps + 1):  # the first round is the warm-up
            for k in legs:
                reset()
                field = None
                if k == "s":
                    field = sw.obstacle_field(obs)
                elif k in "zv":
                    field = sw.obstacle_field(obs, np.zeros((m, 2)) if k == "z" else vel)
                if field is not None:
                    info[k] = {x: field.info[x] for x in ("live", "ncx", "ncy", "cell", "pairs", "longest")}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if k == "p":
                    cur, s_total = obs.copy(), 0
                    for _ in range(ticks):
                        f = sw.obstacle_field(cur)
                        s_total += sw.update_loop_radio(1, rc, rs, obstacles=f, seed=5, dt=dt)["singular"]
                        f.close()
                        cur[:, :2] = cur[:, :2] + step
                    r = {"singular": s_total}
                else:
                    r = sw.update_loop_radio(ticks, rc, rs, obstacles=field, seed=5, dt=dt)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / ticks
                print(f"[bench_moving_obstacles] m={m} {k} {'warm-up' if rep == 0 else rep}: {ms:.4f} ms per tick",
                      file=sys.stderr, flush=True)
                if rep:
                    times[k].append(ms)
                sums[k] = [float(sw.pos[:, 0].sum()), float(sw.pos[:, 1].sum())]
                leaders[k] = int(sw.leader.to(torch.int64).sum())
                sing[k] = int(r["singular"])
                if field is not None:
                    field.close()
        for x, y in (("s", "z"), ("v", "p")):
            if x in legs and y in legs:
                assert sums[x] == sums[y] and leaders[x] == leaders[y] and sing[x] == sing[y], \
                    (f"legs {x} and {y} ended differently", m, sums, leaders, sing)
        e = {"field": info, "ms_per_tick": times, "pos_checksum": sums, "leader_checksum": leaders, "singular": sing}
        if "v" in legs and "p" in legs:
            e["v_slowest_below_p_fastest"] = max(times["v"]) < min(times["p"])
        if "z" in legs and "s" in legs:
            e["builder_cost_ms_per_tick_z_minus_s_medians"] = float(np.median(times["z"]) - np.median(times["s"]))
        res["m"][str(m)] = e
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out[a.label] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({a.label: res}))


if __name__ == "__main__":
    main()
